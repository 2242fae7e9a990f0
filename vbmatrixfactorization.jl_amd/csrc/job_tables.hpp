// job_tables.hpp -- the bookkeeping of a call over (bag, model) jobs: what vbmf_sparse_fixed_basis_jobs, vbmf_sparse_scored_jobs,
// vbmf_fixed_basis_jobs and (for the refusals its texts share) vbmf_bag_least_squares_jobs do on the host before the first launch.
// Plain C++17, no HIP and no vbmf_ctx: the host compiler alone builds it (tests/job_tables_check.cpp drives it under sanitizers).
//   JobRefusal        a refusal as (kind, text); the caller turns the kind into its error code and passes the text to FAIL
//   job_*_check       the refusals every entry words alike.  Three calls and not one: each entry refuses its own scalars and null
//                     pointers between them, and the first refusal a call meets stays the one it was
//   job_walk          the models' ranks, the jobs' ranges, the five sums every layout needs, and a hook per job for what is one entry's
//   JobTable          the int64 prefix of the upload, [col_off nb + 1 | job_bag | job_model | job_off | job_sa | job_h | idx (nj each) |
//                     model_H | b_off | k_off | h_off (nk each)], which the kernels read through VjobsModels, VjobsArgs and FjobsArgs;
//                     job_table_fill writes it and sorts the jobs into idx by group (the groups in order, a group's jobs in job order)
//   first_nonfinite   the first non-finite entry of a per-model packed array, as (model, entry within the model)
#pragma once

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>

namespace vbmf {

enum { JOBS_OK = 0, JOBS_INVALID = 1, JOBS_UNSUPPORTED = 2 };

struct JobRefusal {
    int kind = JOBS_OK;
    char msg[384] = "";
    int set(int k, const char* fmt, ...) __attribute__((format(printf, 3, 4))) {
        va_list ap;
        va_start(ap, fmt); vsnprintf(msg, sizeof msg, fmt, ap); va_end(ap);
        return kind = k;
    }
};

// The arguments that say what a call's jobs are.  model_H nullptr: every model has rank H_all.  col_off is only read once the caller
// has checked it (bags_check), and only for bags in range.
struct JobShape {
    int64_t nbags; const int64_t* col_off;
    int64_t nmodels; const int64_t* model_H; int64_t H_all;
    int64_t njobs; const int64_t* job_bag; const int64_t* job_model;
    int64_t H(int64_t k) const { return model_H ? model_H[k] : H_all; }
    int64_t width(int64_t b) const { return col_off[b + 1] - col_off[b]; }
};

// sum H_k, sum H_k^2 over the models; sum M_b H_k, sum H_k, sum H_k^2 over the jobs
struct JobSums { int64_t sumH = 0, sumH2 = 0, SMH = 0, SJH = 0, SJH2 = 0; };

// nmodels: the argument's name in the texts ("nmodels", "nbasis")
inline int job_counts_check(const char* fn, int64_t nmodels, int64_t njobs, const char* nmodels_name, JobRefusal& r) {
    if (nmodels < 1) return r.set(JOBS_INVALID, "%s: %s must be >= 1", fn, nmodels_name);
    if (njobs < 1) return r.set(JOBS_INVALID, "%s: njobs must be >= 1", fn);
    return JOBS_OK;
}

// what one grid holds: a launch is kept to 2^32 - 1 threads in all, so to grid_cap workgroups
inline int job_grid_check(const char* fn, int64_t nmodels, int64_t njobs, int64_t grid_cap, JobRefusal& r) {
    if (njobs > grid_cap || nmodels > grid_cap)
        return r.set(JOBS_UNSUPPORTED, "%s: %lld jobs, %lld models (more than the %lld workgroups of one grid)", fn, (long long)njobs,
                     (long long)nmodels, (long long)grid_cap);
    return JOBS_OK;
}

// job j's bag and model (or basis: the names go into the texts) against 0..nbags-1 and 0..nmodels-1
inline int job_range_check(const char* fn, int64_t j, int64_t b, int64_t nbags, int64_t k, int64_t nmodels, const char* job_model_name,
                           const char* nmodels_name, JobRefusal& r) {
    if (b < 0 || b >= nbags) return r.set(JOBS_INVALID, "%s: job_bag[%lld] = %lld outside 0..nbags-1", fn, (long long)j, (long long)b);
    if (k < 0 || k >= nmodels)
        return r.set(JOBS_INVALID, "%s: %s[%lld] = %lld outside 0..%s-1", fn, job_model_name, (long long)j, (long long)k, nmodels_name);
    return JOBS_OK;
}

// Every model's rank against 1..H_cap, then every job in order: its ranges, then hook(j, b, k, M_b, H_k, r) -> kind for what the entry
// itself refuses or counts about the job.  The first refusal met in that order comes back; the sums are whole only after JOBS_OK.
template <class Hook>
int job_walk(const char* fn, const JobShape& s, int64_t H_cap, JobSums& t, JobRefusal& r, Hook hook) {
    t = JobSums{};
    for (int64_t k = 0; k < s.nmodels; ++k) {
        const int64_t H = s.H(k);
        if (H < 1 || H > H_cap)
            return r.set(JOBS_UNSUPPORTED, "%s: model_H[%lld] = %lld (built for 1 <= H <= %lld)", fn, (long long)k, (long long)H, (long long)H_cap);
        t.sumH += H;
        t.sumH2 += H * H;
    }
    for (int64_t j = 0; j < s.njobs; ++j) {
        const int64_t b = s.job_bag[j], k = s.job_model[j];
        if (job_range_check(fn, j, b, s.nbags, k, s.nmodels, "job_model", "nmodels", r)) return r.kind;
        const int64_t Mb = s.width(b), H = s.H(k);
        if (hook(j, b, k, Mb, H, r)) return r.kind;
        t.SMH += Mb * H;                                          // (at most 2^24 terms of at most 2^60 / 8: no overflow)
        t.SJH += H;
        t.SJH2 += H * H;
    }
    return JOBS_OK;
}

// word offsets of the blocks of the int64 prefix; words: its length
struct JobTable {
    int64_t bag, mod, off, jsa, jh, idx, mh, bo, ko, ho, words;
    JobTable(int64_t nb, int64_t nk, int64_t nj)
        : bag(nb + 1), mod(bag + nj), off(mod + nj), jsa(off + nj), jh(jsa + nj), idx(jh + nj), mh(idx + nj), bo(mh + nk), ko(bo + nk),
          ho(ko + nk), words(ho + nk) {}
};
inline int64_t job_table_words(int64_t nb, int64_t nk, int64_t nj) { return JobTable(nb, nk, nj).words; }

// Fills ui[0 .. words): the models' offsets into the packed bases (L H_k), SigmaB (H_k^2) and per-column arrays (H_k), the jobs' offsets
// into the M_b H_k-, H_k^2- and H_k-long output blocks, and idx.  group_of(j) in 0..ngroups-1; grp_n[g] jobs of group g stand at
// idx[grp_at[g] ..] in job order.
template <class GroupOf>
void job_table_fill(long long* ui, const JobShape& s, int64_t L, int ngroups, GroupOf group_of, int64_t* grp_n, int64_t* grp_at) {
    const JobTable u(s.nbags, s.nmodels, s.njobs);
    for (int64_t b = 0; b <= s.nbags; ++b) ui[b] = s.col_off[b];
    for (int64_t k = 0, bo = 0, ko = 0, ho = 0; k < s.nmodels; ++k) {
        const int64_t H = s.H(k);
        ui[u.mh + k] = H; ui[u.bo + k] = bo; ui[u.ko + k] = ko; ui[u.ho + k] = ho;
        bo += L * H; ko += H * H; ho += H;
    }
    for (int g = 0; g < ngroups; ++g) grp_n[g] = 0;
    for (int64_t j = 0; j < s.njobs; ++j) ++grp_n[group_of(j)];
    for (int g = 0; g < ngroups; ++g) grp_at[g] = g ? grp_at[g - 1] + grp_n[g - 1] : 0;
    for (int64_t j = 0, off = 0, sa = 0, jh = 0; j < s.njobs; ++j) {
        const int64_t b = s.job_bag[j], k = s.job_model[j], H = s.H(k);
        ui[u.bag + j] = b; ui[u.mod + j] = k; ui[u.off + j] = off; ui[u.jsa + j] = sa; ui[u.jh + j] = jh;
        ui[u.idx + grp_at[group_of(j)]++] = j;
        off += s.width(b) * H; sa += H * H; jh += H;
    }
    for (int g = 0; g < ngroups; ++g) grp_at[g] -= grp_n[g];
}

// v packs stride(k) entries per model, model after model: the first entry that is not finite, as (model, entry within the model)
template <class Stride>
bool first_nonfinite(const double* v, int64_t nmodels, Stride stride, int64_t& model, int64_t& entry) {
    for (int64_t k = 0; k < nmodels; ++k) {
        const int64_t n = stride(k);
        for (int64_t i = 0; i < n; ++i)
            if (!std::isfinite(v[i])) { model = k; entry = i; return true; }
        v += n;
    }
    return false;
}

}  // namespace vbmf
