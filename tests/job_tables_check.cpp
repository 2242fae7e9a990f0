// Stand-alone check of csrc/job_tables.hpp (built and run by tests/test_job_tables_host.py with the host compiler and its sanitizers).
// The walk's sums and refusals, the table against a second, naive construction (offsets by summing from the start, idx by a stable
// sort), and the (model, entry) naming of a planted NaN for every stride.  Every buffer is a std::vector of exactly the size the header
// says it needs, so a write or read past it is the sanitizers' to find.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <limits>
#include <numeric>
#include <string>
#include <vector>

#include "../vbmatrixfactorization.jl_amd/csrc/job_tables.hpp"

using namespace vbmf;
using I = int64_t;

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { ++failures; std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

struct Case {
    std::vector<I> col_off, model_H, job_bag, job_model, group;     // group[j] in 0..ngroups-1
    int ngroups;
    I L;
    JobShape shape() const {
        return JobShape{(I)col_off.size() - 1, col_off.data(), (I)model_H.size(), model_H.data(), 0, (I)job_bag.size(), job_bag.data(),
                        job_model.data()};
    }
};

static auto no_hook = [](I, I, I, I, I, JobRefusal&) { return (int)JOBS_OK; };

static void check_table(const Case& q) {
    const JobShape s = q.shape();
    const I nb = s.nbags, nk = s.nmodels, nj = s.njobs;
    JobSums t;
    JobRefusal r;
    CHECK(job_walk("f", s, 32, t, r, no_hook) == JOBS_OK && r.kind == JOBS_OK);
    // the sums, term by term
    I sumH = 0, sumH2 = 0, SMH = 0, SJH = 0, SJH2 = 0;
    for (I k = 0; k < nk; ++k) { sumH += q.model_H[k]; sumH2 += q.model_H[k] * q.model_H[k]; }
    for (I j = 0; j < nj; ++j) {
        const I H = q.model_H[q.job_model[j]], w = q.col_off[q.job_bag[j] + 1] - q.col_off[q.job_bag[j]];
        SMH += w * H; SJH += H; SJH2 += H * H;
    }
    CHECK(t.sumH == sumH && t.sumH2 == sumH2 && t.SMH == SMH && t.SJH == SJH && t.SJH2 == SJH2);
    // the naive table: [col_off | job_bag | job_model | job_off | job_sa | job_h | idx | model_H | b_off | k_off | h_off]
    std::vector<long long> want;
    for (I b = 0; b <= nb; ++b) want.push_back(q.col_off[b]);
    for (I j = 0; j < nj; ++j) want.push_back(q.job_bag[j]);
    for (I j = 0; j < nj; ++j) want.push_back(q.job_model[j]);
    for (int p = 0; p < 3; ++p)
        for (I j = 0; j < nj; ++j) {
            long long o = 0;
            for (I i = 0; i < j; ++i) {
                const I H = q.model_H[q.job_model[i]], w = q.col_off[q.job_bag[i] + 1] - q.col_off[q.job_bag[i]];
                o += p == 0 ? w * H : p == 1 ? H * H : H;
            }
            want.push_back(o);
        }
    std::vector<I> order((size_t)nj);
    std::iota(order.begin(), order.end(), (I)0);
    std::stable_sort(order.begin(), order.end(), [&](I x, I y) { return q.group[x] < q.group[y]; });
    for (I j = 0; j < nj; ++j) want.push_back(order[j]);
    for (I k = 0; k < nk; ++k) want.push_back(q.model_H[k]);
    for (int p = 0; p < 3; ++p)
        for (I k = 0; k < nk; ++k) {
            long long o = 0;
            for (I i = 0; i < k; ++i) o += p == 0 ? q.L * q.model_H[i] : p == 1 ? q.model_H[i] * q.model_H[i] : q.model_H[i];
            want.push_back(o);
        }
    CHECK((I)want.size() == job_table_words(nb, nk, nj));
    const JobTable u(nb, nk, nj);
    CHECK(u.bag == nb + 1 && u.idx == nb + 1 + 5 * nj && u.mh == u.idx + nj && u.ho == u.mh + 3 * nk && u.words == u.ho + nk);
    std::vector<long long> got((size_t)job_table_words(nb, nk, nj), -7);
    std::vector<I> grp_n((size_t)q.ngroups, -1), grp_at((size_t)q.ngroups, -1);
    job_table_fill(got.data(), s, q.L, q.ngroups, [&](I j) { return (int)q.group[j]; }, grp_n.data(), grp_at.data());
    CHECK(got == want);
    // idx: a permutation, grouped, in job order within a group; grp_at the groups' first slots
    std::vector<int> seen((size_t)nj, 0);
    for (I i = 0; i < nj; ++i) {
        const I j = got[(size_t)(u.idx + i)];
        CHECK(j >= 0 && j < nj);
        if (j >= 0 && j < nj) ++seen[(size_t)j];
    }
    for (I j = 0; j < nj; ++j) CHECK(seen[(size_t)j] == 1);
    I at = 0;
    for (int g = 0; g < q.ngroups; ++g) {
        CHECK(grp_at[(size_t)g] == at);
        CHECK(grp_n[(size_t)g] == std::count(q.group.begin(), q.group.end(), (I)g));
        for (I i = 0; i < grp_n[(size_t)g]; ++i) {
            const I j = got[(size_t)(u.idx + at + i)];
            CHECK(q.group[(size_t)j] == g);
            if (i) CHECK(got[(size_t)(u.idx + at + i - 1)] < j);
        }
        at += grp_n[(size_t)g];
    }
    CHECK(at == nj);
}

static void check_refusals() {
    const Case q{{0, 3, 4}, {5, 17}, {0, 1, 1}, {1, 0, 1}, {0, 0, 0}, 1, 7};
    JobRefusal r;
    CHECK(job_counts_check("f", 1, 1, "nmodels", r) == JOBS_OK && r.kind == JOBS_OK && !r.msg[0]);
    CHECK(job_counts_check("f", 0, 0, "nmodels", r) == JOBS_INVALID && std::string(r.msg) == "f: nmodels must be >= 1");     // (the first of two)
    CHECK(job_counts_check("f", 0, 3, "nbasis", r) == JOBS_INVALID && std::string(r.msg) == "f: nbasis must be >= 1");
    CHECK(job_counts_check("f", 2, 0, "nmodels", r) == JOBS_INVALID && std::string(r.msg) == "f: njobs must be >= 1");
    r = JobRefusal{};
    CHECK(job_grid_check("f", 16, 16, 16, r) == JOBS_OK);
    CHECK(job_grid_check("f", 3, 17, 16, r) == JOBS_UNSUPPORTED && std::string(r.msg) == "f: 17 jobs, 3 models (more than the 16 workgroups of one grid)");
    CHECK(job_grid_check("f", 17, 3, 16, r) == JOBS_UNSUPPORTED && std::string(r.msg) == "f: 3 jobs, 17 models (more than the 16 workgroups of one grid)");
    r = JobRefusal{};
    CHECK(job_range_check("f", 2, 1, 2, 1, 2, "job_model", "nmodels", r) == JOBS_OK);
    CHECK(job_range_check("f", 2, 2, 2, 5, 2, "job_model", "nmodels", r) == JOBS_INVALID && std::string(r.msg) == "f: job_bag[2] = 2 outside 0..nbags-1");
    CHECK(job_range_check("f", 2, -1, 2, 0, 2, "job_model", "nmodels", r) == JOBS_INVALID && std::string(r.msg) == "f: job_bag[2] = -1 outside 0..nbags-1");
    CHECK(job_range_check("f", 4, 0, 2, 2, 2, "job_model", "nmodels", r) == JOBS_INVALID && std::string(r.msg) == "f: job_model[4] = 2 outside 0..nmodels-1");
    CHECK(job_range_check("f", 4, 0, 2, -3, 2, "job_basis", "nbasis", r) == JOBS_INVALID && std::string(r.msg) == "f: job_basis[4] = -3 outside 0..nbasis-1");
    // the walk: a rank outside the cap comes before any job's fault, a job's range before its hook, the first bad job before a later one
    JobSums t;
    Case b = q;
    b.model_H[1] = 33;
    b.job_bag[0] = 9;
    r = JobRefusal{};
    CHECK(job_walk("f", b.shape(), 32, t, r, no_hook) == JOBS_UNSUPPORTED && std::string(r.msg) == "f: model_H[1] = 33 (built for 1 <= H <= 32)");
    b.model_H[1] = 0;
    CHECK(job_walk("f", b.shape(), 32, t, r, no_hook) == JOBS_UNSUPPORTED && std::string(r.msg) == "f: model_H[1] = 0 (built for 1 <= H <= 32)");
    b = q;
    b.job_model[1] = 2;
    b.job_bag[2] = -1;
    int hooked = 0;
    auto refuse1 = [&](I j, I, I, I, I, JobRefusal& rr) { ++hooked; return j == 1 ? rr.set(JOBS_INVALID, "f: hook at %lld", (long long)j) : (int)JOBS_OK; };
    r = JobRefusal{};
    CHECK(job_walk("f", b.shape(), 32, t, r, refuse1) == JOBS_INVALID && std::string(r.msg) == "f: job_model[1] = 2 outside 0..nmodels-1" && hooked == 1);
    hooked = 0;
    r = JobRefusal{};
    CHECK(job_walk("f", q.shape(), 32, t, r, refuse1) == JOBS_INVALID && std::string(r.msg) == "f: hook at 1" && hooked == 2);
    // the hook sees the job's bag, model, width and rank; one rank for every model when model_H is null
    JobShape one = q.shape();
    one.model_H = nullptr;
    one.H_all = 6;
    I seenH = 0, seenW = 0;
    r = JobRefusal{};
    CHECK(job_walk("f", one, 32, t, r, [&](I j, I bb, I k, I Mb, I H, JobRefusal&) {
              CHECK(bb == q.job_bag[(size_t)j] && k == q.job_model[(size_t)j]);
              seenH += H; seenW += Mb;
              return (int)JOBS_OK;
          }) == JOBS_OK);
    CHECK(seenH == 18 && seenW == 3 + 1 + 1 && t.sumH == 12 && t.sumH2 == 72 && t.SMH == 30 && t.SJH == 18 && t.SJH2 == 108);
}

static void check_nonfinite() {
    const std::vector<I> Hs = {5, 16, 17, 32, 3};
    const I L = 7, nk = (I)Hs.size();
    const double bads[] = {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity()};
    int which = 0;
    auto run = [&](auto stride) {
        I n = 0;
        std::vector<I> first;
        for (I k = 0; k < nk; ++k) { first.push_back(n); n += stride(k); }
        std::vector<double> v((size_t)n, 1.5);
        I k = -1, e = -1;
        CHECK(!first_nonfinite(v.data(), nk, stride, k, e) && k == -1 && e == -1);
        for (const I m : {(I)0, nk / 2, nk - 1})
            for (const I at : {(I)0, stride(m) / 2, stride(m) - 1}) {
                v[(size_t)(first[(size_t)m] + at)] = bads[which++ & 1];
                if (m + 1 < nk) v[(size_t)first[(size_t)(m + 1)]] = bads[which & 1];      // a later one does not win
                CHECK(first_nonfinite(v.data(), nk, stride, k, e) && k == m && e == at);
                std::fill(v.begin(), v.end(), 1.5);
            }
    };
    run([&](I k) { return L * Hs[(size_t)k]; });
    run([&](I k) { return Hs[(size_t)k] * Hs[(size_t)k]; });
    run([&](I k) { return Hs[(size_t)k]; });
    run([](I) { return (I)1; });
}

int main() {
    // two tiers and two forms mixed, jobs repeated
    check_table(Case{{0, 1, 3, 6, 14, 84}, {5, 16, 17, 32}, {4, 0, 2, 2, 1, 3, 0, 4, 3}, {3, 0, 1, 1, 2, 0, 3, 3, 2}, {3, 0, 2, 0, 1, 2, 1, 3, 1}, 4, 33});
    check_table(Case{{0, 9}, {17}, {0, 0, 0}, {0, 0, 0}, {1, 0, 1}, 2, 5});                  // one model
    check_table(Case{{0, 2, 5}, {5, 32}, {1}, {1}, {1}, 2, 3});                              // one job
    check_table(Case{{0, 2, 5, 6}, {5, 8, 3}, {2, 0, 1, 1}, {0, 1, 2, 0}, {0, 0, 0, 0}, 4, 9});   // every job in one group
    check_table(Case{{0, 2, 5, 6}, {5, 8, 3}, {2, 0, 1, 1}, {0, 1, 2, 0}, {3, 3, 3, 3}, 4, 9});   // every job in the last group
    check_refusals();
    check_nonfinite();
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("the sums, the table, the refusals and the non-finite search hold\n");
    return 0;
}
