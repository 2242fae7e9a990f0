// host_bags.hpp -- the many-bags entries of the C ABI (batched vbls! of the basic and the sparse models, per-bag residuals, least
// squares and lower bounds, vbls! for (bag, model) jobs with and without each job's bound, many whole fits of the sparse and of the basic model, the bags' Y Y') and the host bookkeeping they share.  Part of vbmf_hip.hip's one translation unit: included there after the
// helpers it uses, never on its own.  The context's Y holds the bags side by side: bag b = columns col_off[b] .. col_off[b+1]-1.
//   bags_check     what every entry refuses about (nbags, col_off) and a sharded context; the widest bag, the residual slices
//   bags_reserve   ONE device scratch buffer (c->bags), grown on demand.  Every entry synchronises before it returns, so no two layouts
//                  are live together, and writes every slot before it reads it: it starts on whatever the last entry left there
// The (bag, model) job entries keep their bookkeeping -- the shared refusals, the sums, the int64 job table, the search for a non-finite
// input -- in job_tables.hpp, which knows nothing of the context; the parts that do are here:
//   jobs_refused, jobs_finite, jobs_stage, jobs_run_drained   that header's refusals as this library's errors, the host copies of the one
//                                                             upload and read-back, the launches with the stream drained on error
//   lb_of_bag      one bag's or job's bound from the device's sums (vjobs_call, vbmf_sparse_lower_bound_batched)
#pragma once

#include "job_tables.hpp"

struct BagDims { int64_t widest = 0, nslices = 0; };          // columns of the widest bag; residual workgroups (SCORE_CW columns each)

static int bags_check(vbmf_ctx* c, const char* fn, int64_t nbags, const int64_t* col_off, BagDims& bd) {
    if (c->o.nranks > 1) FAIL(c, VBMF_ERR_INVALID, "%s: row-sharded context (one rank only)", fn);
    if (nbags < 1 || nbags > (1ll << 30) || !col_off) FAIL(c, VBMF_ERR_INVALID, "%s: bad nbags / col_off", fn);
    if (col_off[0] != 0 || col_off[nbags] != c->M) FAIL(c, VBMF_ERR_INVALID, "%s: col_off must run from 0 to M = %lld", fn, (long long)c->M);
    bd = BagDims{};
    for (int64_t b = 0; b < nbags; ++b) {
        const int64_t w = col_off[b + 1] - col_off[b];
        if (w <= 0) FAIL(c, VBMF_ERR_INVALID, "%s: bag %lld is empty or col_off decreases", fn, (long long)b);
        bd.widest = std::max(bd.widest, w);
        bd.nslices += (w + SCORE_CW - 1) / SCORE_CW;
    }
    return VBMF_OK;
}

static int bags_reserve(vbmf_ctx* c, int64_t doubles, double** d) {
    if ((size_t)doubles * 8 > c->bags_bytes) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->bags_bytes = 0;
        MEMCHK(c, c->mem.regrow(c->bags, (size_t)doubles * 8));
        c->bags_bytes = (size_t)doubles * 8;
    }
    *d = c->bags;
    return VBMF_OK;
}

// S_b = P_b'P_b (S = nullptr: not formed) and ||Y_b||^2 of every bag; frag_nh: P is fragment-major (0: row-major [h][x])
static int bags_launch_gram(vbmf_ctx* c, int64_t nb, const float* P, int frag_nh, const long long* d_off, double* S, double* yy) {
    dispatch<MODE_F32, MODE_BF16>(ymode_of(c->mode), [&](auto ym) {
        hipLaunchKernelGGL((bag_gram_kernel<decltype(ym)::value>), dim3((unsigned)nb), dim3(256), 0, c->stream, P, (long long)c->d1.XT * 32, frag_nh,
                           c->Y2, c->d2.KS, (long long)c->L, d_off, (int)c->H, S, yy);
    });
    HIPCHK(c, hipGetLastError());
    return VBMF_OK;
}

// ---- vbls! over many bags ---------------------------------------------------------------------------------------------------------
extern "C" {

// vbls! over many bags with one fixed basis (examples/mil_util.jl:473-479 in one call).  B, SigmaB, CB come from the state, every
// other input and output is per bag and lives in c->bags -- the state itself (A, SigmaA, CA, sigma2) is not touched, so the same
// upload can be run against another basis after another vbmf_set_state.
int vbmf_run_fixed_basis_batched(vbmf_ctx* c, int64_t nbags, const int64_t* col_off, int64_t niter, double* sigma2, double* CA_diag,
                                 double* SigmaA, double* AHat, int64_t ldA) {
    if (!c) return VBMF_ERR_INVALID;
    const char* fn = "vbmf_run_fixed_basis_batched";
    if (c->sparse) FAIL(c, VBMF_ERR_INVALID, "%s: sparse context (the basic model only)", fn);
    if (c->has_mask) FAIL(c, VBMF_ERR_INVALID, "%s: a label mask is set (use vbmf_run_fixed_basis per bag)", fn);
    if (c->H > 64) FAIL(c, VBMF_ERR_INVALID, "%s: H = %lld > 64", fn, (long long)c->H);
    if (niter < 1 || niter > (1ll << 30)) FAIL(c, VBMF_ERR_INVALID, "%s: niter must be >= 1", fn);
    BagDims bd;
    TRY(bags_check(c, fn, nbags, col_off, bd));
    if (!sigma2 || !CA_diag) FAIL(c, VBMF_ERR_INVALID, "%s: null sigma2 / CA_diag", fn);
    if (AHat && ldA < c->M) FAIL(c, VBMF_ERR_INVALID, "%s: ldA < M", fn);
    HIPCHK(c, hipSetDevice(c->o.device));
    TRY(ensure_ready(c));
    c->cache.W_dropped();
    TRY(ensure_gram_B(c));
    const int H = (int)c->H;
    const int64_t nb = nbags, h2 = (int64_t)H * H;
    // c->bags: [col_off (nb + 1 int64) | sigma2 nb | CA nb H | SigmaA nb H^2 | T nb H^2 | S nb H^2 | ||Y_b||^2 nb | A M H]
    const int64_t n_off = nb + 1, o_s2 = n_off, o_ca = o_s2 + nb, o_sa = o_ca + nb * H, o_t = o_sa + nb * h2, o_s = o_t + nb * h2,
                  o_yy = o_s + nb * h2, o_a = o_yy + nb, total = o_a + (int64_t)c->M * H;
    double* d = nullptr;
    TRY(bags_reserve(c, total, &d));
    long long* d_off = reinterpret_cast<long long*>(d);
    std::vector<double> in((size_t)(nb + nb * H));
    memcpy(in.data(), sigma2, (size_t)nb * 8);
    memcpy(in.data() + nb, CA_diag, (size_t)nb * H * 8);
    HIPCHK(c, hipMemcpyAsync(d_off, col_off, (size_t)n_off * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d + o_s2, in.data(), in.size() * 8, hipMemcpyHostToDevice, c->stream));
    // P = Y'B of every bag: one pass 1 with the frozen B (no control chain, no A update: the state stays as it is)
    c->P_frag = fused_gram(c) || frag_post(c);
    TRY(launch_stream(c, 0, 0, false, nullptr, c->P_frag));
    c->cache.P_overwritten();
    if (sharded(c) || c->d1.nsplit > 1) {
        const long long n = (long long)c->Hp * c->d1.XT * 32;
        hipLaunchKernelGGL(slab_sum_kernel, dim3(grid_for(n / 4, 256, 2048)), dim3(256), 0, c->stream, c->P, c->d1.nsplit, n,
                           sharded(c) ? c->P : c->Pred, n, c->ints + I_STOP, SideCopy{});
        HIPCHK(c, hipGetLastError());
        if (sharded(c)) TRY(allreduce_sum(c, c->P, c->Pred, (size_t)n, false));
    }
    const float* Psrc = (sharded(c) || c->d1.nsplit > 1) ? c->Pred : c->P;
    const long long ldP = (long long)c->d1.XT * 32;
    const int fnh = c->P_frag ? c->NH : 0;
    TRY(bags_launch_gram(c, nb, Psrc, fnh, d_off, d + o_s, d + o_yy));
    const size_t lds = vbls_lds_bytes(nb_tier(H));
    dispatch<1, 2, 4>(nb_tier(H), [&](auto nbk) {
        hipLaunchKernelGGL((vbls_batch_kernel<decltype(nbk)::value>), dim3((unsigned)nb), dim3(256), lds, c->stream, c->st, c->lay, H, (double)c->Lg, d_off,
                           (int)niter, d + o_s, d + o_yy, d + o_s2, d + o_ca, d + o_sa, d + o_t, c->ints);
    });
    HIPCHK(c, hipGetLastError());
    if (AHat) {
        hipLaunchKernelGGL(bag_a_kernel, dim3(grid_for(c->M * H)), dim3(256), 0, c->stream, Psrc, ldP, fnh, d_off, (int)nb, H, d + o_t,
                           (long long)c->M, d + o_a);
        HIPCHK(c, hipGetLastError());
    }
    // read-back: [sigma2 | CA | SigmaA] is one contiguous block, A one 2-D copy into the caller's leading dimension
    std::vector<double> out((size_t)(o_t - o_s2));
    HIPCHK(c, hipMemcpyAsync(out.data(), d + o_s2, out.size() * 8, hipMemcpyDeviceToHost, c->stream));
    if (AHat)
        HIPCHK(c, hipMemcpy2DAsync(AHat, (size_t)ldA * 8, d + o_a, (size_t)c->M * 8, (size_t)c->M * 8, (size_t)H, hipMemcpyDeviceToHost,
                                   c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    memcpy(sigma2, out.data(), (size_t)nb * 8);
    memcpy(CA_diag, out.data() + nb, (size_t)nb * H * 8);
    if (SigmaA) memcpy(SigmaA, out.data() + (o_sa - o_s2), (size_t)nb * h2 * 8);     // symmetric: row- and column-major alike
    return check_device_err(c);
}

// vbls! of the sparse models over many bags with one fixed basis (examples/mil_util.jl:187-197 in one call, both updateA! forms).
// B, SigmaB come from the state, every other input and output is per bag and lives in c->bags -- the state itself (A, CA, beta,
// SigmaA, sigma, zeta) is not touched, so one upload serves another basis.
int vbmf_sparse_run_fixed_basis_batched(vbmf_ctx* c, int64_t nbags, const int64_t* col_off, int64_t niter, int full_cov,
                                        const double* alpha, const double* beta0, const double* eta, const double* zeta0,
                                        double* sigmaHat, double* CA, double* zeta, double* beta, double* diagSigmaATVec,
                                        double* SigmaA, double* ATVecHat) {
    if (!c) return VBMF_ERR_INVALID;
    const char* fn = "vbmf_sparse_run_fixed_basis_batched";
    if (!c->sparse) FAIL(c, VBMF_ERR_INVALID, "%s: basic context (the sparse models only; use vbmf_run_fixed_basis_batched)", fn);
    if (c->diagvar) FAIL(c, VBMF_ERR_INVALID, "%s: diag_var context (homoscedastic only; use vbmf_sparse_run_fixed_basis per bag)", fn);
    if (c->has_mask) FAIL(c, VBMF_ERR_INVALID, "%s: a label mask is set (use vbmf_sparse_run_fixed_basis per bag)", fn);
    if (c->H > 64) FAIL(c, VBMF_ERR_INVALID, "%s: H = %lld > 64", fn, (long long)c->H);
    if (niter < 1 || niter > (1ll << 30)) FAIL(c, VBMF_ERR_INVALID, "%s: niter must be >= 1", fn);
    BagDims bd;
    TRY(bags_check(c, fn, nbags, col_off, bd));
    if (!alpha || !beta0 || !eta || !zeta0 || !sigmaHat || !CA) FAIL(c, VBMF_ERR_INVALID, "%s: null alpha / beta0 / eta / zeta0 / sigmaHat / CA", fn);
    HIPCHK(c, hipSetDevice(c->o.device));
    TRY(ensure_ready(c));
    TRY(ensure_gram_B(c));
    const int H = (int)c->H;
    const int64_t nb = nbags, MH = (int64_t)c->M * H, h2 = (int64_t)H * H;
    // c->bags: [col_off nb + 1 | alpha nb H | beta0 nb H | eta | zeta0 | sigma | zeta | ||Y_b||^2 (nb each) | CA | A | dS | beta | P (M H each)
    //           | SigmaA nb H^2 | G H^2 | diag(B'B) H | L diag(SigmaB) H]
    const int64_t o_al = nb + 1, o_b0 = o_al + nb * H, o_eta = o_b0 + nb * H, o_z0 = o_eta + nb, o_sig = o_z0 + nb, o_zeta = o_sig + nb,
                  o_yy = o_zeta + nb, o_ca = o_yy + nb, o_a = o_ca + MH, o_ds = o_a + MH, o_be = o_ds + MH, o_p = o_be + MH,
                  o_sa = o_p + MH, o_g = o_sa + nb * h2, o_gd = o_g + h2, o_sd = o_gd + H, total = o_sd + H;
    double* d = nullptr;
    TRY(bags_reserve(c, total, &d));
    long long* d_off = reinterpret_cast<long long*>(d);
    std::vector<double> in((size_t)(o_zeta - o_al));
    memcpy(in.data(), alpha, (size_t)nb * H * 8);
    memcpy(in.data() + (o_b0 - o_al), beta0, (size_t)nb * H * 8);
    memcpy(in.data() + (o_eta - o_al), eta, (size_t)nb * 8);
    memcpy(in.data() + (o_z0 - o_al), zeta0, (size_t)nb * 8);
    memcpy(in.data() + (o_sig - o_al), sigmaHat, (size_t)nb * 8);
    // The pass and slab kernels are gated by the stop flag, so a raised flag is lowered for this call and raised again after it.  No
    // path arrives here with it up: only a run loop's closing control step raises it, and every run ends (RunFrame::finish) by writing
    // zeros over the first four ints.  It could stay up only if that copy itself failed; the step is kept as the guard for that.
    int ints0[4];
    HIPCHK(c, memcpy_sync(c, ints0, c->ints, sizeof ints0, hipMemcpyDeviceToHost));
    if (ints0[I_STOP]) HIPCHK(c, hipMemsetAsync(c->ints + I_STOP, 0, sizeof(int), c->stream));
    HIPCHK(c, hipMemcpyAsync(d_off, col_off, (size_t)(nb + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d + o_al, in.data(), in.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d + o_ca, CA, (size_t)MH * 8, hipMemcpyHostToDevice, c->stream));
    // P = Y'B of every bag in the plain [h][m] layout: one pass 1 with the frozen B (no A update: the state stays as it is)
    const int* stop = c->ints + I_STOP;
    c->P_frag = false;
    TRY(launch_stream(c, 0));
    const long long np = (long long)c->Hp * c->d1.XT * 32;
    hipLaunchKernelGGL(slab_sum_kernel, dim3(grid_for(np / 4, 256, 2048)), dim3(256), 0, c->stream, c->P, c->d1.nsplit, np, c->Pred, np, stop,
                       SideCopy{});
    c->cache.P_overwritten();
    const long long ldP = (long long)c->d1.XT * 32;
    TRY(bags_launch_gram(c, nb, c->Pred, 0, d_off, nullptr, d + o_yy));
    hipLaunchKernelGGL(sbatch_g_kernel, dim3(cdiv(h2, 256)), dim3(256), 0, c->stream, c->st, c->lay, H, (double)c->Lg, d + o_g, d + o_gd,
                       d + o_sd);
    HIPCHK(c, hipGetLastError());
    // the bag's state in LDS up to the launch's budget (every bag of an MIL study fits), else in its slices of c->bags
    const int NBK = nb_tier(H);
    const size_t cap = (full_cov && NBK == 4) ? SBATCH_LDS_BIG : SBATCH_LDS_SMALL;
    const int nfix = sbatch_fixed_doubles(full_cov != 0, NBK, H);
    const int64_t room = (int64_t)(cap / 8) - nfix;
    const int lds_state = (int)std::max<int64_t>(0, std::min<int64_t>(4 * bd.widest * H, room));
    const size_t lds = (size_t)(nfix + lds_state) * 8;
    SbatchArgs a{c->Pred, ldP, d_off, H, (int)niter, (c->o.reference_compat & VBMF_COMPAT_SPARSE_REPEAT) ? 1 : 0, lds_state, (double)c->Lg,
                 d + o_g, d + o_gd, d + o_sd, d + o_al, d + o_b0, d + o_eta, d + o_z0, d + o_yy, d + o_sig, d + o_zeta,
                 d + o_ca, d + o_a, d + o_ds, d + o_be, d + o_p, d + o_sa, c->ints + I_ERR};
    dispatch<1, 2, 4>(NBK, [&](auto nbk) {
        dispatch<0, 1>(full_cov ? 1 : 0, [&](auto full) {
            hipLaunchKernelGGL((sparse_batch_kernel<decltype(nbk)::value, decltype(full)::value != 0>), dim3((unsigned)nb), dim3(SBATCH_THREADS), lds,
                               c->stream, a);
        });
    });
    HIPCHK(c, hipGetLastError());
    if (ints0[I_STOP]) HIPCHK(c, hipMemcpyAsync(c->ints + I_STOP, &ints0[I_STOP], sizeof(int), hipMemcpyHostToDevice, c->stream));
    // read-back: [sigma | zeta] and [CA | A | dS | beta] and SigmaA are contiguous blocks
    std::vector<double> sz((size_t)2 * nb);
    HIPCHK(c, hipMemcpyAsync(sz.data(), d + o_sig, sz.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(CA, d + o_ca, (size_t)MH * 8, hipMemcpyDeviceToHost, c->stream));
    if (ATVecHat) HIPCHK(c, hipMemcpyAsync(ATVecHat, d + o_a, (size_t)MH * 8, hipMemcpyDeviceToHost, c->stream));
    if (diagSigmaATVec) HIPCHK(c, hipMemcpyAsync(diagSigmaATVec, d + o_ds, (size_t)MH * 8, hipMemcpyDeviceToHost, c->stream));
    if (beta) HIPCHK(c, hipMemcpyAsync(beta, d + o_be, (size_t)MH * 8, hipMemcpyDeviceToHost, c->stream));
    if (SigmaA) HIPCHK(c, hipMemcpyAsync(SigmaA, d + o_sa, (size_t)(nb * h2) * 8, hipMemcpyDeviceToHost, c->stream));   // symmetric
    HIPCHK(c, hipStreamSynchronize(c->stream));
    memcpy(sigmaHat, sz.data(), (size_t)nb * 8);
    if (zeta) memcpy(zeta, sz.data() + nb, (size_t)nb * 8);
    return check_device_err(c);
}

}  // extern "C"

// ---- per-bag scoring (score_kernels.hpp) ----------------------------------------------------------------------------------------
// what the three scoring entries refuse before any launch
static int score_check(vbmf_ctx* c, const char* fn, int64_t nbags, const int64_t* col_off, BagDims& bd) {
    if (c->diagvar) FAIL(c, VBMF_ERR_INVALID, "%s: diag_var context (homoscedastic only)", fn);
    TRY(bags_check(c, fn, nbags, col_off, bd));
    if (score_resid_lds_bytes((int)c->H) > 64 * 1024) FAIL(c, VBMF_ERR_UNSUPPORTED, "%s: H = %lld (a slice's rows of A exceed 64 KiB of LDS)", fn, (long long)c->H);
    return VBMF_OK;
}

// uploads [col_off | chunk_off] to d_off: chunk_off[b] = bag b's first slice number
static int score_upload_offsets(vbmf_ctx* c, int64_t nb, const int64_t* col_off, long long* d_off) {
    std::vector<long long> off((size_t)(2 * (nb + 1)));
    off[(size_t)(nb + 1)] = 0;
    for (int64_t b = 0; b <= nb; ++b) off[(size_t)b] = col_off[b];
    for (int64_t b = 0; b < nb; ++b)
        off[(size_t)(nb + 2 + b)] = off[(size_t)(nb + 1 + b)] + (col_off[b + 1] - col_off[b] + SCORE_CW - 1) / SCORE_CW;
    HIPCHK(c, hipMemcpyAsync(d_off, off.data(), off.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));                // (off is a local)
    return VBMF_OK;
}

// uploads the offsets and enqueues the two residual kernels: r2 of every bag into d_r2 (d_part: ns partials).
// d_A: the device copy of A with element strides (sm, sh).
static int score_launch_resid(vbmf_ctx* c, int64_t nb, const int64_t* col_off, int64_t ns, long long* d_off, const double* d_A,
                              long long sm, long long sh, double* d_part, double* d_r2) {
    TRY(score_upload_offsets(c, nb, col_off, d_off));
    TRY(rebuild_B32_if_stale(c));
    const size_t lds = score_resid_lds_bytes((int)c->H);
    dispatch<MODE_F32, MODE_BF16>(ymode_of(c->mode), [&](auto ym) {
        hipLaunchKernelGGL((bag_resid_kernel<decltype(ym)::value>), dim3((unsigned)ns), dim3(SCORE_THREADS), lds, c->stream, c->Y2, c->d2.KS,
                           (long long)c->L, c->B32[c->bcur], c->Hp, (int)c->H, d_A, sm, sh, d_off, d_off + nb + 1, (int)nb, d_part);
    });
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(bag_resid_fold_kernel, dim3(cdiv(nb, 256)), dim3(256), 0, c->stream, d_part, d_off + nb + 1, (int)nb, d_r2);
    HIPCHK(c, hipGetLastError());
    return VBMF_OK;
}

// ---- what the job entries share on top of job_tables.hpp: the parts that need the context ------------------------------------------
// a refusal of job_tables.hpp as this library's error text and code
static int jobs_refused(vbmf_ctx* c, const JobRefusal& r) {
    FAIL(c, r.kind == JOBS_UNSUPPORTED ? VBMF_ERR_UNSUPPORTED : VBMF_ERR_INVALID, "%s", r.msg);
}

// refuses a per-model packed input (stride(k) entries of model k) with an entry that is not finite, naming the model and the entry
template <class Stride>
static int jobs_finite(vbmf_ctx* c, const char* fn, const char* name, const double* v, int64_t nk, Stride stride, bool with_entry = true) {
    int64_t k = 0, e = 0;
    if (!first_nonfinite(v, nk, stride, k, e)) return VBMF_OK;
    if (!with_entry) FAIL(c, VBMF_ERR_INVALID, "%s: %s of model %lld is not finite", fn, name, (long long)k);
    FAIL(c, VBMF_ERR_INVALID, "%s: %s of model %lld is not finite (entry %lld)", fn, name, (long long)k, (long long)e);
}

// the host copies of the one upload and the one read-back; bytes, what: how the refusal words the request
static int jobs_stage(vbmf_ctx* c, const char* fn, std::vector<double>& up, int64_t n_up, std::vector<double>& res, int64_t n_res,
                      int64_t bytes, const char* what) {
    try {
        up.resize((size_t)n_up);
        res.resize((size_t)n_res);
    } catch (const std::bad_alloc&) {
        FAIL(c, VBMF_ERR_UNSUPPORTED, "%s: no host memory to stage %lld bytes of %s", fn, (long long)bytes, what);
    }
    return VBMF_OK;
}

// run() enqueues from and reads back into the caller's locals: after an error nothing may still be copying when they go
template <class Run>
static int jobs_run_drained(vbmf_ctx* c, Run run) {
    const int rc = run();
    if (rc != VBMF_OK) hipStreamSynchronize(c->stream);
    return rc;
}

// The bound of one bag (or job) from what the device summed: sums = SCORE_NS column sums for each of its H columns, quad = its pair,
// r2 its residual; a_pri, b_pri, a_post its H prior entries.  The caller has filled s.L, s.H, the noise and hyper fields and the basis'
// sums; this fills the rest and grp[0 .. H).  finite: the bound and every sum it was made of are.
static double lb_of_bag(LbSums& s, LbGroup* grp, int H, double Mb, double r2, const double* sums, const double* quad, bool trimmed,
                        bool grouped, const double* a_pri, const double* b_pri, const double* a_post, int clamp, bool& finite) {
    // src/vbmf_sparse.jl:482-486 trims beta and CA with ATVecHat; the grouped models' per-group fields stay whole
    const bool cut = trimmed && !grouped;
    double n_keep = 0, s_caq = 0, s_logds = 0;
    for (int h = 0; h < H; ++h) {
        const double* q = sums + (size_t)h * SCORE_NS;
        n_keep += q[2]; s_caq += q[5]; s_logds += q[6];
        grp[h] = LbGroup{cut ? q[2] : Mb, cut ? q[3] : q[0], cut ? q[4] : q[1], a_pri[h], b_pri[h], a_post[h]};
    }
    s.M = Mb;
    s.MH = trimmed ? n_keep : Mb * (double)H;
    s.quad = r2 + s.L * quad[0] + quad[1];
    s.s_caq = s_caq; s.s_logds = s_logds;
    s.g = grp; s.ng = H;
    const double v = lb_assemble(s, clamp);
    finite = std::isfinite(v) && std::isfinite(s.quad) && std::isfinite(s_caq) && std::isfinite(s_logds);
    return v;
}

extern "C" {

// norm(Y - BHat*AHat')^2 of every bag (examples/mil_util.jl:476-479, :518-521) in one call, entry by entry in fp64
int vbmf_bag_residuals(vbmf_ctx* c, int64_t nbags, const int64_t* col_off, const double* AHat, int64_t ldA, double* r2) {
    if (!c) return VBMF_ERR_INVALID;
    const char* fn = "vbmf_bag_residuals";
    BagDims bd;
    TRY(score_check(c, fn, nbags, col_off, bd));
    if (!AHat || !r2) FAIL(c, VBMF_ERR_INVALID, "%s: null AHat / r2", fn);
    if (ldA < c->M) FAIL(c, VBMF_ERR_INVALID, "%s: ldA < M", fn);
    HIPCHK(c, hipSetDevice(c->o.device));
    TRY(ensure_ready(c));
    const int64_t nb = nbags, ns = bd.nslices, H = c->H;
    // c->bags: [col_off nb + 1 | chunk_off nb + 1 | r2 nb | partials ns | A M H (column-major, ld M)]
    const int64_t o_r2 = 2 * (nb + 1), o_part = o_r2 + nb, o_a = o_part + ns, total = o_a + c->M * H;
    double* d = nullptr;
    TRY(bags_reserve(c, total, &d));
    HIPCHK(c, hipMemcpy2DAsync(d + o_a, (size_t)c->M * 8, AHat, (size_t)ldA * 8, (size_t)c->M * 8, (size_t)H, hipMemcpyHostToDevice, c->stream));
    TRY(score_launch_resid(c, nb, col_off, ns, reinterpret_cast<long long*>(d), d + o_a, 1, (long long)c->M, d + o_part, d + o_r2));
    HIPCHK(c, memcpy_sync(c, r2, d + o_r2, (size_t)nb * 8, hipMemcpyDeviceToHost));
    for (int64_t b = 0; b < nb; ++b)
        if (!std::isfinite(r2[b])) FAIL(c, VBMF_ERR_NUMERIC, "%s: non-finite residual in bag %lld", fn, (long long)b);
    return VBMF_OK;
}

// ols / rls of examples/mil_util.jl:159-171 and the norm(Y - BHat*AT)^2 of :483-484 for every bag, against the caller's fp64 basis
int vbmf_bag_least_squares(vbmf_ctx* c, int64_t nbags, const int64_t* col_off, const double* BHat, int64_t ldB, int64_t H, double lambda,
                           double* X, int64_t ldX, double* r2) {
    if (!c) return VBMF_ERR_INVALID;
    const char* fn = "vbmf_bag_least_squares";
    if (H < 1 || H > LS_MAX_H) FAIL(c, VBMF_ERR_UNSUPPORTED, "%s: H = %lld (built for 1 <= H <= %d)", fn, (long long)H, LS_MAX_H);
    BagDims bd;
    TRY(score_check(c, fn, nbags, col_off, bd));
    if (!(lambda >= 0.0) || !std::isfinite(lambda)) FAIL(c, VBMF_ERR_INVALID, "%s: lambda must be finite and >= 0", fn);
    if (!BHat) FAIL(c, VBMF_ERR_INVALID, "%s: null BHat", fn);
    if (!X && !r2) FAIL(c, VBMF_ERR_INVALID, "%s: X and r2 are both NULL", fn);
    const int64_t L = c->L, M = c->M, nb = nbags, ns = bd.nslices;
    if (ldB < L) FAIL(c, VBMF_ERR_INVALID, "%s: ldB < L", fn);
    if (X && ldX < H) FAIL(c, VBMF_ERR_INVALID, "%s: ldX < H", fn);
    std::vector<double> Bt((size_t)(L * H));                   // row-major [L][H]
    for (int64_t h = 0; h < H; ++h)
        for (int64_t l = 0; l < L; ++l) {
            const double v = BHat[h * ldB + l];
            if (!std::isfinite(v)) FAIL(c, VBMF_ERR_INVALID, "%s: BHat[%lld, %lld] is not finite", fn, (long long)l, (long long)h);
            Bt[(size_t)(l * H + h)] = v;
        }
    if (!c->cache.have_Y()) FAIL(c, VBMF_ERR_INVALID, "%s: no Y: call vbmf_set_Y first", fn);     // (no state needed: the basis is an argument)
    HIPCHK(c, hipSetDevice(c->o.device));
    const int64_t nchunk = cdiv(L, LS_ROWS), h2 = H * H;
    // c->bags: [col_off nb + 1 | chunk_off nb + 1 | r2 nb | bad-pivot flag | partials ns | B L H (row-major) | Gram partials nchunk H^2
    //           | K H^2 | X M H (column m at m H)]
    // (the flag slot starts with another entry's bytes: bag_ls_inverse_kernel stores it on every launch)
    const int64_t o_r2 = 2 * (nb + 1), o_flag = o_r2 + nb, o_part = o_flag + 1, o_b = o_part + ns, o_g = o_b + L * H,
                  o_k = o_g + nchunk * h2, o_x = o_k + h2, total = o_x + M * H;
    double* d = nullptr;
    TRY(bags_reserve(c, total, &d));
    long long* d_off = reinterpret_cast<long long*>(d);
    HIPCHK(c, hipMemcpyAsync(d + o_b, Bt.data(), Bt.size() * 8, hipMemcpyHostToDevice, c->stream));
    TRY(score_upload_offsets(c, nb, col_off, d_off));           // (its synchronize also covers Bt)
    hipLaunchKernelGGL(bag_ls_gram_kernel, dim3((unsigned)nchunk), dim3(SCORE_THREADS), 0, c->stream, d + o_b, (long long)L, (int)H, d + o_g);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(bag_ls_inverse_kernel, dim3(1), dim3(256), spd_inverse_lds_bytes(LS_MAX_H / 16), c->stream, d + o_g, (int)nchunk,
                       (int)H, lambda, d + o_k, reinterpret_cast<int*>(d + o_flag));
    HIPCHK(c, hipGetLastError());
    double* d_x = X ? d + o_x : nullptr;
    double* d_part = r2 ? d + o_part : nullptr;
    const size_t lds = score_ls_lds_bytes((int)H);
    dispatch<MODE_F32, MODE_BF16>(ymode_of(c->mode), [&](auto ym) {
        hipLaunchKernelGGL((bag_ls_kernel<decltype(ym)::value>), dim3((unsigned)ns), dim3(SCORE_THREADS), lds, c->stream, c->Y2, c->d2.KS, (long long)L,
                           d + o_b, (int)H, d + o_k, d_off, d_off + nb + 1, (int)nb, d_x, d_part);
    });
    HIPCHK(c, hipGetLastError());
    if (r2) {
        hipLaunchKernelGGL(bag_resid_fold_kernel, dim3(cdiv(nb, 256)), dim3(256), 0, c->stream, d_part, d_off + nb + 1, (int)nb, d + o_r2);
        HIPCHK(c, hipGetLastError());
    }
    std::vector<double> res((size_t)(nb + 1));                  // r2 | flag
    HIPCHK(c, memcpy_sync(c, res.data(), d + o_r2, res.size() * 8, hipMemcpyDeviceToHost));
    int bad = 0;
    std::memcpy(&bad, &res[(size_t)nb], sizeof(int));
    if (bad) FAIL(c, VBMF_ERR_NUMERIC, "%s: B'B + lambda I is not positive definite (a pivot is not positive or not finite)", fn);
    if (r2)
        for (int64_t b = 0; b < nb; ++b)
            if (!std::isfinite(res[(size_t)b])) FAIL(c, VBMF_ERR_NUMERIC, "%s: non-finite residual in bag %lld", fn, (long long)b);
    if (X) {
        HIPCHK(c, hipMemcpy2DAsync(X, (size_t)ldX * 8, d + o_x, (size_t)H * 8, (size_t)H * 8, (size_t)M, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    if (r2) std::memcpy(r2, res.data(), (size_t)nb * 8);
    return VBMF_OK;
}

// test_classification (examples/mil_util.jl:558-587) of every fold of validate_with_cvs (:627-648) at once: many bases, and a list of
// (bag, basis) jobs each of which is what vbmf_bag_least_squares computes for that bag with that basis and lambda, bit for bit -- the
// kernels of both entries run the same __device__ functions (score_kernels.hpp).  Four launches and one synchronising read-back,
// whatever nbasis and njobs are.
int vbmf_bag_least_squares_jobs(vbmf_ctx* c, int64_t nbags, const int64_t* col_off, int64_t nbasis, const int64_t* Hs, const double* BHat,
                                const double* lambda, int64_t njobs, const int64_t* job_bag, const int64_t* job_basis, double* X,
                                double* r2, int64_t* status) {
    if (!c) return VBMF_ERR_INVALID;
    const char* fn = "vbmf_bag_least_squares_jobs";
    JobRefusal ref;
    if (job_counts_check(fn, nbasis, njobs, "nbasis", ref)) return jobs_refused(c, ref);
    if (!Hs || !BHat || !lambda || !job_bag || !job_basis || !status)
        FAIL(c, VBMF_ERR_INVALID, "%s: null pointer (only X or r2 may be NULL)", fn);
    if (!X && !r2) FAIL(c, VBMF_ERR_INVALID, "%s: X and r2 are both NULL", fn);
    const int64_t L = c->L, nb = nbags, nk = nbasis, nj = njobs, nchunk = cdiv(L, LS_ROWS);
    // what one grid holds: a launch is kept to 2^32 - 1 threads in all, so to LS_MAX_GROUPS workgroups of SCORE_THREADS
    if (nk > LS_MAX_GROUPS / nchunk)
        FAIL(c, VBMF_ERR_UNSUPPORTED, "%s: %lld bases of %lld row chunks (more than %lld workgroups in one grid)", fn, (long long)nk, (long long)nchunk,
             (long long)LS_MAX_GROUPS);
    if (nj > LS_MAX_GROUPS)                                       // (a job has at least one slice)
        FAIL(c, VBMF_ERR_UNSUPPORTED, "%s: %lld jobs (more job slices than the %lld workgroups of one grid)", fn, (long long)nj, (long long)LS_MAX_GROUPS);
    int64_t sumH = 0, sumH2 = 0, Hmax = 0;
    for (int64_t k = 0; k < nk; ++k) {
        if (Hs[k] < 1 || Hs[k] > LS_MAX_H)
            FAIL(c, VBMF_ERR_UNSUPPORTED, "%s: Hs[%lld] = %lld (built for 1 <= H <= %d)", fn, (long long)k, (long long)Hs[k], LS_MAX_H);
        sumH += Hs[k];
        sumH2 += Hs[k] * Hs[k];
        Hmax = std::max(Hmax, Hs[k]);
    }
    BagDims bd;
    TRY(score_check(c, fn, nbags, col_off, bd));
    for (int64_t k = 0; k < nk; ++k)
        if (!(lambda[k] >= 0.0) || !std::isfinite(lambda[k]))
            FAIL(c, VBMF_ERR_INVALID, "%s: lambda[%lld] must be finite and >= 0", fn, (long long)k);
    int64_t nsl = 0, sumX = 0;
    for (int64_t j = 0; j < nj; ++j) {
        const int64_t b = job_bag[j], k = job_basis[j];
        if (job_range_check(fn, j, b, nb, k, nk, "job_basis", "nbasis", ref)) return jobs_refused(c, ref);
        const int64_t Mb = col_off[b + 1] - col_off[b];
        nsl += (Mb + SCORE_CW - 1) / SCORE_CW;                    // (at most 2^24 terms of at most 2^60 / 8: no overflow)
        sumX += Hs[k] * Mb;
    }
    if (nsl > LS_MAX_GROUPS)
        FAIL(c, VBMF_ERR_UNSUPPORTED, "%s: %lld job slices (more than the %lld workgroups of one grid)", fn, (long long)nsl, (long long)LS_MAX_GROUPS);
    // the upload, one block: [col_off nb + 1 | sl0 nj + 1 | job_bag | job_basis | x_off (nj each) | Hs | b_off | k_off (nk each) (int64)
    //                         | lambda nk | the bases row-major [L][H_k], one after the other]
    const int64_t u_sl = nb + 1, u_bag = u_sl + nj + 1, u_bas = u_bag + nj, u_xo = u_bas + nj, u_hs = u_xo + nj, u_bo = u_hs + nk,
                  u_ko = u_bo + nk, u_lam = u_ko + nk, u_b = u_lam + nk, n_up = u_b + L * sumH;
    std::vector<double> up, res;                                  // (up outlives the copy: an error after it drains the stream); res: r2 | the flags
    TRY(jobs_stage(c, fn, up, n_up, res, nj + nk, n_up * 8, "bases and job tables"));
    long long* ui = reinterpret_cast<long long*>(up.data());
    for (int64_t j = 0, sl = 0, xo = 0; j < nj; ++j) {
        const int64_t b = job_bag[j], k = job_basis[j], Mb = col_off[b + 1] - col_off[b];
        ui[u_sl + j] = sl;
        ui[u_bag + j] = b;
        ui[u_bas + j] = k;
        ui[u_xo + j] = xo;
        sl += (Mb + SCORE_CW - 1) / SCORE_CW;
        xo += Hs[k] * Mb;
    }
    ui[u_sl + nj] = nsl;
    for (int64_t b = 0; b <= nb; ++b) ui[b] = col_off[b];
    for (int64_t k = 0, bo = 0, ko = 0; k < nk; ++k) {
        const int64_t H = Hs[k];
        ui[u_hs + k] = H;
        ui[u_bo + k] = bo;
        ui[u_ko + k] = ko;
        up[(size_t)(u_lam + k)] = lambda[k];
        double* Bt = up.data() + u_b + bo;
        for (int64_t h = 0; h < H; ++h)
            for (int64_t l = 0; l < L; ++l) {
                const double v = BHat[bo + h * L + l];
                if (!std::isfinite(v))
                    FAIL(c, VBMF_ERR_INVALID, "%s: BHat of basis %lld [%lld, %lld] is not finite", fn, (long long)k, (long long)l, (long long)h);
                Bt[l * H + h] = v;
            }
        bo += L * H;
        ko += H * H;
    }
    if (!c->cache.have_Y()) FAIL(c, VBMF_ERR_INVALID, "%s: no Y: call vbmf_set_Y first", fn);     // (no state needed: the bases are arguments)
    TRY(jobs_run_drained(c, [&]() -> int {
        HIPCHK(c, hipSetDevice(c->o.device));
        // c->bags: [the upload | r2 nj | bad-pivot flags nk (an int in each slot) | partials nsl | Gram partials nchunk sum H_k^2
        //           | K sum H_k^2 | X sum H_k M_b (job j's block at x_off[j])]
        // (every slot is written before it is read: the flags by the inverse kernel, the partials by the job kernel)
        const int64_t o_r2 = n_up, o_flag = o_r2 + nj, o_part = o_flag + nk, o_g = o_part + nsl, o_k = o_g + nchunk * sumH2,
                      o_x = o_k + sumH2, total = o_x + (X ? sumX : 0);
        double* d = nullptr;
        TRY(bags_reserve(c, total, &d));
        HIPCHK(c, hipMemcpyAsync(d, up.data(), (size_t)n_up * 8, hipMemcpyHostToDevice, c->stream));
        const long long* di = reinterpret_cast<const long long*>(d);
        const LsBases bs{di + u_hs, di + u_bo, di + u_ko, d + u_lam, d + u_b};
        const LsJobs jobs{di + u_sl, di + u_bag, di + u_bas, di + u_xo, (int)nj};
        int* d_flag = reinterpret_cast<int*>(d + o_flag);
        hipLaunchKernelGGL(bag_ls_gram_jobs_kernel, dim3((unsigned)(nk * nchunk)), dim3(SCORE_THREADS), 0, c->stream, bs, (long long)L,
                           (int)nchunk, d + o_g);
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(bag_ls_inverse_jobs_kernel, dim3((unsigned)nk), dim3(256), spd_inverse_lds_bytes(LS_MAX_H / 16), c->stream, bs,
                           d + o_g, (int)nchunk, d + o_k, d_flag);
        HIPCHK(c, hipGetLastError());
        double* d_x = X ? d + o_x : nullptr;
        double* d_part = r2 ? d + o_part : nullptr;
        const size_t lds = score_ls_lds_bytes((int)Hmax);
        dispatch<MODE_F32, MODE_BF16>(ymode_of(c->mode), [&](auto ym) {
            hipLaunchKernelGGL((bag_ls_jobs_kernel<decltype(ym)::value>), dim3((unsigned)nsl), dim3(SCORE_THREADS), lds, c->stream, c->Y2,
                               c->d2.KS, (long long)L, bs, d + o_k, d_flag, di, jobs, d_x, d_part);
        });
        HIPCHK(c, hipGetLastError());
        if (r2) {
            hipLaunchKernelGGL(bag_resid_fold_kernel, dim3(cdiv(nj, 256)), dim3(256), 0, c->stream, d_part, di + u_sl, (int)nj, d + o_r2);
            HIPCHK(c, hipGetLastError());
        }
        if (X) HIPCHK(c, hipMemcpyAsync(X, d + o_x, (size_t)sumX * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, memcpy_sync(c, res.data(), d + o_r2, res.size() * 8, hipMemcpyDeviceToHost));
        return VBMF_OK;
    }));
    // (the outputs are written whatever the scan below finds: X came back with the one read-back)
    for (int64_t k = 0; k < nk; ++k) {
        int bad = 0;
        std::memcpy(&bad, &res[(size_t)(nj + k)], sizeof(int));
        status[k] = bad ? 1 : 0;
    }
    if (r2) {
        std::memcpy(r2, res.data(), (size_t)nj * 8);
        for (int64_t j = 0; j < nj; ++j)
            if (!std::isfinite(r2[j]) && status[job_basis[j]] == 0)
                FAIL(c, VBMF_ERR_NUMERIC, "%s: non-finite residual in job %lld (bag %lld, basis %lld)", fn, (long long)j, (long long)job_bag[j],
                     (long long)job_basis[j]);
    }
    return VBMF_OK;
}

// What vbmf_sparse_fixed_basis_jobs and vbmf_sparse_scored_jobs share: vbls! of the ARD families (examples/mil_util.jl:187-197) for a
// list of (bag, model) jobs, every model with its own fp64 basis, each job's norm(Y - BHat*AHat')^2 and -- for a scored call -- its bound.
struct VjobsCall {
    const char* fn;
    int64_t nbags; const int64_t* col_off; int64_t niter;
    // per model (packed in model order); model_H nullptr: every model has rank H_all.  CB .. gamma0, delta0, a_pri: a scored call's only
    int64_t nmodels; const int64_t* model_H; int64_t H_all;
    const double* BHat; const double* SigmaB; const double* CB; const double* delta; const double* gamma; const double* gamma0;
    const double* delta0; const double* a_pri; const double* b_pri; const double* a_post; const double* eta0; const double* zeta0;
    const double* sigma0; const double* ca0;
    // per job; job_full_cov nullptr: every job has the form full_all.  job_trim: a scored call's only
    int64_t njobs; const int64_t* job_bag; const int64_t* job_model; const int64_t* job_full_cov; int full_all; const double* job_trim;
    bool scored; int clamp, grouped;
    double* lb; double* r2; double* ATVecHat; double* diagSigmaATVec; double* CA; double* beta; double* SigmaA; double* sigmaHat;
    double* zeta; int64_t* status;
};

// One launch per model, one per non-empty (16-block tier of H_k, form) group of jobs -- at most four, the jobs sorted into them through
// an index table -- and one synchronising read-back, whatever nmodels and njobs are (vbls_jobs_kernels.hpp).  Every refusal comes
// before any launch or copy and leaves every output untouched.
static int vjobs_call(vbmf_ctx* c, const VjobsCall& a) {
    const char* fn = a.fn;
    const int64_t nk = a.nmodels, nj = a.njobs, nb = a.nbags, L = c->L;
    const JobShape js{nb, a.col_off, nk, a.model_H, a.H_all, nj, a.job_bag, a.job_model};
    JobRefusal ref;
    if (job_counts_check(fn, nk, nj, "nmodels", ref)) return jobs_refused(c, ref);
    if (a.niter < 1 || a.niter > (1ll << 30)) FAIL(c, VBMF_ERR_INVALID, "%s: niter must be >= 1", fn);
    if (!a.BHat || !a.SigmaB || !a.b_pri || !a.a_post || !a.eta0 || !a.zeta0 || !a.sigma0 || !a.ca0 || !a.job_bag || !a.job_model || !a.status)
        FAIL(c, VBMF_ERR_INVALID, "%s: null pointer (only the outputs but status may be NULL)", fn);
    if (a.scored && (!a.model_H || !a.CB || !a.delta || !a.gamma || !a.gamma0 || !a.delta0 || !a.a_pri || !a.job_full_cov || !a.job_trim))
        FAIL(c, VBMF_ERR_INVALID, "%s: null pointer (only the outputs but status may be NULL)", fn);
    if (!a.lb && !a.r2 && !a.ATVecHat) FAIL(c, VBMF_ERR_INVALID, "%s: %sr2 and ATVecHat are both NULL", fn, a.scored ? "lb, " : "");
    if (job_grid_check(fn, nk, nj, LS_MAX_GROUPS, ref)) return jobs_refused(c, ref);
    if (c->has_mask) FAIL(c, VBMF_ERR_INVALID, "%s: a label mask is set", fn);
    BagDims bd;
    TRY(bags_check(c, fn, nb, a.col_off, bd));
    const bool compat = (c->o.reference_compat & VBMF_COMPAT_SPARSE_REPEAT) != 0;
    // the jobs' groups (tier of H_k, form): NBK - 1 + 2 * full; per group the widest state kept in LDS (doubles)
    auto full_of = [&](int64_t j) { return (a.job_full_cov ? a.job_full_cov[j] : (int64_t)a.full_all) != 0; };
    auto group_of = [&](int64_t j) { return nb_tier(js.H(a.job_model[j])) - 1 + (full_of(j) ? 2 : 0); };
    int64_t grp_lds[4] = {0, 0, 0, 0};
    bool spill = false;
    JobSums t;
    if (job_walk(fn, js, VJOBS_MAX_H, t, ref, [&](int64_t j, int64_t, int64_t, int64_t Mb, int64_t H, JobRefusal& r) {
            if (a.job_full_cov && a.job_full_cov[j] != 0 && a.job_full_cov[j] != 1)
                return r.set(JOBS_INVALID, "%s: job_full_cov[%lld] = %lld (0 or 1)", fn, (long long)j, (long long)a.job_full_cov[j]);
            const bool full = full_of(j);
            if (!full && compat && Mb < 2)
                return r.set(JOBS_INVALID, "%s: job %lld works on a 1-column bag: the diagonal form under VBMF_COMPAT_SPARSE_REPEAT needs M >= 2",
                             fn, (long long)j);
            if (a.scored && !std::isfinite(a.job_trim[j])) return r.set(JOBS_INVALID, "%s: job_trim[%lld] is not finite", fn, (long long)j);
            const int gi = group_of(j);
            if (vjobs_in_lds(full, nb_tier(H), (int)H, Mb)) grp_lds[gi] = std::max(grp_lds[gi], 4 * Mb * H);
            else spill = true;
            return (int)JOBS_OK;
        }))
        return jobs_refused(c, ref);
    const int64_t sumH = t.sumH, sumH2 = t.sumH2, SMH = t.SMH, SJH = t.SJH, SJH2 = t.SJH2;
    {
        auto per_col = [&](int64_t k) { return js.H(k); };
        auto per_model = [](int64_t) { return (int64_t)1; };
        TRY(jobs_finite(c, fn, "BHat", a.BHat, nk, [&](int64_t k) { return L * js.H(k); }));
        TRY(jobs_finite(c, fn, "SigmaB", a.SigmaB, nk, [&](int64_t k) { return js.H(k) * js.H(k); }));
        const struct { const char* name; const double* v; bool per_col; } ins[] = {
            {a.scored ? "a_post" : "alpha", a.a_post, true}, {a.scored ? "b_pri" : "beta0", a.b_pri, true}, {"eta0", a.eta0, false},
            {"zeta0", a.zeta0, false}, {"sigma0", a.sigma0, false}, {"ca0", a.ca0, false}, {"a_pri", a.a_pri, true}, {"CB", a.CB, true},
            {"delta", a.delta, true}, {"gamma", a.gamma, false}, {"gamma0", a.gamma0, false}, {"delta0", a.delta0, false}};
        for (const auto& in : ins) {
            if (!in.v) continue;                                 // (a call without the bound)
            TRY(in.per_col ? jobs_finite(c, fn, in.name, in.v, nk, per_col) : jobs_finite(c, fn, in.name, in.v, nk, per_model));
        }
    }
    if (!c->cache.have_Y()) FAIL(c, VBMF_ERR_INVALID, "%s: no Y: call vbmf_set_Y first", fn);     // (no state needed: the bases are arguments)
    const int64_t nsc = a.scored ? 1 : 0;
    // the upload, one block: [the job table (job_tables.hpp) | trim nj | a_post | b_pri | CB | delta (sum H each) | eta0 | zeta0 | sigma0 |
    //                         ca0 (nk each) | the bases, column-major L x H_k | SigmaB (H_k^2 each)]; trim, CB, delta: a scored call's only
    const JobTable u(nb, nk, nj);
    const int64_t u_trim = u.words, u_al = u_trim + nsc * nj, u_b0 = u_al + sumH, u_cb = u_b0 + sumH, u_de = u_cb + nsc * sumH,
                  u_eta = u_de + nsc * sumH, u_z0 = u_eta + nk, u_sig = u_z0 + nk, u_ca0 = u_sig + nk, u_b = u_ca0 + nk, u_sb = u_b + L * sumH,
                  n_up = u_sb + sumH2;
    // behind it: [Bt L sum H | G sum H^2 | gd | sd (sum H) | r2 | sigma | zeta | status (nj each) | quad 2 nj | the bases' sums VJOBS_NB nk
    //             | SigmaA (the jobs' H_k^2) | the bound's column sums (SCORE_NS per job and column) | CA | A | dS | beta (the jobs'
    //             M_b H_k-long blocks in job order) | P of the jobs whose state is not in LDS]; [r2 .. beta] is the read-back
    const int64_t o_bt = n_up, o_g = o_bt + L * sumH, o_gd = o_g + sumH2, o_sd = o_gd + sumH, o_r2 = o_sd + sumH, o_sig = o_r2 + nj,
                  o_zeta = o_sig + nj, o_st = o_zeta + nj, o_quad = o_st + nj, o_nb = o_quad + nsc * 2 * nj, o_sa = o_nb + nsc * VJOBS_NB * nk,
                  o_sums = o_sa + SJH2, o_ca = o_sums + nsc * SCORE_NS * SJH, o_a = o_ca + SMH, o_ds = o_a + SMH, o_be = o_ds + SMH,
                  o_p = o_be + SMH, total = o_p + (spill ? SMH : 0);
    std::vector<double> up, res;                                  // (up outlives the copy: an error after it drains the stream)
    TRY(jobs_stage(c, fn, up, n_up, res, o_p - o_r2, (n_up + o_p - o_r2) * 8, "models, job tables and results"));
    int64_t grp_n[4], grp_at[4];                                  // the groups' sizes and first slots of idx
    job_table_fill(reinterpret_cast<long long*>(up.data()), js, L, 4, group_of, grp_n, grp_at);
    if (a.scored) {
        memcpy(up.data() + u_trim, a.job_trim, (size_t)nj * 8);
        memcpy(up.data() + u_cb, a.CB, (size_t)sumH * 8);
        memcpy(up.data() + u_de, a.delta, (size_t)sumH * 8);
    }
    memcpy(up.data() + u_al, a.a_post, (size_t)sumH * 8);
    memcpy(up.data() + u_b0, a.b_pri, (size_t)sumH * 8);
    memcpy(up.data() + u_eta, a.eta0, (size_t)nk * 8);
    memcpy(up.data() + u_z0, a.zeta0, (size_t)nk * 8);
    memcpy(up.data() + u_sig, a.sigma0, (size_t)nk * 8);
    memcpy(up.data() + u_ca0, a.ca0, (size_t)nk * 8);
    memcpy(up.data() + u_b, a.BHat, (size_t)(L * sumH) * 8);
    memcpy(up.data() + u_sb, a.SigmaB, (size_t)sumH2 * 8);
    TRY(jobs_run_drained(c, [&]() -> int {
        HIPCHK(c, hipSetDevice(c->o.device));
        double* d = nullptr;
        TRY(bags_reserve(c, total, &d));
        HIPCHK(c, hipMemcpyAsync(d, up.data(), (size_t)n_up * 8, hipMemcpyHostToDevice, c->stream));
        const long long* di = reinterpret_cast<const long long*>(d);
        const VjobsModels ms{di + u.mh, di + u.bo, di + u.ko, di + u.ho};
        hipLaunchKernelGGL(vbls_jobs_model_kernel, dim3((unsigned)nk), dim3(SCORE_THREADS), 0, c->stream, ms, d + u_b, d + u_sb, (long long)L,
                           d + o_bt, d + o_g, d + o_gd, d + o_sd, a.scored ? d + u_cb : nullptr, a.scored ? d + u_de : nullptr,
                           a.scored ? d + o_nb : nullptr);
        HIPCHK(c, hipGetLastError());
        VjobsArgs g{c->Y2, c->d2.KS, (long long)L, di, di + u.bag, di + u.mod, di + u.off, di + u.jsa, di + u.jh, nullptr, ms,
                    (int)a.niter, compat ? 1 : 0,
                    d + o_bt, d + o_g, d + u_sb, d + o_gd, d + o_sd, d + u_al, d + u_b0, d + u_eta, d + u_z0, d + u_sig, d + u_ca0,
                    spill ? d + o_p : nullptr, d + o_ca, d + o_a, d + o_ds, d + o_be, d + o_sa, d + o_sig, d + o_zeta, d + o_r2,
                    reinterpret_cast<long long*>(d + o_st), a.scored ? d + u_trim : nullptr, a.scored ? d + o_sums : nullptr,
                    a.scored ? d + o_quad : nullptr};
        for (int gi = 0; gi < 4; ++gi) {
            if (!grp_n[gi]) continue;
            const int NBK = (gi & 1) + 1;
            const bool full = gi >= 2;
            g.idx = di + u.idx + grp_at[gi];
            // (the fixed part does not depend on H up to VJOBS_MAX_H within a tier: H^2 <= VJOBS_STAGE)
            const size_t lds = (size_t)(vjobs_fixed_doubles(full, NBK, 16 * NBK) + grp_lds[gi]) * 8;
            dispatch<MODE_F32, MODE_BF16>(ymode_of(c->mode), [&](auto ym) {
                dispatch<1, 2>(NBK, [&](auto nbk) {
                    dispatch<0, 1>(full ? 1 : 0, [&](auto fc) {
                        hipLaunchKernelGGL((vbls_jobs_kernel<decltype(ym)::value, decltype(nbk)::value, decltype(fc)::value != 0>),
                                           dim3((unsigned)grp_n[gi]), dim3(SBATCH_THREADS), lds, c->stream, g);
                    });
                });
            });
            HIPCHK(c, hipGetLastError());
        }
        HIPCHK(c, memcpy_sync(c, res.data(), d + o_r2, res.size() * 8, hipMemcpyDeviceToHost));
        return VBMF_OK;
    }));
    auto at = [&](int64_t o_x) { return res.data() + (o_x - o_r2); };   // block x of the read-back
    int64_t* st = reinterpret_cast<int64_t*>(at(o_st));
    if (a.lb) {
        // the bound of every job from its sums (lb_of_bag); a job whose bound or sums are not finite fails like one the device flagged
        const double nan = std::nan("");
        const long long* ui = reinterpret_cast<const long long*>(up.data());
        LbGroup grp[VJOBS_MAX_H];
        for (int64_t j = 0; j < nj; ++j) {
            const int64_t b = a.job_bag[j], k = a.job_model[j], H = js.H(k), ho = ui[u.ho + k], off = ui[u.off + j], sa = ui[u.jsa + j];
            const double Mb = (double)js.width(b);
            const int64_t n = js.width(b) * H;
            double v = nan;
            if (st[j] == 0) {
                const double* mb = at(o_nb) + VJOBS_NB * k;
                LbSums s{};
                s.L = (double)L; s.H = (double)H;
                s.sig = at(o_sig)[j]; s.zeta = at(o_zeta)[j]; s.eta = a.eta0[k] + 0.5 * (double)L * Mb;
                s.hyp.gamma0 = a.gamma0[k]; s.hyp.delta0 = a.delta0[k]; s.hyp.eta0 = a.eta0[k]; s.hyp.zeta0 = a.zeta0[k];
                s.cbq = mb[0]; s.sumcb = mb[1]; s.sumlogdelta = mb[2]; s.logdet_sb = mb[3]; s.gamma_ = a.gamma[k];
                bool finite = false;
                v = lb_of_bag(s, grp, (int)H, Mb, at(o_r2)[j], at(o_sums) + (size_t)ui[u.jh + j] * SCORE_NS, at(o_quad) + 2 * j,
                              a.job_trim[j] >= 0.0, a.grouped != 0, a.a_pri + ho, a.b_pri + ho, a.a_post + ho, a.clamp, finite);
                if (!finite) {
                    v = nan;
                    st[j] = 1;
                    at(o_r2)[j] = at(o_sig)[j] = at(o_zeta)[j] = nan;
                    std::fill(at(o_sa) + sa, at(o_sa) + sa + H * H, nan);
                    for (const int64_t o_x : {o_ca, o_a, o_ds, o_be}) std::fill(at(o_x) + off, at(o_x) + off + n, nan);
                }
            }
            a.lb[j] = v;
        }
    }
    if (a.r2) memcpy(a.r2, at(o_r2), (size_t)nj * 8);
    if (a.sigmaHat) memcpy(a.sigmaHat, at(o_sig), (size_t)nj * 8);
    if (a.zeta) memcpy(a.zeta, at(o_zeta), (size_t)nj * 8);
    memcpy(a.status, st, (size_t)nj * 8);
    if (a.SigmaA) memcpy(a.SigmaA, at(o_sa), (size_t)SJH2 * 8);     // symmetric: row- and column-major alike
    if (a.CA) memcpy(a.CA, at(o_ca), (size_t)SMH * 8);
    if (a.ATVecHat) memcpy(a.ATVecHat, at(o_a), (size_t)SMH * 8);
    if (a.diagSigmaATVec) memcpy(a.diagSigmaATVec, at(o_ds), (size_t)SMH * 8);
    if (a.beta) memcpy(a.beta, at(o_be), (size_t)SMH * 8);
    return VBMF_OK;
}

// vbls! of the ARD families (examples/mil_util.jl:187-197) for a list of (bag, model) jobs, every model with its own fp64 basis, and
// each job's norm(Y - BHat*AHat')^2 (:518-521) in the same launch: the "dual" classifier of :515-530 for every fold of
// validate_with_cvs at once.  The context supplies Y only.  Two launches (per model, per job) and one synchronising read-back,
// whatever nmodels and njobs are: vjobs_call with one H and one form.
int vbmf_sparse_fixed_basis_jobs(vbmf_ctx* c, int64_t nbags, const int64_t* col_off, int64_t H, int64_t niter, int full_cov,
                                 int64_t nmodels, const double* BHat, const double* SigmaB, const double* alpha, const double* beta0,
                                 const double* eta0, const double* zeta0, const double* sigma0, const double* ca0, int64_t njobs,
                                 const int64_t* job_bag, const int64_t* job_model, double* r2, double* ATVecHat, double* diagSigmaATVec,
                                 double* CA, double* beta, double* SigmaA, double* sigmaHat, double* zeta, int64_t* status) {
    if (!c) return VBMF_ERR_INVALID;
    const char* fn = "vbmf_sparse_fixed_basis_jobs";
    if (H < 1 || H > VJOBS_MAX_H) FAIL(c, VBMF_ERR_UNSUPPORTED, "%s: H = %lld (built for 1 <= H <= %d)", fn, (long long)H, VJOBS_MAX_H);
    VjobsCall a{};
    a.fn = fn; a.nbags = nbags; a.col_off = col_off; a.niter = niter;
    a.nmodels = nmodels; a.H_all = H; a.BHat = BHat; a.SigmaB = SigmaB; a.b_pri = beta0; a.a_post = alpha; a.eta0 = eta0; a.zeta0 = zeta0;
    a.sigma0 = sigma0; a.ca0 = ca0;
    a.njobs = njobs; a.job_bag = job_bag; a.job_model = job_model; a.full_all = full_cov != 0;
    a.r2 = r2; a.ATVecHat = ATVecHat; a.diagSigmaATVec = diagSigmaATVec; a.CA = CA; a.beta = beta; a.SigmaA = SigmaA; a.sigmaHat = sigmaHat;
    a.zeta = zeta; a.status = status;
    return vjobs_call(c, a);
}

// factorize_bag (examples/mil_util.jl:393-416) and the bound of each fit (:502-514) for a list of (bag, model) jobs: the jobs of
// vbmf_sparse_fixed_basis_jobs with a rank per model, a form and a trim per job, and lowerBound / lowerBoundTrimmed of every job
// assembled on the host (lb_assemble) from the sums the job kernel leaves.
int vbmf_sparse_scored_jobs(vbmf_ctx* c, int64_t nbags, const int64_t* col_off, int64_t niter, int clamp, int grouped, int64_t nmodels,
                            const int64_t* model_H, const double* BHat, const double* SigmaB, const double* CB, const double* delta,
                            const double* gamma, const double* gamma0, const double* delta0, const double* a_pri, const double* b_pri,
                            const double* a_post, const double* eta0, const double* zeta0, const double* sigma0, const double* ca0,
                            int64_t njobs, const int64_t* job_bag, const int64_t* job_model, const int64_t* job_full_cov,
                            const double* job_trim, double* lb, double* r2, double* ATVecHat, double* diagSigmaATVec, double* CA,
                            double* beta, double* SigmaA, double* sigmaHat, double* zeta, int64_t* status) {
    if (!c) return VBMF_ERR_INVALID;
    const char* fn = "vbmf_sparse_scored_jobs";
    VjobsCall a{};
    a.fn = fn; a.nbags = nbags; a.col_off = col_off; a.niter = niter;
    a.nmodels = nmodels; a.model_H = model_H; a.BHat = BHat; a.SigmaB = SigmaB; a.CB = CB; a.delta = delta; a.gamma = gamma; a.gamma0 = gamma0;
    a.delta0 = delta0; a.a_pri = a_pri; a.b_pri = b_pri; a.a_post = a_post; a.eta0 = eta0; a.zeta0 = zeta0; a.sigma0 = sigma0; a.ca0 = ca0;
    a.njobs = njobs; a.job_bag = job_bag; a.job_model = job_model; a.job_full_cov = job_full_cov; a.job_trim = job_trim;
    a.scored = true; a.clamp = clamp; a.grouped = grouped;
    a.lb = lb; a.r2 = r2; a.ATVecHat = ATVecHat; a.diagSigmaATVec = diagSigmaATVec; a.CA = CA; a.beta = beta; a.SigmaA = SigmaA;
    a.sigmaHat = sigmaHat; a.zeta = zeta; a.status = status;
    return vjobs_call(c, a);
}

// the widest bag whose job keeps its state in LDS at this H and form (vjobs_in_lds): the tests place a bag on either side of it
int vbmf_debug_vbls_jobs_lds_cols(int64_t H, int full_cov) {
    if (H < 1 || H > VJOBS_MAX_H) return 0;
    int64_t Mb = 0;
    while (vjobs_in_lds(full_cov != 0, nb_tier(H), (int)H, Mb + 1)) ++Mb;
    return (int)Mb;
}

// vbls! of the basic model (examples/mil_util.jl:182-185) for a list of (bag, model) jobs, every model with its own fp64 basis and rank, and
// each job's norm(Y - BHat*AHat')^2: the "vbls" classifier of :469-479 for every fold of validate_with_cvs at once.  The context supplies Y
// only.  One launch per model (vbls_jobs_model_kernel, no bound), one per non-empty 16-block tier of H_k -- at most two, the jobs sorted
// into them through an index table -- and one synchronising read-back, whatever nmodels and njobs are (vbls_basic_jobs_kernels.hpp).
// Every refusal comes before any launch or copy and leaves every output untouched.
int vbmf_fixed_basis_jobs(vbmf_ctx* c, int64_t nbags, const int64_t* col_off, int64_t niter, int64_t nmodels, const int64_t* model_H,
                          const double* BHat, const double* SigmaB, const double* sigma2_0, const double* ca0, int64_t njobs,
                          const int64_t* job_bag, const int64_t* job_model, double* r2, double* AHat, double* SigmaA, double* CA_diag,
                          double* sigma2, int64_t* status) {
    if (!c) return VBMF_ERR_INVALID;
    const char* fn = "vbmf_fixed_basis_jobs";
    const int64_t nk = nmodels, nj = njobs, nb = nbags, L = c->L;
    const JobShape js{nb, col_off, nk, model_H, 0, nj, job_bag, job_model};
    JobRefusal ref;
    if (job_counts_check(fn, nk, nj, "nmodels", ref)) return jobs_refused(c, ref);
    if (niter < 1 || niter > (1ll << 30)) FAIL(c, VBMF_ERR_INVALID, "%s: niter must be >= 1", fn);
    if (!model_H || !BHat || !SigmaB || !sigma2_0 || !ca0 || !job_bag || !job_model || !status)
        FAIL(c, VBMF_ERR_INVALID, "%s: null pointer (only the outputs but status may be NULL)", fn);
    if (!r2 && !AHat) FAIL(c, VBMF_ERR_INVALID, "%s: r2 and AHat are both NULL", fn);
    if (job_grid_check(fn, nk, nj, LS_MAX_GROUPS, ref)) return jobs_refused(c, ref);
    if (c->has_mask) FAIL(c, VBMF_ERR_INVALID, "%s: a label mask is set", fn);
    BagDims bd;
    TRY(bags_check(c, fn, nb, col_off, bd));
    // the jobs' tiers of H_k; per tier the widest P kept in LDS (doubles)
    auto group_of = [&](int64_t j) { return nb_tier(model_H[job_model[j]]) - 1; };
    int64_t grp_lds[2] = {0, 0};
    bool spill = false;
    JobSums t;
    if (job_walk(fn, js, VJOBS_MAX_H, t, ref, [&](int64_t, int64_t, int64_t, int64_t Mb, int64_t H, JobRefusal&) {
            const int gi = nb_tier(H) - 1;
            if (fjobs_in_lds(gi + 1, (int)H, Mb)) grp_lds[gi] = std::max(grp_lds[gi], Mb * H);
            else spill = true;
            return (int)JOBS_OK;
        }))
        return jobs_refused(c, ref);
    const int64_t sumH = t.sumH, sumH2 = t.sumH2, SMH = t.SMH, SJH = t.SJH, SJH2 = t.SJH2;
    auto per_model = [](int64_t) { return (int64_t)1; };
    TRY(jobs_finite(c, fn, "BHat", BHat, nk, [&](int64_t k) { return L * model_H[k]; }));
    TRY(jobs_finite(c, fn, "SigmaB", SigmaB, nk, [&](int64_t k) { return model_H[k] * model_H[k]; }));
    TRY(jobs_finite(c, fn, "sigma2_0", sigma2_0, nk, per_model, false));
    TRY(jobs_finite(c, fn, "ca0", ca0, nk, per_model, false));
    if (!c->cache.have_Y()) FAIL(c, VBMF_ERR_INVALID, "%s: no Y: call vbmf_set_Y first", fn);     // (no state needed: the bases are arguments)
    // the upload, one block: [the job table (job_tables.hpp) | sigma2_0 | ca0 (nk each) | the bases, column-major L x H_k | SigmaB (H_k^2 each)]
    const JobTable u(nb, nk, nj);
    const int64_t u_sig = u.words, u_ca0 = u_sig + nk, u_b = u_ca0 + nk, u_sb = u_b + L * sumH, n_up = u_sb + sumH2;
    // behind it: [Bt L sum H | G sum H^2 | gd | sd (sum H) | r2 | sigma2 | status (nj each) | SigmaA (the jobs' H_k^2) | CA (the jobs' H_k)
    //             | A (the jobs' M_b x H_k blocks in job order) | T (the jobs' H_k^2) | P of the jobs that do not keep it in LDS];
    //             [r2 .. A] is the read-back
    const int64_t o_bt = n_up, o_g = o_bt + L * sumH, o_gd = o_g + sumH2, o_sd = o_gd + sumH, o_r2 = o_sd + sumH, o_sig = o_r2 + nj,
                  o_st = o_sig + nj, o_sa = o_st + nj, o_ca = o_sa + SJH2, o_a = o_ca + SJH, o_t = o_a + SMH, o_p = o_t + SJH2,
                  total = o_p + (spill ? SMH : 0);
    std::vector<double> up, res;                                  // (up outlives the copy: an error after it drains the stream)
    TRY(jobs_stage(c, fn, up, n_up, res, o_t - o_r2, (n_up + o_t - o_r2) * 8, "models, job tables and results"));
    int64_t grp_n[2], grp_at[2];                                  // the tiers' sizes and first slots of idx
    job_table_fill(reinterpret_cast<long long*>(up.data()), js, L, 2, group_of, grp_n, grp_at);
    memcpy(up.data() + u_sig, sigma2_0, (size_t)nk * 8);
    memcpy(up.data() + u_ca0, ca0, (size_t)nk * 8);
    memcpy(up.data() + u_b, BHat, (size_t)(L * sumH) * 8);
    memcpy(up.data() + u_sb, SigmaB, (size_t)sumH2 * 8);
    TRY(jobs_run_drained(c, [&]() -> int {
        HIPCHK(c, hipSetDevice(c->o.device));
        double* d = nullptr;
        TRY(bags_reserve(c, total, &d));
        HIPCHK(c, hipMemcpyAsync(d, up.data(), (size_t)n_up * 8, hipMemcpyHostToDevice, c->stream));
        const long long* di = reinterpret_cast<const long long*>(d);
        const VjobsModels ms{di + u.mh, di + u.bo, di + u.ko, di + u.ho};
        hipLaunchKernelGGL(vbls_jobs_model_kernel, dim3((unsigned)nk), dim3(SCORE_THREADS), 0, c->stream, ms, d + u_b, d + u_sb, (long long)L,
                           d + o_bt, d + o_g, d + o_gd, d + o_sd, (const double*)nullptr, (const double*)nullptr, (double*)nullptr);
        HIPCHK(c, hipGetLastError());
        FjobsArgs g{c->Y2, c->d2.KS, (long long)L, di, di + u.bag, di + u.mod, di + u.off, di + u.jsa, di + u.jh, nullptr, ms, (int)niter,
                    d + o_bt, d + o_g, d + u_sig, d + u_ca0, spill ? d + o_p : nullptr, d + o_a, d + o_sa, d + o_t, d + o_ca, d + o_sig,
                    d + o_r2, reinterpret_cast<long long*>(d + o_st)};
        for (int gi = 0; gi < 2; ++gi) {
            if (!grp_n[gi]) continue;
            g.idx = di + u.idx + grp_at[gi];
            const size_t lds = (size_t)(fjobs_fixed_doubles(gi + 1) + grp_lds[gi]) * 8;
            dispatch<MODE_F32, MODE_BF16>(ymode_of(c->mode), [&](auto ym) {
                dispatch<1, 2>(gi + 1, [&](auto nbk) {
                    hipLaunchKernelGGL((vbls_basic_jobs_kernel<decltype(ym)::value, decltype(nbk)::value>), dim3((unsigned)grp_n[gi]),
                                       dim3(FJOBS_THREADS), lds, c->stream, g);
                });
            });
            HIPCHK(c, hipGetLastError());
        }
        HIPCHK(c, memcpy_sync(c, res.data(), d + o_r2, res.size() * 8, hipMemcpyDeviceToHost));
        return VBMF_OK;
    }));
    auto at = [&](int64_t o_x) { return res.data() + (o_x - o_r2); };   // block x of the read-back
    if (r2) memcpy(r2, at(o_r2), (size_t)nj * 8);
    if (sigma2) memcpy(sigma2, at(o_sig), (size_t)nj * 8);
    memcpy(status, at(o_st), (size_t)nj * 8);
    if (SigmaA) memcpy(SigmaA, at(o_sa), (size_t)SJH2 * 8);       // symmetric: row- and column-major alike
    if (CA_diag) memcpy(CA_diag, at(o_ca), (size_t)SJH * 8);
    if (AHat) memcpy(AHat, at(o_a), (size_t)SMH * 8);
    return VBMF_OK;
}

// the widest bag whose job keeps its P in LDS at this H (fjobs_in_lds): the tests place a bag on either side of it
int vbmf_debug_fixed_basis_jobs_lds_cols(int64_t H) {
    if (H < 1 || H > VJOBS_MAX_H) return 0;
    int64_t Mb = 0;
    while (fjobs_in_lds(nb_tier(H), (int)H, Mb + 1)) ++Mb;
    return (int)Mb;
}

// lowerBound / lowerBoundTrimmed of every bag (examples/mil_util.jl:502-514 after a batched vbls!)
int vbmf_sparse_lower_bound_batched(vbmf_ctx* c, int64_t nbags, const int64_t* col_off, int clamp, double trim, int grouped,
                                    const double* ATVecHat, const double* diagSigmaATVec, const double* CA, const double* beta,
                                    const double* SigmaA, const double* sigmaHat, const double* zeta, const double* eta,
                                    const double* eta0, const double* zeta0, const double* a_pri, const double* b_pri,
                                    const double* a_post, double* lb, double* r2) {
    if (!c) return VBMF_ERR_INVALID;
    const char* fn = "vbmf_sparse_lower_bound_batched";
    if (!c->sparse) FAIL(c, VBMF_ERR_INVALID, "%s: basic context (the sparse models only)", fn);
    BagDims bd;
    TRY(score_check(c, fn, nbags, col_off, bd));
    if (!ATVecHat || !diagSigmaATVec || !CA || !beta || !SigmaA || !sigmaHat || !zeta || !eta || !eta0 || !zeta0 || !a_pri || !b_pri ||
        !a_post || !lb)
        FAIL(c, VBMF_ERR_INVALID, "%s: null pointer (only r2 may be NULL)", fn);
    HIPCHK(c, hipSetDevice(c->o.device));
    TRY(ensure_ready(c));
    TRY(ensure_gram_B(c));
    const int H = (int)c->H;
    const int64_t nb = nbags, ns = bd.nslices, MH = (int64_t)c->M * H, h2 = (int64_t)H * H;
    // c->bags: [col_off nb + 1 | chunk_off nb + 1 | r2 nb | partials ns | A | dS | CA | beta (M H each, vec(A') order) | SigmaA nb H^2
    //           | sums nb H SCORE_NS | quad 2 nb]
    const int64_t o_r2 = 2 * (nb + 1), o_part = o_r2 + nb, o_a = o_part + ns, o_ds = o_a + MH, o_ca = o_ds + MH, o_be = o_ca + MH,
                  o_sa = o_be + MH, o_sums = o_sa + nb * h2, o_quad = o_sums + nb * H * SCORE_NS, total = o_quad + 2 * nb;
    double* d = nullptr;
    TRY(bags_reserve(c, total, &d));
    HIPCHK(c, hipMemcpyAsync(d + o_a, ATVecHat, (size_t)MH * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d + o_ds, diagSigmaATVec, (size_t)MH * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d + o_ca, CA, (size_t)MH * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d + o_be, beta, (size_t)MH * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d + o_sa, SigmaA, (size_t)(nb * h2) * 8, hipMemcpyHostToDevice, c->stream));
    long long* d_off = reinterpret_cast<long long*>(d);
    TRY(score_launch_resid(c, nb, col_off, ns, d_off, d + o_a, (long long)H, 1, d + o_part, d + o_r2));
    hipLaunchKernelGGL(bag_lb_sums_kernel, dim3((unsigned)nb), dim3(SCORE_THREADS), 0, c->stream, d + o_a, d + o_ds, d + o_ca, d + o_be,
                       d + o_sa, c->st, c->lay, H, (double)c->Lg, d_off, trim, d + o_sums, d + o_quad);
    HIPCHK(c, hipGetLastError());
    std::vector<double> res((size_t)nb), sums((size_t)(total - o_sums)), buf((size_t)c->lay.total());
    HIPCHK(c, hipMemcpyAsync(res.data(), d + o_r2, (size_t)nb * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(sums.data(), d + o_sums, sums.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, memcpy_sync(c, buf.data(), c->st, buf.size() * 8, hipMemcpyDeviceToHost));
    LbSums s{};
    lb_basis_sums(c, buf, s);
    const bool trimmed = trim >= 0.0;
    std::vector<LbGroup> grp((size_t)H);
    const double* quad = sums.data() + (o_quad - o_sums);
    for (int64_t b = 0; b < nb; ++b) {
        s.sig = sigmaHat[b]; s.zeta = zeta[b]; s.eta = eta[b];
        s.hyp.eta0 = eta0[b]; s.hyp.zeta0 = zeta0[b];
        bool finite = false;
        const double v = lb_of_bag(s, grp.data(), H, (double)(col_off[b + 1] - col_off[b]), res[(size_t)b], sums.data() + (size_t)b * H * SCORE_NS,
                                   quad + 2 * b, trimmed, grouped != 0, a_pri + b * H, b_pri + b * H, a_post + b * H, clamp, finite);
        if (!finite) FAIL(c, VBMF_ERR_NUMERIC, "%s: non-finite sum in bag %lld", fn, (long long)b);
        lb[b] = v;
        if (r2) r2[b] = res[(size_t)b];
    }
    return VBMF_OK;
}

}  // extern "C"

// ---- many fits in one launch (fit_batch_kernels.hpp) ------------------------------------------------------------------------------
// enqueues fit_stage_kernel: Y as stored into the two fp32 planes
static int fit_stage(vbmf_ctx* c, float* Yr, float* Yc) {
    dispatch<MODE_F32, MODE_BF16>(ymode_of(c->mode), [&](auto ym) {
        hipLaunchKernelGGL((fit_stage_kernel<decltype(ym)::value>), dim3(grid_for(c->L * c->M, 256, 2048)), dim3(256), 0, c->stream, c->Y2, c->d2.KS,
                           (long long)c->L, (long long)c->M, Yr, Yc);
    });
    HIPCHK(c, hipGetLastError());
    return VBMF_OK;
}

// What vbmf_sparse_fit_batched, vbmf_local_fit_batched and vbmf_rows_fit_batched share once each has refused what it refuses about the
// context and the scalar arguments: the per-fit checks, the layout of c->bags, the staging, the one launch and the read-back.
// M0 = nullptr without rows: the two-group sweep with four priors per fit; else the three-group / masked sweep with nine (M0[f] checked
// against the fit's own M_b here).  rows: the row-noise sweep -- sigmaHat and zeta are nfits x L, eta[f] = eta0 + M_b / 2, and
// M0 = nullptr stands for M0[f] = M_b.
static int fit_batched_run(vbmf_ctx* c, const char* fn, int64_t nbags, const int64_t* col_off, int64_t nfits, const int64_t* fit_bag,
                           int64_t niter, double eps, int full_cov, int est_cb, int est_priors, int64_t H0, const int64_t* M0,
                           int64_t mask_H1, const double* gamma, const double* delta0, const double* eta, const double* zeta0,
                           double* priors, double* BHat, double* SigmaB, double* CB, double* sigmaHat, double* CA, double* delta,
                           double* zeta, double* beta, double* diagSigmaATVec, double* SigmaA, double* ATVecHat, int64_t* iters_done,
                           double* d_last, int64_t* status, double* trace, bool rows = false, int64_t slice_cols = 0) {
    const bool local = M0 != nullptr || rows;
    const bool split = slice_cols > 0;                              // (the split schedule is the three-group sweep: its callers pass M0)
    const int64_t npri = local ? 9 : 4;
    const bool compat = (c->o.reference_compat & VBMF_COMPAT_SPARSE_REPEAT) != 0;
    const int H = (int)c->H, NBK = nb_tier(H);
    const int64_t L = c->L, nf = nfits, nb = nbags, h2 = (int64_t)H * H, LH = L * H;
    std::vector<long long> idx((size_t)(nb + 1 + nf + nf + 1 + (local ? nf : 0)));   // col_off | fit_bag | fit_off | M0
    long long* fit_off = idx.data() + nb + 1 + nf;
    fit_off[0] = 0;
    size_t lds_doubles = 0;
    std::vector<long long> sl_fit, sl_c0, fit_sl0;                  // split: the slices (fit_split_kernels.hpp)
    for (int64_t f = 0; f < nf; ++f) {
        const int64_t b = fit_bag[f];
        if (b < 0 || b >= nb) FAIL(c, VBMF_ERR_INVALID, "%s: fit_bag[%lld] = %lld outside 0..nbags-1", fn, (long long)f, (long long)b);
        const int64_t Mb = col_off[b + 1] - col_off[b];
        if (!full_cov && compat && Mb < 2)
            FAIL(c, VBMF_ERR_INVALID, "%s: fit %lld works on a 1-column bag: the diagonal form under VBMF_COMPAT_SPARSE_REPEAT needs M >= 2", fn, (long long)f);
        if (M0 && (M0[f] < 0 || M0[f] > Mb))
            FAIL(c, VBMF_ERR_INVALID, "%s: M0[%lld] = %lld outside 0..M_b = %lld", fn, (long long)f, (long long)M0[f], (long long)Mb);
        fit_off[f + 1] = fit_off[f] + Mb;
        lds_doubles = std::max(lds_doubles, (size_t)fitb_lds_doubles(full_cov != 0, NBK, L, Mb, H, rows));
        idx[(size_t)(nb + 1 + f)] = b;
        if (local) idx[(size_t)(nb + 1 + nf + nf + 1 + f)] = M0 ? M0[f] : Mb;
        if (split) {
            fit_sl0.push_back((long long)sl_fit.size());
            for (int64_t c0 = 0; c0 < Mb; c0 += slice_cols) {
                sl_fit.push_back(f);
                sl_c0.push_back(c0);
            }
        }
    }
    fit_sl0.push_back((long long)sl_fit.size());
    const int64_t nsl = (int64_t)sl_fit.size();
    if (nsl > (1ll << 31) - 1) FAIL(c, VBMF_ERR_UNSUPPORTED, "%s: %lld slices (more than 2^31 - 1 workgroups)", fn, (long long)nsl);
    for (int64_t b = 0; b <= nb; ++b) idx[(size_t)b] = col_off[b];
    if (!c->cache.have_Y()) FAIL(c, VBMF_ERR_INVALID, "%s: no Y: call vbmf_set_Y first", fn);           // (no state needed)
    // the staging vectors outlive every copy: an error between the first asynchronous copy and the synchronise drains the stream below
    std::vector<double> in, out, sg;
    std::vector<long long> done;                                    // split: the fits' done words, read between chunks of sweeps
    auto run = [&]() -> int {
    HIPCHK(c, hipSetDevice(c->o.device));
    const int64_t SMH = fit_off[nf] * H, nidx = (int64_t)idx.size(), ntr = trace ? 2 * nf * niter : 0, ny = (L * c->M + 1) / 2;
    const int64_t nrow = rows ? nf * L : 0;                         // rows: sigmaVec | zetaVec | the row norms, nf L each, behind beta
    // c->bags: [col_off | fit_bag | fit_off | M0 (int64) | gamma | delta0 | eta | zeta0 | sigma (nf each) | priors 4 or 9 nf | zeta | d_last
    //           | iters | status (int64) (nf each) | B | Bw | Qw (nf L H each) | SigmaB | SigmaA (nf H^2) | CB | delta (nf H) | CA | A | dS |
    //           beta (sum M_b H each) | rows: sigmaVec | zetaVec | row norms (nf L each) | trace | Yr | Yc (L M floats each)]
    const int64_t o_sc = nidx, o_pri = o_sc + 5 * nf, o_zeta = o_pri + npri * nf, o_dl = o_zeta + nf, o_it = o_dl + nf, o_st = o_it + nf,
                  o_b = o_st + nf, o_bw = o_b + nf * LH, o_qw = o_bw + nf * LH, o_sb = o_qw + nf * LH, o_sa = o_sb + nf * h2,
                  o_cb = o_sa + nf * h2, o_de = o_cb + nf * H, o_ca = o_de + nf * H, o_a = o_ca + SMH, o_ds = o_a + SMH, o_be = o_ds + SMH,
                  o_sv = o_be + SMH, o_zv = o_sv + nrow, o_yn = o_zv + nrow, o_tr = o_yn + nrow, o_yr = o_tr + ntr, o_yc = o_yr + ny;
    // split: [sl_fit | sl_c0 (nsl) | fit_sl0 (nf + 1) | done (nf) (int64) | the fits' published blocks | the slices' slots] behind Yc
    const int64_t o_sl = o_yc + ny, o_done = o_sl + (split ? 2 * nsl + nf + 1 : 0), o_pub = o_done + (split ? nf : 0),
                  o_slot = o_pub + (split ? nf * fits_pub_doubles(H) : 0), total = o_slot + (split ? nsl * fits_slot_doubles(L, H) : 0);
    double* d = nullptr;
    TRY(bags_reserve(c, total, &d));
    in.resize((size_t)((5 + npri) * nf));
    memcpy(in.data(), gamma, (size_t)nf * 8);
    memcpy(in.data() + nf, delta0, (size_t)nf * 8);
    memcpy(in.data() + 2 * nf, eta, (size_t)nf * 8);
    memcpy(in.data() + 3 * nf, zeta0, (size_t)nf * 8);
    if (!rows) memcpy(in.data() + 4 * nf, sigmaHat, (size_t)nf * 8);
    memcpy(in.data() + 5 * nf, priors, (size_t)(nf * npri) * 8);
    HIPCHK(c, hipMemcpyAsync(d, idx.data(), (size_t)nidx * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d + o_sc, in.data(), in.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d + o_b, BHat, (size_t)(nf * LH) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d + o_sb, SigmaB, (size_t)(nf * h2) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d + o_cb, CB, (size_t)(nf * H) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d + o_ca, CA, (size_t)SMH * 8, hipMemcpyHostToDevice, c->stream));
    if (rows) HIPCHK(c, hipMemcpyAsync(d + o_sv, sigmaHat, (size_t)nrow * 8, hipMemcpyHostToDevice, c->stream));
    if (ntr) HIPCHK(c, hipMemsetAsync(d + o_tr, 0, (size_t)ntr * 8, c->stream));
    float* Yr = reinterpret_cast<float*>(d + o_yr);
    float* Yc = reinterpret_cast<float*>(d + o_yc);
    TRY(fit_stage(c, Yr, Yc));
    long long* di = reinterpret_cast<long long*>(d);
    FitArgs a{Yr, Yc, (long long)L, (long long)c->M, di, di + nb + 1, di + nb + 1 + nf, H, (int)H0, (int)niter, compat ? 1 : 0,
              (c->o.reference_compat & VBMF_COMPAT_SPECTRAL_DELTA) ? 1 : 0, est_cb ? 1 : 0, est_priors ? 1 : 0, eps,
              d + o_sc, d + o_sc + nf, d + o_sc + 2 * nf, d + o_sc + 3 * nf, d + o_pri,
              d + o_b, d + o_sb, d + o_cb, rows ? d + o_sv : d + o_sc + 4 * nf, d + o_ca,
              d + o_de, rows ? d + o_zv : d + o_zeta, d + o_be, d + o_ds, d + o_sa, d + o_a, d + o_bw, d + o_qw,
              reinterpret_cast<long long*>(d + o_it), d + o_dl, reinterpret_cast<long long*>(d + o_st), trace ? d + o_tr : nullptr};
    const size_t lds = lds_doubles * 8;
    // (the fit kernels exist for NB = 1 and 2: every rank above 16 runs the NB = 2 instance)
    const FitLocalArgs la{a, di + nb + 1 + nf + nf + 1, (int)mask_H1};
    const FitRowsArgs ra{la, d + o_yn};
    if (split) {
        // a sweep = the column pass over every slice + the fold per fit; the host reads the done words between chunks of sweeps
        sl_fit.insert(sl_fit.end(), sl_c0.begin(), sl_c0.end());
        sl_fit.insert(sl_fit.end(), fit_sl0.begin(), fit_sl0.end());
        HIPCHK(c, hipMemcpyAsync(d + o_sl, sl_fit.data(), sl_fit.size() * 8, hipMemcpyHostToDevice, c->stream));
        const int NB2 = std::min(NBK, 2);
        long long* dsl = reinterpret_cast<long long*>(d + o_sl);
        const bool x_lds = fits_cols_x_lds(full_cov != 0, NB2, L, H, slice_cols), b_lds = fits_fold_b_lds(NB2, L, H);
        const FitSplitArgs sa{ra, dsl, dsl + nsl, dsl + 2 * nsl, (int)slice_cols, full_cov ? 1 : 0, x_lds ? 1 : 0, b_lds ? 1 : 0,
                              d + o_pub, d + o_slot, reinterpret_cast<long long*>(d + o_done)};
        const size_t lds_i = (size_t)6 * h2 * 8,
                     lds_c = (size_t)(fits_cols_min_doubles(full_cov != 0, NB2, H, slice_cols) + (x_lds ? LH : 0)) * 8,
                     lds_f = (size_t)(fits_fold_fixed_doubles(NB2, H) + (b_lds ? 2 * LH : 0)) * 8;
        if (rows) hipLaunchKernelGGL((fit_split_init_kernel<true>), dim3((unsigned)nf), dim3(FITB_THREADS), lds_i, c->stream, sa);
        else hipLaunchKernelGGL((fit_split_init_kernel<false>), dim3((unsigned)nf), dim3(FITB_THREADS), lds_i, c->stream, sa);
        HIPCHK(c, hipGetLastError());
        done.resize((size_t)nf);
        int64_t chunk_len = VBMF_FIT_SPLIT_CHUNK;
        if (const char* e = getenv("VBMF_FIT_SPLIT_CHUNK")) {       // tuning switch (include/vbmf_hip.h)
            if (atoll(e) >= 1 && atoll(e) <= (1 << 16)) chunk_len = atoll(e);
        }
        for (int64_t enq = 0; enq < niter;) {
            const int64_t chunk = std::min<int64_t>(chunk_len, niter - enq);
            for (int64_t k = 0; k < chunk; ++k)
                dispatch<1, 2>(NB2, [&](auto nbk) {
                    dispatch<0, 1>(rows ? 1 : 0, [&](auto rw) {
                        constexpr int NBc = decltype(nbk)::value;
                        constexpr bool ROWSc = decltype(rw)::value != 0;
                        if (full_cov) hipLaunchKernelGGL((fit_cols_kernel<NBc, true, ROWSc>), dim3((unsigned)nsl), dim3(FITB_THREADS), lds_c, c->stream, sa);
                        else hipLaunchKernelGGL((fit_cols_kernel<NBc, false, ROWSc>), dim3((unsigned)nsl), dim3(FITB_THREADS), lds_c, c->stream, sa);
                        hipLaunchKernelGGL((fit_fold_kernel<NBc, ROWSc>), dim3((unsigned)nf), dim3(FITB_THREADS), lds_f, c->stream, sa);
                    });
                });
            HIPCHK(c, hipGetLastError());
            enq += chunk;
            if (enq >= niter) break;
            HIPCHK(c, hipMemcpyAsync(done.data(), d + o_done, (size_t)nf * 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (std::all_of(done.begin(), done.end(), [](long long x) { return x != 0; })) break;
        }
    } else
    dispatch<1, 2>(std::min(NBK, 2), [&](auto nbk) {
        dispatch<0, 1>(full_cov ? 1 : 0, [&](auto full) {
            constexpr int NBc = decltype(nbk)::value;
            constexpr bool FULLc = decltype(full)::value != 0;
            if (rows) hipLaunchKernelGGL((fit_batch_kernel<NBc, FULLc, true, true>), dim3((unsigned)nf), dim3(FITB_THREADS), lds, c->stream, ra);
            else if (local) hipLaunchKernelGGL((fit_batch_kernel<NBc, FULLc, true>), dim3((unsigned)nf), dim3(FITB_THREADS), lds, c->stream, la);
            else hipLaunchKernelGGL((fit_batch_kernel<NBc, FULLc>), dim3((unsigned)nf), dim3(FITB_THREADS), lds, c->stream, a);
        });
    });
    HIPCHK(c, hipGetLastError());
    // read-back: [priors | zeta | d_last | iters | status] is one block; the per-fit matrices and the M H-long fields one block each
    out.resize((size_t)(o_b - o_pri));
    sg.resize((size_t)nf);
    HIPCHK(c, hipMemcpyAsync(out.data(), d + o_pri, out.size() * 8, hipMemcpyDeviceToHost, c->stream));
    if (rows) {
        HIPCHK(c, hipMemcpyAsync(sigmaHat, d + o_sv, (size_t)nrow * 8, hipMemcpyDeviceToHost, c->stream));
        if (zeta) HIPCHK(c, hipMemcpyAsync(zeta, d + o_zv, (size_t)nrow * 8, hipMemcpyDeviceToHost, c->stream));
    } else {
        HIPCHK(c, hipMemcpyAsync(sg.data(), d + o_sc + 4 * nf, (size_t)nf * 8, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(BHat, d + o_b, (size_t)(nf * LH) * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(SigmaB, d + o_sb, (size_t)(nf * h2) * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(CB, d + o_cb, (size_t)(nf * H) * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(CA, d + o_ca, (size_t)SMH * 8, hipMemcpyDeviceToHost, c->stream));
    if (delta && est_cb) HIPCHK(c, hipMemcpyAsync(delta, d + o_de, (size_t)(nf * H) * 8, hipMemcpyDeviceToHost, c->stream));
    if (SigmaA) HIPCHK(c, hipMemcpyAsync(SigmaA, d + o_sa, (size_t)(nf * h2) * 8, hipMemcpyDeviceToHost, c->stream));
    if (ATVecHat) HIPCHK(c, hipMemcpyAsync(ATVecHat, d + o_a, (size_t)SMH * 8, hipMemcpyDeviceToHost, c->stream));
    if (diagSigmaATVec) HIPCHK(c, hipMemcpyAsync(diagSigmaATVec, d + o_ds, (size_t)SMH * 8, hipMemcpyDeviceToHost, c->stream));
    if (beta) HIPCHK(c, hipMemcpyAsync(beta, d + o_be, (size_t)SMH * 8, hipMemcpyDeviceToHost, c->stream));
    if (trace) HIPCHK(c, hipMemcpyAsync(trace, d + o_tr, (size_t)ntr * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    memcpy(priors, out.data(), (size_t)(nf * npri) * 8);
    if (zeta && !rows) memcpy(zeta, out.data() + (o_zeta - o_pri), (size_t)nf * 8);
    memcpy(d_last, out.data() + (o_dl - o_pri), (size_t)nf * 8);
    memcpy(iters_done, out.data() + (o_it - o_pri), (size_t)nf * 8);
    memcpy(status, out.data() + (o_st - o_pri), (size_t)nf * 8);
    if (!rows) memcpy(sigmaHat, sg.data(), (size_t)nf * 8);
    return VBMF_OK;
    };
    const int rc = run();
    if (rc != VBMF_OK) hipStreamSynchronize(c->stream);
    return rc;
}

extern "C" {

// The restart loops of examples/mil_util.jl:124-145,347-379 (and the folds x classes around them) in one call: every fit's whole
// vbmf_sparse! / vbmf_dual! loop in one workgroup of one launch.  The context supplies Y only; its state is neither read nor changed,
// so no RunFrame: that frame settles the context's own B buffers and counters, which this call leaves alone.
int vbmf_sparse_fit_batched(vbmf_ctx* c, int64_t nbags, const int64_t* col_off, int64_t nfits, const int64_t* fit_bag, int64_t niter,
                            double eps, int full_cov, int est_cb, int est_priors, int64_t H0, const double* gamma, const double* delta0,
                            const double* eta, const double* zeta0, double* priors4, double* BHat, double* SigmaB, double* CB,
                            double* sigmaHat, double* CA, double* delta, double* zeta, double* beta, double* diagSigmaATVec,
                            double* SigmaA, double* ATVecHat, int64_t* iters_done, double* d_last, int64_t* status, double* trace) {
    if (!c) return VBMF_ERR_INVALID;
    const char* fn = "vbmf_sparse_fit_batched";
    if (c->H > 32) FAIL(c, VBMF_ERR_UNSUPPORTED, "%s: H = %lld (built for H <= 32)", fn, (long long)c->H);
    if (!c->sparse) FAIL(c, VBMF_ERR_INVALID, "%s: basic context (the sparse and two-group models only)", fn);
    if (c->diagvar) FAIL(c, VBMF_ERR_INVALID, "%s: diag_var context (homoscedastic only; use vbmf_rows_fit_batched, or vbmf_sparse_run / vbmf_dual_run per fit)", fn);
    if (c->trial) FAIL(c, VBMF_ERR_INVALID, "%s: trial context (the sparse and two-group models only)", fn);
    if (c->has_mask) FAIL(c, VBMF_ERR_INVALID, "%s: a label mask is set (use vbmf_sparse_run per fit)", fn);
    BagDims bd;
    TRY(bags_check(c, fn, nbags, col_off, bd));
    if (nfits < 1 || nfits > (1ll << 20)) FAIL(c, VBMF_ERR_INVALID, "%s: nfits must be >= 1", fn);
    if (niter < 1 || niter > (1ll << 24)) FAIL(c, VBMF_ERR_INVALID, "%s: niter must be >= 1", fn);
    if (H0 < 1 || H0 > c->H) FAIL(c, VBMF_ERR_INVALID, "%s: H0 = %lld outside 1..H = %lld", fn, (long long)H0, (long long)c->H);
    if (!fit_bag || !gamma || !delta0 || !eta || !zeta0 || !priors4 || !BHat || !SigmaB || !CB || !sigmaHat || !CA || !iters_done ||
        !d_last || !status)
        FAIL(c, VBMF_ERR_INVALID, "%s: null pointer (only delta, zeta, beta, diagSigmaATVec, SigmaA, ATVecHat and trace may be NULL)", fn);
    return fit_batched_run(c, fn, nbags, col_off, nfits, fit_bag, niter, eps, full_cov, est_cb, est_priors, H0, nullptr, 0, gamma, delta0,
                           eta, zeta0, priors4, BHat, SigmaB, CB, sigmaHat, CA, delta, zeta, beta, diagSigmaATVec, SigmaA, ATVecHat,
                           iters_done, d_last, status, trace);
}

}  // extern "C"

// What vbmf_local_fit_batched and vbmf_rows_fit_batched refuse alike before fit_batched_run's per-fit checks.  rows: a *_DIAGVAR context
// serves as well (only its Y is used), and M0 may be NULL (M0[f] = M_b).
static int local_fit_checks(vbmf_ctx* c, const char* fn, bool rows, int64_t nbags, const int64_t* col_off, int64_t nfits, int64_t niter,
                            int est_priors, int64_t H0, int64_t mask_H1, bool null_required) {
    if (c->H > 32) FAIL(c, VBMF_ERR_UNSUPPORTED, "%s: H = %lld (built for H <= 32)", fn, (long long)c->H);
    if (!c->sparse) FAIL(c, VBMF_ERR_INVALID, "%s: basic context (the sparse, two-group and three-group models only)", fn);
    if (c->diagvar && !rows)
        FAIL(c, VBMF_ERR_INVALID, "%s: diag_var context (homoscedastic only; use vbmf_rows_fit_batched, or vbmf_trial_run / vbmf_sparse_run per fit)", fn);
    if (c->has_mask) FAIL(c, VBMF_ERR_INVALID, "%s: a label mask is set on the context (the call's own M0 / mask_H1 describe the mask)", fn);
    BagDims bd;
    TRY(bags_check(c, fn, nbags, col_off, bd));
    if (nfits < 1 || nfits > (1ll << 20)) FAIL(c, VBMF_ERR_INVALID, "%s: nfits must be >= 1", fn);
    if (niter < 1 || niter > (1ll << 24)) FAIL(c, VBMF_ERR_INVALID, "%s: niter must be >= 1", fn);
    if (H0 < 0 || H0 > c->H) FAIL(c, VBMF_ERR_INVALID, "%s: H0 = %lld outside 0..H = %lld", fn, (long long)H0, (long long)c->H);
    if (mask_H1 < 0 || mask_H1 > c->H) FAIL(c, VBMF_ERR_INVALID, "%s: mask_H1 = %lld outside 0..H = %lld", fn, (long long)mask_H1, (long long)c->H);
    if (mask_H1 > 0 && (H0 != c->H || est_priors))
        FAIL(c, VBMF_ERR_INVALID, "%s: mask_H1 > 0 needs H0 = H and est_priors = 0 (the masked model has one prior group and no hyper-prior fit)", fn);
    if (null_required)
        FAIL(c, VBMF_ERR_INVALID, "%s: null pointer (only %sdelta, %s, beta, diagSigmaATVec, SigmaA, ATVecHat and trace may be NULL)", fn,
             rows ? "M0, " : "", rows ? "zetaVec" : "zeta");
    return VBMF_OK;
}

extern "C" {

// The three-group fit (vbmf_trial!, src/vbmf_trial.jl:528-604) and the label-masked sparse fit (train_local, examples/mil_util.jl:302-320)
// of many [Y0 Y1] matrices in one call: vbmf_sparse_fit_batched's launch with a per-fit M0 and the two per-entry rules of FitLocalArgs.
int vbmf_local_fit_batched(vbmf_ctx* c, int64_t nbags, const int64_t* col_off, int64_t nfits, const int64_t* fit_bag, int64_t niter,
                           double eps, int full_cov, int est_cb, int est_priors, int64_t H0, const int64_t* M0, int64_t mask_H1,
                           const double* gamma, const double* delta0, const double* eta, const double* zeta0, double* priors9,
                           double* BHat, double* SigmaB, double* CB, double* sigmaHat, double* CA, double* delta, double* zeta,
                           double* beta, double* diagSigmaATVec, double* SigmaA, double* ATVecHat, int64_t* iters_done, double* d_last,
                           int64_t* status, double* trace) {
    if (!c) return VBMF_ERR_INVALID;
    const char* fn = "vbmf_local_fit_batched";
    TRY(local_fit_checks(c, fn, false, nbags, col_off, nfits, niter, est_priors, H0, mask_H1,
                         !fit_bag || !M0 || !gamma || !delta0 || !eta || !zeta0 || !priors9 || !BHat || !SigmaB || !CB || !sigmaHat || !CA ||
                             !iters_done || !d_last || !status));
    return fit_batched_run(c, fn, nbags, col_off, nfits, fit_bag, niter, eps, full_cov, est_cb, est_priors, H0, M0, mask_H1, gamma, delta0,
                           eta, zeta0, priors9, BHat, SigmaB, CB, sigmaHat, CA, delta, zeta, beta, diagSigmaATVec, SigmaA, ATVecHat,
                           iters_done, d_last, status, trace);
}

// The same fits under the heteroscedastic noise model, diag_var = true (examples/mil_util.jl:667 sets it for train, train_local and
// train_dual): one noise precision per row of Y.  src/vbmf_sparse.jl:180-193 (updateA!, full_cov: s to the first power), :207-230
// (updateA!, diagonal: v_h = sum_l (s_l B_lh)^2 + L mean(s) SigmaB_hh -- s enters SQUARED, the reference takes norm2 of the product),
// :256-261 (updateB!), :309-315 (updateSigma!, row by row; sigmaHat and zeta are not touched); src/vbmf_dual.jl:222-299,370-386 and
// src/vbmf_trial.jl:256-334,419-435 are the same.  One kernel family serves the sparse (H0 = H, est_priors = 0), two-group
// (M0 = NULL: M0[f] = M_b), three-group and masked fits.  The context supplies Y only: a *_DIAG or a *_DIAGVAR context serves alike.
int vbmf_rows_fit_batched(vbmf_ctx* c, int64_t nbags, const int64_t* col_off, int64_t nfits, const int64_t* fit_bag, int64_t niter,
                          double eps, int full_cov, int est_cb, int est_priors, int64_t H0, const int64_t* M0, int64_t mask_H1,
                          const double* gamma, const double* delta0, const double* etaVec, const double* zeta0, double* priors9,
                          double* BHat, double* SigmaB, double* CB, double* sigmaVec, double* CA, double* delta, double* zetaVec,
                          double* beta, double* diagSigmaATVec, double* SigmaA, double* ATVecHat, int64_t* iters_done, double* d_last,
                          int64_t* status, double* trace) {
    if (!c) return VBMF_ERR_INVALID;
    const char* fn = "vbmf_rows_fit_batched";
    TRY(local_fit_checks(c, fn, true, nbags, col_off, nfits, niter, est_priors, H0, mask_H1,
                         !fit_bag || !gamma || !delta0 || !etaVec || !zeta0 || !priors9 || !BHat || !SigmaB || !CB || !sigmaVec || !CA ||
                             !iters_done || !d_last || !status));
    return fit_batched_run(c, fn, nbags, col_off, nfits, fit_bag, niter, eps, full_cov, est_cb, est_priors, H0, M0, mask_H1, gamma, delta0,
                           etaVec, zeta0, priors9, BHat, SigmaB, CB, sigmaVec, CA, delta, zetaVec, beta, diagSigmaATVec, SigmaA, ATVecHat,
                           iters_done, d_last, status, trace, true);
}

// vbmf_ard_fit_batched_form: the same fits with the form chosen per call or per fit.  form = 0 is the entry above (rows) or
// vbmf_local_fit_batched (M0 = NULL: M0[f] = M_b) unchanged; form = 3 runs every fit in the split schedule of fit_split_kernels.hpp;
// form = 2 picks per fit by (M_b, full_cov) alone and runs the two groups one after the other, each on its own compact copy of the
// per-fit arguments (a call whose fits all take one form runs on the caller's arrays).
int vbmf_ard_fit_batched_form(vbmf_ctx* c, int64_t nbags, const int64_t* col_off, int64_t nfits, const int64_t* fit_bag, int64_t niter,
                              double eps, int full_cov, int est_cb, int est_priors, int64_t H0, const int64_t* M0, int64_t mask_H1,
                              const double* gamma, const double* delta0, const double* etaVec, const double* zeta0, double* priors9,
                              double* BHat, double* SigmaB, double* CB, double* sigmaVec, double* CA, double* delta, double* zetaVec,
                              double* beta, double* diagSigmaATVec, double* SigmaA, double* ATVecHat, int64_t* iters_done, double* d_last,
                              int64_t* status, double* trace, int diag_var, int64_t form, int64_t slice_cols, int64_t* form_used) {
    if (!c) return VBMF_ERR_INVALID;
    const char* fn = "vbmf_ard_fit_batched_form";
    const bool rows = diag_var != 0;
    TRY(local_fit_checks(c, fn, rows, nbags, col_off, nfits, niter, est_priors, H0, mask_H1,
                         !fit_bag || !gamma || !delta0 || !etaVec || !zeta0 || !priors9 || !BHat || !SigmaB || !CB || !sigmaVec || !CA ||
                             !iters_done || !d_last || !status));
    if (form == VBMF_FIT_FORM_GRAM)
        FAIL(c, VBMF_ERR_UNSUPPORTED, "%s: form = 1: the ARD families have no Gram form (the element-wise precision on A breaks A = Y'V)", fn);
    if (form != VBMF_FIT_FORM_STREAM && form != VBMF_FIT_FORM_AUTO && form != VBMF_FIT_FORM_SPLIT)
        FAIL(c, VBMF_ERR_INVALID, "%s: form = %lld (0 = stream, 2 = auto, 3 = split)", fn, (long long)form);
    if (slice_cols != 0 && (slice_cols < 8 || slice_cols % 8 != 0 || slice_cols > (1ll << 30)))
        FAIL(c, VBMF_ERR_INVALID, "%s: slice_cols = %lld (0, or a multiple of 8)", fn, (long long)slice_cols);
    const int H = (int)c->H, NB2 = std::min(nb_tier(H), 2);
    int64_t sc = slice_cols ? slice_cols : VBMF_FIT_SPLIT_COLS;
    const bool sc_fits = fits_cols_min_doubles(full_cov != 0, NB2, H, sc) <= (long long)(FITB_LDS_CAP / 8);
    if (!sc_fits && slice_cols == 0) {                              // the default width, narrowed to what a slice's state leaves of LDS
        sc = ((long long)(FITB_LDS_CAP / 8) - fits_cols_min_doubles(full_cov != 0, NB2, H, 0)) / (3 * H) / 8 * 8;
    } else if (!sc_fits && form != VBMF_FIT_FORM_STREAM) {
        FAIL(c, VBMF_ERR_UNSUPPORTED, "%s: slice_cols = %lld at H = %d: a slice's state (3 slice_cols H doubles) does not fit in LDS", fn,
             (long long)slice_cols, H);
    }
    const int64_t nf = nfits, nb = nbags;
    std::vector<int64_t> M0v, Mbs((size_t)nf), used((size_t)nf);
    int64_t nsplit = 0;
    for (int64_t f = 0; f < nf; ++f) {
        const int64_t b = fit_bag[f];
        if (b < 0 || b >= nb) FAIL(c, VBMF_ERR_INVALID, "%s: fit_bag[%lld] = %lld outside 0..nbags-1", fn, (long long)f, (long long)b);
        const int64_t Mb = Mbs[(size_t)f] = col_off[b + 1] - col_off[b];
        // fit_batched_run's per-fit refusals, made here on the caller's own indices before either group of a mixed call runs
        if (!full_cov && (c->o.reference_compat & VBMF_COMPAT_SPARSE_REPEAT) && Mb < 2)
            FAIL(c, VBMF_ERR_INVALID, "%s: fit %lld works on a 1-column bag: the diagonal form under VBMF_COMPAT_SPARSE_REPEAT needs M >= 2", fn, (long long)f);
        if (M0 && (M0[f] < 0 || M0[f] > Mb))
            FAIL(c, VBMF_ERR_INVALID, "%s: M0[%lld] = %lld outside 0..M_b = %lld", fn, (long long)f, (long long)M0[f], (long long)Mb);
        used[(size_t)f] = form == VBMF_FIT_FORM_SPLIT ||
                                  (form == VBMF_FIT_FORM_AUTO && Mbs[(size_t)f] >= (full_cov ? VBMF_FIT_SPLIT_MIN_COLS_FULL : VBMF_FIT_SPLIT_MIN_COLS))
                              ? VBMF_FIT_FORM_SPLIT : VBMF_FIT_FORM_STREAM;
        nsplit += used[(size_t)f] != 0;
    }
    if (!c->cache.have_Y()) FAIL(c, VBMF_ERR_INVALID, "%s: no Y: call vbmf_set_Y first", fn);
    if (!M0 && !rows) {                                             // the homoscedastic sweeps take M0 per fit: M0[f] = M_b
        M0v = Mbs;
        M0 = M0v.data();
    }
    auto run = [&](bool split, int64_t nfr, const int64_t* fb, const int64_t* m0, const double* ga, const double* de0, const double* et,
                   const double* ze0, double* pri, double* B, double* SB, double* cb, double* sg, double* ca, double* de, double* ze,
                   double* be, double* ds, double* SA, double* A, int64_t* itd, double* dl, int64_t* stt, double* tr) {
        return fit_batched_run(c, fn, nbags, col_off, nfr, fb, niter, eps, full_cov, est_cb, est_priors, H0, m0, mask_H1, ga, de0, et, ze0,
                               pri, B, SB, cb, sg, ca, de, ze, be, ds, SA, A, itd, dl, stt, tr, rows, split ? sc : 0);
    };
    if (nsplit == 0 || nsplit == nf) {
        TRY(run(nsplit != 0, nf, fit_bag, M0, gamma, delta0, etaVec, zeta0, priors9, BHat, SigmaB, CB, sigmaVec, CA, delta, zetaVec, beta,
                diagSigmaATVec, SigmaA, ATVecHat, iters_done, d_last, status, trace));
        if (form_used) memcpy(form_used, used.data(), (size_t)nf * 8);
        return VBMF_OK;
    }
    // a mixed call: each group on compact copies; the results are scattered into the caller's arrays only once BOTH groups have run, so
    // a failure in the second (device memory, a HIP error) leaves them as they were.  A field is (pointer, doubles per fit or 0 = M_b H)
    const int64_t L = c->L, LH = L * H, h2 = (int64_t)H * H, nsg = rows ? L : 1;
    std::vector<int64_t> off((size_t)nf + 1, 0);
    for (int64_t f = 0; f < nf; ++f) off[(size_t)f + 1] = off[(size_t)f] + Mbs[(size_t)f] * H;
    struct Field { double* p; int64_t per; bool in; };
    const Field fields[] = {{const_cast<double*>(gamma), 1, true}, {const_cast<double*>(delta0), 1, true}, {const_cast<double*>(etaVec), 1, true},
                            {const_cast<double*>(zeta0), 1, true}, {priors9, 9, true}, {BHat, LH, true}, {SigmaB, h2, true}, {CB, H, true},
                            {sigmaVec, nsg, true}, {CA, 0, true}, {delta, H, false}, {zetaVec, nsg, false}, {beta, 0, false},
                            {diagSigmaATVec, 0, false}, {SigmaA, h2, false}, {ATVecHat, 0, false}, {d_last, 1, false}, {trace, 2 * niter, false}};
    constexpr int NFLD = sizeof(fields) / sizeof(fields[0]);
    std::vector<int64_t> sels[2], itds[2], stts[2];
    std::vector<double> bufs[2][NFLD];
    for (int grp = 0; grp < 2; ++grp) {
        const int64_t want = grp ? VBMF_FIT_FORM_SPLIT : VBMF_FIT_FORM_STREAM;
        std::vector<int64_t>&sel = sels[grp], &itd = itds[grp], &stt = stts[grp];
        std::vector<int64_t> fb, m0;
        for (int64_t f = 0; f < nf; ++f)
            if (used[(size_t)f] == want) {
                sel.push_back(f);
                fb.push_back(fit_bag[f]);
                if (M0) m0.push_back(M0[f]);
            }
        const int64_t ng = (int64_t)sel.size();
        itd.resize((size_t)ng);
        stt.resize((size_t)ng);
        std::vector<double>* buf = bufs[grp];
        for (int k = 0; k < NFLD; ++k) {
            if (!fields[k].p) continue;
            for (int64_t f : sel) {
                const int64_t per = fields[k].per ? fields[k].per : Mbs[(size_t)f] * H, o = fields[k].per ? f * per : off[(size_t)f];
                if (fields[k].in) buf[k].insert(buf[k].end(), fields[k].p + o, fields[k].p + o + per);
                else buf[k].insert(buf[k].end(), (size_t)per, 0.0);
            }
        }
        auto P = [&](int k) { return fields[k].p ? buf[k].data() : nullptr; };
        TRY(run(grp != 0, ng, fb.data(), M0 ? m0.data() : nullptr, P(0), P(1), P(2), P(3), P(4), P(5), P(6), P(7), P(8), P(9), P(10), P(11),
                P(12), P(13), P(14), P(15), itd.data(), P(16), stt.data(), P(17)));
    }
    for (int grp = 0; grp < 2; ++grp) {
        const std::vector<int64_t>&sel = sels[grp], &itd = itds[grp], &stt = stts[grp];
        const std::vector<double>* buf = bufs[grp];
        const int64_t ng = (int64_t)sel.size();
        for (int k = 4; k < NFLD; ++k) {
            if (!fields[k].p) continue;
            int64_t at = 0;
            for (int64_t f : sel) {
                const int64_t per = fields[k].per ? fields[k].per : Mbs[(size_t)f] * H, o = fields[k].per ? f * per : off[(size_t)f];
                memcpy(fields[k].p + o, buf[k].data() + at, (size_t)per * 8);
                at += per;
            }
        }
        for (int64_t i = 0; i < ng; ++i) {
            iters_done[sel[(size_t)i]] = itd[(size_t)i];
            status[sel[(size_t)i]] = stt[(size_t)i];
        }
    }
    if (form_used) memcpy(form_used, used.data(), (size_t)nf * 8);
    return VBMF_OK;
}

}  // extern "C"

// ---- many basic-model fits in one launch (fit_basic_kernels.hpp, fit_basic_gram_kernels.hpp) ---------------------------------------
static_assert(FITB_LDS_CAP == VBMF_FIT_LDS_CAP_BYTES, "include/vbmf_hip.h documents the LDS a fit may use");

// form = 2's per-fit rule, a function of (L, M_b, H) alone: the Gram form where the bag is wide enough and B, T, V fit in LDS
static bool fit_basic_auto_gram(int NBK, int64_t L, int64_t Mb, int H) {
    return Mb >= VBMF_FIT_GRAM_WIDE_FACTOR * L && fitb_gram_fits(NBK, L, H);
}

// enqueues fit_rowgram_kernel for the nk bags listed in d_kbag
static int fit_rowgram(vbmf_ctx* c, const char* fn, const float* Yc, const long long* d_off, const long long* d_kbag, int64_t nk, double* K) {
    const int64_t NT = (c->L + 15) / 16, blocks = nk * (NT * (NT + 1) / 2);
    if (blocks > (1ll << 31) - 1) FAIL(c, VBMF_ERR_UNSUPPORTED, "%s: %lld bags of %lld rows need more than 2^31 - 1 tiles of K", fn, (long long)nk, (long long)c->L);
    hipLaunchKernelGGL(fit_rowgram_kernel, dim3((unsigned)blocks), dim3(RG_THREADS), 0, c->stream, Yc, (long long)c->L, d_off, d_kbag, (int)NT, K);
    HIPCHK(c, hipGetLastError());
    return VBMF_OK;
}

// The two vbmf! calls of examples/mil_util.jl:110-114 (and the folds x p x repetitions around them) in one call: every fit's whole
// loop of src/vbmf.jl:175-231 in one workgroup of one launch.  The context supplies Y only; its state is neither read nor changed, so
// no RunFrame (see vbmf_sparse_fit_batched).  form: 0 = every fit streams Y (fit_basic_kernel), 1 = every fit iterates on K = Y Y'
// (fit_basic_gram_kernel), 2 = fit_basic_auto_gram per fit.
static int fit_basic_run(vbmf_ctx* c, const char* fn, int64_t nbags, const int64_t* col_off, int64_t nfits, const int64_t* fit_bag,
                         int64_t niter, double eps, int est_covs, int est_var, double* BHat, double* SigmaB, double* CA, double* CB,
                         double* sigma2, double* AHat, double* SigmaA, int64_t* iters_done, double* d_last, int64_t* status, double* trace,
                         int64_t form, int64_t* form_used) {
    if (!c) return VBMF_ERR_INVALID;
    if (form < 0 || form > 2) FAIL(c, VBMF_ERR_INVALID, "%s: form = %lld (0: stream, 1: Gram, 2: per fit)", fn, (long long)form);
    if (c->H > 32) FAIL(c, VBMF_ERR_UNSUPPORTED, "%s: H = %lld (built for H <= 32)", fn, (long long)c->H);
    if (c->sparse) FAIL(c, VBMF_ERR_INVALID, "%s: sparse context (the basic model only; use vbmf_sparse_fit_batched)", fn);
    if (c->has_mask) FAIL(c, VBMF_ERR_INVALID, "%s: a label mask is set (use vbmf_run per fit)", fn);
    BagDims bd;
    TRY(bags_check(c, fn, nbags, col_off, bd));
    if (nfits < 1 || nfits > (1ll << 20)) FAIL(c, VBMF_ERR_INVALID, "%s: nfits must be >= 1", fn);
    if (niter < 1 || niter > (1ll << 24)) FAIL(c, VBMF_ERR_INVALID, "%s: niter must be >= 1", fn);
    if (!fit_bag || !BHat || !SigmaB || !CA || !CB || !sigma2 || !iters_done || !d_last || !status)
        FAIL(c, VBMF_ERR_INVALID, "%s: null pointer (only AHat, SigmaA and trace may be NULL)", fn);
    const int H = (int)c->H, NBK = nb_tier(H);
    const int64_t L = c->L, nf = nfits, nb = nbags, h2 = (int64_t)H * H, LH = L * H;
    if (form == 1 && !fitb_gram_fits(NBK, L, H))
        FAIL(c, VBMF_ERR_UNSUPPORTED, "%s: form = 1 at L = %lld, H = %d: the Gram form's state (3 L H doubles) does not fit in LDS", fn,
             (long long)L, H);
    if (form && bd.widest > 65535ll * RG_THREADS) FAIL(c, VBMF_ERR_UNSUPPORTED, "%s: form = %lld with a bag of %lld columns", fn, (long long)form, (long long)bd.widest);
    // col_off | fit_bag | fit_off | fit_form | fit_k | kbag (the last three only when a fit may take the Gram form)
    std::vector<long long> idx((size_t)(nb + 1 + nf + nf + 1 + (form ? nf + nf + nb : 0)));
    long long* fit_off = idx.data() + nb + 1 + nf;
    long long* fit_form = form ? fit_off + nf + 1 : nullptr;
    long long* fit_k = form ? fit_form + nf : nullptr;
    long long* kbag = form ? fit_k + nf : nullptr;
    fit_off[0] = 0;
    size_t lds_doubles = 0;
    int64_t nk = 0, ngram = 0, widest_gram = 0;                    // bags whose K is built; Gram-form fits; their widest bag
    std::vector<long long> k_of(form ? (size_t)nb : 0, -1);
    for (int64_t f = 0; f < nf; ++f) {
        const int64_t b = fit_bag[f];
        if (b < 0 || b >= nb) FAIL(c, VBMF_ERR_INVALID, "%s: fit_bag[%lld] = %lld outside 0..nbags-1", fn, (long long)f, (long long)b);
        const int64_t Mb = col_off[b + 1] - col_off[b];
        fit_off[f + 1] = fit_off[f] + Mb;
        idx[(size_t)(nb + 1 + f)] = b;
        const bool gram = form == 1 || (form == 2 && fit_basic_auto_gram(NBK, L, Mb, H));
        if (form) {
            fit_form[f] = gram;
            fit_k[f] = 0;
        }
        if (gram) {
            if (k_of[(size_t)b] < 0) { k_of[(size_t)b] = nk; kbag[nk++] = b; }
            fit_k[f] = k_of[(size_t)b];
            ++ngram;
            widest_gram = std::max(widest_gram, Mb);
        } else {
            lds_doubles = std::max(lds_doubles, (size_t)fitb_basic_lds_doubles(NBK, L, Mb, H));
        }
    }
    for (int64_t b = 0; b <= nb; ++b) idx[(size_t)b] = col_off[b];
    for (int64_t k = nk; form && k < nb; ++k) kbag[k] = 0;
    if (!c->cache.have_Y()) FAIL(c, VBMF_ERR_INVALID, "%s: no Y: call vbmf_set_Y first", fn);           // (no state needed)
    // the staging vectors outlive every copy: an error between the first asynchronous copy and the synchronise drains the stream below
    std::vector<double> in, out;
    auto run = [&]() -> int {
    HIPCHK(c, hipSetDevice(c->o.device));
    const int64_t SMH = fit_off[nf] * H, nidx = (int64_t)idx.size(), ntr = trace ? 2 * nf * niter : 0, ny = (L * c->M + 1) / 2;
    // c->bags: [col_off | fit_bag | fit_off | fit_form | fit_k | kbag (int64) | sigma2 nf | CA | CB (nf H each) | d_last | iters | status (int64) (nf each) | B | Bw |
    //           Qw (nf L H each) | SigmaB | SigmaA (nf H^2) | A | Aw (sum M_b H each) | trace | Yr | Yc (L M floats each) | K (L^2 per bag a
    //           Gram-form fit works on) | V (nf L H, when there is such a fit)]
    const int64_t o_s2 = nidx, o_ca = o_s2 + nf, o_cb = o_ca + nf * H, o_dl = o_cb + nf * H, o_it = o_dl + nf, o_st = o_it + nf,
                  o_b = o_st + nf, o_bw = o_b + nf * LH, o_qw = o_bw + nf * LH, o_sb = o_qw + nf * LH, o_sa = o_sb + nf * h2,
                  o_a = o_sa + nf * h2, o_aw = o_a + SMH, o_tr = o_aw + SMH, o_yr = o_tr + ntr, o_yc = o_yr + ny, o_k = o_yc + ny,
                  o_v = o_k + nk * L * L, total = o_v + (ngram ? nf * LH : 0);
    double* d = nullptr;
    TRY(bags_reserve(c, total, &d));
    in.resize((size_t)(o_dl - o_s2));
    memcpy(in.data(), sigma2, (size_t)nf * 8);
    memcpy(in.data() + (o_ca - o_s2), CA, (size_t)(nf * H) * 8);
    memcpy(in.data() + (o_cb - o_s2), CB, (size_t)(nf * H) * 8);
    HIPCHK(c, hipMemcpyAsync(d, idx.data(), (size_t)nidx * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d + o_s2, in.data(), in.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d + o_b, BHat, (size_t)(nf * LH) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d + o_sb, SigmaB, (size_t)(nf * h2) * 8, hipMemcpyHostToDevice, c->stream));
    if (ntr) HIPCHK(c, hipMemsetAsync(d + o_tr, 0, (size_t)ntr * 8, c->stream));
    float* Yr = reinterpret_cast<float*>(d + o_yr);
    float* Yc = reinterpret_cast<float*>(d + o_yc);
    TRY(fit_stage(c, Yr, Yc));
    long long* di = reinterpret_cast<long long*>(d);
    long long* d_form = di + nb + 1 + nf + nf + 1;                  // fit_form | fit_k | kbag
    FitBasicArgs a{Yr, Yc, (long long)L, (long long)c->M, di, di + nb + 1, di + nb + 1 + nf, H, (int)niter,
                   (c->o.reference_compat & VBMF_COMPAT_SPECTRAL_DELTA) ? 1 : 0, est_covs ? 1 : 0, est_var ? 1 : 0, eps,
                   d + o_b, d + o_sb, d + o_ca, d + o_cb, d + o_s2, d + o_sa, d + o_a, d + o_bw, d + o_qw, d + o_aw,
                   reinterpret_cast<long long*>(d + o_it), d + o_dl, reinterpret_cast<long long*>(d + o_st), trace ? d + o_tr : nullptr,
                   form ? d_form : nullptr};
    if (ngram < nf) {
        const size_t lds = lds_doubles * 8;
        dispatch<1, 2>(std::min(NBK, 2), [&](auto nbk) {
            hipLaunchKernelGGL((fit_basic_kernel<decltype(nbk)::value>), dim3((unsigned)nf), dim3(FITB_THREADS), lds, c->stream, a);
        });
        HIPCHK(c, hipGetLastError());
    }
    if (ngram) {
        TRY(fit_rowgram(c, fn, Yc, di, d_form + nf + nf, nk, d + o_k));
        FitBasicGramArgs ga{a, d + o_k, d_form + nf, d + o_v};
        const size_t lds = (size_t)fitb_gram_lds_doubles(NBK, L, H) * 8;
        dispatch<1, 2>(std::min(NBK, 2), [&](auto nbk) {
            hipLaunchKernelGGL((fit_basic_gram_kernel<decltype(nbk)::value>), dim3((unsigned)nf), dim3(FITB_THREADS), lds, c->stream, ga);
        });
        HIPCHK(c, hipGetLastError());
        if (AHat) {
            const dim3 grid((unsigned)nf, (unsigned)cdiv(widest_gram, RG_THREADS));
            dispatch<16, 32>(std::min(16 * NBK, 32), [&](auto ht) {
                hipLaunchKernelGGL((fit_rowgram_finish_kernel<decltype(ht)::value>), grid, dim3(RG_THREADS), (size_t)LH * 8, c->stream, ga);
            });
            HIPCHK(c, hipGetLastError());
        }
    }
    // read-back: [sigma2 | CA | CB | d_last | iters | status] is one block; the per-fit matrices one block each
    out.resize((size_t)(o_b - o_s2));
    HIPCHK(c, hipMemcpyAsync(out.data(), d + o_s2, out.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(BHat, d + o_b, (size_t)(nf * LH) * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(SigmaB, d + o_sb, (size_t)(nf * h2) * 8, hipMemcpyDeviceToHost, c->stream));
    if (SigmaA) HIPCHK(c, hipMemcpyAsync(SigmaA, d + o_sa, (size_t)(nf * h2) * 8, hipMemcpyDeviceToHost, c->stream));
    if (AHat) HIPCHK(c, hipMemcpyAsync(AHat, d + o_a, (size_t)SMH * 8, hipMemcpyDeviceToHost, c->stream));
    if (trace) HIPCHK(c, hipMemcpyAsync(trace, d + o_tr, (size_t)ntr * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    memcpy(sigma2, out.data(), (size_t)nf * 8);
    memcpy(CA, out.data() + (o_ca - o_s2), (size_t)(nf * H) * 8);
    memcpy(CB, out.data() + (o_cb - o_s2), (size_t)(nf * H) * 8);
    memcpy(d_last, out.data() + (o_dl - o_s2), (size_t)nf * 8);
    memcpy(iters_done, out.data() + (o_it - o_s2), (size_t)nf * 8);
    memcpy(status, out.data() + (o_st - o_s2), (size_t)nf * 8);
    for (int64_t f = 0; form_used && f < nf; ++f) form_used[f] = form ? fit_form[f] : 0;
    return VBMF_OK;
    };
    const int rc = run();
    if (rc != VBMF_OK) hipStreamSynchronize(c->stream);
    return rc;
}

extern "C" {

int vbmf_fit_batched(vbmf_ctx* c, int64_t nbags, const int64_t* col_off, int64_t nfits, const int64_t* fit_bag, int64_t niter, double eps,
                     int est_covs, int est_var, double* BHat, double* SigmaB, double* CA, double* CB, double* sigma2, double* AHat,
                     double* SigmaA, int64_t* iters_done, double* d_last, int64_t* status, double* trace) {
    return fit_basic_run(c, "vbmf_fit_batched", nbags, col_off, nfits, fit_bag, niter, eps, est_covs, est_var, BHat, SigmaB, CA, CB, sigma2,
                         AHat, SigmaA, iters_done, d_last, status, trace, 0, nullptr);
}

int vbmf_fit_batched_form(vbmf_ctx* c, int64_t nbags, const int64_t* col_off, int64_t nfits, const int64_t* fit_bag, int64_t niter,
                          double eps, int est_covs, int est_var, double* BHat, double* SigmaB, double* CA, double* CB, double* sigma2,
                          double* AHat, double* SigmaA, int64_t* iters_done, double* d_last, int64_t* status, double* trace, int64_t form,
                          int64_t* form_used) {
    return fit_basic_run(c, "vbmf_fit_batched_form", nbags, col_off, nfits, fit_bag, niter, eps, est_covs, est_var, BHat, SigmaB, CA, CB,
                         sigma2, AHat, SigmaA, iters_done, d_last, status, trace, form, form_used);
}

// K_b = Y_b Y_b' of every bag (fit_rowgram_kernel): what the Gram form iterates on, and the B'K B of the least-squares callers
int vbmf_bags_row_gram(vbmf_ctx* c, int64_t nbags, const int64_t* col_off, double* K) {
    if (!c) return VBMF_ERR_INVALID;
    const char* fn = "vbmf_bags_row_gram";
    BagDims bd;
    TRY(bags_check(c, fn, nbags, col_off, bd));
    if (!K) FAIL(c, VBMF_ERR_INVALID, "%s: null K", fn);
    if (!c->cache.have_Y()) FAIL(c, VBMF_ERR_INVALID, "%s: no Y: call vbmf_set_Y first", fn);
    HIPCHK(c, hipSetDevice(c->o.device));
    const int64_t nb = nbags, L = c->L, ny = (L * c->M + 1) / 2;
    std::vector<long long> idx((size_t)(2 * nb + 1));               // col_off | kbag = 0 .. nb - 1
    for (int64_t b = 0; b <= nb; ++b) idx[(size_t)b] = col_off[b];
    for (int64_t b = 0; b < nb; ++b) idx[(size_t)(nb + 1 + b)] = b;
    auto run = [&]() -> int {
        // c->bags: [col_off | kbag (int64) | K nb L^2 | Yr | Yc (L M floats each)]
        const int64_t o_k = (int64_t)idx.size(), o_yr = o_k + nb * L * L, o_yc = o_yr + ny, total = o_yc + ny;
        double* d = nullptr;
        TRY(bags_reserve(c, total, &d));
        long long* di = reinterpret_cast<long long*>(d);
        HIPCHK(c, hipMemcpyAsync(d, idx.data(), idx.size() * 8, hipMemcpyHostToDevice, c->stream));
        float* Yc = reinterpret_cast<float*>(d + o_yc);
        TRY(fit_stage(c, reinterpret_cast<float*>(d + o_yr), Yc));
        TRY(fit_rowgram(c, fn, Yc, di, di + nb + 1, nb, d + o_k));
        HIPCHK(c, hipMemcpyAsync(K, d + o_k, (size_t)(nb * L * L) * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return VBMF_OK;
    };
    const int rc = run();
    if (rc != VBMF_OK) hipStreamSynchronize(c->stream);             // (idx is a local)
    return rc;
}

}  // extern "C"
