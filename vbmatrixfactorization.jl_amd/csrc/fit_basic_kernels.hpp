// fit_basic_kernels.hpp -- many small basic-model fits in one launch (vbmf_fit_batched; the two vbmf! calls of
// examples/mil_util.jl:110-114 and the folds x p x repetitions around them in one call).
//
// The sibling of fit_batch_kernels.hpp, from which it takes the staging kernel (fit_stage_kernel: Y as stored into two fp32 planes, once
// per call), the products (fitb_product), the chunked Gram reductions (fitb_chunk_reduce), the workgroup folds and lambda_max
// (fitb_lambda_max, fitb_scale).  ONE launch of fit_basic_kernel runs the whole `while i <= niter && d > eps` loop of src/vbmf.jl:175-231
// for every fit, one 512-thread workgroup per fit, everything in fp64 (Y widened on load).  Fit f works on bag fit_bag[f].  Per sweep:
//   updateA!       P = Y_b'B; SigmaA = sigma2 inv(B'B + L SigmaB + sigma2 invCA) by one wave's blk_sweep; A = P SigmaA / sigma2, a row
//                  per thread (:95-98)
//   updateB!       A'A; SigmaB = sigma2 inv(A'A + M_b SigmaA + sigma2 invCB); Q = Y_b A; B = Q SigmaB / sigma2 (:109-112); Q's rows then
//                  hold B_old - B
//   updateCA! / updateCB! (est_covs)   CA_h = ||A_h||^2 / M_b + SigmaA_hh, CB_h = ||B_h||^2 / L + SigmaB_hh (:129-146): diagonals of the
//                  Grams the sweep holds
//   updateSigma2! (est_var)   sigma2 = (||Y_b||^2 - 2 sum B o Q + tr((A'A + M_b SigmaA)(B'B + L SigmaB))) / (L M_b) (:153-157)
//   d              norm(B - B_old) / norm(B_old), as in fit_batch_kernel
// B'B of the new B serves d, updateCB!, updateSigma2! and the next sweep's updateA!: one Gram of B per sweep.  The fit leaves the loop
// when !(d > eps) (a NaN d stops it) or with status = 1 after a sweep that met a non-finite sigma2, a CA_h / CB_h that is not positive and
// finite, or a pivot that is not positive and finite.
// State: B, Q (L x H each, row-major) and P / A (M_b x H, sharing storage) in LDS when they fit under FITB_LDS_CAP, else in the fit's own
// slices of the scratch buffer (fitb_basic_placement).  Every sum's order is fixed by (L, M_b, H); no atomics, no hand-off between
// workgroups.
#pragma once
#include "fit_batch_kernels.hpp"

namespace vbmf {

// doubles of dynamic LDS in front of a fit's state: one inverse image and nine H x H matrices (B'B, A'A + M_b SigmaA, SigmaA, SigmaB,
// dB'dB and the two ping-pong pairs of the eigenvalue iteration)
__host__ __device__ constexpr int fitb_basic_fixed_doubles(int NBK, int H) { return (16 * NBK) * (16 * NBK + 2) + 9 * H * H; }
// where a fit's state lives: 2 = everything in LDS, 1 = B and Q only, 0 = nothing
__host__ __device__ constexpr int fitb_basic_placement(int NBK, long long L, long long Mb, int H) {
    const long long room = (long long)(FITB_LDS_CAP / 8) - fitb_basic_fixed_doubles(NBK, H);
    return 2 * L * H + Mb * H <= room ? 2 : (2 * L * H <= room ? 1 : 0);
}
__host__ __device__ constexpr long long fitb_basic_lds_doubles(int NBK, long long L, long long Mb, int H) {
    const int pl = fitb_basic_placement(NBK, L, Mb, H);
    return fitb_basic_fixed_doubles(NBK, H) + (pl >= 1 ? 2 * L * H : 0) + (pl == 2 ? Mb * H : 0);
}

struct FitBasicArgs {
    const float* Yr; const float* Yc; long long L, Mtot;
    const long long* col_off; const long long* fit_bag; const long long* fit_off;   // fit_off[f]: columns of the fits before f
    int H, niter, spectral, est_covs, est_var;
    double eps;
    double* B; double* SB; double* CA; double* CB; double* sigma2;                   // in / out (B: L x H column-major per fit)
    double* SA; double* A;                                                          // out (A: M_b x H column-major per fit)
    double* Bw; double* Qw; double* Aw;            // working B, Q (nfits x L x H) and P / A (sum M_b x H) of fits whose state is not in LDS
    long long* iters; double* dlast; long long* status; double* trace;
    const long long* form;                         // nullptr: every fit streams; else form[f] != 0: fit f belongs to fit_basic_gram_kernel
};

// the H x H block of -inv(W) a blk_sweep left in the upper blocks of the image, times -scale, into the dense symmetric out
__device__ __forceinline__ void fitb_basic_take(const double* Wk, int LD, int H, double scale, double* out) {
    for (int t = threadIdx.x; t < H * H; t += FITB_THREADS) {
        const int i = t / H, j = t % H;
        out[t] = -scale * (i <= j ? Wk[i * LD + j] : Wk[j * LD + i]);
    }
}

template <int NBK>
__global__ __launch_bounds__(FITB_THREADS) void fit_basic_kernel(FitBasicArgs g) {
    extern __shared__ __attribute__((aligned(16))) double lds_fbb[];
    __shared__ double part[1024];
    __shared__ double red[16];
    __shared__ double ca_s[32], cb_s[32], ata_s[32], vec_s[64];
    __shared__ int bad_s;
    constexpr int NP = 16 * NBK, LD = NP + 2;
    const int f = blockIdx.x, H = g.H, tid = threadIdx.x, h2 = H * H;
    if (g.form && g.form[f]) return;                                // (uniform, before any barrier)
    const long long L = g.L, b = g.fit_bag[f], m0 = g.col_off[b], Mb = g.col_off[b + 1] - m0;
    const long long n = Mb * H, o = g.fit_off[f] * H, nb = L * H;
    const int place = fitb_basic_placement(NBK, L, Mb, H);
    // dynamic LDS: [image | B'B | A'A + M_b SigmaA | SigmaA | SigmaB | dB'dB | eigen 4 H^2 | B, Q | P / A]
    double* Wk = lds_fbb;
    double* BB = lds_fbb + NP * LD;
    double* AA = BB + h2;
    double* SAm = AA + h2;
    double* SBm = SAm + h2;
    double* Dm = SBm + h2;
    double* E = Dm + h2;
    double* st = E + 4 * h2;
    double* Bl = place >= 1 ? st : g.Bw + (long long)f * nb;
    double* Ql = place >= 1 ? st + nb : g.Qw + (long long)f * nb;
    double* PAb = place == 2 ? st + 2 * nb : g.Aw + o;
    const float* Yr = g.Yr + m0;                                    // Y_b[l, m] = Yr[l * Mtot + m] = Yc[m * L + l]
    const float* Yc = g.Yc + m0 * L;
    const int lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nbu = (H + 15) >> 4;

    for (long long t = tid; t < nb; t += FITB_THREADS) {
        const long long l = t / H;
        const int h = (int)(t - l * H);
        Bl[t] = g.B[(long long)f * nb + (long long)h * L + l];
    }
    for (int t = tid; t < h2; t += FITB_THREADS) {
        SBm[t] = g.SB[(long long)f * h2 + t];
        SAm[t] = 0.0;
    }
    if (tid < H) {
        ca_s[tid] = g.CA[(long long)f * H + tid];
        cb_s[tid] = g.CB[(long long)f * H + tid];
    }
    if (tid == 0) bad_s = 0;
    const double Lg = (double)L, Mg = (double)Mb;
    double sig = g.sigma2[f], d = g.eps + 1.0;
    // ||Y_b||^2
    double yy = 0.0;
    for (long long t = tid; t < L * Mb; t += FITB_THREADS) {
        const long long l = t / Mb, m = t - l * Mb;
        const double y = (double)Yr[l * g.Mtot + m];
        yy += y * y;
    }
    yy = fitb_sum(yy, red);                                        // (its barriers publish B, SigmaB, CA, CB)
    fitb_chunk_reduce(h2, L, part, BB, [&](int e, long long l) { return Bl[l * H + e / H] * Bl[l * H + e % H]; });
    // norm(B): sqrt(lambda_max(B'B)), the Gram of B scaled into range when B's own would underflow
    double nrmB;
    {
        double mB = 0.0;
        for (long long t = tid; t < nb; t += FITB_THREADS) mB = fmax(mB, fabs(Bl[t]));
        mB = fitb_max(mB, red);
        const double sB = fitb_scale(mB);
        if (sB != 1.0)
            fitb_chunk_reduce(h2, L, part, AA, [&](int e, long long l) { return (sB * Bl[l * H + e / H]) * (sB * Bl[l * H + e % H]); });
        const double* Gb = sB != 1.0 ? AA : BB;
        double lam, lam_unused;
        fitb_lambda_max(Gb, Gb, H, g.spectral, E, vec_s, lam, lam_unused);
        nrmB = sqrt(lam) / sB;
    }
    int it = 0, status = 0;
    for (; it < g.niter; ++it) {
        int bad = 0;
        // ---- updateA! ------------------------------------------------------------------------------------------------------------
        for (int t = tid; t < NP * NP; t += FITB_THREADS) {
            const int i = t / NP, j = t % NP;
            Wk[i * LD + j] = (i < H && j < H) ? BB[i * H + j] + Lg * SBm[i * H + j] + (i == j ? sig / ca_s[i] : 0.0) : (i == j ? 1.0 : 0.0);
        }
        fitb_product<NP>(Mb, L, Yr, g.Mtot, Yc, L, Bl, H, PAb);
        __syncthreads();
        if (w == 0) {
            PivAcc pv;
            blk_sweep<NBK, 1>(Wk, LD, nbu, 0, lane, pv);
            bad |= pv.bad;
        }
        __syncthreads();
        fitb_basic_take(Wk, LD, H, sig, SAm);
        __syncthreads();
        // A = P SigmaA / sigma2, a row per thread
        for (long long m = tid; m < Mb; m += FITB_THREADS) {
            double p[NP];
#pragma unroll
            for (int j = 0; j < NP; ++j) p[j] = j < H ? PAb[m * H + j] : 0.0;
            for (int h = 0; h < H; ++h) {
                double s = 0.0;
#pragma unroll
                for (int j = 0; j < NP; ++j)
                    if (j < H) s += p[j] * SAm[j * H + h];
                PAb[m * H + h] = s / sig;
            }
        }
        __syncthreads();
        // ---- updateB! ------------------------------------------------------------------------------------------------------------
        fitb_chunk_reduce(h2, Mb, part, AA, [&](int e, long long m) { return PAb[m * H + e / H] * PAb[m * H + e % H]; });
        for (int t = tid; t < h2; t += FITB_THREADS) {
            const int i = t / H, j = t % H;
            if (i == j) ata_s[i] = AA[t];
            AA[t] += Mg * SAm[t];
        }
        __syncthreads();
        for (int t = tid; t < NP * NP; t += FITB_THREADS) {
            const int i = t / NP, j = t % NP;
            Wk[i * LD + j] = (i < H && j < H) ? AA[i * H + j] + (i == j ? sig / cb_s[i] : 0.0) : (i == j ? 1.0 : 0.0);
        }
        __syncthreads();
        if (w == 0) {
            PivAcc pv;
            blk_sweep<NBK, 1>(Wk, LD, nbu, 0, lane, pv);
            bad |= pv.bad;
        }
        __syncthreads();
        fitb_basic_take(Wk, LD, H, sig, SBm);
        fitb_product<NP>(L, Mb, Yc, L, Yr, g.Mtot, PAb, H, Ql);
        __syncthreads();
        // B = Q SigmaB / sigma2, a row per thread; Q's row then holds B_old - B
        double bq = 0.0;
        for (long long l = tid; l < L; l += FITB_THREADS) {
            double q[NP];
#pragma unroll
            for (int j = 0; j < NP; ++j) q[j] = j < H ? Ql[l * H + j] : 0.0;
            for (int h = 0; h < H; ++h) {
                double s = 0.0;
#pragma unroll
                for (int j = 0; j < NP; ++j)
                    if (j < H) s += q[j] * SBm[j * H + h];
                const double bn = s / sig, bo = Bl[l * H + h];
                bq += bn * Ql[l * H + h];
                Bl[l * H + h] = bn;
                Ql[l * H + h] = bo - bn;
            }
        }
        bq = fitb_sum(bq, red);
        fitb_chunk_reduce(h2, L, part, BB, [&](int e, long long l) { return Bl[l * H + e / H] * Bl[l * H + e % H]; });
        double mB = 0.0, mD = 0.0;
        for (long long t = tid; t < nb; t += FITB_THREADS) {
            mB = fmax(mB, fabs(Bl[t]));
            mD = fmax(mD, fabs(Ql[t]));
        }
        mB = fitb_max(mB, red);
        mD = fitb_max(mD, red);
        const double sB = fitb_scale(mB), sD = fitb_scale(mD);
        fitb_chunk_reduce(h2, L, part, Dm, [&](int e, long long l) { return (sD * Ql[l * H + e / H]) * (sD * Ql[l * H + e % H]); });
        // ---- updateCA!, updateCB!, updateSigma2! -------------------------------------------------------------------------------------
        if (g.est_covs && tid < H) {
            const double ca = ata_s[tid] / Mg + SAm[tid * H + tid], cb = BB[tid * H + tid] / Lg + SBm[tid * H + tid];
            bad |= !(ca > 0.0 && isfinite(ca)) || !(cb > 0.0 && isfinite(cb));
            ca_s[tid] = ca;
            cb_s[tid] = cb;
        }
        if (g.est_var) {
            double tr = 0.0;
            for (int t = tid; t < h2; t += FITB_THREADS) tr += AA[t] * (BB[t] + Lg * SBm[t]);
            tr = fitb_sum(tr, red);
            sig = (yy - 2.0 * bq + tr) / (Lg * Mg);
            bad |= !isfinite(sig);
        }
        // ---- d, the stop test -------------------------------------------------------------------------------------------------------
        if (sB != 1.0)                                              // (uniform; A'A + M_b SigmaA is free until the next sweep)
            fitb_chunk_reduce(h2, L, part, AA, [&](int e, long long l) { return (sB * Bl[l * H + e / H]) * (sB * Bl[l * H + e % H]); });
        double lamD, lamBn;
        fitb_lambda_max(Dm, sB != 1.0 ? AA : BB, H, g.spectral, E, vec_s, lamD, lamBn);
        d = (sqrt(lamD) / sD) / nrmB;
        nrmB = sqrt(lamBn) / sB;
        if (bad) bad_s = 1;                                         // (same value from every writer)
        __syncthreads();                                            // (also publishes ca_s, cb_s)
        if (tid == 0 && g.trace) {
            g.trace[((long long)f * g.niter + it) * 2] = d;
            g.trace[((long long)f * g.niter + it) * 2 + 1] = sig;
        }
        if (bad_s) { status = 1; ++it; break; }
        if (!(d > g.eps)) { ++it; break; }
    }
    // ---- outputs ---------------------------------------------------------------------------------------------------------------------
    for (long long t = tid; t < nb; t += FITB_THREADS) {
        const long long l = t / H;
        const int h = (int)(t - l * H);
        g.B[(long long)f * nb + (long long)h * L + l] = Bl[t];
    }
    for (long long t = tid; t < n; t += FITB_THREADS) {
        const long long m = t / H;
        const int h = (int)(t - m * H);
        g.A[o + (long long)h * Mb + m] = PAb[t];
    }
    for (int t = tid; t < h2; t += FITB_THREADS) {
        g.SB[(long long)f * h2 + t] = SBm[t];
        g.SA[(long long)f * h2 + t] = SAm[t];
    }
    if (tid < H) {
        g.CA[(long long)f * H + tid] = ca_s[tid];
        g.CB[(long long)f * H + tid] = cb_s[tid];
    }
    if (tid == 0) {
        g.sigma2[f] = sig;
        g.iters[f] = it;
        g.dlast[f] = d;
        g.status[f] = status;
    }
}

}  // namespace vbmf
