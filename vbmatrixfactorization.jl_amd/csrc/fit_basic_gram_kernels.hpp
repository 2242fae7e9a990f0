// fit_basic_gram_kernels.hpp -- the Gram form of fit_basic_kernel's sweep for WIDE bags (vbmf_fit_batched_form; the basic-model fits of
// examples/mil_util.jl:110-114 on 166 x thousands).
//
// updateA! of the basic model is A = Y'B SigmaA / sigma2 with no mask (src/vbmf.jl:95-98), so after any sweep A = Y'V with
// V = B SigmaA / sigma2 (L x H), and everything the sweep takes from Y comes from the L x L matrix K = Y Y':
//   Y A = K V =: T          A'A = V'T          sum B o (Y A) = sum B o T          ||Y||^2 = tr K
// The same iteration, not an approximation: section 10's identity turned on its side.  A sweep costs 2 L^2 H flops instead of 4 L M_b H,
// K is built once per BAG (restarts that share a bag share it) and A is formed once, after the loop.  Three kernels:
//   fit_rowgram_kernel         K_b = Y_b Y_b' in fp64 on v_mfma_f64_16x16x4_f64 from the fp32 plane Yc that fit_stage_kernel wrote (an fp32
//                              value widened to fp64 makes every product exact).  One workgroup per (bag, pair of 16-row tiles i <= j);
//                              its four waves split the columns in fixed chunks and are folded through LDS in wave order, the lower
//                              triangle is stored as the mirror of the upper: K_b is a function of (L, M_b) alone and symmetric bit for bit
//   fit_basic_gram_kernel      fit_basic_kernel's loop (src/vbmf.jl:175-231: the same order, the same sigma2 in the same places, the same
//                              bad / status rules, the same trace) with the two streaming products replaced as above.  State: B, T, V
//                              (3 L H doubles) in LDS behind fit_basic_kernel's fixed part; K is read from global memory (L2-resident at
//                              the sizes this is for).  Leaves V in the fit's scratch slice and writes everything fit_basic_kernel writes
//                              except A
//   fit_rowgram_finish_kernel  A = Y_b'V once per fit in fp64, a column per thread, V in LDS
// A workgroup whose fit does not take the kernel's form (FitBasicArgs::form) returns at once: a uniform test before any barrier.
// Every sum's order is fixed by (L, M_b, H); no atomics, no hand-off between workgroups.
#pragma once
#include "fit_basic_kernels.hpp"

namespace vbmf {

constexpr int RG_THREADS = 256, RG_NW = RG_THREADS / 64;

// a fit can take the Gram form when B, T and V fit beside fit_basic_kernel's fixed part under FITB_LDS_CAP
__host__ __device__ constexpr bool fitb_gram_fits(int NBK, long long L, int H) {
    return 3 * L * H <= (long long)(FITB_LDS_CAP / 8) - fitb_basic_fixed_doubles(NBK, H);
}
__host__ __device__ constexpr long long fitb_gram_lds_doubles(int NBK, long long L, int H) {
    return fitb_basic_fixed_doubles(NBK, H) + 3 * L * H;
}

// K of bag kbag[slot] into K + slot L^2 (full storage: one plane is both the row-major and the column-major operand).
// blockIdx.x = slot * NT (NT + 1) / 2 + the number of the tile pair (i, j), i <= j < NT = ceil(L / 16), counted row by row.
__global__ __launch_bounds__(RG_THREADS) void fit_rowgram_kernel(const float* __restrict__ Yc, long long L, const long long* __restrict__ col_off,
                                                                 const long long* __restrict__ kbag, int NT, double* __restrict__ K) {
    __shared__ double acc_s[RG_NW][RG_THREADS];
    const int npairs = NT * (NT + 1) / 2;
    const long long slot = blockIdx.x / npairs;
    int p = (int)(blockIdx.x - slot * npairs), i = 0;
    while (p >= NT - i) { p -= NT - i; ++i; }
    const int j = i + p;
    const long long b = kbag[slot], m0 = col_off[b], Mb = col_off[b + 1] - m0;
    const float* Y = Yc + m0 * L;                                   // Y_b[l, m] = Y[m * L + l]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, q = lane >> 4, c = lane & 15;
    // blk_inverse.hpp's layouts: A operand = Y[16 i + c][m = 4 s + q], B operand = Y'[m = 4 s + q][16 j + c]
    const long long ra = 16ll * i + c, rb = 16ll * j + c;
    const bool oa = ra < L, ob = rb < L;                            // rows beyond L contribute zeros
    const long long nsteps = (Mb + 3) / 4, per = (nsteps + RG_NW - 1) / RG_NW;
    const long long s0 = w * per, s1 = s0 + per < nsteps ? s0 + per : nsteps;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (long long s = s0; s < s1; ++s) {
        const long long m = 4 * s + q;
        const bool on = m < Mb;                                     // columns beyond M_b contribute zeros
        const double ya = on && oa ? (double)Y[m * L + ra] : 0.0;
        const double yb = on && ob ? (double)Y[m * L + rb] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ya, yb, acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) acc_s[w][r * 64 + lane] = acc[r];
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < RG_NW; ++k) s += acc_s[k][tid];             // wave order
    // thread t holds register t / 64 of lane t % 64: element [row q + 4 r][column c] of the tile
    const int row = q + 4 * w, col = c;
    const long long gi = 16ll * i + row, gj = 16ll * j + col;
    if (gi < L && gj < L && (i != j || row <= col)) {
        double* Kb = K + slot * L * L;
        Kb[gi * L + gj] = s;
        Kb[gj * L + gi] = s;
    }
}

struct FitBasicGramArgs {
    FitBasicArgs b;                                // b.form[f] != 0: fit f takes this form; b.A: written by fit_rowgram_finish_kernel
    const double* K; const long long* fit_k;       // K of fit f: K + fit_k[f] L^2
    double* Vw;                                    // nfits x L x H (row-major): V on leaving the loop
};

template <int NBK>
__global__ __launch_bounds__(FITB_THREADS) void fit_basic_gram_kernel(FitBasicGramArgs ga) {
    extern __shared__ __attribute__((aligned(16))) double lds_fbg[];
    __shared__ double part[1024];
    __shared__ double red[16];
    __shared__ double ca_s[32], cb_s[32], ata_s[32], vec_s[64];
    __shared__ int bad_s;
    const FitBasicArgs& g = ga.b;
    constexpr int NP = 16 * NBK, LD = NP + 2;
    const int f = blockIdx.x;
    if (!g.form[f]) return;                                         // (uniform, before any barrier)
    const int H = g.H, tid = threadIdx.x, h2 = H * H;
    const long long L = g.L, b = g.fit_bag[f], Mb = g.col_off[b + 1] - g.col_off[b], nb = L * H;
    // dynamic LDS: [image | B'B | A'A + M_b SigmaA | SigmaA | SigmaB | dB'dB | eigen 4 H^2 | B, T, V]
    double* Wk = lds_fbg;
    double* BB = lds_fbg + NP * LD;
    double* AA = BB + h2;
    double* SAm = AA + h2;
    double* SBm = SAm + h2;
    double* Dm = SBm + h2;
    double* E = Dm + h2;
    double* Bl = E + 4 * h2;
    double* Tl = Bl + nb;
    double* Vl = Tl + nb;
    const double* Kb = ga.K + ga.fit_k[f] * L * L;                  // symmetric: K_b[l, k] = Kb[l * L + k] = Kb[k * L + l]
    const int lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nbu = (H + 15) >> 4;

    for (long long t = tid; t < nb; t += FITB_THREADS) {
        const long long l = t / H;
        const int h = (int)(t - l * H);
        Bl[t] = g.B[(long long)f * nb + (long long)h * L + l];
        Vl[t] = 0.0;                                                // (niter >= 1: overwritten by the first sweep)
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
    // ||Y_b||^2 = tr K_b
    double yy = 0.0;
    for (long long l = tid; l < L; l += FITB_THREADS) yy += Kb[l * L + l];
    yy = fitb_sum(yy, red);                                        // (its barriers publish B, SigmaB, CA, CB)
    fitb_chunk_reduce(h2, L, part, BB, [&](int e, long long l) { return Bl[l * H + e / H] * Bl[l * H + e % H]; });
    // norm(B), as in fit_basic_kernel
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
        // ---- updateA!: SigmaA, and V in place of A -----------------------------------------------------------------------------------
        for (int t = tid; t < NP * NP; t += FITB_THREADS) {
            const int i = t / NP, j = t % NP;
            Wk[i * LD + j] = (i < H && j < H) ? BB[i * H + j] + Lg * SBm[i * H + j] + (i == j ? sig / ca_s[i] : 0.0) : (i == j ? 1.0 : 0.0);
        }
        __syncthreads();
        if (w == 0) {
            PivAcc pv;
            blk_sweep<NBK, 1>(Wk, LD, nbu, 0, lane, pv);
            bad |= pv.bad;
        }
        __syncthreads();
        fitb_basic_take(Wk, LD, H, sig, SAm);
        __syncthreads();
        // V = B SigmaA / sigma2, a row per thread (A = Y_b'V)
        for (long long l = tid; l < L; l += FITB_THREADS) {
            double p[NP];
#pragma unroll
            for (int j = 0; j < NP; ++j) p[j] = j < H ? Bl[l * H + j] : 0.0;
            for (int h = 0; h < H; ++h) {
                double s = 0.0;
#pragma unroll
                for (int j = 0; j < NP; ++j)
                    if (j < H) s += p[j] * SAm[j * H + h];
                Vl[l * H + h] = s / sig;
            }
        }
        __syncthreads();
        // ---- updateB! ------------------------------------------------------------------------------------------------------------
        fitb_product<NP>(L, L, Kb, L, Kb, L, Vl, H, Tl);           // T = K V = Y_b A
        __syncthreads();
        // A'A = V'T: entry (i, j) and its mirror are the same sum of the same products
        fitb_chunk_reduce(h2, L, part, AA, [&](int e, long long l) {
            const int i = e / H, j = e % H;
            return i <= j ? Vl[l * H + i] * Tl[l * H + j] : Vl[l * H + j] * Tl[l * H + i];
        });
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
        __syncthreads();
        // B = T SigmaB / sigma2, a row per thread; T's row then holds B_old - B
        double bq = 0.0;
        for (long long l = tid; l < L; l += FITB_THREADS) {
            double q[NP];
#pragma unroll
            for (int j = 0; j < NP; ++j) q[j] = j < H ? Tl[l * H + j] : 0.0;
            for (int h = 0; h < H; ++h) {
                double s = 0.0;
#pragma unroll
                for (int j = 0; j < NP; ++j)
                    if (j < H) s += q[j] * SBm[j * H + h];
                const double bn = s / sig, bo = Bl[l * H + h];
                bq += bn * Tl[l * H + h];
                Bl[l * H + h] = bn;
                Tl[l * H + h] = bo - bn;
            }
        }
        bq = fitb_sum(bq, red);
        fitb_chunk_reduce(h2, L, part, BB, [&](int e, long long l) { return Bl[l * H + e / H] * Bl[l * H + e % H]; });
        double mB = 0.0, mD = 0.0;
        for (long long t = tid; t < nb; t += FITB_THREADS) {
            mB = fmax(mB, fabs(Bl[t]));
            mD = fmax(mD, fabs(Tl[t]));
        }
        mB = fitb_max(mB, red);
        mD = fitb_max(mD, red);
        const double sB = fitb_scale(mB), sD = fitb_scale(mD);
        fitb_chunk_reduce(h2, L, part, Dm, [&](int e, long long l) { return (sD * Tl[l * H + e / H]) * (sD * Tl[l * H + e % H]); });
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
    // ---- outputs: fit_basic_kernel's, with V in place of A -----------------------------------------------------------------------------
    for (long long t = tid; t < nb; t += FITB_THREADS) {
        const long long l = t / H;
        const int h = (int)(t - l * H);
        g.B[(long long)f * nb + (long long)h * L + l] = Bl[t];
        ga.Vw[(long long)f * nb + t] = Vl[t];
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

// A = Y_b'V of fit blockIdx.x, columns blockIdx.y * 256 .. + 255 of its bag, into the column-major per-fit layout of AHat.
// Dynamic LDS: L H doubles.
template <int HP>
__global__ __launch_bounds__(RG_THREADS) void fit_rowgram_finish_kernel(FitBasicGramArgs ga) {
    extern __shared__ __attribute__((aligned(16))) double lds_fin[];
    const FitBasicArgs& g = ga.b;
    const int f = blockIdx.x, H = g.H;
    const long long L = g.L, b = g.fit_bag[f], m0 = g.col_off[b], Mb = g.col_off[b + 1] - m0;
    if (!g.form[f] || (long long)blockIdx.y * RG_THREADS >= Mb) return;   // (uniform, before any barrier)
    for (long long t = threadIdx.x; t < L * H; t += RG_THREADS) lds_fin[t] = ga.Vw[(long long)f * L * H + t];
    __syncthreads();
    const long long m = (long long)blockIdx.y * RG_THREADS + threadIdx.x;
    if (m >= Mb) return;
    const float* y = g.Yr + m0 + m;                                 // Y_b[l, m] = y[l * Mtot]: neighbouring lanes, neighbouring columns
    double acc[HP];
#pragma unroll
    for (int h = 0; h < HP; ++h) acc[h] = 0.0;
    for (long long l = 0; l < L; ++l) {
        const double yv = (double)y[l * g.Mtot];
        const double* v = lds_fin + l * H;
#pragma unroll
        for (int h = 0; h < HP; ++h)
            if (h < H) acc[h] = fma(yv, v[h], acc[h]);
    }
    double* A = g.A + g.fit_off[f] * H;
#pragma unroll
    for (int h = 0; h < HP; ++h)
        if (h < H) A[(long long)h * Mb + m] = acc[h];
}

}  // namespace vbmf
