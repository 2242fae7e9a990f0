// fit_split_kernels.hpp -- ONE wide ARD-family fit over many workgroups (vbmf_ard_fit_batched_form, form = VBMF_FIT_FORM_SPLIT): the sweep
// of fit_batch_kernel (fit_batch_kernels.hpp: its header describes the updates and their places in the reference) cut at the one point
// where it is a sum over columns.  A fit's columns are cut into slices of slice_cols columns counted from the fit's own first column; a
// sweep is two plain launches on the context's stream, and the launch boundary is the only synchronisation:
//   fit_cols_kernel  one workgroup per (fit, slice): P = Y_slice'X (X = B, ROWS: diag(s) B), updateA! (diagonal form, or full_cov with one
//                    column per wavefront), updateCA!; writes the slice's A, dS, CA, beta and, into the slice's own slot, A_slice'A_slice,
//                    the slice's share of SigmaA, Q_slice = Y_slice A_slice, the six group sums of log beta / CA and its `bad` word
//   fit_fold_kernel  one workgroup per fit: folds the slots in slice order and runs the rest of the sweep as fit_batch_kernel does from
//                    its Wk on (SigmaB, B, B'B, dB'dB, updateCB!, updateSigma!, est_priors, d, the stop test, the trace row); writes the
//                    fit's outputs and publishes what the next column pass reads: B (row-major, g.Bw), ROWS: diag(s) B (g.Qw), B'B,
//                    B'diag(s)B and v_h (pub), SigmaB, CB, sigma / s, the priors (the output arrays themselves) and the done word
//   fit_split_init_kernel  one workgroup per fit, once: ||Y_b||^2 or the row norms, B row-major, B'B, norm(B), ROWS: diag(s) B and its sums
// A workgroup of a fit whose done word is set returns at once: nothing of that fit is written again.  No workgroup waits for another, no
// atomics.  Every sum's order is a function of (L, M_b, H, H0, M0, slice_cols): inside a slice what fitb_* fix, across slices slice order.
// The three per-entry rules take the entry's position in the FIT: the repeat layout's v index, the prior group and the prefix mask.
// The kernels are the three-group (LOCAL) sweep throughout: a two-group fit is M0[f] = M_b, a sparse one H0 = H (as vbmf_rows_fit_batched).
#pragma once
#include "fit_batch_kernels.hpp"

namespace vbmf {

constexpr int FITS_PUB = 8;                       // scalars in front of a fit's published block: sig | ||Y_b||^2 | norm(B) | - | - | sweeps
// a fit's published block: [scalars | B'B | B'diag(s)B (H^2 each) | v (32)]; a slice's slot: [A'A | SigmaA share (H^2 each) | Q (L H) |
// group sums 6 | bad | -]
__host__ __device__ constexpr long long fits_pub_doubles(int H) { return FITS_PUB + 2 * H * H + 32; }
__host__ __device__ constexpr long long fits_slot_doubles(long long L, int H) { return 2 * H * H + L * H + 8; }
// dynamic LDS of fit_cols_kernel: full_cov's images and p_m vectors, the slice's P/A, CA and dS, and X when it fits beside them (x_lds)
__host__ __device__ constexpr long long fits_cols_min_doubles(bool full, int NBK, int H, long long sc) {
    return (full ? FITB_NW * (16 * NBK) * (16 * NBK + 2) + FITB_NW * 16 * NBK : 0) + 3 * sc * H;
}
__host__ __device__ constexpr bool fits_cols_x_lds(bool full, int NBK, long long L, int H, long long sc) {
    return fits_cols_min_doubles(full, NBK, H, sc) + L * H <= (long long)(FITB_LDS_CAP / 8);
}
// ... of fit_fold_kernel: one image, eight H x H matrices, and B and Q when they fit (else they live in g.Bw / g.Qw)
__host__ __device__ constexpr long long fits_fold_fixed_doubles(int NBK, int H) { return (16 * NBK) * (16 * NBK + 2) + 8 * H * H; }
__host__ __device__ constexpr bool fits_fold_b_lds(int NBK, long long L, int H) {
    return fits_fold_fixed_doubles(NBK, H) + 2 * L * H <= (long long)(FITB_LDS_CAP / 8);
}

// sl_fit / sl_c0: a slice's fit and its first column inside the fit; fit_sl0[f] .. fit_sl0[f+1]-1: the slices of fit f
struct FitSplitArgs : FitRowsArgs {
    const long long* sl_fit; const long long* sl_c0; const long long* fit_sl0;
    int slice_cols, full, x_lds, b_lds;
    double* pub; double* slot; long long* done;
};

template <bool ROWS>
__global__ __launch_bounds__(FITB_THREADS) void fit_split_init_kernel(FitSplitArgs g) {
    extern __shared__ __attribute__((aligned(16))) double lds_fi[];
    __shared__ double part[1024];
    __shared__ double red[16];
    __shared__ double vec_s[64];
    const int f = blockIdx.x, H = g.H, tid = threadIdx.x, h2 = H * H;
    const long long L = g.L, b = g.fit_bag[f], m0 = g.col_off[b], Mb = g.col_off[b + 1] - m0, nb = L * H;
    double* BB = lds_fi;
    double* AA = BB + h2;
    double* E = AA + h2;
    double* Bl = g.Bw + (long long)f * nb;
    double* Ql = g.Qw + (long long)f * nb;
    double* pub = g.pub + (long long)f * fits_pub_doubles(H);
    const float* Yr = g.Yr + m0;
    const double Lg = (double)L;
    for (long long t = tid; t < nb; t += FITB_THREADS) {
        const long long l = t / H;
        const int h = (int)(t - l * H);
        Bl[t] = g.B[(long long)f * nb + (long long)h * L + l];
    }
    if (tid >= 6 && tid < 9) g.priors4[(long long)f * 9 + tid] = g.priors4[(long long)f * 9 + 2 * (tid - 6)] + 0.5;
    double sig = 0.0, yy = 0.0;
    if constexpr (ROWS) {
        double* yn = g.yn + (long long)f * L;
        int T = 1;
        while (T < 64 && L * T < FITB_THREADS) T <<= 1;
        for (long long base = 0; base < L * T; base += FITB_THREADS) {
            const long long it = base + tid;
            const bool on = it < L * T;
            const long long l = on ? it / T : 0;
            double s = 0.0;
            if (on)
                for (long long m = it & (T - 1); m < Mb; m += T) {
                    const double y = (double)Yr[l * g.Mtot + m];
                    s = fma(y, y, s);
                }
            for (int off = T >> 1; off > 0; off >>= 1) s += __shfl_xor(s, off);
            if (on && (it & (T - 1)) == 0) yn[l] = s;
        }
        double ss = 0.0;
        for (long long l = tid; l < L; l += FITB_THREADS) ss += g.sigma[(long long)f * L + l];
        sig = fitb_sum(ss, red) / Lg;
    } else {
        sig = g.sigma[f];
        for (long long t = tid; t < L * Mb; t += FITB_THREADS) {
            const long long l = t / Mb, m = t - l * Mb;
            const double y = (double)Yr[l * g.Mtot + m];
            yy += y * y;
        }
        yy = fitb_sum(yy, red);
    }
    fitb_chunk_reduce(h2, L, part, BB, [&](int e, long long l) { return Bl[l * H + e / H] * Bl[l * H + e % H]; });
    double mB = 0.0;
    for (long long t = tid; t < nb; t += FITB_THREADS) mB = fmax(mB, fabs(Bl[t]));
    mB = fitb_max(mB, red);
    const double sB = fitb_scale(mB);
    if (sB != 1.0)
        fitb_chunk_reduce(h2, L, part, AA, [&](int e, long long l) { return (sB * Bl[l * H + e / H]) * (sB * Bl[l * H + e % H]); });
    const double* Gb = sB != 1.0 ? AA : BB;
    double lam, lam_unused;
    fitb_lambda_max(Gb, Gb, H, g.spectral, E, vec_s, lam, lam_unused);
    for (int t = tid; t < h2; t += FITB_THREADS) pub[FITS_PUB + t] = BB[t];
    if constexpr (ROWS) {
        const double* sv = g.sigma + (long long)f * L;
        for (long long t = tid; t < nb; t += FITB_THREADS) Ql[t] = sv[t / H] * Bl[t];
        __syncthreads();
        fitb_chunk_reduce(H, L, part, pub + FITS_PUB + 2 * h2, [&](int h, long long l) { return Ql[l * H + h] * Ql[l * H + h]; });
        if (g.full)
            fitb_chunk_reduce(h2, L, part, pub + FITS_PUB + h2, [&](int e, long long l) {
                const int i = e / H, j = e % H;
                return Ql[l * H + (i < j ? i : j)] * Bl[l * H + (i < j ? j : i)];
            });
    }
    if (tid == 0) {
        pub[0] = sig;
        pub[1] = yy;
        pub[2] = sqrt(lam) / sB;
        pub[5] = 0.0;
        g.done[f] = 0;
    }
}

// TWINS, kept in step by hand (fit_batch_kernel may not be edited): in fit_cols_kernel the diagonal updateA! / updateCA! loop is
// fit_batch_kernels.hpp:419-453 (LOCAL branch), the full_cov wave loop :454-566, the group sums :567-570; fit_fold_kernel from its
// "updateB!" comment on is :580-699 with the fold of the slots in place of :572-579 and :595; fit_split_init_kernel is :324-389.
// What differs on purpose: m and t become the entry's column mg = c0 + m and index tg = t0 + t in the FIT wherever a per-entry rule
// reads them (vi, the prior group, the prefix mask); outputs go straight to the output arrays; sums end in the slice's slot.
template <int NBK, bool FULL, bool ROWS>
__global__ __launch_bounds__(FITB_THREADS) void fit_cols_kernel(FitSplitArgs g) {
    extern __shared__ __attribute__((aligned(16))) double lds_fs[];
    __shared__ double part[1024];
    __shared__ double red[16];
    __shared__ double v_s[32], pri_s[6];
    __shared__ int bad_s;
    constexpr int NP = 16 * NBK, LD = NP + 2, NUP = NBK * (NBK + 1) / 2, NW = FITB_NW;
    const long long sl = blockIdx.x, f = g.sl_fit[sl];
    if (g.done[f]) return;
    const int H = g.H, H0 = g.H0, tid = threadIdx.x, h2 = H * H, hmask = H - g.mask_H1;
    const long long L = g.L, b = g.fit_bag[f], m0 = g.col_off[b], Mb = g.col_off[b + 1] - m0, c0 = g.sl_c0[sl];
    const long long nc = Mb - c0 < g.slice_cols ? Mb - c0 : g.slice_cols, n = nc * H, t0 = c0 * H, o = g.fit_off[f] * H + t0, nb = L * H;
    const long long M0f = g.M0[f];
    const double* pub = g.pub + f * fits_pub_doubles(H);
    const double* Gp = pub + FITS_PUB + (ROWS ? h2 : 0);            // B'B, ROWS: B'diag(s)B
    const double* SBp = g.SB + f * h2;
    double* slot = g.slot + sl * fits_slot_doubles(L, H);
    double* AAo = slot;
    double* SAo = slot + h2;
    double* Qo = slot + 2 * h2;
    double* gso = Qo + nb;
    double* st = lds_fs + (FULL ? NW * NP * LD + NW * NP : 0);
    const double* X = (ROWS ? g.Qw : g.Bw) + f * nb;
    if (g.x_lds) {
        for (long long t = tid; t < nb; t += FITB_THREADS) st[t] = X[t];
        X = st;
        st += nb;
    }
    double* PAb = st;
    double* CAb = PAb + n;
    double* dSb = CAb + n;
    const float* Yr = g.Yr + m0 + c0;                               // Y_slice[l, m] = Yr[l * Mtot + m] = Yc[m * L + l]
    const float* Yc = g.Yc + (m0 + c0) * L;
    const int lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, q16 = lane >> 4;
    const int nbu = (H + 15) >> 4;
    const double sig = pub[0], Lg = (double)L;
    for (long long t = tid; t < n; t += FITB_THREADS) CAb[t] = g.CA[o + t];
    if (tid < 6) pri_s[tid] = g.priors4[f * 9 + tid];
    if (tid < H) {
        if constexpr (ROWS) {
            double v = pub[FITS_PUB + 2 * h2 + tid];
            v += Lg * sig * SBp[tid * H + tid];
            v_s[tid] = v;
        } else {
            v_s[tid] = sig * Gp[tid * H + tid] + Lg * SBp[tid * H + tid];
        }
    }
    if (tid == 0) bad_s = 0;
    __syncthreads();
    fitb_product<NP>(nc, L, Yr, g.Mtot, Yc, L, X, H, PAb);
    __syncthreads();
    int bad = 0;
    double gs[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) gs[k] = 0.0;
    if constexpr (!FULL) {
        for (long long t = tid; t < n; t += FITB_THREADS) {
            const long long m = t / H, mg = c0 + m, tg = t0 + t;   // mg, tg: the entry's column and index in the FIT
            const int h = (int)(t - m * H);
            const long long vi = !g.compat ? h : (tg < H ? tg : (tg - H) / (Mb - 1));   // repeat(v, inner = M_b - 1) after the first H
            const double prec = v_s[vi] + CAb[t];
            bad |= !isfinite(prec);
            const double ds = 1.0 / prec, a = (mg < M0f && h >= hmask) ? 0.0 : (ROWS ? ds * PAb[t] : sig * ds * PAb[t]);
            PAb[t] = a;
            dSb[t] = ds;
            const int grp = h < H0 ? 0 : (mg < M0f ? 1 : 2);
            const double be = pri_s[2 * grp + 1] + 0.5 * (a * a + ds), ca = (pri_s[2 * grp] + 0.5) / be;
            g.A[o + t] = a;
            g.dS[o + t] = ds;
            g.CA[o + t] = ca;
            g.beta[o + t] = be;
            const double lb = log(be);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                gs[2 * k] += grp == k ? lb : 0.0;
                gs[2 * k + 1] += grp == k ? ca : 0.0;
            }
        }
        __syncthreads();
        fitb_chunk_reduce(H, nc, part, SAo, [&](int h, long long m) { return dSb[m * H + h]; });
    } else {
        double* W = lds_fs + (size_t)w * NP * LD;
        double* pvec = lds_fs + (size_t)NW * NP * LD + w * NP;
        f64x4 g0[NUP], acc[NUP];
        {   // G = B'B + L SigmaB (ROWS: B'diag(s)B + L mean(s) SigmaB): its upper blocks in the MFMA's C/D layout (zero beyond H)
            int u = 0;
#pragma unroll
            for (int I = 0; I < NBK; ++I)
#pragma unroll
                for (int J = I; J < NBK; ++J, ++u)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i = 16 * I + q16 + 4 * r, j = 16 * J + c16;
                        if constexpr (ROWS) g0[u][r] = (i < H && j < H) ? Gp[i * H + j] + Lg * sig * SBp[i * H + j] : 0.0;
                        else g0[u][r] = (i < H && j < H) ? Gp[i * H + j] + Lg * SBp[i * H + j] : 0.0;
                        acc[u][r] = 0.0;
                    }
        }
        for (long long m = w; m < nc; m += NW) {
            const long long mg = c0 + m;
            {
                double cad[NBK];
#pragma unroll
                for (int I = 0; I < NBK; ++I) {
                    const int i = 16 * I + c16;
                    cad[I] = i < H ? CAb[m * H + i] : 1.0;
                }
                int u = 0;
#pragma unroll
                for (int I = 0; I < NBK; ++I)
#pragma unroll
                    for (int J = I; J < NBK; ++J, ++u) {
                        f64x4 x;
                        if constexpr (ROWS) x = g0[u];
                        else x = sig * g0[u];
                        if (I == J) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) x[r] += (q16 == (c16 & 3) && r == (c16 >> 2)) ? cad[I] : 0.0;
                        }
                        if (I < nbu && J < nbu) blk_st_rows(W, LD, I, J, lane, x);
                    }
            }
            if (lane < NP) pvec[lane] = lane < H ? PAb[m * H + lane] : 0.0;
            PivAcc pv;
            blk_sweep<NBK, 1>(W, LD, nbu, 0, lane, pv);            // W's upper blocks = -Sigma_m
            bad |= pv.bad;
            const int i = lane < H ? lane : 0;
            double sm = 0.0;
            const int nj = 16 * nbu;
            for (int j = 0; j < nj; ++j) {
                const int lo = j < i ? j : i, hi = j < i ? i : j;
                sm += W[lo * LD + hi] * pvec[j];
            }
            const double a = (lane < H && !(mg < M0f && lane >= hmask)) ? (ROWS ? -sm : -sig * sm) : 0.0;
            if (lane < H) {
                const long long t = m * H + lane;
                const double ds = -W[lane * LD + lane];
                PAb[t] = a;
                const int grp = lane < H0 ? 0 : (mg < M0f ? 1 : 2);
                const double be = pri_s[2 * grp + 1] + 0.5 * (a * a + ds), ca = (pri_s[2 * grp] + 0.5) / be;
                g.A[o + t] = a;
                g.dS[o + t] = ds;
                g.CA[o + t] = ca;
                g.beta[o + t] = be;
                const double lb = log(be);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    gs[2 * k] += grp == k ? lb : 0.0;
                    gs[2 * k + 1] += grp == k ? ca : 0.0;
                }
            }
            {
                int u = 0;
#pragma unroll
                for (int I = 0; I < NBK; ++I)
#pragma unroll
                    for (int J = I; J < NBK; ++J, ++u)
                        if (I < nbu && J < nbu) acc[u] -= blk_ld_rows(W, LD, I, J, lane);
            }
        }
        {   // the slice's share of SigmaA = the waves' sums folded through their images (fixed order)
            int u = 0;
#pragma unroll
            for (int I = 0; I < NBK; ++I)
#pragma unroll
                for (int J = I; J < NBK; ++J, ++u)
                    if (I < nbu && J < nbu) blk_st_rows(W, LD, I, J, lane, acc[u]);
        }
        __syncthreads();
        for (int t = tid; t < h2; t += FITB_THREADS) {
            const int i = t / H, j = t % H;
            const int lo = i <= j ? i : j, hi = i <= j ? j : i;
            double s = 0.0;
#pragma unroll
            for (int ww = 0; ww < NW; ++ww) s += lds_fs[(size_t)ww * NP * LD + lo * LD + hi];
            SAo[t] = s;
        }
        __syncthreads();
    }
    if (g.est_priors) {
#pragma unroll
        for (int k = 0; k < 6; ++k) gs[k] = fitb_sum(gs[k], red);
    }
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) gso[k] = gs[k];
    }
    fitb_chunk_reduce(h2, nc, part, AAo, [&](int e, long long m) { return PAb[m * H + e / H] * PAb[m * H + e % H]; });
    fitb_product<NP>(L, nc, Yc, L, Yr, g.Mtot, PAb, H, Qo);
    if (bad) bad_s = 1;                                             // (same value from every writer)
    __syncthreads();
    if (tid == 0) gso[6] = bad_s ? 1.0 : 0.0;
}

template <int NBK, bool ROWS>
__global__ __launch_bounds__(FITB_THREADS) void fit_fold_kernel(FitSplitArgs g) {
    extern __shared__ __attribute__((aligned(16))) double lds_ff[];
    __shared__ double part[1024];
    __shared__ double red[16];
    __shared__ double cb_s[32], dl_s[32], vec_s[64], pri_s[9], gs_s[6];
    __shared__ int bad_s;
    constexpr int NP = 16 * NBK, LD = NP + 2;
    const int f = blockIdx.x;
    if (g.done[f]) return;
    const int H = g.H, H0 = g.H0, tid = threadIdx.x, h2 = H * H;
    const long long L = g.L, b = g.fit_bag[f], m0 = g.col_off[b], Mb = g.col_off[b + 1] - m0, nb = L * H;
    const long long M0f = g.M0[f], s0 = g.fit_sl0[f], s1 = g.fit_sl0[f + 1], SS = fits_slot_doubles(L, H);
    double* pub = g.pub + (long long)f * fits_pub_doubles(H);
    const double* slot0 = g.slot + s0 * SS;
    const int nsl = (int)(s1 - s0);
    double* Wk = lds_ff;
    double* BB = Wk + NP * LD;
    double* AA = BB + h2;
    double* SBm = AA + h2;
    double* Dm = SBm + h2;
    double* E = Dm + h2;
    double* st = E + 4 * h2;
    double* Bg = g.Bw + (long long)f * nb;
    double* Qg = g.Qw + (long long)f * nb;
    double* Bl = g.b_lds ? st : Bg;
    double* Ql = g.b_lds ? st + nb : Qg;
    double* sv = nullptr;
    double* yn = nullptr;
    if constexpr (ROWS) {
        sv = g.sigma + (long long)f * L;
        yn = g.yn + (long long)f * L;
    }
    const int lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nbu = (H + 15) >> 4;
    const double eta = g.eta[f], zeta0 = g.zeta0[f], gam = g.gamma[f], delta0 = g.delta0[f], Lg = (double)L;
    double sig = pub[0], zeta = 0.0;
    const double yy = pub[1];
    double nrmB = pub[2];
    int it = (int)pub[5];
    // ---- the slices' partials, in slice order -------------------------------------------------------------------------------------------
    if (g.b_lds)
        for (long long t = tid; t < nb; t += FITB_THREADS) Bl[t] = Bg[t];
    for (int t = tid; t < h2; t += FITB_THREADS) {
        const int i = t / H, j = t % H;
        SBm[t] = g.SB[(long long)f * h2 + t];
        BB[t] = pub[FITS_PUB + t];
        double a = 0.0, s = 0.0;
        for (int k = 0; k < nsl; ++k) a += slot0[k * SS + t];
        if (g.full) {
            for (int k = 0; k < nsl; ++k) s += slot0[k * SS + h2 + t];
        } else if (i == j) {
            for (int k = 0; k < nsl; ++k) s += slot0[k * SS + h2 + i];
        }
        AA[t] = a + s;
        g.SA[(long long)f * h2 + t] = s;
    }
    for (long long t = tid; t < nb; t += FITB_THREADS) {
        double q = 0.0;
        for (int k = 0; k < nsl; ++k) q += slot0[k * SS + 2 * h2 + t];
        Ql[t] = q;
    }
    if (tid < 7) {
        double s = 0.0;
        for (int k = 0; k < nsl; ++k) s += slot0[k * SS + 2 * h2 + nb + tid];
        if (tid < 6) gs_s[tid] = s;
        else bad_s = s != 0.0;
    }
    if (tid < H) {
        cb_s[tid] = g.CB[(long long)f * H + tid];
        dl_s[tid] = 0.0;
    }
    if (tid < 9) pri_s[tid] = g.priors4[(long long)f * 9 + tid];
    int bad = 0;
    __syncthreads();
    // ---- updateB! (fit_batch_kernel from its Wk on) -------------------------------------------------------------------------------------
    for (int t = tid; t < NP * NP; t += FITB_THREADS) {
        const int i = t / NP, j = t % NP;
        Wk[i * LD + j] = (i < H && j < H) ? sig * AA[i * H + j] + (i == j ? cb_s[i] : 0.0) : (i == j ? 1.0 : 0.0);   // (ROWS: mean(s))
    }
    __syncthreads();
    if (w == 0) {
        PivAcc pv;
        blk_sweep<NBK, 1>(Wk, LD, nbu, 0, lane, pv);
        bad |= pv.bad;
    }
    __syncthreads();
    for (int t = tid; t < h2; t += FITB_THREADS) {
        const int i = t / H, j = t % H;
        SBm[t] = -(i <= j ? Wk[i * LD + j] : Wk[j * LD + i]);
    }
    __syncthreads();
    double trG = 0.0;                                               // ROWS: sum G o SigmaB, G = A'A + SigmaA
    if constexpr (ROWS) {
        for (int t = tid; t < h2; t += FITB_THREADS) trG += AA[t] * SBm[t];
        trG = fitb_sum(trG, red);
    }
    double bq = 0.0, ssum = 0.0;
    for (long long l = tid; l < L; l += FITB_THREADS) {
        double q[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) q[j] = j < H ? Ql[l * H + j] : 0.0;
        double sl = sig, rl = 0.0;
        if constexpr (ROWS) sl = sv[l];
        for (int h = 0; h < H; ++h) {
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < NP; ++j)
                if (j < H) s += q[j] * SBm[j * H + h];
            const double bn = sl * s, bo = Bl[l * H + h];
            if constexpr (ROWS) rl += bn * Ql[l * H + h];
            else bq += bn * Ql[l * H + h];
            Bl[l * H + h] = bn;
            Ql[l * H + h] = bo - bn;
        }
        if constexpr (ROWS) {
#pragma unroll
            for (int j = 0; j < NP; ++j) q[j] = j < H ? Bl[l * H + j] : 0.0;
            double quad = 0.0;
            for (int h = 0; h < H; ++h) {
                double s = 0.0;
#pragma unroll
                for (int j = 0; j < NP; ++j)
                    if (j < H) s += q[j] * AA[j * H + h];
                quad += s * Bl[l * H + h];
            }
            const double zv = zeta0 + 0.5 * yn[l] - rl + 0.5 * (quad + trG), sn = eta / zv;
            bad |= !isfinite(zv) || !isfinite(sn);
            g.zeta[(long long)f * L + l] = zv;
            sv[l] = sn;
            ssum += sn;
        }
    }
    if constexpr (ROWS) sig = fitb_sum(ssum, red) / Lg;
    else bq = fitb_sum(bq, red);
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
    // ---- updateCB!, updateSigma!, est_priors ---------------------------------------------------------------------------------------------
    if (g.est_cb && tid < H) {
        const double dl = delta0 + 0.5 * (BB[tid * H + tid] + SBm[tid * H + tid]);
        dl_s[tid] = dl;
        cb_s[tid] = gam / dl;
    }
    if constexpr (!ROWS) {
        double tr = 0.0;
        for (int t = tid; t < h2; t += FITB_THREADS) tr += AA[t] * (BB[t] + Lg * SBm[t]);
        tr = fitb_sum(tr, red);
        zeta = zeta0 + 0.5 * yy - bq + 0.5 * tr;
        sig = eta / zeta;
    }
    if (g.est_priors && tid == 0) {
        const double ng[3] = {(double)Mb * (double)H0, (double)M0f * (double)(H - H0), (double)(Mb - M0f) * (double)(H - H0)};
        for (int grp = 0; grp < 3; ++grp) {
            const double nn = ng[grp];
            pri_s[6 + grp] = pri_s[2 * grp] + 0.5;
            if (!(nn > 0.0)) continue;
            const double a_post = pri_s[2 * grp] + 0.5;
            const double y = log(pri_s[2 * grp + 1]) + digamma_dev(a_post) - gs_s[2 * grp] / nn;
            double a_new = pri_s[2 * grp];
            if (isfinite(y) && y < 23.025850929890457 && y > -1e10) {
                a_new = digamma_inv_dev(y);
                a_new = fmin(fmax(a_new, 1e-10), 1e10);
            }
            pri_s[2 * grp] = a_new;
            pri_s[2 * grp + 1] = nn * a_new / gs_s[2 * grp + 1];
        }
    }
    // ---- d, the stop test ----------------------------------------------------------------------------------------------------------------
    if (sB != 1.0)
        fitb_chunk_reduce(h2, L, part, AA, [&](int e, long long l) { return (sB * Bl[l * H + e / H]) * (sB * Bl[l * H + e % H]); });
    double lamD, lamBn;
    fitb_lambda_max(Dm, sB != 1.0 ? AA : BB, H, g.spectral, E, vec_s, lamD, lamBn);
    const double d = (sqrt(lamD) / sD) / nrmB;
    nrmB = sqrt(lamBn) / sB;
    if (bad) bad_s = 1;                                             // (same value from every writer)
    __syncthreads();                                                // (also publishes pri_s, cb_s)
    const int status = bad_s ? 1 : 0;
    if (tid == 0 && g.trace) {
        g.trace[((long long)f * g.niter + it) * 2] = d;
        g.trace[((long long)f * g.niter + it) * 2 + 1] = sig;
    }
    ++it;
    const bool stop = status || !(d > g.eps) || it >= g.niter;
    // ---- outputs, and what the next column pass reads --------------------------------------------------------------------------------------
    for (long long t = tid; t < nb; t += FITB_THREADS) {
        const long long l = t / H;
        const int h = (int)(t - l * H);
        g.B[(long long)f * nb + (long long)h * L + l] = Bl[t];
        if (g.b_lds) Bg[t] = Bl[t];
    }
    for (int t = tid; t < h2; t += FITB_THREADS) {
        g.SB[(long long)f * h2 + t] = SBm[t];
        pub[FITS_PUB + t] = BB[t];
    }
    if (tid < H) {
        g.CB[(long long)f * H + tid] = cb_s[tid];
        if (g.est_cb) g.delta[(long long)f * H + tid] = dl_s[tid];
    }
    if (tid < 9) g.priors4[(long long)f * 9 + tid] = pri_s[tid];
    if constexpr (ROWS) {
        if (!stop) {
            // diag(s) B, v_h = sum_l (s_l B_lh)^2 and B'diag(s)B of the next sweep (Ql is free: dB'dB has consumed its B_old - B)
            for (long long t = tid; t < nb; t += FITB_THREADS) {
                const double x = sv[t / H] * Bl[t];
                Ql[t] = x;
                if (g.b_lds) Qg[t] = x;
            }
            __syncthreads();
            fitb_chunk_reduce(H, L, part, pub + FITS_PUB + 2 * h2, [&](int h, long long l) { return Ql[l * H + h] * Ql[l * H + h]; });
            if (g.full)
                fitb_chunk_reduce(h2, L, part, pub + FITS_PUB + h2, [&](int e, long long l) {
                    const int i = e / H, j = e % H;
                    return Ql[l * H + (i < j ? i : j)] * Bl[l * H + (i < j ? j : i)];
                });
        }
    }
    if (tid == 0) {
        if constexpr (!ROWS) {
            g.sigma[f] = sig;
            g.zeta[f] = zeta;
        }
        pub[0] = sig;
        pub[2] = nrmB;
        pub[5] = (double)it;
        g.iters[f] = it;
        g.dlast[f] = d;
        g.status[f] = status;
        g.done[f] = stop ? 1 : 0;
    }
}

}  // namespace vbmf
