// fit_batch_kernels.hpp -- many small ARD-sparse / two-group fits in one launch (vbmf_sparse_fit_batched; the restart loops of
// examples/mil_util.jl:124-145, 347-379 and the folds x classes around them in one call), and with LOCAL = true the three-group and
// label-masked fits on concatenated matrices [Y0 Y1] (vbmf_local_fit_batched; src/vbmf_trial.jl:528-604, examples/mil_util.jl:302-320).
//
// The context's Y holds the bags side by side: bag b = columns col_off[b] .. col_off[b+1]-1.  fit_stage_kernel copies Y as stored (the
// pass-2 tiles) ONCE per call into two dense fp32 planes, row-major Yr[l][m] and column-major Yc[m][l], so that each of the two products
// of a sweep has a plane it reads with neighbouring lanes on neighbouring addresses.  Then ONE launch of fit_batch_kernel runs the whole
// `while i <= niter && d > eps` loop of every fit, one 512-thread workgroup per fit, everything in fp64 (Y widened on load).  Fit f works
// on bag fit_bag[f]; restarts share a bag.  Per sweep, in the reference's order (src/vbmf_sparse.jl:369-377, src/vbmf_dual.jl:476-495):
//   updateA!      P = Y_b'B; diagonal form (:204-240, QS1 under VBMF_COMPAT_SPARSE_REPEAT with the fit's own M_b) or full_cov (:178-202:
//                 one column per wavefront, blk_sweep in the wave's LDS image), as in sparse_batch_kernels.hpp
//   updateCA!     fused behind updateA! (updateB! reads neither CA nor beta): per-column (alpha_h, beta0_h) from the fit's two prior pairs
//   updateB!      SigmaB = inv(diag(CB) + sigma (A'A + SigmaA)) by one wave's blk_sweep, Q = Y_b A, B = sigma Q SigmaB (:263-266)
//   updateCB!     delta_h = delta0 + (B_h'B_h + SigmaB_hh) / 2, CB = gamma / delta (:295-300)
//   updateSigma!  zeta = zeta0 + ||Y_b||^2 / 2 - sum B o Q + tr((A'A + SigmaA)(B'B + L SigmaB)) / 2 (:317-321)
//   est_priors    group_priors_kernel's fit on thread 0 (src/vbmf_dual.jl:393-434)
//   d             norm(B_old - B) / norm(B_old): operator 2-norms under VBMF_COMPAT_SPECTRAL_DELTA (src/util.jl:27-29), lambda_max of the
//                 two H x H Grams by fp64 repeated squaring + a Rayleigh quotient on the original matrix; Frobenius norms otherwise
// The fit leaves the loop when !(d > eps) (a NaN d stops it) or when it met a non-finite precision or a bad pivot (status = 1).
// State: B, Q (L x H) and PA, CA, dS (M_b x H; P and A share storage) in LDS when they fit under FITB_LDS_CAP, else in the fit's own
// slices of the scratch buffer.  Every sum's order is fixed by (L, M_b, H): chunked partials folded in chunk order, xor-butterflies over
// a lane group whose width depends on the row count alone (LOCAL: and by H0, M0 for the per-group sums).  No atomics, no hand-off
// between workgroups.
//
// ROWS = true (vbmf_rows_fit_batched; with LOCAL only): the heteroscedastic noise model, diag_var = true, of the same three families
// (src/vbmf_sparse.jl:180-193, 207-230, 256-261, 309-315; src/vbmf_dual.jl:222-299, 370-386; src/vbmf_trial.jl:256-334, 419-435).  A fit
// holds s = sigmaVecHat and the row norms ||Y_b[l,:]||^2 (L doubles each) behind the H x H matrices, in LDS when they fit, else in its
// slices of g.sigma and g.yn.  Per sweep Ql = diag(s) B is formed where Ql is free (its B_old - B went into dB'dB), and
//   updateA!      P = Y_b' Ql, no factor sigmaHat on a; diagonal form: v_h = sum_l Ql_lh^2 + L mean(s) SigmaB_hh -- s enters SQUARED
//                 (:211 takes norm2 of the product); full_cov: K_m = sum_l Ql_li B_lj + L mean(s) SigmaB + diag(CA[m,:]), s to the first power
//   updateB!      SigmaB = inv(diag(CB) + mean(s) (A'A + SigmaA)), B = diag(s) Q SigmaB
//   updateSigma!  fused into the row-per-thread loop that forms B: zetaVec_l = zeta0 + ||Y_b[l,:]||^2 / 2 - sum_h Q_lh B_lh
//                 + (b_l'G b_l + sum G o SigmaB) / 2, s_l = etaVec / zetaVec_l; sigmaHat and zeta do not exist here
// The second trace column is mean(s).  A zetaVec_l or s_l that is not finite sets status = 1 like a non-finite precision.
#pragma once
#include <type_traits>
#include "common.hpp"
#include "ctrl_kernels.hpp"
#include "blk_inverse.hpp"
#include "score_kernels.hpp"
#include "sparse_kernels.hpp"

namespace vbmf {

constexpr int FITB_THREADS = 512, FITB_NW = FITB_THREADS / 64;
constexpr size_t FITB_LDS_CAP = 144 * 1024;       // dynamic LDS a fit may use (the static arrays take 9 KiB more)
constexpr int FITB_EIG_NSQ = 40;                  // squarings at most: (1 - r) r^(2^41) < 2e-13 for any eigenvalue ratio r

// doubles of dynamic LDS in front of a fit's state: the inverse images (one, or one per wave with its p_m vector) and eight
// H x H matrices (B'B, A'A + SigmaA, SigmaB, dB'dB and the two ping-pong pairs of the eigenvalue iteration)
__host__ __device__ constexpr int fitb_fixed_doubles(bool full, int NBK, int H) {
    return (full ? FITB_NW * (16 * NBK) * (16 * NBK + 2) + FITB_NW * 16 * NBK : (16 * NBK) * (16 * NBK + 2)) + 8 * H * H;
}
// where a fit's state lives: 2 = everything in LDS, 1 = B and Q only, 0 = nothing
// rows (ROWS = true): the fit's two L-vectors (s, the row norms) come off the room first; they stay in LDS whenever they fit at all
__host__ __device__ constexpr bool fitb_rows_in_lds(bool full, int NBK, long long L, int H) {
    return 2 * L <= (long long)(FITB_LDS_CAP / 8) - fitb_fixed_doubles(full, NBK, H);
}
__host__ __device__ constexpr int fitb_placement(bool full, int NBK, long long L, long long Mb, int H, bool rows = false) {
    const long long room = (long long)(FITB_LDS_CAP / 8) - fitb_fixed_doubles(full, NBK, H)
                           - (rows && fitb_rows_in_lds(full, NBK, L, H) ? 2 * L : 0);
    return 2 * L * H + 3 * Mb * H <= room ? 2 : (2 * L * H <= room ? 1 : 0);
}
__host__ __device__ constexpr long long fitb_lds_doubles(bool full, int NBK, long long L, long long Mb, int H, bool rows = false) {
    const int pl = fitb_placement(full, NBK, L, Mb, H, rows);
    return fitb_fixed_doubles(full, NBK, H) + (rows && fitb_rows_in_lds(full, NBK, L, H) ? 2 * L : 0) + (pl >= 1 ? 2 * L * H : 0)
           + (pl == 2 ? 3 * Mb * H : 0);
}

// Y as stored -> Yr[l * M + m] and Yc[m * L + l] (fp32: exact for both storage types)
template <int MODE>
__global__ __launch_bounds__(256) void fit_stage_kernel(const uint4* __restrict__ Y2, int KSpad, long long L, long long M,
                                                        float* __restrict__ Yr, float* __restrict__ Yc) {
    const long long n = L * M, stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) {
        const long long l = t / M, m = t - l * M;
        Yr[t] = score_y_at<MODE>(Y2, KSpad, l, m);
    }
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) {
        const long long m = t / L, l = t - m * L;
        Yc[t] = score_y_at<MODE>(Y2, KSpad, l, m);
    }
}

struct FitArgs {
    const float* Yr; const float* Yc; long long L, Mtot;
    const long long* col_off; const long long* fit_bag; const long long* fit_off;   // fit_off[f]: columns of the fits before f
    int H, H0, niter, compat, spectral, est_cb, est_priors;
    double eps;
    const double* gamma; const double* delta0; const double* eta; const double* zeta0;   // nfits
    double* priors4;                               // nfits x 4 (FitLocalArgs: nfits x 9)
    double* B; double* SB; double* CB; double* sigma; double* CA;                        // in / out
    double* delta; double* zeta; double* beta; double* dS; double* SA; double* A;       // out
    double* Bw; double* Qw;                        // nfits x L x H each: working B (row-major) and Q for fits whose B is not in LDS
    long long* iters; double* dlast; long long* status; double* trace;
};

// vbmf_local_fit_batched: the same sweep with two per-entry rules on A (M0[f] = the fit's leading rows, the negative instances)
//   three prior groups (src/vbmf_trial.jl:357-400)  entry (m, h): group 1 if h < H0, group 2 if m < M0[f], else group 3; `priors4` then
//                 holds nine doubles per fit in vbmf_trial_get_priors' order (three pairs in/out, the three posterior shapes out)
//   prefix mask (src/vbmf_sparse.jl:245)            mask_H1 > 0: a(m, h) = 0 for m < M0[f], h >= H - mask_H1, before anything reads it
struct FitLocalArgs : FitArgs {
    const long long* M0; int mask_H1;
};
// vbmf_rows_fit_batched: sigma is nfits x L (in / out), zeta nfits x L (out), eta[f] = eta0 + M_b / 2; yn: nfits x L, the row norms of
// the fits whose L-vectors are not in LDS
struct FitRowsArgs : FitLocalArgs {
    double* yn;
};

// sum over the workgroup's 512 threads, lanes first, then the eight waves in order (block_sum of ctrl_kernels.hpp folds the first 256
// threads of a 512-thread launch only: the streaming kernel's control half).  red: FITB_NW doubles; two barriers.
__device__ __forceinline__ double fitb_sum(double v, double* red) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < FITB_NW; ++i) s += red[i];
    return s;
}

__device__ __forceinline__ double fitb_max(double v, double* red) {
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int i = 1; i < FITB_NW; ++i) s = fmax(s, red[i]);
    return s;
}
// A matrix whose largest entry m lies this far from 1 loses its Gram to underflow / overflow (the reference's norm is an SVD of the matrix
// itself, which does not): its norm is then taken from the Gram of the matrix scaled by a power of two
__device__ __forceinline__ bool fitb_far(double m) { return m > 0.0 && isfinite(m) && (m < 0x1p-400 || m > 0x1p400); }
__device__ __forceinline__ double fitb_scale(double m) {
    if (!fitb_far(m)) return 1.0;
    int e;
    frexp(m, &e);
    return ldexp(1.0, -e < 1000 ? -e : 1000);
}

// out[item] = sum over rows of f(item, row), nitem <= 1024: the rows are cut into 512 / nitem chunks summed side by side and folded
// in chunk order.  part: 1024 doubles.  Ends with a barrier (out is published, part is free).
template <class F>
__device__ __forceinline__ void fitb_chunk_reduce(int nitem, long long rows, double* part, double* out, F f) {
    const int nch = nitem >= FITB_THREADS ? 1 : FITB_THREADS / nitem;
    const long long per = (rows + nch - 1) / nch;
    for (int t = threadIdx.x; t < nitem * nch; t += FITB_THREADS) {
        const int item = t % nitem, ch = t / nitem;
        const long long r0 = ch * per, r1 = r0 + per < rows ? r0 + per : rows;
        double s = 0.0;
        for (long long r = r0; r < r1; ++r) s += f(item, r);
        part[t] = s;
    }
    __syncthreads();
    for (int item = threadIdx.x; item < nitem; item += FITB_THREADS) {
        double s = 0.0;
        for (int ch = 0; ch < nch; ++ch) s += part[ch * nitem + item];
        out[item] = s;
    }
    __syncthreads();
}

// out[r * H + h] = sum_k y(r, k) X[k * H + h] for r < R: T lanes per row (T = the power of two that fills the workgroup, from R alone)
// split k, an xor-butterfly folds them.  y(r, k) = yc[k * ldc + r] when T = 1 (neighbouring lanes = neighbouring r), else
// yk[r * ldk + k] (neighbouring lanes = neighbouring k).  YT: float (the planes of Y) or double (fit_basic_gram_kernels.hpp's K).
// Every thread of the workgroup must call it.
template <int HP, class YT>
__device__ __forceinline__ void fitb_product(long long R, long long K, const YT* __restrict__ yc, long long ldc,
                                             const YT* __restrict__ yk, long long ldk, const double* X, int H, double* out) {
    int T = 1;
    while (T < 64 && R * T < FITB_THREADS) T <<= 1;
    const long long items = R * T;
    for (long long base = 0; base < items; base += FITB_THREADS) {
        const long long it = base + threadIdx.x;
        const bool on = it < items;
        const long long r = on ? it / T : 0;
        const int s = (int)(it & (T - 1));
        double acc[HP];
#pragma unroll
        for (int h = 0; h < HP; ++h) acc[h] = 0.0;
        if (on) {
            for (long long k = s; k < K; k += T) {
                const double y = (double)(T == 1 ? yc[k * ldc + r] : yk[r * ldk + k]);
                const double* x = X + k * H;
#pragma unroll
                for (int h = 0; h < HP; ++h)
                    if (h < H) acc[h] = fma(y, x[h], acc[h]);
            }
        }
        for (int off = T >> 1; off > 0; off >>= 1) {
#pragma unroll
            for (int h = 0; h < HP; ++h)
                if (h < H) acc[h] += __shfl_xor(acc[h], off);
        }
        if (on && s == 0) {
#pragma unroll
            for (int h = 0; h < HP; ++h)
                if (h < H) out[r * H + h] = acc[h];
        }
    }
}

// lambda_max of the symmetric PSD H x H matrices M0 and M1 (spectral = 0: their traces), every thread gets both.  E: 4 H^2 doubles.
// T <- T T / tr(T T) drives T to the dominant eigenprojector; its largest-diagonal column, polished by two power steps on the original
// matrix, gives lambda as a Rayleigh quotient (error quadratic in the vector's).  A zero matrix gives 0, a NaN propagates.
__device__ __forceinline__ void fitb_lambda_max(const double* M0, const double* M1, int H, int spectral, double* E, double* vec,
                                                double& lam0, double& lam1) {
    const int h2 = H * H;
    double tr[2] = {0.0, 0.0};
    for (int i = 0; i < H; ++i) { tr[0] += M0[i * H + i]; tr[1] += M1[i * H + i]; }
    const bool run0 = spectral && tr[0] > 0.0 && isfinite(tr[0]), run1 = spectral && tr[1] > 0.0 && isfinite(tr[1]);
    lam0 = tr[0]; lam1 = tr[1];
    if (!run0 && !run1) return;                                     // (uniform: every thread read the same traces)
    double* cur = E;
    double* nxt = E + 2 * h2;
    for (int t = threadIdx.x; t < 2 * h2; t += FITB_THREADS) {
        const int w = t >= h2, e = t - w * h2;
        cur[t] = (w ? run1 : run0) ? (w ? M1[e] : M0[e]) / tr[w] : (e == 0 ? 1.0 : 0.0);   // (a skipped matrix: a projector already)
    }
    __syncthreads();
    double sc[2] = {1.0, 1.0};                                      // cur * sc has trace 1 (the scaling is applied by the next product)
    for (int sq = 0; sq < FITB_EIG_NSQ; ++sq) {
        for (int t = threadIdx.x; t < 2 * h2; t += FITB_THREADS) {
            const int w = t >= h2, e = t - w * h2, i = e / H, j = e - i * H;
            const double* c = cur + w * h2;
            double s = 0.0;
            for (int k = 0; k < H; ++k) s += c[i * H + k] * c[k * H + j];
            nxt[t] = s * (sc[w] * sc[w]);
        }
        __syncthreads();
        double t0 = 0.0, t1 = 0.0;                                  // tr(T T) = ||T||_F^2 with tr(T) = 1: -> 1 iff T is a rank-1 projector
        for (int i = 0; i < H; ++i) { t0 += nxt[i * H + i]; t1 += nxt[h2 + i * H + i]; }
        double* tmp = cur; cur = nxt; nxt = tmp;                    // (the next product writes what every thread has finished reading)
        if (!(t0 > 0.0) || !(t1 > 0.0)) break;                      // underflow or NaN (uniform): the quotient below reports it
        sc[0] = 1.0 / t0;
        sc[1] = 1.0 / t1;
        if (t0 > 1.0 - 1e-14 && t1 > 1.0 - 1e-14) break;            // (uniform)
    }
    // per matrix: v = the column with the largest diagonal entry, two power steps on the original, lambda = v'Mv / v'v
    for (int w = 0; w < 2; ++w) {
        if (!(w ? run1 : run0)) continue;
        const double* Mo = w ? M1 : M0;
        const double* c = cur + w * h2;
        int arg = 0;
        for (int i = 1; i < H; ++i) if (c[i * H + i] > c[arg * H + arg]) arg = i;
        double* v0 = vec;
        double* v1 = vec + 32;
        if (threadIdx.x < H) v0[threadIdx.x] = c[threadIdx.x * H + arg];
        __syncthreads();
        for (int st = 0; st < 2; ++st) {
            if (threadIdx.x < H) {
                double s = 0.0;
                for (int j = 0; j < H; ++j) s += Mo[threadIdx.x * H + j] * v0[j];
                v1[threadIdx.x] = s / tr[w];
            }
            __syncthreads();
            double* tmp = v0; v0 = v1; v1 = tmp;
        }
        double num = 0.0, den = 0.0;
        for (int i = 0; i < H; ++i) {
            double s = 0.0;
            for (int j = 0; j < H; ++j) s += Mo[i * H + j] * v0[j];
            num += v0[i] * s;
            den += v0[i] * v0[i];
        }
        const double lam = num / den;
        if (w) lam1 = lam; else lam0 = lam;
        __syncthreads();
    }
}

template <int NBK, bool FULL, bool LOCAL = false, bool ROWS = false>
__global__ __launch_bounds__(FITB_THREADS) void fit_batch_kernel(
    std::conditional_t<ROWS, FitRowsArgs, std::conditional_t<LOCAL, FitLocalArgs, FitArgs>> g) {
    static_assert(LOCAL || !ROWS, "the row-noise sweep is built on the three-group sweep");
    extern __shared__ __attribute__((aligned(16))) double lds_fb[];
    __shared__ double part[1024];
    __shared__ double red[16];
    __shared__ double v_s[32], al_s[32], b0_s[32], sa_s[32], cb_s[32], dl_s[32], vec_s[64];
    constexpr int NP = 16 * NBK, LD = NP + 2, NUP = NBK * (NBK + 1) / 2, NW = FITB_NW;
    constexpr int NPRI = LOCAL ? 9 : 4, NGS = LOCAL ? 6 : 4;      // doubles of priors per fit; running sums (log beta, CA per group)
    __shared__ double pri_s[NPRI];
    __shared__ int bad_s;
    const int f = blockIdx.x, H = g.H, H0 = g.H0, tid = threadIdx.x, h2 = H * H;
    const long long L = g.L, b = g.fit_bag[f], m0 = g.col_off[b], Mb = g.col_off[b + 1] - m0;
    const long long n = Mb * H, o = g.fit_off[f] * H, nb = L * H;
    const int place = fitb_placement(FULL, NBK, L, Mb, H, ROWS);
    long long M0f = 0;                                              // LOCAL: rows m < M0f are the fit's negative instances
    int hmask = H;                                                  // LOCAL: columns h >= hmask of those rows are zeroed
    if constexpr (LOCAL) {
        M0f = g.M0[f];
        hmask = H - g.mask_H1;
    }
    // dynamic LDS: [images (+ p_m, a_m) | B'B | A'A + SigmaA | SigmaB | dB'dB | eigen 4 H^2 | ROWS: s, row norms | B, Q | PA, CA, dS]
    double* Wk = lds_fb;                                            // the image of updateB!'s inverse (full_cov: wave 0's)
    double* BB = lds_fb + (fitb_fixed_doubles(FULL, NBK, H) - 8 * h2);
    double* AA = BB + h2;
    double* SBm = AA + h2;
    double* Dm = SBm + h2;
    double* E = Dm + h2;
    double* st = E + 4 * h2;
    double* sv = nullptr;                                           // ROWS: s = sigmaVecHat and ||Y_b[l,:]||^2
    double* yn = nullptr;
    if constexpr (ROWS) {
        const bool in_lds = fitb_rows_in_lds(FULL, NBK, L, H);
        sv = in_lds ? st : g.sigma + (long long)f * L;
        yn = in_lds ? st + L : g.yn + (long long)f * L;
        if (in_lds) st += 2 * L;
    }
    double* Bl = place >= 1 ? st : g.Bw + (long long)f * nb;
    double* Ql = place >= 1 ? st + nb : g.Qw + (long long)f * nb;
    double* PAb = place == 2 ? st + 2 * nb : g.A + o;
    double* CAb = place == 2 ? PAb + n : g.CA + o;
    double* dSb = place == 2 ? CAb + n : g.dS + o;
    const float* Yr = g.Yr + m0;                                    // Y_b[l, m] = Yr[l * Mtot + m] = Yc[m * L + l]
    const float* Yc = g.Yc + m0 * L;
    const int lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, q16 = lane >> 4;
    const int nbu = (H + 15) >> 4;

    for (long long t = tid; t < nb; t += FITB_THREADS) {
        const long long l = t / H;
        const int h = (int)(t - l * H);
        Bl[t] = g.B[(long long)f * nb + (long long)h * L + l];
    }
    for (int t = tid; t < h2; t += FITB_THREADS) SBm[t] = g.SB[(long long)f * h2 + t];
    if (place == 2)
        for (long long t = tid; t < n; t += FITB_THREADS) CAb[t] = g.CA[o + t];
    if (tid < H) {
        cb_s[tid] = g.CB[(long long)f * H + tid];
        dl_s[tid] = 0.0;
    }
    if (tid < NPRI) pri_s[tid] = LOCAL && tid >= 6 ? g.priors4[(long long)f * NPRI + 2 * (tid - 6)] + 0.5
                                                   : g.priors4[(long long)f * NPRI + tid];
    if (tid == 0) bad_s = 0;
    const double eta = g.eta[f], zeta0 = g.zeta0[f], gam = g.gamma[f], delta0 = g.delta0[f], Lg = (double)L;
    double sig = ROWS ? 0.0 : g.sigma[f], zeta = 0.0, d = g.eps + 1.0;   // ROWS: sig = mean(s)
    double yy = 0.0;
    if constexpr (ROWS) {
        // ||Y_b[l,:]||^2 per row: T lanes per row split the columns, an xor-butterfly folds them (T from L alone, as in fitb_product)
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
        for (long long l = tid; l < L; l += FITB_THREADS) {
            const double s = g.sigma[(long long)f * L + l];
            sv[l] = s;
            ss += s;
        }
        sig = fitb_sum(ss, red) / Lg;                               // (its barriers publish B, SigmaB, CA, s and the row norms)
    } else {
        // ||Y_b||^2
        for (long long t = tid; t < L * Mb; t += FITB_THREADS) {
            const long long l = t / Mb, m = t - l * Mb;
            const double y = (double)Yr[l * g.Mtot + m];
            yy += y * y;
        }
        yy = fitb_sum(yy, red);                                    // (its barriers publish B, SigmaB, CA)
    }
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
        // ---- updateA!, updateCA! -------------------------------------------------------------------------------------------------
        if (tid < H) {
            const int grp = tid < H0 ? 0 : 1;
            al_s[tid] = pri_s[2 * grp] + 0.5;
            b0_s[tid] = pri_s[2 * grp + 1];
            if constexpr (!ROWS) v_s[tid] = sig * BB[tid * H + tid] + Lg * SBm[tid * H + tid];
        }
        if constexpr (ROWS) {
            // Ql = diag(s) B (Ql is free: dB'dB has consumed its B_old - B); v_h = sum_l Ql_lh^2 + L mean(s) SigmaB_hh
            for (long long t = tid; t < nb; t += FITB_THREADS) Ql[t] = sv[t / H] * Bl[t];
            __syncthreads();
            fitb_chunk_reduce(H, L, part, v_s, [&](int h, long long l) { return Ql[l * H + h] * Ql[l * H + h]; });
            if (tid < H) v_s[tid] += Lg * sig * SBm[tid * H + tid];
            if constexpr (FULL)                                     // B' diag(s) B, symmetric bit for bit (Dm is free until SigmaA's sum)
                fitb_chunk_reduce(h2, L, part, Dm, [&](int e, long long l) {
                    const int i = e / H, j = e % H;
                    return Ql[l * H + (i < j ? i : j)] * Bl[l * H + (i < j ? j : i)];
                });
            fitb_product<NP>(Mb, L, Yr, g.Mtot, Yc, L, Ql, H, PAb);
        } else {
            fitb_product<NP>(Mb, L, Yr, g.Mtot, Yc, L, Bl, H, PAb);
        }
        __syncthreads();
        int bad = 0;
        double gs[NGS];                                            // sum log beta, sum CA of each prior group: this thread's shares
#pragma unroll
        for (int k = 0; k < NGS; ++k) gs[k] = 0.0;
        if constexpr (!FULL) {
            for (long long t = tid; t < n; t += FITB_THREADS) {
                const long long m = t / H;
                const int h = (int)(t - m * H);
                const long long vi = !g.compat ? h : (t < H ? t : (t - H) / (Mb - 1));   // repeat(v, inner = M_b - 1) after the first H
                const double prec = v_s[vi] + CAb[t];
                bad |= !isfinite(prec);
                if constexpr (LOCAL) {
                    const double ds = 1.0 / prec, a = (m < M0f && h >= hmask) ? 0.0 : (ROWS ? ds * PAb[t] : sig * ds * PAb[t]);
                    PAb[t] = a;
                    dSb[t] = ds;
                    const int grp = h < H0 ? 0 : (m < M0f ? 1 : 2);
                    const double be = pri_s[2 * grp + 1] + 0.5 * (a * a + ds), ca = (pri_s[2 * grp] + 0.5) / be;
                    CAb[t] = ca;
                    g.beta[o + t] = be;
                    const double lb = log(be);
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        gs[2 * k] += grp == k ? lb : 0.0;
                        gs[2 * k + 1] += grp == k ? ca : 0.0;
                    }
                    continue;
                }
                const double ds = 1.0 / prec, a = sig * ds * PAb[t];
                PAb[t] = a;
                dSb[t] = ds;
                const double be = b0_s[h] + 0.5 * (a * a + ds), ca = al_s[h] / be;
                CAb[t] = ca;
                g.beta[o + t] = be;
                const int grp = h < H0 ? 0 : 2;
                gs[grp] += log(be);
                gs[grp + 1] += ca;
            }
            __syncthreads();
            fitb_chunk_reduce(H, Mb, part, sa_s, [&](int h, long long m) { return dSb[m * H + h]; });
        } else {
            double* W = lds_fb + (size_t)w * NP * LD;
            double* pvec = lds_fb + (size_t)NW * NP * LD + w * NP;
            f64x4 g0[NUP], acc[NUP];
            {   // G = B'B + L SigmaB: its upper blocks in the MFMA's C/D layout (zero beyond H)
                int u = 0;
#pragma unroll
                for (int I = 0; I < NBK; ++I)
#pragma unroll
                    for (int J = I; J < NBK; ++J, ++u)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int i = 16 * I + q16 + 4 * r, j = 16 * J + c16;
                            if constexpr (ROWS) g0[u][r] = (i < H && j < H) ? Dm[i * H + j] + Lg * sig * SBm[i * H + j] : 0.0;
                            else g0[u][r] = (i < H && j < H) ? BB[i * H + j] + Lg * SBm[i * H + j] : 0.0;
                            acc[u][r] = 0.0;
                        }
            }
            for (long long m = w; m < Mb; m += NW) {
                {   // K_m = sigma G + diag(CA[m,:]) into the image (upper blocks; identity beyond H).  The diagonal element of row
                    // 16 I + c sits in lane row c & 3, register c >> 2
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
                            if constexpr (ROWS) x = g0[u];          // (s is inside g0)
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
                // a_m = sigma Sigma_m p_m: lane i takes row i of the symmetric matrix (upper storage)
                const int i = lane < H ? lane : 0;
                double sm = 0.0;
                const int nj = 16 * nbu;
                for (int j = 0; j < nj; ++j) {
                    const int lo = j < i ? j : i, hi = j < i ? i : j;
                    sm += W[lo * LD + hi] * pvec[j];                    // (pvec is zero beyond H; W is the identity padding there)
                }
                const double a = (lane < H && !(LOCAL && m < M0f && lane >= hmask)) ? (ROWS ? -sm : -sig * sm) : 0.0;
                if constexpr (LOCAL) {
                    if (lane < H) {
                        const long long t = m * H + lane;
                        const double ds = -W[lane * LD + lane];
                        PAb[t] = a;
                        dSb[t] = ds;
                        const int grp = lane < H0 ? 0 : (m < M0f ? 1 : 2);
                        const double be = pri_s[2 * grp + 1] + 0.5 * (a * a + ds), ca = (pri_s[2 * grp] + 0.5) / be;
                        CAb[t] = ca;
                        g.beta[o + t] = be;
                        const double lb = log(be);
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            gs[2 * k] += grp == k ? lb : 0.0;
                            gs[2 * k + 1] += grp == k ? ca : 0.0;
                        }
                    }
                } else if (lane < H) {
                    const long long t = m * H + lane;
                    const double ds = -W[lane * LD + lane];
                    PAb[t] = a;
                    dSb[t] = ds;
                    const double be = b0_s[lane] + 0.5 * (a * a + ds), ca = al_s[lane] / be;
                    CAb[t] = ca;
                    g.beta[o + t] = be;
                    const int grp = lane < H0 ? 0 : 2;
                    gs[grp] += log(be);
                    gs[grp + 1] += ca;
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
            // SigmaA = the waves' sums folded through their images (fixed order)
            {
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
                for (int ww = 0; ww < NW; ++ww) s += lds_fb[(size_t)ww * NP * LD + lo * LD + hi];
                Dm[t] = s;                                          // (Dm is free until the end of the sweep)
            }
            __syncthreads();
        }
        if (g.est_priors) {
#pragma unroll
            for (int k = 0; k < NGS; ++k) gs[k] = fitb_sum(gs[k], red);
        }
        // ---- updateB! -----------------------------------------------------------------------------------------------------------
        fitb_chunk_reduce(h2, Mb, part, AA, [&](int e, long long m) { return PAb[m * H + e / H] * PAb[m * H + e % H]; });
        for (int t = tid; t < h2; t += FITB_THREADS) {
            const int i = t / H, j = t % H;
            const double s = FULL ? Dm[t] : (i == j ? sa_s[i] : 0.0);
            AA[t] += s;
            g.SA[(long long)f * h2 + t] = s;
        }
        __syncthreads();
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
        fitb_product<NP>(L, Mb, Yc, L, Yr, g.Mtot, PAb, H, Ql);
        __syncthreads();
        double trG = 0.0;                                           // ROWS: sum G o SigmaB, G = A'A + SigmaA
        if constexpr (ROWS) {
            for (int t = tid; t < h2; t += FITB_THREADS) trG += AA[t] * SBm[t];
            trG = fitb_sum(trG, red);
        }
        // B = sigma Q SigmaB, a row per thread; Q's row then holds B_old - B (ROWS: sigma = s_l, and the row's updateSigma! follows)
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
                // zetaVec_l = zeta0 + ||Y_b[l,:]||^2 / 2 - r_l + (b_l'G b_l + tr) / 2 with the row's new b_l; then the new s_l
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
        // (either sum's barriers publish the new B to the Grams below)
        if constexpr (ROWS) sig = fitb_sum(ssum, red) / Lg;         // mean(s): every thread summed the rows it wrote, in row order
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
        // ---- updateCB!, updateSigma!, est_priors -----------------------------------------------------------------------------------
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
            // group sizes: M H0, M H1 (two groups); M H0, M0 H1, (M - M0) H1 (three: src/vbmf_trial.jl:442-507)
            const double ng[3] = {(double)Mb * (double)H0, (double)(LOCAL ? M0f : Mb) * (double)(H - H0),
                                  (double)(Mb - M0f) * (double)(H - H0)};
            for (int grp = 0; grp < NGS / 2; ++grp) {
                const double nn = ng[grp];
                if constexpr (LOCAL) pri_s[6 + grp] = pri_s[2 * grp] + 0.5;   // the posterior shape this sweep's updateCA! used
                if (!(nn > 0.0)) continue;                          // empty group: nothing to fit
                const double a_post = pri_s[2 * grp] + 0.5;         // what this sweep's updateCA! used
                const double y = log(pri_s[2 * grp + 1]) + digamma_dev(a_post) - gs[2 * grp] / nn;
                double a_new = pri_s[2 * grp];
                if (isfinite(y) && y < 23.025850929890457 && y > -1e10) {
                    a_new = digamma_inv_dev(y);
                    a_new = fmin(fmax(a_new, 1e-10), 1e10);
                }
                pri_s[2 * grp] = a_new;
                pri_s[2 * grp + 1] = nn * a_new / gs[2 * grp + 1];
            }
        }
        // ---- d, the stop test -------------------------------------------------------------------------------------------------------
        if (sB != 1.0)                                              // (uniform; A'A + SigmaA is free until the next sweep)
            fitb_chunk_reduce(h2, L, part, AA, [&](int e, long long l) { return (sB * Bl[l * H + e / H]) * (sB * Bl[l * H + e % H]); });
        double lamD, lamBn;
        fitb_lambda_max(Dm, sB != 1.0 ? AA : BB, H, g.spectral, E, vec_s, lamD, lamBn);
        d = (sqrt(lamD) / sD) / nrmB;
        nrmB = sqrt(lamBn) / sB;
        if (bad) bad_s = 1;                                         // (same value from every writer)
        __syncthreads();                                            // (also publishes pri_s, cb_s)
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
    for (int t = tid; t < h2; t += FITB_THREADS) g.SB[(long long)f * h2 + t] = SBm[t];
    if (tid < H) {
        g.CB[(long long)f * H + tid] = cb_s[tid];
        if (g.est_cb) g.delta[(long long)f * H + tid] = dl_s[tid];
    }
    for (long long t = tid; t < n; t += FITB_THREADS) {
        if (place == 2) {
            g.CA[o + t] = CAb[t];
            g.dS[o + t] = dSb[t];
        }
        if (place == 2) g.A[o + t] = PAb[t];                        // (otherwise PAb is the fit's slice of g.A)
    }
    if (tid < NPRI) g.priors4[(long long)f * NPRI + tid] = pri_s[tid];
    if constexpr (ROWS) {
        if (sv != g.sigma + (long long)f * L)
            for (long long l = tid; l < L; l += FITB_THREADS) g.sigma[(long long)f * L + l] = sv[l];
    }
    if (tid == 0) {
        if constexpr (!ROWS) {
            g.sigma[f] = sig;
            g.zeta[f] = zeta;
        }
        g.iters[f] = it;
        g.dlast[f] = d;
        g.status[f] = status;
    }
}

}  // namespace vbmf
