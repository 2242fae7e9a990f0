// sparse_batch_kernels.hpp -- vbls! on the ARD-sparse models over many bags with one fixed basis
// (vbmf_sparse_run_fixed_basis_batched; examples/mil_util.jl:187-197 in one call).
//
// The context's Y holds the bags side by side: bag b = columns col_off[b] .. col_off[b+1]-1.  One pass 1 with the frozen B forms
// P = Y'B for all of them, bag_gram_kernel (batch_kernels.hpp, S not formed) each bag's ||Y_b||^2, and then ONE launch of
// sparse_batch_kernel runs all niter iterations of every bag, one workgroup per bag (updateA! never reads the previous A).  Per
// iteration and bag, with G = B'B + L SigmaB and sigma the bag's noise precision:
//   updateA!, diagonal (src/vbmf_sparse.jl:204-240)  v = sigma diag(B'B) + L diag(SigmaB) (QS2), spread over vec(A') (QS1 under
//             VBMF_COMPAT_SPARSE_REPEAT with the bag's own M), dS = 1 / (v + CA), a = sigma dS p, SigmaA = diag(sum_m dS[m,:])
//   updateA!, full_cov (:178-202)  per column: Sigma_m = inv(sigma G + diag(CA[m,:])), a_m = sigma Sigma_m p_m, dS = diag(Sigma_m),
//             SigmaA = sum_m Sigma_m -- each wave takes whole columns and inverts in its own LDS image (blk_sweep, no barrier)
//   updateCA! (:284-288; src/vbmf_dual.jl:322-351; src/vbmf_trial.jl:357-400)  beta = beta0_h + (a^2 + dS) / 2, CA = alpha_h / beta
//             with per-bag (alpha_h, beta0_h): the three families differ only there
//   updateSigma! (:317-321)  zeta = zeta0 + ||Y_b||^2 / 2 - sum P o A + tr((A'A + SigmaA) G) / 2, sigma = eta / zeta
// The bag's state (P, CA, A, dS) is fp64: in LDS when it fits (lds_state), else in the bag's own slices of the device buffers.
// Bags do not align with the 32-column tiles of P: every access goes through the column index.
// The loop itself is sbatch_iterate, a __device__ function that vbls_jobs_kernel (vbls_jobs_kernels.hpp: many bases, fp64 P) calls too.
#pragma once
#include "common.hpp"
#include "ctrl_kernels.hpp"
#include "blk_inverse.hpp"

namespace vbmf {

constexpr int SBATCH_THREADS = 256, SBATCH_NW = SBATCH_THREADS / 64;
// dynamic LDS per workgroup: 56 KiB (64 with the static arrays), except full_cov at 32 < H <= 64 (four 64 x 66 fp64 images, 136 KiB, before any state;
// the attribute is set in vbmf_create)
constexpr size_t SBATCH_LDS_SMALL = 56 * 1024, SBATCH_LDS_BIG = 150 * 1024;

// doubles of dynamic LDS in front of a bag's state: G (diagonal form), or the waves' images, p_m and a_m vectors (full_cov)
__host__ __device__ constexpr int sbatch_fixed_doubles(bool full, int NBK, int H) {
    return full ? SBATCH_NW * (16 * NBK) * (16 * NBK + 2) + 2 * SBATCH_NW * 16 * NBK : H * H;
}

// G = B'B + L SigmaB (H x H, ld H) and the two terms of v apart: gd = diag(B'B), sd = L diag(SigmaB)
__global__ void sbatch_g_kernel(const double* __restrict__ st, StateLayout lay, int H, double Lg, double* __restrict__ G,
                                double* __restrict__ gd, double* __restrict__ sd) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= H * H) return;
    const int i = t / H, j = t % H;
    const long long e = (long long)i * lay.Hp + j;
    G[t] = st[lay.GB() + e] + Lg * st[lay.SB() + e];
    if (i == j) {
        gd[i] = st[lay.GB() + e];
        sd[i] = Lg * st[lay.SB() + e];
    }
}

struct SbatchArgs {
    const float* P; long long ldP;                 // Y'B of all bags, [h][x] at leading dimension ldP (fp32)
    const long long* col_off;
    int H, niter, compat, lds_state;               // compat: the QS1 layout; lds_state: LDS doubles for a bag's state
    double Lg;
    const double* G; const double* gd; const double* sd;
    const double* alpha; const double* beta0;      // nbags x H
    const double* eta; const double* zeta0; const double* yy;   // nbags
    double* sigma; double* zeta;                   // nbags: sigma start values in, both final values out
    double* ca; double* A; double* dS; double* beta; double* Pd;   // M x H in vec(A') order; ca: start values in, final out
    double* SA;                                    // nbags x H x H
    int* err;
};

// What one workgroup's vbls! loop works on: a bag's state (P, CA, A, dS; LDS or global, M_b x H in vec(A') order), the basis' G, gd, sd
// (global), updateCA!'s (alpha_h, beta0_h) in al_s / b0_s, and where the last iteration's beta and SigmaA go (nullptr: not wanted).
// lds_sb: sbatch_fixed_doubles of dynamic LDS; red: 16 doubles, v_s, al_s, b0_s, sa_s: 64 each (static LDS of the calling kernel).
struct SbatchBody {
    int H, niter, compat;
    long long Mb;
    const double* G; const double* gd; const double* sd;
    double* Pb; double* CAb; double* Ab; double* dSb;
    double* beta; double* SA;
    double eta, zeta0, yy;
    double* lds_sb; double* red; double* v_s; double* al_s; double* b0_s; double* sa_s;
};

// The niter iterations of one bag, by the whole workgroup of SBATCH_THREADS: sparse_batch_kernel's loop, shared with vbls_jobs_kernel
// (vbls_jobs_kernels.hpp).  The caller has filled Pb, CAb, al_s, b0_s (no barrier needed after that: the one below covers it).
// sig: the start value in, the final one out; bad: raised on a non-finite precision or a bad pivot.
template <int NBK, bool FULL>
__device__ __forceinline__ void sbatch_iterate(const SbatchBody& q, double& sig, double& zeta, int& bad) {
    constexpr int NP = 16 * NBK, LD = NP + 2, NUP = NBK * (NBK + 1) / 2, NW = SBATCH_NW;
    const int H = q.H, tid = threadIdx.x;
    const long long Mb = q.Mb, n = Mb * H;
    double* const lds_sb = q.lds_sb;
    double* const red = q.red;
    double* const v_s = q.v_s; double* const al_s = q.al_s; double* const b0_s = q.b0_s; double* const sa_s = q.sa_s;
    double* const Pb = q.Pb; double* const CAb = q.CAb; double* const Ab = q.Ab; double* const dSb = q.dSb;
    const double eta = q.eta, zeta0 = q.zeta0, yy = q.yy;
    if constexpr (!FULL)
        for (int t = tid; t < H * H; t += SBATCH_THREADS) lds_sb[t] = q.G[t];
    // full_cov: G's upper blocks in the MFMA's C/D layout (zero beyond H), the running sum of this wave's Sigma_m
    const int lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, q16 = lane >> 4;
    const int nbu = (H + 15) >> 4;
    f64x4 g0[FULL ? NUP : 1], acc[FULL ? NUP : 1];
    if constexpr (FULL) {
        int u = 0;
#pragma unroll
        for (int I = 0; I < NBK; ++I)
#pragma unroll
            for (int J = I; J < NBK; ++J, ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = 16 * I + q16 + 4 * r, j = 16 * J + c16;
                    g0[u][r] = (i < H && j < H) ? q.G[i * H + j] : 0.0;
                }
    }
    __syncthreads();
    for (int it = 0; it < q.niter; ++it) {
        const bool last = it + 1 == q.niter;
        double pa = 0.0, tq = 0.0, tsa = 0.0;          // sum P o A, sum_m a_m' G a_m, tr(SigmaA G): this thread's shares
        if constexpr (!FULL) {
            const double* Gs = lds_sb;
            if (tid < H) v_s[tid] = sig * q.gd[tid] + q.sd[tid];
            __syncthreads();
            for (long long t = tid; t < n; t += SBATCH_THREADS) {
                const long long m = t / H;
                const int h = (int)(t - m * H);
                const long long vi = !q.compat ? h : (t < H ? t : (t - H) / (Mb - 1));   // repeat(v, inner = M_b - 1) after the first H
                const double prec = v_s[vi] + CAb[t];
                bad |= !isfinite(prec);
                const double d = 1.0 / prec, p = Pb[t], a = sig * d * p;
                Ab[t] = a;
                dSb[t] = d;
                const double be = b0_s[h] + 0.5 * (a * a + d);
                CAb[t] = al_s[h] / be;
                if (last && q.beta) q.beta[t] = be;
                pa += p * a;
            }
            __syncthreads();
            for (long long t = tid; t < n; t += SBATCH_THREADS) {
                const long long m = t / H;
                const int i = (int)(t - m * H);
                const double* am = Ab + m * H;
                double s = 0.0;
                for (int j = 0; j < H; ++j) s += Gs[i * H + j] * am[j];
                tq += am[i] * s;
            }
            if (tid < H) {
                double s = 0.0;
                for (long long m = 0; m < Mb; ++m) s += dSb[m * H + tid];
                sa_s[tid] = s;
                tsa = s * Gs[tid * H + tid];
            }
        } else {
            double* W = lds_sb + (size_t)w * NP * LD;
            double* pvec = lds_sb + (size_t)NW * NP * LD + w * NP;
            double* avec = pvec + NW * NP;
#pragma unroll
            for (int u = 0; u < NUP; ++u) acc[u] = f64x4{0.0, 0.0, 0.0, 0.0};
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
                            f64x4 x = sig * g0[u];
                            if (I == J) {
#pragma unroll
                                for (int r = 0; r < 4; ++r) x[r] += (q16 == (c16 & 3) && r == (c16 >> 2)) ? cad[I] : 0.0;
                            }
                            if (I < nbu && J < nbu) blk_st_rows(W, LD, I, J, lane, x);
                        }
                }
                if (lane < NP) pvec[lane] = lane < H ? Pb[m * H + lane] : 0.0;
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
                const double a = lane < H ? -sig * sm : 0.0;
                if (lane < NP) avec[lane] = a;
                if (lane < H) {
                    const long long t = m * H + lane;
                    const double d = -W[lane * LD + lane];
                    Ab[t] = a;
                    dSb[t] = d;
                    const double be = b0_s[lane] + 0.5 * (a * a + d);
                    CAb[t] = al_s[lane] / be;
                    if (last && q.beta) q.beta[t] = be;
                    pa += pvec[lane] * a;
                    double s = 0.0;
                    for (int j = 0; j < H; ++j) s += q.G[lane * H + j] * avec[j];
                    tq += a * s;
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
                    for (int J = I; J < NBK; ++J, ++u) blk_st_rows(W, LD, I, J, lane, acc[u]);
            }
            __syncthreads();
            for (int t = tid; t < H * H; t += SBATCH_THREADS) {
                const int i = t / H, j = t % H;
                const int lo = i <= j ? i : j, hi = i <= j ? j : i;
                double s = 0.0;
#pragma unroll
                for (int ww = 0; ww < NW; ++ww) s += lds_sb[(size_t)ww * NP * LD + lo * LD + hi];
                tsa += s * q.G[t];
                if (last && q.SA) q.SA[t] = s;
            }
        }
        pa = block_sum(pa, red);                        // (its barriers also end every read of this iteration's LDS)
        tq = block_sum(tq, red);
        tsa = block_sum(tsa, red);
        zeta = zeta0 + 0.5 * yy - pa + 0.5 * (tq + tsa);
        sig = eta / zeta;
        if (!FULL && last && q.SA)
            for (int t = tid; t < H * H; t += SBATCH_THREADS) {
                const int i = t / H, j = t % H;
                q.SA[t] = i == j ? sa_s[i] : 0.0;
            }
    }
}

template <int NBK, bool FULL>
__global__ __launch_bounds__(SBATCH_THREADS) void sparse_batch_kernel(SbatchArgs g) {
    extern __shared__ __attribute__((aligned(16))) double lds_sb[];
    __shared__ double red[16];
    __shared__ double v_s[64], al_s[64], b0_s[64], sa_s[64];
    const int b = blockIdx.x, H = g.H, tid = threadIdx.x;
    const long long m0 = g.col_off[b], Mb = g.col_off[b + 1] - m0;
    const long long n = Mb * H, o = m0 * H;
    const int nfix = sbatch_fixed_doubles(FULL, NBK, H);
    const bool in_lds = 4 * n <= (long long)g.lds_state;
    double* Pb = in_lds ? lds_sb + nfix : g.Pd + o;
    double* CAb = in_lds ? Pb + n : g.ca + o;
    double* Ab = in_lds ? CAb + n : g.A + o;
    double* dSb = in_lds ? Ab + n : g.dS + o;
    for (long long t = tid; t < n; t += SBATCH_THREADS) {
        const long long m = t / H;
        const int h = (int)(t - m * H);
        Pb[t] = (double)g.P[(long long)h * g.ldP + m0 + m];
        if (in_lds) CAb[t] = g.ca[o + t];
    }
    if (tid < H) {
        al_s[tid] = g.alpha[(long long)b * H + tid];
        b0_s[tid] = g.beta0[(long long)b * H + tid];
    }
    double sig = g.sigma[b], zeta = 0.0;
    int bad = 0;
    const SbatchBody q{H, g.niter, g.compat, Mb, g.G, g.gd, g.sd, Pb, CAb, Ab, dSb, g.beta ? g.beta + o : nullptr,
                       g.SA ? g.SA + (long long)b * H * H : nullptr, g.eta[b], g.zeta0[b], g.yy[b], lds_sb, red, v_s, al_s, b0_s, sa_s};
    sbatch_iterate<NBK, FULL>(q, sig, zeta, bad);
    if (in_lds)
        for (long long t = tid; t < n; t += SBATCH_THREADS) {
            g.ca[o + t] = CAb[t];
            g.A[o + t] = Ab[t];
            g.dS[o + t] = dSb[t];
        }
    if (tid == 0) {
        g.sigma[b] = sig;
        g.zeta[b] = zeta;
    }
    if (bad) atomicExch(g.err, 1);
}

}  // namespace vbmf
