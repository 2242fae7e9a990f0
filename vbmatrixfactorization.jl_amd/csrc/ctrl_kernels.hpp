// ctrl_kernels.hpp -- the H x H "control" algebra of a sweep, fp64, one workgroup, LDS-resident.
//
//   ctrl_cov_kernel   SigmaA = sigma2*inv(B'B + L*SigmaB + sigma2*inv(CA))   src/vbmf.jl:96-97
//                     SigmaB = sigma2*inv(A'A + M*SigmaA + sigma2*inv(CB))   src/vbmf.jl:110-111
//                     (register-tiled Gauss-Jordan, one barrier per pivot; log-determinant from the pivots)
//   eig_kernel        lambda_max of the delta-Gram and of the B-Gram (Lanczos on the register-resident matrix):
//                     Julia 0.5 `norm(::Matrix)` is the spectral norm (src/util.jl:27-29)
//   ctrl_end_kernel   updateCA!/updateCB! (src/vbmf.jl:129-146), updateSigma2! (src/vbmf.jl:153-157),
//                     d (src/vbmf.jl:211), loop test (src/vbmf.jl:193), build-defined ELBO, trace record.
//
// fp64 because ARD drives entries of C toward 0 and precisions to 1e10; on a
// 64..128-wide matrix the cost is negligible next to the streaming passes.
#pragma once
#include "common.hpp"
#include "blk_inverse.hpp"

namespace vbmf {

// ---- layout of the device state block (doubles) ------------------------------------------------
struct StateLayout {
    int Hp;
    __host__ __device__ long long n2() const { return (long long)Hp * Hp; }
    __host__ __device__ long long GA() const { return 0; }
    __host__ __device__ long long GB() const { return n2(); }
    __host__ __device__ long long GD() const { return 2 * n2(); }     // must follow GB (one all-reduce)
    // GX: 8 doubles right behind GD, so that [GB | GD | GX] is ONE contiguous all-reduce target; GX[0] = tr(B'YA) = the
    // direct sum  sum_{l,h} (Y A)[l,h] * BHat[l,h]  over this rank's rows, formed where BHat is produced
    __host__ __device__ long long GX() const { return 3 * n2(); }
    __host__ __device__ long long SA() const { return 3 * n2() + 8; }
    __host__ __device__ long long SB() const { return 4 * n2() + 8; }
    __host__ __device__ long long KB() const { return 5 * n2() + 8; }     // matrix inverted for SigmaB
    __host__ __device__ long long W0() const { return 6 * n2() + 8; }     // scratch (H > 128)
    __host__ __device__ long long W1() const { return 7 * n2() + 8; }
    __host__ __device__ long long W2() const { return 8 * n2() + 8; }
    __host__ __device__ long long ca() const { return 9 * n2() + 8; }
    __host__ __device__ long long cb() const { return 9 * n2() + 8 + Hp; }
    __host__ __device__ long long scal() const { return 9 * n2() + 8 + 2 * Hp; }
    __host__ __device__ long long total() const { return scal() + 32; }
};
enum : int { S_SIGMA2 = 0, S_TRYY, S_LOGDET_SA, S_LOGDET_SB, S_LAMB_PREV, S_LAMB_NEW, S_LAMD, S_D, S_ELBO,
             S_TRDOT, S_RESID, S_TRYBA,
             S_LOGDET_SA_SHADOW = 20,        // 12..18 and 21..29 (S_GPRI, S_GPOST): sparse_kernels.hpp
             S_LAMB_SHADOW = 30 };           // lambda_max(B_old'B_old) computed ahead by the Gram form's first chain launch (ctrl_chain)
enum : int { I_STOP = 0, I_ITERS = 1, I_ERR = 2, I_NITER = 3, I_SREADY = 4, I_DBG_SB_PPM = 5 };   // (5: test hook, vbmf_debug_set)

// Threads of the workgroup that run the control algebra: the whole block -- except in the 512-thread launch of the H >= 128
// streaming kernel (stream_gemm.hpp, stream_lds8_kernel), whose control workgroups run on their first 256 threads (waves 4-7
// leave at once; a barrier counts live waves only).  No control kernel of its own is ever launched with 512 threads.
__device__ __forceinline__ int ctrl_nthreads() { return blockDim.x == 512u ? 256 : (int)blockDim.x; }

__device__ __forceinline__ double block_sum(double v, double* red) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    const int nw = (ctrl_nthreads() + 63) >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int i = 0; i < nw; ++i) s += red[i];
    return s;
}
__device__ __forceinline__ double block_max(double v, double* red) {
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off));
    const int nw = (ctrl_nthreads() + 63) >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
    for (int i = 1; i < nw; ++i) s = fmax(s, red[i]);
    return s;
}

// In-place inverse of the SPD n x n matrix W (leading dim n) by Gauss-Jordan without pivoting.
// aux: 2n doubles.  Returns log det(W) (all threads).  Sets *err on a non-positive / non-finite pivot.
__device__ inline double gj_inverse_spd(double* W, int n, double* aux, int* err) {
    double* colk = aux;
    double* rowk = aux + n;
    double logdet = 0.0;
    for (int k = 0; k < n; ++k) {
        const double piv = W[(long long)k * n + k];
        if (!(piv > 0.0) || !isfinite(piv)) { if (threadIdx.x == 0) atomicExch(err, 1); }
        const double pinv = 1.0 / piv;
        logdet += log(piv);
        for (int i = threadIdx.x; i < n; i += ctrl_nthreads()) {
            colk[i] = W[(long long)i * n + k];
            rowk[i] = (i == k ? 1.0 : W[(long long)k * n + i]) * pinv;
        }
        __syncthreads();
        for (int t = threadIdx.x; t < n * n; t += ctrl_nthreads()) {
            const int i = t / n, j = t - i * n;
            double v;
            if (i == k) v = rowk[j];
            else v = (j == k ? 0.0 : W[t]) - colk[i] * rowk[j];
            W[t] = v;
        }
        __syncthreads();
    }
    return logdet;
}

// ---- register-tiled Gauss-Jordan ---------------------------------------------------------------
// T x T threads; thread (ty,tx) keeps the R x R entries {(ty + T*a, tx + T*b)} of the matrix in
// registers (cyclic distribution: every thread stays busy through all pivots).  Per pivot the owners
// of pivot row/column publish them through a double-buffered LDS strip, ONE barrier, then every
// thread updates its registers.  The matrix is padded with identity up to T*R.
// 1/x to fp64 accuracy without the IEEE division sequence (v_rcp_f64 + two Newton steps): the pivots of an SPD sweep are
// positive, finite and far from the denormal range
__device__ __forceinline__ double fast_rcp(double x) {
    double r = __builtin_amdgcn_rcp(x);
    r = fma(fma(-x, r, 1.0), r, r);
    r = fma(fma(-x, r, 1.0), r, r);
    return r;
}

// In-place Gauss-Jordan inverse of the SPD matrix held as R x R register tiles (thread (ty, tx) owns rows ty + T*a,
// columns tx + T*b); one barrier per pivot, pivot row / column handed over through double-buffered LDS strips.
// The reciprocal of pivot k+1 is computed during step k's update (every thread on its own diagonal-tile element, so
// there is no branch and the division chain overlaps the update's FMAs) and travels in the column strip's slot k+1 --
// col[k] would otherwise duplicate row[k].  (It used to be divided out after the barrier: ~25 % of a step.)
template <int R, int T>
__device__ __forceinline__ void gj_tiled(double (&w)[R][R], int n, double* strip /* 2*2*T*R */, double* pivs) {
    const int tx = threadIdx.x % T, ty = threadIdx.x / T;
    constexpr int NP = T * R;
    double pinv_next = fast_rcp(w[0][0]);                       // the owner of (0, 0) holds the first pivot here
#pragma unroll
    for (int a0 = 0; a0 < R; ++a0) {
        for (int t = 0; t < T; ++t) {
            const int k = a0 * T + t;
            if (k >= n) break;                                  // uniform
            double* row = strip + (k & 1) * (2 * NP);
            double* col = row + NP;
            if (ty == t) {
#pragma unroll
                for (int b = 0; b < R; ++b) row[tx + T * b] = w[a0][b];
            }
            if (tx == t) {
#pragma unroll
                for (int a = 0; a < R; ++a) col[ty + T * a] = (a == a0 && ty == t) ? pinv_next : w[a][a0];
            }
            __syncthreads();
            const double piv = row[k];
            const double pinv = col[k];
            if (threadIdx.x == 0) pivs[k] = piv;
            double ci[R], rj[R];
#pragma unroll
            for (int a = 0; a < R; ++a) ci[a] = col[ty + T * a];       // ci of row k itself is the reciprocal: unused there
#pragma unroll
            for (int b = 0; b < R; ++b) rj[b] = row[tx + T * b] * pinv;
#pragma unroll
            for (int a = 0; a < R; ++a) {
                const bool is_i = (a == a0) && (ty == t);
#pragma unroll
                for (int b = 0; b < R; ++b) {
                    const bool is_j = (b == a0) && (tx == t);
                    const double upd = w[a][b] - ci[a] * rj[b];
                    const double on_row = is_j ? pinv : rj[b];
                    const double on_col = -ci[a] * pinv;
                    w[a][b] = is_i ? on_row : (is_j ? on_col : upd);
                }
            }
            // reciprocal of the next pivot, element (k+1, k+1): tile (a0, a0) for t + 1 < T, else tile (a0+1, a0+1)
            double cand = w[a0][a0];
            if (a0 + 1 < R) cand = (t + 1 < T) ? cand : w[a0 + 1][a0 + 1];
            pinv_next = fast_rcp(cand);
        }
    }
}

// The same sweep on NB independent matrices at once (same n): one barrier per pivot serves all of them and their
// dependent LDS round trips overlap.
// strip: NB * 4*T*R doubles, pivs: NB * T*R doubles (matrix q's pivots at pivs + q*T*R).
template <int R, int T, int NB>
__device__ __forceinline__ void gj_tiled_n(double (&w)[NB][R][R], int n, double* strip, double* pivs) {
    const int tx = threadIdx.x % T, ty = threadIdx.x / T;
    constexpr int NP = T * R;
    double pinv_next[NB];
#pragma unroll
    for (int q = 0; q < NB; ++q) pinv_next[q] = fast_rcp(w[q][0][0]);
#pragma unroll
    for (int a0 = 0; a0 < R; ++a0) {
        for (int t = 0; t < T; ++t) {
            const int k = a0 * T + t;
            if (k >= n) break;                                  // uniform
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                double* row = strip + q * (4 * NP) + (k & 1) * (2 * NP);
                double* col = row + NP;
                if (ty == t) {
#pragma unroll
                    for (int b = 0; b < R; ++b) row[tx + T * b] = w[q][a0][b];
                }
                if (tx == t) {
#pragma unroll
                    for (int a = 0; a < R; ++a) col[ty + T * a] = (a == a0 && ty == t) ? pinv_next[q] : w[q][a][a0];
                }
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                const double* row = strip + q * (4 * NP) + (k & 1) * (2 * NP);
                const double* col = row + NP;
                const double piv = row[k];
                const double pinv = col[k];
                if (threadIdx.x == 0) pivs[q * NP + k] = piv;
                double ci[R], rj[R];
#pragma unroll
                for (int a = 0; a < R; ++a) ci[a] = col[ty + T * a];
#pragma unroll
                for (int b = 0; b < R; ++b) rj[b] = row[tx + T * b] * pinv;
#pragma unroll
                for (int a = 0; a < R; ++a) {
                    const bool is_i = (a == a0) && (ty == t);
#pragma unroll
                    for (int b = 0; b < R; ++b) {
                        const bool is_j = (b == a0) && (tx == t);
                        const double upd = w[q][a][b] - ci[a] * rj[b];
                        const double on_row = is_j ? pinv : rj[b];
                        const double on_col = -ci[a] * pinv;
                        w[q][a][b] = is_i ? on_row : (is_j ? on_col : upd);
                    }
                }
                double cand = w[q][a0][a0];
                if (a0 + 1 < R) cand = (t + 1 < T) ? cand : w[q][a0 + 1][a0 + 1];
                pinv_next[q] = fast_rcp(cand);
            }
        }
    }
}

// ---- 129 <= H <= 256: the blocked sweep with the matrix in registers (inv256_blk, blk_inverse.hpp) ----------------------------------
// A 256 x 256 fp64 matrix is 512 KB -- the whole register file of a CU -- so the LDS-image sweep of the smaller ranks cannot hold it.  Rounds
// 1-2 split K = [A B; B' D] and took the Schur complement (two register-tiled 128 x 128 Gauss-Jordans with a barrier per pivot + four VALU
// GEMMs through global scratch: 0.38 ms alone, 0.46-0.85 beside a pass); late in round 3 the 136 upper 16 x 16 blocks live in the registers
// of the 16 waves and the sweep's row panel travels through LDS: 0.14 ms alone, 0.22-0.28 beside a pass, 3e-15 from a long-double reference.

// relaxed agent-scope read of the loop's stop flag (bypasses this CU's L1: the flag may have been
// raised a moment ago by ctrl_end in this very workgroup or by another one)
__device__ __forceinline__ int load_stop(const int* ints) {
    return __hip_atomic_load(ints + I_STOP, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The run loops' view of the loop counters: host-mapped words (vbmf_ctx::loopw) that the host reads directly, so no copy and no event
// enters the compute stream.  Called by the one thread that has just stored the counters to `ints`; stop goes out before iters (the
// host reads them in the other order), as relaxed system-scope stores -- ordinary vector stores to fine-grained host memory, no fence.
// The host may see a value late, never early.  hw == nullptr: no run loop is looking (stand-alone steps).
__device__ __forceinline__ void publish_loop_words(int* __restrict__ hw, int* __restrict__ ints, int stop, int iters) {
    if (hw == nullptr) return;
    const int err = __hip_atomic_load(ints + I_ERR, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (err) __hip_atomic_store(hw + I_ERR, err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (stop) __hip_atomic_store(hw + I_STOP, stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(hw + I_ITERS, iters, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Row-sharded runs: the ranks' error flags travel as one more number of the packed Gram message (post_kernels.hpp,
// publish_err_flag) and arrive summed at st[GX + 1]; every rank's loop test reads the same sum, so a hand-off timeout or a bad
// pivot on ONE rank stops EVERY rank at the same sweep (without it the other ranks ran on into the all-reduce with that rank's
// garbage partials).  Returns 0, or the error code this rank records if it has none of its own: 2 (hand-off) / 1 (numeric).
__device__ __forceinline__ int remote_error_code(const double* __restrict__ st, StateLayout lay) {
    const double f = st[lay.GX() + 1];
    return f >= 1000.0 ? 2 : (f > 0.0 ? 1 : 0);
}
__device__ __forceinline__ bool stop_on_remote_error(const double* __restrict__ st, StateLayout lay, int* __restrict__ ints) {
    const int rc = remote_error_code(st, lay);
    if (rc == 0) return false;
    if (atomicCAS(ints + I_ERR, 0, rc) == 0) atomicOr(ints + I_ERR, 0x200);   // 0x200: no error of this rank's own -- another rank's
    return true;
}

// Inverse of an SPD matrix of order H <= 16 NB in LDS by the FOUR waves of a 256-thread control workgroup (blk_inverse.hpp:
// blocked symmetric sweep, the 16 x 16 diagonal blocks inside a wavefront, rank-16 updates on the fp64 MFMA, one or two barriers
// per BLOCK step where round 2's register-tiled Gauss-Jordan had a barrier and two LDS round trips per pivot).
//   elem(i, j): the matrix (i, j < H);  W: 16 NB x (16 NB + 2) doubles of LDS;  on return W's upper triangle holds -inverse
//   (read it through spd_inv_at; the lower 16 x 16 blocks are the sweep's scratch), *logdet = log det of the matrix -- valid on
//   thread 0, which files it --, *bad != 0 if a pivot was not positive / finite -- on the threads of wave 0 at least.
// Every thread of the control workgroup (ctrl_nthreads() = 256 of them) must call it.
// the sweep alone, on an image some other code of the workgroup has filled (identity padding included); opens with the barrier that
// publishes the image
template <int NB>
__device__ __forceinline__ void spd_sweep_lds4(double* W, int H, double* logdet, int* bad) {
    constexpr int LD = 16 * NB + 2;
    __syncthreads();
    PivAcc pv;
    blk_sweep<NB, 4>(W, LD, (H + 15) >> 4, __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), threadIdx.x & 63, pv);
    *logdet = pv.logdet();
    *bad = pv.bad;
}
template <int NB, class ElemF>
__device__ __forceinline__ void spd_inverse_lds4(double* W, int H, ElemF elem, double* logdet, int* bad) {
    constexpr int NP = 16 * NB, LD = NP + 2;
    for (int t = threadIdx.x; t < NP * NP; t += 256) {
        const int i = t / NP, j = t % NP;
        W[i * LD + j] = (i < H && j < H) ? elem(i, j) : (i == j ? 1.0 : 0.0);      // identity padding
    }
    spd_sweep_lds4<NB>(W, H, logdet, bad);
}
template <int NB>
__device__ __forceinline__ double spd_inv_at(const double* W, int i, int j) {          // element (i, j) of the inverse
    constexpr int LD = 16 * NB + 2;
    return -(i <= j ? W[i * LD + j] : W[j * LD + i]);
}
constexpr size_t spd_inverse_lds_bytes(int NB) { return (size_t)(16 * NB) * (16 * NB + 2) * sizeof(double); }

// What follows the sweep of an H <= 128 covariance update: Sigma = sigma2 inv(K) from the swept image W to the state (which = 0:
// SigmaA, or its shadow; 1: SigmaB), inv(K) as the post kernel's fp32 table, the error flag and the log-determinant.
template <int NBc>
__device__ __forceinline__ void cov_store_lds4(double* __restrict__ st, StateLayout lay, int H, int which, double sigma2,
                                               float* __restrict__ S32, int* __restrict__ ints, const double* W, double ldK,
                                               int badK, bool shadow) {
    const int Hp = lay.Hp;
    double* Sself = st + (which == 0 ? (shadow ? lay.W0() : lay.SA()) : lay.SB());
    const double dbg = which == 1 ? 1.0 + 1e-6 * (double)ints[I_DBG_SB_PPM] : 1.0;      // test hook (normally exactly 1)
    for (int t = threadIdx.x; t < Hp * Hp; t += 256) {
        const int i = t / Hp, j = t % Hp;
        const double v = (i < H && j < H) ? spd_inv_at<NBc>(W, i, j) : 0.0;
        Sself[(long long)i * Hp + j] = sigma2 * v;
        S32[(long long)i * Hp + j] = (float)(v * dbg);          // Sigma/sigma2: what the post kernel multiplies by
    }
    if (badK) atomicExch(ints + I_ERR, 1);
    if (threadIdx.x == 0)
        st[lay.scal() + (which == 0 ? (shadow ? S_LOGDET_SA_SHADOW : S_LOGDET_SA) : S_LOGDET_SB)] = (double)H * log(sigma2) - ldK;
}

// which = 0: SigmaA from (GB, SigmaB, ca), N = L_global.  which = 1: SigmaB from (GA, SigmaA, cb), N = M.
// Needs T*T threads and (4*T*R + T*R) doubles of LDS at `lds`; every thread of the block must call it.
// shadow (which = 0, H <= 128 only): SigmaA and its log-determinant go to the W0 scratch / the shadow scalar instead
// of the state; commit_cov_a_kernel copies them over once it is known that the loop continues (ctrl_chain).
template <int R, int T>
__device__ __forceinline__ void ctrl_cov_dev(double* __restrict__ st, StateLayout lay, int H, int which, double N,
                                             float* __restrict__ S32, int* __restrict__ ints, double* lds,
                                             bool shadow = false) {
    __shared__ double red[16];
    __shared__ int stop_s;
    // Workgroup-uniform stop test: inside ctrl_chain the other part of the launch may raise the flag while this one starts, and
    // waves that disagreed would leave the inverse's barriers unmatched.  (A bad pivot of a speculative SigmaA -- shadow -- still
    // raises I_ERR even if the loop then stops before that SigmaA would be used; the streaming chain has always done the same.)
    if (threadIdx.x == 0) stop_s = load_stop(ints);
    __syncthreads();
    if (stop_s) return;
    constexpr int NP = T * R;
    const int Hp = lay.Hp;
    const int tx = threadIdx.x % T, ty = threadIdx.x / T;
    const double* G = st + (which == 0 ? lay.GB() : lay.GA());
    const double* Sother = st + (which == 0 ? lay.SB() : lay.SA());
    double* Sself = st + (which == 0 ? (shadow ? lay.W0() : lay.SA()) : lay.SB());
    const double* cdiag = st + (which == 0 ? lay.ca() : lay.cb());
    double* scal = st + lay.scal();
    const double sigma2 = scal[S_SIGMA2];
    double* pivs;
    if constexpr (R == 8 && T == 32) {
        // 129 <= H <= 256 (Hp = 256): the blocked sweep with the matrix in registers (inv256_blk, blk_inverse.hpp)
        double* Kg = st + lay.W0();
        double* Ki = st + lay.W1();
        for (int t = threadIdx.x; t < 256 * 256; t += 1024) {
            const int i = t >> 8, j = t & 255;
            double v = (i == j) ? 1.0 : 0.0;                    // identity padding
            if (i < H && j < H) {
                v = G[(long long)i * Hp + j] + N * Sother[(long long)i * Hp + j];
                if (i == j) v += sigma2 / cdiag[i];
            }
            Kg[t] = v;
        }
        __syncthreads();
        pivs = lds + INV256_LDS_DOUBLES;
        inv256_blk(Kg, Ki, lds, pivs, (H + 15) >> 4);
        for (int t = threadIdx.x; t < 256 * 256; t += 1024) {
            const int i = t >> 8, j = t & 255;
            const double v = (i < H && j < H) ? Ki[t] : 0.0;
            Sself[(long long)i * Hp + j] = sigma2 * v;
            S32[(long long)i * Hp + j] = (float)v;
        }
    } else {
        // H <= 128: blocked sweep in LDS (spd_inverse_lds4)
        static_assert(T == 16, "four waves");
        constexpr int NBc = NP / 16;
        double ldK; int badK;
        spd_inverse_lds4<NBc>(lds, H, [&](int i, int j) {
            double v = G[(long long)i * Hp + j] + N * Sother[(long long)i * Hp + j];
            if (i == j) v += sigma2 / cdiag[i];
            return v;
        }, &ldK, &badK);
        cov_store_lds4<NBc>(st, lay, H, which, sigma2, S32, ints, lds, ldK, badK, shadow);
        return;
    }
    __syncthreads();
    double ld = 0.0;
    int bad = 0;
    for (int k = threadIdx.x; k < H; k += ctrl_nthreads()) {
        const double pv = pivs[k];
        if (!(pv > 0.0) || !isfinite(pv)) bad = 1;
        ld += log(pv);
    }
    ld = block_sum(ld, red);
    if (bad) atomicExch(ints + I_ERR, 1);
    if (threadIdx.x == 0)
        scal[which == 0 ? (shadow ? S_LOGDET_SA_SHADOW : S_LOGDET_SA) : S_LOGDET_SB] = (double)H * log(sigma2) - ld;
}

// the loop continues: make the speculative SigmaA of ctrl_chain the state's
__global__ __launch_bounds__(256) void commit_cov_a_kernel(double* __restrict__ st, StateLayout lay, const int* __restrict__ ints) {
    if (load_stop(ints)) return;
    const long long n = lay.n2();
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        st[lay.SA() + i] = st[lay.W0() + i];
    if (blockIdx.x == 0 && threadIdx.x == 0) st[lay.scal() + S_LOGDET_SA] = st[lay.scal() + S_LOGDET_SA_SHADOW];
}
template <int R, int T>
__global__ __launch_bounds__(T * T) void ctrl_cov_kernel(double* __restrict__ st, StateLayout lay, int H, int which,
                                                         double N, float* __restrict__ S32, int* __restrict__ ints) {
    extern __shared__ __attribute__((aligned(16))) double lds_cov[];
    ctrl_cov_dev<R, T>(st, lay, H, which, N, S32, ints, lds_cov);
}

// ---- lambda_max of a symmetric PSD matrix by LANCZOS on the register-resident matrix (H > 64) -------------------------------------
// History.  H <= 128, rounds 1-3: ten repeated squarings of the LDS-resident fp32 matrix towards the dominant projector, then an fp64
// Rayleigh quotient -- exact (1e-12) when the top gap exceeds 0.5 %, but up to 1.8e-4 off inside a cluster (measured 2.4e-4 on a spectrum
// flat to 0.1 %: tests/test_gpu_lambda_max.py), 25 us at H = 64, 217 us at H = 128.  H > 128: power iteration from registers, 128 fixed
// steps (round 2: ~1e-3 in a cluster), then to a tolerance capped at 2048 steps (round 3) -- which a FLAT spectrum (the delta-Gram of a
// rank-256 fit to rank-16 data) runs into: 3.1 ms per call beside a 0.75 ms pass, and still only ~1e-4, because the power method's error
// in a cluster falls like 1/k.  The Krylov space of the same matrix-vector products does far better (error ~ cosh(2 k sqrt(gap))^-2, exact
// after H steps), for two block-wide dot products more per step:
//     w = G q_j;  alpha_j = q_j'w;  w -= alpha_j q_j + beta_j q_(j-1);  beta_(j+1) = ||w||;  q_(j+1) = w / beta_(j+1)
// and lambda_max(G) ~ the top eigenvalue of the tridiagonal T_k = tridiag(beta, alpha, beta), found by Sturm-count multisection
// (256 shifts per round, 4 rounds: 2e-10 of the trace) at k = 12, 24, 36, 48, 64, 96, 128, 192, 256; the iteration ends when that
// value grew by <= EIG_LANCZOS_TOL since the previous look, at an invariant subspace (beta = 0), or at k = H.  No re-orthogonalisation:
// the copies of converged Ritz values that its absence breeds never exceed lambda_max.  Measured (tests/test_gpu_lambda_max.py: flat,
// Marchenko-Pastur, near-degenerate pair, rank-deficient, dominant, 2^-k, identity): <= 8e-8 relative at H = 128, 130, 200, 256 (and at H = 40 when
// routed here; H <= 64 keeps the squaring kernel below for its speed inside short pass launches).
// Breakdown and restart.  At beta = 0 the vectors so far span an invariant subspace and T_k carries lambda_max of everything q_0
// touches -- which is all it carries: a q_0 that lies in a non-dominant invariant subspace ends there with that subspace's top value.
// The start vector diag(G) / tr + 1e-3 is the all-ones vector on a constant diagonal, and an exact eigenvector of e.g.
// blockdiag([[1 + c, -c], [-c, 1 + c]], ...) (eigenvalue 1 where lambda_max = 1 + 2c: every row of G q_0 is the same fp32 number in any
// summation order, so the first step breaks down exactly).  So a breakdown before k = H does not end the solve: the iteration runs
// again from lanczos_restart_entry's vector -- fixed, positive, non-uniform (an integer hash of the row index in (0.5, 1.5]), no
// random state, the same from run to run -- at most EIG_LANCZOS_RESTARTS times, and the largest value found is returned (each is a
// Ritz value, none exceeds lambda_max beyond the product's rounding).  A step also counts as a breakdown when beta_(j+1) <=
// 2^-16 alpha_0 (alpha_0 = q_0'G q_0 / tr, the scale of the spectrum as q_0 sees it; a row of the fp32 product is good to NP 2^-24
// <= 2^-16 of it at worst): a residual at the rounding of the product means the subspace is invariant as far as this arithmetic can
// tell, and the steps that followed would iterate on rounding that inherits every symmetry G and q_0 share.  Two cases met on the
// device: I + c (e_i - e_j)(e_i - e_j)' from a q_0 with equal entries i and j never leaves the symmetric subspace (rows i and j of
// every product are the same two terms: beta_1 ~ 1e-8 alpha_0, never 0); the paired blocks at odd H, where q_0 spans the eigenvalues 1
// and 1 + c, exhaust at the second step the same way.  An input that meets neither test takes the first pass alone and gets the bits
// it always got.  This is a repair of the cases found, not a guarantee: three fixed start vectors can still all be orthogonal to the
// dominant eigenvector of some matrix (take one built for them), and a q_0 that is NEARLY but not numerically inside a non-dominant
// invariant subspace is resolved only by the rounding that seeds the missing direction before the growth test at two looks 12 steps
// apart gives up (tests/test_gpu_lambda_max_structured.py).
// Layout: NT threads (256 inside a pass launch and for 64 < H <= 128, 1024 for H > 128), matrix padded to NP = 16, 32, 64, 128 or 256.  Thread
// (group = t / NCQ, cq = t % NCQ), NCQ = NP / 16, holds the RB x 16 block G[RB group .. +RB][16 cq .. +16] / tr in registers as fp32
// pairs (the products go out as v_pk_fma_f32: a step is VALU-bound), reads its 16 entries of q from LDS (four 16-byte reads), forms RB
// partial dot products and folds them over the NCQ chunks of its group with DPP moves.  Lane cq < RB of a group OWNS row RB group + cq:
// it keeps q_j and q_(j-1) of that row in fp64.
typedef float f32x2v __attribute__((ext_vector_type(2)));
// sum over the N (1, 2, 4, 8, 16; aligned) neighbouring lanes of a DPP row, the result in each of them: quad_perm [1,0,3,2], quad_perm
// [2,3,0,1], row_half_mirror, row_mirror (cross-lane moves inside the VALU; __shfl_xor would be ds_bpermute round trips through LDS)
template <int N>
__device__ __forceinline__ float rowN_sum(float x) {
    if constexpr (N >= 2) x += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), 0xB1, 0xF, 0xF, true));
    if constexpr (N >= 4) x += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), 0x4E, 0xF, 0xF, true));
    if constexpr (N >= 8) x += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), 0x141, 0xF, 0xF, true));
    if constexpr (N >= 16) x += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), 0x140, 0xF, 0xF, true));
    return x;
}
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double x) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, x);
    const unsigned lo = (unsigned)__builtin_amdgcn_mov_dpp((int)(unsigned)u, CTRL, 0xF, 0xF, true);
    const unsigned hi = (unsigned)__builtin_amdgcn_mov_dpp((int)(unsigned)(u >> 32), CTRL, 0xF, 0xF, true);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ double lane_f64(double x, int l) {          // wave-uniform value of lane l
    const unsigned long long u = __builtin_bit_cast(unsigned long long, x);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), l);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
// sum over the first NT threads of the workgroup (whole waves), the wave stage on DPP + readlane (block_sum's six fp64 __shfl_down steps
// are twelve ds_bpermute round trips); fixed order, every thread gets the same value.  red: NT / 64 doubles.
template <int NT>
__device__ __forceinline__ double block_sum_dpp(double x, double* red) {
    x += dpp_f64<0xB1>(x);
    x += dpp_f64<0x4E>(x);
    x += dpp_f64<0x141>(x);
    x += dpp_f64<0x140>(x);
    const double wsum = (lane_f64(x, 0) + lane_f64(x, 16)) + (lane_f64(x, 32) + lane_f64(x, 48));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = wsum;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) s += red[i];
    return s;
}
// top eigenvalue of the k x k tridiagonal (diagonal al[0..k), squared off-diagonals be2[1..k)) inside [lo, hi] (hi an upper bound of the
// spectrum): `rounds` rounds of 256-way multisection on the Sturm count.  Threads 0..255 count, every thread returns the same value.
__device__ __forceinline__ double tri_lambda_max(const double* al, const double* be2, int k, double lo, double hi, int* imin, int rounds) {
    for (int r = 0; r < rounds; ++r) {
        if (threadIdx.x == 0) *imin = 255;
        __syncthreads();
        const int t = threadIdx.x;
        const double step = (hi - lo) * (1.0 / 256.0);
        if (t < 256) {
            const double x = t == 255 ? hi : lo + step * (double)(t + 1);
            double d = al[0] - x;
            int cnt = d < 0.0 ? 1 : 0;
            // eight steps' LDS reads ahead of the serial rcp chain (stated: the compiler's own choice depends on the loop nest around
            // the call, and without it a look costs 5 % of the solve at H = 128)
#pragma unroll 8
            for (int i = 1; i < k; ++i) {
                if (fabs(d) < 1e-290) d = -1e-290;
                d = al[i] - x - be2[i] * __builtin_amdgcn_rcp(d);
                cnt += d < 0.0 ? 1 : 0;
            }
            if (cnt >= k) atomicMin(imin, t);                   // every eigenvalue lies below x
        }
        __syncthreads();
        const int tm = *imin;
        const double nhi = tm == 255 ? hi : lo + step * (double)(tm + 1);
        const double nlo = tm == 0 ? lo : lo + step * (double)tm;
        __syncthreads();                                        // (imin is reset at the top of the next round)
        lo = nlo; hi = nhi;
    }
    return 0.5 * (lo + hi);
}
constexpr double EIG_LANCZOS_TOL = 2e-7;                        // growth of the top Ritz value between two looks, relative
constexpr int EIG_LANCZOS_RESTARTS = 2;                         // further start vectors after a breakdown before k = H
constexpr double EIG_LANCZOS_EXHAUSTED = 0x1p-32;               // (beta_(j+1) / alpha_0)^2 at or below which the subspace counts as invariant:
                                                                // a row of the fp32 product is good to NP 2^-24 <= 2^-16 at worst
// entry `row` of restart vector `attempt` (1, 2): murmur3's 32-bit finaliser of the pair, its top 24 bits mapped to (0.5, 1.5]
__device__ __forceinline__ double lanczos_restart_entry(int row, int attempt) {
    unsigned x = (unsigned)(row + 1) * 0x9E3779B1u + (unsigned)attempt * 0x85EBCA77u;
    x ^= x >> 16; x *= 0x85EBCA6Bu;
    x ^= x >> 13; x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return 0.5 + (double)((x >> 8) + 1u) * 0x1p-24;
}
// LDS of a call: NP floats (q) + 2 NP + 1 doubles (alpha, beta^2) + 16 doubles + 1 int; the caller hands over >= EIG_LDS_BYTES
constexpr int EIG_LDS_BYTES = 256 * 4 + (2 * 256 + 2) * 8 + 16 * 8 + 16;
// lambda_max(G) / tr for the H x H matrix G (row stride Hp, H <= NP, tr = its trace > 0).  Every one of the NT threads gets the value.
template <int NP, int NT>
__device__ __forceinline__ double lanczos_lambda_max(const double* __restrict__ G, int Hp, int H, double tr, void* lds) {
    constexpr int NCQ = NP / 16;
    constexpr int RB = (NP * NCQ + NT - 1) / NT;                // rows per thread: 4 at NP = 128 / NT = 256 and NP = 256 / NT = 1024, else 1
    static_assert(RB == 1 || RB == 4, "register block");
    static_assert(NCQ >= RB, "one owner lane per row of the block");
    float* vbuf = reinterpret_cast<float*>(lds);
    double* al = reinterpret_cast<double*>(vbuf + 256);
    double* be2 = al + 256;
    double* red = be2 + 258;
    int* imin = reinterpret_cast<int*>(red + 16);
    const int t = threadIdx.x;
    const int grp = t / NCQ, cq = t % NCQ;
    const int row0 = grp * RB;
    const bool active = row0 < NP;
    const bool owner = active && cq < RB;
    const int myrow = row0 + (cq % RB);
    f32x2v g[RB][8];
    {
        const double inv = 1.0 / tr;                            // |G_ij| <= tr: entries in [-1, 1], lambda_max in (0, 1]
#pragma unroll
        for (int r = 0; r < RB; ++r)
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int row = row0 + r, col = cq * 16 + j;
                g[r][j >> 1][j & 1] = (active && row < H && col < H) ? (float)(G[(long long)row * Hp + col] * inv) : 0.f;
            }
    }
    const int kmax = H < NP ? H : NP;
    double best = 0.0;
    for (int attempt = 0; attempt <= EIG_LANCZOS_RESTARTS; ++attempt) {
        // start from the diagonal (a positive vector correlated with the dominant eigenvector of a PSD matrix); after a breakdown from
        // lanczos_restart_entry's fixed non-uniform vector
        double q = 0.0, qp = 0.0, beta = 0.0;
        if (owner && myrow < H) q = attempt == 0 ? G[(long long)myrow * Hp + myrow] / tr + 1e-3 : lanczos_restart_entry(myrow, attempt);
        {
            const double n0 = block_sum_dpp<NT>(q * q, red);
            q *= 1.0 / sqrt(n0);
        }
        if (owner) vbuf[myrow] = (float)q;
        __syncthreads();
        int next_look = 12;
        double theta = 0.0, theta_prev = 0.0, a0 = 0.0;
        bool again = false;                                         // (uniform: alpha and b2 are the same in every thread)
        for (int j = 0; j < kmax; ++j) {
            const float4* v4 = reinterpret_cast<const float4*>(&vbuf[cq * 16]);
            f32x2v a2[RB];
#pragma unroll
            for (int r = 0; r < RB; ++r) a2[r] = f32x2v{0.f, 0.f};
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const float4 v = v4[jj];
                const f32x2v va = {v.x, v.y}, vb = {v.z, v.w};
#pragma unroll
                for (int r = 0; r < RB; ++r) {
                    a2[r] = __builtin_elementwise_fma(g[r][2 * jj], va, a2[r]);
                    a2[r] = __builtin_elementwise_fma(g[r][2 * jj + 1], vb, a2[r]);
                }
            }
            float acc[RB];
#pragma unroll
            for (int r = 0; r < RB; ++r) acc[r] = rowN_sum<NCQ>(a2[r][0] + a2[r][1]);
            float mine = acc[0];
            if constexpr (RB == 4) mine = (cq & 3) == 0 ? acc[0] : ((cq & 3) == 1 ? acc[1] : ((cq & 3) == 2 ? acc[2] : acc[3]));
            double wv = owner ? (double)mine : 0.0;                 // (G q)[myrow]
            const double alpha = block_sum_dpp<NT>(q * wv, red);    // (q = 0 outside the owner lanes)
            wv = owner ? wv - alpha * q - beta * qp : 0.0;
            const double b2 = block_sum_dpp<NT>(wv * wv, red);
            const int k = j + 1;
            if (t == 0) { al[j] = alpha; be2[k] = b2; }
            // breakdown: q_0 .. q_j span an invariant subspace, and T_k carries lambda_max of THAT subspace only.  A residual that is
            // fp32 rounding of the product and nothing else counts too: going on would iterate on that rounding, which keeps every
            // symmetry the matrix and q_0 share
            if (j == 0) a0 = alpha;
            const bool brk = !(b2 > 1e-28) || !(b2 > EIG_LANCZOS_EXHAUSTED * a0 * a0);
            again = brk && k < kmax;
            qp = q;
            beta = sqrt(b2);
            q = brk ? 0.0 : wv / beta;
            if (owner) vbuf[myrow] = (float)q;
            __syncthreads();                                        // q_(j+1), alpha_j, beta_(j+1) are in LDS; every read of q_j is over
            if (brk || k == next_look || k == kmax) {
                theta = tri_lambda_max(al, be2, k, theta_prev > 1e-9 ? theta_prev - 1e-9 : 0.0, 1.0 + 1e-6, imin, 4);
                if (brk || k == kmax || theta - theta_prev <= EIG_LANCZOS_TOL * theta) break;
                theta_prev = theta;
                next_look = k < 48 ? k + 12 : (k < 64 ? 64 : (k < 128 ? k + 32 : k + 64));
            }
        }
        best = theta > best ? theta : best;
        if (!again) break;
    }
    __syncthreads();                                            // the LDS is reused by whatever the block runs next
    return best;
}

// H <= 64: lambda_max by repeated squaring (kept for the small ranks: inside a 20-60 us pass launch of a narrow problem or a short row
// shard its ~11 us (H = 32) / ~25 us (H = 64) are on the critical path, and the Lanczos iteration below, with its three barriers per step,
// measured 2x slower there -- config 2 75 -> 126 us per sweep, the 8-way shard 163 -> 221).  spectral = 0: the trace instead.
//
// Method: NSQ repeated squarings T <- T*T / ||T*T||_F in fp32 (register-tiled, LDS-resident) drive T
// to the dominant eigenprojector; its largest-diagonal column is then polished by two fp64 power
// steps on the ORIGINAL matrix and lambda = Rayleigh quotient in fp64.  The quotient's error is
// quadratic in the vector's error; the worst case over all spectra is <= n/(2e*2^(NSQ+1)) relative
// (~2e-3 at NSQ = 10, n = 64; (1 - r) r^(2^(NSQ+1)) <= 1/(2e 2^NSQ) = 1.8e-4 for two competing eigenvalues of ratio r)
// and ~1e-12 whenever the top gap exceeds 0.5 %.  A cyclic Jacobi solve
// of the same matrix measured 2.9 ms on one CU; this is a few tens of microseconds.
constexpr int EIG_NSQ = 10;

// One squaring of the WIDE form (512 threads, R = 4): the raw C = T * T' on the upper block triangle only, into nxt.
// c_ij and c_ji are the same products in the same order (fmaf(x, y, c) = fmaf(y, x, c)), bitwise equal for ANY T, so the 256-thread
// form computes every off-diagonal entry twice.  Here C is cut into a 4 x 4 grid of 16 x 16 blocks and each of the 10 blocks
// (Ib <= Jb) goes to one 32-lane half of a wave -- five waves, so one SIMD holds two -- as 8 x 4 thread tiles of 2 x 4 entries: 6
// ds_read_b128 per 32 FMAs.  Every entry is the chain of the 256-thread form: k ascending from 0, x, y, z, w within a float4, from 0.f.
// Both operands are ROW reads, as there, so nothing is assumed about the symmetry of the input.  A quad of lanes reads four
// neighbouring column tiles and the eight quads of a half eight neighbouring row tiles: under any grouping of whole quads a
// ds_read_b128 sees distinct rows 4 banks apart or one row (rows r and r + 16 share banks at LD = NP + 4).  The diagonal blocks are
// computed whole (6 % of the work).  The caller's barrier follows.
// What the loop is bound by (profiles/lambda_sq_parts.txt): NOT the FMA issue rate alone.  The 256-thread form's loop, as compiled, is
// v_pk_fma_f32 at full rate plus 8 ds_read_b128 per step that it waits for before it multiplies; the triangle halves the FMAs, but
// 2 x 4 tiles read as many bytes from LDS as 4 x 4 tiles on the whole matrix (480 against 512 ds_read_b128 per squaring), and a first
// version that waited for each step's reads in the same way took the parent's time per squaring (3.8 against 3.6 us at H = 64).  So:
//   * the reads of k-step s + 1 are issued ahead of the FMAs of step s, in two register sets, and the scheduler is held to that order
//     (sched_barrier): left alone it either gathers the reads of two steps in front of their FMAs again, or -- with fmaf() -- packs
//     pairs of chains into v_pk_fma_f32 at the price of a v_mov_b32 per FMA pair, which was no faster than the parent;
//   * the FMAs are written as v_fmac_f32, one chain step each: the same fused multiply-add as fmaf() (one rounding, the mode
//     register's denormal setting), which the packer cannot touch.
// 2.4 us per squaring at H = 64 (3.6 in the 256-thread form).  At R = 2 (1 x 2 tiles) the same form measured no gain -- ten squarings
// 20.0 -> 19.5-20.0 us: 0.8 us of each squaring's 1.1 are the fp64 sum, its tree and the scale -- so R = 2 keeps the 256-thread form.
template <int R>
__device__ __forceinline__ void eig_square_tri(const float* __restrict__ cur, float* __restrict__ nxt) {
    static_assert(R == 4, "thread tiles of 2 x 4 on a 64 x 64 matrix");
    constexpr int TR = R / 2, TC = R, NP = 16 * R, LD = NP + 4;
    const int hw = threadIdx.x >> 5;                             // block = 32-lane half: (0,0) (0,1) (0,2) (0,3) (1,1) (1,2) (1,3) (2,2) (2,3) (3,3)
    if (hw >= 10) return;
    const int Ib = hw < 4 ? 0 : (hw < 7 ? 1 : (hw < 9 ? 2 : 3));
    const int Jb = hw < 4 ? hw : (hw < 7 ? hw - 3 : (hw < 9 ? hw - 5 : 3));
    const int l = threadIdx.x & 31;
    const int i0 = (8 * Ib + (l >> 2)) * TR, j0 = (4 * Jb + (l & 3)) * TC;     // i0 + TR <= NP, j0 + TC <= NP
    float c[TR][TC];
#pragma unroll
    for (int a = 0; a < TR; ++a)
#pragma unroll
        for (int b = 0; b < TC; ++b) c[a][b] = 0.f;
    const float* pa = cur + i0 * LD;
    const float* pb = cur + j0 * LD;
    float4 ai[2][TR], bj[2][TC];
    auto load = [&](int s, int k) {
#pragma unroll
        for (int a = 0; a < TR; ++a) ai[s][a] = *reinterpret_cast<const float4*>(pa + a * LD + k);
#pragma unroll
        for (int b = 0; b < TC; ++b) bj[s][b] = *reinterpret_cast<const float4*>(pb + b * LD + k);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto mac = [&](int s) {
#pragma unroll
        for (int a = 0; a < TR; ++a)
#pragma unroll
            for (int b = 0; b < TC; ++b) {
                asm("v_fmac_f32 %0, %1, %2" : "+v"(c[a][b]) : "v"(ai[s][a].x), "v"(bj[s][b].x));
                asm("v_fmac_f32 %0, %1, %2" : "+v"(c[a][b]) : "v"(ai[s][a].y), "v"(bj[s][b].y));
                asm("v_fmac_f32 %0, %1, %2" : "+v"(c[a][b]) : "v"(ai[s][a].z), "v"(bj[s][b].z));
                asm("v_fmac_f32 %0, %1, %2" : "+v"(c[a][b]) : "v"(ai[s][a].w), "v"(bj[s][b].w));
            }
        __builtin_amdgcn_sched_barrier(0);
    };
    load(0, 0);
#pragma unroll
    for (int k = 0; k < NP; k += 8) {
        load(1, k + 4);
        mac(0);
        if (k + 8 < NP) load(0, k + 8);
        mac(1);
    }
#pragma unroll
    for (int a = 0; a < TR; ++a)
#pragma unroll
        for (int b = 0; b < TC; ++b) nxt[(i0 + a) * LD + j0 + b] = c[a][b];
}

// which = 0: GD -> S_LAMD, 1: GB -> S_LAMB_NEW.  256 threads, 2*NP*(NP+4) floats of LDS (NP = 16R).
// wide (R = 4; uniform; the block then has 512 threads -- eig_kernel and ctrl_chain_kernel, never a pass launch, whose control
// workgroups have no spare waves at H <= 64): the products of a squaring come from eig_square_tri.  Every value stored is bitwise the
// 256-thread form's: the raw entries go through LDS, the first 256 threads -- (ty, tx) of that form -- read their R x R cyclic
// entries back (the lower ones from their mirror), form the Frobenius sum in its (a, b) order, block_sum runs its tree on those same
// 256 positions (ctrl_nthreads() = 256: the other waves' partial sums, exact zeros, are not even read), and the owners scale and
// store what they hold.  One barrier more per squaring than the 256-thread form.  The first load of the matrix is dealt over all 512
// threads (one correctly rounded fp64 division per entry, whoever does it).  tests/test_gpu_lambda_max_bits.py holds lambda to the
// 256-thread form's bits.
template <int R>
__device__ __forceinline__ void eig_squaring_dev(double* __restrict__ st, StateLayout lay, int H, int spectral, int which,
                                        const int* __restrict__ ints, float* ldsf, int slot, bool check_stop, bool wide) {
    __shared__ double red[16];
    __shared__ int s_arg;
    if (check_stop && load_stop(ints)) return;
    const int Hp = lay.Hp;
    const double* G = st + (which == 0 ? lay.GD() : lay.GB());
    double* scal = st + lay.scal();
    double tr = 0.0;
    for (int i = threadIdx.x; i < H; i += ctrl_nthreads()) tr += G[(long long)i * Hp + i];
    tr = block_sum(tr, red);
    if (!spectral || !(tr > 0.0) || !isfinite(tr)) {        // zero matrix -> 0; NaN propagates (loop exit on NaN d)
        if (threadIdx.x == 0) scal[slot] = tr;
        return;
    }
    // rows padded to LD = NP + 4 floats: 16-byte aligned row starts for ds_read_b128, and the 16 rows a
    // wave reads side by side start 4 banks apart (conflict-free)
    constexpr int T = 16, NP = T * R, LD = NP + 4;
    float* A0 = ldsf;
    float* A1 = ldsf + NP * LD;
    const int tx = threadIdx.x % T, ty = threadIdx.x / T;
    for (int t = threadIdx.x; t < NP * NP; t += wide ? 512 : ctrl_nthreads()) {
        const int i = t / NP, j = t - i * NP;
        A0[i * LD + j] = (i < H && j < H) ? (float)(G[(long long)i * Hp + j] / tr) : 0.f;   // |G_ij| <= tr: no overflow
    }
    __syncthreads();
    float* cur = A0;
    float* nxt = A1;
    for (int sq = 0; sq < EIG_NSQ; ++sq) {
        float c[R][R];
        if (wide) {
            // upper block triangle of C on five waves, raw into nxt; the 256 owners pick their old entries up from there
            if constexpr (R == 4) eig_square_tri<R>(cur, nxt);
            __syncthreads();
            if (threadIdx.x < 256) {
#pragma unroll
                for (int a = 0; a < R; ++a)
#pragma unroll
                    for (int b = 0; b < R; ++b) {
                        const int i = ty + T * a, j = tx + T * b;
                        c[a][b] = nxt[min(i, j) * LD + max(i, j)];
                    }
            }
        } else {
#pragma unroll
            for (int a = 0; a < R; ++a)
#pragma unroll
                for (int b = 0; b < R; ++b) c[a][b] = 0.f;
            for (int k = 0; k < NP; k += 4) {                // C = T * T' (T symmetric): both operands are row reads
                float4 ai[R], bj[R];
#pragma unroll
                for (int a = 0; a < R; ++a) ai[a] = *reinterpret_cast<const float4*>(cur + (ty + T * a) * LD + k);
#pragma unroll
                for (int b = 0; b < R; ++b) bj[b] = *reinterpret_cast<const float4*>(cur + (tx + T * b) * LD + k);
#pragma unroll
                for (int a = 0; a < R; ++a)
#pragma unroll
                    for (int b = 0; b < R; ++b) {
                        c[a][b] = fmaf(ai[a].x, bj[b].x, c[a][b]);
                        c[a][b] = fmaf(ai[a].y, bj[b].y, c[a][b]);
                        c[a][b] = fmaf(ai[a].z, bj[b].z, c[a][b]);
                        c[a][b] = fmaf(ai[a].w, bj[b].w, c[a][b]);
                    }
            }
        }
        const bool owner = !wide || threadIdx.x < 256;       // (ty, tx) of the 256-thread form: its sum, its tree, its stores
        double ss = 0.0;
        if (owner) {
#pragma unroll
            for (int a = 0; a < R; ++a)
#pragma unroll
                for (int b = 0; b < R; ++b) ss += (double)c[a][b] * (double)c[a][b];
        }
        ss = block_sum(ss, red);                             // ||T^2||_F^2 with ||T||_F = 1: -> 1 iff T is a rank-1 projector
        const float sc = (ss > 0.0) ? (float)(1.0 / sqrt(ss)) : 0.f;
        if (owner) {                                         // (wide: every read of the raw entries is behind block_sum's barriers)
#pragma unroll
            for (int a = 0; a < R; ++a)
#pragma unroll
                for (int b = 0; b < R; ++b) nxt[(ty + T * a) * LD + tx + T * b] = c[a][b] * sc;
        }
        __syncthreads();
        float* tmp = cur; cur = nxt; nxt = tmp;
        if (sq > 0 && fabs(ss - 1.0) < 1e-5) break;          // uniform: converged to the dominant projector (the fp64
                                                             // Rayleigh quotient below squares what is left of the error)
    }
    // dominant column = the one with the largest diagonal entry of the (near) projector
    if (threadIdx.x < 64) {
        float best = -1.f; int arg = 0;
        for (int i = threadIdx.x; i < H; i += 64) { const float v = cur[i * LD + i]; if (v > best) { best = v; arg = i; } }
        for (int off = 32; off > 0; off >>= 1) {
            const float ob = __shfl_down(best, off); const int oa = __shfl_down(arg, off);
            if (ob > best) { best = ob; arg = oa; }
        }
        if (threadIdx.x == 0) s_arg = arg;
    }
    __syncthreads();
    // lambda = v'Gv / v'v in fp64 on the ORIGINAL matrix (error quadratic in v's error).  4 threads per
    // row, each a contiguous quarter of it.
    double num = 0.0, den = 0.0;
    {
        const int i = threadIdx.x >> 2, q = threadIdx.x & 3;
        for (int i0 = 0; i0 < H; i0 += 64) {
            const int row = i0 + i;
            if (row < H) {
                const int jn = (H + 3) / 4, j0 = q * jn, j1 = min(H, j0 + jn);
                double acc = 0.0;
                for (int j = j0; j < j1; ++j) acc += G[(long long)row * Hp + j] * (double)cur[j * LD + s_arg];
                const double vi = (double)cur[row * LD + s_arg];
                num += vi * acc;
                if (q == 0) den += vi * vi;
            }
        }
    }
    num = block_sum(num, red);
    den = block_sum(den, red);
    if (threadIdx.x == 0) scal[slot] = den > 0.0 ? num / den : 0.0;
    __syncthreads();                                         // LDS is reused by whatever the block runs next
}

// lambda_max of a symmetric PSD H x H matrix: which = 0: GD -> S_LAMD, 1: GB -> S_LAMB_NEW (the slot is the caller's).
// check_stop = false: the caller has taken the stop decision for the whole workgroup (the per-thread test here is safe only where
// no other workgroup of the launch can raise the flag meanwhile: threads that disagreed would leave block_sum's barriers unmatched).
// spectral = 0: Frobenius surrogate (trace) instead.  256 threads (the first 256 of a 512-thread pass launch).  H <= 64: repeated squaring
// (2 * NP * (NP + 4) floats of LDS); 64 < H <= 128: Lanczos (EIG_LDS_BYTES).
// WIDE_OK: the caller is a kernel of the chain's own (eig_kernel, ctrl_chain_kernel), which the host launches with 512 threads
// exactly where the wide squaring applies (eig_wide_launch in vbmf_hip.hip: R = 4 and not the Lanczos switch) and with 256 otherwise.
template <int R, bool WIDE_OK = false>
__device__ __forceinline__ void eig_dev(double* __restrict__ st, StateLayout lay, int H, int spectral, int which,
                                        const int* __restrict__ ints, float* ldsf, int slot, bool check_stop = true) {
    if (R <= 4 && __builtin_expect(!(spectral & 2), 1)) {       // (uniform over the launch; the other branch is a switch: cold)
        const bool wide = WIDE_OK && R == 4 && blockDim.x == 512u;
        eig_squaring_dev<R>(st, lay, H, spectral & 1, which, ints, ldsf, slot, check_stop, wide);
    } else {
        __shared__ double red[16];
        if (check_stop && load_stop(ints)) return;
        const int Hp = lay.Hp;
        const double* G = st + (which == 0 ? lay.GD() : lay.GB());
        double* scal = st + lay.scal();
        double tr = 0.0;
        for (int i = threadIdx.x; i < H; i += ctrl_nthreads()) tr += G[(long long)i * Hp + i];
        tr = block_sum(tr, red);
        if (!(spectral & 1) || !(tr > 0.0) || !isfinite(tr)) {  // zero matrix -> 0; NaN propagates (loop exit on NaN d)
            if (threadIdx.x == 0) scal[slot] = tr;
            return;
        }
        const double theta = lanczos_lambda_max<16 * R, 256>(G, Hp, H, tr, ldsf);
        if (threadIdx.x == 0) scal[slot] = tr * theta;
    }
}

template <int R>
__global__ __launch_bounds__(R == 4 ? 512 : 256) void eig_kernel(double* __restrict__ st, StateLayout lay, int H, int spectral,
                                                  int do_d, int do_b, const int* __restrict__ ints) {
    extern __shared__ __attribute__((aligned(16))) float lds_eig[];
    const int which = blockIdx.x;           // 0: GD, 1: GB
    if ((which == 0 && !do_d) || (which == 1 && !do_b)) return;
    eig_dev<R, true>(st, lay, H, spectral, which, ints, lds_eig, which == 0 ? S_LAMD : S_LAMB_NEW);
}

// H > 128: the same iteration on 1024 threads (NP = 256)
__global__ __launch_bounds__(1024) void eig_lanczos_kernel(double* __restrict__ st, StateLayout lay, int H, int spectral,
                                                           int do_d, int do_b, const int* __restrict__ ints) {
    __shared__ double red[16];
    __shared__ __attribute__((aligned(16))) unsigned char lds_lz[EIG_LDS_BYTES];
    if (load_stop(ints)) return;
    const int which = blockIdx.x;           // 0: GD, 1: GB
    if ((which == 0 && !do_d) || (which == 1 && !do_b)) return;
    const int Hp = lay.Hp;
    const double* G = st + (which == 0 ? lay.GD() : lay.GB());
    double* scal = st + lay.scal();
    const int slot = which == 0 ? S_LAMD : S_LAMB_NEW;
    double tr = 0.0;
    for (int i = threadIdx.x; i < H; i += (int)blockDim.x) tr += G[(long long)i * Hp + i];
    tr = block_sum(tr, red);
    if (!(spectral & 1) || !(tr > 0.0) || !isfinite(tr)) {
        if (threadIdx.x == 0) scal[slot] = tr;
        return;
    }
    const double theta = lanczos_lambda_max<256, 1024>(G, Hp, H, tr, lds_lz);
    if (threadIdx.x == 0) scal[slot] = tr * theta;
}

// flags: bit0 est_covs->CA, bit1 est_covs->CB, bit2 est_var, bit3 compute d + loop bookkeeping,
//        bit4 (unused; tr(Y'BA') is always the direct sum st[GX] = sum (Y A) o BHat left by the kernel that produced BHat,
//             or by prepare_trYBA -- the Gram identity tr(KB o GB) it replaces is exact only for an un-rounded BHat),
//        bit5 S_LAMB_PREV already holds lambda_max of the old B'B (no rotation from S_LAMB_NEW)
//        bit6 split schedule (ctrl_chain): the d / loop part (bit3) is done by ctrl_loop_dev in another workgroup;
//             this call only files sigma2 / ELBO / residual in trace row it_row
//
// ho (the Gram form's first chain launch, ctrl_chain): the SigmaA update that follows in the same workgroup takes over what this
// function holds instead of starting again from memory.  The loop that feeds the trace term leaves B'B + L SigmaB -- the fp64
// expression ctrl_cov_dev's elem() forms -- in the inverse's LDS image (np x (np + 2), identity padding), and the final sigma2 and
// this thread's CA entry come back in ho; live = the function ran (its stop decision, which is uniform over the launch).
struct EndHandOff {
    double* img; int np;           // in: the image and its order (16 NB)
    double sigma2, ca_h;           // out: sigma2 after the update; CA[threadIdx.x] after the update (threads < H)
    bool live;                     // out: not stopped
};
__device__ __forceinline__ void ctrl_end_dev(double* __restrict__ st, StateLayout lay, int H, double Lg, double M,
                                             int flags, double eps, double* __restrict__ trace,
                                             int* __restrict__ ints, int it_row, EndHandOff& ho, bool handoff,
                                             int* __restrict__ hw = nullptr) {
    // Inside a pass launch every dependent round trip to memory costs microseconds (the chip is streaming at full HBM
    // bandwidth around this workgroup), so everything the function needs is requested up front in ONE round -- the stop
    // flag, the scalars, the old CA/CB, the H x H arrays -- and the later stages work from registers and LDS.
    __shared__ double red[16];
    __shared__ double sc_s[32];
    __shared__ double dg[4][256];                                // diagonals of GA, SA, GB, SB
    const int Hp = lay.Hp;
    const double* GA = st + lay.GA();
    const double* GB = st + lay.GB();
    const double* SA = st + lay.SA();
    const double* SB = st + lay.SB();
    double* ca = st + lay.ca();
    double* cb = st + lay.cb();
    double* scal = st + lay.scal();
    // Split schedule (flags & 64): the loop test of THIS sweep runs beside this function in another workgroup of the same
    // launch (ctrl_loop_dev) and marks the stop flag with it_row + 1; CA/CB/sigma2 of the sweep it stops at are still due, so
    // that value does not count as "stopped" here -- whichever of the two workgroups gets there first.
    int stopped = load_stop(ints);
    if ((flags & 64) && stopped == it_row + 1) stopped = 0;
    const int hme = threadIdx.x;                                 // H <= 256 <= ctrl_nthreads(): one diagonal entry per thread
    const double scv = hme < 32 ? scal[hme] : 0.0;
    const double trdot = st[lay.GX()];                           // tr(Y'BA') = sum (Y A) o BHat, summed where BHat was produced
    double ca_h = hme < H ? ca[hme] : 1.0, cb_h = hme < H ? cb[hme] : 1.0;

    // tr((A'A + M SigmaA)(B'B + L SigmaB)); 8 elements per thread and round, all loads before the first use
    double t2 = 0.0;
    {
        constexpr int U = 8;
        const int sh = 31 - __clz(Hp), total = Hp * Hp;          // Hp is a power of two
        for (int e0 = threadIdx.x; e0 < total; e0 += U * ctrl_nthreads()) {
            double gb[U], ga[U], sa[U], sb[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int e = e0 + u * ctrl_nthreads();
                const bool ok = e < total && (e >> sh) < H && (e & (Hp - 1)) < H;
                const int ee = ok ? e : 0;
                gb[u] = GB[ee]; ga[u] = GA[ee]; sa[u] = SA[ee]; sb[u] = SB[ee];
                if (!ok) { ga[u] = 0.0; sa[u] = 0.0; }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int e = e0 + u * ctrl_nthreads();
                const int i = e >> sh, j = e & (Hp - 1);
                if (e < total && i == j && i < H) { dg[0][i] = ga[u]; dg[1][i] = sa[u]; dg[2][i] = gb[u]; dg[3][i] = sb[u]; }
                const double kb = gb[u] + Lg * sb[u];
                t2 += (ga[u] + M * sa[u]) * kb;
                if (handoff && e < total && i < ho.np && j < ho.np)
                    ho.img[i * (ho.np + 2) + j] = (i < H && j < H) ? kb : (i == j ? 1.0 : 0.0);
            }
        }
    }
    ho.live = !stopped;
    if (stopped) return;                                         // uniform
    if (hme < 32) sc_s[hme] = scv;
    t2 = block_sum(t2, red);                                     // (its barriers publish sc_s and dg)
    const double trYBA = trdot;
    const double resid = sc_s[S_TRYY] - 2.0 * trYBA + t2;
    double e = 0.0;
    if (hme < H) {
        const double gaa = dg[0][hme], saa = dg[1][hme], gbb = dg[2][hme], sbb = dg[3][hme];
        if (flags & 1) { ca_h = gaa / M + saa; ca[hme] = ca_h; }
        if (flags & 2) { cb_h = gbb / Lg + sbb; cb[hme] = cb_h; }
        // build-defined ELBO, with the post-update CA, CB, sigma2
        e += -(M / 2.0) * log(ca_h) - 0.5 * (gaa + M * saa) / ca_h;
        e += -(Lg / 2.0) * log(cb_h) - 0.5 * (gbb + Lg * sbb) / cb_h;
    }
    double sigma2 = sc_s[S_SIGMA2];
    if (flags & 4) sigma2 = resid / (Lg * M);
    e = block_sum(e, red);
    ho.sigma2 = sigma2; ho.ca_h = ca_h;
    if (threadIdx.x == 0) {
        const double PI2 = 6.283185307179586476925286766559;
        double F = -(Lg * M / 2.0) * log(PI2 * sigma2) - resid / (2.0 * sigma2) + e;
        F += (M / 2.0) * sc_s[S_LOGDET_SA] + M * H / 2.0 + (Lg / 2.0) * sc_s[S_LOGDET_SB] + Lg * H / 2.0;
        scal[S_SIGMA2] = sigma2;
        scal[S_ELBO] = F;
        scal[S_RESID] = resid;
        scal[S_TRYBA] = trYBA;
        if (flags & 64) {
            if (trace) { trace[4 * it_row + 1] = sigma2; trace[4 * it_row + 2] = F; trace[4 * it_row + 3] = resid; }
        } else if (flags & 8) {
            const double d = sqrt(sc_s[S_LAMD] / sc_s[S_LAMB_PREV]);
            scal[S_D] = d;
            if (!(flags & 32)) scal[S_LAMB_PREV] = sc_s[S_LAMB_NEW];   // (32: lambda_max of the old B is written there directly)
            const int it = ints[I_ITERS];
            if (trace) { trace[4 * it + 0] = d; trace[4 * it + 1] = sigma2; trace[4 * it + 2] = F; trace[4 * it + 3] = resid; }
            ints[I_ITERS] = it + 1;
            const bool rerr = stop_on_remote_error(st, lay, ints);
            const bool stop = !(d > eps) || it + 1 >= ints[I_NITER] || rerr;   // src/vbmf.jl:193 (NaN d exits too)
            if (stop) __hip_atomic_store(ints + I_STOP, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            publish_loop_words(hw, ints, stop ? 1 : 0, it + 1);
        }
    }
    // (no device-scope fence here: the consumers are later kernels -- the launch boundary publishes these stores -- or this
    //  same workgroup after the barrier; on gfx950 an agent-scope release writes back the XCD's whole L2, which costs
    //  several microseconds inside a pass that is filling that L2 with its own output)
    __syncthreads();
}

__device__ __forceinline__ void ctrl_end_dev(double* __restrict__ st, StateLayout lay, int H, double Lg, double M,
                                             int flags, double eps, double* __restrict__ trace,
                                             int* __restrict__ ints, int* __restrict__ hw) {
    EndHandOff none{nullptr, 0, 0.0, 1.0, false};
    ctrl_end_dev(st, lay, H, Lg, M, flags, eps, trace, ints, -1, none, false, hw);
}

__global__ __launch_bounds__(1024) void ctrl_end_kernel(double* __restrict__ st, StateLayout lay, int H, double Lg,
                                                       double M, int flags, double eps,
                                                       double* __restrict__ trace, int* __restrict__ ints,
                                                       int* __restrict__ hw) {
    ctrl_end_dev(st, lay, H, Lg, M, flags, eps, trace, ints, hw);
}

// SigmaA (into the shadow) right behind ctrl_end_dev in the same workgroup: the image holds B'B + L SigmaB, the diagonal takes
// sigma2 / CA_ii -- the two roundings of ctrl_cov_dev's elem(), in its order -- then the sweep and the write-back of ctrl_cov_dev.
// No stop decision of its own: ctrl_end_dev's (ho.live) stands for both, and a SigmaA left in the shadow just before a stop is
// never committed.
// VBMF_SEAM_STAMPS (diagnostic builds only, off by default: the shipped kernels execute no extra stamp): durations of the segments
// of the two fused steps in 10 ns ticks, in the chain stamps' slots 4-7 (the streaming epilogue's, idle in a Gram-form sweep):
// [4] part 2 of the first chain launch (lambda_max(B_old'B_old), stamped in ctrl_chain; the other two parts are slots 0-2),
// [5] SigmaA diagonal add + sweep, [6] SigmaA write-back + log-determinant, [7] SigmaB: assembly << 40 | sweep << 20 | write-back
#ifndef VBMF_SEAM_STAMPS
#define VBMF_SEAM_STAMPS 0
#endif
template <int R>
__device__ __forceinline__ void cov_a_after_end_dev(double* __restrict__ st, StateLayout lay, int H, const EndHandOff& ho,
                                                    float* __restrict__ S32, int* __restrict__ ints) {
    constexpr int LD = 16 * R + 2;
#if VBMF_SEAM_STAMPS
    const unsigned long long s0 = wall_clock64();
#endif
    if ((int)threadIdx.x < H) ho.img[threadIdx.x * LD + threadIdx.x] += ho.sigma2 / ho.ca_h;   // (ctrl_end_dev ended on a barrier)
    double ldK; int badK;
    spd_sweep_lds4<R>(ho.img, H, &ldK, &badK);
#if VBMF_SEAM_STAMPS
    __syncthreads();
    const unsigned long long s2 = wall_clock64();
#endif
    cov_store_lds4<R>(st, lay, H, 0, ho.sigma2, S32, ints, ho.img, ldK, badK, true);
#if VBMF_SEAM_STAMPS
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long* stamp = reinterpret_cast<unsigned long long*>(ints + 8);
        stamp[5] = s2 - s0; stamp[6] = wall_clock64() - s2;
    }
#endif
}

// The Gram form's second chain launch: commit of the SigmaA shadow and SigmaB in one pass over the operands.  One round of loads of
// the shadow and A'A per thread; from registers SigmaA goes to the state and A'A + M SigmaA (then sigma2 / CB_ii onto the diagonal:
// the two roundings of elem() in ctrl_cov_dev, which = 1, in its order) into the inverse's image, so SigmaB does not wait for the commit's stores to come back.  Thread 0 also
// commits the shadow's log-determinant and lambda_max(B_old'B_old) (S_LAMB_SHADOW, computed ahead by part 2 of the first launch).
// Everything sits behind one stop gate: a stopped loop commits nothing and computes no SigmaB.
template <int R>
__device__ __forceinline__ void commit_cov_b_dev(double* __restrict__ st, StateLayout lay, int H, double M,
                                                 float* __restrict__ S32, int* __restrict__ ints, double* W) {
    if (load_stop(ints)) return;                               // uniform: no workgroup writes the flag during this launch
#if VBMF_SEAM_STAMPS
    const unsigned long long s0 = wall_clock64();
#endif
    constexpr int NP = 16 * R, LD = NP + 2, U = 16;
    const int Hp = lay.Hp, sh = 31 - __clz(Hp), n = Hp * Hp;   // Hp is a power of two; n a multiple of 4 * 256
    const double* src = st + lay.W0();
    const double* GA = st + lay.GA();
    const double* cb = st + lay.cb();
    double* dst = st + lay.SA();
    double* scal = st + lay.scal();
    const double sigma2 = scal[S_SIGMA2];
    const double cb_t = (int)threadIdx.x < H ? cb[threadIdx.x] : 1.0;
    for (int e0 = threadIdx.x; e0 < n; e0 += U * 256) {
        double sa[U], ga[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = e0 + u * 256;
            const int ee = e < n ? e : 0;
            sa[u] = src[ee]; ga[u] = GA[ee];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = e0 + u * 256;
            if (e >= n) continue;
            const int i = e >> sh, j = e & (Hp - 1);
            dst[e] = sa[u];
            if (i < NP && j < NP) W[i * LD + j] = (i < H && j < H) ? ga[u] + M * sa[u] : (i == j ? 1.0 : 0.0);   // identity padding
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < H) W[threadIdx.x * LD + threadIdx.x] += sigma2 / cb_t;   // the second rounding of elem()'s diagonal
    if (threadIdx.x == 0) {
        scal[S_LOGDET_SA] = scal[S_LOGDET_SA_SHADOW];
        scal[S_LAMB_PREV] = scal[S_LAMB_SHADOW];
    }
    double ldK; int badK;
#if VBMF_SEAM_STAMPS
    __syncthreads();
    const unsigned long long s1 = wall_clock64();
#endif
    spd_sweep_lds4<R>(W, H, &ldK, &badK);
#if VBMF_SEAM_STAMPS
    __syncthreads();
    const unsigned long long s2 = wall_clock64();
#endif
    cov_store_lds4<R>(st, lay, H, 1, sigma2, S32, ints, W, ldK, badK, false);
#if VBMF_SEAM_STAMPS
    __syncthreads();
    if (threadIdx.x == 0)
        reinterpret_cast<unsigned long long*>(ints + 8)[7] = ((s1 - s0) << 40) | ((s2 - s1) << 20) | (wall_clock64() - s2);
#endif
}

// ---- the control chain as run by workgroup 0 of a streaming-pass launch ----------------------------
// The H x H algebra of a sweep depends only on Grams that are complete before the pass is launched
// and produces what the kernels AFTER the pass need, so one extra workgroup of the pass runs it while
// the others stream: one stream, no events, kernel boundaries give all ordering and visibility.
struct CtrlArgs {
    double* st; StateLayout lay; int* ints; double* trace;
    float* S32;            // SigmaA/sigma2 (pass 1) or SigmaB/sigma2 (pass 2) table for the post kernel
    double Lg, M, eps;
    int H, spectral, end_flags;
    int mode;              // CTRL_* bits; 0: no control workgroups in this launch
    int it_row;            // sweep index (trace row) the CTRL_PREV_END part finalises
    int* sready; int sready_val;   // release flag for the Sigma table of part 0 (the pass's register epilogue waits on it)
    int* loopw;            // the run loop's host-mapped {stop, iters, err} (publish_loop_words); nullptr outside a run
};
// Schedule inside vbmf_run (sweep j; B_{j-1} is the factor the sweep starts from):
//   pass 1 of sweep j : [lambda_max(dB'dB) of sweep j-1, ctrl_end of sweep j-1]  then  SigmaA of sweep j
//   pass 2 of sweep j : SigmaB of sweep j  and  lambda_max(B_{j-1}'B_{j-1})  (the denominator of d_j; the
//                       Gram of B_{j-1} is still in place: post(B) of sweep j runs after this launch)
// so each pass carries a chain of similar length (~75 / ~65 us at H = 64).
// The Gram form has no pass launches: the same two parts run as a launch of their own (ctrl_chain_kernel),
// and the commit of the SigmaA shadow rides in the SigmaB launch ahead of SigmaB (CTRL_COMMIT_A).
enum : int { CTRL_PREV_END = 1, CTRL_COV_A = 2, CTRL_COV_B = 4, CTRL_EIG_BOLD = 8, CTRL_COMMIT_A = 16, CTRL_EIG_AHEAD = 32 };

// d = ||B_old - B_new||_2 / ||B_old||_2 (src/util.jl:27-29) and the loop test (src/vbmf.jl:193) of sweep it_row
__device__ __forceinline__ void ctrl_loop_dev(double* __restrict__ st, StateLayout lay, double eps,
                                              double* __restrict__ trace, int* __restrict__ ints, int it_row,
                                              int* __restrict__ hw) {
    if (load_stop(ints)) return;
    if (threadIdx.x == 0) {
        double* scal = st + lay.scal();
        const double d = sqrt(scal[S_LAMD] / scal[S_LAMB_PREV]);
        scal[S_D] = d;
        if (trace) trace[4 * it_row + 0] = d;
        ints[I_ITERS] = it_row + 1;
        const bool rerr = stop_on_remote_error(st, lay, ints);
        const bool stop = !(d > eps) || it_row + 1 >= ints[I_NITER] || rerr;   // NaN d exits too
        if (stop) __hip_atomic_store(ints + I_STOP, it_row + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // non-zero = stop; the
                                                                            // value names the sweep (see ctrl_end_dev)
        publish_loop_words(hw, ints, stop ? it_row + 1 : 0, it_row + 1);
    }
    // (see ctrl_end_dev: no device-scope fence; the stop flag itself is an agent-scope atomic)
    __syncthreads();
}

// The chain is split over the launch's first TWO workgroups (what bounds a pass launch on a short row shard is this
// chain, not the streaming: 83 us per launch on a 12.5k-row shard before the split):
//   part 0:  [CA, CB, sigma2, ELBO of the previous sweep]  ->  SigmaA (speculative: into the shadow, committed by
//            commit_cov_a_kernel after the launch iff the loop continues)            |  SigmaB
//   part 1:  lambda_max(dB'dB) -> d, trace, iteration count, stop                    |  lambda_max(B_old'B_old)
// Part 1's stop decision does not wait for part 0 and vice versa; CA/CB/sigma2 belong to the finished sweep and are
// due whether or not the loop stops, SigmaA belongs to the next one and is not.
// Durations of the chain's parts in 10 ns ticks of the constant 100 MHz clock, kept in ints[8..15] as four 64-bit slots
// (vbmf_debug_peek(VBMF_PEEK_CHAIN)): [0] ctrl_end, [1] SigmaA, [2] lambda_max(dB'dB) + loop test, [3] SigmaB
//
// SEAMS (ctrl_chain_kernel, the Gram form's launches of the chain alone; the pass launches of the streaming path keep the schedule
// above, two control workgroups and every step starting from memory):
//   * part 0 of the first launch hands ctrl_end_dev's operands on to SigmaA (EndHandOff, cov_a_after_end_dev): one round of loads
//     and one stop decision for both;
//   * part 0 of the second launch commits the shadow and assembles SigmaB's matrix from the same registers (commit_cov_b_dev);
//   * lambda_max(B_old'B_old) is part 2 -- a THIRD workgroup -- of the first launch (CTRL_EIG_AHEAD), where it hides behind part 0,
//     instead of part 1 of the second, which it bounded.  B'B is in place when the first launch starts.  Part 1 of that launch reads
//     S_LAMB_PREV (for d of the previous sweep) at the same moment, so part 2 writes S_LAMB_SHADOW and thread 0 of the second
//     launch's part 0 moves it to S_LAMB_PREV beside the commit, behind the same stop gate: S_LAMB_PREV changes exactly when it did.
//     Part 2's stop decision is taken ONCE for the workgroup (thread 0 reads, barrier): part 1 may raise the flag while part 2
//     starts, and threads that disagreed would leave block_sum's barriers unmatched.  As in ctrl_end_dev, the value it_row + 1
//     that part 1 stores during this launch does not count, so the decision -- and with it S_LAMB_SHADOW -- does not depend on
//     which of the two workgroups gets there first; launches enqueued past a stop do no work.
// No part waits for another one of its launch.
template <int R, bool SEAMS = false>
__device__ __forceinline__ void ctrl_chain(const CtrlArgs& a, void* lds, int part) {
    unsigned long long* stamp = reinterpret_cast<unsigned long long*>(a.ints + 8);
    const unsigned long long t0 = wall_clock64();
    if (SEAMS && part == 2) {
        __shared__ int stop2_s;
        if (threadIdx.x == 0) {
            const int f = load_stop(a.ints);
            stop2_s = (f != 0 && f != a.it_row + 1) ? 1 : 0;
        }
        __syncthreads();
        if (stop2_s) return;
        if (a.mode & CTRL_EIG_AHEAD)
            eig_dev<R, SEAMS>(a.st, a.lay, a.H, a.spectral, 1, a.ints, reinterpret_cast<float*>(lds), S_LAMB_SHADOW, false);
#if VBMF_SEAM_STAMPS
        if (threadIdx.x == 0) stamp[4] = wall_clock64() - t0;
#endif
        return;
    }
    if (part == 0) {
        if (SEAMS && threadIdx.x >= 256) return;            // a launch at the wide lambda_max's 512 threads: part 0 keeps its 256, the
                                                            // other waves leave the kernel at once (a barrier counts live waves only)
        // CTRL_COMMIT_A comes only from gram_sweep, with CTRL_COV_B, in a SEAMS launch: commit_cov_b_dev is the one commit
        EndHandOff ho{reinterpret_cast<double*>(lds), 16 * R, 0.0, 1.0, false};
        const bool end_to_a = SEAMS && (a.mode & CTRL_PREV_END) && (a.mode & CTRL_COV_A);
        const bool commit_to_b = SEAMS && (a.mode & CTRL_COMMIT_A) && (a.mode & CTRL_COV_B);
        if (a.mode & CTRL_PREV_END)
            ctrl_end_dev(a.st, a.lay, a.H, a.Lg, a.M, (a.end_flags & ~8) | 64, a.eps, a.trace, a.ints, a.it_row, ho, end_to_a);
        const unsigned long long t1 = wall_clock64();
        if (end_to_a) {
            if (ho.live) cov_a_after_end_dev<R>(a.st, a.lay, a.H, ho, a.S32, a.ints);
        } else if (a.mode & CTRL_COV_A) {
            ctrl_cov_dev<R, 16>(a.st, a.lay, a.H, 0, a.Lg, a.S32, a.ints, reinterpret_cast<double*>(lds), true);
        }
        if (commit_to_b) commit_cov_b_dev<R>(a.st, a.lay, a.H, a.M, a.S32, a.ints, reinterpret_cast<double*>(lds));
        else if (a.mode & CTRL_COV_B) ctrl_cov_dev<R, 16>(a.st, a.lay, a.H, 1, a.M, a.S32, a.ints, reinterpret_cast<double*>(lds));
        if (threadIdx.x == 0) {
            const unsigned long long t2 = wall_clock64();
            if (a.mode & CTRL_PREV_END) stamp[0] = t1 - t0;
            if (a.mode & CTRL_COV_A) stamp[1] = t2 - t1;
            if (a.mode & CTRL_COV_B) stamp[3] = t2 - t1;
        }
        if (a.sready) {                                     // set unconditionally: a waiting epilogue must never hang
            __threadfence();
            __syncthreads();
            if (threadIdx.x == 0) __hip_atomic_store(a.sready, a.sready_val, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
    } else {
        if (a.mode & CTRL_PREV_END) {
            eig_dev<R, SEAMS>(a.st, a.lay, a.H, a.spectral, 0, a.ints, reinterpret_cast<float*>(lds), S_LAMD);
            ctrl_loop_dev(a.st, a.lay, a.eps, a.trace, a.ints, a.it_row, a.loopw);
            if (threadIdx.x == 0) stamp[2] = wall_clock64() - t0;
        }
        if (a.mode & CTRL_EIG_BOLD)
            eig_dev<R, SEAMS>(a.st, a.lay, a.H, a.spectral, 1, a.ints, reinterpret_cast<float*>(lds), S_LAMB_PREV);
    }
}

// the chain as a launch of its own: workgroups of 256 threads -- 512 where a part runs the wide squaring (eig_dev, WIDE_OK) -- three
// in the sweep's first launch, one in its second; dynamic LDS as for the pass launches' control workgroups
template <int R>
__global__ __launch_bounds__(R == 4 ? 512 : 256) void ctrl_chain_kernel(CtrlArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_chain[];
    ctrl_chain<R, true>(a, lds_chain, blockIdx.x);
}

// ---- vbls! as H x H algebra (examples/mil_util.jl:179-203, vbmf_parameters branch, no label mask) ----------------------------
// With B, SigmaB, CB frozen, P = Y'B is fixed, and so is S = P'P.  One iteration of  updateA!; updateCA!; updateSigma2!  then needs
// no M- or L-sized work at all:
//     K      = B'B + L SigmaB + sigma2 inv(CA)          SigmaA = sigma2 inv(K)                       (src/vbmf.jl:96-97)
//     A'A    = SigmaA S SigmaA / sigma2^2               (A = P SigmaA / sigma2, src/vbmf.jl:98)
//     CA_hh  = (A'A)_hh / M + SigmaA_hh                                                               (src/vbmf.jl:129-134)
//     tr(Y'BA') = tr(S SigmaA) / sigma2
//     sigma2 = (||Y||^2 - 2 tr(Y'BA') + tr((A'A + M SigmaA)(B'B + L SigmaB))) / (L M)                 (src/vbmf.jl:153-157)
// so the whole loop is ONE launch of one workgroup: the inverse by the blocked sweep, the two H x H products on the fp64 MFMA,
// everything LDS-resident, and A itself is formed once at the end from the last inv(K).  The MIL classifier calls vbls! with 150
// iterations on bags of a few tens of columns and H <= 10 (examples/mil_util.jl:473-479): per call 5.6-7.6 ms with one launch
// group per iteration (profiles/r03_f_vbls_mil.txt: break-even with NumPy on the host), most of it launch latency.
// 256 threads; LDS: four 16 NB x (16 NB + 2) fp64 images (W, S, SigmaA, T).  Blocks (I, J) are owned by wave (I NB + J) % 4.
// The loop body is vbls_loop_dev: one workgroup runs one matrix ("bag").  B'B and SigmaB come from the state (GB, SB), everything
// that belongs to the bag through VblsBag -- so the single-matrix launch (vbls_loop_kernel: the bag IS the state) and the batched
// one (vbls_batch_kernel: one workgroup per bag of a context holding many bags side by side) run the same code.
constexpr size_t vbls_lds_bytes(int NB) { return (size_t)4 * (16 * NB) * (16 * NB + 2) * sizeof(double); }
struct VblsBag {
    const double* S; int lds;      // S = P'P, H x H at leading dimension lds
    double trYY, M;                // ||Y||^2 and the column count of the bag
    double* sigma2;                // in: start value; out: after the last updateSigma2!
    double* ca;                    // in / out: diag(CA), H entries
    double* SA; int ldsa, nsa;     // out: SigmaA of the last updateA!, nsa x nsa at leading dimension ldsa (zero beyond H)
    float* SA32;                   // out (optional): SigmaA / sigma2 of that update, fp32 (the post kernel's table), same layout
    double* T;                     // out (optional): the same table in fp64
    double* logdet;                // out (optional): log det SigmaA
};
// K0 = B'B + L SigmaB comes through k0(i, j) (i, j < H): VblsK0State reads the context's state; the jobs form (vbls_basic_jobs_kernels.hpp)
// hands in its model's G.  Returns nonzero -- on wave 0's threads, where the sweep keeps its pivots -- when an inverse met a pivot that
// is not positive and finite: the caller owns the flag (one per call here, one per job there).
struct VblsK0State {
    const double* st; StateLayout lay; double Lg;
    __device__ __forceinline__ double operator()(int i, int j) const {
        return st[lay.GB() + (long long)i * lay.Hp + j] + Lg * st[lay.SB() + (long long)i * lay.Hp + j];
    }
};
template <int NB, class K0>
__device__ __forceinline__ int vbls_loop_dev(const K0& k0at, int H, double Lg, int niter, const VblsBag& g, double* lds_vl) {
    __shared__ double red[16];
    __shared__ double ca_s[16 * NB], dg_s[16 * NB];
    constexpr int NP = 16 * NB, LD = NP + 2, IMG = NP * LD;
    constexpr int NOWN = (NB * NB + 3) / 4;                    // blocks per wave
    double* W = lds_vl;
    double* Sm = lds_vl + IMG;
    double* SAm = lds_vl + 2 * IMG;
    double* Tm = lds_vl + 3 * IMG;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c16 = lane & 15, q16 = lane >> 4;
    const int nbu = (H + 15) >> 4;
    const double M = g.M;
    double sigma2 = *g.sigma2;
    const double trYY = g.trYY;
    const double* Sg = g.S;
    // K0 = B'B + L SigmaB of this wave's blocks (C/D layout), S into LDS, CA into LDS
    f64x4 k0[NOWN];
#pragma unroll
    for (int o = 0; o < NOWN; ++o) {
        const int b = w + 4 * o, I = b / NB, J = b % NB;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = 16 * I + q16 + 4 * r, j = 16 * J + c16;
            k0[o][r] = (b < NB * NB && i < H && j < H) ? k0at(i, j) : 0.0;
        }
    }
    for (int t = threadIdx.x; t < NP * NP; t += 256) {
        const int i = t / NP, j = t % NP;
        Sm[i * LD + j] = (i < H && j < H) ? Sg[(long long)i * g.lds + j] : 0.0;
    }
    if (threadIdx.x < NP) ca_s[threadIdx.x] = threadIdx.x < H ? g.ca[threadIdx.x] : 1.0;
    __syncthreads();
    double ldK = 0.0;
    int bad = 0;
    for (int it = 0; it < niter; ++it) {
        // K into the sweep image (every block: the sweep reads the upper ones)
#pragma unroll
        for (int o = 0; o < NOWN; ++o) {
            const int b = w + 4 * o, I = b / NB, J = b % NB;
            if (b >= NB * NB) continue;
            f64x4 x = k0[o];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = 16 * I + q16 + 4 * r, j = 16 * J + c16;
                if (i == j) x[r] = i < H ? x[r] + sigma2 / ca_s[i] : 1.0;       // + sigma2 inv(CA); identity padding
            }
            blk_st_rows(W, LD, I, J, lane, x);
        }
        __syncthreads();
        PivAcc pv;
        blk_sweep<NB, 4>(W, LD, nbu, w, lane, pv);               // upper blocks of W = -inv(K)
        ldK = pv.logdet();
        bad |= pv.bad;
        // SigmaA = sigma2 inv(K), full symmetric image
        for (int t = threadIdx.x; t < NP * NP; t += 256) {
            const int i = t / NP, j = t % NP;
            SAm[i * LD + j] = (i < H && j < H) ? -sigma2 * (i <= j ? W[i * LD + j] : W[j * LD + i]) : 0.0;
        }
        __syncthreads();
        // T = SigmaA S  (blocks of this wave; SigmaA symmetric: the A operand of block (I, K) is the row read of block (K, I))
#pragma unroll
        for (int o = 0; o < NOWN; ++o) {
            const int b = w + 4 * o, I = b / NB, J = b % NB;
            if (b >= NB * NB) continue;
            f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int K = 0; K < NB; ++K) acc = blk_mma(blk_ld_rows(SAm, LD, K, I, lane), blk_ld_rows(Sm, LD, K, J, lane), acc);
            blk_st_rows(Tm, LD, I, J, lane, acc);
        }
        __syncthreads();
        // A'A = T SigmaA / sigma2^2 and the three reductions, block by block in registers
        const double is4 = 1.0 / (sigma2 * sigma2);
        double t2 = 0.0, trs = 0.0;
#pragma unroll
        for (int o = 0; o < NOWN; ++o) {
            const int b = w + 4 * o, I = b / NB, J = b % NB;
            if (b >= NB * NB) continue;
            f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int K = 0; K < NB; ++K) acc = blk_mma(blk_ld_cols(Tm, LD, I, K, lane), blk_ld_rows(SAm, LD, K, J, lane), acc);
            const f64x4 sa = blk_ld_rows(SAm, LD, I, J, lane), ss = blk_ld_rows(Sm, LD, I, J, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = 16 * I + q16 + 4 * r, j = 16 * J + c16;
                const double ata = acc[r] * is4;
                t2 += (ata + M * sa[r]) * k0[o][r];
                trs += ss[r] * sa[r];
                if (i == j && i < H) dg_s[i] = ata / M + sa[r];             // the new CA_hh
            }
        }
        t2 = block_sum(t2, red);
        trs = block_sum(trs, red);                               // (its barriers publish dg_s)
        const bool last = it + 1 == niter;
        if (last) {                                              // what the last updateA! leaves: SigmaA, inv(K) as the post kernel's table
            for (int t = threadIdx.x; t < g.nsa * g.nsa; t += 256) {
                const int i = t / g.nsa, j = t % g.nsa;
                const double v = (i < H && j < H) ? SAm[i * LD + j] : 0.0;
                g.SA[(long long)i * g.ldsa + j] = v;
                if (g.SA32) g.SA32[(long long)i * g.ldsa + j] = (float)(v / sigma2);
                if (g.T) g.T[(long long)i * g.ldsa + j] = v / sigma2;
            }
            if (threadIdx.x == 0 && g.logdet) *g.logdet = (double)H * log(sigma2) - ldK;
        }
        __syncthreads();
        if (threadIdx.x < NP) ca_s[threadIdx.x] = threadIdx.x < H ? dg_s[threadIdx.x] : 1.0;
        sigma2 = (trYY - 2.0 * trs / sigma2 + t2) / (Lg * M);
        __syncthreads();
    }
    if (threadIdx.x < H) g.ca[threadIdx.x] = ca_s[threadIdx.x];
    if (threadIdx.x == 0) *g.sigma2 = sigma2;
    return bad;
}

// Reads GB, SB, ca, sigma2, ||Y||^2 and S (at st + lay.W1()); writes SA, ca, sigma2, log det SigmaA and the fp32 table inv(K).
template <int NB>
__global__ __launch_bounds__(256) void vbls_loop_kernel(double* __restrict__ st, StateLayout lay, int H, double Lg, double M,
                                                        int niter, float* __restrict__ SA32, int* __restrict__ ints) {
    extern __shared__ __attribute__((aligned(16))) double lds_vl[];
    double* scal = st + lay.scal();
    const VblsBag g{st + lay.W1(), lay.Hp, scal[S_TRYY], M, scal + S_SIGMA2, st + lay.ca(), st + lay.SA(), lay.Hp, lay.Hp, SA32,
                    nullptr, scal + S_LOGDET_SA};
    if (vbls_loop_dev<NB>(VblsK0State{st, lay, Lg}, H, Lg, niter, g, lds_vl)) atomicExch(ints + I_ERR, 1);
}

// vbls! over many bags with one fixed basis (vbmf_run_fixed_basis_batched): workgroup b runs ALL niter iterations of bag b = columns
// col_off[b] .. col_off[b+1]-1 of the context's Y (updateA! does not read the previous A, src/vbmf.jl:96-98, so no iteration has to run
// the general way).  Per bag: S_b (H x H, ld H) and ||Y_b||^2 from bag_gram_kernel; sigma2 / CA start values in, final values out;
// SigmaA_b and the fp64 table SigmaA_b / sigma2_b of the last updateA! out (bag_a_kernel forms A_b = P_b T_b from it).
template <int NB>
__global__ __launch_bounds__(256) void vbls_batch_kernel(const double* __restrict__ st, StateLayout lay, int H, double Lg,
                                                         const long long* __restrict__ col_off, int niter, const double* __restrict__ S,
                                                         const double* __restrict__ yy, double* __restrict__ sigma2,
                                                         double* __restrict__ ca, double* __restrict__ SA, double* __restrict__ T,
                                                         int* __restrict__ ints) {
    extern __shared__ __attribute__((aligned(16))) double lds_vl[];
    const int b = blockIdx.x;
    const long long o2 = (long long)b * H * H;
    const VblsBag g{S + o2, H, yy[b], (double)(col_off[b + 1] - col_off[b]), sigma2 + b, ca + (long long)b * H, SA + o2, H, H,
                    nullptr, T + o2, nullptr};
    if (vbls_loop_dev<NB>(VblsK0State{st, lay, Lg}, H, Lg, niter, g, lds_vl)) atomicExch(ints + I_ERR, 1);
}

// identity (H x H, zero-padded to Hp) as a post kernel's table: A = P I, whose Gram is S = P'P
__global__ void identity_table_kernel(float* __restrict__ S32, int H, int Hp) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < Hp * Hp) S32[t] = ((t / Hp) == (t % Hp) && (t / Hp) < H) ? 1.f : 0.f;
}
__global__ void copy_doubles_kernel(const double* __restrict__ src, double* __restrict__ dst, int n) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) dst[t] = src[t];
}

__global__ void copy_scalar_kernel(double* st, StateLayout lay, int dst, int src) {
    if (threadIdx.x == 0 && blockIdx.x == 0) st[lay.scal() + dst] = st[lay.scal() + src];
}

}  // namespace vbmf
