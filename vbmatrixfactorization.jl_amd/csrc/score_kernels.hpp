// score_kernels.hpp -- what the MIL classifier compares after a batched vbls!: per-bag residuals and the per-bag sums of
// lowerBound / lowerBoundTrimmed (vbmf_bag_residuals, vbmf_sparse_lower_bound_batched; examples/mil_util.jl:469-530).
//
// The context's Y holds the bags side by side: bag b = columns col_off[b] .. col_off[b+1]-1 (batch_kernels.hpp); bags do not align
// with the 32-column tiles, so every access goes through the column index.
//   bag_resid_kernel     r2 partials: sum over a slice of a bag's columns of (Y[l,m] - sum_h B[l,h] A[m,h])^2, formed entry by
//                        entry from Y as stored (the pass-2 tiles bag_gram_kernel reads) in fp64 -- NOT the trace form
//                        ||Y||^2 - 2 tr(B'YA) + tr(A'A B'B): on a fitted bag r2 is 1/400 .. 1/2500 of ||Y_b||^2 and the trace
//                        form would lose that many digits of the fp32 Y'B.  A bag is cut into slices of SCORE_CW columns counted
//                        from ITS OWN first column, one workgroup per slice (chunk_off: the bags' first slice numbers), so a
//                        1-column bag costs one workgroup, a 70-column bag nine, and no bag's result depends on where it sits in Y.
//                        B is the context's BHat as stored (fp32 row-major [Lp][Hp], the values vbmf_get_state returns), widened
//                        to fp64; A is the caller's fp64 AHat.
//   bag_resid_fold_kernel  r2[b] = the bag's slice partials, summed in slice order
//   bag_lb_sums_kernel   one workgroup per bag: the M_b*H-long sums of lowerBound per column h (SCORE_NS values each; lb_column_sums,
//                        the __device__ function vbls_jobs_kernel of vbls_jobs_kernels.hpp calls on its own state) and the two
//                        H x H contractions of its data term
// Least squares against a caller's fp64 basis (vbmf_bag_least_squares; ols / rls of examples/mil_util.jl:159-171 and the
// norm(Y - BHat*AT) of :483-484), H <= 64.  B travels as fp64 row-major [L][H] (reads coalesce over h); nothing of the context's state
// is read:
//   bag_ls_gram_kernel     B'B partials over LS_ROWS rows of B per workgroup, each entry a plain fma chain in row order
//   bag_ls_inverse_kernel  one workgroup: the partials summed in chunk order, + lambda I, inverted by the control chain's blocked
//                          sweep (spd_inverse_lds4); K = inv(B'B + lambda I) to global, both triangles, and the bad-pivot flag
//   bag_ls_kernel          one workgroup per bag slice (the slices of bag_resid_kernel): z = B'y per column with Y staged LS_ROWS rows
//                          at a time in LDS, x = K z, then the slice's sum of (y - B x)^2 entry by entry -- NOT ||y||^2 - z'Kz, which
//                          cancels 400- to 3000-fold on fitted bags.  Every sum has one order fixed by (L, H, the slice's width): a
//                          bag's X and r2 do not depend on where it sits in Y or on the other bags of the call.
// Many bases and a list of (bag, basis) jobs in one call (vbmf_bag_least_squares_jobs; test_classification of every fold of
// examples/mil_util.jl:627-648 at once).  The arithmetic of the three kernels above lives in __device__ functions (ls_gram_chunk,
// ls_inverse, ls_slice) that these call with their own basis, so a job's numbers are the one-basis entry's by construction:
//   bag_ls_gram_jobs_kernel     one workgroup per (basis, chunk of LS_ROWS rows), each with its own H_k
//   bag_ls_inverse_jobs_kernel  one workgroup per basis, its own lambda_k and bad-pivot flag
//   bag_ls_jobs_kernel          one workgroup per (job, slice of SCORE_CW columns of the job's bag, counted from the bag's own first
//                               column), found by score_bag_of on the jobs' first slice numbers; ls_slice on that job's Bt, K, H and
//                               X block.  A job whose basis raised its flag gets NaN in its X block and its partials instead.
//   bag_resid_fold_kernel       r2[j] = the job's slice partials in slice order (the jobs' first slice numbers as chunk_off)
// Data term of the per-bag bound: r2 + L tr(A'A SigmaB) + tr(SigmaA (B'B + L SigmaB)), algebraically the reference's
// ||Y||^2 - 2 tr(B'YA) + tr((A'A + SigmaA)(B'B + L SigmaB)) (src/vbmf_sparse.jl:439-440) with the direct residual of the same
// call in place of its three cancelling terms; so neither tr(B'Y_b A_b) nor ||Y_b||^2 is formed here.
#pragma once
#include "common.hpp"
#include "ctrl_kernels.hpp"

namespace vbmf {

constexpr int SCORE_CW = 8;        // columns of a bag per residual workgroup
constexpr int SCORE_THREADS = 256;
// per column h of a bag: [ sum log beta, sum CA, count', sum' log beta, sum' CA, sum' CA (a^2 + dS), sum' log dS ]; sum' / count'
// run over the entries lowerBoundTrimmed keeps, |(float)a| > trim (trim < 0 keeps everything: lowerBound)
constexpr int SCORE_NS = 7;
// dynamic LDS of bag_resid_kernel: the slice's rows of A
inline size_t score_resid_lds_bytes(int H) { return (size_t)SCORE_CW * H * sizeof(double); }

// vbmf_bag_least_squares
constexpr int LS_MAX_H = 64;
constexpr int LS_ROWS = 256;       // rows of B per Gram workgroup; rows of a slice of Y staged in LDS at a time
// vbmf_bag_least_squares_jobs: the workgroups of SCORE_THREADS one grid is given, so that a launch stays within 2^32 - 1 threads
constexpr long long LS_MAX_GROUPS = ((1ll << 32) - 1) / SCORE_THREADS;
// dynamic LDS of bag_ls_kernel: K | z | x | the staged rows of Y | the row stripes' shares of z
inline size_t score_ls_lds_bytes(int H) {
    const int P = SCORE_CW * H;
    return (size_t)(H * H + 2 * P + SCORE_CW * LS_ROWS + (P > SCORE_THREADS ? P : SCORE_THREADS)) * sizeof(double);
}

// Y[l, m] as stored, from the pass-2 tiles
template <int MODE>
__device__ __forceinline__ float score_y_at(const uint4* __restrict__ Y2, int KSpad, long long l, long long m) {
    constexpr int KSTEP = (MODE == MODE_F32) ? 8 : 16;
    const int xt = (int)(l >> 5), c = (int)(l & 31);
    const int ks = (int)(m / KSTEP), wi = (int)(m % KSTEP);
    int half, e;
    if (MODE == MODE_F32) { half = wi >> 2; e = wi & 3; }
    else { half = (wi >> 2) & 1; e = 4 * (wi >> 3) + (wi & 3); }
    const uint4 f = Y2[((long long)xt * KSpad + ks) * 64 + half * 32 + c];
    const unsigned wd[4] = {f.x, f.y, f.z, f.w};
    if (MODE == MODE_F32) return bitsf(wd[e]);
    return bf2f((unsigned short)((wd[e >> 1] >> (16 * (e & 1))) & 0xFFFFu));
}

// the last bag whose first slice number is <= w
__device__ __forceinline__ int score_bag_of(const long long* __restrict__ chunk_off, int nbags, long long w) {
    int lo = 0, hi = nbags - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (chunk_off[mid] <= w) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// A[m, h] = A[m * sm + h * sh]: (1, ldA) for a column-major AHat, (H, 1) for vec(A')
template <int MODE>
__global__ __launch_bounds__(SCORE_THREADS) void bag_resid_kernel(const uint4* __restrict__ Y2, int KSpad, long long L,
                                                                  const float* __restrict__ B32, int Hp, int H,
                                                                  const double* __restrict__ A, long long sm, long long sh,
                                                                  const long long* __restrict__ col_off,
                                                                  const long long* __restrict__ chunk_off, int nbags,
                                                                  double* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) double Al[];      // [SCORE_CW][H]
    __shared__ double red[SCORE_THREADS / 64];
    const long long w = blockIdx.x;
    const int b = score_bag_of(chunk_off, nbags, w);
    const long long m0 = col_off[b] + (w - chunk_off[b]) * SCORE_CW;
    const long long mend = col_off[b + 1];
    const int nc = (int)(mend - m0 < SCORE_CW ? mend - m0 : SCORE_CW);
    for (int t = threadIdx.x; t < nc * H; t += SCORE_THREADS) {
        const int cc = t / H, h = t % H;
        Al[t] = A[(m0 + cc) * sm + h * sh];
    }
    __syncthreads();
    double acc = 0.0;
    const long long n = (long long)nc * L;
    for (long long t = threadIdx.x; t < n; t += SCORE_THREADS) {
        const long long l = t % L;
        const int cc = (int)(t / L);
        const float v = score_y_at<MODE>(Y2, KSpad, l, m0 + cc);
        const float* brow = B32 + l * Hp;
        const double* arow = Al + cc * H;
        double pred = 0.0;
        for (int h = 0; h < H; ++h) pred += (double)brow[h] * arow[h];
        const double d = (double)v - pred;
        acc += d * d;
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) part[w] = acc;
}

__global__ void bag_resid_fold_kernel(const double* __restrict__ part, const long long* __restrict__ chunk_off, int nbags,
                                      double* __restrict__ r2) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nbags) return;
    double s = 0.0;
    for (long long w = chunk_off[b]; w < chunk_off[b + 1]; ++w) s += part[w];
    r2[b] = s;
}

// The H x H Gram partial of rows l0 .. l1-1 of Bt (B row-major [L][H]) into Gc; entry (i, j) and entry (j, i) are the same products in
// the same order.
__device__ __forceinline__ void ls_gram_chunk(const double* __restrict__ Bt, long long l0, long long l1, int H, double* __restrict__ Gc) {
    for (int e = threadIdx.x; e < H * H; e += SCORE_THREADS) {
        const int i = e / H, j = e % H;
        double s = 0.0;
        for (long long l = l0; l < l1; ++l) s = fma(Bt[l * H + i], Bt[l * H + j], s);
        Gc[e] = s;
    }
}

// Bt: B row-major [L][H].  Gp: [gridDim.x][H * H]
__global__ __launch_bounds__(SCORE_THREADS) void bag_ls_gram_kernel(const double* __restrict__ Bt, long long L, int H,
                                                                    double* __restrict__ Gp) {
    const long long l0 = (long long)blockIdx.x * LS_ROWS;
    const long long l1 = l0 + LS_ROWS < L ? l0 + LS_ROWS : L;
    ls_gram_chunk(Bt, l0, l1, H, Gp + (long long)blockIdx.x * H * H);
}

// The bases of a jobs call: basis k is Bt + b_off[k] (row-major [L][Hs[k]]); its Gram partials are Gp + nchunk * k_off[k]
// ([nchunk][H_k^2]), its inverse K + k_off[k]: k_off[k] = the sum of H_q^2 over q < k.
struct LsBases {
    const long long* Hs;
    const long long* b_off;
    const long long* k_off;
    const double* lambda;
    const double* Bt;
};

// workgroup (k, q) = blockIdx.x: chunk q of basis k
__global__ __launch_bounds__(SCORE_THREADS) void bag_ls_gram_jobs_kernel(LsBases bs, long long L, int nchunk, double* __restrict__ Gp) {
    const int k = blockIdx.x / nchunk, q = blockIdx.x % nchunk;
    const int H = (int)bs.Hs[k];
    const long long l0 = (long long)q * LS_ROWS;
    const long long l1 = l0 + LS_ROWS < L ? l0 + LS_ROWS : L;
    ls_gram_chunk(bs.Bt + bs.b_off[k], l0, l1, H, Gp + (long long)nchunk * bs.k_off[k] + (long long)q * H * H);
}

// K[H][H] = inv(sum of the nchunk Gram partials + lambda I); *bad != 0: a pivot was not positive / finite.  Wl: spd_inverse_lds_bytes(4)
// of LDS; the whole workgroup of 256 calls it.
__device__ __forceinline__ void ls_inverse(double* Wl, const double* __restrict__ Gp, int nchunk, int H, double lambda,
                                           double* __restrict__ K, int* __restrict__ bad) {
    double logdet;
    int notpd;
    spd_inverse_lds4<LS_MAX_H / 16>(Wl, H, [&](int i, int j) {
        double s = 0.0;
        for (int q = 0; q < nchunk; ++q) s += Gp[((long long)q * H + i) * H + j];
        return i == j ? s + lambda : s;
    }, &logdet, &notpd);
    __syncthreads();
    for (int t = threadIdx.x; t < H * H; t += 256) K[t] = spd_inv_at<LS_MAX_H / 16>(Wl, t / H, t % H);
    if (threadIdx.x == 0) *bad = notpd;
}

__global__ __launch_bounds__(256) void bag_ls_inverse_kernel(const double* __restrict__ Gp, int nchunk, int H, double lambda,
                                                             double* __restrict__ K, int* __restrict__ bad) {
    extern __shared__ __attribute__((aligned(16))) double Wl[];
    ls_inverse(Wl, Gp, nchunk, H, lambda, K, bad);
}

// one workgroup per basis; bad: one int per basis, 8 bytes apart (the slots of the call's read-back block)
__global__ __launch_bounds__(256) void bag_ls_inverse_jobs_kernel(LsBases bs, const double* __restrict__ Gp, int nchunk,
                                                                  double* __restrict__ K, int* __restrict__ bad) {
    extern __shared__ __attribute__((aligned(16))) double Wl[];
    const int k = blockIdx.x;
    ls_inverse(Wl, Gp + (long long)nchunk * bs.k_off[k], nchunk, (int)bs.Hs[k], bs.lambda[k], K + bs.k_off[k], bad + 2 * k);
}

// One slice of a bag against one basis: columns m0 .. m0 + nc - 1 of Y (nc <= SCORE_CW), Bt row-major [L][H], K = inv(B'B + lambda I).
// Xs: the slice's columns of the estimate (column cc at Xs + cc * H) or nullptr; part_w: the slice's residual partial or nullptr.
// ls: score_ls_lds_bytes(H) of LDS; red: SCORE_THREADS / 64 doubles.
// Output o = (column cc, component h) = cc * H + h of the slice's P = nc * H.  z: with P <= 256 the threads split into S = 256 / P row
// stripes (rows s, s + S, ... of every staged tile, tiles in order), whose shares meet in LDS in stripe order; above, every thread
// owns outputs o and o + 256 whole.
template <int MODE>
__device__ __forceinline__ void ls_slice(const uint4* __restrict__ Y2, int KSpad, long long L, const double* __restrict__ Bt, int H,
                                         const double* __restrict__ K, long long m0, int nc, double* __restrict__ Xs,
                                         double* __restrict__ part_w, double* ls, double* red) {
    double* Kl = ls;                                   // [H][H]
    double* zl = Kl + H * H;                           // [SCORE_CW][H]
    double* xl = zl + SCORE_CW * H;                    // [SCORE_CW][H]
    double* yt = xl + SCORE_CW * H;                    // [SCORE_CW][LS_ROWS]
    double* zp = yt + SCORE_CW * LS_ROWS;              // [S][P]
    const int P = nc * H;
    const int S = P > SCORE_THREADS ? 1 : SCORE_THREADS / P;
    const int tid = threadIdx.x;
    for (int t = tid; t < H * H; t += SCORE_THREADS) Kl[t] = K[t];
    // this thread's (at most two) outputs and its row stripe
    int o[2] = {-1, -1};
    int s = 0;
    if (S == 1) { o[0] = tid < P ? tid : -1; o[1] = tid + SCORE_THREADS < P ? tid + SCORE_THREADS : -1; }
    else if (tid < P * S) { o[0] = tid % P; s = tid / P; }
    double acc[2] = {0.0, 0.0};
    for (long long l0 = 0; l0 < L; l0 += LS_ROWS) {
        const int rows = (int)(L - l0 < LS_ROWS ? L - l0 : LS_ROWS);
        for (int t = tid; t < nc * rows; t += SCORE_THREADS) {
            const int cc = t / rows, r = t % rows;
            yt[cc * LS_ROWS + r] = (double)score_y_at<MODE>(Y2, KSpad, l0 + r, m0 + cc);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (o[k] < 0) continue;
            const int cc = o[k] / H, h = o[k] % H;
            const double* bcol = Bt + l0 * H + h;
            const double* ycol = yt + cc * LS_ROWS;
            double a = acc[k];
            for (int r = s; r < rows; r += S) a = fma(bcol[(long long)r * H], ycol[r], a);
            acc[k] = a;
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 2; ++k)
        if (o[k] >= 0) zp[s * P + o[k]] = acc[k];
    __syncthreads();
    for (int q = tid; q < P; q += SCORE_THREADS) {
        double z = 0.0;
        for (int i = 0; i < S; ++i) z += zp[i * P + q];
        zl[q] = z;
    }
    __syncthreads();
    for (int q = tid; q < P; q += SCORE_THREADS) {
        const int cc = q / H, h = q % H;
        const double* zc = zl + cc * H;
        double x = 0.0;
        for (int j = 0; j < H; ++j) x = fma(Kl[j * H + h], zc[j], x);      // (K is symmetric bit for bit: one triangle, mirrored)
        xl[q] = x;
        if (Xs != nullptr) Xs[cc * H + h] = x;
    }
    if (part_w == nullptr) return;
    __syncthreads();
    double r2 = 0.0;
    const long long n = (long long)nc * L;
    for (long long t = tid; t < n; t += SCORE_THREADS) {
        const long long l = t % L;
        const int cc = (int)(t / L);
        const double* brow = Bt + l * H;
        const double* xc = xl + cc * H;
        double pred = 0.0;
        for (int h = 0; h < H; ++h) pred += brow[h] * xc[h];
        const double d = (double)score_y_at<MODE>(Y2, KSpad, l, m0 + cc) - pred;
        r2 += d * d;
    }
    r2 = block_sum(r2, red);
    if (tid == 0) *part_w = r2;
}

// X: [M][H] (column m of the H x M estimate at X + m * H) or nullptr; part: the slices' residual partials or nullptr.
template <int MODE>
__global__ __launch_bounds__(SCORE_THREADS) void bag_ls_kernel(const uint4* __restrict__ Y2, int KSpad, long long L,
                                                               const double* __restrict__ Bt, int H, const double* __restrict__ K,
                                                               const long long* __restrict__ col_off,
                                                               const long long* __restrict__ chunk_off, int nbags,
                                                               double* __restrict__ X, double* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) double ls[];
    __shared__ double red[SCORE_THREADS / 64];
    const long long w = blockIdx.x;
    const int b = score_bag_of(chunk_off, nbags, w);
    const long long m0 = col_off[b] + (w - chunk_off[b]) * SCORE_CW;
    const long long mend = col_off[b + 1];
    const int nc = (int)(mend - m0 < SCORE_CW ? mend - m0 : SCORE_CW);
    ls_slice<MODE>(Y2, KSpad, L, Bt, H, K, m0, nc, X ? X + m0 * H : nullptr, part ? part + w : nullptr, ls, red);
}

// The jobs of a call: job j scores bag job_bag[j] against basis job_basis[j]; its slices are numbers sl0[j] .. sl0[j+1]-1 and its
// H_k x M_b block of X starts at x_off[j] (column-major, ld = H_k).
struct LsJobs {
    const long long* sl0;
    const long long* bag;
    const long long* basis;
    const long long* x_off;
    int njobs;
};

// One workgroup per job slice.  bad: the bases' flags as bag_ls_inverse_jobs_kernel left them; X, part: nullptr = not wanted.
// Dynamic LDS: score_ls_lds_bytes(the largest H of the call).
template <int MODE>
__global__ __launch_bounds__(SCORE_THREADS) void bag_ls_jobs_kernel(const uint4* __restrict__ Y2, int KSpad, long long L, LsBases bs,
                                                                    const double* __restrict__ K, const int* __restrict__ bad,
                                                                    const long long* __restrict__ col_off, LsJobs jobs,
                                                                    double* __restrict__ X, double* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) double ls[];
    __shared__ double red[SCORE_THREADS / 64];
    const long long w = blockIdx.x;
    const int j = score_bag_of(jobs.sl0, jobs.njobs, w);
    const long long c0 = (w - jobs.sl0[j]) * SCORE_CW;            // the slice's first column within the bag
    const int b = (int)jobs.bag[j], k = (int)jobs.basis[j];
    const long long m0 = col_off[b] + c0;
    const long long mend = col_off[b + 1];
    const int nc = (int)(mend - m0 < SCORE_CW ? mend - m0 : SCORE_CW);
    const int H = (int)bs.Hs[k];
    double* Xs = X ? X + jobs.x_off[j] + c0 * H : nullptr;
    if (bad[2 * k]) {                                             // (the same for the whole workgroup)
        const double nan = __longlong_as_double(0x7FF8000000000000ll);
        if (Xs != nullptr)
            for (int t = threadIdx.x; t < nc * H; t += SCORE_THREADS) Xs[t] = nan;
        if (part != nullptr && threadIdx.x == 0) part[w] = nan;
        return;
    }
    ls_slice<MODE>(Y2, KSpad, L, bs.Bt + bs.b_off[k], H, K + bs.k_off[k], m0, nc, Xs, part ? part + w : nullptr, ls, red);
}

// The per-column sums of one bag (SCORE_NS per column h into out[h * SCORE_NS ..]), by the whole workgroup of SCORE_THREADS.  a, dS, CA,
// beta: the bag's own M_b H-long blocks in vec(A') order (LDS or global).  sh: SCORE_THREADS * SCORE_NS doubles of LDS.
// Thread (h, s) of the first (SCORE_THREADS / H) * H takes the bag's columns m = s, s + S, ... of vec column h; the S shares meet in
// LDS in slice order, so a bag's sums depend on its own entries only.  F32CMP: the mask compares the fp32 rounding of a
// (vbmf_sparse_lower_bound_batched, like the whole-context entry) or a itself (src/vbmf_sparse.jl:481; vbmf_sparse_scored_jobs).
template <bool F32CMP>
__device__ __forceinline__ void lb_column_sums(const double* a, const double* dS, const double* CA, const double* beta, int H, int Mb,
                                               double trim, double* sh, double* __restrict__ out) {
    const int Hc = H < SCORE_THREADS ? H : SCORE_THREADS;             // columns per round (H > 256: several rounds)
    const int S = SCORE_THREADS / Hc;
    for (int h0 = 0; h0 < H; h0 += Hc) {
        const int hh = threadIdx.x % Hc, s = threadIdx.x / Hc, h = h0 + hh;
        double v[SCORE_NS] = {0, 0, 0, 0, 0, 0, 0};
        if (s < S && h < H) {
            for (int m = s; m < Mb; m += S) {
                const long long i = (long long)m * H + h;
                const double av = a[i], ds = dS[i], ca = CA[i], lb = log(beta[i]);
                v[0] += lb; v[1] += ca;
                if (trim < 0.0 || fabs(F32CMP ? (double)(float)av : av) > trim) {
                    v[2] += 1.0; v[3] += lb; v[4] += ca; v[5] += ca * (av * av + ds); v[6] += log(ds);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < SCORE_NS; ++k) sh[threadIdx.x * SCORE_NS + k] = v[k];
        __syncthreads();
        if (s == 0 && h < H) {
#pragma unroll
            for (int k = 0; k < SCORE_NS; ++k) {
                double t = 0.0;
                for (int q = 0; q < S; ++q) t += sh[(q * Hc + hh) * SCORE_NS + k];
                out[(long long)h * SCORE_NS + k] = t;
            }
        }
        __syncthreads();
    }
}

// a, dS, CA, beta: M*H in vec(A') order (index m*H + h); SA: nbags x H x H.  sums: [nbags][H][SCORE_NS] (lb_column_sums);
// quad: [nbags][2] = { sum_m a_m' SigmaB a_m = tr(A_b'A_b SigmaB),  tr(SigmaA_b (B'B + L SigmaB)) }.
__global__ __launch_bounds__(SCORE_THREADS) void bag_lb_sums_kernel(const double* __restrict__ a, const double* __restrict__ dS,
                                                                    const double* __restrict__ CA, const double* __restrict__ beta,
                                                                    const double* __restrict__ SA, const double* __restrict__ st,
                                                                    StateLayout lay, int H, double Lg,
                                                                    const long long* __restrict__ col_off, double trim,
                                                                    double* __restrict__ sums, double* __restrict__ quad) {
    __shared__ double sh[SCORE_THREADS * SCORE_NS];
    __shared__ double red[SCORE_THREADS / 64];
    const int b = blockIdx.x;
    const long long m0 = col_off[b];
    const int Mb = (int)(col_off[b + 1] - m0);
    lb_column_sums<true>(a + m0 * H, dS + m0 * H, CA + m0 * H, beta + m0 * H, H, Mb, trim, sh, sums + (long long)b * H * SCORE_NS);
    const double* SB = st + lay.SB();
    const double* GB = st + lay.GB();
    double qa = 0.0;
    for (long long t = threadIdx.x; t < (long long)Mb * H; t += SCORE_THREADS) {
        const int m = (int)(t / H), i = (int)(t % H);
        const double* am = a + (m0 + m) * H;
        double r = 0.0;
        for (int j = 0; j < H; ++j) r += SB[(long long)i * lay.Hp + j] * am[j];
        qa += am[i] * r;
    }
    qa = block_sum(qa, red);
    double ts = 0.0;
    const double* SAb = SA + (long long)b * H * H;
    for (int t = threadIdx.x; t < H * H; t += SCORE_THREADS) {
        const long long e = (long long)(t / H) * lay.Hp + (t % H);
        ts += SAb[t] * (GB[e] + Lg * SB[e]);
    }
    __syncthreads();
    ts = block_sum(ts, red);
    if (threadIdx.x == 0) { quad[2 * b] = qa; quad[2 * b + 1] = ts; }
}

}  // namespace vbmf
