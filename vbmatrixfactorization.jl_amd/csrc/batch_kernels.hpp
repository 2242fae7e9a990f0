// batch_kernels.hpp -- the per-bag kernels of vbls! over many bags (vbmf_run_fixed_basis_batched).
//
// The context's Y holds the bags side by side: bag b = columns col_off[b] .. col_off[b+1]-1.  One pass 1 with the frozen B forms
// P = Y'B for all of them; then
//   bag_gram_kernel   S_b = P_b'P_b (fp64 accumulate; S = nullptr: not formed) and ||Y_b||^2 of Y as stored, one workgroup per bag
//   vbls_batch_kernel the niter iterations, one workgroup per bag (ctrl_kernels.hpp)
//   bag_a_kernel      A_b = P_b T_b with T_b = SigmaA_b / sigma2_b of the bag's last updateA!, row by row (fp64 out)
// Bags do not align with the 32-column tiles of P or Y: every access goes through the column index.
#pragma once
#include "common.hpp"
#include "ctrl_kernels.hpp"
#include "post_kernels.hpp"

namespace vbmf {

// element (h, x) of the pass-1 product: fragment-major (frag_nh = Hp / 32) or row-major [h][x] at leading dimension ldP
__device__ __forceinline__ long long p_index(int h, long long x, long long ldP, int frag_nh) {
    return frag_nh > 0 ? frag_index(h, x, frag_nh) : (long long)h * ldP + x;
}

// H <= 64.  256 threads: thread t owns entries t, t + 256, ... of the row-major H x H image; the bag's P rows pass through LDS in
// chunks of 32 columns.  Each S entry is a sum over the bag's columns in column order (fp32 products are exact in fp64), and each
// thread's share of ||Y_b||^2 runs over the bag's own (l, m) indices: the results do not depend on where the bag sits in Y.
template <int MODE>
__global__ __launch_bounds__(256) void bag_gram_kernel(const float* __restrict__ P, long long ldP, int frag_nh,
                                                       const uint4* __restrict__ Y2, int KSpad, long long L,
                                                       const long long* __restrict__ col_off, int H, double* __restrict__ S,
                                                       double* __restrict__ yy) {
    constexpr int KSTEP = (MODE == MODE_F32) ? 8 : 16;
    constexpr int CH = 32, EPT = 64 * 64 / 256;
    __shared__ float Pl[CH][65];
    __shared__ double red[16];
    const int b = blockIdx.x;
    const long long m0 = col_off[b], m1 = col_off[b + 1];
    const int nent = H * H;
    double acc[EPT];
#pragma unroll
    for (int k = 0; k < EPT; ++k) acc[k] = 0.0;
    for (long long c0 = m0; S != nullptr && c0 < m1; c0 += CH) {         // (S = nullptr: ||Y_b||^2 only)
        const int nc = (int)(m1 - c0 < CH ? m1 - c0 : CH);
        for (int t = threadIdx.x; t < nc * H; t += 256) {
            const int h = t / nc, cc = t % nc;
            Pl[cc][h] = P[p_index(h, c0 + cc, ldP, frag_nh)];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < EPT; ++k) {
            const int t = threadIdx.x + 256 * k;
            if (t < nent) {
                const int i = t / H, j = t % H;
                for (int cc = 0; cc < nc; ++cc) acc[k] += (double)Pl[cc][i] * (double)Pl[cc][j];
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
        const int t = threadIdx.x + 256 * k;
        if (S != nullptr && t < nent) S[(long long)b * nent + t] = acc[k];
    }
    // ||Y_b||^2 from the pass-2 tiles (the layout untile_y_kernel reads), the quantity vbmf_get_trYY reports for a whole matrix
    double ys = 0.0;
    const long long n = (m1 - m0) * L;
    for (long long t = threadIdx.x; t < n; t += 256) {
        const long long l = t % L, m = m0 + t / L;
        const int xt = (int)(l >> 5), c = (int)(l & 31);
        const int ks = (int)(m / KSTEP), w = (int)(m % KSTEP);
        int half, e;
        if (MODE == MODE_F32) { half = w >> 2; e = w & 3; }
        else { half = (w >> 2) & 1; e = 4 * (w >> 3) + (w & 3); }
        const uint4 f = Y2[((long long)xt * KSpad + ks) * 64 + half * 32 + c];
        const unsigned wd[4] = {f.x, f.y, f.z, f.w};
        float v;
        if (MODE == MODE_F32) v = bitsf(wd[e]);
        else v = bf2f((unsigned short)((wd[e >> 1] >> (16 * (e & 1))) & 0xFFFFu));
        ys += (double)v * (double)v;
    }
    ys = block_sum(ys, red);
    if (threadIdx.x == 0) yy[b] = ys;
}

// A (M x H, column-major, fp64): A[m, h] = sum_k P[k, m] T_b[k, h], b the bag of column m (T_b row-major H x H)
__global__ __launch_bounds__(256) void bag_a_kernel(const float* __restrict__ P, long long ldP, int frag_nh,
                                                    const long long* __restrict__ col_off, int nbags, int H,
                                                    const double* __restrict__ T, long long M, double* __restrict__ A) {
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < M * H; t += (long long)gridDim.x * blockDim.x) {
        const long long m = t % M;
        const int h = (int)(t / M);
        int lo = 0, hi = nbags - 1;                          // the last bag with col_off[b] <= m
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (col_off[mid] <= m) lo = mid; else hi = mid - 1;
        }
        const double* Tb = T + (long long)lo * H * H;
        double a = 0.0;
        for (int k = 0; k < H; ++k) a += (double)P[p_index(k, m, ldP, frag_nh)] * Tb[k * H + h];
        A[t] = a;
    }
}

}  // namespace vbmf
