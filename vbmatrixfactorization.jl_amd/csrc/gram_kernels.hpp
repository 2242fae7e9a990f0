// gram_kernels.hpp -- the Gram-form sweep of vbmf_run for tall matrices.
//
// updateB! is B = Y A SigmaB / sigma2 with no mask on B, so after any sweep B = Y W with W = A SigmaB / sigma2 (M x H).  Every
// quantity a sweep takes from Y then comes from the M x M Gram matrix G = Y'Y, built once per Y:
//     Y'B = G W (= P, from which updateA! builds A),   B'B = W'(G W),   tr(B'YA) = sum A o (G W),   dB'dB = D'(G D), D = W_new - W_old.
//
//   gram_build_kernel      G = Y'Y from the pass-1 tiles of Y (bf16 products are exact in fp32; fp32 over chunks of GRAM_CHUNK
//                          k-steps, the chunks summed in fp64, rounded once); upper 128 x 128 blocks, each stored with its mirror
//   gram_w_kernel          W_new = A (SigmaB / sigma2), D = W_new - W_old; fp32 W and the product's bf16 operand planes
//   gram_prod_kernel       [P | Q] = G [W | D] as split-K slabs in the fragment-major layout of the pass-1 product
//   gram_part_kernel       per-chunk fp64 shares of W'P, D'Q and sum A o P
//   gram_part_reduce_kernel  fixed-order sum of the shares -> the state's [B'B | dB'dB | tr(B'YA)] (symmetrised)
//
// Layouts.  G is stored as MFMA operand fragments, fp32: Gt[row tile p][k-step j][lane][8], lane (half, c) holds
// G[32p + c][16j + 8 half + e], e = 0..7 (GT row tiles, KT = 2 GT k-steps; rows / columns >= M are zero).  Because G is symmetric this
// fragment is also the B operand "k = 16j + 8 half + e, column 32p + c", so mfma(W^T fragment, G fragment) yields the TRANSPOSED product
// tile (row h, column m): exactly the accumulator of the streaming pass 1, and it is written fragment-major like that pass
// (post_kernels.hpp, frag_index).  The operand planes Wt[plane][j][h tile][lane] (16 bytes: 8 bf16) hold X[16j + 8 half + e][32 ht + c]:
// planes 0..2 the three bf16 parts of W, planes 3..4 the two parts of D.
//
// Precision: P takes the SIX-term product of three-part G and three-part W (part indices i + j <= 2: exact to an fp32 rounding, the
// form of load_sigma_table); Q = G D the three-term product (its only consumer is the delta-Gram of the stop test).
#pragma once
#include "common.hpp"
#include "ctrl_kernels.hpp"
#include "post_kernels.hpp"

namespace vbmf {

#ifndef GRAM_CHUNK
#define GRAM_CHUNK 256                 // k-steps (16 rows each) accumulated in fp32 before the fp64 fold: 4096 rows
#endif
constexpr int GRAM_PLANES = 5;         // W: 3 bf16 parts, D: 2 bf16 parts

__device__ __forceinline__ unsigned pack_bf2(unsigned short lo, unsigned short hi) { return (unsigned)lo | ((unsigned)hi << 16); }

// G = Y'Y.  Grid (NB, NB), NB = GT / 4: workgroup (Q, P) with P <= Q forms the 128 x 128 block (P, Q), wave (wr, wc) its 64 x 64
// quarter (2 x 2 tiles).  Tiles at or beyond XT (Y's x tiles) are zero.  Only tiles p <= q are stored, each with its mirror, so
// G is exactly symmetric as stored.
__global__ __launch_bounds__(256) void gram_build_kernel(const uint4* __restrict__ Y1, int XT, int KS, float* __restrict__ Gt,
                                                         int GT) {
    const int P = blockIdx.y, Q = blockIdx.x;
    if (P > Q) return;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int p0 = 4 * P + 2 * (w >> 1), q0 = 4 * Q + 2 * (w & 1);
    const long long KT = 2LL * GT;
    double g64[2][2][16];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) g64[a][b][r] = 0.0;
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    const uint4* pa[2];
    const uint4* pb[2];
    bool oka[2], okb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        oka[i] = p0 + i < XT; okb[i] = q0 + i < XT;
        pa[i] = Y1 + ((long long)(oka[i] ? p0 + i : 0) * KS) * 64 + lane;
        pb[i] = Y1 + ((long long)(okb[i] ? q0 + i : 0) * KS) * 64 + lane;
    }
    constexpr int U = 4;                                    // k-steps whose fragments are requested together
    for (int k0 = 0; k0 < KS; k0 += GRAM_CHUNK) {
        const int k1 = min(k0 + GRAM_CHUNK, KS);
        f32x16 acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
        for (int ks = k0; ks < k1; ks += U) {
            uint4 fa[U][2], fb[U][2];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool in = ks + u < k1;
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    fa[u][i] = (in && oka[i]) ? pa[i][(long long)(ks + u) * 64] : z;
                    fb[u][i] = (in && okb[i]) ? pb[i][(long long)(ks + u) * 64] : z;
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b)
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[u][a]),
                                                                            __builtin_bit_cast(bf16x8, fb[u][b]), acc[a][b], 0, 0, 0);
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) g64[a][b][r] += (double)acc[a][b][r];
    }
    // accumulator (a, b): lane (half, c), register r = G[32 p + rho(r, half)][32 q + c]
    const int half = lane >> 5, c = lane & 31;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int p = p0 + a, q = q0 + b;
            if (p > q) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = rho(r, half);
                const float v = (float)g64[a][b][r];
                // G[32p + i][32q + c]: row tile p, k-step 2q + (c >> 4), lane 32 ((c >> 3) & 1) + i, element c & 7
                Gt[(((long long)p * KT + 2 * q + (c >> 4)) * 64 + 32 * ((c >> 3) & 1) + i) * 8 + (c & 7)] = v;
                // the mirror G[32q + c][32p + i]
                if (p != q) Gt[(((long long)q * KT + 2 * p + (i >> 4)) * 64 + 32 * ((i >> 3) & 1) + c) * 8 + (i & 7)] = v;
            }
        }
}

// W_new = A S (S = SigmaB / sigma2, Hp x Hp fp32, zero outside H x H), D = W_new - W_old.  Workgroup j: the 16 rows of k-step j
// (A rows through LDS); thread (h tile ht, lane) the eight rows m = 16 j + 8 half + e of column h = 32 ht + c.  Rows >= M are zero.
__global__ __launch_bounds__(256) void gram_w_kernel(const float* __restrict__ A32, const float* __restrict__ S,
                                                     const float* __restrict__ Wold, float* __restrict__ Wnew,
                                                     uint4* __restrict__ Wt, long long M, int Hp, int KT, const int* __restrict__ stop) {
    if (*stop) return;
    __shared__ float sA[16][128];
    const long long j = blockIdx.x;
    for (int t = threadIdx.x; t < 16 * Hp; t += blockDim.x) {
        const int r = t / Hp, i = t % Hp;
        const long long m = 16 * j + r;
        sA[r][i] = m < M ? A32[m * Hp + i] : 0.f;
    }
    __syncthreads();
    const int NH = Hp / 32;
    if ((int)threadIdx.x >= NH * 64) return;
    const int lane = threadIdx.x & 63, ht = threadIdx.x >> 6;
    const int half = lane >> 5, h = 32 * ht + (lane & 31);
    double acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.0;
    for (int i = 0; i < Hp; ++i) {
        const double sv = (double)S[(long long)i * Hp + h];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += (double)sA[8 * half + e][i] * sv;
    }
    unsigned short wp[3][8], dp[2][8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const long long m = 16 * j + 8 * half + e;
        const float wv = (float)acc[e];
        const float dv = (float)((double)wv - (double)Wold[m * Hp + h]);
        Wnew[m * Hp + h] = wv;
        wp[0][e] = f2bf(wv);
        float res = wv - bf2f(wp[0][e]);
        wp[1][e] = f2bf(res);
        res -= bf2f(wp[1][e]);
        wp[2][e] = f2bf(res);
        dp[0][e] = f2bf(dv);
        dp[1][e] = f2bf(dv - bf2f(dp[0][e]));
    }
    const long long plane = (long long)KT * NH * 64;
    const long long o = (j * NH + ht) * 64 + lane;
#pragma unroll
    for (int q = 0; q < 3; ++q)
        Wt[q * plane + o] = make_uint4(pack_bf2(wp[q][0], wp[q][1]), pack_bf2(wp[q][2], wp[q][3]), pack_bf2(wp[q][4], wp[q][5]),
                                       pack_bf2(wp[q][6], wp[q][7]));
#pragma unroll
    for (int q = 0; q < 2; ++q)
        Wt[(3 + q) * plane + o] = make_uint4(pack_bf2(dp[q][0], dp[q][1]), pack_bf2(dp[q][2], dp[q][3]), pack_bf2(dp[q][4], dp[q][5]),
                                             pack_bf2(dp[q][6], dp[q][7]));
}

// three bf16 parts of 8 fp32 values as MFMA operand fragments
__device__ __forceinline__ void split3_frag(const float4& x0, const float4& x1, uint4& g0, uint4& g1, uint4& g2) {
    const float v[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
    unsigned short p[3][8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        p[0][e] = f2bf(v[e]);
        float r = v[e] - bf2f(p[0][e]);
        p[1][e] = f2bf(r);
        r -= bf2f(p[1][e]);
        p[2][e] = f2bf(r);
    }
    g0 = make_uint4(pack_bf2(p[0][0], p[0][1]), pack_bf2(p[0][2], p[0][3]), pack_bf2(p[0][4], p[0][5]), pack_bf2(p[0][6], p[0][7]));
    g1 = make_uint4(pack_bf2(p[1][0], p[1][1]), pack_bf2(p[1][2], p[1][3]), pack_bf2(p[1][4], p[1][5]), pack_bf2(p[1][6], p[1][7]));
    g2 = make_uint4(pack_bf2(p[2][0], p[2][1]), pack_bf2(p[2][2], p[2][3]), pack_bf2(p[2][4], p[2][5]), pack_bf2(p[2][6], p[2][7]));
}

__device__ __forceinline__ f32x16 mfma_bf(const uint4& a, const uint4& b, const f32x16& c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// [P | Q] = G [W | D], split-K.  Workgroup b: row group b % nrg (4 waves x NXW row tiles), k-steps [s sps, (s + 1) sps) of split
// s = b / nrg.  Out: slab s at Out + s * slab_floats, P fragment-major (tiles x < XT1) followed by Q at Out + s * slab_floats + n.
// Each wave loads its G fragments one k-step ahead and reads the W / D planes (5 NH fragments per k-step, small and shared by every
// workgroup) from L2.  Measured alternatives at 100k x 10k, H = 64 (this kernel: 0.157-0.162 ms): the planes shared through LDS (one
// load per workgroup, a barrier per k-step) 0.26 ms; a three-deep G ring plus the planes one k-step ahead 0.178 ms; twice the split-K
// workgroups (two waves per SIMD) 0.157 ms.
template <int NH, int NXW>
__global__ __launch_bounds__(256) void gram_prod_kernel(const float4* __restrict__ Gt, const uint4* __restrict__ Wt,
                                                        float* __restrict__ Out, int GT, int XT1, int sps, int nrg, long long n,
                                                        long long slab_floats, const int* __restrict__ stop) {
    if (*stop) return;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int rg = blockIdx.x % nrg, s = blockIdx.x / nrg;
    const int KT = 2 * GT;
    const int j0 = s * sps, j1 = min(j0 + sps, KT);
    const int pt0 = (rg * 4 + w) * NXW;
    const long long plane = (long long)KT * NH * 64;
    f32x16 accP[NXW][NH], accQ[NXW][NH];
#pragma unroll
    for (int i = 0; i < NXW; ++i)
#pragma unroll
        for (int h = 0; h < NH; ++h)
#pragma unroll
            for (int r = 0; r < 16; ++r) { accP[i][h][r] = 0.f; accQ[i][h][r] = 0.f; }
    const float4* gp[NXW];
#pragma unroll
    for (int i = 0; i < NXW; ++i) gp[i] = Gt + (((long long)(pt0 + i) * KT) * 64 + lane) * 2;
    float4 gn[NXW][2];
#pragma unroll
    for (int i = 0; i < NXW; ++i) { gn[i][0] = gp[i][(long long)j0 * 128]; gn[i][1] = gp[i][(long long)j0 * 128 + 1]; }
    for (int j = j0; j < j1; ++j) {
        float4 gc[NXW][2];
#pragma unroll
        for (int i = 0; i < NXW; ++i) { gc[i][0] = gn[i][0]; gc[i][1] = gn[i][1]; }
        if (j + 1 < j1) {
#pragma unroll
            for (int i = 0; i < NXW; ++i) { gn[i][0] = gp[i][(long long)(j + 1) * 128]; gn[i][1] = gp[i][(long long)(j + 1) * 128 + 1]; }
        }
        uint4 wf[GRAM_PLANES][NH];
#pragma unroll
        for (int q = 0; q < GRAM_PLANES; ++q)
#pragma unroll
            for (int h = 0; h < NH; ++h) wf[q][h] = Wt[q * plane + ((long long)j * NH + h) * 64 + lane];
#pragma unroll
        for (int i = 0; i < NXW; ++i) {
            uint4 g0, g1, g2;
            split3_frag(gc[i][0], gc[i][1], g0, g1, g2);
#pragma unroll
            for (int h = 0; h < NH; ++h) {
                // smallest terms first: W2 G0, W1 G1, W0 G2, W1 G0, W0 G1, W0 G0
                f32x16 a = accP[i][h];
                a = mfma_bf(wf[2][h], g0, a);
                a = mfma_bf(wf[1][h], g1, a);
                a = mfma_bf(wf[0][h], g2, a);
                a = mfma_bf(wf[1][h], g0, a);
                a = mfma_bf(wf[0][h], g1, a);
                accP[i][h] = mfma_bf(wf[0][h], g0, a);
                f32x16 d = accQ[i][h];
                d = mfma_bf(wf[4][h], g0, d);
                d = mfma_bf(wf[3][h], g1, d);
                accQ[i][h] = mfma_bf(wf[3][h], g0, d);
            }
        }
    }
    float4* oP = reinterpret_cast<float4*>(Out + (long long)s * slab_floats);
    float4* oQ = reinterpret_cast<float4*>(Out + (long long)s * slab_floats + n);
#pragma unroll
    for (int i = 0; i < NXW; ++i) {
        const int p = pt0 + i;
        if (p >= XT1) continue;
#pragma unroll
        for (int h = 0; h < NH; ++h) {
            const long long o = (((long long)p * NH + h) * 64 + lane) * 4;
            const f32x16 a = accP[i][h], d = accQ[i][h];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                oP[o + q] = float4{a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]};
                oQ[o + q] = float4{d[4 * q], d[4 * q + 1], d[4 * q + 2], d[4 * q + 3]};
            }
        }
    }
}

// per-chunk fp64 shares: part[c] = [W'P + P'W (Hp^2) | D'Q + Q'D (Hp^2) | sum A o P] over rows [c rpc, (c + 1) rpc) of the M real
// rows (symmetrised here, halved by the reduction).  1024 threads; rows pass through LDS GPART_ROWS at a time, P and Q read through
// frag_index from the fragment-major products.  (Staging them as fp64 instead, to save the conversions, was slower: 50 vs 33 us.)
constexpr int GPART_ROWS = 16;
template <int HP>
__global__ __launch_bounds__(1024) void gram_part_kernel(const float* __restrict__ PQ, long long n, const float* __restrict__ Wn,
                                                         const float* __restrict__ Wo, const float* __restrict__ A32, long long M,
                                                         int rpc, double* __restrict__ part, const int* __restrict__ stop) {
    if (*stop) return;
    constexpr int NH = HP / 32, EPT = HP * HP / 1024, RB = GPART_ROWS;
    __shared__ float sW[RB][HP], sP[RB][HP], sD[RB][HP], sQ[RB][HP];
    __shared__ double red[16];
    double gb[EPT], gd[EPT], tr = 0.0;
#pragma unroll
    for (int u = 0; u < EPT; ++u) { gb[u] = 0.0; gd[u] = 0.0; }
    const long long m0 = (long long)blockIdx.x * rpc, m1 = min(m0 + rpc, M);
    for (long long mb = m0; mb < m1; mb += RB) {
        __syncthreads();
        for (int t = threadIdx.x; t < RB * HP; t += 1024) {
            const int r = t / HP, h = t % HP;
            const long long m = mb + r;
            float w = 0.f, p = 0.f, d = 0.f, q = 0.f;
            if (m < m1) {
                const long long f = frag_index(h, m, NH);
                w = Wn[m * HP + h];
                d = (float)((double)w - (double)Wo[m * HP + h]);
                p = PQ[f];
                q = PQ[n + f];
                tr += (double)A32[m * HP + h] * (double)p;
            }
            sW[r][h] = w; sP[r][h] = p; sD[r][h] = d; sQ[r][h] = q;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < EPT; ++u) {
            const int e = threadIdx.x + 1024 * u, i = e / HP, k = e % HP;
            double sb = 0.0, sd = 0.0;
#pragma unroll 4
            for (int r = 0; r < RB; ++r) {
                sb += (double)sW[r][i] * (double)sP[r][k] + (double)sW[r][k] * (double)sP[r][i];
                sd += (double)sD[r][i] * (double)sQ[r][k] + (double)sD[r][k] * (double)sQ[r][i];
            }
            gb[u] += sb;
            gd[u] += sd;
        }
    }
    double* o = part + (long long)blockIdx.x * (2 * HP * HP + 1);
#pragma unroll
    for (int u = 0; u < EPT; ++u) {
        const int e = threadIdx.x + 1024 * u;
        o[e] = gb[u];
        o[HP * HP + e] = gd[u];
    }
    tr = block_sum(tr, red);
    if (threadIdx.x == 0) o[2 * HP * HP] = tr;
}

// the shares summed in a fixed order into st: GB = (W'P + P'W) / 2, GD likewise, GX[0] = sum A o P.  Workgroup: 16 entries x 16
// chunk groups (group g sums chunks g, g + 16, ...; eight loads in flight), the 16 group sums then added in group order.
constexpr int GRED_E = 16, GRED_G = 16;
__global__ __launch_bounds__(256) void gram_part_reduce_kernel(const double* __restrict__ part, int nchunk, int Hp,
                                                               double* __restrict__ st, StateLayout lay, const int* __restrict__ stop) {
    if (*stop) return;
    __shared__ double sum[GRED_G][GRED_E];
    const int n2 = Hp * Hp;
    const long long stride = 2LL * n2 + 1;
    const int el = threadIdx.x % GRED_E, g = threadIdx.x / GRED_E;
    const int t = blockIdx.x * GRED_E + el;
    double a = 0.0;
    if (t <= 2 * n2) {
        int c = g;
        for (; c + 7 * GRED_G < nchunk; c += 8 * GRED_G) {
            double v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = part[(long long)(c + k * GRED_G) * stride + t];
#pragma unroll
            for (int k = 0; k < 8; ++k) a += v[k];
        }
        for (; c < nchunk; c += GRED_G) a += part[(long long)c * stride + t];
    }
    sum[g][el] = a;
    __syncthreads();
    if (g != 0 || t > 2 * n2) return;
    double s = 0.0;
    for (int k = 0; k < GRED_G; ++k) s += sum[k][el];
    if (t == 2 * n2) st[lay.GX()] = s;
    else st[(t < n2 ? lay.GB() : lay.GD()) + (t % n2)] = 0.5 * s;
}

}  // namespace vbmf
