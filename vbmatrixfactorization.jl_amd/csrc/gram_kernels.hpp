// gram_kernels.hpp -- the Gram-form sweep of vbmf_run for tall matrices.
//
// updateB! is B = Y A SigmaB / sigma2 with no mask on B, so after any sweep B = Y W with W = A SigmaB / sigma2 (M x H).  Every
// quantity a sweep takes from Y then comes from the M x M Gram matrix G = Y'Y, built once per Y:
//     Y'B = G W (= P, from which updateA! builds A),   B'B = W'(G W),   tr(B'YA) = sum A o (G W),   dB'dB = D'(G D), D = W_new - W_old.
//
//   gram_build_kernel      G = Y'Y from the pass-1 tiles of Y (bf16 products are exact in fp32; fp32 over chunks of GRAM_CHUNK
//                          k-steps, the chunks summed in fp64, rounded once); upper 128 x 128 blocks, each stored with its mirror
//   gram_w_kernel          W_new = A (SigmaB / sigma2) on fp64 MFMA, D = W_new - W_old; fp32 W and the product's bf16 operand planes
//   gram_prod_kernel       [P | Q] = G [W | D] as split-K slabs in the fragment-major layout of the pass-1 product
//   gram_tail_kernel       the slabs folded into [P | Q] and, from the folded values, per-chunk fp64 shares of W'P, D'Q (each
//                          product once, on fp64 MFMA) and sum A o P
//   gram_part_reduce_kernel  fixed-order sum of the shares -> the state's [B'B | dB'dB | tr(B'YA)], symmetrised as (C + C') / 2
//
// Rank 256 (Hp = 256, the ARD-sparse model under VBMF_GRAM_FORM_ON) runs on the Hp = 128 geometry of each kernel, blocked:
// gram_w_cols_kernel<256, 2> (two workgroups per row block, one per column half), gram_prod_kernel<4, 8> (two h-tile groups),
// gram_tail_kernel<128, 256> (four 128 x 128 blocks per product and chunk), gram_part_reduce_kernel<128, 256>.
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
// gram_prod_kernel streams a G of more bytes than this past the caches ("G past the caches"): with the rest
// of a sweep's traffic such a G no longer fits the 256 MiB Infinity Cache.  Measured at 100k rows, H = 64: the default policy is
// 2.5-3.5 % ahead in sweeps/s at M = 4000 .. 7000 (G 67-206 MB), non-temporal pieces 1.7 % at M = 8000 (268 MB), 4 % at 10 000.
constexpr long long GRAM_G_NT_BYTES = 240LL << 20;

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

// W_new = A S (S = SigmaB / sigma2, Hp x Hp fp32, zero outside H x H), D = W_new - W_old, on v_mfma_f64_16x16x4_f64 (blk_inverse.hpp's
// register layouts).  Workgroup b: the GW_ROWS rows of k-steps [GW_KS b, GW_KS (b + 1)); wave cb (HP / 16 of them) the 16 columns
// [16 cb, 16 cb + 16).  The wave holds its column panel of S in registers as B operands (lane (q, c), chunk (s, t): S[16 s + 4 q + t]
// [16 cb + c]) and reads A as float4 rows (lane (q, c): A[m0 + c][16 s + 4 q .. + 3], element t the A operand of chunk (s, t)), so
// every product is an fp64 sum of exact fp32 x fp32 products.  W, rounded to fp32, goes through LDS to the pack stage: thread
// (k-step, h tile ht, lane) the eight rows m = 16 j + 8 half + e of column h = 32 ht + c, written as the old one-workgroup-per-k-step
// kernel wrote them (fp32 W, D formed in fp64 then rounded, 3 + 2 bf16 planes).  Rows >= M are zero.
constexpr int GW_KS = 2, GW_ROWS = 16 * GW_KS;
template <int HP>
__global__ __launch_bounds__(HP * 4) void gram_w_kernel(const float* __restrict__ A32, const float* __restrict__ S,
                                                        const float* __restrict__ Wold, float* __restrict__ Wnew,
                                                        uint4* __restrict__ Wt, long long M, int KT, const int* __restrict__ stop) {
    if (*stop) return;
    constexpr int NS = HP / 16, NH = HP / 32, NT = HP * 4;
    __shared__ float sW[GW_ROWS][HP + 1];
    const int lane = threadIdx.x & 63, cb = threadIdx.x >> 6;
    const int q = lane >> 4, c = lane & 15;
    const long long row0 = (long long)blockIdx.x * GW_ROWS;
    double sb[NS][4];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int t = 0; t < 4; ++t) sb[s][t] = (double)S[(long long)(16 * s + 4 * q + t) * HP + 16 * cb + c];
#pragma unroll
    for (int mb = 0; mb < GW_KS; ++mb) {
        const long long m = row0 + 16 * mb + c;
        float4 a[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s)
            a[s] = m < M ? *reinterpret_cast<const float4*>(A32 + m * HP + 16 * s + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
        f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a[s].x, sb[s][0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a[s].y, sb[s][1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a[s].z, sb[s][2], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a[s].w, sb[s][3], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) sW[16 * mb + q + 4 * r][16 * cb + c] = (float)acc[r];
    }
    __syncthreads();
    const long long plane = (long long)KT * NH * 64;
    for (int it = threadIdx.x; it < GW_KS * NH * 64; it += NT) {
        const int jj = it / (NH * 64), ht = (it / 64) % NH, ln = it & 63;
        const int half = ln >> 5, h = 32 * ht + (ln & 31);
        const long long j = (long long)blockIdx.x * GW_KS + jj;
        if (j >= KT) continue;
        unsigned short wp[3][8], dp[2][8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const long long m = 16 * j + 8 * half + e;
            const float wv = sW[16 * jj + 8 * half + e][h];
            const float dv = (float)((double)wv - (double)Wold[m * HP + h]);
            Wnew[m * HP + h] = wv;
            wp[0][e] = f2bf(wv);
            float res = wv - bf2f(wp[0][e]);
            wp[1][e] = f2bf(res);
            res -= bf2f(wp[1][e]);
            wp[2][e] = f2bf(res);
            dp[0][e] = f2bf(dv);
            dp[1][e] = f2bf(dv - bf2f(dp[0][e]));
        }
        const long long o = (j * NH + ht) * 64 + ln;
#pragma unroll
        for (int p = 0; p < 3; ++p)
            Wt[p * plane + o] = make_uint4(pack_bf2(wp[p][0], wp[p][1]), pack_bf2(wp[p][2], wp[p][3]), pack_bf2(wp[p][4], wp[p][5]),
                                           pack_bf2(wp[p][6], wp[p][7]));
#pragma unroll
        for (int p = 0; p < 2; ++p)
            Wt[(3 + p) * plane + o] = make_uint4(pack_bf2(dp[p][0], dp[p][1]), pack_bf2(dp[p][2], dp[p][3]), pack_bf2(dp[p][4], dp[p][5]),
                                                 pack_bf2(dp[p][6], dp[p][7]));
    }
}

// The same at HP = 256, where one workgroup would be 1024 threads (a 128-register budget) holding 64 doubles of S per lane: the
// columns go to NCG = 2 workgroups of 512 threads (blockIdx.y = column group: HP / NCG columns, HP / NCG / 16 waves), the register
// budget doubles and the panel fits.  Every wave still sums its column over all HP rows of S in the order above, so an element of
// W is the value the one-workgroup form would give; the pack stage writes the column group's h tiles of the NH = HP / 32 layout.
template <int HP, int NCG>
__global__ __launch_bounds__(HP * 4 / NCG) void gram_w_cols_kernel(const float* __restrict__ A32, const float* __restrict__ S,
                                                                   const float* __restrict__ Wold, float* __restrict__ Wnew,
                                                                   uint4* __restrict__ Wt, long long M, int KT,
                                                                   const int* __restrict__ stop) {
    if (*stop) return;
    constexpr int NS = HP / 16, NH = HP / 32, HC = HP / NCG, NHC = NH / NCG, NT = HP * 4 / NCG;
    static_assert(HC % 32 == 0 && NT <= 512, "gram_w_cols geometry");
    __shared__ float sW[GW_ROWS][HC + 1];
    const int lane = threadIdx.x & 63, cb = threadIdx.x >> 6;
    const int q = lane >> 4, c = lane & 15;
    const int col0 = blockIdx.y * HC;                              // first column of this workgroup
    const long long row0 = (long long)blockIdx.x * GW_ROWS;
    double sb[NS][4];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int t = 0; t < 4; ++t) sb[s][t] = (double)S[(long long)(16 * s + 4 * q + t) * HP + col0 + 16 * cb + c];
#pragma unroll
    for (int mb = 0; mb < GW_KS; ++mb) {
        const long long m = row0 + 16 * mb + c;
        f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const float4 a = m < M ? *reinterpret_cast<const float4*>(A32 + m * HP + 16 * s + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a.x, sb[s][0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a.y, sb[s][1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a.z, sb[s][2], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a.w, sb[s][3], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) sW[16 * mb + q + 4 * r][16 * cb + c] = (float)acc[r];
    }
    __syncthreads();
    const long long plane = (long long)KT * NH * 64;
    for (int it = threadIdx.x; it < GW_KS * NHC * 64; it += NT) {
        const int jj = it / (NHC * 64), htl = (it / 64) % NHC, ln = it & 63;
        const int half = ln >> 5, hl = 32 * htl + (ln & 31), h = col0 + hl, ht = blockIdx.y * NHC + htl;
        const long long j = (long long)blockIdx.x * GW_KS + jj;
        if (j >= KT) continue;
        unsigned short wp[3][8], dp[2][8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const long long m = 16 * j + 8 * half + e;
            const float wv = sW[16 * jj + 8 * half + e][hl];
            const float dv = (float)((double)wv - (double)Wold[m * HP + h]);
            Wnew[m * HP + h] = wv;
            wp[0][e] = f2bf(wv);
            float res = wv - bf2f(wp[0][e]);
            wp[1][e] = f2bf(res);
            res -= bf2f(wp[1][e]);
            wp[2][e] = f2bf(res);
            dp[0][e] = f2bf(dv);
            dp[1][e] = f2bf(dv - bf2f(dp[0][e]));
        }
        const long long o = (j * NH + ht) * 64 + ln;
#pragma unroll
        for (int p = 0; p < 3; ++p)
            Wt[p * plane + o] = make_uint4(pack_bf2(wp[p][0], wp[p][1]), pack_bf2(wp[p][2], wp[p][3]), pack_bf2(wp[p][4], wp[p][5]),
                                           pack_bf2(wp[p][6], wp[p][7]));
#pragma unroll
        for (int p = 0; p < 2; ++p)
            Wt[(3 + p) * plane + o] = make_uint4(pack_bf2(dp[p][0], dp[p][1]), pack_bf2(dp[p][2], dp[p][3]), pack_bf2(dp[p][4], dp[p][5]),
                                                 pack_bf2(dp[p][6], dp[p][7]));
    }
}

// a - b as one v_sub_f32.  Written out because the compiler packs neighbouring fp32 subtractions into v_pk_add_f32, which beside
// MFMAs costs more than the two scalar instructions it replaces; the result is the same IEEE difference.
__device__ __forceinline__ float sub_f32(float a, float b) {
    float r;
    asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// two fp32 values rounded to bf16 (RNE) in one v_cvt_pk_bf16_f32: lo in bits 0..15, hi in bits 16..31
__device__ __forceinline__ unsigned cvt_pk_bf16(float lo, float hi) {
    typedef __attribute__((ext_vector_type(2))) float f32x2v;
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2v;
    const f32x2v v = {lo, hi};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2v));
}
// three bf16 parts of 8 fp32 values as MFMA operand fragments: x = p0 + p1 + p2 to an fp32 rounding, each part the RNE bf16 of what
// the parts before it left.  Pairs stay packed as the conversion leaves them: the high half is unpacked by one v_and_b32, the low
// half by one v_lshlrev_b32.
__device__ __forceinline__ void split3_frag(const f32x4& x0, const f32x4& x1, u32x4v& g0, u32x4v& g1, u32x4v& g2) {
    const float v[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float a = v[2 * e], b = v[2 * e + 1];
        const unsigned p0 = cvt_pk_bf16(a, b);
        a = sub_f32(a, bitsf(p0 << 16));
        b = sub_f32(b, bitsf(p0 & 0xffff0000u));
        const unsigned p1 = cvt_pk_bf16(a, b);
        a = sub_f32(a, bitsf(p1 << 16));
        b = sub_f32(b, bitsf(p1 & 0xffff0000u));
        g0[e] = p0;
        g1[e] = p1;
        g2[e] = cvt_pk_bf16(a, b);
    }
}

__device__ __forceinline__ f32x16 mfma_bf(const u32x4v& a, const u32x4v& b, const f32x16& c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// [P | Q] = G [W | D], split-K.  Workgroup b: row group b % nrg (TPG = 16 / NH row tiles), k-steps [s sps, (s + 1) sps) of split
// s = b / nrg.  Out: slab s at Out + s * slab_floats, P fragment-major (tiles x < XT1) followed by Q at Out + s * slab_floats + n.
//
// Geometry.  NW = 8 waves, two per SIMD: while one wave splits its G fragment into bf16 parts (vector ALU) or waits for a load, the
// other keeps the SIMD's matrix pipe busy.  Wave w takes NXW = TPG / 8 row tiles with all NH h tiles (NH = 1, 2); at NH = 4 the
// row group has four tiles, so waves w and w + 4 share tile w % 4 and take two h tiles each (both stream and split that tile's G).
//
// Pipeline.  Nothing the k-loop loads passes through registers: G and the W / D planes arrive by LDS-DMA in 1 KB pieces (one
// wave-instruction each, lds_dma_piece), so no load result is carried round the loop edge and every wait is a counted vmcnt that
// the source states.  G: each wave owns a ring of D slots of its own fragments (2 NXW pieces per k-step, LDS image = memory image,
// lane l's 32 bytes at 32 l), filled D k-steps ahead; slot t % D is refilled with k-step t + D right after k-step t has been read
// out of it and split.  The wait before reading k-step t leaves the D - 1 younger k-steps (and any plane pieces issued among them)
// in flight.  No other wave reads the ring, so it needs no barrier.  Planes: 5 NH pieces per k-step, the same for every wave,
// double-buffered by chunks of CH k-steps; the workgroup's waves issue chunk c + 1 (PPW pieces each; where 5 NH CH is no multiple
// of 8 the last piece is issued more than once so that every wave counts the same loads) at the first k-step of chunk c, wait for
// them after its last k-step with the G refills issued since still in flight, and one raw s_barrier per chunk publishes them
// (__syncthreads would drain vmcnt).  The prologue issues the same sequence the loop would have issued for k-steps -D .. -1, so
// the loop's wait counts hold from its first trip.  Loads past the split's end are clamped to its last k-step (always in bounds,
// never branched round); the k-steps they stand for do no MFMA.  Every DMA is waited for before the workgroup's LDS is given up.
// Every accumulator sees the MFMA sequence of the kernels this replaced (term order, k-step order, split plan), so [P | Q] is
// bitwise what it was.
// Measured at 100k x 10k, H = 64 (config 4, 1M x 10k, H = 128, in brackets; roofline.pass1 of the bench, parent and this build
// alternated on one machine, profiles/gram_prod_overlap_bench_ab.txt): 0.119-0.120 ms (0.201-0.204 ms); the kernel this replaced,
// G in a register ring and four waves per workgroup, 0.130-0.131 ms (0.249-0.251 ms).  Its counters (profiles/gram_prod_overlap_*): the matrix pipe was busy for 50 % of a
// wave's life, the wave parked at a wait or barrier for 16 % only; the rest was its own vector work, issued between the MFMA
// blocks and not beside them.  With two waves per SIMD the pipe is busy for 63 %.
// Tried on this kernel in an earlier alternated run (this form 0.118-0.119 ms there, the parent 0.134 ms), all within 1 % of it
// at the headline and therefore not kept: a ring five k-steps deep (all 160 KB of
// LDS) 0.119 ms (0.206-0.207 ms); waves 4-7 rotated by half a k-step, so that SIMD partners alternate between split and MFMAs
// from every barrier on, 0.118-0.119 ms (0.205-0.206 ms); the k-step's DMA pieces issued between its MFMAs (sched_group_barrier,
// one per two to six MFMAs) instead of ahead of them 0.119 ms (0.213-0.214 ms).  None of ring depth, barrier lockstep or the
// place of the DMA issue is what bounds it now.
// Cache policy.  G is read once per sweep, by one wave per fragment.  Where it is larger than the caches can keep from one sweep
// to the next (GRAM_G_NT_BYTES), its pieces are non-temporal (lds_dma_piece_nt): the same bytes, which then do not push the
// planes, the slabs and the other kernels' operands out of L2 and the Infinity Cache.  At the headline 4564-4580 -> 4745-4763
// sweeps/s in a first alternated run, the kernel itself 117-118 -> 113 us (profiles/gram_prod_nt_*); a smaller G stays on the
// default policy, under which the Infinity Cache serves it from the second sweep on.  The planes, which every workgroup
// re-reads, always do.
//
// VBMF_GRAMPROD_PROBE (timing builds only, passed through VBMF_HIPCC_FLAGS; off by default: the shipped kernels execute nothing
// extra).  A probe build's [P | Q] is wrong, so it never goes through the tests, and bench.py ends such a run after one sweep
// (the stop test sees d = 0 or a non-finite value); scripts/gram_prod_probe_time.py launches the kernel for a kernel trace.
//   1: G's descriptors get zero records, so the range check drops every G load (zeros arrive); the instruction stream, the waits
//      and the barriers stay as they are.
//   2: the loop issues no G piece; the ring keeps what the prologue loaded and the wait counts are those of the shorter queue.
//   3: every G piece reads its row tile's first k-step (2 KB per tile, cache-resident): the stream of 1 on real operands, since
//      all-zero operands alone let the chip hold a higher clock.
// What the three decided (G's arrival from memory costs 11-12 us of 115, issuing its pieces 2-3): DESIGN.md section 10,
// "Fourth form, not kept".
#ifndef VBMF_GRAMPROD_PROBE
#define VBMF_GRAMPROD_PROBE 0
#endif
template <int NH>
struct GramProd {
    static constexpr int NW = 8;                              // waves per workgroup
    static constexpr int THREADS = 64 * NW;
    static constexpr int TPG = 16 / NH;                       // row tiles per row group (the split plan's unit: gram_prepare)
    static constexpr int NXW = TPG >= NW ? TPG / NW : 1;      // row tiles per wave
    static constexpr int HS = TPG >= NW ? 1 : NW / TPG;       // waves sharing a row tile
    static constexpr int NHW = NH / HS;                       // h tiles per wave
    static constexpr int CH = NH == 2 ? 4 : 2;                // k-steps per plane chunk (one barrier each)
    static constexpr int D = 4;                               // G ring depth in k-steps (slot = k-step mod D, a scalar counter)
    static constexpr int U = CH;                              // k-steps per unrolled loop body
    static constexpr int NP = GRAM_PLANES * CH * NH;          // 1 KB pieces of one plane chunk
    static constexpr int PPW = (NP + NW - 1) / NW;            // plane pieces a wave issues per chunk
    static constexpr int GL = 2 * NXW;                        // G pieces a wave issues per k-step
    static constexpr int GQ = VBMF_GRAMPROD_PROBE == 2 ? 0 : GL;   // of them in the loop's queue
    static constexpr int PLANE_BYTES = 2 * NP * 1024;         // 20 / 80 / 80 KB
    static constexpr int RING_BYTES = NW * D * GL * 1024;     // 128 / 64 / 64 KB
    static constexpr int LDS_BYTES = PLANE_BYTES + RING_BYTES;
    static_assert(NXW * (NW / HS) == TPG && NHW * HS == NH, "gram_prod geometry");
    static_assert(LDS_BYTES <= 160 * 1024, "gram_prod LDS");
    // loads a wave has issued after the G pieces of k-step t (t mod U = u) by the time it reads them: the G refills of the D - 1
    // k-steps t - D + 1 .. t - 1 and the plane pieces issued at those of them that open a chunk
    static constexpr int g_wait(int u) {
        int n = (D - 1) * GQ;
        for (int d = 1; d < D; ++d) n += ((u + CH * D - d) % CH == 0) ? PPW : 0;
        return n;
    }
};
//
// NHT > NH: the workgroup multiplies h-tile group blockIdx.y (NH tiles) of NHT in all -- the operand planes and the output are in the
// NHT layout, the geometry, the loop and every accumulator's MFMA sequence are those of NH.  Rank 256 runs as two groups of <4>:
// G is read once per group; the other way, GramProd<8> with one k-step per plane chunk, is in DESIGN.md section 10.
template <int NH, int NHT = NH>
__global__ __launch_bounds__(GramProd<NH>::THREADS) void gram_prod_kernel(const float4* __restrict__ Gt, const uint4* __restrict__ Wt,
                                                                          float* __restrict__ Out, int GT, int XT1, int sps, int nrg,
                                                                          long long n, long long slab_floats,
                                                                          const int* __restrict__ stop) {
    using C = GramProd<NH>;
    constexpr int NW = C::NW, NXW = C::NXW, NHW = C::NHW, D = C::D, CH = C::CH, U = C::U, NP = C::NP, PPW = C::PPW, GL = C::GL;
    extern __shared__ __attribute__((aligned(1024))) unsigned char gram_lds[];   // [2][plane][k-step of the chunk][h tile] 1 KB, then [wave][slot][tile][2] 1 KB
    if (*stop) return;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int rg = blockIdx.x % nrg, s = blockIdx.x / nrg;
    const int KT = 2 * GT;
    const int j0 = s * sps, j1 = min(j0 + sps, KT), nk = j1 - j0;
    const int pt0 = rg * C::TPG + (w % (C::TPG / NXW)) * NXW;          // first row tile of this wave
    const int h0 = (w / (C::TPG / NXW)) * NHW;                        // first h tile of this wave
    const int hg0 = NHT == NH ? 0 : (int)blockIdx.y * NH;             // first h tile of this workgroup's group
    const long long plane = (long long)KT * NHT * 64;
    f32x16 accP[NXW][NHW], accQ[NXW][NHW];
#pragma unroll
    for (int i = 0; i < NXW; ++i)
#pragma unroll
        for (int h = 0; h < NHW; ++h)
#pragma unroll
            for (int r = 0; r < 16; ++r) { accP[i][h][r] = 0.f; accQ[i][h][r] = 0.f; }
    // one descriptor per row tile (its KT k-steps of 2 KB) and one for the planes: a load is range-checked against its own array
    __amdgpu_buffer_rsrc_t gr[NXW];
#pragma unroll
    for (int i = 0; i < NXW; ++i)
        gr[i] = __builtin_amdgcn_make_buffer_rsrc((void*)(Gt + (long long)(pt0 + i) * KT * 128), 0,
                                                  VBMF_GRAMPROD_PROBE == 1 ? 0u : (unsigned)KT * 2048u, 0x00020000);
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc((void*)Wt, 0, (unsigned)(GRAM_PLANES * plane * 16), 0x00020000);
    const int voff = lane * 16;
    unsigned char* const ring = gram_lds + C::PLANE_BYTES + w * (D * GL * 1024);
    // a G the caches cannot keep from one sweep to the next is streamed past them (non-temporal pieces): read once per sweep, it
    // would only push out what the sweep's other kernels re-read.  One wave-uniform branch per k-step; the bytes are the same.
    // Not at NH = 4 with one h-tile group (config 4): there the kernel itself measured 8 us slower with them (202 -> 210 us) and
    // the sweep 0.7 % slower, so that instantiation keeps the default policy.
    const bool g_nt = !(NH == 4 && NHT == 4) && (long long)GT * GT * 4096 > GRAM_G_NT_BYTES;
    auto load_g = [&](int slot, int t) __attribute__((always_inline)) {      // k-step j0 + t, clamped to the split
        const int so = VBMF_GRAMPROD_PROBE == 3 ? 0 : min(j0 + t, j1 - 1) * 2048;
        if (g_nt) {
#pragma unroll
            for (int i = 0; i < NXW; ++i) {
                lds_dma_piece_nt(gr[i], ring + (slot * GL + 2 * i) * 1024, voff, so);
                lds_dma_piece_nt(gr[i], ring + (slot * GL + 2 * i + 1) * 1024, voff, so + 1024);
            }
        } else {
#pragma unroll
            for (int i = 0; i < NXW; ++i) {
                lds_dma_piece(gr[i], ring + (slot * GL + 2 * i) * 1024, voff, so);
                lds_dma_piece(gr[i], ring + (slot * GL + 2 * i + 1) * 1024, voff, so + 1024);
            }
        }
    };
    // this wave's pieces of the plane chunk starting at k-step j0 + t into buffer cc: piece x = (plane q, k-step kk, h tile h)
    auto load_planes = [&](int cc, int t) __attribute__((always_inline)) {
#pragma unroll
        for (int v = 0; v < PPW; ++v) {
            const int x = min(w + NW * v, NP - 1);
            const int q = x / (CH * NH), r = x % (CH * NH);
            const int j = min(j0 + t + r / NH, j1 - 1);
            lds_dma_piece(wr, gram_lds + (cc * NP + x) * 1024, voff, (int)(q * plane + ((long long)j * NHT + hg0 + r % NH) * 64) * 16);
        }
    };
    // the sequence the loop issues at k-steps -D .. -1: chunk 0's planes (at each chunk start among them; the same bytes to the same
    // place) and G k-steps 0 .. D - 1
#pragma unroll
    for (int d = 0; d < D; ++d) {
        if ((d + CH * D - D) % CH == 0) load_planes(0, 0);
        load_g(d, d);
    }
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(CH * GL) : "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    u32x4v wf[GRAM_PLANES][NHW], g[NXW][3];
    auto mma = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < NXW; ++i) {
#pragma unroll
            for (int h = 0; h < NHW; ++h) {
                // smallest terms first: W2 G0, W1 G1, W0 G2, W1 G0, W0 G1, W0 G0
                f32x16 a = accP[i][h];
                a = mfma_bf(wf[2][h], g[i][0], a);
                a = mfma_bf(wf[1][h], g[i][1], a);
                a = mfma_bf(wf[0][h], g[i][2], a);
                a = mfma_bf(wf[1][h], g[i][0], a);
                a = mfma_bf(wf[0][h], g[i][1], a);
                accP[i][h] = mfma_bf(wf[0][h], g[i][0], a);
                f32x16 d = accQ[i][h];
                d = mfma_bf(wf[4][h], g[i][0], d);
                d = mfma_bf(wf[3][h], g[i][1], d);
                accQ[i][h] = mfma_bf(wf[3][h], g[i][0], d);
            }
        }
    };
    int slot = 0;                                             // ring slot of the current k-step
    // U k-steps from t0 (a multiple of U).  tail: k-steps at or past nk do no MFMA (their loads and waits still run).
    auto body = [&](int t0, bool tail) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = t0 + u, kk = u % CH;
            const int cc = (t / CH) & 1;
            const bool live = !tail || t < nk;
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(C::g_wait(u)) : "memory");
            if (live) {
                const unsigned char* gs = ring + slot * (GL * 1024) + lane * 32;
                f32x4 x[NXW][2];
#pragma unroll
                for (int i = 0; i < NXW; ++i) {
                    x[i][0] = *reinterpret_cast<const f32x4*>(gs + i * 2048);
                    x[i][1] = *reinterpret_cast<const f32x4*>(gs + i * 2048 + 16);
                }
                const unsigned char* pl = gram_lds + (cc * NP + kk * NH + h0) * 1024 + lane * 16;
#pragma unroll
                for (int q = 0; q < GRAM_PLANES; ++q)
#pragma unroll
                    for (int h = 0; h < NHW; ++h) wf[q][h] = *reinterpret_cast<const u32x4v*>(pl + (q * CH * NH + h) * 1024);
#pragma unroll
                for (int i = 0; i < NXW; ++i) split3_frag(x[i][0], x[i][1], g[i][0], g[i][1], g[i][2]);
            }
            // the slot is refilled only after its fragments have arrived in registers (the split has consumed them)
            __builtin_amdgcn_sched_barrier(0);
            if (kk == 0) load_planes(cc ^ 1, t + CH);
            if (VBMF_GRAMPROD_PROBE != 2) load_g(slot, t + D);
            slot = slot + 1 == D ? 0 : slot + 1;
            __builtin_amdgcn_sched_barrier(0);
            if (live) mma();
            if (kk == CH - 1) {
                // my pieces of the next chunk have landed (the G refills issued since stay in flight) and my reads of this chunk's
                // buffer have returned; after the barrier everybody's have, and the next chunk's first k-step may refill the buffer
                asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(CH * C::GQ) : "memory");
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
            }
        }
    };
    int t0 = 0;
    for (; t0 + U <= nk; t0 += U) body(t0, false);
    if (t0 < nk) body(t0, true);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // run-ahead pieces still target this workgroup's LDS
    float4* oP = reinterpret_cast<float4*>(Out + (long long)s * slab_floats);
    float4* oQ = reinterpret_cast<float4*>(Out + (long long)s * slab_floats + n);
#pragma unroll
    for (int i = 0; i < NXW; ++i) {
        const int p = pt0 + i;
        if (p >= XT1) continue;
#pragma unroll
        for (int h = 0; h < NHW; ++h) {
            const long long o = (((long long)p * NHT + hg0 + h0 + h) * 64 + lane) * 4;
            const f32x16 a = accP[i][h], d = accQ[i][h];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                oP[o + q] = float4{a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]};
                oQ[o + q] = float4{d[4 * q], d[4 * q + 1], d[4 * q + 2], d[4 * q + 3]};
            }
        }
    }
}

// gram_tail_kernel: the split-K slabs of [P | Q] folded and the per-chunk fp64 shares formed from the folded values in one launch.
// part[c] = [W'P (Hp^2) | D'Q (Hp^2) | sum A o P] over rows [c rpc, (c + 1) rpc) of the M real rows, on v_mfma_f64_16x16x4_f64, each
// product formed once (the reduction symmetrises).
//
// Grid 2 nchunk: workgroup (chunk, pi) takes product P (pi = 0) or Q (pi = 1) of one row chunk; the two halves share nothing but the
// chunk's trace slot, which only the P half has a share in.  512 threads = S row subsets x V column offsets, V = HP / 16, S = 8 / V.
//
// Fold.  The chunk's rows of the product go by in blocks of ROWS rows (three 16-byte pieces per thread, two at HP = 128: the
// headline's 80-row chunk is one block).  Thread t takes pieces t, t + 512, t + 1024 of the block in memory order (a wave: one contiguous 1 KB of a
// 16-row group), requests each from up to eight slabs at once, adds them in slab order in fp32 as slab_sum_kernel does
// (((s0 + s1) + s2) + ...; further rounds of eight for more slabs), stores the sum to PQ (not when there is one slab: then PQ is the
// product itself and is read in place) and leaves it in LDS as rows x HP.  Every piece is folded once.  The last chunk's workgroups
// also fold the rows from the end of their chunk to Mp1, which belong to no chunk, so that all of PQ is written.  The stop flag and
// the W / A values of the block are requested with the block's first round; only the return and the stores wait for the flag.  The
// next block's first round is requested before the barrier that publishes this one (a raw s_barrier behind an LDS-only wait:
// __syncthreads would drain the loads), into the other LDS buffer.
//
// Shares.  Lane (q, c) of wave (s, tw) takes, per 4-row step of its subset (steps s, s + S, ... of the chunk, in that order), row
// m = m0 + 4 step + q: the V columns V c .. V c + V - 1 of the folded product from LDS, which are its B operands (column V c + t in
// accumulator t), and the one value of W (or D, formed in fp64 and rounded to fp32, as gram_w forms it) at column V c + tw, its A
// operand.  Accumulator t thus holds C[V (q + 4 r) + tw][V c + t] in register r; fp32 x fp32 products are exact in fp64.  Rows at or
// past the chunk's end enter as zeros, which leave every accumulator as it was.  The P half also sums A o P at its column; the
// workgroup's sum is taken over lanes as block_sum takes it and over waves in (s, tw) order -- the order of the 1024-thread kernel
// this replaced, whose Q waves added exact zeros.  The S subsets are folded through LDS in subset order; the share is stored in
// register order (gpart_index).
template <int HP>
struct GPart {
    static constexpr int V = HP / 16, S = 8 / V, NH = HP / 32;
    static constexpr int NT = 512, SD = 8;                    // threads, slabs per round
    static constexpr int PPT = HP == 128 ? 2 : 3;             // pieces per thread and block (V = 8: 64 accumulator registers)
    static constexpr int ROWS = PPT * NT * 4 / HP;            // rows per block: 192 / 96 / 32
    static constexpr int NSTEP = ROWS / 4 / S;                // 4-row steps per wave and block: 12 / 12 / 8
    static constexpr int BUF = ROWS * HP;                     // floats per LDS buffer (24 / 24 / 16 KB); two of them: 48 / 48 / 32 KB
    static constexpr int SU = V == 8 ? 2 : 4;                  // steps skipped or taken together
    static_assert(NSTEP % SU == 0 && (ROWS / 4) % S == 0 && ROWS % 16 == 0, "gram_tail geometry");
    static_assert((S - 1) * V * V * 64 * 32 <= 2 * BUF * 4, "gram_tail: the subset fold reuses the block buffers");
};
// position of C[a][b] of one product inside a share (register order of gram_tail_kernel)
template <int HP>
__device__ __forceinline__ int gpart_index(int a, int b) {
    constexpr int V = GPart<HP>::V;
    const int tw = a % V, i = a / V, t = b % V, c = b / V;
    return ((((tw * V + t) * 4 + (i >> 2)) << 6) + 16 * (i & 3) + c);
}
__device__ __forceinline__ void add4(float4& s, const float4& v) { s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w; }
// one round of gram_tail's fold for one piece: the loads of cnt (1 .. 8) slabs as one straight-line run entered at its cnt-th last
// load (slab u through its own descriptor r[u], the piece's byte offset in voff), and their sum in slab order
struct GTailRound { float4 a0, a1, a2, a3, a4, a5, a6, a7; };
__device__ __forceinline__ void gtail_load(GTailRound& v, const __amdgpu_buffer_rsrc_t (&r)[8], int voff, int cnt) {
    const auto ld = [&](int u) __attribute__((always_inline)) {
        return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r[u], voff, 0, 0));
    };
    switch (cnt) {
        default: v.a7 = ld(7); [[fallthrough]];
        case 7: v.a6 = ld(6); [[fallthrough]];
        case 6: v.a5 = ld(5); [[fallthrough]];
        case 5: v.a4 = ld(4); [[fallthrough]];
        case 4: v.a3 = ld(3); [[fallthrough]];
        case 3: v.a2 = ld(2); [[fallthrough]];
        case 2: v.a1 = ld(1); [[fallthrough]];
        case 1: v.a0 = ld(0);
    }
}
template <bool FIRST>
__device__ __forceinline__ float4 gtail_sum(const GTailRound& v, float4 f, int cnt) {
    if (FIRST) f = v.a0;
    else add4(f, v.a0);
    if (cnt > 1) add4(f, v.a1);
    if (cnt > 2) add4(f, v.a2);
    if (cnt > 3) add4(f, v.a3);
    if (cnt > 4) add4(f, v.a4);
    if (cnt > 5) add4(f, v.a5);
    if (cnt > 6) add4(f, v.a6);
    if (cnt > 7) add4(f, v.a7);
    return f;
}
//
// HPT > HP (rank 256 as HP = 128): a share of HPT x HPT would be 256 fp64 registers per thread, so it is blocked.  NQ^2 workgroups
// (NQ = HPT / HP) per product and chunk, workgroup (qa, qb) forming the HP x HP block C[HP qa ..][HP qb ..] with the geometry above:
// it folds the HP columns from HP qb of the chunk's rows (both workgroups of a column half fold it; the qa = 0 one stores it to PQ)
// and takes its A operands from column HP qa on.  The share is [P blocks (qa, qb) in that order | Q blocks | NQ trace slots], each
// block in the register order of HP; trace slot q holds sum A o P over the columns of block (q, q), from that workgroup.
template <int HP, int HPT>
struct GPartBlk {
    static constexpr int NQ = HPT / HP;
    static constexpr long long STRIDE = 2LL * HPT * HPT + (NQ == 1 ? 1 : NQ);   // doubles per chunk share
};
template <int HP, int HPT = HP>
__global__ __launch_bounds__(512) void gram_tail_kernel(const float* slabs, int nslab, long long slab_floats, float* PQ, long long n,
                                                        long long Mp1, const float* __restrict__ Wn, const float* __restrict__ Wo,
                                                        const float* __restrict__ A32, long long M, int rpc, int nchunk,
                                                        double* __restrict__ part, const int* __restrict__ stop) {
    using C = GPart<HP>;
    constexpr int V = C::V, S = C::S, NH = C::NH, PPT = C::PPT, SD = C::SD, ROWS = C::ROWS, NSTEP = C::NSTEP, SU = C::SU;
    constexpr int NQ = GPartBlk<HP, HPT>::NQ, NHT = HPT / 32;
    constexpr bool BLK = NQ > 1;
    constexpr long long STRIDE = GPartBlk<HP, HPT>::STRIDE;
    static_assert(HPT % HP == 0, "gram_tail blocks");
    __shared__ __attribute__((aligned(32))) float stage[2 * C::BUF];
    __shared__ double red[8];
    const int stopv = *stop;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // known to be the same for the whole wave
    const int s = w / V, tw = w % V;
    const int q = lane >> 4, c = lane & 15;
    const unsigned cp = BLK ? blockIdx.x / (NQ * NQ) : blockIdx.x;     // (chunk, product)
    const int qa = BLK ? (blockIdx.x / NQ) % NQ : 0, qb = BLK ? blockIdx.x % NQ : 0;
    const int chunk = cp >> 1, pi = cp & 1;
    const long long m0 = (long long)chunk * rpc, m1 = min(m0 + rpc, M);
    const long long fend = chunk == nchunk - 1 ? Mp1 : m0 + rpc;     // rows folded here: a multiple of 16, as m0 is
    const float* src = slabs + (pi ? n : 0);
    float* dst = PQ + (pi ? n : 0);
    const float* X = pi ? Wo : A32;
    // piece j of this thread: 16-row group grp[j] of the block (the same for the whole wave), row xr of it, h tile ht, columns
    // 32 ht + 8 r4 + 4 half .. + 3 (post_kernels.hpp, frag_index)
    const int xr = lane >> 2, r4 = lane & 3;
    int grp[PPT], ht[PPT], half[PPT];
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const int sg = 8 * j + w;
        grp[j] = sg / (2 * NH);
        ht[j] = (sg % (2 * NH)) >> 1;
        half[j] = sg & 1;
    }
    GTailRound v[PPT];
    static_assert(SD == 8, "gram_tail: GTailRound");
    float wv[NSTEP], xv[NSTEP];
    auto piece_off = [&](long long rb, int j) __attribute__((always_inline)) {
        const long long row = rb + 16 * grp[j] + xr;
        return ((((row >> 5) * NHT + qb * NH + ht[j]) * 64 + half[j] * 32 + (row & 31)) << 4) + 4 * r4;
    };
    // slabs k0 .. k0 + cnt - 1 of the block at row rb: cnt = 1 .. SD picks one straight-line run of loads (gtail_load) or adds.
    // Buffer loads: a slab's descriptor is uniform and the piece's 32-bit offset serves all of its slabs.
    auto issue_slabs = [&](long long rb, int k0) __attribute__((always_inline)) {
        __amdgpu_buffer_rsrc_t r[SD];
#pragma unroll
        for (int u = 0; u < SD; ++u)
            r[u] = __builtin_amdgcn_make_buffer_rsrc((void*)(src + (long long)(k0 + u) * slab_floats), 0, (unsigned)(n * 4), 0x00020000);
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            if (rb + 16 * grp[j] >= fend) continue;
            gtail_load(v[j], r, (int)(piece_off(rb, j) * 4), min(SD, nslab - k0));
        }
    };
    auto fold_slabs = [&](long long rb, int k0, float4 (&f)[PPT]) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            if (rb + 16 * grp[j] >= fend) continue;
            if (k0 == 0) f[j] = gtail_sum<true>(v[j], f[j], min(SD, nslab));
            else f[j] = gtail_sum<false>(v[j], f[j], min(SD, nslab - k0));
        }
    };
    // W and A (or W_old) of the block's steps.  The descriptors end with the chunk, so rows at or past its end load as zeros.
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc((void*)Wn, 0, (unsigned)(m1 * HPT * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t xd = __builtin_amdgcn_make_buffer_rsrc((void*)X, 0, (unsigned)(m1 * HPT * 4), 0x00020000);
    auto issue_w = [&](long long rb) __attribute__((always_inline)) {
        const int o = (int)(((rb + 4 * s + q) * HPT + qa * HP + V * c + tw) * 4);
#pragma unroll
        for (int i = 0; i < NSTEP; ++i) {
            wv[i] = bitsf(__builtin_amdgcn_raw_buffer_load_b32(wr, o + i * (4 * S * HPT * 4), 0, 0));
            xv[i] = bitsf(__builtin_amdgcn_raw_buffer_load_b32(xd, o + i * (4 * S * HPT * 4), 0, 0));
        }
    };
    issue_slabs(m0, 0);
    issue_w(m0);
    if (stopv) return;
    f64x4 acc[V];
#pragma unroll
    for (int t = 0; t < V; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
    double tr = 0.0;
    int buf = 0;
    for (long long rb = m0; rb < fend; rb += ROWS, buf ^= 1) {
        float* sb = stage + buf * C::BUF;
        float4 f[PPT];
        fold_slabs(rb, 0, f);
        for (int k0 = SD; k0 < nslab; k0 += SD) {
            issue_slabs(rb, k0);
            fold_slabs(rb, k0, f);
        }
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            if (rb + 16 * grp[j] >= fend) continue;
            if (nslab > 1 && (!BLK || qa == 0)) *reinterpret_cast<float4*>(dst + piece_off(rb, j)) = f[j];
            *reinterpret_cast<float4*>(sb + (16 * grp[j] + xr) * HP + 32 * ht[j] + 8 * r4 + 4 * half[j]) = f[j];
        }
        // this block's A operands, so that the next block's may be requested
        float ac[NSTEP], xc[NSTEP];
#pragma unroll
        for (int i = 0; i < NSTEP; ++i) {
            xc[i] = xv[i];
            ac[i] = pi ? (float)((double)wv[i] - (double)xc[i]) : wv[i];
        }
        if (rb + ROWS < fend) {
            issue_slabs(rb + ROWS, 0);
            issue_w(rb + ROWS);
        }
        // everybody's pieces of this block are in LDS; the buffer is written again two blocks on, behind the next block's barrier
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
#pragma unroll
        for (int i0 = 0; i0 < NSTEP; i0 += SU) {
            if (rb + 4 * (s + S * i0) >= m1) break;
            __builtin_amdgcn_sched_barrier(0);                        // one group's LDS reads in registers at a time
#pragma unroll
            for (int i = i0; i < i0 + SU; ++i) {
                const int rl = 4 * (s + S * i) + q;
                const bool in = rb + rl < m1;
                float pv[V];
                if constexpr (V == 2) {
                    const float2 x = *reinterpret_cast<const float2*>(sb + rl * HP + 2 * c);
                    pv[0] = x.x; pv[1] = x.y;
                } else {
#pragma unroll
                    for (int g = 0; g < V / 4; ++g) {
                        const float4 x = *reinterpret_cast<const float4*>(sb + rl * HP + V * c + 4 * g);
                        pv[4 * g] = x.x; pv[4 * g + 1] = x.y; pv[4 * g + 2] = x.z; pv[4 * g + 3] = x.w;
                    }
                }
#pragma unroll
                for (int t = 0; t < V; ++t) pv[t] = in ? pv[t] : 0.f;
                if (!pi && (!BLK || qa == qb)) {
                    float p = 0.f;
#pragma unroll
                    for (int t = 0; t < V; ++t) p = t == tw ? pv[t] : p;
                    tr += (double)xc[i] * (double)p;
                }
#pragma unroll
                for (int t = 0; t < V; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)ac[i], (double)pv[t], acc[t], 0, 0, 0);
            }
        }
    }
    if constexpr (S > 1) {
        f64x4* fold = reinterpret_cast<f64x4*>(stage);
        __syncthreads();                                              // the last block has been read
        if (s > 0) {
#pragma unroll
            for (int t = 0; t < V; ++t) fold[(((s - 1) * V + tw) * V + t) * 64 + lane] = acc[t];
        }
        __syncthreads();
        if (s == 0) {
            for (int s2 = 1; s2 < S; ++s2)
#pragma unroll
                for (int t = 0; t < V; ++t) acc[t] += fold[(((s2 - 1) * V + tw) * V + t) * 64 + lane];
        }
    }
    double* o = part + (long long)chunk * STRIDE + pi * HPT * HPT + (qa * NQ + qb) * HP * HP;
    if (s == 0) {
#pragma unroll
        for (int t = 0; t < V; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[(((tw * V + t) * 4 + r) << 6) + lane] = acc[t][r];
    }
    if (pi || (BLK && qa != qb)) return;
    for (int off = 32; off > 0; off >>= 1) tr += __shfl_down(tr, off);
    if (lane == 0) red[w] = tr;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < 8; ++i) t += red[i];
        part[(long long)chunk * STRIDE + 2 * HPT * HPT + qa] = t;
    }
}

// the shares summed in a fixed order into st: GB[a][b] = (sum_c C_c[a][b] + sum_c C_c[b][a]) / 2 (every sum in chunk order, so GB is
// exactly symmetric), GD likewise, GX[0] = sum A o P.  Workgroup: 64 share positions (register order) x 4 chunk groups (group g sums
// chunks g, g + 4, ... in that order), each position together with its transposed one; the group sums added in group order.  A
// thread requests all of its group's values of both positions (and the workgroup the stop flag) before its first add: 8, 16 or 32
// chunks deep, the smallest that holds the group (gram_prepare plans at most 128 chunks; more would take further rounds).  Requests
// past the last chunk are clamped to it and their values left out of the sums.
constexpr int GRED_E = 64, GRED_G = 4;
template <int DP>
__device__ __forceinline__ void gred_round(const double* __restrict__ part, int k, int nchunk, long long stride, long long i0,
                                           long long i1, double& s0, double& s1) {
    double v0[DP], v1[DP];
#pragma unroll
    for (int u = 0; u < DP; ++u) {
        const long long o = (long long)min(k + u * GRED_G, nchunk - 1) * stride;
        v0[u] = part[o + i0];
        v1[u] = part[o + i1];
    }
    __builtin_amdgcn_sched_barrier(0);                            // no add is moved up among the loads
#pragma unroll
    for (int u = 0; u < DP; ++u)
        if (k + u * GRED_G < nchunk) { s0 += v0[u]; s1 += v1[u]; }
}
// HPT > HP: the blocked shares of gram_tail_kernel<HP, HPT>.  Position e lies in block (qa, qb) of its product; its transposed
// position lies in block (qb, qa), at the transposed place of HP's register order.  The NQ trace slots are added in slot order.
template <int HP, int HPT = HP>
__global__ __launch_bounds__(256) void gram_part_reduce_kernel(const double* __restrict__ part, int nchunk, double* __restrict__ st,
                                                               StateLayout lay, const int* __restrict__ stop) {
    const int stopv = *stop;
    constexpr int V = GPart<HP>::V, n2 = HPT * HPT, nb = HP * HP, NQ = GPartBlk<HP, HPT>::NQ;
    constexpr bool BLK = NQ > 1;
    static_assert(NQ <= 2, "gram_part_reduce: two trace slots");
    constexpr long long stride = GPartBlk<HP, HPT>::STRIDE;
    __shared__ double sum[2][GRED_G][GRED_E];
    const int el = threadIdx.x % GRED_E, g = threadIdx.x / GRED_E;
    const int e = blockIdx.x * GRED_E + el;                       // < 2 n2 + GRED_E; e == 2 n2: the trace
    // e = pi n2 + register-order index ((tw V + t) 4 + rq) 64 + 16 q + c  <->  C[a][b], a = V (q + 4 rq) + tw, b = V c + t
    const int pi = e / n2, blk = BLK ? (e % n2) / nb : 0, x = BLK ? e % nb : e % n2;
    const int qa = blk / NQ, qb = blk % NQ;
    const int tw = (x >> 8) / V, t = (x >> 8) % V, rq = (x >> 6) & 3, q = (x >> 4) & 3, c = x & 15;
    const int al = V * (q + 4 * rq) + tw, bl = V * c + t;
    const int a = qa * HP + al, b = qb * HP + bl;
    const bool mat = e < 2 * n2, tro = e == 2 * n2;
    const long long i0 = mat ? e : 2LL * n2;
    const long long i1 = mat ? (long long)pi * n2 + (qb * NQ + qa) * nb + gpart_index<HP>(bl, al) : 2LL * n2 + (BLK ? 1 : 0);
    double s0 = 0.0, s1 = 0.0;
    for (int k = g; k < nchunk; k += 32 * GRED_G) {
        const int left = (nchunk - k + GRED_G - 1) / GRED_G;     // the same for the whole wave
        if (left <= 8) gred_round<8>(part, k, nchunk, stride, i0, i1, s0, s1);
        else if (left <= 16) gred_round<16>(part, k, nchunk, stride, i0, i1, s0, s1);
        else gred_round<32>(part, k, nchunk, stride, i0, i1, s0, s1);
    }
    if (stopv) return;
    sum[0][g][el] = s0;
    sum[1][g][el] = s1;
    __syncthreads();
    if (g != 0 || !(mat || tro)) return;
    double t0 = 0.0, t1 = 0.0;
    for (int k = 0; k < GRED_G; ++k) { t0 += sum[0][k][el]; t1 += sum[1][k][el]; }
    if (tro) st[lay.GX()] = BLK ? t0 + t1 : t0;
    else st[(pi ? lay.GD() : lay.GB()) + a * HPT + b] = 0.5 * (t0 + t1);
}

}  // namespace vbmf
