// out_kernels.hpp -- results into the caller's memory (vbmf_get_YHat_rows, vbmf_get_factor_rows; updateYHat!, src/vbmf.jl:120-122;
// DESIGN.md section 17): the mirror of tile_kernels.hpp's ingestion.
//
//   yhat_out_kernel<ACC, DST, RESID, YMODE>   C[x, y] = sum_h X[x, h] Yf[y, h]  (or Y[l, m] - that), one 128 x 128 output tile per
//       256-thread workgroup, written ONCE as dst[x sx + y sy] and never read back: a write-bound GEMM with K = Hp <= 256.
//       X and Yf are the fp32 factors as stored ([rows][Hp] row-major: A32, B32[bcur]).  The lanes of an MFMA result own columns, so
//       the host makes the factor of the dst's unit-stride dimension the y side (row-major dst: x = l, y = m; column-major: x = m,
//       y = l) and the 32 / 16 lanes of one stored register cover 128 contiguous bytes of fp32 / fp64.  A product is commutative bit
//       for bit and both roles run the same k order from a zero accumulator, so an entry is the same bits whichever side it sits on,
//       wherever its tile starts and whatever the strides are.
//         ACC = float    v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain of exact fp32 products (one rounding per term); a wave owns
//                        64 x 64 = 2 x 2 blocks, four independent accumulators
//         ACC = double   v_mfma_f64_16x16x4_f64 on the widened factors; a wave owns 64 x 64 = 4 x 4 blocks
//       Columns h >= H of a panel are zeroed on their way into LDS (the stored pads are never trusted), rows past the end too.
//       RESID: fl(y - s) in ACC, y = Y[l, m] as stored, read from the pass-2 tiles (out_y_at: score_y_at's element, one word).  DST = bf16 rounds the fp32 value
//       to nearest even, so it is bitwise the rounding of the fp32 output.  Every store is guarded by x < X, y < Yn.
//   factor_out_kernel<DST>   dst[x rs + h cs] = convert(F[(row0 + x) Hp + h]): a copy, a widening or one RNE.
#pragma once
#include "common.hpp"
#include "score_kernels.hpp"

namespace vbmf {

constexpr int OUT_TILE = 128;      // output tile edge per workgroup
constexpr int OUT_THREADS = 256;

typedef float out_f32x16 __attribute__((ext_vector_type(16)));
typedef double out_f64x4 __attribute__((ext_vector_type(4)));

struct out_bf16 { unsigned short v; };

template <class ACC> struct OutMma;
template <> struct OutMma<float> {
    static constexpr int BS = 32, KK = 2, NB = 2, NR = 16, KC = 32;   // block edge, k per MFMA, blocks per wave side, registers, k per LDS chunk
    typedef out_f32x16 acc_t;
    static __device__ __forceinline__ int row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }
    static __device__ __forceinline__ acc_t mma(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
};
template <> struct OutMma<double> {
    static constexpr int BS = 16, KK = 4, NB = 4, NR = 4, KC = 16;
    typedef out_f64x4 acc_t;
    static __device__ __forceinline__ int row(int r, int lane) { return (lane >> 4) + 4 * r; }
    static __device__ __forceinline__ acc_t mma(double a, double b, acc_t c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
};
template <class ACC> constexpr int out_lds_stride() { return OutMma<ACC>::KC + 1; }
template <class ACC> constexpr size_t out_lds_bytes() { return 2 * (size_t)OUT_TILE * out_lds_stride<ACC>() * sizeof(ACC); }

template <class DST, class ACC> struct OutStore;
template <class ACC> struct OutStore<double, ACC> {
    static __device__ __forceinline__ void put(double* p, ACC v) { *p = (double)v; }
};
template <class ACC> struct OutStore<float, ACC> {
    static __device__ __forceinline__ void put(float* p, ACC v) { *p = (float)v; }
};
template <class ACC> struct OutStore<out_bf16, ACC> {
    static __device__ __forceinline__ void put(out_bf16* p, ACC v) { p->v = f2bf((float)v); }
};

// Y[l, m] as stored, from the pass-2 tiles: score_y_at's element, read as the ONE 32-bit word that holds it (a lane of the epilogue
// wants one value of a fragment, not its 16 bytes)
template <int MODE>
__device__ __forceinline__ float out_y_at(const unsigned* __restrict__ Yw, long long tile_words, long long l, long long m) {
    constexpr int KSTEP = (MODE == MODE_F32) ? 8 : 16;
    const int ks = (int)(m / KSTEP), wi = (int)(m % KSTEP);
    int half, e;
    if (MODE == MODE_F32) { half = wi >> 2; e = wi & 3; }
    else { half = (wi >> 2) & 1; e = 4 * (wi >> 3) + (wi & 3); }
    const long long frag = (l >> 5) * tile_words + ((long long)ks * 64 + half * 32 + (int)(l & 31)) * 4;
    if (MODE == MODE_F32) return bitsf(Yw[frag + e]);
    return bf2f((unsigned short)((Yw[frag + (e >> 1)] >> (16 * (e & 1))) & 0xFFFFu));
}

// one [128][KC] panel of a factor: rows x0 .. x0+127 (zero past X), columns k0 .. k0+KC-1 (zero from H on).  Fetched into registers
// and written to LDS in two steps, so that the next chunk's loads are in flight under this chunk's MFMAs.
template <class ACC> constexpr int out_panel_vecs() { return OUT_TILE * (OutMma<ACC>::KC / 4) / OUT_THREADS; }
template <class ACC>
__device__ __forceinline__ void out_fetch_panel(float4 (&v)[out_panel_vecs<ACC>()], const float* __restrict__ F, int Hp, int H, long long X,
                                                long long x0, int k0) {
    constexpr int V = OutMma<ACC>::KC / 4;                         // float4 per row
#pragma unroll
    for (int t = 0; t < out_panel_vecs<ACC>(); ++t) {
        const int i = threadIdx.x + t * OUT_THREADS, r = i / V, k = k0 + 4 * (i % V);
        v[t] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (x0 + r < X && k < H) v[t] = *reinterpret_cast<const float4*>(F + (x0 + r) * (long long)Hp + k);   // Hp is a multiple of 32 >= H
        if (k + 1 >= H) v[t].y = 0.f;
        if (k + 2 >= H) v[t].z = 0.f;
        if (k + 3 >= H) v[t].w = 0.f;
    }
}
template <class ACC>
__device__ __forceinline__ void out_store_panel(ACC* __restrict__ S, const float4 (&v)[out_panel_vecs<ACC>()]) {
    constexpr int V = OutMma<ACC>::KC / 4, LS = out_lds_stride<ACC>();
#pragma unroll
    for (int t = 0; t < out_panel_vecs<ACC>(); ++t) {
        const int i = threadIdx.x + t * OUT_THREADS;
        ACC* s = S + (i / V) * LS + 4 * (i % V);
        s[0] = (ACC)v[t].x; s[1] = (ACC)v[t].y; s[2] = (ACC)v[t].z; s[3] = (ACC)v[t].w;
    }
}

// swap = 0: x = l, y = m (lanes along m);  swap = 1: x = m, y = l (lanes along l).  ntx * nty workgroups, y tiles fastest.
template <class ACC, class DST, bool RESID, int YMODE>
__global__ __launch_bounds__(OUT_THREADS) void yhat_out_kernel(const float* __restrict__ Xf, const float* __restrict__ Yf, int Hp, int H,
                                                               long long X, long long Yn, long long xrow0, long long yrow0,
                                                               DST* __restrict__ dst, long long sx, long long sy, int nty, int swap,
                                                               const uint4* __restrict__ Y2, int KSpad) {
    typedef OutMma<ACC> MM;
    constexpr int BS = MM::BS, KK = MM::KK, NB = MM::NB, NR = MM::NR, KC = MM::KC, LS = out_lds_stride<ACC>();
    extern __shared__ __attribute__((aligned(16))) unsigned char out_lds_raw[];
    ACC* Xs = reinterpret_cast<ACC*>(out_lds_raw);
    ACC* Ys = Xs + OUT_TILE * LS;
    const long long x0 = (long long)(blockIdx.x / nty) * OUT_TILE, y0 = (long long)(blockIdx.x % nty) * OUT_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wx = (wave >> 1) * 64, wy = (wave & 1) * 64;
    const int li = lane % BS, lk = lane / BS;                      // operand row / column and k inside one MFMA
    typename MM::acc_t acc[NB][NB];
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int r = 0; r < NR; ++r) acc[i][j][r] = (ACC)0;
    float4 px[out_panel_vecs<ACC>()], py[out_panel_vecs<ACC>()];
    out_fetch_panel<ACC>(px, Xf, Hp, H, xrow0 + X, xrow0 + x0, 0);
    out_fetch_panel<ACC>(py, Yf, Hp, H, yrow0 + Yn, yrow0 + y0, 0);
    for (int k0 = 0; k0 < H; k0 += KC) {
        __syncthreads();                                           // every wave has read the chunk before
        out_store_panel<ACC>(Xs, px);
        out_store_panel<ACC>(Ys, py);
        __syncthreads();
        if (k0 + KC < H) {
            out_fetch_panel<ACC>(px, Xf, Hp, H, xrow0 + X, xrow0 + x0, k0 + KC);
            out_fetch_panel<ACC>(py, Yf, Hp, H, yrow0 + Yn, yrow0 + y0, k0 + KC);
        }
#pragma unroll
        for (int kk = 0; kk < KC; kk += KK) {
            ACC a[NB], b[NB];
#pragma unroll
            for (int i = 0; i < NB; ++i) a[i] = Xs[(wx + i * BS + li) * LS + kk + lk];
#pragma unroll
            for (int j = 0; j < NB; ++j) b[j] = Ys[(wy + j * BS + li) * LS + kk + lk];
#pragma unroll
            for (int i = 0; i < NB; ++i)
#pragma unroll
                for (int j = 0; j < NB; ++j) acc[i][j] = MM::mma(a[i], b[j], acc[i][j]);
        }
    }
    // a lane's results: column y = ylane + j BS, rows x = xlane + i BS + row(r, 0); one 64-bit address per lane, the rest are uniform steps
    const long long xlane = x0 + wx + MM::row(0, lane), ylane = y0 + wy + li;
    DST* const plane = dst + xlane * sx + ylane * sy;
    const bool whole = x0 + OUT_TILE <= X && y0 + OUT_TILE <= Yn;  // uniform: an inner tile stores without looking
    const unsigned* Yw = reinterpret_cast<const unsigned*>(Y2);
    const long long tile_words = (long long)KSpad * 256;           // 32 rows of the pass-2 copy: KSpad fragments of 64 x 16 bytes
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const long long y = ylane + j * BS;
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const int dx = i * BS + MM::row(r, 0);
                const long long x = xlane + dx;
                if (whole || (x < X && y < Yn)) {
                    ACC v = acc[i][j][r];
                    if (RESID) {
                        const long long l = swap ? yrow0 + y : xrow0 + x, m = swap ? xrow0 + x : yrow0 + y;
                        v = (ACC)out_y_at<YMODE>(Yw, tile_words, l, m) - v;
                    }
                    OutStore<DST, ACC>::put(plane + dx * sx + (j * BS) * sy, v);
                }
            }
        }
}

// rows row0 .. row0+n-1 of a factor [.][Hp]; hfast: consecutive threads walk h (col_stride 1), else the rows
template <class DST>
__global__ __launch_bounds__(256) void factor_out_kernel(const float* __restrict__ F, int Hp, int H, long long row0, long long n,
                                                         DST* __restrict__ dst, long long rs, long long cs, int hfast) {
    const long long total = n * H;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long x = hfast ? i / H : i % n;
        const int h = (int)(hfast ? i % H : i / n);
        OutStore<DST, float>::put(dst + x * rs + (long long)h * cs, F[(row0 + x) * Hp + h]);
    }
}

}  // namespace vbmf
