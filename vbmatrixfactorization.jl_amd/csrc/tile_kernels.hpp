// tile_kernels.hpp -- build the two MFMA-fragment-tiled device copies of Y, and read Y back.
//
// Tiled format ("Y tiles"): a fragment is the 16 bytes one lane feeds to one MFMA as the B operand;
// 64 lanes = 1 KiB = one tile of 32 x-columns by one k-step (16 k in bf16, 8 k in f32).  Tiles are
// stored [x-tile][k-step][lane], so a wave that walks the contraction reads one contiguous stream
// with fully coalesced 1 KiB wave-loads.  Two copies exist because the two passes contract over
// different indices (288 GB of HBM make the second copy free; neither pass re-reads the other's):
//     pass 1  P = Y'B :  x = column m, k = row l      (Y1)
//     pass 2  Q = Y A :  x = row l,    k = column m   (Y2)
#pragma once
#include "common.hpp"
#include "rng.hpp"

namespace vbmf {

// source functors: value of Y at (local row l, column m); rows/cols out of range are zero padding
struct ColMajorF64Src {
    const double* buf; long long ld; long long m0, mc;   // staging chunk: columns [m0, m0+mc)
    long long L, M;
    __device__ __forceinline__ double operator()(long long l, long long m) const {
        if (l >= L || m >= M) return 0.0;
        return buf[(m - m0) * ld + l];
    }
};
struct SynthSrc {
    SynthGen g; long long L, M, row_offset;
    __device__ __forceinline__ double operator()(long long l, long long m) const {
        if (l >= L || m >= M) return 0.0;
        return (double)g(l + row_offset, m);
    }
};

// A block of rows in the caller's own dtype and layout (vbmf_set_Y_rows): local row l, column m at buf[(l - row0) * rs + m * cs],
// strides in elements, rows [row0, row1) present.  The block ends at L or at a multiple of 32, so the tiles it owns never ask for a
// row of another block; anything outside it reads as zero padding and is never fetched.
__device__ __forceinline__ double src_f64(double v) { return v; }
__device__ __forceinline__ double src_f64(float v) { return (double)v; }
__device__ __forceinline__ double src_f64(__bf16 v) { return (double)bf2f(__builtin_bit_cast(unsigned short, v)); }
template <class T>
struct StridedSrc {
    const T* buf; long long rs, cs;
    long long row0, row1, M;
    __device__ __forceinline__ double operator()(long long l, long long m) const {
        if (l < row0 || l >= row1 || m >= M) return 0.0;
        return src_f64(buf[(l - row0) * rs + m * cs]);
    }
};

// Columns of ANOTHER context's Y (vbmf_set_Y_gather): column m of the Y being built is column idx[m] of the source, decoded from the
// source's pass-2 copy (x = l, k = column) with untile_y_kernel's index arithmetic.  f32 names the storage type both contexts share, so
// the value is on the storage grid already and tile_y_kernel's one rounding returns it unchanged.  The host has checked every idx
// against the source's M and both contexts have one L: the fragment read lies inside the source's copy.  KS: k-steps per x tile there.
struct GatherSrc {
    const uint4* Y2; const int* idx; int KS; bool f32;
    long long L, M;
    __device__ __forceinline__ double operator()(long long l, long long m) const {
        const int KSTEP = f32 ? 8 : 16;
        if (l >= L || m >= M) return 0.0;
        const int j = idx[m];
        const int xt = (int)(l >> 5), c = (int)(l & 31);
        const int ks = j / KSTEP, w = j % KSTEP;
        int half, e;
        if (f32) { half = w >> 2; e = w & 3; }
        else { half = (w >> 2) & 1; e = 4 * (w >> 3) + (w & 3); }
        const unsigned* f = reinterpret_cast<const unsigned*>(Y2 + ((long long)xt * KS + ks) * 64 + half * 32 + c);
        if (f32) return (double)bitsf(f[e]);
        return (double)bf2f((unsigned short)((f[e >> 1] >> (16 * (e & 1))) & 0xFFFFu));
    }
};

// One thread = one 16-byte fragment.  TRANSPOSED=false: x=m,k=l (Y1); true: x=l,k=m (Y2).
// Fragments in [xt0,xt1) x [ks0,ks1) are produced.  When sumsq != nullptr each block writes the fp64 sum of
// its squared stored values to sumsq[blockIdx.x] -- done on exactly one of the two copies.
template <int MODE, bool TRANSPOSED, class Src>
__global__ __launch_bounds__(256) void tile_y_kernel(uint4* __restrict__ out, Src src, int xt0, int xt1, int ks0,
                                                     int ks1, int KSpad, double* sumsq) {
    constexpr int KSTEP = (MODE == MODE_F32) ? 8 : 16;
    constexpr int NE = (MODE == MODE_F32) ? 4 : 8;
    const long long nks = ks1 - ks0;
    const long long total = (long long)(xt1 - xt0) * nks * 64;
    double acc = 0.0;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (long long)gridDim.x * blockDim.x) {
        const int lane = (int)(t & 63);
        const long long q = t >> 6;
        const int ks = ks0 + (int)(q % nks);
        const int xt = xt0 + (int)(q / nks);
        const int c = lane & 31, half = lane >> 5;
        const long long x = (long long)xt * 32 + c;
        // values are rounded ONCE, from the source's fp64, to the device dtype (round-to-nearest-even)
        double v[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const long long k = (long long)ks * KSTEP + kperm(MODE, half, e);
            v[e] = TRANSPOSED ? src(x, k) : src(k, x);
        }
        uint4 o;
        if (MODE == MODE_F32) {
            float f[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) { f[e] = (float)v[e]; acc += (double)f[e] * (double)f[e]; }
            o.x = fbits(f[0]); o.y = fbits(f[1]); o.z = fbits(f[2]); o.w = fbits(f[3]);
        } else {
            unsigned short b[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const __bf16 q = (__bf16)v[e];
                b[e] = __builtin_bit_cast(unsigned short, q);
                const float r = bf2f(b[e]);
                acc += (double)r * (double)r;
            }
            o.x = b[0] | ((unsigned)b[1] << 16); o.y = b[2] | ((unsigned)b[3] << 16);
            o.z = b[4] | ((unsigned)b[5] << 16); o.w = b[6] | ((unsigned)b[7] << 16);
        }
        out[((long long)xt * KSpad + ks) * 64 + lane] = o;
    }
    if (sumsq) {                                  // one partial per block, summed later in a fixed order
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
        __shared__ double part[4];
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0) sumsq[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
    }
}

// ---- both copies from ONE read of a source with a unit stride (vbmf_set_Y_rows) --------------------------------------------------
// A workgroup takes a block of 32 (dimension s, any stride) x 128 (dimension u, unit stride) source values -- s = row, u = column for a
// row-major source; s = column, u = row for a column-major one -- loads it coalesced along u, rounds every value once to the storage
// type exactly as tile_y_kernel does, and keeps the rounded values as fp32 in LDS (a bf16 value is an fp32 with a zero low half).  It
// then writes the fragments of both copies from LDS with 16-byte stores:
//     copy A  x along s, k along u: one x tile, 128 / KSTEP k-steps; a lane's elements are 4 consecutive u (one or two 16-byte LDS reads)
//     copy B  x along u, k along s: four x tiles, 32 / KSTEP k-steps; a lane's elements are NE single reads, lanes along u
// Rows are PAIR_PITCH = 132 floats apart: 16-byte aligned, and the 16 lanes of a 16-byte read (16 consecutive s) fall on 16 different
// 16-byte slots of the 256-byte bank row (132 / 4 = 33 = 1 mod 16); the single reads and all writes run along u and have no conflict.
// The blocks also cover the padding of both copies (zeros, never fetched); each copy's own tile / k-step ranges decide what is stored.
struct PairGeom {
    long long ss;                          // source stride along s, in elements
    long long s_org, u_org;                // source element 0 is (s_org, u_org)
    long long s_lo, s_hi, u_lo, u_hi;      // the source holds [s_lo, s_hi) x [u_lo, u_hi); everything else is zero padding
    long long s0, u0;                      // origin of block (0, 0): multiples of 32
    int ns, nu;                            // blocks along s and along u
    int xa0, xa1, ka0, ka1, KSA;           // copy A: x tiles and k-steps this call owns, k-steps per x tile of the buffer
    int xb0, xb1, kb0, kb1, KSB;           // copy B
};
constexpr int PAIR_U = 128, PAIR_PITCH = PAIR_U + 4;

template <int MODE, class T>
__global__ __launch_bounds__(256) void tile_pair_kernel(uint4* __restrict__ outA, uint4* __restrict__ outB, const T* __restrict__ src,
                                                        PairGeom g, double* sumsq) {
    constexpr int KSTEP = (MODE == MODE_F32) ? 8 : 16;
    constexpr int NE = (MODE == MODE_F32) ? 4 : 8;
    constexpr int KA = PAIR_U / KSTEP, KB = 32 / KSTEP;
    __shared__ __attribute__((aligned(16))) float S[32 * PAIR_PITCH];
    const int t = threadIdx.x;
    const long long nblk = (long long)g.ns * g.nu;
    double acc = 0.0;
    for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const long long sb = g.s0 + (blk / g.nu) * 32, ub = g.u0 + (blk % g.nu) * PAIR_U;
#pragma unroll
        for (int i = 0; i < 32 * PAIR_U / 256; ++i) {
            const int idx = t + 256 * i, u = idx & (PAIR_U - 1), s = idx / PAIR_U;
            const long long sg = sb + s, ug = ub + u;
            float r = 0.0f;
            if (sg >= g.s_lo && sg < g.s_hi && ug >= g.u_lo && ug < g.u_hi) {
                // rounded ONCE, from the source's fp64, to the device dtype (round-to-nearest-even), as in tile_y_kernel
                const double v = src_f64(src[(sg - g.s_org) * g.ss + (ug - g.u_org)]);
                if (MODE == MODE_F32) r = (float)v;
                else { const __bf16 q = (__bf16)v; r = bf2f(__builtin_bit_cast(unsigned short, q)); }
                acc += (double)r * (double)r;
            }
            S[s * PAIR_PITCH + u] = r;
        }
        __syncthreads();
        const int xtA = (int)(sb >> 5);
        if (xtA >= g.xa0 && xtA < g.xa1) {
            for (int f = t; f < KA * 64; f += 256) {
                const int lane = f & 63, ksl = f >> 6, c = lane & 31, half = lane >> 5;
                const int ks = (int)(ub / KSTEP) + ksl;
                if (ks < g.ka0 || ks >= g.ka1) continue;
                const float* row = S + c * PAIR_PITCH + ksl * KSTEP + 4 * half;
                const float4 a = *reinterpret_cast<const float4*>(row);
                uint4 o;
                if (MODE == MODE_F32) { o.x = fbits(a.x); o.y = fbits(a.y); o.z = fbits(a.z); o.w = fbits(a.w); }
                else {
                    const float4 b = *reinterpret_cast<const float4*>(row + 8);
                    o.x = (fbits(a.x) >> 16) | (fbits(a.y) & 0xFFFF0000u); o.y = (fbits(a.z) >> 16) | (fbits(a.w) & 0xFFFF0000u);
                    o.z = (fbits(b.x) >> 16) | (fbits(b.y) & 0xFFFF0000u); o.w = (fbits(b.z) >> 16) | (fbits(b.w) & 0xFFFF0000u);
                }
                outA[((long long)xtA * g.KSA + ks) * 64 + lane] = o;
            }
        }
        for (int f = t; f < 4 * KB * 64; f += 256) {
            const int lane = f & 63, q = f >> 6, ksl = q % KB, xtl = q / KB, c = lane & 31, half = lane >> 5;
            const int xt = (int)(ub >> 5) + xtl, ks = (int)(sb / KSTEP) + ksl;
            if (xt < g.xb0 || xt >= g.xb1 || ks < g.kb0 || ks >= g.kb1) continue;
            unsigned w[NE];
#pragma unroll
            for (int e = 0; e < NE; ++e) w[e] = fbits(S[(ksl * KSTEP + kperm(MODE, half, e)) * PAIR_PITCH + xtl * 32 + c]);
            uint4 o;
            if (MODE == MODE_F32) { o.x = w[0]; o.y = w[1]; o.z = w[2]; o.w = w[3]; }
            else {
                o.x = (w[0] >> 16) | (w[1] & 0xFFFF0000u); o.y = (w[2] >> 16) | (w[3] & 0xFFFF0000u);
                o.z = (w[NE - 4] >> 16) | (w[NE - 3] & 0xFFFF0000u); o.w = (w[NE - 2] >> 16) | (w[NE - 1] & 0xFFFF0000u);
            }
            outB[((long long)xt * g.KSB + ks) * 64 + lane] = o;
        }
        __syncthreads();
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);   // one partial per workgroup, summed later in a fixed order
    __shared__ double part[4];
    if ((t & 63) == 0) part[t >> 6] = acc;
    __syncthreads();
    if (t == 0) sumsq[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// *dst += sum(partials[0..n)) in a fixed order (run-to-run reproducible ||Y||^2)
__global__ __launch_bounds__(256) void sum_partials_kernel(const double* __restrict__ partials, int n,
                                                           double* __restrict__ dst) {
    __shared__ double sh[256];
    double a = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) a += partials[i];
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) *dst += sh[0];
}

// Decode the pass-2 copy (x = l, k = m) back to column-major fp64: out[(l-row0) + m*ld].
template <int MODE>
__global__ __launch_bounds__(256) void untile_y_kernel(const uint4* __restrict__ Y2, double* __restrict__ out,
                                                       long long ld, long long row0, long long nrows, long long M,
                                                       int KSpad) {
    constexpr int KSTEP = (MODE == MODE_F32) ? 8 : 16;
    const long long total = nrows * M;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (long long)gridDim.x * blockDim.x) {
        const long long li = t % nrows, m = t / nrows;
        const long long l = row0 + li;
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
        out[li + m * ld] = (double)v;
    }
}

}  // namespace vbmf
