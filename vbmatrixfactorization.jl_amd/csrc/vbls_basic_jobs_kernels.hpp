// vbls_basic_jobs_kernels.hpp -- vbls! of the basic model (examples/mil_util.jl:182-185: niter x (updateA!, updateCA!, updateSigma2!), B
// frozen) for a list of (bag, model) jobs, every model with its own fp64 basis and its own rank, and each job's norm(Y_b - BHat_k AHat_j')^2
// (vbmf_fixed_basis_jobs: the "vbls" classifier of examples/mil_util.jl:469-479 for every fold's test bags in one call).
//
// The context supplies Y only (bags side by side, bag b = columns col_off[b] .. col_off[b+1]-1); nothing of its state is read.  The
// models' part is vbls_jobs_model_kernel's (vbls_jobs_kernels.hpp, no bound requested): Bt = B row-major and G = B'B + L SigmaB.
//   vbls_basic_jobs_kernel  one workgroup of 256 threads per job of one 16-block tier of H_k -- workgroup w runs job idx[w] --, everything
//                           fp64 with Y widened on load from Y as stored (score_y_at):
//                             1. P = Y_b'B_k and ||Y_b||^2 (vjobs_product: the ARD jobs' function)
//                             2. S = P'P (fjobs_gram): entry (i, j) is a plain fma chain over the columns m = s, s + NS, ... of each of
//                                NS = 256 / H^2 stripes (one chain over all of them once H^2 > 128), the stripes' shares added in stripe
//                                order; a * b commutes, so S is symmetric bit for bit
//                             3. the whole loop as H x H algebra on S (vbls_loop_dev, ctrl_kernels.hpp: the function of the one-basis
//                                entries), K0 = G_k, from sigma2 = sigma0[k] and CA = ca0[k] I, every image in LDS
//                             4. A = P T with T = SigmaA / sigma2 of the last updateA!
//                             5. r2 = ||Y_b - B_k A'||^2 entry by entry -- not the trace form (score_kernels.hpp's header says why)
//                           The job's P (M_b H doubles) lives in LDS behind the fixed part when fjobs_in_lds says so, else in the job's
//                           slice of the call's scratch.  The fixed part is first the staging area of step 1, then the stripes' shares and
//                           S of step 2, then the loop's four images, then T.
// Every sum's order is fixed by (L, M_b, H); no workgroup waits for another and nothing is shared between jobs but read-only input, so
// a job's numbers do not depend on the other jobs of the call, on their order or tier, or on where the bag sits in Y.  A job that meets
// a pivot that is not positive and finite (or ends with a non-finite sigma2, CA or r2) gets status = 1 and NaN in every output.
#pragma once
#include "common.hpp"
#include "ctrl_kernels.hpp"
#include "score_kernels.hpp"
#include "vbls_jobs_kernels.hpp"

namespace vbmf {

constexpr int FJOBS_THREADS = 256;
static_assert(FJOBS_THREADS == SCORE_THREADS, "one workgroup size for the product and the loop");

// doubles of dynamic LDS in front of a job's P: the loop's four images or the product's staging area, whichever is larger
__host__ __device__ constexpr int fjobs_image_doubles(int NBK) { return (16 * NBK) * (16 * NBK + 2); }
__host__ __device__ constexpr int fjobs_fixed_doubles(int NBK) {
    return 4 * fjobs_image_doubles(NBK) > VJOBS_STAGE ? 4 * fjobs_image_doubles(NBK) : VJOBS_STAGE;
}
// the placement rule: a job of Mb columns keeps its P in LDS (the host sizes LDS and scratch by it, the kernel places by it)
__host__ __device__ constexpr bool fjobs_in_lds(int NBK, int H, long long Mb) {
    return Mb * H <= (long long)(VJOBS_LDS / sizeof(double)) - fjobs_fixed_doubles(NBK);
}
static_assert(vbls_lds_bytes(1) == 4 * fjobs_image_doubles(1) * sizeof(double) && vbls_lds_bytes(2) == 4 * fjobs_image_doubles(2) * sizeof(double),
              "the loop's images");
static_assert(FJOBS_THREADS <= 3 * fjobs_image_doubles(1), "the stripes' shares stand in front of S");
static_assert(VJOBS_MAX_H <= 32, "two 16-block tiers");

struct FjobsArgs {
    const uint4* Y2; int KSpad; long long L;
    const long long* col_off;
    // per job: job_off[j] = the doubles of the M_b H_k-long blocks of the jobs before j, job_sa[j] the same of their H_k^2 blocks,
    // job_h[j] of their H_k-long ones.  idx: the jobs of this launch (workgroup w runs job idx[w])
    const long long* job_bag; const long long* job_model; const long long* job_off; const long long* job_sa; const long long* job_h;
    const long long* idx;
    VjobsModels ms;
    int niter;
    // per model: Bt L H, G H^2, sigma0, ca0 one each
    const double* Bt; const double* G; const double* sigma0; const double* ca0;
    // per job: A M_b x H_k column-major at job_off[j]; SA and T H^2 at job_sa[j]; ca H at job_h[j]; sigma, r2 one each.
    // Pd: P of the jobs that do not keep it in LDS, at job_off[j]
    double* Pd; double* A; double* SA; double* T; double* ca; double* sigma; double* r2;
    long long* status;
};

struct FjobsK0 {                                        // K0 of the loop: the model's G = B'B + L SigmaB (H x H, ld H)
    const double* G; int H;
    __device__ __forceinline__ double operator()(int i, int j) const { return G[i * H + j]; }
};

// S = P'P (H x H, ld H) from Pb[m * H + h].  zp: FJOBS_THREADS doubles of LDS, apart from S.  Every thread of the workgroup calls it;
// it ends behind a barrier.
__device__ __forceinline__ void fjobs_gram(const double* Pb, int H, long long Mb, double* S, double* zp) {
    const int tid = threadIdx.x, E = H * H;
    if (2 * E <= FJOBS_THREADS) {
        const int NS = FJOBS_THREADS / E;
        const int o = tid < E * NS ? tid % E : -1, s = tid / E;
        if (o >= 0) {
            const int i = o / H, j = o % H;
            double acc = 0.0;
            for (long long m = s; m < Mb; m += NS) acc = fma(Pb[m * H + i], Pb[m * H + j], acc);
            zp[s * E + o] = acc;
        }
        __syncthreads();
        for (int e = tid; e < E; e += FJOBS_THREADS) {
            double z = 0.0;
            for (int i = 0; i < NS; ++i) z += zp[i * E + e];
            S[e] = z;
        }
    } else {
        for (int e = tid; e < E; e += FJOBS_THREADS) {
            const int i = e / H, j = e % H;
            double acc = 0.0;
            for (long long m = 0; m < Mb; ++m) acc = fma(Pb[m * H + i], Pb[m * H + j], acc);
            S[e] = acc;
        }
    }
    __syncthreads();
}

template <int MODE, int NBK>
__global__ __launch_bounds__(FJOBS_THREADS) void vbls_basic_jobs_kernel(FjobsArgs g) {
    extern __shared__ __attribute__((aligned(16))) double lds_fj[];
    __shared__ double red[16];
    __shared__ double ca_o[16 * NBK];
    __shared__ double sig_o;
    __shared__ int bad_s;
    const int j = (int)g.idx[blockIdx.x], tid = threadIdx.x;
    const int b = (int)g.job_bag[j], k = (int)g.job_model[j];
    const int H = (int)g.ms.Hs[k];
    const long long ko = g.ms.k_off[k];
    const long long m0 = g.col_off[b], Mb = g.col_off[b + 1] - m0;
    const long long n = Mb * H, o = g.job_off[j], so = g.job_sa[j], jh = g.job_h[j];
    double* Pb = fjobs_in_lds(NBK, H, Mb) ? lds_fj + fjobs_fixed_doubles(NBK) : g.Pd + o;
    const double* Bt = g.Bt + g.ms.b_off[k];
    if (tid == 0) {
        bad_s = 0;
        sig_o = g.sigma0[k];
    }
    if (tid < 16 * NBK) ca_o[tid] = g.ca0[k];
    double yy = vjobs_product<MODE>(g.Y2, g.KSpad, g.L, Bt, H, m0, Mb, Pb, lds_fj);
    yy = block_sum(yy, red);                           // (its barriers end the product's use of the staging area and publish sig_o, ca_o)
    double* Sg = lds_fj + 3 * fjobs_image_doubles(NBK);         // where the loop's fourth image will stand: read before that is written
    fjobs_gram(Pb, H, Mb, Sg, lds_fj);
    const VblsBag q{Sg, H, yy, (double)Mb, &sig_o, ca_o, g.SA + so, H, H, nullptr, g.T + so, nullptr};
    int bad = vbls_loop_dev<NBK>(FjobsK0{g.G + ko, H}, H, (double)g.L, g.niter, q, lds_fj);
    __syncthreads();                                   // (sig_o, ca_o and the job's T as the last iteration left them; the images are free)
    double* Tl = lds_fj;
    for (int t = tid; t < H * H; t += FJOBS_THREADS) Tl[t] = g.T[so + t];
    __syncthreads();
    double* Ab = g.A + o;                              // M_b x H column-major
    for (long long t = tid; t < n; t += FJOBS_THREADS) {
        const long long m = t / H;
        const int h = (int)(t - m * H);
        const double* pm = Pb + m * H;
        double a = 0.0;
        for (int c = 0; c < H; ++c) a = fma(pm[c], Tl[c * H + h], a);
        Ab[(long long)h * Mb + m] = a;
    }
    __syncthreads();                                   // (Ab for every thread)
    double r2 = 0.0;
    const long long ny = Mb * g.L;
    for (long long t = tid; t < ny; t += FJOBS_THREADS) {
        const long long m = t / g.L, l = t - m * g.L;
        const double* brow = Bt + l * H;
        double pred = 0.0;
        for (int h = 0; h < H; ++h) pred += brow[h] * Ab[(long long)h * Mb + m];
        const double d = (double)score_y_at<MODE>(g.Y2, g.KSpad, l, m0 + m) - pred;
        r2 += d * d;
    }
    r2 = block_sum(r2, red);
    const double sig = sig_o;
    bad |= !isfinite(sig) || !isfinite(r2);
    if (tid < H) bad |= !isfinite(ca_o[tid]);
    if (bad) bad_s = 1;                                // (same value from every writer)
    __syncthreads();
    const bool failed = bad_s != 0;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    if (failed) {
        for (long long t = tid; t < n; t += FJOBS_THREADS) Ab[t] = nan;
        for (int t = tid; t < H * H; t += FJOBS_THREADS) g.SA[so + t] = nan;
    }
    if (tid < H) g.ca[jh + tid] = failed ? nan : ca_o[tid];
    if (tid == 0) {
        g.sigma[j] = failed ? nan : sig;
        g.r2[j] = failed ? nan : r2;
        g.status[j] = failed ? 1 : 0;
    }
}

}  // namespace vbmf
