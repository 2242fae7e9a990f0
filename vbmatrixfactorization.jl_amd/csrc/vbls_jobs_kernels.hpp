// vbls_jobs_kernels.hpp -- vbls! of the ARD families for a list of (bag, model) jobs, every model with its own fp64 basis and its own
// rank, and what the bound of each job's fit reads (vbmf_sparse_fixed_basis_jobs: the "dual" classifier of examples/mil_util.jl:515-530
// for every fold's test bags in one call, :187-197 per job; vbmf_sparse_scored_jobs: factorize_bag, :393-416, and lowerBound /
// lowerBoundTrimmed behind it, the "lower_bound" and "min_err" classifiers of :493-514).
//
// The context supplies Y only (bags side by side, bag b = columns col_off[b] .. col_off[b+1]-1); nothing of its state is read.
//   vbls_jobs_model_kernel  one workgroup per model, with the model's own H_k (VjobsModels: the offset tables, as LsBases for the
//                           least-squares jobs): Bt = B row-major [L][H] (what the job kernel reads, coalesced over h), then
//                           G = B'B + L SigmaB, gd = diag(B'B), sd = L diag(SigmaB).  Each entry of B'B is the sum, in chunk order, of
//                           plain fma chains over LS_ROWS rows (ls_gram_chunk's order), so G is symmetric bit for bit.  A scored call also
//                           gets the basis' share of the bound: sum_h CB_h (B'B + L SigmaB)_hh, sum CB, sum log delta (thread 0, in
//                           column order) and log det SigmaB from the pivots of an in-LDS Cholesky (LDL') of the H x H matrix; a pivot
//                           that is not positive gives -inf, which the reference's clamp turns into its floor (src/util.jl:118-122).
//   vbls_jobs_kernel        one workgroup per job of one (16-block tier of H_k, form) group -- workgroup w runs job idx[w] --,
//                           everything fp64 with Y widened on load from Y as stored (score_y_at):
//                             1. P = Y_b'B_k and ||Y_b||^2, SCORE_CW columns at a time with LS_ROWS rows of them staged in LDS
//                                (ls_slice's staged read and its row stripes, whose shares meet in LDS in stripe order)
//                             2. the niter iterations of sparse_batch_kernel (sbatch_iterate: the same __device__ function), from
//                                sigmaHat = sigma0[k], CA = ca0[k] ones, eta = eta0[k] + L M_b / 2
//                             3. r2 = ||Y_b - B_k A'||^2 entry by entry -- not the trace form (score_kernels.hpp's header says why)
//                             4. a scored call: the per-column sums of the bound (lb_column_sums, bag_lb_sums_kernel's function, with
//                                the fp64 mask |a| > trim[j]) and the contractions tr(A'A SigmaB_k), tr(SigmaA_j G_k), while the state
//                                is where the iterations left it; the sums' shares meet in the fixed part of dynamic LDS, free by then
//                           The job's state (P, CA, A, dS: 4 M_b H doubles) lives in LDS behind the fixed part when vjobs_in_lds says
//                           so, else in the job's own slices of the call's buffers.  The fixed part is first the staging area of
//                           step 1, then what sbatch_iterate keeps there (G, or the waves' inverse images).
// Every sum's order is fixed by (L, M_b, H); no workgroup waits for another and nothing is shared between jobs but read-only input,
// so a job's numbers do not depend on the other jobs of the call, on their order or grouping, or on where the bag sits in Y.  A job
// that meets a non-finite precision or a bad pivot (or ends with a non-finite sigmaHat, zeta or r2) gets status = 1 and NaN in every
// output.
#pragma once
#include "common.hpp"
#include "score_kernels.hpp"
#include "sparse_batch_kernels.hpp"

namespace vbmf {

constexpr int VJOBS_MAX_H = 32;                              // the whole-fit entries' cap: two 16-blocks per inverse image
constexpr size_t VJOBS_LDS = SBATCH_LDS_SMALL;               // dynamic LDS per workgroup (64 KiB with the static arrays: two per CU)
constexpr int VJOBS_STAGE = SCORE_CW * LS_ROWS + SBATCH_THREADS;   // step 1: the staged rows of Y | the row stripes' shares
constexpr int VJOBS_NB = 4;                                  // per model: sum CB (B'B + L SigmaB)_hh, sum CB, sum log delta, log det SigmaB
static_assert(SCORE_THREADS * SCORE_NS <= VJOBS_STAGE, "the bound's column sums meet in the fixed part of dynamic LDS");

// doubles of dynamic LDS in front of a job's state
__host__ __device__ constexpr int vjobs_fixed_doubles(bool full, int NBK, int H) {
    return sbatch_fixed_doubles(full, NBK, H) > VJOBS_STAGE ? sbatch_fixed_doubles(full, NBK, H) : VJOBS_STAGE;
}
// the placement rule: a job of Mb columns keeps its state in LDS (the host sizes LDS and scratch by it, the kernel places by it)
__host__ __device__ constexpr bool vjobs_in_lds(bool full, int NBK, int H, long long Mb) {
    return 4 * Mb * H <= (long long)(VJOBS_LDS / sizeof(double)) - vjobs_fixed_doubles(full, NBK, H);
}

// The models of a call: model k has rank Hs[k]; its L x H_k blocks (B, Bt) start at b_off[k] = L * the sum of H_q over q < k, its
// H_k x H_k blocks (SigmaB, G) at k_off[k] = the sum of H_q^2, its H_k-long blocks at h_off[k] = the sum of H_q.
struct VjobsModels {
    const long long* Hs;
    const long long* b_off;
    const long long* k_off;
    const long long* h_off;
};

// One workgroup per model.  B: the models' bases one after the other, column-major L x H_k; SB: H_k x H_k each.
// CB, delta: H_k each and nb: VJOBS_NB per model, or all three nullptr (no bound wanted).
__global__ __launch_bounds__(SCORE_THREADS) void vbls_jobs_model_kernel(VjobsModels ms, const double* __restrict__ B,
                                                                        const double* __restrict__ SB, long long L,
                                                                        double* __restrict__ Bt, double* __restrict__ G,
                                                                        double* __restrict__ gd, double* __restrict__ sd,
                                                                        const double* __restrict__ CB, const double* __restrict__ delta,
                                                                        double* __restrict__ nb) {
    __shared__ double Ch[VJOBS_MAX_H * VJOBS_MAX_H];
    const int k = blockIdx.x, H = (int)ms.Hs[k];
    const long long LH = L * H, ko = ms.k_off[k], ho = ms.h_off[k];
    const double* Bk = B + ms.b_off[k];
    double* Btk = Bt + ms.b_off[k];
    for (long long t = threadIdx.x; t < LH; t += SCORE_THREADS) {
        const long long l = t / H;
        const int h = (int)(t - l * H);
        Btk[t] = Bk[(long long)h * L + l];
    }
    __syncthreads();
    const double Lg = (double)L;
    for (int e = threadIdx.x; e < H * H; e += SCORE_THREADS) {
        const int i = e / H, j = e % H;
        double s = 0.0;
        for (long long l0 = 0; l0 < L; l0 += LS_ROWS) {
            const long long l1 = l0 + LS_ROWS < L ? l0 + LS_ROWS : L;
            double p = 0.0;
            for (long long l = l0; l < l1; ++l) p = fma(Btk[l * H + i], Btk[l * H + j], p);
            s += p;
        }
        const double sb = Lg * SB[ko + e];
        G[ko + e] = s + sb;
        if (i == j) {
            gd[ho + i] = s;
            sd[ho + i] = sb;
        }
        Ch[e] = SB[ko + e];
    }
    if (nb == nullptr) return;
    // log det SigmaB = the sum of the logs of the pivots of SigmaB = L D L' (right-looking, one barrier per column)
    double logdet = 0.0;
    for (int c = 0; c < H; ++c) {
        __syncthreads();
        const double p = Ch[c * H + c];                   // (the same value for every thread: the exit below is uniform)
        if (!(p > 0.0)) {
            logdet = -__longlong_as_double(0x7FF0000000000000ll);
            break;
        }
        logdet += log(p);
        const int n = H - c - 1;
        for (int e = threadIdx.x; e < n * n; e += SCORE_THREADS) {
            const int i = c + 1 + e / n, j = c + 1 + e % n;
            Ch[i * H + j] -= Ch[i * H + c] * Ch[j * H + c] / p;
        }
    }
    if (threadIdx.x == 0) {                               // (gd, sd: written by this workgroup before the barriers above; H >= 1)
        double cbq = 0.0, sumcb = 0.0, sumlogdelta = 0.0;
        for (int h = 0; h < H; ++h) {
            const double cb = CB[ho + h];
            cbq += cb * (gd[ho + h] + sd[ho + h]);
            sumcb += cb;
            sumlogdelta += log(delta[ho + h]);
        }
        nb[VJOBS_NB * k] = cbq;
        nb[VJOBS_NB * k + 1] = sumcb;
        nb[VJOBS_NB * k + 2] = sumlogdelta;
        nb[VJOBS_NB * k + 3] = logdet;
    }
}

struct VjobsArgs {
    const uint4* Y2; int KSpad; long long L;
    const long long* col_off;
    // per job: job_off[j] = the doubles of the M_b H_k-long blocks of the jobs before j, job_sa[j] the same of their H_k^2 blocks,
    // job_h[j] of their H_k-long ones.  idx: the jobs of this launch (workgroup w runs job idx[w])
    const long long* job_bag; const long long* job_model; const long long* job_off; const long long* job_sa; const long long* job_h;
    const long long* idx;
    VjobsModels ms;
    int niter, compat;
    // per model: Bt L H, G, SigmaB H^2, gd, sd, alpha, beta0 H, eta0, zeta0, sigma0, ca0 one each
    const double* Bt; const double* G; const double* SB; const double* gd; const double* sd; const double* alpha; const double* beta0;
    const double* eta0; const double* zeta0; const double* sigma0; const double* ca0;
    // per job: the M_b H-long blocks at job_off[j], SA H^2 at job_sa[j], sigma, zeta, r2 one each.  Pd: the state's P when it is not in LDS
    double* Pd; double* ca; double* A; double* dS; double* beta; double* SA; double* sigma; double* zeta; double* r2;
    long long* status;
    // a scored call (else all three nullptr): trim per job; sums H SCORE_NS at job_h[j] SCORE_NS; quad two per job
    const double* trim; double* sums; double* quad;
};

// P = Y_b'B (Pb[m * H + h]) and this thread's share of ||Y_b||^2.  st: VJOBS_STAGE doubles of LDS.  Every thread of the workgroup
// calls it.  A slice of nc <= SCORE_CW columns has nc H <= SCORE_THREADS outputs; the threads split into S = SCORE_THREADS / (nc H) row
// stripes (rows s, s + S, ... of every staged tile, tiles in order), whose shares meet in LDS in stripe order.
template <int MODE>
__device__ __forceinline__ double vjobs_product(const uint4* __restrict__ Y2, int KSpad, long long L, const double* __restrict__ Bt,
                                                int H, long long m0, long long Mb, double* Pb, double* st) {
    double* yt = st;                                   // [SCORE_CW][LS_ROWS]
    double* zp = st + SCORE_CW * LS_ROWS;              // [S][nc H]
    const int tid = threadIdx.x;
    double yy = 0.0;
    for (long long c0 = 0; c0 < Mb; c0 += SCORE_CW) {
        const int nc = (int)(Mb - c0 < SCORE_CW ? Mb - c0 : SCORE_CW);
        const int P = nc * H, S = SCORE_THREADS / P;
        const int o = tid < P * S ? tid % P : -1, s = tid / P;
        const int cc = o < 0 ? 0 : o / H, h = o < 0 ? 0 : o % H;
        double acc = 0.0;
        for (long long l0 = 0; l0 < L; l0 += LS_ROWS) {
            const int rows = (int)(L - l0 < LS_ROWS ? L - l0 : LS_ROWS);
            for (int t = tid; t < nc * rows; t += SCORE_THREADS) {
                const int c = t / rows, r = t % rows;
                const double v = (double)score_y_at<MODE>(Y2, KSpad, l0 + r, m0 + c0 + c);
                yt[c * LS_ROWS + r] = v;
                yy = fma(v, v, yy);
            }
            __syncthreads();
            if (o >= 0) {
                const double* bcol = Bt + l0 * H + h;
                const double* ycol = yt + cc * LS_ROWS;
                for (int r = s; r < rows; r += S) acc = fma(bcol[(long long)r * H], ycol[r], acc);
            }
            __syncthreads();
        }
        if (o >= 0) zp[s * P + o] = acc;
        __syncthreads();
        for (int e = tid; e < P; e += SCORE_THREADS) {
            double z = 0.0;
            for (int i = 0; i < S; ++i) z += zp[i * P + e];
            Pb[c0 * H + e] = z;
        }
        // (the next slice writes zp only after two more barriers)
    }
    return yy;
}

template <int MODE, int NBK, bool FULL>
__global__ __launch_bounds__(SBATCH_THREADS) void vbls_jobs_kernel(VjobsArgs g) {
    static_assert(SBATCH_THREADS == SCORE_THREADS, "one workgroup size for the product and the loop");
    extern __shared__ __attribute__((aligned(16))) double lds_vj[];
    __shared__ double red[16];
    __shared__ double v_s[64], al_s[64], b0_s[64], sa_s[64];
    __shared__ int bad_s;
    const int j = (int)g.idx[blockIdx.x], tid = threadIdx.x;
    const int b = (int)g.job_bag[j], k = (int)g.job_model[j];
    const int H = (int)g.ms.Hs[k];
    const long long ko = g.ms.k_off[k], ho = g.ms.h_off[k];
    const long long m0 = g.col_off[b], Mb = g.col_off[b + 1] - m0;
    const long long n = Mb * H, o = g.job_off[j], so = g.job_sa[j];
    const bool in_lds = vjobs_in_lds(FULL, NBK, H, Mb);
    double* Pb = in_lds ? lds_vj + vjobs_fixed_doubles(FULL, NBK, H) : g.Pd + o;
    double* CAb = in_lds ? Pb + n : g.ca + o;
    double* Ab = in_lds ? CAb + n : g.A + o;
    double* dSb = in_lds ? Ab + n : g.dS + o;
    const double* Bt = g.Bt + g.ms.b_off[k];
    if (tid == 0) bad_s = 0;
    if (tid < H) {
        al_s[tid] = g.alpha[ho + tid];
        b0_s[tid] = g.beta0[ho + tid];
    }
    const double ca0 = g.ca0[k];
    for (long long t = tid; t < n; t += SBATCH_THREADS) CAb[t] = ca0;
    double yy = vjobs_product<MODE>(g.Y2, g.KSpad, g.L, Bt, H, m0, Mb, Pb, lds_vj);
    yy = block_sum(yy, red);                           // (its barriers end the product's use of the staging area)
    double sig = g.sigma0[k], zeta = 0.0;
    int bad = 0;
    const SbatchBody q{H, g.niter, g.compat, Mb, g.G + ko, g.gd + ho, g.sd + ho, Pb, CAb, Ab, dSb,
                       g.beta ? g.beta + o : nullptr, g.SA ? g.SA + so : nullptr,
                       g.eta0[k] + 0.5 * (double)g.L * (double)Mb, g.zeta0[k], yy, lds_vj, red, v_s, al_s, b0_s, sa_s};
    sbatch_iterate<NBK, FULL>(q, sig, zeta, bad);
    __syncthreads();                                   // (Ab as the last iteration left it, for every thread)
    double r2 = 0.0;
    const long long ny = Mb * g.L;
    for (long long t = tid; t < ny; t += SBATCH_THREADS) {
        const long long m = t / g.L, l = t - m * g.L;
        const double* brow = Bt + l * H;
        const double* am = Ab + m * H;
        double pred = 0.0;
        for (int h = 0; h < H; ++h) pred += brow[h] * am[h];
        const double d = (double)score_y_at<MODE>(g.Y2, g.KSpad, l, m0 + m) - pred;
        r2 += d * d;
    }
    r2 = block_sum(r2, red);
    if (g.sums != nullptr) {
        // (beta and SigmaA of the last iteration are in the call's buffers: this workgroup wrote them before the barriers above;
        //  the fixed part of dynamic LDS is free since sbatch_iterate returned)
        lb_column_sums<false>(Ab, dSb, CAb, g.beta + o, H, (int)Mb, g.trim[j], lds_vj, g.sums + g.job_h[j] * SCORE_NS);
        const double* SBk = g.SB + ko;
        const double* Gk = g.G + ko;
        double qa = 0.0;
        for (long long t = tid; t < n; t += SBATCH_THREADS) {
            const long long m = t / H;
            const int i = (int)(t - m * H);
            const double* am = Ab + m * H;
            double r = 0.0;
            for (int c = 0; c < H; ++c) r += SBk[i * H + c] * am[c];
            qa += am[i] * r;
        }
        qa = block_sum(qa, red);
        double ts = 0.0;
        for (int t = tid; t < H * H; t += SBATCH_THREADS) ts += g.SA[so + t] * Gk[t];
        ts = block_sum(ts, red);
        if (tid == 0) {
            g.quad[2 * (long long)j] = qa;
            g.quad[2 * (long long)j + 1] = ts;
        }
    }
    bad |= !isfinite(sig) || !isfinite(zeta) || !isfinite(r2);
    if (bad) bad_s = 1;                                // (same value from every writer)
    __syncthreads();
    const bool failed = bad_s != 0;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    if (failed) {
        for (long long t = tid; t < n; t += SBATCH_THREADS) {
            g.ca[o + t] = nan;
            g.A[o + t] = nan;
            g.dS[o + t] = nan;
            if (g.beta) g.beta[o + t] = nan;
        }
        if (g.SA)
            for (int t = tid; t < H * H; t += SBATCH_THREADS) g.SA[so + t] = nan;
    } else if (in_lds) {
        for (long long t = tid; t < n; t += SBATCH_THREADS) {
            g.ca[o + t] = CAb[t];
            g.A[o + t] = Ab[t];
            g.dS[o + t] = dSb[t];
        }
    }
    if (tid == 0) {
        g.sigma[j] = failed ? nan : sig;
        g.zeta[j] = failed ? nan : zeta;
        g.r2[j] = failed ? nan : r2;
        g.status[j] = failed ? 1 : 0;
    }
}

}  // namespace vbmf
