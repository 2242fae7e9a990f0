// vbmf_hip.hip -- context, sweep orchestration and the C ABI declared in include/vbmf_hip.h.
//
// One sweep of vbmf! (src/vbmf.jl:193-214) on the device:
//
//   ctrl_cov(A)   SigmaA                      H x H fp64, one workgroup          src/vbmf.jl:96-97
//   stream pass 1 P[s] = Y' B   (split-K)     reads Y once (copy tiled for k=l)  src/vbmf.jl:98
//   [slab_sum + RCCL all-reduce of P when Y is row-sharded]
//   post(A)       AHat = P SigmaA/sigma2, label mask, fp32 store, operand tiles  src/vbmf.jl:98,101
//   gram(A)       A'A -> fp64
//   ctrl_cov(B)   SigmaB                                                         src/vbmf.jl:110-111
//   stream pass 2 Q = Y A                     reads Y once (copy tiled for k=m)  src/vbmf.jl:112
//   post(B)       BHat = Q SigmaB/sigma2, fp32 store, operand tiles              src/vbmf.jl:112
//   gram(B)       B'B and (Bold-B)'(Bold-B) -> fp64 [+ RCCL all-reduce]
//   eig           lambda_max of both (spectral norms of src/util.jl:27-29)
//   ctrl_end      CA, CB, sigma2, d, loop test, ELBO, trace                      src/vbmf.jl:129-157,193,211
//
// Every kernel of a sweep starts with `if (*stop) return`, and ctrl_end raises `stop` exactly when
// the reference's `while (i <= niter) && (d > eps)` would exit, so the host can enqueue sweeps ahead
// without a per-sweep synchronisation and the state still freezes at the reference's iteration.
//
// Tall matrices (gram_eligible): vbmf_run takes the Gram form instead -- B = Y W with W = A SigmaB / sigma2, so a sweep reads the
// M x M matrix G = Y'Y (built once per Y) in place of Y (gram_kernels.hpp); so does vbmf_sparse_run for the
// diagonal homoscedastic ARD-sparse model (sparse_gram_sweep), up to rank 128 by that rule and up to rank 256 when vbmf_set_gram_form
// (or VBMF_GRAM=3) switches the form on.
//
// vbls! over many bags with one fixed basis (vbmf_run_fixed_basis_batched): ONE pass 1 with the frozen B over the bags side by side,
// then bag_gram (S_b = P_b'P_b, ||Y_b||^2), vbls_batch (all iterations, one workgroup per bag) and bag_a (A_b = P_b SigmaA_b / sigma2_b).
// Here: the context, the launchers, set-up and read-back, the single-matrix updates and run loops (vbmf_run and sparse_run_impl around
// one RunFrame), the sparse / grouped variants and the lower bounds.  The many-bags entries and what they share: host_bags.hpp.
#include "../../include/vbmf_hip.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "common.hpp"
#include "ctx_cache.hpp"
#include "ctx_mem.hpp"
#include "ctrl_kernels.hpp"
#include "post_kernels.hpp"
#include "rng.hpp"
#include "sparse_kernels.hpp"
#include "stream_gemm.hpp"
#include "tile_kernels.hpp"
#include "prep_kernels.hpp"
#include "batch_kernels.hpp"
#include "sparse_batch_kernels.hpp"
#include "fit_batch_kernels.hpp"
#include "fit_split_kernels.hpp"
#include "fit_basic_kernels.hpp"
#include "fit_basic_gram_kernels.hpp"
#include "score_kernels.hpp"
#include "vbls_jobs_kernels.hpp"
#include "vbls_basic_jobs_kernels.hpp"
#include "gram_kernels.hpp"
#include "out_kernels.hpp"

using namespace vbmf;

static thread_local std::string g_create_error;

struct ProfEvent { hipEvent_t a, b; int pass; };

// Device memory (ctx_mem.hpp): the one place that names the device allocator.  A context's and a plan's buffers go through their
// MemOwner, a call's temporaries through a DevScratch; nothing else allocates or frees.
struct HipMem {
    static int alloc(void** p, size_t bytes) { return (int)hipMalloc(p, bytes); }
    static void free(void* p) { hipFree(p); }
};
template <class T>
using DevScratch = Scratch<HipMem, T>;
static const char* mem_errstr(int rc) { return rc == MEM_SLOT_BUSY ? "the slot already holds a buffer" : hipGetErrorString((hipError_t)rc); }

struct vbmf_ctx {
    std::string err;
    vbmf_opts o{};
    int64_t L = 0, M = 0, H = 0, Lg = 0;
    int Hp = 0, NH = 0, mode = 0, kstep = 16, npart = 1;
    Dims d1{}, d2{};                 // pass 1: x=m,k=l ; pass 2: x=l,k=m
    int64_t Mp = 0, Lp = 0;
    uint4 *Y1 = nullptr, *Y2 = nullptr, *FA = nullptr, *FB = nullptr;   // FA/FB point PAST PIPE_D leading zero k-steps
    uint4 *FA_alloc = nullptr, *FB_alloc = nullptr;
    uint4* SBf = nullptr;            // SigmaB table pre-split into bf16 hi / lo MFMA fragments (H >= 128, bf16 factor modes)
    uint4* FD = nullptr;             // delta tiles of B (H >= 128, bf16 factor modes): old - new as bf16 hi + lo operand fragments
    size_t nY1 = 0, nY2 = 0, nFA = 0, nFB = 0;
    float *P = nullptr, *Q = nullptr, *Pred = nullptr;
    float *A32 = nullptr, *B32[2] = {nullptr, nullptr};
    int bcur = 0;
    float *SA32 = nullptr, *SB32 = nullptr, *gslab = nullptr;
    int tiles_per_chunk = 32;
    double* st = nullptr;
    double* gtmp = nullptr;          // [B'B | dB'dB | tr(B'YA), pad] local sums: the send side of the packed all-reduce
    double* gw = nullptr;            // full_cov with diag_var: [this rank's B' diag(sigmaVec) B | its sum over the ranks], Hp^2 each
    double* trpart = nullptr;        // per-wave shares of tr(B'YA) left by the kernel that produced BHat
    int trpart_cap = 0, ntr = 0;     // ntr: shares waiting for the next B-side Gram reduction (0: none)
    double* ypart = nullptr;         // per-block partials of ||Y||^2 (fixed-order sum)
    // ARD-sparse variant (src/vbmf_sparse.jl, diagonal branch)
    bool sparse = false;
    float *dS32 = nullptr, *CA32 = nullptr, *beta32 = nullptr;   // diagSigmaATVec, CA, beta as [Mp][Hp]
    // heteroscedastic rows (variant SPARSE_DIAGVAR): sigmaVecHat / zetaVec, ||Y_l||^2, G = A'A + SigmaA, scaled-B tiles
    bool diagvar = false;
    double *sigv = nullptr, *zetav = nullptr, *yrow = nullptr, *hpart = nullptr, *vsq = nullptr, *hmean = nullptr;
    float *sig32 = nullptr, *G32 = nullptr;
    uint4 *FBs_alloc = nullptr, *FBs = nullptr;
    double etaVec = 0.0;
    double* vtab = nullptr;          // v[h] of src/vbmf_sparse.jl:217
    // two-group ARD variant (src/vbmf_dual.jl, diagonal branch): columns h < H0 / h >= H0 have their own hyper-priors
    bool dual = false;               // grouped model: VBMF_VARIANT_DUAL_DIAG (two groups) or VBMF_VARIANT_TRIAL_DIAG (three)
    bool trial = false;
    int64_t H0 = 0, M0 = 0;          // group 0: columns h < H0; groups 1 / 2: the other columns of rows m < M0 / m >= M0
    double* gpart = nullptr;         // per-block [sum log beta, sum CA] per group
    int gpart_blocks = 0;
    // full_cov = true: block-diagonal posterior of vec(A') (one H x H inverse per column of Y)
    bool full_cov = false;
    bool narrow = false;             // NarrowCfg geometry of the streaming kernel (small problems)
    double* fpart = nullptr;         // per-block sums of Sigma_m
    double* t2part = nullptr;        // sparse run loops: sparse_t2_kernel's shares of sum (GA + SA) o (GB + L SB)
    double* fws = nullptr;           // full_cov, H > 128: per-workgroup [K | inv(K) | W | S] of the blocked Schur inverse
    int fblocks = 0;
    vbmf_sparse_hyper hyp{};
    double alpha = 0, gamma_ = 0, eta = 0;
    StateLayout lay{};
    int* ints = nullptr;
    int* ints_host = nullptr;        // pinned
    // the run loops' view of {stop, iters, err}: host-mapped words that the device's loop test stores into (ctrl_kernels.hpp,
    // publish_loop_words) and the host reads directly -- no copy and no event on the compute stream
    int* loopw = nullptr;            // host address
    int* loopw_dev = nullptr;        // the same words as the device sees them
    double* scal_host = nullptr;     // pinned, 32 doubles
    unsigned char* mask = nullptr;
    int64_t H1 = 0;
    bool has_mask = false;
    hipStream_t stream = nullptr;
    // H > 128: the stand-alone control kernels (1024 threads: they cannot ride inside a 256-thread pass launch) run on a
    // side stream beside the passes, ordered by events
    hipStream_t side = nullptr;
    hipEvent_t ev_main = nullptr, ev_side = nullptr;
    bool use_side = false, side_pending = false;
    bool in_run = false;              // inside vbmf_run: the control chain rides in workgroups 0-1 of the pass launches
    int gslab_cap = 256;
    size_t gslab_bytes = 0;           // allocated size of gslab: every Gram launcher checks its slab count against it
    bool xcd_map = true;              // XCD-aware work map for split-K pass launches (env VBMF_XCD_MAP=0 turns it off)
    // stream-K split of the un-split Y*A pass on the LDS-DMA kernel (stream_gemm.hpp): units per workgroup (0: off), workgroups,
    // the blocks that end up in two parts (device list) and the second slab they go to (c->Q + one slab)
    int sk_per = 0, sk_grid = 0, sk_ntail = 0;      // sk_per: pieces per cut block (T; 0: off); sk_grid: segments = workgroups
    int* sk_tail = nullptr;                          // the cut blocks (device list)
    int* sk_list = nullptr;                          // the segment list: int4 (block, first stage, stages, slab) per workgroup
    bool lds8 = true;                 // H >= 128, bf16x2 operands: the 512-thread LDS-DMA streaming kernel (env VBMF_LDS8=0: the per-wave kernel,
                                      // kept for A/B runs and for the fp32 / single-bf16 operand modes)
    bool exact_lambda = false;        // Lanczos lambda_max at H <= 64 too (VBMF_EXACT_LAMBDA=1, vbmf_debug_set(VBMF_DEBUG_EXACT_LAMBDA))
    bool sparse_a_fused = true;       // ARD-sparse A update writes its operand tiles itself (VBMF_SPARSE_A_FUSED=0: update kernel + retile)
    bool post3 = true;                // H >= 128 factor update with the table shared through LDS (post_frag3_kernel); VBMF_POST3=0: post_frag2
    bool P_frag = false;              // the Y'B product in c->P / c->Pred is fragment-major (stream_gemm.hpp, frag_out)
    bool frag_last[2] = {false, false};   // test surface (VBMF_PEEK_DIMS): the last launch of pass 1 / pass 2 wrote fragment-major output
    bool epi_last = false;            // ... the last launch of pass 2 ran the register epilogue (no product stored)
    int sready_seq = 0;               // sequence number of the Sigma-table release flag (register epilogue)
    bool epi_balance = false;         // x groups of the register-epilogue pass dealt three per workgroup over the whole chip instead
                                      // of four per workgroup: measured SLOWER (0.372 vs 0.366 ms at 100k rows), kept behind
                                      // VBMF_EPI_BALANCE=1 for the record (profiles/r02_f_epilogue_pass_ab.txt)
    int epi_spin_limit = 1 << 22;     // bounded wait of the register epilogue for that flag (~2 s), then VBMF_ERR_SYNC
    int epi_expect_skew = 0;          // test hook (vbmf_debug_set): makes the epilogue wait for a sequence number nobody publishes
    int dbg_sb_ppm = 0;               // test hook (vbmf_debug_set): SigmaB / sigma2 table scaled by (1 + ppm * 1e-6) on the device
    int64_t ends_enqueued = 0;        // sweeps whose closing control step has been enqueued in this run (trace row)
    bool tail_pending = false;        // eig + ctrl_end of the last enqueued sweep not issued yet
    int run_flags = 0;
    double run_eps = 0.0;
    double* run_trace = nullptr;
    CtxCache cache;                   // which derived device data are current, and the only way to change that (ctx_cache.hpp)
    MemOwner<HipMem> mem;             // every device buffer above and below: acquired through it, freed by it (ctx_mem.hpp)
    hipEvent_t ev_y[2] = {nullptr, nullptr};   // around the device work of the last vbmf_set_Y_rows call (created by the first one)
    double set_y_ms = 0.0;            // ... and what they measured: staged copies, tiling kernels, ||Y||^2 (VBMF_PEEK_DIMS word 27, us)
    double out_ms = 0.0;              // the same pair around the last vbmf_get_YHat_rows / vbmf_get_factor_rows call: kernels, staged copies (word 30, us)
    int64_t y_rows = 0;               // vbmf_set_Y_rows: rows of the Y being built that have arrived (L once Y is complete)
    double trYY_local = 0.0;
    int prof = 0;                     // 0 off; k: HIP events around every k-th launch of each pass
    bool prof_skip = true;
    long long prof_seen[2] = {0, 0};
    std::vector<ProfEvent> pev;
    double prof_ms[2] = {0, 0};
    double prof_n[2] = {0, 0};
    ncclComm_t comm = nullptr;
    bool comm_ready = false;
    vbmf_allreduce_fn ar_hook = nullptr;   // bring-up transport instead of RCCL (vbmf_comm_set_transport)
    void* ar_user = nullptr;
    int lds_limit = 65536;
    double* bags = nullptr;           // the many-bags entries (host_bags.hpp): per-bag inputs, partials and outputs of the call in
    size_t bags_bytes = 0;            // flight, each entry in its own layout (grown on demand)
    // Gram-form sweep of vbmf_run (gram_kernels.hpp); buffers allocated by the first run that takes it
    int gram_env = -1;                // VBMF_GRAM: -1 the size rule (gram_eligible), 0 never, 1 whenever the structure allows (basic model), 2 the sparse model too, 3 VBMF_GRAM_FORM_ON
    int gram_form = VBMF_GRAM_FORM_DEFAULT;   // vbmf_set_gram_form: DEFAULT the rule above, OFF never, ON wherever the structure allows (rank 256 included)
    int GT = 0;                       // row tiles of G (multiple of 16); KT = 2 GT k-steps
    int g_nsplit = 1, g_sps = 0, g_nrg = 0, g_nchunk = 0, g_rpc = 0;
    float* Gt = nullptr;              // G = Y'Y as fp32 MFMA operand fragments [GT][2 GT][64][8]
    float* W32g[2] = {nullptr, nullptr};   // W = A SigmaB / sigma2, fp32 [32 GT][Hp], double-buffered like B32
    int wcur = 0;
    uint4* Wt = nullptr;              // operand planes of the product: W in 3 bf16 parts, D in 2
    float* gslabs = nullptr;          // the product's split-K slabs [g_nsplit][P | Q]
    float* gPQ = nullptr;             // [P = G W | Q = G D], fragment-major (P in the layout of the pass-1 product)
    double* g_part = nullptr;         // per-chunk shares of [W'P | D'Q | sum A o P]
    double* gsave = nullptr;          // [GB | GD | GX] kept across the B materialisation after a run
    long long b_materialised = 0;     // test surface (VBMF_PEEK_DIMS): how often ensure_B ran its pass
    double gram_build_ms = 0.0;       // device time of the last G build (HIP events)
};

// the collective code path runs whenever a communicator is attached (also a 1-rank one: used to test it)
static bool sharded(const vbmf_ctx* c) { return c->comm_ready; }

// Host <-> device copies of the set-up and read-back paths: on the context's OWN stream and waited for there.  (A plain
// hipMemcpy runs on the null stream, which the context's non-blocking streams are not ordered against -- neither the copy
// after the kernels that produce its source, nor the kernels that consume its destination after the copy.)
static hipError_t memcpy_sync(vbmf_ctx* c, void* dst, const void* src, size_t n, hipMemcpyKind kind) {
    const hipError_t e = hipMemcpyAsync(dst, src, n, kind, c->stream);
    return e != hipSuccess ? e : hipStreamSynchronize(c->stream);
}

// ------------------------------------------------------------------------------------------------
#define FAIL(ctx, code, ...)                                   \
    do {                                                       \
        char _b[512];                                          \
        snprintf(_b, sizeof _b, __VA_ARGS__);                  \
        (ctx)->err = _b;                                       \
        return (code);                                         \
    } while (0)

#define HIPCHK(ctx, call)                                                                              \
    do {                                                                                               \
        hipError_t _e = (call);                                                                        \
        if (_e != hipSuccess) FAIL(ctx, VBMF_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), \
                                   __FILE__, __LINE__);                                                \
    } while (0)

// an acquire / regrow of the context's MemOwner or an alloc of a DevScratch
#define MEMCHK(ctx, call)                                                                              \
    do {                                                                                               \
        int _m = (call);                                                                               \
        if (_m != 0) FAIL(ctx, VBMF_ERR_HIP, "%s failed: %s (%s:%d)", #call, mem_errstr(_m), __FILE__, __LINE__); \
    } while (0)

#define NCCLCHK(ctx, call)                                                                               \
    do {                                                                                                 \
        ncclResult_t _e = (call);                                                                        \
        if (_e != ncclSuccess) FAIL(ctx, VBMF_ERR_COMM, "%s failed: %s (%s:%d)", #call, ncclGetErrorString(_e), \
                                    __FILE__, __LINE__);                                                 \
    } while (0)

#define TRY(expr)                 \
    do {                          \
        int _rc = (expr);         \
        if (_rc != VBMF_OK) return _rc; \
    } while (0)

// Runtime value -> template argument, the one way: dispatch<V1, V2, ...>(v, f) calls f(std::integral_constant<int, Vk>{}) for the
// listed Vk that equals v and returns false when none does (the caller FAILs: a missing kernel is an error).  The list at the call
// site IS the set of instances that exist -- a kernel is instantiated for exactly the values named there.  f is a generic lambda,
// inlined: nothing is erased and nothing allocated on the launch path.  An f that returns bool hands its answer through (nested lists).
template <int V, class F>
static inline bool dispatch_one(F& f) {
    if constexpr (std::is_same_v<decltype(f(std::integral_constant<int, V>{})), bool>) return f(std::integral_constant<int, V>{});
    else { f(std::integral_constant<int, V>{}); return true; }
}
template <int... Vs, class F>
static inline bool dispatch(int v, F&& f) { return ((v == Vs && dispatch_one<Vs>(f)) || ...); }
#define NO_KERNEL(ctx) FAIL(ctx, VBMF_ERR_INVALID, "internal: no kernel instance for this rank / mode (%s:%d)", __FILE__, __LINE__)

// Y as the kernels read it from its tiles: fp32 or bf16 (bf16x2 is a factor mode; Y itself is bf16 there)
static inline int ymode_of(int mode) { return mode == MODE_F32 ? MODE_F32 : MODE_BF16; }
// NB = 16 x 16 blocks across an H x H image of the one-workgroup vbls! kernels (H <= 64)
static inline int nb_tier(int64_t H) { return H <= 16 ? 1 : (H <= 32 ? 2 : 4); }
// The control tiers H -> (R, T): R 16-column blocks across the H x H image, T x T threads (T = 32: the 1024-thread kernels of
// 128 < H <= 256).  f(integral_constant R, integral_constant T); every ladder over H that picks a control kernel goes through here.
template <class F>
static inline void ctrl_tier(int64_t H, F&& f) {
    using std::integral_constant;
    if (H <= 16) f(integral_constant<int, 1>{}, integral_constant<int, 16>{});
    else if (H <= 32) f(integral_constant<int, 2>{}, integral_constant<int, 16>{});
    else if (H <= 64) f(integral_constant<int, 4>{}, integral_constant<int, 16>{});
    else if (H <= 128) f(integral_constant<int, 8>{}, integral_constant<int, 16>{});
    else f(integral_constant<int, 8>{}, integral_constant<int, 32>{});
}

static inline int64_t rup(int64_t a, int64_t b) { return (a + b - 1) / b * b; }
static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
static inline int grid_for(int64_t n, int block = 256, int cap = 8192) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((n + block - 1) / block, cap));
}

// host-side guard of every launcher that writes Gram partial slabs: `nslab` slabs of `floats` fp32 values must fit c->gslab
#define GSLAB_CHECK(c, nslab, floats)                                                                                       \
    do {                                                                                                                    \
        if ((size_t)(nslab) * (size_t)(floats) * 4 > (c)->gslab_bytes)                                                      \
            FAIL(c, VBMF_ERR_INVALID, "internal: %lld Gram slabs of %lld floats exceed the slab buffer (%zu bytes) (%s:%d)", \
                 (long long)(nslab), (long long)(floats), (c)->gslab_bytes, __FILE__, __LINE__);                            \
    } while (0)

// per-NH geometry of the streaming kernel: NXW * NH accumulator tiles per wave -- 8 (128 registers) up to H = 64,
// 16 (all 256 AGPRs) from H = 128 on, where the factor operand's L2->L1 traffic per Y byte is what limits a CU
// (measured, scripts/bigh_tune.hip: H=128 0.64 -> 0.51 ms per 2.5 GB pass, H=256 1.48 -> 0.83 ms per 2 GB pass);
// Y ring DY and factor ring DF k-steps deep (VGPR budget: 4*(DY*NXW + DF*NF) + addressing)
template <int NH> struct StreamCfg;
template <> struct StreamCfg<1> { static constexpr int NXWc = 8; static constexpr int DYc = 3; static constexpr int DFc = 3; static constexpr int Rc = 2; };
template <> struct StreamCfg<2> { static constexpr int NXWc = 4; static constexpr int DYc = 6; static constexpr int DFc = 2; static constexpr int Rc = 4; };
template <> struct StreamCfg<4> { static constexpr int NXWc = 4; static constexpr int DYc = 4; static constexpr int DFc = 2; static constexpr int Rc = 8; };
template <> struct StreamCfg<8> { static constexpr int NXWc = 2; static constexpr int DYc = 2; static constexpr int DFc = 2; static constexpr int Rc = 0; };

// "narrow" geometry (H <= 64, small problems): half the x tiles per wave, so twice the column groups -- a 1000-column matrix
// is ONE column group of the wide H <= 32 kernel (64 split-K workgroups on 256 CUs), and an 8-way row shard needs half the
// split-K slices.  Costs factor-operand traffic per Y byte: chosen only when the wide geometry has <= 2 column groups.
template <int NH> struct NarrowCfg;
template <> struct NarrowCfg<1> { static constexpr int NXWc = 4; static constexpr int DYc = 6; static constexpr int DFc = 3; static constexpr int Rc = 2; };
template <> struct NarrowCfg<2> { static constexpr int NXWc = 2; static constexpr int DYc = 12; static constexpr int DFc = 2; static constexpr int Rc = 4; };

static int nxw_of(int NH, bool narrow = false) {                                     // = StreamCfg<NH>::NXWc / NarrowCfg<NH>::NXWc
    if (narrow && NH <= 2) return NH == 1 ? 4 : 2;
    return NH == 1 ? 8 : (NH == 8 ? 2 : 4);
}
static int dy_of(int NH, bool narrow = false) {                                      // = ...::DYc
    if (narrow && NH <= 2) return NH == 1 ? 6 : 12;
    return NH == 1 ? 3 : (NH == 2 ? 6 : (NH == 4 ? 4 : 2));
}
// two CUs are left to the control workgroups that ride in each pass launch
constexpr int NUM_CU = 254;

// Split-K plan.  A CU streams at most ~24-30 GB/s with this kernel (so ~220+ busy CUs are needed to
// saturate HBM), and a pass ends with its most loaded CU, so it takes
//     max( rounds * bytes_per_block / R_CU ,  total_bytes / R_HBM )  +  slab write+read
// with rounds = ceil(blocks / 256).  Pick the split factor minimising that (measured at 100k x 10k:
// 240 blocks 0.35 ms, 260 blocks 0.61 ms, 160 blocks 0.44 ms -- the model's ordering).
// Y ring depth of the H = 64 register-epilogue pass (tuning switch, A/B on the GPU): with three waves per CU (balanced map) a
// deeper ring keeps more bytes in flight per wave
#ifndef VBMF_EPI_DY
#define VBMF_EPI_DY 6
#endif

static void plan_pass(Dims& d, int64_t X, int64_t K, int kstep, int NH, int Hp, double ybytes, int want_splits, bool narrow,
                      int kq_also = 0, bool two_rounds_at_nh8 = true) {
    // padding quanta: x tiles to the per-wave tile count, k-steps to the Y ring depth (zero tiles are streamed
    // like real ones, so padding is pure waste: 3.7 % of pass 2 at 100k x 10k with the old 8-tile / 12-step quanta)
    const int xq = nxw_of(NH, narrow), kq = std::max(dy_of(NH, narrow), kq_also);
    static_assert(VBMF_EPI_DY % 6 == 0 && PIPE_D % VBMF_EPI_DY == 0, "the epilogue pass's ring depth must be a multiple of the wide geometry's");
    d.XT = (int)rup(cdiv(X, 32), xq);
    const int64_t ks_min = rup(cdiv(rup(K, 32 * xq), kstep), kq);   // K padded like the other pass's x tiles
    const int XG = d.XT / xq;
    const int bps = (XG + 3) / 4;
    int ns = want_splits;
    if (ns <= 0) {
        // measured in the sweep pipeline (H=64: 200 vs 240 blocks 0.434 vs 0.390 ms); a CU's rate falls with H
        // (more MFMA work and factor traffic per Y byte): H=128 ~20 GB/s, H=256 ~10 GB/s (scripts/bigh_tune.hip)
        const double R_CU = NH <= 2 ? 24e9 : (NH == 4 ? 20e9 : 10e9), R_HBM = 5.4e12;
        const double total = (double)d.XT * 32.0 * (double)ks_min * kstep * ybytes;
        const double out_bytes = (double)Hp * d.XT * 32.0 * 4.0;
        const int ns_max = (int)std::max<int64_t>(1, std::min<int64_t>(64, ks_min / (2 * kq)));
        double best = 1e300;
        ns = 1;
        for (int cand = 1; cand <= ns_max; ++cand) {
            const int blocks = bps * cand;
            const int rounds = (blocks + NUM_CU - 1) / NUM_CU;
            // split-K partials: written at HBM rate, re-read by a latency-bound consumer at ~1.5 TB/s
            // (measured: 5 slabs of 25.6 MB cost the post kernel +150 us)
            const double slab = cand > 1 ? cand * out_bytes * (1.0 / R_HBM + 1.0 / 1.5e12) : 0.0;
            const double t = std::max(rounds * (total / blocks) / R_CU, total / R_HBM) + slab;
            if (t < best * 0.999) { best = t; ns = cand; }
        }
    }
    // H > 128: the stand-alone control kernels run beside the passes on a side stream and hold a CU each for
    // 0.3-0.5 ms; a one-round pass then ends that much later (its last workgroup waits for the busy CU), a two-round
    // pass of half-size workgroups just gives that CU fewer of them (measured at 100k x 10k, H = 256: 1.13 -> 0.83 ms)
    // (round 3: not with the 512-thread LDS-DMA kernel -- one round of whole-size workgroups is as fast there, and half the slices
    //  are half the partial slabs to write and to sum: config 5 +1.3 %, profiles/r03_h_cfg5_splits.txt)
    if (want_splits <= 0 && NH == 8 && two_rounds_at_nh8 && bps * ns <= NUM_CU && 2 * ns <= ks_min / (2 * kq)) ns *= 2;
    ns = (int)std::max<int64_t>(1, std::min<int64_t>(ns, std::max<int64_t>(1, ks_min / kq)));
    d.nsplit = ns;
    d.steps_per_split = (int)rup(cdiv(ks_min, d.nsplit), kq);
    d.KS = d.steps_per_split * d.nsplit;
}

// ------------------------------------------------------------------------------------------------
static void prof_begin(vbmf_ctx* c, int pass) {
    c->prof_skip = true;
    if (!c->prof) return;
    if ((c->prof_seen[pass]++ % c->prof) != 0) return;       // every prof-th launch of each pass is timed
    c->prof_skip = false;
    ProfEvent e{};
    e.pass = pass;
    hipEventCreate(&e.a);
    hipEventCreate(&e.b);
    hipEventRecord(e.a, c->stream);
    c->pev.push_back(e);
}
static void prof_end(vbmf_ctx* c) {
    if (!c->prof || c->prof_skip) return;
    hipEventRecord(c->pev.back().b, c->stream);
}
static void prof_harvest(vbmf_ctx* c) {
    for (auto& e : c->pev) {
        hipEventSynchronize(e.b);
        float ms = 0.f;
        hipEventElapsedTime(&ms, e.a, e.b);
        c->prof_ms[e.pass] += ms;
        c->prof_n[e.pass] += 1;
        hipEventDestroy(e.a);
        hipEventDestroy(e.b);
    }
    c->pev.clear();
}

// argument `spectral` of the lambda_max kernels: bit 0 = d uses spectral norms (else the trace), bit 1 = Lanczos at EVERY rank (H <= 64
// otherwise keeps the repeated squaring: exact off clusters, up to ~2.5e-4 inside one, half the time inside short pass launches)
static int spectral_arg(const vbmf_ctx* c) {
    return ((c->o.reference_compat & VBMF_COMPAT_SPECTRAL_DELTA) ? 1 : 0) | (c->exact_lambda ? 2 : 0);
}
// threads per workgroup of the lambda_max kernels of the chain's own (eig_kernel, ctrl_chain_kernel): 512 where the squaring runs in
// its wide form (eig_squaring_dev: R = 4, 32 < H <= 64), else 256 -- R = 1 and 2, the Lanczos tiers and the Lanczos switch
static int eig_wide_launch(int R, int spectral) { return (R == 4 && !(spectral & 2)) ? 512 : 256; }
static bool use_lds8(const vbmf_ctx* c) { return c->lds8 && c->NH >= 4 && c->mode == MODE_BF16X2; }

// dynamic LDS of the control chain's workgroups at R = NP / 16 (pass launches: R = 2 NH; ctrl_chain_kernel: R of the stand-alone kernels)
static size_t ctrl_lds_bytes_r(int R) {
    const size_t NP = 16 * (size_t)R;
    // lambda_max (Lanczos vector + tridiagonal: EIG_LDS_BYTES) | the blocked inverse's NP x (NP + 2) fp64 image (ctrl_kernels.hpp)
    const size_t eig = std::max(R <= 4 ? (size_t)2 * NP * (NP + 4) * sizeof(float) : (size_t)0, (size_t)EIG_LDS_BYTES);      // squaring | Lanczos
    return std::max(eig, spd_inverse_lds_bytes(R));
}
static size_t ctrl_lds_bytes(int NH) { return NH <= 4 ? ctrl_lds_bytes_r(2 * NH) : 0; }
// dynamic LDS of sparse_update_a_full_wave_kernel<NBK, NW>: per wavefront the 16 NBK x (16 NBK + 2) fp64 image and one column.  The launcher
// and vbmf_create's table of large-LDS kernels both take it from here.
constexpr size_t full_a_wave_lds_bytes(int NBK, int NW) { return ((size_t)NW * 16 * NBK * (16 * NBK + 2) + (size_t)NW * 16 * NBK) * sizeof(double); }
static bool fused_ctrl(const vbmf_ctx* c) { return c->in_run && c->NH <= 4; }
// the host-mapped loop counters, for the device's loop test: only a run loop looks at them
static int* loop_words(const vbmf_ctx* c) { return c->in_run ? c->loopw_dev : nullptr; }

// One factor side as its launchers see it.  which = 0: A (M rows, the x side of pass 1, the label mask); 1: B (L rows, pass 2).
struct Side {
    const Dims& d;
    const float* S;                  // the side's Sigma / sigma2 table
    float* Fac;                      // the fp32 factor the launch writes
    uint4* Ft;                       // ... and its operand tiles
    const unsigned char* mask;       // label mask (A side, when one is set) or null
    int hstart;                      // first masked column
};
// B is double-buffered: an update writes the NEXT buffer (the delta-Gram reads the current one beside it), a retile rewrites the
// CURRENT one in place.  Every caller says which.
enum BSlot { B_CUR = 0, B_NEXT = 1 };
static Side side_of(vbmf_ctx* c, int which, BSlot slot) {
    if (which == 0) return Side{c->d1, c->SA32, c->A32, c->FA, c->has_mask ? c->mask : nullptr, (int)(c->H - c->H1)};
    return Side{c->d2, c->SB32, c->B32[c->bcur ^ (int)slot], c->FB, nullptr, (int)(c->H - c->H1)};
}

// the control chain's arguments, for a pass launch that carries it (launch_stream) or a launch of its own (launch_chain)
static CtrlArgs ctrl_args(vbmf_ctx* c, int mode, float* S32) {
    CtrlArgs ca{};
    ca.st = c->st; ca.lay = c->lay; ca.ints = c->ints; ca.trace = c->run_trace;
    ca.S32 = S32;
    ca.Lg = (double)c->Lg; ca.M = (double)c->M; ca.eps = c->run_eps;
    ca.H = (int)c->H; ca.spectral = spectral_arg(c);
    ca.end_flags = c->run_flags; ca.mode = mode; ca.it_row = (int)c->ends_enqueued; ca.loopw = loop_words(c);
    return ca;
}

// ctrl_mode != 0: workgroup 0 of the launch runs that part of the control chain (CtrlArgs)
// epi (pass 2 only, un-split, NH <= 2): B, its operand tiles and the Gram partials are produced in the kernel's register
// epilogue (no separate post kernel); the caller then only reduces c->gslab over `*epi_slabs` workgroup slabs
static int launch_stream(vbmf_ctx* c, int pass, int ctrl_mode = 0, bool epi = false, int* epi_slabs = nullptr, bool frag_out = false) {
    const Dims& d = pass == 0 ? c->d1 : c->d2;
    const uint4* Y = pass == 0 ? c->Y1 : c->Y2;
    const uint4* F = pass == 0 ? (c->diagvar ? c->FBs : c->FB) : c->FA;
    float* out = pass == 0 ? c->P : c->Q;
    const long long ld = (long long)d.XT * 32;
    int XG = d.XT / nxw_of(c->NH, c->narrow);
    int bps = (XG + 3) / 4;
    EpiArgs ea{};
    if (epi) {
        // balanced workgroup -> x-group map of the un-split pass (stream_gemm.hpp, EpiArgs): three groups per workgroup while
        // that fits one round of the chip, four otherwise
        int nb = bps;
        if (c->epi_balance && cdiv(XG, 3) <= NUM_CU) nb = cdiv(XG, 3);
        else if (c->epi_balance && cdiv(XG, NUM_CU) <= 4) nb = std::max(bps, std::min(NUM_CU, XG));
        ea.g_base = XG / nb;
        ea.g_rem = XG % nb;
        bps = nb;
        XG = 4 * nb;                                   // (the kernel derives its workgroup count per split from XG)
    }
    // split-K launches use the XCD-aware work map (stream_gemm.hpp): 8 * per workgroups, per = ceil(blocks / 8)
    const int xper = (d.nsplit > 1 && c->xcd_map) ? cdiv(bps * d.nsplit, 8) : 0;
    const int grid = (xper ? 8 * xper : bps * d.nsplit) + (ctrl_mode ? 2 : 0);
    CtrlArgs ca = ctrl_args(c, ctrl_mode, pass == 0 ? c->SA32 : c->SB32);
    ea.frag_out = frag_out ? 1 : 0;
    if (epi) {
        c->sready_seq = (c->sready_seq + 1) & 0x3fffffff;
        ea.S = c->SB32; ea.Fac = c->B32[c->bcur ^ 1]; ea.Prev = c->B32[c->bcur]; ea.Ft = c->FB; ea.slabs = c->gslab;
        ea.sready = c->ints + I_SREADY; ea.expect = ctrl_mode ? c->sready_seq + c->epi_expect_skew : -1; ea.err = c->ints + I_ERR;
        ea.spin_limit = c->epi_spin_limit;
        ea.store_fac = c->in_run ? 0 : 1;
        ea.trpart = c->trpart;
#if VBMF_SEAM_STAMPS
        ea.stamp = nullptr;                                        // slots 4-7 carry the seams' stamps past a run's closing pass
#else
        ea.stamp = reinterpret_cast<unsigned long long*>(c->ints + 16);
#endif
        c->ntr = 4 * bps;
        if (c->in_run) c->cache.B32_store_skipped();
        if (ctrl_mode) { ca.sready = c->ints + I_SREADY; ca.sready_val = c->sready_seq; }
        if (epi_slabs) *epi_slabs = bps;
        GSLAB_CHECK(c, bps, 2 * (c->NH * (c->NH + 1) / 2) * 1024);
    }
    const size_t lds = ctrl_mode ? ctrl_lds_bytes(c->NH) : 0;
    c->frag_last[pass] = frag_out && !epi;
    if (pass == 1) c->epi_last = epi;
    prof_begin(c, pass);
    bool ok = true;
    if (use_lds8(c) && !epi) {
        if (lds > (size_t)LDS8_BYTES) FAIL(c, VBMF_ERR_INVALID, "internal: control chain needs %zu bytes of LDS", lds);
        // stream-K: the fragment-major product of the un-split Y*A pass, balanced over the chip (plan: vbmf_create)
        const bool sk = pass == 1 && frag_out && c->sk_per > 0 && d.nsplit == 1;
        const int sk_per = sk ? c->sk_grid : 0;                                   // (the kernel's argument: number of segments)
        const float* out2 = sk ? reinterpret_cast<const float*>(c->sk_list) : nullptr;   // ... and the segment list
        const int grid8 = sk ? c->sk_grid + (ctrl_mode ? 2 : 0) : grid;
        const int xper8 = sk ? 0 : xper;
        ok = dispatch<4, 8>(c->NH, [&](auto nh) {
            return dispatch<0, 1>(sk ? 1 : 0, [&](auto skc) {
                constexpr int NHc = decltype(nh)::value;
                hipLaunchKernelGGL((stream_lds8_kernel<NHc, StreamCfg<NHc>::Rc, decltype(skc)::value != 0>), dim3(grid8), dim3(512), LDS8_BYTES,
                                   c->stream, Y, F, out, d.XT, d.KS, d.steps_per_split, d.nsplit, ld, c->ints + I_STOP, ca, xper8,
                                   ea.frag_out, sk_per, out2);
            });
        });
        if (sk && c->sk_ntail > 0) {
            // the blocks that were cut: product += its second part (a block is contiguous in the fragment-major layout)
            const long long blk = (long long)(c->NH == 8 ? 8 : 16) * c->NH * 1024;        // x tiles per workgroup * NH tiles * 1024 floats
            hipLaunchKernelGGL(streamk_fixup_kernel, dim3(16, std::min(c->sk_ntail, 1024)), dim3(256), 0, c->stream, out, c->sk_per, c->sk_tail,
                               c->sk_ntail, blk, (long long)c->Hp * c->Lp, c->ints + I_STOP);
        }
    } else {
        // the pass kernel's geometry: the register-epilogue pass and the narrow geometry exist for NH <= 2 only, the wide one for every NH
        ok = dispatch<MODE_F32, MODE_BF16, MODE_BF16X2>(c->mode, [&](auto md) {
            constexpr int MODEc = decltype(md)::value;
            if (epi) return dispatch<1, 2>(c->NH, [&](auto nh) {
                constexpr int NHc = decltype(nh)::value;
                using Cfg = StreamCfg<NHc>;
                constexpr int DYc = NHc == 1 ? Cfg::DYc : VBMF_EPI_DY;
                hipLaunchKernelGGL((stream_gemm_kernel<MODEc, NHc, Cfg::NXWc, DYc, Cfg::DFc, Cfg::Rc, 0, 1>), dim3(grid), dim3(256), lds,
                                   c->stream, Y, F, out, XG, d.KS, d.steps_per_split, d.nsplit, ld, c->ints + I_STOP, ca, xper, ea);
            });
            if (c->narrow) return dispatch<1, 2>(c->NH, [&](auto nh) {
                constexpr int NHc = decltype(nh)::value;
                using Cfg = NarrowCfg<NHc>;
                hipLaunchKernelGGL((stream_gemm_kernel<MODEc, NHc, Cfg::NXWc, Cfg::DYc, Cfg::DFc, Cfg::Rc>), dim3(grid), dim3(256), lds,
                                   c->stream, Y, F, out, XG, d.KS, d.steps_per_split, d.nsplit, ld, c->ints + I_STOP, ca, xper, ea);
            });
            return dispatch<1, 2, 4, 8>(c->NH, [&](auto nh) {
                constexpr int NHc = decltype(nh)::value;
                using Cfg = StreamCfg<NHc>;
                hipLaunchKernelGGL((stream_gemm_kernel<MODEc, NHc, Cfg::NXWc, Cfg::DYc, Cfg::DFc, Cfg::Rc>), dim3(grid), dim3(256), lds,
                                   c->stream, Y, F, out, XG, d.KS, d.steps_per_split, d.nsplit, ld, c->ints + I_STOP, ca, xper, ea);
            });
        });
    }
    prof_end(c);
    if (!ok) NO_KERNEL(c);
    HIPCHK(c, hipGetLastError());
    return VBMF_OK;
}

// recv = sum over the ranks of send (recv == send: in place), ordered on the context's stream.
// The two per-sweep reductions are OUT OF PLACE on purpose: their send buffers are written by stop-gated kernels only, so a
// sweep enqueued after the device-side stop re-reduces the SAME partials into the SAME result -- the frozen state stays
// frozen without a staging buffer and a gated copy behind every collective (one launch fewer per sweep).
static int allreduce_sum(vbmf_ctx* c, const void* send, void* recv, size_t count, bool is_double) {
    if (c->ar_hook) {
        if (send != recv)
            HIPCHK(c, hipMemcpyAsync(recv, send, count * (is_double ? 8 : 4), hipMemcpyDeviceToDevice, c->stream));
        const int rc = c->ar_hook(c->ar_user, recv, count, is_double ? 1 : 0, (void*)c->stream);
        if (rc != 0) FAIL(c, VBMF_ERR_COMM, "all-reduce transport hook failed (%d)", rc);
        return VBMF_OK;
    }
    NCCLCHK(c, ncclAllReduce(send, recv, count, is_double ? ncclDouble : ncclFloat, ncclSum, c->comm, c->stream));
    return VBMF_OK;
}
static int allreduce_sum(vbmf_ctx* c, void* buf, size_t count, bool is_double) { return allreduce_sum(c, buf, buf, count, is_double); }

// What a B-side post kernel leaves beside B for the Gram reduction behind it (launch_post, both branches of launch_post_frag,
// launch_post_gram; grid: the launch's workgroups, four waves each): trp, the per-wave shares of tr(B'YA), c->ntr of which then wait
// in c->trpart (not with heteroscedastic rows: B is rescaled afterwards); fd, the delta tiles old - new; store_fac = 0 inside a run
// whose delta-Gram needs no fp32 B (the operand tiles carry the factor: rebuild_B32_if_stale).  The A side touches nothing.
// The four launchers' own copies agreed wherever each is reached: vbmf_create allocates c->FD exactly when
// NH >= 4, the mode is not fp32 and diag_var is off, so every "may this launch write delta tiles" test IS c->FD; post_gram's grid is at
// most gslab_cap <= trpart_cap / 4, so the capacity test it left out always held; and c->ntr is read only by the reduction of a B
// update, behind the B-side launch of that update, so launch_post's reset on the A side was never seen.
// fused_delta is the one real difference: post_gram2 forms the delta-Gram itself (the previous rows from their operand tiles) and skips
// the store without delta tiles; behind the other kernels launch_gram, lacking delta tiles, needs both fp32 factors stored.
struct BSideOut { double* trp; uint4* fd; int store_fac; };
static BSideOut b_side_outputs(vbmf_ctx* c, int which, int grid, bool fused_delta) {
    if (which != 1) return BSideOut{nullptr, nullptr, 1};
    double* trp = (!c->diagvar && 4 * grid <= c->trpart_cap) ? c->trpart : nullptr;
    c->ntr = trp ? 4 * grid : 0;
    uint4* fd = c->FD;
    const int store_fac = (c->in_run && (fd != nullptr || fused_delta)) ? 0 : 1;
    c->cache.delta_tiles_written(fd != nullptr);
    if (!store_fac) c->cache.B32_store_skipped();
    return BSideOut{trp, fd, store_fac};
}

static int launch_post(vbmf_ctx* c, int which, const float* In, int nslab) {
    const Side sd = side_of(c, which, B_NEXT);
    const long long ld = (long long)sd.d.XT * 32;
    const long long slabStride = (long long)c->Hp * ld;
    const int nxt = c->NH >= 8 ? VBMF_POST_NXT8 : 1;                          // = PostCfg<NH>::NXT
    const int grid = (cdiv(sd.d.XT, nxt) + 3) / 4;
    // B side at H >= 128 (bf16 factor modes): delta tiles for the delta-Gram; inside the run loops no fp32 copy of B per sweep
    // (heteroscedastic rows: B = diag(sigmaVecHat) (Y A) SigmaB is scaled AFTER this kernel, from the fp32 factor it stores -- no
    //  delta tiles of the un-scaled product, and the fp32 store stays)
    const BSideOut bo = b_side_outputs(c, which, grid, false);
    const bool ok = dispatch<MODE_F32, MODE_BF16, MODE_BF16X2>(c->mode, [&](auto md) {
        return dispatch<1, 2, 4, 8>(c->NH, [&](auto nh) {
            hipLaunchKernelGGL((post_kernel<decltype(md)::value, decltype(nh)::value>), dim3(grid), dim3(256), 0, c->stream, In, ld, nslab,
                               slabStride, sd.S, sd.Fac, sd.Ft, sd.mask, sd.hstart, sd.d.XT, c->ints + I_STOP, bo.trp, bo.fd, bo.store_fac);
        });
    });
    if (!ok) NO_KERNEL(c);
    HIPCHK(c, hipGetLastError());
    return VBMF_OK;
}

// fused post + Gram (+ delta-Gram) for NH <= 2; reduction into the state block (or the all-reduce staging)
static bool fused_gram(const vbmf_ctx* c) { return c->NH <= 2; }

static int gram_reduce_tail(vbmf_ctx* c, int which, bool gated, int ntr, bool pair_slabs, int nslab);

// A (which = 0) or B (which = 1) from ONE fragment-major product (H >= 128): bf16 factor modes run the software-pipelined
// post_frag2_kernel on a table pre-split into VBMF_POST_NT bf16 parts in order of use; the fp32 mode keeps the exact-f32 kernel
#ifndef VBMF_POST_NT
#define VBMF_POST_NT 3            // 3: six-term product (exact to an fp32 rounding); 2: round 1's three-term product (2^-17 per term)
#endif
static bool frag_post(const vbmf_ctx* c) { return c->NH >= 4 && c->mode != MODE_F32; }
static int launch_post_frag(vbmf_ctx* c, int which = 1, const float* In = nullptr) {
    const Side sd = side_of(c, which, B_NEXT);
    if (In == nullptr) In = c->Q;
    const float4* In4 = (const float4*)In;
    const int* stop = c->ints + I_STOP;
    if (c->mode == MODE_F32) {
        if (which != 1) FAIL(c, VBMF_ERR_INVALID, "fragment-major A update in the fp32 mode");
        const int nxt = c->NH >= 8 ? VBMF_POST_NXT8 : 1;                          // = PostCfg<NH>::NXT
        const int grid = (cdiv(sd.d.XT, nxt) + 3) / 4;
        const BSideOut bo = b_side_outputs(c, which, grid, false);                // (no c->FD in the fp32 mode: no delta tiles, B stored)
        if (!dispatch<4, 8>(c->NH, [&](auto nh) {
                hipLaunchKernelGGL((post_frag_kernel<MODE_F32, decltype(nh)::value>), dim3(grid), dim3(256), 0, c->stream, In4, sd.S, sd.Fac, sd.Ft,
                                   sd.mask, 0, sd.d.XT, stop, bo.trp, bo.fd, bo.store_fac, (const uint4*)nullptr);
            })) NO_KERNEL(c);
        HIPCHK(c, hipGetLastError());
        return VBMF_OK;
    }
    // row tiles per wave: 256 accumulator registers' worth on the long side; ONE on a short side (the 10k-row A side would
    // otherwise occupy 20 workgroups)
    const bool short_side = sd.d.XT < 2048;
    // post_frag3 (table through LDS, two workgroups per CU): 128 accumulator registers per wave on the long side
    const int nxt = short_side ? 1 : (c->post3 ? (c->NH >= 8 ? 1 : 2) : (c->NH >= 8 ? VBMF_POST2_NXT8 : VBMF_POST2_NXT4));
    const int grid = (cdiv(sd.d.XT, nxt) + 3) / 4;
    const BSideOut bo = b_side_outputs(c, which, grid, false);
    const uint4* Sf = c->SBf;
    // one instance per (mode, NH, side) and per tile count that side length can pick: 1 or the kernel's long-side count at that NH
    const bool ok = dispatch<MODE_BF16, MODE_BF16X2>(c->mode, [&](auto md) {
        return dispatch<4, 8>(c->NH, [&](auto nh) {
            constexpr int MODEc = decltype(md)::value, NHc = decltype(nh)::value;
            constexpr int LONG3 = NHc >= 8 ? 1 : 2, LONG2 = NHc >= 8 ? VBMF_POST2_NXT8 : VBMF_POST2_NXT4;
            const int nthr = NHc * 2 * NHc * 64;
            hipLaunchKernelGGL((split_table_parts_kernel<NHc, VBMF_POST_NT>), dim3((nthr + 255) / 256), dim3(256), 0, c->stream, sd.S, c->SBf, stop);
            return dispatch<0, 1>(which, [&](auto bs) {
                constexpr bool BS = decltype(bs)::value != 0;
                if (c->post3) return dispatch<1, LONG3>(nxt, [&](auto nx) {
                    hipLaunchKernelGGL((post_frag3_kernel<MODEc, NHc, decltype(nx)::value, VBMF_POST_NT, BS>), dim3(grid), dim3(256), 0, c->stream,
                                       In4, Sf, sd.Fac, sd.Ft, sd.mask, sd.hstart, sd.d.XT, stop, bo.trp, bo.fd, bo.store_fac);
                });
                return dispatch<1, LONG2>(nxt, [&](auto nx) {
                    hipLaunchKernelGGL((post_frag2_kernel<MODEc, NHc, decltype(nx)::value, VBMF_POST_NT, BS>), dim3(grid), dim3(256), 0, c->stream,
                                       In4, Sf, sd.Fac, sd.Ft, sd.mask, sd.hstart, sd.d.XT, stop, bo.trp, bo.fd, bo.store_fac);
                });
            });
        });
    });
    if (!ok) NO_KERNEL(c);
    HIPCHK(c, hipGetLastError());
    return VBMF_OK;
}
// post + Gram (+ delta-Gram, tr(B'YA)) of ONE fragment-major product (NH <= 2): post_gram2_kernel
static int launch_post_gram(vbmf_ctx* c, int which, const float* In) {
    const Side sd = side_of(c, which, B_NEXT);
    const int grid = std::min(c->gslab_cap, (sd.d.XT + 3) / 4);
    GSLAB_CHECK(c, grid, 2 * (c->NH * (c->NH + 1) / 2) * 1024);
    // inside the run loops the fp32 copy of B is not written per sweep: the operand tiles carry the factor (rebuilt once at the end)
    const BSideOut bo = b_side_outputs(c, which, grid, true);
    const bool ok = dispatch<MODE_F32, MODE_BF16, MODE_BF16X2>(c->mode, [&](auto md) {
        return dispatch<1, 2>(c->NH, [&](auto nh) {
            return dispatch<0, 1>(which, [&](auto bs) {
                hipLaunchKernelGGL((post_gram2_kernel<decltype(md)::value, decltype(nh)::value, decltype(bs)::value != 0>), dim3(grid), dim3(256), 0,
                                   c->stream, In, sd.S, sd.Fac, sd.Ft, sd.mask, sd.hstart, sd.d.XT, c->gslab, c->ints + I_STOP, bo.trp, bo.store_fac);
            });
        });
    });
    if (!ok) NO_KERNEL(c);
    HIPCHK(c, hipGetLastError());
    return gram_reduce_tail(c, which, true, bo.trp ? 4 * grid : 0, true, grid);
}

// The end of every Gram of a factor: fp64 reduction of the `nslab` partial slabs in c->gslab (pair slabs: the upper pairs only, as the
// fused kernels and gram_tiles3 leave them; else dense) and of the `ntr` trace shares into the state -- or, B side of a row-sharded
// run, into the packed message [B'B | dB'dB | tr(B'YA) | error flag] that one all-reduce puts straight into the state block (GB, GD, GX
// are contiguous).  gated = false (ensure_gram_B: state just set, no sweep has run): no stop test, and only the Gram travels.
static int gram_reduce_tail(vbmf_ctx* c, int which, bool gated, int ntr, bool pair_slabs, int nslab) {
    const int* stop = gated ? c->ints + I_STOP : nullptr;
    const int n = c->Hp * c->Hp;
    const bool shard = (which == 1 && sharded(c));
    double* outG = shard ? c->gtmp : c->st + (which == 0 ? c->lay.GA() : c->lay.GB());
    double* outD = which == 0 ? nullptr : (shard ? c->gtmp + n : c->st + c->lay.GD());
    double* outTr = (which == 1 && ntr > 0) ? (shard ? c->gtmp + 2 * n : c->st + c->lay.GX()) : nullptr;
    double* outErr = (shard && gated) ? c->gtmp + 2 * n + 1 : nullptr;   // this rank's error flag rides in the packed message
    if (pair_slabs) {
        if (!dispatch<1, 2, 4, 8>(c->NH, [&](auto nh) {
                constexpr int NHc = decltype(nh)::value, NPAIR = NHc * (NHc + 1) / 2;
                hipLaunchKernelGGL((pair_slab_reduce_kernel<NHc>), dim3(2 * NPAIR * 1024 / 64), dim3(1024), 0, c->stream, c->gslab, nslab, outG, outD,
                                   stop, c->trpart, ntr, outTr, outErr);
            })) NO_KERNEL(c);
    } else {
        hipLaunchKernelGGL(gram_reduce_kernel, dim3((2 * n + 31) / 32), dim3(256), 0, c->stream, c->gslab, nslab, n,
                           outG, outD, stop, c->trpart, ntr, outTr, outErr);
    }
    HIPCHK(c, hipGetLastError());
    // (sharded(c) is "a communicator is attached": the collective below cannot find none)
    if (shard) TRY(allreduce_sum(c, c->gtmp, c->st + c->lay.GB(), gated ? 2 * (size_t)n + 2 : (size_t)n, true));
    return VBMF_OK;
}

// which = 0: A (x tiles of pass 1's factor... i.e. M rows), 1: B (L rows).  Fac -> operand tiles Ft; with writeback the
// fp32 factor becomes exactly what the tiles encode.  rowscale: per-row factor applied on the way (heteroscedastic rows).
static int launch_retile_ex(vbmf_ctx* c, int which, float* Fac, uint4* Ft, const float* rowscale, int writeback, bool gated) {
    const int XT = which == 0 ? c->d1.XT : c->d2.XT;
    const int grid = (XT + 3) / 4;
    const bool ok = dispatch<MODE_F32, MODE_BF16, MODE_BF16X2>(c->mode, [&](auto md) {
        return dispatch<1, 2, 4, 8>(c->NH, [&](auto nh) {
            hipLaunchKernelGGL((retile_kernel<decltype(md)::value, decltype(nh)::value>), dim3(grid), dim3(256), 0, c->stream, Fac, Ft, XT, rowscale,
                               writeback, gated ? c->ints + I_STOP : (const int*)nullptr);
        });
    });
    if (!ok) NO_KERNEL(c);
    HIPCHK(c, hipGetLastError());
    return VBMF_OK;
}
// the side's own factor, in place: the CURRENT B, not the one an update is writing
static int launch_retile(vbmf_ctx* c, int which, bool gated = false) {
    const Side sd = side_of(c, which, B_CUR);
    return launch_retile_ex(c, which, sd.Fac, sd.Ft, nullptr, 1, gated);
}

// 32-row tiles per Gram chunk (= per workgroup) of side `which`.  H >= 128: a chunk's slab is 2 Hp^2 floats (512 KiB at H = 256), so
// the long side keeps >= 16 tiles per chunk (the slab traffic of the reduction); a SHORT side (the 10k-row A side: 313 tiles) would
// then fill 20 CUs only -- it takes 4 tiles per chunk or more (measured at 10k x 256: 40 -> see DESIGN.md section 7).
static int gram_tiles_per_chunk(const vbmf_ctx* c, int which) {
    if (c->NH < 4) return c->tiles_per_chunk;
    const int XT = which == 0 ? c->d1.XT : c->d2.XT;
    // long side: one round of ~250 workgroups (fp32 factor mode: the dense-slab kernels keep the context-wide value)
    if (XT >= 2048) return c->mode == MODE_F32 ? c->tiles_per_chunk : std::max(8, cdiv(XT, 250));
    return std::max(4, cdiv(XT, 96));
}
// Gram of A (which=0) or of B with optional delta-Gram against prev (which=1) into the state block.
static int launch_gram(vbmf_ctx* c, int which, const float* cur, const float* prev, bool gated, int ntr = 0) {
    const Side sd = side_of(c, which, B_NEXT);         // (its Dims and tiles: the fp32 factors come as `cur` and `prev`)
    const int XT = sd.d.XT;
    const int tpc = gram_tiles_per_chunk(c, which);
    const int nchunk = cdiv(XT, tpc);
    const int nw = nchunk * c->NH * c->NH;
    const int* stop = gated ? c->ints + I_STOP : nullptr;
    // H >= 128 with a bf16 factor: from the operand tiles with bf16 MFMAs (the tiles of `cur` are current whenever a
    // Gram of it is asked for: every producer of the fp32 factor writes them in the same kernel)
    const bool from_tiles = c->NH >= 4 && c->mode != MODE_F32;
    // delta-Gram: a plain tile Gram of the delta tiles the post kernel left (two parts: hi + lo) -- or, without them
    // (f32-free callers that bring their own previous fp32 factor), from `prev` with row gathers
    const bool from_fd = from_tiles && which == 1 && prev != nullptr && c->cache.delta_tiles() && c->FD != nullptr;
    const bool pair_slabs = from_tiles && (from_fd || prev == nullptr);      // gram_tiles3 leaves pair slabs (the H <= 64 kernels' format)
    GSLAB_CHECK(c, nchunk, 2 * c->Hp * c->Hp);         // dense slabs; pair slabs (upper pairs only) are smaller
    bool ok;
    if (from_tiles) {
        ok = dispatch<4, 8>(c->NH, [&](auto nh) {
            return dispatch<1, 2>(c->npart, [&](auto np) {
                constexpr int NHc = decltype(nh)::value, NPc = decltype(np)::value;
                if (pair_slabs) {
                    hipLaunchKernelGGL((gram_tiles3_kernel<NHc, NPc>), dim3(nchunk), dim3(256), 0, c->stream, sd.Ft,
                                       from_fd ? (const uint4*)c->FD : (const uint4*)nullptr, c->gslab, XT, tpc, stop);
                } else {
                    hipLaunchKernelGGL((gram_tiles_kernel<NHc, NPc, 0>), dim3(nchunk), dim3(256), 0, c->stream, sd.Ft, prev, c->gslab, XT, tpc, stop, 0);
                    hipLaunchKernelGGL((gram_tiles_kernel<NHc, NPc, 1>), dim3(nchunk), dim3(256), 0, c->stream, sd.Ft, prev, c->gslab, XT, tpc, stop, 1);
                }
            });
        });
    } else {
        ok = dispatch<1, 2, 4, 8>(c->NH, [&](auto nh) {
            hipLaunchKernelGGL((gram_kernel<decltype(nh)::value>), dim3((nw + 3) / 4), dim3(256), 0, c->stream, cur, prev, c->gslab, XT, tpc, nchunk, stop);
        });
    }
    if (!ok) NO_KERNEL(c);
    return gram_reduce_tail(c, which, gated, ntr, pair_slabs, nchunk);
}

static int ctrl_threads(int H) { return H <= 16 ? 64 : (H <= 32 ? 256 : 1024); }

static hipStream_t ctrl_stream(vbmf_ctx* c) { return c->use_side ? c->side : c->stream; }
// fork: what follows on ctrl_stream() runs beside the main stream, after everything enqueued on it so far;
// end: back to the main stream; join: the main stream waits for the side section (no-op if none is pending)
static int side_fork(vbmf_ctx* c) {
    HIPCHK(c, hipEventRecord(c->ev_main, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->side, c->ev_main, 0));
    c->use_side = true;
    return VBMF_OK;
}
static int side_end(vbmf_ctx* c) {
    c->use_side = false;
    HIPCHK(c, hipEventRecord(c->ev_side, c->side));
    c->side_pending = true;
    return VBMF_OK;
}
static int side_join(vbmf_ctx* c) {
    if (!c->side_pending) return VBMF_OK;
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_side, 0));
    c->side_pending = false;
    return VBMF_OK;
}
static bool side_overlap(const vbmf_ctx* c) { return c->in_run && c->NH == 8; }

// dynamic LDS of the covariance kernels (ctrl_cov, sparse_cov_b) at a control tier
template <int R, int T>
constexpr size_t cov_lds_bytes() { return (R == 8 && T == 32) ? (size_t)(INV256_LDS_DOUBLES + 256) * sizeof(double) : spd_inverse_lds_bytes(R); }

static int launch_ctrl_cov(vbmf_ctx* c, int which) {
    const double N = which == 0 ? (double)c->Lg : (double)c->M;
    float* S32 = which == 0 ? c->SA32 : c->SB32;
    ctrl_tier(c->H, [&](auto r, auto t) {
        constexpr int R = decltype(r)::value, T = decltype(t)::value;
        hipLaunchKernelGGL((ctrl_cov_kernel<R, T>), dim3(1), dim3(T * T), (cov_lds_bytes<R, T>()), ctrl_stream(c), c->st, c->lay, (int)c->H, which,
                           N, S32, c->ints);
    });
    HIPCHK(c, hipGetLastError());
    return VBMF_OK;
}

static int launch_eig(vbmf_ctx* c, int do_d, int do_b) {
    const int H = (int)c->H, spectral = spectral_arg(c);
    hipStream_t s = ctrl_stream(c);
    ctrl_tier(H, [&](auto r, auto t) {
        constexpr int R = decltype(r)::value, NP = 16 * R;
        if constexpr (decltype(t)::value == 32) {             // 128 < H <= 256: the stand-alone Lanczos kernel
            hipLaunchKernelGGL(eig_lanczos_kernel, dim3(2), dim3(1024), 0, s, c->st, c->lay, H, spectral, do_d, do_b, c->ints);
        } else {
            const size_t lds = std::max(R <= 4 ? (size_t)2 * NP * (NP + 4) * sizeof(float) : (size_t)0, (size_t)EIG_LDS_BYTES);     // squaring | Lanczos
            hipLaunchKernelGGL((eig_kernel<R>), dim3(2), dim3(eig_wide_launch(R, spectral)), lds, s, c->st, c->lay, H, spectral, do_d, do_b,
                               c->ints);
        }
    });
    HIPCHK(c, hipGetLastError());
    return VBMF_OK;
}

static int launch_ctrl_end(vbmf_ctx* c, int flags, double eps, double* trace) {
    hipLaunchKernelGGL(ctrl_end_kernel, dim3(1), dim3(c->H > 128 ? 1024 : 256), 0, ctrl_stream(c), c->st, c->lay, (int)c->H, (double)c->Lg,
                       (double)c->M, flags, eps, trace, c->ints, loop_words(c));
    HIPCHK(c, hipGetLastError());
    return VBMF_OK;
}

// need_Y = false: updateCA!/updateCB! read the factors and covariances only (src/vbmf.jl:129-146, src/vbmf_sparse.jl:284-300 --
// the reference's signatures take no Y), so a context that was never given a matrix can run them
// want_B = false: the caller (a run loop's frame) decides itself whether it needs B -- a Gram-form run that finds W valid does not
static int ensure_B(vbmf_ctx* c);
static int ensure_ready(vbmf_ctx* c, bool need_Y = true, bool want_B = true) {
    if (need_Y && !c->cache.have_Y()) FAIL(c, VBMF_ERR_INVALID, "no Y: call vbmf_set_Y or vbmf_set_Y_synthetic first");
    if (!c->cache.have_state()) FAIL(c, VBMF_ERR_INVALID, "no state: call vbmf_set_state first");
    if (c->o.nranks > 1 && !c->comm_ready) FAIL(c, VBMF_ERR_COMM, "nranks > 1 but vbmf_comm_init was not called");
    if (want_B) TRY(ensure_B(c));
    if (c->cache.have_Y() && !c->cache.trYY_reduced()) {
        double* dst = c->st + c->lay.scal() + S_TRYY;
        HIPCHK(c, hipMemcpyAsync(dst, &c->trYY_local, sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        TRY(allreduce_sum(c, dst, 1, true));
        c->cache.trYY_summed();
    }
    if (c->diagvar && c->cache.have_noise() && !c->cache.noise_mean_reduced()) {
        if (sharded(c)) TRY(allreduce_sum(c, c->st + c->lay.scal() + S_SIGMA2, 1, true));   // shares of mean(sigmaVecHat)
        c->cache.noise_mean_summed();
    }
    return VBMF_OK;
}

static int ensure_gram_A(vbmf_ctx* c) {
    if (c->cache.gram_A()) return VBMF_OK;
    TRY(launch_gram(c, 0, c->A32, nullptr, false));
    c->cache.gram_A_made();
    return VBMF_OK;
}
static int ensure_gram_B(vbmf_ctx* c) {
    if (c->cache.gram_B()) return VBMF_OK;
    TRY(launch_gram(c, 1, c->B32[c->bcur], nullptr, false));
    c->cache.gram_B_made();
    return VBMF_OK;
}

// Inside vbmf_run (NH <= 4) the control chain rides in workgroup 0 of the pass launches:
//   pass 1 of sweep i : [lambda_max + ctrl_end of sweep i-1] + SigmaA of sweep i
//   pass 2 of sweep i : SigmaB of sweep i
// Outside (vbmf_step, H > 128) the same device code runs as stand-alone kernels before the pass.
// reuse_P: B has not changed since Y'B was last formed (fixed-basis inference, vbls!): skip the pass over Y
static int do_update_A(vbmf_ctx* c, bool reuse_P = false) {
    TRY(ensure_gram_B(c));
    const bool have_P = reuse_P && c->cache.P();
    bool commit_pending = false;
    if (have_P) {
        TRY(launch_ctrl_cov(c, 0));
    } else if (fused_ctrl(c)) {
        c->P_frag = fused_gram(c) || frag_post(c);   // Y'B travels fragment-major to the post kernel (16-byte accesses)
        TRY(launch_stream(c, 0, CTRL_COV_A | (c->tail_pending ? CTRL_PREV_END : 0), false, nullptr, c->P_frag));
        if (c->tail_pending) ++c->ends_enqueued;
        c->tail_pending = false;
        // SigmaA was computed speculatively beside the previous sweep's stop test: commit it iff the loop continues
        // (inside the slab-sum launch when there is one, else as its own small kernel)
        commit_pending = true;
        if (!(sharded(c) || c->d1.nsplit > 1)) {
            hipLaunchKernelGGL(commit_cov_a_kernel, dim3(8), dim3(256), 0, c->stream, c->st, c->lay, c->ints);
            HIPCHK(c, hipGetLastError());
            commit_pending = false;
        }
    } else if (side_overlap(c)) {
        // H > 128: SigmaA (after the previous sweep's lambda_max / ctrl_end, already on the side stream) beside the pass
        TRY(side_fork(c));
        TRY(launch_ctrl_cov(c, 0));
        TRY(side_end(c));
        c->P_frag = frag_post(c);
        TRY(launch_stream(c, 0, 0, false, nullptr, c->P_frag));
    } else {
        TRY(launch_ctrl_cov(c, 0));
        c->P_frag = fused_gram(c) || frag_post(c);
        TRY(launch_stream(c, 0, 0, false, nullptr, c->P_frag));
    }
    if (sharded(c) || c->d1.nsplit > 1) {
        const long long n = (long long)c->Hp * c->d1.XT * 32;
        if (!have_P) {
            SideCopy sc{};
            if (commit_pending)
                sc = SideCopy{c->st + c->lay.W0(), c->st + c->lay.SA(), c->lay.n2(), c->st + c->lay.scal() + S_LOGDET_SA_SHADOW,
                              c->st + c->lay.scal() + S_LOGDET_SA};
            // row-sharded: this rank's sum stays in slab 0 (written by stop-gated kernels only) and the all-reduce goes
            // out of place into Pred (see allreduce_sum)
            hipLaunchKernelGGL(slab_sum_kernel, dim3(grid_for(n / 4, 256, 2048)), dim3(256), 0, c->stream, c->P, c->d1.nsplit, n,
                               sharded(c) ? c->P : c->Pred, n, c->ints + I_STOP, sc);
            HIPCHK(c, hipGetLastError());
            if (sharded(c))
                TRY(allreduce_sum(c, c->P, c->Pred, (size_t)n, false));
        }
        TRY(side_join(c));
        if (fused_gram(c)) TRY(launch_post_gram(c, 0, c->Pred));
        else if (c->P_frag) TRY(launch_post_frag(c, 0, c->Pred));
        else TRY(launch_post(c, 0, c->Pred, 1));
    } else {
        TRY(side_join(c));
        if (fused_gram(c)) TRY(launch_post_gram(c, 0, c->P));
        else if (c->P_frag) TRY(launch_post_frag(c, 0, c->P));
        else TRY(launch_post(c, 0, c->P, 1));
    }
    if (!fused_gram(c)) TRY(launch_gram(c, 0, c->A32, nullptr, true));
    c->cache.A_moved_basic();
    return VBMF_OK;
}

// split-K partials of the Y*A pass (short row shards): fold them into slab 0 at HBM/L2 rate; the latency-bound post
// kernel then reads one slab (measured on a 12.5k-row shard: post_gram 85 -> 15 us)
static int fold_Q_slabs(vbmf_ctx* c) {
    if (c->d2.nsplit <= 1) return VBMF_OK;
    const long long n = (long long)c->Hp * c->d2.XT * 32;
    hipLaunchKernelGGL(slab_sum_kernel, dim3(grid_for(n / 4, 256, 2048)), dim3(256), 0, c->stream, c->Q, c->d2.nsplit, n, c->Q, n,
                       c->ints + I_STOP, SideCopy{});
    HIPCHK(c, hipGetLastError());
    return VBMF_OK;
}

// keep_sigma: B from the SigmaB / sigma2 table already in place (the end of a Gram-form run materialises B with the last sweep's table)
static int do_update_B(vbmf_ctx* c, bool keep_sigma = false) {
    TRY(ensure_gram_A(c));
    // un-split pass at H <= 64: B, its tiles and the Gram partials come out of the pass's register epilogue
    const bool epi = fused_gram(c) && !c->narrow && c->d2.nsplit == 1 && (c->d2.XT / nxw_of(c->NH) + 3) / 4 <= c->gslab_cap;
    if (epi) {
        int nslab = 0;
        if (fused_ctrl(c)) {
            TRY(launch_stream(c, 1, CTRL_COV_B | CTRL_EIG_BOLD, true, &nslab));
        } else {
            if (!keep_sigma) TRY(launch_ctrl_cov(c, 1));
            TRY(launch_stream(c, 1, 0, true, &nslab));
        }
        TRY(gram_reduce_tail(c, 1, true, c->ntr, true, nslab));
        c->bcur ^= 1;
        c->cache.B_moved_basic();
        return VBMF_OK;
    }
    // H >= 128, un-split pass: the product travels fragment-major (16-byte accesses on both sides)
    // H <= 64 without the register epilogue (split pass on short row shards, narrow geometry): always fragment-major -- slabs
    // are folded element-wise and post_gram2_kernel reads the layout
    const bool fragq = fused_gram(c) || c->d2.nsplit == 1;
    if (fused_ctrl(c)) {
        TRY(launch_stream(c, 1, CTRL_COV_B | CTRL_EIG_BOLD, false, nullptr, fragq));
    } else if (side_overlap(c)) {
        TRY(side_fork(c));
        TRY(launch_ctrl_cov(c, 1));
        TRY(side_end(c));
        TRY(launch_stream(c, 1, 0, false, nullptr, fragq));
    } else {
        if (!keep_sigma) TRY(launch_ctrl_cov(c, 1));
        TRY(launch_stream(c, 1, 0, false, nullptr, fragq));
    }
    TRY(fold_Q_slabs(c));
    TRY(side_join(c));
    if (fused_gram(c)) {
        TRY(launch_post_gram(c, 1, c->Q));
    } else {
        if (fragq) TRY(launch_post_frag(c));
        else TRY(launch_post(c, 1, c->Q, 1));
        TRY(launch_gram(c, 1, c->B32[c->bcur ^ 1], c->B32[c->bcur], true, c->ntr));
    }
    c->bcur ^= 1;
    c->cache.B_moved_basic();
    return VBMF_OK;
}

// ---- Gram-form sweep (gram_kernels.hpp) ----------------------------------------------------------------
// Taken by vbmf_run when the structure allows it (basic variant, one rank, bf16 Y, bf16x2 factors, Hp <= 128) and Y is tall enough
// for building G = Y'Y once to pay: L >= 4 M and L M >= 2^27 (below that a streaming pass costs a few launch latencies).
// VBMF_GRAM=0 turns it off, VBMF_GRAM=1 on whenever the structure allows.
// The ARD-sparse model's diagonal homoscedastic branch (vbmf_sparse_run, sparse_gram_sweep below) has the same structure -- nothing on
// the B side is masked, B = Y W with W = sigmaHat A SigmaB -- and follows the same size rule (measured at 100k x 10k: 2.7x the streaming
// sweep at H = 64, 2.1x at H = 128).  It is forced on by VBMF_GRAM=2, which forces the basic model too; VBMF_GRAM=1
// forces the basic model only and leaves a sparse context to the size rule.
// vbmf_set_gram_form (or VBMF_GRAM=3 at creation) overrides both: OFF always streams, ON takes the form wherever the structure
// allows it -- and only ON admits the sparse model at Hp = 256 (gram_w_cols, gram_prod<4, 8>, the blocked gram_tail), which no size
// rule and no other VBMF_GRAM value turns on.  The basic model at Hp = 256 stays streaming: its Gram sweep is the fused one (NH <= 4).
static bool gram_form_on(const vbmf_ctx* c) {
    return c->gram_form == VBMF_GRAM_FORM_ON || (c->gram_form == VBMF_GRAM_FORM_DEFAULT && c->gram_env == 3);
}
static bool gram_structural(const vbmf_ctx* c) {
    return !c->diagvar && !c->dual && !c->trial && !c->full_cov && !sharded(c) && c->o.nranks == 1 && c->o.y_dtype == VBMF_Y_BF16 &&
           c->mode == MODE_BF16X2 && (c->Hp <= 128 || (c->Hp == 256 && c->sparse && gram_form_on(c)));
}
static bool gram_eligible(const vbmf_ctx* c) {
    if (c->gram_form == VBMF_GRAM_FORM_OFF || !gram_structural(c)) return false;
    if (gram_form_on(c)) return true;
    if (c->gram_env == 0) return false;
    if (c->gram_env == 2 || (c->gram_env == 1 && !c->sparse)) return true;
    return c->L >= 4 * c->M && (double)c->L * (double)c->M >= 134217728.0;
}

// h tiles per workgroup of the product kernel: all NH up to 4; rank 256 runs as two groups of the NH = 4 geometry
static int gram_prod_nh(const vbmf_ctx* c) { return c->NH == 8 ? 4 : c->NH; }

// buffers (first time) and G of the current Y (once per Y)
static int gram_prepare(vbmf_ctx* c) {
    if (!c->Gt) {
        c->GT = (int)rup(c->d1.XT, 16);
        const int KT = 2 * c->GT;
        const int nhp = gram_prod_nh(c);
        c->g_nrg = c->GT / (16 / nhp);                                         // row groups of GramProd<nhp>::TPG row tiles
        // split-K: about one workgroup per CU, each split at least 8 k-steps
        c->g_nsplit = std::max(1, std::min(KT / 8, NUM_CU / std::max(1, c->g_nrg)));
        if (c->NH != nhp) {
            // rank 256: NH / nhp h-tile groups, so w = g_nrg NH / nhp workgroups per split, one per CU at a time (144 KB of LDS).  A
            // split count s runs in ceil(w s / NUM_CU) rounds of 1 / s of the k-steps each: the s <= 4 with the smallest product, the
            // smaller s on a tie (a slab is written and read back once per split).  Config 5: w = 160, s = 3, 480 workgroups in two
            // rounds of 1/3; one split from w = 193 on (GT >= 400).
            const int w = c->g_nrg * (c->NH / nhp), smax = std::max(1, std::min(KT / 8, 4));
            int best = 1;
            for (int s = 2; s <= smax; ++s)
                if ((int64_t)cdiv(w * s, NUM_CU) * best < (int64_t)cdiv(w * best, NUM_CU) * s) best = s;
            c->g_nsplit = best;
        }
        c->g_sps = cdiv(KT, c->g_nsplit);
        c->g_nsplit = cdiv(KT, c->g_sps);
        const int64_t Mp1 = (int64_t)c->d1.XT * 32;
        // gram_tail: two workgroups of 8 waves per chunk (one per product); 128 chunks at Hp <= 64 (one workgroup per CU), 64 at
        // Hp = 128, where a share is 4x larger.  The plan is the one the 16-wave gram_part had: the sums' order depends on it.
        // Hp = 256: eight workgroups per chunk (two products x four 128 x 128 blocks) and a share of 1 MB: 32 chunks, one workgroup
        // per CU, 32 MB of shares; gram_part_reduce then sums eight chunks per group in one round.
        c->g_nchunk = (int)std::max<int64_t>(1, std::min<int64_t>(c->Hp == 256 ? 32 : (c->Hp == 128 ? 64 : 128), cdiv(c->M, 64)));
        c->g_rpc = (int)rup(cdiv(c->M, c->g_nchunk), 16);
        c->g_nchunk = cdiv(c->M, c->g_rpc);
        const size_t n = (size_t)c->Hp * Mp1;
        const size_t wrows = (size_t)32 * c->GT;
        // the zero fill goes on the context's stream: a hipMemset on the null stream is not ordered before the build kernel on this
        // non-blocking stream, and a fill still running over G's tail zeroed entries the build had already stored
        // all eight or none: a failure rolls the group back, so !c->Gt above stays the test for "not prepared"
        const size_t group = c->mem.mark();
        auto alloc = [&](auto*& slot, size_t bytes) -> int {
            int e = c->mem.acquire(slot, bytes);
            if (e == 0) e = (int)hipMemsetAsync(slot, 0, bytes, c->stream);
            return e;
        };
        int e = alloc(c->Gt, (size_t)c->GT * KT * 64 * 8 * 4);
        if (e == 0) e = alloc(c->W32g[0], wrows * c->Hp * 4);
        if (e == 0) e = alloc(c->W32g[1], wrows * c->Hp * 4);
        if (e == 0) e = alloc(c->Wt, (size_t)GRAM_PLANES * KT * c->NH * 64 * 16);
        if (e == 0) e = alloc(c->gPQ, 2 * n * 4);
        if (e == 0 && c->g_nsplit > 1) e = alloc(c->gslabs, (size_t)c->g_nsplit * 2 * n * 4);
        if (e == 0) e = alloc(c->g_part, (size_t)c->g_nchunk * (2 * (size_t)c->Hp * c->Hp + 2) * 8);   // (+2: the blocked share's trace slots)
        if (e == 0) e = alloc(c->gsave, (2 * (size_t)c->Hp * c->Hp + 8) * 8);
        if (e != 0) {
            c->mem.rollback(group);
            FAIL(c, VBMF_ERR_HIP, "Gram-form sweep: device allocation failed (%s)", mem_errstr(e));
        }
        c->cache.G_buffers_new();
    }
    if (c->cache.G()) return VBMF_OK;
    hipEvent_t a, b;
    HIPCHK(c, hipEventCreate(&a));
    HIPCHK(c, hipEventCreate(&b));
    hipEventRecord(a, c->stream);
    const int NB = c->GT / 4;
    hipLaunchKernelGGL(gram_build_kernel, dim3(NB, NB), dim3(256), 0, c->stream, c->Y1, c->d1.XT, c->d1.KS, c->Gt, c->GT);
    const hipError_t le = hipGetLastError();
    hipEventRecord(b, c->stream);
    const hipError_t se = hipEventSynchronize(b);
    float ms = 0.f;
    hipEventElapsedTime(&ms, a, b);
    hipEventDestroy(a);
    hipEventDestroy(b);
    HIPCHK(c, le);
    HIPCHK(c, se);
    c->gram_build_ms = ms;
    c->cache.G_built();
    return VBMF_OK;
}

// W_new = A SigmaB / sigma2 and D = W_new - W_old (into W32g[wcur ^ 1]; the caller flips wcur), then [P | Q] = G [W_new | D];
// partials: the state's [B'B | dB'dB | tr(B'YA)] of B = Y W_new from it (gram_tail folds the slabs and forms the shares; without
// partials the old slab_sum launch folds them).  Profile slot 1 brackets the product.
static int gram_product(vbmf_ctx* c, bool partials) {
    const int* stop = c->ints + I_STOP;
    const int KT = 2 * c->GT;
    const int64_t Mp1 = (int64_t)c->d1.XT * 32;
    const long long n = (long long)c->Hp * Mp1;
    const float* Wo = c->W32g[c->wcur];
    float* Wn = c->W32g[c->wcur ^ 1];
    const dim3 wg(cdiv(KT, GW_KS));
    // rank 256 (Hp = 256, NH = 8) runs as blocks of the rank-128 geometry: W in two column groups, the product in two h-tile groups of
    // the NH = 4 kernel, the shares in four 128 x 128 blocks per product
    const bool ok = dispatch<32, 64, 128, 256>(c->Hp, [&](auto hp) {
        constexpr int HPT = decltype(hp)::value, HPc = HPT == 256 ? 128 : HPT;
        if constexpr (HPT == 256)
            hipLaunchKernelGGL((gram_w_cols_kernel<256, 2>), dim3(wg.x, 2), dim3(512), 0, c->stream, c->A32, c->SB32, Wo, Wn, c->Wt, (long long)c->M, KT, stop);
        else
            hipLaunchKernelGGL((gram_w_kernel<HPT>), wg, dim3(HPT * 4), 0, c->stream, c->A32, c->SB32, Wo, Wn, c->Wt, (long long)c->M, KT, stop);
        float* out = c->g_nsplit > 1 ? c->gslabs : c->gPQ;
        const dim3 grid(c->g_nrg * c->g_nsplit, c->NH / gram_prod_nh(c));
        prof_begin(c, 0);
        {
            constexpr int NHT = HPT / 32, NHc = NHT == 8 ? 4 : NHT;           // = gram_prod_nh
            hipLaunchKernelGGL((gram_prod_kernel<NHc, NHT>), grid, dim3(GramProd<NHc>::THREADS), GramProd<NHc>::LDS_BYTES, c->stream,
                               reinterpret_cast<const float4*>(c->Gt), c->Wt, out, c->GT, c->d1.XT, c->g_sps, c->g_nrg, n, 2 * n, stop);
        }
        prof_end(c);
        if (!partials) {
            // no shares wanted (the run boundary): only the folded [P | Q], by the plain slab sum
            if (c->g_nsplit > 1)
                hipLaunchKernelGGL(slab_sum_kernel, dim3(grid_for(2 * n / 4, 256, 2048)), dim3(256), 0, c->stream, c->gslabs, c->g_nsplit, 2 * n,
                                   c->gPQ, 2 * n, stop, SideCopy{});
            return;
        }
        // the slabs folded into gPQ (one split: gPQ read in place) and the chunk shares from the folded values, in one launch
        const dim3 tg((HPT == 256 ? 8 : 2) * c->g_nchunk);
        hipLaunchKernelGGL((gram_tail_kernel<HPc, HPT>), tg, dim3(512), 0, c->stream, out, c->g_nsplit, 2 * n, c->gPQ, n, (long long)Mp1, Wn, Wo,
                           c->A32, (long long)c->M, c->g_rpc, c->g_nchunk, c->g_part, stop);
        const dim3 rg(cdiv(2 * (int64_t)c->Hp * c->Hp + 1, GRED_E));
        hipLaunchKernelGGL((gram_part_reduce_kernel<HPc, HPT>), rg, dim3(256), 0, c->stream, c->g_part, c->g_nchunk, c->st, c->lay, stop);
    });
    if (!ok) FAIL(c, VBMF_ERR_INVALID, "internal: the Gram-form sweep covers Hp <= 256");
    HIPCHK(c, hipGetLastError());
    return VBMF_OK;
}

// the control chain as a launch of its own (ctrl_chain_kernel: one workgroup per part of ctrl_chain that the mode asks for).  R follows
// H as for the stand-alone control kernels, so every fp64 operation sees the inputs, the work split and the summation order it saw there.
static int launch_chain(vbmf_ctx* c, int mode, float* S32) {
    if (c->H > 128) FAIL(c, VBMF_ERR_INVALID, "internal: the stand-alone control chain covers H <= 128");
    const CtrlArgs ca = ctrl_args(c, mode, S32);
    const int parts = (mode & CTRL_EIG_AHEAD) ? 3 : ((mode & (CTRL_PREV_END | CTRL_EIG_BOLD)) ? 2 : 1);
    ctrl_tier(c->H, [&](auto r, auto t) {
        constexpr int R = decltype(r)::value;
        // part 0 runs on the first 256 threads whatever the width; a launch without a lambda_max part (the sweep's second) stays at 256
        const int nthr = (mode & (CTRL_PREV_END | CTRL_EIG_AHEAD | CTRL_EIG_BOLD)) ? eig_wide_launch(R, ca.spectral) : 256;
        if constexpr (decltype(t)::value == 16)
            hipLaunchKernelGGL((ctrl_chain_kernel<R>), dim3(parts), dim3(nthr), ctrl_lds_bytes_r(R), c->stream, ca);
    });
    HIPCHK(c, hipGetLastError());
    return VBMF_OK;
}

// one sweep from P = Y'B_old = G W_old (in gPQ) and the state's B'B: SigmaA, A (label mask) and A'A, SigmaB, then W and the product.
// The H x H chain runs in two launches of ctrl_chain_kernel, split as in the pass launches of the streaming sweep:
//   L1  part 0: [ctrl_end of the previous sweep] -> SigmaA (speculative, into the shadow)  |  part 1: [lambda_max(dB'dB) -> d, stop]
//                                                                                           |  part 2: lambda_max(B_old'B_old)
//   L2  part 0: commit of the shadow and of part 2's lambda_max -> SigmaB
// so the lambda_max solves leave the critical path.  L1 part 2 reads GB long before gram_part_reduce overwrites it.
// This sweep's closing step rides in the next sweep's L1, or is the run's stand-alone tail (vbmf_run).
static int gram_sweep(vbmf_ctx* c) {
    TRY(launch_chain(c, CTRL_COV_A | CTRL_EIG_AHEAD | (c->tail_pending ? CTRL_PREV_END : 0), c->SA32));
    if (c->tail_pending) ++c->ends_enqueued;
    c->tail_pending = false;
    c->P_frag = true;
    if (fused_gram(c)) TRY(launch_post_gram(c, 0, c->gPQ));
    else {
        TRY(launch_post_frag(c, 0, c->gPQ));
        TRY(launch_gram(c, 0, c->A32, nullptr, true));
    }
    TRY(launch_chain(c, CTRL_COMMIT_A | CTRL_COV_B, c->SB32));
    TRY(gram_product(c, true));
    c->wcur ^= 1;
    c->cache.gram_sweep_done_basic();
    return VBMF_OK;
}

// make st[GX] = tr(Y'BA') when the last B update did not leave it (state set by the caller, A changed since); *flag: legacy, 0
static int prepare_trYBA(vbmf_ctx* c, int* flag) {
    *flag = 0;
    if (c->cache.tr()) return VBMF_OK;
    double* dst = c->st + c->lay.GX();
    HIPCHK(c, hipMemsetAsync(dst, 0, sizeof(double), c->stream));
    // per-workgroup shares into c->ypart (scratch outside set_Y: <= 1024 of its 16384 doubles), folded in fixed order
    if (c->cache.P()) {
        const float* In = (sharded(c) || c->d1.nsplit > 1) ? c->Pred : c->P;
        const int ns = 1;
        const long long ld = (long long)c->d1.XT * 32;
        const int g = grid_for(c->M, 256, 1024);
        hipLaunchKernelGGL(dot_kernel, dim3(g), dim3(256), 0, c->stream, In, ld, ns,
                           (long long)c->Hp * ld, c->A32, c->Hp, (long long)c->M, c->ypart, c->P_frag ? c->NH : 0);
        hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, c->stream, c->ypart, g, dst);
    } else {
        TRY(launch_stream(c, 1));
        const long long ld = (long long)c->d2.XT * 32;
        const int g = grid_for(c->L, 256, 1024);
        hipLaunchKernelGGL(dot_kernel, dim3(g), dim3(256), 0, c->stream, c->Q, ld, c->d2.nsplit,
                           (long long)c->Hp * ld, c->B32[c->bcur], c->Hp, (long long)c->L, c->ypart, 0);
        hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, c->stream, c->ypart, g, dst);
        if (sharded(c)) TRY(allreduce_sum(c, dst, 1, true));
    }
    HIPCHK(c, hipGetLastError());
    c->cache.tr_made();
    return VBMF_OK;
}

// The reference's default eps = 1e-6 (src/vbmf.jl:175) sits at or below what d = ||B_old - B||_2 / ||B_old||_2 can resolve on the
// device: BHat is stored in fp32 (bf16x2 mode: as bf16 hi + lo, a 2^-17 grid), so near convergence d is the norm of a few one-ulp
// flips -- ~1e-6 (f32) / ~1e-5 (bf16x2) -- where the fp64 reference keeps falling.  A run that used all its sweeps with d still
// above such an eps is not an error, but the caller is told: the note is what vbmf_last_error returns after the OK.
static double d_resolution(const vbmf_ctx* c) { return c->mode == MODE_F32 ? 2e-6 : (c->mode == MODE_BF16X2 ? 1e-5 : 4e-3); }
static void run_note_eps(vbmf_ctx* c, int64_t niter, double eps, int64_t done, double d) {
    c->err.clear();
    if (done >= niter && eps > 0.0 && d > eps && eps < d_resolution(c)) {
        char b[400];
        snprintf(b, sizeof b, "note: all %lld sweeps ran and d = %.3g is still above eps = %.3g, which is below what d resolves in this "
                              "storage mode (~%.0e: BHat lives in %s); the fp64 reference may have stopped earlier -- use eps >= %.0e, "
                              "or fp32 storage", (long long)niter, d, eps, d_resolution(c),
                 c->mode == MODE_F32 ? "fp32" : (c->mode == MODE_BF16X2 ? "bf16 hi + lo" : "bf16"), d_resolution(c));
        c->err = b;
    }
}

// I_ERR on the device: 1 = a pivot of an H x H inverse was non-positive / non-finite, 2 = the register epilogue's bounded
// wait for the SigmaB table of its own launch gave up (stream_gemm.hpp)
static int device_err_status(vbmf_ctx* c, int e) {
    // bit 0x200: this rank's own kernels completed -- the error arrived with the packed Gram message of a row-sharded run
    // (ctrl_kernels.hpp, stop_on_remote_error): every rank stops at the same sweep and returns the same error class
    const char* where = (e & 0x200) ? " (reported by another rank of the row-sharded run; every rank stopped at that sweep)" : "";
    if ((e & 0xff) == 2) {
        // the epilogue left without touching B (stream_gemm.hpp), but A, SigmaA and the control scalars of that sweep are already
        // written: the device state is a mixture -- the handle asks for vbmf_set_state before it steps or runs again
        c->cache.state_mixed();
        FAIL(c, VBMF_ERR_SYNC, "in-launch hand-off timed out: the Y*A pass's register epilogue gave up waiting for the SigmaB "
                               "table of its own launch (bounded spin); this sweep's state is not valid, set the state again%s", where);
    }
    FAIL(c, VBMF_ERR_NUMERIC, "non-positive or non-finite pivot while inverting an H x H posterior precision%s", where);
}

// the fp32 row-major BHat from its operand tiles, after run loops that skipped the per-sweep fp32 store
static int rebuild_B32_if_stale(vbmf_ctx* c) {
    if (!c->cache.B32_stale()) return VBMF_OK;
    const int grid = (c->d2.XT + 3) / 4;
    const bool ok = dispatch<MODE_F32, MODE_BF16, MODE_BF16X2>(c->mode, [&](auto md) {
        return dispatch<1, 2, 4, 8>(c->NH, [&](auto nh) {
            hipLaunchKernelGGL((untile_factor_kernel<decltype(md)::value, decltype(nh)::value>), dim3(grid), dim3(256), 0, c->stream, c->FB,
                               c->B32[c->bcur], c->d2.XT);
        });
    });
    if (!ok) NO_KERNEL(c);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->cache.B32_rebuilt();
    return VBMF_OK;
}

static int check_device_err(vbmf_ctx* c) {
    HIPCHK(c, hipMemcpyAsync(c->ints_host, c->ints, 4 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->ints_host[I_ERR]) {
        const int e = c->ints_host[I_ERR];
        int zero = 0;
        memcpy_sync(c, c->ints + I_ERR, &zero, sizeof(int), hipMemcpyHostToDevice);
        return device_err_status(c, e);
    }
    return VBMF_OK;
}

// What vbmf_run and sparse_run_impl do around their (deliberately different) loops.  The frame owns the device trace: its
// destructor frees it on every path out of the run, early returns included.
struct RunFrame {
    vbmf_ctx* c;
    int64_t niter;
    double eps;
    int64_t* iters_done;
    double *d_last, *trace;
    DevScratch<double> trace_dev;
    int64_t done = -1;                                     // sweeps the device executed (-1: not read back)
    // the Gram form: whether this run takes it, the B and W buffers it started from, and the sweeps enqueued
    // by the streaming path (Gram form: at most the first)
    bool gram = false;
    int bstart = 0, wstart = 0;
    int64_t stream_sweeps = 0;

    // the device, the state, the callers' defaults
    int open() {
        HIPCHK(c, hipSetDevice(c->o.device));
        TRY(ensure_ready(c, true, false));                 // (B: only a run that starts by the streaming path needs it, see begin_gram)
        if (iters_done) *iters_done = 0;
        if (d_last) *d_last = eps + 1.0;                   // src/vbmf.jl:189, src/vbmf_sparse.jl:364
        return VBMF_OK;
    }
    // G = Y'Y is built here once per Y; a run that starts without a valid W does its first sweep by the streaming path, which starts
    // from B.  After open(), before arm().
    int begin_gram() {
        gram = gram_eligible(c);
        if (gram) TRY(gram_prepare(c));
        else c->cache.W_dropped();
        if (!(gram && c->cache.W())) TRY(ensure_B(c));
        bstart = c->bcur;
        wstart = c->wcur;
        return VBMF_OK;
    }
    // after the two updates of a streaming sweep: in the Gram form, W of this sweep and P = G W for the next one (the Grams of this
    // sweep came from the B update)
    int close_stream_sweep(int rc) {
        ++stream_sweeps;
        if (rc == VBMF_OK && gram) {
            rc = gram_product(c, false);
            c->wcur ^= 1;
            c->cache.W_made();
        }
        return rc;
    }
    // the trace buffer, the loop counters {stop, iters, err, niter} and the ranks' summed error flag
    int arm() {
        if (trace) {
            MEMCHK(c, trace_dev.alloc((size_t)niter * 4 * 8));
            HIPCHK(c, hipMemsetAsync(trace_dev, 0, (size_t)niter * 4 * 8, c->stream));
        }
        int init[4] = {0, 0, 0, (int)niter};
        HIPCHK(c, hipMemcpyAsync(c->ints, init, sizeof init, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(c->st + c->lay.GX() + 1, 0, sizeof(double), c->stream));   // the ranks' summed error flags (packed message)
        // the host's view of them, before the first launch: no flag of an earlier run is left (that run's stores are all complete,
        // finish() drained the stream)
        volatile int* w = c->loopw;
        w[I_STOP] = 0; w[I_ITERS] = 0; w[I_ERR] = 0;
        return VBMF_OK;
    }
    // The look at the device's stop and error flags after sweep `it` (a multiple of `check`) has been enqueued.  The device's loop test
    // stores {stop, iters, err} into host-mapped words (ctrl_kernels.hpp, publish_loop_words): nothing is queued on the compute
    // stream, the device never waits for the host, and the host sees a value late but never early.  The host in turn waits here
    // -- on memory, not on the stream -- until the device has finished sweep it - check, so it is never more than 2 * check sweeps
    // ahead: sweeps enqueued past the stop are no-ops on the device (every kernel tests the stop flag), at most 2 * check of them.
    // Returns true when the enqueueing ends.  Row-sharded: only the COLLECTIVE decision (the stop flag, raised at the same sweep on
    // every rank -- a rank's error reaches the others with the packed Gram message) may end it, or the ranks' all-reduce counts diverge.
    bool look(int64_t it, int64_t check) {
        volatile const int* w = c->loopw;
        auto t_last = std::chrono::steady_clock::now();
        int seen = -1;
        for (;;) {
            const int iters = w[I_ITERS];                  // iters before stop: the device stores them in the other order
            if (w[I_STOP] || (!sharded(c) && w[I_ERR])) return true;
            if (iters >= it - check) return false;
            const auto now = std::chrono::steady_clock::now();
            if (iters != seen) { seen = iters; t_last = now; }
            else if (now - t_last > std::chrono::milliseconds(200)) {
                // no sweep finished for a long time: is the stream still working?  (asked this rarely, the query costs nothing that matters)
                const hipError_t q = hipStreamQuery(c->stream);
                (void)hipGetLastError();                   // "not ready" must not surface behind the next launch
                if (q == hipSuccess) return w[I_STOP] || (!sharded(c) && w[I_ERR]);   // drained: the words are final
                if (q != hipErrorNotReady) return true;                               // finish() reports the failure
                t_last = now;
            }
            std::this_thread::yield();
        }
    }
    // drains both streams, reads back the counters and the 32 scalars, settles c->bcur (B moved in the first `b_sweeps` executed sweeps,
    // from buffer `bstart`), the fp32 B, the outputs and the trace, maps the device's error flag to a status, clears the counters;
    // Gram form: settles c->wcur (every executed sweep moved W) and what the run owes
    int finish(int rc, int bstart, int64_t b_sweeps) {
        c->in_run = false;
        c->use_side = false;
        c->side_pending = false;
        hipStreamSynchronize(c->side);
        hipStreamSynchronize(c->stream);
        if (rc == VBMF_OK) {
            hipError_t e = hipMemcpyAsync(c->ints_host, c->ints, 4 * sizeof(int), hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(c->scal_host, c->st + c->lay.scal(), 32 * 8, hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) { c->err = std::string("run readback: ") + hipGetErrorString(e); rc = VBMF_ERR_HIP; }
        }
        if (rc == VBMF_OK) {
            done = c->ints_host[I_ITERS];                  // sweeps after `stop` were no-ops on the device
            c->bcur = bstart ^ (int)(std::min<int64_t>(done, b_sweeps) & 1);
            rc = rebuild_B32_if_stale(c);                  // the fp32 factor from the tiles the last executed sweep wrote
            if (iters_done) *iters_done = done;
            if (d_last && done > 0) *d_last = c->scal_host[S_D];
            if (rc == VBMF_OK && trace && done > 0 && memcpy_sync(c, trace, trace_dev, (size_t)done * 4 * 8, hipMemcpyDeviceToHost) != hipSuccess) { c->err = "trace copy failed"; rc = VBMF_ERR_HIP; }
            const int e = c->ints_host[I_ERR];
            if (e && c->sparse) {
                c->err = std::string("non-positive or non-finite pivot while inverting the posterior precision of B") +
                         ((e & 0x200) ? " (reported by another rank of the row-sharded run; every rank stopped at that sweep)" : "");
                rc = VBMF_ERR_NUMERIC;
            } else if (e) {
                rc = device_err_status(c, e);
            } else if (rc == VBMF_OK) {
                run_note_eps(c, niter, eps, done, c->scal_host[S_D]);
            }
        }
        int zero4[4] = {0, 0, 0, 0};
        memcpy_sync(c, c->ints, zero4, sizeof zero4, hipMemcpyHostToDevice);
        trace_dev.reset();
        if (c->sparse) c->cache.run_ended_sparse(c->diagvar);
        else c->cache.run_ended_basic();
        if (gram) {
            int64_t gram_done = 0;                             // Gram-form sweeps the device executed
            if (done >= 0) {
                c->wcur = wstart ^ (int)(done & 1);
                gram_done = done - std::min<int64_t>(done, stream_sweeps);
            }
            c->cache.gram_run_ended(rc == VBMF_OK, gram_done > 0);
        }
        return rc;
    }
};

__global__ void logdet_kernel(double* st, StateLayout lay, int H, int which, int use_lds) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ int err;
    if (threadIdx.x == 0) err = 0;
    double* W = use_lds ? lds : (st + lay.W0());
    double* aux = use_lds ? (lds + (long long)H * H) : (st + lay.W1());
    const double* S = st + (which == 0 ? lay.SA() : lay.SB());
    for (int t = threadIdx.x; t < H * H; t += blockDim.x) W[t] = S[(long long)(t / H) * lay.Hp + (t % H)];
    __syncthreads();
    const double ld = gj_inverse_spd(W, H, aux, &err);
    __syncthreads();
    if (threadIdx.x == 0) st[lay.scal() + (which == 0 ? S_LOGDET_SA : S_LOGDET_SB)] = err ? -INFINITY : ld;
}

// ================================================================================================
extern "C" {

void vbmf_default_opts(vbmf_opts* o) {
    memset(o, 0, sizeof *o);
    o->struct_size = (int32_t)sizeof(vbmf_opts);
    o->y_dtype = VBMF_Y_BF16;
    o->factor_dtype = VBMF_FACTOR_AUTO;
    o->variant = VBMF_VARIANT_BASIC;
    o->reference_compat = VBMF_COMPAT_DEFAULT;
    o->nranks = 1;
}

const char* vbmf_last_error(const vbmf_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int vbmf_destroy(vbmf_ctx* c) {
    if (!c) return VBMF_OK;
    hipSetDevice(c->o.device);
    if (c->stream) hipStreamSynchronize(c->stream);
    prof_harvest(c);
    if (c->comm) ncclCommDestroy(c->comm);
    c->mem.release_all();
    if (c->ints_host) hipHostFree(c->ints_host);
    if (c->loopw) hipHostFree(c->loopw);
    if (c->scal_host) hipHostFree(c->scal_host);
    if (c->stream) hipStreamDestroy(c->stream);
    if (c->side) hipStreamDestroy(c->side);
    if (c->ev_main) hipEventDestroy(c->ev_main);
    if (c->ev_side) hipEventDestroy(c->ev_side);
    for (auto& e : c->ev_y) if (e) hipEventDestroy(e);
    delete c;
    return VBMF_OK;
}

int vbmf_create(vbmf_ctx** out, int64_t L, int64_t M, int64_t H, const vbmf_opts* opts) {
    if (!out) return VBMF_ERR_INVALID;
    *out = nullptr;
    vbmf_ctx* c = new vbmf_ctx();
    auto bail = [&](int code) { g_create_error = c->err; vbmf_destroy(c); return code; };
    if (opts) {
        if (opts->struct_size != (int32_t)sizeof(vbmf_opts)) { c->err = "vbmf_opts.struct_size mismatch"; return bail(VBMF_ERR_INVALID); }
        c->o = *opts;
    } else {
        vbmf_default_opts(&c->o);
    }
    if (L <= 0 || M <= 0 || H <= 0) { c->err = "L, M, H must be positive"; return bail(VBMF_ERR_INVALID); }
    if (H > 256) { c->err = "H > 256 is not supported"; return bail(VBMF_ERR_UNSUPPORTED); }
    if (c->o.variant != VBMF_VARIANT_BASIC && c->o.variant != VBMF_VARIANT_SPARSE_DIAG && c->o.variant != VBMF_VARIANT_SPARSE_DIAGVAR &&
        c->o.variant != VBMF_VARIANT_DUAL_DIAG && c->o.variant != VBMF_VARIANT_TRIAL_DIAG &&
        c->o.variant != VBMF_VARIANT_DUAL_DIAGVAR && c->o.variant != VBMF_VARIANT_TRIAL_DIAGVAR) {
        c->err = "unknown variant"; return bail(VBMF_ERR_INVALID);
    }
    c->sparse = (c->o.variant != VBMF_VARIANT_BASIC);
    c->diagvar = (c->o.variant == VBMF_VARIANT_SPARSE_DIAGVAR || c->o.variant == VBMF_VARIANT_DUAL_DIAGVAR ||
                  c->o.variant == VBMF_VARIANT_TRIAL_DIAGVAR);
    c->trial = (c->o.variant == VBMF_VARIANT_TRIAL_DIAG || c->o.variant == VBMF_VARIANT_TRIAL_DIAGVAR);
    c->dual = (c->o.variant == VBMF_VARIANT_DUAL_DIAG || c->o.variant == VBMF_VARIANT_DUAL_DIAGVAR) || c->trial;
    c->H0 = H;
    c->M0 = M;
    if (c->o.nranks < 1 || c->o.rank < 0 || c->o.rank >= c->o.nranks) { c->err = "bad nranks/rank"; return bail(VBMF_ERR_INVALID); }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        c->err = "no HIP device visible: this library has no CPU fallback (MI355X / gfx950 required)";
        return bail(VBMF_ERR_NO_DEVICE);
    }
    if (c->o.device < 0 || c->o.device >= ndev) { c->err = "bad device ordinal"; return bail(VBMF_ERR_INVALID); }
    hipDeviceProp_t prop;
    if (hipSetDevice(c->o.device) != hipSuccess || hipGetDeviceProperties(&prop, c->o.device) != hipSuccess) {
        c->err = "hipSetDevice/hipGetDeviceProperties failed"; return bail(VBMF_ERR_NO_DEVICE);
    }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        c->err = std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only";
        return bail(VBMF_ERR_NO_DEVICE);
    }
    c->L = L; c->M = M; c->H = H;
    c->Lg = c->o.L_global > 0 ? c->o.L_global : L;
    if (c->o.nranks == 1 && c->Lg != L) { c->err = "L_global != L with nranks == 1"; return bail(VBMF_ERR_INVALID); }
    c->Hp = (int)rup(H, 32);
    if (c->Hp == 96) c->Hp = 128;
    if (c->Hp > 128 && c->Hp < 256) c->Hp = 256;
    c->NH = c->Hp / 32;
    if (const char* e = getenv("VBMF_XCD_MAP")) c->xcd_map = atoi(e) != 0;      // A/B switch for the tuning record
    if (const char* e = getenv("VBMF_GRAM")) {          // Gram-form sweep: force off / on / on for the ARD-sparse model too (gram_eligible)
        const int v = atoi(e);
        c->gram_env = v == 0 ? 0 : (v == 2 || v == 3 ? v : 1);   // 3: VBMF_GRAM_FORM_ON from creation on
    }
    if (const char* e = getenv("VBMF_EPI_BALANCE")) c->epi_balance = atoi(e) != 0;
    if (const char* e = getenv("VBMF_LDS8")) c->lds8 = atoi(e) != 0;
    if (const char* e = getenv("VBMF_POST3")) c->post3 = atoi(e) != 0;
    if (const char* e = getenv("VBMF_SPARSE_A_FUSED")) c->sparse_a_fused = atoi(e) != 0;
    // H >= 128: one Gram workgroup per chunk (gram_tiles_kernel): enough chunks to fill the chip, few enough that the
    // fp64 reduction over the chunks' dense H x H slabs stays small (it was 412 us at 1M rows with 16-tile chunks)
    c->tiles_per_chunk = c->NH >= 4 ? (int)std::max<int64_t>(16, cdiv(cdiv(std::max(L, M), 32), 384)) : 32;
    if (c->o.y_dtype == VBMF_Y_F32) {
        if (c->o.factor_dtype != VBMF_FACTOR_AUTO) { c->err = "f32 Y takes f32 factor operands (factor_dtype must be AUTO)"; return bail(VBMF_ERR_INVALID); }
        c->mode = MODE_F32;
    } else if (c->o.y_dtype == VBMF_Y_BF16) {
        // single-bf16 factor operands carry ~3 significant digits: a speed option whose stated tolerance (factors 4e-2,
        // sigma2 only loosely) holds up to rank 128 in the GPU suite; at H = 200 on rank-8 data the residual
        // ||Y||^2 - 2 tr + tr(..) falls below that noise and sigma2 comes out 157x off after three sweeps.  Refused above 128.
        if (c->o.factor_dtype == VBMF_FACTOR_BF16 && H > VBMF_FACTOR_BF16_MAX_H) {
            c->err = "factor_dtype VBMF_FACTOR_BF16 (single bf16 rounding of the factor operand) is supported up to H = 128; "
                     "use VBMF_FACTOR_BF16X2 (hi + lo) or fp32 storage at this rank";
            return bail(VBMF_ERR_UNSUPPORTED);
        }
        c->mode = (c->o.factor_dtype == VBMF_FACTOR_BF16) ? MODE_BF16 : MODE_BF16X2;
    } else { c->err = "bad y_dtype"; return bail(VBMF_ERR_INVALID); }
    c->kstep = kstep_of(c->mode);
    c->npart = npart_of(c->mode);
    const double ybytes = c->mode == MODE_F32 ? 4.0 : 2.0;
    {   // narrow geometry when a pass of the wide one would have at most two column groups (VBMF_NARROW=0|1 forces it off|on).
        // Measured (scripts/narrow_ab.sh): 10k x 1k, H = 32: 9 795 -> 11 724 sweeps/s; row shards of 100k x 10k (20+ column
        // groups): no gain at 12.5k rows, 12 % slower at 25k and 50k rows -- hence the rule on the group count, not on bytes.
        const char* ev = getenv("VBMF_NARROW");
        const int wq = nxw_of(c->NH) * 4 * 32;                      // columns per workgroup of the wide geometry
        // Every rank of a row-sharded job must take the SAME decision (the padded width of the all-reduced Y'B partial
        // depends on it), so the row count that enters is the nominal shard size, not this rank's.
        const int64_t Lnom = cdiv(c->Lg, c->o.nranks);
        const int64_t groups = std::min(cdiv(M, wq), cdiv(Lnom, wq));
        c->narrow = c->NH <= 2 && (ev ? atoi(ev) != 0 : groups <= 2);
    }
    // lambda_max at H <= 64: the repeated squaring unless asked otherwise (VBMF_EXACT_LAMBDA=1: the Lanczos iteration every larger rank
    // uses, exact inside eigenvalue clusters too).  Measured at the headline (scripts/r03_exact_ab.sh, profiles/r03_k_lambda_max.txt): the
    // Lanczos chain inside the pass launches costs 0.3 % (200 sweeps) to 0.6 % (the driver's 20: the last sweep's stand-alone tail) of the
    // sweep rate and moves `d` in no digit a comparison shows; on narrow problems and short row shards, where the chain is the critical
    // path, 40 %.  A switch for every rank of a job alike (the loop-test decisions must agree).
    if (const char* e = getenv("VBMF_EXACT_LAMBDA")) c->exact_lambda = atoi(e) != 0;
    plan_pass(c->d1, M, L, c->kstep, c->NH, c->Hp, ybytes, c->o.pass1_splits, c->narrow, 0, !use_lds8(c));
    plan_pass(c->d2, L, M, c->kstep, c->NH, c->Hp, ybytes, 0, c->narrow, (c->NH == 2 && !c->narrow) ? VBMF_EPI_DY : 0);
    c->Mp = (int64_t)c->d1.XT * 32;
    c->Lp = (int64_t)c->d2.XT * 32;
    // the post kernel writes operand tiles for every 32-row tile of the factor: the consumer's KS must cover them
    if ((int64_t)c->d1.KS * c->kstep < c->Lp || (int64_t)c->d2.KS * c->kstep < c->Mp) { c->err = "internal: tile plan"; return bail(VBMF_ERR_INVALID); }
    c->lay.Hp = c->Hp;

    // (the fill runs on the null stream: see the hipDeviceSynchronize that closes this function)
#define ALLOC(ptr, bytes)                                                                       \
    do {                                                                                        \
        const int _m = c->mem.acquire((ptr), (bytes));                                          \
        if (_m != 0) { c->err = std::string("hipMalloc failed for " #ptr ": ") + mem_errstr(_m); return bail(VBMF_ERR_HIP); } \
        if (hipMemset((ptr), 0, (bytes)) != hipSuccess) { c->err = "hipMemset failed"; return bail(VBMF_ERR_HIP); } \
    } while (0)

    const size_t slack = (size_t)PIPE_D * 64;
    c->nY1 = (size_t)c->d1.XT * c->d1.KS * 64 + slack * 2;
    c->nY2 = (size_t)c->d2.XT * c->d2.KS * 64 + slack * 2;
    // factor tiles: PIPE_D zero k-steps in front (the streaming kernel's lead-in reads steps -DF..-1) and behind
    const size_t flead = (size_t)PIPE_D * c->npart * c->NH * 64;
    c->nFB = ((size_t)c->d1.KS + PIPE_D) * c->npart * c->NH * 64;
    c->nFA = ((size_t)c->d2.KS + PIPE_D) * c->npart * c->NH * 64;
    ALLOC(c->Y1, c->nY1 * 16);
    ALLOC(c->Y2, c->nY2 * 16);
    ALLOC(c->FB_alloc, (c->nFB + flead) * 16);
    if (c->NH >= 4 && c->mode != MODE_F32) ALLOC(c->SBf, (size_t)c->NH * 2 * c->NH * VBMF_POST_NT * 64 * 16);
    if (c->NH >= 4 && c->mode != MODE_F32 && !c->diagvar)
        ALLOC(c->FD, ((size_t)c->d1.KS + PIPE_D) * 2 * c->NH * 64 * 16);
    ALLOC(c->FA_alloc, (c->nFA + flead) * 16);
    c->FB = c->FB_alloc + flead;
    c->FA = c->FA_alloc + flead;
    ALLOC(c->P, (size_t)c->d1.nsplit * c->Hp * c->Mp * 4);
    {   // Segment-list plan of the Y*A pass (LDS-DMA kernel, un-split, the last round of workgroups mostly empty): whole blocks
        // for the full rounds, then the R remaining blocks cut T ways in k, pieces k-major (stream_gemm.hpp, SK)
        const char* ev = getenv("VBMF_STREAMK");
        const int xpw = c->NH == 8 ? 8 : 16;                                   // x tiles per workgroup of stream_lds8_kernel
        const int bps2 = cdiv(c->d2.XT, xpw), nst = c->d2.steps_per_split / 2;
        const int nfull = bps2 / NUM_CU * NUM_CU, R = bps2 - nfull;
        // OFF unless VBMF_STREAMK=1 -- measured, not faster (profiles/r03_g_segment_list_ab.txt): config 5's Y*A pass 0.80 ms + a
        // 0.04 ms fix-up against 0.83 ms for the plain two rounds (391 blocks on 254 CUs, nominally 77 % efficient).  Alone, a full round
        // of 254 workgroups takes 0.48 ms and the second round of 137 only 0.34 (fewer workgroups in flight run faster each): the schedule's
        // idle CUs cost ~80 us against a perfect balance, far less than their count says (profiles/r03_i_pass2_probes.txt).  (An earlier cut at arbitrary stages,
        // every workgroup at its own k, was 25 % SLOWER: the factor then comes from beyond L2.)  Kept as a tested switch.
        if (use_lds8(c) && c->d2.nsplit == 1 && nfull > 0 && R > 0 && (double)R / NUM_CU < 0.8 && (ev && atoi(ev) == 1)) {
            int bestT = 0;
            double best = 0.93;                                                // time of the last round, in whole-block times (1.0 un-cut)
            for (int T : {2, 3, 4, 5}) {
                if (nst / T < 6) break;                                        // a piece keeps >= 6 stages (pipeline fill / drain per piece)
                const double t = (double)cdiv((int64_t)R * T, NUM_CU) / T;
                if (t < best - 1e-9) { best = t; bestT = T; }
            }
            if (bestT > 0) {
                std::vector<int> seg, tails;
                for (int b = 0; b < nfull; ++b) { seg.push_back(b); seg.push_back(0); seg.push_back(nst); seg.push_back(0); }
                for (int t = 0; t < bestT; ++t)
                    for (int b = nfull; b < bps2; ++b) {
                        const int s0 = (int)((int64_t)nst * t / bestT), s1 = (int)((int64_t)nst * (t + 1) / bestT);
                        seg.push_back(b); seg.push_back(s0); seg.push_back(s1 - s0); seg.push_back(t);
                    }
                for (int b = nfull; b < bps2; ++b) tails.push_back(b);
                c->sk_per = bestT; c->sk_grid = (int)(seg.size() / 4); c->sk_ntail = (int)tails.size();
                ALLOC(c->sk_list, seg.size() * sizeof(int));
                ALLOC(c->sk_tail, tails.size() * sizeof(int));
                if (hipMemcpy(c->sk_list, seg.data(), seg.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
                    hipMemcpy(c->sk_tail, tails.data(), tails.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
                    c->err = "segment-list plan upload failed"; return bail(VBMF_ERR_HIP);
                }
            }
        }
    }
    ALLOC(c->Q, (size_t)(c->sk_per > 0 ? c->sk_per : c->d2.nsplit) * c->Hp * c->Lp * 4);
    ALLOC(c->Pred, (size_t)c->Hp * c->Mp * 4);
    ALLOC(c->A32, (size_t)c->Mp * c->Hp * 4);
    ALLOC(c->B32[0], (size_t)c->Lp * c->Hp * 4);
    ALLOC(c->B32[1], (size_t)c->Lp * c->Hp * 4);
    ALLOC(c->SA32, (size_t)c->Hp * c->Hp * 4);
    ALLOC(c->SB32, (size_t)c->Hp * c->Hp * 4);
    // every chunking any Gram launcher can use: the per-side choice of gram_tiles_per_chunk() AND the context-wide
    // tiles_per_chunk of the dense-slab kernel (weighted_gram_B of full_cov + diag_var runs it in every storage mode)
    const int nchunk = std::max(std::max(cdiv(c->d1.XT, gram_tiles_per_chunk(c, 0)), cdiv(c->d2.XT, gram_tiles_per_chunk(c, 1))),
                                std::max(cdiv(c->d1.XT, c->tiles_per_chunk), cdiv(c->d2.XT, c->tiles_per_chunk)));
    // Gram partial slabs: one per chunk (generic path), per post_gram workgroup (<= 256), or per pass-2 workgroup when the
    // pass carries the register epilogue (capped at 1024 slabs = 24 MB; longer shards use the separate post kernel)
    {
        const int epi_blocks = (c->NH <= 2) ? std::min(1024, (c->d2.XT / nxw_of(c->NH) + 3) / 4) : 0;
        c->gslab_cap = std::max(256, epi_blocks);
        c->gslab_bytes = std::max((size_t)nchunk * 2 * c->Hp * c->Hp * 4, (size_t)c->gslab_cap * 2 * 3 * 1024 * 4);
        ALLOC(c->gslab, c->gslab_bytes);
    }
    ALLOC(c->st, (size_t)c->lay.total() * 8);
    ALLOC(c->gtmp, ((size_t)2 * c->Hp * c->Hp + 8) * 8);
    c->trpart_cap = 4 * std::max(c->gslab_cap, (c->d2.XT + 3) / 4 + 1);
    ALLOC(c->trpart, (size_t)c->trpart_cap * 8);
    ALLOC(c->ypart, (size_t)16384 * 8);
    ALLOC(c->ints, 32 * sizeof(int));          // [0..7] flags, [8..15] control-chain stamps, [16..23] epilogue stamps
    ALLOC(c->mask, (size_t)c->Mp);
    if (c->sparse) {
        ALLOC(c->dS32, (size_t)c->Mp * c->Hp * 4);
        ALLOC(c->CA32, (size_t)c->Mp * c->Hp * 4);
        ALLOC(c->beta32, (size_t)c->Mp * c->Hp * 4);
        ALLOC(c->vtab, (size_t)c->Hp * 8);
    }
    if (c->dual) {
        c->gpart_blocks = grid_for((int64_t)c->M * c->Hp);
        ALLOC(c->gpart, (size_t)c->gpart_blocks * 6 * 8);
    }
    if (c->diagvar) {
        ALLOC(c->sigv, (size_t)c->Lp * 8);
        ALLOC(c->zetav, (size_t)c->Lp * 8);
        ALLOC(c->yrow, (size_t)c->Lp * 8);
        ALLOC(c->hpart, (size_t)cdiv(c->Lp, 256) * 8 + 64);
        ALLOC(c->hmean, 2 * 8);                    // [this rank's share of mean(sigmaVecHat) | its sum over the ranks]
        ALLOC(c->vsq, (size_t)c->Hp * 8);
        ALLOC(c->sig32, (size_t)c->Lp * 4);
        ALLOC(c->G32, (size_t)c->Hp * c->Hp * 4);
        ALLOC(c->FBs_alloc, (c->nFB + flead) * 16);
        c->FBs = c->FBs_alloc + flead;
    }
#undef ALLOC
    if (hipHostMalloc((void**)&c->ints_host, 16 * sizeof(int)) != hipSuccess ||
        hipHostMalloc((void**)&c->scal_host, 32 * sizeof(double)) != hipSuccess) {
        c->err = "pinned alloc failed"; return bail(VBMF_ERR_HIP);
    }
    // the run loops' host-mapped words: fine-grained (coherent), so the device's stores reach the host while the kernel still runs
    if (hipHostMalloc((void**)&c->loopw, 16 * sizeof(int), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer((void**)&c->loopw_dev, c->loopw, 0) != hipSuccess) {
        c->err = "host-mapped alloc failed"; return bail(VBMF_ERR_HIP);
    }
    memset(c->loopw, 0, 16 * sizeof(int));
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { c->err = "stream create failed"; return bail(VBMF_ERR_HIP); }
    if (hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_main, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_side, hipEventDisableTiming) != hipSuccess) { c->err = "side stream create failed"; return bail(VBMF_ERR_HIP); }
    // large dynamic LDS (160 KiB per CU on gfx950) for the lambda_max kernel at 64 < H <= 128
    c->lds_limit = 160 * 1024 - 16384;         // leaves room for the kernels' static LDS (ctrl_end's tables: 8.4 KB)
    {
        const int lim = c->lds_limit, vb = (int)vbls_lds_bytes(4), fb = (int)FITB_LDS_CAP;
        const struct { const void* kernel; int bytes; int nh; } big_lds[] = {        // nh: the context's NH the row applies to (0: any)
            {(const void*)eig_kernel<8>, lim, 0},
            // 64 < H <= 128: the blocked inverse keeps the 128 x 130 fp64 image in LDS (133 KB)
            {(const void*)ctrl_cov_kernel<8, 16>, lim, 0},
            {(const void*)ctrl_chain_kernel<8>, lim, 0},
            {(const void*)sparse_cov_b_kernel<8, 16>, lim, 0},
            // 128 < H <= 256: the register-resident blocked sweep's two panel strips (70 KB: above the 64 KB a launch may ask for unannounced)
            {(const void*)ctrl_cov_kernel<8, 32>, lim, 0}, {(const void*)sparse_cov_b_kernel<8, 32>, lim, 0},
            {(const void*)sparse_update_a_full256_kernel, lim, 0},
            // full_cov A update at H <= 64, one column per wavefront: a wavefront's image and column (19 / 70 / 134 KB per workgroup)
            {(const void*)sparse_update_a_full_wave_kernel<1, 8>, (int)full_a_wave_lds_bytes(1, 8), 0},
            {(const void*)sparse_update_a_full_wave_kernel<2, 8>, (int)full_a_wave_lds_bytes(2, 8), 0},
            {(const void*)sparse_update_a_full_wave_kernel<4, 4>, (int)full_a_wave_lds_bytes(4, 4), 0},
            // vbls! as H x H algebra at 32 < H <= 64: four 64 x 66 fp64 images (135 KB)
            {(const void*)vbls_loop_kernel<4>, vb, 0}, {(const void*)vbls_batch_kernel<4>, vb, 0},
            // batched vbls! of the sparse models, full_cov at 32 < H <= 64: four 64 x 66 fp64 images and the bag's state
            {(const void*)sparse_batch_kernel<4, true>, (int)SBATCH_LDS_BIG, 0},
            // many fits in one launch: the images, the H x H matrices and a fit's state (fit_batch_kernels.hpp)
            {(const void*)fit_batch_kernel<1, false>, fb, 0}, {(const void*)fit_batch_kernel<1, true>, fb, 0},
            {(const void*)fit_batch_kernel<2, false>, fb, 0}, {(const void*)fit_batch_kernel<2, true>, fb, 0},
            // ... and their three-group / masked twins (vbmf_local_fit_batched)
            {(const void*)fit_batch_kernel<1, false, true>, fb, 0}, {(const void*)fit_batch_kernel<1, true, true>, fb, 0},
            {(const void*)fit_batch_kernel<2, false, true>, fb, 0}, {(const void*)fit_batch_kernel<2, true, true>, fb, 0},
            // ... and the row-noise sweeps built on those (vbmf_rows_fit_batched)
            {(const void*)fit_batch_kernel<1, false, true, true>, fb, 0}, {(const void*)fit_batch_kernel<1, true, true, true>, fb, 0},
            {(const void*)fit_batch_kernel<2, false, true, true>, fb, 0}, {(const void*)fit_batch_kernel<2, true, true, true>, fb, 0},
            // ... and one fit over many workgroups: the column pass and the fold (vbmf_ard_fit_batched_form, fit_split_kernels.hpp)
            {(const void*)fit_cols_kernel<1, false, false>, fb, 0}, {(const void*)fit_cols_kernel<1, true, false>, fb, 0},
            {(const void*)fit_cols_kernel<2, false, false>, fb, 0}, {(const void*)fit_cols_kernel<2, true, false>, fb, 0},
            {(const void*)fit_cols_kernel<1, false, true>, fb, 0}, {(const void*)fit_cols_kernel<1, true, true>, fb, 0},
            {(const void*)fit_cols_kernel<2, false, true>, fb, 0}, {(const void*)fit_cols_kernel<2, true, true>, fb, 0},
            {(const void*)fit_fold_kernel<1, false>, fb, 0}, {(const void*)fit_fold_kernel<2, false>, fb, 0},
            {(const void*)fit_fold_kernel<1, true>, fb, 0}, {(const void*)fit_fold_kernel<2, true>, fb, 0},
            {(const void*)fit_basic_kernel<1>, fb, 0}, {(const void*)fit_basic_kernel<2>, fb, 0},
            {(const void*)fit_basic_gram_kernel<1>, fb, 0}, {(const void*)fit_basic_gram_kernel<2>, fb, 0},
            {(const void*)stream_lds8_kernel<4, StreamCfg<4>::Rc, false>, LDS8_BYTES, 4},
            {(const void*)stream_lds8_kernel<4, StreamCfg<4>::Rc, true>, LDS8_BYTES, 4},
            {(const void*)stream_lds8_kernel<8, 0, false>, LDS8_BYTES, 8}, {(const void*)stream_lds8_kernel<8, 0, true>, LDS8_BYTES, 8},
            // the Gram-form product's W / D plane buffers and G rings (148 / 144 / 144 KB at NH = 1 / 2 / 4)
            {(const void*)gram_prod_kernel<1>, GramProd<1>::LDS_BYTES, 1},
            {(const void*)gram_prod_kernel<2>, GramProd<2>::LDS_BYTES, 2},
            {(const void*)gram_prod_kernel<4>, GramProd<4>::LDS_BYTES, 4},
            {(const void*)gram_prod_kernel<4, 8>, GramProd<4>::LDS_BYTES, 8},          // rank 256: two h-tile groups of the NH = 4 geometry
        };
        hipError_t e = hipSuccess;
        for (const auto& r : big_lds)
            if (e == hipSuccess && (r.nh == 0 || r.nh == c->NH))
                e = hipFuncSetAttribute(r.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, r.bytes);
        if (e == hipSuccess && c->NH == 4) {
            using Cfg = StreamCfg<4>;
            dispatch<MODE_F32, MODE_BF16, MODE_BF16X2>(c->mode, [&](auto md) {
                e = hipFuncSetAttribute((const void*)stream_gemm_kernel<decltype(md)::value, 4, Cfg::NXWc, Cfg::DYc, Cfg::DFc, Cfg::Rc>,
                                        hipFuncAttributeMaxDynamicSharedMemorySize, c->lds_limit);
            });
        }
        if (e != hipSuccess) { c->err = "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed"; return bail(VBMF_ERR_HIP); }
    }
    // the zero-fills above ran on the null stream; all later work runs on a non-blocking stream
    // that does not order against it, so drain the device once here
    if (hipDeviceSynchronize() != hipSuccess) { c->err = "hipDeviceSynchronize failed"; return bail(VBMF_ERR_HIP); }
    *out = c;
    return VBMF_OK;
}

// ---- Y -----------------------------------------------------------------------------------------
}  // extern "C"

// Tiles of both copies from a source functor: fragments [xa, xb) x [ka, kb) of the pass-1 copy (r1) and of the pass-2 copy (r2).
// ||.||^2 of the stored values is taken on the pass-2 copy and ADDED to *sumsq.
struct TileRange { int xa, xb, ka, kb; };
template <class Src>
static int launch_tiles(vbmf_ctx* c, const Src& src, TileRange r1, TileRange r2, double* sumsq) {
    const int64_t n1 = (int64_t)(r1.xb - r1.xa) * (r1.kb - r1.ka) * 64, n2 = (int64_t)(r2.xb - r2.xa) * (r2.kb - r2.ka) * 64;
    dispatch<MODE_F32, MODE_BF16>(ymode_of(c->mode), [&](auto ym) {
        constexpr int TM = decltype(ym)::value;
        hipLaunchKernelGGL((tile_y_kernel<TM, false, Src>), dim3(grid_for(n1, 256, 16384)), dim3(256), 0, c->stream, c->Y1,
                           src, r1.xa, r1.xb, r1.ka, r1.kb, c->d1.KS, (double*)nullptr);
        const int g2 = grid_for(n2, 256, 16384);
        hipLaunchKernelGGL((tile_y_kernel<TM, true, Src>), dim3(g2), dim3(256), 0, c->stream, c->Y2,
                           src, r2.xa, r2.xb, r2.ka, r2.kb, c->d2.KS, sumsq ? c->ypart : nullptr);
        if (sumsq) hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, c->stream, c->ypart, g2, sumsq);
    });
    HIPCHK(c, hipGetLastError());
    return VBMF_OK;
}

template <class Src>
static int build_tiles(vbmf_ctx* c, const Src& src, int64_t m0, int64_t m1, double* sumsq) {
    // pass-1 copy: x tiles covering columns [m0,m1), all k-steps; pass-2 copy: all x tiles, k-steps of [m0,m1)
    const int xt0 = (int)(m0 / 32), xt1 = (m1 >= c->M) ? c->d1.XT : (int)(m1 / 32);
    const int ks0 = (int)(m0 / c->kstep), ks1 = (m1 >= c->M) ? c->d2.KS : (int)(m1 / c->kstep);
    return launch_tiles(c, src, TileRange{xt0, xt1, 0, c->d1.KS}, TileRange{0, c->d2.XT, ks0, ks1}, sumsq);
}

template <class Src>
static int build_tiles_rows(vbmf_ctx* c, const Src& src, int64_t l0, int64_t l1, double* sumsq) {
    // rows [l0,l1), l0 a multiple of 32 and l1 one too unless l1 = L.  pass-1 copy: all x tiles, k-steps of the rows; pass-2 copy:
    // x tiles of the rows, all k-steps.  The block that ends at L also writes every pad tile behind it, as build_tiles does.
    const int ks0 = (int)(l0 / c->kstep), ks1 = (l1 >= c->L) ? c->d1.KS : (int)(l1 / c->kstep);
    const int xt0 = (int)(l0 / 32), xt1 = (l1 >= c->L) ? c->d2.XT : (int)(l1 / 32);
    return launch_tiles(c, src, TileRange{0, c->d1.XT, ks0, ks1}, TileRange{xt0, xt1, 0, c->d2.KS}, sumsq);
}

// rows [l0, l1) from a device buffer with one unit stride: both copies from one read (tile_pair_kernel)
template <class T>
static int launch_tile_pair(vbmf_ctx* c, const T* dev, int64_t l0, int64_t l1, int64_t rs, int64_t cs, double* sumsq) {
    const bool last = l1 >= c->L;
    const int ks = c->kstep;
    // what this block of rows owns: in the pass-1 copy all x tiles and the rows' k-steps, in the pass-2 copy the rows' x tiles and all
    // k-steps; the block that ends at L owns every pad tile behind it (build_tiles_rows)
    const int k1a = (int)(l0 / ks), k1b = last ? c->d1.KS : (int)(l1 / ks);
    const int x2a = (int)(l0 / 32), x2b = last ? c->d2.XT : (int)(l1 / 32);
    const int64_t l_end = last ? std::max<int64_t>((int64_t)c->d2.XT * 32, (int64_t)c->d1.KS * ks) : l1;
    const int64_t m_end = std::max<int64_t>((int64_t)c->d1.XT * 32, (int64_t)c->d2.KS * ks);
    PairGeom g;
    uint4 *outA, *outB;
    if (cs == 1) {                                     // row-major: s = row, u = column; copy A = pass 2 (x = l), copy B = pass 1 (x = m)
        g.ss = rs; g.s_org = l0; g.u_org = 0; g.s_lo = l0; g.s_hi = l1; g.u_lo = 0; g.u_hi = c->M; g.s0 = l0; g.u0 = 0;
        g.ns = (int)cdiv(l_end - l0, 32); g.nu = (int)cdiv(m_end, PAIR_U);
        g.xa0 = x2a; g.xa1 = x2b; g.ka0 = 0; g.ka1 = c->d2.KS; g.KSA = c->d2.KS; outA = c->Y2;
        g.xb0 = 0; g.xb1 = c->d1.XT; g.kb0 = k1a; g.kb1 = k1b; g.KSB = c->d1.KS; outB = c->Y1;
    } else {                                           // column-major: s = column, u = row; copy A = pass 1, copy B = pass 2
        g.ss = cs; g.s_org = 0; g.u_org = l0; g.s_lo = 0; g.s_hi = c->M; g.u_lo = l0; g.u_hi = l1; g.s0 = 0; g.u0 = l0;
        g.ns = (int)cdiv(m_end, 32); g.nu = (int)cdiv(l_end - l0, PAIR_U);
        g.xa0 = 0; g.xa1 = c->d1.XT; g.ka0 = k1a; g.ka1 = k1b; g.KSA = c->d1.KS; outA = c->Y1;
        g.xb0 = x2a; g.xb1 = x2b; g.kb0 = 0; g.kb1 = c->d2.KS; g.KSB = c->d2.KS; outB = c->Y2;
    }
    const int grid = (int)std::min<int64_t>((int64_t)g.ns * g.nu, 16384);   // c->ypart holds 16384 partials
    dispatch<MODE_F32, MODE_BF16>(ymode_of(c->mode), [&](auto ym) {
        constexpr int TM = decltype(ym)::value;
        hipLaunchKernelGGL((tile_pair_kernel<TM, T>), dim3(grid), dim3(256), 0, c->stream, outA, outB, dev, g, c->ypart);
        hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, c->stream, c->ypart, grid, sumsq);
    });
    HIPCHK(c, hipGetLastError());
    return VBMF_OK;
}

template <class T>
static int tile_rows_typed(vbmf_ctx* c, const T* dev, int64_t l0, int64_t n, int64_t rs, int64_t cs, double* tr) {
    // one unit stride: both copies from one coalesced read (2.2-3.0 ms against 4.5-5.3 ms at 100k x 10k, profiles/set_y_sources.txt);
    // general strides: tile_y_kernel gathers once per copy
    if (rs == 1 || cs == 1) return launch_tile_pair(c, dev, l0, l0 + n, rs, cs, tr);
    return build_tiles_rows(c, StridedSrc<T>{dev, rs, cs, l0, l0 + n, c->M}, l0, l0 + n, tr);
}

// tiles of rows [l0, l0+n) from a DEVICE buffer whose element (0, 0) is row l0
static int tile_rows_from(vbmf_ctx* c, const void* dev, int dt, int64_t l0, int64_t n, int64_t rs, int64_t cs, double* tr) {
    if (dt == VBMF_SRC_F64) return tile_rows_typed(c, (const double*)dev, l0, n, rs, cs, tr);
    if (dt == VBMF_SRC_F32) return tile_rows_typed(c, (const float*)dev, l0, n, rs, cs, tr);
    return tile_rows_typed(c, (const __bf16*)dev, l0, n, rs, cs, tr);
}

static int finish_Y(vbmf_ctx* c) {
    double* tr = c->st + c->lay.scal() + S_TRYY;
    HIPCHK(c, hipMemcpyAsync(c->scal_host, tr, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->trYY_local = c->scal_host[0];
    c->cache.Y_complete(!sharded(c) && c->o.nranks == 1);
    c->y_rows = c->L;
    if (c->diagvar) {                                  // ||Y_l||^2 of every row (:310), from the stored values
        dispatch<MODE_F32, MODE_BF16>(ymode_of(c->mode), [&](auto ym) {
            constexpr int TM = decltype(ym)::value;
            hipLaunchKernelGGL((row_sumsq_kernel<TM>), dim3((c->d2.XT + 3) / 4), dim3(256), 0, c->stream, c->Y2, c->d2.XT, c->d2.KS,
                               (long long)c->L, c->yrow);
        });
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return VBMF_OK;
}

extern "C" {

int vbmf_set_Y(vbmf_ctx* c, const double* Y, int64_t ldY) {
    if (!c) return VBMF_ERR_INVALID;
    if (!Y || ldY < c->L) FAIL(c, VBMF_ERR_INVALID, "vbmf_set_Y: null Y or ldY < L");
    HIPCHK(c, hipSetDevice(c->o.device));
    double* tr = c->st + c->lay.scal() + S_TRYY;
    HIPCHK(c, hipMemsetAsync(tr, 0, sizeof(double), c->stream));
    int64_t mc = std::max<int64_t>(32, ((int64_t)(256ll << 20) / (c->L * 8)) / 32 * 32);
    mc = std::min<int64_t>(mc, rup(c->M, 32));
    DevScratch<double> stage;
    MEMCHK(c, stage.alloc((size_t)c->L * mc * 8));
    for (int64_t m0 = 0; m0 < c->M; m0 += mc) {
        const int64_t m1 = std::min(c->M, m0 + mc);
        const hipError_t e = hipMemcpy2DAsync(stage, (size_t)c->L * 8, Y + m0 * ldY, (size_t)ldY * 8, (size_t)c->L * 8,
                                              (size_t)(m1 - m0), hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) FAIL(c, VBMF_ERR_HIP, "hipMemcpy2DAsync: %s", hipGetErrorString(e));
        ColMajorF64Src src{stage.get(), c->L, m0, m1 - m0, c->L, c->M};
        TRY(build_tiles(c, src, m0, m1, tr));
        if (hipStreamSynchronize(c->stream) != hipSuccess) FAIL(c, VBMF_ERR_HIP, "sync failed in vbmf_set_Y");
    }
    stage.reset();                                     // (before finish_Y's launches, where it has always been freed)
    return finish_Y(c);
}

// ---- Y from the columns of another context's Y (get_matrices, examples/mil_util.jl:46) -------------------------------------------
int vbmf_set_Y_gather(vbmf_ctx* c, vbmf_ctx* s, const int64_t* col_index, int64_t ncols) {
    if (!c) { g_create_error = "vbmf_set_Y_gather: NULL dst"; return VBMF_ERR_INVALID; }
    // every refusal comes before the first launch or copy and leaves dst, its current Y included, as it was
    if (!s) FAIL(c, VBMF_ERR_INVALID, "vbmf_set_Y_gather: NULL src");
    if (!col_index) FAIL(c, VBMF_ERR_INVALID, "vbmf_set_Y_gather: NULL col_index");
    if (c == s) FAIL(c, VBMF_ERR_INVALID, "vbmf_set_Y_gather: dst and src are the same context");
    if (c->o.nranks > 1 || s->o.nranks > 1 || sharded(c) || sharded(s))
        FAIL(c, VBMF_ERR_UNSUPPORTED, "vbmf_set_Y_gather: row-sharded contexts (nranks > 1 or a communicator) are not supported");
    if (ncols != c->M) FAIL(c, VBMF_ERR_INVALID, "vbmf_set_Y_gather: ncols = %lld, dst has M = %lld columns", (long long)ncols, (long long)c->M);
    if (s->L != c->L) FAIL(c, VBMF_ERR_INVALID, "vbmf_set_Y_gather: src has L = %lld rows, dst has L = %lld", (long long)s->L, (long long)c->L);
    if (s->o.y_dtype != c->o.y_dtype)
        FAIL(c, VBMF_ERR_INVALID, "vbmf_set_Y_gather: src stores Y as y_dtype %d, dst as y_dtype %d", (int)s->o.y_dtype, (int)c->o.y_dtype);
    if (s->o.device != c->o.device) FAIL(c, VBMF_ERR_INVALID, "vbmf_set_Y_gather: src lives on device %d, dst on device %d", s->o.device, c->o.device);
    if (!s->cache.have_Y()) FAIL(c, VBMF_ERR_INVALID, "vbmf_set_Y_gather: src has no complete Y");
    if (s->M > (int64_t)INT32_MAX) FAIL(c, VBMF_ERR_INVALID, "vbmf_set_Y_gather: src has M = %lld columns, more than an int32 index names", (long long)s->M);
    std::vector<int> idx((size_t)ncols);               // the whole table is checked here: no kernel ever sees a bad index
    for (int64_t m = 0; m < ncols; ++m) {
        if (col_index[m] < 0 || col_index[m] >= s->M)
            FAIL(c, VBMF_ERR_INVALID, "vbmf_set_Y_gather: col_index[%lld] = %lld outside 0..%lld", (long long)m, (long long)col_index[m], (long long)(s->M - 1));
        idx[(size_t)m] = (int)col_index[m];
    }
    HIPCHK(c, hipSetDevice(c->o.device));
    HIPCHK(c, hipStreamSynchronize(s->stream));        // whatever still writes src's tiles has finished
    DevScratch<int> table;
    MEMCHK(c, table.alloc((size_t)ncols * sizeof(int)));
    HIPCHK(c, hipMemcpyAsync(table, idx.data(), (size_t)ncols * sizeof(int), hipMemcpyHostToDevice, c->stream));
    double* tr = c->st + c->lay.scal() + S_TRYY;
    HIPCHK(c, hipMemsetAsync(tr, 0, sizeof(double), c->stream));
    // the column chunks of vbmf_set_Y, so that the partials of ||Y||^2 have its shape and are summed in its order
    int64_t mc = std::max<int64_t>(32, ((int64_t)(256ll << 20) / (c->L * 8)) / 32 * 32);
    mc = std::min<int64_t>(mc, rup(c->M, 32));
    const GatherSrc src{s->Y2, table.get(), s->d2.KS, ymode_of(c->mode) == MODE_F32, c->L, c->M};
    for (int64_t m0 = 0; m0 < c->M; m0 += mc) TRY(build_tiles(c, src, m0, std::min(c->M, m0 + mc), tr));
    if (hipStreamSynchronize(c->stream) != hipSuccess) FAIL(c, VBMF_ERR_HIP, "sync failed in vbmf_set_Y_gather");
    table.reset();
    return finish_Y(c);
}

// ---- Y from the caller's own dtype, layout and memory, in row blocks ------------------------------------------------------------
static size_t src_elem_size(int dt) { return dt == VBMF_SRC_F64 ? 8 : dt == VBMF_SRC_F32 ? 4 : 2; }

int vbmf_set_Y_rows(vbmf_ctx* c, const void* src, int32_t dt, int32_t on_device, int64_t row0, int64_t nrows, int64_t rs, int64_t cs) {
    if (!c) return VBMF_ERR_INVALID;
    // every refusal comes before the first launch or copy and leaves the context, its current Y included, as it was
    if (!src) FAIL(c, VBMF_ERR_INVALID, "vbmf_set_Y_rows: null source");
    if (dt != VBMF_SRC_F64 && dt != VBMF_SRC_F32 && dt != VBMF_SRC_BF16) FAIL(c, VBMF_ERR_INVALID, "vbmf_set_Y_rows: unknown src_dtype %d", (int)dt);
    if (rs <= 0 || cs <= 0) FAIL(c, VBMF_ERR_INVALID, "vbmf_set_Y_rows: strides must be positive");
    if (row0 < 0 || nrows <= 0 || row0 % 32 != 0 || nrows > c->L - row0 || (nrows % 32 != 0 && row0 + nrows != c->L))
        FAIL(c, VBMF_ERR_INVALID, "vbmf_set_Y_rows: rows [%lld, %lld) of %lld: a block starts at a multiple of 32 and ends at one or at L",
             (long long)row0, (long long)(row0 + nrows), (long long)c->L);
    if (row0 != 0 && (c->cache.have_Y() || row0 != c->y_rows))
        FAIL(c, VBMF_ERR_INVALID, "vbmf_set_Y_rows: blocks come in ascending, contiguous order (row0 = %lld, the next block starts at %lld)",
             (long long)row0, (long long)(c->cache.have_Y() ? 0 : c->y_rows));
    const size_t es = src_elem_size(dt);
    if (!on_device) {
        if (rs != 1 && cs != 1) FAIL(c, VBMF_ERR_INVALID, "vbmf_set_Y_rows: a host source needs row_stride = 1 or col_stride = 1");
        // the staged 2-D copy takes whole lines of the unit-stride dimension: they must not overlap
        if (cs == 1 ? (rs < c->M && nrows > 1) : (cs < nrows && c->M > 1))
            FAIL(c, VBMF_ERR_INVALID, "vbmf_set_Y_rows: the host source's lines overlap (the other stride is shorter than a line)");
    }
    HIPCHK(c, hipSetDevice(c->o.device));
    {   // what kind of memory is it?  A wrong pointer comes back as an error code: no kernel and no copy ever reads it.
        hipPointerAttribute_t at;
        hipError_t e = hipPointerGetAttributes(&at, src);
        if (e != hipSuccess) (void)hipGetLastError();                  // memory the runtime has never seen: plain host memory
        const bool is_dev = e == hipSuccess && (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged);
        if (on_device) {
            if (!is_dev) FAIL(c, VBMF_ERR_INVALID, "vbmf_set_Y_rows: src_on_device is set but src is not device memory");
            if (at.device != c->o.device) FAIL(c, VBMF_ERR_INVALID, "vbmf_set_Y_rows: src lives on device %d, the context on device %d", at.device, c->o.device);
            const unsigned __int128 last = (unsigned __int128)(nrows - 1) * (unsigned __int128)rs + (unsigned __int128)(c->M - 1) * (unsigned __int128)cs;
            hipDeviceptr_t base = nullptr;
            size_t size = 0;
            e = hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)src);
            if (e != hipSuccess) { (void)hipGetLastError(); FAIL(c, VBMF_ERR_INVALID, "vbmf_set_Y_rows: src belongs to no device allocation"); }
            const uintptr_t b = (uintptr_t)base, p = (uintptr_t)src;
            if (p < b || p - b > size || (last + 1) * es > (unsigned __int128)(size - (p - b)))
                FAIL(c, VBMF_ERR_INVALID, "vbmf_set_Y_rows: the strided extent of the block leaves its device allocation");
        } else if (e == hipSuccess && at.type == hipMemoryTypeDevice) {
            FAIL(c, VBMF_ERR_INVALID, "vbmf_set_Y_rows: src is device memory but src_on_device is 0");
        }
    }
    if (!c->ev_y[0]) { HIPCHK(c, hipEventCreate(&c->ev_y[0])); HIPCHK(c, hipEventCreate(&c->ev_y[1])); }
    HIPCHK(c, hipEventRecord(c->ev_y[0], c->stream));
    double* tr = c->st + c->lay.scal() + S_TRYY;
    if (row0 == 0) {                                   // a new Y begins: none until its last block has arrived
        c->cache.Y_begins();
        c->y_rows = 0;
        HIPCHK(c, hipMemsetAsync(tr, 0, sizeof(double), c->stream));
    }
    if (on_device) {
        TRY(tile_rows_from(c, src, dt, row0, nrows, rs, cs, tr));
    } else {
        // staged in the source's own dtype and order, whole 32-row groups per chunk of at most 256 MB (one group if that is larger)
        const bool rowmajor = cs == 1;
        int64_t rc = std::max<int64_t>(32, ((int64_t)(256ll << 20) / (c->M * (int64_t)es)) / 32 * 32);
        rc = std::min<int64_t>(rc, rup(nrows, 32));
        DevScratch<void> stage;
        MEMCHK(c, stage.alloc((size_t)rc * c->M * es));
        for (int64_t r = 0; r < nrows; r += rc) {
            const int64_t n = std::min(rc, nrows - r);
            const char* from = (const char*)src + (size_t)r * rs * es;
            const hipError_t e = rowmajor ? hipMemcpy2DAsync(stage, (size_t)c->M * es, from, (size_t)rs * es, (size_t)c->M * es, (size_t)n, hipMemcpyHostToDevice, c->stream)
                                          : hipMemcpy2DAsync(stage, (size_t)n * es, from, (size_t)cs * es, (size_t)n * es, (size_t)c->M, hipMemcpyHostToDevice, c->stream);
            if (e != hipSuccess) FAIL(c, VBMF_ERR_HIP, "vbmf_set_Y_rows: hipMemcpy2DAsync: %s", hipGetErrorString(e));
            TRY(rowmajor ? tile_rows_from(c, stage, dt, row0 + r, n, c->M, 1, tr) : tile_rows_from(c, stage, dt, row0 + r, n, 1, n, tr));
            if (hipStreamSynchronize(c->stream) != hipSuccess) FAIL(c, VBMF_ERR_HIP, "sync failed in vbmf_set_Y_rows");
        }
    }
    HIPCHK(c, hipEventRecord(c->ev_y[1], c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));        // the caller may reuse its buffer once this returns
    float ms = 0.0f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev_y[0], c->ev_y[1]));
    c->set_y_ms = ms;
    c->y_rows = row0 + nrows;
    return c->y_rows == c->L ? finish_Y(c) : VBMF_OK;
}

// ---- preprocess (src/util.jl:36-54, 73-86) fused into the upload ---------------------------------
struct vbmf_prep {
    int device = 0;
    int64_t L = 0, M = 0, L_used = 0;
    double* Y = nullptr;            // resident fp64 copy, column-major, ld = L
    double *mu = nullptr, *den = nullptr;
    long long* rows = nullptr;      // kept rows (device)
    std::vector<int64_t> rows_host;
    std::vector<double> mu_host, den_host;
    MemOwner<HipMem> mem;           // owns Y, mu, den, rows (ctx_mem.hpp)
};

int vbmf_preprocess_open(vbmf_prep** out, int device, const double* Y, int64_t L, int64_t M, int64_t ldY, int64_t* L_used) {
    if (!out || !Y || L <= 0 || M <= 0 || ldY < L) return VBMF_ERR_INVALID;
    *out = nullptr;
    if (hipSetDevice(device) != hipSuccess) { g_create_error = "vbmf_preprocess_open: bad device"; return VBMF_ERR_NO_DEVICE; }
    vbmf_prep* p = new vbmf_prep();
    p->device = device; p->L = L; p->M = M;
    DevScratch<double> part, rowsum;
    DevScratch<unsigned char> keep;
    auto bail = [&](const char* what) { g_create_error = std::string("vbmf_preprocess_open: ") + what; delete p; return VBMF_ERR_HIP; };
    if (p->mem.acquire(p->Y, (size_t)L * M * 8) != 0) return bail("device allocation of the fp64 copy failed");
    if (p->mem.acquire(p->mu, (size_t)L * 8) != 0 || p->mem.acquire(p->den, (size_t)L * 8) != 0 ||
        rowsum.alloc((size_t)L * 8) != 0 || keep.alloc((size_t)L) != 0 ||
        part.alloc((size_t)PREP_CHUNKS * L * 8) != 0) return bail("allocation failed");
    if (hipMemcpy2D(p->Y, (size_t)L * 8, Y, (size_t)ldY * 8, (size_t)L * 8, (size_t)M, hipMemcpyHostToDevice) != hipSuccess) return bail("upload failed");
    const dim3 g((unsigned)((L + 255) / 256), PREP_CHUNKS), gf((unsigned)((L + 255) / 256));
    double* outs[3] = {p->mu, p->den, rowsum.get()};
    for (int what = 0; what < 3; ++what) {
        hipLaunchKernelGGL(prep_row_partial_kernel, g, dim3(256), 0, 0, p->Y, (long long)L, (long long)M, (long long)L, what, p->mu, p->den, part.get());
        hipLaunchKernelGGL(prep_row_fold_kernel, gf, dim3(256), 0, 0, part.get(), (long long)L, (long long)M, what, outs[what], keep.get());
    }
    std::vector<unsigned char> kh((size_t)L);
    p->mu_host.resize((size_t)L); p->den_host.resize((size_t)L);
    if (hipMemcpy(kh.data(), keep, (size_t)L, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(p->mu_host.data(), p->mu, (size_t)L * 8, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(p->den_host.data(), p->den, (size_t)L * 8, hipMemcpyDeviceToHost) != hipSuccess) return bail("statistics kernels failed");
    for (int64_t l = 0; l < L; ++l) if (kh[(size_t)l]) p->rows_host.push_back(l);
    p->L_used = (int64_t)p->rows_host.size();
    if (p->mem.acquire(p->rows, std::max<size_t>(8, (size_t)p->L_used * 8)) != 0) return bail("allocation failed");
    if (p->L_used && hipMemcpy(p->rows, p->rows_host.data(), (size_t)p->L_used * 8, hipMemcpyHostToDevice) != hipSuccess) return bail("upload failed");
    hipDeviceSynchronize();                         // (null-stream work above; the context that consumes p runs on its own stream)
    part.reset(); keep.reset(); rowsum.reset();
    if (L_used) *L_used = p->L_used;
    *out = p;
    return VBMF_OK;
}

int vbmf_preprocess_rows(const vbmf_prep* p, int64_t* used_rows0, double* mu, double* den) {
    if (!p) return VBMF_ERR_INVALID;
    if (used_rows0) memcpy(used_rows0, p->rows_host.data(), (size_t)p->L_used * 8);
    if (mu) memcpy(mu, p->mu_host.data(), (size_t)p->L * 8);
    if (den) memcpy(den, p->den_host.data(), (size_t)p->L * 8);
    return VBMF_OK;
}

int vbmf_preprocess_close(vbmf_prep* p) {
    if (!p) return VBMF_ERR_INVALID;
    hipSetDevice(p->device);
    p->mem.release_all();
    delete p;
    return VBMF_OK;
}

int vbmf_set_Y_preprocessed(vbmf_ctx* c, const vbmf_prep* p, double lambda) {
    if (!c || !p) return VBMF_ERR_INVALID;
    if (p->device != c->o.device) FAIL(c, VBMF_ERR_INVALID, "vbmf_set_Y_preprocessed: plan lives on another device");
    if (p->M != c->M) FAIL(c, VBMF_ERR_INVALID, "vbmf_set_Y_preprocessed: M mismatch");
    if (c->Lg != p->L_used || c->o.row_offset < 0 || c->o.row_offset + c->L > p->L_used)
        FAIL(c, VBMF_ERR_INVALID, "vbmf_set_Y_preprocessed: the context (or, row-sharded, L_global) must have the plan's kept-row count %lld",
             (long long)p->L_used);
    HIPCHK(c, hipSetDevice(c->o.device));
    HIPCHK(c, hipDeviceSynchronize());                      // the plan's kernels ran on the null stream
    double* tr = c->st + c->lay.scal() + S_TRYY;
    HIPCHK(c, hipMemsetAsync(tr, 0, sizeof(double), c->stream));
    PrepSrc src{p->Y, (long long)p->L, p->rows, p->mu, p->den, lambda, (long long)c->L, (long long)c->M, (long long)c->o.row_offset};
    TRY(build_tiles(c, src, 0, c->M, tr));
    return finish_Y(c);
}

int vbmf_set_Y_synthetic(vbmf_ctx* c, uint64_t seed, int64_t Hstar, double noise_std) {
    if (!c) return VBMF_ERR_INVALID;
    if (Hstar <= 0) FAIL(c, VBMF_ERR_INVALID, "Hstar must be positive");
    HIPCHK(c, hipSetDevice(c->o.device));
    double* tr = c->st + c->lay.scal() + S_TRYY;
    HIPCHK(c, hipMemsetAsync(tr, 0, sizeof(double), c->stream));
    SynthSrc src{SynthGen{seed, (long long)Hstar, (long long)c->M, (float)noise_std}, c->L, c->M, c->o.row_offset};
    TRY(build_tiles(c, src, 0, c->M, tr));
    return finish_Y(c);
}

int vbmf_get_Y(vbmf_ctx* c, double* Y, int64_t ldY, int64_t row0, int64_t nrows) {
    if (!c) return VBMF_ERR_INVALID;
    if (!c->cache.have_Y()) FAIL(c, VBMF_ERR_INVALID, "no Y");
    if (!Y || row0 < 0 || nrows <= 0 || row0 + nrows > c->L || ldY < nrows) FAIL(c, VBMF_ERR_INVALID, "vbmf_get_Y: bad range");
    HIPCHK(c, hipSetDevice(c->o.device));
    // column chunks of a multiple of 32 (= whole k-steps of the pass-2 copy)
    int64_t mc = std::max<int64_t>(32, ((int64_t)(256ll << 20) / (nrows * 8)) / 32 * 32);
    mc = std::min<int64_t>(mc, rup(c->M, 32));
    DevScratch<double> tmp;
    MEMCHK(c, tmp.alloc((size_t)nrows * mc * 8));
    for (int64_t m0 = 0; m0 < c->M; m0 += mc) {
        const int64_t m1 = std::min(c->M, m0 + mc);
        // shifting the tile pointer by whole k-steps makes the kernel's column 0 equal to column m0
        const uint4* base = c->Y2 + (size_t)(m0 / c->kstep) * 64;
        dispatch<MODE_F32, MODE_BF16>(ymode_of(c->mode), [&](auto ym) {
            constexpr int TM = decltype(ym)::value;
            hipLaunchKernelGGL((untile_y_kernel<TM>), dim3(grid_for(nrows * (m1 - m0))), dim3(256), 0, c->stream, base,
                               tmp.get(), (long long)nrows, (long long)row0, (long long)nrows, (long long)(m1 - m0), c->d2.KS);
        });
        hipError_t e = hipMemcpy2DAsync(Y + m0 * ldY, (size_t)ldY * 8, tmp, (size_t)nrows * 8, (size_t)nrows * 8,
                                        (size_t)(m1 - m0), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) FAIL(c, VBMF_ERR_HIP, "vbmf_get_Y copy failed: %s", hipGetErrorString(e));
    }
    return VBMF_OK;
}

int vbmf_get_trYY(vbmf_ctx* c, double* trYY) {
    if (!c || !trYY) return VBMF_ERR_INVALID;
    if (!c->cache.have_Y()) FAIL(c, VBMF_ERR_INVALID, "no Y");
    HIPCHK(c, hipSetDevice(c->o.device));
    if (!c->cache.trYY_reduced()) { *trYY = c->trYY_local; return VBMF_OK; }     // this rank's part until the first step/run
    HIPCHK(c, hipMemcpyAsync(c->scal_host, c->st + c->lay.scal() + S_TRYY, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *trYY = c->scal_host[0];
    return VBMF_OK;
}

// ---- state -------------------------------------------------------------------------------------
static int upload_factor(vbmf_ctx* c, const double* src, int64_t ld, int64_t X, int64_t Xp, float* dst) {
    DevScratch<double> tmp;
    MEMCHK(c, tmp.alloc((size_t)X * c->H * 8));
    hipError_t e = hipMemcpy2DAsync(tmp, (size_t)X * 8, src, (size_t)ld * 8, (size_t)X * 8, (size_t)c->H,
                                    hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(pack_factor_kernel, dim3(grid_for(Xp * c->Hp)), dim3(256), 0, c->stream, tmp.get(), (long long)X,
                           (long long)X, (int)c->H, c->Hp, (long long)Xp, dst);
        e = hipStreamSynchronize(c->stream);
    }
    if (e != hipSuccess) FAIL(c, VBMF_ERR_HIP, "factor upload failed: %s", hipGetErrorString(e));
    return VBMF_OK;
}
static int download_factor(vbmf_ctx* c, const float* src, int64_t X, double* dst, int64_t ld) {
    DevScratch<double> tmp;
    MEMCHK(c, tmp.alloc((size_t)X * c->H * 8));
    hipLaunchKernelGGL(unpack_factor_kernel, dim3(grid_for(X * c->H)), dim3(256), 0, c->stream, src, c->Hp, (long long)X,
                       (int)c->H, tmp.get(), (long long)X);
    hipError_t e = hipMemcpy2DAsync(dst, (size_t)ld * 8, tmp, (size_t)X * 8, (size_t)X * 8, (size_t)c->H,
                                    hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) FAIL(c, VBMF_ERR_HIP, "factor download failed: %s", hipGetErrorString(e));
    return VBMF_OK;
}

static int upload_small(vbmf_ctx* c, const double* srcHxH, long long off, bool matrix) {
    // H x H column-major (ld=H) -> Hp-strided block; symmetric matrices, so row/column-major agree
    std::vector<double> buf(matrix ? (size_t)c->Hp * c->Hp : (size_t)c->Hp, matrix ? 0.0 : 1.0);
    if (matrix) {
        for (int64_t j = 0; j < c->H; ++j)
            for (int64_t i = 0; i < c->H; ++i) buf[(size_t)i * c->Hp + j] = srcHxH[i + j * c->H];
    } else {
        for (int64_t i = 0; i < c->H; ++i) buf[i] = srcHxH[i];
    }
    HIPCHK(c, memcpy_sync(c, c->st + off, buf.data(), buf.size() * 8, hipMemcpyHostToDevice));
    return VBMF_OK;
}

int vbmf_set_state(vbmf_ctx* c, const double* AHat, int64_t ldA, const double* BHat, int64_t ldB,
                   const double* SigmaA, const double* SigmaB, const double* CA_diag, const double* CB_diag,
                   double sigma2, const int64_t* labels0, int64_t nlabels, int64_t H1) {
    if (!c) return VBMF_ERR_INVALID;
    if (c->sparse) FAIL(c, VBMF_ERR_INVALID, "sparse context: use vbmf_sparse_set_state");
    if (!AHat || !BHat || !SigmaA || !SigmaB || !CA_diag || !CB_diag) FAIL(c, VBMF_ERR_INVALID, "vbmf_set_state: null pointer");
    if (ldA < c->M || ldB < c->L) FAIL(c, VBMF_ERR_INVALID, "vbmf_set_state: leading dimension too small");
    if (H1 < 0 || H1 > c->H || nlabels < 0 || (nlabels > 0 && !labels0)) FAIL(c, VBMF_ERR_INVALID, "vbmf_set_state: bad H1/labels");
    if (!(sigma2 > 0.0)) FAIL(c, VBMF_ERR_INVALID, "vbmf_set_state: sigma2 must be positive");
    for (int64_t h = 0; h < c->H; ++h)
        if (!(CA_diag[h] > 0.0) || !(CB_diag[h] > 0.0)) FAIL(c, VBMF_ERR_INVALID, "vbmf_set_state: CA/CB diagonals must be positive");
    HIPCHK(c, hipSetDevice(c->o.device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->bcur = 0;
    TRY(upload_factor(c, AHat, ldA, c->M, c->Mp, c->A32));
    TRY(upload_factor(c, BHat, ldB, c->L, c->Lp, c->B32[0]));
    TRY(upload_small(c, SigmaA, c->lay.SA(), true));
    TRY(upload_small(c, SigmaB, c->lay.SB(), true));
    TRY(upload_small(c, CA_diag, c->lay.ca(), false));
    TRY(upload_small(c, CB_diag, c->lay.cb(), false));
    HIPCHK(c, memcpy_sync(c, c->st + c->lay.scal() + S_SIGMA2, &sigma2, 8, hipMemcpyHostToDevice));
    std::vector<unsigned char> mk((size_t)c->Mp, 0);
    for (int64_t i = 0; i < nlabels; ++i) {
        if (labels0[i] < 0 || labels0[i] >= c->M) FAIL(c, VBMF_ERR_INVALID, "vbmf_set_state: label %lld out of range", (long long)labels0[i]);
        mk[(size_t)labels0[i]] = 1;
    }
    HIPCHK(c, memcpy_sync(c, c->mask, mk.data(), mk.size(), hipMemcpyHostToDevice));
    c->H1 = H1;
    c->has_mask = (nlabels > 0 && H1 > 0);
    TRY(launch_retile(c, 0));
    TRY(launch_retile(c, 1));
    const int H = (int)c->H;
    const size_t need = ((size_t)H * H + 2 * H) * sizeof(double);
    const int use_lds = need <= 60 * 1024;
    for (int w = 0; w < 2; ++w)
        hipLaunchKernelGGL(logdet_kernel, dim3(1), dim3(ctrl_threads(H)), use_lds ? need : 0, c->stream, c->st, c->lay, H, w, use_lds);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemsetAsync(c->ints, 0, 16 * sizeof(int), c->stream));
    if (c->dbg_sb_ppm) HIPCHK(c, hipMemcpyAsync(c->ints + I_DBG_SB_PPM, &c->dbg_sb_ppm, sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->cache.state_set_basic();
    return VBMF_OK;
}

int vbmf_get_state(vbmf_ctx* c, double* AHat, int64_t ldA, double* BHat, int64_t ldB, double* SigmaA,
                   double* SigmaB, double* CA_diag, double* CB_diag, double* sigma2) {
    if (!c) return VBMF_ERR_INVALID;
    if (!c->cache.have_state()) FAIL(c, VBMF_ERR_INVALID, "no state");
    HIPCHK(c, hipSetDevice(c->o.device));
    if (BHat) TRY(ensure_B(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (AHat) { if (ldA < c->M) FAIL(c, VBMF_ERR_INVALID, "ldA < M"); TRY(download_factor(c, c->A32, c->M, AHat, ldA)); }
    if (BHat) { if (ldB < c->L) FAIL(c, VBMF_ERR_INVALID, "ldB < L"); TRY(download_factor(c, c->B32[c->bcur], c->L, BHat, ldB)); }
    std::vector<double> buf((size_t)c->lay.total());
    HIPCHK(c, memcpy_sync(c, buf.data(), c->st, buf.size() * 8, hipMemcpyDeviceToHost));
    auto mat = [&](long long off, double* dst) {
        if (!dst) return;
        for (int64_t j = 0; j < c->H; ++j)
            for (int64_t i = 0; i < c->H; ++i) dst[i + j * c->H] = buf[(size_t)off + (size_t)i * c->Hp + j];
    };
    mat(c->lay.SA(), SigmaA);
    mat(c->lay.SB(), SigmaB);
    if (CA_diag) for (int64_t i = 0; i < c->H; ++i) CA_diag[i] = buf[(size_t)c->lay.ca() + i];
    if (CB_diag) for (int64_t i = 0; i < c->H; ++i) CB_diag[i] = buf[(size_t)c->lay.cb() + i];
    if (sigma2) *sigma2 = buf[(size_t)c->lay.scal() + S_SIGMA2];
    return VBMF_OK;
}

// ---- updates -----------------------------------------------------------------------------------
int vbmf_step(vbmf_ctx* c, int which) {
    if (!c) return VBMF_ERR_INVALID;
    if (c->sparse) FAIL(c, VBMF_ERR_INVALID, "sparse context: use vbmf_sparse_step");
    if (which & ~31) FAIL(c, VBMF_ERR_INVALID, "vbmf_step: unknown update bits");
    HIPCHK(c, hipSetDevice(c->o.device));
    TRY(ensure_ready(c, (which & (VBMF_STEP_A | VBMF_STEP_B | VBMF_STEP_SIGMA2)) != 0));
    c->cache.W_dropped();
    if (which & VBMF_STEP_A) TRY(do_update_A(c));
    if (which & VBMF_STEP_B) TRY(do_update_B(c));
    int flags = 0;
    if (which & VBMF_STEP_CA) { TRY(ensure_gram_A(c)); flags |= 1; }
    if (which & VBMF_STEP_CB) { TRY(ensure_gram_B(c)); flags |= 2; }
    if (which & VBMF_STEP_SIGMA2) {
        TRY(ensure_gram_A(c));
        TRY(ensure_gram_B(c));
        int f = 0;
        TRY(prepare_trYBA(c, &f));
        flags |= 4 | f;
    }
    if (flags) {
        if (!(flags & 4)) { TRY(ensure_gram_A(c)); TRY(ensure_gram_B(c)); }
        TRY(launch_ctrl_end(c, flags, 0.0, nullptr));
    }
    return check_device_err(c);
}

// vbls! (examples/mil_util.jl:179-203), vbmf_parameters branch: niter x (updateA!, updateCA!, updateSigma2!) with
// B, SigmaB, CB frozen.  B is fixed, so Y'B is formed ONCE (one pass over Y for the whole call, where the reference
// reads Y twice per iteration) and tr(Y'BA') is the dot product of that M x H matrix with AHat.
int vbmf_run_fixed_basis(vbmf_ctx* c, int64_t niter) {
    if (!c) return VBMF_ERR_INVALID;
    if (c->sparse) FAIL(c, VBMF_ERR_INVALID, "sparse context: use vbmf_sparse_run_fixed_basis");
    if (niter < 0 || niter > (1ll << 30)) FAIL(c, VBMF_ERR_INVALID, "vbmf_run_fixed_basis: bad niter");
    HIPCHK(c, hipSetDevice(c->o.device));
    TRY(ensure_ready(c));
    c->cache.W_dropped();
    // Without a label mask the loop is H x H algebra on S = P'P (ctrl_kernels.hpp, vbls_loop_kernel): the first iteration runs the
    // general way (it forms P = Y'B), the rest in ONE launch of one workgroup, and A is formed once at the end.  H <= 64.
    // (VBMF_VBLS_LOOP=0: every iteration the general way -- the A/B switch of profiles/r03_f_vbls_mil.txt)
    const char* ev = getenv("VBMF_VBLS_LOOP");
    const bool fast = !c->has_mask && c->NH <= 2 && niter >= 3 && !(ev && atoi(ev) == 0);
    for (int64_t it = 0; it < (fast ? 1 : niter); ++it) {
        TRY(do_update_A(c, true));
        TRY(ensure_gram_A(c));
        int f = 0;
        TRY(prepare_trYBA(c, &f));                          // P is current: the dot(P, A) branch
        TRY(launch_ctrl_end(c, 1 | 4 | f, 0.0, nullptr));
        if ((it & 63) == 63) TRY(check_device_err(c));      // bounds the launch queue
    }
    if (fast) {
        const int H = (int)c->H, n2 = c->Hp * c->Hp;
        const float* Psrc = (sharded(c) || c->d1.nsplit > 1) ? c->Pred : c->P;
        // S = P'P: the A update with the identity as its table leaves A = P and A'A = S in the state (the Gram of what the post
        // kernel stores, like every other Gram of the sweep)
        hipLaunchKernelGGL(identity_table_kernel, dim3(cdiv(n2, 256)), dim3(256), 0, c->stream, c->SA32, H, c->Hp);
        TRY(launch_post_gram(c, 0, Psrc));
        hipLaunchKernelGGL(copy_doubles_kernel, dim3(cdiv(n2, 256)), dim3(256), 0, c->stream, c->st + c->lay.GA(), c->st + c->lay.W1(), n2);
        const size_t lds = vbls_lds_bytes(nb_tier(H));         // (the attribute for NB = 4: vbmf_create)
        dispatch<1, 2, 4>(nb_tier(H), [&](auto nbk) {
            hipLaunchKernelGGL((vbls_loop_kernel<decltype(nbk)::value>), dim3(1), dim3(256), lds, c->stream, c->st, c->lay, H, (double)c->Lg, (double)c->M,
                               (int)(niter - 1), c->SA32, c->ints);
        });
        HIPCHK(c, hipGetLastError());
        TRY(launch_post_gram(c, 0, Psrc));                  // A = P SigmaA / sigma2 of the last updateA!, its tiles and A'A
        c->cache.A_moved_by_vbls_loop();
    }
    return check_device_err(c);
}

int vbmf_run(vbmf_ctx* c, int64_t niter, double eps, int est_covs, int est_var, int64_t* iters_done,
             double* d_last, double* trace) {
    if (!c) return VBMF_ERR_INVALID;
    if (c->sparse) FAIL(c, VBMF_ERR_INVALID, "sparse context: use vbmf_sparse_run");
    if (niter < 0 || niter > (1ll << 30)) FAIL(c, VBMF_ERR_INVALID, "vbmf_run: bad niter");
    RunFrame run{c, niter, eps, iters_done, d_last, trace};
    TRY(run.open());
    if (niter == 0) return VBMF_OK;
    TRY(run.begin_gram());
    TRY(run.arm());
    // ||B_old||_2 of the first comparison (src/vbmf.jl:187-188: old = params.BHat): in the fused schedule
    // every sweep's pass-2 launch computes it; otherwise once here, then rotated by ctrl_end
    int rc = ensure_gram_B(c);
    const bool fused_run = (c->NH <= 4);
    if (rc == VBMF_OK && !fused_run) {
        rc = launch_eig(c, 0, 1);
        if (rc == VBMF_OK)
            hipLaunchKernelGGL(copy_scalar_kernel, dim3(1), dim3(1), 0, c->stream, c->st, c->lay, (int)S_LAMB_PREV, (int)S_LAMB_NEW);
    }
    const int flags = (est_covs ? 3 : 0) | (est_var ? 4 : 0) | 8 | 16;
    c->in_run = true;
    c->ends_enqueued = 0;
    c->tail_pending = false;
    c->run_flags = flags;
    c->run_eps = eps;
    c->run_trace = run.trace_dev;
    // The host runs ahead of the device; every `check` sweeps it looks at the device's stop/error flags in host-mapped words
    // (RunFrame::look: nothing enters the stream, the device never waits for the host).  Sweeps enqueued past the stop are
    // no-ops on the device (every kernel tests the stop flag): at most 2*check of them.
    const int64_t check = 8;
    int64_t it = 0;
    bool stopped = false;
    while (rc == VBMF_OK && it < niter && !stopped) {
        if (run.gram && c->cache.W()) {
            rc = gram_sweep(c);              // carries the closing control step of the previous sweep
        } else {
            rc = do_update_A(c);             // carries lambda_max + ctrl_end of the previous sweep when fused
            if (rc == VBMF_OK) rc = do_update_B(c);
            rc = run.close_stream_sweep(rc);
        }
        ++it;
        const bool last = (it == niter);
        if (rc == VBMF_OK) {                 // (the Gram form is always fused: Hp <= 128)
            if (fused_ctrl(c) && !last) {
                c->tail_pending = true;      // rides in the next sweep's pass-1 launch (Gram form: its first chain launch)
            } else if (fused_ctrl(c)) {
                rc = launch_eig(c, 1, 0);
                if (rc == VBMF_OK) rc = launch_ctrl_end(c, flags | 32, eps, run.trace_dev);
                ++c->ends_enqueued;
            } else {
                // H > 128: beside the next sweep's Y'B pass (side stream)
                if (side_overlap(c)) rc = side_fork(c);
                if (rc == VBMF_OK) rc = launch_eig(c, 1, 1);
                if (rc == VBMF_OK) rc = launch_ctrl_end(c, flags, eps, run.trace_dev);
                if (rc == VBMF_OK && c->use_side) rc = side_end(c);
            }
        }
        if (rc == VBMF_OK && !last && it % check == 0) stopped = run.look(it, check);
    }
    c->tail_pending = false;
    c->run_trace = nullptr;
    // in the Gram form only the streaming sweep (the first, if any) moves B, and every sweep moves W
    return run.finish(rc, run.bstart, run.stream_sweeps);
}

int vbmf_get_YHat(vbmf_ctx* c, double* YHat, int64_t ld) {
    if (!c) return VBMF_ERR_INVALID;
    if (!c->cache.have_state()) FAIL(c, VBMF_ERR_INVALID, "no state");
    if (!YHat || ld < c->L) FAIL(c, VBMF_ERR_INVALID, "vbmf_get_YHat: bad arguments");
    HIPCHK(c, hipSetDevice(c->o.device));
    TRY(ensure_B(c));
    int64_t mc = std::max<int64_t>(1, (int64_t)(256ll << 20) / (c->L * 8));
    mc = std::min(mc, c->M);
    DevScratch<double> tmp;
    MEMCHK(c, tmp.alloc((size_t)c->L * mc * 8));
    for (int64_t m0 = 0; m0 < c->M; m0 += mc) {
        const int64_t m1 = std::min(c->M, m0 + mc);
        hipLaunchKernelGGL(yhat_kernel, dim3(grid_for(c->L * (m1 - m0))), dim3(256), 0, c->stream, c->B32[c->bcur],
                           c->A32 + (size_t)m0 * c->Hp, c->Hp, (int)c->H, (long long)c->L, (long long)(m1 - m0), tmp.get(),
                           (long long)c->L);
        hipError_t e = hipMemcpy2DAsync(YHat + m0 * ld, (size_t)ld * 8, tmp, (size_t)c->L * 8, (size_t)c->L * 8,
                                        (size_t)(m1 - m0), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) FAIL(c, VBMF_ERR_HIP, "vbmf_get_YHat failed: %s", hipGetErrorString(e));
    }
    return VBMF_OK;
}

}  // extern "C"

// ---- results into the caller's own dtype, layout and memory, in row blocks (out_kernels.hpp) ----------------
static size_t dst_elem_size(int dt) { return dt == VBMF_DST_F64 ? 8 : dt == VBMF_DST_F32 ? 4 : 2; }

// Every refusal of the two output entries, in the order of include/vbmf_hip.h: nothing is launched, copied or materialised before
// this has returned VBMF_OK, so a wrong pointer comes back as a code and no kernel writes it.
static int check_dst(vbmf_ctx* c, const char* fn, const void* dst, int32_t dt, int32_t on_device, int64_t row0, int64_t nrows,
                     int64_t rows_total, int64_t ncols, int64_t rs, int64_t cs) {
    if (!dst) FAIL(c, VBMF_ERR_INVALID, "%s: null dst", fn);
    if (dt != VBMF_DST_F64 && dt != VBMF_DST_F32 && dt != VBMF_DST_BF16) FAIL(c, VBMF_ERR_INVALID, "%s: unknown dst_dtype %d", fn, (int)dt);
    if (rs <= 0 || cs <= 0) FAIL(c, VBMF_ERR_INVALID, "%s: strides must be positive", fn);
    if (row0 < 0 || nrows < 1 || nrows > rows_total - row0)
        FAIL(c, VBMF_ERR_INVALID, "%s: rows [%lld, %lld) are not inside 0 .. %lld", fn, (long long)row0, (long long)(row0 + nrows), (long long)rows_total);
    typedef unsigned __int128 u128;
    const u128 row_span = (u128)(ncols - 1) * (u128)cs + 1, col_span = (u128)(nrows - 1) * (u128)rs + 1;
    if ((u128)rs < row_span && (u128)cs < col_span)
        FAIL(c, VBMF_ERR_INVALID, "%s: the lines of dst overlap (neither stride is as long as a line of the other)", fn);
    if (!on_device && rs != 1 && cs != 1) FAIL(c, VBMF_ERR_INVALID, "%s: a host dst needs row_stride = 1 or col_stride = 1", fn);
    HIPCHK(c, hipSetDevice(c->o.device));
    hipPointerAttribute_t at;
    hipError_t e = hipPointerGetAttributes(&at, dst);
    if (e != hipSuccess) (void)hipGetLastError();                      // memory the runtime has never seen: plain host memory
    const bool is_dev = e == hipSuccess && (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged);
    if (on_device) {
        if (!is_dev) FAIL(c, VBMF_ERR_INVALID, "%s: dst_on_device is set but dst is not device memory", fn);
        if (at.device != c->o.device) FAIL(c, VBMF_ERR_INVALID, "%s: dst lives on device %d, the context on device %d", fn, at.device, c->o.device);
        const u128 last = (u128)(nrows - 1) * (u128)rs + (u128)(ncols - 1) * (u128)cs;
        hipDeviceptr_t base = nullptr;
        size_t size = 0;
        e = hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)dst);
        if (e != hipSuccess) { (void)hipGetLastError(); FAIL(c, VBMF_ERR_INVALID, "%s: dst belongs to no device allocation", fn); }
        const uintptr_t b = (uintptr_t)base, p = (uintptr_t)dst;
        if (p < b || p - b > size || (last + 1) * dst_elem_size(dt) > (u128)(size - (p - b)))
            FAIL(c, VBMF_ERR_INVALID, "%s: the strided extent of the block leaves its device allocation", fn);
    } else if (e == hipSuccess && at.type == hipMemoryTypeDevice) {
        FAIL(c, VBMF_ERR_INVALID, "%s: dst is device memory but dst_on_device is 0", fn);
    }
    return VBMF_OK;
}

// rows [l0, l0 + n) of YHat (or of Y - YHat) to DEVICE memory dev[(l - l0) rs + m cs]
template <class ACC, class DST>
static int launch_yhat_typed(vbmf_ctx* c, int what, DST* dev, int64_t l0, int64_t n, int64_t rs, int64_t cs) {
    // the factor of the dst's shorter-stride dimension is the MFMA's column side: its lanes then store side by side
    const bool swap = rs < cs;
    const float* Bf = c->B32[c->bcur];
    const float *Xf = swap ? c->A32 : Bf, *Yf = swap ? Bf : c->A32;
    const int64_t X = swap ? c->M : n, Yn = swap ? n : c->M;
    const int64_t xr0 = swap ? 0 : l0, yr0 = swap ? l0 : 0;
    const int64_t sx = swap ? cs : rs, sy = swap ? rs : cs;
    const int64_t ntx = (X + OUT_TILE - 1) / OUT_TILE, nty = (Yn + OUT_TILE - 1) / OUT_TILE;
    if (ntx * nty > 0x7fffffffll) FAIL(c, VBMF_ERR_UNSUPPORTED, "vbmf_get_YHat_rows: more than 2^31 output tiles in one block of rows: pass fewer rows per call");
    const size_t lds = out_lds_bytes<ACC>();
#define VBMF_OUT_LAUNCH(RESIDc, YMc)                                                                                               \
    hipLaunchKernelGGL((yhat_out_kernel<ACC, DST, RESIDc, YMc>), dim3((unsigned)(ntx * nty)), dim3(OUT_THREADS), lds, c->stream, Xf, Yf, \
                       c->Hp, (int)c->H, (long long)X, (long long)Yn, (long long)xr0, (long long)yr0, dev, (long long)sx,        \
                       (long long)sy, (int)nty, (int)swap, (const uint4*)c->Y2, c->d2.KS)
    if (what == VBMF_OUT_RESIDUAL) {
        if (c->mode == MODE_F32) VBMF_OUT_LAUNCH(true, MODE_F32); else VBMF_OUT_LAUNCH(true, MODE_BF16);
    } else {
        VBMF_OUT_LAUNCH(false, MODE_F32);
    }
#undef VBMF_OUT_LAUNCH
    HIPCHK(c, hipGetLastError());
    return VBMF_OK;
}
static int launch_yhat_out(vbmf_ctx* c, int what, void* dev, int dt, int64_t l0, int64_t n, int64_t rs, int64_t cs) {
    if (dt == VBMF_DST_F64) return launch_yhat_typed<double, double>(c, what, (double*)dev, l0, n, rs, cs);
    if (dt == VBMF_DST_F32) return launch_yhat_typed<float, float>(c, what, (float*)dev, l0, n, rs, cs);
    return launch_yhat_typed<float, out_bf16>(c, what, (out_bf16*)dev, l0, n, rs, cs);
}
static int launch_factor_out(vbmf_ctx* c, const float* F, void* dev, int dt, int64_t x0, int64_t n, int64_t rs, int64_t cs) {
    const int grid = grid_for(n * c->H), hfast = cs <= rs;
#define VBMF_FAC_LAUNCH(T)                                                                                                  \
    hipLaunchKernelGGL((factor_out_kernel<T>), dim3(grid), dim3(256), 0, c->stream, F, c->Hp, (int)c->H, (long long)x0, \
                       (long long)n, (T*)dev, (long long)rs, (long long)cs, hfast)
    if (dt == VBMF_DST_F64) VBMF_FAC_LAUNCH(double);
    else if (dt == VBMF_DST_F32) VBMF_FAC_LAUNCH(float);
    else VBMF_FAC_LAUNCH(out_bf16);
#undef VBMF_FAC_LAUNCH
    HIPCHK(c, hipGetLastError());
    return VBMF_OK;
}

// The block to dst: straight into device memory, or -- host memory -- through a device buffer of the dst's OWN dtype and order, whole
// rows per chunk of at most 256 MB (one row if that is larger).  emit(dev, first row, rows, row stride, column stride) enqueues the kernel.
template <class Emit>
static int write_block(vbmf_ctx* c, const char* fn, void* dst, int dt, int on_device, int64_t row0, int64_t nrows, int64_t ncols,
                       int64_t rs, int64_t cs, Emit emit) {
    const size_t es = dst_elem_size(dt);
    if (!c->ev_y[0]) { HIPCHK(c, hipEventCreate(&c->ev_y[0])); HIPCHK(c, hipEventCreate(&c->ev_y[1])); }
    HIPCHK(c, hipEventRecord(c->ev_y[0], c->stream));
    if (on_device) {
        TRY(emit(dst, row0, nrows, rs, cs));
    } else {
        const bool rowmajor = cs == 1 && (nrows == 1 || rs >= ncols);
        int64_t rc = std::max<int64_t>(1, (int64_t)(256ll << 20) / (ncols * (int64_t)es));
        rc = std::min(rc, nrows);
        DevScratch<void> stage;
        MEMCHK(c, stage.alloc((size_t)rc * ncols * es));
        for (int64_t r = 0; r < nrows; r += rc) {
            const int64_t n = std::min(rc, nrows - r);
            TRY(rowmajor ? emit(stage.get(), row0 + r, n, ncols, (int64_t)1) : emit(stage.get(), row0 + r, n, (int64_t)1, n));
            char* to = (char*)dst + (size_t)r * rs * es;
            hipError_t e = rowmajor ? hipMemcpy2DAsync(to, (size_t)rs * es, stage, (size_t)ncols * es, (size_t)ncols * es, (size_t)n, hipMemcpyDeviceToHost, c->stream)
                                    : hipMemcpy2DAsync(to, (size_t)cs * es, stage, (size_t)n * es, (size_t)n * es, (size_t)ncols, hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) FAIL(c, VBMF_ERR_HIP, "%s: copy to the host failed: %s", fn, hipGetErrorString(e));
        }
    }
    HIPCHK(c, hipEventRecord(c->ev_y[1], c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));            // the caller may read its buffer once this returns
    float ms = 0.0f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev_y[0], c->ev_y[1]));
    c->out_ms = ms;
    return VBMF_OK;
}

// vbmf_debug_blk_sweep: the test kernel of blk_inverse.hpp at tier NB, one workgroup, default stream
template <int NB>
static hipError_t debug_blk_sweep_launch(int waves, const double* dK, int H, double* dOut, double* dLd, int* dBad) {
    const void* fn = waves == 1 ? (const void*)debug_blk_sweep_kernel<NB, 1> : (const void*)debug_blk_sweep_kernel<NB, 4>;
    const size_t lds = spd_inverse_lds_bytes(NB);
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    if (waves == 1) hipLaunchKernelGGL((debug_blk_sweep_kernel<NB, 1>), dim3(1), dim3(256), lds, 0, dK, H, dOut, dLd, dBad);
    else hipLaunchKernelGGL((debug_blk_sweep_kernel<NB, 4>), dim3(1), dim3(256), lds, 0, dK, H, dOut, dLd, dBad);
    return hipGetLastError();
}

extern "C" {

int vbmf_get_YHat_rows(vbmf_ctx* c, int32_t what, void* dst, int32_t dt, int32_t on_device, int64_t row0, int64_t nrows,
                       int64_t rs, int64_t cs) {
    if (!c) return VBMF_ERR_INVALID;
    static const char* fn = "vbmf_get_YHat_rows";
    if (!dst) FAIL(c, VBMF_ERR_INVALID, "%s: null dst", fn);
    if (what != VBMF_OUT_YHAT && what != VBMF_OUT_RESIDUAL) FAIL(c, VBMF_ERR_INVALID, "%s: unknown what %d", fn, (int)what);
    TRY(check_dst(c, fn, dst, dt, on_device, row0, nrows, c->L, c->M, rs, cs));
    if (!c->cache.have_state()) FAIL(c, VBMF_ERR_INVALID, "%s: no state", fn);
    if (what == VBMF_OUT_RESIDUAL && !c->cache.have_Y()) FAIL(c, VBMF_ERR_INVALID, "%s: no Y", fn);
    TRY(ensure_B(c));
    TRY(rebuild_B32_if_stale(c));
    return write_block(c, fn, dst, dt, on_device, row0, nrows, c->M, rs, cs,
                       [&](void* dev, int64_t l0, int64_t n, int64_t r, int64_t s) { return launch_yhat_out(c, what, dev, dt, l0, n, r, s); });
}

int vbmf_get_factor_rows(vbmf_ctx* c, int32_t which, void* dst, int32_t dt, int32_t on_device, int64_t row0, int64_t nrows,
                         int64_t rs, int64_t cs) {
    if (!c) return VBMF_ERR_INVALID;
    static const char* fn = "vbmf_get_factor_rows";
    if (!dst) FAIL(c, VBMF_ERR_INVALID, "%s: null dst", fn);
    if (which != VBMF_FACTOR_A && which != VBMF_FACTOR_B) FAIL(c, VBMF_ERR_INVALID, "%s: unknown which %d", fn, (int)which);
    TRY(check_dst(c, fn, dst, dt, on_device, row0, nrows, which == VBMF_FACTOR_A ? c->M : c->L, c->H, rs, cs));
    if (!c->cache.have_state()) FAIL(c, VBMF_ERR_INVALID, "%s: no state", fn);
    if (which == VBMF_FACTOR_B) {
        TRY(ensure_B(c));
        TRY(rebuild_B32_if_stale(c));
    }
    return write_block(c, fn, dst, dt, on_device, row0, nrows, c->H, rs, cs, [&](void* dev, int64_t x0, int64_t n, int64_t r, int64_t s) {
        return launch_factor_out(c, which == VBMF_FACTOR_A ? c->A32 : c->B32[c->bcur], dev, dt, x0, n, r, s);
    });
}

int vbmf_elbo(vbmf_ctx* c, double* elbo) {
    if (!c || !elbo) return VBMF_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->o.device));
    TRY(ensure_ready(c));
    TRY(ensure_gram_A(c));
    TRY(ensure_gram_B(c));
    int f = 0;
    TRY(prepare_trYBA(c, &f));
    TRY(launch_ctrl_end(c, f, 0.0, nullptr));
    HIPCHK(c, hipMemcpyAsync(c->scal_host, c->st + c->lay.scal(), 32 * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *elbo = c->scal_host[S_ELBO];
    return VBMF_OK;
}

// ---- multi-GPU ---------------------------------------------------------------------------------
int vbmf_comm_unique_id(void* id128) {
    if (!id128) return VBMF_ERR_INVALID;
    static_assert(sizeof(ncclUniqueId) <= VBMF_UNIQUE_ID_BYTES, "unique id size");
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return VBMF_ERR_COMM;
    memset(id128, 0, VBMF_UNIQUE_ID_BYTES);
    memcpy(id128, &id, sizeof id);
    return VBMF_OK;
}

int vbmf_comm_init(vbmf_ctx* c, const void* id128) {
    if (!c || !id128) return VBMF_ERR_INVALID;
    if (c->comm_ready) FAIL(c, VBMF_ERR_INVALID, "communicator already initialised");
    HIPCHK(c, hipSetDevice(c->o.device));
    TRY(ensure_B(c));
    ncclUniqueId id;
    memcpy(&id, id128, sizeof id);
    NCCLCHK(c, ncclCommInitRank(&c->comm, c->o.nranks, id, c->o.rank));
    c->comm_ready = true;
    c->cache.communicator_attached();  // ||Y||^2 (if already set) and the Grams must be summed over the ranks
    return VBMF_OK;
}

int vbmf_comm_set_transport(vbmf_ctx* c, vbmf_allreduce_fn fn, void* user) {
    if (!c || !fn) return VBMF_ERR_INVALID;
    if (c->comm_ready) FAIL(c, VBMF_ERR_INVALID, "communicator already initialised");
    HIPCHK(c, hipSetDevice(c->o.device));
    TRY(ensure_B(c));                 // (a row-sharded context leaves the Gram form)
    c->ar_hook = fn;
    c->ar_user = user;
    c->comm_ready = true;
    c->cache.communicator_attached();
    return VBMF_OK;
}

// ---- measurement -------------------------------------------------------------------------------
int vbmf_profile_enable(vbmf_ctx* c, int on) {
    if (!c) return VBMF_ERR_INVALID;
    hipSetDevice(c->o.device);
    prof_harvest(c);
    c->prof = on > 0 ? on : 0;
    c->prof_seen[0] = c->prof_seen[1] = 0;
    return VBMF_OK;
}

int vbmf_profile_read(vbmf_ctx* c, double* out8, int reset) {
    if (!c || !out8) return VBMF_ERR_INVALID;
    hipSetDevice(c->o.device);
    prof_harvest(c);
    memset(out8, 0, 8 * sizeof(double));
    out8[0] = c->prof_ms[0]; out8[1] = c->prof_n[0]; out8[2] = c->prof_ms[1]; out8[3] = c->prof_n[1];
    if (reset) { c->prof_ms[0] = c->prof_ms[1] = 0; c->prof_n[0] = c->prof_n[1] = 0; }
    return VBMF_OK;
}

int vbmf_pass_bytes(vbmf_ctx* c, int pass, double* bytes) {
    if (!c || !bytes || (pass != 1 && pass != 2)) return VBMF_ERR_INVALID;
    // algorithmic traffic of one launch: Y once in its device dtype, the factor in
    // (fp32 equivalent), the H-wide result out (fp32)
    const double ybytes = (c->mode == MODE_F32) ? 4.0 : 2.0;
    const double LM = (double)c->L * (double)c->M;
    if (pass == 1 && gram_eligible(c)) {
        // Gram form: profile slot 1 times the product [G W | G D] -- G once (fp32), the five bf16 operand planes, the fp32 slabs out
        const double n = (double)c->Hp * c->d1.XT * 32.0;
        const int nsplit = c->Gt ? c->g_nsplit : 1;
        // (rank 256: G once per h-tile group)
        *bytes = (double)c->M * c->M * 4.0 * (c->NH / gram_prod_nh(c)) + 5.0 * c->M * c->H * 2.0 + 2.0 * n * 4.0 * nsplit;
        return VBMF_OK;
    }
    if (pass == 1) *bytes = LM * ybytes + (double)c->L * c->H * 4.0 + (double)c->M * c->H * 4.0;
    else {
        // with the register epilogue (un-split pass, H <= 64) the launch writes B and re-reads B_old instead of writing
        // the product: SURVEY 8d's "B written and B_old re-read in pass 2"
        const bool epi = c->NH <= 2 && !c->narrow && c->d2.nsplit == 1 && (c->d2.XT / nxw_of(c->NH) + 3) / 4 <= c->gslab_cap;
        *bytes = LM * ybytes + (double)c->M * c->H * 4.0 + (double)c->L * c->H * 4.0 * (epi ? 2.0 : 1.0);
    }
    return VBMF_OK;
}

int vbmf_debug_peek(vbmf_ctx* c, int what, uint32_t* out, int64_t nwords, int64_t word_offset) {
    if (!c || !out || nwords < 0 || word_offset < 0) return VBMF_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->o.device));
    if (what != VBMF_PEEK_DIMS) TRY(ensure_B(c));          // every buffer is shown as an eager run end left it; the dimensions never pay
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (what == VBMF_PEEK_DIMS) {
        const int v[31] = {c->Hp, c->NH, c->mode, c->d1.XT, c->d1.KS, c->d1.nsplit, c->d1.steps_per_split,
                           c->d2.XT, c->d2.KS, c->d2.nsplit, c->d2.steps_per_split, c->kstep, c->npart, c->narrow ? 1 : 0, c->sk_per, c->sk_grid,
                           gram_eligible(c) ? 1 : 0, c->cache.G() ? 1 : 0, (int)std::lround(c->gram_build_ms * 1000.0), c->g_nsplit,
                           c->frag_last[0] ? 1 : 0, c->frag_last[1] ? 1 : 0, c->epi_last ? 1 : 0, use_lds8(c) ? 1 : 0, c->xcd_map ? 1 : 0,
                           c->post3 ? 1 : 0, c->sparse_a_fused ? 1 : 0, (int)std::lround(c->set_y_ms * 1000.0),
                           c->cache.B_owed() ? 1 : 0, (int)std::min<long long>(c->b_materialised, 0x7fffffff),
                           (int)std::lround(c->out_ms * 1000.0)};
        memcpy(out, v, sizeof(int) * (size_t)std::min<int64_t>(31, nwords));
        return VBMF_OK;
    }
    if (what == VBMF_PEEK_CHAIN) {
        if (nwords > 16) FAIL(c, VBMF_ERR_INVALID, "vbmf_debug_peek: the chain stamps are 16 words");
        HIPCHK(c, memcpy_sync(c, out, c->ints + 8, (size_t)nwords * 4, hipMemcpyDeviceToHost));
        return VBMF_OK;
    }
    const void* base = nullptr;
    size_t words = 0;
    switch (what) {
        case VBMF_PEEK_P: base = c->P; words = (size_t)c->d1.nsplit * c->Hp * c->Mp; break;
        case VBMF_PEEK_Q: base = c->Q; words = (size_t)c->d2.nsplit * c->Hp * c->Lp; break;
        case VBMF_PEEK_A32: base = c->A32; words = (size_t)c->Mp * c->Hp; break;
        case VBMF_PEEK_B32: base = c->B32[c->bcur]; words = (size_t)c->Lp * c->Hp; break;
        case VBMF_PEEK_FA: base = c->FA; words = c->nFA * 4; break;
        case VBMF_PEEK_FB: base = c->FB; words = c->nFB * 4; break;
        case VBMF_PEEK_Y1: base = c->Y1; words = c->nY1 * 4; break;
        case VBMF_PEEK_Y2: base = c->Y2; words = c->nY2 * 4; break;
        case VBMF_PEEK_STATE: base = c->st; words = (size_t)c->lay.total() * 2; break;
        case VBMF_PEEK_GRAM_W: base = c->W32g[c->wcur]; words = c->W32g[c->wcur] ? (size_t)32 * c->GT * c->Hp : 0; break;
        case VBMF_PEEK_GRAM_PQ: base = c->gPQ; words = c->gPQ ? (size_t)2 * c->Hp * c->d1.XT * 32 : 0; break;
        case VBMF_PEEK_GRAM_G: base = c->Gt; words = c->Gt ? (size_t)c->GT * 2 * c->GT * 64 * 8 : 0; break;
        case VBMF_PEEK_SA32: base = c->SA32; words = (size_t)c->Hp * c->Hp; break;
        case VBMF_PEEK_SB32: base = c->SB32; words = (size_t)c->Hp * c->Hp; break;
        default: FAIL(c, VBMF_ERR_INVALID, "vbmf_debug_peek: unknown buffer");
    }
    if ((size_t)(word_offset + nwords) > words) FAIL(c, VBMF_ERR_INVALID, "vbmf_debug_peek: range exceeds buffer (%zu words)", words);
    HIPCHK(c, memcpy_sync(c, out, (const uint32_t*)base + word_offset, (size_t)nwords * 4, hipMemcpyDeviceToHost));
    return VBMF_OK;
}

int vbmf_debug_time_pass(vbmf_ctx* c, int pass, int iters, double* ms) {
    if (!c || !ms || (pass != 1 && pass != 2) || iters < 1) return VBMF_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->o.device));
    TRY(ensure_ready(c));
    hipEvent_t a, b;
    HIPCHK(c, hipEventCreate(&a));
    HIPCHK(c, hipEventCreate(&b));
    const int prof = c->prof;
    c->prof = 0;
    int rc = launch_stream(c, pass - 1);
    if (rc == VBMF_OK) rc = launch_stream(c, pass - 1);
    hipEventRecord(a, c->stream);
    for (int i = 0; i < iters && rc == VBMF_OK; ++i) rc = launch_stream(c, pass - 1);
    hipEventRecord(b, c->stream);
    hipEventSynchronize(b);
    float t = 0.f;
    hipEventElapsedTime(&t, a, b);
    hipEventDestroy(a);
    hipEventDestroy(b);
    c->prof = prof;
    c->cache.P_overwritten();
    *ms = t / iters;
    return rc;
}

int vbmf_debug_lambda_max(vbmf_ctx* c, const double* G, double* lam, double* kernel_us) {
    if (!c || !G || !lam) return VBMF_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->o.device));
    TRY(ensure_B(c));
    const int H = (int)c->H, Hp = c->Hp;
    std::vector<double> g((size_t)Hp * Hp, 0.0);
    for (int j = 0; j < H; ++j)
        for (int i = 0; i < H; ++i) g[(size_t)i * Hp + j] = G[(size_t)j * H + i];
    HIPCHK(c, hipMemcpyAsync(c->st + c->lay.GD(), g.data(), g.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->ints + I_STOP, 0, sizeof(int), c->stream));      // (the kernels are stop-gated)
    hipEvent_t a, b;
    HIPCHK(c, hipEventCreate(&a));
    HIPCHK(c, hipEventCreate(&b));
    hipEventRecord(a, c->stream);
    int rc = launch_eig(c, 1, 0);
    hipEventRecord(b, c->stream);
    hipEventSynchronize(b);
    float t = 0.f;
    hipEventElapsedTime(&t, a, b);
    hipEventDestroy(a);
    hipEventDestroy(b);
    if (rc != VBMF_OK) return rc;
    HIPCHK(c, hipMemcpyAsync(lam, c->st + c->lay.scal() + S_LAMD, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (kernel_us) *kernel_us = 1e3 * (double)t;
    return VBMF_OK;
}

int vbmf_debug_blk_sweep(const double* K, int64_t H, int waves, double* out, double* logdet, int* bad) {
    if (!K || !out || !logdet || !bad || H < 1 || H > 128 || (waves != 1 && waves != 4)) return VBMF_ERR_INVALID;
    const int h = (int)H, n = 16 * ((h + 15) >> 4);
    const size_t kb = (size_t)h * h * sizeof(double), ob = (size_t)n * n * sizeof(double);
    double* d = nullptr;                                          // [K | out | logdet | bad]
    if (hipMalloc(&d, kb + ob + 2 * sizeof(double)) != hipSuccess) return VBMF_ERR_HIP;
    double* dOut = d + (size_t)h * h;
    double* dLd = dOut + (size_t)n * n;
    int* dBad = reinterpret_cast<int*>(dLd + 1);
    hipError_t e = hipMemcpy(d, K, kb, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = h <= 16 ? debug_blk_sweep_launch<1>(waves, d, h, dOut, dLd, dBad)
          : h <= 32 ? debug_blk_sweep_launch<2>(waves, d, h, dOut, dLd, dBad)
          : h <= 64 ? debug_blk_sweep_launch<4>(waves, d, h, dOut, dLd, dBad)
                    : debug_blk_sweep_launch<8>(waves, d, h, dOut, dLd, dBad);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dOut, ob, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(logdet, dLd, sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(bad, dBad, sizeof(int), hipMemcpyDeviceToHost);
    hipFree(d);
    return e == hipSuccess ? VBMF_OK : VBMF_ERR_HIP;
}

int vbmf_debug_set(vbmf_ctx* c, int what, int64_t value) {
    if (!c) return VBMF_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->o.device));
    TRY(ensure_B(c));                 // a B that is owed is made as the run left things, before a knob moves
    switch (what) {
        case VBMF_DEBUG_EXACT_LAMBDA:
            c->exact_lambda = value != 0;
            return VBMF_OK;
        case VBMF_DEBUG_EPI_SPIN_LIMIT:
            if (value < 1 || value > (1ll << 30)) FAIL(c, VBMF_ERR_INVALID, "vbmf_debug_set: spin limit out of range");
            c->epi_spin_limit = (int)value;
            return VBMF_OK;
        case VBMF_DEBUG_EPI_EXPECT_SKEW:
            c->epi_expect_skew = value ? 1 : 0;
            return VBMF_OK;
        case VBMF_DEBUG_SIGMA_B_PPM: {
            if (value < -1000000 || value > 1000000) FAIL(c, VBMF_ERR_INVALID, "vbmf_debug_set: ppm out of range");
            c->dbg_sb_ppm = (int)value;
            HIPCHK(c, hipSetDevice(c->o.device));
            HIPCHK(c, memcpy_sync(c, c->ints + I_DBG_SB_PPM, &c->dbg_sb_ppm, sizeof(int), hipMemcpyHostToDevice));
            return VBMF_OK;
        }
        default: FAIL(c, VBMF_ERR_INVALID, "vbmf_debug_set: unknown knob");
    }
}

int vbmf_device_sync(vbmf_ctx* c) {
    if (!c) return VBMF_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->o.device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VBMF_OK;
}


// ================================================================================================
// ARD-sparse variant (src/vbmf_sparse.jl, full_cov=false, diag_var=false)
// ================================================================================================
}  // extern "C"

static double digamma_host(double x) {
    double r = 0.0;
    while (x < 10.0) { r -= 1.0 / x; x += 1.0; }
    const double f = 1.0 / (x * x);
    return r + std::log(x) - 0.5 / x -
           f * (1.0 / 12 - f * (1.0 / 120 - f * (1.0 / 252 - f * (1.0 / 240 - f * (5.0 / 660 - f * (691.0 / 32760))))));
}

static int launch_sparse_cov_b(vbmf_ctx* c) {
    ctrl_tier(c->H, [&](auto r, auto t) {
        constexpr int R = decltype(r)::value, T = decltype(t)::value;
        hipLaunchKernelGGL((sparse_cov_b_kernel<R, T>), dim3(1), dim3(T * T), (cov_lds_bytes<R, T>()), ctrl_stream(c), c->st, c->lay, (int)c->H,
                           c->SB32, c->ints, c->diagvar ? 1 : 0);
    });
    HIPCHK(c, hipGetLastError());
    return VBMF_OK;
}

static int sparse_colsum(vbmf_ctx* c) {
    double* part = c->st + c->lay.W1();      // scratch: COLSUM_CHUNKS * Hp <= Hp * Hp doubles (Hp >= 32)
    const int* stop = c->ints + I_STOP;
    hipLaunchKernelGGL(colsum_part_kernel, dim3(c->Hp / 32, COLSUM_CHUNKS), dim3(256), 0, c->stream, c->dS32, (long long)c->M, (int)c->H, c->Hp, part,
                       (const float*)nullptr, stop);
    hipLaunchKernelGGL(colsum_fold_kernel, dim3(c->Hp / 32), dim3(256), 0, c->stream, part, (int)c->H, c->Hp, c->st, c->lay, (double*)nullptr, stop);
    HIPCHK(c, hipGetLastError());
    return VBMF_OK;
}

template <int R, int T, int NB = 2>
static void launch_full_a_t(vbmf_ctx* c, const double* Gw = nullptr) {
    hipLaunchKernelGGL((sparse_update_a_full_kernel<R, T, NB>), dim3(c->fblocks), dim3(T * T), (size_t)(6 * NB * T * R) * sizeof(double), c->stream,
                       c->Pred, (long long)c->d1.XT * 32, c->CA32, c->st, c->lay, c->A32, c->dS32, c->has_mask ? c->mask : nullptr,
                       (int)(c->H - c->H1), (long long)c->M, (int)c->H, c->Hp, (double)c->Lg, c->fpart, c->ints, Gw);
}

// H <= 64: one column of Y per wavefront (sparse_kernels.hpp, sparse_update_a_full_wave_kernel); returns the number of partial
// sums of Sigma_m it leaves in c->fpart (one per workgroup)
template <int NBK, int NW>
static int launch_full_a_wave(vbmf_ctx* c, const double* Gw) {
    constexpr size_t lds = full_a_wave_lds_bytes(NBK, NW);      // (the attribute that admits it: vbmf_create)
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(c->fblocks, cdiv(c->M, NW)), 2 * (NUM_CU + 2)));
    hipLaunchKernelGGL((sparse_update_a_full_wave_kernel<NBK, NW>), dim3(grid), dim3(NW * 64), lds, c->stream,
                       c->Pred, (long long)c->d1.XT * 32, c->CA32, c->st, c->lay, c->A32, c->dS32, c->has_mask ? c->mask : nullptr,
                       (int)(c->H - c->H1), (long long)c->M, (int)c->H, c->Hp, (double)c->Lg, c->fpart, c->ints, Gw);
    return grid;
}

// B' diag(sigmaVecHat) B summed over the row shards (full_cov with diag_var, src/vbmf_sparse.jl:180-182): the plain Gram (exact-f32
// kernel, any H) of sqrt(sigma_l) * B[l,:], formed in the fp32 buffer of the PREVIOUS B (free between the B update's delta-Gram
// and the next B update).  Local sum in c->gw, reduced OUT OF PLACE into c->gw + Hp^2 (idempotent after the device-side stop,
// like the two per-sweep reductions); *out: where the result is.
static int weighted_gram_B(vbmf_ctx* c, const double** out) {
    const int* stop = c->ints + I_STOP;
    float* scratch = c->B32[c->bcur ^ 1];
    const long long nel = (long long)c->Lp * c->Hp;
    hipLaunchKernelGGL(sqrt_rowscale_kernel, dim3(grid_for(nel, 256, 4096)), dim3(256), 0, c->stream, c->B32[c->bcur], c->sig32, scratch,
                       nel, c->Hp, stop);
    // the dense-slab kernel with the context-wide chunk size (NOT gram_tiles_per_chunk(): that is the tile kernels' choice and
    // gives fewer, larger chunks on some shapes); vbmf_create sizes gslab for this chunking too, and the guard below says so
    const int tpc = c->tiles_per_chunk;
    const int nchunk = cdiv(c->d2.XT, tpc);
    const int nw = nchunk * c->NH * c->NH;
    GSLAB_CHECK(c, nchunk, 2 * c->Hp * c->Hp);
    if (!dispatch<1, 2, 4, 8>(c->NH, [&](auto nh) {
            hipLaunchKernelGGL((gram_kernel<decltype(nh)::value>), dim3((nw + 3) / 4), dim3(256), 0, c->stream, scratch, (const float*)nullptr,
                               c->gslab, c->d2.XT, tpc, nchunk, stop);
        })) NO_KERNEL(c);
    // (its own reduction, not gram_reduce_tail: the sum goes to c->gw, not the state, and is all-reduced out of place)
    const int n = c->Hp * c->Hp;
    hipLaunchKernelGGL(gram_reduce_kernel, dim3((2 * n + 31) / 32), dim3(256), 0, c->stream, c->gslab, nchunk, n, c->gw, (double*)nullptr,
                       stop, (const double*)nullptr, 0, (double*)nullptr);
    HIPCHK(c, hipGetLastError());
    *out = c->gw;
    if (sharded(c)) {
        TRY(allreduce_sum(c, c->gw, c->gw + n, (size_t)n, true));
        *out = c->gw + n;
    }
    return VBMF_OK;
}

static int do_sparse_update_A(vbmf_ctx* c, bool reuse_P = false) {
    TRY(ensure_gram_B(c));
    const int* stop = c->ints + I_STOP;
    if (c->diagvar) {
        // :211, :230 -- B enters as diag(sigmaVecHat) * B: tiles of the row-scaled factor for the pass, and
        // sum_l (sigma_l B[l,h])^2 for the precision of vec(A')
        if (!c->cache.have_noise()) FAIL(c, VBMF_ERR_INVALID, "no row noise state: call vbmf_sparse_set_noise_rows first");
        TRY(launch_retile_ex(c, 1, c->B32[c->bcur], c->FBs, c->sig32, 0, true));
        double* part = c->st + c->lay.W1();
        hipLaunchKernelGGL(colsum_part_kernel, dim3(c->Hp / 32, COLSUM_CHUNKS), dim3(256), 0, c->stream, c->B32[c->bcur], (long long)c->L,
                           (int)c->H, c->Hp, part, (const float*)c->sig32, stop);
        hipLaunchKernelGGL(colsum_fold_kernel, dim3(c->Hp / 32), dim3(256), 0, c->stream, part, (int)c->H, c->Hp, c->st, c->lay, c->vsq, stop);
        if (sharded(c)) TRY(allreduce_sum(c, c->vsq, (size_t)c->Hp, true));    // scratch, rebuilt before every use
        reuse_P = false;                            // sigma changes every iteration, so does Y' diag(sigma) B
    }
    if (!(reuse_P && c->cache.P())) {
        c->P_frag = false;                          // the element-wise A update reads the plain [h][m] product
        TRY(launch_stream(c, 0));
        const long long n = (long long)c->Hp * c->d1.XT * 32;
        hipLaunchKernelGGL(slab_sum_kernel, dim3(grid_for(n / 4, 256, 2048)), dim3(256), 0, c->stream, c->P, c->d1.nsplit, n,
                           sharded(c) ? c->P : c->Pred, n, stop, SideCopy{});
        if (sharded(c)) TRY(allreduce_sum(c, c->P, c->Pred, (size_t)n, false));      // Y'B summed over the row shards (out of place)
    }
    TRY(side_join(c));                              // the previous sweep's lambda_max / CB / sigma / stop test (side stream)
    if (c->full_cov) {
        // :178-202 -- M independent H x H inverses (the dense MH x MH matrix of the reference is block diagonal)
        const int H = (int)c->H;
        const double* Gw = nullptr;
        if (c->diagvar) TRY(weighted_gram_B(c, &Gw));
        int nparts = c->fblocks;
        ctrl_tier(H, [&](auto r, auto t) {
            constexpr int R = decltype(r)::value;
            if constexpr (decltype(t)::value == 32)            // 128 < H <= 256: blocked Schur inverse through a global workspace
                hipLaunchKernelGGL(sparse_update_a_full256_kernel, dim3(c->fblocks), dim3(1024), (size_t)(INV256_LDS_DOUBLES + 256 + 256) * sizeof(double),
                                   c->stream, c->Pred, (long long)c->d1.XT * 32, c->CA32, c->st, c->lay, c->A32, c->dS32,
                                   c->has_mask ? c->mask : nullptr, (int)(c->H - c->H1), (long long)c->M, H, (double)c->Lg, c->fpart, c->ints, Gw, c->fws);
            else if constexpr (R == 8) launch_full_a_t<8, 16, 1>(c, Gw);   // 64 < H <= 128: one column per round and workgroup
            // H <= 64: one column per wavefront, blocked sweep in the wave's LDS image (eight wavefronts while their images fit)
            else nparts = launch_full_a_wave<R, (R == 4 ? 4 : 8)>(c, Gw);
        });
        hipLaunchKernelGGL(full_sa_fold_kernel, dim3(cdiv(c->Hp * c->Hp, 256)), dim3(256), 0, c->stream, c->fpart, nparts, c->Hp, c->st, c->lay, stop);
        HIPCHK(c, hipGetLastError());
        TRY(launch_retile(c, 0, true));
        TRY(launch_gram(c, 0, c->A32, nullptr, true));
        c->cache.A_moved_sparse(true);
        return VBMF_OK;
    }
    hipLaunchKernelGGL(sparse_v_kernel, dim3((c->Hp + 63) / 64), dim3(64), 0, c->stream, c->st, c->lay, (int)c->H, (double)c->Lg, c->vtab,
                       c->diagvar ? (const double*)c->vsq : (const double*)nullptr, stop);
    const int compat = (c->o.reference_compat & VBMF_COMPAT_SPARSE_REPEAT) ? 1 : 0;
    if (compat && c->M < 2) FAIL(c, VBMF_ERR_INVALID, "repeat(v, inner=M-1) needs M >= 2");
    if (c->sparse_a_fused) {
        // the update and the operand tiles of the next pass in one launch (A32 := the value the tiles encode, as retile leaves it)
        const bool ok = dispatch<MODE_F32, MODE_BF16, MODE_BF16X2>(c->mode, [&](auto md) {
            return dispatch<1, 2, 4, 8>(c->NH, [&](auto nh) {
                constexpr int NHc = decltype(nh)::value;
                hipLaunchKernelGGL((sparse_update_a_tiles_kernel<decltype(md)::value, NHc>), dim3((c->d1.XT * NHc + 3) / 4), dim3(256), 0, c->stream,
                                   c->Pred, (long long)c->d1.XT * 32, c->CA32, c->vtab, c->st, c->lay, c->A32, c->dS32, c->FA,
                                   c->has_mask ? c->mask : nullptr, (int)(c->H - c->H1), (long long)c->M, (int)c->H, compat,
                                   c->diagvar ? 1 : 0, c->d1.XT, stop);
            });
        });
        if (!ok) NO_KERNEL(c);
        HIPCHK(c, hipGetLastError());
    } else {
        hipLaunchKernelGGL(sparse_update_a_kernel, dim3(grid_for((int64_t)c->M * c->Hp)), dim3(256), 0, c->stream, c->Pred,
                           (long long)c->d1.XT * 32, c->CA32, c->vtab, c->st, c->lay, c->A32, c->dS32,
                           c->has_mask ? c->mask : nullptr, (int)(c->H - c->H1), (long long)c->M, (int)c->H, c->Hp, compat,
                           c->diagvar ? 1 : 0, stop);
        HIPCHK(c, hipGetLastError());
        TRY(launch_retile(c, 0, true));             // operand tiles; A32 := the value the tiles encode
    }
    TRY(launch_gram(c, 0, c->A32, nullptr, true));
    TRY(sparse_colsum(c));                          // SigmaA = diag(sum_m diagSigma)
    c->cache.A_moved_sparse(!c->diagvar);           // (diag_var: c->Pred is Y' diag(sigma) B)
    return VBMF_OK;
}

// keep_sigma: B from the sigmaHat SigmaB table already in place (the end of a Gram-form run materialises B with the last sweep's table)
static int do_sparse_update_B(vbmf_ctx* c, bool keep_sigma = false) {
    TRY(ensure_gram_A(c));
    if (!keep_sigma && side_overlap(c)) {           // SigmaB beside the pass: only the post kernel needs it
        TRY(side_fork(c));
        TRY(launch_sparse_cov_b(c));
        TRY(side_end(c));
    } else if (!keep_sigma) {
        TRY(launch_sparse_cov_b(c));
    }
    // fragment-major product: H <= 64 always (folded element-wise when split), H >= 128 when un-split; the row-noise update
    // reads the plain product
    const bool fragq = !c->diagvar && (fused_gram(c) || c->d2.nsplit == 1);
    TRY(launch_stream(c, 1, 0, false, nullptr, fragq));
    TRY(fold_Q_slabs(c));
    TRY(side_join(c));
    if (fused_gram(c) && !c->diagvar) {
        TRY(launch_post_gram(c, 1, c->Q));
    } else {
        if (fragq) TRY(launch_post_frag(c));
        else TRY(launch_post(c, 1, c->Q, 1));
        // :261 -- B = diag(sigmaVecHat) * Y A SigmaB: the post kernel applied SigmaB, the rows are scaled here
        if (c->diagvar) TRY(launch_retile_ex(c, 1, c->B32[c->bcur ^ 1], c->FB, c->sig32, 1, true));
        TRY(launch_gram(c, 1, c->B32[c->bcur ^ 1], c->B32[c->bcur], true, c->ntr));
    }
    c->bcur ^= 1;
    c->cache.B_moved_sparse(c->diagvar);
    return VBMF_OK;
}

// B after a Gram-form run, on demand.  The run's sweeps moved W, not B; what is owed is B of the last executed sweep, by the
// streaming pass 2 with that sweep's A and SigmaB / sigma2 (sparse model: sigmaHat SigmaB) table, which is still in place: B, its
// operand tiles and the fp32 copy as a streaming run leaves them.  The state's [B'B | dB'dB | tr(B'YA)] stay the Gram form's, so a
// run that continues from here computes what one longer run computes.  Every entry point that reads B, its tiles or anything
// derived from them comes through here first (ensure_ready does it for most); a Gram-form run that finds W valid, and vbmf_destroy,
// never pay.  What drops the debt: ctx_cache.hpp.
static int ensure_B(vbmf_ctx* c) {
    if (!c->cache.B_owed()) return VBMF_OK;
    c->cache.B_payment_begins();
    ++c->b_materialised;
    const size_t nsave = 2 * (size_t)c->Hp * c->Hp + 8;
    int rc = VBMF_OK;
    hipError_t e = hipMemcpyAsync(c->gsave, c->st + c->lay.GB(), nsave * 8, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) rc = c->sparse ? do_sparse_update_B(c, true) : do_update_B(c, true);
    else { c->err = std::string("B after a Gram-form run: ") + hipGetErrorString(e); rc = VBMF_ERR_HIP; }
    if (rc == VBMF_OK) {
        e = hipMemcpyAsync(c->st + c->lay.GB(), c->gsave, nsave * 8, hipMemcpyDeviceToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) { c->err = std::string("B after a Gram-form run: ") + hipGetErrorString(e); rc = VBMF_ERR_HIP; }
    }
    if (rc == VBMF_OK) rc = check_device_err(c);
    c->cache.B_payment_ends(c->sparse, rc == VBMF_OK);
    return rc;
}

// updateSigma!, diag_var = true (:308-315): every row's Gamma posterior; S_SIGMA2 := mean(sigmaVecHat)
static int do_hetero_sigma(vbmf_ctx* c) {
    TRY(ensure_gram_A(c));
    if (!c->cache.Q()) {                              // Y*A for the current A (not left over from updateB!)
        TRY(launch_stream(c, 1));
        TRY(fold_Q_slabs(c));
        c->cache.Q_made();
    }
    const int* stop = c->ints + I_STOP;
    hipLaunchKernelGGL(hetero_g_kernel, dim3(1), dim3(1024), 0, c->stream, c->st, c->lay, (int)c->H, c->G32, stop);
    const int nb = (int)cdiv(c->L, 256);
    hipLaunchKernelGGL(hetero_sigma_kernel, dim3(nb), dim3(256), 0, c->stream, c->Q, (long long)c->d2.XT * 32, c->B32[c->bcur], c->G32,
                       c->yrow, c->st, c->lay, c->etaVec, (long long)c->L, (int)c->H, c->Hp, c->zetav, c->sigv, c->sig32, c->hpart, stop);
    if (sharded(c)) {
        // this rank's share of the mean goes through a staging pair of its own, reduced OUT OF PLACE (after `stop` the gated
        // kernels leave the share alone and the re-reduction reproduces the same sum; c->gtmp is NOT scratch: it holds the B
        // side's partials, which a sweep enqueued after the stop reduces again), then a gated copy into the state
        hipLaunchKernelGGL(hetero_mean_kernel, dim3(1), dim3(256), 0, c->stream, c->hpart, nb, (double)c->Lg, c->hmean, stop);
        TRY(allreduce_sum(c, c->hmean, c->hmean + 1, 1, true));
        hipLaunchKernelGGL(gated_copy_kernel, dim3(1), dim3(64), 0, c->stream, c->hmean + 1, c->st + c->lay.scal() + S_SIGMA2, 1, stop);
    } else {
        hipLaunchKernelGGL(hetero_mean_kernel, dim3(1), dim3(256), 0, c->stream, c->hpart, nb, (double)c->L, c->st + c->lay.scal() + S_SIGMA2, stop);
    }
    HIPCHK(c, hipGetLastError());
    return VBMF_OK;
}

static int sparse_update_CA(vbmf_ctx* c) {
    hipLaunchKernelGGL(sparse_update_ca_kernel, dim3(grid_for((int64_t)c->M * c->Hp)), dim3(256), 0, ctrl_stream(c), c->A32, c->dS32,
                       c->beta32, c->CA32, c->alpha, c->hyp.beta0, (long long)c->M, (int)c->H, c->Hp, c->ints + I_STOP,
                       c->dual ? c->st + c->lay.scal() : (double*)nullptr, (int)c->H0, (long long)c->M0,
                       c->dual ? c->gpart : (double*)nullptr);
    HIPCHK(c, hipGetLastError());
    return VBMF_OK;
}
// est_priors of vbmf_dual! (src/vbmf_dual.jl:491-495); needs the group sums of the sweep's updateCA!
static int dual_update_priors(vbmf_ctx* c) {
    hipLaunchKernelGGL(group_priors_kernel, dim3(1), dim3(256), 0, c->stream, c->gpart, c->gpart_blocks, c->st, c->lay,
                       (double)c->M, (int)c->H, (int)c->H0, (double)c->M0, c->ints + I_STOP);
    HIPCHK(c, hipGetLastError());
    return VBMF_OK;
}

// t2_ahead: the shares of sum (GA + SA) o (GB + L SB) were left in c->t2part by launch_sparse_t2 (same stream, earlier)
static int launch_sparse_t2(vbmf_ctx* c) {
    if (!c->t2part) {
        MEMCHK(c, c->mem.acquire(c->t2part, T2_BLOCKS * 8));
        HIPCHK(c, hipMemsetAsync(c->t2part, 0, T2_BLOCKS * 8, ctrl_stream(c)));   // ordered before the kernel below
    }
    hipLaunchKernelGGL(sparse_t2_kernel, dim3(T2_BLOCKS), dim3(256), 0, ctrl_stream(c), c->st, c->lay, (int)c->H, (double)c->Lg, c->t2part, c->ints);
    HIPCHK(c, hipGetLastError());
    return VBMF_OK;
}
static int launch_sparse_ctrl_end(vbmf_ctx* c, int flags, double eps, double* trace, bool t2_ahead = false) {
    hipLaunchKernelGGL(sparse_ctrl_end_kernel, dim3(1), dim3(c->H > 64 ? 1024 : 256), 0, ctrl_stream(c), c->st, c->lay, (int)c->H, (double)c->Lg, flags, eps, trace, c->ints,
                       t2_ahead ? (const double*)c->t2part : (const double*)nullptr, loop_words(c));
    HIPCHK(c, hipGetLastError());
    return VBMF_OK;
}

// One sweep of the diagonal homoscedastic model from P = Y'B_old = G W_old (in gPQ) and the state's B'B = W'P:
// v, the A update straight from the fragment-major P (label mask, operand tiles), A'A, SigmaA, SigmaB with its sigmaHat SigmaB table, then
// W_new = A (sigmaHat SigmaB), [P | Q] = G [W_new | W_new - W_old] and the state's [B'B | dB'dB | tr(B'YA)] from them.  Y is not read.
// updateCA!, lambda_max and the closing control step follow in sparse_run_impl, as after a streaming sweep.
static int sparse_gram_sweep(vbmf_ctx* c) {
    const int* stop = c->ints + I_STOP;
    hipLaunchKernelGGL(sparse_v_kernel, dim3((c->Hp + 63) / 64), dim3(64), 0, c->stream, c->st, c->lay, (int)c->H, (double)c->Lg, c->vtab,
                       (const double*)nullptr, stop);
    const int compat = (c->o.reference_compat & VBMF_COMPAT_SPARSE_REPEAT) ? 1 : 0;
    if (compat && c->M < 2) FAIL(c, VBMF_ERR_INVALID, "repeat(v, inner=M-1) needs M >= 2");
    const float4* P4 = reinterpret_cast<const float4*>(c->gPQ);
    const unsigned char* mk = c->has_mask ? c->mask : nullptr;
    const int hstart = (int)(c->H - c->H1);
    const dim3 grid((c->d1.XT * c->NH + 3) / 4);
    if (!dispatch<1, 2, 4, 8>(c->NH, [&](auto nh) {
            hipLaunchKernelGGL((sparse_update_a_frag_kernel<MODE_BF16X2, decltype(nh)::value>), grid, dim3(256), 0, c->stream, P4, c->CA32, c->vtab,
                               c->st, c->lay, c->A32, c->dS32, c->FA, mk, hstart, (long long)c->M, (int)c->H, compat, c->d1.XT, stop);
        })) FAIL(c, VBMF_ERR_INVALID, "internal: the Gram-form sweep covers Hp <= 256");
    HIPCHK(c, hipGetLastError());
    c->P_frag = true;
    c->frag_last[0] = true;                         // test surface: this sweep's Y'B was the fragment-major G W, not a pass over Y
    TRY(launch_gram(c, 0, c->A32, nullptr, true));
    TRY(sparse_colsum(c));                          // SigmaA = diag(sum_m diagSigma)
    TRY(launch_sparse_cov_b(c));
    TRY(gram_product(c, true));
    c->wcur ^= 1;
    c->cache.gram_sweep_done_sparse();
    return VBMF_OK;
}

static int upload_vec(vbmf_ctx* c, const double* src, float* dst, float fill) {
    DevScratch<double> tmp;
    const size_t n = (size_t)c->M * c->H;
    MEMCHK(c, tmp.alloc(n * 8));
    hipError_t e = hipMemcpyAsync(tmp, src, n * 8, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(pack_vec_kernel, dim3(grid_for(c->Mp * c->Hp)), dim3(256), 0, c->stream, tmp.get(), (long long)c->M, (int)c->H, c->Hp, (long long)c->Mp, dst, fill);
        e = hipStreamSynchronize(c->stream);
    }
    if (e != hipSuccess) FAIL(c, VBMF_ERR_HIP, "vec upload failed: %s", hipGetErrorString(e));
    return VBMF_OK;
}
static int download_vec(vbmf_ctx* c, const float* src, double* dst) {
    DevScratch<double> tmp;
    const size_t n = (size_t)c->M * c->H;
    MEMCHK(c, tmp.alloc(n * 8));
    hipLaunchKernelGGL(unpack_vec_kernel, dim3(grid_for((int64_t)n)), dim3(256), 0, c->stream, src, (long long)c->M, (int)c->H, c->Hp, tmp.get());
    hipError_t e = hipMemcpyAsync(dst, tmp, n * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) FAIL(c, VBMF_ERR_HIP, "vec download failed: %s", hipGetErrorString(e));
    return VBMF_OK;
}

extern "C" {

int vbmf_sparse_set_state(vbmf_ctx* c, const double* ATVecHat, const double* diagSigmaATVec, const double* CA,
                          const double* beta, const double* BHat, int64_t ldB, const double* SigmaB,
                          const double* CB, const double* delta, double sigmaHat, double zeta,
                          const vbmf_sparse_hyper* hyper, const int64_t* labels0, int64_t nlabels, int64_t H1) {
    if (!c) return VBMF_ERR_INVALID;
    if (!c->sparse) FAIL(c, VBMF_ERR_INVALID, "not a sparse context (opts.variant)");
    if (!ATVecHat || !diagSigmaATVec || !CA || !beta || !BHat || !SigmaB || !CB || !delta || !hyper)
        FAIL(c, VBMF_ERR_INVALID, "vbmf_sparse_set_state: null pointer");
    if (ldB < c->L) FAIL(c, VBMF_ERR_INVALID, "ldB < L");
    if (H1 < 0 || H1 > c->H || nlabels < 0 || (nlabels > 0 && !labels0)) FAIL(c, VBMF_ERR_INVALID, "bad H1/labels");
    if (c->dual && nlabels > 0) FAIL(c, VBMF_ERR_INVALID, "the grouped models have no label mask (src/vbmf_dual.jl:282-284)");
    if (!(sigmaHat > 0.0)) FAIL(c, VBMF_ERR_INVALID, "sigmaHat must be positive");
    for (int64_t h = 0; h < c->H; ++h) if (!(CB[h] > 0.0)) FAIL(c, VBMF_ERR_INVALID, "CB must be positive");
    HIPCHK(c, hipSetDevice(c->o.device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->hyp = *hyper;
    c->alpha = hyper->alpha0 + 0.5;                                   // src/vbmf_sparse.jl:131
    c->gamma_ = hyper->gamma0 + 0.5 * (double)c->Lg;                  // :137
    c->eta = hyper->eta0 + 0.5 * (double)c->Lg * (double)c->M;        // :143
    c->bcur = 0;
    TRY(upload_vec(c, ATVecHat, c->A32, 0.f));
    TRY(upload_vec(c, diagSigmaATVec, c->dS32, 0.f));
    TRY(upload_vec(c, CA, c->CA32, 1.f));
    TRY(upload_vec(c, beta, c->beta32, 1.f));
    TRY(upload_factor(c, BHat, ldB, c->L, c->Lp, c->B32[0]));
    TRY(upload_small(c, SigmaB, c->lay.SB(), true));
    TRY(upload_small(c, CB, c->lay.cb(), false));
    TRY(upload_small(c, delta, c->lay.ca(), false));
    double sc[32];
    HIPCHK(c, memcpy_sync(c, sc, c->st + c->lay.scal(), sizeof sc, hipMemcpyDeviceToHost));
    sc[S_SIGMA2] = sigmaHat; sc[S_ZETA] = zeta; sc[S_ALPHA] = c->alpha; sc[S_GAMMA] = c->gamma_; sc[S_ETA] = c->eta;
    sc[S_BETA0] = hyper->beta0; sc[S_DELTA0] = hyper->delta0; sc[S_ZETA0] = hyper->zeta0;
    // two-group model: both groups start from (alpha0, beta0) and H0 = H until vbmf_dual_set_priors says otherwise
    for (int g = 0; g < 3; ++g) { sc[S_GPRI + 2 * g] = hyper->alpha0; sc[S_GPRI + 2 * g + 1] = hyper->beta0; sc[S_GPOST + g] = hyper->alpha0 + 0.5; }
    if (c->dual) { c->H0 = c->H; c->M0 = c->M; }
    HIPCHK(c, memcpy_sync(c, c->st + c->lay.scal(), sc, sizeof sc, hipMemcpyHostToDevice));
    std::vector<unsigned char> mk((size_t)c->Mp, 0);
    for (int64_t i = 0; i < nlabels; ++i) {
        if (labels0[i] < 0 || labels0[i] >= c->M) FAIL(c, VBMF_ERR_INVALID, "label out of range");
        mk[(size_t)labels0[i]] = 1;
    }
    HIPCHK(c, memcpy_sync(c, c->mask, mk.data(), mk.size(), hipMemcpyHostToDevice));
    c->H1 = H1;
    c->has_mask = (nlabels > 0 && H1 > 0);
    TRY(launch_retile(c, 0));
    TRY(launch_retile(c, 1));
    TRY(sparse_colsum(c));
    const int H = (int)c->H;
    const size_t need = ((size_t)H * H + 2 * H) * sizeof(double);
    const int use_lds = need <= 60 * 1024;
    hipLaunchKernelGGL(logdet_kernel, dim3(1), dim3(ctrl_threads(H)), use_lds ? need : 0, c->stream, c->st, c->lay, H, 1, use_lds);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemsetAsync(c->ints, 0, 16 * sizeof(int), c->stream));
    if (c->dbg_sb_ppm) HIPCHK(c, hipMemcpyAsync(c->ints + I_DBG_SB_PPM, &c->dbg_sb_ppm, sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->cache.state_set_sparse();
    return VBMF_OK;
}

int vbmf_sparse_get_state(vbmf_ctx* c, double* ATVecHat, double* diagSigmaATVec, double* CA, double* beta,
                          double* SigmaA_diag, double* BHat, int64_t ldB, double* SigmaB, double* CB,
                          double* delta, double* sigmaHat, double* zeta) {
    if (!c) return VBMF_ERR_INVALID;
    if (!c->sparse || !c->cache.have_state()) FAIL(c, VBMF_ERR_INVALID, "no sparse state");
    HIPCHK(c, hipSetDevice(c->o.device));
    if (BHat) TRY(ensure_B(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (ATVecHat) TRY(download_vec(c, c->A32, ATVecHat));
    if (diagSigmaATVec) TRY(download_vec(c, c->dS32, diagSigmaATVec));
    if (CA) TRY(download_vec(c, c->CA32, CA));
    if (beta) TRY(download_vec(c, c->beta32, beta));
    if (BHat) { if (ldB < c->L) FAIL(c, VBMF_ERR_INVALID, "ldB < L"); TRY(download_factor(c, c->B32[c->bcur], c->L, BHat, ldB)); }
    std::vector<double> buf((size_t)c->lay.total());
    HIPCHK(c, memcpy_sync(c, buf.data(), c->st, buf.size() * 8, hipMemcpyDeviceToHost));
    for (int64_t h = 0; h < c->H; ++h) {
        if (SigmaA_diag) SigmaA_diag[h] = buf[(size_t)c->lay.SA() + (size_t)h * c->Hp + h];
        if (CB) CB[h] = buf[(size_t)c->lay.cb() + h];
        if (delta) delta[h] = buf[(size_t)c->lay.ca() + h];
    }
    if (SigmaB)
        for (int64_t j = 0; j < c->H; ++j)
            for (int64_t i = 0; i < c->H; ++i) SigmaB[i + j * c->H] = buf[(size_t)c->lay.SB() + (size_t)i * c->Hp + j];
    if (sigmaHat) *sigmaHat = buf[(size_t)c->lay.scal() + S_SIGMA2];
    if (zeta) *zeta = buf[(size_t)c->lay.scal() + S_ZETA];
    return VBMF_OK;
}

int vbmf_sparse_step(vbmf_ctx* c, int which) {
    if (!c) return VBMF_ERR_INVALID;
    if (!c->sparse) FAIL(c, VBMF_ERR_INVALID, "not a sparse context");
    if (which & ~(c->dual ? 63 : 31)) FAIL(c, VBMF_ERR_INVALID, "vbmf_sparse_step: unknown update bits");
    if ((which & VBMF_SSTEP_PRIORS) && !(which & VBMF_SSTEP_CA))
        FAIL(c, VBMF_ERR_INVALID, "VBMF_SSTEP_PRIORS needs the group sums of VBMF_SSTEP_CA in the same call");
    HIPCHK(c, hipSetDevice(c->o.device));
    TRY(ensure_ready(c, (which & (VBMF_SSTEP_A | VBMF_SSTEP_B | VBMF_SSTEP_SIGMA)) != 0));
    c->cache.W_dropped();
    if (which & VBMF_SSTEP_A) TRY(do_sparse_update_A(c));
    if (which & VBMF_SSTEP_B) TRY(do_sparse_update_B(c));
    if (which & VBMF_SSTEP_CA) TRY(sparse_update_CA(c));
    int flags = 0;
    if (which & VBMF_SSTEP_CB) { TRY(ensure_gram_B(c)); flags |= 2; }
    if ((which & VBMF_SSTEP_SIGMA) && c->diagvar) {
        if (flags) TRY(launch_sparse_ctrl_end(c, flags, 0.0, nullptr));
        flags = 0;
        TRY(do_hetero_sigma(c));
    } else if (which & VBMF_SSTEP_SIGMA) {
        TRY(ensure_gram_A(c));
        TRY(ensure_gram_B(c));
        int f = 0;
        TRY(prepare_trYBA(c, &f));
        flags |= 4 | f;
    }
    if (flags) TRY(launch_sparse_ctrl_end(c, flags, 0.0, nullptr));
    if (which & VBMF_SSTEP_PRIORS) TRY(dual_update_priors(c));
    return check_device_err(c);
}

// vbls!, vbmf_sparse_parameters branch (examples/mil_util.jl:187-190): updateA!, updateCA!, updateSigma! with B frozen
int vbmf_sparse_run_fixed_basis(vbmf_ctx* c, int64_t niter) {
    if (!c) return VBMF_ERR_INVALID;
    if (!c->sparse) FAIL(c, VBMF_ERR_INVALID, "not a sparse context");
    if (niter < 0 || niter > (1ll << 30)) FAIL(c, VBMF_ERR_INVALID, "bad niter");
    HIPCHK(c, hipSetDevice(c->o.device));
    TRY(ensure_ready(c));
    c->cache.W_dropped();
    for (int64_t it = 0; it < niter; ++it) {
        TRY(do_sparse_update_A(c, true));
        TRY(sparse_update_CA(c));
        TRY(ensure_gram_A(c));
        if (c->diagvar) {                               // sigma_l changes Y' diag(sigma) B every iteration: both passes
            TRY(do_hetero_sigma(c));
            continue;
        }
        int f = 0;
        TRY(prepare_trYBA(c, &f));
        TRY(launch_sparse_ctrl_end(c, 4 | f, 0.0, nullptr));
        if ((it & 63) == 63) TRY(check_device_err(c));
    }
    return check_device_err(c);
}

static int sparse_run_impl(vbmf_ctx* c, int64_t niter, double eps, int est_cb, int est_priors, int64_t* iters_done,
                           double* d_last, double* trace) {
    if (!c) return VBMF_ERR_INVALID;
    if (!c->sparse) FAIL(c, VBMF_ERR_INVALID, "not a sparse context");
    if (niter < 0 || niter > (1ll << 30)) FAIL(c, VBMF_ERR_INVALID, "bad niter");
    RunFrame run{c, niter, eps, iters_done, d_last, trace};
    TRY(run.open());
    if (niter == 0) return VBMF_OK;
    TRY(run.begin_gram());
    TRY(run.arm());
    int rc = ensure_gram_B(c);
    if (rc == VBMF_OK) rc = launch_eig(c, 0, 1);
    if (rc == VBMF_OK)
        hipLaunchKernelGGL(copy_scalar_kernel, dim3(1), dim3(1), 0, c->stream, c->st, c->lay, (int)S_LAMB_PREV, (int)S_LAMB_NEW);
    // diag_var: the rows' noise update (:308-315) replaces the scalar one and runs before the stop test of the sweep
    const int flags = (est_cb ? 2 : 0) | (c->diagvar ? 0 : 4 | 16) | 8;
    const int64_t check = 8;                               // sweeps between two looks at the stop flag (RunFrame::look)
    int64_t it = 0;
    bool stopped = false;
    c->in_run = true;
    while (rc == VBMF_OK && it < niter && !stopped) {
        if (run.gram && c->cache.W()) {
            rc = sparse_gram_sweep(c);
        } else {
            rc = do_sparse_update_A(c);
            if (rc == VBMF_OK) rc = do_sparse_update_B(c);
            rc = run.close_stream_sweep(rc);
        }
        // updateCA! reads what the A update left and writes what the NEXT A update reads: with a side stream (H > 128) it runs there too,
        // beside the next sweep's Y'B pass, instead of 13 us between the sweeps (not with the group priors or the row noise behind it)
        // In a Gram-form run (rank 256 under VBMF_GRAM_FORM_ON) nothing is forked: whatever follows this sweep -- a Gram sweep, whose
        // first kernel (sparse_v) reads the sigmaHat, B'B and SigmaB the control step writes, or the run's end -- has no pass over Y to
        // hide the chain behind.  The run's first, streaming sweep keeps the forks inside its two updates (joined before its post kernel).
        const bool overlap = side_overlap(c) && !run.gram;
        const bool ca_on_side = overlap && !est_priors && !c->diagvar;
        if (rc == VBMF_OK && !ca_on_side) rc = sparse_update_CA(c);
        if (rc == VBMF_OK && est_priors) rc = dual_update_priors(c);      // depends on updateCA!'s outputs only
        if (rc == VBMF_OK && c->diagvar) rc = do_hetero_sigma(c);
        // lambda_max, CB, sigma, d and the stop test: beside the next sweep's Y'B pass when they run on the side stream
        if (rc == VBMF_OK && overlap) rc = side_fork(c);
        if (rc == VBMF_OK && ca_on_side) rc = sparse_update_CA(c);
        const bool t2_ahead = c->use_side && !c->diagvar;        // (diag_var: no scalar noise update, t2 is not used)
        if (rc == VBMF_OK && t2_ahead) rc = launch_sparse_t2(c);   // 64 workgroups, before the long lambda_max kernel
        if (rc == VBMF_OK) rc = launch_eig(c, 1, 1);
        if (rc == VBMF_OK) rc = launch_sparse_ctrl_end(c, flags, eps, run.trace_dev, t2_ahead);
        if (rc == VBMF_OK && c->use_side) rc = side_end(c);
        ++it;
        if (rc == VBMF_OK && (it % check == 0 || it == niter)) {
            rc = side_join(c);
            if (rc != VBMF_OK) break;
            if (it < niter) stopped = run.look(it, check);      // (see vbmf_run; the run's end drains the stream in finish())
        }
    }
    // every streaming sweep moves B; in the Gram form only the streaming sweep (the first, if any) does, and every sweep moves W
    return run.finish(rc, run.bstart, run.gram ? run.stream_sweeps : niter);
}

int vbmf_sparse_run(vbmf_ctx* c, int64_t niter, double eps, int est_cb, int64_t* iters_done, double* d_last,
                    double* trace) {
    return sparse_run_impl(c, niter, eps, est_cb, 0, iters_done, d_last, trace);
}

// full_cov = true of updateA! (src/vbmf_sparse.jl:178-202): homoscedastic models, H <= 64
int vbmf_sparse_set_full_cov(vbmf_ctx* c, int on) {
    if (!c) return VBMF_ERR_INVALID;
    if (!c->sparse) FAIL(c, VBMF_ERR_INVALID, "not a sparse context");
    if (on && c->H > 256) FAIL(c, VBMF_ERR_UNSUPPORTED, "full_cov is built for H <= 256");
    HIPCHK(c, hipSetDevice(c->o.device));
    TRY(ensure_B(c));
    if (on && !c->fpart) {
        // two columns per round and workgroup (one for H > 64); H > 128: one 1024-thread workgroup per CU with its own workspace
        c->fblocks = (int)std::max<int64_t>(1, std::min<int64_t>(c->H > 64 ? c->M : (c->M + 1) / 2, c->H > 128 ? NUM_CU : 1024));
        const size_t bytes = (size_t)c->fblocks * c->Hp * c->Hp * 8;
        // fws and fpart are one group: a failure leaves both null, so the guard above never sees one without the other
        const size_t group = c->mem.mark();
        int e = c->H > 128 ? c->mem.acquire(c->fws, (size_t)c->fblocks * FULL256_WS * 8) : 0;
        if (e == 0) e = c->mem.acquire(c->fpart, bytes);
        if (e != 0) {
            c->mem.rollback(group);
            FAIL(c, VBMF_ERR_HIP, "vbmf_sparse_set_full_cov: device allocation failed (%s)", mem_errstr(e));
        }
        HIPCHK(c, hipMemsetAsync(c->fpart, 0, bytes, c->stream));   // its kernels run on c->stream
    }
    if (on && c->diagvar && !c->gw) {
        const size_t bytes = (size_t)2 * c->Hp * c->Hp * 8;
        MEMCHK(c, c->mem.acquire(c->gw, bytes));
        HIPCHK(c, hipMemsetAsync(c->gw, 0, bytes, c->stream));
    }
    c->full_cov = on != 0;
    c->cache.W_dropped();                              // (full_cov on: the context leaves the Gram form, gram_structural)
    return VBMF_OK;
}

// which form the run loops take (gram_eligible); never fails for a structure that cannot take the Gram form -- VBMF_PEEK_DIMS
// reports what was resolved.  The next run starts by the streaming path.
int vbmf_set_gram_form(vbmf_ctx* c, int mode) {
    if (!c) return VBMF_ERR_INVALID;
    if (mode != VBMF_GRAM_FORM_DEFAULT && mode != VBMF_GRAM_FORM_OFF && mode != VBMF_GRAM_FORM_ON)
        FAIL(c, VBMF_ERR_INVALID, "vbmf_set_gram_form: unknown mode %d", mode);
    HIPCHK(c, hipSetDevice(c->o.device));
    TRY(ensure_B(c));
    c->gram_form = mode;
    c->cache.W_dropped();
    return VBMF_OK;
}

// SigmaA as a full H x H matrix (column-major): the diagonal branch keeps it diagonal, the full branch does not, and
// vbmf_sparse_set_state derives it from diagSigmaATVec -- a caller continuing a full_cov state sets it explicitly.
int vbmf_sparse_set_SigmaA(vbmf_ctx* c, const double* SigmaA) {
    if (!c || !SigmaA) return VBMF_ERR_INVALID;
    if (!c->sparse || !c->cache.have_state()) FAIL(c, VBMF_ERR_INVALID, "no sparse state");
    HIPCHK(c, hipSetDevice(c->o.device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    TRY(upload_small(c, SigmaA, c->lay.SA(), true));
    c->cache.SigmaA_set();
    return VBMF_OK;
}

int vbmf_sparse_get_SigmaA(vbmf_ctx* c, double* SigmaA) {
    if (!c || !SigmaA) return VBMF_ERR_INVALID;
    if (!c->sparse || !c->cache.have_state()) FAIL(c, VBMF_ERR_INVALID, "no sparse state");
    HIPCHK(c, hipSetDevice(c->o.device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<double> buf((size_t)c->Hp * c->Hp);
    HIPCHK(c, memcpy_sync(c, buf.data(), c->st + c->lay.SA(), buf.size() * 8, hipMemcpyDeviceToHost));
    for (int64_t j = 0; j < c->H; ++j)
        for (int64_t i = 0; i < c->H; ++i) SigmaA[i + j * c->H] = buf[(size_t)i * c->Hp + j];
    return VBMF_OK;
}

// ---- grouped ARD variants (src/vbmf_dual.jl, src/vbmf_trial.jl; full_cov=false, diag_var=false) -------------------
// priors9 = {alpha0 prior, beta0 prior} x 3 groups, then the 3 posterior shapes
static int group_set_priors(vbmf_ctx* c, int64_t H0, int64_t M0, const double* v9) {
    if (!c->cache.have_state()) FAIL(c, VBMF_ERR_INVALID, "call vbmf_sparse_set_state first");
    if (H0 < 0 || H0 > c->H) FAIL(c, VBMF_ERR_INVALID, "H must be at least H0!");          // src/vbmf_dual.jl:126-128
    if (M0 < 0 || M0 > c->M) FAIL(c, VBMF_ERR_INVALID, "M0 must lie in 0..M");
    for (int i = 0; i < 9; ++i)
        if (!(v9[i] > 0.0) || !std::isfinite(v9[i])) FAIL(c, VBMF_ERR_INVALID, "the Gamma hyper-priors must be positive");
    HIPCHK(c, hipSetDevice(c->o.device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, memcpy_sync(c, c->st + c->lay.scal() + S_GPRI, v9, 9 * 8, hipMemcpyHostToDevice));
    c->H0 = H0;
    c->M0 = M0;
    return VBMF_OK;
}

int vbmf_dual_set_priors(vbmf_ctx* c, int64_t H0, double alpha00, double beta00, double alpha01, double beta01,
                         double alpha0, double alpha1) {
    if (!c) return VBMF_ERR_INVALID;
    if (!c->dual || c->trial) FAIL(c, VBMF_ERR_INVALID, "not a two-group context (opts.variant = VBMF_VARIANT_DUAL_DIAG)");
    const double v[9] = {alpha00, beta00, alpha01, beta01, alpha01, beta01, alpha0, alpha1, alpha1};   // third group: empty
    return group_set_priors(c, H0, c->M, v);
}

int vbmf_dual_get_priors(vbmf_ctx* c, int64_t* H0, double* priors6) {
    if (!c) return VBMF_ERR_INVALID;
    if (!c->dual || c->trial || !c->cache.have_state()) FAIL(c, VBMF_ERR_INVALID, "no two-group state");
    HIPCHK(c, hipSetDevice(c->o.device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (H0) *H0 = c->H0;
    if (priors6) {
        double v[9];
        HIPCHK(c, memcpy_sync(c, v, c->st + c->lay.scal() + S_GPRI, sizeof v, hipMemcpyDeviceToHost));
        priors6[0] = v[0]; priors6[1] = v[1]; priors6[2] = v[2]; priors6[3] = v[3]; priors6[4] = v[6]; priors6[5] = v[7];
    }
    return VBMF_OK;
}

int vbmf_dual_run(vbmf_ctx* c, int64_t niter, double eps, int est_cb, int est_priors, int64_t* iters_done,
                  double* d_last, double* trace) {
    if (!c) return VBMF_ERR_INVALID;
    if (!c->dual || c->trial) FAIL(c, VBMF_ERR_INVALID, "not a two-group context (opts.variant = VBMF_VARIANT_DUAL_DIAG)");
    return sparse_run_impl(c, niter, eps, est_cb, est_priors ? 1 : 0, iters_done, d_last, trace);
}

int vbmf_trial_set_priors(vbmf_ctx* c, int64_t H0, int64_t M0, const double* priors9) {
    if (!c || !priors9) return VBMF_ERR_INVALID;
    if (!c->trial) FAIL(c, VBMF_ERR_INVALID, "not a three-group context (opts.variant = VBMF_VARIANT_TRIAL_DIAG)");
    return group_set_priors(c, H0, M0, priors9);
}

int vbmf_trial_get_priors(vbmf_ctx* c, int64_t* H0, int64_t* M0, double* priors9) {
    if (!c) return VBMF_ERR_INVALID;
    if (!c->trial || !c->cache.have_state()) FAIL(c, VBMF_ERR_INVALID, "no three-group state");
    HIPCHK(c, hipSetDevice(c->o.device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (H0) *H0 = c->H0;
    if (M0) *M0 = c->M0;
    if (priors9) HIPCHK(c, memcpy_sync(c, priors9, c->st + c->lay.scal() + S_GPRI, 9 * 8, hipMemcpyDeviceToHost));
    return VBMF_OK;
}

int vbmf_trial_run(vbmf_ctx* c, int64_t niter, double eps, int est_cb, int est_priors, int64_t* iters_done,
                   double* d_last, double* trace) {
    if (!c) return VBMF_ERR_INVALID;
    if (!c->trial) FAIL(c, VBMF_ERR_INVALID, "not a three-group context (opts.variant = VBMF_VARIANT_TRIAL_DIAG)");
    return sparse_run_impl(c, niter, eps, est_cb, est_priors ? 1 : 0, iters_done, d_last, trace);
}

// sigmaVecHat, zetaVec (length L each) and the common shape etaVec = eta0 + M/2 (src/vbmf_sparse.jl:145-147) of the
// heteroscedastic model (opts.variant = VBMF_VARIANT_SPARSE_DIAGVAR).  Call after vbmf_sparse_set_state.
int vbmf_sparse_set_noise_rows(vbmf_ctx* c, const double* sigmaVecHat, const double* zetaVec, double etaVec) {
    if (!c || !sigmaVecHat || !zetaVec) return VBMF_ERR_INVALID;
    if (!c->diagvar) FAIL(c, VBMF_ERR_INVALID, "not a heteroscedastic context (opts.variant)");
    HIPCHK(c, hipSetDevice(c->o.device));
    std::vector<float> s32((size_t)c->Lp, 0.f);
    double mean = 0.0;
    for (int64_t l = 0; l < c->L; ++l) { s32[(size_t)l] = (float)sigmaVecHat[l]; mean += sigmaVecHat[l]; }
    mean /= (double)c->Lg;                                   // this rank's share of the mean over ALL rows
    HIPCHK(c, memcpy_sync(c, c->sigv, sigmaVecHat, (size_t)c->L * 8, hipMemcpyHostToDevice));
    HIPCHK(c, memcpy_sync(c, c->zetav, zetaVec, (size_t)c->L * 8, hipMemcpyHostToDevice));
    HIPCHK(c, memcpy_sync(c, c->sig32, s32.data(), (size_t)c->Lp * 4, hipMemcpyHostToDevice));
    HIPCHK(c, memcpy_sync(c, c->st + c->lay.scal() + S_SIGMA2, &mean, 8, hipMemcpyHostToDevice));
    c->etaVec = etaVec;
    c->cache.noise_rows_set();
    return VBMF_OK;
}

int vbmf_sparse_get_noise_rows(vbmf_ctx* c, double* sigmaVecHat, double* zetaVec) {
    if (!c) return VBMF_ERR_INVALID;
    if (!c->diagvar || !c->cache.have_noise()) FAIL(c, VBMF_ERR_INVALID, "no row noise state");
    HIPCHK(c, hipSetDevice(c->o.device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (sigmaVecHat) HIPCHK(c, memcpy_sync(c, sigmaVecHat, c->sigv, (size_t)c->L * 8, hipMemcpyDeviceToHost));
    if (zetaVec) HIPCHK(c, memcpy_sync(c, zetaVec, c->zetav, (size_t)c->L * 8, hipMemcpyDeviceToHost));
    return VBMF_OK;
}

}  // extern "C"

// Everything lowerBound reads, as sums: filled from a whole context (sparse_lower_bound_impl, three ARD groups) or from one bag of a
// batched call (vbmf_sparse_lower_bound_batched, one ARD group per column of A), assembled by lb_assemble.
struct LbGroup { double n, s_logbeta, s_ca, a_pri, b_pri, a_post; };   // entries, sum log beta, sum CA, prior (shape, rate), posterior shape
struct LbSums {
    double L, M, H, MH;                  // MH: params.MH, the length of the (trimmed) ATVecHat (:483); every other size is the model's own
    double sig, zeta, eta;               // noise precision, its Gamma posterior (eta, zeta)
    double quad;                         // ||Y||^2 - 2 tr(B'YA) + tr((A'A + SigmaA)(B'B + L SigmaB))  (:439-440)
    double s_caq, s_logds;               // sum' CA (a^2 + dS), sum' log dS
    double cbq, sumcb, sumlogdelta;      // sum_h CB_h (B'B + L SigmaB)_hh, sum CB, sum log delta
    double logdet_sb, gamma_;
    vbmf_sparse_hyper hyp;               // gamma0, delta0, eta0, zeta0 (alpha0 / beta0 travel per group)
    const LbGroup* g; int ng;
};

// src/vbmf_sparse.jl:438-469 with the group terms of src/vbmf_dual.jl:556-599 and src/vbmf_trial.jl:630-680, fp64 on the host
static double lb_assemble(const LbSums& s, int clamp) {
    const double L = s.L, M = s.M, H = s.H, MH = s.MH;
    const double LN2PI = std::log(2.0 * M_PI);
    const double sig = s.sig, zeta = s.zeta;
    const vbmf_sparse_hyper& hp = s.hyp;
    const double eln_sig = digamma_host(s.eta) - std::log(zeta);
    std::vector<double> eln_g((size_t)s.ng);
    double s_eln_ca = 0.0;
    for (int g = 0; g < s.ng; ++g) {
        eln_g[(size_t)g] = s.g[g].n > 0 ? s.g[g].n * digamma_host(s.g[g].a_post) - s.g[g].s_logbeta : 0.0;
        s_eln_ca = g == 0 ? eln_g[0] : s_eln_ca + eln_g[(size_t)g];
    }
    const double s_eln_cb = H * digamma_host(s.gamma_) - s.sumlogdelta;
    double Lb = 0.0;
    Lb += -L * M / 2 * LN2PI + L * M / 2 * eln_sig;                                        // :438
    Lb += -sig / 2 * s.quad;                                                               // :439-440
    Lb += -MH / 2 * LN2PI + 0.5 * s_eln_ca;                                                // :442
    Lb += -0.5 * s.s_caq;                                                                  // :443
    Lb += -L * H / 2 * LN2PI;                                                              // :445
    Lb += L / 2 * s_eln_cb;                                                                // :446
    Lb += -0.5 * s.cbq;                                                                    // :447
    Lb += hp.eta0 * std::log(hp.zeta0) - std::lgamma(hp.eta0);                             // :449
    Lb += (hp.eta0 - 1) * eln_sig - hp.zeta0 * sig;                                        // :450
    for (int g = 0; g < s.ng; ++g) {                                                       // one group in the sparse model
        const LbGroup& q = s.g[g];
        if (!(q.n > 0)) continue;
        Lb += q.n * (q.a_pri * std::log(q.b_pri) - std::lgamma(q.a_pri));                  // :452   (dual :575, 579)
        Lb += (q.a_pri - 1) * eln_g[(size_t)g];                                            // :453   (dual :576, 580)
        Lb += -q.b_pri * q.s_ca;                                                           // :454   (dual :577, 581)
    }
    Lb += H * (hp.gamma0 * std::log(hp.delta0) - std::lgamma(hp.gamma0));                  // :456
    Lb += (hp.gamma0 - 1) * s_eln_cb;                                                      // :457
    Lb += -hp.gamma0 * s.sumcb;                                                            // :458 (sic: gamma0)
    Lb += MH / 2 + MH / 2 * LN2PI + 0.5 * s.s_logds;                                       // :461 normalEntropy(diag)
    double logdet_kron = L * s.logdet_sb;                                                  // det(kron(SigmaB, I_L)) = det(SigmaB)^L
    if (clamp) logdet_kron = std::max(logdet_kron, std::log(4.9406564584124654e-324));     // src/util.jl:118-122
    Lb += L * H / 2 + L * H / 2 * LN2PI + 0.5 * logdet_kron;                               // :463
    Lb += s.eta + std::log(zeta) + std::lgamma(s.eta) + (1 - s.eta) * digamma_host(s.eta);                   // :465
    for (int g = 0; g < s.ng; ++g) {                                                                         // :467 (dual :594, 596)
        const LbGroup& q = s.g[g];
        if (q.n > 0) Lb += q.n * (q.a_post + std::lgamma(q.a_post) + (1 - q.a_post) * digamma_host(q.a_post)) + q.s_logbeta;
    }
    Lb += H * (s.gamma_ + std::lgamma(s.gamma_) + (1 - s.gamma_) * digamma_host(s.gamma_)) + s.sumlogdelta;  // :469
    return Lb;
}

// the basis' share of the sums (B'B, SigmaB, CB, delta of the state image `buf`)
static void lb_basis_sums(const vbmf_ctx* c, const std::vector<double>& buf, LbSums& s) {
    const double L = (double)c->Lg;
    auto at = [&](long long off, int i, int j) { return buf[(size_t)off + (size_t)i * c->Hp + j]; };
    double cbq = 0, sumcb = 0, sumlogdelta = 0;
    for (int i = 0; i < c->H; ++i) {
        const double cb = buf[(size_t)c->lay.cb() + i];
        cbq += cb * (at(c->lay.GB(), i, i) + L * at(c->lay.SB(), i, i));
        sumcb += cb;
        sumlogdelta += std::log(buf[(size_t)c->lay.ca() + i]);
    }
    s.cbq = cbq; s.sumcb = sumcb; s.sumlogdelta = sumlogdelta;
    s.logdet_sb = buf[(size_t)c->lay.scal() + S_LOGDET_SB];
    s.gamma_ = c->gamma_;
    s.hyp = c->hyp;
    s.L = L; s.H = (double)c->H;
}

// trim < 0: lowerBound; trim >= 0: lowerBoundTrimmed
static int sparse_lower_bound_impl(vbmf_ctx* c, int clamp, double trim, double* lb) {
    if (!c || !lb) return VBMF_ERR_INVALID;
    if (!c->sparse) FAIL(c, VBMF_ERR_INVALID, "not a sparse context");
    if (c->diagvar) FAIL(c, VBMF_ERR_UNSUPPORTED, "lowerBound is defined for the homoscedastic model only (src/vbmf_sparse.jl:435)");
    HIPCHK(c, hipSetDevice(c->o.device));
    TRY(ensure_ready(c));
    TRY(ensure_gram_A(c));
    TRY(ensure_gram_B(c));
    int f = 0;
    TRY(prepare_trYBA(c, &f));
    TRY(launch_sparse_ctrl_end(c, f, 0.0, nullptr));       // no updates: stores tr(B'YA) in S_TRYBA
    const int nb = 256;
    hipLaunchKernelGGL(sparse_lb_sums_kernel, dim3(nb), dim3(256), 0, c->stream, c->A32, c->dS32, c->CA32, c->beta32,
                       (long long)c->M, (int)c->H, c->Hp, (int)(c->dual ? c->H0 : c->H), (long long)(c->dual ? c->M0 : c->M), c->ypart, trim);
    HIPCHK(c, hipGetLastError());
    std::vector<double> part((size_t)nb * LB_NS), buf((size_t)c->lay.total());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, memcpy_sync(c, part.data(), c->ypart, part.size() * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, memcpy_sync(c, buf.data(), c->st, buf.size() * 8, hipMemcpyDeviceToHost));
    double s_logbeta_g[3] = {0, 0, 0}, s_ca_g[3] = {0, 0, 0}, s_caq = 0, s_logds = 0, n_keep = 0, s_logbeta_keep = 0, s_ca_keep = 0;
    for (int b = 0; b < nb; ++b) {
        for (int g = 0; g < 3; ++g) { s_logbeta_g[g] += part[LB_NS * b + g]; s_ca_g[g] += part[LB_NS * b + 4 + g]; }
        s_caq += part[LB_NS * b + 3]; s_logds += part[LB_NS * b + 7];
        n_keep += part[LB_NS * b + 8]; s_logbeta_keep += part[LB_NS * b + 9]; s_ca_keep += part[LB_NS * b + 10];
    }
    const bool trimmed = trim >= 0.0;
    if (trimmed && !c->dual) {            // src/vbmf_sparse.jl:482-486: beta and CA are trimmed with ATVecHat (one group)
        s_logbeta_g[0] = s_logbeta_keep; s_logbeta_g[1] = s_logbeta_g[2] = 0.0;
        s_ca_g[0] = s_ca_keep; s_ca_g[1] = s_ca_g[2] = 0.0;
    }
    const double* sc = buf.data() + c->lay.scal();
    LbSums s{};
    lb_basis_sums(c, buf, s);
    const double L = s.L, M = (double)c->M;
    s.M = M;
    s.MH = trimmed ? n_keep : M * s.H;
    s.sig = sc[S_SIGMA2]; s.zeta = sc[S_ZETA]; s.eta = c->eta;
    const double trYY = sc[S_TRYY], trBQ = sc[S_TRYBA];
    auto at = [&](long long off, int i, int j) { return buf[(size_t)off + (size_t)i * c->Hp + j]; };
    double t2 = 0;
    for (int i = 0; i < c->H; ++i)
        for (int j = 0; j < c->H; ++j)
            t2 += (at(c->lay.GA(), i, j) + at(c->lay.SA(), i, j)) * (at(c->lay.GB(), i, j) + L * at(c->lay.SB(), i, j));
    s.quad = trYY - 2 * trBQ + t2;
    s.s_caq = s_caq; s.s_logds = s_logds;
    // grouped models (src/vbmf_dual.jl:556-599, src/vbmf_trial.jl:630-680): posterior shapes and priors per group
    LbGroup grp[3];
    for (int g = 0; g < 3; ++g) grp[g] = LbGroup{0.0, s_logbeta_g[g], s_ca_g[g], c->hyp.alpha0, c->hyp.beta0, c->alpha};
    grp[0].n = s.MH;
    grp[0].s_logbeta = s_logbeta_g[0] + s_logbeta_g[1] + s_logbeta_g[2];
    if (c->dual) {
        const double H1 = (double)(c->H - c->H0);
        grp[0].n = M * (double)c->H0; grp[1].n = (double)c->M0 * H1; grp[2].n = (M - (double)c->M0) * H1;
        for (int g = 0; g < 3; ++g) {
            grp[g].s_logbeta = s_logbeta_g[g];
            grp[g].a_pri = sc[S_GPRI + 2 * g]; grp[g].b_pri = sc[S_GPRI + 2 * g + 1];
            grp[g].a_post = sc[S_GPOST + g];
        }
    }
    s.g = grp; s.ng = 3;
    *lb = lb_assemble(s, clamp);
    return VBMF_OK;
}

extern "C" {

int vbmf_sparse_lower_bound(vbmf_ctx* c, int clamp, double* lb) { return sparse_lower_bound_impl(c, clamp, -1.0, lb); }

int vbmf_sparse_lower_bound_trimmed(vbmf_ctx* c, int clamp, double trim, double* lb) {
    if (c && !(trim >= 0.0)) FAIL(c, VBMF_ERR_INVALID, "vbmf_sparse_lower_bound_trimmed: trim must be >= 0");
    return sparse_lower_bound_impl(c, clamp, trim, lb);
}

}  // extern "C"

#include "host_bags.hpp"
