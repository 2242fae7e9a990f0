/*
 * vbmf_hip.h -- C ABI of the MI355X-native VB matrix-factorization sweep.
 *
 * The reference (vitskvara/VBMatrixFactorization.jl) has no FFI layer: its boundary for this path is
 * the Julia call surface of src/vbmf.jl.  Each entry point below names the reference interface it
 * replaces (file:line relative to the reference root).  A Julia host `ccall`s these (see
 * INTEGRATION.md and vbmatrixfactorization.jl_amd/julia/VBMatrixFactorizationHIP.jl); the tested
 * twin is the Python ctypes host in vbmatrixfactorization.jl_amd/.
 *
 * Conventions
 *   - extern "C", no exceptions cross the boundary.  Every function returns 0 on success or a
 *     negative vbmf_status; vbmf_last_error(ctx) gives the message (Julia `error(...)` analogue).
 *   - All matrices at the boundary are `double`, COLUMN-MAJOR, leading dimension >= rows (Julia
 *     Array{Float64,2} memory as is).  Indices are 0-based (the Julia wrapper subtracts 1 from labels).
 *   - Every pointer is borrowed for the duration of the call; the library copies in/out and never
 *     retains host pointers.  One ctx = one problem (one row-shard of it when nranks > 1) on one GPU;
 *     a ctx is not thread-safe, distinct ctxs are independent.
 *   - There is NO CPU fallback: vbmf_create fails (VBMF_ERR_NO_DEVICE) without a gfx950 device.
 */
#ifndef VBMF_HIP_H
#define VBMF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vbmf_ctx vbmf_ctx;

typedef enum {
    VBMF_OK = 0,
    VBMF_ERR_INVALID = -1,     /* bad argument / shape / state */
    VBMF_ERR_NO_DEVICE = -2,   /* no usable HIP device (no CPU fallback exists) */
    VBMF_ERR_HIP = -3,         /* a HIP runtime call failed */
    VBMF_ERR_NUMERIC = -4,     /* non-positive pivot / non-finite value in the H x H algebra */
    VBMF_ERR_COMM = -5,        /* RCCL failure */
    VBMF_ERR_UNSUPPORTED = -6,
    VBMF_ERR_SYNC = -7         /* an in-launch hand-off gave up: the Y*A pass's register epilogue waited for the SigmaB
                                  table longer than its bounded spin allows (the control workgroup of the same launch
                                  did not run beside it); the state of that sweep is not valid */
} vbmf_status;

/* storage of Y on the device / arithmetic of the two streaming contractions */
#define VBMF_Y_F32 0           /* Y fp32, exact-f32 MFMA (v_mfma_f32_32x32x2_f32) */
#define VBMF_Y_BF16 1          /* Y bf16, v_mfma_f32_32x32x16_bf16, fp32 accumulate */
/* factor operand (BHat in Y'B, AHat in Y*A) fed to the MFMA */
#define VBMF_FACTOR_AUTO 0     /* f32 with f32 Y; bf16x2 with bf16 Y */
#define VBMF_FACTOR_BF16 1     /* one bf16 rounding of the factor: ~3 significant digits in A/B, sigma2 only loosely (a speed
                                  option, not a parity mode); vbmf_create returns VBMF_ERR_UNSUPPORTED for H > VBMF_FACTOR_BF16_MAX_H */
#define VBMF_FACTOR_BF16_MAX_H 128
#define VBMF_FACTOR_BF16X2 2   /* hi+lo bf16 split (two MFMAs), ~16 mantissa bits */

#define VBMF_VARIANT_BASIC 0        /* src/vbmf.jl */
#define VBMF_VARIANT_SPARSE_DIAG 1  /* src/vbmf_sparse.jl, full_cov=false, diag_var=false */
#define VBMF_VARIANT_SPARSE_DIAGVAR 2 /* src/vbmf_sparse.jl, full_cov=false, diag_var=true: one noise precision per row */
#define VBMF_VARIANT_DUAL_DIAG 3    /* src/vbmf_dual.jl, full_cov=false, diag_var=false: two column groups A = [A0 A1] */
#define VBMF_VARIANT_TRIAL_DIAG 4   /* src/vbmf_trial.jl, full_cov=false, diag_var=false: three groups A = [A1 [A2; A3]] */
#define VBMF_VARIANT_DUAL_DIAGVAR 5  /* src/vbmf_dual.jl, full_cov=false, diag_var=true (rows' noise as in VBMF_VARIANT_SPARSE_DIAGVAR) */
#define VBMF_VARIANT_TRIAL_DIAGVAR 6 /* src/vbmf_trial.jl, full_cov=false, diag_var=true */

/* reference_compat bits (default: all set = behave like the reference) */
#define VBMF_COMPAT_SPECTRAL_DELTA 1u  /* d uses operator 2-norms (src/util.jl:27-29, Julia 0.5 norm) */
#define VBMF_COMPAT_SPARSE_REPEAT 2u   /* repeat(v, inner=M-1) layout of src/vbmf_sparse.jl:221 */
#define VBMF_COMPAT_DEFAULT 0xFFFFFFFFu

typedef struct {
    int32_t struct_size;       /* = sizeof(vbmf_opts); for ABI evolution */
    int32_t device;            /* HIP device ordinal */
    int32_t y_dtype;           /* VBMF_Y_* */
    int32_t factor_dtype;      /* VBMF_FACTOR_* */
    int32_t variant;           /* VBMF_VARIANT_* */
    uint32_t reference_compat; /* VBMF_COMPAT_* bitmask */
    int32_t nranks;            /* row-shards of Y (one process per GPU); 1 = single GPU */
    int32_t rank;
    int64_t L_global;          /* total rows over all ranks (0 => = L) */
    int64_t row_offset;        /* first global row owned by this ctx */
    int32_t pass1_splits;      /* split-K factor of the Y'B pass; 0 = auto */
    int32_t reserved;
} vbmf_opts;

/* update selectors for vbmf_step -- one bit per reference update function */
#define VBMF_STEP_A 1       /* updateA!      src/vbmf.jl:95-102 */
#define VBMF_STEP_B 2       /* updateB!      src/vbmf.jl:109-113 */
#define VBMF_STEP_CA 4      /* updateCA!     src/vbmf.jl:129-134 */
#define VBMF_STEP_CB 8      /* updateCB!     src/vbmf.jl:141-146 */
#define VBMF_STEP_SIGMA2 16 /* updateSigma2! src/vbmf.jl:153-157 */

void vbmf_default_opts(vbmf_opts* o);

/* One problem of L (local) x M with rank H.  Replaces the allocation half of vbmf_init
 * (src/vbmf.jl:48-73); the random draw stays on the host side. */
int vbmf_create(vbmf_ctx** out, int64_t L, int64_t M, int64_t H, const vbmf_opts* opts);
int vbmf_destroy(vbmf_ctx* ctx);
const char* vbmf_last_error(const vbmf_ctx* ctx); /* ctx may be NULL: error of a failed create */

/* Upload this rank's rows of Y (L x M, column-major, ld >= L): converts to the device dtype, builds
 * the two MFMA-fragment-tiled copies and caches ||Y||_F^2 (of the values as stored).  Replaces the
 * `Y::Array{Float64,2}` argument of vbmf!/updateA!/updateB!/updateSigma2! (src/vbmf.jl:95,109,153,175). */
int vbmf_set_Y(vbmf_ctx* ctx, const double* Y, int64_t ldY);
/* The same Y from the caller's own number format, layout and memory, whole or in row blocks: no fp64 copy is made anywhere.  The
 * reference has Float32 methods on this path (scaleY, preprocess: src/util.jl:60,94).
 *   src: element (l, m) of the block, l in 0..nrows-1, m in 0..M-1, is src[l*row_stride + m*col_stride]; strides count elements of
 *     src_dtype (VBMF_SRC_*).  Rows are this rank's local rows, as for vbmf_get_Y.  Every value is converted ONCE to the context's
 *     storage type, round-to-nearest-even through fp64, as vbmf_set_Y does: the same values give the same stored bits, pad tiles included.
 *   Blocks come in ascending, contiguous order: row0 equals the number of rows supplied so far and is a multiple of 32; nrows is a
 *     multiple of 32 unless row0 + nrows = L.  The block with row0 = 0 starts a new Y: from then on the context has no Y (every entry
 *     that needs one fails as on a fresh context), ||Y||^2 starts from zero and G, W of the Gram form are invalid.  The block that
 *     reaches L completes Y (the per-row norms of the *_DIAGVAR variants included).  row0 = 0, nrows = L is the whole matrix at once.
 *   src_on_device != 0: src is device memory on the context's device; any positive strides (views, slices, transposes).  The caller
 *     guarantees that the buffer is complete and stays valid until the call returns; the entry runs on the context's stream and
 *     returns after that stream is idle.
 *   src_on_device == 0: src is host memory with row_stride = 1 or col_stride = 1 (and the other stride no shorter than a line).  It is
 *     staged through a device buffer of its OWN dtype in chunks of at most 256 MB.
 * VBMF_ERR_INVALID, before any launch or copy and with the context -- its current Y included -- untouched, for: NULL src; an unknown
 * dtype; a non-positive stride; a host source with neither stride 1 (or with overlapping lines); a row0 / nrows that is misaligned,
 * out of order or past L; a pointer whose kind contradicts src_on_device or that lives on another device (hipPointerGetAttributes); a
 * device source whose extent [src, src + ((nrows-1)*row_stride + (M-1)*col_stride + 1) elements) does not lie inside one allocation
 * (hipMemGetAddressRange).  A wrong pointer comes back as an error code; no kernel reads it. */
#define VBMF_SRC_F64 0
#define VBMF_SRC_F32 1
#define VBMF_SRC_BF16 2
int vbmf_set_Y_rows(vbmf_ctx* ctx, const void* src, int32_t src_dtype, int32_t src_on_device,
                    int64_t row0, int64_t nrows, int64_t row_stride, int64_t col_stride);
/* Y of dst := columns col_index[0..ncols) of the Y stored in src, in that order: the device-side get_matrices
 * (examples/mil_util.jl:46-58), which the reference's drivers call with the bag ids of every fold (validate_with_cvs :627,
 * validate_dataset :670) on one resident data set.  src is a context that holds the whole data set; dst is a context of ncols columns.
 *   dst is left exactly as vbmf_set_Y(dst, Ysrc_as_stored[:, col_index]) leaves it: both tiled copies, pad tiles included, bit for bit
 *     (the stored values are on the storage grid already, so the one rounding cannot move them); ||Y||^2 of the stored values, summed
 *     over the same partials in the same order; the per-row norms of the *_DIAGVAR variants; and the same "new Y" event, so G, W, P, Q
 *     and everything else derived from the old Y are dropped.  A row-block upload in progress on dst is abandoned.
 *   col_index is host memory; duplicates are allowed and ncols may exceed src's M.  src is only read.
 *   src's stream is synchronised first; the kernels run on dst's stream and the entry returns after that stream is idle.
 * VBMF_ERR_INVALID, before any launch, copy or change and with dst -- its current Y included -- untouched: NULL dst, src or col_index;
 * dst == src; ncols != dst's M; a different local L; a different y_dtype; a different device; src without a complete Y (fresh, or in
 * the middle of a row-block upload); an index outside 0 .. src's M - 1 (the whole table is checked on the host: no kernel sees a bad
 * index).  VBMF_ERR_UNSUPPORTED: either context with nranks > 1 or a communicator. */
int vbmf_set_Y_gather(vbmf_ctx* dst, vbmf_ctx* src, const int64_t* col_index, int64_t ncols);
/* Device-side generator of the toy model (examples/toy_data.jl:7-18): Y = B* A*' + noise_std*N(0,1),
 * A* one-hot rows over Hstar columns, values rounded to the device dtype; counter-based, so the
 * matrix does not depend on nranks. */
int vbmf_set_Y_synthetic(vbmf_ctx* ctx, uint64_t seed, int64_t Hstar, double noise_std);
/* Read back Y exactly as stored on the device (rows [row0,row0+nrows) of this rank, column-major). */
int vbmf_get_Y(vbmf_ctx* ctx, double* Y, int64_t ldY, int64_t row0, int64_t nrows);
int vbmf_get_trYY(vbmf_ctx* ctx, double* trYY);

/* State = the numeric fields of `vbmf_parameters` (src/vbmf.jl:22-40).  AHat is M x H (ldA >= M),
 * BHat is L x H (this rank's rows, ldB >= L), SigmaA/SigmaB are H x H (ld = H), CA/CB are passed as
 * their diagonals (length H; the reference keeps them diagonal by construction, src/vbmf.jl:65-66,131,143).
 * labels0: 0-based rows of AHat whose last H1 columns are forced to zero (src/vbmf.jl:61,101). */
int vbmf_set_state(vbmf_ctx* ctx, const double* AHat, int64_t ldA, const double* BHat, int64_t ldB,
                   const double* SigmaA, const double* SigmaB, const double* CA_diag, const double* CB_diag,
                   double sigma2, const int64_t* labels0, int64_t nlabels, int64_t H1);
int vbmf_get_state(vbmf_ctx* ctx, double* AHat, int64_t ldA, double* BHat, int64_t ldB, double* SigmaA,
                   double* SigmaB, double* CA_diag, double* CB_diag, double* sigma2);

/* Apply the selected reference updates once, in the reference's order A, B, CA, CB, SIGMA2
 * (src/vbmf.jl:194-204).  For callers that drive the updates themselves (examples/mil_util.jl:183-185). */
int vbmf_step(vbmf_ctx* ctx, int which);

/* Fixed-basis inference, the reference's main caller of the update functions outside vbmf! -- vbls!
 * (examples/mil_util.jl:179-203, vbmf_parameters branch): niter x (updateA!, updateCA!, updateSigma2!) with BHat,
 * SigmaB, CB frozen.  B is fixed, so Y'B is formed once: ONE pass over Y per call instead of two per iteration. */
int vbmf_run_fixed_basis(vbmf_ctx* ctx, int64_t niter);

/* vbls! over many bags with one fixed basis (examples/mil_util.jl:473-479 in one call).  The context's Y is the bags side by
 * side: bag b = columns col_off[b] .. col_off[b+1]-1 (col_off[0] = 0, col_off[nbags] = M, every bag >= 1 column).
 * BHat, SigmaB, CB from vbmf_set_state; no label mask; H <= 64; one rank; niter >= 1.
 * In/out per bag: sigma2[nbags], CA_diag[nbags*H] (start values in, final values out).  Out: SigmaA[nbags*H*H],
 * AHat (M x H, ldA >= M).  The context's state is not changed.  SigmaA or AHat may be NULL (not formed / not copied).
 * Any other input returns VBMF_ERR_INVALID before a launch; a non-finite pivot in any bag VBMF_ERR_NUMERIC. */
int vbmf_run_fixed_basis_batched(vbmf_ctx* ctx, int64_t nbags, const int64_t* col_off, int64_t niter,
                                 double* sigma2, double* CA_diag, double* SigmaA, double* AHat, int64_t ldA);

/* vbmf_fit_batched: many independent vbmf! fits of the basic model (A and B both move) in ONE launch, one workgroup per fit with the
 * whole `while i <= niter && d > eps` loop of src/vbmf.jl:175-231 inside it -- the two basic-model fits of examples/mil_util.jl:110-114
 * and the folds x p x repetitions around them in one call.  The context is VBMF_VARIANT_BASIC and supplies only Y, bags side by side
 * (bag b = columns col_off[b] .. col_off[b+1]-1); its own state is neither read nor changed (none needs to be set).  Fit f works on bag
 * fit_bag[f], so several fits may share a bag.  One rank, no label mask, H <= 32; a 1-column bag is valid.
 *   est_covs / est_var: updateCA! + updateCB! / updateSigma2! after every sweep's updateA!, updateB!, as vbmf! takes them
 *   in/out, per-fit blocks in fit order: BHat (L*H, column-major), SigmaB (H*H), CA, CB (H: the diagonals), sigma2 (1)
 *   out (either may be NULL): AHat (M_b*H column-major per fit, concatenated by each fit's own M_b), SigmaA (H*H)
 *   iters_done, d_last, status (nfits): the sweeps run, the last d, and 1 for a fit that met a non-finite sigma2, a CA_h or CB_h that
 *       is not positive and finite, or a pivot that is not positive and finite in either inverse, and left its loop after that sweep
 *       (0 otherwise).  Such fits do not fail the call.  trace (nfits*niter*2, may be NULL): (d, sigma2) per sweep run, zeros after.
 * d = norm(B - B_old) / norm(B_old) with operator 2-norms under VBMF_COMPAT_SPECTRAL_DELTA (src/util.jl:27-29), Frobenius norms
 * otherwise; the loop ends when !(d > eps), so a NaN d ends it as the reference's comparison does.  Everything is fp64 on Y as stored.
 * VBMF_ERR_UNSUPPORTED: H > 32.  VBMF_ERR_INVALID, all before any launch: a non-basic context, a label mask, nranks > 1, a bad
 * col_off, a fit_bag entry outside 0..nbags-1, nfits < 1, niter < 1, a required pointer NULL, no Y. */
int vbmf_fit_batched(vbmf_ctx* ctx, int64_t nbags, const int64_t* col_off, int64_t nfits, const int64_t* fit_bag,
                     int64_t niter, double eps, int est_covs, int est_var,
                     double* BHat, double* SigmaB, double* CA, double* CB, double* sigma2,
                     double* AHat, double* SigmaA,
                     int64_t* iters_done, double* d_last, int64_t* status, double* trace);

/* vbmf_fit_batched_form: vbmf_fit_batched with a choice of how a fit's sweep takes what it needs from Y.  updateA! of the basic model
 * is A = Y'B SigmaA / sigma2 with no mask (src/vbmf.jl:95-98), so after any sweep A = Y'V with V = B SigmaA / sigma2 (L x H), and
 * updateB!, updateCA! and updateSigma2! (src/vbmf.jl:95-157) need only K = Y Y' (L x L): Y A = K V, A'A = V'K V,
 * tr(B'Y A) = sum B o (K V), ||Y||^2 = tr K.  The same iteration, 2 L^2 H flops per sweep instead of 4 L M_b H: the form for WIDE bags.
 * K is built once per bag (fits that share a bag share it), A is formed once after the loop.
 *   form = VBMF_FIT_FORM_STREAM (0)  every fit streams Y_b twice per sweep: every output is bit-identical to vbmf_fit_batched
 *   form = VBMF_FIT_FORM_GRAM (1)    every fit iterates on K.  Its state is 3 L H doubles of LDS behind a fixed part F; when
 *        3 L H > VBMF_FIT_LDS_CAP_BYTES / 8 - F the call returns VBMF_ERR_UNSUPPORTED before any launch.
 *        F = P (P + 2) + 9 H^2 with P = 16 for H <= 16 and P = 32 for H <= 32
 *   form = VBMF_FIT_FORM_AUTO (2)    per fit: the Gram form when M_b >= VBMF_FIT_GRAM_WIDE_FACTOR * L and its state fits, else the
 *        streaming form -- a function of (L, M_b, H) alone, so a fit's numbers depend neither on its place in the call nor on the
 *        other fits in it
 * Any other form returns VBMF_ERR_INVALID before a launch.  form_used (nfits, may be NULL): 0 / 1 per fit, the form it ran in.
 * Both forms run the reference's updates in the reference's order in fp64 on Y as stored; they differ by rounding only. */
#define VBMF_FIT_FORM_STREAM 0
#define VBMF_FIT_FORM_GRAM 1
#define VBMF_FIT_FORM_AUTO 2
#define VBMF_FIT_GRAM_WIDE_FACTOR 2
#define VBMF_FIT_LDS_CAP_BYTES 147456
int vbmf_fit_batched_form(vbmf_ctx* ctx, int64_t nbags, const int64_t* col_off, int64_t nfits, const int64_t* fit_bag,
                          int64_t niter, double eps, int est_covs, int est_var,
                          double* BHat, double* SigmaB, double* CA, double* CB, double* sigma2,
                          double* AHat, double* SigmaA,
                          int64_t* iters_done, double* d_last, int64_t* status, double* trace,
                          int64_t form, int64_t* form_used);

/* K_b = Y_b Y_b' of every bag in fp64 on Y as stored (bags side by side as in vbmf_fit_batched; any variant, no state needed):
 * K holds nbags blocks of L x L doubles, each symmetric bit for bit and a function of (L, M_b) and the bag's data alone.  What
 * vbmf_fit_batched_form iterates on; callers of ols / rls (examples/mil_util.jl:159-171) form B'K_b B from it.
 * VBMF_ERR_INVALID before any launch: nranks > 1, a bad col_off, K NULL, no Y. */
int vbmf_bags_row_gram(vbmf_ctx* ctx, int64_t nbags, const int64_t* col_off, double* K);

/* The vbmf! loop (src/vbmf.jl:187-214): while i <= niter && d > eps { A; B; [CA; CB]; [sigma2]; d }.
 * Runs entirely on the device; the stop test is evaluated device-side so the state freezes exactly
 * where the reference would stop.  iters_done = i-1 (src/vbmf.jl:221), d_last = last d.
 * trace (optional, niter x 4 doubles, row-major): per sweep d, sigma2, elbo, reserved.
 * eps: the reference's default 1e-6 (src/vbmf.jl:175) is at or below what d resolves on the device (BHat is stored in fp32 /
 * as bf16 hi + lo: d floors at ~1e-6 / ~1e-5 where the fp64 reference keeps falling).  A run that uses all niter sweeps with d
 * still above such an eps returns VBMF_OK and leaves a text starting with "note:" in vbmf_last_error (cleared by the next run);
 * the Python / Julia hosts turn it into a warning.
 * Row-sharded runs: a device error on one rank (VBMF_ERR_NUMERIC / VBMF_ERR_SYNC) stops every rank at the same sweep and every
 * rank returns that error class -- the ranks' error flags travel with the packed Gram all-reduce. */
int vbmf_run(vbmf_ctx* ctx, int64_t niter, double eps, int est_covs, int est_var, int64_t* iters_done,
             double* d_last, double* trace);

/* updateYHat! (src/vbmf.jl:120-122) on demand: YHat = BHat*AHat' (L x M column-major). */
int vbmf_get_YHat(vbmf_ctx* ctx, double* YHat, int64_t ld);
/* updateYHat! (src/vbmf.jl:120-122) into memory the caller names -- the mirror of vbmf_set_Y_rows: host or device, the caller's dtype
 * and strides, whole or in row blocks; no fp64 copy and no host round trip is made for a device dst.
 *   what: VBMF_OUT_YHAT = BHat*AHat'; VBMF_OUT_RESIDUAL = Y as stored (what vbmf_get_Y returns) - BHat*AHat'.
 *   dst: element (l, j) of the block, l in 0..nrows-1 (this rank's local rows row0 + l), j in 0..M-1, is dst[l*row_stride + j*col_stride];
 *     strides count elements of dst_dtype (VBMF_DST_*).  Any row range inside L; no alignment is asked for.
 *   Arithmetic, fixed per dst dtype and per entry -- an entry depends on row l of BHat and row j of AHat (the fp32 values vbmf_get_state
 *     returns) and on Y[l, j] alone, never on row0, nrows, the strides or where dst lives:
 *       VBMF_DST_F64   fp64 products and sums (v_mfma_f64_16x16x4_f64), as accurate as vbmf_get_YHat
 *       VBMF_DST_F32   an fp32 fma chain in the order h = 0, 1, ... of exact fp32 products (v_mfma_f32_32x32x2_f32)
 *       VBMF_DST_BF16  the round-to-nearest-even of the VBMF_DST_F32 value, bit for bit
 *     and the residual is fl(y - s) in the accumulation type.
 *   dst_on_device != 0: device memory on the context's device, any positive strides whose lines do not overlap.
 *   dst_on_device == 0: host memory with row_stride = 1 or col_stride = 1; staged through a device buffer of the dst's OWN dtype in
 *     chunks of at most 256 MB.
 *   The entry runs on the context's stream and returns after that stream is idle.  After a Gram-form run the first call pays the owed
 *   BHat once, as vbmf_get_state does; nothing else of the context's state or caches changes.
 * VBMF_ERR_INVALID, in this order and before any launch, copy or materialisation of BHat, with the context and dst untouched: NULL dst;
 * an unknown what or dtype; a non-positive stride; nrows < 1 or a row range outside 0..L; lines that overlap (neither row_stride >=
 * (M-1)*col_stride + 1 nor col_stride >= (nrows-1)*row_stride + 1); a host dst with neither stride 1; a pointer whose kind contradicts
 * dst_on_device or that lives on another device (hipPointerGetAttributes); a device extent [dst, dst + ((nrows-1)*row_stride +
 * (M-1)*col_stride + 1) elements) that does not lie inside one allocation (hipMemGetAddressRange); then no state, and for
 * VBMF_OUT_RESIDUAL no Y.  A wrong pointer comes back as an error code; no kernel writes it. */
#define VBMF_DST_F64 0   /* same codes as VBMF_SRC_* */
#define VBMF_DST_F32 1
#define VBMF_DST_BF16 2
#define VBMF_OUT_YHAT 0      /* BHat*AHat' */
#define VBMF_OUT_RESIDUAL 1  /* Y as stored (what vbmf_get_Y returns) - BHat*AHat' */
int vbmf_get_YHat_rows(vbmf_ctx* ctx, int32_t what, void* dst, int32_t dst_dtype, int32_t dst_on_device,
                       int64_t row0, int64_t nrows, int64_t row_stride, int64_t col_stride);
/* The factors of updateYHat! (src/vbmf.jl:120-122) the same way: rows row0 .. row0+nrows-1 of AHat (M x H; ATVecHat as a matrix for
 * the sparse family) or of this rank's BHat (L x H), element (x, h) at dst[x*row_stride + h*col_stride].  The values are exactly the
 * fp32 ones vbmf_get_state / vbmf_sparse_get_state return: VBMF_DST_F32 is a copy, VBMF_DST_F64 a widening, VBMF_DST_BF16 one
 * round-to-nearest-even.  dst, the validation (with H columns in place of M) and the owed BHat as for vbmf_get_YHat_rows. */
#define VBMF_FACTOR_A 0      /* M x H */
#define VBMF_FACTOR_B 1      /* this rank's L x H */
int vbmf_get_factor_rows(vbmf_ctx* ctx, int32_t which, void* dst, int32_t dst_dtype, int32_t dst_on_device,
                         int64_t row0, int64_t nrows, int64_t row_stride, int64_t col_stride);
/* Build-defined ELBO of the basic model (the reference has none). */
int vbmf_elbo(vbmf_ctx* ctx, double* elbo);

/* ---- ARD-sparse variant: src/vbmf_sparse.jl with full_cov=false, diag_var=false (opts.variant =
 * VBMF_VARIANT_SPARSE_DIAG).  vec(A') is element-wise: index m*H + h (src/vbmf_sparse.jl:119,244-246).
 * Shapes: ATVecHat, diagSigmaATVec, CA, beta: M*H; BHat: L x H column-major; SigmaB: H x H; CB, delta: H.
 * sigmaHat is the noise PRECISION with Gamma posterior (eta, zeta) (src/vbmf_sparse.jl:35-39,321).
 * Derived constants (src/vbmf_sparse.jl:131,137,143): alpha = alpha0 + 1/2, gamma = gamma0 + L/2,
 * eta = eta0 + L*M/2 (L = L_global).  diag_var=true: VBMF_VARIANT_*_DIAGVAR + vbmf_sparse_set_noise_rows below;
 * full_cov=true: vbmf_sparse_set_full_cov below (per-column H x H blocks; the dense MH x MH fields are never formed). */
typedef struct { double alpha0, beta0, gamma0, delta0, eta0, zeta0; } vbmf_sparse_hyper;

#define VBMF_SSTEP_A 1      /* updateA! diagonal branch  src/vbmf_sparse.jl:204-247 */
#define VBMF_SSTEP_B 2      /* updateB!                  src/vbmf_sparse.jl:263-266 */
#define VBMF_SSTEP_CA 4     /* updateCA!                 src/vbmf_sparse.jl:284-288 */
#define VBMF_SSTEP_CB 8     /* updateCB!                 src/vbmf_sparse.jl:295-300 */
#define VBMF_SSTEP_SIGMA 16 /* updateSigma! homoscedastic src/vbmf_sparse.jl:317-321 */
#define VBMF_SSTEP_PRIORS 32 /* grouped models only, together with VBMF_SSTEP_CA: updateAlpha0g!, updateBeta0g!  src/vbmf_dual.jl:393-434, src/vbmf_trial.jl:442-507 */

int vbmf_sparse_set_state(vbmf_ctx* ctx, const double* ATVecHat, const double* diagSigmaATVec, const double* CA,
                          const double* beta, const double* BHat, int64_t ldB, const double* SigmaB,
                          const double* CB, const double* delta, double sigmaHat, double zeta,
                          const vbmf_sparse_hyper* hyper, const int64_t* labels0, int64_t nlabels, int64_t H1);
/* any output pointer may be NULL; SigmaA_diag: the diagonal of SigmaA (H), src/vbmf_sparse.jl:236-239 */
int vbmf_sparse_get_state(vbmf_ctx* ctx, double* ATVecHat, double* diagSigmaATVec, double* CA, double* beta,
                          double* SigmaA_diag, double* BHat, int64_t ldB, double* SigmaB, double* CB,
                          double* delta, double* sigmaHat, double* zeta);
/* Heteroscedastic rows (VBMF_VARIANT_SPARSE_DIAGVAR; src/vbmf_sparse.jl:207-212,229-230,256-261,308-315): the same
 * vbmf_sparse_* entry points then run the diag_var=true updates; the row-noise state travels separately:
 * sigmaVecHat, zetaVec (length L) and the common Gamma shape etaVec = eta0 + M/2 (:145-147).  set: after
 * vbmf_sparse_set_state (whose sigmaHat/zeta are ignored); get_state's sigmaHat is mean(sigmaVecHat). */
int vbmf_sparse_set_noise_rows(vbmf_ctx* ctx, const double* sigmaVecHat, const double* zetaVec, double etaVec);
int vbmf_sparse_get_noise_rows(vbmf_ctx* ctx, double* sigmaVecHat, double* zetaVec);
/* vbls! on the sparse model (examples/mil_util.jl:187-190): niter x (updateA!, updateCA!, updateSigma!), B frozen */
int vbmf_sparse_run_fixed_basis(vbmf_ctx* ctx, int64_t niter);
/* vbls! on the sparse models over many bags with one fixed basis (examples/mil_util.jl:187-197 in one call), the diagonal or
 * (full_cov != 0) the full_cov form of updateA!.  Context: VBMF_VARIANT_SPARSE_DIAG, _DUAL_DIAG or _TRIAL_DIAG whose Y is the bags side
 * by side (col_off as in vbmf_run_fixed_basis_batched); BHat, SigmaB from vbmf_sparse_set_state; no label mask; H <= 64; one rank;
 * niter >= 1.  Per bag: alpha[nbags*H], beta0[nbags*H] (updateCA!'s alpha_h and beta0_h: the three families differ only there),
 * eta[nbags] (eta0 + L*M_b/2), zeta0[nbags].  In/out: sigmaHat[nbags], CA[M*H] in vec(A') order (start values in, final values out).
 * Out: zeta[nbags], beta[M*H], diagSigmaATVec[M*H], SigmaA[nbags*H*H], ATVecHat[M*H]; each may be NULL (not copied).  The QS1 layout
 * (VBMF_COMPAT_SPARSE_REPEAT) follows each bag's own M_b; a 1-column bag is valid.  The context's state is not changed.  Any other
 * input returns VBMF_ERR_INVALID before a launch; a non-positive or non-finite pivot, or a non-finite precision, in any bag
 * VBMF_ERR_NUMERIC. */
int vbmf_sparse_run_fixed_basis_batched(vbmf_ctx* ctx, int64_t nbags, const int64_t* col_off, int64_t niter, int full_cov,
                                        const double* alpha, const double* beta0, const double* eta, const double* zeta0,
                                        double* sigmaHat, double* CA, double* zeta, double* beta, double* diagSigmaATVec,
                                        double* SigmaA, double* ATVecHat);
/* vbmf_sparse_fit_batched: many independent vbmf_sparse! / vbmf_dual! fits (B moves too) in ONE launch, one workgroup per fit with the
 * whole `while i <= niter && d > eps` loop inside it -- the restart loops of examples/mil_util.jl:124-145,347-379 and the folds x
 * classes around them (:670-788) in one call.  The context supplies only Y, bags side by side (bag b = columns col_off[b] ..
 * col_off[b+1]-1); its own state is neither read nor changed (none needs to be set).  Fit f works on bag fit_bag[f], so several fits
 * (restarts) may share a bag.  A sparse-model or two-group context (`*_DIAG` variants), one rank, no label mask, H <= 32.  This entry is
 * the homoscedastic noise model; the same fits with one noise precision per row of Y (diag_var): vbmf_rows_fit_batched.
 *   per fit (nfits): gamma, delta0, eta, zeta0 -- the derived shapes gamma0 + L/2, eta0 + L M_b/2 and the prior rates
 *   priors4 (nfits*4, in/out): alpha00, beta00, alpha01, beta01 -- columns h < H0 of A take the first pair, the others the second
 *       (src/vbmf_dual.jl:322-351); the sparse model passes its pair twice with H0 = H.  est_priors != 0 refits them every sweep
 *       (:393-434) and returns the fitted values
 *   in/out, per-fit blocks in fit order: BHat (L*H, column-major), SigmaB (H*H), CB (H), sigmaHat (1), CA (M_b*H, vec(A') order,
 *       concatenated by each fit's own M_b)
 *   out (any may be NULL): delta (H; written only when est_cb), zeta (1), beta, diagSigmaATVec, ATVecHat (M_b*H), SigmaA (H*H:
 *       diagonal in the diagonal form, the sum of the per-column blocks under full_cov)
 *   iters_done, d_last, status (nfits): the sweeps run, the last d, and 1 for a fit that met a non-finite precision or a pivot that is
 *       not positive and left its loop after that sweep (0 otherwise).  Such fits do not fail the call: the restart loops expect them
 *       (:130-132).  trace (nfits*niter*2, may be NULL): (d, sigmaHat) per sweep run, zeros after.
 * d = norm(B_old - B) / norm(B_old) with operator 2-norms under VBMF_COMPAT_SPECTRAL_DELTA (src/util.jl:27-29), Frobenius norms
 * otherwise; the loop ends when !(d > eps), so a NaN d ends it as the reference's comparison does.  Everything is fp64 on Y as stored.
 * VBMF_ERR_UNSUPPORTED: H > 32.  VBMF_ERR_INVALID, all before any launch: a `*_DIAGVAR`, basic or trial context, a label mask,
 * nranks > 1, a bad col_off, a fit_bag entry outside 0..nbags-1, nfits < 1, niter < 1, H0 outside 1..H, a required pointer NULL, a
 * 1-column bag in the diagonal form under VBMF_COMPAT_SPARSE_REPEAT (repeat(v, inner = M-1) needs M >= 2). */
int vbmf_sparse_fit_batched(vbmf_ctx* ctx, int64_t nbags, const int64_t* col_off, int64_t nfits, const int64_t* fit_bag,
                            int64_t niter, double eps, int full_cov, int est_cb, int est_priors, int64_t H0,
                            const double* gamma, const double* delta0, const double* eta, const double* zeta0,
                            double* priors4, double* BHat, double* SigmaB, double* CB, double* sigmaHat, double* CA,
                            double* delta, double* zeta, double* beta, double* diagSigmaATVec, double* SigmaA, double* ATVecHat,
                            int64_t* iters_done, double* d_last, int64_t* status, double* trace);
/* vbmf_local_fit_batched: many independent fits on concatenated matrices [Y0 Y1] whose first M0 columns are the negative instances, in
 * ONE launch -- the three-group model (vbmf_trial!, src/vbmf_trial.jl:528-604) and the label-masked sparse model (train_local,
 * examples/mil_util.jl:302-320: vbmf_sparse! with labels = 1:M0 and H1).  Everything is as in vbmf_sparse_fit_batched (shapes, in/out
 * rules, status, trace, d under either compat bit, the QS1 layout by each fit's own M_b, the 1-column refusal in the diagonal form)
 * except:
 *   M0 (nfits): the fit's leading columns of its bag, 0 <= M0[f] <= M_b
 *   H0: entry (m, h) of A belongs to prior group 1 if h < H0, to group 2 if h >= H0 and m < M0[f], to group 3 otherwise
 *       (src/vbmf_trial.jl:357-400); 0 <= H0 <= H.  est_priors != 0 refits the three pairs every sweep (:442-507); an empty group keeps
 *       its pair
 *   mask_H1 > 0: once updateA! has produced a(m, h), the entries with m < M0[f], h >= H - mask_H1 become exactly 0 before updateCA!,
 *       A'A and Y*A read them; diagSigmaATVec and SigmaA are not masked (src/vbmf_sparse.jl:236-246), so beta = beta0 + ds/2 there.
 *       Needs H0 = H and est_priors = 0: the masked model has one prior group (slots 0, 1 of priors9) and no hyper-prior fit
 *   priors9 (nfits*9), laid out as vbmf_trial_get_priors lays it out: slots 0-5 alpha01, beta01, alpha02, beta02, alpha03, beta03 are
 *       in/out; slots 6-8 are out: the posterior shapes alpha1, alpha2, alpha3 the last updateCA! used
 * The context is any `*_DIAG` sparse, two-group or three-group context; its state is neither read nor changed.  Homoscedastic noise;
 * with one noise precision per row of Y (diag_var): vbmf_rows_fit_batched.
 * VBMF_ERR_UNSUPPORTED: H > 32.  VBMF_ERR_INVALID, all before any launch, copy or change: a basic or `*_DIAGVAR` context, a label mask
 * set on the context, nranks > 1, no Y, a bad col_off, a fit_bag entry outside 0..nbags-1, nfits < 1, niter < 1, a required pointer
 * NULL, H0 outside 0..H, an M0[f] outside 0..M_b, mask_H1 outside 0..H, mask_H1 > 0 together with H0 != H or est_priors != 0, a 1-column
 * bag in the diagonal form under VBMF_COMPAT_SPARSE_REPEAT. */
int vbmf_local_fit_batched(vbmf_ctx* ctx, int64_t nbags, const int64_t* col_off, int64_t nfits, const int64_t* fit_bag,
                           int64_t niter, double eps, int full_cov, int est_cb, int est_priors,
                           int64_t H0, const int64_t* M0, int64_t mask_H1,
                           const double* gamma, const double* delta0, const double* eta, const double* zeta0,
                           double* priors9, double* BHat, double* SigmaB, double* CB, double* sigmaHat, double* CA,
                           double* delta, double* zeta, double* beta, double* diagSigmaATVec, double* SigmaA, double* ATVecHat,
                           int64_t* iters_done, double* d_last, int64_t* status, double* trace);
/* vbmf_rows_fit_batched: the fits of vbmf_sparse_fit_batched and vbmf_local_fit_batched under the heteroscedastic noise model,
 * diag_var = true -- one noise precision per row of Y, what examples/mil_util.jl:667 sets for train, train_local and train_dual (:129,
 * :140, :314, :351, :376).  src/vbmf_sparse.jl (src/vbmf_dual.jl:222-299,370-386 and src/vbmf_trial.jl:256-334,419-435 are the same),
 * with s = sigmaVecHat, G = A'A + SigmaA, Q = Y A:
 *   updateA!, diagonal form (:207-230): v_h = sum_l (s_l B_lh)^2 + L mean(s) SigmaB_hh -- s enters SQUARED here, the reference takes
 *       norm2 of the product diag(s) B, and this library keeps that; prec = spread(v) + CA, ds = 1/prec, a = ds (B' diag(s) Y), with
 *       NO factor sigmaHat
 *   updateA!, full_cov (:180-193): K_m = B' diag(s) B + L mean(s) SigmaB + diag(CA[m,:]) -- s to the first power; a_m = inv(K_m)
 *       (B' diag(s) y_m), SigmaA = sum_m inv(K_m)
 *   updateB! (:256-261): SigmaB = inv(diag(CB) + mean(s) G), B = diag(s) Q SigmaB
 *   updateSigma! (:309-315): zetaVec_l = zeta0 + ||Y[l,:]||^2 / 2 - sum_h Q_lh B_lh + (b_l'G b_l + sum G o SigmaB) / 2,
 *       s_l = etaVec / zetaVec_l; sigmaHat and zeta are not touched
 * updateCA!, updateCB!, the prior groups, the prefix mask, est_priors, d and the stop test are those of vbmf_local_fit_batched, whose
 * shapes, in/out rules, priors9 layout, status and trace hold here except:
 *   M0 may be NULL: M0[f] = M_b, which makes the three-group rule the two-group model (with H0 = H and est_priors = 0: the sparse one)
 *   etaVec (nfits): eta0 + M_b / 2
 *   sigmaVec (nfits*L, in/out) and zetaVec (nfits*L, out, may be NULL) stand where sigmaHat and zeta stand
 *   trace: (d, mean(sigmaVec)) per sweep run; status 1 also for a zetaVec_l or s_l that is not finite
 * The context supplies only Y: any sparse-family context serves, `*_DIAG` or `*_DIAGVAR`; its state is neither read nor changed.
 * Refusals: those of vbmf_local_fit_batched with the same codes, all before any launch, copy or change (a `*_DIAGVAR` context and a
 * NULL M0 are accepted). */
int vbmf_rows_fit_batched(vbmf_ctx* ctx, int64_t nbags, const int64_t* col_off, int64_t nfits, const int64_t* fit_bag,
                          int64_t niter, double eps, int full_cov, int est_cb, int est_priors,
                          int64_t H0, const int64_t* M0, int64_t mask_H1,
                          const double* gamma, const double* delta0, const double* etaVec, const double* zeta0,
                          double* priors9, double* BHat, double* SigmaB, double* CB, double* sigmaVec, double* CA,
                          double* delta, double* zetaVec, double* beta, double* diagSigmaATVec, double* SigmaA, double* ATVecHat,
                          int64_t* iters_done, double* d_last, int64_t* status, double* trace);
/* vbmf_ard_fit_batched_form: the fits of vbmf_local_fit_batched (diag_var = 0) and of vbmf_rows_fit_batched (diag_var != 0) with the
 * form chosen by the caller.  The argument list is vbmf_rows_fit_batched's.  diag_var = 0: etaVec, sigmaVec and zetaVec are the per-fit
 * scalars eta, sigmaHat and zeta of vbmf_local_fit_batched, a `*_DIAG` context is required, and M0 may be NULL (M0[f] = M_b).
 *   form = VBMF_FIT_FORM_STREAM (0)  one workgroup per fit, the whole loop in one launch: every output is bit-identical to
 *        vbmf_local_fit_batched / vbmf_rows_fit_batched for the same arguments
 *   form = VBMF_FIT_FORM_SPLIT (3)   every fit is spread over ceil(M_b / slice_cols) workgroups.  A fit's columns are cut into slices of
 *        slice_cols columns counted from its own first column (the last may be short); a sweep is two launches, a column pass with one
 *        workgroup per (fit, slice) -- updateA!, updateCA! and the slice's shares of A'A, SigmaA, Q = Y A and the prior sums -- and a
 *        fold with one workgroup per fit that sums the shares in slice order and does the rest of the sweep.  No workgroup waits for
 *        another and nothing is an atomic: a fit's numbers are a function of (L, M_b, H, H0, M0, slice_cols) and its own inputs, not of
 *        its place in the call.  They differ from form 0's in rounding only (another summation order).  The host enqueues
 *        VBMF_FIT_SPLIT_CHUNK sweeps at a time and reads the fits' done words in between; a stopped fit's workgroups return at once.
 *        iters_done, d_last, status and trace mean what they mean in form 0.
 *   form = VBMF_FIT_FORM_AUTO (2)    per fit: split when M_b >= VBMF_FIT_SPLIT_MIN_COLS (full_cov: VBMF_FIT_SPLIT_MIN_COLS_FULL), else
 *        the one-workgroup loop; the two groups run one after the other
 *   form = VBMF_FIT_FORM_GRAM (1)    VBMF_ERR_UNSUPPORTED: these models have no Gram form.  Any other form: VBMF_ERR_INVALID.
 * slice_cols: 0 = VBMF_FIT_SPLIT_COLS (narrowed to the widest multiple of 8 whose state, 3 slice_cols H doubles, fits in LDS beside
 * full_cov's images); otherwise a multiple of 8, at least 8 (else VBMF_ERR_INVALID); one too wide for LDS returns VBMF_ERR_UNSUPPORTED.
 * form_used (nfits, may be NULL): 0 / 3 per fit.  Refusals: those of vbmf_local_fit_batched / vbmf_rows_fit_batched with their codes,
 * then form and slice_cols, all before any launch, copy or change.
 * The constants are measured ones (MI355X, L = 166, H = 5, 50 sweeps, profiles/fit_split_tune.txt, fit_split_widths.txt; DESIGN.md
 * section 19).  VBMF_FIT_SPLIT_COLS: of 64 / 128 / 256 / 512 the fastest on 20 diagonal fits at 166 x 3000; 20 full_cov fits at
 * 166 x 640 prefer 64 by 15 %, and the two cases together tie at 64 and 128.  VBMF_FIT_SPLIT_MIN_COLS (diagonal form) and
 * VBMF_FIT_SPLIT_MIN_COLS_FULL: the split form beat the one-workgroup loop by more than the spread at every width tested, 160 the
 * narrowest; narrower bags were not measured and stay with the loop.  VBMF_FIT_SPLIT_CHUNK: 4, 8, 16 and 50 sweeps between two reads
 * of the done words came out within the spread of each other; 8 bounds the empty launches behind the last stop at sixteen.
 * Tuning switch, like the library's other VBMF_* environment variables: VBMF_FIT_SPLIT_CHUNK = 1 .. 65536 in the environment replaces
 * the chunk length for the calls of that process (scripts/fit_split_mil.py measures with it).  It changes how often the host looks,
 * never a number a fit computes.  In a mixed form = 2 call the caller's arrays are written only after both groups have run. */
#define VBMF_FIT_FORM_SPLIT 3
#define VBMF_FIT_SPLIT_COLS 128
#define VBMF_FIT_SPLIT_MIN_COLS 160
#define VBMF_FIT_SPLIT_MIN_COLS_FULL 160
#define VBMF_FIT_SPLIT_CHUNK 8
int vbmf_ard_fit_batched_form(vbmf_ctx* ctx, int64_t nbags, const int64_t* col_off, int64_t nfits, const int64_t* fit_bag,
                              int64_t niter, double eps, int full_cov, int est_cb, int est_priors,
                              int64_t H0, const int64_t* M0, int64_t mask_H1,
                              const double* gamma, const double* delta0, const double* etaVec, const double* zeta0,
                              double* priors9, double* BHat, double* SigmaB, double* CB, double* sigmaVec, double* CA,
                              double* delta, double* zetaVec, double* beta, double* diagSigmaATVec, double* SigmaA, double* ATVecHat,
                              int64_t* iters_done, double* d_last, int64_t* status, double* trace,
                              int diag_var, int64_t form, int64_t slice_cols, int64_t* form_used);
int vbmf_sparse_step(vbmf_ctx* ctx, int which);           /* reference order A, B, CA, CB, SIGMA (:369-376) */
/* vbmf_sparse! loop (src/vbmf_sparse.jl:344-410): returns d like the reference; trace: niter x 4 (d, sigmaHat, 0, 0)
 * Gram form.  A VBMF_VARIANT_SPARSE_DIAG context with full_cov off, one rank, bf16 Y, bf16x2 factors and
 * H <= 128 iterates on G = Y'Y instead of streaming Y twice per sweep under the size rule of vbmf_run (L >= 4 M and L M >= 2^27), or
 * at any size when it was created under VBMF_GRAM=2 (VBMF_GRAM=1 forces the basic model only; VBMF_GRAM=0 and every other sparse
 * context -- the grouped models, diag_var, full_cov, H > 128, row shards, fp32 storage -- keep the streaming sweep).  128 < H <= 256
 * takes the form only under vbmf_set_gram_form(ctx, VBMF_GRAM_FORM_ON) or VBMF_GRAM=3.  In that form B = Y W with W = sigmaHat A SigmaB: the first sweep
 * of a run that holds no W streams Y and forms W, the later ones read G only, and W is carried from run to run.  Before the run returns,
 * BHat of the last executed sweep is formed by one streaming pass, so vbmf_sparse_get_state, the lower bounds and a following run see
 * what a streaming run leaves, and run(3) + run(3) computes what run(6) computes.  vbmf_sparse_set_state, vbmf_set_Y*,
 * vbmf_sparse_step, vbmf_sparse_run_fixed_basis, vbmf_sparse_set_full_cov, vbmf_set_gram_form and a failed run drop W: the next run
 * starts by streaming. */
int vbmf_sparse_run(vbmf_ctx* ctx, int64_t niter, double eps, int est_cb, int64_t* iters_done, double* d_last,
                    double* trace);
/* lowerBound (src/vbmf_sparse.jl:435-471), verbatim quirks QS4; H(B) as L*logdet(SigmaB), clamped like
 * normalEntropy's det (src/util.jl:118-122) when clamp != 0 */
int vbmf_sparse_lower_bound(vbmf_ctx* ctx, int clamp, double* lb);
/* lowerBoundTrimmed (src/vbmf_sparse.jl:478-489; dual src/vbmf_dual.jl:606-617; trial src/vbmf_trial.jl:687-698; called by
 * examples/mil_util.jl:505): the bound with the entries of vec(A') whose |ATVecHat| <= trim removed from ATVecHat, beta, CA,
 * diagSigmaATVec and MH -- a mask in front of the M*H-long sums (AHat itself, and with it Y*AHat and AHat'AHat, stays
 * whole, as in the reference, which trims the vec fields only; the grouped models' per-group fields beta0/beta1/CA0/...
 * are not trimmed there either, so for them only MH, the CA-weighted second moment and H(vec(A')) change).
 * The comparison runs on the device's fp32 copy of ATVecHat. */
int vbmf_sparse_lower_bound_trimmed(vbmf_ctx* ctx, int clamp, double trim, double* lb);

/* ---- per-bag scoring: what the MIL classifier compares after a batched vbls! (examples/mil_util.jl:469-530) ----
 * The context's Y is the bags side by side (col_off as in vbmf_run_fixed_basis_batched).  All entries refuse, with VBMF_ERR_INVALID
 * and before any launch: col_off not running from 0 to M or not increasing (an empty bag), a *_DIAGVAR context, nranks > 1, a NULL
 * required pointer.  A non-finite sum in a bag returns VBMF_ERR_NUMERIC and vbmf_last_error names the bag.  The context's state is
 * not changed by any of them.
 *
 * vbmf_bag_residuals: r2[b] = ||Y_b - BHat*AHat_b'||_F^2, the square of norm(Y - BHat*AHat') of examples/mil_util.jl:476-479 (and of
 * norm(YHat - Y), :518-521), for every bag.  Formed entry by entry in fp64 from Y as stored (what vbmf_get_Y returns), the context's
 * BHat as stored (vbmf_set_state / vbmf_sparse_set_state keep it in fp32: the values vbmf_get_state returns) and the caller's fp64
 * AHat (M x H column-major, ldA >= M) -- never from the trace form ||Y||^2 - 2 tr(B'YA) + tr(A'A B'B), whose cancellation costs the
 * digits the comparison between two models needs.  Basic and sparse-family contexts, any H up to 1024. */
int vbmf_bag_residuals(vbmf_ctx* ctx, int64_t nbags, const int64_t* col_off, const double* AHat, int64_t ldA, double* r2);
/* vbmf_bag_least_squares: ols / rls of examples/mil_util.jl:159-171 and the norm(Y - BHat*AT) of :483-484 for every bag of the
 * context's Y -- what classify's "ols" and "rls" branches compute per bag (examples/mil_util.jl:457-468).  The context supplies only Y;
 * the basis is the argument BHat (L x H fp64 column-major, ldB >= L), used in fp64 as given: H is the call's own (1 <= H <= 64,
 * independent of the H the context was created with, so models of different rank share one upload), the context's state is neither read
 * nor changed (none needs to be set), and any context kind works as for vbmf_bag_residuals.
 *   X   (H x M column-major, ldX >= H, may be NULL): columns col_off[b] .. col_off[b+1]-1 = inv(BHat'BHat + lambda I) BHat' Y_b, the
 *       reference's ols(Y_b, BHat) for lambda == 0 and rls(Y_b, BHat, lambda) for lambda > 0
 *   r2  (nbags, may be NULL; not both): r2[b] = ||Y_b - BHat X_b||_F^2
 * All fp64 from Y as stored (what vbmf_get_Y returns).  K = inv(BHat'BHat + lambda I) is formed once per call on the device by the
 * control chain's blocked inverse; per column z = BHat'y, x = K z, and the residual entry by entry as y - BHat x -- never
 * ||y||^2 - z'Kz, which cancels 400- to 3000-fold on fitted bags.  Every sum has a fixed order and no bag's numbers depend on where
 * it sits in Y or on the other bags of the call.
 * Refused before any launch: H < 1 or H > 64 (VBMF_ERR_UNSUPPORTED); with VBMF_ERR_INVALID what the block above lists, lambda < 0 or
 * not finite, a non-finite entry of BHat, ldB < L, ldX < H, NULL BHat, X and r2 both NULL.  A pivot of BHat'BHat + lambda I that is
 * not positive or not finite (a rank-deficient basis at lambda == 0: the case rls exists for, :463-464) returns VBMF_ERR_NUMERIC and
 * leaves X and r2 unwritten. */
int vbmf_bag_least_squares(vbmf_ctx* ctx, int64_t nbags, const int64_t* col_off, const double* BHat, int64_t ldB, int64_t H, double lambda,
                           double* X, int64_t ldX, double* r2);
/* vbmf_bag_least_squares_jobs: test_classification (examples/mil_util.jl:558-587) of every fold of validate_with_cvs
 * (examples/mil_util.jl:627-648) in one call -- many bases and a list of (bag, basis) jobs on the one context that holds every bag of the
 * data set (col_off as in vbmf_bag_least_squares).
 *   Hs, BHat, lambda   basis k is L x Hs[k] fp64 column-major with leading dimension L, 1 <= Hs[k] <= 64; the bases are packed one after
 *                      the other in BHat; lambda[k] is that basis' own value (0 = ols, > 0 = rls)
 *   job_bag, job_basis job j scores bag job_bag[j] against basis job_basis[j].  Jobs may come in any order, a bag may appear in many
 *                      jobs, a basis in many or none, and a job may repeat
 *   X       (may be NULL) per-job blocks in job order, Hs[k] x M_b column-major with ld = Hs[k]: inv(B_k'B_k + lambda_k I) B_k' Y_b
 *   r2      (njobs, may be NULL; not both) r2[j] = ||Y_b - B_k X_j||_F^2, formed entry by entry
 *   status  (nbasis, required) 1 for a basis whose B'B + lambda I met a pivot that is not positive or not finite, else 0
 * Job j's X block and r2[j] are bit for bit what vbmf_bag_least_squares returns for that bag with that basis and lambda, whatever
 * else is in the call and wherever the job, the bag or the basis sits: both entries run the same device functions.  Four launches
 * (Gram partials per (basis, row chunk); one inverse per basis; one workgroup per (job, 8-column slice of its bag); the fold of the
 * slices per job) and one synchronising read-back, whatever nbasis and njobs are.
 * A bad basis (status 1) does not fail the call, as in the *_fit_batched entries: its jobs get NaN in r2 and in every entry of their X
 * block (written on the device), the other jobs are computed as if it were not in the call.  A non-finite r2 of a job whose basis has
 * status 0 returns VBMF_ERR_NUMERIC and vbmf_last_error names the job; X, r2 and status HAVE been written by then (they come back
 * with the one read-back that the scan follows), unlike vbmf_bag_least_squares, which leaves its outputs unwritten on a numeric
 * failure.  Every refusal leaves X, r2 and status untouched.  The context's state, caches and Y are not changed; only Y is read.
 * Refused before any launch, copy or change: VBMF_ERR_UNSUPPORTED for an Hs[k] outside 1..64 or more job slices than one grid holds
 * -- a launch is kept to 2^32 - 1 threads, which is 16 777 215 workgroups of 256: that many 8-column job slices in all (so at most
 * that many jobs), and that many (basis, 256-row chunk) pairs; nbasis and njobs have no other cap -- or a call whose bases and job
 * tables the host cannot stage in memory;
 * VBMF_ERR_INVALID for everything vbmf_bag_least_squares refuses, nbasis < 1, njobs < 1, a NULL Hs, BHat, lambda, job_bag, job_basis
 * or status, X and r2 both NULL, a lambda[k] that is negative or not finite, a non-finite entry of any basis, a job_bag[j] outside
 * 0..nbags-1, a job_basis[j] outside 0..nbasis-1, no Y. */
int vbmf_bag_least_squares_jobs(vbmf_ctx* ctx, int64_t nbags, const int64_t* col_off, int64_t nbasis, const int64_t* Hs, const double* BHat,
                                const double* lambda, int64_t njobs, const int64_t* job_bag, const int64_t* job_basis, double* X,
                                double* r2, int64_t* status);
/* vbmf_sparse_fixed_basis_jobs: vbls! of the ARD families (examples/mil_util.jl:187-197) for a list of (bag, model) jobs and each job's
 * norm(Y - BHat*AHat')^2 -- the "dual" classifier of examples/mil_util.jl:515-530 (20 vbls! iterations with full_cov = true against each
 * of a fold's two models) for every fold of validate_with_cvs in one call, on the one context that holds every bag of the data set
 * (col_off as in vbmf_bag_least_squares).  Any context variant serves, with one rank and no label mask: only its Y is read, and the
 * call's H has nothing to do with the context's own.
 *   H, niter, full_cov  1 <= H <= 32 for every model of the call (the whole-fit entries' cap), niter >= 1 iterations of updateA! with
 *                       updateCA! behind it and updateSigma!, the diagonal (0) or the full_cov (1) form of updateA!; homoscedastic noise
 *   per model k < nmodels, packed in model order:
 *   BHat, SigmaB        L x H fp64 column-major with ld = L, used in fp64 as given; H x H
 *   alpha, beta0        (H each) updateCA!'s posterior shape and prior rate per column of A: the three families differ only there
 *   eta0, zeta0         the noise precision's Gamma prior; the device forms eta = eta0 + L M_b / 2 per job
 *   sigma0, ca0         every job of the model starts from sigmaHat = sigma0[k] and CA = ca0[k] ones (what copy_vbmf_params gives)
 *   job_bag, job_model  job j runs bag job_bag[j] against model job_model[j].  Jobs may come in any order, a bag may appear in many
 *                       jobs, a model in many or none, and a job may repeat
 *   r2                  (njobs, may be NULL) ||Y_b - BHat_k AHat_j'||_F^2, formed entry by entry in fp64, never by the trace form
 *   ATVecHat, diagSigmaATVec, CA, beta   (each may be NULL; r2 and ATVecHat not both) per-job blocks in job order, each M_b H long in
 *                       vec(A') order as in vbmf_sparse_run_fixed_basis_batched
 *   SigmaA (njobs H H), sigmaHat, zeta (njobs)   may be NULL
 *   status              (njobs, required) 1 for a job that met a non-finite precision or a pivot that is not positive and finite (or ended
 *                       with a non-finite sigmaHat, zeta or r2), else 0
 * Everything is fp64, Y widened on load from Y as stored.  Every sum has an order fixed by (L, M_b, H) alone, so a job's numbers do not
 * depend on the other jobs, on their order, or on where the bag sits in Y.  Two launches (one workgroup per model: G = B'B + L SigmaB;
 * one workgroup per job: Y_b'B_k, the iterations, the residual) and one synchronising read-back, whatever nmodels and njobs are.
 * A failed job (status 1) does not fail the call, as in the *_fit_batched entries: it gets NaN in r2 and in every entry of its blocks
 * (written on the device), the other jobs are computed as if it were not in the call.  The context's state, caches and Y are not
 * changed.  Under VBMF_COMPAT_SPARSE_REPEAT the diagonal form carries the QS1 layout with the job's own M_b.
 * Refused before any launch, copy or change, every output left untouched: VBMF_ERR_UNSUPPORTED for H outside 1..32, more jobs or models
 * than the 16 777 215 workgroups one grid holds, or a call whose models and results the host cannot stage in memory;
 * VBMF_ERR_INVALID for everything bags_check refuses (a sharded context, nbags < 1, a col_off that does not run from 0 to M or that
 * decreases), nmodels < 1, njobs < 1, niter < 1, a NULL input or status, r2 and ATVecHat both NULL, a non-finite entry of any BHat,
 * SigmaB, alpha, beta0, eta0, zeta0, sigma0 or ca0, a job_bag[j] outside 0..nbags-1, a job_model[j] outside 0..nmodels-1, a label
 * mask, no Y, and a 1-column bag in the diagonal form under VBMF_COMPAT_SPARSE_REPEAT (as vbmf_sparse_fit_batched). */
int vbmf_sparse_fixed_basis_jobs(vbmf_ctx* ctx, int64_t nbags, const int64_t* col_off, int64_t H, int64_t niter, int full_cov,
                                 int64_t nmodels, const double* BHat, const double* SigmaB, const double* alpha, const double* beta0,
                                 const double* eta0, const double* zeta0, const double* sigma0, const double* ca0, int64_t njobs,
                                 const int64_t* job_bag, const int64_t* job_model, double* r2, double* ATVecHat, double* diagSigmaATVec,
                                 double* CA, double* beta, double* SigmaA, double* sigmaHat, double* zeta, int64_t* status);
/* vbmf_sparse_scored_jobs: factorize_bag (examples/mil_util.jl:393-416) and the scores behind it -- lowerBound of the fit against the
 * basis without its last H1 columns, lowerBoundTrimmed(threshold) of the fit against the whole basis (:502-514), and the two residual
 * norms (:493-501) -- for a list of (bag, model) jobs in one call: the "lower_bound" and "min_err" classifiers of every fold of
 * validate_with_cvs (:627-648) at once.  It is vbmf_sparse_fixed_basis_jobs (same context, same kernels, same numbers: for a job with the
 * same bag, model and form every block and r2 are that entry's bit for bit) with a rank per model, a form and a trim per job, and the
 * bound of every job.
 *   niter, clamp, grouped   niter >= 1 iterations; clamp and grouped as in vbmf_sparse_lower_bound_batched
 *   per model k < nmodels, packed in model order (model k's blocks behind those of the models before it):
 *   model_H             the model's own rank, 1 <= H_k <= 32
 *   BHat, SigmaB        L x H_k fp64 column-major with ld = L; H_k x H_k
 *   CB, delta           (H_k each) the precisions of B's columns and their Gamma posterior rates
 *   gamma, gamma0, delta0   their posterior shape and prior (one each)
 *   a_pri, b_pri, a_post    (H_k each) per column of A the ARD hyper-prior (shape, rate) and the posterior shape, the layout of
 *                       vbmf_sparse_lower_bound_batched; a_post and b_pri are what updateCA! reads (vbmf_sparse_fixed_basis_jobs' alpha, beta0)
 *   eta0, zeta0, sigma0, ca0   as in vbmf_sparse_fixed_basis_jobs
 *   per job j < njobs:
 *   job_bag, job_model  as in vbmf_sparse_fixed_basis_jobs
 *   job_full_cov        0: the diagonal form of updateA!, 1: full_cov
 *   job_trim            < 0: lowerBound; >= 0: lowerBoundTrimmed(job_trim[j]).  The mask |ATVecHat| > trim compares the fp64 ATVecHat, as
 *                       the reference does (src/vbmf_sparse.jl:481)
 *   lb, r2              (njobs each, may be NULL; lb, r2 and ATVecHat not all three) the bound and ||Y_b - BHat_k AHat_j'||_F^2.  The
 *                       bound's data term is r2 + L tr(A'A SigmaB) + tr(SigmaA (B'B + L SigmaB)) with that direct residual, never the
 *                       trace form
 *   ATVecHat, diagSigmaATVec, CA, beta, SigmaA, sigmaHat, zeta   as in vbmf_sparse_fixed_basis_jobs (SigmaA: the jobs' H_k x H_k blocks one
 *                       after the other), in the caller's job order
 *   status              (njobs, required) 1 for a job the device flagged (as in vbmf_sparse_fixed_basis_jobs) or whose bound or sums are not
 *                       finite: NaN in lb, r2 and every block of that job; the other jobs are computed as if it were not in the call
 * One launch of the model kernel (which also leaves the basis' share of the bound: sum CB_h (B'B + L SigmaB)_hh, sum CB, sum log delta and
 * log det SigmaB from an in-LDS Cholesky), one launch of the job kernel per non-empty (16-block tier of H_k, form) group of jobs -- at
 * most four; the host sorts the jobs into them through an index table -- and one synchronising read-back.  The host assembles lb.
 * Refused before any launch, copy or change, every output left untouched: what vbmf_sparse_fixed_basis_jobs refuses (a 1-column bag only
 * for a job whose own form is the diagonal one under VBMF_COMPAT_SPARSE_REPEAT), a model_H[k] outside 1..32 (VBMF_ERR_UNSUPPORTED), a
 * job_full_cov[j] other than 0 or 1, and a non-finite CB, delta, gamma, gamma0, delta0, a_pri or job_trim. */
int vbmf_sparse_scored_jobs(vbmf_ctx* ctx, int64_t nbags, const int64_t* col_off, int64_t niter, int clamp, int grouped, int64_t nmodels,
                            const int64_t* model_H, const double* BHat, const double* SigmaB, const double* CB, const double* delta,
                            const double* gamma, const double* gamma0, const double* delta0, const double* a_pri, const double* b_pri,
                            const double* a_post, const double* eta0, const double* zeta0, const double* sigma0, const double* ca0,
                            int64_t njobs, const int64_t* job_bag, const int64_t* job_model, const int64_t* job_full_cov,
                            const double* job_trim, double* lb, double* r2, double* ATVecHat, double* diagSigmaATVec, double* CA,
                            double* beta, double* SigmaA, double* sigmaHat, double* zeta, int64_t* status);
/* test hook: the widest bag whose job keeps its state in LDS in vbmf_sparse_fixed_basis_jobs at this H and form (wider ones work in the
 * call's scratch buffer); 0 for an H outside 1..32 */
int vbmf_debug_vbls_jobs_lds_cols(int64_t H, int full_cov);
/* vbmf_fixed_basis_jobs: vbls! of the basic model (examples/mil_util.jl:182-185: niter x (updateA!, updateCA!, updateSigma2!) with B, SigmaB
 * frozen) for a list of (bag, model) jobs and each job's norm(Y - BHat*AHat')^2 -- the "vbls" classifier of examples/mil_util.jl:469-479
 * (150 vbls! iterations against each of a fold's two models) for every fold of validate_with_cvs in one call, on the one context that
 * holds every bag of the data set (col_off as in vbmf_bag_least_squares).  Any context variant serves, with one rank and no label mask:
 * only its Y is read, and the models' ranks have nothing to do with the context's own.
 *   niter               >= 1 iterations
 *   per model k < nmodels, packed in model order (model k's blocks behind those of the models before it):
 *   model_H             the model's own rank, 1 <= H_k <= 32 (vbmf_fit_batched's cap, which produces these models)
 *   BHat, SigmaB        L x H_k fp64 column-major with ld = L, used in fp64 as given; H_k x H_k.  CB is not an argument: updateA!
 *                       (src/vbmf.jl:95-98) never reads it
 *   sigma2_0, ca0       every job of the model starts from sigma2 = sigma2_0[k] and CA = ca0[k] I (copy_vbmf_params: the trained
 *                       sigma2 and 1.0)
 *   job_bag, job_model  job j runs bag job_bag[j] against model job_model[j].  Jobs may come in any order, a bag may appear in many
 *                       jobs, a model in many or none, and a job may repeat
 *   r2                  (njobs, may be NULL) ||Y_b - BHat_k AHat_j'||_F^2, formed entry by entry in fp64, never by the trace form
 *   AHat                (may be NULL; r2 and AHat not both) per-job M_b x H_k blocks, column-major, one after the other in job order, as
 *                       vbmf_fit_batched lays them out
 *   SigmaA, CA_diag, sigma2   (each may be NULL) the jobs' H_k x H_k blocks, H_k-long blocks, one value per job
 *   status              (njobs, required) 1 for a job that met a pivot that is not positive and finite (or ended with a non-finite
 *                       sigma2, CA or r2), else 0
 * Per job, with S = P'P, P = Y_b'BHat_k and G_k = BHat_k'BHat_k + L SigmaB_k (vbmf_run_fixed_basis' H x H form of the loop):
 *   K = G_k + sigma2 inv(CA);  SigmaA = sigma2 inv(K);  A'A = SigmaA S SigmaA / sigma2^2;  CA_hh = (A'A)_hh / M_b + SigmaA_hh;
 *   sigma2 = (||Y_b||^2 - 2 tr(S SigmaA) / sigma2 + tr((A'A + M_b SigmaA) G_k)) / (L M_b);  AHat = P SigmaA / sigma2 once, from the last
 *   updateA!.
 * Everything is fp64, Y widened on load from Y as stored.  Every sum has an order fixed by (L, M_b, H_k) alone, so a job's numbers do
 * not depend on the other jobs, on their order or tier, or on where the bag sits in Y.  One launch of the model kernel (one workgroup
 * per model: G_k), one launch of the job kernel per non-empty 16-block tier of H_k -- at most two; the host sorts the jobs into them
 * through an index table -- and one synchronising read-back, whatever nmodels and njobs are.
 * A failed job (status 1) does not fail the call, as in the *_fit_batched entries: it gets NaN in r2, sigma2 and every entry of its
 * blocks (written on the device), the other jobs are computed as if it were not in the call.  The context's state, caches and Y are
 * not changed.
 * Refused before any launch, copy or change, every output left untouched: VBMF_ERR_UNSUPPORTED for a model_H[k] outside 1..32, more
 * jobs or models than the 16 777 215 workgroups one grid holds, or a call whose models and results the host cannot stage in memory;
 * VBMF_ERR_INVALID for everything bags_check refuses (a sharded context, nbags < 1, a col_off that does not run from 0 to M or that
 * decreases), nmodels < 1, njobs < 1, niter < 1, a NULL input or status, r2 and AHat both NULL, a non-finite entry of any BHat, SigmaB,
 * sigma2_0 or ca0, a job_bag[j] outside 0..nbags-1, a job_model[j] outside 0..nmodels-1, a label mask, no Y. */
int vbmf_fixed_basis_jobs(vbmf_ctx* ctx, int64_t nbags, const int64_t* col_off, int64_t niter, int64_t nmodels, const int64_t* model_H,
                          const double* BHat, const double* SigmaB, const double* sigma2_0, const double* ca0, int64_t njobs,
                          const int64_t* job_bag, const int64_t* job_model, double* r2, double* AHat, double* SigmaA, double* CA_diag,
                          double* sigma2, int64_t* status);
/* test hook: the widest bag whose job keeps its P in LDS in vbmf_fixed_basis_jobs at this H (wider ones work in the call's scratch
 * buffer); 0 for an H outside 1..32 */
int vbmf_debug_fixed_basis_jobs_lds_cols(int64_t H);
/* lowerBound (src/vbmf_sparse.jl:435-471; dual src/vbmf_dual.jl:556-599; trial src/vbmf_trial.jl:630-680) for trim < 0 and
 * lowerBoundTrimmed (src/vbmf_sparse.jl:478-489; dual :606-617; trial :687-698) for trim >= 0 of every bag, as called per bag by
 * examples/mil_util.jl:502-514.  Sparse-family context, homoscedastic, one fixed basis: BHat, SigmaB, CB, delta and the hyper-priors
 * gamma0, delta0 (with gamma = gamma0 + L/2) from vbmf_sparse_set_state.  Per bag, laid out as vbmf_sparse_run_fixed_basis_batched
 * leaves them: ATVecHat, diagSigmaATVec, CA, beta (M*H, vec(A') order), SigmaA (nbags*H*H), sigmaHat, zeta (nbags); eta, eta0, zeta0
 * (nbags: the noise precision's Gamma posterior shape and prior); a_pri, b_pri, a_post (nbags*H): the Gamma hyper-prior (shape, rate)
 * and the posterior shape of the ARD precisions of column h of A -- one pair for the sparse model, per column group for the dual and
 * trial models (a trial set with M0 = M_b, what copy_vbmf_params gives: its third group is empty).
 * grouped = 0: the sparse model's lowerBoundTrimmed, which trims beta and CA with ATVecHat (src/vbmf_sparse.jl:482-486); != 0: the
 * grouped models', whose per-group fields stay whole (see vbmf_sparse_lower_bound_trimmed).  The mask |ATVecHat| > trim runs on the
 * fp32 rounding of ATVecHat, like that entry's.  clamp as in vbmf_sparse_lower_bound.
 * Data term: r2 + L tr(A'A SigmaB) + tr(SigmaA (B'B + L SigmaB)) with r2 the direct residual of vbmf_bag_residuals formed in the same
 * call -- algebraically the reference's ||Y||^2 - 2 tr(B'YA) + tr((A'A + SigmaA)(B'B + L SigmaB)) (:439-440) without its cancellation.
 * Out: lb[nbags]; r2[nbags] (may be NULL). */
int vbmf_sparse_lower_bound_batched(vbmf_ctx* ctx, int64_t nbags, const int64_t* col_off, int clamp, double trim, int grouped,
                                    const double* ATVecHat, const double* diagSigmaATVec, const double* CA, const double* beta,
                                    const double* SigmaA, const double* sigmaHat, const double* zeta, const double* eta,
                                    const double* eta0, const double* zeta0, const double* a_pri, const double* b_pri,
                                    const double* a_post, double* lb, double* r2);
/* full_cov = true of updateA! (src/vbmf_sparse.jl:178-202; dual :218-243; trial :252-277).  The reference's dense MH x MH
 * invSigmaATVec = sigmaHat*kron(I_M, B'B + L*SigmaB) + diag(CA) is block diagonal, so the device inverts the M H x H blocks
 * (one workgroup per column of Y) and never forms it: diagSigmaATVec = the blocks' diagonals, SigmaA = their sum (a full
 * H x H matrix).  Applies to VBMF_SSTEP_A, the run loops and run_fixed_basis from then on.  Up to H = 128 the H x H fp64 block of
 * a column lives in one workgroup's registers (two columns per round up to H = 64, one above); 128 < H <= 256 goes through a
 * blocked Schur inverse in a per-workgroup global workspace (~0.4 ms per column: for small M).  Either noise model: in the
 * *_DIAGVAR variants (:180-182, :192-193) the blocks are B' diag(sigmaVec) B + L mean(sigmaVec) SigmaB + diag(CA[m,:]) and the
 * mean carries no sigmaHat factor.  The dense SigmaATVec / invSigmaATVec fields are not materialised. */
int vbmf_sparse_set_full_cov(vbmf_ctx* ctx, int on);
/* Which form the run loops take (vbmf_run, and vbmf_sparse_run for src/vbmf_sparse.jl:344-412):
 *   VBMF_GRAM_FORM_DEFAULT  the rule a context has from its creation: VBMF_GRAM as read then (0 never; 1 the basic model whenever
 *                           its structure allows; 2 the ARD-sparse model too; 3 = VBMF_GRAM_FORM_ON; any other value parses as 1),
 *                           else the size rule (L >= 4 M and L M >= 2^27).  Neither the size rule nor VBMF_GRAM = 0 / 1 / 2 ever
 *                           takes the form at H > 128.
 *   VBMF_GRAM_FORM_OFF      every sweep streams Y.
 *   VBMF_GRAM_FORM_ON       the Gram form wherever the structure allows it: one rank, bf16 Y, bf16x2 factors, no full_cov / diag_var /
 *                           grouped model, H <= 128 -- and for VBMF_VARIANT_SPARSE_DIAG also 128 < H <= 256 (stored as Hp = 256), which
 *                           no other setting turns on.  The basic model at H > 128 keeps streaming.
 * The call drops W, so the next run starts by a streaming sweep.  It does not fail for a structure that cannot take the form:
 * word 16 of VBMF_PEEK_DIMS reports what was resolved.  Any other mode returns VBMF_ERR_INVALID and changes nothing. */
#define VBMF_GRAM_FORM_DEFAULT 0
#define VBMF_GRAM_FORM_OFF 1
#define VBMF_GRAM_FORM_ON 2
int vbmf_set_gram_form(vbmf_ctx* ctx, int mode);
/* SigmaA as a full H x H matrix, column-major (vbmf_sparse_set_state derives a diagonal one from diagSigmaATVec; set it
 * explicitly to continue a full_cov state) */
int vbmf_sparse_set_SigmaA(vbmf_ctx* ctx, const double* SigmaA);
int vbmf_sparse_get_SigmaA(vbmf_ctx* ctx, double* SigmaA);

/* ---- Two-group ARD variant (opts.variant = VBMF_VARIANT_DUAL_DIAG, or VBMF_VARIANT_DUAL_DIAGVAR for diag_var = true with the
 * rows' noise state of vbmf_sparse_set_noise_rows; src/vbmf_dual.jl, diagonal branch) -----------------
 * vbmf_dual_parameters (src/vbmf_dual.jl:59-112): A = [A0 A1], H = H0 + H1; the element-wise precisions of columns
 * h < H0 have the Gamma hyper-prior (alpha00, beta00), those of the other columns (alpha01, beta01); posterior shapes are
 * alpha0g + 1/2 (:324-325).  updateA!/updateB!/updateCB!/updateSigma! are the sparse model's bodies (no label mask), so the
 * state travels through vbmf_sparse_set_state / vbmf_sparse_get_state (CA and beta as the interleaved vectors of :146-165,
 * hyper.alpha0/beta0 = the initial value of both groups' priors), and vbmf_sparse_step, vbmf_sparse_run_fixed_basis
 * (vbls!, examples/mil_util.jl:190-193) and vbmf_sparse_lower_bound (lowerBound, src/vbmf_dual.jl:556-599) apply.
 * set_priors: after vbmf_sparse_set_state; alpha0 / alpha1 are the posterior shapes the fields of those names hold (what
 * the last updateCA! set; lowerBound reads them, :564-565).  get_priors: priors6 = {alpha00, beta00, alpha01, beta01, alpha0, alpha1}. */
int vbmf_dual_set_priors(vbmf_ctx* ctx, int64_t H0, double alpha00, double beta00, double alpha01, double beta01,
                         double alpha0, double alpha1);
int vbmf_dual_get_priors(vbmf_ctx* ctx, int64_t* H0, double* priors6);
/* vbmf_dual! loop (src/vbmf_dual.jl:455-530; convergence on BHat).  est_priors != 0 re-fits the four hyper-priors every
 * sweep (:491-495) on the device: alpha0g = the root of the reference's fAlpha0g on its bracket [1e-10, 1e10] (the
 * reference calls Roots.jl's fzero, a dependency it neither vendors nor pins: PARITY UNPINNED; unchanged when the bracket
 * holds no sign change, like the reference's `try ... end`), beta0g = M*Hg*alpha0g / sum(CAg).  trace as vbmf_sparse_run. */
int vbmf_dual_run(vbmf_ctx* ctx, int64_t niter, double eps, int est_cb, int est_priors, int64_t* iters_done,
                  double* d_last, double* trace);

/* ---- Three-group ARD variant (opts.variant = VBMF_VARIANT_TRIAL_DIAG / VBMF_VARIANT_TRIAL_DIAGVAR; src/vbmf_trial.jl,
 * diagonal branch) ---------------
 * vbmf_trial_parameters (src/vbmf_trial.jl:68-131): A = [A1 [A2; A3]] -- A1 the first H0 columns (all M rows), A2 / A3 the
 * other H1 columns of rows m < M0 / m >= M0; each block has its own Gamma hyper-prior (alpha0g, beta0g), g = 1, 2, 3
 * (:357-400).  Everything else is the two-group model's: state through vbmf_sparse_set_state / get_state, updates through
 * vbmf_sparse_step, vbls! through vbmf_sparse_run_fixed_basis (examples/mil_util.jl:194-197), lowerBound
 * (src/vbmf_trial.jl:630-680) through vbmf_sparse_lower_bound.
 * priors9 = {alpha01, beta01, alpha02, beta02, alpha03, beta03, alpha1, alpha2, alpha3} (the last three: the posterior shapes
 * the fields alpha1..alpha3 hold).  vbmf_trial_run: the vbmf_trial! loop (:528-604), est_priors as in vbmf_dual_run. */
int vbmf_trial_set_priors(vbmf_ctx* ctx, int64_t H0, int64_t M0, const double* priors9);
int vbmf_trial_get_priors(vbmf_ctx* ctx, int64_t* H0, int64_t* M0, double* priors9);
int vbmf_trial_run(vbmf_ctx* ctx, int64_t niter, double eps, int est_cb, int est_priors, int64_t* iters_done,
                   double* d_last, double* trace);


/* ---- preprocess (src/util.jl:73-86; examples/mil_util.jl:829) fused into the upload -------------------------
 * scaleY (:36-54: row mean / sqrt(row variance, n-1), variance <= 1e-15 -> 1, |y - mu| <= 1e-8 -> 0), drop the rows whose
 * scaled absolute sum is < 1e-5 (:75-78), multiply by lambda (:86).  Dropping rows changes L, which a context is
 * created with, hence two steps: open() uploads the caller's fp64 Y ONCE, keeps it resident on the device and
 * returns the kept-row count; the caller creates the context with that L and set_Y_preprocessed() tiles the kept
 * rows from the resident copy, transform applied on the fly (no second upload, no L x M temporaries). */
typedef struct vbmf_prep vbmf_prep;
int vbmf_preprocess_open(vbmf_prep** out, int device, const double* Y, int64_t L, int64_t M, int64_t ldY, int64_t* L_used);
/* optional read-back: kept rows (0-based, L_used of them), row means and denominators (L each); any may be NULL */
int vbmf_preprocess_rows(const vbmf_prep* plan, int64_t* used_rows0, double* mu, double* den);
int vbmf_set_Y_preprocessed(vbmf_ctx* ctx, const vbmf_prep* plan, double lambda);
int vbmf_preprocess_close(vbmf_prep* plan);

/* ---- multi-GPU: one process per GPU, Y row-sharded, RCCL all-reduce of Y'B and of the Grams ---- */
#define VBMF_UNIQUE_ID_BYTES 128
int vbmf_comm_unique_id(void* id128);                       /* rank 0 creates, host broadcasts */
int vbmf_comm_init(vbmf_ctx* ctx, const void* id128);       /* collective over all nranks ctxs */
/* Bring-up / test transport INSTEAD of RCCL: fn must sum `count` floats (is_double = 0) or doubles (1) of the DEVICE
 * buffer `buf` over all ranks in place, ordered after everything already enqueued on `hip_stream` and complete
 * (or stream-ordered) on return; returns 0 on success.  Lets N ranks share one GPU over a host-staged reduction
 * (tests/test_gpu_two_ranks.py), which RCCL refuses ("Duplicate GPU detected").  Not a performance path. */
typedef int (*vbmf_allreduce_fn)(void* user, void* buf, size_t count, int is_double, void* hip_stream);
int vbmf_comm_set_transport(vbmf_ctx* ctx, vbmf_allreduce_fn fn, void* user);

/* ---- measurement hooks (bench.py): HIP-event timing of the two streaming kernels ---- */
int vbmf_profile_enable(vbmf_ctx* ctx, int on);   /* 0: off; k > 0: time every k-th launch of each pass (the probe costs two
                                                     * event packets per timed launch, so a stride keeps it out of the throughput) */
/* out[0]=ms in Y'B pass, out[1]=launches, out[2]=ms in Y*A pass, out[3]=launches, out[4..7] reserved */
int vbmf_profile_read(vbmf_ctx* ctx, double* out8, int reset);
/* algorithmic bytes one launch of pass p (1|2) moves: Y once + factor in + result out */
int vbmf_pass_bytes(vbmf_ctx* ctx, int pass, double* bytes);
int vbmf_device_sync(vbmf_ctx* ctx);

/* ---- test hook: raw 32-bit words of an internal device buffer (layout tests, debugging) ---- */
#define VBMF_PEEK_P 0      /* pass-1 result slabs  [nsplit][Hp][Mp] fp32 */
#define VBMF_PEEK_Q 1      /* pass-2 result slabs  [nsplit][Hp][Lp] fp32 */
#define VBMF_PEEK_A32 2    /* AHat fp32 row-major  [Mp][Hp] */
#define VBMF_PEEK_B32 3    /* BHat fp32 row-major  [Lp][Hp] */
#define VBMF_PEEK_FA 4     /* AHat MFMA operand tiles */
#define VBMF_PEEK_FB 5     /* BHat MFMA operand tiles */
#define VBMF_PEEK_Y1 6     /* Y tiled for pass 1 */
#define VBMF_PEEK_Y2 7     /* Y tiled for pass 2 */
#define VBMF_PEEK_DIMS 8   /* int32 x 31: Hp, NH, mode, XT1, KS1, nsplit1, sps1, XT2, KS2, nsplit2, sps2, kstep, npart, narrow, streamk_per, streamk_grid, gram (vbmf_run / vbmf_sparse_run takes the Gram form), gram_built, gram_build_us, gram_nsplit,
                              p_frag / q_frag (the last pass 1 / pass 2 launch wrote its product fragment-major: [XT][NH][64][16]),
                              q_epi (the last pass 2 launch ran the register epilogue and stored no product), lds8 (H >= 128 bf16x2
                              passes run the LDS-DMA kernel), xcd_map (split-K launches use the XCD-aware work map), post3 (H >= 128
                              bf16 factor updates run post_frag3 rather than post_frag2), sparse_a_fused (the ARD-sparse A update writes its
                              operand tiles itself, VBMF_SPARSE_A_FUSED), set_y_rows_us (device time of the last vbmf_set_Y_rows call
                              between two HIP events on the context's stream: staged copies, tiling kernels, ||Y||^2),
                              b_pending (a Gram-form run has ended and BHat of its last sweep is not materialised yet: the first
                              reader of B pays one streaming pass), b_materialised (how often that pass has run on demand), out_rows_us (device time of the last
                              vbmf_get_YHat_rows / vbmf_get_factor_rows call between two HIP events on the context's stream: kernels, staged copies).
                              This peek never materialises B; every other one does, and shows its buffer as a run's end left it */
#define VBMF_PEEK_CHAIN 9  /* uint64 x 8 (16 words): last durations in 10 ns ticks of the in-launch control chain's parts
                              (ctrl_end, SigmaA, lambda_max(dB'dB) + loop test, SigmaB) and of the register epilogue's tail in
                              workgroup 0 of the Y*A pass (wait for + load of the SigmaB table, tiles, fold + store, reserved) */
#define VBMF_PEEK_STATE 10 /* fp64 control state (two words per double): [A'A | B'B | dB'dB | tr(B'YA) x 8 | ...], Hp x Hp blocks */
#define VBMF_PEEK_GRAM_W 11 /* Gram form: the current W fp32 row-major [32 GT][Hp] (rows >= M zero) */
#define VBMF_PEEK_GRAM_PQ 12 /* Gram form: [P | Q] = G [W | W - W_old], fp32, each [XT1][NH][64][16] fragment-major */
#define VBMF_PEEK_GRAM_G 13  /* Gram form: G = Y'Y as fp32 MFMA operand fragments [GT][2 GT][64][8], GT = XT1 rounded up to 16:
                               word ((p 2 GT + j) 64 + lane) 8 + e, lane = 32 half + c, holds G[32 p + c][16 j + 8 half + e];
                               rows / columns >= M zero (0 words before the first run that takes the Gram form) */
#define VBMF_PEEK_SA32 14  /* SigmaA / sigma2 as the fp32 table the last A update multiplied by, row-major [Hp][Hp] */
#define VBMF_PEEK_SB32 15  /* SigmaB / sigma2 as the fp32 table the last B update multiplied by, row-major [Hp][Hp] */
int vbmf_debug_peek(vbmf_ctx* ctx, int what, uint32_t* out, int64_t nwords, int64_t word_offset);
/* tuning hook: average milliseconds of `iters` back-to-back launches of streaming pass p (1|2) alone */
int vbmf_debug_time_pass(vbmf_ctx* ctx, int pass, int iters, double* ms);
/* test hooks for the in-launch hand-off of the Y*A pass's register epilogue (VBMF_ERR_SYNC path) */
#define VBMF_DEBUG_EPI_SPIN_LIMIT 0   /* polls (~0.4 us each) the epilogue waits for the SigmaB table before giving up; default 2^22 */
#define VBMF_DEBUG_EPI_EXPECT_SKEW 1  /* != 0: the epilogue waits for a sequence number nobody publishes (forces the timeout) */
#define VBMF_DEBUG_SIGMA_B_PPM 2      /* test hook: the SigmaB / sigma2 table the B update multiplies by is scaled by (1 + value * 1e-6) --
                                         a deliberate, known-size regression that the parity asserts must catch (tests/test_gpu_soak.py) */
#define VBMF_DEBUG_EXACT_LAMBDA 3      /* lambda_max of the spectral norms at H <= 64: != 0 the Lanczos iteration every larger rank uses (exact inside
                                         eigenvalue clusters too), 0 (default) the repeated squaring: exact off clusters, up to ~2.5e-4 inside one, and
                                         faster -- 0.3-0.6 % of the sweep rate at 100k x 10k, 40 % on narrow problems and short row shards, where the
                                         control chain is the critical path.  Environment VBMF_EXACT_LAMBDA=1 at vbmf_create sets it for a whole job. */
int vbmf_debug_set(vbmf_ctx* ctx, int what, int64_t value);
/* test hook for the spectral norm behind `delta` (src/util.jl:27-29: norm(::Matrix) of Julia 0.5 = the largest singular value; for the
   H x H Gram the library keeps, its largest eigenvalue): lambda_max of the symmetric positive semi-definite H x H matrix G (column-major
   doubles, H = the context's rank) by the SAME device kernel the run loop uses for that rank (H <= 64: repeated squaring + Rayleigh
   quotient; H > 64: Lanczos), and the kernel's time in microseconds.  Overwrites the context's delta-Gram scratch (recomputed by every
   sweep), nothing else. */
int vbmf_debug_lambda_max(vbmf_ctx* ctx, const double* G, double* lambda_max, double* kernel_us);
/* test hook for the blocked inverse of the H x H covariance updates (csrc/blk_inverse.hpp): one 256-thread workgroup on the current
   device sweeps the identity-padded LDS image of the symmetric matrix K (row-major doubles, order 1 <= H <= 128) at the tier H selects
   (16, 32, 64 or 128 rows), with the four-wave schedule of the control chain (waves = 4) or with one wave of it running the one-wave
   schedule of the per-column inverses (waves = 1).  out: the n x n image afterwards, n = H rounded up to a multiple of 16, row-major --
   the upper 16 x 16 blocks hold -inv(K) (identity padding beyond H), the lower blocks are returned as zeros; logdet: log det K from
   the pivots; bad: != 0 if a pivot was not positive or not finite.  Needs no context. */
int vbmf_debug_blk_sweep(const double* K, int64_t H, int waves, double* out, double* logdet, int* bad);

#ifdef __cplusplus
}
#endif
#endif /* VBMF_HIP_H */
