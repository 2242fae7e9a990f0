"""ctypes binding of include/vbmf_hip.h -- the same entry points a Julia `ccall` binds.

The library is loaded from this directory only (built in-tree by build.py).  If it is missing the
import fails loudly: there is no CPU fallback and no alternate backend.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# VBMF_HIP_LIB: another build of the SAME library (A/B tuning builds under variants/); default: the in-tree build.
# An override must exist and export every symbol of include/vbmf_hip.h (lib() binds them all and fails loudly otherwise); it is NOT
# covered by build.py's source-hash stamp -- whoever builds a variant is responsible for building it from the current sources.
LIB_PATH = os.environ.get("VBMF_HIP_LIB") or os.path.join(_HERE, "libvbmf_hip.so")
if os.environ.get("VBMF_HIP_LIB") and not os.path.isfile(LIB_PATH):
    raise FileNotFoundError(f"VBMF_HIP_LIB={LIB_PATH}: no such library (A/B variant builds: scripts/README.md)")

VBMF_Y_F32, VBMF_Y_BF16 = 0, 1
VBMF_SRC_F64, VBMF_SRC_F32, VBMF_SRC_BF16 = 0, 1, 2      # src_dtype of vbmf_set_Y_rows
VBMF_DST_F64, VBMF_DST_F32, VBMF_DST_BF16 = 0, 1, 2      # dst_dtype of vbmf_get_YHat_rows / vbmf_get_factor_rows
VBMF_OUT_YHAT, VBMF_OUT_RESIDUAL = 0, 1                  # `what` of vbmf_get_YHat_rows
VBMF_FACTOR_A, VBMF_FACTOR_B = 0, 1                      # `which` of vbmf_get_factor_rows
VBMF_FACTOR_AUTO, VBMF_FACTOR_BF16, VBMF_FACTOR_BF16X2 = 0, 1, 2
VBMF_FACTOR_BF16_MAX_H = 128      # vbmf_create refuses the single-bf16 factor operand above this rank (include/vbmf_hip.h)
VBMF_VARIANT_BASIC, VBMF_VARIANT_SPARSE_DIAG, VBMF_VARIANT_SPARSE_DIAGVAR, VBMF_VARIANT_DUAL_DIAG, VBMF_VARIANT_TRIAL_DIAG = 0, 1, 2, 3, 4
VBMF_VARIANT_DUAL_DIAGVAR, VBMF_VARIANT_TRIAL_DIAGVAR = 5, 6
VBMF_COMPAT_SPECTRAL_DELTA, VBMF_COMPAT_SPARSE_REPEAT, VBMF_COMPAT_DEFAULT = 1, 2, 0xFFFFFFFF
STEP_A, STEP_B, STEP_CA, STEP_CB, STEP_SIGMA2 = 1, 2, 4, 8, 16
UNIQUE_ID_BYTES = 128
# vbmf_fit_batched_form (include/vbmf_hip.h): the forms, form = 2's width factor and the LDS a fit may use
VBMF_FIT_FORM_STREAM, VBMF_FIT_FORM_GRAM, VBMF_FIT_FORM_AUTO = 0, 1, 2
VBMF_FIT_GRAM_WIDE_FACTOR = 2
VBMF_FIT_LDS_CAP_BYTES = 144 * 1024
VBMF_GRAM_FORM_DEFAULT, VBMF_GRAM_FORM_OFF, VBMF_GRAM_FORM_ON = 0, 1, 2
GRAM_FORMS = {"stream": VBMF_GRAM_FORM_OFF, "gram": VBMF_GRAM_FORM_ON}
FIT_FORMS = {"stream": VBMF_FIT_FORM_STREAM, "gram": VBMF_FIT_FORM_GRAM, "auto": VBMF_FIT_FORM_AUTO}
# vbmf_ard_fit_batched_form (include/vbmf_hip.h): one wide ARD-family fit over many workgroups.  The four constants are measured there
VBMF_FIT_FORM_SPLIT = 3
VBMF_FIT_SPLIT_COLS, VBMF_FIT_SPLIT_MIN_COLS, VBMF_FIT_SPLIT_MIN_COLS_FULL, VBMF_FIT_SPLIT_CHUNK = 128, 160, 160, 8
ARD_FIT_FORMS = {"stream": VBMF_FIT_FORM_STREAM, "auto": VBMF_FIT_FORM_AUTO, "split": VBMF_FIT_FORM_SPLIT}


def fit_form_code(form):
    """'stream' / 'gram' / 'auto' -> the C ABI's form; anything else is refused (before the library is touched)"""
    if not isinstance(form, str) or form not in FIT_FORMS:
        raise ValueError(f"form = {form!r} ('stream', 'gram' or 'auto')")
    return FIT_FORMS[form]


def ard_fit_form_code(form):
    """'stream' / 'split' / 'auto' -> the C ABI's form for the ARD families; 'gram' is the basic model's alone"""
    if form == "gram":
        raise ValueError("form = 'gram': the ARD-sparse, two-group and three-group models have no Gram form (the element-wise precision "
                         "on A breaks A = Y'V); it serves the basic model's wide bags through vbmf_batch_")
    if not isinstance(form, str) or form not in ARD_FIT_FORMS:
        raise ValueError(f"form = {form!r} ('stream', 'split' or 'auto')")
    return ARD_FIT_FORMS[form]


def ard_slice_cols(slice_cols):
    """None / 0 -> 0 (VBMF_FIT_SPLIT_COLS); otherwise a multiple of 8, at least 8"""
    sc = 0 if slice_cols is None else int(slice_cols)
    if sc != 0 and (sc < 8 or sc % 8):
        raise ValueError(f"slice_cols = {slice_cols!r} (None, or a multiple of 8)")
    return sc


def ard_fit_slices(Mb, slice_cols=None):
    """the workgroups of the column pass a fit of Mb columns takes under form='split'"""
    sc = ard_slice_cols(slice_cols) or VBMF_FIT_SPLIT_COLS
    return -(-int(Mb) // sc)


def ard_fit_form_auto(Mb, full_cov=False):
    """the form a fit of Mb columns takes under form='auto': 3 (split) or 0 (stream)"""
    return VBMF_FIT_FORM_SPLIT if Mb >= (VBMF_FIT_SPLIT_MIN_COLS_FULL if full_cov else VBMF_FIT_SPLIT_MIN_COLS) else VBMF_FIT_FORM_STREAM


def fit_gram_fits(L, H):
    """the Gram form's state (B, T, V: 3 L H doubles) fits in LDS behind the fixed part: one P x (P + 2) inverse image and nine
    H x H matrices, P = 16 for H <= 16, else 32 (include/vbmf_hip.h)"""
    P = 16 if H <= 16 else 32
    return 3 * L * H <= VBMF_FIT_LDS_CAP_BYTES // 8 - (P * (P + 2) + 9 * H * H)


def fit_form_auto(L, Mb, H):
    """the form a fit of an L x Mb bag takes under form='auto': 1 (Gram) or 0 (stream)"""
    return int(Mb >= VBMF_FIT_GRAM_WIDE_FACTOR * L and fit_gram_fits(L, H))

# every symbol include/vbmf_hip.h declares (checked by tests/test_capi_symbols.py)
SYMBOLS = [
    "vbmf_default_opts", "vbmf_create", "vbmf_destroy", "vbmf_last_error", "vbmf_set_Y", "vbmf_set_Y_rows", "vbmf_set_Y_synthetic",
    "vbmf_get_Y", "vbmf_get_trYY", "vbmf_set_state", "vbmf_get_state", "vbmf_step", "vbmf_run", "vbmf_run_fixed_basis",
    "vbmf_run_fixed_basis_batched", "vbmf_fit_batched", "vbmf_fit_batched_form", "vbmf_bags_row_gram", "vbmf_get_YHat",
    "vbmf_elbo", "vbmf_comm_unique_id", "vbmf_comm_init", "vbmf_comm_set_transport", "vbmf_profile_enable", "vbmf_profile_read",
    "vbmf_pass_bytes", "vbmf_device_sync", "vbmf_debug_peek", "vbmf_debug_time_pass", "vbmf_debug_lambda_max",
    "vbmf_sparse_set_state", "vbmf_sparse_get_state", "vbmf_sparse_step", "vbmf_sparse_run", "vbmf_sparse_run_fixed_basis",
    "vbmf_sparse_run_fixed_basis_batched", "vbmf_sparse_fit_batched", "vbmf_local_fit_batched", "vbmf_rows_fit_batched",
    "vbmf_ard_fit_batched_form",
    "vbmf_sparse_lower_bound", "vbmf_sparse_set_noise_rows", "vbmf_sparse_get_noise_rows", "vbmf_preprocess_open", "vbmf_preprocess_rows", "vbmf_set_Y_preprocessed",
    "vbmf_preprocess_close", "vbmf_dual_set_priors", "vbmf_dual_get_priors", "vbmf_dual_run",
    "vbmf_trial_set_priors", "vbmf_trial_get_priors", "vbmf_trial_run",
    "vbmf_sparse_set_full_cov", "vbmf_sparse_set_SigmaA", "vbmf_sparse_get_SigmaA",
    "vbmf_sparse_lower_bound_trimmed", "vbmf_debug_set",
    "vbmf_bag_residuals", "vbmf_sparse_lower_bound_batched", "vbmf_bag_least_squares", "vbmf_bag_least_squares_jobs", "vbmf_set_gram_form",
    "vbmf_sparse_fixed_basis_jobs", "vbmf_sparse_scored_jobs", "vbmf_debug_vbls_jobs_lds_cols",
    "vbmf_fixed_basis_jobs", "vbmf_debug_fixed_basis_jobs_lds_cols",
    "vbmf_get_YHat_rows", "vbmf_get_factor_rows", "vbmf_set_Y_gather", "vbmf_debug_blk_sweep",
]
VBMF_OK, VBMF_ERR_INVALID, VBMF_ERR_NO_DEVICE, VBMF_ERR_HIP, VBMF_ERR_NUMERIC, VBMF_ERR_COMM, VBMF_ERR_UNSUPPORTED, VBMF_ERR_SYNC = 0, -1, -2, -3, -4, -5, -6, -7
DEBUG_EPI_SPIN_LIMIT, DEBUG_EPI_EXPECT_SKEW, DEBUG_SIGMA_B_PPM, DEBUG_EXACT_LAMBDA = 0, 1, 2, 3
SSTEP_A, SSTEP_B, SSTEP_CA, SSTEP_CB, SSTEP_SIGMA, SSTEP_PRIORS = 1, 2, 4, 8, 16, 32
(PEEK_P, PEEK_Q, PEEK_A32, PEEK_B32, PEEK_FA, PEEK_FB, PEEK_Y1, PEEK_Y2, PEEK_DIMS, PEEK_CHAIN, PEEK_STATE, PEEK_GRAM_W,
 PEEK_GRAM_PQ, PEEK_GRAM_G, PEEK_SA32, PEEK_SB32) = range(16)


class VbmfOpts(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("device", C.c_int32), ("y_dtype", C.c_int32), ("factor_dtype", C.c_int32),
        ("variant", C.c_int32), ("reference_compat", C.c_uint32), ("nranks", C.c_int32), ("rank", C.c_int32),
        ("L_global", C.c_int64), ("row_offset", C.c_int64), ("pass1_splits", C.c_int32), ("reserved", C.c_int32),
    ]


class VbmfSparseHyper(C.Structure):
    _fields_ = [("alpha0", C.c_double), ("beta0", C.c_double), ("gamma0", C.c_double), ("delta0", C.c_double),
                ("eta0", C.c_double), ("zeta0", C.c_double)]


# int fn(void* user, void* buf, size_t count, int is_double, void* hip_stream)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)


class VbmfError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"vbmf_hip error {code}: {msg}")
        self.code = code


_lib = None


def lib():
    """Load libvbmf_hip.so (once).  Raises if the HIP library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # Load order matters in a process that also uses PyTorch-ROCm: torch bundles its own copies of
    # libamdhip64/librccl (same SONAMEs as /opt/rocm's).  If torch is imported AFTER this library the
    # process aborts at interpreter exit (double free in the duplicated runtime); torch first is fine --
    # this library then binds to the runtime torch loaded.  So load torch (when present) first.  It is
    # not used for anything here.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python vbmatrixfactorization.jl_amd/build.py` "
            "(hipcc, gfx950).  This package has no CPU fallback.")
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    dp, i64, i32, vp = C.POINTER(C.c_double), C.c_int64, C.c_int, C.c_void_p
    L.vbmf_default_opts.argtypes = [C.POINTER(VbmfOpts)]
    L.vbmf_default_opts.restype = None
    L.vbmf_create.argtypes = [C.POINTER(vp), i64, i64, i64, C.POINTER(VbmfOpts)]
    L.vbmf_destroy.argtypes = [vp]
    L.vbmf_last_error.argtypes = [vp]
    L.vbmf_last_error.restype = C.c_char_p
    L.vbmf_set_Y.argtypes = [vp, dp, i64]
    L.vbmf_set_Y_rows.argtypes = [vp, vp, C.c_int32, C.c_int32, i64, i64, i64, i64]
    L.vbmf_set_Y_gather.argtypes = [vp, vp, C.POINTER(i64), i64]
    L.vbmf_set_Y_synthetic.argtypes = [vp, C.c_uint64, i64, C.c_double]
    L.vbmf_get_Y.argtypes = [vp, dp, i64, i64, i64]
    L.vbmf_get_trYY.argtypes = [vp, dp]
    L.vbmf_set_state.argtypes = [vp, dp, i64, dp, i64, dp, dp, dp, dp, C.c_double, C.POINTER(i64), i64, i64]
    L.vbmf_get_state.argtypes = [vp, dp, i64, dp, i64, dp, dp, dp, dp, dp]
    L.vbmf_step.argtypes = [vp, i32]
    L.vbmf_run.argtypes = [vp, i64, C.c_double, i32, i32, C.POINTER(i64), dp, dp]
    L.vbmf_run_fixed_basis.argtypes = [vp, i64]
    L.vbmf_run_fixed_basis_batched.argtypes = [vp, i64, C.POINTER(i64), i64, dp, dp, dp, dp, i64]
    L.vbmf_fit_batched.argtypes = ([vp, i64, C.POINTER(i64), i64, C.POINTER(i64), i64, C.c_double, i32, i32] + [dp] * 7
                                   + [C.POINTER(i64), dp, C.POINTER(i64), dp])
    L.vbmf_fit_batched_form.argtypes = L.vbmf_fit_batched.argtypes + [i64, C.POINTER(i64)]
    L.vbmf_bags_row_gram.argtypes = [vp, i64, C.POINTER(i64), dp]
    L.vbmf_sparse_run_fixed_basis.argtypes = [vp, i64]
    L.vbmf_sparse_run_fixed_basis_batched.argtypes = [vp, i64, C.POINTER(i64), i64, i32, dp, dp, dp, dp, dp, dp, dp, dp, dp, dp, dp]
    L.vbmf_sparse_fit_batched.argtypes = ([vp, i64, C.POINTER(i64), i64, C.POINTER(i64), i64, C.c_double, i32, i32, i32, i64] + [dp] * 16
                                          + [C.POINTER(i64), dp, C.POINTER(i64), dp])
    L.vbmf_local_fit_batched.argtypes = ([vp, i64, C.POINTER(i64), i64, C.POINTER(i64), i64, C.c_double, i32, i32, i32, i64,
                                          C.POINTER(i64), i64] + [dp] * 16 + [C.POINTER(i64), dp, C.POINTER(i64), dp])
    L.vbmf_rows_fit_batched.argtypes = L.vbmf_local_fit_batched.argtypes
    L.vbmf_ard_fit_batched_form.argtypes = L.vbmf_local_fit_batched.argtypes + [C.c_int, i64, i64, C.POINTER(i64)]
    L.vbmf_get_YHat.argtypes = [vp, dp, i64]
    L.vbmf_get_YHat_rows.argtypes = [vp, C.c_int32, vp, C.c_int32, C.c_int32, i64, i64, i64, i64]
    L.vbmf_get_factor_rows.argtypes = [vp, C.c_int32, vp, C.c_int32, C.c_int32, i64, i64, i64, i64]
    L.vbmf_elbo.argtypes = [vp, dp]
    L.vbmf_comm_unique_id.argtypes = [vp]
    L.vbmf_comm_init.argtypes = [vp, vp]
    L.vbmf_comm_set_transport.argtypes = [vp, ALLREDUCE_FN, vp]
    L.vbmf_profile_enable.argtypes = [vp, i32]
    L.vbmf_profile_read.argtypes = [vp, dp, i32]
    L.vbmf_pass_bytes.argtypes = [vp, i32, dp]
    L.vbmf_device_sync.argtypes = [vp]
    L.vbmf_debug_peek.argtypes = [vp, i32, C.POINTER(C.c_uint32), i64, i64]
    L.vbmf_debug_time_pass.argtypes = [vp, i32, i32, dp]
    L.vbmf_debug_lambda_max.argtypes = [vp, dp, dp, dp]
    L.vbmf_sparse_set_state.argtypes = [vp, dp, dp, dp, dp, dp, i64, dp, dp, dp, C.c_double, C.c_double,
                                        C.POINTER(VbmfSparseHyper), C.POINTER(i64), i64, i64]
    L.vbmf_sparse_get_state.argtypes = [vp, dp, dp, dp, dp, dp, dp, i64, dp, dp, dp, dp, dp]
    L.vbmf_sparse_step.argtypes = [vp, i32]
    L.vbmf_sparse_run.argtypes = [vp, i64, C.c_double, i32, C.POINTER(i64), dp, dp]
    L.vbmf_sparse_lower_bound.argtypes = [vp, i32, dp]
    L.vbmf_sparse_lower_bound_trimmed.argtypes = [vp, i32, C.c_double, dp]
    L.vbmf_debug_set.argtypes = [vp, i32, i64]
    L.vbmf_bag_residuals.argtypes = [vp, i64, C.POINTER(i64), dp, i64, dp]
    L.vbmf_sparse_lower_bound_batched.argtypes = [vp, i64, C.POINTER(i64), i32, C.c_double, i32] + [dp] * 15
    L.vbmf_bag_least_squares.argtypes = [vp, i64, C.POINTER(i64), dp, i64, i64, C.c_double, dp, i64, dp]
    L.vbmf_bag_least_squares_jobs.argtypes = [vp, i64, C.POINTER(i64), i64, C.POINTER(i64), dp, dp, i64, C.POINTER(i64), C.POINTER(i64), dp, dp,
                                              C.POINTER(i64)]
    L.vbmf_sparse_fixed_basis_jobs.argtypes = [vp, i64, C.POINTER(i64), i64, i64, i32, i64, dp, dp, dp, dp, dp, dp, dp, dp, i64,
                                               C.POINTER(i64), C.POINTER(i64), dp, dp, dp, dp, dp, dp, dp, dp, C.POINTER(i64)]
    L.vbmf_sparse_scored_jobs.argtypes = ([vp, i64, C.POINTER(i64), i64, i32, i32, i64, C.POINTER(i64)] + [dp] * 14
                                          + [i64, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)] + [dp] * 10 + [C.POINTER(i64)])
    L.vbmf_debug_vbls_jobs_lds_cols.argtypes = [i64, i32]
    L.vbmf_fixed_basis_jobs.argtypes = [vp, i64, C.POINTER(i64), i64, i64, C.POINTER(i64), dp, dp, dp, dp, i64, C.POINTER(i64),
                                        C.POINTER(i64), dp, dp, dp, dp, dp, C.POINTER(i64)]
    L.vbmf_debug_fixed_basis_jobs_lds_cols.argtypes = [i64]
    L.vbmf_debug_blk_sweep.argtypes = [dp, i64, i32, dp, dp, C.POINTER(i32)]
    L.vbmf_sparse_set_full_cov.argtypes = [vp, i32]
    L.vbmf_set_gram_form.argtypes = [vp, i32]
    L.vbmf_sparse_set_SigmaA.argtypes = [vp, dp]
    L.vbmf_sparse_get_SigmaA.argtypes = [vp, dp]
    L.vbmf_dual_set_priors.argtypes = [vp, i64] + [C.c_double] * 6
    L.vbmf_dual_get_priors.argtypes = [vp, C.POINTER(i64), dp]
    L.vbmf_dual_run.argtypes = [vp, i64, C.c_double, i32, i32, C.POINTER(i64), dp, dp]
    L.vbmf_trial_set_priors.argtypes = [vp, i64, i64, dp]
    L.vbmf_trial_get_priors.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), dp]
    L.vbmf_trial_run.argtypes = [vp, i64, C.c_double, i32, i32, C.POINTER(i64), dp, dp]
    L.vbmf_sparse_set_noise_rows.argtypes = [vp, dp, dp, C.c_double]
    L.vbmf_sparse_get_noise_rows.argtypes = [vp, dp, dp]
    L.vbmf_preprocess_open.argtypes = [C.POINTER(vp), i32, dp, i64, i64, i64, C.POINTER(i64)]
    L.vbmf_preprocess_rows.argtypes = [vp, C.POINTER(i64), dp, dp]
    L.vbmf_set_Y_preprocessed.argtypes = [vp, vp, C.c_double]
    L.vbmf_preprocess_close.argtypes = [vp]
    for name in SYMBOLS:
        if name not in ("vbmf_default_opts", "vbmf_last_error"):
            getattr(L, name).restype = C.c_int
    _lib = L
    return L


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def _i64ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64)) if a is not None else None


def _fcol(a, shape=None):
    """float64, column-major (Julia Array{Float64,2} memory)."""
    a = np.asarray(a, dtype=np.float64)
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError(f"expected shape {shape}, got {a.shape}")
    return np.asfortranarray(a)


def _pack_models(models, key, order="C"):
    """every model's m[key] as fp64, flattened in `order`, one after the other: how the (bag, model) job entries take a per-model input"""
    if not models:
        return np.empty(0)
    return np.concatenate([np.asarray(m[key], dtype=np.float64).reshape(-1, order=order) for m in models])


def _job_blocks(off, nb, jb, jk, Hs, noffs=3):
    """Where the (bag, model) job entries put job j's outputs.  Hs: the models' ranks, or one int where every model has that rank (the
    model index then does not bear on a block's size).  Returns (ok, Hj, widths) -- whether the job is in range, its model's rank, its
    bag's width (0 and 0 for a job out of range: that one is the library's to refuse, no block for it) -- and the first noffs of
    (boff, soff, hoff), the cumulative offsets (njobs + 1,) of the M_b*H_k-, H_k^2- and H_k-long blocks."""
    ok = (jb >= 0) & (jb < nb)
    Hj = Hs
    if np.ndim(Hs):
        ok &= (jk >= 0) & (jk < Hs.size)
        Hj = np.where(ok, Hs[np.clip(jk, 0, max(Hs.size - 1, 0))], 0) if Hs.size >= 1 else np.zeros(jb.size, np.int64)
    b = np.clip(jb, 0, max(nb - 1, 0))
    widths = np.where(ok, off[b + 1] - off[b], 0) if nb >= 1 else np.zeros(jb.size, np.int64)
    return (ok, Hj, widths) + tuple(np.concatenate([[0], np.cumsum(v)]).astype(np.int64) for v in (widths * Hj, Hj * Hj, Hj)[:noffs])


def _is_tensor(a):
    """A torch tensor, told by its surface: torch itself is imported only once such an object has been passed."""
    return hasattr(a, "data_ptr") and hasattr(a, "is_cuda")


def y_source(src, device=0):
    """What vbmf_set_Y_rows needs to read `src` where it lies: (keep, address, VBMF_SRC_*, on_device, row_stride, col_stride), strides in
    elements; `keep` owns the memory for the duration of the call.  A float64 / float32 NumPy array that is C- or F-contiguous, or a
    view with one unit stride, is passed by its own address; any other view takes ONE contiguous copy in its own dtype.  A torch
    tensor (float64, float32, bfloat16; CPU, or the GPU with index `device`) is passed by data_ptr() and stride(); a CPU tensor with
    no unit stride is made contiguous first.  Raises TypeError / ValueError on anything else, before the library is touched."""
    if _is_tensor(src):
        import torch
        codes = {torch.float64: VBMF_SRC_F64, torch.float32: VBMF_SRC_F32, torch.bfloat16: VBMF_SRC_BF16}
        if src.dtype not in codes:
            raise TypeError(f"Y must be float64, float32 or bfloat16, got {src.dtype}")
        if src.dim() != 2:
            raise ValueError("Y must be a matrix")
        if src.is_cuda:
            if src.device.index != device:
                raise ValueError(f"Y lives on {src.device}, the context on GPU {device}")
            torch.cuda.current_stream(src.device).synchronize()         # whatever produces the tensor has finished
        elif src.device.type != "cpu":
            raise ValueError(f"Y lives on {src.device}: only CPU and GPU tensors can be read")
        rs, cs = _unit(src.shape, src.stride())
        if min(rs, cs) <= 0 or (not src.is_cuda and 1 not in (rs, cs)):  # an expanded tensor; a host view with no unit stride
            src = src.contiguous()
            rs, cs = _unit(src.shape, src.stride())
        return src, src.data_ptr(), codes[src.dtype], int(src.is_cuda), rs, cs
    a = src if isinstance(src, np.ndarray) else np.asarray(src)
    if a.dtype not in (np.float64, np.float32):
        raise TypeError(f"Y must be float64 or float32, got {a.dtype}")
    if a.ndim != 2:
        raise ValueError("Y must be a matrix")
    es = a.itemsize
    st = _unit(a.shape, tuple(x // es if x % es == 0 else 0 for x in a.strides))
    if min(st) <= 0 or 1 not in st:
        a = np.ascontiguousarray(a)                                     # one copy, in its own dtype
        st = _unit(a.shape, tuple(x // es for x in a.strides))
    return a, a.ctypes.data, VBMF_SRC_F64 if a.dtype == np.float64 else VBMF_SRC_F32, 0, st[0], st[1]


def y_sink(dst, device=0):
    """What vbmf_get_YHat_rows / vbmf_get_factor_rows need to write into `dst` where it lies -- the counterpart of y_source:
    (target, address, VBMF_DST_*, on_device, row_stride, col_stride, finish), strides in elements.  `target` owns the memory the library
    writes for the duration of the call; `finish` is None, or -- for a host view with no unit stride, which is filled through one
    contiguous temporary of its own dtype -- the call that assigns the temporary back into dst afterwards.  Accepted: a writable
    float64 / float32 NumPy array; a torch tensor (float64, float32, bfloat16) on the CPU or on the GPU with index `device`, whose
    current stream is synchronised first.  Raises TypeError / ValueError, before the library is touched, on a read-only array, any other
    dtype, anything that is not a matrix, another GPU and an expanded (stride-0) tensor."""
    if _is_tensor(dst):
        import torch
        codes = {torch.float64: VBMF_DST_F64, torch.float32: VBMF_DST_F32, torch.bfloat16: VBMF_DST_BF16}
        if dst.dtype not in codes:
            raise TypeError(f"the output must be float64, float32 or bfloat16, got {dst.dtype}")
        if dst.dim() != 2:
            raise ValueError("the output must be a matrix")
        if dst.is_cuda:
            if dst.device.index != device:
                raise ValueError(f"the output lives on {dst.device}, the context on GPU {device}")
        elif dst.device.type != "cpu":
            raise ValueError(f"the output lives on {dst.device}: only CPU and GPU tensors can be written")
        if any(n > 1 and st == 0 for n, st in zip(dst.shape, dst.stride())):
            raise ValueError("the output is an expanded (stride-0) tensor: its entries share memory")
        if dst.is_cuda:
            torch.cuda.current_stream(dst.device).synchronize()         # whatever still reads or writes the tensor has finished
        rs, cs = _unit(dst.shape, dst.stride())
        if not dst.is_cuda and 1 not in (rs, cs):
            tmp = torch.empty(tuple(dst.shape), dtype=dst.dtype)
            return tmp, tmp.data_ptr(), codes[dst.dtype], 0, *_unit(tmp.shape, tmp.stride()), (lambda: dst.copy_(tmp))
        return dst, dst.data_ptr(), codes[dst.dtype], int(dst.is_cuda), rs, cs, None
    if not isinstance(dst, np.ndarray):
        raise TypeError(f"the output must be a NumPy array or a torch tensor, got {type(dst).__name__}")
    if dst.dtype not in (np.float64, np.float32):
        raise TypeError(f"the output must be float64 or float32, got {dst.dtype}")
    if dst.ndim != 2:
        raise ValueError("the output must be a matrix")
    if not dst.flags.writeable:
        raise ValueError("the output array is read-only")
    es = dst.itemsize
    code = VBMF_DST_F64 if dst.dtype == np.float64 else VBMF_DST_F32
    st = _unit(dst.shape, tuple(x // es if x % es == 0 else 0 for x in dst.strides))
    if min(st) <= 0 or 1 not in st:
        tmp = np.empty(dst.shape, dtype=dst.dtype)

        def finish():
            dst[...] = tmp
        return tmp, tmp.ctypes.data, code, 0, *_unit(tmp.shape, tuple(x // es for x in tmp.strides)), finish
    return dst, dst.ctypes.data, code, 0, st[0], st[1], None


def _unit(shape, strides):
    """Element strides of a matrix with the free stride of a length-1 dimension set so that lines do not overlap."""
    rs, cs = int(strides[0]), int(strides[1])
    if shape[0] == 1:
        rs = max(1, shape[1] * cs) if cs > 0 else rs
    if shape[1] == 1:
        cs = max(1, shape[0] * rs) if rs > 0 else cs
    return rs, cs


class PreprocessPlan:
    """preprocess (src/util.jl:73-86) fused into the upload: holds the caller's fp64 Y on the device with its row
    statistics and the kept rows; Context.set_Y_preprocessed tiles from it.  Use as a context manager."""

    def __init__(self, Y, device=0):
        Yf = np.asfortranarray(Y, dtype=np.float64)
        self.L, self.M = Yf.shape
        self._lib = lib()
        self._h = C.c_void_p()
        n = C.c_int64()
        rc = self._lib.vbmf_preprocess_open(C.byref(self._h), device, _dptr(Yf), self.L, self.M, self.L, C.byref(n))
        if rc != 0:
            raise VbmfError(rc, self._lib.vbmf_last_error(None).decode())
        self.L_used = n.value

    def rows(self):
        r = np.empty(self.L_used, dtype=np.int64); mu = np.empty(self.L); den = np.empty(self.L)
        self._lib.vbmf_preprocess_rows(self._h, r.ctypes.data_as(C.POINTER(C.c_int64)), _dptr(mu), _dptr(den))
        return r, mu, den

    def close(self):
        if self._h:
            self._lib.vbmf_preprocess_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """One problem on one GPU: thin, explicit wrapper over the C ABI (no numerics on the host)."""

    def __init__(self, L, M, H, y_dtype=VBMF_Y_BF16, factor_dtype=VBMF_FACTOR_AUTO, device=0, nranks=1, rank=0,
                 L_global=0, row_offset=0, reference_compat=VBMF_COMPAT_DEFAULT, pass1_splits=0,
                 variant=VBMF_VARIANT_BASIC):
        self._lib = lib()
        o = VbmfOpts()
        self._lib.vbmf_default_opts(C.byref(o))
        o.device, o.y_dtype, o.factor_dtype = device, y_dtype, factor_dtype
        o.variant = variant
        o.nranks, o.rank, o.L_global, o.row_offset = nranks, rank, L_global, row_offset
        o.reference_compat, o.pass1_splits = reference_compat, pass1_splits
        self._h = C.c_void_p()
        rc = self._lib.vbmf_create(C.byref(self._h), L, M, H, C.byref(o))
        if rc != 0:
            msg = self._lib.vbmf_last_error(None).decode()
            self._h = C.c_void_p()
            raise VbmfError(rc, msg)
        self.L, self.M, self.H = int(L), int(M), int(H)
        self.device = int(device)

    def _chk(self, rc):
        if rc != 0:
            raise VbmfError(rc, self._lib.vbmf_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.vbmf_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- Y ----
    def set_Y(self, Y):
        Y = _fcol(Y, (self.L, self.M))
        self._chk(self._lib.vbmf_set_Y(self._h, _dptr(Y), Y.shape[0]))

    def set_Y_rows(self, src, row0=0, nrows=None):
        """Rows [row0, row0 + nrows) of Y from `src` as it lies (vbmf_set_Y_rows): a float64 / float32 NumPy array or a torch tensor
        (float64, float32, bfloat16; CPU or this context's GPU), see y_source.  nrows defaults to src's rows; blocks come in
        ascending order, each a multiple of 32 rows but the last."""
        shape = tuple(src.shape) if hasattr(src, "shape") else np.shape(src)
        if len(shape) != 2:
            raise ValueError("Y must be a matrix")
        n = shape[0] if nrows is None else int(nrows)
        if shape[1] != self.M or shape[0] != n:
            raise ValueError(f"expected a block of shape ({n}, {self.M}), got {shape}")
        if row0 < 0 or n < 1 or row0 + n > self.L:
            raise ValueError(f"rows [{row0}, {row0 + n}) do not lie in a matrix of {self.L} rows")
        keep, addr, code, on_dev, rs, cs = y_source(src, self.device)
        self._chk(self._lib.vbmf_set_Y_rows(self._h, addr, code, on_dev, int(row0), int(n), rs, cs))
        del keep

    def set_Y_gather(self, src_ctx, col_index):
        """Y := columns col_index (0-based, in that order, duplicates allowed) of the Y stored in the context src_ctx, gathered on the
        device (vbmf_set_Y_gather): what set_Y(src_ctx.get_Y()[:, col_index]) leaves, bit for bit, with no host matrix and no upload."""
        idx = np.ascontiguousarray(col_index, dtype=np.int64).reshape(-1)
        self._chk(self._lib.vbmf_set_Y_gather(self._h, src_ctx._h, _i64ptr(idx), idx.size))

    def set_Y_preprocessed(self, plan, lam):
        self._chk(self._lib.vbmf_set_Y_preprocessed(self._h, plan._h, float(lam)))

    def set_Y_synthetic(self, seed, Hstar, noise_std):
        self._chk(self._lib.vbmf_set_Y_synthetic(self._h, seed, Hstar, noise_std))

    def get_Y(self, row0=0, nrows=None):
        nrows = self.L - row0 if nrows is None else nrows
        out = np.empty((nrows, self.M), dtype=np.float64, order="F")
        self._chk(self._lib.vbmf_get_Y(self._h, _dptr(out), nrows, row0, nrows))
        return out

    def trYY(self):
        v = C.c_double()
        self._chk(self._lib.vbmf_get_trYY(self._h, C.byref(v)))
        return v.value

    # ---- state ----
    def set_state(self, AHat, BHat, SigmaA, SigmaB, CA_diag, CB_diag, sigma2, labels0=(), H1=0):
        A = _fcol(AHat, (self.M, self.H)); B = _fcol(BHat, (self.L, self.H))
        SA = _fcol(SigmaA, (self.H, self.H)); SB = _fcol(SigmaB, (self.H, self.H))
        ca = np.ascontiguousarray(CA_diag, dtype=np.float64); cb = np.ascontiguousarray(CB_diag, dtype=np.float64)
        if ca.shape != (self.H,) or cb.shape != (self.H,):
            raise ValueError("CA_diag/CB_diag must have length H")
        lab = np.ascontiguousarray(labels0, dtype=np.int64)
        self._chk(self._lib.vbmf_set_state(self._h, _dptr(A), self.M, _dptr(B), self.L, _dptr(SA), _dptr(SB), _dptr(ca),
                                           _dptr(cb), float(sigma2), lab.ctypes.data_as(C.POINTER(C.c_int64)),
                                           lab.size, int(H1)))

    def get_state(self, want_B=True):
        A = np.empty((self.M, self.H), order="F"); B = np.empty((self.L, self.H), order="F") if want_B else None
        SA = np.empty((self.H, self.H), order="F"); SB = np.empty((self.H, self.H), order="F")
        ca = np.empty(self.H); cb = np.empty(self.H); s2 = C.c_double()
        self._chk(self._lib.vbmf_get_state(self._h, _dptr(A), self.M, _dptr(B), self.L, _dptr(SA), _dptr(SB), _dptr(ca),
                                           _dptr(cb), C.byref(s2)))
        return dict(AHat=A, BHat=B, SigmaA=SA, SigmaB=SB, CA_diag=ca, CB_diag=cb, sigma2=s2.value)

    # ---- updates ----
    def step(self, which):
        self._chk(self._lib.vbmf_step(self._h, which))

    def note(self):
        """The library's note on the last call that returned OK ('' if none): vbmf_last_error after success carries e.g. the
        'eps below the resolution of d' remark of vbmf_run (include/vbmf_hip.h)."""
        m = self._lib.vbmf_last_error(self._h).decode()
        return m if m.startswith("note:") else ""

    def _warn_note(self):
        m = self.note()
        if m:
            import warnings
            warnings.warn(m, RuntimeWarning, stacklevel=3)

    def run(self, niter, eps=1e-6, est_covs=False, est_var=False, want_trace=False):
        it = C.c_int64(); d = C.c_double()
        tr = np.zeros((max(niter, 1), 4)) if want_trace else None
        self._chk(self._lib.vbmf_run(self._h, niter, eps, int(est_covs), int(est_var), C.byref(it), C.byref(d),
                                     _dptr(tr)))
        self._warn_note()
        return it.value, d.value, (tr[:it.value] if want_trace else None)

    def run_fixed_basis(self, niter):
        self._chk(self._lib.vbmf_run_fixed_basis(self._h, int(niter)))

    def run_fixed_basis_batched(self, col_off, niter, sigma2, CA_diag, want_A=True):
        """vbls! over the bags side by side in this context's Y (vbmf_run_fixed_basis_batched): bag b = columns
        col_off[b] .. col_off[b+1]-1; B, SigmaB, CB from set_state; per-bag start values sigma2 (nbags,) and CA_diag (nbags, H).
        Returns dict(sigma2 (nbags,), CA_diag (nbags, H), SigmaA (nbags, H, H), AHat (M, H) or None).  The state is not changed."""
        off = np.ascontiguousarray(col_off, dtype=np.int64)
        nb = off.size - 1
        s2 = np.array(sigma2, dtype=np.float64, copy=True).reshape(-1)
        ca = np.array(CA_diag, dtype=np.float64, copy=True, order="C")
        if nb < 1 or s2.shape != (nb,) or ca.shape != (nb, self.H):
            raise ValueError(f"col_off describes {nb} bags: sigma2 must be ({nb},) and CA_diag ({nb}, {self.H})")
        SA = np.empty((nb, self.H, self.H))
        A = np.empty((self.M, self.H), order="F") if want_A else None
        self._chk(self._lib.vbmf_run_fixed_basis_batched(self._h, nb, off.ctypes.data_as(C.POINTER(C.c_int64)), int(niter), _dptr(s2),
                                                         _dptr(ca), _dptr(SA), _dptr(A), self.M))
        return dict(sigma2=s2, CA_diag=ca, SigmaA=SA, AHat=A)

    def fit_batched(self, col_off, fit_bag, niter, eps, BHat, SigmaB, CA, CB, sigma2, est_covs=False, est_var=False, want_trace=False,
                    form="stream", want_A=True):
        """Many independent vbmf! fits of the basic model in one launch (vbmf_fit_batched): fit f works on bag fit_bag[f] of the bags
        side by side in this context's Y (bag b = columns col_off[b] .. col_off[b+1]-1).  Per fit the start values BHat (nfits, L, H),
        SigmaB (nfits, H, H), the diagonals CA, CB (nfits, H) and sigma2 (nfits,).  Returns dict(BHat, SigmaB, CA, CB, sigma2, SigmaA
        (nfits, H, H), AHat (a list of M_b x H arrays; None with want_A=False), iters, d, status, trace (nfits, niter, 2) or None,
        form_used (nfits,)).  form: "stream" (vbmf_fit_batched itself), "gram" (every fit iterates on Y Y': the form for wide bags) or
        "auto" (fit_form_auto per fit) -- vbmf_fit_batched_form.  Neither the context's state nor its Y is changed."""
        code = fit_form_code(form)
        H = self.H
        off, fb, nb, nf, B, per_fit, tail = self._fit_prologue(col_off, fit_bag, niter, BHat, want_trace)
        SB = np.array(SigmaB, dtype=np.float64, copy=True, order="C")
        ca = np.array(CA, dtype=np.float64, copy=True, order="C")
        cb = np.array(CB, dtype=np.float64, copy=True, order="C")
        s2 = np.array(sigma2, dtype=np.float64, copy=True).reshape(-1)
        if SB.shape != (nf, H, H) or ca.shape != (nf, H) or cb.shape != (nf, H) or s2.shape != (nf,):
            raise ValueError(f"{nf} fits: SigmaB must be ({nf}, {H}, {H}), CA and CB ({nf}, {H}) and sigma2 ({nf},)")
        Ms = off[fb + 1] - off[fb]
        A = np.empty(int(np.sum(Ms)) * H) if want_A else None
        SA = np.empty((nf, H, H))
        used = np.zeros(nf, dtype=np.int64)
        args = (self._h, nb, _i64ptr(off), nf, _i64ptr(fb), int(niter), float(eps), int(bool(est_covs)), int(bool(est_var)), _dptr(B),
                _dptr(SB), _dptr(ca), _dptr(cb), _dptr(s2), _dptr(A), _dptr(SA), *tail)
        if code == VBMF_FIT_FORM_STREAM:
            self._chk(self._lib.vbmf_fit_batched(*args))
        else:
            self._chk(self._lib.vbmf_fit_batched_form(*args, code, _i64ptr(used)))
        ends = np.cumsum(Ms) * H
        As = [A[e - m * H:e].reshape(H, m).T for e, m in zip(ends, Ms)] if want_A else None   # column-major M_b x H blocks
        return dict(BHat=B.transpose(0, 2, 1), SigmaB=SB, CA=ca, CB=cb, sigma2=s2, SigmaA=SA, AHat=As, form_used=used, **per_fit)

    def _fit_prologue(self, col_off, fit_bag, niter, BHat, want_trace):
        """What the whole-fit batched calls marshal alike: col_off and fit_bag as int64 arrays (every fit_bag entry checked against the
        bags), nbags, nfits, the start values BHat (nfits, L, H) copied per fit column-major, the per-fit outputs as the entries of the
        returned dictionary -- iters, d, status, trace (None unless want_trace) -- and the pointers to them, every entry's last four
        arguments."""
        off = np.ascontiguousarray(col_off, dtype=np.int64)
        fb = np.ascontiguousarray(fit_bag, dtype=np.int64).reshape(-1)
        nb, nf = off.size - 1, fb.size
        if nb < 1 or nf < 1 or off.ndim != 1 or np.any(fb < 0) or np.any(fb >= nb):
            raise ValueError(f"col_off describes {nb} bags: every fit_bag entry must lie in 0..{nb - 1}")
        B = np.ascontiguousarray(np.asarray(BHat, dtype=np.float64).reshape(nf, self.L, self.H).transpose(0, 2, 1))
        per_fit = dict(iters=np.zeros(nf, dtype=np.int64), d=np.empty(nf), status=np.zeros(nf, dtype=np.int64),
                       trace=np.zeros((nf, int(niter), 2)) if want_trace else None)
        return off, fb, nb, nf, B, per_fit, (_i64ptr(per_fit["iters"]), _dptr(per_fit["d"]), _i64ptr(per_fit["status"]), _dptr(per_fit["trace"]))

    def row_gram(self, col_off):
        """K_b = Y_b Y_b' of every bag side by side in this context's Y, in fp64 on Y as stored (vbmf_bags_row_gram): (nbags, L, L)."""
        off = np.ascontiguousarray(col_off, dtype=np.int64)
        nb = off.size - 1
        if nb < 1 or off.ndim != 1:
            raise ValueError("col_off must describe at least one bag")
        K = np.empty((nb, self.L, self.L))
        self._chk(self._lib.vbmf_bags_row_gram(self._h, nb, off.ctypes.data_as(C.POINTER(C.c_int64)), _dptr(K)))
        return K

    def sparse_run_fixed_basis(self, niter):
        self._chk(self._lib.vbmf_sparse_run_fixed_basis(self._h, int(niter)))

    def sparse_run_fixed_basis_batched(self, col_off, niter, alpha, beta0, eta, zeta0, sigmaHat, CA, full_cov=False):
        """vbls! of the sparse models over the bags side by side in this context's Y (vbmf_sparse_run_fixed_basis_batched): bag b =
        columns col_off[b] .. col_off[b+1]-1; B, SigmaB from sparse_set_state; per bag alpha, beta0 (nbags, H), eta, zeta0 and the start
        value sigmaHat (nbags,); CA (M*H,) the start values in vec(A') order.  Returns dict(sigmaHat, zeta (nbags,), CA, beta,
        diagSigmaATVec, ATVecHat (M*H,), SigmaA (nbags, H, H)).  The state is not changed."""
        off = np.ascontiguousarray(col_off, dtype=np.int64)
        nb = off.size - 1
        al = np.array(alpha, dtype=np.float64, copy=True, order="C")
        b0 = np.array(beta0, dtype=np.float64, copy=True, order="C")
        et = np.array(eta, dtype=np.float64, copy=True).reshape(-1)
        z0 = np.array(zeta0, dtype=np.float64, copy=True).reshape(-1)
        sg = np.array(sigmaHat, dtype=np.float64, copy=True).reshape(-1)
        ca = np.array(CA, dtype=np.float64, copy=True).reshape(-1)
        if (nb < 1 or al.shape != (nb, self.H) or b0.shape != (nb, self.H) or et.shape != (nb,) or z0.shape != (nb,)
                or sg.shape != (nb,) or ca.shape != (self.M * self.H,)):
            raise ValueError(f"col_off describes {nb} bags: alpha, beta0 must be ({nb}, {self.H}), eta, zeta0, sigmaHat ({nb},) "
                             f"and CA ({self.M * self.H},)")
        MH = self.M * self.H
        zeta, beta, dS, A = np.empty(nb), np.empty(MH), np.empty(MH), np.empty(MH)
        SA = np.empty((nb, self.H, self.H))
        self._chk(self._lib.vbmf_sparse_run_fixed_basis_batched(self._h, nb, off.ctypes.data_as(C.POINTER(C.c_int64)), int(niter),
                                                                int(bool(full_cov)), _dptr(al), _dptr(b0), _dptr(et), _dptr(z0),
                                                                _dptr(sg), _dptr(ca), _dptr(zeta), _dptr(beta), _dptr(dS), _dptr(SA),
                                                                _dptr(A)))
        return dict(sigmaHat=sg, zeta=zeta, CA=ca, beta=beta, diagSigmaATVec=dS, ATVecHat=A, SigmaA=SA)

    def sparse_fit_batched(self, col_off, fit_bag, niter, eps, gamma, delta0, eta, zeta0, priors4, BHat, SigmaB, CB, sigmaHat, CA,
                           H0=None, full_cov=False, est_cb=True, est_priors=False, want_trace=False):
        """Many independent vbmf_sparse! / vbmf_dual! fits in one launch (vbmf_sparse_fit_batched): fit f works on bag fit_bag[f] of the
        bags side by side in this context's Y (bag b = columns col_off[b] .. col_off[b+1]-1).  Per fit: gamma, delta0, eta, zeta0,
        sigmaHat (nfits,), priors4 (nfits, 4) = alpha00, beta00, alpha01, beta01 (the sparse model: its pair twice, H0 = H), the start
        values BHat (nfits, L, H), SigmaB (nfits, H, H), CB (nfits, H) and CA: the fits' vec(A')-ordered vectors concatenated.
        Returns dict(BHat, SigmaB, CB, delta (None unless est_cb), sigmaHat, zeta, priors4, CA, beta, diagSigmaATVec, ATVecHat, SigmaA,
        iters, d, status, trace (nfits, niter, 2) or None).  Neither the context's state nor its Y is changed."""
        return self._ard_fit_batched(col_off, fit_bag, niter, eps, gamma, delta0, eta, zeta0, priors4, BHat, SigmaB, CB, sigmaHat, CA, H0,
                                     full_cov, est_cb, est_priors, want_trace)

    def local_fit_batched(self, col_off, fit_bag, niter, eps, gamma, delta0, eta, zeta0, priors9, BHat, SigmaB, CB, sigmaHat, CA, M0,
                          H0=None, mask_H1=0, full_cov=False, est_cb=True, est_priors=False, want_trace=False):
        """Many independent three-group (vbmf_trial!) or label-masked sparse (train_local) fits in one launch (vbmf_local_fit_batched): as
        sparse_fit_batched, with M0 (nfits,) the leading columns of each fit's bag that are its negative instances.  Entry (m, h) of A takes
        the prior pair of group 1 if h < H0, of group 2 if m < M0[f], else of group 3; with mask_H1 > 0 (H0 = H, est_priors off) the
        entries m < M0[f], h >= H - mask_H1 of A are held at zero.  priors9 (nfits, 9) in trial_get_priors' order: three (alpha0g, beta0g)
        pairs in, the pairs and the three posterior shapes out; (nfits, 6) is accepted and padded.  Returns sparse_fit_batched's dict with
        priors9 in place of priors4."""
        return self._ard_fit_batched(col_off, fit_bag, niter, eps, gamma, delta0, eta, zeta0, priors9, BHat, SigmaB, CB, sigmaHat, CA, H0,
                                     full_cov, est_cb, est_priors, want_trace, M0=M0, mask_H1=mask_H1)

    def rows_fit_batched(self, col_off, fit_bag, niter, eps, gamma, delta0, etaVec, zeta0, priors9, BHat, SigmaB, CB, sigmaVecHat, CA,
                         M0=None, H0=None, mask_H1=0, full_cov=False, est_cb=True, est_priors=False, want_trace=False):
        """local_fit_batched under the heteroscedastic noise model, diag_var = true (vbmf_rows_fit_batched; examples/mil_util.jl:667): one
        noise precision per row of Y.  etaVec (nfits,) = eta0 + M_b / 2; sigmaVecHat (nfits, L) the start values; M0 None: M0[f] = M_b, the
        two-group model (with H0 = H and est_priors off: the sparse one).  The diagonal form of updateA! takes the rows' precisions
        SQUARED into v (src/vbmf_sparse.jl:211), full_cov to the first power (:180-182).  Returns local_fit_batched's dict with
        sigmaVecHat (nfits, L) and zetaVec (nfits, L) in place of sigmaHat and zeta; the second trace column is mean(sigmaVecHat).  The
        context may be a `*_DIAG` or a `*_DIAGVAR` one: only its Y is used."""
        return self._ard_fit_batched(col_off, fit_bag, niter, eps, gamma, delta0, etaVec, zeta0, priors9, BHat, SigmaB, CB, sigmaVecHat, CA,
                                     H0, full_cov, est_cb, est_priors, want_trace, M0=M0, mask_H1=mask_H1, rows=True)

    def ard_fit_batched_form(self, col_off, fit_bag, niter, eps, gamma, delta0, etaVec, zeta0, priors9, BHat, SigmaB, CB, sigmaVecHat, CA,
                             M0=None, H0=None, mask_H1=0, full_cov=False, est_cb=True, est_priors=False, want_trace=False,
                             diag_var=False, form="split", slice_cols=None):
        """local_fit_batched (diag_var False: etaVec and sigmaVecHat are its per-fit scalars eta and sigmaHat; M0 None: M0[f] = M_b) or
        rows_fit_batched (diag_var True) with the form chosen by the caller (vbmf_ard_fit_batched_form): "stream" = one workgroup per
        fit, bit-identical to those calls; "split" = every fit over ceil(M_b / slice_cols) workgroups, two launches per sweep; "auto" =
        ard_fit_form_auto per fit.  slice_cols None: VBMF_FIT_SPLIT_COLS.  Returns their dict with form_used (nfits,): 0 / 3."""
        return self._ard_fit_batched(col_off, fit_bag, niter, eps, gamma, delta0, etaVec, zeta0, priors9, BHat, SigmaB, CB, sigmaVecHat, CA,
                                     H0, full_cov, est_cb, est_priors, want_trace, M0=M0, mask_H1=mask_H1, rows=bool(diag_var),
                                     form=(ard_fit_form_code(form), ard_slice_cols(slice_cols)))

    def _ard_fit_batched(self, col_off, fit_bag, niter, eps, gamma, delta0, eta, zeta0, priors, BHat, SigmaB, CB, sigmaHat, CA, H0, full_cov,
                         est_cb, est_priors, want_trace, M0=None, mask_H1=0, rows=False, form=None):
        """sparse_fit_batched (M0 is None: vbmf_sparse_fit_batched, four prior values per fit), local_fit_batched
        (vbmf_local_fit_batched: M0 and mask_H1 behind H0, nine prior values per fit, six accepted and padded) and rows_fit_batched
        (vbmf_rows_fit_batched: local_fit_batched's arguments with sigmaHat and zeta (nfits, L); M0 None goes down as NULL)."""
        local = M0 is not None or rows or form is not None
        H = self.H
        off, fb, nb, nf, B, per_fit, tail = self._fit_prologue(col_off, fit_bag, niter, BHat, want_trace)
        vec = lambda v: np.array(v, dtype=np.float64, copy=True).reshape(-1)
        ga, d0, et, z0, ca = vec(gamma), vec(delta0), vec(eta), vec(zeta0), vec(CA)
        sg = np.array(sigmaHat, dtype=np.float64, copy=True, order="C") if rows else vec(sigmaHat)
        if local:
            m0 = None if M0 is None else np.array(M0, dtype=np.int64, copy=True).reshape(-1)
            pin = np.asarray(priors, dtype=np.float64)
            if not (pin.ndim == 2 and pin.shape[0] == nf and pin.shape[1] in (6, 9)):
                raise ValueError(f"{nf} fits: priors9 must be ({nf}, 9) or ({nf}, 6)")
            pri = np.zeros((nf, 9))
            pri[:, :pin.shape[1]] = pin
        else:
            pri = np.array(priors, dtype=np.float64, copy=True, order="C")
        SB = np.array(SigmaB, dtype=np.float64, copy=True, order="C")
        cb = np.array(CB, dtype=np.float64, copy=True, order="C")
        MH = int(np.sum(off[fb + 1] - off[fb])) * H
        scalars = (ga, d0, et, z0) + (() if rows else (sg,)) + ((m0,) if local and m0 is not None else ())
        if (any(v.shape != (nf,) for v in scalars) or pri.shape != (nf, 9 if local else 4) or SB.shape != (nf, H, H) or cb.shape != (nf, H)
                or ca.shape != (MH,) or (rows and sg.shape != (nf, self.L))):
            if rows:
                raise ValueError(f"{nf} fits: gamma, delta0, etaVec, zeta0{'' if m0 is None else ', M0'} must be ({nf},), sigmaVecHat "
                                 f"({nf}, {self.L}), SigmaB ({nf}, {H}, {H}), CB ({nf}, {H}) and CA ({MH},)")
            raise ValueError(f"{nf} fits: gamma, delta0, eta, zeta0, sigmaHat{', M0' if local else ''} must be ({nf},), "
                             f"{'' if local else f'priors4 ({nf}, 4), '}SigmaB ({nf}, {H}, {H}), CB ({nf}, {H}) and CA ({MH},)")
        delta = np.empty((nf, H)) if est_cb else None
        zeta, beta, dS, A = np.empty((nf, self.L) if rows else nf), np.empty(MH), np.empty(MH), np.empty(MH)
        SA = np.empty((nf, H, H))
        entry = (self._lib.vbmf_ard_fit_batched_form if form is not None else self._lib.vbmf_rows_fit_batched if rows
                 else self._lib.vbmf_local_fit_batched if local else self._lib.vbmf_sparse_fit_batched)
        used = np.zeros(nf, dtype=np.int64)
        if form is not None:
            tail = tail + (int(rows), int(form[0]), int(form[1]), _i64ptr(used))
        self._chk(entry(
            self._h, nb, _i64ptr(off), nf, _i64ptr(fb), int(niter), float(eps), int(bool(full_cov)), int(bool(est_cb)), int(bool(est_priors)),
            int(H if H0 is None else H0), *((_i64ptr(m0), int(mask_H1)) if local else ()), _dptr(ga), _dptr(d0), _dptr(et), _dptr(z0),
            _dptr(pri), _dptr(B), _dptr(SB), _dptr(cb), _dptr(sg), _dptr(ca), _dptr(delta), _dptr(zeta), _dptr(beta), _dptr(dS), _dptr(SA),
            _dptr(A), *tail))
        noise = dict(sigmaVecHat=sg, zetaVec=zeta) if rows else dict(sigmaHat=sg, zeta=zeta)
        return dict(BHat=B.transpose(0, 2, 1), SigmaB=SB, CB=cb, delta=delta, **noise, CA=ca, beta=beta, diagSigmaATVec=dS,
                    ATVecHat=A, SigmaA=SA, **{"priors9" if local else "priors4": pri}, **per_fit,
                    **(dict(form_used=used) if form is not None else {}))

    def YHat(self):
        out = np.empty((self.L, self.M), order="F")
        self._chk(self._lib.vbmf_get_YHat(self._h, _dptr(out), self.L))
        return out

    def _block(self, dst, row0, nrows, rows_total, ncols):
        shape = tuple(dst.shape) if hasattr(dst, "shape") else ()
        if len(shape) != 2:
            raise ValueError("the output must be a matrix")
        n = shape[0] if nrows is None else int(nrows)
        if shape != (n, ncols):
            raise ValueError(f"expected an output of shape ({n}, {ncols}), got {shape}")
        if row0 < 0 or n < 1 or row0 + n > rows_total:
            raise ValueError(f"rows [{row0}, {row0 + n}) do not lie in a matrix of {rows_total} rows")
        return n

    def YHat_into(self, dst, row0=0, nrows=None, residual=False):
        """Rows [row0, row0 + nrows) of BHat*AHat' -- or, residual=True, of Y as stored minus it -- written into `dst` as it lies
        (vbmf_get_YHat_rows): a writable float64 / float32 NumPy array or a torch tensor (float64, float32, bfloat16; CPU or this
        context's GPU), see y_sink.  nrows defaults to dst's rows.  Returns dst."""
        n = self._block(dst, row0, nrows, self.L, self.M)
        keep, addr, code, on_dev, rs, cs, finish = y_sink(dst, self.device)
        self._chk(self._lib.vbmf_get_YHat_rows(self._h, VBMF_OUT_RESIDUAL if residual else VBMF_OUT_YHAT, addr, code, on_dev, int(row0), n,
                                               rs, cs))
        if finish is not None:
            finish()
        del keep
        return dst

    def factor_into(self, which, dst, row0=0, nrows=None):
        """Rows [row0, row0 + nrows) of AHat (which = "A" / VBMF_FACTOR_A: M x H) or of this rank's BHat ("B" / VBMF_FACTOR_B: L x H),
        the fp32 values get_state returns, written into `dst` as it lies (vbmf_get_factor_rows; dst as for YHat_into).  Returns dst."""
        w = {"A": VBMF_FACTOR_A, "B": VBMF_FACTOR_B}.get(which, which)
        if w not in (VBMF_FACTOR_A, VBMF_FACTOR_B):
            raise ValueError(f"which = {which!r} ('A' or 'B')")
        n = self._block(dst, row0, nrows, self.M if w == VBMF_FACTOR_A else self.L, self.H)
        keep, addr, code, on_dev, rs, cs, finish = y_sink(dst, self.device)
        self._chk(self._lib.vbmf_get_factor_rows(self._h, w, addr, code, on_dev, int(row0), n, rs, cs))
        if finish is not None:
            finish()
        del keep
        return dst

    def elbo(self):
        v = C.c_double()
        self._chk(self._lib.vbmf_elbo(self._h, C.byref(v)))
        return v.value

    # ---- ARD-sparse variant (variant=VBMF_VARIANT_SPARSE_DIAG) ----
    def sparse_set_state(self, ATVecHat, diagSigmaATVec, CA, beta, BHat, SigmaB, CB, delta, sigmaHat, zeta, hyper,
                         labels0=(), H1=0):
        n = self.M * self.H
        vecs = [np.ascontiguousarray(v, dtype=np.float64) for v in (ATVecHat, diagSigmaATVec, CA, beta)]
        for v in vecs:
            if v.shape != (n,):
                raise ValueError("vec(A')-shaped arguments must have length M*H")
        B = _fcol(BHat, (self.L, self.H)); SB = _fcol(SigmaB, (self.H, self.H))
        cb = np.ascontiguousarray(CB, dtype=np.float64); dl = np.ascontiguousarray(delta, dtype=np.float64)
        hp = VbmfSparseHyper(*[float(hyper[k]) for k in ("alpha0", "beta0", "gamma0", "delta0", "eta0", "zeta0")])
        lab = np.ascontiguousarray(labels0, dtype=np.int64)
        self._chk(self._lib.vbmf_sparse_set_state(self._h, _dptr(vecs[0]), _dptr(vecs[1]), _dptr(vecs[2]), _dptr(vecs[3]),
                                                  _dptr(B), self.L, _dptr(SB), _dptr(cb), _dptr(dl), float(sigmaHat),
                                                  float(zeta), C.byref(hp), lab.ctypes.data_as(C.POINTER(C.c_int64)),
                                                  lab.size, int(H1)))

    def sparse_get_state(self, want_B=True):
        n = self.M * self.H
        a, ds, ca, be = (np.empty(n) for _ in range(4))
        sa = np.empty(self.H); B = np.empty((self.L, self.H), order="F") if want_B else None
        SB = np.empty((self.H, self.H), order="F"); cb = np.empty(self.H); dl = np.empty(self.H)
        sh, ze = C.c_double(), C.c_double()
        self._chk(self._lib.vbmf_sparse_get_state(self._h, _dptr(a), _dptr(ds), _dptr(ca), _dptr(be), _dptr(sa), _dptr(B),
                                                  self.L, _dptr(SB), _dptr(cb), _dptr(dl), C.byref(sh), C.byref(ze)))
        return dict(ATVecHat=a, diagSigmaATVec=ds, CA=ca, beta=be, SigmaA_diag=sa, BHat=B, SigmaB=SB, CB=cb, delta=dl,
                    sigmaHat=sh.value, zeta=ze.value)

    def sparse_step(self, which):
        self._chk(self._lib.vbmf_sparse_step(self._h, which))

    def sparse_run(self, niter, eps=1e-6, est_cb=True, want_trace=False):
        it = C.c_int64(); d = C.c_double()
        tr = np.zeros((max(niter, 1), 4)) if want_trace else None
        self._chk(self._lib.vbmf_sparse_run(self._h, niter, eps, int(est_cb), C.byref(it), C.byref(d), _dptr(tr)))
        self._warn_note()
        return it.value, d.value, (tr[:it.value] if want_trace else None)

    def sparse_set_noise_rows(self, sigmaVecHat, zetaVec, etaVec):
        s = np.ascontiguousarray(sigmaVecHat, dtype=np.float64); z = np.ascontiguousarray(zetaVec, dtype=np.float64)
        if s.shape != (self.L,) or z.shape != (self.L,):
            raise ValueError("sigmaVecHat and zetaVec must have length L")
        self._chk(self._lib.vbmf_sparse_set_noise_rows(self._h, _dptr(s), _dptr(z), float(etaVec)))

    def sparse_get_noise_rows(self):
        s, z = np.empty(self.L), np.empty(self.L)
        self._chk(self._lib.vbmf_sparse_get_noise_rows(self._h, _dptr(s), _dptr(z)))
        return s, z

    def sparse_set_full_cov(self, on=True):
        self._chk(self._lib.vbmf_sparse_set_full_cov(self._h, int(bool(on))))

    def set_gram_form(self, mode):
        """VBMF_GRAM_FORM_DEFAULT / _OFF / _ON (vbmf_set_gram_form): which form the run loops take; dims()["gram"] reports the outcome."""
        self._chk(self._lib.vbmf_set_gram_form(self._h, int(mode)))

    def sparse_set_SigmaA(self, SigmaA):
        S = _fcol(SigmaA, (self.H, self.H))
        self._chk(self._lib.vbmf_sparse_set_SigmaA(self._h, _dptr(S)))

    def sparse_get_SigmaA(self):
        S = np.empty((self.H, self.H), order="F")
        self._chk(self._lib.vbmf_sparse_get_SigmaA(self._h, _dptr(S)))
        return S

    def sparse_lower_bound(self, clamp=True):
        v = C.c_double()
        self._chk(self._lib.vbmf_sparse_lower_bound(self._h, int(clamp), C.byref(v)))
        return v.value

    def sparse_lower_bound_trimmed(self, trim=1e-1, clamp=True):
        v = C.c_double()
        self._chk(self._lib.vbmf_sparse_lower_bound_trimmed(self._h, int(clamp), float(trim), C.byref(v)))
        return v.value

    # ---- per-bag scoring of the bags side by side in this context's Y ----
    def bag_residuals(self, col_off, AHat):
        """||Y_b - BHat AHat_b'||_F^2 of every bag (vbmf_bag_residuals): bag b = columns col_off[b] .. col_off[b+1]-1, BHat from
        set_state / sparse_set_state, AHat (M, H) the bags' rows stacked.  Returns r2 (nbags,).  The state is not changed."""
        off = np.ascontiguousarray(col_off, dtype=np.int64)
        nb = off.size - 1
        A = _fcol(AHat, (self.M, self.H))
        r2 = np.empty(max(nb, 0))
        self._chk(self._lib.vbmf_bag_residuals(self._h, nb, off.ctypes.data_as(C.POINTER(C.c_int64)), _dptr(A), self.M, _dptr(r2)))
        return r2

    def bag_least_squares(self, col_off, BHat, lam=0.0, want_X=True, want_r2=True):
        """inv(BHat'BHat + lam I) BHat' Y_b and ||Y_b - BHat X_b||_F^2 of every bag (vbmf_bag_least_squares): bag b = columns
        col_off[b] .. col_off[b+1]-1, BHat (L, H) the caller's fp64 basis with its own H <= 64 (not this context's; no state is read).
        Returns (X (H, M) or None, r2 (nbags,) or None).  The state is not changed."""
        off = np.ascontiguousarray(col_off, dtype=np.int64)
        nb = off.size - 1
        B = _fcol(BHat)
        if B.ndim != 2 or B.shape[0] != self.L:
            raise ValueError(f"BHat must be ({self.L}, H), got {B.shape}")
        H = B.shape[1]
        X = np.empty((H, self.M), order="F") if want_X else None
        r2 = np.empty(max(nb, 0)) if want_r2 else None
        self._chk(self._lib.vbmf_bag_least_squares(self._h, nb, off.ctypes.data_as(C.POINTER(C.c_int64)), _dptr(B), self.L, H, float(lam),
                                                   _dptr(X), H, _dptr(r2)))
        return X, r2

    def bag_least_squares_jobs(self, col_off, bases, lams, job_bag, job_basis, want_X=False, want_r2=True):
        """Many bases and a list of (bag, basis) jobs in one device call (vbmf_bag_least_squares_jobs): bases[k] (L, H_k) fp64 with its
        own H_k <= 64 and lams[k] its lambda, job j scores bag job_bag[j] of col_off against basis job_basis[j].  Returns (Xs, r2,
        status): Xs a list of (H_k, M_b) arrays per job or None, r2 (njobs,) or None, status (nbasis,) with 1 for a basis whose
        B'B + lam I is not positive definite (its jobs are NaN, the others are computed).  Every job is bit for bit what
        bag_least_squares gives for that bag with that basis and lambda.  The state is not changed."""
        off = np.ascontiguousarray(col_off, dtype=np.int64)
        nb = off.size - 1
        Bs = [_fcol(B) for B in bases]
        for B in Bs:
            if B.ndim != 2 or B.shape[0] != self.L:
                raise ValueError(f"every basis must be ({self.L}, H), got {B.shape}")
        lam = np.ascontiguousarray(lams, dtype=np.float64).reshape(-1)
        jb = np.ascontiguousarray(job_bag, dtype=np.int64).reshape(-1)
        jk = np.ascontiguousarray(job_basis, dtype=np.int64).reshape(-1)
        if lam.size != len(Bs) or jb.size != jk.size:
            raise ValueError(f"{len(Bs)} bases but {lam.size} lambdas, or {jb.size} job bags but {jk.size} job bases")
        Hs = np.array([B.shape[1] for B in Bs], dtype=np.int64)
        Ball = np.concatenate([B.reshape(-1, order="F") for B in Bs]) if Bs else np.empty(0)
        X = shapes = None
        if want_X:                                                   # (a job out of range is the library's to refuse: no block for it)
            ok = (jb >= 0) & (jb < nb) & (jk >= 0) & (jk < len(Bs))
            shapes = [(int(Hs[k]), int(off[b + 1] - off[b])) if g else (0, 0) for b, k, g in zip(jb, jk, ok)]
            xoff = np.concatenate([[0], np.cumsum([h * m for h, m in shapes])]).astype(np.int64)
            X = np.empty(max(int(xoff[-1]), 1))
        r2 = np.empty(jb.size) if want_r2 else None
        status = np.zeros(len(Bs), dtype=np.int64)
        self._chk(self._lib.vbmf_bag_least_squares_jobs(self._h, nb, _i64ptr(off), len(Bs), _i64ptr(Hs), _dptr(Ball), _dptr(lam), jb.size,
                                                        _i64ptr(jb), _i64ptr(jk), _dptr(X), _dptr(r2), _i64ptr(status)))
        Xs = None
        if want_X:
            Xs = [X[xoff[j]:xoff[j + 1]].reshape(shapes[j], order="F") for j in range(jb.size)]
        return Xs, r2, status

    def sparse_fixed_basis_jobs(self, col_off, H, models, job_bag, job_model, niter, full_cov=False):
        """vbls! of the ARD families for a list of (bag, model) jobs in one device call (vbmf_sparse_fixed_basis_jobs): models[k] is a
        dict of BHat (L, H) and SigmaB (H, H) fp64, alpha and beta0 (H,), eta0, zeta0, sigma0, ca0 (scalars), all of the one H <= 32;
        job j runs bag job_bag[j] of col_off against model job_model[j] for niter iterations from sigmaHat = sigma0, CA = ca0.  Only
        this context's Y is read.  Returns dict(r2, sigmaHat, zeta (njobs,), status (njobs,) with 1 for a failed job (NaN in its
        outputs, the others are computed), SigmaA (njobs, H, H), CA, beta, diagSigmaATVec, ATVecHat: the jobs' M_b*H-long blocks in
        vec(A') order one after the other, and off (njobs + 1,): job j's block is [off[j] : off[j + 1]])."""
        off = np.ascontiguousarray(col_off, dtype=np.int64)
        nb = off.size - 1
        H = int(H)
        nk = len(models)
        for m in models:
            if np.shape(m["BHat"]) != (self.L, H) or np.shape(m["SigmaB"]) != (H, H) or np.size(m["alpha"]) != H or np.size(m["beta0"]) != H:
                raise ValueError(f"every model needs BHat ({self.L}, {H}), SigmaB ({H}, {H}), alpha and beta0 ({H},)")
        per_model = [_pack_models(models, "BHat", "F"), _pack_models(models, "SigmaB", "F")] + [_pack_models(models, f) for f in (
            "alpha", "beta0", "eta0", "zeta0", "sigma0", "ca0")]
        jb = np.ascontiguousarray(job_bag, dtype=np.int64).reshape(-1)
        jk = np.ascontiguousarray(job_model, dtype=np.int64).reshape(-1)
        if jb.size != jk.size:
            raise ValueError(f"{jb.size} job bags but {jk.size} job models")
        nj = jb.size
        boff = _job_blocks(off, nb, jb, jk, H, 1)[3]
        n = max(int(boff[-1]), 1)
        r2, sg, zeta = np.empty(nj), np.empty(nj), np.empty(nj)
        A, dS, CA, beta = np.empty(n), np.empty(n), np.empty(n), np.empty(n)
        SA = np.empty((nj, H, H))
        status = np.zeros(nj, dtype=np.int64)
        self._chk(self._lib.vbmf_sparse_fixed_basis_jobs(self._h, nb, _i64ptr(off), H, int(niter), int(bool(full_cov)), nk,
                                                         *[_dptr(v) for v in per_model], nj, _i64ptr(jb), _i64ptr(jk), _dptr(r2), _dptr(A),
                                                         _dptr(dS), _dptr(CA), _dptr(beta), _dptr(SA), _dptr(sg), _dptr(zeta), _i64ptr(status)))
        return dict(r2=r2, sigmaHat=sg, zeta=zeta, status=status, SigmaA=SA, CA=CA, beta=beta, diagSigmaATVec=dS, ATVecHat=A, off=boff)

    def fixed_basis_jobs(self, col_off, models, job_bag, job_model, niter):
        """vbls! of the basic model for a list of (bag, model) jobs in one device call (vbmf_fixed_basis_jobs): models[k] is a dict of
        BHat (L, H_k) and SigmaB (H_k, H_k) fp64, sigma2_0 and ca0 (scalars), each model of its own H_k <= 32; job j runs bag job_bag[j]
        of col_off against model job_model[j] for niter iterations from sigma2 = sigma2_0, CA = ca0 I.  Only this context's Y is read.
        Returns dict(r2, sigma2 (njobs,), status (njobs,) with 1 for a failed job (NaN in its outputs, the others are computed), and
        the lists AHat (M_b, H_k), SigmaA (H_k, H_k), CA (H_k,) per job)."""
        off = np.ascontiguousarray(col_off, dtype=np.int64)
        nb = off.size - 1
        nk = len(models)
        Hs = np.array([np.shape(m["BHat"])[1] if np.ndim(m["BHat"]) == 2 else -1 for m in models], dtype=np.int64)
        for m, H in zip(models, Hs):
            H = int(H)
            if np.shape(m["BHat"]) != (self.L, H) or np.shape(m["SigmaB"]) != (H, H):
                raise ValueError(f"every model needs BHat ({self.L}, H) and SigmaB (H, H)")
        B, SB, s0, c0 = _pack_models(models, "BHat", "F"), _pack_models(models, "SigmaB", "F"), _pack_models(models, "sigma2_0"), _pack_models(models, "ca0")
        jb = np.ascontiguousarray(job_bag, dtype=np.int64).reshape(-1)
        jk = np.ascontiguousarray(job_model, dtype=np.int64).reshape(-1)
        nj = jb.size
        if jk.size != nj:
            raise ValueError(f"{nj} job bags but {jk.size} job models")
        _, Hj, widths, boff, soff, hoff = _job_blocks(off, nb, jb, jk, Hs)
        r2, sg = np.empty(nj), np.empty(nj)
        A, SA, CA = np.empty(max(int(boff[-1]), 1)), np.empty(max(int(soff[-1]), 1)), np.empty(max(int(hoff[-1]), 1))
        status = np.zeros(nj, dtype=np.int64)
        self._chk(self._lib.vbmf_fixed_basis_jobs(self._h, nb, _i64ptr(off), int(niter), nk, _i64ptr(Hs), _dptr(B), _dptr(SB), _dptr(s0),
                                                  _dptr(c0), nj, _i64ptr(jb), _i64ptr(jk), _dptr(r2), _dptr(A), _dptr(SA), _dptr(CA),
                                                  _dptr(sg), _i64ptr(status)))
        As = [A[boff[j]:boff[j + 1]].reshape((int(widths[j]), int(Hj[j])), order="F") for j in range(nj)]
        SAs = [SA[soff[j]:soff[j + 1]].reshape(int(Hj[j]), int(Hj[j])) for j in range(nj)]
        CAs = [CA[hoff[j]:hoff[j + 1]] for j in range(nj)]
        return dict(r2=r2, sigma2=sg, status=status, AHat=As, SigmaA=SAs, CA=CAs)

    def sparse_scored_jobs(self, col_off, models, job_bag, job_model, job_full_cov, job_trim, niter, clamp=True, grouped=False):
        """factorize_bag and its scores for a list of (bag, model) jobs in one device call (vbmf_sparse_scored_jobs): models[k] is a dict
        of BHat (L, H_k) and SigmaB (H_k, H_k) fp64, CB, delta, a_pri, b_pri, a_post (H_k,), gamma, gamma0, delta0, eta0, zeta0, sigma0,
        ca0 (scalars), each model of its own H_k <= 32; job j runs bag job_bag[j] against model job_model[j] for niter iterations in
        the diagonal (job_full_cov[j] = 0) or the full_cov form, and scores it with lowerBound (job_trim[j] < 0 or None) or
        lowerBoundTrimmed(job_trim[j]).  Only this context's Y is read.  Returns what sparse_fixed_basis_jobs returns plus lb (njobs,);
        SigmaA is a list of (H_k, H_k) arrays, and status is 1 also for a job whose bound is not finite."""
        off = np.ascontiguousarray(col_off, dtype=np.int64)
        nb = off.size - 1
        nk = len(models)
        Hs = np.array([np.shape(m["BHat"])[1] if np.ndim(m["BHat"]) == 2 else -1 for m in models], dtype=np.int64)
        for m, H in zip(models, Hs):
            H = int(H)
            if (np.shape(m["BHat"]) != (self.L, H) or np.shape(m["SigmaB"]) != (H, H)
                    or any(np.size(m[f]) != H for f in ("CB", "delta", "a_pri", "b_pri", "a_post"))):
                raise ValueError(f"every model needs BHat ({self.L}, H), SigmaB (H, H), CB, delta, a_pri, b_pri and a_post (H,)")
        per_model = [_pack_models(models, "BHat", "F"), _pack_models(models, "SigmaB", "F")] + [_pack_models(models, f) for f in (
            "CB", "delta", "gamma", "gamma0", "delta0", "a_pri", "b_pri", "a_post", "eta0", "zeta0", "sigma0", "ca0")]
        jb = np.ascontiguousarray(job_bag, dtype=np.int64).reshape(-1)
        jk = np.ascontiguousarray(job_model, dtype=np.int64).reshape(-1)
        jf = np.ascontiguousarray([int(bool(f)) for f in job_full_cov], dtype=np.int64).reshape(-1)
        jt = np.ascontiguousarray([-1.0 if t is None else float(t) for t in job_trim], dtype=np.float64).reshape(-1)
        nj = jb.size
        if not (jk.size == jf.size == jt.size == nj):
            raise ValueError(f"{nj} job bags but {jk.size} job models, {jf.size} forms and {jt.size} trims")
        _, Hj, _, boff, soff = _job_blocks(off, nb, jb, jk, Hs, 2)
        n = max(int(boff[-1]), 1)
        lb, r2, sg, zeta = np.empty(nj), np.empty(nj), np.empty(nj), np.empty(nj)
        A, dS, CA, beta = np.empty(n), np.empty(n), np.empty(n), np.empty(n)
        SA = np.empty(max(int(soff[-1]), 1))
        status = np.zeros(nj, dtype=np.int64)
        self._chk(self._lib.vbmf_sparse_scored_jobs(self._h, nb, _i64ptr(off), int(niter), int(bool(clamp)), int(bool(grouped)), nk, _i64ptr(Hs),
                                                    *[_dptr(v) for v in per_model], nj, _i64ptr(jb), _i64ptr(jk), _i64ptr(jf), _dptr(jt),
                                                    _dptr(lb), _dptr(r2), _dptr(A), _dptr(dS), _dptr(CA), _dptr(beta), _dptr(SA), _dptr(sg),
                                                    _dptr(zeta), _i64ptr(status)))
        SAs = [SA[soff[j]:soff[j + 1]].reshape(int(Hj[j]), int(Hj[j])) for j in range(nj)]
        return dict(lb=lb, r2=r2, sigmaHat=sg, zeta=zeta, status=status, SigmaA=SAs, CA=CA, beta=beta, diagSigmaATVec=dS, ATVecHat=A,
                    off=boff)

    def sparse_lower_bound_batched(self, col_off, ATVecHat, diagSigmaATVec, CA, beta, SigmaA, sigmaHat, zeta, eta, eta0, zeta0,
                                   a_pri, b_pri, a_post, trim=None, clamp=True, grouped=False):
        """lowerBound (trim None) / lowerBoundTrimmed of every bag (vbmf_sparse_lower_bound_batched): BHat, SigmaB, CB, delta, gamma0,
        delta0 from sparse_set_state; ATVecHat, diagSigmaATVec, CA, beta (M*H,) in vec(A') order; SigmaA (nbags, H, H); sigmaHat, zeta,
        eta, eta0, zeta0 (nbags,); a_pri, b_pri, a_post (nbags, H): per column of A the ARD hyper-prior (shape, rate) and posterior
        shape.  grouped: the dual / trial models' trimming rule.  Returns (lb, r2), each (nbags,).  The state is not changed."""
        off = np.ascontiguousarray(col_off, dtype=np.int64)
        nb = off.size - 1
        MH = self.M * self.H
        vecs = [np.ascontiguousarray(v, dtype=np.float64).reshape(-1) for v in (ATVecHat, diagSigmaATVec, CA, beta)]
        SA = np.ascontiguousarray(SigmaA, dtype=np.float64)
        per_bag = [np.ascontiguousarray(v, dtype=np.float64).reshape(-1) for v in (sigmaHat, zeta, eta, eta0, zeta0)]
        per_col = [np.ascontiguousarray(v, dtype=np.float64) for v in (a_pri, b_pri, a_post)]
        if (nb < 1 or any(v.shape != (MH,) for v in vecs) or SA.shape != (nb, self.H, self.H)
                or any(v.shape != (nb,) for v in per_bag) or any(v.shape != (nb, self.H) for v in per_col)):
            raise ValueError(f"col_off describes {nb} bags: the vec(A') fields must be ({MH},), SigmaA ({nb}, {self.H}, {self.H}), "
                             f"the per-bag scalars ({nb},) and a_pri, b_pri, a_post ({nb}, {self.H})")
        lb, r2 = np.empty(nb), np.empty(nb)
        self._chk(self._lib.vbmf_sparse_lower_bound_batched(
            self._h, nb, off.ctypes.data_as(C.POINTER(C.c_int64)), int(clamp), -1.0 if trim is None else float(trim), int(bool(grouped)),
            *[_dptr(v) for v in vecs], _dptr(SA), *[_dptr(v) for v in per_bag], *[_dptr(v) for v in per_col], _dptr(lb), _dptr(r2)))
        return lb, r2

    # ---- two-group ARD variant (variant=VBMF_VARIANT_DUAL_DIAG) ----
    def dual_set_priors(self, H0, alpha00, beta00, alpha01, beta01, alpha0=None, alpha1=None):
        alpha0 = alpha00 + 0.5 if alpha0 is None else alpha0
        alpha1 = alpha01 + 0.5 if alpha1 is None else alpha1
        self._chk(self._lib.vbmf_dual_set_priors(self._h, int(H0), float(alpha00), float(beta00), float(alpha01), float(beta01),
                                                 float(alpha0), float(alpha1)))

    def dual_get_priors(self):
        h0 = C.c_int64(); v = np.empty(6)
        self._chk(self._lib.vbmf_dual_get_priors(self._h, C.byref(h0), _dptr(v)))
        return h0.value, dict(alpha00=v[0], beta00=v[1], alpha01=v[2], beta01=v[3], alpha0=v[4], alpha1=v[5])

    def dual_run(self, niter, eps=1e-6, est_cb=True, est_priors=True, want_trace=False):
        it = C.c_int64(); d = C.c_double()
        tr = np.zeros((max(niter, 1), 4)) if want_trace else None
        self._chk(self._lib.vbmf_dual_run(self._h, niter, eps, int(est_cb), int(est_priors), C.byref(it), C.byref(d), _dptr(tr)))
        return it.value, d.value, (tr[:it.value] if want_trace else None)

    # ---- three-group ARD variant (variant=VBMF_VARIANT_TRIAL_DIAG) ----
    TRIAL_KEYS = ("alpha01", "beta01", "alpha02", "beta02", "alpha03", "beta03", "alpha1", "alpha2", "alpha3")

    def trial_set_priors(self, H0, M0, priors):
        v = np.array([float(priors[k]) for k in self.TRIAL_KEYS])
        self._chk(self._lib.vbmf_trial_set_priors(self._h, int(H0), int(M0), _dptr(v)))

    def trial_get_priors(self):
        h0, m0 = C.c_int64(), C.c_int64(); v = np.empty(9)
        self._chk(self._lib.vbmf_trial_get_priors(self._h, C.byref(h0), C.byref(m0), _dptr(v)))
        return h0.value, m0.value, {k: float(v[i]) for i, k in enumerate(self.TRIAL_KEYS)}

    def trial_run(self, niter, eps=1e-6, est_cb=True, est_priors=True, want_trace=False):
        it = C.c_int64(); d = C.c_double()
        tr = np.zeros((max(niter, 1), 4)) if want_trace else None
        self._chk(self._lib.vbmf_trial_run(self._h, niter, eps, int(est_cb), int(est_priors), C.byref(it), C.byref(d), _dptr(tr)))
        return it.value, d.value, (tr[:it.value] if want_trace else None)

    # ---- multi-GPU ----
    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(UNIQUE_ID_BYTES)
        rc = lib().vbmf_comm_unique_id(buf)
        if rc != 0:
            raise VbmfError(rc, "ncclGetUniqueId failed")
        return bytes(buf.raw)

    def comm_init(self, uid):
        buf = C.create_string_buffer(bytes(uid), UNIQUE_ID_BYTES)
        self._chk(self._lib.vbmf_comm_init(self._h, buf))

    def comm_set_transport(self, fn):
        """Bring-up transport instead of RCCL: fn(buf_ptr, count, is_double, stream_ptr) -> 0 sums a device buffer
        over the ranks in place (see include/vbmf_hip.h).  The ctypes thunk is kept alive with the context."""
        def thunk(user, buf, count, is_double, stream):
            try:
                return int(fn(buf, count, bool(is_double), stream) or 0)
            except Exception:            # never let a Python exception unwind through the C frames
                import traceback
                traceback.print_exc()
                return 1
        self._ar_thunk = ALLREDUCE_FN(thunk)
        self._chk(self._lib.vbmf_comm_set_transport(self._h, self._ar_thunk, None))

    # ---- measurement ----
    def profile_enable(self, on=True):
        self._chk(self._lib.vbmf_profile_enable(self._h, int(on)))

    def profile_read(self, reset=True):
        out = np.zeros(8)
        self._chk(self._lib.vbmf_profile_read(self._h, _dptr(out), int(reset)))
        return dict(pass1_ms=out[0], pass1_n=int(out[1]), pass2_ms=out[2], pass2_n=int(out[3]))

    def pass_bytes(self, p):
        v = C.c_double()
        self._chk(self._lib.vbmf_pass_bytes(self._h, p, C.byref(v)))
        return v.value

    def peek(self, what, nwords, offset=0, dtype=np.uint32):
        out = np.zeros(nwords, dtype=np.uint32)
        self._chk(self._lib.vbmf_debug_peek(self._h, what, out.ctypes.data_as(C.POINTER(C.c_uint32)), nwords, offset))
        return out.view(dtype)

    def chain_us(self):
        """Last durations (microseconds) of the in-launch control chain's parts."""
        v = self.peek(PEEK_CHAIN, 16, dtype=np.uint64)
        return dict(zip(("ctrl_end", "SigmaA", "lambda_max_dB_and_loop", "SigmaB", "epilogue_table", "epilogue_tiles", "epilogue_fold"),
                        (float(x) * 0.01 for x in v)))

    def dims(self):
        v = self.peek(PEEK_DIMS, 30, dtype=np.int32)
        keys = ["Hp", "NH", "mode", "XT1", "KS1", "nsplit1", "sps1", "XT2", "KS2", "nsplit2", "sps2", "kstep", "npart", "narrow",
                "streamk_per", "streamk_grid",       # segment-list plan of the Y*A pass: pieces per cut block (0: off), segments = workgroups
                "gram", "gram_built", "gram_build_us", "gram_nsplit",   # vbmf_run takes the Gram form; G built; its build time; split-K
                "p_frag", "q_frag", "q_epi",         # the last pass 1 / pass 2 product is fragment-major; the last pass 2 ran the register epilogue
                "lds8", "xcd_map", "post3",          # variant switches as the context resolved them (VBMF_LDS8, VBMF_XCD_MAP, VBMF_POST3)
                "sparse_a_fused",                    # the ARD-sparse A update writes its operand tiles itself (VBMF_SPARSE_A_FUSED)
                "set_y_rows_us",                     # device time of the last vbmf_set_Y_rows call (HIP events: staged copies, tiling, ||Y||^2)
                "b_pending", "b_materialised"]       # B of the last Gram-form run is still owed; how often it has been made on demand
        return dict(zip(keys, (int(x) for x in v)))

    def out_rows_us(self):
        """Device time (microseconds) of the last vbmf_get_YHat_rows / vbmf_get_factor_rows call between two HIP events on the context's
        stream: kernels and staged copies (word 30 of VBMF_PEEK_DIMS; dims() keeps its 30 keys)."""
        return int(self.peek(PEEK_DIMS, 31, dtype=np.int32)[30])

    def time_pass(self, p, iters=10):
        v = C.c_double()
        self._chk(self._lib.vbmf_debug_time_pass(self._h, p, iters, C.byref(v)))
        return v.value

    def lambda_max(self, G):
        """lambda_max of the symmetric PSD H x H matrix G by the device kernel the run loop uses for this rank; (value, kernel us)."""
        G = np.asfortranarray(G, dtype=np.float64)
        assert G.shape == (self.H, self.H)
        v, us = C.c_double(), C.c_double()
        self._chk(self._lib.vbmf_debug_lambda_max(self._h, _dptr(G), C.byref(v), C.byref(us)))
        return v.value, us.value

    def sync(self):
        self._chk(self._lib.vbmf_device_sync(self._h))

    def debug_set(self, what, value):
        self._chk(self._lib.vbmf_debug_set(self._h, int(what), int(value)))


def blk_sweep(K, waves=4):
    """The blocked LDS inverse of the H x H covariance updates on one 256-thread workgroup (vbmf_debug_blk_sweep): K symmetric of order
    H <= 128, waves = 4 (the control chain's schedule) or 1 (the one-wave schedule).  Returns (image, log det K, bad): the n x n image,
    n = H rounded up to 16, whose upper 16 x 16 blocks hold -inv(K); lower blocks zero."""
    K = np.ascontiguousarray(K, dtype=np.float64)
    H = K.shape[0]
    assert K.shape == (H, H)
    n = 16 * ((H + 15) // 16)
    out = np.empty((n, n), dtype=np.float64)
    ld, bad = C.c_double(), C.c_int32()
    rc = lib().vbmf_debug_blk_sweep(_dptr(K), H, int(waves), _dptr(out), C.byref(ld), C.byref(bad))
    if rc != VBMF_OK:
        raise RuntimeError("vbmf_debug_blk_sweep failed: %d" % rc)
    return out, ld.value, bad.value


def vbls_jobs_lds_cols(H, full_cov=False):
    """The widest bag whose job keeps its state in LDS in Context.sparse_fixed_basis_jobs (vbmf_debug_vbls_jobs_lds_cols)."""
    return int(lib().vbmf_debug_vbls_jobs_lds_cols(int(H), int(bool(full_cov))))


def fixed_basis_jobs_lds_cols(H):
    """The widest bag whose job keeps its P in LDS in Context.fixed_basis_jobs (vbmf_debug_fixed_basis_jobs_lds_cols)."""
    return int(lib().vbmf_debug_fixed_basis_jobs_lds_cols(int(H)))
