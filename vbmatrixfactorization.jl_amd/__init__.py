"""MI355X-native drop-in for the VB matrix-factorization sweep of vitskvara/VBMatrixFactorization.jl.

Host-side mirror of the reference's Julia surface for this path (src/vbmf.jl), over the C ABI in
include/vbmf_hip.h (hand-written HIP kernels for gfx950).  Names follow the reference; Julia's `!`
becomes a trailing underscore:

    reference (src/vbmf.jl)                      here
    ------------------------------------------  ------------------------------
    type vbmf_parameters            :22-40       class vbmf_parameters (same field names/order)
    vbmf_init(Y, H; ca, cb, sigma2, H1, labels)  vbmf_init(...)            :48-73
    copy(params)                    :80-88       copy(params)   (shallow, like the reference)
    updateA!/updateB!               :95-113      updateA_/updateB_
    updateYHat!                     :120-122     updateYHat_
    updateCA!/updateCB!             :129-146     updateCA_/updateCB_
    updateSigma2!                   :153-157     updateSigma2_
    vbmf!(Y, params, niter; eps, est_covs, est_var, logdir, desc, verb)   vbmf_(...)   :175-231
    vbmf(Y, params_in, niter; ...)  :238-248     vbmf(...)

`labels` are 1-based row indices of AHat exactly as in the reference struct; they are converted to
0-based at the C boundary.  Arrays are float64; Y is (L, M), AHat (M, H), BHat (L, H).

There is no CPU implementation in this package: every numeric update runs in libvbmf_hip.so, and
importing/using it without that library (or without an MI355X) raises.
"""
from __future__ import annotations

import copy as _copy
import weakref
from contextlib import contextmanager
from dataclasses import dataclass, field, fields
from typing import Callable, NamedTuple, Optional

import numpy as np

from . import capi, dist
from .data_manip import create_log, update_log_, save_log, load_log, extract_params_
from .capi import PreprocessPlan
from .capi import (Context, VbmfError, VBMF_Y_F32, VBMF_Y_BF16, VBMF_FACTOR_AUTO, VBMF_FACTOR_BF16,
                   VBMF_FACTOR_BF16X2, VBMF_VARIANT_SPARSE_DIAG, VBMF_VARIANT_SPARSE_DIAGVAR, VBMF_VARIANT_DUAL_DIAG, VBMF_VARIANT_TRIAL_DIAG, VBMF_VARIANT_DUAL_DIAGVAR, VBMF_VARIANT_TRIAL_DIAGVAR, STEP_A, STEP_B, STEP_CA, STEP_CB, STEP_SIGMA2,
                   SSTEP_A, SSTEP_B, SSTEP_CA, SSTEP_CB, SSTEP_SIGMA, SSTEP_PRIORS)

__all__ = ["vbmf_parameters", "vbmf_init", "vbmf", "vbmf_", "copy", "updateA_", "updateB_", "updateCA_",
           "updateCB_", "updateSigma2_", "updateYHat_", "elbo", "Session", "set_defaults", "capi",
           "vbmf_sparse_parameters", "vbmf_sparse_init", "vbmf_sparse", "vbmf_sparse_", "lowerBound", "lowerBoundTrimmed", "invalidate",
           "sparse_updateA_", "sparse_updateB_", "sparse_updateCA_", "sparse_updateCB_", "sparse_updateSigma_",
           "vbmf_dual_parameters", "vbmf_dual_init", "vbmf_dual", "vbmf_dual_", "lowerBound_dual", "dual_updateA_",
           "dual_updateB_", "dual_updateCA_", "dual_updateCB_", "dual_updateSigma_", "dual_updateCA_and_priors_",
           "vbmf_trial_parameters", "vbmf_trial_init", "vbmf_trial", "vbmf_trial_", "lowerBound_trial", "trial_updateA_",
           "trial_updateB_", "trial_updateCA_", "trial_updateCB_", "trial_updateSigma_", "trial_updateCA_and_priors_",
           "vbls_batch_", "Bags", "vbls_sparse_batch_", "SparseBags", "vbmf_sparse_batch_", "vbmf_dual_batch_", "fit_restarts",
           "vbmf_batch_", "train_folds", "row_gram_batch", "vbmf_trial_batch_", "vbmf_sparse_masked_batch_", "train_local_folds",
           "train_dual_folds", "BagPool",
           "residual_batch", "lowerBound_batch", "lowerBoundTrimmed_batch", "classify_batch",
           "ols_batch", "rls_batch", "ls_residual_batch", "classify_bags", "test_classification_batch", "vbls_sparse_jobs_", "vbls_jobs_",
           "classify_folds", "test_classification_folds", "validate_folds", "factorize_folds", "validate_local_folds"]

# YHat (L x M float64) is materialised eagerly by the reference (src/vbmf.jl:70,217); above this many
# elements the field is left None and computed on demand with updateYHat_ (8 GB at 100k x 10k).
YHAT_AUTO_LIMIT = 1 << 24

# The reference-style functions take the caller's Array{Float64} Y; by default it is stored on the device in fp32 (exact-f32
# MFMA, 2^-24 per entry).  bf16 storage (2^-9 per entry of Y: the BASELINE headline configuration, what bench.py passes
# explicitly) is an opt-in through set_defaults(y_dtype=VBMF_Y_BF16): it changes the data the model sees, which a drop-in
# caller must choose knowingly -- sigma2 is a cancellation of ||Y||^2 against the reconstruction.
_defaults = dict(y_dtype=VBMF_Y_F32, factor_dtype=VBMF_FACTOR_AUTO, device=0)


def set_defaults(**kw):
    """Device storage of Y / MFMA operand precision used by the reference-style functions (y_dtype: VBMF_Y_F32 (default) or
    VBMF_Y_BF16; factor_dtype: VBMF_FACTOR_AUTO / _BF16 / _BF16X2 with bf16 Y)."""
    for k in kw:
        if k not in _defaults:
            raise KeyError(k)
    _defaults.update(kw)


@dataclass
class vbmf_parameters:
    """src/vbmf.jl:22-40 -- same field names, order and meaning."""
    L: int = 0
    M: int = 0
    H: int = 0
    H1: int = 0
    labels: np.ndarray = field(default_factory=lambda: np.zeros(0, dtype=np.int64))   # 1-based, as in Julia
    AHat: Optional[np.ndarray] = None
    BHat: Optional[np.ndarray] = None
    SigmaA: Optional[np.ndarray] = None
    SigmaB: Optional[np.ndarray] = None
    CA: Optional[np.ndarray] = None
    CB: Optional[np.ndarray] = None
    invCA: Optional[np.ndarray] = None
    invCB: Optional[np.ndarray] = None
    sigma2: float = 1.0
    YHat: Optional[np.ndarray] = None


def copy(params_in):
    """src/vbmf.jl:80-88 -- shallow: the new struct shares every array with params_in."""
    p = vbmf_parameters()
    for f in fields(params_in):
        setattr(p, f.name, getattr(params_in, f.name))
    return p


def _labels0(p):
    lab = np.asarray(p.labels, dtype=np.int64)
    if lab.size and (lab.min() < 1 or lab.max() > p.M):
        raise IndexError("labels must be 1-based row indices of AHat (as in the reference)")
    return lab - 1


def _shape2(Y):
    """(L, M) of a matrix: a NumPy array, anything np.asarray takes, or a torch tensor (left where it is)."""
    shape = tuple(Y.shape) if capi._is_tensor(Y) else np.asarray(Y).shape
    if len(shape) != 2:
        raise ValueError("Y must be a matrix")
    return int(shape[0]), int(shape[1])


def vbmf_init(Y, H, ca=1.0, cb=1.0, sigma2=1.0, H1=0, labels=(), rng=None, materialize_yhat=None):
    """src/vbmf.jl:48-73.  Host-side (the random draw is outside the hot path); `rng` is a
    numpy Generator standing in for Julia's global RNG."""
    L, M = _shape2(Y)                                          # the shape is all that is read of Y
    rng = np.random.default_rng() if rng is None else rng
    p = vbmf_parameters()
    p.L, p.M, p.H, p.H1 = L, M, int(H), int(H1)
    p.labels = np.asarray(labels, dtype=np.int64)
    p.AHat = rng.standard_normal((M, H))
    if p.H1 > 0 and p.labels.size:
        p.AHat[_labels0(p), H - p.H1:] = 0.0                  # :61
    p.BHat = rng.standard_normal((L, H))
    p.SigmaA = np.zeros((H, H))
    p.SigmaB = np.zeros((H, H))
    p.CA = ca * np.eye(H)
    p.CB = cb * np.eye(H)
    p.invCA = np.eye(H) / ca
    p.invCB = np.eye(H) / cb
    p.sigma2 = float(sigma2)
    if materialize_yhat is None:
        materialize_yhat = L * M <= YHAT_AUTO_LIMIT
    p.YHat = p.BHat @ p.AHat.T if materialize_yhat else None  # :70 (host: initialisation only)
    return p


class Session:
    """Device-resident problem: Y uploaded (or generated) once, state kept on the GPU between calls.

    The reference-style functions below are thin shells over a cached Session; use a Session
    directly to avoid the state round trip per call at large sizes."""

    def __init__(self, L, M, H, **ctx_kw):
        kw = dict(_defaults)
        kw.update(ctx_kw)
        self.ctx = Context(L, M, H, **kw)
        self.L, self.M, self.H = L, M, H

    # -- data --
    def set_Y(self, Y):
        """The whole matrix.  A float64 NumPy array (or anything that is not an array or tensor: converted to one) goes through
        vbmf_set_Y; a float32 array or a torch tensor (float64, float32, bfloat16; CPU or this session's GPU) is read where it lies,
        in its own dtype, through vbmf_set_Y_rows."""
        if capi._is_tensor(Y) or (isinstance(Y, np.ndarray) and Y.dtype != np.float64):
            if _shape2(Y) != (self.L, self.M):
                raise ValueError(f"expected shape {(self.L, self.M)}, got {tuple(Y.shape)}")
            self.ctx.set_Y_rows(Y, 0, self.L)
        else:
            self.ctx.set_Y(Y)

    def set_Y_rows(self, block, row0):
        """Rows row0 .. of a matrix that never exists whole on the host: blocks in ascending order, each a multiple of 32 rows but
        the last (capi.Context.set_Y_rows).  The session has no Y between the first block and the last."""
        self.ctx.set_Y_rows(block, row0)

    def set_Y_synthetic(self, seed, Hstar, noise_std):
        self.ctx.set_Y_synthetic(seed, Hstar, noise_std)

    # -- state <-> vbmf_parameters --
    def push(self, p):
        ca, cb = np.diag(p.CA).copy(), np.diag(p.CB).copy()
        self.ctx.set_state(p.AHat, p.BHat, p.SigmaA, p.SigmaB, ca, cb, p.sigma2, labels0=_labels0(p), H1=p.H1)

    def pull(self, p, want_B=True):
        """Rebind fields with fresh arrays (the reference's updates rebind, src/vbmf.jl:96-98,110-112);
        CA/CB diagonals are written in place (src/vbmf.jl:131,143)."""
        s = self.ctx.get_state(want_B=want_B)
        p.AHat = s["AHat"]
        if want_B:
            p.BHat = s["BHat"]
        p.SigmaA, p.SigmaB = s["SigmaA"], s["SigmaB"]
        idx = np.arange(p.H)
        p.CA[idx, idx] = s["CA_diag"]
        p.CB[idx, idx] = s["CB_diag"]
        p.invCA = np.diag(1.0 / s["CA_diag"])
        p.invCB = np.diag(1.0 / s["CB_diag"])
        p.sigma2 = s["sigma2"]
        return p

    def step(self, which):
        self.ctx.step(which)

    def run(self, niter, eps=1e-6, est_covs=False, est_var=False, want_trace=False):
        return self.ctx.run(niter, eps=eps, est_covs=est_covs, est_var=est_var, want_trace=want_trace)

    # -- results where the caller wants them (vbmf_get_YHat_rows / vbmf_get_factor_rows: no fp64 host round trip) --
    def yhat(self, out=None, dtype=None, device=None, residual=False):
        """BHat*AHat' of the state on the device (residual=True: Y as stored minus it), written into `out` as it lies -- a writable
        NumPy array or a torch tensor, see capi.y_sink -- or, without one, into a fresh result (_alloc_out): a torch tensor on this
        session's GPU when `device` asks for it, else a NumPy array.  Returns the result."""
        out = _out_or_new(out, (self.L, self.M), dtype, device, self.ctx.device)
        return self.ctx.YHat_into(out, 0, self.L, residual=residual)

    def yhat_rows(self, out, row0, residual=False):
        """Rows row0 .. row0 + out.shape[0] - 1 of the same result into `out`: a matrix that never exists whole leaves in blocks, as
        it came (set_Y_rows); any row range, no alignment."""
        return self.ctx.YHat_into(out, int(row0), None, residual=residual)

    def factors(self, out_A=None, out_B=None, dtype=None, device=None):
        """(AHat M x H, BHat L x H): the fp32 values pull() widens, each into `out_*` if given, else into a fresh result allocated as
        yhat allocates its own."""
        A = _out_or_new(out_A, (self.M, self.H), dtype, device, self.ctx.device)
        B = _out_or_new(out_B, (self.L, self.H), dtype, device, self.ctx.device)
        return self.ctx.factor_into("A", A), self.ctx.factor_into("B", B)

    def close(self):
        self.ctx.close()


def _is_torch_dtype(dtype):
    return type(dtype).__module__.split(".")[0] == "torch"


def _alloc_out(shape, dtype, device, gpu):
    """A fresh result for Session.yhat / Session.factors.  device None / False / "cpu": host memory -- a column-major NumPy array
    (float64 unless dtype says float32), or a CPU torch tensor when dtype is a torch dtype (bfloat16 has no NumPy twin).  device True /
    "cuda" / an index / a torch.device: a torch tensor on the session's GPU `gpu` (float32 unless dtype says otherwise; any other GPU
    is refused).  dtype: float64, float32 (NumPy or torch) or torch.bfloat16; anything else raises TypeError."""
    want_gpu = not (device is None or device is False or (isinstance(device, str) and device == "cpu"))
    if want_gpu or _is_torch_dtype(dtype):
        import torch
        if dtype is None:
            td = torch.float32
        elif _is_torch_dtype(dtype):
            td = dtype
        else:
            td = {np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32}.get(np.dtype(dtype))
        if td not in (torch.float64, torch.float32, torch.bfloat16):
            raise TypeError(f"the output must be float64, float32 or bfloat16, got {dtype}")
        if not want_gpu:
            return torch.empty(tuple(shape), dtype=td)
        if device is True:
            idx = gpu
        elif isinstance(device, int):
            idx = device
        else:
            dev = torch.device(device)
            if dev.type != "cuda":
                raise ValueError(f"device = {device!r}: a result lives on the CPU or on the session's GPU")
            idx = gpu if dev.index is None else dev.index
        if idx != gpu:
            raise ValueError(f"device = {device!r}, the session lives on GPU {gpu}")
        return torch.empty(tuple(shape), dtype=td, device=f"cuda:{gpu}")
    nd = np.dtype(np.float64 if dtype is None else dtype)
    if nd not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise TypeError(f"the output must be float64 or float32, got {nd}")
    return np.empty(tuple(shape), dtype=nd, order="F")


def _out_or_new(out, shape, dtype, device, gpu):
    """`out` itself (its dtype must be the one asked for, if any was), or a fresh result of _alloc_out."""
    if out is None:
        return _alloc_out(shape, dtype, device, gpu)
    if dtype is not None:
        if capi._is_tensor(out):
            same = out.dtype == dtype if _is_torch_dtype(dtype) else str(out.dtype) == "torch." + np.dtype(dtype).name
        else:
            same = not _is_torch_dtype(dtype) and getattr(out, "dtype", None) == np.dtype(dtype)
        if not same:
            raise TypeError(f"out is {getattr(out, 'dtype', type(out).__name__)}, dtype asks for {dtype}")
    return out


def _wants_gpu(Y):
    return capi._is_tensor(Y) and bool(Y.is_cuda)


# ---- cached sessions keyed on the caller's Y array ------------------------------------------------
# The reference reads the caller's Y on every call; here the matrix is uploaded once and kept on the device, so a cache hit
# must notice when the SAME array object has been changed in place (Y *= lam, Y[:] = other, preprocess into the same buffer).
# Every hit therefore re-checks a content fingerprint: the whole array up to _FP_FULL elements, beyond that an evenly strided
# sample of _FP_SAMPLE elements (sum, sum of |.|, CRC32 of the bytes).  A change that touches only entries between the
# sample points of a huge array is the one case it cannot see: call invalidate(Y) after such an edit.
_sessions = {}
_FP_FULL, _FP_SAMPLE = 1 << 22, 1 << 16


_POOL_ELEMS = 1 << 20      # sessions of matrices up to this many elements are pooled after their matrix died ...
_POOL_MAX = 48             # ... at most this many


def _fingerprint(Y):
    """Content fingerprint of the caller's matrix (whole matrix up to _FP_FULL elements, a strided sample beyond).  Compared as
    BYTES: the CRC of the sampled values, plus two sums kept as bit patterns so that a matrix holding NaN still equals itself
    (NaN != NaN would re-upload it on every call).  A non-contiguous Y (a sliced view) is sampled through its strides -- no copy
    of the matrix is made to take the fingerprint."""
    import zlib
    if Y.flags.c_contiguous or Y.flags.f_contiguous:
        flat = Y.ravel(order="K")              # a view
        if flat.size > _FP_FULL:
            flat = flat[::max(1, flat.size // _FP_SAMPLE)]
    elif Y.size > _FP_FULL:
        # sample rows and columns by strides of the view itself (~_FP_SAMPLE elements), then copy only the sample
        step = max(1, int(np.sqrt(Y.size / _FP_SAMPLE)))
        flat = Y[::step, ::step]
    else:
        flat = Y
    flat = np.ascontiguousarray(flat).reshape(-1)
    sums = np.array([flat.sum(), np.abs(flat).sum()], dtype=np.float64)
    return (sums.tobytes(), zlib.crc32(flat.tobytes()))


def invalidate(Y=None):
    """Drop the device copies cached for `Y` (all of them when Y is None): the next call uploads the matrix again."""
    for cache in (_sessions, _sparse_sessions):
        for k in [k for k, v in cache.items() if Y is None or v[1]() is Y or v[1]() is None]:
            ent = cache.pop(k)
            ent[0].close()


def _session_for(Y, H):
    if capi._is_tensor(Y):
        # a tensor: keyed on where it lies; torch counts its in-place edits (no content fingerprint, which on a GPU tensor would
        # need a read-back of the matrix)
        _shape2(Y)
        key = (id(Y), tuple(Y.shape), Y.data_ptr(), int(H), tuple(sorted(_defaults.items())), str(Y.dtype), str(Y.device))
        fp = ("version", Y._version)
    else:
        if not (isinstance(Y, np.ndarray) and Y.dtype == np.float32):   # a float32 array is uploaded, and fingerprinted, as it is
            Y = np.asarray(Y, dtype=np.float64)
        if Y.ndim != 2:
            raise ValueError("Y must be a matrix")
        key = (id(Y), Y.shape, Y.__array_interface__["data"][0], int(H), tuple(sorted(_defaults.items())))
        fp = _fingerprint(Y)
    ent = _sessions.get(key)

    if ent is not None and ent[1]() is Y:
        if ent[2] != fp:                       # same array object, new contents: upload again
            ent[0].set_Y(Y)
            _sessions[key] = (ent[0], ent[1], fp)
        return ent[0]
    # A session whose matrix has been garbage-collected is RE-USED for a new matrix of the same shape, rank and storage
    # defaults (set_Y on the existing context: no allocation, no stream / event creation -- what a caller that walks over many
    # small matrices of a few shapes pays per call otherwise; the MIL classifier's bags, examples/mil_util.jl:473-479).  Small
    # problems only (a dead session of a large matrix holds gigabytes: closed at once), at most _POOL_MAX of them.
    dead = [k for k, v in _sessions.items() if v[1]() is None or k[:3] == key[:3]]
    s = None
    for k in dead:
        if s is None and k[0] != "noY" and k[1] == key[1] and k[3:] == key[3:] and key[1][0] * key[1][1] <= _POOL_ELEMS:
            s = _sessions.pop(k)[0]
    keep = 0
    for k in dead:
        if k not in _sessions:
            continue
        if k[0] != "noY" and k[:3] != key[:3] and k[1][0] * k[1][1] <= _POOL_ELEMS and keep < _POOL_MAX:
            keep += 1                           # stays pooled for a later matrix of its shape
            continue
        _sessions.pop(k)[0].close()
    if s is None:
        s = Session(Y.shape[0], Y.shape[1], H)
    s.set_Y(Y)
    try:
        ref = weakref.ref(Y)
    except TypeError:
        ref = (lambda y: (lambda: y))(Y)
    _sessions[key] = (s, ref, fp)
    return s


def _session_for_params(p):
    """Device session for the updates whose reference signatures take NO Y (updateCA!, updateCB!, updateYHat!,
    src/vbmf.jl:120-146): any cached session of the same problem size serves (state is pushed on every call); without one,
    a context that is never given a matrix (the library runs these updates from the factors and covariances alone)."""
    for k, v in _sessions.items():
        if k[1] == (p.L, p.M) and k[3] == int(p.H) and k[4] == tuple(sorted(_defaults.items())):
            return v[0]
    key = ("noY", (p.L, p.M), 0, int(p.H), tuple(sorted(_defaults.items())))
    for k in [k for k in _sessions if k[0] == "noY"]:
        _sessions.pop(k)[0].close()
    s = Session(p.L, p.M, p.H)
    _sessions[key] = (s, lambda: None, None)
    return s


def _check(Y, p):
    if _shape2(Y) != (p.L, p.M):
        raise ValueError(f"Y is {_shape2(Y)}, params describe {(p.L, p.M)}")


def _one(Y, p, which, want_B):
    _check(Y, p)
    s = _session_for(Y, p.H)
    s.push(p)
    s.step(which)
    s.pull(p, want_B=want_B)


def updateA_(Y, params):
    """updateA! -- src/vbmf.jl:95-102."""
    _one(Y, params, STEP_A, False)


def updateB_(Y, params):
    """updateB! -- src/vbmf.jl:109-113."""
    _one(Y, params, STEP_B, True)


def _one_noY(params, which):
    s = _session_for_params(params)
    s.push(params)
    s.step(which)
    s.pull(params, want_B=False)


def updateCA_(params, Y=None):
    """updateCA! -- src/vbmf.jl:129-134: the reference's signature, no Y (a Y, if given, only selects its cached session)."""
    if Y is None:
        return _one_noY(params, STEP_CA)
    _one(Y, params, STEP_CA, False)


def updateCB_(params, Y=None):
    """updateCB! -- src/vbmf.jl:141-146: the reference's signature, no Y."""
    if Y is None:
        return _one_noY(params, STEP_CB)
    _one(Y, params, STEP_CB, False)


def updateSigma2_(Y, params):
    """updateSigma2! -- src/vbmf.jl:153-157."""
    _one(Y, params, STEP_SIGMA2, False)


def updateYHat_(params, Y=None, out=None, dtype=None, residual=False):
    """updateYHat! -- src/vbmf.jl:120-122 (device GEMM, fp64 out): the reference's signature, no Y.
    out / dtype / residual (extensions): the product goes through vbmf_get_YHat_rows into `out` as it lies (a writable NumPy array or
    a torch tensor, CPU or the session's GPU), or into a fresh result of `dtype` -- a GPU tensor when Y is one, else host memory --
    and params.YHat is bound to it; residual=True gives Y as stored minus the product and needs Y.  Without them: the fp64 host
    array, as before."""
    if out is None and dtype is None and not residual:
        s = _session_for_params(params) if Y is None else _session_for(Y, params.H)
        s.push(params)
        params.YHat = s.ctx.YHat()
        return
    if residual and Y is None:
        raise ValueError("updateYHat_: residual=True needs Y")
    s = _session_for_params(params) if Y is None else _session_for(Y, params.H)
    s.push(params)
    params.YHat = s.yhat(out=out, dtype=dtype, device=_wants_gpu(Y), residual=residual)


def elbo(Y, params):
    """Build-defined ELBO of the basic model (the reference has none)."""
    _check(Y, params)
    s = _session_for(Y, params.H)
    s.push(params)
    return s.ctx.elbo()


def _fit(Y, params, niter, eps, logdir, desc, verb, log_every, run, pull, yhat, say_saving=False):
    """The sweep loop of vbmf! and of the ARD models' twins around two callables: run(k) runs up to k sweeps on the device and
    returns (sweeps done, d, trace), pull() brings the device state into params.  logdir != "": the trajectory is logged like the
    reference does (slice 0 = the initial state, then one slice per chunk of log_every sweeps, src/vbmf.jl:181-184,205-207) and
    saved under logdir/desc (data_manip.py).  Sets params.YHat (yhat(), up to YHAT_AUTO_LIMIT elements) and params._last_run;
    returns d."""
    if logdir != "":
        logVar = create_log(params)
        i, d, iters = 1, eps + 1.0, 0
        while i <= niter and d > eps:                          # src/vbmf.jl:193 on the host, one device call per chunk
            k = int(min(max(1, log_every), niter - i + 1))
            done, d, _ = run(k)
            pull()
            update_log_(logVar, params)
            iters += done
            i += done
            if done < k:
                break
    else:
        iters, d, _ = run(int(niter))
        pull()
    params.YHat = yhat() if params.L * params.M <= YHAT_AUTO_LIMIT else None    # src/vbmf.jl:217
    if verb:
        print(f"Factorization finished after {iters} iterations, eps = {d}")   # :221
    if logdir != "":
        if say_saving:
            print(f"Saving outputs and inputs under {logdir}/")                # :226
        save_log(logVar, Y, {}, logdir, desc=desc)
    params._last_run = (iters, d)
    return d


def _gram_refusal(H, sparse, grouped=False, diag_var=False, full_cov=False):
    """Why a context made from the current defaults cannot take the Gram form (gram_structural of the library), as a phrase;
    "" when nothing on the host's side stands against it."""
    if _defaults["y_dtype"] != VBMF_Y_BF16:
        return "Y is stored in fp32 (the hosts' default): set_defaults(y_dtype=VBMF_Y_BF16) first"
    if _defaults["factor_dtype"] == VBMF_FACTOR_BF16:
        return "the single-bf16 factor (factor_dtype=VBMF_FACTOR_BF16): the form needs VBMF_FACTOR_BF16X2"
    if grouped:
        return "a grouped model (vbmf_dual / vbmf_trial) masks its B side by group"
    if diag_var:
        return ("diag_var=True: the rows' noise precisions change Y'diag(sigma)B every sweep (many small fits with per-row noise: "
                "vbmf_sparse_batch_ / vbmf_dual_batch_(..., diag_var=True))")
    if full_cov:
        return "full_cov=True: the per-column covariance blocks are built from the streamed product"
    if H > (256 if sparse else 128):
        return f"H = {H} > {256 if sparse else 128}, the largest rank the {'ARD-sparse' if sparse else 'basic'} model's Gram sweep covers"
    return ""


def _apply_form(c, form, fn, why):
    """form=None | "stream" | "gram" of the fit functions on context c (vbmf_set_gram_form).  None makes no call on a context
    whose form was never pinned, and gives one that was back to its default rule.  "gram" on a context that cannot take the form
    raises ValueError naming why (`why()`: the host's reading of gram_structural; row shards are what is left when it has none)."""
    if form is None:
        if getattr(c, "_form_pinned", False):
            c.set_gram_form(capi.VBMF_GRAM_FORM_DEFAULT)
            c._form_pinned = False
        return
    if form not in capi.GRAM_FORMS:
        raise ValueError(f"{fn}: form must be None, 'stream' or 'gram', not {form!r}")
    c.set_gram_form(capi.GRAM_FORMS[form])
    c._form_pinned = True
    if form == "gram" and not c.dims()["gram"]:
        c.set_gram_form(capi.VBMF_GRAM_FORM_DEFAULT)
        c._form_pinned = False
        raise ValueError(f"{fn}: form='gram' refused: " + (why() or "the context is one of several row shards (nranks > 1)"))


def vbmf_(Y, params, niter, eps=1e-6, est_covs=False, est_var=False, logdir="", desc="", verb=False, log_every=1, form=None):
    """vbmf! -- src/vbmf.jl:175-231.  `params` is modified in place and returned.
    logdir != "": the trajectory is logged like the reference does (slice 0 = the initial state, then one slice per
    sweep, src/vbmf.jl:181-184,205-207) and saved under logdir/desc (data_manip.py); that pulls the state off the
    device every `log_every` sweeps (an extension; 1 = the reference's behaviour), so it is a debugging mode.
    form: None (the library's rule: VBMF_GRAM, then the size rule), "stream" or "gram" (iterate on Y'Y whatever the size; a
    ValueError says why where the context cannot: fp32 storage, the single-bf16 factor, H > 128)."""
    _check(Y, params)
    s = _session_for(Y, params.H)
    _apply_form(s.ctx, form, "vbmf_", lambda: _gram_refusal(params.H, sparse=False))
    s.push(params)
    _fit(Y, params, niter, eps, logdir, desc, verb, log_every, run=lambda k: s.run(k, eps=eps, est_covs=est_covs, est_var=est_var),
         pull=lambda: s.pull(params), yhat=s.ctx.YHat, say_saving=True)
    return params


def vbmf(Y, params_in, niter, **kw):
    """vbmf -- src/vbmf.jl:238-248: shallow-copies params_in, then vbmf!."""
    p = copy(params_in)
    # the reference's shallow copy would let updateCA!/updateCB! write into params_in.CA/CB
    # (SURVEY App. A Q2); keep params_in reusable as the docstring at :235 promises
    p.CA, p.CB = p.CA.copy(), p.CB.copy()
    return vbmf_(Y, p, niter, **kw)


# =================================================================================================
# ARD-sparse variant -- src/vbmf_sparse.jl with full_cov=false, diag_var=false
# =================================================================================================
@dataclass
class vbmf_sparse_parameters:
    """src/vbmf_sparse.jl:47-90 -- same field names and order.  SigmaATVec/invSigmaATVec (dense MH x MH,
    eagerly eye()'d by the reference at :120,122) are left None: they belong to the full_cov branch only
    and cannot exist at scale.  sigmaVecHat/etaVec/zetaVec belong to diag_var=true."""
    L: int = 0
    M: int = 0
    H: int = 0
    MH: int = 0
    H1: int = 0
    labels: np.ndarray = field(default_factory=lambda: np.zeros(0, dtype=np.int64))   # 1-based
    AHat: Optional[np.ndarray] = None
    ATVecHat: Optional[np.ndarray] = None
    SigmaATVec: Optional[np.ndarray] = None
    diagSigmaATVec: Optional[np.ndarray] = None
    invSigmaATVec: Optional[np.ndarray] = None
    SigmaA: Optional[np.ndarray] = None
    BHat: Optional[np.ndarray] = None
    SigmaB: Optional[np.ndarray] = None
    CA: Optional[np.ndarray] = None
    alpha0: float = 1e-10
    beta0: float = 1e-10
    alpha: float = 0.0
    beta: Optional[np.ndarray] = None
    CB: Optional[np.ndarray] = None
    gamma0: float = 1e-10
    delta0: float = 1e-10
    gamma: float = 0.0
    delta: Optional[np.ndarray] = None
    sigmaHat: float = 1.0
    eta0: float = 1e-10
    zeta0: float = 1e-10
    eta: float = 0.0
    zeta: float = 0.0
    sigmaVecHat: Optional[np.ndarray] = None
    etaVec: Optional[np.ndarray] = None
    zetaVec: Optional[np.ndarray] = None
    YHat: Optional[np.ndarray] = None
    trYTY: float = 0.0


def vbmf_sparse_init(Y, H, ca=1.0, alpha0=1e-10, beta0=1e-10, cb=1.0, gamma0=1e-10, delta0=1e-10, sigma=1.0,
                     eta0=1e-10, zeta0=1e-10, H1=0, labels=(), rng=None):
    """src/vbmf_sparse.jl:101-153 (host side)."""
    p = vbmf_sparse_parameters()
    p.L, p.M = np.shape(Y)
    p.H, p.MH, p.H1 = int(H), p.M * int(H), int(H1)
    p.labels = np.asarray(labels, dtype=np.int64)
    return _ard_init(p, Y, ca, alpha0, beta0, cb, gamma0, delta0, sigma, eta0, zeta0, rng)


def _ard_init(p, Y, ca, alpha0, beta0, cb, gamma0, delta0, sigma, eta0, zeta0, rng):
    """What vbmf_sparse_init and its grouped twins (src/vbmf_dual.jl:122-193, src/vbmf_trial.jl:139-226) fill alike once the
    sizes of p are set: every ARD group starts from the same hyper-priors, so CA and beta are constant and the group views
    are cut from them."""
    m = _MODELS[type(p)]
    Y = np.asarray(Y)
    rng = np.random.default_rng() if rng is None else rng
    L, M, H = p.L, p.M, p.H
    p.AHat = rng.standard_normal((M, H))
    if m.labels and p.H1 > 0 and p.labels.size:
        p.AHat[_labels0(p), H - p.H1:] = 0.0
    p.ATVecHat = p.AHat.reshape(M * H).copy()
    p.diagSigmaATVec = np.ones(M * H)
    p.SigmaA = np.zeros((H, H))
    p.BHat = rng.standard_normal((L, H))
    p.SigmaB = np.zeros((H, H))
    p.CA, p.beta = ca * np.ones(M * H), beta0 * np.ones(M * H)
    for a0, b0, a in m.groups:
        setattr(p, a0, alpha0)
        setattr(p, b0, beta0)
        setattr(p, a, alpha0 + 0.5)
    if m.views is not None:
        m.views(p)
        p.alpha = _posterior_shapes(p, m)
    p.CB = cb * np.ones(H)
    p.gamma0, p.delta0, p.gamma, p.delta = gamma0, delta0, gamma0 + L / 2, delta0 * np.ones(H)
    p.sigmaHat, p.eta0, p.zeta0, p.eta, p.zeta = float(sigma), eta0, zeta0, eta0 + L * M / 2, zeta0
    p.sigmaVecHat, p.etaVec, p.zetaVec = sigma * np.ones(L), (eta0 + M / 2) * np.ones(L), zeta0 * np.ones(L)   # :145-147
    p.YHat = _host_YHat(p)
    p.trYTY = float(np.sum(Y * Y))
    return p


_sparse_sessions = {}


class _SparseKey(NamedTuple):
    Y: object                  # id() of the caller's matrix, or "noY": the context that is never given one
    shape: tuple               # (L, M)
    data: int                  # address of the matrix's buffer (0 without one)
    H: int
    diag_var: bool
    model: object              # the _Model of the parameter type
    defaults: tuple            # sorted _defaults


def _sparse_ctx(Y, p, diag_var, model):
    """Y = None: the updates whose reference signatures take no Y (updateCA!, updateCB!: src/vbmf_sparse.jl:284-300 and the
    grouped models' twins) -- a cached context of the same problem serves, else one that is never given a matrix."""
    defaults = tuple(sorted(_defaults.items()))
    if Y is None:
        # updateCA! / updateCB! do not depend on the noise model: ANY cached context of this problem and model serves, whatever
        # its diag_var (a heteroscedastic step-wise loop would otherwise evict -- and re-upload -- its own Y-holding session on every
        # CA / CB call), and a context that holds no matrix lives in its own slot instead of closing the ones that do
        for k, v in _sparse_sessions.items():
            if k.shape == (p.L, p.M) and k.H == int(p.H) and k.model is model and k.defaults == defaults:
                return v[0]
        for k in [k for k in _sparse_sessions if k.Y == "noY"]:
            _sparse_sessions.pop(k)[0].close()
        c = Context(p.L, p.M, p.H, variant=model.diag, **_defaults)
        _sparse_sessions[_SparseKey("noY", (p.L, p.M), 0, int(p.H), bool(diag_var), model, defaults)] = (c, lambda: None, None)
        return c
    Y = np.asarray(Y, dtype=np.float64)
    if Y.ndim != 2:
        raise ValueError("Y must be a matrix")
    key = _SparseKey(id(Y), Y.shape, Y.__array_interface__["data"][0], int(p.H), bool(diag_var), model, defaults)
    fp = _fingerprint(Y)
    ent = _sparse_sessions.get(key)
    if ent is not None and ent[1]() is Y:
        if ent[2] != fp:                       # same array object, new contents (see _session_for)
            ent[0].set_Y(Y)
            _sparse_sessions[key] = (ent[0], ent[1], fp)
        return ent[0]
    for k in [k for k in _sparse_sessions if k.Y != "noY"]:
        _sparse_sessions.pop(k)[0].close()
    c = Context(Y.shape[0], Y.shape[1], p.H, variant=model.diag_var if diag_var else model.diag, **_defaults)
    c.set_Y(Y)
    _sparse_sessions[key] = (c, weakref.ref(Y), fp)
    return c


def _check_derived(p):
    """alpha, gamma, eta are DERIVED constants in the reference (alpha0 + 1/2, gamma0 + L/2, eta0 + L*M/2, src/vbmf_sparse.jl:
    131,137,143) and the device derives them the same way from the hyper-priors; a struct that carries other values would be
    silently overruled, so it is refused instead."""
    for name, want in (("gamma", p.gamma0 + p.L / 2), ("eta", p.eta0 + p.L * p.M / 2)):
        have = getattr(p, name, None)
        if have is not None and np.isscalar(have) and have != 0.0 and abs(have - want) > 1e-9 * max(1.0, abs(want)):
            raise ValueError(f"params.{name} = {have} is not the derived value {want} the updates use "
                             f"(src/vbmf_sparse.jl:131-143): set the hyper-prior instead")


def _alpha_not_derived(m, p):
    """The sparse model's scalar alpha set to something other than alpha0 + 1/2 (src/vbmf_sparse.jl:131)."""
    return m.labels and np.isscalar(p.alpha) and p.alpha != 0.0 and abs(p.alpha - (p.alpha0 + 0.5)) > 1e-12


def _check_full_cov(full_cov, diag_var, H):
    if full_cov and H > 256:
        raise NotImplementedError("full_cov=true is built for H <= 256 (either noise model)")


def _push(c, p, m, diag_var=False, full_cov=False):
    """params -> device, in this order: the state, the grouped models' priors, full_cov on/off for the calls that follow, the
    caller's SigmaA as it is (vbmf_sparse_set_state derives a diagonal one from diagSigmaATVec, which is NOT what a fresh init
    state holds -- SigmaA = zeros beside diagSigmaATVec = ones, src/vbmf_sparse.jl:120-123 -- nor what a full_cov state holds),
    and under diag_var the per-row noise."""
    _check_derived(p)
    if _alpha_not_derived(m, p):
        raise ValueError(f"params.alpha = {p.alpha} is not alpha0 + 1/2 (src/vbmf_sparse.jl:131): set alpha0 instead")
    a0, b0, _ = m.groups[0]
    hyper = dict(alpha0=getattr(p, a0), beta0=getattr(p, b0), gamma0=p.gamma0, delta0=p.delta0, eta0=p.eta0, zeta0=p.zeta0)
    mask = dict(labels0=_labels0(p), H1=p.H1) if m.labels else {}
    c.sparse_set_state(p.ATVecHat, p.diagSigmaATVec, p.CA, p.beta, p.BHat, p.SigmaB, p.CB, p.delta, p.sigmaHat, p.zeta, hyper,
                       **mask)
    if m.set_priors is not None:
        m.set_priors(c, p)
    c.sparse_set_full_cov(full_cov)
    if p.SigmaA is not None:
        c.sparse_set_SigmaA(np.asarray(p.SigmaA, dtype=np.float64))
    if diag_var:
        c.sparse_set_noise_rows(p.sigmaVecHat, p.zetaVec, float(np.asarray(p.etaVec).reshape(-1)[0]))


def _posterior_shapes(p, m):
    return np.array([getattr(p, a) for _, _, a in m.groups])


def _pull(c, p, m, diag_var=False):
    """device -> params: the state, the group views, and the grouped models' priors as the last updateCA! left them (dual
    :324-325).  Under diag_var the per-row noise replaces sigmaHat / zeta, which stay as they are."""
    s = c.sparse_get_state()
    if diag_var:
        p.sigmaVecHat, p.zetaVec = c.sparse_get_noise_rows()
    p.ATVecHat, p.diagSigmaATVec, p.CA, p.beta = s["ATVecHat"], s["diagSigmaATVec"], s["CA"], s["beta"]
    p.AHat = p.ATVecHat.reshape(p.M, p.H).copy()
    p.SigmaA = np.ascontiguousarray(c.sparse_get_SigmaA())          # diagonal in the diagonal branch, full under full_cov
    p.BHat, p.SigmaB, p.CB, p.delta = s["BHat"], s["SigmaB"], s["CB"], s["delta"]
    if not diag_var:
        p.sigmaHat, p.zeta = s["sigmaHat"], s["zeta"]
    if m.views is not None:
        m.views(p)
    if m.get_priors is not None:
        for k, v in m.get_priors(c).items():
            setattr(p, k, float(v))
        p.alpha = _posterior_shapes(p, m)


def _pushed(Y, p, diag_var=False, full_cov=False):
    """The device context of p's model for Y (None: see _sparse_ctx) with p pushed into it: (context, model)."""
    m = _MODELS[type(p)]
    _check_full_cov(full_cov, diag_var, p.H)
    c = _sparse_ctx(Y, p, diag_var, m)
    _push(c, p, m, diag_var, full_cov)
    return c, m


def _step(Y, p, which, diag_var=False, full_cov=False):
    c, m = _pushed(Y, p, diag_var, full_cov)
    c.sparse_step(which)
    _pull(c, p, m, diag_var)


def _vbmf_ard(Y, params, niter, eps, diag_var, full_cov, logdir, desc, verb, est_cb, log_every, est_priors=True, form=None,
              fn="vbmf_sparse_", out=None, dtype=None):
    """vbmf_sparse! / vbmf_dual! / vbmf_trial!: returns d (like the reference).  form: see vbmf_sparse_.  out / dtype: params.YHat
    from the device (_ard_YHat), at any size; default: the host product up to YHAT_AUTO_LIMIT elements."""
    c, m = _pushed(Y, params, diag_var, full_cov)
    _apply_form(c, form, fn, lambda: _gram_refusal(params.H, sparse=True, grouped=m.set_priors is not None, diag_var=diag_var,
                                                   full_cov=full_cov))
    if out is not None or dtype is not None:
        if out is not None:
            _out_or_new(out, (params.L, params.M), dtype, None, c.device)        # an out of another dtype is refused before the run
        d = _fit(Y, params, niter, eps, logdir, desc, verb, log_every, run=lambda k: m.run(c, k, eps, est_cb, est_priors),
                 pull=lambda: _pull(c, params, m, diag_var), yhat=lambda: None)
        params.YHat = _ard_YHat(c, params, out, dtype)
        return d
    return _fit(Y, params, niter, eps, logdir, desc, verb, log_every, run=lambda k: m.run(c, k, eps, est_cb, est_priors),
                pull=lambda: _pull(c, params, m, diag_var), yhat=lambda: params.BHat @ params.AHat.T)   # host, small problems only


def _on_deep_copy(fit, Y, params_in, niter, kw):
    """vbmf_sparse / vbmf_dual / vbmf_trial: `fit` on a deep copy of params_in; returns (params, d)."""
    p = _copy.deepcopy(params_in)
    return p, fit(Y, p, niter, **kw)


def _lower_bound(Y, p, clamp, trim=None):
    c, _ = _pushed(Y, p)
    return c.sparse_lower_bound(clamp=clamp) if trim is None else c.sparse_lower_bound_trimmed(trim, clamp=clamp)


def _host_YHat(p):
    return p.BHat @ p.AHat.T if p.L * p.M <= YHAT_AUTO_LIMIT else None


def _ard_YHat(c, p, out, dtype):
    """YHat of an ARD-family shell: the host product (the default), or -- only when out / dtype ask for it -- the device product
    of context c through vbmf_get_YHat_rows, into `out` as it lies or into a fresh host result of `dtype`."""
    if out is None and dtype is None:
        return _host_YHat(p)
    return c.YHat_into(_out_or_new(out, (p.L, p.M), dtype, None, c.device), 0, p.L)


def sparse_updateA_(Y, params, full_cov=False, diag_var=False):
    """updateA! -- src/vbmf_sparse.jl:176-247.  full_cov=true (:178-202): the M diagonal blocks of the reference's dense
    MH x MH covariance, inverted one per column on the device; SigmaATVec/invSigmaATVec are not materialised."""
    _step(Y, params, SSTEP_A, diag_var, full_cov)


def sparse_updateB_(Y, params, diag_var=False):
    """updateB! -- src/vbmf_sparse.jl:254-268."""
    _step(Y, params, SSTEP_B, diag_var)


def sparse_updateCA_(params, Y=None):
    """updateCA! -- src/vbmf_sparse.jl:284-288."""
    _step(Y, params, SSTEP_CA)


def sparse_updateCB_(params, Y=None):
    """updateCB! -- src/vbmf_sparse.jl:295-300."""
    _step(Y, params, SSTEP_CB)


def sparse_updateSigma_(Y, params, diag_var=False):
    """updateSigma! -- src/vbmf_sparse.jl:307-322 (diag_var: one Gamma posterior per row, :308-315)."""
    _step(Y, params, SSTEP_SIGMA, diag_var)


def vbmf_sparse_(Y, params, niter, eps=1e-6, diag_var=False, full_cov=False, logdir="", desc="", verb=False, est_cb=True,
                 log_every=1, form=None, out=None, dtype=None):
    """vbmf_sparse! -- src/vbmf_sparse.jl:344-410.  Returns d (like the reference).  logdir: see vbmf_.  out / dtype: see _vbmf_ard.
    form: None (the library's rule: VBMF_GRAM, then the size rule, which never takes the Gram form at H > 128), "stream", or "gram":
    iterate on Y'Y at any size and up to H = 256.  "gram" raises ValueError naming the reason where the
    context cannot take the form: fp32 storage (the default here: set_defaults(y_dtype=VBMF_Y_BF16)), the single-bf16 factor,
    diag_var, full_cov, H > 256."""
    return _vbmf_ard(Y, params, niter, eps, diag_var, full_cov, logdir, desc, verb, est_cb, log_every, form=form, out=out, dtype=dtype)


def vbmf_sparse(Y, params_in, niter, **kw):
    """vbmf_sparse -- src/vbmf_sparse.jl:418-428: deep-copies params_in (:160-168), returns (params, d)."""
    return _on_deep_copy(vbmf_sparse_, Y, params_in, niter, kw)


def lowerBound(Y, params, clamp=True):
    """lowerBound -- src/vbmf_sparse.jl:435-471."""
    return _lower_bound(Y, params, clamp)


def lowerBoundTrimmed(Y, params, trim=1e-1, clamp=True):
    """lowerBoundTrimmed -- src/vbmf_sparse.jl:478-489 (dual: src/vbmf_dual.jl:606-617, trial: src/vbmf_trial.jl:687-698): the
    bound without the entries of vec(A') with |ATVecHat| <= trim (the mask sits in front of the device's M*H-long sums)."""
    return _lower_bound(Y, params, clamp, trim)

# =================================================================================================
# Two-group ARD variant -- src/vbmf_dual.jl with full_cov=false (either noise model)
# =================================================================================================
@dataclass
class vbmf_dual_parameters:
    """src/vbmf_dual.jl:59-112 -- same field names and order (SigmaATVec/invSigmaATVec stay None: full_cov branch only).
    NB the reference's naming: alpha0/alpha1 are the POSTERIOR shapes, beta0/beta1 the per-group rate vectors,
    alpha00/beta00/alpha01/beta01 the scalar hyper-priors; CA/beta are the (m, h)-interleaved vectors of :146-165."""
    L: int = 0
    M: int = 0
    MH: int = 0
    H: int = 0
    H0: int = 0
    H1: int = 0
    AHat: Optional[np.ndarray] = None
    ATVecHat: Optional[np.ndarray] = None
    SigmaATVec: Optional[np.ndarray] = None
    diagSigmaATVec: Optional[np.ndarray] = None
    invSigmaATVec: Optional[np.ndarray] = None
    SigmaA: Optional[np.ndarray] = None
    A0Hat: Optional[np.ndarray] = None
    A1Hat: Optional[np.ndarray] = None
    BHat: Optional[np.ndarray] = None
    SigmaB: Optional[np.ndarray] = None
    CA: Optional[np.ndarray] = None
    alpha: Optional[np.ndarray] = None
    beta: Optional[np.ndarray] = None
    CA0: Optional[np.ndarray] = None
    alpha00: float = 1e-10
    beta00: float = 1e-10
    alpha0: float = 0.0
    beta0: Optional[np.ndarray] = None
    CA1: Optional[np.ndarray] = None
    alpha01: float = 1e-10
    beta01: float = 1e-10
    alpha1: float = 0.0
    beta1: Optional[np.ndarray] = None
    CB: Optional[np.ndarray] = None
    gamma0: float = 1e-10
    delta0: float = 1e-10
    gamma: float = 0.0
    delta: Optional[np.ndarray] = None
    sigmaHat: float = 1.0
    eta0: float = 1e-10
    zeta0: float = 1e-10
    eta: float = 0.0
    zeta: float = 0.0
    sigmaVecHat: Optional[np.ndarray] = None
    etaVec: Optional[np.ndarray] = None
    zetaVec: Optional[np.ndarray] = None
    YHat: Optional[np.ndarray] = None
    trYTY: float = 0.0


def _dual_split(v, M, H, H0):
    a = np.asarray(v).reshape(M, H)
    return a[:, :H0].reshape(M * H0).copy(), a[:, H0:].reshape(M * (H - H0)).copy()


def vbmf_dual_init(Y, H, H0, ca=1.0, alpha0=1e-10, beta0=1e-10, cb=1.0, gamma0=1e-10, delta0=1e-10, sigma=1.0,
                   eta0=1e-10, zeta0=1e-10, rng=None):
    """src/vbmf_dual.jl:122-193 (host side)."""
    if H < H0:
        raise ValueError("H must be at least H0!")                        # :126-128
    p = vbmf_dual_parameters()
    p.L, p.M = np.shape(Y)
    p.H, p.H0 = int(H), int(H0)
    p.MH, p.H1 = p.M * p.H, p.H - p.H0
    return _ard_init(p, Y, ca, alpha0, beta0, cb, gamma0, delta0, sigma, eta0, zeta0, rng)


def _dual_views(p):
    """The per-group copies of AHat, CA and beta (src/vbmf_dual.jl:146-165)."""
    p.A0Hat, p.A1Hat = p.AHat[:, :p.H0].copy(), p.AHat[:, p.H0:].copy()
    p.CA0, p.CA1 = _dual_split(p.CA, p.M, p.H, p.H0)
    p.beta0, p.beta1 = _dual_split(p.beta, p.M, p.H, p.H0)


def dual_updateA_(Y, params, full_cov=False, diag_var=False):
    """updateA! -- src/vbmf_dual.jl:216-285 (full_cov=true, :218-243: per-column blocks, see sparse_updateA_)."""
    _step(Y, params, SSTEP_A, diag_var, full_cov)


def dual_updateB_(Y, params, diag_var=False):
    """updateB! -- src/vbmf_dual.jl:292-306."""
    _step(Y, params, SSTEP_B, diag_var)


def dual_updateCA_(params, Y=None):
    """updateCA! -- src/vbmf_dual.jl:322-351."""
    _step(Y, params, SSTEP_CA)


def dual_updateCB_(params, Y=None):
    """updateCB! -- src/vbmf_dual.jl:358-363."""
    _step(Y, params, SSTEP_CB)


def dual_updateSigma_(Y, params, diag_var=False):
    """updateSigma! -- src/vbmf_dual.jl:370-386 (diag_var: one Gamma posterior per row, :371-378)."""
    _step(Y, params, SSTEP_SIGMA, diag_var)


def dual_updateCA_and_priors_(params, Y=None):
    """updateCA! followed by updateAlpha00!, updateAlpha01!, updateBeta00!, updateBeta01! (src/vbmf_dual.jl:393-434):
    the fits read the group sums of the CA update, so the device does the pair in one call."""
    _step(Y, params, SSTEP_CA | SSTEP_PRIORS)


def vbmf_dual_(Y, params, niter, eps=1e-6, diag_var=False, full_cov=False, logdir="", desc="", verb=False, est_priors=True,
               est_cb=True, log_every=1, out=None, dtype=None):
    """vbmf_dual! -- src/vbmf_dual.jl:455-530.  Returns d (like the reference).  logdir: see vbmf_.  out / dtype: see _vbmf_ard."""
    return _vbmf_ard(Y, params, niter, eps, diag_var, full_cov, logdir, desc, verb, est_cb, log_every, est_priors, out=out, dtype=dtype)


def vbmf_dual(Y, params_in, niter, **kw):
    """vbmf_dual -- src/vbmf_dual.jl:538-549: deep-copies params_in (:200-208), returns (params, d)."""
    return _on_deep_copy(vbmf_dual_, Y, params_in, niter, kw)


def lowerBound_dual(Y, params, clamp=True):
    """lowerBound(Y, ::vbmf_dual_parameters) -- src/vbmf_dual.jl:556-599."""
    return _lower_bound(Y, params, clamp)
# =================================================================================================
# Three-group ARD variant -- src/vbmf_trial.jl with full_cov=false (either noise model)
# =================================================================================================
@dataclass
class vbmf_trial_parameters:
    """src/vbmf_trial.jl:68-131 -- same field names and order (SigmaATVec/invSigmaATVec stay None).  alpha1..alpha3 are
    the posterior shapes, beta1..beta3 the per-group rate vectors, alpha0g/beta0g the scalar hyper-priors."""
    L: int = 0
    M: int = 0
    M0: int = 0
    M1: int = 0
    MH: int = 0
    H: int = 0
    H0: int = 0
    H1: int = 0
    AHat: Optional[np.ndarray] = None
    ATVecHat: Optional[np.ndarray] = None
    SigmaATVec: Optional[np.ndarray] = None
    diagSigmaATVec: Optional[np.ndarray] = None
    invSigmaATVec: Optional[np.ndarray] = None
    SigmaA: Optional[np.ndarray] = None
    A1Hat: Optional[np.ndarray] = None
    A2Hat: Optional[np.ndarray] = None
    A3Hat: Optional[np.ndarray] = None
    BHat: Optional[np.ndarray] = None
    SigmaB: Optional[np.ndarray] = None
    CA: Optional[np.ndarray] = None
    alpha: Optional[np.ndarray] = None
    beta: Optional[np.ndarray] = None
    CA1: Optional[np.ndarray] = None
    alpha01: float = 1e-10
    beta01: float = 1e-10
    alpha1: float = 0.0
    beta1: Optional[np.ndarray] = None
    CA2: Optional[np.ndarray] = None
    alpha02: float = 1e-10
    beta02: float = 1e-10
    alpha2: float = 0.0
    beta2: Optional[np.ndarray] = None
    CA3: Optional[np.ndarray] = None
    alpha03: float = 1e-10
    beta03: float = 1e-10
    alpha3: float = 0.0
    beta3: Optional[np.ndarray] = None
    CB: Optional[np.ndarray] = None
    gamma0: float = 1e-10
    delta0: float = 1e-10
    gamma: float = 0.0
    delta: Optional[np.ndarray] = None
    sigmaHat: float = 1.0
    eta0: float = 1e-10
    zeta0: float = 1e-10
    eta: float = 0.0
    zeta: float = 0.0
    sigmaVecHat: Optional[np.ndarray] = None
    etaVec: Optional[np.ndarray] = None
    zetaVec: Optional[np.ndarray] = None
    YHat: Optional[np.ndarray] = None
    trYTY: float = 0.0


def _trial_split(v, M, H, H0, M0):
    a = np.asarray(v).reshape(M, H)
    H1 = H - H0
    return (a[:, :H0].reshape(M * H0).copy(), a[:M0, H0:].reshape(M0 * H1).copy(), a[M0:, H0:].reshape((M - M0) * H1).copy())


def vbmf_trial_init(Y, H, H0, M0, ca=1.0, alpha0=1e-10, beta0=1e-10, cb=1.0, gamma0=1e-10, delta0=1e-10, sigma=1.0,
                    eta0=1e-10, zeta0=1e-10, rng=None):
    """src/vbmf_trial.jl:139-226 (host side)."""
    if H < H0:
        raise ValueError("H must be at least H0!")                        # :143-145
    p = vbmf_trial_parameters()
    p.L, p.M = np.shape(Y)
    p.H, p.H0, p.M0 = int(H), int(H0), int(M0)
    if not 0 <= p.M0 <= p.M:
        raise ValueError("M0 must lie in 0..M")
    p.MH, p.H1, p.M1 = p.M * p.H, p.H - p.H0, p.M - p.M0
    return _ard_init(p, Y, ca, alpha0, beta0, cb, gamma0, delta0, sigma, eta0, zeta0, rng)


def _trial_views(p):
    """The per-group copies of AHat, CA and beta."""
    p.A1Hat, p.A2Hat, p.A3Hat = p.AHat[:, :p.H0].copy(), p.AHat[:p.M0, p.H0:].copy(), p.AHat[p.M0:, p.H0:].copy()
    p.CA1, p.CA2, p.CA3 = _trial_split(p.CA, p.M, p.H, p.H0, p.M0)
    p.beta1, p.beta2, p.beta3 = _trial_split(p.beta, p.M, p.H, p.H0, p.M0)


def trial_updateA_(Y, params, full_cov=False, diag_var=False):
    """updateA! -- src/vbmf_trial.jl:250-320 (full_cov=true, :252-277: per-column blocks, see sparse_updateA_)."""
    _step(Y, params, SSTEP_A, diag_var, full_cov)


def trial_updateB_(Y, params, diag_var=False):
    """updateB! -- src/vbmf_trial.jl:327-341."""
    _step(Y, params, SSTEP_B, diag_var)


def trial_updateCA_(params, Y=None):
    """updateCA! -- src/vbmf_trial.jl:357-400."""
    _step(Y, params, SSTEP_CA)


def trial_updateCB_(params, Y=None):
    """updateCB! -- src/vbmf_trial.jl:407-412."""
    _step(Y, params, SSTEP_CB)


def trial_updateSigma_(Y, params, diag_var=False):
    """updateSigma! -- src/vbmf_trial.jl:419-435."""
    _step(Y, params, SSTEP_SIGMA, diag_var)


def trial_updateCA_and_priors_(params, Y=None):
    """updateCA! followed by updateAlpha01!..03!, updateBeta01!..03! (src/vbmf_trial.jl:442-507)."""
    _step(Y, params, SSTEP_CA | SSTEP_PRIORS)


def vbmf_trial_(Y, params, niter, eps=1e-6, diag_var=False, full_cov=False, logdir="", desc="", verb=False, est_priors=True,
                est_cb=True, log_every=1, out=None, dtype=None):
    """vbmf_trial! -- src/vbmf_trial.jl:528-604.  Returns d (like the reference).  logdir: see vbmf_.  out / dtype: see _vbmf_ard."""
    return _vbmf_ard(Y, params, niter, eps, diag_var, full_cov, logdir, desc, verb, est_cb, log_every, est_priors, out=out, dtype=dtype)


def vbmf_trial(Y, params_in, niter, **kw):
    """vbmf_trial -- src/vbmf_trial.jl:612-623: deep-copies params_in (:234-242), returns (params, d)."""
    return _on_deep_copy(vbmf_trial_, Y, params_in, niter, kw)


def lowerBound_trial(Y, params, clamp=True):
    """lowerBound(Y, ::vbmf_trial_parameters) -- src/vbmf_trial.jl:630-680."""
    return _lower_bound(Y, params, clamp)


# =================================================================================================
# What differs between the ARD-sparse model and its grouped siblings; everything else is one code path (_push, _pull, _step,
# _vbmf_ard, _lower_bound, vbls_, vbls_sparse_batch_, _sparse_fit_batch) over the one vbmf_sparse_* device context
# =================================================================================================
@dataclass(frozen=True, eq=False)
class _Model:
    diag: int                              # variant id, one noise variance
    diag_var: int                          # variant id, one noise variance per row of Y
    groups: tuple                          # per ARD group: (hyper-prior shape, hyper-prior rate, posterior shape) field names;
                                           # group 0 feeds alpha0 / beta0 of vbmf_sparse_hyper
    run: Callable                          # (ctx, niter, eps, est_cb, est_priors) -> (sweeps done, d, trace)
    labels: bool = False                   # sparse only: labels0 / H1 pushed, alpha == alpha0 + 1/2 checked
    M0: bool = False                       # trial only: the last group is split at row M0 of A (a batched fit takes M0 per fit)
    set_priors: Optional[Callable] = None  # (ctx, params)
    get_priors: Optional[Callable] = None  # ctx -> {field: value}
    views: Optional[Callable] = None       # params: the group views of AHat / CA / beta


_MODELS = {
    vbmf_sparse_parameters: _Model(
        VBMF_VARIANT_SPARSE_DIAG, VBMF_VARIANT_SPARSE_DIAGVAR, (("alpha0", "beta0", "alpha"),), labels=True,
        run=lambda c, k, eps, est_cb, est_priors: c.sparse_run(k, eps=eps, est_cb=est_cb)),
    vbmf_dual_parameters: _Model(
        VBMF_VARIANT_DUAL_DIAG, VBMF_VARIANT_DUAL_DIAGVAR, (("alpha00", "beta00", "alpha0"), ("alpha01", "beta01", "alpha1")),
        run=lambda c, k, eps, est_cb, est_priors: c.dual_run(k, eps=eps, est_cb=est_cb, est_priors=est_priors),
        set_priors=lambda c, p: c.dual_set_priors(p.H0, p.alpha00, p.beta00, p.alpha01, p.beta01, p.alpha0, p.alpha1),
        get_priors=lambda c: c.dual_get_priors()[1], views=_dual_views),
    vbmf_trial_parameters: _Model(
        VBMF_VARIANT_TRIAL_DIAG, VBMF_VARIANT_TRIAL_DIAGVAR,
        (("alpha01", "beta01", "alpha1"), ("alpha02", "beta02", "alpha2"), ("alpha03", "beta03", "alpha3")),
        run=lambda c, k, eps, est_cb, est_priors: c.trial_run(k, eps=eps, est_cb=est_cb, est_priors=est_priors),
        set_priors=lambda c, p: c.trial_set_priors(p.H0, p.M0, {k: getattr(p, k) for k in Context.TRIAL_KEYS}),
        get_priors=lambda c: c.trial_get_priors()[2], views=_trial_views, M0=True),
}


# =================================================================================================
# Fixed-basis inference -- examples/mil_util.jl:179-236 (vbls!, copy_vbmf_params): the main caller of the
# update functions outside vbmf!/vbmf_sparse! (150 resp. 20 iterations per bag in the MIL study,
# examples/mil_util.jl:473-479,518-521)
# =================================================================================================
def vbls_(Y, params, niter, diag_var=False, full_cov=False, out=None, dtype=None):
    """vbls! -- examples/mil_util.jl:179-203: solves Y = B A' + E for A with B (and SigmaB, CB) fixed: niter x
    (updateA!, updateCA!, updateSigma2! / updateSigma!), then updateYHat!; returns params.AHat.
    On the device Y'B is formed once per call (B is fixed), so the call reads Y once, not 2 x niter times.
    out / dtype: params.YHat from the device through vbmf_get_YHat_rows (see updateYHat_), at any size; default: as before."""
    if type(params) in _MODELS:                                          # examples/mil_util.jl:187-197
        c, m = _pushed(Y, params, diag_var, full_cov)
        c.sparse_run_fixed_basis(int(niter))
        _pull(c, params, m, diag_var)
        params.YHat = _ard_YHat(c, params, out, dtype)
        return params.AHat
    _check_full_cov(full_cov, diag_var, params.H)
    _check(Y, params)
    s = _session_for(Y, params.H)
    s.push(params)
    s.ctx.run_fixed_basis(int(niter))
    s.pull(params)
    if out is not None or dtype is not None:
        params.YHat = s.yhat(out=out, dtype=dtype, device=_wants_gpu(Y))
        return params.AHat
    params.YHat = s.ctx.YHat() if params.L * params.M <= YHAT_AUTO_LIMIT else None     # :201
    return params.AHat


_BATCH_MAX_H = 64


def _batch_refuse(why):
    raise ValueError(f"vbls_batch_: {why}; run such bags one at a time with vbls_")


def _batch_shapes(Ys, H, refuse=_batch_refuse):
    """(L, [M_b]) of a list of bags, checked on the host: matrices, one L, H <= 64."""
    if int(H) > _BATCH_MAX_H:
        refuse(f"H = {int(H)} > {_BATCH_MAX_H}")
    if len(Ys) == 0:
        refuse("no bags")
    Ls, Ms = [], []
    for Y in Ys:
        shape = np.shape(Y)
        if len(shape) != 2 or shape[1] < 1:
            refuse(f"every bag must be a matrix with at least one column (got shape {shape})")
        Ls.append(int(shape[0]))
        Ms.append(int(shape[1]))
    if len(set(Ls)) != 1:
        refuse(f"the bags have different row counts L {sorted(set(Ls))}")
    return Ls[0], Ms


def _side_by_side(Ys, H, refuse):
    """Bags (L x M_b matrices with one L, checked by _batch_shapes) laid side by side: (L, [M_b], column offsets, the
    L x sum(M_b) matrix)."""
    L, Ms = _batch_shapes(Ys, H, refuse)
    col_off = np.concatenate([[0], np.cumsum(Ms)]).astype(np.int64)
    Yall = np.empty((L, int(col_off[-1])), order="F")
    for Y, c0, c1 in zip(Ys, col_off[:-1], col_off[1:]):
        Yall[:, c0:c1] = Y
    return L, Ms, col_off, Yall


class _Uploaded:
    """Many bags (L x M_b matrices with one L) uploaded side by side as ONE L x sum(M_b) matrix on the device: .ctx holds it, bag b is
    its columns col_off[b] .. col_off[b+1]-1."""

    def _lay_out(self, Ys, H, refuse):
        self.L, self.Ms, self.col_off, Yall = _side_by_side(Ys, H, refuse)
        self.H, self.M = int(H), Yall.shape[1]
        return Yall

    @classmethod
    def _gathered(cls, pool_ctx, idx, L, Ms, H, ctx_kw):
        """An upload whose matrices are columns `idx` of the Y in pool_ctx (BagPool.select): one Context of the class's kind and one
        set_Y_gather -- no host matrix, no set_Y.  Ms: the widths of the matrices, in order; they sum to len(idx)."""
        self = cls.__new__(cls)
        self.L, self.Ms, self.H = int(L), [int(m) for m in Ms], int(H)
        self.col_off = np.concatenate([[0], np.cumsum(self.Ms)]).astype(np.int64)
        self.M = int(self.col_off[-1])
        self._open(ctx_kw)
        try:
            self.ctx.set_Y_gather(pool_ctx, idx)
        except Exception:
            self.close()
            raise
        return self

    def __len__(self):
        return len(self.Ms)

    def close(self):
        self.ctx.close()


class Bags(_Uploaded):
    """The bags in a basic-model context, for vbls_batch_ and vbmf_batch_.  One upload serves several bases: the MIL classifier runs
    every bag against two trained models (examples/mil_util.jl:473-479)."""

    def __init__(self, Ys, H):
        Yall = self._lay_out(Ys, H, _batch_refuse)
        self.session = Session(self.L, self.M, self.H)
        self.session.set_Y(Yall)

    def _open(self, ctx_kw):
        self.session = Session(self.L, self.M, self.H, **ctx_kw)

    @property
    def ctx(self):
        return self.session.ctx


def _bag_shapes(Ys, H, cls, refuse):
    """(L, [M_b]) of the bags the sets of rank H are for, checked on the host: an upload (a `cls` made for this H) or a list of
    matrices (_batch_shapes)."""
    if isinstance(Ys, _Uploaded):
        if not isinstance(Ys, cls):
            refuse(f"a {type(Ys).__name__} where a {cls.__name__} or a list of matrices is taken")
        if Ys.H != H:
            refuse(f"the {type(Ys).__name__} were uploaded for H = {Ys.H}, the parameters have H = {H}")
        return Ys.L, Ys.Ms
    return _batch_shapes(Ys, H, refuse)


@contextmanager
def _on_device(Ys, H, cls):
    """Ys on the device: itself where it is an upload already, else a `cls` opened here and closed on the way out."""
    if isinstance(Ys, _Uploaded):
        yield Ys
        return
    bags = cls(Ys, H)
    try:
        yield bags
    finally:
        bags.close()


def _batch_check_params(L, Ms, H, params, refuse=_batch_refuse):
    if len(params) != len(Ms):
        refuse(f"{len(Ms)} bags but {len(params)} parameter sets")
    p0 = params[0]
    for b, (p, M) in enumerate(zip(params, Ms)):
        if type(p) is not vbmf_parameters:
            refuse(f"bag {b}: {type(p).__name__} (the basic model's vbmf_parameters only)")
        if int(p.H) != H:
            refuse(f"bag {b}: H = {p.H}, the bags are for H = {H}")
        if p.L != L or p.M != M:
            refuse(f"bag {b} is {L} x {M}, its parameters describe {(p.L, p.M)}")
        if int(p.H1) > 0 or np.asarray(p.labels).size > 0:
            refuse(f"bag {b} has labels / H1 > 0 (a label mask)")
        if p is not p0 and not (np.array_equal(p.BHat, p0.BHat) and np.array_equal(p.SigmaB, p0.SigmaB)
                                and np.array_equal(p.CB, p0.CB)):
            refuse(f"bag {b} does not share BHat, SigmaB and CB with bag 0 (one fixed basis per call)")


def vbls_batch_(Ys, params, niter):
    """vbls! over many bags with one fixed basis in one device call: does what [vbls_(Y, p, niter) for Y, p in zip(Ys, params)]
    does for the basic model (examples/mil_util.jl:473-479) -- fills AHat, SigmaA, CA, invCA, sigma2 (and YHat under
    YHAT_AUTO_LIMIT) of every p and returns the list of AHat.  Ys: a list of L x M_b arrays, or a Bags holding them on the device.
    params: one vbmf_parameters per bag (copy_vbmf_params), all with the same BHat, SigmaB and CB, no labels, H <= 64.
    Every bag runs all niter iterations in one workgroup of one launch (include/vbmf_hip.h, vbmf_run_fixed_basis_batched)."""
    params = list(params)
    H = int(params[0].H) if params else 0
    L, Ms = _bag_shapes(Ys, H, Bags, _batch_refuse)
    _batch_check_params(L, Ms, H, params)
    bags = Ys if isinstance(Ys, Bags) else Bags(Ys, H)
    p0 = params[0]
    ctx = bags.ctx
    ctx.set_state(np.zeros((bags.M, H)), p0.BHat, p0.SigmaA, p0.SigmaB, np.diag(p0.CA), np.diag(p0.CB), p0.sigma2)
    r = ctx.run_fixed_basis_batched(bags.col_off, int(niter), [p.sigma2 for p in params], [np.diag(p.CA) for p in params])
    idx = np.arange(H)
    out = []
    for b, p in enumerate(params):
        c0, c1 = bags.col_off[b], bags.col_off[b + 1]
        ca = r["CA_diag"][b]
        p.AHat = np.array(r["AHat"][c0:c1], order="F")             # rebound, like updateA! (src/vbmf.jl:96-98)
        p.SigmaA = r["SigmaA"][b].copy()
        p.CA[idx, idx] = ca                                          # in place (src/vbmf.jl:131)
        p.invCA = np.diag(1.0 / ca)
        p.sigma2 = float(r["sigma2"][b])
        p.YHat = _host_YHat(p)                                       # :201
        out.append(p.AHat)
    return out


def _sbatch_refuse(why):
    raise ValueError(f"vbls_sparse_batch_: {why}; run such bags one at a time with vbls_")


class SparseBags(_Uploaded):
    """The bags in a sparse-variant context, for vbls_sparse_batch_ and the sparse family's batched fits.  One upload serves several
    bases (examples/mil_util.jl:469-521 runs every bag against two trained models).  ctx_kw: Context options over the package
    defaults (e.g. reference_compat)."""

    def __init__(self, Ys, H, **ctx_kw):
        Yall = self._lay_out(Ys, H, _sbatch_refuse)
        self.ctx_kw = {**_defaults, **ctx_kw}
        self.ctx = Context(self.L, self.M, self.H, variant=VBMF_VARIANT_SPARSE_DIAG, **self.ctx_kw)
        self.ctx.set_Y(Yall)

    def _open(self, ctx_kw):
        self.ctx_kw = {**_defaults, **ctx_kw}
        self.ctx = Context(self.L, self.M, self.H, variant=VBMF_VARIANT_SPARSE_DIAG, **self.ctx_kw)


# =================================================================================================
# The data set on the device once, a call's bags gathered there -- get_matrices (examples/mil_util.jl:46) as the drivers call it
# with the bag ids of every fold (validate_with_cvs :627, validate_dataset :670)
# =================================================================================================
class BagPool:
    """A data set of bags (L x M_b matrices with one L) resident on the GPU, uploaded ONCE: a basic-variant context of rank 1 that holds
    them side by side.  select() lays chosen bags side by side in a fresh Bags / SparseBags by a device-to-device gather
    (vbmf_set_Y_gather) -- what the reference's get_matrices does on the host for every fold, p_known and repetition -- and every
    function that takes an upload takes that selection.  shapes() gives stand-ins of the selections' shapes for the initialisers.

    Ys: a list of float64 or float32 NumPy arrays (laid side by side in their own dtype: float32 when all are, else float64), or of
    torch tensors of one dtype (float64, float32, bfloat16) on the CPU or on the context's GPU (concatenated where they are); no fp64
    copy is made of a non-fp64 source.  ctx_kw: Context options over the package defaults (y_dtype, device, ...); a selection is
    stored as the pool is.  .session is the Session that holds the matrix: set_Y / set_Y_rows on it refill the pool in place with a
    matrix of the same shape (row blocks, a tensor produced on the GPU)."""

    def __init__(self, Ys, **ctx_kw):
        fn = "BagPool"
        Ys = list(Ys)
        if not Ys:
            _pool_refuse(fn, "no bags")
        shapes = []
        for b, Y in enumerate(Ys):
            shape = tuple(Y.shape) if capi._is_tensor(Y) else np.shape(Y)
            if len(shape) != 2 or shape[1] < 1:
                _pool_refuse(fn, f"every bag must be a matrix with at least one column (bag {b} has shape {tuple(shape)})")
            shapes.append((int(shape[0]), int(shape[1])))
        if len({l for l, _ in shapes}) != 1:
            _pool_refuse(fn, f"the bags have different row counts L {sorted({l for l, _ in shapes})}")
        tens = [capi._is_tensor(Y) for Y in Ys]
        if any(tens):
            if not all(tens) or len({(Y.dtype, str(Y.device)) for Y in Ys}) != 1:
                _pool_refuse(fn, "the bags must be all arrays, or all tensors of one dtype on one device")
            import torch
            Yall = Ys[0] if len(Ys) == 1 else torch.cat(Ys, dim=1)       # where they are, in their own dtype
        else:
            Ys = [Y if isinstance(Y, np.ndarray) else np.asarray(Y, dtype=np.float64) for Y in Ys]
            dtype = np.float32 if all(Y.dtype == np.float32 for Y in Ys) else np.float64
            Yall = np.empty((shapes[0][0], sum(m for _, m in shapes)), dtype=dtype, order="F")
            c0 = 0
            for Y, (_, m) in zip(Ys, shapes):
                Yall[:, c0:c0 + m] = Y
                c0 += m
        self._fill(Yall, [m for _, m in shapes], ctx_kw)

    @classmethod
    def from_matrix(cls, Yall, col_off, **ctx_kw):
        """The pool of a data set that is one L x M matrix already (an array or tensor Session.set_Y takes, as it lies): bag b is its
        columns col_off[b] .. col_off[b+1]-1."""
        fn = "BagPool.from_matrix"
        shape = tuple(Yall.shape) if capi._is_tensor(Yall) else np.shape(Yall)
        off = np.asarray(col_off, dtype=np.int64).reshape(-1)
        if len(shape) != 2:
            _pool_refuse(fn, f"Yall must be a matrix (got shape {tuple(shape)})")
        if off.size < 2 or off[0] != 0 or off[-1] != shape[1] or np.any(np.diff(off) < 1):
            _pool_refuse(fn, f"col_off must run from 0 to M = {shape[1]}, increasing (no empty bag)")
        self = cls.__new__(cls)
        self._fill(Yall if capi._is_tensor(Yall) or isinstance(Yall, np.ndarray) else np.asarray(Yall, dtype=np.float64),
                   np.diff(off), ctx_kw)
        return self

    def _fill(self, Yall, Ms, ctx_kw):
        self.Ms = [int(m) for m in Ms]
        self.col_off = np.concatenate([[0], np.cumsum(self.Ms)]).astype(np.int64)
        self.L, self.M = int(Yall.shape[0]), int(self.col_off[-1])
        self.ctx_kw = dict(ctx_kw)
        self.session = Session(self.L, self.M, 1, **ctx_kw)
        try:
            self.session.set_Y(Yall)
        except Exception:
            self.session.close()
            raise
        self._closed = False

    @property
    def ctx(self):
        return self.session.ctx

    def __len__(self):
        return len(self.Ms)

    def close(self):
        self._closed = True
        self.session.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _groups(self, fn, groups, need_columns):
        """The groups as lists of bag ids, checked on the host: a group is one id or a sequence of ids."""
        if getattr(self, "_closed", True):
            _pool_refuse(fn, "the pool is closed")
        out = []
        for k, g in enumerate(groups):
            ids = [int(g)] if np.ndim(g) == 0 else [int(b) for b in g]
            for b in ids:
                if not 0 <= b < len(self.Ms):
                    _pool_refuse(fn, f"group {k}: bag id {b} outside 0..{len(self.Ms) - 1}")
            if need_columns and not ids:
                _pool_refuse(fn, f"group {k} is empty (a matrix needs at least one bag)")
            out.append(ids)
        return out

    def widths(self, groups, _fn="BagPool.widths"):
        """Columns of every group: the sum of its bags' widths."""
        return [sum(self.Ms[b] for b in ids) for ids in self._groups(_fn, groups, False)]

    def shapes(self, groups, _fn="BagPool.shapes"):
        """One stand-in per group (a bag id or a sequence of ids; may be empty): a read-only L x M_g view of a single zero that holds
        no L x M memory, for the functions that read only the shape of Y -- vbmf_init, vbmf_sparse_init, vbmf_dual_init,
        vbmf_trial_init, copy_vbmf_params."""
        return [np.broadcast_to(np.float64(0.0), (self.L, m)) for m in self.widths(groups, _fn)]

    def select(self, groups, H, kind="basic", _fn="BagPool.select", **ctx_kw):
        """The bags of every group side by side, as a Bags (kind="basic") or a SparseBags (kind="sparse") for rank H: matrix k of the
        result is the pool's bags groups[k] in the order given (a group is a bag id or a sequence of ids; ids may repeat).  One
        Context, one vbmf_set_Y_gather: no host matrix and no upload.  ctx_kw: options over the pool's own.  Close it like any
        upload."""
        if kind not in ("basic", "sparse"):
            _pool_refuse(_fn, f"kind = {kind!r} ('basic' or 'sparse')")
        if int(H) > _BATCH_MAX_H:
            _pool_refuse(_fn, f"H = {int(H)} > {_BATCH_MAX_H}")
        if int(H) < 1:
            _pool_refuse(_fn, f"H = {int(H)} < 1")
        ids = self._groups(_fn, groups, True)
        if not ids:
            _pool_refuse(_fn, "no groups")
        off = self.col_off
        idx = np.concatenate([np.arange(off[b], off[b + 1]) for g in ids for b in g]).astype(np.int64)
        cls = Bags if kind == "basic" else SparseBags
        return cls._gathered(self.ctx, idx, self.L, [sum(self.Ms[b] for b in g) for g in ids], H, {**self.ctx_kw, **ctx_kw})


def _pool_refuse(fn, why):
    raise ValueError(f"{fn}: {why}")


def _pool_front(pool, fn, H):
    """What a training loop refuses about its pool before it draws a set or touches the library"""
    if pool is None:
        return
    if not isinstance(pool, BagPool):
        _pool_refuse(fn, f"pool is a {type(pool).__name__}, not a BagPool")
    if pool._closed:
        _pool_refuse(fn, "the pool is closed")
    if int(H) > _FIT_MAX_H:
        _pool_refuse(fn, f"H = {int(H)} > {_FIT_MAX_H}")


@contextmanager
def _selected(pool, groups, Ys, H, kind, fn):
    """What a training loop hands to its batched call: the matrices themselves, or with a pool the one selection of their groups,
    closed on the way out."""
    if pool is None:
        yield Ys
        return
    bags = pool.select(groups, H, kind=kind, _fn=fn)
    try:
        yield bags
    finally:
        bags.close()


def _sbatch_check_params(L, Ms, H, params, refuse=_sbatch_refuse):
    if len(params) != len(Ms):
        refuse(f"{len(Ms)} bags but {len(params)} parameter sets")
    p0 = params[0]
    kind = type(p0)
    m = _MODELS.get(kind)
    if m is None:
        refuse(f"{kind.__name__} (vbmf_sparse_parameters, vbmf_dual_parameters or vbmf_trial_parameters only)")
    for b, (p, M) in enumerate(zip(params, Ms)):
        if type(p) is not kind:
            refuse(f"bag {b}: {type(p).__name__} beside {kind.__name__} (one model type per call)")
        if int(p.H) != H:
            refuse(f"bag {b}: H = {p.H}, the bags are for H = {H}")
        if p.L != L or p.M != M:
            refuse(f"bag {b} is {L} x {M}, its parameters describe {(p.L, p.M)}")
        if m.labels and (int(p.H1) > 0 or np.asarray(p.labels).size > 0):
            refuse(f"bag {b} has labels / H1 > 0 (a label mask)")
        if kind is vbmf_trial_parameters and int(p.M0) != M:
            refuse(f"bag {b}: trial set with M0 = {p.M0} != M = {M} (copy_vbmf_params gives M0 = M)")
        if np.size(p.CA) != M * H:
            refuse(f"bag {b}: CA has {np.size(p.CA)} entries, not M H = {M * H}")
        if p is not p0 and not (np.array_equal(p.BHat, p0.BHat) and np.array_equal(p.SigmaB, p0.SigmaB)):
            refuse(f"bag {b} does not share BHat and SigmaB with bag 0 (one fixed basis per call)")
        _check_derived(p)
        if _alpha_not_derived(m, p):
            refuse(f"bag {b}: params.alpha = {p.alpha} is not alpha0 + 1/2 (src/vbmf_sparse.jl:131)")
    return m


def _sbatch_priors(m, p, H):
    """updateCA!'s per-column (alpha_h, beta0_h) of one parameter set (src/vbmf_sparse.jl:284-288, src/vbmf_dual.jl:322-351,
    src/vbmf_trial.jl:357-400 with M0 = M: its third group is empty)."""
    (a0, b0, _), (a1, b1, _) = m.groups[0], m.groups[min(1, len(m.groups) - 1)]
    first = np.arange(H) < getattr(p, "H0", H)
    return (np.where(first, getattr(p, a0), getattr(p, a1)) + 0.5,
            np.where(first, getattr(p, b0), getattr(p, b1)).astype(np.float64))


def vbls_sparse_batch_(Ys, params, niter, full_cov=False):
    """vbls! of the sparse models over many bags with one fixed basis in one device call: does what
    [vbls_(Y, p, niter, full_cov=full_cov) for Y, p in zip(Ys, params)] does (examples/mil_util.jl:187-197; the MIL classifiers of
    :393-416, :469-479, :497-521) -- fills on every p the fields per-bag vbls_ fills and returns the list of AHat.
    Ys: a list of L x M_b arrays, or a SparseBags holding them on the device.  params: one vbmf_sparse_parameters,
    vbmf_dual_parameters or vbmf_trial_parameters (with M0 = M_b, what copy_vbmf_params returns) per bag, all of one type, with
    the same BHat and SigmaB, no labels, H <= 64.  Every bag runs all niter iterations in one workgroup of one launch
    (include/vbmf_hip.h, vbmf_sparse_run_fixed_basis_batched)."""
    params = list(params)
    H = int(params[0].H) if params else 0
    if H > _BATCH_MAX_H:
        _sbatch_refuse(f"H = {H} > {_BATCH_MAX_H}")
    L, Ms = _bag_shapes(Ys, H, SparseBags, _sbatch_refuse)
    m = _sbatch_check_params(L, Ms, H, params)
    with _on_device(Ys, H, SparseBags) as bags:
        p0 = params[0]
        ctx = bags.ctx
        zero = np.zeros(bags.M * H)
        hyper = dict(alpha0=1e-10, beta0=1e-10, gamma0=p0.gamma0, delta0=p0.delta0, eta0=p0.eta0, zeta0=p0.zeta0)
        ctx.sparse_set_state(zero, zero + 1.0, zero + 1.0, zero + 1.0, p0.BHat, p0.SigmaB, np.ones(H), np.ones(H), 1.0, 0.0, hyper)
        pri = [_sbatch_priors(m, p, H) for p in params]
        r = ctx.sparse_run_fixed_basis_batched(bags.col_off, int(niter), np.array([a for a, _ in pri]), np.array([b for _, b in pri]),
                                               [p.eta0 + p.L * p.M / 2 for p in params], [p.zeta0 for p in params],
                                               [p.sigmaHat for p in params], np.concatenate([np.asarray(p.CA, dtype=np.float64).reshape(-1)
                                                                                              for p in params]), full_cov=full_cov)
    return [_vbls_filled(p, m, r, b, bags.col_off[b] * H) for b, p in enumerate(params)]


def _vbls_filled(p, m, r, k, s0):
    """What a batched vbls! call's results r give set p (entry k, its M H-long vectors starting at s0): the fields per-bag vbls_ fills.
    Returns p.AHat."""
    _write_A_side(p, r, k, s0)
    if m.views is not None:                                             # what _pull fills, the priors as updateCA! sets them:
        m.views(p)                                                      # src/vbmf_dual.jl:324-325, src/vbmf_trial.jl:359-361
        for a0, _, a in m.groups:
            setattr(p, a, getattr(p, a0) + 0.5)
        p.alpha = _posterior_shapes(p, m)
    p.YHat = _host_YHat(p)                                              # :201
    return p.AHat


# =================================================================================================
# Many fits in one device call -- the restart loops of examples/mil_util.jl:124-145 (train, solver "sparse") and :347-379
# (train_dual), and the folds x classes validate_dataset wraps around them (:670-788)
# =================================================================================================
_FIT_MAX_H = 32


def _fit_front(fn, one, kind, cls, Ys, params, niter, bag_of):
    """What every whole-fit batched function does before its own checks: the refuser, the sets as a list, one H <= 32, niter >= 1, the
    bags' shapes (Ys: a list of matrices or a `cls`), bag_of defaulted and validated, and per fit its type, bag, H and (L, M).
    Returns (refuse, params, bag_of, H, L, [M_b])."""
    def refuse(why):
        raise ValueError(f"{fn}: {why}; run such fits one at a time with {one}")
    only = "the basic model's vbmf_parameters only" if kind is vbmf_parameters else f"{kind.__name__} only, one model type per call"
    params = list(params)
    if not params:
        refuse("no parameter sets")
    if type(params[0]) is not kind:
        refuse(f"fit 0: {type(params[0]).__name__} ({only})")
    H = int(params[0].H)
    if H > _FIT_MAX_H:
        refuse(f"H = {H} > {_FIT_MAX_H}")
    if int(niter) < 1:
        refuse(f"niter = {niter} < 1")
    L, Ms = _bag_shapes(Ys, H, cls, refuse)
    if bag_of is None:
        if len(params) != len(Ms):
            refuse(f"{len(Ms)} bags but {len(params)} parameter sets and no bag_of")
        bag_of = range(len(Ms))
    bag_of = [int(b) for b in bag_of]
    if len(bag_of) != len(params):
        refuse(f"{len(params)} parameter sets but {len(bag_of)} entries in bag_of")
    for f, (p, b) in enumerate(zip(params, bag_of)):
        if type(p) is not kind:
            refuse(f"fit {f}: {type(p).__name__} ({only})")
        if not 0 <= b < len(Ms):
            refuse(f"fit {f}: bag_of = {b} outside 0..{len(Ms) - 1}")
        if int(p.H) != H:
            refuse(f"fit {f}: H = {p.H} beside H = {H}")
        if (p.L, p.M) != (L, Ms[b]):
            refuse(f"fit {f}: bag {b} is {L} x {Ms[b]}, its parameters describe {(p.L, p.M)}")
    return refuse, params, bag_of, H, L, Ms


def _write_A_side(p, r, k, s0):
    """What a batched call's results r hold of set k's A side, its M H-long vectors starting at s0: ATVecHat, diagSigmaATVec, CA, beta,
    AHat, SigmaA, sigmaHat, zeta (all copies) -- or, from a row-noise call, sigmaVecHat and zetaVec, with sigmaHat and zeta left as they
    were (as _pull leaves them).  Returns where the next set's vectors start."""
    s1 = s0 + p.M * p.H
    p.ATVecHat, p.diagSigmaATVec = r["ATVecHat"][s0:s1].copy(), r["diagSigmaATVec"][s0:s1].copy()
    p.CA, p.beta = r["CA"][s0:s1].copy(), r["beta"][s0:s1].copy()
    p.AHat = p.ATVecHat.reshape(p.M, p.H).copy()
    p.SigmaA = r["SigmaA"][k].copy()
    if "sigmaVecHat" in r:
        p.sigmaVecHat, p.zetaVec = r["sigmaVecHat"][k].copy(), r["zetaVec"][k].copy()
    else:
        p.sigmaHat, p.zeta = float(r["sigmaHat"][k]), float(r["zeta"][k])
    return s1


def _sparse_fit_batch(fn, one, kind, Ys, params, niter, eps, full_cov, est_cb, est_priors, bag_of, masked=False, diag_var=False,
                      form="stream", slice_cols=None):
    """The four batched fits of the sparse family: the host checks, the one device call, the fields of every set; returns the list of d.
    The models with a per-fit M0 -- the three-group one and, with masked, the sparse one under a label mask -- go through
    vbmf_local_fit_batched (H0 in 0..H), the other two through vbmf_sparse_fit_batched (H0 in 1..H).  diag_var: all four go through
    vbmf_rows_fit_batched (the models without a per-fit M0 with M0 = None: every column in group 2), from sigmaVecHat and etaVec[0];
    sigmaVecHat and zetaVec are filled, sigmaHat and zeta are left as they were.  form "split" / "auto" (and "stream" with a
    slice_cols): all four go through vbmf_ard_fit_batched_form in either noise model, nine prior values per fit; the default, "stream"
    with slice_cols None, makes the calls above as it always did.  Every set gets p.form: 0 (one workgroup) or 3 (split)."""
    code, sc = capi.ard_fit_form_code(form), capi.ard_slice_cols(slice_cols)
    by_form = code != capi.VBMF_FIT_FORM_STREAM or sc != 0
    refuse, params, bag_of, H, L, Ms = _fit_front(fn, one, kind, SparseBags, Ys, params, niter, bag_of)
    m = _MODELS[kind]
    local = masked or m.M0
    ctx_kw = Ys.ctx_kw if isinstance(Ys, SparseBags) else _defaults
    repeat = bool(ctx_kw.get("reference_compat", capi.VBMF_COMPAT_DEFAULT) & capi.VBMF_COMPAT_SPARSE_REPEAT)
    M0s = []
    for f, (p, b) in enumerate(zip(params, bag_of)):
        if masked:
            if int(p.H1) != int(params[0].H1) or not 0 <= int(p.H1) <= H:
                refuse(f"fit {f}: H1 = {p.H1} (one H1 in 0..H per call)")
            lab = np.asarray(p.labels).reshape(-1)
            if lab.size > Ms[b] or not np.array_equal(lab, np.arange(1, lab.size + 1)):
                refuse(f"fit {f}: labels are not the prefix 1..M0 of the columns (the rows of AHat the batched mask covers)")
            M0s.append(int(lab.size))
        elif m.labels:
            if int(p.H1) > 0 or np.asarray(p.labels).size > 0:
                refuse(f"fit {f} has labels / H1 > 0 (a label mask)")
        else:
            lo = 0 if local else 1
            if int(p.H0) != int(params[0].H0) or not lo <= int(p.H0) <= H:
                refuse(f"fit {f}: H0 = {p.H0} (one H0 in {lo}..H per call)")
            if local:
                if not 0 <= int(p.M0) <= Ms[b]:
                    refuse(f"fit {f}: M0 = {p.M0} outside 0..M = {Ms[b]}")
                M0s.append(int(p.M0))
        if np.shape(p.BHat) != (L, H) or np.shape(p.SigmaB) != (H, H) or np.size(p.CB) != H or np.size(p.CA) != Ms[b] * H:
            refuse(f"fit {f}: BHat, SigmaB, CB or CA does not have the shape of a {L} x {Ms[b]} problem at H = {H}")
        if not full_cov and repeat and Ms[b] < 2:
            refuse(f"fit {f} works on a 1-column bag: the diagonal form under the repeat layout needs M >= 2")
        if diag_var and (np.shape(p.sigmaVecHat) != (L,) or np.size(p.etaVec) < 1):
            refuse(f"fit {f}: sigmaVecHat is not ({L},) or etaVec is empty (diag_var=True starts from the rows' noise)")
        _check_derived(p)
        if _alpha_not_derived(m, p):
            refuse(f"fit {f}: params.alpha = {p.alpha} is not alpha0 + 1/2 (src/vbmf_sparse.jl:131)")
    rows_local = local or diag_var or by_form
    # the hyper-prior pairs of the entry's two (three) groups; a model with fewer groups gives its last pair again
    pairs = [k for g in range(3 if rows_local else 2) for k in m.groups[min(g, len(m.groups) - 1)][:2]]
    if diag_var:
        eta = [float(np.asarray(p.etaVec).reshape(-1)[0]) for p in params]       # (as _push hands it down)
        sigma = np.stack([np.asarray(p.sigmaVecHat, dtype=np.float64) for p in params])
    else:
        eta, sigma = [p.eta0 + p.L * p.M / 2 for p in params], [p.sigmaHat for p in params]
    args = (bag_of, int(niter), float(eps), [p.gamma0 + p.L / 2 for p in params], [p.delta0 for p in params],
            eta, [p.zeta0 for p in params], [[getattr(p, k) for k in pairs] for p in params],
            np.stack([np.asarray(p.BHat, dtype=np.float64) for p in params]), np.stack([np.asarray(p.SigmaB, dtype=np.float64) for p in params]),
            np.stack([np.asarray(p.CB, dtype=np.float64).reshape(H) for p in params]), sigma,
            np.concatenate([np.asarray(p.CA, dtype=np.float64).reshape(-1) for p in params]))
    kw = dict(H0=H if m.labels else int(params[0].H0), full_cov=full_cov, est_cb=est_cb, est_priors=est_priors and not m.labels)
    with _on_device(Ys, H, SparseBags) as bags:
        if by_form:
            r = bags.ctx.ard_fit_batched_form(bags.col_off, *args, M0s if local else None, mask_H1=int(params[0].H1) if masked else 0, **kw,
                                              diag_var=diag_var, form=form, slice_cols=slice_cols)
        elif diag_var:
            r = bags.ctx.rows_fit_batched(bags.col_off, *args, M0s if local else None, mask_H1=int(params[0].H1) if masked else 0, **kw)
        elif local:
            r = bags.ctx.local_fit_batched(bags.col_off, *args, M0s, mask_H1=int(params[0].H1) if masked else 0, **kw)
        else:
            r = bags.ctx.sparse_fit_batched(bags.col_off, *args, **kw)
    s0 = 0
    for f, p in enumerate(params):
        s0 = _write_A_side(p, r, f, s0)
        p.BHat, p.SigmaB, p.CB = np.array(r["BHat"][f], order="F"), r["SigmaB"][f].copy(), r["CB"][f].copy()
        if est_cb:
            p.delta = r["delta"][f].copy()
        p.iters, p.status = int(r["iters"][f]), int(r["status"][f])
        p.form = int(r["form_used"][f]) if by_form else capi.VBMF_FIT_FORM_STREAM
        if m.views is not None:
            m.views(p)
            if local:
                for k, v in zip(Context.TRIAL_KEYS, r["priors9"][f]):   # the pairs, and the shapes the last updateCA! used
                    setattr(p, k, float(v))
            elif rows_local:                                        # the two-group model through the nine-slot entry: slots 6, 7
                p.alpha00, p.beta00, p.alpha01, p.beta01 = (float(v) for v in r["priors9"][f, :4])
                p.alpha0, p.alpha1 = float(r["priors9"][f, 6]), float(r["priors9"][f, 7])
            else:
                # the posterior shapes as the last updateCA! left them (src/vbmf_dual.jl:324-325): the hyper-prior that sweep STARTED
                # from + 1/2, which est_priors has since refitted -- recovered as CA * beta of the group's first entry
                # (a fit that stopped on a non-finite value, status 1, keeps the shapes of its start values)
                ok = est_priors and p.iters > 0 and p.status == 0
                p.alpha0 = float(p.CA0[0] * p.beta0[0]) if ok else p.alpha00 + 0.5
                p.alpha1 = float(p.CA1[0] * p.beta1[0]) if ok and p.CA1.size else p.alpha01 + 0.5
                p.alpha00, p.beta00, p.alpha01, p.beta01 = (float(v) for v in r["priors4"][f])
            p.alpha = _posterior_shapes(p, m)
        p.YHat = _host_YHat(p)
    return [float(v) for v in r["d"]]


def _rows(diag_var):
    """the keyword of the row-noise path, absent when it is off: the homoscedastic calls are made as they always were"""
    return dict(diag_var=True) if diag_var else {}


def _split(form, slice_cols):
    """the keywords of the form choice, absent at their defaults: the default calls are made as they always were"""
    return {} if form == "stream" and slice_cols is None else dict(form=form, slice_cols=slice_cols)


def vbmf_sparse_batch_(Ys, params, niter, eps=1e-6, full_cov=False, est_cb=True, bag_of=None, diag_var=False, form="stream", slice_cols=None):
    """vbmf_sparse! for many independent fits in one device call: does what [vbmf_sparse_(Ys[bag_of[f]], p, niter, eps=eps, ...) for
    f, p in enumerate(params)] does (the restart loop of examples/mil_util.jl:124-145) -- fills on every p the fields vbmf_sparse_
    fills, plus p.iters (sweeps run) and p.status (1: the fit met a non-finite precision or a bad pivot and stopped), and returns the
    list of d.  Ys: a list of L x M_b arrays or a SparseBags; params: one vbmf_sparse_parameters per fit, one H <= 32, no labels;
    bag_of[f]: the fit's bag (default: fit f on bag f), so restarts share one upload.  Every fit's whole loop runs in one workgroup of
    one launch (include/vbmf_hip.h, vbmf_sparse_fit_batched).  diag_var=True: one noise precision per row of Y (examples/mil_util.jl:667),
    through vbmf_rows_fit_batched -- the fits start from p.sigmaVecHat and p.etaVec[0] and fill p.sigmaVecHat and p.zetaVec; p.sigmaHat
    and p.zeta stay as they were, as after vbmf_sparse_(..., diag_var=True).
    form: "stream" (the default: as above), "split" (every fit spread over ceil(M_b / slice_cols) workgroups, two launches per sweep:
    the form for a few wide fits; slice_cols None = capi.VBMF_FIT_SPLIT_COLS, else a multiple of 8) or "auto" (capi.ard_fit_form_auto
    per fit) -- the same iteration, another summation order (include/vbmf_hip.h, vbmf_ard_fit_batched_form).  p.form: 0 or 3.  These
    models have no Gram form: form="gram" is refused (it is vbmf_batch_'s, for the basic model)."""
    return _sparse_fit_batch("vbmf_sparse_batch_", "vbmf_sparse_", vbmf_sparse_parameters, Ys, params, niter, eps, full_cov, est_cb, False, bag_of,
                             **_rows(diag_var), **_split(form, slice_cols))


def vbmf_dual_batch_(Ys, params, niter, eps=1e-6, full_cov=False, est_cb=True, bag_of=None, est_priors=True, diag_var=False,
                     form="stream", slice_cols=None):
    """vbmf_dual! for many independent fits in one device call (the restart loop of examples/mil_util.jl:347-379): see
    vbmf_sparse_batch_, diag_var, form and slice_cols included; params: one vbmf_dual_parameters per fit, all with one H0."""
    return _sparse_fit_batch("vbmf_dual_batch_", "vbmf_dual_", vbmf_dual_parameters, Ys, params, niter, eps, full_cov, est_cb, est_priors, bag_of,
                             **_rows(diag_var), **_split(form, slice_cols))


def vbmf_trial_batch_(Ys, params, niter, eps=1e-6, full_cov=False, est_cb=True, bag_of=None, est_priors=True, diag_var=False,
                      form="stream", slice_cols=None):
    """vbmf_trial! for many independent fits in one device call: does what [vbmf_trial_(Ys[bag_of[f]], p, niter, eps=eps, ...) for f, p
    in enumerate(params)] does (src/vbmf_trial.jl:528-604) -- fills on every p the fields vbmf_trial_ fills (the group views A1Hat..A3Hat,
    CA1..3, beta1..3, the posterior shapes alpha1..3 and the six hyper-priors included), plus p.iters and p.status as vbmf_sparse_batch_
    does, and returns the list of d.  params: one vbmf_trial_parameters per fit, one H <= 32 and one H0 per call, M0 per fit.  Every
    fit's whole loop runs in one workgroup of one launch (include/vbmf_hip.h, vbmf_local_fit_batched).  diag_var, form, slice_cols: as
    in vbmf_sparse_batch_."""
    return _sparse_fit_batch("vbmf_trial_batch_", "vbmf_trial_", vbmf_trial_parameters, Ys, params, niter, eps, full_cov, est_cb, est_priors,
                             bag_of, **_rows(diag_var), **_split(form, slice_cols))


def vbmf_sparse_masked_batch_(Ys, params, niter, eps=1e-6, full_cov=False, est_cb=True, bag_of=None, diag_var=False, form="stream",
                              slice_cols=None):
    """vbmf_sparse! with a label mask for many independent fits in one device call (the fit of train_local, examples/mil_util.jl:302-320,
    on Y = [Y0 Y1]): see vbmf_sparse_batch_.  params: one vbmf_sparse_parameters per fit whose labels are exactly the prefix 1..M0 of
    the columns (possibly empty; M0 per fit), with one H1 per call: the last H1 columns of AHat stay zero in the rows 1..M0
    (src/vbmf_sparse.jl:245).  Any other label set is refused: run it with vbmf_sparse_.  diag_var, form,
    slice_cols: as in vbmf_sparse_batch_."""
    return _sparse_fit_batch("vbmf_sparse_masked_batch_", "vbmf_sparse_", vbmf_sparse_parameters, Ys, params, niter, eps, full_cov, est_cb,
                             False, bag_of, masked=True, **_rows(diag_var), **_split(form, slice_cols))


def train_local_folds(folds, H, H1, niter, eps=1e-4, rng=None, diag_var=False, form="stream", slice_cols=None, pool=None):
    """The reference's train_local (examples/mil_util.jl:302-320) over many (Y0, Y1) pairs with all the fits in ONE device call per
    round: per pair Y = [Y0 Y1] and vbmf_sparse_init(Y, H, H1=H1, labels=1:M0), drawn in fold order from the one generator; every fold
    runs vbmf_sparse! in the diagonal form (:314); then, as the loop of :312-317 does, a fold whose norm(AHat) and norm(BHat) (operator
    2-norms) are both below 1e-2 runs again from where it stands, one further call per round, ten rounds at most.  diag_var goes to
    every vbmf_sparse! as it does at :314; form and slice_cols to every vbmf_sparse_masked_batch_ call.  Returns the list of parameter
    sets.
    pool: a BagPool; every fold is then a pair of groups (bag ids of class 0, bag ids of class 1) in place of the two matrices -- the
    fit's matrix is the bags of group 0 followed by those of group 1, M0 group 0's width -- the same sets are drawn in the same order
    (from pool.shapes), the folds are selected ONCE on the device, and every round's call runs on that selection."""
    capi.ard_fit_form_code(form)
    rng = np.random.default_rng() if rng is None else rng
    if pool is not None:
        _pool_front(pool, "train_local_folds", H)
        return _train_local_pool(pool, folds, H, H1, niter, eps, rng, diag_var, form, slice_cols)
    Ys, ps = [], []
    for Y0, Y1 in folds:
        Y = np.concatenate([np.asarray(Y0, dtype=np.float64), np.asarray(Y1, dtype=np.float64)], axis=1)
        Ys.append(Y)
        ps.append(vbmf_sparse_init(Y, H, H1=H1, labels=np.arange(1, np.shape(Y0)[1] + 1), rng=rng))
    if not ps:
        return ps
    norms = lambda p: (np.linalg.norm(p.AHat, 2), np.linalg.norm(p.BHat, 2))   # Julia 0.5 norm(::Matrix): the operator 2-norm
    bound = [sum(norms(p)) for p in ps]                             # delta of :312: the first round runs whatever the norms are
    for _ in range(10):                                             # max_restarts (:310)
        again = [k for k, p in enumerate(ps) if all(v < bound[k] for v in norms(p))]
        if not again:
            break
        vbmf_sparse_masked_batch_([Ys[k] for k in again], [ps[k] for k in again], niter, eps=eps, full_cov=False, **_rows(diag_var),
                                  **_split(form, slice_cols))
        bound = [1e-2] * len(ps)                                    # :315
    return ps


def _train_local_pool(pool, folds, H, H1, niter, eps, rng, diag_var, form, slice_cols):
    """train_local_folds on the bags of a pool: its loop, with one selection in place of the matrices"""
    fn = "train_local_folds"
    groups = [[b for g in pool._groups(fn, pair, False) for b in g] for pair in folds]
    pool._groups(fn, groups, True)                                  # a fold needs at least one bag
    M0s = [pool.widths([pair[0]], fn)[0] for pair in folds]
    ps = [vbmf_sparse_init(Y, H, H1=H1, labels=np.arange(1, M0 + 1), rng=rng) for Y, M0 in zip(pool.shapes(groups, fn), M0s)]
    if not ps:
        return ps
    norms = lambda p: (np.linalg.norm(p.AHat, 2), np.linalg.norm(p.BHat, 2))
    bound = [sum(norms(p)) for p in ps]
    with _selected(pool, groups, None, H, "sparse", fn) as bags:
        for _ in range(10):
            again = [k for k, p in enumerate(ps) if all(v < bound[k] for v in norms(p))]
            if not again:
                break
            vbmf_sparse_masked_batch_(bags, [ps[k] for k in again], niter, eps=eps, full_cov=False, bag_of=again, **_rows(diag_var),
                                      **_split(form, slice_cols))
            bound = [1e-2] * len(ps)
    return ps


def fit_restarts(Y, H, niter, model="sparse", H0=None, nstarts=10, eps=None, full_cov=None, diag_var=False, rng=None, form="stream",
                 slice_cols=None):
    """The restart loops of examples/mil_util.jl:124-134 (model="sparse": eps = 1e-6, full_cov = false) and :347-354 (model="dual":
    eps = 1e-4, full_cov = true) with all nstarts initialisations drawn in order and run in ONE device call.  Returns the parameter set
    the reference's loop would have returned: sparse -- the first with d <= 2 eps and not NaN, else the last; dual -- the first with
    norm(AHat) + norm(BHat) >= 1e-2, else the last.  All nstarts fits run, also when the first would have been accepted: the launch
    costs what its slowest fit costs, and the starts behind the accepted one are discarded.  form, slice_cols: vbmf_sparse_batch_'s
    (a wide Y is the case form="split" exists for)."""
    capi.ard_fit_form_code(form)
    if model not in ("sparse", "dual"):
        raise ValueError(f"fit_restarts: model = {model!r} ('sparse' or 'dual')")
    if diag_var:
        raise ValueError("fit_restarts: diag_var=True is not batched; run the restarts one at a time with vbmf_sparse_ / vbmf_dual_ "
                         "(or all at once with vbmf_sparse_batch_ / vbmf_dual_batch_(..., diag_var=True))")
    if int(nstarts) < 1:
        raise ValueError("fit_restarts: nstarts must be >= 1")
    rng = np.random.default_rng() if rng is None else rng
    if model == "sparse":
        eps = 1e-6 if eps is None else eps
        ps = [vbmf_sparse_init(Y, H, rng=rng) for _ in range(int(nstarts))]
        ds = vbmf_sparse_batch_([Y], ps, niter, eps=eps, full_cov=bool(full_cov), bag_of=[0] * len(ps), **_split(form, slice_cols))
        for p, d in zip(ps, ds):
            if d <= 2 * eps:                                             # (false for NaN, which :130-132 turns into a restart)
                return p
        return ps[-1]
    eps = 1e-4 if eps is None else eps
    ps = [vbmf_dual_init(Y, H, H if H0 is None else H0, rng=rng) for _ in range(int(nstarts))]
    vbmf_dual_batch_([Y], ps, niter, eps=eps, full_cov=True if full_cov is None else bool(full_cov), bag_of=[0] * len(ps),
                     **_split(form, slice_cols))
    for p in ps:
        if not (np.linalg.norm(p.AHat, 2) + np.linalg.norm(p.BHat, 2) < 1e-2):   # Julia 0.5 norm(::Matrix): the operator 2-norm
            return p
    return ps[-1]


def vbmf_batch_(Ys, params, niter, eps=1e-6, est_covs=False, est_var=False, bag_of=None, form="stream"):
    """vbmf! for many independent fits of the basic model in one device call: does what [vbmf_(Ys[bag_of[f]], p, niter, eps=eps,
    est_covs=est_covs, est_var=est_var) for f, p in enumerate(params)] does (the two fits of examples/mil_util.jl:110-114, and the
    folds around them) -- fills on every p AHat, BHat, SigmaA, SigmaB (rebound), the diagonals of CA and CB (in place), invCA, invCB,
    sigma2 and YHat (under YHAT_AUTO_LIMIT), plus p.iters (sweeps run), p.d (the last d) and p.status (1: the fit met a non-finite
    sigma2, a CA / CB entry that is not positive, or a bad pivot, and stopped) -- and returns the list of params.  Ys: a list of
    L x M_b arrays or a Bags; params: one vbmf_parameters per fit, one H <= 32, no labels; bag_of[f]: the fit's bag (default: fit f on
    bag f).  Every fit's whole loop runs in fp64 in one workgroup of one launch (include/vbmf_hip.h, vbmf_fit_batched).
    form: "stream" (Y is read twice per sweep), "gram" (the sweep runs on Y Y', built once per bag: the form for bags much wider than
    tall; refused by the library where 3 L H doubles do not fit in LDS) or "auto" (capi.fit_form_auto per fit) -- the same iteration,
    different rounding (include/vbmf_hip.h, vbmf_fit_batched_form).  p.form_used: 0 (stream) or 1 (Gram)."""
    capi.fit_form_code(form)
    refuse, params, bag_of, H, L, Ms = _fit_front("vbmf_batch_", "vbmf_", vbmf_parameters, Bags, Ys, params, niter, bag_of)
    for f, (p, b) in enumerate(zip(params, bag_of)):
        if int(p.H1) > 0 or np.asarray(p.labels).size > 0:
            refuse(f"fit {f} has labels / H1 > 0 (a label mask)")
        if (np.shape(p.BHat) != (L, H) or np.shape(p.SigmaB) != (H, H) or np.shape(p.CA) != (H, H) or np.shape(p.CB) != (H, H)):
            refuse(f"fit {f}: BHat, SigmaB, CA or CB does not have the shape of a {L} x {Ms[b]} problem at H = {H}")
    with _on_device(Ys, H, Bags) as bags:
        r = bags.ctx.fit_batched(
            bags.col_off, bag_of, int(niter), float(eps), np.stack([np.asarray(p.BHat, dtype=np.float64) for p in params]),
            np.stack([np.asarray(p.SigmaB, dtype=np.float64) for p in params]), np.stack([np.diag(p.CA) for p in params]),
            np.stack([np.diag(p.CB) for p in params]), [p.sigma2 for p in params], est_covs=est_covs, est_var=est_var, form=form)
    idx = np.arange(H)
    for f, p in enumerate(params):
        p.form_used = int(r["form_used"][f])
        p.AHat = np.array(r["AHat"][f], order="F")                  # rebound, like updateA! / updateB! (src/vbmf.jl:96-98,110-112)
        p.BHat = np.array(r["BHat"][f], order="F")
        p.SigmaA, p.SigmaB = r["SigmaA"][f].copy(), r["SigmaB"][f].copy()
        p.CA[idx, idx] = r["CA"][f]                                  # in place (src/vbmf.jl:131,143)
        p.CB[idx, idx] = r["CB"][f]
        p.invCA, p.invCB = np.diag(1.0 / r["CA"][f]), np.diag(1.0 / r["CB"][f])
        p.sigma2 = float(r["sigma2"][f])
        p.iters, p.d, p.status = int(r["iters"][f]), float(r["d"][f]), int(r["status"][f])
        p.YHat = _host_YHat(p)                                       # :217
    return params


def row_gram_batch(bags):
    """K_b = Y_b Y_b' of every bag in one device call, in fp64 on Y as stored: an (nbags, L, L) array, each block symmetric bit for
    bit (include/vbmf_hip.h, vbmf_bags_row_gram).  bags: a list of L x M_b arrays (uploaded in fp32 storage for H = 1), a Bags or a
    SparseBags."""
    def refuse(why):
        raise ValueError(f"row_gram_batch: {why}")
    if not isinstance(bags, _Uploaded):
        _batch_shapes(bags, 1, refuse)
    with _on_device(bags, 1, Bags) as up:
        return up.ctx.row_gram(up.col_off)


def train_folds(folds, solver, H, niter, eps=1e-6, diag_var=False, rng=None, form="stream", slice_cols=None, pool=None):
    """The reference's train (examples/mil_util.jl:93-152) over many (Y0, Y1) pairs -- the folds, p and repetitions of a validation
    run -- with all the fits in ONE device call.  solver="basic": 2 x len(folds) fits through vbmf_batch_ with est_covs = est_var =
    True (:110-114), vbmf_init drawn in the order (fold, class) from the one generator.  solver="sparse": ten vbmf_sparse_init per class
    per fold, drawn in the order (fold, class, restart), one vbmf_sparse_batch_ call with full_cov=False, and per class the set the
    restart loop of :124-145 keeps (fit_restarts): the first with d <= 2 eps and not NaN, else the last.  Returns a list of
    (res0, res1); (0, 0) for a pair whose Y0 or Y1 has no columns (:97-100).  form: vbmf_batch_'s for solver="basic"; for
    solver="sparse" vbmf_sparse_batch_'s "stream", "split" or "auto" with its slice_cols (that solver has no Gram form: "gram" is
    refused).
    pool: a BagPool; every fold is then a pair of groups (bag ids of class 0, bag ids of class 1) in place of the two matrices, as
    get_matrices (:46) takes them: the same sets are drawn in the same order (from pool.shapes), the classes are selected once on the
    device and the one batched call runs on that selection.  (0, 0) for a pair with an empty group."""
    if solver not in ("basic", "sparse"):
        raise ValueError(f"train_folds: solver = {solver!r} ('basic' or 'sparse')")
    if solver == "sparse":
        capi.ard_fit_form_code(form)
    else:
        capi.fit_form_code(form)
    if diag_var:
        raise ValueError("train_folds: diag_var=True is not batched; train such folds one at a time with vbmf_sparse_ / vbmf_ "
                         "(or the sparse solver's fits at once with vbmf_sparse_batch_(..., diag_var=True))")
    _pool_front(pool, "train_folds", H)
    rng = np.random.default_rng() if rng is None else rng
    nstarts = 1 if solver == "basic" else 10                        # max_restarts of :108
    init = vbmf_init if solver == "basic" else vbmf_sparse_init
    Ys, ps, bag_of, where, groups = [], [], [], [], []
    for k, pair in enumerate(folds if pool is None else [pool.shapes(pair, "train_folds") for pair in folds]):
        if any(np.shape(Y)[1:] == (0,) for Y in pair):              # n0 == 0 || n1 == 0 (:97-100)
            continue
        for c, Y in enumerate(pair):
            Ys.append(Y)
            groups.append(folds[k][c])
            for _ in range(nstarts):
                ps.append(init(Y, H, rng=rng))
                bag_of.append(len(Ys) - 1)
            where.append((k, c))
    out = [(0, 0)] * len(folds)
    if not ps:
        return out
    if solver == "basic":
        kw = {} if form == "stream" else dict(form=form)            # (the default call is what it was)
        with _selected(pool, groups, Ys, H, "basic", "train_folds") as bags:
            vbmf_batch_(bags, ps, niter, eps=eps, est_covs=True, est_var=True, bag_of=bag_of, **kw)
        kept = ps
    else:
        with _selected(pool, groups, Ys, H, "sparse", "train_folds") as bags:
            ds = vbmf_sparse_batch_(bags, ps, niter, eps=eps, full_cov=False, bag_of=bag_of, **_split(form, slice_cols))
        kept = []
        for b in range(len(Ys)):
            sets = list(zip(ps[b * nstarts:(b + 1) * nstarts], ds[b * nstarts:(b + 1) * nstarts]))
            kept.append(next((p for p, d in sets if d <= 2 * eps), sets[-1][0]))   # (d <= 2 eps is false for NaN: :130-132)
    res = {}
    for (k, c), p in zip(where, kept):
        res[k, c] = p
    for k in {k for k, _ in where}:
        out[k] = (res[k, 0], res[k, 1])
    return out


def train_dual_folds(folds, H, H0, niter, eps=1e-4, diag_var=False, nstarts=10, rng=None, form="stream", slice_cols=None, pool=None):
    """The reference's train_dual (examples/mil_util.jl:327-385) over many (Y0, Y1) pairs with all the fits in ONE device call: nstarts
    vbmf_dual_init per class per fold, drawn in the order (fold, class, restart) from the one generator, one vbmf_dual_batch_ call with
    full_cov=True (:351, :376) in which the restarts of a class share its upload, and per class the set the restart loops of :347-354
    and :372-379 keep (fit_restarts(model="dual")): the first with norm(AHat) + norm(BHat) >= 1e-2 (operator 2-norms), else the last.
    diag_var goes to every vbmf_dual! as it does there.  The column subsample of :342-344 is the caller's: pass the columns to train
    on.  form, slice_cols: vbmf_dual_batch_'s.  Returns a list of (res0, res1); (0, 0) for a pair whose Y0 or Y1 has no columns, as
    train_folds does.  pool: a BagPool and folds of (bag ids of class 0, bag ids of class 1), as in train_folds."""
    capi.ard_fit_form_code(form)
    if int(nstarts) < 1:
        raise ValueError("train_dual_folds: nstarts must be >= 1")
    _pool_front(pool, "train_dual_folds", H)
    rng = np.random.default_rng() if rng is None else rng
    nstarts = int(nstarts)
    Ys, ps, bag_of, where, groups = [], [], [], [], []
    for k, pair in enumerate(folds if pool is None else [pool.shapes(pair, "train_dual_folds") for pair in folds]):
        if any(np.shape(Y)[1:] == (0,) for Y in pair):
            continue
        for c, Y in enumerate(pair):
            Ys.append(Y)
            groups.append(folds[k][c])
            for _ in range(nstarts):
                ps.append(vbmf_dual_init(Y, H, H0, rng=rng))
                bag_of.append(len(Ys) - 1)
            where.append((k, c))
    out = [(0, 0)] * len(folds)
    if not ps:
        return out
    with _selected(pool, groups, Ys, H, "sparse", "train_dual_folds") as bags:
        vbmf_dual_batch_(bags, ps, niter, eps=eps, full_cov=True, bag_of=bag_of, **_rows(diag_var), **_split(form, slice_cols))
    res = {}
    for b, kc in enumerate(where):
        sets = ps[b * nstarts:(b + 1) * nstarts]
        # Julia 0.5 norm(::Matrix): the operator 2-norm
        res[kc] = next((p for p in sets if not (np.linalg.norm(p.AHat, 2) + np.linalg.norm(p.BHat, 2) < 1e-2)), sets[-1])
    for k in {k for k, _ in where}:
        out[k] = (res[k, 0], res[k, 1])
    return out


def copy_vbmf_params(Y, old_params, rng=None):
    """copy_vbmf_params -- examples/mil_util.jl:212-290: a fresh parameter set for a NEW Y (other M), keeping what
    vbls! leaves fixed (BHat, SigmaB, CB, invCB [, gamma, delta]) and, for the grouped models, the fitted hyper-priors
    (the three-group model returns TWO sets: groups (1, 2) and (1, 3) of the trained model, each with M0 = M so that its own
    third group is empty).  Labels and H1 are not carried over (:218)."""
    def keep(p):                                                        # :240-245, 255-259, 272-276
        p.BHat, p.SigmaB, p.CB = old_params.BHat.copy(), old_params.SigmaB.copy(), old_params.CB.copy()
        p.gamma, p.delta = old_params.gamma, old_params.delta.copy()
        return p
    if isinstance(old_params, vbmf_trial_parameters):                   # :262-290: TWO parameter sets, one per special basis
        M = np.asarray(Y).shape[1]
        kw = dict(gamma0=old_params.gamma0, delta0=old_params.delta0, eta0=old_params.eta0, zeta0=old_params.zeta0, rng=rng)
        p0 = keep(vbmf_trial_init(Y, old_params.H, old_params.H0, M, **kw))
        p0.alpha01, p0.beta01, p0.alpha02, p0.beta02 = old_params.alpha01, old_params.beta01, old_params.alpha02, old_params.beta02
        p0.alpha03, p0.beta03 = 1e-10, 1e-10
        p1 = keep(vbmf_trial_init(Y, old_params.H, old_params.H0, M, **kw))
        p1.alpha01, p1.beta01, p1.alpha02, p1.beta02 = old_params.alpha01, old_params.beta01, old_params.alpha03, old_params.beta03
        p1.alpha03, p1.beta03 = 1e-10, 1e-10
        return p0, p1
    if isinstance(old_params, vbmf_dual_parameters):                    # :248-261
        p = keep(vbmf_dual_init(Y, old_params.H, old_params.H0, gamma0=old_params.gamma0, delta0=old_params.delta0,
                                eta0=old_params.eta0, zeta0=old_params.zeta0, rng=rng))
        p.alpha00, p.beta00, p.alpha01, p.beta01 = old_params.alpha00, old_params.beta00, old_params.alpha01, old_params.beta01
        return p
    if isinstance(old_params, vbmf_sparse_parameters):
        return keep(vbmf_sparse_init(Y, old_params.H, alpha0=old_params.alpha0, beta0=old_params.beta0, gamma0=old_params.gamma0,
                                     delta0=old_params.delta0, eta0=old_params.eta0, zeta0=old_params.zeta0, rng=rng))
    p = vbmf_init(Y, old_params.H, sigma2=old_params.sigma2, rng=rng)
    p.BHat, p.SigmaB = old_params.BHat.copy(), old_params.SigmaB.copy()
    p.CB, p.invCB = old_params.CB.copy(), old_params.invCB.copy()
    return p


# =================================================================================================
# Scoring many bags -- what classify (examples/mil_util.jl:453-535) compares once vbls! has run: residual norms and lower bounds,
# per bag, in one device call each (include/vbmf_hip.h: vbmf_bag_residuals, vbmf_sparse_lower_bound_batched)
# =================================================================================================
def _score_refuser(fn):
    def refuse(why):
        raise ValueError(f"{fn}: {why}; score such bags one at a time")
    return refuse


def _score_check(fn, Ys, params, bound=False):
    """Every refusal of the batched vbls! entries, before any device call.  Returns the class of the upload `params` take (Bags for
    the basic model, SparseBags for the sparse family) and the _Model (None: basic)."""
    refuse = _score_refuser(fn)
    params = list(params)
    if not params:
        refuse("no parameter sets")
    p0 = params[0]
    H = int(p0.H)
    basic = type(p0) is vbmf_parameters
    if basic and bound:
        refuse("vbmf_parameters (the bound is defined for vbmf_sparse_parameters, vbmf_dual_parameters and vbmf_trial_parameters)")
    cls = Bags if basic else SparseBags
    if isinstance(Ys, _Uploaded) and not isinstance(Ys, cls):
        refuse(f"{type(Ys).__name__} uploaded for another model family than {type(p0).__name__}")
    L, Ms = _bag_shapes(Ys, H, cls, refuse)
    if basic:
        _batch_check_params(L, Ms, H, params, refuse)
        m = None
    else:
        m = _sbatch_check_params(L, Ms, H, params, refuse)
        for b, p in enumerate(params):
            if p is not p0 and not (np.array_equal(p.CB, p0.CB) and np.array_equal(p.delta, p0.delta) and p.gamma0 == p0.gamma0
                                    and p.delta0 == p0.delta0):
                refuse(f"bag {b} does not share CB, delta, gamma0 and delta0 with bag 0 (one fixed basis per call)")
    return cls, m


def _score_ctx(bags, p0, m):
    """The bags' context with p0's basis as its state (the per-bag fields of the state are placeholders: the scoring entries take
    them as arguments)."""
    H = bags.H
    if m is None:
        bags.ctx.set_state(np.zeros((bags.M, H)), p0.BHat, p0.SigmaA, p0.SigmaB, np.diag(p0.CA), np.diag(p0.CB), p0.sigma2)
        return bags.ctx
    one = np.ones(bags.M * H)
    hyper = dict(alpha0=1e-10, beta0=1e-10, gamma0=p0.gamma0, delta0=p0.delta0, eta0=p0.eta0, zeta0=p0.zeta0)
    bags.ctx.sparse_set_state(one * 0.0, one, one, one, p0.BHat, p0.SigmaB, p0.CB, p0.delta, 1.0, 1.0, hyper)
    return bags.ctx


def _score_columns(m, p, H):
    """Per column of A: the ARD hyper-prior (shape, rate) and the posterior shape the bound reads (src/vbmf_sparse.jl:452-454, 467;
    src/vbmf_dual.jl:564-565, 575-581, 593-596; src/vbmf_trial.jl with M0 = M: its third group is empty)."""
    (a0, b0, a), (a1, b1, a_) = m.groups[0], m.groups[min(1, len(m.groups) - 1)]
    first = np.arange(H) < getattr(p, "H0", H)
    shape = lambda name: float(np.asarray(getattr(p, name)).reshape(-1)[0])
    return (np.where(first, getattr(p, a0), getattr(p, a1)).astype(np.float64),
            np.where(first, getattr(p, b0), getattr(p, b1)).astype(np.float64),
            np.where(first, shape(a), shape(a_)))


def _stacked_A(params):
    return np.concatenate([np.asarray(p.AHat, dtype=np.float64).reshape(p.M, p.H) for p in params], axis=0)


def _residual_sq(fn, Ys, params):
    params = list(params)
    cls, m = _score_check(fn, Ys, params)
    with _on_device(Ys, params[0].H, cls) as bags:
        return _score_ctx(bags, params[0], m).bag_residuals(bags.col_off, _stacked_A(params))


def residual_batch(Ys, params):
    """norm(Y_b - BHat*AHat_b') of every bag (examples/mil_util.jl:483-484) in one device call, entry by entry in fp64 from Y as the
    device stores it.  Ys: a list of L x M_b arrays, a Bags (basic model) or a SparseBags; params: the parameter sets a batched
    vbls! filled (one basis, no labels).  Returns the (nbags,) array."""
    return np.sqrt(_residual_sq("residual_batch", Ys, params))


def _bound_batch(fn, Ys, params, clamp, trim):
    params = list(params)
    cls, m = _score_check(fn, Ys, params, bound=True)
    with _on_device(Ys, params[0].H, cls) as bags:
        H = bags.H
        cols = [_score_columns(m, p, H) for p in params]
        vec = lambda f: np.concatenate([np.asarray(getattr(p, f), dtype=np.float64).reshape(-1) for p in params])
        lb, _ = _score_ctx(bags, params[0], m).sparse_lower_bound_batched(
            bags.col_off, vec("ATVecHat"), vec("diagSigmaATVec"), vec("CA"), vec("beta"),
            np.array([np.asarray(p.SigmaA, dtype=np.float64).reshape(H, H) for p in params]),
            [p.sigmaHat for p in params], [p.zeta for p in params], [p.eta for p in params], [p.eta0 for p in params],
            [p.zeta0 for p in params], np.array([c[0] for c in cols]), np.array([c[1] for c in cols]), np.array([c[2] for c in cols]),
            trim=trim, clamp=clamp, grouped=type(params[0]) is not vbmf_sparse_parameters)
        return lb


def lowerBound_batch(Ys, params, clamp=True):
    """[lowerBound(Y, p, clamp) for Y, p in zip(Ys, params)] in one device call (src/vbmf_sparse.jl:435-471, src/vbmf_dual.jl:556-599,
    src/vbmf_trial.jl:630-680 with M0 = M_b).  Ys: a list of L x M_b arrays or a SparseBags (one upload serves several models);
    params: one model type, one basis (BHat, SigmaB, CB, delta, gamma0, delta0 shared), no labels, H <= 64.  Returns (nbags,)."""
    return _bound_batch("lowerBound_batch", Ys, params, clamp, None)


def lowerBoundTrimmed_batch(Ys, params, trim=1e-1, clamp=True):
    """[lowerBoundTrimmed(Y, p, trim, clamp) for Y, p in zip(Ys, params)] in one device call (src/vbmf_sparse.jl:478-489; dual
    :606-617; trial :687-698); arguments as lowerBound_batch."""
    if not trim >= 0.0:
        raise ValueError("lowerBoundTrimmed_batch: trim must be >= 0")
    return _bound_batch("lowerBoundTrimmed_batch", Ys, params, clamp, float(trim))


_CLASS_ALGS = ("vbls", "dual", "lower_bound")


_TRIAL_TWO_SETS = ("a vbmf_trial_parameters model gives two parameter sets per bag (copy_vbmf_params), which classify does not take "
                   "either")


def _one_set(fn, q):
    if isinstance(q, tuple):
        _score_refuser(fn)(_TRIAL_TWO_SETS)
    return q


def _truncated_basis(res):
    """factorize_bag's first model (examples/mil_util.jl:398-404): the basis without its last H1 columns."""
    H0 = int(res.H) - int(res.H1)
    return dict(H=H0, BHat=np.array(res.BHat[:, :H0], order="F"), SigmaB=np.array(res.SigmaB[:H0, :H0], order="F"),
                CB=np.array(res.CB[:H0]), gamma=res.gamma, delta=np.array(res.delta[:H0]))


def _full_cov_groups(Ms, H0):
    """factorize_bag's choice of the updateA! form (:405-409), per bag: (indices with full_cov, indices without)."""
    full = [b for b, M in enumerate(Ms) if M * H0 < 1600]
    diag = [b for b, M in enumerate(Ms) if not M * H0 < 1600]
    return full, diag


def _factorize_bags(Ys, res, niter, score0=None):
    """factorize_bag (examples/mil_util.jl:393-416) over many bags: per bag (params0, params1), fitted by the batched vbls! in at
    most two groups per basis (full_cov or not), and scored where they sit: returns (L0, L1 as functions of the threshold).
    score0(bags0, ps0): what is taken from the truncated basis' fit in place of lowerBound_batch (classify_bags' "min_err")."""
    H, H1 = int(res.H), int(res.H1)
    tb = _truncated_basis(res)
    L0, sets1 = np.empty(len(Ys)), []
    for full_cov, idx in zip((True, False), _full_cov_groups([np.shape(Y)[1] for Y in Ys], H - H1)):
        if not idx:
            continue
        sub = [Ys[b] for b in idx]
        ps0 = []
        for Y in sub:
            p = vbmf_sparse_init(Y, tb["H"])
            p.BHat, p.SigmaB, p.CB, p.gamma, p.delta = tb["BHat"], tb["SigmaB"], tb["CB"], tb["gamma"], tb["delta"]
            ps0.append(p)
        ps1 = [copy_vbmf_params(Y, res) for Y in sub]
        bags0, bags1 = SparseBags(sub, tb["H"]), SparseBags(sub, H)
        try:
            vbls_sparse_batch_(bags0, ps0, niter, full_cov=full_cov)
            L0[idx] = lowerBound_batch(bags0, ps0) if score0 is None else score0(bags0, ps0)
            vbls_sparse_batch_(bags1, ps1, niter, full_cov=full_cov)
            sets1.append((idx, bags1, ps1))
        except BaseException:
            for _, opened, _ in sets1 + [(idx, bags1, ps1)]:
                opened.close()
            raise
        finally:
            bags0.close()
    return L0, sets1


def classify_batch(res0, res1, Ys, class_alg, threshold=1e-1, niter=None):
    """classify (examples/mil_util.jl:453-535) over many bags: (labels, err0, err1) as arrays, every number formed on the device by
    the batched vbls! entries and the two scoring entries.  class_alg:
      "vbls"         basic models, 150 iterations (:473-479), err = norm(Y - BHat*AHat'), label 1 where err0 > err1
      "dual"         sparse / dual models, full_cov, 20 iterations (:516-521), err = norm(YHat - Y) / (L*M), label 0 where err0 < err1
      "lower_bound"  factorize_bag on res0 (a vbmf_sparse_parameters with H1 > 0; res1 is not read, as in the reference), 20
                     iterations, full_cov per bag by M_b (H - H1) < 1600; err0 = lowerBound of the truncated basis' fit, err1 =
                     lowerBoundTrimmed(threshold) of the whole basis' fit, label 1 where err1 > err0
    niter overrides the iteration count.  "ols", "rls" and "min_err" are not taken here: classify_bags takes all six.
    Ys: a list of L x M_b arrays; for "vbls" also an uploaded Bags, for "dual" an uploaded SparseBags, of the models' H (a BagPool
    selection: nothing is uploaded and the upload is left open)."""
    fn = "classify_batch"
    refuse = _score_refuser(fn)
    if class_alg not in _CLASS_ALGS:
        refuse(f"class_alg = {class_alg!r} (one of {', '.join(_CLASS_ALGS)})")
    uploaded = isinstance(Ys, _Uploaded)
    if uploaded and class_alg == "lower_bound":
        refuse("lower_bound takes a list of matrices (it uploads them for two bases of different H)")
    if not uploaded:
        Ys = list(Ys)
    if class_alg == "lower_bound":
        if type(res0) is not vbmf_sparse_parameters or not 0 < int(res0.H1) < int(res0.H):
            refuse("lower_bound needs res0 to be a vbmf_sparse_parameters with 0 < H1 < H (factorize_bag)")
        _batch_shapes(Ys, int(res0.H), refuse)
        L0, sets1 = _factorize_bags(Ys, res0, 20 if niter is None else int(niter))
        L1 = np.empty(len(Ys))
        try:
            for idx, bags1, ps1 in sets1:
                L1[idx] = lowerBoundTrimmed_batch(bags1, ps1, threshold)
        finally:
            for _, bags1, _ in sets1:
                bags1.close()
        return (L1 > L0).astype(np.int64), L0, L1
    basic = class_alg == "vbls"
    for r in (res0, res1):
        if basic != (type(r) is vbmf_parameters) or (not basic and type(r) not in (vbmf_sparse_parameters, vbmf_dual_parameters)):
            refuse(f"class_alg = {class_alg!r} with a {type(r).__name__} model")
    if int(res0.H) != int(res1.H):
        refuse(f"the two models have different H ({res0.H}, {res1.H}): they cannot share one upload")
    H = int(res0.H)
    cls = Bags if basic else SparseBags
    L, Ms = _bag_shapes(Ys, H, cls, refuse)
    # (copy_vbmf_params reads only the shape of Y: stand-ins for an upload's bags, as BagPool.shapes gives them)
    like = [np.broadcast_to(np.float64(0.0), (L, m)) for m in Ms] if uploaded else Ys
    with _on_device(Ys, H, cls) as bags:
        errs = []
        for res in (res0, res1):
            ps = [_one_set(fn, copy_vbmf_params(Y, res)) for Y in like]
            if basic:
                vbls_batch_(bags, ps, 150 if niter is None else int(niter))
            else:
                vbls_sparse_batch_(bags, ps, 20 if niter is None else int(niter), full_cov=True)
            # the batched fit has just checked these sets and left this model's basis as the context's state
            errs.append(np.sqrt(bags.ctx.bag_residuals(bags.col_off, _stacked_A(ps))))
    err0, err1 = errs
    if basic:
        return (err0 > err1).astype(np.int64), err0, err1                # :487-491
    scale = L * np.asarray(Ms, dtype=np.float64)
    err0, err1 = err0 / scale, err1 / scale                              # :523-524
    return np.where(err0 < err1, 0, 1).astype(np.int64), err0, err1      # :526-530


# =================================================================================================
# Least-squares classifiers over many bags -- ols / rls (examples/mil_util.jl:159-171), classify's "ols", "rls" and "min_err"
# branches (:457-468, :483-501) and test_classification (:558-587); include/vbmf_hip.h: vbmf_bag_least_squares
# =================================================================================================
_LS_MAX_H = 64
_LS_ALGS = ("ols", "rls", "min_err")


def _ls_refuser(fn):
    def refuse(why):
        raise ValueError(f"{fn}: {why}")
    return refuse


def _ls_basis(fn, B, lam):
    """The caller's basis as an fp64 L x H matrix, after the refusals that need nothing else."""
    refuse = _ls_refuser(fn)
    lam = float(lam)
    if not (lam >= 0.0 and np.isfinite(lam)):
        refuse(f"lam = {lam} (must be finite and >= 0)")
    B = np.asarray(B, dtype=np.float64)
    if B.ndim != 2 or B.shape[1] < 1:
        refuse(f"B must be an L x H matrix (got shape {B.shape})")
    if B.shape[1] > _LS_MAX_H:
        refuse(f"H = {B.shape[1]} > {_LS_MAX_H}")
    if not np.all(np.isfinite(B)):
        refuse("B has non-finite entries")
    return B


def _ls_open(fn, Ys, Bs):
    """The bags on the device (_on_device) for bases Bs (checked by _ls_basis), which all must be L x H_k; an upload made here is a
    Bags at the first basis' rank -- the entry takes every call's own H."""
    refuse = _ls_refuser(fn)
    if isinstance(Ys, _Uploaded):
        L = Ys.L
    else:
        Ys = list(Ys)
        L, _ = _batch_shapes(Ys, Bs[0].shape[1], refuse)
    for B in Bs:
        if B.shape[0] != L:
            refuse(f"B is {B.shape[0]} x {B.shape[1]}, the bags have L = {L} rows (B must be L x H)")
    return _on_device(Ys, Bs[0].shape[1], Bags)


def _ls_call(fn, Ys, B, lam, want_X, want_r2):
    B = _ls_basis(fn, B, lam)
    with _ls_open(fn, Ys, [B]) as bags:
        X, r2 = bags.ctx.bag_least_squares(bags.col_off, B, lam, want_X=want_X, want_r2=want_r2)
    if want_X:
        X = [np.array(X[:, c0:c1], order="F") for c0, c1 in zip(bags.col_off[:-1], bags.col_off[1:])]
    return X, r2


def ols_batch(Ys, B):
    """[ols(Y, B) for Y in Ys] = inv(B'B)*B'*Y per bag (examples/mil_util.jl:159-161) in one device call, in fp64 from Y as the device
    stores it and B as given.  Ys: a list of L x M_b arrays, or an uploaded Bags / SparseBags (one upload serves several bases, of
    any rank); B: L x H, H <= 64.  Returns the list of H x M_b arrays."""
    return _ls_call("ols_batch", Ys, B, 0.0, True, False)[0]


def rls_batch(Ys, B, lam):
    """[rls(Y, B, lam) for Y in Ys] = inv(B'B + lam*I)*B'*Y per bag (examples/mil_util.jl:168-171) in one device call; arguments as
    ols_batch, lam >= 0."""
    return _ls_call("rls_batch", Ys, B, lam, True, False)[0]


def ls_residual_batch(Ys, B, lam=0.0):
    """norm(Y_b - B*X_b) with X_b the ols (lam = 0) or rls estimate of every bag (examples/mil_util.jl:483-484 after :459 / :466), in
    the same device pass that forms X_b, entry by entry in fp64.  Arguments as rls_batch.  Returns the (nbags,) array."""
    return np.sqrt(_ls_call("ls_residual_batch", Ys, B, lam, False, True)[1])


def classify_bags(res0, res1, Ys, class_alg="ols", threshold=1e-1, niter=None):
    """classify (examples/mil_util.jl:453-535) over many bags with the reference's default class_alg: (labels, err0, err1) as arrays.
      "ols", "rls"   err = norm(Y - BHat*AT) with AT = ols(Y, BHat) / rls(Y, BHat, 1e-2) (:457-468, :483-484), label 1 where
                     err0 > err1; any two models that have a BHat (only BHat is read), of the same or different H <= 64; one upload,
                     one device call per model
      "min_err"      factorize_bag on res0 (a vbmf_sparse_parameters with 0 < H1 < H; res1 is not read), 20 iterations, full_cov per
                     bag by M_b (H - H1) < 1600; err0 = norm(Y - YHat) of the truncated basis' fit, err1 of the whole basis' fit,
                     label 0 where |(err0 - err1)/err0| < threshold (:493-501)
      "vbls", "dual", "lower_bound"   classify_batch, unchanged
    Ys: a list of L x M_b arrays; for "ols" / "rls" also an uploaded Bags / SparseBags, for "vbls" an uploaded Bags and for "dual" an
    uploaded SparseBags of the models' H.  niter overrides the iteration count of the iterating classifiers."""
    fn = "classify_bags"
    refuse = _ls_refuser(fn)
    if class_alg in _CLASS_ALGS:
        return classify_batch(res0, res1, Ys, class_alg, threshold=threshold, niter=niter)
    if class_alg not in _LS_ALGS:
        refuse(f"class_alg = {class_alg!r} (one of {', '.join(_LS_ALGS + _CLASS_ALGS)})")
    if class_alg == "min_err":
        if type(res0) is not vbmf_sparse_parameters or not 0 < int(res0.H1) < int(res0.H):
            refuse("min_err needs res0 to be a vbmf_sparse_parameters with 0 < H1 < H (factorize_bag)")
        Ys = list(Ys)
        _batch_shapes(Ys, int(res0.H), refuse)
        err0, sets1 = _factorize_bags(Ys, res0, 20 if niter is None else int(niter), score0=residual_batch)
        err1 = np.empty(len(Ys))
        try:
            for idx, bags1, ps1 in sets1:
                err1[idx] = residual_batch(bags1, ps1)
        finally:
            for _, bags1, _ in sets1:
                bags1.close()
        with np.errstate(divide="ignore", invalid="ignore"):
            close = np.abs((err0 - err1) / err0) < threshold             # :497
        return np.where(close, 0, 1).astype(np.int64), err0, err1
    lam = 0.0 if class_alg == "ols" else 1e-2                            # :466
    Bs = []
    for k, r in enumerate((res0, res1)):
        if getattr(r, "BHat", None) is None:
            refuse(f"res{k} ({type(r).__name__}) has no BHat")
        Bs.append(_ls_basis(fn, r.BHat, lam))
    with _ls_open(fn, Ys, Bs) as bags:
        err0, err1 = [np.sqrt(bags.ctx.bag_least_squares(bags.col_off, B, lam, want_X=False)[1]) for B in Bs]
    return (err0 > err1).astype(np.int64), err0, err1                    # :487-491


def test_classification_batch(res0, res1, Ys, labels, class_alg="ols", threshold=1e-1):
    """test_classification (examples/mil_util.jl:558-587) over many bags: (mer, eer, fp, fn, n0, n1) from classify_bags' labels and the
    true labels (0 / 1, one per bag).  label - est_label == 1 counts as a false negative, -1 as a false positive; a count of zero in
    a denominator gives inf / nan as Julia's float division does."""
    labels = np.asarray(labels).reshape(-1)
    est = np.asarray(classify_bags(res0, res1, Ys, class_alg, threshold=threshold)[0]).reshape(-1)
    return _classification_counts("test_classification_batch", labels, est)


def _classification_counts(fn, labels, est):
    """(mer, eer, fp, fn, n0, n1) of test_classification (examples/mil_util.jl:574-586) from the true and the estimated labels"""
    if labels.shape != est.shape:
        raise ValueError(f"{fn}: {est.size} bags but {labels.size} labels")
    diff = labels.astype(np.int64) - est.astype(np.int64)
    fn_, fp = int(np.sum(diff == 1)), int(np.sum(diff == -1))
    n0 = int(np.sum(labels == 0))
    n1 = int(labels.size - n0)
    with np.errstate(divide="ignore", invalid="ignore"):
        mer = float(np.float64(fp + fn_) / np.float64(labels.size))
        eer = float((np.float64(fp) / np.float64(n0) + np.float64(fn_) / np.float64(n1)) / 2)
    return mer, eer, fp, fn_, n0, n1


test_classification_batch.__test__ = False        # (the reference's name; not a test for a collector that meets it)


# =================================================================================================
# vbls! for a list of (bag, model) jobs, every model with its own basis, in one device call -- what classify's "dual" branch
# (examples/mil_util.jl:515-530) runs per bag and model; include/vbmf_hip.h: vbmf_sparse_fixed_basis_jobs
# =================================================================================================
_JOBS_MAX_H = 32
_JOBS_KINDS = (vbmf_sparse_parameters, vbmf_dual_parameters)


def _jobs_refuser(fn):
    def refuse(why):
        raise ValueError(f"{fn}: {why}; run such jobs one at a time with vbls_")
    return refuse


def _jobs_model(fn, res, L, H, name, refuse):
    """One trained set as the arrays of one model of Context.sparse_fixed_basis_jobs, checked on the host.  The start values are
    copy_vbmf_params': vbmf_sparse_init / vbmf_dual_init with their default ca = 1 and sigma = 1 (_ard_init: CA = ca ones, sigmaHat =
    sigma)."""
    if isinstance(res, vbmf_trial_parameters):
        _score_refuser(fn)(_TRIAL_TWO_SETS)
    if type(res) not in _JOBS_KINDS:
        refuse(f"{name} is a {type(res).__name__} (vbmf_sparse_parameters or vbmf_dual_parameters only)")
    if int(res.H) != H:
        refuse(f"{name} has H = {res.H} beside H = {H} (one H per call)")
    B, SB = np.asarray(res.BHat, dtype=np.float64), np.asarray(res.SigmaB, dtype=np.float64)
    if B.shape != (L, H) or SB.shape != (H, H):
        refuse(f"{name}: BHat is {B.shape} and SigmaB {SB.shape}, the bags have L = {L} rows and H = {H}")
    al, b0 = _sbatch_priors(_MODELS[type(res)], res, H)
    if not all(np.all(np.isfinite(v)) for v in (B, SB, al, b0, res.eta0, res.zeta0)):
        refuse(f"{name} has a BHat, SigmaB, hyper-prior, eta0 or zeta0 that is not finite")
    return dict(BHat=B, SigmaB=SB, alpha=al, beta0=b0, eta0=float(res.eta0), zeta0=float(res.zeta0), sigma0=1.0, ca0=1.0)


def _jobs_bags(fn, Ys, refuse):
    """(L, [M_b]) of what a jobs call runs on, checked on the host: a BagPool, an upload or a list of matrices"""
    if isinstance(Ys, BagPool):
        if getattr(Ys, "_closed", True):
            refuse("the pool is closed")
        return Ys.L, Ys.Ms
    if isinstance(Ys, _Uploaded):
        return Ys.L, Ys.Ms
    return _batch_shapes(Ys, 1, refuse)


def _jobs_run(Ys, call):
    """The one device call, call(context, col_off): on the pool's own context, on the upload's, or on a Bags of rank 1 opened for the
    list and closed after"""
    if isinstance(Ys, BagPool):
        return call(Ys.ctx, Ys.col_off)
    with _on_device(Ys, 1, Bags) as bags:
        return call(bags.ctx, bags.col_off)


def _job_list(job_bag, job_model, nbags, nmodels, refuse):
    """A call's (bag, model) jobs as two lists of ints, as many of each and at least one, every one in range"""
    job_bag, job_model = [int(b) for b in job_bag], [int(k) for k in job_model]
    if len(job_bag) != len(job_model) or not job_bag:
        refuse(f"{len(job_bag)} job bags and {len(job_model)} job models (as many of each, at least one)")
    for j, (b, k) in enumerate(zip(job_bag, job_model)):
        if not 0 <= b < nbags:
            refuse(f"job {j}: bag {b} outside 0..{nbags - 1}")
        if not 0 <= k < nmodels:
            refuse(f"job {j}: model {k} outside 0..{nmodels - 1}")
    return job_bag, job_model


def vbls_sparse_jobs_(Ys, models, job_bag, job_model, niter, full_cov=False):
    """vbls! of the ARD-sparse models for a list of (bag, model) jobs in ONE device call: job j does what
    vbls_(Ys[job_bag[j]], copy_vbmf_params(Ys[job_bag[j]], models[job_model[j]]), niter, full_cov=full_cov) does
    (examples/mil_util.jl:187-197), every model with its own fp64 basis.
    Ys: a BagPool (the call runs on the pool's own context: no select, no gather, no new context), an uploaded Bags / SparseBags of
    any rank, or a list of L x M_b matrices.  models: trained vbmf_sparse_parameters / vbmf_dual_parameters, all of one H <= 32.  Jobs
    may come in any order and repeat.  Returns (sets, r2, status): per job the parameter set copy_vbmf_params gives for that bag,
    filled as vbls_sparse_batch_ fills it; r2[j] = norm(Y_b - BHat*AHat')^2 formed entry by entry on the device; status[j] = 1 for a
    job that met a non-finite precision or a bad pivot (NaN in its fields and r2; the other jobs are computed)."""
    fn = "vbls_sparse_jobs_"
    refuse = _jobs_refuser(fn)
    models = list(models)
    if not models:
        refuse("no models")
    if isinstance(models[0], vbmf_trial_parameters):
        _score_refuser(fn)(_TRIAL_TWO_SETS)
    H = int(getattr(models[0], "H", 0))
    if H > _JOBS_MAX_H:
        refuse(f"H = {H} > {_JOBS_MAX_H}")
    if int(niter) < 1:
        refuse(f"niter = {niter} < 1")
    L, Ms = _jobs_bags(fn, Ys, refuse)
    mods = [_jobs_model(fn, res, L, H, f"model {k}", refuse) for k, res in enumerate(models)]
    job_bag, job_model = _job_list(job_bag, job_model, len(Ms), len(models), refuse)
    r = _jobs_run(Ys, lambda ctx, off: ctx.sparse_fixed_basis_jobs(off, H, mods, job_bag, job_model, int(niter), full_cov=full_cov))
    sets = []
    for j, (b, k) in enumerate(zip(job_bag, job_model)):
        p = copy_vbmf_params(np.broadcast_to(np.float64(0.0), (L, Ms[b])), models[k])
        _vbls_filled(p, _MODELS[type(p)], r, j, int(r["off"][j]))
        sets.append(p)
    return sets, r["r2"], r["status"]


def _basic_jobs_model(res, L, name, refuse, what="vbmf_parameters only"):
    """One trained basic-model set as the arrays of one model of Context.fixed_basis_jobs, checked on the host.  The start values are
    copy_vbmf_params': sigma2 = the trained sigma2, CA = I (vbmf_init's default ca = 1).  CB is not read (src/vbmf.jl:95-98)."""
    if type(res) is not vbmf_parameters:
        refuse(f"{name} is a {type(res).__name__} ({what})")
    H = int(res.H)
    if not 1 <= H <= _JOBS_MAX_H:
        refuse(f"{name}: H = {H} > {_JOBS_MAX_H}" if H > _JOBS_MAX_H else f"{name}: H = {H} < 1")
    B, SB = np.asarray(res.BHat, dtype=np.float64), np.asarray(res.SigmaB, dtype=np.float64)
    if B.shape != (L, H) or SB.shape != (H, H):
        refuse(f"{name}: BHat is {B.shape} and SigmaB {SB.shape}, the bags have L = {L} rows and H = {H}")
    if not (np.all(np.isfinite(B)) and np.all(np.isfinite(SB)) and np.isfinite(float(res.sigma2))):
        refuse(f"{name} has a BHat, SigmaB or sigma2 that is not finite")
    return dict(BHat=B, SigmaB=SB, sigma2_0=float(res.sigma2), ca0=1.0)


def vbls_jobs_(Ys, models, job_bag, job_model, niter):
    """vbls! of the basic model for a list of (bag, model) jobs in ONE device call: job j does what
    vbls_(Ys[job_bag[j]], copy_vbmf_params(Ys[job_bag[j]], models[job_model[j]]), niter) does (examples/mil_util.jl:182-185), every
    model with its own fp64 basis and its own H <= 32.
    Ys: a BagPool (the call runs on the pool's own context: no select, no gather, no new context), an uploaded Bags / SparseBags of
    any rank, or a list of L x M_b matrices.  models: trained vbmf_parameters.  Jobs may come in any order and repeat.  Returns
    (sets, r2, status): per job a parameter set for that bag with AHat, SigmaA, CA, invCA, sigma2 as the iterations leave them and the
    model's BHat, SigmaB, CB, invCB (YHat is not formed); r2[j] = norm(Y_b - BHat*AHat')^2 formed entry by entry on the device;
    status[j] = 1 for a job that met a bad pivot or ended non-finite (NaN in its fields and r2; the other jobs are computed)."""
    fn = "vbls_jobs_"
    refuse = _jobs_refuser(fn)
    models = list(models)
    if not models:
        refuse("no models")
    if int(niter) < 1:
        refuse(f"niter = {niter} < 1")
    L, Ms = _jobs_bags(fn, Ys, refuse)
    mods = [_basic_jobs_model(res, L, f"model {k}", refuse) for k, res in enumerate(models)]
    job_bag, job_model = _job_list(job_bag, job_model, len(Ms), len(models), refuse)
    r = _jobs_run(Ys, lambda ctx, off: ctx.fixed_basis_jobs(off, mods, job_bag, job_model, int(niter)))
    sets = []
    for j, (b, k) in enumerate(zip(job_bag, job_model)):
        old, p = models[k], vbmf_parameters()
        p.L, p.M, p.H = L, int(Ms[b]), int(old.H)
        p.BHat, p.SigmaB = mods[k]["BHat"].copy(), mods[k]["SigmaB"].copy()
        p.CB, p.invCB = np.array(old.CB, dtype=np.float64), np.array(old.invCB, dtype=np.float64)
        ca = np.asarray(r["CA"][j])
        p.AHat, p.SigmaA = np.array(r["AHat"][j], order="F"), np.array(r["SigmaA"][j])
        with np.errstate(divide="ignore"):
            p.CA, p.invCA = np.diag(ca), np.diag(1.0 / ca)
        p.sigma2 = float(r["sigma2"][j])
        sets.append(p)
    return sets, r["r2"], r["status"]


# =================================================================================================
# Every fold's test bags against its own models in one device call -- test_classification (examples/mil_util.jl:558-587) as
# validate_with_cvs (:627-648), validate (:594-620) and validate_dataset (:670-788) run it per fold, p_known and repetition;
# include/vbmf_hip.h: vbmf_bag_least_squares_jobs ("ols", "rls"), vbmf_sparse_fixed_basis_jobs ("dual"), vbmf_fixed_basis_jobs ("vbls")
# =================================================================================================
_FOLD_LAMS = {"ols": 0.0, "rls": 1e-2}                                   # :459, :466
_FOLD_ALGS = tuple(_FOLD_LAMS) + ("dual", "vbls")


def _untrained(pair):
    """(0, 0): what train_folds returns for a fold it could not train (:97-100)"""
    return isinstance(pair, (tuple, list)) and len(pair) == 2 and all(type(r) is int and r == 0 for r in pair)


def _folds_bags(fn, Ys):
    """(L, number of bags) of what the fold functions classify, checked on the host: a BagPool, an upload or a list of matrices"""
    refuse = _ls_refuser(fn)
    if isinstance(Ys, BagPool):
        if getattr(Ys, "_closed", True):
            refuse("the pool is closed")
        return Ys.L, len(Ys.Ms)
    if isinstance(Ys, _Uploaded):
        return Ys.L, len(Ys.Ms)
    L, Ms = _batch_shapes(Ys, 1, refuse)
    return L, len(Ms)


def _fold_ids(fn, tests, nb):
    """the folds' bag indices as lists of ints, each inside 0..nb-1"""
    out = []
    for f, t in enumerate(tests):
        ids = []
        for b in (t if np.ndim(t) else [t]):
            if isinstance(b, (bool, np.bool_)) or not isinstance(b, (int, np.integer)):
                _ls_refuser(fn)(f"fold {f}: bag index {b!r} is not an integer")
            if not 0 <= b < nb:
                _ls_refuser(fn)(f"fold {f}: bag index {b} outside 0..{nb - 1}")
            ids.append(int(b))
        out.append(ids)
    return out


def _fold_alg(fn, class_alg):
    """lambda of the least-squares classifiers, None for 'dual' and 'vbls'"""
    if class_alg not in _FOLD_ALGS:
        _ls_refuser(fn)(f"class_alg = {class_alg!r} ('ols', 'rls' or 'dual', or 'vbls' with solver = 'basic'; 'lower_bound' and 'min_err' "
                        f"take a train_local model: validate_local_folds, or run them per fold with classify_bags)")
    return _FOLD_LAMS.get(class_alg)


_FOLD_SCORED_ALGS = ("lower_bound", "min_err")                           # factorize_bag's classifiers (:493-514): factorize_folds


def _fold_alg_scored(fn, class_alg):
    """_fold_alg for the functions that take factorize_bag's classifiers too (classify_folds, test_classification_folds)"""
    if class_alg in _FOLD_SCORED_ALGS:
        return None
    if class_alg not in _FOLD_ALGS:
        _ls_refuser(fn)(f"class_alg = {class_alg!r} ('ols', 'rls' or 'dual', 'vbls', 'lower_bound' or 'min_err'; any other classifier "
                        f"runs per fold with classify_bags)")
    return _FOLD_LAMS.get(class_alg)


def _fold_labels(fn, labels, nb):
    labels = np.asarray(labels).reshape(-1)
    if labels.size != nb:
        _ls_refuser(fn)(f"{nb} bags but {labels.size} labels")
    if not np.all((labels == 0) | (labels == 1)):
        _ls_refuser(fn)("labels must be 0 or 1")
    return labels.astype(np.int64)


def classify_folds(models, tests, Ys, class_alg="ols", niter=None, threshold=1e-1):
    """classify (examples/mil_util.jl:453-535) with class_alg "ols", "rls", "dual", "vbls", "lower_bound" or "min_err" for every fold of a
    validation run in ONE device call: fold f's test bags tests[f] (bag indices into Ys) against its own pair models[f] = (res0, res1).  Any objects with a BHat serve as
    models, of the same or different H <= 64; (0, 0) -- what train_folds returns for a fold it could not train -- is accepted.
    Ys: a BagPool (the indices are pool bag ids and the call runs on the pool's own context: no select, no gather, no new context), an
    uploaded Bags / SparseBags, or a list of L x M_b matrices (uploaded once as Bags).
    The call's bases are the trained folds' res0.BHat, res1.BHat in fold order -- 2 t and 2 t + 1 for the t-th trained fold, 2 f and
    2 f + 1 when every fold is trained -- with lambda 0 for "ols" and 1e-2 for "rls" (:466), its jobs (bag, 2 t) and (bag, 2 t + 1)
    for every tested bag (Context.bag_least_squares_jobs).  Returns a list with (labels, err0, err1) per fold as classify_bags gives
    them (err = sqrt(r2), label 1 where err0 > err1, bit for bit classify_bags' on that fold alone); None for a (0, 0) fold, three
    empty arrays for a fold with no test bags.
    A fold one of whose bases has a B'B + lambda I that is not positive definite (a rank-deficient basis at "ols") raises VbmfError
    naming the fold, after the other folds have been computed (the exception's .results holds them, None in that fold's place):
    "rls" is the classifier for such bases, as the reference says (:463-464).
    "dual" (:515-530): the pairs are vbmf_sparse_parameters or vbmf_dual_parameters sets, the two of a fold of one type and every
    set of the call of one H <= 32; the call's models are the trained folds' res0, res1 in fold order as above, its jobs (bag, 2 t)
    and (bag, 2 t + 1) run niter = 20 iterations of vbls! with full_cov = true (niter overrides; the least-squares classifiers do not
    read it) from what copy_vbmf_params gives (Context.sparse_fixed_basis_jobs); err = sqrt(r2) / (L M_b), label 0 where
    err0 < err1.  A fold with a job that met a non-finite precision or a bad pivot raises VbmfError naming the fold after the others
    have been computed, with .results as above.
    "lower_bound" and "min_err" (:493-514): factorize_folds(models, tests, Ys, niter, threshold) -- fold f's model is the
    vbmf_sparse_parameters with 0 < H1 < H that train_local_folds returns, bare or as the first of a pair -- and from its scores
    (labels = L1 > L0, L0, L1) for "lower_bound", (label 0 where |(err0 - err1) / err0| < threshold (:497), err0, err1) for "min_err".
    The folds may differ in H and H1.  A fold with a failed job raises VbmfError as "dual" does.  threshold is read by these two only.
    "vbls" (:469-479): the pairs are the basic model's vbmf_parameters, as train_folds(..., "basic") returns them, each of its own
    H <= 32 (a fold's two may differ); the call's models are the trained folds' res0, res1 in fold order as above, its jobs (bag, 2 t)
    and (bag, 2 t + 1) run niter = 150 iterations of vbls! (niter overrides) from what copy_vbmf_params gives -- sigma2 = the trained
    sigma2, CA = I -- (Context.fixed_basis_jobs); err = sqrt(r2), label 1 where err0 > err1 (:483-491).  A fold with a job that met
    a bad pivot or ended non-finite raises VbmfError naming the fold after the others have been computed, with .results as above."""
    fn = "classify_folds"
    refuse = _ls_refuser(fn)
    lam = _fold_alg_scored(fn, class_alg)
    if class_alg in _FOLD_SCORED_ALGS:
        models, tests = list(models), list(tests)
        if len(models) != len(tests):
            refuse(f"{len(models)} models but {len(tests)} test lists")
        try:
            scores = _factorize_folds(fn, models, tests, Ys, 20 if niter is None else int(niter), threshold, class_alg)
        except VbmfError as e:
            if hasattr(e, "results"):
                e.results = [_scored_labels(r, class_alg, threshold) for r in e.results]
            raise
        return [_scored_labels(r, class_alg, threshold) for r in scores]
    models, tests = list(models), list(tests)
    if len(models) != len(tests):
        refuse(f"{len(models)} models but {len(tests)} test lists")
    L, nb = _folds_bags(fn, Ys)
    ids = _fold_ids(fn, tests, nb)
    if class_alg == "dual":
        return _classify_folds_dual(fn, models, ids, Ys, L, 20 if niter is None else int(niter))
    if class_alg == "vbls":
        return _classify_folds_vbls(fn, models, ids, Ys, L, 150 if niter is None else int(niter))
    def two_bases(f, pair):
        out = []
        for k, r in enumerate(pair):
            if getattr(r, "BHat", None) is None:
                refuse(f"fold {f}: res{k} ({type(r).__name__}) has no BHat")
            B = _ls_basis(f"{fn}: fold {f}: res{k}", r.BHat, lam)
            if B.shape[0] != L:
                refuse(f"fold {f}: res{k}.BHat is {B.shape[0]} x {B.shape[1]}, the bags have L = {L} rows")
            out.append(B)
        return out

    def call(bases, job_bag, job_basis):
        run = lambda ctx, off: ctx.bag_least_squares_jobs(off, bases, [lam] * len(bases), job_bag, job_basis)
        if isinstance(Ys, BagPool):                                     # (Xs, r2, status) -> (r2, status): a basis is flagged, not a job
            return run(Ys.ctx, Ys.col_off)[1:]
        with _on_device(Ys, bases[0].shape[1], Bags) as bags:           # (a Bags of the first basis' rank: the call reads Y only)
            return run(bags.ctx, bags.col_off)[1:]
    return _fold_jobs(fn, models, ids, two_bases, call, _residual_labels,
                      lambda k, b: f"BHat'BHat + lambda I of res{k} is not positive definite (a pivot is not positive or not finite); "
                                   f"class_alg='rls' is the classifier for such bases", model_flags=True)


# What a fold's entry of `models` may be: (is it an untrained fold?, must it be a pair?, what a trained fold with no test bags returns).
_PAIR_FOLDS = (_untrained, True, lambda: (np.empty(0, dtype=np.int64), np.empty(0), np.empty(0)))      # (res0, res1) or (0, 0)
_SCORED_FOLDS = (lambda m: _untrained(m) or (type(m) is int and m == 0), False,                         # a bare model, a bare 0 too
                 lambda: dict(L0=np.empty(0), L1=np.empty(0), err0=np.empty(0), err1=np.empty(0), status=np.empty(0, dtype=np.int64)))


def _fold_front(fn, models, two_models, kind=_PAIR_FOLDS):
    """(the call's models, the trained folds): models 2 t and 2 t + 1 are two_models(f, models[f]) of the t-th trained fold f; a fold
    that was not trained is passed over"""
    mods, trained = [], []
    for f, pair in enumerate(models):
        if kind[0](pair):
            continue
        if kind[1] and (not isinstance(pair, (tuple, list)) or len(pair) != 2):
            _ls_refuser(fn)(f"fold {f}: a model is a pair (res0, res1) or (0, 0)")
        mods += two_models(f, pair)
        trained.append(f)
    return mods, trained


def _residual_labels(f, r2, j0, j1):
    """"ols", "rls" and "vbls": err = norm(Y - BHat*AHat') (:483-484), label 1 where err0 > err1 (:487-491)"""
    err0, err1 = np.sqrt(r2[j0]), np.sqrt(r2[j1])
    return (err0 > err1).astype(np.int64), err0, err1


def _fold_jobs(fn, models, ids, two_models, call, result, failed, kind=_PAIR_FOLDS, model_flags=False):
    """What the fold functions share: every fold's test bags ids[f] against the fold's two models in one device call.
    two_models(f, models[f]): the fold's two call models, checked on the host (_fold_front).  The jobs are (bag, 2 t) for every test
    bag of the t-th trained fold, then (bag, 2 t + 1) for every one.  call(mods, job_bag, job_model) -> (r, flags): the one device call;
    flags[j] is set for a failed job (model_flags: flags[k] for a failed model, and b below is None).  result(f, r, j0, j1): fold f's
    result from r, j0 and j1 the slices of its jobs against its first and its second model.  Returns a list with result() per fold,
    None for an untrained fold, kind[2]() for one with no test bags.  If anything is flagged, VbmfError is raised after every fold
    has been computed -- f"{fn}: fold {f}: " + failed(k, b) for the first fold with a flag, k and b the model (0 / 1) and the bag of its
    first flagged job -- with .results the list, None in every such fold's place."""
    mods, trained = _fold_front(fn, models, two_models, kind)
    job_bag, job_model, where = [], [], {}
    for t, f in enumerate(trained):
        n = len(ids[f])
        if n:
            where[f] = (t, len(job_bag), n)
            job_bag += ids[f] + ids[f]
            job_model += [2 * t] * n + [2 * t + 1] * n
    out = [None if kind[0](pair) else kind[2]() for pair in models]
    if not job_bag:
        return out
    r, flags = call(mods, job_bag, job_model)
    for f, (t, j0, n) in where.items():
        out[f] = result(f, r, slice(j0, j0 + n), slice(j0 + n, j0 + 2 * n))
    bad = []
    for f, (t, j0, n) in where.items() if np.any(flags) else ():
        st = np.flatnonzero(flags[2 * t:2 * t + 2] if model_flags else flags[j0:j0 + 2 * n])
        if st.size:
            bad.append((f, int(st[0]), None) if model_flags else (f, int(st[0]) // n, ids[f][int(st[0]) % n]))
            out[f] = None
    if bad:                                                              # (a flagged basis whose fold has no test bags fails nothing)
        f, k, b = bad[0]
        e = VbmfError(capi.VBMF_ERR_NUMERIC, f"{fn}: fold {f}: " + failed(k, b))
        e.results = out
        raise e
    return out


def _classify_folds_dual(fn, models, ids, Ys, L, niter):
    """classify_folds' "dual" branch: the folds' sets as one call's models, two jobs per tested bag"""
    refuse = _ls_refuser(fn)
    if niter < 1:
        refuse(f"niter = {niter} < 1")
    Ms = Ys.Ms if isinstance(Ys, (BagPool, _Uploaded)) else [int(np.shape(Y)[1]) for Y in Ys]
    Hs = []                                                              # (the first trained fold's H is the call's)

    def two_models(f, pair):
        if any(isinstance(r, vbmf_trial_parameters) for r in pair):
            _score_refuser(fn)(f"fold {f}: " + _TRIAL_TWO_SETS)
        for k, r in enumerate(pair):
            if type(r) not in _JOBS_KINDS:
                refuse(f"fold {f}: res{k} is a {type(r).__name__} (class_alg = 'dual' takes vbmf_sparse_parameters or "
                       f"vbmf_dual_parameters sets)")
        if type(pair[0]) is not type(pair[1]) or int(pair[0].H) != int(pair[1].H):
            refuse(f"fold {f}: res0 is a {type(pair[0]).__name__} with H = {pair[0].H}, res1 a {type(pair[1]).__name__} with "
                   f"H = {pair[1].H} (one type and one H per fold)")
        Hs.append(int(pair[0].H))
        if Hs[0] > _JOBS_MAX_H:
            refuse(f"fold {f}: H = {Hs[0]} > {_JOBS_MAX_H}")
        return [_jobs_model(fn, r, L, Hs[0], f"fold {f}: res{k}", refuse) for k, r in enumerate(pair)]

    def call(mods, job_bag, job_model):
        r = _jobs_run(Ys, lambda ctx, off: ctx.sparse_fixed_basis_jobs(off, Hs[0], mods, job_bag, job_model, int(niter), full_cov=True))
        return r["r2"], r["status"]

    def labels(f, r2, j0, j1):
        scale = L * np.asarray([Ms[b] for b in ids[f]], dtype=np.float64)
        err0, err1 = np.sqrt(r2[j0]) / scale, np.sqrt(r2[j1]) / scale                           # :523-524
        return np.where(err0 < err1, 0, 1).astype(np.int64), err0, err1                         # :526-530
    return _fold_jobs(fn, models, ids, two_models, call, labels,
                      lambda k, b: f"vbls! of bag {b} against res{k} met a precision that is not finite or a pivot that is not positive "
                                   f"and finite")


def _vbls_two_models(fn, L):
    """the "vbls" classifier's two call models of a fold, checked on the host"""
    what = ("class_alg = 'vbls' takes the basic model's vbmf_parameters, as train_folds(..., 'basic') returns them; "
            "'ols', 'rls' or 'dual' take other models, and any pair of models runs per fold with classify_bags")
    return lambda f, pair: [_basic_jobs_model(r, L, f"fold {f}: res{k}", _ls_refuser(fn), what) for k, r in enumerate(pair)]


def _fold_models_vbls(fn, models, L):
    """(the call's models, the trained folds) of the "vbls" classifier, checked on the host: models 2 t and 2 t + 1 are the t-th trained
    fold's res0 and res1"""
    return _fold_front(fn, models, _vbls_two_models(fn, L))


def _classify_folds_vbls(fn, models, ids, Ys, L, niter):
    """classify_folds' "vbls" branch: the folds' basic-model sets as one call's models, two jobs per tested bag"""
    if niter < 1:
        _ls_refuser(fn)(f"niter = {niter} < 1")

    def call(mods, job_bag, job_model):
        r = _jobs_run(Ys, lambda ctx, off: ctx.fixed_basis_jobs(off, mods, job_bag, job_model, int(niter)))
        return r["r2"], r["status"]

    return _fold_jobs(fn, models, ids, _vbls_two_models(fn, L), call, _residual_labels,
                      lambda k, b: f"vbls! of bag {b} against res{k} met a pivot that is not positive and finite or ended with a sigma2, "
                                   f"CA or residual that is not finite")


def _scored_labels(r, class_alg, threshold):
    """classify's "lower_bound" (:502-514) or "min_err" (:493-501) triple from one fold's scores"""
    if r is None:
        return None
    if class_alg == "lower_bound":
        return (r["L1"] > r["L0"]).astype(np.int64), r["L0"], r["L1"]
    err0, err1 = r["err0"], r["err1"]
    with np.errstate(divide="ignore", invalid="ignore"):
        close = np.abs((err0 - err1) / err0) < threshold                 # :497
    return np.where(close, 0, 1).astype(np.int64), err0, err1


def _scored_model(res, H, d):
    """One model of Context.sparse_scored_jobs from the fields copy_vbmf_params keeps (d: BHat, SigmaB, CB, gamma, delta) and the
    sparse model's hyper-priors `res` carries (vbmf_sparse_init's defaults for the truncated basis); the start values are
    vbmf_sparse_init's (CA = ones, sigmaHat = 1)."""
    one = np.ones(H)
    return dict(BHat=d["BHat"], SigmaB=d["SigmaB"], CB=np.asarray(d["CB"], dtype=np.float64), delta=np.asarray(d["delta"], dtype=np.float64),
                gamma=float(d["gamma"]), gamma0=float(res.gamma0), delta0=float(res.delta0), a_pri=one * float(res.alpha0),
                b_pri=one * float(res.beta0), a_post=one * (float(res.alpha0) + 0.5), eta0=float(res.eta0), zeta0=float(res.zeta0),
                sigma0=1.0, ca0=1.0)


class _SparseInitPriors:
    """vbmf_sparse_init's default hyper-priors (src/vbmf_sparse.jl:101-103): what factorize_bag's truncated model carries (:398-404)"""
    alpha0 = beta0 = gamma0 = delta0 = eta0 = zeta0 = 1e-10


def _factorize_folds(fn, models, tests, Ys, niter, threshold, alg=None):
    """factorize_folds for fn; alg: the class_alg the refusal of a model names (None: factorize_bag itself)"""
    refuse = _ls_refuser(fn)
    what = "factorize_bag" if alg is None else f"class_alg = {alg!r}"
    if len(models) != len(tests):
        refuse(f"{len(models)} models but {len(tests)} test lists")
    if niter < 1:
        refuse(f"niter = {niter} < 1")
    threshold = float(threshold)
    if not np.isfinite(threshold) or threshold < 0.0:
        refuse(f"threshold = {threshold} (lowerBoundTrimmed takes a finite threshold >= 0)")
    L, Ms = _jobs_bags(fn, Ys, refuse)
    ids = _fold_ids(fn, tests, len(Ms))
    fulls = []                                                           # per trained fold and test bag: the full_cov form? (:405-409)

    def two_models(f, m):
        res = m[0] if isinstance(m, (tuple, list)) and len(m) == 2 else m            # (res0, anything): the second is not read (:610)
        if type(res) is not vbmf_sparse_parameters or not 0 < int(getattr(res, "H1", 0)) < int(res.H):
            refuse(f"fold {f}: {what} takes a vbmf_sparse_parameters with 0 < H1 < H (what train_local_folds returns), bare or first "
                   f"in a pair, not a {type(res).__name__}"
                   + (f" with H = {res.H}, H1 = {getattr(res, 'H1', None)}" if type(res) is vbmf_sparse_parameters else "")
                   + "; 'ols', 'rls' or 'dual' take other models, and any pair of models runs per fold with classify_bags")
        H = int(res.H)
        if H > _JOBS_MAX_H:
            refuse(f"fold {f}: H = {H} > {_JOBS_MAX_H}")
        B, SB = np.asarray(res.BHat, dtype=np.float64), np.asarray(res.SigmaB, dtype=np.float64)
        if B.shape != (L, H) or SB.shape != (H, H):
            refuse(f"fold {f}: BHat is {B.shape} and SigmaB {SB.shape}, the bags have L = {L} rows and H = {H}")
        if not all(np.all(np.isfinite(np.asarray(v, dtype=np.float64))) for v in (B, SB, res.CB, res.delta, res.gamma, res.gamma0, res.delta0,
                                                                                    res.alpha0, res.beta0, res.eta0, res.zeta0)):
            refuse(f"fold {f}: the model has a BHat, SigmaB, CB, delta, gamma or hyper-prior that is not finite")
        tb = _truncated_basis(res)
        fulls.append([Ms[b] * (H - int(res.H1)) < 1600 for b in ids[f]])
        return [_scored_model(_SparseInitPriors, tb["H"], tb),                                 # :398-404
                _scored_model(res, H, dict(BHat=B, SigmaB=SB, CB=res.CB, gamma=res.gamma, delta=res.delta))]

    def call(mods, job_bag, job_model):
        job_full, job_trim = [], []                                      # (the jobs' order: a fold's bags against 2 t, then against 2 t + 1)
        for ff in fulls:
            job_full += ff + ff
            job_trim += [-1.0] * len(ff) + [threshold] * len(ff)
        r = _jobs_run(Ys, lambda ctx, off: ctx.sparse_scored_jobs(off, mods, job_bag, job_model, job_full, job_trim, niter))
        return r, r["status"]

    def scores(f, r, j0, j1):
        return dict(L0=r["lb"][j0].copy(), L1=r["lb"][j1].copy(), err0=np.sqrt(r["r2"][j0]), err1=np.sqrt(r["r2"][j1]),
                    status=(r["status"][j0] | r["status"][j1]).astype(np.int64))
    return _fold_jobs(fn, models, ids, two_models, call, scores,
                      lambda k, b: f"vbls! of bag {b} against {'the whole' if k else 'the truncated'} basis met a precision that is not "
                                   f"finite or a pivot that is not positive and finite, or its bound is not finite", kind=_SCORED_FOLDS)


def factorize_folds(models, tests, Ys, niter=20, threshold=1e-1):
    """factorize_bag (examples/mil_util.jl:393-416) and its four scores for every fold's test bags in ONE device call
    (Context.sparse_scored_jobs): per tested bag 20 vbls! iterations against the fold's basis without its last H1 columns and 20
    against the whole basis, both in the full_cov form where M_b (H - H1) < 1600 (:405-409) and in the diagonal one otherwise, then
    lowerBound of the first fit, lowerBoundTrimmed(threshold) of the second, and the two residual norms.
    models[f]: the vbmf_sparse_parameters with 0 < H1 < H that train_local_folds returns for fold f, bare or as the first of a pair
    (res0, anything) -- the second is not read (:610) --, or (0, 0) / 0 for an untrained fold; the folds may differ in H <= 32 and
    H1.  tests[f]: bag indices into Ys; Ys: a BagPool (the call runs on the pool's own context), an uploaded Bags / SparseBags or a
    list of L x M_b matrices.
    The call's models are 2 t and 2 t + 1 for the t-th trained fold: the truncated basis with vbmf_sparse_init's default priors
    (:398-404), and what copy_vbmf_params keeps; its jobs (bag, 2 t, lowerBound) then (bag, 2 t + 1, lowerBoundTrimmed(threshold)).
    Returns per fold dict(L0, L1, err0, err1, status) with one entry per tested bag (err = norm(Y_b - BHat*AHat'), formed entry by
    entry on the device), None for an untrained fold.  A fold with a job the device flagged or whose bound is not finite raises
    VbmfError naming it after the others have been computed; the exception's .results holds them, None in that fold's place."""
    return _factorize_folds("factorize_folds", list(models), list(tests), Ys, int(niter), threshold)


def test_classification_folds(models, tests, Ys, labels, class_alg="ols", niter=None, threshold=None):
    """test_classification (examples/mil_util.jl:558-587) of every fold in one device call (classify_folds): a list with
    (mer, eer, fp, fn, n0, n1) per fold, counted as test_classification_batch counts, from the fold's estimated labels and
    labels[tests[f]].  labels: 0 / 1, one per bag of Ys.  A (0, 0) fold gives (-1.0,) * 6 (:612-614).  niter, threshold:
    classify_folds', handed on only when given."""
    fn = "test_classification_folds"
    _fold_alg_scored(fn, class_alg)
    models, tests = list(models), list(tests)
    if len(models) != len(tests):
        _ls_refuser(fn)(f"{len(models)} models but {len(tests)} test lists")
    L, nb = _folds_bags(fn, Ys)
    labels = _fold_labels(fn, labels, nb)
    ids = _fold_ids(fn, tests, nb)
    if class_alg == "vbls":
        _fold_models_vbls(fn, models, L)                                 # (its refusals under this function's name)
    out = []
    kw = {k: v for k, v in (("niter", niter), ("threshold", threshold)) if v is not None}
    for t, r in zip(ids, classify_folds(models, ids, Ys, class_alg, **kw)):
        if r is None:
            out.append((-1.0,) * 6)
        else:
            out.append(_classification_counts(fn, labels[np.asarray(t, dtype=np.int64)], np.asarray(r[0]).reshape(-1)))
    return out


test_classification_folds.__test__ = False        # (named after the reference's test_classification; not a test)


def validate_folds(pool, labels, splits, solver, H, niter, eps=1e-6, class_alg="ols", rng=None, form="stream", slice_cols=None, H1=1,
                   diag_var=False, nstarts=10):
    """validate_with_cvs (examples/mil_util.jl:627-648) over all splits = [(train_ids, test_ids), ...] of a BagPool in two device
    calls: one train_folds(..., pool=pool) on the folds' training groups -- the train_ids with label 0 and those with label 1, in the
    order given (get_matrices, :46) -- and one test_classification_folds on the test_ids.  labels: 0 / 1, one per bag of the pool;
    solver, H, niter, eps, rng, form, slice_cols: train_folds'; class_alg: "ols", "rls", "dual", or "vbls" with solver = "basic" (the
    basic model's classifier, :469-479: H <= 32).  With "dual" the third branch of
    validate_with_cvs (:633-634) runs instead: train_dual_folds(folds, H, H - H1, niter, eps, diag_var=diag_var, nstarts=nstarts,
    pool=pool) trains and solver is not read; H1, diag_var and nstarts are read by that branch only.  Returns the list of
    (mer, eer, fp, fn, n0, n1) per split, (-1.0,) * 6 for a split with an empty class."""
    fn = "validate_folds"
    refuse = _ls_refuser(fn)
    _fold_alg(fn, class_alg)
    if class_alg == "vbls" and solver != "basic":
        refuse(f"class_alg = 'vbls' with solver = {solver!r} (it takes the basic model's vbmf_parameters: solver = 'basic'; 'ols', 'rls' or "
               f"'dual' take the other solvers' models, and any pair of models runs per fold with classify_bags)")
    if not isinstance(pool, BagPool):
        refuse(f"pool is a {type(pool).__name__}, not a BagPool")
    _, nb = _folds_bags(fn, pool)
    if int(H) > (_JOBS_MAX_H if class_alg == "vbls" else _LS_MAX_H):
        refuse(f"H = {int(H)} > {_JOBS_MAX_H if class_alg == 'vbls' else _LS_MAX_H}")
    labels = _fold_labels(fn, labels, nb)
    splits = [tuple(s) for s in splits]
    if any(len(s) != 2 for s in splits):
        refuse("every split is a pair (train_ids, test_ids)")
    train = _fold_ids(fn, [s[0] for s in splits], nb)
    tests = _fold_ids(fn, [s[1] for s in splits], nb)
    folds = [([b for b in t if labels[b] == 0], [b for b in t if labels[b] == 1]) for t in train]
    if class_alg == "dual":
        models = train_dual_folds(folds, H, int(H) - int(H1), niter, eps=eps, diag_var=diag_var, nstarts=nstarts, rng=rng, form=form,
                                  slice_cols=slice_cols, pool=pool)
    else:
        models = train_folds(folds, solver, H, niter, eps=eps, rng=rng, form=form, slice_cols=slice_cols, pool=pool)
    return test_classification_folds(models, tests, pool, labels, class_alg)


def validate_local_folds(pool, labels, splits, H, H1, niter, eps=1e-6, class_alg="lower_bound", threshold=1e-1, diag_var=False, rng=None,
                         form="stream", slice_cols=None):
    """The train_local branch of validate_with_cvs (examples/mil_util.jl:635-637, "the better approach") over all splits =
    [(train_ids, test_ids), ...] of a BagPool: one train_local_folds(folds, H, H1, niter, eps, pool=pool) per round on the folds'
    training groups (as validate_folds forms them) and one test_classification_folds on the test_ids with class_alg "lower_bound" or
    "min_err" (factorize_folds: one device call).  labels: 0 / 1, one per bag of the pool; threshold: classify's; diag_var, rng,
    form, slice_cols: train_local_folds'.  Returns the list of (mer, eer, fp, fn, n0, n1) per split."""
    fn = "validate_local_folds"
    refuse = _ls_refuser(fn)
    if class_alg not in _FOLD_SCORED_ALGS:
        refuse(f"class_alg = {class_alg!r} ('lower_bound' or 'min_err': the classifiers of a train_local model; validate_folds takes "
               f"'ols', 'rls' and 'dual')")
    if not isinstance(pool, BagPool):
        refuse(f"pool is a {type(pool).__name__}, not a BagPool")
    _, nb = _folds_bags(fn, pool)
    if int(H) > _JOBS_MAX_H:
        refuse(f"H = {int(H)} > {_JOBS_MAX_H}")
    if not 0 < int(H1) < int(H):
        refuse(f"H1 = {int(H1)} (factorize_bag needs 0 < H1 < H = {int(H)})")
    labels = _fold_labels(fn, labels, nb)
    splits = [tuple(s) for s in splits]
    if any(len(s) != 2 for s in splits):
        refuse("every split is a pair (train_ids, test_ids)")
    train = _fold_ids(fn, [s[0] for s in splits], nb)
    tests = _fold_ids(fn, [s[1] for s in splits], nb)
    folds = [([b for b in t if labels[b] == 0], [b for b in t if labels[b] == 1]) for t in train]
    models = train_local_folds(folds, H, H1, niter, eps=eps, rng=rng, diag_var=diag_var, form=form, slice_cols=slice_cols, pool=pool)
    return test_classification_folds(models, tests, pool, labels, class_alg, threshold=threshold)


# =================================================================================================
# Pre-processing -- src/util.jl:36-97 (the step before the factorization: examples/mil_util.jl:829)
# =================================================================================================
def scaleY(Y):
    """scaleY -- src/util.jl:36-54 (host array in, host array out, like the reference)."""
    Y = np.asarray(Y, dtype=np.float64)
    mu = Y.mean(axis=1, keepdims=True)
    den = Y.var(axis=1, ddof=1, keepdims=True)
    den = np.where(np.abs(den) <= 1e-15, 1.0, den)
    nom = Y - mu
    nom[np.abs(nom) <= 1e-8] = 0.0
    return nom / np.sqrt(den)


def preprocess(Y, lam, verb=False):
    """preprocess -- src/util.jl:73-86 with the reference's call shape (returns lambda * scaled kept rows as a host
    array).  To avoid materialising it, use `preprocessed_session`, which standardises, filters and scales inside the
    upload (PreprocessPlan + Context.set_Y_preprocessed) and never builds the L x M temporaries."""
    sY = scaleY(Y)
    used = np.nonzero(np.abs(sY).sum(axis=1) >= 1e-5)[0]
    if verb:
        print(f"Original problem size: {Y.shape[0]} rows, {Y.shape[0] - used.size} rows not relevant and are not used.")
    return lam * sY[used, :]


def preprocessed_session(Y, lam, H, **ctx_kw):
    """Device-side preprocess: returns (Session over the pre-processed matrix, kept rows 0-based).  The Session's
    ctx holds lambda * scaleY(Y)[kept rows] in the device dtype; use Session.run / push / pull with parameters
    created for L = len(kept rows)."""
    with PreprocessPlan(Y) as plan:
        rows, _, _ = plan.rows()
        s = Session(plan.L_used, plan.M, int(H), **ctx_kw)
        s.ctx.set_Y_preprocessed(plan, lam)
    return s, rows
