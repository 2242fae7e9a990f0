"""Many basic-model fits in one device call (vbmf_fit_batched / vbmf_batch_ / train_folds): the parts that need no GPU -- the C ABI is
declared, exported and bound, the Julia host binds it, vbmf_batch_ refuses what the batched path does not cover BEFORE any device call,
and train_folds draws its start values in the reference's order and returns the sets the reference's train would have returned."""
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as G

ROOT = G.ROOT


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


def test_header_declares_and_library_exports(pkg):
    hdr = open(os.path.join(ROOT, "include", "vbmf_hip.h")).read()
    assert re.search(r"int\s+vbmf_fit_batched\s*\(\s*vbmf_ctx\*\s*ctx\s*,\s*int64_t\s+nbags\s*,\s*const\s+int64_t\*\s*col_off\s*,\s*"
                     r"int64_t\s+nfits\s*,\s*const\s+int64_t\*\s*fit_bag\s*,\s*int64_t\s+niter\s*,\s*double\s+eps\s*,\s*int\s+est_covs\s*,\s*"
                     r"int\s+est_var\s*,\s*double\*\s*BHat\s*,\s*double\*\s*SigmaB\s*,\s*double\*\s*CA\s*,\s*double\*\s*CB\s*,\s*"
                     r"double\*\s*sigma2\s*,\s*double\*\s*AHat\s*,\s*double\*\s*SigmaA\s*,\s*int64_t\*\s*iters_done\s*,\s*"
                     r"double\*\s*d_last\s*,\s*int64_t\*\s*status\s*,\s*double\*\s*trace\s*\)", hdr)
    assert "examples/mil_util.jl:110-114" in hdr and "src/vbmf.jl:175-231" in hdr
    assert hasattr(ctypes.CDLL(pkg.capi.LIB_PATH), "vbmf_fit_batched")
    assert "vbmf_fit_batched" in pkg.capi.SYMBOLS
    assert len(pkg.capi.lib().vbmf_fit_batched.argtypes) == 20
    assert hasattr(pkg.capi.Context, "fit_batched")
    for name in ("vbmf_batch_", "train_folds"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))


def test_julia_host_binds_it():
    jl = open(os.path.join(G.PKG_DIR, "julia", "VBMatrixFactorizationHIP.jl")).read()
    assert re.search(r"ccall\(\(:vbmf_fit_batched,\s*libvbmf\)", jl)
    assert re.search(r"function vbmf_batch!\(Ys::Vector\{Matrix\{Float64\}\},\s*ps::Vector\{vbmf_parameters\},\s*niter::Int;\s*eps::Float64[^)]*"
                     r"est_covs::Bool[^)]*est_var::Bool[^)]*bag_of::Vector\{Int\}", jl)
    assert re.search(r"export[^\n]*\n?[^\n]*\bvbmf_batch!", jl)


@pytest.fixture
def no_device(pkg, monkeypatch):
    """Any attempt to reach the library fails the test (the refusals happen on the host)."""
    def boom(*a, **k):
        raise AssertionError("the batched fit touched the device before refusing")
    monkeypatch.setattr(pkg.capi, "lib", boom)
    monkeypatch.setattr(pkg.capi.Context, "__init__", boom)
    monkeypatch.setattr(pkg.Session, "__init__", boom)
    return pkg


def _fits(pkg, L=30, Ms=(3, 1, 7), H=4, seed=0, bag_of=None):
    rng = np.random.default_rng(seed)
    Ys = [rng.standard_normal((L, m)) for m in Ms]
    bag_of = range(len(Ms)) if bag_of is None else bag_of
    return Ys, [pkg.vbmf_init(Ys[b], H, rng=rng) for b in bag_of]


def _refused(pkg, Ys, ps, match=None, niter=10, **kw):
    with pytest.raises(ValueError, match=match or "vbmf_batch_") as e:
        pkg.vbmf_batch_(Ys, ps, niter, **kw)
    assert "vbmf_batch_" in str(e.value) and "with vbmf_" in str(e.value)       # names itself, points to the per-fit call


def test_refusals_happen_on_the_host(no_device):
    pkg = no_device
    Ys, ps = _fits(pkg)
    Ys[1] = np.zeros((31, 1))
    _refused(pkg, Ys, ps, match="row counts")                       # mismatched L
    Ys, ps = _fits(pkg)
    Ys[2] = np.zeros(30)
    _refused(pkg, Ys, ps, match="matrix")                           # a bag that is no matrix
    Ys, ps = _fits(pkg)
    ps[0], ps[2] = ps[2], ps[0]
    _refused(pkg, Ys, ps, match="its parameters describe")          # parameters of another bag's shape
    Ys, ps = _fits(pkg)
    ps[1].BHat = ps[1].BHat[:-1]
    _refused(pkg, Ys, ps, match="shape")
    Ys, ps = _fits(pkg)
    ps[1].CA = np.ones(4)                                           # a vector where the basic model keeps a matrix
    _refused(pkg, Ys, ps, match="shape")
    Ys, ps = _fits(pkg)
    ps[2] = pkg.vbmf_init(Ys[2], 3, rng=np.random.default_rng(1))
    _refused(pkg, Ys, ps, match="H = 3 beside H = 4")               # mixed H
    Ys, ps = _fits(pkg)
    ps[1] = pkg.vbmf_sparse_init(Ys[1], 4, rng=np.random.default_rng(1))
    _refused(pkg, Ys, ps, match="vbmf_sparse_parameters")           # a wrong parameter type
    _refused(pkg, Ys, [ps[1], ps[0], ps[2]], match="vbmf_sparse_parameters")
    Ys, ps = _fits(pkg)
    ps[0].labels = np.array([1], dtype=np.int64)
    ps[0].H1 = 1
    _refused(pkg, Ys, ps, match="label")
    Ys, ps = _fits(pkg)
    _refused(pkg, Ys, ps[:2], match="bag_of")                       # fewer sets than bags and no bag_of
    _refused(pkg, Ys, ps, match="bag_of", bag_of=[0, 1, 3])         # a bag that does not exist
    _refused(pkg, Ys, ps, match="bag_of", bag_of=[0, -1, 2])
    _refused(pkg, Ys, ps, match="bag_of", bag_of=[0, 1])
    _refused(pkg, Ys, [], match="no parameter sets")
    _refused(pkg, Ys, ps, match="niter", niter=0)
    Ys, ps = _fits(pkg, H=33)
    _refused(pkg, Ys, ps, match="32")
    # restarts on one bag and a 1-column bag are fine as far as the host checks go: the first device call is the upload
    Ys, ps = _fits(pkg, bag_of=[2, 2, 1])
    with pytest.raises(AssertionError, match="touched the device"):
        pkg.vbmf_batch_(Ys, ps, 10, bag_of=[2, 2, 1])


def test_train_folds_refuses_before_any_draw(no_device):
    pkg = no_device
    Y = np.zeros((5, 4))
    with pytest.raises(ValueError, match="solver"):
        pkg.train_folds([(Y, Y)], "dual", 2, 10)
    with pytest.raises(ValueError, match=r"vbmf_sparse_ / vbmf_"):   # points to the per-fit calls
        pkg.train_folds([(Y, Y)], "sparse", 2, 10, diag_var=True)
    with pytest.raises(ValueError, match="diag_var"):
        pkg.train_folds([(Y, Y)], "basic", 2, 10, diag_var=True)


def _folds(L=12, shapes=((9, 4), (0, 5), (3, 7), (6, 0))):
    rng = np.random.default_rng(0)
    return [(rng.standard_normal((L, a)), rng.standard_normal((L, b))) for a, b in shapes]


def _scripted(pkg, monkeypatch, name, ds):
    """replaces the batch call by one that records what it was given; the sparse one returns the scripted d per set"""
    seen = {}

    def fake(Ys, params, niter, **kw):
        seen.update(Ys=list(Ys), params=list(params), niter=niter, kw=kw, B0=[p.BHat.copy() for p in params])
        return list(params) if name == "vbmf_batch_" else list(ds)
    monkeypatch.setattr(pkg, name, fake)
    return seen


def test_train_folds_basic_draws_in_order_and_returns_every_set(pkg, monkeypatch):
    folds = _folds()
    seen = _scripted(pkg, monkeypatch, "vbmf_batch_", None)
    out = pkg.train_folds(folds, "basic", 3, 50, eps=1e-3, rng=np.random.default_rng(5))
    assert len(out) == 4 and out[1] == (0, 0) and out[3] == (0, 0)  # examples/mil_util.jl:97-100
    assert seen["niter"] == 50 and seen["kw"] == dict(eps=1e-3, est_covs=True, est_var=True, bag_of=[0, 1, 2, 3])
    assert [Y is W for Y, W in zip(seen["Ys"], (folds[0][0], folds[0][1], folds[2][0], folds[2][1]))] == [True] * 4
    assert out[0][0] is seen["params"][0] and out[0][1] is seen["params"][1]
    assert out[2][0] is seen["params"][2] and out[2][1] is seen["params"][3]
    rng = np.random.default_rng(5)                                  # one generator, (fold, class) order, skipped pairs draw nothing
    for B0, Y in zip(seen["B0"], seen["Ys"]):
        assert np.array_equal(B0, pkg.vbmf_init(Y, 3, rng=rng).BHat)
    assert all(type(p) is pkg.vbmf_parameters for p in seen["params"])


def test_train_folds_sparse_keeps_the_references_set(pkg, monkeypatch):
    folds = _folds(shapes=((9, 4), (0, 5), (3, 7)))
    eps = 1e-6
    nan = np.nan
    # per class ten restarts (:108): restart while delta > 2 eps, a NaN counts as not converged (:127-134)
    ds = ([1e-7] + [0.3] * 9                                        # fold 0, class 0: the first is accepted
          + [0.3, nan, 2e-6] + [1e-7] * 7                           # fold 0, class 1: NaN skipped, d = 2 eps accepted
          + [0.3, nan] * 5                                          # fold 2, class 0: none accepted -> the last
          + [2.1e-6] * 9 + [1e-9])                                  # fold 2, class 1: the last, accepted
    seen = _scripted(pkg, monkeypatch, "vbmf_sparse_batch_", ds)
    out = pkg.train_folds(folds, "sparse", 3, 50, eps=eps, rng=np.random.default_rng(5))
    P = seen["params"]
    assert len(P) == 40 and seen["niter"] == 50
    assert seen["kw"] == dict(eps=eps, full_cov=False, bag_of=[b for b in range(4) for _ in range(10)])
    assert out[1] == (0, 0)
    assert out[0][0] is P[0] and out[0][1] is P[12] and out[2][0] is P[29] and out[2][1] is P[39]
    rng = np.random.default_rng(5)                                  # (fold, class, restart) order from the one generator
    for B0, b in zip(seen["B0"], seen["kw"]["bag_of"]):
        assert np.array_equal(B0, pkg.vbmf_sparse_init(seen["Ys"][b], 3, rng=rng).BHat)


def test_train_folds_with_nothing_to_fit(no_device):
    pkg = no_device
    assert pkg.train_folds([(np.zeros((4, 0)), np.zeros((4, 3)))], "basic", 2, 10) == [(0, 0)]
    assert pkg.train_folds([], "sparse", 2, 10) == []
