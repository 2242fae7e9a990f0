"""Many fits in one device call (vbmf_sparse_fit_batched / vbmf_sparse_batch_ / vbmf_dual_batch_ / fit_restarts): the parts that need
no GPU -- the C ABI is declared, exported and bound, the Julia host binds it, the Python hosts refuse what the batched path does not
cover BEFORE any device call, and fit_restarts returns the set the reference's restart loops would have returned."""
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
    assert re.search(r"int\s+vbmf_sparse_fit_batched\s*\(\s*vbmf_ctx\*\s*ctx\s*,\s*int64_t\s+nbags\s*,\s*const\s+int64_t\*\s*col_off\s*,\s*"
                     r"int64_t\s+nfits\s*,\s*const\s+int64_t\*\s*fit_bag\s*,\s*int64_t\s+niter\s*,\s*double\s+eps\s*,\s*int\s+full_cov\s*,\s*"
                     r"int\s+est_cb\s*,\s*int\s+est_priors\s*,\s*int64_t\s+H0", hdr)
    assert "examples/mil_util.jl:124-145,347-379" in hdr
    assert hasattr(ctypes.CDLL(pkg.capi.LIB_PATH), "vbmf_sparse_fit_batched")
    assert "vbmf_sparse_fit_batched" in pkg.capi.SYMBOLS
    assert len(pkg.capi.lib().vbmf_sparse_fit_batched.argtypes) == 31
    assert hasattr(pkg.capi.Context, "sparse_fit_batched")
    for name in ("vbmf_sparse_batch_", "vbmf_dual_batch_", "fit_restarts"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))


def test_julia_host_binds_it():
    jl = open(os.path.join(G.PKG_DIR, "julia", "VBMatrixFactorizationHIP.jl")).read()
    assert re.search(r"ccall\(\(:vbmf_sparse_fit_batched,\s*libvbmf\)", jl)
    assert re.search(r"function vbmf_sparse_batch!\(Ys::Vector\{Matrix\{Float64\}\},\s*ps::Vector\{vbmf_sparse_parameters\},\s*niter::Int;", jl)
    assert re.search(r"function vbmf_dual_batch!\(Ys::Vector\{Matrix\{Float64\}\},\s*ps::Vector\{vbmf_dual_parameters\},\s*niter::Int;", jl)
    assert re.search(r"export[^\n]*\n?[^\n]*vbmf_sparse_batch!,\s*vbmf_dual_batch!", jl)


@pytest.fixture
def no_device(pkg, monkeypatch):
    """Any attempt to reach the library fails the test (the refusals happen on the host)."""
    def boom(*a, **k):
        raise AssertionError("the batched fit touched the device before refusing")
    monkeypatch.setattr(pkg.capi, "lib", boom)
    monkeypatch.setattr(pkg.capi.Context, "__init__", boom)
    monkeypatch.setattr(pkg.Session, "__init__", boom)
    return pkg


def _fits(pkg, kind="sparse", L=30, Ms=(3, 1, 7), H=4, seed=0, bag_of=None):
    rng = np.random.default_rng(seed)
    Ys = [rng.standard_normal((L, m)) for m in Ms]
    bag_of = range(len(Ms)) if bag_of is None else bag_of
    if kind == "sparse":
        return Ys, [pkg.vbmf_sparse_init(Ys[b], H, rng=rng) for b in bag_of]
    return Ys, [pkg.vbmf_dual_init(Ys[b], H, max(1, H // 2), rng=rng) for b in bag_of]


def _refused(pkg, kind, Ys, ps, match=None, niter=10, **kw):
    fit = pkg.vbmf_sparse_batch_ if kind == "sparse" else pkg.vbmf_dual_batch_
    kw.setdefault("full_cov", True)
    with pytest.raises(ValueError, match=match or ("vbmf_sparse_batch_" if kind == "sparse" else "vbmf_dual_batch_")):
        fit(Ys, ps, niter, **kw)


@pytest.mark.parametrize("kind", ["sparse", "dual"])
def test_refusals_happen_on_the_host(no_device, kind):
    pkg = no_device
    Ys, ps = _fits(pkg, kind)
    Ys[1] = np.zeros((31, 1))
    _refused(pkg, kind, Ys, ps)                                     # mismatched L
    Ys, ps = _fits(pkg, kind)
    ps[0], ps[2] = ps[2], ps[0]
    _refused(pkg, kind, Ys, ps)                                     # parameters of another bag's shape
    Ys, ps = _fits(pkg, kind)
    _refused(pkg, kind, Ys, ps[:2], match="bag_of")                 # fewer sets than bags and no bag_of
    _refused(pkg, kind, Ys, ps, match="bag_of", bag_of=[0, 1, 3])   # a bag that does not exist
    _refused(pkg, kind, Ys, ps, match="bag_of", bag_of=[0, 1])
    _refused(pkg, kind, Ys, [], match="no parameter sets")
    _refused(pkg, kind, Ys, ps, match="niter", niter=0)
    _refused(pkg, kind, Ys, ps, match="1-column", full_cov=False)   # the diagonal form under the repeat layout needs M >= 2
    ps[1].CA = np.ones(5)
    _refused(pkg, kind, Ys, ps)
    Ys, ps = _fits(pkg, kind)
    ps[1].BHat = ps[1].BHat[:-1]
    _refused(pkg, kind, Ys, ps)
    Ys, ps = _fits(pkg, kind)
    ps[1].eta = ps[1].eta + 3.0
    _refused(pkg, kind, Ys, ps, match="eta")
    Ys, ps = _fits(pkg, kind, H=33)
    _refused(pkg, kind, Ys, ps, match="32")
    Ys, ps = _fits(pkg, kind)
    other = _fits(pkg, "dual" if kind == "sparse" else "sparse")[1]
    ps[1] = other[1]
    _refused(pkg, kind, Ys, ps, match="one model type")
    # restarts: several sets on one bag are fine as far as the host checks go, and the first device call is the upload
    Ys, ps = _fits(pkg, kind, bag_of=[2, 2, 0])
    with pytest.raises(AssertionError, match="touched the device"):
        (pkg.vbmf_sparse_batch_ if kind == "sparse" else pkg.vbmf_dual_batch_)(Ys, ps, 10, bag_of=[2, 2, 0])


def test_refuses_labels_and_mixed_H0(no_device):
    pkg = no_device
    Ys, ps = _fits(pkg, "sparse")
    ps[0].labels = np.array([1], dtype=np.int64)
    ps[0].H1 = 1
    _refused(pkg, "sparse", Ys, ps, match="label")
    Ys, ps = _fits(pkg, "dual")
    ps[2] = pkg.vbmf_dual_init(Ys[2], 4, 3, rng=np.random.default_rng(1))
    _refused(pkg, "dual", Ys, ps, match="H0")


def test_fit_restarts_refuses_diag_var_with_a_pointer(no_device):
    pkg = no_device
    with pytest.raises(ValueError, match="vbmf_sparse_ / vbmf_dual_"):
        pkg.fit_restarts(np.zeros((5, 4)), 2, 10, diag_var=True)
    with pytest.raises(ValueError, match="model"):
        pkg.fit_restarts(np.zeros((5, 4)), 2, 10, model="trial")


def _scripted(pkg, monkeypatch, name, outcomes):
    """replaces the batch call by one that leaves the scripted outcome on every set and records what it was given"""
    seen = {}

    def fake(Ys, params, niter, **kw):
        seen.update(Ys=Ys, params=list(params), niter=niter, kw=kw, B0=[p.BHat.copy() for p in params])
        for p, out in zip(params, outcomes):
            if name == "vbmf_dual_batch_":
                p.AHat, p.BHat = out[0] * np.ones_like(p.AHat), out[1] * np.ones_like(p.BHat)
        return [o if np.isscalar(o) else 0.5 for o in outcomes]
    monkeypatch.setattr(pkg, name, fake)
    return seen


def test_fit_restarts_sparse_picks_the_references_set(pkg, monkeypatch):
    Y = np.random.default_rng(0).standard_normal((12, 9))
    eps = 1e-6
    # :127-134: restart while delta > 2 eps, a NaN counts as not converged
    for outcomes, want in (([1e-7, 0.3, 1e-7, 0.2], 0),             # the first is accepted
                           ([0.3, np.nan, 2e-6, 1e-7], 2),          # NaN skipped, d = 2 eps accepted
                           ([0.3, np.nan, 2.1e-6, np.nan], 3)):     # none accepted: the last
        seen = _scripted(pkg, monkeypatch, "vbmf_sparse_batch_", outcomes)
        p = pkg.fit_restarts(Y, 3, 50, model="sparse", nstarts=4, eps=eps, rng=np.random.default_rng(5))
        assert p is seen["params"][want]
        assert seen["kw"]["bag_of"] == [0, 0, 0, 0] and seen["kw"]["full_cov"] is False and seen["niter"] == 50
        assert len(seen["Ys"]) == 1 and seen["Ys"][0] is Y
        # the initialisations are drawn in order from the one generator, as the loop would have drawn them
        rng = np.random.default_rng(5)
        for B0 in seen["B0"]:
            assert np.array_equal(B0, pkg.vbmf_sparse_init(Y, 3, rng=rng).BHat)


def test_fit_restarts_dual_picks_the_references_set(pkg, monkeypatch):
    Y = np.random.default_rng(0).standard_normal((12, 9))
    # :348-354: restart while norm(AHat) + norm(BHat) < 1e-2 (operator 2-norms: ones(M, H) c has norm c sqrt(M H))
    z = 1e-6
    for outcomes, want in (([(1.0, 1.0), (z, z), (1.0, 1.0)], 0),
                           ([(z, z), (z, 1.0), (1.0, 1.0)], 1),
                           ([(z, z), (z, z), (z, z)], 2)):
        seen = _scripted(pkg, monkeypatch, "vbmf_dual_batch_", outcomes)
        p = pkg.fit_restarts(Y, 4, 20, model="dual", H0=1, nstarts=3, rng=np.random.default_rng(5))
        assert p is seen["params"][want]
        assert seen["kw"]["full_cov"] is True and seen["kw"]["eps"] == 1e-4 and seen["kw"]["bag_of"] == [0, 0, 0]
        assert all(q.H0 == 1 for q in seen["params"])
