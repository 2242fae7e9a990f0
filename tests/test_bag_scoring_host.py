"""Scoring many bags in one device call (vbmf_bag_residuals, vbmf_sparse_lower_bound_batched; residual_batch, lowerBound_batch,
lowerBoundTrimmed_batch, classify_batch): the parts that need no GPU -- the C ABI is declared, exported and bound by both hosts,
the Python host refuses what the batched path does not cover BEFORE any device call, and the "lower_bound" classifier cuts the
basis and splits the bags the way factorize_bag does (examples/mil_util.jl:393-416)."""
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as G
from tests.test_julia_binding import header_prototypes

ROOT = G.ROOT
ENTRIES = ("vbmf_bag_residuals", "vbmf_sparse_lower_bound_batched")


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


def test_public_names(pkg):
    for name in ("residual_batch", "lowerBound_batch", "lowerBoundTrimmed_batch", "classify_batch"):
        assert hasattr(pkg, name) and name in pkg.__all__, name
    for name in ("bag_residuals", "sparse_lower_bound_batched"):
        assert hasattr(pkg.capi.Context, name), name


def test_header_declares_and_library_exports(pkg):
    protos = header_prototypes()
    assert set(pkg.capi.SYMBOLS) == set(protos)
    lib = ctypes.CDLL(pkg.capi.LIB_PATH)
    for name in ENTRIES:
        assert name in protos and hasattr(lib, name) and name in pkg.capi.SYMBOLS
        assert len(getattr(pkg.capi.lib(), name).argtypes) == len(protos[name][1])
    hdr = open(os.path.join(ROOT, "include", "vbmf_hip.h")).read()
    for cite in ("examples/mil_util.jl:476-479", "examples/mil_util.jl:502-514", "src/vbmf_sparse.jl:478-489", "src/vbmf_dual.jl:556-599",
                 "src/vbmf_trial.jl:630-680"):
        assert cite in hdr, cite


def test_new_kernels_live_in_their_own_header():
    src = open(os.path.join(G.PKG_DIR, "csrc", "score_kernels.hpp")).read()
    for k in ("bag_resid_kernel", "bag_resid_fold_kernel", "bag_lb_sums_kernel"):
        assert re.search(r"__global__[^;{]*\b" + k + r"\b", src), k
    hip = open(os.path.join(G.PKG_DIR, "csrc", "vbmf_hip.hip")).read()
    assert '#include "score_kernels.hpp"' in hip
    # one assembly routine for the per-context and the per-bag bound (the per-bag entry lives in host_bags.hpp, part of the same
    # translation unit)
    assert '#include "host_bags.hpp"' in hip
    bags = open(os.path.join(G.PKG_DIR, "csrc", "host_bags.hpp")).read()
    assert hip.count("lb_assemble(s, clamp)") == 1 and bags.count("lb_assemble(s, clamp)") == 1


def test_julia_host_binds_them():
    jl = open(os.path.join(G.PKG_DIR, "julia", "VBMatrixFactorizationHIP.jl")).read()
    for name in ENTRIES:
        assert re.search(r"ccall\(\(:" + name + r",\s*libvbmf\)", jl), name
    for fn in ("residual_batch", "lowerBound_batch", "lowerBoundTrimmed_batch"):
        assert re.search(r"^(function )?" + fn + r"\(", jl, flags=re.M), fn
        assert re.search(r"export[^\n]*(\n\s+[^\n]*)*\b" + fn + r"\b", jl), fn


@pytest.fixture
def no_device(pkg, monkeypatch):
    """Any attempt to reach the library fails the test (the refusals happen on the host)."""
    def boom(*a, **k):
        raise AssertionError("the scoring host touched the device before refusing")
    monkeypatch.setattr(pkg.capi, "lib", boom)
    monkeypatch.setattr(pkg.capi.Context, "__init__", boom)
    monkeypatch.setattr(pkg.Session, "__init__", boom)
    return pkg


def _trained(pkg, kind, L, H, rng):
    Ytr = rng.standard_normal((L, 20))
    if kind == "basic":
        return pkg.vbmf_init(Ytr, H, rng=rng)
    if kind == "sparse":
        return pkg.vbmf_sparse_init(Ytr, H, rng=rng)
    if kind == "dual":
        return pkg.vbmf_dual_init(Ytr, H, max(1, H // 2), rng=rng)
    return pkg.vbmf_trial_init(Ytr, H, max(1, H // 2), 12, rng=rng)


def _bags(pkg, kind="sparse", L=30, Ms=(3, 1, 7), H=4, seed=0):
    rng = np.random.default_rng(seed)
    Ys = [rng.standard_normal((L, m)) for m in Ms]
    res = _trained(pkg, kind, L, H, rng)
    ps = []
    for Y in Ys:
        q = pkg.copy_vbmf_params(Y, res, rng=np.random.default_rng(1))
        ps.append(q[0] if isinstance(q, tuple) else q)
    return Ys, ps, res


def _scorers(pkg, kind):
    fs = [("residual_batch", lambda Ys, ps: pkg.residual_batch(Ys, ps))]
    if kind != "basic":
        fs += [("lowerBound_batch", lambda Ys, ps: pkg.lowerBound_batch(Ys, ps)),
               ("lowerBoundTrimmed_batch", lambda Ys, ps: pkg.lowerBoundTrimmed_batch(Ys, ps, 0.1))]
    return fs


def _refused(pkg, kind, Ys, ps, match=""):
    for name, f in _scorers(pkg, kind):
        with pytest.raises(ValueError, match=name + ".*" + match):
            f(Ys, ps)


@pytest.mark.parametrize("kind", ["basic", "sparse", "dual", "trial"])
def test_refuses_wrong_bag_count_and_shapes(no_device, kind):
    pkg = no_device
    Ys, ps, _ = _bags(pkg, kind)
    _refused(pkg, kind, Ys, ps[:2], "3 bags but 2 parameter sets")
    Ys, ps, _ = _bags(pkg, kind)
    ps[0], ps[2] = ps[2], ps[0]
    _refused(pkg, kind, Ys, ps)
    Ys, ps, _ = _bags(pkg, kind)
    Ys[1] = np.zeros((31, 1))
    _refused(pkg, kind, Ys, ps, "row counts")
    _refused(pkg, kind, [], [])


def test_refuses_mixed_types(no_device):
    pkg = no_device
    Ys, ps, _ = _bags(pkg, "sparse")
    _, pd, _ = _bags(pkg, "dual")
    ps[1] = pd[1]
    _refused(pkg, "sparse", Ys, ps, "one model type")
    Ys, pb, _ = _bags(pkg, "basic")
    _, psp, _ = _bags(pkg, "sparse")
    pb[2] = psp[2]
    _refused(pkg, "basic", Ys, pb, "vbmf_parameters only")
    # the bound is not defined for the basic model
    Ys, pb, _ = _bags(pkg, "basic")
    with pytest.raises(ValueError, match="lowerBound_batch"):
        pkg.lowerBound_batch(Ys, pb)


@pytest.mark.parametrize("kind", ["basic", "sparse", "dual", "trial"])
def test_refuses_differing_bases(no_device, kind):
    pkg = no_device
    for f in ("BHat", "SigmaB"):
        Ys, ps, _ = _bags(pkg, kind)
        setattr(ps[2], f, getattr(ps[2], f).copy())
        getattr(ps[2], f)[0, 0] += 1e-3
        _refused(pkg, kind, Ys, ps, "does not share BHat")
    if kind != "basic":                      # CB, delta and their hyper-priors enter the bound: part of the basis here
        for f in ("CB", "delta"):
            Ys, ps, _ = _bags(pkg, kind)
            setattr(ps[1], f, getattr(ps[1], f) * 2.0)
            _refused(pkg, kind, Ys, ps, "CB, delta")


def test_refuses_labels(no_device):
    pkg = no_device
    for kind in ("sparse", "basic"):
        Ys, ps, _ = _bags(pkg, kind)
        ps[0].labels = np.array([1], dtype=np.int64)
        ps[0].H1 = 1
        _refused(pkg, kind, Ys, ps, "label")


@pytest.mark.parametrize("kind", ["sparse", "dual", "trial"])
def test_refuses_non_derived_constants(no_device, kind):
    pkg = no_device
    Ys, ps, _ = _bags(pkg, kind)
    ps[1].eta = ps[1].eta + 3.0
    for name, f in _scorers(pkg, kind):
        with pytest.raises(ValueError, match="eta"):
            f(Ys, ps)


class _FakeBags:
    """An uploaded bag set without a device: what the host checks before its first call."""
    def __init__(self, cls, L, Ms, H):
        self.__class__ = type("Fake" + cls.__name__, (cls,), {"__init__": lambda s: None, "close": lambda s: None})
        self.L, self.Ms, self.H, self.M = L, list(Ms), H, sum(Ms)
        self.col_off = np.concatenate([[0], np.cumsum(Ms)]).astype(np.int64)


def test_refuses_uploaded_bags_of_another_rank_or_family(no_device):
    pkg = no_device
    Ys, ps, _ = _bags(pkg, "sparse", H=4)
    _refused(pkg, "sparse", _FakeBags(pkg.SparseBags, 30, (3, 1, 7), 5), ps, "uploaded for H = 5")
    _refused(pkg, "sparse", _FakeBags(pkg.Bags, 30, (3, 1, 7), 4), ps, "another model family")
    _refused(pkg, "sparse", _FakeBags(pkg.SparseBags, 30, (3, 1), 4), ps, "2 bags but 3 parameter sets")
    Ys, pb, _ = _bags(pkg, "basic", H=4)
    _refused(pkg, "basic", _FakeBags(pkg.Bags, 30, (3, 1, 7), 5), pb, "uploaded for H = 5")


def test_classify_batch_refusals(no_device):
    pkg = no_device
    rng = np.random.default_rng(3)
    Ys = [rng.standard_normal((30, m)) for m in (3, 1, 7)]
    basic, sparse, dual, trial = (_trained(pkg, k, 30, 4, rng) for k in ("basic", "sparse", "dual", "trial"))
    for alg in ("ols", "rls", "min_err", "nonsense"):
        with pytest.raises(ValueError, match="class_alg"):
            pkg.classify_batch(basic, basic, Ys, alg)
    with pytest.raises(ValueError, match="classify_batch"):
        pkg.classify_batch(sparse, sparse, Ys, "vbls")                 # the basic model only
    with pytest.raises(ValueError, match="classify_batch"):
        pkg.classify_batch(basic, sparse, Ys, "dual")
    with pytest.raises(ValueError, match="classify_batch"):
        pkg.classify_batch(trial, trial, Ys, "dual")                   # two parameter sets per bag: classify takes neither
    with pytest.raises(ValueError, match="different H"):
        pkg.classify_batch(dual, _trained(pkg, "dual", 30, 6, rng), Ys, "dual")
    with pytest.raises(ValueError, match="H1"):
        pkg.classify_batch(sparse, None, Ys, "lower_bound")            # H1 = 0: nothing to cut
    with pytest.raises(ValueError, match="H1"):
        pkg.classify_batch(dual, None, Ys, "lower_bound")
    sparse.H1 = 2
    with pytest.raises(ValueError, match="row counts"):
        pkg.classify_batch(sparse, None, Ys[:2] + [np.zeros((31, 2))], "lower_bound")
    with pytest.raises(ValueError, match="no bags"):
        pkg.classify_batch(basic, basic, [], "vbls")


def test_full_cov_split_and_truncated_basis(pkg):
    """factorize_bag: full_cov where M_b (H - H1) < 1600, and the first H - H1 columns of the basis with their slices"""
    assert pkg._full_cov_groups([1, 533, 534, 70, 800], 3) == ([0, 1, 3], [2, 4])          # 533 * 3 = 1599 < 1600 <= 534 * 3
    assert pkg._full_cov_groups([40, 39], 40) == ([1], [0])
    assert pkg._full_cov_groups([5, 6], 2) == ([0, 1], [])
    rng = np.random.default_rng(5)
    res = pkg.vbmf_sparse_init(rng.standard_normal((30, 20)), 5, rng=rng)
    res.SigmaB = rng.standard_normal((5, 5)); res.CB = rng.uniform(1, 2, 5); res.delta = rng.uniform(1, 2, 5)
    res.H1 = 2
    tb = pkg._truncated_basis(res)
    assert tb["H"] == 3 and tb["gamma"] == res.gamma
    assert np.array_equal(tb["BHat"], res.BHat[:, :3]) and np.array_equal(tb["SigmaB"], res.SigmaB[:3, :3])
    assert np.array_equal(tb["CB"], res.CB[:3]) and np.array_equal(tb["delta"], res.delta[:3])


def test_lower_bound_branch_on_a_stubbed_device(pkg, monkeypatch):
    """classify_batch("lower_bound") with the device calls replaced by recorders: which bags go into which call, with which basis,
    updateA! form and threshold, and how the two bounds become labels"""
    rng = np.random.default_rng(6)
    L, H, H1 = 12, 5, 2
    Ms = [3, 600, 2, 533, 534]                                         # (H - H1) M_b < 1600 for bags 0, 2, 3
    Ys = [rng.standard_normal((L, m)) for m in Ms]
    res = pkg.vbmf_sparse_init(rng.standard_normal((L, 20)), H, rng=rng)
    res.H1 = H1
    calls = []

    class StubBags:
        def __init__(self, ys, h, **kw):
            self.Ys, self.H, self.Ms = ys, h, [y.shape[1] for y in ys]
            self.closed = False
            calls.append(("upload", h, self.Ms))

        def close(self):
            self.closed = True

    def stub_vbls(bags, ps, niter, full_cov=False):
        assert all(p.H == bags.H and p.M == m for p, m in zip(ps, bags.Ms))
        calls.append(("vbls", bags.H, bags.Ms, niter, full_cov, ps[0].BHat.shape))

    def stub_lb(bags, ps, clamp=True):
        calls.append(("lb", bags.H, bags.Ms))
        return np.array([float(m) for m in bags.Ms])                   # L0 = M_b

    def stub_lbt(bags, ps, trim=1e-1, clamp=True):
        calls.append(("lbt", bags.H, bags.Ms, trim))
        return np.array([float(m) + (1.0 if m % 2 else -1.0) for m in bags.Ms])   # L1 > L0 for odd M_b

    monkeypatch.setattr(pkg, "SparseBags", StubBags)
    monkeypatch.setattr(pkg, "vbls_sparse_batch_", stub_vbls)
    monkeypatch.setattr(pkg, "lowerBound_batch", stub_lb)
    monkeypatch.setattr(pkg, "lowerBoundTrimmed_batch", stub_lbt)
    labels, e0, e1 = pkg.classify_batch(res, None, Ys, "lower_bound", threshold=0.25)
    full, diag = [3, 2, 533], [600, 534]
    assert calls == [("upload", 3, full), ("upload", 5, full), ("vbls", 3, full, 20, True, (L, 3)), ("lb", 3, full),
                     ("vbls", 5, full, 20, True, (L, 5)),
                     ("upload", 3, diag), ("upload", 5, diag), ("vbls", 3, diag, 20, False, (L, 3)), ("lb", 3, diag),
                     ("vbls", 5, diag, 20, False, (L, 5)),
                     ("lbt", 5, full, 0.25), ("lbt", 5, diag, 0.25)]
    assert np.array_equal(e0, np.array(Ms, dtype=float))
    assert np.array_equal(e1, np.array([4.0, 599.0, 1.0, 534.0, 533.0]))
    assert np.array_equal(labels, np.array([1, 0, 0, 1, 0]))
