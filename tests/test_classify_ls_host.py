"""Least-squares classifiers over many bags (vbmf_bag_least_squares; ols_batch, rls_batch, ls_residual_batch, classify_bags,
test_classification_batch): the parts that need no GPU -- the C ABI is declared, exported and bound by both hosts, the Python host
refuses BEFORE any device call, the "min_err" classifier cuts the basis and splits the bags the way factorize_bag does
(examples/mil_util.jl:393-416, :493-501), and the error-rate summary counts as test_classification does (:558-587)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import __graft_entry__ as G
from tests.test_julia_binding import header_prototypes

ROOT = G.ROOT
ENTRY = "vbmf_bag_least_squares"
NAMES = ("ols_batch", "rls_batch", "ls_residual_batch", "classify_bags", "test_classification_batch")


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


def test_public_names(pkg):
    for name in NAMES:
        assert hasattr(pkg, name) and name in pkg.__all__, name
    assert hasattr(pkg.capi.Context, "bag_least_squares")


def test_header_declares_and_library_exports(pkg):
    protos = header_prototypes()
    assert set(pkg.capi.SYMBOLS) == set(protos)
    lib = ctypes.CDLL(pkg.capi.LIB_PATH)
    assert ENTRY in protos and hasattr(lib, ENTRY) and ENTRY in pkg.capi.SYMBOLS
    assert protos[ENTRY] == ("int", ["vbmf_ctx*", "int64_t", "int64_t*", "double*", "int64_t", "int64_t", "double", "double*", "int64_t",
                                     "double*"])
    assert len(getattr(pkg.capi.lib(), ENTRY).argtypes) == len(protos[ENTRY][1])
    hdr = open(os.path.join(ROOT, "include", "vbmf_hip.h")).read()
    for cite in ("examples/mil_util.jl:159-171", "examples/mil_util.jl:457-468"):
        assert cite in hdr, cite


def test_the_kernel_lives_beside_the_residual_kernel():
    src = open(os.path.join(G.PKG_DIR, "csrc", "score_kernels.hpp")).read()
    for k in ("bag_ls_kernel", "bag_ls_gram_kernel", "bag_ls_inverse_kernel"):
        assert re.search(r"__global__[^;{]*\b" + k + r"\b", src), k
    assert "spd_inverse_lds4" in src                                   # the control chain's inverse, not another one
    assert "atomicAdd" not in src


def test_julia_host_binds_it():
    jl = open(os.path.join(G.PKG_DIR, "julia", "VBMatrixFactorizationHIP.jl")).read()
    assert re.search(r"ccall\(\(:" + ENTRY + r",\s*libvbmf\)", jl)
    for fn in ("ols_batch", "rls_batch", "ls_residual_batch"):
        assert re.search(r"^(function )?" + fn + r"\(", jl, flags=re.M), fn
        assert re.search(r"export[^\n]*(\n\s+[^\n]*)*\b" + fn + r"\b", jl), fn


@pytest.fixture
def no_device(pkg, monkeypatch):
    """Any attempt to reach the library fails the test (the refusals happen on the host)."""
    def boom(*a, **k):
        raise AssertionError("the least-squares host touched the device before refusing")
    monkeypatch.setattr(pkg.capi, "lib", boom)
    monkeypatch.setattr(pkg.capi.Context, "__init__", boom)
    monkeypatch.setattr(pkg.Session, "__init__", boom)
    return pkg


class _Res:
    """classify reads nothing of an "ols" / "rls" model but its BHat"""
    def __init__(self, B):
        self.BHat = B


def _callers(pkg):
    return [("ols_batch", lambda Ys, B, lam=0.0: pkg.ols_batch(Ys, B)),
            ("rls_batch", lambda Ys, B, lam=0.5: pkg.rls_batch(Ys, B, lam)),
            ("ls_residual_batch", lambda Ys, B, lam=0.0: pkg.ls_residual_batch(Ys, B, lam)),
            ("classify_bags", lambda Ys, B, lam=0.0: pkg.classify_bags(_Res(B), _Res(B), Ys, "ols")),
            ("classify_bags", lambda Ys, B, lam=0.0: pkg.classify_bags(_Res(B[..., :2]), _Res(B), Ys, "rls"))]


def test_host_refusals(no_device):
    pkg = no_device
    rng = np.random.default_rng(0)
    L, H = 30, 4
    Ys = [rng.standard_normal((L, m)) for m in (3, 1, 7)]
    B = rng.standard_normal((L, H))
    for name, f in _callers(pkg):
        with pytest.raises(ValueError, match=name + ".*row counts"):
            f(Ys[:2] + [np.zeros((L + 1, 2))], B)
        with pytest.raises(ValueError, match=name + ".*no bags"):
            f([], B)
        with pytest.raises(ValueError, match=name + ".*L x H"):
            f(Ys, rng.standard_normal((L + 1, H)))
        with pytest.raises(ValueError, match=name + ".*L x H"):
            f(Ys, rng.standard_normal(L))
        with pytest.raises(ValueError, match=name + ".*H = 65 > 64"):
            f(Ys, rng.standard_normal((L, 65)))
        with pytest.raises(ValueError, match=name + ".*matrix"):
            f(Ys[:2] + [np.zeros(L)], B)
    for name, f in _callers(pkg)[1:3]:
        for lam in (-1e-3, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=name + ".*lam"):
                f(Ys, B, lam)
    Bn = B.copy(); Bn[3, 1] = np.inf
    with pytest.raises(ValueError, match="ols_batch.*finite"):
        pkg.ols_batch(Ys, Bn)


def test_classify_bags_refusals(no_device):
    pkg = no_device
    rng = np.random.default_rng(1)
    Ys = [rng.standard_normal((30, m)) for m in (3, 1, 7)]
    Ytr = rng.standard_normal((30, 20))
    basic, sparse, dual = pkg.vbmf_init(Ytr, 4, rng=rng), pkg.vbmf_sparse_init(Ytr, 4, rng=rng), pkg.vbmf_dual_init(Ytr, 4, 2, rng=rng)
    with pytest.raises(ValueError, match="classify_bags.*class_alg"):
        pkg.classify_bags(basic, basic, Ys, "nonsense")
    with pytest.raises(ValueError, match="classify_bags.*BHat"):
        pkg.classify_bags(basic, None, Ys)                             # the default, "ols", reads both models
    for res0 in (sparse, dual, basic):                                 # H1 = 0: nothing to cut; factorize_bag is the sparse model's
        with pytest.raises(ValueError, match="classify_bags.*H1"):
            pkg.classify_bags(res0, None, Ys, "min_err")
    sparse.H1 = 2
    with pytest.raises(ValueError, match="classify_bags.*row counts"):
        pkg.classify_bags(sparse, None, Ys[:2] + [np.zeros((31, 2))], "min_err")
    with pytest.raises(ValueError, match="classify_bags.*no bags"):
        pkg.classify_bags(sparse, None, [], "min_err")
    # the other three are classify_batch's, refusals included
    with pytest.raises(ValueError, match="classify_batch"):
        pkg.classify_bags(sparse, sparse, Ys, "vbls")


def test_the_ls_classifiers_make_one_upload_and_two_calls(pkg, monkeypatch):
    """"ols" / "rls" on a stubbed device: one upload for two models of different rank, one call per model with that model's own
    BHat and lambda, and label 1 exactly where err0 > err1"""
    rng = np.random.default_rng(2)
    L, Ms = 12, [3, 1, 4, 2]
    Ys = [rng.standard_normal((L, m)) for m in Ms]
    res0, res1 = _Res(rng.standard_normal((L, 3))), _Res(rng.standard_normal((L, 6)))
    calls = []
    r2 = {3: np.array([4.0, 1.0, 9.0, 16.0]), 6: np.array([1.0, 4.0, 9.0, 25.0])}

    class StubCtx:
        def bag_least_squares(self, col_off, B, lam, want_X=True, want_r2=True):
            calls.append(("ls", list(col_off), B.shape, lam, want_X, want_r2))
            assert np.array_equal(B, res0.BHat if B.shape[1] == 3 else res1.BHat)
            return None, r2[B.shape[1]].copy()

    class StubBags(pkg.Bags):
        def __init__(self, ys, h):
            self.Ms, self.H, self.L = [y.shape[1] for y in ys], h, ys[0].shape[0]
            self.col_off = np.concatenate([[0], np.cumsum(self.Ms)]).astype(np.int64)
            self.session = type("S", (), {"ctx": StubCtx()})()
            calls.append(("upload", h, self.Ms))

        def close(self):
            calls.append(("close",))

    monkeypatch.setattr(pkg, "Bags", StubBags)
    for alg, lam in (("ols", 0.0), ("rls", 1e-2)):
        del calls[:]
        labels, e0, e1 = pkg.classify_bags(res0, res1, Ys, alg)
        off = [0, 3, 4, 8, 10]
        assert calls == [("upload", 3, Ms), ("ls", off, (L, 3), lam, False, True), ("ls", off, (L, 6), lam, False, True), ("close",)]
        assert np.array_equal(e0, [2.0, 1.0, 3.0, 4.0]) and np.array_equal(e1, [1.0, 2.0, 3.0, 5.0])
        assert np.array_equal(labels, [1, 0, 0, 0])                    # a tie is label 0 (:487-491)
    # an upload the caller made is used as it is and left open
    del calls[:]
    bags = StubBags(Ys, 9)
    pkg.classify_bags(res0, res1, bags, "ols")
    assert [c[0] for c in calls] == ["upload", "ls", "ls"]


def test_min_err_branch_on_a_stubbed_device(pkg, monkeypatch):
    """classify_bags("min_err") with the device calls replaced by recorders: which bags go into which upload / fit / residual
    call, with which basis and updateA! form, and how the two residuals become labels on both sides of the threshold"""
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
            calls.append(("close", self.H, self.Ms))

    def stub_vbls(bags, ps, niter, full_cov=False):
        assert all(p.H == bags.H and p.M == m for p, m in zip(ps, bags.Ms))
        calls.append(("vbls", bags.H, bags.Ms, niter, full_cov, ps[0].BHat.shape))

    # err0 = 10 for every bag; err1 by M_b: 9.5 (ratio 0.05), 8 (0.2), 10.4 (0.04), 12.6 (0.26), 9 (0.1)
    err1 = {3: 9.5, 600: 8.0, 2: 10.4, 533: 12.6, 534: 9.0}

    def stub_resid(bags, ps):
        assert not bags.closed
        calls.append(("resid", bags.H, bags.Ms))
        return np.array([10.0 if bags.H == H - H1 else err1[m] for m in bags.Ms])

    def no_bound(*a, **k):
        raise AssertionError("min_err reads no lower bound")

    monkeypatch.setattr(pkg, "SparseBags", StubBags)
    monkeypatch.setattr(pkg, "vbls_sparse_batch_", stub_vbls)
    monkeypatch.setattr(pkg, "residual_batch", stub_resid)
    monkeypatch.setattr(pkg, "lowerBound_batch", no_bound)
    monkeypatch.setattr(pkg, "lowerBoundTrimmed_batch", no_bound)
    labels, e0, e1 = pkg.classify_bags(res, None, Ys, "min_err", threshold=0.15)
    full, diag = [3, 2, 533], [600, 534]
    assert calls == [("upload", 3, full), ("upload", 5, full), ("vbls", 3, full, 20, True, (L, 3)), ("resid", 3, full),
                     ("vbls", 5, full, 20, True, (L, 5)), ("close", 3, full),
                     ("upload", 3, diag), ("upload", 5, diag), ("vbls", 3, diag, 20, False, (L, 3)), ("resid", 3, diag),
                     ("vbls", 5, diag, 20, False, (L, 5)), ("close", 3, diag),
                     ("resid", 5, full), ("resid", 5, diag), ("close", 5, full), ("close", 5, diag)]
    assert np.array_equal(e0, np.full(5, 10.0))
    assert np.array_equal(e1, np.array([err1[m] for m in Ms]))
    assert np.array_equal(labels, np.array([0, 1, 0, 1, 0]))           # |(e0 - e1)/e0| < 0.15 is label 0, either sign of e0 - e1
    # the reference's threshold is the default, and niter reaches both fits
    del calls[:]
    labels, _, _ = pkg.classify_bags(res, None, Ys, "min_err", niter=7)
    assert np.array_equal(labels, np.array([0, 1, 0, 1, 1]))           # 0.1 < 0.1 is false (:497)
    assert [c[3] for c in calls if c[0] == "vbls"] == [7, 7, 7, 7]


def test_classification_summary(pkg, monkeypatch):
    """test_classification (examples/mil_util.jl:558-587): label - est_label == 1 is a false negative, -1 a false positive"""
    est = np.array([0, 1, 1, 0, 0, 1, 1, 1], dtype=np.int64)
    seen = []

    def stub(res0, res1, Ys, class_alg="ols", threshold=1e-1, niter=None):
        seen.append((res0, res1, class_alg, threshold))
        return est[:len(Ys)].copy(), np.zeros(len(Ys)), np.zeros(len(Ys))

    monkeypatch.setattr(pkg, "classify_bags", stub)
    Ys = [np.zeros((3, 1))] * 8
    labels = np.array([0, 1, 0, 1, 0, 0, 1, 1])                        # fp at 2 and 5, fn at 3
    out = pkg.test_classification_batch("r0", "r1", Ys, labels)
    assert out == (3 / 8, (2 / 4 + 1 / 4) / 2, 2, 1, 4, 4)
    assert all(type(v) is t for v, t in zip(out, (float, float, int, int, int, int)))
    assert seen == [("r0", "r1", "ols", 1e-1)]                         # the reference's defaults
    pkg.test_classification_batch("r0", "r1", Ys, labels, class_alg="min_err", threshold=0.3)
    assert seen[-1] == ("r0", "r1", "min_err", 0.3)
    # no positive bag: fn / n1 = 0 / 0 is NaN, as Julia's float division gives; nothing is raised
    mer, eer, fp, fn, n0, n1 = pkg.test_classification_batch("r0", "r1", Ys, np.zeros(8, dtype=np.int64))
    assert (mer, fp, fn, n0, n1) == (5 / 8, 5, 0, 8, 0) and math.isnan(eer)
    # no negative bag, with a false positive impossible and false negatives present: 0 / 0 again; a count over zero is inf
    mer, eer, fp, fn, n0, n1 = pkg.test_classification_batch("r0", "r1", Ys, np.ones(8, dtype=np.int64))
    assert (mer, fp, fn, n0, n1) == (3 / 8, 0, 3, 0, 8) and math.isnan(eer)
    monkeypatch.setattr(pkg, "classify_bags", lambda *a, **k: (np.ones(2, dtype=np.int64), None, None))
    mer, eer, fp, fn, n0, n1 = pkg.test_classification_batch("r0", "r1", Ys[:2], np.zeros(2, dtype=np.int64))
    assert (mer, fp, fn, n0, n1) == (1.0, 2, 0, 2, 0) and eer != eer  # 2/2 + 0/0
    with pytest.raises(ValueError, match="test_classification_batch"):
        pkg.test_classification_batch("r0", "r1", Ys, labels[:3])
