"""Every fold's test bags against its own models in one call (vbmf_bag_least_squares_jobs; classify_folds, test_classification_folds,
validate_folds): the parts that need no GPU -- the C ABI is declared, exported and bound by both hosts, the Python host refuses
BEFORE any device call, the error-rate summary counts as test_classification_batch does (examples/mil_util.jl:558-587, :612-614),
classify_folds turns folds into ONE call's bases and jobs, and validate_folds hands train_folds the label-0 and label-1 subsets of
every split's training ids (get_matrices, :46)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import __graft_entry__ as G
from tests.test_julia_binding import header_prototypes

ROOT = G.ROOT
ENTRY = "vbmf_bag_least_squares_jobs"
NAMES = ("classify_folds", "test_classification_folds", "validate_folds")


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


# ---- ABI and bindings ---------------------------------------------------------------------------------------------------------
def test_abi_and_bindings(pkg):
    protos = header_prototypes()
    assert set(pkg.capi.SYMBOLS) == set(protos)
    lib = ctypes.CDLL(pkg.capi.LIB_PATH)
    assert ENTRY in protos and hasattr(lib, ENTRY) and ENTRY in pkg.capi.SYMBOLS
    assert protos[ENTRY] == ("int", ["vbmf_ctx*", "int64_t", "int64_t*", "int64_t", "int64_t*", "double*", "double*", "int64_t", "int64_t*",
                                     "int64_t*", "double*", "double*", "int64_t*"])
    assert len(getattr(pkg.capi.lib(), ENTRY).argtypes) == len(protos[ENTRY][1])
    hdr = open(os.path.join(ROOT, "include", "vbmf_hip.h")).read()
    for cite in ("examples/mil_util.jl:627-648", "examples/mil_util.jl:558-587"):
        assert cite in hdr, cite
    jl = open(os.path.join(G.PKG_DIR, "julia", "VBMatrixFactorizationHIP.jl")).read()
    assert re.search(r"ccall\(\(:" + ENTRY + r",\s*libvbmf\)", jl)
    assert re.search(r"^function bag_least_squares_jobs\(", jl, flags=re.M)
    assert re.search(r"export[^\n]*(\n\s+[^\n]*)*\bbag_least_squares_jobs\b", jl)
    for name in NAMES:
        assert hasattr(pkg, name) and name in pkg.__all__, name
    assert hasattr(pkg.capi.Context, "bag_least_squares_jobs")


def test_the_job_kernels_share_the_device_functions_of_the_old_ones():
    src = open(os.path.join(G.PKG_DIR, "csrc", "score_kernels.hpp")).read()
    bodies = {}
    for m in re.finditer(r"__global__[^;{]*?\b(\w+_kernel)\s*\([^{]*\{", src):
        end = src.find("\n}\n", m.end())
        bodies[m.group(1)] = src[m.end():end]
    for f, old, new in (("ls_gram_chunk", "bag_ls_gram_kernel", "bag_ls_gram_jobs_kernel"),
                        ("ls_inverse", "bag_ls_inverse_kernel", "bag_ls_inverse_jobs_kernel"), ("ls_slice", "bag_ls_kernel", "bag_ls_jobs_kernel")):
        assert re.search(r"__device__[^;{]*\b" + f + r"\b", src), f
        for k in (old, new):
            assert re.search(r"\b" + f + r"\b", bodies[k]), (f, k)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(pkg, monkeypatch):
    """Any attempt to reach the library fails the test (the refusals happen on the host)."""
    def boom(*a, **k):
        raise AssertionError("the fold host touched the device before refusing")
    monkeypatch.setattr(pkg.capi, "lib", boom)
    monkeypatch.setattr(pkg.capi.Context, "__init__", boom)
    monkeypatch.setattr(pkg.Session, "__init__", boom)
    return pkg


class _Res:
    def __init__(self, B):
        self.BHat = B


def _fake_pool(pkg, L, Ms, closed=False):
    """a BagPool's host side without its context"""
    pool = pkg.BagPool.__new__(pkg.BagPool)
    pool.Ms = list(Ms)
    pool.col_off = np.concatenate([[0], np.cumsum(Ms)]).astype(np.int64)
    pool.L, pool.M, pool.ctx_kw, pool._closed = L, int(sum(Ms)), {}, closed
    return pool


def test_host_refusals(no_device):
    pkg = no_device
    rng = np.random.default_rng(0)
    L, H = 30, 4
    Ys = [rng.standard_normal((L, m)) for m in (3, 1, 7, 2)]
    good = (_Res(rng.standard_normal((L, H))), _Res(rng.standard_normal((L, 2))))
    labels = [0, 1, 0, 1]
    pool, closed = _fake_pool(pkg, L, [3, 1, 7, 2]), _fake_pool(pkg, L, [3, 1, 7, 2], closed=True)
    Bn = rng.standard_normal((L, H)); Bn[3, 1] = np.inf

    def callers(fn):
        if fn == "classify_folds":
            return lambda models, tests, ys=Ys, alg="ols", lab=labels: pkg.classify_folds(models, tests, ys, alg)
        return lambda models, tests, ys=Ys, alg="ols", lab=labels: pkg.test_classification_folds(models, tests, ys, lab, alg)

    for fn in ("classify_folds", "test_classification_folds"):
        f = callers(fn)
        for ys in (Ys, pool):
            with pytest.raises(ValueError, match=fn + ".*outside 0"):
                f([good], [[0, 4]], ys)
            with pytest.raises(ValueError, match=fn + ".*outside 0"):
                f([good, (0, 0)], [[0], [-1]], ys)
            with pytest.raises(ValueError, match=fn + ".*2 models but 1 test"):
                f([good, good], [[0]], ys)
        with pytest.raises(ValueError, match=fn + ".*closed"):
            f([good], [[0]], closed)
        for t in ([2.7], [1.0], [True], np.array([0.0, 1.0]), ["1"]):
            with pytest.raises(ValueError, match=fn + ".*fold 0.*not an integer"):
                f([good], [t])
        with pytest.raises(ValueError, match=fn + ".*class_alg.*classify_bags"):
            f([good], [[0]], alg="vbls")
        with pytest.raises(ValueError, match=fn + ".*class_alg.*classify_bags"):
            f([good], [[0]], alg="nonsense")
        with pytest.raises(ValueError, match="classify_folds.*fold 1.*res1.*no BHat"):
            f([good, (good[0], object())], [[0], [1]])
        with pytest.raises(ValueError, match="classify_folds.*fold 0.*res0.*L = 30"):
            f([(_Res(rng.standard_normal((L + 1, H))), good[1])], [[0]])
        with pytest.raises(ValueError, match="classify_folds.*fold 0.*res1.*H = 65 > 64"):
            f([(good[0], _Res(rng.standard_normal((L, 65))))], [[0]])
        with pytest.raises(ValueError, match="classify_folds.*fold 2.*res0.*finite"):
            f([good, (0, 0), (_Res(Bn), good[1])], [[0], [1], [2]])
        with pytest.raises(ValueError, match=fn + ".*row counts"):
            f([good], [[0]], Ys[:2] + [np.zeros((L + 1, 2))])
    for lab, why in ((labels[:3], "4 bags but 3 labels"), ([0, 1, 2, 0], "0 or 1")):
        with pytest.raises(ValueError, match="test_classification_folds.*" + why):
            pkg.test_classification_folds([good], [[0]], Ys, lab)
        with pytest.raises(ValueError, match="validate_folds.*" + why):
            pkg.validate_folds(pool, lab, [([0, 1], [2, 3])], "basic", H, 5)
    with pytest.raises(ValueError, match="validate_folds.*closed"):
        pkg.validate_folds(closed, labels, [([0, 1], [2, 3])], "basic", H, 5)
    with pytest.raises(ValueError, match="validate_folds.*BagPool"):
        pkg.validate_folds(Ys, labels, [([0, 1], [2, 3])], "basic", H, 5)
    with pytest.raises(ValueError, match="validate_folds.*outside 0"):
        pkg.validate_folds(pool, labels, [([0, 1], [2, 3]), ([0, 9], [1])], "basic", H, 5)
    with pytest.raises(ValueError, match="validate_folds.*outside 0"):
        pkg.validate_folds(pool, labels, [([0, 1], [2, 4])], "basic", H, 5)
    with pytest.raises(ValueError, match="validate_folds.*not an integer"):
        pkg.validate_folds(pool, labels, [([0, 1.5], [2, 3])], "basic", H, 5)
    with pytest.raises(ValueError, match="validate_folds.*H = 65 > 64"):
        pkg.validate_folds(pool, labels, [([0, 1], [2, 3])], "basic", 65, 5)
    with pytest.raises(ValueError, match="validate_folds.*class_alg.*classify_bags"):
        pkg.validate_folds(pool, labels, [([0, 1], [2, 3])], "basic", H, 5, class_alg="min_err")


# ---- counting -----------------------------------------------------------------------------------------------------------------
def test_counting_is_test_classification_batch_s(pkg, monkeypatch):
    """label - est_label == 1 is a false negative, -1 a false positive (examples/mil_util.jl:574-586); a (0, 0) fold is -1 six times"""
    labels = np.array([0, 1, 0, 1, 0, 0, 1, 1, 0, 0, 0, 1])
    tests = [[0, 1, 2, 3, 4, 5, 6, 7], [8, 9, 10], [11, 3], [4, 5], []]
    est = [np.array([0, 1, 1, 0, 0, 1, 1, 1]), np.array([1, 0, 1]), None, np.array([1, 0]), np.empty(0, dtype=np.int64)]
    Ys = [np.zeros((3, 1))] * 12
    models = ["m0", "m1", (0, 0), "m3", "m4"]
    seen = []

    def stub(ms, ts, ys, class_alg="ols"):
        seen.append((list(ms), [list(t) for t in ts], ys, class_alg))
        return [None if e is None else (e.copy(), np.zeros(e.size), np.zeros(e.size)) for e in est]

    monkeypatch.setattr(pkg, "classify_folds", stub)
    out = pkg.test_classification_folds(models, tests, Ys, labels, "rls")
    assert seen == [(models, tests, Ys, "rls")]
    assert out[0] == (3 / 8, (2 / 4 + 1 / 4) / 2, 2, 1, 4, 4)          # fp at 2 and 5, fn at 3
    assert all(type(v) is t for v, t in zip(out[0], (float, float, int, int, int, int)))
    mer, eer, fp, fn, n0, n1 = out[1]                                 # no positive bag: fn / n1 = 0 / 0 is NaN as in Julia
    assert (mer, fp, fn, n0, n1) == (2 / 3, 2, 0, 3, 0) and math.isnan(eer)
    assert out[2] == (-1.0,) * 6
    mer, eer, fp, fn, n0, n1 = out[3]                                 # n0 == 2, n1 == 0 again, one false positive
    assert (mer, fp, fn, n0, n1) == (1 / 2, 1, 0, 2, 0) and math.isnan(eer)
    assert math.isnan(out[4][0]) and out[4][2:] == (0, 0, 0, 0)       # nothing tested: 0 / 0
    # n0 == 0 with a false negative: 0 / 0 + 1 / 2 is NaN; n0 == 0 is where a count over zero would be inf
    est[:] = [np.array([0, 1]), np.array([1]), None, np.array([1, 1]), np.empty(0, dtype=np.int64)]
    out = pkg.test_classification_folds(models, [[1, 3], [4], [0], [6, 7], []], Ys, labels)
    mer, eer, fp, fn, n0, n1 = out[0]
    assert (mer, fp, fn, n0, n1) == (1 / 2, 0, 1, 0, 2) and math.isnan(eer)
    mer, eer, fp, fn, n0, n1 = out[1]                                 # one negative bag called positive: 1 / 1 + 0 / 0
    assert (mer, fp, fn, n0, n1) == (1.0, 1, 0, 1, 0) and math.isnan(eer)
    # the same hand-made labels through test_classification_batch
    for f, t in ((0, [1, 3]), (3, [6, 7])):
        monkeypatch.setattr(pkg, "classify_bags", lambda *a, _e=est[f], **k: (_e.copy(), None, None))
        want = pkg.test_classification_batch("r0", "r1", [Ys[b] for b in t], labels[t])
        assert all(a == b or (a != a and b != b) for a, b in zip(out[f], want)), (out[f], want)


# ---- job construction ---------------------------------------------------------------------------------------------------------
class _RecCtx:
    def __init__(self, calls, status=None):
        self.calls, self.status = calls, status

    def bag_least_squares_jobs(self, col_off, bases, lams, job_bag, job_basis, want_X=False, want_r2=True):
        self.calls.append(dict(col_off=list(col_off), bases=list(bases), lams=list(lams), job_bag=list(job_bag),
                               job_basis=list(job_basis), want_X=want_X, want_r2=want_r2))
        r2 = np.array([(100.0 * k + b) ** 2 for b, k in zip(job_bag, job_basis)])
        return None, r2, np.zeros(len(bases), dtype=np.int64) if self.status is None else np.array(self.status)


def test_classify_folds_issues_one_call_with_the_folds_jobs(pkg):
    rng = np.random.default_rng(3)
    L, Ms = 12, [3, 1, 4, 2, 5, 1]
    pool = _fake_pool(pkg, L, Ms)
    calls = []
    pool.session = type("S", (), {"ctx": _RecCtx(calls)})()
    B = [rng.standard_normal((L, h)) for h in (3, 6, 2, 2, 5, 1)]
    trained_all = [(_Res(B[0]), _Res(B[1])), (_Res(B[2]), _Res(B[3])), (_Res(B[4]), _Res(B[5]))]
    tests = [[4, 0, 4], [5], [1, 2]]
    for alg, lam in (("ols", 0.0), ("rls", 1e-2)):
        del calls[:]
        out = pkg.classify_folds(trained_all, tests, pool, alg)
        assert len(calls) == 1
        c = calls[0]
        assert c["col_off"] == [0, 3, 4, 8, 10, 15, 16] and c["lams"] == [lam] * 6 and (c["want_X"], c["want_r2"]) == (False, True)
        assert all(np.array_equal(a, b) for a, b in zip(c["bases"], B)) and len(c["bases"]) == 6
        assert c["job_bag"] == [4, 0, 4, 4, 0, 4, 5, 5, 1, 2, 1, 2]     # the pool ids as given, once per model of the fold
        assert c["job_basis"] == [0, 0, 0, 1, 1, 1, 2, 3, 4, 4, 5, 5]   # 2 f and 2 f + 1
        for f, (labels, e0, e1) in enumerate(out):
            assert np.array_equal(e0, [200.0 * f + b for b in tests[f]]) and np.array_equal(e1, [100.0 * (2 * f + 1) + b for b in tests[f]])
            assert np.array_equal(labels, np.zeros(len(tests[f]), dtype=np.int64)) and labels.dtype == np.int64
    # an untrained fold and an empty test list contribute no jobs; the bases of the trained folds keep their order
    del calls[:]
    out = pkg.classify_folds([trained_all[0], (0, 0), trained_all[1], trained_all[2]], [[], [3], np.array([2, 0]), [1]], pool)
    assert len(calls) == 1 and len(calls[0]["bases"]) == 6
    assert calls[0]["job_bag"] == [2, 0, 2, 0, 1, 1] and calls[0]["job_basis"] == [2, 2, 3, 3, 4, 5]
    assert out[1] is None and all(a.size == 0 for a in out[0]) and out[0][0].dtype == np.int64
    assert np.array_equal(out[2][1], [202.0, 200.0]) and np.array_equal(out[3][2], [501.0])
    # nothing to classify: no call at all
    del calls[:]
    assert pkg.classify_folds([(0, 0), (0, 0)], [[1], [2]], pool) == [None, None]
    out = pkg.classify_folds([trained_all[0]], [[]], pool)
    assert calls == [] and all(a.size == 0 for a in out[0])
    # a fold with a bad basis raises after the others were computed
    pool.session = type("S", (), {"ctx": _RecCtx(calls, status=[0, 0, 0, 1, 0, 0])})()
    with pytest.raises(pkg.VbmfError, match="classify_folds: fold 1.*res1.*rls") as e:
        pkg.classify_folds(trained_all, tests, pool)
    assert e.value.code == pkg.capi.VBMF_ERR_NUMERIC and e.value.results[1] is None
    assert np.array_equal(e.value.results[2][1], [401.0, 402.0])


# ---- validate_folds -----------------------------------------------------------------------------------------------------------
def test_validate_folds_hands_train_folds_the_label_groups(pkg, monkeypatch):
    pool = _fake_pool(pkg, 12, [3, 1, 4, 2, 5, 1, 2, 2])
    labels = [0, 1, 1, 0, 0, 1, 0, 1]
    splits = [([5, 0, 1, 3, 2], [4, 6, 7]), ([7, 6, 4], [0, 1]), ([0, 3], [1])]
    seen = {}
    rng = np.random.default_rng(1)

    def train(folds, solver, H, niter, **kw):
        seen["train"] = (folds, solver, H, niter, kw)
        return ["m0", "m1", (0, 0)]

    def summarise(models, tests, Ys, lab, class_alg="ols"):
        seen["test"] = (models, tests, Ys, list(lab), class_alg)
        return ["t0", "t1", "t2"]

    monkeypatch.setattr(pkg, "train_folds", train)
    monkeypatch.setattr(pkg, "test_classification_folds", summarise)
    out = pkg.validate_folds(pool, labels, splits, "sparse", 5, 20, eps=1e-4, class_alg="rls", rng=rng, form="split", slice_cols=16)
    assert out == ["t0", "t1", "t2"]
    folds, solver, H, niter, kw = seen["train"]
    assert folds == [([0, 3], [5, 1, 2]), ([6, 4], [7]), ([0, 3], [])]   # label 0, label 1, each in the order given
    assert (solver, H, niter) == ("sparse", 5, 20)
    assert kw == dict(eps=1e-4, rng=rng, form="split", slice_cols=16, pool=pool)
    assert seen["test"] == (["m0", "m1", (0, 0)], [[4, 6, 7], [0, 1], [1]], pool, labels, "rls")
