"""factorize_bag and its scores for every fold's test bags in one device call (vbmf_sparse_scored_jobs; factorize_folds, classify_folds
with class_alg = "lower_bound" / "min_err", validate_local_folds): the parts that need no GPU -- the prototype and bindings, the host's
refusals before any device call, the models and job tables it builds, and the fp64 reference of the four scores (ref_factorize: the
block-wise ref_vbls of tests/test_vbls_jobs_host.py with the oracle's lowerBound / lowerBoundTrimmed on its state) that
tests/test_gpu_scored_jobs.py uses where the oracle's dense M_b H x M_b H inverse is too large, pinned here to the oracle's own loop."""
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as G
from oracle import vbmf_oracle as O
from tests.test_classify_folds_host import _fake_pool
from tests.test_gpu_vbls_sparse_batch import _convert
from tests.test_julia_binding import header_prototypes
from tests.test_vbls_jobs_host import ref_vbls, trained

ENTRY = "vbmf_sparse_scored_jobs"
NAMES = ("factorize_folds", "validate_local_folds")
DENSE_MAX = 300          # the oracle's dense full_cov inverse up to this M_b H


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


# ---- the reference --------------------------------------------------------------------------------------------------------------
def full_form(M, H, H1):
    """factorize_bag's choice of the updateA! form (examples/mil_util.jl:405-409)"""
    return M * (H - H1) < 1600


def oracle_pair(Y, po):
    """factorize_bag's two fresh sets for bag Y from the oracle set po with 0 < H1 < H (examples/mil_util.jl:398-404, :410)"""
    H0 = po.H - po.H1
    q0 = O.vbmf_sparse_init(Y, H0, rng=np.random.default_rng(1), full_cov=False, materialize_yhat=False)
    q0.BHat, q0.SigmaB, q0.CB = po.BHat[:, :H0].copy(), po.SigmaB[:H0, :H0].copy(), po.CB[:H0].copy()
    q0.gamma, q0.delta = po.gamma, po.delta[:H0].copy()
    q1 = O.copy_vbmf_params(Y, po, rng=np.random.default_rng(2))
    return q0, q1


def scored_arrays(q):
    """one model of Context.sparse_scored_jobs from an oracle (or package) sparse set"""
    H, one = int(q.H), np.ones(int(q.H))
    return dict(BHat=np.array(q.BHat, dtype=np.float64), SigmaB=np.array(q.SigmaB, dtype=np.float64), CB=np.array(q.CB, dtype=np.float64),
                delta=np.array(q.delta, dtype=np.float64), gamma=float(q.gamma), gamma0=float(q.gamma0), delta0=float(q.delta0),
                a_pri=one * q.alpha0, b_pri=one * q.beta0, a_post=one * (q.alpha0 + 0.5), eta0=float(q.eta0), zeta0=float(q.zeta0), sigma0=1.0,
                ca0=1.0, alpha=one * (q.alpha0 + 0.5), beta0=one * float(q.beta0))


def fill(q, r):
    """the state ref_vbls (or a device job) left, on the oracle set q"""
    q.ATVecHat = np.array(r["ATVecHat"], dtype=np.float64).reshape(-1)
    q.AHat = q.ATVecHat.reshape(q.M, q.H).copy()
    q.diagSigmaATVec, q.CA, q.beta = (np.array(r[f], dtype=np.float64).reshape(-1) for f in ("diagSigmaATVec", "CA", "beta"))
    q.SigmaA = np.array(r["SigmaA"], dtype=np.float64).reshape(q.H, q.H)
    q.sigmaHat, q.zeta = float(r["sigmaHat"]), float(r["zeta"])
    return q


def ref_factorize(Y, po, niter, threshold):
    """factorize_bag's four scores of bag Y (L0 = lowerBound of the truncated basis' fit, L1 = lowerBoundTrimmed(threshold) of the
    whole basis' fit, the two residual norms) and the two filled oracle sets, with the block-wise ref_vbls as the iteration"""
    full = full_form(Y.shape[1], po.H, po.H1)
    q0, q1 = oracle_pair(Y, po)
    r0, r1 = (ref_vbls(Y, scored_arrays(q), niter, full) for q in (q0, q1))
    fill(q0, r0), fill(q1, r1)
    return dict(L0=O.lowerBound(Y, q0), L1=O.lowerBoundTrimmed(Y, q1, threshold), err0=np.sqrt(r0["r2"]), err1=np.sqrt(r1["r2"]),
                sets=(q0, q1), fits=(r0, r1))


def oracle_factorize(Y, po, niter, threshold):
    """the same by the oracle's own updateA! / updateCA! / updateSigma! loop (its dense inverse under full_cov)"""
    full = full_form(Y.shape[1], po.H, po.H1)
    q0, q1 = oracle_pair(Y, po)
    for q in (q0, q1):
        for _ in range(niter):
            O.sparse_updateA(Y, q, full_cov=full)
            O.sparse_updateCA(q)
            O.sparse_updateSigma(Y, q)
    err = [float(np.linalg.norm(Y - q.BHat @ q.AHat.T)) for q in (q0, q1)]
    return dict(L0=O.lowerBound(Y, q0), L1=O.lowerBoundTrimmed(Y, q1, threshold), err0=err[0], err1=err[1], sets=(q0, q1))


@pytest.mark.parametrize("L,H,H1", [(33, 5, 1), (33, 5, 2), (33, 17, 1)])
def test_block_wise_reference_is_the_oracle_s(L, H, H1):
    po, draw = trained("sparse", L, H, 4000 + 10 * H + L)
    po.H1 = H1
    worst = {}
    for w in [1, 2, 3, 8, 9, 17]:
        if w * H > DENSE_MAX:
            continue
        Y = draw(w)
        for thr in (1e-1, 0.5, 0.0):
            a, b = ref_factorize(Y, po, 20, thr), oracle_factorize(Y, po, 20, thr)
            for k in ("L0", "L1", "err0", "err1"):
                worst[k] = max(worst.get(k, 0.0), abs(a[k] - b[k]) / abs(b[k]))
            assert np.array_equal(np.abs(a["sets"][1].ATVecHat) > thr, np.abs(b["sets"][1].ATVecHat) > thr)
    assert worst and all(v <= 1e-10 for v in worst.values()), worst


# ---- 0. ABI and bindings --------------------------------------------------------------------------------------------------------
def test_abi_and_bindings(pkg):
    protos = header_prototypes()
    lib = ctypes.CDLL(pkg.capi.LIB_PATH)
    assert ENTRY in protos and hasattr(lib, ENTRY) and ENTRY in pkg.capi.SYMBOLS
    d, i = "double*", "int64_t*"
    assert protos[ENTRY] == ("int", ["vbmf_ctx*", "int64_t", i, "int64_t", "int", "int", "int64_t", i] + [d] * 14 + ["int64_t", i, i, i]
                             + [d] * 10 + [i])
    assert len(getattr(pkg.capi.lib(), ENTRY).argtypes) == len(protos[ENTRY][1])
    # the old entry keeps its prototype
    assert protos["vbmf_sparse_fixed_basis_jobs"] == ("int", ["vbmf_ctx*", "int64_t", i, "int64_t", "int64_t", "int", "int64_t", d, d, d, d, d,
                                                              d, d, d, "int64_t", i, i, d, d, d, d, d, d, d, d, i])
    hdr = open(os.path.join(G.ROOT, "include", "vbmf_hip.h")).read()
    for cite in ("examples/mil_util.jl:393-416", "examples/mil_util.jl:627-648", "src/vbmf_sparse.jl:481"):
        assert cite in hdr, cite
    jl = open(os.path.join(G.PKG_DIR, "julia", "VBMatrixFactorizationHIP.jl")).read()
    assert re.search(r"ccall\(\(:" + ENTRY + r",\s*libvbmf\)", jl)
    assert re.search(r"^function sparse_scored_jobs\(", jl, flags=re.M)
    assert re.search(r"export[^\n]*(\n\s+[^\n]*)*\bsparse_scored_jobs\b", jl)
    for name in NAMES:
        assert hasattr(pkg, name) and name in pkg.__all__, name
    assert hasattr(pkg.capi.Context, "sparse_scored_jobs")


def test_both_kernels_share_the_sums_and_both_entries_the_host():
    src = open(os.path.join(G.PKG_DIR, "csrc", "score_kernels.hpp")).read() + open(os.path.join(G.PKG_DIR, "csrc", "vbls_jobs_kernels.hpp")).read()
    assert re.search(r"__device__[^;{]*\blb_column_sums\b", src)
    for kernel in ("bag_lb_sums_kernel", "vbls_jobs_kernel"):
        m = re.search(r"__global__[^;{]*?\b" + kernel + r"\s*\([^{]*\{", src)
        body = src[m.end():src.find("\n}\n", m.end())]
        assert re.search(r"\blb_column_sums<(true|false)>\(", body), kernel
    host = open(os.path.join(G.PKG_DIR, "csrc", "host_bags.hpp")).read()
    for entry in ("vbmf_sparse_fixed_basis_jobs", "vbmf_sparse_scored_jobs"):
        m = re.search(r"\nint " + entry + r"\([^{]*\{", host)
        assert "return vjobs_call(c, a);" in host[m.end():host.find("\n}\n", m.end())], entry


# ---- 1. the models and job tables ---------------------------------------------------------------------------------------------------
class _RecCtx:
    def __init__(self, calls, status_of=None):
        self.calls, self.status_of = calls, status_of

    def sparse_scored_jobs(self, col_off, models, job_bag, job_model, job_full_cov, job_trim, niter, clamp=True, grouped=False):
        self.calls.append(dict(col_off=list(col_off), models=list(models), job_bag=list(job_bag), job_model=list(job_model),
                               job_full_cov=[bool(f) for f in job_full_cov], job_trim=list(job_trim), niter=niter, clamp=clamp, grouped=grouped))
        nj = len(job_bag)
        st = np.zeros(nj, dtype=np.int64)
        if self.status_of is not None:
            st[self.status_of] = 1
        jb, jk = np.asarray(job_bag, dtype=np.float64), np.asarray(job_model, dtype=np.float64)
        return dict(lb=-(1000.0 * jk + jb + 1), r2=(100.0 * jk + jb + 1) ** 2, status=st)


def _local_set(pkg, L, H, H1, seed):
    rng = np.random.default_rng(seed)
    p = pkg.vbmf_sparse_init(np.zeros((L, 3)), H, alpha0=0.25 + seed, beta0=4.0, gamma0=0.5, delta0=0.75, eta0=0.3, zeta0=0.9, H1=H1, rng=rng)
    p.BHat, p.SigmaB = rng.standard_normal((L, H)), np.diag(rng.uniform(0.1, 1.0, H))
    p.CB, p.delta, p.gamma = rng.uniform(0.5, 2.0, H), rng.uniform(0.5, 2.0, H), 0.5 + L / 2
    return p


def test_factorize_folds_builds_one_call(pkg):
    L, Ms = 12, [1599, 1600, 3, 399, 400, 1]
    pool = _fake_pool(pkg, L, Ms)
    calls = []
    pool.session = type("S", (), {"ctx": _RecCtx(calls)})()
    a, b = _local_set(pkg, L, 2, 1, 0), _local_set(pkg, L, 5, 1, 1)                     # the folds differ in H
    models, tests = [a, (0, 0), (b, "not read"), 0], [[0, 1, 2], [5], [3, 4, 2], [2]]
    out = pkg.factorize_folds(models, tests, pool, threshold=0.25)
    assert len(calls) == 1
    c = calls[0]
    assert c["col_off"] == list(pool.col_off) and c["niter"] == 20 and c["clamp"] is True and c["grouped"] is False
    assert c["job_bag"] == [0, 1, 2, 0, 1, 2, 3, 4, 2, 3, 4, 2] and c["job_model"] == [0] * 3 + [1] * 3 + [2] * 3 + [3] * 3
    assert c["job_full_cov"] == [True, False, True] * 2 + [True, False, True] * 2          # M_b (H - H1) = 1599 | 1600, 1596 | 1600
    assert c["job_trim"] == [-1.0] * 3 + [0.25] * 3 + [-1.0] * 3 + [0.25] * 3
    assert len(c["models"]) == 4
    for t, p in enumerate((a, b)):
        m0, m1, H0 = c["models"][2 * t], c["models"][2 * t + 1], p.H - p.H1
        assert np.array_equal(m0["BHat"], p.BHat[:, :H0]) and np.array_equal(m0["SigmaB"], p.SigmaB[:H0, :H0])
        assert np.array_equal(m0["CB"], p.CB[:H0]) and np.array_equal(m0["delta"], p.delta[:H0]) and m0["gamma"] == p.gamma
        assert (m0["gamma0"], m0["delta0"], m0["eta0"], m0["zeta0"]) == (1e-10,) * 4            # vbmf_sparse_init's defaults (:398-404)
        assert np.array_equal(m0["a_pri"], [1e-10] * H0) and np.array_equal(m0["b_pri"], [1e-10] * H0)
        assert np.array_equal(m0["a_post"], [1e-10 + 0.5] * H0)
        assert np.array_equal(m1["BHat"], p.BHat) and np.array_equal(m1["SigmaB"], p.SigmaB) and np.array_equal(m1["CB"], p.CB)
        assert np.array_equal(m1["delta"], p.delta) and m1["gamma"] == p.gamma
        assert (m1["gamma0"], m1["delta0"], m1["eta0"], m1["zeta0"]) == (0.5, 0.75, 0.3, 0.9)      # what copy_vbmf_params keeps
        assert np.array_equal(m1["a_pri"], [p.alpha0] * p.H) and np.array_equal(m1["b_pri"], [4.0] * p.H)
        assert np.array_equal(m1["a_post"], [p.alpha0 + 0.5] * p.H)
        assert all((m["sigma0"], m["ca0"]) == (1.0, 1.0) for m in (m0, m1))
    assert out[1] is None and out[3] is None
    assert np.array_equal(out[0]["L0"], [-1.0, -2.0, -3.0]) and np.array_equal(out[0]["L1"], [-1001.0, -1002.0, -1003.0])
    assert np.array_equal(out[2]["err0"], [204.0, 205.0, 203.0]) and np.array_equal(out[2]["err1"], [304.0, 305.0, 303.0])
    assert not out[0]["status"].any() and out[0]["status"].dtype == np.int64
    # classify_folds: the two classifiers from the same scores; niter and threshold reach the call
    del calls[:]
    lb = pkg.classify_folds(models, tests, pool, "lower_bound", niter=7, threshold=0.5)
    assert calls[0]["niter"] == 7 and calls[0]["job_trim"][3:6] == [0.5] * 3 and lb[1] is None
    assert np.array_equal(lb[0][0], [0, 0, 0]) and lb[0][0].dtype == np.int64 and np.array_equal(lb[0][1], out[0]["L0"])     # L1 < L0
    me = pkg.classify_folds(models, tests, pool, "min_err")
    assert calls[-1]["niter"] == 20 and calls[-1]["job_trim"][3:6] == [1e-1] * 3
    assert np.array_equal(me[2][1], out[2]["err0"]) and np.array_equal(me[2][0], [1, 1, 1])       # |204 - 304| / 204 >= 0.1
    assert np.array_equal(pkg.classify_folds(models, tests, pool, "min_err", threshold=0.6)[2][0], [0, 0, 0])
    # nothing to classify: no call at all
    del calls[:]
    assert pkg.factorize_folds([(0, 0), 0], [[1], [2]], pool) == [None, None]
    out = pkg.factorize_folds([a], [[]], pool)
    assert calls == [] and all(v.size == 0 for v in out[0].values())
    # a failed job fails its fold after the others were computed
    pool.session = type("S", (), {"ctx": _RecCtx(calls, status_of=[10])})()              # fold 2, the whole basis, bag 4
    with pytest.raises(pkg.VbmfError, match="classify_folds: fold 2: vbls! of bag 4 against the whole basis") as e:
        pkg.classify_folds(models, tests, pool, "lower_bound")
    assert e.value.code == pkg.capi.VBMF_ERR_NUMERIC and e.value.results[2] is None and e.value.results[1] is None
    assert np.array_equal(e.value.results[0][1], [-1.0, -2.0, -3.0])
    with pytest.raises(pkg.VbmfError, match="factorize_folds: fold 2") as e:
        pkg.factorize_folds(models, tests, pool)
    assert e.value.results[2] is None and np.array_equal(e.value.results[0]["L0"], [-1.0, -2.0, -3.0])
    # test_classification_folds counts from those labels
    pool.session = type("S", (), {"ctx": _RecCtx(calls)})()
    summ = pkg.test_classification_folds(models, tests, pool, [0, 1, 1, 0, 0, 1], "min_err")
    assert summ[1] == (-1.0,) * 6 and summ[3] == (-1.0,) * 6 and summ[0][2:] == (1, 0, 1, 2)      # every label 1: bag 0 a false positive


def test_test_classification_folds_forwards_only_what_it_was_given(pkg, monkeypatch):
    pool = _fake_pool(pkg, 12, [3, 1])
    seen = []

    def stub(ms, ts, ys, class_alg="ols", **kw):
        seen.append((class_alg, kw))
        return [(np.array([0]), np.zeros(1), np.zeros(1))]
    monkeypatch.setattr(pkg, "classify_folds", stub)
    pkg.test_classification_folds(["m"], [[0]], pool, [0, 1], "min_err")
    pkg.test_classification_folds(["m"], [[0]], pool, [0, 1], "lower_bound", niter=3, threshold=0.5)
    pkg.test_classification_folds(["m"], [[0]], pool, [0, 1], "ols", threshold=0.2)
    assert seen == [("min_err", {}), ("lower_bound", dict(niter=3, threshold=0.5)), ("ols", dict(threshold=0.2))]


def test_validate_local_folds_trains_with_train_local_folds(pkg, monkeypatch):
    pool = _fake_pool(pkg, 12, [3, 1, 4, 2, 5, 1, 2, 2])
    labels = [0, 1, 1, 0, 0, 1, 0, 1]
    splits = [([5, 0, 1, 3, 2], [4, 6, 7]), ([7, 6, 4], [0, 1])]
    seen = {}
    rng = np.random.default_rng(1)

    def train_local(folds, H, H1, niter, **kw):
        seen["train"] = (folds, H, H1, niter, kw)
        return ["m0", "m1"]

    def summarise(models, tests, Ys, lab, class_alg="ols", **kw):
        seen["test"] = (models, tests, Ys, list(lab), class_alg, kw)
        return ["t0", "t1"]
    monkeypatch.setattr(pkg, "train_local_folds", train_local)
    monkeypatch.setattr(pkg, "test_classification_folds", summarise)
    out = pkg.validate_local_folds(pool, labels, splits, 5, 2, 20, eps=1e-4, class_alg="min_err", threshold=0.2, diag_var=True, rng=rng)
    assert out == ["t0", "t1"]
    folds, H, H1, niter, kw = seen["train"]
    assert folds == [([0, 3], [5, 1, 2]), ([6, 4], [7])] and (H, H1, niter) == (5, 2, 20)
    assert kw == dict(eps=1e-4, rng=rng, diag_var=True, form="stream", slice_cols=None, pool=pool)
    assert seen["test"] == (["m0", "m1"], [[4, 6, 7], [0, 1]], pool, labels, "min_err", dict(threshold=0.2))
    pkg.validate_local_folds(pool, labels, splits, 5, 1, 20)
    assert seen["train"][4]["eps"] == 1e-6 and seen["test"][4] == "lower_bound" and seen["test"][5] == dict(threshold=1e-1)


# ---- 2. host refusals -----------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(pkg, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the host touched the device before refusing")
    monkeypatch.setattr(pkg.capi, "lib", boom)
    monkeypatch.setattr(pkg.capi.Context, "__init__", boom)
    monkeypatch.setattr(pkg.Session, "__init__", boom)
    return pkg


def test_host_refusals(no_device):
    pkg = no_device
    rng = np.random.default_rng(0)
    L, H = 12, 3
    Ms = [3, 1, 4, 2]
    Ys = [rng.standard_normal((L, m)) for m in Ms]
    pool, closed = _fake_pool(pkg, L, Ms), _fake_pool(pkg, L, Ms, closed=True)
    good = _local_set(pkg, L, H, 1, 0)
    noH1, allH1 = _local_set(pkg, L, H, 0, 1), _local_set(pkg, L, H, H, 2)
    dual = pkg.vbmf_dual_init(np.zeros((L, 3)), H, 2, rng=rng)
    basic = pkg.vbmf_init(np.zeros((L, 3)), H, rng=rng)
    big = _local_set(pkg, L, 33, 1, 3)
    tall = _local_set(pkg, L + 1, H, 1, 4)
    nan = _local_set(pkg, L, H, 1, 5); nan.BHat[3, 1] = np.nan
    inf = _local_set(pkg, L, H, 1, 6); inf.delta[0] = np.inf

    class Bare:
        pass
    Bare.H, Bare.BHat = H, np.zeros((L, H))

    def runs(fn):
        if fn == "factorize_folds":
            return lambda ms, ts, ys, **kw: pkg.factorize_folds(ms, ts, ys, **kw)
        if fn == "classify_folds":
            return lambda ms, ts, ys, **kw: pkg.classify_folds(ms, ts, ys, "lower_bound", **kw)
        return lambda ms, ts, ys, **kw: pkg.test_classification_folds(ms, ts, ys, [0, 1, 0, 1], "min_err", **kw)

    for fn in ("factorize_folds", "classify_folds", "test_classification_folds"):
        f = runs(fn)
        for ys in (Ys, pool):
            for bad, what in ((noH1, "H1 = 0"), (allH1, "H1 = 3"), (dual, "vbmf_dual_parameters"), (basic, "vbmf_parameters"), (Bare(), "Bare"),
                              ((dual, good), "vbmf_dual_parameters")):
                with pytest.raises(ValueError, match="fold 1.*vbmf_sparse_parameters with 0 < H1 < H.*" + what):
                    f([good, bad], [[0], [1]], ys)
            with pytest.raises(ValueError, match="fold 0.*H = 33 > 32"):
                f([big], [[0]], ys)
            with pytest.raises(ValueError, match="fold 0.*L = 12 rows"):
                f([tall], [[0]], ys)
            with pytest.raises(ValueError, match="fold 2.*not finite"):
                f([good, (0, 0), nan], [[0], [1], [2]], ys)
            with pytest.raises(ValueError, match="fold 0.*not finite"):
                f([inf], [[0]], ys)
            for thr in (np.nan, np.inf, -0.5):
                with pytest.raises(ValueError, match="threshold"):
                    f([good], [[0]], ys, threshold=thr)
            with pytest.raises(ValueError, match="niter = 0 < 1"):
                f([good], [[0]], ys, niter=0)
            with pytest.raises(ValueError, match=fn + ".*fold 0: bag index 4 outside 0..3"):
                f([good], [[0, 4]], ys)
            with pytest.raises(ValueError, match=fn + ".*fold 1.*not an integer"):
                f([good, good], [[0], [1.5]], ys)
            with pytest.raises(ValueError, match=fn + ".*2 models but 1 test"):
                f([good, good], [[0]], ys)
        with pytest.raises(ValueError, match="closed"):
            f([good], [[0]], closed)
        with pytest.raises(ValueError, match="row counts"):
            f([good], [[0]], Ys[:2] + [np.zeros((L + 1, 2))])
        # an untrained fold takes no model check and gives None
        assert f([(0, 0), 0], [[0], [1]], pool) in ([None, None], [(-1.0,) * 6] * 2)
    fn = "validate_local_folds"
    labels = [0, 1, 0, 1]
    for alg in ("ols", "dual", "vbls", "nonsense"):
        with pytest.raises(ValueError, match=fn + ".*class_alg = '" + alg + "'.*'lower_bound' or 'min_err'"):
            pkg.validate_local_folds(pool, labels, [([0, 1], [2, 3])], H, 1, 5, class_alg=alg)
    with pytest.raises(ValueError, match=fn + ".*BagPool"):
        pkg.validate_local_folds(Ys, labels, [([0, 1], [2, 3])], H, 1, 5)
    with pytest.raises(ValueError, match=fn + ".*closed"):
        pkg.validate_local_folds(closed, labels, [([0, 1], [2, 3])], H, 1, 5)
    for H1 in (0, H):
        with pytest.raises(ValueError, match=fn + ".*0 < H1 < H"):
            pkg.validate_local_folds(pool, labels, [([0, 1], [2, 3])], H, H1, 5)
    with pytest.raises(ValueError, match=fn + ".*H = 33 > 32"):
        pkg.validate_local_folds(pool, labels, [([0, 1], [2, 3])], 33, 1, 5)
    with pytest.raises(ValueError, match=fn + ".*4 bags but 3 labels"):
        pkg.validate_local_folds(pool, labels[:3], [([0, 1], [2, 3])], H, 1, 5)
    with pytest.raises(ValueError, match=fn + ".*outside 0"):
        pkg.validate_local_folds(pool, labels, [([0, 1], [2, 4])], H, 1, 5)
