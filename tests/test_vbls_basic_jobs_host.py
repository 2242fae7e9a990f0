"""vbls! of the basic model for a list of (bag, model) jobs in one device call (vbmf_fixed_basis_jobs; vbls_jobs_, classify_folds with
class_alg = "vbls"): the parts that need no GPU -- the C ABI is declared, exported and bound by both hosts, the job tables and
per-model arrays the Python host builds, its refusals before any device call, and the fp64 reference that
tests/test_gpu_vbls_basic_jobs.py compares with (oracle_job).

oracle_job is the oracle's literal vbls! (O.vbls_ on O.copy_vbmf_params' set).  Its updateSigma2 forms an M_b x M_b product per
iteration (src/vbmf.jl:153-157, kept faithfully), which at the 4865 columns the placement rule reaches at H = 1 is 190 MB per
iteration; above WIDE columns the same loop runs with the oracle's own updateSigma2_fused ("same value as updateSigma2") instead,
pinned here to the literal loop on bags the literal loop can take."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import __graft_entry__ as G
from oracle import vbmf_oracle as O
from tests.helpers import relF
from tests.test_classify_folds_host import _fake_pool
from tests.test_julia_binding import header_prototypes

ENTRY = "vbmf_fixed_basis_jobs"
FIELDS = ("AHat", "SigmaA", "CA", "sigma2", "r2")
SHAPES = [(33, 5), (300, 5), (20, 1), (30, 16), (40, 17), (64, 32)]
WIDTHS = [1, 2, 3, 7, 8, 9, 17, 64, 70]
WIDE = 1000


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def _model(L, H, seed, Mtrain=400):
    """A basis trained by the oracle's vbmf! on toy data (one active column of a random basis per data column, noise 0.05), and a
    sampler of bags in its row space: draw(columns, seed), the same bag whenever it is asked for"""
    rng = np.random.default_rng(seed)
    Bs = rng.standard_normal((L, H)) * np.linspace(1.0, 2.5, H)

    def draw(m, seed):
        r = np.random.default_rng(seed)
        As = np.zeros((m, H)); As[np.arange(m), r.integers(0, H, m)] = 1.0
        return Bs @ As.T + 0.05 * r.standard_normal((L, m))
    Ytr = draw(Mtrain, seed + 2)
    po = O.vbmf_init(Ytr, H, ca=0.1, cb=0.1, sigma2=0.1, rng=np.random.default_rng(seed + 1), materialize_yhat=False)
    O.vbmf_(Ytr, po, 15, eps=0.0, est_covs=True, est_var=True)
    return po, draw


@functools.lru_cache(maxsize=None)
def basic_models(L, H):
    """two (trained set, sampler) per (L, H); computed once and left unchanged"""
    return [_model(L, H, 6000 + 10 * H + k + L) for k in range(2)]


def oracle_job(Y, po, niter, seed=0, wide=WIDE):
    """FIELDS of one job from the oracle: vbls! on copy_vbmf_params' set for this bag, and norm(Y - BHat*AHat')^2"""
    q = O.copy_vbmf_params(Y, po, rng=np.random.default_rng(seed))
    if Y.shape[1] <= wide:
        O.vbls_(Y, q, niter)
    else:
        trYY = O.norm2(Y)
        for _ in range(niter):
            O.updateA(Y, q)
            O.updateCA(q)
            O.updateSigma2_fused(Y, q, trYY, Y @ q.AHat)
    R = Y - po.BHat @ q.AHat.T
    return dict(AHat=q.AHat, SigmaA=q.SigmaA, CA=np.diag(q.CA).copy(), sigma2=float(q.sigma2), r2=float(np.sum(R * R)))


def test_the_wide_bags_reference_is_the_literal_loop():
    """oracle_job above WIDE columns against O.vbls_ itself, on bags both can take: two fp64 evaluations of one recurrence"""
    for (L, H), niter in zip(SHAPES, (150, 20, 150, 20, 150, 20)):
        po, draw = basic_models(L, H)[0]
        for w in (1, 9, 70):
            Y = draw(w, w)
            lit, fused = oracle_job(Y, po, niter), oracle_job(Y, po, niter, wide=0)
            for f in FIELDS:
                e = abs(fused[f] - lit[f]) / abs(lit[f]) if np.isscalar(lit[f]) else relF(fused[f], lit[f])
                assert e <= 1e-10, (L, H, w, f, e)


# ---- 0. ABI and bindings ---------------------------------------------------------------------------------------------------------
def test_abi_and_bindings(pkg):
    protos = header_prototypes()
    lib = ctypes.CDLL(pkg.capi.LIB_PATH)
    assert set(pkg.capi.SYMBOLS) == set(protos)
    assert ENTRY in protos and hasattr(lib, ENTRY) and ENTRY in pkg.capi.SYMBOLS
    d, i = "double*", "int64_t*"
    assert protos[ENTRY] == ("int", ["vbmf_ctx*", "int64_t", i, "int64_t", "int64_t", i, d, d, d, d, "int64_t", i, i, d, d, d, d, d, i])
    assert len(getattr(pkg.capi.lib(), ENTRY).argtypes) == len(protos[ENTRY][1])
    assert protos["vbmf_debug_fixed_basis_jobs_lds_cols"] == ("int", ["int64_t"])
    hdr = open(os.path.join(G.ROOT, "include", "vbmf_hip.h")).read()
    for cite in ("examples/mil_util.jl:182-185", "examples/mil_util.jl:469-479"):
        assert cite in hdr, cite
    jl = open(os.path.join(G.PKG_DIR, "julia", "VBMatrixFactorizationHIP.jl")).read()
    assert re.search(r"ccall\(\(:" + ENTRY + r",\s*libvbmf\)", jl)
    assert re.search(r"^function fixed_basis_jobs\(", jl, flags=re.M)
    assert re.search(r"export[^\n]*(\n\s+[^\n]*)*[ ,]fixed_basis_jobs\b", jl)
    assert hasattr(pkg, "vbls_jobs_") and "vbls_jobs_" in pkg.__all__
    assert hasattr(pkg.capi.Context, "fixed_basis_jobs")
    # the placement rule the host sizes LDS by, through the exported query: one more column does not fit
    for H in (1, 5, 16, 17, 32):
        w = pkg.capi.fixed_basis_jobs_lds_cols(H)
        NP = 16 if H <= 16 else 32
        fixed = max(4 * NP * (NP + 2), 8 * 256 + 256)
        assert w * H <= 56 * 1024 // 8 - fixed < (w + 1) * H, (H, w)
    assert pkg.capi.fixed_basis_jobs_lds_cols(33) == 0 and pkg.capi.fixed_basis_jobs_lds_cols(0) == 0


def test_the_job_kernel_shares_the_loop_and_the_product():
    """one vbls_loop_dev for the one-basis kernels and the job kernel; one vjobs_product for the ARD jobs and these"""
    src = {f: open(os.path.join(G.PKG_DIR, "csrc", f)).read() for f in ("ctrl_kernels.hpp", "vbls_jobs_kernels.hpp", "vbls_basic_jobs_kernels.hpp")}
    assert len(re.findall(r"__device__[^;{]*\bvbls_loop_dev\s*\(", "".join(src.values()))) == 1
    assert len(re.findall(r"__device__[^;{]*\bvjobs_product\s*\(", "".join(src.values()))) == 1
    for f, kernel, calls in (("ctrl_kernels.hpp", "vbls_loop_kernel", ("vbls_loop_dev<NB>",)), ("ctrl_kernels.hpp", "vbls_batch_kernel", ("vbls_loop_dev<NB>",)),
                             ("vbls_basic_jobs_kernels.hpp", "vbls_basic_jobs_kernel", ("vbls_loop_dev<NBK>", "vjobs_product<MODE>")),
                             ("vbls_jobs_kernels.hpp", "vbls_jobs_kernel", ("vjobs_product<MODE>",))):
        m = re.search(r"__global__[^;{]*?\b" + kernel + r"\s*\([^{]*\{", src[f])
        body = src[f][m.end():src[f].find("\n}\n", m.end())]
        for c in calls:
            assert c + "(" in body, (kernel, c)


# ---- 1. job tables and per-model arrays ------------------------------------------------------------------------------------------
class _RecCtx:
    def __init__(self, calls, status_of=None):
        self.calls, self.status_of = calls, status_of

    def fixed_basis_jobs(self, col_off, models, job_bag, job_model, niter):
        self.calls.append(dict(col_off=list(col_off), models=list(models), job_bag=list(job_bag), job_model=list(job_model), niter=niter))
        off = np.asarray(col_off)
        nj = len(job_bag)
        st = np.zeros(nj, dtype=np.int64)
        if self.status_of is not None:
            st[self.status_of] = 1
        Hs = [models[k]["BHat"].shape[1] for k in job_model]
        r2 = np.array([(100.0 * k + b + 1) ** 2 for b, k in zip(job_bag, job_model)])
        return dict(r2=r2, sigma2=np.arange(nj) + 2.0, status=st,
                    AHat=[np.full((int(off[b + 1] - off[b]), H), j + 0.5) for j, (b, H) in enumerate(zip(job_bag, Hs))],
                    SigmaA=[np.full((H, H), j + 0.25) for j, H in enumerate(Hs)], CA=[np.arange(H) + j + 1.0 for j, H in enumerate(Hs)])


def _basic_set(pkg, L, H, seed):
    rng = np.random.default_rng(seed)
    p = pkg.vbmf_init(np.zeros((L, 3)), H, rng=rng)
    p.BHat, p.SigmaB = rng.standard_normal((L, H)), np.diag(rng.uniform(0.1, 1.0, H))
    p.CB = np.diag(rng.uniform(0.5, 2.0, H)); p.invCB = np.diag(1.0 / np.diag(p.CB))
    p.sigma2 = 0.25 + seed
    return p


def test_classify_folds_vbls_builds_one_call(pkg):
    L, Ms = 12, [3, 1, 4, 2, 5, 1]
    pool = _fake_pool(pkg, L, Ms)
    calls = []
    pool.session = type("S", (), {"ctx": _RecCtx(calls)})()
    res = [_basic_set(pkg, L, H, s) for s, H in enumerate((3, 3, 4, 2, 3, 32))]           # a fold's two models may differ in H
    folds = [(res[0], res[1]), (res[2], res[3]), (res[4], res[5])]
    tests = [[4, 0, 4], [5], [1, 2]]
    out = pkg.classify_folds(folds, tests, pool, "vbls")
    assert len(calls) == 1
    c = calls[0]
    assert c["col_off"] == [0, 3, 4, 8, 10, 15, 16] and c["niter"] == 150
    assert c["job_bag"] == [4, 0, 4, 4, 0, 4, 5, 5, 1, 2, 1, 2] and c["job_model"] == [0, 0, 0, 1, 1, 1, 2, 3, 4, 4, 5, 5]
    assert len(c["models"]) == 6
    for m, p in zip(c["models"], res):
        assert sorted(m) == ["BHat", "SigmaB", "ca0", "sigma2_0"]
        assert np.array_equal(m["BHat"], p.BHat) and np.array_equal(m["SigmaB"], p.SigmaB)
        assert (m["sigma2_0"], m["ca0"]) == (p.sigma2, 1.0)                                 # copy_vbmf_params: old.sigma2, CA = I
    for f, (labels, e0, e1) in enumerate(out):
        assert np.array_equal(e0, np.array([200.0 * f + b + 1 for b in tests[f]]))          # sqrt(r2), :483-484
        assert np.array_equal(e1, np.array([100.0 * (2 * f + 1) + b + 1 for b in tests[f]]))
        assert np.array_equal(labels, np.zeros(len(tests[f]), dtype=np.int64)) and labels.dtype == np.int64   # err0 > err1 nowhere: 0
    # niter overrides; an untrained fold and an empty test list contribute no jobs; the trained folds' models keep their order
    del calls[:]
    out = pkg.classify_folds([folds[0], (0, 0), folds[1], folds[2]], [[], [3], np.array([2, 0]), [1]], pool, "vbls", niter=7)
    assert len(calls) == 1 and calls[0]["niter"] == 7 and len(calls[0]["models"]) == 6
    assert calls[0]["job_bag"] == [2, 0, 2, 0, 1, 1] and calls[0]["job_model"] == [2, 2, 3, 3, 4, 5]
    assert out[1] is None and all(a.size == 0 for a in out[0]) and out[0][0].dtype == np.int64
    assert np.array_equal(out[2][1], [203.0, 201.0]) and np.array_equal(out[2][2], [303.0, 301.0])
    # label 1 where err0 > err1: swap a fold's models
    del calls[:]
    out = pkg.classify_folds([(res[1], res[0])], [[0, 2]], pool, "vbls")
    assert calls[0]["job_model"] == [0, 0, 1, 1] and np.array_equal(out[0][0], [0, 0])
    # nothing to classify: no call at all
    del calls[:]
    assert pkg.classify_folds([(0, 0), (0, 0)], [[1], [2]], pool, "vbls") == [None, None]
    out = pkg.classify_folds([folds[0]], [[]], pool, "vbls")
    assert calls == [] and all(a.size == 0 for a in out[0])
    # a failed job fails its fold after the others were computed
    pool.session = type("S", (), {"ctx": _RecCtx(calls, status_of=[7])})()           # fold 1, res1, bag 5
    with pytest.raises(pkg.VbmfError, match="classify_folds: fold 1: vbls! of bag 5 against res1") as e:
        pkg.classify_folds(folds, tests, pool, "vbls")
    assert e.value.code == pkg.capi.VBMF_ERR_NUMERIC and e.value.results[1] is None
    assert np.array_equal(e.value.results[2][0], [0, 0]) and len(e.value.results[0][1]) == 3
    # test_classification_folds counts from those labels
    pool.session = type("S", (), {"ctx": _RecCtx(calls)})()
    labels = [0, 1, 1, 0, 0, 1]
    summ = pkg.test_classification_folds(folds + [(0, 0)], tests + [[0]], pool, labels, "vbls")
    assert summ[3] == (-1.0,) * 6 and summ[0][2:] == (0, 0, 3, 0) and summ[2][2:] == (0, 2, 0, 2)
    del calls[:]
    pkg.test_classification_folds(folds, tests, pool, labels, "vbls", niter=9)
    assert len(calls) == 1 and calls[0]["niter"] == 9


def test_validate_folds_vbls_trains_the_basic_model(pkg, monkeypatch):
    pool = _fake_pool(pkg, 12, [3, 1, 4, 2, 5, 1, 2, 2])
    labels = [0, 1, 1, 0, 0, 1, 0, 1]
    splits = [([5, 0, 1, 3, 2], [4, 6, 7]), ([7, 6, 4], [0, 1])]
    seen = {}

    def train(folds, solver, H, niter, **kw):
        seen["train"] = (folds, solver, H, niter, kw)
        return ["m0", "m1"]

    def summarise(models, tests, Ys, lab, class_alg="ols"):
        seen["test"] = (models, tests, Ys, list(lab), class_alg)
        return ["t0", "t1"]

    monkeypatch.setattr(pkg, "train_folds", train)
    monkeypatch.setattr(pkg, "test_classification_folds", summarise)
    assert pkg.validate_folds(pool, labels, splits, "basic", 5, 30, eps=1e-3, class_alg="vbls") == ["t0", "t1"]
    folds, solver, H, niter, kw = seen["train"]
    assert folds == [([0, 3], [5, 1, 2]), ([6, 4], [7])] and (solver, H, niter) == ("basic", 5, 30) and kw["eps"] == 1e-3 and kw["pool"] is pool
    assert seen["test"] == (["m0", "m1"], [[4, 6, 7], [0, 1]], pool, labels, "vbls")
    # any other solver: refused before training
    monkeypatch.setattr(pkg, "train_folds", lambda *a, **k: pytest.fail("refused before training"))
    for solver in ("sparse", "dual", "trial", "nonsense"):
        with pytest.raises(ValueError, match="validate_folds: class_alg = 'vbls' with solver = '" + solver + "'.*'ols', 'rls' or 'dual'.*per fold with classify_bags"):
            pkg.validate_folds(pool, labels, splits, solver, 5, 30, class_alg="vbls")
    with pytest.raises(ValueError, match="validate_folds.*H = 33 > 32"):
        pkg.validate_folds(pool, labels, splits, "basic", 33, 30, class_alg="vbls")


def test_vbls_jobs_fills_the_sets(pkg):
    L, Ms = 12, [3, 1, 4]
    pool = _fake_pool(pkg, L, Ms)
    calls = []
    pool.session = type("S", (), {"ctx": _RecCtx(calls)})()
    res = [_basic_set(pkg, L, 3, 0), _basic_set(pkg, L, 5, 1)]
    sets, r2, status = pkg.vbls_jobs_(pool, res, [2, 0, 2], [1, 0, 0], 9)
    assert len(calls) == 1 and calls[0]["niter"] == 9 and calls[0]["job_bag"] == [2, 0, 2] and calls[0]["job_model"] == [1, 0, 0]
    assert [(m["sigma2_0"], m["ca0"]) for m in calls[0]["models"]] == [(0.25, 1.0), (1.25, 1.0)]
    assert np.array_equal(r2, [103.0 ** 2, 1.0, 9.0]) and not status.any()
    for j, (p, b, k) in enumerate(zip(sets, [2, 0, 2], [1, 0, 0])):
        H = res[k].H
        assert type(p) is pkg.vbmf_parameters and (p.L, p.M, p.H, p.H1) == (L, Ms[b], H, 0) and p.labels.size == 0
        assert all(np.array_equal(getattr(p, f), getattr(res[k], f)) and getattr(p, f) is not getattr(res[k], f) for f in ("BHat", "SigmaB", "CB", "invCB"))
        assert np.array_equal(p.AHat, np.full((Ms[b], H), j + 0.5)) and np.array_equal(p.SigmaA, np.full((H, H), j + 0.25))
        assert np.array_equal(p.CA, np.diag(np.arange(H) + j + 1.0)) and np.array_equal(p.invCA, np.diag(1.0 / (np.arange(H) + j + 1.0)))
        assert p.sigma2 == j + 2.0 and p.YHat is None


# ---- 2. host refusals ------------------------------------------------------------------------------------------------------------
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
    b = [_basic_set(pkg, L, H, s) for s in range(2)]
    b4 = _basic_set(pkg, L, 4, 5)
    b33 = _basic_set(pkg, L, 33, 6)
    bL = _basic_set(pkg, L + 1, H, 7)
    bn = _basic_set(pkg, L, H, 8); bn.BHat[3, 1] = np.nan
    bs = _basic_set(pkg, L, H, 9); bs.SigmaB[1, 1] = np.inf
    b2 = _basic_set(pkg, L, H, 10); b2.sigma2 = np.nan
    dual = pkg.vbmf_dual_init(np.zeros((L, 3)), H, 2, rng=rng)
    sp = pkg.vbmf_sparse_init(np.zeros((L, 3)), H)
    fn = "vbls_jobs_"
    for ys in (Ys, pool):
        with pytest.raises(ValueError, match=fn + ".*no models"):
            pkg.vbls_jobs_(ys, [], [0], [0], 5)
        with pytest.raises(ValueError, match=fn + ".*model 1 is a vbmf_dual_parameters.*vbmf_parameters only"):
            pkg.vbls_jobs_(ys, [b[0], dual], [0], [0], 5)
        with pytest.raises(ValueError, match=fn + ".*model 0 is a vbmf_sparse_parameters"):
            pkg.vbls_jobs_(ys, [sp], [0], [0], 5)
        with pytest.raises(ValueError, match=fn + ".*model 0 is a object"):
            pkg.vbls_jobs_(ys, [object()], [0], [0], 5)
        with pytest.raises(ValueError, match=fn + ".*model 1: H = 33 > 32"):
            pkg.vbls_jobs_(ys, [b[0], b33], [0], [0], 5)
        with pytest.raises(ValueError, match=fn + ".*niter = 0 < 1"):
            pkg.vbls_jobs_(ys, [b[0]], [0], [0], 0)
        with pytest.raises(ValueError, match=fn + ".*model 0.*L = 12 rows"):
            pkg.vbls_jobs_(ys, [bL], [0], [0], 5)
        for k, bad in enumerate((bn, bs, b2)):
            with pytest.raises(ValueError, match=fn + ".*model 1.*not finite"):
                pkg.vbls_jobs_(ys, [b[0], bad], [0], [0], 5)
        with pytest.raises(ValueError, match=fn + ".*2 job bags and 1 job models"):
            pkg.vbls_jobs_(ys, [b[0]], [0, 1], [0], 5)
        with pytest.raises(ValueError, match=fn + ".*0 job bags"):
            pkg.vbls_jobs_(ys, [b[0]], [], [], 5)
        with pytest.raises(ValueError, match=fn + ".*job 1: bag 4 outside 0..3"):
            pkg.vbls_jobs_(ys, [b[0]], [0, 4], [0, 0], 5)
        with pytest.raises(ValueError, match=fn + ".*job 0: bag -1 outside"):
            pkg.vbls_jobs_(ys, [b[0]], [-1], [0], 5)
        with pytest.raises(ValueError, match=fn + ".*job 0: model 1 outside 0..0"):
            pkg.vbls_jobs_(ys, [b[0]], [0], [1], 5)
    with pytest.raises(ValueError, match=fn + ".*closed"):
        pkg.vbls_jobs_(closed, [b[0]], [0], [0], 5)
    with pytest.raises(ValueError, match=fn + ".*row counts"):
        pkg.vbls_jobs_(Ys[:2] + [np.zeros((L + 1, 2))], [b[0]], [0], [0], 5)
    for fn, call in (("classify_folds", lambda models, tests, ys, **kw: pkg.classify_folds(models, tests, ys, "vbls", **kw)),
                     ("test_classification_folds", lambda models, tests, ys, **kw: pkg.test_classification_folds(models, tests, ys, [0, 1, 0, 1], "vbls", **kw))):
        for ys in (Ys, pool):
            with pytest.raises(ValueError, match=fn + ".*fold 0.*a pair"):
                call([(b[0], b[1], b[0])], [[0]], ys)
            with pytest.raises(ValueError, match=fn + ".*fold 0.*a pair"):
                call([b[0]], [[0]], ys)
            with pytest.raises(ValueError, match=fn + ": fold 1: res1 is a vbmf_dual_parameters .class_alg = 'vbls' takes the basic model's vbmf_parameters"):
                call([(b[0], b[1]), (b[0], dual)], [[0], [1]], ys)
            with pytest.raises(ValueError, match=fn + ": fold 0: res0 is a vbmf_sparse_parameters.*'ols', 'rls' or 'dual'.*per fold with classify_bags"):
                call([(sp, b[1])], [[0]], ys)
            with pytest.raises(ValueError, match=fn + ".*fold 2: res0: H = 33 > 32"):
                call([(b[0], b4), (0, 0), (b33, b[1])], [[0], [1], [2]], ys)
            with pytest.raises(ValueError, match=fn + ".*fold 0: res1.*L = 12 rows"):
                call([(b[0], bL)], [[0]], ys)
            for bad in (bn, bs, b2):
                with pytest.raises(ValueError, match=fn + ".*fold 2: res1.*not finite"):
                    call([(b[0], b[1]), (0, 0), (b[0], bad)], [[0], [1], [2]], ys)
            with pytest.raises(ValueError, match=fn + ".*outside 0"):
                call([(b[0], b[1])], [[0, 4]], ys)
            with pytest.raises(ValueError, match=fn + ".*2 models but 1 test"):
                call([(b[0], b[1]), (b[0], b[1])], [[0]], ys)
        with pytest.raises(ValueError, match=fn + ".*closed"):
            call([(b[0], b[1])], [[0]], closed)
    with pytest.raises(ValueError, match="classify_folds.*niter = 0 < 1"):
        pkg.classify_folds([(b[0], b[1])], [[0]], Ys, "vbls", niter=0)
    # validate_folds with "vbls" and another solver: refused before train_folds is reached (no device, no training)
    with pytest.raises(ValueError, match="validate_folds: class_alg = 'vbls' with solver = 'sparse'"):
        pkg.validate_folds(pool, [0, 1, 0, 1], [([0, 1], [2, 3])], "sparse", H, 5, class_alg="vbls")
    # the unknown-algorithm text still matches the two pinned patterns, under each function's own name
    for name, call in (("classify_folds", lambda alg: pkg.classify_folds([(b[0], b[1])], [[0]], Ys, alg)),
                       ("test_classification_folds", lambda alg: pkg.test_classification_folds([(b[0], b[1])], [[0]], Ys, [0, 1, 0, 1], alg)),
                       ("validate_folds", lambda alg: pkg.validate_folds(pool, [0, 1, 0, 1], [([0, 1], [2, 3])], "basic", H, 5, class_alg=alg))):
        for pat in (name + ".*class_alg.*classify_bags", "class_alg = 'nonsense'.*'ols', 'rls' or 'dual'.*per fold with classify_bags"):
            with pytest.raises(ValueError, match=pat):
                call("nonsense")
    # validate_local_folds keeps to its two classifiers
    with pytest.raises(ValueError, match="validate_local_folds.*class_alg = 'vbls'"):
        pkg.validate_local_folds(pool, [0, 1, 0, 1], [([0, 1], [2, 3])], 4, 1, 5, class_alg="vbls")
