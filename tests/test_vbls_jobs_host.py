"""vbls! for a list of (bag, model) jobs in one device call (vbmf_sparse_fixed_basis_jobs; vbls_sparse_jobs_, classify_folds with
class_alg = "dual"): the parts that need no GPU -- the job tables and per-model arrays the Python host builds, its refusals before any
device call, and the block-wise fp64 reference (ref_vbls) that tests/test_gpu_vbls_jobs.py uses where the oracle's dense
M_b H x M_b H inverse is too large, pinned here to the oracle's own loop on small bags."""
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as G
from oracle import vbmf_oracle as O
from tests.helpers import relF
from tests.test_classify_folds_host import _fake_pool
from tests.test_gpu_vbls_sparse_batch import _convert, _pkg_type
from tests.test_julia_binding import header_prototypes

ENTRY = "vbmf_sparse_fixed_basis_jobs"
FIELDS = ("ATVecHat", "diagSigmaATVec", "CA", "beta", "SigmaA", "sigmaHat", "zeta")


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


# ---- the block-wise reference ---------------------------------------------------------------------------------------------------
def model_arrays(po):
    """The per-model inputs of the entry from an oracle (or package) parameter set: updateCA!'s (alpha_h, beta0_h) by column group
    (src/vbmf_sparse.jl:284-288, src/vbmf_dual.jl:322-351) and the start values copy_vbmf_params gives (CA = ones, sigmaHat = 1)."""
    H = int(po.H)
    if hasattr(po, "alpha00"):
        first = np.arange(H) < int(po.H0)
        alpha = np.where(first, po.alpha00, po.alpha01) + 0.5
        beta0 = np.where(first, po.beta00, po.beta01).astype(np.float64)
    else:
        alpha, beta0 = np.full(H, po.alpha0 + 0.5), np.full(H, float(po.beta0))
    return dict(BHat=np.array(po.BHat, dtype=np.float64), SigmaB=np.array(po.SigmaB, dtype=np.float64), alpha=alpha, beta0=beta0,
                eta0=float(po.eta0), zeta0=float(po.zeta0), sigma0=1.0, ca0=1.0)


def ref_vbls(Y, m, niter, full_cov, compat=True):
    """niter iterations of updateA! (src/vbmf_sparse.jl:178-240), updateCA! (:284-288) and updateSigma! (:317-321) on one bag with one
    model's arrays, in NumPy fp64.  full_cov inverts the M_b blocks sigma G + diag(CA[m, :]) one by one -- the dense
    M_b H x M_b H matrix of the reference is block diagonal -- so a wide bag costs M_b inverses of H x H.  Returns FIELDS and r2."""
    B, SB = m["BHat"], m["SigmaB"]
    (L, M), H = Y.shape, B.shape[1]
    G0 = B.T @ B
    Gm = G0 + L * SB
    P = Y.T @ B
    yy = float(np.sum(Y * Y))
    eta = m["eta0"] + L * M / 2
    CA = np.full((M, H), float(m["ca0"]))
    sig = float(m["sigma0"])
    for _ in range(niter):
        if full_cov:
            A, dS, SA = np.empty((M, H)), np.empty((M, H)), np.zeros((H, H))
            for c in range(M):
                S = np.linalg.inv(sig * Gm + np.diag(CA[c]))
                A[c], dS[c] = sig * (S @ P[c]), np.diag(S)
                SA += S
        else:
            v = sig * np.diag(G0) + L * np.diag(SB)
            t = np.arange(M * H)
            vi = np.where(t < H, t, (t - H) // max(M - 1, 1)) if compat else t % H        # QS1: repeat(v, inner = M - 1) after the first H
            dS = (1.0 / (v[vi] + CA.reshape(-1))).reshape(M, H)
            A = sig * dS * P
            SA = np.diag(dS.sum(axis=0))
        beta = m["beta0"][None, :] + 0.5 * (A * A + dS)
        CA = m["alpha"][None, :] / beta
        zeta = m["zeta0"] + 0.5 * yy - float(np.sum(P * A)) + 0.5 * (float(np.sum((A @ Gm) * A)) + float(np.sum(SA * Gm)))
        sig = eta / zeta
    R = Y - B @ A.T
    return dict(ATVecHat=A.reshape(-1), diagSigmaATVec=dS.reshape(-1), CA=CA.reshape(-1), beta=beta.reshape(-1), SigmaA=SA,
                sigmaHat=sig, zeta=zeta, r2=float(np.sum(R * R)))


def oracle_vbls(pkg, Y, po, niter, full_cov, seed=0):
    """the oracle's literal loop on the oracle twin of copy_vbmf_params' set for this bag (the package's copy_vbmf_params: the
    oracle's own knows the sparse model only); returns the set"""
    P, Oc = _pkg_type(pkg, po)
    q = _convert(Oc, pkg.copy_vbmf_params(Y, _convert(P, po), rng=np.random.default_rng(seed)))
    dual = isinstance(po, O.vbmf_dual_parameters)
    if not full_cov:
        (O.vbls_dual_ if dual else O.vbls_sparse_)(Y, q, niter)
        return q
    for _ in range(niter):
        (O.dual_updateA if dual else O.sparse_updateA)(Y, q, full_cov=True)
        (O.dual_updateCA if dual else O.sparse_updateCA)(q)
        O.sparse_updateSigma(Y, q)
    return q


def trained(kind, L, H, seed, Mtrain=400, niter=12):
    """(a set trained by the oracle, a sampler of bags in its basis' row space).  400 training columns: with much fewer the oracle's
    fit collapses to BHat = 0 at H >= 17, and vbls! on a zero basis exercises nothing: asserted here on a bag of nine columns, whose
    full_cov fit must leave r2 < ||Y||^2 / 10."""
    rng = np.random.default_rng(seed)
    Bs = rng.standard_normal((L, H)) * np.linspace(1.0, 2.5, H)

    def draw(m):
        As = np.zeros((m, H)); As[np.arange(m), rng.integers(0, H, m)] = 1.0
        return Bs @ As.T + 0.05 * rng.standard_normal((L, m))
    Ytr = draw(Mtrain)
    r = np.random.default_rng(seed + 1)
    if kind == "sparse":
        po = O.vbmf_sparse_init(Ytr, H, rng=r, full_cov=False, materialize_yhat=False)
        O.vbmf_sparse_(Ytr, po, niter, eps=0.0)
    else:
        po = O.vbmf_dual_init(Ytr, H, max(1, H // 2), rng=r, materialize_yhat=False)
        O.vbmf_dual_(Ytr, po, niter, eps=0.0, est_priors=False)
    Y9 = draw(9)
    assert ref_vbls(Y9, model_arrays(po), 20, True)["r2"] < 0.1 * float(np.sum(Y9 * Y9)), (kind, L, H, seed)
    return po, draw


# ---- 0. ABI and bindings ----------------------------------------------------------------------------------------------------------
def test_abi_and_bindings(pkg):
    protos = header_prototypes()
    lib = ctypes.CDLL(pkg.capi.LIB_PATH)
    assert ENTRY in protos and hasattr(lib, ENTRY) and ENTRY in pkg.capi.SYMBOLS
    d, i = "double*", "int64_t*"
    assert protos[ENTRY] == ("int", ["vbmf_ctx*", "int64_t", i, "int64_t", "int64_t", "int", "int64_t", d, d, d, d, d, d, d, d, "int64_t", i, i,
                                     d, d, d, d, d, d, d, d, i])
    assert len(getattr(pkg.capi.lib(), ENTRY).argtypes) == len(protos[ENTRY][1])
    hdr = open(os.path.join(G.ROOT, "include", "vbmf_hip.h")).read()
    for cite in ("examples/mil_util.jl:187-197", "examples/mil_util.jl:515-530"):
        assert cite in hdr, cite
    jl = open(os.path.join(G.PKG_DIR, "julia", "VBMatrixFactorizationHIP.jl")).read()
    assert re.search(r"ccall\(\(:" + ENTRY + r",\s*libvbmf\)", jl)
    assert re.search(r"^function sparse_fixed_basis_jobs\(", jl, flags=re.M)
    assert re.search(r"export[^\n]*(\n\s+[^\n]*)*\bsparse_fixed_basis_jobs\b", jl)
    assert hasattr(pkg, "vbls_sparse_jobs_") and "vbls_sparse_jobs_" in pkg.__all__
    assert hasattr(pkg.capi.Context, "sparse_fixed_basis_jobs")
    # the placement rule the host sizes LDS by, through the exported query: one more column does not fit
    for H in (1, 5, 16, 17, 32):
        for full in (False, True):
            w = pkg.capi.vbls_jobs_lds_cols(H, full)
            fixed = max(4 * (16 * (1 if H <= 16 else 2)) * (16 * (1 if H <= 16 else 2) + 2) + 8 * 16 * (1 if H <= 16 else 2) if full else H * H,
                        8 * 256 + 256)
            assert 4 * w * H <= 56 * 1024 // 8 - fixed < 4 * (w + 1) * H, (H, full, w)
    assert pkg.capi.vbls_jobs_lds_cols(33) == 0 and pkg.capi.vbls_jobs_lds_cols(0) == 0


def test_the_job_kernel_shares_the_loop_of_the_batched_one():
    src = open(os.path.join(G.PKG_DIR, "csrc", "sparse_batch_kernels.hpp")).read() + open(os.path.join(G.PKG_DIR, "csrc", "vbls_jobs_kernels.hpp")).read()
    assert re.search(r"__device__[^;{]*\bsbatch_iterate\b", src)
    for kernel in ("sparse_batch_kernel", "vbls_jobs_kernel"):
        m = re.search(r"__global__[^;{]*?\b" + kernel + r"\s*\([^{]*\{", src)
        body = src[m.end():src.find("\n}\n", m.end())]
        assert re.search(r"\bsbatch_iterate<NBK, FULL>\(", body), kernel


# ---- 1. job tables and per-model arrays -------------------------------------------------------------------------------------------
class _RecCtx:
    def __init__(self, calls, status_of=None):
        self.calls, self.status_of = calls, status_of

    def sparse_fixed_basis_jobs(self, col_off, H, models, job_bag, job_model, niter, full_cov=False):
        self.calls.append(dict(col_off=list(col_off), H=H, models=list(models), job_bag=list(job_bag), job_model=list(job_model),
                               niter=niter, full_cov=full_cov))
        off = np.asarray(col_off)
        w = np.array([off[b + 1] - off[b] for b in job_bag])
        boff = np.concatenate([[0], np.cumsum(w * H)]).astype(np.int64)
        n, nj = int(boff[-1]), len(job_bag)
        st = np.zeros(nj, dtype=np.int64)
        if self.status_of is not None:
            st[self.status_of] = 1
        r2 = np.array([(100.0 * k + b + 1) ** 2 for b, k in zip(job_bag, job_model)])
        return dict(r2=r2, sigmaHat=np.arange(nj) + 2.0, zeta=np.arange(nj) + 3.0, status=st, SigmaA=np.zeros((nj, H, H)),
                    CA=np.arange(n) + 0.5, beta=np.arange(n) + 0.25, diagSigmaATVec=np.arange(n) + 0.125, ATVecHat=np.arange(n) * 1.0,
                    off=boff)


def _dual_set(pkg, L, H, H0, seed):
    rng = np.random.default_rng(seed)
    p = pkg.vbmf_dual_init(np.zeros((L, 3)), H, H0, rng=rng)
    p.BHat, p.SigmaB = rng.standard_normal((L, H)), np.diag(rng.uniform(0.1, 1.0, H))
    p.alpha00, p.beta00, p.alpha01, p.beta01 = 0.7 + seed, 1.5, 2.25, 0.5 + seed
    p.eta0, p.zeta0 = 0.3, 0.9
    return p


def test_classify_folds_dual_builds_one_call(pkg):
    L, Ms, H = 12, [3, 1, 4, 2, 5, 1], 3
    pool = _fake_pool(pkg, L, Ms)
    calls = []
    pool.session = type("S", (), {"ctx": _RecCtx(calls)})()
    res = [_dual_set(pkg, L, H, 2, s) for s in range(6)]
    folds = [(res[0], res[1]), (res[2], res[3]), (res[4], res[5])]
    tests = [[4, 0, 4], [5], [1, 2]]
    out = pkg.classify_folds(folds, tests, pool, "dual")
    assert len(calls) == 1
    c = calls[0]
    assert c["col_off"] == [0, 3, 4, 8, 10, 15, 16] and c["H"] == H and c["niter"] == 20 and c["full_cov"] is True
    assert c["job_bag"] == [4, 0, 4, 4, 0, 4, 5, 5, 1, 2, 1, 2] and c["job_model"] == [0, 0, 0, 1, 1, 1, 2, 3, 4, 4, 5, 5]
    assert len(c["models"]) == 6
    for m, p in zip(c["models"], res):
        assert np.array_equal(m["BHat"], p.BHat) and np.array_equal(m["SigmaB"], p.SigmaB)
        assert np.array_equal(m["alpha"], [p.alpha00 + 0.5, p.alpha00 + 0.5, p.alpha01 + 0.5])         # by column group, H0 = 2
        assert np.array_equal(m["beta0"], [p.beta00, p.beta00, p.beta01])
        assert (m["eta0"], m["zeta0"], m["sigma0"], m["ca0"]) == (0.3, 0.9, 1.0, 1.0)
        want = model_arrays(p)
        assert all(np.array_equal(m[k], want[k]) for k in want)
    for f, (labels, e0, e1) in enumerate(out):
        w = np.array([Ms[b] for b in tests[f]], dtype=np.float64)
        assert np.array_equal(e0, np.array([200.0 * f + b + 1 for b in tests[f]]) / (L * w))           # sqrt(r2) / (L M_b), :523-524
        assert np.array_equal(e1, np.array([100.0 * (2 * f + 1) + b + 1 for b in tests[f]]) / (L * w))
        assert np.array_equal(labels, np.zeros(len(tests[f]), dtype=np.int64)) and labels.dtype == np.int64   # err0 < err1: 0
    # niter overrides; an untrained fold and an empty test list contribute no jobs; the trained folds' models keep their order
    del calls[:]
    out = pkg.classify_folds([folds[0], (0, 0), folds[1], folds[2]], [[], [3], np.array([2, 0]), [1]], pool, "dual", niter=7)
    assert len(calls) == 1 and calls[0]["niter"] == 7 and len(calls[0]["models"]) == 6
    assert calls[0]["job_bag"] == [2, 0, 2, 0, 1, 1] and calls[0]["job_model"] == [2, 2, 3, 3, 4, 5]
    assert out[1] is None and all(a.size == 0 for a in out[0]) and out[0][0].dtype == np.int64
    assert np.array_equal(out[2][1], np.array([203.0, 201.0]) / (L * np.array([4.0, 3.0])))
    # a sparse pair serves as well: one (alpha0 + 1/2, beta0) for every column
    sp = pkg.vbmf_sparse_init(np.zeros((L, 3)), H, alpha0=0.25, beta0=4.0)
    del calls[:]
    pkg.classify_folds([(sp, sp)], [[0]], pool, "dual")
    assert np.array_equal(calls[0]["models"][0]["alpha"], [0.75] * 3) and np.array_equal(calls[0]["models"][1]["beta0"], [4.0] * 3)
    # nothing to classify: no call at all
    del calls[:]
    assert pkg.classify_folds([(0, 0), (0, 0)], [[1], [2]], pool, "dual") == [None, None]
    out = pkg.classify_folds([folds[0]], [[]], pool, "dual")
    assert calls == [] and all(a.size == 0 for a in out[0])
    # a failed job fails its fold after the others were computed
    pool.session = type("S", (), {"ctx": _RecCtx(calls, status_of=[7])})()           # fold 1, res1, bag 5
    with pytest.raises(pkg.VbmfError, match="classify_folds: fold 1: vbls! of bag 5 against res1") as e:
        pkg.classify_folds(folds, tests, pool, "dual")
    assert e.value.code == pkg.capi.VBMF_ERR_NUMERIC and e.value.results[1] is None
    assert np.array_equal(e.value.results[2][0], [0, 0]) and len(e.value.results[0][1]) == 3
    # test_classification_folds counts from those labels; validate_folds trains with train_dual_folds
    pool.session = type("S", (), {"ctx": _RecCtx(calls)})()
    labels = [0, 1, 1, 0, 0, 1]
    summ = pkg.test_classification_folds(folds + [(0, 0)], tests + [[0]], pool, labels, "dual")
    assert summ[3] == (-1.0,) * 6 and summ[0][2:] == (0, 0, 3, 0) and summ[2][2:] == (0, 2, 0, 2)


def test_validate_folds_dual_trains_with_train_dual_folds(pkg, monkeypatch):
    pool = _fake_pool(pkg, 12, [3, 1, 4, 2, 5, 1, 2, 2])
    labels = [0, 1, 1, 0, 0, 1, 0, 1]
    splits = [([5, 0, 1, 3, 2], [4, 6, 7]), ([7, 6, 4], [0, 1])]
    seen = {}
    rng = np.random.default_rng(1)

    def train_dual(folds, H, H0, niter, **kw):
        seen["train"] = (folds, H, H0, niter, kw)
        return ["m0", "m1"]

    def summarise(models, tests, Ys, lab, class_alg="ols"):
        seen["test"] = (models, tests, Ys, list(lab), class_alg)
        return ["t0", "t1"]

    monkeypatch.setattr(pkg, "train_dual_folds", train_dual)
    monkeypatch.setattr(pkg, "train_folds", lambda *a, **k: pytest.fail("class_alg = 'dual' does not read solver"))
    monkeypatch.setattr(pkg, "test_classification_folds", summarise)
    out = pkg.validate_folds(pool, labels, splits, "ignored", 5, 20, eps=1e-4, class_alg="dual", rng=rng, H1=2, diag_var=True, nstarts=3)
    assert out == ["t0", "t1"]
    folds, H, H0, niter, kw = seen["train"]
    assert folds == [([0, 3], [5, 1, 2]), ([6, 4], [7])] and (H, H0, niter) == (5, 3, 20)
    assert kw == dict(eps=1e-4, diag_var=True, nstarts=3, rng=rng, form="stream", slice_cols=None, pool=pool)
    assert seen["test"] == (["m0", "m1"], [[4, 6, 7], [0, 1]], pool, labels, "dual")
    pkg.validate_folds(pool, labels, splits, "ignored", 5, 20, class_alg="dual")
    assert seen["train"][2] == 4 and seen["train"][4]["nstarts"] == 10 and seen["train"][4]["diag_var"] is False      # H1 = 1


def test_vbls_sparse_jobs_fills_the_sets(pkg):
    L, Ms, H = 12, [3, 1, 4], 3
    pool = _fake_pool(pkg, L, Ms)
    calls = []
    pool.session = type("S", (), {"ctx": _RecCtx(calls)})()
    res = [_dual_set(pkg, L, H, 1, 0), _dual_set(pkg, L, H, 1, 1)]
    sets, r2, status = pkg.vbls_sparse_jobs_(pool, res, [2, 0, 2], [1, 0, 0], 9, full_cov=True)
    assert len(calls) == 1 and calls[0]["niter"] == 9 and calls[0]["full_cov"] is True and calls[0]["job_model"] == [1, 0, 0]
    assert np.array_equal(r2, [103.0 ** 2, 1.0, 9.0]) and not status.any()
    s0 = 0
    for j, (p, b, k) in enumerate(zip(sets, [2, 0, 2], [1, 0, 0])):
        n = Ms[b] * H
        assert type(p) is pkg.vbmf_dual_parameters and (p.L, p.M, p.H, p.H0) == (L, Ms[b], H, 1)
        assert np.array_equal(p.BHat, res[k].BHat) and p.BHat is not res[k].BHat and p.alpha01 == res[k].alpha01
        assert np.array_equal(p.ATVecHat, np.arange(s0, s0 + n)) and np.array_equal(p.AHat, p.ATVecHat.reshape(Ms[b], H))
        assert np.array_equal(p.CA, np.arange(s0, s0 + n) + 0.5) and (p.sigmaHat, p.zeta) == (j + 2.0, j + 3.0)
        assert np.array_equal(p.A0Hat, p.AHat[:, :1]) and np.array_equal(p.CA1, p.CA.reshape(Ms[b], H)[:, 1:].reshape(-1))
        assert (p.alpha0, p.alpha1) == (p.alpha00 + 0.5, p.alpha01 + 0.5) and np.array_equal(p.alpha, [p.alpha0, p.alpha1])
        assert np.array_equal(p.YHat, p.BHat @ p.AHat.T)
        s0 += n


# ---- 2. host refusals -------------------------------------------------------------------------------------------------------------
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
    d = [_dual_set(pkg, L, H, 2, s) for s in range(2)]
    sp = pkg.vbmf_sparse_init(np.zeros((L, 3)), H)
    basic = pkg.vbmf_init(np.zeros((L, 3)), H, rng=rng)
    tr = pkg.vbmf_trial_init(np.zeros((L, 3)), H, 1, 2, rng=rng)
    d4 = _dual_set(pkg, L, 4, 2, 5)
    d33 = _dual_set(pkg, L, 33, 2, 6)
    dL = _dual_set(pkg, L + 1, H, 2, 7)
    dn = _dual_set(pkg, L, H, 2, 8); dn.BHat[3, 1] = np.nan
    di = _dual_set(pkg, L, H, 2, 9); di.beta01 = np.inf
    fn = "classify_folds"
    for ys in (Ys, pool):
        with pytest.raises(ValueError, match=fn + ".*fold 0.*res1 is a vbmf_parameters.*'dual'"):
            pkg.classify_folds([(d[0], basic)], [[0]], ys, "dual")
        with pytest.raises(ValueError, match=fn + ".*fold 1.*vbmf_dual_parameters with H = 3.*vbmf_sparse_parameters.*one type and one H per fold"):
            pkg.classify_folds([(d[0], d[1]), (d[0], sp)], [[0], [1]], ys, "dual")
        with pytest.raises(ValueError, match=fn + ".*fold 0.*H = 3.*H = 4.*one type and one H per fold"):
            pkg.classify_folds([(d[0], d4)], [[0]], ys, "dual")
        with pytest.raises(ValueError, match=fn + ".*fold 1: res0 has H = 4 beside H = 3.*one H per call"):
            pkg.classify_folds([(d[0], d[1]), (d4, d4)], [[0], [1]], ys, "dual")
        with pytest.raises(ValueError, match=fn + ".*fold 0.*H = 33 > 32"):
            pkg.classify_folds([(d33, d33)], [[0]], ys, "dual")
        with pytest.raises(ValueError, match=fn + ".*fold 0.*two parameter sets per bag"):
            pkg.classify_folds([(tr, tr)], [[0]], ys, "dual")
        with pytest.raises(ValueError, match=fn + ".*fold 0: res0.*L = 12 rows"):
            pkg.classify_folds([(dL, dL)], [[0]], ys, "dual")
        with pytest.raises(ValueError, match=fn + ".*fold 2: res1.*not finite"):
            pkg.classify_folds([(d[0], d[1]), (0, 0), (d[0], dn)], [[0], [1], [2]], ys, "dual")
        with pytest.raises(ValueError, match=fn + ".*fold 0: res0.*not finite"):
            pkg.classify_folds([(di, d[1])], [[0]], ys, "dual")
        with pytest.raises(ValueError, match=fn + ".*outside 0"):
            pkg.classify_folds([(d[0], d[1])], [[0, 4]], ys, "dual")
        with pytest.raises(ValueError, match=fn + ".*niter = 0 < 1"):
            pkg.classify_folds([(d[0], d[1])], [[0]], ys, "dual", niter=0)
        with pytest.raises(ValueError, match=fn + ".*a pair"):
            pkg.classify_folds([(d[0], d[1], d[0])], [[0]], ys, "dual")
    with pytest.raises(ValueError, match=fn + ".*closed"):
        pkg.classify_folds([(d[0], d[1])], [[0]], closed, "dual")
    # the classifiers that stay per fold, by the reworded text
    for alg in ("vbls", "lower_bound", "min_err", "nonsense"):
        for call in (lambda: pkg.classify_folds([(d[0], d[1])], [[0]], Ys, alg),
                     lambda: pkg.test_classification_folds([(d[0], d[1])], [[0]], Ys, [0, 1, 0, 1], alg),
                     lambda: pkg.validate_folds(pool, [0, 1, 0, 1], [([0, 1], [2, 3])], "sparse", H, 5, class_alg=alg)):
            with pytest.raises(ValueError, match="class_alg = '" + alg + "'.*'ols', 'rls' or 'dual'.*per fold with classify_bags"):
                call()
    fn = "vbls_sparse_jobs_"
    for ys in (Ys, pool):
        with pytest.raises(ValueError, match=fn + ".*no models"):
            pkg.vbls_sparse_jobs_(ys, [], [0], [0], 5)
        with pytest.raises(ValueError, match=fn + ".*two parameter sets per bag"):
            pkg.vbls_sparse_jobs_(ys, [tr], [0], [0], 5)
        with pytest.raises(ValueError, match=fn + ".*two parameter sets per bag"):
            pkg.vbls_sparse_jobs_(ys, [d[0], tr], [0], [0], 5)
        with pytest.raises(ValueError, match=fn + ".*model 1 is a vbmf_parameters"):
            pkg.vbls_sparse_jobs_(ys, [d[0], basic], [0], [0], 5)
        with pytest.raises(ValueError, match=fn + ".*model 1 has H = 4 beside H = 3"):
            pkg.vbls_sparse_jobs_(ys, [d[0], d4], [0], [0], 5)
        with pytest.raises(ValueError, match=fn + ".*H = 33 > 32"):
            pkg.vbls_sparse_jobs_(ys, [d33], [0], [0], 5)
        with pytest.raises(ValueError, match=fn + ".*niter = 0 < 1"):
            pkg.vbls_sparse_jobs_(ys, [d[0]], [0], [0], 0)
        with pytest.raises(ValueError, match=fn + ".*model 0.*L = 12 rows"):
            pkg.vbls_sparse_jobs_(ys, [dL], [0], [0], 5)
        with pytest.raises(ValueError, match=fn + ".*model 1.*not finite"):
            pkg.vbls_sparse_jobs_(ys, [d[0], dn], [0], [0], 5)
        with pytest.raises(ValueError, match=fn + ".*2 job bags and 1 job models"):
            pkg.vbls_sparse_jobs_(ys, [d[0]], [0, 1], [0], 5)
        with pytest.raises(ValueError, match=fn + ".*0 job bags"):
            pkg.vbls_sparse_jobs_(ys, [d[0]], [], [], 5)
        with pytest.raises(ValueError, match=fn + ".*job 1: bag 4 outside 0..3"):
            pkg.vbls_sparse_jobs_(ys, [d[0]], [0, 4], [0, 0], 5)
        with pytest.raises(ValueError, match=fn + ".*job 0: model 1 outside 0..0"):
            pkg.vbls_sparse_jobs_(ys, [d[0]], [0], [1], 5)
    with pytest.raises(ValueError, match=fn + ".*closed"):
        pkg.vbls_sparse_jobs_(closed, [d[0]], [0], [0], 5)
    with pytest.raises(ValueError, match=fn + ".*row counts"):
        pkg.vbls_sparse_jobs_(Ys[:2] + [np.zeros((L + 1, 2))], [d[0]], [0], [0], 5)


# ---- 3. the block-wise reference is the oracle's dense form ---------------------------------------------------------------------
@pytest.mark.parametrize("kind,H", [("sparse", 5), ("dual", 5), ("dual", 17), ("sparse", 1)])
@pytest.mark.parametrize("full_cov", [False, True])
def test_block_wise_reference_is_the_oracle_s(pkg, kind, H, full_cov):
    """ref_vbls against the oracle's updateA! (the dense M_b H x M_b H inverse under full_cov), updateCA!, updateSigma! loop on
    small bags, every field: two fp64 evaluations of the same recurrence, held to 1e-10 relative"""
    L, niter = 33, 20
    po, draw = trained(kind, L, H, 3000 + H)
    m = model_arrays(po)
    worst = {f: 0.0 for f in FIELDS + ("r2",)}
    for b, w in enumerate([1, 3, 2, 7, 8, 9] if H <= 5 else [1, 3, 2, 7]):
        if w == 1 and not full_cov:
            continue                                                   # (the QS1 layout needs M >= 2)
        Y = draw(w)
        q = oracle_vbls(pkg, Y, po, niter, full_cov, seed=b)
        r = ref_vbls(Y, m, niter, full_cov)
        for f in FIELDS:
            a, o = r[f], getattr(q, f)
            worst[f] = max(worst[f], abs(a - o) / abs(o) if np.isscalar(o) else relF(a, o))
        r2 = float(np.sum((Y - po.BHat @ q.AHat.T) ** 2))
        worst["r2"] = max(worst["r2"], abs(r["r2"] - r2) / r2)
    assert all(v <= 1e-10 for v in worst.values()), worst
