"""vbls! of the basic model for a list of (bag, model) jobs in one device call (vbmf_fixed_basis_jobs, Context.fixed_basis_jobs,
vbls_jobs_, classify_folds with class_alg = "vbls"): every output field of every job against fp64 (the oracle's literal vbls! on the
oracle's copy_vbmf_params set; tests/test_vbls_basic_jobs_host.py says what stands in for it on bags of more than WIDE columns), the
independence of a job from everything else in the call bit for bit, the isolation of a failed job, the C ABI's refusals, and the fold
functions against the oracle's classifier.

Shapes: (L, H) = (33, 5), (300, 5) (one and two 256-row stages), (20, 1), (30, 16), (40, 17), (64, 32) (both edges of both 16-block
tiers), 20 and 150 iterations, bags of 1, 2, 3, 7, 8, 9, 17, 64 and 70 columns and, from the placement rule itself
(vbmf_debug_fixed_basis_jobs_lds_cols), the widest bag whose P stays in LDS at that H and one column more; two models per call.  Y is
rounded to fp32 and stored as fp32, so that Y as stored is Y; the bf16-storage case rounds to bf16 on the host and checks vbmf_get_Y.

Bounds.  Against fp64 every field is held to 3 x the error measured on an MI355X (the project's rule), worst over this file's cases;
MEASURED below carries the measured values.  Both sides are fp64 evaluations of one recurrence on the same operands, so the errors
are summation-order movement amplified by the recurrence.  None is looser than what the one-basis entry is held to
(tests/test_gpu_vbls_batch.py's TOL; tests/test_gpu_bag_scoring.py's RESID_TOL for r2), asserted below.  r2 is compared twice: with
the oracle's norm(Y - BHat*AHat')^2, and with NumPy on the device's own AHat (RESID_TOL), both relative to the reference value.
"""
import functools
import zlib

import numpy as np
import pytest

import __graft_entry__ as G
from oracle import vbmf_oracle as O
from tests.helpers import bf16_round, relF, report, to_pkg_params
from tests.test_gpu_bag_scoring import RESID_TOL
from tests.test_gpu_vbls_batch import TOL as TOL_ONE_BASIS
from tests.test_vbls_basic_jobs_host import FIELDS, SHAPES, WIDTHS, basic_models, oracle_job

pytestmark = pytest.mark.gpu

NITERS = (20, 150)
# measured on an MI355X, per field the largest relative error of any job: worst over the 13 cases of test_against_fp64 (AHat at
# (30, 16) x 20, SigmaA at (30, 16) x 20, CA and sigma2 at (30, 16) x 150; r2 there 6.87e-14 at (64, 32) x 20) and, for r2, the 44 jobs
# of test_classify_folds_vbls (bags of 1 to 39 columns at 150 iterations), which moved it most.  SigmaA = sigma2 inv(K) carries
# sigma2's error, and sigma2 = (||Y||^2 - 2 tr(S SigmaA) / sigma2 + ...) / (L M_b) cancels, as in the one-basis entry
MEASURED = dict(AHat=1.77e-14, SigmaA=5.38e-12, CA=4.17e-14, sigma2=5.16e-12, r2=3.10e-13)
TOL = {f: 3 * v for f, v in MEASURED.items()}
ONE_BASIS = dict(AHat=TOL_ONE_BASIS["default"], CA=TOL_ONE_BASIS["default"], SigmaA=TOL_ONE_BASIS["SigmaA"], sigma2=TOL_ONE_BASIS["sigma2"],
                 r2=RESID_TOL)


def test_no_bound_is_looser_than_the_one_basis_entry_s():
    assert set(TOL) == set(FIELDS)
    for f in FIELDS:
        assert TOL[f] <= ONE_BASIS[f], f


@pytest.fixture(scope="module")
def pkg():
    G.build()
    p = G.load_package()
    p.set_defaults(y_dtype=p.VBMF_Y_F32, factor_dtype=p.VBMF_FACTOR_AUTO)
    yield p
    p.invalidate()
    p.set_defaults(y_dtype=p.VBMF_Y_F32, factor_dtype=p.VBMF_FACTOR_AUTO)


def _f32(Y):
    return Y.astype(np.float32).astype(np.float64)


def model_arrays(po):
    """one model of Context.fixed_basis_jobs from a trained set: what copy_vbmf_params gives (sigma2 = the trained one, CA = I)"""
    return dict(BHat=np.array(po.BHat, dtype=np.float64), SigmaB=np.array(po.SigmaB, dtype=np.float64), sigma2_0=float(po.sigma2), ca0=1.0)


def _upload(pkg, Ys, storage="f32"):
    C = pkg.capi
    off = np.concatenate([[0], np.cumsum([Y.shape[1] for Y in Ys])]).astype(np.int64)
    c = C.Context(Ys[0].shape[0], int(off[-1]), 1, y_dtype=C.VBMF_Y_BF16 if storage == "bf16" else C.VBMF_Y_F32)
    c.set_Y(np.asfortranarray(np.hstack(Ys)))
    return c, off


def _block(r, j, f):
    return float(r[f][j]) if f in ("sigma2", "r2") else r[f][j]


def _job_equal(ra, ja, rb, jb):
    return all(np.array_equal(_block(ra, ja, f), _block(rb, jb, f)) for f in FIELDS) and ra["status"][ja] == rb["status"][jb]


def _errs(got, want):
    """per field the relative error of one job against its reference"""
    return {f: abs(got[f] - want[f]) / abs(want[f]) if np.isscalar(want[f]) else relF(got[f], want[f]) for f in FIELDS}


# ---- 1. against fp64, and the residual ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(L, H, niter, storage, lds):
    """the bags, the shuffled jobs and the oracle's result per job; computed once and left unchanged"""
    mods = basic_models(L, H)
    widths = WIDTHS + [lds, lds + 1]
    rnd = _f32 if storage == "f32" else bf16_round
    Ys = [rnd(mods[b % 2][1](w, 100 + b)) for b, w in enumerate(widths)]
    jobs = [(b, k) for b in range(len(Ys)) for k in range(2)]
    jobs = [jobs[i] for i in np.random.default_rng(77 + H).permutation(len(jobs))]
    want = [oracle_job(Ys[b], mods[k][0], niter, seed=j) for j, (b, k) in enumerate(jobs)]
    for w in want:                                                     # (the inputs keep the oracle finite for every job)
        assert all(np.all(np.isfinite(w[f])) for f in FIELDS) and w["sigma2"] > 0 and np.all(w["CA"] > 0)
    return mods, Ys, jobs, want


def _against_fp64(pkg, L, H, niter, storage):
    lds = pkg.capi.fixed_basis_jobs_lds_cols(H)
    assert lds >= 71                                                   # (the fixed widths are all on the LDS side)
    mods, Ys, jobs, want = _case(L, H, niter, storage, lds)
    arrays = [model_arrays(po) for po, _ in mods]
    c, off = _upload(pkg, Ys, storage)
    with c:
        Yst = c.get_Y()
        r = c.fixed_basis_jobs(off, arrays, [b for b, _ in jobs], [k for _, k in jobs], niter)
    assert all(np.array_equal(Yst[:, off[b]:off[b + 1]], Y) for b, Y in enumerate(Ys))      # Y as stored is Y
    assert not r["status"].any()
    worst, resid = {f: 0.0 for f in FIELDS}, 0.0
    for j, (b, k) in enumerate(jobs):
        got = {f: _block(r, j, f) for f in FIELDS}
        assert got["AHat"].shape == (Ys[b].shape[1], H) and got["SigmaA"].shape == (H, H) and got["CA"].shape == (H,)
        for f, e in _errs(got, want[j]).items():
            worst[f] = max(worst[f], e)
        r2 = float(np.sum((Ys[b] - mods[k][0].BHat @ got["AHat"].T) ** 2))
        resid = max(resid, abs(got["r2"] - r2) / r2)
    report(f"vbls_basic_jobs L{L} H{H} x{niter} {storage} {len(jobs)} jobs (lds up to {lds} columns): "
           + " ".join(f"{k}={v:.2e}" for k, v in worst.items()) + f" r2_own={resid:.2e}")
    return worst, resid


@pytest.mark.parametrize("niter", NITERS)
@pytest.mark.parametrize("L,H", SHAPES)
def test_against_fp64(pkg, L, H, niter):
    worst, resid = _against_fp64(pkg, L, H, niter, "f32")
    bad = {k: v for k, v in worst.items() if not v <= TOL[k]}
    assert not bad, bad
    assert resid <= RESID_TOL, resid


def test_against_fp64_bf16_storage(pkg):
    worst, resid = _against_fp64(pkg, 33, 5, 20, "bf16")
    bad = {k: v for k, v in worst.items() if not v <= TOL[k]}
    assert not bad, bad
    assert resid <= RESID_TOL, resid


# ---- 2. independence, bitwise ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mixed_case(lds16, lds17, lds32):
    """models of H = 5, 16, 17 and 32 on one L; bags on both sides of the placement rule at H = 16, 17 and 32"""
    L = 40
    mods = [basic_models(L, H)[0] for H in (5, 16, 17, 32)]
    widths = [1, 3, 8, 9, 70, lds32, lds32 + 1, lds17, lds17 + 1, lds16, lds16 + 1]
    Ys = [_f32(mods[b % 4][1](w, 200 + b)) for b, w in enumerate(widths)]
    return L, [model_arrays(po) for po, _ in mods], Ys


def test_jobs_are_independent_bitwise(pkg):
    niter = 20
    lds = {H: pkg.capi.fixed_basis_jobs_lds_cols(H) for H in (5, 16, 17, 32)}
    L, arrays, Ys = _mixed_case(lds[16], lds[17], lds[32])
    nb = len(Ys)
    jobs = [(b, k) for b in range(nb) for k in range(4)]
    jobs += [jobs[4], jobs[17], jobs[4]]                               # repeated jobs
    rng = np.random.default_rng(5)
    jobs = [jobs[i] for i in rng.permutation(len(jobs))]
    c, off = _upload(pkg, Ys)
    with c:
        run = lambda js, ms=arrays: c.fixed_basis_jobs(off, ms, [b for b, _ in js], [k for _, k in js], niter)
        base = run(jobs)
        assert not base["status"].any()
        # both tiers and both placements are in the call
        Hs = [a["BHat"].shape[1] for a in arrays]
        assert {(Hs[k] > 16, Ys[b].shape[1] > lds[Hs[k]]) for b, k in jobs} == {(False, False), (False, True), (True, False), (True, True)}
        # a repeated job gives identical blocks
        first = {}
        for j, job in enumerate(jobs):
            if job in first:
                assert _job_equal(base, j, base, first[job]), job
            first.setdefault(job, j)
        # each job alone in its own call, with only its own model
        for j, (b, k) in enumerate(jobs):
            one = run([(b, 0)], [arrays[k]])
            assert _job_equal(one, 0, base, j), (j, b, k)
        # another order of the jobs
        perm = rng.permutation(len(jobs))
        pr = run([jobs[i] for i in perm])
        assert all(_job_equal(pr, j, base, int(i)) for j, i in enumerate(perm))
        # one output at a time: the other pointers NULL
        C = pkg.capi
        dp, ip = C.C.POINTER(C.C.c_double), C.C.POINTER(C.C.c_int64)
        pk = lambda key, order="C": np.concatenate([np.asarray(m[key], dtype=np.float64).reshape(-1, order=order) for m in arrays])
        P = lambda v, t=dp: None if v is None else v.ctypes.data_as(t)
        ins = [pk("BHat", "F"), pk("SigmaB", "F"), pk("sigma2_0"), pk("ca0")]
        mh = np.array(Hs, dtype=np.int64)
        jb, jk = np.array([b for b, _ in jobs], dtype=np.int64), np.array([k for _, k in jobs], dtype=np.int64)
        r2, st = np.empty(len(jobs)), np.empty(len(jobs), dtype=np.int64)
        rc = C.lib().vbmf_fixed_basis_jobs(c._h, nb, P(off, ip), niter, 4, P(mh, ip), *[P(v) for v in ins], len(jobs), P(jb, ip), P(jk, ip),
                                           P(r2), None, None, None, None, P(st, ip))
        assert rc == C.VBMF_OK and np.array_equal(r2, base["r2"]) and not st.any()
    # a second upload that holds the bags in another order
    order = [int(i) for i in np.random.default_rng(6).permutation(nb)]
    c2, off2 = _upload(pkg, [Ys[i] for i in order])
    with c2:
        r2nd = c2.fixed_basis_jobs(off2, arrays, [order.index(b) for b, _ in jobs], [k for _, k in jobs], niter)
    assert all(_job_equal(r2nd, j, base, j) for j in range(len(jobs)))
    # the same bags through a BagPool's context
    with pkg.BagPool(Ys) as pool:
        pr = pool.ctx.fixed_basis_jobs(pool.col_off, arrays, [b for b, _ in jobs], [k for _, k in jobs], niter)
    assert all(_job_equal(pr, j, base, j) for j in range(len(jobs)))


# ---- 3. isolation ------------------------------------------------------------------------------------------------------------------
def test_a_failed_job_leaves_the_other_jobs_alone(pkg):
    """A model that starts from sigma2_0 = 0.0: SigmaA = 0 inv(K) = 0 and A = P 0 / 0"""
    L, niter = 40, 20
    mods = [basic_models(L, H)[0] for H in (5, 17)]
    arrays = [model_arrays(mods[0][0]), dict(model_arrays(mods[1][0]), sigma2_0=0.0), model_arrays(mods[1][0])]
    lds17 = pkg.capi.fixed_basis_jobs_lds_cols(17)
    Ys = [_f32(mods[b % 2][1](w, 300 + b)) for b, w in enumerate([3, 2, 9, 17, 70, lds17 + 1])]
    jobs = [(b, k) for b in range(len(Ys)) for k in range(3)]
    keep = [0, 2]
    c, off = _upload(pkg, Ys)
    with c:
        r = c.fixed_basis_jobs(off, arrays, [b for b, _ in jobs], [k for _, k in jobs], niter)           # returns: success
        jobs2 = [(b, keep.index(k)) for b, k in jobs if k != 1]
        r2 = c.fixed_basis_jobs(off, [arrays[k] for k in keep], [b for b, _ in jobs2], [k for _, k in jobs2], niter)
    assert np.array_equal(r["status"], [int(k == 1) for _, k in jobs]) and not r2["status"].any()
    good = [j for j, (_, k) in enumerate(jobs) if k != 1]
    for j, (b, k) in enumerate(jobs):
        if k == 1:
            assert all(np.all(np.isnan(_block(r, j, f))) for f in FIELDS), j
            assert r["AHat"][j].shape == (Ys[b].shape[1], 17) and r["SigmaA"][j].shape == (17, 17) and r["CA"][j].shape == (17,)
    for j2, j in enumerate(good):
        assert _job_equal(r, j, r2, j2), (j, jobs[j])
        assert all(np.all(np.isfinite(_block(r, j, f))) for f in FIELDS)


# ---- 4. C ABI refusals -------------------------------------------------------------------------------------------------------------
def _state_crc(c):
    s = c.get_state()
    return zlib.crc32(b"".join(np.ascontiguousarray(s[k]).tobytes() for k in ("AHat", "BHat", "SigmaA", "SigmaB", "CA_diag", "CB_diag"))
                      + np.float64(s["sigma2"]).tobytes())


def test_refusals_change_nothing(pkg):
    C = pkg.capi
    VI, VU = C.VBMF_ERR_INVALID, C.VBMF_ERR_UNSUPPORTED
    L = 40
    mods = [basic_models(L, 5)[0], basic_models(L, 17)[0]]
    arrays = [model_arrays(po) for po, _ in mods]
    Ys = [_f32(mods[b % 2][1](w, 400 + b)) for b, w in enumerate([3, 1, 2, 7, 8, 9, 17, 4])]
    ip, dp = C.C.POINTER(C.C.c_int64), C.C.POINTER(C.C.c_double)
    i64 = lambda v: np.array(v, dtype=np.int64)
    pk = lambda key, order="C": np.concatenate([np.asarray(m[key], dtype=np.float64).reshape(-1, order=order) for m in arrays])
    SENT = -7.0
    c, off = _upload(pkg, Ys)
    nb, M = len(Ys), int(off[-1])
    good = dict(o=off, niter=20, mh=i64([5, 17]), B=pk("BHat", "F"), SB=pk("SigmaB", "F"), s0=pk("sigma2_0"), c0=pk("ca0"),
                jb=i64([0, 3, 7, 3]), jk=i64([1, 0, 1, 1]))
    outs = dict(r2=np.full(8, SENT), A=np.full(32 * M * 2, SENT), SA=np.full(8 * 32 * 32, SENT), CA=np.full(8 * 32, SENT), sg=np.full(8, SENT))
    sbuf = np.full(8, -7, dtype=np.int64)

    def raw(ctx, nk=2, nj=None, s=sbuf, null=(), **kw):
        a = {**good, **kw}
        p = lambda v, t: None if v is None else v.ctypes.data_as(t)
        o = {k: (None if k in null else v) for k, v in outs.items()}
        nj = (4 if a["jb"] is None else len(a["jb"])) if nj is None else nj
        return C.lib().vbmf_fixed_basis_jobs(ctx._h, len(a["o"]) - 1, p(a["o"], ip), a["niter"], nk, p(a["mh"], ip), p(a["B"], dp), p(a["SB"], dp),
                                             p(a["s0"], dp), p(a["c0"], dp), nj, p(a["jb"], ip), p(a["jk"], ip), p(o["r2"], dp), p(o["A"], dp),
                                             p(o["SA"], dp), p(o["CA"], dp), p(o["sg"], dp), p(s, ip))

    def untouched():
        return all(np.all(v == SENT) for v in outs.values()) and np.all(sbuf == -7)

    def spoiled(key, i, v):
        x = good[key].copy(); x[i] = v
        return {key: x}

    refused = [(VU, dict(mh=i64([0, 17]))), (VU, dict(mh=i64([5, 33]))), (VU, dict(mh=i64([-1, 17]))),
               (VI, dict(nk=0)), (VI, dict(nj=0)), (VI, dict(nk=-1)), (VI, dict(nj=-3)), (VI, dict(niter=0)), (VI, dict(niter=-2)),
               (VI, dict(s=None)), (VI, dict(null=("r2", "A")))]
    refused += [(VU, dict(nj=1 << 24)), (VU, dict(nk=1 << 24))]          # more workgroups than one grid holds: refused before any table is read
    refused += [(VI, {k: None}) for k in ("mh", "B", "SB", "s0", "c0", "jb", "jk")]
    refused += [(VI, spoiled(k, i, v)) for k, i in (("B", -1), ("B", 7), ("SB", 3), ("SB", -1), ("s0", 0), ("s0", 1), ("c0", 1))
                for v in (np.nan, np.inf, -np.inf)]
    refused += [(VI, dict(jb=i64([0, 3, nb, 3]))), (VI, dict(jb=i64([-1, 3, 7, 3]))), (VI, dict(jk=i64([1, 0, 2, 1]))), (VI, dict(jk=i64([1, -1, 1, 1])))]
    refused += [(VI, dict(o=i64(b))) for b in ([0, 1, 1, M], [1, 17, M], [0, 17, M - 1], [0, 20, 10, M], [0, M + 1])]
    with c:
        z = np.zeros
        c.set_state(np.ones((M, 1)), np.ones((L, 1)), z((1, 1)), z((1, 1)), np.ones(1), np.ones(1), 0.5)
        Y0, dims0, crc0 = c.get_Y(), c.dims(), _state_crc(c)
        ref = c.fixed_basis_jobs(off, arrays, good["jb"], good["jk"], 20)
        assert _state_crc(c) == crc0
        for code, kw in refused:
            if "o" in kw:                                             # (the jobs name bags of the shorter col_off)
                kw = dict(kw, jb=i64([0, 0, 0, 0]))
            assert raw(c, **kw) == code, kw
            assert untouched(), kw
        assert raw(c, **spoiled("B", 7, np.nan)) == VI and "not finite" in c._lib.vbmf_last_error(c._h).decode()
        assert np.array_equal(c.get_Y(), Y0) and c.dims() == dims0 and _state_crc(c) == crc0
        # after the refusals a good call returns the former bits, and writes only its own jobs
        assert raw(c) == C.VBMF_OK and np.array_equal(sbuf[:4], [0, 0, 0, 0]) and np.all(sbuf[4:] == -7)
        flat = lambda key, order="C": np.concatenate([np.asarray(v).reshape(-1, order=order) for v in ref[key]])
        for key, want in (("r2", ref["r2"]), ("sg", ref["sigma2"]), ("A", flat("AHat", "F")), ("SA", flat("SigmaA")), ("CA", flat("CA"))):
            assert np.array_equal(outs[key][:want.size], want) and np.all(outs[key][want.size:] == SENT), key
        assert np.array_equal(c.get_Y(), Y0) and c.dims() == dims0 and _state_crc(c) == crc0
        # a label mask on the context
        c.set_state(z((M, 1)), np.ones((L, 1)), z((1, 1)), z((1, 1)), np.ones(1), np.ones(1), 1.0, labels0=[0], H1=1)
        for v in outs.values():
            v[:] = SENT
        sbuf[:] = -7
        assert raw(c) == VI and "label mask" in c._lib.vbmf_last_error(c._h).decode() and untouched()
    with C.Context(L, M, 5, y_dtype=pkg.VBMF_Y_F32) as c2:             # no Y
        assert raw(c2) == VI and "no Y" in c2._lib.vbmf_last_error(c2._h).decode() and untouched()
    with C.Context(L, M, 5, y_dtype=pkg.VBMF_Y_F32, nranks=2, rank=0, L_global=2 * L, variant=C.VBMF_VARIANT_SPARSE_DIAG) as c2:
        assert raw(c2) == VI and "rank" in c2._lib.vbmf_last_error(c2._h).decode() and untouched()


# ---- 5. the fold functions ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fold_case():
    """24 bags of two classes, four folds -- untrained, no test bags, two models of different H, two of one H -- and the oracle's
    classifier per tested bag (examples/mil_util.jl:469-491); computed once and left unchanged"""
    L, niter = 33, 150
    (a5, draw_a), (b5, draw_b) = basic_models(L, 5)
    Ytr = draw_b(400, 13)                                              # class 1 again, fitted with two columns more than it has
    b7 = O.vbmf_init(Ytr, 7, ca=0.1, cb=0.1, sigma2=0.1, rng=np.random.default_rng(12), materialize_yhat=False)
    O.vbmf_(Ytr, b7, 15, eps=0.0, est_covs=True, est_var=True)
    rng = np.random.default_rng(11)
    labels = np.array([b % 2 for b in range(24)])
    Ys = [_f32((draw_b if lab else draw_a)(int(w), 500 + b)) for b, (lab, w) in enumerate(zip(labels, rng.integers(1, 40, 24)))]
    pairs = [(0, 0), (a5, b5), (a5, b7), (a5, b5)]
    tests = [[0, 1, 2], [], [3, 4, 5, 6, 7, 8, 9, 10, 11, 12], [13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 3]]
    want = []
    for pair, ids in zip(pairs, tests):
        if pair == (0, 0) or not ids:
            want.append(None)
            continue
        errs = []
        for k, po in enumerate(pair):
            errs.append(np.array([np.sqrt(oracle_job(Ys[b], po, niter, seed=b)["r2"]) for b in ids]))
        want.append(((errs[0] > errs[1]).astype(np.int64), errs[0], errs[1]))
    # the conditions on the inputs, from the oracle's numbers: both labels occur, and no bag's decision is within reach of the tolerance
    for w in want:
        if w is None:
            continue
        est, e0, e1 = w
        assert set(est) == {0, 1}
        assert np.all(np.abs(e0 - e1) > 100 * TOL["r2"] * np.maximum(e0, e1))
    return L, niter, Ys, labels, pairs, tests, want


def test_classify_folds_vbls(pkg):
    L, niter, Ys, labels, pairs, tests, want = _fold_case()
    models = [p if p == (0, 0) else tuple(to_pkg_params(pkg, r) for r in p) for p in pairs]
    with pkg.BagPool(Ys) as pool:
        got = pkg.classify_folds(models, tests, pool, "vbls")                                  # niter: the default, 150
        counts = pkg.test_classification_folds(models, tests, pool, labels, "vbls")
        splits = [([b for b in range(24) if b not in t], t) for t in (tests[2], tests[3], [0, 1, 2, 5])]
        val = pkg.validate_folds(pool, labels, splits, "basic", 5, 30, eps=1e-3, class_alg="vbls")
    lst = pkg.classify_folds(models, tests, Ys, "vbls", niter=niter)
    assert got[0] is None and lst[0] is None
    assert all(a.size == 0 for a in got[1]) and len(got[1]) == 3 and got[1][0].dtype == np.int64
    worst = 0.0
    for f in (2, 3):
        est, e0, e1 = got[f]
        assert np.array_equal(est, want[f][0]), f
        for e, w in ((e0, want[f][1]), (e1, want[f][2])):               # as r2's relative error: err = sqrt(r2)
            worst = max(worst, float(np.max(np.abs(e * e - w * w) / (w * w))))
        assert all(np.array_equal(a, b) for a, b in zip(got[f], lst[f])), f                     # the pool and the list: the same bits
    report(f"classify_folds vbls 4 folds: r2={worst:.2e}")
    assert worst <= TOL["r2"], worst
    assert counts[0] == (-1.0,) * 6
    for f in (1, 2, 3):
        ids = np.asarray(tests[f], dtype=np.int64)
        cnt = pkg._classification_counts("t", labels[ids], np.asarray(got[f][0]).reshape(-1))
        assert np.array_equal(np.array(counts[f], dtype=float), np.array(cnt, dtype=float), equal_nan=True), f      # (no test bags: nan rates)
    assert len(val) == 3 and all(len(v) == 6 and all(np.isfinite(x) for x in v) for v in val)


def test_vbls_jobs_fills_the_sets(pkg):
    """vbls_jobs_ on a pool and on a list of matrices: every job's set carries the call's blocks, and agrees with the oracle"""
    L, niter = 33, 20
    mods = [basic_models(L, 5)[0], basic_models(L, 7)[1]]
    res = [to_pkg_params(pkg, po) for po, _ in mods]
    Ys = [_f32(mods[b % 2][1](w, 600 + b)) for b, w in enumerate([3, 1, 8, 17])]
    jb, jk = [3, 0, 1, 2, 3], [1, 0, 1, 0, 0]
    with pkg.BagPool(Ys) as pool:
        sets, r2, status = pkg.vbls_jobs_(pool, res, jb, jk, niter)
        raw = pool.ctx.fixed_basis_jobs(pool.col_off, [model_arrays(r) for r in res], jb, jk, niter)
    sets2, r22, _ = pkg.vbls_jobs_(Ys, res, jb, jk, niter)
    assert not status.any() and np.array_equal(r2, raw["r2"]) and np.array_equal(r2, r22)
    for j, (p, b, k) in enumerate(zip(sets, jb, jk)):
        H = int(res[k].H)
        assert type(p) is pkg.vbmf_parameters and (p.L, p.M, p.H) == (L, Ys[b].shape[1], H)
        assert np.array_equal(p.AHat, raw["AHat"][j]) and np.array_equal(p.SigmaA, raw["SigmaA"][j]) and p.sigma2 == raw["sigma2"][j]
        assert np.array_equal(p.CA, np.diag(raw["CA"][j])) and np.array_equal(p.invCA, np.diag(1.0 / raw["CA"][j]))
        assert all(np.array_equal(getattr(p, f), getattr(res[k], f)) for f in ("BHat", "SigmaB", "CB", "invCB"))
        assert all(np.array_equal(getattr(p, f), getattr(sets2[j], f)) for f in ("AHat", "SigmaA", "CA", "invCA", "BHat", "SigmaB", "CB"))
        assert p.sigma2 == sets2[j].sigma2
        w = oracle_job(Ys[b], mods[k][0], niter, seed=j)
        got = dict(AHat=p.AHat, SigmaA=p.SigmaA, CA=np.diag(p.CA), sigma2=p.sigma2, r2=float(r2[j]))
        bad = {f: e for f, e in _errs(got, w).items() if not e <= TOL[f]}
        assert not bad, (j, bad)
