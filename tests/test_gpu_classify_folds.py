"""Every fold's test bags against its own models in one device call (vbmf_bag_least_squares_jobs; classify_folds,
test_classification_folds, validate_folds): a job is bit for bit what vbmf_bag_least_squares returns for that bag with that basis and
lambda -- whatever else is in the call -- and both reproduce the CRC-32s the parent commit's build gave
(tests/golden/bag_ls_jobs_crc.json, written by tests/golden/make_bag_ls_jobs_crc.py before csrc/score_kernels.hpp was touched).

Inputs (tests/golden/make_bag_ls_jobs_crc.py cases()): _two_bases(H, 7100 + H, rows) of tests/test_gpu_classify_ls.py, eight bags per
rank of widths (1, 8, 9, 70, 3, 16, 17, 2) drawn alternately from the two bases with one-hot A and noise 0.05, rounded to fp32; a
context holds the bags of all its ranks side by side.  The tests assert cond(B'B + lam I) <= 1e3, a relative label margin >= 0.5
between a bag's own two bases and max ||Y||^2 / r2 > 100 from their own NumPy evaluation.

Bounds.  Bitwise tests have none.  Against fp64 NumPy, estimate and residual are two fp64 evaluations of the same expression on the
same operands and are held to RESID_TOL = 1e-10, the project's bound for fp64 on stored operands (tests/test_gpu_classify_ls.py).

Measured on an MI355X, worst over the jobs of test_jobs_against_fp64 (these figures set no bound):
  X against NumPy   L = 300: 1.2e-15, L = 33: 2.6e-15        norms against NumPy   L = 300: 6.7e-16, L = 33: 3.3e-15
  label margin 0.95 (L = 300), 0.96 (L = 33), 0.945 (L = 166); best ||Y||^2 / r2 1775, 5062, 5029
"""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest

import __graft_entry__ as G
from tests.helpers import relF, report
from tests.test_gpu_classify_ls import RESID_TOL, _ls, _model_with, _split, _two_bases

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_bag_ls_jobs_crc", os.path.join(G.ROOT, "tests", "golden", "make_bag_ls_jobs_crc.py"))
GOLD = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(GOLD)


@pytest.fixture(scope="module")
def pkg():
    G.build()
    p = G.load_package()
    p.set_defaults(y_dtype=p.VBMF_Y_F32, factor_dtype=p.VBMF_FACTOR_AUTO)
    yield p
    p.invalidate()
    p.set_defaults(y_dtype=p.VBMF_Y_F32, factor_dtype=p.VBMF_FACTOR_AUTO)


@functools.lru_cache(maxsize=None)
def _cases():
    """computed once and left unchanged"""
    return GOLD.cases(_two_bases)


@functools.lru_cache(maxsize=None)
def _gold():
    with open(GOLD.GOLDEN) as f:
        return json.load(f)["crc"]


def _well_posed(case, Ysts, lams):
    """what the inputs must be for a tolerance to mean something, from fp64 NumPy on the operands as stored"""
    ratio, margin = 0.0, np.inf
    for H, Bs in case["bases"].items():
        own = [b for b, (h, _) in enumerate(case["drawn"]) if h == H]
        for lam in lams:
            errs = []
            for B in Bs:
                _, r, cond = _ls(B, lam, [Ysts[b] for b in own])
                assert cond <= 1e3, (H, lam, cond)
                errs.append(r)
                ratio = max(ratio, max(float(np.sum(Ysts[b] ** 2)) / e ** 2 for b, e in zip(own, r)))
            assert np.array_equal((errs[0] > errs[1]).astype(int), [case["drawn"][b][1] for b in own]), (H, lam)
            margin = min(margin, float(np.min(np.abs(errs[0] - errs[1]) / np.maximum(errs[0], errs[1]))))
    assert margin >= 0.5 and ratio > 100, (margin, ratio)
    return margin, ratio


# ---- 1. a job equals the old entry, bitwise ------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_a_job_is_the_old_entry_bitwise(pkg, storage):
    case = _cases()[storage, 166]
    Ys, Bk = case["Ys"], case["bases"]
    # two bases each of H = 1, 5 and 64 (a slice's outputs within / beyond one per thread), lambdas mixed; the seventh is in no job
    bases = [(Bk[1][0], 0.0), (Bk[1][1], 1e-2), (Bk[5][0], 1e-2), (Bk[5][1], 0.0), (Bk[64][0], 5.0), (Bk[64][1], 0.0), (Bk[5][0], 5.0)]
    nbag = len(Ys)
    jobs = []
    for b, (H, _) in enumerate(case["drawn"]):
        g = (1, 5, 64).index(H)
        jobs += [(b, 2 * g), (b, 2 * g + 1), (b, 2 * ((g + 1 + b % 2) % 3) + b % 2)]     # its own rank's two and one of another rank
    jobs.append(jobs[10])                                                               # one job twice
    rng = np.random.default_rng(41)
    jobs = [jobs[i] for i in rng.permutation(len(jobs))]
    assert all(sum(1 for b, _ in jobs if b == q) >= 3 for q in range(nbag)) and all(k != 6 for _, k in jobs)
    c, off = GOLD.upload(pkg, storage, Ys)
    with c:
        _well_posed(case, _split(c.get_Y(), np.diff(off)), (0.0, 1e-2))
        old = [c.bag_least_squares(off, B, lam) for B, lam in bases]

        def run(js):
            Xs, r2, status = c.bag_least_squares_jobs(off, [B for B, _ in bases], [lam for _, lam in bases], [b for b, _ in js],
                                                      [k for _, k in js], want_X=True)
            assert np.array_equal(status, np.zeros(7, dtype=np.int64))
            return Xs, r2

        def check(js, Xs, r2):
            for j, (b, k) in enumerate(js):
                assert Xs[j].shape == (bases[k][0].shape[1], Ys[b].shape[1])
                assert np.array_equal(Xs[j], old[k][0][:, off[b]:off[b + 1]]), (j, b, k)
                assert r2[j] == old[k][1][b], (j, b, k)

        check(jobs, *run(jobs))
        check(jobs[::-1], *run(jobs[::-1]))                           # wherever the job sits
        check(jobs[5:6], *run(jobs[5:6]))                             # whatever else is in the call
        # one output at a time gives the same bits
        r2_only = c.bag_least_squares_jobs(off, [B for B, _ in bases], [lam for _, lam in bases], [b for b, _ in jobs], [k for _, k in jobs])
        assert r2_only[0] is None and np.array_equal(r2_only[1], run(jobs)[1])
        X_only = c.bag_least_squares_jobs(off, [B for B, _ in bases], [lam for _, lam in bases], [b for b, _ in jobs], [k for _, k in jobs],
                                          want_X=True, want_r2=False)
        assert X_only[1] is None and all(np.array_equal(a, b) for a, b in zip(X_only[0], run(jobs)[0]))
    for b in (0, 3, 7):                                               # wherever the bag sits: a context that holds it alone
        c1, off1 = GOLD.upload(pkg, storage, [Ys[b]])
        with c1:
            for k in sorted({k for q, k in jobs if q == b}):
                X1, r1 = c1.bag_least_squares(off1, *bases[k])
                assert np.array_equal(X1, old[k][0][:, off[b]:off[b + 1]]) and r1[0] == old[k][1][b], (b, k)
                Xj, rj, _ = c1.bag_least_squares_jobs(off1, [bases[k][0]], [bases[k][1]], [0], [0], want_X=True)
                assert np.array_equal(Xj[0], X1) and rj[0] == r1[0], (b, k)


# ---- 2. against fp64 NumPy: two row chunks with a short second one, and one row past a tile ----------------------------------------
@pytest.mark.parametrize("L", [300, 33])
def test_jobs_against_fp64(pkg, L):
    case = _cases()["f32", L]
    Ys = case["Ys"]
    bases = [(B, lam) for H in (5, 20) for B in case["bases"][H] for lam in (0.0, 1e-2)]
    jobs = [(b, k) for b in range(len(Ys)) for k in range(len(bases))]
    c, off = GOLD.upload(pkg, "f32", Ys)
    with c:
        Ysts = _split(c.get_Y(), np.diff(off))
        Xs, r2, status = c.bag_least_squares_jobs(off, [B for B, _ in bases], [lam for _, lam in bases], [b for b, _ in jobs],
                                                  [k for _, k in jobs], want_X=True)
    assert all(np.array_equal(a, b) for a, b in zip(Ysts, Ys))
    margin, ratio = _well_posed(case, Ysts, (0.0, 1e-2))
    assert not status.any()
    ex = er = 0.0
    for k, (B, lam) in enumerate(bases):
        Xw, rw, _ = _ls(B, lam, Ysts)
        for b in range(len(Ys)):
            j = b * len(bases) + k
            ex = max(ex, relF(Xs[j], Xw[b]))
            er = max(er, abs(np.sqrt(r2[j]) - rw[b]) / rw[b])
    report(f"ls_jobs L{L} f32 H5+H20 {len(jobs)} jobs: r={er:.2e} X={ex:.2e} margin={margin:.2e} max_YY_over_r2={ratio:.0f}")
    assert ex <= RESID_TOL and er <= RESID_TOL, (ex, er)


# ---- 3. a bad basis does not take the call down --------------------------------------------------------------------------------
def test_a_bad_basis_leaves_the_other_jobs_alone(pkg):
    case = _cases()["f32", 166]
    Ys, (B0, B1) = case["Ys"], case["bases"][5]
    Bz = B0.copy(); Bz[:, 2] = 0.0                                    # not positive definite at lambda = 0: the case rls exists for
    B64 = case["bases"][64][0]
    bases = [(B0, 0.0), (Bz, 0.0), (B64, 1e-2), (Bz, 1e-2), (B1, 0.0)]
    bags = [3, 8, 11, 0, 19, 3]
    jobs = [(b, k) for b in bags for k in range(5)]
    keep = [0, 2, 3, 4]
    c, off = GOLD.upload(pkg, "f32", Ys)
    with c:
        Xs, r2, status = c.bag_least_squares_jobs(off, [B for B, _ in bases], [lam for _, lam in bases], [b for b, _ in jobs],
                                                  [k for _, k in jobs], want_X=True)         # returns: the call is OK
        jobs2 = [(b, keep.index(k)) for b, k in jobs if k != 1]
        Xs2, r22, status2 = c.bag_least_squares_jobs(off, [bases[k][0] for k in keep], [bases[k][1] for k in keep], [b for b, _ in jobs2],
                                                     [k for _, k in jobs2], want_X=True)
    assert np.array_equal(status, [0, 1, 0, 0, 0]) and not status2.any()
    good = [j for j, (_, k) in enumerate(jobs) if k != 1]
    for j, (b, k) in enumerate(jobs):
        if k == 1:
            assert np.isnan(r2[j]) and Xs[j].shape == (5, Ys[b].shape[1]) and np.all(np.isnan(Xs[j])), j
    assert len(good) == len(jobs2)
    for j2, j in enumerate(good):
        assert np.array_equal(Xs[j], Xs2[j2]) and r2[j] == r22[j2], (j, jobs[j])
        assert np.all(np.isfinite(Xs[j])) and np.isfinite(r2[j])
    assert all(np.all(Xs[j][2] == 0.0) for j, (_, k) in enumerate(jobs) if k == 3)       # the zero column at lambda = 1e-2


# ---- 4. C ABI refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(pkg):
    C = pkg.capi
    VI, VU = C.VBMF_ERR_INVALID, C.VBMF_ERR_UNSUPPORTED
    case = _cases()["f32", 33]
    L, Ys = 33, case["Ys"][:8]
    Ba, Bb = case["bases"][5][0], case["bases"][20][1]
    ip, dp = C.C.POINTER(C.C.c_int64), C.C.POINTER(C.C.c_double)
    i64 = lambda v: np.array(v, dtype=np.int64)
    pack = lambda Bs: np.concatenate([np.asarray(B).reshape(-1, order="F") for B in Bs])
    SENT = -7.0
    c, off = GOLD.upload(pkg, "f32", Ys)
    nb, M = len(Ys), int(off[-1])
    good = dict(o=off, hs=i64([5, 20]), B=pack([Ba, Bb]), lam=np.array([0.0, 1e-2]), jb=i64([0, 3, 7, 3]), jk=i64([1, 0, 1, 1]))
    Xbuf, rbuf, sbuf = np.full(25 * M, SENT), np.full(8, SENT), np.full(4, -7, dtype=np.int64)

    def raw(ctx, nk=None, nj=None, X=Xbuf, r=rbuf, s=sbuf, **kw):
        a = {**good, **kw}
        p = lambda v, t: None if v is None else v.ctypes.data_as(t)
        nk = (2 if a["hs"] is None else len(a["hs"])) if nk is None else nk
        nj = (4 if a["jb"] is None else len(a["jb"])) if nj is None else nj
        return C.lib().vbmf_bag_least_squares_jobs(ctx._h, len(a["o"]) - 1, p(a["o"], ip), nk, p(a["hs"], ip),
                                                   p(a["B"], dp), p(a["lam"], dp), nj, p(a["jb"], ip),
                                                   p(a["jk"], ip), p(X, dp), p(r, dp), p(s, ip))

    def untouched():
        return np.all(Xbuf == SENT) and np.all(rbuf == SENT) and np.all(sbuf == -7)

    Bn = pack([Ba, Bb]); Bn[-1] = np.nan
    Bi = pack([Ba, Bb]); Bi[7] = np.inf
    refused = [(VU, dict(hs=i64([0, 20]))), (VU, dict(hs=i64([5, 65]), B=np.zeros(33 * 70))),
               (VI, dict(nk=0)), (VI, dict(nj=0)), (VI, dict(nk=-1)), (VI, dict(nj=-3)),
               (VI, dict(hs=None)), (VI, dict(B=None)), (VI, dict(lam=None)), (VI, dict(jb=None)), (VI, dict(jk=None)), (VI, dict(s=None)),
               (VI, dict(X=None, r=None)),
               (VI, dict(lam=np.array([0.0, -1e-3]))), (VI, dict(lam=np.array([np.nan, 0.0]))), (VI, dict(lam=np.array([0.0, np.inf]))),
               (VI, dict(B=Bn)), (VI, dict(B=Bi)),
               (VI, dict(jb=i64([0, 3, nb, 3]))), (VI, dict(jb=i64([-1, 3, 7, 3]))), (VI, dict(jk=i64([1, 0, 2, 1]))), (VI, dict(jk=i64([1, -1, 1, 1])))]
    refused += [(VI, dict(o=i64(bad))) for bad in ([0, 1, 1, M], [1, 17, M], [0, 17, M - 1], [0, 20, 10, M], [0, M + 1])]
    with c:
        Y0, dims0 = c.get_Y(), c.dims()
        X0, r0 = c.bag_least_squares(off, Bb, 1e-2)
        for code, kw in refused:
            if "o" in kw:                                             # (the jobs name bags of the shorter col_off)
                kw = dict(kw, jb=i64([0, 0, 0, 0]))
            assert raw(c, **kw) == code, kw
            assert untouched(), kw
        assert raw(c, B=Bn) == VI and "not finite" in c._lib.vbmf_last_error(c._h).decode()
        assert np.array_equal(c.get_Y(), Y0) and c.dims() == dims0
        # the scratch is shared and regrown: after a refused call and after a good one the old entry returns its former bits
        X1, r1 = c.bag_least_squares(off, Bb, 1e-2)
        assert np.array_equal(X1, X0) and np.array_equal(r1, r0)
        assert raw(c) == C.VBMF_OK and np.array_equal(sbuf[:2], [0, 0]) and np.all(sbuf[2:] == -7)
        assert rbuf[0] == r0[0] and rbuf[1] != SENT and np.all(rbuf[4:] == SENT)
        assert np.array_equal(Xbuf[:20 * Ys[0].shape[1]].reshape((20, -1), order="F"), X0[:, off[0]:off[1]])
        X1, r1 = c.bag_least_squares(off, Bb, 1e-2)
        assert np.array_equal(X1, X0) and np.array_equal(r1, r0)
        assert np.array_equal(c.get_Y(), Y0) and c.dims() == dims0
    Xbuf[:], rbuf[:], sbuf[:] = SENT, SENT, -7
    # more job slices than one grid holds (2^32 - 1 threads = 2^24 - 1 workgroups of 256): jobs may repeat a bag, so one bag of 2^15
    # columns = 2^12 slices and 2^12 jobs on it are one slice too many.  Refused before any reserve, copy or launch.
    Mw, njw = 1 << 15, 1 << 12
    Yw = np.asfortranarray(np.random.default_rng(9).standard_normal((L, Mw)).astype(np.float32).astype(np.float64))
    wide = dict(o=i64([0, Mw]), hs=i64([5]), B=pack([Ba]), lam=np.array([0.0]), jb=np.zeros(njw, dtype=np.int64), jk=np.zeros(njw, dtype=np.int64))
    with C.Context(L, Mw, 1, y_dtype=pkg.VBMF_Y_F32) as cw:
        cw.set_Y(Yw)
        Yw0, dimsw = cw.get_Y(), cw.dims()
        assert raw(cw, **wide) == VU and "job slices" in cw._lib.vbmf_last_error(cw._h).decode() and untouched()
        assert raw(cw, X=None, **wide) == VU and untouched()
        assert np.array_equal(cw.get_Y(), Yw0) and cw.dims() == dimsw
        Xw, rw = cw.bag_least_squares(i64([0, 5, Mw]), Ba, 0.0, want_X=False)       # the context still serves
        assert Xw is None and np.all(np.isfinite(rw))
    with C.Context(L, M, 5, y_dtype=pkg.VBMF_Y_F32) as c2:             # no Y
        assert raw(c2) == VI and "no Y" in c2._lib.vbmf_last_error(c2._h).decode() and untouched()
    for v in (C.VBMF_VARIANT_SPARSE_DIAGVAR, C.VBMF_VARIANT_DUAL_DIAGVAR, C.VBMF_VARIANT_TRIAL_DIAGVAR):
        with C.Context(L, M, 5, y_dtype=pkg.VBMF_Y_F32, variant=v) as c2:
            assert raw(c2) == VI and "diag_var" in c2._lib.vbmf_last_error(c2._h).decode() and untouched()
    with C.Context(L, M, 5, y_dtype=pkg.VBMF_Y_F32, nranks=2, rank=0, L_global=2 * L, variant=C.VBMF_VARIANT_SPARSE_DIAG) as c2:
        assert raw(c2) == VI and "rank" in c2._lib.vbmf_last_error(c2._h).decode() and untouched()


# ---- 5. classify_folds and test_classification_folds ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pool_case():
    """24 bags of L = 166 drawn alternately from the two bases of rank 5, their labels, three folds of 8 test bags"""
    Bs, draw = _two_bases(5, 7105, rows=166)
    Ys = [GOLD._f32(draw(b % 2, m)) for b, m in enumerate(GOLD.WIDTHS * 3)]
    labels = np.array([b % 2 for b in range(24)])
    perm = np.random.default_rng(52).permutation(24)
    tests = [[int(b) for b in perm[8 * f:8 * f + 8]] for f in range(3)]
    return Bs, Ys, labels, tests


def test_classify_folds_is_classify_bags_per_fold(pkg, monkeypatch):
    Bs, Ys, labels, tests = _pool_case()
    res = [_model_with(pkg, "basic", B) for B in Bs]
    models = [(res[0], res[1]), (res[1], res[0]), (res[0], res[1]), (0, 0)]           # fold 1: the bases swapped
    tests4 = tests + [[2, 5]]
    made = []
    init = pkg.capi.Context.__init__

    def counting(self, *a, **k):
        made.append(a)
        return init(self, *a, **k)

    with pkg.BagPool(Ys) as pool:
        for alg in ("ols", "rls"):
            monkeypatch.setattr(pkg.capi.Context, "__init__", counting)
            del made[:]
            out = pkg.classify_folds(models, tests4, pool, alg)
            summ = pkg.test_classification_folds(models, tests4, pool, labels, alg)
            assert made == []                                          # on the pool's own context: no select, no new context
            monkeypatch.setattr(pkg.capi.Context, "__init__", init)
            assert out[3] is None and summ[3] == (-1.0,) * 6
            for f in range(3):
                sel = pool.select(tests[f], 5)
                try:
                    want = pkg.classify_bags(models[f][0], models[f][1], sel, alg)
                    wsum = pkg.test_classification_batch(models[f][0], models[f][1], sel, labels[tests[f]], alg)
                finally:
                    sel.close()
                assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(out[f], want)), (alg, f)
                assert summ[f] == wsum, (alg, f, summ[f], wsum)
                drawn = labels[tests[f]]
                assert np.array_equal(out[f][0], 1 - drawn if f == 1 else drawn)
                assert summ[f][2] + summ[f][3] == (8 if f == 1 else 0)
            uploaded = pkg.Bags(Ys, 5)
            try:
                for src in (Ys, uploaded):
                    got = pkg.classify_folds(models, tests4, src, alg)
                    assert got[3] is None
                    assert all(np.array_equal(a, b) for f in range(3) for a, b in zip(got[f], out[f]))
                    assert pkg.test_classification_folds(models, tests4, src, labels, alg) == summ
            finally:
                uploaded.close()


# ---- 6. validate_folds ---------------------------------------------------------------------------------------------------------
def test_validate_folds_is_train_folds_then_test_classification_folds(pkg):
    _, Ys, labels, tests = _pool_case()
    splits = [(tests[1] + tests[2], tests[0]), (tests[0] + tests[2], tests[1])]
    with pkg.BagPool(Ys) as pool:
        got = pkg.validate_folds(pool, labels, splits, "basic", 5, 20, rng=np.random.default_rng(77))
        folds = [([b for b in tr if labels[b] == 0], [b for b in tr if labels[b] == 1]) for tr, _ in splits]
        models = pkg.train_folds(folds, "basic", 5, 20, rng=np.random.default_rng(77), pool=pool)
        want = pkg.test_classification_folds(models, [te for _, te in splits], pool, labels)
    assert got == want and len(got) == 2
    assert all(t[4] + t[5] == 8 and 0.0 <= t[0] <= 1.0 for t in got)


# ---- 7. the parent commit's bits -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage,L", sorted(GOLD.CONTEXTS))
def test_old_entry_and_jobs_reproduce_the_parent_build(pkg, storage, L):
    """CRC-32s recorded on the parent commit's build through vbmf_bag_least_squares, per (storage, L, H, basis, lambda, bag): the old
    entry still returns them after the kernels' bodies moved into shared device functions, and so does every job of the new one"""
    case, gold = _cases()[storage, L], _gold()
    Ys = case["Ys"]
    bases = [(H, k, B, lam) for H, Bs in case["bases"].items() for k, B in enumerate(Bs) for lam in case["lams"]]
    jobs = [(b, q) for q in range(len(bases)) for b in range(len(Ys))]
    c, off = GOLD.upload(pkg, storage, Ys)
    with c:
        for H, k, B, lam in bases:
            assert GOLD.bag_crcs(*c.bag_least_squares(off, B, lam), off) == gold[GOLD.key(storage, L, H, k, lam)], (H, k, lam)
        Xs, r2, status = c.bag_least_squares_jobs(off, [B for _, _, B, _ in bases], [lam for _, _, _, lam in bases], [b for b, _ in jobs],
                                                  [q for _, q in jobs], want_X=True)
    assert not status.any()
    for j, (b, q) in enumerate(jobs):
        H, k, _, lam = bases[q]
        assert [GOLD.crc(Xs[j]), GOLD.crc(r2[j:j + 1])] == gold[GOLD.key(storage, L, H, k, lam)][b], (j, b, H, k, lam)
