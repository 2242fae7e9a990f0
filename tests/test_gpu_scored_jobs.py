"""factorize_bag and its scores for a list of (bag, model) jobs in one device call (vbmf_sparse_scored_jobs, Context.sparse_scored_jobs;
factorize_folds, classify_folds with "lower_bound" / "min_err", validate_local_folds): every per-job field and r2 against fp64, the
bound against the oracle's lowerBound / lowerBoundTrimmed, both classifiers' labels against the oracle's, the segmentation properties
bit for bit, the parent build's bits of the old entry and of the bound's sums, the isolation of a failed job, the C ABI's refusals,
and validate_local_folds end to end.

Models: trained("sparse", L, H, 4000 + 10 H + L) of tests/test_vbls_jobs_host.py with H1 assigned afterwards, bags from its sampler
rounded to fp32 (one bf16-storage case compares on vbmf_get_Y's values).  Shapes: L = 33 and 300; (H, H1) = (2, 1), (5, 1), (5, 2),
(17, 1) -- the truncated model in the one-block tier, the whole one in the two-block tier: two launches in one call -- and (32, 1);
widths 1, 2, 3, 8, 9, 17, 60, the widest bag whose state stays in LDS for the whole model (vbmf_debug_vbls_jobs_lds_cols) and one
more, and on either side of factorize_bag's M_b (H - H1) < 1600: 99 | 100 at (17, 1), 51 | 52 at (32, 1).

Reference: ref_factorize of tests/test_scored_jobs_host.py (pinned there to the oracle's own loop where its dense inverse is
affordable).  Bounds: every field, r2 and the bound are held to 3 x the worst error measured on an MI355X over this file's cases
(MEASURED, LB_SCALED_MEASURED below), none looser than TOL of tests/test_gpu_vbls_jobs.py or BOUND_SCALED_TOL of
tests/test_gpu_bag_scoring.py.  The bound's error is scaled by L M_b as there (a bound is a sum of about L M_b terms of order one;
no zero crossing inflates it).
"""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest

import __graft_entry__ as G
from oracle import vbmf_oracle as O
from tests.helpers import relF, report
from tests.test_gpu_bag_scoring import BOUND_SCALED_TOL, CLASSIFY_BOUND_TOL
from tests.test_gpu_vbls_jobs import TOL as TOL_JOBS
from tests.test_gpu_vbls_sparse_batch import _convert
from tests.test_scored_jobs_host import full_form, oracle_pair, ref_factorize, scored_arrays
from tests.test_vbls_jobs_host import FIELDS, model_arrays, oracle_vbls, trained

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_vbls_jobs_crc", os.path.join(G.ROOT, "tests", "golden", "make_vbls_jobs_crc.py"))
GOLD = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(GOLD)

NITER = 20
THRS = (1e-1, 0.5, 0.0)
CASES = [(33, 2, 1), (33, 5, 1), (300, 5, 2), (33, 17, 1), (300, 32, 1)]
WIDTHS = [1, 2, 3, 8, 9, 17, 60]
EDGE = {(17, 1): [99, 100], (32, 1): [51, 52]}            # M_b (H - H1) = 1584 | 1600 and 1581 | 1612
# measured on an MI355X, worst over the five cases of test_against_fp64 and its bf16-storage case, per form of updateA! (False: the
# diagonal form, which only the bags of 100 and 52 columns take).  Both sides are fp64 evaluations of one recurrence on the same
# operands; sigmaHat, zeta, SigmaA and diagSigmaATVec move together under full_cov, as in tests/test_gpu_vbls_jobs.py.  r2 is compared
# with the reference's own residual, so it carries the movement of A.  Where 3 x the measured value would exceed that file's TOL
# (sigmaHat and zeta under full_cov: 1.44e-12 here, 1.35e-12 there), its TOL holds.
MEASURED = {False: dict(ATVecHat=3.72e-16, diagSigmaATVec=1.81e-15, CA=1.40e-15, beta=7.43e-16, SigmaA=1.45e-15, sigmaHat=3.90e-15,
                        zeta=4.01e-15, r2=2.55e-16),
            True: dict(ATVecHat=1.93e-15, diagSigmaATVec=8.42e-13, CA=3.13e-13, beta=2.61e-15, SigmaA=8.35e-13, sigmaHat=1.44e-12,
                       zeta=1.44e-12, r2=6.68e-14)}
TOL = {full: {f: min(3 * v, TOL_JOBS[full].get(f, np.inf)) for f, v in m.items()} for full, m in MEASURED.items()}
# |lb - oracle| / (L M_b), worst over the same cases, THRS and the grouped dual case (4.05e-14): at (33, 2, 1).
# BOUND_SCALED_MEASURED of tests/test_gpu_bag_scoring.py is 3.73e-7: that entry reads BHat and Y'B through fp32
LB_SCALED_MEASURED = 6.20e-13
LB_SCALED_TOL = 3 * LB_SCALED_MEASURED


def test_no_bound_is_looser_than_the_issue_allows():
    for full in (False, True):
        assert all(TOL[full][f] <= TOL_JOBS[full][f] for f in FIELDS), full
    assert LB_SCALED_TOL <= BOUND_SCALED_TOL


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


def _lds_cols(H):
    return G.load_package().capi.vbls_jobs_lds_cols(H, True)


@functools.lru_cache(maxsize=None)
def _model(L, H, H1):
    po, draw = trained("sparse", L, H, 4000 + 10 * H + L)
    po.H1 = H1
    return po, draw


@functools.lru_cache(maxsize=None)
def _case(L, H, H1, small=False):
    """(the oracle set, the bags, the reference of every bag at every threshold); computed once, shared and left unchanged"""
    po, draw = _model(L, H, H1)
    lds = _lds_cols(H)
    widths = [1, 3, 9] if small else WIDTHS + EDGE.get((H, H1), []) + [lds, lds + 1]
    Ys = [_f32(draw(w)) for w in widths]
    return po, Ys, _refs(po, Ys)


def _refs(po, Ys):
    refs = []
    for Y in Ys:
        r = ref_factorize(Y, po, NITER, THRS[0])
        r["L1"] = {t: (r["L1"] if t == THRS[0] else O.lowerBoundTrimmed(Y, r["sets"][1], t)) for t in THRS}
        refs.append(r)
    return refs


def _upload(pkg, Ys, storage="f32"):
    C = pkg.capi
    off = np.concatenate([[0], np.cumsum([Y.shape[1] for Y in Ys])]).astype(np.int64)
    c = C.Context(Ys[0].shape[0], int(off[-1]), 1, y_dtype=C.VBMF_Y_BF16 if storage == "bf16" else C.VBMF_Y_F32)
    c.set_Y(np.asfortranarray(np.hstack(Ys)))
    return c, off


def _block(r, j, f):
    if f in ("sigmaHat", "zeta"):
        return float(r[f][j])
    if f == "SigmaA":
        return np.asarray(r[f][j])
    return r[f][r["off"][j]:r["off"][j + 1]]


def _job_equal(ra, ja, rb, jb, lb=True):
    return all(np.array_equal(_block(ra, ja, f), _block(rb, jb, f)) for f in FIELDS) and ra["r2"][ja] == rb["r2"][jb] \
        and ra["status"][ja] == rb["status"][jb] and (not lb or ra["lb"][ja] == rb["lb"][jb])


def _jobs_of(po, Ys):
    """per bag: (b, 0, lowerBound) and (b, 1, lowerBoundTrimmed(t)) for every t of THRS, with factorize_bag's form"""
    jobs = []
    for b, Y in enumerate(Ys):
        full = full_form(Y.shape[1], po.H, po.H1)
        jobs += [(b, 0, full, -1.0)] + [(b, 1, full, t) for t in THRS]
    return jobs


def _run(c, off, mods, jobs, **kw):
    return c.sparse_scored_jobs(off, mods, [j[0] for j in jobs], [j[1] for j in jobs], [j[2] for j in jobs], [j[3] for j in jobs], NITER, **kw)


# ---- 1. against fp64: the fields, r2 and the bound -------------------------------------------------------------------------------------
def _against_fp64(pkg, L, H, H1, storage):
    if storage == "f32":
        po, Ys, refs = _case(L, H, H1)
    else:
        po, draw = _model(L, H, H1)
        Ys = [draw(w) for w in (1, 2, 3, 8, 9, 17, 60)]
    mods = [scored_arrays(q) for q in oracle_pair(Ys[0], po)]
    jobs = _jobs_of(po, Ys)
    perm = np.random.default_rng(77 + H).permutation(len(jobs))
    jobs = [jobs[i] for i in perm]
    c, off = _upload(pkg, Ys, storage)
    with c:
        Yst = c.get_Y()
        r = _run(c, off, mods, jobs)
    Ysts = [Yst[:, off[b]:off[b + 1]] for b in range(len(Ys))]
    if storage == "f32":
        assert all(np.array_equal(a, b) for a, b in zip(Ysts, Ys))
    else:
        refs = _refs(po, Ysts)                                         # (the reference works on Y as stored)
    # the oracle's side: no |ATVecHat| within 1e-9 of a threshold, so the fp64 mask cannot differ
    a = np.abs(np.concatenate([ref["sets"][1].ATVecHat for ref in refs]))
    for t in THRS:
        assert np.min(np.abs(a - t)) > 1e-9, t
    assert not r["status"].any()
    forms = {full_form(Y.shape[1], H, H1) for Y in Ys}
    worst = {full: {f: 0.0 for f in FIELDS + ("r2",)} for full in forms}
    lb_scaled = 0.0
    for j, (b, k, full, t) in enumerate(jobs):
        ref, w = refs[b], worst[full]
        want = ref["fits"][k]
        for f in FIELDS:
            x, o = _block(r, j, f), want[f]
            w[f] = max(w[f], abs(x - o) / abs(o) if np.isscalar(o) else relF(x, o))
        w["r2"] = max(w["r2"], abs(r["r2"][j] - want["r2"]) / want["r2"])
        lb = ref["L0"] if k == 0 else ref["L1"][t]
        lb_scaled = max(lb_scaled, abs(r["lb"][j] - lb) / (L * Ys[b].shape[1]))
    for full, w in worst.items():
        report(f"scored_jobs L{L} H{H} H1={H1} full_cov={int(full)} {storage} {len(jobs)} jobs: "
               + " ".join(f"{k}={v:.2e}" for k, v in w.items()) + f" lb_over_LM={lb_scaled:.2e}")
    return worst, lb_scaled


def _assert_fp64(worst, lb_scaled):
    for full, w in worst.items():
        bad = {k: v for k, v in w.items() if not v <= TOL[full][k]}
        assert not bad, (full, bad)
    assert lb_scaled <= LB_SCALED_TOL and lb_scaled <= BOUND_SCALED_TOL, lb_scaled


@pytest.mark.parametrize("L,H,H1", CASES)
def test_against_fp64(pkg, L, H, H1):
    _assert_fp64(*_against_fp64(pkg, L, H, H1, "f32"))


def test_against_fp64_bf16_storage(pkg):
    _assert_fp64(*_against_fp64(pkg, 33, 5, 1, "bf16"))


# ---- 2. the classifiers' labels -------------------------------------------------------------------------------------------------------
def _oracle_labels(refs, thr):
    L0 = np.array([r["L0"] for r in refs])
    L1 = np.array([r["L1"][thr] for r in refs])
    e0, e1 = np.array([r["err0"] for r in refs]), np.array([r["err1"] for r in refs])
    rel = np.abs((e0 - e1) / e0)
    return dict(lower_bound=(L1 > L0).astype(np.int64), min_err=np.where(rel < thr, 0, 1).astype(np.int64), L0=L0, L1=L1, e0=e0, e1=e1,
                rel=rel)


def test_both_labels_occur_in_the_oracle_s_numbers():
    lb, me = [], []
    for L, H, H1 in CASES:
        refs = _case(L, H, H1)[2]
        lb.append(_oracle_labels(refs, 0.0)["lower_bound"])            # (at threshold 0, as tests/test_gpu_bag_scoring.py does)
        me.append(_oracle_labels(refs, THRS[0])["min_err"])
    for v in (np.concatenate(lb), np.concatenate(me)):
        assert 0 < v.sum() < v.size, v


@pytest.mark.parametrize("L", [33, 300])
def test_labels_equal_the_oracle_s(pkg, L):
    """one classify_folds call per classifier and threshold over folds of different H and H1: fold f's bags against fold f's model"""
    cases = [c for c in CASES if c[0] == L]
    Ys, tests, models, want = [], [], [], {}
    for Lc, H, H1 in cases:
        po, ys, refs = _case(Lc, H, H1)
        tests.append(list(range(len(Ys), len(Ys) + len(ys))))
        Ys += ys
        res = _convert(pkg.vbmf_sparse_parameters, po)
        res.H1 = H1
        models.append(res if len(models) % 2 else (res, None))
        for thr in (THRS[0], 0.0):
            o = _oracle_labels(refs, thr)
            scale = Lc * np.array([y.shape[1] for y in ys], dtype=np.float64)
            # the margins, on the oracle's numbers alone: no bag is left out
            assert np.min(np.abs(o["L1"] - o["L0"]) / scale) > 100 * LB_SCALED_TOL, (H, H1, thr)
            if thr > 0:
                assert np.min(np.abs(o["rel"] - thr)) > 100 * 2 * TOL[True]["r2"], (H, H1, thr)
            want[len(models) - 1, thr] = o
    with pkg.BagPool(Ys) as pool:
        for thr in (THRS[0], 0.0):
            got = pkg.classify_folds(models, tests, pool, "lower_bound", threshold=thr)
            for f in range(len(models)):
                assert np.array_equal(got[f][0], want[f, thr]["lower_bound"]), (f, thr)
        got = pkg.classify_folds(models, tests, pool, "min_err", threshold=THRS[0])
        for f in range(len(models)):
            o = want[f, THRS[0]]
            assert np.array_equal(got[f][0], o["min_err"]), f
            assert max(relF(got[f][1], o["e0"]), relF(got[f][2], o["e1"])) <= TOL[True]["r2"]
        scores = pkg.factorize_folds(models, tests, pool)
    listed = pkg.factorize_folds(models, tests, Ys)                      # the same bags as a list of matrices: the same bits
    for a, b in zip(scores, listed):
        assert all(np.array_equal(a[k], b[k]) for k in ("L0", "L1", "err0", "err1", "status"))


# ---- 3. a grouped model through the capi wrapper ---------------------------------------------------------------------------------------
def test_grouped_dual_model(pkg):
    L, H = 33, 5
    po, draw = trained("dual", L, H, 4000 + 10 * H + 1 + L)
    Ys = [_f32(draw(w)) for w in (1, 3, 8, 9, 17)]
    first = np.arange(H) < int(po.H0)
    a_pri, b_pri = np.where(first, po.alpha00, po.alpha01), np.where(first, po.beta00, po.beta01).astype(np.float64)
    m = dict(model_arrays(po), CB=po.CB, delta=po.delta, gamma=po.gamma, gamma0=po.gamma0, delta0=po.delta0, a_pri=a_pri, b_pri=b_pri,
             a_post=a_pri + 0.5)
    jobs = [(b, 0, True, t) for b in range(len(Ys)) for t in (-1.0,) + THRS]
    c, off = _upload(pkg, Ys)
    with c:
        r = _run(c, off, [m], jobs, grouped=True)
    assert not r["status"].any()
    worst = 0.0
    for j, (b, _, _, t) in enumerate(jobs):
        q = oracle_vbls(pkg, Ys[b], po, NITER, True, seed=b)
        assert t < 0 or np.min(np.abs(np.abs(q.ATVecHat) - t)) > 1e-9
        want = O.lowerBound_dual(Ys[b], q) if t < 0 else O.lowerBoundTrimmed(Ys[b], q, t)
        worst = max(worst, abs(r["lb"][j] - want) / (L * Ys[b].shape[1]))
    report(f"scored_jobs dual grouped L{L} H{H}: lb_over_LM={worst:.2e}")
    assert worst <= LB_SCALED_TOL, worst


# ---- 4. bitwise properties ------------------------------------------------------------------------------------------------------------
def test_jobs_do_not_depend_on_each_other_or_on_their_grouping(pkg):
    """(17, 1): the truncated model runs in the one-block tier, the whole one in the two-block tier, and the bags of 100 columns and
    more in the diagonal form -- four groups in one call"""
    L, H, H1 = 33, 17, 1
    po, Ys, _ = _case(L, H, H1)
    mods = [scored_arrays(q) for q in oracle_pair(Ys[0], po)]
    jobs = _jobs_of(po, Ys)
    assert {(k, f) for _, k, f, _ in jobs} == {(0, True), (0, False), (1, True), (1, False)}
    perm = np.random.default_rng(5).permutation(len(jobs))
    c, off = _upload(pkg, Ys)
    with c:
        base = _run(c, off, mods, jobs)
        assert not base["status"].any()
        pr = _run(c, off, mods, [jobs[i] for i in perm])
        assert all(_job_equal(pr, j, base, int(i)) for j, i in enumerate(perm))
        for j in (0, 1, 5, len(jobs) - 4, len(jobs) - 1):
            b, k, full, t = jobs[j]
            assert _job_equal(_run(c, off, mods, [jobs[j]]), 0, base, j), j
            assert _job_equal(_run(c, off, [mods[k]], [(b, 0, full, t)]), 0, base, j), j           # with only its own model in the call
        # the form is the job's: a bag's two forms side by side equal the two forms run apart
        b = 3
        both = _run(c, off, mods, [(b, 1, True, 0.1), (b, 1, False, 0.1)])
        assert _job_equal(both, 0, _run(c, off, mods, [(b, 1, True, 0.1)]), 0) and _job_equal(both, 1, _run(c, off, mods, [(b, 1, False, 0.1)]), 0)
        assert not np.array_equal(_block(both, 0, "ATVecHat"), _block(both, 1, "ATVecHat"))
        # the old entry, block for block, on the jobs it can run: one H and one form per call
        for k in (0, 1):
            for full in (True, False):
                sub = [j for j, q in enumerate(jobs) if q[1] == k and q[2] == full and q[3] in (-1.0, THRS[0])]
                old = c.sparse_fixed_basis_jobs(off, mods[k]["BHat"].shape[1], [mods[k]], [jobs[j][0] for j in sub], [0] * len(sub), NITER,
                                                full_cov=full)
                old["SigmaA"] = list(old["SigmaA"])
                assert sub and all(_job_equal(old, i, base, j, lb=False) for i, j in enumerate(sub)), (k, full)
    with pkg.BagPool(Ys) as pool:                                        # where the bag sits in Y: a pool, and a bag uploaded alone
        pr = _run(pool.ctx, pool.col_off, mods, jobs)
        assert all(_job_equal(pr, j, base, j) for j in range(len(jobs)))
    for b in (0, 4, len(Ys) - 1):
        bags = pkg.Bags([Ys[b]], 1)
        try:
            sub = [j for j, q in enumerate(jobs) if q[0] == b]
            fr = _run(bags.ctx, bags.col_off, mods, [(0,) + jobs[j][1:] for j in sub])
        finally:
            bags.close()
        assert all(_job_equal(fr, i, base, j) for i, j in enumerate(sub)), b


@functools.lru_cache(maxsize=None)
def _gold():
    with open(GOLD.GOLDEN) as f:
        return json.load(f)["crc"]


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("L,H", GOLD.SHAPES)
def test_the_old_entry_reproduces_the_parent_build(pkg, L, H, full):
    """CRC-32s recorded on the parent commit's build (tests/golden/make_vbls_jobs_crc.py): the old entry still returns them, and so does
    every such job of the new one"""
    mods, Ys, jobs = GOLD.case(L, H, full)
    c, off = GOLD.upload(pkg, Ys)
    with c:
        old = c.sparse_fixed_basis_jobs(off, H, mods, [b for b, _ in jobs], [k for _, k in jobs], GOLD.NITER, full_cov=full)
        one = np.ones(H)
        sm = [dict(m, CB=one, delta=one, gamma=1.0 + L / 2, gamma0=1.0, delta0=1.0, a_pri=m["alpha"] - 0.5, b_pri=m["beta0"], a_post=m["alpha"])
              for m in mods]
        new = c.sparse_scored_jobs(off, sm, [b for b, _ in jobs], [k for _, k in jobs], [full] * len(jobs), [0.1] * len(jobs), GOLD.NITER)
    assert not old["status"].any() and not new["status"].any() and np.isfinite(new["lb"]).all()
    gold = _gold()[GOLD.key(L, H, full)]
    assert [GOLD.job_crcs(old, j) for j in range(len(jobs))] == gold
    assert [GOLD.job_crcs(new, j) for j in range(len(jobs))] == gold


def test_the_bound_s_sums_reproduce_the_parent_build(pkg):
    """bag_lb_sums_kernel's arithmetic moved into the __device__ function the job kernel shares: lowerBound_batch and
    lowerBoundTrimmed_batch on one fixed input against the CRC-32s of the parent commit's build"""
    Ys, qs = GOLD.bound_inputs(pkg)
    assert [GOLD.crc(pkg.lowerBound_batch(Ys, qs)), GOLD.crc(pkg.lowerBoundTrimmed_batch(Ys, qs, 1e-1))] == _gold()["lowerBound_batch"]


# ---- 5. a failed job --------------------------------------------------------------------------------------------------------------------
def test_a_failed_job_leaves_the_other_jobs_alone(pkg):
    """a model with a zero in delta: sum log delta = -inf, which no refusal catches (delta is finite) and the device does not flag;
    the host finds the bound not finite and fails those jobs alone"""
    L, H, H1 = 33, 5, 1
    po, Ys, _ = _case(L, H, H1, small=True)
    mods = [scored_arrays(q) for q in oracle_pair(Ys[0], po)]
    bad = dict(mods[1], delta=mods[1]["delta"].copy())
    bad["delta"][2] = 0.0
    jobs = [(b, k, True, -1.0 if k == 0 else 0.1) for b in range(len(Ys)) for k in (0, 1, 2)]
    c, off = _upload(pkg, Ys)
    with c:
        r = _run(c, off, mods + [bad], jobs)
        good = [q for q in jobs if q[1] != 2]
        r2 = _run(c, off, mods, good)
    assert np.array_equal(r["status"], [int(k == 2) for _, k, _, _ in jobs]) and not r2["status"].any()
    for j, (b, k, _, _) in enumerate(jobs):
        if k == 2:
            assert np.isnan(r["lb"][j]) and np.isnan(r["r2"][j]) and all(np.all(np.isnan(_block(r, j, f))) for f in FIELDS), j
            assert _block(r, j, "ATVecHat").shape == (Ys[b].shape[1] * H,)
    for j2, q in enumerate(good):
        j = jobs.index(q)
        assert _job_equal(r, j, r2, j2), q
        assert np.isfinite(r["lb"][j]) and np.isfinite(r["r2"][j]) and all(np.all(np.isfinite(_block(r, j, f))) for f in FIELDS)


# ---- 6. C ABI refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(pkg):
    C = pkg.capi
    VI, VU = C.VBMF_ERR_INVALID, C.VBMF_ERR_UNSUPPORTED
    L = 33
    po5, po2 = _model(L, 5, 1)[0], _model(L, 2, 1)[0]
    Ys = [_f32(_model(L, 5, 1)[1](w)) for w in (3, 1, 2, 7, 8, 9, 17, 4)]
    mods = [scored_arrays(q) for q in oracle_pair(Ys[0], po5)] + [scored_arrays(oracle_pair(Ys[0], po2)[1])]       # H = 4, 5, 2
    ip, dp = C.C.POINTER(C.C.c_int64), C.C.POINTER(C.C.c_double)
    i64 = lambda v: np.array(v, dtype=np.int64)
    pk = lambda key, order="C": np.concatenate([np.asarray(m[key], dtype=np.float64).reshape(-1, order=order) for m in mods])
    SENT = -7.0
    c, off = _upload(pkg, Ys)
    nb, M = len(Ys), int(off[-1])
    PER_MODEL = ("B", "SB", "CB", "de", "ga", "g0", "d0", "ap", "bp", "po", "e0", "z0", "s0", "c0")
    good = dict(o=off, niter=NITER, mh=i64([4, 5, 2]), B=pk("BHat", "F"), SB=pk("SigmaB", "F"), CB=pk("CB"), de=pk("delta"), ga=pk("gamma"),
                g0=pk("gamma0"), d0=pk("delta0"), ap=pk("a_pri"), bp=pk("b_pri"), po=pk("a_post"), e0=pk("eta0"), z0=pk("zeta0"),
                s0=pk("sigma0"), c0=pk("ca0"), jb=i64([0, 3, 7, 3]), jk=i64([1, 0, 2, 1]), jf=i64([1, 1, 0, 0]), jt=np.array([-1.0, 0.1, 0.5, 0.0]))
    outs = {k: np.full(5 * M * 2, SENT) for k in ("A", "dS", "CA", "be")}
    outs.update(lb=np.full(8, SENT), r2=np.full(8, SENT), SA=np.full(8 * 25, SENT), sg=np.full(8, SENT), ze=np.full(8, SENT))
    sbuf = np.full(8, -7, dtype=np.int64)

    def raw(ctx, nk=3, nj=None, s=sbuf, null=(), **kw):
        a = {**good, **kw}
        p = lambda v, t=dp: None if v is None else v.ctypes.data_as(t)
        o = {k: (None if k in null else v) for k, v in outs.items()}
        nj = (4 if a["jb"] is None else len(a["jb"])) if nj is None else nj
        return C.lib().vbmf_sparse_scored_jobs(ctx._h, len(a["o"]) - 1, p(a["o"], ip), a["niter"], 1, 0, nk, p(a["mh"], ip),
                                               *[p(a[k]) for k in PER_MODEL], nj, p(a["jb"], ip), p(a["jk"], ip), p(a["jf"], ip), p(a["jt"]),
                                               p(o["lb"]), p(o["r2"]), p(o["A"]), p(o["dS"]), p(o["CA"]), p(o["be"]), p(o["SA"]), p(o["sg"]),
                                               p(o["ze"]), p(s, ip))

    def untouched():
        return all(np.all(v == SENT) for v in outs.values()) and np.all(sbuf == -7)

    def spoiled(key, i, v):
        x = good[key].copy(); x[i] = v
        return {key: x}

    refused = [(VU, dict(mh=i64([4, 0, 2]))), (VU, dict(mh=i64([33, 5, 2]))), (VU, dict(mh=i64([4, 5, -1]))),
               (VI, dict(nk=0)), (VI, dict(nj=0)), (VI, dict(nk=-1)), (VI, dict(nj=-3)), (VI, dict(niter=0)), (VI, dict(niter=-2)),
               (VI, dict(s=None)), (VI, dict(null=("lb", "r2", "A")))]
    refused += [(VU, dict(nj=1 << 24)), (VU, dict(nk=1 << 24))]          # more workgroups than one grid holds: refused before any table is read
    refused += [(VI, {k: None}) for k in PER_MODEL + ("mh", "jb", "jk", "jf", "jt")]
    refused += [(VI, spoiled(k, i, v)) for k, i in (("B", -1), ("B", 7), ("SB", 3), ("CB", 5), ("de", 0), ("ga", 1), ("g0", 2), ("d0", 0),
                                                    ("ap", 4), ("bp", 9), ("po", 1), ("e0", 0), ("z0", 1), ("s0", 0), ("c0", 1), ("jt", 2))
                for v in (np.nan, np.inf)]
    refused += [(VI, dict(jb=i64([0, 3, nb, 3]))), (VI, dict(jb=i64([-1, 3, 7, 3]))), (VI, dict(jk=i64([1, 0, 3, 1]))), (VI, dict(jk=i64([1, -1, 1, 1]))),
                (VI, dict(jf=i64([1, 2, 0, 0]))), (VI, dict(jf=i64([-1, 1, 0, 0])))]
    refused += [(VI, dict(o=i64(b))) for b in ([0, 1, 1, M], [1, 17, M], [0, 17, M - 1], [0, 20, 10, M], [0, M + 1])]
    refused += [(VI, dict(jb=i64([0, 3, 1, 3])))]                        # a 1-column bag in a job whose own form is the diagonal one (QS1)
    with c:
        Y0, dims0 = c.get_Y(), c.dims()
        ref = c.sparse_scored_jobs(off, mods, good["jb"], good["jk"], good["jf"], good["jt"], NITER)
        for code, kw in refused:
            if "o" in kw:                                             # (the jobs name bags of the shorter col_off)
                kw = dict(kw, jb=i64([0, 0, 0, 0]), jf=i64([1, 1, 1, 1]))
            assert raw(c, **kw) == code, kw
            assert untouched(), kw
        assert raw(c, **spoiled("de", 0, np.nan)) == VI and "delta of model 0 is not finite" in c._lib.vbmf_last_error(c._h).decode()
        assert raw(c, **refused[-1][1]) == VI and "1-column bag" in c._lib.vbmf_last_error(c._h).decode()
        # the same 1-column bag in the full_cov form is a job like any other
        assert raw(c, jb=i64([0, 3, 7, 1]), jf=i64([1, 1, 0, 1])) == C.VBMF_OK
        for v in outs.values():
            v[:] = SENT
        sbuf[:] = -7
        assert np.array_equal(c.get_Y(), Y0) and c.dims() == dims0
        # after the refusals a good call returns the former bits, and writes only its own jobs
        assert raw(c) == C.VBMF_OK and np.array_equal(sbuf[:4], [0, 0, 0, 0]) and np.all(sbuf[4:] == -7)
        n = int(ref["off"][-1])
        assert np.array_equal(outs["lb"][:4], ref["lb"]) and np.all(outs["lb"][4:] == SENT) and np.isfinite(ref["lb"]).all()
        assert np.array_equal(outs["r2"][:4], ref["r2"]) and np.all(outs["r2"][4:] == SENT)
        assert np.array_equal(outs["A"][:n], ref["ATVecHat"]) and np.all(outs["A"][n:] == SENT)
        nsa = 25 + 16 + 4 + 25
        assert np.array_equal(outs["SA"][:nsa], np.concatenate([s.reshape(-1) for s in ref["SigmaA"]])) and np.all(outs["SA"][nsa:] == SENT)
        # one output at a time: the other pointers NULL
        for v in outs.values():
            v[:] = SENT
        assert raw(c, null=("r2", "A", "dS", "CA", "be", "SA", "sg", "ze")) == C.VBMF_OK and np.array_equal(outs["lb"][:4], ref["lb"])
        assert all(np.all(v == SENT) for k, v in outs.items() if k != "lb")
        # a label mask on the context
        z = np.zeros
        c.set_state(z((M, 1)), np.ones((L, 1)), z((1, 1)), z((1, 1)), np.ones(1), np.ones(1), 1.0, labels0=[0], H1=1)
        for v in outs.values():
            v[:] = SENT
        sbuf[:] = -7
        assert raw(c) == VI and "label mask" in c._lib.vbmf_last_error(c._h).decode() and untouched()
    with C.Context(L, M, 5, y_dtype=pkg.VBMF_Y_F32) as c2:             # no Y
        assert raw(c2) == VI and "no Y" in c2._lib.vbmf_last_error(c2._h).decode() and untouched()
    with C.Context(L, M, 5, y_dtype=pkg.VBMF_Y_F32, nranks=2, rank=0, L_global=2 * L, variant=C.VBMF_VARIANT_SPARSE_DIAG) as c2:
        assert raw(c2) == VI and "rank" in c2._lib.vbmf_last_error(c2._h).decode() and untouched()


# ---- 7. validate_local_folds end to end ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ["lower_bound", "min_err"])
def test_validate_local_folds_end_to_end(pkg, alg):
    """a 12-bag pool, three splits: validate_local_folds against train_local_folds and classify_bags per fold (the loop the parent
    offers, fp32 Y'B and a fresh upload per basis).  The scores agree within that path's own bound, the labels are equal."""
    L, H, H1, niter = 33, 5, 1, 12
    rng = np.random.default_rng(8100)
    Bs = rng.standard_normal((L, H)) * np.linspace(1.0, 2.5, H)
    labels = [b % 2 for b in range(12)]
    Ys = []
    for b, m in enumerate([3, 5, 8, 2, 9, 4, 6, 7, 3, 5, 4, 6]):
        As = np.zeros((m, H)); As[np.arange(m), rng.integers(0, H - H1, m) if labels[b] == 0 else rng.integers(0, H, m)] = 1.0
        Ys.append(_f32(Bs @ As.T + 0.05 * rng.standard_normal((L, m))))
    splits = [([b for b in range(12) if b % 3 != s], [b for b in range(12) if b % 3 == s]) for s in range(3)]
    with pkg.BagPool(Ys) as pool:
        got = pkg.validate_local_folds(pool, labels, splits, H, H1, niter, class_alg=alg, rng=np.random.default_rng(3))
        folds = [([b for b in tr if labels[b] == 0], [b for b in tr if labels[b] == 1]) for tr, _ in splits]
        models = pkg.train_local_folds(folds, H, H1, niter, eps=1e-6, rng=np.random.default_rng(3), pool=pool)
        new = pkg.classify_folds(models, [te for _, te in splits], pool, alg)
        again = pkg.test_classification_folds(models, [te for _, te in splits], pool, labels, alg)
    assert got == again
    for f, (_, te) in enumerate(splits):
        lab, s0, s1 = pkg.classify_bags(models[f], 0, [Ys[b] for b in te], alg)
        d = max(float(np.max(np.abs(new[f][1] - s0) / np.abs(s0))), float(np.max(np.abs(new[f][2] - s1) / np.abs(s1))))
        report(f"validate_local_folds {alg} fold {f}: score diff to classify_bags {d:.2e}")
        assert d <= CLASSIFY_BOUND_TOL, (f, d)
        # a label may differ only where the per-fold path's own error bound reaches the decision
        if alg == "lower_bound":
            safe = np.abs(s1 - s0) / np.maximum(np.abs(s0), np.abs(s1)) > 2 * CLASSIFY_BOUND_TOL
        else:
            safe = np.abs(np.abs((s0 - s1) / s0) - 1e-1) > 4 * CLASSIFY_BOUND_TOL
        assert safe.all(), (f, s0, s1)
        assert np.array_equal(new[f][0], lab), f
