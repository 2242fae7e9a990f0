"""Scoring many bags in one device call (vbmf_bag_residuals, vbmf_sparse_lower_bound_batched; residual_batch, lowerBound_batch,
lowerBoundTrimmed_batch, classify_batch): the numbers the MIL classifier compares after vbls! (examples/mil_util.jl:453-535),
against fp64 NumPy, against the oracle's lowerBound / lowerBoundTrimmed per bag, against the per-bag device calls, and the C ABI's
refusals.  The bags sit side by side in one context: 1-column bags, bags straddling the 32-column tiles, up to 70 columns.

Measured on an MI355X, worst over each test's parametrisation (the asserted bounds are 3 x these, the project's margin for
summation-order movement):
  residual, Y and BHat as stored (direct form, fp64)   1.6e-15 (held to the issue's 1e-10, RESID_TOL)
  residual against the caller's fp64 BHat              2.01e-7 beside an fp32 Y, 1.36e-5 beside a bf16 Y (RESID_B64_MEASURED)
  bound against the oracle, |d| / |lb|                 2.96e-5 at a bag whose bound passes through zero, else 2e-10 .. 2e-6 (BOUND_MEASURED)
  bound against the oracle, |d| / (L M_b)              3.73e-7 (BOUND_SCALED_MEASURED)
  batched bound against the per-bag device calls       6.4e-8 (held to the bound against the oracle)
"""
import copy
import functools

import numpy as np
import pytest

import __graft_entry__ as G
from oracle import vbmf_oracle as O
from tests.helpers import report, to_pkg_params
from tests.test_gpu_vbls_sparse_batch import RAGGED, SMALL, _convert, _f32, _model, _sets

pytestmark = pytest.mark.gpu

L = 166
HS = (2, 5, 20, 64)
# residual_batch against NumPy on the operands as the device holds them: Y from vbmf_get_Y, BHat from vbmf_get_state, the caller's AHat
RESID_TOL = 1e-10
# the same against the caller's fp64 BHat: the context stores BHat in fp32 (as bf16 hi + lo, ~16 mantissa bits, beside a bf16 Y) -- the
# one fp32 operand copy of the residual; on a fitted bag ||BHat AHat'|| is 20 .. 60 times the residual, which scales BHat's rounding up
RESID_B64_MEASURED = {"f32": 2.01e-7, "bf16": 1.36e-5}      # worst over H in HS on an MI355X
RESID_B64_TOL = {k: 3 * v for k, v in RESID_B64_MEASURED.items()}
# max over the bags of |lb - oracle| / |oracle| for lowerBound_batch / lowerBoundTrimmed_batch fed the oracle's fp64 states (BHat, and
# with it r2 and B'B, again through fp32).  Worst over BOUND_CASES on an MI355X: 2.96e-5, at a bag whose trimmed bound passes through
# zero (lb = -4.7 where |lb| ~ L M_b = 5300 is typical: trial, H = 5, full_cov, trim 0.5); the other cases measure 2e-10 .. 2e-6.
BOUND_MEASURED = 2.96e-5
BOUND_TOL = 3 * BOUND_MEASURED
# the same error against the bound's own scale L M_b (every bag's bound is a sum of about L M_b terms of order one), which no
# zero crossing inflates
BOUND_SCALED_MEASURED = 3.73e-7       # worst over BOUND_CASES on an MI355X (dual, H = 64)
BOUND_SCALED_TOL = 3 * BOUND_SCALED_MEASURED
TRIMS = (1e-1, 0.5)


@pytest.fixture(scope="module")
def pkg():
    G.build()
    p = G.load_package()
    p.set_defaults(y_dtype=p.VBMF_Y_F32, factor_dtype=p.VBMF_FACTOR_AUTO)
    yield p
    p.invalidate()
    p.set_defaults(y_dtype=p.VBMF_Y_F32, factor_dtype=p.VBMF_FACTOR_AUTO)


# ---- 1. residual against fp64 ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _resid_case(H):
    """bags in the row space of a random basis, and the least-squares A of every bag plus a small perturbation: the residual is at
    the noise level, 1/400 .. 1/2500 of ||Y_b||^2, where a trace form would cancel"""
    rng = np.random.default_rng(1700 + H)
    B = rng.standard_normal((L, H)) * np.linspace(1.0, 2.5, H)
    Ys, As = [], []
    for m in RAGGED:
        A0 = np.zeros((m, H)); A0[np.arange(m), rng.integers(0, H, m)] = 1.0
        Y = B @ A0.T + 0.05 * rng.standard_normal((L, m))
        Ys.append(Y)
        As.append(np.linalg.lstsq(B, Y, rcond=None)[0].T + 1e-3 * rng.standard_normal((m, H)))
    return B, Ys, As


def _basic_sets(pkg, B, Ys, As):
    H = B.shape[1]
    ps = []
    for Y, A in zip(Ys, As):
        p = pkg.vbmf_init(Y, H, rng=np.random.default_rng(0))
        p.BHat, p.SigmaB, p.CB, p.invCB = B, np.eye(H) * 1e-3, np.eye(H), np.eye(H)
        p.AHat = A
        ps.append(p)
    return ps


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_residual_against_fp64(pkg, H, storage):
    B, Ys, As = _resid_case(H)
    try:
        pkg.set_defaults(y_dtype=pkg.VBMF_Y_BF16 if storage == "bf16" else pkg.VBMF_Y_F32, factor_dtype=pkg.VBMF_FACTOR_AUTO)
        bags = pkg.Bags(Ys, H)
        r = pkg.residual_batch(bags, _basic_sets(pkg, B, Ys, As))
        ctx = bags.session.ctx
        Yst, Bst = ctx.get_Y(), ctx.get_state()["BHat"]
        bags.close()
    finally:
        pkg.set_defaults(y_dtype=pkg.VBMF_Y_F32, factor_dtype=pkg.VBMF_FACTOR_AUTO)
    off = np.concatenate([[0], np.cumsum(RAGGED)])
    Ysts = [Yst[:, c0:c1] for c0, c1 in zip(off[:-1], off[1:])]
    want = np.array([np.linalg.norm(Y - Bst @ A.T) for Y, A in zip(Ysts, As)])
    want64 = np.array([np.linalg.norm(Y - B @ A.T) for Y, A in zip(Ysts, As)])
    ratio = max(float(np.sum(Y * Y)) / w ** 2 for Y, w in zip(Ysts, want))
    e, e64 = float(np.max(np.abs(r - want) / want)), float(np.max(np.abs(r - want64) / want64))
    report(f"residual_batch {storage} H{H} {len(Ys)} ragged bags: stored={e:.2e} fp64_BHat={e64:.2e} max_YY_over_r2={ratio:.0f}")
    assert ratio > 100                                   # the regime the direct form is for
    assert e <= RESID_TOL, e
    assert e64 <= RESID_B64_TOL[storage], e64


def test_residual_on_a_sparse_context_equals_the_basic_one(pkg):
    H = 5
    B, Ys, As = _resid_case(H)
    r0 = pkg.residual_batch(Ys, _basic_sets(pkg, B, Ys, As))
    po, _ = _model("sparse", L, H, 605)
    po.BHat = B
    qg, _ = _sets(pkg, Ys, po, 7)
    for q, A in zip(qg, As):
        q.AHat = A
    r1 = pkg.residual_batch(Ys, qg)
    assert np.array_equal(r0, r1)


# ---- 2. bound against the oracle ---------------------------------------------------------------------------------------------
def _oracle_vbls(kind, Y, q, niter, full_cov):
    upA, upCA = {"sparse": (O.sparse_updateA, O.sparse_updateCA), "dual": (O.dual_updateA, O.dual_updateCA),
                 "trial": (O.trial_updateA, O.trial_updateCA)}[kind]
    for _ in range(niter):
        upA(Y, q, full_cov=full_cov)
        upCA(q)
        O.sparse_updateSigma(Y, q)


def _oracle_bound(kind, Y, q, trim=None):
    if trim is not None:
        return O.lowerBoundTrimmed(Y, q, trim)
    return {"sparse": O.lowerBound, "dual": O.lowerBound_dual, "trial": O.lowerBound_trial}[kind](Y, q)


@functools.lru_cache(maxsize=None)
def _bound_case(kind, H, full_cov, layout):
    """Oracle-trained model, bags, the oracle's vbls! state of every bag and its bounds; computed once and shared.  The bags are
    redrawn until no |ATVecHat| lies within 1e-5 of a trim value (the device compares in fp32)."""
    pkg = G.load_package()
    Ms = {"ragged": RAGGED, "small": SMALL, "small6": SMALL[:6]}[layout]
    po, draw = _model(kind, L, H, {"sparse": 2600, "dual": 2800, "trial": 2900}[kind] + H)
    niter = 3 if full_cov else 6
    for attempt in range(50):
        Ys = [_f32(draw(m)) for m in Ms]
        qg, qo = _sets(pkg, Ys, po, 4000 + 100 * attempt)
        for Y, q in zip(Ys, qo):
            _oracle_vbls(kind, Y, q, niter, full_cov)
        a = np.abs(np.concatenate([q.ATVecHat for q in qo]))
        if all(np.min(np.abs(a - t)) > 1e-5 for t in TRIMS):
            break
    else:
        raise AssertionError("no draw keeps |ATVecHat| away from the trim values")
    # the device gets the oracle's fp64 state, field by field
    P = type(qg[0])
    qg = [_convert(P, q) for q in qo]
    bounds = {None: np.array([_oracle_bound(kind, Y, q) for Y, q in zip(Ys, qo)])}
    for t in TRIMS:
        bounds[t] = np.array([_oracle_bound(kind, Y, q, t) for Y, q in zip(Ys, qo)])
    kept = {t: np.array([int(np.sum(np.abs(q.ATVecHat) > t)) for q in qo]) for t in TRIMS}
    return Ys, qo, qg, bounds, kept


BOUND_CASES = ([(k, H, False, "ragged") for k in ("sparse", "dual", "trial") for H in HS]
               + [("sparse", 2, True, "ragged"), ("sparse", 5, True, "ragged"), ("sparse", 20, True, "small"),
                  ("sparse", 64, True, "small6"), ("dual", 5, True, "ragged"), ("trial", 5, True, "ragged")])


@pytest.mark.parametrize("kind,H,full_cov,layout", BOUND_CASES)
def test_bound_against_the_oracle(pkg, kind, H, full_cov, layout):
    Ys, qo, qg, bounds, kept = _bound_case(kind, H, full_cov, layout)
    a = np.abs(np.concatenate([q.ATVecHat for q in qo]))
    for t in TRIMS:
        assert np.min(np.abs(a - t)) > 1e-5                          # the fp32 comparison cannot flip an entry
    # the mask must do something: in at least half the bags the kept count differs from M_b H
    full = np.array([q.M * H for q in qo])
    assert np.sum(kept[TRIMS[0]] != full) * 2 >= len(Ys), (kept[TRIMS[0]], full)
    bags = pkg.SparseBags(Ys, H)
    got = {None: pkg.lowerBound_batch(bags, qg)}
    for t in TRIMS:
        got[t] = pkg.lowerBoundTrimmed_batch(bags, qg, t)
    bags.close()
    errs = {t: float(np.max(np.abs(got[t] - bounds[t]) / np.abs(bounds[t]))) for t in got}
    scale = L * np.array([q.M for q in qo], dtype=np.float64)
    scaled = max(float(np.max(np.abs(got[t] - bounds[t]) / scale)) for t in got)
    report(f"lowerBound_batch {kind} H{H} full_cov={int(full_cov)} {len(Ys)} bags: "
           + " ".join(f"{'lb' if t is None else 'trim%g' % t}={e:.2e}" for t, e in errs.items()) + f" over_LM={scaled:.2e}")
    assert all(np.isfinite(v).all() for v in got.values())
    assert max(errs.values()) <= BOUND_TOL, errs
    assert scaled <= BOUND_SCALED_TOL, scaled
    # lowerBoundTrimmed is another number than lowerBound wherever the mask removed something
    cut = kept[TRIMS[0]] != full
    assert np.all(got[TRIMS[0]][cut] != got[None][cut])


# ---- 3. batched against per-bag device calls ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sparse", "dual", "trial"])
def test_batched_against_per_bag_device_calls(pkg, kind):
    """the states vbls_sparse_batch_ left, scored by the batched entry and by lowerBound / lowerBoundTrimmed per bag (a context,
    an upload and fp32 copies of the state per call).  Held to the bound of test_bound_against_the_oracle."""
    H, niter = 5, 20
    po, draw = _model(kind, L, H, 3100)
    Ys = [_f32(draw(m)) for m in RAGGED]
    qg, _ = _sets(pkg, Ys, po, 4100)
    bags = pkg.SparseBags(Ys, H)
    pkg.vbls_sparse_batch_(bags, qg, niter)
    got = {None: pkg.lowerBound_batch(bags, qg)}
    for t in TRIMS:
        got[t] = pkg.lowerBoundTrimmed_batch(bags, qg, t)
    bags.close()
    a = np.abs(np.concatenate([q.ATVecHat for q in qg]))
    safe = {t: np.min(np.abs(a - t)) > 1e-5 for t in TRIMS}
    errs = {}
    for t in got:
        if t is not None and not safe[t]:
            continue
        one = np.array([pkg.lowerBound(Y, q) if t is None else pkg.lowerBoundTrimmed(Y, q, t) for Y, q in zip(Ys, qg)])
        errs[t] = float(np.max(np.abs(got[t] - one) / np.abs(one)))
    pkg.invalidate()
    report(f"lowerBound_batch vs per-bag lowerBound {kind} H{H}: "
           + " ".join(f"{'lb' if t is None else 'trim%g' % t}={e:.2e}" for t, e in errs.items()))
    assert None in errs and len(errs) >= 2
    assert max(errs.values()) <= BOUND_TOL, errs


# ---- 4. segmentation ---------------------------------------------------------------------------------------------------------
def test_permuting_the_bags_permutes_the_outputs_bitwise(pkg):
    H = 5
    Ys, qo, qg, _, _ = _bound_case("sparse", H, False, "ragged")

    def score(idx):
        ys, qs = [Ys[i] for i in idx], [qg[i] for i in idx]
        bags = pkg.SparseBags(ys, H)
        out = (pkg.residual_batch(bags, qs), pkg.lowerBound_batch(bags, qs), pkg.lowerBoundTrimmed_batch(bags, qs, TRIMS[0]))
        bags.close()
        return out
    base = score(list(range(len(Ys))))
    perm = [int(i) for i in np.random.default_rng(21).permutation(len(Ys))]
    moved = score(perm)
    for a, b in zip(base, moved):
        assert np.array_equal(a[perm], b)
    for i in (0, 3, 9, len(Ys) - 1):                                  # 1-column, 70-column, 64-column, last
        alone = score([i])
        for a, b in zip(base, alone):
            assert a[i] == b[0], (i, a[i], b[0])


# ---- 5. classify_batch -------------------------------------------------------------------------------------------------------
def _two_bases(H, seed):
    rng = np.random.default_rng(seed)
    Bs = [rng.standard_normal((L, H)) * np.linspace(1.0, 2.5, H) for _ in range(2)]

    def draw(k, m):
        As = np.zeros((m, H)); As[np.arange(m), rng.integers(0, H, m)] = 1.0
        return Bs[k] @ As.T + 0.05 * rng.standard_normal((L, m))
    return draw


def _margin(e0, e1):
    return float(np.min(np.abs(e0 - e1) / np.maximum(np.abs(e0), np.abs(e1))))


def _moved_by(B, A, r, tolA):
    """|r(A + dA) - r(A)| <= ||B dA'||_F <= ||B||_2 ||dA||_F with ||dA||_F <= tolA ||A||_F, relative to r"""
    return float(np.linalg.norm(B, 2) * tolA * np.linalg.norm(A) / r)


def test_classify_vbls(pkg):
    H, niter = 5, 150
    draw = _two_bases(H, 5100)
    res = []
    for k in range(2):
        Ytr = draw(k, 300)
        po = O.vbmf_init(Ytr, H, ca=0.1, cb=0.1, sigma2=0.1, rng=np.random.default_rng(5110 + k), materialize_yhat=False)
        O.vbmf_(Ytr, po, 15, eps=0.0, est_covs=True, est_var=True)
        res.append(po)
    Ys = [_f32(draw(b % 2, m)) for b, m in enumerate(RAGGED)]
    errs, moved = [], 0.0
    for po in res:
        e = []
        for b, Y in enumerate(Ys):
            q = O.copy_vbmf_params(Y, po, rng=np.random.default_rng(b))
            O.vbls_(Y, q, niter)
            e.append(np.linalg.norm(Y - po.BHat @ q.AHat.T))
            # tests/test_gpu_vbls_batch.py holds the batched AHat to 3e-4 of the oracle's
            moved = max(moved, _moved_by(po.BHat, q.AHat, e[-1], 3e-4))
        errs.append(np.array(e))
    want = (errs[0] > errs[1]).astype(np.int64)
    margin = _margin(*errs)
    assert margin >= 100 * RESID_TOL and margin > 2 * moved, (margin, moved)
    labels, e0, e1 = pkg.classify_batch(to_pkg_params(pkg, res[0]), to_pkg_params(pkg, res[1]), Ys, "vbls")
    d = max(float(np.max(np.abs(e0 - errs[0]) / errs[0])), float(np.max(np.abs(e1 - errs[1]) / errs[1])))
    report(f"classify_batch vbls H{H} {len(Ys)} bags: err={d:.2e} bound={moved:.2e} margin={margin:.2e} ones={int(want.sum())}")
    assert 0 < want.sum() < len(Ys)
    assert np.array_equal(labels, want)
    assert d <= moved, (d, moved)


def test_classify_dual(pkg):
    H, niter = 5, 20
    draw = _two_bases(H, 5200)
    res = []
    for k in range(2):
        Ytr = draw(k, 200)
        po = O.vbmf_dual_init(Ytr, H, 2, rng=np.random.default_rng(5210 + k), materialize_yhat=False)
        O.vbmf_dual_(Ytr, po, 12, eps=0.0, est_priors=False)
        res.append(po)
    Ms = SMALL * 2                                                     # full_cov: the oracle inverts M_b H x M_b H
    Ys = [_f32(draw(b % 2, m)) for b, m in enumerate(Ms)]
    errs, moved = [], 0.0
    for po in res:
        _, qo = _sets(pkg, Ys, po, 5300)
        e = []
        for Y, q in zip(Ys, qo):
            _oracle_vbls("dual", Y, q, niter, True)
            r = np.linalg.norm(po.BHat @ q.AHat.T - Y)
            e.append(r / (L * Y.shape[1]))
            # tests/test_gpu_vbls_sparse_batch.py holds the batched full_cov ATVecHat to 5e-6 of the oracle's
            moved = max(moved, _moved_by(po.BHat, q.AHat, r, 5e-6))
        errs.append(np.array(e))
    want = np.where(errs[0] < errs[1], 0, 1)
    margin = _margin(*errs)
    assert margin >= 100 * RESID_TOL and margin > 2 * moved, (margin, moved)
    P = pkg.vbmf_dual_parameters
    labels, e0, e1 = pkg.classify_batch(_convert(P, res[0]), _convert(P, res[1]), Ys, "dual")
    d = max(float(np.max(np.abs(e0 - errs[0]) / errs[0])), float(np.max(np.abs(e1 - errs[1]) / errs[1])))
    report(f"classify_batch dual H{H} {len(Ys)} bags: err={d:.2e} bound={moved:.2e} margin={margin:.2e} ones={int(want.sum())}")
    assert 0 < want.sum() < len(Ys)
    assert np.array_equal(labels, want)
    assert d <= moved, (d, moved)


# the bound's terms are sums of the state's fields or of their logarithms, so its relative movement is at most the fields': the
# largest bound tests/test_gpu_vbls_sparse_batch.py puts on a full_cov field of the batched vbls! (CA, 2e-3)
CLASSIFY_BOUND_TOL = 2e-3


def test_classify_lower_bound(pkg):
    """factorize_bag + lowerBound / lowerBoundTrimmed per bag by the oracle against classify_batch.  Bags of even index use the first
    H - H1 columns of the trained basis only, the others its last H1.  At the reference's threshold 1e-1 the trimmed bound wins in
    every bag (trimming removes prior terms, whichever columns made the bag); at threshold 0 nothing is trimmed and both labels occur."""
    H, H1, niter = 5, 2, 8
    draw = _two_bases(H, 5400)
    Ytr = draw(0, 200)
    po = O.vbmf_sparse_init(Ytr, H, rng=np.random.default_rng(5410), full_cov=False, materialize_yhat=False)
    O.vbmf_sparse_(Ytr, po, 12, eps=0.0)
    po.H1 = H1
    H0 = H - H1
    rng = np.random.default_rng(5420)
    Ys = []
    for b, m in enumerate(SMALL * 2):                                  # full_cov: the oracle inverts M_b H x M_b H
        As = np.zeros((m, H)); As[np.arange(m), rng.integers(0, H0, m) if b % 2 == 0 else rng.integers(H0, H, m)] = 1.0
        Ys.append(_f32(po.BHat @ As.T + 0.05 * rng.standard_normal((L, m))))
    res = _convert(pkg.vbmf_sparse_parameters, po)
    fits = []
    for b, Y in enumerate(Ys):                                         # factorize_bag, examples/mil_util.jl:393-416
        p0 = O.vbmf_sparse_init(Y, H0, rng=np.random.default_rng(b), full_cov=False, materialize_yhat=False)
        p0.BHat, p0.SigmaB, p0.CB = po.BHat[:, :H0].copy(), po.SigmaB[:H0, :H0].copy(), po.CB[:H0].copy()
        p0.gamma, p0.delta = po.gamma, po.delta[:H0].copy()
        assert Y.shape[1] * H0 < 1600
        _oracle_vbls("sparse", Y, p0, niter, True)
        res1 = copy.copy(po); res1.H1 = 0
        p1 = O.copy_vbmf_params(Y, res1, rng=np.random.default_rng(b))
        _oracle_vbls("sparse", Y, p1, niter, True)
        fits.append((Y, p0, p1))
    L0 = np.array([O.lowerBound(Y, p0) for Y, p0, _ in fits])
    a = np.abs(np.concatenate([p1.ATVecHat for _, _, p1 in fits]))
    ones = {}
    for thr in (1e-1, 0.0):
        assert np.min(np.abs(a - thr)) > 1e-5
        L1 = np.array([O.lowerBoundTrimmed(Y, p1, thr) for Y, _, p1 in fits])
        want = (L1 > L0).astype(np.int64)
        margin = _margin(L0, L1)
        assert margin >= 100 * BOUND_TOL and margin > 2 * CLASSIFY_BOUND_TOL, margin
        labels, e0, e1 = pkg.classify_batch(res, None, Ys, "lower_bound", threshold=thr, niter=niter)
        d = max(float(np.max(np.abs(e0 - L0) / np.abs(L0))), float(np.max(np.abs(e1 - L1) / np.abs(L1))))
        ones[thr] = int(want.sum())
        report(f"classify_batch lower_bound H{H} H1={H1} threshold={thr:g} {len(Ys)} bags: err={d:.2e} margin={margin:.2e} "
               f"ones={ones[thr]}")
        assert np.array_equal(labels, want)
        assert d <= CLASSIFY_BOUND_TOL, d
    assert 0 < ones[0.0] < len(Ys)


# ---- 6. C ABI refusals -------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(pkg):
    C = pkg.capi
    VI = C.VBMF_ERR_INVALID
    M, H = 40, 4
    rng = np.random.default_rng(13)
    Y = rng.standard_normal((L, M))
    B = rng.standard_normal((L, H))
    off = np.array([0, 1, 17, 33, M], dtype=np.int64)
    nb = off.size - 1
    hyper = dict(alpha0=1e-3, beta0=1e-3, gamma0=1e-3, delta0=1e-3, eta0=1e-3, zeta0=1e-3)
    A = rng.standard_normal((M, H))
    ip = C.C.POINTER(C.C.c_int64)

    def bound(c, o=off, trim=None):
        n = len(o) - 1
        return c.sparse_lower_bound_batched(o, A.reshape(-1), np.full(M * H, 0.3), np.full(M * H, 0.7), np.full(M * H, 2.0),
                                            np.tile(np.eye(H) * 0.1, (n, 1, 1)), np.full(n, 3.0), np.full(n, 7.0), np.full(n, 40.0),
                                            np.full(n, 1e-3), np.full(n, 1e-3), np.full((n, H), 1e-3), np.full((n, H), 1e-3),
                                            np.full((n, H), 0.501), trim=trim)

    def refused(call):
        with pytest.raises(pkg.VbmfError) as e:
            call()
        assert e.value.code == VI, e.value
        return str(e.value)

    with C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32, variant=C.VBMF_VARIANT_SPARSE_DIAG) as c:
        c.set_Y(Y)
        c.sparse_set_state(A.reshape(-1), np.full(M * H, 0.3), np.full(M * H, 0.7), np.full(M * H, 2.0), B, 0.01 * np.eye(H),
                           np.ones(H), np.ones(H), 3.0, 7.0, hyper)
        before, lb0 = c.sparse_get_state(), c.sparse_lower_bound()
        r2 = c.bag_residuals(off, A)
        lbs, r2b = bound(c)
        assert np.array_equal(r2, r2b) and np.isfinite(lbs).all()
        for bad in ([0, 1, 1, M], [1, 17, M], [0, 17, M - 1], [0, 20, 10, M], [0, M + 1]):
            o = np.array(bad, dtype=np.int64)
            refused(lambda: c.bag_residuals(o, A))
            refused(lambda: bound(c, o=o))
        assert C.lib().vbmf_bag_residuals(c._h, nb, off.ctypes.data_as(ip), None, M, None) == VI
        assert C.lib().vbmf_bag_residuals(c._h, nb, None, None, M, None) == VI
        assert C.lib().vbmf_sparse_lower_bound_batched(c._h, nb, off.ctypes.data_as(ip), 1, -1.0, 0, *([None] * 15)) == VI
        # a non-finite sum: VBMF_ERR_NUMERIC naming the bag; the next call is clean
        An = A.copy(); An[20, 1] = np.nan
        with pytest.raises(pkg.VbmfError) as e:
            c.bag_residuals(off, An)
        assert e.value.code == C.VBMF_ERR_NUMERIC and "bag 2" in str(e.value)
        assert np.array_equal(c.bag_residuals(off, A), r2)
        # neither entry touched the state
        after = c.sparse_get_state()
        for k, v in before.items():
            assert np.array_equal(np.asarray(v), np.asarray(after[k])), k
        assert c.sparse_lower_bound() == lb0
    with C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32) as c:
        assert "basic" in refused(lambda: bound(c))
    for v in (C.VBMF_VARIANT_SPARSE_DIAGVAR, C.VBMF_VARIANT_DUAL_DIAGVAR, C.VBMF_VARIANT_TRIAL_DIAGVAR):
        with C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32, variant=v) as c:
            assert "diag_var" in refused(lambda: bound(c))
            assert "diag_var" in refused(lambda: c.bag_residuals(off, A))
    with C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32, nranks=2, rank=0, L_global=2 * L, variant=C.VBMF_VARIANT_SPARSE_DIAG) as c:
        assert "rank" in refused(lambda: bound(c))
        assert "rank" in refused(lambda: c.bag_residuals(off, A))
