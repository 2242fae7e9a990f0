"""Many three-group / label-masked sparse fits in one launch (vbmf_local_fit_batched, vbmf_trial_batch_, vbmf_sparse_masked_batch_,
train_local_folds): every fit's whole vbmf_trial! / masked vbmf_sparse! loop on a concatenated matrix [Y0 Y1] in one workgroup, against
the oracle's loop on Y as stored (get_Y) from the same start values -- field by field, sweep counts and the trace of d included -- plus
the independence of the fits from each other and the C ABI's refusals.  "trial" = the three-group model (src/vbmf_trial.jl), "masked" =
vbmf_sparse! with labels = 1:M0 and H1 (examples/mil_util.jl:302-320)."""
import copy
import dataclasses
import os

import numpy as np
import pytest

import __graft_entry__ as G
from oracle import vbmf_oracle as O

pytestmark = pytest.mark.gpu

# Largest relative error per field against the oracle measured on an MI355X over every case of this file
# (profiles/fit_local_batch_parity.txt).  Asserted: 3 x the figure, at least FLOOR, and never above CAP -- the cap is a condition, not a
# measurement: an fp32 intermediate shows up at 1e-7 and must fail.
# Every figure of the table comes from ONE case, the three-group fits of the diagonal form with eight fixed sweeps (test 1).  Among its
# bags is (M, M0) = (64, 64) with H0 = 1: the second and third factor carry no signal (M0 = M), so eight sweeps end in the middle of their
# pruning, where the hyper-prior fit of group 2 amplifies a rounding -- on that bag the oracle itself moves by 1.5e-11 in CB when ONE start
# value's last bit changes (2e-16 into BHat), 40 times more than on any other bag of the case.  Every other case of the file stays below
# 8e-12 in d and trace_d and below 3e-13 in every other field, the sibling file's order.
MEASURED = dict(BHat=4.08e-10, SigmaB=3.65e-10, CB=7.97e-10, delta=5.64e-10, sigmaHat=4.31e-11, zeta=4.31e-11, CA=1.38e-10, beta=1.23e-09,
                diagSigmaATVec=8.26e-10, ATVecHat=5.61e-10, SigmaA=8.34e-10, priors=2.04e-10, shapes=1.11e-11, d=1.55e-10, trace_d=1.55e-10)
FLOOR, CAP, FACTOR = 1e-12, 1e-8, 3.0
TOL = {k: max(FACTOR * v, FLOOR) for k, v in MEASURED.items()}
assert all(v <= CAP for v in TOL.values())

FIELDS = ("BHat", "SigmaB", "CB", "delta", "sigmaHat", "zeta", "CA", "beta", "diagSigmaATVec", "ATVecHat", "SigmaA")
PAIRS = ("alpha01", "beta01", "alpha02", "beta02", "alpha03", "beta03")
SHAPES = ("alpha1", "alpha2", "alpha3")
KINDS = ("trial", "masked")
REPORT = os.path.join(G.ROOT, "build", "fit_local_batch_parity.txt")     # (build/ is not tracked)
_worst = {}


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


@pytest.fixture(scope="module", autouse=True)
def _report_file():
    """one report per session: started empty, closed with the largest figure per field (what MEASURED is taken from)"""
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    open(REPORT, "w").close()
    _worst.clear()
    yield
    with open(REPORT, "a") as fh:
        fh.write("worst: " + " ".join(f"{k}={v:.2e}" for k, v in sorted(_worst.items())) + "\n")


def _f32(Y):
    return Y.astype(np.float32).astype(np.float64)


def _two_class(L, M, M0, H, H0, s):
    """[Y0 Y1]: a rank-H matrix plus 10 % noise whose first M0 columns (the negative instances) do not use the last H - H0 factors"""
    rng = np.random.default_rng(2000 + s)
    B = rng.standard_normal((L, H))
    A = rng.standard_normal((M, H))
    A[:M0, H0:] = 0.0
    return _f32(B @ A.T + 0.1 * rng.standard_normal((L, M)))


def _start(kind, Y, H, Hx, M0, seed):
    """the oracle's init with default_rng(seed): the start values of both sides.  Hx: H0 of the three-group, H1 of the masked model"""
    rng = np.random.default_rng(seed)
    if kind == "trial":
        return O.vbmf_trial_init(Y, H, Hx, M0, rng=rng, materialize_yhat=False)
    return O.vbmf_sparse_init(Y, H, H1=Hx, labels=np.arange(M0), rng=rng, full_cov=False, materialize_yhat=False)


def _m0(p):
    return int(p.M0) if hasattr(p, "M0") else int(np.size(p.labels))


def _oracle(kind, Y, p0, niter, eps, full_cov, compat=True, est_cb=True, est_priors=True):
    p = copy.deepcopy(p0)
    tr = []
    if kind == "trial":
        d, it = O.vbmf_trial_(Y, p, niter, eps=eps, full_cov=full_cov, reference_compat=compat, trace=tr, est_cb=est_cb,
                              est_priors=est_priors)
    else:
        d, it = O.vbmf_sparse_(Y, p, niter, eps=eps, full_cov=full_cov, reference_compat=compat, trace=tr, est_cb=est_cb)
    return p, d, it, np.array([t[0] for t in tr])


class Call:
    """bags side by side in one context (fp32 storage), Y as stored per bag"""

    def __init__(self, pkg, Ys, H, kind, compat=None, variant=None):
        C = pkg.capi
        self.C, self.H, self.kind = C, H, kind
        self.off = np.concatenate([[0], np.cumsum([Y.shape[1] for Y in Ys])]).astype(np.int64)
        L, M = Ys[0].shape[0], int(self.off[-1])
        kw = {} if compat is None else dict(reference_compat=compat)
        if variant is None:
            variant = C.VBMF_VARIANT_TRIAL_DIAG if kind == "trial" else C.VBMF_VARIANT_SPARSE_DIAG
        self.ctx = C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32, **kw, variant=variant)
        self.ctx.set_Y(np.concatenate(Ys, axis=1))
        Yall = self.ctx.get_Y()
        self.Ys = [np.ascontiguousarray(Yall[:, a:b]) for a, b in zip(self.off[:-1], self.off[1:])]

    def run(self, starts, bag_of, niter, eps, full_cov, est_cb=True, est_priors=True, pri=None, H0=None):
        """starts: the oracle's parameter sets; returns the library's dict"""
        trial = self.kind == "trial"
        if pri is None:
            pri = [[getattr(p, k) for k in PAIRS] if trial else [p.alpha0, p.beta0] * 3 for p in starts]
        if H0 is None:
            H0 = starts[0].H0 if trial else self.H
        return self.ctx.local_fit_batched(
            self.off, bag_of, niter, eps, [p.gamma for p in starts], [p.delta0 for p in starts], [p.eta for p in starts],
            [p.zeta0 for p in starts], pri, np.stack([p.BHat for p in starts]), np.stack([p.SigmaB for p in starts]),
            np.stack([p.CB for p in starts]), [p.sigmaHat for p in starts], np.concatenate([p.CA for p in starts]),
            [_m0(p) for p in starts], H0=H0, mask_H1=0 if trial else starts[0].H1, full_cov=full_cov, est_cb=est_cb,
            est_priors=trial and est_priors, want_trace=True)

    def close(self):
        self.ctx.close()


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


def _fit_fields(r, f, s0, s1):
    delta = {} if r["delta"] is None else dict(delta=r["delta"][f])                # (not written without est_cb)
    return dict(BHat=r["BHat"][f], SigmaB=r["SigmaB"][f], CB=r["CB"][f], **delta, sigmaHat=r["sigmaHat"][f],
                zeta=r["zeta"][f], CA=r["CA"][s0:s1], beta=r["beta"][s0:s1], diagSigmaATVec=r["diagSigmaATVec"][s0:s1],
                ATVecHat=r["ATVecHat"][s0:s1], SigmaA=r["SigmaA"][f])


def _compare(tag, call, r, starts, bag_of, niter, eps, full_cov, compat=True, oracle=_oracle):
    """every fit of the call against the oracle: the fields, the priors, the sweep count, the trace of d; returns the worst errors"""
    H, worst, s0 = call.H, {}, 0
    for f, (p0, b) in enumerate(zip(starts, bag_of)):
        po, d, it, trd = oracle(call.kind, call.Ys[b], p0, niter, eps, full_cov, compat)
        s1 = s0 + po.M * H
        e = {k: _rel(v, getattr(po, k)) for k, v in _fit_fields(r, f, s0, s1).items()}
        if call.kind == "trial":
            e["priors"] = _rel(r["priors9"][f, :6], [getattr(po, k) for k in PAIRS])
            e["shapes"] = _rel(r["priors9"][f, 6:], [getattr(po, k) for k in SHAPES])
        else:
            assert np.array_equal(r["priors9"][f, :6], [po.alpha0, po.beta0] * 3), (tag, f)    # no hyper-prior fit in this model
            e["shapes"] = _rel(r["priors9"][f, 6:], [po.alpha] * 3)
            M0, H1 = _m0(po), int(po.H1)
            if H1 > 0:                                              # the masked block is exactly zero, not merely small
                assert np.all(r["ATVecHat"][s0:s1].reshape(po.M, H)[:M0, H - H1:] == 0.0), (tag, f)
        assert r["iters"][f] == it, (tag, f, int(r["iters"][f]), it, r["trace"][f, :, 0], trd)
        assert r["status"][f] == 0, (tag, f)
        e["d"] = _rel(r["d"][f], d)
        e["trace_d"] = float(np.max(np.abs(r["trace"][f, :it, 0] - trd) / np.abs(trd)))
        assert np.all(r["trace"][f, it:] == 0.0)
        for k, v in e.items():
            worst[k] = max(worst.get(k, 0.0), v)
        s0 = s1
    _record(tag, worst)
    return worst


def _record(tag, worst):
    """prints and files the figures of one case, then asserts them"""
    line = f"{tag}: " + " ".join(f"{k}={v:.2e}" for k, v in worst.items())
    print(line)
    with open(REPORT, "a") as fh:
        fh.write(line + "\n")
    for k, v in worst.items():
        _worst[k] = max(_worst.get(k, 0.0), v)
    bad = {k: (v, TOL[k]) for k, v in worst.items() if not v <= TOL[k]}
    assert not bad, (tag, bad)


def _hx(kind, H, H0):
    """the model's own split parameter for data whose last H - H0 factors the first M0 columns do not use"""
    return H0 if kind == "trial" else H - H0


# ---- 1. the diagonal form, fixed sweeps ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("repeat", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_diagonal_fixed_sweeps(pkg, kind, repeat):
    L, H, H0, bags = 24, 3, 1, ((37, 20), (2, 1), (9, 0), (64, 64), (9, 4))
    C = pkg.capi
    call = Call(pkg, [_two_class(L, m, m0, H, H0, 10 + i) for i, (m, m0) in enumerate(bags)], H, kind,
                compat=None if repeat else C.VBMF_COMPAT_SPECTRAL_DELTA)
    try:
        bag_of = [b for b in range(len(bags)) for _ in range(3)]
        starts = [_start(kind, call.Ys[b], H, _hx(kind, H, H0), bags[b][1], 10 * b + k) for b in range(len(bags)) for k in range(3)]
        r = call.run(starts, bag_of, 8, 0.0, False)
        _compare(f"diag {kind} repeat={int(repeat)}", call, r, starts, bag_of, 8, 0.0, False, compat=repeat)
        assert np.all(r["iters"] == 8)
        if kind == "masked":                                        # H1 = 2: the last two columns of the first M0 rows
            s0 = 0
            for b in bag_of:
                m, m0 = bags[b]
                assert np.all(r["ATVecHat"][s0:s0 + m * H].reshape(m, H)[:m0, 1:] == 0.0)
                assert np.all(r["ATVecHat"][s0:s0 + m * H].reshape(m, H)[m0:, :] != 0.0)
                s0 += m * H
    finally:
        call.close()


# ---- 2. the stop test, full_cov -------------------------------------------------------------------------------------------------------
STOP_EPS, STOP_NITER = 1e-3, 30
# (L, M, M0, H, H0); the masked model runs the same (L, M, M0, H) with the H1 of STOP_H1
STOP_SHAPES = ((24, 37, 20, 3, 1), (166, 64, 40, 5, 3), (7, 30, 11, 2, 1), (24, 37, 0, 3, 1), (24, 37, 37, 3, 1), (24, 37, 20, 3, 3),
               (530, 12, 5, 2, 1), (50, 2, 1, 2, 1))
STOP_H1 = (2, 2, 1, 2, 2, 3, 1, 1)
# six starts per shape: seeds 0..5, except those of which some sweep's d lies within 1 % of eps on the oracle -- they are replaced by
# the next seeds that keep the margin (the test asserts the margin on the oracle alone, before the device call)
# (three-group: seed 1 of the first shape, seeds 3 and 5 of (7, 30, 11, 2, 1); masked, on the same matrices: none)
STOP_SEEDS = {("trial", 0): (0, 6, 2, 3, 4, 5), ("trial", 2): (0, 1, 2, 6, 4, 7)}


@pytest.mark.parametrize("kind", KINDS)
def test_stop_test_full_cov(pkg, kind):
    for si, (L, M, M0, H, H0) in enumerate(STOP_SHAPES):
        Hx = H0 if kind == "trial" else STOP_H1[si]
        call = Call(pkg, [_two_class(L, M, M0, H, H0, si)], H, kind)
        try:
            starts = [_start(kind, call.Ys[0], H, Hx, M0, s) for s in STOP_SEEDS.get((kind, si), (0, 1, 2, 3, 4, 5))]
            for p0 in starts:                                       # the margin, on the oracle alone
                trd = _oracle(kind, call.Ys[0], p0, STOP_NITER, STOP_EPS, True)[3]
                assert np.all(np.abs(trd - STOP_EPS) > 0.01 * STOP_EPS), (kind, si, trd)
            r = call.run(starts, [0] * 6, STOP_NITER, STOP_EPS, True)
            _compare(f"stop {kind} {(L, M, M0, H, Hx)}", call, r, starts, [0] * 6, STOP_NITER, STOP_EPS, True)
        finally:
            call.close()


# ---- 3. the tier edges (NBK = 1 against NBK = 2) ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,full_cov,niter", [((40, 21, 9, 16, 8), True, 6), ((33, 20, 9, 17, 8), True, 6), ((33, 20, 9, 17, 8), False, 3)])
def test_tier_edges(pkg, kind, shape, full_cov, niter):
    L, M, M0, H, H0 = shape
    call = Call(pkg, [_two_class(L, M, M0, H, H0, 40 + H)], H, kind)
    try:
        starts = [_start(kind, call.Ys[0], H, _hx(kind, H, H0), M0, s) for s in (0, 1)]
        r = call.run(starts, [0, 0], niter, 0.0, full_cov)
        _compare(f"tier {kind} {shape} full={int(full_cov)}", call, r, starts, [0, 0], niter, 0.0, full_cov)
    finally:
        call.close()


# ---- 4. state in global memory beside state in LDS -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_global_state_beside_lds_state(pkg, kind):
    L, H, H0, bags = 12, 3, 1, ((2500, 1200), (5, 2))
    call = Call(pkg, [_two_class(L, m, m0, H, H0, 50 + i) for i, (m, m0) in enumerate(bags)], H, kind)
    try:
        bag_of = [0, 1, 0, 1]
        starts = [_start(kind, call.Ys[b], H, _hx(kind, H, H0), bags[b][1], 3 + k) for k, b in enumerate(bag_of)]
        r = call.run(starts, bag_of, 4, 0.0, False)
        _compare(f"global+lds {kind}", call, r, starts, bag_of, 4, 0.0, False)
    finally:
        call.close()


# ---- 5. independence ------------------------------------------------------------------------------------------------------------------------
def _same(r, f, s, q, g, t):
    """fit f of call r (its M H-long fields at s) equals fit g of call q (at t), bit for bit"""
    for k in ("BHat", "SigmaB", "CB", "delta", "sigmaHat", "zeta", "SigmaA", "priors9", "iters", "d", "status", "trace"):
        assert np.array_equal(r[k][f], q[k][g], equal_nan=True), k
    for k in ("CA", "beta", "diagSigmaATVec", "ATVecHat"):
        assert np.array_equal(r[k][s], q[k][t], equal_nan=True), k


@pytest.mark.parametrize("full_cov", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_independence(pkg, kind, full_cov):
    L, H, H0, Ms = 24, 3, 1, (37, 2, 9, 64)
    Hx = _hx(kind, H, H0)
    call = Call(pkg, [_two_class(L, m, m // 2, H, H0, 60 + i) for i, m in enumerate(Ms)], H, kind)
    try:
        me = _start(kind, call.Ys[0], H, Hx, 20, 77)
        ob = [1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3]
        om0 = [1, 0, 64, 5, 2, 9, 31, 37, 0, 4, 0]                 # the others differ from it in M0, on its own bag too
        others = [_start(kind, call.Ys[b], H, Hx, m0, 100 + k) for k, (b, m0) in enumerate(zip(ob, om0))]
        n = Ms[0] * H
        alone = call.run([me], [0], 8, 1e-3, full_cov)
        first = call.run([me] + others, [0] + ob, 8, 1e-3, full_cov)
        last = call.run(others + [me], ob + [0], 8, 1e-3, full_cov)
        twice = call.run([me, others[0], me], [0, 1, 0], 8, 1e-3, full_cov)
        _same(alone, 0, slice(0, n), first, 0, slice(0, n))
        tot = len(last["CA"])
        _same(alone, 0, slice(0, n), last, 11, slice(tot - n, tot))
        _same(alone, 0, slice(0, n), twice, 0, slice(0, n))
        tot = len(twice["CA"])
        _same(alone, 0, slice(0, n), twice, 2, slice(tot - n, tot))
    finally:
        call.close()


# ---- 6. without est_cb and est_priors ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_without_est_cb_and_est_priors(pkg, kind):
    L, H, H0, bags = 24, 3, 1, ((37, 20), (9, 4))
    call = Call(pkg, [_two_class(L, m, m0, H, H0, 70 + i) for i, (m, m0) in enumerate(bags)], H, kind)
    try:
        bag_of = [0, 1, 0]
        starts = [_start(kind, call.Ys[b], H, _hx(kind, H, H0), bags[b][1], 30 + k) for k, b in enumerate(bag_of)]
        r = call.run(starts, bag_of, 8, 0.0, False, est_cb=False, est_priors=False)
        fixed = lambda *a: _oracle(*a, est_cb=False, est_priors=False)
        _compare(f"est_cb=0 est_priors=0 {kind}", call, r, starts, bag_of, 8, 0.0, False, oracle=fixed)
        for f, p0 in enumerate(starts):                             # neither CB nor the hyper-priors moved
            assert np.array_equal(r["CB"][f], p0.CB)
            want = [getattr(p0, k) for k in PAIRS] if kind == "trial" else [p0.alpha0, p0.beta0] * 3
            assert np.array_equal(r["priors9"][f, :6], want)
    finally:
        call.close()


# ---- 7. the three-group sweep with M0 = M_b, H0 = H is the two-group sweep with H0 = H ------------------------------------------------------
@pytest.mark.parametrize("full_cov", [False, True])
def test_one_group_matches_the_two_group_oracle(pkg, full_cov):
    L, H, Ms = 24, 3, (37, 9)
    call = Call(pkg, [_two_class(L, m, m, H, H, 80 + i) for i, m in enumerate(Ms)], H, "trial", variant=pkg.capi.VBMF_VARIANT_DUAL_DIAG)
    try:
        bag_of = [0, 1, 0]
        starts = [O.vbmf_dual_init(call.Ys[b], H, H, rng=np.random.default_rng(90 + k), materialize_yhat=False) for k, b in enumerate(bag_of)]
        for p in starts:
            p.M0 = p.M
        spare = [0.3, 0.7, 1.5, 2.5]                                # the pairs of the two empty groups
        r = call.run(starts, bag_of, 8, 0.0, full_cov, pri=[[p.alpha00, p.beta00] + spare for p in starts], H0=H)
        worst, s0 = {}, 0
        for f, (p0, b) in enumerate(zip(starts, bag_of)):
            po = copy.deepcopy(p0)
            d, it = O.vbmf_dual_(call.Ys[b], po, 8, eps=0.0, full_cov=full_cov)
            s1 = s0 + po.M * H
            e = {k: _rel(v, getattr(po, k)) for k, v in _fit_fields(r, f, s0, s1).items()}
            e["priors"] = _rel(r["priors9"][f, :2], [po.alpha00, po.beta00])
            e["shapes"] = _rel(r["priors9"][f, 6], po.alpha0)
            e["d"] = _rel(r["d"][f], d)
            assert r["iters"][f] == it == 8 and r["status"][f] == 0
            assert np.array_equal(r["priors9"][f, 2:6], spare)      # the untouched pairs come back as given
            assert np.array_equal(r["priors9"][f, 7:], [0.3 + 0.5, 1.5 + 0.5])
            for k, v in e.items():
                worst[k] = max(worst.get(k, 0.0), v)
            s0 = s1
        _record(f"one group full={int(full_cov)}", worst)
    finally:
        call.close()


# ---- 8. a fit that meets a non-finite precision --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full_cov", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_status_of_a_fit_that_meets_a_non_finite_precision(pkg, kind, full_cov):
    """a NaN noise precision in one fit: status 1 after its first sweep, the call succeeds, the neighbours are what they are without it"""
    L, H, H0, bags = 24, 3, 1, ((37, 20), (9, 4))
    Hx = _hx(kind, H, H0)
    call = Call(pkg, [_two_class(L, m, m0, H, H0, 70 + i) for i, (m, m0) in enumerate(bags)], H, kind)
    try:
        good = [_start(kind, call.Ys[b], H, Hx, bags[b][1], 40 + b) for b in (0, 1)]
        sick = _start(kind, call.Ys[0], H, Hx, 11, 42)
        sick.sigmaHat = float("nan")
        r = call.run([good[0], sick, good[1]], [0, 0, 1], 8, 1e-3, full_cov)
        q = call.run(good, [0, 1], 8, 1e-3, full_cov)
        assert list(r["status"]) == [0, 1, 0] and r["iters"][1] == 1
        n0, n1 = bags[0][0] * H, bags[1][0] * H
        _same(r, 0, slice(0, n0), q, 0, slice(0, n0))
        _same(r, 2, slice(2 * n0, 2 * n0 + n1), q, 1, slice(n0, n0 + n1))
    finally:
        call.close()


# ---- 9. the refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg):
    C = pkg.capi
    VI, VU = C.VBMF_ERR_INVALID, C.VBMF_ERR_UNSUPPORTED
    L, M, H = 24, 20, 3
    Y = _two_class(L, M, 8, H, 1, 9)
    off = np.array([0, 1, 12, M], dtype=np.int64)                   # bags of 1, 11 and 8 columns
    hyper = dict(alpha0=1e-3, beta0=1e-3, gamma0=1e-3, delta0=1e-3, eta0=1e-3, zeta0=1e-3)
    rng = np.random.default_rng(3)

    def state(c, h=H, **kw):
        c.sparse_set_state(rng.standard_normal(M * h), np.ones(M * h), np.ones(M * h), np.ones(M * h), rng.standard_normal((L, h)),
                           0.01 * np.eye(h), np.ones(h), np.ones(h), 1.0, 0.5, hyper, **kw)

    def run(c, o=off, fit_bag=(1, 2), niter=5, h=H, H0=1, M0=(4, 8), mask_H1=0, full_cov=False, est_priors=False):
        nf, fb = len(fit_bag), np.asarray(fit_bag, dtype=np.int64)
        w = np.diff(np.asarray(o))
        mh = int(sum(w[b] for b in fb if 0 <= b < len(w))) * h
        return c.local_fit_batched(o, fb, niter, 1e-3, np.full(nf, 12.0), np.full(nf, 1e-3), np.full(nf, 100.0), np.full(nf, 1e-3),
                                   np.full((nf, 9), 1e-3), rng.standard_normal((nf, L, h)), np.zeros((nf, h, h)), np.ones((nf, h)),
                                   np.ones(nf), np.ones(mh), M0, H0=H0, mask_H1=mask_H1, full_cov=full_cov, est_priors=est_priors)

    def refused(c, code=VI, get=None, **kw):
        get = get or c.sparse_get_state
        before = get()
        with pytest.raises(pkg.VbmfError) as e:
            run(c, **kw)
        assert e.value.code == code, e.value
        after = get()
        for k, v in before.items():
            assert np.array_equal(v, after[k]), k
        return str(e.value)

    for v in (C.VBMF_VARIANT_SPARSE_DIAG, C.VBMF_VARIANT_DUAL_DIAG, C.VBMF_VARIANT_TRIAL_DIAG):
        with C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32, variant=v) as c:
            state(c)
            assert "no Y" in refused(c)                             # nothing uploaded yet
            c.set_Y(Y)
            before = c.sparse_get_state()
            assert np.all(run(c, est_priors=True)["iters"] >= 1)    # the call itself is fine on every *_DIAG context ...
            assert np.all(run(c, H0=H, mask_H1=2)["iters"] >= 1)
            after = c.sparse_get_state()
            assert all(np.array_equal(v, after[k]) for k, v in before.items())   # ... and leaves its state alone
    with C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32, variant=C.VBMF_VARIANT_TRIAL_DIAG) as c:
        c.set_Y(Y)
        state(c)
        for bad in ([0, 1, 1, M], [1, 12, M], [0, 12, M - 1], [0, 15, 10, M], [0, M + 1]):
            refused(c, o=np.array(bad, dtype=np.int64), fit_bag=(0,), M0=(0,), full_cov=True)
        # (Context.local_fit_batched checks fit_bag itself: the C entry is asked directly)
        p64, dp = (lambda a: a.ctypes.data_as(C.C.POINTER(C.C.c_int64))), C._dptr
        one, st, it = np.ones(64), np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int64)
        m0 = np.array([4, 8], dtype=np.int64)

        def raw(fit_bag, nfits=2, null=False, null_m0=False):
            fb = np.asarray(fit_bag, dtype=np.int64)
            before = c.sparse_get_state()
            rc = C.lib().vbmf_local_fit_batched(c._h, 3, p64(off), nfits, p64(fb), 5, 1e-3, 1, 1, 0, 1, None if null_m0 else p64(m0), 0,
                                                dp(one), dp(one), dp(one), dp(one), dp(one), None if null else dp(np.ones(2 * L * H)),
                                                dp(np.ones(2 * H * H)), dp(one), dp(one), dp(np.ones(2 * M * H)), None, None, None, None,
                                                None, None, p64(it), dp(one), p64(st), None)
            after = c.sparse_get_state()
            assert all(np.array_equal(v, after[k]) for k, v in before.items())
            return rc
        assert raw([1, 2]) == C.VBMF_OK
        assert raw([0, 3]) == VI and raw([-1, 0]) == VI             # fit_bag outside 0..nbags-1
        assert raw([1, 2], nfits=0) == VI
        assert raw([1, 2], null=True) == VI and raw([1, 2], null_m0=True) == VI   # a required pointer that is NULL
        refused(c, niter=0)
        assert "H0" in refused(c, H0=-1)
        assert "H0" in refused(c, H0=H + 1)
        assert np.all(run(c, H0=0)["iters"] >= 1) and np.all(run(c, H0=H)["iters"] >= 1)     # both ends are models
        assert "M0" in refused(c, M0=(-1, 8))
        assert "M0" in refused(c, M0=(4, 9))                        # bag 2 has 8 columns
        assert np.all(run(c, M0=(0, 8))["iters"] >= 1)
        assert "mask_H1" in refused(c, H0=H, mask_H1=-1)
        assert "mask_H1" in refused(c, H0=H, mask_H1=H + 1)
        assert "mask_H1" in refused(c, H0=1, mask_H1=1)             # the masked model has one prior group ...
        assert "mask_H1" in refused(c, H0=H, mask_H1=1, est_priors=True)   # ... and no hyper-prior fit
        assert np.all(run(c, H0=H, mask_H1=H)["iters"] >= 1)
        assert "1-column" in refused(c, fit_bag=(0, 1), M0=(1, 4))  # the diagonal form under the repeat layout needs M >= 2 ...
        assert np.all(run(c, fit_bag=(0, 1), M0=(1, 4), full_cov=True)["iters"] >= 1)   # ... full_cov does not
    with C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32, variant=C.VBMF_VARIANT_SPARSE_DIAG) as c:   # (only the sparse model takes a mask)
        c.set_Y(Y)
        state(c, labels0=[0, 5], H1=1)
        assert "mask" in refused(c)
    with C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32) as c:
        c.set_Y(Y)
        c.set_state(np.ones((M, H)), np.ones((L, H)), np.eye(H), np.eye(H), np.ones(H), np.ones(H), 1.0)
        assert "basic" in refused(c, get=c.get_state)
    for v in (C.VBMF_VARIANT_SPARSE_DIAGVAR, C.VBMF_VARIANT_DUAL_DIAGVAR, C.VBMF_VARIANT_TRIAL_DIAGVAR):
        with C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32, variant=v) as c:
            state(c)
            assert "diag_var" in refused(c)
    with C.Context(L, M, 33, y_dtype=pkg.VBMF_Y_F32, variant=C.VBMF_VARIANT_TRIAL_DIAG) as c:
        state(c, h=33)
        assert "32" in refused(c, code=VU, h=33)
    with C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32, nranks=2, rank=0, L_global=2 * L, variant=C.VBMF_VARIANT_TRIAL_DIAG) as c:
        state(c)
        assert "rank" in refused(c)


# ---- 10. the Python hosts ----------------------------------------------------------------------------------------------------------------------
def _convert(cls, src):
    dst = cls()
    for f in dataclasses.fields(cls):
        if hasattr(src, f.name):
            setattr(dst, f.name, copy.deepcopy(getattr(src, f.name)))
    return dst


@pytest.mark.parametrize("kind", KINDS)
def test_python_host_fills_what_the_per_fit_call_fills(pkg, kind):
    """vbmf_trial_batch_ / vbmf_sparse_masked_batch_ on package parameter sets: the fields of every set against the oracle (fp32 storage)"""
    L, H, H0, bags = 24, 3, 1, ((9, 4), (37, 20))
    Ys = [_two_class(L, m, m0, H, H0, 10 + i) for i, (m, m0) in enumerate(bags)]
    bag_of, m0s = [0, 1, 1], [4, 20, 0]
    starts = [_start(kind, Ys[b], H, _hx(kind, H, H0), m0, 60 + k) for k, (b, m0) in enumerate(zip(bag_of, m0s))]
    if kind == "trial":
        ps = [_convert(pkg.vbmf_trial_parameters, s) for s in starts]
        ds = pkg.vbmf_trial_batch_(Ys, ps, 8, eps=0.0, full_cov=False, bag_of=bag_of)
        names = FIELDS + PAIRS + SHAPES + ("A1Hat", "A2Hat", "A3Hat", "CA1", "CA2", "CA3", "beta1", "beta2", "beta3")
    else:
        ps = [_convert(pkg.vbmf_sparse_parameters, s) for s in starts]
        for p in ps:
            p.labels = p.labels + 1                                 # the package's labels are 1-based, like the reference's
        ds = pkg.vbmf_sparse_masked_batch_(Ys, ps, 8, eps=0.0, full_cov=False, bag_of=bag_of)
        names = FIELDS
    key = lambda k: (k if k in TOL else "shapes" if k in SHAPES else "priors" if k in PAIRS else
                     "CA" if k.startswith("CA") else "beta" if k.startswith("beta") else "ATVecHat")
    worst = {}
    for p, s, b, d, m0 in zip(ps, starts, bag_of, ds, m0s):
        po, do, it, _ = _oracle(kind, Ys[b], s, 8, 0.0, False)
        assert p.iters == it == 8 and p.status == 0
        worst["d"] = max(worst.get("d", 0.0), abs(d - do) / abs(do))
        for k in names + ("AHat",):
            worst[key(k)] = max(worst.get(key(k), 0.0), _rel(getattr(p, k), getattr(po, k)))
        if kind == "trial":
            assert np.array_equal(p.alpha, [p.alpha1, p.alpha2, p.alpha3])
        else:
            assert np.all(p.AHat[:m0, 1:] == 0.0)
    _record(f"python host {kind}", worst)


def test_train_local_folds_runs_on_the_device(pkg):
    L, H, H1 = 24, 3, 2
    folds = []
    for i, (m, m0) in enumerate(((37, 20), (9, 4))):
        Y = _two_class(L, m, m0, H, H - H1, 10 + i)
        folds.append((Y[:, :m0], Y[:, m0:]))
    ps = pkg.train_local_folds(folds, H, H1, 30, eps=1e-3, rng=np.random.default_rng(1))
    assert len(ps) == 2
    for p, (Y0, Y1) in zip(ps, folds):
        m0 = Y0.shape[1]
        assert isinstance(p, pkg.vbmf_sparse_parameters) and p.status == 0 and 1 <= p.iters <= 30
        assert p.M == m0 + Y1.shape[1] and np.array_equal(p.labels, np.arange(1, m0 + 1)) and p.H1 == H1
        assert np.all(p.AHat[:m0, H - H1:] == 0.0) and np.all(p.AHat[m0:, :] != 0.0)
        assert not (np.linalg.norm(p.AHat, 2) < 1e-2 and np.linalg.norm(p.BHat, 2) < 1e-2)
