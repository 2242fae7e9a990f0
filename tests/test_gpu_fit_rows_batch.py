"""Many ARD-sparse / two-group / three-group / label-masked fits under the heteroscedastic noise model (diag_var = true: one noise
precision per row of Y) in one launch -- vbmf_rows_fit_batched, and vbmf_*_batch_(..., diag_var=True), train_local_folds and
train_dual_folds above it.  Through the C ABI in fp32 storage, every fit against the oracle's update functions stepped on Y as stored
(get_Y) from the oracle's own init: field by field, d and mean(sigmaVecHat) per sweep and the sweep count; plus the stop test, the
independence of the fits from each other, the homoscedastic entries' bits around a row-noise call, the refusals and the Python hosts.

These trajectories are not contractive (from a default random init B collapses or grows within 30 sweeps on several shapes, and a 1e-13
perturbation of the start grows to 3e-12 in 6 sweeps, 1e-10 in 12, 1e-3 in 30), so parity runs 6 sweeps with eps = 0 -- 3 at
(7, 2, 3), whose B reaches exactly 0 by sweep 6 -- and every case first checks on the oracle alone that ||BHat|| stays within
1e-3 .. 1e3 of its start."""
import copy
import dataclasses
import os

import numpy as np
import pytest

import __graft_entry__ as G
from oracle import vbmf_oracle as O

pytestmark = pytest.mark.gpu

# Largest relative error per field against the oracle measured on an MI355X over every case of this file
# (profiles/fit_rows_batch_parity.txt).  Asserted: 3 x the figure, at least FLOOR (summation-order noise times the ~30 x growth of a
# perturbation over 6 sweeps), and never above CAP -- the cap is a condition, not a measurement: an fp32 intermediate shows up at 1e-7
# and must fail.
# Every largest figure but two comes from the diagonal form at (100, 9, 32): 32 factors on 9 columns fit the bag exactly, zetaVec_l is
# what is left of terms 1e3 times its size, and six sweeps carry that cancellation into every field (the oracle, in fp64 too, loses the
# same digits).  Away from H = 32 on 9 or 2 columns no field exceeds 1.3e-12.
MEASURED = dict(BHat=6.33e-11, SigmaB=4.01e-11, CB=1.30e-12, delta=4.31e-11, sigmaVecHat=9.80e-10, zetaVec=7.31e-10, CA=6.27e-13,
                beta=2.35e-10, diagSigmaATVec=3.82e-11, ATVecHat=1.35e-10, SigmaA=3.76e-11, priors=6.47e-13, shapes=3.48e-14, d=9.71e-13,
                trace_d=9.71e-13, trace_s=6.55e-10)
FLOOR, CAP, FACTOR = 1e-12, 1e-8, 3.0
TOL = {k: max(FACTOR * v, FLOOR) for k, v in MEASURED.items()}
assert all(v <= CAP for v in TOL.values())

KINDS = ("sparse", "dual", "trial", "masked")
TRIAL_PAIRS = ("alpha01", "beta01", "alpha02", "beta02", "alpha03", "beta03")
DUAL_PAIRS = ("alpha00", "beta00", "alpha01", "beta01")
REPORT = os.path.join(G.ROOT, "build", "fit_rows_batch_parity.txt")      # (build/ is not tracked)
_worst = {}

# the ROWS placement rule (csrc/fit_batch_kernels.hpp: fitb_fixed_doubles, fitb_rows_in_lds, fitb_placement), restated
LDS_CAP_DOUBLES = 144 * 1024 // 8


def placement(full, L, Mb, H):
    """2: B, Q and the A side in LDS; 1: B and Q only; 0: nothing -- after the fit's two L-vectors have come off the room"""
    np_ = 16 * (1 if H <= 16 else 2)
    fixed = (8 * np_ * (np_ + 2) + 8 * np_ if full else np_ * (np_ + 2)) + 8 * H * H
    room = LDS_CAP_DOUBLES - fixed
    if 2 * L <= room:
        room -= 2 * L
    return 2 if 2 * L * H + 3 * Mb * H <= room else 1 if 2 * L * H <= room else 0


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


def _bag(L, M, H, s):
    """a rank-H product plus noise whose standard deviation runs linearly from 0.05 to 0.4 down the rows"""
    rng = np.random.default_rng(3000 + s)
    B, A = rng.standard_normal((L, H)), rng.standard_normal((M, H))
    return _f32(B @ A.T + np.linspace(0.05, 0.4, L)[:, None] * rng.standard_normal((L, M)))


def _h0(H):
    return max(1, H // 2)


def _start(kind, Y, H, seed, M0=None):
    """the oracle's own init with default_rng(seed).  dual, trial: H0 = max(1, H // 2); trial, masked: M0 = M // 2; masked: H1 = 1"""
    rng = np.random.default_rng(seed)
    M0 = Y.shape[1] // 2 if M0 is None else M0
    if kind == "dual":
        return O.vbmf_dual_init(Y, H, _h0(H), rng=rng, materialize_yhat=False)
    if kind == "trial":
        return O.vbmf_trial_init(Y, H, _h0(H), M0, rng=rng, materialize_yhat=False)
    if kind == "masked":
        return O.vbmf_sparse_init(Y, H, H1=1, labels=np.arange(M0), rng=rng, full_cov=False, materialize_yhat=False)
    return O.vbmf_sparse_init(Y, H, rng=rng, full_cov=False, materialize_yhat=False)


def _oracle(kind, Y, p0, niter, eps, full_cov, compat=True, spectral=True, est_cb=True, est_priors=True):
    """the loops of src/vbmf_sparse.jl:364-378, src/vbmf_dual.jl:476-495 and src/vbmf_trial.jl:560-575 with diag_var = true, stepped
    here because the oracle's own trace records the untouched sigmaHat: returns (p, d, sweeps, [(d, mean(sigmaVecHat))], ||BHat||s)"""
    p = copy.deepcopy(p0)
    old, d, tr, nb = p.BHat.copy(), eps + 1.0, [], [np.linalg.norm(p.BHat)]
    while len(tr) < niter and d > eps:
        if kind == "dual":
            O.dual_updateA(Y, p, reference_compat=compat, diag_var=True, full_cov=full_cov)
        elif kind == "trial":
            O.trial_updateA(Y, p, reference_compat=compat, diag_var=True, full_cov=full_cov)
        else:
            O.sparse_updateA(Y, p, full_cov=full_cov, reference_compat=compat, diag_var=True)
        O.sparse_updateB(Y, p, diag_var=True)
        {"dual": O.dual_updateCA, "trial": O.trial_updateCA}.get(kind, O.sparse_updateCA)(p)
        if est_cb:
            O.sparse_updateCB(p)
        O.sparse_updateSigma(Y, p, diag_var=True)
        if est_priors and kind == "dual":
            O.dual_updatePriors(p)
        if est_priors and kind == "trial":
            O.trial_updatePriors(p)
        with np.errstate(divide="ignore", invalid="ignore"):
            d = O.delta(p.BHat, old) if spectral else float(np.float64(np.linalg.norm(p.BHat - old)) / np.float64(np.linalg.norm(old)))
        old = p.BHat.copy()
        tr.append((d, float(np.mean(p.sigmaVecHat))))
        nb.append(np.linalg.norm(p.BHat))
    return p, d, len(tr), np.array(tr), np.array(nb)


def _pairs(kind, p):
    """the six hyper-prior values the entry takes: a model with fewer groups gives its last pair again"""
    if kind == "trial":
        return [getattr(p, k) for k in TRIAL_PAIRS]
    if kind == "dual":
        return [p.alpha00, p.beta00, p.alpha01, p.beta01, p.alpha01, p.beta01]
    return [p.alpha0, p.beta0] * 3


def _m0(kind, p):
    return int(p.M0) if kind == "trial" else int(np.size(p.labels))


class Call:
    """bags side by side in one context (fp32 storage), Y as stored per bag"""

    def __init__(self, pkg, Ys, H, compat=None, variant=None):
        C = pkg.capi
        self.C, self.H = C, H
        self.off = np.concatenate([[0], np.cumsum([Y.shape[1] for Y in Ys])]).astype(np.int64)
        L, M = Ys[0].shape[0], int(self.off[-1])
        kw = {} if compat is None else dict(reference_compat=compat)
        self.ctx = C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32, **kw, variant=C.VBMF_VARIANT_SPARSE_DIAGVAR if variant is None else variant)
        self.ctx.set_Y(np.concatenate(Ys, axis=1))
        Yall = self.ctx.get_Y()
        self.Ys = [np.ascontiguousarray(Yall[:, a:b]) for a, b in zip(self.off[:-1], self.off[1:])]

    def run(self, kind, starts, bag_of, niter, eps, full_cov, est_cb=True, est_priors=True):
        """starts: the oracle's parameter sets; returns the library's dict"""
        grouped = kind in ("dual", "trial")
        return self.ctx.rows_fit_batched(
            self.off, bag_of, niter, eps, [p.gamma for p in starts], [p.delta0 for p in starts], [p.etaVec[0] for p in starts],
            [p.zeta0 for p in starts], [_pairs(kind, p) for p in starts], np.stack([p.BHat for p in starts]),
            np.stack([p.SigmaB for p in starts]), np.stack([p.CB for p in starts]), np.stack([p.sigmaVecHat for p in starts]),
            np.concatenate([p.CA for p in starts]), [_m0(kind, p) for p in starts] if kind in ("trial", "masked") else None,
            H0=starts[0].H0 if grouped else self.H, mask_H1=starts[0].H1 if kind == "masked" else 0, full_cov=full_cov, est_cb=est_cb,
            est_priors=grouped and est_priors, want_trace=True)

    def close(self):
        self.ctx.close()


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


def _fit_fields(r, f, s0, s1):
    delta = {} if r["delta"] is None else dict(delta=r["delta"][f])                # (not written without est_cb)
    return dict(BHat=r["BHat"][f], SigmaB=r["SigmaB"][f], CB=r["CB"][f], **delta, sigmaVecHat=r["sigmaVecHat"][f],
                zetaVec=r["zetaVec"][f], CA=r["CA"][s0:s1], beta=r["beta"][s0:s1], diagSigmaATVec=r["diagSigmaATVec"][s0:s1],
                ATVecHat=r["ATVecHat"][s0:s1], SigmaA=r["SigmaA"][f])


def _compare(tag, call, kind, r, starts, bag_of, niter, eps, full_cov, stay=True, **okw):
    """every fit of the call against the oracle: the fields, the priors, the sweep count, the trace; returns the worst errors"""
    H, worst, s0 = call.H, {}, 0
    for f, (p0, b) in enumerate(zip(starts, bag_of)):
        po, d, it, tr, nb = _oracle(kind, call.Ys[b], p0, niter, eps, full_cov, **okw)
        if stay:                                                    # the case is worth trusting: B neither collapsed nor blew up
            assert np.all(nb[1:] > 1e-3 * nb[0]) and np.all(nb[1:] < 1e3 * nb[0]), (tag, f, nb)
        s1 = s0 + po.M * H
        e = {k: _rel(v, getattr(po, k)) for k, v in _fit_fields(r, f, s0, s1).items()}
        pri = r["priors9"][f]
        if kind == "trial":
            e["priors"] = _rel(pri[:6], [getattr(po, k) for k in TRIAL_PAIRS])
            e["shapes"] = _rel(pri[6:], [po.alpha1, po.alpha2, po.alpha3])
        elif kind == "dual":
            e["priors"] = _rel(pri[:4], [getattr(po, k) for k in DUAL_PAIRS])
            e["shapes"] = _rel(pri[6:8], [po.alpha0, po.alpha1])
            assert np.array_equal(pri[4:6], [p0.alpha01, p0.beta01]), (tag, f)         # group 3 is empty (M0 = M_b): its pair comes back
        else:
            assert np.array_equal(pri[:6], [po.alpha0, po.beta0] * 3), (tag, f)        # no hyper-prior fit in this model
            e["shapes"] = _rel(pri[6:], [po.alpha] * 3)
        if kind == "masked":                                        # the masked block is exactly zero, not merely small
            assert np.all(r["ATVecHat"][s0:s1].reshape(po.M, H)[:_m0(kind, po), H - int(po.H1):] == 0.0), (tag, f)
        assert r["iters"][f] == it, (tag, f, int(r["iters"][f]), it, r["trace"][f, :, 0], tr[:, 0])
        assert r["status"][f] == 0, (tag, f)
        e["d"] = _rel(r["d"][f], d)
        e["trace_d"] = float(np.max(np.abs(r["trace"][f, :it, 0] - tr[:, 0]) / np.abs(tr[:, 0])))
        e["trace_s"] = float(np.max(np.abs(r["trace"][f, :it, 1] - tr[:, 1]) / np.abs(tr[:, 1])))
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


# ---- 1. every code path's smallest shape, every model, both forms -----------------------------------------------------------------
# (L, M_b, H), the form, the placement class the ROWS rule gives it, the sweeps, the two start seeds (the first two of 0, 1, 2, ... from
# which the oracle's ||BHat|| stays within 1e-3 .. 1e3 of its start in all four models: _compare asserts it).  A 2-column bag's B
# collapses to 0 within 6 sweeps: 3 there.
SHAPES = [
    ((7, 2, 3), False, 2, 3, (2, 3)),        # fewest rows and columns; T > 1 in fitb_product; the repeat layout at M_b = 2
    ((40, 9, 3), False, 2, 6, (0, 2)),       # a typical small bag
    ((33, 70, 16), False, 2, 6, (0, 1)),     # NBK = 1 at its edge, M_b > 64
    ((24, 12, 17), False, 2, 6, (0, 1)),     # NBK = 2 at its lower edge
    ((100, 9, 32), False, 2, 6, (0, 1)),     # the three placement classes of the diagonal form at H = 32 ...
    ((100, 40, 32), False, 1, 6, (0, 1)),
    ((166, 9, 32), False, 0, 6, (0, 2)),
    ((166, 30, 5), False, 2, 6, (1, 3)),     # the MIL shape
    ((7, 2, 3), True, 2, 3, (2, 3)),
    ((40, 9, 3), True, 2, 6, (0, 1)),
    ((33, 70, 16), True, 2, 6, (0, 1)),
    ((24, 12, 17), True, 2, 6, (0, 1)),
    ((7, 2, 32), True, 2, 3, (0, 1)),        # ... and of the full_cov form
    ((18, 9, 32), True, 1, 6, (0, 1)),
    ((24, 12, 32), True, 0, 6, (0, 1)),
    ((166, 30, 5), True, 2, 6, (0, 1)),
]


def test_every_placement_class_is_present_in_each_form():
    for full in (False, True):
        assert {placement(full, *s) for s, f, *_ in SHAPES if f == full} == {0, 1, 2}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,full_cov,place,niter,seeds", SHAPES)
def test_shapes(pkg, kind, shape, full_cov, place, niter, seeds):
    L, M, H = shape
    assert placement(full_cov, L, M, H) == place
    call = Call(pkg, [_bag(L, M, H, L + M + H)], H)
    try:
        starts = [_start(kind, call.Ys[0], H, s) for s in seeds]
        r = call.run(kind, starts, [0, 0], niter, 0.0, full_cov)
        _compare(f"shape {kind} {shape} full={int(full_cov)}", call, kind, r, starts, [0, 0], niter, 0.0, full_cov)
        assert np.all(r["iters"] == niter)
    finally:
        call.close()


# ---- 2. the compat bits, est_cb and est_priors off, several bags in one call -----------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("repeat,spectral", [(False, True), (True, False), (False, False)])
def test_compat_bits_on_several_bags(pkg, kind, repeat, spectral):
    """the diagonal form without the repeat layout, d in Frobenius norms, and fits of different M_b in one call"""
    C = pkg.capi
    L, H, Ms = 40, 3, (9, 3, 21, 70)
    compat = (C.VBMF_COMPAT_SPARSE_REPEAT if repeat else 0) | (C.VBMF_COMPAT_SPECTRAL_DELTA if spectral else 0)
    call = Call(pkg, [_bag(L, m, H, 10 + i) for i, m in enumerate(Ms)], H, compat=compat)
    try:
        bag_of = [0, 1, 2, 3, 2, 0]
        starts = [_start(kind, call.Ys[b], H, 20 + k) for k, b in enumerate(bag_of)]
        # (the 3-column bag's B collapses within 6 sweeps, as at (7, 2, 3): every fit of this call runs 3)
        r = call.run(kind, starts, bag_of, 3, 0.0, False)
        _compare(f"compat {kind} repeat={int(repeat)} spectral={int(spectral)}", call, kind, r, starts, bag_of, 3, 0.0, False,
                 compat=repeat, spectral=spectral)
    finally:
        call.close()


@pytest.mark.parametrize("full_cov", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_without_est_cb_and_est_priors(pkg, kind, full_cov):
    L, H, Ms = 40, 3, (9, 21)
    call = Call(pkg, [_bag(L, m, H, 30 + i) for i, m in enumerate(Ms)], H)
    try:
        bag_of = [0, 1, 0]
        starts = [_start(kind, call.Ys[b], H, 40 + k) for k, b in enumerate(bag_of)]
        r = call.run(kind, starts, bag_of, 6, 0.0, full_cov, est_cb=False, est_priors=False)
        _compare(f"est_cb=0 est_priors=0 {kind} full={int(full_cov)}", call, kind, r, starts, bag_of, 6, 0.0, full_cov, est_cb=False,
                 est_priors=False)
        for f, p0 in enumerate(starts):                             # neither CB nor the hyper-priors moved
            assert np.array_equal(r["CB"][f], p0.CB)
            assert np.array_equal(r["priors9"][f, :6], _pairs(kind, p0))
    finally:
        call.close()


# ---- 3. the stop test -----------------------------------------------------------------------------------------------------------------
# eps and seeds chosen on the oracle's own traces (d stays near 0.8 on these fits and dips below eps at sweeps 6, 5 and 4).  The
# diagonal form only: under full_cov no eps in 0.2 .. 0.95 separates three of the first 24 seeds on three shapes tried.
STOP_SHAPE, STOP_NITER, STOP_EPS, STOP_SEEDS = (40, 9, 3), 12, 0.56, (2, 8, 13)


@pytest.mark.parametrize("full_cov", [False])
def test_stop_test(pkg, full_cov):
    """three fits, one eps a factor >= 1.05 away from every d of every fit up to its stop, three different stopping sweeps"""
    L, M, H = STOP_SHAPE
    call = Call(pkg, [_bag(L, M, H, 5)], H)
    try:
        starts = [_start("sparse", call.Ys[0], H, s) for s in STOP_SEEDS]
        its = []
        for p0 in starts:                                           # the margin and the stops, on the oracle alone
            _, _, it, tr, _ = _oracle("sparse", call.Ys[0], p0, STOP_NITER, STOP_EPS, full_cov)
            assert np.all((tr[:, 0] > 1.05 * STOP_EPS) | (tr[:, 0] < STOP_EPS / 1.05)), tr[:, 0]
            its.append(it)
        assert len(set(its)) == 3 and max(its) < STOP_NITER, its
        r = call.run("sparse", starts, [0, 0, 0], STOP_NITER, STOP_EPS, full_cov)
        assert list(r["iters"]) == its
        _compare(f"stop full={int(full_cov)}", call, "sparse", r, starts, [0, 0, 0], STOP_NITER, STOP_EPS, full_cov, stay=False)
    finally:
        call.close()


# ---- 4. independence and determinism -----------------------------------------------------------------------------------------------------
def _same(r, f, s, q, g, t):
    """fit f of call r (its M H-long fields at s) equals fit g of call q (at t), bit for bit"""
    for k in ("BHat", "SigmaB", "CB", "delta", "sigmaVecHat", "zetaVec", "SigmaA", "priors9", "iters", "d", "status", "trace"):
        assert np.array_equal(r[k][f], q[k][g], equal_nan=True), k
    for k in ("CA", "beta", "diagSigmaATVec", "ATVecHat"):
        assert np.array_equal(r[k][s], q[k][t], equal_nan=True), k


@pytest.mark.parametrize("full_cov", [False, True])
@pytest.mark.parametrize("kind", ("dual", "trial"))
def test_independence_and_determinism(pkg, kind, full_cov):
    L, H, Ms = 40, 3, (21, 2, 9, 70)
    call = Call(pkg, [_bag(L, m, H, 60 + i) for i, m in enumerate(Ms)], H)
    try:
        me = _start(kind, call.Ys[0], H, 77, M0=8)
        ob = [1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3]
        om0 = [1, 0, 70, 5, 2, 9, 31, 21, 0, 4, 0]                 # the others differ from it in M0, on its own bag too
        others = [_start(kind, call.Ys[b], H, 100 + k, M0=m0) for k, (b, m0) in enumerate(zip(ob, om0))]
        n = Ms[0] * H
        alone = call.run(kind, [me], [0], 6, 1e-3, full_cov)
        again = call.run(kind, [me], [0], 6, 1e-3, full_cov)
        first = call.run(kind, [me] + others, [0] + ob, 6, 1e-3, full_cov)
        last = call.run(kind, others + [me], ob + [0], 6, 1e-3, full_cov)
        twice = call.run(kind, [me, others[0], me], [0, 1, 0], 6, 1e-3, full_cov)   # two restarts on a shared bag
        _same(alone, 0, slice(0, n), again, 0, slice(0, n))
        _same(alone, 0, slice(0, n), first, 0, slice(0, n))
        tot = len(last["CA"])
        _same(alone, 0, slice(0, n), last, 11, slice(tot - n, tot))
        _same(alone, 0, slice(0, n), twice, 0, slice(0, n))
        tot = len(twice["CA"])
        _same(alone, 0, slice(0, n), twice, 2, slice(tot - n, tot))
        assert alone["status"][0] == 0 and alone["iters"][0] >= 1
    finally:
        call.close()


# ---- 5. the homoscedastic entries around a row-noise call -------------------------------------------------------------------------------
def test_homoscedastic_entries_untouched(pkg):
    C = pkg.capi
    L, H, Ms = 40, 3, (21, 9)
    call = Call(pkg, [_bag(L, m, H, 80 + i) for i, m in enumerate(Ms)], H, variant=C.VBMF_VARIANT_SPARSE_DIAG)
    try:
        bag_of = [0, 1, 0]
        sp = [_start("sparse", call.Ys[b], H, 50 + k) for k, b in enumerate(bag_of)]
        tr = [_start("trial", call.Ys[b], H, 50 + k) for k, b in enumerate(bag_of)]

        def homo():
            a = call.ctx.sparse_fit_batched(
                call.off, bag_of, 6, 0.0, [p.gamma for p in sp], [p.delta0 for p in sp], [p.eta for p in sp], [p.zeta0 for p in sp],
                [[p.alpha0, p.beta0] * 2 for p in sp], np.stack([p.BHat for p in sp]), np.stack([p.SigmaB for p in sp]),
                np.stack([p.CB for p in sp]), [p.sigmaHat for p in sp], np.concatenate([p.CA for p in sp]), H0=H, want_trace=True)
            b = call.ctx.local_fit_batched(
                call.off, bag_of, 6, 0.0, [p.gamma for p in tr], [p.delta0 for p in tr], [p.eta for p in tr], [p.zeta0 for p in tr],
                [_pairs("trial", p) for p in tr], np.stack([p.BHat for p in tr]), np.stack([p.SigmaB for p in tr]),
                np.stack([p.CB for p in tr]), [p.sigmaHat for p in tr], np.concatenate([p.CA for p in tr]), [p.M0 for p in tr],
                H0=tr[0].H0, est_priors=True, want_trace=True)
            return a, b
        before = homo()
        r = call.run("trial", tr, bag_of, 6, 0.0, False)
        assert np.all(r["iters"] == 6)
        after = homo()
        for x, y in zip(before, after):
            for k, v in x.items():
                if v is not None:
                    assert np.array_equal(v, y[k], equal_nan=True), k
    finally:
        call.close()


# ---- 6. the refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg):
    C = pkg.capi
    VI, VU = C.VBMF_ERR_INVALID, C.VBMF_ERR_UNSUPPORTED
    L, M, H = 24, 20, 3
    Y = _bag(L, M, H, 9)
    off = np.array([0, 1, 12, M], dtype=np.int64)                   # bags of 1, 11 and 8 columns
    rng = np.random.default_rng(3)
    SENT = -7.25                                                    # what every output holds before a refused call

    def run(c, o=off, fit_bag=(1, 2), niter=5, h=H, H0=1, M0=(4, 8), mask_H1=0, full_cov=False, est_priors=False, keep=None):
        nf, fb = len(fit_bag), np.asarray(fit_bag, dtype=np.int64)
        w = np.diff(np.asarray(o))
        mh = int(sum(w[b] for b in fb if 0 <= b < len(w))) * h
        return c.rows_fit_batched(o, fb, niter, 1e-3, np.full(nf, 12.0), np.full(nf, 1e-3), np.full(nf, 5.0), np.full(nf, 1e-3),
                                  np.full((nf, 9), 1e-3), rng.standard_normal((nf, L, h)), np.zeros((nf, h, h)), np.ones((nf, h)),
                                  np.ones((nf, L)), np.ones(mh), M0, H0=H0, mask_H1=mask_H1, full_cov=full_cov, est_priors=est_priors)

    def refused(c, code=VI, **kw):
        with pytest.raises(pkg.VbmfError) as e:
            run(c, **kw)
        assert e.value.code == code, e.value
        return str(e.value)

    p64, dp = (lambda a: a.ctypes.data_as(C.C.POINTER(C.C.c_int64))), C._dptr

    def raw(c, fit_bag=(1, 2), nfits=2, null=False, null_m0=False, o=off, H0=1, mask_H1=0, full=0, est_priors=0, m0=(4, 8), h=H, niter=5):
        """the C entry itself, every in/out and out array primed with SENT: returns (code, whether anything was written)"""
        fb, m0 = np.asarray(fit_bag, dtype=np.int64), np.asarray(m0, dtype=np.int64)
        one = np.ones(64)
        outs = [np.full(n, SENT) for n in (2 * 9, 2 * L * h, 2 * h * h, 2 * h, 2 * L, 2 * M * h, 2 * h, 2 * L, 2 * M * h, 2 * M * h, 2 * h * h,
                                           2 * M * h, 2, 2 * niter * 2 if niter > 0 else 2)]
        pri, B, SB, CB, sv, CA, de, zv, be, dS, SA, A, dl, tr = outs
        it, st = np.full(2, -7, dtype=np.int64), np.full(2, -7, dtype=np.int64)
        rc = C.lib().vbmf_rows_fit_batched(c._h, len(o) - 1, p64(np.asarray(o, dtype=np.int64)), nfits, p64(fb), niter, 1e-3, full, 1,
                                           est_priors, H0, None if null_m0 else p64(m0), mask_H1, dp(one), dp(one), dp(one), dp(one),
                                           dp(pri), None if null else dp(B), dp(SB), dp(CB), dp(sv), dp(CA), dp(de), dp(zv), dp(be),
                                           dp(dS), dp(SA), dp(A), p64(it), dp(dl), p64(st), dp(tr))
        wrote = any(np.any(a != SENT) for a in outs) or np.any(it != -7) or np.any(st != -7)
        return rc, bool(wrote)

    # every sparse-family context serves, *_DIAG or *_DIAGVAR: only its Y is used
    for v in (C.VBMF_VARIANT_SPARSE_DIAG, C.VBMF_VARIANT_DUAL_DIAG, C.VBMF_VARIANT_TRIAL_DIAG, C.VBMF_VARIANT_SPARSE_DIAGVAR,
              C.VBMF_VARIANT_DUAL_DIAGVAR, C.VBMF_VARIANT_TRIAL_DIAGVAR):
        with C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32, variant=v) as c:
            assert "no Y" in refused(c)                             # nothing uploaded yet
            assert raw(c) == (VI, False)
            c.set_Y(Y)
            assert np.all(run(c, est_priors=True)["iters"] >= 1)
            assert np.all(run(c, H0=H, mask_H1=2)["iters"] >= 1)
            assert np.all(run(c, M0=None)["iters"] >= 1)            # M0 = NULL: M0[f] = M_b
    with C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32, variant=C.VBMF_VARIANT_TRIAL_DIAGVAR) as c:
        c.set_Y(Y)
        assert raw(c) == (C.VBMF_OK, True) and raw(c, null_m0=True) == (C.VBMF_OK, True)
        for bad in ([0, 1, 1, M], [1, 12, M], [0, 12, M - 1], [0, 15, 10, M], [0, M + 1]):
            refused(c, o=np.array(bad, dtype=np.int64), fit_bag=(0,), M0=(0,), full_cov=True)
            assert raw(c, o=bad, fit_bag=(0, 0), m0=(0, 0), full=1) == (VI, False)
        assert raw(c, fit_bag=[0, 3]) == (VI, False) and raw(c, fit_bag=[-1, 0]) == (VI, False)   # fit_bag outside 0..nbags-1
        assert raw(c, nfits=0) == (VI, False)
        assert raw(c, null=True) == (VI, False)                     # a required pointer that is NULL
        assert raw(c, niter=0) == (VI, False)
        refused(c, niter=0)
        assert "H0" in refused(c, H0=-1) and raw(c, H0=-1) == (VI, False)
        assert "H0" in refused(c, H0=H + 1) and raw(c, H0=H + 1) == (VI, False)
        assert np.all(run(c, H0=0)["iters"] >= 1) and np.all(run(c, H0=H)["iters"] >= 1)     # both ends are models
        assert "M0" in refused(c, M0=(-1, 8)) and raw(c, m0=(-1, 8)) == (VI, False)
        assert "M0" in refused(c, M0=(4, 9)) and raw(c, m0=(4, 9)) == (VI, False)            # bag 2 has 8 columns
        assert np.all(run(c, M0=(0, 8))["iters"] >= 1)
        assert "mask_H1" in refused(c, H0=H, mask_H1=-1) and raw(c, H0=H, mask_H1=-1) == (VI, False)
        assert "mask_H1" in refused(c, H0=H, mask_H1=H + 1) and raw(c, H0=H, mask_H1=H + 1) == (VI, False)
        assert "mask_H1" in refused(c, H0=1, mask_H1=1) and raw(c, H0=1, mask_H1=1) == (VI, False)   # one prior group ...
        assert "mask_H1" in refused(c, H0=H, mask_H1=1, est_priors=True)                    # ... and no hyper-prior fit
        assert raw(c, H0=H, mask_H1=1, est_priors=1) == (VI, False)
        assert np.all(run(c, H0=H, mask_H1=H)["iters"] >= 1)
        assert "1-column" in refused(c, fit_bag=(0, 1), M0=(1, 4))  # the diagonal form under the repeat layout needs M >= 2 ...
        assert raw(c, fit_bag=(0, 1), m0=(1, 4)) == (VI, False)
        assert np.all(run(c, fit_bag=(0, 1), M0=(1, 4), full_cov=True)["iters"] >= 1)   # ... full_cov does not
    hyper = dict(alpha0=1e-3, beta0=1e-3, gamma0=1e-3, delta0=1e-3, eta0=1e-3, zeta0=1e-3)
    with C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32, variant=C.VBMF_VARIANT_SPARSE_DIAGVAR) as c:   # (only the sparse model takes a mask)
        c.set_Y(Y)
        c.sparse_set_state(rng.standard_normal(M * H), np.ones(M * H), np.ones(M * H), np.ones(M * H), rng.standard_normal((L, H)),
                           0.01 * np.eye(H), np.ones(H), np.ones(H), 1.0, 0.5, hyper, labels0=[0, 5], H1=1)
        before = c.sparse_get_state()
        assert "mask" in refused(c) and raw(c) == (VI, False)
        after = c.sparse_get_state()
        assert all(np.array_equal(v, after[k]) for k, v in before.items())
    with C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32) as c:
        c.set_Y(Y)
        assert "basic" in refused(c) and raw(c) == (VI, False)
    with C.Context(L, M, 33, y_dtype=pkg.VBMF_Y_F32, variant=C.VBMF_VARIANT_TRIAL_DIAGVAR) as c:
        assert "32" in refused(c, code=VU, h=33) and raw(c, h=33) == (VU, False)
    with C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32, nranks=2, rank=0, L_global=2 * L, variant=C.VBMF_VARIANT_TRIAL_DIAGVAR) as c:
        assert "rank" in refused(c) and raw(c) == (VI, False)


# ---- 7. the Python hosts -------------------------------------------------------------------------------------------------------------------
# The per-fit path (vbmf_dual_ / vbmf_sparse_ with diag_var=True) accumulates in fp32: the tolerance its own tests state for it against
# the oracle in fp32 storage (tests/test_gpu_dual.py, tests/test_gpu_trial.py: 2e-3 per field, 2e-2 d + 2e-6 for d), at 3 sweeps
PER_FIT_TOL = 2e-3


def _convert(cls, src):
    dst = cls()
    for f in dataclasses.fields(cls):
        if hasattr(src, f.name):
            setattr(dst, f.name, copy.deepcopy(getattr(src, f.name)))
    return dst


def _close(tag, p, q, names):
    for k in names:
        assert _rel(getattr(p, k), getattr(q, k)) <= PER_FIT_TOL, (tag, k, _rel(getattr(p, k), getattr(q, k)))


HOST_FIELDS = ("BHat", "SigmaB", "CB", "delta", "sigmaVecHat", "zetaVec", "CA", "beta", "diagSigmaATVec", "ATVecHat", "AHat", "SigmaA")


def test_dual_batch_against_the_per_fit_calls(pkg):
    L, H, H0, Ms = 40, 3, 1, (9, 21)
    pkg.set_defaults(y_dtype=pkg.VBMF_Y_F32)
    Ys = [_bag(L, m, H, 90 + i) for i, m in enumerate(Ms)]
    bag_of = [0, 1, 1]
    for full_cov in (False, True):
        ps = [pkg.vbmf_dual_init(Ys[b], H, H0, rng=np.random.default_rng(5 + k)) for k, b in enumerate(bag_of)]
        qs = copy.deepcopy(ps)
        keep = [(p.sigmaHat, p.zeta) for p in ps]
        ds = pkg.vbmf_dual_batch_(Ys, ps, 3, eps=0.0, full_cov=full_cov, bag_of=bag_of, diag_var=True)
        for k, (p, q, b) in enumerate(zip(ps, qs, bag_of)):
            dq = pkg.vbmf_dual_(Ys[b], q, 3, eps=0.0, full_cov=full_cov, diag_var=True)
            assert p.iters == 3 and p.status == 0 and (p.sigmaHat, p.zeta) == keep[k]
            assert abs(ds[k] - dq) <= 2e-2 * abs(dq) + 2e-6
            _close(f"dual full={int(full_cov)}", p, q, HOST_FIELDS + ("alpha00", "beta00", "alpha01", "beta01", "alpha0", "alpha1",
                                                                    "A0Hat", "A1Hat", "CA0", "CA1", "beta0", "beta1"))


def test_train_local_folds_against_the_per_fit_calls(pkg):
    L, H, H1 = 40, 3, 1
    pkg.set_defaults(y_dtype=pkg.VBMF_Y_F32)
    folds = []
    for i, (m, m0) in enumerate(((21, 10), (9, 4))):
        Y = _bag(L, m, H, 95 + i)
        folds.append((Y[:, :m0], Y[:, m0:]))
    ps = pkg.train_local_folds(folds, H, H1, 3, eps=0.0, rng=np.random.default_rng(1), diag_var=True)
    rng = np.random.default_rng(1)
    assert len(ps) == 2
    for p, (Y0, Y1) in zip(ps, folds):
        Y = np.concatenate([Y0, Y1], axis=1)
        q = pkg.vbmf_sparse_init(Y, H, H1=H1, labels=np.arange(1, Y0.shape[1] + 1), rng=rng)
        pkg.vbmf_sparse_(Y, q, 3, eps=0.0, diag_var=True, full_cov=False)
        assert p.iters == 3 and p.status == 0 and np.all(p.AHat[:Y0.shape[1], H - H1:] == 0.0)
        _close("train_local_folds", p, q, HOST_FIELDS)


def test_train_dual_folds_against_the_per_fit_calls(pkg):
    L, H, H0 = 40, 3, 1
    pkg.set_defaults(y_dtype=pkg.VBMF_Y_F32)
    folds = [(_bag(L, 9, H, 97), _bag(L, 21, H, 98)), (_bag(L, 5, H, 99), np.zeros((L, 0)))]
    out = pkg.train_dual_folds(folds, H, H0, 3, eps=0.0, diag_var=True, nstarts=2, rng=np.random.default_rng(2))
    assert out[1] == (0, 0)
    rng = np.random.default_rng(2)
    for c, Y in enumerate(folds[0]):
        kept = None
        for _ in range(2):                                          # the restart loop of examples/mil_util.jl:347-354, every start run
            q = pkg.vbmf_dual_init(Y, H, H0, rng=rng)
            pkg.vbmf_dual_(Y, q, 3, eps=0.0, full_cov=True, diag_var=True)
            if kept is None and not (np.linalg.norm(q.AHat, 2) + np.linalg.norm(q.BHat, 2) < 1e-2):
                kept = q
        kept = q if kept is None else kept
        _close(f"train_dual_folds class {c}", out[0][c], kept, HOST_FIELDS + ("alpha00", "beta00", "alpha01", "beta01"))
