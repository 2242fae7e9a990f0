"""The Gram form of the batched basic-model fits (vbmf_fit_batched_form, vbmf_bags_row_gram; vbmf_batch_(..., form=...)): K = Y Y' entry
by entry against fp64 NumPy under a derived bound, and every fit's whole loop on K against the oracle's loop on Y as stored (get_Y)
from the same start values -- field by field, sweep counts and the trace of d included -- plus the LDS limit, the per-fit rule of
form = 2, the bit-identity of form = 0 with vbmf_fit_batched, the independence of the fits from each other and the refusals.
The helpers are those of tests/test_gpu_fit_basic_batch.py."""
import copy
import dataclasses
import os

import numpy as np
import pytest

import __graft_entry__ as G
from oracle import vbmf_oracle as O

pytestmark = pytest.mark.gpu

# Largest relative error per field against the oracle measured on an MI355X over every case of this file
# (profiles/fit_basic_gram_parity.txt).  Asserted: 3 x the figure, at least FLOOR, and never above CAP -- the form's own fp64 error is
# four orders below CAP, so a layout or indexing error cannot hide under it.
MEASURED = dict(BHat=2.05e-13, AHat=2.75e-13, SigmaA=3.27e-13, SigmaB=1.80e-13, CA=1.94e-13, CB=6.63e-14, sigma2=5.42e-13, d=2.76e-12,
                trace_d=2.76e-12, invCA=2.34e-15, invCB=3.05e-15, YHat=5.22e-16)
FLOOR, CAP, FACTOR = 1e-12, 1e-8, 3.0
TOL = {k: max(FACTOR * v, FLOOR) for k, v in MEASURED.items()}
assert all(v <= CAP for v in TOL.values())

REPORT = os.path.join(G.ROOT, "build", "fit_basic_gram_parity.txt")      # (build/ is not tracked)
_worst = {}
STREAM, GRAM, AUTO = 0, 1, 2


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


def _bag(L, M, H, seed):
    """a rank-H matrix plus noise, as in tests/test_gpu_fit_batch.py"""
    rng = np.random.default_rng(1000 + seed)
    return _f32(rng.standard_normal((L, H)) @ rng.standard_normal((H, M)) + 0.1 * rng.standard_normal((L, M)))


def _start(Y, H, seed):
    """the oracle's init with default_rng(seed): the start values of both sides"""
    return O.vbmf_init(Y, H, rng=np.random.default_rng(seed), materialize_yhat=False)


def _oracle(Y, p0, niter, eps, est_covs, est_var):
    p = copy.deepcopy(p0)
    tr = []
    with np.errstate(all="ignore"):                                 # (the trace's ELBO takes logs the comparison does not use)
        p, it, d = O.vbmf_(Y, p, niter, eps=eps, est_covs=est_covs, est_var=est_var, trace=tr)
    return p, d, it, np.array([t[0] for t in tr])


def _oracle_frobenius(Y, p0, niter, eps, est_covs, est_var):
    """vbmf!'s loop (src/vbmf.jl:193-214) from the oracle's update functions with d in Frobenius norms: what the library computes when
    VBMF_COMPAT_SPECTRAL_DELTA is off (the oracle's own delta is the operator 2-norm)"""
    p = copy.deepcopy(p0)
    old, d, tr = p.BHat, eps + 1.0, []
    while len(tr) < niter and d > eps:
        O.updateA(Y, p)
        O.updateB(Y, p)
        if est_covs:
            O.updateCA(p)
            O.updateCB(p)
        if est_var:
            O.updateSigma2(Y, p)
        d = float(np.linalg.norm(p.BHat - old) / np.linalg.norm(old))
        old = p.BHat
        tr.append(d)
    return p, d, len(tr), np.array(tr)


_FORM_NAME = {STREAM: "stream", GRAM: "gram", AUTO: "auto"}


class Call:
    """bags side by side in one basic context (fp32 storage), Y as stored per bag"""

    def __init__(self, pkg, Ys, H, compat=None):
        C = pkg.capi
        self.C, self.H = C, H
        self.off = np.concatenate([[0], np.cumsum([Y.shape[1] for Y in Ys])]).astype(np.int64)
        L, M = Ys[0].shape[0], int(self.off[-1])
        kw = {} if compat is None else dict(reference_compat=compat)
        self.ctx = C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32, **kw)
        self.ctx.set_Y(np.concatenate(Ys, axis=1))
        Yall = self.ctx.get_Y()
        self.Ys = [np.ascontiguousarray(Yall[:, a:b]) for a, b in zip(self.off[:-1], self.off[1:])]

    def run(self, starts, bag_of, niter, eps, est_covs=True, est_var=True, form=GRAM, want_A=True):
        """starts: the oracle's parameter sets; returns the library's dict"""
        return self.ctx.fit_batched(self.off, bag_of, niter, eps, np.stack([p.BHat for p in starts]), np.stack([p.SigmaB for p in starts]),
                                    np.stack([np.diag(p.CA) for p in starts]), np.stack([np.diag(p.CB) for p in starts]),
                                    [p.sigma2 for p in starts], est_covs=est_covs, est_var=est_var, want_trace=True,
                                    form=_FORM_NAME[form], want_A=want_A)

    def close(self):
        self.ctx.close()


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


def _fit_fields(r, f):
    return dict(BHat=r["BHat"][f], AHat=r["AHat"][f], SigmaA=r["SigmaA"][f], SigmaB=r["SigmaB"][f], CA=np.diag(r["CA"][f]),
                CB=np.diag(r["CB"][f]), sigma2=r["sigma2"][f])


def _compare(tag, call, r, starts, bag_of, niter, eps, est_covs=True, est_var=True, want_iters=None, oracle=_oracle):
    """every fit of the call against the oracle: the fields, the sweep count, the trace of d; returns the worst errors"""
    worst = {}
    for f, (p0, b) in enumerate(zip(starts, bag_of)):
        po, d, it, trd = oracle(call.Ys[b], p0, niter, eps, est_covs, est_var)
        e = {k: _rel(v, getattr(po, k)) for k, v in _fit_fields(r, f).items()}
        assert r["iters"][f] == it, (tag, f, int(r["iters"][f]), it, r["trace"][f, :, 0], trd)
        assert r["status"][f] == 0, (tag, f)
        if want_iters is not None:
            assert it in want_iters, (tag, f, it)
        e["d"] = _rel(r["d"][f], d)
        e["trace_d"] = float(np.max(np.abs(r["trace"][f, :it, 0] - trd) / np.abs(trd)))
        assert np.all(r["trace"][f, it:] == 0.0)
        if est_var:
            assert r["trace"][f, it - 1, 1] == r["sigma2"][f]
        for k, v in e.items():
            worst[k] = max(worst.get(k, 0.0), v)
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


def _same(r, f, q, g, skip=()):
    """fit f of call r equals fit g of call q, bit for bit"""
    for k in ("BHat", "AHat", "SigmaA", "SigmaB", "CA", "CB", "sigma2", "iters", "d", "status", "trace"):
        if k not in skip:
            assert np.array_equal(r[k][f], q[k][g], equal_nan=True), k


# ---- 1. K entry by entry --------------------------------------------------------------------------------------------------------------
K_MS = (257, 1, 3, 4, 64, 5)
U = 2.0 ** -53


@pytest.mark.parametrize("y_dtype", ["f32", "bf16"])
@pytest.mark.parametrize("L", [1, 7, 16, 17, 33, 166])
def test_row_gram_entry_by_entry(pkg, L, y_dtype):
    """every K_b against fp64 Y Y' of Y as stored.  Each side is a sum of M_b exact products (an fp32 or bf16 value squared needs 48
    bits at most), so each differs from the true sum by at most gamma_n (|Y| |Y|')_ij, n = M_b: the bound is twice that"""
    C = pkg.capi
    dt = pkg.VBMF_Y_F32 if y_dtype == "f32" else pkg.VBMF_Y_BF16
    rng = np.random.default_rng(7 * L)
    Ys = [rng.standard_normal((L, m)) for m in K_MS]

    def gram(order):
        off = np.concatenate([[0], np.cumsum([K_MS[b] for b in order])]).astype(np.int64)
        with C.Context(L, int(off[-1]), 1, y_dtype=dt) as c:
            c.set_Y(np.concatenate([Ys[b] for b in order], axis=1))
            Yall = c.get_Y()
            return c.row_gram(off), [Yall[:, a:b] for a, b in zip(off[:-1], off[1:])]

    order = list(range(len(K_MS)))
    K, stored = gram(order)
    assert K.shape == (len(K_MS), L, L)
    for b, Y in enumerate(stored):
        n = Y.shape[1]
        bound = 2.0 * (n * U / (1.0 - n * U)) * (np.abs(Y) @ np.abs(Y).T)
        err = np.abs(K[b] - Y @ Y.T)
        assert np.all(err <= bound), (L, y_dtype, b, float(np.max(err - bound)))
        assert np.array_equal(K[b], K[b].T)
        assert np.all(np.diag(K[b]) > 0.0)
    # the 257- and the 5-column bag: first, last and alone in the call
    Kr, _ = gram(order[::-1])
    for b in order:
        assert np.array_equal(K[b], Kr[len(order) - 1 - b]), b
    for b in (0, 5):
        Ka, _ = gram([b])
        assert np.array_equal(K[b], Ka[0]), b


# ---- 2. fixed sweeps ------------------------------------------------------------------------------------------------------------------
FIXED_L, FIXED_H, FIXED_MS = 24, 3, (37, 2, 9, 64, 200)


def _fixed(pkg, compat):
    L, H, Ms = FIXED_L, FIXED_H, FIXED_MS
    call = Call(pkg, [_bag(L, m, H, i) for i, m in enumerate(Ms)], H, compat=compat)
    bag_of = [b for b in range(len(Ms)) for _ in range(2)]
    starts = [_start(call.Ys[b], H, 10 * b + k) for b in range(len(Ms)) for k in range(2)]
    return call, bag_of, starts


@pytest.mark.parametrize("est_var", [False, True])
@pytest.mark.parametrize("est_covs", [False, True])
def test_fixed_sweeps(pkg, est_covs, est_var):
    call, bag_of, starts = _fixed(pkg, None)
    try:
        r = call.run(starts, bag_of, 6, 0.0, est_covs, est_var)
        assert np.all(r["form_used"] == 1)
        _compare(f"fixed est_covs={int(est_covs)} est_var={int(est_var)}", call, r, starts, bag_of, 6, 0.0, est_covs, est_var)
        assert np.all(r["iters"] == 6)
        for f, p0 in enumerate(starts):                             # what is not estimated does not move
            if not est_covs:
                assert np.array_equal(r["CA"][f], np.diag(p0.CA)) and np.array_equal(r["CB"][f], np.diag(p0.CB))
            if not est_var:
                assert r["sigma2"][f] == p0.sigma2
    finally:
        call.close()


def test_fixed_sweeps_frobenius_d(pkg):
    """without VBMF_COMPAT_SPECTRAL_DELTA: d = ||B - B_old||_F / ||B_old||_F"""
    call, bag_of, starts = _fixed(pkg, pkg.capi.VBMF_COMPAT_SPARSE_REPEAT)
    try:
        r = call.run(starts, bag_of, 6, 0.0)
        _compare("fixed frobenius d", call, r, starts, bag_of, 6, 0.0, oracle=_oracle_frobenius)
    finally:
        call.close()


# ---- 3. the stop test -------------------------------------------------------------------------------------------------------------------
STOP_EPS, STOP_NITER = 1e-3, 30
STOP_SHAPES = ((24, 200, 3), (166, 640, 5), (7, 300, 1), (50, 1, 2))
# bag seed = start seed.  The test asserts on the oracle that no sweep's d of these seeds lies within 1 % of eps (the closest is
# 5.6 %: (7, 300, 1), seed 2); a seed that did would have to be replaced, never the case dropped
STOP_SEEDS = (0, 1, 2, 3)


@pytest.mark.parametrize("si", range(len(STOP_SHAPES)))
def test_stop_test(pkg, si):
    L, M, H = STOP_SHAPES[si]
    call = Call(pkg, [_bag(L, M, H, s) for s in STOP_SEEDS], H)
    try:
        bag_of = list(range(len(STOP_SEEDS)))
        starts = [_start(call.Ys[b], H, s) for b, s in enumerate(STOP_SEEDS)]
        for b, p0 in enumerate(starts):                             # the margin, on the oracle alone
            trd = _oracle(call.Ys[b], p0, STOP_NITER, STOP_EPS, True, True)[3]
            assert np.all(np.abs(trd - STOP_EPS) > 0.01 * STOP_EPS), (si, b, trd)
        r = call.run(starts, bag_of, STOP_NITER, STOP_EPS)
        assert np.all(r["form_used"] == 1)
        _compare(f"stop {(L, M, H)}", call, r, starts, bag_of, STOP_NITER, STOP_EPS)   # sweep counts equal the oracle's exactly
    finally:
        call.close()


# ---- 4. the tier edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(40, 200, 16), (33, 150, 17), (36, 160, 32)])
def test_tier_edges(pkg, shape):
    L, M, H = shape
    call = Call(pkg, [_bag(L, M, H, 40 + H)], H)
    try:
        starts = [_start(call.Ys[0], H, s) for s in (0, 1)]
        r = call.run(starts, [0, 0], 6, 0.0)
        _compare(f"tier {shape}", call, r, starts, [0, 0], 6, 0.0)
    finally:
        call.close()


# ---- 5. the LDS limit ---------------------------------------------------------------------------------------------------------------------
def _gram_room(H):
    """doubles left for the Gram form's state: VBMF_FIT_LDS_CAP_BYTES / 8 minus one P x (P + 2) inverse image and nine H x H matrices,
    P = 16 for H <= 16, else 32 (include/vbmf_hip.h)"""
    P = 16 if H <= 16 else 32
    return 147456 // 8 - P * (P + 2) - 9 * H * H


def test_lds_limit(pkg):
    H = 3
    L = _gram_room(H) // (3 * H) + 1                                # the smallest L whose B, T and V do not fit
    assert L == 2008 and 3 * (L - 1) * H <= _gram_room(H) < 3 * L * H
    call = Call(pkg, [_bag(L, 2 * L, H, 70)], H)
    try:
        starts = [_start(call.Ys[0], H, 5)]
        with pytest.raises(pkg.VbmfError) as e:
            call.run(starts, [0], 3, 0.0, form=GRAM)
        assert e.value.code == pkg.capi.VBMF_ERR_UNSUPPORTED and "LDS" in str(e.value)
        r = call.run(starts, [0], 3, 0.0, form=AUTO)
        q = call.run(starts, [0], 3, 0.0, form=STREAM)
        assert list(r["form_used"]) == [0]
        _same(r, 0, q, 0)
    finally:
        call.close()
    # one row fewer fits
    call = Call(pkg, [_bag(L - 1, 5, H, 71)], H)
    try:
        starts = [_start(call.Ys[0], H, 6)]
        r = call.run(starts, [0], 3, 0.0, form=GRAM)
        _compare("lds limit L - 1", call, r, starts, [0], 3, 0.0)
    finally:
        call.close()


# ---- 6. form = 2 ----------------------------------------------------------------------------------------------------------------------------
def test_auto_rule_in_one_call(pkg):
    """bags on both sides of M_b >= VBMF_FIT_GRAM_WIDE_FACTOR L in one call: form_used is the documented rule, and every fit is what it
    is alone under the forced form"""
    C = pkg.capi
    L, H = 24, 3
    w = C.VBMF_FIT_GRAM_WIDE_FACTOR * L
    Ms = (w - 1, w, 5, 4 * w, w + 1)
    call = Call(pkg, [_bag(L, m, H, 80 + i) for i, m in enumerate(Ms)], H)
    try:
        bag_of = [0, 1, 2, 3, 4, 1, 0]
        starts = [_start(call.Ys[b], H, 30 + k) for k, b in enumerate(bag_of)]
        r = call.run(starts, bag_of, 8, 1e-3, form=AUTO)
        want = [C.fit_form_auto(L, Ms[b], H) for b in bag_of]
        assert want == [0, 1, 0, 1, 1, 1, 0] and list(r["form_used"]) == want
        for f, (b, fm) in enumerate(zip(bag_of, want)):
            alone = call.run([starts[f]], [b], 8, 1e-3, form=GRAM if fm else STREAM)
            assert alone["iters"][0] >= 2
            _same(r, f, alone, 0)
    finally:
        call.close()


# ---- 7. form = 0 ----------------------------------------------------------------------------------------------------------------------------
def test_form_stream_is_vbmf_fit_batched(pkg):
    """form = 0 through vbmf_fit_batched_form against vbmf_fit_batched on section 12's fixed-sweep case: every array bit for bit"""
    C = pkg.capi
    L, H, Ms = 24, 3, (37, 2, 9, 64)
    call = Call(pkg, [_bag(L, m, H, i) for i, m in enumerate(Ms)], H)
    try:
        bag_of = [b for b in range(len(Ms)) for _ in range(3)]
        starts = [_start(call.Ys[b], H, 10 * b + k) for b in range(len(Ms)) for k in range(3)]
        q = call.run(starts, bag_of, 8, 0.0, form=STREAM)          # (Context.fit_batched calls vbmf_fit_batched for "stream")
        nf, off = len(starts), call.off
        fb = np.asarray(bag_of, dtype=np.int64)
        B = np.ascontiguousarray(np.stack([p.BHat for p in starts]).transpose(0, 2, 1))
        SB = np.stack([p.SigmaB for p in starts]).copy()
        ca, cb = np.stack([np.diag(p.CA) for p in starts]).copy(), np.stack([np.diag(p.CB) for p in starts]).copy()
        s2 = np.array([p.sigma2 for p in starts])
        Msf = off[fb + 1] - off[fb]
        A, SA = np.empty(int(Msf.sum()) * H), np.empty((nf, H, H))
        it, dl, st, used = np.zeros(nf, dtype=np.int64), np.empty(nf), np.zeros(nf, dtype=np.int64), np.full(nf, -1, dtype=np.int64)
        tr = np.zeros((nf, 8, 2))
        p64, dp = (lambda a: a.ctypes.data_as(C.C.POINTER(C.C.c_int64))), C._dptr
        rc = C.lib().vbmf_fit_batched_form(call.ctx._h, len(Ms), p64(off), nf, p64(fb), 8, 0.0, 1, 1, dp(B), dp(SB), dp(ca), dp(cb), dp(s2),
                                           dp(A), dp(SA), p64(it), dp(dl), p64(st), dp(tr), 0, p64(used))
        assert rc == C.VBMF_OK and np.all(used == 0)
        ends = np.cumsum(Msf) * H
        for f in range(nf):
            assert np.array_equal(B[f].T, q["BHat"][f]) and np.array_equal(SB[f], q["SigmaB"][f]) and np.array_equal(SA[f], q["SigmaA"][f])
            assert np.array_equal(A[ends[f] - Msf[f] * H:ends[f]].reshape(H, Msf[f]).T, q["AHat"][f])
        for mine, k in ((ca, "CA"), (cb, "CB"), (s2, "sigma2"), (it, "iters"), (dl, "d"), (st, "status"), (tr, "trace")):
            assert np.array_equal(mine, q[k]), k
    finally:
        call.close()


# ---- 8. independence ------------------------------------------------------------------------------------------------------------------------
def test_independence(pkg):
    L, H, Ms = 24, 3, (37, 2, 9, 64)
    call = Call(pkg, [_bag(L, m, H, i) for i, m in enumerate(Ms)], H)
    try:
        me = _start(call.Ys[0], H, 77)
        ob = [1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3]
        others = [_start(call.Ys[b], H, 100 + k) for k, b in enumerate(ob)]
        alone = call.run([me], [0], 8, 1e-3)
        first = call.run([me] + others, [0] + ob, 8, 1e-3)
        last = call.run(others + [me], ob + [0], 8, 1e-3)
        twice = call.run([me, others[0], me], [0, 1, 0], 8, 1e-3)
        assert alone["iters"][0] >= 2
        _same(alone, 0, first, 0)
        _same(alone, 0, last, 11)
        _same(alone, 0, twice, 0)
        _same(alone, 0, twice, 2)
    finally:
        call.close()


def test_fits_that_share_a_bag(pkg):
    """two fits on one bag (one K) equal the same fits on two copies of the bag (two Ks)"""
    L, H = 24, 3
    Y, Z = _bag(L, 64, H, 3), _bag(L, 9, H, 2)
    shared, copies = Call(pkg, [Y, Z], H), Call(pkg, [Y, Z, Y], H)
    try:
        s = [_start(shared.Ys[0], H, 11), _start(shared.Ys[0], H, 12)]
        r = shared.run(s, [0, 0], 8, 1e-3)
        q = copies.run(s, [0, 2], 8, 1e-3)
        assert not np.array_equal(r["BHat"][0], r["BHat"][1])
        _same(r, 0, q, 0)
        _same(r, 1, q, 1)
    finally:
        shared.close()
        copies.close()


# ---- 9. an all-zero bag and a sick fit among normal ones ---------------------------------------------------------------------------------------
def test_zero_bag(pkg):
    L, H = 24, 3
    Ya, Yb, Z = _bag(L, 9, H, 2), _bag(L, 37, H, 0), np.zeros((L, 11))
    with_z, without = Call(pkg, [Ya, Z, Yb], H), Call(pkg, [Ya, Yb], H)
    try:
        sa, sz, sb = _start(Ya, H, 5), _start(Z, H, 6), _start(Yb, H, 7)
        po, d, it, _ = _oracle(Z, sz, 8, 1e-3, True, True)
        assert it == 2 and np.isnan(d)                              # what the reference's loop does on a zero matrix
        r = with_z.run([sa, sz, sb], [0, 1, 2], 8, 1e-3)
        q = without.run([sa, sb], [0, 1], 8, 1e-3)
        assert r["iters"][1] == 2 and np.isnan(r["d"][1]) and r["status"][1] == 0
        assert np.all(r["BHat"][1] == 0.0) and np.all(r["AHat"][1] == 0.0)
        _same(r, 0, q, 0)
        _same(r, 2, q, 1)
    finally:
        with_z.close()
        without.close()


def test_status_of_a_fit_that_meets_a_non_finite_value(pkg):
    """a NaN sigma2 in one fit: status 1 after its first sweep, the call succeeds, the neighbours are what they are without it"""
    L, H, Ms = 24, 3, (37, 9)
    call = Call(pkg, [_bag(L, m, H, i) for i, m in enumerate(Ms)], H)
    try:
        good = [_start(call.Ys[b], H, 40 + b) for b in (0, 1)]
        sick = _start(call.Ys[0], H, 42)
        sick.sigma2 = float("nan")
        r = call.run([good[0], sick, good[1]], [0, 0, 1], 8, 1e-3)
        q = call.run(good, [0, 1], 8, 1e-3)
        assert list(r["status"]) == [0, 1, 0] and r["iters"][1] == 1
        _same(r, 0, q, 0)
        _same(r, 2, q, 1)
    finally:
        call.close()


# ---- 10. AHat = NULL --------------------------------------------------------------------------------------------------------------------------
def test_without_ahat(pkg):
    L, H, Ms = 24, 3, (37, 300)
    call = Call(pkg, [_bag(L, m, H, i) for i, m in enumerate(Ms)], H)
    try:
        starts = [_start(call.Ys[b], H, 50 + b) for b in (0, 1)]
        r = call.run(starts, [0, 1], 8, 1e-3)
        q = call.run(starts, [0, 1], 8, 1e-3, want_A=False)
        assert q["AHat"] is None
        for f in (0, 1):
            _same(r, f, q, f, skip=("AHat",))
    finally:
        call.close()


# ---- 11. the Python host --------------------------------------------------------------------------------------------------------------------
def _convert(cls, src):
    dst = cls()
    for f in dataclasses.fields(cls):
        if hasattr(src, f.name):
            setattr(dst, f.name, copy.deepcopy(getattr(src, f.name)))
    return dst


@pytest.mark.parametrize("as_bags", [False, True])
def test_python_host_fills_what_the_stream_form_fills(pkg, as_bags):
    """vbmf_batch_(..., form="gram") on package parameter sets: every field form="stream" fills, against the oracle (fp32 storage)"""
    L, H, Ms = 24, 3, (9, 137)
    Ys = [_bag(L, m, H, i) for i, m in enumerate(Ms)]
    bag_of = [0, 1, 1]
    starts = [_start(Ys[b], H, 60 + k) for k, b in enumerate(bag_of)]
    ps = [_convert(pkg.vbmf_parameters, s) for s in starts]
    held = [(p.CA, p.CB, p.AHat, p.BHat) for p in ps]
    src = pkg.Bags(Ys, H) if as_bags else Ys
    try:
        out = pkg.vbmf_batch_(src, ps, 30, eps=1e-3, est_covs=True, est_var=True, bag_of=bag_of, form="gram")
        if as_bags:
            K = pkg.row_gram_batch(src)
            assert K.shape == (2, L, L) and _rel(K[1], Ys[1] @ Ys[1].T) < 1e-14
    finally:
        if as_bags:
            src.close()
    assert len(out) == 3 and all(a is b for a, b in zip(out, ps))
    worst = {}
    for p, s, b, (ca, cb, a0, b0) in zip(ps, starts, bag_of, held):
        po, do, it, _ = _oracle(Ys[b], s, 30, 1e-3, True, True)
        assert p.iters == it and 2 <= it < 30 and p.status == 0 and p.form_used == 1
        assert p.CA is ca and p.CB is cb and p.AHat is not a0 and p.BHat is not b0   # diagonals in place, factors rebound
        worst["d"] = max(worst.get("d", 0.0), abs(p.d - do) / abs(do))
        po.YHat = po.BHat @ po.AHat.T                               # src/vbmf.jl:217
        for k in ("AHat", "BHat", "SigmaA", "SigmaB", "CA", "CB", "invCA", "invCB", "sigma2", "YHat"):
            worst[k] = max(worst.get(k, 0.0), _rel(getattr(p, k), getattr(po, k)))
    _record(f"python host bags={int(as_bags)}", worst)


def test_train_folds_auto_runs_on_the_device(pkg):
    L, H = 24, 3
    folds = [(_bag(L, 9, H, 0), _bag(L, 137, H, 1)), (np.zeros((L, 0)), _bag(L, 5, H, 2))]
    out = pkg.train_folds(folds, "basic", H, 30, eps=1e-3, rng=np.random.default_rng(1), form="auto")
    assert out[1] == (0, 0)
    rng = np.random.default_rng(1)
    for Y, p, used in zip(folds[0], out[0], (0, 1)):
        s = pkg.vbmf_init(Y, H, rng=rng)
        q = pkg.vbmf_batch_([Y], [s], 30, eps=1e-3, est_covs=True, est_var=True, form="auto")[0]
        assert isinstance(p, pkg.vbmf_parameters) and p.status == 0 and 2 <= p.iters < 30 and p.form_used == q.form_used == used
        assert p.iters == q.iters and np.array_equal(p.BHat, q.BHat) and np.array_equal(p.AHat, q.AHat)


def test_refusals(pkg):
    C = pkg.capi
    VI = C.VBMF_ERR_INVALID
    L, M, H = 24, 60, 3
    Y = _bag(L, M, H, 9)
    off = np.array([0, 1, 12, M], dtype=np.int64)
    rng = np.random.default_rng(3)
    p64, dp = (lambda a: a.ctypes.data_as(C.C.POINTER(C.C.c_int64))), C._dptr
    one, st, it = np.ones(64), np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int64)

    def raw(c, form, null=None):
        fb = np.array([1, 2], dtype=np.int64)
        args = dict(BHat=dp(np.ones(2 * L * H)), SigmaB=dp(np.ones(2 * H * H)), CA=dp(one), CB=dp(one), sigma2=dp(one), iters=p64(it),
                    d=dp(one), status=p64(st), fit_bag=p64(fb))
        if null:
            args[null] = None
        return C.lib().vbmf_fit_batched_form(c._h, 3, p64(off), 2, args["fit_bag"], 5, 1e-3, 1, 1, args["BHat"], args["SigmaB"], args["CA"],
                                             args["CB"], args["sigma2"], None, None, args["iters"], args["d"], args["status"], None, form, None)

    with C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32) as c:
        c.set_Y(Y)
        for form in (0, 1, 2):
            assert raw(c, form) == C.VBMF_OK                        # AHat, SigmaA, trace and form_used may be NULL
        for form in (-1, 3, 1 << 40):
            assert raw(c, form) == VI
        for name in ("BHat", "SigmaB", "CA", "CB", "sigma2", "iters", "d", "status", "fit_bag"):
            assert raw(c, 1, null=name) == VI, name                 # a required pointer that is NULL
        assert C.lib().vbmf_bags_row_gram(c._h, 3, p64(off), None) == VI
        assert C.lib().vbmf_bags_row_gram(c._h, 3, p64(np.array([0, 12, 12, M], dtype=np.int64)), dp(np.empty(3 * L * L))) == VI
        with pytest.raises(ValueError, match="form"):               # a bad form string: refused on the host
            c.fit_batched(off, [1, 2], 5, 1e-3, np.ones((2, L, H)), np.zeros((2, H, H)), np.ones((2, H)), np.ones((2, H)), np.ones(2),
                          form="wide")
        c.set_state(rng.standard_normal((M, H)), rng.standard_normal((L, H)), 0.01 * np.eye(H), 0.01 * np.eye(H), np.ones(H), np.ones(H),
                    1.0, labels0=[0, 5], H1=1)
        assert raw(c, 1) == VI                                      # a label mask
    with C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32) as c:           # no Y
        assert raw(c, 1) == VI
        assert C.lib().vbmf_bags_row_gram(c._h, 3, p64(off), dp(np.empty(3 * L * L))) == VI
    with C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32, variant=C.VBMF_VARIANT_SPARSE_DIAG) as c:
        c.set_Y(Y)
        assert raw(c, 1) == VI                                      # a sparse context has no Gram form ...
        K = c.row_gram(off)                                         # ... but its bags have a K
        Ys = c.get_Y()
        assert _rel(K[2], Ys[:, 12:] @ Ys[:, 12:].T) < 1e-14
