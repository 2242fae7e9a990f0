"""Many basic-model fits in one launch (vbmf_fit_batched, vbmf_batch_): every fit's whole vbmf! loop in one workgroup, against the
oracle's loop on Y as stored (get_Y) from the same start values -- field by field, sweep counts and the trace of d included -- plus the
independence of the fits from each other, the three state placements and the C ABI's refusals."""
import copy
import dataclasses
import os

import numpy as np
import pytest

import __graft_entry__ as G
from oracle import vbmf_oracle as O

pytestmark = pytest.mark.gpu

# Largest relative error per field against the oracle measured on an MI355X over every case of this file
# (profiles/fit_basic_batch_parity.txt).  Asserted: 3 x the figure, at least FLOOR, and never above CAP -- an fp32 intermediate shows
# up at 1e-7, which CAP must catch.
MEASURED = dict(BHat=3.31e-13, AHat=2.42e-13, SigmaA=3.27e-13, SigmaB=2.78e-13, CA=1.87e-13, CB=2.80e-13, sigma2=2.15e-13, d=4.36e-12,
                trace_d=4.36e-12, invCA=2.47e-15, invCB=1.81e-15, YHat=5.69e-16)
FLOOR, CAP, FACTOR = 1e-12, 1e-8, 3.0
TOL = {k: max(FACTOR * v, FLOOR) for k, v in MEASURED.items()}
assert all(v <= CAP for v in TOL.values())

REPORT = os.path.join(G.ROOT, "build", "fit_basic_batch_parity.txt")     # (build/ is not tracked)
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

    def run(self, starts, bag_of, niter, eps, est_covs=True, est_var=True):
        """starts: the oracle's parameter sets; returns the library's dict"""
        return self.ctx.fit_batched(self.off, bag_of, niter, eps, np.stack([p.BHat for p in starts]), np.stack([p.SigmaB for p in starts]),
                                    np.stack([np.diag(p.CA) for p in starts]), np.stack([np.diag(p.CB) for p in starts]),
                                    [p.sigma2 for p in starts], est_covs=est_covs, est_var=est_var, want_trace=True)

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


# ---- 1. fixed sweeps ------------------------------------------------------------------------------------------------------------------
FIXED_L, FIXED_H, FIXED_MS = 24, 3, (37, 2, 9, 64)


def _fixed(pkg, compat):
    L, H, Ms = FIXED_L, FIXED_H, FIXED_MS
    call = Call(pkg, [_bag(L, m, H, i) for i, m in enumerate(Ms)], H, compat=compat)
    bag_of = [b for b in range(len(Ms)) for _ in range(3)]
    starts = [_start(call.Ys[b], H, 10 * b + k) for b in range(len(Ms)) for k in range(3)]
    return call, bag_of, starts


@pytest.mark.parametrize("est_var", [False, True])
@pytest.mark.parametrize("est_covs", [False, True])
def test_fixed_sweeps(pkg, est_covs, est_var):
    call, bag_of, starts = _fixed(pkg, None)
    try:
        r = call.run(starts, bag_of, 8, 0.0, est_covs, est_var)
        _compare(f"fixed est_covs={int(est_covs)} est_var={int(est_var)}", call, r, starts, bag_of, 8, 0.0, est_covs, est_var)
        assert np.all(r["iters"] == 8)
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
        r = call.run(starts, bag_of, 8, 0.0)
        _compare("fixed frobenius d", call, r, starts, bag_of, 8, 0.0, oracle=_oracle_frobenius)
    finally:
        call.close()


# ---- 2. the stop test -------------------------------------------------------------------------------------------------------------------
STOP_EPS, STOP_NITER = 1e-3, 30
STOP_SHAPES = ((24, 37, 3), (166, 64, 5), (7, 30, 1), (50, 1, 2))
# six starts per shape.  The test asserts on the oracle that no sweep's d of these seeds lies within 1 % of eps (with these bags the
# closest is 3.2 %: (166, 64, 5), seed 0); a seed that did would have to be replaced, never the case dropped
STOP_SEEDS = (0, 1, 2, 3, 4, 5)


@pytest.mark.parametrize("si", range(len(STOP_SHAPES)))
def test_stop_test(pkg, si):
    L, M, H = STOP_SHAPES[si]
    call = Call(pkg, [_bag(L, M, H, 20 + si)], H)
    try:
        starts = [_start(call.Ys[0], H, s) for s in STOP_SEEDS]
        for p0 in starts:                                           # the margin, on the oracle alone
            trd = _oracle(call.Ys[0], p0, STOP_NITER, STOP_EPS, True, True)[3]
            assert np.all(np.abs(trd - STOP_EPS) > 0.01 * STOP_EPS), (si, trd)
        r = call.run(starts, [0] * 6, STOP_NITER, STOP_EPS)
        _compare(f"stop {(L, M, H)}", call, r, starts, [0] * 6, STOP_NITER, STOP_EPS,
                 want_iters=(STOP_NITER,) if M == 1 else (5, 6, 7))  # the 1-column bag never meets eps: d ~ 0.98 every sweep
    finally:
        call.close()


# ---- 3. the tier edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(40, 21, 16), (33, 20, 17), (36, 20, 32)])
def test_tier_edges(pkg, shape):
    L, M, H = shape
    call = Call(pkg, [_bag(L, M, H, 40 + H)], H)
    try:
        starts = [_start(call.Ys[0], H, s) for s in (0, 1)]
        r = call.run(starts, [0, 0], 6, 0.0)
        _compare(f"tier {shape}", call, r, starts, [0, 0], 6, 0.0)
    finally:
        call.close()


# ---- 4. the three state placements --------------------------------------------------------------------------------------------------------
LDS_DOUBLES = 144 * 1024 // 8                                       # the cap of DESIGN.md section 11


def _room(H):
    """doubles left for a fit's state: the cap minus one 16 NBK x (16 NBK + 2) inverse image and nine H x H matrices (section 12)"""
    NP = 16 if H <= 16 else 32
    return LDS_DOUBLES - NP * (NP + 2) - 9 * H * H


def test_state_placements_in_one_call(pkg):
    """L = 12, H = 3: B, Q and A in LDS up to 5997 columns; from 5998 on A lives in global memory, B and Q stay in LDS"""
    L, H = 12, 3
    first_out = (_room(H) - 2 * L * H) // H + 1                     # the smallest bag whose P / A no longer fits beside B and Q
    assert first_out == 5998
    Ms = (first_out, 5, first_out - 1)
    call = Call(pkg, [_bag(L, m, H, 50 + i) for i, m in enumerate(Ms)], H)
    try:
        bag_of = [0, 1, 2, 0, 1]
        starts = [_start(call.Ys[b], H, 3 + k) for k, b in enumerate(bag_of)]
        r = call.run(starts, bag_of, 4, 0.0)
        _compare("placement A global + lds", call, r, starts, bag_of, 4, 0.0)
    finally:
        call.close()


def test_state_all_in_global_memory(pkg):
    """the third placement: B and Q alone (2 L H doubles) exceed the LDS room, so all of the fit's state lives in its scratch slices.
    One call has one L, so this placement cannot stand beside an LDS-resident fit: two fits on two tall bags"""
    H = 3
    L = _room(H) // (2 * H) + 1                                     # the smallest L whose B and Q do not fit
    assert L == 3011
    call = Call(pkg, [_bag(L, 4, H, 60), _bag(L, 7, H, 61)], H)
    try:
        starts = [_start(call.Ys[b], H, 5 + b) for b in (0, 1)]
        r = call.run(starts, [0, 1], 4, 0.0)
        _compare("placement all global", call, r, starts, [0, 1], 4, 0.0)
    finally:
        call.close()


# ---- 5. independence ------------------------------------------------------------------------------------------------------------------------
def _same(r, f, q, g):
    """fit f of call r equals fit g of call q, bit for bit"""
    for k in ("BHat", "AHat", "SigmaA", "SigmaB", "CA", "CB", "sigma2", "iters", "d", "status", "trace"):
        assert np.array_equal(r[k][f], q[k][g], equal_nan=True), k


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


# ---- 6. an all-zero bag among normal ones ------------------------------------------------------------------------------------------------------
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


# ---- 7. the refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg):
    C = pkg.capi
    VI, VU = C.VBMF_ERR_INVALID, C.VBMF_ERR_UNSUPPORTED
    L, M, H = 24, 20, 3
    Y = _bag(L, M, H, 9)
    off = np.array([0, 1, 12, M], dtype=np.int64)
    rng = np.random.default_rng(3)

    def state(c, h=H, **kw):
        c.set_state(rng.standard_normal((M, h)), rng.standard_normal((L, h)), 0.01 * np.eye(h), 0.01 * np.eye(h), np.ones(h), np.ones(h),
                    1.0, **kw)

    def run(c, o=off, fit_bag=(1, 2), niter=5, h=H):
        nf = len(fit_bag)
        return c.fit_batched(o, np.asarray(fit_bag, dtype=np.int64), niter, 1e-3, rng.standard_normal((nf, L, h)), np.zeros((nf, h, h)),
                             np.ones((nf, h)), np.ones((nf, h)), np.ones(nf), est_covs=True, est_var=True)

    def refused(c, code=VI, get=None, **kw):
        get = get or c.get_state
        before = get()
        with pytest.raises(pkg.VbmfError) as e:
            run(c, **kw)
        assert e.value.code == code, e.value
        after = get()
        for k, v in before.items():
            assert np.array_equal(v, after[k]), k
        return str(e.value)

    with C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32) as c:
        c.set_Y(Y)
        state(c)
        before = c.get_state()
        assert np.all(run(c)["iters"] >= 1)                         # the call itself is fine, 1-column bag included ...
        assert np.all(run(c, fit_bag=(0, 0, 1))["iters"] >= 1)
        after = c.get_state()
        assert all(np.array_equal(v, after[k]) for k, v in before.items())   # ... and leaves the context's state alone
        for bad in ([0, 1, 1, M], [1, 12, M], [0, 12, M - 1], [0, 15, 10, M], [0, M + 1]):
            refused(c, o=np.array(bad, dtype=np.int64), fit_bag=(0,))
        # (Context.fit_batched checks fit_bag itself: the C entry is asked directly)
        p64, dp = (lambda a: a.ctypes.data_as(C.C.POINTER(C.C.c_int64))), C._dptr
        one, st, it = np.ones(64), np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int64)

        def raw(fit_bag, nfits=2, null=None, niter=5):
            fb = np.asarray(fit_bag, dtype=np.int64)
            args = dict(BHat=dp(np.ones(2 * L * H)), SigmaB=dp(np.ones(2 * H * H)), CA=dp(one), CB=dp(one), sigma2=dp(one), iters=p64(it),
                        d=dp(one), status=p64(st), fit_bag=p64(fb))
            if null:
                args[null] = None
            before = c.get_state()
            rc = C.lib().vbmf_fit_batched(c._h, 3, p64(off), nfits, args["fit_bag"], niter, 1e-3, 1, 1, args["BHat"], args["SigmaB"],
                                          args["CA"], args["CB"], args["sigma2"], None, None, args["iters"], args["d"], args["status"], None)
            after = c.get_state()
            assert all(np.array_equal(v, after[k]) for k, v in before.items())
            return rc
        assert raw([1, 2]) == C.VBMF_OK                             # AHat, SigmaA and trace may be NULL
        assert raw([0, 3]) == VI and raw([-1, 0]) == VI             # fit_bag outside 0..nbags-1
        assert raw([1, 2], nfits=0) == VI and raw([1, 2], nfits=-1) == VI
        assert raw([1, 2], niter=0) == VI
        for name in ("BHat", "SigmaB", "CA", "CB", "sigma2", "iters", "d", "status", "fit_bag"):
            assert raw([1, 2], null=name) == VI, name               # a required pointer that is NULL
        refused(c, niter=0)
        state(c, labels0=[0, 5], H1=1)
        assert "mask" in refused(c)
    with C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32) as c:           # no Y
        state(c)
        assert "no Y" in refused(c)
    hyper = dict(alpha0=1e-3, beta0=1e-3, gamma0=1e-3, delta0=1e-3, eta0=1e-3, zeta0=1e-3)
    for v in (C.VBMF_VARIANT_SPARSE_DIAG, C.VBMF_VARIANT_DUAL_DIAG, C.VBMF_VARIANT_TRIAL_DIAG, C.VBMF_VARIANT_SPARSE_DIAGVAR):
        with C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32, variant=v) as c:
            c.set_Y(Y)
            c.sparse_set_state(rng.standard_normal(M * H), np.ones(M * H), np.ones(M * H), np.ones(M * H), rng.standard_normal((L, H)),
                               0.01 * np.eye(H), np.ones(H), np.ones(H), 1.0, 0.5, hyper)
            assert "basic model only" in refused(c, get=c.sparse_get_state)
    with C.Context(L, M, 33, y_dtype=pkg.VBMF_Y_F32) as c:
        c.set_Y(Y)
        state(c, h=33)
        assert "32" in refused(c, code=VU, h=33)
    with C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32, nranks=2, rank=0, L_global=2 * L) as c:
        state(c)
        assert "rank" in refused(c)


# ---- 8. the Python host ------------------------------------------------------------------------------------------------------------------------
def _convert(cls, src):
    dst = cls()
    for f in dataclasses.fields(cls):
        if hasattr(src, f.name):
            setattr(dst, f.name, copy.deepcopy(getattr(src, f.name)))
    return dst


@pytest.mark.parametrize("as_bags", [False, True])
def test_python_host_fills_what_the_per_fit_call_fills(pkg, as_bags):
    """vbmf_batch_ on package parameter sets: every field it fills against the oracle (fp32 storage), restarts on one bag"""
    L, H, Ms = 24, 3, (9, 37)
    Ys = [_bag(L, m, H, i) for i, m in enumerate(Ms)]
    bag_of = [0, 1, 1]
    starts = [_start(Ys[b], H, 60 + k) for k, b in enumerate(bag_of)]
    ps = [_convert(pkg.vbmf_parameters, s) for s in starts]
    held = [(p.CA, p.CB, p.AHat, p.BHat) for p in ps]
    src = pkg.Bags(Ys, H) if as_bags else Ys
    try:
        out = pkg.vbmf_batch_(src, ps, 30, eps=1e-3, est_covs=True, est_var=True, bag_of=bag_of)
    finally:
        if as_bags:
            src.close()
    assert len(out) == 3 and all(a is b for a, b in zip(out, ps))
    worst = {}
    for p, s, b, (ca, cb, a0, b0) in zip(ps, starts, bag_of, held):
        po, do, it, _ = _oracle(Ys[b], s, 30, 1e-3, True, True)
        assert p.iters == it and 2 <= it < 30 and p.status == 0
        assert p.CA is ca and p.CB is cb and p.AHat is not a0 and p.BHat is not b0   # diagonals in place, factors rebound
        worst["d"] = max(worst.get("d", 0.0), abs(p.d - do) / abs(do))
        po.YHat = po.BHat @ po.AHat.T                               # src/vbmf.jl:217
        for k in ("AHat", "BHat", "SigmaA", "SigmaB", "CA", "CB", "invCA", "invCB", "sigma2", "YHat"):
            worst[k] = max(worst.get(k, 0.0), _rel(getattr(p, k), getattr(po, k)))
    _record(f"python host bags={int(as_bags)}", worst)


def test_train_folds_runs_on_the_device(pkg):
    L, H = 24, 3
    folds = [(_bag(L, 9, H, 0), _bag(L, 37, H, 1)), (np.zeros((L, 0)), _bag(L, 5, H, 2))]
    out = pkg.train_folds(folds, "basic", H, 30, eps=1e-3, rng=np.random.default_rng(1))
    assert out[1] == (0, 0)
    rng = np.random.default_rng(1)
    for Y, p in zip(folds[0], out[0]):
        s = pkg.vbmf_init(Y, H, rng=rng)
        q = pkg.vbmf_batch_([Y], [s], 30, eps=1e-3, est_covs=True, est_var=True)[0]
        assert isinstance(p, pkg.vbmf_parameters) and p.status == 0 and 2 <= p.iters < 30
        assert p.iters == q.iters and np.array_equal(p.BHat, q.BHat) and np.array_equal(p.AHat, q.AHat)


# ---- status ------------------------------------------------------------------------------------------------------------------------------------
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
