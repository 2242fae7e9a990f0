"""Many ARD-sparse / two-group fits in one launch (vbmf_sparse_fit_batched, vbmf_sparse_batch_, vbmf_dual_batch_): every fit's whole
vbmf_sparse! / vbmf_dual! loop in one workgroup, against the oracle's loop on Y as stored (get_Y) from the same start values -- field by
field, sweep counts and the trace of d included -- plus the independence of the fits from each other and the C ABI's refusals."""
import copy
import dataclasses
import os

import numpy as np
import pytest

import __graft_entry__ as G
from oracle import vbmf_oracle as O

pytestmark = pytest.mark.gpu

# Largest relative error per field against the oracle measured on an MI355X over every case of this file (profiles/fit_batch_parity.txt).
# Asserted: 3 x the figure, at least FLOOR, and never above CAP -- an fp32 intermediate shows up at 1e-7, which CAP must catch.
MEASURED = dict(BHat=3.65e-13, SigmaB=4.64e-13, CB=1.04e-12, delta=7.20e-13, sigmaHat=3.23e-13, zeta=3.23e-13, CA=2.13e-13, beta=5.42e-13,
                diagSigmaATVec=3.40e-13, ATVecHat=2.35e-13, SigmaA=2.73e-13, priors=8.27e-14, d=2.21e-12, trace_d=2.21e-12)
FLOOR, CAP, FACTOR = 1e-12, 1e-8, 3.0
TOL = {k: max(FACTOR * v, FLOOR) for k, v in MEASURED.items()}
assert all(v <= CAP for v in TOL.values())

FIELDS = ("BHat", "SigmaB", "CB", "delta", "sigmaHat", "zeta", "CA", "beta", "diagSigmaATVec", "ATVecHat", "SigmaA")
REPORT = os.path.join(G.ROOT, "build", "fit_batch_parity.txt")           # (build/ is not tracked)
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
    """a rank-H matrix plus noise (an all-noise bag for H = 0 would not converge; this is what a trained class looks like)"""
    rng = np.random.default_rng(1000 + seed)
    return _f32(rng.standard_normal((L, H)) @ rng.standard_normal((H, M)) + 0.1 * rng.standard_normal((L, M)))


def _start(kind, Y, H, seed):
    """the oracle's init with default_rng(seed): the start values of both sides"""
    rng = np.random.default_rng(seed)
    if kind == "sparse":
        return O.vbmf_sparse_init(Y, H, rng=rng, full_cov=False, materialize_yhat=False)
    return O.vbmf_dual_init(Y, H, max(1, H // 2), rng=rng, materialize_yhat=False)


def _oracle(kind, Y, p0, niter, eps, full_cov, compat=True, est_cb=True, est_priors=True):
    p = copy.deepcopy(p0)
    tr = []
    if kind == "sparse":
        d, it = O.vbmf_sparse_(Y, p, niter, eps=eps, full_cov=full_cov, reference_compat=compat, trace=tr, est_cb=est_cb)
    else:
        d, it = O.vbmf_dual_(Y, p, niter, eps=eps, full_cov=full_cov, reference_compat=compat, trace=tr, est_cb=est_cb,
                             est_priors=est_priors)
    return p, d, it, np.array([t[0] for t in tr])


def _oracle_frobenius(kind, Y, p0, niter, eps, full_cov, compat=True):
    """the sparse model's loop (src/vbmf_sparse.jl:364-378) with d in Frobenius norms: what the library computes when
    VBMF_COMPAT_SPECTRAL_DELTA is off (the oracle's own delta is the operator 2-norm)"""
    assert kind == "sparse"
    p = copy.deepcopy(p0)
    old, d, tr = p.BHat.copy(), eps + 1.0, []
    while len(tr) < niter and d > eps:
        O.sparse_updateA(Y, p, full_cov=full_cov, reference_compat=compat)
        O.sparse_updateB(Y, p)
        O.sparse_updateCA(p)
        O.sparse_updateCB(p)
        O.sparse_updateSigma(Y, p)
        d = float(np.linalg.norm(p.BHat - old) / np.linalg.norm(old))
        old = p.BHat.copy()
        tr.append(d)
    return p, d, len(tr), np.array(tr)


class Call:
    """bags side by side in one context (fp32 storage), Y as stored per bag"""

    def __init__(self, pkg, Ys, H, kind, compat=None):
        C = pkg.capi
        self.C, self.H, self.kind = C, H, kind
        self.off = np.concatenate([[0], np.cumsum([Y.shape[1] for Y in Ys])]).astype(np.int64)
        L, M = Ys[0].shape[0], int(self.off[-1])
        kw = {} if compat is None else dict(reference_compat=compat)
        self.ctx = C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32, **kw,
                             variant=C.VBMF_VARIANT_SPARSE_DIAG if kind == "sparse" else C.VBMF_VARIANT_DUAL_DIAG)
        self.ctx.set_Y(np.concatenate(Ys, axis=1))
        Yall = self.ctx.get_Y()
        self.Ys = [np.ascontiguousarray(Yall[:, a:b]) for a, b in zip(self.off[:-1], self.off[1:])]

    def run(self, starts, bag_of, niter, eps, full_cov, est_cb=True, est_priors=True):
        """starts: the oracle's parameter sets; returns the library's dict"""
        H, dual = self.H, self.kind == "dual"
        pri = [[p.alpha00, p.beta00, p.alpha01, p.beta01] if dual else [p.alpha0, p.beta0, p.alpha0, p.beta0] for p in starts]
        return self.ctx.sparse_fit_batched(
            self.off, bag_of, niter, eps, [p.gamma for p in starts], [p.delta0 for p in starts], [p.eta for p in starts],
            [p.zeta0 for p in starts], pri, np.stack([p.BHat for p in starts]), np.stack([p.SigmaB for p in starts]),
            np.stack([p.CB for p in starts]), [p.sigmaHat for p in starts], np.concatenate([p.CA for p in starts]),
            H0=starts[0].H0 if dual else H, full_cov=full_cov, est_cb=est_cb, est_priors=dual and est_priors, want_trace=True)

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


def _compare(tag, call, r, starts, bag_of, niter, eps, full_cov, compat=True, want_iters=None, oracle=_oracle):
    """every fit of the call against the oracle: the fields, the priors, the sweep count, the trace of d; returns the worst errors"""
    H, worst, s0 = call.H, {}, 0
    for f, (p0, b) in enumerate(zip(starts, bag_of)):
        po, d, it, trd = oracle(call.kind, call.Ys[b], p0, niter, eps, full_cov, compat)
        s1 = s0 + po.M * H
        e = {k: _rel(v, getattr(po, k)) for k, v in _fit_fields(r, f, s0, s1).items()}
        if call.kind == "dual":
            e["priors"] = _rel(r["priors4"][f], [po.alpha00, po.beta00, po.alpha01, po.beta01])
        assert r["iters"][f] == it, (tag, f, int(r["iters"][f]), it, r["trace"][f, :, 0], trd)
        assert r["status"][f] == 0, (tag, f)
        if want_iters is not None:
            assert it in want_iters, (tag, f, it)
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


# ---- 1. the diagonal form, fixed sweeps ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("repeat", [True, False])
@pytest.mark.parametrize("kind", ["sparse", "dual"])
def test_diagonal_fixed_sweeps(pkg, kind, repeat):
    L, H, Ms = 24, 3, (37, 2, 9, 64)
    C = pkg.capi
    call = Call(pkg, [_bag(L, m, H, i) for i, m in enumerate(Ms)], H, kind,
                compat=None if repeat else C.VBMF_COMPAT_SPECTRAL_DELTA)
    try:
        bag_of = [b for b in range(len(Ms)) for _ in range(3)]
        starts = [_start(kind, call.Ys[b], H, 10 * b + k) for b in range(len(Ms)) for k in range(3)]
        r = call.run(starts, bag_of, 8, 0.0, False)
        _compare(f"diag {kind} repeat={int(repeat)}", call, r, starts, bag_of, 8, 0.0, False, compat=repeat)
        assert np.all(r["iters"] == 8)
    finally:
        call.close()


# ---- 2. the stop test, full_cov -------------------------------------------------------------------------------------------------------
STOP_EPS, STOP_NITER = 1e-3, 30
STOP_SHAPES = ((24, 37, 3), (166, 64, 5), (7, 30, 1), (50, 1, 2))
# six starts per shape.  The test asserts on the oracle that no sweep's d of these seeds lies within 1 % of eps (with these bags the
# closest is 2.5 %: dual, (166, 64, 5), seed 2); a seed that did would have to be replaced, never the case dropped
STOP_SEEDS = (0, 1, 2, 3, 4, 5)


@pytest.mark.parametrize("kind", ["sparse", "dual"])
def test_stop_test_full_cov(pkg, kind):
    for si, (L, M, H) in enumerate(STOP_SHAPES):
        call = Call(pkg, [_bag(L, M, H, 20 + si)], H, kind)
        try:
            starts = [_start(kind, call.Ys[0], H, s) for s in STOP_SEEDS]
            for p0 in starts:                                       # the margin, on the oracle alone
                trd = _oracle(kind, call.Ys[0], p0, STOP_NITER, STOP_EPS, True)[3]
                assert np.all(np.abs(trd - STOP_EPS) > 0.01 * STOP_EPS), (kind, si, trd)
            r = call.run(starts, [0] * 6, STOP_NITER, STOP_EPS, True)
            _compare(f"stop {kind} {(L, M, H)}", call, r, starts, [0] * 6, STOP_NITER, STOP_EPS, True)
            if M == 1:
                assert np.all(r["iters"] == STOP_NITER)             # the 1-column bag never meets eps
            else:
                assert np.all(r["iters"] < STOP_NITER)
        finally:
            call.close()


# ---- 3. the tier edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sparse", "dual"])
@pytest.mark.parametrize("shape,full_cov,niter", [((40, 21, 16), True, 6), ((33, 20, 17), True, 6), ((33, 20, 17), False, 3)])
def test_tier_edges(pkg, kind, shape, full_cov, niter):
    L, M, H = shape
    call = Call(pkg, [_bag(L, M, H, 40 + H)], H, kind)
    try:
        starts = [_start(kind, call.Ys[0], H, s) for s in (0, 1)]
        r = call.run(starts, [0, 0], niter, 0.0, full_cov)
        _compare(f"tier {kind} {shape} full={int(full_cov)}", call, r, starts, [0, 0], niter, 0.0, full_cov)
    finally:
        call.close()


# ---- 4. state in global memory beside state in LDS -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sparse", "dual"])
def test_global_state_beside_lds_state(pkg, kind):
    L, H, Ms = 12, 3, (2500, 5)
    call = Call(pkg, [_bag(L, m, H, 50 + i) for i, m in enumerate(Ms)], H, kind)
    try:
        bag_of = [0, 1, 0, 1]
        starts = [_start(kind, call.Ys[b], H, 3 + k) for k, b in enumerate(bag_of)]
        r = call.run(starts, bag_of, 4, 0.0, False)
        _compare(f"global+lds {kind}", call, r, starts, bag_of, 4, 0.0, False)
    finally:
        call.close()


# ---- 5. independence ------------------------------------------------------------------------------------------------------------------------
def _same(r, f, s, q, g, t):
    """fit f of call r (its M H-long fields at s) equals fit g of call q (at t), bit for bit"""
    for k in ("BHat", "SigmaB", "CB", "delta", "sigmaHat", "zeta", "SigmaA", "priors4", "iters", "d", "status", "trace"):
        assert np.array_equal(r[k][f], q[k][g], equal_nan=True), k
    for k in ("CA", "beta", "diagSigmaATVec", "ATVecHat"):
        assert np.array_equal(r[k][s], q[k][t], equal_nan=True), k


@pytest.mark.parametrize("full_cov", [False, True])
def test_independence(pkg, full_cov):
    L, H, Ms = 24, 3, (37, 2, 9, 64)
    call = Call(pkg, [_bag(L, m, H, i) for i, m in enumerate(Ms)], H, "dual")
    try:
        me = _start("dual", call.Ys[0], H, 77)
        others = [_start("dual", call.Ys[b], H, 100 + k) for k, b in enumerate([1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3])]
        ob = [1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3]
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


# ---- 6. an all-zero bag among normal ones ------------------------------------------------------------------------------------------------------
def test_zero_bag(pkg):
    L, H = 24, 3
    Ya, Yb, Z = _bag(L, 9, H, 2), _bag(L, 37, H, 0), np.zeros((L, 11))
    with_z, without = Call(pkg, [Ya, Z, Yb], H, "sparse"), Call(pkg, [Ya, Yb], H, "sparse")
    try:
        sa, sz, sb = _start("sparse", Ya, H, 5), _start("sparse", Z, H, 6), _start("sparse", Yb, H, 7)
        po, d, it, _ = _oracle("sparse", Z, sz, 8, 1e-3, False)
        assert it == 2 and np.isnan(d)                              # what the reference's loop does on a zero matrix
        r = with_z.run([sa, sz, sb], [0, 1, 2], 8, 1e-3, False)
        q = without.run([sa, sb], [0, 1], 8, 1e-3, False)
        assert r["iters"][1] == 2 and np.isnan(r["d"][1])
        na, nz, nb = 9 * H, 11 * H, 37 * H
        _same(r, 0, slice(0, na), q, 0, slice(0, na))
        _same(r, 2, slice(na + nz, na + nz + nb), q, 1, slice(na, na + nb))
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
    hyper = dict(alpha0=1e-3, beta0=1e-3, gamma0=1e-3, delta0=1e-3, eta0=1e-3, zeta0=1e-3)
    rng = np.random.default_rng(3)

    def state(c, h=H, **kw):
        c.sparse_set_state(rng.standard_normal(M * h), np.ones(M * h), np.ones(M * h), np.ones(M * h), rng.standard_normal((L, h)),
                           0.01 * np.eye(h), np.ones(h), np.ones(h), 1.0, 0.5, hyper, **kw)

    def run(c, o=off, fit_bag=(1, 2), niter=5, h=H, H0=None, full_cov=False):
        nf, fb = len(fit_bag), np.asarray(fit_bag, dtype=np.int64)
        w = np.diff(np.asarray(o))
        mh = int(sum(w[b] for b in fb if 0 <= b < len(w))) * h
        return c.sparse_fit_batched(o, fb, niter, 1e-3, np.full(nf, 12.0), np.full(nf, 1e-3), np.full(nf, 100.0), np.full(nf, 1e-3),
                                    np.full((nf, 4), 1e-3), rng.standard_normal((nf, L, h)), np.zeros((nf, h, h)), np.ones((nf, h)),
                                    np.ones(nf), np.ones(mh), H0=H0, full_cov=full_cov)

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

    with C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32, variant=C.VBMF_VARIANT_SPARSE_DIAG) as c:
        c.set_Y(Y)
        state(c)
        assert np.all(run(c)["iters"] >= 1)                         # the call itself is fine
        for bad in ([0, 1, 1, M], [1, 12, M], [0, 12, M - 1], [0, 15, 10, M], [0, M + 1]):
            refused(c, o=np.array(bad, dtype=np.int64), fit_bag=(0,), full_cov=True)
        # (Context.sparse_fit_batched checks fit_bag itself: the C entry is asked directly)
        p64, dp = (lambda a: a.ctypes.data_as(C.C.POINTER(C.C.c_int64))), C._dptr
        one, st, it = np.ones(64), np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int64)

        def raw(fit_bag, nfits=2, null=False):
            fb = np.asarray(fit_bag, dtype=np.int64)
            before = c.sparse_get_state()
            rc = C.lib().vbmf_sparse_fit_batched(c._h, 3, p64(off), nfits, p64(fb), 5, 1e-3, 1, 1, 0, H, dp(one), dp(one), dp(one), dp(one),
                                                 dp(one), None if null else dp(np.ones(2 * L * H)), dp(np.ones(2 * H * H)), dp(one), dp(one),
                                                 dp(np.ones(2 * M * H)), None, None, None, None, None, None, p64(it), dp(one),
                                                 p64(st), None)
            after = c.sparse_get_state()
            assert all(np.array_equal(v, after[k]) for k, v in before.items())
            return rc
        assert raw([0, 3]) == VI and raw([-1, 0]) == VI             # fit_bag outside 0..nbags-1
        assert raw([1, 2], nfits=0) == VI
        assert raw([1, 2], null=True) == VI                         # a required pointer that is NULL
        refused(c, niter=0)
        refused(c, H0=0)
        refused(c, H0=H + 1)
        assert "1-column" in refused(c, fit_bag=(0, 1))             # the diagonal form under the repeat layout needs M >= 2 ...
        assert np.all(run(c, fit_bag=(0, 1), full_cov=True)["iters"] >= 1)   # ... full_cov does not
        state(c, labels0=[0, 5], H1=1)
        assert "mask" in refused(c)
    with C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32) as c:
        c.set_state(np.ones((M, H)), np.ones((L, H)), np.eye(H), np.eye(H), np.ones(H), np.ones(H), 1.0)
        assert "basic" in refused(c, get=c.get_state)
    for v in (C.VBMF_VARIANT_SPARSE_DIAGVAR, C.VBMF_VARIANT_DUAL_DIAGVAR, C.VBMF_VARIANT_TRIAL_DIAGVAR):
        with C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32, variant=v) as c:
            state(c)
            assert "diag_var" in refused(c)
    with C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32, variant=C.VBMF_VARIANT_TRIAL_DIAG) as c:
        state(c)
        assert "trial" in refused(c)
    with C.Context(L, M, 33, y_dtype=pkg.VBMF_Y_F32, variant=C.VBMF_VARIANT_SPARSE_DIAG) as c:
        state(c, h=33)
        assert "32" in refused(c, code=VU, h=33)
    with C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32, nranks=2, rank=0, L_global=2 * L, variant=C.VBMF_VARIANT_SPARSE_DIAG) as c:
        state(c)
        assert "rank" in refused(c)


# ---- the Python hosts ------------------------------------------------------------------------------------------------------------------------------
def _convert(cls, src):
    dst = cls()
    for f in dataclasses.fields(cls):
        if hasattr(src, f.name):
            setattr(dst, f.name, copy.deepcopy(getattr(src, f.name)))
    return dst


@pytest.mark.parametrize("kind", ["sparse", "dual"])
def test_python_host_fills_what_the_per_fit_call_fills(pkg, kind):
    """vbmf_sparse_batch_ / vbmf_dual_batch_ on package parameter sets: the fields of every set against the oracle (fp32 storage)"""
    L, H, Ms = 24, 3, (9, 37)
    Ys = [_bag(L, m, H, i) for i, m in enumerate(Ms)]
    P = pkg.vbmf_sparse_parameters if kind == "sparse" else pkg.vbmf_dual_parameters
    bag_of = [0, 1, 1]
    starts = [_start(kind, Ys[b], H, 60 + k) for k, b in enumerate(bag_of)]
    ps = [_convert(P, s) for s in starts]
    fit = pkg.vbmf_sparse_batch_ if kind == "sparse" else pkg.vbmf_dual_batch_
    ds = fit(Ys, ps, 8, eps=0.0, full_cov=False, bag_of=bag_of)
    names = FIELDS + (("alpha00", "beta00", "alpha01", "beta01", "alpha0", "alpha1", "CA0", "CA1", "beta0", "beta1") if kind == "dual" else ())
    key = lambda k: (k if k in TOL else "priors" if k.startswith("alpha") or k in ("beta00", "beta01") else
                     "CA" if k.startswith("CA") else "beta" if k.startswith("beta") else "ATVecHat")
    worst = {}
    for p, s, b, d in zip(ps, starts, bag_of, ds):
        po, do, it, _ = _oracle(kind, Ys[b], s, 8, 0.0, False)
        assert p.iters == it == 8 and p.status == 0
        worst["d"] = max(worst.get("d", 0.0), abs(d - do) / abs(do))
        for k in names + ("AHat",):
            worst[key(k)] = max(worst.get(key(k), 0.0), _rel(getattr(p, k), getattr(po, k)))
    _record(f"python host {kind}", worst)


def test_fit_restarts_runs_on_the_device(pkg):
    L, M, H = 24, 37, 3
    Y = _bag(L, M, H, 0)
    p = pkg.fit_restarts(Y, H, 30, model="dual", H0=1, nstarts=3, eps=1e-3, rng=np.random.default_rng(1))
    assert isinstance(p, pkg.vbmf_dual_parameters) and p.status == 0 and 1 <= p.iters < 30
    assert np.linalg.norm(p.AHat, 2) + np.linalg.norm(p.BHat, 2) >= 1e-2
    p = pkg.fit_restarts(Y, H, 30, model="sparse", nstarts=3, eps=1e-3, full_cov=True, rng=np.random.default_rng(1))
    assert isinstance(p, pkg.vbmf_sparse_parameters) and p.iters >= 1


# ---- paths the cases above do not take ------------------------------------------------------------------------------------------------------------
def test_frobenius_d_without_the_spectral_bit(pkg):
    """reference_compat = 0: d = ||B - B_old||_F / ||B_old||_F under full_cov, the stop test on it"""
    L, M, H = 24, 37, 3
    call = Call(pkg, [_bag(L, M, H, 20)], H, "sparse", compat=0)
    try:
        starts = [_start("sparse", call.Ys[0], H, s) for s in STOP_SEEDS]
        for p0 in starts:
            trd = _oracle_frobenius("sparse", call.Ys[0], p0, STOP_NITER, STOP_EPS, True, False)[3]
            assert np.all(np.abs(trd - STOP_EPS) > 0.01 * STOP_EPS), trd
        r = call.run(starts, [0] * 6, STOP_NITER, STOP_EPS, True)
        _compare("frobenius d", call, r, starts, [0] * 6, STOP_NITER, STOP_EPS, True, compat=False, oracle=_oracle_frobenius)
        assert np.all(r["iters"] < STOP_NITER)
    finally:
        call.close()


def test_without_est_cb_and_est_priors(pkg):
    L, H, Ms = 24, 3, (37, 9)
    call = Call(pkg, [_bag(L, m, H, i) for i, m in enumerate(Ms)], H, "dual")
    try:
        bag_of = [0, 1, 0]
        starts = [_start("dual", call.Ys[b], H, 30 + k) for k, b in enumerate(bag_of)]
        r = call.run(starts, bag_of, 8, 0.0, False, est_cb=False, est_priors=False)
        fixed = lambda *a: _oracle(*a, est_cb=False, est_priors=False)
        _compare("est_cb=0 est_priors=0", call, r, starts, bag_of, 8, 0.0, False, oracle=fixed)
        for f, p0 in enumerate(starts):                             # neither CB nor the hyper-priors moved
            assert np.array_equal(r["CB"][f], p0.CB)
            assert np.array_equal(r["priors4"][f], [p0.alpha00, p0.beta00, p0.alpha01, p0.beta01])
    finally:
        call.close()


@pytest.mark.parametrize("full_cov", [False, True])
def test_status_of_a_fit_that_meets_a_non_finite_precision(pkg, full_cov):
    """a NaN noise precision in one fit: status 1 after its first sweep, the call succeeds, the neighbours are what they are without it"""
    L, H, Ms = 24, 3, (37, 9)
    call = Call(pkg, [_bag(L, m, H, i) for i, m in enumerate(Ms)], H, "sparse")
    try:
        good = [_start("sparse", call.Ys[b], H, 40 + b) for b in (0, 1)]
        sick = _start("sparse", call.Ys[0], H, 42)
        sick.sigmaHat = float("nan")
        r = call.run([good[0], sick, good[1]], [0, 0, 1], 8, 1e-3, full_cov)
        q = call.run(good, [0, 1], 8, 1e-3, full_cov)
        assert list(r["status"]) == [0, 1, 0] and r["iters"][1] == 1
        n0, n1 = Ms[0] * H, Ms[1] * H
        _same(r, 0, slice(0, n0), q, 0, slice(0, n0))
        _same(r, 2, slice(2 * n0, 2 * n0 + n1), q, 1, slice(n0, n0 + n1))
    finally:
        call.close()
