"""GPU tests of the Gram-form sweep of vbmf_sparse_run ("The ARD-sparse model"): in the diagonal homoscedastic
branch B = Y W with W = sigmaHat A SigmaB, so a sweep reads G = Y'Y instead of streaming Y twice.  A sparse context takes the form under
the size rule of the basic model, and at the small shapes of this file when it is created under VBMF_GRAM=2 (VBMF_GRAM=1 forces the basic
model only); VBMF_GRAM=0 is the streaming path.

Bounds.  tests/test_gpu_sparse.py holds the streaming bf16x2 sparse run to 5e-3 on every field and on sigmaHat, to 2e-2 d + 2e-6 on d and
to 2e-3 on lowerBound; the trace's sigmaHat column takes sigmaHat's bound, its d column d's.  That file has no bound on zeta; zeta is the
noise posterior's rate (sigmaHat = eta / zeta), the sparse model's counterpart of sigma2, and takes tests/test_gpu_gram_path.py's
TOL["sigma2"] = 1e-3.  The only escape is test_gpu_gram_path.py's: where the streaming run itself exceeds a bound, the Gram form stays
within 1.5 x the streaming error (and is not compared with the streaming run on that field); at most two of the parity cases may take it.

Sweep counts: six in the consistent `repeat` layout, three in the reference's (tests/test_gram_sparse_identity.py says why)."""
import copy

import numpy as np
import pytest

import __graft_entry__ as G
from oracle import vbmf_oracle as O
from tests import sparse_entry_reference as R
from tests.helpers import frag_to_rows, relF, report
from tests.test_gpu_stream_passes import TILE_R, U, _f32
from tests.test_gram_sparse_identity import problem

pytestmark = pytest.mark.gpu

E = R.E
BOUND = 5e-3                                         # test_gpu_sparse.py: every field and sigmaHat of the bf16x2 run
ZETA_BOUND = 1e-3                                    # test_gpu_gram_path.py: TOL["sigma2"]
D_BOUND = (2e-2, 2e-6)                               # test_gpu_sparse.py: |d - d_ref| <= 2e-2 d_ref + 2e-6
LB_BOUND = 2e-3                                      # test_gpu_sparse.py: lowerBound
VEC_FIELDS = ("ATVecHat", "diagSigmaATVec", "CA", "beta", "SigmaA_diag", "BHat", "SigmaB", "CB", "delta")
KEYS = VEC_FIELDS + ("sigmaHat", "zeta")
ESCAPES = []                                         # parity cases that took the escape


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


def _ctx(pkg, env, L, M, H, gram, compat=True, variant=None, factor=None):
    cap = pkg.capi
    env.setenv("VBMF_GRAM", "2" if gram else "0")
    rc = cap.VBMF_COMPAT_DEFAULT if compat else (cap.VBMF_COMPAT_DEFAULT & ~cap.VBMF_COMPAT_SPARSE_REPEAT)
    try:
        return cap.Context(L, M, H, y_dtype=pkg.VBMF_Y_BF16, factor_dtype=pkg.VBMF_FACTOR_BF16X2 if factor is None else factor,
                           variant=cap.VBMF_VARIANT_SPARSE_DIAG if variant is None else variant, reference_compat=rc)
    finally:
        env.delenv("VBMF_GRAM")


def _set(c, po):
    hyper = dict(alpha0=po.alpha0, beta0=po.beta0, gamma0=po.gamma0, delta0=po.delta0, eta0=po.eta0, zeta0=po.zeta0)
    c.sparse_set_state(po.ATVecHat, po.diagSigmaATVec, po.CA, po.beta, po.BHat, po.SigmaB, po.CB, po.delta, po.sigmaHat, po.zeta,
                       hyper, labels0=po.labels, H1=po.H1)


def _runs(pkg, env, Y, po, plan, gram=True, compat=True, est_cb=True, bounds=False, between=None):
    """One context; runs (niter, eps) one after the other from the initial state.  Returns [dict(it, d, trace, state, dims[, lb, lbt])]
    and the Y the device holds."""
    L, M = Y.shape
    out = []
    with _ctx(pkg, env, L, M, po.H, gram, compat) as c:
        assert c.dims()["gram"] == (1 if gram else 0)
        c.set_Y(Y)
        _set(c, po)
        for i, (n, eps) in enumerate(plan):
            if between is not None and i > 0:
                between(c)
            it, d, tr = c.sparse_run(n, eps=eps, est_cb=est_cb, want_trace=True)
            r = dict(it=it, d=d, trace=tr.copy(), state=c.sparse_get_state(), dims=c.dims())
            if bounds:
                r["lb"], r["lbt"] = c.sparse_lower_bound(), c.sparse_lower_bound_trimmed(1e-1)
            out.append(r)
        Ys = np.ascontiguousarray(c.get_Y())
    return out, Ys


def _oracle(Ys, po, n, compat, est_cb):
    """n sweeps of the fp64 oracle on the stored Y; returns the reference fields, the trace and the two bounds"""
    q = copy.deepcopy(po)
    q.trYTY = float(np.sum(Ys * Ys))
    tr = []
    O.vbmf_sparse_(Ys, q, n, eps=0.0, full_cov=False, est_cb=est_cb, reference_compat=compat, trace=tr)
    ref = {k: getattr(q, k) for k in KEYS if k != "SigmaA_diag"}
    ref["SigmaA_diag"] = np.diag(q.SigmaA).copy()
    return ref, np.array(tr), O.lowerBound(Ys, q), O.lowerBoundTrimmed(Ys, q, trim=1e-1)


def _errs(r, ref, rtr, lb=None, lbt=None):
    """every measured deviation of one run from a reference, each as (value, bound)"""
    s, tr = r["state"], r["trace"]
    e = {k: (relF(s[k], ref[k]), BOUND) for k in VEC_FIELDS}
    e["sigmaHat"] = (abs(s["sigmaHat"] - ref["sigmaHat"]) / ref["sigmaHat"], BOUND)
    e["zeta"] = (abs(s["zeta"] - ref["zeta"]) / ref["zeta"], ZETA_BOUND)
    # the d column as |dev| / (2e-2 d_ref + 2e-6) (<= 1: within), the sigmaHat column relative
    e["d_tr"] = (float(np.max(np.abs(tr[:, 0] - rtr[:, 0]) / (D_BOUND[0] * rtr[:, 0] + D_BOUND[1]))), 1.0)
    e["sigma_tr"] = (float(np.max(np.abs(tr[:, 1] - rtr[:, 1]) / rtr[:, 1])), BOUND)
    if lb is not None:
        e["lb"] = (abs(r["lb"] - lb) / abs(lb), LB_BOUND)
        e["lbt"] = (abs(r["lbt"] - lbt) / abs(lbt), LB_BOUND)
    return e


def measure_parity(pkg, env, H, M, labels, est_cb, compat):
    """The Gram-form run, the streaming run and the oracle on one problem: {field: (gram vs oracle, streaming vs oracle, gram vs
    streaming, bound)} and the Gram run's state (scripts/gram_sparse_parity.py prints the same figures)."""
    L, n = 7 * M, (3 if compat else 6)
    Y, po = problem(L, M, H, 500 + H, labels)
    (g,), Ys = _runs(pkg, env, Y, po, [(n, 0.0)], True, compat, est_cb, bounds=True)
    (s,), Ys2 = _runs(pkg, env, Y, po, [(n, 0.0)], False, compat, est_cb, bounds=True)
    assert np.array_equal(Ys, Ys2)
    assert g["dims"]["gram"] == 1 and g["dims"]["gram_built"] == 1 and s["dims"]["gram"] == 0 and s["dims"]["gram_built"] == 0
    assert g["it"] == s["it"] == n
    ref, rtr, lb, lbt = _oracle(Ys, po, n, compat, est_cb)
    eg, es = _errs(g, ref, rtr, lb, lbt), _errs(s, ref, rtr, lb, lbt)
    sref = dict(s["state"])
    egs = _errs(g, sref, s["trace"], s["lb"], s["lbt"])
    return {k: (eg[k][0], es[k][0], egs[k][0], eg[k][1]) for k in eg}, g, po


PARITY_SHAPES = [(8, 352), (32, 352), (64, 512), (128, 1024), (32, 353)]


@pytest.mark.parametrize("compat", [False, True], ids=["consistent6", "repeat3"])
@pytest.mark.parametrize("est_cb", [True, False], ids=["cb", "nocb"])
@pytest.mark.parametrize("labels", [False, True], ids=["nolabels", "labels"])
@pytest.mark.parametrize("H,M", PARITY_SHAPES)
def test_parity_with_oracle_and_streaming(pkg, monkeypatch, H, M, labels, est_cb, compat):
    m, g, po = measure_parity(pkg, monkeypatch, H, M, labels, est_cb, compat)
    tag = f"gram sparse {7 * M}x{M} H{H} labels={labels} est_cb={est_cb} compat={compat}"
    report(f"{tag}: " + " ".join(f"{k}={v[0]:.2e}" for k, v in m.items()))
    report(f"{tag} streaming: " + " ".join(f"{k}={v[1]:.2e}" for k, v in m.items()))
    report(f"{tag} gram-streaming: " + " ".join(f"{k}={v[2]:.2e}" for k, v in m.items()))
    bad, escaped = {}, []
    for k, (vg, vs, vgs, b) in m.items():
        if vs > b:                                                     # the streaming run itself is beyond the bound
            escaped.append(k)
            if not vg <= 1.5 * vs:
                bad[k] = (vg, vs, b)
        elif not (vg <= b and vgs <= b):
            bad[k] = (vg, vs, vgs, b)
    if escaped:
        ESCAPES.append((tag, escaped))
    assert not bad, (tag, bad, m)
    assert len(ESCAPES) <= 2, ("more than two cases took the escape", ESCAPES)
    if labels:
        A = g["state"]["ATVecHat"].reshape(M, H)
        assert np.all(A[po.labels, H - po.H1:] == 0.0)
        rest = np.ones((M, H), dtype=bool)
        rest[po.labels, H - po.H1:] = False
        assert np.all(A[rest] != 0.0)


def test_G_at_more_than_one_chunk(pkg, monkeypatch):
    """8 200 rows: two full 4 096-row chunks of G's fp32 accumulation and a ragged one; six sweeps, the bounds above"""
    L, M, H = 8200, 352, 32
    Y, po = problem(L, M, H, 1700, True)
    (g,), Ys = _runs(pkg, monkeypatch, Y, po, [(6, 0.0)], True, False)
    (s,), _ = _runs(pkg, monkeypatch, Y, po, [(6, 0.0)], False, False)
    ref, rtr, _, _ = _oracle(Ys, po, 6, False, True)
    eg, es = _errs(g, ref, rtr), _errs(s, ref, rtr)
    report(f"gram sparse {L}x{M} H{H} chunks: " + " ".join(f"{k}={v[0]:.2e}" for k, v in eg.items()))
    report(f"gram sparse {L}x{M} H{H} chunks streaming: " + " ".join(f"{k}={v[0]:.2e}" for k, v in es.items()))
    bad = {k: (v, es[k][0], b) for k, (v, b) in eg.items() if not v <= (b if es[k][0] <= b else 1.5 * es[k][0])}
    assert not bad, bad


# ---- dispatch -----------------------------------------------------------------------------------------------------------------
def test_dispatch(pkg, monkeypatch):
    """The diagonal homoscedastic sparse model takes the form under VBMF_GRAM=2 and under the size rule, and reports it as a basic
    context does; the grouped models, diag_var, full_cov, H = 130 and the single-bf16 factor keep the streaming sweep; VBMF_GRAM=1
    forces the basic model only."""
    cap = pkg.capi
    L, M, H = 2464, 352, 32
    Y, po = problem(L, M, H, 540)
    with _ctx(pkg, monkeypatch, L, M, H, True) as c:
        assert c.dims()["gram"] == 1 and c.dims()["gram_built"] == 0
        c.set_Y(Y)
        _set(c, po)
        it, _, _ = c.sparse_run(2, eps=0.0)
        d = c.dims()
        assert it == 2 and d["gram"] == 1 and d["gram_built"] == 1 and d["p_frag"] == 1
        c.sparse_set_full_cov(True)
        assert c.dims()["gram"] == 0
        c.sparse_set_full_cov(False)
        assert c.dims()["gram"] == 1
        c.set_Y(Y)
        assert c.dims()["gram_built"] == 0
    for variant in (cap.VBMF_VARIANT_DUAL_DIAG, cap.VBMF_VARIANT_TRIAL_DIAG, cap.VBMF_VARIANT_SPARSE_DIAGVAR):
        with _ctx(pkg, monkeypatch, L, M, H, True, variant=variant) as c:
            assert c.dims()["gram"] == 0, variant
    with _ctx(pkg, monkeypatch, L, M, 130, True) as c:
        assert c.dims()["gram"] == 0                                  # Hp = 256
    with _ctx(pkg, monkeypatch, L, M, H, True, factor=pkg.VBMF_FACTOR_BF16) as c:
        assert c.dims()["gram"] == 0
    monkeypatch.setenv("VBMF_GRAM", "1")
    with cap.Context(L, M, H, y_dtype=pkg.VBMF_Y_BF16, variant=cap.VBMF_VARIANT_SPARSE_DIAG) as c:
        assert c.dims()["gram"] == 0                                  # below the size rule, and 1 forces the basic model only
    monkeypatch.delenv("VBMF_GRAM")
    with cap.Context(L, M, H, y_dtype=pkg.VBMF_Y_BF16, variant=cap.VBMF_VARIANT_SPARSE_DIAG) as c:
        assert c.dims()["gram"] == 0                                  # below the size rule
    with cap.Context(100000, 10000, 64, y_dtype=pkg.VBMF_Y_BF16, variant=cap.VBMF_VARIANT_SPARSE_DIAG) as c:
        assert c.dims()["gram"] == 1                                  # the size rule
    with cap.Context(100000, 10000, 256, y_dtype=pkg.VBMF_Y_BF16, variant=cap.VBMF_VARIANT_SPARSE_DIAG) as c:
        assert c.dims()["gram"] == 0                                  # config 5 itself: H > 128
    monkeypatch.setenv("VBMF_GRAM", "0")
    with cap.Context(100000, 10000, 64, y_dtype=pkg.VBMF_Y_BF16, variant=cap.VBMF_VARIANT_SPARSE_DIAG) as c:
        assert c.dims()["gram"] == 0
    monkeypatch.setenv("VBMF_GRAM", "2")
    with cap.Context(2400, 352, 64, y_dtype=pkg.VBMF_Y_BF16) as c:
        assert c.dims()["gram"] == 1                                  # 2 forces the basic model as 1 does


# ---- one Gram sweep, entry by entry ----------------------------------------------------------------------------------------------
def _block(c, cap, Hp):
    n2 = Hp * Hp
    st = c.peek(cap.PEEK_STATE, 2 * (9 * n2 + 8 + 2 * Hp + 32), dtype=np.float64)
    mat = lambda off: st[off:off + n2].reshape(Hp, Hp).copy()
    return dict(GB=mat(n2), SB=mat(4 * n2 + 8), sig=float(st[9 * n2 + 8 + 2 * Hp]))


@pytest.mark.parametrize("compat", [True, False], ids=["repeat", "consistent"])
@pytest.mark.parametrize("H", [32, 128])
def test_one_gram_sweep_entry_by_entry(pkg, monkeypatch, H, compat):
    """run(1) streams Y and leaves W and P = G W; run(1) again is one Gram-form sweep.  Its ATVecHat and diagSigmaATVec against fp64
    from the P, the state block and the CA table read back between the two runs, per entry, with the bounds
    tests/test_gpu_sparse_entries.py derives for the streaming A update (fp32 diagSigma: one fp32 rounding of an fp64 quotient; A: that,
    the bf16 hi + lo grid of the operand tiles and the fp64 chain, on sigmaHat d |P|; one slab: no split term)."""
    cap = pkg.capi
    M = 353
    L = 7 * M
    Y, po = problem(L, M, H, 2500 + H, True)
    with _ctx(pkg, monkeypatch, L, M, H, True, compat) as c:
        c.set_Y(Y)
        _set(c, po)
        c.sparse_run(1, eps=0.0)
        d = c.dims()
        assert d["gram"] == 1 and d["gram_built"] == 1 and d["p_frag"] == 0
        Hp, XT = d["Hp"], d["XT1"]
        blk = _block(c, cap, Hp)
        s0 = c.sparse_get_state()
        assert blk["sig"] == s0["sigmaHat"]
        P = frag_to_rows(c.peek(cap.PEEK_GRAM_PQ, Hp * XT * 32, dtype=np.float32), M, Hp)
        W = _f32(c, cap, cap.PEEK_GRAM_W, 32 * d["XT1"] * Hp).reshape(-1, Hp)[:M]
        Ys = c.get_Y()
        # what was read back is the sweep's input: P = Y'B = G W of the B the first run left, W = sigmaHat_B A SigmaB
        assert not np.any(P[:, H:]) and not np.any(W[:, H:])
        assert relF(Ys @ W[:, :H], s0["BHat"]) <= 1e-4 and relF(P[:, :H], Ys.T @ s0["BHat"]) <= 1e-4
        c.sparse_run(1, eps=0.0)
        assert c.dims()["p_frag"] == 1
        s1 = c.sparse_get_state(want_B=False)
        A1 = _f32(c, cap, cap.PEEK_A32, 32 * XT * Hp).reshape(32 * XT, Hp)
    v = R.ref_v(blk["sig"], np.diag(blk["GB"])[:H], np.diag(blk["SB"])[:H], L)
    dref, aref, ascale, mask = R.ref_updateA(P[:, :H], np.abs(P[:, :H]), v, s0["CA"].reshape(M, H), blk["sig"], compat,
                                             po.labels, po.H1)
    worst = lambda err, bound: float(np.max(np.where(err == 0.0, 0.0, err / np.maximum(bound, 1e-300))))
    wd = worst(np.abs(s1["diagSigmaATVec"].reshape(M, H) - dref), (U + 16 * E) * dref)
    wa = worst(np.abs(A1[:M, :H] - aref), (U + TILE_R["bf16x2"] + 16 * E) * ascale)
    report(f"gram sparse entries M{M} H{H} compat={compat}: [dS={wd:.3f} A={wa:.3f} of the bound]")
    assert wd <= 1.0 and wa <= 1.0, (wd, wa)
    assert np.array_equal(s1["ATVecHat"].reshape(M, H), A1[:M, :H])
    assert mask.sum() == len(po.labels) * po.H1 and not np.any(A1[:M, :H][mask]) and np.all(A1[:M, :H][~mask] != 0.0)
    assert not np.any(A1[M:]) and not np.any(A1[:, H:])


# ---- run boundaries -----------------------------------------------------------------------------------------------------------------
SHAPES = {16: (2000, 300), 64: (2400, 512), 128: (3000, 1024)}


def _same(tag, a, b):
    for k in KEYS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and np.array_equal(x, y), (tag, k, np.max(np.abs(x - y)))


@pytest.mark.parametrize("H", [16, 64, 128])
def test_split_runs_equal_one_run_bitwise(pkg, monkeypatch, H):
    """run(3) + run(3) equals run(6) bitwise, trace and bounds included: W and P = G W carry over, B is materialised at each end."""
    L, M = SHAPES[H]
    Y, po = problem(L, M, H, 900 + H, True)
    (r6,), _ = _runs(pkg, monkeypatch, Y, po, [(6, 0.0)], bounds=True)
    (ra, rb), _ = _runs(pkg, monkeypatch, Y, po, [(3, 0.0), (3, 0.0)], bounds=True)
    assert r6["it"] == 6 and ra["it"] == rb["it"] == 3
    assert ra["dims"]["p_frag"] == 1 and rb["dims"]["p_frag"] == 1
    _same("run3+run3 vs run6", rb["state"], r6["state"])
    assert rb["d"] == r6["d"] and np.array_equal(np.vstack([ra["trace"], rb["trace"]]), r6["trace"])
    assert rb["lb"] == r6["lb"] and rb["lbt"] == r6["lbt"]
    # the B the first run left is the B of its third sweep
    (r3,), _ = _runs(pkg, monkeypatch, Y, po, [(3, 0.0)])
    _same("run3 of the split vs run3", ra["state"], r3["state"])


@pytest.mark.parametrize("H", [16, 64, 128])
def test_eps_stop_freezes_the_state_of_its_sweep(pkg, monkeypatch, H):
    """An eps stop at sweep k leaves the state of run(k, eps = 0) bitwise; the stop lands at the first sweep whose d is <= eps."""
    L, M = SHAPES[H]
    Y, po = problem(L, M, H, 950 + H)
    n = 12                                                            # past the host's look at the stop flag (every 8 sweeps)
    (r0,), _ = _runs(pkg, monkeypatch, Y, po, [(n, 0.0)])
    assert r0["it"] == n
    d = r0["trace"][:, 0]
    for k in (1, 3, 9):
        eps = float(d[k - 1])
        expect = 1 + int(np.argmax(d <= eps))
        (r,), _ = _runs(pkg, monkeypatch, Y, po, [(n, eps)])
        assert r["it"] == expect and r["d"] == d[expect - 1], (k, r["it"], expect, d)
        assert np.array_equal(r["trace"], r0["trace"][:expect])
        (rk,), _ = _runs(pkg, monkeypatch, Y, po, [(expect, 0.0)])
        assert rk["it"] == expect and np.array_equal(rk["trace"], r["trace"])
        _same(f"eps stop at {expect} vs run({expect})", r["state"], rk["state"])


@pytest.mark.parametrize("what", ["step", "set_state", "fixed_basis"])
def test_a_state_change_between_runs_restarts_by_streaming(pkg, monkeypatch, what):
    """sparse_step, sparse_set_state and sparse_run_fixed_basis drop W: the next run's first sweep streams Y (its Y'B is not the
    fragment-major G W), and what it computes is what the streaming path computes from that state."""
    cap = pkg.capi
    L, M, H = SHAPES[64][0], SHAPES[64][1], 64
    Y, po = problem(L, M, H, 1000)
    mid = {}

    def between(c):
        if what == "step":
            c.sparse_step(cap.SSTEP_CA)
        elif what == "fixed_basis":
            c.sparse_run_fixed_basis(1)
        mid.update(c.sparse_get_state())
        if what == "set_state":
            _set(c, po)

    (ra, rb), Ys = _runs(pkg, monkeypatch, Y, po, [(3, 0.0), (1, 0.0)], between=between)
    assert ra["dims"]["p_frag"] == 1 and rb["dims"]["p_frag"] == 0
    (rc, rd), _ = _runs(pkg, monkeypatch, Y, po, [(3, 0.0), (2, 0.0)], between=between)
    assert rd["dims"]["p_frag"] == 1                                  # ... and the sweep after it is in the Gram form again
    if what == "set_state":
        (r1,), _ = _runs(pkg, monkeypatch, Y, po, [(1, 0.0)])
        _same("set_state between runs", rb["state"], r1["state"])
        return
    # one fp64 sweep from the state the run started from
    q = copy.deepcopy(po)
    q.trYTY = float(np.sum(Ys * Ys))
    for k in ("ATVecHat", "diagSigmaATVec", "CA", "beta", "BHat", "SigmaB", "CB", "delta", "sigmaHat", "zeta"):
        setattr(q, k, copy.deepcopy(mid[k]))
    q.AHat = q.ATVecHat.reshape(M, H).copy()
    q.SigmaA = np.diag(mid["SigmaA_diag"])
    tr = []
    O.vbmf_sparse_(Ys, q, 1, eps=0.0, full_cov=False, trace=tr)
    ref = {k: getattr(q, k) for k in KEYS if k != "SigmaA_diag"}
    ref["SigmaA_diag"] = np.diag(q.SigmaA).copy()
    e = _errs(rb, ref, np.array(tr))
    bad = {k: v for k, v in e.items() if not v[0] <= v[1]}
    assert not bad, (what, bad)
