"""GPU tests of the Gram-form sweep of vbmf_sparse_run at rank 256 (Hp = 256, NH = 8; DESIGN.md section 10, "Rank 256").  The form is
opt-in there: contexts are made with bf16 Y, bf16x2 factors and VBMF_VARIANT_SPARSE_DIAG, then vbmf_set_gram_form(VBMF_GRAM_FORM_ON);
VBMF_GRAM is not set.  The streaming run of the same build (VBMF_GRAM_FORM_OFF) and the fp64 oracle on the Y the device stores are the
references; data, bounds and helpers are those of tests/test_gpu_gram_sparse.py, tests/test_gpu_gram_numerics.py and
tests/test_gpu_gram_partials.py.

The split plan asserted here (gram_prepare): the product runs as two h-tile groups of the NH = 4 geometry, w = 2 (GT / 4) workgroups per
split; the split count is the s <= min(KT / 8, 4) with the smallest ceil(w s / 256) / s, the smaller s on a tie.  M = 353: GT = 16, w = 8,
four splits of 8 k-steps; M = 2093: GT = 80, w = 40, four splits of 40; one split from GT = 400 on (w = 200), i.e. M >= 12289."""
import copy

import numpy as np
import pytest

import __graft_entry__ as G
from oracle import vbmf_oracle as O
from tests import sparse_entry_reference as R
from tests.helpers import frag_to_rows, gram_frag_to_matrix, relF, report
from tests.test_gpu_stream_passes import TILE_R, U, _f32
from tests.test_gram_sparse_identity import problem
from tests.test_gpu_gram_numerics import _check_products, _int_data
from tests.test_gpu_gram_sparse import KEYS, _block, _errs, _oracle, _same, _set

pytestmark = pytest.mark.gpu

E = R.E
ESCAPES = []                                         # parity cases that took the escape: at most one


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


@pytest.fixture(autouse=True)
def _no_gram_env(monkeypatch):
    monkeypatch.delenv("VBMF_GRAM", raising=False)


def _ctx(pkg, L, M, H, form="on", compat=True, variant=None, factor=None):
    """A context of the shapes' storage with the form set by the public switch (form None: never called)."""
    cap = pkg.capi
    rc = cap.VBMF_COMPAT_DEFAULT if compat else (cap.VBMF_COMPAT_DEFAULT & ~cap.VBMF_COMPAT_SPARSE_REPEAT)
    c = cap.Context(L, M, H, y_dtype=pkg.VBMF_Y_BF16, factor_dtype=pkg.VBMF_FACTOR_BF16X2 if factor is None else factor,
                    variant=cap.VBMF_VARIANT_SPARSE_DIAG if variant is None else variant, reference_compat=rc)
    if form is not None:
        c.set_gram_form({"default": cap.VBMF_GRAM_FORM_DEFAULT, "off": cap.VBMF_GRAM_FORM_OFF, "on": cap.VBMF_GRAM_FORM_ON}[form])
    return c


def _runs(pkg, Y, po, plan, form="on", compat=True, est_cb=True, bounds=False, between=None, ctx=None):
    """tests/test_gpu_gram_sparse.py's _runs with the form taken from vbmf_set_gram_form"""
    L, M = Y.shape
    out = []
    with (ctx if ctx is not None else _ctx(pkg, L, M, po.H, form, compat)) as c:
        if ctx is None:
            assert c.dims()["gram"] == (1 if form == "on" else 0)
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


# ---- 1. dispatch ----------------------------------------------------------------------------------------------------------------
def test_dispatch(pkg, monkeypatch):
    """VBMF_GRAM_FORM_ON admits the diagonal homoscedastic sparse model at Hp = 256 and nothing else there; DEFAULT and OFF do not;
    ON at H = 32 is VBMF_GRAM=2; VBMF_GRAM=3 at creation is ON; an unknown mode is refused."""
    cap = pkg.capi
    L, M = 2464, 352
    for H in (130, 256):
        with _ctx(pkg, L, M, H, None) as c:
            assert c.dims()["Hp"] == 256 and c.dims()["gram"] == 0
            c.set_gram_form(cap.VBMF_GRAM_FORM_ON)
            assert c.dims()["gram"] == 1 and c.dims()["gram_built"] == 0
            c.set_gram_form(cap.VBMF_GRAM_FORM_OFF)
            assert c.dims()["gram"] == 0
            c.set_gram_form(cap.VBMF_GRAM_FORM_ON)
            c.set_gram_form(cap.VBMF_GRAM_FORM_DEFAULT)
            assert c.dims()["gram"] == 0
            c.set_gram_form(cap.VBMF_GRAM_FORM_ON)
            c.sparse_set_full_cov(True)
            assert c.dims()["gram"] == 0
            c.sparse_set_full_cov(False)
            assert c.dims()["gram"] == 1
            with pytest.raises(pkg.VbmfError) as ei:
                c.set_gram_form(7)
            assert ei.value.code == -1                                 # VBMF_ERR_INVALID, and nothing changed
            assert c.dims()["gram"] == 1
    with cap.Context(L, M, 256, y_dtype=pkg.VBMF_Y_BF16, factor_dtype=pkg.VBMF_FACTOR_BF16X2) as c:
        c.set_gram_form(cap.VBMF_GRAM_FORM_ON)
        assert c.dims()["gram"] == 0                                   # the basic model at Hp = 256 streams
    for variant in (cap.VBMF_VARIANT_DUAL_DIAG, cap.VBMF_VARIANT_TRIAL_DIAG, cap.VBMF_VARIANT_SPARSE_DIAGVAR):
        with _ctx(pkg, L, M, 256, "on", variant=variant) as c:
            assert c.dims()["gram"] == 0, variant
    with _ctx(pkg, L, M, 32, "on", factor=pkg.VBMF_FACTOR_BF16) as c:  # (the single-bf16 factor exists up to H = 128)
        assert c.dims()["gram"] == 0
    with cap.Context(L, M, 256, y_dtype=pkg.VBMF_Y_F32, variant=cap.VBMF_VARIANT_SPARSE_DIAG) as c:
        c.set_gram_form(cap.VBMF_GRAM_FORM_ON)
        assert c.dims()["gram"] == 0                                   # fp32 storage
    # ON at H = 32 is what VBMF_GRAM=2 gives, bit for bit
    Y, po = problem(L, M, 32, 540)
    monkeypatch.setenv("VBMF_GRAM", "2")
    c2 = _ctx(pkg, L, M, 32, None)
    monkeypatch.delenv("VBMF_GRAM")
    (a,), _ = _runs(pkg, Y, po, [(3, 0.0)], ctx=c2)
    (b,), _ = _runs(pkg, Y, po, [(3, 0.0)], "on")
    assert a["dims"]["gram"] == b["dims"]["gram"] == 1 and a["dims"]["p_frag"] == b["dims"]["p_frag"] == 1
    _same("ON vs VBMF_GRAM=2", a["state"], b["state"])
    assert np.array_equal(a["trace"], b["trace"])
    # VBMF_GRAM=3 at creation is ON, rank 256 included
    Y, po = problem(L, M, 256, 541)
    monkeypatch.setenv("VBMF_GRAM", "3")
    c3 = _ctx(pkg, L, M, 256, None)
    monkeypatch.delenv("VBMF_GRAM")
    assert c3.dims()["gram"] == 1
    (a,), _ = _runs(pkg, Y, po, [(3, 0.0)], ctx=c3)
    (b,), _ = _runs(pkg, Y, po, [(3, 0.0)], "on")
    assert a["dims"]["gram"] == b["dims"]["gram"] == 1 and a["dims"]["p_frag"] == b["dims"]["p_frag"] == 1
    _same("ON vs VBMF_GRAM=3", a["state"], b["state"])
    assert np.array_equal(a["trace"], b["trace"])


# ---- 2. parity with the oracle and with the streaming run ---------------------------------------------------------------------------
def measure_parity(pkg, H, M, labels, est_cb, compat):
    """tests/test_gpu_gram_sparse.py's measure_parity with the two runs told apart by vbmf_set_gram_form: {field: (gram vs oracle,
    streaming vs oracle, gram vs streaming, bound)} (scripts/gram_sparse_parity.py prints the same figures)"""
    L, n = 7 * M, (3 if compat else 6)
    Y, po = problem(L, M, H, 500 + H, labels)
    (g,), Ys = _runs(pkg, Y, po, [(n, 0.0)], "on", compat, est_cb, bounds=True)
    (s,), Ys2 = _runs(pkg, Y, po, [(n, 0.0)], "off", compat, est_cb, bounds=True)
    assert np.array_equal(Ys, Ys2)
    assert g["dims"]["gram"] == 1 and g["dims"]["gram_built"] == 1 and s["dims"]["gram"] == 0 and s["dims"]["gram_built"] == 0
    assert g["dims"]["p_frag"] == 1 and s["dims"]["p_frag"] == 0
    assert g["it"] == s["it"] == n
    ref, rtr, lb, lbt = _oracle(Ys, po, n, compat, est_cb)
    eg, es = _errs(g, ref, rtr, lb, lbt), _errs(s, ref, rtr, lb, lbt)
    egs = _errs(g, dict(s["state"]), s["trace"], s["lb"], s["lbt"])
    return {k: (eg[k][0], es[k][0], egs[k][0], eg[k][1]) for k in eg}, g, po


PARITY_CASES = [(256, 1024, True, True), (256, 1024, True, False), (256, 1025, False, True), (130, 1040, True, True)]


@pytest.mark.parametrize("compat", [False, True], ids=["consistent6", "repeat3"])
@pytest.mark.parametrize("H,M,labels,est_cb", PARITY_CASES)
def test_parity_with_oracle_and_streaming(pkg, H, M, labels, est_cb, compat):
    m, g, po = measure_parity(pkg, H, M, labels, est_cb, compat)
    tag = f"gram sparse h256 {7 * M}x{M} H{H} labels={labels} est_cb={est_cb} compat={compat}"
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
    assert len(ESCAPES) <= 1, ("more than one case took the escape", ESCAPES)
    if labels:
        A = g["state"]["ATVecHat"].reshape(M, H)
        assert np.all(A[po.labels, H - po.H1:] == 0.0)
        rest = np.ones((M, H), dtype=bool)
        rest[po.labels, H - po.H1:] = False
        assert np.all(A[rest] != 0.0)


# ---- 3. one Gram sweep, entry by entry ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compat", [True, False], ids=["repeat", "consistent"])
@pytest.mark.parametrize("H", [256, 130])
def test_one_gram_sweep_entry_by_entry(pkg, H, compat):
    """tests/test_gpu_gram_sparse.py's test of the same name at Hp = 256: run(1) streams Y and leaves W and P = G W; run(1) again is one
    Gram-form sweep (sparse_update_a_frag_kernel<., 8>), its ATVecHat and diagSigmaATVec held per entry to fp64 from the P, the state
    block and the CA table read back between the two runs."""
    cap = pkg.capi
    M = 353
    L = 7 * M
    Y, po = problem(L, M, H, 2500 + H, True)
    with _ctx(pkg, L, M, H, "on", compat) as c:
        c.set_Y(Y)
        _set(c, po)
        c.sparse_run(1, eps=0.0)
        d = c.dims()
        assert d["gram"] == 1 and d["gram_built"] == 1 and d["p_frag"] == 0 and d["Hp"] == 256 and d["gram_nsplit"] == 4
        Hp, XT = d["Hp"], d["XT1"]
        blk = _block(c, cap, Hp)
        s0 = c.sparse_get_state()
        assert blk["sig"] == s0["sigmaHat"]
        P = frag_to_rows(c.peek(cap.PEEK_GRAM_PQ, Hp * XT * 32, dtype=np.float32), M, Hp)
        W = _f32(c, cap, cap.PEEK_GRAM_W, 32 * d["XT1"] * Hp).reshape(-1, Hp)[:M]
        Ys = c.get_Y()
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
    report(f"gram sparse h256 entries M{M} H{H} compat={compat}: [dS={wd:.3f} A={wa:.3f} of the bound]")
    assert wd <= 1.0 and wa <= 1.0, (wd, wa)
    assert np.array_equal(s1["ATVecHat"].reshape(M, H), A1[:M, :H])
    assert mask.sum() == len(po.labels) * po.H1 and not np.any(A1[:M, :H][mask]) and np.all(A1[:M, :H][~mask] != 0.0)
    assert not np.any(A1[M:]) and not np.any(A1[:, H:])


# ---- 4. products and partials after one Gram sweep ----------------------------------------------------------------------------------
def _sweep(pkg, Y, po, rows=None, want_G=True):
    """One streaming sweep, then one Gram-form sweep; G (all, or the row tiles holding `rows`), W_old, W_new, [P | Q], A32, the
    sigmaHat SigmaB table and the state's [GB | GD | GX] read back."""
    cap = pkg.capi
    L, M = Y.shape
    with _ctx(pkg, L, M, po.H, "on") as c:
        c.set_Y(Y)
        _set(c, po)
        c.sparse_run(1, eps=0.0)
        d = c.dims()
        assert d["gram"] == 1 and d["gram_built"] == 1 and d["p_frag"] == 0
        Hp, XT = d["Hp"], d["XT1"]
        GT = (XT + 15) // 16 * 16
        nW = 32 * GT * Hp
        W0 = c.peek(cap.PEEK_GRAM_W, nW, dtype=np.float32).reshape(-1, Hp).astype(np.float64)
        c.sparse_run(1, eps=0.0)
        d = c.dims()
        assert d["p_frag"] == 1
        W1 = c.peek(cap.PEEK_GRAM_W, nW, dtype=np.float32).reshape(-1, Hp).astype(np.float64)
        n, n2 = Hp * XT * 32, Hp * Hp
        PQ = c.peek(cap.PEEK_GRAM_PQ, 2 * n, dtype=np.float32).copy()
        A32 = c.peek(cap.PEEK_A32, M * Hp, dtype=np.float32).reshape(M, Hp).astype(np.float64)
        SB32 = c.peek(cap.PEEK_SB32, n2, dtype=np.float32).reshape(Hp, Hp).astype(np.float64)
        st = c.peek(cap.PEEK_STATE, 2 * (3 * n2 + 8), dtype=np.float64).copy()
        tile_words = 2 * GT * 64 * 8
        Gm = None
        if want_G and rows is None:
            Gm = gram_frag_to_matrix(c.peek(cap.PEEK_GRAM_G, GT * tile_words, dtype=np.float32), GT)
        elif want_G:
            Gm = {}
            for p in sorted({r // 32 for r in rows}):
                T = gram_frag_to_matrix(c.peek(cap.PEEK_GRAM_G, tile_words, offset=p * tile_words, dtype=np.float32), GT)
                for r in rows:
                    if r // 32 == p:
                        Gm[r] = T[r - 32 * p].astype(np.float64)
        Ys = c.get_Y() if want_G else None
    return dict(M=M, H=po.H, GT=GT, XT=XT, Hp=Hp, NH=d["NH"], nsplit=d["gram_nsplit"], G=Gm, Ys=Ys, W0=W0, W1=W1, A=A32, SB32=SB32,
                P=frag_to_rows(PQ[:n], 32 * XT, Hp), Q=frag_to_rows(PQ[n:], 32 * XT, Hp),
                GB=st[n2:2 * n2].reshape(Hp, Hp), GD=st[2 * n2:3 * n2].reshape(Hp, Hp), GX=st[3 * n2])


def _check_partials(tag, r):
    """gram_w_cols, the blocked gram_tail and gram_part_reduce: tests/test_gpu_gram_partials.py's checks"""
    M, H, Hp = r["M"], r["H"], r["Hp"]
    assert Hp == 256 and r["NH"] == 8
    W = r["W1"][:M]
    D = (W - r["W0"][:M]).astype(np.float32).astype(np.float64)
    assert not np.any(r["W1"][M:]) and not np.any(r["W1"][:, H:]), "rows >= M and columns >= H of W stay zero"
    Wref = (r["A"] @ r["SB32"]).astype(np.float32).astype(np.float64)          # the table already holds sigmaHat SigmaB
    rel = lambda a, b: np.linalg.norm(a - b) / np.linalg.norm(b)
    P, Q = r["P"][:M], r["Q"][:M]
    WP, DQ = W.T @ P, D.T @ Q
    eW, eB, eD = rel(W, Wref), rel(r["GB"], 0.5 * (WP + WP.T)), rel(r["GD"], 0.5 * (DQ + DQ.T))
    tr = np.sum(r["A"] * P)
    eX = abs(r["GX"] - tr) / np.sum(np.abs(r["A"] * P))
    report(f"gram sparse h256 partials {tag}: W={eW:.2e} GB={eB:.2e} GD={eD:.2e} GX={eX:.2e}")
    assert eW < 1e-6 and eB < 1e-12 and eD < 1e-12 and eX <= 1e-12, (tag, eW, eB, eD, eX)
    assert np.array_equal(r["GB"], r["GB"].T) and np.array_equal(r["GD"], r["GD"].T)
    for k in ("P", "Q"):
        assert not np.any(r[k][M:]) and not np.any(r[k][:, H:]), (tag, k)
    for k in ("GB", "GD"):
        assert not np.any(r[k][H:]) and not np.any(r[k][:, H:]), (tag, k)


def _repeatable(a, b, keys=("W0", "W1", "P", "Q", "A", "SB32", "GB", "GD")):
    for k in keys:
        assert np.array_equal(a[k], b[k]), k
    assert a["GX"] == b["GX"]


@pytest.mark.parametrize("H,M,L", [(256, 8 * 256 + 45, 5 * (8 * 256 + 45)), (256, 353, 7 * 353), (130, 353, 7 * 353)])
def test_products_and_partials_entry_by_entry(pkg, H, M, L):
    Y, po = problem(L, M, H, 2700 + H + M, True)
    r = _sweep(pkg, Y, po)
    assert r["nsplit"] == 4, r["nsplit"]
    tag = f"{L}x{M} H{H}"
    Gm = r["G"].astype(np.float64)
    assert not np.any(Gm[M:]) and not np.any(Gm[:, M:]) and np.array_equal(Gm, Gm.T)
    assert relF(Gm[:M, :M], r["Ys"].T @ r["Ys"]) < 1e-6
    _check_products(tag, r, Gm, None)
    _check_partials(tag, r)
    b = _sweep(pkg, Y, po)
    _repeatable(r, b)
    assert np.array_equal(r["G"], b["G"])


def test_products_and_partials_single_split(pkg):
    """M = 12 320 (GT = 400): 200 workgroups per split leave gram_prod one split, so there is no slab buffer, the two h-tile groups
    write [P | Q] directly and gram_tail reads it in place.  Integer data in [-3, 3]: G is exact; it is 655 MB and is checked on a
    row subset holding the first and last rows, both sides of every row-group edge (128 rows) and the zero padding."""
    L, M, H = 512, 12320, 256
    Y = _int_data(L, M, 3500)
    po = O.vbmf_sparse_init(Y, H, ca=0.1, cb=0.1, sigma=0.1, rng=np.random.default_rng(3501), full_cov=False, materialize_yhat=False,
                            H1=2, labels=[0, 5, 17, M - 1])
    edges = [e for b in range(128, M, 128) for e in (b - 1, b)]
    rows = sorted(set([0, 1, M - 1, M, 32 * ((M + 31) // 32) - 1] + edges))
    r = _sweep(pkg, Y, po, rows=rows)
    assert r["nsplit"] == 1 and r["GT"] == 400
    Ys = r["Ys"]
    assert np.array_equal(Ys, Y)
    n = 32 * r["GT"]
    for i in rows:
        ref = np.zeros(n)
        if i < M:
            ref[:M] = Ys[:, i] @ Ys
        assert np.array_equal(r["G"][i], ref), i
    tag = f"int {L}x{M} H{H} one split"
    _check_products(tag, r, np.array([r["G"][i] for i in rows]), rows)
    _check_partials(tag, r)
    b = _sweep(pkg, Y, po, want_G=False)
    _repeatable(r, b)


# ---- 5. run boundaries ----------------------------------------------------------------------------------------------------------------
SHAPES = {256: (3000, 1024), 130: (2400, 520)}


@pytest.mark.parametrize("H", [256, 130])
def test_split_runs_equal_one_run_bitwise(pkg, H):
    """run(3) + run(3) equals run(6) bitwise, trace and bounds included.  No control chain of a Gram-form run is forked onto the side
    stream (sparse_run_impl): a chain still running beside the next sweep's sparse_v would show here."""
    L, M = SHAPES[H]
    Y, po = problem(L, M, H, 900 + H, True)
    (r6,), _ = _runs(pkg, Y, po, [(6, 0.0)], bounds=True)
    (ra, rb), _ = _runs(pkg, Y, po, [(3, 0.0), (3, 0.0)], bounds=True)
    assert r6["it"] == 6 and ra["it"] == rb["it"] == 3
    assert ra["dims"]["p_frag"] == 1 and rb["dims"]["p_frag"] == 1
    _same("run3+run3 vs run6", rb["state"], r6["state"])
    assert rb["d"] == r6["d"] and np.array_equal(np.vstack([ra["trace"], rb["trace"]]), r6["trace"])
    assert rb["lb"] == r6["lb"] and rb["lbt"] == r6["lbt"]
    (r3,), _ = _runs(pkg, Y, po, [(3, 0.0)])
    _same("run3 of the split vs run3", ra["state"], r3["state"])
    (r6b,), _ = _runs(pkg, Y, po, [(6, 0.0)], bounds=True)             # and the run repeats itself
    _same("run6 twice", r6b["state"], r6["state"])
    assert np.array_equal(r6b["trace"], r6["trace"])


@pytest.mark.parametrize("H", [256, 130])
def test_eps_stop_freezes_the_state_of_its_sweep(pkg, H):
    """An eps stop at sweep k leaves the state of run(k, eps = 0) bitwise; the stop lands at the first sweep whose d is <= eps."""
    L, M = SHAPES[H]
    Y, po = problem(L, M, H, 950 + H)
    n = 12                                                            # past the host's look at the stop flag (every 8 sweeps)
    (r0,), _ = _runs(pkg, Y, po, [(n, 0.0)])
    assert r0["it"] == n
    d = r0["trace"][:, 0]
    for k in (1, 3, 9):
        eps = float(d[k - 1])
        expect = 1 + int(np.argmax(d <= eps))
        (r,), _ = _runs(pkg, Y, po, [(n, eps)])
        assert r["it"] == expect and r["d"] == d[expect - 1], (k, r["it"], expect, d)
        assert np.array_equal(r["trace"], r0["trace"][:expect])
        (rk,), _ = _runs(pkg, Y, po, [(expect, 0.0)])
        assert rk["it"] == expect and np.array_equal(rk["trace"], r["trace"])
        _same(f"eps stop at {expect} vs run({expect})", r["state"], rk["state"])


@pytest.mark.parametrize("what", ["step", "set_state", "fixed_basis"])
def test_a_state_change_between_runs_restarts_by_streaming(pkg, what):
    """sparse_step, sparse_set_state and sparse_run_fixed_basis drop W: the next run's first sweep streams Y, the sweep after it is in
    the Gram form again, and what the streamed sweep computes is what the streaming path computes from that state."""
    cap = pkg.capi
    H = 256
    L, M = SHAPES[H]
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

    (ra, rb), Ys = _runs(pkg, Y, po, [(3, 0.0), (1, 0.0)], between=between)
    assert ra["dims"]["p_frag"] == 1 and rb["dims"]["p_frag"] == 0
    (rc, rd), _ = _runs(pkg, Y, po, [(3, 0.0), (2, 0.0)], between=between)
    assert rd["dims"]["p_frag"] == 1
    if what == "set_state":
        (r1,), _ = _runs(pkg, Y, po, [(1, 0.0)])
        _same("set_state between runs", rb["state"], r1["state"])
        return
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
