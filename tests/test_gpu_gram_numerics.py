"""The Gram form's kernels against fp64, entry by entry (csrc/gram_kernels.hpp).  VBMF_GRAM=1 forces the
form; run(1) is a streaming sweep that builds G and W, a second run(1) is one Gram-form sweep.  Then G, W_old, W_new and
[P | Q] = G [W_new | D] are read back (D = fp32(W_new - W_old), formed as gram_w forms it).

* G on integer data in [-3, 3]: exact in bf16, every product and every chunk sum is an integer below 2^24, so G must equal
  Ys'Ys BITWISE, zero padding included.  Rounding cannot hide a dropped or doubled row, k-step, chunk, tile or mirror.
* G on real-valued data: a per-entry bound from the chunked fp32 accumulation (gram_bound), and a Frobenius figure.
* P = G W (six-term product) and Q = G D (three-term product) against fp64 products of the G and W read back, per entry.
* The split-K geometry of gram_prod: NH = 1, 2, 4; an uneven last split that holds real rows; one split (no slab buffer,
  the product writes [P | Q] directly).  Each case asserts the nsplit it is meant to reach."""
import numpy as np
import pytest

import __graft_entry__ as G
from oracle import vbmf_oracle as O
from tests.helpers import frag_to_rows, gram_frag_to_matrix, report

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
CHUNK_KSTEPS = 256                 # GRAM_CHUNK: k-steps of 16 rows accumulated in fp32 before the fp64 fold


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


def _int_data(L, M, seed):
    return np.random.default_rng(seed).integers(-3, 4, size=(L, M)).astype(np.float64)


def _real_data(L, M, H, seed):
    """tests/test_gpu_gram_path.py's separated problem"""
    rng = np.random.default_rng(seed)
    _, A, B = O.toy_matrix(L, M, H, 0.05, rng)
    return (B * np.linspace(1.0, 3.0, H)) @ A.T + 0.05 * rng.standard_normal((L, M))


def _sweep(pkg, monkeypatch, Y, H, seed, rows=None):
    """One streaming sweep, then one Gram-form sweep; G (all of it, or only the row tiles holding `rows`), W and [P | Q] read
    back.  Returns G as a dict {row: fp64 row of length 32 GT} when `rows` is given, else the 32 GT x 32 GT matrix."""
    L, M = Y.shape
    cap = pkg.capi
    po = O.vbmf_init(Y, H, ca=0.1, cb=0.1, sigma2=0.1, rng=np.random.default_rng(seed), materialize_yhat=False)
    monkeypatch.setenv("VBMF_GRAM", "1")
    c = cap.Context(L, M, H, y_dtype=pkg.VBMF_Y_BF16, factor_dtype=pkg.VBMF_FACTOR_BF16X2)
    monkeypatch.delenv("VBMF_GRAM")
    with c:
        with pytest.raises(pkg.VbmfError):
            c.peek(cap.PEEK_GRAM_G, 1)                                 # no G before the first run that takes the form
        c.set_Y(Y)
        c.set_state(po.AHat, po.BHat, po.SigmaA, po.SigmaB, np.diag(po.CA), np.diag(po.CB), po.sigma2)
        c.run(1, eps=0.0, est_covs=True, est_var=True)
        d = c.dims()
        assert d["gram"] == 1 and d["gram_built"] == 1
        Hp, XT = d["Hp"], d["XT1"]
        GT = (XT + 15) // 16 * 16
        nW = 32 * GT * Hp
        W0 = c.peek(cap.PEEK_GRAM_W, nW, dtype=np.float32).reshape(-1, Hp).astype(np.float64)
        c.run(1, eps=0.0, est_covs=True, est_var=True)
        W1 = c.peek(cap.PEEK_GRAM_W, nW, dtype=np.float32).reshape(-1, Hp).astype(np.float64)
        n = Hp * XT * 32
        PQ = c.peek(cap.PEEK_GRAM_PQ, 2 * n, dtype=np.float32)
        tile_words = 2 * GT * 64 * 8
        with pytest.raises(pkg.VbmfError):
            c.peek(cap.PEEK_GRAM_G, 1, offset=GT * tile_words)          # the peek knows G's size
        if rows is None:
            Gm = gram_frag_to_matrix(c.peek(cap.PEEK_GRAM_G, GT * tile_words, dtype=np.float32), GT)
        else:
            Gm = {}
            for p in sorted({r // 32 for r in rows}):
                T = gram_frag_to_matrix(c.peek(cap.PEEK_GRAM_G, tile_words, offset=p * tile_words, dtype=np.float32), GT)
                for r in rows:
                    if r // 32 == p:
                        Gm[r] = T[r - 32 * p].astype(np.float64)
        Ys = c.get_Y()
        d = c.dims()
    return dict(GT=GT, XT=XT, Hp=Hp, NH=d["NH"], nsplit=d["gram_nsplit"], G=Gm, Ys=Ys, W0=W0, W1=W1,
                P=frag_to_rows(PQ[:n], 32 * XT, Hp), Q=frag_to_rows(PQ[n:], 32 * XT, Hp))


def _splits(r):
    """gram_prod's k-steps per split, as the host plans them (dims()["gram_nsplit"] is asserted separately)"""
    KT = 2 * r["GT"]
    return -(-KT // r["nsplit"])


def _check_products(tag, r, Grows, rows):
    """P = G W_new and Q = G D against fp64 products of the G read back, on `rows` (all rows of [P | Q] when None).

    P: G (fp32) splits exactly into three bf16 parts and so does W; the six products kept drop terms below 2^-26 |G||W|.  The
    MFMA products are exact in fp32 and every fp32 addition into the accumulator costs at most one rounding u = 2^-24 of a value
    bounded by (|G||W|): six MFMAs per k-step over the split's k-steps, one addition per split in the slab fold and the final
    fp32 store: |P - GW| <= (6 sps + nsplit + 4) u (|G||W|).  Q: D keeps two bf16 parts and only hi.hi, hi.lo, lo.hi are formed,
    so each term carries up to 3 x 2^-18 relative: |Q - GD| <= (2^-16 + (3 sps + nsplit + 4) u) (|G||D|)."""
    W = r["W1"]
    D = (r["W1"] - r["W0"]).astype(np.float32).astype(np.float64)
    Mp1 = 32 * r["XT"]
    if rows is None:
        rows = np.arange(Mp1)
    rows = np.asarray(rows)
    rows = rows[rows < Mp1]
    GR = Grows[: len(rows)]
    sps, ns = _splits(r), r["nsplit"]
    kP = (6 * sps + ns + 4) * U
    kQ = 2.0 ** -16 + (3 * sps + ns + 4) * U
    P, Q = r["P"][rows], r["Q"][rows]
    GW, GD = GR @ W, GR @ D
    aGW, aGD = np.abs(GR) @ np.abs(W), np.abs(GR) @ np.abs(D)
    eP, eQ = np.abs(P - GW), np.abs(Q - GD)
    worstP = float(np.max(eP / np.maximum(aGW, 1e-300)))
    worstQ = float(np.max(eQ / np.maximum(aGD, 1e-300)))
    relP = float(np.linalg.norm(P - GW) / np.linalg.norm(GW))
    relQ = float(np.linalg.norm(Q - GD) / np.linalg.norm(GD))
    report(f"gram numerics {tag} products: P_entry={worstP:.2e} P_fro={relP:.2e} Q_entry={worstQ:.2e} Q_fro={relQ:.2e}"
           f"  [nsplit {ns}, sps {sps}]")
    assert np.all(eP <= kP * aGW), (tag, worstP, kP)
    assert np.all(eQ <= kQ * aGD), (tag, worstQ, kQ)
    # the rows >= M of P and Q are exactly zero
    M = r["M"]
    assert not np.any(r["P"][M:]) and not np.any(r["Q"][M:]), tag
    return relP, relQ


# (L, M, H, expected gram_nsplit, uneven last split): L below one chunk (3000), exactly two chunks (8192), three chunks + 37 rows (a ragged chunk
# with a partial k-step), ~10 chunks (41 003); M = 1 mod 32 (257, 545, 4769, 4609), a multiple of 128 (384), several
# 128-blocks; Hp = 32 / 64 / 128 (NH = 1 / 2 / 4).  4769 at Hp = 64 (12 splits of 27, the last of 23) and 4609 at Hp = 128
# (6 of 54, the last of 50) end on an uneven split that holds real rows.
INT_CASES = [(3000, 257, 24, 4, False), (8192, 384, 64, 4, False), (12325, 545, 100, 8, False), (41003, 1000, 12, 8, False),
             (5000, 4769, 64, 12, True), (3000, 4609, 128, 6, True)]


@pytest.mark.parametrize("L,M,H,nsplit,uneven", INT_CASES)
def test_gram_exact_on_integer_data(pkg, monkeypatch, L, M, H, nsplit, uneven):
    Y = _int_data(L, M, 3100 + M)
    r = _sweep(pkg, monkeypatch, Y, H, 3200 + M)
    r["M"] = M
    assert r["nsplit"] == nsplit and r["NH"] == r["Hp"] // 32
    last = 2 * r["GT"] - (nsplit - 1) * _splits(r)
    assert (last < _splits(r)) == uneven
    if uneven:
        assert (nsplit - 1) * _splits(r) < (M + 15) // 16, "the last split holds real rows"
    Ys = r["Ys"]
    assert np.array_equal(Ys, Y)                                  # integers are exact in bf16
    n = 32 * r["GT"]
    ref = np.zeros((n, n))
    ref[:M, :M] = Ys.T @ Ys                                       # integer sums below 2^53: exact in fp64
    assert np.abs(ref).max() < 2 ** 24
    bad = np.argwhere(r["G"] != ref)
    assert bad.size == 0, (f"{len(bad)} entries of G differ from Ys'Ys", bad[:8].tolist())
    _check_products(f"int {L}x{M} H{H}", r, r["G"].astype(np.float64), None)


def test_gram_exact_single_split_large_M(pkg, monkeypatch):
    """M = 16 400 at H = 128: 132 row groups leave gram_prod one split, so there is no slab buffer and the product writes
    [P | Q] directly.  G is 1.1 GB: it is checked on a row subset (= a column subset, G is symmetric) holding the first and
    last rows, both sides of every 128-block edge and the zero padding."""
    L, M, H = 600, 16400, 128
    Y = _int_data(L, M, 3300)
    edges = [e for b in range(128, M, 128) for e in (b - 1, b)]
    rows = sorted(set([0, 1, M - 1, M, 32 * ((M + 31) // 32) - 1] + edges))
    r = _sweep(pkg, monkeypatch, Y, H, 3301, rows=rows)
    r["M"] = M
    assert r["nsplit"] == 1 and r["NH"] == 4
    Ys = r["Ys"]
    n = 32 * r["GT"]
    for i in rows:
        ref = np.zeros(n)
        if i < M:
            ref[:M] = Ys[:, i] @ Ys
        assert np.array_equal(r["G"][i], ref), i
    Grows = np.array([r["G"][i] for i in rows])
    _check_products(f"int {L}x{M} H{H} one split", r, Grows, rows)


def gram_bound(KS):
    """Per-entry bound on G from real-valued bf16 data: the products are exact in fp32; a chunk of at most min(256, KS) k-steps
    adds one 16-product MFMA per k-step into an fp32 accumulator, at most two roundings of u (|Ys|'|Ys|) each (the MFMA's
    internal sum and the accumulation), so a chunk is off by at most 2 min(256, KS) u times its share of |Ys|'|Ys|; the chunks
    are folded in fp64 (error below 2^-40) and the sum is rounded to fp32 once (u).  |G - G64| <= gamma (|Ys|'|Ys|) with
    gamma = (2 min(256, KS) + 2) u, the extra u for the fp64 fold."""
    return (2 * min(CHUNK_KSTEPS, KS) + 2) * U


def test_gram_real_data_against_fp64(pkg, monkeypatch):
    L, M, H = 41003, 1000, 64
    Y = _real_data(L, M, H, 3400)
    r = _sweep(pkg, monkeypatch, Y, H, 3401)
    r["M"] = M
    assert r["nsplit"] == 8
    Ys = r["Ys"]
    G64 = Ys.T @ Ys
    aYY = np.abs(Ys).T @ np.abs(Ys)
    Gd = r["G"][:M, :M].astype(np.float64)
    assert not np.any(r["G"][M:]) and not np.any(r["G"][:, M:])
    gamma = gram_bound((L + 15) // 16)
    ratio = float(np.max(np.abs(Gd - G64) / aYY))
    fro = float(np.linalg.norm(Gd - G64) / np.linalg.norm(G64))
    report(f"gram numerics real {L}x{M} H{H} G: entry={ratio:.2e} fro={fro:.2e}")
    assert ratio <= gamma, (ratio, gamma)
    # 3 x the figures measured on an MI355X (G 1.10e-7, P 7.0e-8, Q 1.13e-6)
    assert fro < 3.3e-7, fro
    relP, relQ = _check_products(f"real {L}x{M} H{H}", r, r["G"].astype(np.float64), None)
    assert relP < 2.1e-7 and relQ < 3.4e-6, (relP, relQ)
