"""gram_prod_kernel's pipeline edges (csrc/gram_kernels.hpp): the G register ring (4 k-steps deep) and the W / D planes staged
through LDS in chunks of 4 k-steps.  VBMF_GRAM=1 forces the Gram form; run(1) is a streaming sweep that builds G and W, a second
run(1) one Gram-form sweep.  Each shape asserts the split plan it is meant to reach (dims(): gram_nsplit, NH):

* k-steps per split (sps) = 1, 2 and 3 mod the chunk, so the last chunk of every split is partial;
* a last split shorter than the ring depth and the chunk (2 and 3 k-steps);
* one split (NH = 4, no slab buffer: the product writes [P | Q] directly);
* NH = 1, 2 and 4.

On integer data G = Ys'Ys exactly (tests/test_gpu_gram_numerics.py), so P and Q are checked against fp64 products of Ys'Ys with
the W read back, per entry, by the bound of that file's _check_products (restated here).  Rows >= M of P and Q are zero, and a
second context run on the same inputs gives bitwise the same [P | Q]."""
import numpy as np
import pytest

import __graft_entry__ as G
from oracle import vbmf_oracle as O
from tests.helpers import frag_to_rows, report

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


def _plan(M, H):
    """the host's split plan (gram_prepare): NH, GT, nsplit, k-steps per split, k-steps of the last split"""
    Hp = 32 if H <= 32 else (64 if H <= 64 else 128)
    NH = Hp // 32
    XT = -(-M // 32)
    GT = -(-XT // 16) * 16
    KT = 2 * GT
    nrg = GT // (4 * (4 // NH))
    ns = max(1, min(KT // 8, 256 // max(1, nrg)))
    sps = -(-KT // ns)
    ns = -(-KT // sps)
    return NH, GT, ns, sps, KT - (ns - 1) * sps


def _run(pkg, monkeypatch, Y, H, seed):
    L, M = Y.shape
    cap = pkg.capi
    po = O.vbmf_init(Y, H, ca=0.1, cb=0.1, sigma2=0.1, rng=np.random.default_rng(seed), materialize_yhat=False)
    monkeypatch.setenv("VBMF_GRAM", "1")
    c = cap.Context(L, M, H, y_dtype=pkg.VBMF_Y_BF16, factor_dtype=pkg.VBMF_FACTOR_BF16X2)
    monkeypatch.delenv("VBMF_GRAM")
    with c:
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
        Ys = c.get_Y()
        d = c.dims()
    return dict(GT=GT, XT=XT, Hp=Hp, NH=d["NH"], nsplit=d["gram_nsplit"], Ys=Ys, W0=W0, W1=W1, PQ=PQ, n=n)


# (L, M, H, what the shape is for); the plan is asserted against _plan and the property named
CASES = [
    (600, 3086, 64, "sps 1 mod 4, last split 3"),
    (600, 2568, 64, "sps 2 mod 4, last split 2"),
    (600, 4640, 64, "sps 3 mod 4"),
    (600, 4122, 24, "NH 1, sps 3 mod 4, last split 2"),
    (600, 2050, 128, "NH 4, sps 2 mod 4"),
    (600, 3086, 128, "NH 4, sps 1 mod 4"),
    (600, 16400, 128, "NH 4, one split"),
]


@pytest.mark.parametrize("L,M,H,what", CASES)
def test_gram_prod_pipeline_edges(pkg, monkeypatch, L, M, H, what):
    NH, GT, ns, sps, last = _plan(M, H)
    if "mod 4" in what:
        assert sps % 4 == int(what.split("sps ")[1][0]), (what, sps)
    if "last split" in what:
        assert last == int(what.split("last split ")[1][0]) and last < 4, (what, last)
    if "one split" in what:
        assert ns == 1
    Y = np.random.default_rng(5100 + M + H).integers(-3, 4, size=(L, M)).astype(np.float64)
    r = _run(pkg, monkeypatch, Y, H, 5200 + M)
    assert r["NH"] == NH and r["GT"] == GT and r["nsplit"] == ns, (what, r["NH"], r["nsplit"])
    Ys = r["Ys"]
    assert np.array_equal(Ys, Y)                                  # integers are exact in bf16, so G = Ys'Ys exactly
    n, Mp1, Hp = r["n"], 32 * r["XT"], r["Hp"]
    P = frag_to_rows(r["PQ"][:n], Mp1, Hp)
    Q = frag_to_rows(r["PQ"][n:], Mp1, Hp)
    assert not np.any(P[M:]) and not np.any(Q[M:]), what
    # rows checked: all of them on the small shapes, a spread subset (first, last, chunk and split edges) on the one-split shape
    if M <= 5000:
        rows = np.arange(M)
    else:
        edges = (np.arange(0, M, 16 * sps)[1:, None] + np.arange(-8, 8)).ravel()
        rows = np.unique(np.concatenate([np.arange(64), np.arange(M - 64, M), edges, np.arange(0, M, 997)]))
    rows = rows[(rows >= 0) & (rows < M)]
    Wr = r["W1"][:32 * GT]
    D = (r["W1"] - r["W0"]).astype(np.float32).astype(np.float64)[:32 * GT]
    Gr = np.zeros((len(rows), 32 * GT))
    Gr[:, :M] = Ys[:, rows].T @ Ys                                # integer sums below 2^53: exact in fp64
    assert np.abs(Gr).max() < 2 ** 24
    # the bound of test_gpu_gram_numerics._check_products: |P - GW| <= (6 sps + nsplit + 4) u (|G||W|),
    # |Q - GD| <= (2^-16 + (3 sps + nsplit + 4) u) (|G||D|)
    kP = (6 * sps + ns + 4) * U
    kQ = 2.0 ** -16 + (3 * sps + ns + 4) * U
    GW, GD = Gr @ Wr, Gr @ D
    aGW, aGD = np.abs(Gr) @ np.abs(Wr), np.abs(Gr) @ np.abs(D)
    eP, eQ = np.abs(P[rows] - GW), np.abs(Q[rows] - GD)
    worstP = float(np.max(eP / np.maximum(aGW, 1e-300)))
    worstQ = float(np.max(eQ / np.maximum(aGD, 1e-300)))
    report(f"gram_prod pipeline {what} ({L}x{M} H{H}): nsplit {ns}, sps {sps}, last {last}: P_entry={worstP:.2e} "
           f"Q_entry={worstQ:.2e}")
    assert np.all(eP <= kP * aGW), (what, worstP, kP)
    assert np.all(eQ <= kQ * aGD), (what, worstQ, kQ)
    # the same inputs through a second context: bitwise the same product
    r2 = _run(pkg, monkeypatch, Y, H, 5200 + M)
    assert np.array_equal(r2["PQ"].view(np.uint32), r["PQ"].view(np.uint32)), what
