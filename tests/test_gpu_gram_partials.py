"""GPU tests of the Gram form's fp64 kernels (gram_w, gram_part, gram_part_reduce).  After one Gram-form
sweep W must equal fp32(A (SigmaB / sigma2)), and the state's [B'B | dB'dB | tr(B'YA)] slots must equal an fp64 recomputation
from the W, [P | Q] and A the sweep left on the device: B'B = sym(W'P), dB'dB = sym(D'Q) with D = fp32(W - W_old),
tr = sum A o P.  Those are fp64 sums of exact fp32 products, so only the summation order differs.  Shapes force the form
(VBMF_GRAM=1) at Hp = 32, 64, 128 with M a multiple of neither the row chunk nor the 4-row MFMA step."""
import numpy as np
import pytest

import __graft_entry__ as G
from oracle import vbmf_oracle as O
from tests.helpers import frag_to_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


def _sweep(pkg, monkeypatch, L, M, H, seed):
    rng = np.random.default_rng(seed)
    _, A, B = O.toy_matrix(L, M, H, 0.05, rng)
    Y = (B * np.linspace(1.0, 3.0, H)) @ A.T + 0.05 * rng.standard_normal((L, M))
    po = O.vbmf_init(Y, H, ca=0.1, cb=0.1, sigma2=0.1, rng=np.random.default_rng(seed + 1), materialize_yhat=False)
    monkeypatch.setenv("VBMF_GRAM", "1")
    c = pkg.capi.Context(L, M, H, y_dtype=pkg.VBMF_Y_BF16, factor_dtype=pkg.VBMF_FACTOR_BF16X2)
    monkeypatch.delenv("VBMF_GRAM")
    cap = pkg.capi
    with c:
        c.set_Y(Y)
        c.set_state(po.AHat, po.BHat, po.SigmaA, po.SigmaB, np.diag(po.CA), np.diag(po.CB), po.sigma2)
        c.run(1, eps=0.0, est_covs=True, est_var=True)          # streaming sweep; leaves W and G W
        d = c.dims()
        assert d["gram"] == 1 and d["gram_built"] == 1
        Hp, XT = d["Hp"], d["XT1"]
        nW = ((XT + 15) // 16) * 16 * 32 * Hp           # 32 GT rows, GT = XT rounded up to 16
        W0 = c.peek(cap.PEEK_GRAM_W, nW, dtype=np.float32).copy()
        n2 = Hp * Hp
        sig2 = c.peek(cap.PEEK_STATE, 2, offset=2 * (9 * n2 + 8 + 2 * Hp), dtype=np.float64)[0]   # sigma2 the sweep's SigmaB uses
        c.run(1, eps=0.0, est_covs=True, est_var=True)          # one Gram-form sweep
        W1 = c.peek(cap.PEEK_GRAM_W, nW, dtype=np.float32).copy()
        PQ = c.peek(cap.PEEK_GRAM_PQ, 2 * Hp * XT * 32, dtype=np.float32).copy()
        A32 = c.peek(cap.PEEK_A32, M * Hp, dtype=np.float32).copy()
        st = c.peek(cap.PEEK_STATE, 2 * (5 * n2 + 8), dtype=np.float64).copy()
    n = Hp * XT * 32
    return dict(M=M, Hp=Hp, W0=W0.reshape(-1, Hp), W1=W1.reshape(-1, Hp), P=PQ[:n], Q=PQ[n:], A=A32.reshape(M, Hp),
                GB=st[n2:2 * n2].reshape(Hp, Hp), GD=st[2 * n2:3 * n2].reshape(Hp, Hp), GX=st[3 * n2],
                S=(st[4 * n2 + 8:5 * n2 + 8] / sig2).astype(np.float32).reshape(Hp, Hp))


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@pytest.mark.parametrize("H", [24, 64, 100])
def test_partials_match_fp64_recomputation(pkg, monkeypatch, H):
    M = 8 * max(H, 32) + 45                     # not a multiple of any row chunk, nor of the 4-row step
    r = _sweep(pkg, monkeypatch, 5 * M, M, H, 900 + H)
    M, Hp = r["M"], r["Hp"]
    assert Hp == {24: 32, 64: 64, 100: 128}[H]
    W = r["W1"][:M].astype(np.float64)
    D = (W - r["W0"][:M].astype(np.float64)).astype(np.float32).astype(np.float64)
    assert not np.any(r["W1"][M:]), "rows >= M of W must stay zero"
    # gram_w: W = fp32(A (SigmaB / sigma2)) with the fp32 table the sweep used (SigmaB slot / sigma2, rounded as ctrl_cov rounds it)
    Wref = (r["A"].astype(np.float64) @ r["S"].astype(np.float64)).astype(np.float32).astype(np.float64)
    assert _rel(W, Wref) < 1e-6
    P, Q = frag_to_rows(r["P"], M, Hp), frag_to_rows(r["Q"], M, Hp)
    WP, DQ = W.T @ P, D.T @ Q
    assert _rel(r["GB"], 0.5 * (WP + WP.T)) < 1e-12
    assert _rel(r["GD"], 0.5 * (DQ + DQ.T)) < 1e-12
    tr = np.sum(r["A"].astype(np.float64) * P)
    assert abs(r["GX"] - tr) <= 1e-12 * np.sum(np.abs(r["A"].astype(np.float64) * P))
    assert np.array_equal(r["GB"], r["GB"].T) and np.array_equal(r["GD"], r["GD"].T)


@pytest.mark.parametrize("H", [24, 64, 100])
def test_partials_bitwise_repeatable(pkg, monkeypatch, H):
    M = 8 * max(H, 32) + 45
    a = _sweep(pkg, monkeypatch, 5 * M, M, H, 950 + H)
    b = _sweep(pkg, monkeypatch, 5 * M, M, H, 950 + H)
    for k in ("W0", "W1", "P", "Q", "A", "GB", "GD"):
        assert np.array_equal(a[k], b[k]), k
    assert a["GX"] == b["GX"]
