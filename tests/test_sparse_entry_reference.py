"""The per-entry references of tests/sparse_entry_reference.py against the oracle (1e-12), and the properties of the synthetic
states that tests/test_gpu_sparse_entries.py relies on.  The oracle is pinned to the reference's recordings
(tests/test_oracle_golden.py), so the GPU test's references are pinned through this file; no GPU is needed here."""
import numpy as np
import pytest

from oracle import vbmf_oracle as O
from tests import sparse_entry_reference as R

TOL = 1e-12
SHAPES = [(9, 2, 3), (40, 33, 5), (23, 31, 12), (30, 17, 1)]          # (L, M, H)


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(np.abs(np.asarray(b)), 1e-300)))


def _oracle_params(L, M, H, st, hyper=R.HYPER, labels=(), H1=0, noise=None):
    p = O.vbmf_sparse_parameters()
    p.L, p.M, p.H, p.MH, p.H1 = L, M, H, M * H, H1
    p.labels = np.asarray(labels, dtype=np.int64)
    for f in ("ATVecHat", "diagSigmaATVec", "CA", "beta", "BHat", "SigmaB", "CB", "delta"):
        setattr(p, f, np.array(st[f], dtype=np.float64))
    p.AHat = p.ATVecHat.reshape(M, H).copy()
    p.SigmaA = np.diag(p.diagSigmaATVec.reshape(M, H).sum(axis=0))
    p.sigmaHat, p.zeta = st["sigmaHat"], st["zeta"]
    for k, v in hyper.items():
        setattr(p, k, v)
    p.alpha, p.gamma, p.eta = hyper["alpha0"] + 0.5, hyper["gamma0"] + 0.5 * L, hyper["eta0"] + 0.5 * L * M
    if noise is not None:
        p.sigmaVecHat, p.zetaVec = noise[0].copy(), noise[1].copy()
        p.etaVec = noise[2] * np.ones(L)
    return p


def _case(L, M, H, seed=5):
    rng = np.random.default_rng(seed)
    Y = rng.standard_normal((L, M))
    st = R.synthetic_state(L, M, H, seed + 1)
    return Y, st


@pytest.mark.parametrize("L,M,H", SHAPES)
@pytest.mark.parametrize("compat", [True, False])
def test_updateA_reference_against_the_oracle(L, M, H, compat):
    Y, st = _case(L, M, H)
    labels, H1 = ([0, M - 1], min(2, H))
    p = _oracle_params(L, M, H, st, labels=labels, H1=H1)
    B = st["BHat"]
    v = R.ref_v(st["sigmaHat"], np.sum(B * B, axis=0), np.diag(st["SigmaB"]), L)
    P = Y.T @ B
    d, a, scale, mask = R.ref_updateA(P, np.abs(P), v, st["CA"], st["sigmaHat"], compat, labels, H1)
    O.sparse_updateA(Y, p, full_cov=False, reference_compat=compat)
    assert _rel(d.reshape(-1), p.diagSigmaATVec) < TOL
    assert _rel(a.reshape(-1), p.ATVecHat) < TOL
    assert np.all(a[mask] == 0.0) and mask.sum() == 2 * H1 and np.all(p.ATVecHat.reshape(M, H)[mask] == 0.0)
    assert np.all(scale >= np.abs(a))
    assert _rel(np.diag(d.sum(axis=0)), p.SigmaA + np.diag(np.full(H, 1e-300))) < TOL
    if H > 1 and M > 2:
        assert np.any(R.v_index(M, H, True) != R.v_index(M, H, False))
    assert np.array_equal(np.arange(float(H))[R.v_index(M, H, compat)].reshape(-1), O.spread_v(np.arange(float(H)), M, compat))


@pytest.mark.parametrize("L,M,H", SHAPES)
@pytest.mark.parametrize("compat", [True, False])
def test_updateA_rows_reference_against_the_oracle(L, M, H, compat):
    Y, st = _case(L, M, H, seed=8)
    noise = R.synthetic_noise_rows(L, M, 3)
    p = _oracle_params(L, M, H, st, noise=noise)
    sig, B = noise[0], st["BHat"]
    v = R.ref_v_rows(sig, B, float(np.mean(sig)), np.diag(st["SigmaB"]), L)
    P = Y.T @ (sig[:, None] * B)
    d, a, _, _ = R.ref_updateA(P, np.abs(P), v, st["CA"], 1.0, compat)
    O.sparse_updateA(Y, p, full_cov=False, reference_compat=compat, diag_var=True)
    assert _rel(d.reshape(-1), p.diagSigmaATVec) < TOL
    assert _rel(a.reshape(-1), p.ATVecHat) < TOL


@pytest.mark.parametrize("L,M,H", SHAPES)
def test_updateCA_updateCB_references_against_the_oracle(L, M, H):
    _, st = _case(L, M, H, seed=11)
    p = _oracle_params(L, M, H, st)
    A, dS, B = st["ATVecHat"].reshape(M, H), st["diagSigmaATVec"].reshape(M, H), st["BHat"]
    b, ca = R.ref_updateCA(A, dS, p.alpha, p.beta0)
    delta, CB = R.ref_updateCB(np.sum(B * B, axis=0), np.diag(st["SigmaB"]), p.gamma, p.delta0)
    O.sparse_updateCA(p)
    O.sparse_updateCB(p)
    assert _rel(b.reshape(-1), p.beta) < TOL and _rel(ca.reshape(-1), p.CA) < TOL
    assert _rel(delta, p.delta) < TOL and _rel(CB, p.CB) < TOL
    # grouped priors: each entry takes its own group's pair; one group everywhere gives the plain update back
    g = R.ca_group(M, H, min(3, H), M // 2)
    assert set(np.unique(g)) <= {0, 1, 2} and np.all(g[:, :min(3, H)] == 0)
    if H > 3:
        assert np.all(g[:M // 2, 3:] == 1) and np.all(g[M // 2:, 3:] == 2)
    al, b0 = np.array([0.6, 1.2, 1.8])[g], np.array([1e-10, 0.02, 0.5])[g]
    bg, cag = R.ref_updateCA(A, dS, al, b0)
    for k in range(3):
        bk, cak = R.ref_updateCA(A, dS, (0.6, 1.2, 1.8)[k], (1e-10, 0.02, 0.5)[k])
        assert np.array_equal(bg[g == k], bk[g == k]) and np.array_equal(cag[g == k], cak[g == k])


@pytest.mark.parametrize("L,M,H", SHAPES)
def test_updateSigma_references_against_the_oracle(L, M, H):
    Y, st = _case(L, M, H, seed=14)
    A, B, SB = st["ATVecHat"].reshape(M, H), st["BHat"], st["SigmaB"]
    SA = np.diag(st["diagSigmaATVec"].reshape(M, H).sum(axis=0))
    GA, GB, Q = A.T @ A, B.T @ B, Y @ A
    p = _oracle_params(L, M, H, st)
    p.trYTY = float(np.sum(Y * Y))
    zeta, mag = R.ref_zeta(p.zeta0, p.trYTY, float(np.sum(Q * B)), GA, SA, GB, SB, L)
    O.sparse_updateSigma(Y, p)
    assert abs(zeta - p.zeta) <= TOL * mag and zeta > 0.0 and mag >= zeta
    assert abs(p.eta / zeta - p.sigmaHat) <= TOL * p.sigmaHat
    noise = R.synthetic_noise_rows(L, M, 4)
    p = _oracle_params(L, M, H, st, noise=noise)
    zl, magl, aquad = R.ref_zeta_rows(p.zeta0, Y, Q, B, GA + SA, SB)
    O.sparse_updateSigma(Y, p, diag_var=True)
    assert np.all(np.abs(zl - p.zetaVec) <= TOL * magl) and np.all(zl > 0.0) and np.all(magl >= zl) and np.all(aquad >= 0.0)
    assert _rel(noise[2] / zl, p.sigmaVecHat) < TOL


@pytest.mark.parametrize("L,M,H", SHAPES)
def test_updateB_matrix_against_the_oracle(L, M, H):
    Y, st = _case(L, M, H, seed=17)
    p = _oracle_params(L, M, H, st)
    A = st["ATVecHat"].reshape(M, H)
    K = R.ref_K(st["CB"], st["sigmaHat"], A.T @ A, p.SigmaA)
    O.sparse_updateB(Y, p)
    assert np.allclose(np.linalg.inv(K), p.SigmaB, rtol=1e-10, atol=0.0)
    assert np.all(np.linalg.eigvalsh(K) > 0.0)


# the shapes of tests/test_gpu_sparse_entries.py (L = 257 throughout) at which the decades are claimed
@pytest.mark.parametrize("M,H", [(97, 33), (33, 129), (2, 31), (31, 31), (1057, 33), (97, 256)])
def test_synthetic_states_meet_what_the_gpu_test_assumes(M, H):
    L = 257
    Y = np.random.default_rng(M + H).standard_normal((L, M))
    st = R.synthetic_state(L, M, H, 9000 + H)
    A, B, SB, CA = st["ATVecHat"].reshape(M, H), st["BHat"], st["SigmaB"], st["CA"]
    dS = st["diagSigmaATVec"].reshape(M, H)
    decades = lambda x: float(np.log10(np.max(np.abs(x)) / np.min(np.abs(x))))
    assert decades(A) >= 4.0 and decades(B) >= 4.0
    if M * H >= 1000:
        assert decades(CA) >= 4.0
    assert np.all(CA > 0) and np.all(st["beta"] > 0) and np.all(st["CB"] > 0) and np.all(dS > 0)
    assert np.all(np.linalg.eigvalsh(SB) > 0.0)
    SA, GA, GB, Q = np.diag(dS.sum(axis=0)), A.T @ A, B.T @ B, Y @ A
    assert np.all(np.linalg.eigvalsh(R.ref_K(st["CB"], st["sigmaHat"], GA, SA)) > 0.0)          # K is SPD
    zeta, _ = R.ref_zeta(R.HYPER["zeta0"], float(np.sum(Y * Y)), float(np.sum(Q * B)), GA, SA, GB, SB, L)
    zl, _, _ = R.ref_zeta_rows(R.HYPER["zeta0"], Y, Q, B, GA + SA, SB)
    assert zeta > 0.0 and np.all(zl > 0.0)
    # the A update's result spans the decades too (what the per-entry bound is for)
    v = R.ref_v(st["sigmaHat"], np.diag(GB), np.diag(SB), L)
    P = Y.T @ B
    d, a, _, _ = R.ref_updateA(P, np.abs(P), v, CA, st["sigmaHat"], True)
    assert np.all(d > 0.0) and decades(a) >= 4.0
