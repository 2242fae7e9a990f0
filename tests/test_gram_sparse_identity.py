"""The Gram form of the ARD-sparse sweep ("The ARD-sparse model"), restated in fp64 NumPy and held to the
oracle's vbmf_sparse_ before any kernel is involved.

In the diagonal homoscedastic branch nothing on the B side is masked, so after any sweep B = Y W with W = sigmaHat A SigmaB, where
sigmaHat is the one the B update used (not the one updateSigma! leaves behind it).  Every quantity a sweep takes from Y then comes
from G = Y'Y:  vec(B'Y) = G W (= P),  ||B[:,h]||^2 = diag(W'P),  B'B = W'P,  tr(B'YA) = sum A o P of the new W,  and the stop test's
dB'dB = D'(G D) with D = W_new - W_old.  sigmaHat multiplies ||B[:,h]||^2 in v but not L SigmaB (QS2), and the precision of vec(A')
spreads v by `repeat(v, inner=M-1)` (QS1) or by the consistent tiling.

Sweep counts: the restatement and the oracle are two fp64 evaluations of the same map, and that map amplifies roundings from sweep
to sweep -- to 6e-13 after six sweeps in the consistent layout, 4e-11 in the QS1 layout; after eight QS1 sweeps at H >= 32 to 6e-8,
in the oracle run on a perturbed input as much as in the restatement.  Hence six sweeps in the consistent layout and three in the
reference's; the tolerance 1e-9 leaves room for another BLAS's summation order."""
import copy

import numpy as np
import pytest

from oracle import vbmf_oracle as O

TOL = 1e-9
FIELDS = ("ATVecHat", "diagSigmaATVec", "CA", "beta", "SigmaA", "BHat", "SigmaB", "CB", "delta")


def problem(L, M, H, seed, labels=False, noise=0.05):
    """tests/test_gpu_gram_path.py's `_problem` data (H latent columns of distinct scales) with the sparse model's start state"""
    rng = np.random.default_rng(seed)
    _, A, B = O.toy_matrix(L, M, H, 0.05, rng)
    Y = (B * np.linspace(1.0, 3.0, H)) @ A.T + noise * rng.standard_normal((L, M))
    kw = dict(H1=min(2, H), labels=[0, 5, 17, M - 1]) if labels else {}
    po = O.vbmf_sparse_init(Y, H, ca=0.1, cb=0.1, sigma=0.1, rng=np.random.default_rng(seed + 1), full_cov=False,
                            materialize_yhat=False, **kw)
    return Y, po


def lam_max(S):
    return float(np.linalg.eigvalsh(0.5 * (S + S.T))[-1])


def gram_form_run(Y, p, niter, est_cb=True, compat=True):
    """vbmf_sparse_ in the schedule of sparse_gram_sweep: one ordinary sweep, then sweeps that read G = Y'Y only.  Leaves the fields of
    the last sweep in p (BHat = Y W at the end) and returns the trace [(d, sigmaHat)]."""
    L, M, H = p.L, p.M, p.H
    trace = []
    # the ordinary sweep, W taken where updateB! forms B
    old = p.BHat.copy()
    O.sparse_updateA(Y, p, full_cov=False, reference_compat=compat)
    O.sparse_updateB(Y, p)
    W = p.sigmaHat * (p.AHat @ p.SigmaB)
    O.sparse_updateCA(p)
    if est_cb:
        O.sparse_updateCB(p)
    O.sparse_updateSigma(Y, p)
    trace.append((O.delta(p.BHat, old), p.sigmaHat))
    G = Y.T @ Y
    P = G @ W
    BB = W.T @ P
    for _ in range(1, niter):
        # updateA! (:217-246) from P and diag(B'B)
        v = p.sigmaHat * np.diag(BB) + L * np.diag(p.SigmaB)
        p.diagSigmaATVec = 1.0 / (O.spread_v(v, M, compat) + p.CA)
        p.ATVecHat = p.sigmaHat * p.diagSigmaATVec * P.reshape(M * H)
        p.SigmaA = np.diag(p.diagSigmaATVec.reshape(M, H).sum(axis=0))
        p.AHat = p.ATVecHat.reshape(M, H).copy()
        O._mask(p.AHat, p.labels, p.H1)
        p.ATVecHat = p.AHat.reshape(M * H).copy()
        # updateB! (:263-265) as W, then the product
        p.SigmaB = np.linalg.inv(np.diag(p.CB) + p.sigmaHat * (p.AHat.T @ p.AHat + p.SigmaA))
        Wn = p.sigmaHat * (p.AHat @ p.SigmaB)
        D = Wn - W
        P, Q = G @ Wn, G @ D
        BBold, BB, DD, trBYA = BB, Wn.T @ P, D.T @ Q, float(np.sum(p.AHat * P))
        W = Wn
        O.sparse_updateCA(p)
        if est_cb:                                                    # :295-300
            p.delta = p.delta0 + 0.5 * np.diag(BB) + 0.5 * np.diag(p.SigmaB)
            p.CB = p.gamma / p.delta
        p.zeta = p.zeta0 + 0.5 * p.trYTY - trBYA + 0.5 * O.traceXTY(p.AHat.T @ p.AHat + p.SigmaA, BB + L * p.SigmaB)   # :317-321
        p.sigmaHat = p.eta / p.zeta
        trace.append((np.sqrt(max(lam_max(DD), 0.0) / lam_max(BBold)), p.sigmaHat))                                    # :389
    if niter > 1:
        p.BHat = Y @ W
    return trace


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


@pytest.mark.parametrize("est_cb", [True, False])
@pytest.mark.parametrize("labels", [False, True])
@pytest.mark.parametrize("compat,niter", [(False, 6), (True, 3)])
@pytest.mark.parametrize("L,M,H", [(2464, 352, 8), (2471, 353, 32), (3584, 512, 64)])
def test_gram_form_is_the_oracles_sweep(L, M, H, compat, niter, labels, est_cb):
    Y, po = problem(L, M, H, 500 + H, labels)
    pg = copy.deepcopy(po)
    otr = []
    O.vbmf_sparse_(Y, po, niter, eps=0.0, full_cov=False, est_cb=est_cb, reference_compat=compat, trace=otr)
    gtr = gram_form_run(Y, pg, niter, est_cb=est_cb, compat=compat)
    errs = {f: rel(getattr(pg, f), getattr(po, f)) for f in FIELDS}
    errs["sigmaHat"] = abs(pg.sigmaHat - po.sigmaHat) / po.sigmaHat
    errs["zeta"] = abs(pg.zeta - po.zeta) / po.zeta
    otr, gtr = np.array(otr), np.array(gtr)
    errs["d"] = float(np.max(np.abs(gtr[:, 0] - otr[:, 0]) / otr[:, 0]))
    errs["sigma_trace"] = float(np.max(np.abs(gtr[:, 1] - otr[:, 1]) / otr[:, 1]))
    bad = {k: v for k, v in errs.items() if not v <= TOL}
    assert not bad, (bad, errs)
    if labels:
        assert np.all(pg.AHat[po.labels, H - po.H1:] == 0.0)


def test_sigma_hat_sits_where_the_reference_puts_it():
    """QS2 and W's sigmaHat: moving either breaks the identity by far more than the tolerance."""
    L, M, H = 2464, 352, 8
    Y, po = problem(L, M, H, 508)
    p1 = copy.deepcopy(po)
    O.vbmf_sparse_(Y, po, 3, eps=0.0, full_cov=False, reference_compat=True)
    # W with the sigmaHat updateSigma! leaves instead of the one updateB! used
    O.sparse_updateA(Y, p1, full_cov=False)
    O.sparse_updateB(Y, p1)
    W_right = p1.sigmaHat * (p1.AHat @ p1.SigmaB)
    O.sparse_updateCA(p1); O.sparse_updateCB(p1); O.sparse_updateSigma(Y, p1)
    W_wrong = p1.sigmaHat * (p1.AHat @ p1.SigmaB)
    assert rel(Y @ W_right, p1.BHat) < 1e-12 and rel(Y @ W_wrong, p1.BHat) > 1e-3
    # v with sigmaHat on both terms (what QS2 is not)
    G = Y.T @ Y
    BB = W_right.T @ (G @ W_right)
    assert rel(BB, p1.BHat.T @ p1.BHat) < 1e-12
    v = p1.sigmaHat * np.diag(BB) + L * np.diag(p1.SigmaB)
    v_wrong = p1.sigmaHat * (np.diag(BB) + L * np.diag(p1.SigmaB))
    p2 = copy.deepcopy(p1)
    O.sparse_updateA(Y, p2, full_cov=False)
    d_right = 1.0 / (O.spread_v(v, M, True) + p1.CA)
    d_wrong = 1.0 / (O.spread_v(v_wrong, M, True) + p1.CA)
    assert rel(d_right, p2.diagSigmaATVec) < 1e-12 and rel(d_wrong, p2.diagSigmaATVec) > 1e-3
