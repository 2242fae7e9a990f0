"""Least-squares classifiers over many bags (vbmf_bag_least_squares; ols_batch, rls_batch, ls_residual_batch, classify_bags): the
reference's ols / rls per bag (examples/mil_util.jl:159-171) and classify's "ols", "rls" and "min_err" branches (:457-501), against
fp64 NumPy on the operands as the device holds them, against the oracle's factorize_bag per bag, and the C ABI's refusals.

The bags sit side by side in one context: L = 166 rows (no multiple of 32), the 40 ragged widths of the batched vbls! tests (1-column
bags, bags straddling the 32-column tiles, up to 70 columns), drawn from two Gaussian bases scaled by linspace(1, 2.5, H) with one-hot
A and noise 0.05, alternating, rounded to fp32.  The bases themselves stay fp64: the entry must not round them.

Bounds.  Estimate and residual are two fp64 evaluations of the same expression on the same operands; they differ by about
cond(B'B + lam I) 2^-53, under 1e-13 at the asserted cond <= 1e3, and are held to RESID_TOL = 1e-10, the project's bound for fp64 on
stored operands.  The regularised rank-deficient basis of the C ABI test has cond = ||b||^2 / lam ~ 1e5 by construction; its estimate
is held to L cond 2^-53 (L-term dot products on either side of an explicit inverse).  "min_err" compares fitted residuals: each moves
with the batched full_cov vbls!'s AHat (5e-6 of the oracle's, tests/test_gpu_vbls_sparse_batch.py) by at most ||B||_2 5e-6 ||A||_F / r.

Measured on an MI355X, worst over each test's parametrisation (none of these figures sets a bound):
  X against NumPy                      3.8e-15        norms against NumPy   2.1e-14 (lam = 5, H = 64)
  classify_bags "ols" / "rls" errs     1.5e-15        label margin          0.94
  zero-column basis at lam = 1e-2      X 3.2e-16, norms 2.0e-16, cond 1.07e5
  "min_err" errs against the oracle    2.1e-7 under a bound of 3.7e-5; ratio gap around the threshold 0.093
"""
import copy
import dataclasses
import functools

import numpy as np
import pytest

import __graft_entry__ as G
from oracle import vbmf_oracle as O
from tests.helpers import relF, report
from tests.test_gpu_vbls_sparse_batch import RAGGED, SMALL

pytestmark = pytest.mark.gpu

L = 166
HS = (1, 2, 5, 20, 64)
LAMS = (0.0, 1e-2, 5.0)
RESID_TOL = 1e-10
# the batched full_cov vbls! holds ATVecHat to this much of the oracle's (tests/test_gpu_vbls_sparse_batch.py, TOL[True])
FULL_COV_A_TOL = 5e-6


@pytest.fixture(scope="module")
def pkg():
    G.build()
    p = G.load_package()
    p.set_defaults(y_dtype=p.VBMF_Y_F32, factor_dtype=p.VBMF_FACTOR_AUTO)
    yield p
    p.invalidate()
    p.set_defaults(y_dtype=p.VBMF_Y_F32, factor_dtype=p.VBMF_FACTOR_AUTO)


def _f32(Y):
    return Y.astype(np.float32).astype(np.float64)


def _convert(cls, src):
    dst = cls()
    for f in dataclasses.fields(cls):
        if hasattr(src, f.name):
            setattr(dst, f.name, copy.deepcopy(getattr(src, f.name)))
    return dst


def _two_bases(H, seed, rows=L):
    rng = np.random.default_rng(seed)
    Bs = [rng.standard_normal((rows, H)) * np.linspace(1.0, 2.5, H) for _ in range(2)]

    def draw(k, m):
        As = np.zeros((m, H)); As[np.arange(m), rng.integers(0, H, m)] = 1.0
        return Bs[k] @ As.T + 0.05 * rng.standard_normal((rows, m))
    return Bs, draw


def _ls(B, lam, Ys):
    """the reference's expressions in fp64: inv(B'B + lam I) * B' * Y and norm(Y - B X), with the condition number of the inverse"""
    Gm = B.T @ B + lam * np.eye(B.shape[1])
    K = np.linalg.inv(Gm)
    Xs = [K @ B.T @ Y for Y in Ys]
    return Xs, np.array([np.linalg.norm(Y - B @ X) for Y, X in zip(Ys, Xs)]), float(np.linalg.cond(Gm))


@functools.lru_cache(maxsize=None)
def _case(H):
    """the two bases and the 40 alternating ragged bags for rank H; computed once and left unchanged"""
    Bs, draw = _two_bases(H, 6100 + H)
    return Bs, [_f32(draw(b % 2, m)) for b, m in enumerate(RAGGED)]


def _split(Yall, Ms):
    off = np.concatenate([[0], np.cumsum(Ms)])
    return [Yall[:, c0:c1] for c0, c1 in zip(off[:-1], off[1:])]


def _storage(pkg, storage):
    pkg.set_defaults(y_dtype=pkg.VBMF_Y_BF16 if storage == "bf16" else pkg.VBMF_Y_F32, factor_dtype=pkg.VBMF_FACTOR_AUTO)


def _check_estimate_and_residual(pkg, tag, B, lam, Ys, storage):
    H = B.shape[1]
    try:
        _storage(pkg, storage)
        bags = pkg.Bags(Ys, H)                                          # no state is ever set on this context
        Xg = pkg.ols_batch(bags, B) if lam == 0.0 else pkg.rls_batch(bags, B, lam)
        rg = pkg.ls_residual_batch(bags, B, lam)
        Ysts = _split(bags.session.ctx.get_Y(), [Y.shape[1] for Y in Ys])
        bags.close()
    finally:
        _storage(pkg, "f32")
    if storage == "f32":
        assert all(np.array_equal(a, b) for a, b in zip(Ysts, Ys))
    Xw, rw, cond = _ls(B, lam, Ysts)
    ratio = max(float(np.sum(Y * Y)) / r ** 2 for Y, r in zip(Ysts, rw))
    er = float(np.max(np.abs(rg - rw) / rw))
    ex = max(relF(a, b) for a, b in zip(Xg, Xw))
    report(f"ls_batch {tag} {storage} H{H} lam{lam:g} {len(Ys)} bags: r={er:.2e} X={ex:.2e} cond={cond:.1f} max_YY_over_r2={ratio:.0f}")
    assert all(a.shape == (H, Y.shape[1]) for a, Y in zip(Xg, Ys)) and rg.shape == (len(Ys),)
    assert cond <= 1e3 and ratio > 100, (cond, ratio)                 # well conditioned, and the regime the direct residual is for
    assert er <= RESID_TOL, er
    assert ex <= RESID_TOL, ex


# ---- 1. estimate and residual against fp64 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("H,storage", [(H, "f32") for H in HS] + [(5, "bf16"), (64, "bf16")])
def test_estimate_and_residual_against_fp64(pkg, H, storage, lam):
    Bs, Ys = _case(H)
    _check_estimate_and_residual(pkg, "ragged", Bs[0], lam, Ys, storage)


def test_estimate_and_residual_small(pkg):
    Bs, draw = _two_bases(5, 6133, rows=33)
    Ys = [_f32(draw(0, m)) for m in (1, 2, 9)]
    for lam in (0.0, 1e-2):
        _check_estimate_and_residual(pkg, "L33", Bs[0], lam, Ys, "f32")


# ---- 2. position independence ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [5, 64])                                  # a slice's outputs within / beyond one per thread
def test_permuting_the_bags_permutes_the_outputs_bitwise(pkg, H):
    Bs, Ys = _case(H)
    B, lam = Bs[1], 1e-2

    def run(idx):
        bags = pkg.Bags([Ys[i] for i in idx], H)
        out = pkg.rls_batch(bags, B, lam), pkg.ls_residual_batch(bags, B, lam)
        bags.close()
        return out
    n = len(Ys)
    X0, r0 = run(list(range(n)))
    perm = [int(i) for i in np.random.default_rng(22).permutation(n)]
    X1, r1 = run(perm)
    assert np.array_equal(r0[perm], r1)
    assert all(np.array_equal(X0[i], x) for i, x in zip(perm, X1))
    for i in (0, 3, 9, n - 1):                                          # 1-column, 70-column, 64-column, last
        Xa, ra = run([i])
        assert ra[0] == r0[i] and np.array_equal(Xa[0], X0[i]), i


# ---- 3. classify_bags "ols" / "rls" ------------------------------------------------------------------------------------------
def _model_with(pkg, kind, B):
    Ytr = np.zeros((B.shape[0], 3))
    p = (pkg.vbmf_init if kind == "basic" else pkg.vbmf_sparse_init)(Ytr, B.shape[1], rng=np.random.default_rng(0))
    p.BHat = B.copy()
    return p


def _check_ls_classifier(pkg, tag, alg, res, Bs, Ys, Yarg):
    lam = {"ols": 0.0, "rls": 1e-2}[alg]
    errs = [_ls(B, lam, Ys)[1] for B in Bs]
    want = (errs[0] > errs[1]).astype(np.int64)
    margin = float(np.min(np.abs(errs[0] - errs[1]) / np.maximum(errs[0], errs[1])))
    labels, e0, e1 = pkg.classify_bags(res[0], res[1], Yarg, alg)
    d = max(float(np.max(np.abs(e0 - errs[0]) / errs[0])), float(np.max(np.abs(e1 - errs[1]) / errs[1])))
    report(f"classify_bags {alg} {tag} {len(Ys)} bags: err={d:.2e} margin={margin:.2e} ones={int(want.sum())}")
    assert margin >= 100 * RESID_TOL, margin
    assert 0 < want.sum() < len(Ys)
    assert np.array_equal(labels, want)
    assert d <= RESID_TOL, d


@pytest.mark.parametrize("H", [5, 20])
def test_classify_ols_rls(pkg, H):
    Bs, Ys = _case(H)
    res = [_model_with(pkg, "basic", B) for B in Bs]
    _check_ls_classifier(pkg, f"H{H}", "ols", res, Bs, Ys, Ys)
    _check_ls_classifier(pkg, f"H{H}", "rls", res, Bs, Ys, Ys)
    bags = pkg.SparseBags(Ys, H)                                        # an upload made for something else serves too
    _check_ls_classifier(pkg, f"H{H} uploaded", "rls", res, Bs, Ys, bags)
    bags.close()
    # the default class_alg is the reference's
    assert np.array_equal(pkg.classify_bags(res[0], res[1], Ys)[1], pkg.classify_bags(res[0], res[1], Ys, "ols")[1])


def test_classify_two_ranks_two_model_types(pkg):
    (B5, _), d5 = _two_bases(5, 6105)
    (_, B20), d20 = _two_bases(20, 6120)
    Ys = [_f32(d5(0, m) if b % 2 == 0 else d20(1, m)) for b, m in enumerate(RAGGED)]
    res = [_model_with(pkg, "basic", B5), _model_with(pkg, "sparse", B20)]
    for alg in ("ols", "rls"):
        _check_ls_classifier(pkg, "H5 basic / H20 sparse", alg, res, [B5, B20], Ys, Ys)


# ---- 4. classify_bags "min_err" ----------------------------------------------------------------------------------------------
def _oracle_vbls(Y, q, niter):
    for _ in range(niter):
        O.sparse_updateA(Y, q, full_cov=True)
        O.sparse_updateCA(q)
        O.sparse_updateSigma(Y, q)


def _moved_by(B, A, r, tolA):
    """|r(A + dA) - r(A)| <= ||B dA'||_F <= ||B||_2 ||dA||_F with ||dA||_F <= tolA ||A||_F, relative to r"""
    return float(np.linalg.norm(B, 2) * tolA * np.linalg.norm(A) / r)


def test_classify_min_err(pkg):
    """factorize_bag per bag by the oracle (examples/mil_util.jl:393-416) and the two norm(Y - YHat) against classify_bags.  Model and
    bags of the lower_bound classifier's test: bags of even index use the first H - H1 columns of the trained basis only (both fits
    explain them: label 0), the others its last H1 (only the whole basis does: label 1)."""
    H, H1, niter, thr = 5, 2, 8, 1e-1
    _, draw = _two_bases(H, 5400)
    Ytr = draw(0, 200)
    po = O.vbmf_sparse_init(Ytr, H, rng=np.random.default_rng(5410), full_cov=False, materialize_yhat=False)
    O.vbmf_sparse_(Ytr, po, 12, eps=0.0)
    po.H1 = H1
    H0 = H - H1
    rng = np.random.default_rng(5420)
    Ys = []
    for b, m in enumerate(SMALL * 2):                                  # full_cov: the oracle inverts M_b H x M_b H
        As = np.zeros((m, H)); As[np.arange(m), rng.integers(0, H0, m) if b % 2 == 0 else rng.integers(H0, H, m)] = 1.0
        Ys.append(_f32(po.BHat @ As.T + 0.05 * rng.standard_normal((L, m))))
    res = _convert(pkg.vbmf_sparse_parameters, po)
    errs, moved = [[], []], 0.0
    for b, Y in enumerate(Ys):
        p0 = O.vbmf_sparse_init(Y, H0, rng=np.random.default_rng(b), full_cov=False, materialize_yhat=False)
        p0.BHat, p0.SigmaB, p0.CB = po.BHat[:, :H0].copy(), po.SigmaB[:H0, :H0].copy(), po.CB[:H0].copy()
        p0.gamma, p0.delta = po.gamma, po.delta[:H0].copy()
        assert Y.shape[1] * H0 < 1600
        _oracle_vbls(Y, p0, niter)
        res1 = copy.copy(po); res1.H1 = 0
        p1 = O.copy_vbmf_params(Y, res1, rng=np.random.default_rng(b))
        _oracle_vbls(Y, p1, niter)
        for k, q in enumerate((p0, p1)):
            r = np.linalg.norm(Y - q.BHat @ q.AHat.T)                  # = norm(Y - params.YHat), :435-436
            errs[k].append(r)
            moved = max(moved, _moved_by(q.BHat, q.AHat, r, FULL_COV_A_TOL))
    errs = [np.array(e) for e in errs]
    ratio = np.abs((errs[0] - errs[1]) / errs[0])
    want = np.where(ratio < thr, 0, 1)
    gap = float(np.min(np.abs(ratio - thr)))
    # err0 and err1 each move by at most `moved` of themselves, the ratio |1 - err1/err0| by at most about 2 moved
    assert gap > 2 * moved, (gap, moved)
    labels, e0, e1 = pkg.classify_bags(res, None, Ys, "min_err", threshold=thr, niter=niter)
    d = max(float(np.max(np.abs(e0 - errs[0]) / errs[0])), float(np.max(np.abs(e1 - errs[1]) / errs[1])))
    report(f"classify_bags min_err H{H} H1={H1} {len(Ys)} bags: err={d:.2e} bound={moved:.2e} gap={gap:.2e} ones={int(want.sum())}")
    assert 0 < want.sum() < len(Ys)
    assert np.array_equal(labels, want)
    assert d <= moved, (d, moved)


# ---- 5. the other three classifiers are classify_batch's ---------------------------------------------------------------------
def test_delegation_is_bitwise(pkg):
    H = 5
    Bs, draw = _two_bases(H, 6205)
    Ys = [_f32(draw(b % 2, m)) for b, m in enumerate(SMALL)]
    res = [_model_with(pkg, "basic", B) for B in Bs]
    a = pkg.classify_bags(res[0], res[1], Ys, "vbls", niter=5)
    b = pkg.classify_batch(res[0], res[1], Ys, "vbls", niter=5)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 6. C ABI refusals and the error return ----------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_rank_deficiency(pkg):
    C = pkg.capi
    VI, VU, VN = C.VBMF_ERR_INVALID, C.VBMF_ERR_UNSUPPORTED, C.VBMF_ERR_NUMERIC
    M, H = 40, 4
    Bs, draw = _two_bases(H, 6304)
    B = Bs[0]
    Y = _f32(draw(0, M))
    off = np.array([0, 1, 17, 33, M], dtype=np.int64)
    nb = off.size - 1
    Ysplit = _split(Y, np.diff(off))
    ip, dp = C.C.POINTER(C.C.c_int64), C.C.POINTER(C.C.c_double)
    Bf = np.asfortranarray(B)
    Xbuf, rbuf = np.empty((H, M), order="F"), np.empty(nb)

    def raw(c, o=off, Bp=Bf, ldB=L, h=H, lam=0.0, X=Xbuf, ldX=H, r=rbuf):
        return C.lib().vbmf_bag_least_squares(c._h, len(o) - 1, o.ctypes.data_as(ip), None if Bp is None else Bp.ctypes.data_as(dp), ldB,
                                              h, lam, None if X is None else X.ctypes.data_as(dp), ldX,
                                              None if r is None else r.ctypes.data_as(dp))

    with C.Context(L, M, 7, y_dtype=pkg.VBMF_Y_F32) as c:               # the context's own H is not the call's
        c.set_Y(Y)
        rng = np.random.default_rng(5)
        c.set_state(rng.standard_normal((M, 7)), rng.standard_normal((L, 7)), np.eye(7), np.eye(7), np.ones(7), np.ones(7), 0.3)
        before = c.get_state()
        X0, r0 = c.bag_least_squares(off, B, 1e-2)
        Xw, rw, _ = _ls(B, 1e-2, Ysplit)
        assert relF(X0, np.hstack(Xw)) <= RESID_TOL and float(np.max(np.abs(np.sqrt(r0) - rw) / rw)) <= RESID_TOL
        # one output at a time gives the same bits
        assert np.array_equal(c.bag_least_squares(off, B, 1e-2, want_r2=False)[0], X0)
        assert np.array_equal(c.bag_least_squares(off, B, 1e-2, want_X=False)[1], r0)
        assert raw(c, h=0) == VU and raw(c, h=65, Bp=np.zeros((L, 65), order="F")) == VU
        for lam in (-1e-3, float("nan"), float("inf")):
            assert raw(c, lam=lam) == VI, lam
        for v in (np.nan, np.inf):
            Bn = Bf.copy(order="F"); Bn[L - 1, H - 1] = v
            assert raw(c, Bp=Bn) == VI
            assert "BHat" in c._lib.vbmf_last_error(c._h).decode()
        assert raw(c, ldB=L - 1) == VI and raw(c, ldX=H - 1) == VI
        assert raw(c, Bp=None) == VI and raw(c, X=None, r=None) == VI
        for bad in ([0, 1, 1, M], [1, 17, M], [0, 17, M - 1], [0, 20, 10, M], [0, M + 1]):
            assert raw(c, o=np.array(bad, dtype=np.int64)) == VI, bad
        # a basis with an all-zero column: not positive definite at lam = 0, the case rls exists for (examples/mil_util.jl:463-464)
        Bz = Bf.copy(order="F"); Bz[:, 2] = 0.0
        Xbuf[:] = -7.0; rbuf[:] = -7.0
        assert raw(c, Bp=Bz) == VN
        assert "positive definite" in c._lib.vbmf_last_error(c._h).decode()
        assert np.all(Xbuf == -7.0) and np.all(rbuf == -7.0)          # nothing written
        Xz, rz = c.bag_least_squares(off, Bz, 1e-2)
        Xzw, rzw, cond = _ls(Bz, 1e-2, Ysplit)
        ex, er = relF(Xz, np.hstack(Xzw)), float(np.max(np.abs(np.sqrt(rz) - rzw) / rzw))
        report(f"ls_batch zero column H{H} lam0.01: r={er:.2e} X={ex:.2e} cond={cond:.3g}")
        assert 1e4 < cond < 1e6 and np.all(Xz[2] == 0.0)
        assert ex <= L * cond * 2.0 ** -53 and er <= RESID_TOL, (ex, er)
        # after all that a valid call returns the same bits as before, and the state was never touched
        X1, r1 = c.bag_least_squares(off, B, 1e-2)
        assert np.array_equal(X1, X0) and np.array_equal(r1, r0)
        after = c.get_state()
        for k, v in before.items():
            assert np.array_equal(np.asarray(v), np.asarray(after[k])), k
    for v in (C.VBMF_VARIANT_SPARSE_DIAGVAR, C.VBMF_VARIANT_DUAL_DIAGVAR, C.VBMF_VARIANT_TRIAL_DIAGVAR):
        with C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32, variant=v) as c:
            assert raw(c) == VI and "diag_var" in c._lib.vbmf_last_error(c._h).decode()
    with C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32, nranks=2, rank=0, L_global=2 * L, variant=C.VBMF_VARIANT_SPARSE_DIAG) as c:
        assert raw(c) == VI and "rank" in c._lib.vbmf_last_error(c._h).decode()
