"""lambda_max, and the stop test's d = ||B_old - B||_2 / ||B_old||_2 that is built on it, on Grams with STRUCTURE: a constant diagonal,
exact symmetries, an eigenvector equal to the all-ones vector, a top eigenspace of dimension H / 2.  tests/test_gpu_lambda_max.py builds
every matrix as Q diag(lambda) Q' with a random orthogonal Q, so the Lanczos iteration's deterministic start vector, diag(G) / tr + 1e-3
(lanczos_lambda_max, csrc/ctrl_kernels.hpp), is always in general position there; here it is an exact eigenvector of a NON-dominant
eigenvalue (paired, halves, alternating, circulant, edge), which the iteration before its restart answered with that eigenvalue.  Every
matrix is written down by formula; the reference is numpy.linalg.eigvalsh in fp64 (part 1) and the oracle's own delta after its own
single sweep from the same state (part 2)."""
import copy

import numpy as np
import pytest

import __graft_entry__ as G
from oracle import vbmf_oracle as O
from tests.helpers import report

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


# ---- 1. lambda_max ------------------------------------------------------------------------------------------------------------------------
def _paired(H, c):
    """2 x 2 diagonal blocks [[1 + c, -c], [-c, 1 + c]] (odd H: the last diagonal entry is 1 + c): eigenvalues 1 (the all-ones vector
    among its eigenvectors) and 1 + 2c (H // 2 times)"""
    Gm = (1.0 + c) * np.eye(H)
    for i in range(0, H - 1, 2):
        Gm[i, i + 1] = Gm[i + 1, i] = -c
    return Gm


def _signed(H, c, s):
    return np.eye(H) + c * np.outer(s, s)


def _halves(H, c):
    """I + c s s', s = +1 on the first H // 2 rows, -1 on the rest"""
    return _signed(H, c, np.where(np.arange(H) < H // 2, 1.0, -1.0))


def _alternating(H, c):
    """I + c s s', s = (+, -, +, -, ...)"""
    return _signed(H, c, np.where(np.arange(H) % 2 == 0, 1.0, -1.0))


def _circulant(H):
    """0.5 I + cos(2 pi 3 (i - j) / H): the all-ones vector has eigenvalue 0.5, the top eigenvalue 0.5 + H / 2 is double"""
    i = np.arange(H)
    Gm = 0.5 * np.eye(H) + np.cos(2.0 * np.pi * 3.0 * (i[:, None] - i[None, :]) / H)
    return 0.5 * (Gm + Gm.T)


def _edge(H, c):
    """I + c (e_(H-1) - e_(H-2))(e_(H-1) - e_(H-2))': the dominant eigenvector lives in the last two rows alone and is orthogonal to the
    start vector in exact arithmetic"""
    v = np.zeros(H)
    v[H - 1], v[H - 2] = 1.0, -1.0
    return np.eye(H) + c * np.outer(v, v)


def _permuted(Gm, H):
    """P G P' for one fixed-seed permutation: the diagonal stays constant, the structure moves across the 16-column register chunks
    and the owner lanes"""
    p = np.random.default_rng(20170104 + H).permutation(H)
    return Gm[np.ix_(p, p)]


def _families(H):
    fam = [(f"paired({c})", _paired(H, c)) for c in (0.0025, 0.37, 10)]
    fam += [(f"halves({c})", _halves(H, c)) for c in (0.3, 1)]
    fam += [(f"alternating({c})", _alternating(H, c)) for c in (0.3, 1)]
    fam.append(("circulant", _circulant(H)))
    fam += [("permuted paired(0.37)", _permuted(_paired(H, 0.37), H)), ("permuted halves(1)", _permuted(_halves(H, 1), H)),
            ("permuted alternating(1)", _permuted(_alternating(H, 1), H))]
    fam += [("paired(0.37) x 1e-30", 1e-30 * _paired(H, 0.37)), ("paired(0.37) x 1e+30", 1e+30 * _paired(H, 0.37))]
    fam.append(("edge(0.37)", _edge(H, 0.37)))
    return fam


def _top_gap(ev):
    """(lambda_max - the next DISTINCT eigenvalue) / lambda_max: an exactly degenerate top eigenvalue counts as one"""
    top = ev[-1]
    below = ev[ev < top * (1.0 - 1e-9)]
    return 1.0 if below.size == 0 else float((top - below[-1]) / top)


# tolerances: the project's existing figures (tests/test_gpu_lambda_max.py, test_lambda_max_on_hard_spectra).  Lanczos: 2e-6.  Squaring:
# 2e-6 where the top gap is >= 5 %, 5e-4 for paired(0.0025), whose 0.5 % gap is the edge of the route's documented cluster bound
TOL = 2e-6
TOL_SQUARING_CLUSTER = 5e-4
LANCZOS_H = (65, 66, 128, 129, 130, 200, 255, 256)       # NP = 128 and 256, RB = 4, rows at and above H zeroed
FORCED_H = (2, 16, 17, 64)                                # DEBUG_EXACT_LAMBDA: the iteration at H <= 64 too (NP = 16, 32, 64: RB = 1)
SQUARING_H = (2, 16, 17, 32, 33, 64)


def _check(pkg, H, route):
    capi = pkg.capi
    bad = []
    with capi.Context(600, 300, H, y_dtype=capi.VBMF_Y_F32) as c:
        if route == "forced lanczos":
            c.debug_set(capi.DEBUG_EXACT_LAMBDA, 1)
        for name, Gm in _families(H):
            assert np.array_equal(Gm, Gm.T)
            ev = np.linalg.eigvalsh(Gm)
            assert ev[0] > 0.0
            ref, gap = float(ev[-1]), _top_gap(ev)
            tol = TOL
            if route == "squaring":
                if name == "paired(0.0025)":
                    tol = TOL_SQUARING_CLUSTER
                else:
                    assert gap >= 0.05, (H, name, gap)            # (what the 2e-6 of the squaring route presumes)
            got, us = c.lambda_max(Gm)
            err = abs(got - ref) / ref
            line = f"lambda_max structured H={H} {route} {name}: lam={err:.2e}  [{us:.0f} us]"
            print(line)
            try:
                report(line)
            except AssertionError as e:                           # (the 3 x guard of the measured baseline: every line first)
                bad.append((name, "baseline guard", str(e)))
            if not err <= tol:
                bad.append((name, got, ref, err, tol))
    assert not bad, (H, route, bad)


@pytest.mark.parametrize("H", LANCZOS_H)
def test_lanczos_on_structured_grams(pkg, H):
    _check(pkg, H, "lanczos")


@pytest.mark.parametrize("H", FORCED_H)
def test_forced_lanczos_on_structured_grams(pkg, H):
    _check(pkg, H, "forced lanczos")


@pytest.mark.parametrize("H", SQUARING_H)
def test_squaring_on_structured_grams(pkg, H):
    _check(pkg, H, "squaring")


def test_restart_is_deterministic(pkg):
    """no random state behind the restart: the same bits from call to call and from context to context"""
    capi = pkg.capi
    H = 130
    vals = []
    for _ in range(2):
        with capi.Context(600, 300, H, y_dtype=capi.VBMF_Y_F32) as c:
            vals.append([c.lambda_max(Gm)[0] for name, Gm in _families(H) for rep in range(2)])
    assert vals[0] == vals[1]
    assert all(a == b for a, b in zip(vals[0][0::2], vals[0][1::2]))


# ---- 2. d end to end --------------------------------------------------------------------------------------------------------------------
def _B0(L, H):
    """rows 0 .. H-1: blockdiag([[1.5, -0.5], [-0.5, 1.5]], ...), every other row zero.  Every entry is exact in bf16 and every Gram
    entry a sum of at most two exact products, so B0'B0 = blockdiag([[2.5, -1.5], [-1.5, 2.5]]) on the device in any storage:
    ||B0||_2 = 2, where the all-ones start vector's eigenvalue gives 1"""
    assert H % 2 == 0 and L >= H
    B = np.zeros((L, H))
    for i in range(0, H, 2):
        B[i, i] = B[i + 1, i + 1] = 1.5
        B[i, i + 1] = B[i + 1, i] = -0.5
    assert np.array_equal(B.T @ B, _paired(H, 1.5))
    return B


def _f32(X):
    return X.astype(np.float32).astype(np.float64)


# the bounds on d of the existing comparisons, by storage:
#   streaming, basic model, f32 and bf16x2: 5e-3 d + D_ATOL with D_ATOL = 2e-6 (tests/test_gpu_parity.py:142, test_run_three_sweeps; the
#       one-sweep trace comparison of test_elbo_and_trace, :321, is the same figure)
#   streaming, ARD-sparse run: 2e-2 d + 2e-6 (tests/test_gpu_sparse.py:112, test_sparse_run_and_lower_bound)
#   batched fits (fp64 throughout): trace_d's rule of tests/test_gpu_fit_basic_batch.py:19-22 -- max(3 x measured, 1e-12), capped at 1e-8
D_RTOL_BASIC, D_ATOL = 5e-3, 2e-6
D_RTOL_SPARSE = 2e-2
TOL_TRACE_D = max(3.0 * 4.36e-12, 1e-12)
assert TOL_TRACE_D <= 1e-8


@pytest.mark.parametrize("L,M,H,mode,exact", [(256, 40, 128, "f32", 0), (256, 40, 128, "bf16x2", 0), (320, 40, 256, "f32", 0),
                                              (320, 40, 256, "bf16x2", 0), (256, 40, 16, "f32", 1), (256, 40, 16, "bf16x2", 1)])
def test_d_of_one_streaming_sweep(pkg, L, M, H, mode, exact):
    capi = pkg.capi
    rng = np.random.default_rng(4000 + H + exact)
    Y = _f32(rng.standard_normal((L, M)))
    po = O.vbmf_init(Y, H, ca=0.1, cb=0.1, sigma2=0.1, rng=rng, materialize_yhat=False)
    po.AHat, po.BHat = _f32(po.AHat), _B0(L, H)
    ydt, fdt = (capi.VBMF_Y_F32, capi.VBMF_FACTOR_AUTO) if mode == "f32" else (capi.VBMF_Y_BF16, capi.VBMF_FACTOR_BF16X2)
    with capi.Context(L, M, H, y_dtype=ydt, factor_dtype=fdt) as c:
        c.set_Y(Y)
        Ys = np.ascontiguousarray(c.get_Y())
        c.set_state(po.AHat, po.BHat, po.SigmaA, po.SigmaB, np.diag(po.CA), np.diag(po.CB), po.sigma2)
        if exact:
            c.debug_set(capi.DEBUG_EXACT_LAMBDA, 1)
        it, d, tr = c.run(1, eps=0.0, est_covs=True, est_var=True, want_trace=True)
        gram = c.dims()["gram"]
    _, n, d_ref = O.vbmf_(Ys, po, 1, eps=0.0, est_covs=True, est_var=True)
    err = abs(d - d_ref) / d_ref
    print(f"d structured basic {L}x{M} H{H} {mode} exact={exact}: d={err:.2e}  [gpu {d:.9e} oracle {d_ref:.9e} gram form {gram}]")
    report(f"d structured basic {L}x{M} H{H} {mode} exact={exact}: d={err:.2e}")
    assert it == 1 and n == 1 and tr[0, 0] == d and gram == 0
    assert abs(d - d_ref) <= D_RTOL_BASIC * d_ref + D_ATOL, (d, d_ref, err)


def test_d_of_one_streaming_sparse_sweep(pkg):
    """the ARD-sparse run, diagonal homoscedastic"""
    L, M, H = 256, 40, 128
    rng = np.random.default_rng(4500)
    Y = _f32(rng.standard_normal((L, M)))
    # (the default start values: with ca = cb = sigma = 0.1 the first sweep sends B to ~0, d = ||B0|| / ||B0|| whatever the norm is)
    po = O.vbmf_sparse_init(Y, H, rng=rng, full_cov=False, materialize_yhat=False)
    po.AHat = _f32(po.AHat)
    po.ATVecHat = po.AHat.reshape(M * H).copy()
    po.BHat = _B0(L, H)
    pkg.set_defaults(y_dtype=pkg.VBMF_Y_F32, factor_dtype=pkg.VBMF_FACTOR_AUTO)
    pg = pkg.vbmf_sparse_parameters()                               # (the host's parameter set from the oracle's, labels 1-based)
    for f in ("L", "M", "H", "MH", "H1", "alpha0", "beta0", "alpha", "gamma0", "delta0", "gamma", "sigmaHat", "eta0", "zeta0", "eta",
              "zeta", "trYTY"):
        setattr(pg, f, getattr(po, f))
    pg.labels = np.asarray(po.labels, dtype=np.int64) + 1
    for f in ("AHat", "ATVecHat", "diagSigmaATVec", "SigmaA", "BHat", "SigmaB", "CA", "beta", "CB", "delta"):
        setattr(pg, f, getattr(po, f).copy())
    d = pkg.vbmf_sparse_(Y, pg, 1, eps=0.0, est_cb=True)
    d_ref, n = O.vbmf_sparse_(Y, po, 1, eps=0.0, full_cov=False, est_cb=True)
    err = abs(d - d_ref) / d_ref
    print(f"d structured sparse {L}x{M} H{H} f32: d={err:.2e}  [gpu {d:.9e} oracle {d_ref:.9e}]")
    report(f"d structured sparse {L}x{M} H{H} f32: d={err:.2e}")
    assert pg._last_run[0] == 1 and n == 1
    assert abs(d - d_ref) <= D_RTOL_SPARSE * d_ref + 2e-6, (d, d_ref, err)


BATCH_L, BATCH_MS = 40, (21, 64)


def _batch_ctx(pkg, H, variant=None):
    """two bags side by side in one fp32 context; Y as stored per bag"""
    capi = pkg.capi
    rng = np.random.default_rng(5000 + H)
    Ys = [_f32(rng.standard_normal((BATCH_L, m))) for m in BATCH_MS]
    off = np.concatenate([[0], np.cumsum(BATCH_MS)]).astype(np.int64)
    kw = {} if variant is None else dict(variant=variant)
    ctx = capi.Context(BATCH_L, int(off[-1]), H, y_dtype=capi.VBMF_Y_F32, **kw)
    ctx.set_Y(np.concatenate(Ys, axis=1))
    Yall = ctx.get_Y()
    return ctx, off, [np.ascontiguousarray(Yall[:, a:b]) for a, b in zip(off[:-1], off[1:])]


def _trace_d_check(tag, r, d_refs):
    errs = []
    for f, d_ref in enumerate(d_refs):
        assert r["iters"][f] == 1 and r["status"][f] == 0, (tag, f)
        assert r["d"][f] == r["trace"][f, 0, 0]
        errs.append(abs(r["trace"][f, 0, 0] - d_ref) / d_ref)
    print(f"{tag}: trace_d={max(errs):.2e}  [per fit {errs}]")
    report(f"{tag}: trace_d={max(errs):.2e}")
    assert max(errs) <= TOL_TRACE_D, (tag, errs, r["trace"][:, 0, 0], d_refs)


@pytest.mark.parametrize("form", ["stream", "gram"])
@pytest.mark.parametrize("H", [8, 32])
def test_d_of_one_batched_sweep(pkg, H, form):
    """fp64 squaring (fitb_lambda_max) on a top eigenspace of dimension H / 2, where the squarings never reach a rank-one projector"""
    ctx, off, Ys = _batch_ctx(pkg, H)
    try:
        starts = [O.vbmf_init(Y, H, rng=np.random.default_rng(60 + b), materialize_yhat=False) for b, Y in enumerate(Ys)]
        for p in starts:
            p.BHat = _B0(BATCH_L, H)
        r = ctx.fit_batched(off, [0, 1], 1, 0.0, np.stack([p.BHat for p in starts]), np.stack([p.SigmaB for p in starts]),
                            np.stack([np.diag(p.CA) for p in starts]), np.stack([np.diag(p.CB) for p in starts]),
                            [p.sigma2 for p in starts], est_covs=True, est_var=True, want_trace=True, form=form)
        if form == "gram":
            assert np.all(r["form_used"] == pkg.capi.VBMF_FIT_FORM_GRAM)
    finally:
        ctx.close()
    d_refs = [O.vbmf_(Y, copy.deepcopy(p), 1, eps=0.0, est_covs=True, est_var=True)[2] for Y, p in zip(Ys, starts)]
    _trace_d_check(f"d structured batched basic H{H} {form}", r, d_refs)


@pytest.mark.parametrize("H", [8, 32])
def test_d_of_one_batched_sparse_sweep(pkg, H):
    ctx, off, Ys = _batch_ctx(pkg, H, variant=pkg.capi.VBMF_VARIANT_SPARSE_DIAG)
    try:
        starts = [O.vbmf_sparse_init(Y, H, rng=np.random.default_rng(70 + b), full_cov=False, materialize_yhat=False)
                  for b, Y in enumerate(Ys)]
        for p in starts:
            p.BHat = _B0(BATCH_L, H)
        r = ctx.sparse_fit_batched(
            off, [0, 1], 1, 0.0, [p.gamma for p in starts], [p.delta0 for p in starts], [p.eta for p in starts],
            [p.zeta0 for p in starts], [[p.alpha0, p.beta0, p.alpha0, p.beta0] for p in starts], np.stack([p.BHat for p in starts]),
            np.stack([p.SigmaB for p in starts]), np.stack([p.CB for p in starts]), [p.sigmaHat for p in starts],
            np.concatenate([p.CA for p in starts]), H0=H, full_cov=False, est_cb=True, est_priors=False, want_trace=True)
    finally:
        ctx.close()
    d_refs = [O.vbmf_sparse_(Y, copy.deepcopy(p), 1, eps=0.0, full_cov=False, est_cb=True)[0] for Y, p in zip(Ys, starts)]
    _trace_d_check(f"d structured batched sparse H{H}", r, d_refs)
