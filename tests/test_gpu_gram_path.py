"""GPU tests of the Gram-form sweep of vbmf_run: with B = Y W, W = A SigmaB / sigma2, a sweep reads the
M x M Gram matrix G = Y'Y instead of streaming Y twice.  VBMF_GRAM=1 forces the form at small shapes (read when a context is
created); VBMF_GRAM=0 forces the streaming path.  Tolerances are test_gpu_parity.py's bf16x2 ones (1e-4 per field, 1e-3 on sigma2)."""
import numpy as np
import pytest

import __graft_entry__ as G
from oracle import vbmf_oracle as O
from tests.helpers import relF

pytestmark = pytest.mark.gpu

TOL = dict(default=1e-4, sigma2=1e-3)
FIELDS = ("AHat", "BHat", "SigmaA", "SigmaB", "CA_diag", "CB_diag")


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


def _problem(L, M, H, seed, labels=False):
    """Well-conditioned data (test_gpu_parity.py's `separated` form: H latent columns of distinct scales): on rank-deficient
    toy data the factors drift by rotations that rounding noise amplifies ~2x per sweep, and six sweeps of the streaming path
    already leave the oracle by 1e-2, so a six-sweep comparison there measures that drift, not the Gram form."""
    rng = np.random.default_rng(seed)
    _, A, B = O.toy_matrix(L, M, H, 0.05, rng)
    Y = (B * np.linspace(1.0, 3.0, H)) @ A.T + 0.05 * rng.standard_normal((L, M))
    kw = dict(H1=min(2, H), labels=[0, 5, 17, M - 1]) if labels else {}
    po = O.vbmf_init(Y, H, ca=0.1, cb=0.1, sigma2=0.1, rng=np.random.default_rng(seed + 1), materialize_yhat=False, **kw)
    return Y, po


def _ctx(pkg, monkeypatch, L, M, H, gram):
    monkeypatch.setenv("VBMF_GRAM", "1" if gram else "0")
    c = pkg.capi.Context(L, M, H, y_dtype=pkg.VBMF_Y_BF16, factor_dtype=pkg.VBMF_FACTOR_BF16X2)
    monkeypatch.delenv("VBMF_GRAM")
    return c


def _set(c, po):
    c.set_state(po.AHat, po.BHat, po.SigmaA, po.SigmaB, np.diag(po.CA), np.diag(po.CB), po.sigma2,
                labels0=po.labels, H1=po.H1)


def _run(pkg, monkeypatch, Y, po, n, gram, eps=0.0):
    L, M = Y.shape
    with _ctx(pkg, monkeypatch, L, M, po.H, gram) as c:
        c.set_Y(Y)
        _set(c, po)
        it, d, tr = c.run(n, eps=eps, est_covs=True, est_var=True, want_trace=True)
        return dict(dims=c.dims(), it=it, d=d, trace=tr.copy(), state=c.get_state(), Ys=c.get_Y())


def _errs(s, ref):
    e = {k: relF(s[k], ref[k]) for k in FIELDS}
    e["sigma2"] = abs(s["sigma2"] - ref["sigma2"]) / abs(ref["sigma2"])
    return e


def _check(tag, e, tol):
    bad = {k: v for k, v in e.items() if not v <= tol.get(k, tol["default"])}
    assert not bad, (tag, bad, e)


@pytest.mark.parametrize("labels", [False, True])
@pytest.mark.parametrize("H", [8, 32, 64, 128])
def test_parity_with_oracle_and_streaming(pkg, monkeypatch, H, labels):
    """Six sweeps in the Gram form against the fp64 oracle on the stored Y, and against the same run on the streaming path."""
    M = max(352, 8 * H)
    L = 7 * M
    Y, po = _problem(L, M, H, 500 + H, labels)
    g = _run(pkg, monkeypatch, Y, po, 6, True)
    s = _run(pkg, monkeypatch, Y, po, 6, False)
    assert g["dims"]["gram"] == 1 and g["dims"]["gram_built"] == 1 and s["dims"]["gram"] == 0
    assert g["it"] == s["it"] == 6
    O.vbmf_(g["Ys"], po, 6, eps=0.0, est_covs=True, est_var=True)
    ref = dict(AHat=po.AHat, BHat=po.BHat, SigmaA=po.SigmaA, SigmaB=po.SigmaB, CA_diag=np.diag(po.CA), CB_diag=np.diag(po.CB),
               sigma2=po.sigma2)
    tol6 = {k: (v if k == "sigma2" else 2 * v) for k, v in TOL.items()}
    # no worse than the streaming path where that path itself drifts from the oracle beyond the tolerance (H = 64 here: SigmaB
    # 4.4e-4 streaming, 4.3e-4 Gram form after six sweeps)
    es = _errs(s["state"], ref)
    bound = {k: max(tol6.get(k, tol6["default"]), 1.5 * v) for k, v in es.items()}
    bound["default"] = tol6["default"]
    _check(f"gram vs oracle H{H} labels={labels}", _errs(g["state"], ref), bound)
    if all(v <= tol6.get(k, tol6["default"]) for k, v in es.items()):
        _check(f"gram vs streaming H{H} labels={labels}", _errs(g["state"], s["state"]), tol6)
    if labels:
        A = g["state"]["AHat"]
        assert np.all(A[po.labels, H - po.H1:] == 0.0)
    # the per-sweep trace: d, sigma2, ELBO
    tg, ts = g["trace"], s["trace"]
    assert np.all(np.abs(tg[:, 1] - ts[:, 1]) <= 1e-3 * np.abs(ts[:, 1])), (tg[:, 1], ts[:, 1])
    assert np.all(np.abs(tg[:, 2] - ts[:, 2]) <= 1e-4 * np.abs(ts[:, 2])), (tg[:, 2], ts[:, 2])
    assert np.all(np.abs(tg[:, 0] - ts[:, 0]) <= 5e-3 * np.abs(ts[:, 0]) + 1e-5), (tg[:, 0], ts[:, 0])


@pytest.mark.parametrize("H", [16, 64])
def test_split_runs_continue_the_gram_form(pkg, monkeypatch, H):
    """run(3) + run(3) computes what run(6) computes: W and P = G W carry over, B is materialised at the end of each run."""
    L, M = 2000, 300
    Y, po = _problem(L, M, H, 610 + H)
    one = _run(pkg, monkeypatch, Y, po, 6, True)
    with _ctx(pkg, monkeypatch, L, M, H, True) as c:
        c.set_Y(Y)
        _set(c, po)
        c.run(3, eps=0.0, est_covs=True, est_var=True)
        mid = c.get_state()
        it, d, tr = c.run(3, eps=0.0, est_covs=True, est_var=True, want_trace=True)
        two = c.get_state()
    assert it == 3
    _check("run3+run3 vs run6", _errs(two, one["state"]), dict(default=1e-6, sigma2=1e-6))
    assert np.allclose(tr, one["trace"][3:], rtol=1e-6, atol=1e-9)
    # the B the first run left is the B of its third sweep (materialised eagerly)
    three = _run(pkg, monkeypatch, Y, po, 3, False)
    _check("run3 B materialised", _errs(mid, three["state"]), {k: 2 * v for k, v in TOL.items()})


def test_set_state_and_set_Y_between_runs(pkg, monkeypatch):
    """set_state and set_Y between runs are honoured (W cleared, G rebuilt for the new Y)."""
    L, M, H = 2000, 300, 32
    Y, po = _problem(L, M, H, 700)
    Y2, _ = _problem(L, M, H, 701)
    fresh = _run(pkg, monkeypatch, Y, po, 4, True)
    fresh2 = _run(pkg, monkeypatch, Y2, po, 4, True)
    with _ctx(pkg, monkeypatch, L, M, H, True) as c:
        c.set_Y(Y)
        _set(c, po)
        c.run(5, eps=0.0, est_covs=True, est_var=True)
        _set(c, po)
        c.run(4, eps=0.0, est_covs=True, est_var=True)
        after_state = c.get_state()
        c.set_Y(Y2)
        assert c.dims()["gram_built"] == 0
        _set(c, po)
        c.run(4, eps=0.0, est_covs=True, est_var=True)
        after_Y = c.get_state()
    _check("set_state between runs", _errs(after_state, fresh["state"]), dict(default=1e-7, sigma2=1e-7))
    _check("set_Y between runs", _errs(after_Y, fresh2["state"]), dict(default=1e-7, sigma2=1e-7))


def test_eps_stop_lands_on_the_same_sweep(pkg, monkeypatch):
    """The device-side stop test ends the Gram form at the sweep the oracle stops at; the state is that sweep's."""
    L, M, H = 2000, 300, 8
    Y, po = _problem(L, M, H, 800)
    g = _run(pkg, monkeypatch, Y, po, 200, True, eps=2e-3)
    s = _run(pkg, monkeypatch, Y, po, 200, False, eps=2e-3)
    _, n, _ = O.vbmf_(g["Ys"], po, 200, eps=2e-3, est_covs=True, est_var=True)
    assert 3 < n < 200
    assert g["it"] == s["it"] and abs(g["it"] - n) <= 1, (g["it"], s["it"], n)
    assert g["d"] <= 2e-3
    # the frozen state is that of the sweep the loop stopped at
    _, po2 = _problem(L, M, H, 800)
    same = _run(pkg, monkeypatch, Y, po2, g["it"], True)
    _check("frozen at the stop", _errs(g["state"], same["state"]), dict(default=1e-7, sigma2=1e-7))


def test_dispatch(pkg, monkeypatch):
    """The headline shape takes the Gram form by default; f32 Y, a row-sharded context and the sparse variant do not."""
    monkeypatch.delenv("VBMF_GRAM", raising=False)
    with pkg.capi.Context(100000, 10000, 64, y_dtype=pkg.VBMF_Y_BF16) as c:
        assert c.dims()["gram"] == 1
    with pkg.capi.Context(2400, 352, 64, y_dtype=pkg.VBMF_Y_BF16) as c:
        assert c.dims()["gram"] == 0                                  # below the size rule
    monkeypatch.setenv("VBMF_GRAM", "1")
    with pkg.capi.Context(2400, 352, 64, y_dtype=pkg.VBMF_Y_F32) as c:
        assert c.dims()["gram"] == 0
    with pkg.capi.Context(2400, 352, 200, y_dtype=pkg.VBMF_Y_BF16) as c:
        assert c.dims()["gram"] == 0                                  # Hp = 256
    with pkg.capi.Context(2400, 352, 64, y_dtype=pkg.VBMF_Y_BF16, variant=pkg.capi.VBMF_VARIANT_SPARSE_DIAG) as c:
        assert c.dims()["gram"] == 0
    with pkg.capi.Context(2400, 352, 64, y_dtype=pkg.VBMF_Y_BF16) as c:
        assert c.dims()["gram"] == 1
        c.comm_init(pkg.capi.Context.unique_id())
        assert c.dims()["gram"] == 0
    monkeypatch.setenv("VBMF_GRAM", "0")
    with pkg.capi.Context(100000, 10000, 64, y_dtype=pkg.VBMF_Y_BF16) as c:
        assert c.dims()["gram"] == 0
