"""GPU tests of the Gram-form sweep's control chain: the fp64 H x H chain runs as two launches of two
workgroups each, with the closing step of a sweep (CA, CB, sigma2, ELBO, d, stop test) riding in the next sweep's first launch
and a speculative SigmaA committed in its second.  These checks are bitwise: the split moves no input of any fp64 operation."""
import numpy as np
import pytest

import __graft_entry__ as G
from oracle import vbmf_oracle as O

pytestmark = pytest.mark.gpu

KEYS = ("AHat", "BHat", "SigmaA", "SigmaB", "CA_diag", "CB_diag", "sigma2")


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


def _problem(L, M, H, seed):
    """test_gpu_gram_path.py's well-conditioned data: H latent columns of distinct scales."""
    rng = np.random.default_rng(seed)
    _, A, B = O.toy_matrix(L, M, H, 0.05, rng)
    Y = (B * np.linspace(1.0, 3.0, H)) @ A.T + 0.05 * rng.standard_normal((L, M))
    po = O.vbmf_init(Y, H, ca=0.1, cb=0.1, sigma2=0.1, rng=np.random.default_rng(seed + 1), materialize_yhat=False)
    return Y, po


def _ctx(pkg, monkeypatch, L, M, H, gram):
    monkeypatch.setenv("VBMF_GRAM", "1" if gram else "0")
    c = pkg.capi.Context(L, M, H, y_dtype=pkg.VBMF_Y_BF16, factor_dtype=pkg.VBMF_FACTOR_BF16X2)
    monkeypatch.delenv("VBMF_GRAM")
    return c


def _set(c, po):
    c.set_state(po.AHat, po.BHat, po.SigmaA, po.SigmaB, np.diag(po.CA), np.diag(po.CB), po.sigma2, labels0=po.labels, H1=po.H1)


def _runs(pkg, monkeypatch, Y, po, plan, gram=True):
    """One context; runs (niter, eps) one after the other from the initial state.  Returns [(iters, d, trace, state)]."""
    L, M = Y.shape
    out = []
    with _ctx(pkg, monkeypatch, L, M, po.H, gram) as c:
        assert c.dims()["gram"] == (1 if gram else 0)
        c.set_Y(Y)
        _set(c, po)
        for n, eps in plan:
            it, d, tr = c.run(n, eps=eps, est_covs=True, est_var=True, want_trace=True)
            out.append((it, d, tr.copy(), c.get_state()))
    return out


def _same(tag, a, b):
    for k in KEYS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and np.array_equal(x, y), (tag, k, np.max(np.abs(x - y)))


def _complete(tag, it, tr):
    """Every executed sweep filed d, sigma2, ELBO and the residual (the trace buffer starts as zeros)."""
    assert tr.shape == (it, 4), (tag, tr.shape)
    assert np.all(np.isfinite(tr)), (tag, tr)
    assert np.all(tr[:, 0] > 0) and np.all(tr[:, 1] > 0) and np.all(tr[:, 3] != 0) and np.all(tr[:, 2] != 0), (tag, tr)


SHAPES = {16: (2000, 300), 64: (2400, 512), 128: (3000, 1024)}


@pytest.mark.parametrize("H", [16, 64, 128])
def test_split_runs_equal_one_run_bitwise(pkg, monkeypatch, H):
    """run(3) + run(3) equals run(6) bitwise, trace included: nothing of the chain carries across vbmf_run calls."""
    L, M = SHAPES[H]
    Y, po = _problem(L, M, H, 900 + H)
    (it6, d6, tr6, s6), = _runs(pkg, monkeypatch, Y, po, [(6, 0.0)])
    (ia, _, tra, _), (ib, db, trb, s33) = _runs(pkg, monkeypatch, Y, po, [(3, 0.0), (3, 0.0)])
    assert it6 == 6 and ia == ib == 3
    _complete("run6", it6, tr6)
    _complete("run3", ia, tra)
    _complete("run3+3", ib, trb)
    _same("run3+run3 vs run6", s33, s6)
    assert db == d6
    # the first sweep of each run (streaming for the first run, Gram form for the second) files the same row as in run(6)
    assert np.array_equal(np.vstack([tra, trb]), tr6)


@pytest.mark.parametrize("H", [16, 64, 128])
def test_eps_stop_freezes_the_state_of_its_sweep(pkg, monkeypatch, H):
    """An eps stop at sweep k leaves the state of run(k, eps = 0) bitwise: the speculative SigmaA of sweep k + 1 is not
    committed, and CA, CB and sigma2 of sweep k are filed.  The stop lands at the first sweep whose d is <= eps."""
    L, M = SHAPES[H]
    Y, po = _problem(L, M, H, 950 + H)
    n = 8
    (it0, _, tr0, _), = _runs(pkg, monkeypatch, Y, po, [(n, 0.0)])
    assert it0 == n
    d = tr0[:, 0]
    for k in (1, 2, 3, 5):
        eps = float(d[k - 1])
        expect = 1 + int(np.argmax(d <= eps))                    # first sweep whose d is at or below eps (k or earlier)
        (it, dl, tr, st), = _runs(pkg, monkeypatch, Y, po, [(n, eps)])
        assert it == expect, (k, it, expect, d)
        assert dl == d[expect - 1]
        _complete(f"stop {k}", it, tr)
        assert np.array_equal(tr, tr0[:expect])
        (itk, _, trk, sk), = _runs(pkg, monkeypatch, Y, po, [(expect, 0.0)])
        assert itk == expect and np.array_equal(trk, tr)
        _same(f"eps stop at {expect} vs run({expect})", st, sk)


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("H", [16, 64, 128])
def test_stop_on_the_first_sweeps_matches_streaming(pkg, monkeypatch, H, k):
    """The run ends on its first sweep (streaming), on the first Gram-form sweep, or on the one after: niter = k gives k complete
    trace rows, and an eps stop at sweep k lands where the streaming path's does."""
    L, M = SHAPES[H]
    # seeds on which d falls over the first three sweeps by > 10 % each (checked on the fp64 oracle; on most problems of these
    # shapes d of the third sweep is above the second's, and no eps then stops a run there)
    Y, po = _problem(L, M, H, {16: 1016, 64: 1065, 128: 1137}[H])
    (it, _, tr, _), = _runs(pkg, monkeypatch, Y, po, [(k, 0.0)])
    assert it == k
    _complete(f"niter {k}", it, tr)
    (_, _, trs, _), = _runs(pkg, monkeypatch, Y, po, [(6, 0.0)], gram=False)
    ds = trs[:, 0]
    # eps half-way (geometrically) between the streaming path's d of sweeps k - 1 and k, which must be well apart for the two
    # paths to agree on the side of eps; k = 1: above d of the first sweep
    if k == 1:
        eps = 2.0 * float(ds[0])
    else:
        assert ds[k - 1] < 0.9 * ds[k - 2] and np.all(ds[:k - 2] > ds[k - 2]), ds
        eps = float(np.sqrt(ds[k - 2] * ds[k - 1]))
    (ig, _, trg, _), = _runs(pkg, monkeypatch, Y, po, [(20, eps)])
    (is_, _, _, _), = _runs(pkg, monkeypatch, Y, po, [(20, eps)], gram=False)
    assert ig == is_ == k, (ig, is_, k, ds)
    _complete(f"eps stop at {k}", ig, trg)
    assert np.array_equal(trg, tr)
