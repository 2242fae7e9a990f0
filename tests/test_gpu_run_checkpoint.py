"""GPU tests of the run loops' look at the device's stop flag (vbmf_run, vbmf_sparse_run).  The host runs ahead of the device and
looks every 8 sweeps at host-mapped words the device's loop test stores into; sweeps enqueued past a stop are no-ops on the device.
A stop that falls BETWEEN two looks must therefore leave exactly the state of the sweep it happened at, and the words of one run
must not reach the next.  Everything is bitwise.  2 400 x 352, H = 16, in the Gram form and on the streaming path."""
import numpy as np
import pytest

import __graft_entry__ as G
from tests.test_gpu_deferred_b import Basic, Sparse, same

pytestmark = pytest.mark.gpu

NITER = 40


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


_MODELS = {}


def model(kind):
    """The sparse model's d does not fall steadily on this data: on most seeds it settles near 1 within a few sweeps, and no eps
    then stops a run between sweeps 9 and 15.  Seed 4302 in the reference's `repeat` layout is one on which d of the fp64 oracle
    falls by more than a third per sweep from sweep 10 to 15 (scanned on the oracle, seeds 4300-4311)."""
    if kind not in _MODELS:
        _MODELS[kind] = Sparse(16, seed=4302, repeat=True) if kind == "sparse" else Basic(16)
    return _MODELS[kind]


def ctx(pkg, env, m, gram):
    return m.ctx(pkg, env, gram)


def run(m, c, n, eps):
    if isinstance(m, Sparse):
        return c.sparse_run(n, eps=eps, est_cb=True, want_trace=True)
    return c.run(n, eps=eps, est_covs=True, est_var=True, want_trace=True)


def stop_sweep(d):
    """a sweep near 11, strictly between the looks at 8 and 16, whose d is below every earlier one: eps = d of that sweep stops there"""
    for k in (11, 10, 12, 13, 9, 14, 15):
        if np.all(d[:k - 1] > d[k - 1]):
            return k
    raise AssertionError(f"no sweep between two looks at which an eps stops this run: {d[:16]}")


@pytest.mark.parametrize("gram", [True, False], ids=["gram", "stream"])
@pytest.mark.parametrize("kind", ["basic", "sparse"])
def test_stop_between_two_looks(pkg, monkeypatch, kind, gram):
    """eps from the recorded d trace of the same seeded run stops the run at sweep k, 8 < k < 16: the iteration count, d, the trace
    (exactly k rows) and the whole state are those of run(k) with eps = 0.  Then a second run on the same context does not stop at
    once: it runs all its sweeps."""
    m = model(kind)
    with ctx(pkg, monkeypatch, m, gram) as c:
        it0, _, tr0 = run(m, c, NITER, 0.0)
    assert it0 == NITER and tr0.shape == (NITER, 4)
    d = tr0[:, 0]
    k = stop_sweep(d)
    eps = float(d[k - 1])
    with ctx(pkg, monkeypatch, m, gram) as c:
        it, dl, tr = run(m, c, NITER, eps)
        st = m.state(c)
        it2, _, tr2 = run(m, c, 20, 0.0)                     # a stale stop word would end this run at its first look
    assert it == k, (it, k, d[:16])
    assert dl == d[k - 1]
    assert tr.shape == (k, 4) and np.array_equal(tr, tr0[:k])
    assert it2 == 20 and tr2.shape == (20, 4) and np.all(tr2[:, 0] > 0)
    with ctx(pkg, monkeypatch, m, gram) as c:
        itk, dk, trk = run(m, c, k, 0.0)
        sk = m.state(c)
    assert itk == k and dk == dl and np.array_equal(trk, tr)
    same(f"{kind}: eps stop at {k} vs run({k})", m, st, sk)
