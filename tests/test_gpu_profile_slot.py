"""GPU tests of the Gram form's profile slot (vbmf_profile_enable / vbmf_profile_read): slot 1 brackets the launch of gram_prod that the
stride selects with a pair of HIP events; launches the stride does not select are plain launches.  The slot counts and times what
it says, and profiling does not change a bit of the state.  With B materialised on demand, a profiled Gram-form run also files
nothing in slot 2: no streaming pass runs inside it.
2 400 x 352, H = 64, twelve Gram-form sweeps behind a two-sweep run that leaves W valid."""
import time

import numpy as np
import pytest

import __graft_entry__ as G
from tests.test_gpu_deferred_b import model, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


@pytest.fixture(scope="module")
def unprofiled(pkg):
    """the state after run(2) + run(12) with profiling off: the reference of both strides, computed once"""
    m = model("basic64")
    mp = pytest.MonkeyPatch()
    try:
        with m.ctx(pkg, mp) as c:
            m.run(c, 2)
            d = m.run(c, 12)
            return d, m.state(c)
    finally:
        mp.undo()


@pytest.mark.parametrize("stride,expect_n", [(1, 12), (4, 3)])
def test_gram_slot_counts_and_times(pkg, monkeypatch, unprofiled, stride, expect_n):
    m = model("basic64")
    with m.ctx(pkg, monkeypatch) as c:
        m.run(c, 2)                                          # the streaming first sweep and one Gram-form sweep: W is valid
        c.profile_enable(stride)
        c.sync()
        t0 = time.perf_counter()
        d = m.run(c, 12)
        c.sync()
        wall_ms = 1e3 * (time.perf_counter() - t0)
        prof = c.profile_read()
        c.profile_enable(False)
        st = m.state(c)
    print(f"stride {stride}: pass1_n {prof['pass1_n']}, pass1_ms {prof['pass1_ms']:.4f}, wall {wall_ms:.3f} ms")
    assert prof["pass1_n"] == expect_n, prof
    assert prof["pass2_n"] == 0, prof                        # no streaming pass: B of the last sweep is still owed
    assert 0.0 < prof["pass1_ms"] < wall_ms, (prof, wall_ms)
    assert np.isfinite(prof["pass1_ms"])
    d0, s0 = unprofiled
    assert d == d0
    same(f"stride {stride}: state vs profiling off", m, st, s0)
