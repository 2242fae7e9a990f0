"""The five many-bags entries share ONE device scratch buffer (csrc/host_bags.hpp), each in its own layout.  Whatever an entry finds
there -- another entry's bytes, or its own from a call with another bag count, which moves every slot behind the offset table --
must not reach its results: every call of a mixed sequence on one context returns, bit for bit, what the same call returns as the
first and only bag call of a fresh context with the same Y and state.  Device result against device result: no tolerance."""
import numpy as np
import pytest

import __graft_entry__ as G

pytestmark = pytest.mark.gpu

L, M, H = 33, 41, 5
PART_A = np.cumsum([0, 1, 9, 8, 23])          # a one-column bag, one wider than a residual slice (8 columns), one exactly a slice wide
PART_B = np.arange(M + 1)                     # 41 one-column bags: a larger offset table, every later slot moves
PARTS = {"A": PART_A.astype(np.int64), "B": PART_B.astype(np.int64)}

_rng = np.random.default_rng(20241018)
Y = _rng.integers(-3, 4, (L, M)).astype(np.float64)          # integer-valued: exact in bf16 as in fp32
B0 = _rng.standard_normal((L, H))                            # the contexts' basis
BLS = _rng.standard_normal((L, H))                           # the caller's basis of bag_least_squares
A0 = _rng.standard_normal((M, H))                            # the caller's AHat of bag_residuals / the bound
HYPER = dict(alpha0=1e-3, beta0=1e-3, gamma0=1e-3, delta0=1e-3, eta0=1e-3, zeta0=1e-3)


@pytest.fixture(scope="module")
def pkg():
    G.build()
    p = G.load_package()
    yield p
    p.set_defaults(y_dtype=p.VBMF_Y_F32, factor_dtype=p.VBMF_FACTOR_AUTO)


def _context(pkg, ydt, sparse):
    C = pkg.capi
    c = C.Context(L, M, H, y_dtype=ydt, variant=C.VBMF_VARIANT_SPARSE_DIAG if sparse else C.VBMF_VARIANT_BASIC)
    c.set_Y(Y)
    if sparse:
        c.sparse_set_state(A0.reshape(-1), np.full(M * H, 0.3), np.full(M * H, 0.7), np.full(M * H, 2.0), B0, 0.01 * np.eye(H),
                           np.ones(H), np.ones(H), 3.0, 7.0, HYPER)
    else:
        c.set_state(np.zeros((M, H)), B0, np.zeros((H, H)), 0.01 * np.eye(H), np.ones(H), np.ones(H), 0.1)
    return c


# ---- the calls: (context, col_off) -> list of output arrays --------------------------------------------------------------------
def _arrays(out):
    vals = out.values() if isinstance(out, dict) else out
    return [np.asarray(v, dtype=np.float64) for v in vals if v is not None]


def _vbls(c, off):
    n = off.size - 1
    return _arrays(c.run_fixed_basis_batched(off, 10, np.full(n, 0.1), np.linspace(0.5, 1.5, n * H).reshape(n, H)))


def _resid(c, off):
    return [c.bag_residuals(off, A0)]


def _ls(lam):
    return lambda c, off: _arrays(c.bag_least_squares(off, BLS, lam))


def _svbls(full_cov):
    def call(c, off):
        n = off.size - 1
        return _arrays(c.sparse_run_fixed_basis_batched(off, 10, np.full((n, H), 0.5), np.full((n, H), 1e-3), np.full(n, 40.0),
                                                        np.full(n, 1e-3), np.linspace(20.0, 30.0, n), np.ones(M * H), full_cov=full_cov))
    return call


def _bound(c, off):
    n = off.size - 1
    return _arrays(c.sparse_lower_bound_batched(off, A0.reshape(-1), np.full(M * H, 0.3), np.full(M * H, 0.7), np.full(M * H, 2.0),
                                                np.tile(np.eye(H) * 0.1, (n, 1, 1)), np.full(n, 3.0), np.full(n, 7.0), np.full(n, 40.0),
                                                np.full(n, 1e-3), np.full(n, 1e-3), np.full((n, H), 1e-3), np.full((n, H), 1e-3),
                                                np.full((n, H), 0.501)))


def _sequence(model):
    if model == "basic":
        return [("vbls", _vbls, "A"), ("resid", _resid, "B"), ("ls0", _ls(0.0), "A"), ("ls0.5", _ls(0.5), "A"), ("vbls", _vbls, "B"),
                ("resid", _resid, "A"), ("ls0", _ls(0.0), "B")]
    full_cov = model == "sparse_full"
    return [("svbls", _svbls(full_cov), "A"), ("bound", _bound, "B"), ("resid", _resid, "A"), ("svbls", _svbls(full_cov), "B"),
            ("bound", _bound, "A")]


@pytest.mark.parametrize("model", ["basic", "sparse_diag", "sparse_full"])
@pytest.mark.parametrize("ydt", ["F32", "BF16"])
def test_no_call_sees_what_another_left_in_the_buffer(pkg, ydt, model):
    ydt = getattr(pkg, "VBMF_Y_" + ydt)
    sparse = model != "basic"
    seq = _sequence(model)
    with _context(pkg, ydt, sparse) as c:
        got = [call(c, PARTS[part]) for _, call, part in seq]
    for (name, call, part), out in zip(seq, got):
        with _context(pkg, ydt, sparse) as fresh:                       # this call as the context's first and only bag call
            ref = call(fresh, PARTS[part])
        assert len(out) == len(ref) and len(out) > 0, (name, part)
        for k, (a, b) in enumerate(zip(out, ref)):
            assert np.isfinite(b).all(), (name, part, k)
            assert a.shape == b.shape and np.array_equal(a, b), (name, part, k, float(np.max(np.abs(a - b))))
