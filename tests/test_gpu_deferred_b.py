"""GPU tests of B on demand after a Gram-form run ("Run boundaries").  A Gram-form run moves W, not B; the
streaming pass that materialises B of its last sweep is owed when the run returns and paid by the first entry point that reads B, its
tiles or anything derived from them.  Everything here is bitwise: who pays the pass, and when, changes no number the library returns.

Shapes: 2 400 x 352 at H = 16 and 64 (the basic model), H = 64 for the ARD-sparse diagonal model -- the small Gram-form shapes of
tests/test_gpu_gram_path.py, forced into the form by VBMF_GRAM at context creation."""
import numpy as np
import pytest

import __graft_entry__ as G
from oracle import vbmf_oracle as O
from tests.test_gram_sparse_identity import problem as sparse_problem

pytestmark = pytest.mark.gpu

L, M = 2400, 352
COL_OFF = np.array([0, 100, 229, 352], dtype=np.int64)


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


class Basic:
    keys = ("AHat", "BHat", "SigmaA", "SigmaB", "CA_diag", "CB_diag", "sigma2")

    def __init__(self, H):
        self.H = H
        rng = np.random.default_rng(4100 + H)
        _, A, B = O.toy_matrix(L, M, H, 0.05, rng)
        self.Y = (B * np.linspace(1.0, 3.0, H)) @ A.T + 0.05 * rng.standard_normal((L, M))
        self.po = O.vbmf_init(self.Y, H, ca=0.1, cb=0.1, sigma2=0.1, rng=np.random.default_rng(4101 + H), materialize_yhat=False)

    def ctx(self, pkg, env, gram=True):
        env.setenv("VBMF_GRAM", "1" if gram else "0")
        try:
            c = pkg.capi.Context(L, M, self.H, y_dtype=pkg.VBMF_Y_BF16, factor_dtype=pkg.VBMF_FACTOR_BF16X2)
        finally:
            env.delenv("VBMF_GRAM")
        assert c.dims()["gram"] == (1 if gram else 0)
        c.set_Y(self.Y)
        self.set(c)
        return c

    def set(self, c, B=None):
        po = self.po
        c.set_state(po.AHat, po.BHat if B is None else B, po.SigmaA, po.SigmaB, np.diag(po.CA), np.diag(po.CB), po.sigma2,
                    labels0=po.labels, H1=po.H1)

    def run(self, c, n):
        it, d, _ = c.run(n, eps=0.0, est_covs=True, est_var=True)
        assert it == n
        return d

    def state(self, c):
        return c.get_state()

    def calls(self, pkg):
        cap = pkg.capi
        A = self.po.AHat
        return {
            "yhat": (lambda c: c.YHat(), False),
            "elbo": (lambda c: np.float64(c.elbo()), True),
            "bag_residuals": (lambda c: c.bag_residuals(COL_OFF, A), False),
            "step": (lambda c: c.step(cap.STEP_A | cap.STEP_B | cap.STEP_CA | cap.STEP_CB | cap.STEP_SIGMA2), True),
            "step_a": (lambda c: c.step(cap.STEP_A), True),
            "fixed_basis": (lambda c: c.run_fixed_basis(3), True),
        }


class Sparse:
    keys = ("ATVecHat", "diagSigmaATVec", "CA", "beta", "SigmaA_diag", "BHat", "SigmaB", "CB", "delta", "sigmaHat", "zeta")

    def __init__(self, H, seed=None, repeat=False):
        """repeat: the reference's `repeat` layout of v (VBMF_COMPAT_SPARSE_REPEAT) instead of the consistent one"""
        self.H, self.repeat = H, repeat
        self.Y, self.po = sparse_problem(L, M, H, 4200 + H if seed is None else seed)

    def ctx(self, pkg, env, gram=True):
        cap = pkg.capi
        env.setenv("VBMF_GRAM", "2" if gram else "0")
        rc = cap.VBMF_COMPAT_DEFAULT if self.repeat else (cap.VBMF_COMPAT_DEFAULT & ~cap.VBMF_COMPAT_SPARSE_REPEAT)
        try:
            c = cap.Context(L, M, self.H, y_dtype=pkg.VBMF_Y_BF16, factor_dtype=pkg.VBMF_FACTOR_BF16X2,
                            variant=cap.VBMF_VARIANT_SPARSE_DIAG, reference_compat=rc)
        finally:
            env.delenv("VBMF_GRAM")
        assert c.dims()["gram"] == (1 if gram else 0)
        c.set_Y(self.Y)
        self.set(c)
        return c

    def set(self, c, B=None):
        po = self.po
        hyper = dict(alpha0=po.alpha0, beta0=po.beta0, gamma0=po.gamma0, delta0=po.delta0, eta0=po.eta0, zeta0=po.zeta0)
        c.sparse_set_state(po.ATVecHat, po.diagSigmaATVec, po.CA, po.beta, po.BHat if B is None else B, po.SigmaB, po.CB, po.delta,
                           po.sigmaHat, po.zeta, hyper, labels0=po.labels, H1=po.H1)

    def run(self, c, n):
        it, d, _ = c.sparse_run(n, eps=0.0, est_cb=True)
        assert it == n
        return d

    def state(self, c):
        return c.sparse_get_state()

    def calls(self, pkg):
        cap = pkg.capi
        return {
            "yhat": (lambda c: c.YHat(), False),
            "lower_bound": (lambda c: np.float64(c.sparse_lower_bound()), True),
            "step": (lambda c: c.sparse_step(cap.SSTEP_A | cap.SSTEP_B | cap.SSTEP_CA | cap.SSTEP_CB | cap.SSTEP_SIGMA), True),
            "fixed_basis": (lambda c: c.sparse_run_fixed_basis(3), True),
        }


_MODELS = {}


def model(name):
    """the problem of a case, built once: "basic16", "basic64", "sparse64" """
    if name not in _MODELS:
        _MODELS[name] = (Sparse if name.startswith("sparse") else Basic)(int(name[-2:]))
    return _MODELS[name]


def same(tag, m, a, b):
    for k in m.keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and np.array_equal(x, y), (tag, k, float(np.max(np.abs(x - y))))


ORDER_CASES = ([("basic16", k) for k in ("yhat", "elbo", "bag_residuals", "step", "step_a", "fixed_basis")] +
               [("basic64", k) for k in ("yhat", "elbo", "step", "fixed_basis")] +
               [("sparse64", k) for k in ("yhat", "lower_bound", "step", "fixed_basis")])


@pytest.mark.parametrize("name,call", ORDER_CASES, ids=[f"{n}-{k}" for n, k in ORDER_CASES])
def test_first_reader_of_B_does_not_matter(pkg, monkeypatch, name, call):
    """Two contexts run the same six sweeps.  X reads the state at once, then makes a call that consumes B; Y makes that call first,
    with B still owed, and reads the state afterwards.  The call returns the same bits to both, and both end in the same state; a
    call that leaves the state alone also leaves Y's state equal to what X read before it."""
    m = model(name)
    fn, mutates = m.calls(pkg)[call]
    with m.ctx(pkg, monkeypatch) as x, m.ctx(pkg, monkeypatch) as y:
        assert m.run(x, 6) == m.run(y, 6)
        assert x.dims()["b_pending"] == 1 and y.dims()["b_pending"] == 1
        sx0 = m.state(x)
        assert x.dims()["b_pending"] == 0 and x.dims()["b_materialised"] == 1
        ry = fn(y)
        assert y.dims()["b_pending"] == 0 and y.dims()["b_materialised"] == 1
        rx = fn(x)
        sy1 = m.state(y)
        sx1 = m.state(x)
        assert x.dims()["b_materialised"] == 1 and y.dims()["b_materialised"] == 1
    if rx is not None or ry is not None:
        assert np.array_equal(np.asarray(rx), np.asarray(ry)), (name, call)
    same(f"{name} {call}: end states", m, sx1, sy1)
    if not mutates:
        same(f"{name} {call}: the call left the state alone", m, sx0, sy1)


@pytest.mark.parametrize("name", ["basic16", "basic64", "sparse64"])
def test_chunked_run_pays_no_pass_between_chunks(pkg, monkeypatch, name):
    """run(2) three times with no read in between equals run(6), B included, and no streaming pass materialises B between the
    chunks: the debt stays open (dims()["b_pending"]) and the on-demand pass has not run (dims()["b_materialised"]) until the read."""
    m = model(name)
    with m.ctx(pkg, monkeypatch) as c:
        d6 = m.run(c, 6)
        s6 = m.state(c)
    with m.ctx(pkg, monkeypatch) as c:
        for i in range(3):
            d = m.run(c, 2)
            dm = c.dims()
            assert dm["b_pending"] == 1 and dm["b_materialised"] == 0, (i, dm)
        s222 = m.state(c)
        dm = c.dims()
        assert dm["b_pending"] == 0 and dm["b_materialised"] == 1, dm
        again = m.state(c)                                   # a second read pays nothing and sees the same B
        assert c.dims()["b_materialised"] == 1
    assert d == d6
    same(f"{name}: run(2) x 3 vs run(6)", m, s222, s6)
    same(f"{name}: second read", m, again, s222)


@pytest.mark.parametrize("name", ["basic16", "basic64", "sparse64"])
def test_set_state_drops_the_owed_B(pkg, monkeypatch, name):
    """set_state after a Gram-form run: the B that was owed is never made, and the next read returns exactly the B that was set
    (as a context that never ran returns it: the device stores B in bf16 hi + lo)."""
    m = model(name)
    B2 = 0.5 * m.po.BHat[::-1].copy() + 0.25
    with m.ctx(pkg, monkeypatch) as c:
        m.set(c, B2)
        fresh = m.state(c)
    with m.ctx(pkg, monkeypatch) as c:
        m.run(c, 4)
        assert c.dims()["b_pending"] == 1
        m.set(c, B2)
        dm = c.dims()
        assert dm["b_pending"] == 0 and dm["b_materialised"] == 0, dm
        got = m.state(c)
        assert c.dims()["b_materialised"] == 0
    same(f"{name}: state after set_state", m, got, fresh)


@pytest.mark.parametrize("name", ["basic16", "basic64", "sparse64"])
def test_streaming_run_after_a_gram_run_starts_from_the_owed_B(pkg, monkeypatch, name):
    """A run forced back to the streaming path (set_gram_form OFF) after a Gram-form run starts from the materialised B: its
    result equals that of a context that read B in between."""
    m = model(name)
    off = pkg.capi.VBMF_GRAM_FORM_OFF
    res = []
    for read_between in (False, True):
        with m.ctx(pkg, monkeypatch) as c:
            m.run(c, 3)
            assert c.dims()["b_pending"] == 1
            if read_between:
                m.state(c)
            c.set_gram_form(off)
            assert c.dims()["gram"] == 0 and c.dims()["b_pending"] == 0 and c.dims()["b_materialised"] == 1
            d = m.run(c, 3)
            assert c.dims()["b_pending"] == 0 and c.dims()["b_materialised"] == 1
            res.append((d, m.state(c)))
    assert res[0][0] == res[1][0]
    same(f"{name}: streaming run after a Gram-form run", m, res[0][1], res[1][1])
