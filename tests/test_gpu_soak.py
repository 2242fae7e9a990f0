"""Robustness of the device loop over many sweeps and many handles: no drift into non-finite values, no dependence on
how the sweeps are chunked into calls, no device-memory leak across create/destroy, errors leave the handle usable."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as G
from oracle import vbmf_oracle as O
from tests.helpers import relF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


def _free_bytes():
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_two_thousand_sweeps_and_chunking(pkg):
    """2000 sweeps in one call (the host only looks at the device every 8 sweeps) == the same 2000 sweeps in uneven chunks."""
    L, M, H = 2000, 600, 8
    rng = np.random.default_rng(1)
    Bs = rng.standard_normal((L, H)) * np.linspace(1.0, 3.0, H)
    As = np.zeros((M, H)); As[np.arange(M), rng.integers(0, H, M)] = 1.0
    Y = Bs @ As.T + 0.05 * rng.standard_normal((L, M))
    A0, B0 = rng.standard_normal((M, H)), rng.standard_normal((L, H))
    z = np.zeros((H, H))
    out = []
    for chunks in ([2000], [1, 7, 8, 9, 975, 1000]):
        with pkg.capi.Context(L, M, H, y_dtype=pkg.VBMF_Y_BF16) as c:
            c.set_Y(Y)
            c.set_state(A0, B0, z, z, 0.1 * np.ones(H), 0.1 * np.ones(H), 0.1)
            total = 0
            for k in chunks:
                it, d, _ = c.run(k, eps=0.0, est_covs=True, est_var=True)
                total += it
            out.append((total, d, c.get_state(), c.elbo()))
    (n0, d0, s0, e0), (n1, d1, s1, e1) = out
    assert n0 == n1 == 2000
    for k in ("AHat", "BHat", "SigmaA", "SigmaB", "CA_diag", "CB_diag"):
        assert np.all(np.isfinite(s0[k])), k
    assert np.isfinite(d0) and np.isfinite(e0) and s0["sigma2"] > 0
    # chunk boundaries re-enter through the host (state kept on the device): same fixed point, tiny path differences
    assert relF(s1["AHat"], s0["AHat"]) < 1e-4 and relF(s1["BHat"], s0["BHat"]) < 1e-4
    assert abs(s1["sigma2"] - s0["sigma2"]) < 1e-3 * s0["sigma2"] and abs(e1 - e0) < 1e-5 * abs(e0)
    # converged: the factorization explains the data to the noise level
    assert relF(s0["BHat"] @ s0["AHat"].T, Bs @ As.T) < 0.05


def test_create_destroy_does_not_leak(pkg):
    rng = np.random.default_rng(2)
    Y = rng.standard_normal((3000, 900))

    def cycle(variant):
        with pkg.capi.Context(3000, 900, 40, y_dtype=pkg.VBMF_Y_BF16, variant=variant) as c:
            c.set_Y(Y)

    for v in (pkg.capi.VBMF_VARIANT_BASIC, pkg.capi.VBMF_VARIANT_SPARSE_DIAG, pkg.capi.VBMF_VARIANT_SPARSE_DIAGVAR):
        cycle(v)                                  # warm the allocator's pools
    before = _free_bytes()
    for i in range(30):
        cycle((pkg.capi.VBMF_VARIANT_BASIC, pkg.capi.VBMF_VARIANT_SPARSE_DIAG, pkg.capi.VBMF_VARIANT_SPARSE_DIAGVAR)[i % 3])
    after = _free_bytes()
    assert before - after < 64 << 20, (before, after)          # well under one context's footprint (~30 MB of tiles each)


def _gram_group_bytes(d, M):
    """Bytes of the eight buffers gram_prepare allocates together (csrc/vbmf_hip.hip), from dims() after a Gram-form run."""
    Hp, NH, XT1, nsplit = d["Hp"], d["NH"], d["XT1"], d["gram_nsplit"]
    GT = -(-XT1 // 16) * 16
    KT, n = 2 * GT, Hp * XT1 * 32
    nchunk = max(1, min(32 if Hp == 256 else 64 if Hp == 128 else 128, -(-M // 64)))
    rpc = -(-(-(-M // nchunk)) // 16) * 16
    nchunk = -(-M // rpc)
    return (GT * KT * 64 * 8 * 4                    # Gt
            + 2 * 32 * GT * Hp * 4                  # W32g[0], W32g[1]
            + 5 * KT * NH * 64 * 16                 # Wt (GRAM_PLANES = 5)
            + 2 * n * 4                             # gPQ
            + (nsplit * 2 * n * 4 if nsplit > 1 else 0)   # gslabs
            + nchunk * (2 * Hp * Hp + 2) * 8        # g_part
            + (2 * Hp * Hp + 8) * 8)                # gsave


def test_lazy_buffers_do_not_leak(pkg):
    """Create, use and destroy four contexts and one preprocess plan per cycle, so that every lazily allocated device buffer exists
    when its context goes: the Gram-form group, the many-bags scratch (grown once), the run trace, fws / fpart / t2part (rank
    130: the side stream too), gw (diag_var) and the plan's four buffers.  After one warming cycle, 20 cycles may lower the
    device's free memory by less than the basic context's Gram-form group of ONE cycle (23 069 120 bytes): a leak of that group, or of
    anything larger, per cycle shows twentyfold.  Buffers too small for this count (t2part, hmean) are held by the counting
    allocator of tests/ctx_mem_check.cpp.
    Measured on an MI355X before csrc/ctx_mem.hpp existed (the hand-written free lists): a drop of 0 bytes over the 20 cycles."""
    cap = pkg.capi
    rng = np.random.default_rng(7)
    L0, M0, H0 = 2048, 1536, 40
    Y0 = rng.standard_normal((L0, H0)) @ rng.standard_normal((H0, M0)) + 0.05 * rng.standard_normal((L0, M0))
    A0, B0 = rng.standard_normal((M0, H0)), rng.standard_normal((L0, H0))
    z0 = np.zeros((H0, H0))
    L1, M1 = 512, 96
    sparse = {}
    for H in (130, 40):
        Y, _, _ = O.toy_matrix(L1, M1, 8, 0.05, np.random.default_rng(70 + H))
        po = O.vbmf_sparse_init(Y, H, ca=0.1, cb=0.1, sigma=0.1, rng=np.random.default_rng(71 + H), full_cov=False,
                                materialize_yhat=False)
        sparse[H] = (Y, po, dict(alpha0=po.alpha0, beta0=po.beta0, gamma0=po.gamma0, delta0=po.delta0, eta0=po.eta0, zeta0=po.zeta0))
    Yraw = rng.standard_normal((L1, M1)) * rng.uniform(0.5, 20.0, (L1, 1)) + rng.uniform(-5.0, 5.0, (L1, 1))

    def sparse_ctx(variant, H, niter, trace):
        Y, po, hyper = sparse[H]
        with cap.Context(L1, M1, H, y_dtype=pkg.VBMF_Y_BF16, variant=variant) as c:
            c.set_Y(Y)
            c.sparse_set_state(po.ATVecHat, po.diagSigmaATVec, po.CA, po.beta, po.BHat, po.SigmaB, po.CB, po.delta, po.sigmaHat,
                               po.zeta, hyper)
            c.sparse_set_full_cov(True)
            if variant == cap.VBMF_VARIANT_SPARSE_DIAGVAR:
                c.sparse_set_noise_rows(np.ones(L1), 1e-10 * np.ones(L1), 1e-10 + M1 / 2)
            it, _, tr = c.sparse_run(niter, eps=0.0, est_cb=True, want_trace=trace)
            assert it == niter and (tr is None or tr.shape == (niter, 4))
            if variant == cap.VBMF_VARIANT_SPARSE_DIAGVAR:
                with cap.PreprocessPlan(Yraw) as plan:
                    assert plan.L_used == L1
                    c.set_Y_preprocessed(plan, 1.0)

    def cycle():
        with cap.Context(L0, M0, H0, y_dtype=pkg.VBMF_Y_BF16) as c:
            c.set_Y(Y0)
            c.set_state(A0, B0, z0, z0, 0.1 * np.ones(H0), 0.1 * np.ones(H0), 0.1)
            c.set_gram_form(cap.VBMF_GRAM_FORM_ON)
            it, _, tr = c.run(4, eps=0.0, est_covs=True, est_var=True, want_trace=True)
            d = c.dims()
            assert it == 4 and tr.shape == (4, 4) and d["gram"] == 1 and d["gram_built"] == 1, d
            for nb in (2, 16):                      # the second call needs more scratch than the first: c->bags is regrown
                off = np.linspace(0, M0, nb + 1).astype(np.int64)
                c.run_fixed_basis_batched(off, 2, 0.1 * np.ones(nb), 0.1 * np.ones((nb, H0)))
            c.YHat(); c.get_Y(); c.get_state()
        sparse_ctx(cap.VBMF_VARIANT_SPARSE_DIAG, 130, 2, True)
        sparse_ctx(cap.VBMF_VARIANT_SPARSE_DIAG, 40, 2, False)
        sparse_ctx(cap.VBMF_VARIANT_SPARSE_DIAGVAR, 40, 2, False)
        return _gram_group_bytes(d, M0)

    bound = cycle()                                 # warms the runtime's pools
    assert bound > 9 << 20, bound                   # G alone is 9 MB at M = 1536
    before = _free_bytes()
    for _ in range(20):
        cycle()
    after = _free_bytes()
    print(f"lazy buffers: free memory dropped by {before - after} bytes over 20 cycles (bound {bound})")
    assert before - after < bound, (before, after, bound)


def test_numeric_error_leaves_the_handle_usable(pkg):
    """A singular posterior precision (all-zero data and zero prior precisions) is reported as VBMF_ERR_NUMERIC; the same
    handle then runs a well-posed state."""
    L, M, H = 64, 48, 3
    rng = np.random.default_rng(3)
    z = np.zeros((H, H))
    with pkg.capi.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32) as c:
        c.set_Y(rng.standard_normal((L, M)))
        c.set_state(np.zeros((M, H)), np.zeros((L, H)), z, z, np.full(H, np.inf), np.full(H, np.inf), 0.1)
        with pytest.raises(pkg.VbmfError) as ei:
            c.run(3, eps=0.0, est_covs=True, est_var=True)
        assert ei.value.code == -4
        c.set_state(rng.standard_normal((M, H)), rng.standard_normal((L, H)), z, z, 0.1 * np.ones(H), 0.1 * np.ones(H), 0.1)
        it, d, _ = c.run(3, eps=0.0, est_covs=True, est_var=True)
        assert it == 3 and np.isfinite(d) and np.all(np.isfinite(c.get_state()["BHat"]))


def test_epilogue_handoff_timeout_is_reported(pkg):
    """The Y*A pass's register epilogue waits (bounded) for the SigmaB table that control workgroup 0 of the SAME launch
    releases.  Force the wait to fail (the epilogue is told to expect a sequence number nobody publishes, with a short spin
    limit): the run must come back with VBMF_ERR_SYNC and its own message -- not hang, not be folded into the pivot error --
    and the handle must run normally afterwards.  (In every other GPU test a run that returns OK has I_ERR == 0 on the
    device: vbmf_run fails on any non-zero value.)"""
    L, M, H = 70000, 1100, 48                                   # un-split Y*A pass at H <= 64: the register-epilogue path
    rng = np.random.default_rng(5)
    A0, B0 = rng.standard_normal((M, H)), rng.standard_normal((L, H))
    z = np.zeros((H, H))
    with pkg.capi.Context(L, M, H, y_dtype=pkg.VBMF_Y_BF16) as c:
        dims = c.dims()
        if dims["nsplit2"] != 1 or dims["NH"] > 2 or dims["narrow"]:
            pytest.skip(f"planner did not choose the un-split pass here: {dims}")
        c.set_Y_synthetic(11, H, 0.05)
        c.set_state(A0, B0, z, z, 0.1 * np.ones(H), 0.1 * np.ones(H), 0.1)
        it, d, _ = c.run(3, eps=0.0, est_covs=True, est_var=True)
        ok = c.get_state()
        assert it == 3 and np.isfinite(d)
        c.debug_set(pkg.capi.DEBUG_EPI_SPIN_LIMIT, 2000)        # ~1 ms
        c.debug_set(pkg.capi.DEBUG_EPI_EXPECT_SKEW, 1)
        c.set_state(A0, B0, z, z, 0.1 * np.ones(H), 0.1 * np.ones(H), 0.1)
        with pytest.raises(pkg.VbmfError) as ei:
            c.run(3, eps=0.0, est_covs=True, est_var=True)
        assert ei.value.code == pkg.capi.VBMF_ERR_SYNC and "hand-off" in str(ei.value), ei.value
        c.debug_set(pkg.capi.DEBUG_EPI_EXPECT_SKEW, 0)
        c.debug_set(pkg.capi.DEBUG_EPI_SPIN_LIMIT, 1 << 22)
        c.set_state(A0, B0, z, z, 0.1 * np.ones(H), 0.1 * np.ones(H), 0.1)
        it, d2, _ = c.run(3, eps=0.0, est_covs=True, est_var=True)
        again = c.get_state()
        assert it == 3 and d2 == d and np.array_equal(again["BHat"], ok["BHat"])


def test_parity_asserts_catch_a_tenfold_regression(pkg):
    """The parity asserts are meant to fail on a 10x regression, not only on a broken kernel: scale the SigmaB / sigma2 table the
    B update multiplies by (vbmf_debug_set, VBMF_DEBUG_SIGMA_B_PPM) by 1 + 1e-4 -- ten times the ~1e-5 the three-sweep comparison
    measures on BHat -- and the same comparison that passes un-perturbed must raise, from the stated tolerance or from the
    measured-baseline guard of helpers.report()."""
    from tests import helpers
    from oracle import vbmf_oracle as O
    L, M, H = 777, 555, 64
    rng = np.random.default_rng(364)
    Y, _, _ = O.toy_matrix(L, M, 8, 0.05, rng)
    Yf = Y.astype(np.float32).astype(np.float64)
    p0 = O.vbmf_init(Yf, H, ca=0.1, cb=0.1, sigma2=0.1, rng=np.random.default_rng(365))
    A0, B0 = p0.AHat.copy(), p0.BHat.copy()
    z = np.zeros((H, H))
    O.vbmf_(Yf, p0, 3, eps=0.0, est_covs=True, est_var=True)

    def errs_of(ppm):
        with pkg.capi.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32) as c:
            c.set_Y(Yf)
            c.debug_set(pkg.capi.DEBUG_SIGMA_B_PPM, ppm)
            c.set_state(A0, B0, z, z, 0.1 * np.ones(H), 0.1 * np.ones(H), 0.1)
            c.run(3, eps=0.0, est_covs=True, est_var=True)
            s = c.get_state()
        return dict(BHat=helpers.relF(s["BHat"], p0.BHat), AHat=helpers.relF(s["AHat"], p0.AHat),
                    SigmaB=helpers.relF(s["SigmaB"], p0.SigmaB))

    clean = errs_of(0)
    helpers.report("soak 777x555 H64 f32 run3 clean: " + " ".join(f"{k}={v:.2e}" for k, v in clean.items()))
    assert clean["BHat"] < 1e-4 and clean["AHat"] < 5e-5, clean            # measured: BHat 3.1e-5, AHat 8.3e-6
    bad = errs_of(100)
    assert bad["BHat"] > 3 * max(clean["BHat"], 1e-5), (clean, bad)        # the perturbation is visible ...
    line = "f32 777x555 H64 run3: " + " ".join(f"{k}={v:.2e}" for k, v in bad.items())
    with pytest.raises(AssertionError):                                    # ... and the guard under every comparison catches it
        helpers.baseline_guard(line)
