"""Parity at BASELINE.json's FULL sizes: config 3 (100 000 x 10 000, H = 64, bf16 Y), config 4
(1M x 10k, H = 128: one rank's 125 000-row share against the oracle, the whole matrix through its properties) and
config 5 (ARD-sparse, H = 256) against the fp64 oracle fed the matrix exactly as the device stores it
(`vbmf_get_Y`), plus size-independent properties of the sweep.  The oracle needs the 8 GB fp64 Y on the host and
~0.3-1 TFLOP of fp64 BLAS per sweep, so the trajectories are short (3 resp. 2 sweeps).  Tolerances as in
tests/test_gpu_parity.py (bf16x2 path: 1e-4, sigma2 1e-3).  PARITY UNPINNED beyond the oracle: the reference holds
no recorded run at these sizes."""
import gc

import numpy as np
import pytest

import __graft_entry__ as G
from oracle import vbmf_oracle as O
from tests.helpers import relF, report

pytestmark = pytest.mark.gpu

L, M = 100000, 10000


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


def _oracle_params(A0, B0, H):
    po = O.vbmf_parameters()
    po.L, po.M, po.H = L, M, H
    po.AHat, po.BHat = A0.copy(), B0.copy()
    po.SigmaA = np.zeros((H, H)); po.SigmaB = np.zeros((H, H))
    po.CA = 0.1 * np.eye(H); po.CB = 0.1 * np.eye(H); po.invCA = 10 * np.eye(H); po.invCB = 10 * np.eye(H)
    po.sigma2 = 0.1
    return po


def test_config3_full_size_three_sweeps(pkg):
    """Headline configuration, exactly as bench.py runs it (same seeds, generator, initial state)."""
    H = 64
    rng = np.random.default_rng(20170102)
    A0, B0 = rng.standard_normal((M, H)), rng.standard_normal((L, H))
    z = np.zeros((H, H))
    with pkg.capi.Context(L, M, H, y_dtype=pkg.VBMF_Y_BF16) as c:
        c.set_Y_synthetic(20170101, H, 0.05)
        c.set_state(A0, B0, z, z, 0.1 * np.ones(H), 0.1 * np.ones(H), 0.1)
        it, d, tr = c.run(3, eps=0.0, est_covs=True, est_var=True, want_trace=True)
        s = c.get_state()
        trYY = c.trYY()
        # size-independent properties on the device alone
        # (1) determinism: the same three sweeps again, bit for bit (fixed-order reductions, no atomics)
        c.set_state(A0, B0, z, z, 0.1 * np.ones(H), 0.1 * np.ones(H), 0.1)
        it2, d2, tr2 = c.run(3, eps=0.0, est_covs=True, est_var=True, want_trace=True)
        s2 = c.get_state()
        assert it2 == 3 and d2 == d and np.array_equal(tr2[:, :3], tr[:, :3])
        assert np.array_equal(s2["AHat"], s["AHat"]) and np.array_equal(s2["BHat"], s["BHat"])
        # (2) with the hyper-parameters frozen (est_covs = est_var = false) coordinate ascent cannot lower the bound
        #     (from the initial state, where the steps are large against the fp32 noise of the residual term)
        c.set_state(A0, B0, z, z, 0.1 * np.ones(H), 0.1 * np.ones(H), 0.1)
        it3, d3, tr3 = c.run(6, eps=0.0, est_covs=False, est_var=False, want_trace=True)
        e = tr3[:, 2]
        report("cfg3 FULL SIZE frozen-hyperparameter ELBO trace: " + " ".join(f"{v:.6e}" for v in e))
        assert it3 == 6 and np.all(np.isfinite(e)) and np.all(np.diff(e) >= -1e-5 * np.abs(e[:-1])), e
        Ys = c.get_Y()
    assert it == 3
    assert abs(float(np.vdot(Ys, Ys)) - trYY) <= 1e-12 * trYY
    po = _oracle_params(A0, B0, H)
    otr = []
    O.vbmf_(Ys, po, 3, eps=0.0, est_covs=True, est_var=True, fused=True, trace=otr)
    del Ys
    gc.collect()
    errs = dict(A=relF(s["AHat"], po.AHat), B=relF(s["BHat"], po.BHat), SA=relF(s["SigmaA"], po.SigmaA),
                SB=relF(s["SigmaB"], po.SigmaB), ca=relF(s["CA_diag"], np.diag(po.CA)),
                cb=relF(s["CB_diag"], np.diag(po.CB)), s2=abs(s["sigma2"] - po.sigma2) / po.sigma2,
                d=abs(d - otr[-1][0]) / otr[-1][0], elbo=abs(tr[-1, 2] - otr[-1][2]) / abs(otr[-1][2]))
    report("cfg3 FULL SIZE 100000x10000 H=64 bf16x2, 3 sweeps: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    # measured (round 3): worst factor / covariance / ARD field 2.4e-5 (SA), s2 5.9e-6, d 4.1e-5, elbo 1.9e-6
    assert max(errs[k] for k in ("A", "B", "SA", "SB", "ca", "cb")) < 7.5e-5, errs
    assert errs["s2"] < 1.8e-5 and errs["d"] < 1.3e-4 and errs["elbo"] < 6e-6, errs


def test_config5_full_size_sparse_two_sweeps(pkg):
    """ARD-sparse diagonal branch at config 5's size (H = 256), bench.py's initial state, 2 sweeps + lowerBound."""
    H = 256
    rng = np.random.default_rng(20170102)
    A0, B0 = rng.standard_normal((M, H)), rng.standard_normal((L, H))
    hyper = dict(alpha0=1e-10, beta0=1e-10, gamma0=1e-10, delta0=1e-10, eta0=1e-10, zeta0=1e-10)
    with pkg.capi.Context(L, M, H, y_dtype=pkg.VBMF_Y_BF16, variant=pkg.capi.VBMF_VARIANT_SPARSE_DIAG) as c:
        c.set_Y_synthetic(20170101, H, 0.05)
        c.sparse_set_state(A0.reshape(M * H), np.ones(M * H), 0.1 * np.ones(M * H), 1e-10 * np.ones(M * H), B0,
                           np.zeros((H, H)), 0.1 * np.ones(H), 1e-10 * np.ones(H), 0.1, 1e-10, hyper)
        it, d, _ = c.sparse_run(2, eps=0.0, est_cb=True)
        s = c.sparse_get_state()
        lb = c.sparse_lower_bound()
        Ys = c.get_Y()
    assert it == 2
    po = O.vbmf_sparse_parameters()
    po.L, po.M, po.H, po.MH, po.H1 = L, M, H, M * H, 0
    po.labels = np.zeros(0, dtype=np.int64)
    po.AHat = A0.copy(); po.ATVecHat = A0.reshape(M * H).copy()
    po.SigmaATVec = po.invSigmaATVec = None
    po.diagSigmaATVec = np.ones(M * H); po.SigmaA = np.zeros((H, H))
    po.BHat = B0.copy(); po.SigmaB = np.zeros((H, H))
    po.CA = 0.1 * np.ones(M * H); po.beta = 1e-10 * np.ones(M * H)
    po.CB = 0.1 * np.ones(H); po.delta = 1e-10 * np.ones(H)
    po.alpha0 = po.beta0 = po.gamma0 = po.delta0 = po.eta0 = po.zeta0 = 1e-10
    po.alpha = 1e-10 + 0.5; po.gamma = 1e-10 + L / 2; po.eta = 1e-10 + L * M / 2
    po.sigmaHat, po.zeta = 0.1, 1e-10
    po.YHat = None
    po.trYTY = float(np.vdot(Ys, Ys))
    d_ref, n = O.vbmf_sparse_(Ys, po, 2, eps=0.0, full_cov=False, est_cb=True)
    lb_ref = O.lowerBound(Ys, po)
    del Ys
    gc.collect()
    errs = {k: relF(s[k], getattr(po, k)) for k in ("ATVecHat", "diagSigmaATVec", "CA", "beta", "BHat", "SigmaB", "CB", "delta")}
    errs["SigmaA"] = relF(s["SigmaA_diag"], np.diag(po.SigmaA))
    errs["sigmaHat"] = abs(s["sigmaHat"] - po.sigmaHat) / po.sigmaHat
    errs["d"] = abs(d - d_ref) / d_ref
    errs["lowerBound"] = abs(lb - lb_ref) / abs(lb_ref)
    report("cfg5 FULL SIZE sparse 100000x10000 H=256 bf16x2, 2 sweeps: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert n == 2
    # measured (round 3): worst field 1.3e-5 (CA), sigmaHat 2.9e-8, d 5.6e-4, lowerBound 1.3e-8
    assert max(v for k, v in errs.items() if k not in ("sigmaHat", "d", "lowerBound")) < 4e-5, errs
    assert errs["sigmaHat"] < 1e-6 and errs["d"] < 1.7e-3 and errs["lowerBound"] < 1e-6, errs


# ---- BASELINE config 4: 1M x 10k, H = 128, Y row-sharded over 8 GPUs ---------------------------------------------------------
L4, M4, H4, SHARDS4 = 1000000, 10000, 128, 8


def test_config4_rank_share_vs_oracle(pkg):
    """One rank's share of config 4 at its REAL size: 125 000 x 10 000, H = 128, bf16 Y, the collective code path
    (1-rank RCCL communicator: slab sum, out-of-place all-reduces of Y'B and of [B'B | dB'dB | tr(B'YA)]), two sweeps against
    the fused fp64 oracle on the matrix exactly as the device stores it (10 GB on the host, ~0.6 TFLOP per sweep).
    Tolerances: config 3's (bf16x2 path)."""
    Ls, H = L4 // SHARDS4, H4
    rng = np.random.default_rng(20170102)
    A0, B0 = rng.standard_normal((M4, H)), rng.standard_normal((Ls, H))
    z = np.zeros((H, H))
    with pkg.capi.Context(Ls, M4, H, y_dtype=pkg.VBMF_Y_BF16, nranks=1, rank=0, L_global=Ls, row_offset=0) as c:
        c.comm_init(pkg.capi.Context.unique_id())
        c.set_Y_synthetic(20170101, H, 0.05)
        c.set_state(A0, B0, z, z, 0.1 * np.ones(H), 0.1 * np.ones(H), 0.1)
        it, d, tr = c.run(2, eps=0.0, est_covs=True, est_var=True, want_trace=True)
        s = c.get_state()
        trYY = c.trYY()
        dims = c.dims()
        Ys = c.get_Y()
    assert it == 2 and dims["NH"] == 4
    assert abs(float(np.vdot(Ys, Ys)) - trYY) <= 1e-12 * trYY
    po = O.vbmf_parameters()
    po.L, po.M, po.H = Ls, M4, H
    po.AHat, po.BHat = A0.copy(), B0.copy()
    po.SigmaA = np.zeros((H, H)); po.SigmaB = np.zeros((H, H))
    po.CA = 0.1 * np.eye(H); po.CB = 0.1 * np.eye(H); po.invCA = 10 * np.eye(H); po.invCB = 10 * np.eye(H)
    po.sigma2 = 0.1
    otr = []
    O.vbmf_(Ys, po, 2, eps=0.0, est_covs=True, est_var=True, fused=True, trace=otr)
    del Ys
    gc.collect()
    errs = dict(A=relF(s["AHat"], po.AHat), B=relF(s["BHat"], po.BHat), SA=relF(s["SigmaA"], po.SigmaA),
                SB=relF(s["SigmaB"], po.SigmaB), ca=relF(s["CA_diag"], np.diag(po.CA)),
                cb=relF(s["CB_diag"], np.diag(po.CB)), s2=abs(s["sigma2"] - po.sigma2) / po.sigma2,
                d=abs(d - otr[-1][0]) / otr[-1][0], elbo=abs(tr[-1, 2] - otr[-1][2]) / abs(otr[-1][2]))
    report(f"cfg4 RANK SHARE {Ls}x{M4} H={H} bf16x2 (1 of {SHARDS4} shards of 1M x 10k, collective path), 2 sweeps: "
           + " ".join(f"{k}={v:.2e}" for k, v in errs.items()) + f"  [plan: pass1 nsplit {dims['nsplit1']}, pass2 nsplit {dims['nsplit2']}]")
    # measured (round 3): worst field 1.8e-5 (SB), s2 5.2e-6, d 2.0e-6, elbo 1.1e-5
    assert max(errs[k] for k in ("A", "B", "SA", "SB", "ca", "cb")) < 5.5e-5, errs
    assert errs["s2"] < 1.6e-5 and errs["d"] < 1e-5 and errs["elbo"] < 3.3e-5, errs


def test_config4_whole_matrix_properties(pkg):
    """The whole 1M x 10k matrix of config 4 on ONE GPU (two tiled bf16 copies, 40 GB), H = 128: no host copy of it can
    exist (80 GB fp64), so the checks are the size-independent properties used at config 3 -- bit-determinism, ascent of
    the bound with frozen hyper-parameters, ||Y||^2 -- plus the generator's independence of the sharding at this scale:
    a 4096-row window of the 1M-row matrix equals, bit for bit, the same window generated as its own shard."""
    H = H4
    rng = np.random.default_rng(20170102)
    A0 = rng.standard_normal((M4, H))
    B0 = rng.standard_normal((L4, H))
    z = np.zeros((H, H))
    ones = 0.1 * np.ones(H)
    win0, wn = 531072, 4096
    with pkg.capi.Context(L4, M4, H, y_dtype=pkg.VBMF_Y_BF16) as c:
        c.set_Y_synthetic(20170101, H, 0.05)
        trYY = c.trYY()
        window = c.get_Y(win0, wn)
        c.set_state(A0, B0, z, z, ones, ones, 0.1)
        it, d, tr = c.run(2, eps=0.0, est_covs=True, est_var=True, want_trace=True)
        s = c.get_state(want_B=False)
        c.set_state(A0, B0, z, z, ones, ones, 0.1)
        it2, d2, tr2 = c.run(2, eps=0.0, est_covs=True, est_var=True, want_trace=True)
        s2 = c.get_state(want_B=False)
        assert it == it2 == 2 and d2 == d and np.array_equal(tr2[:, :3], tr[:, :3])
        assert np.array_equal(s2["AHat"], s["AHat"]) and np.array_equal(s2["SigmaB"], s["SigmaB"]) and s2["sigma2"] == s["sigma2"]
        c.set_state(A0, B0, z, z, ones, ones, 0.1)
        it3, d3, tr3 = c.run(4, eps=0.0, est_covs=False, est_var=False, want_trace=True)
        e = tr3[:, 2]
    report(f"cfg4 WHOLE MATRIX {L4}x{M4} H={H}: trYY/(LM) = {trYY / (L4 * M4):.6f}; sigma2 after 2 sweeps {s['sigma2']:.6e}; "
           "frozen-hyperparameter ELBO trace " + " ".join(f"{v:.6e}" for v in e))
    assert it3 == 4 and np.all(np.isfinite(e)) and np.all(np.diff(e) >= -1e-5 * np.abs(e[:-1])), e
    # toy_matrix entries are N(0,1) (one latent column per matrix column) + N(0, 0.05^2): second moment 1.0025 (1e10 samples)
    assert abs(trYY / (L4 * M4) - 1.0025) < 2e-3, trYY / (L4 * M4)
    assert np.isfinite(s["sigma2"]) and s["sigma2"] > 0
    with pkg.capi.Context(wn, M4, H, y_dtype=pkg.VBMF_Y_BF16, nranks=1, rank=0, L_global=wn, row_offset=win0) as c:
        c.set_Y_synthetic(20170101, H, 0.05)
        shard = c.get_Y()
    assert np.array_equal(shard, window)


def test_config4_share_gram_form_vs_oracle(pkg, monkeypatch):
    """Config 4's rank-share size (125 000 x 10 000, H = 128) on a plain whole-matrix context, which takes the Gram form by the
    size rule (no comm_init: test_config4_rank_share_vs_oracle's collective context runs the streaming path).  Separated data
    as in tests/test_gpu_gram_path.py's _problem (each column one latent column of scale 1 .. 3, noise 0.05), so the VB fixed
    point is well conditioned and a ten-sweep trajectory is a meaningful target.  Against the fused fp64 oracle on the stored Y,
    and against the streaming path (VBMF_GRAM=0) on the same stored Y; bounds: the 25-sweep trajectory bounds of
    test_run_trajectory_well_conditioned (factors 4e-5, SigmaA / SigmaB / sigma2 1.6e-4, d rtol 8e-3, ELBO rtol 4e-4)."""
    Ls, H, noise, n = L4 // SHARDS4, H4, 0.05, 10
    rng = np.random.default_rng(20170105)
    Bt = rng.standard_normal((Ls, H)) * np.linspace(1.0, 3.0, H)
    col = rng.integers(0, H, size=M4)
    Y = np.empty((Ls, M4), order="F")
    for j0 in range(0, M4, 500):
        j1 = min(j0 + 500, M4)
        Y[:, j0:j1] = Bt[:, col[j0:j1]] + noise * rng.standard_normal((Ls, j1 - j0))
    del Bt
    po = O.vbmf_init(np.broadcast_to(0.0, (Ls, M4)), H, ca=0.1, cb=0.1, sigma2=0.1, rng=np.random.default_rng(20170106),
                     materialize_yhat=False)
    z = np.zeros((H, H))

    def go(c):
        c.set_state(po.AHat, po.BHat, z, z, 0.1 * np.ones(H), 0.1 * np.ones(H), 0.1)
        it, d, tr = c.run(n, eps=0.0, est_covs=True, est_var=True, want_trace=True)
        assert it == n
        return d, tr.copy(), c.get_state(want_B=True)

    monkeypatch.delenv("VBMF_GRAM", raising=False)
    with pkg.capi.Context(Ls, M4, H, y_dtype=pkg.VBMF_Y_BF16) as c:
        dims = c.dims()
        assert dims["gram"] == 1 and dims["NH"] == 4
        c.set_Y(Y)
        del Y
        gc.collect()
        dg, trg, sg = go(c)
        nsplit = c.dims()["gram_nsplit"]
        Ys = c.get_Y()
    monkeypatch.setenv("VBMF_GRAM", "0")
    with pkg.capi.Context(Ls, M4, H, y_dtype=pkg.VBMF_Y_BF16) as c:
        monkeypatch.delenv("VBMF_GRAM")
        assert c.dims()["gram"] == 0
        c.set_Y(Ys)
        ds, trs, ss = go(c)
    otr = []
    O.vbmf_(Ys, po, n, eps=0.0, est_covs=True, est_var=True, fused=True, trace=otr)
    del Ys
    gc.collect()
    otr = np.array(otr)

    def errs(s, d, tr):
        return dict(A=relF(s["AHat"], po.AHat), B=relF(s["BHat"], po.BHat), SA=relF(s["SigmaA"], po.SigmaA),
                    SB=relF(s["SigmaB"], po.SigmaB), ca=relF(s["CA_diag"], np.diag(po.CA)), cb=relF(s["CB_diag"], np.diag(po.CB)),
                    s2=abs(s["sigma2"] - po.sigma2) / po.sigma2, d=abs(d - otr[-1, 0]) / otr[-1, 0],
                    elbo=abs(tr[-1, 2] - otr[-1, 2]) / abs(otr[-1, 2]),
                    d_tr=float(np.max(np.abs(tr[:, 0] - otr[:, 0]) / (1e-5 + 8e-3 * otr[:, 0]))),
                    s2_tr=float(np.max(np.abs(tr[:, 1] - otr[:, 1]) / otr[:, 1])),
                    elbo_tr=float(np.max(np.abs(tr[:, 2] - otr[:, 2]) / (1.0 + 4e-4 * np.abs(otr[:, 2])))))
    eg, es = errs(sg, dg, trg), errs(ss, ds, trs)
    gs = dict(A=relF(sg["AHat"], ss["AHat"]), B=relF(sg["BHat"], ss["BHat"]), SB=relF(sg["SigmaB"], ss["SigmaB"]),
              s2=abs(sg["sigma2"] - ss["sigma2"]) / ss["sigma2"])
    within = np.abs(otr[:, 1] - noise ** 2) <= 0.1 * noise ** 2
    reach = int(np.argmax(within)) + 1 if within.any() else -1
    tail = f"  [gram_nsplit {nsplit}; oracle sigma2 {otr[-1, 1]:.7e} (noise^2 {noise ** 2:.1e}), within 10 % from sweep {reach}]"
    report(f"cfg4 SHARE GRAM FORM {Ls}x{M4} H={H} separated, {n} sweeps, gram vs oracle: "
           + " ".join(f"{k}={v:.2e}" for k, v in eg.items()) + tail)
    report(f"cfg4 SHARE STREAMING {Ls}x{M4} H={H} separated, {n} sweeps, streaming vs oracle: "
           + " ".join(f"{k}={v:.2e}" for k, v in es.items()))
    report(f"cfg4 SHARE GRAM vs STREAMING {Ls}x{M4} H={H} separated, {n} sweeps: " + " ".join(f"{k}={v:.2e}" for k, v in gs.items())
           + f"  [sigma2 gram {sg['sigma2']:.7e} streaming {ss['sigma2']:.7e}]")
    assert 0 < reach <= n, (reach, otr[:, 1])
    assert max(eg[k] for k in ("A", "B", "ca", "cb")) < 4e-5, eg
    assert max(eg[k] for k in ("SA", "SB", "s2", "s2_tr")) < 1.6e-4, eg
    assert eg["d_tr"] <= 1.0 and eg["elbo_tr"] <= 1.0, eg
