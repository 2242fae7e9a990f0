"""vbls! over many bags with one fixed basis in one call (vbmf_run_fixed_basis_batched, vbls_batch_): the MIL classifier's loop
(examples/mil_util.jl:473-479) against the oracle's literal vbls! per bag, against the single-bag device path, and the C ABI's
refusals.  The bags sit side by side in one context; bag boundaries do not align with the 32-column tiles."""
import numpy as np
import pytest

import __graft_entry__ as G
from oracle import vbmf_oracle as O
from tests.helpers import compare, relF, report, to_pkg_params

pytestmark = pytest.mark.gpu

TOL = dict(default=3e-4, SigmaA=2e-3, sigma2=2e-3)          # test_gpu_vbls.py, test_vbls_hxh_loop_...
# test_gpu_vbls.py, test_vbls_basic_device_loop (bf16x2); SigmaA = sigma2 inv(K) carries sigma2's cancellation, as in TOL (measured
# 5.9e-4 on both at a 1-column bag)
TOL_BF16 = dict(default=4e-4, SigmaA=4e-3, sigma2=4e-3)


@pytest.fixture(scope="module")
def pkg():
    G.build()
    p = G.load_package()
    yield p
    p.set_defaults(y_dtype=p.VBMF_Y_F32, factor_dtype=p.VBMF_FACTOR_AUTO)


# 40 ragged bags: 1-column bags, bags that straddle the 32-column tile boundaries, up to 70 columns
RAGGED = [1, 31, 2, 70, 1, 1, 33, 29, 5, 64, 1, 17, 40, 3, 60, 1, 32, 31, 2, 45,
          7, 1, 66, 12, 30, 4, 1, 50, 9, 33, 1, 20, 6, 69, 2, 1, 15, 38, 11, 1]


def _model(L, H, seed, Mtrain=300):
    """A basis trained by the oracle (the classifier's res), and a sampler of bags in its row space."""
    rng = np.random.default_rng(seed)
    Bs = rng.standard_normal((L, H)) * np.linspace(1.0, 2.5, H)

    def draw(m):
        As = np.zeros((m, H)); As[np.arange(m), rng.integers(0, H, m)] = 1.0
        return Bs @ As.T + 0.05 * rng.standard_normal((L, m))
    Ytr = draw(Mtrain)
    po = O.vbmf_init(Ytr, H, ca=0.1, cb=0.1, sigma2=0.1, rng=np.random.default_rng(seed + 1), materialize_yhat=False)
    O.vbmf_(Ytr, po, 15, eps=0.0, est_covs=True, est_var=True)
    return po, draw


def _f32(Y):
    return Y.astype(np.float32).astype(np.float64)


def _pairs(pkg, Ys, po, seed):
    qo = [O.copy_vbmf_params(Y, po, rng=np.random.default_rng(seed + b)) for b, Y in enumerate(Ys)]
    qg = [pkg.copy_vbmf_params(Y, to_pkg_params(pkg, po), rng=np.random.default_rng(seed + b)) for b, Y in enumerate(Ys)]
    return qo, qg


def _worst(tag, qg, qo, tol, fields=("AHat", "SigmaA", "CA")):
    worst = {f: 0.0 for f in fields + ("sigma2",)}
    for g, o in zip(qg, qo):
        for f in fields:
            worst[f] = max(worst[f], relF(getattr(g, f), getattr(o, f)))
        worst["sigma2"] = max(worst["sigma2"], abs(g.sigma2 - o.sigma2) / abs(o.sigma2))
    report(f"{tag}: " + " ".join(f"{k}={v:.2e}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= tol.get(k, tol["default"])}
    assert not bad, (tag, bad)
    return worst


@pytest.mark.parametrize("H,niter", [(2, 150), (5, 150), (20, 40), (64, 12)])
def test_batch_against_the_oracle_and_the_single_bag_path(pkg, H, niter):
    L = 166
    pkg.set_defaults(y_dtype=pkg.VBMF_Y_F32, factor_dtype=pkg.VBMF_FACTOR_AUTO)
    po, draw = _model(L, H, 500 + H)
    Ys = [_f32(draw(m)) for m in RAGGED]
    qo, qg = _pairs(pkg, Ys, po, 40)
    for Y, q in zip(Ys, qo):
        O.vbls_(Y, q, niter)
    A = pkg.vbls_batch_(Ys, qg, niter)
    assert all(a is q.AHat for a, q in zip(A, qg))
    assert all(q.AHat.shape == (Y.shape[1], H) for Y, q in zip(Ys, qg))
    _worst(f"vbls_batch_ {len(Ys)} ragged bags H{H} x{niter}", qg, qo, TOL)
    for q in qg:
        assert np.allclose(q.invCA, np.linalg.inv(q.CA), rtol=1e-12)
        assert relF(q.YHat, q.BHat @ q.AHat.T) < 1e-14
    # the single-bag device path (vbmf_run_fixed_basis) on every bag
    _, q1 = _pairs(pkg, Ys, po, 40)
    worst = 0.0
    for Y, q in zip(Ys, q1):
        pkg.vbls_(Y, q, niter)
    for a, b in zip(qg, q1):
        worst = max(worst, relF(a.AHat, b.AHat))
    report(f"vbls_batch_ vs vbls_ per bag H{H} x{niter}: AHat={worst:.2e}")
    assert worst < 2e-5, worst
    pkg.invalidate()


def test_per_bag_start_values_and_segmentation(pkg):
    """Different sigma2 / CA starts per bag are honoured, and permuting the bags changes no bag's result."""
    L, H, niter = 166, 5, 60
    pkg.set_defaults(y_dtype=pkg.VBMF_Y_F32, factor_dtype=pkg.VBMF_FACTOR_AUTO)
    po, draw = _model(L, H, 71)
    Ys = [_f32(draw(m)) for m in RAGGED[:24]]
    rng = np.random.default_rng(9)
    s2 = rng.uniform(0.02, 0.5, len(Ys))
    cas = rng.uniform(0.05, 2.0, (len(Ys), H))

    def fresh(order):
        qo, qg = _pairs(pkg, [Ys[i] for i in order], po, 70)
        for k, i in enumerate(order):
            for q in (qo[k], qg[k]):
                q.sigma2 = float(s2[i]); q.CA = np.diag(cas[i]); q.invCA = np.diag(1.0 / cas[i])
        return qo, qg
    order = list(range(len(Ys)))
    qo, qg = fresh(order)
    for k in order:
        O.vbls_(Ys[k], qo[k], niter)
    pkg.vbls_batch_(Ys, qg, niter)
    _worst("vbls_batch_ per-bag start values H5 x60", qg, qo, TOL)
    perm = list(np.random.default_rng(4).permutation(len(Ys)))
    _, qp = fresh(perm)
    pkg.vbls_batch_([Ys[i] for i in perm], qp, niter)
    for k, i in enumerate(perm):
        a, b = qp[k], qg[i]
        assert relF(a.AHat, b.AHat) < 1e-6 and relF(a.SigmaA, b.SigmaA) < 1e-6 and relF(a.CA, b.CA) < 1e-6, i
        assert abs(a.sigma2 - b.sigma2) < 1e-6 * b.sigma2, i


def test_state_untouched_and_two_bases_on_one_upload(pkg):
    L, H, niter = 166, 4, 50
    pkg.set_defaults(y_dtype=pkg.VBMF_Y_F32, factor_dtype=pkg.VBMF_FACTOR_AUTO)
    po0, draw = _model(L, H, 81)
    po1, _ = _model(L, H, 82)
    Ys = [draw(m) for m in RAGGED[:16]]
    bags = pkg.Bags(Ys, H)
    ctx = bags.session.ctx
    # the context's own state is the same before and after a batched call
    g0 = to_pkg_params(pkg, po0)
    A0 = np.random.default_rng(5).standard_normal((bags.M, H))
    ctx.set_state(A0, g0.BHat, 0.01 * np.eye(H), g0.SigmaB, np.full(H, 0.7), np.diag(g0.CB), 0.3)
    before = ctx.get_state()
    ctx.run_fixed_basis_batched(bags.col_off, niter, np.full(len(Ys), 0.1), np.ones((len(Ys), H)))
    after = ctx.get_state()
    for k, v in before.items():
        assert np.array_equal(np.asarray(v), np.asarray(after[k])), k
    # res0 then res1 on one upload == two fresh runs
    runs = {}
    for tag, po in (("res0", po0), ("res1", po1)):
        _, qs = _pairs(pkg, Ys, po, 90)
        pkg.vbls_batch_(bags, qs, niter)
        _, qf = _pairs(pkg, Ys, po, 90)
        pkg.vbls_batch_(Ys, qf, niter)
        for a, b in zip(qs, qf):
            assert relF(a.AHat, b.AHat) < 1e-12 and relF(a.SigmaA, b.SigmaA) < 1e-12 and a.sigma2 == pytest.approx(b.sigma2, rel=1e-12)
        runs[tag] = qs
    assert relF(runs["res0"][0].AHat, runs["res1"][0].AHat) > 1e-3          # two bases, two answers
    bags.close()


def test_bf16_storage(pkg):
    L, H, niter = 166, 6, 20
    try:
        pkg.set_defaults(y_dtype=pkg.VBMF_Y_BF16, factor_dtype=pkg.VBMF_FACTOR_AUTO)
        po, draw = _model(L, H, 91)
        Ys = [draw(m) for m in RAGGED[:20]]
        bags = pkg.Bags(Ys, H)
        Yst = bags.session.ctx.get_Y()                        # the bags exactly as the device stores them
        Yss = [np.ascontiguousarray(Yst[:, c0:c1]) for c0, c1 in zip(bags.col_off[:-1], bags.col_off[1:])]
        qo, qg = _pairs(pkg, Yss, po, 30)
        for Y, q in zip(Yss, qo):
            O.vbls_(Y, q, niter)
        pkg.vbls_batch_(bags, qg, niter)
        _worst(f"vbls_batch_ bf16 storage H{H} x{niter}", qg, qo, TOL_BF16)
        bags.close()
    finally:
        pkg.set_defaults(y_dtype=pkg.VBMF_Y_F32, factor_dtype=pkg.VBMF_FACTOR_AUTO)


def test_many_bags_in_one_call(pkg):
    L, H, niter, nb = 166, 5, 150, 4096
    pkg.set_defaults(y_dtype=pkg.VBMF_Y_F32, factor_dtype=pkg.VBMF_FACTOR_AUTO)
    po, draw = _model(L, H, 101)
    Ms = np.random.default_rng(11).integers(1, 41, nb)
    Ys = [_f32(draw(int(m))) for m in Ms]
    qo, qg = _pairs(pkg, Ys, po, 5000)
    pkg.vbls_batch_(Ys, qg, niter)
    sample = sorted(set(np.random.default_rng(12).choice(nb, 24, replace=False).tolist()) | {0, nb - 1})
    for b in sample:
        O.vbls_(Ys[b], qo[b], niter)
    _worst(f"vbls_batch_ {nb} bags H{H} x{niter} (sample)", [qg[b] for b in sample], [qo[b] for b in sample], TOL)
    compare(f"vbls_batch_ {nb} bags H{H} x{niter}, last bag", qg[-1], qo[-1], TOL, fields=("AHat", "SigmaA", "CA"))
    assert all(np.isfinite(q.AHat).all() and q.sigma2 > 0 for q in qg)


def test_refusals_launch_nothing(pkg):
    VI = pkg.capi.VBMF_ERR_INVALID
    L, M, H = 64, 40, 4
    rng = np.random.default_rng(13)
    Y = rng.standard_normal((L, M))
    B = rng.standard_normal((L, H))
    off = np.array([0, 1, 17, 33, M], dtype=np.int64)
    nb = off.size - 1

    def refused(c, o=off, niter=10, h=H):
        n = len(o) - 1
        with pytest.raises(pkg.VbmfError) as e:
            c.run_fixed_basis_batched(o, niter, np.full(n, 0.1), np.ones((n, h)))
        assert e.value.code == VI, e.value
        return str(e.value)

    with pkg.capi.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32) as c:
        c.set_Y(Y)
        c.set_state(np.zeros((M, H)), B, np.zeros((H, H)), 0.01 * np.eye(H), np.ones(H), np.ones(H), 0.1)
        c.run_fixed_basis_batched(off, 10, np.full(nb, 0.1), np.ones((nb, H)))
        words = c.dims()["Hp"] * c.dims()["XT1"] * 32
        P0, s0 = c.peek(pkg.capi.PEEK_P, words), c.get_state()
        refused(c, niter=0)
        for bad in ([0, 1, 1, M], [1, 17, M], [0, 17, M - 1], [0, 20, 10, M], [0, M + 1]):
            refused(c, np.array(bad, dtype=np.int64))
        c.set_state(np.zeros((M, H)), B, np.zeros((H, H)), 0.01 * np.eye(H), np.ones(H), np.ones(H), 0.1, labels0=[0, 5], H1=1)
        assert "mask" in refused(c)
        assert np.array_equal(c.peek(pkg.capi.PEEK_P, words), P0)          # nothing ran
        c.set_state(np.zeros((M, H)), B, np.zeros((H, H)), 0.01 * np.eye(H), np.ones(H), np.ones(H), 0.1)
        after = c.get_state()
        for k in ("BHat", "SigmaB", "CB_diag"):
            assert np.array_equal(after[k], s0[k]), k
        # a non-finite pivot in one bag: VBMF_ERR_NUMERIC; the next call is clean
        s2 = np.full(nb, 0.1); s2[2] = np.nan
        with pytest.raises(pkg.VbmfError) as e:
            c.run_fixed_basis_batched(off, 10, s2, np.ones((nb, H)))
        assert e.value.code == pkg.capi.VBMF_ERR_NUMERIC
        r = c.run_fixed_basis_batched(off, 10, np.full(nb, 0.1), np.ones((nb, H)))
        assert np.isfinite(r["AHat"]).all()
    with pkg.capi.Context(L, M, 65, y_dtype=pkg.VBMF_Y_F32) as c:
        assert "64" in refused(c, h=65)
    with pkg.capi.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32, variant=pkg.capi.VBMF_VARIANT_SPARSE_DIAG) as c:
        assert "sparse" in refused(c)
    with pkg.capi.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32, nranks=2, rank=0, L_global=2 * L) as c:
        assert "rank" in refused(c)
