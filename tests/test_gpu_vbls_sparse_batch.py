"""vbls! of the ARD-sparse models over many bags with one fixed basis in one call (vbmf_sparse_run_fixed_basis_batched,
vbls_sparse_batch_): the MIL classifiers' loops (examples/mil_util.jl:393-416, :469-479, :497-521) in both updateA! forms, against
the oracle's literal vbls! per bag, against the single-bag device path, and the C ABI's refusals.  The bags sit side by side in one
context; bag boundaries do not align with the 32-column tiles."""
import copy
import dataclasses

import numpy as np
import pytest

import __graft_entry__ as G
from oracle import vbmf_oracle as O
from tests.helpers import relF, report

pytestmark = pytest.mark.gpu

FIELDS = ("ATVecHat", "diagSigmaATVec", "CA", "beta", "SigmaA", "sigmaHat", "zeta")


def _tol(ATVecHat, dS, CA, beta, sigma):
    """bounds by field, the grouped models' views under the field they are cut from; sigmaHat, zeta, SigmaA and diagSigmaATVec move
    together (SigmaA = sum_m dS_m; every dS_m carries sigmaHat's error, whose zeta = zeta0 + ||Y||^2/2 - sum P o A + ... cancels)"""
    t = dict(ATVecHat=ATVecHat, diagSigmaATVec=dS, SigmaA=dS, sigmaHat=sigma, zeta=sigma, CA=CA, beta=beta)
    for g in ("0", "1", "2"):
        t["CA" + g], t["beta" + g], t[f"A{g}Hat"] = CA, beta, ATVecHat
    t["A1Hat"] = t["A2Hat"] = ATVecHat
    return t


# about 3 x the largest error measured on an MI355X over this file's cases (the diagonal / full_cov form; f32 storage unless named)
TOL = {False: _tol(2e-6, 4e-4, 2e-5, 4e-6, 4e-4),            # measured 5.5e-7, 1.2e-4 (H = 2), 7.0e-6 (QS1 off), 1.2e-6, 1.2e-4
       True: _tol(5e-6, 1.6e-3, 2e-3, 7e-6, 1.6e-3)}           # 1.4e-6, 5.2e-4, 6.6e-4, 2.3e-6, 5.3e-4 (4096 bags, sampled)
TOL_BF16 = {False: _tol(4e-6, 1.1e-5, 9e-5, 5e-6, 1.1e-5),    # 1.2e-6, 3.6e-6, 3.0e-5, 1.7e-6, 3.5e-6
            True: _tol(4e-6, 5e-4, 1.1e-3, 5e-6, 5e-4)}        # 1.2e-6, 1.5e-4, 3.6e-4, 1.5e-6, 1.5e-4
# against the single-bag device path (fp32 per-column state there)
TOL_DEV = {False: _tol(1.6e-6, 8e-5, 1.4e-6, 2.5e-7, 8e-5),  # 5.2e-7 (H = 64), 2.6e-5 (H = 2), 4.5e-7, 7.5e-8, 2.6e-5
           True: _tol(1.6e-7, 7e-5, 1e-5, 3.5e-7, 7e-5)}       # 5.3e-8, 2.3e-5 (H = 3), 3.2e-6, 1.1e-7, 2.3e-5


@pytest.fixture(scope="module")
def pkg():
    G.build()
    p = G.load_package()
    yield p
    p.set_defaults(y_dtype=p.VBMF_Y_F32, factor_dtype=p.VBMF_FACTOR_AUTO)


# 40 ragged bags: 1-column bags, bags that straddle the 32-column tile boundaries, up to 70 columns
RAGGED = [1, 31, 2, 70, 1, 1, 33, 29, 5, 64, 1, 17, 40, 3, 60, 1, 32, 31, 2, 45,
          7, 1, 66, 12, 30, 4, 1, 50, 9, 33, 1, 20, 6, 69, 2, 1, 15, 38, 11, 1]
# full_cov: the oracle inverts the dense M_b H x M_b H matrix, so the bags stay small
SMALL = [1, 3, 2, 7, 1, 5, 4, 1, 6, 2, 8, 3]


def _f32(Y):
    return Y.astype(np.float32).astype(np.float64)


def _model(kind, L, H, seed, Mtrain=200, niter=12):
    """A basis trained by the oracle (the classifier's res), and a sampler of bags in its row space."""
    rng = np.random.default_rng(seed)
    Bs = rng.standard_normal((L, H)) * np.linspace(1.0, 2.5, H)

    def draw(m):
        As = np.zeros((m, H)); As[np.arange(m), rng.integers(0, H, m)] = 1.0
        return Bs @ As.T + 0.05 * rng.standard_normal((L, m))
    Ytr = draw(Mtrain)
    r = np.random.default_rng(seed + 1)
    if kind == "sparse":
        po = O.vbmf_sparse_init(Ytr, H, rng=r, full_cov=False, materialize_yhat=False)
        O.vbmf_sparse_(Ytr, po, niter, eps=0.0)
    elif kind == "dual":
        po = O.vbmf_dual_init(Ytr, H, max(1, H // 2), rng=r, materialize_yhat=False)
        O.vbmf_dual_(Ytr, po, niter, eps=0.0, est_priors=False)
    else:
        po = O.vbmf_trial_init(Ytr, H, max(1, H // 2), Mtrain // 2, rng=r, materialize_yhat=False)
        O.vbmf_trial_(Ytr, po, niter, eps=0.0, est_priors=False)
    return po, draw


def _convert(cls, src):
    """field-by-field deep copy between the oracle's and the package's parameter types (same field names)"""
    dst = cls()
    for f in dataclasses.fields(cls):
        if hasattr(src, f.name):
            setattr(dst, f.name, copy.deepcopy(getattr(src, f.name)))
    return dst


def _pkg_type(pkg, po):
    for name in ("vbmf_trial_parameters", "vbmf_dual_parameters", "vbmf_sparse_parameters"):
        if isinstance(po, getattr(O, name)):
            return getattr(pkg, name), getattr(O, name)


def _sets(pkg, Ys, po, seed, which=0):
    """per bag: the package's copy_vbmf_params (which = the trial model's first or second set) and its oracle twin"""
    P, Oc = _pkg_type(pkg, po)
    res = _convert(P, po)
    qg = []
    for b, Y in enumerate(Ys):
        q = pkg.copy_vbmf_params(Y, res, rng=np.random.default_rng(seed + b))
        qg.append(q[which] if isinstance(q, tuple) else q)
    return qg, [_convert(Oc, q) for q in qg]


def _clone(qs):
    return [copy.deepcopy(q) for q in qs]


def _oracle_full(Y, q, niter, kind):
    """the oracle's literal full_cov loop: updateA!(full_cov = true), updateCA!, updateSigma! (src/vbmf_sparse.jl:178-202, 284-288,
    317-321; src/vbmf_dual.jl:218-243, 322-351)"""
    for _ in range(niter):
        if kind == "dual":
            O.dual_updateA(Y, q, full_cov=True)
            O.dual_updateCA(q)
        else:
            O.sparse_updateA(Y, q, full_cov=True)
            O.sparse_updateCA(q)
        O.sparse_updateSigma(Y, q)


def _errs(g, o, fields=FIELDS):
    e = {}
    for f in fields:
        a, b = getattr(g, f), getattr(o, f)
        e[f] = abs(a - b) / abs(b) if np.isscalar(b) else relF(a, b)
    return e


def _worst(tag, qg, qo, tol, fields=FIELDS):
    worst = {f: 0.0 for f in fields}
    for g, o in zip(qg, qo):
        for k, v in _errs(g, o, fields).items():
            worst[k] = max(worst[k], v)
    report(f"{tag}: " + " ".join(f"{k}={v:.2e}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= tol[k]}
    assert not bad, (tag, bad)
    return worst


def _single_bag(pkg, Ys, qs, niter, full_cov, tag, skip_one_column=False):
    """the single-bag device path (vbmf_sparse_run_fixed_basis) on every bag it takes"""
    worst = {f: 0.0 for f in FIELDS}
    for Y, q in zip(Ys, qs):
        if skip_one_column and Y.shape[1] < 2:
            continue
        q1 = copy.deepcopy(q)
        # the start values of the batched call, not what it left
        q1.CA, q1.sigmaHat = q._start_CA.copy(), q._start_sigma
        pkg.vbls_(Y, q1, niter, full_cov=full_cov)
        for k, v in _errs(q, q1).items():
            worst[k] = max(worst[k], v)
    pkg.invalidate()
    report(f"{tag}: " + " ".join(f"{k}={v:.2e}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= TOL_DEV[full_cov][k]}
    assert not bad, (tag, bad)


def _mark_starts(qs):
    for q in qs:
        q._start_CA, q._start_sigma = np.array(q.CA, copy=True), q.sigmaHat


@pytest.mark.parametrize("H,niter", [(2, 150), (5, 150), (20, 40), (64, 12)])
def test_sparse_diagonal_ragged(pkg, H, niter):
    L = 166
    pkg.set_defaults(y_dtype=pkg.VBMF_Y_F32, factor_dtype=pkg.VBMF_FACTOR_AUTO)
    po, draw = _model("sparse", L, H, 600 + H)
    Ys = [_f32(draw(m)) for m in RAGGED]
    qg, qo = _sets(pkg, Ys, po, 40)
    _mark_starts(qg)
    for Y, q in zip(Ys, qo):
        O.vbls_sparse_(Y, q, niter)
    A = pkg.vbls_sparse_batch_(Ys, qg, niter)
    assert all(a is q.AHat for a, q in zip(A, qg))
    assert all(q.AHat.shape == (Y.shape[1], H) and np.array_equal(q.AHat.reshape(-1), q.ATVecHat) for Y, q in zip(Ys, qg))
    assert all(relF(q.YHat, q.BHat @ q.AHat.T) < 1e-14 for q in qg)
    _worst(f"vbls_sparse_batch_ diag {len(Ys)} ragged bags H{H} x{niter}", qg, qo, TOL[False])
    # the single-bag path refuses M = 1 under the QS1 layout: the rest
    _single_bag(pkg, Ys, qg, niter, False, f"vbls_sparse_batch_ diag vs vbls_ per bag H{H} x{niter}", skip_one_column=True)


# (20, 50-column bag: its state does not fit the launch's LDS and lives in its slices of the device buffers)
@pytest.mark.parametrize("H,niter,Ms", [(3, 20, SMALL), (20, 20, SMALL + [50]), (40, 8, SMALL[:6])])
def test_sparse_full_cov(pkg, H, niter, Ms):
    L = 166
    pkg.set_defaults(y_dtype=pkg.VBMF_Y_F32, factor_dtype=pkg.VBMF_FACTOR_AUTO)
    po, draw = _model("sparse", L, H, 700 + H)
    Ys = [_f32(draw(m)) for m in Ms]
    qg, qo = _sets(pkg, Ys, po, 50)
    _mark_starts(qg)
    for Y, q in zip(Ys, qo):
        _oracle_full(Y, q, niter, "sparse")
    pkg.vbls_sparse_batch_(Ys, qg, niter, full_cov=True)
    _worst(f"vbls_sparse_batch_ full_cov {len(Ys)} bags H{H} x{niter}", qg, qo, TOL[True])
    _single_bag(pkg, Ys, qg, niter, True, f"vbls_sparse_batch_ full_cov vs vbls_ per bag H{H} x{niter}")


@pytest.mark.parametrize("full_cov", [False, True])
def test_dual(pkg, full_cov):
    L, H, niter = 166, 6, 20
    pkg.set_defaults(y_dtype=pkg.VBMF_Y_F32, factor_dtype=pkg.VBMF_FACTOR_AUTO)
    po, draw = _model("dual", L, H, 801)
    Ys = [_f32(draw(m)) for m in (SMALL if full_cov else RAGGED)]
    qg, qo = _sets(pkg, Ys, po, 60)
    for Y, q in zip(Ys, qo):
        if full_cov:
            _oracle_full(Y, q, niter, "dual")
        else:
            O.vbls_dual_(Y, q, niter)
    pkg.vbls_sparse_batch_(Ys, qg, niter, full_cov=full_cov)
    _worst(f"vbls_sparse_batch_ dual full_cov={int(full_cov)} {len(Ys)} bags H{H} x{niter}", qg, qo, TOL[full_cov],
           FIELDS + ("CA0", "CA1", "beta0", "beta1", "A0Hat", "A1Hat"))
    for g, o in zip(qg, qo):
        assert g.alpha0 == o.alpha0 and g.alpha1 == o.alpha1 and np.array_equal(g.alpha, o.alpha)


def test_trial(pkg):
    L, H, niter = 166, 6, 20
    pkg.set_defaults(y_dtype=pkg.VBMF_Y_F32, factor_dtype=pkg.VBMF_FACTOR_AUTO)
    po, draw = _model("trial", L, H, 901)
    Ys = [_f32(draw(m)) for m in RAGGED[:24]]
    for which in (0, 1):                          # the two sets copy_vbmf_params returns (groups (1, 2) and (1, 3))
        qg, qo = _sets(pkg, Ys, po, 70, which)
        for Y, q in zip(Ys, qo):
            O.vbls_trial_(Y, q, niter)
        pkg.vbls_sparse_batch_(Ys, qg, niter)
        _worst(f"vbls_sparse_batch_ trial set {which} {len(Ys)} bags H{H} x{niter}", qg, qo, TOL[False],
               FIELDS + ("CA1", "CA2", "beta1", "beta2", "A1Hat", "A2Hat"))
        for g, o in zip(qg, qo):
            assert np.array_equal(g.alpha, o.alpha) and g.A3Hat.shape[0] == 0


def test_qs1_layout_off(pkg):
    L, H, niter = 166, 5, 60
    pkg.set_defaults(y_dtype=pkg.VBMF_Y_F32, factor_dtype=pkg.VBMF_FACTOR_AUTO)
    po, draw = _model("sparse", L, H, 1001)
    Ys = [_f32(draw(m)) for m in RAGGED[:20]]
    qg, qo = _sets(pkg, Ys, po, 80)
    for Y, q in zip(Ys, qo):
        O.vbls_sparse_(Y, q, niter, reference_compat=False)
    bags = pkg.SparseBags(Ys, H, reference_compat=pkg.capi.VBMF_COMPAT_DEFAULT & ~pkg.capi.VBMF_COMPAT_SPARSE_REPEAT)
    pkg.vbls_sparse_batch_(bags, qg, niter)
    bags.close()
    _worst(f"vbls_sparse_batch_ diag QS1 off {len(Ys)} bags H{H} x{niter}", qg, qo, TOL[False])


@pytest.mark.parametrize("full_cov", [False, True])
def test_start_values_and_order(pkg, full_cov):
    """Different sigma / CA starts per bag are honoured, and permuting the bags changes no bag's result."""
    L, H, niter = 166, 5, 30
    pkg.set_defaults(y_dtype=pkg.VBMF_Y_F32, factor_dtype=pkg.VBMF_FACTOR_AUTO)
    po, draw = _model("sparse", L, H, 1101)
    Ms = SMALL if full_cov else RAGGED[:24]
    Ys = [_f32(draw(m)) for m in Ms]
    rng = np.random.default_rng(9)
    sig = rng.uniform(5.0, 400.0, len(Ys))
    cas = [rng.uniform(0.05, 2.0, m * H) for m in Ms]

    def fresh(order):
        qg, qo = _sets(pkg, [Ys[i] for i in order], po, 90)
        for k, i in enumerate(order):
            for q in (qg[k], qo[k]):
                q.sigmaHat, q.CA = float(sig[i]), cas[i].copy()
        return qg, qo
    order = list(range(len(Ys)))
    qg, qo = fresh(order)
    for k in order:
        if full_cov:
            _oracle_full(Ys[k], qo[k], niter, "sparse")
        else:
            O.vbls_sparse_(Ys[k], qo[k], niter)
    pkg.vbls_sparse_batch_(Ys, qg, niter, full_cov=full_cov)
    _worst(f"vbls_sparse_batch_ full_cov={int(full_cov)} per-bag start values H{H} x{niter}", qg, qo, TOL[full_cov])
    perm = list(np.random.default_rng(4).permutation(len(Ys)))
    qp, _ = fresh(perm)
    pkg.vbls_sparse_batch_([Ys[i] for i in perm], qp, niter, full_cov=full_cov)
    for k, i in enumerate(perm):
        e = _errs(qp[k], qg[i])
        assert max(e.values()) < 1e-6, (i, e)


def test_state_untouched_and_two_bases_on_one_upload(pkg):
    L, H, niter = 166, 4, 40
    pkg.set_defaults(y_dtype=pkg.VBMF_Y_F32, factor_dtype=pkg.VBMF_FACTOR_AUTO)
    po0, draw = _model("sparse", L, H, 1201)
    po1, _ = _model("sparse", L, H, 1202)
    Ys = [draw(m) for m in RAGGED[:16]]
    bags = pkg.SparseBags(Ys, H)
    ctx = bags.ctx
    nb, M = len(Ys), bags.M
    rng = np.random.default_rng(5)
    hyper = dict(alpha0=1e-3, beta0=1e-3, gamma0=1e-3, delta0=1e-3, eta0=1e-3, zeta0=1e-3)
    ctx.sparse_set_state(rng.standard_normal(M * H), np.full(M * H, 0.3), np.full(M * H, 0.7), np.full(M * H, 2.0), po0.BHat,
                         po0.SigmaB, po0.CB, po0.delta, 3.0, 7.0, hyper)
    before = ctx.sparse_get_state()
    for full_cov in (False, True):
        ctx.sparse_run_fixed_basis_batched(bags.col_off, niter, np.full((nb, H), 0.5), np.full((nb, H), 1e-3), np.full(nb, 10.0),
                                           np.full(nb, 1e-3), np.full(nb, 50.0), np.ones(M * H), full_cov=full_cov)
        after = ctx.sparse_get_state()
        for k, v in before.items():
            assert np.array_equal(np.asarray(v), np.asarray(after[k])), k
    # res0 then res1 on one upload == two fresh runs
    runs = {}
    for tag, po in (("res0", po0), ("res1", po1)):
        qs, _ = _sets(pkg, Ys, po, 100)
        pkg.vbls_sparse_batch_(bags, qs, niter)
        qf, _ = _sets(pkg, Ys, po, 100)
        pkg.vbls_sparse_batch_(Ys, qf, niter)
        for a, b in zip(qs, qf):
            e = _errs(a, b)
            assert max(e.values()) < 1e-12, e
        runs[tag] = qs
    assert relF(runs["res0"][0].AHat, runs["res1"][0].AHat) > 1e-3          # two bases, two answers
    bags.close()


@pytest.mark.parametrize("full_cov", [False, True])
def test_bf16_storage(pkg, full_cov):
    L, H, niter = 166, 6, 20
    try:
        pkg.set_defaults(y_dtype=pkg.VBMF_Y_BF16, factor_dtype=pkg.VBMF_FACTOR_AUTO)
        po, draw = _model("sparse", L, H, 1301)
        Ys = [draw(m) for m in (SMALL if full_cov else RAGGED[:20])]
        bags = pkg.SparseBags(Ys, H)
        Yst = bags.ctx.get_Y()                        # the bags exactly as the device stores them
        Yss = [np.ascontiguousarray(Yst[:, c0:c1]) for c0, c1 in zip(bags.col_off[:-1], bags.col_off[1:])]
        qg, qo = _sets(pkg, Yss, po, 110)
        for Y, q in zip(Yss, qo):
            if full_cov:
                _oracle_full(Y, q, niter, "sparse")
            else:
                O.vbls_sparse_(Y, q, niter)
        pkg.vbls_sparse_batch_(bags, qg, niter, full_cov=full_cov)
        _worst(f"vbls_sparse_batch_ full_cov={int(full_cov)} bf16 storage H{H} x{niter}", qg, qo, TOL_BF16[full_cov])
        bags.close()
    finally:
        pkg.set_defaults(y_dtype=pkg.VBMF_Y_F32, factor_dtype=pkg.VBMF_FACTOR_AUTO)


def test_many_bags_in_one_call(pkg):
    L, H, nb = 166, 5, 4096
    pkg.set_defaults(y_dtype=pkg.VBMF_Y_F32, factor_dtype=pkg.VBMF_FACTOR_AUTO)
    po, draw = _model("sparse", L, H, 1401)
    Ms = np.random.default_rng(11).integers(1, 41, nb)
    Ys = [_f32(draw(int(m))) for m in Ms]
    sample = sorted(set(np.random.default_rng(12).choice(nb, 16, replace=False).tolist()) | {0, nb - 1})
    for full_cov, niter in ((False, 150), (True, 20)):
        qg, qo = _sets(pkg, Ys, po, 5000)
        pkg.vbls_sparse_batch_(Ys, qg, niter, full_cov=full_cov)
        for b in sample:
            if full_cov:
                _oracle_full(Ys[b], qo[b], niter, "sparse")
            else:
                O.vbls_sparse_(Ys[b], qo[b], niter)
        _worst(f"vbls_sparse_batch_ full_cov={int(full_cov)} {nb} bags H{H} x{niter} (sample)", [qg[b] for b in sample],
               [qo[b] for b in sample], TOL[full_cov])
        assert all(np.isfinite(q.ATVecHat).all() and q.sigmaHat > 0 for q in qg)


def test_refusals_launch_nothing(pkg):
    C = pkg.capi
    VI = C.VBMF_ERR_INVALID
    L, M, H = 64, 40, 4
    rng = np.random.default_rng(13)
    Y = rng.standard_normal((L, M))
    B = rng.standard_normal((L, H))
    off = np.array([0, 1, 17, 33, M], dtype=np.int64)
    nb = off.size - 1
    hyper = dict(alpha0=1e-3, beta0=1e-3, gamma0=1e-3, delta0=1e-3, eta0=1e-3, zeta0=1e-3)

    def state(c, m=M, h=H, **kw):
        c.sparse_set_state(np.zeros(m * h), np.ones(m * h), np.ones(m * h), np.ones(m * h), B[:, :h] if h <= H else
                           rng.standard_normal((L, h)), 0.01 * np.eye(h), np.ones(h), np.ones(h), 1.0, 0.0, hyper, **kw)

    def run(c, o=off, niter=10, h=H, sig=None, full_cov=False):
        n = len(o) - 1
        return c.sparse_run_fixed_basis_batched(o, niter, np.full((n, h), 0.5), np.full((n, h), 1e-3), np.full(n, 40.0),
                                                np.full(n, 1e-3), np.full(n, 30.0) if sig is None else sig, np.ones(M * h),
                                                full_cov=full_cov)

    def refused(c, **kw):
        with pytest.raises(pkg.VbmfError) as e:
            run(c, **kw)
        assert e.value.code == VI, e.value
        return str(e.value)

    with C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32, variant=C.VBMF_VARIANT_SPARSE_DIAG) as c:
        c.set_Y(Y)
        state(c)
        run(c)
        words = c.dims()["Hp"] * c.dims()["XT1"] * 32
        P0 = c.peek(C.PEEK_P, words)
        refused(c, niter=0)
        for bad in ([0, 1, 1, M], [1, 17, M], [0, 17, M - 1], [0, 20, 10, M], [0, M + 1]):
            refused(c, o=np.array(bad, dtype=np.int64))
        # a required pointer that is NULL
        n = nb
        rc = C.lib().vbmf_sparse_run_fixed_basis_batched(c._h, n, off.ctypes.data_as(C.C.POINTER(C.C.c_int64)), 10, 0, None, None,
                                                         None, None, None, None, None, None, None, None, None)
        assert rc == VI
        state(c, labels0=[0, 5], H1=1)
        assert "mask" in refused(c)
        assert np.array_equal(c.peek(C.PEEK_P, words), P0)          # nothing ran
        state(c)
        # a NaN sigma in one bag: VBMF_ERR_NUMERIC, either form; the next call is clean
        for full_cov in (False, True):
            s = np.full(nb, 30.0); s[2] = np.nan
            with pytest.raises(pkg.VbmfError) as e:
                run(c, sig=s, full_cov=full_cov)
            assert e.value.code == C.VBMF_ERR_NUMERIC
            r = run(c, full_cov=full_cov)
            assert np.isfinite(r["ATVecHat"]).all() and np.isfinite(r["sigmaHat"]).all()
    with C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32) as c:
        assert "basic" in refused(c)
    for v in (C.VBMF_VARIANT_SPARSE_DIAGVAR, C.VBMF_VARIANT_DUAL_DIAGVAR, C.VBMF_VARIANT_TRIAL_DIAGVAR):
        with C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32, variant=v) as c:
            assert "diag_var" in refused(c)
    with C.Context(L, M, 65, y_dtype=pkg.VBMF_Y_F32, variant=C.VBMF_VARIANT_SPARSE_DIAG) as c:
        assert "64" in refused(c, h=65)
    with C.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32, nranks=2, rank=0, L_global=2 * L, variant=C.VBMF_VARIANT_SPARSE_DIAG) as c:
        assert "rank" in refused(c)
