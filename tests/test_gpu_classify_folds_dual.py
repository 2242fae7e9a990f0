"""classify_folds, test_classification_folds and validate_folds with class_alg = "dual" (vbmf_sparse_fixed_basis_jobs): every fold's
test bags against its own two dual models in ONE device call on the pool's own context, against the oracle's classify
(examples/mil_util.jl:515-530: 20 vbls! iterations with full_cov = true per model, err = norm(YHat - Y) / (L M), label 0 where
err0 < err1) and against classify_bags on a selection per fold.

Models and bags as test_classify_dual of tests/test_gpu_bag_scoring.py: _two_bases, the oracle's vbmf_dual_ with 12 sweeps and
est_priors = False, bags of widths SMALL * 2 drawn alternately from the two bases, rounded to fp32; three folds, each with its own
pair of bases and models.  Before the device is touched the test asserts, from the oracle alone, that the labels are decided: the
relative margin between err0 and err1 is at least 100 RESID_TOL and more than twice what the A tolerance of
tests/test_gpu_vbls_jobs.py (TOL[True]["ATVecHat"], 3 x the measured error) can move an err (_moved_by), and both labels occur in
every fold."""
import functools

import numpy as np
import pytest

import __graft_entry__ as G
from oracle import vbmf_oracle as O
from tests.helpers import report
from tests.test_gpu_bag_scoring import L, RESID_TOL, _margin, _moved_by, _oracle_vbls, _two_bases
from tests.test_gpu_vbls_jobs import TOL
from tests.test_gpu_vbls_sparse_batch import SMALL, _convert, _f32, _sets

pytestmark = pytest.mark.gpu

H, NITER, NFOLDS = 5, 20, 3
TOL_A = TOL[True]["ATVecHat"]


@pytest.fixture(scope="module")
def pkg():
    G.build()
    p = G.load_package()
    p.set_defaults(y_dtype=p.VBMF_Y_F32, factor_dtype=p.VBMF_FACTOR_AUTO)
    yield p
    p.invalidate()
    p.set_defaults(y_dtype=p.VBMF_Y_F32, factor_dtype=p.VBMF_FACTOR_AUTO)


@functools.lru_cache(maxsize=None)
def _case():
    """per fold: (res0, res1) trained by the oracle and its test bags; computed once and left unchanged"""
    folds = []
    for f in range(NFOLDS):
        draw = _two_bases(H, 6200 + 10 * f)
        res = []
        for k in range(2):
            Ytr = draw(k, 200)
            po = O.vbmf_dual_init(Ytr, H, 2, rng=np.random.default_rng(6210 + 10 * f + k), materialize_yhat=False)
            O.vbmf_dual_(Ytr, po, 12, eps=0.0, est_priors=False)
            res.append(po)
        Ys = [_f32(draw(b % 2, m)) for b, m in enumerate(SMALL * 2)]
        folds.append((res, Ys))
    return folds


@functools.lru_cache(maxsize=None)
def _oracle_side():
    """per fold: (labels, err0, err1, the largest movement TOL_A allows) from the oracle's loop, and the asserted preconditions"""
    pkg = G.load_package()                                             # (copy_vbmf_params on the host: no device)
    out = []
    for res, Ys in _case():
        errs, moved = [], 0.0
        for po in res:
            _, qo = _sets(pkg, Ys, po, 6300)
            e = []
            for Y, q in zip(Ys, qo):
                _oracle_vbls("dual", Y, q, NITER, True)
                r = np.linalg.norm(po.BHat @ q.AHat.T - Y)
                e.append(r / (L * Y.shape[1]))
                moved = max(moved, _moved_by(po.BHat, q.AHat, r, TOL_A))
            errs.append(np.array(e))
        want = np.where(errs[0] < errs[1], 0, 1)
        margin = _margin(*errs)
        assert margin >= 100 * RESID_TOL and margin > 2 * moved, (margin, moved)
        assert 0 < want.sum() < len(Ys)
        out.append((want, errs[0], errs[1], moved, margin))
    return out


def _pool_side(pkg):
    """(all bags, the folds' models as package sets, the folds' test ids, the bags' true labels)"""
    P = pkg.vbmf_dual_parameters
    Yall, models, tests = [], [], []
    for res, Ys in _case():
        tests.append(list(range(len(Yall), len(Yall) + len(Ys))))
        Yall += Ys
        models.append((_convert(P, res[0]), _convert(P, res[1])))
    labels = np.array([b % 2 for _, Ys in _case() for b in range(len(Ys))])
    return Yall, models, tests, labels


def test_classify_folds_dual_gives_the_oracle_s_labels(pkg, monkeypatch):
    want = _oracle_side()                                              # (asserts the preconditions before any device call)
    Yall, models, tests, labels = _pool_side(pkg)
    models4, tests4 = models + [(0, 0)], tests + [[2, 5]]
    made = []
    init = pkg.capi.Context.__init__

    def counting(self, *a, **k):
        made.append(a)
        return init(self, *a, **k)

    with pkg.BagPool(Yall) as pool:
        monkeypatch.setattr(pkg.capi.Context, "__init__", counting)
        out = pkg.classify_folds(models4, tests4, pool, "dual")
        summ = pkg.test_classification_folds(models4, tests4, pool, labels, "dual")
        assert made == []                                              # on the pool's own context: no select, no new context
        monkeypatch.setattr(pkg.capi.Context, "__init__", init)
        assert out[3] is None and summ[3] == (-1.0,) * 6
        for f, (lab, e0, e1, moved, margin) in enumerate(want):
            got = out[f]
            d = max(float(np.max(np.abs(got[1] - e0) / e0)), float(np.max(np.abs(got[2] - e1) / e1)))
            report(f"classify_folds dual fold {f} H{H} {len(lab)} bags: err={d:.2e} bound={moved:.2e} margin={margin:.2e} ones={int(lab.sum())}")
            assert np.array_equal(got[0], lab) and got[0].dtype == np.int64
            assert d <= moved, (f, d, moved)
            # the same labels as classify_bags on a selection of the fold's bags; the counts from those labels
            sel = pool.select(tests[f], H, kind="sparse")
            try:
                per_fold = pkg.classify_bags(models[f][0], models[f][1], sel, "dual")
            finally:
                sel.close()
            assert np.array_equal(per_fold[0], got[0])
            assert summ[f] == pkg._classification_counts("t", labels[tests[f]], got[0])
            assert summ[f] == pkg.test_classification_batch(models[f][0], models[f][1], [Yall[b] for b in tests[f]], labels[tests[f]], "dual")
        # a list of matrices and an upload of any rank serve as the pool does, bit for bit
        uploaded = pkg.Bags(Yall, 3)
        try:
            for src in (Yall, uploaded):
                again = pkg.classify_folds(models4, tests4, src, "dual")
                assert again[3] is None
                assert all(np.array_equal(a, b) for f in range(NFOLDS) for a, b in zip(again[f], out[f]))
        finally:
            uploaded.close()
        # niter reaches the device: one iteration gives other errs
        one = pkg.classify_folds(models, tests, pool, "dual", niter=1)
        assert not np.array_equal(one[0][1], out[0][1])


def test_validate_folds_dual_is_train_dual_folds_then_test_classification_folds(pkg):
    Yall, _, tests, labels = _pool_side(pkg)
    ids = tests[0]
    splits = [(ids[8:], ids[:8]), (ids[:8] + ids[16:], ids[8:16])]
    with pkg.BagPool(Yall) as pool:
        got = pkg.validate_folds(pool, labels, splits, "unread", H, 8, eps=1e-4, class_alg="dual", rng=np.random.default_rng(78), H1=3, nstarts=2)
        folds = [([b for b in tr if labels[b] == 0], [b for b in tr if labels[b] == 1]) for tr, _ in splits]
        models = pkg.train_dual_folds(folds, H, H - 3, 8, eps=1e-4, nstarts=2, rng=np.random.default_rng(78), pool=pool)
        want = pkg.test_classification_folds(models, [te for _, te in splits], pool, labels, "dual")
        # a split with an empty class trains nothing: -1 six times
        empty = pkg.validate_folds(pool, labels, [([b for b in ids if labels[b] == 0], ids[:4])], "unread", H, 8, class_alg="dual",
                                   rng=np.random.default_rng(78), nstarts=2)
    assert got == want and len(got) == 2
    assert all(t[4] + t[5] == 8 and 0.0 <= t[0] <= 1.0 for t in got)
    assert empty == [(-1.0,) * 6]
