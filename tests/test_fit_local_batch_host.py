"""Many three-group / label-masked sparse fits in one device call (vbmf_local_fit_batched / vbmf_trial_batch_ /
vbmf_sparse_masked_batch_ / train_local_folds): the parts that need no GPU -- the C ABI is declared, exported and bound, the Julia host
binds it, the Python hosts refuse what the batched path does not cover BEFORE any device call, and train_local_folds draws its start
values in fold order and repeats exactly the folds the reference's loop (examples/mil_util.jl:312-317) would repeat."""
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as G

ROOT = G.ROOT


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


def test_header_declares_and_library_exports(pkg):
    hdr = open(os.path.join(ROOT, "include", "vbmf_hip.h")).read()
    assert re.search(r"int\s+vbmf_local_fit_batched\s*\(\s*vbmf_ctx\*\s*ctx\s*,\s*int64_t\s+nbags\s*,\s*const\s+int64_t\*\s*col_off\s*,\s*"
                     r"int64_t\s+nfits\s*,\s*const\s+int64_t\*\s*fit_bag\s*,\s*int64_t\s+niter\s*,\s*double\s+eps\s*,\s*int\s+full_cov\s*,\s*"
                     r"int\s+est_cb\s*,\s*int\s+est_priors\s*,\s*int64_t\s+H0\s*,\s*const\s+int64_t\*\s*M0\s*,\s*int64_t\s+mask_H1", hdr)
    assert hasattr(ctypes.CDLL(pkg.capi.LIB_PATH), "vbmf_local_fit_batched")
    assert "vbmf_local_fit_batched" in pkg.capi.SYMBOLS
    assert len(pkg.capi.lib().vbmf_local_fit_batched.argtypes) == 33
    assert hasattr(pkg.capi.Context, "local_fit_batched")
    for name in ("vbmf_trial_batch_", "vbmf_sparse_masked_batch_", "train_local_folds"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))


def test_julia_host_binds_it():
    jl = open(os.path.join(G.PKG_DIR, "julia", "VBMatrixFactorizationHIP.jl")).read()
    assert re.search(r"ccall\(\(:vbmf_local_fit_batched,\s*libvbmf\)", jl)
    assert re.search(r"function vbmf_trial_batch!\(Ys::Vector\{Matrix\{Float64\}\},\s*ps::Vector\{vbmf_trial_parameters\},\s*niter::Int;", jl)
    assert re.search(r"function vbmf_sparse_masked_batch!\(Ys::Vector\{Matrix\{Float64\}\},\s*ps::Vector\{vbmf_sparse_parameters\},\s*niter::Int;", jl)
    assert re.search(r"export[^\n]*\n?[^\n]*vbmf_trial_batch!,\s*vbmf_sparse_masked_batch!", jl)


@pytest.fixture
def no_device(pkg, monkeypatch):
    """Any attempt to reach the library fails the test (the refusals happen on the host)."""
    def boom(*a, **k):
        raise AssertionError("the batched fit touched the device before refusing")
    monkeypatch.setattr(pkg.capi, "lib", boom)
    monkeypatch.setattr(pkg.capi.Context, "__init__", boom)
    monkeypatch.setattr(pkg.Session, "__init__", boom)
    return pkg


M0S = (2, 0, 7)


def _fits(pkg, kind, L=30, Ms=(3, 2, 7), H=4, seed=0, bag_of=None):
    rng = np.random.default_rng(seed)
    Ys = [rng.standard_normal((L, m)) for m in Ms]
    bag_of = range(len(Ms)) if bag_of is None else bag_of
    if kind == "trial":
        return Ys, [pkg.vbmf_trial_init(Ys[b], H, 2, M0S[b], rng=rng) for b in bag_of]
    return Ys, [pkg.vbmf_sparse_init(Ys[b], H, H1=2, labels=np.arange(1, M0S[b] + 1), rng=rng) for b in bag_of]


def _fit(pkg, kind):
    return pkg.vbmf_trial_batch_ if kind == "trial" else pkg.vbmf_sparse_masked_batch_


def _refused(pkg, kind, Ys, ps, match=None, niter=10, **kw):
    kw.setdefault("full_cov", True)
    with pytest.raises(ValueError, match=match or _fit(pkg, kind).__name__):
        _fit(pkg, kind)(Ys, ps, niter, **kw)


@pytest.mark.parametrize("kind", ["trial", "masked"])
def test_refusals_happen_on_the_host(no_device, kind):
    pkg = no_device
    one = "vbmf_trial_" if kind == "trial" else "vbmf_sparse_"
    Ys, ps = _fits(pkg, kind)
    Ys[1] = np.zeros((31, 2))
    _refused(pkg, kind, Ys, ps, match=f"one at a time with {one}")  # mismatched L, and the pointer to the per-fit call
    Ys, ps = _fits(pkg, kind)
    ps[0], ps[2] = ps[2], ps[0]
    _refused(pkg, kind, Ys, ps)                                     # parameters of another bag's shape
    Ys, ps = _fits(pkg, kind)
    _refused(pkg, kind, Ys, ps[:2], match="bag_of")                 # fewer sets than bags and no bag_of
    _refused(pkg, kind, Ys, ps, match="bag_of", bag_of=[0, 1, 3])   # a bag that does not exist
    _refused(pkg, kind, Ys, [], match="no parameter sets")
    _refused(pkg, kind, Ys, ps, match="niter", niter=0)
    ps[1].CA = np.ones(5)
    _refused(pkg, kind, Ys, ps, match="shape")                      # wrong shapes
    Ys, ps = _fits(pkg, kind)
    ps[1].BHat = ps[1].BHat[:-1]
    _refused(pkg, kind, Ys, ps, match="shape")
    Ys, ps = _fits(pkg, kind)
    ps[2].SigmaB = np.zeros((3, 3))
    _refused(pkg, kind, Ys, ps, match="shape")
    Ys, ps = _fits(pkg, kind, Ms=(3, 1, 7))
    ps[1] = (pkg.vbmf_trial_init(Ys[1], 4, 2, 0) if kind == "trial" else pkg.vbmf_sparse_init(Ys[1], 4, H1=2))
    _refused(pkg, kind, Ys, ps, match="1-column", full_cov=False)   # the diagonal form under the repeat layout needs M >= 2
    Ys, ps = _fits(pkg, kind)
    ps[1].eta = ps[1].eta + 3.0
    _refused(pkg, kind, Ys, ps, match="eta")
    Ys, ps = _fits(pkg, kind, H=33)
    _refused(pkg, kind, Ys, ps, match="32")                         # H > 32
    Ys, ps = _fits(pkg, kind)
    ps[1] = _fits(pkg, "masked" if kind == "trial" else "trial")[1][1]
    _refused(pkg, kind, Ys, ps, match="one model type")             # wrong parameter type beside the right one
    Ys, ps = _fits(pkg, kind)
    _refused(pkg, kind, Ys, [pkg.vbmf_dual_init(Y, 4, 2) for Y in Ys], match="one model type")   # ... and in front
    _refused(pkg, kind, Ys, [pkg.vbmf_init(Y, 4) for Y in Ys], match="one model type")
    # restarts: several sets on one bag are fine as far as the host checks go, and the first device call is the upload
    Ys, ps = _fits(pkg, kind, bag_of=[2, 2, 0])
    with pytest.raises(AssertionError, match="touched the device"):
        _fit(pkg, kind)(Ys, ps, 10, bag_of=[2, 2, 0])


def test_trial_refuses_mixed_H0_and_bad_M0(no_device):
    pkg = no_device
    Ys, ps = _fits(pkg, "trial")
    ps[2] = pkg.vbmf_trial_init(Ys[2], 4, 3, 7, rng=np.random.default_rng(1))
    _refused(pkg, "trial", Ys, ps, match="H0")                      # mixed H0
    Ys, ps = _fits(pkg, "trial")
    ps[0].M0 = 4                                                    # M = 3
    _refused(pkg, "trial", Ys, ps, match="M0")
    Ys, ps = _fits(pkg, "trial")                                    # M0 = 0, M0 = M and H0 = 0 / H are all models the entry runs
    for p in ps:
        p.H0 = 0
    with pytest.raises(AssertionError, match="touched the device"):
        pkg.vbmf_trial_batch_(Ys, ps, 10)


def test_masked_refuses_non_prefix_labels_and_mixed_H1(no_device):
    pkg = no_device
    for labels in ([2, 3], [1, 3], [2], [1, 1], [1, 2, 3, 4, 5, 6, 7, 8], [0, 1]):
        Ys, ps = _fits(pkg, "masked")
        ps[2].labels = np.array(labels, dtype=np.int64)
        _refused(pkg, "masked", Ys, ps, match="prefix")             # non-prefix labels (1-based, like the reference's)
        _refused(pkg, "masked", Ys, ps, match="vbmf_sparse_")
    Ys, ps = _fits(pkg, "masked")
    ps[1].H1 = 1
    _refused(pkg, "masked", Ys, ps, match="H1")                     # mixed H1
    Ys, ps = _fits(pkg, "masked")
    for p in ps:
        p.H1 = 5
    _refused(pkg, "masked", Ys, ps, match="H1")                     # H1 > H
    Ys, ps = _fits(pkg, "masked")                                   # empty labels and full prefixes are fine
    with pytest.raises(AssertionError, match="touched the device"):
        pkg.vbmf_sparse_masked_batch_(Ys, ps, 10)


# ---- train_local_folds --------------------------------------------------------------------------------------------------------------------
def _folds(seed=0, L=12, shapes=((4, 5), (0, 6), (3, 3), (7, 2))):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((L, a)), rng.standard_normal((L, b))) for a, b in shapes]


def _scripted(pkg, monkeypatch, rounds):
    """replaces the batch call by one that leaves, on the k-th set of call r, AHat and BHat filled with rounds[r][k] (a pair of scalars)
    and records what every call was given"""
    calls = []

    def fake(Ys, params, niter, **kw):
        params = list(params)
        r = len(calls)
        calls.append(dict(Ys=list(Ys), params=params, niter=niter, kw=kw, B0=[p.BHat.copy() for p in params],
                          A0=[p.AHat.copy() for p in params]))
        for p, (a, b) in zip(params, rounds[r]):
            p.AHat, p.BHat = a * np.ones_like(p.AHat), b * np.ones_like(p.BHat)
        return [0.5] * len(params)
    monkeypatch.setattr(pkg, "vbmf_sparse_masked_batch_", fake)
    return calls


def test_train_local_folds_draws_in_fold_order_and_runs_one_diagonal_call(pkg, monkeypatch):
    folds = _folds()
    calls = _scripted(pkg, monkeypatch, [[(1.0, 1.0)] * 4])
    ps = pkg.train_local_folds(folds, 3, 2, 40, rng=np.random.default_rng(5))
    assert len(calls) == 1 and len(ps) == 4
    c = calls[0]
    assert c["niter"] == 40 and c["kw"]["eps"] == 1e-4 and c["kw"]["full_cov"] is False      # :302, :314
    assert all(p is q for p, q in zip(ps, c["params"]))
    rng = np.random.default_rng(5)
    for (Y0, Y1), Y, p, A0, B0 in zip(folds, c["Ys"], ps, c["A0"], c["B0"]):
        M0 = Y0.shape[1]
        assert np.array_equal(Y, np.concatenate([Y0, Y1], axis=1))                          # :304
        assert isinstance(p, pkg.vbmf_sparse_parameters) and p.H1 == 2 and (p.L, p.M, p.H) == (12, Y.shape[1], 3)
        assert np.array_equal(p.labels, np.arange(1, M0 + 1))                               # :308, 1-based
        q = pkg.vbmf_sparse_init(Y, 3, H1=2, labels=np.arange(1, M0 + 1), rng=rng)          # the one generator, fold by fold
        assert np.array_equal(A0, q.AHat) and np.array_equal(B0, q.BHat)
        assert np.all(A0[:M0, 1:] == 0.0) and np.all(A0[M0:, :] != 0.0)
    assert pkg.train_local_folds([], 3, 2, 40) == []


def test_train_local_folds_repeats_what_the_references_loop_repeats(pkg, monkeypatch):
    """:312-317: after the first run a fold runs again while norm(AHat) < 1e-2 and norm(BHat) < 1e-2, ten runs at most, from where it
    stands (ones(M, H) c has the operator norm c sqrt(M H))"""
    folds = _folds()
    z = 1e-6
    rounds = [[(1.0, 1.0), (z, z), (z, 1.0), (z, z)],               # folds 1 and 3 fell to zero; fold 2 kept BHat: it stays
              [(z, z), (1.0, z)],                                   # fold 1 again; fold 3 recovered AHat
              [(1.0, 1.0)]]
    calls = _scripted(pkg, monkeypatch, rounds)
    ps = pkg.train_local_folds(folds, 3, 2, 40, eps=1e-5, rng=np.random.default_rng(5))
    assert [len(c["params"]) for c in calls] == [4, 2, 1]
    assert calls[1]["params"] == [ps[1], ps[3]] and calls[2]["params"] == [ps[1]]
    assert all(np.array_equal(Y, np.concatenate(folds[k], axis=1)) for Y, k in zip(calls[1]["Ys"], (1, 3)))
    assert np.all(calls[1]["B0"][0] == z) and np.all(calls[2]["A0"][0] == z)                # from where it stands, no new draw
    assert all(c["kw"]["eps"] == 1e-5 and c["kw"]["full_cov"] is False and c["niter"] == 40 for c in calls)
    # a fold that never recovers runs max_restarts = 10 times in all (:310)
    calls = _scripted(pkg, monkeypatch, [[(z, z), (1.0, 1.0)]] + [[(z, z)]] * 12)
    ps = pkg.train_local_folds(folds[:2], 3, 2, 40, rng=np.random.default_rng(5))
    assert [len(c["params"]) for c in calls] == [2] + [1] * 9
    assert all(c["params"] == [ps[0]] for c in calls[1:])
