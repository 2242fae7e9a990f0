"""Batched whole fits with per-row noise (vbmf_rows_fit_batched / vbmf_*_batch_(..., diag_var=True) / train_local_folds(diag_var) /
train_dual_folds): the parts that need no GPU -- the C ABI is declared, exported and bound, the Julia host binds it, diag_var=True
reaches Context.rows_fit_batched with the right arguments and the results land in the right fields, the host-side refusals of the new
keyword paths (recorded in tests/golden/fit_rows_batch_refusals.json), train_dual_folds' draw order and keep rule, and the refusals of
fit_restarts / train_folds that stay."""
import contextlib
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import __graft_entry__ as G

ROOT = G.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "fit_rows_batch_refusals.json")


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports(pkg):
    hdr = open(os.path.join(ROOT, "include", "vbmf_hip.h")).read()
    m = re.search(r"int\s+vbmf_rows_fit_batched\s*\(([^;]*)\);", hdr)
    local = re.search(r"int\s+vbmf_local_fit_batched\s*\(([^;]*)\);", hdr)
    types = lambda s: [re.sub(r"\s*\w+$", "", a.strip()) for a in re.sub(r"/\*.*?\*/", "", s, flags=re.S).split(",")]
    assert m and types(m.group(1)) == types(local.group(1)) and len(types(m.group(1))) == 33
    assert re.search(r"const\s+int64_t\*\s*M0\s*,\s*int64_t\s+mask_H1\s*,[^;]*etaVec[^;]*sigmaVec[^;]*zetaVec", m.group(1))
    doc = hdr[:m.start()].rsplit("/*", 1)[1]
    for cite in ("examples/mil_util.jl:667", ":207-230", ":180-193", ":256-261", ":309-315", "SQUARED"):
        assert cite in doc, cite
    assert hasattr(C.CDLL(pkg.capi.LIB_PATH), "vbmf_rows_fit_batched")
    assert "vbmf_rows_fit_batched" in pkg.capi.SYMBOLS
    assert pkg.capi.lib().vbmf_rows_fit_batched.argtypes == pkg.capi.lib().vbmf_local_fit_batched.argtypes
    assert hasattr(pkg.capi.Context, "rows_fit_batched")
    assert "train_dual_folds" in pkg.__all__ and callable(pkg.train_dual_folds)


def test_julia_host_binds_it():
    jl = open(os.path.join(G.PKG_DIR, "julia", "VBMatrixFactorizationHIP.jl")).read()
    assert re.search(r"ccall\(\(:vbmf_rows_fit_batched,\s*libvbmf\)", jl)
    for fn in ("vbmf_sparse_batch!", "vbmf_dual_batch!", "vbmf_trial_batch!", "vbmf_sparse_masked_batch!"):
        sig = re.search(r"function " + re.escape(fn) + r"\((.*?)\)\n", jl, flags=re.S)
        assert sig and re.search(r"diag_var::Bool\s*=\s*false", sig.group(1)), fn


# ---- Context.rows_fit_batched against a library written in Python ---------------------------------------------------------------------------
L, H = 5, 3
COL_OFF, FIT_BAG, HANDLE = [0, 3, 4, 6], [2, 0, 2, 1], 0x5EED
NB, NF, MH = 3, 4, 8 * H


class FakeLib:
    """vbmf_rows_fit_batched in Python: records every argument as the C ABI reads it and fills every output with values of its own"""
    NAMES = ("ctx", "nbags", "col_off", "nfits", "fit_bag", "niter", "eps", "full_cov", "est_cb", "est_priors", "H0", "M0", "mask_H1",
             "gamma", "delta0", "etaVec", "zeta0", "priors9", "BHat", "SigmaB", "CB", "sigmaVec", "CA", "delta", "zetaVec", "beta",
             "diagSigmaATVec", "SigmaA", "ATVecHat", "iters", "d", "status", "trace")

    def __init__(self):
        self.calls = []

    def vbmf_destroy(self, h):
        pass

    def vbmf_rows_fit_batched(self, *args):
        assert len(args) == len(self.NAMES)
        a = dict(zip(self.NAMES, args))
        nf, niter = a["nfits"], a["niter"]
        sizes = dict(col_off=a["nbags"] + 1, fit_bag=nf, M0=nf, gamma=nf, delta0=nf, etaVec=nf, zeta0=nf, priors9=nf * 9, BHat=nf * L * H,
                     SigmaB=nf * H * H, CB=nf * H, sigmaVec=nf * L, CA=MH, delta=nf * H, zetaVec=nf * L, beta=MH, diagSigmaATVec=MH,
                     SigmaA=nf * H * H, ATVecHat=MH, iters=nf, d=nf, status=nf, trace=nf * niter * 2)
        seen = {}
        for pos, k in enumerate(self.NAMES):
            v = a[k]
            if k not in sizes or v is None:
                seen[k] = v
                continue
            view = np.ctypeslib.as_array(v, shape=(sizes[k],))
            seen[k] = view.copy()
            if pos >= self.NAMES.index("priors9"):
                view[:] = (pos + 1) * 1000 + np.arange(sizes[k])
        self.calls.append(seen)
        return 0


@pytest.fixture
def ctx(pkg):
    c = pkg.capi.Context.__new__(pkg.capi.Context)
    c.L, c.M, c.H, c._h, c._lib = L, COL_OFF[-1], H, C.c_void_p(HANDLE), FakeLib()
    return c


def _inputs(seed=0):
    rng = np.random.default_rng(seed)
    r = lambda *s: rng.standard_normal(s)
    return dict(gamma=r(NF), delta0=r(NF), etaVec=r(NF), zeta0=r(NF), priors9=r(NF, 9), BHat=r(NF, L, H), SigmaB=r(NF, H, H), CB=r(NF, H),
                sigmaVecHat=r(NF, L), CA=r(MH))


@pytest.mark.parametrize("m0", [None, [1, 3, 0, 1]])
def test_context_marshals_the_rows_entry(ctx, m0):
    x = _inputs()
    keep = {k: v.copy() for k, v in x.items()}
    r = ctx.rows_fit_batched(COL_OFF, FIT_BAG, 7, 1e-3, x["gamma"], x["delta0"], x["etaVec"], x["zeta0"], x["priors9"], x["BHat"],
                             x["SigmaB"], x["CB"], x["sigmaVecHat"], x["CA"], M0=m0, H0=2, mask_H1=0, full_cov=True, est_cb=True,
                             est_priors=True, want_trace=True)
    (s,) = ctx._lib.calls
    assert s["ctx"].value == HANDLE and (s["nbags"], s["nfits"], s["niter"], s["eps"]) == (NB, NF, 7, 1e-3)
    assert (s["full_cov"], s["est_cb"], s["est_priors"], s["H0"], s["mask_H1"]) == (1, 1, 1, 2, 0)
    assert np.array_equal(s["col_off"], COL_OFF) and np.array_equal(s["fit_bag"], FIT_BAG)
    assert s["M0"] is None if m0 is None else np.array_equal(s["M0"], m0)               # None goes down as NULL: M0[f] = M_b
    for k in ("gamma", "delta0", "etaVec", "zeta0", "CB", "CA", "SigmaB", "priors9"):
        assert np.array_equal(s[k], keep[k].reshape(-1)), k
    assert np.array_equal(s["sigmaVec"], keep["sigmaVecHat"].reshape(-1))               # (nfits, L), fit by fit
    assert np.array_equal(s["BHat"].reshape(NF, H, L), keep["BHat"].transpose(0, 2, 1))  # per fit column-major
    assert all(np.array_equal(x[k], keep[k]) for k in x)                                # the caller's arrays are copied, not written
    pos = FakeLib.NAMES.index
    assert r["sigmaVecHat"].shape == (NF, L) and r["zetaVec"].shape == (NF, L) and "sigmaHat" not in r and "zeta" not in r
    assert np.array_equal(r["sigmaVecHat"].ravel(), (pos("sigmaVec") + 1) * 1000 + np.arange(NF * L))
    assert np.array_equal(r["zetaVec"].ravel(), (pos("zetaVec") + 1) * 1000 + np.arange(NF * L))
    assert r["priors9"].shape == (NF, 9) and r["trace"].shape == (NF, 7, 2) and r["delta"].shape == (NF, H)
    assert np.array_equal(r["iters"], (pos("iters") + 1) * 1000 + np.arange(NF))
    with pytest.raises(ValueError, match="sigmaVecHat"):
        ctx.rows_fit_batched(COL_OFF, FIT_BAG, 7, 1e-3, x["gamma"], x["delta0"], x["etaVec"], x["zeta0"], x["priors9"], x["BHat"],
                             x["SigmaB"], x["CB"], x["sigmaVecHat"][:, 0], x["CA"])
    r = ctx.rows_fit_batched(COL_OFF, FIT_BAG, 7, 1e-3, x["gamma"], x["delta0"], x["etaVec"], x["zeta0"], x["priors9"][:, :6], x["BHat"],
                             x["SigmaB"], x["CB"], x["sigmaVecHat"], x["CA"], est_cb=False)
    s = ctx._lib.calls[-1]
    assert s["H0"] == H and s["delta"] is None and s["trace"] is None and np.all(s["priors9"].reshape(NF, 9)[:, 6:] == 0.0)


# ---- the Python hosts on a scripted context ----------------------------------------------------------------------------------------------------
class ScriptedCtx:
    """stands where SparseBags.ctx stands: records the one call, answers with values that name their field and fit"""

    def __init__(self):
        self.calls = []

    def _any(self, name):
        def call(*a, **kw):
            self.calls.append((name, a, kw))
            return self._answer(name, a, kw)
        return call

    def __getattr__(self, name):
        if name.endswith("_fit_batched"):
            return self._any(name)
        raise AttributeError(name)

    def _answer(self, name, a, kw):
        col_off, bag_of, B = np.asarray(a[0]), list(a[1]), np.asarray(a[9])
        nf, Lr, Hr = B.shape
        mh = sum(int(col_off[b + 1] - col_off[b]) for b in bag_of) * Hr
        fill = lambda base, *shape: base + np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape)
        pri = np.tile(np.arange(1.0, 10.0), (nf, 1)) + 10.0 * np.arange(nf)[:, None]
        if name == "rows_fit_batched":
            noise = dict(sigmaVecHat=fill(500.0, nf, Lr), zetaVec=fill(600.0, nf, Lr), priors9=pri)
        else:
            noise = dict(sigmaHat=fill(500.0, nf), zeta=fill(600.0, nf), **({"priors4": pri[:, :4]} if name == "sparse_fit_batched" else {"priors9": pri}))
        return dict(BHat=fill(100.0, nf, Lr, Hr), SigmaB=fill(200.0, nf, Hr, Hr), CB=fill(300.0, nf, Hr), delta=fill(400.0, nf, Hr),
                    CA=fill(700.0, mh), beta=fill(800.0, mh), diagSigmaATVec=fill(900.0, mh), ATVecHat=fill(1000.0, mh),
                    SigmaA=fill(1100.0, nf, Hr, Hr), iters=np.arange(3, 3 + nf), d=0.25 + np.arange(nf), status=np.arange(nf) % 2,
                    trace=None, **noise)


@pytest.fixture
def scripted(pkg, monkeypatch):
    sc = ScriptedCtx()

    @contextlib.contextmanager
    def on_device(Ys, Hh, cls):
        class B:
            ctx = sc
            col_off = np.concatenate([[0], np.cumsum([np.shape(Y)[1] for Y in Ys])]).astype(np.int64)
        yield B
    monkeypatch.setattr(pkg, "_on_device", on_device)
    return sc


MS, M0S = (3, 2, 7), (2, 0, 7)


def _sets(pkg, kind, Ls=6, Hh=4, bag_of=(0, 1, 2, 2), seed=0):
    rng = np.random.default_rng(seed)
    Ys = [rng.standard_normal((Ls, m)) for m in MS]
    if kind == "sparse":
        ps = [pkg.vbmf_sparse_init(Ys[b], Hh, sigma=0.5 + b, rng=rng) for b in bag_of]
    elif kind == "dual":
        ps = [pkg.vbmf_dual_init(Ys[b], Hh, 1, sigma=0.5 + b, rng=rng) for b in bag_of]
    elif kind == "trial":
        ps = [pkg.vbmf_trial_init(Ys[b], Hh, 1, M0S[b], sigma=0.5 + b, rng=rng) for b in bag_of]
    else:
        ps = [pkg.vbmf_sparse_init(Ys[b], Hh, H1=2, labels=np.arange(1, M0S[b] + 1), sigma=0.5 + b, rng=rng) for b in bag_of]
    return Ys, ps


BATCH = dict(sparse="vbmf_sparse_batch_", dual="vbmf_dual_batch_", trial="vbmf_trial_batch_", masked="vbmf_sparse_masked_batch_")


@pytest.mark.parametrize("kind", list(BATCH))
def test_diag_var_reaches_the_rows_entry_and_fills_the_fields(pkg, scripted, kind):
    Hh, bag_of = 4, [0, 1, 2, 2]
    Ys, ps = _sets(pkg, kind)
    for k, p in enumerate(ps):
        p.sigmaVecHat = 0.1 * (k + 1) + np.arange(p.L)
        p.sigmaHat, p.zeta = 11.0 + k, 21.0 + k
    before = [(p.sigmaHat, p.zeta) for p in ps]
    sv0 = [p.sigmaVecHat.copy() for p in ps]
    extra = dict(est_priors=True) if kind in ("dual", "trial") else {}
    dual0 = [[p.alpha00, p.beta00, p.alpha01, p.beta01, p.alpha01, p.beta01] for p in ps] if kind == "dual" else None
    ds = getattr(pkg, BATCH[kind])(Ys, ps, 9, eps=1e-3, full_cov=(kind == "dual"), bag_of=bag_of, diag_var=True, **extra)
    ((name, a, kw),) = scripted.calls
    assert name == "rows_fit_batched"
    col_off, bo, niter, eps, gamma, delta0, eta, zeta0, pri, B, SB, CB, sv, CA, M0 = a
    assert list(bo) == bag_of and (niter, eps) == (9, 1e-3)
    assert list(eta) == [p.eta0 + p.M / 2 for p in ps]                               # etaVec[0] = eta0 + M_b / 2, not eta0 + L M_b / 2
    assert np.array_equal(np.asarray(sv), np.stack(sv0))                             # the start values are sigmaVecHat
    assert list(gamma) == [p.gamma0 + p.L / 2 for p in ps] and list(zeta0) == [p.zeta0 for p in ps]
    if kind in ("trial", "masked"):
        assert list(M0) == [M0S[b] for b in bag_of]
    else:
        assert M0 is None                                                            # every column in group 2: M0[f] = M_b
    assert kw["H0"] == (Hh if kind in ("sparse", "masked") else 1)                   # the sparse model: one prior group
    assert kw["mask_H1"] == (2 if kind == "masked" else 0)
    assert kw["full_cov"] == (kind == "dual") and kw["est_cb"] is True and bool(kw["est_priors"]) == (kind in ("dual", "trial"))
    assert np.shape(pri) == (4, 6)
    if kind == "dual":
        assert [list(row) for row in pri] == dual0
    # the fill rules
    assert ds == [0.25, 1.25, 2.25, 3.25]
    s0 = 0
    for k, p in enumerate(ps):
        assert (p.sigmaHat, p.zeta) == before[k]                                     # left as they were, as after vbmf_sparse_(diag_var)
        assert np.array_equal(p.sigmaVecHat, 500.0 + k * p.L + np.arange(p.L)) and np.array_equal(p.zetaVec, 600.0 + k * p.L + np.arange(p.L))
        assert p.iters == 3 + k and p.status == k % 2
        n = p.M * Hh
        assert np.array_equal(p.ATVecHat, 1000.0 + s0 + np.arange(n)) and np.array_equal(p.CA, 700.0 + s0 + np.arange(n))
        assert np.array_equal(p.AHat, p.ATVecHat.reshape(p.M, Hh)) and np.array_equal(p.BHat, 100.0 + k * p.L * Hh + np.arange(p.L * Hh).reshape(p.L, Hh))
        assert np.array_equal(p.delta, 400.0 + k * Hh + np.arange(Hh))
        s0 += n
        row = 10.0 * k + np.arange(1.0, 10.0)
        if kind == "dual":                                                           # slots 0-3 the pairs, 6 and 7 the posterior shapes
            assert [p.alpha00, p.beta00, p.alpha01, p.beta01] == list(row[:4]) and (p.alpha0, p.alpha1) == (row[6], row[7])
            assert np.array_equal(p.alpha, [row[6], row[7]]) and np.array_equal(p.A0Hat, p.AHat[:, :1])
        if kind == "trial":
            assert [getattr(p, n_) for n_ in pkg.capi.Context.TRIAL_KEYS] == list(row)


@pytest.mark.parametrize("kind", list(BATCH))
def test_without_diag_var_the_call_is_what_it_was(pkg, scripted, kind):
    Ys, ps = _sets(pkg, kind)
    sv0, sg0 = [p.sigmaVecHat.copy() for p in ps], [p.sigmaHat for p in ps]
    getattr(pkg, BATCH[kind])(Ys, ps, 9, bag_of=[0, 1, 2, 2])
    assert [p.sigmaHat for p in ps] == [500.0, 501.0, 502.0, 503.0] and all(np.array_equal(p.sigmaVecHat, v) for p, v in zip(ps, sv0))
    ((name, a, kw),) = scripted.calls
    assert name == ("local_fit_batched" if kind in ("trial", "masked") else "sparse_fit_batched")
    assert list(a[6]) == [p.eta0 + p.L * p.M / 2 for p in ps] and list(a[12]) == sg0
    assert np.shape(a[8]) == (4, 6 if kind in ("trial", "masked") else 4)


def test_train_local_folds_passes_diag_var_through(pkg, monkeypatch):
    seen = []
    monkeypatch.setattr(pkg, "vbmf_sparse_masked_batch_", lambda Ys, ps, niter, **kw: seen.append(kw) or [0.5] * len(ps))
    rng = np.random.default_rng(0)
    folds = [(rng.standard_normal((6, 2)), rng.standard_normal((6, 3)))]
    pkg.train_local_folds(folds, 3, 1, 5, rng=np.random.default_rng(1), diag_var=True)
    pkg.train_local_folds(folds, 3, 1, 5, rng=np.random.default_rng(1))
    assert seen == [dict(eps=1e-4, full_cov=False, diag_var=True), dict(eps=1e-4, full_cov=False)]     # (:314)


# ---- the host-side refusals of the new keyword paths -----------------------------------------------------------------------------------------
@pytest.fixture
def no_device(pkg, monkeypatch):
    """Any attempt to reach the library fails the test (the refusals happen on the host)."""
    def boom(*a, **k):
        raise AssertionError("the batched fit touched the device before refusing")
    monkeypatch.setattr(pkg.capi, "lib", boom)
    monkeypatch.setattr(pkg.capi.Context, "__init__", boom)
    monkeypatch.setattr(pkg.Session, "__init__", boom)
    return pkg


def _refusal_texts(pkg):
    """the text of every host-side refusal of the diag_var=True paths, by case"""
    out = {}

    def note(case, fn, *a, **kw):
        with pytest.raises(ValueError) as e:
            fn(*a, **kw)
        out[case] = str(e.value)
    for kind, fn in BATCH.items():
        f = getattr(pkg, fn)
        Ys, ps = _sets(pkg, kind)
        ps[1].sigmaVecHat = np.ones(5)
        note(f"{kind}: sigmaVecHat of another length", f, Ys, ps, 9, bag_of=[0, 1, 2, 2], diag_var=True)
        Ys, ps = _sets(pkg, kind)
        ps[2].sigmaVecHat = None
        note(f"{kind}: no sigmaVecHat", f, Ys, ps, 9, bag_of=[0, 1, 2, 2], diag_var=True)
        Ys, ps = _sets(pkg, kind)
        ps[0].etaVec = np.zeros(0)
        note(f"{kind}: empty etaVec", f, Ys, ps, 9, bag_of=[0, 1, 2, 2], diag_var=True)
        Ys, ps = _sets(pkg, kind, Hh=33)
        note(f"{kind}: H = 33", f, Ys, ps, 9, bag_of=[0, 1, 2, 2], diag_var=True)
        Ys, ps = _sets(pkg, kind)
        note(f"{kind}: niter = 0", f, Ys, ps, 0, bag_of=[0, 1, 2, 2], diag_var=True)
    rng = np.random.default_rng(0)
    Y = rng.standard_normal((6, 4))
    note("fit_restarts", pkg.fit_restarts, Y, 3, 5, diag_var=True)
    note("train_folds", pkg.train_folds, [(Y, Y)], "sparse", 3, 5, diag_var=True)
    note("train_dual_folds: nstarts = 0", pkg.train_dual_folds, [(Y, Y)], 3, 1, 5, diag_var=True, nstarts=0)
    return out


def test_refusals_happen_on_the_host_with_the_recorded_texts(no_device):
    got = _refusal_texts(no_device)
    want = json.load(open(GOLDEN))
    assert got == want
    for case, text in got.items():
        if ":" in case and case.split(":")[0] in BATCH:
            assert text.startswith(BATCH[case.split(":")[0]] + ":") and "one at a time with" in text


def test_fit_restarts_and_train_folds_still_refuse_diag_var(no_device):
    pkg = no_device
    Y = np.random.default_rng(0).standard_normal((6, 4))
    for model in ("sparse", "dual"):
        with pytest.raises(ValueError, match="fit_restarts: diag_var=True is not batched"):
            pkg.fit_restarts(Y, 3, 5, model=model, diag_var=True)
    for solver in ("basic", "sparse"):
        with pytest.raises(ValueError, match="train_folds: diag_var=True is not batched"):
            pkg.train_folds([(Y, Y)], solver, 3, 5, diag_var=True)


# ---- train_dual_folds ----------------------------------------------------------------------------------------------------------------------------
def _dual_scripted(pkg, monkeypatch, norms):
    """replaces vbmf_dual_batch_ by one that leaves on the k-th set AHat and BHat filled with norms[k] (a pair of scalars)"""
    calls = []

    def fake(Ys, params, niter, **kw):
        params = list(params)
        calls.append(dict(Ys=list(Ys), params=params, niter=niter, kw=kw, A0=[p.AHat.copy() for p in params], B0=[p.BHat.copy() for p in params]))
        for p, (a, b) in zip(params, norms):
            p.AHat, p.BHat = a * np.ones_like(p.AHat), b * np.ones_like(p.BHat)
        return [0.5] * len(params)
    monkeypatch.setattr(pkg, "vbmf_dual_batch_", fake)
    return calls


def test_train_dual_folds_draw_order_keep_rule_and_empty_sides(pkg, monkeypatch):
    rng = np.random.default_rng(0)
    Lf = 8
    folds = [(rng.standard_normal((Lf, 4)), rng.standard_normal((Lf, 5))), (rng.standard_normal((Lf, 0)), rng.standard_normal((Lf, 6))),
             (rng.standard_normal((Lf, 3)), rng.standard_normal((Lf, 2)))]
    z = 1e-6                                                        # ones(M, H) z has the operator norm z sqrt(M H)
    # per class three restarts: (fold 0, class 0) keeps its second, (0, 1) none -> the last, (2, 0) its first, (2, 1) its third
    norms = [(z, z), (1.0, z), (1.0, 1.0),   (z, z), (z, z), (z, z),   (z, 1.0), (1.0, 1.0), (z, z),   (z, z), (z, z), (1.0, 1.0)]
    calls = _dual_scripted(pkg, monkeypatch, norms)
    out = pkg.train_dual_folds(folds, 3, 1, 40, diag_var=True, nstarts=3, rng=np.random.default_rng(5))
    (c,) = calls                                                    # one call for everything
    assert c["niter"] == 40 and c["kw"] == dict(eps=1e-4, full_cov=True, bag_of=[0] * 3 + [1] * 3 + [2] * 3 + [3] * 3, diag_var=True)
    assert [Y.shape[1] for Y in c["Ys"]] == [4, 5, 3, 2] and c["Ys"][0] is folds[0][0] and c["Ys"][3] is folds[2][1]
    g = np.random.default_rng(5)                                    # drawn in the order (fold, class, restart) from the one generator
    for k, (b, A0, B0) in enumerate(zip(c["kw"]["bag_of"], c["A0"], c["B0"])):
        q = pkg.vbmf_dual_init(c["Ys"][b], 3, 1, rng=g)
        assert np.array_equal(A0, q.AHat) and np.array_equal(B0, q.BHat) and c["params"][k].H0 == 1
    ps = c["params"]
    assert out[1] == (0, 0)                                         # an empty side
    assert out[0][0] is ps[1] and out[0][1] is ps[5] and out[2][0] is ps[6] and out[2][1] is ps[11]
    # without diag_var the keyword is not passed; nothing to fit -> no call
    calls = _dual_scripted(pkg, monkeypatch, norms)
    pkg.train_dual_folds(folds[:1], 3, 1, 40, eps=1e-5, nstarts=2, rng=np.random.default_rng(5))
    assert calls[0]["kw"] == dict(eps=1e-5, full_cov=True, bag_of=[0, 0, 1, 1])
    calls = _dual_scripted(pkg, monkeypatch, norms)
    assert pkg.train_dual_folds(folds[1:2], 3, 1, 40) == [(0, 0)] and not calls
