"""One wide ARD-family fit over many workgroups (vbmf_ard_fit_batched_form / vbmf_*_batch_(..., form=..., slice_cols=...) and the
training loops above them): the parts that need no GPU -- the C ABI is declared, exported and bound with the header's constants, the
Julia host binds it, the form and slice_cols arithmetic of capi, Context.ard_fit_batched_form against a library written in Python,
form="split" reaches that entry from every Python host with the right arguments and fills the fields, the host-side refusals, and the
default call path still reaches the older entries."""
import contextlib
import ctypes as C
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


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports(pkg):
    hdr = open(os.path.join(ROOT, "include", "vbmf_hip.h")).read()
    m = re.search(r"int\s+vbmf_ard_fit_batched_form\s*\(([^;]*)\);", hdr)
    rows = re.search(r"int\s+vbmf_rows_fit_batched\s*\(([^;]*)\);", hdr)
    types = lambda s: [re.sub(r"\s*\w+$", "", a.strip()) for a in re.sub(r"/\*.*?\*/", "", s, flags=re.S).split(",")]
    assert m and types(m.group(1))[:33] == types(rows.group(1)) and types(m.group(1))[33:] == ["int", "int64_t", "int64_t", "int64_t*"]
    assert re.search(r"int\s+diag_var\s*,\s*int64_t\s+form\s*,\s*int64_t\s+slice_cols\s*,\s*int64_t\*\s*form_used", m.group(1))
    cap = pkg.capi
    for name in ("VBMF_FIT_FORM_SPLIT", "VBMF_FIT_SPLIT_COLS", "VBMF_FIT_SPLIT_MIN_COLS", "VBMF_FIT_SPLIT_MIN_COLS_FULL", "VBMF_FIT_SPLIT_CHUNK"):
        d = re.search(r"#define\s+" + name + r"\s+(\d+)", hdr)
        assert d and int(d.group(1)) == getattr(cap, name), name
    assert cap.VBMF_FIT_FORM_SPLIT == 3 and cap.VBMF_FIT_SPLIT_COLS % 8 == 0 and cap.VBMF_FIT_SPLIT_COLS >= 8
    assert hasattr(C.CDLL(cap.LIB_PATH), "vbmf_ard_fit_batched_form") and "vbmf_ard_fit_batched_form" in cap.SYMBOLS
    assert cap.lib().vbmf_ard_fit_batched_form.argtypes[:33] == cap.lib().vbmf_rows_fit_batched.argtypes
    assert len(cap.lib().vbmf_ard_fit_batched_form.argtypes) == 37 and hasattr(cap.Context, "ard_fit_batched_form")


def test_julia_host_binds_it():
    jl = open(os.path.join(G.PKG_DIR, "julia", "VBMatrixFactorizationHIP.jl")).read()
    call = re.search(r"ccall\(\(:vbmf_ard_fit_batched_form,\s*libvbmf\),\s*Cint,\s*\((.*?)\),\n", jl, flags=re.S)
    assert call and len([t for t in re.split(r",\s*", call.group(1).replace("\n", " ")) if t.strip()]) == 37
    assert re.search(r"ARD_FIT_FORMS\s*=\s*Dict\(:stream => 0, :auto => 2, :split => 3\)", jl)
    for fn in ("vbmf_sparse_batch!", "vbmf_dual_batch!", "vbmf_trial_batch!", "vbmf_sparse_masked_batch!"):
        sig = re.search(r"function " + re.escape(fn) + r"\((.*?)\)\n", jl, flags=re.S)
        assert sig and re.search(r"form::Symbol\s*=\s*:stream", sig.group(1)) and re.search(r"slice_cols::Int\s*=\s*0", sig.group(1)), fn


# ---- capi's arithmetic --------------------------------------------------------------------------------------------------------------------
def test_form_codes_slice_widths_and_the_auto_rule(pkg):
    cap = pkg.capi
    assert [cap.ard_fit_form_code(f) for f in ("stream", "auto", "split")] == [0, 2, 3]
    with pytest.raises(ValueError, match="vbmf_batch_"):
        cap.ard_fit_form_code("gram")
    for bad in ("Split", "", None, 3):
        with pytest.raises(ValueError, match="'stream', 'split' or 'auto'"):
            cap.ard_fit_form_code(bad)
    assert cap.ard_slice_cols(None) == 0 and cap.ard_slice_cols(0) == 0 and cap.ard_slice_cols(8) == 8 and cap.ard_slice_cols(512) == 512
    for bad in (4, 12, -8, 7):
        with pytest.raises(ValueError, match="multiple of 8"):
            cap.ard_slice_cols(bad)
    sc = cap.VBMF_FIT_SPLIT_COLS
    assert [cap.ard_fit_slices(m) for m in (1, sc - 1, sc, sc + 1, 2 * sc + 3)] == [1, 1, 1, 2, 3]
    assert [cap.ard_fit_slices(m, 8) for m in (8, 9, 21, 70)] == [1, 2, 3, 9]
    for full, wide in ((False, cap.VBMF_FIT_SPLIT_MIN_COLS), (True, cap.VBMF_FIT_SPLIT_MIN_COLS_FULL)):
        assert [cap.ard_fit_form_auto(m, full) for m in (1, wide - 1, wide, wide + 1)] == [0, 0, 3, 3]


# ---- Context.ard_fit_batched_form against a library written in Python -----------------------------------------------------------------------
L, H = 5, 3
COL_OFF, FIT_BAG, HANDLE = [0, 3, 4, 6], [2, 0, 2, 1], 0x5EED
NB, NF, MH = 3, 4, 8 * H


class FakeLib:
    """the entry in Python: records every argument as the C ABI reads it and fills every output with values of its own"""
    NAMES = ("ctx", "nbags", "col_off", "nfits", "fit_bag", "niter", "eps", "full_cov", "est_cb", "est_priors", "H0", "M0", "mask_H1",
             "gamma", "delta0", "etaVec", "zeta0", "priors9", "BHat", "SigmaB", "CB", "sigmaVec", "CA", "delta", "zetaVec", "beta",
             "diagSigmaATVec", "SigmaA", "ATVecHat", "iters", "d", "status", "trace", "diag_var", "form", "slice_cols", "form_used")

    def __init__(self):
        self.calls = []

    def vbmf_destroy(self, h):
        pass

    def vbmf_ard_fit_batched_form(self, *args):
        assert len(args) == len(self.NAMES)
        a = dict(zip(self.NAMES, args))
        nf, niter, nr = a["nfits"], a["niter"], L if a["diag_var"] else 1
        sizes = dict(col_off=a["nbags"] + 1, fit_bag=nf, M0=nf, gamma=nf, delta0=nf, etaVec=nf, zeta0=nf, priors9=nf * 9, BHat=nf * L * H,
                     SigmaB=nf * H * H, CB=nf * H, sigmaVec=nf * nr, CA=MH, delta=nf * H, zetaVec=nf * nr, beta=MH, diagSigmaATVec=MH,
                     SigmaA=nf * H * H, ATVecHat=MH, iters=nf, d=nf, status=nf, trace=nf * niter * 2, form_used=nf)
        seen = {}
        for pos, k in enumerate(self.NAMES):
            v = a[k]
            if k not in sizes or v is None:
                seen[k] = v
                continue
            view = np.ctypeslib.as_array(v, shape=(sizes[k],))
            seen[k] = view.copy()
            if k == "form_used":
                view[:] = 3
            elif pos >= self.NAMES.index("priors9"):
                view[:] = (pos + 1) * 1000 + np.arange(sizes[k])
        self.calls.append(seen)
        return 0


@pytest.fixture
def ctx(pkg):
    c = pkg.capi.Context.__new__(pkg.capi.Context)
    c.L, c.M, c.H, c._h, c._lib = L, COL_OFF[-1], H, C.c_void_p(HANDLE), FakeLib()
    return c


def _inputs(diag_var, seed=0):
    rng = np.random.default_rng(seed)
    r = lambda *s: rng.standard_normal(s)
    return dict(gamma=r(NF), delta0=r(NF), eta=r(NF), zeta0=r(NF), priors9=r(NF, 9), BHat=r(NF, L, H), SigmaB=r(NF, H, H), CB=r(NF, H),
                sigma=r(NF, L) if diag_var else r(NF), CA=r(MH))


@pytest.mark.parametrize("diag_var", [False, True])
@pytest.mark.parametrize("m0", [None, [1, 3, 0, 1]])
def test_context_marshals_the_entry(ctx, m0, diag_var):
    x = _inputs(diag_var)
    keep = {k: v.copy() for k, v in x.items()}
    r = ctx.ard_fit_batched_form(COL_OFF, FIT_BAG, 7, 1e-3, x["gamma"], x["delta0"], x["eta"], x["zeta0"], x["priors9"], x["BHat"],
                                 x["SigmaB"], x["CB"], x["sigma"], x["CA"], M0=m0, H0=2, full_cov=True, est_priors=True, want_trace=True,
                                 diag_var=diag_var, form="split", slice_cols=16)
    (s,) = ctx._lib.calls
    assert s["ctx"].value == HANDLE and (s["nbags"], s["nfits"], s["niter"], s["eps"]) == (NB, NF, 7, 1e-3)
    assert (s["full_cov"], s["est_cb"], s["est_priors"], s["H0"], s["mask_H1"]) == (1, 1, 1, 2, 0)
    assert (s["diag_var"], s["form"], s["slice_cols"]) == (int(diag_var), 3, 16)
    assert s["M0"] is None if m0 is None else np.array_equal(s["M0"], m0)               # None goes down as NULL: M0[f] = M_b
    for k in ("gamma", "delta0", "zeta0", "CB", "CA", "SigmaB", "priors9"):
        assert np.array_equal(s[k], keep[k].reshape(-1)), k
    assert np.array_equal(s["etaVec"], keep["eta"]) and np.array_equal(s["sigmaVec"], keep["sigma"].reshape(-1))
    assert np.array_equal(s["BHat"].reshape(NF, H, L), keep["BHat"].transpose(0, 2, 1))  # per fit column-major
    assert all(np.array_equal(x[k], keep[k]) for k in x)                                # the caller's arrays are copied, not written
    pos = FakeLib.NAMES.index
    sk, zk = ("sigmaVecHat", "zetaVec") if diag_var else ("sigmaHat", "zeta")
    shape = (NF, L) if diag_var else (NF,)
    assert r[sk].shape == shape and r[zk].shape == shape
    assert np.array_equal(r[sk].ravel(), (pos("sigmaVec") + 1) * 1000 + np.arange(r[sk].size))
    assert r["priors9"].shape == (NF, 9) and r["trace"].shape == (NF, 7, 2) and list(r["form_used"]) == [3] * NF
    r = ctx.ard_fit_batched_form(COL_OFF, FIT_BAG, 7, 1e-3, x["gamma"], x["delta0"], x["eta"], x["zeta0"], x["priors9"][:, :6], x["BHat"],
                                 x["SigmaB"], x["CB"], x["sigma"], x["CA"], diag_var=diag_var, form="auto", est_cb=False)
    s = ctx._lib.calls[-1]
    assert (s["form"], s["slice_cols"], s["H0"]) == (2, 0, H) and s["delta"] is None and s["trace"] is None
    assert np.all(s["priors9"].reshape(NF, 9)[:, 6:] == 0.0)
    n = len(ctx._lib.calls)
    for kw, word in ((dict(form="gram"), "vbmf_batch_"), (dict(form="fast"), "'stream', 'split' or 'auto'"), (dict(slice_cols=12), "multiple of 8")):
        with pytest.raises(ValueError, match=word):
            ctx.ard_fit_batched_form(COL_OFF, FIT_BAG, 7, 1e-3, x["gamma"], x["delta0"], x["eta"], x["zeta0"], x["priors9"], x["BHat"],
                                     x["SigmaB"], x["CB"], x["sigma"], x["CA"], diag_var=diag_var, **kw)
    assert len(ctx._lib.calls) == n                                 # refused before the library is touched


# ---- the Python hosts on a scripted context ----------------------------------------------------------------------------------------------------
class ScriptedCtx:
    """stands where SparseBags.ctx stands: records the one call, answers with values that name their field and fit"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name.endswith("_fit_batched") or name == "ard_fit_batched_form":
            def call(*a, **kw):
                self.calls.append((name, a, kw))
                return self._answer(name, a, kw)
            return call
        raise AttributeError(name)

    def _answer(self, name, a, kw):
        col_off, bag_of, B = np.asarray(a[0]), list(a[1]), np.asarray(a[9])
        nf, Lr, Hr = B.shape
        mh = sum(int(col_off[b + 1] - col_off[b]) for b in bag_of) * Hr
        fill = lambda base, *shape: base + np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape)
        pri = np.tile(np.arange(1.0, 10.0), (nf, 1)) + 10.0 * np.arange(nf)[:, None]
        rows = name == "rows_fit_batched" or kw.get("diag_var")
        noise = dict(sigmaVecHat=fill(500.0, nf, Lr), zetaVec=fill(600.0, nf, Lr)) if rows else dict(sigmaHat=fill(500.0, nf), zeta=fill(600.0, nf))
        pris = {"priors4": pri[:, :4]} if name == "sparse_fit_batched" else {"priors9": pri}
        used = dict(form_used=np.array([3, 0] * nf)[:nf]) if name == "ard_fit_batched_form" else {}
        return dict(BHat=fill(100.0, nf, Lr, Hr), SigmaB=fill(200.0, nf, Hr, Hr), CB=fill(300.0, nf, Hr), delta=fill(400.0, nf, Hr),
                    CA=fill(700.0, mh), beta=fill(800.0, mh), diagSigmaATVec=fill(900.0, mh), ATVecHat=fill(1000.0, mh),
                    SigmaA=fill(1100.0, nf, Hr, Hr), iters=np.arange(3, 3 + nf), d=0.25 + np.arange(nf), status=np.arange(nf) % 2,
                    trace=None, **noise, **pris, **used)


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
BATCH = dict(sparse="vbmf_sparse_batch_", dual="vbmf_dual_batch_", trial="vbmf_trial_batch_", masked="vbmf_sparse_masked_batch_")
OLD = dict(sparse="sparse_fit_batched", dual="sparse_fit_batched", trial="local_fit_batched", masked="local_fit_batched")


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


@pytest.mark.parametrize("diag_var", [False, True])
@pytest.mark.parametrize("kind", list(BATCH))
def test_form_reaches_the_entry_and_fills_the_fields(pkg, scripted, kind, diag_var):
    Hh, bag_of = 4, [0, 1, 2, 2]
    Ys, ps = _sets(pkg, kind)
    for k, p in enumerate(ps):
        p.sigmaVecHat = 0.1 * (k + 1) + np.arange(p.L)
    sg0, sv0 = [p.sigmaHat for p in ps], [p.sigmaVecHat.copy() for p in ps]
    extra = dict(est_priors=True) if kind in ("dual", "trial") else {}
    ds = getattr(pkg, BATCH[kind])(Ys, ps, 9, eps=1e-3, full_cov=(kind == "dual"), bag_of=bag_of, form="split", slice_cols=16,
                                   **(dict(diag_var=True) if diag_var else {}), **extra)
    ((name, a, kw),) = scripted.calls
    assert name == "ard_fit_batched_form"
    col_off, bo, niter, eps, gamma, delta0, eta, zeta0, pri, B, SB, CB, sg, CA, M0 = a
    assert list(bo) == bag_of and (niter, eps) == (9, 1e-3)
    assert (kw["form"], kw["slice_cols"], bool(kw["diag_var"])) == ("split", 16, diag_var)
    if diag_var:
        assert list(eta) == [p.eta0 + p.M / 2 for p in ps] and np.array_equal(np.asarray(sg), np.stack(sv0))
    else:
        assert list(eta) == [p.eta0 + p.L * p.M / 2 for p in ps] and list(sg) == sg0
    assert (list(M0) == [M0S[b] for b in bag_of]) if kind in ("trial", "masked") else M0 is None
    assert kw["H0"] == (Hh if kind in ("sparse", "masked") else 1) and kw["mask_H1"] == (2 if kind == "masked" else 0)
    assert kw["full_cov"] == (kind == "dual") and bool(kw["est_priors"]) == (kind in ("dual", "trial"))
    assert np.shape(pri) == (4, 6)                                  # nine-slot priors in either noise model
    assert ds == [0.25, 1.25, 2.25, 3.25]
    for k, p in enumerate(ps):
        assert p.form == (3, 0)[k % 2] and p.iters == 3 + k and p.status == k % 2
        if diag_var:
            assert np.array_equal(p.sigmaVecHat, 500.0 + k * p.L + np.arange(p.L)) and p.sigmaHat == sg0[k]
        else:
            assert p.sigmaHat == 500.0 + k and np.array_equal(p.sigmaVecHat, sv0[k])
        row = 10.0 * k + np.arange(1.0, 10.0)
        if kind == "dual":                                          # slots 0-3 the pairs, 6 and 7 the posterior shapes
            assert [p.alpha00, p.beta00, p.alpha01, p.beta01] == list(row[:4]) and (p.alpha0, p.alpha1) == (row[6], row[7])
        if kind == "trial":
            assert [getattr(p, n_) for n_ in pkg.capi.Context.TRIAL_KEYS] == list(row)


@pytest.mark.parametrize("kind", list(BATCH))
def test_the_default_call_still_reaches_the_older_entries(pkg, scripted, kind):
    Ys, ps = _sets(pkg, kind)
    getattr(pkg, BATCH[kind])(Ys, ps, 9, bag_of=[0, 1, 2, 2])
    getattr(pkg, BATCH[kind])(Ys, ps, 9, bag_of=[0, 1, 2, 2], form="stream", slice_cols=None)
    getattr(pkg, BATCH[kind])(Ys, ps, 9, bag_of=[0, 1, 2, 2], diag_var=True)
    assert [c[0] for c in scripted.calls] == [OLD[kind], OLD[kind], "rows_fit_batched"]
    assert all("form" not in c[2] and "slice_cols" not in c[2] for c in scripted.calls)
    assert all(p.form == 0 for p in ps)
    getattr(pkg, BATCH[kind])(Ys, ps, 9, bag_of=[0, 1, 2, 2], form="auto")
    assert scripted.calls[-1][0] == "ard_fit_batched_form" and scripted.calls[-1][2]["form"] == "auto"
    assert scripted.calls[-1][2]["slice_cols"] is None


@pytest.mark.parametrize("kind", list(BATCH))
def test_host_refusals_come_before_the_device(pkg, scripted, kind):
    Ys, ps = _sets(pkg, kind)
    for kw, word in ((dict(form="gram"), "vbmf_batch_"), (dict(form="wide"), "'stream', 'split' or 'auto'"),
                     (dict(form="split", slice_cols=12), "multiple of 8"), (dict(slice_cols=-8), "multiple of 8")):
        with pytest.raises(ValueError, match=word):
            getattr(pkg, BATCH[kind])(Ys, ps, 9, bag_of=[0, 1, 2, 2], **kw)
    assert scripted.calls == []


def test_training_loops_hand_the_form_down(pkg, scripted):
    rng = np.random.default_rng(0)
    Ls, Hh = 6, 3
    folds = [(rng.standard_normal((Ls, 3)), rng.standard_normal((Ls, 4))), (rng.standard_normal((Ls, 2)), rng.standard_normal((Ls, 5)))]
    sent = lambda: (scripted.calls[-1][0], scripted.calls[-1][2].get("form"), scripted.calls[-1][2].get("slice_cols"))
    pkg.train_local_folds(folds, Hh, 1, 5, rng=np.random.default_rng(1), form="split", slice_cols=8)
    assert sent() == ("ard_fit_batched_form", "split", 8)
    pkg.train_dual_folds(folds, Hh, 1, 5, nstarts=2, rng=np.random.default_rng(1), form="auto")
    assert sent() == ("ard_fit_batched_form", "auto", None)
    pkg.train_folds(folds, "sparse", Hh, 5, rng=np.random.default_rng(1), form="split")
    assert sent() == ("ard_fit_batched_form", "split", None)
    pkg.fit_restarts(folds[0][1], Hh, 5, nstarts=2, rng=np.random.default_rng(1), form="split", slice_cols=16)
    assert sent() == ("ard_fit_batched_form", "split", 16)
    pkg.fit_restarts(folds[0][1], Hh, 5, model="dual", H0=1, nstarts=2, rng=np.random.default_rng(1), form="split")
    assert sent() == ("ard_fit_batched_form", "split", None)
    n = len(scripted.calls)
    pkg.train_local_folds(folds, Hh, 1, 5, rng=np.random.default_rng(1))                # the defaults: the older entries
    pkg.train_dual_folds(folds, Hh, 1, 5, nstarts=2, rng=np.random.default_rng(1))
    pkg.train_folds(folds, "sparse", Hh, 5, rng=np.random.default_rng(1))
    assert [c[0] for c in scripted.calls[n:]] == ["local_fit_batched", "sparse_fit_batched", "sparse_fit_batched"]
    n = len(scripted.calls)
    for call in (lambda: pkg.train_local_folds(folds, Hh, 1, 5, form="gram"), lambda: pkg.train_dual_folds(folds, Hh, 1, 5, form="gram"),
                 lambda: pkg.train_folds(folds, "sparse", Hh, 5, form="gram"), lambda: pkg.fit_restarts(folds[0][1], Hh, 5, form="gram")):
        with pytest.raises(ValueError, match="vbmf_batch_"):
            call()
    with pytest.raises(ValueError):
        pkg.train_folds(folds, "basic", Hh, 5, form="split")        # the basic model's forms are vbmf_batch_'s
    assert len(scripted.calls) == n
