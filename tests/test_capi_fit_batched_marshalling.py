"""The ctypes layer of the whole-fit batched calls (capi.Context.fit_batched, sparse_fit_batched, local_fit_batched) against a
library written in Python: a Context made without __init__, whose _lib holds three callables in place of vbmf_fit_batched[_form],
vbmf_sparse_fit_batched and vbmf_local_fit_batched.  The fake reads every argument back through its pointer at the length the C ABI
gives it (include/vbmf_hip.h), records it and fills every output buffer with values of its own; the tests check position and value
of every argument, the per-fit column-major BHat, that inputs are copied, which optional outputs are NULL, and the returned
dictionary.  No GPU, no library."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as G

L, H = 5, 3
COL_OFF = [0, 3, 4, 6]                       # bags of 3, 1 and 2 columns
FIT_BAG = [2, 0, 2, 1]                       # a bag twice, not sorted
WIDTHS = [2, 3, 2, 1]
NB, NF, MH = 3, 4, 8 * H
HANDLE = 0x5EED


def _spec(entry, nf, MH, niter):
    """(name, kind, length) per argument, in the ABI's order.  kind: val (by value), i64 / f64 (read), io (read and written), o64 /
    oi64 (written: doubles / int64)."""
    head = [("ctx", "val"), ("nbags", "val"), ("col_off", "i64", NB + 1), ("nfits", "val"), ("fit_bag", "i64", nf), ("niter", "val"),
            ("eps", "val")]
    tail = [("iters", "oi64", nf), ("d", "o64", nf), ("status", "oi64", nf), ("trace", "o64", nf * niter * 2)]
    if entry.startswith("vbmf_fit_batched"):
        form = [("form", "val"), ("form_used", "oi64", nf)] if entry.endswith("_form") else []
        return head + [("est_covs", "val"), ("est_var", "val"), ("BHat", "io", nf * L * H), ("SigmaB", "io", nf * H * H), ("CA", "io", nf * H),
                       ("CB", "io", nf * H), ("sigma2", "io", nf), ("AHat", "o64", MH), ("SigmaA", "o64", nf * H * H)] + tail + form
    local = [("M0", "i64", nf), ("mask_H1", "val")] if entry == "vbmf_local_fit_batched" else []
    width = 9 if local else 4
    return (head + [("full_cov", "val"), ("est_cb", "val"), ("est_priors", "val"), ("H0", "val")] + local
            + [("gamma", "f64", nf), ("delta0", "f64", nf), ("eta", "f64", nf), ("zeta0", "f64", nf), ("priors", "io", nf * width),
               ("BHat", "io", nf * L * H), ("SigmaB", "io", nf * H * H), ("CB", "io", nf * H), ("sigmaHat", "io", nf), ("CA", "io", MH),
               ("delta", "o64", nf * H), ("zeta", "o64", nf), ("beta", "o64", MH), ("diagSigmaATVec", "o64", MH), ("SigmaA", "o64", nf * H * H),
               ("ATVecHat", "o64", MH)] + tail)


def written(pos, n):
    """What the fake writes into the buffer at argument position pos."""
    return (pos + 1) * 1000.0 + np.arange(n)


class FakeLib:
    def __init__(self):
        self.calls = []
        for entry in ("vbmf_fit_batched", "vbmf_fit_batched_form", "vbmf_sparse_fit_batched", "vbmf_local_fit_batched"):
            setattr(self, entry, self._entry(entry))

    def vbmf_destroy(self, h):
        pass

    def _entry(self, entry):
        def call(*args):
            nf, niter = args[3], args[5]
            fb = np.ctypeslib.as_array(args[4], shape=(nf,))
            off = np.ctypeslib.as_array(args[2], shape=(args[1] + 1,))
            spec = _spec(entry, nf, int(np.sum(off[fb + 1] - off[fb])) * H, niter)
            assert len(args) == len(spec), (entry, len(args), len(spec))
            seen, where = {}, {}
            for pos, (a, (name, kind, *n)) in enumerate(zip(args, spec)):
                if kind == "val" or a is None:
                    assert kind in ("val", "o64"), f"{name} is NULL"             # only outputs are optional
                    seen[name] = a
                    continue
                assert isinstance(a, C.POINTER(C.c_int64 if kind in ("i64", "oi64") else C.c_double)), (name, type(a))
                view = np.ctypeslib.as_array(a, shape=(n[0],))
                where[name] = (C.addressof(a.contents), view.nbytes)
                if kind in ("i64", "f64", "io"):
                    seen[name] = view.copy()
                if kind in ("io", "o64", "oi64"):
                    view[:] = written(pos, n[0])
            self.calls.append((entry, seen, where, [s[0] for s in spec]))
            return 0
        return call


@pytest.fixture
def ctx():
    pkg = G.load_package()
    c = pkg.capi.Context.__new__(pkg.capi.Context)
    c.L, c.M, c.H, c._h, c._lib = L, COL_OFF[-1], H, C.c_void_p(HANDLE), FakeLib()
    return c


def _inputs(seed=0):
    rng = np.random.default_rng(seed)
    r = lambda *s: rng.standard_normal(s)
    return dict(BHat=r(NF, L, H), SigmaB=r(NF, H, H), CA_diag=r(NF, H), CB=r(NF, H), sigma=r(NF), CA=r(MH), gamma=r(NF), delta0=r(NF),
                eta=r(NF), zeta0=r(NF), priors4=r(NF, 4), priors9=r(NF, 9), M0=[1, 3, 0, 1])


def _pos(names, name):
    return names.index(name)


def _no_aliasing(where, inputs):
    """No buffer the library was given lies in memory the caller owns, and no two of them overlap."""
    spans = sorted(where.values())
    assert all(a + n <= b for (a, n), (b, _) in zip(spans, spans[1:]))
    for v in inputs.values():
        if isinstance(v, np.ndarray):
            lo, hi = np.byte_bounds(v) if hasattr(np, "byte_bounds") else np.lib.array_utils.byte_bounds(v)
            assert all(a + n <= lo or a >= hi for a, n in spans)


def _common(seen, niter, eps):
    assert seen["ctx"].value == HANDLE and (seen["nbags"], seen["nfits"], seen["niter"], seen["eps"]) == (NB, NF, niter, eps)
    assert type(seen["niter"]) is int and type(seen["eps"]) is float
    assert np.array_equal(seen["col_off"], COL_OFF) and np.array_equal(seen["fit_bag"], FIT_BAG)


def _per_fit_outputs(r, names, niter, want_trace):
    assert np.array_equal(r["iters"], written(_pos(names, "iters"), NF)) and r["iters"].dtype == np.int64
    assert np.array_equal(r["status"], written(_pos(names, "status"), NF)) and r["status"].dtype == np.int64
    assert np.array_equal(r["d"], written(_pos(names, "d"), NF))
    if want_trace:
        assert np.array_equal(r["trace"], written(_pos(names, "trace"), NF * niter * 2).reshape(NF, niter, 2))
    else:
        assert r["trace"] is None


def _B_out(names):
    """BHat as the library wrote it: per fit column-major, so fit f's entry (l, h) is at f L H + h L + l."""
    return written(_pos(names, "BHat"), NF * L * H).reshape(NF, H, L).transpose(0, 2, 1)


@pytest.mark.parametrize("form", ["stream", "gram", "auto"])
@pytest.mark.parametrize("want_trace", [False, True])
@pytest.mark.parametrize("want_A", [True, False])
def test_fit_batched(ctx, form, want_trace, want_A):
    x = _inputs()
    before = {k: np.copy(v) for k, v in x.items()}
    r = ctx.fit_batched(COL_OFF, FIT_BAG, 7, 1e-3, x["BHat"], x["SigmaB"], x["CA_diag"], x["CB"], x["sigma"], est_covs=True, est_var=False,
                        want_trace=want_trace, form=form, want_A=want_A)
    (entry, seen, where, names), = ctx._lib.calls
    assert entry == ("vbmf_fit_batched" if form == "stream" else "vbmf_fit_batched_form")
    _common(seen, 7, 1e-3)
    assert (seen["est_covs"], seen["est_var"]) == (1, 0)
    if form != "stream":
        assert seen["form"] == dict(gram=1, auto=2)[form]
    assert np.array_equal(seen["BHat"].reshape(NF, H, L), x["BHat"].transpose(0, 2, 1))          # per fit column-major
    assert np.array_equal(seen["SigmaB"], x["SigmaB"].reshape(-1)) and np.array_equal(seen["CA"], x["CA_diag"].reshape(-1))
    assert np.array_equal(seen["CB"], x["CB"].reshape(-1)) and np.array_equal(seen["sigma2"], x["sigma"])
    assert (seen.get("AHat", 0) is None) == (not want_A) and (seen.get("trace", 0) is None) == (not want_trace)
    assert "SigmaA" in where
    _no_aliasing(where, x)
    assert all(np.array_equal(x[k], before[k]) for k in x)
    assert sorted(r) == sorted(["BHat", "SigmaB", "CA", "CB", "sigma2", "SigmaA", "AHat", "iters", "d", "status", "trace", "form_used"])
    assert np.array_equal(r["BHat"], _B_out(names))
    for k, shape in (("SigmaB", (NF, H, H)), ("CA", (NF, H)), ("CB", (NF, H)), ("sigma2", (NF,)), ("SigmaA", (NF, H, H))):
        assert np.array_equal(r[k], written(_pos(names, k), int(np.prod(shape))).reshape(shape)), k
    if want_A:
        flat, at = written(_pos(names, "AHat"), MH), 0
        assert len(r["AHat"]) == NF
        for A, m in zip(r["AHat"], WIDTHS):                                                      # column-major M_b x H blocks
            assert A.shape == (m, H) and np.array_equal(A, flat[at:at + m * H].reshape(H, m).T)
            at += m * H
    else:
        assert r["AHat"] is None
    _per_fit_outputs(r, names, 7, want_trace)
    used = written(_pos(names, "form_used"), NF) if form != "stream" else np.zeros(NF)
    assert np.array_equal(r["form_used"], used) and r["form_used"].dtype == np.int64


@pytest.mark.parametrize("local", [False, True])
@pytest.mark.parametrize("est_cb", [True, False])
@pytest.mark.parametrize("want_trace", [False, True])
@pytest.mark.parametrize("six", [False, True])
def test_sparse_and_local_fit_batched(ctx, local, est_cb, want_trace, six):
    x = _inputs()
    before = {k: np.copy(v) for k, v in x.items()}
    lead = (COL_OFF, FIT_BAG, 7, 1e-3, x["gamma"], x["delta0"], x["eta"], x["zeta0"])
    rest = (x["BHat"], x["SigmaB"], x["CB"], x["sigma"], x["CA"])
    kw = dict(H0=2, full_cov=True, est_cb=est_cb, est_priors=True, want_trace=want_trace)
    if local:
        pri = x["priors9"][:, :6] if six else x["priors9"]
        r = ctx.local_fit_batched(*lead, pri, *rest, x["M0"], mask_H1=1, **kw)
    else:
        pri = x["priors4"]
        r = ctx.sparse_fit_batched(*lead, pri, *rest, **kw)
    (entry, seen, where, names), = ctx._lib.calls
    assert entry == ("vbmf_local_fit_batched" if local else "vbmf_sparse_fit_batched")
    _common(seen, 7, 1e-3)
    assert (seen["full_cov"], seen["est_cb"], seen["est_priors"], seen["H0"]) == (1, int(est_cb), 1, 2)
    if local:
        assert np.array_equal(seen["M0"], x["M0"]) and seen["mask_H1"] == 1
        want_pri = np.zeros((NF, 9))
        want_pri[:, :pri.shape[1]] = pri                                                         # (nfits, 6) is padded to nine
    else:
        want_pri = pri
    assert np.array_equal(seen["priors"], want_pri.reshape(-1))
    for k in ("gamma", "delta0", "eta", "zeta0", "CA"):
        assert np.array_equal(seen[k], x[k]), k
    assert np.array_equal(seen["BHat"].reshape(NF, H, L), x["BHat"].transpose(0, 2, 1))          # per fit column-major
    assert np.array_equal(seen["SigmaB"], x["SigmaB"].reshape(-1)) and np.array_equal(seen["CB"], x["CB"].reshape(-1))
    assert np.array_equal(seen["sigmaHat"], x["sigma"])
    assert (seen.get("delta", 0) is None) == (not est_cb) and (seen.get("trace", 0) is None) == (not want_trace)
    assert all(k in where for k in ("zeta", "beta", "diagSigmaATVec", "SigmaA", "ATVecHat"))
    _no_aliasing(where, x)
    assert all(np.array_equal(x[k], before[k]) for k in x)
    key = "priors9" if local else "priors4"
    assert sorted(r) == sorted(["BHat", "SigmaB", "CB", "delta", "sigmaHat", "zeta", key, "CA", "beta", "diagSigmaATVec", "ATVecHat",
                                "SigmaA", "iters", "d", "status", "trace"])
    assert np.array_equal(r["BHat"], _B_out(names))
    shapes = dict(SigmaB=(NF, H, H), CB=(NF, H), sigmaHat=(NF,), zeta=(NF,), CA=(MH,), beta=(MH,), diagSigmaATVec=(MH,), ATVecHat=(MH,),
                  SigmaA=(NF, H, H))
    for k, shape in shapes.items():
        assert np.array_equal(r[k], written(_pos(names, k), int(np.prod(shape))).reshape(shape)), k
    assert np.array_equal(r[key], written(_pos(names, "priors"), want_pri.size).reshape(want_pri.shape))
    if est_cb:
        assert np.array_equal(r["delta"], written(_pos(names, "delta"), NF * H).reshape(NF, H))
    else:
        assert r["delta"] is None
    _per_fit_outputs(r, names, 7, want_trace)


def test_H0_defaults_to_H_and_the_mask_to_none(ctx):
    x = _inputs()
    lead = (COL_OFF, FIT_BAG, 7, 1e-3, x["gamma"], x["delta0"], x["eta"], x["zeta0"])
    rest = (x["BHat"], x["SigmaB"], x["CB"], x["sigma"], x["CA"])
    ctx.sparse_fit_batched(*lead, x["priors4"], *rest)
    ctx.local_fit_batched(*lead, x["priors9"], *rest, x["M0"])
    for _, seen, _, _ in ctx._lib.calls:
        assert (seen["H0"], seen["full_cov"], seen["est_cb"], seen["est_priors"]) == (H, 0, 1, 0) and seen["trace"] is None
    assert ctx._lib.calls[1][1]["mask_H1"] == 0


@pytest.mark.parametrize("method", ["fit_batched", "sparse_fit_batched", "local_fit_batched"])
def test_value_errors(ctx, method):
    x = _inputs()

    def call(fit_bag=FIT_BAG, col_off=COL_OFF, **over):
        y = {**x, **over}
        if method == "fit_batched":
            return ctx.fit_batched(col_off, fit_bag, 7, 1e-3, y["BHat"], y["SigmaB"], y["CA_diag"], y["CB"], y["sigma"])
        lead = (col_off, fit_bag, 7, 1e-3, y["gamma"], y["delta0"], y["eta"], y["zeta0"])
        rest = (y["BHat"], y["SigmaB"], y["CB"], y["sigma"], y["CA"])
        if method == "sparse_fit_batched":
            return ctx.sparse_fit_batched(*lead, y["priors4"], *rest)
        return ctx.local_fit_batched(*lead, y["priors9"], *rest, y["M0"])

    bags = "col_off describes 3 bags: every fit_bag entry must lie in 0..2"
    for bad in ([2, 0, 3, 1], [2, -1, 2, 1]):
        with pytest.raises(ValueError) as e:
            call(fit_bag=bad)
        assert str(e.value) == bags
    with pytest.raises(ValueError) as e:
        call(col_off=[0])
    assert str(e.value) == "col_off describes 0 bags: every fit_bag entry must lie in 0..-1"
    shapes = dict(
        fit_batched="4 fits: SigmaB must be (4, 3, 3), CA and CB (4, 3) and sigma2 (4,)",
        sparse_fit_batched="4 fits: gamma, delta0, eta, zeta0, sigmaHat must be (4,), priors4 (4, 4), SigmaB (4, 3, 3), CB (4, 3) and CA (24,)",
        local_fit_batched="4 fits: gamma, delta0, eta, zeta0, sigmaHat, M0 must be (4,), SigmaB (4, 3, 3), CB (4, 3) and CA (24,)")[method]
    faults = [dict(SigmaB=x["SigmaB"][:, :2, :2]), dict(CB=x["CB"][:3]), dict(sigma=x["sigma"][:3])]
    if method == "fit_batched":
        faults.append(dict(CA_diag=x["CA_diag"][:, :2]))
    else:
        faults += [dict(CA=x["CA"][:-1]), dict(gamma=x["gamma"][:3]), dict(zeta0=np.ones(5))]
    if method == "sparse_fit_batched":
        faults.append(dict(priors4=x["priors9"]))
    if method == "local_fit_batched":
        faults.append(dict(M0=[1, 2]))
    for over in faults:
        with pytest.raises(ValueError) as e:
            call(**over)
        assert str(e.value) == shapes, over.keys()
    if method == "local_fit_batched":
        for pri in (x["priors4"], x["priors9"][:3], x["priors9"].reshape(-1)):
            with pytest.raises(ValueError) as e:
                call(priors9=pri)
            assert str(e.value) == "4 fits: priors9 must be (4, 9) or (4, 6)"
    assert ctx._lib.calls == []                                                                  # refused before the library
