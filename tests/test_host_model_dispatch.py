"""What the Python host sends to the device for the ARD-sparse model and its grouped siblings (vbmf_dual, vbmf_trial), and for
the basic model's paths that share code with them: the package's Context is replaced by a recorder that logs every method call
with its bound arguments and returns deterministic results.  Each case checks the full call sequence and every field written
back to params (and that no other field changed).  The whole-fit batched calls (vbmf_sparse_batch_, vbmf_dual_batch_,
vbmf_trial_batch_, vbmf_sparse_masked_batch_, vbmf_batch_) and their callers are covered the same way.  No GPU and no library are
needed."""
import copy
import inspect
from dataclasses import fields

import numpy as np
import pytest

import __graft_entry__ as G

L, M, H, H0, M0 = 6, 5, 4, 2, 3
MODELS = ("sparse", "dual", "trial")
PREFIX = dict(sparse="sparse_", dual="dual_", trial="trial_")
HYPER = dict(sparse=("alpha0", "beta0"), dual=("alpha00", "beta00"), trial=("alpha01", "beta01"))
SHAPES = dict(sparse=(), dual=("alpha0", "alpha1"), trial=("alpha1", "alpha2", "alpha3"))


@pytest.fixture(scope="module")
def pkg():
    return G.load_package()


def _frozen(v):
    if isinstance(v, np.ndarray):
        return v.copy()
    if isinstance(v, dict):
        return {k: _frozen(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return type(v)(_frozen(x) for x in v)
    return v


class Call:
    def __init__(self, cid, name, args, ret=None):
        self.cid, self.name, self.args, self.ret = cid, name, args, ret

    def __repr__(self):
        return f"Call({self.cid}, {self.name})"


def bound(pkg, cid, name, *a, **k):
    """The call as the real Context method would receive it: arguments bound to its signature, defaults applied."""
    b = inspect.signature(getattr(pkg.capi.Context, name)).bind(None, *a, **k)
    b.apply_defaults()
    return Call(cid, name, {n: _frozen(v) for n, v in list(b.arguments.items())[1:]})


class Recorder:
    """Stands in for capi.Context.  Every value it returns is distinct (a running serial number), positive and exact in fp64."""
    log, serial, runs, count = [], 0, 0, 0
    fit_iters = fit_status = fit_d = None

    def __init__(self, *a, **k):
        self.L, self.M, self.H = a[:3]
        self.cid = Recorder.count
        Recorder.count += 1
        self.log.append(bound(G.load_package(), self.cid, "__init__", *a, **k))

    def v(self, *shape):
        Recorder.serial += 1
        n = int(np.prod(shape))
        return np.asfortranarray(((Recorder.serial * 1000 + 1 + np.arange(n)) / 8.0).reshape(shape))

    def s(self):
        return float(self.v(1)[0])

    def _run(self, a):
        done = a["niter"] if Recorder.runs == 0 else a["niter"] - 1      # a second run stops one sweep short
        Recorder.runs += 1
        return done, 0.5 ** Recorder.runs, None


def _returns(c, name, a):
    nb = len(a["col_off"]) - 1 if "col_off" in a else 0
    MH = c.M * c.H
    if name == "get_state":
        return dict(AHat=c.v(c.M, c.H), BHat=c.v(c.L, c.H) if a["want_B"] else None, SigmaA=c.v(c.H, c.H), SigmaB=c.v(c.H, c.H),
                    CA_diag=c.v(c.H), CB_diag=c.v(c.H), sigma2=c.s())
    if name == "sparse_get_state":
        return dict(ATVecHat=c.v(MH), diagSigmaATVec=c.v(MH), CA=c.v(MH), beta=c.v(MH), SigmaA_diag=c.v(c.H),
                    BHat=c.v(c.L, c.H) if a["want_B"] else None, SigmaB=c.v(c.H, c.H), CB=c.v(c.H), delta=c.v(c.H),
                    sigmaHat=c.s(), zeta=c.s())
    if name in ("run", "sparse_run", "dual_run", "trial_run"):
        return c._run(a)
    if name == "run_fixed_basis_batched":
        return dict(sigma2=c.v(nb), CA_diag=c.v(nb, c.H), SigmaA=c.v(nb, c.H, c.H), AHat=c.v(c.M, c.H) if a["want_A"] else None)
    if name == "sparse_run_fixed_basis_batched":
        return dict(sigmaHat=c.v(nb), zeta=c.v(nb), CA=c.v(MH), beta=c.v(MH), diagSigmaATVec=c.v(MH), ATVecHat=c.v(MH),
                    SigmaA=c.v(nb, c.H, c.H))
    if name == "YHat":
        return c.v(c.L, c.M)
    if name in ("elbo", "sparse_lower_bound", "sparse_lower_bound_trimmed"):
        return c.s()
    if name == "sparse_get_noise_rows":
        return c.v(c.L).ravel(), c.v(c.L).ravel()
    if name == "sparse_get_SigmaA":
        return c.v(c.H, c.H)
    if name == "row_gram":
        return c.v(nb, c.L, c.L)
    if name in ("fit_batched", "sparse_fit_batched", "local_fit_batched"):
        return _fit_returns(c, name, a)
    if name == "dual_get_priors":
        pr = c.v(6).ravel()
        return H0, dict(alpha00=pr[0], beta00=pr[1], alpha01=pr[2], beta01=pr[3], alpha0=pr[4], alpha1=pr[5])
    if name == "trial_get_priors":
        pr = c.v(9).ravel()
        return H0, M0, {k: float(pr[i]) for i, k in enumerate(c.TRIAL_KEYS)}
    return None


def _fit_returns(c, name, a):
    """The whole-fit batched calls: the shapes capi.Context documents.  iters, status and d are 3 + f, 0 and distinct values unless the
    test scripts them through Recorder.fit_iters / fit_status / fit_d."""
    fb = np.asarray(a["fit_bag"])
    Ms = np.asarray(a["col_off"])[fb + 1] - np.asarray(a["col_off"])[fb]
    nf, Hc = fb.size, c.H
    MH = int(Ms.sum()) * Hc
    scripted = lambda v, default: np.asarray(default if v is None else v)
    out = dict(BHat=c.v(nf, c.L, Hc), SigmaB=c.v(nf, Hc, Hc), SigmaA=c.v(nf, Hc, Hc), iters=scripted(Recorder.fit_iters, 3 + np.arange(nf)),
               d=scripted(Recorder.fit_d, c.v(nf)), status=scripted(Recorder.fit_status, np.zeros(nf, dtype=np.int64)),
               trace=c.v(nf, a["niter"], 2) if a["want_trace"] else None)
    if name == "fit_batched":
        used = dict(stream=np.zeros(nf), gram=np.ones(nf), auto=np.arange(nf) % 2)[a["form"]].astype(np.int64)
        out.update(CA=c.v(nf, Hc), CB=c.v(nf, Hc), sigma2=c.v(nf), AHat=[c.v(m, Hc) for m in Ms] if a["want_A"] else None, form_used=used)
    else:
        width = 4 if name == "sparse_fit_batched" else 9
        out.update({f"priors{width}": c.v(nf, width)}, CB=c.v(nf, Hc), delta=c.v(nf, Hc) if a["est_cb"] else None, sigmaHat=c.v(nf),
                   zeta=c.v(nf), CA=c.v(MH), beta=c.v(MH), diagSigmaATVec=c.v(MH), ATVecHat=c.v(MH))
    return out


def _method(name):
    def call(self, *a, **k):
        e = bound(G.load_package(), self.cid, name, *a, **k)
        self.log.append(e)
        e.ret = _returns(self, name, e.args)
        return e.ret
    return call


for _name in ("set_Y", "close", "set_state", "get_state", "step", "run", "run_fixed_basis", "run_fixed_basis_batched", "YHat",
              "elbo", "sparse_set_state", "sparse_get_state", "sparse_step", "sparse_run", "sparse_run_fixed_basis",
              "sparse_run_fixed_basis_batched", "sparse_set_noise_rows", "sparse_get_noise_rows", "sparse_set_full_cov",
              "sparse_set_SigmaA", "sparse_get_SigmaA", "sparse_lower_bound", "sparse_lower_bound_trimmed", "dual_set_priors",
              "dual_get_priors", "dual_run", "trial_set_priors", "trial_get_priors", "trial_run", "fit_batched", "sparse_fit_batched",
              "local_fit_batched", "row_gram"):
    setattr(Recorder, _name, _method(_name))


@pytest.fixture
def rec(pkg, monkeypatch):
    """The recorder in place of Context, empty session caches, and the log writers as stubs that log too."""
    Recorder.log, Recorder.serial, Recorder.runs, Recorder.count = [], 0, 0, 0
    Recorder.fit_iters = Recorder.fit_status = Recorder.fit_d = None
    Recorder.TRIAL_KEYS = pkg.capi.Context.TRIAL_KEYS
    monkeypatch.setattr(pkg, "Context", Recorder)
    monkeypatch.setattr(pkg, "_sessions", {})
    monkeypatch.setattr(pkg, "_sparse_sessions", {})
    marker = object()

    def create_log(params):
        Recorder.log.append(Call(None, "create_log", dict(params=copy.deepcopy(params))))
        return marker

    def update_log_(logVar, params):
        assert logVar is marker
        Recorder.log.append(Call(None, "update_log_", dict(params=copy.deepcopy(params))))

    def save_log(logVar, Y, priors, logdir, desc=""):
        assert logVar is marker
        Recorder.log.append(Call(None, "save_log", dict(Y=Y, priors=priors, logdir=logdir, desc=desc)))

    monkeypatch.setattr(pkg, "create_log", create_log)
    monkeypatch.setattr(pkg, "update_log_", update_log_)
    monkeypatch.setattr(pkg, "save_log", save_log)
    return Recorder.log


# ---- comparisons -----------------------------------------------------------------------------------------------------------------
def same(a, b):
    if isinstance(a, dict) or isinstance(b, dict):
        return isinstance(a, dict) and isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, (np.ndarray, list, tuple)) or isinstance(b, (np.ndarray, list, tuple)):
        a, b = np.asarray(a), np.asarray(b)
        return a.shape == b.shape and np.array_equal(a, b)
    return a == b


def check_calls(log, want):
    assert [(c.cid, c.name) for c in log] == [(w.cid, w.name) for w in want]
    for c, w in zip(log, want):
        assert c.args.keys() == w.args.keys(), c
        for k in w.args:
            if c.name in ("create_log", "update_log_"):
                continue
            assert same(c.args[k], w.args[k]), (c, k, c.args[k], w.args[k])


def check_fields(p, p0, written):
    """Fields in `written` hold those values, every other field is unchanged, no two array fields share memory."""
    assert set(written) <= {f.name for f in fields(p)}, set(written) - {f.name for f in fields(p)}
    for f in fields(p):
        want = written[f.name] if f.name in written else getattr(p0, f.name)
        got = getattr(p, f.name)
        if f.name == "YHat" and want is not None and got is not None:
            np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-9)
        else:
            assert same(got, want), (f.name, got, want)
    arrays = [(f.name, getattr(p, f.name)) for f in fields(p) if isinstance(getattr(p, f.name), np.ndarray)]
    for i, (n1, a1) in enumerate(arrays):
        for n2, a2 in arrays[i + 1:]:
            assert not np.shares_memory(a1, a2), (n1, n2)


# ---- parameter sets --------------------------------------------------------------------------------------------------------------
def make(pkg, model, seed=0, Lr=L, Mr=M):
    rng = np.random.default_rng(seed)
    Y = rng.standard_normal((Lr, Mr))
    if model == "sparse":
        p = pkg.vbmf_sparse_init(Y, H, alpha0=0.1, beta0=0.2, gamma0=0.3, delta0=0.4, eta0=0.5, zeta0=0.6, labels=[2, Mr], H1=1,
                                 rng=rng)
    elif model == "dual":
        p = pkg.vbmf_dual_init(Y, H, H0, alpha0=0.1, beta0=0.2, gamma0=0.3, delta0=0.4, eta0=0.5, zeta0=0.6, rng=rng)
        p.alpha00, p.beta00, p.alpha01, p.beta01 = 0.15, 0.25, 0.35, 0.45
        p.alpha0, p.alpha1 = 0.65, 0.85
        p.alpha = np.array([p.alpha0, p.alpha1])
    elif model == "trial":
        p = pkg.vbmf_trial_init(Y, H, H0, M0, alpha0=0.1, beta0=0.2, gamma0=0.3, delta0=0.4, eta0=0.5, zeta0=0.6, rng=rng)
        for g, (a, b) in enumerate(((0.15, 0.25), (0.35, 0.45), (0.55, 0.65)), start=1):
            setattr(p, f"alpha0{g}", a)
            setattr(p, f"beta0{g}", b)
            setattr(p, f"alpha{g}", a + 0.5)
        p.alpha = np.array([p.alpha1, p.alpha2, p.alpha3])
    else:
        p = pkg.vbmf_init(Y, H, ca=0.5, cb=0.7, sigma2=0.9, rng=rng)
        p.SigmaA, p.SigmaB = rng.standard_normal((H, H)), rng.standard_normal((H, H))
        return Y, p
    p.SigmaA = rng.standard_normal((H, H))
    p.sigmaVecHat, p.zetaVec = 1.0 + np.arange(Lr) / 4.0, 2.0 + np.arange(Lr) / 8.0
    p.CA = p.CA + np.arange(p.CA.size) / 16.0
    p.beta = p.beta + np.arange(p.beta.size) / 32.0
    return Y, p


def variant(pkg, model, diag_var):
    name = f"VBMF_VARIANT_{model.upper()}_{'DIAGVAR' if diag_var else 'DIAG'}"
    return getattr(pkg, name) if hasattr(pkg, name) else getattr(pkg.capi, name)


def open_ctx(pkg, cid, model, Y, diag_var=False):
    out = [bound(pkg, cid, "__init__", L, M, H, variant=variant(pkg, model, diag_var), **pkg._defaults)]
    if Y is not None:
        out.append(bound(pkg, cid, "set_Y", Y))
    return out


def want_push(pkg, cid, model, p, diag_var=False, full_cov=False):
    a0, b0 = HYPER[model]
    hyper = dict(alpha0=getattr(p, a0), beta0=getattr(p, b0), gamma0=p.gamma0, delta0=p.delta0, eta0=p.eta0, zeta0=p.zeta0)
    lab = dict(labels0=np.asarray(p.labels) - 1, H1=p.H1) if model == "sparse" else {}
    out = [bound(pkg, cid, "sparse_set_state", p.ATVecHat, p.diagSigmaATVec, p.CA, p.beta, p.BHat, p.SigmaB, p.CB, p.delta,
                 p.sigmaHat, p.zeta, hyper, **lab)]
    if model == "dual":
        out.append(bound(pkg, cid, "dual_set_priors", p.H0, p.alpha00, p.beta00, p.alpha01, p.beta01, p.alpha0, p.alpha1))
    if model == "trial":
        out.append(bound(pkg, cid, "trial_set_priors", p.H0, p.M0, {k: getattr(p, k) for k in pkg.capi.Context.TRIAL_KEYS}))
    out.append(bound(pkg, cid, "sparse_set_full_cov", full_cov))
    if p.SigmaA is not None:
        out.append(bound(pkg, cid, "sparse_set_SigmaA", p.SigmaA))
    if diag_var:
        out.append(bound(pkg, cid, "sparse_set_noise_rows", p.sigmaVecHat, p.zetaVec, float(p.etaVec[0])))
    return out


def want_pull(pkg, cid, model, diag_var=False):
    out = [bound(pkg, cid, "sparse_get_state")]
    if diag_var:
        out.append(bound(pkg, cid, "sparse_get_noise_rows"))
    out.append(bound(pkg, cid, "sparse_get_SigmaA"))
    if model in ("dual", "trial"):
        out.append(bound(pkg, cid, f"{model}_get_priors"))
    return out


def views(model, p, A, CA, beta):
    """The per-group copies of AHat / CA / beta (src/vbmf_dual.jl:146-165, src/vbmf_trial.jl)."""
    m, h0 = p.M, getattr(p, "H0", 0)
    blocks = dict(dual=((slice(None), slice(0, h0)), (slice(None), slice(h0, None))),
                  trial=((slice(None), slice(0, h0)), (slice(0, getattr(p, "M0", 0)), slice(h0, None)),
                         (slice(getattr(p, "M0", 0), None), slice(h0, None)))).get(model, ())
    names = dict(dual=(("A0Hat", "CA0", "beta0"), ("A1Hat", "CA1", "beta1")),
                 trial=(("A1Hat", "CA1", "beta1"), ("A2Hat", "CA2", "beta2"), ("A3Hat", "CA3", "beta3"))).get(model, ())
    out = {}
    for blk, (a, c, b) in zip(blocks, names):
        out[a] = A[blk]
        out[c] = CA.reshape(m, H)[blk].reshape(-1)
        out[b] = beta.reshape(m, H)[blk].reshape(-1)
    return out


def pulled(model, p0, calls, diag_var=False):
    """The fields one pull writes, from the recorder's results of the calls want_pull lists."""
    it = iter(c.ret for c in calls)
    s = next(it)
    w = {k: s[k] for k in ("ATVecHat", "diagSigmaATVec", "CA", "beta", "BHat", "SigmaB", "CB", "delta")}
    if diag_var:
        w["sigmaVecHat"], w["zetaVec"] = next(it)
    else:
        w["sigmaHat"], w["zeta"] = s["sigmaHat"], s["zeta"]
    w["SigmaA"] = next(it)
    w["AHat"] = s["ATVecHat"].reshape(p0.M, H)
    w.update(views(model, p0, w["AHat"], w["CA"], w["beta"]))
    if model != "sparse":
        pr = next(it)[-1]
        w.update({k: float(v) for k, v in pr.items()})
        w["alpha"] = [pr[k] for k in SHAPES[model]]
    return w


def with_yhat(w):
    w["YHat"] = w["BHat"] @ w["AHat"].T
    return w


# ---- the step-wise updates -------------------------------------------------------------------------------------------------------
UPDATES = [("updateA_", "SSTEP_A", "Y", {}), ("updateA_", "SSTEP_A", "Y", dict(full_cov=True)),
           ("updateA_", "SSTEP_A", "Y", dict(diag_var=True)), ("updateA_", "SSTEP_A", "Y", dict(full_cov=True, diag_var=True)),
           ("updateB_", "SSTEP_B", "Y", {}), ("updateB_", "SSTEP_B", "Y", dict(diag_var=True)),
           ("updateSigma_", "SSTEP_SIGMA", "Y", {}), ("updateSigma_", "SSTEP_SIGMA", "Y", dict(diag_var=True)),
           ("updateCA_", "SSTEP_CA", None, {}), ("updateCA_", "SSTEP_CA", "kw", {}),
           ("updateCB_", "SSTEP_CB", None, {}), ("updateCB_", "SSTEP_CB", "kw", {}),
           ("updateCA_and_priors_", "SSTEP_CA|SSTEP_PRIORS", None, {}), ("updateCA_and_priors_", "SSTEP_CA|SSTEP_PRIORS", "kw", {})]


@pytest.mark.parametrize("model,fn,which,how,kw", [(m,) + u for m in MODELS for u in UPDATES
                                                    if not (m == "sparse" and u[0] == "updateCA_and_priors_")])
@pytest.mark.parametrize("no_SigmaA", [False, True])
def test_updates(pkg, rec, model, fn, which, how, kw, no_SigmaA):
    Y, p = make(pkg, model)
    if no_SigmaA:
        p.SigmaA = None
    p0 = copy.deepcopy(p)
    f = getattr(pkg, PREFIX[model] + fn)
    if how == "Y":
        f(Y, p, **kw)
    elif how == "kw":
        f(p, Y=Y)
    else:
        f(p)
    step = 0
    for w in which.split("|"):
        step |= getattr(pkg, w)
    dv = kw.get("diag_var", False)
    want = open_ctx(pkg, 0, model, None if how is None else Y, dv) + want_push(pkg, 0, model, p0, dv, kw.get("full_cov", False))
    want += [bound(pkg, 0, "sparse_step", step)] + want_pull(pkg, 0, model, dv)
    check_calls(rec, want)
    check_fields(p, p0, pulled(model, p0, rec[-len(want_pull(pkg, 0, model, dv)):], dv))


# ---- vbmf_sparse! / vbmf_dual! / vbmf_trial! ---------------------------------------------------------------------------------------
RUNS = [dict(), dict(diag_var=True), dict(full_cov=True), dict(diag_var=True, full_cov=True),
        dict(logdir="out", desc="d1", log_every=3, eps=1e-4, est_cb=False, est_priors=False),
        dict(logdir="out", log_every=3, diag_var=True)]


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("kw", RUNS)
@pytest.mark.parametrize("verb", [False, True])
def test_runs(pkg, rec, capsys, model, kw, verb):
    kw = dict(kw)
    if model == "sparse":
        kw.pop("est_priors", None)
    Y, p = make(pkg, model)
    p0 = copy.deepcopy(p)
    niter = 8
    d = getattr(pkg, f"vbmf_{model}_")(Y, p, niter, verb=verb, **kw)
    dv, eps = kw.get("diag_var", False), kw.get("eps", 1e-6)
    run_kw = dict(eps=eps, est_cb=kw.get("est_cb", True))
    if model != "sparse":
        run_kw["est_priors"] = kw.get("est_priors", True)
    run = "sparse_run" if model == "sparse" else f"{model}_run"
    pull = want_pull(pkg, 0, model, dv)
    want = open_ctx(pkg, 0, model, Y, dv) + want_push(pkg, 0, model, p0, dv, kw.get("full_cov", False))
    if "logdir" in kw:
        want += [Call(None, "create_log", dict(params=None))]
        for k in (3, 3):                                    # the second chunk stops one sweep short: the loop ends there
            want += [bound(pkg, 0, run, k, **run_kw)] + pull + [Call(None, "update_log_", dict(params=None))]
        want += [Call(None, "save_log", dict(Y=Y, priors={}, logdir="out", desc=kw.get("desc", "")))]
        iters, d_want = 5, 0.25
    else:
        want += [bound(pkg, 0, run, niter, **run_kw)] + pull
        iters, d_want = niter, 0.5
    check_calls(rec, want)
    assert d == d_want and p._last_run == (iters, d_want)
    last = [i for i, c in enumerate(rec) if c.name == "sparse_get_state"][-1]
    check_fields(p, p0, with_yhat(pulled(model, p0, rec[last:last + len(pull)], dv)))
    if "logdir" in kw:
        logged = [c.args["params"] for c in rec if c.name in ("create_log", "update_log_")]
        assert same(logged[0].ATVecHat, p0.ATVecHat) and same(logged[-1].ATVecHat, p.ATVecHat)
        first = [i for i, c in enumerate(rec) if c.name == "sparse_get_state"][0]
        assert same(logged[1].ATVecHat, rec[first].ret["ATVecHat"])
    out = capsys.readouterr().out
    assert out == (f"Factorization finished after {iters} iterations, eps = {d_want}\n" if verb else "")


@pytest.mark.parametrize("model", MODELS)
def test_deep_copy_wrappers(pkg, rec, model):
    Y, p = make(pkg, model)
    p0 = copy.deepcopy(p)
    q, d = getattr(pkg, f"vbmf_{model}")(Y, p, 4, diag_var=True, est_cb=False)
    assert q is not p and d == 0.5 and q._last_run == (4, 0.5)
    check_fields(p, p0, {})
    assert rec[-len(want_pull(pkg, 0, model, True)) - 1].args["est_cb"] is False


# ---- bounds ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_bounds(pkg, rec, model):
    Y, p = make(pkg, model)
    p0 = copy.deepcopy(p)
    lb = getattr(pkg, dict(sparse="lowerBound", dual="lowerBound_dual", trial="lowerBound_trial")[model])(Y, p, clamp=False)
    lbt = pkg.lowerBoundTrimmed(Y, p, 0.3, clamp=False)
    lbd = pkg.lowerBoundTrimmed(Y, p)
    push = want_push(pkg, 0, model, p0)
    want = (open_ctx(pkg, 0, model, Y) + push + [bound(pkg, 0, "sparse_lower_bound", clamp=False)]
            + push + [bound(pkg, 0, "sparse_lower_bound_trimmed", 0.3, clamp=False)]
            + push + [bound(pkg, 0, "sparse_lower_bound_trimmed")])
    check_calls(rec, want)
    assert [lb, lbt, lbd] == [c.ret for c in rec if c.name.startswith("sparse_lower_bound")]
    check_fields(p, p0, {})


# ---- vbls! -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("kw", [dict(), dict(diag_var=True), dict(full_cov=True), dict(diag_var=True, full_cov=True)])
def test_vbls(pkg, rec, model, kw):
    Y, p = make(pkg, model)
    p0 = copy.deepcopy(p)
    A = pkg.vbls_(Y, p, 7, **kw)
    dv = kw.get("diag_var", False)
    pull = want_pull(pkg, 0, model, dv)
    want = (open_ctx(pkg, 0, model, Y, dv) + want_push(pkg, 0, model, p0, dv, kw.get("full_cov", False))
            + [bound(pkg, 0, "sparse_run_fixed_basis", 7)] + pull)
    check_calls(rec, want)
    check_fields(p, p0, with_yhat(pulled(model, p0, rec[-len(pull):], dv)))
    assert A is p.AHat


def _basic_push(pkg, cid, p):
    return bound(pkg, cid, "set_state", p.AHat, p.BHat, p.SigmaA, p.SigmaB, np.diag(p.CA), np.diag(p.CB), p.sigma2,
                 labels0=np.asarray(p.labels) - 1, H1=p.H1)


def _basic_pulled(p0, s, yhat):
    ca, cb = p0.CA.copy(), p0.CB.copy()
    np.fill_diagonal(ca, s["CA_diag"])
    np.fill_diagonal(cb, s["CB_diag"])
    return dict(AHat=s["AHat"], BHat=s["BHat"], SigmaA=s["SigmaA"], SigmaB=s["SigmaB"], CA=ca, CB=cb,
                invCA=np.diag(1.0 / s["CA_diag"]), invCB=np.diag(1.0 / s["CB_diag"]), sigma2=s["sigma2"], YHat=yhat)


def test_vbls_basic(pkg, rec):
    Y, p = make(pkg, "basic")
    p0 = copy.deepcopy(p)
    CA = p.CA
    A = pkg.vbls_(Y, p, 7)
    want = [bound(pkg, 0, "__init__", L, M, H, **pkg._defaults), bound(pkg, 0, "set_Y", Y), _basic_push(pkg, 0, p0),
            bound(pkg, 0, "run_fixed_basis", 7), bound(pkg, 0, "get_state"), bound(pkg, 0, "YHat")]
    check_calls(rec, want)
    check_fields(p, p0, _basic_pulled(p0, rec[-2].ret, rec[-1].ret))
    assert A is p.AHat and p.CA is CA


@pytest.mark.parametrize("logged", [False, True])
def test_vbmf_basic(pkg, rec, capsys, logged):
    Y, p = make(pkg, "basic")
    p0 = copy.deepcopy(p)
    kw = dict(logdir="out", desc="b", log_every=3) if logged else {}
    r = pkg.vbmf_(Y, p, 8, eps=1e-5, est_covs=True, est_var=True, verb=True, **kw)
    run_kw = dict(eps=1e-5, est_covs=True, est_var=True)
    want = [bound(pkg, 0, "__init__", L, M, H, **pkg._defaults), bound(pkg, 0, "set_Y", Y), _basic_push(pkg, 0, p0)]
    if logged:
        want += [Call(None, "create_log", dict(params=None))]
        for k in (3, 3):
            want += [bound(pkg, 0, "run", k, **run_kw), bound(pkg, 0, "get_state"), Call(None, "update_log_", dict(params=None))]
        iters, d = 5, 0.25
    else:
        want += [bound(pkg, 0, "run", 8, **run_kw), bound(pkg, 0, "get_state")]
        iters, d = 8, 0.5
    want += [bound(pkg, 0, "YHat")]
    if logged:
        want += [Call(None, "save_log", dict(Y=Y, priors={}, logdir="out", desc="b"))]
    check_calls(rec, want)
    assert r is p and p._last_run == (iters, d)
    s = [c for c in rec if c.name == "get_state"][-1].ret
    check_fields(p, p0, _basic_pulled(p0, s, [c for c in rec if c.name == "YHat"][0].ret))
    saving = "Saving outputs and inputs under out/\n" if logged else ""
    assert capsys.readouterr().out == f"Factorization finished after {iters} iterations, eps = {d}\n" + saving


# ---- batched vbls! ---------------------------------------------------------------------------------------------------------------
def _bags(pkg, model, Ms=(3, 1, 2)):
    rng = np.random.default_rng(5)
    Ys = [rng.standard_normal((L, m)) for m in Ms]
    _, res = make(pkg, model, seed=9)
    ps = []
    for Y in Ys:
        q = pkg.copy_vbmf_params(Y, res, rng=np.random.default_rng(1))
        ps.append(q[0] if isinstance(q, tuple) else q)
    for b, p in enumerate(ps):
        if model == "basic":
            p.sigma2 = 0.5 + b
            p.CA = p.CA * (1.0 + b)
        else:
            p.sigmaHat = 0.5 + b
            p.CA = p.CA + b + np.arange(p.CA.size) / 16.0
    Yall = np.concatenate(Ys, axis=1)
    col_off = np.concatenate([[0], np.cumsum(Ms)])
    return Ys, ps, Yall, col_off


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("full_cov", [False, True])
@pytest.mark.parametrize("prebuilt", [False, True])
def test_vbls_sparse_batch(pkg, rec, model, full_cov, prebuilt):
    Ys, ps, Yall, col_off = _bags(pkg, model)
    p0s = copy.deepcopy(ps)
    bags = pkg.SparseBags(Ys, H) if prebuilt else Ys
    out = pkg.vbls_sparse_batch_(bags, ps, 9, full_cov=full_cov)
    q = p0s[0]
    nM = int(col_off[-1])
    zero = np.zeros(nM * H)
    hyper = dict(alpha0=1e-10, beta0=1e-10, gamma0=q.gamma0, delta0=q.delta0, eta0=q.eta0, zeta0=q.zeta0)
    first, second = dict(sparse=(("alpha0", "beta0"), ("alpha0", "beta0")), dual=(("alpha00", "beta00"), ("alpha01", "beta01")),
                         trial=(("alpha01", "beta01"), ("alpha02", "beta02")))[model]
    h0 = H if model == "sparse" else H0
    alpha = [[getattr(p, first[0] if h < h0 else second[0]) + 0.5 for h in range(H)] for p in p0s]
    beta0 = [[getattr(p, first[1] if h < h0 else second[1]) for h in range(H)] for p in p0s]
    want = [bound(pkg, 0, "__init__", L, nM, H, variant=pkg.VBMF_VARIANT_SPARSE_DIAG, **pkg._defaults), bound(pkg, 0, "set_Y", Yall),
            bound(pkg, 0, "sparse_set_state", zero, zero + 1, zero + 1, zero + 1, q.BHat, q.SigmaB, np.ones(H), np.ones(H), 1.0, 0.0,
                  hyper),
            bound(pkg, 0, "sparse_run_fixed_basis_batched", col_off, 9, alpha, beta0, [p.eta0 + p.L * p.M / 2 for p in p0s],
                  [p.zeta0 for p in p0s], [p.sigmaHat for p in p0s], np.concatenate([p.CA for p in p0s]), full_cov=full_cov)]
    if not prebuilt:
        want.append(bound(pkg, 0, "close"))
    check_calls(rec, want)
    r = rec[3].ret
    for b, (p, p0) in enumerate(zip(ps, p0s)):
        s0, s1 = col_off[b] * H, col_off[b + 1] * H
        w = dict(ATVecHat=r["ATVecHat"][s0:s1], diagSigmaATVec=r["diagSigmaATVec"][s0:s1], CA=r["CA"][s0:s1], beta=r["beta"][s0:s1],
                 SigmaA=r["SigmaA"][b], sigmaHat=r["sigmaHat"][b], zeta=r["zeta"][b])
        w["AHat"] = w["ATVecHat"].reshape(p0.M, H)
        w.update(views(model, p0, w["AHat"], w["CA"], w["beta"]))
        if model != "sparse":
            hyp = dict(dual=("alpha00", "alpha01"), trial=("alpha01", "alpha02", "alpha03"))[model]
            for a, h in zip(SHAPES[model], hyp):
                w[a] = getattr(p0, h) + 0.5
            w["alpha"] = [w[a] for a in SHAPES[model]]
        w["YHat"] = p0.BHat @ w["AHat"].T
        check_fields(p, p0, w)
        assert out[b] is p.AHat


@pytest.mark.parametrize("prebuilt", [False, True])
def test_vbls_basic_batch(pkg, rec, prebuilt):
    Ys, ps, Yall, col_off = _bags(pkg, "basic")
    p0s = copy.deepcopy(ps)
    CAs = [p.CA for p in ps]
    bags = pkg.Bags(Ys, H) if prebuilt else Ys
    out = pkg.vbls_batch_(bags, ps, 9)
    q = p0s[0]
    nM = int(col_off[-1])
    want = [bound(pkg, 0, "__init__", L, nM, H, **pkg._defaults), bound(pkg, 0, "set_Y", Yall),
            bound(pkg, 0, "set_state", np.zeros((nM, H)), q.BHat, q.SigmaA, q.SigmaB, np.diag(q.CA), np.diag(q.CB), q.sigma2),
            bound(pkg, 0, "run_fixed_basis_batched", col_off, 9, [p.sigma2 for p in p0s], [np.diag(p.CA) for p in p0s])]
    check_calls(rec, want)
    r = rec[3].ret
    for b, (p, p0) in enumerate(zip(ps, p0s)):
        ca = p0.CA.copy()
        np.fill_diagonal(ca, r["CA_diag"][b])
        A = r["AHat"][col_off[b]:col_off[b + 1]]
        check_fields(p, p0, dict(AHat=A, SigmaA=r["SigmaA"][b], CA=ca, invCA=np.diag(1.0 / r["CA_diag"][b]),
                                 sigma2=r["sigma2"][b], YHat=p0.BHat @ A.T))
        assert out[b] is p.AHat and p.CA is CAs[b]


# ---- the session cache of the sparse models --------------------------------------------------------------------------------------
def test_sparse_ctx_cache(pkg, rec):
    Y, ps = make(pkg, "sparse")
    _, pd = make(pkg, "dual")
    _, pt = make(pkg, "trial")
    kinds = {}

    def opened():
        return [(c.cid, c.name) for c in rec if c.name in ("__init__", "set_Y", "close", "sparse_step")]

    pkg.sparse_updateB_(Y, ps, diag_var=True)                  # ctx 0 holds Y (diagonal-noise-rows variant)
    pkg.sparse_updateCA_(ps)                                   # no Y: ctx 0 serves whatever its diag_var
    pkg.dual_updateCA_(pd)                                     # no dual context: ctx 1 holds no matrix, ctx 0 stays
    pkg.dual_updateCB_(pd)                                     # ctx 1 again
    pkg.trial_updateCA_(pt)                                    # ctx 2 replaces ctx 1 in the slot without a matrix
    pkg.sparse_updateB_(Y, ps)                                 # another diag_var: ctx 3 evicts ctx 0, ctx 2 stays
    pkg.sparse_updateCA_(ps, Y=Y)                              # ctx 3
    Y *= 2.0                                                   # same array, new contents: uploaded again into ctx 3
    pkg.sparse_updateCB_(ps, Y=Y)
    pkg.sparse_updateCA_(ps)                                   # no Y: ctx 3 (ctx 2 is a trial context)
    pkg.trial_updateB_(Y, pt)                                  # ctx 4 evicts ctx 3, ctx 2 stays
    pkg.trial_updateCB_(pt)                                    # no Y: the first trial context cached, ctx 2
    for c in rec:
        if c.name == "__init__":
            kinds[c.cid] = (c.args["variant"], c.args["L"], c.args["M"], c.args["H"])
    assert opened() == [(0, "__init__"), (0, "set_Y"), (0, "sparse_step"),
                        (0, "sparse_step"),
                        (1, "__init__"), (1, "sparse_step"),
                        (1, "sparse_step"),
                        (1, "close"), (2, "__init__"), (2, "sparse_step"),
                        (0, "close"), (3, "__init__"), (3, "set_Y"), (3, "sparse_step"),
                        (3, "sparse_step"),
                        (3, "set_Y"), (3, "sparse_step"),
                        (3, "sparse_step"),
                        (3, "close"), (4, "__init__"), (4, "set_Y"), (4, "sparse_step"),
                        (2, "sparse_step")]
    assert kinds == {0: (pkg.VBMF_VARIANT_SPARSE_DIAGVAR, L, M, H), 1: (pkg.VBMF_VARIANT_DUAL_DIAG, L, M, H),
                     2: (pkg.VBMF_VARIANT_TRIAL_DIAG, L, M, H), 3: (pkg.VBMF_VARIANT_SPARSE_DIAG, L, M, H),
                     4: (pkg.VBMF_VARIANT_TRIAL_DIAG, L, M, H)}
    n = len(opened())
    pkg.invalidate(Y)                                          # Y's context and the one without a matrix
    assert opened()[n:] == [(2, "close"), (4, "close")]
    pkg.invalidate()
    assert len(opened()) == n + 2


# ---- whole fits, many in one device call -----------------------------------------------------------------------------------------
BAG_OF = [2, 0, 2, 1]                       # a bag twice, not sorted
FIT_M0 = (1, 3, 0, 1)                       # per fit: inside its bag, all of it, none of it
FIT_FN = dict(sparse="vbmf_sparse_batch_", dual="vbmf_dual_batch_", trial="vbmf_trial_batch_", masked="vbmf_sparse_masked_batch_")
FIT_GROUPS = dict(sparse=(("alpha0", "beta0"),) * 2, dual=(("alpha00", "beta00"), ("alpha01", "beta01")),
                  trial=(("alpha01", "beta01"), ("alpha02", "beta02"), ("alpha03", "beta03")), masked=(("alpha0", "beta0"),) * 3)


def _fit_sets(pkg, model, Ms, h0=H0, bag_of=BAG_OF):
    """Bags of unequal width and one parameter set per entry of bag_of, no two alike in anything the device call is given."""
    rng = np.random.default_rng(11)
    Ys = [rng.standard_normal((L, m)) for m in Ms]
    hyp = lambda f: dict(gamma0=0.3 + f, delta0=0.4 + f, eta0=0.5 + f, zeta0=0.6 + f)
    ps = []
    for f, b in enumerate(bag_of):
        m0 = min(FIT_M0[f], Ms[b])
        if model == "basic":
            p = pkg.vbmf_init(Ys[b], H, ca=0.5 + f, cb=0.7 + f, sigma2=0.9 + f, rng=rng)
            p.SigmaB = rng.standard_normal((H, H))
            p.CA, p.CB = p.CA + np.diag(np.arange(H) / 4.0) + 0.125, p.CB + np.diag(np.arange(H) / 8.0) + 0.25   # off-diagonals too
            ps.append(p)
            continue
        if model == "sparse":
            p = pkg.vbmf_sparse_init(Ys[b], H, alpha0=0.1 + f, beta0=0.2 + f, rng=rng, **hyp(f))
        elif model == "masked":
            p = pkg.vbmf_sparse_init(Ys[b], H, alpha0=0.1 + f, beta0=0.2 + f, H1=1, labels=np.arange(1, m0 + 1), rng=rng, **hyp(f))
        elif model == "dual":
            p = pkg.vbmf_dual_init(Ys[b], H, h0, rng=rng, **hyp(f))
            p.alpha00, p.beta00, p.alpha01, p.beta01 = 0.15 + f, 0.25 + f, 0.35 + f, 0.45 + f
        else:
            p = pkg.vbmf_trial_init(Ys[b], H, h0, m0, rng=rng, **hyp(f))
            for g in (1, 2, 3):
                setattr(p, f"alpha0{g}", 0.1 * g + f)
                setattr(p, f"beta0{g}", 0.2 * g + f)
        p.SigmaB = rng.standard_normal((H, H))
        p.CB, p.sigmaHat = p.CB + np.arange(H) / 4.0 + f, 1.5 + f
        p.CA = p.CA + f + np.arange(p.CA.size) / 16.0
        ps.append(p)
    return Ys, ps, np.concatenate(Ys, axis=1), np.concatenate([[0], np.cumsum(Ms)])


def _open_bags(pkg, cid, model, Yall):
    kw = {} if model == "basic" else dict(variant=pkg.VBMF_VARIANT_SPARSE_DIAG)
    return [bound(pkg, cid, "__init__", L, Yall.shape[1], H, **kw, **pkg._defaults), bound(pkg, cid, "set_Y", Yall)]


def _want_sparse_family_call(pkg, model, p0s, col_off, niter, eps, full_cov, est_cb, est_priors, bag_of=BAG_OF):
    common = (col_off, bag_of, niter, eps, [p.gamma0 + p.L / 2 for p in p0s], [p.delta0 for p in p0s],
              [p.eta0 + p.L * p.M / 2 for p in p0s], [p.zeta0 for p in p0s],
              [[getattr(p, k) for pair in FIT_GROUPS[model] for k in pair] for p in p0s],
              [p.BHat for p in p0s], [p.SigmaB for p in p0s], [p.CB for p in p0s], [p.sigmaHat for p in p0s],
              np.concatenate([p.CA for p in p0s]))
    grouped = model in ("dual", "trial")
    kw = dict(H0=p0s[0].H0 if grouped else H, full_cov=full_cov, est_cb=est_cb, est_priors=est_priors and grouped)
    if model in ("sparse", "dual"):
        return bound(pkg, 0, "sparse_fit_batched", *common, **kw)
    M0s = [p.M0 if model == "trial" else len(p.labels) for p in p0s]
    return bound(pkg, 0, "local_fit_batched", *common, M0s, mask_H1=1 if model == "masked" else 0, **kw)


def _sparse_family_written(model, p0, r, f, s0, est_cb, est_priors):
    s1 = s0 + p0.M * H
    w = {k: r[k][s0:s1] for k in ("ATVecHat", "diagSigmaATVec", "CA", "beta")}
    w.update(AHat=w["ATVecHat"].reshape(p0.M, H), SigmaA=r["SigmaA"][f], BHat=r["BHat"][f], SigmaB=r["SigmaB"][f], CB=r["CB"][f],
             sigmaHat=r["sigmaHat"][f], zeta=r["zeta"][f])
    if est_cb:
        w["delta"] = r["delta"][f]
    if model in ("dual", "trial"):
        w.update(views(model, p0, w["AHat"], w["CA"], w["beta"]))
    if model == "dual":
        # the posterior shapes of the last updateCA!: read back from CA * beta where est_priors refitted them and the fit ran and
        # ended well, else the start values' (src/vbmf_dual.jl:324-325)
        ok = est_priors and r["iters"][f] > 0 and r["status"][f] == 0
        w["alpha0"] = w["CA0"][0] * w["beta0"][0] if ok else p0.alpha00 + 0.5
        w["alpha1"] = w["CA1"][0] * w["beta1"][0] if ok and w["CA1"].size else p0.alpha01 + 0.5
        w["alpha00"], w["beta00"], w["alpha01"], w["beta01"] = r["priors4"][f]
    if model == "trial":
        w.update(zip(("alpha01", "beta01", "alpha02", "beta02", "alpha03", "beta03", "alpha1", "alpha2", "alpha3"), r["priors9"][f]))
    if model in ("dual", "trial"):
        w["alpha"] = [w[a] for a in SHAPES[model]]
    w["YHat"] = w["BHat"] @ w["AHat"].T
    return w


@pytest.mark.parametrize("model,h0,est_priors", [("sparse", H0, True), ("masked", H0, True)]      # (these two have no est_priors)
                         + [(m, h, e) for m, h in (("dual", H0), ("dual", H), ("trial", H0), ("trial", 0)) for e in (True, False)])
@pytest.mark.parametrize("full_cov", [False, True])
@pytest.mark.parametrize("est_cb", [True, False])
@pytest.mark.parametrize("prebuilt", [False, True])
def test_fit_batch_sparse_family(pkg, rec, model, h0, full_cov, est_cb, est_priors, prebuilt):
    grouped = model in ("dual", "trial")
    Ys, ps, Yall, col_off = _fit_sets(pkg, model, (3, 1, 2) if full_cov else (3, 2, 4), h0)   # (the diagonal form needs M >= 2)
    p0s = copy.deepcopy(ps)
    Recorder.fit_iters, Recorder.fit_status = [5, 0, 7, 6], [0, 0, 1, 0]      # one fit that never ran, one that stopped on a bad value
    bags = pkg.SparseBags(Ys, H) if prebuilt else Ys
    kw = dict(est_priors=est_priors) if grouped else {}
    ds = getattr(pkg, FIT_FN[model])(bags, ps, 9, eps=1e-3, full_cov=full_cov, est_cb=est_cb, bag_of=list(BAG_OF), **kw)
    want = _open_bags(pkg, 0, model, Yall) + [_want_sparse_family_call(pkg, model, p0s, col_off, 9, 1e-3, full_cov, est_cb, est_priors)]
    if not prebuilt:
        want.append(bound(pkg, 0, "close"))
    check_calls(rec, want)
    r = rec[2].ret
    assert ds == [float(v) for v in r["d"]] and all(type(v) is float for v in ds)
    s0 = 0
    for f, (p, p0) in enumerate(zip(ps, p0s)):
        check_fields(p, p0, _sparse_family_written(model, p0, r, f, s0, est_cb, est_priors))
        assert (p.iters, p.status) == (Recorder.fit_iters[f], Recorder.fit_status[f])
        assert type(p.iters) is int and type(p.status) is int and type(p.sigmaHat) is float and type(p.zeta) is float
        assert p.BHat.flags.f_contiguous
        s0 += p0.M * H


@pytest.mark.parametrize("model", ["sparse", "dual", "trial", "masked", "basic"])
def test_fit_batch_defaults(pkg, rec, model):
    """bag_of left out: fit f on bag f; eps, full_cov, est_cb, est_priors and form at their defaults."""
    Ys, ps, Yall, col_off = _fit_sets(pkg, model, (3, 2, 4), bag_of=[0, 1, 2])
    p0s = copy.deepcopy(ps)
    if model == "basic":
        pkg.vbmf_batch_(Ys, ps, 4)
        want = _want_basic_call(pkg, p0s, col_off, 4, 1e-6, False, False, "stream", bag_of=[0, 1, 2])
    else:
        getattr(pkg, FIT_FN[model])(Ys, ps, 4)
        want = _want_sparse_family_call(pkg, model, p0s, col_off, 4, 1e-6, False, True, True, bag_of=[0, 1, 2])
    check_calls(rec, _open_bags(pkg, 0, model, Yall) + [want, bound(pkg, 0, "close")])


def _want_basic_call(pkg, p0s, col_off, niter, eps, est_covs, est_var, form, bag_of=BAG_OF):
    return bound(pkg, 0, "fit_batched", col_off, bag_of, niter, eps, [p.BHat for p in p0s], [p.SigmaB for p in p0s],
                 [np.diag(p.CA) for p in p0s], [np.diag(p.CB) for p in p0s], [p.sigma2 for p in p0s], est_covs=est_covs, est_var=est_var,
                 form=form)


@pytest.mark.parametrize("form", ["stream", "gram", "auto"])
@pytest.mark.parametrize("est", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("prebuilt", [False, True])
def test_fit_batch_basic(pkg, rec, form, est, prebuilt):
    Ys, ps, Yall, col_off = _fit_sets(pkg, "basic", (3, 1, 2))
    p0s = copy.deepcopy(ps)
    CAs, CBs = [p.CA for p in ps], [p.CB for p in ps]
    Recorder.fit_iters, Recorder.fit_status = [5, 0, 7, 6], [0, 0, 1, 0]
    bags = pkg.Bags(Ys, H) if prebuilt else Ys
    out = pkg.vbmf_batch_(bags, ps, 9, eps=1e-3, est_covs=est[0], est_var=est[1], bag_of=list(BAG_OF), form=form)
    want = _open_bags(pkg, 0, "basic", Yall) + [_want_basic_call(pkg, p0s, col_off, 9, 1e-3, est[0], est[1], form)]
    if not prebuilt:
        want.append(bound(pkg, 0, "close"))
    check_calls(rec, want)
    r = rec[2].ret
    assert len(out) == len(ps) and all(a is b for a, b in zip(out, ps))
    for f, (p, p0) in enumerate(zip(ps, p0s)):
        ca, cb = p0.CA.copy(), p0.CB.copy()
        np.fill_diagonal(ca, r["CA"][f])
        np.fill_diagonal(cb, r["CB"][f])
        check_fields(p, p0, dict(AHat=r["AHat"][f], BHat=r["BHat"][f], SigmaA=r["SigmaA"][f], SigmaB=r["SigmaB"][f], CA=ca, CB=cb,
                                 invCA=np.diag(1.0 / r["CA"][f]), invCB=np.diag(1.0 / r["CB"][f]), sigma2=r["sigma2"][f],
                                 YHat=r["BHat"][f] @ r["AHat"][f].T))
        assert p.CA is CAs[f] and p.CB is CBs[f]                         # the diagonals are written in place (src/vbmf.jl:131,143)
        assert (p.form_used, p.iters, p.d, p.status) == (r["form_used"][f], Recorder.fit_iters[f], r["d"][f], Recorder.fit_status[f])
        assert [type(v) for v in (p.form_used, p.iters, p.d, p.status, p.sigma2)] == [int, int, float, int, float]
        assert p.AHat.flags.f_contiguous and p.BHat.flags.f_contiguous


@pytest.mark.parametrize("kind", ["list", "Bags", "SparseBags"])
def test_row_gram_batch(pkg, rec, kind):
    Ys, _, Yall, col_off = _fit_sets(pkg, "basic", (3, 1, 2))
    if kind == "list":
        K = pkg.row_gram_batch(Ys)
        want = [bound(pkg, 0, "__init__", L, 6, 1, **pkg._defaults), bound(pkg, 0, "set_Y", Yall), bound(pkg, 0, "row_gram", col_off),
                bound(pkg, 0, "close")]
    else:
        K = pkg.row_gram_batch(getattr(pkg, kind)(Ys, H))
        want = _open_bags(pkg, 0, "basic" if kind == "Bags" else "sparse", Yall) + [bound(pkg, 0, "row_gram", col_off)]
    check_calls(rec, want)
    assert K is rec[2].ret


# ---- the callers of the batched fits: which call, which sets in which order, what comes back ---------------------------------------
def _only_fit_call(rec, name, n_bags_cols):
    assert [c.name for c in rec] == ["__init__", "set_Y", name, "close"]
    assert rec[0].args["M"] == n_bags_cols
    return rec[2]


@pytest.mark.parametrize("accepted", [None, 2])
def test_fit_restarts_sparse(pkg, rec, accepted):
    Y = np.random.default_rng(3).standard_normal((L, M))
    Recorder.fit_d = [0.5, np.nan, 2e-5 if accepted else 0.25, 1e-9 if accepted else 0.125]
    p = pkg.fit_restarts(Y, H, 30, nstarts=4, eps=1e-5, rng=np.random.default_rng(5))
    c = _only_fit_call(rec, "sparse_fit_batched", M)
    rng = np.random.default_rng(5)
    inits = [pkg.vbmf_sparse_init(Y, H, rng=rng) for _ in range(4)]
    a = c.args
    assert same(rec[1].args["Y"], Y) and same(a["col_off"], [0, M]) and same(a["fit_bag"], [0, 0, 0, 0])
    assert (a["niter"], a["eps"], a["H0"], a["full_cov"], a["est_cb"], a["est_priors"]) == (30, 1e-5, H, False, True, False)
    assert same(a["BHat"], [q.BHat for q in inits]) and same(a["CA"], np.concatenate([q.CA for q in inits]))
    k = 3 if accepted is None else accepted                         # the first with d <= 2 eps, else the last
    assert same(p.BHat, c.ret["BHat"][k]) and p.iters == 3 + k


def test_fit_restarts_dual(pkg, rec):
    Y = np.random.default_rng(3).standard_normal((L, M))
    p = pkg.fit_restarts(Y, H, 30, model="dual", H0=H0, nstarts=3, rng=np.random.default_rng(5))
    c = _only_fit_call(rec, "sparse_fit_batched", M)
    rng = np.random.default_rng(5)
    inits = [pkg.vbmf_dual_init(Y, H, H0, rng=rng) for _ in range(3)]
    a = c.args
    assert same(a["fit_bag"], [0, 0, 0]) and same(a["BHat"], [q.BHat for q in inits])
    assert (a["niter"], a["eps"], a["H0"], a["full_cov"], a["est_cb"], a["est_priors"]) == (30, 1e-4, H0, True, True, True)
    assert same(p.BHat, c.ret["BHat"][0])                           # the recorder's factors are far from zero: the first set


def test_train_local_folds(pkg, rec):
    rng = np.random.default_rng(4)
    folds = [(rng.standard_normal((L, a)), rng.standard_normal((L, b))) for a, b in ((2, 3), (0, 2), (3, 1))]
    ps = pkg.train_local_folds(folds, H, 1, 25, rng=np.random.default_rng(5))
    c = _only_fit_call(rec, "local_fit_batched", 11)                # one round: the recorder's factors are far from zero
    rng = np.random.default_rng(5)
    inits = [pkg.vbmf_sparse_init(np.concatenate(f, axis=1), H, H1=1, labels=np.arange(1, f[0].shape[1] + 1), rng=rng) for f in folds]
    a = c.args
    assert same(rec[1].args["Y"], np.concatenate([np.concatenate(f, axis=1) for f in folds], axis=1))
    assert same(a["col_off"], [0, 5, 7, 11]) and same(a["fit_bag"], [0, 1, 2]) and same(a["M0"], [2, 0, 3])
    assert (a["niter"], a["eps"], a["H0"], a["mask_H1"], a["full_cov"], a["est_cb"], a["est_priors"]) == (25, 1e-4, H, 1, False, True, False)
    assert same(a["BHat"], [q.BHat for q in inits])
    assert len(ps) == 3 and all(same(p.BHat, c.ret["BHat"][f]) for f, p in enumerate(ps))


@pytest.mark.parametrize("solver", ["basic", "sparse"])
def test_train_folds(pkg, rec, solver):
    rng = np.random.default_rng(4)
    folds = [(rng.standard_normal((L, a)), rng.standard_normal((L, b))) for a, b in ((2, 3), (0, 2), (3, 2))]
    n = 1 if solver == "basic" else 10
    Recorder.fit_d = None if solver == "basic" else [1.0] * 10 + [1.0, 1e-7] + [1.0] * 8 + [1.0] * 20   # bag 1: the second start is kept
    out = pkg.train_folds(folds, solver, H, 25, eps=1e-5, rng=np.random.default_rng(5), **(dict(form="auto") if solver == "basic" else {}))
    c = _only_fit_call(rec, "fit_batched" if solver == "basic" else "sparse_fit_batched", 10)
    used = [Y for k in (0, 2) for Y in folds[k]]                    # the fold with an empty class is left out (:97-100)
    rng = np.random.default_rng(5)
    init = pkg.vbmf_init if solver == "basic" else pkg.vbmf_sparse_init
    inits = [init(Y, H, rng=rng) for Y in used for _ in range(n)]
    a = c.args
    assert same(rec[1].args["Y"], np.concatenate(used, axis=1)) and same(a["col_off"], [0, 2, 5, 8, 10])
    assert same(a["fit_bag"], np.repeat(np.arange(4), n)) and same(a["BHat"], [q.BHat for q in inits])
    if solver == "basic":
        assert (a["niter"], a["eps"], a["est_covs"], a["est_var"], a["form"]) == (25, 1e-5, True, True, "auto")
        kept = [0, 1, 2, 3]
    else:
        assert (a["niter"], a["eps"], a["H0"], a["full_cov"], a["est_cb"], a["est_priors"]) == (25, 1e-5, H, False, True, False)
        kept = [9, 11, 29, 39]                                      # the first start with d <= 2 eps, else the last
    assert out[1] == (0, 0)
    got = [out[0][0], out[0][1], out[2][0], out[2][1]]
    assert all(same(p.BHat, c.ret["BHat"][f]) for p, f in zip(got, kept))
