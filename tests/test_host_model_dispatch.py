"""What the Python host sends to the device for the ARD-sparse model and its grouped siblings (vbmf_dual, vbmf_trial), and for
the basic model's paths that share code with them: the package's Context is replaced by a recorder that logs every method call
with its bound arguments and returns deterministic results.  Each case checks the full call sequence and every field written
back to params (and that no other field changed).  No GPU and no library are needed."""
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
    if name == "dual_get_priors":
        pr = c.v(6).ravel()
        return H0, dict(alpha00=pr[0], beta00=pr[1], alpha01=pr[2], beta01=pr[3], alpha0=pr[4], alpha1=pr[5])
    if name == "trial_get_priors":
        pr = c.v(9).ravel()
        return H0, M0, {k: float(pr[i]) for i, k in enumerate(c.TRIAL_KEYS)}
    return None


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
              "dual_get_priors", "dual_run", "trial_set_priors", "trial_get_priors", "trial_run"):
    setattr(Recorder, _name, _method(_name))


@pytest.fixture
def rec(pkg, monkeypatch):
    """The recorder in place of Context, empty session caches, and the log writers as stubs that log too."""
    Recorder.log, Recorder.serial, Recorder.runs, Recorder.count = [], 0, 0, 0
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
