#!/usr/bin/env python3
"""The bag pool (BagPool, vbmf_set_Y_gather) at the sizes of the MIL experiments: what a batched call costs end to end when its bags
are a list of matrices (laid side by side on the host, uploaded in fp64, staged again on the device) and when they are a selection
gathered on the device from a data set that was uploaded once.  L = 166, fp32 storage of Y, the same initialisations on every arm.
Cases (the rows of the tables DESIGN.md already publishes):
    basic20    20 basic fits at 166 x 3000, form="gram", 50 sweeps                     (the 32 ms call of section 15)
    sparse20   20 sparse fits (2 bags x 10 starts) at 166 x 3000, form="split"         (section 19)
    dual100    100 two-group full_cov fits (10 bags x 10 starts) at 166 x 640          (section 11)
    vbls256    vbls_batch_, 30 iterations, on 256 bags of 166 x U(1, 40)               (section 9.6)
    ols256     classify_bags(..., "ols") on the same 256 bags
    folds5     a five-fold train_folds(solver="basic", form="gram") over one data set of 50 bags of 166 x 120
Arms:
    parent     a built checkout of the parent commit on the list path (--parent DIR; without it the arm is left out)
    list       this build on the list path
    pool       this build through a pool uploaded once OUTSIDE the window
    pool+up    this build through a pool whose upload is INSIDE the window (folds5: one upload, five folds; the row gives the call's
               share, the whole window divided by five)
Wall time end to end (perf_counter around the call; every call synchronises before it returns), best of three windows.  Each arm is run
twice (arm and arm'); a side's spread is the relative difference between its two bests, and the spread a verdict is read against is the
larger of the two sides' (DESIGN.md section 19).  Every arm runs in a process of its own (two builds of one library do not share a
process, and an arm that holds an 80 MB pool changes the allocator state the others' host work meets): a round starts one process
per arm, one after the other, so the arms alternate; inside a process arm and arm' alternate.
pool+up on a single call holds one upload AND one gather, so it cannot beat the list path; it is shown for the price of a pool that is
used once.  Its verdict is taken on folds5, the case it exists for.
Beside the whole call every window also stamps its "layout and upload" stage: the time inside the Bags / SparseBags constructor (host
concatenation, fp64 upload, tiling) -- for folds5 also the host's get_matrices concatenation -- or inside BagPool.select (the gather).
For basic20 the other stages are stamped too, in windows of their own: parameter marshalling (Context.fit_batched around the library
call), the device call (the library entry), write-back (the fields of every set) and YHat (_host_YHat).
    python scripts/bag_pool_mil.py [--parent DIR] [--out profiles/bag_pool_mil.txt]       (GPU box, repo root)
    python scripts/bag_pool_mil.py --profile basic20                                      the case once through a pool, no timing: run
                                                                                          under rocprofv3 --kernel-trace --stats --"""
import copy
import importlib.util
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, H, NITER, ROUNDS = 166, 5, 50, 3
CASES = ("basic20", "sparse20", "dual100", "vbls256", "ols256", "folds5")
STAGES = ("layout+upload", "marshal", "device", "write-back", "YHat")


def load(tree):
    spec = importlib.util.spec_from_file_location("entry_" + str(abs(hash(tree))), os.path.join(tree, "__graft_entry__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.load_package()


def low_rank(M, n, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((L, H)) @ rng.standard_normal((H, m)) + 0.1 * rng.standard_normal((L, m))
            for m in ([M] * n if np.ndim(M) == 0 else M)]


class Clock:
    """seconds spent inside the wrapped callables since reset()"""

    def __init__(self):
        self.t = {}

    def reset(self):
        self.t = {}

    def add(self, key, dt):
        self.t[key] = self.t.get(key, 0.0) + dt

    def wrap(self, key, fn):
        def timed(*a, **kw):
            t0 = time.perf_counter()
            try:
                return fn(*a, **kw)
            finally:
                self.add(key, time.perf_counter() - t0)
        return timed


class TimedLib:
    """the loaded library with the batched-fit entries stamped"""

    def __init__(self, lib, clock):
        self._lib, self._clock = lib, clock

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        return self._clock.wrap("device", f) if name in ("vbmf_fit_batched", "vbmf_fit_batched_form") else f


def make_case(pkg, name):
    """(prepare, run): prepare() -> fresh parameter sets; run(Ys_or_selection, sets) makes the call.  Also the bags, the groups that make
    the call's matrices from them, the kind of upload and H."""
    if name == "basic20":
        bags = low_rank(3000, 20, 1)
        groups, kind = list(range(20)), "basic"
        mats = bags
        rng = np.random.default_rng(7)
        ps0 = [pkg.vbmf_init(Y, H, rng=rng) for Y in mats]
        run = lambda Ys, ps: pkg.vbmf_batch_(Ys, ps, NITER, eps=0.0, est_covs=True, est_var=True, form="gram")
    elif name in ("sparse20", "dual100"):
        nb, M = (2, 3000) if name == "sparse20" else (10, 640)
        bags = low_rank(M, nb, 2)
        groups, kind, mats = list(range(nb)), "sparse", bags
        bag_of = [b for b in range(nb) for _ in range(10)]
        rng = np.random.default_rng(7)
        if name == "sparse20":
            ps0 = [pkg.vbmf_sparse_init(mats[b], H, rng=rng) for b in bag_of]
            run = lambda Ys, ps: pkg.vbmf_sparse_batch_(Ys, ps, NITER, eps=0.0, bag_of=bag_of, form="split")
        else:
            ps0 = [pkg.vbmf_dual_init(mats[b], H, 2, rng=rng) for b in bag_of]
            run = lambda Ys, ps: pkg.vbmf_dual_batch_(Ys, ps, NITER, eps=0.0, full_cov=True, bag_of=bag_of)
    elif name in ("vbls256", "ols256"):
        bags = low_rank(np.random.default_rng(3).integers(1, 41, 256), 256, 4)
        groups, kind, mats = list(range(256)), "basic", bags
        rng = np.random.default_rng(7)
        res = [pkg.vbmf_init(np.zeros((L, 300)), H, ca=0.1, cb=0.1, sigma2=0.1, rng=rng) for _ in range(2)]
        if name == "vbls256":
            ps0 = [pkg.copy_vbmf_params(Y, res[0], rng=rng) for Y in mats]
            run = lambda Ys, ps: pkg.vbls_batch_(Ys, ps, 30)
        else:
            ps0 = []
            run = lambda Ys, ps: pkg.classify_bags(res[0], res[1], Ys, "ols")
    else:
        raise SystemExit(f"unknown case {name}")
    return dict(bags=bags, groups=groups, kind=kind, mats=mats, ps0=ps0, run=run)


def folds5(pkg, arm, clock):
    """one window of the five-fold train_folds: returns nothing, stamps the layout in the clock"""
    nb = 50
    if not hasattr(folds5, "bags"):
        folds5.bags = low_rank(120, nb, 5)
        folds5.labels = np.arange(nb) % 2
    bags, labels = folds5.bags, folds5.labels
    folds = []
    for k in range(5):
        train = [b for b in range(nb) if b % 5 != k]
        folds.append(([b for b in train if labels[b] == 0], [b for b in train if labels[b] == 1]))
    kw = dict(rng=np.random.default_rng(7), form="gram")
    if arm in ("list", "parent"):
        t0 = time.perf_counter()                                     # get_matrices (examples/mil_util.jl:46): the host concatenation
        pairs = [tuple(np.concatenate([bags[b] for b in g], axis=1) for g in pair) for pair in folds]
        clock.add("layout+upload", time.perf_counter() - t0)
        return pkg.train_folds(pairs, "basic", H, NITER, eps=0.0, **kw)
    pool = folds5.pool if arm == "pool" else pkg.BagPool(bags)
    try:
        return pkg.train_folds(folds, "basic", H, NITER, eps=0.0, pool=pool, **kw)
    finally:
        if arm != "pool":
            pool.close()


def worker(tree, arms, cases, stages):
    pkg = load(tree)
    pkg.set_defaults(y_dtype=pkg.VBMF_Y_F32, factor_dtype=pkg.VBMF_FACTOR_AUTO)
    clock = Clock()
    for cls in (pkg.Bags, pkg.SparseBags):
        cls.__init__ = clock.wrap("layout+upload", cls.__init__)
    if hasattr(pkg, "BagPool"):
        pkg.BagPool.select = clock.wrap("layout+upload", pkg.BagPool.select)
    if stages:
        real = pkg.capi.lib()
        pkg.capi.lib = lambda: TimedLib(real, clock)
        pkg.Context.fit_batched = clock.wrap("fit_batched", pkg.Context.fit_batched)
        pkg._host_YHat = clock.wrap("YHat", pkg._host_YHat)
    out = {}
    for name in cases:
        c = None if name == "folds5" else make_case(pkg, name)
        pool = None
        if any(a.startswith("pool") for a in arms):
            if name == "folds5":
                folds5(pkg, "list", clock)
                folds5.pool = pkg.BagPool(folds5.bags)
            else:
                pool = pkg.BagPool(c["bags"])

        def window(arm):
            ps = copy.deepcopy(c["ps0"]) if c else None
            clock.reset()
            t0 = time.perf_counter()
            if name == "folds5":
                folds5(pkg, arm, clock)
            elif arm in ("list", "parent"):
                c["run"](c["mats"], ps)
            else:
                p = pool if arm == "pool" else pkg.BagPool(c["bags"])
                sel = p.select(c["groups"], H, kind=c["kind"])
                try:
                    c["run"](sel, ps)
                finally:
                    sel.close()
                    if p is not pool:
                        p.close()
            dt = time.perf_counter() - t0
            return dt, dict(clock.t)
        res = {}
        for a in arms:                                               # warm up: contexts, code objects
            window(a)
        for a in [x for a in arms for x in (a, a + "'")]:
            dt, st = window(a.rstrip("'"))
            res[a] = dict(t=dt, up=st.get("layout+upload", 0.0))
            if stages:
                dev, fb, yh = st.get("device", 0.0), st.get("fit_batched", 0.0), st.get("YHat", 0.0)
                res[a]["stages"] = {"layout+upload": res[a]["up"], "marshal": fb - dev, "device": dev, "YHat": yh,
                                    "write-back": dt - res[a]["up"] - fb - yh}
        out[name] = res
        if pool is not None:
            pool.close()
        if name == "folds5" and hasattr(folds5, "pool"):
            folds5.pool.close()
    print("RESULT " + json.dumps(out), flush=True)


def spawn(tree, arms, cases, stages=False):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--tree", tree, "--arms", ",".join(arms), "--cases", ",".join(cases)]
    p = subprocess.run(cmd + (["--stages"] if stages else []), capture_output=True, text=True, timeout=900)
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(f"worker {arms} failed (exit {p.returncode})")
    return json.loads(line[-1][7:])


def main():
    argv = sys.argv[1:]
    opt = lambda k, d=None: argv[argv.index(k) + 1] if k in argv else d
    if "--worker" in argv:
        return worker(opt("--tree", ROOT), opt("--arms").split(","), opt("--cases").split(","), "--stages" in argv)
    if "--profile" in argv:
        pkg = load(ROOT)
        pkg.set_defaults(y_dtype=pkg.VBMF_Y_F32, factor_dtype=pkg.VBMF_FACTOR_AUTO)
        c = make_case(pkg, opt("--profile"))
        with pkg.BagPool(c["bags"]) as pool:
            sel = pool.select(c["groups"], H, kind=c["kind"])
            c["run"](sel, c["ps0"])
            sel.close()
        return
    out, parent = opt("--out", os.path.join(ROOT, "profiles", "bag_pool_mil.txt")), opt("--parent")
    cases = opt("--cases").split(",") if opt("--cases") else list(CASES)
    mine = ["list", "pool", "pool+up"]
    arms = (["parent"] if parent else []) + mine
    best = {n: {} for n in cases}                                    # case -> arm (or arm') -> [best t, best up]
    for r in range(ROUNDS):
        got = {}
        for a in arms:
            for n, v in spawn(parent if a == "parent" else ROOT, [a], cases).items():
                got.setdefault(n, {}).update(v)
        for n in cases:
            for a, v in got[n].items():
                b = best[n].setdefault(a, [np.inf, np.inf])
                b[0], b[1] = min(b[0], v["t"]), min(b[1], v["up"])
        print(f"round {r}: " + "  ".join(f"{n} " + "/".join(f"{1e3 * got[n][a]['t']:.1f}" for a in arms) for n in cases), flush=True)
    ms = lambda x: 1e3 * x
    lines = [f"L = {L}, H = {H}, fp32 storage of Y, {NITER} sweeps per fit (eps = 0); wall ms per call end to end, best of {ROUNDS} windows, one "
             "process per arm and round, the arms alternated; every arm run twice (arm, arm')",
             "spread = max over the two sides of |best - best'| / best; up = the layout-and-upload stage of the same windows (list: host "
             "concatenation + fp64 upload + tiling; pool: the gather)",
             "folds5, pool+up: the whole window holds ONE upload and five folds' work; call/5 and up/5 are the per-fold shares",
             "", "whole call"
             "\ncase        " + "".join(f"{a:>10s} {a + chr(39):>10s}" for a in arms) + "   spread  list/parent  pool/parent  pool+up/parent  verdicts"]
    ups = ["", "layout and upload", "case        " + "".join(f"{a:>10s} {a + chr(39):>10s}" for a in arms) + "   spread  parent - pool  verdict"]
    ok = True
    base = "parent" if parent else "list"
    for n in cases:
        b = best[n]
        T = {a: min(b[a][0], b[a + "'"][0]) for a in arms}
        U = {a: min(b[a][1], b[a + "'"][1]) for a in arms}
        sp = {a: abs(b[a][0] - b[a + "'"][0]) / T[a] for a in arms}
        spu = {a: abs(b[a][1] - b[a + "'"][1]) / max(U[a], 1e-9) for a in arms}
        v = []
        if parent:
            s = max(sp["list"], sp["parent"])
            v.append("list overlaps parent" if abs(T["list"] - T["parent"]) <= s * max(T["list"], T["parent"]) else "LIST DOES NOT OVERLAP PARENT")
        for a in ("pool", "pool+up") if n == "folds5" else ("pool",):
            s = max(sp[a], sp[base])
            v.append(f"{a} not slower" if T[a] - T[base] <= s * T[base] else f"{a.upper()} SLOWER THAN {base.upper()}")
        ok = ok and not any(x.isupper() for x in v)
        lines.append(f"{n:10s}  " + "".join(f"{ms(b[a][0]):10.2f} {ms(b[a + chr(39)][0]):10.2f}" for a in arms)
                     + f"  {max(sp.values()):7.3f}  " + (f"{T['list'] / T['parent']:11.3f}  {T['pool'] / T['parent']:11.3f}  {T['pool+up'] / T['parent']:14.3f}"
                                                         if parent else f"{'n/a':>11s}  {'n/a':>11s}  {'n/a':>14s}") + "  " + "; ".join(v))
        s = max(spu["pool"], spu[base])
        won = U[base] - U["pool"] > s * U[base]
        ok = ok and won
        ups.append(f"{n:10s}  " + "".join(f"{ms(b[a][1]):10.3f} {ms(b[a + chr(39)][1]):10.3f}" for a in arms)
                   + f"  {s:7.3f}  {ms(U[base] - U['pool']):13.3f}  " + (f"pool shorter than {base} beyond the spread" if won else f"POOL NOT SHORTER THAN {base.upper()}"))
    lines += ups
    # the stages of the section-15 call, windows of their own
    if "basic20" in cases:
        st = {}
        if parent:
            st.update(spawn(parent, ["parent"], ["basic20"], stages=True)["basic20"])
        for a in ("list", "pool"):
            st.update(spawn(ROOT, [a], ["basic20"], stages=True)["basic20"])
        lines += ["", "basic20 by stage, ms (one window per arm and arm'; the smaller total of the two is shown; write-back = the rest of the call:"
                  " the sets' fields, host checks, close)", f"{'arm':8s} " + "".join(f"{s:>15s}" for s in STAGES) + f"{'total':>10s}"]
        for a in [x for x in ("parent", "list", "pool") if x in st]:
            w = min((st[a], st[a + "'"]), key=lambda x: x["t"])
            lines.append(f"{a:8s} " + "".join(f"{ms(w['stages'][s]):15.3f}" for s in STAGES) + f"{ms(w['t']):10.2f}")
    lines.append("all acceptance points met" if ok else "NOT ALL ACCEPTANCE POINTS MET (see the verdicts in capitals)")
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
