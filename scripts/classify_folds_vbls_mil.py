#!/usr/bin/env python3
"""classify_folds with class_alg = "vbls" (vbmf_fixed_basis_jobs) at the sizes of the MIL experiments: what the "vbls" classification
of every fold's test bags (examples/mil_util.jl:469-479: 150 vbls! iterations of the basic model against each of the fold's two
models) costs end to end as a loop over the folds -- pool.select of the fold's test bags and classify_bags(res0, res1, the selection,
"vbls"), which runs one batched vbls! and one residual call per model on a new context -- and as ONE classify_folds call on the pool's
own context.  L = 166, fp32 storage of Y, the pool uploaded once outside every window.
Cases:
    f1, f5, f10   256 bags of 166 x U(1, 40) at H = 5, split into 1, 5 and 10 folds (fold k tests the bags b with b % folds == k)
    b50           50 bags of 166 x 120 at H = 5 in 5 folds
    h32           the 256 bags in 5 folds at H = 32
Arms:
    parent   a built checkout of the parent commit running the loop (--parent DIR; without it the arm is left out)
    loop     the same loop on this build (classify_bags and the entries under it are the parent's)
    folds    classify_folds on this build
Wall time of the whole call (perf_counter around it; every device call synchronises before it returns).  A process makes one warm
call per case, then three timed windows, and reports the best; every arm runs in a process of its own and is run twice (arm, arm'),
the arms alternating.  An arm's spread is the relative gap between its two bests; a verdict is read against the SUM of the two
arms' spreads (DESIGN.md sections 19-22).
    python scripts/classify_folds_vbls_mil.py [--parent DIR] [--out profiles/classify_folds_vbls_mil.txt]       (GPU box, repo root)
    python scripts/classify_folds_vbls_mil.py --profile      f5 ten times through classify_folds, no timing:
                                                             run under rocprofv3 --kernel-trace --stats --"""
import importlib.util
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, WINDOWS = 166, 3
CASES = {"f1": (256, None, 5, 1), "f5": (256, None, 5, 5), "f10": (256, None, 5, 10), "b50": (50, 120, 5, 5), "h32": (256, None, 32, 5)}


def load(tree):
    spec = importlib.util.spec_from_file_location("entry_" + str(abs(hash(tree))), os.path.join(tree, "__graft_entry__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.load_package()


def make_case(pkg, name):
    """(bags, the folds' basic models, the folds' test ids): two bases, bags drawn alternately from them, per fold a pair of basic sets
    around the bases as a short training leaves them (a small diagonal SigmaB, sigma2 near the noise variance)"""
    nb, M, H, nf = CASES[name]
    rng = np.random.default_rng(3)
    Ms = rng.integers(1, 41, nb) if M is None else [M] * nb
    Bs = [rng.standard_normal((L, H)) for _ in range(2)]
    bags = [Bs[b % 2] @ rng.standard_normal((H, m)) + 0.1 * rng.standard_normal((L, m)) for b, m in enumerate(Ms)]

    def model(B):
        p = pkg.vbmf_init(np.broadcast_to(np.float64(0.0), (L, 2)), H, rng=rng)
        p.BHat = np.asfortranarray(B + 0.01 * rng.standard_normal((L, H)))
        p.SigmaB = np.diag(rng.uniform(1e-4, 1e-3, H))
        p.sigma2 = float(rng.uniform(0.009, 0.011))
        return p
    models = [(model(Bs[0]), model(Bs[1])) for _ in range(nf)]
    tests = [[b for b in range(nb) if b % nf == k] for k in range(nf)]
    return bags, models, tests


def run_loop(pkg, pool, models, tests):
    out = []
    for (res0, res1), t in zip(models, tests):
        sel = pool.select(t, int(res0.H))
        try:
            out.append(pkg.classify_bags(res0, res1, sel, "vbls"))
        finally:
            sel.close()
    return out


def worker(tree, arm, cases):
    pkg = load(tree)
    pkg.set_defaults(y_dtype=pkg.VBMF_Y_F32, factor_dtype=pkg.VBMF_FACTOR_AUTO)
    out = {}
    for name in cases:
        bags, models, tests = make_case(pkg, name)
        with pkg.BagPool(bags) as pool:
            call = (lambda: pkg.classify_folds(models, tests, pool, "vbls")) if arm == "folds" else (lambda: run_loop(pkg, pool, models, tests))
            ref = call()                                                 # the warm call
            if arm == "folds":                                          # the two routes give the same labels (the loop's Y'B is fp32)
                assert all(np.array_equal(x[0], y[0]) for x, y in zip(ref, run_loop(pkg, pool, models, tests))), name
            best = np.inf
            for _ in range(WINDOWS):
                t0 = time.perf_counter()
                call()
                best = min(best, time.perf_counter() - t0)
        out[name] = best
    print("RESULT " + json.dumps(out), flush=True)


def spawn(tree, arm, cases):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--tree", tree, "--arm", arm, "--cases", ",".join(cases)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(f"worker {arm} failed (exit {p.returncode})")
    return json.loads(line[-1][7:])


def main():
    argv = sys.argv[1:]
    opt = lambda k, d=None: argv[argv.index(k) + 1] if k in argv else d
    if "--worker" in argv:
        return worker(opt("--tree", ROOT), opt("--arm"), opt("--cases").split(","))
    if "--profile" in argv:
        pkg = load(ROOT)
        pkg.set_defaults(y_dtype=pkg.VBMF_Y_F32, factor_dtype=pkg.VBMF_FACTOR_AUTO)
        bags, models, tests = make_case(pkg, "f5")
        with pkg.BagPool(bags) as pool:
            for _ in range(10):
                pkg.classify_folds(models, tests, pool, "vbls")
        return
    out, parent = opt("--out", os.path.join(ROOT, "profiles", "classify_folds_vbls_mil.txt")), opt("--parent")
    cases = opt("--cases").split(",") if opt("--cases") else list(CASES)
    arms = (["parent"] if parent else []) + ["loop", "folds"]
    got = {}                                                             # arm (or arm') -> case -> best
    for tick in ("", "'"):
        for a in arms:
            got[a + tick] = spawn(parent if a == "parent" else ROOT, a, cases)
        print(f"run{tick or ' '}: " + "  ".join(f"{n} " + "/".join(f"{1e3 * got[a + tick][n]:.2f}" for a in arms) for n in cases), flush=True)
    base = "parent" if parent else "loop"
    lines = [f"L = {L}, fp32 storage of Y, class_alg = \"vbls\" (150 vbls! iterations of the basic model); wall ms of the whole "
             f"classification (every fold's test bags against its two models), the pool uploaded outside the window",
             f"a process = one warm call, then the best of {WINDOWS} windows; one process per arm and run, the arms alternated; every arm run "
             "twice (arm, arm'); spread = |best - best'| / min",
             "verdicts are read against the SUM of the two arms' spreads; loop = per fold pool.select of its test bags and classify_bags on "
             "the selection (a context, a gather, two batched vbls!, two residual calls); folds = one classify_folds",
             "",
             f"{'case':5s} {'bags':>5s} {'H':>3s} {'folds':>5s} " + "".join(f"{a:>9s} {a + chr(39):>9s} {'spread':>7s}" for a in arms)
             + f"  {'folds/' + base:>12s}  verdicts"]
    ok = True
    for n in cases:
        nb, _, H, nf = CASES[n]
        T = {a: min(got[a][n], got[a + "'"][n]) for a in arms}
        sp = {a: abs(got[a][n] - got[a + "'"][n]) / T[a] for a in arms}
        s = sp["folds"] + sp[base]
        v = []
        if T[base] - T["folds"] > s * T[base]:
            v.append(f"folds beats {base} beyond the spreads")
        elif T["folds"] - T[base] > s * T[base]:
            v.append(f"FOLDS IS SLOWER THAN {base.upper()} BEYOND THE SPREADS")
        else:
            v.append(f"folds and {base} overlap within the spreads")
        if parent:
            sl = sp["loop"] + sp["parent"]
            v.append("loop overlaps parent" if abs(T["loop"] - T["parent"]) <= sl * max(T["loop"], T["parent"]) else "LOOP DOES NOT OVERLAP PARENT")
        ok = ok and not any(x.isupper() for x in v)
        lines.append(f"{n:5s} {nb:5d} {H:3d} {nf:5d} " + "".join(f"{1e3 * got[a][n]:9.3f} {1e3 * got[a + chr(39)][n]:9.3f} {sp[a]:7.3f}" for a in arms)
                     + f"  {T['folds'] / T[base]:12.3f}  " + "; ".join(v))
    lines.append("every row at least as fast as the " + base + " arm outside the spreads" if ok
                 else "NOT EVERY ROW IS AS FAST AS THE " + base.upper() + " ARM (see the verdicts in capitals)")
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
