#!/usr/bin/env python3
"""classify_folds with class_alg = "lower_bound" and "min_err" (vbmf_sparse_scored_jobs) at the sizes of the MIL experiments: what
factorize_bag's classifiers (examples/mil_util.jl:393-416, :493-514: per test bag 20 vbls! iterations against the fold's basis without
its last H1 columns, 20 against the whole basis, then lowerBound against lowerBoundTrimmed or the two residual norms) cost end to end
as a loop over the folds -- classify_bags(res0, 0, the fold's test bags, alg), which uploads the bags once per basis and runs up to
eight batched launches and a host copy_vbmf_params per bag and basis -- and as ONE classify_folds call on the pool's own context.
L = 166, fp32 storage of Y, the pool uploaded once outside every window.
Cases (each with both classifiers: name/lb, name/me):
    f1, f5, f10   256 bags of 166 x U(1, 40) at H = 5, H1 = 1, split into 1, 5 and 10 folds (fold k tests the bags b with b % folds == k)
    b50           50 bags of 166 x 120 at H = 5, H1 = 1 in 5 folds
    h32           the 256 bags in 5 folds at H = 32, H1 = 1
    wide          50 bags of 166 x 450 at H = 5, H1 = 1 in 5 folds: M_b (H - H1) = 1800, the diagonal form of updateA! (:405-409)
Arms:
    parent   a built checkout of the parent commit running the loop (--parent DIR; without it the arm is left out)
    loop     the same loop on this build
    folds    classify_folds on this build
Wall time of the whole call (perf_counter around it; every device call synchronises before it returns).  A process makes one warm
call per case, then three timed windows, and reports the best; every arm runs in a process of its own and is run twice (arm, arm'),
the arms alternating.  An arm's spread is the relative gap between its two bests; a verdict is read against the SUM of the two
arms' spreads (DESIGN.md sections 19-23).
    python scripts/classify_folds_local_mil.py [--parent DIR] [--out profiles/classify_folds_local_mil.txt]     (GPU box, repo root)
    python scripts/classify_folds_local_mil.py --profile     f5 ten times through classify_folds ("lower_bound"), no timing:
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
SIZES = {"f1": (256, None, 5, 1, 1), "f5": (256, None, 5, 1, 5), "f10": (256, None, 5, 1, 10), "b50": (50, 120, 5, 1, 5),
         "h32": (256, None, 32, 1, 5), "wide": (50, 450, 5, 1, 5)}
ALGS = {"lb": "lower_bound", "me": "min_err"}
CASES = {f"{n}/{a}": v for n, v in SIZES.items() for a in ALGS}
SCORE_TOL = 2e-3          # the per-fold path's own bound on its scores (CLASSIFY_BOUND_TOL of tests/test_gpu_bag_scoring.py)


def load(tree):
    spec = importlib.util.spec_from_file_location("entry_" + str(abs(hash(tree))), os.path.join(tree, "__graft_entry__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.load_package()


def make_case(pkg, name):
    """(bags, the folds' models, the folds' test ids, the classifier): one basis, the bags of even index drawn from its first H - H1
    columns only, per fold a sparse set with H1 around the basis as a short training leaves it (a small diagonal SigmaB, the
    hyper-priors of vbmf_sparse_init)"""
    nb, M, H, H1, nf = CASES[name]
    rng = np.random.default_rng(3)
    Ms = rng.integers(1, 41, nb) if M is None else [M] * nb
    B = rng.standard_normal((L, H))
    bags = []
    for b, m in enumerate(Ms):
        A = rng.standard_normal((H, m))
        if b % 2 == 0:
            A[H - H1:] = 0.0
        bags.append(B @ A + 0.1 * rng.standard_normal((L, m)))

    def model():
        p = pkg.vbmf_sparse_init(np.broadcast_to(np.float64(0.0), (L, 2)), H, H1=H1, rng=rng)
        p.BHat = np.asfortranarray(B + 0.01 * rng.standard_normal((L, H)))
        p.SigmaB = np.diag(rng.uniform(1e-4, 1e-3, H))
        return p
    models = [model() for _ in range(nf)]
    tests = [[b for b in range(nb) if b % nf == k] for k in range(nf)]
    return bags, models, tests, ALGS[name.split("/")[1]]


def run_loop(pkg, bags, models, tests, alg):
    return [pkg.classify_bags(res0, 0, [bags[b] for b in t], alg) for res0, t in zip(models, tests)]


def worker(tree, arm, cases):
    pkg = load(tree)
    pkg.set_defaults(y_dtype=pkg.VBMF_Y_F32, factor_dtype=pkg.VBMF_FACTOR_AUTO)
    out = {}
    for name in cases:
        bags, models, tests, alg = make_case(pkg, name)
        with pkg.BagPool(bags) as pool:
            call = (lambda: pkg.classify_folds(models, tests, pool, alg)) if arm == "folds" else (lambda: run_loop(pkg, bags, models, tests, alg))
            ref = call()                                                 # the warm call
            if arm == "folds":                                          # the two routes give the same scores within the loop's own bound
                for x, y in zip(ref, run_loop(pkg, bags, models, tests, alg)):
                    assert all(np.max(np.abs(x[i] - y[i]) / np.abs(y[i])) <= SCORE_TOL for i in (1, 2)), name
            best = np.inf
            for _ in range(WINDOWS):
                t0 = time.perf_counter()
                call()
                best = min(best, time.perf_counter() - t0)
        out[name] = best
    print("RESULT " + json.dumps(out), flush=True)


def spawn(tree, arm, cases):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--tree", tree, "--arm", arm, "--cases", ",".join(cases)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
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
        bags, models, tests, alg = make_case(pkg, "f5/lb")
        with pkg.BagPool(bags) as pool:
            for _ in range(10):
                pkg.classify_folds(models, tests, pool, alg)
        return
    out, parent = opt("--out", os.path.join(ROOT, "profiles", "classify_folds_local_mil.txt")), opt("--parent")
    cases = opt("--cases").split(",") if opt("--cases") else list(CASES)
    arms = (["parent"] if parent else []) + ["loop", "folds"]
    got = {}                                                             # arm (or arm') -> case -> best
    for tick in ("", "'"):
        for a in arms:
            got[a + tick] = spawn(parent if a == "parent" else ROOT, a, cases)
        print(f"run{tick or ' '}: " + "  ".join(f"{n} " + "/".join(f"{1e3 * got[a + tick][n]:.2f}" for a in arms) for n in cases), flush=True)
    base = "parent" if parent else "loop"
    lines = [f"L = {L}, fp32 storage of Y, class_alg = \"lower_bound\" (lb) and \"min_err\" (me): factorize_bag, 2 x 20 vbls! iterations per bag; "
             f"wall ms of the whole classification (every fold's test bags against its model), the pool uploaded outside the window",
             f"a process = one warm call, then the best of {WINDOWS} windows; one process per arm and run, the arms alternated; every arm run "
             "twice (arm, arm'); spread = |best - best'| / min",
             "verdicts are read against the SUM of the two arms' spreads; loop = classify_bags on the fold's test bags per fold (two uploads, "
             "up to four batched vbls! and four scoring calls); folds = one classify_folds",
             "",
             f"{'case':8s} {'bags':>5s} {'H':>3s} {'folds':>5s} " + "".join(f"{a:>9s} {a + chr(39):>9s} {'spread':>7s}" for a in arms)
             + f"  {'folds/' + base:>12s}  verdicts"]
    ok = True
    for n in cases:
        nb, _, H, _, nf = CASES[n]
        T = {a: min(got[a][n], got[a + "'"][n]) for a in arms}
        sp = {a: abs(got[a][n] - got[a + "'"][n]) / T[a] for a in arms}
        s = sp["folds"] + sp[base]
        v = []
        if nf == 1:                                                      # (printed as measured: no verdict is set for one fold)
            v.append(f"one fold: folds / {base} as measured")
        else:
            v.append(f"folds beats {base} beyond the spreads" if T[base] - T["folds"] > s * T[base] else f"FOLDS DOES NOT BEAT {base.upper()}")
        if parent:
            sl = sp["loop"] + sp["parent"]
            v.append("loop overlaps parent" if abs(T["loop"] - T["parent"]) <= sl * max(T["loop"], T["parent"]) else "LOOP DOES NOT OVERLAP PARENT")
        ok = ok and not any(x.isupper() for x in v)
        lines.append(f"{n:8s} {nb:5d} {H:3d} {nf:5d} " + "".join(f"{1e3 * got[a][n]:9.3f} {1e3 * got[a + chr(39)][n]:9.3f} {sp[a]:7.3f}" for a in arms)
                     + f"  {T['folds'] / T[base]:12.3f}  " + "; ".join(v))
    lines.append("all acceptance points met" if ok else "NOT ALL ACCEPTANCE POINTS MET (see the verdicts in capitals)")
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
