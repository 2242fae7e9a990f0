#!/usr/bin/env python3
"""The Gram form of the batched basic-model fits (vbmf_batch_(..., form=...); vbmf_fit_batched_form) at the sizes of the MIL experiments'
training sets (examples/mil_util.jl:110-114 inside folds x p x repetitions), against the streaming form and against the parent commit's
vbmf_batch_.  The protocol of scripts/fit_basic_batch_mil.py: 50 sweeps (eps = 0), L = 166, est_covs = est_var = True, the same
initialisations on every arm, wall time per fit end to end (parameter copies, upload, the sweeps, read-back; every call synchronises
before it returns), best of three windows.  Arms:
    parent    vbmf_batch_ of a built checkout of the parent commit (--parent DIR; without it the arm is left out)
    stream    this build, form="stream"
    gram      this build, form="gram"
    auto      this build, form="auto"
Each arm runs in a process of its own (two builds of one library do not share a process); a round starts one process per arm, one after
the other, and each process runs every row once after a warm-up call, so the arms alternate.  Three rounds.
    python scripts/fit_basic_gram_mil.py [--parent DIR] [--out profiles/fit_basic_gram_mil.txt]     (GPU box, repo root)
    python scripts/fit_basic_gram_mil.py --worker gram --rows wide20                                   (one arm, one row: for a profiler)"""
import copy
import importlib.util
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NITER, L, ROUNDS = 50, 166, 3
# name, M, H, fits, one shared bag
ROWS = (("small1", 24, 1, 100, False), ("small5", 24, 5, 100, False), ("edge5", 332, 5, 20, False), ("mid5", 640, 5, 20, False),
        ("wide20", 3000, 5, 20, False), ("wide2", 3000, 5, 2, False), ("shared20", 3000, 5, 20, True))
ARMS = ("parent", "stream", "gram", "auto")


def load(tree):
    spec = importlib.util.spec_from_file_location("entry_" + str(abs(hash(tree))), os.path.join(tree, "__graft_entry__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.load_package()


def bags(M, H, n, seed):
    """rank-H signal plus noise, as in scripts/fit_basic_batch_mil.py"""
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((L, H)) @ rng.standard_normal((H, M)) + 0.1 * rng.standard_normal((L, M)) for _ in range(n)]


def worker(arm, tree, rows):
    pkg = load(tree)
    pkg.set_defaults(y_dtype=pkg.VBMF_Y_F32, factor_dtype=pkg.VBMF_FACTOR_AUTO)
    kw = {} if arm == "parent" else dict(form=arm)
    out = {}
    for name, M, H, n, shared in ROWS:
        if rows and name not in rows:
            continue
        Ys = bags(M, H, 1 if shared else n, 1)
        bag_of = [0] * n if shared else list(range(n))
        rng = np.random.default_rng(7)
        ps0 = [pkg.vbmf_init(Ys[b], H, rng=rng) for b in bag_of]
        for k in range(2):                                          # the first call warms up (context, code objects)
            ps = copy.deepcopy(ps0)
            t0 = time.perf_counter()
            pkg.vbmf_batch_(Ys, ps, NITER, eps=0.0, est_covs=True, est_var=True, bag_of=bag_of, **kw)
            dt = time.perf_counter() - t0
        out[name] = dict(t=dt, B0=float(np.linalg.norm(ps[0].BHat)), Bsum=float(sum(np.linalg.norm(p.BHat) for p in ps)),
                         gram=int(sum(getattr(p, "form_used", 0) for p in ps)))
    print("RESULT " + json.dumps(out), flush=True)


def main():
    argv = sys.argv[1:]
    opt = lambda k, d=None: argv[argv.index(k) + 1] if k in argv else d
    if "--worker" in argv:
        return worker(opt("--worker"), opt("--tree", ROOT), (opt("--rows") or "").split(",") if opt("--rows") else ())
    out, parent = opt("--out", os.path.join(ROOT, "profiles", "fit_basic_gram_mil.txt")), opt("--parent")
    arms = [a for a in ARMS if a != "parent" or parent]
    res = {a: [] for a in arms}
    for r in range(ROUNDS):
        for a in arms:
            tree = parent if a == "parent" else ROOT
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", a, "--tree", tree], capture_output=True, text=True,
                               timeout=600)
            line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"arm {a} failed in round {r} (exit {p.returncode})")
            res[a].append(json.loads(line[-1][7:]))
            print(f"round {r} {a}: " + " ".join(f"{k}={1e3 * v['t']:.2f}ms" for k, v in res[a][-1].items()), flush=True)
    lines = [f"basic-model fits of {NITER} sweeps (eps = 0, est_covs = est_var = true), L = {L}, fp32 Y; wall time per fit end to end, best of "
             f"{ROUNDS} windows (spread = (worst - best) / best of the windows), one process per arm and window, arms alternated",
             "row       M     H  fits bags  " + "  ".join(f"{a + ' ms/fit':>14s} {'spread':>6s}" for a in arms)
             + "   gram/parent  gram/stream  auto/stream  fits in Gram form under auto  verdicts"]
    ok = True
    for name, M, H, n, shared in ROWS:
        t = {a: [w[name]["t"] for w in res[a]] for a in arms}
        best = {a: min(v) for a, v in t.items()}
        sp = {a: max(v) - min(v) for a, v in t.items()}             # seconds
        base = "parent" if parent else "stream"
        v = []
        if parent:
            v.append("stream overlaps parent" if abs(best["stream"] - best["parent"]) <= sp["stream"] + sp["parent"]
                     else "STREAM DOES NOT OVERLAP PARENT")
        if name in ("mid5", "wide20", "wide2", "shared20"):
            v.append(f"gram faster than {base}" if best[base] - best["gram"] > sp[base] + sp["gram"] else f"GRAM NOT FASTER THAN {base.upper()}")
        v.append("auto not slower than stream" if best["auto"] - best["stream"] <= sp["auto"] + sp["stream"] else "AUTO SLOWER THAN STREAM")
        ok = ok and not any(s.isupper() for s in v)
        d = max(abs(res[a][0][name]["Bsum"] - res["stream"][0][name]["Bsum"]) / res["stream"][0][name]["Bsum"] for a in arms)
        lines.append(f"{name:8s} {M:5d} {H:2d}  {n:4d} {1 if shared else n:4d}  "
                     + "  ".join(f"{1e3 * best[a] / n:14.3f} {100 * sp[a] / best[a]:5.1f}%" for a in arms)
                     + (f"   {best['gram'] / best['parent']:11.3f}" if parent else "           n/a")
                     + f"  {best['gram'] / best['stream']:11.3f}  {best['auto'] / best['stream']:11.3f}  {res['auto'][0][name]['gram']:4d} of {n:4d}"
                     + f"  rel d sum|BHat| {d:.1e}  " + "; ".join(v))
        print(lines[-1], flush=True)
    lines.append("all acceptance points met" if ok else "NOT ALL ACCEPTANCE POINTS MET (see the verdicts in capitals)")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
