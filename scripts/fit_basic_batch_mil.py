#!/usr/bin/env python3
"""Many basic-model fits in one device call (vbmf_batch_; vbmf_fit_batched) at the sizes of the MIL experiments' training sets
(examples/mil_util.jl:110-114 inside folds x p x repetitions), against the loop of per-fit vbmf_ calls from the SAME initialisations.
Fixed 50 sweeps on both sides (eps = 0), est_covs = est_var = True, wall time per fit end to end (parameter copies, upload, the sweeps,
read-back; every call synchronises before it returns), best of three windows.  The two sides differ in arithmetic: the per-fit path
accumulates in fp32 (MFMA on Y as stored), the batch is fp64 throughout.
    small1    100 fits at 166 x 24, H = 1, fp32 Y     (the notebooks' small-p training sets)
    small5    100 fits at 166 x 24, H = 5, fp32 Y
    mid5       20 fits at 166 x 640, H = 5, fp32 Y
    wide5      20 fits at 166 x 3000, H = 5, fp32 Y
    mid5       once more with bf16 Y
    python scripts/fit_basic_batch_mil.py [--out profiles/fit_basic_batch_mil.txt]     (GPU box, repo root)"""
import copy
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G          # noqa: E402

pkg = G.load_package()
NITER, L = 50, 166
CASES = (("small1", 24, 1, 100, "fp32"), ("small5", 24, 5, 100, "fp32"), ("mid5", 640, 5, 20, "fp32"), ("wide5", 3000, 5, 20, "fp32"),
         ("mid5", 640, 5, 20, "bf16"))


def bags(M, H, n, seed):
    """one bag per fit (every fold's class is its own matrix): rank-H signal plus noise"""
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((L, H)) @ rng.standard_normal((H, M)) + 0.1 * rng.standard_normal((L, M)) for _ in range(n)]


def loop(Ys, ps):
    return [pkg.vbmf_(Y, p, NITER, eps=0.0, est_covs=True, est_var=True) for Y, p in zip(Ys, ps)]


def batch(Ys, ps):
    return pkg.vbmf_batch_(Ys, ps, NITER, eps=0.0, est_covs=True, est_var=True)


def timed(fn, Ys, ps0, reps=3):
    best, ps = np.inf, None
    for k in range(reps + 1):                                       # the first window warms up (context, code objects)
        ps = copy.deepcopy(ps0)
        pkg.invalidate()
        t0 = time.perf_counter()
        fn(Ys, ps)
        best = min(best, time.perf_counter() - t0) if k else best
    return best, ps


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "fit_basic_batch_mil.txt")
    lines = [f"basic-model fits of {NITER} sweeps (eps = 0, est_covs = est_var = true), L = {L}, one bag per fit; wall time per fit, best of 3 "
             "windows; loop: fp32-accumulate per-fit vbmf_, batch: fp64 vbmf_batch_",
             "case    M     H  Y     fits  loop ms/fit  batch ms/fit  ratio  max rel dBHat  verdict"]
    for name, M, H, n, yname in CASES:
        pkg.set_defaults(y_dtype=pkg.VBMF_Y_BF16 if yname == "bf16" else pkg.VBMF_Y_F32, factor_dtype=pkg.VBMF_FACTOR_AUTO)
        Ys = bags(M, H, n, 1)
        rng = np.random.default_rng(7)
        ps0 = [pkg.vbmf_init(Y, H, rng=rng) for Y in Ys]
        tl, pl = timed(loop, Ys, ps0)
        tb, pb = timed(batch, Ys, ps0)
        diff = max(np.linalg.norm(a.BHat - b.BHat) / np.linalg.norm(a.BHat) for a, b in zip(pl, pb))
        lines.append(f"{name:7s} {M:5d} {H:2d}  {yname}  {n:4d}  {1e3 * tl / n:11.3f}  {1e3 * tb / n:12.3f}  {tl / tb:5.1f}  {diff:13.2e}  "
                     + ("batch faster" if tb < tl else "BATCH NOT FASTER"))
        print(lines[-1], flush=True)
    pkg.set_defaults(y_dtype=pkg.VBMF_Y_F32, factor_dtype=pkg.VBMF_FACTOR_AUTO)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
