#!/usr/bin/env python3
"""Many ARD-sparse / two-group fits in one device call (vbmf_sparse_batch_, vbmf_dual_batch_; vbmf_sparse_fit_batched) at the MIL
training loop's sizes (examples/mil_util.jl:93-152, :327-385, :670-788), against the loop of per-fit vbmf_sparse_ / vbmf_dual_ calls
from the SAME initialisations.  Fixed 50 sweeps on both sides (eps = 0), bf16 and fp32 storage of Y, wall time per fit end to end
(parameter copies, upload, the sweeps, read-back; every call synchronises before it returns):
    dual20    2 classes x 10 starts at 166 x 640, H = 5, H0 = 2, two-group model, full_cov
    sparse20  2 classes x 10 starts at 166 x 3000, H = 5, sparse model, diagonal form
    dual100   5 folds x 2 classes x 10 starts of the first case
    python scripts/fit_batch_mil.py [--out profiles/fit_batch_mil.txt]     (GPU box, repo root)
    python scripts/fit_batch_mil.py --profile batch|loop                   (dual20 and sparse20 once each, fp32 storage, no timing: run it
                                                                            under rocprofv3 --kernel-trace --stats for the kernel time)
    python scripts/fit_batch_mil.py --diag-var [--out profiles/fit_rows_batch_mil.txt]
        the same three cases under the heteroscedastic noise model (diag_var=True on both sides, examples/mil_util.jl:667; the bags' noise
        runs from 0.05 to 0.4 down the rows): vbmf_rows_fit_batched against the loop of per-fit calls.  These fits do not settle in 50
        sweeps, so the two sides' BHat are not compared; the last column is the fewest sweeps a batched fit ran (50: none stopped early)"""
import copy
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G          # noqa: E402

pkg = G.load_package()
NITER, NSTARTS, L, H = 50, 10, 166, 5
DIAG_VAR = "--diag-var" in sys.argv
ROWS = dict(diag_var=True) if DIAG_VAR else {}
CASES = (("dual20", "dual", 640, 2, True), ("sparse20", "sparse", 3000, 2, False), ("dual100", "dual", 640, 10, True))


def bags(M, nbags, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(nbags):
        Bs = rng.standard_normal((L, H)) * np.linspace(1.0, 2.5, H)
        As = np.zeros((M, H)); As[np.arange(M), rng.integers(0, H, M)] = 1.0
        std = np.linspace(0.05, 0.4, L)[:, None] if DIAG_VAR else 0.05
        out.append(Bs @ As.T + std * rng.standard_normal((L, M)))
    return out


def starts(kind, Ys):
    rng = np.random.default_rng(7)
    init = (lambda Y: pkg.vbmf_sparse_init(Y, H, rng=rng)) if kind == "sparse" else (lambda Y: pkg.vbmf_dual_init(Y, H, 2, rng=rng))
    bag_of = [b for b in range(len(Ys)) for _ in range(NSTARTS)]
    return [init(Ys[b]) for b in bag_of], bag_of


def loop(kind, Ys, ps, bag_of, full_cov):
    fit = pkg.vbmf_sparse_ if kind == "sparse" else pkg.vbmf_dual_
    return [fit(Ys[b], p, NITER, eps=0.0, full_cov=full_cov, **ROWS) for p, b in zip(ps, bag_of)]


def batch(kind, Ys, ps, bag_of, full_cov):
    fit = pkg.vbmf_sparse_batch_ if kind == "sparse" else pkg.vbmf_dual_batch_
    return fit(Ys, ps, NITER, eps=0.0, full_cov=full_cov, bag_of=bag_of, **ROWS)


def timed(fn, kind, Ys, ps0, bag_of, full_cov, reps=3):
    best, ps = np.inf, None
    for _ in range(reps + 1):                                       # the first window warms up (context, code objects)
        ps = copy.deepcopy(ps0)
        pkg.invalidate()
        t0 = time.perf_counter()
        fn(kind, Ys, ps, bag_of, full_cov)
        best = min(best, time.perf_counter() - t0) if _ else best
    return best, ps


def main():
    if "--profile" in sys.argv:
        which = sys.argv[sys.argv.index("--profile") + 1]
        pkg.set_defaults(y_dtype=pkg.VBMF_Y_F32, factor_dtype=pkg.VBMF_FACTOR_AUTO)
        for name, kind, M, nb, full_cov in CASES[:2]:
            Ys = bags(M, nb, 1)
            ps, bag_of = starts(kind, Ys)
            (batch if which == "batch" else loop)(kind, Ys, ps, bag_of, full_cov)
        return
    name = "fit_rows_batch_mil.txt" if DIAG_VAR else "fit_batch_mil.txt"
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", name)
    lines = [f"fits of {NITER} sweeps (eps = 0), L = {L}, H = {H}, {NSTARTS} starts per bag; wall time per fit, best of 3 windows"
             + ("; diag_var=True on both sides" if DIAG_VAR else ""),
             "case      Y     fits  loop ms/fit  batch ms/fit  ratio  " + ("batch sweeps >= " if DIAG_VAR else "max rel dBHat") + "  verdict"]
    for ydt, yname in ((pkg.VBMF_Y_F32, "fp32"), (pkg.VBMF_Y_BF16, "bf16")):
        pkg.set_defaults(y_dtype=ydt, factor_dtype=pkg.VBMF_FACTOR_AUTO)
        for name, kind, M, nb, full_cov in CASES:
            Ys = bags(M, nb, 1)
            ps0, bag_of = starts(kind, Ys)
            tl, pl = timed(loop, kind, Ys, ps0, bag_of, full_cov)
            tb, pb = timed(batch, kind, Ys, ps0, bag_of, full_cov)
            diff = max(np.linalg.norm(a.BHat - b.BHat) / np.linalg.norm(a.BHat) for a, b in zip(pl, pb))
            n = len(ps0)
            last = f"{min(p.iters for p in pb):13d}" if DIAG_VAR else f"{diff:13.2e}"
            lines.append(f"{name:9s} {yname}  {n:4d}  {1e3 * tl / n:11.3f}  {1e3 * tb / n:12.3f}  {tl / tb:5.1f}  {last}  "
                         + ("batch faster" if tb < tl else "BATCH NOT FASTER"))
            print(lines[-1], flush=True)
    pkg.set_defaults(y_dtype=pkg.VBMF_Y_F32, factor_dtype=pkg.VBMF_FACTOR_AUTO)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
