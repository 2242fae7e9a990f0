#!/usr/bin/env python3
"""Many three-group / label-masked sparse fits in one device call (vbmf_trial_batch_, vbmf_sparse_masked_batch_; vbmf_local_fit_batched)
at the MIL training loop's sizes on concatenated matrices [Y0 Y1] (src/vbmf_trial.jl:528-604; train_local, examples/mil_util.jl:302-320),
against the loop of per-fit vbmf_trial_ / vbmf_sparse_ calls from the SAME initialisations.  Fixed 50 sweeps on both sides (eps = 0),
fp32 and bf16 storage of Y, wall time per fit end to end (parameter copies, upload, the sweeps, read-back; every call synchronises
before it returns):
    trial20   2 matrices x 10 starts at 166 x 640, M0 = 320, H = 5, H0 = 3, three-group model, full_cov
    trial100  10 matrices x 10 starts of the first case
    masked10  1 matrix x 10 starts at 166 x 3000, M0 = 1500, H = 5, H1 = 2, masked sparse model, diagonal form
    python scripts/fit_local_batch_mil.py [--out profiles/fit_local_batch_mil.txt]     (GPU box, repo root)"""
import copy
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G          # noqa: E402

pkg = G.load_package()
NITER, NSTARTS, L, H, H0, H1 = 50, 10, 166, 5, 3, 2
CASES = (("trial20", "trial", 640, 320, 2, True), ("trial100", "trial", 640, 320, 10, True), ("masked10", "masked", 3000, 1500, 1, False))


def bags(M, M0, Hneg, nbags, seed):
    """[Y0 Y1]: every column one scaled basis vector plus noise; the first M0 columns (the negative instances) use the first Hneg only"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(nbags):
        Bs = rng.standard_normal((L, H)) * np.linspace(1.0, 2.5, H)
        which = np.concatenate([rng.integers(0, Hneg, M0), rng.integers(0, H, M - M0)])
        As = np.zeros((M, H)); As[np.arange(M), which] = 1.0
        out.append(Bs @ As.T + 0.05 * rng.standard_normal((L, M)))
    return out


def starts(kind, Ys, M0):
    rng = np.random.default_rng(7)
    init = ((lambda Y: pkg.vbmf_trial_init(Y, H, H0, M0, rng=rng)) if kind == "trial" else
            (lambda Y: pkg.vbmf_sparse_init(Y, H, H1=H1, labels=np.arange(1, M0 + 1), rng=rng)))
    bag_of = [b for b in range(len(Ys)) for _ in range(NSTARTS)]
    return [init(Ys[b]) for b in bag_of], bag_of


def loop(kind, Ys, ps, bag_of, full_cov):
    fit = pkg.vbmf_trial_ if kind == "trial" else pkg.vbmf_sparse_
    return [fit(Ys[b], p, NITER, eps=0.0, full_cov=full_cov) for p, b in zip(ps, bag_of)]


def batch(kind, Ys, ps, bag_of, full_cov):
    fit = pkg.vbmf_trial_batch_ if kind == "trial" else pkg.vbmf_sparse_masked_batch_
    return fit(Ys, ps, NITER, eps=0.0, full_cov=full_cov, bag_of=bag_of)


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
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "fit_local_batch_mil.txt")
    lines = [f"fits of {NITER} sweeps (eps = 0), L = {L}, H = {H}, {NSTARTS} starts per matrix; wall time per fit, best of 3 windows",
             "case      Y     fits  loop ms/fit  batch ms/fit  ratio  max rel dBHat  verdict"]
    for ydt, yname in ((pkg.VBMF_Y_F32, "fp32"), (pkg.VBMF_Y_BF16, "bf16")):
        pkg.set_defaults(y_dtype=ydt, factor_dtype=pkg.VBMF_FACTOR_AUTO)
        for name, kind, M, M0, nb, full_cov in CASES:
            Ys = bags(M, M0, H0 if kind == "trial" else H - H1, nb, 1)
            ps0, bag_of = starts(kind, Ys, M0)
            tl, pl = timed(loop, kind, Ys, ps0, bag_of, full_cov)
            tb, pb = timed(batch, kind, Ys, ps0, bag_of, full_cov)
            diff = max(np.linalg.norm(a.BHat - b.BHat) / np.linalg.norm(a.BHat) for a, b in zip(pl, pb))
            n = len(ps0)
            lines.append(f"{name:9s} {yname}  {n:4d}  {1e3 * tl / n:11.3f}  {1e3 * tb / n:12.3f}  {tl / tb:5.1f}  {diff:13.2e}  "
                         + ("batch faster" if tb < tl else "BATCH NOT FASTER"))
            print(lines[-1], flush=True)
    pkg.set_defaults(y_dtype=pkg.VBMF_Y_F32, factor_dtype=pkg.VBMF_FACTOR_AUTO)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
