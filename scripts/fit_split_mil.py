#!/usr/bin/env python3
"""One wide ARD-family fit over many workgroups (form="split" of vbmf_*_batch_; vbmf_ard_fit_batched_form) at the MIL training loop's
sizes, in the manner of scripts/fit_batch_mil.py: L = 166, H = 5, 50 sweeps with eps = 0, the same initialisations on every side, fp32
storage of Y, wall time per fit end to end (parameter copies, upload, the sweeps, read-back; every call synchronises before it returns).
Every shape is warmed up, the sides are alternated in one process, best of three windows.  The stream side and the split side are each
run twice; a side's spread is the relative difference between its two bests, and `spread` -- the noise floor every verdict is read
against -- is the larger of the two.
Sides: loop = the per-fit vbmf_sparse_ / vbmf_dual_ calls; stream = the one-workgroup batch (form="stream", the default); split =
form="split"; auto = form="auto".
    python scripts/fit_split_mil.py [--out profiles/fit_split_mil.txt]      the acceptance table
    python scripts/fit_split_mil.py --tune [--out ...]                      slice_cols 64 / 128 / 256 / 512 on the 20-fit cases
    python scripts/fit_split_mil.py --widths [--out ...]                    20 fits at M_b = 160 .. 3000, stream against split, per form
    python scripts/fit_split_mil.py --profile split|stream                  sparse 2 x 166 x 3000 and dual 2 x 166 x 640 once each, no timing: run
                                                                            under rocprofv3 --kernel-trace --stats for the kernel times
VBMF_FIT_SPLIT_CHUNK in the environment overrides the sweeps enqueued between two reads of the done words (the header's constant)."""
import copy
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G          # noqa: E402

pkg = G.load_package()
NITER, L, H = 50, 166, 5
# name, kind, M_b, bags, starts per bag, full_cov, diag_var
CASES = (("sparse2", "sparse", 3000, 2, 1, False, False), ("sparse20", "sparse", 3000, 2, 10, False, False),
         ("masked10", "masked", 3000, 10, 1, False, False), ("dual2", "dual", 640, 2, 1, True, False),
         ("dual20", "dual", 640, 2, 10, True, False), ("dual100", "dual", 640, 10, 10, True, False),
         ("sparse20r", "sparse", 3000, 2, 10, False, True), ("dual20r", "dual", 640, 2, 10, True, True))


def bags(M, nbags, seed, rows):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(nbags):
        Bs = rng.standard_normal((L, H)) * np.linspace(1.0, 2.5, H)
        As = np.zeros((M, H)); As[np.arange(M), rng.integers(0, H, M)] = 1.0
        std = np.linspace(0.05, 0.4, L)[:, None] if rows else 0.05
        out.append(Bs @ As.T + std * rng.standard_normal((L, M)))
    return out


def starts(kind, Ys, nstarts):
    rng = np.random.default_rng(7)
    bag_of = [b for b in range(len(Ys)) for _ in range(nstarts)]
    if kind == "dual":
        return [pkg.vbmf_dual_init(Ys[b], H, 2, rng=rng) for b in bag_of], bag_of
    if kind == "masked":                                            # train_local: the first half of the columns is Y0, H1 = 1
        return [pkg.vbmf_sparse_init(Ys[b], H, H1=1, labels=np.arange(1, Ys[b].shape[1] // 2 + 1), rng=rng) for b in bag_of], bag_of
    return [pkg.vbmf_sparse_init(Ys[b], H, rng=rng) for b in bag_of], bag_of


def run(side, kind, Ys, ps, bag_of, full_cov, rows, slice_cols=None):
    kw = dict(diag_var=True) if rows else {}
    if side == "loop":
        fit = pkg.vbmf_dual_ if kind == "dual" else pkg.vbmf_sparse_
        return [fit(Ys[b], p, NITER, eps=0.0, full_cov=full_cov, **kw) for p, b in zip(ps, bag_of)]
    fit = {"dual": pkg.vbmf_dual_batch_, "masked": pkg.vbmf_sparse_masked_batch_, "sparse": pkg.vbmf_sparse_batch_}[kind]
    if side != "stream":
        kw.update(form=side, slice_cols=slice_cols)
    return fit(Ys, ps, NITER, eps=0.0, full_cov=full_cov, bag_of=bag_of, **kw)


def timed(sides, kind, Ys, ps0, bag_of, full_cov, rows, reps=3):
    """sides: (label, side, slice_cols); the windows of the sides are interleaved, the first round warms up.  Returns {label: (best, ps)}"""
    best, last = {k: np.inf for k, _, _ in sides}, {}
    for r in range(reps + 1):
        for label, side, sc in sides:
            ps = copy.deepcopy(ps0)
            pkg.invalidate()
            t0 = time.perf_counter()
            run(side, kind, Ys, ps, bag_of, full_cov, rows, sc)
            dt = time.perf_counter() - t0
            if r:
                best[label] = min(best[label], dt)
            last[label] = ps
    return {k: (best[k], last[k]) for k in best}


def table():
    lines = [f"fits of {NITER} sweeps (eps = 0), L = {L}, H = {H}, fp32 storage; wall ms per fit, best of 3 interleaved windows; "
             f"slice_cols = {pkg.capi.VBMF_FIT_SPLIT_COLS}, chunk = {os.environ.get('VBMF_FIT_SPLIT_CHUNK', pkg.capi.VBMF_FIT_SPLIT_CHUNK)}",
             "r = diag_var; spread = max(|stream - stream'| / stream, |split - split'| / split); dB = max rel ||BHat_split - BHat_stream||",
             "case       M_b  fits     loop   stream  stream'    split   split'     auto  spread  split/stream  split/loop  auto form        dB  verdict"]
    for name, kind, M, nb, ns, full_cov, rows in CASES:
        Ys = bags(M, nb, 1, rows)
        ps0, bag_of = starts(kind, Ys, ns)
        sides = [("loop", "loop", None), ("stream", "stream", None), ("split", "split", None), ("auto", "auto", None),
                 ("again", "stream", None), ("split2", "split", None)]
        t = timed(sides, kind, Ys, ps0, bag_of, full_cov, rows)
        n = len(ps0)
        tl, tb, tc, td, tb2, tc2 = (t[k][0] for k in ("loop", "stream", "split", "auto", "again", "split2"))
        spread = max(abs(tb - tb2) / tb, abs(tc - tc2) / tc)
        diff = max(np.linalg.norm(a.BHat - b.BHat) / np.linalg.norm(b.BHat) for a, b in zip(t["split"][1], t["stream"][1]))
        forms = sorted({p.form for p in t["auto"][1]})
        win = tc < min(tl, tb) * (1 - spread)
        reg = td > min(tb, tc) * (1 + spread)
        lines.append(f"{name:9s} {M:5d} {n:5d} {1e3 * tl / n:8.3f} {1e3 * tb / n:8.3f} {1e3 * tb2 / n:8.3f} {1e3 * tc / n:8.3f} {1e3 * tc2 / n:8.3f} "
                     f"{1e3 * td / n:8.3f} {spread:7.3f} "
                     f"{tb / tc:13.2f} {tl / tc:11.2f}  {str(forms):9s} {diff:9.2e}  "
                     + ("split beats both" if win else "split does NOT beat both") + ("; AUTO SLOWER than the better form" if reg else ""))
        print(lines[-1], flush=True)
    return lines


def tune():
    lines = [f"slice_cols on the 20-fit cases: {NITER} sweeps, L = {L}, H = {H}, fp32; wall ms per fit, best of 3 interleaved windows; "
             f"chunk = {os.environ.get('VBMF_FIT_SPLIT_CHUNK', pkg.capi.VBMF_FIT_SPLIT_CHUNK)}",
             "case       M_b  fits   stream      64     128     256     512    128 again"]
    for name, kind, M, nb, ns, full_cov, rows in (c for c in CASES if c[0] in ("sparse20", "dual20")):
        Ys = bags(M, nb, 1, rows)
        ps0, bag_of = starts(kind, Ys, ns)
        sides = [("stream", "stream", None)] + [(str(sc), "split", sc) for sc in (64, 128, 256, 512)] + [("again", "split", 128)]
        t = timed(sides, kind, Ys, ps0, bag_of, full_cov, rows)
        n = len(ps0)
        lines.append(f"{name:9s} {M:5d} {n:5d} " + " ".join(f"{1e3 * t[k][0] / n:8.3f}" for k in ("stream", "64", "128", "256", "512", "again")))
        print(lines[-1], flush=True)
    return lines


def widths():
    lines = [f"20 fits (2 bags x 10 starts), {NITER} sweeps, L = {L}, H = {H}, fp32; wall ms per fit, best of 3 interleaved windows; "
             f"slice_cols = {pkg.capi.VBMF_FIT_SPLIT_COLS}",
             "form       M_b   stream    split  spread  stream/split"]
    for kind, full_cov in (("sparse", False), ("dual", True)):
        for M in (160, 320, 640, 1280, 3000):
            Ys = bags(M, 2, 1, False)
            ps0, bag_of = starts(kind, Ys, 10)
            t = timed([("stream", "stream", None), ("split", "split", None), ("again", "stream", None)], kind, Ys, ps0, bag_of, full_cov, False)
            tb, tc, tb2 = (t[k][0] for k in ("stream", "split", "again"))
            lines.append(f"{'full_cov' if full_cov else 'diagonal':9s} {M:5d} {1e3 * tb / 20:8.3f} {1e3 * tc / 20:8.3f} {abs(tb - tb2) / tb:7.3f} "
                         f"{tb / tc:13.2f}")
            print(lines[-1], flush=True)
    return lines


def main():
    pkg.set_defaults(y_dtype=pkg.VBMF_Y_F32, factor_dtype=pkg.VBMF_FACTOR_AUTO)
    if "--profile" in sys.argv:
        side = sys.argv[sys.argv.index("--profile") + 1]
        for name, kind, M, nb, ns, full_cov, rows in (CASES[0], CASES[3]):
            Ys = bags(M, nb, 1, rows)
            ps, bag_of = starts(kind, Ys, ns)
            run(side, kind, Ys, ps, bag_of, full_cov, rows)
        return
    mode = "tune" if "--tune" in sys.argv else "widths" if "--widths" in sys.argv else "table"
    default = {"table": "fit_split_mil.txt", "tune": "fit_split_tune.txt", "widths": "fit_split_widths.txt"}[mode]
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", default)
    lines = {"table": table, "tune": tune, "widths": widths}[mode]()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
