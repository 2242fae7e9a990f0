#!/usr/bin/env python3
"""The one parity case of tests/test_gpu_fit_split.py whose figures exceed 1.8e-12 -- the masked diagonal homoscedastic fit at
(L, M_b, H) = (100, 40, 32) from start seed 3 -- run in BOTH forms of vbmf_ard_fit_batched_form against the fp64 oracle, beside the
second start seed of that case: is the distance the split schedule's or the case's?
    python scripts/fit_split_outlier.py [--out profiles/fit_split_outlier.txt]     (GPU box, repo root)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as G          # noqa: E402
import test_gpu_fit_split as T       # noqa: E402  (its _bag, _start, _oracle, Call and _rel)

FIELDS = (("BHat", "BHat"), ("SigmaB", "SigmaB"), ("sigmaHat", "sigmaHat"), ("zeta", "zeta"), ("beta", "beta"), ("ATVecHat", "ATVecHat"))


def main():
    G.build()
    pkg = G.load_package()
    L, M, H = 100, 40, 32
    call = T.Call(pkg, [T._bag(L, M, H, L + M + H)], H)
    lines = [f"masked diagonal homoscedastic fit at (L, M_b, H) = ({L}, {M}, {H}), M0 = {M // 2}, H1 = 1, 6 sweeps, eps = 0, fp32 storage: "
             "relative error per field against the fp64 oracle",
             "seed form    " + " ".join(f"{k:>9s}" for k, _ in FIELDS) + "   oracle zeta  ||Y||^2 / 2"]
    try:
        for seed in (3, 0):
            st = [T._start("masked", call.Ys[0], H, seed)]
            po = T._oracle("masked", call.Ys[0], st[0], 6, 0.0, False, False)[0]
            for form in ("split", "stream"):
                r = call.run("masked", st, [0], 6, 0.0, False, False, form=form, slice_cols=8 if form == "split" else None)
                vals = [T._rel(r[k][0] if r[k].ndim and len(r[k]) == 1 else r[k], getattr(po, name)) for k, name in FIELDS]
                lines.append(f"{seed:4d} {form:7s} " + " ".join(f"{v:9.2e}" for v in vals)
                             + f"  {float(po.zeta):12.4f} {0.5 * float((call.Ys[0] ** 2).sum()):12.4f}")
                print(lines[-1], flush=True)
    finally:
        call.close()
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "fit_split_outlier.txt")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
