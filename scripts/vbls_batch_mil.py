#!/usr/bin/env python3
"""vbls! over many bags in one device call (vbls_batch_, vbmf_run_fixed_basis_batched) at the MIL classifier's sizes
(examples/mil_util.jl:473-479: one vbls!(Y, copy_vbmf_params(Y, res), 150) per bag, thousands of small bags, one basis).
Per bag, end to end (parameter copies, upload, the iterations, read-back; a device synchronise inside every timed window):
the fp64 oracle on the host, per-bag vbls_ (one vbmf_run_fixed_basis call per bag), and vbls_batch_ (all bags in one call;
also on an already uploaded Bags, the classifier's second model).  The shapes of scripts/r03_vbls_mil.py plus 1024 bags of
166 x U(1, 40) at H = 5.
    python scripts/vbls_batch_mil.py              (GPU box, repo root)
    python scripts/vbls_batch_mil.py --profile    (the 1024-bag batched call only: run it under rocprofv3 --kernel-trace --stats)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G          # noqa: E402
from oracle import vbmf_oracle as O  # noqa: E402  (the checker, timed here as the CPU side)

pkg = G.load_package()
pkg.set_defaults(y_dtype=pkg.VBMF_Y_F32, factor_dtype=pkg.VBMF_FACTOR_AUTO)
NITER = 150


def setup(L, Mtrain, Ms, H, seed):
    rng = np.random.default_rng(seed)
    Bs = rng.standard_normal((L, H)) * np.linspace(1.0, 2.5, H)

    def draw(m):
        As = np.zeros((m, H)); As[np.arange(m), rng.integers(0, H, m)] = 1.0
        return Bs @ As.T + 0.05 * rng.standard_normal((L, m))
    Ytr = draw(Mtrain)
    res = O.vbmf_init(Ytr, H, ca=0.1, cb=0.1, sigma2=0.1, rng=np.random.default_rng(3), materialize_yhat=False)
    O.vbmf_(Ytr, res, 30, eps=0.0, est_covs=True, est_var=True)
    resg = pkg.vbmf_parameters()
    for f in ("L", "M", "H", "H1", "sigma2"):
        setattr(resg, f, getattr(res, f))
    resg.labels = np.zeros(0, dtype=np.int64)
    for f in ("AHat", "BHat", "SigmaB", "SigmaA", "CA", "CB", "invCA", "invCB"):
        setattr(resg, f, getattr(res, f).copy())
    return res, resg, [draw(int(m)) for m in Ms]


def batched(Ys, resg):
    ps = [pkg.copy_vbmf_params(Y, resg, rng=np.random.default_rng(1)) for Y in Ys]
    bags = pkg.Bags(Ys, resg.H)
    pkg.vbls_batch_(bags, ps, NITER)
    bags.ctx.sync()
    return ps, bags


def main():
    prof = "--profile" in sys.argv
    rng = np.random.default_rng(7)
    cases = [("L=166 M=6 H=2", 166, 400, [6] * 40, 2), ("L=166 M=30 H=5", 166, 400, [30] * 40, 5),
             ("L=230 M=60 H=10", 230, 600, [60] * 30, 10), ("L=1000 M=200 H=10", 1000, 2000, [200] * 10, 10),
             ("1024 bags L=166 M=U(1,40) H=5", 166, 400, rng.integers(1, 41, 1024), 5)]
    if prof:
        cases = cases[-1:]
    rows = []
    for name, L, Mtrain, Ms, H in cases:
        res, resg, Ys = setup(L, Mtrain, Ms, H, L + len(Ms))
        nb = len(Ys)
        batched(Ys[:2], resg)                                   # warm the library and the kernels
        if prof:
            for _ in range(3):
                batched(Ys, resg)
            print(f"profiled: 3 x vbls_batch_ over {nb} bags ({name})")
            return
        t0 = time.perf_counter()
        po = []
        for Y in Ys:
            p = O.copy_vbmf_params(Y, res, rng=np.random.default_rng(1))
            O.vbls_(Y, p, NITER)
            po.append(p)
        t_cpu = (time.perf_counter() - t0) / nb
        pkg.vbls_(Ys[0], pkg.copy_vbmf_params(Ys[0], resg, rng=np.random.default_rng(1)), NITER)
        t0 = time.perf_counter()
        pg = []
        for Y in Ys:
            p = pkg.copy_vbmf_params(Y, resg, rng=np.random.default_rng(1))
            pkg.vbls_(Y, p, NITER)
            pg.append(p)
        t_bag = (time.perf_counter() - t0) / nb
        pkg.invalidate()
        tb = []
        for _ in range(3):
            t0 = time.perf_counter()
            pb, bags = batched(Ys, resg)
            tb.append(time.perf_counter() - t0)
        t_bat = float(np.median(tb)) / nb
        ts = []                                                 # the same upload, another call (a second model's pass)
        for _ in range(3):
            ps = [pkg.copy_vbmf_params(Y, resg, rng=np.random.default_rng(1)) for Y in Ys]
            t0 = time.perf_counter()
            pkg.vbls_batch_(bags, ps, NITER)
            bags.ctx.sync()
            ts.append(time.perf_counter() - t0)
        t_up = float(np.median(ts)) / nb
        bags.close()
        err_o = max(np.linalg.norm(a.AHat - b.AHat) / np.linalg.norm(b.AHat) for a, b in zip(pb, po))
        err_b = max(np.linalg.norm(a.AHat - b.AHat) / np.linalg.norm(b.AHat) for a, b in zip(pb, pg))
        rows.append((name, nb, t_cpu, t_bag, t_bat, t_up, err_o, err_b))
    print(f"# vbls! x{NITER}, basic model, per BAG, end to end (ms)")
    print(f"{'case':32s} {'bags':>5s} {'oracle':>9s} {'vbls_':>9s} {'batch_':>9s} {'uploaded':>9s} {'vs vbls_':>9s} "
          f"{'vs oracle':>10s} {'relerr A (oracle)':>18s} {'(vbls_)':>9s}")
    for name, nb, tc, tg, tb, tu, eo, eb in rows:
        print(f"{name:32s} {nb:5d} {tc * 1e3:9.4f} {tg * 1e3:9.4f} {tb * 1e3:9.4f} {tu * 1e3:9.4f} {tg / tb:8.1f}x {tc / tb:9.1f}x "
              f"{eo:18.2e} {eb:9.2e}")


if __name__ == "__main__":
    main()
