#!/usr/bin/env python3
"""vbls! of the ARD-sparse models over many bags in one device call (vbls_sparse_batch_, vbmf_sparse_run_fixed_basis_batched) at
the MIL classifier's sizes, in its two forms: the sparse model's diagonal updateA! x150 (examples/mil_util.jl:469-479) and the
two-group model's full_cov updateA! x20 (:514-521).  Per bag, end to end (parameter copies, upload, the iterations, read-back; a
device synchronise inside every timed window): the fp64 oracle on the host, per-bag vbls_ (one vbmf_sparse_run_fixed_basis call
per bag), and vbls_sparse_batch_ (all bags in one call; also on an already uploaded SparseBags, the classifier's second model).
The shapes of scripts/vbls_batch_mil.py: four MIL shapes plus 1024 bags of 166 x U(1, 40) at H = 5.  The oracle and per-bag
vbls_ are timed on the first 128 bags of a case at most (per-bag vbls_ in the diagonal form on those with M_b >= 2: the single-bag path
refuses one column under the QS1 layout); the oracle's full_cov form (a dense M H x M H inverse) only up to M H = 1600,
the classifier's own gate (examples/mil_util.jl:393-416).
    python scripts/vbls_sparse_batch_mil.py              (GPU box, repo root)
    python scripts/vbls_sparse_batch_mil.py --profile    (the 1024-bag batched calls only: run it under rocprofv3 --kernel-trace --stats)
    python scripts/vbls_sparse_batch_mil.py --score a|b  (the whole classifier step, examples/mil_util.jl:453-535, on 256 bags of
        166 x 30 at H = 5 against two models, per bag amortised, one warm-up and five timed windows per classifier.  a: the batched
        fits, then the scores one bag at a time -- NumPy residuals, lowerBound / lowerBoundTrimmed through a context per bag; it uses
        nothing newer than the batched fits, so it also runs on a build without the scoring entries.  b: classify_batch.  With
        --profile: three classify_batch calls per classifier and no timing, for rocprofv3 --kernel-trace --stats.
        The least-squares classifiers "ols", "rls" and "min_err" (:457-468, :493-501) run at the same shape.  a: inv(B'B)*B'*Y and
        the residual per bag in NumPy on the host, for min_err the batched fits and NumPy residuals.  b: classify_bags, for
        ols / rls also on bags uploaded once.
        --algs ols,rls,min_err restricts either to the named classifiers)"""
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
FORMS = (("sparse diagonal x150", "sparse", 150, False), ("dual full_cov x20", "dual", 20, True))
NSUB = 128


def setup(kind, L, Mtrain, Ms, H, seed):
    """an oracle-trained model of the family, its package twin, and the bags"""
    rng = np.random.default_rng(seed)
    Bs = rng.standard_normal((L, H)) * np.linspace(1.0, 2.5, H)

    def draw(m):
        As = np.zeros((m, H)); As[np.arange(m), rng.integers(0, H, m)] = 1.0
        return Bs @ As.T + 0.05 * rng.standard_normal((L, m))
    Ytr = draw(Mtrain)
    r = np.random.default_rng(3)
    if kind == "sparse":
        res = O.vbmf_sparse_init(Ytr, H, rng=r, full_cov=False, materialize_yhat=False)
        O.vbmf_sparse_(Ytr, res, 20, eps=0.0)
        resg = pkg.vbmf_sparse_parameters()
    else:
        res = O.vbmf_dual_init(Ytr, H, max(1, H // 2), rng=r, materialize_yhat=False)
        O.vbmf_dual_(Ytr, res, 20, eps=0.0, est_priors=False)
        resg = pkg.vbmf_dual_parameters()
    for f in resg.__dataclass_fields__:
        if hasattr(res, f):
            v = getattr(res, f)
            setattr(resg, f, v.copy() if isinstance(v, np.ndarray) else v)
    return res, resg, [draw(int(m)) for m in Ms]


def oracle_one(Y, p, kind, niter, full_cov):
    if not full_cov:
        return O.vbls_sparse_(Y, p, niter) if kind == "sparse" else O.vbls_dual_(Y, p, niter)
    for _ in range(niter):
        if kind == "dual":
            O.dual_updateA(Y, p, full_cov=True)
            O.dual_updateCA(p)
        else:
            O.sparse_updateA(Y, p, full_cov=True)
            O.sparse_updateCA(p)
        O.sparse_updateSigma(Y, p)


def oracle_params(p, kind):
    q = (O.vbmf_sparse_parameters if kind == "sparse" else O.vbmf_dual_parameters)()
    for f in q.__dataclass_fields__:
        if hasattr(p, f):
            v = getattr(p, f)
            setattr(q, f, v.copy() if isinstance(v, np.ndarray) else v)
    return q


def batched(Ys, resg, niter, full_cov):
    ps = [pkg.copy_vbmf_params(Y, resg, rng=np.random.default_rng(1)) for Y in Ys]
    bags = pkg.SparseBags(Ys, resg.H)
    pkg.vbls_sparse_batch_(bags, ps, niter, full_cov=full_cov)
    bags.ctx.sync()
    return ps, bags


def relA(a, b):
    return np.linalg.norm(a.ATVecHat - b.ATVecHat) / np.linalg.norm(b.ATVecHat)


def score_models(L, H, H1):
    """two trained models per family (bags come alternately from their bases), as the package's types"""
    rng = np.random.default_rng(11)
    Bs = [rng.standard_normal((L, H)) * np.linspace(1.0, 2.5, H) for _ in range(2)]

    def draw(k, m):
        As = np.zeros((m, H)); As[np.arange(m), rng.integers(0, H, m)] = 1.0
        return Bs[k] @ As.T + 0.05 * rng.standard_normal((L, m))

    def twin(cls, res):
        out = cls()
        for f in out.__dataclass_fields__:
            if hasattr(res, f):
                v = getattr(res, f)
                setattr(out, f, v.copy() if isinstance(v, np.ndarray) else v)
        return out
    models = {"vbls": [], "dual": [], "lower_bound": []}
    for k in range(2):
        Ytr = draw(k, 400)
        r = O.vbmf_init(Ytr, H, ca=0.1, cb=0.1, sigma2=0.1, rng=np.random.default_rng(3 + k), materialize_yhat=False)
        O.vbmf_(Ytr, r, 15, eps=0.0, est_covs=True, est_var=True)
        b = twin(pkg.vbmf_parameters, r)
        b.labels = np.zeros(0, dtype=np.int64)
        models["vbls"].append(b)
        r = O.vbmf_dual_init(Ytr, H, max(1, H // 2), rng=np.random.default_rng(5 + k), materialize_yhat=False)
        O.vbmf_dual_(Ytr, r, 20, eps=0.0, est_priors=False)
        models["dual"].append(twin(pkg.vbmf_dual_parameters, r))
        r = O.vbmf_sparse_init(Ytr, H, rng=np.random.default_rng(7 + k), full_cov=False, materialize_yhat=False)
        O.vbmf_sparse_(Ytr, r, 20, eps=0.0)
        s = twin(pkg.vbmf_sparse_parameters, r)
        s.H1 = H1
        models["lower_bound"].append(s)
    return models, draw


def classify_per_bag_scores(res0, res1, Ys, alg, threshold=1e-1):
    """classify over many bags with the batched fits and the scores one bag at a time (what a build without the scoring entries does)"""
    L = Ys[0].shape[0]
    if alg in ("ols", "rls"):                                          # the reference's own per-bag expressions, :159-171, :483-484
        errs = []
        for res in (res0, res1):
            B = res.BHat
            lam = np.eye(B.shape[1]) * (0.0 if alg == "ols" else 1e-2)
            errs.append(np.array([np.linalg.norm(Y - B @ (np.linalg.inv(B.T @ B + lam) @ B.T @ Y)) for Y in Ys]))
        return (errs[0] > errs[1]).astype(np.int64), errs[0], errs[1]
    if alg in ("lower_bound", "min_err"):
        H, H0 = res0.H, res0.H - res0.H1
        ps0 = []
        for Y in Ys:
            p = pkg.vbmf_sparse_init(Y, H0)
            p.BHat, p.SigmaB, p.CB = res0.BHat[:, :H0].copy(), res0.SigmaB[:H0, :H0].copy(), res0.CB[:H0].copy()
            p.gamma, p.delta = res0.gamma, res0.delta[:H0].copy()
            ps0.append(p)
        ps1 = [pkg.copy_vbmf_params(Y, res0) for Y in Ys]
        full_cov = Ys[0].shape[1] * H0 < 1600                          # (one bag size here: one group)
        pkg.vbls_sparse_batch_(Ys, ps0, 20, full_cov=full_cov)
        pkg.vbls_sparse_batch_(Ys, ps1, 20, full_cov=full_cov)
        if alg == "min_err":
            e0, e1 = (np.array([np.linalg.norm(Y - p.BHat @ p.AHat.T) for Y, p in zip(Ys, ps)]) for ps in (ps0, ps1))
            return np.where(np.abs((e0 - e1) / e0) < threshold, 0, 1), e0, e1
        e0 = np.array([pkg.lowerBound(Y, p) for Y, p in zip(Ys, ps0)])
        e1 = np.array([pkg.lowerBoundTrimmed(Y, p, threshold) for Y, p in zip(Ys, ps1)])
        return (e1 > e0).astype(np.int64), e0, e1
    errs = []
    bags = pkg.Bags(Ys, res0.H) if alg == "vbls" else pkg.SparseBags(Ys, res0.H)
    for res in (res0, res1):
        ps = [pkg.copy_vbmf_params(Y, res) for Y in Ys]
        if alg == "vbls":
            pkg.vbls_batch_(bags, ps, 150)
        else:
            pkg.vbls_sparse_batch_(bags, ps, 20, full_cov=True)
        errs.append(np.array([np.linalg.norm(Y - p.BHat @ p.AHat.T) for Y, p in zip(Ys, ps)]))
    bags.close()
    if alg == "vbls":
        return (errs[0] > errs[1]).astype(np.int64), errs[0], errs[1]
    e0, e1 = errs[0] / (L * Ys[0].shape[1]), errs[1] / (L * Ys[0].shape[1])
    return np.where(e0 < e1, 0, 1), e0, e1


def score_main(how, prof):
    L, M, H, H1, nb = 166, 30, 5, 2, 256
    models, draw = score_models(L, H, H1)
    Ys = [draw(b % 2, M).astype(np.float32).astype(np.float64) for b in range(nb)]
    algs = ("vbls", "dual", "lower_bound", "ols", "rls", "min_err")
    if "--algs" in sys.argv:
        algs = tuple(sys.argv[sys.argv.index("--algs") + 1].split(","))
    models["ols"] = models["rls"] = models["vbls"]                     # classify reads nothing but their BHat
    models["min_err"] = models["lower_bound"]
    print(f"# classify over {nb} bags of {L} x {M} at H = {H}, two models, per BAG amortised (ms): "
          + ("(a) batched fits, scores one bag at a time; ols / rls per bag in NumPy" if how == "a"
             else "(b) classify_batch; ols / rls / min_err: classify_bags"))
    print(f"{'classifier':12s} {'median':>9s} {'min':>9s} {'max':>9s} {'label 1':>8s}")
    for alg in algs:
        res0, res1 = models[alg]
        batch = pkg.classify_batch if alg in ("vbls", "dual", "lower_bound") else getattr(pkg, "classify_bags", None)
        run = ((lambda: classify_per_bag_scores(res0, res1, Ys, alg)) if how == "a"
               else (lambda: batch(res0, res1, Ys, alg)))
        labels, _, _ = run()                                            # warm-up: library, kernels, allocator
        if prof:
            for _ in range(3):
                run()
            print(f"profiled: 3 x {batch.__name__} {alg}")
            continue
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            run()
            ts.append((time.perf_counter() - t0) / nb * 1e3)
        pkg.invalidate()
        print(f"{alg:12s} {np.median(ts):9.4f} {min(ts):9.4f} {max(ts):9.4f} {int(np.sum(labels)):8d}")
        if how == "b" and alg in ("ols", "rls"):                        # the same on bags uploaded once (the two device calls alone)
            bags = pkg.Bags(Ys, H)
            ts = []
            for _ in range(6):
                t0 = time.perf_counter()
                batch(res0, res1, bags, alg)
                ts.append((time.perf_counter() - t0) / nb * 1e3)
            bags.close()
            print(f"{alg + ' uploaded':12s} {np.median(ts[1:]):9.4f} {min(ts[1:]):9.4f} {max(ts[1:]):9.4f} {int(np.sum(labels)):8d}")


def main():
    prof = "--profile" in sys.argv
    if "--score" in sys.argv:
        return score_main(sys.argv[sys.argv.index("--score") + 1], prof)
    rng = np.random.default_rng(7)
    cases = [("L=166 M=6 H=2", 166, 400, [6] * 40, 2), ("L=166 M=30 H=5", 166, 400, [30] * 40, 5),
             ("L=230 M=60 H=10", 230, 600, [60] * 30, 10), ("L=1000 M=200 H=10", 1000, 2000, [200] * 10, 10),
             ("1024 bags L=166 M=U(1,40) H=5", 166, 400, rng.integers(1, 41, 1024), 5)]
    if prof:
        cases = cases[-1:]
    for form, kind, niter, full_cov in FORMS:
        rows = []
        for name, L, Mtrain, Ms, H in cases:
            res, resg, Ys = setup(kind, L, Mtrain, Ms, H, L + len(Ms))
            nb = len(Ys)
            batched(Ys[:2], resg, niter, full_cov)                  # warm the library and the kernels
            if prof:
                for _ in range(3):
                    batched(Ys, resg, niter, full_cov)
                print(f"profiled: 3 x vbls_sparse_batch_ over {nb} bags ({name}, {form})")
                continue
            sub = Ys[:NSUB]
            t_cpu, po = float("nan"), None
            if not full_cov or max(Y.shape[1] for Y in sub) * H <= 1600:
                t0 = time.perf_counter()
                po = []
                for Y in sub:
                    p = oracle_params(pkg.copy_vbmf_params(Y, resg, rng=np.random.default_rng(1)), kind)
                    oracle_one(Y, p, kind, niter, full_cov)
                    po.append(p)
                t_cpu = (time.perf_counter() - t0) / len(sub)
            # (the single-bag diagonal form refuses a 1-column bag under the QS1 layout: those bags are left out of its timing)
            dev = [b for b, Y in enumerate(sub) if full_cov or Y.shape[1] >= 2]
            pkg.vbls_(sub[dev[0]], pkg.copy_vbmf_params(sub[dev[0]], resg, rng=np.random.default_rng(1)), niter, full_cov=full_cov)
            t0 = time.perf_counter()
            pg = []
            for Y in (sub[b] for b in dev):
                p = pkg.copy_vbmf_params(Y, resg, rng=np.random.default_rng(1))
                pkg.vbls_(Y, p, niter, full_cov=full_cov)
                pg.append(p)
            t_bag = (time.perf_counter() - t0) / len(dev)
            pkg.invalidate()
            tb = []
            for _ in range(3):
                t0 = time.perf_counter()
                pb, bags = batched(Ys, resg, niter, full_cov)
                tb.append(time.perf_counter() - t0)
            t_bat = float(np.median(tb)) / nb
            ts = []                                                 # the same upload, another call (a second model's pass)
            for _ in range(3):
                ps = [pkg.copy_vbmf_params(Y, resg, rng=np.random.default_rng(1)) for Y in Ys]
                t0 = time.perf_counter()
                pkg.vbls_sparse_batch_(bags, ps, niter, full_cov=full_cov)
                bags.ctx.sync()
                ts.append(time.perf_counter() - t0)
            t_up = float(np.median(ts)) / nb
            bags.close()
            err_o = max(relA(a, b) for a, b in zip(pb, po)) if po else float("nan")
            err_b = max(relA(pb[b], g) for b, g in zip(dev, pg))
            rows.append((name, nb, t_cpu, t_bag, t_bat, t_up, err_o, err_b))
        if prof:
            continue
        print(f"# vbls! {form} ({kind} model), per BAG, end to end (ms)")
        print(f"{'case':32s} {'bags':>5s} {'oracle':>9s} {'vbls_':>9s} {'batch_':>9s} {'uploaded':>9s} {'vs vbls_':>9s} "
              f"{'vs oracle':>10s} {'relerr A (oracle)':>18s} {'(vbls_)':>9s}")
        for name, nb, tc, tg, tb, tu, eo, eb in rows:
            print(f"{name:32s} {nb:5d} {tc * 1e3:9.4f} {tg * 1e3:9.4f} {tb * 1e3:9.4f} {tu * 1e3:9.4f} {tg / tb:8.1f}x "
                  f"{tc / tb:9.1f}x {eo:18.2e} {eb:9.2e}")
        print()


if __name__ == "__main__":
    main()
