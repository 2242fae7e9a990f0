"""CRC-32s of what vbmf_sparse_fixed_basis_jobs and lowerBound_batch / lowerBoundTrimmed_batch return on fixed inputs, recorded on the
build of the commit BEFORE vbmf_sparse_scored_jobs and the changes to csrc/vbls_jobs_kernels.hpp and csrc/score_kernels.hpp that came
with it.

    python tests/golden/make_vbls_jobs_crc.py [OUT.json] [--commit ID]     (on an MI355X; default tests/golden/vbls_jobs_crc.json)

The fixture is made ONCE, on the parent build (its id goes into the file: --commit, or git's HEAD), and committed as it came out;
tests/test_gpu_scored_jobs.py asserts that the old entry, the shared jobs of the new one and the bound's sums reproduce it.  Never
regenerate it from the code under test.

The inputs (shared with the test) come from NumPy's PCG64 stream through element-wise arithmetic and indexing only -- no matrix
product, no LAPACK -- so that every machine builds the same bits: per (L, H) two models (a basis of normal draws scaled per column, a
diagonal SigmaB, the ARD shapes and rates of a sparse and of a dual set) and bags of WIDTHS columns, each column one basis column
plus noise 0.05, rounded to fp32.  One record per (form, L, H): per job, in the order of jobs(), the CRC-32 of each of FIELDS and of
r2.  bound_inputs() is one model and four bags with states drawn the same way; its record holds the CRC-32 of lowerBound_batch's
and of lowerBoundTrimmed_batch(0.1)'s results.
"""
import json
import os
import subprocess
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "vbls_jobs_crc.json")
FIELDS = ("ATVecHat", "diagSigmaATVec", "CA", "beta", "SigmaA", "sigmaHat", "zeta")
WIDTHS = (3, 2, 8, 9, 17, 70)
SHAPES = ((33, 5), (300, 17))
NITER = 20


def _f32(Y):
    return Y.astype(np.float32).astype(np.float64)


def model(L, H, seed, dual):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((L, H)) * np.linspace(1.0, 2.5, H)
    SB = np.diag(rng.uniform(0.5, 2.0, H) / 1024.0)
    first = np.arange(H) < (max(1, H // 2) if dual else H)
    alpha = np.where(first, 0.5 + 1e-10, 0.5 + 0.25)
    beta0 = np.where(first, 1e-10, 0.125)
    return dict(BHat=B, SigmaB=SB, alpha=alpha, beta0=beta0, eta0=1e-10, zeta0=1e-10, sigma0=1.0, ca0=1.0)


def draw(m, width, rng):
    B = m["BHat"]
    cols = rng.integers(0, B.shape[1], width)
    return _f32(B[:, cols] + 0.05 * rng.standard_normal((B.shape[0], width)))


def case(L, H, full):
    """(the two models' arrays, the bags, the jobs as (bag, model))"""
    mods = [model(L, H, 9000 + 10 * H + L, False), model(L, H, 9001 + 10 * H + L, True)]
    rng = np.random.default_rng(9500 + H)
    widths = ((1,) if full else ()) + WIDTHS
    Ys = [draw(mods[b % 2], w, rng) for b, w in enumerate(widths)]
    return mods, Ys, [(b, k) for b in range(len(Ys)) for k in range(2)]


def key(L, H, full):
    return f"{'full' if full else 'diag'}/L{L}/H{H}"


def crc(a):
    return "%08x" % (zlib.crc32(np.ascontiguousarray(np.asarray(a, dtype=np.float64)).tobytes()) & 0xFFFFFFFF)


def job_crcs(r, j):
    """r: what Context.sparse_fixed_basis_jobs returns (or the same blocks of Context.sparse_scored_jobs)"""
    out = []
    for f in FIELDS:
        if f in ("sigmaHat", "zeta"):
            out.append(crc(r[f][j:j + 1]))
        elif f == "SigmaA":
            out.append(crc(r[f][j]))
        else:
            out.append(crc(r[f][r["off"][j]:r["off"][j + 1]]))
    return out + [crc(r["r2"][j:j + 1])]


def upload(pkg, Ys):
    C = pkg.capi
    off = np.concatenate([[0], np.cumsum([Y.shape[1] for Y in Ys])]).astype(np.int64)
    c = C.Context(Ys[0].shape[0], int(off[-1]), 1, y_dtype=C.VBMF_Y_F32)
    c.set_Y(np.asfortranarray(np.hstack(Ys)))
    return c, off


def bound_inputs(pkg):
    """(the bags, one filled vbmf_sparse_parameters per bag) for lowerBound_batch"""
    L, H = 33, 5
    m = model(L, H, 9700, False)
    rng = np.random.default_rng(9701)
    p = pkg.vbmf_sparse_init(np.zeros((L, 3)), H, rng=np.random.default_rng(0))
    p.BHat, p.SigmaB = m["BHat"], m["SigmaB"]
    p.CB, p.delta = rng.uniform(0.5, 2.0, H), rng.uniform(0.5, 2.0, H)
    Ys, qs = [], []
    for w in (3, 1, 8, 17):
        Y = draw(m, w, rng)
        q = pkg.copy_vbmf_params(Y, p, rng=np.random.default_rng(1))
        q.ATVecHat = rng.standard_normal(w * H) * 0.3
        q.AHat = q.ATVecHat.reshape(w, H)
        q.diagSigmaATVec = rng.uniform(0.01, 0.5, w * H)
        q.CA, q.beta = rng.uniform(0.5, 4.0, w * H), rng.uniform(0.1, 2.0, w * H)
        q.SigmaA = np.diag(rng.uniform(0.1, 1.0, H))
        q.sigmaHat, q.zeta = float(rng.uniform(100.0, 400.0)), float(rng.uniform(0.1, 1.0))
        Ys.append(Y)
        qs.append(q)
    return Ys, qs


def main():
    import __graft_entry__ as G
    args = sys.argv[1:]
    commit = None
    if "--commit" in args:
        i = args.index("--commit")
        commit = args[i + 1]
        del args[i:i + 2]
    out = args[0] if args else GOLDEN
    G.build()
    pkg = G.load_package()
    pkg.set_defaults(y_dtype=pkg.VBMF_Y_F32, factor_dtype=pkg.VBMF_FACTOR_AUTO)
    if commit is None:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    rec = {}
    for L, H in SHAPES:
        for full in (False, True):
            mods, Ys, jobs = case(L, H, full)
            c, off = upload(pkg, Ys)
            with c:
                run = lambda: c.sparse_fixed_basis_jobs(off, H, mods, [b for b, _ in jobs], [k for _, k in jobs], NITER, full_cov=full)
                ra, rb = run(), run()
            assert not ra["status"].any(), (L, H, full, ra["status"])
            a, b = [[job_crcs(r, j) for j in range(len(jobs))] for r in (ra, rb)]
            assert a == b, ("two runs on the parent build differ", L, H, full)
            rec[key(L, H, full)] = a
            print(key(L, H, full), a[0], flush=True)
    Ys, qs = bound_inputs(pkg)
    lb, lt = pkg.lowerBound_batch(Ys, qs), pkg.lowerBoundTrimmed_batch(Ys, qs, 1e-1)
    assert np.all(np.isfinite(lb)) and np.all(np.isfinite(lt)) and np.any(lb != lt), (lb, lt)
    rec["lowerBound_batch"] = [crc(lb), crc(lt)]
    print("lowerBound_batch", lb, lt, rec["lowerBound_batch"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(dict(made_by_commit=commit, widths=list(WIDTHS), crc=rec), f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(rec)} records -> {out}")


if __name__ == "__main__":
    main()
