"""CRC-32s of what vbmf_fixed_basis_jobs and vbmf_sparse_scored_jobs return on fixed inputs, recorded on the build of the commit BEFORE
the job bookkeeping of csrc/host_bags.hpp moved into csrc/job_tables.hpp.

    python tests/golden/make_job_calls_crc.py [OUT.json] [--commit ID]     (on an MI355X; default tests/golden/job_calls_crc.json)

The fixture is made ONCE, on the parent build (its id goes into the file: --commit, or git's HEAD), and committed as it came out;
tests/test_gpu_job_calls_bits.py asserts that this build reproduces it.  Never regenerate it from the code under test.

The inputs (shared with the test) follow make_vbls_jobs_crc.py: NumPy's PCG64 stream through element-wise arithmetic and indexing
only.  Two calls, chosen for what the index table and the offsets have to get right:
  fixed_basis_jobs    models of H = 5, 16, 17, 32 in one call (both tiers), L = 33, bags of WIDTHS columns -- every (bag, model) pair --
                      and two more bags, fixed_basis_jobs_lds_cols(32) columns and one more, against the H = 32 model (P in LDS, P in
                      scratch); the jobs shuffled, the first few repeated at the end
  sparse_scored_jobs  models of H = 5 (sparse priors) and 17 (dual priors), the same widths and one bag on each side of
                      vbls_jobs_lds_cols(17, False) against the H = 17 model, both in the diagonal form (the limit is that form's) and
                      in the full form (where both spill); the form and the trim (-1 or 0.1) vary from job to job,
                      so all four (tier, form) groups have jobs (the 1-column bag in the full form only); shuffled, with repeats
One record per call: per job, in the order of the job list, the CRC-32 of each field.
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
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import make_vbls_jobs_crc as V  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "job_calls_crc.json")
L = 33
NITER = 20
WIDTHS = (1, 2, 3, 8, 9, 17, 70)
BASIC_H = (5, 16, 17, 32)
BASIC_FIELDS = ("AHat", "SigmaA", "CA", "sigma2", "r2", "status")
SCORED_H = (5, 17)
SCORED_FIELDS = V.FIELDS + ("r2", "lb", "status")
NREPEAT = 5


def crc(a, dtype=np.float64):
    return "%08x" % (zlib.crc32(np.ascontiguousarray(np.asarray(a, dtype=dtype)).tobytes()) & 0xFFFFFFFF)


def _shuffled(jobs, seed):
    jobs = [jobs[i] for i in np.random.default_rng(seed).permutation(len(jobs))]
    return jobs + jobs[:NREPEAT]


def basic_case(lds32):
    """(the models' arrays, the bags, the jobs as (bag, model)); lds32 = fixed_basis_jobs_lds_cols(32)"""
    base = [V.model(L, H, 9100 + H, False) for H in BASIC_H]
    mods = [dict(BHat=m["BHat"], SigmaB=m["SigmaB"], sigma2_0=0.01, ca0=1.0) for m in base]
    rng = np.random.default_rng(9600)
    Ys = [V.draw(base[b % len(base)], w, rng) for b, w in enumerate(WIDTHS)]
    Ys += [V.draw(base[-1], w, rng) for w in (lds32, lds32 + 1)]
    nw, last = len(WIDTHS), len(BASIC_H) - 1
    jobs = [(b, k) for b in range(nw) for k in range(len(mods))] + [(nw, last), (nw + 1, last)]
    return mods, Ys, _shuffled(jobs, 9601)


def scored_case(lds17):
    """(the models' arrays, the bags, the jobs as (bag, model, full_cov, trim)); lds17 = vbls_jobs_lds_cols(17, False)"""
    mods = []
    for i, H in enumerate(SCORED_H):
        m = V.model(L, H, 9200 + H, dual=bool(i))
        rng = np.random.default_rng(9300 + H)
        mods.append(dict(m, CB=rng.uniform(0.5, 2.0, H), delta=rng.uniform(0.5, 2.0, H), gamma=1.0 + L / 2, gamma0=1.0, delta0=1.0,
                         a_pri=m["alpha"] - 0.5, b_pri=m["beta0"], a_post=m["alpha"]))
    rng = np.random.default_rng(9700)
    Ys = [V.draw(mods[b % 2], w, rng) for b, w in enumerate(WIDTHS)]
    Ys += [V.draw(mods[1], w, rng) for w in (lds17, lds17 + 1)]
    nw = len(WIDTHS)
    pairs = [(b, k) for b in range(nw) for k in range(2)] + [(nw, 1), (nw + 1, 1)]
    # the form alternates within each model's jobs and the trim every other pair: every (model, form) meets both trims
    # (the 1-column bag in the full form only: the diagonal form under VBMF_COMPAT_SPARSE_REPEAT, the default, needs M >= 2)
    jobs = [(b, k, bool((i // 2) % 2) or Ys[b].shape[1] < 2, -1.0 if (i // 4) % 2 else 0.1) for i, (b, k) in enumerate(pairs)]
    # the index rule gives the two boundary bags the full form (where both spill: that form's own limit is lower); here they run in
    # the diagonal form, whose limit lds17 is: the state of one in LDS, of the other in scratch
    jobs += [(nw, 1, False, 0.1), (nw + 1, 1, False, -1.0)]
    return mods, Ys, _shuffled(jobs, 9701)


def run_basic(pkg):
    mods, Ys, jobs = basic_case(pkg.capi.fixed_basis_jobs_lds_cols(32))
    c, off = V.upload(pkg, Ys)
    with c:
        r = c.fixed_basis_jobs(off, mods, [q[0] for q in jobs], [q[1] for q in jobs], NITER)
    return r, jobs


def run_scored(pkg):
    mods, Ys, jobs = scored_case(pkg.capi.vbls_jobs_lds_cols(17, False))
    c, off = V.upload(pkg, Ys)
    with c:
        r = c.sparse_scored_jobs(off, mods, [q[0] for q in jobs], [q[1] for q in jobs], [q[2] for q in jobs], [q[3] for q in jobs], NITER)
    return r, jobs


def basic_crcs(r, j):
    return [crc(r[f][j:j + 1], np.int64) if f == "status" else crc(r[f][j:j + 1]) if f in ("sigma2", "r2") else crc(r[f][j])
            for f in BASIC_FIELDS]


def scored_crcs(r, j):
    """V.job_crcs gives FIELDS and r2"""
    return V.job_crcs(r, j) + [crc(r["lb"][j:j + 1]), crc(r["status"][j:j + 1], np.int64)]


CALLS = {"fixed_basis_jobs": (run_basic, basic_crcs, BASIC_FIELDS), "sparse_scored_jobs": (run_scored, scored_crcs, SCORED_FIELDS)}


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
    for name, (run, crcs, fields) in CALLS.items():
        (ra, jobs), (rb, _) = run(pkg), run(pkg)
        assert not ra["status"].any() and not rb["status"].any(), (name, ra["status"], rb["status"])
        a, b = [[crcs(r, j) for j in range(len(jobs))] for r in (ra, rb)]
        assert a == b, ("two runs on the parent build differ", name)
        rec[name] = dict(fields=list(fields), jobs=[list(map(float, q)) for q in jobs], crc=a)
        print(name, len(jobs), "jobs", a[0], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(dict(made_by_commit=commit, widths=list(WIDTHS), calls=rec), f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(rec)} records -> {out}")


if __name__ == "__main__":
    main()
