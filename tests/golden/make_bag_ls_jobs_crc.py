"""CRC-32s of what vbmf_bag_least_squares returns at the shapes of tests/test_gpu_classify_folds.py, recorded on the build of the
commit BEFORE vbmf_bag_least_squares_jobs and the refactor of csrc/score_kernels.hpp that came with it.

    python tests/golden/make_bag_ls_jobs_crc.py [OUT.json] [--commit ID]     (on an MI355X; default tests/golden/bag_ls_jobs_crc.json)

The fixture is made ONCE, on the parent build (its id goes into the file: --commit, or git's HEAD), and committed as it came out;
the test asserts that the old entry and every job of the new one reproduce it.  Never regenerate it from the code under test.

The inputs (cases(), shared with the test): _two_bases(H, 7100 + H, rows) of tests/test_gpu_classify_ls.py, eight bags per rank drawn
alternately from the two bases, widths WIDTHS, rounded to fp32; a context holds the bags of all its ranks side by side, so that every
bag meets bases of its own rank and of the others.  One record per (storage, L, H, basis 0 / 1, lambda): per bag of the context the
CRC-32 of its H x M_b block of X (column-major) and of its r2.
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

GOLDEN = os.path.join(ROOT, "tests", "golden", "bag_ls_jobs_crc.json")
WIDTHS = (1, 8, 9, 70, 3, 16, 17, 2)      # one column, one slice, one past a slice, many slices, a bag straddling a 32-column tile
LAMS = (0.0, 1e-2, 5.0)
# (storage, L) -> (the ranks whose bags and bases the context sees, the lambdas)
CONTEXTS = {("f32", 166): ((1, 5, 64), LAMS), ("bf16", 166): ((1, 5, 64), LAMS),
            ("f32", 300): ((5, 20), LAMS[:2]), ("f32", 33): ((5, 20), LAMS[:2])}


def _f32(Y):
    return Y.astype(np.float32).astype(np.float64)


def cases(two_bases):
    """(storage, L) -> dict(bases={H: [B0, B1]}, Ys=[the bags, eight per rank in the order of the ranks], drawn=[(H, k) per bag],
    lams).  two_bases: tests/test_gpu_classify_ls.py's _two_bases."""
    out = {}
    for (storage, L), (Hs, lams) in CONTEXTS.items():
        bases, Ys, drawn = {}, [], []
        for H in Hs:
            Bs, draw = two_bases(H, 7100 + H, rows=L)
            bases[H] = Bs
            for b, m in enumerate(WIDTHS):
                Ys.append(_f32(draw(b % 2, m)))
                drawn.append((H, b % 2))
        out[storage, L] = dict(bases=bases, Ys=Ys, drawn=drawn, lams=lams)
    return out


def key(storage, L, H, k, lam):
    return f"{storage}/L{L}/H{H}/B{k}/lam{lam:g}"


def crc(a):
    return "%08x" % (zlib.crc32(np.asfortranarray(a).tobytes(order="F")) & 0xFFFFFFFF)


def bag_crcs(X, r2, col_off):
    """[[CRC of the bag's block of X, CRC of its r2]] per bag"""
    return [[crc(X[:, c0:c1]), crc(r2[b:b + 1])] for b, (c0, c1) in enumerate(zip(col_off[:-1], col_off[1:]))]


def upload(pkg, storage, Ys):
    """(context of rank 1 holding the bags side by side, col_off)"""
    C = pkg.capi
    off = np.concatenate([[0], np.cumsum([Y.shape[1] for Y in Ys])]).astype(np.int64)
    c = C.Context(Ys[0].shape[0], int(off[-1]), 1, y_dtype=C.VBMF_Y_BF16 if storage == "bf16" else C.VBMF_Y_F32)
    c.set_Y(np.asfortranarray(np.hstack(Ys)))
    return c, off


def main():
    import __graft_entry__ as G
    from tests.test_gpu_classify_ls import _two_bases
    args = sys.argv[1:]
    commit = None
    if "--commit" in args:
        i = args.index("--commit")
        commit = args[i + 1]
        del args[i:i + 2]
    out = args[0] if args else GOLDEN
    G.build()
    pkg = G.load_package()
    if commit is None:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    rec = {}
    for (storage, L), case in cases(_two_bases).items():
        c, off = upload(pkg, storage, case["Ys"])
        with c:
            for H, Bs in case["bases"].items():
                for k, B in enumerate(Bs):
                    for lam in case["lams"]:
                        a, b = [bag_crcs(*c.bag_least_squares(off, B, lam), off) for _ in range(2)]
                        assert a == b, ("two runs on the parent build differ", storage, L, H, k, lam)
                        rec[key(storage, L, H, k, lam)] = a
                        print(key(storage, L, H, k, lam), a[3], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(dict(made_by_commit=commit, widths=list(WIDTHS), crc=rec), f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(rec)} records of {len(next(iter(rec.values())))}+ bags -> {out}")


if __name__ == "__main__":
    main()
