"""lambda_max of structured H x H matrices by the device kernel the run loop uses (vbmf_debug_lambda_max -> eig_kernel), as hex doubles:
the bitwise lock of tests/test_gpu_lambda_max_bits.py on the repeated squaring of H <= 64 (eig_squaring_dev, csrc/ctrl_kernels.hpp).

    VBMF_HIP_LIB=<parent build> python scripts/lambda_max_bits.py [OUT.json]
                                              (on an MI355X; default tests/golden/lambda_max_bits.json)

The fixture is made ONCE, on the build of the commit BEFORE the squaring took its wide form (upper triangle, two waves per SIMD),
loaded through VBMF_HIP_LIB, and committed as it came out; the test asserts it on the current build.  Never regenerate it from the
code under test.

Orders: both sides of every tier edge of the control kernels (R = 1: H <= 16, R = 2: H <= 32, R = 4: H <= 64) and orders whose rows
are padded.  Matrices: built from integers (and decimal literals), every entry one correctly rounded fp64 operation at the most, so
the inputs are the same bits on every host.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ORDERS = [2, 15, 16, 17, 31, 32, 33, 48, 63, 64]


def matrices(H):
    """name -> H x H fp64 matrix, in the order of the fixture."""
    i = np.arange(H, dtype=np.int64)
    out = {}
    # a dominant rank-one term over a small positive diagonal: gap of ~1e3, the squaring leaves its loop after two or three rounds
    u = (3 * i) % 4 + 1
    out["separated"] = (np.diag(1 + (7 * i) % 5) + 1000 * np.outer(u, u)).astype(np.float64)
    # two EQUAL top eigenvalues: p, q with disjoint supports, |q|^2 p p' + |p|^2 q q' + I has |p|^2 |q|^2 + 1 twice and ones: the
    # squaring converges to a rank-two projector, ||T^2||_F^2 -> 1/2, and all ten rounds run
    p = (i % 2 == 0).astype(np.int64)
    q = 1 - p
    out["double_top"] = (int(q @ q) * np.outer(p, p) + int(p @ p) * np.outer(q, q) + np.eye(H, dtype=np.int64)).astype(np.float64)
    w = (5 * i + 2) % 9 - 4
    w[w == 0] = 5
    out["rank_one"] = np.outer(w, w).astype(np.float64)
    out["zero"] = np.zeros((H, H))
    # ONE NaN entry, off the diagonal (the trace stays finite: the NaN goes through the squarings, not round the trace test), and
    # only on one side of it: the input is not symmetric
    nan = out["separated"].copy()
    nan[H - 1, 0] = np.nan
    out["one_nan"] = nan
    # eighteen decades on the diagonal plus a rank-one term
    d = np.array([float("1e%d" % (-8 + (7 * k) % 19)) for k in range(H)])
    v = (2 * i) % 5 - 2
    out["spread"] = np.diag(d) + np.outer(v, v).astype(np.float64)
    return out


def key(H, name):
    return "H%d/%s" % (H, name)


def lambda_hex(pkg):
    """key -> float.hex(lambda) ('nan' for a NaN) and the kernel time of each call, one tiny context per order."""
    capi = pkg.capi
    lam, us = {}, {}
    for H in ORDERS:
        with capi.Context(600, 300, H, y_dtype=capi.VBMF_Y_F32) as c:
            for name, Gm in matrices(H).items():
                v, t = c.lambda_max(Gm)
                lam[key(H, name)] = float(v).hex()
                us[key(H, name)] = t
    return lam, us


def main():
    import __graft_entry__ as G
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "lambda_max_bits.json")
    G.build()
    pkg = G.load_package()
    print("library:", pkg.capi.LIB_PATH, flush=True)
    lam, us = lambda_hex(pkg)
    for k in lam:
        print("%-22s %-26s %8.1f us" % (k, lam[k], us[k]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(lam, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
