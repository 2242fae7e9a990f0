"""CRC-32 of gram_prod_kernel's read-back [P | Q] (PEEK_GRAM_PQ) on seeded inputs, one entry per shape of CASES.

    python scripts/gram_prod_pq_crc.py [OUT.json]          (on an MI355X; default tests/golden/gram_prod_pq_crc.json)

The product is pinned bit for bit by its split plan and its order of additions, so a rework of the kernel's
geometry or pipeline must reproduce these CRCs.  The fixture is made ONCE, on the build of the commit BEFORE such a rework, and
committed as it came out; tests/test_gpu_gram_prod_overlap.py asserts it on the current build.  Never regenerate it from the code
under test.

Each case: integer Y (exact in bf16), VBMF_GRAM=1, run(1) as a streaming sweep that builds G and W, run(1) again as one Gram-form
sweep, then [P | Q] as fp32 words.
"""
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# (L, M, H, what the shape is for): the shapes of tests/test_gpu_gram_prod_overlap.py
CASES = [
    (600, 250, 24, "NH 1, one row group, second half past XT1"),
    (600, 500, 24, "NH 1, one row group"),
    (600, 4568, 24, "NH 1, last split 2"),
    (600, 2870, 64, "NH 2, second half past XT1, last split 2"),
    (600, 3544, 64, "NH 2, last split 3"),
    (600, 2050, 128, "NH 4, second half past XT1"),
    (600, 3086, 128, "NH 4, sps odd"),
    (600, 16400, 128, "NH 4, one split"),
]


def key(L, M, H):
    return f"{L}x{M}xH{H}"


def seeded_Y(L, M, H):
    return np.random.default_rng(7100 + M + H).integers(-3, 4, size=(L, M)).astype(np.float64)


def run_pq(pkg, Y, H, seed):
    """one streaming sweep (builds G, W), one Gram-form sweep; the read-back product and what the checks need beside it"""
    from oracle import vbmf_oracle as O
    L, M = Y.shape
    cap = pkg.capi
    po = O.vbmf_init(Y, H, ca=0.1, cb=0.1, sigma2=0.1, rng=np.random.default_rng(seed), materialize_yhat=False)
    old = os.environ.get("VBMF_GRAM")
    os.environ["VBMF_GRAM"] = "1"
    try:
        c = cap.Context(L, M, H, y_dtype=pkg.VBMF_Y_BF16, factor_dtype=pkg.VBMF_FACTOR_BF16X2)
    finally:
        if old is None:
            del os.environ["VBMF_GRAM"]
        else:
            os.environ["VBMF_GRAM"] = old
    with c:
        c.set_Y(Y)
        c.set_state(po.AHat, po.BHat, po.SigmaA, po.SigmaB, np.diag(po.CA), np.diag(po.CB), po.sigma2)
        c.run(1, eps=0.0, est_covs=True, est_var=True)
        d = c.dims()
        assert d["gram"] == 1 and d["gram_built"] == 1
        Hp, XT = d["Hp"], d["XT1"]
        GT = (XT + 15) // 16 * 16
        nW = 32 * GT * Hp
        W0 = c.peek(cap.PEEK_GRAM_W, nW, dtype=np.float32).reshape(-1, Hp).astype(np.float64)
        c.run(1, eps=0.0, est_covs=True, est_var=True)
        W1 = c.peek(cap.PEEK_GRAM_W, nW, dtype=np.float32).reshape(-1, Hp).astype(np.float64)
        n = Hp * XT * 32
        PQ = c.peek(cap.PEEK_GRAM_PQ, 2 * n, dtype=np.float32)
        Ys = c.get_Y()
        d = c.dims()
    return dict(GT=GT, XT=XT, Hp=Hp, NH=d["NH"], nsplit=d["gram_nsplit"], Ys=Ys, W0=W0, W1=W1, PQ=PQ, n=n)


def pq_crc(PQ):
    return "%08x" % (zlib.crc32(np.ascontiguousarray(PQ, dtype=np.float32).view(np.uint8).tobytes()) & 0xFFFFFFFF)


def main():
    import __graft_entry__ as G
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "gram_prod_pq_crc.json")
    G.build()
    pkg = G.load_package()
    crcs = {}
    for L, M, H, what in CASES:
        r = run_pq(pkg, seeded_Y(L, M, H), H, 7200 + M)
        crcs[key(L, M, H)] = pq_crc(r["PQ"])
        print(key(L, M, H), what, "NH", r["NH"], "nsplit", r["nsplit"], crcs[key(L, M, H)], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(crcs, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
