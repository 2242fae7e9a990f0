"""CRC-32s of what the tail of the Gram-form product leaves (gram_tail_kernel, gram_part_reduce_kernel) on
seeded inputs, one entry per shape of CASES: the folded [P | Q] (PEEK_GRAM_PQ, all 2 n floats) and the state's
[B'B | dB'dB | tr(B'YA)] (PEEK_STATE, 2 Hp^2 + 1 doubles).

    python scripts/gram_tail_state_crc.py [OUT.json] [--commit ID]     (on an MI355X; default tests/golden/gram_tail_state_crc.json)

Fold order, step order, subset order and chunk order of these sums are pinned, so a rework of the kernels must reproduce the CRCs.
The fixture is made ONCE, on the build of the commit BEFORE such a rework (its id goes into the file: --commit, or git's HEAD),
and committed as it came out; tests/test_gpu_gram_tail.py asserts it on the current build.  Never regenerate it from the code
under test.

Each case: integer Y (exact in bf16), VBMF_GRAM=1, run(1) as a streaming sweep that builds G and W, run(1) again as one Gram-form
sweep (scripts/gram_prod_pq_crc.py does the same for the product alone).
"""
import json
import os
import subprocess
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

L = 600
# (M, H, what the shape is for)
CASES = [
    (61, 24, "Hp 32, one chunk"),
    (353, 64, "Hp 64, 6 chunks, last 33 rows, padding rows"),
    (353, 100, "Hp 128, 6 chunks, last 33 rows, padding rows"),
    (2357, 64, "Hp 64, 37 chunks, padding rows"),
    (2357, 24, "Hp 32, 37 chunks, padding rows"),
    (2357, 100, "Hp 128, 37 chunks, padding rows"),
]


def key(M, H):
    return f"{L}x{M}xH{H}"


def seeded_Y(M, H):
    return np.random.default_rng(8100 + M + H).integers(-3, 4, size=(L, M)).astype(np.float64)


def chunk_plan(M, H):
    """the host's chunk plan (gram_prepare: g_nchunk, g_rpc) and the kernel's geometry (GPart<HP>)"""
    Hp = 32 if H <= 32 else (64 if H <= 64 else 128)
    nchunk = max(1, min(64 if Hp == 128 else 128, -(-M // 64)))
    rpc = -(-(-(-M // nchunk)) // 16) * 16
    nchunk = -(-M // rpc)
    V = Hp // 16
    return dict(Hp=Hp, V=V, S=8 // V, nchunk=nchunk, rpc=rpc, last=M - (nchunk - 1) * rpc)


def run_tail(pkg, Y, H, seed):
    """one streaming sweep (builds G, W), one Gram-form sweep; [P | Q], the state's slots and what the checks need beside them"""
    from oracle import vbmf_oracle as O
    Lr, M = Y.shape
    cap = pkg.capi
    po = O.vbmf_init(Y, H, ca=0.1, cb=0.1, sigma2=0.1, rng=np.random.default_rng(seed), materialize_yhat=False)
    old = os.environ.get("VBMF_GRAM")
    os.environ["VBMF_GRAM"] = "1"
    try:
        c = cap.Context(Lr, M, H, y_dtype=pkg.VBMF_Y_BF16, factor_dtype=pkg.VBMF_FACTOR_BF16X2)
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
        W0 = c.peek(cap.PEEK_GRAM_W, nW, dtype=np.float32).reshape(-1, Hp).copy()
        c.run(1, eps=0.0, est_covs=True, est_var=True)
        W1 = c.peek(cap.PEEK_GRAM_W, nW, dtype=np.float32).reshape(-1, Hp).copy()
        n = Hp * XT * 32
        PQ = c.peek(cap.PEEK_GRAM_PQ, 2 * n, dtype=np.float32).copy()
        A32 = c.peek(cap.PEEK_A32, M * Hp, dtype=np.float32).reshape(M, Hp).copy()
        n2 = Hp * Hp
        st = c.peek(cap.PEEK_STATE, 2 * (3 * n2 + 1), dtype=np.float64).copy()
        d = c.dims()
    return dict(XT=XT, Hp=Hp, nsplit=d["gram_nsplit"], W0=W0, W1=W1, A=A32, PQ=PQ, n=n, slots=st[n2:3 * n2 + 1].copy())


def crc(a):
    return "%08x" % (zlib.crc32(np.ascontiguousarray(a).view(np.uint8).tobytes()) & 0xFFFFFFFF)


def main():
    import __graft_entry__ as G
    args = sys.argv[1:]
    commit = None
    if "--commit" in args:
        i = args.index("--commit")
        commit = args[i + 1]
        del args[i:i + 2]
    if commit is None:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    out = args[0] if args else os.path.join(ROOT, "tests", "golden", "gram_tail_state_crc.json")
    G.build()
    pkg = G.load_package()
    cases = {}
    for M, H, what in CASES:
        r = run_tail(pkg, seeded_Y(M, H), H, 8200 + M)
        cases[key(M, H)] = dict(pq=crc(r["PQ"]), state=crc(r["slots"]))
        print(key(M, H), what, "nsplit", r["nsplit"], cases[key(M, H)], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(dict(made_by_commit=commit, cases=cases), f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
