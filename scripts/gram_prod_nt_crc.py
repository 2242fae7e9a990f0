"""CRC-32 of gram_prod_kernel's read-back [P | Q] on seeded inputs at the shapes of tests/test_gpu_gram_prod_nt.py: Grams on both
sides of GRAM_G_NT_BYTES (csrc/gram_kernels.hpp), above which the kernel streams G by non-temporal pieces.

    VBMF_HIP_LIB=<parent build> python scripts/gram_prod_nt_crc.py [OUT.json]
                                              (on an MI355X; default tests/golden/gram_prod_nt_crc.json)

The fixture is made ONCE, on the build of the commit BEFORE the kernel had a cache policy to choose (loaded through VBMF_HIP_LIB),
and committed as it came out; the test asserts it on the current build.  Never regenerate it from the code under test.  Inputs,
run and CRC are those of scripts/gram_prod_pq_crc.py (seeded_Y, run_pq, pq_crc).
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from gram_prod_pq_crc import key, pq_crc, run_pq, seeded_Y  # noqa: E402

# (L, M, H, what the shape is for): GT = 256 is the first Gram above the threshold, GT = 240 the last below it
CASES = [
    (600, 7700, 64, "NH 2, GT 256, non-temporal"),
    (600, 7700, 24, "NH 1, GT 256, non-temporal"),
    (600, 7600, 64, "NH 2, GT 240, default policy"),
]


def main():
    import __graft_entry__ as G
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "gram_prod_nt_crc.json")
    G.build()
    pkg = G.load_package()
    print("library:", pkg.capi.LIB_PATH, flush=True)
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
