"""Launches of gram_prod_kernel at the headline shape (100 000 x 10 000, H = 64, bf16 Y) for builds whose product is wrong on
purpose (-DVBMF_GRAMPROD_PROBE=1|2, csrc/gram_kernels.hpp), to be read from a kernel trace:

    VBMF_HIP_LIB=<build> rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/gram_prod_probe_time.py [N]

bench.py cannot time such a build: a wrong [P | Q] sends the stop test's d to zero or NaN and the run ends after its first sweep,
and a stopped run's gram_prod returns at once.  Here every launch follows a fresh, valid state: set_state, then run(2) = one
streaming sweep (which forms W from that state) and one Gram-form sweep, whose gram_prod therefore does all its work on finite
operands whatever it then stores.  N such rounds (default 40); the trace's average over the gram_prod launches is the figure.
Compare builds only under this script: the clocks here are not those of a run of back-to-back Gram sweeps."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    import __graft_entry__ as G
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    pkg = G.load_package()
    capi = pkg.capi
    L, M, H = 100000, 10000, 64
    ctx = capi.Context(L, M, H, y_dtype=pkg.VBMF_Y_BF16, factor_dtype=pkg.VBMF_FACTOR_BF16X2)
    with ctx:
        ctx.set_Y_synthetic(20170101, H, 0.05)
        rng = np.random.default_rng(20170102)
        A0, B0 = rng.standard_normal((M, H)), rng.standard_normal((L, H))
        z, c = np.zeros((H, H)), 0.1 * np.ones(H)
        its = []
        for _ in range(n):
            ctx.set_state(A0, B0, z, z, c, c, 0.1)
            it, d, _ = ctx.run(2, eps=0.0, est_covs=True, est_var=True)
            its.append(it)
        ctx.sync()
        dm = ctx.dims()
    print("library", capi.LIB_PATH, "rounds", n, "sweeps per round", sorted(set(its)), "gram", dm["gram"], "nsplit", dm["gram_nsplit"])


if __name__ == "__main__":
    main()
