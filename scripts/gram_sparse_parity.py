#!/usr/bin/env python3
"""Measured parity of the Gram-form sweep of vbmf_sparse_run ("The ARD-sparse model"): every case of
tests/test_gpu_gram_sparse.py::test_parity_with_oracle_and_streaming -- the Gram-form run and the streaming run against the fp64
oracle on the stored Y, and against each other -- one line per case and field: value and bound.
    python scripts/gram_sparse_parity.py [--out profiles/gram_sparse_parity.txt]     (GPU box, repo root)
--h256: the rank-256 form instead (H = 130 / 200 / 256 at M = 1040 / 1024 / 1024, the form taken through vbmf_set_gram_form:
tests/test_gpu_gram_sparse_h256.py's measure_parity), APPENDED to --out."""
import argparse
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G                                  # noqa: E402
from tests import test_gpu_gram_sparse as T                  # noqa: E402
from tests import test_gpu_gram_sparse_h256 as T256          # noqa: E402

H256_SHAPES = [(130, 1040), (200, 1024), (256, 1024)]


class Env:
    """monkeypatch's two calls, on os.environ"""
    @staticmethod
    def setenv(k, v):
        os.environ[k] = v

    @staticmethod
    def delenv(k):
        os.environ.pop(k, None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gram_sparse_parity.txt"))
    ap.add_argument("--h256", action="store_true")
    a = ap.parse_args()
    G.build()
    pkg = G.load_package()
    if a.h256:
        os.environ.pop("VBMF_GRAM", None)
        lines = ["", "# Rank 256 (Hp = 256; vbmf_set_gram_form(VBMF_GRAM_FORM_ON) against VBMF_GRAM_FORM_OFF of the same build): the same figures"]
        shapes, measure = H256_SHAPES, lambda *c: T256.measure_parity(pkg, *c)
    else:
        lines = ["# Gram-form sweep of vbmf_sparse_run: measured parity (scripts/gram_sparse_parity.py).  Per case and field: the Gram-form run",
                 "# against the fp64 oracle | the streaming run against the oracle | Gram form against streaming | the bound",
                 "# (d_tr: |d - d_ref| / (2e-2 d_ref + 2e-6), worst sweep; the other figures are relative errors)"]
        shapes, measure = T.PARITY_SHAPES, lambda *c: T.measure_parity(pkg, Env, *c)
    worst = {}
    for (H, M), labels, est_cb, compat in itertools.product(shapes, (False, True), (True, False), (False, True)):
        m, _, _ = measure(H, M, labels, est_cb, compat)
        lines.append(f"{7 * M}x{M} H={H} labels={int(labels)} est_cb={int(est_cb)} layout={'repeat, 3 sweeps' if compat else 'consistent, 6 sweeps'}")
        for k, (vg, vs, vgs, b) in m.items():
            lines.append(f"    {k:16s} gram {vg:.3e}  streaming {vs:.3e}  gram-streaming {vgs:.3e}  bound {b:.1e}"
                         + ("" if vs <= b else "  (streaming beyond the bound)"))
            w = worst.setdefault(k, [0.0, 0.0, 0.0, b])
            w[0], w[1], w[2] = max(w[0], vg), max(w[1], vs), max(w[2], vgs)
        print(lines[-len(m) - 1], flush=True)
    lines.append("worst over the cases")
    for k, (vg, vs, vgs, b) in worst.items():
        lines.append(f"    {k:16s} gram {vg:.3e}  streaming {vs:.3e}  gram-streaming {vgs:.3e}  bound {b:.1e}")
    with open(a.out, "a" if a.h256 else "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-len(worst) - 1:]))


if __name__ == "__main__":
    main()
