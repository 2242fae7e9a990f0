"""The tail of the Gram-form product (csrc/gram_kernels.hpp): gram_tail_kernel folds the split-K slabs of [P | Q] and forms the
per-chunk fp64 shares from the folded values in one launch, gram_part_reduce_kernel sums the shares with all of a thread's loads in
one round.  VBMF_GRAM=1 forces the Gram form; run(1) is a streaming sweep that builds G and W, a second run(1) one Gram-form sweep
(scripts/gram_tail_state_crc.py: run_tail).  Each shape asserts, from the host's chunk plan (gram_prepare) and dims(), the
property it is there for:

* Hp = 32, 64, 128 (V = 2, 4, 8 column offsets; S = 4, 2, 1 row subsets: S = 1 has no subset fold);
* one chunk (the reduce with three of its four chunk groups empty), M = 1 mod 4;
* a ragged last chunk of 33 rows that ends in a partial 4-row step;
* 37 chunks = 4 * 9 + 1: reduce groups of 10, 9, 9, 9 chunks;
* rows of [P | Q] past the last 4-row step that belong to no chunk (32 XT1 > 4 ceil(M / 4)) exist.  They are zero in every slab
  and in the zero-filled [P | Q], so neither the zero check nor the CRC can tell whether the fold wrote them: that the last chunk's
  workgroups fold up to 32 XT1 is a property of the code (fend in gram_tail_kernel), not one this test establishes.

The bitwise lock: tests/golden/gram_tail_state_crc.json holds, per shape, the CRC-32 of all 2 n floats of [P | Q] and of the state's
2 Hp^2 + 1 doubles [B'B | dB'dB | tr(B'YA)], written by scripts/gram_tail_state_crc.py on the build of the commit before the fold
moved into the partials kernel (the file names it).  No sum changed its order, so the current build must reproduce them.

Beside it: the slots are within 1e-12 of an fp64 recomputation from the W, [P | Q] and A read back (the bound of
tests/test_gpu_gram_partials.py, restated here: fp64 sums of exact fp32 products, so only the summation order differs), rows >= M
of P and Q are exactly zero, and a second context gives bitwise the same [P | Q] and slots."""
import importlib.util
import json
import os

import numpy as np
import pytest

import __graft_entry__ as G
from tests.helpers import frag_to_rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gram_tail_state_crc.json")

_spec = importlib.util.spec_from_file_location("gram_tail_state_crc", os.path.join(ROOT, "scripts", "gram_tail_state_crc.py"))
crc_script = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(crc_script)

GRED_G = 4                            # chunk groups of gram_part_reduce_kernel


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def test_case_list_is_the_fixtures():
    g = json.load(open(GOLDEN))
    assert sorted(crc_script.key(M, H) for M, H, _ in crc_script.CASES) == sorted(g["cases"])
    assert len(g["made_by_commit"]) >= 7


@pytest.mark.parametrize("M,H,what", crc_script.CASES)
def test_gram_tail(pkg, M, H, what):
    p = crc_script.chunk_plan(M, H)
    Hp, nchunk, rpc = p["Hp"], p["nchunk"], p["rpc"]
    assert f"Hp {Hp}" in what and (p["V"], p["S"]) == {32: (2, 4), 64: (4, 2), 128: (8, 1)}[Hp]
    groups = [len(range(g, nchunk, GRED_G)) for g in range(GRED_G)]
    if "one chunk" in what:
        assert nchunk == 1 and groups == [1, 0, 0, 0] and M % 4 == 1, (what, p)
    if "6 chunks" in what:
        assert nchunk == 6 and rpc == 64 and p["last"] == 33 and p["last"] % 4 != 0, (what, p)
    if "37 chunks" in what:
        assert nchunk == 37 and groups == [10, 9, 9, 9], (what, p)         # one full round of eight plus tails of unequal length
    Y = crc_script.seeded_Y(M, H)
    r = crc_script.run_tail(pkg, Y, H, 8200 + M)
    assert r["Hp"] == Hp
    n, Mp1 = r["n"], 32 * r["XT"]
    if "padding rows" in what:
        assert Mp1 > 4 * -(-M // 4), (what, Mp1)                            # padding rows that no chunk's steps reach exist
    P = frag_to_rows(r["PQ"][:n], Mp1, Hp)
    Q = frag_to_rows(r["PQ"][n:], Mp1, Hp)
    assert not np.any(P[M:]) and not np.any(Q[M:]), what
    # the slots against fp64 sums of the read-back factors
    n2 = Hp * Hp
    GB, GD, GX = r["slots"][:n2].reshape(Hp, Hp), r["slots"][n2:2 * n2].reshape(Hp, Hp), r["slots"][2 * n2]
    W = r["W1"][:M].astype(np.float64)
    D = (W - r["W0"][:M].astype(np.float64)).astype(np.float32).astype(np.float64)
    A = r["A"].astype(np.float64)
    WP, DQ = W.T @ P[:M], D.T @ Q[:M]
    tr = np.sum(A * P[:M])
    eB, eD = _rel(GB, 0.5 * (WP + WP.T)), _rel(GD, 0.5 * (DQ + DQ.T))
    eX = abs(GX - tr) / np.sum(np.abs(A * P[:M]))
    got = dict(pq=crc_script.crc(r["PQ"]), state=crc_script.crc(r["slots"]))
    print(f"gram_tail {what} ({crc_script.key(M, H)}): nsplit {r['nsplit']}, nchunk {nchunk}, rpc {rpc}, crc {got}: "
          f"GB={eB:.2e} GD={eD:.2e} GX={eX:.2e}")
    assert eB < 1e-12 and eD < 1e-12 and eX <= 1e-12, (what, eB, eD, eX)
    assert np.array_equal(GB, GB.T) and np.array_equal(GD, GD.T)
    # bitwise what the separate slab sum and partials kernel gave
    assert got == json.load(open(GOLDEN))["cases"][crc_script.key(M, H)], (what, got)
    # the same inputs through a second context: bitwise the same
    r2 = crc_script.run_tail(pkg, Y, H, 8200 + M)
    assert np.array_equal(r2["PQ"].view(np.uint32), r["PQ"].view(np.uint32)), what
    assert np.array_equal(r2["slots"].view(np.uint64), r["slots"].view(np.uint64)), what
