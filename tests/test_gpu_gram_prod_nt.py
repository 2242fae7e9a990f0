"""gram_prod_kernel's cache policy for G (csrc/gram_kernels.hpp): a Gram of more than GRAM_G_NT_BYTES is streamed by non-temporal
LDS-DMA pieces, a smaller one on the default policy.  The policy moves no byte and no addition, so [P | Q] must be what the kernel
gave before it had the choice.  The shapes sit on both sides of the threshold: GT = 256 row tiles (256 MiB, the first Gram above
it) at NH = 2 and NH = 1, and GT = 240 (225 MiB, the last below it); at NH = 4 the one-split shape of
tests/test_gpu_gram_prod_overlap.py (GT = 528) already runs non-temporal.  VBMF_GRAM=1 forces the Gram form; run(1) is a streaming
sweep that builds G and W, a second run(1) one Gram-form sweep.

On integer data G = Ys'Ys exactly, so P and Q are checked per entry, on a spread subset of rows, against fp64 products of Ys'Ys
with the W read back, by the bounds of tests/test_gpu_gram_prod_pipeline.py (restated here).  Rows >= M of P and Q are zero, and a
second context gives bitwise the same [P | Q].

The bitwise lock: tests/golden/gram_prod_nt_crc.json holds the CRC-32 of [P | Q] for every shape here, written by
scripts/gram_prod_nt_crc.py on the build of the commit before the policy."""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

import __graft_entry__ as G
from tests.helpers import frag_to_rows, report

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gram_prod_nt_crc.json")
NT_BYTES = 240 << 20                 # GRAM_G_NT_BYTES


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod                                       # the generator imports gram_prod_pq_crc by name
    spec.loader.exec_module(mod)
    return mod


pq_script = _load("gram_prod_pq_crc")
crc_script = _load("gram_prod_nt_crc")


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


def _plan(M, H):
    """the host's split plan (gram_prepare)"""
    Hp = 32 if H <= 32 else (64 if H <= 64 else 128)
    NH = Hp // 32
    XT = -(-M // 32)
    GT = -(-XT // 16) * 16
    KT = 2 * GT
    nrg = GT // (16 // NH)
    ns = max(1, min(KT // 8, 254 // max(1, nrg)))            # NUM_CU of the host
    sps = -(-KT // ns)
    ns = -(-KT // sps)
    return dict(NH=NH, XT=XT, GT=GT, ns=ns, sps=sps)


def test_case_list_is_the_fixtures():
    assert sorted(pq_script.key(L, M, H) for L, M, H, _ in crc_script.CASES) == sorted(json.load(open(GOLDEN)))


@pytest.mark.parametrize("L,M,H,what", crc_script.CASES)
def test_gram_prod_cache_policy(pkg, L, M, H, what):
    p = _plan(M, H)
    NH, GT, ns, sps = p["NH"], p["GT"], p["ns"], p["sps"]
    assert f"NH {NH}" in what and f"GT {GT}" in what
    g_bytes = (32 * GT) ** 2 * 4
    assert (g_bytes > NT_BYTES) == ("non-temporal" in what), (what, g_bytes)
    # the two sides are neighbours: one step of GT (16 row tiles) apart at most
    assert abs(g_bytes - NT_BYTES) <= (32 * 256) ** 2 * 4 - (32 * 240) ** 2 * 4, (what, g_bytes)
    Y = pq_script.seeded_Y(L, M, H)
    r = pq_script.run_pq(pkg, Y, H, 7200 + M)
    assert r["NH"] == NH and r["GT"] == GT and r["nsplit"] == ns, (what, r["NH"], r["nsplit"])
    Ys = r["Ys"]
    assert np.array_equal(Ys, Y)                                  # integers are exact in bf16, so G = Ys'Ys exactly
    n, Mp1, Hp = r["n"], 32 * r["XT"], r["Hp"]
    P = frag_to_rows(r["PQ"][:n], Mp1, Hp)
    Q = frag_to_rows(r["PQ"][n:], Mp1, Hp)
    assert not np.any(P[M:]) and not np.any(Q[M:]), what
    # rows checked: first, last, the split edges and a stride through the rest
    edges = (np.arange(0, M, 16 * sps)[1:, None] + np.arange(-8, 8)).ravel()
    rows = np.unique(np.concatenate([np.arange(64), np.arange(M - 64, M), edges, np.arange(0, M, 61)]))
    rows = rows[(rows >= 0) & (rows < M)]
    Wr = r["W1"][:32 * GT]
    D = (r["W1"] - r["W0"]).astype(np.float32).astype(np.float64)[:32 * GT]
    Gr = np.zeros((len(rows), 32 * GT))
    Gr[:, :M] = Ys[:, rows].T @ Ys                                # integer sums below 2^53: exact in fp64
    assert np.abs(Gr).max() < 2 ** 24
    # the bounds of test_gpu_gram_prod_pipeline: |P - GW| <= (6 sps + nsplit + 4) u (|G||W|),
    # |Q - GD| <= (2^-16 + (3 sps + nsplit + 4) u) (|G||D|)
    kP = (6 * sps + ns + 4) * U
    kQ = 2.0 ** -16 + (3 * sps + ns + 4) * U
    GW, GD = Gr @ Wr, Gr @ D
    aGW, aGD = np.abs(Gr) @ np.abs(Wr), np.abs(Gr) @ np.abs(D)
    eP, eQ = np.abs(P[rows] - GW), np.abs(Q[rows] - GD)
    worstP = float(np.max(eP / np.maximum(aGW, 1e-300)))
    worstQ = float(np.max(eQ / np.maximum(aGD, 1e-300)))
    crc = pq_script.pq_crc(r["PQ"])
    report(f"gram_prod cache policy {what} ({L}x{M} H{H}): nsplit {ns}, sps {sps}, G {g_bytes >> 20} MiB, crc {crc}: "
           f"P_entry={worstP:.2e} Q_entry={worstQ:.2e}")
    assert np.all(eP <= kP * aGW), (what, worstP, kP)
    assert np.all(eQ <= kQ * aGD), (what, worstQ, kQ)
    # bitwise what the kernel gave before it chose a policy
    assert crc == json.load(open(GOLDEN))[pq_script.key(L, M, H)], (what, crc)
    # the same inputs through a second context: bitwise the same product
    r2 = pq_script.run_pq(pkg, Y, H, 7200 + M)
    assert np.array_equal(r2["PQ"].view(np.uint32), r["PQ"].view(np.uint32)), what
