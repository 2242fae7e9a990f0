"""gram_prod_kernel's workgroup geometry and LDS-DMA pipeline (csrc/gram_kernels.hpp): eight waves per workgroup (two per SIMD), each
wave's G fragments in a private LDS ring 4 k-steps deep, the W / D planes in double-buffered LDS chunks of 4 (NH = 2) or 2 k-steps.
Wave w of a row group of TPG = 16 / NH row tiles takes NXW = TPG / 8 tiles (NH = 1, 2); at NH = 4 waves w and w + 4 share tile
w % 4 and take two h tiles each.  VBMF_GRAM=1 forces the Gram form; run(1) is a streaming sweep that builds G and W, a second run(1)
one Gram-form sweep (scripts/gram_prod_pq_crc.py: run_pq).  Each shape asserts, from dims() and the split plan, the property it is
there for:

* one row group only (M <= 512), with and without row tiles past XT1 in it;
* a last row group in which every wave of the second half of the workgroup (waves 4-7) has only tiles past XT1;
* a last split shorter than the ring depth (2 and 3 k-steps; at NH = 2 shorter than the plane chunk as well), and k-steps per
  split that are no multiple of the chunk;
* NH = 1, 2 and 4; one split (no slab buffer).

On integer data G = Ys'Ys exactly, so P and Q are checked per entry against fp64 products of Ys'Ys with the W read back, by the
bounds of tests/test_gpu_gram_prod_pipeline.py (restated here).  Rows >= M of P and Q are zero, and a second context gives bitwise
the same [P | Q].

The bitwise lock: tests/golden/gram_prod_pq_crc.json holds the CRC-32 of [P | Q] for every shape here, written by
scripts/gram_prod_pq_crc.py on the build of the commit before the kernel took this geometry.  The split plan and the order of
additions are pinned, so the current build must reproduce them."""
import importlib.util
import json
import os

import numpy as np
import pytest

import __graft_entry__ as G
from tests.helpers import frag_to_rows, report

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gram_prod_pq_crc.json")

_spec = importlib.util.spec_from_file_location("gram_prod_pq_crc", os.path.join(ROOT, "scripts", "gram_prod_pq_crc.py"))
crc_script = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(crc_script)

NW, RING = 8, 4                      # GramProd<NH>::NW, ::D


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


def _plan(M, H):
    """the host's split plan (gram_prepare) and the kernel's geometry (GramProd<NH>)"""
    Hp = 32 if H <= 32 else (64 if H <= 64 else 128)
    NH = Hp // 32
    XT = -(-M // 32)
    GT = -(-XT // 16) * 16
    KT = 2 * GT
    TPG = 16 // NH
    nrg = GT // TPG
    ns = max(1, min(KT // 8, 256 // max(1, nrg)))
    sps = -(-KT // ns)
    ns = -(-KT // sps)
    return dict(NH=NH, XT=XT, GT=GT, TPG=TPG, nrg=nrg, ns=ns, sps=sps, last=KT - (ns - 1) * sps, NXW=max(1, TPG // NW),
                CH=4 if NH == 2 else 2)


def _wave_tiles(p, rg, w):
    """row tiles of wave w of row group rg"""
    per = p["TPG"] // p["NXW"]                                   # waves that cover the row group once
    return [rg * p["TPG"] + (w % per) * p["NXW"] + i for i in range(p["NXW"])]


def test_case_list_is_the_fixtures():
    assert sorted(crc_script.key(L, M, H) for L, M, H, _ in crc_script.CASES) == sorted(json.load(open(GOLDEN)))


@pytest.mark.parametrize("L,M,H,what", crc_script.CASES)
def test_gram_prod_overlap_geometry(pkg, L, M, H, what):
    p = _plan(M, H)
    NH, GT, ns, sps, last = p["NH"], p["GT"], p["ns"], p["sps"], p["last"]
    assert f"NH {NH}" in what
    if "one row group" in what:
        assert M <= 512 and p["nrg"] == 1, (what, p)
    if "last split" in what:
        assert last == int(what.split("last split ")[1][0]) and last < RING and (NH != 2 or last < p["CH"]), (what, p)
    if "sps odd" in what:
        assert sps % p["CH"] != 0, (what, p)
    if "one split" in what:
        assert ns == 1
    Y = crc_script.seeded_Y(L, M, H)
    r = crc_script.run_pq(pkg, Y, H, 7200 + M)
    assert r["NH"] == NH and r["GT"] == GT and r["nsplit"] == ns, (what, r["NH"], r["nsplit"])
    assert p["XT"] <= r["XT"] <= GT                              # dims()' XT1: the x tiles of pass 1, padded to its wave tile count
    if "second half past XT1" in what:
        tiles = [t for w in range(NW // 2, NW) for t in _wave_tiles(p, p["nrg"] - 1, w)]
        assert tiles and all(t >= r["XT"] for t in tiles), (what, p, tiles)
    Ys = r["Ys"]
    assert np.array_equal(Ys, Y)                                  # integers are exact in bf16, so G = Ys'Ys exactly
    n, Mp1, Hp = r["n"], 32 * r["XT"], r["Hp"]
    P = frag_to_rows(r["PQ"][:n], Mp1, Hp)
    Q = frag_to_rows(r["PQ"][n:], Mp1, Hp)
    assert not np.any(P[M:]) and not np.any(Q[M:]), what
    # rows checked: all of them on the small shapes, a spread subset (first, last, split edges) on the one-split shape
    if M <= 5000:
        rows = np.arange(M)
    else:
        edges = (np.arange(0, M, 16 * sps)[1:, None] + np.arange(-8, 8)).ravel()
        rows = np.unique(np.concatenate([np.arange(64), np.arange(M - 64, M), edges, np.arange(0, M, 997)]))
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
    crc = crc_script.pq_crc(r["PQ"])
    report(f"gram_prod overlap {what} ({L}x{M} H{H}): nsplit {ns}, sps {sps}, last {last}, crc {crc}: P_entry={worstP:.2e} "
           f"Q_entry={worstQ:.2e}")
    assert np.all(eP <= kP * aGW), (what, worstP, kP)
    assert np.all(eQ <= kQ * aGD), (what, worstQ, kQ)
    # bitwise what the kernel before this geometry gave
    assert crc == json.load(open(GOLDEN))[crc_script.key(L, M, H)], (what, crc)
    # the same inputs through a second context: bitwise the same product
    r2 = crc_script.run_pq(pkg, Y, H, 7200 + M)
    assert np.array_equal(r2["PQ"].view(np.uint32), r["PQ"].view(np.uint32)), what
