"""The seams of the Gram-form sweep's H x H control chain (csrc/ctrl_kernels.hpp: ctrl_chain): what crosses a run
boundary or an eps stop.  lambda_max(B_old'B_old) is computed one launch ahead into a shadow slot and committed to S_LAMB_PREV
beside the SigmaA shadow, ctrl_end hands its operands on to the SigmaA update, and the commit feeds SigmaB's matrix from registers.
None of this may move a bit of any fp64 result: the first d after a run boundary and after a stop (where the commit of lambda_max
can go wrong) and every SigmaA / SigmaB / CA / CB / scalar at all four tiers of the inverse (R = 1, 2, 4, 8; lambda_max by repeated
squaring up to H = 64, by Lanczos above) are pinned.

The bitwise lock: tests/golden/gram_seams_trace_crc.json holds, per rank, CRC-32s of the traces and final states of

  a  run(6)                        b  run(3), run(3)
  c  run(6, eps) stopping early, then run(2)          k  run(k), k the stopping sweep of c

(after one streaming sweep each; scripts/gram_seams_trace_crc.py: case), written by that script on the build of the commit before the
chain's seams were reworked (the file names it) together with the identities that held there: b == a, c's stop trace is a prefix of
a's, c's stop state is run(k)'s.  The current build must reproduce every CRC and every listed identity; eps is the fixture's.
Beside it: variant a through a second context is bitwise the same, the context takes the Gram form, and the chain's four stamps
(ctrl_end, SigmaA, lambda_max(dB'dB) + loop test, SigmaB) are positive after a Gram-form run."""
import importlib.util
import json
import os

import numpy as np
import pytest

import __graft_entry__ as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gram_seams_trace_crc.json")

_spec = importlib.util.spec_from_file_location("gram_seams_trace_crc", os.path.join(ROOT, "scripts", "gram_seams_trace_crc.py"))
crc_script = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(crc_script)


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_case_list_is_the_fixtures(golden):
    assert sorted(crc_script.key(H) for H, _, _ in crc_script.CASES) == sorted(golden["cases"])
    assert len(golden["made_by_commit"]) >= 7
    assert set(golden["identities"]) <= set(crc_script.IDENTITIES)
    assert [R for _, R, _ in crc_script.CASES] == [1, 2, 4, 8]


@pytest.mark.parametrize("H,R,method", crc_script.CASES)
def test_gram_seams(pkg, golden, H, R, method):
    want = golden["cases"][crc_script.key(H)]
    eps = float.fromhex(want["c"]["eps"])
    arr, got, held = crc_script.case(pkg, H, eps=eps)
    d = arr["a"][1][:, 0]
    print(f"gram_seams {crc_script.key(H)} (R {R}, {method}): d {d}, eps {eps:.6e}, stop at {got['c']['stop_sweep']}, "
          f"identities {held}, chain_us {arr['chain']}")
    print("got ", json.dumps(got, sort_keys=True))
    print("want", json.dumps(want, sort_keys=True))
    assert arr["dims"]["gram"] == 1 and arr["dims"]["gram_built"] == 1, arr["dims"]
    assert arr["a"][0] == crc_script.NSWEEP and arr["b"][0][0] == arr["b"][1][0] == 3
    # the eps stop lands on the fixture's sweep, strictly inside the run, and the run after it does its two sweeps
    assert got["c"]["stop_sweep"] == want["c"]["stop_sweep"] and 1 <= want["c"]["stop_sweep"] < crc_script.NSWEEP
    assert arr["c"][1][0] == 2
    for v in ("a", "b", "c", "k"):
        assert got[v] == want[v], (H, v, got[v], want[v])
    for name in golden["identities"]:
        assert held[name], (H, name)
    # the four stamps of the chain's parts after a Gram-form run
    for part in ("ctrl_end", "SigmaA", "lambda_max_dB_and_loop", "SigmaB"):
        assert arr["chain"][part] > 0.0, (part, arr["chain"])
    # variant a through a second context: bitwise the same
    (a2,), _, _ = crc_script.runs(pkg, H, [(crc_script.NSWEEP, 0.0)])
    assert a2[0] == arr["a"][0] and crc_script.same_trace(a2[1], arr["a"][1]) and crc_script.same_state(a2[2], arr["a"][2]), H
