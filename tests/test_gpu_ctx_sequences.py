"""Call sequences on one context, bit for bit against the build that kept the validity of its derived data in loose flags
(tests/golden/ctx_sequences_crc.json, made by scripts/ctx_sequences_crc.py on the commit named in the file).  Every sequence crosses a
point where the host reuses or drops a cached quantity -- the Grams, Y'B, Y A, tr(B'YA), G = Y'Y, W, the owed B -- so a cache kept too
long or dropped too early (csrc/ctx_cache.hpp) changes a CRC somewhere down the sequence.  Two recordings per sequence: the state read
after every call, and only once at the end (a read of B pays the pass a Gram-form run owes)."""
import importlib.util
import json
import os

import pytest

import __graft_entry__ as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("ctx_sequences_crc", os.path.join(ROOT, "scripts", "ctx_sequences_crc.py"))
S = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(S)


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


@pytest.fixture(scope="module")
def golden():
    with open(S.GOLDEN) as f:
        return json.load(f)


def test_the_fixture_covers_the_sequences(golden):
    assert len(golden["made_by_commit"]) == 40
    assert len(golden["unrepeatable"]) <= 2, sorted(golden["unrepeatable"])
    assert set(golden["cases"]) | set(golden["unrepeatable"]) == set(S.CASES)
    assert not set(golden["cases"]) & set(golden["unrepeatable"])


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_sequence_reproduces_the_recorded_bits(pkg, golden, name):
    if name in golden["unrepeatable"]:
        pytest.skip("not repeatable on the build that made the fixture: " + golden["unrepeatable"][name][:120])
    got, want = S.run_case(pkg, name), golden["cases"][name]
    for record in ("each", "end"):
        calls = [" ".join(str(x) for x in op) for op in S.CASES[name][5]] + ["final state"]
        diff = [(i, calls[i]) for i, (a, b) in enumerate(zip(got[record], want[record])) if a != b]
        assert len(got[record]) == len(want[record]) and not diff, (name, record, "first difference after call", diff[:1])
