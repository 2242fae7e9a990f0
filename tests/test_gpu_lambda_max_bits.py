"""The repeated squaring behind lambda_max at H <= 64 (eig_squaring_dev, csrc/ctrl_kernels.hpp), bit for bit: lambda of six structured
matrices at ten orders -- both sides of every tier edge (16 | 17, 32 | 33, 64) and orders whose rows are padded -- against the hex
doubles the build BEFORE the squaring took its wide form at 32 < H <= 64 (upper triangle of T T' only, 512 threads) returned for them
(tests/golden/lambda_max_bits.json, made once by scripts/lambda_max_bits.py through VBMF_HIP_LIB; never regenerated from the code
under test).  The matrices -- a well separated top eigenvalue (the loop leaves after two or three squarings), two equal top
eigenvalues (all ten), rank one, zero, one NaN entry on one side of the diagonal, eighteen decades on the diagonal plus a rank-one
term -- come from integers, so the inputs are the same bits everywhere.  One tiny context per order, shared by all of its cases."""
import importlib.util
import json
import math
import os

import pytest

import __graft_entry__ as G
from tests.helpers import report

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generator():
    spec = importlib.util.spec_from_file_location("lambda_max_bits", os.path.join(ROOT, "scripts", "lambda_max_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def gen():
    return _generator()


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "lambda_max_bits.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def measured(gen):
    G.build()
    return gen.lambda_hex(G.load_package())[0]


def test_fixture_covers_every_order_and_matrix(gen, golden):
    assert gen.ORDERS == [2, 15, 16, 17, 31, 32, 33, 48, 63, 64]
    names = list(gen.matrices(4))
    assert names == ["separated", "double_top", "rank_one", "zero", "one_nan", "spread"]
    assert sorted(golden) == sorted(gen.key(H, n) for H in gen.ORDERS for n in names)


@pytest.mark.parametrize("H", [2, 15, 16, 17, 31, 32, 33, 48, 63, 64])
def test_lambda_max_bits(gen, golden, measured, H):
    bad = []
    for name in gen.matrices(H):
        k = gen.key(H, name)
        report(f"lambda_max bits {k}: {measured[k]} (stored {golden[k]})")
        if measured[k] != golden[k]:
            bad.append((k, measured[k], golden[k]))
    assert not bad, bad


def test_fixture_values_are_what_the_cases_are_for(gen, golden):
    """The stored values themselves: the exact cases come out exact to the Rayleigh quotient's rounding (its error is quadratic in
    the fp32 vector's, ~1e-14), zero gives 0, and a NaN off the diagonal -- the trace stays finite, every squaring's Frobenius sum is
    NaN, the scale 0 -- ends in the quotient's den > 0 test: 0."""
    for H in gen.ORDERS:
        m = gen.matrices(H)
        w = m["rank_one"][0] / m["rank_one"][0, 0] * math.sqrt(m["rank_one"][0, 0])
        lam = float.fromhex(golden[gen.key(H, "rank_one")])
        assert abs(lam - float(w @ w)) <= 1e-12 * float(w @ w)
        assert float.fromhex(golden[gen.key(H, "zero")]) == 0.0
        assert float.fromhex(golden[gen.key(H, "one_nan")]) == 0.0
        top = (H // 2) * (H - H // 2) + 1.0
        assert abs(float.fromhex(golden[gen.key(H, "double_top")]) - top) <= 1e-12 * top
