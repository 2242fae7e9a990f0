"""The (bag, model) job calls, bit for bit against the build of the commit before their host bookkeeping moved into
csrc/job_tables.hpp: tests/golden/job_calls_crc.json holds a CRC-32 per job and field of one Context.fixed_basis_jobs call (models of
H = 5, 16, 17, 32, so both tiers of the index table; a job with P in LDS and one with P in scratch) and one
Context.sparse_scored_jobs call (H = 5 and 17, the form and the trim varying per job, so all four groups), the jobs shuffled and
repeated.  tests/golden/make_job_calls_crc.py made it on that build and builds the inputs here.  A job table with one wrong offset, or
an idx that sends a job to another tier's kernel, changes some job's bits."""
import importlib.util
import json
import os

import pytest

import __graft_entry__ as G

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_job_calls_crc", os.path.join(G.ROOT, "tests", "golden", "make_job_calls_crc.py"))
GOLD = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(GOLD)


@pytest.fixture(scope="module")
def pkg():
    G.build()
    p = G.load_package()
    p.set_defaults(y_dtype=p.VBMF_Y_F32, factor_dtype=p.VBMF_FACTOR_AUTO)
    yield p
    p.invalidate()
    p.set_defaults(y_dtype=p.VBMF_Y_F32, factor_dtype=p.VBMF_FACTOR_AUTO)


@pytest.mark.parametrize("name", sorted(GOLD.CALLS))
def test_the_call_reproduces_the_parent_build(pkg, name):
    with open(GOLD.GOLDEN) as f:
        gold = json.load(f)["calls"][name]
    run, crcs, fields = GOLD.CALLS[name]
    r, jobs = run(pkg)
    assert gold["fields"] == list(fields) and gold["jobs"] == [list(map(float, q)) for q in jobs]      # the inputs are the recorded ones
    assert not r["status"].any()
    got = [crcs(r, j) for j in range(len(jobs))]
    wrong = [(j, jobs[j], f) for j in range(len(jobs)) for f, a, b in zip(fields, got[j], gold["crc"][j]) if a != b]
    assert not wrong, wrong
