"""csrc/job_tables.hpp on the host: tests/job_tables_check.cpp (its own main, nothing but that header) built with the host C++ compiler
under the address and undefined-behaviour sanitizers and run.  The walk's five sums, every shared refusal with its text and its
precedence, the int64 job table against a second, naive construction (mixed groups, one model, one job, every job in the first group,
every job in the last), idx as a grouped permutation in job order with grp_at its groups' first slots, and the model and entry a
planted NaN or Inf is reported at for each stride.  Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _compiler():
    for cand in (os.environ.get("CXX"), "g++", "clang++", "c++"):
        if cand and shutil.which(cand):
            return shutil.which(cand)
    return None


def test_the_job_bookkeeping_under_sanitizers(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "job_tables_check")
    b = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(HERE, "job_tables_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "the sums, the table, the refusals and the non-finite search hold" in r.stdout, r.stdout
