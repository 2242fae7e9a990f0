"""csrc/ctx_cache.hpp on the host: tests/ctx_cache_check.cpp (its own main, nothing but that header) built with the host C++
compiler under the address and undefined-behaviour sanitizers and run.  It holds every event of the record to the complete flag
vector the assignments at that site produced before the record existed, from all flags set and from all clear, and walks the
chains DESIGN.md section 10 promises.  Nothing is loaded into Python."""
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


def test_every_event_and_the_promised_chains(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "ctx_cache_check")
    b = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(HERE, "ctx_cache_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "events from both ends and the chains hold" in r.stdout, r.stdout


def test_a_write_from_outside_does_not_compile(tmp_path):
    """the flags are private: the compiler refuses a call site that flips one itself"""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "poke.cpp"
    src.write_text('#include "%s"\nint main() { vbmf::CtxCache c; c.W_ = true; return c.W(); }\n'
                   % os.path.join(HERE, "..", "vbmatrixfactorization.jl_amd", "csrc", "ctx_cache.hpp"))
    b = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert b.returncode != 0 and "private" in b.stderr, b.stderr
