"""csrc/ctx_mem.hpp on the host: tests/ctx_mem_check.cpp (its own main, nothing but that header) built with the host C++ compiler
under the address and undefined-behaviour sanitizers and run.  Its allocator is a counting malloc / free that fails on request:
release_all frees every recorded buffer once and nulls its slot, a taken slot is refused, a group of eight rolls back to what was
owned before it whichever allocation fails, the one buffer that grows is regrown as bags_reserve does it, and the scratch guard
frees on every way out of a function.  Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "vbmatrixfactorization.jl_amd", "csrc", "ctx_mem.hpp")


def _compiler():
    for cand in (os.environ.get("CXX"), "g++", "clang++", "c++"):
        if cand and shutil.which(cand):
            return shutil.which(cand)
    return None


def test_owner_and_scratch_under_a_failing_allocator(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "ctx_mem_check")
    b = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(HERE, "ctx_mem_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "release, refusal, rollback at every k, regrow and the scratch guard hold" in r.stdout, r.stdout


POLICY = "struct A { static int alloc(void** p, size_t) { *p = nullptr; return 0; } static void free(void*) {} };\n"


def test_copying_a_scratch_guard_does_not_compile(tmp_path):
    """two guards of one buffer would free it twice: the compiler refuses the copy (and takes the same program without it)"""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    for copy, ok in (("", True), ("vbmf::Scratch<A, double> t = s; (void)t;", False)):
        src = tmp_path / ("copy.cpp" if copy else "nocopy.cpp")
        src.write_text('#include "%s"\n%sint main() { vbmf::Scratch<A, double> s; %s return s.alloc(8); }\n' % (HEADER, POLICY, copy))
        b = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", str(src)], capture_output=True, text=True)
        assert (b.returncode == 0) == ok, b.stderr
        assert ok or "deleted" in b.stderr, b.stderr
