"""vbls! over many bags (vbmf_run_fixed_basis_batched / vbls_batch_): the parts that need no GPU -- the C ABI is declared and
exported, the Julia host binds it, and the Python host refuses what the batched path does not cover BEFORE any device call."""
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as G

ROOT = G.ROOT


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


def test_header_declares_and_library_exports(pkg):
    hdr = open(os.path.join(ROOT, "include", "vbmf_hip.h")).read()
    assert re.search(r"int\s+vbmf_run_fixed_basis_batched\s*\(\s*vbmf_ctx\*\s*ctx\s*,\s*int64_t\s+nbags\s*,\s*const\s+int64_t\*\s*col_off",
                     hdr)
    assert hasattr(ctypes.CDLL(pkg.capi.LIB_PATH), "vbmf_run_fixed_basis_batched")
    assert "vbmf_run_fixed_basis_batched" in pkg.capi.SYMBOLS


def test_julia_host_binds_it():
    jl = open(os.path.join(G.PKG_DIR, "julia", "VBMatrixFactorizationHIP.jl")).read()
    assert re.search(r"ccall\(\(:vbmf_run_fixed_basis_batched,\s*libvbmf\)", jl)
    assert re.search(r"function vbls_batch!\(Ys::Vector\{Matrix\{Float64\}\},\s*ps::Vector\{vbmf_parameters\},\s*niter::Int\)", jl)
    assert re.search(r"export[^\n]*\n?[^\n]*vbls_batch!", jl)


@pytest.fixture
def no_device(pkg, monkeypatch):
    """Any attempt to reach the library fails the test (the refusals happen on the host)."""
    def boom(*a, **k):
        raise AssertionError("vbls_batch_ touched the device before refusing")
    monkeypatch.setattr(pkg.capi, "lib", boom)
    monkeypatch.setattr(pkg.capi.Context, "__init__", boom)
    monkeypatch.setattr(pkg.Session, "__init__", boom)
    return pkg


def _bags(pkg, L=30, Ms=(3, 1, 7), H=4, seed=0):
    rng = np.random.default_rng(seed)
    Ys = [rng.standard_normal((L, m)) for m in Ms]
    res = pkg.vbmf_init(rng.standard_normal((L, 20)), H, rng=rng)
    ps = [pkg.copy_vbmf_params(Y, res, rng=np.random.default_rng(1)) for Y in Ys]
    return Ys, ps, res


def test_refuses_mismatched_L(no_device):
    pkg = no_device
    Ys, ps, res = _bags(pkg)
    Ys[1] = np.zeros((31, 1))
    ps[1] = pkg.copy_vbmf_params(Ys[1], res)
    with pytest.raises(ValueError, match="vbls_"):
        pkg.vbls_batch_(Ys, ps, 10)
    with pytest.raises(ValueError, match="vbls_"):
        pkg.Bags(Ys, 4)


def test_refuses_params_of_another_shape(no_device):
    pkg = no_device
    Ys, ps, _ = _bags(pkg)
    ps[0], ps[2] = ps[2], ps[0]
    with pytest.raises(ValueError, match="vbls_"):
        pkg.vbls_batch_(Ys, ps, 10)
    with pytest.raises(ValueError, match="vbls_"):
        pkg.vbls_batch_(Ys, ps[:2], 10)


def test_refuses_differing_bases(no_device):
    pkg = no_device
    for f in ("BHat", "SigmaB", "CB"):
        Ys, ps, _ = _bags(pkg)
        getattr(ps[2], f)[0, 0] += 1e-3
        with pytest.raises(ValueError, match="vbls_"):
            pkg.vbls_batch_(Ys, ps, 10)


def test_refuses_labels(no_device):
    pkg = no_device
    Ys, ps, _ = _bags(pkg)
    ps[0].labels = np.array([1], dtype=np.int64)
    ps[0].H1 = 1
    with pytest.raises(ValueError, match="vbls_"):
        pkg.vbls_batch_(Ys, ps, 10)
    Ys, ps, _ = _bags(pkg)
    ps[1].H1 = 2
    with pytest.raises(ValueError, match="vbls_"):
        pkg.vbls_batch_(Ys, ps, 10)


def test_refuses_rank_above_64(no_device):
    pkg = no_device
    Ys, ps, _ = _bags(pkg, H=65)
    with pytest.raises(ValueError, match="vbls_"):
        pkg.vbls_batch_(Ys, ps, 10)
    with pytest.raises(ValueError, match="vbls_"):
        pkg.Bags(Ys, 65)


def test_refuses_other_models(no_device):
    pkg = no_device
    rng = np.random.default_rng(3)
    Ys = [rng.standard_normal((20, 4)) for _ in range(2)]
    ps = [pkg.vbmf_sparse_init(Y, 3, rng=rng) for Y in Ys]
    with pytest.raises(ValueError, match="vbls_"):
        pkg.vbls_batch_(Ys, ps, 10)
