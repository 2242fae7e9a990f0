"""vbls! of the sparse models over many bags (vbmf_sparse_run_fixed_basis_batched / vbls_sparse_batch_): the parts that need no
GPU -- the C ABI is declared and exported, the Julia host binds it, and the Python host refuses what the batched path does not
cover BEFORE any device call."""
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
    assert re.search(r"int\s+vbmf_sparse_run_fixed_basis_batched\s*\(\s*vbmf_ctx\*\s*ctx\s*,\s*int64_t\s+nbags\s*,\s*const\s+int64_t\*\s*"
                     r"col_off\s*,\s*int64_t\s+niter\s*,\s*int\s+full_cov", hdr)
    assert "examples/mil_util.jl:187-197" in hdr
    assert hasattr(ctypes.CDLL(pkg.capi.LIB_PATH), "vbmf_sparse_run_fixed_basis_batched")
    assert "vbmf_sparse_run_fixed_basis_batched" in pkg.capi.SYMBOLS
    assert len(pkg.capi.lib().vbmf_sparse_run_fixed_basis_batched.argtypes) == 16
    assert hasattr(pkg.capi.Context, "sparse_run_fixed_basis_batched")


def test_julia_host_binds_it():
    jl = open(os.path.join(G.PKG_DIR, "julia", "VBMatrixFactorizationHIP.jl")).read()
    assert re.search(r"ccall\(\(:vbmf_sparse_run_fixed_basis_batched,\s*libvbmf\)", jl)
    for T in ("vbmf_sparse_parameters", "vbmf_dual_parameters"):
        assert re.search(r"function vbls_batch!\(Ys::Vector\{Matrix\{Float64\}\},\s*ps::Vector\{" + T + r"\},\s*niter::Int;\s*"
                         r"full_cov::Bool\s*=\s*false\)", jl), T
    assert re.search(r"export[^\n]*\n?[^\n]*vbls_batch!", jl)


@pytest.fixture
def no_device(pkg, monkeypatch):
    """Any attempt to reach the library fails the test (the refusals happen on the host)."""
    def boom(*a, **k):
        raise AssertionError("vbls_sparse_batch_ touched the device before refusing")
    monkeypatch.setattr(pkg.capi, "lib", boom)
    monkeypatch.setattr(pkg.capi.Context, "__init__", boom)
    monkeypatch.setattr(pkg.Session, "__init__", boom)
    return pkg


def _trained(pkg, kind, L, H, rng):
    Ytr = rng.standard_normal((L, 20))
    if kind == "sparse":
        return pkg.vbmf_sparse_init(Ytr, H, rng=rng)
    if kind == "dual":
        return pkg.vbmf_dual_init(Ytr, H, max(1, H // 2), rng=rng)
    return pkg.vbmf_trial_init(Ytr, H, max(1, H // 2), 12, rng=rng)


def _bags(pkg, kind="sparse", L=30, Ms=(3, 1, 7), H=4, seed=0):
    rng = np.random.default_rng(seed)
    Ys = [rng.standard_normal((L, m)) for m in Ms]
    res = _trained(pkg, kind, L, H, rng)
    ps = []
    for Y in Ys:
        q = pkg.copy_vbmf_params(Y, res, rng=np.random.default_rng(1))
        ps.append(q[0] if isinstance(q, tuple) else q)
    return Ys, ps, res


def _refused(pkg, Ys, ps, match="vbls_", **kw):
    with pytest.raises(ValueError, match=match):
        pkg.vbls_sparse_batch_(Ys, ps, 10, **kw)


@pytest.mark.parametrize("kind", ["sparse", "dual", "trial"])
def test_refuses_mismatched_L(no_device, kind):
    pkg = no_device
    Ys, ps, res = _bags(pkg, kind)
    Ys[1] = np.zeros((31, 1))
    _refused(pkg, Ys, ps)
    with pytest.raises(ValueError, match="vbls_"):
        pkg.SparseBags(Ys, 4)


@pytest.mark.parametrize("kind", ["sparse", "dual", "trial"])
def test_refuses_params_of_another_shape(no_device, kind):
    pkg = no_device
    Ys, ps, _ = _bags(pkg, kind)
    ps[0], ps[2] = ps[2], ps[0]
    _refused(pkg, Ys, ps)
    Ys, ps, _ = _bags(pkg, kind)
    _refused(pkg, Ys, ps[:2])
    Ys, ps, _ = _bags(pkg, kind)
    ps[1].CA = np.ones(5)
    _refused(pkg, Ys, ps)


def test_refuses_mixed_types(no_device):
    pkg = no_device
    Ys, ps, _ = _bags(pkg, "sparse")
    _, pd, _ = _bags(pkg, "dual")
    ps[1] = pd[1]
    _refused(pkg, Ys, ps, match="one model type")
    Ys, pb, _ = _bags(pkg, "sparse")
    rng = np.random.default_rng(2)
    res = pkg.vbmf_init(rng.standard_normal((30, 20)), 4, rng=rng)
    basic = [pkg.copy_vbmf_params(Y, res) for Y in Ys]
    _refused(pkg, Ys, basic)


@pytest.mark.parametrize("kind", ["sparse", "dual", "trial"])
def test_refuses_differing_bases(no_device, kind):
    pkg = no_device
    for f in ("BHat", "SigmaB"):
        Ys, ps, _ = _bags(pkg, kind)
        setattr(ps[2], f, getattr(ps[2], f).copy())
        getattr(ps[2], f)[0, 0] += 1e-3
        _refused(pkg, Ys, ps, match="BHat and SigmaB")


def test_refuses_labels(no_device):
    pkg = no_device
    Ys, ps, _ = _bags(pkg)
    ps[0].labels = np.array([1], dtype=np.int64)
    ps[0].H1 = 1
    _refused(pkg, Ys, ps, match="label")
    Ys, ps, _ = _bags(pkg)
    ps[1].H1 = 2
    _refused(pkg, Ys, ps, match="label")


def test_refuses_trial_with_a_third_group(no_device):
    pkg = no_device
    Ys, ps, res = _bags(pkg, "trial")
    ps[2] = pkg.vbmf_trial_init(Ys[2], 4, 2, 3, rng=np.random.default_rng(4))
    ps[2].BHat, ps[2].SigmaB = ps[0].BHat, ps[0].SigmaB
    _refused(pkg, Ys, ps, match="M0")


@pytest.mark.parametrize("kind", ["sparse", "dual", "trial"])
def test_refuses_rank_above_64(no_device, kind):
    pkg = no_device
    Ys, ps, _ = _bags(pkg, kind, H=65)
    _refused(pkg, Ys, ps, match="64")
    with pytest.raises(ValueError, match="vbls_"):
        pkg.SparseBags(Ys, 65)


@pytest.mark.parametrize("kind", ["sparse", "dual", "trial"])
def test_refuses_non_derived_constants(no_device, kind):
    pkg = no_device
    Ys, ps, _ = _bags(pkg, kind)
    ps[1].eta = ps[1].eta + 3.0
    _refused(pkg, Ys, ps, match="eta")
    Ys, ps, _ = _bags(pkg, kind)
    ps[2].gamma = ps[2].gamma * 2.0
    _refused(pkg, Ys, ps, match="gamma")
    if kind == "sparse":
        Ys, ps, _ = _bags(pkg, kind)
        ps[0].alpha = ps[0].alpha0 + 0.75
        _refused(pkg, Ys, ps, match="alpha")


def test_refuses_empty_and_columnless(no_device):
    pkg = no_device
    Ys, ps, _ = _bags(pkg)
    Ys[1] = np.zeros((30, 0))
    _refused(pkg, Ys, ps)
    _refused(pkg, [], [])
