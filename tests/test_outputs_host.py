"""Results into the caller's memory (vbmf_get_YHat_rows / vbmf_get_factor_rows): the parts that need no GPU --
the C ABI is declared, exported and bound in both hosts, capi.y_sink describes a destination where it lies and refuses what cannot
be written BEFORE the library is touched, and the host shells route their new arguments."""
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


@pytest.fixture
def no_device(pkg, monkeypatch):
    """Any attempt to reach the library fails the test (the refusals happen on the host)."""
    def boom(*a, **k):
        raise AssertionError("the library was touched before the refusal")
    monkeypatch.setattr(pkg.capi, "lib", boom)
    monkeypatch.setattr(pkg.capi.Context, "__init__", boom)
    monkeypatch.setattr(pkg.Session, "__init__", boom)
    return pkg


def test_header_declares_and_library_exports(pkg):
    hdr = open(os.path.join(ROOT, "include", "vbmf_hip.h")).read()
    tail = (r"\s*\(\s*vbmf_ctx\*\s*ctx?\s*,\s*int32_t\s+%s\s*,\s*void\*\s*dst\s*,\s*int32_t\s+dst_dtype\s*,\s*int32_t\s+dst_on_device\s*,"
            r"\s*int64_t\s+row0\s*,\s*int64_t\s+nrows\s*,\s*int64_t\s+row_stride\s*,\s*int64_t\s+col_stride\s*\)\s*;")
    assert re.search(r"int\s+vbmf_get_YHat_rows" + tail % "what", hdr)
    assert re.search(r"int\s+vbmf_get_factor_rows" + tail % "which", hdr)
    assert hdr.count("src/vbmf.jl:120-122") >= 3                        # vbmf_get_YHat and the two new entries cite updateYHat!
    for name, val in (("VBMF_DST_F64", 0), ("VBMF_DST_F32", 1), ("VBMF_DST_BF16", 2), ("VBMF_OUT_YHAT", 0), ("VBMF_OUT_RESIDUAL", 1),
                      ("VBMF_FACTOR_A", 0), ("VBMF_FACTOR_B", 1)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), hdr), name
        assert getattr(pkg.capi, name) == val
    lib = ctypes.CDLL(pkg.capi.LIB_PATH)
    for fn in ("vbmf_get_YHat_rows", "vbmf_get_factor_rows"):
        assert hasattr(lib, fn) and fn in pkg.capi.SYMBOLS
        assert len(getattr(pkg.capi.lib(), fn).argtypes) == 9
    for m in ("YHat_into", "factor_into"):
        assert callable(getattr(pkg.capi.Context, m))
    for m in ("yhat", "yhat_rows", "factors"):
        assert callable(getattr(pkg.Session, m))


def test_julia_host_binds_them():
    jl = open(os.path.join(G.PKG_DIR, "julia", "VBMatrixFactorizationHIP.jl")).read()
    assert len(re.findall(r"ccall\(\(:vbmf_get_YHat_rows,\s*libvbmf\)", jl)) == 2
    assert len(re.findall(r"ccall\(\(:vbmf_get_factor_rows,\s*libvbmf\)", jl)) == 2
    assert re.search(r"function get_YHat!\(c::Ctx,\s*dst::Array\{Float32,2\};\s*residual::Bool = false,\s*row0::Int = 0\)", jl)
    assert re.search(r"function get_YHat!\(c::Ctx,\s*dst::Array\{Float64,2\};\s*residual::Bool = false,\s*row0::Int = 0\)", jl)
    assert re.search(r"function get_factor!\(c::Ctx,\s*which::Symbol,\s*dst::Array\{Float32,2\}", jl)
    assert re.search(r"export[^\n]*(\n[^\n]*)*get_YHat!,\s*get_factor!", jl)


def test_y_sink_describes_a_destination_where_it_lies(no_device):
    capi = no_device.capi
    for dt, code in ((np.float64, capi.VBMF_DST_F64), (np.float32, capi.VBMF_DST_F32)):
        a = np.zeros((6, 4), dtype=dt)
        assert capi.y_sink(a)[1:] == (a.ctypes.data, code, 0, 4, 1, None) and capi.y_sink(a)[0] is a
        f = np.zeros((6, 4), dtype=dt, order="F")
        assert capi.y_sink(f)[1:] == (f.ctypes.data, code, 0, 1, 6, None)
        big = np.zeros((12, 12), dtype=dt)
        w = big[2:8, 3:7]                                               # one unit stride: written in place
        assert capi.y_sink(w)[1:] == (w.ctypes.data, code, 0, 12, 1, None)
        w = big.T[3:7, 2:8]
        assert capi.y_sink(w)[1:] == (w.ctypes.data, code, 0, 1, 12, None)
        v = big[::2, ::3]                                               # no unit stride: a temporary, assigned back by finish()
        tmp, addr, c2, on_dev, rs, cs, finish = capi.y_sink(v)
        assert tmp is not v and tmp.shape == v.shape and tmp.dtype == v.dtype and addr == tmp.ctypes.data
        assert (c2, on_dev, rs, cs) == (code, 0, 4, 1) and callable(finish)
        tmp[...] = np.arange(24, dtype=dt).reshape(6, 4)
        finish()
        assert np.array_equal(v, tmp) and big[1, 1] == 0 and big[0, 1] == 0
        r = big[::-1, :]                                                # a negative stride: the same route
        tmp, _, _, _, rs, cs, finish = capi.y_sink(r)
        assert (rs, cs) == (12, 1) and callable(finish)
    one = np.zeros((1, 5), dtype=np.float32)                            # a single row: lines cannot overlap
    assert capi.y_sink(one)[4:6] == (5, 1)


def test_y_sink_takes_cpu_tensors(no_device):
    torch = pytest.importorskip("torch")
    capi = no_device.capi
    for dt, code in ((torch.float64, capi.VBMF_DST_F64), (torch.float32, capi.VBMF_DST_F32), (torch.bfloat16, capi.VBMF_DST_BF16)):
        t = torch.zeros(6, 4, dtype=dt)
        assert capi.y_sink(t)[1:] == (t.data_ptr(), code, 0, 4, 1, None)
        assert capi.y_sink(t.t())[1:] == (t.data_ptr(), code, 0, 1, 4, None)
        big = torch.zeros(12, 12, dtype=dt)
        v = big[::2, ::3]
        tmp, addr, c2, on_dev, rs, cs, finish = capi.y_sink(v)
        assert tmp is not v and addr == tmp.data_ptr() and (c2, on_dev, rs, cs) == (code, 0, 4, 1)
        tmp.copy_(torch.arange(24).reshape(6, 4).to(dt))
        finish()
        assert torch.equal(v, tmp) and float(big[1, 1]) == 0.0


class _FakeGpuTensor:
    """what y_sink looks at, of a tensor on a GPU this machine need not have"""

    def __init__(self, torch, index):
        self.dtype, self.is_cuda, self.device, self.shape = torch.float32, True, torch.device("cuda", index), (6, 4)

    def dim(self):
        return 2

    def stride(self):
        return (4, 1)

    def data_ptr(self):
        raise AssertionError("refused before the address is taken")


def test_y_sink_refusals_come_before_the_library(no_device):
    capi = no_device.capi
    ro = np.zeros((6, 4))
    ro.setflags(write=False)
    with pytest.raises(ValueError, match="read-only"):
        capi.y_sink(ro)
    with pytest.raises(ValueError, match="read-only"):
        capi.y_sink(np.broadcast_to(np.zeros(4), (6, 4)))
    for bad in (np.zeros((6, 4), dtype=np.float16), np.zeros((6, 4), dtype=np.int32), np.zeros((6, 4), dtype=np.complex128)):
        with pytest.raises(TypeError, match="float64 or float32"):
            capi.y_sink(bad)
    for bad in (np.zeros(6), np.zeros((2, 3, 4))):
        with pytest.raises(ValueError, match="matrix"):
            capi.y_sink(bad)
    with pytest.raises(TypeError, match="NumPy array or a torch tensor"):
        capi.y_sink([[0.0, 1.0], [2.0, 3.0]])
    torch = pytest.importorskip("torch")
    with pytest.raises(TypeError, match="float64, float32 or bfloat16"):
        capi.y_sink(torch.zeros(6, 4, dtype=torch.float16))
    with pytest.raises(ValueError, match="matrix"):
        capi.y_sink(torch.zeros(6))
    with pytest.raises(ValueError, match="expanded"):
        capi.y_sink(torch.zeros(1, 4).expand(6, 4))
    with pytest.raises(ValueError, match="expanded"):
        capi.y_sink(torch.zeros(6, 1).expand(6, 4))
    with pytest.raises(ValueError, match="GPU 0"):
        capi.y_sink(_FakeGpuTensor(torch, 1), device=0)


def _bare_context(pkg, L=6, M=4, H=2):
    c = object.__new__(pkg.capi.Context)
    c.L, c.M, c.H, c.device, c._h = L, M, H, 0, None
    return c


def test_context_methods_check_the_block_on_the_host(no_device):
    c = _bare_context(no_device)
    with pytest.raises(ValueError, match=r"shape \(6, 4\)"):
        c.YHat_into(np.zeros((6, 5)))
    with pytest.raises(ValueError, match=r"shape \(3, 4\)"):
        c.YHat_into(np.zeros((6, 4)), row0=0, nrows=3)
    with pytest.raises(ValueError, match="do not lie"):
        c.YHat_into(np.zeros((3, 4)), row0=4)
    with pytest.raises(ValueError, match="matrix"):
        c.YHat_into(np.zeros(24))
    with pytest.raises(ValueError, match="'A' or 'B'"):
        c.factor_into("C", np.zeros((4, 2)))
    with pytest.raises(ValueError, match=r"shape \(4, 2\)"):
        c.factor_into("A", np.zeros((4, 3)))
    with pytest.raises(ValueError, match="do not lie"):
        c.factor_into("B", np.zeros((6, 2)), row0=1)
    with pytest.raises(ValueError, match="read-only"):
        c.YHat_into(np.broadcast_to(np.zeros(4), (6, 4)))


def test_fresh_results_are_allocated_as_asked(no_device):
    pkg = no_device
    a = pkg._alloc_out((6, 4), None, None, 0)
    assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.f_contiguous and a.shape == (6, 4)
    assert pkg._alloc_out((6, 4), np.float32, False, 0).dtype == np.float32
    assert pkg._alloc_out((6, 4), "float32", "cpu", 0).dtype == np.float32
    for bad in (np.float16, np.int64):
        with pytest.raises(TypeError):
            pkg._alloc_out((6, 4), bad, None, 0)
    torch = pytest.importorskip("torch")
    t = pkg._alloc_out((6, 4), torch.bfloat16, None, 0)                 # no NumPy twin: a CPU tensor
    assert t.dtype == torch.bfloat16 and not t.is_cuda and tuple(t.shape) == (6, 4)
    with pytest.raises(TypeError):
        pkg._alloc_out((6, 4), torch.float16, None, 0)
    with pytest.raises(ValueError, match="GPU 0"):
        pkg._alloc_out((6, 4), None, "cuda:1", 0)
    with pytest.raises(ValueError, match="GPU 0"):
        pkg._alloc_out((6, 4), None, 1, 0)
    with pytest.raises(ValueError, match="CPU or on the session's GPU"):
        pkg._alloc_out((6, 4), None, "meta", 0)
    out = np.zeros((6, 4), dtype=np.float32)
    assert pkg._out_or_new(out, (6, 4), None, None, 0) is out
    assert pkg._out_or_new(out, (6, 4), np.float32, None, 0) is out
    with pytest.raises(TypeError, match="dtype asks for"):
        pkg._out_or_new(out, (6, 4), np.float64, None, 0)
    with pytest.raises(TypeError, match="dtype asks for"):
        pkg._out_or_new(out, (6, 4), torch.float32, None, 0)
    tt = torch.zeros(6, 4)
    assert pkg._out_or_new(tt, (6, 4), torch.float32, None, 0) is tt and pkg._out_or_new(tt, (6, 4), np.float32, None, 0) is tt
    with pytest.raises(TypeError, match="dtype asks for"):
        pkg._out_or_new(tt, (6, 4), torch.float64, None, 0)


class _FakeSession:
    def __init__(self):
        self.calls = []
        self.ctx = self

    def push(self, p):
        self.calls.append("push")

    def YHat(self):
        self.calls.append("YHat")
        return "fp64 host array"

    def yhat(self, **kw):
        self.calls.append(("yhat", kw))
        return "new route"


def test_updateYHat_routes_its_arguments(no_device, monkeypatch):
    pkg = no_device
    s = _FakeSession()
    monkeypatch.setattr(pkg, "_session_for_params", lambda p: s)
    monkeypatch.setattr(pkg, "_session_for", lambda Y, H: s)
    rng = np.random.default_rng(0)
    Y = rng.standard_normal((6, 4))
    p = pkg.vbmf_init(Y, 2, rng=rng)
    pkg.updateYHat_(p)                                                  # today's path, untouched
    assert s.calls == ["push", "YHat"] and p.YHat == "fp64 host array"
    s.calls.clear()
    out = np.zeros((6, 4), dtype=np.float32)
    pkg.updateYHat_(p, out=out)
    assert s.calls == ["push", ("yhat", dict(out=out, dtype=None, device=False, residual=False))] and p.YHat == "new route"
    s.calls.clear()
    pkg.updateYHat_(p, Y, dtype=np.float32, residual=True)
    assert s.calls[1] == ("yhat", dict(out=None, dtype=np.float32, device=False, residual=True))
    s.calls.clear()
    with pytest.raises(ValueError, match="needs Y"):
        pkg.updateYHat_(p, residual=True)
    assert s.calls == []


def test_ard_shells_keep_the_host_product_unless_asked(no_device):
    pkg = no_device
    rng = np.random.default_rng(1)
    Y = rng.standard_normal((6, 4))
    p = pkg.vbmf_sparse_init(Y, 2, rng=rng)

    class Ctx:
        device = 0

        def YHat_into(self, dst, row0, nrows):
            self.got = (dst, row0, nrows)
            return dst
    c = Ctx()
    assert np.array_equal(pkg._ard_YHat(c, p, None, None), p.BHat @ p.AHat.T) and not hasattr(c, "got")
    r = pkg._ard_YHat(c, p, None, np.float32)
    assert r is c.got[0] and r.dtype == np.float32 and r.shape == (6, 4) and c.got[1:] == (0, 6)
    out = np.zeros((6, 4))
    assert pkg._ard_YHat(c, p, out, None) is out
    with pytest.raises(TypeError, match="dtype asks for"):
        pkg._ard_YHat(c, p, out, np.float32)
    import inspect
    for fn in (pkg.vbls_, pkg.vbmf_sparse_, pkg.vbmf_dual_, pkg.vbmf_trial_):
        sig = inspect.signature(fn).parameters
        assert sig["out"].default is None and sig["dtype"].default is None, fn.__name__
