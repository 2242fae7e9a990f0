"""Y from float32 arrays and torch tensors (vbmf_set_Y_rows / Context.set_Y_rows / Session.set_Y / the reference-style calls): the
parts that need no GPU.  A recording stand-in for the library shows WHAT the host hands over -- the caller's own address, dtype code
and element strides, with no float64 copy -- and a recording stand-in for the session shows WHEN the cached matrix is uploaded again."""
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


class RecordingLib:
    """Stands where libvbmf_hip.so would: records the arguments of the two upload entries, knows no other symbol."""

    def __init__(self):
        self.rows, self.whole = [], []

    def vbmf_set_Y_rows(self, h, addr, code, on_device, row0, nrows, rs, cs):
        self.rows.append(dict(addr=addr, code=code, on_device=on_device, row0=row0, nrows=nrows, rs=rs, cs=cs))
        return 0

    def vbmf_set_Y(self, h, ptr, ld):
        self.whole.append(ld)
        return 0

    def vbmf_destroy(self, h):
        return 0

    def vbmf_last_error(self, h):
        return b""


class UntouchableLib:
    def __getattr__(self, name):
        raise AssertionError(f"the host reached the library ({name}) before refusing")


def _ctx(pkg, L, M, lib, device=0):
    c = object.__new__(pkg.capi.Context)
    c._lib, c._h = lib, ctypes.c_void_p(1)
    c.L, c.M, c.H, c.device = L, M, 2, device
    return c


def _session(pkg, L, M, lib):
    s = object.__new__(pkg.Session)
    s.ctx, s.L, s.M, s.H = _ctx(pkg, L, M, lib), L, M, 2
    return s


@pytest.fixture
def count_copies(monkeypatch):
    """dtypes of every array np.ascontiguousarray / np.asfortranarray / np.asarray(dtype=...) hands back that is NOT its argument"""
    made = []

    def spy(fn):
        def wrapped(a, *args, **kw):
            out = fn(a, *args, **kw)
            if out is not a:
                made.append(out.dtype)
            return out
        return wrapped
    for name in ("ascontiguousarray", "asfortranarray", "asarray"):
        monkeypatch.setattr(np, name, spy(getattr(np, name)))
    return made


def test_symbol_is_declared_listed_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "vbmf_hip.h")).read()
    assert re.search(r"int\s+vbmf_set_Y_rows\s*\(\s*vbmf_ctx\*\s*ctx\s*,\s*const\s+void\*\s*src\s*,\s*int32_t\s+src_dtype\s*,\s*"
                     r"int32_t\s+src_on_device\s*,\s*int64_t\s+row0\s*,\s*int64_t\s+nrows\s*,\s*int64_t\s+row_stride\s*,\s*"
                     r"int64_t\s+col_stride\s*\)\s*;", hdr)
    for name, val in (("VBMF_SRC_F64", 0), ("VBMF_SRC_F32", 1), ("VBMF_SRC_BF16", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), hdr)
        assert getattr(pkg.capi, name) == val
    assert "vbmf_set_Y_rows" in pkg.capi.SYMBOLS
    assert hasattr(ctypes.CDLL(pkg.capi.LIB_PATH), "vbmf_set_Y_rows")
    assert len(pkg.capi.lib().vbmf_set_Y_rows.argtypes) == 8
    assert hasattr(pkg.capi.Context, "set_Y_rows") and hasattr(pkg.Session, "set_Y_rows")


def test_julia_host_binds_it():
    jl = open(os.path.join(G.PKG_DIR, "julia", "VBMatrixFactorizationHIP.jl")).read()
    assert re.search(r"ccall\(\(:vbmf_set_Y_rows,\s*libvbmf\)", jl)
    assert re.search(r"function set_Y!\(h::Ptr\{Cvoid\},\s*Y::Array\{Float32,2\}\)", jl)
    assert re.search(r"function vbmf!\(Y::Array\{Float32,2\},\s*params::vbmf_parameters,\s*niter::Int;", jl)


@pytest.mark.parametrize("layout", ["C", "F", "cols_stepped"])
def test_float32_array_goes_by_its_own_address(pkg, count_copies, layout):
    L, M = 12, 7
    rng = np.random.default_rng(0)
    if layout == "C":
        a = np.ascontiguousarray(rng.standard_normal((L, M)).astype(np.float32)); want = (M, 1)
    elif layout == "F":
        a = np.asfortranarray(rng.standard_normal((L, M)).astype(np.float32)); want = (1, L)
    else:
        big = np.asfortranarray(rng.standard_normal((L, 2 * M)).astype(np.float32))
        a = big[:, ::2]; want = (1, 2 * L)
    del count_copies[:]
    lib = RecordingLib()
    _session(pkg, L, M, lib).set_Y(a)
    assert lib.whole == [] and len(lib.rows) == 1
    r = lib.rows[0]
    assert r["addr"] == a.ctypes.data and r["code"] == pkg.capi.VBMF_SRC_F32 and r["on_device"] == 0
    assert (r["row0"], r["nrows"]) == (0, L) and (r["rs"], r["cs"]) == want
    assert count_copies == []                                  # no copy at all, so no float64 one


def test_view_without_a_unit_stride_is_copied_once_as_float32(pkg, count_copies):
    big = np.random.default_rng(1).standard_normal((24, 21)).astype(np.float32)
    a = big[::2, ::3]
    del count_copies[:]
    lib = RecordingLib()
    _ctx(pkg, 12, 7, lib).set_Y_rows(a)
    assert count_copies == [np.dtype(np.float32)]
    r = lib.rows[0]
    assert r["code"] == pkg.capi.VBMF_SRC_F32 and (r["rs"], r["cs"]) == (7, 1) and r["nrows"] == 12
    lo, hi = big.ctypes.data, big.ctypes.data + big.nbytes
    assert not lo <= r["addr"] < hi


def test_float64_array_keeps_going_through_set_Y(pkg):
    lib = RecordingLib()
    _session(pkg, 12, 7, lib).set_Y(np.zeros((12, 7)))
    assert lib.whole == [12] and lib.rows == []


def test_cpu_tensors_arrive_in_their_own_dtype(pkg):
    import torch
    L, M = 12, 7
    for dt, code in ((torch.bfloat16, pkg.capi.VBMF_SRC_BF16), (torch.float32, pkg.capi.VBMF_SRC_F32), (torch.float64, pkg.capi.VBMF_SRC_F64)):
        t = torch.randn(L, M, dtype=torch.float32).to(dt)
        tt = torch.randn(M, L, dtype=torch.float32).to(dt).t()                 # column-major
        lib = RecordingLib()
        s = _session(pkg, L, M, lib)
        s.set_Y(t)
        s.set_Y(tt)
        assert lib.whole == []
        assert [(r["addr"], r["code"], r["on_device"], r["rs"], r["cs"]) for r in lib.rows] == \
            [(t.data_ptr(), code, 0, M, 1), (tt.data_ptr(), code, 0, 1, L)]


def test_row_blocks_pass_row0_and_the_block_rows(pkg):
    lib = RecordingLib()
    s = _session(pkg, 70, 5, lib)
    a = np.ones((70, 5), dtype=np.float32)
    s.set_Y_rows(a[:64], 0)
    s.set_Y_rows(a[64:], 64)
    assert [(r["row0"], r["nrows"], r["addr"]) for r in lib.rows] == [(0, 64, a.ctypes.data), (64, 6, a.ctypes.data + 64 * 5 * 4)]


class _ElsewhereTensor:
    """Has the surface of a GPU tensor on device index 1; nothing behind it may be touched."""
    is_cuda = True
    shape = (12, 7)

    def __init__(self):
        import torch
        self.dtype, self.device = torch.float32, torch.device("cuda", 1)

    def dim(self):
        return 2

    def stride(self):
        return (7, 1)

    def data_ptr(self):
        raise AssertionError("the address of a tensor on another device was taken")


def test_refusals_happen_before_the_library_is_touched(pkg):
    import torch
    lib = UntouchableLib()
    c, s = _ctx(pkg, 12, 7, lib), _session(pkg, 12, 7, lib)
    with pytest.raises(ValueError, match="matrix"):
        c.set_Y_rows(np.zeros(12, dtype=np.float32))
    with pytest.raises(ValueError, match="matrix"):
        s.set_Y(torch.zeros(12, 7, 1))
    with pytest.raises(TypeError, match="float"):
        c.set_Y_rows(np.zeros((12, 7), dtype=np.int32))
    with pytest.raises(TypeError, match="float"):
        s.set_Y(torch.zeros(12, 7, dtype=torch.int64))
    with pytest.raises(TypeError, match="float"):
        s.set_Y(torch.zeros(12, 7, dtype=torch.float16))
    with pytest.raises(ValueError, match="shape"):
        s.set_Y(np.zeros((12, 8), dtype=np.float32))
    with pytest.raises(ValueError, match="shape"):
        s.set_Y(torch.zeros(11, 7))
    with pytest.raises(ValueError, match="shape"):
        c.set_Y_rows(np.zeros((12, 6), dtype=np.float32))
    with pytest.raises(ValueError, match="rows"):
        c.set_Y_rows(np.zeros((12, 7), dtype=np.float32), row0=32)
    with pytest.raises(ValueError, match="cuda:1"):
        s.set_Y(_ElsewhereTensor())


class RecordingSession:
    made = []

    def __init__(self, L, M, H, **kw):
        self.L, self.M, self.H, self.ctx, self.uploads = L, M, H, self, []
        RecordingSession.made.append(self)

    def set_Y(self, Y):
        self.uploads.append((type(Y).__name__, str(Y.dtype)))

    def push(self, p):
        pass

    def step(self, which):
        pass

    def run(self, k, **kw):
        return k, 0.0, None

    def pull(self, p, want_B=True):
        return p

    def YHat(self):
        return np.zeros((self.L, self.M))

    def close(self):
        pass


@pytest.fixture
def recorded(pkg, monkeypatch):
    monkeypatch.setattr(pkg, "Session", RecordingSession)
    monkeypatch.setattr(pkg, "_sessions", {})
    RecordingSession.made = []
    return pkg


def test_vbmf_uploads_a_cpu_tensor_once_and_again_after_an_in_place_edit(recorded):
    import torch
    pkg = recorded
    Y = torch.randn(20, 9, dtype=torch.float32)
    p = pkg.vbmf_init(Y, 3, rng=np.random.default_rng(0))
    assert (p.L, p.M) == (20, 9)
    pkg.vbmf_(Y, p, 2)
    pkg.vbmf_(Y, p, 2)
    assert len(RecordingSession.made) == 1 and RecordingSession.made[0].uploads == [("Tensor", "torch.float32")]
    Y.mul_(2)
    pkg.vbmf_(Y, p, 2)
    pkg.updateA_(Y, p)
    assert len(RecordingSession.made) == 1 and len(RecordingSession.made[0].uploads) == 2


def test_vbmf_uploads_a_float32_array_once_and_again_after_an_in_place_edit(recorded):
    pkg = recorded
    Y = np.random.default_rng(2).standard_normal((20, 9)).astype(np.float32)
    p = pkg.vbmf_init(Y, 3, rng=np.random.default_rng(0))
    pkg.vbmf_(Y, p, 2)
    pkg.vbmf(Y, p, 2)
    assert len(RecordingSession.made) == 1 and RecordingSession.made[0].uploads == [("ndarray", "float32")]
    Y *= 2
    pkg.vbmf_(Y, p, 2)
    assert len(RecordingSession.made) == 1 and RecordingSession.made[0].uploads == [("ndarray", "float32")] * 2
