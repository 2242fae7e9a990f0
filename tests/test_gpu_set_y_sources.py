"""vbmf_set_Y_rows on the GPU: Y from device memory and from float32 / bfloat16 / float64 sources in any layout, whole or in row
blocks, must leave the context EXACTLY as vbmf_set_Y leaves it when given the same values as float64 -- both tiled copies bit for
bit over the whole tiled buffers (pad tiles included), get_Y bit for bit, and ||Y||^2 to the bound that holds for any order of fp64
summation of non-negative terms (relative L M 2^-52).  The shapes have a partial x tile, a partial k-step in both storage types and
more than one 32-row block.  No test here passes a host pointer as device memory or an extent that leaves its allocation: if those
two checks were wrong such a test would make a kernel read the bad address."""
import copy

import numpy as np
import pytest

import __graft_entry__ as G

pytestmark = pytest.mark.gpu

SHAPES = [(77, 45, 4), (33, 31, 2), (130, 70, 5)]
CONFIGS = [(L, M, H, y, "basic") for (L, M, H) in SHAPES for y in ("f32", "bf16")] + [(77, 45, 4, "f32", "diagvar")]
DTYPES = ["float64", "float32", "bfloat16"]


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


def _ctx(pkg, cfg):
    L, M, H, y, variant = cfg
    return pkg.capi.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32 if y == "f32" else pkg.VBMF_Y_BF16,
                            variant=pkg.VBMF_VARIANT_SPARSE_DIAGVAR if variant == "diagvar" else pkg.capi.VBMF_VARIANT_BASIC)


def _snapshot(pkg, c):
    d = c.dims()
    return dict(Y1=c.peek(pkg.capi.PEEK_Y1, d["XT1"] * d["KS1"] * 64 * 4), Y2=c.peek(pkg.capi.PEEK_Y2, d["XT2"] * d["KS2"] * 64 * 4),
                Y=c.get_Y(), tr=c.trYY())


def _same(got, want, L, M, what):
    for k in ("Y1", "Y2"):
        assert np.array_equal(got[k], want[k]), (what, k, int(np.sum(got[k] != want[k])))
    assert np.array_equal(got["Y"].view(np.uint64), want["Y"].view(np.uint64)), (what, "get_Y")
    bound = L * M * 2.0 ** -52
    rel = abs(got["tr"] - want["tr"]) / want["tr"]
    print(f"{what}: trYY rel {rel:.3e} (bound {bound:.3e})")
    assert rel <= bound, (what, rel, bound)


def _values(L, M, dtype, seed):
    """a GPU tensor of the source dtype and the float64 array of exactly its values"""
    import torch
    base = np.random.default_rng(seed).standard_normal((L, M)) * 3.0
    t = torch.from_numpy(base).to(getattr(torch, dtype)).cuda()
    return t, t.double().cpu().numpy()


_reference = {}


def _ref(pkg, cfg, dtype):
    """what vbmf_set_Y leaves for the values of (cfg, dtype): computed once, shared, never changed"""
    key = (cfg, dtype)
    if key not in _reference:
        L, M = cfg[0], cfg[1]
        t, Y64 = _values(L, M, dtype, 100 + 7 * L + M)
        with _ctx(pkg, cfg) as c:
            c.set_Y(Y64)
            snap = _snapshot(pkg, c)
        for v in snap.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _reference[key] = (t, Y64, snap)
    return _reference[key]


def _layouts(t):
    import torch
    L, M = t.shape
    yield "row-major", t.contiguous()
    yield "column-major", t.t().contiguous().t()
    big = torch.zeros(L + 9, M + 11, dtype=t.dtype, device=t.device)
    big[3:3 + L, 5:5 + M] = t
    yield "window", big[3:3 + L, 5:5 + M]
    big = torch.full((2 * L, 3 * M), 7.0, dtype=t.dtype, device=t.device)
    big[::2, ::3] = t
    yield "stepped", big[::2, ::3]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "%dx%d_H%d_%s_%s" % c)
def test_tiles_are_those_of_set_Y_bit_for_bit(pkg, cfg, dtype):
    L, M = cfg[0], cfg[1]
    t, Y64, want = _ref(pkg, cfg, dtype)
    with _ctx(pkg, cfg) as c:
        for name, src in _layouts(t):
            assert tuple(src.shape) == (L, M)
            c.set_Y_rows(src)
            _same(_snapshot(pkg, c), want, L, M, f"{cfg} gpu {dtype} {name}")
        if dtype == "float32":
            a = t.cpu().numpy()
            for name, src in (("C", np.ascontiguousarray(a)), ("F", np.asfortranarray(a))):
                c.set_Y_rows(src)
                _same(_snapshot(pkg, c), want, L, M, f"{cfg} host float32 {name}")


@pytest.mark.parametrize("where", ["gpu", "host"])
@pytest.mark.parametrize("y", ["f32", "bf16"])
def test_row_blocks_give_the_one_shot_result(pkg, y, where):
    cfg = (130, 70, 5, y, "basic")
    L, M, H = cfg[:3]
    t, Y64, want = _ref(pkg, cfg, "float32")
    src = t if where == "gpu" else t.cpu().numpy()
    rng = np.random.default_rng(5)
    z = np.zeros((H, H))
    with _ctx(pkg, cfg) as c:
        c.set_state(rng.standard_normal((M, H)), rng.standard_normal((L, H)), z, z, np.ones(H), np.ones(H), 1.0)
        c.set_Y_rows(src[0:64], 0)
        with pytest.raises(pkg.VbmfError, match="no Y") as e:
            c.run(1, eps=0.0)
        assert e.value.code == pkg.capi.VBMF_ERR_INVALID
        with pytest.raises(pkg.VbmfError, match="no Y"):
            c.get_Y()
        with pytest.raises(pkg.VbmfError, match="order"):       # a block out of order is refused and changes nothing ...
            c.set_Y_rows(src[96:130], 96)
        c.set_Y_rows(src[64:96], 64)                             # ... so the block that is due is still accepted
        c.set_Y_rows(src[96:130], 96)
        _same(_snapshot(pkg, c), want, L, M, f"{cfg} {where} blocks")
        it, d, _ = c.run(1, eps=0.0)
        assert it == 1 and np.isfinite(d)


def test_refusals_leave_the_context_untouched(pkg):
    import torch
    cfg = (130, 70, 5, "f32", "basic")
    L, M, H = cfg[:3]
    t, Y64, want = _ref(pkg, cfg, "float32")
    a = np.ascontiguousarray(t.cpu().numpy())                    # (130, 70) float32, row stride 70, column stride 1
    wide = np.zeros((2 * L, 2 * M), dtype=np.float32)           # room for a (140, 2)-strided block
    F32, INVALID = pkg.capi.VBMF_SRC_F32, pkg.capi.VBMF_ERR_INVALID
    rng = np.random.default_rng(6)
    z = np.zeros((H, H))
    cases = {
        "row0 = 16": (a.ctypes.data, F32, 0, 16, 32, M, 1),
        "out of order": (a.ctypes.data, F32, 0, 64, 32, M, 1),
        "past L": (a.ctypes.data, F32, 0, 96, 64, M, 1),
        "whole but too long": (wide.ctypes.data, F32, 0, 0, L + 30, 2 * M, 1),
        "nrows = 40 in the middle": (a.ctypes.data, F32, 0, 0, 40, M, 1),
        "dtype 7": (a.ctypes.data, 7, 0, 0, L, M, 1),
        "row stride 0": (a.ctypes.data, F32, 0, 0, L, 0, 1),
        "column stride 0": (a.ctypes.data, F32, 0, 0, L, 1, 0),
        "host source, no unit stride": (wide.ctypes.data, F32, 0, 0, L, 2 * 2 * M, 2),
        "NULL": (None, F32, 0, 0, L, M, 1),
        "device pointer passed as host memory": (t.contiguous().data_ptr(), F32, 0, 0, L, M, 1),
    }
    with _ctx(pkg, cfg) as c:
        c.set_Y(Y64)
        c.set_state(rng.standard_normal((M, H)), rng.standard_normal((L, H)), z, z, np.ones(H), np.ones(H), 1.0)
        before = c.get_state()
        for name, args in cases.items():
            rc = c._lib.vbmf_set_Y_rows(c._h, *args)
            assert rc == INVALID, (name, rc)
            assert "vbmf_set_Y_rows" in c._lib.vbmf_last_error(c._h).decode(), name
            _same(_snapshot(pkg, c), want, L, M, f"after the refusal '{name}'")
        after = c.get_state()
        for k, v in before.items():
            assert np.array_equal(v, after[k]), k
        torch.cuda.synchronize()


def test_fit_from_a_gpu_tensor_equals_the_fit_from_float64(pkg):
    import torch
    L, M, H = 200, 60, 4
    t = (torch.from_numpy(np.random.default_rng(11).standard_normal((L, M))).float() * 2.0).cuda()
    Y64 = t.double().cpu().numpy()
    pkg.set_defaults(y_dtype=pkg.VBMF_Y_F32)
    p0 = pkg.vbmf_init(Y64, H, ca=0.1, cb=0.1, sigma2=0.1, rng=np.random.default_rng(12))
    pt, pn = copy.deepcopy(p0), copy.deepcopy(p0)
    try:
        pkg.vbmf_(t, pt, 3, eps=0.0, est_covs=True, est_var=True)
        pkg.vbmf_(Y64, pn, 3, eps=0.0, est_covs=True, est_var=True)
    finally:
        pkg.invalidate()
    for f in ("AHat", "BHat", "SigmaA", "SigmaB"):
        assert np.array_equal(getattr(pt, f), getattr(pn, f)), f
    assert pt.sigma2 == pn.sigma2 and np.isfinite(pt.sigma2)
