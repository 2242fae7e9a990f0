"""vbmf_get_YHat_rows / vbmf_get_factor_rows on the GPU: BHat*AHat', the residual Y - BHat*AHat' and the factors
written into the caller's memory -- host or device, float64 / float32 / bfloat16, any strides, whole or in row blocks.

Reference, per case: the factors as get_state() / sparse_get_state() return them (the fp32 values the device holds), Y64 = B @ A.T in
NumPy fp64, S = |B| @ |A|.T, Ystored = get_Y(), u = 2^-24.
  derived     F64 dst: |out - Y64| <= 2 H 2^-53 S per entry (any order of fp64 summation), and the same against ctx.YHat();
              F64 residual: 2 H 2^-53 S + 2^-53 |R64| against R64 = Ystored - Y64;
              BF16 dst: bitwise torch's rounding of the F32 dst of the same call; factors: bitwise (F32 a copy, F64 a widening, BF16 RNE)
  measured    F32 dst: the a-priori (H + 1) u S is too loose to catch a dropped low-order term at H >= 33, so the test runs the NumPy
              float32 k-ordered chain acc = fl(acc + fl(b_h a_h)) on the same factors, r_ref = max |chain - Y64| / (u S), and asserts
              max |out - Y64| / (u S) <= 2 r_ref (the reference chain rounds twice per term where fmaf rounds once; the factor also
              allows another fixed order); the F32 residual the same plus u |R64|.  Both figures are printed and filed per case in
              build/outputs_parity.txt (a copy of an MI355X run: profiles/outputs_parity.txt).
  bitwise     per dst dtype and `what`: row-major = column-major = a window inside a larger tensor = a stepped view big[::2, ::3];
              GPU dst = host dst; row blocks = the rows of the whole-matrix call.  Windows and stepped views live in tensors
              pre-filled with a sentinel bit pattern that must survive everywhere outside the view.
No test here passes a host pointer as device memory or an extent that leaves its allocation: if those two checks were wrong such a
test would make a kernel write the bad address (they precede every launch and copy: check_dst in csrc/vbmf_hip.hip)."""
import os

import numpy as np
import pytest

import __graft_entry__ as G

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SHAPES = [(70, 45, 5), (257, 130, 33), (129, 131, 130)]      # < one tile, Hp = 32 | one past a tile edge both ways, Hp = 64 | Hp = 256
CASES = [(L, M, H, y, "basic") for (L, M, H) in SHAPES for y in ("f32", "bf16")] + [(70, 45, 5, "f32", "sparse")]
IDS = ["%dx%d_H%d_%s_%s" % c for c in CASES]
DTYPES = ["float64", "float32", "bfloat16"]
REPORT = os.path.join(G.ROOT, "build", "outputs_parity.txt")           # (build/ is not tracked)
HYPER = dict(alpha0=1e-10, beta0=1e-10, gamma0=1e-10, delta0=1e-10, eta0=1e-10, zeta0=1e-10)


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


def _file(line):
    print(line)
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "a") as f:
        f.write(line + "\n")


def _load(pkg, c, cfg):
    L, M, H, y, variant = cfg
    rng = np.random.default_rng(1000 + 13 * L + 7 * M + H + (y == "bf16"))
    c.set_Y(rng.standard_normal((L, M)) * 2.0)
    A, B = rng.standard_normal((M, H)), rng.standard_normal((L, H)) * np.linspace(0.5, 2.0, H)
    if variant == "sparse":
        one = np.ones(M * H)
        c.sparse_set_state(A.reshape(-1), one, one, one, B, 0.1 * np.eye(H), np.ones(H), np.ones(H), 1.0, 1.0, HYPER)
    else:
        z = np.zeros((H, H))
        c.set_state(A, B, z, z, np.ones(H), np.ones(H), 1.0)


def _factors(c, cfg):
    L, M, H, _, variant = cfg
    if variant == "sparse":
        s = c.sparse_get_state()
        return s["ATVecHat"].reshape(M, H), s["BHat"]
    s = c.get_state()
    return s["AHat"], s["BHat"]


def _chain32(A, B):
    """the NumPy float32 chain in the order h = 0, 1, ...: acc = fl(acc + fl(b_h a_h))"""
    A32, B32 = A.astype(np.float32), B.astype(np.float32)
    acc = np.zeros((B.shape[0], A.shape[0]), dtype=np.float32)
    for h in range(A.shape[1]):
        acc = acc + B32[:, h:h + 1] * A32[:, h][None, :]
    return acc.astype(np.float64)


class _Case:
    """A context with its state and Y, and the reference: computed once, shared by the tests, never changed."""

    def __init__(self, pkg, cfg):
        L, M, H, y, variant = cfg
        self.cfg, self.L, self.M, self.H = cfg, L, M, H
        self.c = pkg.capi.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32 if y == "f32" else pkg.VBMF_Y_BF16,
                                  variant=pkg.VBMF_VARIANT_SPARSE_DIAG if variant == "sparse" else pkg.capi.VBMF_VARIANT_BASIC)
        _load(pkg, self.c, cfg)
        self.A, self.B = _factors(self.c, cfg)
        assert np.array_equal(self.A, self.A.astype(np.float32)) and np.array_equal(self.B, self.B.astype(np.float32))
        self.Y64 = self.B @ self.A.T
        self.S = np.abs(self.B) @ np.abs(self.A).T
        self.Ys = self.c.get_Y()
        self.R64 = self.Ys - self.Y64
        self.r_ref = float(np.max(np.abs(_chain32(self.A, self.B) - self.Y64) / (U * self.S)))
        for v in (self.A, self.B, self.Y64, self.S, self.Ys, self.R64):
            v.setflags(write=False)
        self._base = {}

    def base(self, dtype, residual):
        """the whole-matrix result in a row-major GPU tensor: what every other layout must equal bit for bit"""
        import torch
        key = (dtype, residual)
        if key not in self._base:
            t = torch.empty((self.L, self.M), dtype=getattr(torch, dtype), device="cuda")
            self.c.YHat_into(t, residual=residual)
            self._base[key] = t
        return self._base[key]


@pytest.fixture(scope="module")
def cases(pkg):
    made = {}

    def get(cfg):
        if cfg not in made:
            made[cfg] = _Case(pkg, cfg)
        return made[cfg]
    yield get
    for k in made.values():
        k.c.close()


def _bits(t):
    import torch
    return t.view({8: torch.int64, 4: torch.int32, 2: torch.int16}[t.element_size()])


def _sentinel(rows, cols, dtype, device):
    """a tensor whose every byte is 0x5A"""
    import torch
    es = torch.empty((), dtype=dtype).element_size()
    return torch.full((rows, cols * es), 0x5A, dtype=torch.uint8, device=device).view(dtype)


def _views(L, M, dtype, device="cuda"):
    """(name, the tensor that owns the memory, the L x M view to fill)"""
    import torch
    t = _sentinel(M, L, dtype, device)
    yield "column-major", t, t.t()
    big = _sentinel(L + 9, M + 11, dtype, device)
    yield "window", big, big[3:3 + L, 5:5 + M]
    big = _sentinel(2 * L, 3 * M, dtype, device)
    yield "stepped", big, big[::2, ::3]
    big = _sentinel(3 * M, 2 * L, dtype, device)
    yield "stepped column-major", big, big[::3, ::2].t()


def _expect_only_view_written(owner, view, want, what):
    """owner equals a sentinel tensor with `want` assigned to the view: the view holds the result, every other byte is untouched"""
    import torch
    exp = torch.full_like(owner.view(torch.uint8), 0x5A).view(owner.dtype)
    exp.as_strided(view.shape, view.stride(), view.storage_offset())[...] = want.to(exp.device)
    assert torch.equal(_bits(owner), _bits(exp)), (what, int((_bits(owner) != _bits(exp)).sum()))


@pytest.mark.parametrize("cfg", CASES, ids=IDS)
def test_values_against_the_fp64_product(pkg, cases, cfg):
    import torch
    k = cases(cfg)
    H, S, Y64, R64 = k.H, k.S, k.Y64, k.R64
    b64 = 2.0 * H * 2.0 ** -53 * S
    # float64: derived bounds, and the parent's route
    y64 = k.base("float64", False).cpu().numpy()
    r64 = k.base("float64", True).cpu().numpy()
    e64, er64 = np.abs(y64 - Y64), np.abs(r64 - R64)
    print(f"{cfg}: F64 max err/bound {np.max(e64 / b64):.3f}, residual {np.max(er64 / (b64 + 2.0 ** -53 * np.abs(R64))):.3f}")
    assert np.all(e64 <= b64)
    assert np.all(er64 <= b64 + 2.0 ** -53 * np.abs(R64))
    assert np.all(np.abs(y64 - k.c.YHat()) <= b64)
    # float32: measured against the float32 chain of the same factors
    y32 = k.base("float32", False).double().cpu().numpy()
    r32 = k.base("float32", True).double().cpu().numpy()
    ry = float(np.max(np.abs(y32 - Y64) / (U * S)))
    rr = float(np.max((np.abs(r32 - R64) - U * np.abs(R64)) / (U * S)))
    _file("%dx%d H=%d %s %s: r_ref %.3f  yhat_f32 %.3f  residual_f32 %.3f  (limit %.3f)" % (*cfg, k.r_ref, ry, rr, 2 * k.r_ref))
    assert ry <= 2 * k.r_ref
    assert rr <= 2 * k.r_ref
    # bfloat16: the rounding of the float32 result, bit for bit
    for residual in (False, True):
        assert torch.equal(_bits(k.base("bfloat16", residual)), _bits(k.base("float32", residual).to(torch.bfloat16))), residual


@pytest.mark.parametrize("residual", [False, True], ids=["yhat", "residual"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", CASES, ids=IDS)
def test_every_layout_and_place_gives_the_same_bits(pkg, cases, cfg, dtype, residual):
    import torch
    k = cases(cfg)
    L, M = k.L, k.M
    want = k.base(dtype, residual)
    td = getattr(torch, dtype)
    for name, owner, view in _views(L, M, td):
        assert tuple(view.shape) == (L, M)
        k.c.YHat_into(view, residual=residual)
        _expect_only_view_written(owner, view, want, (cfg, dtype, residual, name))
    # row blocks, into a window of a sentinel tensor
    cuts = [b for b in (0, 37, 87) if b < L] + [L]
    owner = _sentinel(L + 2, M + 3, td, "cuda")
    view = owner[1:1 + L, 2:2 + M]
    for a, b in zip(cuts[:-1], cuts[1:]):
        k.c.YHat_into(view[a:b], row0=a, residual=residual)
    _expect_only_view_written(owner, view, want, (cfg, dtype, residual, "row blocks"))
    # host memory
    hw = want.cpu()
    if dtype != "bfloat16":
        nd = np.dtype(dtype)
        for order in ("C", "F"):
            a = np.empty((L, M), dtype=nd, order=order)
            k.c.YHat_into(a, residual=residual)
            assert np.array_equal(a.view(f"i{nd.itemsize}"), hw.numpy().view(f"i{nd.itemsize}")), (cfg, dtype, residual, "host", order)
        big = np.frombuffer(bytes([0x5A]) * (2 * L * 3 * M * nd.itemsize), dtype=nd).reshape(2 * L, 3 * M).copy()
        k.c.YHat_into(big[::2, ::3], residual=residual)                  # no unit stride: through y_sink's temporary
        exp = np.frombuffer(bytes([0x5A]) * (2 * L * 3 * M * nd.itemsize), dtype=nd).reshape(2 * L, 3 * M).copy()
        exp[::2, ::3] = hw.numpy()
        assert np.array_equal(big.view(f"i{nd.itemsize}"), exp.view(f"i{nd.itemsize}")), (cfg, dtype, residual, "host stepped")
        blocks = np.empty((L, M), dtype=nd)
        for a_, b_ in zip(cuts[:-1], cuts[1:]):
            k.c.YHat_into(blocks[a_:b_], row0=a_, residual=residual)
        assert np.array_equal(blocks.view(f"i{nd.itemsize}"), hw.numpy().view(f"i{nd.itemsize}")), (cfg, dtype, residual, "host blocks")
    else:
        for name, owner, view in list(_views(L, M, td, "cpu"))[:2]:      # column-major, window (one unit stride: written in place)
            k.c.YHat_into(view, residual=residual)
            _expect_only_view_written(owner, view, hw, (cfg, dtype, residual, "host", name))


@pytest.mark.parametrize("cfg", [CASES[2], CASES[5], CASES[6]], ids=[IDS[2], IDS[5], IDS[6]])
def test_factors_are_the_stored_fp32_values(pkg, cases, cfg):
    import torch
    k = cases(cfg)
    for which, F in (("A", k.A), ("B", k.B)):
        X, H = F.shape
        f32 = torch.from_numpy(F.astype(np.float32))
        want = {"float32": f32, "float64": torch.from_numpy(np.array(F, order="C")), "bfloat16": f32.to(torch.bfloat16)}
        cuts = [b for b in (0, 37, 87) if b < X] + [X]
        for dtype in DTYPES:
            td = getattr(torch, dtype)
            w = want[dtype]
            t = torch.empty((X, H), dtype=td, device="cuda")
            k.c.factor_into(which, t)
            assert torch.equal(_bits(t.cpu()), _bits(w)), (cfg, which, dtype)
            for name, owner, view in _views(X, H, td):
                k.c.factor_into(which, view)
                _expect_only_view_written(owner, view, w, (cfg, which, dtype, name))
            owner = _sentinel(X + 2, H + 3, td, "cuda")
            view = owner[1:1 + X, 2:2 + H]
            for a, b in zip(cuts[:-1], cuts[1:]):
                k.c.factor_into(which, view[a:b], row0=a)
            _expect_only_view_written(owner, view, w, (cfg, which, dtype, "row blocks"))
            if dtype != "bfloat16":
                for order in ("C", "F"):
                    a = np.empty((X, H), dtype=np.dtype(dtype), order=order)
                    k.c.factor_into(which, a)
                    assert np.array_equal(a.view(f"i{a.itemsize}"), w.numpy().view(f"i{a.itemsize}")), (cfg, which, dtype, order)
    st = k.c.sparse_get_state() if cfg[4] == "sparse" else k.c.get_state()
    assert np.array_equal(st["BHat"], k.B)                              # the state is as it was


def test_after_a_gram_form_run_the_first_call_pays_B_once(pkg, monkeypatch):
    import torch
    L, M, H = 400, 96, 16
    rng = np.random.default_rng(77)
    Y = (rng.standard_normal((L, H)) * np.linspace(1.0, 3.0, H)) @ rng.standard_normal((M, H)).T + 0.05 * rng.standard_normal((L, M))
    monkeypatch.setenv("VBMF_GRAM", "1")
    c = pkg.capi.Context(L, M, H, y_dtype=pkg.VBMF_Y_BF16, factor_dtype=pkg.VBMF_FACTOR_BF16X2)
    monkeypatch.delenv("VBMF_GRAM")
    with c:
        c.set_Y(Y)
        z = np.zeros((H, H))
        c.set_state(rng.standard_normal((M, H)), rng.standard_normal((L, H)), z, z, 0.1 * np.ones(H), 0.1 * np.ones(H), 0.1)
        c.run(5, eps=0.0, est_covs=True, est_var=True)
        d = c.dims()
        assert d["gram"] == 1 and d["b_pending"] == 1
        n0 = d["b_materialised"]
        t = torch.empty((L, M), dtype=torch.float32, device="cuda")
        c.YHat_into(t)
        d = c.dims()
        assert d["b_materialised"] == n0 + 1 and d["b_pending"] == 0
        s = c.get_state()
        A, B = s["AHat"], s["BHat"]
        Y64, S = B @ A.T, np.abs(B) @ np.abs(A).T
        r_ref = float(np.max(np.abs(_chain32(A, B) - Y64) / (U * S)))
        r = float(np.max(np.abs(t.double().cpu().numpy() - Y64) / (U * S)))
        _file(f"gram form {L}x{M} H={H} bf16: r_ref {r_ref:.3f}  yhat_f32 {r:.3f}  (limit {2 * r_ref:.3f})")
        assert r <= 2 * r_ref
        t2 = torch.empty_like(t)
        c.YHat_into(t2)
        c.factor_into("B", torch.empty((L, H), dtype=torch.float32, device="cuda"))
        assert c.dims()["b_materialised"] == n0 + 1
        assert torch.equal(_bits(t), _bits(t2))


def test_refusals_leave_the_context_and_dst_untouched(pkg, cases):
    import torch
    cfg = CASES[2]
    k = cases(cfg)
    c, L, M, H = k.c, k.L, k.M, k.H
    F32, INVALID = pkg.capi.VBMF_DST_F32, pkg.capi.VBMF_ERR_INVALID
    dev = _sentinel(2 * L, 2 * M, torch.float32, "cuda")               # room for every extent asked for below
    host = np.frombuffer(bytes([0x5A]) * (2 * L * 2 * M * 4), dtype=np.float32).copy()
    hp, dp = host.ctypes.data, dev.data_ptr()
    # (what / which, dst, dtype, on_device, row0, nrows, row stride, column stride)
    common = {
        "NULL": (0, None, F32, 1, 0, L, M, 1),
        "selector 2": (2, dp, F32, 1, 0, L, M, 1),
        "selector -1": (-1, dp, F32, 1, 0, L, M, 1),
        "dtype 3": (0, dp, 3, 1, 0, L, M, 1),
        "dtype -1": (0, hp, -1, 0, 0, L, M, 1),
        "row stride 0": (0, dp, F32, 1, 0, L, 0, 1),
        "column stride 0": (0, dp, F32, 1, 0, L, 1, 0),
        "row stride -M": (0, hp, F32, 0, 0, L, -M, 1),
        "column stride -1": (0, dp, F32, 1, 0, L, M, -1),
        "nrows 0": (0, dp, F32, 1, 0, 0, M, 1),
        "nrows -1": (0, hp, F32, 0, 0, -1, M, 1),
        "row0 -1": (0, dp, F32, 1, -1, 10, M, 1),
        "device dst, both strides 1": (0, dp, F32, 1, 0, 8, 1, 1),
        "device dst, row stride shorter than a row": (0, dp, F32, 1, 0, 8, 2, 1),
        "host dst, lines overlap": (0, hp, F32, 0, 0, 8, 2, 1),
        "host dst, no unit stride": (0, hp, F32, 0, 0, 8, 4 * M, 2),
        "device pointer passed as host memory": (0, dp, F32, 0, 0, 8, 2 * M, 1),
    }
    yhat = dict(common)
    yhat["past L"] = (0, dp, F32, 1, L - 10, 20, M, 1)
    yhat["row0 = L"] = (0, hp, F32, 0, L, 1, M, 1)
    fac = dict(common)
    fac["A: past M"] = (0, dp, F32, 1, M - 10, 20, H, 1)
    fac["B: past L"] = (1, dp, F32, 1, L - 10, 20, H, 1)
    before = c.get_state()
    for fn, table in (("vbmf_get_YHat_rows", yhat), ("vbmf_get_factor_rows", fac)):
        for name, args in table.items():
            rc = getattr(c._lib, fn)(c._h, *args)
            assert rc == INVALID, (fn, name, rc)
            assert fn in c._lib.vbmf_last_error(c._h).decode(), (fn, name)
    torch.cuda.synchronize()
    assert bool((dev.view(torch.uint8) == 0x5A).all())
    assert np.all(host.view(np.uint8) == 0x5A)
    after = c.get_state()
    for key, v in before.items():
        assert np.array_equal(v, after[key]), key
    # the residual needs Y; the product does not
    with pkg.capi.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32) as c2:
        t = _sentinel(L, M, torch.float32, "cuda")
        rc = c2._lib.vbmf_get_YHat_rows(c2._h, 0, t.data_ptr(), F32, 1, 0, L, M, 1)
        assert rc == INVALID and "no state" in c2._lib.vbmf_last_error(c2._h).decode()
        z = np.zeros((H, H))
        c2.set_state(k.A, k.B, z, z, np.ones(H), np.ones(H), 1.0)
        with pytest.raises(pkg.VbmfError, match="no Y") as e:
            c2.YHat_into(t, residual=True)
        assert e.value.code == INVALID and "vbmf_get_YHat_rows" in str(e.value)
        assert bool((t.view(torch.uint8) == 0x5A).all())
        c2.YHat_into(t)
        assert torch.equal(_bits(t), _bits(k.base("float32", False)))


def test_python_shells(pkg):
    import torch
    L, M, H = 257, 130, 33
    rng = np.random.default_rng(21)
    Yt = (torch.from_numpy(rng.standard_normal((L, M))).float() * 2.0).cuda()
    Y64 = Yt.double().cpu().numpy()
    pkg.set_defaults(y_dtype=pkg.VBMF_Y_F32)
    p = pkg.vbmf_init(Y64, H, ca=0.1, cb=0.1, sigma2=0.1, rng=np.random.default_rng(22))
    A, B = p.AHat.astype(np.float32).astype(np.float64), p.BHat.astype(np.float32).astype(np.float64)
    P64, S = B @ A.T, np.abs(B) @ np.abs(A).T
    r_ref = float(np.max(np.abs(_chain32(A, B) - P64) / (U * S)))
    try:
        t32 = torch.empty((L, M), dtype=torch.float32, device="cuda")
        pkg.updateYHat_(p, Yt, out=t32)
        assert p.YHat is t32
        r = float(np.max(np.abs(t32.double().cpu().numpy() - P64) / (U * S)))
        print(f"updateYHat_(out=t32): r_ref {r_ref:.3f}  yhat_f32 {r:.3f}")
        assert r <= 2 * r_ref
        pkg.updateYHat_(p, Yt, dtype=torch.bfloat16)
        assert p.YHat.is_cuda and p.YHat.dtype == torch.bfloat16 and tuple(p.YHat.shape) == (L, M)
        assert torch.equal(_bits(p.YHat), _bits(t32.to(torch.bfloat16)))
        pkg.updateYHat_(p, Yt, dtype=np.float32, residual=True)
        assert p.YHat.is_cuda and p.YHat.dtype == torch.float32
        R64 = Y64 - P64
        rr = float(np.max((np.abs(p.YHat.double().cpu().numpy() - R64) - U * np.abs(R64)) / (U * S)))
        assert rr <= 2 * r_ref
        pkg.updateYHat_(p, Y64, dtype=np.float32)                        # a host Y: a host result
        assert isinstance(p.YHat, np.ndarray) and p.YHat.dtype == np.float32
        assert np.array_equal(p.YHat.view(np.int32), t32.cpu().numpy().view(np.int32))
        pkg.updateYHat_(p, Yt)                                           # without the new arguments: the fp64 host array, as before
        s = pkg._session_for(Yt, H)
        assert isinstance(p.YHat, np.ndarray) and p.YHat.dtype == np.float64
        assert np.array_equal(p.YHat.view(np.int64), s.ctx.YHat().view(np.int64))
        assert np.all(np.abs(p.YHat - P64) <= 2.0 * H * 2.0 ** -53 * S)
        At, Bt = s.factors(device=True)
        q = pkg.vbmf_init(Y64, H, rng=np.random.default_rng(23))
        s.pull(q)
        assert At.is_cuda and At.dtype == torch.float32 and Bt.is_cuda
        assert np.array_equal(At.cpu().numpy().view(np.int32), q.AHat.astype(np.float32).view(np.int32))
        assert np.array_equal(Bt.cpu().numpy().view(np.int32), q.BHat.astype(np.float32).view(np.int32))
        blk = torch.empty((50, M), dtype=torch.float32, device="cuda")
        s.yhat_rows(blk, 100)
        assert torch.equal(_bits(blk), _bits(t32[100:150]))
        h64 = s.yhat()
        assert isinstance(h64, np.ndarray) and h64.dtype == np.float64 and np.all(np.abs(h64 - P64) <= 2.0 * H * 2.0 ** -53 * S)
    finally:
        pkg.invalidate()
