"""The two streaming passes (csrc/stream_gemm.hpp) against fp64, entry by entry, in every variant the planner can choose.

Pass 1 forms P = Y'B (split-K slabs, row or fragment-major layout), pass 2 forms Q = Y A (slabs folded into slab 0, the
stream-K pieces fixed up, or no Q at all when the register epilogue writes B directly).  Each case forces the streaming sweep
(VBMF_GRAM=0), sets Y and the state, runs c.step(STEP_A) and c.step(STEP_B) (or one sweep of c.run), reads the buffers back
(vbmf_debug_peek) and asserts through dims() that it reached the variant it names.

(a) Exact products.  Y in {-1, 0, 1} with at most 2^13 non-zeros on any contracted line, factor entries a + b 2^-9 with
    a, b in {-1, 0, 1}.  Those are exact in bf16 hi + lo, in single bf16 after rounding (and B32 / A32 are read back as the
    operand the MFMA saw: write_factor_tiles), and every partial sum is a multiple of 2^-9 below 2^14: exact in fp32.  So
    sum_slabs P == Ys' B32 and Q == Ys A32 BITWISE, padding (rows >= M or L, columns >= H) exactly zero.
(b) Real data: |P - Ys'F| <= gamma (|Ys|'|F|) per entry, gamma from the accumulation structure (pass_bound).
(c) The consumers: A = tile(fp32(P SA32)) and B = tile(fp32(Q SB32)) per entry (post_bound), the operand tiles decode to
    A32 / B32 bitwise with zero padding, and the state's A'A, B'B, dB'dB, tr(B'YA) against fp64 recomputations (gram_bound).
(d) Pass 1 of c.step and of the first sweep of c.run on the same state are bitwise equal (deterministic plain stores; only
    the block offset of the two control workgroups differs)."""
import numpy as np
import pytest

import __graft_entry__ as G
from oracle import vbmf_oracle as O
from tests.helpers import frag_to_rows, report

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
PIPE_D = 12                    # zero k-steps behind the factor tiles (common.hpp)
# |tile(f) - f| <= TILE_R |f|: the value the operand tiles encode (write_factor_tiles): fp32 as is; one bf16 rounding (8
# significant bits); bf16 hi + bf16 lo of the remainder (the remainder is exact in fp32, lo rounds it to 8 bits: 2^-8 2^-8)
TILE_R = {"f32": 0.0, "bf16": 2.0 ** -8, "bf16x2": 2.0 ** -16}


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


def _dtypes(pkg, mode):
    return {"f32": (pkg.VBMF_Y_F32, pkg.VBMF_FACTOR_AUTO), "bf16": (pkg.VBMF_Y_BF16, pkg.VBMF_FACTOR_BF16),
            "bf16x2": (pkg.VBMF_Y_BF16, pkg.VBMF_FACTOR_BF16X2)}[mode]


# ---- data ------------------------------------------------------------------------------------------------------------------
def _exact_Y(L, M, seed):
    rng = np.random.default_rng(seed)
    dens = min(0.5, 4096.0 / max(L, M))
    Y = rng.integers(-1, 2, size=(L, M)).astype(np.float64) * (rng.random((L, M)) < dens)
    assert max(np.count_nonzero(Y, axis=0).max(), np.count_nonzero(Y, axis=1).max()) <= 2 ** 13
    return Y


def _exact_F(n, H, rng):
    return rng.integers(-1, 2, size=(n, H)) + rng.integers(-1, 2, size=(n, H)) * 2.0 ** -9


def _real_Y(L, M, H, seed):
    rng = np.random.default_rng(seed)
    _, A, B = O.toy_matrix(L, M, H, 0.05, rng)
    return (B * np.linspace(1.0, 3.0, H)) @ A.T + 0.05 * rng.standard_normal((L, M))


def _state(L, M, H, seed, exact):
    rng = np.random.default_rng(seed)
    if exact:
        A, B = _exact_F(M, H, rng), _exact_F(L, H, rng)
    else:
        A, B = rng.standard_normal((M, H)), rng.standard_normal((L, H))
    R = rng.standard_normal((H, H)) / np.sqrt(H)
    SA = 0.01 * (R @ R.T + np.eye(H))
    R = rng.standard_normal((H, H)) / np.sqrt(H)
    SB = 0.01 * (R @ R.T + np.eye(H))
    return A, B, SA, SB, np.full(H, 0.7), np.full(H, 1.3), 0.5


# ---- device buffers --------------------------------------------------------------------------------------------------------
def _f32(c, cap, what, n):
    return c.peek(what, n, dtype=np.float32).astype(np.float64)


def _product(c, cap, which, d, nslab=None):
    """The slabs of pass 1 (which = 0) or pass 2 (1) as a list of fp64 [X32][Hp] matrices, decoded from the layout dims() names."""
    Hp = d["Hp"]
    X = 32 * (d["XT1"] if which == 0 else d["XT2"])
    ns = nslab if nslab is not None else d["nsplit1" if which == 0 else "nsplit2"]
    raw = _f32(c, cap, cap.PEEK_P if which == 0 else cap.PEEK_Q, ns * Hp * X)
    frag = d["p_frag" if which == 0 else "q_frag"]
    out = []
    for s in range(ns):
        sl = raw[s * Hp * X:(s + 1) * Hp * X]
        out.append(frag_to_rows(sl, X, Hp) if frag else sl.reshape(Hp, X).T.copy())
    return out


def decode_tiles(raw_u32, mode, NH, npart):
    """The factor's MFMA operand tiles (write_factor_tiles: k-step ks of 16 rows (8 in the fp32 mode), [part][h tile][lane
    (half, c)][8 bf16 | 4 fp32]) -> the fp32 factor they encode, row-major [KS kstep][32 NH]."""
    if mode == "f32":
        V = raw_u32.view(np.float32).astype(np.float64).reshape(-1, NH, 2, 32, 4)         # ks, h tile, half, c, e: row 8 ks + 4 half + e
        return V.transpose(0, 2, 4, 1, 3).reshape(-1, NH * 32)
    u16 = raw_u32.view(np.uint16).astype(np.uint32)
    vals = (u16 << 16).view(np.float32).astype(np.float64).reshape(-1, npart, NH, 2, 32, 2, 4)   # ks, part, h, half, c, e>>2, e&3
    V = vals.sum(axis=1)                                                   # hi + lo: exact (the tiles encode exactly that)
    return V.transpose(0, 4, 2, 5, 1, 3).reshape(-1, NH * 32)              # row 16 ks + 8 (e>>2) + 4 half + (e&3)


def _state_block(c, cap, Hp):
    n2 = Hp * Hp
    st = c.peek(cap.PEEK_STATE, 2 * (3 * n2 + 1), dtype=np.float64)
    return st[:n2].reshape(Hp, Hp), st[n2:2 * n2].reshape(Hp, Hp), st[2 * n2:3 * n2].reshape(Hp, Hp), float(st[3 * n2])


def _session(pkg, monkeypatch, L, M, H, mode, Y, state, env=None, splits=0, what="step"):
    """One context: set Y and the state, then the update(s) `what` ("step": STEP_A, then STEP_B from the set state again; "chain":
    STEP_A, then STEP_B on the A it left; "A": STEP_A only; "run": run(1)); every buffer the checks need, read back."""
    cap = pkg.capi
    env = dict({"VBMF_GRAM": "0"}, **(env or {}))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ydt, fdt = _dtypes(pkg, mode)
    c = cap.Context(L, M, H, y_dtype=ydt, factor_dtype=fdt, pass1_splits=splits)
    for k in env:
        monkeypatch.delenv(k)
    r = {}
    with c:
        c.set_Y(Y)
        c.set_state(*state)
        d = c.dims()
        Hp, NH, Mp, Lp = d["Hp"], d["NH"], 32 * d["XT1"], 32 * d["XT2"]
        r.update(Hp=Hp, NH=NH, Mp=Mp, Lp=Lp, Ys=c.get_Y())
        r["A0"] = _f32(c, cap, cap.PEEK_A32, Mp * Hp).reshape(Mp, Hp)
        r["B0"] = _f32(c, cap, cap.PEEK_B32, Lp * Hp).reshape(Lp, Hp)
        npart = d["npart"]
        nFA = (d["KS2"] + PIPE_D) * npart * NH * 64 * 4
        nFB = (d["KS1"] + PIPE_D) * npart * NH * 64 * 4
        if what == "run":
            c.run(1, eps=0.0, est_covs=False, est_var=False)
        else:
            c.step(cap.STEP_A)
        d = c.dims()
        r["dA"] = d
        r["P"] = _product(c, cap, 0, d)
        r["A1"] = _f32(c, cap, cap.PEEK_A32, Mp * Hp).reshape(Mp, Hp)
        r["SA32"] = _f32(c, cap, cap.PEEK_SA32, Hp * Hp).reshape(Hp, Hp)
        r["FA"] = decode_tiles(c.peek(cap.PEEK_FA, nFA), mode, NH, npart)
        if what == "step":
            r["GA"] = _state_block(c, cap, Hp)[0]
            # STEP_B from the set state again: Q = Ys A0 with the exactly representable A0 (Ys A1 has no exact fp32 sums)
            c.set_state(*state)
            c.step(cap.STEP_B)
            d = c.dims()
        if what == "chain":
            r["GA"] = _state_block(c, cap, Hp)[0]
            c.step(cap.STEP_B)
            d = c.dims()
        if what in ("step", "chain", "run"):
            r["dB"] = d
            r["Q"] = None if d["q_epi"] else _product(c, cap, 1, d, nslab=1)[0]      # split: folded into slab 0
            r["B1"] = _f32(c, cap, cap.PEEK_B32, Lp * Hp).reshape(Lp, Hp)
            r["SB32"] = _f32(c, cap, cap.PEEK_SB32, Hp * Hp).reshape(Hp, Hp)
            r["FB"] = decode_tiles(c.peek(cap.PEEK_FB, nFB), mode, NH, npart)
            if what == "step":
                _, r["GB"], r["GD"], r["GX"] = _state_block(c, cap, Hp)
    return r


# ---- bounds ----------------------------------------------------------------------------------------------------------------
def _mfma_per_kstep(mode):
    """(MFMAs into one accumulator per k-step, fp32 roundings each).  fp32: 8 rows = four 32x32x2 MFMAs, whose products are
    rounded too (3: product, internal sum, accumulation); bf16 modes: one 32x32x16 MFMA per factor part, exact products
    (2: internal sum, accumulation).  The LDS-DMA kernel's 16x16x32 MFMA covers two k-steps per part: fewer roundings."""
    return {"f32": (4, 3), "bf16": (1, 2), "bf16x2": (2, 2)}[mode]


def pass_bound(mode, sps, nslab):
    """Real-data product: an accumulator sums one split's sps k-steps (m MFMAs of rho roundings each per k-step, each rounding
    at most u of the running |Y|'|F| share), then the nslab - 1 slab additions (fold / fix-up / slab sum) and one for luck:
    |P - Ys'F| <= (rho m sps + nslab + 1) u (|Ys|'|F|)."""
    m, rho = _mfma_per_kstep(mode)
    return (rho * m * sps + nslab + 1) * U


def post_bound(mode, Hp):
    """A = tile(fp32(P S)): the contraction over Hp runs either as exact-f32 MFMAs (Hp / 2 of them, 3 roundings each) or as
    the six-term bf16 product (dropped terms below 2 u, 6 Hp / 16 MFMAs of 2 roundings each); the larger, (1.5 Hp + 1) u,
    bounds both.  The tile rounding adds TILE_R |f| <= TILE_R (1 + gamma) |P||S|."""
    g = (1.5 * Hp + 1) * U
    return g + TILE_R[mode] * (1.0 + g)


def gram_tiles(r, side):
    """32-row tiles one fp32 Gram accumulator sums at most before the fp64 slab reduction (the host's chunking): NH <= 2, four
    waves of at most max(8, ceil(XT / 1024)) tiles folded in LDS (post_gram2, register epilogue); NH >= 4, a whole chunk
    (gram_tiles_per_chunk, or the context-wide tiles_per_chunk of the fp32 mode's gram_kernel)."""
    d = r["dA"]
    XT = d["XT1"] if side == 0 else d["XT2"]
    if r["NH"] <= 2:
        return 4 * max(8, _cdiv(XT, 1024))
    if XT >= 2048:
        return max(16, _cdiv(_cdiv(max(r["Lp"], r["Mp"]), 32), 384)) if d["mode"] == 0 else max(8, _cdiv(XT, 250))   # (mode 0: fp32)
    return max(4, _cdiv(XT, 96))


def _cdiv(a, b):
    return -(-a // b)


def gram_bound(r, side):
    """Each row adds at most 4 part products (hi/lo x hi/lo) plus one product rounding to an fp32 accumulator, 32 rows per tile:
    worst-case recursive summation over T tiles, then the fp64 reduction (one u for the fp32 slab store, margin):
    |G - F'F| <= (160 T + 8) u (|F|'|F|)."""
    return (160 * gram_tiles(r, side) + 8) * U


# ---- checks ----------------------------------------------------------------------------------------------------------------
def _check_exact_products(tag, r, H):
    Ys, L, M = r["Ys"], r["Ys"].shape[0], r["Ys"].shape[1]
    Mp, Lp, Hp = r["Mp"], r["Lp"], r["Hp"]
    B0 = r["B0"]
    assert not np.any(B0[L:]) and not np.any(B0[:, H:])
    ref = np.zeros((Mp, Hp))
    ref[:M] = Ys.T @ B0[:L]
    assert np.abs(ref).max() < 2 ** 14
    for s, sl in enumerate(r["P"]):
        assert not np.any(sl[M:]) and not np.any(sl[:, H:]), (tag, "P padding", s)
    Psum = np.sum(r["P"], axis=0)
    bad = np.argwhere(Psum != ref)
    assert bad.size == 0, (tag, f"{len(bad)} entries of sum_slabs P differ from Ys'B32", bad[:8].tolist())
    if r.get("Q") is not None:
        A = r["A0"]                                                   # the A pass 2 multiplied by (STEP_B from the set state)
        refQ = np.zeros((Lp, Hp))
        refQ[:L] = Ys @ A[:M]
        badQ = np.argwhere(r["Q"] != refQ)
        assert badQ.size == 0, (tag, f"{len(badQ)} entries of Q differ from Ys A32", badQ[:8].tolist())
        assert not np.any(r["Q"][L:]) and not np.any(r["Q"][:, H:]), (tag, "Q padding")
    return ref


def _check_factor(tag, Fnew, X, prod, S, mode, Hp, H, prod_scale=None, g_prod=0.0):
    """Fnew = tile(fp32(prod S)) per entry.  prod is the fp64 product; when the device's product is exact, the bound is the
    post kernel's own; otherwise the device's product is within g_prod prod_scale of it, which the table carries along:
    |Fnew - prod S| <= (g_prod + post_bound (1 + g_prod)) (prod_scale |S|)."""
    ref = prod @ S
    scale = (np.abs(prod) if prod_scale is None else prod_scale) @ np.abs(S)
    g = g_prod + post_bound(mode, Hp) * (1.0 + g_prod)
    err = np.abs(Fnew - ref)
    worst = float(np.max(err / np.maximum(scale, 1e-300)))
    assert np.all(err <= g * scale), (tag, worst, g)
    assert not np.any(Fnew[X:]) and not np.any(Fnew[:, H:]), (tag, "factor padding")
    return worst


def _check_tiles(tag, Fdec, F32, rows):
    n = min(len(Fdec), len(F32))
    assert len(Fdec) >= rows
    assert np.array_equal(Fdec[:n], F32[:n]), (tag, "operand tiles differ from the fp32 factor")
    assert not np.any(Fdec[rows:]) and not np.any(F32[rows:]), (tag, "tile padding")


def _check_gram(tag, G, F, bound, H):
    Fh = F[:, :H]
    ref, scale = Fh.T @ Fh, np.abs(Fh).T @ np.abs(Fh)
    err = np.abs(G[:H, :H] - ref)
    worst = float(np.max(err / np.maximum(scale, 1e-300)))
    assert np.all(err <= bound * scale), (tag, worst, bound)
    assert not np.any(G[H:]) and not np.any(G[:, H:]), (tag, "Gram padding")
    return worst


def _expect(tag, d, exp):
    got = {k: d[k] for k in exp}
    for k, v in exp.items():
        if callable(v):
            assert v(d[k]), (tag, k, d[k])
        else:
            assert d[k] == v, (tag, k, d[k], v)
    return got


# (id, L, M, H, mode, env, pass1_splits, expected dims after STEP_A, expected dims after STEP_B)
# L, M = 1 mod 32 (and 1 mod the ring depths 3 / 6 / 12 and the x groups of 128 / 256 / 512 / 1024 rows); H = 1 mod 32 or 32 n - 1.
GT1 = lambda v: v > 1
LONG = lambda v: v >= 2048                     # the side's 32-row tiles: launch_post_frag's NXT > 1, the long-side Gram chunks
CASES = [
    # NH = 1 / 2, wide geometry, un-split pass 2: the register epilogue (no Q stored)
    ("f32-nh1-wide-epi", 150001, 33, 1, "f32", {"VBMF_NARROW": "0"}, 0, dict(NH=1, narrow=0, p_frag=1), dict(q_epi=1, nsplit2=1)),
    ("bf16-nh1-wide-epi", 60001, 97, 31, "bf16", {"VBMF_NARROW": "0"}, 0, dict(NH=1, narrow=0, p_frag=1), dict(q_epi=1)),
    ("bf16x2-nh1-wide-epi", 60001, 97, 31, "bf16x2", {"VBMF_NARROW": "0"}, 0, dict(NH=1, narrow=0, p_frag=1), dict(q_epi=1)),
    ("f32-nh2-wide-epi", 4097, 97, 64, "f32", {"VBMF_NARROW": "0"}, 0, dict(NH=2, narrow=0, nsplit1=GT1), dict(q_epi=1)),
    ("bf16-nh2-wide-epi", 4097, 97, 33, "bf16", {"VBMF_NARROW": "0"}, 0, dict(NH=2, narrow=0, nsplit1=GT1), dict(q_epi=1)),
    ("bf16x2-nh2-wide-epi", 4097, 97, 64, "bf16x2", {"VBMF_NARROW": "0"}, 0, dict(NH=2, narrow=0, nsplit1=GT1), dict(q_epi=1)),
    # NH = 1 / 2, wide geometry, split pass 2 (fragment-major slabs, folded)
    ("bf16x2-nh1-wide-split2", 4097, 97, 31, "bf16x2", {"VBMF_NARROW": "0"}, 0, dict(NH=1, narrow=0), dict(q_epi=0, q_frag=1, nsplit2=GT1)),
    ("f32-nh1-wide-split2-long", 201, 20001, 1, "f32", {"VBMF_NARROW": "0"}, 0, dict(NH=1, narrow=0), dict(q_epi=0, q_frag=1, nsplit2=GT1)),
    ("bf16x2-nh2-wide-split2-long", 201, 20001, 63, "bf16x2", {"VBMF_NARROW": "0"}, 0, dict(NH=2, narrow=0), dict(q_epi=0, q_frag=1, nsplit2=GT1)),
    # NH = 1 / 2, narrow geometry
    ("f32-nh1-narrow", 1057, 385, 1, "f32", {"VBMF_NARROW": "1"}, 0, dict(NH=1, narrow=1), dict(q_epi=0, q_frag=1)),
    ("bf16-nh1-narrow", 1057, 385, 31, "bf16", {"VBMF_NARROW": "1"}, 0, dict(NH=1, narrow=1), dict(q_epi=0, q_frag=1)),
    ("bf16x2-nh1-narrow", 1057, 385, 31, "bf16x2", {"VBMF_NARROW": "1"}, 0, dict(NH=1, narrow=1), dict(q_epi=0, q_frag=1)),
    ("f32-nh2-narrow", 1057, 385, 64, "f32", {"VBMF_NARROW": "1"}, 0, dict(NH=2, narrow=1), dict(q_epi=0, q_frag=1)),
    ("bf16-nh2-narrow", 1057, 385, 33, "bf16", {"VBMF_NARROW": "1"}, 0, dict(NH=2, narrow=1), dict(q_epi=0, q_frag=1)),
    ("bf16x2-nh2-narrow", 1057, 385, 64, "bf16x2", {"VBMF_NARROW": "1"}, 0, dict(NH=2, narrow=1), dict(q_epi=0, q_frag=1)),
    # NH = 4 / 8, per-wave kernel: fp32 (row-major products, post_kernel; un-split pass 2: post_frag_kernel), single bf16
    ("f32-nh4-h65", 2049, 161, 65, "f32", {}, 0, dict(NH=4, lds8=0, p_frag=0), dict(q_frag=0, nsplit2=GT1)),
    ("f32-nh4-h96", 2049, 161, 96, "f32", {}, 0, dict(NH=4, Hp=128, lds8=0, p_frag=0), dict(q_frag=0)),
    ("f32-nh4-h65-unsplit2", 20001, 161, 65, "f32", {}, 0, dict(NH=4, lds8=0, p_frag=0), dict(q_frag=1, nsplit2=1)),
    ("f32-nh8-h129", 2049, 161, 129, "f32", {}, 0, dict(NH=8, lds8=0, p_frag=0), dict(q_frag=0)),
    ("f32-nh8-h256", 2049, 161, 256, "f32", {}, 0, dict(NH=8, lds8=0, p_frag=0), dict(q_frag=0)),
    ("bf16-nh4-h100", 2049, 161, 100, "bf16", {}, 0, dict(NH=4, lds8=0, p_frag=1, post3=1), dict(q_frag=0)),
    # NH = 4 / 8 bf16x2: the LDS-DMA kernel (default), the per-wave kernel (VBMF_LDS8=0), post_frag2 (VBMF_POST3=0)
    ("bf16x2-nh4-lds8", 2049, 161, 128, "bf16x2", {}, 0, dict(NH=4, lds8=1, p_frag=1, post3=1), dict(q_frag=0)),
    ("bf16x2-nh8-lds8", 2049, 161, 129, "bf16x2", {}, 0, dict(NH=8, lds8=1, p_frag=1, post3=1), dict(q_frag=0)),
    ("bf16x2-nh4-wave", 2049, 161, 128, "bf16x2", {"VBMF_LDS8": "0"}, 0, dict(NH=4, lds8=0, p_frag=1), dict(q_frag=0)),
    ("bf16x2-nh8-wave", 2049, 161, 256, "bf16x2", {"VBMF_LDS8": "0"}, 0, dict(NH=8, lds8=0, p_frag=1), dict(q_frag=0)),
    ("bf16x2-nh8-lds8-post2", 257, 6145, 256, "bf16x2", {"VBMF_POST3": "0"}, 0, dict(NH=8, lds8=1, post3=0, nsplit1=1), dict(nsplit2=GT1)),
    ("bf16x2-nh4-lds8-unsplit2", 20001, 161, 128, "bf16x2", {}, 0, dict(NH=4, lds8=1), dict(q_frag=1, nsplit2=1)),
    ("bf16x2-nh4-lds8-unsplit2-post2", 20001, 161, 128, "bf16x2", {"VBMF_POST3": "0"}, 0, dict(NH=4, lds8=1, post3=0), dict(q_frag=1, nsplit2=1)),
    # split-K pass 1 at forced split counts that do not divide the contracted length; XCD map on / off
    ("bf16x2-split1x2", 3001, 225, 33, "bf16x2", {}, 2, dict(nsplit1=2, xcd_map=1), dict()),
    ("bf16x2-split1x3-noxcd", 3001, 225, 33, "bf16x2", {"VBMF_XCD_MAP": "0"}, 3, dict(nsplit1=3, xcd_map=0), dict()),
    ("f32-split1x5", 3001, 225, 65, "f32", {}, 5, dict(nsplit1=5, xcd_map=1), dict()),
    ("bf16x2-nh8-split1x5-noxcd", 3001, 225, 129, "bf16x2", {"VBMF_XCD_MAP": "0"}, 5, dict(nsplit1=5, xcd_map=0, lds8=1), dict()),
    # stream-K pieces and fix-up of the un-split Y*A pass (the shape of test_gpu_parity.py's stream-K test)
    ("bf16x2-streamk", 66001, 400, 140, "bf16x2", {"VBMF_STREAMK": "1"}, 0, dict(NH=8, lds8=1, streamk_per=GT1), dict(q_frag=1, nsplit2=1)),
    # a long A side (M >= 65 536: 2051 tiles hold rows, XT1 = 2052 >= 2048 after rounding to the wave's tile count): the NXT > 1
    # A-side instantiations of post_frag3 / post_frag2 (the AHEAD tails with BSIDE = false), the long-side Gram chunking of the A
    # side, with a last wave and a last workgroup that are not full
    ("bf16x2-nh4-longA-post3", 97, 65601, 128, "bf16x2", {}, 0, dict(NH=4, p_frag=1, post3=1, XT1=LONG), dict()),
    ("bf16x2-nh4-longA-post2", 97, 65601, 128, "bf16x2", {"VBMF_POST3": "0"}, 0, dict(NH=4, p_frag=1, post3=0, XT1=LONG), dict()),
    ("bf16x2-nh8-longA-post2", 97, 65601, 129, "bf16x2", {"VBMF_POST3": "0"}, 0, dict(NH=8, p_frag=1, post3=0, XT1=LONG), dict()),
    ("bf16-nh4-longA", 97, 65601, 100, "bf16", {}, 0, dict(NH=4, p_frag=1, XT1=LONG), dict()),
    ("bf16x2-nh2-longA", 97, 65601, 33, "bf16x2", {"VBMF_NARROW": "0"}, 0, dict(NH=2, XT1=LONG), dict()),
    ("f32-nh4-longA", 97, 65601, 65, "f32", {}, 0, dict(NH=4, p_frag=0, XT1=LONG), dict()),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_exact_products_and_consumers(pkg, monkeypatch, case):
    tag, L, M, H, mode, env, splits, expA, expB = case
    Y = _exact_Y(L, M, 7000 + L + M + H)
    st = _state(L, M, H, 7100 + H, exact=True)
    r = _session(pkg, monkeypatch, L, M, H, mode, Y, st, env, splits)
    _expect(tag, r["dA"], expA)
    _expect(tag, r["dB"], expB)
    if splits:
        d = r["dA"]
        n = d["sps1"] * d["kstep"]                                        # rows per split
        assert (d["nsplit1"] - 1) * n < L < d["nsplit1"] * n, (tag, "the last split holds real rows and is partial", L, n)
    assert np.array_equal(r["Ys"], Y)                                    # ternary data is exact in bf16
    Hp = r["Hp"]
    # (a) products
    P = _check_exact_products(tag, r, H)
    # (c) consumers: A from P, B from Q = Ys A (exact, stored or not)
    wA = _check_factor(tag + " A", r["A1"], M, P, r["SA32"], mode, Hp, H)
    Qx = np.zeros((r["Lp"], Hp))
    Qx[:L] = r["Ys"] @ r["A0"][:M]                                   # exact: the product pass 2 formed (stored or not)
    wB = _check_factor(tag + " B", r["B1"], L, Qx, r["SB32"], mode, Hp, H)
    _check_tiles(tag + " FA", r["FA"], r["A1"], M)
    _check_tiles(tag + " FB", r["FB"], r["B1"], L)
    # state: A'A, B'B, dB'dB, tr(B'YA)
    wGA = _check_gram(tag + " A'A", r["GA"], r["A1"][:M], gram_bound(r, 0), H)
    wGB = _check_gram(tag + " B'B", r["GB"], r["B1"][:L], gram_bound(r, 1), H)
    Dm = r["B0"][:L] - r["B1"][:L]
    # the delta is formed in fp32 (one rounding) and, at NH >= 4 in the bf16 modes, re-split into bf16 hi + lo (2^-16):
    # each factor of a product is off by at most 2^-16 + u, so the product by 2 (2^-16 + u) + its square < 2^-14
    wGD = _check_gram(tag + " dB'dB", r["GD"], Dm, gram_bound(r, 1) + 2.0 ** -14, H)
    tr = float(np.sum(Qx[:L, :H] * r["B1"][:L, :H]))                 # (B1 = what the tiles encode: the value the trace uses)
    trs = float(np.sum(np.abs(Qx[:L, :H] * r["B1"][:L, :H])))
    # per lane a 16-term fp32 fma chain per 32 x 32 block (tile_dot_qb), then fp64: |tr - tr64| <= 18 u sum |Q o B|
    assert abs(r["GX"] - tr) <= 18 * U * trs, (tag, "tr(B'YA)", r["GX"], tr, trs)
    report(f"stream passes exact {tag}: A_entry={wA:.2e} B_entry={wB:.2e} AA={wGA:.2e} BB={wGB:.2e} dBdB={wGD:.2e}"
           f" tr={abs(r['GX'] - tr) / max(trs, 1e-300):.2e}")


# real-valued data: (id, L, M, H, mode, env, splits, expected dims after STEP_A, after STEP_B)
REAL = [
    ("f32-nh1-wide-split2", 4097, 97, 1, "f32", {"VBMF_NARROW": "0"}, 0, dict(NH=1), dict(q_frag=1)),
    ("bf16x2-nh2-narrow", 1057, 385, 64, "bf16x2", {"VBMF_NARROW": "1"}, 0, dict(NH=2, narrow=1), dict(q_frag=1)),
    ("bf16-nh2-wide-split2-long", 201, 20001, 33, "bf16", {"VBMF_NARROW": "0"}, 0, dict(NH=2), dict(nsplit2=GT1)),
    ("f32-nh8-h256", 2049, 161, 256, "f32", {}, 0, dict(NH=8, p_frag=0), dict(q_frag=0)),
    ("bf16x2-nh4-lds8-split1x3", 3001, 225, 128, "bf16x2", {}, 3, dict(NH=4, lds8=1, nsplit1=3), dict()),
    ("bf16x2-nh8-wave", 2049, 161, 256, "bf16x2", {"VBMF_LDS8": "0"}, 0, dict(NH=8, lds8=0), dict(q_frag=0)),
    ("bf16x2-streamk", 66001, 400, 140, "bf16x2", {"VBMF_STREAMK": "1"}, 0, dict(NH=8, streamk_per=GT1), dict(q_frag=1)),
]


@pytest.mark.parametrize("case", REAL, ids=[c[0] for c in REAL])
def test_real_data_products_against_fp64(pkg, monkeypatch, case):
    tag, L, M, H, mode, env, splits, expA, expB = case
    Y = _real_Y(L, M, H, 7200 + L + H)
    st = _state(L, M, H, 7300 + H, exact=False)
    r = _session(pkg, monkeypatch, L, M, H, mode, Y, st, env, splits)
    dA, dB = r["dA"], r["dB"]
    _expect(tag, dA, expA)
    _expect(tag, dB, expB)
    Ys = r["Ys"]
    aY = np.abs(Ys)
    # pass 1
    F = r["B0"][:L]
    P = np.sum(r["P"], axis=0)[:M]
    g1 = pass_bound(mode, dA["sps1"], dA["nsplit1"])
    ref, scale = Ys.T @ F, aY.T @ np.abs(F)
    w1 = float(np.max(np.abs(P - ref) / np.maximum(scale, 1e-300)))
    assert np.all(np.abs(P - ref) <= g1 * scale), (tag, "P", w1, g1)
    for sl in r["P"]:
        assert not np.any(sl[M:]) and not np.any(sl[:, H:]), (tag, "P padding")
    fro1 = float(np.linalg.norm(P - ref) / np.linalg.norm(ref))
    # pass 2 (slab 0 after the fold / the fix-up)
    w2 = fro2 = 0.0
    if r["Q"] is not None:
        A = r["A0"][:M]                                                # STEP_B ran from the set state
        nsl = max(dB["nsplit2"], dB["streamk_per"])
        g2 = pass_bound(mode, dB["sps2"], nsl)
        ref2, scale2 = Ys @ A, aY @ np.abs(A)
        Q = r["Q"][:L]
        w2 = float(np.max(np.abs(Q - ref2) / np.maximum(scale2, 1e-300)))
        assert np.all(np.abs(Q - ref2) <= g2 * scale2), (tag, "Q", w2, g2)
        assert not np.any(r["Q"][L:]) and not np.any(r["Q"][:, H:]), (tag, "Q padding")
        fro2 = float(np.linalg.norm(Q - ref2) / np.linalg.norm(ref2))
    report(f"stream passes real {tag}: P_entry={w1:.2e} P_fro={fro1:.2e} Q_entry={w2:.2e} Q_fro={fro2:.2e}"
           f"  [sps {dA['sps1']}/{dB['sps2']}, nsplit {dA['nsplit1']}/{dB['nsplit2']}]")


# step versus run: (id, L, M, H, mode, env, splits, expected dims of the run)
STEP_RUN = [
    ("f32-nh1-wide-epi", 150001, 33, 1, "f32", {"VBMF_NARROW": "0"}, 0, dict(NH=1, q_epi=1)),
    ("bf16x2-nh2-wide-epi", 4097, 97, 64, "bf16x2", {"VBMF_NARROW": "0"}, 0, dict(NH=2, q_epi=1)),
    ("bf16-nh1-narrow", 1057, 385, 31, "bf16", {"VBMF_NARROW": "1"}, 0, dict(NH=1, narrow=1, q_epi=0)),
    ("bf16x2-narrow-split1x3-noxcd", 3001, 225, 33, "bf16x2", {"VBMF_XCD_MAP": "0"}, 3, dict(nsplit1=3, xcd_map=0, narrow=1, q_epi=0)),
    ("f32-nh4-h65", 2049, 161, 65, "f32", {}, 0, dict(NH=4)),
    ("bf16x2-nh4-lds8-split1x3", 3001, 225, 128, "bf16x2", {}, 3, dict(NH=4, lds8=1, nsplit1=3)),
    ("bf16x2-nh8-lds8", 2049, 161, 129, "bf16x2", {}, 0, dict(NH=8, lds8=1)),
]


@pytest.mark.parametrize("case", STEP_RUN, ids=[c[0] for c in STEP_RUN])
def test_step_and_run_pass1_bitwise(pkg, monkeypatch, case):
    """Pass 1 of c.step(STEP_A) and of the first sweep of c.run(1) on the same state are the same launch up to the two control
    workgroups in front (ctrl_mode; NH <= 4 only) -- plain stores of a fixed summation order: bitwise equal slabs.  The run's
    pass 2 (epilogue or stored Q) is checked on exact data: B = tile(fp32(Ys A SB32)) per entry, Q == Ys A32 bitwise."""
    tag, L, M, H, mode, env, splits, exp = case
    Y = _real_Y(L, M, H, 7400 + L + H)
    st = _state(L, M, H, 7500 + H, exact=False)
    a = _session(pkg, monkeypatch, L, M, H, mode, Y, st, env, splits, what="A")
    b = _session(pkg, monkeypatch, L, M, H, mode, Y, st, env, splits, what="run")
    _expect(tag, b["dB"], exp)
    assert len(a["P"]) == len(b["P"])
    for s, (x, y) in enumerate(zip(a["P"], b["P"])):
        assert np.array_equal(x, y), (tag, "slab", s, int(np.sum(x != y)))
    # the run's pass 2 on exact data
    Yx = _exact_Y(L, M, 7600 + L + H)
    stx = _state(L, M, H, 7700 + H, exact=True)
    r = _session(pkg, monkeypatch, L, M, H, mode, Yx, stx, env, splits, what="run")
    _expect(tag, r["dB"], exp)
    Q = r.pop("Q")
    _check_exact_products(tag + " run", r, H)                    # P from the set (exact) B
    # the sweep's A is real-valued: Ys A1 is not exact in fp32, so pass 2 gets the real-data bound
    Hp, dB = r["Hp"], r["dB"]
    A1 = r["A1"][:M]
    g2 = pass_bound(mode, dB["sps2"], max(dB["nsplit2"], dB["streamk_per"]))
    Qx = np.zeros((r["Lp"], Hp))
    Qx[:L] = r["Ys"] @ A1
    Qs = np.zeros((r["Lp"], Hp))
    Qs[:L] = np.abs(r["Ys"]) @ np.abs(A1)
    if Q is not None:
        assert np.all(np.abs(Q - Qx) <= g2 * Qs), (tag, "run Q", float(np.max(np.abs(Q - Qx) / np.maximum(Qs, 1e-300))), g2)
        assert not np.any(Q[L:]) and not np.any(Q[:, H:]), (tag, "run Q padding")
    _check_factor(tag + " run B", r["B1"], L, Qx, r["SB32"], mode, Hp, H, prod_scale=Qs, g_prod=g2)
    _check_tiles(tag + " run FB", r["FB"], r["B1"], L)
