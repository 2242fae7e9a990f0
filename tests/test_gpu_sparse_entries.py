"""The ARD-sparse updates (csrc/sparse_kernels.hpp and the kernels they share with the basic model) against fp64, entry by entry,
in every variant the dispatch of do_sparse_update_A / do_sparse_update_B / sparse_run_impl can reach.

Each case names its variant, creates a context of that variant (the env switch set around the constructor only), loads a
synthetic state whose arrays span the decades an ARD model reaches (tests/sparse_entry_reference.py: |A| and CA over more than
four decades -- a trajectory state at these edge shapes has collapsed to A ~ 1e-6 and tests nothing), runs ONE update at a time
through sparse_step, reads the device's buffers back (sparse_get_state, vbmf_debug_peek) and asserts through dims() that it
reached the kernel it names.  Every reference is formed in fp64 from what the device itself holds before the update, so each
bound is that ONE update's rounding; every entry (m, h), m < M, h < H, is compared, denominators floored at 1e-300 only.
u = 2^-24, e = 2^-53.

(1) updateA!, diagonal branch.  v[h] = sigmaHat (B'B)[h,h] + L SigmaB[h,h] (diag_var: sum_l (fp32(sigma_l) B32[l,h])^2 +
    L mean(sigma) SigmaB[h,h]); vi = QS1's `repeat(v, inner = M-1)` index or h; d = 1 / (v[vi] + fp32(CA)); a = sigmaHat d sum_s P_s
    (diag_var: a = d sum_s P_s).  One fp64 division and one fp32 rounding per entry:
        |dS - d| <= (u + 16 e) d,      |A - a| <= (u + TILE_R + (nsplit1 - 1) u + 16 e) sigmaHat d sum_s |P_s|
    (the slab sum's fp32 additions, the value the operand tiles encode; 16 e: fp64 contraction differences).  Masked entries are
    exactly 0 and no other entry is; rows >= M and columns >= H of A32 are exactly 0; the operand tiles decode to A32 bitwise.
    P itself against Ys' F, F = B32 (diag_var: fp32(sigma_l) B32, re-tiled: + TILE_R + u): pass_bound -- the only check on the
    row-scaled tiles.
(2) VBMF_SPARSE_A_FUSED = 1 and 0 (sparse_update_a_tiles_kernel; sparse_update_a_kernel + retile_kernel) leave A32 with its
    padding, diagSigmaATVec and the operand tiles bitwise equal.
(3) SigmaA = diag(sum_m dS32[m,h]) to M e, every other entry of the Hp x Hp block exactly 0; A'A by gram_bound.
(4) updateCA!: b = beta0 + (a^2 + ds)/2, ca = alpha / b from the device's A32, dS32: (u + 16 e) b and (2 u + 16 e) ca; the
    grouped models with each entry's own group's (alpha, beta0).
(5) updateB!: SigmaB against the fp64 inverse of diag(CB) + sigmaHat (GA + SA) of the device's own GA, SA (Frobenius 5e-5, the bound
    of tests/test_gpu_sparse.py: the inverse tiers have their own tests), SB32 = fp32(sigmaHat SigmaB) bitwise, then B per entry against
    Q SB32 (post_bound; diag_var: rows times fp32(sigma_l), one more u and one more TILE_R for the second tiling), the operand tiles,
    B'B, dB'dB, tr(B'YA) as in tests/test_gpu_stream_passes.py.
(6) updateCB! / updateSigma! (sparse_ctrl_end_kernel, 256 threads up to H = 64, 1024 above): delta, CB to 8 e;
    |zeta - ref| <= (H^2 + 16) e (zeta0 + trYY/2 + |tr(B'YA)| + sum |terms|/2); sigmaHat = eta / zeta to 8 e.
(7) diag_var rows (row_sumsq_kernel, hetero_g_kernel, hetero_sigma_kernel): zeta_l within
    (H + 2) u |B_l|'|G32||B_l|/2 + (M + 2 H + 16) e (sum of the terms' magnitudes), sigma_l = etaVec / zeta_l to 8 e, the mean to L e.
(8) One sweep of sparse_run equals the same sweep as sparse_step, bitwise (zeta and sigmaHat at NH = 8: to the bound of (6) -- the
    run sums t2 in sparse_t2_kernel's 64 shares); sparse_run_fixed_basis(2) equals two rounds of step(A), step(CA), step(SIGMA).

L = 257 throughout (two workgroups of hetero_sigma_kernel, the second with one row; nine row tiles: row_sumsq_kernel's last
workgroup is partial); the A-side kernels scale with M x H only.  M = 1057 is 1 mod 32 and gives colsum_part_kernel 34 rows per
chunk (one unrolled iteration plus a tail for every lane group, a last chunk of three rows); M = 33 leaves chunks empty."""
import numpy as np
import pytest

import __graft_entry__ as G
from tests import sparse_entry_reference as R
from tests.helpers import relF, report
from tests.test_gpu_stream_passes import (PIPE_D, TILE_R, U, _check_gram, _check_tiles, _dtypes, _expect, _f32, _product, _real_Y,
                                          decode_tiles, gram_bound, pass_bound, post_bound)

pytestmark = pytest.mark.gpu

E = R.E
L = 257
MODE_ID = {"f32": 0, "bf16": 1, "bf16x2": 2}
NH_OF = lambda H: 1 if H <= 32 else (2 if H <= 64 else (4 if H <= 128 else 8))
GROUP_PRIORS = ((0.3, 0.02), (0.9, 0.5), (1.7, 1e-3))          # (alpha0g, beta0g) of the grouped models' three groups
H0, M0 = 3, 40                                                   # both axes split off a tile edge (H = 33, M = 97)
# split count plan_pass picks for the Y'B pass at L = 257 (it depends on the contracted length, the mode's k-step and NH only at these
# widths; read from dims() on an MI355X): (NH 1, 2, 4, 8).  nsplit1 = 1 skips no kernel -- slab_sum_kernel then copies slab 0
AUTO_NSPLIT1 = {"f32": {1: 4, 2: 2, 4: 6, 8: 10}, "bf16": {1: 2, 2: 1, 4: 3, 8: 5}, "bf16x2": {1: 2, 2: 1, 4: 3, 8: 5}}
# the checks whose bound is a few fp64 roundings: their ratio moves in steps of one rounding of the HOST reference (a measured 0
# becomes 1e-3 where NumPy sums in another order), so they are reported in the bracketed tail of the line, which the measured
# baseline (tests/golden/make_parity_baseline.py) does not parse; the derived bound alone holds them
E_LEVEL = ("SA", "delta", "CB", "zeta", "sigma", "sigma_l", "mean")


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


def K(tag, M, H, mode, fused=1, compat=True, mask=None, diag_var=False, splits=0, group=None):
    return dict(tag=tag, M=M, H=H, mode=mode, fused=fused, compat=compat, mask=mask, diag_var=diag_var, splits=splits, group=group,
                nsplit1=splits if splits else AUTO_NSPLIT1[mode][NH_OF(H)])


def _labels(M):
    return sorted({0, M // 2, M - 1})


# ---- context, state, buffers ------------------------------------------------------------------------------------------------
def _context(pkg, monkeypatch, cs):
    cap = pkg.capi
    monkeypatch.setenv("VBMF_SPARSE_A_FUSED", str(cs["fused"]))
    ydt, fdt = _dtypes(pkg, cs["mode"])
    variant = {None: cap.VBMF_VARIANT_SPARSE_DIAG, "dual": cap.VBMF_VARIANT_DUAL_DIAG, "trial": cap.VBMF_VARIANT_TRIAL_DIAG}[cs["group"]]
    if cs["diag_var"]:
        variant = cap.VBMF_VARIANT_SPARSE_DIAGVAR
    rc = cap.VBMF_COMPAT_DEFAULT if cs["compat"] else (cap.VBMF_COMPAT_DEFAULT & ~cap.VBMF_COMPAT_SPARSE_REPEAT)
    try:
        return cap.Context(L, cs["M"], cs["H"], y_dtype=ydt, factor_dtype=fdt, variant=variant, reference_compat=rc,
                           pass1_splits=cs["splits"])
    finally:
        monkeypatch.delenv("VBMF_SPARSE_A_FUSED")


def _inputs(cs):
    M, H = cs["M"], cs["H"]
    Y = _real_Y(L, M, H, 8000 + M + H)
    st = R.synthetic_state(L, M, H, 8100 + M + H)
    noise = R.synthetic_noise_rows(L, M, 8200 + M) if cs["diag_var"] else None
    return Y, st, noise


def _load(c, cs, Y, st, noise):
    M, H = cs["M"], cs["H"]
    labels, H1 = cs["mask"] if cs["mask"] else ((), 0)
    c.set_Y(Y)
    c.sparse_set_state(st["ATVecHat"], st["diagSigmaATVec"], st["CA"], st["beta"], st["BHat"], st["SigmaB"], st["CB"], st["delta"],
                       st["sigmaHat"], st["zeta"], R.HYPER, labels0=labels, H1=H1)
    if cs["diag_var"]:
        c.sparse_set_noise_rows(*noise)
    (a0, b0), (a1, b1), (a2, b2) = GROUP_PRIORS
    if cs["group"] == "dual":
        c.dual_set_priors(H0, a0, b0, a1, b1)
    elif cs["group"] == "trial":
        c.trial_set_priors(H0, M0, dict(alpha01=a0, beta01=b0, alpha02=a1, beta02=b1, alpha03=a2, beta03=b2, alpha1=a0 + 0.5,
                                        alpha2=a1 + 0.5, alpha3=a2 + 0.5))


def _block(c, cap, Hp):
    """The device state block (ctrl_kernels.hpp, StateLayout): GA, GB, GD, tr(B'YA), SigmaA, SigmaB, the delta and CB strips, the scalars."""
    n2 = Hp * Hp
    st = c.peek(cap.PEEK_STATE, 2 * (9 * n2 + 8 + 2 * Hp + 32), dtype=np.float64)
    mat = lambda off: st[off:off + n2].reshape(Hp, Hp).copy()
    sc = st[9 * n2 + 8 + 2 * Hp:].copy()
    return dict(GA=mat(0), GB=mat(n2), GD=mat(2 * n2), GX=float(st[3 * n2]), SA=mat(3 * n2 + 8), SB=mat(4 * n2 + 8),
                delta=st[9 * n2 + 8:9 * n2 + 8 + Hp].copy(), CB=st[9 * n2 + 8 + Hp:9 * n2 + 8 + 2 * Hp].copy(), scal=sc,
                sig=float(sc[0]), trYY=float(sc[1]), trBQ=float(sc[11]), zeta=float(sc[12]))


def _tiles(c, cap, d, which, mode):
    """The operand tiles of A (which = 0: the factor of pass 2) or B (1: of pass 1), decoded."""
    n = (d["KS2" if which == 0 else "KS1"] + PIPE_D) * d["npart"] * d["NH"] * 64 * 4
    return decode_tiles(c.peek(cap.PEEK_FA if which == 0 else cap.PEEK_FB, n), mode, d["NH"], d["npart"])


def _worst(err, bound):
    """Largest error / bound over the entries (a zero bound admits a zero error only)."""
    r = np.where(err == 0.0, 0.0, err / np.maximum(bound, 1e-300))
    return float(np.max(r))


def _expect_variant(tag, cs, d):
    _expect(tag, d, dict(NH=NH_OF(cs["H"]), mode=MODE_ID[cs["mode"]], p_frag=0, sparse_a_fused=cs["fused"], nsplit1=cs["nsplit1"]))
    if cs["splits"]:
        n = d["sps1"] * d["kstep"]                                    # rows per split
        assert (d["nsplit1"] - 1) * n < L < d["nsplit1"] * n, (tag, "the last split holds real rows and is partial", n)


# ---- (1), (3): updateA! -----------------------------------------------------------------------------------------------------
def _step_A(c, cap, cs, Y, st, noise, tag):
    """set state -> sparse_step(SSTEP_A); returns everything the checks read."""
    M, H, mode = cs["M"], cs["H"], cs["mode"]
    _load(c, cs, Y, st, noise)
    d0 = c.dims()
    Hp, Mp, Lp = d0["Hp"], 32 * d0["XT1"], 32 * d0["XT2"]
    s0 = c.sparse_get_state()                                        # the fp32 tables as the device holds them
    r = dict(Hp=Hp, NH=d0["NH"], Mp=Mp, Lp=Lp, Ys=c.get_Y(), CA0=s0["CA"].reshape(M, H), sig0=s0["sigmaHat"])
    r["B0"] = _f32(c, cap, cap.PEEK_B32, Lp * Hp).reshape(Lp, Hp)
    c.sparse_step(cap.SSTEP_A)
    d = c.dims()
    _expect_variant(tag, cs, d)
    r["dA"] = d
    r["P"] = _product(c, cap, 0, d)
    r["A1"] = _f32(c, cap, cap.PEEK_A32, Mp * Hp).reshape(Mp, Hp)
    r["FA"] = _tiles(c, cap, d, 0, mode)
    s1 = c.sparse_get_state(want_B=False)
    r["dS1"], r["At1"], r["SAdiag"] = s1["diagSigmaATVec"].reshape(M, H), s1["ATVecHat"].reshape(M, H), s1["SigmaA_diag"]
    r["blkA"] = _block(c, cap, Hp)                                    # B'B (of the set B: the A update forms it), A'A, SigmaA, SigmaB
    return r


def _check_A(tag, cs, r, noise, w):
    M, H, mode = cs["M"], cs["H"], cs["mode"]
    Hp, dA, blk, Ys = r["Hp"], r["dA"], r["blkA"], r["Ys"]
    B0 = r["B0"]
    assert not np.any(B0[L:]) and not np.any(B0[:, H:]), (tag, "B32 padding")
    w["BB0"] = _check_gram(tag + " B'B of the set state", blk["GB"], B0[:L], gram_bound(r, 1), H) / gram_bound(r, 1)
    SBd, GBd = np.diag(blk["SB"])[:H], np.diag(blk["GB"])[:H]
    if cs["diag_var"]:
        s32 = noise[0].astype(np.float32).astype(np.float64)
        F = s32[:, None] * B0[:L, :H]
        v = R.ref_v_rows(s32, B0[:L, :H], r["sig0"], SBd, L)
        assert abs(r["sig0"] - np.mean(noise[0])) <= L * E * r["sig0"], (tag, "mean(sigma) of the set rows")
        sig, gF = 1.0, TILE_R[mode] + U
    else:
        F = B0[:L, :H]
        v = R.ref_v(r["sig0"], GBd, SBd, L)
        sig, gF = r["sig0"], 0.0
    # P against Ys' F per entry
    for s, sl in enumerate(r["P"]):
        assert not np.any(sl[M:]) and not np.any(sl[:, H:]), (tag, "P padding", s)
    Psum, Pabs = np.sum(r["P"], axis=0)[:M, :H], np.sum(np.abs(r["P"]), axis=0)[:M, :H]
    gP = pass_bound(mode, dA["sps1"], dA["nsplit1"])
    gP = gP + gF * (1.0 + gP)
    refP, scP = Ys.T @ F, np.abs(Ys).T @ np.abs(F)
    w["P"] = _worst(np.abs(Psum - refP), gP * scP)
    assert w["P"] <= 1.0, (tag, "P", w["P"])
    # d and a per entry
    labels, H1 = cs["mask"] if cs["mask"] else ((), 0)
    dref, aref, ascale, mask = R.ref_updateA(Psum, Pabs, v, r["CA0"], sig, cs["compat"], labels, H1)
    w["dS"] = _worst(np.abs(r["dS1"] - dref), (U + 16 * E) * dref)
    assert w["dS"] <= 1.0, (tag, "diagSigmaATVec", w["dS"])
    A1 = r["A1"]
    gA = U + TILE_R[mode] + (dA["nsplit1"] - 1) * U + 16 * E
    w["A"] = _worst(np.abs(A1[:M, :H] - aref), gA * ascale)
    assert w["A"] <= 1.0, (tag, "A", w["A"])
    assert np.array_equal(r["At1"], A1[:M, :H]), (tag, "ATVecHat is A32")
    assert not np.any(A1[:M, :H][mask]) and np.all(A1[:M, :H][~mask] != 0.0), (tag, "label mask")
    assert mask.sum() == len(labels) * H1
    assert not np.any(A1[M:]) and not np.any(A1[:, H:]), (tag, "A32 padding")
    _check_tiles(tag + " FA", r["FA"], A1, M)
    # (3) SigmaA and A'A
    SA = blk["SA"]
    sref = np.sum(r["dS1"], axis=0)
    w["SA"] = _worst(np.abs(np.diag(SA)[:H] - sref), M * E * sref)
    assert w["SA"] <= 1.0, (tag, "SigmaA diagonal", w["SA"])
    assert np.array_equal(np.diag(SA)[:H], r["SAdiag"])
    off = SA.copy()
    off[np.arange(H), np.arange(H)] = 0.0
    assert not np.any(off), (tag, "SigmaA off the diagonal / padding")
    w["AA"] = _check_gram(tag + " A'A", blk["GA"], A1[:M], gram_bound(r, 0), H) / gram_bound(r, 0)


# ---- (4): updateCA! ---------------------------------------------------------------------------------------------------------
def _check_CA(c, cap, tag, cs, r, w):
    M, H = cs["M"], cs["H"]
    c.sparse_step(cap.SSTEP_CA)
    s = c.sparse_get_state(want_B=False)
    alpha, beta0 = R.HYPER["alpha0"] + 0.5, R.HYPER["beta0"]
    if cs["group"]:
        g = R.ca_group(M, H, H0, M0 if cs["group"] == "trial" else M)
        assert [int(np.sum(g == k)) > 0 for k in range(3)] == [True, True, cs["group"] == "trial"]
        alpha = np.array([p[0] + 0.5 for p in GROUP_PRIORS])[g]
        beta0 = np.array([p[1] for p in GROUP_PRIORS])[g]
    b, ca = R.ref_updateCA(r["A1"][:M, :H], r["dS1"], alpha, beta0)
    w["beta"] = _worst(np.abs(s["beta"].reshape(M, H) - b), (U + 16 * E) * b)
    w["CA"] = _worst(np.abs(s["CA"].reshape(M, H) - ca), (2 * U + 16 * E) * ca)
    assert w["beta"] <= 1.0 and w["CA"] <= 1.0, (tag, "updateCA", w["beta"], w["CA"])
    assert np.array_equal(s["ATVecHat"].reshape(M, H), r["At1"]) and np.array_equal(s["diagSigmaATVec"].reshape(M, H), r["dS1"])


# ---- (5): updateB! ----------------------------------------------------------------------------------------------------------
def _check_B(c, cap, tag, cs, r, noise, w):
    M, H, mode = cs["M"], cs["H"], cs["mode"]
    Hp, Lp, blk0 = r["Hp"], r["Lp"], r["blkA"]
    c.sparse_step(cap.SSTEP_B)
    d = c.dims()
    blk = _block(c, cap, Hp)
    sig = blk0["sig"]
    Kref = R.ref_K(blk0["CB"][:H], sig, blk0["GA"][:H, :H], blk0["SA"][:H, :H])
    SB = blk["SB"]
    w["SB_fro"] = relF(SB[:H, :H], np.linalg.inv(Kref)) / 5e-5
    assert w["SB_fro"] <= 1.0, (tag, "SigmaB", w["SB_fro"])
    assert not np.any(SB[H:]) and not np.any(SB[:, H:]), (tag, "SigmaB padding")
    SB32 = _f32(c, cap, cap.PEEK_SB32, Hp * Hp).reshape(Hp, Hp)
    want32 = (SB if cs["diag_var"] else sig * SB).astype(np.float32).astype(np.float64)
    assert np.array_equal(SB32, want32), (tag, "SB32 is fp32(sigmaHat SigmaB)")
    Q = _product(c, cap, 1, d, nslab=1)[0]                            # folded into slab 0 when split
    assert not np.any(Q[L:]) and not np.any(Q[:, H:]), (tag, "Q padding")
    B1 = _f32(c, cap, cap.PEEK_B32, Lp * Hp).reshape(Lp, Hp)
    ref, scale = Q @ SB32, np.abs(Q) @ np.abs(SB32)
    g = post_bound(mode, Hp)
    if cs["diag_var"]:
        s32 = np.zeros(Lp)
        s32[:L] = noise[0].astype(np.float32).astype(np.float64)
        ref, scale = s32[:, None] * ref, s32[:, None] * scale
        g = g + (U + TILE_R[mode]) * (1.0 + g)                        # the row scaling's rounding, then the second tiling
    w["B"] = _worst(np.abs(B1 - ref)[:L, :H], (g * scale)[:L, :H])
    assert w["B"] <= 1.0, (tag, "B", w["B"])
    assert not np.any(B1[L:]) and not np.any(B1[:, H:]), (tag, "B32 padding")
    _check_tiles(tag + " FB", _tiles(c, cap, d, 1, mode), B1, L)
    gb = gram_bound(r, 1)
    w["BB"] = _check_gram(tag + " B'B", blk["GB"], B1[:L], gb, H) / gb
    # (the delta is formed in fp32 and, at NH >= 4 in the bf16 modes, re-split into bf16 hi + lo: tests/test_gpu_stream_passes.py)
    w["dBdB"] = _check_gram(tag + " dB'dB", blk["GD"], r["B0"][:L] - B1[:L], gb + 2.0 ** -14, H) / (gb + 2.0 ** -14)
    if not cs["diag_var"]:                                            # (diag_var rescales the rows afterwards: no trace from the post kernel)
        tr, trs = float(np.sum(Q[:L, :H] * B1[:L, :H])), float(np.sum(np.abs(Q[:L, :H] * B1[:L, :H])))
        w["tr"] = abs(blk["GX"] - tr) / max(18 * U * trs, 1e-300)
        assert w["tr"] <= 1.0, (tag, "tr(B'YA)", blk["GX"], tr, trs)
    assert np.array_equal(blk["GA"], blk0["GA"]) and np.array_equal(blk["SA"], blk0["SA"])
    return dict(blk=blk, B1=B1, Q=Q, d=d)


# ---- (6), (7): updateCB!, updateSigma! --------------------------------------------------------------------------------------
def _check_CB_sigma(c, cap, tag, cs, r, rb, noise, w):
    M, H = cs["M"], cs["H"]
    Hp, blk0 = r["Hp"], rb["blk"]
    c.sparse_step(cap.SSTEP_CB | cap.SSTEP_SIGMA)
    blk = _block(c, cap, Hp)
    hy = R.HYPER
    dl, cb = R.ref_updateCB(np.diag(blk0["GB"])[:H], np.diag(blk0["SB"])[:H], hy["gamma0"] + 0.5 * L, hy["delta0"])
    w["delta"] = _worst(np.abs(blk["delta"][:H] - dl), 8 * E * dl)
    w["CB"] = _worst(np.abs(blk["CB"][:H] - cb), 8 * E * cb)
    assert w["delta"] <= 1.0 and w["CB"] <= 1.0, (tag, "updateCB", w["delta"], w["CB"])
    GA, SA, GB, SB = (blk0[k][:H, :H] for k in ("GA", "SA", "GB", "SB"))
    if not cs["diag_var"]:
        assert blk["trBQ"] == blk0["GX"], (tag, "tr(B'YA) is the B update's")
        zref, mag = R.ref_zeta(hy["zeta0"], blk0["trYY"], blk["trBQ"], GA, SA, GB, SB, L)
        assert zref > 0.0
        w["zeta"] = abs(blk["zeta"] - zref) / ((H * H + 16) * E * mag)
        sref = (hy["eta0"] + 0.5 * L * M) / blk["zeta"]
        w["sigma"] = abs(blk["sig"] - sref) / (8 * E * sref)
        assert w["zeta"] <= 1.0 and w["sigma"] <= 1.0, (tag, "updateSigma", w["zeta"], w["sigma"], blk["zeta"], zref)
        s = c.sparse_get_state(want_B=False)
        assert s["zeta"] == blk["zeta"] and s["sigmaHat"] == blk["sig"]
        return
    sigv, zetav = c.sparse_get_noise_rows()
    G64 = GA + SA
    G32 = G64.astype(np.float32).astype(np.float64)
    zl, magl, aquad = R.ref_zeta_rows(hy["zeta0"], r["Ys"], rb["Q"][:L, :H], rb["B1"][:L, :H], G64, SB, Gq=G32)
    assert np.all(zl > 0.0)
    w["zeta_l"] = _worst(np.abs(zetav - zl), 0.5 * (H + 2) * U * aquad + (M + 2 * H + 16) * E * magl)
    w["sigma_l"] = _worst(np.abs(sigv - noise[2] / zetav), 8 * E * noise[2] / zetav)
    w["mean"] = abs(blk["sig"] - float(np.mean(sigv))) / (L * E * float(np.mean(sigv)))
    assert w["zeta_l"] <= 1.0 and w["sigma_l"] <= 1.0 and w["mean"] <= 1.0, (tag, "row noise", w["zeta_l"], w["sigma_l"], w["mean"])


# ---- the case table ---------------------------------------------------------------------------------------------------------
# (tag, M, H, mode; fused, compat, mask = (labels0, H1), diag_var, forced pass1_splits, grouped model)
MK = lambda M, H1: (_labels(M), H1)
CASES = [
    # the 11 reachable sparse_update_a_tiles_kernel<MODE, NH> (single bf16 is refused above H = 128), M = 97 or 33
    K("fused-f32-nh1-h1-m33", 33, 1, "f32", mask=MK(33, 1)),                          # H1 = H: every column of the labelled rows
    K("fused-f32-nh2-h33", 97, 33, "f32"),
    K("fused-f32-nh4-h65", 97, 65, "f32", mask=MK(97, 2)),
    K("fused-f32-nh8-h129", 97, 129, "f32"),
    K("fused-bf16-nh1-h31", 97, 31, "bf16", mask=MK(97, 2)),
    K("fused-bf16-nh2-h64-m33", 33, 64, "bf16"),
    K("fused-bf16-nh4-h128", 97, 128, "bf16"),
    K("fused-bf16x2-nh1-h31-m33", 33, 31, "bf16x2"),
    K("fused-bf16x2-nh2-h33", 97, 33, "bf16x2", mask=MK(97, 2)),
    K("fused-bf16x2-nh4-h65-nocompat", 97, 65, "bf16x2", compat=False),
    K("fused-bf16x2-nh8-h256", 97, 256, "bf16x2", mask=MK(97, 2)),
    # sparse_update_a_kernel + retile_kernel, one H per NH
    K("unfused-f32-nh1-h31", 97, 31, "f32", fused=0),
    K("unfused-f32-nh2-h64", 97, 64, "f32", fused=0, mask=MK(97, 2)),
    K("unfused-f32-nh4-h128-m33", 33, 128, "f32", fused=0),
    K("unfused-f32-nh8-h256", 97, 256, "f32", fused=0),
    K("unfused-bf16x2-nh1-h1", 97, 1, "bf16x2", fused=0),
    K("unfused-bf16x2-nh2-h33-nocompat", 97, 33, "bf16x2", fused=0, compat=False),
    K("unfused-bf16x2-nh4-h128", 97, 128, "bf16x2", fused=0, mask=MK(97, 2)),
    K("unfused-bf16x2-nh8-h129-m33", 33, 129, "bf16x2", fused=0),
    # M below one tile: M = 2 (the smallest the repeat(v, inner = M-1) layout admits), M = 31
    K("fused-bf16x2-nh1-h31-m2", 2, 31, "bf16x2", mask=([0, 1], 2)),
    K("fused-f32-nh1-h31-m31", 31, 31, "f32"),
    # M = 1057: colsum_part_kernel's unrolled loop runs
    K("fused-bf16x2-nh2-h33-m1057", 1057, 33, "bf16x2"),
    K("fused-f32-nh8-h129-m1057", 1057, 129, "f32"),
    # a forced split count of the Y'B pass: slab_sum_kernel over three slabs
    # (at NH <= 2 the bf16 modes' 24 k-steps of L = 257 admit two splits only)
    K("fused-bf16x2-nh8-h129-split3", 97, 129, "bf16x2", splits=3),
    K("fused-f32-nh4-h65-split3", 97, 65, "f32", splits=3),
    # heteroscedastic rows, one case per NH in f32 and bf16x2
    K("diagvar-f32-nh1-h31", 97, 31, "f32", diag_var=True),
    K("diagvar-f32-nh2-h33", 97, 33, "f32", diag_var=True, mask=MK(97, 2)),
    K("diagvar-f32-nh4-h65", 97, 65, "f32", diag_var=True),
    K("diagvar-f32-nh8-h129-m33", 33, 129, "f32", diag_var=True),
    K("diagvar-bf16x2-nh1-h1-m33", 33, 1, "bf16x2", diag_var=True),
    K("diagvar-bf16x2-nh2-h64", 97, 64, "bf16x2", diag_var=True),
    K("diagvar-bf16x2-nh4-h128", 97, 128, "bf16x2", diag_var=True),
    K("diagvar-bf16x2-nh8-h256", 97, 256, "bf16x2", diag_var=True),
    # the grouped models: updateCA! with each entry's own group's hyper-prior
    K("dual-f32-nh2-h33", 97, 33, "f32", group="dual"),
    K("trial-bf16x2-nh2-h33", 97, 33, "bf16x2", group="trial"),
]


@pytest.mark.parametrize("cs", CASES, ids=[c["tag"] for c in CASES])
def test_each_update_entry_by_entry(pkg, monkeypatch, cs):
    cap, tag = pkg.capi, cs["tag"]
    Y, st, noise = _inputs(cs)
    w = {}
    with _context(pkg, monkeypatch, cs) as c:
        r = _step_A(c, cap, cs, Y, st, noise, tag)
        _check_A(tag, cs, r, noise, w)
        _check_CA(c, cap, tag, cs, r, w)
        rb = _check_B(c, cap, tag, cs, r, noise, w)
        _check_CB_sigma(c, cap, tag, cs, r, rb, noise, w)
    report(f"sparse entries {tag}: " + " ".join(f"{k}={v:.2e}" for k, v in w.items() if k not in E_LEVEL)
           + "  [" + " ".join(f"{k}={v:.2e}" for k, v in w.items() if k in E_LEVEL)
           + f"; nsplit {r['dA']['nsplit1']}/{rb['d']['nsplit2']}, sps {r['dA']['sps1']}/{rb['d']['sps2']}, q_frag {rb['d']['q_frag']}]")


def test_single_bf16_is_refused_above_rank_128(pkg, monkeypatch):
    with pytest.raises(pkg.capi.VbmfError):
        _context(pkg, monkeypatch, K("bf16-h129", 97, 129, "bf16"))


# ---- (2): fused equals unfused ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", [c for c in CASES if not c["fused"]], ids=[c["tag"] for c in CASES if not c["fused"]])
def test_fused_update_equals_update_plus_retile(pkg, monkeypatch, cs):
    cap, tag = pkg.capi, cs["tag"]
    Y, st, noise = _inputs(cs)
    out = []
    for fused in (1, 0):
        k = dict(cs, fused=fused)
        with _context(pkg, monkeypatch, k) as c:
            out.append(_step_A(c, cap, k, Y, st, noise, tag))
    a, b = out
    assert a["dA"]["sparse_a_fused"] == 1 and b["dA"]["sparse_a_fused"] == 0
    assert np.array_equal(a["A1"], b["A1"]), (tag, "A32", int(np.sum(a["A1"] != b["A1"])))
    assert np.array_equal(a["dS1"], b["dS1"]), (tag, "diagSigmaATVec")
    assert np.array_equal(a["FA"], b["FA"]), (tag, "operand tiles")
    assert np.array_equal(a["blkA"]["GA"], b["blkA"]["GA"]) and np.array_equal(a["blkA"]["SA"], b["blkA"]["SA"])


# ---- (8): a sweep as a run equals the sweep as steps ------------------------------------------------------------------------
RUN_CASES = [
    K("run-bf16x2-nh2-h33", 97, 33, "bf16x2", mask=MK(97, 2)),              # no side stream
    K("run-f32-nh8-h129", 97, 129, "f32"),                                  # side stream: updateCA! beside the next pass, sparse_t2_kernel
    K("run-bf16x2-nh8-h256", 97, 256, "bf16x2"),
    K("run-diagvar-bf16x2-nh8-h129", 97, 129, "bf16x2", diag_var=True),     # side stream without the t2 pre-sum
]
STATE_FIELDS = ("ATVecHat", "diagSigmaATVec", "CA", "beta", "BHat", "SigmaB", "CB", "delta")


def _sweep(pkg, monkeypatch, cs, how):
    cap = pkg.capi
    Y, st, noise = _inputs(cs)
    with _context(pkg, monkeypatch, cs) as c:
        _load(c, cs, Y, st, noise)
        if how == "run":
            it, _, _ = c.sparse_run(1, eps=0.0, est_cb=True)
            assert it == 1
        elif how == "steps":
            c.sparse_step(cap.SSTEP_A | cap.SSTEP_B | cap.SSTEP_CA | cap.SSTEP_CB | cap.SSTEP_SIGMA)
        elif how == "fixed":
            c.sparse_run_fixed_basis(2)
        else:
            for _ in range(2):
                c.sparse_step(cap.SSTEP_A)
                c.sparse_step(cap.SSTEP_CA)
                c.sparse_step(cap.SSTEP_SIGMA)
        d = c.dims()
        _expect_variant(cs["tag"], cs, d)
        s = c.sparse_get_state()
        s["blk"] = _block(c, cap, d["Hp"])
        if cs["diag_var"]:
            s["sigmaVecHat"], s["zetaVec"] = c.sparse_get_noise_rows()
    return s


@pytest.mark.parametrize("cs", RUN_CASES, ids=[c["tag"] for c in RUN_CASES])
def test_one_sweep_as_a_run_equals_the_sweep_as_steps(pkg, monkeypatch, cs):
    tag, M, H = cs["tag"], cs["M"], cs["H"]
    a, b = _sweep(pkg, monkeypatch, cs, "run"), _sweep(pkg, monkeypatch, cs, "steps")
    for f in STATE_FIELDS + (("sigmaVecHat", "zetaVec", "sigmaHat") if cs["diag_var"] else ()):
        assert np.array_equal(a[f], b[f]), (tag, f, int(np.sum(np.asarray(a[f]) != np.asarray(b[f]))))
    if cs["diag_var"]:
        return
    if NH_OF(H) < 8:
        assert a["zeta"] == b["zeta"] and a["sigmaHat"] == b["sigmaHat"], (tag, a["zeta"], b["zeta"])
        return
    # NH = 8: the run sums t2 in sparse_t2_kernel's 64 shares, the step in one workgroup: each to the bound of (6)
    blk = b["blk"]                                                    # GA, SA, GB, SB, tr(B'YA): untouched by updateCB! / updateSigma!
    assert all(np.array_equal(a["blk"][k], blk[k]) for k in ("GA", "SA", "GB", "SB")) and a["blk"]["trBQ"] == blk["trBQ"]
    zref, mag = R.ref_zeta(R.HYPER["zeta0"], blk["trYY"], blk["trBQ"], *(blk[k][:H, :H] for k in ("GA", "SA", "GB", "SB")), L)
    eta = R.HYPER["eta0"] + 0.5 * L * M
    worst = 0.0
    for s in (a, b):
        wz = abs(s["zeta"] - zref) / ((H * H + 16) * E * mag)
        ws = abs(s["sigmaHat"] - eta / s["zeta"]) / (8 * E * eta / s["zeta"])
        assert wz <= 1.0 and ws <= 1.0, (tag, "zeta", s["zeta"], zref, wz, ws)
        worst = max(worst, wz)
    report(f"sparse entries {tag}: [zeta={worst:.2e}]")


@pytest.mark.parametrize("cs", RUN_CASES[:2], ids=[c["tag"].replace("run-", "fixed-") for c in RUN_CASES[:2]])
def test_fixed_basis_run_equals_its_steps(pkg, monkeypatch, cs):
    """sparse_run_fixed_basis(2) (the second round reuses Y'B: reuse_P) against two rounds of step(A), step(CA), step(SIGMA), each of
    which forms Y'B again from the unchanged B: plain stores of a fixed summation order, bitwise equal."""
    a, b = _sweep(pkg, monkeypatch, cs, "fixed"), _sweep(pkg, monkeypatch, cs, "fixed-steps")
    for f in STATE_FIELDS + ("zeta", "sigmaHat"):
        assert np.array_equal(a[f], b[f]), (cs["tag"], f)
    assert a["zeta"] != R.synthetic_state(L, cs["M"], cs["H"], 0)["zeta"]
