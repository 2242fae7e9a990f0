"""The label mask AHat[labels, end-H1+1:end] = 0 (src/vbmf.jl:101) of the basic model's streaming sweep, entry by entry, in every
A-update variant the host can choose (csrc/post_kernels.hpp: post_gram_tile_regs of post_gram2_kernel, post_kernel, and
post_frag_tail of post_frag2_kernel / post_frag3_kernel), and on the paths around the update (fixed basis, row shards).

Each case of test_mask_per_entry runs one masked session m and one unmasked session u of the same Y, state and environment
(the scaffolding of test_gpu_stream_passes.py: STEP_A, then STEP_B on the A it left) and asserts through dims() that it reached
the variant it names:
 1. pass 1 does not see the mask: every P slab of m equals that of u bitwise;
 2. A1_m == where(masked, +0.0, A1_u) on the uint32 views (fixed-order plain stores: an equality; a -0.0, a mask tested with
    > for >=, a missed second tile of a wave or a changed unmasked entry fails);
 3. the operand tiles decode to A1_m bitwise with zero padding (a mask applied after write_factor_tiles fails);
 4. A'A of the state against the fp64 Gram of A1_m (gram_bound), where every masked column must differ from the unmasked Gram by
    more than 4 gram_bound (a condition on the inputs: a Gram taken before the mask cannot pass);
 5. pass 2 multiplied by the masked tiles: B1 (and Q where it is stored) against Ys A1_m per entry;
 6. u itself: sum_slabs P against Ys'B32 (bitwise on the exact data) and A1_u = tile(fp32(P SA32)) per entry.

Label sets: `prefix`, rows 0 .. M // 4 (how the reference's train_local uses the mask; not a multiple of 32), and `scattered`,
{0, 31, 32, 63, 64, M - 2, M - 1} plus every seventh row (tile edges, both halves of a 32-row tile, the ragged last tile).
H1 in {1, H} and, for H > 32, the H1 that puts hmask_start = H - H1 three columns before the last 32-column tile edge inside H."""
import threading

import numpy as np
import pytest

import __graft_entry__ as G
from oracle import vbmf_oracle as O
from tests.helpers import compare, relF, report, to_pkg_params
from tests.test_gpu_many_ranks import ThreadAllReduce
from tests.test_gpu_parity import TOL_F32, TOL_X2, _problem
from tests.test_gpu_stream_passes import (LONG, _check_factor, _check_gram, _check_tiles, _exact_Y, _expect, _real_Y, _session,
                                          _state, gram_bound, pass_bound)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


SHORT = lambda v: v < 2048                     # launch_post_frag: one 32-row tile per wave
NARROW = {"VBMF_NARROW": "1"}
POST2 = {"VBMF_POST3": "0"}
# (id, L, M, H, mode, env, pass1_splits, expected dims after STEP_A, the A update's kernel)
# (pass1_splits = 1: an un-split pass 1, so that post_gram2 reads c->P itself; the planner's own choice at this shape is six
#  slabs, summed into c->Pred like the three forced ones of the -pred case)
CASES = [
    ("f32-nh1-gram2", 1057, 385, 31, "f32", NARROW, 1, dict(NH=1, narrow=1, p_frag=1, nsplit1=1), "post_gram2_kernel<F32, 1, false> on P"),
    ("bf16-nh1-gram2", 1057, 385, 31, "bf16", NARROW, 1, dict(NH=1, narrow=1, p_frag=1, nsplit1=1), "post_gram2_kernel<BF16, 1, false> on P"),
    ("bf16x2-nh1-gram2", 1057, 385, 31, "bf16x2", NARROW, 1, dict(NH=1, narrow=1, p_frag=1, nsplit1=1), "post_gram2_kernel<BF16X2, 1, false> on P"),
    ("f32-nh2-gram2", 1057, 385, 64, "f32", NARROW, 1, dict(NH=2, narrow=1, p_frag=1, nsplit1=1), "post_gram2_kernel<F32, 2, false> on P"),
    ("bf16-nh2-gram2", 1057, 385, 64, "bf16", NARROW, 1, dict(NH=2, narrow=1, p_frag=1, nsplit1=1), "post_gram2_kernel<BF16, 2, false> on P"),
    ("bf16x2-nh2-gram2", 1057, 385, 64, "bf16x2", NARROW, 1, dict(NH=2, narrow=1, p_frag=1, nsplit1=1), "post_gram2_kernel<BF16X2, 2, false> on P"),
    ("bf16x2-nh2-gram2-pred", 3001, 225, 33, "bf16x2", {}, 3, dict(NH=2, p_frag=1, nsplit1=3), "post_gram2_kernel<BF16X2, 2, false> on Pred"),
    ("f32-nh4-post", 2049, 161, 65, "f32", {}, 0, dict(NH=4, mode=0, p_frag=0), "post_kernel<F32, 4>"),
    ("f32-nh8-post", 2049, 161, 129, "f32", {}, 0, dict(NH=8, mode=0, p_frag=0), "post_kernel<F32, 8> (NXT = 2)"),
    ("bf16-nh4-post3", 2049, 161, 100, "bf16", {}, 0, dict(NH=4, p_frag=1, post3=1, XT1=SHORT), "post_frag3_kernel<BF16, 4, 1, false>"),
    ("bf16x2-nh4-post3", 2049, 161, 128, "bf16x2", {}, 0, dict(NH=4, p_frag=1, post3=1, XT1=SHORT), "post_frag3_kernel<BF16X2, 4, 1, false>"),
    ("bf16x2-nh8-post3", 2049, 161, 129, "bf16x2", {}, 0, dict(NH=8, p_frag=1, post3=1, XT1=SHORT), "post_frag3_kernel<BF16X2, 8, 1, false>"),
    ("bf16-nh4-post2", 2049, 161, 100, "bf16", POST2, 0, dict(NH=4, p_frag=1, post3=0, XT1=SHORT), "post_frag2_kernel<BF16, 4, 1, false>"),
    ("bf16x2-nh4-post2", 2049, 161, 128, "bf16x2", POST2, 0, dict(NH=4, p_frag=1, post3=0, XT1=SHORT), "post_frag2_kernel<BF16X2, 4, 1, false>"),
    ("bf16x2-nh8-post2", 2049, 161, 129, "bf16x2", POST2, 0, dict(NH=8, p_frag=1, post3=0, XT1=SHORT), "post_frag2_kernel<BF16X2, 8, 1, false>"),
    ("bf16x2-nh4-longA-post3", 97, 65601, 128, "bf16x2", {}, 0, dict(NH=4, p_frag=1, post3=1, XT1=LONG), "post_frag3_kernel<BF16X2, 4, 2, false>"),
    ("bf16x2-nh4-longA-post2", 97, 65601, 128, "bf16x2", POST2, 0, dict(NH=4, p_frag=1, post3=0, XT1=LONG), "post_frag2_kernel<BF16X2, 4, NXT4, false>"),
    ("bf16x2-nh8-longA-post2", 97, 65601, 129, "bf16x2", POST2, 0, dict(NH=8, p_frag=1, post3=0, XT1=LONG), "post_frag2_kernel<BF16X2, 8, NXT8, false>"),
]
# the real-data flavour: one case per kernel family
REAL = ["bf16x2-nh2-gram2", "f32-nh8-post", "bf16x2-nh4-post3", "bf16x2-nh8-post2", "bf16x2-nh4-longA-post3"]
LABELS = ["prefix", "scattered"]
H1S = ["one", "all", "intile"]


def _labels(kind, M):
    if kind == "prefix":
        return np.arange(M // 4 + 1)
    return np.unique(np.concatenate([[0, 31, 32, 63, 64, M - 2, M - 1], np.arange(0, M, 7)]))


def _h1(kind, H):
    """H1, or None where the kind does not apply (H <= 32: no 32-column tile edge inside H).  "intile": hmask_start = H - H1 lies
    three columns before the edge of the last tile that holds real columns, so the mask starts inside one tile and covers a whole
    later one (and the padding columns behind it)."""
    if kind == "one":
        return 1
    if kind == "all":
        return H
    k = -(-H // 32) - 1
    return H - (32 * k - 3) if k >= 1 else None


def _bits(F):
    return np.ascontiguousarray(F, dtype=np.float32).view(np.uint32)


_unmasked = {}                                 # the unmasked session of the case in hand: made once, shared, left unchanged


def _pair(pkg, monkeypatch, case, exact, labels, H1):
    tag, L, M, H, mode, env, splits = case[:7]
    key = (tag, exact)
    if key not in _unmasked:
        _unmasked.clear()                      # (one case's buffers at a time: the long side's are 100 MB)
        Y = _exact_Y(L, M, 8000 + L + M + H) if exact else _real_Y(L, M, H, 8200 + L + H)
        st = _state(L, M, H, 8100 + H, exact)
        _unmasked[key] = (Y, st, _session(pkg, monkeypatch, L, M, H, mode, Y, st, env, splits, what="A"))
    Y, st, u = _unmasked[key]
    m = _session(pkg, monkeypatch, L, M, H, mode, Y, st + (labels, H1), env, splits, what="chain")
    return m, u


def _check_mask_pair(tag, case, m, u, labels, H1, exact):
    _, L, M, H, mode, env, splits, exp, kernel = case
    Hp, Mp, Lp, dA, dB = m["Hp"], m["Mp"], m["Lp"], m["dA"], m["dB"]
    got = _expect(tag, dA, exp)
    assert _expect(tag, u["dA"], exp) == got
    hs = H - H1                                                        # hmask_start
    Ys, aY = m["Ys"], np.abs(m["Ys"])
    assert np.array_equal(Ys, u["Ys"]) and np.array_equal(m["B0"], u["B0"])
    # 6. the unmasked session is right: P against Ys'B32, A from P
    B0 = u["B0"][:L]
    Pref, Pscale = np.zeros((Mp, Hp)), np.zeros((Mp, Hp))
    Pref[:M], Pscale[:M] = Ys.T @ B0, aY.T @ np.abs(B0)
    Psum = np.sum(u["P"], axis=0)
    g1 = 0.0 if exact else pass_bound(mode, dA["sps1"], dA["nsplit1"])
    if exact:
        assert np.array_equal(Psum, Pref), (tag, "sum_slabs P differs from Ys'B32")
    else:
        assert np.all(np.abs(Psum - Pref) <= g1 * Pscale), (tag, "P", float(np.max(np.abs(Psum - Pref) / np.maximum(Pscale, 1e-300))), g1)
    for sl in u["P"]:
        assert not np.any(sl[M:]) and not np.any(sl[:, H:]), (tag, "P padding")
    wA = _check_factor(tag + " A unmasked", u["A1"], M, Pref, u["SA32"], mode, Hp, H, prod_scale=None if exact else Pscale, g_prod=g1)
    # 1. pass 1 does not see the mask
    assert len(m["P"]) == len(u["P"]) == dA["nsplit1"]
    for s, (x, y) in enumerate(zip(m["P"], u["P"])):
        assert np.array_equal(_bits(x), _bits(y)), (tag, "P slab differs under the mask", s, int(np.sum(x != y)))
    assert np.array_equal(m["SA32"], u["SA32"])
    # 2. the mask is exact and changes nothing else
    masked = np.zeros((Mp, Hp), dtype=bool)
    masked[np.ix_(labels, np.arange(hs, Hp))] = True
    want = np.where(masked, 0.0, u["A1"])
    bad = np.argwhere(_bits(m["A1"]) != _bits(want))
    assert bad.size == 0, (tag, f"{len(bad)} entries of the masked A differ from where(masked, +0.0, unmasked A)", bad[:8].tolist())
    assert np.count_nonzero(u["A1"][np.ix_(labels, np.arange(hs, H))]) > 0.9 * len(labels) * H1, (tag, "the unmasked A is zero there anyway")
    # 3. operand tiles
    _check_tiles(tag + " FA", m["FA"], m["A1"], M)
    # 4. A'A of the masked A; the Gram of the unmasked A is further away than the bound in every masked column
    gb = gram_bound(m, 0)
    wG = _check_gram(tag + " A'A", m["GA"], m["A1"][:M], gb, H)
    Au, Am = u["A1"][:M, hs:H], m["A1"][:M, hs:H]
    gap, scale = np.sum(Au * Au, axis=0) - np.sum(Am * Am, axis=0), np.sum(Au * Au, axis=0)
    assert np.all(gap > 4 * gb * scale), (tag, "the Gram check has no power here", float(np.min(gap / scale)), gb)
    # 5. pass 2 reads the masked tiles: Q = Ys A1_m, B = tile(fp32(Q SB32))
    A1 = m["A1"][:M]
    g2 = pass_bound(mode, dB["sps2"], max(dB["nsplit2"], dB["streamk_per"]))
    Qx, Qs = np.zeros((Lp, Hp)), np.zeros((Lp, Hp))
    Qx[:L], Qs[:L] = Ys @ A1, aY @ np.abs(A1)
    wQ = 0.0
    if m["Q"] is not None:
        Q = m["Q"]
        wQ = float(np.max(np.abs(Q - Qx) / np.maximum(Qs, 1e-300)))
        assert np.all(np.abs(Q - Qx) <= g2 * Qs), (tag, "Q", wQ, g2)
        assert not np.any(Q[L:]) and not np.any(Q[:, H:]), (tag, "Q padding")
    wB = _check_factor(tag + " B", m["B1"], L, Qx, m["SB32"], mode, Hp, H, prod_scale=Qs, g_prod=g2)
    _check_tiles(tag + " FB", m["FB"], m["B1"], L)
    report(f"label mask {'exact' if exact else 'real'} {tag}: A_entry={wA:.2e} AA={wG:.2e} Q_entry={wQ:.2e} B_entry={wB:.2e}"
           f" gap={float(np.min(gap / scale)):.2e}  [{kernel}; " + " ".join(f"{k}={v}" for k, v in got.items()) + "]")


# (case, label set, H1 kind): the in-tile H1 needs a tile edge inside H
MASKS = [(c, lab, h1) for c in CASES for lab in LABELS for h1 in H1S if _h1(h1, c[3]) is not None]


@pytest.mark.parametrize("case,lab,h1", MASKS, ids=[f"{c[0]}-{lab}-{h1}" for c, lab, h1 in MASKS])
def test_mask_per_entry(pkg, monkeypatch, case, lab, h1):
    tag, L, M, H = case[:4]
    H1 = _h1(h1, H)
    labels = _labels(lab, M)
    m, u = _pair(pkg, monkeypatch, case, True, labels, H1)
    _check_mask_pair(f"{tag} {lab} H1={H1}", case, m, u, labels, H1, True)


@pytest.mark.parametrize("tag", REAL)
def test_mask_per_entry_real_data(pkg, monkeypatch, tag):
    case = next(c for c in CASES if c[0] == tag)
    M, H = case[2], case[3]
    H1 = _h1("intile", H)
    labels = _labels("scattered", M)
    m, u = _pair(pkg, monkeypatch, case, False, labels, H1)
    _check_mask_pair(f"{tag} scattered H1={H1}", case, m, u, labels, H1, False)


# ---- the mask around the update -----------------------------------------------------------------------------------------------
@pytest.fixture
def defaults(pkg):
    """set_defaults for one test; the package's defaults as they were afterwards."""
    saved = dict(pkg._defaults)
    yield pkg.set_defaults
    pkg.set_defaults(**saved)


def test_fixed_basis_with_mask(pkg, defaults):
    """vbls! with a label mask: run_fixed_basis leaves the H x H loop (fast = !has_mask && ...) and runs every iteration the general
    way on the stored P."""
    L, M, H, H1 = 160, 70, 4, 2
    labels = _labels("scattered", M)
    Y, po = _problem(L, M, H, 9, H1=H1, labels=labels)
    defaults(y_dtype=pkg.VBMF_Y_F32, factor_dtype=pkg.VBMF_FACTOR_AUTO)
    Yf = Y.astype(np.float32).astype(np.float64)
    O.vbmf_(Yf, po, 5, eps=0.0, est_covs=True, est_var=True)
    pg = to_pkg_params(pkg, po)
    B0 = po.BHat.copy()
    pkg.vbls_(Yf, pg, 4)
    O.vbls_(Yf, po, 4)
    assert np.array_equal(_bits(pg.BHat), _bits(B0))                  # (B is fp32 on the device; set and read back unchanged)
    assert relF(pg.BHat, B0) < 1e-6
    blk = pg.AHat[np.ix_(labels, np.arange(H - H1, H))]
    assert not np.any(blk) and not np.any(np.signbit(blk))
    assert np.all(pg.AHat[np.ix_(labels, np.arange(H - H1))] != 0.0)
    compare("vbls masked 4 iters", pg, po, {k: 4 * v for k, v in TOL_F32.items()})


def test_fixed_basis_general_path_wide_rank(pkg, defaults):
    """vbls! at H = 100 (NH = 4 never takes the H x H loop): every iteration the general way, bf16x2."""
    L, M, H = 300, 180, 100
    Y, po = _problem(L, M, H, 19)
    ydt, fdt = pkg.VBMF_Y_BF16, pkg.VBMF_FACTOR_BF16X2
    with pkg.capi.Context(L, M, H, y_dtype=ydt, factor_dtype=fdt) as c:
        c.set_Y(Y)
        Ys = np.ascontiguousarray(c.get_Y())
        assert c.dims()["NH"] == 4
    defaults(y_dtype=ydt, factor_dtype=fdt)
    O.vbmf_(Ys, po, 2, eps=0.0, est_covs=True, est_var=True)
    pg = to_pkg_params(pkg, po)
    B0 = po.BHat.copy()
    pkg.vbls_(Ys, pg, 4)
    O.vbls_(Ys, po, 4)
    assert relF(pg.BHat, B0) <= 2.0 ** -16                           # B comes back as its operand tiles encode it (bf16 hi + lo)
    compare("vbls H100 bf16x2 4 iters", pg, po, {k: 4 * v for k, v in TOL_X2.items()})


def test_row_sharded_with_mask(pkg):
    """Three row shards (threads of this process, tests/test_gpu_many_ranks.py) carry the mask: the replicated AHat is masked on
    every rank, bit-identical over the ranks, and the run follows the fp64 oracle with the same labels."""
    world, L, M, H, niter, H1 = 3, 2603, 700, 40, 3, 3
    labels = _labels("prefix", M)
    rng = np.random.default_rng(9130)
    Bs = rng.standard_normal((L, H)) * np.linspace(1.0, 3.0, H)
    As = np.zeros((M, H))
    As[np.arange(M), rng.integers(0, H, M)] = 1.0
    Y = Bs @ As.T + 0.05 * rng.standard_normal((L, M))
    A0, B0 = rng.standard_normal((M, H)), rng.standard_normal((L, H))
    z = np.zeros((H, H))
    ar = ThreadAllReduce(world)
    out, errs_t = [None] * world, []

    def rank_main(r):
        try:
            r0, n = pkg.dist.row_shard(L, world, r)
            with pkg.capi.Context(n, M, H, y_dtype=pkg.VBMF_Y_BF16, nranks=world, rank=r, L_global=L, row_offset=r0) as c:
                c.comm_set_transport(pkg.dist.host_staged_transport(ar.make(r)))
                c.set_Y(Y[r0:r0 + n])
                c.set_state(A0, B0[r0:r0 + n], z, z, 0.1 * np.ones(H), 0.1 * np.ones(H), 0.1, labels, H1)
                it, d, _ = c.run(niter, eps=0.0, est_covs=True, est_var=True)
                out[r] = dict(it=it, d=d, Ys=c.get_Y(), **c.get_state())
        except Exception as e:                                 # a failed rank must not leave the others at the barrier
            errs_t.append((r, repr(e)))
            ar.bar.abort()

    ths = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in ths)
    assert not errs_t, errs_t
    assert all(o is not None for o in out)
    for k in ("AHat", "SigmaA", "SigmaB", "CA_diag", "CB_diag", "sigma2", "d", "it"):
        for o in out[1:]:
            assert np.array_equal(out[0][k], o[k]), k
    for o in out:
        blk = o["AHat"][np.ix_(labels, np.arange(H - H1, H))]
        assert not np.any(blk) and not np.any(np.signbit(blk))
        assert np.all(o["AHat"][np.ix_(labels, np.arange(H - H1))] != 0.0)
    B = np.concatenate([o["BHat"] for o in out], axis=0)
    Ys = np.concatenate([o["Ys"] for o in out], axis=0)
    po = O.vbmf_parameters()
    po.L, po.M, po.H, po.H1 = L, M, H, H1
    po.labels = labels.astype(np.int64)
    po.AHat, po.BHat = A0.copy(), B0.copy()
    po.SigmaA = np.zeros((H, H)); po.SigmaB = np.zeros((H, H))
    po.CA = 0.1 * np.eye(H); po.CB = 0.1 * np.eye(H); po.invCA = 10 * np.eye(H); po.invCB = 10 * np.eye(H)
    po.sigma2 = 0.1
    _, n, d = O.vbmf_(Ys, po, niter, eps=0.0, est_covs=True, est_var=True, fused=True)
    assert out[0]["it"] == n == niter
    e = dict(A=relF(out[0]["AHat"], po.AHat), B=relF(B, po.BHat), SA=relF(out[0]["SigmaA"], po.SigmaA), SB=relF(out[0]["SigmaB"], po.SigmaB),
             ca=relF(out[0]["CA_diag"], np.diag(po.CA)), cb=relF(out[0]["CB_diag"], np.diag(po.CB)),
             s2=abs(float(out[0]["sigma2"]) - po.sigma2) / po.sigma2, d=abs(float(out[0]["d"]) - d) / d)
    report(f"{world} ranks (threads, one GPU) with a label mask vs fp64 ORACLE, {L}x{M} H={H}, {niter} sweeps: "
           + " ".join(f"{k}={v:.2e}" for k, v in e.items()))
    assert max(e[k] for k in ("A", "B", "SA", "SB", "ca", "cb")) < 2e-4, e
    assert e["s2"] < 1e-3 and e["d"] < 2e-2, e
