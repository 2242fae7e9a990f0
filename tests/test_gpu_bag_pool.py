"""The bag pool on the GPU: a data set uploaded once (BagPool), a call's bags gathered on the device (vbmf_set_Y_gather).

The gather must leave a context EXACTLY as vbmf_set_Y leaves it when given the pool's stored values at the chosen columns: both tiled
copies bit for bit over the whole buffers (pad tiles included), get_Y bit for bit, and -- because the gather runs tile_y_kernel on
vbmf_set_Y's own grids and column chunks, so the partials of ||Y||^2 have the same shape and order -- trYY EQUAL (the figure against
the looser bound of tests/test_gpu_set_y_sources.py, relative L M 2^-52, is printed first).  Everything a batched function computes
from a selection therefore equals, bit for bit, what it computes from the same matrices as a list: both routes round the same
float64 values once to the same storage, and no batched call used here reads the context-wide ||Y||^2.

Shapes: L = 130 (not a multiple of 32), seven bags of widths 1, 31, 32, 33, 7, 64, 2 (170 columns: bag edges on both sides of the
32-column tile edges and of the 8- and 16-column k-steps), H = 5.

The refusal "src on another device" needs a second GPU: it is asserted where torch sees one and cannot be reached otherwise.

The ARD initialisers store trYTY = sum(Y .* Y) of the matrix they are given, a field nothing in the package reads; with a pool they
are given a stand-in of zeros (BagPool.shapes), so the training loops' sets carry trYTY = 0.  That field is the one exception to
"every field bit for bit" in the fold tests below."""
import copy
import ctypes as C
import dataclasses
import re

import numpy as np
import pytest

import __graft_entry__ as G
from tests.test_gpu_gram_sparse import _ctx as gram_ctx, _set as gram_set
from tests.test_gram_sparse_identity import problem

pytestmark = pytest.mark.gpu

L, H = 130, 5
MS = [1, 31, 32, 33, 7, 64, 2]
OFF = np.concatenate([[0], np.cumsum(MS)])
SELECTIONS = {
    "identity": [0, 1, 2, 3, 4, 5, 6],
    "reversed": [6, 5, 4, 3, 2, 1, 0],
    "width 33": [0, 2],
    "width 95": [1, 5],
    "one column": [0],
    "a bag twice": [4, 5, 4],
    "wider than the pool": [0, 1, 2, 3, 4, 5, 6, 5, 3, 1],
}


@pytest.fixture(scope="module")
def pkg():
    G.build()
    p = G.load_package()
    p.set_defaults(y_dtype=p.VBMF_Y_F32, factor_dtype=p.VBMF_FACTOR_AUTO)
    yield p
    p.set_defaults(y_dtype=p.VBMF_Y_F32, factor_dtype=p.VBMF_FACTOR_AUTO)


def _bags(seed=3):
    """low-rank bags with noise, float64"""
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((L, 4)) * np.linspace(1.0, 2.0, 4)
    return [B @ rng.standard_normal((4, m)) + 0.1 * rng.standard_normal((L, m)) for m in MS]


def _cols(ids):
    return np.concatenate([np.arange(OFF[b], OFF[b + 1]) for b in ids])


def _snapshot(pkg, c):
    d = c.dims()
    return dict(Y1=c.peek(pkg.capi.PEEK_Y1, d["XT1"] * d["KS1"] * 64 * 4), Y2=c.peek(pkg.capi.PEEK_Y2, d["XT2"] * d["KS2"] * 64 * 4),
                Y=c.get_Y(), tr=c.trYY())


def _same(got, want, Lr, M, what, exact=True):
    for k in ("Y1", "Y2"):
        assert np.array_equal(got[k], want[k]), (what, k, int(np.sum(got[k] != want[k])))
    assert np.array_equal(got["Y"].view(np.uint64), want["Y"].view(np.uint64)), (what, "get_Y")
    bound = Lr * M * 2.0 ** -52
    rel = abs(got["tr"] - want["tr"]) / want["tr"]
    print(f"{what}: trYY rel {rel:.3e} (bound {bound:.3e})")
    assert rel <= bound, (what, rel, bound)
    if exact:                                                       # the same partials in the same order
        assert got["tr"] == want["tr"], (what, got["tr"], want["tr"])


def _ydt(pkg, y):
    return pkg.VBMF_Y_F32 if y == "f32" else pkg.VBMF_Y_BF16


_pools = {}


def _pool(pkg, y):
    """the pool of the seven bags in storage y and the float64 matrix of its stored values: made once, shared, never changed"""
    if y not in _pools:
        pool = pkg.BagPool(_bags(), y_dtype=_ydt(pkg, y))
        stored = pool.ctx.get_Y()
        stored.setflags(write=False)
        _pools[y] = (pool, stored)
    return _pools[y]


# ---- 1. the stored bits ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SELECTIONS))
@pytest.mark.parametrize("y", ["f32", "bf16"])
def test_gather_leaves_what_set_Y_leaves(pkg, y, name):
    pool, stored = _pool(pkg, y)
    idx = _cols(SELECTIONS[name])
    M = idx.size
    with pkg.capi.Context(L, M, H, y_dtype=_ydt(pkg, y)) as dst, pkg.capi.Context(L, M, H, y_dtype=_ydt(pkg, y)) as ref:
        ref.set_Y(stored[:, idx])
        dst.set_Y_gather(pool.ctx, idx)
        _same(_snapshot(pkg, dst), _snapshot(pkg, ref), L, M, f"{y} {name}")
        dst.set_Y_gather(pool.ctx, idx[::-1])                            # a second gather on a context that holds a Y
        ref.set_Y(stored[:, idx[::-1]])
        _same(_snapshot(pkg, dst), _snapshot(pkg, ref), L, M, f"{y} {name}, then its mirror")
    assert np.array_equal(pool.ctx.get_Y().view(np.uint64), stored.view(np.uint64))       # src is only read


@pytest.mark.parametrize("name", ["width 95", "a bag twice"])
def test_gather_into_a_row_noise_context(pkg, name):
    """a VBMF_VARIANT_SPARSE_DIAGVAR pair: the tiles, and one diag_var sweep from the same state -- which reads the per-row norms"""
    cap = pkg.capi
    pool, stored = _pool(pkg, "f32")
    idx = _cols(SELECTIONS[name])
    M = idx.size
    Yg = np.asfortranarray(stored[:, idx])
    p = pkg.vbmf_sparse_init(Yg, H, ca=0.1, cb=0.1, sigma=0.1, rng=np.random.default_rng(9))
    hyper = dict(alpha0=p.alpha0, beta0=p.beta0, gamma0=p.gamma0, delta0=p.delta0, eta0=p.eta0, zeta0=p.zeta0)
    out = []
    for gather in (True, False):
        with cap.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32, variant=cap.VBMF_VARIANT_SPARSE_DIAGVAR) as c:
            if gather:
                c.set_Y_gather(pool.ctx, idx)
            else:
                c.set_Y(Yg)
            snap = _snapshot(pkg, c)
            c.sparse_set_state(p.ATVecHat, p.diagSigmaATVec, p.CA, p.beta, p.BHat, p.SigmaB, p.CB, p.delta, p.sigmaHat, p.zeta, hyper)
            c.sparse_set_noise_rows(np.ones(L), 1e-10 * np.ones(L), 1e-10 + M / 2)
            it, d, _ = c.sparse_run(1, eps=0.0, est_cb=True)
            assert it == 1 and np.isfinite(d)
            out.append((snap, c.sparse_get_state(), c.sparse_get_noise_rows(), d))
    (sg, stg, ng, dg), (sr, str_, nr, dr) = out
    _same(sg, sr, L, M, f"diag_var {name}")
    for k, v in str_.items():
        assert np.array_equal(np.asarray(stg[k]), np.asarray(v)), k
    assert np.array_equal(ng[0], nr[0]) and np.array_equal(ng[1], nr[1]) and dg == dr
    assert np.all(np.isfinite(ng[0])) and not np.array_equal(ng[0], np.ones(L))         # the row update ran


# ---- 2. derived data are dropped ---------------------------------------------------------------------------------------------------------
def test_gather_drops_what_was_made_from_the_old_Y(pkg, monkeypatch):
    cap = pkg.capi
    Lg, Mg, Hg = 2464, 352, 32
    Y, po = problem(Lg, Mg, Hg, 540)
    idx = np.arange(Mg)[::-1].copy()
    idx[:7] = 100                                                    # a permutation with a repeated column
    with cap.Context(Lg, Mg, 1, y_dtype=pkg.VBMF_Y_BF16) as src:
        src.set_Y(Y)
        stored = src.get_Y()
        with gram_ctx(pkg, monkeypatch, Lg, Mg, Hg, True) as c:
            c.set_Y(Y)
            gram_set(c, po)
            it, _, _ = c.sparse_run(2, eps=0.0)
            assert it == 2 and c.dims()["gram"] == 1 and c.dims()["gram_built"] == 1
            c.set_Y_gather(src, idx)
            assert c.dims()["gram_built"] == 0
            gram_set(c, po)
            it, dg, _ = c.sparse_run(2, eps=0.0)
            assert it == 2 and c.dims()["gram_built"] == 1
            got = c.sparse_get_state()
        with gram_ctx(pkg, monkeypatch, Lg, Mg, Hg, True) as f:
            f.set_Y(stored[:, idx])
            gram_set(f, po)
            it, df, _ = f.sparse_run(2, eps=0.0)
            assert it == 2 and f.dims()["gram_built"] == 1
            want = f.sparse_get_state()
    assert dg == df
    for k, v in want.items():
        assert np.array_equal(np.asarray(got[k]), np.asarray(v)), k


# ---- 3. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_dst_untouched(pkg):
    import torch
    cap = pkg.capi
    INVALID, UNSUPPORTED = cap.VBMF_ERR_INVALID, cap.VBMF_ERR_UNSUPPORTED
    pool, stored = _pool(pkg, "f32")
    pool16, _ = _pool(pkg, "bf16")
    src = pool.ctx
    M = 33
    good = _cols([3])
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    rng = np.random.default_rng(4)
    Y0 = rng.standard_normal((L, M))
    high, neg = good.copy(), good.copy()
    high[17], neg[32] = 170, -1
    lib = cap.lib()
    with cap.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32) as dst, cap.Context(L + 1, 170, 1, y_dtype=pkg.VBMF_Y_F32) as tall, \
            cap.Context(L, 170, 1, y_dtype=pkg.VBMF_Y_F32) as fresh, cap.Context(L, 170, 1, y_dtype=pkg.VBMF_Y_F32) as partial, \
            cap.Context(L, 170, 1, y_dtype=pkg.VBMF_Y_F32, nranks=2, rank=0, L_global=2 * L) as shard, \
            cap.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32, nranks=2, rank=0, L_global=2 * L) as shard_dst:
        dst.set_Y(Y0)
        tall.set_Y(rng.standard_normal((L + 1, 170)))
        partial.set_Y_rows(np.asarray(stored[:64], dtype=np.float32), 0)                # in the middle of a row-block upload
        want = _snapshot(pkg, dst)
        cases = {
            "NULL src": (dst._h, None, ptr(good), M, INVALID, "NULL src"),
            "NULL col_index": (dst._h, src._h, None, M, INVALID, "NULL col_index"),
            "dst == src": (dst._h, dst._h, ptr(good), M, INVALID, "same context"),
            "ncols != M": (dst._h, src._h, ptr(good), M - 1, INVALID, "ncols = 32, dst has M = 33"),
            "another L": (dst._h, tall._h, ptr(good), M, INVALID, "src has L = 131 rows, dst has L = 130"),
            "another y_dtype": (dst._h, pool16.ctx._h, ptr(good), M, INVALID, "y_dtype"),
            "a fresh src": (dst._h, fresh._h, ptr(good), M, INVALID, "src has no complete Y"),
            "src in a row-block upload": (dst._h, partial._h, ptr(good), M, INVALID, "src has no complete Y"),
            "index = src's M": (dst._h, src._h, ptr(high), M, INVALID, r"col_index\[17\] = 170 outside 0..169"),
            "index -1": (dst._h, src._h, ptr(neg), M, INVALID, r"col_index\[32\] = -1 outside 0..169"),
            "a row-sharded src": (dst._h, shard._h, ptr(good), M, UNSUPPORTED, "row-sharded"),
        }
        if torch.cuda.device_count() > 1:
            other = cap.Context(L, 170, 1, y_dtype=pkg.VBMF_Y_F32, device=1)
            other.set_Y(np.asarray(stored))
            cases["another device"] = (dst._h, other._h, ptr(good), M, INVALID, "src lives on device 1, dst on device 0")
        for name, (d, s, i, n, code, text) in cases.items():
            rc = lib.vbmf_set_Y_gather(d, s, i, n)
            msg = lib.vbmf_last_error(dst._h).decode()
            assert rc == code, (name, rc, msg)
            assert "vbmf_set_Y_gather" in msg and re.search(text, msg), (name, msg)
            _same(_snapshot(pkg, dst), want, L, M, f"after the refusal '{name}'")
        if torch.cuda.device_count() > 1:
            other.close()
        assert lib.vbmf_set_Y_gather(None, src._h, ptr(good), M) == INVALID
        assert "vbmf_set_Y_gather: NULL dst" in lib.vbmf_last_error(None).decode()
        rc = lib.vbmf_set_Y_gather(shard_dst._h, src._h, ptr(good), M)
        assert rc == UNSUPPORTED and "row-sharded" in lib.vbmf_last_error(shard_dst._h).decode()
        # a dst in the middle of a row-block upload stays there: the block that is due is still accepted and completes the same Y
        with cap.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32) as mid:
            mid.set_Y_rows(Y0[:64], 0)
            assert lib.vbmf_set_Y_gather(mid._h, src._h, ptr(high), M) == INVALID
            with pytest.raises(pkg.VbmfError, match="no Y"):
                mid.get_Y()
            mid.set_Y_rows(Y0[64:], 64)
            _same(_snapshot(pkg, mid), want, L, M, "row blocks around a refused gather")
            mid.set_Y_rows(Y0[:64], 0)                               # ... and an accepted gather abandons the upload
            mid.set_Y_gather(src, good)
            with cap.Context(L, M, H, y_dtype=pkg.VBMF_Y_F32) as ref:
                ref.set_Y(stored[:, good])
                _same(_snapshot(pkg, mid), _snapshot(pkg, ref), L, M, "a gather over an abandoned upload")
            with pytest.raises(pkg.VbmfError, match="order"):
                mid.set_Y_rows(Y0[64:], 64)
        torch.cuda.synchronize()


# ---- 4. end to end: a selection against the same matrices as a list -----------------------------------------------------------------------------
GROUPS = [[0, 1], 2, [3], [6, 4], [5, 0]]                            # widths 32, 32, 33, 9, 65


def _matrices(bags, groups=GROUPS):
    return [np.concatenate([bags[b] for b in (g if isinstance(g, list) else [g])], axis=1) for g in groups]


def _same_params(a, b, what, skip=()):
    assert type(a) is type(b)
    names = [f.name for f in dataclasses.fields(a)] + ["iters", "status", "d", "form", "form_used"]
    seen = 0
    for n in names:
        if n in skip or not hasattr(b, n):
            continue
        va, vb = getattr(a, n), getattr(b, n)
        if vb is None:
            assert va is None, (what, n)
            continue
        assert np.array_equal(np.asarray(va), np.asarray(vb), equal_nan=True), (what, n)
        seen += 1
    assert seen >= 10, (what, seen)


def test_batched_calls_on_a_selection_equal_the_list_path(pkg):
    bags = _bags()
    Ys = _matrices(bags)
    pool = pkg.BagPool(bags)
    basic, sparse = pool.select(GROUPS, H), pool.select(GROUPS, H, kind="sparse")
    try:
        assert basic.Ms == [Y.shape[1] for Y in Ys] == sparse.Ms
        # vbmf_batch_: 6 sweeps, eps = 0
        p0 = [pkg.vbmf_init(Y, H, ca=0.1, cb=0.1, sigma2=0.1, rng=np.random.default_rng(20 + k)) for k, Y in enumerate(Ys)]
        pl, pp = copy.deepcopy(p0), copy.deepcopy(p0)
        pkg.vbmf_batch_(Ys, pl, 6, eps=0.0, est_covs=True, est_var=True)
        pkg.vbmf_batch_(basic, pp, 6, eps=0.0, est_covs=True, est_var=True)
        for k, (a, b) in enumerate(zip(pp, pl)):
            assert b.iters == 6 and b.status == 0 and not np.array_equal(b.AHat, p0[k].AHat)
            _same_params(a, b, f"vbmf_batch_ fit {k}")
        # vbmf_sparse_batch_, one workgroup per fit and split over many
        s0 = [pkg.vbmf_sparse_init(Y, H, ca=0.1, cb=0.1, sigma=0.1, rng=np.random.default_rng(30 + k)) for k, Y in enumerate(Ys)]
        for kw in (dict(form="stream"), dict(form="split", slice_cols=8)):
            sl, sp = copy.deepcopy(s0), copy.deepcopy(s0)
            dl = pkg.vbmf_sparse_batch_(Ys, sl, 6, eps=0.0, **kw)
            dp = pkg.vbmf_sparse_batch_(sparse, sp, 6, eps=0.0, **kw)
            assert dl == dp and all(np.isfinite(dl))
            for k, (a, b) in enumerate(zip(sp, sl)):
                assert b.iters == 6 and b.status == 0 and b.form == (3 if kw["form"] == "split" else 0)
                _same_params(a, b, f"vbmf_sparse_batch_ {kw} fit {k}")
        # vbls_batch_ with the basis of fit 2
        ql = [pkg.copy_vbmf_params(Y, pl[2], rng=np.random.default_rng(40 + k)) for k, Y in enumerate(Ys)]
        qp = copy.deepcopy(ql)
        Al, Ap = pkg.vbls_batch_(Ys, ql, 10), pkg.vbls_batch_(basic, qp, 10)
        for k, (a, b) in enumerate(zip(qp, ql)):
            assert np.array_equal(Ap[k], Al[k]) and np.all(np.isfinite(Al[k]))
            _same_params(a, b, f"vbls_batch_ bag {k}")
        # classify_bags("ols"): one upload, two bases
        for up in (basic, sparse):
            rl, rp = pkg.classify_bags(pl[0], pl[3], Ys, "ols"), pkg.classify_bags(pl[0], pl[3], up, "ols")
            for a, b in zip(rp, rl):
                assert np.array_equal(a, b) and np.all(np.isfinite(b))
    finally:
        basic.close()
        sparse.close()
        pool.close()


# ---- 5. a pool from a non-fp64 source ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("y", ["f32", "bf16"])
def test_pool_from_float32_gpu_tensors_equals_the_pool_from_float64(pkg, y):
    import torch
    t = [torch.from_numpy(b).float().cuda() for b in _bags()]
    a = [x.double().cpu().numpy() for x in t]                       # the float64 arrays of exactly those values
    pt, pa = pkg.BagPool(t, y_dtype=_ydt(pkg, y)), pkg.BagPool(a, y_dtype=_ydt(pkg, y))
    pm = pkg.BagPool.from_matrix(torch.cat(t, dim=1).t().contiguous().t(), OFF, y_dtype=_ydt(pkg, y))    # one column-major matrix
    try:
        _same(_snapshot(pkg, pt.ctx), _snapshot(pkg, pa.ctx), L, 170, f"{y} pools", exact=False)     # two upload routes
        for kind in ("basic", "sparse"):
            sels = [p.select(GROUPS, H, kind=kind) for p in (pt, pa, pm)]
            try:
                snaps = [_snapshot(pkg, s.ctx) for s in sels]
                _same(snaps[0], snaps[1], L, sels[0].M, f"{y} {kind} selections")
                _same(snaps[2], snaps[1], L, sels[0].M, f"{y} {kind} selections, from_matrix")
            finally:
                for s in sels:
                    s.close()
    finally:
        for p in (pt, pa, pm):
            p.close()
        torch.cuda.synchronize()


# ---- 6. the training loops ----------------------------------------------------------------------------------------------------------------------
FOLDS = [([0, 1, 2], [3, 4]), ([5], [6, 0]), ([1], []), ([2, 3], [1, 4, 5])]     # three folds of the seven bags and one with an empty class


def _pairs(bags):
    cat = lambda g: np.concatenate([bags[b] for b in g], axis=1) if g else np.zeros((L, 0))
    return [(cat(g0), cat(g1)) for g0, g1 in FOLDS]


def _same_folds(got, want, what, skip=()):
    assert len(got) == len(want) == len(FOLDS)
    for k, (a, b) in enumerate(zip(got, want)):
        if k == 2:
            assert a == (0, 0) and b == (0, 0), what
            continue
        for c in (0, 1):
            _same_params(a[c], b[c], f"{what} fold {k} class {c}", skip)


@pytest.mark.parametrize("solver", ["basic", "sparse"])
def test_train_folds_on_a_pool(pkg, solver):
    bags = _bags()
    with pkg.BagPool(bags) as pool:
        got = pkg.train_folds(FOLDS, solver, H, 5, rng=np.random.default_rng(50), pool=pool)
    want = pkg.train_folds(_pairs(bags), solver, H, 5, rng=np.random.default_rng(50))
    assert all(np.all(np.isfinite(p.AHat)) for k in (0, 1, 3) for p in want[k])
    _same_folds(got, want, f"train_folds {solver}", skip=("trYTY",))


def test_train_dual_folds_on_a_pool(pkg):
    bags = _bags()
    with pkg.BagPool(bags) as pool:
        got = pkg.train_dual_folds(FOLDS, H, 2, 5, nstarts=2, rng=np.random.default_rng(51), pool=pool)
    want = pkg.train_dual_folds(_pairs(bags), H, 2, 5, nstarts=2, rng=np.random.default_rng(51))
    _same_folds(got, want, "train_dual_folds", skip=("trYTY",))


def test_train_local_folds_on_a_pool(pkg):
    bags = _bags()
    folds = [f for k, f in enumerate(FOLDS) if k != 2]
    pairs = [f for k, f in enumerate(_pairs(bags)) if k != 2]
    with pkg.BagPool(bags) as pool:
        got = pkg.train_local_folds(folds, H, 2, 5, rng=np.random.default_rng(52), pool=pool)
    want = pkg.train_local_folds(pairs, H, 2, 5, rng=np.random.default_rng(52))
    assert len(got) == len(want) == 3
    for k, (a, b) in enumerate(zip(got, want)):
        assert b.M == sum(MS[i] for g in folds[k] for i in g) and list(b.labels) == list(range(1, sum(MS[i] for i in folds[k][0]) + 1))
        _same_params(a, b, f"train_local_folds fold {k}", skip=("trYTY",))
