"""The bag pool (BagPool, vbmf_set_Y_gather and the training loops' pool= keyword): the parts that need no GPU -- the C ABI is declared,
exported and bound, the Julia host binds it, and the Python host against a context that records what it is asked: a selection is one
Context and one set_Y_gather with the expected index vector and no upload, its shapes are those of the grouped ids, the stand-ins
hold no L x M memory, the training loops draw from the generator in the documented order and make their one batched call on the
selection, and every host refusal comes before the library is touched."""
import ctypes as C
import os
import re
import tracemalloc

import numpy as np
import pytest

import __graft_entry__ as G
from tests.test_fit_split_host import ScriptedCtx

ROOT = G.ROOT
L = 6
MS = [1, 4, 2, 3, 5]
OFF = np.concatenate([[0], np.cumsum(MS)])


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_declares_library_exports_and_hosts_bind(pkg):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vbmf_hip.h")).read(), flags=re.S)
    assert re.search(r"int\s+vbmf_set_Y_gather\s*\(\s*vbmf_ctx\*\s*dst\s*,\s*vbmf_ctx\*\s*src\s*,\s*const\s+int64_t\*\s*col_index\s*,\s*int64_t\s+ncols\s*\)\s*;", hdr)
    cap = pkg.capi
    assert hasattr(C.CDLL(cap.LIB_PATH), "vbmf_set_Y_gather") and "vbmf_set_Y_gather" in cap.SYMBOLS
    assert cap.lib().vbmf_set_Y_gather.argtypes == [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int64]
    assert cap.lib().vbmf_set_Y_gather.restype is C.c_int
    jl = open(os.path.join(G.PKG_DIR, "julia", "VBMatrixFactorizationHIP.jl")).read()
    assert re.search(r"ccall\(\(:vbmf_set_Y_gather,\s*libvbmf\),\s*Cint,\s*\(Ptr\{Cvoid\},\s*Ptr\{Cvoid\},\s*Ptr\{Int64\},\s*Int64\)", jl)
    assert re.search(r"function set_Y_gather!\(", jl) and re.search(r"export[^#]*?set_Y_gather!", jl, flags=re.S)


def test_context_marshals_the_gather(pkg):
    calls = []

    class Lib:
        def vbmf_set_Y_gather(self, dst, src, idx, n):
            calls.append((dst.value, src.value, np.ctypeslib.as_array(idx, shape=(n,)).copy(), n))
            return 0

        def vbmf_destroy(self, h):
            pass
    dst, src = (pkg.capi.Context.__new__(pkg.capi.Context) for _ in range(2))
    dst._h, src._h, dst._lib, src._lib = C.c_void_p(0xD57), C.c_void_p(0x5EC), Lib(), Lib()
    dst.set_Y_gather(src, np.array([4, 0, 4, 2], dtype=np.int32)[::1])
    dst.set_Y_gather(src, [7])
    assert [(c[0], c[1], list(c[2]), c[3]) for c in calls] == [(0xD57, 0x5EC, [4, 0, 4, 2], 4), (0xD57, 0x5EC, [7], 1)]
    assert calls[0][2].dtype == np.int64


# ---- the Python host against a recording context -------------------------------------------------------------------------------------------
class RecCtx:
    """stands where capi.Context stands: records its creation and every call, answers the batched fits with values of its own"""
    log = []

    def __init__(self, Lr, M, H, **kw):
        self.L, self.M, self.H, self.kw, self.device = int(Lr), int(M), int(H), kw, kw.get("device", 0)
        RecCtx.log.append(("create", self, (self.L, self.M, self.H), kw))

    def set_Y(self, Y):
        RecCtx.log.append(("set_Y", self, tuple(Y.shape), str(Y.dtype)))

    def set_Y_rows(self, src, row0=0, nrows=None):
        RecCtx.log.append(("set_Y_rows", self, tuple(src.shape), str(src.dtype)))

    def set_Y_gather(self, src, idx):
        RecCtx.log.append(("set_Y_gather", self, src, np.array(idx)))

    def close(self):
        RecCtx.log.append(("close", self))

    def fit_batched(self, col_off, bag_of, niter, eps, B, SB, CA, CB, s2, **kw):
        RecCtx.log.append(("fit_batched", self, (np.array(col_off), list(bag_of), niter, eps, np.array(B)), kw))
        off, nf, H = np.asarray(col_off), len(bag_of), self.H
        return dict(BHat=np.array(B) + 1.0, SigmaB=np.array(SB), CA=np.array(CA) + 1.0, CB=np.array(CB) + 1.0, sigma2=np.array(s2, dtype=float),
                    SigmaA=np.zeros((nf, H, H)), AHat=[np.full((int(off[b + 1] - off[b]), H), float(f)) for f, b in enumerate(bag_of)],
                    form_used=np.zeros(nf, dtype=np.int64), iters=np.full(nf, niter), d=np.zeros(nf), status=np.zeros(nf, dtype=np.int64))

    def __getattr__(self, name):
        if name.endswith("_fit_batched") or name == "ard_fit_batched_form":
            def call(*a, **kw):
                RecCtx.log.append((name, self, a, kw))
                return ScriptedCtx._answer(None, name, a, kw)
            return call
        raise AttributeError(name)


def _calls(*names):
    return [c for c in RecCtx.log if c[0] in names]


@pytest.fixture
def pool(pkg, monkeypatch):
    monkeypatch.setattr(pkg, "Context", RecCtx)
    RecCtx.log = []
    rng = np.random.default_rng(0)
    pool = pkg.BagPool([rng.standard_normal((L, m)) for m in MS])
    yield pool
    RecCtx.log = []


def test_pool_is_one_rank_one_basic_context_filled_once(pkg, pool):
    (cr,), (sy,) = _calls("create"), _calls("set_Y", "set_Y_rows")
    assert cr[2] == (L, sum(MS), 1) and "variant" not in cr[3] and cr[3]["y_dtype"] == pkg.VBMF_Y_F32
    assert sy[0] == "set_Y" and sy[1] is cr[1] and sy[2] == (L, sum(MS)) and sy[3] == "float64"
    assert (pool.L, pool.Ms, len(pool)) == (L, MS, len(MS)) and np.array_equal(pool.col_off, OFF)
    assert pool.ctx is cr[1]
    pool.close()
    assert _calls("close")[-1][1] is cr[1]


def test_pool_keeps_the_sources_dtype(pkg, monkeypatch):
    import torch
    monkeypatch.setattr(pkg, "Context", RecCtx)
    RecCtx.log = []
    a32 = [np.ones((L, m), dtype=np.float32) for m in MS]
    pkg.BagPool(a32, y_dtype=pkg.VBMF_Y_BF16)
    pkg.BagPool([torch.ones(L, m, dtype=torch.bfloat16) for m in MS])
    pkg.BagPool.from_matrix(np.broadcast_to(np.float32(0.0), (L, sum(MS))), OFF)
    p = pkg.BagPool.from_matrix(np.zeros((L, sum(MS))), OFF)
    assert [(c[0], c[3]) for c in _calls("set_Y", "set_Y_rows")] == [("set_Y_rows", "float32"), ("set_Y_rows", "torch.bfloat16"),
                                                                    ("set_Y_rows", "float32"), ("set_Y", "float64")]
    assert _calls("create")[0][3]["y_dtype"] == pkg.VBMF_Y_BF16 and p.Ms == MS
    for bad in ([0, 3], [0, 3, 3, 15], [1, 15], [0, 16]):
        with pytest.raises(ValueError, match="BagPool.from_matrix: col_off"):
            pkg.BagPool.from_matrix(np.zeros((L, sum(MS))), bad)


@pytest.mark.parametrize("kind", ["basic", "sparse"])
def test_select_is_one_context_and_one_gather(pkg, pool, kind):
    RecCtx.log = []
    groups = [[3, 0], 1, [4], (2, 2, 0)]
    bags = pool.select(groups, 5, kind=kind)
    assert [c[0] for c in RecCtx.log] == ["create", "set_Y_gather"]
    cr, ga = RecCtx.log
    want = np.concatenate([np.arange(OFF[b], OFF[b + 1]) for b in (3, 0, 1, 4, 2, 2, 0)])
    assert ga[1] is cr[1] and ga[2] is pool.ctx and np.array_equal(ga[3], want) and ga[3].dtype == np.int64
    Ms = [MS[3] + MS[0], MS[1], MS[4], 2 * MS[2] + MS[0]]
    assert cr[2] == (L, sum(Ms), 5) and (bags.L, bags.Ms, bags.H, bags.M, len(bags)) == (L, Ms, 5, sum(Ms), 4)
    assert np.array_equal(bags.col_off, np.concatenate([[0], np.cumsum(Ms)])) and bags.col_off.dtype == np.int64
    assert bags.ctx is cr[1]
    if kind == "basic":
        assert isinstance(bags, pkg.Bags) and "variant" not in cr[3]
    else:
        assert isinstance(bags, pkg.SparseBags) and cr[3]["variant"] == pkg.VBMF_VARIANT_SPARSE_DIAG and bags.ctx_kw["y_dtype"] == pkg.VBMF_Y_F32
    bags.close()
    assert RecCtx.log[-1] == ("close", cr[1])


def test_select_and_shapes_allocate_no_matrix(pkg, monkeypatch):
    monkeypatch.setattr(pkg, "Context", RecCtx)
    Lb, Mb, nb = 4096, 10000, 100
    big = pkg.BagPool.from_matrix(np.broadcast_to(np.float32(0.0), (Lb, Mb)), np.arange(0, Mb + 1, Mb // nb))
    groups = [list(range(0, 60)), list(range(40, 100))]
    tracemalloc.start()
    try:
        sh = big.shapes(groups)
        bags = big.select(groups, 4, kind="sparse")
        peak = tracemalloc.get_traced_memory()[1]
    finally:
        tracemalloc.stop()
    assert [s.shape for s in sh] == [(Lb, 6000), (Lb, 6000)] and all(s.strides == (0, 0) and not s.flags.writeable for s in sh)
    assert bags.M == 12000 and peak < Lb * 8 * 100                  # index vectors of M entries; an L x M fp64 matrix is 393 MB
    assert [s.shape for s in big.shapes([[], 3])] == [(Lb, 0), (Lb, 100)]


def test_host_refusals_come_before_the_library(pkg, pool):
    RecCtx.log = []
    for call, word in ((lambda: pool.select([[0, 5]], 3), r"BagPool.select: group 0: bag id 5 outside 0\.\.4"),
                       (lambda: pool.select([1, [-1]], 3), r"BagPool.select: group 1: bag id -1 outside"),
                       (lambda: pool.select([1, []], 3), r"BagPool.select: group 1 is empty"),
                       (lambda: pool.select([], 3), r"BagPool.select: no groups"),
                       (lambda: pool.select([1], 3, kind="dual"), r"BagPool.select: kind = 'dual'"),
                       (lambda: pool.select([1], 65), r"BagPool.select: H = 65 > 64"),
                       (lambda: pool.shapes([[9]]), r"BagPool.shapes: group 0: bag id 9 outside"),
                       (lambda: pkg.BagPool([np.zeros((L, 2)), np.zeros((L + 1, 2))]), r"BagPool: the bags have different row counts L \[6, 7\]"),
                       (lambda: pkg.BagPool([np.zeros((L, 2)), np.zeros((L, 0))]), r"BagPool: every bag must be a matrix with at least one column"),
                       (lambda: pkg.BagPool([]), r"BagPool: no bags"),
                       (lambda: pkg.train_folds([([0], [7])], "basic", 3, 5, pool=pool), r"train_folds: group 1: bag id 7 outside"),
                       (lambda: pkg.train_folds([([0], [1])], "basic", 33, 5, pool=pool), r"train_folds: H = 33 > 32"),
                       (lambda: pkg.train_dual_folds([([0], [1])], 3, 1, 5, pool=pool.ctx), r"train_dual_folds: pool is a RecCtx"),
                       (lambda: pkg.train_local_folds([([0], [8])], 3, 1, 5, pool=pool), r"train_local_folds: group 1: bag id 8 outside"),
                       (lambda: pkg.train_local_folds([([], [])], 3, 1, 5, pool=pool), r"train_local_folds: group 0 is empty")):
        with pytest.raises(ValueError, match=word):
            call()
    assert RecCtx.log == []
    pool.close()
    RecCtx.log = []
    for call, fn in ((lambda: pool.select([1], 3), "BagPool.select"), (lambda: pool.shapes([1]), "BagPool.shapes"),
                     (lambda: pkg.train_folds([([0], [1])], "sparse", 3, 5, pool=pool), "train_folds"),
                     (lambda: pkg.train_dual_folds([([0], [1])], 3, 1, 5, pool=pool), "train_dual_folds"),
                     (lambda: pkg.train_local_folds([([0], [1])], 3, 1, 5, pool=pool), "train_local_folds")):
        with pytest.raises(ValueError, match=fn + ": the pool is closed"):
            call()
    assert RecCtx.log == []


# ---- the training loops ----------------------------------------------------------------------------------------------------------------------
FOLDS = [([0, 1], [2, 3, 4]), ([4], []), ([3, 2], 1)]                # the middle fold has an empty class
H = 3


def test_train_folds_draws_in_order_and_makes_one_call(pkg, pool):
    for solver, entry, nstarts in (("basic", "fit_batched", 1), ("sparse", "sparse_fit_batched", 10)):
        RecCtx.log = []
        out = pkg.train_folds(FOLDS, solver, H, 7, rng=np.random.default_rng(5), pool=pool)
        assert [c[0] for c in RecCtx.log] == ["create", "set_Y_gather", entry, "close"]
        cr, ga, call, _ = RecCtx.log
        groups = [[0, 1], [2, 3, 4], [3, 2], [1]]                   # (fold, class), the fold with an empty class left out
        assert np.array_equal(ga[3], np.concatenate([np.arange(OFF[b], OFF[b + 1]) for g in groups for b in g])) and ga[2] is pool.ctx
        Ms = [sum(MS[b] for b in g) for g in groups]
        assert call[1] is cr[1] and cr[2] == (L, sum(Ms), H)
        rng, init = np.random.default_rng(5), (pkg.vbmf_init if solver == "basic" else pkg.vbmf_sparse_init)
        want = [init(np.zeros((L, m)), H, rng=rng) for m in Ms for _ in range(nstarts)]     # the matrix-pair path's draws
        if solver == "basic":
            col_off, bag_of, niter, eps, B = call[2]
        else:
            col_off, bag_of, niter, eps, B = call[2][0], call[2][1], call[2][2], call[2][3], call[2][9]
        assert np.array_equal(col_off, np.concatenate([[0], np.cumsum(Ms)])) and list(bag_of) == [b for b in range(4) for _ in range(nstarts)]
        assert niter == 7 and np.array_equal(np.asarray(B), np.stack([p.BHat for p in want]))
        assert out[1] == (0, 0) and all(type(p) is type(want[0]) for k in (0, 2) for p in out[k])
        assert [p.M for k in (0, 2) for p in out[k]] == Ms


def test_train_dual_and_local_folds_draw_in_order_and_make_one_call(pkg, pool):
    RecCtx.log = []
    out = pkg.train_dual_folds(FOLDS, H, 1, 7, nstarts=2, rng=np.random.default_rng(6), pool=pool)
    assert [c[0] for c in RecCtx.log] == ["create", "set_Y_gather", "sparse_fit_batched", "close"]
    Ms = [5, 10, 5, 4]
    rng = np.random.default_rng(6)
    want = [pkg.vbmf_dual_init(np.zeros((L, m)), H, 1, rng=rng) for m in Ms for _ in range(2)]
    a = RecCtx.log[2][2]
    assert np.array_equal(np.asarray(a[9]), np.stack([p.BHat for p in want])) and list(a[1]) == [0, 0, 1, 1, 2, 2, 3, 3]
    assert out[1] == (0, 0) and [p.M for k in (0, 2) for p in out[k]] == Ms
    RecCtx.log = []
    folds = [([0, 1], [2, 3, 4]), ([], [4]), ([3, 2], 1)]            # (an empty class 0 is a fit without labels)
    ps = pkg.train_local_folds(folds, H, 1, 7, rng=np.random.default_rng(7), pool=pool)
    assert [c[0] for c in RecCtx.log] == ["create", "set_Y_gather", "local_fit_batched", "close"]
    cr, ga, call, _ = RecCtx.log
    groups = [[0, 1, 2, 3, 4], [4], [3, 2, 1]]                      # group 0 followed by group 1
    assert np.array_equal(ga[3], np.concatenate([np.arange(OFF[b], OFF[b + 1]) for g in groups for b in g]))
    Ms, M0s = [15, 5, 9], [5, 0, 5]
    rng = np.random.default_rng(7)
    want = [pkg.vbmf_sparse_init(np.zeros((L, m)), H, H1=1, labels=np.arange(1, m0 + 1), rng=rng) for m, m0 in zip(Ms, M0s)]
    a, kw = call[2], call[3]
    assert np.array_equal(a[0], np.concatenate([[0], np.cumsum(Ms)])) and list(a[1]) == [0, 1, 2] and list(a[14]) == M0s and kw["mask_H1"] == 1
    assert np.array_equal(np.asarray(a[9]), np.stack([p.BHat for p in want]))
    assert [(p.M, list(p.labels)) for p in ps] == [(m, list(range(1, m0 + 1))) for m, m0 in zip(Ms, M0s)]


def test_pool_none_is_the_list_path(pkg, pool, monkeypatch):
    """without a pool the loops upload their matrices as they always did: a Bags / SparseBags from the list, no gather"""
    rng = np.random.default_rng(1)
    folds = [(rng.standard_normal((L, 3)), rng.standard_normal((L, 4)))]
    RecCtx.log = []
    pkg.train_folds(folds, "basic", H, 5, rng=np.random.default_rng(2))
    pkg.train_dual_folds(folds, H, 1, 5, nstarts=2, rng=np.random.default_rng(2))
    assert [c[0] for c in RecCtx.log] == ["create", "set_Y", "fit_batched", "close", "create", "set_Y", "sparse_fit_batched", "close"]
