"""vbls! for a list of (bag, model) jobs in one device call (vbmf_sparse_fixed_basis_jobs, Context.sparse_fixed_basis_jobs): every
output field of every job against fp64 (the oracle's updateA! / updateCA! / updateSigma! loop; where its dense M_b H x M_b H inverse
is too large the block-wise ref_vbls that tests/test_vbls_jobs_host.py pins to it), the residual against NumPy on the device's own A,
the segmentation properties bit for bit, the isolation of a failed job, and the C ABI's refusals.

Shapes: L = 33 and 300 (odd; above one 256-row stage), H = 1, 5, 16, 17, 32 (the 16-block edge), 20 iterations, bags of 1, 3, 2, 7, 8,
9, 17, 64 and 70 columns and, from the placement rule itself (vbmf_debug_vbls_jobs_lds_cols), the widest bag whose state stays in LDS
at that H and form and one column more; a sparse and a dual model per call (three in the segmentation tests).  Y is rounded to fp32
and stored as fp32, so that Y as stored is Y; one bf16-storage case compares on vbmf_get_Y's values.

Bounds.  Against fp64 every field is held to 3 x the error measured on an MI355X (the project's rule), worst over this file's cases
per form; TOL below carries the measured values.  Both sides are fp64 evaluations of one recurrence on the same operands, so the
errors are summation-order movement amplified by the recurrence; none is looser than what tests/test_gpu_vbls_sparse_batch.py holds
the one-basis entry to (its TOL, asserted below).  The residual is held to RESID_TOL = 1e-10 of tests/test_gpu_bag_scoring.py.
"""
import functools

import numpy as np
import pytest

import __graft_entry__ as G
from tests.helpers import relF, report
from tests.test_gpu_bag_scoring import RESID_TOL
from tests.test_gpu_vbls_sparse_batch import TOL as TOL_ONE_BASIS
from tests.test_vbls_jobs_host import FIELDS, model_arrays, oracle_vbls, ref_vbls, trained

pytestmark = pytest.mark.gpu

NITER = 20
WIDTHS = [1, 3, 2, 7, 8, 9, 17, 64, 70]
DENSE_MAX = 300          # the oracle's dense full_cov inverse up to this M_b H; the block-wise reference above it
# measured on an MI355X, worst over the 22 cases of test_against_fp64 and test_against_fp64_bf16_storage (the reference works on Y as
# stored, so the storage does not enter); sigmaHat, zeta, SigmaA and diagSigmaATVec move together, as in the one-basis entry:
# zeta = zeta0 + ||Y||^2 / 2 - sum P o A + ... cancels, and every dS carries sigmaHat's error
MEASURED = {False: dict(ATVecHat=3.20e-15, diagSigmaATVec=1.15e-12, CA=5.46e-15, beta=3.26e-15, SigmaA=1.15e-12, sigmaHat=1.15e-12,
                        zeta=1.15e-12),
            True: dict(ATVecHat=3.56e-15, diagSigmaATVec=1.35e-12, CA=4.87e-13, beta=3.74e-15, SigmaA=1.35e-12, sigmaHat=1.35e-12,
                       zeta=1.35e-12)}
# (r2 against NumPy on the device's own A measured 3.1e-15; it is held to RESID_TOL)
TOL = {full: {f: 3 * v for f, v in m.items()} for full, m in MEASURED.items()}

def test_no_bound_is_looser_than_the_one_basis_entry_s():
    for full in (False, True):
        for f in FIELDS:
            assert TOL[full][f] <= TOL_ONE_BASIS[full][f], (full, f)


@pytest.fixture(scope="module")
def pkg():
    G.build()
    p = G.load_package()
    p.set_defaults(y_dtype=p.VBMF_Y_F32, factor_dtype=p.VBMF_FACTOR_AUTO)
    yield p
    p.invalidate()
    p.set_defaults(y_dtype=p.VBMF_Y_F32, factor_dtype=p.VBMF_FACTOR_AUTO)


def _f32(Y):
    return Y.astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _models(L, H):
    """a sparse and a dual set trained by the oracle, and a sampler per model; computed once and left unchanged"""
    return [trained(kind, L, H, 4000 + 10 * H + k + L) for k, kind in enumerate(("sparse", "dual"))]


def _upload(pkg, Ys, storage="f32"):
    C = pkg.capi
    off = np.concatenate([[0], np.cumsum([Y.shape[1] for Y in Ys])]).astype(np.int64)
    c = C.Context(Ys[0].shape[0], int(off[-1]), 1, y_dtype=C.VBMF_Y_BF16 if storage == "bf16" else C.VBMF_Y_F32)
    c.set_Y(np.asfortranarray(np.hstack(Ys)))
    return c, off


def _block(r, j, f):
    if f in ("sigmaHat", "zeta"):
        return float(r[f][j])
    if f == "SigmaA":
        return r[f][j]
    return r[f][r["off"][j]:r["off"][j + 1]]


def _job_equal(ra, ja, rb, jb):
    return all(np.array_equal(_block(ra, ja, f), _block(rb, jb, f)) for f in FIELDS) and ra["r2"][ja] == rb["r2"][jb] \
        and ra["status"][ja] == rb["status"][jb]


# ---- 1. against fp64, and the residual ---------------------------------------------------------------------------------------------
def _against_fp64(pkg, L, H, full, storage):
    lds = pkg.capi.vbls_jobs_lds_cols(H, full)
    assert lds >= 1
    widths = WIDTHS + [lds, lds + 1]
    if not full:
        widths = [w for w in widths if w > 1]                          # (the QS1 layout of the diagonal form needs M >= 2)
    mods = _models(L, H)
    rng = np.random.default_rng(77 + H)
    Ys = [mods[b % 2][1](w) for b, w in enumerate(widths)]
    Ys = [_f32(Y) if storage == "f32" else Y for Y in Ys]
    jobs = [(b, k) for b in range(len(Ys)) for k in range(2)]
    jobs = [jobs[i] for i in rng.permutation(len(jobs))]
    arrays = [model_arrays(po) for po, _ in mods]
    c, off = _upload(pkg, Ys, storage)
    with c:
        Yst = c.get_Y()
        r = c.sparse_fixed_basis_jobs(off, H, arrays, [b for b, _ in jobs], [k for _, k in jobs], NITER, full_cov=full)
    Ysts = [Yst[:, off[b]:off[b + 1]] for b in range(len(Ys))]
    if storage == "f32":
        assert all(np.array_equal(a, b) for a, b in zip(Ysts, Ys))
    assert not r["status"].any()
    worst, resid = {f: 0.0 for f in FIELDS}, 0.0
    for j, (b, k) in enumerate(jobs):
        Y, po = Ysts[b], mods[k][0]
        if full and Y.shape[1] * H > DENSE_MAX:
            want = ref_vbls(Y, arrays[k], NITER, True)
        else:
            q = oracle_vbls(pkg, Y, po, NITER, full, seed=j)
            want = {f: getattr(q, f) for f in FIELDS}
        for f in FIELDS:
            a, o = _block(r, j, f), want[f]
            worst[f] = max(worst[f], abs(a - o) / abs(o) if np.isscalar(o) else relF(a, o))
        A = _block(r, j, "ATVecHat").reshape(Y.shape[1], H)
        r2 = float(np.sum((Y - po.BHat @ A.T) ** 2))
        resid = max(resid, abs(r["r2"][j] - r2) / r2)
    report(f"vbls_jobs L{L} H{H} full_cov={int(full)} {storage} {len(jobs)} jobs (lds up to {lds} columns): "
           + " ".join(f"{k}={v:.2e}" for k, v in worst.items()) + f" r2={resid:.2e}")
    return worst, resid


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("H", [1, 5, 16, 17, 32])
@pytest.mark.parametrize("L", [33, 300])
def test_against_fp64(pkg, L, H, full):
    worst, resid = _against_fp64(pkg, L, H, full, "f32")
    bad = {k: v for k, v in worst.items() if not v <= TOL[full][k]}
    assert not bad, bad
    assert resid <= RESID_TOL, resid


@pytest.mark.parametrize("full", [False, True])
def test_against_fp64_bf16_storage(pkg, full):
    worst, resid = _against_fp64(pkg, 33, 5, full, "bf16")
    bad = {k: v for k, v in worst.items() if not v <= TOL[full][k]}
    assert not bad, bad
    assert resid <= RESID_TOL, resid


# ---- 2. segmentation, bitwise --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _seg_case(full, lds):
    """lds: the widest bag whose state stays in LDS at H = 17 in this form; it and one column more are among the widths"""
    L, H = 300, 17
    mods = _models(L, H) + [trained("dual", L, H, 4900)]
    widths = ([1] if full else []) + [3, 2, 7, 8, 9, 17, 64, 70, lds, lds + 1]
    Ys = [_f32(mods[b % 3][1](w)) for b, w in enumerate(widths)]
    return L, H, [model_arrays(po) for po, _ in mods], Ys


@pytest.mark.parametrize("full", [False, True])
def test_segmentation_is_bitwise(pkg, full):
    L, H, arrays, Ys = _seg_case(full, pkg.capi.vbls_jobs_lds_cols(17, full))
    nb = len(Ys)
    jobs = [(b, k) for b in range(nb) for k in range(3)]
    jobs += [jobs[4], jobs[17]]                                        # two jobs twice
    assert len(jobs) >= 29
    rng = np.random.default_rng(5)
    perm = rng.permutation(len(jobs))
    c, off = _upload(pkg, Ys)
    with c:
        run = lambda js: c.sparse_fixed_basis_jobs(off, H, arrays, [b for b, _ in js], [k for _, k in js], NITER, full_cov=full)
        base = run(jobs)
        assert not base["status"].any()
        # permuting the jobs permutes every output
        pj = [jobs[i] for i in perm]
        pr = run(pj)
        assert all(_job_equal(pr, j, base, int(i)) for j, i in enumerate(perm))
        # repeating a job gives two identical blocks
        assert _job_equal(base, len(jobs) - 2, base, 4) and _job_equal(base, len(jobs) - 1, base, 17)
        # a job alone equals the same job among 40 others
        many = [jobs[i % len(jobs)] for i in range(41)]
        mr = run(many)
        for j in (0, 7, 20, 28, 40):
            one = run([many[j]])
            assert _job_equal(one, 0, mr, j), j
            # ... and with only its own model in the call
            b, k = many[j]
            alone = c.sparse_fixed_basis_jobs(off, H, [arrays[k]], [b], [0], NITER, full_cov=full)
            assert _job_equal(alone, 0, mr, j), j
        # one output at a time: the other pointers NULL
        C = pkg.capi
        dp, ip = C.C.POINTER(C.C.c_double), C.C.POINTER(C.C.c_int64)
        pk = lambda key, order="C": np.concatenate([np.asarray(m[key], dtype=np.float64).reshape(-1, order=order) for m in arrays])
        ins = [pk("BHat", "F"), pk("SigmaB", "F"), pk("alpha"), pk("beta0"), pk("eta0"), pk("zeta0"), pk("sigma0"), pk("ca0")]
        jb, jk = np.array([b for b, _ in jobs], dtype=np.int64), np.array([k for _, k in jobs], dtype=np.int64)
        r2, st = np.empty(len(jobs)), np.empty(len(jobs), dtype=np.int64)
        P = lambda v, t=dp: None if v is None else v.ctypes.data_as(t)
        rc = C.lib().vbmf_sparse_fixed_basis_jobs(c._h, nb, P(off, ip), H, NITER, int(full), 3, *[P(v) for v in ins], len(jobs), P(jb, ip),
                                                  P(jk, ip), P(r2), None, None, None, None, None, None, None, P(st, ip))
        assert rc == C.VBMF_OK and np.array_equal(r2, base["r2"]) and not st.any()
    # the same bag through a BagPool's context and through a fresh Bags upload of that bag alone
    with pkg.BagPool(Ys) as pool:
        pr = pool.ctx.sparse_fixed_basis_jobs(pool.col_off, H, arrays, [b for b, _ in jobs], [k for _, k in jobs], NITER, full_cov=full)
        assert all(_job_equal(pr, j, base, j) for j in range(len(jobs)))
        for b in (0, 4, nb - 1):
            bags = pkg.Bags([Ys[b]], 1)
            try:
                fr = bags.ctx.sparse_fixed_basis_jobs(bags.col_off, H, arrays, [0, 0, 0], [0, 1, 2], NITER, full_cov=full)
            finally:
                bags.close()
            for k in range(3):
                assert _job_equal(fr, k, pr, jobs.index((b, k))), (b, k)


def test_vbls_sparse_jobs_fills_the_sets_of_the_single_bag_path(pkg):
    """vbls_sparse_jobs_ on a pool: every job's set carries the call's blocks, and agrees with the oracle as the entry does"""
    L, H = 33, 5
    mods = _models(L, H)
    Ys = [_f32(mods[b % 2][1](w)) for b, w in enumerate([3, 1, 8, 17])]
    P = [(pkg.vbmf_sparse_parameters, pkg.vbmf_dual_parameters)[k] for k in range(2)]
    from tests.test_gpu_vbls_sparse_batch import _convert
    res = [_convert(P[k], mods[k][0]) for k in range(2)]
    jb, jk = [3, 0, 1, 2, 3], [1, 0, 1, 0, 0]
    with pkg.BagPool(Ys) as pool:
        sets, r2, status = pkg.vbls_sparse_jobs_(pool, res, jb, jk, NITER, full_cov=True)
        raw = pool.ctx.sparse_fixed_basis_jobs(pool.col_off, H, [model_arrays(r) for r in res], jb, jk, NITER, full_cov=True)
    sets2, r22, _ = pkg.vbls_sparse_jobs_(Ys, res, jb, jk, NITER, full_cov=True)
    assert not status.any() and np.array_equal(r2, raw["r2"]) and np.array_equal(r2, r22)
    for j, (p, b, k) in enumerate(zip(sets, jb, jk)):
        assert type(p) is P[k] and (p.L, p.M, p.H) == (L, Ys[b].shape[1], H)
        assert all(np.array_equal(getattr(p, f), _block(raw, j, f)) for f in FIELDS)
        assert all(np.array_equal(getattr(p, f), getattr(sets2[j], f)) for f in FIELDS)
        assert np.array_equal(p.AHat, p.ATVecHat.reshape(p.M, H)) and relF(p.YHat, p.BHat @ p.AHat.T) < 1e-14
        q = oracle_vbls(pkg, Ys[b], mods[k][0], NITER, True, seed=j)
        assert all((abs(getattr(p, f) - getattr(q, f)) / abs(getattr(q, f)) if np.isscalar(getattr(q, f)) else relF(getattr(p, f), getattr(q, f)))
                   <= TOL[True][f] for f in FIELDS)
        if k == 1:
            assert np.array_equal(p.A0Hat, p.AHat[:, :p.H0]) and p.alpha0 == p.alpha00 + 0.5 and p.alpha1 == p.alpha01 + 0.5


# ---- 3. isolation ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full", [False, True])
def test_a_failed_job_leaves_the_other_jobs_alone(pkg, full):
    """A model whose start makes a precision exactly zero: ca0 = -G_hh sigma0 with sigma0 = 1 on column h of a basis of multiples of
    1/8 and a SigmaB of multiples of 1/64, so that G = B'B + L SigmaB is exact in fp64 whatever the order of its sums."""
    L, H, h = 300, 5, 2
    mods = _models(L, H)
    rng = np.random.default_rng(31)
    bad = dict(model_arrays(mods[1][0]))
    bad["BHat"] = np.round(rng.standard_normal((L, H)) * 8) / 8
    bad["SigmaB"] = np.diag(np.arange(1, H + 1) / 64.0)
    Gm = bad["BHat"].T @ bad["BHat"] + L * bad["SigmaB"]
    bad["ca0"], bad["sigma0"] = -float(Gm[h, h]), 1.0
    arrays = [model_arrays(mods[0][0]), bad, model_arrays(mods[1][0])]
    Ys = [_f32(mods[b % 2][1](w)) for b, w in enumerate([3, 2, 9, 17, 70])]
    jobs = [(b, k) for b in range(len(Ys)) for k in range(3)]
    keep = [0, 2]
    c, off = _upload(pkg, Ys)
    with c:
        r = c.sparse_fixed_basis_jobs(off, H, arrays, [b for b, _ in jobs], [k for _, k in jobs], NITER, full_cov=full)     # returns: success
        jobs2 = [(b, keep.index(k)) for b, k in jobs if k != 1]
        r2 = c.sparse_fixed_basis_jobs(off, H, [arrays[k] for k in keep], [b for b, _ in jobs2], [k for _, k in jobs2], NITER, full_cov=full)
    assert np.array_equal(r["status"], [int(k == 1) for _, k in jobs]) and not r2["status"].any()
    good = [j for j, (_, k) in enumerate(jobs) if k != 1]
    for j, (b, k) in enumerate(jobs):
        if k == 1:
            assert np.isnan(r["r2"][j]) and all(np.all(np.isnan(_block(r, j, f))) for f in FIELDS), j
            assert _block(r, j, "ATVecHat").shape == (Ys[b].shape[1] * H,)
    for j2, j in enumerate(good):
        assert _job_equal(r, j, r2, j2), (j, jobs[j])
        assert np.isfinite(r["r2"][j]) and all(np.all(np.isfinite(_block(r, j, f))) for f in FIELDS)


# ---- 4. C ABI refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(pkg):
    C = pkg.capi
    VI, VU = C.VBMF_ERR_INVALID, C.VBMF_ERR_UNSUPPORTED
    L, H = 33, 5
    mods = _models(L, H)
    arrays = [model_arrays(po) for po, _ in mods]
    Ys = [_f32(mods[b % 2][1](w)) for b, w in enumerate([3, 1, 2, 7, 8, 9, 17, 4])]
    ip, dp = C.C.POINTER(C.C.c_int64), C.C.POINTER(C.C.c_double)
    i64 = lambda v: np.array(v, dtype=np.int64)
    pk = lambda key, order="C": np.concatenate([np.asarray(m[key], dtype=np.float64).reshape(-1, order=order) for m in arrays])
    SENT = -7.0
    c, off = _upload(pkg, Ys)
    nb, M = len(Ys), int(off[-1])
    good = dict(o=off, H=H, niter=NITER, full=1, B=pk("BHat", "F"), SB=pk("SigmaB", "F"), al=pk("alpha"), b0=pk("beta0"), e0=pk("eta0"),
                z0=pk("zeta0"), s0=pk("sigma0"), c0=pk("ca0"), jb=i64([0, 3, 7, 3]), jk=i64([1, 0, 1, 1]))
    outs = {k: np.full(H * M * 2, SENT) for k in ("A", "dS", "CA", "be")}
    outs.update(r2=np.full(8, SENT), SA=np.full(8 * H * H, SENT), sg=np.full(8, SENT), ze=np.full(8, SENT))
    sbuf = np.full(8, -7, dtype=np.int64)

    def raw(ctx, nk=2, nj=None, s=sbuf, null=(), **kw):
        a = {**good, **kw}
        p = lambda v, t: None if v is None else v.ctypes.data_as(t)
        o = {k: (None if k in null else v) for k, v in outs.items()}
        nj = (4 if a["jb"] is None else len(a["jb"])) if nj is None else nj
        return C.lib().vbmf_sparse_fixed_basis_jobs(ctx._h, len(a["o"]) - 1, p(a["o"], ip), a["H"], a["niter"], a["full"], nk, p(a["B"], dp),
                                                    p(a["SB"], dp), p(a["al"], dp), p(a["b0"], dp), p(a["e0"], dp), p(a["z0"], dp), p(a["s0"], dp),
                                                    p(a["c0"], dp), nj, p(a["jb"], ip), p(a["jk"], ip), p(o["r2"], dp), p(o["A"], dp),
                                                    p(o["dS"], dp), p(o["CA"], dp), p(o["be"], dp), p(o["SA"], dp), p(o["sg"], dp), p(o["ze"], dp),
                                                    p(s, ip))

    def untouched():
        return all(np.all(v == SENT) for v in outs.values()) and np.all(sbuf == -7)

    def spoiled(key, i, v):
        x = good[key].copy(); x[i] = v
        return {key: x}

    refused = [(VU, dict(H=0)), (VU, dict(H=33)), (VU, dict(H=-1)),
               (VI, dict(nk=0)), (VI, dict(nj=0)), (VI, dict(nk=-1)), (VI, dict(nj=-3)), (VI, dict(niter=0)), (VI, dict(niter=-2)),
               (VI, dict(s=None)), (VI, dict(null=("r2", "A")))]
    refused += [(VU, dict(nj=1 << 24)), (VU, dict(nk=1 << 24))]          # more workgroups than one grid holds: refused before any table is read
    refused += [(VI, {k: None}) for k in ("B", "SB", "al", "b0", "e0", "z0", "s0", "c0", "jb", "jk")]
    refused += [(VI, spoiled(k, i, v)) for k, i in (("B", -1), ("B", 7), ("SB", 3), ("al", 1), ("b0", 9), ("e0", 0), ("z0", 1), ("s0", 0), ("c0", 1))
                for v in (np.nan, np.inf)]
    refused += [(VI, dict(jb=i64([0, 3, nb, 3]))), (VI, dict(jb=i64([-1, 3, 7, 3]))), (VI, dict(jk=i64([1, 0, 2, 1]))), (VI, dict(jk=i64([1, -1, 1, 1])))]
    refused += [(VI, dict(o=i64(b))) for b in ([0, 1, 1, M], [1, 17, M], [0, 17, M - 1], [0, 20, 10, M], [0, M + 1])]
    refused += [(VI, dict(full=0, jb=i64([0, 1, 7, 3])))]              # a 1-column bag in the diagonal form under the QS1 layout
    with c:
        Y0, dims0 = c.get_Y(), c.dims()
        ref = c.sparse_fixed_basis_jobs(off, H, arrays, good["jb"], good["jk"], NITER, full_cov=True)
        for code, kw in refused:
            if "o" in kw:                                             # (the jobs name bags of the shorter col_off)
                kw = dict(kw, jb=i64([0, 0, 0, 0]))
            assert raw(c, **kw) == code, kw
            assert untouched(), kw
        assert raw(c, **spoiled("B", 7, np.nan)) == VI and "not finite" in c._lib.vbmf_last_error(c._h).decode()
        assert raw(c, **refused[-1][1]) == VI and "1-column bag" in c._lib.vbmf_last_error(c._h).decode()
        assert np.array_equal(c.get_Y(), Y0) and c.dims() == dims0
        # after the refusals a good call returns the former bits, and writes only its own jobs
        assert raw(c) == C.VBMF_OK and np.array_equal(sbuf[:4], [0, 0, 0, 0]) and np.all(sbuf[4:] == -7)
        n = int(ref["off"][-1])
        assert np.array_equal(outs["r2"][:4], ref["r2"]) and np.all(outs["r2"][4:] == SENT)
        assert np.array_equal(outs["A"][:n], ref["ATVecHat"]) and np.all(outs["A"][n:] == SENT)
        assert np.array_equal(outs["SA"][:4 * H * H], ref["SigmaA"].reshape(-1)) and np.all(outs["SA"][4 * H * H:] == SENT)
        assert np.array_equal(c.get_Y(), Y0) and c.dims() == dims0
        # a label mask on the context
        z = np.zeros
        c.set_state(z((M, 1)), np.ones((L, 1)), z((1, 1)), z((1, 1)), np.ones(1), np.ones(1), 1.0, labels0=[0], H1=1)
        for v in outs.values():
            v[:] = SENT
        sbuf[:] = -7
        assert raw(c) == VI and "label mask" in c._lib.vbmf_last_error(c._h).decode() and untouched()
    with C.Context(L, M, 5, y_dtype=pkg.VBMF_Y_F32) as c2:             # no Y
        assert raw(c2) == VI and "no Y" in c2._lib.vbmf_last_error(c2._h).decode() and untouched()
    with C.Context(L, M, 5, y_dtype=pkg.VBMF_Y_F32, nranks=2, rank=0, L_global=2 * L, variant=C.VBMF_VARIANT_SPARSE_DIAG) as c2:
        assert raw(c2) == VI and "rank" in c2._lib.vbmf_last_error(c2._h).decode() and untouched()
