"""CRC-32s along call sequences on one context: what every call returns and leaves, across the points where the host reuses or drops
a cached quantity derived from (Y, A, B) -- the Grams A'A and B'B, Y'B, Y A, tr(B'YA), G = Y'Y, W, the owed B (csrc/ctx_cache.hpp,
DESIGN.md section 10 "Run boundaries").

    python scripts/ctx_sequences_crc.py [OUT.json] [--commit ID]     (on an MI355X; default tests/golden/ctx_sequences_crc.json)
    python scripts/ctx_sequences_crc.py --check-only                  (runs every sequence once against the stored file, writes nothing)

A cache kept too long or dropped too early shows as another bit somewhere down the sequence, so a rework of the host bookkeeping must
reproduce the CRCs.  The fixture is made ONCE, on the build of the commit BEFORE such a rework (its id goes into the file: --commit,
or git's HEAD), and committed as it came out; tests/test_gpu_ctx_sequences.py asserts it on the current build.  Never regenerate it
from the code under test.

Every sequence runs in two recordings.  "each": after every call one CRC over every field of get_state / sparse_get_state, the
scalars the call returned and dims().  Reading B pays the pass a Gram-form run owes, so "end" records only the scalars and dims()
after every call and the state once, after the last: there the debt stays open across the calls as it does for a caller who never
looks.  dims() goes in without its two timings (gram_build_us, set_y_rows_us).  A call that the library refuses goes in with its
error code; a sequence states which refusals it expects.  The generator runs every sequence twice and refuses to record one whose
two runs differ.
"""
import json
import os
import subprocess
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "ctx_sequences_crc.json")
TIMINGS = ("gram_build_us", "set_y_rows_us")
INVALID = -1                                                  # VBMF_ERR_INVALID

# ---- the sequences: (op, argument...) per call; ("refused", code, op...) is a call that must come back with that error code ----
BASIC_SEQS = {
    "steps": [("step", "A"), ("step", "CA|SIGMA2"), ("step", "B"), ("elbo",)],
    "noY_setY_run_vbls": [("set_state",), ("step", "CA|CB"), ("set_Y", 0), ("run", 3), ("step", "A"), ("fixed_basis", 4), ("elbo",)],
    "run_newY_run": [("run", 3), ("set_Y", 1), ("run", 2)],
    "run_newB_vbls_batched": [("run", 2), ("set_state", "B2"), ("fixed_basis", 3), ("fixed_basis_batched", 4), ("step", "SIGMA2")],
    "transport": [("step", "A"), ("transport",), ("step", "CA|SIGMA2"), ("run", 2)],
    "Y_rows_two_blocks": [("set_Y_rows", 1, 0, 320), ("refused", INVALID, "step", "A"), ("set_Y_rows", 1, 320, None), ("run", 2)],
}
GRAM_SEQS = {
    "run_run_stepA_run": [("run", 2), ("run", 2), ("step", "A"), ("run", 3)],
    "run_newY_run_bound": [("run", 3), ("set_Y", 1), ("run", 2), ("bound",)],
    "form_off_default": [("run", 2), ("gram_form", "OFF"), ("run", 2), ("gram_form", "DEFAULT"), ("run", 2)],
    "run_batched_run": [("run", 2), ("fixed_basis_batched", 3), ("run", 2)],
}
SPARSE_GRAM_SEQS = {
    "run_run_stepA_run": GRAM_SEQS["run_run_stepA_run"],
    "form_off_default": GRAM_SEQS["form_off_default"],
    "run_batched_run": GRAM_SEQS["run_batched_run"],          # W survives the sparse batched call
    "full_cov_on_off": [("run", 2), ("full_cov", 1), ("run", 1), ("full_cov", 0), ("run", 2)],
}
SPARSE_SEQS = {
    "steps": [("step", "A"), ("step", "CA"), ("step", "SIGMA"), ("step", "B"), ("bound",)],
    "run_SigmaA_sigma": [("run", 2), ("SigmaA",), ("step", "SIGMA")],
}
DIAGVAR_SEQS = {
    "noise_steps_vbls_run": [("noise_rows",), ("step", "A"), ("step", "SIGMA"), ("step", "B"), ("step", "SIGMA"), ("fixed_basis", 2), ("run", 2)],
}


def _cases():
    """name -> (model kind, L, M, H, mode, sequence).  Modes: f32 (fp32 Y), bf16x2 (bf16 Y, bf16 hi + lo factors), bf16 (bf16 Y, one
    bf16 factor operand), gram (bf16x2, forced into the Gram form by VBMF_GRAM at creation), auto (bf16 Y, the factor operand the
    library picks)"""
    out = {}
    for mode in ("f32", "bf16x2"):
        for k, s in BASIC_SEQS.items():
            out[f"basic-{mode}-601x97xH24-{k}"] = ("basic", 601, 97, 24, mode, s)
        for k in ("steps", "run_newY_run"):                   # two h tiles: the streaming sweep's other narrow / epilogue instances
            out[f"basic-{mode}-601x97xH40-{k}"] = ("basic", 601, 97, 40, mode, BASIC_SEQS[k])
    out["basic-bf16-257x161xH100-steps"] = ("basic", 257, 161, 100, "bf16", BASIC_SEQS["steps"])     # four h tiles, single-bf16 operand
    out["sparse-257x161xH130-steps"] = ("sparse", 257, 161, 130, "auto", SPARSE_SEQS["steps"])       # eight h tiles, streaming
    out["basic-bf16x2-257x161xH130-noY_setY_run_vbls"] = ("basic", 257, 161, 130, "bf16x2", BASIC_SEQS["noY_setY_run_vbls"])   # side stream
    for M, H in ((61, 24), (353, 100)):
        for k, s in GRAM_SEQS.items():
            if k == "run_batched_run" and H > 64:             # the batched call covers H <= 64: its refusal must leave W alone too
                s = [s[0], ("refused", INVALID) + s[1], s[2]]
            out[f"gram-basic-600x{M}xH{H}-{k}"] = ("basic", 600, M, H, "gram", s)
    for M in (61, 353):
        for k, s in SPARSE_GRAM_SEQS.items():
            out[f"gram-sparse-600x{M}xH64-{k}"] = ("sparse", 600, M, 64, "gram", s)
    for kind in ("sparse", "fullcov"):
        for k, s in SPARSE_SEQS.items():
            out[f"{kind}-257x61xH12-{k}"] = (kind, 257, 61, 12, "auto", s)
    for k, s in DIAGVAR_SEQS.items():
        out[f"diagvar-257x61xH12-{k}"] = ("diagvar", 257, 61, 12, "auto", s)
    return out


CASES = _cases()


def crc(parts):
    v = 0
    for a in parts:
        v = zlib.crc32(np.ascontiguousarray(a).view(np.uint8).tobytes(), v)
    return "%08x" % (v & 0xFFFFFFFF)


_PROBLEMS = {}


def problem(kind, L, M, H):
    """(Y, another Y, the oracle's start state), built once per shape"""
    from oracle import vbmf_oracle as O
    key = (kind != "basic", L, M, H)
    if key not in _PROBLEMS:
        rng = np.random.default_rng(9100 + L + M + H)
        _, A, B = O.toy_matrix(L, M, H, 0.05, rng)
        Ys = [(B * np.linspace(1.0, 3.0, H)) @ A.T + s * rng.standard_normal((L, M)) for s in (0.05, 0.08)]
        Ys[1] = Ys[1][::-1] * 1.25
        if kind == "basic":
            po = O.vbmf_init(Ys[0], H, ca=0.1, cb=0.1, sigma2=0.1, rng=np.random.default_rng(9101 + H), materialize_yhat=False)
        else:
            po = O.vbmf_sparse_init(Ys[0], H, ca=0.1, cb=0.1, sigma=0.1, rng=np.random.default_rng(9101 + H), full_cov=False,
                                    materialize_yhat=False)
        _PROBLEMS[key] = (Ys[0], np.ascontiguousarray(Ys[1]), po)
    return _PROBLEMS[key]


class Runner:
    """one context of a case and the calls of its sequence"""

    def __init__(self, pkg, name):
        self.pkg, self.cap = pkg, pkg.capi
        self.kind, self.L, self.M, self.H, self.mode, self.seq = CASES[name]
        self.sparse = self.kind != "basic"
        self.Ys = problem(self.kind, self.L, self.M, self.H)[:2]
        self.po = problem(self.kind, self.L, self.M, self.H)[2]
        third = self.M // 3
        self.col_off = np.array([0, third, 2 * third + 1, self.M], dtype=np.int64)

    def context(self):
        cap = self.cap
        kw = dict(y_dtype=cap.VBMF_Y_F32 if self.mode == "f32" else cap.VBMF_Y_BF16,
                  factor_dtype=dict(f32=cap.VBMF_FACTOR_AUTO, auto=cap.VBMF_FACTOR_AUTO, bf16=cap.VBMF_FACTOR_BF16).get(self.mode, cap.VBMF_FACTOR_BF16X2))
        if self.sparse:
            kw["variant"] = cap.VBMF_VARIANT_SPARSE_DIAGVAR if self.kind == "diagvar" else cap.VBMF_VARIANT_SPARSE_DIAG
        old = os.environ.get("VBMF_GRAM")
        os.environ["VBMF_GRAM"] = ("2" if self.sparse else "1") if self.mode == "gram" else "0"
        try:
            c = cap.Context(self.L, self.M, self.H, **kw)
        finally:
            if old is None:
                del os.environ["VBMF_GRAM"]
            else:
                os.environ["VBMF_GRAM"] = old
        assert c.dims()["gram"] == (1 if self.mode == "gram" else 0)
        return c

    def set_state(self, c, B=None):
        po = self.po
        B = po.BHat if B is None else B
        if self.sparse:
            hyper = dict(alpha0=po.alpha0, beta0=po.beta0, gamma0=po.gamma0, delta0=po.delta0, eta0=po.eta0, zeta0=po.zeta0)
            c.sparse_set_state(po.ATVecHat, po.diagSigmaATVec, po.CA, po.beta, B, po.SigmaB, po.CB, po.delta, po.sigmaHat, po.zeta, hyper)
        else:
            c.set_state(po.AHat, B, po.SigmaA, po.SigmaB, np.diag(po.CA), np.diag(po.CB), po.sigma2)

    def state(self, c):
        """every field of the state, in a fixed order; none before the first set_state"""
        try:
            s = c.sparse_get_state() if self.sparse else c.get_state()
        except self.cap.VbmfError as e:
            return [np.array([e.code], dtype=np.int64)]
        out = [np.asarray(s[k], dtype=np.float64) for k in sorted(s)]
        if self.kind == "diagvar":
            try:
                out += list(c.sparse_get_noise_rows())
            except self.cap.VbmfError as e:
                out.append(np.array([e.code], dtype=np.int64))
        if self.kind == "fullcov":
            out.append(c.sparse_get_SigmaA())
        return out

    def dims(self, c):
        d = c.dims()
        return np.array([d[k] for k in sorted(d) if k not in TIMINGS], dtype=np.int64)

    def bits(self, which, table):
        v = 0
        for b in which.split("|"):
            v |= table[b]
        return v

    def call(self, c, op):
        """the scalars and arrays the call returned, as a list of arrays"""
        cap, po, H, M = self.cap, self.po, self.H, self.M
        k, a = op[0], op[1:]
        if k == "step":
            if self.sparse:
                c.sparse_step(self.bits(a[0], dict(A=cap.SSTEP_A, B=cap.SSTEP_B, CA=cap.SSTEP_CA, CB=cap.SSTEP_CB, SIGMA=cap.SSTEP_SIGMA)))
            else:
                c.step(self.bits(a[0], dict(A=cap.STEP_A, B=cap.STEP_B, CA=cap.STEP_CA, CB=cap.STEP_CB, SIGMA2=cap.STEP_SIGMA2)))
            return []
        if k == "run":
            it, d, _ = c.sparse_run(a[0], eps=0.0, est_cb=True) if self.sparse else c.run(a[0], eps=0.0, est_covs=True, est_var=True)
            return [np.array([it], dtype=np.int64), np.array([d])]
        if k == "bound" or k == "elbo":
            return [np.array([c.sparse_lower_bound() if self.sparse else c.elbo()])]
        if k == "set_state":
            self.set_state(c, 0.5 * po.BHat[::-1].copy() + 0.25 if a else None)
            return []
        if k == "set_Y":
            c.set_Y(self.Ys[a[0]])
            return []
        if k == "set_Y_rows":
            Y, r0, n = self.Ys[a[0]], a[1], a[2]
            c.set_Y_rows(np.ascontiguousarray(Y[r0:] if n is None else Y[r0:r0 + n]), row0=r0)
            return []
        if k == "fixed_basis":
            (c.sparse_run_fixed_basis if self.sparse else c.run_fixed_basis)(a[0])
            return []
        if k == "fixed_basis_batched":
            nb = self.col_off.size - 1
            if self.sparse:
                r = c.sparse_run_fixed_basis_batched(self.col_off, a[0], np.full((nb, H), 0.5), np.full((nb, H), 1e-3), np.full(nb, 40.0),
                                                     np.full(nb, 1e-3), np.full(nb, 30.0), np.ones(M * H))
            else:
                r = c.run_fixed_basis_batched(self.col_off, a[0], np.linspace(0.1, 0.3, nb), np.full((nb, H), 0.1))
            return [np.asarray(r[q], dtype=np.float64) for q in sorted(r)]
        if k == "transport":
            c.comm_set_transport(self.pkg.dist.host_staged_transport(lambda buf: None))     # one rank: the sum is the buffer itself
            return []
        if k == "gram_form":
            c.set_gram_form(dict(OFF=cap.VBMF_GRAM_FORM_OFF, DEFAULT=cap.VBMF_GRAM_FORM_DEFAULT)[a[0]])
            return []
        if k == "full_cov":
            c.sparse_set_full_cov(bool(a[0]))
            return []
        if k == "SigmaA":
            c.sparse_set_SigmaA(0.5 * np.eye(H) + 0.01)
            return []
        if k == "noise_rows":
            c.sparse_set_noise_rows(po.sigmaVecHat * np.linspace(0.5, 2.0, self.L), po.zetaVec + 0.25, float(po.etaVec[0]))
            return []
        raise ValueError(op)

    def run(self, record):
        """record = "each" or "end": the list of CRCs, one per call (and one for the final state in "end")"""
        out = []
        bare = self.seq[0][0] == "set_state"                 # the sequence itself brings the state, and Y later
        with self.context() as c:
            if not bare:
                c.set_Y(self.Ys[0])
                self.set_state(c)
                if self.kind == "fullcov":
                    c.sparse_set_full_cov(True)
            for op in self.seq:
                if op[0] == "refused":
                    try:
                        self.call(c, op[2:])
                        raise AssertionError(f"{op}: the call was not refused")
                    except self.cap.VbmfError as e:
                        assert e.code == op[1], (op, e.code, str(e))
                        got = [np.array([e.code], dtype=np.int64)]
                else:
                    got = self.call(c, op)
                out.append(crc((self.state(c) if record == "each" else []) + got + [self.dims(c)]))
            if record == "end":
                out.append(crc(self.state(c)))
        return out


def run_case(pkg, name):
    r = Runner(pkg, name)
    return dict(each=r.run("each"), end=r.run("end"))


def main():
    import __graft_entry__ as G
    args = sys.argv[1:]
    check_only = "--check-only" in args
    if check_only:
        args.remove("--check-only")
    commit = None
    if "--commit" in args:
        i = args.index("--commit")
        commit = args[i + 1]
        del args[i:i + 2]
    out = args[0] if args else GOLDEN
    G.build()
    pkg = G.load_package()
    if check_only:
        with open(GOLDEN) as f:
            gold = json.load(f)
        bad = [n for n in CASES if n not in gold["unrepeatable"] and run_case(pkg, n) != gold["cases"][n]]
        print(f"{len(CASES) - len(bad)} of {len(CASES)} sequences match {os.path.relpath(GOLDEN, ROOT)} (made by {gold['made_by_commit'][:12]})")
        for n in bad:
            print("MISMATCH", n)
        sys.exit(1 if bad else 0)
    if commit is None:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    cases, unrepeatable = {}, {}
    for n in CASES:
        a, b = run_case(pkg, n), run_case(pkg, n)
        if a != b:
            unrepeatable[n] = "two runs on the parent build differ: " + json.dumps(dict(first=a, second=b))
            print("UNREPEATABLE", n, flush=True)
            continue
        cases[n] = a
        print(n, a["end"][-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(dict(made_by_commit=commit, cases=cases, unrepeatable=unrepeatable), f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(cases)} sequences recorded, {len(unrepeatable)} unrepeatable")


if __name__ == "__main__":
    main()
