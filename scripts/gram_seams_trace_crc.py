"""CRC-32s of what whole Gram-form runs leave across run boundaries and eps stops (the seams of the sweep's H x H control chain,
DESIGN.md section 10), on seeded inputs, one entry per rank of CASES (one per tier of the fp64 inverse, R = 1, 2, 4, 8; lambda_max by
repeated squaring up to H = 64, by Lanczos above).

    python scripts/gram_seams_trace_crc.py [OUT.json] [--commit ID]    (on an MI355X; default tests/golden/gram_seams_trace_crc.json)

Each case: the integer Y of scripts/gram_tail_state_crc.py (seeded_Y, exact in bf16), VBMF_GRAM=1, run(1) as a streaming sweep that
builds G and W, then Gram-form runs with a trace, each variant in a context of its own:

  a  run(6): all 6 x 4 trace doubles (d, sigma2, ELBO, residual) and the final state (SigmaA, SigmaB, ca, cb, scalars 0-15);
  b  run(3), run(3): the concatenated traces and the final state;
  c  run(6, eps) with eps between two consecutive d of (a) that differ by more than 0.1 % (the first such pair; eps is their
     geometric mean and goes into the file): the stopping sweep, the trace up to it and the state; then run(2) from there, its
     trace and state;
  k  run(k), k the stopping sweep of (c): what (c)'s stop state is compared with.

Identities asserted HERE, on the build that makes the fixture, and listed in the file ("identities"): b == a (trace and state),
c's stop trace == the first k rows of a, c's stop state == k's state.  tests/test_gpu_gram_seams.py re-asserts the listed ones.

No fp64 operation of the chain may change its operands or its order, so a rework of its schedule must reproduce every CRC.  The
fixture is made ONCE, on the build of the commit BEFORE such a rework (its id goes into the file: --commit, or git's HEAD), and
committed as it came out.  Never regenerate it from the code under test.
"""
import importlib.util
import json
import os
import subprocess
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

_spec = importlib.util.spec_from_file_location("gram_tail_state_crc", os.path.join(ROOT, "scripts", "gram_tail_state_crc.py"))
tail_script = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tail_script)

L, M = 600, 353
# (H, R = tier of the inverse / lambda_max kernels, lambda_max method)
CASES = [
    (12, 1, "repeated squaring"),
    (24, 2, "repeated squaring"),
    (64, 4, "repeated squaring"),
    (100, 8, "Lanczos"),
]
NSWEEP = 6
STATE_KEYS = ("SigmaA", "SigmaB", "ca", "cb", "scalars")
IDENTITIES = ("b_equals_a", "c_stop_trace_is_prefix_of_a", "c_stop_state_equals_run_k")


def key(H):
    return f"{L}x{M}xH{H}"


def crc(a):
    return "%08x" % (zlib.crc32(np.ascontiguousarray(a).view(np.uint8).tobytes()) & 0xFFFFFFFF)


def read_state(c):
    """SigmaA, SigmaB, ca, cb and the state block's scalars 0-15, as the device holds them"""
    cap = sys.modules["vbmf_amd"].capi
    Hp = c.dims()["Hp"]
    scal = 9 * Hp * Hp + 8 + 2 * Hp                             # StateLayout::scal(), in doubles
    sc = c.peek(cap.PEEK_STATE, 32, offset=2 * scal, dtype=np.float64).copy()
    s = c.get_state(want_B=False)
    return dict(SigmaA=np.ascontiguousarray(s["SigmaA"]), SigmaB=np.ascontiguousarray(s["SigmaB"]), ca=s["CA_diag"].copy(),
                cb=s["CB_diag"].copy(), scalars=sc)


def runs(pkg, H, plan):
    """A fresh context: one streaming sweep, then the Gram-form runs (niter, eps) of plan with a trace.  Returns (per run
    (iters, trace, state), dims, chain_us)."""
    from oracle import vbmf_oracle as O
    cap = pkg.capi
    Y = tail_script.seeded_Y(M, H)
    po = O.vbmf_init(Y, H, ca=0.1, cb=0.1, sigma2=0.1, rng=np.random.default_rng(9300 + H), materialize_yhat=False)
    old = os.environ.get("VBMF_GRAM")
    os.environ["VBMF_GRAM"] = "1"
    try:
        c = cap.Context(L, M, H, y_dtype=pkg.VBMF_Y_BF16, factor_dtype=pkg.VBMF_FACTOR_BF16X2)
    finally:
        if old is None:
            del os.environ["VBMF_GRAM"]
        else:
            os.environ["VBMF_GRAM"] = old
    out = []
    with c:
        c.set_Y(Y)
        c.set_state(po.AHat, po.BHat, po.SigmaA, po.SigmaB, np.diag(po.CA), np.diag(po.CB), po.sigma2)
        c.run(1, eps=0.0, est_covs=True, est_var=True)
        for n, eps in plan:
            it, _, tr = c.run(n, eps=eps, est_covs=True, est_var=True, want_trace=True)
            out.append((it, tr.copy(), read_state(c)))
        dims = c.dims()
        chain = c.chain_us()
    return out, dims, chain


def _cover(s, k):
    return s[k][:16] if k == "scalars" else s[k]                # scalars 16-31 hold scratch (the shadows of speculative results)


def same_state(a, b):
    """bitwise, over what the CRCs cover"""
    return all(np.array_equal(_cover(a, k).view(np.uint64), _cover(b, k).view(np.uint64)) for k in STATE_KEYS)


def same_trace(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def state_crc(s):
    return {k: crc(_cover(s, k)) for k in STATE_KEYS}


def pick_eps(d):
    """eps between the first two consecutive d of which the later is the lowest so far by more than 0.1 %; (eps, stopping sweep)"""
    for k in range(1, len(d)):
        if d[k] < (1.0 - 1e-3) * np.min(d[:k]):
            eps = float(np.sqrt(d[k - 1] * d[k]))
            assert d[k] < eps < np.min(d[:k]), (d, eps)
            return eps, k + 1
    raise AssertionError(("no two consecutive d more than 0.1 % apart", d))


def case(pkg, H, eps=None):
    """Runs variants a, b, c, k.  eps: the fixture's (None: chosen from a's trace).  Returns the arrays and the CRC record."""
    (a,), dims, chain = runs(pkg, H, [(NSWEEP, 0.0)])
    assert a[0] == NSWEEP and a[1].shape == (NSWEEP, 4), (H, a[0])
    b, _, _ = runs(pkg, H, [(3, 0.0), (3, 0.0)])
    if eps is None:
        eps, _ = pick_eps(a[1][:, 0])
    c, _, _ = runs(pkg, H, [(NSWEEP, eps), (2, 0.0)])
    kstop = c[0][0]
    (k,), _, _ = runs(pkg, H, [(kstop, 0.0)])
    arr = dict(a=a, b=b, c=c, k=k, dims=dims, chain=chain)
    b_trace = np.vstack([b[0][1], b[1][1]])
    rec = dict(
        a=dict(trace=crc(a[1]), state=state_crc(a[2])),
        b=dict(trace=crc(b_trace), state=state_crc(b[1][2])),
        c=dict(eps=float(eps).hex(), stop_sweep=int(kstop), trace=crc(c[0][1]), state=state_crc(c[0][2]),
               trace2=crc(c[1][1]), state2=state_crc(c[1][2])),
        k=dict(trace=crc(k[1]), state=state_crc(k[2])),
    )
    held = dict(
        b_equals_a=same_trace(b_trace, a[1]) and same_state(b[1][2], a[2]),
        c_stop_trace_is_prefix_of_a=same_trace(c[0][1], a[1][:kstop]),
        c_stop_state_equals_run_k=same_state(c[0][2], k[2]) and same_trace(c[0][1], k[1]),
    )
    return arr, rec, held


def main():
    import __graft_entry__ as G
    args = sys.argv[1:]
    commit = None
    if "--commit" in args:
        i = args.index("--commit")
        commit = args[i + 1]
        del args[i:i + 2]
    if commit is None:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    out = args[0] if args else os.path.join(ROOT, "tests", "golden", "gram_seams_trace_crc.json")
    G.build()
    pkg = G.load_package()
    cases = {}
    held_all = {name: True for name in IDENTITIES}
    for H, R, method in CASES:
        arr, rec, held = case(pkg, H)
        d = arr["a"][1][:, 0]
        eps, kexp = pick_eps(d)
        assert rec["c"]["stop_sweep"] == kexp, (H, rec["c"]["stop_sweep"], kexp, d)
        assert arr["c"][1][0] == 2, (H, arr["c"][1][0])
        assert arr["dims"]["gram"] == 1 and (1 if H <= 16 else 2 if H <= 32 else 4 if H <= 64 else 8) == R, (H, arr["dims"])
        for name in IDENTITIES:
            held_all[name] = held_all[name] and held[name]
        cases[key(H)] = rec
        print(key(H), f"R {R}, {method}: d", " ".join("%.6e" % x for x in d), "eps %.6e stop at" % eps, kexp, held,
              "scalars", " ".join("%.9g" % x for x in arr["a"][2]["scalars"][:16]), "chain_us", arr["chain"], flush=True)
        print(json.dumps(rec, sort_keys=True), flush=True)
    # an identity that this build does not have is not listed, and not asked of a later build
    identities = [name for name in IDENTITIES if held_all[name]]
    print("identities that held:", identities, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(dict(made_by_commit=commit, identities=identities, cases=cases), f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
