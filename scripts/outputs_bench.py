#!/usr/bin/env python3
"""What getting the results back costs, by destination: BHat*AHat' through vbmf_get_YHat_rows into GPU
float32 / bfloat16 / float64 tensors, row- and column-major, the float32 residual on the GPU and a float32 host array -- against the
route there was before, vbmf_get_YHat (a scalar fp64 kernel, then the whole L x M fp64 matrix over PCIe), on the same shapes in the
same run.

    python scripts/outputs_bench.py [--out profiles/outputs_bench.txt] [--shapes big64,big128,small]

Every measurement is a child process of its own (`--one CASE --shape NAME`) under its own time limit; the first child that fails or
runs out of time ends the run, nothing is tried twice.  A child warms its call once and times it three times: wall time around the
call (which returns after the context's stream is idle) and, for the new entries, the device time between two HIP events on the
context's stream (Context.out_rows_us()).  vbmf_get_YHat is left as it was and carries no events: wall time only, into one
preallocated, already touched fp64 array.
Roofs of a device case: bytes written (plus Y as stored read once for the residual) over the 6.3 TB/s copy rate, and 2 L M Hp flop
over 155 TF of fp32 MFMA (78 TF of fp64 MFMA for a float64 dst); `share` is the larger of the two times over the best device time.
--one ... --profile: the case's calls alone (no parent arm), for `rocprofv3 --kernel-trace --stats -- python scripts/outputs_bench.py ...`."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"big64": (100000, 10000, 64), "big128": (125000, 10000, 128), "small": (166, 3000, 5)}
COPY_RATE, F32_RATE, F64_RATE = 6.3e12, 155e12, 78e12
CASES = ["parent_get_YHat", "gpu_f32_rowmajor", "gpu_f32_colmajor", "gpu_bf16_rowmajor", "gpu_bf16_colmajor", "gpu_f64_rowmajor",
         "gpu_f64_colmajor", "gpu_f32_rowmajor_residual", "host_f32"]
ES = {"f64": 8, "f32": 4, "bf16": 2}


def child(case, shape, profile):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    pkg = G.load_package()
    L, M, H = SHAPES[shape]
    rng = np.random.default_rng(3)
    out = dict(case=case, shape=shape)
    with pkg.capi.Context(L, M, H, y_dtype=pkg.VBMF_Y_BF16) as c:
        c.set_Y_synthetic(7, min(H, 16), 0.1)
        z = np.zeros((H, H))
        c.set_state(rng.standard_normal((M, H)), rng.standard_normal((L, H)), z, z, np.ones(H), np.ones(H), 1.0)
        out["Hp"] = c.dims()["Hp"]
        if case == "parent_get_YHat":
            dst = np.zeros((L, M), order="F")                       # touched once: no page faults inside the timed calls
            call = lambda: c._chk(c._lib.vbmf_get_YHat(c._h, dst.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), L))
        else:
            kind, dt = case.split("_")[0], case.split("_")[1]
            residual = case.endswith("_residual")
            if kind == "host":
                dst = np.zeros((L, M), dtype=np.float32)
            else:
                tdt = {"f64": torch.float64, "f32": torch.float32, "bf16": torch.bfloat16}[dt]
                dst = torch.zeros((M, L), dtype=tdt, device="cuda").t() if "colmajor" in case else torch.zeros((L, M), dtype=tdt, device="cuda")
            call = lambda: c.YHat_into(dst, residual=residual)
            out["bytes"] = L * M * ES[dt] + (L * M * 2 if residual else 0)
            out["flop_s"] = 2.0 * L * M * out["Hp"] / (F64_RATE if dt == "f64" else F32_RATE)
        call()
        wall, dev = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t0) * 1e3)
            dev.append(c.out_rows_us() * 1e-3)
        out["wall_ms"], out["dev_ms"] = wall, None if case == "parent_get_YHat" else dev
        if not profile:
            some = dst[:: max(1, L // 64), :: max(1, M // 64)]          # a sample of the result, so that a run that wrote nothing shows
            some = some if isinstance(some, np.ndarray) else some.double().cpu().numpy()
            out["checksum"] = float(np.sum(np.abs(some.astype(np.float64))))
    print("RESULT " + json.dumps(out))


def run_child(case, shape):
    env = dict(os.environ)
    big = shape != "small"
    limit = (420 if case in ("parent_get_YHat", "host_f32") else 180) if big else 90
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", case, "--shape", shape], env=env, capture_output=True,
                       text=True, timeout=limit)
    lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not lines:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"{case} at {shape} failed with status {r.returncode}: the run ends here")
    return json.loads(lines[-1][7:])


def fmt(v):
    return "[" + " ".join(f"{x:.3f}" for x in v) + "]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one")
    ap.add_argument("--shape", default="small")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--shapes", default="big64,big128,small")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outputs_bench.txt"))
    a = ap.parse_args()
    if a.one:
        return child(a.one, a.shape, a.profile)
    text = ["YHat by destination on one MI355X (bf16 Y, bf16x2 factors), each case its own process: one warm call, then three timed ones (ms).",
            "wall: around the call, which returns after the context's stream is idle; device: between two HIP events on that stream (kernels,",
            "staged copies; vbmf_get_YHat carries no events).  roofs: bytes / 6.3 TB/s | 2 L M Hp / 155 TF (78 TF for float64); share: the larger",
            "roof over the best device time; x parent: the parent route's best wall time over this route's best wall time.", ""]

    shown = [0]

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(text) + "\n")
        print("\n".join(text[shown[0]:]), flush=True)                 # progress as it comes
        shown[0] = len(text)

    try:
        for shape in a.shapes.split(","):
            L, M, H = SHAPES[shape]
            text.append(f"--- {L} x {M}, H = {H} ---")
            parent = None
            for case in CASES:
                r = run_child(case, shape)
                if case == "parent_get_YHat":
                    parent = min(r["wall_ms"])
                    text.append(f"{case:26s} wall {fmt(r['wall_ms'])}  ({L * M * 8 / 1e9:.2f} GB of fp64 to the host)")
                else:
                    best = min(r["dev_ms"])
                    tb, tf = r["bytes"] / COPY_RATE * 1e3, r["flop_s"] * 1e3
                    roof = "" if case.startswith("host") else (f"roofs {tb:.3f} | {tf:.3f} ms ({'bytes' if tb >= tf else 'flop'} binds)  "
                                                               f"share {max(tb, tf) / best * 100:5.1f} %  ")
                    text.append(f"{case:26s} wall {fmt(r['wall_ms'])} device {fmt(r['dev_ms'])}  {roof}x parent {parent / min(r['wall_ms']):8.1f}")
                flush()
            text.append("")
    finally:
        flush()


if __name__ == "__main__":
    main()
