#!/usr/bin/env python3
"""What handing Y over costs, by source (vbmf_set_Y from fp64 host memory against vbmf_set_Y_rows from a float32 host array and from
float32 / bfloat16 / float64 GPU tensors), at 100 000 x 10 000 (50 000 rows when the host cannot hold the 8 GB fp64 array), for both
storage types -- and the A/B of the two tilers behind vbmf_set_Y_rows.

    python scripts/set_y_sources.py [--out profiles/set_y_sources.txt] [--lib LIB] [--ab-lib variants/libvbmf_hip_2a.so] [--rows N]

Every measurement is a child process of its own (`--one CASE`) under its own time limit; the first child that fails or runs out of
time ends the run, nothing is tried twice.  A child warms the call once and times it three times: wall time around the call (which
returns after the context's stream is idle) and, for vbmf_set_Y_rows, the device time between two HIP events on the context's
stream (dims()["set_y_rows_us"]).  vbmf_set_Y is left as it was and carries no events: wall time only.
--ab-lib: a second build of the library to compare against, loaded through VBMF_HIP_LIB -- for the recorded run one in which
tile_rows_typed (csrc/vbmf_hip.hip) sends every source through tile_y_kernel, once per copy ("2a"), against the in-tree build whose
sources with a unit stride take tile_pair_kernel ("2b").  Four rounds, the build that runs first alternating from round to round, GPU
float32 row-major and column-major, as in profiles/gram_seams_bench_ab.txt."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, H = 10000, 64
COPY_RATE = 6.3e12          # the device copy rate DESIGN.md uses
CASES = ["host_f64_set_Y", "host_f32", "gpu_f32_rowmajor", "gpu_f32_colmajor", "gpu_bf16", "gpu_f64"]
LIMIT_S = {"host_f64_set_Y": 420, "host_f32": 300}


def child(case, L):
    import torch
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    pkg = G.load_package()
    kind, dt = case.split("_")[0], case.split("_")[1]
    tdt = {"f64": torch.float64, "f32": torch.float32, "bf16": torch.bfloat16}[dt]
    g = torch.Generator(device="cuda").manual_seed(1)
    if case == "gpu_f32_colmajor" or kind == "host":        # host arrays column-major (what vbmf_set_Y takes without a copy)
        t = torch.randn(M, L, generator=g, device="cuda", dtype=torch.float32).to(tdt).t()
    else:
        t = torch.randn(L, M, generator=g, device="cuda", dtype=torch.float32).to(tdt)
    src = t if kind == "gpu" else t.cpu().numpy()
    if kind == "host":
        del t
        torch.cuda.empty_cache()
    out = dict(case=case, L=L, M=M, src_bytes=L * M * {"f64": 8, "f32": 4, "bf16": 2}[dt])
    for y, ydt, yb in (("f32", pkg.VBMF_Y_F32, 4), ("bf16", pkg.VBMF_Y_BF16, 2)):
        with pkg.capi.Context(L, M, H, y_dtype=ydt) as c:
            call = (lambda: c.set_Y(src)) if case == "host_f64_set_Y" else (lambda: c.set_Y_rows(src))
            call()
            wall, dev = [], []
            for _ in range(3):
                t0 = time.perf_counter()
                call()
                wall.append((time.perf_counter() - t0) * 1e3)
                dev.append(c.dims()["set_y_rows_us"] * 1e-3)
            out[y] = dict(wall_ms=wall, dev_ms=None if case == "host_f64_set_Y" else dev, bytes=out["src_bytes"] + 2 * L * M * yb,
                          trYY=c.trYY())
    print("RESULT " + json.dumps(out))


def run_child(case, L, lib=None):
    env = dict(os.environ)
    env.pop("VBMF_HIP_LIB", None)
    if lib:
        env["VBMF_HIP_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", case, "--rows", str(L)], env=env, capture_output=True,
                       text=True, timeout=LIMIT_S.get(case, 120))
    lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not lines:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"{case} ({lib or 'in-tree build'}) failed with status {r.returncode}: the run ends here")
    return json.loads(lines[-1][7:])


def host_rows():
    try:
        avail = next(int(l.split()[1]) * 1024 for l in open("/proc/meminfo") if l.startswith("MemAvailable"))
    except Exception:
        avail = 0
    return 100000 if avail >= 3 * 8e9 else 50000         # the fp64 array, its pageable staging and headroom


def fmt(v):
    return "[" + " ".join(f"{x:.3f}" for x in v) + "]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one")
    ap.add_argument("--rows", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "set_y_sources.txt"))
    ap.add_argument("--ab-lib")
    ap.add_argument("--lib", help="the build the table is measured on (default: the in-tree one)")
    a = ap.parse_args()
    if a.one:
        return child(a.one, a.rows)
    L = a.rows or host_rows()
    text = [f"Y by source at {L} x {M} (H = {H}), one MI355X, each case its own process: one warm call, then three timed ones (ms).",
            "wall: around the call, which returns after the context's stream is idle; device: between two HIP events on that stream",
            "(staged copies, tiling kernels, ||Y||^2; vbmf_set_Y carries no events).  bytes: source read once + both tiled copies written;",
            f"share: bytes / best device time (best wall time for vbmf_set_Y) as a share of the {COPY_RATE / 1e12:.1f} TB/s copy rate.",
            "" if L == 100000 else f"({L} rows: the host could not hold the 8 GB fp64 array of 100 000 rows with its staging)", ""]

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(text) + "\n")

    try:
        for case in CASES:
            r = run_child(case, L, os.path.abspath(a.lib) if a.lib else None)
            for y in ("f32", "bf16"):
                d = r[y]
                best = min(d["dev_ms"]) if d["dev_ms"] else min(d["wall_ms"])
                text.append(f"{case:18s} storage {y:4s} wall {fmt(d['wall_ms'])} device {fmt(d['dev_ms']) if d['dev_ms'] else 'n/a':28s} "
                            f"bytes {d['bytes'] / 1e9:6.2f} GB  share {d['bytes'] / (best * 1e-3) / COPY_RATE * 100:6.2f} %")
            flush()
        if a.ab_lib:
            lib = os.path.abspath(a.ab_lib)
            text += ["", "2a (--ab-lib: tile_y_kernel once per copy for every source) vs 2b (tile_pair_kernel, both copies from one read): device ms of",
                     "three timed calls per process, four rounds, the build that runs first alternating (2a first in rounds 1 and 3)", ""]
            res = {}
            for rnd in range(4):
                for arm in (("2a", "2b") if rnd % 2 == 0 else ("2b", "2a")):
                    for case in ("gpu_f32_rowmajor", "gpu_f32_colmajor"):
                        r = run_child(case, L, lib if arm == "2a" else None)
                        for y in ("f32", "bf16"):
                            res.setdefault((case, y, arm), []).append(min(r[y]["dev_ms"]))
                            text.append(f"round {rnd + 1} {arm} {case:18s} storage {y:4s} device {fmt(r[y]['dev_ms'])} wall {fmt(r[y]['wall_ms'])}")
                        flush()
            text.append("")
            keep = True
            for case in ("gpu_f32_rowmajor", "gpu_f32_colmajor"):
                for y in ("f32", "bf16"):
                    xa, xb = res[(case, y, "2a")], res[(case, y, "2b")]
                    wins = max(xb) < min(xa)
                    keep = keep and wins
                    text.append(f"[{case} storage {y}] 2a {min(xa):.3f}-{max(xa):.3f} ms, 2b {min(xb):.3f}-{max(xb):.3f} ms (best call of each round); "
                                f"2b's worst round {'beats' if wins else 'does not beat'} 2a's best round")
            text.append("decision: " + ("2b wins in every layout and storage type: tile_pair_kernel is kept for sources with a unit stride"
                                        if keep else "2b does not win everywhere: tile_pair_kernel is deleted, every source takes tile_y_kernel"))
    finally:
        flush()
        print("\n".join(text))


if __name__ == "__main__":
    main()
