"""Loop-body census of the gram_prod_kernel instantiations from hipcc's assembly (no GPU needed).

    cat > gp.hip <<'X'
    #include <hip/hip_runtime.h>
    #include "gram_kernels.hpp"
    template __global__ void vbmf::gram_prod_kernel<1>(const float4*, const uint4*, float*, int, int, int, int, long long, long long, const int*);
    template __global__ void vbmf::gram_prod_kernel<2>(const float4*, const uint4*, float*, int, int, int, int, long long, long long, const int*);
    template __global__ void vbmf::gram_prod_kernel<4>(const float4*, const uint4*, float*, int, int, int, int, long long, long long, const int*);
    X
    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S -Ivbmatrixfactorization.jl_amd/csrc -Iinclude gp.hip -o gp.s
    python scripts/gram_prod_isa_report.py gp.s

Per instantiation: registers, scratch, occupancy, and every innermost loop that holds a barrier and MFMAs (the steady k-loop)
counted by instruction class, with its s_waitcnt in program order (profiles/gram_prod_overlap_isa.txt)."""
import re, sys, collections
src = open(sys.argv[1]).read()


def report(seg):
    ins = [x.split("//")[0].split(";")[0].strip() for x in seg]
    ins = [x for x in ins if x and not x.endswith(":") and not x.startswith(".")]
    ops = collections.Counter(x.split()[0] for x in ins)
    cls = collections.Counter()
    for o, c in ops.items():
        if o.startswith("v_mfma"): cls["MFMA"] += c
        elif o.startswith("v_"): cls["VALU"] += c
        elif o.startswith("ds_read") or o.startswith("ds_load"): cls["LDS read"] += c
        elif o.startswith("ds_"): cls["LDS write"] += c
        elif o.startswith("global_load") or o.startswith("buffer_load"): cls["global/buffer load" + (" (to LDS)" if any(("lds" in x) for x in ins if x.startswith(o)) else "")] += c
        elif o.startswith("s_waitcnt"): cls["s_waitcnt"] += c
        elif o.startswith("s_barrier"): cls["s_barrier"] += c
        elif o.startswith("s_"): cls["SALU/other scalar"] += c
        else: cls[o] += c
    print(f"  steady loop body: {len(ins)} instructions; " + ", ".join(f"{k} {v}" for k, v in sorted(cls.items())))
    valu = {o: c for o, c in ops.items() if o.startswith("v_") and not o.startswith("v_mfma")}
    print("    VALU mix: " + ", ".join(f"{c} {o}" for o, c in sorted(valu.items(), key=lambda t: -t[1])))
    waits = [x for x in ins if x.startswith("s_waitcnt")]
    print("    waits in order: " + " | ".join(w.replace("s_waitcnt ", "") for w in waits))


for m in re.finditer(r"^(_ZN4vbmf16gram_prod_kernel\w+):[^\n]*\n(.*?\n; Occupancy: \d+)", src, re.S | re.M):
    name, body = m.group(1), m.group(2)
    inst = re.findall(r"Li(\d+)E", name.split("EvPK")[0])
    lines = body.split("\n")
    meta = {k: re.search(r"\.amdhsa_" + k + r"\s+(\S+)", body) for k in ("next_free_vgpr", "accum_offset", "private_segment_fixed_size", "group_segment_fixed_size")}
    meta = {k: (v.group(1) if v else None) for k, v in meta.items()}
    cm = {k: re.search(r"; " + k + r":\s*(\d+)", body) for k in ("NumVgprs", "NumAgprs", "TotalNumVgprs", "ScratchSize", "Occupancy")}
    cm = {k: (v.group(1) if v else None) for k, v in cm.items()}
    labels = {}
    for i, l in enumerate(lines):
        lm = re.match(r"^(\.LBB\d+_\d+):", l)
        if lm: labels[lm.group(1)] = i
    segs = []
    for i, l in enumerate(lines):
        bm = re.match(r"\s+s_cbranch_\w+\s+(\.LBB\d+_\d+)", l) or re.match(r"\s+s_branch\s+(\.LBB\d+_\d+)", l)
        if bm and bm.group(1) in labels and labels[bm.group(1)] < i:
            seg = lines[labels[bm.group(1)]:i + 1]
            if any("s_barrier" in x for x in seg) and any("v_mfma" in x for x in seg): segs.append(seg)
    # innermost loops that hold a barrier and MFMAs: the steady loop(s) of the k-steps
    segs = [x for x in segs if not any(y is not x and len(y) < len(x) and y[0] in x for y in segs)]
    print(f"gram_prod_kernel<{inst}>: {cm}")
    for seg in segs:
        report(seg)
