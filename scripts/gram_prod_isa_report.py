"""Loop-body census of the gram_prod_kernel instantiations from hipcc's assembly (no GPU needed).

    cat > gp.hip <<'X'
    #include <hip/hip_runtime.h>
    #include "gram_kernels.hpp"
    template __global__ void vbmf::gram_prod_kernel<1>(const float4*, const uint4*, float*, int, int, int, int, long long, long long, const int*);
    template __global__ void vbmf::gram_prod_kernel<2>(const float4*, const uint4*, float*, int, int, int, int, long long, long long, const int*);
    template __global__ void vbmf::gram_prod_kernel<4>(const float4*, const uint4*, float*, int, int, int, int, long long, long long, const int*);
    template __global__ void vbmf::gram_prod_kernel<4, 8>(const float4*, const uint4*, float*, int, int, int, int, long long, long long, const int*);
    X
    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S -Ivbmatrixfactorization.jl_amd/csrc -Iinclude gp.hip -o gp.s
    python scripts/gram_prod_isa_report.py gp.s

Per instantiation: registers, scratch, occupancy, and every innermost loop that holds a barrier and MFMAs (the steady k-loop)
counted by instruction class (LDS-DMA pieces and loads to registers apart), with its s_waitcnt in program order, the count of what
a register ring of G must not bring back (v_mov ring copies, v_pk_add_f32, a vmcnt(0) in the loop), and the whole kernel's
vector-memory stream by barrier, tail body included (profiles/gram_prod_overlap_isa.txt, profiles/gram_prod_regring_isa.txt)."""
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
        elif o.startswith("global_load") or o.startswith("buffer_load"):
            dma = sum(1 for x in ins if x.split()[0] == o and x.split()[-1] == "lds")
            if dma: cls["LDS-DMA pieces"] += dma
            if c - dma: cls["loads to registers"] += c - dma
        elif o.startswith("s_waitcnt"): cls["s_waitcnt"] += c
        elif o.startswith("s_barrier"): cls["s_barrier"] += c
        elif o.startswith("s_"): cls["SALU/other scalar"] += c
        else: cls[o] += c
    print(f"  steady loop body: {len(ins)} instructions; " + ", ".join(f"{k} {v}" for k, v in sorted(cls.items())))
    valu = {o: c for o, c in ops.items() if o.startswith("v_") and not o.startswith("v_mfma")}
    print("    VALU mix: " + ", ".join(f"{c} {o}" for o, c in sorted(valu.items(), key=lambda t: -t[1])))
    waits = [x for x in ins if x.startswith("s_waitcnt")]
    print("    waits in order: " + " | ".join(w.replace("s_waitcnt ", "") for w in waits))
    # what a register ring must not bring back (profiles/gram_prod_overlap_isa.txt, parent: ring copies and a drained back edge)
    bad = {k: ops.get(k, 0) for k in ("v_mov_b32_e32", "v_mov_b64_e32", "v_pk_add_f32")}
    bad["vmcnt(0)"] = sum(1 for w in waits if re.search(r"vmcnt\(0\)", w))
    print("    ring copies / packed adds / drains: " + ", ".join(f"{k} {v}" for k, v in bad.items()))


def stream(lines):
    """The kernel's vector-memory stream in text order, one group per barrier: P = LDS-DMA piece, R = load to registers, each run
    counted, then the vmcnt of the wait in front of the barrier.  Blocks a branch may skip hold no loads, so text order is issue
    order; a counted wait in front of a barrier must find its chunk's pieces (P) ahead of exactly that many register loads."""
    out, cur, last_wait = [], [], None
    for l in lines:
        x = l.split("//")[0].split(";")[0].strip()
        if not x: continue
        if x.startswith("buffer_load"):
            k = "P" if x.split()[-1] == "lds" else "R"
            if cur and cur[-1][0] == k: cur[-1][1] += 1
            else: cur.append([k, 1])
        elif x.startswith("s_waitcnt") and "vmcnt" in x:
            last_wait = re.search(r"vmcnt\((\d+)\)", x).group(1)
        elif x.startswith("s_barrier"):
            out.append(" ".join(f"{k}{n}" for k, n in cur) + f" [vmcnt({last_wait})]")
            cur = []
        elif x.startswith(".LBB") or re.match(r"s_c?branch", x):
            if cur and cur[-1][0] != "/": cur.append(["/", 0])
    print("    memory stream by barrier (text order; / = block edge): " + " | ".join(o.replace("/0", "/") for o in out))


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
    stream(lines)
