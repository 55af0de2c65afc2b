#!/usr/bin/env python3
"""Turn gpurun_out/prof_<tag>/ (tools/profile_bench.sh) into the committed summaries under profiles/."""
import collections
import csv
import glob
import json
import os
import sys

tag = sys.argv[1] if len(sys.argv) > 1 else "r01"
src = f"gpurun_out/prof_{tag}"
os.makedirs("profiles", exist_ok=True)


def short(n):
    n = n.replace("void ", "").replace("s3d::(anonymous namespace)::", "").replace("at::native::", "").replace("(anonymous namespace)::", "")
    return n.split("(")[0][:80]


stats = glob.glob(f"{src}/trace/*/*kernel_stats.csv")[0]
rows = list(csv.DictReader(open(stats)))
tot = sum(float(r["TotalDurationNs"]) for r in rows)
with open(f"profiles/{tag}_kernel_stats.csv", "w") as f:
    w = csv.writer(f)
    w.writerow(["kernel", "calls", "total_ms", "avg_us", "min_us", "max_us", "pct"])
    for r in rows:
        w.writerow([short(r["Name"]), r["Calls"], f"{float(r['TotalDurationNs'])/1e6:.3f}", f"{float(r['AverageNs'])/1e3:.2f}",
                    f"{float(r['MinNs'])/1e3:.2f}", f"{float(r['MaxNs'])/1e3:.2f}", r["Percentage"]])

# timed region = the last 32 training steps: one k_march_count_wave per step
trace = glob.glob(f"{src}/trace/*/*kernel_trace.csv")[0]
ks = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(trace)))
march = [i for i, k in enumerate(ks) if "k_march_count" in k[2]]
# graph mode: bench.py runs 34 extra eager steps (2 discarded + 32) after the timed region for its per-kernel timers; skip them
log = open(f"{src}/trace.log").read()
tail = 34 if '"launch": "hip-graph replay' in log else 0
sel = ks[march[-32 - tail]:(march[-tail] if tail else len(ks))]
agg, cnt = collections.Counter(), collections.Counter()
for s, e, n in sel:
    agg[short(n)] += e - s
    cnt[short(n)] += 1
window = sel[-1][1] - sel[0][0]
busy = sum(agg.values())


def pmc(kind, counter):
    fs = glob.glob(f"{src}/{kind}/*/*counter_collection.csv")
    if not fs:
        return {}
    acc, num = collections.Counter(), collections.Counter()
    for r in csv.DictReader(open(fs[0])):
        if r["Counter_Name"] == counter:
            acc[short(r["Kernel_Name"])] += float(r["Counter_Value"])
            num[short(r["Kernel_Name"])] += 1
    return {k: acc[k] / num[k] for k in acc}


fetch, write = pmc("fetch", "FETCH_SIZE"), pmc("write", "WRITE_SIZE")
sq = {c: pmc("sq", c) for c in ("SQ_WAVES", "SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_LDS", "SQ_WAVE_CYCLES", "SQ_WAIT_INST_ANY",
                                 "SQ_WAIT_ANY", "SQ_INSTS_VMEM_RD")}
mf = {c: pmc("mfma", c) for c in ("SQ_INSTS_VALU_MFMA_MOPS_F16", "SQ_VALU_MFMA_BUSY_CYCLES", "SQ_BUSY_CYCLES", "SQ_INSTS_MFMA", "GRBM_GUI_ACTIVE")}
ca = {c: pmc("cache", c) for c in ("TCP_TOTAL_CACHE_ACCESSES_sum", "TCP_TCC_READ_REQ_sum", "TCC_HIT_sum", "TCC_MISS_sum", "TCC_REQ_sum")}
with open(f"profiles/{tag}_timed_region.md", "w") as f:
    f.write(f"# rocprofv3 summary `{tag}` — `python bench.py --full --steps 32 --warmup 8 --no_cpu_baseline --no_render --no_seal --no_long_run`\n\n")
    import hashlib
    digest = hashlib.sha256(open("seal-3d_amd/csrc/gridencoder.hip", "rb").read()).hexdigest()[:16]
    f.write(f"Measured on gridencoder.hip sha256:{digest} (bench.py quotes `roofline.traffic` from this file only while the source "
            "still has this digest).\n\n")
    f.write(f"Timed region (last 32 steps, profiler attached): {window/1e6/32:.3f} ms/step wall, GPU busy {busy/1e6/32:.3f} ms/step "
            f"({100*busy/window:.0f} %), {len(sel)/32:.0f} kernel launches/step.\n\n")
    f.write("FETCH_SIZE / WRITE_SIZE are per-dispatch averages over the WHOLE run (KiB, raw counter values; on gfx950 FETCH_SIZE "
            "under-reports wide coalesced reads by 2x — MI355X_MICROARCH.md §HBM — the `x2` column applies that correction).\n\n")
    f.write("| kernel | launches/step | us/launch | us/step | FETCH KiB | FETCH x2 KiB | WRITE KiB | VALU insts/wave | wait_any % |\n|---|---|---|---|---|---|---|---|---|\n")
    for n, v in agg.most_common(24):
        wv = sq["SQ_WAVES"].get(n)
        valu = sq["SQ_INSTS_VALU"].get(n)
        wc, wa = sq["SQ_WAVE_CYCLES"].get(n), sq["SQ_WAIT_ANY"].get(n)
        f.write(f"| `{n}` | {cnt[n]/32:.1f} | {v/cnt[n]/1e3:.1f} | {v/32/1e3:.1f} | {fetch.get(n, float('nan')):.0f} | "
                f"{2*fetch.get(n, float('nan')):.0f} | {write.get(n, float('nan')):.0f} | "
                f"{(valu/wv if wv and valu else float('nan')):.0f} | {(100*wa/wc if wc and wa else float('nan')):.0f} |\n")
    # ---- matrix-core utilisation of the MLP kernels
    # SQ_INSTS_VALU_MFMA_MOPS_F16: 512 flop per count (rocprofiler's MOPS unit); SQ_VALU_MFMA_BUSY_CYCLES: cycles the matrix
    # pipes were busy, summed over the chip's 1,024 SIMDs (32 cycles per v_mfma_f32_32x32x16_f16, MI355X_MICROARCH.md);
    # utilisation = busy cycles / (1,024 SIMDs x kernel duration x the shader clock read from GRBM_GUI_ACTIVE (8 XCDs)).
    rows = [(n, v) for n, v in agg.most_common(40) if "ffmlp" in n and mf["SQ_VALU_MFMA_BUSY_CYCLES"].get(n)]
    if rows:
        f.write("\n## Matrix cores (ffmlp kernels)\n\n| kernel | us/launch | MFMA insts | TFLOP/s (MOPS x 512) | frac of 2.5 PF | MFMA busy cycles / SIMD | matrix-pipe utilisation |\n|---|---|---|---|---|---|---|\n")
        for n, v in rows:
            us = v / cnt[n] / 1e3
            mops = mf["SQ_INSTS_VALU_MFMA_MOPS_F16"].get(n, float("nan"))
            busy = mf["SQ_VALU_MFMA_BUSY_CYCLES"].get(n, float("nan"))
            gui = mf["GRBM_GUI_ACTIVE"].get(n, float("nan")) / 8.0  # cycles the kernel was resident, per XCD
            tf = mops * 512 / (us * 1e-6) / 1e12
            f.write(f"| `{n[:70]}` | {us:.1f} | {mf['SQ_INSTS_MFMA'].get(n, float('nan')):.0f} | {tf:.1f} | {tf/2500:.3f} | {busy/1024:.0f} | {busy/1024/gui:.3f} |\n")
    rows = [(n, v) for n, v in agg.most_common(40) if ("k_grid" in n or "k_bin" in n) and ca["TCC_REQ_sum"].get(n)]
    if rows:
        f.write("\n## L1 / L2 traffic of the grid kernels (per launch)\n\n| kernel | us/launch | TCP accesses | TCP->TCC read requests | TCC requests | TCC hit rate | TCC requests/us |\n|---|---|---|---|---|---|---|\n")
        for n, v in rows:
            us = v / cnt[n] / 1e3
            hit, miss = ca["TCC_HIT_sum"].get(n, 0.0), ca["TCC_MISS_sum"].get(n, 0.0)
            f.write(f"| `{n[:70]}` | {us:.1f} | {ca['TCP_TOTAL_CACHE_ACCESSES_sum'].get(n, float('nan')):.3g} | {ca['TCP_TCC_READ_REQ_sum'].get(n, float('nan')):.3g} | "
                    f"{ca['TCC_REQ_sum'][n]:.3g} | {hit / max(hit + miss, 1):.3f} | {ca['TCC_REQ_sum'][n] / us:.3g} |\n")
print(open(f"profiles/{tag}_timed_region.md").read())
