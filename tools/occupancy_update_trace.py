"""The launches of one occupancy-grid update, out of a rocprofv3 kernel trace of bench.py.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python bench.py --steps 64 --warmup 16 --no_cpu_baseline ...
    python tools/occupancy_update_trace.py DIR [--windows 4]

A training step starts with the marcher's count kernel and ends with `k_step_epilogue`; an update window is the stretch
between a step's last kernel and the next step's first one that holds a `k_sweep_*` launch.  Prints (markdown) the launches
of the last window — name, start offset, duration, gap to the previous launch — and, for the last `--windows` windows, the
launch count, the summed kernel time, the wall time of the window and the idle time between the update's last launch and
the first kernel of the next step."""
import argparse
import csv
import glob
import os
import re


def load(trace_dir):
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    return rows


def short(name):
    name = re.sub(r"^void\s+", "", name)
    m = re.search(r"(k_[a-z0-9_]+)", name)
    if m and (name.startswith("_Z") or name.startswith("s3d::")):
        return m.group(1)
    return name[:70]


def windows(rows):
    out, i = [], 0
    starts = [k for k, r in enumerate(rows) if "k_march_count" in r[2]]
    for s in starts:
        # walk back from the step's first kernel to the previous step's last one
        j = s - 1
        while j >= 0 and "k_step_epilogue" not in rows[j][2] and "k_march_count" not in rows[j][2]:
            j -= 1
        if j < 0 or "k_step_epilogue" not in rows[j][2]:
            continue
        body = rows[j + 1:s]
        if any("k_sweep" in b[2] for b in body):
            out.append((rows[j], body, rows[s]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace_dir")
    ap.add_argument("--windows", type=int, default=4)
    args = ap.parse_args()
    rows = load(args.trace_dir)
    wins = windows(rows)[-args.windows:]
    if not wins:
        raise SystemExit("no update window found in the trace")
    prev, body, nxt = wins[-1]
    print("| # | kernel | start us | us | gap before us |")
    print("|---|---|---|---|---|")
    t0, last_end = prev[1], prev[1]
    for n, (a, b, name) in enumerate(body):
        print(f"| {n} | `{short(name)}` | {(a - t0) / 1e3:.1f} | {(b - a) / 1e3:.1f} | {(a - last_end) / 1e3:.1f} |")
        last_end = max(last_end, b)
    print()
    print("| window | launches | kernel time us | wall us (step end -> next step start) | idle after the update us |")
    print("|---|---|---|---|---|")
    for n, (prev, body, nxt) in enumerate(wins):
        busy = sum(b - a for a, b, _ in body) / 1e3
        # the update ends with its last native launch (k_sweep_* / k_packbits*); staging launches of the next step follow
        last = max((k for k, b in enumerate(body) if "k_sweep" in b[2] or "k_packbits" in b[2]), default=len(body) - 1)
        print(f"| {n} | {len(body)} | {busy:.1f} | {(nxt[0] - prev[1]) / 1e3:.1f} | {(nxt[0] - body[last][1]) / 1e3:.1f} |")


if __name__ == "__main__":
    main()
