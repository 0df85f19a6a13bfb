"""Kernel times of the segmentation head from a profiler run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/bench_seg.py --only head --rounds 2 --window_ms 20
    python tools/seg_trace_summary.py OUT

Reads OUT/**/*kernel_trace.csv and prints, per (kernel, dtype, blocks), the median and the minimum duration over its launches; for the fused kernels
also the HBM bytes the kernel needs (tools/bench_seg.py's count) over the median, as TB/s and as a fraction of the 8 TB/s peak.  The sample count b is
the grid's y extent."""
import csv
import glob
import re
import statistics
import sys

VOXELS = 64 * 64 * 32
HBM = 8e12


def main(root):
    rows = {}
    for f in glob.glob(root + "/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"]
            m = re.search(r"(seg_head_\w+_kernel|to1_\w+?_kernel|sigmoid_\w+?_kernel)", name)
            if not m:
                continue
            dt = "bf16" if ("DF16b" in name or "bf16" in name) else ("f32" if re.search(r"_kernel(<float|If)", name) else "-")
            grid = (int(r["Grid_Size_X"]) // max(int(r["Workgroup_Size_X"]), 1), int(r["Grid_Size_Y"]))
            rows.setdefault((m.group(1), dt, grid), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for (kern, dt, grid), v in sorted(rows.items()):
        med = statistics.median(v)
        line = f"{med:9.1f} us  min {min(v):8.1f}  n={len(v):5d}  blocks={grid}  {dt:5s} {kern}"
        if kern in ("seg_head_fwd_kernel", "seg_head_bwd_kernel") and dt != "-":
            es = 2 if dt == "bf16" else 4
            need = grid[1] * VOXELS * ((64 * es + 1) if "fwd" in kern else (128 * es + 1))
            line += f"  needs {need / 1e6:.0f} MB: {need / med / 1e6:.2f} TB/s, {need / (med * 1e-6) / HBM:.2f} of peak"
        print(line)


if __name__ == "__main__":
    main(sys.argv[1])
