"""Per-stage cost of `seg3d.py prepare` on one GPU, on two synthetic cases (tools/luna_prep_probe.py's form):

    brats   4 x 240 x 240 x 155 float32 at 1 mm, a zero background around an ellipsoid  -> crop to the non-zero box, z-score, 1 mm
    lits    1 x 512 x 512 x 300 int16 at 0.7 / 0.7 / 1.5 mm                             -> window normalisation, 1 / 1 / 1.5 mm

    python tools/bench_seg_prep.py [--runs 3] [--out profiles/seg_prep_bench.txt] [--no-cpu]

Stages are wall-clock with a device synchronisation after each (pcrlv2_amd/seg_prep.py's `timing`), median of --runs after a warm-up; files are in the
page cache, so `read` is not a cold disk.  The resample kernel alone is timed with events over 9 launches (median, min - max) and its algorithmic bytes
(the box of every channel and of the label volume read once, both outputs written once) are set against the 6.3 TB/s a copy achieves (DESIGN.md section
4.3).  The CPU line is scipy.ndimage.zoom in float64 (order 1 per channel, order 0 for the labels) plus the numpy normalisation, one thread.
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pcrlv2_amd import nifti, seg_prep as SP  # noqa: E402

COPY_TBS = 6.3


def make_case(kind):
    rng = np.random.default_rng(0)
    if kind == "brats":
        X, Y, Z, C = 240, 240, 155, 4
        g = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
        inside = ((g[0] - 77) / 68.0) ** 2 + ((g[1] - 120) / 95.0) ** 2 + ((g[2] - 120) / 80.0) ** 2 <= 1.0
        chans = [np.where(inside, rng.standard_normal((Z, Y, X), dtype=np.float32) * 100 + 400, 0).astype(np.float32) for _ in range(C)]
        seg = np.where(inside, rng.integers(0, 5, (Z, Y, X)), 0).astype(np.uint8)
        seg[seg == 3] = 0
        return chans, seg, (1.0, 1.0, 1.0), SP.PrepConfig(regions=SP.parse_regions("1,2,4;1,4;4"), spacing=(1.0, 1.0, 1.0), crop_nonzero=True, norm="zscore")
    X, Y, Z = 512, 512, 300
    chans = [rng.integers(-1000, 1500, (Z, Y, X)).astype(np.int16)]
    seg = rng.integers(0, 3, (Z, Y, X)).astype(np.uint8)
    return chans, seg, (0.7, 0.7, 1.5), SP.PrepConfig(regions=SP.parse_regions("1,2;2"), spacing=(1.0, 1.0, 1.5), crop_nonzero=False, norm="window",
                                                     window=(-100.0, 400.0), mean=100.0, std=80.0)


def cpu_restatement(chans, seg, box, out_shape, stats, cfg):
    import scipy.ndimage as ndi
    t0 = time.perf_counter()
    x0, x1, y0, y1, z0, z1 = box
    zoom = [o / n for o, n in zip(out_shape, (x1 - x0, y1 - y0, z1 - z0))]
    mask = None
    if cfg.crop_nonzero:
        mask = np.zeros(chans[0].shape, dtype=bool)
        for c in chans:
            mask |= c != 0
        mask = mask[z0:z1, y0:y1, x0:x1].transpose(2, 1, 0)
    for c, a in enumerate(chans):
        v = a[z0:z1, y0:y1, x0:x1].transpose(2, 1, 0).astype(np.float64)
        u = (np.clip(v, stats[c, 2], stats[c, 3]) - stats[c, 0]) / max(stats[c, 1], 1e-8)
        if mask is not None:
            u = np.where(mask, u, 0.0)
        ndi.zoom(u, zoom, order=1, mode="nearest", grid_mode=True)
    ndi.zoom(seg[z0:z1, y0:y1, x0:x1].transpose(2, 1, 0), zoom, order=0, mode="nearest", grid_mode=True)
    return (time.perf_counter() - t0) * 1e3


def bench(kind, runs, cpu, log):
    dev = torch.device("cuda", 0)
    chans, seg, spacing, cfg = make_case(kind)
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for c, a in enumerate(chans):
            paths.append(os.path.join(tmp, f"c{c}.nii"))
            nifti.write_nifti(paths[-1], a, spacing=spacing)
        nifti.write_nifti(os.path.join(tmp, "seg.nii"), seg, spacing=spacing)
        entry = ("case", os.path.join(tmp, "seg.nii"), paths)
        rows = []
        for r in range(runs + 1):
            t = {}
            t0 = time.perf_counter()
            ch, sg, sp, hdr = SP.read_case(entry)
            t["read"] = time.perf_counter() - t0
            res = SP.prepare_case(ch, sg, sp, cfg, dev, timing=t)
            t0 = time.perf_counter()
            SP.save_case(tmp, "case", res, hdr)
            t["write"] = time.perf_counter() - t0
            if r:
                rows.append(t)
    C, (Z, Y, X) = len(chans), chans[0].shape
    box, out_shape = [int(v) for v in res["meta"]["box"]], tuple(int(v) for v in res["meta"]["prep_shape"])
    log(f"{kind}: {C} x {X} x {Y} x {Z} {chans[0].dtype} at {spacing} mm, --norm {cfg.norm}, --crop_nonzero {int(cfg.crop_nonzero)}; box {box} -> {out_shape}, "
        f"tile {SP.resample_tile(box[1] - box[0], box[5] - box[4], out_shape[0], out_shape[2], cfg.crop_nonzero)}")
    log(f"per case, ms (median of {runs}, min - max):")
    total = []
    for key in ("read", "pack", "upload", "scan", "select", "stats", "resample", "download", "write"):
        vals = [row[key] * 1e3 for row in rows if key in row]
        if vals:
            log(f"  {key:<10}{statistics.median(vals):9.2f}   {min(vals):.2f} - {max(vals):.2f}")
            total.append(statistics.median(vals))
    log(f"  {'total':<10}{sum(total):9.2f}")
    # the resample kernel alone
    src = torch.from_numpy(np.stack(chans)).to(dev)
    lab = torch.from_numpy(seg).to(dev)
    b = (box[0], box[2], box[4], box[1] - box[0], box[3] - box[2], box[5] - box[4])
    ti, tw = (torch.from_numpy(a).to(dev) for a in SP.resample_tables(b[3:], out_shape))
    st = torch.from_numpy(np.ascontiguousarray(res["meta"]["stats"][:, :2])).to(dev)
    cl = torch.from_numpy(np.ascontiguousarray(res["meta"]["stats"][:, 2:])).to(dev) if cfg.norm in ("window", "percentile") else None
    reg = torch.from_numpy(SP.region_table(cfg.regions)).to(dev)
    img = torch.empty((C,) + out_shape, dtype=torch.float32, device=dev)
    out_lab = torch.empty(out_shape, dtype=torch.uint8, device=dev)
    ms = []
    for r in range(10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        SP.gpu_resample(src, lab, b, out_shape, ti, tw, st, cl, reg, len(cfg.regions), cfg.crop_nonzero, img, out_lab)
        e1.record()
        torch.cuda.synchronize()
        if r:
            ms.append(e0.elapsed_time(e1))
    nbox, OV = b[3] * b[4] * b[5], out_shape[0] * out_shape[1] * out_shape[2]
    nbytes = nbox * (C * chans[0].dtype.itemsize + 1) + OV * (C * 4 + 1)
    med = statistics.median(ms)
    log(f"resample kernel alone, 9 launches: median {med:.3f} ms ({min(ms):.3f} - {max(ms):.3f}); {nbytes / 1e6:.1f} MB algorithmic -> "
        f"{nbytes / med / 1e9:.3f} TB/s = {100 * nbytes / med / 1e9 / COPY_TBS:.1f} % of a copy's {COPY_TBS} TB/s")
    if cpu:
        log(f"float64 scipy / numpy restatement of normalise + resample on the CPU (one thread): {cpu_restatement(chans, seg, box, out_shape, res['meta']['stats'], cfg):.0f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log(f"device: {torch.cuda.get_device_name(0)}")
    for kind in ("brats", "lits"):
        bench(kind, args.runs, not args.no_cpu, log)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
