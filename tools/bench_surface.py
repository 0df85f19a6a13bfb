"""Measurements of DESIGN.md section 17 (surface-distance metrics on the device), one JSON line per measurement.

    python tools/bench_surface.py [--rounds 5] [--sizes 128,128,64 240,240,155] [--out profiles/surface_bench.txt]

One synthetic case per size, K = 3 nested, slightly displaced ellipsoids with a rough rim (tumour-like regions), spacing (1, 1, 1).
case     (a) train_seg.surface_metrics on the device (masks already uploaded; the call includes its one read-back and the host's finish);
         (b) the scipy route of MedPy: per class binary_erosion of both masks, two distance_transform_edt, np.percentile / max / means, one CPU thread.
         The two arms alternate inside one process, each warmed; a round is ONE call per arm; (a) between two device events (they span the host work of
         the call as well), (b) by time.perf_counter.  Reported: the median over the rounds and the spread (max - min).  Condition: (a) is faster by more
         than the larger spread.  The two arms' metrics are compared as well (they are the same numbers up to the rounding of ASSD's sums).
kernels  pcrl_surf_extract, pcrl_edt_sq (its three launches; per pass and in all) and pcrl_surf_dist_stats through the raw entry points into
         preallocated outputs, 20 launches queued back to back between two events.  Bytes needed (every input once, every output once per launch
         of a kernel) over the time, against the 6.3 TB/s a copy achieves; for the line passes also the scan steps per voxel actually executed
         (pcrl_edt_sq's `steps`; a step is two multiplications, up to two additions and up to three comparisons in float64).

A run without a GPU fails: nothing here is an estimate.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pcrlv2_amd import ops  # noqa: E402
from pcrlv2_amd._lib import lib, stream_handle  # noqa: E402
from pcrlv2_amd.train_seg import surface_metrics  # noqa: E402

K = 3
COPY_BW = 6.3e12


def phantom(shape, seed):
    """-> (pred, gt) uint8 bitmasks: class k is an ellipsoid of 0.8, 0.55, 0.3 of the half axes with a noisy rim; the prediction is displaced by 2 voxels."""
    rng = np.random.default_rng(seed)
    ax = [(np.arange(n) - (n - 1) / 2) / (n / 2) for n in shape]
    out = []
    for shift in (0, 2):
        r = np.sqrt(sum(np.roll(a, shift)[tuple(slice(None) if i == j else None for j in range(3))] ** 2 for i, a in enumerate(ax)))
        r = r + 0.03 * rng.standard_normal(shape)
        m = np.zeros(shape, np.uint8)
        for k, rad in enumerate((0.8, 0.55, 0.3)):
            m |= ((r < rad).astype(np.uint8) << k).astype(np.uint8)
        out.append(m)
    return out[0], out[1]


def scipy_metrics(pred, gt, spacing, q=0.95):
    from scipy import ndimage as ndi
    cross = ndi.generate_binary_structure(3, 1)
    res = {"hd95": [], "hd": [], "assd": []}
    for k in range(K):
        p, g = (pred >> k & 1).astype(bool), (gt >> k & 1).astype(bool)
        sp, sg = p & ~ndi.binary_erosion(p, cross), g & ~ndi.binary_erosion(g, cross)
        a = ndi.distance_transform_edt(~sg, sampling=spacing)[sp]
        b = ndi.distance_transform_edt(~sp, sampling=spacing)[sg]
        u = np.concatenate([a, b])
        res["hd95"].append(float(np.percentile(u, 100 * q)))
        res["hd"].append(float(u.max()))
        res["assd"].append(float((a.mean() + b.mean()) / 2))
    return res


def event_ms(fn, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def med(v):
    return round(float(np.median(v)), 4), round(float(max(v) - min(v)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", nargs="+", default=["128,128,64", "240,240,155"])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_surface.py measures on the GPU; none is visible")
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    emit({"bench": "device", "name": torch.cuda.get_device_name(0), "rounds": args.rounds, "K": K})
    spacing = (1.0, 1.0, 1.0)
    L, s_ = lib(), stream_handle()
    for size in args.sizes:
        shape = tuple(int(v) for v in size.split(","))
        V = int(np.prod(shape))
        pred, gt = phantom(shape, 7)
        dp, dg = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
        dev = surface_metrics(dp, dg, K, spacing)          # warm both arms
        cpu = scipy_metrics(pred, gt, spacing)
        t_dev, t_cpu = [], []
        for r in range(args.rounds):
            t_dev.append(event_ms(lambda: surface_metrics(dp, dg, K, spacing)))
            t0 = time.perf_counter()
            scipy_metrics(pred, gt, spacing)
            t_cpu.append((time.perf_counter() - t0) * 1e3)
            print(f"# round {r}: device {t_dev[-1]:.2f} ms, scipy {t_cpu[-1]:.0f} ms", flush=True)
        (md, sd), (mc, sc) = med(t_dev), med(t_cpu)
        agree = {k: float(np.max(np.abs(np.asarray(cpu[k]) - dev[k]) / np.maximum(np.asarray(cpu[k]), 1e-300))) for k in cpu}
        emit({"bench": "case", "shape": shape, "device_ms": md, "device_spread_ms": sd, "scipy_ms": mc, "scipy_spread_ms": sc, "ratio": round(mc / md, 1),
              "holds": mc - md > max(sd, sc), "surface_voxels": [int(v) for v in dev["n_pred"] + dev["n_gt"]], "hd95": dev["hd95"].tolist(),
              "max_relative_difference_to_scipy": agree})

        # the kernels on their own
        sp, sg, counts = ops.surf_extract(dp, dg, K)
        d2g, d2p = torch.empty(shape, dtype=torch.float64, device="cuda"), torch.empty(shape, dtype=torch.float64, device="cuda")
        steps = torch.zeros(1, dtype=torch.int64, device="cuda")
        rec = torch.zeros(8, dtype=torch.int64, device="cuda")
        nws = L.call("pcrl_surf_dist_stats_ws_bytes", V)
        ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
        bit = 1
        ops.edt_sq(sp, bit, spacing, out=d2p)
        n_surf = int(((sp >> bit) & 1).sum() + ((sg >> bit) & 1).sum())
        L.call("pcrl_edt_sq", sg, bit, d2g, *spacing, steps, None, 0, *shape, s_)
        per_voxel = int(steps) / V
        kernels = {
            "surf_extract": (lambda: L.call("pcrl_surf_extract", dp, dg, sp, sg, counts, *shape, K, s_), 4 * V),
            "edt_sq_three_passes": (lambda: L.call("pcrl_edt_sq", sg, bit, d2g, *spacing, None, None, 0, *shape, s_), V + 8 * V + 4 * 8 * V),
            "surf_dist_stats_nine_passes": (lambda: L.call("pcrl_surf_dist_stats", d2g, sp, d2p, sg, bit, 0.95, rec, ws, nws, V, s_), 9 * (2 * V + 8 * n_surf)),
        }
        for fn, _ in kernels.values():
            fn()
        ms = {k: [] for k in kernels}
        for _ in range(args.rounds):
            for k, (fn, _) in kernels.items():
                ms[k].append(event_ms(fn, 20))
        for k, (_, need) in kernels.items():
            m, s = med(ms[k])
            out = {"bench": "kernel", "shape": shape, "kernel": k, "ms": m, "spread_ms": s, "bytes_needed": need, "TBps": round(need / (m * 1e-3) / 1e12, 3),
                   "of_copy": round(need / (m * 1e-3) / COPY_BW, 3)}
            if k.startswith("edt"):
                out.update(scan_steps_per_voxel=round(per_voxel, 2), float64_mul_add_per_voxel=round(4 * per_voxel, 1),
                           Gsteps_per_s=round(int(steps) / (m * 1e-3) / 1e9, 1))
            emit(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
