"""Measurements of DESIGN.md section 18 (connected-component clean-up on the device), one JSON line per measurement.

    python tools/bench_components.py [--rounds 5] [--sizes 128,128,64 240,240,155] [--out profiles/components_bench.txt]

One synthetic mask per size and kind, K = 3 classes.  `blobs`: nested ellipsoids with a rough rim and 0.1 % specks around them (a prediction);
`noise`: every class independent noise of density 0.3 (the 6-connected percolation threshold: the most and the most ragged components).
case     label plus filter (keep_largest and min_voxels 8) for all K classes, connectivity 6 and 26:
         (a) ops.label_components + ops.filter_components on the device (mask already uploaded; each class's call includes its one read-back of n);
         (b) scipy.ndimage.label + np.bincount + the same rule in numpy, one CPU thread.
         The two arms alternate inside one process, each warmed; a round is ONE call per arm; (a) between two device events (they span the host work of
         the call as well), (b) by time.perf_counter.  Reported: the median over the rounds and the spread (max - min); `holds`: (a) is faster by more
         than the larger spread.  The two arms' masks are compared (they must be equal).
kernels  pcrl_ccl_label (its six launches) and pcrl_ccl_filter (two) through the raw entry points into preallocated outputs, 20 launches queued back to
         back between two events.  floor_us: the bytes the pass must move (label: the mask in, int32 labels out = 5 V; filter: mask and labels in, mask
         out = 6 V) over the 6.3 TB/s a copy achieves.
speck    smooth ellipsoids (one component per class) against themselves displaced by 2 voxels; one voxel of class 0 set in the far corner of the
         prediction: HD95 / HD of train_seg.surface_metrics with the speck, after train_seg.postprocess_mask(keep_largest = all classes), and of the
         prediction that never had it; the cleaned mask must BE the speck-free one.

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
from pcrlv2_amd.train_seg import postprocess_mask, surface_metrics  # noqa: E402

K = 3
COPY_BW = 6.3e12
MIN_VOXELS = 8


def ellipsoids(shape, seed, shift=0, rim=0.03):
    """Class k is an ellipsoid of 0.8, 0.55, 0.3 of the half axes with a noisy rim (rim = 0: smooth, one component), displaced by `shift` voxels."""
    rng = np.random.default_rng(seed)
    ax = [(np.arange(n) - (n - 1) / 2) / (n / 2) for n in shape]
    r = np.sqrt(sum(np.roll(a, shift)[tuple(slice(None) if i == j else None for j in range(3))] ** 2 for i, a in enumerate(ax)))
    r = r + rim * rng.standard_normal(shape)
    m = np.zeros(shape, np.uint8)
    for k, rad in enumerate((0.8, 0.55, 0.3)):
        m |= ((r < rad).astype(np.uint8) << k).astype(np.uint8)
    return m


def make_mask(kind, shape, seed):
    rng = np.random.default_rng(seed + 100)
    if kind == "blobs":
        m = ellipsoids(shape, seed)
        for k in range(K):
            m |= ((rng.random(shape) < 0.001).astype(np.uint8) << k).astype(np.uint8)
        return m
    m = np.zeros(shape, np.uint8)
    for k in range(K):
        m |= ((rng.random(shape) < 0.3).astype(np.uint8) << k).astype(np.uint8)
    return m


def scipy_clean(mask, conn):
    from scipy import ndimage as ndi
    st = ndi.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[conn])
    out = mask.copy()
    comps = []
    for k in range(K):
        labels, n = ndi.label(mask >> k & 1, structure=st)
        sizes = np.bincount(labels.ravel(), minlength=n + 1)
        comps.append(n)
        keep = np.zeros(n + 1, dtype=bool)
        if n:
            w = 1 + int(np.argmax(sizes[1:]))
            keep[w] = sizes[w] >= MIN_VOXELS
        out[(labels > 0) & ~keep[labels]] &= np.uint8(~(1 << k) & 0xFF)
    return out, comps


def device_clean(dm, conn):
    for k in range(K):
        labels, sizes = ops.label_components(dm, k, conn)
        dm = ops.filter_components(dm, labels, sizes, k, keep_largest=True, min_voxels=MIN_VOXELS)
    return dm


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
        raise SystemExit("tools/bench_components.py measures on the GPU; none is visible")
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    emit({"bench": "device", "name": torch.cuda.get_device_name(0), "rounds": args.rounds, "K": K, "tile": ops.ccl_tile(), "min_voxels": MIN_VOXELS})
    L, s_ = lib(), stream_handle()
    for size in args.sizes:
        shape = tuple(int(v) for v in size.split(","))
        V = int(np.prod(shape))
        for kind in ("blobs", "noise"):
            mask = make_mask(kind, shape, 7)
            dm = torch.from_numpy(mask).cuda()
            for conn in (6, 26):
                dev = device_clean(dm, conn).cpu().numpy()          # warm both arms
                cpu, comps = scipy_clean(mask, conn)
                t_dev, t_cpu = [], []
                for r in range(args.rounds):
                    t_dev.append(event_ms(lambda: device_clean(dm, conn)))
                    t0 = time.perf_counter()
                    scipy_clean(mask, conn)
                    t_cpu.append((time.perf_counter() - t0) * 1e3)
                    print(f"# {kind} {shape} connectivity {conn} round {r}: device {t_dev[-1]:.2f} ms, scipy {t_cpu[-1]:.0f} ms", flush=True)
                (md, sd), (mc, sc) = med(t_dev), med(t_cpu)
                emit({"bench": "case", "shape": shape, "mask": kind, "connectivity": conn, "device_ms": md, "device_spread_ms": sd, "scipy_ms": mc,
                      "scipy_spread_ms": sc, "ratio": round(mc / md, 1), "holds": mc - md > max(sd, sc), "components": comps,
                      "masks_equal": bool(np.array_equal(dev, cpu))})

                # the kernels on their own, class 0
                labels = torch.empty(shape, dtype=torch.int32, device="cuda")
                sizes = torch.empty((V + 1) // 2, dtype=torch.int32, device="cuda")
                n = torch.zeros(1, dtype=torch.int32, device="cuda")
                out = torch.empty_like(dm)
                nws = L.call("pcrl_ccl_ws_bytes", *shape)
                ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
                fws = torch.empty(L.call("pcrl_ccl_filter_ws_bytes"), dtype=torch.uint8, device="cuda")
                kernels = {
                    "ccl_label": (lambda: L.call("pcrl_ccl_label", dm, 0, conn, labels, sizes, n, ws, nws, *shape, s_), 5 * V),
                    "ccl_filter": (lambda: L.call("pcrl_ccl_filter", dm, labels, sizes, n, out, 0, 1, MIN_VOXELS, fws, fws.numel(), *shape, s_), 6 * V),
                }
                for fn, _ in kernels.values():
                    fn()
                ms = {k: [] for k in kernels}
                for _ in range(args.rounds):
                    for k, (fn, _) in kernels.items():
                        ms[k].append(event_ms(fn, 20))
                for k, (_, need) in kernels.items():
                    m, s = med(ms[k])
                    emit({"bench": "kernel", "shape": shape, "mask": kind, "connectivity": conn, "kernel": k, "ms": m, "spread_ms": s, "bytes_needed": need,
                          "floor_us": round(need / COPY_BW * 1e6, 2), "of_copy": round(need / (m * 1e-3) / COPY_BW, 4)})

        # the speck
        gt, pred = ellipsoids(shape, 7, shift=2, rim=0.0), ellipsoids(shape, 7, rim=0.0)
        speck = pred.copy()
        speck[-1, -1, -1] |= 1
        dg = torch.from_numpy(gt).cuda()
        cleaned = postprocess_mask(torch.from_numpy(speck).cuda(), K, range(K))[0]
        rows = {}
        for tag, p in (("with_speck", torch.from_numpy(speck).cuda()), ("cleaned", cleaned), ("never_had_it", torch.from_numpy(pred).cuda())):
            m = surface_metrics(p, dg, K)
            rows[tag] = {"hd95": [round(float(v), 4) for v in m["hd95"]], "hd": [round(float(v), 4) for v in m["hd"]]}
        emit({"bench": "speck", "shape": shape, **rows, "cleaned_mask_is_the_speck_free_mask": bool(np.array_equal(cleaned.cpu().numpy(), pred))})
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
