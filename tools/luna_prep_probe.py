"""Per-series cost of the LUNA16 pre-processing (pcrlv2_amd/luna_prep.py) on one synthetic LUNA-shaped series: 512 x 512 x 300 int16 at
spacing 0.7 / 0.7 / 1.25 mm (358 x 358 x 375 after resampling), `--scale` pairs.  Reports read, upload, resample, window launches (with the
attempts per accepted pair of this phantom), download and write, then the float64 restatement's CPU time (tests/luna_prep_reference.py)
for the same resample and the same evaluated attempts.  The acceptance rate is the synthetic phantom's; real LUNA series differ.

    python tools/luna_prep_probe.py [--scale 16] [--attempts-per-launch 16] [--repeats 3] [--no-cpu]
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from pcrlv2_amd import luna_prep as P  # noqa: E402

SHAPE_ZYX = (300, 512, 512)
SPACING = (0.7, 0.7, 1.25)
NAME = "1.3.6.1.4.1.14519.5.2.1.6279.6001.999"


def phantom(seed=0):
    """Body wall tissue, two lungs at about -850 HU with soft tissue between them, vessels, noise, -3024 outside the field of view."""
    rng = np.random.default_rng(seed)
    Z, Y, X = SHAPE_ZYX
    z, y, x = np.ogrid[0:Z, 0:Y, 0:X]
    v = np.full(SHAPE_ZYX, 40, dtype=np.int16)
    ax = np.abs(x - X / 2)
    v[np.broadcast_to((ax > 0.07 * X) & (ax < 0.4 * X) & (np.abs(y - Y / 2) < 0.36 * Y), SHAPE_ZYX)] = -850
    for _ in range(60):
        c = rng.uniform([0, 0], [X, Y])
        v[np.broadcast_to(((x - c[0]) ** 2 + (y - c[1]) ** 2) < rng.uniform(4, 60), SHAPE_ZYX)] = 60
    v += rng.integers(-30, 31, SHAPE_ZYX, dtype=np.int16)
    v[:, :6, :] = -3024
    return v


def one_series(path, out_dir, scale, K, dev, seed):
    t = {}
    t0 = time.perf_counter()
    vol_zyx, spacing, _ = P.read_metaimage(path)
    t["read"] = time.perf_counter() - t0
    vol, shape = P.prepare_volume(vol_zyx, spacing, dev, timing=t)
    st = {}
    draws = []

    class Recorder(P.GpuEvaluator):
        def __call__(self, ds):
            draws.append(list(ds))
            return super().__call__(ds)
    pairs = list(P.series_pairs(shape, NAME, seed, scale, K, Recorder(vol, shape, timing=t), stats=st))
    t0 = time.perf_counter()
    for k, (g, loc) in pairs:
        P.save_pair(out_dir, NAME, k, g, loc)
    t["write"] = time.perf_counter() - t0
    return t, st, shape, vol_zyx, draws


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=16)
    ap.add_argument("--attempts-per-launch", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    print(f"device: {torch.cuda.get_device_name(0)}; series {SHAPE_ZYX[::-1]} (x, y, z) int16 at {SPACING} mm; scale {a.scale}, "
          f"{a.attempts_per_launch} attempts per launch")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, NAME + ".mhd")
        P.write_metaimage(path, phantom(), SPACING)
        out = os.path.join(tmp, "out")
        os.makedirs(out)
        one_series(path, out, a.scale, a.attempts_per_launch, dev, a.seed)      # warm-up: library load, allocator, page cache
        rows = []
        for r in range(a.repeats):
            t, st, shape, vol_zyx, draws = one_series(path, out, a.scale, a.attempts_per_launch, dev, a.seed)
            rows.append(t)
        keys = ("read", "upload", "resample", "windows", "download", "write")
        print(f"resampled (x, y, z): {shape}; {st['pairs']} pairs from {st['attempts']} attempts (acceptance {st['pairs'] / st['attempts']:.2f} "
              f"on this phantom) in {st['launches']} launches; {sum(len(d) for d in draws)} attempts evaluated on the GPU")
        print("per series, ms (median of %d):" % a.repeats)
        med = {k: float(np.median([r.get(k, 0.0) for r in rows])) * 1e3 for k in keys}
        for k in keys:
            print(f"  {k:9s} {med[k]:9.1f}")
        print(f"  {'total':9s} {sum(med.values()):9.1f}")
        if not a.no_cpu:
            import luna_prep_reference as R
            t0 = time.perf_counter()
            oz = P.resample_size(vol_zyx.shape[::-1], SPACING)[2]
            parts = [R.resample(vol_zyx, SPACING, oz_range=(i, min(i + 25, oz))) for i in range(0, oz, 25)]
            v = R.normalise(np.concatenate(parts).transpose(2, 1, 0))
            t1 = time.perf_counter()
            for ds in draws:
                for d in ds:
                    R.pair_windows(v, d.box1, d.box2, d.size1, d.size2, d.locals)
            t2 = time.perf_counter()
            print(f"float64 restatement on the CPU (numpy, one thread): resample {1e3 * (t1 - t0):.0f} ms, the same "
                  f"{sum(len(d) for d in draws)} attempts {1e3 * (t2 - t1):.0f} ms")


if __name__ == "__main__":
    main()
