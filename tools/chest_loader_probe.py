#!/usr/bin/env python3
"""Cost of the 2D (chest) pre-task loader (pcrlv2_amd/data_chest.py -> csrc/augment2d.hip) at b = 64 on 1024 x 1024 gray sources (NIH
ChestX-ray14's shape): GPU time of the pcrl_aug2d_* kernels per batch (events around the batch on the loader's stream; run under
`rocprofv3 --kernel-trace --stats` for the per-kernel split), PNG decode rate of the workers' decode() over a process pool, and the
host enqueue time per batch of the loader itself (PCRL_LOADER_TIMING=1 prints it).

    python tools/chest_loader_probe.py [--decode-procs 16] [--batches 10]
"""
import argparse
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pcrlv2_amd import data_chest as DC  # noqa: E402


def write_pngs(d, n, side):
    from PIL import Image
    rng = np.random.default_rng(0)
    y, x = np.mgrid[0:side, 0:side]
    base = ((x // 4 + y // 3) % 256).astype(np.int64)
    for k in range(n):
        a = (base + rng.integers(0, 24, base.shape) + 5 * k).clip(0, 255).astype(np.uint8)
        Image.fromarray(a, "L").save(os.path.join(d, f"{k:04d}.png"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=64)
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--decode-procs", type=int, default=16)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        write_pngs(d, a.b, a.side)
        files = sorted(os.path.join(d, f) for f in os.listdir(d))
        import multiprocessing as mp
        with mp.get_context("spawn").Pool(a.decode_procs) as pool:
            pool.map(DC.decode, files[:a.decode_procs])
            t = time.perf_counter()
            for _ in range(3):
                imgs = pool.map(DC.decode, files)
            dt = time.perf_counter() - t
        print(f"decode: {3 * len(files) / dt:.0f} images/s ({a.side}^2 gray PNG, {a.decode_procs} processes)", flush=True)
        cap = a.side * a.side * 3
        pix = torch.zeros((a.b, cap), dtype=torch.uint8).pin_memory()
        for n, im in enumerate(imgs):
            pix[n, :im.size] = torch.from_numpy(im.reshape(-1))
        dims = torch.tensor([im.shape for im in imgs], dtype=torch.int32)
        aug = DC.GpuChestAugment("cuda", seed=0)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            aug(pix, dims)
        s.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        host = 0.0
        with torch.cuda.stream(s):
            e0.record(s)
            for _ in range(a.batches):
                t = time.perf_counter()
                aug(pix, dims)
                host += time.perf_counter() - t
            e1.record(s)
        s.synchronize()
        print(f"augment: {e0.elapsed_time(e1) / a.batches:.3f} ms GPU per b = {a.b} batch (copies + pcrl_aug2d_* kernels, {8 * a.b} views), "
              f"host enqueue {1e3 * host / a.batches:.2f} ms per batch", flush=True)
        os.environ["PCRL_LOADER_TIMING"] = "1"
        from pcrlv2_amd import data as D
        D.LOADER_TIMING = True
        loader = DC.AugmentedLoader(files, a.b, 4, "cuda", True, 0, kind=DC.ChestKind(files))
        for _ in range(2):
            for batch in loader:
                pass
        torch.cuda.synchronize()
        loader.close()


if __name__ == "__main__":
    main()
