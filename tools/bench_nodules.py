"""Measurements of DESIGN.md section 14 (LUNA16 nodule classification), one JSON line per measurement.

    python tools/bench_nodules.py [--rounds 7] [--only cubes,step,predict]

cubes    pcrl_prep_cubes, M = 1 024 cubes of 64 x 64 x 32 out of a 320 x 320 x 300 volume (and 319 x 320 x 300: X odd), int16 and float32 outputs, against the torch composition on
         the device (F.pad with -1000, an indexed gather of the M windows, permute(...).contiguous(), clamp, and for float32 the double-precision
         normalisation).  Bytes moved = one read + one write of the cubes (the HBM floor), as a fraction of 8 TB/s.
step     one train_finetune.train_step of NoduleClassifier at b = 32, 64 x 64 x 32, bf16.
predict  luna_nodules.score_series on one synthetic series of that size with 850 candidates, b = 256, cubes cut by the kernel and by the composition.

The arms alternate inside one process, each warmed, timed with device events; reported: the median of the rounds and the spread (max - min).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pcrlv2_amd import luna_nodules as N  # noqa: E402

DEV = torch.device("cuda")
CUBE = (64, 64, 32)
HBM = 8e12


def torch_cubes(vol, start, cube=CUBE, float32=False, out=None):
    """The torch composition of pcrl_prep_cubes (same signature as luna_nodules.gpu_cubes)."""
    CX, CY, CZ = cube
    Z, Y, X = vol.shape
    vp = F.pad(vol, (CX, CX, CY, CY, CZ, CZ), value=-1000)
    if not torch.is_tensor(start):
        start = torch.from_numpy(np.ascontiguousarray(start, dtype=np.int32))
    s = start.to(vol.device).long()
    x0, y0, z0 = s[:, 0].clamp(-CX, X) + CX, s[:, 1].clamp(-CY, Y) + CY, s[:, 2].clamp(-CZ, Z) + CZ
    ar = lambda n: torch.arange(n, device=vol.device)       # noqa: E731
    win = vp[(z0[:, None] + ar(CZ))[:, :, None, None], (y0[:, None] + ar(CY))[:, None, :, None], (x0[:, None] + ar(CX))[:, None, None, :]]
    c = win.permute(0, 3, 2, 1).contiguous().clamp(-1000, 1000)
    if float32:
        c = ((c.double() + 1000.0) / 2000.0).float()
    if out is not None:
        out[:c.shape[0]].copy_(c)
        return out[:c.shape[0]]
    return c


def timed(fn, warm=2):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def rounds(arms, n):
    """{name: fn} -> {name: (median ms, spread ms)}; the arms alternate within every round."""
    ms = {k: [] for k in arms}
    for _ in range(n):
        for k, fn in arms.items():
            ms[k].append(timed(fn))
    return {k: (float(np.median(v)), float(max(v) - min(v))) for k, v in ms.items()}


def volume_and_starts(m, seed=0, X=320):
    g = torch.Generator(device=DEV).manual_seed(seed)
    vol = torch.randint(-1200, 1200, (300, 320, X), generator=g, device=DEV, dtype=torch.int16)
    rng = np.random.default_rng(seed)
    start = np.stack([rng.integers(-20, X - 44, m), rng.integers(-20, 320 - 44, m), rng.integers(-10, 300 - 22, m)], 1).astype(np.int32)
    return vol, start


def bench_cubes(n):
    M = 1024
    for X, f32 in ((320, False), (320, True), (319, False), (319, True)):       # X odd: every row of the volume has another alignment
        vol, start = volume_and_starts(M, X=X)
        sd = torch.from_numpy(start).to(DEV)
        assert torch.equal(N.gpu_cubes(vol, sd, CUBE, f32), torch_cubes(vol, sd, CUBE, f32))
        out = torch.empty((M,) + CUBE, dtype=torch.float32 if f32 else torch.int16, device=DEV)
        r = rounds({"kernel": lambda: N.gpu_cubes(vol, sd, CUBE, f32, out), "torch": lambda: torch_cubes(vol, sd, CUBE, f32)}, n)
        nbytes = M * CUBE[0] * CUBE[1] * CUBE[2] * (2 + (4 if f32 else 2))
        print(json.dumps({"measurement": "prep_cubes", "out": "float32" if f32 else "int16", "X": X, "M": M, "rounds": n,
                          "kernel_ms": r["kernel"][0], "kernel_spread_ms": r["kernel"][1], "torch_ms": r["torch"][0], "torch_spread_ms": r["torch"][1],
                          "kernel_cubes_per_s": M / r["kernel"][0] * 1e3, "torch_cubes_per_s": M / r["torch"][0] * 1e3,
                          "kernel_fraction_of_8TBps": nbytes / (r["kernel"][0] * 1e-3) / HBM,
                          "faster_by_more_than_the_spreads": r["torch"][0] - r["kernel"][0] > r["torch"][1] + r["kernel"][1]}), flush=True)


def bench_step(n):
    from pcrlv2_amd.data import SyntheticNoduleLoader
    from pcrlv2_amd.models import NoduleClassifier
    from pcrlv2_amd.optim import FusedSGD
    from pcrlv2_amd.train_finetune import train_step
    torch.manual_seed(0)
    model = NoduleClassifier().to(DEV).set_compute_dtype(torch.bfloat16)
    model.train()
    opt = FusedSGD(model.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
    batch = next(iter(SyntheticNoduleLoader(32, 1, CUBE, device=DEV)))
    for _ in range(5):
        train_step(model, opt, batch)
    r = rounds({"step": lambda: [train_step(model, opt, batch) for _ in range(5)]}, n)
    print(json.dumps({"measurement": "train_step", "b": 32, "dtype": "bf16", "rounds": n, "ms_per_step": r["step"][0] / 5, "spread_ms": r["step"][1] / 5}), flush=True)


def bench_predict(n):
    from pcrlv2_amd.models import NoduleClassifier
    torch.manual_seed(0)
    model = NoduleClassifier().to(DEV).set_compute_dtype(torch.bfloat16)
    vol, start = volume_and_starts(850, seed=1)
    a, b = N.score_series(model, vol, start, CUBE, 256), N.score_series(model, vol, start, CUBE, 256, cut=torch_cubes)
    assert torch.equal(a, b)
    r = rounds({"kernel": lambda: N.score_series(model, vol, start, CUBE, 256), "torch": lambda: N.score_series(model, vol, start, CUBE, 256, cut=torch_cubes)}, n)
    print(json.dumps({"measurement": "predict", "candidates": 850, "b": 256, "dtype": "bf16", "rounds": n,
                      "kernel_ms": r["kernel"][0], "kernel_spread_ms": r["kernel"][1], "torch_ms": r["torch"][0], "torch_spread_ms": r["torch"][1],
                      "kernel_cubes_per_s": 850 / r["kernel"][0] * 1e3, "torch_cubes_per_s": 850 / r["torch"][0] * 1e3}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only", default="cubes,step,predict")
    args = ap.parse_args()
    for name in args.only.split(","):
        {"cubes": bench_cubes, "step": bench_step, "predict": bench_predict}[name](args.rounds)


if __name__ == "__main__":
    main()
