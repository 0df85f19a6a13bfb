"""Measurements of DESIGN.md section 22 (the softmax segmentation head), one JSON line per measurement.

    python tools/bench_seg_mc.py [--rounds 5] [--window_ms 100] [--out profiles/seg_mc_bench.txt]

On one random activation of N * S = 8 * 64 * 64 * 32 voxels, bf16 and float32:
  softmax  ops.seg_mc_head_forward, _backward, _eval and _logits alone at K = 2, 4, 8, 16;
  sigmoid  the same four of the sigmoid head (ops.seg_head_*) at K = 7 -- the yardstick: those kernels are the ones the softmax head was modelled on.
The arms alternate inside one process, each warmed; a timed window is as many calls as fill about `window_ms` of device time (sized from a first window of
20) between two device events, as tools/bench_seg.py -- times PER CALL through the Python wrapper (allocations, a workspace lookup, two launches), not
kernel times.  Reported: the median over the rounds, the spread (max - min), the HBM bytes the operator needs (forward / eval: one read of the activation
and the labels; backward: that plus one write of dx; logits: the activation plus the K float32 logits per voxel) and that over the time as a fraction of
the 8 TB/s peak.

A run without a GPU fails: nothing here is an estimate.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_seg import rounds  # noqa: E402
from pcrlv2_amd import ops  # noqa: E402

DEV = torch.device("cuda")
B, CROP = 8, (64, 64, 32)
HBM = 8e12


def arms(kind, K, a, dtype, g):
    w = 0.2 * torch.randn((K, 64, 1, 1, 1), generator=g, device=DEV)
    bias = torch.randn(K, generator=g, device=DEV)
    one = torch.ones((), device=DEV)
    counts = torch.zeros((B, K, 3), dtype=torch.int64, device=DEV)
    z = torch.empty((B,) + CROP + (K,), device=DEV)
    if kind == "softmax":
        lab = torch.randint(0, K, (B,) + CROP, generator=g, device=DEV, dtype=torch.uint8)
        sums = ops.seg_mc_head_forward(a, w, bias, lab, dtype)[1]
        return {"fwd": lambda: ops.seg_mc_head_forward(a, w, bias, lab, dtype), "bwd": lambda: ops.seg_mc_head_backward(a, w, bias, lab, sums, one, dtype),
                "eval": lambda: ops.seg_mc_head_eval(a, w, bias, dtype, labels=lab, counts=counts, want_mask=True),
                "logits": lambda: ops.seg_mc_head_logits(a, w, bias, dtype, out=z)}
    lab = torch.randint(0, 1 << K, (B,) + CROP, generator=g, device=DEV, dtype=torch.uint8)
    sums = ops.seg_head_forward(a, w, bias, lab, dtype)[1]
    return {"fwd": lambda: ops.seg_head_forward(a, w, bias, lab, dtype), "bwd": lambda: ops.seg_head_backward(a, w, bias, lab, sums, one, dtype),
            "eval": lambda: ops.seg_head_eval(a, w, bias, dtype, labels=lab, counts=counts, want_mask=True),
            "logits": lambda: ops.seg_head_logits(a, w, bias, dtype, out=z)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window_ms", type=float, default=100.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_seg_mc.py measures on the GPU; none is visible")
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    emit({"bench": "device", "name": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_ms": args.window_ms, "b": B, "crop": CROP})
    M = B * CROP[0] * CROP[1] * CROP[2]
    for dtype in (torch.bfloat16, torch.float32):
        g = torch.Generator(device=DEV).manual_seed(1)
        a = torch.relu(torch.randn((B,) + CROP + (64,), generator=g, device=DEV)).to(dtype).permute(0, 4, 1, 2, 3)
        es = a.element_size()
        for kind, K in (("sigmoid", 7), ("softmax", 2), ("softmax", 4), ("softmax", 8), ("softmax", 16)):
            need = {"fwd": M * (64 * es + 1), "bwd": M * (2 * 64 * es + 1), "eval": M * (64 * es + 2), "logits": M * (64 * es + 4 * K)}
            for name, (med, spread) in rounds(arms(kind, K, a, dtype, g), args.rounds, args.window_ms).items():
                emit({"bench": "head", "head": kind, "K": K, "arm": name, "dtype": str(dtype).split(".")[1], "ms": round(med, 4), "spread_ms": round(spread, 4),
                      "hbm_bytes_needed": need[name], "fraction_of_8TBps": round(need[name] / (med * 1e-3) / HBM, 4)})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
