"""Measurements of DESIGN.md section 15 (3D segmentation fine-tuning), one JSON line per measurement.

    python tools/bench_seg.py [--rounds 5] [--window_ms 200] [--only head,step] [--out profiles/seg_head_bench.txt]

head   at K = 3, crop 64 x 64 x 32, bf16 and float32, b = 8 and b = 32, on the same random activation:
         (a) the head of the n_class = 3 constructor variant alone -- ops.conv1x1_to1_forward + ops.conv1x1_to1_backward, what functions.OutFn runs,
             with NO loss on top (the gradient of the output is a given tensor);
         (b) ops.seg_head_forward + ops.seg_head_backward, the loss included.
       The two arms alternate inside one process, each warmed; a timed window is as many calls as fill about `window_ms` of device time (sized from a first window of 20) between two device
       events -- these are times PER CALL through the Python wrapper (two allocations, a workspace lookup, two launches), not kernel times: the kernels'
       own times come from a separate `rocprofv3 --kernel-trace --stats` run of this script; reported: the median over
       the rounds of the time per call, the spread (max - min), and for (b) the HBM bytes the operator needs (forward: one read of the activation and
       the labels; backward: that again plus one write of dx) over the time, as a fraction of the 8 TB/s peak.  (b) must be faster than (a).
step   one train_seg.train_step of models.Segmenter3d at the same sizes (bf16; float32 at b = 8): ms per step and crops/s.

A run without a GPU fails: nothing here is an estimate.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pcrlv2_amd import ops  # noqa: E402

DEV = torch.device("cuda")
CROP = (64, 64, 32)
K = 3
HBM = 8e12


def window(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def rounds(arms, n, window_ms):
    reps = {k: max(20, int(window_ms / max(window(fn, 20), 1e-3))) for k, fn in arms.items()}      # calls that fill the window, from a first short one
    ms = {k: [] for k in arms}
    for _ in range(n):
        for k, fn in arms.items():
            ms[k].append(window(fn, reps[k], warm=1))
    return {k: (float(np.median(v)), float(max(v) - min(v))) for k, v in ms.items()}


def bench_head(n, window_ms, emit):
    for dtype in (torch.bfloat16, torch.float32):
        for b in (8, 32):
            g = torch.Generator(device=DEV).manual_seed(b)
            M = b * CROP[0] * CROP[1] * CROP[2]
            a = torch.relu(torch.randn((b,) + CROP + (64,), generator=g, device=DEV)).to(dtype).permute(0, 4, 1, 2, 3)
            w = 0.2 * torch.randn((K, 64, 1, 1, 1), generator=g, device=DEV)
            bias = torch.randn(K, generator=g, device=DEV)
            lab = torch.randint(0, 8, (b,) + CROP, generator=g, device=DEV, dtype=torch.uint8)
            dout = torch.randn((b, K) + CROP, generator=g, device=DEV)
            one = torch.ones((), device=DEV)

            def per_class():
                out = ops.conv1x1_to1_forward(a, w, bias, dtype)
                return ops.conv1x1_to1_backward(a, out, dout, w, dtype)

            def fused_fwd():
                return ops.seg_head_forward(a, w, bias, lab, dtype)

            sums = fused_fwd()[1]

            def fused_bwd():
                return ops.seg_head_backward(a, w, bias, lab, sums, one, dtype)

            def fused():
                fused_fwd()
                return fused_bwd()

            r = rounds({"per_class_head_no_loss": per_class, "seg_head_with_loss": fused, "seg_head_fwd": fused_fwd, "seg_head_bwd": fused_bwd}, n, window_ms)
            es = a.element_size()
            need = {"seg_head_fwd": M * (64 * es + 1), "seg_head_bwd": M * (2 * 64 * es + 1)}
            need["seg_head_with_loss"] = need["seg_head_fwd"] + need["seg_head_bwd"]
            for name, (med, spread) in r.items():
                rec = {"bench": "head", "arm": name, "dtype": str(dtype).split(".")[1], "b": b, "K": K, "crop": CROP, "ms": round(med, 4), "spread_ms": round(spread, 4)}
                if name in need:
                    rec["hbm_bytes_needed"] = need[name]
                    rec["fraction_of_8TBps"] = round(need[name] / (med * 1e-3) / HBM, 4)
                emit(rec)
            emit({"bench": "head", "dtype": str(dtype).split(".")[1], "b": b, "fused_faster_than_per_class": r["seg_head_with_loss"][0] < r["per_class_head_no_loss"][0],
                  "ratio_per_class_over_fused": round(r["per_class_head_no_loss"][0] / r["seg_head_with_loss"][0], 3)})


def bench_step(n, window_ms, emit):
    from pcrlv2_amd import data_seg as D
    from pcrlv2_amd.models import Segmenter3d
    from pcrlv2_amd.optim import FusedSGD
    from pcrlv2_amd.train_seg import train_step
    for dtype, b in ((torch.bfloat16, 8), (torch.bfloat16, 32), (torch.float32, 8)):
        torch.manual_seed(0)
        model = Segmenter3d(K).cuda().train().set_compute_dtype(dtype)
        opt = FusedSGD(model.trainable_parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
        cases = [D.synthetic_case(0, i, CROP, K) for i in range(4)]
        x = torch.from_numpy(np.stack([cases[i % 4].img for i in range(b)])).pin_memory()
        lab = torch.from_numpy(np.stack([cases[i % 4].seg for i in range(b)])).pin_memory()
        med, spread = rounds({"step": lambda: train_step(model, opt, (x, lab))}, n, window_ms)["step"]
        emit({"bench": "step", "dtype": str(dtype).split(".")[1], "b": b, "crop": CROP, "K": K, "ms": round(med, 3), "spread_ms": round(spread, 3),
              "crops_per_s": round(b / (med * 1e-3), 1)})
        del model, opt
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window_ms", type=float, default=200.0)
    ap.add_argument("--only", default="head,step")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_seg.py measures on the GPU; none is visible")
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    emit({"bench": "device", "name": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_ms": args.window_ms})
    if "head" in args.only:
        bench_head(args.rounds, args.window_ms, emit)
    if "step" in args.only:
        bench_step(args.rounds, args.window_ms, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
