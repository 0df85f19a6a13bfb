"""Measurements of DESIGN.md section 21 (mirror test-time augmentation and checkpoint ensembling), one JSON line per measurement.

    python tools/bench_seg_tta.py [--rounds 5] [--out profiles/seg_tta_bench.txt]

Section 16's case: one synthetic case of 128 x 128 x 64 at crop 64 x 64 x 32, overlap 0.5, Gaussian window, K = 3, bf16, b = 8, unlabelled.
case     train_seg.sliding_window (a) un-mirrored -- the code of the revision before the mirrors --, (b) with mirror `all` (8 passes per patch batch),
         (c) with two models and mirror `all` (16 passes).  The arms alternate inside one process, each warmed; a round is ONE call per arm between two
         device events (the events span the host work of the call as well); reported: the median over the rounds, the spread (max - min), the network
         passes per batch E M and the time per pass = ms per case / (E M).  Condition: the time per pass of (b) and of (c) exceeds (a)'s time per
         case by no more than the larger of the two spreads (per pass) -- a pass adds one mirrored cut and one read of the logits inside the head kernel
         to what (a) does, and (a) pays the upload and the blend once per case where (b) and (c) spread them over their passes.
kernels  pcrl_seg_head_logits next to pcrl_seg_head_logits_acc for the mirror codes 0, 4 (z) and 7 (x, y and z), adding (first = 0, the extra read of
         z) and, for code 7, overwriting (first = 1), and pcrl_seg_cut_patches next to pcrl_seg_cut_patches_mirror for the same codes: one batch of 8
         patches through the raw entry points into preallocated buffers, 200 launches queued back to back between two events.  Bytes needed (every
         input once, every output once) over the time, against the 6.3 TB/s a copy achieves.  The operands of a window stay the same and fit the
         Infinity Cache, so these are Infinity-Cache-resident figures, as section 16's.

A run without a GPU fails: nothing here is an estimate.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pcrlv2_amd import data_seg as D  # noqa: E402
from pcrlv2_amd._lib import lib, stream_handle  # noqa: E402
from pcrlv2_amd.models import Segmenter3d  # noqa: E402
from pcrlv2_amd.train_seg import sliding_window  # noqa: E402

DEV = torch.device("cuda")
SHAPE, CROP, K, B = (128, 128, 64), (64, 64, 32), 3, 8
OVERLAP, WINDOW = 0.5, "gaussian"
COPY_BW = 6.3e12


def timed(fn, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def rounds(arms, n, reps):
    for fn in arms.values():
        fn()
    ms = {k: [] for k in arms}
    for _ in range(n):
        for k, fn in arms.items():
            ms[k].append(timed(fn, reps))
    return {k: (float(np.median(v)), float(max(v) - min(v))) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_seg_tta.py measures on the GPU; none is visible")
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    emit({"bench": "device", "name": torch.cuda.get_device_name(0), "rounds": args.rounds, "shape": SHAPE, "crop": CROP, "K": K, "b": B, "dtype": "bfloat16",
          "overlap": OVERLAP, "window": WINDOW})
    models = []
    for seed in (0, 1):
        torch.manual_seed(seed)
        models.append(Segmenter3d(K).cuda().eval().set_compute_dtype(torch.bfloat16))
    case = D.synthetic_case(0, 0, SHAPE, K)
    unlabelled = D.Case(case.name, case.img)
    starts = D.window_starts(D.windows(SHAPE, CROP, OVERLAP))
    P, every = len(starts), D.parse_mirror("all")

    def run(**kw):
        return sliding_window(models[0], unlabelled, CROP, B, OVERLAP, WINDOW, **kw)[0].cpu()

    arms = {"unmirrored": (1, lambda: run()), "mirror_all": (8, lambda: run(mirror=every)),
            "two_models_mirror_all": (16, lambda: run(mirror=every, models=models))}
    r = rounds({k: fn for k, (_, fn) in arms.items()}, args.rounds, 1)
    per = {}
    for name, (n_pass, _) in arms.items():
        med, spread = r[name]
        per[name] = (med / n_pass, spread / n_pass)
        emit({"bench": "case", "arm": name, "patches": P, "passes_per_batch": n_pass, "ms_per_case": round(med, 3), "spread_ms": round(spread, 3),
              "ms_per_pass": round(med / n_pass, 3), "spread_ms_per_pass": round(spread / n_pass, 3)})
    for name in ("mirror_all", "two_models_mirror_all"):
        slack = max(per["unmirrored"][1], per[name][1])
        extra = per[name][0] - per["unmirrored"][0]
        emit({"bench": "case", "condition": name, "ms_per_pass_minus_unmirrored_ms_per_case": round(extra, 3), "larger_spread_ms_per_pass": round(slack, 3),
              "holds": extra <= slack})

    # the raw entry points at one batch of 8 patches
    img = torch.from_numpy(case.img).to(DEV)
    st = torch.tensor(starts[:B], dtype=torch.int32, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(1)
    a_rows = torch.relu(torch.randn((B,) + CROP + (64,), generator=g, device=DEV)).to(torch.bfloat16)
    fc = models[0].out_tr.final_conv
    wc, bc = fc.weight.detach().reshape(K, 64).contiguous(), fc.bias.detach().contiguous()
    zb = torch.zeros((B,) + CROP + (K,), device=DEV)
    x = torch.empty((B, 1) + CROP, device=DEV)
    L, s_ = lib(), stream_handle()
    S = CROP[0] * CROP[1] * CROP[2]
    karms = {"seg_head_logits_b8": lambda: L.call("pcrl_seg_head_logits", a_rows, wc, bc, zb, B, S, K, 1, s_),
             "seg_cut_patches_b8": lambda: L.call("pcrl_seg_cut_patches", img, 0, st, x, B, 1, *SHAPE, *CROP, s_)}
    need = {"seg_head_logits_b8": B * S * (64 * 2 + 4 * K), "seg_cut_patches_b8": B * S * 8}
    for code in (0, 4, 7):
        # the adding arms keep adding the same logits into zb: a few thousand additions of values of order 1 over the whole run, far from overflow
        karms[f"seg_head_logits_acc_b8_flip{code}_add"] = lambda c=code: L.call("pcrl_seg_head_logits_acc", a_rows, wc, bc, zb, B, S, K, 1, *CROP, c, 0, 1.0, s_)
        need[f"seg_head_logits_acc_b8_flip{code}_add"] = B * S * (64 * 2 + 8 * K)
        karms[f"seg_cut_patches_mirror_b8_flip{code}"] = lambda c=code: L.call("pcrl_seg_cut_patches_mirror", img, 0, st, x, B, 1, *SHAPE, *CROP, c, s_)
        need[f"seg_cut_patches_mirror_b8_flip{code}"] = B * S * 8
    karms["seg_head_logits_acc_b8_flip7_first"] = lambda: L.call("pcrl_seg_head_logits_acc", a_rows, wc, bc, zb, B, S, K, 1, *CROP, 7, 1, 1.0, s_)
    need["seg_head_logits_acc_b8_flip7_first"] = B * S * (64 * 2 + 4 * K)
    r = rounds(karms, args.rounds, 200)
    for name, (med, spread) in r.items():
        emit({"bench": "kernels", "arm": name, "ms": round(med, 4), "spread_ms": round(spread, 4), "bytes_needed": need[name],
              "TB_per_s": round(need[name] / (med * 1e-3) / 1e12, 3), "fraction_of_6.3TBps_copy": round(need[name] / (med * 1e-3) / COPY_BW, 4)})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
