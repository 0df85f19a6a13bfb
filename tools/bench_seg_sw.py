"""Measurements of DESIGN.md section 16 (overlap-blended sliding-window inference), one JSON line per measurement.

    python tools/bench_seg_sw.py [--rounds 5] [--out profiles/seg_sw_bench.txt]

One synthetic case of 128 x 128 x 64 at crop 64 x 64 x 32, K = 3, bf16, b = 8.
case     (a) train_seg.predict_case, the stride-tiled path: patches cut on the host, one upload per batch, the mask stitched on the host;
         (b) train_seg.sliding_window at overlap 0.5 with the Gaussian window: one upload, patches cut on the device, one blend.
         The two arms alternate inside one process, each warmed; a round is ONE call per arm between two device events (the events span the host work
         of the call as well: it is part of what a case costs); reported: the median over the rounds, the spread (max - min), the patches per case and
         the time per patch.  Condition 1: (b)'s time per patch exceeds (a)'s by no more than the larger of the two spreads (per patch).
kernels  the device time of the three new kernels on their own at the sizes of arm (b): pcrl_seg_cut_patches and pcrl_seg_head_logits for one batch
         of 8 patches, pcrl_seg_blend for the case (mask only, and with labels, sums and counts), next to one patch-batch forward
         (Segmenter3d.infer_logits).  The kernels are called through the raw entry points into preallocated outputs (no allocation, argument check or
         workspace lookup in the window), 200 launches queued back to back between two events: device time per launch.  Condition 2: the blend of a
         case takes less than one patch-batch forward.  Bytes needed (every input once, every output once) over the time, against the 6.3 TB/s a
         copy achieves; the inputs of a window stay the same, so what fits the Infinity Cache is read from it.

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
from pcrlv2_amd import ops  # noqa: E402
from pcrlv2_amd._lib import lib, stream_handle  # noqa: E402
from pcrlv2_amd.models import Segmenter3d  # noqa: E402
from pcrlv2_amd.train_seg import predict_case, sliding_window  # noqa: E402

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
        raise SystemExit("tools/bench_seg_sw.py measures on the GPU; none is visible")
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    emit({"bench": "device", "name": torch.cuda.get_device_name(0), "rounds": args.rounds, "shape": SHAPE, "crop": CROP, "K": K, "b": B, "dtype": "bfloat16"})
    torch.manual_seed(0)
    model = Segmenter3d(K).cuda().eval().set_compute_dtype(torch.bfloat16)
    case = D.synthetic_case(0, 0, SHAPE, K)
    unlabelled = D.Case(case.name, case.img)
    n_tiled = len(D.tiles(SHAPE, CROP))
    axes = D.windows(SHAPE, CROP, OVERLAP)
    starts = D.window_starts(axes)
    P = len(starts)

    r = rounds({"tiled_predict_case": lambda: predict_case(model, unlabelled, CROP, B),
                "sliding_window": lambda: sliding_window(model, unlabelled, CROP, B, OVERLAP, WINDOW)[0].cpu()}, args.rounds, 1)
    per = {}
    for name, n in (("tiled_predict_case", n_tiled), ("sliding_window", P)):
        med, spread = r[name]
        per[name] = (med / n, spread / n)
        emit({"bench": "case", "arm": name, "overlap": 0.0 if name.startswith("tiled") else OVERLAP, "patches": n, "ms_per_case": round(med, 3),
              "spread_ms": round(spread, 3), "ms_per_patch": round(med / n, 4), "spread_ms_per_patch": round(spread / n, 4)})
    slack = max(per["tiled_predict_case"][1], per["sliding_window"][1])
    emit({"bench": "case", "condition": 1, "sliding_minus_tiled_ms_per_patch": round(per["sliding_window"][0] - per["tiled_predict_case"][0], 4),
          "larger_spread_ms_per_patch": round(slack, 4), "holds": per["sliding_window"][0] - per["tiled_predict_case"][0] <= slack})

    # the kernels on their own, at arm (b)'s sizes
    img = torch.from_numpy(case.img).to(DEV)
    lab = torch.from_numpy(case.seg).to(DEV)
    st = torch.tensor(starts, dtype=torch.int32, device=DEV)
    x = ops.seg_cut_patches(img, st[:B], CROP)
    g = torch.Generator(device=DEV).manual_seed(1)
    a = torch.relu(torch.randn((B,) + CROP + (64,), generator=g, device=DEV)).to(torch.bfloat16).permute(0, 4, 1, 2, 3)
    fc = model.out_tr.final_conv
    z = torch.randn((P,) + CROP + (K,), generator=g, device=DEV)
    zb = torch.empty((B,) + CROP + (K,), device=DEV)
    sd = [torch.tensor(s, dtype=torch.int32, device=DEV) for s in axes]
    wd = [torch.from_numpy(w).to(DEV) for w in D.blend_weights(CROP, WINDOW)]
    counts = torch.zeros((1, K, 3), dtype=torch.int64, device=DEV)
    # raw entry points into preallocated outputs: no allocation, no argument checks, no workspace lookup inside the timed window -- 200 launches
    # queued back to back between two events, so the window is device time
    L, s_ = lib(), stream_handle()
    wc, bc = fc.weight.detach().reshape(K, 64).contiguous(), fc.bias.detach().contiguous()
    a_rows = a.permute(0, 2, 3, 4, 1)
    assert a_rows.is_contiguous()
    S = CROP[0] * CROP[1] * CROP[2]
    mask = torch.empty(SHAPE, dtype=torch.uint8, device=DEV)
    sums, loss = torch.empty(4 * K + 1, dtype=torch.float64, device=DEV), torch.empty(1, device=DEV)
    nb = L.call("pcrl_seg_blend_ws_bytes", *SHAPE)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    n_ax = [len(ax) for ax in axes]

    def blend(labels, cnt, sm, ls, w, wbytes):
        return L.call("pcrl_seg_blend", z, P, *sd, *n_ax, *wd, *CROP, *SHAPE, K, labels, mask, None, None, cnt, sm, ls, 1.0, 1.0, w, wbytes, s_)

    arms = {"seg_cut_patches_b8": lambda: L.call("pcrl_seg_cut_patches", img, 0, st, x, B, 1, *SHAPE, *CROP, s_),
            "seg_head_logits_b8": lambda: L.call("pcrl_seg_head_logits", a_rows, wc, bc, zb, B, S, K, 1, s_),
            "seg_blend_mask_only": lambda: blend(None, None, None, None, None, 0),
            "seg_blend_labels_sums_counts": lambda: blend(lab, counts[0], sums, loss, ws, nb),
            "patch_batch_forward_b8": lambda: model.infer_logits(x, out=zb)}
    r = rounds(arms, args.rounds, 200)
    V, vox = SHAPE[0] * SHAPE[1] * SHAPE[2], CROP[0] * CROP[1] * CROP[2]
    need = {"seg_cut_patches_b8": B * vox * 8, "seg_head_logits_b8": B * vox * (64 * 2 + 4 * K), "seg_blend_mask_only": P * vox * K * 4 + V,
            "seg_blend_labels_sums_counts": P * vox * K * 4 + 2 * V}
    for name, (med, spread) in r.items():
        rec = {"bench": "kernels", "arm": name, "ms": round(med, 4), "spread_ms": round(spread, 4)}
        if name in need:
            rec["bytes_needed"] = need[name]
            rec["TB_per_s"] = round(need[name] / (med * 1e-3) / 1e12, 3)
            rec["fraction_of_6.3TBps_copy"] = round(need[name] / (med * 1e-3) / COPY_BW, 4)
        emit(rec)
    emit({"bench": "kernels", "condition": 2, "blend_ms_per_case": round(r["seg_blend_labels_sums_counts"][0], 4),
          "patch_batch_forward_ms": round(r["patch_batch_forward_b8"][0], 4), "holds": r["seg_blend_labels_sums_counts"][0] < r["patch_batch_forward_b8"][0]})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
