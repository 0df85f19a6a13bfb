"""Measurements of DESIGN.md section 19 (training-time augmentation of 3D segmentation crops), one JSON line per measurement.

    python tools/bench_seg_aug.py [--crop 64,64,32] [--b 8] [--in_channels 4] [--amp] [--rounds 5] [--window_ms 500] [--out profiles/seg_aug_bench.txt]

What the feature costs is a larger upload plus one gather (and one noise / gamma pass) per step, and more host cutting.  Three things are measured, the
augmented arms at `--augment`'s defaults with both probabilities 1 (every crop rotated and zoomed, every channel's intensity changed: the dearest draw):

device  ops.seg_augment alone, and ops.seg_augment + ops.seg_noise_gamma, on resident inputs: ms per call between two device events (through the
        Python wrappers, as tools/bench_seg.py times its head), and two byte counts: crop_bytes (the crops written plus as many source bytes read
        -- what a zoom of 1 touches -- and one read and one write of the crops by the noise / gamma pass), with its fraction of the 8 TB/s peak,
        and box_bytes (the whole source boxes read once instead).  The kernel reads between the two; neighbours are reread from cache.
step    one train_seg.train_step of models.Segmenter3d on a fixed pinned batch: the plain two-entry batch (the parent revision's path, unchanged) and
        the augmented three-entry batch, alternating inside one process; ms per step, their ratio, and the bytes each uploads.
host    the host time of one batch of data_seg.CropLoader with and without `aug` (numpy cutting, no GPU): the loader runs in the training loop's
        thread, so this is added to every step.

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
from pcrlv2_amd import data_seg as D  # noqa: E402
from pcrlv2_amd import ops  # noqa: E402
from bench_seg import rounds  # noqa: E402

DEV = torch.device("cuda")
K = 3
HBM = 8e12


def pinned(batch):
    pin = lambda t: t.pin_memory()      # noqa: E731
    return tuple({k: pin(v) if v.dim() else v for k, v in e.items()} if isinstance(e, dict) else pin(e) for e in batch)


def nbytes(batch):
    return sum(sum(v.numel() * v.element_size() for v in e.values()) if isinstance(e, dict) else e.numel() * e.element_size() for e in batch)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crop", default="64,64,32")
    ap.add_argument("--b", type=int, default=8)
    ap.add_argument("--in_channels", type=int, default=4)
    ap.add_argument("--amp", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window_ms", type=float, default=500.0)
    ap.add_argument("--only", default="device,step,host")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_seg_aug.py measures on the GPU; none is visible")
    crop, b, C = D.parse_crop(args.crop), args.b, args.in_channels
    dtype = torch.bfloat16 if args.amp else torch.float32
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    cfg = D.AugConfig.defaults(p_spatial=1.0, p_intensity=1.0)
    extent = D.source_extent(crop, cfg)
    emit({"bench": "device", "name": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_ms": args.window_ms, "crop": crop, "b": b,
          "in_channels": C, "dtype": str(dtype).split(".")[1], "source_extent": extent,
          "source_over_crop_voxels": round(float(np.prod(extent)) / float(np.prod(crop)), 3)})
    cases = [D.synthetic_case(0, i, D.synthetic_shape(crop), K, C) for i in range(4)]
    plain = pinned(next(iter(D.CropLoader(cases, crop, b, 1, 0, 0))))
    aug = pinned(next(iter(D.CropLoader(cases, crop, b, 1, 0, 0, aug=cfg))))

    if "device" in args.only:
        up = lambda t: t.to(DEV)      # noqa: E731
        src, src_lab, p = up(aug[0]), up(aug[1]), {k: up(v) for k, v in aug[2].items() if v.dim()}
        seed = int(aug[2]["seed"])
        out = ops.seg_augment(src, src_lab, p["inv"], p["gain"], p["bias"], crop=crop)

        def resample():
            return ops.seg_augment(src, src_lab, p["inv"], p["gain"], p["bias"], out=out)

        def both():
            return ops.seg_noise_gamma(resample()[0], p["noise_std"], p["gamma"], seed)

        r = rounds({"seg_augment": resample, "seg_augment_noise_gamma": both}, args.rounds, args.window_ms)
        V, SV = int(np.prod(crop)), int(np.prod(extent))
        # crop_bytes: the crops written (image and label) plus as many source bytes read, what a zoom of 1 touches; box_bytes: every voxel of the
        # source boxes read once instead -- the kernel reads between the two, whatever part of a box its crop maps into
        es = src.element_size()
        crop_bytes = {"seg_augment": b * (C * V * (es + 4) + 2 * V)}
        crop_bytes["seg_augment_noise_gamma"] = crop_bytes["seg_augment"] + b * C * V * 8
        box_extra = b * (C * (SV - V) * es + (SV - V))
        for name, (med, spread) in r.items():
            emit({"bench": "device", "arm": name, "ms": round(med, 4), "spread_ms": round(spread, 4), "crop_bytes": crop_bytes[name],
                  "box_bytes": crop_bytes[name] + box_extra, "crop_bytes_fraction_of_8TBps": round(crop_bytes[name] / (med * 1e-3) / HBM, 4)})

    if "step" in args.only:
        from pcrlv2_amd.models import Segmenter3d
        from pcrlv2_amd.optim import FusedSGD
        from pcrlv2_amd.train_seg import train_step
        torch.manual_seed(0)
        model = Segmenter3d(K, in_channels=C).cuda().train().set_compute_dtype(dtype)
        opt = FusedSGD(model.trainable_parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
        r = rounds({"step_plain": lambda: train_step(model, opt, plain), "step_augmented": lambda: train_step(model, opt, aug)}, args.rounds, args.window_ms)
        for name, batch in (("step_plain", plain), ("step_augmented", aug)):
            med, spread = r[name]
            emit({"bench": "step", "arm": name, "ms": round(med, 3), "spread_ms": round(spread, 3), "crops_per_s": round(b / (med * 1e-3), 1),
                  "upload_bytes": nbytes(batch)})
        emit({"bench": "step", "augmented_over_plain": round(r["step_augmented"][0] / r["step_plain"][0], 4)})

    if "host" in args.only:
        for name, cfg_ in (("loader_plain", None), ("loader_augmented", cfg)):
            ms = []
            for rep in range(args.rounds):
                it = iter(D.CropLoader(cases, crop, b, 4, rep, 0, aug=cfg_))
                next(it)
                t0 = time.perf_counter()
                for _ in range(3):
                    next(it)
                ms.append((time.perf_counter() - t0) / 3 * 1e3)
            emit({"bench": "host", "arm": name, "ms_per_batch": round(float(np.median(ms)), 3), "spread_ms": round(max(ms) - min(ms), 3)})

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
