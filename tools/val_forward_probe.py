"""A/B of the eval-mode forward: model.eval()(x) (conv + apply as two passes per LUConv) against PCRLv23d.infer(x) (normalisation and
activation in the convolution's epilogue), same process, same weights, same input, warmed, ALTERNATING, device-event times.

    python tools/val_forward_probe.py [--reps 24] [--out profiles/val_forward_ab.txt] [--shapes 32x64x64x32,8x128x128x64] [--dtype bf16]
    python tools/val_forward_probe.py --trace-only --shapes 32x64x64x32      # one warm-up + 3 repetitions per arm, for `rocprofv3 --kernel-trace --stats -- python ...`
    python tools/val_forward_probe.py --validate-wall 1000                     # wall time of one validate pass over N synthetic samples next to a training epoch of the same size

Beside the times it prints, from the shapes alone, the bytes the fused layers no longer move: one write and one read of every fused layer's
pre-normalisation tensor (N * D * H * W * Co * element size, twice).  The verdict per shape: the fused forward counts as faster when the gap of the
medians exceeds the two arms' combined spread (half the 10..90 percentile range of each arm, added).
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from pcrlv2_amd import ops  # noqa: E402
from pcrlv2_amd._lib import ACT_RELU  # noqa: E402
from pcrlv2_amd.models import PCRLv23d  # noqa: E402


def luconv_shapes(N, D, H, W):
    """(Ci, Co, N, D, H, W) of the BatchNorm + ReLU LUConvs of the default model."""
    out = []
    lv = lambda s: (D >> s, H >> s, W >> s)
    for s, (a, b) in enumerate(((32, 64), (64, 128), (128, 256), (256, 512))):
        out += [(1 if s == 0 else a, a, N, *lv(s)), (a, b, N, *lv(s))]
    for s, c in ((2, 256), (1, 128), (0, 64)):
        out += [(2 * c, c, N, *lv(s)), (c, c, N, *lv(s))]
    return out


def saved_bytes(N, D, H, W, dt):
    es = torch.empty((), dtype=dt).element_size()
    fused = [(ci, co, n, d, h, w) for ci, co, n, d, h, w in luconv_shapes(N, D, H, W) if ops.infer_fused_route(n, d, h, w, ci, co, ACT_RELU, dt)]
    return sum(2 * n * d * h * w * co * es for _, co, n, d, h, w in fused), len(fused)


def spread(v):
    q = statistics.quantiles(v, n=10)
    return 0.5 * (q[-1] - q[0])


def ab(model, x, reps, warm=3):
    arms = {"eval": lambda: model(x), "infer": lambda: model.infer(x)}
    for _ in range(warm):
        for f in arms.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(reps):
        for k, f in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    return times


def validate_wall(n_samples, b, dt, lines):
    from pcrlv2_amd import train_3d as T
    from pcrlv2_amd.main import SyntheticLunaLoader
    from pcrlv2_amd.optim import FusedSGD
    steps = (n_samples + b - 1) // b
    torch.manual_seed(0)
    model = PCRLv23d().cuda().set_compute_dtype(dt)
    opt = FusedSGD(model.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
    crit, cosine = T.MSELoss(), T.CosineSimilarityMean()
    ev, tr = SyntheticLunaLoader(b, steps, seed=11), SyntheticLunaLoader(b, steps, seed=12)
    model.train()
    T.validate(model, SyntheticLunaLoader(b, 2, seed=13), 0)          # warm both paths
    for batch in SyntheticLunaLoader(b, 3, seed=14):
        T.train_step(model, opt, batch, 0, crit, cosine)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    val = T.validate(model, ev, 0)
    t1 = time.perf_counter()
    for batch in tr:
        T.train_step(model, opt, batch, 0, crit, cosine)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    lines.append(f"validate over {val['n']} synthetic samples (b = {b}, {dt}): {t1 - t0:.2f} s wall; one training epoch of the same size ({steps} steps): {t2 - t1:.2f} s wall")
    lines.append("  validate -> " + "  ".join(f"{k} {v:.5f}" for k, v in val.items() if k != "n"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--shapes", default="32x64x64x32,8x128x128x64")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--out", default="")
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--validate-wall", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("val_forward_probe: no GPU -- this probe measures, it does not fall back")
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    lines = [f"eval-mode forward A/B, {a.dtype}, {torch.cuda.get_device_name(0)}; times from device events, arms alternating, {a.reps} repetitions each after 3 warm-up rounds"]
    torch.manual_seed(0)
    model = PCRLv23d().cuda().set_compute_dtype(dt)
    model.eval()
    ok = True
    for spec in [s for s in a.shapes.split(",") if s]:
        N, D, H, W = (int(v) for v in spec.split("x"))
        x = torch.randn(N, 1, D, H, W, device="cuda")
        if a.trace_only:
            ab(model, x, 3, warm=1)
            continue
        t = ab(model, x, a.reps)
        med = {k: statistics.median(v) for k, v in t.items()}
        sp = {k: spread(v) for k, v in t.items()}
        gap, noise = med["eval"] - med["infer"], sp["eval"] + sp["infer"]
        nbytes, nf = saved_bytes(N, D, H, W, dt)
        faster = gap > noise
        ok = ok and faster
        lines.append(f"b = {N}, {D}x{H}x{W}: eval {med['eval']:.3f} ms (spread +-{sp['eval']:.3f}, min {min(t['eval']):.3f})   infer {med['infer']:.3f} ms "
                     f"(spread +-{sp['infer']:.3f}, min {min(t['infer']):.3f})   gap {gap:.3f} ms vs combined spread {noise:.3f} ms -> "
                     f"{'fused faster beyond the spread' if faster else 'NOT faster beyond the spread'}")
        lines.append(f"    {nf} of 14 LUConvs fused; bytes no longer moved (one write + one read of their pre-normalisation tensors): {nbytes / 1e9:.3f} GB "
                     f"= {nbytes / 1e9 / max(gap, 1e-9) * 1e3 / 1e3:.2f} TB/s if the whole gap were these bytes")
        del x
        torch.cuda.empty_cache()
    if a.validate_wall:
        validate_wall(a.validate_wall, 32, dt, lines)
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if (ok or a.trace_only) else 2


if __name__ == "__main__":
    raise SystemExit(main())
