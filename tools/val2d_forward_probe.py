"""A/B of the 2D eval-mode forward: model.eval()(x) (conv + apply (+ add) as separate passes per layer, every deep-supervision map upsampled and
stored) against PCRLv2.infer(x, upsample=False) (normalisation, identity and activation in the convolution's epilogue; what train_2d.validate runs
on view 1) -- same process, same weights, same input, warmed, ALTERNATING, device-event times around `--fwd` forwards per sample.

    python tools/val2d_forward_probe.py [--rounds 5] [--fwd 20] [--out profiles/val2d_forward_probe.txt] [--shapes 64x224,384x96] [--dtype bf16]
    python tools/val2d_forward_probe.py --trace-only --shapes 64x224        # one warm-up + 3 forwards per arm, for `rocprofv3 --kernel-trace --stats -- python ...`
    python tools/val2d_forward_probe.py --validate-wall 40                   # one validate pass over N synthetic held-out batches next to N training steps

Beside the times it prints, from the shapes alone, the algorithmic bytes both forms move through the convolution + normalisation (+ add) layers and
the deep-supervision maps (weights and the small head tensors left out): per layer the unfused form reads the input, writes y, reads y, writes a
(and with a residual reads a and the identity and writes again); the fused form reads the input (and the identity) and writes a once.  A third arm,
`infer` with ops2d.INFER_FUSED_2D off, separates the epilogues' share from what the stem's pooled normalisation and the missing upsampling save.
The verdict per shape: `infer` counts as not slower when median(eval) - median(infer) > -(the two arms' combined spread); spread = half the range
of the per-round times."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from pcrlv2_amd import ops2d  # noqa: E402
from pcrlv2_amd.models import PCRLv2  # noqa: E402
from val2d_state import model_layers  # noqa: E402


def layer_bytes(N, side, dt):
    """-> (unfused bytes, fused bytes, layers in one pass, layers) of the Conv2d + BatchNorm2d layers and the five deep-supervision maps."""
    es = torch.empty((), dtype=dt).element_size()
    unf = fus = 0
    one = tot = 0
    for Ci, Co, K, s, p, up, H, _bias, res, _relu in model_layers(side):
        Ho = ((2 * H if up else H) + 2 * p - K) // s + 1
        xin, out = N * H * H * Ci * es, N * Ho * Ho * Co * es
        stem = K == 7
        u = xin + 3 * out + (3 * out if res else 0)                  # conv: read x, write y; apply: read y, write a; add: read a, identity, write
        if stem:
            u += out + out // 4                                       # max-pool: read a, write the pooled tensor
        full = stem or ops2d.infer_fused_route2d(N, H, H, Ci, Co, K, K, s, p, up, dt, residual=res)
        part = res and not full and ops2d.infer_fused_route2d(N, H, H, Ci, Co, K, K, s, p, up, dt)
        if stem:
            f = xin + out + out + out // 4                            # conv writes y; normalisation + ReLU inside the pool
        elif full:
            f = xin + out + (out if res else 0)
        elif part:
            f = xin + out + 3 * out
        else:
            f = u
        unf, fus = unf + u, fus + f
        one, tot = one + int(bool(full)), tot + 1
    for i in range(5):                                               # deep-supervision maps: 3 float32 channels at side / 2^(4-i)
        low, fullres = N * (side >> (4 - i)) ** 2 * 3 * 4, N * side * side * 3 * 4
        unf += 2 * low + fullres                                     # write low, read low, write the upsampled map (validate's MSE would read it again)
        fus += low
    return unf, fus, one, tot


def timed(f, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def ab(model, x, rounds, fwd, warm=3):
    def unfused_infer():
        ops2d.INFER_FUSED_2D = False
        try:
            model.infer(x, upsample=False)
        finally:
            ops2d.INFER_FUSED_2D = True
    arms = {"eval": lambda: model(x), "infer": lambda: model.infer(x, upsample=False), "infer, epilogues off": unfused_infer}
    for _ in range(warm):
        for f in arms.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for k, f in arms.items():
            times[k].append(timed(f, fwd))
    return times


def validate_wall(batches, b, side, dt, lines):
    from pcrlv2_amd import train_2d as T
    from pcrlv2_amd.main import SyntheticChestLoader
    from pcrlv2_amd.optim import FusedSGD
    from pcrlv2_amd.train_3d import CosineSimilarityMean
    torch.manual_seed(0)
    model = PCRLv2().cuda().set_compute_dtype(dt)
    opt = FusedSGD(model.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
    crit, cosine = T.MSELoss2d(), CosineSimilarityMean()
    model.train()
    T.validate(model, SyntheticChestLoader(b, 2, side, seed=13), 0)          # warm both paths
    for batch in SyntheticChestLoader(b, 3, side, seed=14):
        T.train_step(model, opt, batch, 0, crit, cosine)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    val = T.validate(model, SyntheticChestLoader(b, batches, side, seed=11), 0)
    t1 = time.perf_counter()
    for batch in SyntheticChestLoader(b, batches, side, seed=12):
        T.train_step(model, opt, batch, 0, crit, cosine)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    lines.append(f"SYNTHETIC held-out stream, {batches} batches of b = {b} at {side}^2 + 6 x 96^2 ({dt}): validate {1e3 * (t1 - t0) / batches:.1f} ms per batch "
                 f"({t1 - t0:.2f} s wall, {val['n']} samples); training step {1e3 * (t2 - t1) / batches:.1f} ms per batch")
    lines.append("  validate -> " + "  ".join(f"{k} {v:.5f}" for k, v in val.items() if k != "n"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--fwd", type=int, default=20)
    ap.add_argument("--shapes", default="64x224,384x96")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--out", default="")
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--validate-wall", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("val2d_forward_probe: no GPU -- this probe measures, it does not fall back")
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    lines = [f"2D eval-mode forward A/B, {a.dtype}, {torch.cuda.get_device_name(0)}; device events around {a.fwd} forwards per sample, arms alternating, "
             f"{a.rounds} rounds after 3 warm-up rounds"]
    torch.manual_seed(0)
    model = PCRLv2().cuda().set_compute_dtype(dt)
    model.eval()
    ok = True
    for spec in [s for s in a.shapes.split(",") if s]:
        N, side = (int(v) for v in spec.split("x"))
        x = torch.randn(N, 3, side, side, device="cuda")
        if a.trace_only:
            ab(model, x, 1, 3, warm=1)
            continue
        t = ab(model, x, a.rounds, a.fwd)
        med = {k: statistics.median(v) for k, v in t.items()}
        sp = {k: 0.5 * (max(v) - min(v)) for k, v in t.items()}
        gap, noise = med["eval"] - med["infer"], sp["eval"] + sp["infer"]
        unf, fus, one, tot = layer_bytes(N, side, dt)
        not_slower = gap > -noise
        ok = ok and not_slower
        for k in t:
            lines.append(f"b = {N}, {side}^2  {k:22s} median {med[k]:.3f} ms  (spread +-{sp[k]:.3f}, rounds " + " ".join(f"{v:.3f}" for v in t[k]) + ")")
        lines.append(f"    eval - infer = {gap:.3f} ms vs combined spread {noise:.3f} ms -> infer is "
                     f"{'faster beyond the spread' if gap > noise else ('not slower beyond the spread' if not_slower else 'SLOWER beyond the spread')}")
        lines.append(f"    algorithmic bytes from the shapes (conv + BatchNorm (+ add) layers and deep-supervision maps): eval {unf / 1e9:.3f} GB, infer {fus / 1e9:.3f} GB; "
                     f"{one} of {tot} layers in one pass")
        del x
        torch.cuda.empty_cache()
    if a.validate_wall:
        validate_wall(a.validate_wall, 64, 224, dt, lines)
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if (ok or a.trace_only) else 2


if __name__ == "__main__":
    raise SystemExit(main())
