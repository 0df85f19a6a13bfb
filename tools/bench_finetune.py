"""Probe of supervised 2D fine-tuning (not bench.py): three measurements in one process, warmed, device-event times, alternating arms.

  step    images/s of train_finetune.train_step at --b (64) x 3 x 224 x 224, bf16 unless --fp32, on a fixed generated batch; next to it the same step
          with the head COMPOSED from existing pieces (arm "composed"), so the step time shows what the fused head's launch count is worth
  head    forward + backward of the fused head (pcrl_cls_head_fwd / _bwd: 2 + 2 launches) on a [b, 7, 7, 512] activation, next to the same arithmetic
          composed from ops2d.gap_forward, torch dropout, ops.linear_forward, torch sigmoid + binary_cross_entropy and their backwards
          (torch autograd for the torch pieces, ops.linear_backward, ops2d.gap_backward)
  auroc   ops2d.auroc at M = 11 218 rows (the chest validation list), K = 14: the launch plus its one host read-back

    python tools/bench_finetune.py [--b 64] [--rounds 7] [--iters 20] [--fp32] [--out FILE]

Per arm: the median over --rounds of the mean over --iters, and the spread (half the range of the rounds).  A difference smaller than the two arms'
combined spread is reported as "no difference measured".  No test asserts any of these numbers."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from pcrlv2_amd import functions as Fn  # noqa: E402
from pcrlv2_amd import ops, ops2d  # noqa: E402
from pcrlv2_amd.main import SyntheticLabelledChestLoader  # noqa: E402
from pcrlv2_amd.models import ChestClassifier  # noqa: E402
from pcrlv2_amd.optim import FusedSGD  # noqa: E402
from pcrlv2_amd.train_finetune import train_step  # noqa: E402


def timed(f, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def alternate(arms, rounds, iters, warm=3):
    for f in arms.values():
        for _ in range(warm):
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in arms}
    for _ in range(rounds):
        for k, f in arms.items():
            ts[k].append(timed(f, iters))
    return {k: (statistics.median(v), (max(v) - min(v)) / 2) for k, v in ts.items()}


def verdict(res, a, b):
    d = res[b][0] - res[a][0]
    noise = res[a][1] + res[b][1]
    if abs(d) <= noise:
        return f"no difference measured between {a} and {b} ({d * 1e3:+.1f} us within +-{noise * 1e3:.1f} us)"
    return f"{a} is {'faster' if d > 0 else 'SLOWER'} than {b} by {abs(d) * 1e3:.1f} us (spread +-{noise * 1e3:.1f} us)"


class ComposedHeadFn(torch.autograd.Function):
    """The head from existing pieces, for the A/B only: gap_forward -> torch dropout -> linear_forward -> torch sigmoid + BCE, and back."""

    @staticmethod
    def forward(ctx, a, w, b, labels, p, mod):
        dt = mod.compute_dtype
        g = ops2d.gap_forward(a, dt)
        with torch.enable_grad():
            gl = g.detach().requires_grad_(True)
            gd = F.dropout(gl, p, training=True) if p > 0 else gl
        z = ops.linear_forward(gd.detach().contiguous(), w, b)
        with torch.enable_grad():
            zl = z.detach().requires_grad_(True)
            probs = torch.sigmoid(zl)
            loss = F.binary_cross_entropy(probs, labels.float())
        ctx.a, ctx.dt, ctx.t = a, dt, (gl, gd, zl, loss)
        ctx.plist = (w, b)
        return loss.detach(), probs.detach()

    @staticmethod
    def backward(ctx, dloss, _dp):
        gl, gd, zl, loss = ctx.t
        w, b = ctx.plist
        (dz,) = torch.autograd.grad(loss, zl, dloss)
        dgd, dw, db = ops.linear_backward(dz.contiguous(), gd.detach().contiguous(), w)
        dg = torch.autograd.grad(gd, gl, dgd)[0] if gd is not gl else dgd
        da = ops2d.gap_backward(dg, ctx.a, ctx.dt)
        return da, Fn._park(w, dw), Fn._park(b, db), None, None, None


def composed_loss(model, x, labels):
    ops2d.bump_stats_epoch()
    pi = ops.next_pass()
    for u in model.encoder._units():
        u._pass_idx = pi
    h = model.encoder.forward_last(x)
    lin = model.classification_head[3]
    return ComposedHeadFn.apply(h, lin.weight, lin.bias, labels, model.dropout, model)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--fp32", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_finetune.py measures on the GPU; there is nothing to measure without one")
    dev = torch.device("cuda")
    dt = torch.float32 if a.fp32 else torch.bfloat16
    out = {"b": a.b, "dtype": str(dt), "device": torch.cuda.get_device_name(0)}
    lines = []

    # ---- step ----
    torch.manual_seed(0)
    model = ChestClassifier().cuda().set_compute_dtype(dt)
    model.train()
    model.mask_generator = torch.Generator(device=dev).manual_seed(1)
    opt = FusedSGD(model.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
    x, y = next(iter(SyntheticLabelledChestLoader(a.b, 1, 224, 14, seed=0, device=dev)))
    fused_loss = model.loss

    def step(loss_fn):
        def run():
            model.loss = loss_fn
            try:
                train_step(model, opt, (x, y))
            finally:
                model.loss = fused_loss
        return run

    res = alternate({"fused": step(fused_loss), "composed": step(lambda xx, yy: composed_loss(model, xx, yy))}, a.rounds, max(a.iters // 2, 5), warm=5)
    for k, (m, s) in res.items():
        lines.append(f"step  {k:9s} {m:8.3f} ms +-{s:.3f}   {a.b / m * 1e3:9.1f} images/s")
        out[f"step_{k}_ms"], out[f"step_{k}_spread_ms"], out[f"step_{k}_images_per_s"] = m, s, a.b / m * 1e3
    lines.append("step  " + verdict(res, "fused", "composed"))

    # ---- head ----
    torch.manual_seed(1)
    act = torch.relu(torch.randn(a.b, 7, 7, 512, device=dev)).to(dt).permute(0, 3, 1, 2)
    lin = model.classification_head[3]
    w, bias = lin.weight.detach(), lin.bias.detach()
    keep = (torch.rand(a.b, 512, device=dev) >= 0.2).to(torch.uint8)
    one = torch.ones((), device=dev)

    def fused_head():
        probs, pooled, loss = ops2d.cls_head_forward(act, w, bias, dt, keep=keep, p=0.2, labels=y)
        ops2d.cls_head_backward(probs, y, one, pooled, w, act, dt, keep=keep, p=0.2)

    yf = y.float()

    def composed_head():
        g = ops2d.gap_forward(act, dt).requires_grad_(True)
        gd = F.dropout(g, 0.2, training=True)
        z = ops.linear_forward(gd.detach().contiguous(), w, bias).requires_grad_(True)
        loss = F.binary_cross_entropy(torch.sigmoid(z), yf)
        (dz,) = torch.autograd.grad(loss, z)
        dgd, _dw, _db = ops.linear_backward(dz.contiguous(), gd.detach().contiguous(), w)
        (dg,) = torch.autograd.grad(gd, g, dgd)
        ops2d.gap_backward(dg, act, dt)

    res = alternate({"fused": fused_head, "composed": composed_head}, a.rounds, a.iters * 5)
    for k, (m, s) in res.items():
        lines.append(f"head  {k:9s} {m * 1e3:8.1f} us +-{s * 1e3:.1f}")
        out[f"head_{k}_us"], out[f"head_{k}_spread_us"] = m * 1e3, s * 1e3
    lines.append("head  " + verdict(res, "fused", "composed"))

    # ---- auroc ----
    M, K = 11218, 14
    g = torch.Generator(device=dev).manual_seed(2)
    probs = torch.rand(M, K, device=dev, generator=g)
    labels = (torch.rand(M, K, device=dev, generator=g) < 0.05).to(torch.uint8)
    res = alternate({"auroc": lambda: ops2d.auroc(probs, labels), "counts only": lambda: ops2d.auroc_counts(probs, labels)}, a.rounds, a.iters)
    for k, (m, s) in res.items():
        lines.append(f"auroc {k:11s} {m * 1e3:8.1f} us +-{s * 1e3:.1f}   (M = {M}, K = {K}: {M * M * K / 1e9:.2f}e9 row pairs walked)")
        out[f"auroc_{k.replace(' ', '_')}_us"] = m * 1e3
    print("\n".join(lines))
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n" + json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
