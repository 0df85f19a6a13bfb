"""Measurements of DESIGN.md section 23 (the fine-tuning optimisers), one JSON line per measurement.

    python tools/bench_optim.py [--rounds 7] [--window_ms 200] [--out profiles/optim_bench.txt]

On the arenas of PCRLv23d (17.1 M parameters) and of the 2D chest classifier, laid out as optim.FusedSGD lays them out (slots padded to 4 floats,
every tensor with a gradient), through the C ABI:
  sgd        pcrl_sgd_step -- the pre-training kernel, the yardstick: 20 bytes per element (p, g, buf read; p, buf written);
  adam       pcrl_adam_prepare + pcrl_adam_step: 28 bytes per element (p, g, m, v read; p, m, v written);
  adam_clip  the same with a device clip coefficient;
  norm       pcrl_grad_norm (two launches): 4 bytes per element.
The arms alternate inside one process, each warmed; a timed window is as many calls as fill about `window_ms` of device time between two device
events (tools/bench_seg.py's rounds) -- times PER CALL, launch overhead included, not kernel times.  Reported: the median over the rounds, the spread
(max - min), the bytes the pass needs and that over the time.  `check`: the Adam step's time against 7/5 of the SGD step's on the same box -- the ratio
of their bytes -- with up to 1.3x of that accepted for the square root's and the divisions' latency; the norm's rate against the SGD kernel's rate.

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
from pcrlv2_amd._lib import lib, stream_handle  # noqa: E402

DEV = torch.device("cuda")
LR, WD, B1, B2, EPS = 1e-3, 1e-2, 0.9, 0.999, 1e-8


def arena_of(model):
    slots = [(p.numel() + 3) // 4 * 4 for p in model.parameters()]
    offs = [0]
    for n in slots:
        offs.append(offs[-1] + n)
    return offs


def arms(offs):
    L, n, total = lib(), len(offs) - 1, offs[-1]
    g = torch.Generator(device=DEV).manual_seed(0)
    p, grad = torch.randn(total, generator=g, device=DEV), 1e-2 * torch.randn(total, generator=g, device=DEV)
    state = [torch.zeros(total, device=DEV) for _ in range(3)]      # momentum, exp_avg, exp_avg_sq
    od = torch.tensor(offs, dtype=torch.int64, device=DEV)
    flags = torch.full((n,), 3, dtype=torch.int32, device=DEV)
    steps, prods, coefs = torch.zeros(n, dtype=torch.int32, device=DEV), torch.ones(2 * n, dtype=torch.float64, device=DEV), torch.zeros(2 * n, device=DEV)
    parts = torch.zeros(L.fn["pcrl_optim_grid_cap"][0](), dtype=torch.float64, device=DEV)
    norm, coef = torch.zeros(1, dtype=torch.float64, device=DEV), torch.ones(1, device=DEV)

    def adam(clip):
        s = stream_handle()
        L.call("pcrl_adam_prepare", flags, steps, prods, coefs, n, LR, B1, B2, s)
        L.call("pcrl_adam_step", p, grad, state[1], state[2], od, flags, coefs, n, total, 1.0 - LR * WD, 1, 1.0 - B1, B2, 1.0 - B2, EPS, 1.0, clip, s)

    return {"sgd": lambda: L.call("pcrl_sgd_step", p, grad, state[0], od, flags, n, total, LR, 0.9, 1e-4, 1.0, stream_handle()),
            "adam": lambda: adam(None), "adam_clip": lambda: adam(coef),
            "norm": lambda: L.call("pcrl_grad_norm", grad, od, None, flags, n, total, 1.0, 1.0, parts, norm, coef, stream_handle())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window_ms", type=float, default=200.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_optim.py measures on the GPU; none is visible")
    from pcrlv2_amd.models import PCRLv23d
    from pcrlv2_amd.models.pcrlv2_model import ChestClassifier
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    emit({"bench": "device", "name": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_ms": args.window_ms})
    per_element = {"sgd": 20, "adam": 28, "adam_clip": 28, "norm": 4}
    for name, model in (("PCRLv23d", PCRLv23d()), ("ChestClassifier", ChestClassifier())):
        offs = arena_of(model)
        res = rounds(arms(offs), args.rounds, args.window_ms)
        for arm, (med, spread) in res.items():
            need = per_element[arm] * offs[-1]
            emit({"bench": "optim", "arena": name, "elements": offs[-1], "tensors": len(offs) - 1, "arm": arm, "ms": round(med, 5), "spread_ms": round(spread, 5),
                  "bytes_needed": need, "TB_per_s": round(need / (med * 1e-3) / 1e12, 3)})
        ratio = res["adam"][0] / res["sgd"][0]
        emit({"bench": "check", "arena": name, "adam_over_sgd": round(ratio, 3), "by_bytes": 1.4, "accepted_up_to": round(1.4 * 1.3, 2), "met": bool(ratio <= 1.4 * 1.3),
              "norm_rate_over_sgd_rate": round((4 / res["norm"][0]) / (20 / res["sgd"][0]), 3)})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
