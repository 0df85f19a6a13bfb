#!/usr/bin/env python3
"""bench.py -- BASELINE.json's metric on its named configuration.

  metric   : 3D crops/sec of the full PCRLv2 pre-training step (2 global 64x64x32 views + 6 local 16^3 views per crop,
             forward + backward + SGD), b = 32 crops per GPU, synthetic data resident in HBM, bf16 activations / MFMA
             operands with fp32 accumulation (BASELINE config C2; C3 with --gpus N, weak scaling).
  step     : one pass of train_3d.train_step over one batch.
  roofline : the dominant kernel (bf16 LDS-halo implicit-GEMM 3x3x3 convolution, forward + data-gradient launches): algorithmic
             FLOPs (2*M*27*Ci*Co per launch) / launch duration measured with HIP events on the launch stream, against
             the dense bf16 MFMA peak (2.5 PFLOP/s, /opt/skills/guides/MI355X_MICROARCH.md).  The step runs on three streams (the
             second global view; weight gradients and the decoder's side branches), so in the timed region this kernel SHARES the chip --
             two convolutions side by side each see about half of it, and how much depends on how the streams line up.  The roofline figure
             is therefore taken over 10 extra ONE-STREAM steps run right after the timed region (same process, model, batch): the kernel's
             rate with the chip to itself, which the one-stream rocprofv3 summary (profiles/*_kernel_stats.txt) reproduces to < 1 %; its
             per-launch time inside the timed region is kept as roofline.in_timed_region (profiles/*_overlap_* is the three-stream trace).
             `value` is always the three-stream timed region.  With --no-alone the roofline is the timed region's.
  cpu_baseline : the CPU oracle (a port of the reference step, oracle/pcrlv2_oracle.py) timed on this box's host cores on
             a bounded sample (b=4, 2-3 timed steps, ~16-25 s), rank 0, N=1 only.

A plain run sets up, runs W warm-up steps, times K steps and prints the line: metric, value, ms_per_step (one timed step), config,
final_loss, step_mfma_frac (from value alone) and, for N > 1, the distributed block with its bucket-setting A/B.  Everything else -- the
per-kernel times and `roofline`, `diag`, `secondary` (C4, C5), `cpu_baseline` -- is measured only with --full (the --no-* switches apply
there).  --dump-outputs DIR writes what the last timed step computed (dump_outputs).

Launch: python bench.py [--gpus 1 --steps K --warmup W] [--full] [--dump-outputs DIR]   or, for N>1,
        python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...
Prints ONE JSON line on rank 0.
"""
import argparse
import collections
import json
import os
import random
import sys
import time
from types import SimpleNamespace as types_ns

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
# GPU_MAX_HW_QUEUES stays at ROCm's default (4): see pcrlv2_amd/__init__.py (8 costs 7.5 ms per step once RCCL is initialised)

import torch  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0   # dense bf16 MFMA, MI355X_MICROARCH.md "Peak BF16/FP16 MFMA ~2.5 PF dense"
FLOP_PER_CROP = 1.2707e12   # fwd+bwd of one crop (2 global + 6 local views), SURVEY 8(d) [torch flop counter on the reference]


ALG_BYTES = collections.Counter()   # key -> algorithmic HBM bytes of the launches seen (input + output + packed weights, each once)


def conv_key(name, args):
    """Classify a pcrl_conv3d_k3_fwd launch the way the library's dispatcher does (conv_igemm.hip / conv_brick.hip) and
    return its algorithmic FLOPs (2 * voxels * 27 * Ci * Co)."""
    # pcrl_conv3d_k3_fwd_ws(x, wp, bias, y, stats, ws, ws_bytes, N, D, H, W, Ci, Co, dtype, stream)   [_fwd: without ws, ws_bytes]
    if name == "pcrl_conv3d_k3_dgrad_bnred":
        # (dy, wp, dx, bn_y, scale, shift, mean, rstd, partial, N, D, H, W, Ci, Co, act, dtype, stream): the wide-brick data gradient with the first pass of
        # the BatchNorm backward of the layer below in its epilogue -- its own instantiation (conv_brick16_bnr.hip), its own row; it also reads bn_y
        N, D, H, W, Ci, Co = args[9:15]
        key = "brick16_conv_kernel<dgrad+bn_reduce>"
        ALG_BYTES[key] += 2.0 * (N * D * H * W * (Ci + 2 * Co) + 27 * Ci * Co)
        return key, 2.0 * N * D * H * W * 27 * Ci * Co
    N, D, H, W, Ci, Co, dt = args[7:14] if name == "pcrl_conv3d_k3_fwd_ws" else args[5:12]
    from pcrlv2_amd import _lib
    kid = _lib.lib().call("pcrl_conv3d_k3_fwd_kernel", N, D, H, W, Ci, Co, dt)
    if kid == 2:
        key = "brick16_conv_kernel"
    elif kid == 1:
        key = "brick_conv_kernel"
    else:
        bn = 128 if Co % 128 == 0 else (64 if Co % 64 == 0 else 32)
        key = "igemm_kernel<%s,%d,conv3>(+split-K finish)" % ("bf16" if dt == 1 else "f32", bn)
    ALG_BYTES[key] += 2.0 * (N * D * H * W * (Ci + Co) + 27 * Ci * Co)
    return key, 2.0 * N * D * H * W * 27 * Ci * Co


def wgrad_key(name, args):
    # pcrl_conv3d_k3_wgrad(x, dy, dw, ws, ws_bytes, N, D, H, W, Ci, Co, dtype, stream)
    N, D, H, W, Ci, Co, dt = args[5:12]
    if dt == 1 and Co % 64 == 0 and ((D % 2 == 0 and H % 8 == 0 and W % 8 == 0) or (W % 2 == 0 and D % 8 == 0 and H % 8 == 0)):
        key = "wgrad_brick_kernel(+reduce)"
    else:
        key = "wgrad_kernel<%s,conv3>(+reduce)" % ("bf16" if dt == 1 else "f32")
    return key, 2.0 * N * D * H * W * 27 * Ci * Co


def upconv_key(name, args):
    """The composed ConvTranspose3d -> Conv3d operator (csrc/upconv_fused.hip): EXECUTED flops = 8 phases x 8 coarse taps per coarse voxel
    (the 27-tap convolution over the upsampled tensor it replaces would be 27/8 of that, plus the transposed convolution)."""
    from pcrlv2_amd import _lib
    L = _lib.lib()
    if name == "pcrl_upconv_fwd":       # (x, wf, w3f, tab, y0, stats, N, D, H, W, Ci, Co, dtype, stream)
        N, D, H, W, Ci, Co, dt = args[6:13]
        # the wide-brick kernel's composed instantiations are separate kernels (template arguments <64, 1> forward, <64, 2> data gradient)
        brick = L.call("pcrl_upconv_fwd_uses_brick", N, D, H, W, Ci, Co, dt)
        key = "brick16_conv_kernel<upconv_fwd>" if brick else "igemm_kernel<%s,upconv_fwd>" % ("bf16" if dt == 1 else "f32")
    elif name in ("pcrl_upconv_dgrad", "pcrl_upconv_dgrad_ws"):   # (dy0, wd, wd3, dx, [ws, ws_bytes,] N, D, H, W, Ci, Co, dtype, stream)
        N, D, H, W, Ci, Co, dt = args[6:13] if name.endswith("_ws") else args[4:11]
        brick = L.call("pcrl_upconv_dgrad_uses_brick", N, D, H, W, Ci, Co, dt)
        key = "brick16_conv_kernel<upconv_dgrad>" if brick else "igemm_kernel<%s,upconv_dgrad>" % ("bf16" if dt == 1 else "f32")
    else:                               # pcrl_upconv_wgrad_accum(x, dy0, dweff, box, first, ws, ws_bytes, N, D, H, W, Ci, Co, dtype, stream)
        N, D, H, W, Ci, Co, dt = args[7:14]
        brick = dt == 1 and Co % 64 == 0 and ((D % 2 == 0 and H % 8 == 0 and W % 8 == 0) or (W % 2 == 0 and D % 8 == 0 and H % 8 == 0))
        key = "wgrad<%s,upconv,%s>(+reduce, class sums)" % ("bf16" if dt == 1 else "f32", "brick kernel" if brick else "gather kernel")
    return key, 2.0 * N * D * H * W * 64 * Ci * Co


def keyfn(name, args):
    if name.startswith("pcrl_upconv"):
        return upconv_key(name, args)
    return conv_key(name, args) if name.startswith(("pcrl_conv3d_k3_fwd", "pcrl_conv3d_k3_dgrad")) else wgrad_key(name, args)


def synthetic_batch(b, dhw, local, device, seed, nlocal=6):
    """x1 ~ N(0,1), x2 = x1 + 0.1 N(0,1) (correlated views), gt ~ U(0,1), 6 local N(0,1) crops."""
    g = torch.Generator().manual_seed(seed)
    D, H, W = dhw
    x1 = torch.randn(b, 1, D, H, W, generator=g)
    x2 = x1 + 0.1 * torch.randn(b, 1, D, H, W, generator=g)
    gt = torch.rand(b, 1, D, H, W, generator=g)
    loc = [torch.randn(b, 1, local, local, local, generator=g) for _ in range(nlocal)]
    to = lambda t: t.to(device)
    return to(x1), to(x2), to(gt), None, [to(t) for t in loc]


DUMP_STATE_SAMPLE = 1 << 22     # float32 elements of the model state written by --dump-outputs (16 MB; the whole state is ~68 MB)


def dump_outputs(out_dir, losses, model):
    """--dump-outputs: what a caller of train_step holds after the last timed step, as float32 .npy files -- the five losses it returned
    (loss, loss1, loss2, loss4, local_loss) and the model state its SGD step left (parameters and BatchNorm running statistics, flattened in
    state_dict order; `state_sample.npy`: the same DUMP_STATE_SAMPLE positions in every run, drawn with seed 0, ascending).  Every input of the
    run is seeded, so two builds given the same arguments can be compared file by file."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    for name, v in zip(("loss", "loss1", "loss2", "loss4", "local_loss"), losses):
        np.save(os.path.join(out_dir, name + ".npy"), v.detach().float().cpu().numpy())
    state = [v.detach().reshape(-1).float() for v in model.state_dict().values() if v.is_floating_point()]
    if state:
        flat = torch.cat(state)
        n = flat.numel()
        idx = torch.randperm(n, generator=torch.Generator().manual_seed(0))[:min(n, DUMP_STATE_SAMPLE)].sort().values
        np.save(os.path.join(out_dir, "state_sample.npy"), flat[idx.to(flat.device)].cpu().numpy())


def cpu_baseline(b=4, budget_s=18.0, threads=None):
    """Time the oracle port of the reference step on the host cores (fp32, default oneDNN) on a BOUNDED sample, following
    BASELINE.md section 3: b = 4 full-size (64x64x32 + 6 x 16^3) crops, one warm-up step (at 32x32x16: it only pages the code in), then
    up to 3 timed steps or ~budget_s (15 s: VERDICT r4 -- it was 80 % of the driver's run at 35 s) of CPU work, whichever comes first (>= 1 step).
    Threads: min(32, cores) -- with all 256 hardware threads of the GPU box a step is >10x SLOWER (oversubscribed oneDNN / ATen
    threading: measured 279 s for b = 2), so "all cores" of the plan is not a fair baseline on that host; the count used is reported."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import pcrlv2_oracle as O
    cores = os.cpu_count() or 1
    torch.set_num_threads(threads or min(32, cores))
    model_name = "unknown"
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                model_name = ln.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    st = O.fill_state(torch.float32)
    O.train_steps(st, [O.fill_batch(2, (32, 32, 16), local=16, dtype=torch.float32, seed=3)])   # warm-up
    per, t0 = [], time.time()
    while True:
        t1 = time.time()
        O.train_steps(st, [O.fill_batch(b, (64, 64, 32), local=16, dtype=torch.float32, seed=7 + len(per))])
        per.append(time.time() - t1)
        dt = time.time() - t0
        # at least TWO timed steps (one step is a sample of one), then up to 3 or ~budget_s
        if len(per) >= 2 and (dt + dt / len(per) > budget_s or len(per) >= 3):
            break
    steps = len(per)
    return {"value": round(b * steps / dt, 4), "unit": "crops/s", "cores": torch.get_num_threads(), "kind": "port",
            "n_timed_steps": steps, "s_per_step": [round(v, 2) for v in per], "value_best_step": round(b / min(per), 4),
            "sample": f"oracle port of train_3d.py:109-151 (oracle/pcrlv2_oracle.py), fp32 oneDNN, b={b}, 64x64x32 + 6x16^3, "
                      f"n = {steps} timed steps in {dt:.1f} s (value = mean rate, value_best_step = the fastest step's) on "
                      f"{torch.get_num_threads()} of {cores} host threads ({model_name})"}



# ---- PCRL_BENCH_DRYRUN=1: the N-rank code path of this file on CPU (tests/test_host_cpu.py, world 4 over gloo) ------------------------------
# Everything that is bench.py's OWN -- the self-spawn of `--gpus N`, rank / device table, the four-setting bucket A/B, the barrier-bracketed
# timed region with MAX over ranks, the JSON line and its `distributed` block -- runs as it does on a node; only the step itself is replaced by a
# stub that parks KNOWN gradients through the engine's own parking / flush / bucket machinery (pcrlv2_amd.functions, ddp.DataParallel) and
# checks the all-reduced arena after every optimizer step.  No GPU, no library call.
class _DryEvent:
    def __init__(self, enable_timing=True):
        self.t = 0.0

    def record(self):
        self.t = time.perf_counter()

    def elapsed_time(self, other):
        return 1e3 * (other.t - self.t)


def _dryrun_parts(rank, world):
    import types
    from pcrlv2_amd import functions as Fn
    torch.manual_seed(0)
    shapes = [(300,), (7, 5), (2000,), (3,), (64, 8), (5000,)]
    params = [torch.nn.Parameter(torch.randn(s)) for s in shapes]
    sizes = [p.numel() for p in params]
    offs = [0]
    for n in sizes:
        offs.append(offs[-1] + n)
    flat_g = torch.full((offs[-1],), 123.0)
    opt = types.SimpleNamespace(_plist=params, flat_g=flat_g, flat_p=torch.cat([p.detach().reshape(-1) for p in params]).clone(),
                                _gviews=[flat_g[o:o + n].view(p.shape) for p, o, n in zip(params, offs, sizes)], grad_scale=1.0, pre_step=None,
                                steps=0, checked=0)
    opt.gather_grads = lambda: None
    model = torch.nn.Module()

    class Dot(torch.autograd.Function):      # stand-in for a stage Function: parks its parameter gradient, final when it ran in pass 0
        @staticmethod
        def forward(ctx, p, x, pass_idx):
            ctx.p, ctx.x, ctx.pass_idx = p, x, pass_idx
            return (p.detach() * x).sum()

        @staticmethod
        def backward(ctx, g):
            out = Fn._park(ctx.p, g * ctx.x)
            Fn.mark_final(ctx, [ctx.p])
            return out, None, None

    def train_step(model_, opt_, batch, epoch, crit, cosine, guard=False):
        k = opt_.steps
        for p in params:
            p.grad = None
        x = [torch.full(s_, float(rank + 1 + (k % 3))) for s_ in shapes]
        l0 = sum(Dot.apply(params[i], x[i], 0) for i in (0, 2, 4, 5))      # pass 0 (final); parameter 3 never gets a gradient, parameter 1 only a non-final one
        l1 = sum(Dot.apply(params[i], x[i], 1) for i in (0, 1, 2, 4, 5))
        (l0 + l1).backward()
        if opt_.pre_step is None:
            Fn.flush_param_grads()
        has = opt_.pre_step(opt_, None) if opt_.pre_step is not None else [p.grad is not None for p in params]
        assert has == [True, True, True, False, True, True], has
        tot = sum(r + 1 + (k % 3) for r in range(world))
        for i, v in enumerate(opt_._gviews):
            mult = {0: 2, 1: 1, 2: 2, 3: 0, 4: 2, 5: 2}[i]
            if has[i]:
                assert torch.allclose(v, torch.full_like(v, float(mult * tot))), ("dry-run gradient check", k, i, float(v.flatten()[0]), mult * tot)
        opt_.steps += 1
        opt_.checked += 1
        z = torch.zeros(())
        return torch.tensor(float(k)), z, z, z, z
    return model, opt, train_step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)     # >= 50 timed steps after >= 10 warm-up steps
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--b", type=int, default=32, help="crops per GPU")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--dhw", default="64,64,32")
    ap.add_argument("--full", action="store_true", help="also measure everything beyond the headline figure: per-kernel times and roofline, the "
                    "secondary configurations C4 / C5, the CPU baseline, per-step diagnostics")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write what the last one computed to DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-alone", action="store_true", help="with --full: skip the extra roofline.alone steps (rocprofv3 runs: the trace then holds the timed configuration only)")
    ap.add_argument("--nlocal", type=int, default=6, help="local views per crop (the reference's loader delivers 6; other values are a probe, labelled custom)")
    ap.add_argument("--no-secondary", action="store_true", help="with --full: skip the extra steps of BASELINE configs C4 (128x128x64, b=8) and C5 reported as `secondary`")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: start the N ranks ourselves (one process per GPU, torchrun rendezvous on
        # 127.0.0.1), as pcrlv2_amd/main.py does for `--gpus 0,1,..`.  Rank 0 of the children prints the JSON line.
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        r = subprocess.run(cmd, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"), stdout=subprocess.PIPE, text=True)
        for ln in r.stdout.splitlines():      # stdout carries exactly the JSON line; library chatter (gloo's connection notes) goes to stderr
            print(ln, file=sys.stdout if ln.startswith("{") else sys.stderr)
        raise SystemExit(r.returncode)

    # Every rank leaves through ddp.shutdown(): a barrier, then destroy_process_group().  A rank that falls off main() with the group alive
    # aborts now and then at interpreter exit ("terminate called without an active exception": gloo's / RCCL's threads are still running when
    # their statics go away) -- AFTER the JSON line, but torchrun then reports rc = 1 for the whole run (reproduced 1 in 4).
    from pcrlv2_amd import ddp
    ok = False
    try:
        _run(args)
        ok = True
    finally:
        ddp.shutdown(ok)


def _run(args):
    dry = os.environ.get("PCRL_BENCH_DRYRUN", "0") == "1"
    from pcrlv2_amd import ddp
    if not dry:
        from pcrlv2_amd import _lib
        from pcrlv2_amd.models import PCRLv23d
        from pcrlv2_amd.optim import FusedSGD
        from pcrlv2_amd.train_3d import CosineSimilarityMean, MSELoss, train_step

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank, local_rank = 0, 0
    if world > 1:
        # "nccl" IS RCCL on ROCm; PCRL_DIST_BACKEND=gloo lets the multi-rank code path be exercised with several ranks on ONE GPU
        rank, world, local_rank = ddp.init_process_group_from_env("gloo" if dry else os.environ.get("PCRL_DIST_BACKEND", "nccl"))
    if args.gpus != world and rank == 0:
        print(f"[bench] note: --gpus {args.gpus} but WORLD_SIZE={world}; using WORLD_SIZE", file=sys.stderr)
    # several ranks on fewer GPUs (PCRL_DIST_BACKEND=gloo on a one-GPU box): ranks share devices round-robin
    ndev = 0 if dry else torch.cuda.device_count()
    if dry:
        dev = torch.device("cpu")
    else:
        local_rank = local_rank % max(ndev, 1)
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)
    dist_info = None
    if world > 1:
        import torch.distributed as dist
        backend = dist.get_backend()
        # every rank reports its device; rank 0 keeps the table (proof that N ranks on N devices took part in the timed region)
        mine = {"rank": rank, "device": local_rank, "name": "cpu (dry run)" if dry else torch.cuda.get_device_name(local_rank)}
        table = [None] * world
        dist.all_gather_object(table, mine)
        ver = None
        if backend == "nccl":
            try:
                ver = ".".join(str(v) for v in torch.cuda.nccl.version())
            except Exception:
                ver = "unknown"
        dist_info = {"backend": backend + (" (RCCL)" if backend == "nccl" else ""), "rccl_version": ver, "world_size": dist.get_world_size(),
                     "visible_devices": ndev, "ranks": table}
        print(f"[bench] rank {rank}/{world} on {'cpu' if dry else 'cuda'}:{local_rank} backend={backend}", file=sys.stderr)
    dhw = tuple(int(v) for v in args.dhw.split(","))

    torch.manual_seed(0)
    random.seed(0)          # same scale draws on every rank (see ddp.DataParallel)
    if dry:
        model, opt, train_step = _dryrun_parts(rank, world)
    else:
        model = PCRLv23d().to(dev).train()
        model.set_compute_dtype(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
        opt = FusedSGD(model.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
    dp = ddp.DataParallel(model, opt) if world > 1 else None  # noqa: F841
    if world == 1 and os.environ.get("PCRL_FORCE_DDP", "0") == "1":
        # probe, not a BASELINE configuration: the data-parallel wrapper on a ONE-rank RCCL group (bucket sums on the communication stream,
        # the collectives, the guarded hooks all run for real) -- what the multi-rank code path costs on one GPU, labelled in the JSON line
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29577")
        dist.init_process_group("nccl", rank=0, world_size=1)
        dp = ddp.DataParallel(model, opt, force_collectives=True)  # noqa: F841
        dist_info = {"backend": "nccl (RCCL)", "world_size": 1, "forced_one_rank_probe": True}
    crit, cosine = (None, None) if dry else (MSELoss(), CosineSimilarityMean())
    batch = None if dry else synthetic_batch(args.b, dhw, 16, dev, 1234 + rank, args.nlocal)
    sync = (lambda: None) if dry else torch.cuda.synchronize
    Event = _DryEvent if dry else torch.cuda.Event

    def barrier():
        sync()
        if world > 1:
            torch.distributed.barrier()
        sync()

    L = types_ns() if dry else _lib.lib()
    # same-box A/B of launch variants (tools/conv_probe.py documents the codes); not used by the default run
    if os.environ.get("PCRL_DEBUG_CONV_IMPL"):
        L.debug_set_conv_impl(int(os.environ["PCRL_DEBUG_CONV_IMPL"]))
    if os.environ.get("PCRL_DEBUG_WGRAD_IMPL"):
        L.debug_set_wgrad_impl(int(os.environ["PCRL_DEBUG_WGRAD_IMPL"]))
    for _ in range(args.warmup):
        train_step(model, opt, batch, 0, crit, cosine, guard=False)
    # N > 1: where the gradient buckets are launched from (inside backward as they become final, or all from optimizer.step()) and how many
    # there are is decided by MEASUREMENT on this node, before the timed region: 6 steps of each of the four settings (same draws), the
    # fastest (max over ranks) is used for the timed region and all four are reported (distributed.ab).  Results do not depend on the setting.
    ddp_ab = None
    if dp is not None and getattr(dp, "_active", False) and os.environ.get("PCRL_BENCH_DDP_AB", "1") != "0":
        mb = 0.004 if dry else 24.0      # the dry run's stand-in parameters are ~30 KB: ~1000-float buckets there, so that several go out
        settings = collections.OrderedDict([("from_step_buckets24MB", (False, mb)), ("overlap_buckets24MB", (True, mb)),
                                            ("from_step_1bucket", (False, 1e6)), ("overlap_1bucket", (True, 1e6))])
        st0 = random.getstate()
        ddp_ab = {}
        for name, (ov, mb) in settings.items():
            dp.configure(ov, mb)
            random.setstate(st0)
            for _ in range(2):
                train_step(model, opt, batch, 0, crit, cosine, guard=False)
            barrier()
            t_ab = time.perf_counter()
            for _ in range(6):
                train_step(model, opt, batch, 0, crit, cosine, guard=False)
            barrier()
            t_ab = torch.tensor([(time.perf_counter() - t_ab) / 6], dtype=torch.float64, device=dev)
            if world > 1:
                torch.distributed.all_reduce(t_ab, op=torch.distributed.ReduceOp.MAX)
            ddp_ab[name] = {"ms_per_step": round(1e3 * float(t_ab.item()), 3), "buckets": len(dp.reducer.buckets)}
        best = min(ddp_ab, key=lambda k: ddp_ab[k]["ms_per_step"])
        dp.configure(*settings[best])
        random.setstate(st0)
        for _ in range(2):
            train_step(model, opt, batch, 0, crit, cosine, guard=False)
        random.setstate(st0)
        ddp_ab = {"settings": ddp_ab, "used_for_timed_region": best, "steps_each": 6}
    # A plain run times the steps alone.  --full adds HIP event pairs around the ~80 matrix launches of every timed step (<= 0.15 ms per step:
    # measured in round 4, profiles/; its `value` includes them), per-step events and the draws of each step.
    full = args.full
    prof = None
    if full:
        prof = types_ns(results=lambda: {"brick16_conv_kernel": (1, 1.0, 1.0)}) if dry else \
            _lib.EventProfiler({"pcrl_conv3d_k3_fwd", "pcrl_conv3d_k3_fwd_ws", "pcrl_conv3d_k3_dgrad_bnred", "pcrl_conv3d_k3_wgrad", "pcrl_upconv_fwd", "pcrl_upconv_dgrad",
                                "pcrl_upconv_dgrad_ws", "pcrl_upconv_wgrad_accum"}, keyfn)
    import gc
    gc.collect()
    barrier()
    ALG_BYTES.clear()
    L.profiler = prof
    ms0 = torch.cuda.memory_stats(dev) if full and not dry else {}
    step_marks = [Event(enable_timing=True) for _ in range(args.steps + 1)] if full else None
    t0 = time.perf_counter()
    if full:
        step_marks[0].record()
    draw_states = []
    for i in range(args.steps):
        if full and i < 256:     # (diagnostics only; a state is a 625-int tuple: keeping thousands of them made the cyclic GC's full collections pause 100-300 ms each in a 1 500-step run)
            draw_states.append(random.getstate())
        out = train_step(model, opt, batch, 0, crit, cosine, guard=False)
        if full:
            step_marks[i + 1].record()
    barrier()
    elapsed = time.perf_counter() - t0
    L.profiler = None
    ms1 = torch.cuda.memory_stats(dev) if full and not dry else {}
    per_step = [round(step_marks[i].elapsed_time(step_marks[i + 1]), 1) for i in range(args.steps)] if full else []
    # the step's 13 scale draws (train_3d.py:87: global pair, then (view 1, local i), (view 2, local i) for the six local views) decide which
    # stages run a backward: view 2's full-resolution decoder stage (up_tr64, ~3.4 ms of kernels) only if a term with view 2 drew scale 2
    draws, v2_full, loc_full = [], [], []
    for st_ in draw_states:
        r_ = random.Random()
        r_.setstate(st_)
        d_ = [r_.randint(0, 2) for _ in range(1 + 2 * args.nlocal)]
        draws.append("".join(str(v) for v in d_))
        v2_full.append(int(d_[0] == 2 or any(v == 2 for v in d_[2::2])))
        loc_full.append(int(any(v == 2 for v in d_[1:])))
    loss = float(out[0])
    t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
    if world > 1:
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
    elapsed = float(t.item())
    if args.dump_outputs and rank == 0:      # before anything below runs more steps on the same model
        dump_outputs(args.dump_outputs, out, model)

    # The step runs on three streams (config.py: the second global view on its own stream, weight gradients and the decoder's side branches on
    # a side stream), so the per-launch times above are times of kernels SHARING the chip -- two convolutions side by side each see about half
    # of it.  A few extra steps on one stream (after the timed region, on every rank) give the dominant kernel's time with the chip to itself:
    # the roofline figure (the one-stream rocprofv3 summary agrees with it), never `value`; the timed region's share stays in roofline.in_timed_region.
    from pcrlv2_amd import config as _cfg
    alone = None
    if dry:
        args.no_alone = args.no_secondary = args.no_cpu_baseline = True
    if full and _cfg.WGRAD_SIDE_STREAM_3D and not args.no_alone:      # every rank runs them (the optimizer step holds a collective)
        _cfg.WGRAD_SIDE_STREAM_3D = False     # also turns the second view's stream off (it needs the side stream)
        _branch, _cfg.FWD_BRANCH_STREAM = _cfg.FWD_BRANCH_STREAM, False
        for _ in range(2):
            train_step(model, opt, batch, 0, crit, cosine, guard=False)
        alone = _lib.EventProfiler({"pcrl_conv3d_k3_fwd", "pcrl_conv3d_k3_fwd_ws", "pcrl_conv3d_k3_dgrad_bnred", "pcrl_conv3d_k3_wgrad", "pcrl_upconv_fwd", "pcrl_upconv_dgrad", "pcrl_upconv_dgrad_ws",
                                    "pcrl_upconv_wgrad_accum"}, keyfn)   # every matrix kernel: roofline.weighted_matrix_frac
        ALG_BYTES.clear()
        torch.cuda.synchronize()
        L.profiler = alone
        for _ in range(min(10, args.steps)):
            train_step(model, opt, batch, 0, crit, cosine, guard=False)
        torch.cuda.synchronize()
        L.profiler = None
        _cfg.WGRAD_SIDE_STREAM_3D, _cfg.FWD_BRANCH_STREAM = True, _branch
    alg_bytes = dict(ALG_BYTES)       # of the launches `roofline.launches` counts (the secondary configurations below classify their own launches too)

    # BASELINE config C4 (128x128x64 crops, b = 8: the large-crop stress case) on the same model, after everything that feeds `value` and
    # `roofline`: 2 warm-up + 5 timed steps (~0.5 s), reported as `secondary` -- never part of `value`.
    secondary = None
    if full and world == 1 and not args.no_secondary and dhw == (64, 64, 32) and args.b == 32 and args.dtype == "bf16" and args.nlocal == 6:
        try:
            c4 = synthetic_batch(8, (128, 128, 64), 16, dev, 4321)
            for _ in range(2):
                train_step(model, opt, c4, 0, crit, cosine, guard=False)
            torch.cuda.synchronize()
            t_c4 = time.perf_counter()
            for _ in range(5):
                train_step(model, opt, c4, 0, crit, cosine, guard=False)
            torch.cuda.synchronize()
            t_c4 = (time.perf_counter() - t_c4) / 5
            secondary = {"C4": {"workload": "C4: 128x128x64 global views x2 + 6 local 16^3, b=8/GPU, fwd+bwd+SGD (5 timed steps after 2 warm-up)",
                                "value": round(8 / t_c4, 2), "unit": "crops/s", "ms_per_step": round(1e3 * t_c4, 3),
                                "step_mfma_frac": round(9.42e12 * 8 / t_c4 / 1e12 / PEAK_BF16_TFLOPS, 4)}}
            if _cfg.WGRAD_SIDE_STREAM_3D and not args.no_alone:
                # the dominant kernel of the large-crop configuration alone on the chip: 3 one-stream steps under HIP events
                _cfg.WGRAD_SIDE_STREAM_3D = False
                _b4, _cfg.FWD_BRANCH_STREAM = _cfg.FWD_BRANCH_STREAM, False
                try:
                    train_step(model, opt, c4, 0, crit, cosine, guard=False)
                    p4 = _lib.EventProfiler({"pcrl_conv3d_k3_fwd", "pcrl_conv3d_k3_fwd_ws", "pcrl_upconv_fwd"}, keyfn)
                    torch.cuda.synchronize()
                    L.profiler = p4
                    for _ in range(3):
                        train_step(model, opt, c4, 0, crit, cosine, guard=False)
                    torch.cuda.synchronize()
                    L.profiler = None
                    r4 = {k: v for k, v in p4.results().items() if k.startswith(("igemm", "brick"))}
                    d4 = max(r4, key=lambda k: r4[k][1])
                    n4, ms4, w4 = r4[d4]
                    secondary["C4"]["roofline"] = {"bound": "mfma", "kernel": d4, "achieved": round(w4 / (ms4 * 1e-3) / 1e12, 1), "peak": PEAK_BF16_TFLOPS,
                                                   "unit": "TFLOP/s", "frac": round(w4 / (ms4 * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4),
                                                   "avg_launch_ms": round(ms4 / n4, 4), "launches": n4, "ms_per_step": round(ms4 / 3, 3),
                                                   "measured": "HIP events over 3 one-stream steps", "traffic": None}
                    try:        # HBM bytes per launch of the same kernel in the C4 step: profiles/LATEST_PMC_C4.txt names the committed PMC summary
                        l4 = os.path.join(ROOT, "profiles", "LATEST_PMC_C4.txt")
                        if os.path.exists(l4):
                            n4f = open(l4).read().strip()
                            j4 = json.load(open(os.path.join(ROOT, "profiles", n4f)))
                            if d4 in j4:
                                secondary["C4"]["roofline"]["traffic"] = round(j4[d4]["hbm_bytes_per_launch"])
                                secondary["C4"]["roofline"]["traffic_source"] = "profiles/" + n4f
                    except Exception:
                        pass
                finally:
                    L.profiler = None
                    _cfg.WGRAD_SIDE_STREAM_3D, _cfg.FWD_BRANCH_STREAM = True, _b4
            del c4
        except Exception as e:      # the secondary figure must never cost the primary line
            secondary = {"C4": {"error": repr(e)[:200]}}
        # BASELINE config C5's per-GPU workload (2D ResNet-18 U-Net, 512x512, b = 64; SURVEY 8f N1 -- parity unpinned): 2 warm-up +
        # 3 timed steps of train_2d.train_step on synthetic batches (tools/bench_2d.py is the stand-alone form), so that the driver's record
        # holds the 2D path's rate as well.  Never part of `value`.
        try:
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            from bench_2d import c5_report, conv_flops_fwd
            from pcrlv2_amd import train_2d
            from pcrlv2_amd.models import PCRLv2
            m2 = PCRLv2().to(dev).set_compute_dtype("bf16")
            o2 = FusedSGD(m2.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
            g2 = torch.Generator(device=dev).manual_seed(1234)
            kw2 = dict(generator=g2, device=dev)
            b2, sz = 64, 512
            x1 = torch.randn(b2, 3, sz, sz, **kw2)
            batch2 = (x1, x1 + 0.1 * torch.randn(b2, 3, sz, sz, **kw2), torch.rand(b2, 3, sz, sz, **kw2), None,
                      [torch.randn(b2, 3, 96, 96, **kw2) for _ in range(6)])
            crit2 = train_2d.MSELoss2d()
            t_c5, rep2, _ = c5_report(m2, o2, batch2, crit2, cosine, train_2d, steps=4, warmup=3)
            flop2 = 3 * b2 * (2 * conv_flops_fwd(sz) + 6 * conv_flops_fwd(96))
            secondary["C5_2d"] = {"workload": "C5 per-GPU: PCRLv2 ResNet-18 U-Net, 512x512 x2 + 6 local 96x96, b=64, fwd+bwd+SGD (4 timed steps after 3 warm-up; 2D parity unpinned)",
                                  "value": round(b2 / t_c5, 2), "unit": "crops/s", "ms_per_step": round(1e3 * t_c5, 3),
                                  "step_mfma_frac": round(flop2 / t_c5 / 1e12 / PEAK_BF16_TFLOPS, 4), **rep2,
                                  "note": "the 2D step is HBM-bound (hbm_total: every operand tensor of every launch once, against 8 TB/s); `roofline` is its "
                                          "dominant MATRIX kernel alone on the chip; PMC traffic of the same kernels: profiles/LATEST_PMC_2D.txt"}
            try:
                latest2 = os.path.join(ROOT, "profiles", "LATEST_PMC_2D.txt")
                if os.path.exists(latest2):
                    d2 = json.load(open(os.path.join(ROOT, "profiles", open(latest2).read().strip())))
                    k2 = secondary["C5_2d"].get("roofline", {}).get("kernel", "").split("<")[0]
                    if k2 in d2:
                        secondary["C5_2d"]["roofline"]["traffic"] = round(d2[k2]["hbm_bytes_per_launch"])
                        secondary["C5_2d"]["roofline"]["traffic_source"] = "profiles/" + open(latest2).read().strip()
            except Exception:
                pass
            del m2, o2, batch2, x1
        except Exception as e:
            secondary["C5_2d"] = {"error": repr(e)[:200]}

    if rank != 0:
        return
    crops = world * args.b * args.steps / elapsed
    # BASELINE configs: C2 = 64x64x32 b=32 (the metric), C4 = 128x128x64 b=8 (9.42 TFLOP per crop); anything else is labelled as such
    cfg_name = {((64, 64, 32), 32): "C2", ((128, 128, 64), 8): "C4"}.get((dhw, args.b), "custom (not a BASELINE config)")
    if args.nlocal != 6:
        cfg_name = "custom (not a BASELINE config: %d local views)" % args.nlocal
    if dry:
        cfg_name = "DRY RUN on CPU (PCRL_BENCH_DRYRUN=1: stub step with known gradients; `value` is NOT a measurement)"
    flop_per_crop = {"C2": FLOP_PER_CROP, "C4": 9.42e12}.get(cfg_name)
    line = {
        "metric": "3D crops/sec (64x64x32, b=32) pretrain step" if cfg_name == "C2" else f"3D crops/sec ({dhw[0]}x{dhw[1]}x{dhw[2]}, b={args.b}) pretrain step", "value": round(crops, 2), "unit": "crops/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
        "config": {"workload": f"{cfg_name}: PCRLv23d pre-train step, {dhw[0]}x{dhw[1]}x{dhw[2]} global views x2 + 6 local 16^3, "
                               f"b={args.b}/GPU, fwd+bwd+SGD", "global_batch": world * args.b, "parallelism": f"dp{world}"},
        "step_mfma_frac": round(flop_per_crop * args.b * args.steps / elapsed / 1e12 / PEAK_BF16_TFLOPS, 4) if flop_per_crop else None,
        "final_loss": round(loss, 5),
    }
    if full:
        res = prof.results()
        detail = {}
        for k, (n, ms, work) in sorted(res.items()):
            detail[k] = {"launches": n, "avg_ms": round(ms / n, 4), "tflops": round(work / (ms * 1e-3) / 1e12, 1)}
        exec_flop = sum(v[2] for v in prof.results().values())     # rank 0's convolution launches in the timed region (per GPU, like step_mfma_frac)
        conv = {k: v for k, v in res.items() if k.startswith(("igemm", "brick"))}   # forward / data-gradient convolution kernels
        dom = max(conv, key=lambda k: conv[k][1])
        n, ms, work = conv[dom]
        achieved = work / (ms * 1e-3) / 1e12
        # HBM bytes per launch of the dominant kernel from the PMC passes (FETCH_SIZE x2 + WRITE_SIZE, collected separately
        # with rocprofv3 --pmc and summarised by tools/summarize_profiles.py); null if no summary for this kernel is committed.
        traffic, traffic_src = None, None
        try:
            import glob
            # profiles/LATEST_PMC.txt names the summary that belongs to the current kernels; older ones stay as the record of the round
            latest = os.path.join(ROOT, "profiles", "LATEST_PMC.txt")
            names = [os.path.join(ROOT, "profiles", open(latest).read().strip())] if os.path.exists(latest) else sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc.json")))
            for f in names:
                d = json.load(open(f))
                if dom in d:
                    traffic, traffic_src = round(d[dom]["hbm_bytes_per_launch"]), os.path.relpath(f, ROOT)
        except Exception:
            pass
        line.update({
            "roofline": {"bound": "mfma", "kernel": dom, "achieved": round(achieved, 1), "peak": PEAK_BF16_TFLOPS if args.dtype == "bf16" else 157.3,
                         "unit": "TFLOP/s", "frac": round(achieved / (PEAK_BF16_TFLOPS if args.dtype == "bf16" else 157.3), 4),
                         "avg_launch_ms": round(ms / n, 4), "launches": n, "traffic": traffic, "traffic_unit": "HBM bytes per launch (PMC)",
                         "traffic_source": traffic_src, "algorithmic_flops_per_launch": round(work / n)},
            "executed_mfma_tflop_per_step": round(exec_flop / args.steps / 1e12, 2) if exec_flop else None,
            "step_mfma_frac_executed": round(exec_flop / elapsed / 1e12 / PEAK_BF16_TFLOPS, 4) if exec_flop else None,
            "mfma_note": "step_mfma_frac prices the REFERENCE's convolution FLOPs (40.66 TFLOP per C2 step) against the dense bf16 peak; the engine executes fewer "
                         "(the composed ConvTranspose3d -> Conv3d operator runs 8 of 27 taps): step_mfma_frac_executed is what the matrix pipes actually did",
            "kernels": detail, "kernels_note": "per-launch times inside the timed region, where kernels of three streams share the chip",
            "diag": {"gpu_ms_per_step": per_step, "gpu_ms_per_step_max_minus_min": round(max(per_step) - min(per_step), 1),
                     "draws_per_step": draws, "view2_full_res_backward": v2_full, "local_full_res_backward": loc_full,
                     "draws_note": "13 scale draws per step (0/1/2 = 256/128/64-channel scale): global pair, then (view 1, local i), (view 2, local i); "
                                   "a step whose draws leave view 2 without a scale-2 term skips that view's up_tr64 backward -- the spread of gpu_ms_per_step is workload, not jitter",
                     "device_mallocs_in_timed_region": ms1.get("num_device_alloc", 0) - ms0.get("num_device_alloc", 0),
                     "alloc_retries": ms1.get("num_alloc_retries", 0) - ms0.get("num_alloc_retries", 0),
                     "reserved_GB": round(ms1.get("reserved_bytes.all.peak", 0) / 2**30, 1)},
        })
        if alone is not None and dom in alone.results():
            # The roofline figure of the dominant kernel is its rate with the chip to itself (the one-stream steps): reproducible, and what the
            # one-stream rocprofv3 summary under profiles/ shows (244.3 vs 244.8 us per launch on one box).  Its per-launch time inside the
            # three-stream timed region is kept beside it: there it shares the chip, and how much depends on how the streams happen to line up
            # (the overlapped rocprofv3 run, whose instrumentation slows the launches, saw 376 us where the timed region saw 471).
            n1, ms1_, work1 = alone.results()[dom]
            a1 = work1 / (ms1_ * 1e-3) / 1e12
            rf = line["roofline"]
            rf["in_timed_region"] = {"achieved": rf["achieved"], "frac": rf["frac"], "avg_launch_ms": rf["avg_launch_ms"], "launches": rf["launches"],
                                     "note": "three streams share the chip (second view; weight gradients + side branches): the kernel's share, not its rate"}
            # every matrix kernel of the one-stream steps, weighted by its time: executed FLOPs / summed kernel time / peak (the dominant
            # kernel's `frac` alone flatters the step: the composed, weight-gradient and small-grid kernels run below it)
            mk = alone.results()
            mk_ms, mk_work = sum(v[1] for v in mk.values()), sum(v[2] for v in mk.values())
            if mk_ms > 0:
                nst = min(10, args.steps)
                rf["weighted_matrix_frac"] = round(mk_work / (mk_ms * 1e-3) / 1e12 / rf["peak"], 4)
                rf["weighted_matrix"] = {"executed_tflop_per_step": round(mk_work / nst / 1e12, 2), "kernel_ms_per_step": round(mk_ms / nst, 3),
                                         "kernels": {k: {"ms_per_step": round(v[1] / nst, 3), "tflops": round(v[2] / (v[1] * 1e-3) / 1e12, 1)} for k, v in sorted(mk.items())},
                                         "note": "all convolution / composed up-conv forward, data-gradient and weight-gradient launches (with their second passes) of the "
                                                 "one-stream steps: executed FLOPs / summed HIP-event time / dense bf16 peak"}
            # the FAMILY next to the dominant instantiation: every brick16_conv_kernel* row -- plain, <dgrad+bn_reduce>, the composed
            # <upconv_fwd> / <upconv_dgrad> -- so that a re-keying of the instantiations cannot move the headline fraction
            fam = {k: v for k, v in mk.items() if k.startswith("brick16_conv_kernel")}
            if fam:
                f_ms, f_work = sum(v[1] for v in fam.values()), sum(v[2] for v in fam.values())
                rf["family"] = {"kernels": sorted(fam), "achieved": round(f_work / (f_ms * 1e-3) / 1e12, 1), "frac": round(f_work / (f_ms * 1e-3) / 1e12 / rf["peak"], 4),
                                "ms_per_step": round(f_ms / min(10, args.steps), 3), "launches_per_step": round(sum(v[0] for v in fam.values()) / min(10, args.steps), 1),
                                "note": "all instantiations of the wide-brick convolution kernel in the one-stream steps: executed FLOPs / summed HIP-event time / peak"}
                plain = {k: v for k, v in fam.items() if "upconv" not in k}
                if plain:
                    p_ms, p_work = sum(v[1] for v in plain.values()), sum(v[2] for v in plain.values())
                    rf["family"]["frac_3x3x3_only"] = round(p_work / (p_ms * 1e-3) / 1e12 / rf["peak"], 4)
            rf["power_note"] = ("the matrix kernels run at the board's 1 400 W cap (rocm-smi 1 390-1 397 W, shader clock 1.90-1.94 GHz of 2.4 nominal while they loop: "
                                "profiles/r06_wgrad_trace.txt section 11); `peak` is the nominal-clock figure")
            rf.update({"achieved": round(a1, 1), "frac": round(a1 / rf["peak"], 4), "avg_launch_ms": round(ms1_ / n1, 4), "launches": n1,
                       "measured": "HIP events over %d one-stream steps run right after the timed region (same process, model and batch; "
                                   "PCRL_WGRAD_STREAM=0 PCRL_BRANCH_STREAM=0 PCRL_VIEW_STREAMS=0 semantics)" % min(10, args.steps)})
        else:
            line["roofline"]["measured"] = "HIP events over the timed region"
        if alg_bytes.get(dom) and line["roofline"]["launches"]:
            ab = alg_bytes[dom] / line["roofline"]["launches"]
            line["roofline"]["algorithmic_bytes_per_launch"] = round(ab)
            if line["roofline"]["traffic"]:
                line["roofline"]["traffic_over_algorithmic"] = round(line["roofline"]["traffic"] / ab, 3)
    if dry:
        line["dry_run"] = {"gradient_checks_passed": opt.checked, "note": "every optimizer step of every rank checked the all-reduced arena against the known sums"}
    if secondary is not None:
        line["secondary"] = secondary
    if dist_info is not None:
        if ddp_ab is not None:
            dist_info["ab"] = ddp_ab
        line["distributed"] = dist_info
        line["per_gpu_value"] = round(crops / world, 2)
    if full and dist_info is not None:
        # relative to the committed one-GPU record of the same code, if there is one (efficiency proper needs a one-GPU run of the same build)
        try:
            one = json.load(open(os.path.join(ROOT, "profiles", "LATEST_BENCH.json")))
            if one.get("n_gpus") == 1 and one.get("config", {}).get("workload") == line["config"]["workload"]:
                line["scaling_vs_committed_1gpu"] = round(crops / one["value"], 3)
        except Exception:
            pass
    if full and world == 1 and not args.no_cpu_baseline:
        line["cpu_baseline"] = cpu_baseline()
    try:        # RCCL's version banner sits in the C stdio buffer of a redirected stdout and would land BEHIND the JSON line at exit: flush it first
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
