"""3D pre-training loop on the MI355X engine -- drop-in for the reference's train_3d.py.

Same entry point `train_pcrlv2_3d(args, data_loader, out_channel=3)`, same `cos_loss(cosine, output1, output2)`, same loss
assembly, LR schedule, log line, checkpoint dict and file name.  The run, the epoch and the bracket around a step are pcrlv2_amd.loop's,
shared with the 2D and the supervised loop; this module holds the 3D losses, metrics and checkpoint layout.  Differences, all deliberate:

  * compute: PCRLv23d, the losses and SGD run on hand-written gfx950 kernels (pcrlv2_amd.models / functions / optim);
  * `--amp` (apex O1 fp16 in the reference, train_3d.py:52-53), `nn.DataParallel` (train_3d.py:54), the meters (the reference calls .item()
    twice and cuda.synchronize() every iteration): see pcrlv2_amd/loop.py;
  * the divergence guard (train_3d.py:140-142, `loss > 1000 and epoch > 10`) is decided ON THE DEVICE by default: a flag kernel,
    MAX-all-reduced under data parallelism, consumed by the SGD kernel (parameters and momentum stay bit-unchanged when it is set) --
    epochs 11..240 run without the forward -> backward host synchronisation the reference's `if loss > 1000` implies.  A skipped
    step still runs its backward (wasted work on a rare event) and its `.grad`s are this step's instead of the previous step's
    (nobody reads them: the next step starts with zero_grad); meters and the "skip the step" line are settled when the log line is
    printed.  PCRL_GUARD_SYNC=1 (or train_step(guard="sync")) restores the reference's host-side decision: the step returns None
    before zero_grad / backward / step;
  * `--seed` is ignored by the reference; here it also decides the scale draws;
  * `--resume CKPT` (not in the reference, which only saves): restores model, momentum buffers and epoch from a checkpoint of
    the layout above -- written by this engine or by the reference -- and continues with the next epoch.
"""
from __future__ import print_function

import math
import os
import random

import torch
import torch.distributed as dist

from . import ddp as _ddp
from . import functions as _fn
from . import loop as _loop
from . import ops as _ops
from .functions import cosine_mean, mse_loss
from .loop import seed_everything, to_gpu  # noqa: F401  (seed_everything: tools import it from here)
from .models import PCRLv23d
from .optim import FusedSGD

BETA_PERIOD = 240   # train_3d.py:136 hard-codes 240 (not args.epochs) in the deep-supervision weight; reproduced (Q2)


class MSELoss:
    """`criterion` of train_3d.py:56: mean squared error on the fused reduction kernel."""

    def cuda(self):
        return self

    def __call__(self, pred, target):
        return mse_loss(pred, target)


LAZY_SKIPS = True            # module attribute (tests / tools/step_ab.py flip it): the encoder stages' unpooled outputs are not stored by the step (PCRLv23d.forward lazy_skips)
SKIP_UNUSED_OUTPUTS = True   # module attribute, flipped by the bit-identity test (no environment switch since round 6)
COS_MAX_TERMS = 32   # csrc/heads_loss.hip
FUSED_COS_LOSSES = os.environ.get("PCRL_FUSED_COS", "1") != "0"   # all 26 cosine means of a step in one launch (0: one launch per mean)


class CosineSimilarityMean:
    """train_3d.py:57's nn.CosineSimilarity(), fused with the `.mean()` that every call site applies to it.  `fusable`: the training
    step may hand all of its cosine terms to one kernel launch instead of calling this object 26 times (same arithmetic)."""
    returns_mean = True
    fusable = True

    def cuda(self):
        return self

    def __call__(self, a, b):
        return cosine_mean(a, b)


def cos_loss(cosine, output1, output2):
    """Symmetric negative cosine similarity between predictor and (stop-gradient) projection on ONE scale drawn from
    python's global `random` -- train_3d.py:86-92.  output*[k] = [projection, prediction] of scale k."""
    k = random.randint(0, len(output1) - 1)
    (pro_a, pre_a), (pro_b, pre_b) = output1[k], output2[k]
    sim_ab, sim_ba = cosine(pre_a, pro_b.detach()), cosine(pre_b, pro_a.detach())
    if not getattr(cosine, "returns_mean", False):      # a plain nn.CosineSimilarity was passed in
        sim_ab, sim_ba = sim_ab.mean(), sim_ba.mean()
    return -(sim_ab + sim_ba) * 0.5, k


def fused_cos_losses(feats1, feats2, feats_loc, n, nlocal, draws=None):
    """The 13 cos_loss calls of train_3d.py:119-134 as ONE launch: the scales are drawn from python's `random` in the reference's
    order (global pair; then for every local view (view 1, local_i), (view 2, local_i)), the 26 cosine means and their weights
    (-1/2 per call; /(2 * nlocal) for the local group) go to pcrl_cosine_terms_*.  -> ([global term, local term] as one float32[2], first drawn
    scale): the pair goes to functions.loss_tail whole (selecting its elements here would cost select_backward's fills and adds)."""
    ns = len(feats1)
    tensors, idx = [], {}
    for name, fs in (("1", feats1), ("2", feats2), ("L", feats_loc)):
        for k in range(ns):
            idx[name, k, 0], idx[name, k, 1] = len(tensors), len(tensors) + 1          # 0 = projection, 1 = prediction
            tensors += [fs[k][0], fs[k][1]]
    spec = []

    def add(a, ra, b, rb, k, w, g):        # -(cos(pre_a, pro_b) + cos(pre_b, pro_a)) / 2 * w   at scale k
        spec.append((idx[a, k, 1], ra, idx[b, k, 0], rb, -0.5 * w, g))
        spec.append((idx[b, k, 1], rb, idx[a, k, 0], ra, -0.5 * w, g))

    # `draws`: the 1 + 2 * nlocal scales already taken from `random` in this order (train_2d.step_losses draws before the forwards)
    nxt = iter(draws).__next__ if draws is not None else (lambda: random.randint(0, ns - 1))
    k0 = nxt()
    add("1", 0, "2", 0, k0, 1.0, 0)
    wl = 1.0 / (2 * nlocal)
    for i in range(nlocal):
        add("1", 0, "L", n * i, nxt(), wl, 1)
        add("2", 0, "L", n * i, nxt(), wl, 1)
    return _fn.cosine_terms(spec, n, 2, tensors), k0


def step_losses(model, batch, epoch, criterion, cosine):
    """Forward half of one iteration (train_3d.py:113-138): three forwards, 13 cosine terms, two restoration terms.
    Returns (total, restoration, global-cosine, deep-supervision, local-cosine) as device scalars."""
    view1, view2, target, _unused_gt2, local_views = batch              # gt2 is never used by the reference either (Q3)
    n = view1.size(0)
    target = to_gpu(target)
    # all cosine means of the step in one launch -- pcrl_cosine_terms_* takes up to 32 terms (2 + 4 per local view: up to 7 local views; the
    # reference's loop accepts any number): beyond that the step falls back to one launch per mean, same arithmetic
    fused = getattr(cosine, "fusable", False) and FUSED_COS_LOSSES and 2 + 4 * len(local_views) <= COS_MAX_TERMS
    view1, view2 = to_gpu(view1), to_gpu(view2)
    _ops.fork_views(view1.device)  # config.VIEW_STREAMS: the second view's forward (and backward) on its own stream, next to the first's
    _ops.prepack(model, view1.device)   # config.PREPACK: this step's packed / composed weight forms on the side stream, ahead of their use
    with _ops.deferred_join():     # the decoder stages' side branches (heads, deep-supervision maps) also run under the NEXT forward; joined on exit
        lz = dict(lazy_skips=True) if LAZY_SKIPS and isinstance(model, PCRLv23d) else {}      # the encoder stages' unpooled outputs have no reader in this step: not stored
        out1, feats1, masks1 = model(view1, **lz)
        # mask2, the local views' reconstruction and their deep-supervision maps are never used (train_3d.py:117,123): the engine's
        # model skips what has no state (out_tr, the trilinear upsampling) when asked for the features only; a plain nn.Module computes them
        fo = dict(features_only=True, **lz) if SKIP_UNUSED_OUTPUTS and isinstance(model, PCRLv23d) else dict(lz)
        with _ops.view_pass(view2.device, view2):
            _out2, feats2, _ = model(view2, **fo)
        if fused:
            loc = _ops.concat_batch([to_gpu(v) for v in local_views])
            chunked = _ddp.chunk_partition_on()       # opt-in: nn.DataParallel's literal scatter of the [6B] local-view tensor (ddp.py)
            if chunked:
                loc = _ddp.chunk_local_inputs(loc, n, len(local_views))
            with _ops.view_pass(loc.device, loc, name="local"):
                _, feats_loc, _ = model(loc, local=True, **fo)
            if chunked:
                _ops.join_side_stream()        # the heads ran on the side stream (config.FWD_BRANCH_STREAM): the exchange reads their outputs on this one
                feats_loc = _ddp.chunk_local_features(feats_loc, n, len(local_views))
    if fused:
        cos2, scale = fused_cos_losses(feats1, feats2, feats_loc, n, len(local_views))
        l_restore = criterion(out1, target)
        beta = 0.5 * (1.0 + math.cos(math.pi * epoch / BETA_PERIOD))
        total, l_deep, l_global, l_local = _fn.loss_tail(l_restore, cos2, criterion(masks1[scale], target), beta)   # one launch: the sum and beta * MSE
        return total, l_restore, l_global, l_deep, l_local
    l_global, scale = cos_loss(cosine, feats1, feats2)
    loc = torch.cat([to_gpu(v) for v in local_views], dim=0)
    if _ddp.chunk_partition_on():
        loc = _ddp.chunk_local_inputs(loc, n, len(local_views))
    _, feats_loc, _ = model(loc, local=True, **fo)
    if _ddp.chunk_partition_on():
        feats_loc = _ddp.chunk_local_features(feats_loc, n, len(local_views))
    stacked = [torch.stack(pair) for pair in feats_loc]                 # [2, 6n, C] per scale
    l_local = 0.0
    for i in range(len(local_views)):
        crop_i = [s[:, n * i: n * (i + 1)] for s in stacked]
        l_local = l_local + cos_loss(cosine, feats1, crop_i)[0]
        l_local = l_local + cos_loss(cosine, feats2, crop_i)[0]
    l_local = l_local / (2 * len(local_views))
    l_restore = criterion(out1, target)
    beta = 0.5 * (1.0 + math.cos(math.pi * epoch / BETA_PERIOD))
    l_deep = beta * criterion(masks1[scale], target)                    # the scale drawn by the FIRST cos_loss call
    return l_restore + l_global + l_deep + l_local, l_restore, l_global, l_deep, l_local


def begin_step():
    """Reset the per-step engine state (ops pass counter; gradients parked by a backward that raised)."""
    _ops.begin_step()
    _fn.reset_parked()


GUARD_THRESHOLD = 1000.0   # train_3d.py:140
GUARD_FIRST_EPOCH = 11     # `epoch > 10`
GUARD_SYNC = os.environ.get("PCRL_GUARD_SYNC", "0") == "1"


class StepLosses(tuple):
    """(loss, loss1, loss2, loss4, local_loss) as detached device scalars, plus `.skipped`: None, or the device flag (float32[1]) of the
    divergence guard -- 1 when the update of this step was skipped on the device."""
    skipped = None


def divergence_flag(loss, group=None, collective=True):
    """float32[1] on loss's device: 1 if loss > 1000 on ANY rank of `group` (the reference is one process with one loss and one decision;
    with one process per GPU the decision must be collective -- a rank that skipped alone would leave its peers waiting in the gradient
    all-reduce).  `collective=False`: this process's own decision (no data-parallel wrapper: nobody to agree with)."""
    flag = torch.empty(1, dtype=torch.float32, device=loss.device)
    if loss.is_cuda:
        _ops.lib().call("pcrl_guard_flag", loss.detach().float().reshape(1), GUARD_THRESHOLD, flag, _ops.stream_handle())
    else:       # host tensors (the gloo tests of the collective form): same predicate
        flag[0] = 1.0 if float(loss) > GUARD_THRESHOLD else 0.0
    if collective and dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(flag, op=dist.ReduceOp.MAX, group=group)
    return flag


def train_step(model, optimizer, batch, epoch, criterion, cosine, guard=True):
    """One iteration of train_3d.py:113-151.  Returns StepLosses (loss, loss1, loss2, loss4, local_loss: detached device scalars).
    Divergence guard (epoch > 10, loss > 1000): by default decided on the device -- the returned `.skipped` flag says whether the SGD
    kernel left the parameters alone; with guard="sync" (PCRL_GUARD_SYNC=1) on the host like the reference -- None is returned before
    zero_grad / backward / step.  guard=False: no guard."""
    flag = None

    def guard_step(loss):
        nonlocal flag
        if guard and epoch >= GUARD_FIRST_EPOCH:
            # the decision is taken by the ranks that share gradients: the data-parallel wrapper's group (a wrapper on a sub-group must not pull
            # ranks outside it into this collective); without a wrapper the process decides alone
            dp = getattr(optimizer, "data_parallel", None)
            flag = divergence_flag(loss, group=getattr(dp, "group", None), collective=dp is not None and getattr(dp, "_active", False))
            if guard == "sync" or GUARD_SYNC:
                if bool(flag):       # device -> host read: the reference's semantics, and its synchronisation
                    print('skip the step')
                    return True
                flag = None
        optimizer.skip_flag = flag

    losses = _loop.run_step(model, optimizer, lambda: step_losses(model, batch, epoch, criterion, cosine),
                            ("3d", tuple(batch[0].shape), len(batch[4])), before_update=guard_step)
    if losses is None:
        return None
    out = StepLosses(l.detach() for l in losses)
    out.skipped = flag
    return out


VAL_KEYS = ("mse_out", "mse_mid0", "mse_mid1", "mse_mid2", "cos_global0", "cos_global1", "cos_global2", "cos_local0", "cos_local1", "cos_local2")


def val_beta(epoch):
    """The deep-supervision weight of train_3d.py:136 (240 hard-coded there, Q2)."""
    return 0.5 * (1.0 + math.cos(math.pi * epoch / BETA_PERIOD))


def mean_scales(m, name, ns=3):
    return sum(m[name + str(k)] for k in range(ns)) / ns


def val_total(m, epoch):
    """The expectation of the training loss (train_3d.py:135-138) over its uniform scale draws, from the ten per-scale means."""
    return m["mse_out"] + mean_scales(m, "cos_global") + mean_scales(m, "cos_local") + val_beta(epoch) * mean_scales(m, "mse_mid")


def val_text(val, ns=3):
    """The `Val:` line of both pre-training loops, after its epoch."""
    return 'total {0:.4f}\tmg {1:.4f}\tcos {2:.4f}\tlocal {3:.4f}\tmid {4:.4f}\t({5} samples)'.format(
        val["total"], val["mse_out"], mean_scales(val, "cos_global", ns), mean_scales(val, "cos_local", ns), mean_scales(val, "mse_mid", ns), val["n"])


def lower_total(val, best):
    """--save_best of both pre-training loops: `total` improves strictly."""
    return best is None or val["total"] < best["total"]


def validate(model, loader, epoch, group=None):
    """One pass over held-out data (the reference builds `dataloader['eval']` over folds 7-9, data.py:63-99, and never reads it): the terms of
    the training loss in eval mode at EVERY scale index -- so no random number is drawn and the total is the expectation of train_3d.py:135-138
    over its draws, comparable to the training log.  Per batch: PCRLv23d.infer on view 1, on view 2 (features only) and on the concatenated local
    views, then pcrl_val_metrics into a device accumulator; ONE host synchronisation and read-back at the end (after ONE all_reduce of the eleven
    sums when there is a process group of more than one rank).  The loader's augmentation generator is reset to its seed first (`reset_rng()`):
    every pass sees the same data, two passes on the same weights give bit-identical numbers.  `model.training` is not changed.
    -> {'mse_out', 'mse_mid0..2', 'cos_global0..2', 'cos_local0..2', 'total', 'n'}; sample-weighted means (a ragged last batch counts by its size)."""
    acc = torch.zeros(len(VAL_KEYS) + 1, dtype=torch.float64, device=next(model.parameters()).device)

    def per_batch(batch):
        view1, view2, target, _gt2, local_views = batch
        view1, view2, target = to_gpu(view1), to_gpu(view2), to_gpu(target)
        out1, feats1, masks1 = model.infer(view1)
        _, feats2, _ = model.infer(view2, features_only=True)
        loc = _ops.concat_batch([to_gpu(v) for v in local_views])
        _, feats_loc, _ = model.infer(loc, local=True, features_only=True)
        _ops.val_metrics(out1, masks1, target, feats1, feats2, feats_loc, acc)

    host = _loop.held_out_pass(loader, group, acc, per_batch)
    n = host[-1]
    out = {k: (v / n if n else float("nan")) for k, v in zip(VAL_KEYS, host)}
    out["total"] = val_total(out, epoch)
    out["n"] = int(round(n))
    return out


def load_checkpoint(path, model, optimizer=None):
    """Load a checkpoint of the layout train_3d.py:71-82 writes ({'opt','state_dict','optimizer','epoch'}); keys saved from a
    DataParallel-wrapped model ('module.' prefix, train_3d.py:54) are accepted.  Returns the stored epoch."""
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    sd = {(k[7:] if k.startswith("module.") else k): v for k, v in ckpt["state_dict"].items()}
    model.load_state_dict(sd)
    if optimizer is not None and ckpt.get("optimizer") is not None:
        optimizer.load_state_dict(ckpt["optimizer"])
    return int(ckpt.get("epoch", -1))


def train_pcrlv2_3d(args, data_loader, out_channel=3):
    return _loop.run_with_group(lambda distributed: _train_pcrlv2_3d(args, data_loader, distributed))


def _train_pcrlv2_3d(args, data_loader, distributed):
    # stateless objects (`.cuda()` returns self): nothing of them depends on the device, the seed or the group that run_epochs sets up after this line
    criterion, cosine = MSELoss().cuda(), CosineSimilarityMean().cuda()
    task = _loop.Task(
        make_model=lambda rank: PCRLv23d(),
        make_optimizer=lambda *a, **k: FusedSGD(*a, **k),
        resume=lambda path, model, optimizer, rank: load_checkpoint(path, model, optimizer),
        resumed="==> resumed from {} (continuing with epoch {})",
        state_dict=lambda model: model.state_dict(),
        epoch=lambda epoch, loader, model, optimizer, verbose: train_pcrlv2_inner(args, epoch, loader, model, optimizer, criterion, cosine, verbose=verbose),
        validate=lambda model, loader, epoch: validate(model, loader, epoch),
        val_text=val_text, better=lower_total)
    return _loop.run_epochs(args, data_loader, task, distributed)[0]


LOGGED = (("cos_loss", 2), ("mg loss", 1), ("local loss", 4))       # the log line of train_3d.py:153-170, in its order: label, index into the step's losses


def train_pcrlv2_inner(args, epoch, train_loader, model, optimizer, criterion, cosine, verbose=True):
    """One epoch (train_3d.py:95-173).  Returns (mean restoration loss, mean local loss)."""
    avg = _loop.run_epoch(epoch, train_loader, model, lambda batch: train_step(model, optimizer, batch, epoch, criterion, cosine), LOGGED, verbose)
    return avg["mg loss"], avg["local loss"]
