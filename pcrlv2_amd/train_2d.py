"""2D pre-training loop on the MI355X engine -- drop-in for the reference's train_2d.py  (SURVEY 8f N1).

Same entry point `train_pcrlv2(args, data_loader, out_channel=3)`, `cos_loss`, loss assembly (five scales, no divergence guard,
train_2d.py:139-171), LR schedule, log line and checkpoint (the ENCODER's state_dict only, train_2d.py:99).  The run, the epoch and the
bracket around a step are pcrlv2_amd.loop's, which also lists the deliberate differences.  `--encoder_weights FILE` initialises the encoder from a local torchvision-named ResNet-18 state_dict (the
reference downloads ImageNet weights at construction, pcrlv2_model.py:200; offline the default is random init, with a warning).
`--resume CKPT` continues from a checkpoint of the reference's 2D layout: that layout holds the ENCODER only (train_2d.py:99), so
the encoder, the epoch counter and -- when the shapes match -- the momentum buffers are restored, the decoder and heads restart.
"""
from __future__ import print_function

import math
import os
import random

import torch

from . import functions as _fn
from . import loop as _loop
from . import ops as _ops
from . import ops2d as _ops2d
from .functions2d import MaskMSEFn, SegMSEFn, mse_loss2d
from .loop import to_gpu
from .models.pcrlv2_model import PCRLv2
from . import optim as _optim
from .optim import FusedSGD
from .train_3d import BETA_PERIOD, COS_MAX_TERMS, LOGGED, CosineSimilarityMean, cos_loss, fused_cos_losses  # noqa: F401  (cos_loss: train_2d.py:111-117)
from .train_3d import lower_total, mean_scales, val_beta, val_text


class MSELoss2d:
    """`criterion` of train_2d.py:78 on NHWC-memory predictions."""

    def cuda(self):
        return self

    def __call__(self, pred, target):
        return mse_loss2d(pred, target)


FUSED_STEP_2D = os.environ.get("PCRL_FUSED_STEP_2D", "1") != "0"     # A/B switch: 0 = the round-3 step (one launch per cosine mean, every map computed)


def step_losses(model, batch, epoch, criterion, cosine):
    """Forward half of one iteration (train_2d.py:139-168).  -> (total, restoration, global-cosine, deep-supervision, local-cosine)

    Engine form (our PCRLv2, our criterion / cosine objects): the 13 scale draws are taken from python's `random` FIRST -- the same 13
    `randint(0, 4)` calls in the same order as the reference's cos_loss calls (global pair; then for every local view (view 1, local_i),
    (view 2, local_i)); nothing in between consumes `random` -- so that the forwards know which deep-supervision map the step reads
    (masks1[scale of the first draw]) and skip the stateless work nobody reads (PCRLv2.forward_engine); all 26 cosine means in one launch,
    the local views concatenated in one launch, both restoration terms against the NCHW image without a layout copy, the total in one."""
    view1, view2, target, _unused_gt2, local_views = batch
    n = view1.size(0)
    target = to_gpu(target)
    view1, view2 = to_gpu(view1), to_gpu(view2)
    nl = len(local_views)
    fused = (FUSED_STEP_2D and isinstance(model, PCRLv2) and isinstance(criterion, MSELoss2d) and getattr(cosine, "fusable", False)
             and 2 + 4 * nl <= COS_MAX_TERMS)
    _ops.fork_views(view1.device, path2d=True)     # config.VIEW_STREAMS_2D: the second view's forward (and backward) on its own stream
    if fused:
        ns = len(model.model.decoder.blocks)
        draws = [random.randint(0, ns - 1) for _ in range(1 + 2 * nl)]
        scale = draws[0]
        feats1, h1, low1 = model.forward_engine(view1, mask_scale=scale)
        with _ops.view_pass(view2.device, view2, path2d=True):
            feats2, _, _ = model.forward_engine(view2)
        loc = _ops.concat_batch([to_gpu(v) for v in local_views])
        feats_loc, _, _ = model.forward_engine(loc)
        _ops.join_side_stream()                    # the cosine terms read both views' features on the main stream
        cos2, _ = fused_cos_losses(feats1, feats2, feats_loc, n, nl, draws=draws)
        seg = model.model.segmentation_head[0]
        l_restore = SegMSEFn.apply(h1, seg.weight, seg.bias, target, model._seg)
        l_deep_raw = MaskMSEFn.apply(low1, target, 2 ** (ns - 1 - scale))
        beta = 0.5 * (1.0 + math.cos(math.pi * epoch / BETA_PERIOD))
        total, l_deep, l_global, l_local = _fn.loss_tail(l_restore, cos2, l_deep_raw, beta)
        return total, l_restore, l_global, l_deep, l_local
    feats1, mask1, masks1 = model(view1)
    with _ops.view_pass(view2.device, view2, path2d=True):
        feats2, _mask2, _ = model(view2)
    _ops.join_side_stream()                        # the cosine term below reads both views' features on the main stream
    l_global, scale = cos_loss(cosine, feats1, feats2)
    feats_loc, _, _ = model(torch.cat([to_gpu(v) for v in local_views], dim=0), local=True)
    return assemble_losses(feats1, feats2, feats_loc, mask1, masks1, target, n, len(local_views), epoch, criterion, cosine, first=(l_global, scale))


def assemble_losses(feats1, feats2, feats_loc, mask1, masks1, target, n, nlocal, epoch, criterion, cosine, first=None):
    """train_2d.py:139-168 from the three forwards' outputs on: the global cosine term (its scale draw also picks the deep-supervision map), the
    2 * nlocal local terms in the reference's order -- (view 1, local_i), (view 2, local_i) for every local view i --, the restoration term,
    beta * the deep-supervision term, the sum.  Pure torch on whatever device the tensors live on: pinned on the CPU against the reference's own
    `cos_loss` and a restatement of its loop body (tests/golden/loss2d_*.npz, oracle/make_golden.py --loss2d).
    `first`: the (global term, scale) pair when the caller has already drawn it (step_losses draws it before the local views' forward, as the
    reference does).  -> (total, restoration, global-cosine, deep-supervision, local-cosine)"""
    l_global, scale = first if first is not None else cos_loss(cosine, feats1, feats2)
    stacked = [torch.stack(pair) for pair in feats_loc]                 # [2, 6n, C] per scale
    l_local = 0.0
    for i in range(nlocal):
        crop_i = [s[:, n * i: n * (i + 1)] for s in stacked]
        l_local = l_local + cos_loss(cosine, feats1, crop_i)[0]
        l_local = l_local + cos_loss(cosine, feats2, crop_i)[0]
    l_local = l_local / (2 * nlocal)
    l_restore = criterion(mask1, target)
    beta = 0.5 * (1.0 + math.cos(math.pi * epoch / BETA_PERIOD))
    l_deep = beta * criterion(masks1[scale], target)
    return l_restore + l_global + l_local + l_deep, l_restore, l_global, l_deep, l_local


def train_step(model, optimizer, batch, epoch, criterion, cosine):
    losses = _loop.run_step(model, optimizer, lambda: step_losses(model, batch, epoch, criterion, cosine), ("2d", tuple(batch[0].shape), len(batch[4])))
    return tuple(l.detach() for l in losses)


NUM_SCALES = 5
VAL_KEYS = (("mse_out",) + tuple("mse_mid%d" % k for k in range(NUM_SCALES)) + tuple("cos_global%d" % k for k in range(NUM_SCALES))
            + tuple("cos_local%d" % k for k in range(NUM_SCALES)))


def val_total(m, epoch):
    """The expectation of the training loss (train_2d.py:139-168) over its uniform scale draws, from the sixteen per-scale means."""
    mean = lambda name: mean_scales(m, name, NUM_SCALES)        # noqa: E731
    return m["mse_out"] + mean("cos_global") + mean("cos_local") + val_beta(epoch) * mean("mse_mid")


def validate(model, loader, epoch, group=None):
    """One pass over held-out data (the reference ships train_val_txt/chest_valid.txt and never reads it: data.py:59 hands the training loader out
    as 'eval'): the terms of the training loss in eval mode at EVERY one of the five scale indices -- so no random number is drawn and the total is
    the expectation of train_2d.py:139-168 over its draws, comparable to the training log.  Per batch: PCRLv2.infer on view 1 (maps at their own
    resolution), on view 2 and on the concatenated local views (features only), then pcrl_val2d_metrics into a device accumulator; ONE host
    synchronisation and read-back at the end (after ONE all_reduce of the seventeen sums when there is a process group of more than one rank).  The
    loader's augmentation draws are reset to its seed first (`reset_rng()`): every pass sees the same data, two passes on the same weights give
    bit-identical numbers.  `model.training` is not changed.
    -> {'mse_out', 'mse_mid0..4', 'cos_global0..4', 'cos_local0..4', 'total', 'n'}; sample-weighted means (a ragged last batch counts by its size)."""
    acc = torch.zeros(len(VAL_KEYS) + 1, dtype=torch.float64, device=next(model.parameters()).device)

    def per_batch(batch):
        view1, view2, target, _gt2, local_views = batch
        view1, view2, target = to_gpu(view1), to_gpu(view2), to_gpu(target)
        feats1, out1, masks1 = model.infer(view1, upsample=False)
        feats2, _, _ = model.infer(view2, features_only=True)
        loc = _ops.concat_batch([to_gpu(v) for v in local_views])
        feats_loc, _, _ = model.infer(loc, local=True, features_only=True)
        _ops2d.val2d_metrics(out1, masks1, target, feats1, feats2, feats_loc, acc)

    host = _loop.held_out_pass(loader, group, acc, per_batch)
    n = host[-1]
    out = {k: (v / n if n else float("nan")) for k, v in zip(VAL_KEYS, host)}
    out["total"] = val_total(out, epoch)
    out["n"] = int(round(n))
    return out


def resume_encoder(path, model, optimizer, rank):
    """`--resume`: the 2D checkpoint layout holds the ENCODER only (train_2d.py:99).  -> the stored epoch"""
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    model.model.encoder.load_state_dict(ckpt["state_dict"])
    try:
        _optim.restore(optimizer, ckpt)       # a checkpoint of another optimiser kind ends the run with a message
    except (ValueError, KeyError) as e:       # a checkpoint of another parameter list (group / size mismatch): keep fresh momentum, say so on EVERY rank
        print("==> [rank {}] optimizer state not restored: {}".format(rank, e))
    return int(ckpt.get("epoch", -1))


def encoder_state(model):
    """What a 2D checkpoint holds under 'state_dict' (train_2d.py:96-107: the ENCODER's weights only)."""
    model.flush_counters()
    return model.model.encoder.state_dict()


def train_pcrlv2(args, data_loader, out_channel=3):
    return _loop.run_with_group(lambda distributed: _train_pcrlv2(args, data_loader, distributed))


def _train_pcrlv2(args, data_loader, distributed):
    criterion, cosine = MSELoss2d().cuda(), CosineSimilarityMean().cuda()       # stateless, like train_3d's: free of device, seed and group

    def make_model(rank):
        enc_w = getattr(args, "encoder_weights", None) or None
        if enc_w is None and rank == 0:
            print("==> warning: encoder starts from RANDOM weights (no --encoder_weights); the reference starts from ImageNet ResNet-18")
        return PCRLv2(encoder_weights=enc_w)

    task = _loop.Task(
        make_model=make_model,
        make_optimizer=lambda *a, **k: FusedSGD(*a, **k),
        resume=resume_encoder,
        resumed="==> resumed the ENCODER from {} (the 2D checkpoint layout holds nothing else); continuing with epoch {}",
        state_dict=encoder_state,
        epoch=lambda epoch, loader, model, optimizer, verbose: train_pcrlv2_inner(args, epoch, loader, model, optimizer, criterion, cosine, verbose=verbose),
        validate=lambda model, loader, epoch: validate(model, loader, epoch),
        val_text=lambda val: val_text(val, NUM_SCALES), better=lower_total)
    return _loop.run_epochs(args, data_loader, task, distributed)[0]


def train_pcrlv2_inner(args, epoch, train_loader, model, optimizer, criterion, cosine, verbose=True):
    """One epoch (train_2d.py:120-195).  Returns (mean cosine loss, mean restoration loss, mean local loss)."""
    avg = _loop.run_epoch(epoch, train_loader, model, lambda batch: train_step(model, optimizer, batch, epoch, criterion, cosine), LOGGED, verbose)
    return avg["cos_loss"], avg["mg loss"], avg["local loss"]
