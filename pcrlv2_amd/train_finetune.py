"""Supervised 2D fine-tuning on the MI355X engine: `--d 2 --phase finetune | scratch` -- the downstream use of the 2D encoder the reference's README
describes ("Load the Encoder Part of a 2D Model": smp.Unet('resnet18', aux_params=dict(pooling='avg', dropout=0.2, activation='sigmoid',
classes=n_class)) with the pre-trained encoder) on the 14-label chest X-ray lists it ships and whose labels its pre-task throws away.

The reference has no fine-tuning loop for this model (its fine-tune branch is not public).  What is pinned: the model (models.ChestClassifier = the
README's recipe), the data split (`--ratio`: first part for pre-training, LAST 1 - ratio here), the training transform (the pre-task's un-jittered
view) and the optimiser / schedule of its 2D pre-training (SGD, cosine).  This project's own choices: multi-label BCE as the loss, mean per-class
AUROC as the metric (the ChestX-ray14 convention), the evaluation transform Resize((224, 224)).

A step follows train_2d.train_step; validation is ONE pass of ChestClassifier.infer with the probabilities and labels kept on the device, one
exact AUROC launch (csrc/auroc.hip) and one host read-back.
"""
from __future__ import print_function

import os
import sys
import time

import torch
import torch.distributed as dist

from . import config as _cfg
from . import ddp as _ddp
from . import functions as _fn
from . import ops as _ops
from . import ops2d as _ops2d
from .models.pcrlv2_model import ChestClassifier
from .optim import FusedSGD
from .train_3d import _to_gpu, _val_shard, seed_everything
from .utils import AverageMeter, adjust_learning_rate


def train_step(model, optimizer, batch):
    """One optimisation step on (x [B,3,H,W] float32, y [B,K] uint8) -- or the 3D classifier's [B,1,X,Y,Z] cubes.  -> (loss, probabilities), detached.
    `model.provision_key` (train_classifier sets it) names the workload in the allocator's provisioning table."""
    _ops.begin_step()
    _fn.reset_parked()
    dev = next(model.parameters()).device
    _ops.throttle_host(dev)
    x, y = _to_gpu(batch[0]), batch[1].to(dev)
    loss, probs = model.loss(x, y)
    optimizer.zero_grad()
    loss.backward(gradient=_fn.root_gradient(loss))
    optimizer.step()
    _ops.throttle_host(dev, step_done=True)
    _ops.provision_allocator(dev, key=(getattr(model, "provision_key", "2d-finetune"), tuple(x.shape)))
    return loss.detach(), probs.detach()


def gather_scores(probs, labels, group=None):
    """All-gather of uneven per-rank shards: probs float32 [m_r, K] and labels uint8 [m_r, K] of every rank r -> ([sum m_r, K], [sum m_r, K]) in rank
    order, the same on every rank.  The shards are padded to the longest one and travel with their true lengths.  Without a process group of more
    than one rank: the inputs."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) <= 1:
        return probs, labels
    world = dist.get_world_size(group)
    m, K = probs.shape
    lens = [torch.zeros(1, dtype=torch.int64, device=probs.device) for _ in range(world)]
    dist.all_gather(lens, torch.tensor([m], dtype=torch.int64, device=probs.device), group=group)
    lens = [int(v) for v in torch.cat(lens).tolist()]
    cap = max(lens)
    # one padded float32 buffer per rank: K score columns, then K label columns (0 / 1 are exact in float32)
    mine = torch.zeros((cap, 2 * K), dtype=torch.float32, device=probs.device)
    mine[:m, :K] = probs
    mine[:m, K:] = labels
    parts = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(parts, mine, group=group)
    full = torch.cat([p[:n] for p, n in zip(parts, lens)], dim=0)
    return full[:, :K].contiguous(), full[:, K:].to(torch.uint8).contiguous()


def evaluate(model, loader, group=None):
    """One pass of `model.infer` over `loader` ((x, y uint8 [B,K]) batches; this rank's shard when there is a process group): the probabilities, the labels
    and the batch-weighted loss sum stay on the device until the end; then (more than one rank: gather_scores + one all-reduce of the loss sums) ONE
    AUROC launch over all rows and ONE host read-back.  `model.training` is not changed; nothing of the model is touched.
    -> {'loss', 'auroc': [K] (NaN for a class without positives or without negatives), 'mean_auroc' (over the other classes), 'n'}"""
    dev = next(model.parameters()).device
    if hasattr(loader, "reset_rng"):
        loader.reset_rng()
    distributed = dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
    K = model.n_class
    ps, ys = [], []
    acc = torch.zeros(2, dtype=torch.float64, device=dev)       # sum of batch-size-weighted losses, rows
    with torch.no_grad():
        for batch in (_val_shard(loader, group) if distributed else loader):
            x, y = _to_gpu(batch[0]), batch[1].to(dev)
            probs, loss = model.infer(x, labels=y)
            ps.append(probs)
            ys.append(y)
            acc += torch.stack([loss.double() * x.shape[0], torch.tensor(float(x.shape[0]), dtype=torch.float64, device=dev)])
    probs = torch.cat(ps) if ps else torch.zeros((0, K), dtype=torch.float32, device=dev)
    labels = torch.cat(ys) if ys else torch.zeros((0, K), dtype=torch.uint8, device=dev)
    if distributed:
        probs, labels = gather_scores(probs, labels, group)
        dist.all_reduce(acc, group=group)
    if probs.shape[0] == 0:
        nan = float("nan")
        return {"loss": nan, "auroc": [nan] * K, "mean_auroc": nan, "n": 0}
    counts = _ops2d.auroc_counts(probs, labels)
    host = torch.cat([counts.double().reshape(-1), acc]).cpu().tolist()          # the pass's one synchronisation (counts < 2^53: exact in float64)
    per, mean = _ops2d.auroc_from_counts([[int(v) for v in host[3 * k:3 * k + 3]] for k in range(K)])
    n = host[-1]
    return {"loss": host[-2] / n, "auroc": per.tolist(), "mean_auroc": mean, "n": int(round(n))}


def _checkpoint_name(args, tag):
    return os.path.join(args.output, "{}_{}_{}_{}_{}.pt".format(args.model, args.n, args.phase, args.ratio, tag))


def save_if_best(args, model, epoch, val, best):
    """--save_best: {'epoch', 'state_dict' (the whole classifier), 'val'} whenever the mean validation AUROC improves strictly.  -> the best so far."""
    m = val["mean_auroc"]
    if m != m or (best is not None and not m > best):
        return best
    torch.save({'epoch': epoch, 'state_dict': model.state_dict(), 'val': dict(val)}, _checkpoint_name(args, "best"))
    return m


def _fmt(val):
    return 'loss {0:.4f}\tmean AUROC {1:.4f}\t({2} samples)'.format(val["loss"], val["mean_auroc"], val["n"])


def train_chest_classifier(args, loaders):
    def make_model():
        enc_w = getattr(args, "encoder_weights", None) or None
        if args.phase == "finetune" and enc_w is None:
            raise SystemExit("--phase finetune needs --encoder_weights (a 2D pre-training checkpoint or a ResNet-18 state_dict); to train the classifier from "
                             "random weights use --phase scratch")
        return ChestClassifier(n_class=int(getattr(args, "n_class", 14)), dropout=float(getattr(args, "dropout", 0.2)),
                               encoder_weights=enc_w if args.phase == "finetune" else None)

    return train_classifier(args, loaders, make_model, "2d-finetune")


def train_classifier(args, loaders, make_model, key):
    """The supervised loop for any model with ChestClassifier's interface (.loss(x, y), .infer(x, labels=), .n_class, .set_compute_dtype,
    .mask_generator): `make_model()` builds it on the host once the process group stands and the seeds are set; `key` names the workload for the
    allocator's provisioning.  -> the trained model (`.test_metrics`: the final test's)."""
    distributed = int(os.environ.get("WORLD_SIZE", "1")) > 1
    owns_group = distributed and not (dist.is_available() and dist.is_initialized())
    ok = False
    try:
        model = _train_classifier(args, loaders, make_model, key, distributed)
        ok = True
        return model
    finally:
        if owns_group:
            _ddp.shutdown(ok)


def _train_classifier(args, loaders, make_model, key, distributed):
    rank = 0
    if distributed:
        rank, _, local_rank = _ddp.init_process_group_from_env()
        torch.cuda.set_device(local_rank)
    seed_everything(getattr(args, "seed", 42))
    chatty = rank == 0
    model = make_model().cuda()
    model.provision_key = key
    dev = next(model.parameters()).device
    model.mask_generator = torch.Generator(device=dev).manual_seed(int(getattr(args, "seed", 42)) + 104729 * (rank + 1))
    if getattr(args, "amp", False):
        model.set_compute_dtype(torch.bfloat16)
    optimizer = FusedSGD(model.parameters(), lr=args.lr, momentum=args.momentum, weight_decay=args.weight_decay)
    first_epoch = 0
    if getattr(args, "resume", None):
        # BEFORE the data-parallel wrapper is built: its initial broadcast carries the resumed state from rank 0 to every rank
        ckpt = torch.load(args.resume, map_location="cpu", weights_only=False)
        model.load_state_dict(ckpt["state_dict"])
        if "optimizer" in ckpt:
            optimizer.load_state_dict(ckpt["optimizer"])
        first_epoch = int(ckpt.get("epoch", -1)) + 1
        if chatty:
            print("==> resumed the classifier from {}; continuing with epoch {}".format(args.resume, first_epoch))
    if distributed:
        _ddp.DataParallel(model, optimizer)
    val_every = int(getattr(args, "val_every", 0) or 0) or 1        # this phase validates: 0 means every epoch
    best, last_epoch = None, None
    for epoch in range(first_epoch, args.epochs + 1):
        adjust_learning_rate(epoch, args, optimizer)
        if hasattr(loaders['train'], 'set_epoch'):
            loaders['train'].set_epoch(epoch)       # a resumed run continues the sequence of per-epoch draws
        if chatty:
            print("==> training...")
        t_start = time.time()
        train_inner(args, epoch, loaders['train'], model, optimizer, verbose=chatty)
        last_epoch = epoch
        if chatty:
            print('epoch {}, total time {:.2f}'.format(epoch, time.time() - t_start))
            if epoch % 100 == 0 or epoch == 240 or epoch == args.epochs:     # train_2d's naming and rhythm, plus the last epoch
                print('==> Saving...')
                torch.save({'opt': args, 'state_dict': model.state_dict(), 'optimizer': optimizer.state_dict(), 'epoch': epoch}, _checkpoint_name(args, epoch))
        if (epoch + 1) % val_every == 0:
            val = evaluate(model, loaders['eval'])
            if chatty:
                print('Val: [{0}]\t{1}'.format(epoch, _fmt(val)))
                sys.stdout.flush()
                if getattr(args, "save_best", False):
                    best = save_if_best(args, model, epoch, val, best)
        if _cfg.EMPTY_CACHE_PER_EPOCH:
            torch.cuda.empty_cache() if _cfg.EMPTY_CACHE_RAW else _ops.empty_cache()
    # the final test: the best model by validation AUROC when one was kept, otherwise the last epoch's -- every rank loads the same file
    if last_epoch is not None:
        if distributed:
            dist.barrier()
        best_file = _checkpoint_name(args, "best")
        which = "last epoch %d" % last_epoch
        if getattr(args, "save_best", False) and os.path.exists(best_file):
            ckpt = torch.load(best_file, map_location="cpu", weights_only=False)
            model.load_state_dict(ckpt["state_dict"])
            which = "best epoch %d" % ckpt["epoch"]
        test = evaluate(model, loaders['test'])
        if chatty:
            print('Test: ({0})\t{1}\tper class {2}'.format(which, _fmt(test), " ".join("%.4f" % a for a in test["auroc"])))
            sys.stdout.flush()
        model.test_metrics = test
    return model


def train_inner(args, epoch, train_loader, model, optimizer, verbose=True):
    """One epoch.  -> mean training loss"""
    model.train()
    meters = {k: AverageMeter() for k in ("bt", "dt", "loss")}
    tick = time.time()
    for it, batch in enumerate(train_loader, start=1):
        meters["dt"].update(time.time() - tick)
        loss, _ = train_step(model, optimizer, batch)
        meters["loss"].update(loss, batch[0].size(0))
        log_now = it % 10 == 0
        if log_now:
            torch.cuda.synchronize()
        meters["bt"].update(time.time() - tick)
        tick = time.time()
        if log_now and verbose:
            m = meters
            print('Train: [{0}][{1}/{2}]\t'
                  'BT {3:.3f} ({4:.3f})\t'
                  'DT {5:.3f} ({6:.3f})\t'
                  'bce loss {7:.3f} ({8:.3f})'.format(epoch, it, len(train_loader), m["bt"].val, m["bt"].avg, m["dt"].val, m["dt"].avg,
                                                      float(m["loss"].val), float(m["loss"].avg)))
            sys.stdout.flush()
    return float(meters["loss"].avg)
