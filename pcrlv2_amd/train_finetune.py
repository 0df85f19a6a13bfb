"""Supervised 2D fine-tuning on the MI355X engine: `--d 2 --phase finetune | scratch` -- the downstream use of the 2D encoder the reference's README
describes ("Load the Encoder Part of a 2D Model": smp.Unet('resnet18', aux_params=dict(pooling='avg', dropout=0.2, activation='sigmoid',
classes=n_class)) with the pre-trained encoder) on the 14-label chest X-ray lists it ships and whose labels its pre-task throws away.

The reference has no fine-tuning loop for this model (its fine-tune branch is not public).  What is pinned: the model (models.ChestClassifier = the
README's recipe), the data split (`--ratio`: first part for pre-training, LAST 1 - ratio here), the training transform (the pre-task's un-jittered
view) and the optimiser / schedule of its 2D pre-training (SGD, cosine).  This project's own choices: multi-label BCE as the loss, mean per-class
AUROC as the metric (the ChestX-ray14 convention), the evaluation transform Resize((224, 224)).

The run, the epoch and the bracket around a step are pcrlv2_amd.loop's; validation is ONE pass of ChestClassifier.infer with the probabilities and labels kept on the device, one
exact AUROC launch (csrc/auroc.hip) and one host read-back.
"""
from __future__ import print_function

import os
import sys

import torch
import torch.distributed as dist

from . import loop as _loop
from . import ops2d as _ops2d
from .loop import to_gpu
from .models.pcrlv2_model import ChestClassifier
from . import optim as _optim
from .optim import FusedSGD


def train_step(model, optimizer, batch):
    """One optimisation step on (x [B,3,H,W] float32, y [B,K] uint8) -- or the 3D classifier's [B,1,X,Y,Z] cubes.  -> (loss, probabilities), detached.
    `model.provision_key` (train_classifier sets it) names the workload in the allocator's provisioning table."""
    def forward():
        x = to_gpu(batch[0])
        return model.loss(x, batch[1].to(x.device))

    loss, probs = _loop.run_step(model, optimizer, forward, (getattr(model, "provision_key", "2d-finetune"), tuple(batch[0].shape)))
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
    K = model.n_class
    ps, ys = [], []
    acc = torch.zeros(2, dtype=torch.float64, device=dev)       # sum of batch-size-weighted losses, rows

    def per_batch(batch):
        x, y = to_gpu(batch[0]), batch[1].to(dev)
        probs, loss = model.infer(x, labels=y)
        ps.append(probs)
        ys.append(y)
        acc.add_(torch.stack([loss.double() * x.shape[0], torch.tensor(float(x.shape[0]), dtype=torch.float64, device=dev)]))

    def counts():       # every rank's rows (gather_scores) -> the AUROC's counts (< 2^53: exact in float64), read back in front of `acc`
        probs = torch.cat(ps) if ps else torch.zeros((0, K), dtype=torch.float32, device=dev)
        labels = torch.cat(ys) if ys else torch.zeros((0, K), dtype=torch.uint8, device=dev)
        probs, labels = gather_scores(probs, labels, group)
        return _ops2d.auroc_counts(probs, labels).double().reshape(-1) if probs.shape[0] else acc.new_zeros(3 * K)

    host = _loop.held_out_pass(loader, group, acc, per_batch, also_read=counts)
    n = host[-1]
    if not n:
        nan = float("nan")
        return {"loss": nan, "auroc": [nan] * K, "mean_auroc": nan, "n": 0}
    per, mean = _ops2d.auroc_from_counts([[int(v) for v in host[3 * k:3 * k + 3]] for k in range(K)])
    return {"loss": host[-2] / n, "auroc": per.tolist(), "mean_auroc": mean, "n": int(round(n))}


def higher_auroc(val, best):
    """--save_best: the mean validation AUROC improves strictly; NaN is never best."""
    m = val["mean_auroc"]
    return m == m and (best is None or m > best["mean_auroc"])


def resume_classifier(path, model, optimizer, rank):
    """`--resume`: the whole classifier, and the momentum buffers when the checkpoint has them.  -> the stored epoch"""
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    model.load_state_dict(ckpt["state_dict"])
    if "optimizer" in ckpt:
        _optim.restore(optimizer, ckpt)       # a checkpoint of another optimiser kind ends the run with a message
    return int(ckpt.get("epoch", -1))


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
    return _loop.run_with_group(lambda distributed: _train_classifier(args, loaders, make_model, key, distributed))


def _train_classifier(args, loaders, make_model, key, distributed):
    def make(rank):
        model = make_model().cuda()         # on the device here: the dropout masks' generator lives there
        model.provision_key = key
        dev = next(model.parameters()).device
        model.mask_generator = torch.Generator(device=dev).manual_seed(int(getattr(args, "seed", 42)) + 104729 * (rank + 1))
        return model

    task = _loop.Task(
        make_model=make,
        make_optimizer=lambda params, **k: _optim.for_task(FusedSGD, params, **k),
        resume=resume_classifier,
        resumed="==> resumed the classifier from {}; continuing with epoch {}",
        state_dict=lambda model: model.state_dict(),
        epoch=lambda epoch, loader, model, optimizer, verbose: train_inner(args, epoch, loader, model, optimizer, verbose=verbose),
        validate=lambda model, loader, epoch: evaluate(model, loader),
        val_text=_fmt, better=higher_auroc, best_keys=('epoch', 'state_dict', 'val'),
        val_every_0_is_1=True,       # this phase validates: 0 means every epoch
        save_last=True)              # train_2d's naming and rhythm, plus the last epoch
    model, last_epoch, chatty = _loop.run_epochs(args, loaders, task, distributed)
    # the final test: the best model by validation AUROC when one was kept, otherwise the last epoch's -- every rank loads the same file
    if last_epoch is not None:
        if distributed:
            dist.barrier()
        best_file = _loop.checkpoint_name(args, "best")
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
    return _loop.run_epoch(epoch, train_loader, model, lambda batch: train_step(model, optimizer, batch), (("bce loss", 0),), verbose)["bce loss"]
