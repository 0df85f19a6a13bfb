"""What the three training loops (train_3d, train_2d, train_finetune) share: the process-group lifecycle, the start-up order, the epochs with
their checkpoints and held-out validation, one epoch's meters and log line, the bracket around one optimisation step, and the skeleton of a
held-out pass.  The loops hand over what differs -- a `Task` -- and keep their losses, metrics, model choice and checkpoint layout.

Common to all three, and said here once: one process per GPU with an RCCL all-reduce (`pcrlv2_amd.ddp`) where the reference has nn.DataParallel,
`--b` per process; `--amp` selects bfloat16 activations / MFMA operands with float32 accumulation, statistics and master weights (no loss
scaling); `--seed` seeds python's `random` and torch; meters hold device scalars that are read only when a log line is printed, so a step
never synchronises the GPU; `--resume` is applied BEFORE the data-parallel wrapper is built, whose initial broadcast then carries rank 0's
resumed state to every rank."""
from __future__ import print_function

import dataclasses
import os
import random
import sys
import time
from typing import Callable

import torch
import torch.distributed as dist

from . import config as _cfg
from . import ddp as _ddp
from . import functions as _fn
from . import ops as _ops
from . import optim_cli as _optim_cli
from .utils import AverageMeter, adjust_learning_rate


def seed_everything(seed):
    random.seed(seed)
    torch.manual_seed(seed)


def to_gpu(t):
    return t.float().cuda(non_blocking=True)


# ---- one optimisation step --------------------------------------------------------------------------------------------------------
def run_step(model, optimizer, forward, key, before_update=None):
    """The bracket around one step: per-step engine state reset (ops pass counter; gradients parked by a backward that raised -- clean even after
    a skipped or failed step), at most config.MAX_STEPS_AHEAD steps of host run-ahead, `forward()` -> a tuple whose first entry is the loss,
    zero_grad, backward, optimizer step, and -- on the first complete step of this `key` -- the allocator's per-stream pools sized for the
    steady state (ops.provision_allocator).  `before_update(loss)` runs between forward and zero_grad; a true result abandons the step there.
    -> forward's tuple, or None for an abandoned step."""
    _ops.begin_step()
    _fn.reset_parked()
    dev = next(model.parameters()).device
    _ops.throttle_host(dev)
    with _ops.trace_range("forward"):
        out = forward()
    if before_update is not None and before_update(out[0]):
        return None
    optimizer.zero_grad()
    with _ops.trace_range("backward"):
        out[0].backward(gradient=_fn.root_gradient(out[0]))
    with _ops.trace_range("optimizer"):
        optimizer.step()
    _ops.throttle_host(dev, step_done=True)
    _ops.provision_allocator(dev, key=key)
    return out


# ---- one epoch --------------------------------------------------------------------------------------------------------------------
def _print_skips(flags, verbose):
    if flags and verbose:
        for _ in range(int(torch.cat(flags).sum().item())):
            print('skip the step')
    del flags[:]


def run_epoch(epoch, loader, model, step, logged, verbose=True):
    """One epoch: `step(batch)` per batch, meters, a log line every tenth iteration (the only point at which the GPU is synchronised).
    `logged`: (label, index into step's result) per metered loss, in the log line's order; they are masked and metered in the result's order.  A step that returns None (abandoned on the host) is not
    metered; one whose result has a `.skipped` device flag (train_3d.StepLosses: the update was skipped ON THE DEVICE) must not enter the meters
    either -- its weight is n * (1 - skipped), a device scalar, AND its values are masked to 0 (a diverged loss is often inf / NaN: inf * 0 would
    poison the running sums); its 'skip the step' line is printed when the flags are read, with the log line.  -> {label: mean}"""
    model.train()
    bt, dt = AverageMeter(), AverageMeter()
    meters = [(label, i, AverageMeter()) for label, i in logged]
    by_index = sorted(meters, key=lambda t: t[1])
    skipped_flags = []
    tick = time.time()
    for it, batch in enumerate(loader, start=1):
        dt.update(time.time() - tick)
        out = step(batch)
        if out is None:
            continue
        n = batch[0].size(0)
        skipped = getattr(out, "skipped", None)
        vals = [out[i] for _, i, _ in by_index]
        if skipped is not None:
            live = 1.0 - skipped.reshape(())
            n = n * live
            vals = [torch.where(live > 0, v, torch.zeros_like(v)) for v in vals]
            skipped_flags.append(skipped)
        for (_, _, m), v in zip(by_index, vals):
            m.update(v, n)
        log_now = it % 10 == 0
        if log_now:
            torch.cuda.synchronize()
            _print_skips(skipped_flags, verbose)
        bt.update(time.time() - tick)
        tick = time.time()
        if log_now and verbose:
            print('Train: [{0}][{1}/{2}]\tBT {3:.3f} ({4:.3f})\tDT {5:.3f} ({6:.3f})\t'.format(epoch, it, len(loader), bt.val, bt.avg, dt.val, dt.avg)
                  + '\t'.join('{0} {1:.3f} ({2:.3f})'.format(label, float(m.val), float(m.avg)) for label, _, m in meters))
            sys.stdout.flush()
    _print_skips(skipped_flags, verbose)       # steps skipped after the last log line of the epoch
    return {label: float(m.avg) for label, _, m in meters}


# ---- one held-out pass ------------------------------------------------------------------------------------------------------------
def val_shard(loader, group):
    """The batches this rank evaluates.  A loader that was built for this rank (luna_pretask_loaders: a contiguous shard of the validation
    files per rank; anything with `sharded = True`) is taken whole; a loader with `shard(rank, world)` is asked; a plain sequence of batches
    is cut into contiguous runs."""
    world = dist.get_world_size(group) if group is not None or (dist.is_available() and dist.is_initialized()) else 1
    if world <= 1 or getattr(loader, "sharded", False):
        return loader
    rank = dist.get_rank(group)
    if hasattr(loader, "shard"):
        return loader.shard(rank, world)
    if isinstance(loader, (list, tuple)):
        n = len(loader)
        return loader[rank * n // world:(rank + 1) * n // world]
    raise TypeError("validate: with a process group the loader must be sharded per rank (`sharded = True`), offer shard(rank, world), or be a sequence of batches")


def held_out_pass(loader, group, acc, per_batch, also_read=None):
    """The skeleton of a pass over held-out data: the loader's augmentation draws are reset to its seed (`reset_rng()`: every pass sees the same
    data, two passes on the same weights give bit-identical numbers); `per_batch(batch)` under no_grad for this rank's batches, accumulating into
    the device tensor `acc`; `also_read()` -> a float64 device vector that is read back in front of `acc`; ONE all_reduce of `acc` when
    the group has more than one rank, and ONE host synchronisation and read-back.  -> the read-back as a list."""
    if hasattr(loader, "reset_rng"):
        loader.reset_rng()
    distributed = dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
    with torch.no_grad():
        for batch in (val_shard(loader, group) if distributed else loader):
            per_batch(batch)
    front = also_read() if also_read is not None else None
    if distributed:
        dist.all_reduce(acc, group=group)
    return (acc if front is None else torch.cat([front, acc])).cpu().tolist()          # the pass's one synchronisation


# ---- one run ----------------------------------------------------------------------------------------------------------------------
def run_with_group(body):
    """`body(distributed)` with the process group's lifecycle around it.  A group this call creates (inside `body`, by run_epochs) is this call's
    to take down (ddp.shutdown: barrier + destroy_process_group, also when an exception propagates): nn.DataParallel needs no teardown, one
    process per GPU does -- ranks that return with the group alive abort now and then.  A group that stood before is left standing."""
    distributed = int(os.environ.get("WORLD_SIZE", "1")) > 1
    owns_group = distributed and not (dist.is_available() and dist.is_initialized())
    ok = False
    try:
        out = body(distributed)
        ok = True
        return out
    finally:
        if owns_group:
            _ddp.shutdown(ok)


CHECKPOINT_KEYS = ('opt', 'state_dict', 'optimizer', 'epoch')       # the reference's layout (train_3d.py:71-82)


@dataclasses.dataclass
class Task:
    """What differs between the loops (DESIGN.md section 5 has the table).  The callables are looked up by the task's module when they run."""
    make_model: Callable         # (rank) -> the model; run_epochs calls .cuda() on it
    make_optimizer: Callable     # (params, lr=, momentum=, weight_decay=[, kind=, betas=, eps=, max_grad_norm=])
    resume: Callable             # (path, model, optimizer, rank) -> the stored epoch
    resumed: str                 # rank 0's line after that: .format(path, first epoch)
    state_dict: Callable         # (model) -> what a checkpoint holds under 'state_dict'
    epoch: Callable              # (epoch, loader, model, optimizer, verbose)
    validate: Callable           # (model, loader, epoch) -> dict
    val_text: Callable           # (val) -> the text after 'Val: [e]\t'
    better: Callable             # (val, best val so far | None) -> whether --save_best writes `val`'s checkpoint
    best_keys: tuple = CHECKPOINT_KEYS + ('val',)
    val_every_0_is_1: bool = False       # --val_every 0: never (the reference), or every epoch
    save_last: bool = False              # the last epoch is checkpointed too


def checkpoint_name(args, tag):
    return os.path.join(args.output, "{}_{}_{}_{}_{}.pt".format(args.model, args.n, args.phase, args.ratio, tag))


def run_epochs(args, loaders, task, distributed):
    """-> (model, the last epoch that ran | None, whether this rank prints)"""
    rank = 0
    if distributed:
        rank, _, local_rank = _ddp.init_process_group_from_env()
        torch.cuda.set_device(local_rank)
    seed_everything(getattr(args, "seed", 42))
    chatty = rank == 0
    model = task.make_model(rank).cuda()
    if getattr(args, "amp", False):
        model.set_compute_dtype(torch.bfloat16)
    optimizer = task.make_optimizer(model.parameters(), lr=args.lr, momentum=args.momentum, weight_decay=args.weight_decay,
                                    **_optim_cli.options(args))      # --optimizer / --betas / --eps / --clip_grad; nothing more for plain SGD
    first_epoch = 0
    if getattr(args, "resume", None):       # BEFORE the data-parallel wrapper is built (module docstring)
        first_epoch = task.resume(args.resume, model, optimizer, rank) + 1
        if chatty:
            print(task.resumed.format(args.resume, first_epoch))
    if distributed:
        _ddp.DataParallel(model, optimizer)          # hooks itself into optimizer.step()
    val_every = int(getattr(args, "val_every", 0) or 0) or int(task.val_every_0_is_1)

    def checkpoint(keys, tag, epoch, val=None):
        parts = {'opt': lambda: args, 'state_dict': lambda: task.state_dict(model), 'optimizer': optimizer.state_dict, 'epoch': lambda: epoch,
                 'val': lambda: dict(val)}
        torch.save({k: parts[k]() for k in keys}, checkpoint_name(args, tag))

    train, best, last_epoch = loaders['train'], None, None
    for epoch in range(first_epoch, args.epochs + 1):          # inclusive upper bound, like the reference (Q1): lr reaches 0 in the last epoch
        adjust_learning_rate(epoch, args, optimizer)
        if hasattr(train, 'set_epoch'):
            train.set_epoch(epoch)       # a resumed run continues the sequence of per-epoch draws
        if chatty:
            print("==> training...")
        t_start = time.time()
        task.epoch(epoch, train, model, optimizer, chatty)
        last_epoch = epoch
        if chatty:
            print('epoch {}, total time {:.2f}'.format(epoch, time.time() - t_start))
            if epoch % 100 == 0 or epoch == 240 or (task.save_last and epoch == args.epochs):     # checkpoint cadence and layout of train_3d.py:71-82
                print('==> Saving...')
                checkpoint(CHECKPOINT_KEYS, epoch, epoch)
        if val_every > 0 and (epoch + 1) % val_every == 0:      # --val_every N: held-out metrics after every N-th epoch
            val = task.validate(model, loaders['eval'], epoch)
            if chatty:
                print('Val: [{0}]\t{1}'.format(epoch, task.val_text(val)))
                sys.stdout.flush()
                if getattr(args, "save_best", False) and task.better(val, best):
                    checkpoint(task.best_keys, "best", epoch, val)
                    best = val
        if _cfg.EMPTY_CACHE_PER_EPOCH:           # the reference's per-epoch empty_cache (train_3d.py:83 / train_2d.py:108); the steady-state pools are kept (ops.empty_cache)
            torch.cuda.empty_cache() if _cfg.EMPTY_CACHE_RAW else _ops.empty_cache()
    return model, last_epoch, chatty
