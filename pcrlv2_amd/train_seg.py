"""3D segmentation fine-tuning on the MI355X engine: `seg3d.py train | predict` -- the downstream use of the WHOLE pre-trained 3D network, decoder
included (the reference's README, "Load the Encoder Part of a 3D Model", loads all of PCRLv23d; BraTS and LiTS in the paper).

The reference's fine-tune branch is not public.  What is pinned: the model (models.Segmenter3d IS a PCRLv23d(n_class, in_channels): a fine-tuned
checkpoint loads into the reference's class) and the optimiser / schedule of its 3D pre-training (SGD, cosine).  This project's own choices: the loss
wb * BCE + wd * (1 - mean Dice) on overlapping sigmoid regions, mean per-case Dice as the metric, crops and stride-tiled evaluation (data_seg).

With --overlap / --val_overlap > 0 a case is predicted by overlap-blended sliding windows instead (sliding_window: patches cut on the device, the head's
logits kept per case, one blend kernel); at 0, the default, everything below is the tiled path.

The run, the epoch and the bracket around a step are pcrlv2_amd.loop's; validation is ONE pass of Segmenter3d.infer over the tiles with the integer
counts {TP, |pred|, |gt|} per (case, class) and the loss sums kept on the device, one all_reduce of both when there is a process group (cases are
sharded by rank, every rank indexes the global case table) and one host read-back.

`seg3d.py score` (surface_metrics, score) scores stored masks: Dice, HD95, HD and ASSD per case and class, the surfaces, the exact
distance transforms and the order statistics on the device (csrc/surface_dist.hip), one host read-back per case.

`seg3d.py postprocess` and the clean-up options of `predict` (postprocess_mask, postprocess) drop connected components of a mask's
classes on the device (csrc/components.hip): all but the largest, and / or those below a volume.

`seg3d.py train --augment` (augment_batch): the loader hands over source boxes and drawn parameters, and the step's forward
resamples image channels and label bitmask together on the device (csrc/seg_augment.hip), then adds noise and gamma (csrc/augment.hip).  Evaluation,
prediction and the sliding window never see it.

`predict --mirror` / `--weights a.pt,b.pt` and `train --val_mirror` (sliding_window(mirror=, models=)): every patch batch is also
shown mirrored and to every checkpoint, and the un-mirrored logits of all passes are averaged in the sliding window's one per-case buffer
(csrc/seg_head.hip's accumulating logits kernel, csrc/seg_blend.hip's mirrored cutter).  At `none` and one checkpoint nothing changes.

Head kinds: a Segmenter3d(head='softmax') trains and evaluates on label maps through the same loop -- `_held_out` takes the
mean per-case Dice over the classes 1..K-1 (dice_from_counts(first=1); the background is excluded) and the softmax form of loss_from_sums.  The kind is
saved as val['head'] in a _best.pt (softmax only) and is in the `opt` of a last-epoch checkpoint; load_segmenter reads it (checkpoint_head: a checkpoint
without it is a sigmoid one) and check_ensemble refuses mixed kinds.  sliding_window blends a softmax model's logits with ops.seg_mc_blend; `predict` of one leaves head.txt next to its label maps, and
`score` / `postprocess` take them with --labelmap (the classes 1..K-1 in groups of at most 7 through the bitmask machinery) and refuse them without.
"""
from __future__ import print_function

import os
import sys

import numpy as np
import torch
import torch.distributed as dist

from . import data_seg as _data
from . import loop as _loop
from . import ops as _ops
from .loop import to_gpu
from .models import Segmenter3d
from . import optim as _optim
from .optim import FusedSGD
from .seg_prep import lerp


def dice_from_counts(counts, first=0):
    """Host, float64: counts [cases][K][3] = {TP, |pred|, |gt|} (nested lists or a tensor) -> (per-class Dice averaged over the cases [K - first], their
    mean over the classes).  A (case, class) pair with empty prediction AND empty ground truth scores 1; an empty prediction against a non-empty ground
    truth scores 0 by the formula.  No cases: NaN.  `first`: the first class that enters -- 1 for the softmax head, whose class 0 is the background."""
    rows = counts.tolist() if torch.is_tensor(counts) else counts
    if not rows:
        return [], float("nan")
    K = len(rows[0])
    per = []
    for k in range(first, K):
        ds = [1.0 if (r[k][1] + r[k][2]) == 0 else 2.0 * float(r[k][0]) / float(r[k][1] + r[k][2]) for r in rows]
        per.append(sum(ds) / len(ds))
    return per, sum(per) / (K - first)


def loss_from_sums(sums, K, wb=1.0, wd=1.0, head="sigmoid", wc=1.0):
    """Host: the operator's loss from its float64 sums [4 K + 1] ({I, P, G, BCE} per class, then the counted voxels), here over a whole pass.
    head='softmax': {I, P, G, CE} per class; wc * sum CE / Mc + wd * (1 - mean Dice of the classes 1..K-1)."""
    mc = sums[4 * K]
    if head == "softmax":
        ce = sum(sums[4 * k + 3] for k in range(K)) / mc if mc > 0 else 0.0
        dice = sum((2.0 * sums[4 * k] + 1.0) / (sums[4 * k + 1] + sums[4 * k + 2] + 1.0) for k in range(1, K)) / (K - 1)
        return wc * ce + wd * (1.0 - dice)
    bce = sum(sums[4 * k + 3] for k in range(K)) / (mc * K) if mc > 0 else 0.0
    dice = sum((2.0 * sums[4 * k] + 1.0) / (sums[4 * k + 1] + sums[4 * k + 2] + 1.0) for k in range(K)) / K
    return wb * bce + wd * (1.0 - dice)


HEAD_FILE = "head.txt"      # next to the <case>_pred.npy of a softmax model: what tells `score` / `postprocess` that the bytes are class indices


def write_head_kind(out_dir, head):
    """`predict` (and `postprocess --labelmap`) of a softmax model leave DIR/head.txt = 'softmax'; a sigmoid run writes nothing and removes a stale one."""
    path = os.path.join(out_dir, HEAD_FILE)
    if head == "softmax":
        with open(path, "w") as f:
            f.write("softmax\n")
    elif os.path.exists(path):
        os.remove(path)


def refuse_labelmap_prediction(pred_dir, command):
    """A directory of label maps read as bitmasks would be scored or cleaned wrongly without any error: class index 3 is 'regions 0 and 1'."""
    path = os.path.join(pred_dir, HEAD_FILE)
    if os.path.exists(path) and open(path).read().strip() == "softmax":
        raise SystemExit(f"{command}: {pred_dir} holds the label maps of a --head softmax model ({HEAD_FILE} says so): pass --labelmap and --n_class K with "
                         "the background counted")


def higher_dice(val, best):
    """--save_best: the mean validation Dice improves strictly; NaN is never best."""
    m = val["mean_dice"]
    return m == m and (best is None or m > best["mean_dice"])


def is_augmented(batch):
    """A batch of data_seg.CropLoader(aug=...): (source boxes, their labels, the dict of drawn parameters)."""
    return len(batch) == 3 and isinstance(batch[2], dict)


def augment_batch(batch, device=None):
    """The device side of an augmented batch (src [B,C,*extent] float32 / float16, src_lab uint8 [B,*extent], params -- host tensors): upload, ONE
    ops.seg_augment launch for image and labels, then pcrl_aug_noise_gamma over the B * C channels when any noise_std != 0 or gamma != 1 (decided on
    the host tensors; skipped otherwise, so neutral intensity is bit-identical to the resampling alone).  On the current stream.
    -> (x float32 [B,C,*crop], lab uint8 [B,*crop])"""
    src, src_lab, p = batch
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    up = lambda t: t.to(dev, non_blocking=True)      # noqa: E731  (a float16 source stays float16: the kernel reads half)
    x, lab = _ops.seg_augment(up(src), up(src_lab), up(p["inv"]), up(p["gain"]), up(p["bias"]), crop=tuple(int(c) for c in p["crop"]))
    if bool((p["noise_std"] != 0).any()) or bool((p["gamma"] != 1).any()):
        x = _ops.seg_noise_gamma(x, up(p["noise_std"]), up(p["gamma"]), int(p["seed"]))
    return x, lab


def train_step(model, optimizer, batch):
    """One optimisation step on (x [B,C,X,Y,Z] float32, labels uint8 [B,X,Y,Z]), or on an augmented batch (is_augmented), which augment_batch turns
    into that inside the step's forward.  -> (loss, sums), detached."""
    def forward():
        if is_augmented(batch):
            return model.loss(*augment_batch(batch))
        x = to_gpu(batch[0])
        return model.loss(x, batch[1].to(x.device, non_blocking=True))

    loss, sums = _loop.run_step(model, optimizer, forward, ("3d-seg", tuple(batch[0].shape)))
    return loss.detach(), sums.detach()


def _held_out(model, n_cases, steps, group, step_sums):
    """ONE loop.held_out_pass over `steps` (its loader-like object): step_sums(step, counts) runs a step's forward, adds {TP, |pred|, |gt|} into its
    cases' rows of `counts` int64 [cases, K, 3] and returns the step's float64 sums [4 K + 1].  One all_reduce carries sums and counts, one host
    read-back follows.  -> {'loss', 'dice': [K], 'mean_dice', 'cases'}"""
    dev = next(model.parameters()).device
    K = model.n_class
    ns = 4 * K + 1
    counts = torch.zeros((max(n_cases, 1), K, 3), dtype=torch.int64, device=dev)
    acc = torch.zeros(ns + n_cases * K * 3, dtype=torch.float64, device=dev)       # the loss sums, then the counts (< 2^53: exact in float64)

    def per_step(step):
        acc[:ns] += step_sums(step, counts)

    def counts_into_acc():       # runs once after the last step, in front of the all_reduce: ONE collective carries counts and sums
        acc[ns:] = counts[:n_cases].reshape(-1).double()
        return acc.new_zeros(0)

    host = _loop.held_out_pass(steps, group, acc, per_step, also_read=counts_into_acc)
    table = [[[int(v) for v in host[ns + (c * K + k) * 3:ns + (c * K + k) * 3 + 3]] for k in range(K)] for c in range(n_cases)]
    head = getattr(model, "head", "sigmoid")
    per, mean = dice_from_counts(table, first=int(head == "softmax"))
    val = {"loss": loss_from_sums(host[:ns], K, model.wb, model.wd, head, getattr(model, "wc", 1.0)) if n_cases else float("nan"), "dice": per,
           "mean_dice": mean, "cases": n_cases}
    if head != "sigmoid":        # what load_segmenter reads from a _best.pt.  Deliberately NOT written for the sigmoid head: its _best.pt stays
        # byte for byte what it was, and a checkpoint without the entry is a sigmoid one (checkpoint_head)
        val["head"] = head
    return val


def evaluate(model, loader, group=None):
    """One pass of `model.infer` over the tiles of `loader` (data_seg.TileLoader: this rank's cases).  -> {'loss', 'dice': [K], 'mean_dice', 'cases'}"""
    dev = next(model.parameters()).device

    def tile_sums(batch, counts):
        x = batch[0].to(dev, non_blocking=True).float()
        return model.infer(x, labels=batch[1].to(dev), case_index=batch[2].to(dev), counts=counts)[2]

    return _held_out(model, len(loader.cases), loader, group, tile_sums)


def _fmt(val):
    return 'loss {0:.4f}\tmean Dice {1:.4f}\t({2} cases)'.format(val["loss"], val["mean_dice"], val["cases"])


# ---- overlap-blended sliding windows ----------------------------------------------------------------------------------------------
def sliding_window(model, case, crop, b, overlap, window, *, counts=None, row=0, want_mask=True, want_probs=False, max_bytes=16 << 30, mirror=(0,),
                   models=None):
    """One case by overlapping crop-sized windows (data_seg.windows) whose logits are blended with a centre-weighted window (data_seg.blend_weights):
    the image (and the labels, when the case has them) is uploaded once, `b` patches per forward are cut on the device (ops.seg_cut_patches),
    model.infer_logits writes into the per-case buffer [P, *crop, K], and ONE ops.seg_blend call turns it into the prediction; with labels, row `row`
    of `counts` gets {TP, |pred|, |gt|} added.  -> (mask uint8 [X, Y, Z] | None, probs float32 [K, X, Y, Z] | None, sums float64 [4 K + 1]), on the
    device; an unlabelled case without `counts` has nothing to sum: its sums are None and the blend runs without them.  A buffer above `max_bytes` is refused before anything is uploaded.

    Mirror test-time augmentation and checkpoint ensembles.  `mirror`: mirror codes (data_seg.parse_mirror; bit 0 = x, bit 1 = y,
    bit 2 = z); `models`: a list that replaces `model` as the source of logits (`model` stays the source of n_class, wb and wd).  Per batch of patches,
    for each model in list order and each code in ascending order, the patches are cut mirrored (ops.seg_cut_patches(flip=code)) and
    infer_logits(flip=code) adds their logits, un-mirrored, into the SAME slice of the per-case buffer, which keeps its size; the first pass overwrites,
    the last multiplies by float32(1 / (E M)) (E models, M codes).  What the blend then averages is the mean of the LOGITS over the passes (not of the
    probabilities), formed in float32 in pass order: the blend is linear in the logits, so this equals averaging blended logits.  With one model and
    mirror (0,) the calls are exactly those without the two arguments."""
    crop, K, b = tuple(int(c) for c in crop), int(model.n_class), int(b)
    nets = [model] if models is None else list(models)
    codes = sorted({int(c) for c in mirror})
    if not nets or not codes or codes[0] < 0 or codes[-1] > 7:
        raise ValueError(f"sliding_window: mirror codes are integers 0..7 and `models` is not empty, got mirror {tuple(mirror)} and {len(nets)} models")
    if any(getattr(net, "head", "sigmoid") != getattr(model, "head", "sigmoid") for net in nets):
        raise ValueError("sliding_window: every model of `models` must have the head kind of `model`")
    if models is not None and any(int(net.n_class) != K for net in nets):
        raise ValueError(f"sliding_window: every model of `models` must have the {K} classes of `model`, got {[int(net.n_class) for net in nets]}")
    passes = [(net, code) for net in nets for code in codes]
    axes = _data.windows(case.shape, crop, overlap)
    weights = _data.blend_weights(crop, window)
    starts = _data.window_starts(axes)
    P = len(starts)
    nbytes = P * crop[0] * crop[1] * crop[2] * K * 4
    if nbytes > max_bytes:
        raise SystemExit(f"{case.name}: the logits of its {P} patches at overlap {overlap:g} need {nbytes / 2 ** 30:.1f} GiB, above the limit of "
                         f"{max_bytes / 2 ** 30:.1f} GiB for one case: use a smaller --overlap")
    dev = next(nets[0].parameters()).device
    img = torch.from_numpy(np.ascontiguousarray(case.img)).to(dev)
    labels = None if case.seg is None else torch.from_numpy(np.ascontiguousarray(case.seg)).to(dev)
    st = torch.tensor(starts, dtype=torch.int32, device=dev)
    z = torch.empty((P,) + crop + (K,), dtype=torch.float32, device=dev)
    for a in range(0, P, b):
        for i, (net, code) in enumerate(passes):       # one pass of code 0: flip=0, overwrite, scale 1 -- the plain cutter and the plain logits kernel
            last = i == len(passes) - 1
            net.infer_logits(_ops.seg_cut_patches(img, st[a:a + b], crop, flip=code), out=z[a:a + b], flip=code, accumulate=i > 0,
                             scale=np.float32(1.0 / len(passes)) if last else 1.0)
    sd, wdev = [torch.tensor(a, dtype=torch.int32, device=dev) for a in axes], [torch.from_numpy(w).to(dev) for w in weights]
    want_sums = labels is not None or counts is not None
    if getattr(model, "head", "sigmoid") == "softmax":       # only the logits call (inside infer_logits) and the blend call differ between the heads
        mask, probs, sums, _, _ = _ops.seg_mc_blend(z, sd, wdev, case.shape, labels=labels, counts=counts, row=row, want_mask=want_mask,
                                                    want_probs=want_probs, want_sums=want_sums, wc=model.wc, wd=model.wd)
    else:
        mask, probs, sums, _, _ = _ops.seg_blend(z, sd, wdev, case.shape, labels=labels, counts=counts, row=row, want_mask=want_mask, want_probs=want_probs,
                                                 want_sums=want_sums, wb=model.wb, wd=model.wd)
    return mask, probs, sums


class _CaseShard:
    """This rank's contiguous shard of a case table as the `loader` of loop.held_out_pass: one case index (into the GLOBAL table) per step."""
    sharded = True

    def __init__(self, n, rank, world):
        self.mine = range(rank * n // world, (rank + 1) * n // world)

    def __iter__(self):
        return iter(self.mine)


def evaluate_sliding(model, cases, crop, b, overlap, window, rank=0, world=1, group=None, mirror=(0,)):
    """`evaluate` with every case predicted by sliding_window: the same dictionary from the same ONE held_out_pass, one all_reduce of sums and counts
    and one host read-back.  The sums of the cases add up (they are sums over counted voxels), so the loss is the pass's, as in `evaluate`.
    `mirror`: sliding_window's mirror codes."""
    def case_sums(ci, counts):
        return sliding_window(model, cases[ci], crop, b, overlap, window, counts=counts, row=ci, want_mask=False, mirror=mirror)[2]

    return _held_out(model, len(cases), _CaseShard(len(cases), rank, world), group, case_sums)


def resume_segmenter(path, model, optimizer, rank):
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    model.load_state_dict(ckpt["state_dict"])
    if "optimizer" in ckpt:
        _optim.restore(optimizer, ckpt)       # a checkpoint of another optimiser kind ends the run with a message
    return int(ckpt.get("epoch", -1))


def train_segmenter(args):
    """-> the trained model (`.test_metrics`: the final test's)."""
    return _loop.run_with_group(lambda distributed: _train_segmenter(args, distributed))


def _train_segmenter(args, distributed):
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    loaders = _data.loaders(args, rank, world)
    overlap, window = float(getattr(args, "val_overlap", 0.0)), getattr(args, "val_window", "gaussian")
    crop = _data.parse_crop(args.crop)
    mirror = _data.parse_mirror(getattr(args, "val_mirror", None), "--val_mirror")
    if len(mirror) > 1:      # mirrored validation and test: sliding windows also at --val_overlap 0, there with the constant window (one patch per voxel)
        window = window if overlap > 0 else "constant"
        held_out = lambda model, loader: evaluate_sliding(model, loader.cases, crop, args.b, overlap, window, rank, world, mirror=mirror)      # noqa: E731
        tail = "\toverlap {0:g} {1}\tmirror {2}".format(overlap, window, _data.mirror_letters(mirror))
    elif overlap > 0:        # validation and the final test by overlap-blended sliding windows; 0 (the default): the tiled pass
        held_out = lambda model, loader: evaluate_sliding(model, loader.cases, crop, args.b, overlap, window, rank, world)      # noqa: E731
        tail = "\toverlap {0:g} {1}".format(overlap, window)
    else:
        held_out, tail = evaluate, ""

    def make(rank):
        return Segmenter3d(args.n_class, in_channels=args.in_channels, weights=args.weights if args.phase == "finetune" else None,
                           head=getattr(args, "head", "sigmoid"), wc=float(getattr(args, "wc", 1.0)))

    task = _loop.Task(
        make_model=make,
        make_optimizer=lambda params, **k: _optim.for_task(FusedSGD, [p for p in params if p.requires_grad], **k),      # only what the loss reaches: the heads are frozen
        resume=resume_segmenter,
        resumed="==> resumed the segmenter from {}; continuing with epoch {}",
        state_dict=lambda model: model.state_dict(),
        epoch=lambda epoch, loader, model, optimizer, verbose: _loop.run_epoch(epoch, loader, model, lambda batch: train_step(model, optimizer, batch),
                                                                               (("seg loss", 0),), verbose),
        validate=lambda model, loader, epoch: held_out(model, loader),
        val_text=lambda val: _fmt(val) + tail, better=higher_dice, best_keys=('epoch', 'state_dict', 'val'),
        val_every_0_is_1=True, save_last=True)
    model, last_epoch, chatty = _loop.run_epochs(args, loaders, task, distributed)
    if last_epoch is not None:       # the final test: the best model by validation Dice when one was kept, otherwise the last epoch's
        if distributed:
            dist.barrier()
        best_file = _loop.checkpoint_name(args, "best")
        which = "last epoch %d" % last_epoch
        if getattr(args, "save_best", False) and os.path.exists(best_file):
            ckpt = torch.load(best_file, map_location="cpu", weights_only=False)
            model.load_state_dict(ckpt["state_dict"])
            which = "best epoch %d" % ckpt["epoch"]
        test = held_out(model, loaders['test'])
        if chatty:
            print('Test: ({0})\t{1}\tper class {2}{3}'.format(which, _fmt(test), " ".join("%.4f" % d for d in test["dice"]), tail))
            sys.stdout.flush()
        model.test_metrics = test
    return model


# ---- predict ----------------------------------------------------------------------------------------------------------------------
def split_weights(text):
    """--weights of `predict`: one checkpoint, or several separated by commas (an ensemble) -> the list of paths; an empty entry exits with its message."""
    files = [f.strip() for f in str(text).split(",")]
    if not files or any(not f for f in files):
        raise SystemExit(f"--weights {text}: one checkpoint of `seg3d.py train`, or several separated by commas (their logits are averaged)")
    return files


def read_state_dict(weights):
    if not os.path.isfile(weights):
        raise SystemExit(f"--weights {weights}: no such file (a checkpoint written by `seg3d.py train`)")
    return torch.load(weights, map_location="cpu", weights_only=False)["state_dict"]


def state_dict_sizes(sd):
    """(n_class, in_channels) of a segmenter's state dict."""
    return int(sd["out_tr.final_conv.weight"].shape[0]), int(sd["down_tr64.ops.0.conv1.weight"].shape[1])


def checkpoint_head(ckpt):
    """The head kind of a checkpoint of `seg3d.py train`: the validation dictionary of a _best.pt (val['head']) or the options of a last-epoch one
    (opt.head); a checkpoint with neither is a sigmoid one."""
    val, opt = ckpt.get("val"), ckpt.get("opt")
    head = val.get("head") if isinstance(val, dict) and "head" in val else getattr(opt, "head", "sigmoid")
    return _data.check_head(head)


def read_head(weights):
    return checkpoint_head(torch.load(weights, map_location="cpu", weights_only=False))


def check_ensemble(files, state_dicts, heads=None):
    """The checkpoints of an ensemble agree in n_class and in_channels (and, with `heads`, in the head kind), or the first one that differs from the
    first exits with a message naming both files.  On the host, on the state dicts.  -> (n_class, in_channels)"""
    if heads is not None:
        for f, h in zip(files[1:], heads[1:]):
            if h != heads[0]:
                raise SystemExit(f"--weights: {f} was trained with --head {h}, {files[0]} with --head {heads[0]}: the checkpoints of an ensemble must "
                                 "have the same head kind (a bitmask and a label map cannot be averaged)")
    first = state_dict_sizes(state_dicts[0])
    for f, sd in zip(files[1:], state_dicts[1:]):
        got = state_dict_sizes(sd)
        if got != first:
            raise SystemExit(f"--weights: {f} has n_class {got[0]} and in_channels {got[1]}, {files[0]} has n_class {first[0]} and in_channels {first[1]}: "
                             "the checkpoints of an ensemble must agree in both (their logits are averaged voxel by voxel)")
    return first


def load_segmenter(weights, device, amp=False, state_dict=None, head=None):
    sd = read_state_dict(weights) if state_dict is None else state_dict
    n_class, in_channels = state_dict_sizes(sd)
    model = Segmenter3d(n_class, in_channels=in_channels, head=read_head(weights) if head is None else head)
    model.load_state_dict(sd)
    model = model.to(device)
    if amp:
        model.set_compute_dtype(torch.bfloat16)
    return model


def predict_case(model, case, crop, b):
    """The predicted bitmask (softmax head: label map) uint8 [X, Y, Z] of one case, stitched from its tiles (each voxel from the one tile that counts it)."""
    dev = next(model.parameters()).device
    out = np.zeros(case.shape, dtype=np.uint8)
    for x, lab, _, starts in _data.TileLoader([case], crop, b):
        mask = model.infer(to_gpu(x), labels=(lab & _data.NOT_COUNTED).to(dev), want_mask=True)[3].cpu().numpy()
        for m, l, st in zip(mask, lab.numpy(), starts.tolist()):
            own = (l & _data.NOT_COUNTED) == 0
            idx = np.nonzero(own)
            out[idx[0] + st[0], idx[1] + st[1], idx[2] + st[2]] = m[own]
    return out


def predict(args, log=print):
    crop = _data.parse_crop(args.crop)
    overlap, window, want_probs = float(getattr(args, "overlap", 0.0)), getattr(args, "window", "gaussian"), bool(getattr(args, "probs", False))
    rules = parse_cleanup(args)          # None (the default): the masks are written as predicted
    mirror = _data.parse_mirror(getattr(args, "mirror", None))
    files = split_weights(args.weights)
    state_dicts = [read_state_dict(f) for f in files]
    heads = [read_head(f) for f in files]
    check_ensemble(files, state_dicts, heads)       # on the host, before any model goes to the device
    # mirrored passes and ensembles add logits into sliding_window's buffer: they take that path also at --overlap 0, where every voxel has one patch
    # and the mask does not depend on the (positive) window
    sliding = overlap > 0 or len(mirror) > 1 or len(files) > 1
    device = torch.device("cuda", args.gpu)
    torch.cuda.set_device(device)
    models = [load_segmenter(f, device, args.amp, state_dict=sd, head=h) for f, sd, h in zip(files, state_dicts, heads)]
    model = models[0]
    del state_dicts
    if rules is not None:
        rules = (resolve_keep(rules[0], model.n_class),) + rules[1:]
    os.makedirs(args.out, exist_ok=True)
    write_head_kind(args.out, model.head)
    clean = postprocess_labelmap if model.head == "softmax" else postprocess_mask
    names = _data.read_list(args.data, args.list)
    for name in names:
        case = _data.open_case(args.data, name, model.n_class, model.in_channels, need_seg=False, head=model.head)
        case.seg = None          # the prediction does not look at labels
        if sliding:
            mask, probs, _ = sliding_window(model, case, crop, args.b, overlap, window, want_probs=want_probs, mirror=mirror, models=models)
            if rules is not None:
                mask = clean(mask, model.n_class, *rules)[0]
            np.save(os.path.join(args.out, name + "_pred.npy"), mask.cpu().numpy())
            if want_probs:
                np.save(os.path.join(args.out, name + "_prob.npy"), probs.half().cpu().numpy())
        else:
            mask = predict_case(model, case, crop, args.b)
            if rules is not None:         # the stitched mask is on the host: one upload
                mask = clean(torch.from_numpy(mask).to(device), model.n_class, *rules)[0].cpu().numpy()
            np.save(os.path.join(args.out, name + "_pred.npy"), mask)
    log(f"[seg3d] {len(names)} masks written to {args.out}")
    return len(names)


# ---- postprocess: connected-component clean-up of masks -----------------------------------------------------------
def kept_components(sizes, keep_largest, min_voxels):
    """Host: the rule of ops.filter_components on the sizes of one class's components -> bool [n].  keep_largest: the first maximum (the lowest label
    among equals); min_voxels: sizes >= min_voxels; both: both."""
    sizes = np.asarray(sizes, dtype=np.int64)
    keep = np.ones(len(sizes), dtype=bool)
    if keep_largest and len(sizes):
        keep = np.arange(len(sizes)) == int(np.argmax(sizes))
    if min_voxels > 0:
        keep &= sizes >= min_voxels
    return keep


def postprocess_mask(mask, K, keep_largest=(), min_voxels=0, connectivity=6):
    """Connected-component clean-up of a device uint8 [X, Y, Z] bitmask, class by class (the classes are independent bits, so their order does not
    matter): the classes in `keep_largest` keep only their largest component (among equals the one that comes first in C order), and with
    min_voxels > 0 every class loses its components below that volume; components under connectivity 6, 18 or 26.  A class that no rule touches is
    not labelled.  Per class that is: one read-back of the component count and one of the sizes, for the report.
    -> (mask, report): report[k] = {'before', 'after': components (None: class k was not touched), 'removed': voxels}"""
    K, keep, min_voxels = int(K), {int(k) for k in keep_largest}, int(min_voxels)
    report = []
    for k in range(K):
        if k not in keep and min_voxels <= 0:
            report.append({"before": None, "after": None, "removed": 0})
            continue
        labels, sizes = _ops.label_components(mask, k, connectivity)
        mask = _ops.filter_components(mask, labels, sizes, k, k in keep, min_voxels)
        host = sizes.cpu().numpy().astype(np.int64)
        kept = kept_components(host, k in keep, min_voxels)
        report.append({"before": len(host), "after": int(kept.sum()), "removed": int(host[~kept].sum())})
    return mask, report


def postprocess_labelmap(lab, K, keep_largest=(), min_voxels=0, connectivity=6):
    """postprocess_mask for a device uint8 [X, Y, Z] LABEL MAP of K classes (0 = background, which no rule touches): the classes 1..K-1 go through the
    bitmask machinery in groups of at most 7 -- ops.seg_labelmap_to_bits, postprocess_mask on the group's bitmask, ops.seg_labelmap_keep, which turns
    a voxel whose class lost its bit into background.  -> (label map, report [K]) with report[0] untouched."""
    K, keep = int(K), {int(k) for k in keep_largest}
    report = [{"before": None, "after": None, "removed": 0}]
    for first in range(1, K, 7):
        n = min(7, K - first)
        bits = _ops.seg_labelmap_to_bits(lab, first, n)
        bits, rep = postprocess_mask(bits, n, [k - first for k in keep if first <= k < first + n], min_voxels, connectivity)
        lab = _ops.seg_labelmap_keep(lab, bits, first, n)
        report.extend(rep)
    return lab, report


def _labelmap_classes(args, flag="--labelmap"):
    """--labelmap: the stored arrays are label maps of --n_class classes, the background included (2..16)."""
    return _data.check_n_class(args.n_class, "softmax")


def _refuse_above(path, arr, K):
    top = int((np.asarray(arr).reshape(-1) & 0x7F).max()) if arr.size else 0
    if top >= K:
        raise SystemExit(f"{path}: label value {top} but --n_class is {K} with --labelmap (a label-map byte holds the class index 0..{K - 1} in bits "
                         "0..6, 0 = background)")


def parse_cleanup(args):
    """--keep_largest, --min_voxels and --connectivity of `predict` and `postprocess` (absent attributes: the defaults), checked on the host.
    -> None when neither rule is given, else (keep, min_voxels, connectivity) with keep a tuple of classes or 'all' (resolve_keep)."""
    raw = str(getattr(args, "keep_largest", "") or "").strip()
    min_voxels, connectivity = getattr(args, "min_voxels", 0) or 0, getattr(args, "connectivity", 6)
    if connectivity not in _ops.CCL_CONNECTIVITIES:
        raise SystemExit(f"--connectivity {connectivity}: 6 (faces), 18 (faces and edges) or 26 (faces, edges and corners)")
    if min_voxels < 0:
        raise SystemExit(f"--min_voxels {min_voxels}: the smallest volume of a component that stays, in voxels; 0 or more")
    keep = "all" if raw == "all" else ()
    if raw and raw != "all":
        try:
            keep = tuple(sorted({int(v) for v in raw.split(",")}))
        except ValueError:
            keep = (-1,)
        if min(keep) < 0:
            raise SystemExit(f"--keep_largest {raw}: class numbers separated by commas, or `all`")
    if not keep and min_voxels == 0:
        return None
    return keep, int(min_voxels), int(connectivity)


def resolve_keep(keep, K):
    """'all' -> every class; a class >= K is refused."""
    if keep == "all":
        return tuple(range(K))
    for k in keep:
        if k >= K:
            raise SystemExit(f"--keep_largest {k}: the masks have the classes 0..{K - 1} (--n_class {K})")
    return tuple(keep)


def postprocess_plan(args):
    """Everything `postprocess` refuses, checked on the host before a GPU is touched.  -> (K, (keep, min_voxels, connectivity), [(case, in, out)])"""
    labelmap = bool(getattr(args, "labelmap", False))
    K = _labelmap_classes(args) if labelmap else _data.check_n_class(args.n_class)
    rules = parse_cleanup(args)
    if rules is None:
        raise SystemExit("postprocess: no rule given: --keep_largest CLASSES|all and / or --min_voxels N")
    rules = (resolve_keep(rules[0], K),) + rules[1:]
    if os.path.realpath(args.out) == os.path.realpath(args.pred):
        raise SystemExit(f"--out {args.out}: the same directory as --pred; the cleaned masks would overwrite the predictions they were made from")
    plan = []
    for name in _data.read_list(args.pred, args.list):
        path = os.path.join(args.pred, name + "_pred.npy")
        if not os.path.exists(path):
            raise SystemExit(f"{path}: missing (the prediction of a case is <case>_pred.npy, as `seg3d.py predict` writes it)")
        pred = np.load(path, mmap_mode="r")
        if pred.ndim != 3 or pred.dtype != np.uint8 or pred.size == 0 or pred.size >= 1 << 31:
            raise SystemExit(f"{path}: a prediction is a non-empty uint8 array [X, Y, Z] of fewer than 2^31 voxels, got {pred.dtype} {pred.shape}")
        if labelmap:
            _refuse_above(path, pred, K)
        else:
            refuse_labelmap_prediction(args.pred, "postprocess")
        plan.append((name, path, os.path.join(args.out, name + "_pred.npy")))
    if not plan:
        raise SystemExit(f"{args.list}: no cases")
    return K, rules, plan


def postprocess(args, log=print):
    """`seg3d.py postprocess`: the stored predictions of --pred cleaned into --out.  -> [(case, report)]"""
    K, rules, plan = postprocess_plan(args)
    device = torch.device("cuda", args.gpu)
    torch.cuda.set_device(device)
    os.makedirs(args.out, exist_ok=True)
    done = []
    for name, src, dst in plan:
        clean = postprocess_labelmap if getattr(args, "labelmap", False) else postprocess_mask
        mask, report = clean(torch.from_numpy(np.load(src)).to(device), K, *rules)
        np.save(dst, mask.cpu().numpy())
        done.append((name, report))
        log(name + "\t" + "\t".join("class {0}: components {1} -> {2}, {3} voxels removed".format(k, r["before"], r["after"], r["removed"])
                                    for k, r in enumerate(report) if r["before"] is not None))
    if getattr(args, "labelmap", False):
        write_head_kind(args.out, "softmax")
    log("Postprocess: {0} cases, connectivity {1}\t".format(len(plan), rules[2]) + "\t".join(
        "class {0}: {1} voxels removed".format(k, sum(rep[k]["removed"] for _, rep in done)) for k in range(K)))
    return done


# ---- score: surface distances of stored masks -----------------------------------------------------------------
SURFACE_KEYS = ("hd95", "hd", "assd")


def surface_from_records(records, q=0.95):
    """Host, float64: the records of ops.surf_dist_stats, int64 [K][8] -> {'hd95', 'hd', 'assd': float64 [K], 'n_pred', 'n_gt': int64 [K]}.
    hd95 is numpy.percentile(U, 100 q) with the default linear method on the distances U = sqrt(d2) (sqrt is monotone, so the order statistics of
    the distances are the square roots of those of d2); hd = max U; assd = (mean A + mean B) / 2, MedPy's.  Both surfaces empty: all three are 0.0;
    exactly one empty: all three are NaN."""
    rec = np.ascontiguousarray(np.asarray(records, dtype=np.int64).reshape(-1, _ops.SURF_REC))
    as_f = rec.view(np.float64)
    K = rec.shape[0]
    out = {k: np.zeros(K, dtype=np.float64) for k in SURFACE_KEYS}
    out["n_pred"], out["n_gt"] = rec[:, 0].copy(), rec[:, 1].copy()
    for k in range(K):
        na, nb = int(rec[k, 0]), int(rec[k, 1])
        if na == 0 and nb == 0:
            continue
        if na == 0 or nb == 0:
            for key in SURFACE_KEYS:
                out[key][k] = np.nan
            continue
        n = na + nb
        virtual = np.float64(q) * np.float64(n - 1)
        lo = np.floor(virtual)
        d_lo, d_hi, d_max = (np.sqrt(as_f[k, 3 + i]) for i in range(3))
        out["hd95"][k] = d_lo if virtual >= n - 1 else lerp(d_lo, d_hi, virtual - lo)
        out["hd"][k] = d_max
        out["assd"][k] = (as_f[k, 6] / na + as_f[k, 7] / nb) / 2.0
    return out


def surface_metrics(pred, gt, K, spacing=(1.0, 1.0, 1.0), q=0.95):
    """HD95, HD and ASSD per class of a predicted against a ground-truth bitmask, device uint8 tensors [X, Y, Z] (bit k = class k; a voxel with bit 7
    of `gt` set belongs to neither mask): the surfaces of all classes in one launch, then per class the two exact squared distance transforms with
    the voxel `spacing` and the order statistics into ONE device table [K][8]; ONE host read-back; the rest (sqrt, numpy's interpolation, the
    empty-mask conventions) on the host in float64.
    -> {'hd95', 'hd', 'assd': float64 [K], 'n_pred', 'n_gt': int64 [K] surface voxels, 'counts': int64 [K, 3] = {TP, |pred|, |gt|}}"""
    K = int(K)
    sp, sg, counts = _ops.surf_extract(pred, gt, K)
    table = torch.zeros((K, _ops.SURF_REC), dtype=torch.int64, device=pred.device)
    d2g = torch.empty(tuple(pred.shape), dtype=torch.float64, device=pred.device)
    d2p = torch.empty_like(d2g)
    for k in range(K):
        _ops.edt_sq(sg, k, spacing, out=d2g)
        _ops.edt_sq(sp, k, spacing, out=d2p)
        _ops.surf_dist_stats(d2g, sp, d2p, sg, k, q, record=table[k])
    host = torch.cat([table.reshape(-1), counts.reshape(-1)]).cpu().numpy()
    out = surface_from_records(host[:K * _ops.SURF_REC], q)
    out["counts"] = host[K * _ops.SURF_REC:].reshape(K, 3).copy()
    return out


def crop_to_masks(pred, seg):
    """Both arrays cut to the bounding box of (pred | seg) & 0x7f, or None when that is empty.  Exact for the surface metrics: both masks are empty
    outside the box, and a face of the box behaves like a face of the volume (what lies beyond is not in the mask)."""
    any_bit = ((pred | seg) & 0x7F) != 0
    if not any_bit.any():
        return None
    box = []
    for axis in range(3):
        hit = np.nonzero(any_bit.any(axis=tuple(a for a in range(3) if a != axis)))[0]
        box.append(slice(int(hit[0]), int(hit[-1]) + 1))
    box = tuple(box)
    return np.ascontiguousarray(pred[box]), np.ascontiguousarray(seg[box])


def parse_spacing(spacing, what="--spacing"):
    """'sx,sy,sz' or a sequence -> three positive finite floats, else SystemExit."""
    try:
        sp = tuple(float(v) for v in (spacing.split(",") if isinstance(spacing, str) else np.asarray(spacing).reshape(-1).tolist()))
    except (TypeError, ValueError):
        sp = ()
    if len(sp) != 3 or not all(np.isfinite(v) and v > 0 for v in sp):
        raise SystemExit(f"{what} {spacing}: three positive finite numbers sx,sy,sz (the voxel size along X, Y, Z)")
    return sp


def score_plan(args):
    """Everything `score` refuses, checked on the host before a GPU is touched.  -> [(case, seg path, pred path, spacing)]"""
    labelmap = bool(getattr(args, "labelmap", False))
    K = _labelmap_classes(args) if labelmap else _data.check_n_class(args.n_class)
    if not labelmap:
        refuse_labelmap_prediction(args.pred, "score")
    default = parse_spacing(args.spacing)
    plan = []
    for name in _data.read_list(args.data, args.list):
        seg_path, pred_path = os.path.join(args.data, name + "_seg.npy"), os.path.join(args.pred, name + "_pred.npy")
        sp_path = os.path.join(args.data, name + "_spacing.npy")
        if not os.path.exists(seg_path):
            raise SystemExit(f"{seg_path}: missing (the ground truth of a case is <case>_seg.npy [X,Y,Z] uint8)")
        if not os.path.exists(pred_path):
            raise SystemExit(f"{pred_path}: missing (the prediction of a case is <case>_pred.npy, as `seg3d.py predict` writes it)")
        seg, pred = np.load(seg_path, mmap_mode="r"), np.load(pred_path, mmap_mode="r")
        if seg.ndim != 3 or seg.dtype != np.uint8:
            raise SystemExit(f"{seg_path}: expected a uint8 array [X, Y, Z], got {seg.dtype} {seg.shape}")
        if pred.dtype != np.uint8 or pred.shape != seg.shape:
            raise SystemExit(f"{pred_path}: a prediction is a uint8 array of its label's shape {seg.shape}, got {pred.dtype} {pred.shape}")
        if labelmap:         # a value >= K is refused before the GPU is touched
            _refuse_above(seg_path, seg, K)
            _refuse_above(pred_path, pred, K)
        spacing = parse_spacing(np.load(sp_path), sp_path + ":") if os.path.exists(sp_path) else default
        plan.append((name, seg_path, pred_path, spacing))
    if not plan:
        raise SystemExit(f"{args.list}: no cases")
    return K, plan


def score(args, log=print):
    """`seg3d.py score`: Dice, HD95, HD and ASSD per case and class of stored predictions.  -> the rows (case, class, dice, hd95, hd, assd, n_pred, n_gt)"""
    K, plan = score_plan(args)
    labelmap = bool(getattr(args, "labelmap", False))
    classes = list(range(1, K)) if labelmap else list(range(K))       # label maps: one row per (case, class 1..K-1); the background is not scored
    device = None
    rows = []
    for name, seg_path, pred_path, spacing in plan:
        cut = crop_to_masks(np.load(pred_path), np.load(seg_path))
        if cut is None:          # nothing predicted, nothing labelled: every class scores Dice 1 and distance 0 without a launch
            nc = len(classes)
            m = {key: np.zeros(nc) for key in SURFACE_KEYS}
            m.update(n_pred=np.zeros(nc, dtype=np.int64), n_gt=np.zeros(nc, dtype=np.int64), counts=np.zeros((nc, 3), dtype=np.int64))
        else:
            if device is None:
                device = torch.device("cuda", args.gpu)
                torch.cuda.set_device(device)
            top = _ops.edt_max_axis()
            if max(cut[0].shape) > top:
                raise SystemExit(f"{name}: the bounding box of its masks is {cut[0].shape}; an axis may have at most {top} voxels")
            pd, gd = torch.from_numpy(cut[0]).to(device), torch.from_numpy(cut[1]).to(device)
            if labelmap:         # the classes 1..K-1 through the bitmask machinery, at most 7 at a time
                parts = [surface_metrics(_ops.seg_labelmap_to_bits(pd, first, min(7, K - first)), _ops.seg_labelmap_to_bits(gd, first, min(7, K - first)),
                                         min(7, K - first), spacing) for first in range(1, K, 7)]
                m = {key: np.concatenate([p[key] for p in parts]) for key in parts[0]}
            else:
                m = surface_metrics(pd, gd, K, spacing)
        for i, k in enumerate(classes):
            dice = dice_from_counts([[m["counts"][i].tolist()]])[1]
            rows.append((name, k, dice, float(m["hd95"][i]), float(m["hd"][i]), float(m["assd"][i]), int(m["n_pred"][i]), int(m["n_gt"][i])))
        log("{0}\tspacing {1}\t".format(name, ",".join("%g" % s for s in spacing)) + "\t".join(
            "class {0}: Dice {1:.4f} HD95 {2:.3f} HD {3:.3f} ASSD {4:.3f}".format(*r[1:6]) for r in rows[-len(classes):]))
    means = []
    for k in classes:
        part = ["class %d:" % k]
        for col, label in ((2, "Dice"), (3, "HD95"), (4, "HD"), (5, "ASSD")):
            vals = [r[col] for r in rows if r[1] == k and r[col] == r[col]]      # a NaN (one empty surface) is left out of the mean
            part.append("{0} {1:.4f} ({2})".format(label, sum(vals) / len(vals) if vals else float("nan"), len(vals)))
        means.append(" ".join(part))
    log("Score: {0} cases\t".format(len(plan)) + "\t".join(means))
    if args.csv:
        with open(args.csv, "w") as f:
            f.write("case,class,dice,hd95,hd,assd,n_pred,n_gt\n")
            for r in rows:
                f.write("{0},{1},{2!r},{3!r},{4!r},{5!r},{6},{7}\n".format(*r))
    return rows
