"""LUNA16 nodule classification (false-positive reduction), the downstream task of the 3D encoder: candidate cubes, fine-tuning, prediction.

    python luna_nodules.py extract --data LUNA16 --candidates candidates_V2.csv --save CUBES
    python luna_nodules.py train   --data CUBES --phase finetune --encoder_weights PRETRAIN.pt --save_best --output OUT
    python luna_nodules.py predict --data LUNA16 --candidates candidates_V2.csv --weights OUT/pcrlv2_luna_nodules_finetune_0.8_best.pt --out scores.csv

The reference's fine-tune branch is not public.  What is pinned: which series are for fine-tuning (`--ratio`: the LAST 1 - ratio of
train_val_txt/luna_train.txt, utils.get_luna_finetune_list), the encoder's checkpoint keys (models.NoduleClassifier), the normalisation (HU clipped to
[-1000, 1000], (v + 1000) / 2000, then the pre-task's z-normalisation) and LUNA16's world-to-voxel rule.  This project's choices: the cube size
(64 x 64 x 32, the pre-task's crop), the per-series negative subsample, balanced epochs, one linear head, BCE, AUROC, the fold split
(train 0-6, validation 7, test 8-9).  DESIGN.md section 14.

extract   per series: read (luna_prep.read_metaimage, one series ahead) -> 1 mm volume on the device (luna_prep.prepare_volume) -> the kept
          candidates' cubes in one or a few `pcrl_prep_cubes` launches (int16) -> `<save>/subset<f>/<series>_cand.npy` [n, CX, CY, CZ] and
          `<series>_cand_meta.npz` (world float64 [n, 3], label uint8 [n], index int64 [n]: the row in the CSV), written by threads.
train     train_finetune.train_classifier on models.NoduleClassifier over data.nodule_loaders (or data.SyntheticNoduleLoader).
predict   no cube touches the disk: per series the volume, then per chunk of --b candidates ONE `pcrl_prep_cubes` launch (float32) straight into the
          batch, the z-normalisation and NoduleClassifier.infer; EVERY candidate is scored; one host read-back per series.
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import os
import sys
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from .data import parse_folds
from .luna_prep import MetaImageError, prepare_volume, read_metaimage, series_list, stable_hash

CUBE = (64, 64, 32)
LAUNCH_CUBES = 2048          # cubes per extract launch: 512 MB of int16 at the default size


# ---- candidates -----------------------------------------------------------------------------------------------------------------
class Candidates(NamedTuple):
    world: np.ndarray       # float64 [n, 3]: coordX, coordY, coordZ in world millimetres
    label: np.ndarray       # uint8 [n] (0 where the file has no class column)
    index: np.ndarray       # int64 [n]: row in the CSV (0 = the first line after the header)
    text: list              # [n] (coordX, coordY, coordZ) as written in the file


def read_candidates(csv_path):
    """LUNA16's candidates format `seriesuid,coordX,coordY,coordZ,class` (one header line) -> {series: Candidates}, rows in file order."""
    rows = {}
    with open(csv_path) as f:
        header = f.readline()
        if "seriesuid" not in header:
            raise ValueError(f"{csv_path}: the first line must be the header `seriesuid,coordX,coordY,coordZ,class`")
        i = 0
        for line in f:
            parts = line.strip().split(",")
            if len(parts) < 4 or parts[0] == "":
                continue
            rows.setdefault(parts[0], []).append((i, parts[1:4], int(parts[4]) if len(parts) > 4 and parts[4] != "" else 0))
            i += 1
    return {s: Candidates(np.array([[float(v) for v in r[1]] for r in rs], dtype=np.float64).reshape(-1, 3), np.array([r[2] for r in rs], dtype=np.uint8),
                          np.array([r[0] for r in rs], dtype=np.int64), [tuple(r[1]) for r in rs]) for s, rs in rows.items()}


def world_to_voxel(world, hdr):
    """World millimetres -> index on the 1 mm grid of luna_prep.prepare_volume (ITK's resample keeps origin and direction):
    floor(d_a * (world_a - Offset_a) + 0.5) per axis, d_a the diagonal of TransformMatrix (+-1: LUNA16 has scans flipped on x and y).  A matrix that
    is no signed identity raises MetaImageError."""
    m = np.asarray(hdr["TransformMatrix"], dtype=np.float64)
    if m.size != 9:
        raise MetaImageError(f"TransformMatrix has {m.size} values (9 are needed)")
    m = m.reshape(3, 3)
    d = np.diag(m)
    if np.any(m - np.diag(d) != 0.0) or np.any(np.abs(d) != 1.0):
        raise MetaImageError(f"TransformMatrix {m.reshape(-1).tolist()} is not diagonal with +-1 entries (an oblique scan is not supported)")
    off = np.asarray(hdr["Offset"], dtype=np.float64)
    return np.floor(d * (np.asarray(world, dtype=np.float64).reshape(-1, 3) - off) + 0.5).astype(np.int64)


def world_to_start(world, hdr, cube=CUBE):
    """-> int32 [n, 3]: (x0, y0, z0) of the cube centred on each candidate, centre - cube / 2; may lie outside the volume (pcrl_prep_cubes pads with air)."""
    return (world_to_voxel(world, hdr) - np.asarray(cube, dtype=np.int64) // 2).astype(np.int32)


def subsample(series, labels, negatives, seed):
    """The rows of one series that extract keeps, sorted: every positive, and of the negatives `rng.permutation(n_neg)[:negatives]` with
    rng = default_rng([seed, stable_hash(series)]) (-1: all).  A function of the series alone: independent of fold grouping, order and process count."""
    labels = np.asarray(labels)
    neg = np.flatnonzero(labels == 0)
    if negatives >= 0:
        rng = np.random.default_rng([int(seed), stable_hash(series)])
        neg = neg[np.sort(rng.permutation(neg.size)[:negatives])]
    return np.sort(np.concatenate([np.flatnonzero(labels != 0), neg])).astype(np.int64)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def check_cube(cube):
    cube = tuple(int(c) for c in cube)
    if len(cube) != 3 or any(c <= 0 or c > 64 or c % 8 for c in cube):
        raise SystemExit(f"--cube {cube}: three positive multiples of 8, each <= 64")
    return cube


def gpu_cubes(vol_dev, start, cube=CUBE, float32=False, out=None):
    """int16 [Z, Y, X] device volume, int32 [M, 3] starts (host array or device tensor) -> [M, CX, CY, CZ] int16, or float32 normalised to [0, 1]
    (pcrl_prep_cubes).  `out`: write into the first M rows of this tensor."""
    Z, Y, X = vol_dev.shape
    if not torch.is_tensor(start):
        start = torch.from_numpy(np.ascontiguousarray(start, dtype=np.int32))
    start = start.to(vol_dev.device).contiguous()
    M = start.shape[0]
    dt = torch.float32 if float32 else torch.int16
    if out is None:
        out = torch.empty((M,) + tuple(cube), dtype=dt, device=vol_dev.device)
    elif out.dtype != dt or tuple(out.shape[1:]) != tuple(cube) or out.shape[0] < M or not out.is_contiguous():
        raise ValueError("gpu_cubes: `out` does not fit")
    _lib.lib().call("pcrl_prep_cubes", vol_dev, X, Y, Z, start, M, out, 1 if float32 else 0, cube[0], cube[1], cube[2], _lib.stream_handle())
    return out[:M]


# ---- extract --------------------------------------------------------------------------------------------------------------------
def _save_series(save_dir, name, cubes, world, label, index):
    np.save(os.path.join(save_dir, name + "_cand.npy"), cubes)
    np.savez(os.path.join(save_dir, name + "_cand_meta.npz"), world=world, label=label, index=index)


MAX_WRITERS = 14      # + the reader thread + the main thread: at most 16 threads whatever the machine reports


def _series_ahead(files, reader):
    """Yields (fold, path, name, (vol, spacing, hdr) | None, error | None) with the next series already being read."""
    nxt = reader.submit(read_metaimage, files[0][1]) if files else None
    for i, (fold, path) in enumerate(files):
        got, err = None, None
        try:
            got = nxt.result()
        except (MetaImageError, OSError, KeyError, ValueError) as e:
            err = e
        nxt = reader.submit(read_metaimage, files[i + 1][1]) if i + 1 < len(files) else None
        yield fold, path, os.path.basename(path)[:-4], got, err


def extract(args, log=print):
    """-> {"series": n written, "cubes": n, "skipped": [(path, reason)]}"""
    cube = check_cube(args.cube)
    cands = read_candidates(args.candidates)
    device = torch.device("cuda", args.gpu)
    torch.cuda.set_device(device)
    files = [(f, p) for f, p in series_list(args.data, parse_folds(args.folds)) if os.path.basename(p)[:-4] in cands]
    result = {"series": 0, "cubes": 0, "skipped": []}
    with cf.ThreadPoolExecutor(1) as reader, cf.ThreadPoolExecutor(max(1, min(MAX_WRITERS, args.writers))) as writer:
        pending = []
        for fold, path, name, got, err in _series_ahead(files, reader):
            if err is None:
                try:
                    c = cands[name]
                    keep = subsample(name, c.label, args.negatives, args.seed)
                    start = world_to_start(c.world[keep], got[2], cube)
                except MetaImageError as e:
                    err = e
            if err is not None:
                log(f"[luna_nodules] skip {path}: {err}")
                result["skipped"].append((path, str(err)))
                continue
            vol, _ = prepare_volume(got[0], got[1], device)
            parts = [gpu_cubes(vol, start[a:a + LAUNCH_CUBES], cube).cpu() for a in range(0, len(keep), LAUNCH_CUBES)]
            cubes = (torch.cat(parts) if parts else torch.empty((0,) + cube, dtype=torch.int16)).numpy()
            save_dir = os.path.join(args.save, f"subset{fold}")
            os.makedirs(save_dir, exist_ok=True)
            pending.append(writer.submit(_save_series, save_dir, name, cubes, c.world[keep], c.label[keep], c.index[keep]))
            result["series"] += 1
            result["cubes"] += len(keep)
            log(f"[luna_nodules] subset{fold}/{name}: {len(keep)} of {len(c.label)} candidates ({int(c.label[keep].sum())} positive)")
            while len(pending) > 8:          # bound the host memory held by queued writes
                pending.pop(0).result()
        for p in pending:
            p.result()
    log(f"[luna_nodules] {result['series']} series, {result['cubes']} cubes written, {len(result['skipped'])} skipped")
    return result


# ---- train ----------------------------------------------------------------------------------------------------------------------
def train(args):
    if args.phase == "finetune" and not args.encoder_weights:
        raise SystemExit("--phase finetune needs --encoder_weights (a 3D pre-training checkpoint); to train the classifier from random weights use --phase scratch")
    from . import optim_cli
    optim_cli.check(args)
    from .main import launch
    launch(args)
    from .data import SyntheticNoduleLoader, nodule_loaders
    from .models import NoduleClassifier
    from .train_finetune import train_classifier
    if args.data == "synthetic":
        rank = int(os.environ.get("RANK", "0"))
        cube = check_cube(args.cube)
        mk = lambda off: SyntheticNoduleLoader(args.b, args.steps_per_epoch, cube, args.seed + off + rank)     # noqa: E731
        loaders = {"train": mk(0), "eval": mk(7919), "test": mk(15485)}
    elif os.path.isdir(args.data):
        loaders = nodule_loaders(args)
    else:
        raise SystemExit("--data must be 'synthetic' or a directory of candidate cubes (subset<f>/<series>_cand.npy; write one with "
                         "`python luna_nodules.py extract --data LUNA16 --candidates candidates_V2.csv --save <dir>`)")
    make = lambda: NoduleClassifier(n_class=1, dropout=args.dropout, encoder_weights=args.encoder_weights if args.phase == "finetune" else None)   # noqa: E731
    return train_classifier(args, loaders, make, "3d-nodules")


# ---- predict --------------------------------------------------------------------------------------------------------------------
def load_classifier(weights, device, amp=False):
    from .models import NoduleClassifier
    ckpt = torch.load(weights, map_location="cpu", weights_only=False)
    sd = ckpt["state_dict"]
    model = NoduleClassifier(n_class=sd["classification_head.3.weight"].shape[0])
    model.load_state_dict(sd)
    model = model.to(device)
    if amp:
        model.set_compute_dtype(torch.bfloat16)
    return model


def score_series(model, vol, start, cube, b, cut=gpu_cubes):
    """Probabilities float32 [n, n_class] ON THE DEVICE of every cube of one volume, `b` at a time: cubes (float32, `cut` = pcrl_prep_cubes) straight
    into the batch buffer, z-normalisation, NoduleClassifier.infer."""
    from .data import normalise_cubes
    start = torch.from_numpy(np.ascontiguousarray(start, dtype=np.int32)).to(vol.device)
    batch = torch.empty((b,) + tuple(cube), dtype=torch.float32, device=vol.device)
    out = []
    for a in range(0, start.shape[0], b):
        unit = cut(vol, start[a:a + b], cube, True, batch)
        out.append(model.infer(normalise_cubes(None, unit=unit)))
    return torch.cat(out) if out else torch.empty((0, model.n_class), dtype=torch.float32, device=vol.device)


def predict(args, log=print):
    """-> {"series": n, "rows": n written, "skipped": [(path, reason)]}"""
    cube = check_cube(args.cube)
    cands = read_candidates(args.candidates)
    device = torch.device("cuda", args.gpu)
    torch.cuda.set_device(device)
    model = load_classifier(args.weights, device, args.amp)
    files = [(f, p) for f, p in series_list(args.data, parse_folds(args.folds)) if os.path.basename(p)[:-4] in cands]
    rows, result = {}, {"series": 0, "rows": 0, "skipped": []}
    with cf.ThreadPoolExecutor(1) as reader:
        for fold, path, name, got, err in _series_ahead(files, reader):
            c = cands[name]
            if err is None:
                try:
                    start = world_to_start(c.world, got[2], cube)
                except MetaImageError as e:
                    err = e
            if err is not None:
                log(f"[luna_nodules] skip {path}: {err}")
                result["skipped"].append((path, str(err)))
                continue
            vol, _ = prepare_volume(got[0], got[1], device)
            probs = score_series(model, vol, start, cube, args.b).cpu().numpy()      # the series' one read-back
            for i, t, p in zip(c.index.tolist(), c.text, probs[:, 0].tolist()):
                rows[i] = f"{name},{t[0]},{t[1]},{t[2]},{p!r}\n"
            result["series"] += 1
    present = {os.path.basename(p)[:-4] for _, p in files}
    missing = sum(len(c.label) for s, c in cands.items() if s not in present)
    with open(args.out, "w") as f:
        f.write("seriesuid,coordX,coordY,coordZ,probability\n")
        for i in sorted(rows):
            f.write(rows[i])
    result["rows"] = len(rows)
    log(f"[luna_nodules] {result['rows']} candidates of {result['series']} series scored -> {args.out}"
        + (f"; {missing} rows belong to series that are not in the folds {args.folds} of {args.data}" if missing else ""))
    return result


# ---- command line ---------------------------------------------------------------------------------------------------------------
def build_parser():
    ap = argparse.ArgumentParser(description="LUNA16 nodule classification on the PCRLv2 3D encoder (HIP kernels on MI355X)")
    sub = ap.add_subparsers(dest="command", required=True)
    ex = sub.add_parser("extract", help="LUNA16 series + candidates CSV -> candidate cubes")
    ex.add_argument("--data", required=True, help="LUNA16 directory with subset0..subset9/*.mhd")
    ex.add_argument("--candidates", required=True, help="candidates_V2.csv (seriesuid,coordX,coordY,coordZ,class)")
    ex.add_argument("--save", required=True, help="output directory (subset<f>/<series>_cand.npy / _cand_meta.npz)")
    ex.add_argument("--cube", type=int, nargs=3, default=list(CUBE), help="cube size in x, y, z (multiples of 8, <= 64)")
    ex.add_argument("--negatives", type=int, default=64, help="negatives kept per series; -1 = all (every positive is kept)")
    ex.add_argument("--seed", type=int, default=1)
    ex.add_argument("--folds", default="0,1,2,3,4,5,6,7,8,9", help="comma-separated subset numbers")
    ex.add_argument("--gpu", type=int, default=0)
    ex.add_argument("--writers", type=int, default=4, help="file-writing threads (at most 14: 16 threads with the reader and the main thread)")
    tr = sub.add_parser("train", help="fine-tune (or train from scratch) the nodule classifier on extracted cubes")
    tr.add_argument("--data", required=True, help="directory of extracted cubes, or 'synthetic'")
    tr.add_argument("--phase", default="finetune", choices=("finetune", "scratch"))
    tr.add_argument("--encoder_weights", default="", help="3D pre-training checkpoint whose down_tr* entries initialise the encoder (--phase finetune)")
    tr.add_argument("--b", type=int, default=16, help="batch size PER PROCESS")
    tr.add_argument("--epochs", type=int, default=100, help="last epoch index (inclusive)")
    tr.add_argument("--lr", type=float, default=1e-3)
    tr.add_argument("--momentum", type=float, default=0.9)
    tr.add_argument("--weight_decay", type=float, default=1e-4)
    from . import optim_cli
    optim_cli.add_arguments(tr)
    tr.add_argument("--ratio", type=float, default=0.8, help="fraction of train_val_txt/luna_train.txt used for PRE-training; the last 1 - ratio train here")
    tr.add_argument("--amp", action="store_true", help="bfloat16 activations and MFMA operands")
    tr.add_argument("--gpus", default="0", help="visible device ids, comma separated")
    tr.add_argument("--val_every", type=int, default=0, help="validation after every N-th epoch; 0 = every epoch")
    tr.add_argument("--save_best", action="store_true", help="write pcrlv2_luna_nodules_<phase>_<ratio>_best.pt whenever the validation AUROC improves")
    tr.add_argument("--resume", default="", help="checkpoint to continue from (model, momentum buffers, epoch)")
    tr.add_argument("--output", default="./model_genesis_pretrain", help="checkpoint directory")
    tr.add_argument("--seed", type=int, default=42)
    tr.add_argument("--dropout", type=float, default=0.2)
    tr.add_argument("--workers", type=int, default=4)
    tr.add_argument("--val_folds", default="7")
    tr.add_argument("--test_folds", default="8,9")
    tr.add_argument("--steps_per_epoch", type=int, default=16, help="only with --data synthetic")
    tr.add_argument("--cube", type=int, nargs=3, default=list(CUBE), help="only with --data synthetic: cube size")
    tr.set_defaults(model="pcrlv2", n="luna_nodules")
    pr = sub.add_parser("predict", help="score every candidate of a CSV straight from the raw series")
    pr.add_argument("--data", required=True, help="LUNA16 directory with subset0..subset9/*.mhd")
    pr.add_argument("--candidates", required=True)
    pr.add_argument("--weights", required=True, help="a checkpoint of `train` (--save_best's or an epoch's)")
    pr.add_argument("--out", required=True, help="output CSV: seriesuid,coordX,coordY,coordZ,probability")
    pr.add_argument("--folds", default="0,1,2,3,4,5,6,7,8,9")
    pr.add_argument("--b", type=int, default=256, help="candidates per launch")
    pr.add_argument("--cube", type=int, nargs=3, default=list(CUBE), help="the cube size the classifier was trained on")
    pr.add_argument("--amp", action="store_true")
    pr.add_argument("--gpu", type=int, default=0)
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    return {"extract": extract, "train": train, "predict": predict}[args.command](args)


if __name__ == "__main__":
    main(sys.argv[1:])
