"""3D segmentation on the pre-trained PCRLv2 network, decoder included: fine-tuning and prediction.

    python seg3d.py train   --data DIR --phase finetune --weights PRETRAIN.pt --n_class 3 --in_channels 4 --save_best --output OUT
    python seg3d.py train   --data DIR --phase finetune --weights PRETRAIN.pt --n_class 3 --in_channels 4 --save_best --output OUT --augment
    python seg3d.py predict --data DIR --list test.txt --weights OUT/pcrlv2_seg3d_finetune_1.0_best.pt --out PRED
    python seg3d.py predict --data DIR --list test.txt --weights OUT/pcrlv2_seg3d_finetune_1.0_best.pt --out PRED --overlap 0.5 --window gaussian --probs
    python seg3d.py predict --data DIR --list test.txt --weights OUT/pcrlv2_seg3d_finetune_1.0_best.pt --out PRED --keep_largest all --min_voxels 8
    python seg3d.py predict --data DIR --list test.txt --weights FOLD0/best.pt,FOLD1/best.pt --out PRED --overlap 0.5 --mirror all --probs
    python seg3d.py train   --data DIR --phase finetune --weights PRETRAIN.pt --n_class 3 --in_channels 4 --val_overlap 0.5 --val_mirror xz --output OUT
    python seg3d.py postprocess --pred PRED --list DIR/test.txt --out CLEAN --n_class 3 --keep_largest 0,2 --min_voxels 8 --connectivity 26
    python seg3d.py score   --data DIR --list test.txt --pred PRED --n_class 3 --spacing 1,1,1 --csv scores.csv

DIR holds <case>_img.npy [C,X,Y,Z] float32 / float16, <case>_seg.npy [X,Y,Z] uint8 (bit k = class k, bit 7 = not counted) and train.txt / val.txt /
test.txt (pcrlv2_amd/data_seg.py); `--data synthetic` trains on phantoms.  The loop is pcrlv2_amd/train_seg.py, the model models.Segmenter3d, the
output head and its Dice/BCE loss one HIP operator (csrc/seg_head.hip).  DESIGN.md section 15.  `--overlap F` (predict) and `--val_overlap F` (train)
replace the stride-tiled patches by overlapping windows blended with a centre-weighted window (csrc/seg_blend.hip); 0, the
default, is the tiled path.  `score` compares the stored <case>_pred.npy of PRED with <case>_seg.npy: Dice, HD95, HD and ASSD per case and class, the
distances in the units of --spacing (or of <case>_spacing.npy, three float64, where DIR has one), computed on the device (csrc/surface_dist.hip,
DESIGN.md section 17).  `postprocess` cleans stored predictions by their connected components (6, 18 or 26 neighbours) into another directory that
`score --pred` reads unchanged: the classes of --keep_largest keep only their largest component, and with --min_voxels N every class loses its
components below N voxels; `predict` takes the same three options and cleans a mask on the device before it is written (csrc/components.hip,
DESIGN.md section 18).  Without them `predict` writes what it always wrote.  `train --augment` (or any `--aug_*` option) resamples the training
crops on the device -- rotation, zoom and flips of image channels and label bitmask in one kernel, then gain, bias, gamma and noise per channel
(csrc/seg_augment.hip); without those options training does what it always did.  `predict --mirror` / `train --val_mirror` show
every patch mirrored along each combination of the named axes as well, and `predict --weights a.pt,b.pt` runs several checkpoints: the un-mirrored
logits of all passes are averaged in the sliding window's one per-case buffer before the blend; `none` and one file are the earlier paths, unchanged.

    python seg3d.py prepare --data RAW --manifest cases.tsv --save DIR --regions "1,2,4;1,4;4" --spacing 1,1,1 --split 0.7,0.1,0.2 --seed 0
    python seg3d.py restore --prep DIR --pred PRED --list DIR/test.txt --out ORIG --paint "2,1,4" --nifti

`prepare` writes DIR from raw NIfTI-1 / .npy volumes (crop to the non-zero box, per-case normalisation, resampling to a common spacing, label values
to the bitmask) and `restore` takes stored predictions back to the original grid (pcrlv2_amd/seg_prep.py, csrc/seg_prep.hip).

`train --head softmax [--wc W]`: `--n_class K` in 2..16 MUTUALLY EXCLUSIVE classes with the background as class 0; <case>_seg.npy
is then a label map (bits 0..6: the class index, bit 7: not counted) and the loss is wc * cross-entropy + wd * (1 - mean Dice of the classes 1..K-1)
(csrc/seg_head_mc.hip).  `--head sigmoid` (bitmasks, the default) is everything above.  `predict` takes the head kind from the checkpoint and writes
label maps for a softmax one (and leaves head.txt next to them), blended, mirrored and ensembled through the label-map blend (pcrl_seg_mc_blend).
`prepare --classes "1;2;3,4"` writes label maps (set i -> class i + 1, everything else background; not with --regions); `restore --labelmap --paint
v0,v1,..` paints class INDEX i with v_i; `score --labelmap` and `postprocess --labelmap` take label maps (--n_class K counts the background), the classes
1..K-1 in groups of at most 7 through the bitmask kernels; without --labelmap both refuse a directory whose head.txt says softmax.
"""
from __future__ import annotations

import argparse
import sys


def check_train(args):
    """Every refused combination exits with its message, before anything touches a GPU."""
    from .data_seg import check_n_class, parse_crop
    head, wc = getattr(args, "head", "sigmoid"), float(getattr(args, "wc", 1.0))      # a namespace from before the options existed is a sigmoid one
    check_n_class(args.n_class, head)
    parse_crop(args.crop)
    if not wc >= 0:
        raise SystemExit(f"--wc {wc}: the weight of the cross-entropy term of --head softmax is a non-negative number")
    if args.in_channels < 1:
        raise SystemExit(f"--in_channels {args.in_channels}: at least 1")
    if args.phase == "finetune" and not args.weights:
        raise SystemExit("--phase finetune needs --weights (a 3D pre-training checkpoint); to train the segmenter from random weights use --phase scratch")
    if args.phase == "scratch" and args.weights:
        raise SystemExit("--phase scratch starts from random weights: drop --weights or use --phase finetune")
    if args.b < 1 or args.epochs < 1 or args.steps_per_epoch < 0:
        raise SystemExit("--b and --epochs must be positive, --steps_per_epoch non-negative")
    from .data_seg import check_overlap, check_window, parse_aug, parse_mirror
    check_overlap(args.val_overlap, "--val_overlap")
    check_window(args.val_window, "--val_window")
    parse_mirror(args.val_mirror, "--val_mirror")
    parse_aug(args)
    from . import optim_cli
    optim_cli.check(args)


def train(args):
    check_train(args)
    from .main import launch
    launch(args)
    from .train_seg import train_segmenter
    return train_segmenter(args)


def check_predict(args):
    """Every refused combination exits with its message, before anything touches a GPU."""
    from .data_seg import check_overlap, check_window, parse_crop, parse_mirror
    from .train_seg import split_weights
    parse_crop(args.crop)
    if args.b < 1:
        raise SystemExit("--b must be positive")
    check_window(args.window)
    sliding = len(parse_mirror(args.mirror)) > 1 or len(split_weights(args.weights)) > 1      # these keep per-patch logits also at --overlap 0
    if check_overlap(args.overlap) == 0 and args.probs and not sliding:
        raise SystemExit("--probs writes the blended probabilities of overlapping windows: it needs --overlap > 0, a --mirror other than none or several "
                         "--weights (the tiled path thresholds its logits inside the kernel)")


def predict(args):
    check_predict(args)
    from .train_seg import predict as run
    return run(args)


def score(args):
    """Every refusal (spacing, --n_class, a missing or mis-shaped prediction) exits with its message in train_seg.score_plan, before anything touches a GPU."""
    from .train_seg import score as run
    return run(args)


def postprocess(args):
    """Every refusal (no rule, a class outside --n_class, a negative volume, the connectivity, a missing or mis-typed prediction, --out equal to --pred)
    exits with its message in train_seg.postprocess_plan, before anything touches a GPU."""
    from .train_seg import postprocess as run
    return run(args)


def prepare(args):
    """Every refusal (regions, spacing, the normalisation's options, the manifest and its files) exits with its message in seg_prep.check_prepare,
    before anything touches a GPU."""
    from .seg_prep import run
    return run(args)


def restore(args):
    """Every refusal (--paint, a missing or mis-shaped prediction, a missing <case>_prep.npz, --out equal to --pred) exits with its message in
    seg_prep.check_restore, before anything touches a GPU."""
    from .seg_prep import run_restore
    return run_restore(args)


def _cleanup_options(p):
    p.add_argument("--keep_largest", default="", help="classes that keep only their largest connected component: 0,2 or `all`")
    p.add_argument("--min_voxels", type=int, default=0, help="every class loses its connected components of fewer voxels; 0 = off")
    p.add_argument("--connectivity", type=int, default=6, help="neighbours of a voxel: 6 (faces), 18 (and edges) or 26 (and corners)")


def build_parser():
    ap = argparse.ArgumentParser(description="3D segmentation fine-tuning of the PCRLv2 network (HIP kernels on MI355X)")
    sub = ap.add_subparsers(dest="command", required=True)
    tr = sub.add_parser("train", help="fine-tune (or train from scratch) the segmenter")
    tr.add_argument("--data", required=True, help="directory of cases (see the module docstring), or 'synthetic'")
    tr.add_argument("--phase", default="finetune", choices=("finetune", "scratch"))
    tr.add_argument("--weights", default="", help="3D pre-training checkpoint (--phase finetune)")
    tr.add_argument("--n_class", type=int, default=3, help="classes = bits of the label byte, 1..7")
    tr.add_argument("--head", default="sigmoid", help="sigmoid: overlapping regions, labels are bitmasks, Dice/BCE (the default) | softmax: 2..16 mutually "
                    "exclusive classes with the background as class 0, labels are label maps, Dice/cross-entropy")
    tr.add_argument("--wc", type=float, default=1.0, help="--head softmax: the weight of the cross-entropy term")
    tr.add_argument("--in_channels", type=int, default=1)
    tr.add_argument("--crop", default="64,64,32", help="training crop = evaluation patch, x,y,z, multiples of 8")
    tr.add_argument("--b", type=int, default=8, help="batch size PER PROCESS")
    tr.add_argument("--epochs", type=int, default=100, help="last epoch index (inclusive)")
    tr.add_argument("--lr", type=float, default=1e-2)
    tr.add_argument("--momentum", type=float, default=0.9)
    tr.add_argument("--weight_decay", type=float, default=1e-4)
    from . import optim_cli
    optim_cli.add_arguments(tr)
    tr.add_argument("--gpus", default="0", help="visible device ids, comma separated")
    tr.add_argument("--amp", action="store_true", help="bfloat16 activations and MFMA operands")
    tr.add_argument("--val_every", type=int, default=0, help="validation after every N-th epoch; 0 = every epoch")
    tr.add_argument("--save_best", action="store_true", help="write pcrlv2_seg3d_<phase>_1.0_best.pt whenever the mean validation Dice improves")
    tr.add_argument("--resume", default="", help="checkpoint to continue from (model, momentum buffers, epoch)")
    tr.add_argument("--output", default="./model_seg3d", help="checkpoint directory")
    tr.add_argument("--seed", type=int, default=42)
    tr.add_argument("--steps_per_epoch", type=int, default=0, help="batches per epoch; 0 = one crop per training case")
    tr.add_argument("--workers", type=int, default=4)
    tr.add_argument("--val_overlap", type=float, default=0.0, help="validation and the final test by sliding windows that overlap by this fraction of "
                    "the crop, blended (0..0.75); 0 = stride-tiled patches")
    tr.add_argument("--val_window", default="gaussian", help="blending window with --val_overlap > 0: gaussian | constant")
    tr.add_argument("--val_mirror", default="none", help="mirror test-time augmentation of validation and the final test: none | all | a subset of the "
                    "letters xyz; with --val_overlap 0 the sliding windows run with the constant window")
    tr.add_argument("--augment", action="store_true", help="resample the training crops on the device: rotation, zoom, gain, bias, gamma and noise at "
                    "the defaults of the --aug_* options; each of those implies it")
    tr.add_argument("--aug_rotate", default=None, help="largest rotation about each axis in degrees, 0..45 (15)")
    tr.add_argument("--aug_scale", default=None, help="LO,HI of the log-uniform isotropic zoom (0.8,1.25)")
    tr.add_argument("--aug_gain", default=None, help="LO,HI of the factor on a channel's intensities (0.75,1.25)")
    tr.add_argument("--aug_bias", default=None, help="a channel's intensities are shifted by a value in [-B, B] (0.1)")
    tr.add_argument("--aug_gamma", default=None, help="LO,HI of the log-uniform exponent of sign(v) |v|^gamma (0.7,1.5)")
    tr.add_argument("--aug_noise", default=None, help="largest standard deviation of the added Gaussian noise (0.1)")
    tr.add_argument("--aug_p_spatial", default=None, help="probability that a crop is rotated and zoomed (0.5)")
    tr.add_argument("--aug_p_intensity", default=None, help="probability, per channel, that its intensities are changed (0.15)")
    tr.set_defaults(model="pcrlv2", n="seg3d", ratio=1.0)
    pr = sub.add_parser("predict", help="write <case>_pred.npy (uint8 bitmask) for every case of a list")
    pr.add_argument("--data", required=True, help="directory with <case>_img.npy")
    pr.add_argument("--list", required=True, help="file of case names (in --data, or a path)")
    pr.add_argument("--weights", required=True, help="a checkpoint of `train`, or several separated by commas: their logits are averaged")
    pr.add_argument("--out", required=True, help="output directory")
    pr.add_argument("--crop", default="64,64,32", help="the crop the segmenter was trained on")
    pr.add_argument("--b", type=int, default=8, help="patches per forward")
    pr.add_argument("--amp", action="store_true")
    pr.add_argument("--gpu", type=int, default=0)
    pr.add_argument("--overlap", type=float, default=0.0, help="sliding windows that overlap by this fraction of the crop, blended (0..0.75); 0 = "
                    "stride-tiled patches, every voxel from one patch")
    pr.add_argument("--window", default="gaussian", help="blending window with --overlap > 0: gaussian | constant")
    pr.add_argument("--probs", action="store_true", help="with --overlap > 0, a --mirror or several --weights: also write <case>_prob.npy, float16 "
                    "[K, X, Y, Z]")
    pr.add_argument("--mirror", default="none", help="mirror test-time augmentation: none | all | a subset of the letters xyz; every patch is also shown "
                    "mirrored along each combination of these axes and the un-mirrored logits are averaged")
    _cleanup_options(pr)
    pp = sub.add_parser("postprocess", help="connected-component clean-up of stored <case>_pred.npy into another directory")
    pp.add_argument("--pred", required=True, help="directory with <case>_pred.npy (the --out of `predict`)")
    pp.add_argument("--list", required=True, help="file of case names (in --pred, or a path)")
    pp.add_argument("--out", required=True, help="output directory for the cleaned <case>_pred.npy; not --pred")
    pp.add_argument("--n_class", type=int, default=3, help="classes = bits of the mask byte, 1..7")
    pp.add_argument("--labelmap", action="store_true", help="the predictions are label maps (--head softmax); --n_class K counts the background, 2..16; "
                    "the background is never touched")
    _cleanup_options(pp)
    pp.add_argument("--gpu", type=int, default=0)
    sc = sub.add_parser("score", help="Dice, HD95, HD and ASSD of stored <case>_pred.npy against <case>_seg.npy")
    sc.add_argument("--data", required=True, help="directory with <case>_seg.npy (and, optionally, <case>_spacing.npy: three float64)")
    sc.add_argument("--list", required=True, help="file of case names (in --data, or a path)")
    sc.add_argument("--pred", required=True, help="directory with <case>_pred.npy (the --out of `predict`)")
    sc.add_argument("--n_class", type=int, default=3, help="classes = bits of the label byte, 1..7")
    sc.add_argument("--labelmap", action="store_true", help="ground truth and predictions are label maps (--head softmax); --n_class K counts the "
                    "background, 2..16; one row per (case, class 1..K-1)")
    sc.add_argument("--spacing", default="1,1,1", help="voxel size sx,sy,sz; a case's <case>_spacing.npy replaces it")
    sc.add_argument("--csv", default="", help="also write case,class,dice,hd95,hd,assd,n_pred,n_gt to this file")
    sc.add_argument("--gpu", type=int, default=0)
    pe = sub.add_parser("prepare", help="raw NIfTI / .npy volumes -> <case>_img.npy, <case>_seg.npy, <case>_spacing.npy, <case>_prep.npz")
    pe.add_argument("--data", required=True, help="directory the manifest's paths are relative to")
    pe.add_argument("--manifest", required=True, help="one case per line: name seg_path|- img_path [img_path ...]")
    pe.add_argument("--save", required=True, help="output directory (the --data of train / predict / score)")
    pe.add_argument("--regions", default=None, help="K = 1..7 sets of label values, bit k = set k: \"1,2,4;1,4;4\" (this or --classes)")
    pe.add_argument("--classes", default=None, help="1..15 DISJOINT sets of label values, set i = class index i + 1 of a label map (--head softmax), a value "
                    "in no set = background 0: \"1;2;3,4\"")
    pe.add_argument("--spacing", default="keep", help="target voxel size sx,sy,sz, or `keep`")
    pe.add_argument("--crop_nonzero", type=int, default=1, help="1: crop to the bounding box of the non-zero voxels and normalise over them; 0: neither")
    pe.add_argument("--norm", default="zscore", help="zscore | percentile | window | none")
    pe.add_argument("--percentiles", default=None, help="LO,HI of --norm percentile: clip to these percentiles of the case (0.5,99.5)")
    pe.add_argument("--window", default=None, help="LO,HI of --norm window: clip to this intensity window")
    pe.add_argument("--mean", type=float, default=None, help="--norm window: subtracted after the clip")
    pe.add_argument("--std", type=float, default=None, help="--norm window: divided by after the clip")
    pe.add_argument("--float16", action="store_true", help="write float16 images (half the disk; the loader reads either)")
    pe.add_argument("--split", default=None, help="train,val,test fractions: also write train.txt / val.txt / test.txt")
    pe.add_argument("--seed", type=int, default=None, help="seed of --split")
    pe.add_argument("--writers", type=int, default=4, help="file-writing threads (at most 16)")
    pe.add_argument("--gpu", type=int, default=0)
    rs = sub.add_parser("restore", help="<case>_pred.npy from the prepared grid back to the original grid")
    rs.add_argument("--prep", required=True, help="the --save of `prepare` (<case>_prep.npz)")
    rs.add_argument("--pred", required=True, help="directory with <case>_pred.npy on the prepared grid (the --out of `predict`)")
    rs.add_argument("--list", required=True, help="file of case names (in --prep, or a path)")
    rs.add_argument("--out", required=True, help="output directory; not --pred")
    rs.add_argument("--paint", default=None, help="also write <case>_label.npy: class k painted with the k-th value, later over earlier: \"2,1,4\"")
    rs.add_argument("--labelmap", action="store_true", help="the predictions are label maps (--head softmax): --paint v0,v1,.. gives the value of class "
                    "INDEX i, the background first")
    rs.add_argument("--nifti", action="store_true", help="also write .nii.gz with the stored header's geometry")
    rs.add_argument("--gpu", type=int, default=0)
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    return {"train": train, "predict": predict, "score": score, "postprocess": postprocess, "prepare": prepare, "restore": restore}[args.command](args)


if __name__ == "__main__":
    main(sys.argv[1:])
