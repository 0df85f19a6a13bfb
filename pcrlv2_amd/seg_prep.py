"""Preparation of raw 3D volumes into the cases `seg3d.py train / predict / score` read, and the way back to the scanner's grid.

    seg3d.py prepare --data RAW --manifest FILE --save DIR --regions "1,2,4;1,4;4" [--spacing sx,sy,sz | keep] [--crop_nonzero 1|0]
                     [--norm zscore|percentile|window|none] [--percentiles 0.5,99.5] [--window LO,HI --mean M --std S] [--float16]
                     [--split 0.7,0.1,0.2 --seed S]
    seg3d.py restore --prep DIR --pred PRED --list FILE --out OUT [--paint "2,1,4"] [--nifti]

Manifest: one case per line, `name seg_path|- img_path [img_path ...]`, paths relative to --data, `-` = unlabelled.  Inputs are NIfTI-1 single files
(pcrlv2_amd/nifti.py: no reorientation, qform / sform are carried, not applied) or `.npy` [X, Y, Z] in C order with the spacing in `<stem>_spacing.npy`
next to it (else 1, 1, 1).  All channels of a case share shape and spacing.  `--regions`: K = 1..7 sets of label values 0..255; bit k of the output byte
is set where the label is in set k (sets may overlap: BraTS's WT; TC; ET is "1,2,4;1,4;4").

Per case, on the device (csrc/seg_prep.hip; the volumes stay in disk order, x fastest, until the resample kernel transposes them):
  scan      bounding box of (any channel != 0), its voxel count, the number of non-finite values (any: the case is refused by name; an all-zero case
            is skipped with a message)
  select    --norm percentile: four exact order statistics per channel; the host forms the two percentiles with numpy's linear interpolation in
            float64 (`percentile_from_values`: equal to np.percentile(values.astype(float64), q))
  stats     --norm zscore | percentile: mean and population standard deviation per channel in float64 over the mask M (the non-zero union with
            --crop_nonzero 1, every voxel otherwise), of the values clipped to the percentiles where those are used
  resample  ONE launch: every channel normalised as (clip(v, lo, hi) - mean) / max(std, 1e-8), trilinear to the output grid (a corner outside M
            counts as 0 with --crop_nonzero 1), and the label volume by nearest neighbour through the 256-entry region table
The tables are the host's, float64: cc = (o + 0.5) * (n_in / n_out) - 0.5, clamped to [0, n_in - 1] for i0, i1, w0 = 1 - t, w1 = 1 - w0, and
nn = clamp(floor(cc + 0.5)); n_out = max(1, round(n_in * spacing_in / spacing_out)) with numpy's round -- scipy.ndimage.zoom(order=1 / 0,
mode='nearest', grid_mode=True).  One upload and one download per case; the box, the count and the selected values are the small read-backs the host
needs to size the output.

Outputs per case: `<case>_img.npy` [C, X, Y, Z] float32 / float16, `<case>_seg.npy` uint8 bitmask (all 0 for an unlabelled case), `<case>_spacing.npy`
(three float64: the spacing of the prepared grid, spacing_in * n_in / n_out), `<case>_prep.npz` (orig_shape, orig_spacing, box, prep_shape,
prep_spacing, stats [C][4] = mean, std, lo, hi as used, norm, crop_nonzero, header = the NIfTI header bytes of channel 0), and `cases.txt`; with
--split also train.txt / val.txt / test.txt by `luna_prep.stable_hash` of (seed, name): independent of the manifest's order.

`restore` takes `<case>_pred.npy` on the prepared grid back to the original one: nearest neighbour through the inverse tables inside the box, 0
outside; `--paint v0,v1,...` also writes `<case>_label.npy`, class k painted with v_k in order, later over earlier; `--nifti` writes `.nii.gz` with
the stored header's geometry.  DESIGN.md section 20.

Label maps: `prepare --classes "1;2;3,4"` instead of --regions writes <case>_seg.npy as a label map for --head softmax (set i ->
class index i + 1, a value in no set -> 0; a value in two sets is refused), `restore --labelmap --paint v0,v1,..` paints class INDEX i with v_i.  Both
are second builders of the kernels' 256-entry tables (class_table, labelmap_paint_table); the kernels are unchanged.
"""
from __future__ import annotations

import concurrent.futures as cf
import dataclasses
import os
import time

import numpy as np
import torch

from . import _lib, nifti
from .luna_prep import stable_hash

MAX_C, MAX_K = 16, 7
NORMS = ("zscore", "percentile", "window", "none")
BOX_EMPTY = 0x7FFFFFFF


class PrepError(ValueError):
    pass


# ---- options ----------------------------------------------------------------------------------------------------------------------
def _numbers(flag, text, n, conv=float):
    try:
        v = [conv(t) for t in str(text).split(",")]
    except ValueError:
        v = []
    if len(v) != n:
        raise SystemExit(f"{flag} {text}: {n} comma-separated numbers")
    return v


def parse_regions(text):
    """'1,2,4;1,4;4' -> [frozenset, ...]: K = 1..7 non-empty sets of label values 0..255."""
    sets = []
    for part in str(text).split(";"):
        try:
            vals = [int(t) for t in part.split(",")]
        except ValueError:
            raise SystemExit(f"--regions {text}: `{part}` is not a comma-separated list of integers") from None
        if not vals or any(v < 0 or v > 255 for v in vals):
            raise SystemExit(f"--regions {text}: every set holds label values 0..255")
        sets.append(frozenset(vals))
    if not 1 <= len(sets) <= MAX_K:
        raise SystemExit(f"--regions {text}: 1..{MAX_K} semicolon-separated sets (bit k of the label byte = set k; bit 7 means 'not counted')")
    return sets


def region_table(regions):
    """uint8 [256]: bit k of entry v is set where v is in set k."""
    tab = np.zeros(256, dtype=np.uint8)
    for k, s in enumerate(regions):
        for v in s:
            tab[v] |= np.uint8(1 << k)
    return tab


MAX_CLASSES = 16      # label maps (--classes, --labelmap): the classes of the softmax head, the background included


def parse_classes(text):
    """--classes '1;2;3,4' -> [frozenset, ...]: 1..15 non-empty, DISJOINT sets of label values 0..255; set i becomes class index i + 1 of a label map,
    a value in no set the background 0."""
    sets = []
    for part in str(text).split(";"):
        try:
            vals = [int(t) for t in part.split(",")]
        except ValueError:
            raise SystemExit(f"--classes {text}: `{part}` is not a comma-separated list of integers") from None
        if not vals or any(v < 0 or v > 255 for v in vals):
            raise SystemExit(f"--classes {text}: every set holds label values 0..255")
        for i, s in enumerate(sets):
            both = sorted(s & set(vals))
            if both:
                raise SystemExit(f"--classes {text}: label value {both[0]} is in set {i + 1} and in set {len(sets) + 1}; the classes of a label map are "
                                 "mutually exclusive (overlapping regions are --regions, with the sigmoid head)")
        sets.append(frozenset(vals))
    if not 1 <= len(sets) <= MAX_CLASSES - 1:
        raise SystemExit(f"--classes {text}: 1..{MAX_CLASSES - 1} semicolon-separated sets (set i = class i + 1 of the label map; 0 is the background)")
    return sets


def class_table(classes):
    """uint8 [256], the second builder of pcrl_segprep_resample's table: entry v is i + 1 where v is in set i, else 0 (the background)."""
    tab = np.zeros(256, dtype=np.uint8)
    for i, s in enumerate(classes):
        for v in s:
            tab[v] = np.uint8(i + 1)
    return tab


def parse_labelmap_paint(text):
    """--labelmap --paint 'v0,v1,..': the label value of class INDEX i, 2..16 values 0..255 (v0 paints the background)."""
    try:
        vals = [int(t) for t in str(text).split(",")]
    except ValueError:
        vals = []
    if not 2 <= len(vals) <= MAX_CLASSES or any(v < 0 or v > 255 for v in vals):
        raise SystemExit(f"--paint {text}: with --labelmap 2..{MAX_CLASSES} comma-separated label values 0..255, one per class index, the background first")
    return vals


def labelmap_paint_table(values):
    """uint8 [256], the second builder of pcrl_segprep_restore's paint table: entry i is v_i for a class index i < K, everything else 0."""
    tab = np.zeros(256, dtype=np.uint8)
    tab[:len(values)] = np.asarray(values, dtype=np.uint8)
    return tab


def parse_paint(text):
    """'2,1,4' -> [2, 1, 4]: the label value of class k, 1..7 values 0..255."""
    try:
        vals = [int(t) for t in str(text).split(",")]
    except ValueError:
        vals = []
    if not 1 <= len(vals) <= MAX_K or any(v < 0 or v > 255 for v in vals):
        raise SystemExit(f"--paint {text}: 1..{MAX_K} comma-separated label values 0..255, one per class")
    return vals


def paint_table(values):
    """uint8 [256]: the label of a mask byte -- 0, then class k's value for every set bit k in order, later over earlier."""
    tab = np.zeros(256, dtype=np.uint8)
    for m in range(256):
        for k, v in enumerate(values):
            if (m >> k) & 1:
                tab[m] = v
    return tab


def parse_spacing(text):
    """'keep' -> None; 'sx,sy,sz' -> three positive finite floats."""
    if str(text).strip().lower() == "keep":
        return None
    v = _numbers("--spacing", text, 3)
    if any(not (s > 0 and np.isfinite(s)) for s in v):
        raise SystemExit(f"--spacing {text}: three positive numbers, or `keep`")
    return tuple(v)


def parse_split(text):
    v = _numbers("--split", text, 3)
    if any(f < 0 for f in v) or abs(sum(v) - 1.0) > 1e-9:
        raise SystemExit(f"--split {text}: three non-negative fractions (train, val, test) that add up to 1")
    return tuple(v)


@dataclasses.dataclass
class PrepConfig:
    regions: list
    spacing: tuple | None = None          # None: keep
    crop_nonzero: bool = True
    norm: str = "zscore"
    percentiles: tuple = (0.5, 99.5)
    window: tuple | None = None           # (lo, hi)
    mean: float = 0.0
    std: float = 1.0
    float16: bool = False
    classes: list | None = None           # --classes: the label values become a LABEL MAP (class_table) and `regions` is empty


def parse_manifest(path, data_dir):
    """-> [(name, seg path or None, [image paths])]; refuses a malformed line, a duplicate name, a missing file and an unknown extension."""
    if not os.path.exists(path):
        raise SystemExit(f"{path}: no such manifest (one case per line: name seg_path|- img_path [img_path ...])")
    cases, seen = [], set()
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            tok = line.split()
            if not tok or tok[0].startswith("#"):
                continue
            if len(tok) < 3:
                raise SystemExit(f"{path}:{ln}: a case is `name seg_path|- img_path [img_path ...]`")
            name, seg, imgs = tok[0], tok[1], tok[2:]
            if name in seen:
                raise SystemExit(f"{path}:{ln}: case {name} appears twice")
            if len(imgs) > MAX_C:
                raise SystemExit(f"{path}:{ln}: case {name} has {len(imgs)} channels, at most {MAX_C}")
            seen.add(name)
            full = [None if seg == "-" else os.path.join(data_dir, seg)] + [os.path.join(data_dir, p) for p in imgs]
            for p in full:
                if p is None:
                    continue
                if not p.endswith((".nii", ".nii.gz", ".npy")):
                    raise SystemExit(f"{path}:{ln}: {p}: a volume is .nii, .nii.gz or .npy")
                if not os.path.exists(p):
                    raise SystemExit(f"{path}:{ln}: {p}: missing")
            cases.append((name, full[0], full[1:]))
    if not cases:
        raise SystemExit(f"{path}: no cases")
    if len({len(c[2]) for c in cases}) != 1:
        raise SystemExit(f"{path}: every case needs the same number of channels")
    return cases


def check_prepare(args):
    """Every refused combination exits with its message, before anything touches a GPU.  -> (PrepConfig, manifest, split or None)"""
    classes_arg = getattr(args, "classes", None)
    if (args.regions is None) == (classes_arg is None):
        raise SystemExit("prepare: exactly one of --regions \"1,2,4;1,4;4\" (overlapping regions -> a bitmask, the sigmoid head) and --classes \"1;2;3,4\" "
                         "(mutually exclusive classes -> a label map, --head softmax)")
    classes = parse_classes(classes_arg) if classes_arg is not None else None
    regions = parse_regions(args.regions) if classes is None else []
    spacing = parse_spacing(args.spacing)
    if args.crop_nonzero not in (0, 1):
        raise SystemExit(f"--crop_nonzero {args.crop_nonzero}: 1 or 0")
    if args.norm not in NORMS:
        raise SystemExit(f"--norm {args.norm}: one of {', '.join(NORMS)}")
    cfg = PrepConfig(regions=regions, spacing=spacing, crop_nonzero=bool(args.crop_nonzero), norm=args.norm, float16=bool(args.float16), classes=classes)
    if args.percentiles is not None and args.norm != "percentile":
        raise SystemExit("--percentiles belongs to --norm percentile")
    if args.norm == "percentile":
        lo, hi = _numbers("--percentiles", args.percentiles if args.percentiles is not None else "0.5,99.5", 2)
        if not 0 <= lo < hi <= 100:
            raise SystemExit(f"--percentiles {args.percentiles}: 0 <= LO < HI <= 100")
        cfg.percentiles = (lo, hi)
    given = [f for f in ("window", "mean", "std") if getattr(args, f) is not None]
    if args.norm == "window":
        if len(given) != 3:
            raise SystemExit("--norm window takes its numbers from the command line: --window LO,HI --mean M --std S (data-set-wide statistics are the "
                             "caller's)")
        lo, hi = _numbers("--window", args.window, 2)
        if not (lo < hi and np.isfinite(lo) and np.isfinite(hi)):
            raise SystemExit(f"--window {args.window}: LO < HI, both finite")
        if not (args.std > 0 and np.isfinite(args.std) and np.isfinite(args.mean)):
            raise SystemExit(f"--mean {args.mean} --std {args.std}: finite, --std positive")
        cfg.window, cfg.mean, cfg.std = (lo, hi), float(args.mean), float(args.std)
    elif given:
        raise SystemExit(f"--{given[0]} belongs to --norm window")
    split = None
    if args.split is not None:
        split = parse_split(args.split)
    elif args.seed is not None:
        raise SystemExit("--seed belongs to --split")
    if os.path.abspath(args.save) == os.path.abspath(args.data):
        raise SystemExit("--save must not be --data")
    if not os.path.isdir(args.data):
        raise SystemExit(f"--data {args.data}: no such directory")
    return cfg, parse_manifest(args.manifest, args.data), split


def check_restore(args):
    """-> (paint values or None, [(name, pred path, prep path)]); every refusal before anything touches a GPU."""
    from .data_seg import read_list
    if getattr(args, "labelmap", False):
        paint = parse_labelmap_paint(args.paint) if args.paint is not None else None
    else:
        paint = parse_paint(args.paint) if args.paint is not None else None
    if os.path.abspath(args.out) == os.path.abspath(args.pred):
        raise SystemExit("--out must not be --pred (both hold <case>_pred.npy)")
    plan = []
    for name in read_list(args.prep, args.list):
        pred, prep = os.path.join(args.pred, name + "_pred.npy"), os.path.join(args.prep, name + "_prep.npz")
        if not os.path.exists(prep):
            raise SystemExit(f"{prep}: missing (`seg3d.py prepare` writes it next to <case>_img.npy)")
        if not os.path.exists(pred):
            raise SystemExit(f"{pred}: missing (the prediction of a case is <case>_pred.npy, as `seg3d.py predict` writes it)")
        p = np.load(pred, mmap_mode="r")
        with np.load(prep) as meta:
            want = tuple(int(v) for v in meta["prep_shape"])
        if p.dtype != np.uint8 or tuple(p.shape) != want:
            raise SystemExit(f"{pred}: a prediction is a uint8 array of the prepared shape {want}, got {p.dtype} {p.shape}")
        plan.append((name, pred, prep))
    if not plan:
        raise SystemExit(f"{args.list}: no cases")
    return paint, plan


# ---- host arithmetic (float64; restated in tests/seg_prep_reference.py) ------------------------------------------------------------------
def n_out(n_in, spacing_in, spacing_out):
    """max(1, round(n_in * spacing_in / spacing_out)), numpy's round (half to even)."""
    return max(1, int(np.round(n_in * spacing_in / spacing_out)))


def axis_tables(n_in, n_o):
    """-> (i0, i1, nn int32 [n_o], w0, w1 float64 [n_o]) of scipy's zoom(mode='nearest', grid_mode=True) from n_in to n_o samples."""
    cc = (np.arange(n_o, dtype=np.float64) + 0.5) * (n_in / n_o) - 0.5
    c = np.clip(cc, 0.0, float(n_in - 1))
    f = np.floor(c)
    t = c - f
    i0 = f.astype(np.int32)
    i1 = np.minimum(i0 + 1, n_in - 1).astype(np.int32)
    w0 = 1.0 - t
    nn = np.clip(np.floor(cc + 0.5), 0, n_in - 1).astype(np.int32)
    return i0, i1, nn, w0, 1.0 - w0


def percentile_ranks(n, q):
    """numpy's 'linear' method: virtual index (n - 1) * (q / 100) -> (rank below, rank above, gamma)."""
    vi = (n - 1) * np.true_divide(q, 100)
    if vi >= n - 1:
        return n - 1, n - 1, 0.0
    lo = int(np.floor(vi))
    return lo, lo + 1, float(vi - lo)


def lerp(a, b, t):
    """numpy.lib._function_base_impl._lerp in float64, one operation at a time."""
    a, b, t = np.float64(a), np.float64(b), np.float64(t)
    d = b - a
    return b - d * (1.0 - t) if t >= 0.5 else a + d * t


def percentile_from_values(n, q, below, above):
    """The q-th percentile of n values whose order statistics at percentile_ranks(n, q) are `below` and `above` (float32 values, widened).  Zeros
    count as +0.0 (the device's select returns +0.0 for either sign)."""
    return lerp(np.float64(below) + 0.0, np.float64(above) + 0.0, percentile_ranks(n, q)[2])


def split_of(name, seed, fractions):
    """'train' | 'val' | 'test' from the stable hash of (seed, name): independent of the manifest's order and of the other cases."""
    u = stable_hash(f"{int(seed)}:{name}") / 2.0 ** 64
    return "train" if u < fractions[0] else "val" if u < fractions[0] + fractions[1] else "test"


# ---- GPU --------------------------------------------------------------------------------------------------------------------------
def _ws(nbytes, device):
    return torch.empty(max(8, int(nbytes)), dtype=torch.uint8, device=device)


def src_kind(t):
    if t.dtype == torch.int16:
        return 0
    if t.dtype == torch.float32:
        return 1
    raise _lib.PcrlError(f"a source volume is int16 or float32, got {t.dtype}")


def gpu_scan(src):
    """src device [C, Z, Y, X] -> rec int64 device [8] = x0, x1, y0, y1, z0, z1, count, non-finite (half-open box)."""
    C, Z, Y, X = src.shape
    rec = torch.empty(8, dtype=torch.int64, device=src.device)
    _lib.call_on_stream("pcrl_segprep_scan", src, src_kind(src), C, X, Y, Z, rec)
    return rec


def gpu_stats(src, use_mask, rec=None, clip=None):
    """-> stats float64 device [C, 2] = mean, population std over the mask (use_mask) or every voxel, of the values clipped to clip [C, 2]."""
    C, Z, Y, X = src.shape
    stats = torch.empty((C, 2), dtype=torch.float64, device=src.device)
    ws = _ws(_lib.lib().call("pcrl_segprep_stats_ws_bytes", C, X * Y * Z), src.device)
    _lib.call_on_stream("pcrl_segprep_stats", src, src_kind(src), C, X, Y, Z, int(bool(use_mask)), rec, clip, stats, ws, ws.numel())
    return stats


def gpu_select(src, ch, use_mask, ranks, out=None):
    """-> float32 device [4]: the order statistics of channel ch at the four 0-based ranks."""
    C, Z, Y, X = src.shape
    if out is None:
        out = torch.empty(4, dtype=torch.float32, device=src.device)
    ws = _ws(_lib.lib().call("pcrl_segprep_select_ws_bytes"), src.device)
    _lib.call_on_stream("pcrl_segprep_select", src, src_kind(src), C, ch, X, Y, Z, int(bool(use_mask)), *[int(r) for r in ranks], out, ws, ws.numel())
    return out


def resample_tables(box_shape, out_shape):
    """-> (tab_i int32 [3 (OX + OY + OZ)], tab_w float64 [2 (OX + OY + OZ)]) in the kernel's layout."""
    ti, tw = [], []
    for n, o in zip(box_shape, out_shape):
        i0, i1, nn, w0, w1 = axis_tables(n, o)
        ti += [i0, i1, nn]
        tw += [w0, w1]
    return np.concatenate(ti).astype(np.int32), np.concatenate(tw).astype(np.float64)


def gpu_resample(src, lab, box, out_shape, tab_i, tab_w, stats, clip, region, K, use_mask, img, out_lab):
    """One launch.  box = (x0, y0, z0, NX, NY, NZ); img device [C, OX, OY, OZ] float32 / float16; out_lab device uint8 [OX, OY, OZ]."""
    C, Z, Y, X = src.shape
    OX, OY, OZ = out_shape
    _lib.call_on_stream("pcrl_segprep_resample", src, src_kind(src), lab, C, X, Y, Z, *[int(b) for b in box], tab_i, tab_w, stats, clip, region, K,
                        int(bool(use_mask)), img, 1 if img.dtype == torch.float16 else 0, out_lab, OX, OY, OZ)


def resample_tile(NX, NZ, OX, OZ, use_mask):
    """-> (TX, TZ, LDS bytes): the output tile one block of the resample kernel takes for these box and output extents."""
    import ctypes
    tx, tz, nb = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
    L = _lib.lib()
    if L.cdll.pcrl_segprep_resample_tile(int(NX), int(NZ), int(OX), int(OZ), int(bool(use_mask)), ctypes.byref(tx), ctypes.byref(tz), ctypes.byref(nb)):
        raise _lib.PcrlError(L.last_error())
    return tx.value, tz.value, nb.value


def restore_tables(box_shape, prep_shape):
    """int32 [NX + NY + NZ]: the prepared index of every voxel of the box (nearest neighbour, the tables of prep -> box)."""
    return np.concatenate([axis_tables(p, n)[2] for n, p in zip(box_shape, prep_shape)]).astype(np.int32)


def gpu_restore(pred, tab, box, orig_shape, paint=None):
    """pred device uint8 [PX, PY, PZ] -> (out, painted or None) device uint8 [X, Y, Z]."""
    PX, PY, PZ = pred.shape
    X, Y, Z = orig_shape
    both = torch.empty((2 if paint is not None else 1, X, Y, Z), dtype=torch.uint8, device=pred.device)
    _lib.call_on_stream("pcrl_segprep_restore", pred, PX, PY, PZ, tab, *[int(b) for b in box], paint, both[0], both[1] if paint is not None else None, X, Y, Z)
    return both


# ---- one case ---------------------------------------------------------------------------------------------------------------------
def _tick(timing, key, t0, device=None):
    if timing is None:
        return t0
    if device is not None:
        torch.cuda.synchronize(device)
    t1 = time.perf_counter()
    timing[key] = timing.get(key, 0.0) + (t1 - t0)
    return t1


def prepare_case(channels, seg, spacing, cfg, device, name="case", timing=None):
    """channels: C arrays [Z, Y, X] (disk order), all int16 or any of them float32; seg: uint8 [Z, Y, X] of raw label values, or None; spacing
    (sx, sy, sz).  -> {'img' [C, X', Y', Z'], 'seg' uint8 [X', Y', Z'], 'spacing' float64 [3], 'meta' dict}, or None for an all-zero case.
    Raises PrepError (naming the case) for non-finite values and mismatched shapes."""
    C = len(channels)
    if not 1 <= C <= MAX_C:
        raise PrepError(f"{name}: {C} channels (1..{MAX_C})")
    shape = channels[0].shape
    if any(c.ndim != 3 or c.shape != shape for c in channels) or (seg is not None and seg.shape != shape):
        raise PrepError(f"{name}: the channels and the label volume do not share one shape: {[c.shape[::-1] for c in channels]}"
                        + (f", label {seg.shape[::-1]}" if seg is not None else ""))
    Z, Y, X = (int(s) for s in shape)
    V = X * Y * Z
    if V >= 2 ** 31:
        raise PrepError(f"{name}: {X} x {Y} x {Z} is 2^31 voxels or more")
    dt = np.int16 if all(c.dtype == np.int16 for c in channels) else np.float32
    es = np.dtype(dt).itemsize
    t0 = time.perf_counter()
    host = np.empty(C * V * es + (V if seg is not None else 0), dtype=np.uint8)
    hv = host[:C * V * es].view(dt).reshape(C, Z, Y, X)
    for c, a in enumerate(channels):
        hv[c] = a
    if seg is not None:
        host[C * V * es:] = np.asarray(seg, dtype=np.uint8).reshape(-1)
    t0 = _tick(timing, "pack", t0)
    dev = torch.from_numpy(host).to(device)                                           # the one upload
    src = dev[:C * V * es].view(torch.int16 if dt == np.int16 else torch.float32).view(C, Z, Y, X)
    lab = dev[C * V * es:] if seg is not None else None
    t0 = _tick(timing, "upload", t0, device)

    rec_d = gpu_scan(src)
    rec = rec_d.cpu().numpy()                                                          # small read-back: the box sizes the output
    t0 = _tick(timing, "scan", t0, device)
    if rec[7]:
        raise PrepError(f"{name}: {int(rec[7])} non-finite values (NaN or inf) in the image channels")
    if rec[1] == 0:
        return None
    use_mask = bool(cfg.crop_nonzero)
    box = (int(rec[0]), int(rec[2]), int(rec[4]), int(rec[1] - rec[0]), int(rec[3] - rec[2]), int(rec[5] - rec[4])) if use_mask else (0, 0, 0, X, Y, Z)
    n = int(rec[6]) if use_mask else V

    used = np.zeros((C, 4), dtype=np.float64)
    used[:, 1], used[:, 2], used[:, 3] = 1.0, -np.inf, np.inf
    clip_d = stats_d = None
    if cfg.norm == "percentile":
        ranks = percentile_ranks(n, cfg.percentiles[0])[:2] + percentile_ranks(n, cfg.percentiles[1])[:2]
        sel = torch.empty((C, 4), dtype=torch.float32, device=device)
        for c in range(C):
            gpu_select(src, c, use_mask, ranks, out=sel[c])
        vals = sel.cpu().numpy()                                                       # small read-back: the host interpolates in float64
        for c in range(C):
            used[c, 2] = percentile_from_values(n, cfg.percentiles[0], vals[c, 0], vals[c, 1])
            used[c, 3] = percentile_from_values(n, cfg.percentiles[1], vals[c, 2], vals[c, 3])
        clip_d = torch.from_numpy(np.ascontiguousarray(used[:, 2:4])).to(device)
        t0 = _tick(timing, "select", t0, device)
    elif cfg.norm == "window":
        used[:, 0], used[:, 1], used[:, 2], used[:, 3] = cfg.mean, cfg.std, cfg.window[0], cfg.window[1]
        clip_d = torch.from_numpy(np.ascontiguousarray(used[:, 2:4])).to(device)
        stats_d = torch.from_numpy(np.ascontiguousarray(used[:, 0:2])).to(device)
    if cfg.norm in ("zscore", "percentile"):
        stats_d = gpu_stats(src, use_mask, rec_d, clip_d)                              # stays on the device for the resample
        t0 = _tick(timing, "stats", t0, device)

    sp_in = tuple(float(s) for s in spacing)
    sp_t = sp_in if cfg.spacing is None else cfg.spacing
    out_shape = tuple(n_out(nb, si, so) for nb, si, so in zip(box[3:], sp_in, sp_t))
    OV = out_shape[0] * out_shape[1] * out_shape[2]
    if OV >= 2 ** 31:
        raise PrepError(f"{name}: the prepared grid {out_shape} has 2^31 voxels or more")
    tab_i, tab_w = resample_tables(box[3:], out_shape)
    # the kernel maps label bytes through ONE 256-entry table; K reaches it only to be checked, so a label-map table travels as one "region"
    table, k_dev = (class_table(cfg.classes), 1) if cfg.classes else (region_table(cfg.regions), len(cfg.regions))
    tabs = np.concatenate([tab_w.view(np.uint8), tab_i.view(np.uint8), table])
    tabs_d = torch.from_numpy(tabs).to(device)
    tw_d = tabs_d[:tab_w.nbytes].view(torch.float64)
    ti_d = tabs_d[tab_w.nbytes:tab_w.nbytes + tab_i.nbytes].view(torch.int32)
    reg_d = tabs_d[tab_w.nbytes + tab_i.nbytes:]
    odt, oes = (torch.float16, 2) if cfg.float16 else (torch.float32, 4)
    out_d = torch.empty(C * OV * oes + OV, dtype=torch.uint8, device=device)
    img_d = out_d[:C * OV * oes].view(odt).view(C, *out_shape)
    lab_d = out_d[C * OV * oes:].view(*out_shape)
    gpu_resample(src, lab, box, out_shape, ti_d, tw_d, stats_d, clip_d, reg_d, k_dev, use_mask, img_d, lab_d)
    t0 = _tick(timing, "resample", t0, device)
    out = out_d.cpu().numpy()                                                          # the one download
    if stats_d is not None and cfg.norm != "window":
        used[:, 0:2] = stats_d.cpu().numpy()
    t0 = _tick(timing, "download", t0, device)
    img = out[:C * OV * oes].view(np.float16 if cfg.float16 else np.float32).reshape(C, *out_shape)
    prep_spacing = np.array([si * nb / o for si, nb, o in zip(sp_in, box[3:], out_shape)], dtype=np.float64)
    meta = {"orig_shape": np.array([X, Y, Z], dtype=np.int64), "orig_spacing": np.array(sp_in, dtype=np.float64),
            "box": np.array([box[0], box[0] + box[3], box[1], box[1] + box[4], box[2], box[2] + box[5]], dtype=np.int64),
            "prep_shape": np.array(out_shape, dtype=np.int64), "prep_spacing": prep_spacing, "stats": used,
            "norm": np.array(cfg.norm), "crop_nonzero": np.array(int(use_mask), dtype=np.int64)}
    return {"img": img, "seg": out[C * OV * oes:].reshape(out_shape), "spacing": prep_spacing, "meta": meta}


def restore_case(pred, meta, device, paint=None, labelmap=False):
    """pred uint8 [X', Y', Z'] on the prepared grid, meta as prepare_case wrote it -> (mask uint8 [X, Y, Z] on the original grid, label map or None)."""
    prep_shape = tuple(int(v) for v in meta["prep_shape"])
    pred = np.ascontiguousarray(pred)
    if pred.dtype != np.uint8 or pred.shape != prep_shape:
        raise PrepError(f"a prediction is a uint8 array of the prepared shape {prep_shape}, got {pred.dtype} {pred.shape}")
    b = [int(v) for v in meta["box"]]
    box = (b[0], b[2], b[4], b[1] - b[0], b[3] - b[2], b[5] - b[4])
    orig = tuple(int(v) for v in meta["orig_shape"])
    tab = restore_tables(box[3:], prep_shape)
    painter = labelmap_paint_table if labelmap else paint_table
    parts = [tab.view(np.uint8)] + ([painter(paint)] if paint is not None else []) + [pred.reshape(-1)]
    up = torch.from_numpy(np.concatenate(parts)).to(device)                            # one upload
    tab_d = up[:tab.nbytes].view(torch.int32)
    off = tab.nbytes + (256 if paint is not None else 0)
    paint_d = up[tab.nbytes:off] if paint is not None else None
    both = gpu_restore(up[off:].view(*prep_shape), tab_d, box, orig, paint_d).cpu().numpy()      # one download
    return both[0], (both[1] if paint is not None else None)


# ---- files ------------------------------------------------------------------------------------------------------------------------
def load_volume(path):
    """-> (volume [Z, Y, X] disk order in its stored type (scaled where the header scales), spacing (sx, sy, sz), NIfTI header bytes or None)"""
    if path.endswith(".npy"):
        a = np.load(path)
        if a.ndim != 3:
            raise PrepError(f"{path}: expected [X, Y, Z], got shape {a.shape}")
        sp = path[:-4] + "_spacing.npy"
        spacing = tuple(float(v) for v in np.load(sp).reshape(-1)) if os.path.exists(sp) else (1.0, 1.0, 1.0)
        if len(spacing) != 3 or any(not (s > 0 and np.isfinite(s)) for s in spacing):
            raise PrepError(f"{sp}: three positive numbers expected")
        return np.ascontiguousarray(a.transpose(2, 1, 0)), spacing, None
    vol, spacing, hdr = nifti.read_nifti(path, raw_values=True)
    return vol, spacing, hdr


def as_channel(vol):
    """int16 stays; every other type becomes float32 (from float64 where the file scaled: one rounding)."""
    return vol if vol.dtype == np.int16 else vol.astype(np.float32)


def as_labels(vol, path):
    """Raw label values as uint8; refuses anything that is not an integer in 0..255."""
    if vol.dtype.kind == "f":
        if not np.all(vol == np.floor(vol)):
            raise PrepError(f"{path}: label values must be integers")
    if vol.size and (vol.min() < 0 or vol.max() > 255):
        raise PrepError(f"{path}: label values outside 0..255 ({vol.min()} .. {vol.max()})")
    return vol.astype(np.uint8)


def read_case(entry):
    """(name, seg path or None, image paths) -> (channels, seg or None, spacing, header bytes or None); PrepError names the case."""
    name, seg_path, img_paths = entry
    try:
        vols = [load_volume(p) for p in img_paths]
        seg = load_volume(seg_path) if seg_path else None
    except (OSError, ValueError) as e:      # NiftiError and PrepError are ValueErrors
        raise PrepError(f"{name}: {e}") from e
    shape, spacing = vols[0][0].shape, vols[0][1]
    for (v, sp, _), p in list(zip(vols, img_paths)) + ([(seg, seg_path)] if seg else []):
        if v.shape != shape:
            raise PrepError(f"{name}: {p} has shape {v.shape[::-1]}, channel 0 has {shape[::-1]}")
        if not np.allclose(sp, spacing, rtol=1e-5, atol=0):
            raise PrepError(f"{name}: {p} has spacing {sp}, channel 0 has {spacing}")
    return [as_channel(v) for v, _, _ in vols], (as_labels(seg[0], seg_path) if seg else None), spacing, vols[0][2]


def save_case(save_dir, name, res, header):
    np.save(os.path.join(save_dir, name + "_img.npy"), res["img"])
    np.save(os.path.join(save_dir, name + "_seg.npy"), res["seg"])
    np.save(os.path.join(save_dir, name + "_spacing.npy"), res["spacing"])
    hdr = np.frombuffer(header, dtype=np.uint8) if header is not None else np.zeros(0, dtype=np.uint8)
    with open(os.path.join(save_dir, name + "_prep.npz"), "wb") as f:
        np.savez(f, header=hdr, **res["meta"])


def _write_list(path, names):
    with open(path, "w") as f:
        f.write("".join(n + "\n" for n in names))


def run(args, log=print):
    """`seg3d.py prepare`.  -> {"cases": [names written], "skipped": [(name, reason)]}"""
    cfg, manifest, split = check_prepare(args)
    device = torch.device("cuda", args.gpu)
    torch.cuda.set_device(device)
    os.makedirs(args.save, exist_ok=True)
    result = {"cases": [], "skipped": []}
    writers = max(1, min(16, args.writers))
    with cf.ThreadPoolExecutor(1) as reader, cf.ThreadPoolExecutor(writers) as writer:
        pending = []
        nxt = reader.submit(read_case, manifest[0])
        for i, entry in enumerate(manifest):
            name = entry[0]
            try:
                channels, seg, spacing, header = nxt.result()
                err = None
            except PrepError as e:
                err = e
            nxt = reader.submit(read_case, manifest[i + 1]) if i + 1 < len(manifest) else None      # parsed while the device works
            if err is not None:
                raise SystemExit(f"[seg_prep] {err}")
            try:
                res = prepare_case(channels, seg, spacing, cfg, device, name)
            except PrepError as e:
                raise SystemExit(f"[seg_prep] {e}") from e
            if res is None:
                log(f"[seg_prep] skip {name}: every voxel of every channel is 0")
                result["skipped"].append((name, "all zero"))
                continue
            pending.append(writer.submit(save_case, args.save, name, res, header))
            result["cases"].append(name)
            log(f"[seg_prep] {name}: {tuple(int(v) for v in res['meta']['orig_shape'])} -> {res['img'].shape}, spacing "
                + ",".join("%g" % s for s in res["spacing"]))
            while len(pending) > 2 * writers:      # bound the host memory held by queued writes
                pending.pop(0).result()
        for p in pending:
            p.result()
    _write_list(os.path.join(args.save, "cases.txt"), result["cases"])
    if split is not None:
        parts = {"train": [], "val": [], "test": []}
        for name in result["cases"]:
            parts[split_of(name, args.seed if args.seed is not None else 0, split)].append(name)
        for k, names in parts.items():
            _write_list(os.path.join(args.save, k + ".txt"), sorted(names))
    log(f"[seg_prep] {len(result['cases'])} cases written to {args.save}, {len(result['skipped'])} skipped")
    return result


def run_restore(args, log=print):
    """`seg3d.py restore`.  -> the case names written"""
    paint, plan = check_restore(args)
    device = torch.device("cuda", args.gpu)
    torch.cuda.set_device(device)
    os.makedirs(args.out, exist_ok=True)
    for name, pred_path, prep_path in plan:
        with np.load(prep_path) as z:
            meta = {k: z[k] for k in z.files}
        mask, label = restore_case(np.load(pred_path), meta, device, paint, labelmap=bool(getattr(args, "labelmap", False)))
        np.save(os.path.join(args.out, name + "_pred.npy"), mask)
        if label is not None:
            np.save(os.path.join(args.out, name + "_label.npy"), label)
        if args.nifti:
            hdr = meta["header"].tobytes() if meta["header"].size else None
            for a, suffix in ((mask, "_pred.nii.gz"), (label, "_label.nii.gz")):
                if a is not None:
                    nifti.write_nifti(os.path.join(args.out, name + suffix), np.ascontiguousarray(a.transpose(2, 1, 0)),
                                      spacing=tuple(float(s) for s in meta["orig_spacing"]), header=hdr)
        log(f"[seg_prep] {name}: {mask.shape}")
    log(f"[seg_prep] {len(plan)} masks restored to {args.out}")
    return [p[0] for p in plan]
