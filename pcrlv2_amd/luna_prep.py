"""LUNA16 pre-processing: raw CT series (`subset<f>/*.mhd`) -> the pre-task directory that pcrlv2_amd/data.py reads.

Reference: `luna_preprocess.py:134-348` (load_sitk_with_resample, infinite_generator_from_one_volume, crop_pair, cal_iou).  Per series:
  read + resample  MetaImage read here (no SimpleITK), ITK's linear resample to 1 mm on the GPU (`pcrl_prep_resample`), kept int16
  crop pairs       `scale` pairs, each from a rejection loop: two global sizes from `col_size`, start positions, IoU > 0.3, crop
                   (rows, cols, deps + 3), skimage's resize to (64, 64, 35) unless (64, 64, 32), the depth-map test on window 1's sizes,
                   six local windows from the union of the two boxes +- 3 (truncated at the volume edge) resized to 16^3
  output           `<save>/subset<f>/<name>_global_<k>.npy` [2, 64, 64, 32] and `<name>_local_<k>.npy` [6, 16, 16, 16], float64, C order

The draws follow the reference's rules and ranges (inclusive `random.randint` for the global starts, exclusive `np.random.randint` for the
sizes and the local windows) from a numpy Generator keyed on (seed, stable hash of the series name, pair k, attempt j): the output does not
depend on how many attempts one launch evaluates, on the fold grouping or on the process count.  Up to K attempts (`--attempts-per-launch`;
a pair's first launch takes one, each further launch twice as many) are normalised, filtered, zoomed and scored in one `pcrl_prep_windows`
launch and the first accepted one is kept.  Deviations from the reference,
all where it crashes or never ends: at most MAX_ATTEMPTS attempts per pair and IOU_BLOCKS * IOU_BLOCK IoU candidates per attempt; a series that
exhausts the attempts, or draws a size whose start range is empty (the reference raises ValueError there), is skipped with a message; a
volume shorter than 98 mm is padded at the end of z with HU -1000 to 99 mm (what the reference's `np.pad(img, [0, 0, -pad + 1])` means; as
written it cannot broadcast).  See DESIGN.md section 10.2.
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import hashlib
import os
import sys
import time

import numpy as np
import torch

from . import _lib

HU_MIN, HU_MAX = -1000.0, 1000.0
HU_THRED = (-150.0 - HU_MIN) / (HU_MAX - HU_MIN)       # luna_preprocess.py:66
LUNG_MAX = 0.15
LEN_BORDER, LEN_BORDER_Z, LEN_DEPTH = 70, 15, 3
COL_SIZE = np.array([(96, 96, 64), (96, 96, 96), (112, 112, 64), (64, 64, 32)], dtype=np.int64)
LOCAL_COL_SIZE = np.array([(32, 32, 16), (16, 16, 16), (32, 32, 32), (8, 8, 8)], dtype=np.int64)
INPUT = (64, 64, 32)
LOCAL_INPUT = (16, 16, 16)
N_LOCAL = 6
MAX_ATTEMPTS = 1024          # depth-map attempts per pair before the series is skipped
IOU_BLOCK, IOU_BLOCKS = 256, 64   # IoU candidates are drawn 256 at a time; 16384 without IoU > 0.3 make a rejected attempt
GLOBAL_ELEMS = INPUT[0] * INPUT[1] * INPUT[2]
LOCAL_ELEMS = LOCAL_INPUT[0] * LOCAL_INPUT[1] * LOCAL_INPUT[2]
ATTEMPT_ELEMS = 2 * GLOBAL_ELEMS + N_LOCAL * LOCAL_ELEMS
NREC, NPRM, RMAX = 16, 32, 8     # PCRL_PREP_NREC / NPRM / RMAX of pcrl_hip.h


# ---- MetaImage ------------------------------------------------------------------------------------------------------------------
class MetaImageError(ValueError):
    pass


def read_metaimage(path):
    """-> (volume int16 [z, y, x], spacing (x, y, z), header dict).  MET_SHORT, uncompressed, one data file: anything else raises."""
    hdr = {}
    with open(path, "r", errors="replace") as f:
        for line in f:
            if "=" not in line:
                continue
            k, v = line.split("=", 1)
            hdr[k.strip()] = v.strip()
            if k.strip() == "ElementDataFile":
                break                    # the tag ends the header
    ndims = int(hdr.get("NDims", "0"))
    if ndims != 3:
        raise MetaImageError(f"{path}: NDims = {hdr.get('NDims')} (3 is supported)")
    et = hdr.get("ElementType")
    if et != "MET_SHORT":
        raise MetaImageError(f"{path}: ElementType = {et} (MET_SHORT is supported)")
    if hdr.get("CompressedData", "False").lower() == "true":
        raise MetaImageError(f"{path}: CompressedData = True (uncompressed data is supported)")
    df = hdr.get("ElementDataFile")
    if df is None or df.split()[0] in ("LIST", "LOCAL") or "%" in df:
        raise MetaImageError(f"{path}: ElementDataFile = {df} (one raw data file is supported)")
    size = [int(v) for v in hdr["DimSize"].split()]
    spacing = [float(v) for v in hdr.get("ElementSpacing", hdr.get("ElementSize", "1 1 1")).split()]
    if len(size) != 3 or len(spacing) != 3:
        raise MetaImageError(f"{path}: DimSize / ElementSpacing need 3 values")
    hdr["Offset"] = [float(v) for v in hdr.get("Offset", hdr.get("Origin", hdr.get("Position", "0 0 0"))).split()]
    hdr["TransformMatrix"] = [float(v) for v in hdr.get("TransformMatrix", "1 0 0 0 1 0 0 0 1").split()]
    msb = hdr.get("BinaryDataByteOrderMSB", hdr.get("ElementByteOrderMSB", "False")).lower() == "true"
    raw = os.path.join(os.path.dirname(os.path.abspath(path)), df)
    n = size[0] * size[1] * size[2]
    vol = np.fromfile(raw, dtype=">i2" if msb else "<i2", count=n)
    if vol.size != n:
        raise MetaImageError(f"{raw}: {vol.size} voxels, DimSize says {n}")
    return vol.astype(np.int16, copy=False).reshape(size[2], size[1], size[0]), tuple(spacing), hdr


def write_metaimage(path, vol_zyx, spacing, offset=(0.0, 0.0, 0.0)):
    """Write an int16 [z, y, x] volume as <path> (.mhd) + <stem>.raw (tests and probes)."""
    raw = os.path.splitext(os.path.basename(path))[0] + ".raw"
    Z, Y, X = vol_zyx.shape
    with open(path, "w") as f:
        f.write("ObjectType = Image\nNDims = 3\nBinaryData = True\nBinaryDataByteOrderMSB = False\nCompressedData = False\n"
                "TransformMatrix = 1 0 0 0 1 0 0 0 1\n" f"Offset = {offset[0]} {offset[1]} {offset[2]}\n"
                "CenterOfRotation = 0 0 0\nAnatomicalOrientation = RAI\n" f"ElementSpacing = {spacing[0]} {spacing[1]} {spacing[2]}\n"
                f"DimSize = {X} {Y} {Z}\nElementType = MET_SHORT\nElementDataFile = {raw}\n")
    np.ascontiguousarray(vol_zyx, dtype="<i2").tofile(os.path.join(os.path.dirname(os.path.abspath(path)), raw))


def resample_size(size_xyz, spacing_xyz):
    """luna_preprocess.py:335-337: int(size * spacing / 1 + 0.5) per axis."""
    return tuple(int(n * s / 1 + 0.5) for n, s in zip(size_xyz, spacing_xyz))


def padded_depth(size_z):
    """luna_preprocess.py:157-166: a volume with size_z - 64 - 3 - 1 - 15 < 15 gets -pad + 1 slices of 0 (normalised) at the end of z."""
    if size_z - 64 - LEN_DEPTH - 1 - LEN_BORDER_Z < LEN_BORDER_Z:
        pad = size_z - 64 - LEN_DEPTH - 1 - LEN_BORDER_Z - LEN_BORDER_Z
        return size_z + (-pad + 1)
    return size_z


# ---- draws ----------------------------------------------------------------------------------------------------------------------
def stable_hash(name: str) -> int:
    return int.from_bytes(hashlib.blake2b(name.encode(), digest_size=8).digest(), "little")


def attempt_rng(seed: int, name_hash: int, k: int, j: int):
    return np.random.default_rng([seed, name_hash, k, j])


class Draw:
    """One attempt: kind "ok" (boxes, pre-resize sizes, local windows), "empty" (a start range is empty on `axis`) or "none" (no IoU > 0.3)."""
    __slots__ = ("kind", "axis", "box1", "box2", "size1", "size2", "locals")

    def __init__(self, kind, axis=None, box1=None, box2=None, size1=None, size2=None, locs=None):
        self.kind, self.axis, self.box1, self.box2, self.size1, self.size2, self.locals = kind, axis, box1, box2, size1, size2, locs


def draw_attempt(rng, shape):
    """The reference's crop_pair draws (luna_preprocess.py:167-191, 251-268) for a padded (x, y, z) volume shape."""
    sx, sy, sz = shape
    for _ in range(IOU_BLOCKS):
        i1 = rng.integers(0, len(COL_SIZE), IOU_BLOCK)
        i2 = rng.integers(0, len(COL_SIZE), IOU_BLOCK)
        cand = []
        for ii in (i1, i2):
            r, c, d = (COL_SIZE[ii, a].copy() for a in range(3))
            shrink = sx - r - 1 - LEN_BORDER <= LEN_BORDER          # only size_x is tested, for rows and cols (:172-177)
            r[shrink] -= 32
            c[shrink] -= 32
            cand.append((r, c, d))
        lohi = []
        for r, c, d in cand:
            lohi += [(LEN_BORDER, sx - r - 1 - LEN_BORDER), (LEN_BORDER, sy - c - 1 - LEN_BORDER),
                     (LEN_BORDER_Z, sz - d - LEN_DEPTH - 1 - LEN_BORDER_Z)]
        st = [rng.integers(lo, np.maximum(hi, lo) + 1) for lo, hi in lohi]     # random.randint: inclusive
        empty = np.zeros(IOU_BLOCK, dtype=bool)
        first_axis = np.full(IOU_BLOCK, -1)
        for a, (lo, hi) in enumerate(lohi):
            e = hi < lo
            first_axis[e & ~empty] = a % 3
            empty |= e
        (r1, c1, d1), (r2, c2, d2) = cand
        b1 = (st[0], st[0] + r1, st[1], st[1] + c1, st[2], st[2] + d1)
        b2 = (st[3], st[3] + r2, st[4], st[4] + c2, st[5], st[5] + d2)
        s1 = r1 * c1 * d1
        s2 = r2 * c2 * d2
        ov = [np.maximum(0, np.minimum(b1[q + 1], b2[q + 1]) - np.maximum(b1[q], b2[q])) for q in (0, 2, 4)]
        area = ov[0] * ov[1] * ov[2]
        iou = area / (s1 + s2 - area)
        hit = np.flatnonzero(empty | (iou > 0.3))
        if hit.size == 0:
            continue
        n = int(hit[0])
        if empty[n]:
            return Draw("empty", axis="xyz"[int(first_axis[n])])
        box1 = tuple(int(v[n]) for v in b1)
        box2 = tuple(int(v[n]) for v in b2)
        lo = [max(min(box1[q], box2[q]) - 3, 0) for q in (0, 2, 4)]
        hi = [min(max(box1[q + 1], box2[q + 1]) + 3, s) for q, s in zip((0, 2, 4), shape)]
        lx = rng.integers(lo[0], hi[0], N_LOCAL)        # np.random.randint: exclusive
        ly = rng.integers(lo[1], hi[1], N_LOCAL)
        lz = rng.integers(lo[2], hi[2], N_LOCAL)
        li = rng.integers(0, len(LOCAL_COL_SIZE), N_LOCAL)
        locs = []
        for q in range(N_LOCAL):
            start = (int(lx[q]), int(ly[q]), int(lz[q]))
            locs.append((start, tuple(min(s0 + int(n0), s) - s0 for s0, n0, s in zip(start, LOCAL_COL_SIZE[li[q]], shape))))
        return Draw("ok", box1=box1, box2=box2, size1=(int(r1[n]), int(c1[n]), int(d1[n])), size2=(int(r2[n]), int(c2[n]), int(d2[n])),
                    locs=locs)
    return Draw("none")


def rejected(score1, score2, size1):
    """luna_preprocess.py:245-249 with the exact scores 2 * sum(d_img); window 1's sizes for both tests (the reference's quirk)."""
    rows1, cols1, deps1 = size1
    lim = LUNG_MAX * cols1 * deps1 * rows1
    return score1 / 2 > lim or score2 / 2 > lim


class SeriesSkipped(Exception):
    pass


def series_pairs(shape, name, seed, scale, attempts_per_launch, evaluate, max_attempts=MAX_ATTEMPTS, stats=None):
    """Yields (k, payload) for pair k = 0 .. scale-1 of one series.  `evaluate(draws)` -> (index of the first accepted draw or -1, payload)
    runs a batch of "ok" draws (1, 2, 4, ... up to `attempts_per_launch` per launch: most pairs are accepted at their first attempt); the
    attempts are visited in order, so the result does not depend on the batch sizes.  Raises
    SeriesSkipped when a pair exhausts `max_attempts` or an attempt draws an empty start range."""
    h = stable_hash(name)
    for k in range(scale):
        j = 0
        width = 1          # the first launch of a pair evaluates one attempt, each further launch twice as many, up to attempts_per_launch
        while True:
            batch, stop = [], None
            while len(batch) < width and j < max_attempts:
                d = draw_attempt(attempt_rng(seed, h, k, j), shape)
                j += 1
                if d.kind == "empty":
                    stop = d
                    break
                if d.kind == "ok":
                    batch.append((j - 1, d))
            first, payload = evaluate([d for _, d in batch]) if batch else (-1, None)
            if stats is not None:
                stats["launches"] = stats.get("launches", 0) + (1 if batch else 0)
            if first >= 0:
                if stats is not None:
                    stats["attempts"] = stats.get("attempts", 0) + batch[first][0] + 1
                    stats["pairs"] = stats.get("pairs", 0) + 1
                yield k, payload
                break
            if stop is not None:
                raise SeriesSkipped(f"pair {k}, attempt {j - 1}: empty start range on axis {stop.axis} for volume {tuple(shape)} "
                                    "(the reference raises ValueError here)")
            if j >= max_attempts:
                raise SeriesSkipped(f"pair {k}: no accepted crop pair in {max_attempts} attempts")
            width = min(2 * width, attempts_per_launch)


# ---- window records -------------------------------------------------------------------------------------------------------------
def gaussian_weights(sigma):
    """scipy's _gaussian_kernel1d(sigma, 0, int(4 * sigma + 0.5)) -> (radius, weights of taps 0..radius)."""
    radius = int(4.0 * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return radius, phi[radius:]


def window_record(start, src, out_shape, out_off, store_depth, ws_off, score_depth):
    """-> (int64 record, float64 parameters) of one window: skimage's resize(src -> out_shape) as sigmas, radii, weights and zoom ratios."""
    rec = np.zeros(NREC, dtype=np.int64)
    prm = np.zeros(NPRM, dtype=np.float64)
    rec[0:3], rec[3:6], rec[6:9] = start, src, out_shape
    rec[12], rec[13], rec[14], rec[15] = out_off, store_depth, ws_off, score_depth
    if any(o < i for i, o in zip(src, out_shape)):            # anti_aliasing default: any axis shrinks
        for a, (i, o) in enumerate(zip(src, out_shape)):
            s = max(0.0, (i / o - 1) / 2)
            if s > 1e-15:
                r, w = gaussian_weights(s)
                if r > RMAX:
                    raise ValueError(f"Gaussian radius {r} > {RMAX} for {src} -> {out_shape}")
                rec[9 + a] = r
                prm[a * (RMAX + 1):a * (RMAX + 1) + r + 1] = w
    prm[3 * (RMAX + 1):3 * (RMAX + 1) + 3] = [i / o for i, o in zip(src, out_shape)]
    return rec, prm


def attempt_windows(d):
    """-> [(start, src size, out shape, store depth, score depth)] * 8: the two globals, then the six locals of one draw."""
    ws = []
    for b, s in ((d.box1, d.size1), (d.box2, d.size2)):
        ws.append(((b[0], b[2], b[4]), (s[0], s[1], s[2] + LEN_DEPTH), (INPUT[0], INPUT[1], INPUT[2] + LEN_DEPTH), INPUT[2], INPUT[2]))
    for start, n in d.locals:
        ws.append((start, n, LOCAL_INPUT, LOCAL_INPUT[2], 0))
    return ws


def build_records(draws):
    """-> (rec [W, NREC] int64, prm [W, NPRM] float64, out elements, workspace elements, max source elements, max output columns)."""
    recs, prms = [], []
    out_off = ws_off = 0
    max_src = max_cols = 1
    for d in draws:
        for start, src, oshape, sd, scored in attempt_windows(d):
            rec, prm = window_record(start, src, oshape, out_off, sd, ws_off, scored)
            recs.append(rec)
            prms.append(prm)
            n = src[0] * src[1] * src[2]
            out_off += oshape[0] * oshape[1] * sd
            ws_off += 2 * n
            max_src = max(max_src, n)
            max_cols = max(max_cols, oshape[0] * oshape[1])
    return np.stack(recs), np.stack(prms), out_off, ws_off, max_src, max_cols


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def gpu_resample(vol_dev, spacing, out_xyz):
    """int16 [Z, Y, X] device volume -> int16 [OZ, OY, OX] at 1 mm."""
    Z, Y, X = vol_dev.shape
    ox, oy, oz = out_xyz
    out = torch.empty((oz, oy, ox), dtype=torch.int16, device=vol_dev.device)
    _lib.call_on_stream("pcrl_prep_resample", vol_dev, out, X, Y, Z, ox, oy, oz, float(spacing[0]), float(spacing[1]), float(spacing[2]))
    return out


def gpu_windows(vol_dev, rec, prm, out_elems, ws_elems, max_src, max_cols, padded_shape):
    """Runs pcrl_prep_windows on W records -> (out float64 device [out_elems], stats int32 device [W, 3])."""
    Z, Y, X = vol_dev.shape
    W = rec.shape[0]
    px, py, pz = padded_shape
    n = rec[:, 3] * rec[:, 4] * rec[:, 5]
    # every read inside the padded volume, every write inside its buffer (the kernels also guard, this names the culprit)
    if ((rec[:, 0] < 0) | (rec[:, 1] < 0) | (rec[:, 2] < 0) | (rec[:, 3] < 1) | (rec[:, 4] < 1) | (rec[:, 5] < 1)
            | (rec[:, 0] + rec[:, 3] > px) | (rec[:, 1] + rec[:, 4] > py) | (rec[:, 2] + rec[:, 5] > pz)).any():
        raise ValueError("window outside the volume")
    if (rec[:, 14] + 2 * n > ws_elems).any() or (rec[:, 12] + rec[:, 6] * rec[:, 7] * rec[:, 13] > out_elems).any():
        raise ValueError("window outside its buffers")
    if (rec[:, 8] > 64).any() or ((rec[:, 15] > 0) & (rec[:, 15] + 2 > rec[:, 8])).any() or (rec[:, 13] > rec[:, 8]).any():
        raise ValueError("bad window depths")
    dev = vol_dev.device
    rec_d = torch.from_numpy(rec).to(dev, non_blocking=False)
    prm_d = torch.from_numpy(prm).to(dev, non_blocking=False)
    out = torch.empty(out_elems, dtype=torch.float64, device=dev)
    ws = torch.empty(ws_elems, dtype=torch.float64, device=dev)
    stats = torch.empty((W, 3), dtype=torch.int32, device=dev)
    _lib.call_on_stream("pcrl_prep_windows", vol_dev, X, Y, Z, rec_d, prm_d, W, int(max_src), int(max_cols), out, out_elems, stats, ws, ws_elems)
    return out, stats


class GpuEvaluator:
    """evaluate(draws) for series_pairs: all windows of the batch in one launch; downloads only the accepted attempt."""

    def __init__(self, vol_dev, padded_shape, timing=None):
        self.vol, self.shape, self.timing = vol_dev, padded_shape, timing

    def __call__(self, draws):
        t0 = time.perf_counter()
        rec, prm, oe, we, ms, mc = build_records(draws)
        out, stats = gpu_windows(self.vol, rec, prm, oe, we, ms, mc, self.shape)
        st = stats.cpu().numpy()        # synchronises
        t1 = time.perf_counter()
        first = -1
        for a, d in enumerate(draws):
            if not rejected(int(st[8 * a, 0]), int(st[8 * a + 1, 0]), d.size1):
                first = a
                break
        payload = None
        if first >= 0:
            flat = out[first * ATTEMPT_ELEMS:(first + 1) * ATTEMPT_ELEMS].cpu().numpy()
            payload = (flat[:2 * GLOBAL_ELEMS].reshape(2, *INPUT), flat[2 * GLOBAL_ELEMS:].reshape(N_LOCAL, *LOCAL_INPUT))
        if self.timing is not None:
            self.timing["windows"] = self.timing.get("windows", 0.0) + (t1 - t0)
            self.timing["download"] = self.timing.get("download", 0.0) + (time.perf_counter() - t1)
        return first, payload


def prepare_volume(vol_zyx, spacing, device, timing=None):
    """Upload + resample -> (int16 device volume [z, y, x] at 1 mm, padded logical shape (x, y, z))."""
    t0 = time.perf_counter()
    src = torch.from_numpy(np.ascontiguousarray(vol_zyx)).to(device)
    torch.cuda.synchronize(device)
    t1 = time.perf_counter()
    Z, Y, X = vol_zyx.shape
    ox, oy, oz = resample_size((X, Y, Z), spacing)
    vol = gpu_resample(src, spacing, (ox, oy, oz))
    torch.cuda.synchronize(device)
    if timing is not None:
        timing["upload"] = timing.get("upload", 0.0) + (t1 - t0)
        timing["resample"] = timing.get("resample", 0.0) + (time.perf_counter() - t1)
    return vol, (ox, oy, padded_depth(oz))


# ---- files ----------------------------------------------------------------------------------------------------------------------
def save_pair(save_dir, name, k, glob_, loc, float32=False):
    dt = np.float32 if float32 else np.float64
    np.save(os.path.join(save_dir, f"{name}_global_{k}.npy"), np.ascontiguousarray(glob_, dtype=dt))
    np.save(os.path.join(save_dir, f"{name}_local_{k}.npy"), np.ascontiguousarray(loc, dtype=dt))


def series_list(data_dir, folds):
    out = []
    for f in folds:
        d = os.path.join(data_dir, f"subset{f}")
        if os.path.isdir(d):
            out += [(f, os.path.join(d, n)) for n in sorted(os.listdir(d)) if n.endswith(".mhd")]
    return out


def build_parser():
    p = argparse.ArgumentParser(description="LUNA16 raw CT -> PCRLv2 pre-task crop pairs (HIP kernels on one GPU)")
    p.add_argument("--data", required=True, help="LUNA16 directory with subset0..subset9/*.mhd")
    p.add_argument("--save", required=True, help="output directory (subset<f>/<series>_global_<k>.npy / _local_<k>.npy)")
    p.add_argument("--scale", type=int, default=16, help="crop pairs per series")
    p.add_argument("--input_rows", type=int, default=64)
    p.add_argument("--input_cols", type=int, default=64)
    p.add_argument("--input_deps", type=int, default=32)
    p.add_argument("--crop_rows", type=int, default=64)
    p.add_argument("--crop_cols", type=int, default=64)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--folds", default="0,1,2,3,4,5,6,7,8,9", help="comma-separated subset numbers")
    p.add_argument("--gpu", type=int, default=0)
    p.add_argument("--attempts-per-launch", type=int, default=16, help="crop-pair attempts evaluated per kernel launch")
    p.add_argument("--float32", action="store_true", help="write float32 files (half the disk; the loader reads either)")
    p.add_argument("--writers", type=int, default=4, help="file-writing threads (at most 16)")
    return p


def run(args, log=print):
    """-> {"series": n done, "skipped": [(path, reason)], "pairs": n}"""
    for flag in ("input_rows", "input_cols", "input_deps", "crop_rows", "crop_cols"):
        want = {"input_deps": 32}.get(flag, 64)
        if getattr(args, flag) != want:
            raise SystemExit(f"--{flag} {getattr(args, flag)}: the reference hard-codes 64 x 64 x 32 crops (luna_preprocess.py:128-131); "
                             "only the default is supported")
    if args.scale < 1 or args.attempts_per_launch < 1:
        raise SystemExit("--scale and --attempts-per-launch must be >= 1")
    folds = [int(f) for f in str(args.folds).split(",") if f.strip() != ""]
    device = torch.device("cuda", args.gpu)
    torch.cuda.set_device(device)
    files = series_list(args.data, folds)
    result = {"series": 0, "skipped": [], "pairs": 0}
    writers = max(1, min(16, args.writers))
    with cf.ThreadPoolExecutor(1) as reader, cf.ThreadPoolExecutor(writers) as writer:
        pending = []
        nxt = reader.submit(read_metaimage, files[0][1]) if files else None
        for i, (fold, path) in enumerate(files):
            try:
                vol_zyx, spacing, _ = nxt.result()
            except (MetaImageError, OSError, KeyError, ValueError) as e:
                vol_zyx, err = None, e
            nxt = reader.submit(read_metaimage, files[i + 1][1]) if i + 1 < len(files) else None
            name = os.path.basename(path)[:-4]
            if vol_zyx is None:
                log(f"[luna_prep] skip {path}: {err}")
                result["skipped"].append((path, str(err)))
                continue
            save_dir = os.path.join(args.save, f"subset{fold}")
            os.makedirs(save_dir, exist_ok=True)
            vol, shape = prepare_volume(vol_zyx, spacing, device)
            pairs = []
            try:
                for k, (g, loc) in series_pairs(shape, name, args.seed, args.scale, args.attempts_per_launch, GpuEvaluator(vol, shape)):
                    pairs.append((k, g, loc))
            except SeriesSkipped as e:
                log(f"[luna_prep] skip {path}: {e}")
                result["skipped"].append((path, str(e)))
                continue
            for k, g, loc in pairs:      # written only once the whole series succeeded
                pending.append(writer.submit(save_pair, save_dir, name, k, g, loc, args.float32))
            result["series"] += 1
            result["pairs"] += len(pairs)
            log(f"[luna_prep] subset{fold}/{name}: volume {shape}, {len(pairs)} pairs")
            while len(pending) > 4 * args.scale:      # bound the host memory held by queued writes
                pending.pop(0).result()
        for p in pending:
            p.result()
    log(f"[luna_prep] {result['series']} series, {result['pairs']} pairs written, {len(result['skipped'])} skipped")
    return result


def main(argv=None):
    args = build_parser().parse_args(argv)
    run(args)


if __name__ == "__main__":
    main(sys.argv[1:])
