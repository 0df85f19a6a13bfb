"""Data of 3D segmentation fine-tuning: cases on disk, training crops, evaluation tiles, synthetic phantoms.

On disk: `DIR/<case>_img.npy` [C, X, Y, Z] float32 or float16, used as stored (intensity normalisation is the preparer's job), `DIR/<case>_seg.npy`
[X, Y, Z] uint8 bitmask (bit k: the voxel belongs to class k -- classes may overlap, as BraTS's WT / TC / ET do; bit 7: the voxel is NOT counted), and
`DIR/train.txt`, `val.txt`, `test.txt` with one case name per line.  Both arrays are memory-mapped: a crop or a tile reads its own voxels only.

Training crops (CropLoader): `crop`-sized, cut on the host; every other crop of a batch is centred on a uniformly drawn labelled voxel, the others are
placed uniformly; an independent flip per axis is applied identically to image and mask; a volume shorter than the crop on an axis is padded with image
0 and label 0x80.  Evaluation tiles (TileLoader): every case is covered by crop-sized patches at stride = crop, the last patch of an axis shifted back
inside the volume; voxels an earlier patch already covered carry bit 7 in the later one, so every voxel of every case is counted exactly once and every
forward has the training crop's shape.  No whole-volume forward.

Overlap-blended sliding windows (window_axis, windows, blend_weights; the pass itself is train_seg.sliding_window): crop-sized patches at stride
int(crop * (1 - overlap)), the last one of an axis shifted back inside the volume, every voxel's logits the window-weighted mean over the patches
that cover it.  The tiled path above is what `--overlap 0` (the default) runs.
"""
from __future__ import annotations

import os

import numpy as np
import torch

NOT_COUNTED = 0x80


def parse_crop(crop):
    """'64,64,32' or a sequence -> (cx, cy, cz); three positive multiples of 8 (the network halves the grid three times), else SystemExit."""
    try:
        c = tuple(int(v) for v in (crop.split(",") if isinstance(crop, str) else crop))
    except ValueError:
        c = ()
    if len(c) != 3 or any(v <= 0 or v % 8 for v in c):
        raise SystemExit(f"--crop {crop}: three positive multiples of 8, comma separated (the network halves the grid three times)")
    return c


def check_n_class(n_class):
    if not 1 <= int(n_class) <= 7:
        raise SystemExit(f"--n_class {n_class}: 1..7 (one bit of the label byte per class; bit 7 means 'not counted')")
    return int(n_class)


# ---- cases ------------------------------------------------------------------------------------------------------------------------
class Case:
    """One volume: img [C, X, Y, Z] (float32 / float16 array or memmap), seg [X, Y, Z] uint8 (None: unlabelled, predict only)."""

    def __init__(self, name, img, seg=None):
        self.name, self.img, self.seg = name, img, seg
        self.shape = tuple(int(s) for s in img.shape[1:])
        self._fg = None

    def foreground(self):
        """Flat indices of the voxels with any class bit, found once per case."""
        if self._fg is None:
            self._fg = np.flatnonzero(np.asarray(self.seg).reshape(-1) & 0x7F)
        return self._fg


def read_list(data_dir, list_file):
    """Case names of DIR/<list_file> (or of a path given as such), one per line."""
    path = list_file if os.path.isabs(list_file) or os.path.exists(list_file) else os.path.join(data_dir, list_file)
    if not os.path.exists(path):
        raise SystemExit(f"{path}: no such case list (one case name per line; DIR/train.txt, val.txt and test.txt)")
    with open(path) as f:
        return [ln.strip() for ln in f if ln.strip()]


def open_case(data_dir, name, n_class, in_channels, need_seg=True):
    img_path, seg_path = os.path.join(data_dir, name + "_img.npy"), os.path.join(data_dir, name + "_seg.npy")
    if not os.path.exists(img_path):
        raise SystemExit(f"{img_path}: missing (a case is <case>_img.npy [C,X,Y,Z] float32 / float16 and <case>_seg.npy [X,Y,Z] uint8)")
    img = np.load(img_path, mmap_mode="r")
    if img.ndim != 4 or img.shape[0] != in_channels or img.dtype not in (np.float32, np.float16):
        raise SystemExit(f"{img_path}: expected a float32 / float16 array [{in_channels}, X, Y, Z] (--in_channels {in_channels}), got {img.dtype} {img.shape}")
    seg = None
    if need_seg or os.path.exists(seg_path):
        if not os.path.exists(seg_path):
            raise SystemExit(f"{seg_path}: missing")
        seg = np.load(seg_path, mmap_mode="r")
        if seg.dtype != np.uint8 or tuple(seg.shape) != tuple(img.shape[1:]):
            raise SystemExit(f"{seg_path}: expected a uint8 bitmask of shape {tuple(img.shape[1:])}, got {seg.dtype} {seg.shape}")
        bits = int(np.bitwise_or.reduce(np.asarray(seg).reshape(-1))) if seg.size else 0
        bad = bits & 0x7F & ~((1 << n_class) - 1)
        if bad:
            raise SystemExit(f"{seg_path}: label bits {bad:#04x} are set but --n_class is {n_class} (bit k = class k < n_class; only bit 7, 'not counted', "
                             "may be set above them)")
    return Case(name, img, seg)


def open_cases(data_dir, list_file, n_class, in_channels, need_seg=True):
    return [open_case(data_dir, n, n_class, in_channels, need_seg) for n in read_list(data_dir, list_file)]


# ---- cutting ----------------------------------------------------------------------------------------------------------------------
def cut(case, start, crop):
    """The crop-sized box at `start` of the volume padded (at the high end) to at least the crop: (x float32 [C, *crop], lab uint8 [*crop]); what lies
    outside the volume is image 0 / label 0x80.  An unlabelled case: label 0 inside."""
    C = case.img.shape[0]
    x = np.zeros((C,) + tuple(crop), dtype=np.float32)
    lab = np.full(tuple(crop), NOT_COUNTED, dtype=np.uint8)
    src = tuple(slice(s, min(s + c, n)) for s, c, n in zip(start, crop, case.shape))
    dst = tuple(slice(0, sl.stop - sl.start) for sl in src)
    x[(slice(None),) + dst] = case.img[(slice(None),) + src]
    lab[dst] = case.seg[src] if case.seg is not None else 0
    return x, lab


def tile_axis(size, crop):
    """[(start, first index this tile is the first to cover)] along one axis: stride = crop, the last tile shifted back inside the volume."""
    if size <= crop:
        return [(0, 0)]
    n = -(-size // crop)
    return [(min(i * crop, size - crop), i * crop) for i in range(n)]


def tiles(shape, crop):
    """-> [(start (x, y, z), own_from (x, y, z))] in x-major order; a tile counts the voxels at or above own_from on every axis."""
    ax = [tile_axis(s, c) for s, c in zip(shape, crop)]
    return [((a[0], b[0], c[0]), (a[1], b[1], c[1])) for a in ax[0] for b in ax[1] for c in ax[2]]


# ---- overlap-blended sliding windows ----------------------------------------------------------------------------------------------
MAX_OVERLAP = 0.75
WINDOWS = ("gaussian", "constant")


def check_overlap(overlap, flag="--overlap"):
    try:
        f = float(overlap)
    except (TypeError, ValueError):
        f = float("nan")
    if not 0.0 <= f <= MAX_OVERLAP:
        raise SystemExit(f"{flag} {overlap}: a fraction of the crop in [0, {MAX_OVERLAP}] (0: stride-tiled patches, no blending; 0.5: MONAI's and nnU-Net's usual "
                         "choice; above 0.75 the patch count explodes)")
    return f


def check_window(window, flag="--window"):
    if window not in WINDOWS:
        raise SystemExit(f"{flag} {window}: one of {', '.join(WINDOWS)}")
    return window


def window_axis(size, crop, overlap):
    """The ascending, distinct patch starts along one axis: stride max(1, int(crop * (1 - overlap))), the last patch shifted back inside the volume; a
    volume no longer than the crop has the one patch at 0 (zero-padded at the high end, as cut pads)."""
    overlap = check_overlap(overlap)
    size, crop = int(size), int(crop)
    if size <= crop:
        return [0]
    interval = max(1, int(crop * (1 - overlap)))
    n = -(-(size - crop) // interval) + 1
    return sorted({min(i * interval, size - crop) for i in range(n)})


def windows(shape, crop, overlap):
    """-> the three per-axis start lists; the patches run in x-major order: patch (ix * ny + iy) * nz + iz starts at (sx[ix], sy[iy], sz[iz])."""
    return [window_axis(s, c, overlap) for s, c in zip(shape, crop)]


def window_starts(axes):
    """The start (x, y, z) of every patch of `windows`' lists, in patch order."""
    return [(a, b, c) for a in axes[0] for b in axes[1] for c in axes[2]]


def blend_weights(crop, window):
    """The separable importance map: three float32 tables wx [cx], wy [cy], wz [cz]; a patch voxel (i, j, k) weighs (wx[i] * wy[j]) * wz[k].  'constant':
    ones.  'gaussian': exp(-0.5 ((i - (c - 1) / 2) / (0.125 c))^2) (nnU-Net's sigma of an eighth of the crop), float64 rounded once to float32; every
    entry is positive (at least exp(-8)), so a covered voxel never has weight 0."""
    check_window(window)
    out = []
    for c in crop:
        c = int(c)
        if window == "constant":
            out.append(np.ones(c, dtype=np.float32))
        else:
            i = np.arange(c, dtype=np.float64)
            out.append(np.exp(-0.5 * ((i - (c - 1) / 2.0) / (0.125 * c)) ** 2).astype(np.float32))
    return out


def cut_tile(case, start, own_from, crop):
    """cut() plus bit 7 on every voxel an earlier tile of the case already covered."""
    x, lab = cut(case, start, crop)
    for axis, (s, o) in enumerate(zip(start, own_from)):
        if o > s:
            sl = [slice(None)] * 3
            sl[axis] = slice(0, o - s)
            lab[tuple(sl)] |= NOT_COUNTED
    return x, lab


def draw_crop(rng, case, crop, centred):
    """One training crop.  -> (x, lab, info): info = {'start', 'flips', 'voxel' (the labelled voxel a centred crop contains, else None)}."""
    room = [max(n - c, 0) for n, c in zip(case.shape, crop)]
    voxel = None
    fg = case.foreground() if centred else ()
    if len(fg):
        voxel = tuple(int(v) for v in np.unravel_index(int(fg[int(rng.integers(len(fg)))]), case.shape))
        start = tuple(min(max(v - c // 2, 0), r) for v, c, r in zip(voxel, crop, room))
    else:
        start = tuple(int(rng.integers(r + 1)) for r in room)
    flips = tuple(bool(rng.integers(2)) for _ in range(3))
    x, lab = cut(case, start, crop)
    for axis, f in enumerate(flips):
        if f:
            x, lab = np.flip(x, axis + 1), np.flip(lab, axis)
    return np.ascontiguousarray(x), np.ascontiguousarray(lab), {"start": start, "flips": flips, "voxel": voxel}


class CropLoader:
    """`steps` batches of `b` training crops per epoch: (x float32 [b, C, *crop], lab uint8 [b, *crop]) host tensors.  The draws are a function of
    (seed, rank, epoch) alone; crop i of a batch is centred on a labelled voxel for even i."""

    def __init__(self, cases, crop, b, steps, seed=0, rank=0):
        if not cases:
            raise SystemExit("no training cases")
        self.cases, self.crop, self.b, self.steps, self.seed, self.rank, self.epoch = cases, tuple(crop), int(b), int(steps), int(seed), int(rank), 0
        self.sharded = True

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        return self.steps

    def __iter__(self):
        rng = np.random.default_rng([self.seed, self.rank, self.epoch])
        for _ in range(self.steps):
            xs, ls = [], []
            for i in range(self.b):
                x, lab, _ = draw_crop(rng, self.cases[int(rng.integers(len(self.cases)))], self.crop, centred=i % 2 == 0)
                xs.append(x)
                ls.append(lab)
            yield torch.from_numpy(np.stack(xs)), torch.from_numpy(np.stack(ls))


class TileLoader:
    """The evaluation tiles of this rank's contiguous shard of `cases`, `b` per batch (the last batch may be shorter):
    (x float32 [n, C, *crop], lab uint8 [n, *crop], case_index int32 [n] into the GLOBAL case table, starts int64 [n, 3]) host tensors."""

    def __init__(self, cases, crop, b, rank=0, world=1):
        self.cases, self.crop, self.b = cases, tuple(crop), int(b)
        n = len(cases)
        self.mine = range(rank * n // world, (rank + 1) * n // world)
        self.sharded = True

    def _items(self):
        return [(ci, t) for ci in self.mine for t in tiles(self.cases[ci].shape, self.crop)]

    def __len__(self):
        return -(-len(self._items()) // self.b)

    def __iter__(self):
        items = self._items()
        for a in range(0, len(items), self.b):
            xs, ls = zip(*[cut_tile(self.cases[ci], st, own, self.crop) for ci, (st, own) in items[a:a + self.b]])
            yield (torch.from_numpy(np.stack(xs)), torch.from_numpy(np.stack(ls)), torch.tensor([ci for ci, _ in items[a:a + self.b]], dtype=torch.int32),
                   torch.tensor([st for _, (st, _) in items[a:a + self.b]], dtype=torch.int64))


# ---- synthetic phantoms -----------------------------------------------------------------------------------------------------------
def synthetic_case(seed, index, shape, n_class, in_channels=1):
    """A phantom, a fixed function of (seed, index): unit noise; class k is an ellipsoid (the K of them overlap: each is drawn around the first one's
    centre) inside which every channel is raised by 1.5 (k + 1).  -> Case with in-memory arrays."""
    rng = np.random.default_rng([int(seed), int(index)])
    shape = tuple(int(s) for s in shape)
    img = rng.standard_normal((in_channels,) + shape, dtype=np.float32)
    seg = np.zeros(shape, dtype=np.uint8)
    grid = np.meshgrid(*[np.arange(n, dtype=np.float32) for n in shape], indexing="ij")
    centre0 = np.array([rng.uniform(0.35, 0.65) * n for n in shape])
    for k in range(n_class):
        centre = centre0 + rng.uniform(-0.1, 0.1, 3) * np.array(shape)
        radii = rng.uniform(0.15, 0.3, 3) * np.array(shape) / (1.0 + 0.35 * k)
        inside = sum(((g - c) / r) ** 2 for g, c, r in zip(grid, centre, radii)) <= 1.0
        seg[inside] |= np.uint8(1 << k)
        img[:, inside] += np.float32(1.5 * (k + 1))
    return Case("phantom%03d" % index, img, seg)


def write_synthetic(data_dir, names, shape, n_class, in_channels=1, seed=0, first_index=0):
    """The phantoms as cases on disk (tests, smoke commands)."""
    os.makedirs(data_dir, exist_ok=True)
    for i, name in enumerate(names):
        c = synthetic_case(seed, first_index + i, shape, n_class, in_channels)
        np.save(os.path.join(data_dir, name + "_img.npy"), c.img)
        np.save(os.path.join(data_dir, name + "_seg.npy"), c.seg)


def synthetic_shape(crop):
    """The phantoms' size for a crop: no multiple of it, so that the tiling's shifted last patches are exercised."""
    return (crop[0] * 3 // 2, crop[1] * 5 // 4 - 4, crop[2] * 5 // 4)


def loaders(args, rank=0, world=1):
    """{'train': CropLoader, 'eval': TileLoader, 'test': TileLoader} for --data DIR | synthetic."""
    crop, K, C = parse_crop(args.crop), check_n_class(args.n_class), int(args.in_channels)
    if args.data == "synthetic":
        shape = synthetic_shape(crop)
        mk = lambda first, n: [synthetic_case(args.seed, first + i, shape, K, C) for i in range(n)]     # noqa: E731
        train, val, test = mk(0, 8), mk(1000, 2), mk(2000, 2)
    elif os.path.isdir(args.data):
        train, val, test = (open_cases(args.data, f, K, C) for f in ("train.txt", "val.txt", "test.txt"))
    else:
        raise SystemExit("--data must be 'synthetic' or a directory with <case>_img.npy / <case>_seg.npy and train.txt, val.txt, test.txt")
    steps = int(args.steps_per_epoch) or -(-len(train) // int(args.b))         # 0: one crop per training case and epoch
    return {"train": CropLoader(train, crop, args.b, steps, args.seed, rank),
            "eval": TileLoader(val, crop, args.b, rank, world), "test": TileLoader(test, crop, args.b, rank, world)}
