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

Training-time augmentation (AugConfig, source_extent, cut_box, draw_aug_crop; CropLoader(aug=...)): the host draws rotation,
zoom, flips and per-channel intensity parameters and cuts a source box around the crop; image channels and label bitmask are resampled together on
the device (ops.seg_augment, csrc/seg_augment.hip) by train_seg.train_step.  Without `aug` nothing changes.

Mirror test-time augmentation (parse_mirror, mirror_letters): the mirror codes train_seg.sliding_window shows every patch in.

Label maps (head='softmax'): a label byte holds the class index in bits 0..6 (0 = background) and 'not counted' in bit 7, so cut,
cut_tile, cut_box and the augmentation carry it unchanged.  check_n_class(n, head) takes 2..16 for it, open_case(head='softmax') refuses a class index
>= n_class naming the file and the value, synthetic_case(head='softmax') draws DISJOINT phantoms as class indices; Case.foreground is "non-background".
"""
from __future__ import annotations

import dataclasses
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


HEADS = ("sigmoid", "softmax")


def check_head(head):
    if head not in HEADS:
        raise SystemExit(f"--head {head}: 'sigmoid' (overlapping regions, labels are bitmasks; the default) or 'softmax' (mutually exclusive classes, "
                         "labels are label maps)")
    return head


def check_n_class(n_class, head="sigmoid"):
    if check_head(head) == "softmax":
        if not 2 <= int(n_class) <= 16:
            raise SystemExit(f"--n_class {n_class}: 2..16 with --head softmax (mutually exclusive classes, the background counted; a label byte holds "
                             "the class index in bits 0..6, bit 7 means 'not counted')")
        return int(n_class)
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


def open_case(data_dir, name, n_class, in_channels, need_seg=True, head="sigmoid"):
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
        if head == "softmax":       # a label map: the class index in bits 0..6
            top = int((np.asarray(seg).reshape(-1) & 0x7F).max()) if seg.size else 0
            if top >= n_class:
                raise SystemExit(f"{seg_path}: label value {top} but --n_class is {n_class} with --head softmax (a label-map byte holds the class index "
                                 f"0..{n_class - 1} in bits 0..6, 0 = background; only bit 7, 'not counted', may be set above it)")
            return Case(name, img, seg)
        bits = int(np.bitwise_or.reduce(np.asarray(seg).reshape(-1))) if seg.size else 0
        bad = bits & 0x7F & ~((1 << n_class) - 1)
        if bad:
            raise SystemExit(f"{seg_path}: label bits {bad:#04x} are set but --n_class is {n_class} (bit k = class k < n_class; only bit 7, 'not counted', "
                             "may be set above them)")
    return Case(name, img, seg)


def open_cases(data_dir, list_file, n_class, in_channels, need_seg=True, head="sigmoid"):
    return [open_case(data_dir, n, n_class, in_channels, need_seg, head) for n in read_list(data_dir, list_file)]


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


# ---- mirror test-time augmentation --------------------------------------------------------------------------
MIRROR_AXES = "xyz"          # a mirror code has bit 0 = x, bit 1 = y, bit 2 = z: the patch's first, second and third spatial axis


def parse_mirror(text, flag="--mirror"):
    """'none' (the default) -> [0]; 'all' -> [0..7]; a non-empty subset of the letters xyz in any order -> every combination of the chosen axes as
    ascending mirror codes, the identity first ('xz' -> [0, 1, 4, 5]).  Anything else exits with its message."""
    t = "none" if text is None else str(text).strip().lower()
    if t == "none":
        return [0]
    letters = MIRROR_AXES if t == "all" else t
    if not letters or any(c not in MIRROR_AXES for c in letters) or len(set(letters)) != len(letters):
        raise SystemExit(f"{flag} {text}: none, all, or the axes to mirror along as distinct letters of xyz (xz: the four combinations of the x and z "
                         "mirrors, the identity among them)")
    chosen = sum(1 << MIRROR_AXES.index(c) for c in letters)
    return [code for code in range(8) if code & ~chosen == 0]


def mirror_letters(codes):
    """The axes a list of mirror codes touches, as parse_mirror spells them: [0, 1, 4, 5] -> 'xz'; [0] -> 'none'."""
    bits = 0
    for code in codes:
        bits |= int(code)
    return "".join(c for i, c in enumerate(MIRROR_AXES) if bits >> i & 1) or "none"


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


# ---- training-time augmentation: the host side of csrc/seg_augment.hip -----------------------------------------------
MAX_ROTATE = 45.0


@dataclasses.dataclass(frozen=True)
class AugConfig:
    """What one training crop may go through.  Spatial, with probability p_spatial per crop: three Euler angles uniform in +-rotate degrees (voxel
    index space) and one log-uniform isotropic scale in `scale`.  Intensity, with probability p_intensity per channel: a gain uniform in `gain`, a
    bias uniform in +-bias, a log-uniform gamma in `gamma` and a noise standard deviation uniform in [0, noise_std].  The default is all neutral."""
    rotate: float = 0.0
    scale: tuple = (1.0, 1.0)
    p_spatial: float = 0.5
    gain: tuple = (1.0, 1.0)
    bias: float = 0.0
    gamma: tuple = (1.0, 1.0)
    noise_std: float = 0.0
    p_intensity: float = 0.15

    @classmethod
    def defaults(cls, **over):
        """What `--augment` alone turns on."""
        return dataclasses.replace(cls(rotate=15.0, scale=(0.8, 1.25), p_spatial=0.5, gain=(0.75, 1.25), bias=0.1, gamma=(0.7, 1.5), noise_std=0.1,
                                       p_intensity=0.15), **over)

    @property
    def spatial(self):
        return self.p_spatial > 0 and (self.rotate != 0 or tuple(self.scale) != (1.0, 1.0))

    @property
    def intensity(self):
        return self.p_intensity > 0 and (tuple(self.gain) != (1.0, 1.0) or self.bias != 0 or tuple(self.gamma) != (1.0, 1.0) or self.noise_std != 0)

    @property
    def enabled(self):
        return self.spatial or self.intensity


AUG_OPTIONS = ("aug_rotate", "aug_scale", "aug_gain", "aug_bias", "aug_gamma", "aug_noise", "aug_p_spatial", "aug_p_intensity")


def _aug_number(flag, value, what):
    try:
        f = float(value)
    except (TypeError, ValueError):
        f = float("nan")
    if f != f or f in (float("inf"), float("-inf")):
        raise SystemExit(f"{flag} {value}: {what}")
    return f


def _aug_range(flag, value, what, positive=False):
    try:
        r = tuple(float(v) for v in (value.split(",") if isinstance(value, str) else value))
    except (TypeError, ValueError):
        r = ()
    if len(r) != 2 or not all(np.isfinite(v) for v in r) or r[0] > r[1] or (positive and r[0] <= 0):
        raise SystemExit(f"{flag} {value}: {what}")
    return r


def parse_aug(args):
    """The augmentation options of `seg3d.py train` (absent attributes: not given) -> AugConfig, or None when none of them is given.  `--augment` turns
    the defaults on; every override implies it and replaces one default.  A bad value exits with its message."""
    given = {k: getattr(args, k, None) for k in AUG_OPTIONS}
    given = {k: v for k, v in given.items() if v is not None}
    if not given and not getattr(args, "augment", False):
        return None
    d = AugConfig.defaults()
    rotate = _aug_number("--aug_rotate", given.get("aug_rotate", d.rotate), "the largest rotation about each axis in degrees, 0..45")
    if not 0.0 <= rotate <= MAX_ROTATE:
        raise SystemExit(f"--aug_rotate {given['aug_rotate']}: the largest rotation about each axis in degrees, 0..45 (beyond that the source box of a "
                         "crop outgrows the crop several times)")
    scale = _aug_range("--aug_scale", given.get("aug_scale", d.scale), "LO,HI with 0 < LO <= HI (the zoom factor is drawn log-uniformly between them)", True)
    gain = _aug_range("--aug_gain", given.get("aug_gain", d.gain), "LO,HI with LO <= HI (the factor on a channel's intensities)")
    gamma = _aug_range("--aug_gamma", given.get("aug_gamma", d.gamma), "LO,HI with 0 < LO <= HI (the exponent of sign(v) |v|^gamma)", True)
    bias = _aug_number("--aug_bias", given.get("aug_bias", d.bias), "B >= 0 (a channel's intensities are shifted by a value in [-B, B])")
    if bias < 0:
        raise SystemExit(f"--aug_bias {given['aug_bias']}: B >= 0 (a channel's intensities are shifted by a value in [-B, B])")
    noise = _aug_number("--aug_noise", given.get("aug_noise", d.noise_std), "STD >= 0 (the largest standard deviation of the added Gaussian noise)")
    if noise < 0:
        raise SystemExit(f"--aug_noise {given['aug_noise']}: STD >= 0 (the largest standard deviation of the added Gaussian noise)")
    ps = []
    for key, default in (("aug_p_spatial", d.p_spatial), ("aug_p_intensity", d.p_intensity)):
        p = _aug_number("--" + key, given.get(key, default), "a probability in [0, 1]")
        if not 0.0 <= p <= 1.0:
            raise SystemExit(f"--{key} {given[key]}: a probability in [0, 1]")
        ps.append(p)
    return AugConfig(rotate=rotate, scale=scale, p_spatial=ps[0], gain=gain, bias=bias, gamma=gamma, noise_std=noise, p_intensity=ps[1])


def _reach(a, b, theta):
    """max over |t| <= theta of cos(t) a + sin|t| b, for a, b >= 0 and 0 <= theta <= pi / 2: the unconstrained maximum hypot(a, b) sits at
    t = atan2(b, a); where that lies beyond theta the expression still rises at theta."""
    return float(np.hypot(a, b)) if np.arctan2(b, a) <= theta else float(np.cos(theta) * a + np.sin(theta) * b)


def source_extent(crop, cfg):
    """The ONE source-box size (ex, ey, ez), even on every axis, of a loader with this crop and config: large enough that for every parameter set
    the config can draw every trilinear corner of every output voxel lies inside the box.

    Derivation.  The kernel samples output voxel i at s = M c + t + E / 2 - 0.5 with c = i + 0.5 - crop / 2, so |c_j| <= crop_j / 2 - 0.5, and
    |t_i| <= 0.5.  The corners floor(s_i) and floor(s_i) + 1 are inside [0, E_i - 1] when 0 <= s_i < E_i - 1, that is when
        |(M c)_i| + 0.5 < E_i / 2 - 0.5       which      E_i / 2 >= sum_j |M_ij| crop_j / 2 + 1 =: r_i + 1
    guarantees (sum_j |M_ij| (crop_j / 2 - 0.5) + 0.5 < r_i + 0.5 whenever a row of M is not zero).  M = R F / z: F the diagonal of flip signs, which
    |.| removes; z the zoom, largest inverse 1 / min(scale_lo, 1) (a crop that draws no spatial change has z = 1 and R = I, which the angle box
    contains); R = Rx(a) Ry(b) Rz(g), every angle within +-theta, theta <= 45 degrees.  With h_j = crop_j / 2
    and reach(A, B) = max_{|t| <= theta} cos(t) A + sin|t| B (_reach), the rows of R, entry by entry under the triangle inequality and every
    angle maximised on its own:
        row x = (cb cg, -cb sg, sb):                       cb (|cg| hx + |sg| hy) + |sb| hz  <=  reach(P, hz),   P = reach(hx, hy)
        row z = sa (row y of Ry Rz) + ca (row z of Ry Rz):  ca (|sb| (|cg| hx + |sg| hy) + cb hz) + |sa| (|sg| hx + |cg| hy)
                                                            <=  reach(U, Q),   U = reach(hz, P),   Q = reach(hy, hx)
        row y = ca (row y of Ry Rz) - sa (row z of Ry Rz):  <=  reach(Q, U)
    Row x's bound is attained; rows y and z are bounded from above (g is maximised separately in P and Q).  E_i is the smallest even integer
    >= 2 (r_i / min(scale_lo, 1) + 1).  No rotation and no zoom: crop + 2."""
    h = [float(c) / 2.0 for c in crop]
    theta = np.deg2rad(min(max(float(cfg.rotate), 0.0), 90.0)) if cfg.p_spatial > 0 else 0.0
    zoom = 1.0 / min(float(cfg.scale[0]), 1.0) if cfg.p_spatial > 0 else 1.0
    P, Q = _reach(h[0], h[1], theta), _reach(h[1], h[0], theta)
    U = _reach(h[2], P, theta)
    rows = (_reach(P, h[2], theta), _reach(Q, U, theta), _reach(U, Q, theta))
    # - 2^-20: a row sum that is an integer up to float64 rounding (no rotation: exactly crop / 2) must not cost two voxels; the inequality above has
    # 0.5 sum_j |M_ij| >= 0.5 / max(scale_hi, 1) to spare
    return tuple(2 * int(np.ceil(r * zoom + 1.0 - 2.0 ** -20)) for r in rows)


def cut_box(case, start, extent):
    """`cut` with starts allowed below 0: the extent-sized box at `start`, (x [C, *extent] in the case's dtype, lab uint8 [*extent]); what lies outside
    the volume ON EITHER SIDE is image 0 / label 0x80.  A float16 case stays float16 up to the device (the kernel reads half).  An unlabelled case:
    label 0 inside."""
    C = case.img.shape[0]
    x = np.zeros((C,) + tuple(extent), dtype=case.img.dtype)
    lab = np.full(tuple(extent), NOT_COUNTED, dtype=np.uint8)
    lo = [min(max(int(s), 0), n) for s, n in zip(start, case.shape)]
    hi = [min(max(int(s) + int(e), 0), n) for s, e, n in zip(start, extent, case.shape)]
    if all(b > a for a, b in zip(lo, hi)):
        src = tuple(slice(a, b) for a, b in zip(lo, hi))
        dst = tuple(slice(a - int(s), b - int(s)) for a, b, s in zip(lo, hi, start))
        x[(slice(None),) + dst] = case.img[(slice(None),) + src]
        lab[dst] = case.seg[src] if case.seg is not None else 0
    return x, lab


def rotation(angles):
    """Rx(a) Ry(b) Rz(g) for angles in radians, float64 [3, 3]; axes in (x, y, z) voxel index order."""
    (sa, sb, sg), (ca, cb, cg) = np.sin(angles), np.cos(angles)
    rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]], dtype=np.float64)
    ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]], dtype=np.float64)
    rz = np.array([[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]], dtype=np.float64)
    return rx @ ry @ rz


def inverse_affine(angles, scale, flips, crop, extent):
    """The kernel's 12 numbers (rows (m0 m1 m2 t) of x, y, z), float32: M = R(angles) diag(flip signs) / scale -- the output crop is the resampled
    box flipped, as draw_crop flips what it has cut -- and t = 0, or -0.5 on an axis where extent - crop is odd (the box then starts at
    start - (extent - crop) // 2 and its centre sits half a voxel above the crop's)."""
    m = rotation(np.asarray(angles, dtype=np.float64)) @ np.diag([-1.0 if f else 1.0 for f in flips]) / float(scale)
    t = np.array([-0.5 if (int(e) - int(c)) % 2 else 0.0 for e, c in zip(extent, crop)])
    return np.concatenate([m, t[:, None]], axis=1).reshape(12).astype(np.float32)


def draw_aug_crop(rng, case, crop, centred, cfg, extent=None):
    """One augmented training crop, still to be resampled on the device.  The crop is placed and flipped by draw_crop's rules with draw_crop's
    draws (the same rng state gives the same start and flips); then, with probability p_spatial, three Euler angles and a zoom, and per channel with
    probability p_intensity a gain, a bias, a gamma and a noise standard deviation (neutral values otherwise).
    -> (src [C, *extent] in the case's dtype, src_lab uint8 [*extent], inv float32 [12], rows {'gain', 'bias', 'gamma', 'noise_std': float32 [C]},
        info = draw_crop's {'start', 'flips', 'voxel'} plus 'box' (the box's start), 'angles' (radians), 'scale' and 'spatial' (whether drawn))"""
    crop = tuple(int(c) for c in crop)
    extent = source_extent(crop, cfg) if extent is None else tuple(int(e) for e in extent)
    room = [max(n - c, 0) for n, c in zip(case.shape, crop)]
    voxel = None
    fg = case.foreground() if centred else ()
    if len(fg):
        voxel = tuple(int(v) for v in np.unravel_index(int(fg[int(rng.integers(len(fg)))]), case.shape))
        start = tuple(min(max(v - c // 2, 0), r) for v, c, r in zip(voxel, crop, room))
    else:
        start = tuple(int(rng.integers(r + 1)) for r in room)
    flips = tuple(bool(rng.integers(2)) for _ in range(3))
    C = case.img.shape[0]
    spatial = bool(rng.random() < cfg.p_spatial)
    theta = np.deg2rad(float(cfg.rotate))
    angles = rng.uniform(-theta, theta, 3)
    scale = float(np.exp(rng.uniform(np.log(cfg.scale[0]), np.log(cfg.scale[1]))))
    if not spatial:
        angles, scale = np.zeros(3), 1.0
    on = rng.random(C) < cfg.p_intensity
    rows = {"gain": np.where(on, rng.uniform(cfg.gain[0], cfg.gain[1], C), 1.0), "bias": np.where(on, rng.uniform(-cfg.bias, cfg.bias, C), 0.0),
            "gamma": np.where(on, np.exp(rng.uniform(np.log(cfg.gamma[0]), np.log(cfg.gamma[1]), C)), 1.0),
            "noise_std": np.where(on, rng.uniform(0.0, cfg.noise_std, C), 0.0)}
    rows = {k: v.astype(np.float32) for k, v in rows.items()}
    box = tuple(s - (e - c) // 2 for s, c, e in zip(start, crop, extent))
    src, src_lab = cut_box(case, box, extent)
    info = {"start": start, "flips": flips, "voxel": voxel, "box": box, "angles": tuple(float(a) for a in angles), "scale": scale, "spatial": spatial}
    return src, src_lab, inverse_affine(angles, scale, flips, crop, extent), rows, info


class CropLoader:
    """`steps` batches of `b` training crops per epoch: (x float32 [b, C, *crop], lab uint8 [b, *crop]) host tensors.  The draws are a function of
    (seed, rank, epoch) alone; crop i of a batch is centred on a labelled voxel for even i.

    With `aug` (an enabled AugConfig) a batch is (src [b, C, *extent] in the cases' dtype, src_lab uint8 [b, *extent], params): the source boxes of
    draw_aug_crop and a dict of host tensors -- inv float32 [b, 12]; gain, bias, gamma, noise_std float32 [b, C]; seed, one int64 from the same
    rng (the noise kernel's); crop int64 [3] -- that train_seg.train_step resamples on the device.  Without it: the code path and the random
    stream of a loader that knows no augmentation."""

    def __init__(self, cases, crop, b, steps, seed=0, rank=0, aug=None):
        if not cases:
            raise SystemExit("no training cases")
        self.cases, self.crop, self.b, self.steps, self.seed, self.rank, self.epoch = cases, tuple(crop), int(b), int(steps), int(seed), int(rank), 0
        self.sharded = True
        self.aug = aug if aug is not None and aug.enabled else None
        self.extent = source_extent(self.crop, self.aug) if self.aug is not None else None

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        return self.steps

    def _augmented(self, rng):
        for _ in range(self.steps):
            srcs, labs, invs, rows = [], [], [], []
            for i in range(self.b):
                case = self.cases[int(rng.integers(len(self.cases)))]
                src, lab, inv, row, _ = draw_aug_crop(rng, case, self.crop, i % 2 == 0, self.aug, self.extent)
                srcs.append(src)
                labs.append(lab)
                invs.append(inv)
                rows.append(row)
            params = {k: torch.from_numpy(np.stack([r[k] for r in rows])) for k in ("gain", "bias", "gamma", "noise_std")}
            params["inv"] = torch.from_numpy(np.stack(invs))
            params["seed"] = torch.tensor(int(rng.integers(1 << 62)), dtype=torch.int64)
            params["crop"] = torch.tensor(self.crop, dtype=torch.int64)
            yield torch.from_numpy(np.stack(srcs)), torch.from_numpy(np.stack(labs)), params

    def __iter__(self):
        rng = np.random.default_rng([self.seed, self.rank, self.epoch])
        if self.aug is not None:
            yield from self._augmented(rng)
            return
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
def synthetic_case(seed, index, shape, n_class, in_channels=1, head="sigmoid"):
    """A phantom, a fixed function of (seed, index): unit noise; class k is an ellipsoid (the K of them overlap: each is drawn around the first one's
    centre) inside which every channel is raised by 1.5 (k + 1).  -> Case with in-memory arrays.
    head='softmax': a LABEL MAP of n_class classes, the background (0) included -- the classes 1..n_class-1 are DISJOINT ellipsoids, one per slab of
    the first axis, inside which every channel is raised by 1.5 k."""
    rng = np.random.default_rng([int(seed), int(index)])
    shape = tuple(int(s) for s in shape)
    if head == "softmax":
        img = rng.standard_normal((in_channels,) + shape, dtype=np.float32)
        seg = np.zeros(shape, dtype=np.uint8)
        grid = np.meshgrid(*[np.arange(n, dtype=np.float32) for n in shape], indexing="ij")
        slab = shape[0] / float(n_class - 1)
        for k in range(1, n_class):
            lo = (k - 1) * slab
            centre = np.array([lo + rng.uniform(0.4, 0.6) * slab, rng.uniform(0.35, 0.65) * shape[1], rng.uniform(0.35, 0.65) * shape[2]])
            radii = np.array([rng.uniform(0.3, 0.5) * slab, rng.uniform(0.15, 0.3) * shape[1], rng.uniform(0.15, 0.3) * shape[2]])
            inside = (sum(((g - c) / r) ** 2 for g, c, r in zip(grid, centre, radii)) <= 1.0) & (grid[0] >= lo) & (grid[0] < lo + slab)
            seg[inside] = np.uint8(k)
            img[:, inside] += np.float32(1.5 * k)
        return Case("phantom%03d" % index, img, seg)
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


def write_synthetic(data_dir, names, shape, n_class, in_channels=1, seed=0, first_index=0, head="sigmoid"):
    """The phantoms as cases on disk (tests, smoke commands)."""
    os.makedirs(data_dir, exist_ok=True)
    for i, name in enumerate(names):
        c = synthetic_case(seed, first_index + i, shape, n_class, in_channels, head)
        np.save(os.path.join(data_dir, name + "_img.npy"), c.img)
        np.save(os.path.join(data_dir, name + "_seg.npy"), c.seg)


def synthetic_shape(crop):
    """The phantoms' size for a crop: no multiple of it, so that the tiling's shifted last patches are exercised."""
    return (crop[0] * 3 // 2, crop[1] * 5 // 4 - 4, crop[2] * 5 // 4)


def loaders(args, rank=0, world=1):
    """{'train': CropLoader, 'eval': TileLoader, 'test': TileLoader} for --data DIR | synthetic."""
    head = getattr(args, "head", "sigmoid")
    crop, K, C = parse_crop(args.crop), check_n_class(args.n_class, head), int(args.in_channels)
    if args.data == "synthetic":
        shape = synthetic_shape(crop)
        mk = lambda first, n: [synthetic_case(args.seed, first + i, shape, K, C, head) for i in range(n)]     # noqa: E731
        train, val, test = mk(0, 8), mk(1000, 2), mk(2000, 2)
    elif os.path.isdir(args.data):
        train, val, test = (open_cases(args.data, f, K, C, head=head) for f in ("train.txt", "val.txt", "test.txt"))
    else:
        raise SystemExit("--data must be 'synthetic' or a directory with <case>_img.npy / <case>_seg.npy and train.txt, val.txt, test.txt")
    steps = int(args.steps_per_epoch) or -(-len(train) // int(args.b))         # 0: one crop per training case and epoch
    return {"train": CropLoader(train, crop, args.b, steps, args.seed, rank, aug=parse_aug(args)),
            "eval": TileLoader(val, crop, args.b, rank, world), "test": TileLoader(test, crop, args.b, rank, world)}
