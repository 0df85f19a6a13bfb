"""Input side of the 2D pre-training path: the reference's chest X-ray pre-task loader with the torchvision augmentations on the GPU.

Reference: `data.py:14-61` (DataGenerator.pcrlv2_chest_pretask), `datasets/chestDataset.py:13-48` (Pcrlv2ChestPretask), `utils.py:7-19`
(get_chest_list), `utils.py:60-98` (Cutout), `utils.py:139-148` (GaussianBlur), `train_2d.py:133-137` (how the batch is consumed).

Each sample is one image, read as `Image.open(path).convert('RGB')`, and yields (y1, y2, x, x2, [6 local views]):
  spatial chain   RandomResizedCrop(224, scale (0.3, 1)) -> RandomRotation(10) -> RandomHorizontalFlip, twice (global views);
                  the same with RandomResizedCrop(96, scale (0.05, 0.3)), six times (local views)
  targets x, x2   Normalize(ToTensor(global spatial view)), before any colour operation
  photometric     RandomGrayscale(0.2) -> RandomApply([GaussianBlur(sigma U[0.1, 2])], 0.5) -> ColorJitter(0.4, 0.4, 0.4, 0.4) -> ToTensor
                  -> Normalize(ImageNet mean / std); the global views then Cutout(3 holes of 32)

The workers only decode (the slot loader of pcrlv2_amd/data.py): uint8 pixels and (H, W, C) go straight into shared page-locked slots, one plane
for a mode-L image (almost all of NIH ChestX-ray14) and three otherwise.  The random parameters are drawn here, vectorised, from a seeded numpy
generator following torchvision's rules (the 10-attempt RandomResizedCrop rejection and its centre-crop fallback included) and shipped as one
int32 record per view with the batch's host-to-device copy -- nothing is read back.  The transforms are the hand-written gfx950 kernels of
csrc/augment2d.hip (`pcrl_aug2d_*`); there is no CPU fallback.

PINNED to Pillow.  On PIL images every torchvision transform of the chain hands its arithmetic to Pillow (the resampler, the nearest affine
transform, the box blur, Image.blend under ImageEnhance, the HSV conversions); the kernels restate that arithmetic and are tested uint8 for
uint8 against Pillow's own output (tests/chest_aug_reference.py, tests/golden/chest_aug_*.npz).  NOT pinned: torchvision's order of random
draws (torchvision is absent, and the reference draws in unseeded DataLoader workers anyway) -- only the rules and distributions match.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from ._lib import call_on_stream
from .data import AugmentedLoader, _LazyLoaders, eval_shard

NPARAM = 40            # PCRL_AUG2D_NPARAM: the per-view record of pcrl_aug2d_* (layout in include/pcrl_hip.h)
(P_SRC, P_H, P_W, P_C, P_J, P_I, P_CW, P_CH, P_A0, P_A1, P_A2, P_A3, P_A4, P_A5, P_FLIP, P_GRAY, P_BLUR, P_BR, P_WW, P_FW,
 P_NOPS, P_ORDER, P_BRI, P_CON, P_SAT, P_HUE, P_NHOLES, P_HOLES) = range(28)
P_INTER = P_HOLES + 12

GLOBAL_SIZE, LOCAL_SIZE, NUM_LOCAL = 224, 96, 6                       # data.py:20, 25; chestDataset.py:13
GLOBAL_SCALE, LOCAL_SCALE = (0.3, 1.0), (0.05, 0.3)
RATIO = (3.0 / 4.0, 4.0 / 3.0)                                        # RandomResizedCrop's default ratio
DEGREES = 10.0                                                        # RandomRotation(10)
P_GRAYSCALE, P_BLUR_APPLY, SIGMA = 0.2, 0.5, (0.1, 2.0)               # data.py:31-32, utils.py:142
JITTER = 0.4                                                          # ColorJitter(0.4, 0.4, 0.4, 0.4)
CUTOUT_HOLES, CUTOUT_LENGTH = 3, 32                                   # data.py:44


# ---------------------------------------------------------------------------------------------------------------
# Pillow's parameter arithmetic (done on the host, in Python doubles / numpy float32 as Pillow's C code does it)
# ---------------------------------------------------------------------------------------------------------------
def rotate_fixed(angle: float, w: int, h: int):
    """Image.rotate(angle, NEAREST, expand=False) of a w x h image -> the 16.16 fixed-point affine (a0, .., a5) of Geometry.c's affine_fixed:
    output pixel (x, y) reads input ((a2 + y a1 + x a0) >> 16, (a5 + y a4 + x a3) >> 16)."""
    angle = angle % 360.0
    c = None
    if angle != 0:
        rad = -math.radians(angle)
        m = [round(math.cos(rad), 15), round(math.sin(rad), 15), 0.0, round(-math.sin(rad), 15), round(math.cos(rad), 15), 0.0]
        if m[1] != 0 or m[3] != 0:
            cx, cy = w / 2, h / 2
            m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
            m[2] += cx
            m[5] += cy
            c = m
    if c is None:          # angle 0 (Image.copy) or a rotation whose sine rounds to zero: the identity
        c = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]

    def fix(v):
        return int(math.floor(v * 65536.0 + 0.5))
    return (fix(c[0]), fix(c[1]), fix(c[2] + c[0] * 0.5 + c[1] * 0.5), fix(c[3]), fix(c[4]), fix(c[5] + c[3] * 0.5 + c[4] * 0.5))


def blur_params(sigma: float, passes: int = 3):
    """ImageFilter.GaussianBlur(radius=sigma) -> (integer box radius, ww, fw) of BoxBlur.c (_gaussian_blur_radius in float32, then
    ImagingHorizontalBoxBlur's 8.24 weights)."""
    f = np.float32
    r = f(sigma)
    sigma2 = f(r * r) / f(passes)
    L = f(math.sqrt(12.0 * float(sigma2) + 1.0))
    l = f(math.floor((float(L) - 1.0) / 2.0))
    a = (f(2) * l + f(1)) * (l * (l + f(1)) - f(3) * sigma2)
    a = a / (f(6) * (sigma2 - (l + f(1)) * (l + f(1))))
    radius = f(l + a)
    ww = int(f(1 << 24) / (radius * f(2) + f(1)))
    ri = int(radius)
    fw = ((1 << 24) - (ri * 2 + 1) * ww) // 2
    return ri, ww, fw


def hue_shift(hue: float) -> int:
    """torchvision adjust_hue on a PIL image: np.array(hue * 255).astype(np.uint8) -- truncated toward zero, then wrapped."""
    return int(math.trunc(hue * 255.0)) % 256


def _f32_bits(x):
    return np.asarray(x, dtype=np.float32).view(np.int32)


# ---------------------------------------------------------------------------------------------------------------
# Vectorised draws (torchvision's rules, this engine's generator)
# ---------------------------------------------------------------------------------------------------------------
def draw_crops(rng, H, W, scale, ratio=RATIO, attempts=10):
    """RandomResizedCrop.get_params for every view at once: H, W int arrays [N] -> (i, j, h, w) int arrays.  Up to `attempts` draws of
    area * U(scale) and exp(U(log ratio)); w = round(sqrt(A r)), h = round(sqrt(A / r)) (Python's round: half to even), accepted when
    0 < w <= W and 0 < h <= H; then i ~ randint(0, H - h + 1), j ~ randint(0, W - w + 1).  No accepted draw: the centre crop with the
    ratio clamped to `ratio`."""
    H, W = np.asarray(H, np.int64), np.asarray(W, np.int64)
    N = H.shape[0]
    area = (H * W).astype(np.float64)
    target = area[:, None] * rng.uniform(scale[0], scale[1], (N, attempts))
    ar = np.exp(rng.uniform(math.log(ratio[0]), math.log(ratio[1]), (N, attempts)))
    w = np.rint(np.sqrt(target * ar)).astype(np.int64)
    h = np.rint(np.sqrt(target / ar)).astype(np.int64)
    ok = (w > 0) & (w <= W[:, None]) & (h > 0) & (h <= H[:, None])
    first = np.argmax(ok, axis=1)
    hit = ok[np.arange(N), first]
    w, h = w[np.arange(N), first], h[np.arange(N), first]
    ui, uj = rng.random(N), rng.random(N)
    i = np.minimum((ui * (H - h + 1)).astype(np.int64), H - h)
    j = np.minimum((uj * (W - w + 1)).astype(np.int64), W - w)
    # fallback: centre crop (torchvision's round(): half to even, as np.rint)
    in_ratio = W / H
    fw = np.where(in_ratio < min(ratio), W, np.where(in_ratio > max(ratio), np.rint(H * max(ratio)).astype(np.int64), W))
    fh = np.where(in_ratio < min(ratio), np.rint(W / min(ratio)).astype(np.int64), H)
    w, h = np.where(hit, w, fw), np.where(hit, h, fh)
    i, j = np.where(hit, i, (H - fh) // 2), np.where(hit, j, (W - fw) // 2)
    return i, j, h, w


def draw_views(rng, H, W, C, S, scale, cutout, raw=None):
    """All random parameters of N views of side S (one per entry of H, W, C) -> int32 records [N, NPARAM] (offsets left 0).  `raw`, a dict,
    receives the draws in torchvision's own terms (angle, sigma, factors, hue) for the Pillow fixtures."""
    N = len(H)
    rec = np.zeros((N, NPARAM), np.int64)
    rec[:, P_H], rec[:, P_W], rec[:, P_C] = H, W, C
    i, j, h, w = draw_crops(rng, H, W, scale)
    rec[:, P_J], rec[:, P_I], rec[:, P_CW], rec[:, P_CH] = j, i, w, h
    angles = rng.uniform(-DEGREES, DEGREES, N)
    rec[:, P_A0:P_A5 + 1] = [rotate_fixed(float(a), S, S) for a in angles]
    rec[:, P_FLIP] = rng.random(N) < 0.5
    rec[:, P_GRAY] = rng.random(N) < P_GRAYSCALE
    rec[:, P_BLUR] = rng.random(N) <= P_BLUR_APPLY            # RandomApply: `if self.p < torch.rand(1): return img`
    sig = rng.uniform(SIGMA[0], SIGMA[1], N)
    rec[:, P_BR:P_FW + 1] = [blur_params(float(s)) for s in sig]
    perm = np.argsort(rng.random((N, 4)), axis=1)             # torch.randperm(4) per view
    rec[:, P_NOPS] = 4
    rec[:, P_ORDER] = perm[:, 0] | (perm[:, 1] << 4) | (perm[:, 2] << 8) | (perm[:, 3] << 12)
    f = rng.uniform(1.0 - JITTER, 1.0 + JITTER, (N, 3))
    rec[:, P_BRI:P_SAT + 1] = _f32_bits(f)
    hf = rng.uniform(-JITTER, JITTER, N)
    rec[:, P_HUE] = [hue_shift(float(x)) for x in hf]
    if cutout:
        rec[:, P_NHOLES] = CUTOUT_HOLES
        cy, cx = rng.integers(0, S, (N, CUTOUT_HOLES)), rng.integers(0, S, (N, CUTOUT_HOLES))
        half = CUTOUT_LENGTH // 2
        holes = np.stack([np.clip(cy - half, 0, S), np.clip(cy + half, 0, S), np.clip(cx - half, 0, S), np.clip(cx + half, 0, S)], axis=2)
        rec[:, P_HOLES:P_HOLES + 4 * CUTOUT_HOLES] = holes.reshape(N, -1)
    if raw is not None:
        raw.update(angle=angles, sigma=sig, factors=f, hue=hf)
    return rec


def pack_offsets(rec, src_offsets, sample, S):
    """Fill the source and intermediate offsets of a view group in place -> bytes of intermediate it needs."""
    rec[:, P_SRC] = np.asarray(src_offsets, np.int64)[sample]
    sizes = rec[:, P_CH] * S * rec[:, P_C]
    off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    rec[:, P_INTER] = off
    total = int(sizes.sum())
    if total >= 2**31 or int(rec[:, P_SRC].max(initial=0)) >= 2**31:
        raise ValueError("aug2d: a batch needs more than 2 GiB of source or intermediate bytes; lower --b")
    return total


# ---------------------------------------------------------------------------------------------------------------
# Device side
# ---------------------------------------------------------------------------------------------------------------
def apply_views(src, rec_dev, rec_host, S, with_target, u8_out=None):
    """Runs the three kernels over one group of views of side S: src = packed uint8 sources on the device, rec_dev / rec_host = the
    records (int32) on the device and on the host.  -> (out [V,3,S,S] float32, target [V,3,S,S] float32 or None)."""
    V = rec_host.shape[0]
    dev = src.device
    inter = torch.empty(int((rec_host[:, P_CH].astype(np.int64) * S * rec_host[:, P_C]).sum()), dtype=torch.uint8, device=dev)
    call_on_stream("pcrl_aug2d_hresample", src, rec_dev, inter, V, S, int(rec_host[:, P_CH].max()))
    view = torch.empty((V, 3, S, S), dtype=torch.uint8, device=dev)
    target = torch.empty((V, 3, S, S), dtype=torch.float32, device=dev) if with_target else None
    call_on_stream("pcrl_aug2d_spatial", inter, rec_dev, view, target, V, S)
    out = torch.empty((V, 3, S, S), dtype=torch.float32, device=dev)
    call_on_stream("pcrl_aug2d_photometric", view, rec_dev, out, u8_out, V, S)
    return out, target


class GpuChestAugment:
    """data.py:14-61 + chestDataset.py:31-48 as one batched device pass.  __call__(pixels [B, cap] uint8, dims [B, 3] int32 (H, W, C) on the
    host) -> (y1, y2, x, x2, [6 local views]) of [B,3,224,224] / [B,3,96,96] float32."""

    def __init__(self, device, seed=0):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("GpuChestAugment runs on the GPU (libpcrl_hip.so); there is no CPU fallback")
        self.rng = np.random.default_rng(seed)

    def reset_rng(self, seed):
        """The draws start over from `seed` (AugmentedLoader.reset_rng: every validation pass draws the same augmentations)."""
        self.rng = np.random.default_rng(seed)

    def draw(self, dims):
        """-> (records [8B, NPARAM] int64, src offsets [B]): the B * 2 global views (view k * B + n is sample n's k-th), then the B * 6 local ones."""
        dims = np.asarray(dims, np.int64)
        B = dims.shape[0]
        H, W, C = dims[:, 0], dims[:, 1], dims[:, 2]
        sizes = H * W * C
        offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        g = draw_views(self.rng, np.tile(H, 2), np.tile(W, 2), np.tile(C, 2), GLOBAL_SIZE, GLOBAL_SCALE, cutout=True)
        loc = draw_views(self.rng, np.tile(H, NUM_LOCAL), np.tile(W, NUM_LOCAL), np.tile(C, NUM_LOCAL), LOCAL_SIZE, LOCAL_SCALE, cutout=False)
        pack_offsets(g, offs, np.tile(np.arange(B), 2), GLOBAL_SIZE)
        pack_offsets(loc, offs, np.tile(np.arange(B), NUM_LOCAL), LOCAL_SIZE)
        return np.concatenate([g, loc]), offs, sizes

    @torch.no_grad()
    def __call__(self, pixels, dims):
        dims_h = dims.numpy() if torch.is_tensor(dims) else np.asarray(dims)
        B = dims_h.shape[0]
        rec, offs, sizes = self.draw(dims_h)
        rec_h = torch.from_numpy(rec.astype(np.int32))
        if self.device.type == "cuda":
            rec_h = rec_h.pin_memory()
        rec_d = rec_h.to(self.device, non_blocking=True)
        src = torch.empty(int(sizes.sum()), dtype=torch.uint8, device=self.device)
        if torch.is_tensor(pixels) and pixels.dim() == 2 and B > 0 and bool((sizes == pixels.shape[1]).all()):
            src.view(B, -1).copy_(pixels, non_blocking=True)          # every sample fills its row: one copy
        else:
            for n in range(B):
                src[int(offs[n]):int(offs[n] + sizes[n])].copy_(pixels[n, :int(sizes[n])], non_blocking=True)
        ng = 2 * B
        gout, gtgt = apply_views(src, rec_d[:ng], rec[:ng], GLOBAL_SIZE, True)
        lout, _ = apply_views(src, rec_d[ng:], rec[ng:], LOCAL_SIZE, False)
        gout, gtgt = gout.view(2, B, 3, GLOBAL_SIZE, GLOBAL_SIZE), gtgt.view(2, B, 3, GLOBAL_SIZE, GLOBAL_SIZE)
        lout = lout.view(NUM_LOCAL, B, 3, LOCAL_SIZE, LOCAL_SIZE)
        return gout[0], gout[1], gtgt[0], gtgt[1], [lout[k] for k in range(NUM_LOCAL)]


# ---------------------------------------------------------------------------------------------------------------
# Decode workers and the loader
# ---------------------------------------------------------------------------------------------------------------
def chest_file_list(data_dir: str, ratio: float, list_file: str = "train_val_txt/chest_train.txt"):
    """utils.get_chest_list + data.py:47-48: `name label...` lines of `list_file` (if it exists: the reference requires it) joined to
    `data_dir`, otherwise every *.png under `data_dir`, sorted; the first `ratio` of the list is kept.  A listed file that is missing is an error."""
    if os.path.exists(list_file):
        with open(list_file) as f:
            names = [os.path.join(data_dir, line.split()[0]) for line in f if line.split()]
        missing = [p for p in names if not os.path.isfile(p)]
        if missing:
            raise FileNotFoundError(f"{len(missing)} file(s) of {list_file} are not in {data_dir}, e.g. {missing[0]}")
    else:
        names = sorted(os.path.join(root, f) for root, _, files in os.walk(data_dir) for f in files if f.lower().endswith(".png"))
    return names[:int(len(names) * ratio)]


def decode(path):
    """Image.open(path).convert('RGB') as chestDataset.py:34 does, kept as ONE plane when the image is mode L (convert('RGB') would only
    replicate it) -> uint8 array [H, W, C]."""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode != "L":
            im = im.convert("RGB")
        a = np.array(im, dtype=np.uint8)
    return a.reshape(a.shape[0], a.shape[1], -1)


class ChestImages(torch.utils.data.Dataset):
    """Decoded images for a DataLoader without slots: (pixels [cap] uint8, dims [3] int32)."""

    def __init__(self, files, cap):
        self.files, self.cap = list(files), cap

    def __len__(self):
        return len(self.files)

    def __getitem__(self, i):
        a = decode(self.files[i])
        if a.size > self.cap:
            raise ValueError(f"{self.files[i]}: {a.shape} does not fit the {self.cap}-byte image slots (sized from the first file)")
        pix = torch.zeros(self.cap, dtype=torch.uint8)
        pix[:a.size] = torch.from_numpy(a.reshape(-1))
        return pix, torch.tensor(a.shape, dtype=torch.int32)


class _SlotImages(ChestImages):
    """ChestImages whose workers write the pixels and (H, W, C) STRAIGHT into a slot of the shared, page-locked batch buffers (key = (slot, row,
    file index)) and send back only (slot, row): data._SlotCrops for images."""

    def __init__(self, files, pix_buf, dims_buf):
        super().__init__(files, pix_buf.shape[2])
        self.pix, self.dims = pix_buf, dims_buf

    def __getitem__(self, key):
        slot, row, i = key
        a = decode(self.files[i])
        if a.size > self.cap:
            raise ValueError(f"{self.files[i]}: {a.shape} does not fit the {self.cap}-byte image slots (sized from the first file)")
        self.pix[slot, row, :a.size] = torch.from_numpy(a.reshape(-1))
        self.dims[slot, row] = torch.tensor(a.shape, dtype=torch.int32)
        return slot, row


class ChestKind:
    """What AugmentedLoader needs to know about the chest pre-task samples: slot buffers of `side x side x 3` bytes per image, side = the larger
    side of the first file."""

    def __init__(self, files):
        from PIL import Image
        with Image.open(files[0]) as im:
            side = max(im.size)
        self.cap = side * side * 3

    def slot_shapes(self):
        return [((self.cap,), torch.uint8), ((3,), torch.int32)]

    def slot_dataset(self, files, bufs):
        return _SlotImages(files, *bufs)

    def dataset(self, files):
        return ChestImages(files, self.cap)

    def augment(self, device, seed):
        return GpuChestAugment(device, seed)

    @staticmethod
    def host_side(i):
        return i == 1           # the dims stay on the host (they size the draws), the pixels go to the device


def chest_valid_list(data_dir: str, list_file: str):
    """The held-out images: the `name label...` lines of `list_file` (the reference ships train_val_txt/chest_valid.txt and never reads it) joined
    to `data_dir`.  A missing list is an error -- the held-out set is never carved out of the training list; so is a listed file that is missing."""
    if not os.path.exists(list_file):
        raise SystemExit(f"--val_every needs the held-out image list {list_file} (--val_list), which does not exist; "
                         "the held-out set is not carved out of the training list")
    with open(list_file) as f:
        names = [os.path.join(data_dir, line.split()[0]) for line in f if line.split()]
    missing = [p for p in names if not os.path.isfile(p)]
    if missing:
        raise FileNotFoundError(f"{len(missing)} file(s) of {list_file} are not in {data_dir}, e.g. {missing[0]}")
    if not names:
        raise SystemExit(f"the held-out image list {list_file} is empty")
    return names


def chest_pretask_loaders(args, device=None):
    """`DataGenerator(args).pcrlv2_chest_pretask()` (data.py:14-61): {'train': ..., 'eval': the same loader}.  With --val_every > 0 'eval' is instead
    this rank's contiguous shard of the held-out list (--val_list), unshuffled, built when somebody first asks for it (data._LazyLoaders)."""
    device = device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu")
    files = chest_file_list(args.data, args.ratio)
    print(f"total train images {len(files)}")
    if not files:
        raise SystemExit(f"no chest images found under {args.data}")
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    seed = getattr(args, "seed", 0)
    if world > 1:                     # equal shards, ragged last batch dropped: see data.luna_pretask_loaders
        files = files[:len(files) - len(files) % world]
    train = AugmentedLoader(files[rank::world], args.b, args.workers, device, True, seed + rank, drop_last=world > 1, kind=ChestKind(files))
    if int(getattr(args, "val_every", 0) or 0) <= 0:
        return {"train": train, "eval": train}
    valid = eval_shard(chest_valid_list(args.data, getattr(args, "val_list", "./train_val_txt/chest_valid.txt")), rank, world)
    print(f"valid images {len(valid)} (this rank)")

    def make_eval():
        ev = AugmentedLoader(valid, args.b, args.workers, device, False, seed, kind=ChestKind(valid))
        ev.sharded = True       # built for this rank: train_2d.validate takes it whole
        return ev

    return _LazyLoaders(train, make_eval)


# ---------------------------------------------------------------------------------------------------------------
# Supervised fine-tuning: the labelled lists, the labelled slot loader, the training and the evaluation transform
# ---------------------------------------------------------------------------------------------------------------
MAX_CLASSES = 31           # the labels of a sample travel through the slots as one non-negative int32 bitmask


def chest_labelled_list(data_dir: str, list_file: str):
    """utils.get_chest_list (utils.py:7-19): the `name l0 ... l(K-1)` lines of `list_file` -> (names joined to `data_dir`, labels uint8 [n, K]).
    Every line must carry the same number K <= 31 of 0/1 labels; a missing list is an error."""
    if not os.path.exists(list_file):
        raise SystemExit(f"the labelled image list {list_file} does not exist")
    names, rows = [], []
    with open(list_file) as f:
        for ln, line in enumerate(f, start=1):
            items = line.split()
            if not items:
                continue
            try:
                lab = [int(v) for v in items[1:]]
            except ValueError:
                raise ValueError(f"{list_file}:{ln}: labels must be integers") from None
            if any(v not in (0, 1) for v in lab):
                raise ValueError(f"{list_file}:{ln}: labels must be 0 or 1")
            if rows and len(lab) != len(rows[0]):
                raise ValueError(f"{list_file}:{ln}: {len(lab)} labels where the lines before have {len(rows[0])}")
            names.append(os.path.join(data_dir, items[0]))
            rows.append(lab)
    K = len(rows[0]) if rows else 0
    if rows and not 1 <= K <= MAX_CLASSES:
        raise ValueError(f"{list_file}: {K} labels per line; 1..{MAX_CLASSES} are supported")
    return names, np.asarray(rows, dtype=np.uint8).reshape(len(rows), K)


def pack_labels(labels) -> np.ndarray:
    """uint8 [n, K] (K <= 31) -> int32 [n] bitmasks, bit k = label k."""
    labels = np.asarray(labels, dtype=np.uint8)
    n, K = labels.shape
    if K > MAX_CLASSES:
        raise ValueError(f"{K} labels do not fit the int32 bitmask ({MAX_CLASSES} at most)")
    return ((labels != 0).astype(np.int64) << np.arange(K, dtype=np.int64)).sum(axis=1).astype(np.int32)


def unpack_labels(masks, K: int) -> np.ndarray:
    """int32 [n] bitmasks -> uint8 [n, K]."""
    masks = np.asarray(masks, dtype=np.int64).reshape(-1, 1)
    return ((masks >> np.arange(K, dtype=np.int64)) & 1).astype(np.uint8)


def chest_finetune_split(data_dir: str, ratio: float, list_file: str = "train_val_txt/chest_train.txt"):
    """The supervised training set: the LAST 1 - ratio of the training list, `names[int(len * ratio):]` (utils.get_luna_finetune_list's rule; the README:
    "top K% images for pre-training and last (100-K)% for fine-tuning") -- the complement of chest_file_list's.  -> (names, labels uint8 [n, K])"""
    names, labels = chest_labelled_list(data_dir, list_file)
    cut = int(len(names) * ratio)
    names, labels = names[cut:], labels[cut:]
    if not names:
        raise SystemExit(f"--ratio {ratio} leaves no image of {list_file} for fine-tuning (the last 1 - ratio of the list is the supervised training set); "
                         "lower --ratio")
    return names, labels


def eval_records(dims, S=GLOBAL_SIZE):
    """The view records of the EVALUATION transform Resize((S, S)) (bilinear) -> ToTensor -> Normalize, expressed for the pre-task's two spatial
    kernels: the crop is the whole image, the rotation is the angle-0 identity, no flip.  dims: [B, >=3] (H, W, C) -> int64 [B, NPARAM] (offsets left 0)."""
    dims = np.asarray(dims, np.int64)
    rec = np.zeros((dims.shape[0], NPARAM), np.int64)
    rec[:, P_H], rec[:, P_W], rec[:, P_C] = dims[:, 0], dims[:, 1], dims[:, 2]
    rec[:, P_CW], rec[:, P_CH] = dims[:, 1], dims[:, 0]
    rec[:, P_A0:P_A5 + 1] = rotate_fixed(0.0, S, S)
    return rec


def apply_spatial(src, rec_dev, rec_host, S):
    """The two spatial kernels alone (no photometric launch) over one group of views: -> (view uint8 [V,3,S,S] (plane 0 only for a one-plane source),
    Normalize(ToTensor(view)) float32 [V,3,S,S])."""
    V = rec_host.shape[0]
    dev = src.device
    inter = torch.empty(int((rec_host[:, P_CH].astype(np.int64) * S * rec_host[:, P_C]).sum()), dtype=torch.uint8, device=dev)
    call_on_stream("pcrl_aug2d_hresample", src, rec_dev, inter, V, S, int(rec_host[:, P_CH].max()))
    view = torch.empty((V, 3, S, S), dtype=torch.uint8, device=dev)
    target = torch.empty((V, 3, S, S), dtype=torch.float32, device=dev)
    call_on_stream("pcrl_aug2d_spatial", inter, rec_dev, view, target, V, S)
    return view, target


class GpuChestLabelledAugment(GpuChestAugment):
    """__call__(pixels [B, cap] uint8, record [B, 4] int32 (H, W, C, label bitmask) on the host) -> (x [B,3,224,224] float32, y [B,K] uint8 on the device).
    train: RandomResizedCrop(224, scale (0.3, 1)) -> RandomRotation(10) -> RandomHorizontalFlip -> ToTensor -> Normalize -- the pre-task's un-jittered
    target; eval: Resize((224, 224)) -> ToTensor -> Normalize (eval_records).  Two launches either way."""

    def __init__(self, device, seed, n_class, train):
        super().__init__(device, seed)
        self.n_class, self.train = int(n_class), bool(train)

    def records(self, dims):
        dims = np.asarray(dims, np.int64)
        H, W, C = dims[:, 0], dims[:, 1], dims[:, 2]
        sizes = H * W * C
        offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        rec = draw_views(self.rng, H, W, C, GLOBAL_SIZE, GLOBAL_SCALE, cutout=False) if self.train else eval_records(dims)
        pack_offsets(rec, offs, np.arange(dims.shape[0]), GLOBAL_SIZE)
        return rec, offs, sizes

    @torch.no_grad()
    def __call__(self, pixels, record):
        rec4 = record.numpy() if torch.is_tensor(record) else np.asarray(record)
        B = rec4.shape[0]
        rec, offs, sizes = self.records(rec4[:, :3])
        both = np.concatenate([rec.astype(np.int32).reshape(-1), unpack_labels(rec4[:, 3], self.n_class).astype(np.int32).reshape(-1)])
        host = torch.from_numpy(both)
        if self.device.type == "cuda":
            host = host.pin_memory()
        dev = host.to(self.device, non_blocking=True)          # the records and the labels in one host-to-device copy
        rec_d, y = dev[:rec.size].view(B, NPARAM), dev[rec.size:].view(B, self.n_class).to(torch.uint8)
        src = torch.empty(int(sizes.sum()), dtype=torch.uint8, device=self.device)
        if torch.is_tensor(pixels) and pixels.dim() == 2 and B > 0 and bool((sizes == pixels.shape[1]).all()):
            src.view(B, -1).copy_(pixels, non_blocking=True)
        else:
            for n in range(B):
                src[int(offs[n]):int(offs[n] + sizes[n])].copy_(pixels[n, :int(sizes[n])], non_blocking=True)
        _view, x = apply_spatial(src, rec_d, rec, GLOBAL_SIZE)
        return x, y


class LabelledImages(ChestImages):
    """ChestImages over (path, label bitmask) entries: (pixels [cap] uint8, (H, W, C, bitmask) int32)."""

    def __init__(self, entries, cap):
        super().__init__([e[0] for e in entries], cap)
        self.masks = [int(e[1]) for e in entries]

    def __getitem__(self, i):
        pix, dims = super().__getitem__(i)
        return pix, torch.cat([dims, torch.tensor([self.masks[i]], dtype=torch.int32)])


class _SlotLabelledImages(_SlotImages):
    """_SlotImages over (path, label bitmask) entries: the slot's int32 record is (H, W, C, bitmask)."""

    def __init__(self, entries, pix_buf, rec_buf):
        super().__init__([e[0] for e in entries], pix_buf, rec_buf)
        self.masks = [int(e[1]) for e in entries]

    def __getitem__(self, key):
        slot, row, i = key
        a = decode(self.files[i])
        if a.size > self.cap:
            raise ValueError(f"{self.files[i]}: {a.shape} does not fit the {self.cap}-byte image slots (sized from the first file)")
        self.pix[slot, row, :a.size] = torch.from_numpy(a.reshape(-1))
        self.dims[slot, row] = torch.tensor(tuple(a.shape) + (self.masks[i],), dtype=torch.int32)
        return slot, row


class ChestLabelledKind(ChestKind):
    """ChestKind whose samples carry their labels through AugmentedLoader's slots as they are: the loader's `files` are (path, label bitmask) entries
    (labelled_entries), the host-side per-sample record is (H, W, C, bitmask) int32 [4], and the augment object unpacks it."""

    def __init__(self, entries, n_class, train):
        super().__init__([e[0] for e in entries])
        self.n_class, self.train = int(n_class), bool(train)

    def slot_shapes(self):
        return [((self.cap,), torch.uint8), ((4,), torch.int32)]

    def slot_dataset(self, files, bufs):
        return _SlotLabelledImages(files, *bufs)

    def dataset(self, files):
        return LabelledImages(files, self.cap)

    def augment(self, device, seed):
        return GpuChestLabelledAugment(device, seed, self.n_class, self.train)


def labelled_entries(names, labels):
    return list(zip(names, pack_labels(labels).tolist()))


class _LazyBuilt(dict):
    """A dict of loaders whose entries are built -- worker processes, shared batch slots, list files read -- when first asked for."""

    def __init__(self, ready, makers):
        super().__init__(ready)
        self._makers = dict(makers)
        for k in makers:
            super().__setitem__(k, None)

    def __getitem__(self, key):
        make = self._makers.pop(key, None)
        if make is not None:
            super().__setitem__(key, make())
        return super().__getitem__(key)

    def get(self, key, default=None):
        return self[key] if key in self else default


def chest_finetune_loaders(args, device=None):
    """{'train', 'eval', 'test'} for --phase finetune / scratch: the last 1 - ratio of ./train_val_txt/chest_train.txt with the training transform (shuffled;
    one equal shard per rank), --val_list and --test_list with the evaluation transform (this rank's contiguous shard, unshuffled; built -- and their
    list files read -- on first use).  Every loader yields (x [B,3,224,224] float32, y [B,K] uint8) on the device."""
    device = device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu")
    K = int(getattr(args, "n_class", 14))
    names, labels = chest_finetune_split(args.data, args.ratio)
    if labels.shape[1] != K:
        raise SystemExit(f"./train_val_txt/chest_train.txt carries {labels.shape[1]} labels per line, --n_class is {K}")
    missing = [p for p in names if not os.path.isfile(p)]
    if missing:
        raise FileNotFoundError(f"{len(missing)} file(s) of train_val_txt/chest_train.txt are not in {args.data}, e.g. {missing[0]}")
    print(f"total fine-tuning images {len(names)}")
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    seed = getattr(args, "seed", 0)
    entries = labelled_entries(names, labels)
    if world > 1:
        entries = entries[:len(entries) - len(entries) % world]
    train = AugmentedLoader(entries[rank::world], args.b, args.workers, device, True, seed + rank, drop_last=world > 1, kind=ChestLabelledKind(entries, K, True))

    def held_out(list_file, flag):
        def make():
            if not os.path.exists(list_file):
                raise SystemExit(f"the labelled image list {list_file} ({flag}) does not exist")
            n, lab = chest_labelled_list(args.data, list_file)
            if not n:
                raise SystemExit(f"the labelled image list {list_file} ({flag}) is empty")
            if lab.shape[1] != K:
                raise SystemExit(f"{list_file} carries {lab.shape[1]} labels per line, --n_class is {K}")
            gone = [p for p in n if not os.path.isfile(p)]
            if gone:
                raise FileNotFoundError(f"{len(gone)} file(s) of {list_file} are not in {args.data}, e.g. {gone[0]}")
            part = eval_shard(labelled_entries(n, lab), rank, world)
            ev = AugmentedLoader(part, args.b, args.workers, device, False, seed, kind=ChestLabelledKind(part or labelled_entries(n, lab), K, False))
            ev.sharded = True
            return ev
        return make

    return _LazyBuilt({"train": train}, {"eval": held_out(getattr(args, "val_list", "./train_val_txt/chest_valid.txt"), "--val_list"),
                                         "test": held_out(getattr(args, "test_list", "./train_val_txt/chest_test.txt"), "--test_list")})
