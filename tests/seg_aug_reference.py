"""TEST INFRASTRUCTURE: float64 numpy restatement of pcrl_seg_aug_resample (csrc/seg_augment.hip), the joint image / label resampling of 3D
segmentation crops.  Takes the SAME inputs as ops.seg_augment; not used by the product path.  Not a test file.

    output voxel i:   c = i + 0.5 - crop / 2        s = M c + t + extent / 2 - 0.5
    image   gain * T + bias, T the trilinear sample at s, a corner outside the source box contributing 0
    label   src_lab at n = floor(s + 0.5), 0x80 where n is outside the box
"""
import itertools

import numpy as np

NOT_COUNTED = 0x80


def coords(inv, extent, crop):
    """-> s float64 [B, 3, X, Y, Z]: the source coordinate of every output voxel; inv [B, 12] (rows (m0 m1 m2 t) of x, y, z)"""
    inv = np.asarray(inv, dtype=np.float64).reshape(-1, 3, 4)
    grid = np.meshgrid(*[np.arange(n, dtype=np.float64) + 0.5 - n / 2.0 for n in crop], indexing="ij")
    c = np.stack(grid).reshape(3, -1)                                                   # [3, V]
    centre = np.array([e / 2.0 - 0.5 for e in extent], dtype=np.float64)
    s = inv[:, :, :3] @ c + inv[:, :, 3:] + centre[None, :, None]
    return s.reshape((inv.shape[0], 3) + tuple(crop))


def corner_range(s):
    """-> (lo, hi) int64 [B, 3]: the smallest and the largest corner index floor(s), floor(s) + 1 that any output voxel touches, per sample and axis"""
    f = np.floor(s).astype(np.int64)
    return f.min(axis=(2, 3, 4)), f.max(axis=(2, 3, 4)) + 1


def ref_resample(src, src_lab, inv, gain, bias, crop, reverse=False):
    """src [B, C, Sx, Sy, Sz] (any float type; read as float64), src_lab uint8 [B, Sx, Sy, Sz], inv [B, 12], gain, bias [B, C]
    -> (y float64 [B, C, *crop], lab uint8 [B, *crop], s float64 [B, 3, *crop]); `reverse` walks the corners in the opposite order"""
    src = np.asarray(src).astype(np.float64)
    src_lab = np.asarray(src_lab)
    gain, bias = np.asarray(gain, dtype=np.float64), np.asarray(bias, dtype=np.float64)
    B, C = src.shape[:2]
    ext = src.shape[2:]
    s = coords(inv, ext, crop)
    f = np.floor(s)
    t = s - f
    f = f.astype(np.int64)
    T = np.zeros((B, C) + tuple(crop), dtype=np.float64)
    corners = list(itertools.product((0, 1), repeat=3))
    bi = np.arange(B).reshape(B, 1, 1, 1)
    for a in (corners[::-1] if reverse else corners):
        idx = [f[:, k] + a[k] for k in range(3)]
        inside = np.ones(idx[0].shape, dtype=bool)
        for k in range(3):
            inside &= (idx[k] >= 0) & (idx[k] < ext[k])
        w = np.ones_like(t[:, 0])
        for k in range(3):
            w = w * (t[:, k] if a[k] else 1.0 - t[:, k])
        cl = [np.clip(idx[k], 0, ext[k] - 1) for k in range(3)]
        for ch in range(C):
            T[:, ch] += np.where(inside, src[bi, ch, cl[0], cl[1], cl[2]], 0.0) * w
    y = gain.reshape(B, C, 1, 1, 1) * T + bias.reshape(B, C, 1, 1, 1)
    return y, nearest_labels(src_lab, s), s


def nearest_labels(src_lab, s):
    """src_lab uint8 [B, Sx, Sy, Sz] at n = floor(s + 0.5) per axis for coordinates s [B, 3, X, Y, Z]; 0x80 where n is outside the box"""
    src_lab = np.asarray(src_lab)
    ext = src_lab.shape[1:]
    bi = np.arange(src_lab.shape[0]).reshape(-1, 1, 1, 1)
    n = np.floor(s + 0.5).astype(np.int64)
    inside = np.ones(n[:, 0].shape, dtype=bool)
    for k in range(3):
        inside &= (n[:, k] >= 0) & (n[:, k] < ext[k])
    cl = [np.clip(n[:, k], 0, ext[k] - 1) for k in range(3)]
    return np.where(inside, src_lab[bi, cl[0], cl[1], cl[2]], NOT_COUNTED).astype(np.uint8)
