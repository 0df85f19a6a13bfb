"""Restatements of the sliding-window blend (csrc/seg_blend.hip) with numpy.  Not a test file.

blend32: the kernel's arithmetic in np.float32, one operation at a time and in the kernel's order -- per voxel the covering patches in ascending
(ix, iy, iz), w = (wx[i] * wy[j]) * wz[k], num = num + w * z, den = den + w.  Walking the PATCHES in ascending index and adding each one's box to the
volume visits every voxel's covering patches in exactly that order.
blend64: the weighted sums in float64 (the order does not matter at that precision), with sum |w z| and the number of covering patches per voxel.
"""
import numpy as np


def _boxes(axes, crop, shape):
    """(patch index, volume box, patch box) for every patch in x-major order; the boxes are clipped to the volume."""
    p = 0
    for a in axes[0]:
        for b in axes[1]:
            for c in axes[2]:
                vol = tuple(slice(s, min(s + n, m)) for s, n, m in zip((a, b, c), crop, shape))
                yield p, vol, tuple(slice(0, sl.stop - sl.start) for sl in vol)
                p += 1


def blend32(z, axes, weights, shape):
    """z float32 [P, cx, cy, cz, K]; axes: three start lists; weights: three float32 tables.  -> (num float32 [X, Y, Z, K], den float32 [X, Y, Z])"""
    z = np.asarray(z, dtype=np.float32)
    crop, K = z.shape[1:4], z.shape[4]
    wx, wy, wz = (np.asarray(w, dtype=np.float32) for w in weights)
    w3 = (wx[:, None, None] * wy[None, :, None]) * wz[None, None, :]
    assert w3.dtype == np.float32
    num, den = np.zeros(tuple(shape) + (K,), dtype=np.float32), np.zeros(tuple(shape), dtype=np.float32)
    for p, vol, box in _boxes(axes, crop, shape):
        w = w3[box]
        prod = w[..., None] * z[p][box]                 # float32 product, rounded
        num[vol] = num[vol] + prod                      # float32 sum, rounded
        den[vol] = den[vol] + w
    assert num.dtype == np.float32 and den.dtype == np.float32
    return num, den


def blend64(z, axes, weights, shape):
    """-> (num float64 [X, Y, Z, K], den float64 [X, Y, Z], sum |w z| float64 [X, Y, Z, K], covering patches int [X, Y, Z]); the weights are the
    float32 tables' values, their products taken in float64."""
    z = np.asarray(z, dtype=np.float64)
    crop, K = z.shape[1:4], z.shape[4]
    wx, wy, wz = (np.asarray(w, dtype=np.float64) for w in weights)
    w3 = wx[:, None, None] * wy[None, :, None] * wz[None, None, :]
    num, den = np.zeros(tuple(shape) + (K,)), np.zeros(tuple(shape))
    absum, cover = np.zeros(tuple(shape) + (K,)), np.zeros(tuple(shape), dtype=np.int64)
    for p, vol, box in _boxes(axes, crop, shape):
        w = w3[box]
        num[vol] += w[..., None] * z[p][box]
        absum[vol] += np.abs(w[..., None] * z[p][box])
        den[vol] += w
        cover[vol] += 1
    return num, den, absum, cover


def mask_of(num, labels=None):
    """uint8 [X, Y, Z]: bit k = (num_k >= 0); 0 where bit 7 of the label is set."""
    K = num.shape[-1]
    m = np.zeros(num.shape[:-1], dtype=np.uint8)
    for k in range(K):
        m |= ((num[..., k] >= 0).astype(np.uint8) << k).astype(np.uint8)
    if labels is not None:
        m[(labels & 0x80) != 0] = 0
    return m


def counts_of(mask, labels, K):
    """int64 [K, 3] = {TP, |pred|, |gt|} over the counted voxels (labels None: nothing labelled, everything counted)."""
    lab = np.zeros(mask.shape, dtype=np.uint8) if labels is None else labels
    on = (lab & 0x80) == 0
    out = np.zeros((K, 3), dtype=np.int64)
    for k in range(K):
        p, g = (((mask >> k) & 1) != 0) & on, (((lab >> k) & 1) != 0) & on
        out[k] = (int((p & g).sum()), int(p.sum()), int(g.sum()))
    return out
