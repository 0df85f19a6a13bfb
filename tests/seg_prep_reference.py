"""float64 numpy restatement of csrc/seg_prep.hip and of the host arithmetic of pcrlv2_amd/seg_prep.py, written independently of both.

Volumes here are in DISK order, [C, Z, Y, X] and [Z, Y, X], as the kernels take them; outputs in project order [C, X', Y', Z'] / [X', Y', Z'].
The image sum follows the order the kernel documents -- corners with the last axis fastest, ((u * wx) * wy) * wz added to 0.0 one at a time -- so
the comparison with the device is bit for bit; against scipy.ndimage.zoom(order=1, mode='nearest', grid_mode=True) it is held at 1e-12
(test_seg_prep_cpu.py), labels exactly.
"""
import math

import numpy as np


def n_out(n_in, spacing_in, spacing_out):
    return max(1, int(np.round(np.float64(n_in) * np.float64(spacing_in) / np.float64(spacing_out))))


def axis(n_in, n_o):
    """-> i0, i1, w0, w1, nn for n_in -> n_o samples: grid_mode coordinates clamped to the first and last sample ('nearest')."""
    i0, i1, w0, w1, nn = [], [], [], [], []
    for o in range(n_o):
        cc = (np.float64(o) + 0.5) * (np.float64(n_in) / np.float64(n_o)) - 0.5
        c = min(max(cc, np.float64(0.0)), np.float64(n_in - 1))
        f = math.floor(c)
        t = c - f
        i0.append(int(f))
        i1.append(min(int(f) + 1, n_in - 1))
        w0.append(np.float64(1.0) - t)
        w1.append(np.float64(1.0) - w0[-1])
        nn.append(min(max(int(math.floor(cc + 0.5)), 0), n_in - 1))
    return np.array(i0), np.array(i1), np.array(w0, dtype=np.float64), np.array(w1, dtype=np.float64), np.array(nn)


def mask_of(src):
    """[C, Z, Y, X] -> bool [Z, Y, X]: any channel != 0."""
    return (np.asarray(src) != 0).any(axis=0)


def scan(src):
    """-> (x0, x1, y0, y1, z0, z1, count, non-finite) with the half-open box; empty: lower bounds 0x7fffffff, upper bounds 0."""
    m = mask_of(src)
    bad = int((~np.isfinite(np.asarray(src, dtype=np.float64))).sum())
    if not m.any():
        return (0x7FFFFFFF, 0, 0x7FFFFFFF, 0, 0x7FFFFFFF, 0, 0, bad)
    z, y, x = np.nonzero(m)
    return (int(x.min()), int(x.max()) + 1, int(y.min()), int(y.max()) + 1, int(z.min()), int(z.max()) + 1, int(m.sum()), bad)


def masked_values(src, ch, use_mask):
    v = np.asarray(src[ch])
    return v[mask_of(src)] if use_mask else v.reshape(-1)


def stats(src, use_mask, clip=None):
    """[C][2] mean and population standard deviation with exactly rounded sums (math.fsum): each is within one rounding of the true value of
    sum / n and of sqrt(sum((x - mean)^2) / n) for the float64 mean."""
    out = np.zeros((len(src), 2))
    for c in range(len(src)):
        x = masked_values(src, c, use_mask).astype(np.float64)
        if clip is not None:
            x = np.minimum(np.maximum(x, clip[c][0]), clip[c][1])
        n = np.float64(x.size)
        mean = np.float64(math.fsum(x)) / n
        d = x - mean
        out[c] = mean, np.sqrt(np.float64(math.fsum(d * d)) / n)
    return out


def order_statistics(values, ranks):
    """The values at the 0-based ranks of the ascending order, zeros as +0.0, float32."""
    s = np.sort(np.asarray(values, dtype=np.float32) + np.float32(0.0), kind="stable")
    return np.array([s[r] for r in ranks], dtype=np.float32)


def percentile(values, q):
    """numpy's 'linear' percentile of float32 values in float64, zeros as +0.0: np.percentile(values.astype(float64) + 0.0, q) restated."""
    s = np.sort(np.asarray(values, dtype=np.float32).astype(np.float64) + 0.0)
    n = s.size
    vi = (n - 1) * (np.float64(q) / 100)
    if vi >= n - 1:
        a = b = s[-1]
        t = np.float64(0.0)
    else:
        lo = int(math.floor(vi))
        a, b, t = s[lo], s[lo + 1], np.float64(vi - lo)
    d = b - a
    return b - d * (1.0 - t) if t >= 0.5 else a + d * t


def resample(src, src_lab, box, out_shape, stats_, clip, region, use_mask):
    """box = (x0, y0, z0, NX, NY, NZ).  -> (img float64 [C, OX, OY, OZ], lab uint8 [OX, OY, OZ])."""
    src = np.asarray(src)
    C = src.shape[0]
    x0, y0, z0, NX, NY, NZ = box
    sub = src[:, z0:z0 + NZ, y0:y0 + NY, x0:x0 + NX].astype(np.float64).transpose(0, 3, 2, 1)      # [C, x, y, z]
    m = mask_of(src)[z0:z0 + NZ, y0:y0 + NY, x0:x0 + NX].transpose(2, 1, 0)
    ax = [axis(n, o) for n, o in zip((NX, NY, NZ), out_shape)]
    img = np.zeros((C,) + tuple(out_shape), dtype=np.float64)
    for c in range(C):
        mean, std = (stats_[c][0], stats_[c][1]) if stats_ is not None else (0.0, 1.0)
        lo, hi = (clip[c][0], clip[c][1]) if clip is not None else (-np.inf, np.inf)
        u = (np.minimum(np.maximum(sub[c], lo), hi) - np.float64(mean)) / max(np.float64(std), np.float64(1e-8))
        if use_mask:
            u = np.where(m, u, 0.0)
        acc = np.zeros(out_shape, dtype=np.float64)
        for bx in (0, 1):
            for by in (0, 1):
                for bz in (0, 1):
                    ix, wx = ax[0][bx], ax[0][2 + bx]
                    iy, wy = ax[1][by], ax[1][2 + by]
                    iz, wz = ax[2][bz], ax[2][2 + bz]
                    acc = acc + ((u[np.ix_(ix, iy, iz)] * wx[:, None, None]) * wy[None, :, None]) * wz[None, None, :]
        img[c] = acc
    if src_lab is None:
        lab = np.zeros(out_shape, dtype=np.uint8)
    else:
        sl = np.asarray(src_lab)[z0:z0 + NZ, y0:y0 + NY, x0:x0 + NX].transpose(2, 1, 0)
        lab = np.asarray(region, dtype=np.uint8)[sl[np.ix_(ax[0][4], ax[1][4], ax[2][4])]]
    return img, lab


def restore(pred, box, orig_shape, paint=None):
    """pred uint8 [PX, PY, PZ] -> (out, painted or None) uint8 [X, Y, Z]."""
    x0, y0, z0, NX, NY, NZ = box
    nn = [axis(p, n)[4] for n, p in zip((NX, NY, NZ), pred.shape)]
    out = np.zeros(orig_shape, dtype=np.uint8)
    out[x0:x0 + NX, y0:y0 + NY, z0:z0 + NZ] = pred[np.ix_(*nn)]
    return out, (np.asarray(paint, dtype=np.uint8)[out] if paint is not None else None)
