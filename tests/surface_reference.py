"""Restatements of the surface-distance metrics (csrc/surface_dist.hip, train_seg.surface_metrics) with numpy.  Not a test file.

surfaces      the bitwise formula on the whole byte: m & ~(m[x-1] & m[x+1] & m[y-1] & m[y+1] & m[z-1] & m[z+1]), 0 outside the volume.
edt_sq        three line passes Z, Y, X, each min_j (fl(fl(s (i - j))^2) + f[j]): every numpy float64 operation below is ONE IEEE operation.
stats         the union order statistics by np.sort, the sums by math.fsum.
metrics       np.percentile (default linear method), max, MedPy's assd, and the empty-mask conventions.
"""
import math

import numpy as np

REC = 8


def effective(pred, gt, K):
    """The masks that count: a voxel whose ground-truth byte has bit 7 set belongs to neither; bits >= K are dropped."""
    keep = np.where(gt & 0x80, 0, (1 << K) - 1).astype(np.uint8)
    return pred & keep, gt & keep


def _shift(m, axis, step):
    out = np.zeros_like(m)
    src = [slice(None)] * 3
    dst = [slice(None)] * 3
    if step > 0:
        src[axis], dst[axis] = slice(0, -1), slice(1, None)
    else:
        src[axis], dst[axis] = slice(1, None), slice(0, -1)
    out[tuple(dst)] = m[tuple(src)]
    return out


def surface(m):
    """All classes of one effective bitmask at once."""
    inner = np.full_like(m, 0x7F)
    for axis in range(3):
        inner &= _shift(m, axis, 1) & _shift(m, axis, -1)
    return m & ~inner


def surfaces(pred, gt, K):
    """-> (surf_pred, surf_gt uint8 [X, Y, Z], counts int64 [K, 3] = {TP, |pred|, |gt|})"""
    P, G = effective(pred, gt, K)
    counts = np.array([[int(((P & G) >> k & 1).sum()), int((P >> k & 1).sum()), int((G >> k & 1).sum())] for k in range(K)], dtype=np.int64).reshape(K, 3)
    return surface(P), surface(G), counts


def line_pass(f, s, axis):
    """out[i] = min_j (fl(fl(s (i - j))^2) + f[j]) along `axis`; f float64 >= 0 (or +inf)."""
    g = np.moveaxis(f, axis, 0)
    L = g.shape[0]
    t = np.float64(s) * np.arange(L, dtype=np.float64)      # fl(s d); (s (-d))^2 = (s d)^2 exactly
    cost = t * t                                           # fl(fl(s d)^2)
    idx = np.arange(L)
    out = np.full(g.shape, np.inf)
    tail = (1,) * (g.ndim - 1)
    for j in range(L):
        np.minimum(out, cost[np.abs(idx - j)].reshape((L,) + tail) + g[j][None], out=out)
    return np.moveaxis(out, 0, axis)


def edt_sq(surf_bit, spacing):
    """surf_bit: bool [X, Y, Z].  The separable squared distance, Z then Y then X."""
    f = np.where(surf_bit, 0.0, np.inf)
    f = line_pass(f, spacing[2], 2)
    f = line_pass(f, spacing[1], 1)
    return line_pass(f, spacing[0], 0)


def brute_d2(surf_bit, spacing):
    """min over the surface voxels of fl(fl(fl(sx dx))^2 + fl(fl(fl(sy dy))^2 + fl(fl(sz dz))^2)), one voxel of the surface at a time."""
    X, Y, Z = surf_bit.shape
    out = np.full((X, Y, Z), np.inf)
    sx, sy, sz = (np.float64(s) for s in spacing)
    for x, y, z in zip(*np.nonzero(surf_bit)):
        tx = sx * (np.arange(X, dtype=np.float64) - x)
        ty = sy * (np.arange(Y, dtype=np.float64) - y)
        tz = sz * (np.arange(Z, dtype=np.float64) - z)
        d = (tx * tx)[:, None, None] + ((ty * ty)[None, :, None] + (tz * tz)[None, None, :])
        np.minimum(out, d, out=out)
    return out


def stats(d2_to_gt, sp_bit, d2_to_pred, sg_bit, q=0.95):
    """-> {'n_a', 'n_b', 'lo', 'd2': the sorted union's entries at lo, hi, n - 1 (None when a surface is empty), 'sum_a', 'sum_b' (math.fsum), 'A', 'B'}"""
    a2, b2 = d2_to_gt[sp_bit], d2_to_pred[sg_bit]
    na, nb = int(a2.size), int(b2.size)
    out = {"n_a": na, "n_b": nb, "lo": None, "d2": None, "sum_a": None, "sum_b": None, "A": np.sqrt(a2), "B": np.sqrt(b2)}
    if na and nb:
        n = na + nb
        u = np.sort(np.concatenate([a2, b2]))
        lo = int(math.floor(q * float(n - 1)))
        hi = min(lo + 1, n - 1)
        out.update(lo=lo, d2=(u[lo], u[hi], u[n - 1]), sum_a=math.fsum(out["A"].tolist()), sum_b=math.fsum(out["B"].tolist()))
    return out


def record_of(st):
    """The device record of `stats` (int64 [8]; slots 3..7 float64 bit patterns), the sums rounded from math.fsum."""
    rec = np.zeros(REC, dtype=np.int64)
    rec[0], rec[1] = st["n_a"], st["n_b"]
    if st["d2"] is not None:
        rec[2] = st["lo"]
        rec[3:8] = np.array(list(st["d2"]) + [st["sum_a"], st["sum_b"]], dtype=np.float64).view(np.int64)
    return rec


def class_stats(pred, gt, K, spacing, q=0.95):
    """-> (per-class `stats`, counts): the whole chain of the restatement."""
    sp, sg, counts = surfaces(pred, gt, K)
    per = []
    for k in range(K):
        spk, sgk = (sp >> k & 1).astype(bool), (sg >> k & 1).astype(bool)
        per.append(stats(edt_sq(sgk, spacing), spk, edt_sq(spk, spacing), sgk, q))
    return per, counts


def metrics_of(per, q=0.95):
    """hd95 = np.percentile(U, 100 q), hd = max U, assd = (mean A + mean B) / 2; both surfaces empty: 0.0; one empty: NaN."""
    K = len(per)
    out = {k: np.zeros(K) for k in ("hd95", "hd", "assd")}
    for k, st in enumerate(per):
        if st["n_a"] == 0 and st["n_b"] == 0:
            continue
        if st["n_a"] == 0 or st["n_b"] == 0:
            for key in out:
                out[key][k] = np.nan
            continue
        u = np.concatenate([st["A"], st["B"]])
        out["hd95"][k] = np.percentile(u, 100.0 * q)
        out["hd"][k] = u.max()
        out["assd"][k] = (st["sum_a"] / st["n_a"] + st["sum_b"] / st["n_b"]) / 2.0
    return out


def metrics(pred, gt, K, spacing=(1.0, 1.0, 1.0), q=0.95):
    per, counts = class_stats(pred, gt, K, spacing, q)
    out = metrics_of(per, q)
    out["n_pred"] = np.array([st["n_a"] for st in per], dtype=np.int64)
    out["n_gt"] = np.array([st["n_b"] for st in per], dtype=np.int64)
    out["counts"] = counts
    return out


# ---- masks ---------------------------------------------------------------------------------------------------------------------------
def blobs(shape, K, seed, level=0.55):
    """Smoothed-noise blobs: K overlapping classes, uint8 bitmask."""
    rng = np.random.default_rng(seed)
    out = np.zeros(shape, dtype=np.uint8)
    for k in range(K):
        v = rng.random(shape)
        for axis in range(3):
            if shape[axis] > 2:
                v = (v + np.roll(v, 1, axis) + np.roll(v, -1, axis)) / 3.0
        out |= ((v > np.quantile(v, level)).astype(np.uint8) << k).astype(np.uint8)
    return out


def sprinkle_not_counted(gt, seed, frac=0.05):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(gt.shape) < frac, gt | 0x80, gt).astype(np.uint8)
