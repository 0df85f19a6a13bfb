"""Float64 NumPy restatement of the LUNA16 pre-processing (the reference's `luna_preprocess.py`) that `csrc/luna_prep.hip` and
`pcrlv2_amd/luna_prep.py` implement: the ITK linear resample to 1 mm, the HU window, `skimage.transform.resize(..., preserve_range=True)`
of the crops, the depth-map score and the draw rules.

skimage is not installed here.  Its `resize` (read from skimage's source) runs, for a float64 image with the default order 1 and
mode 'reflect': `scipy.ndimage.gaussian_filter(image, max(0, (in/out - 1) / 2), mode='mirror')` when any axis shrinks, then
`scipy.ndimage.zoom(filtered, out/in, order=1, mode='mirror', grid_mode=True)`, then a clip to the unfiltered image's min / max.  The
functions below restate scipy's C code for those two calls operation by operation (the symmetric `correlate1d` sums the farthest tap pair
first; `zoom` sums the 8 corners with the last axis fastest, each corner as ((v * w0) * w1) * w2 from 0.0, with weights 1 - t and
1 - (1 - t)); `tests/test_luna_prep_cpu.py` checks them against scipy bit for bit.
"""
from __future__ import annotations

import numpy as np

HU_MIN, HU_MAX = -1000.0, 1000.0
HU_THRED = (-150.0 - HU_MIN) / (HU_MAX - HU_MIN)
LUNG_MAX = 0.15
LEN_BORDER, LEN_BORDER_Z, LEN_DEPTH = 70, 15, 3
COL_SIZE = [(96, 96, 64), (96, 96, 96), (112, 112, 64), (64, 64, 32)]
LOCAL_COL_SIZE = [(32, 32, 16), (16, 16, 16), (32, 32, 32), (8, 8, 8)]
INPUT = (64, 64, 32)
LOCAL_INPUT = (16, 16, 16)


# ---- step 1: ITK ResampleImageFilter, identity transform, linear, output spacing 1 ----------------------------------------------
def resample_size(size, spacing):
    """outsize[a] = int(size[a] * spacing[a] / 1 + 0.5) (luna_preprocess.py:335-337); size / spacing in (x, y, z)."""
    return tuple(int(n * s / 1 + 0.5) for n, s in zip(size, spacing))


def _axis_lerp(n_in, n_out, spacing):
    o = np.arange(n_out, dtype=np.float64)
    ci = (o * 1.0) / spacing
    inside = ci < n_in - 0.5
    f = np.minimum(np.floor(ci).astype(np.int64), n_in - 1)
    t = ci - f
    f1 = np.minimum(f + 1, n_in - 1)
    return inside, f, f1, t


def resample(vol_zyx, spacing_xyz, out_xyz=None, oz_range=None):
    """int16 (z, y, x) -> int16 (z', y', x') at 1 mm: ITK's linear interpolation (x, then y, then z, each a + (b - a) * t), 0 outside,
    cast by clamping to the int16 range and truncating toward zero.  oz_range = (a, b): only output slices a .. b-1."""
    Z, Y, X = vol_zyx.shape
    if out_xyz is None:
        out_xyz = resample_size((X, Y, Z), spacing_xyz)
    ox, oy, oz = out_xyz
    ix, fx, fx1, tx = _axis_lerp(X, ox, spacing_xyz[0])
    iy, fy, fy1, ty = _axis_lerp(Y, oy, spacing_xyz[1])
    iz, fz, fz1, tz = _axis_lerp(Z, oz, spacing_xyz[2])
    if oz_range is not None:
        iz, fz, fz1, tz = (q[oz_range[0]:oz_range[1]] for q in (iz, fz, fz1, tz))
    v = vol_zyx.astype(np.float64)

    def g(zz, yy, xx):
        return v[np.ix_(zz, yy, xx)]
    TX, TY, TZ = tx[None, None, :], ty[None, :, None], tz[:, None, None]
    x00 = g(fz, fy, fx) + (g(fz, fy, fx1) - g(fz, fy, fx)) * TX
    x10 = g(fz, fy1, fx) + (g(fz, fy1, fx1) - g(fz, fy1, fx)) * TX
    xy0 = x00 + (x10 - x00) * TY
    x01 = g(fz1, fy, fx) + (g(fz1, fy, fx1) - g(fz1, fy, fx)) * TX
    x11 = g(fz1, fy1, fx) + (g(fz1, fy1, fx1) - g(fz1, fy1, fx)) * TX
    xy1 = x01 + (x11 - x01) * TY
    r = xy0 + (xy1 - xy0) * TZ
    r = np.trunc(np.clip(r, -32768.0, 32767.0))
    r[~(iz[:, None, None] & iy[None, :, None] & ix[None, None, :])] = 0.0
    return r.astype(np.int16)


# ---- step 2: HU window ----------------------------------------------------------------------------------------------------------
def normalise(v):
    v = np.clip(np.asarray(v, dtype=np.float64), HU_MIN, HU_MAX)
    return 1.0 * (v - HU_MIN) / (HU_MAX - HU_MIN)


# ---- skimage.transform.resize(order=1, mode='reflect', preserve_range=True) ------------------------------------------------------
def gaussian_weights(sigma):
    """scipy's _gaussian_kernel1d(sigma, 0, int(4 * sigma + 0.5)) -> (radius, c[0..radius]), c[j] the weight of the taps at +-j."""
    radius = int(4.0 * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return radius, phi[radius:].copy()


def mirror_index(i, n):
    """scipy.ndimage mode 'mirror' (reflect about the edge voxels, edge not repeated)."""
    i = np.asarray(i)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * n - 2
    i = np.abs(i) % p
    return np.where(i >= n, p - i, i)


def correlate_mirror(a, axis, c):
    """scipy's symmetric correlate1d: c0 * x0, then + (x[-j] + x[+j]) * cj for j = radius .. 1."""
    a = np.moveaxis(a, axis, -1)
    n = a.shape[-1]
    idx = np.arange(n)
    out = a * c[0]
    for j in range(len(c) - 1, 0, -1):
        out = out + (a[..., mirror_index(idx - j, n)] + a[..., mirror_index(idx + j, n)]) * c[j]
    return np.moveaxis(out, -1, axis)


def zoom_axis(n_in, n_out):
    """grid_mode coordinates (o + 0.5) * (in / out) - 0.5, mirrored -> (i0, i1, w0, w1)."""
    ratio = n_in / n_out
    cc = ((np.arange(n_out, dtype=np.float64) + 0.5) * ratio) - 0.5
    if n_in == 1:
        z = np.zeros(n_out, dtype=np.int64)
        return z, z, np.ones(n_out), np.zeros(n_out)
    cc = np.where(cc < 0, -cc, cc)
    f = np.floor(cc)
    t = cc - f
    i0 = f.astype(np.int64)
    i1 = i0 + 1
    i1 = np.where(i1 >= n_in, 2 * n_in - 2 - i1, i1)
    w0 = 1.0 - t
    return i0, i1, w0, 1.0 - w0


def zoom(a, shape):
    ax = [zoom_axis(a.shape[k], shape[k]) for k in range(3)]
    out = np.zeros(shape)
    for b0 in (0, 1):
        for b1 in (0, 1):
            for b2 in (0, 1):
                i0, w0 = ax[0][b0], ax[0][2 + b0]
                i1, w1 = ax[1][b1], ax[1][2 + b1]
                i2, w2 = ax[2][b2], ax[2][2 + b2]
                out = out + ((a[np.ix_(i0, i1, i2)] * w0[:, None, None]) * w1[None, :, None]) * w2[None, None, :]
    return out


def resize_sigmas(in_shape, out_shape):
    """-> per-axis sigma, or None when skimage's anti-aliasing is off (no axis shrinks)."""
    if not any(o < i for i, o in zip(in_shape, out_shape)):
        return None
    return [max(0.0, (i / o - 1) / 2) for i, o in zip(in_shape, out_shape)]


def resize(img, shape):
    img = np.asarray(img, dtype=np.float64)
    lo, hi = img.min(), img.max()
    f = img
    sig = resize_sigmas(img.shape, shape)
    if sig is not None:
        for axis, s in enumerate(sig):
            if s > 1e-15:
                f = correlate_mirror(f, axis, gaussian_weights(s)[1])
    return np.clip(zoom(f, shape), lo, hi)


# ---- depth map (luna_preprocess.py:213-249) -------------------------------------------------------------------------------------
def depth_score(w):
    """Exact 2 * sum(d_img) over d < 32 of a (64, 64, 35) window: d_img = 1 - k / 2, k the first of 0..2 with w[i, j, d + k] >= HU_thred
    (2 if none) -> 2 * n0 + n1."""
    ge = w >= HU_THRED
    n0 = n1 = 0
    for d in range(INPUT[2]):
        k0 = ge[:, :, d]
        k1 = ~k0 & ge[:, :, d + 1]
        n0 += int(k0.sum())
        n1 += int(k1.sum())
    return 2 * n0 + n1


def rejected(score1, score2, rows1, cols1, deps1):
    lim = LUNG_MAX * cols1 * deps1 * rows1
    return score1 / 2 > lim or score2 / 2 > lim


# ---- draw rules (luna_preprocess.py:151-275), scalar form of pcrlv2_amd.luna_prep.draw_attempt ----------------------------------
def cal_iou(b1, b2):
    s1 = (b1[1] - b1[0]) * (b1[3] - b1[2]) * (b1[5] - b1[4])
    s2 = (b2[1] - b2[0]) * (b2[3] - b2[2]) * (b2[5] - b2[4])
    w = max(0, min(b1[1], b2[1]) - max(b1[0], b2[0]))
    h = max(0, min(b1[3], b2[3]) - max(b1[2], b2[2]))
    d = max(0, min(b1[5], b2[5]) - max(b1[4], b2[4]))
    a = w * h * d
    return a / (s1 + s2 - a)


def padded_depth(size_z):
    if size_z - 64 - LEN_DEPTH - 1 - LEN_BORDER_Z < LEN_BORDER_Z:
        pad = size_z - 64 - LEN_DEPTH - 1 - LEN_BORDER_Z - LEN_BORDER_Z
        return size_z + (-pad + 1)
    return size_z


def draw_attempt(rng, shape, block, max_blocks):
    """-> ("ok", box1, box2, sizes1, sizes2, locals) | ("empty", axis) | ("none",).  Same generator calls as the product."""
    sx, sy, sz = shape
    rows = np.array([c[0] for c in COL_SIZE])
    cols = np.array([c[1] for c in COL_SIZE])
    deps = np.array([c[2] for c in COL_SIZE])
    for _ in range(max_blocks):
        i1 = rng.integers(0, len(COL_SIZE), block)
        i2 = rng.integers(0, len(COL_SIZE), block)
        cand = []
        for ii in (i1, i2):
            r, c, d = rows[ii].copy(), cols[ii].copy(), deps[ii].copy()
            shrink = sx - r - 1 - LEN_BORDER <= LEN_BORDER
            r[shrink] -= 32
            c[shrink] -= 32
            cand.append((r, c, d))
        lohi = []
        for r, c, d in cand:
            lohi.append((LEN_BORDER, sx - r - 1 - LEN_BORDER))
            lohi.append((LEN_BORDER, sy - c - 1 - LEN_BORDER))
            lohi.append((LEN_BORDER_Z, sz - d - LEN_DEPTH - 1 - LEN_BORDER_Z))
        starts = [rng.integers(lo, np.maximum(hi, lo) + 1) for lo, hi in lohi]
        for n in range(block):
            for a, (lo, hi) in enumerate(lohi):
                if hi[n] < lo:
                    return ("empty", "xyz"[a % 3])
            (r1, c1, d1), (r2, c2, d2) = [(int(r[n]), int(c[n]), int(d[n])) for r, c, d in cand]
            b1 = (int(starts[0][n]), int(starts[0][n]) + r1, int(starts[1][n]), int(starts[1][n]) + c1, int(starts[2][n]), int(starts[2][n]) + d1)
            b2 = (int(starts[3][n]), int(starts[3][n]) + r2, int(starts[4][n]), int(starts[4][n]) + c2, int(starts[5][n]), int(starts[5][n]) + d2)
            if cal_iou(b1, b2) > 0.3:
                mn = (min(b1[0], b2[0]), min(b1[2], b2[2]), min(b1[4], b2[4]))
                mx = (max(b1[1], b2[1]), max(b1[3], b2[3]), max(b1[5], b2[5]))
                lo = [max(m - 3, 0) for m in mn]
                hi = [min(m + 3, s) for m, s in zip(mx, shape)]
                lx = rng.integers(lo[0], hi[0], 6)
                ly = rng.integers(lo[1], hi[1], 6)
                lz = rng.integers(lo[2], hi[2], 6)
                li = rng.integers(0, len(LOCAL_COL_SIZE), 6)
                locs = []
                for q in range(6):
                    st = (int(lx[q]), int(ly[q]), int(lz[q]))
                    ls = LOCAL_COL_SIZE[int(li[q])]
                    locs.append((st, tuple(min(s0 + n0, s) - s0 for s0, n0, s in zip(st, ls, shape))))
                return ("ok", b1, b2, (r1, c1, d1), (r2, c2, d2), locs)
    return ("none",)


# ---- one crop pair from a normalised, padded (x, y, z) volume -------------------------------------------------------------------
def pair_windows(vol, b1, b2, s1, s2, locs):
    """-> (global [2, 64, 64, 32], local [6, 16, 16, 16], score1, score2) as luna_preprocess.py:193-275 computes them."""
    out, scores = [], []
    for b, s in ((b1, s1), (b2, s2)):
        w = vol[b[0]:b[0] + s[0], b[2]:b[2] + s[1], b[4]:b[4] + s[2] + LEN_DEPTH]
        if s != INPUT:
            w = resize(w, (INPUT[0], INPUT[1], INPUT[2] + LEN_DEPTH))
        scores.append(depth_score(w))
        out.append(w[:, :, :INPUT[2]])
    loc = []
    for st, n in locs:
        w = vol[st[0]:st[0] + n[0], st[1]:st[1] + n[1], st[2]:st[2] + n[2]]
        loc.append(resize(w, LOCAL_INPUT))
    return np.stack(out), np.stack(loc), scores[0], scores[1]


# ---- the whole series ------------------------------------------------------------------------------------------------------------
def attempt_rng(seed, name, k, j):
    """Generator of attempt j of pair k: keyed on (seed, the first 8 bytes of BLAKE2b(name) as a little-endian integer, k, j)."""
    import hashlib
    h = int.from_bytes(hashlib.blake2b(name.encode(), digest_size=8).digest(), "little")
    return np.random.default_rng([seed, h, k, j])


def series(vol_zyx, spacing, name, seed, scale, max_attempts=1024, block=256, max_blocks=64):
    """-> [(global, local)] * scale, or the string "skip" (an empty start range drawn, or max_attempts rejected attempts)."""
    v = normalise(resample(vol_zyx, spacing).transpose(2, 1, 0))
    sz = padded_depth(v.shape[2])
    if sz != v.shape[2]:
        v = np.concatenate([v, np.zeros(v.shape[:2] + (sz - v.shape[2],))], axis=2)
    out = []
    for k in range(scale):
        for j in range(max_attempts):
            d = draw_attempt(attempt_rng(seed, name, k, j), v.shape, block, max_blocks)
            if d[0] == "empty":
                return "skip"
            if d[0] == "none":
                continue
            _, b1, b2, s1, s2, locs = d
            g, loc, sc1, sc2 = pair_windows(v, b1, b2, s1, s2, locs)
            if not rejected(sc1, sc2, *s1):
                out.append((g, loc))
                break
        else:
            return "skip"
    return out
