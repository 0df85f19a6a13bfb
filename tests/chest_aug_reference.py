"""numpy restatement of the 2D (chest) augmentation chain at Pillow's arithmetic, given explicit parameters -- the oracle beside
csrc/augment2d.hip (as tests/aug_reference.py is for the LUNA kernels).  Images are uint8 [H, W, C] arrays (C = 1 for a mode-L image, 3 for RGB).

Every operation restates the Pillow C code torchvision's PIL path hands it to: Resample.c (two-pass fixed-point BILINEAR, horizontal first),
Geometry.c (NEAREST affine in 16.16 fixed point), BoxBlur.c (GaussianBlur = 3-pass extended box blur), Blend.c (ImageEnhance's blend: float
arithmetic, truncation), Convert.c (rgb2l, rgb2hsv, hsv2rgb with their float / double intermediates).  tests/test_chest_data_cpu.py checks
each one against Pillow itself."""
from __future__ import annotations

import math

import numpy as np

PRECISION_BITS = 22
MEAN = np.array([0.485, 0.456, 0.406], np.float32)
STD = np.array([0.229, 0.224, 0.225], np.float32)
f32, f64 = np.float32, np.float64


# ---- Resample.c ----
def resample_coeffs(in_size: int, out_size: int):
    """precompute_coeffs + normalize_coeffs_8bpc (BILINEAR, box [0, in_size)) -> (xmin [out], taps list of int arrays)."""
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ss = 1.0 / filterscale
    xmins, taps = [], []
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        w = []
        for x in range(xmax - xmin):
            d = abs(((x + xmin) - center + 0.5) * ss)
            w.append(1.0 - d if d < 1.0 else 0.0)
        ww = 0.0
        for v in w:
            ww += v
        k = [v / ww if ww != 0.0 else v for v in w]
        taps.append(np.array([int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS)) for v in k], np.int64))
        xmins.append(xmin)
    return xmins, taps


def _pass(img, out_size, axis):
    """One resampling pass along `axis` (1 = horizontal, 0 = vertical), uint8 -> uint8."""
    a = np.moveaxis(img.astype(np.int64), axis, 0)
    xmins, taps = resample_coeffs(a.shape[0], out_size)
    out = np.empty((out_size,) + a.shape[1:], np.int64)
    for xx in range(out_size):
        k = taps[xx]
        seg = a[xmins[xx]:xmins[xx] + len(k)]
        out[xx] = (1 << (PRECISION_BITS - 1)) + np.tensordot(k, seg, axes=(0, 0))
    out = np.clip(out >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize(img, S):
    """Image.resize((S, S), BILINEAR): horizontal pass, then vertical, each rounded to uint8 (a pass whose size does not change is an identity)."""
    return _pass(_pass(img, S, 1), S, 0)


def crop_resize(img, i, j, h, w, S):
    return resize(img[i:i + h, j:j + w], S)


# ---- Geometry.c ----
def rotate_nearest(img, a):
    """Image.rotate(angle, NEAREST) given the 16.16 fixed-point matrix a = (a0..a5) (pcrlv2_amd.data_chest.rotate_fixed); outside = 0."""
    H, W = img.shape[:2]
    a0, a1, a2, a3, a4, a5 = (int(v) for v in a)
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    xin = (a2 + y * a1 + x * a0) >> 16
    yin = (a5 + y * a4 + x * a3) >> 16
    ok = (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)
    out = np.zeros_like(img)
    out[ok] = img[yin[ok], xin[ok]]
    return out


def hflip(img):
    return img[:, ::-1].copy()


# ---- Convert.c ----
def luma(img):
    """convert('L') of an [H, W, 3] image -> [H, W] int64."""
    r, g, b = (img[..., c].astype(np.int64) for c in range(3))
    return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16


def grayscale(img):
    """RandomGrayscale's to_grayscale(num_output_channels=3); a 1-plane image is unchanged."""
    if img.shape[2] == 1:
        return img.copy()
    l = luma(img).astype(np.uint8)
    return np.repeat(l[..., None], 3, axis=2)


# ---- BoxBlur.c ----
def _box_pass(a, r, ww, fw, axis):
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    n = a.shape[0]
    idx = lambda k: a[np.clip(np.arange(n) + k, 0, n - 1)]
    acc = sum(idx(k) for k in range(-r, r + 1))
    bulk = acc * ww + (idx(-r - 1) + idx(r + 1)) * fw
    out = ((bulk + (1 << 23)) >> 24).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def box_blur(img, r, ww, fw, passes=3):
    """ImageFilter.GaussianBlur given BoxBlur.c's (integer radius, ww, fw) (pcrlv2_amd.data_chest.blur_params): 3 horizontal passes, then 3 vertical."""
    a = img
    for _ in range(passes):
        a = _box_pass(a, r, ww, fw, 1)
    for _ in range(passes):
        a = _box_pass(a, r, ww, fw, 0)
    return a


# ---- Blend.c / ImageEnhance ----
def blend(a, b, alpha):
    """Image.blend(a, b, alpha) with alpha rounded to float32 and float32 arithmetic, truncated (clipped when extrapolating)."""
    al = f32(alpha)
    if al == 0:
        return np.broadcast_to(a, np.broadcast(a, b).shape).astype(np.uint8)
    if al == 1:
        return np.broadcast_to(b, np.broadcast(a, b).shape).astype(np.uint8)
    a32 = np.asarray(a, np.int64)
    t = a32.astype(f32) + al * (np.asarray(b, np.int64) - a32).astype(f32)
    return np.clip(np.trunc(t), 0, 255).astype(np.uint8)


def brightness(img, f):
    return blend(np.zeros_like(img), img, f)


def contrast(img, f):
    l = luma(img) if img.shape[2] == 3 else img[..., 0].astype(np.int64)
    n = l.size
    mean = (2 * int(l.sum()) + n) // (2 * n)
    return blend(np.full_like(img, mean), img, f)


def saturation(img, f):
    if img.shape[2] == 1:
        return img.copy()
    return blend(luma(img)[..., None], img, f)


def _rgb2hsv(img):
    r, g, b = (img[..., c].astype(np.int64) for c in range(3))
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    same = maxc == minc
    cr = (maxc - minc).astype(f32)
    crs = np.where(same, f32(1), cr)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = cr / np.where(same, f32(1), maxc.astype(f32))
        rc, gc, bc = ((maxc - c).astype(f32) / crs for c in (r, g, b))
    h = np.where(r == maxc, bc - gc, np.where(g == maxc, (2.0 + rc.astype(f64) - bc.astype(f64)).astype(f32),
                                              (4.0 + gc.astype(f64) - rc.astype(f64)).astype(f32)))
    hd = h.astype(f64) / 6.0 + 1.0
    h = np.fmod(hd, 1.0).astype(f32)
    uh = np.clip((h.astype(f64) * 255.0).astype(np.int64), 0, 255)
    us = np.clip((s.astype(f64) * 255.0).astype(np.int64), 0, 255)
    return np.where(same, 0, uh), np.where(same, 0, us), maxc


def _hsv2rgb(h, s, v):
    h6 = h.astype(f32).astype(f64) * 6.0 / 255.0
    i = np.floor(h6).astype(np.int64)
    f = (h6 - i.astype(f32).astype(f64)).astype(f32)
    fs = (s.astype(f32).astype(f64) / 255.0).astype(f32)
    vf = v.astype(f32).astype(f64)
    rnd = lambda x: np.where(x >= 0, np.floor(x + 0.5), np.ceil(x - 0.5)).astype(np.int64)      # C round(): half away from zero
    p = np.clip(rnd(vf * (1.0 - fs.astype(f64))), 0, 255)
    q = np.clip(rnd(vf * (1.0 - (fs * f).astype(f64))), 0, 255)
    t = np.clip(rnd(vf * (1.0 - fs.astype(f64) * (1.0 - f.astype(f64)))), 0, 255)
    sel = i % 6
    r = np.choose(sel, [v, q, p, p, t, v])
    g = np.choose(sel, [t, v, v, q, p, p])
    b = np.choose(sel, [p, p, t, v, v, q])
    gray = s == 0
    return np.stack([np.where(gray, v, r), np.where(gray, v, g), np.where(gray, v, b)], axis=-1).astype(np.uint8)


def hue(img, shift):
    """adjust_hue with the PIL-H shift `shift` (pcrlv2_amd.data_chest.hue_shift): RGB -> HSV, H + shift mod 256, -> RGB.  Identity on one plane."""
    if img.shape[2] == 1:
        return img.copy()
    h, s, v = _rgb2hsv(img)
    return _hsv2rgb((h + shift) % 256, s, v)


JITTER_OPS = ("brightness", "contrast", "saturation", "hue")


def jitter(img, order, factors, shift):
    """ColorJitter in the drawn order: order = op ids (0 brightness, 1 contrast, 2 saturation, 3 hue), factors = (b, c, s)."""
    for op in order:
        if op == 0:
            img = brightness(img, factors[0])
        elif op == 1:
            img = contrast(img, factors[1])
        elif op == 2:
            img = saturation(img, factors[2])
        else:
            img = hue(img, shift)
    return img


# ---- ToTensor / Normalize / Cutout (torch CPU's float32 order) ----
def normalize(img):
    """uint8 [H, W, C] -> float32 [3, H, W] (u / 255 - mean) / std; a 1-plane image is replicated."""
    if img.shape[2] == 1:
        img = np.repeat(img, 3, axis=2)
    u = np.moveaxis(img, 2, 0).astype(f32)
    return ((u / f32(255)) - MEAN[:, None, None]) / STD[:, None, None]


def cutout(t, holes):
    """Cutout: t * mask, the mask zero on the clipped squares holes = [(y0, y1, x0, x1), ...]."""
    m = np.ones(t.shape[1:], f32)
    for y0, y1, x0, x1 in holes:
        m[y0:y1, x0:x1] = 0
    return t * m


# ---- whole views from one parameter record (pcrlv2_amd.data_chest layout) ----
def view(img, rec, S):
    """(augmented float32 [3,S,S], target float32 [3,S,S], spatial uint8, photometric uint8) for one record."""
    from pcrlv2_amd import data_chest as DC
    j, i, w, h = (int(rec[k]) for k in (DC.P_J, DC.P_I, DC.P_CW, DC.P_CH))
    sp = rotate_nearest(crop_resize(img, i, j, h, w, S), rec[DC.P_A0:DC.P_A5 + 1])
    if rec[DC.P_FLIP]:
        sp = hflip(sp)
    target = normalize(sp)
    a = sp
    if rec[DC.P_GRAY]:
        a = grayscale(a)
    if rec[DC.P_BLUR]:
        a = box_blur(a, int(rec[DC.P_BR]), int(rec[DC.P_WW]), int(rec[DC.P_FW]))
    order = [(int(rec[DC.P_ORDER]) >> (4 * k)) & 15 for k in range(int(rec[DC.P_NOPS]))]
    factors = np.array(rec[DC.P_BRI:DC.P_SAT + 1], np.int32).view(np.float32)
    a = jitter(a, order, [float(x) for x in factors], int(rec[DC.P_HUE]))
    out = normalize(a)
    holes = [tuple(int(v) for v in rec[DC.P_HOLES + 4 * k:DC.P_HOLES + 4 * k + 4]) for k in range(int(rec[DC.P_NHOLES]))]
    if holes:
        out = cutout(out, holes)
    return out, target, sp, a
