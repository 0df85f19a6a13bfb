"""Writes tests/golden/luna_prep_windows.npz: a CT-like int16 phantom (HU -1200 .. 1600, so the HU clip matters) and, for every window size
class the LUNA pre-processing meets, SCIPY's output of what skimage.transform.resize(order=1, mode='reflect', preserve_range=True) runs
(gaussian_filter(mode='mirror') when an axis shrinks, zoom(order=1, mode='mirror', grid_mode=True), clip to the crop's min / max) on the
normalised crop, plus the exact depth score of the global windows.  The float64 outputs are kept as SHA-256 digests of their bytes (bit-exact
checks without megabytes of fixture) and a strided subsample (to name a difference).  Size classes: the four global sizes (+3 depths) with and
without the 32-row reduction -> (64, 64, 35), the four local sizes and edge-truncated local windows down to 1 voxel per axis -> 16^3.

    python tools/make_luna_prep_fixtures.py [OUT_DIR]
"""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

VOL_XYZ = (112, 112, 99)
SUB = 97                       # subsample stride
GLOBAL_OUT, LOCAL_OUT = (64, 64, 35), (16, 16, 16)
# (start x, y, z, source sizes, output shape)
CASES = [
    ((0, 0, 0), (96, 96, 67), GLOBAL_OUT), ((5, 9, 0), (96, 96, 99), GLOBAL_OUT), ((0, 0, 20), (112, 112, 67), GLOBAL_OUT),
    ((30, 11, 40), (64, 64, 35), GLOBAL_OUT),
    ((20, 40, 3), (64, 64, 67), GLOBAL_OUT), ((7, 3, 0), (64, 64, 99), GLOBAL_OUT), ((31, 17, 30), (80, 80, 67), GLOBAL_OUT),
    ((50, 60, 50), (32, 32, 35), GLOBAL_OUT),
    ((10, 20, 30), (32, 32, 16), LOCAL_OUT), ((40, 41, 42), (16, 16, 16), LOCAL_OUT), ((60, 70, 60), (32, 32, 32), LOCAL_OUT),
    ((3, 90, 5), (8, 8, 8), LOCAL_OUT),
    ((111, 111, 98), (1, 1, 1), LOCAL_OUT), ((111, 50, 83), (1, 16, 16), LOCAL_OUT), ((45, 111, 91), (32, 1, 8), LOCAL_OUT),
    ((100, 98, 98), (12, 14, 1), LOCAL_OUT), ((81, 90, 70), (31, 22, 29), LOCAL_OUT), ((94, 0, 67), (18, 17, 32), LOCAL_OUT),
    ((104, 105, 93), (8, 7, 6), LOCAL_OUT), ((88, 10, 80), (24, 32, 19), LOCAL_OUT),
]


def phantom():
    """int16 [z, y, x]: ellipsoids of fixed HU values (air, lung, tissue, bone, values near the -150 HU threshold) over -1200 HU, plus
    +-2 HU of noise (compresses well; the filter and zoom see smooth fields and sharp edges)."""
    rng = np.random.default_rng(20261016)
    X, Y, Z = VOL_XYZ
    z, y, x = np.mgrid[0:Z, 0:Y, 0:X]
    v = np.full((Z, Y, X), -1200, dtype=np.int32)
    for _ in range(40):
        c = rng.uniform([0, 0, 0], [X, Y, Z])
        r = rng.uniform([6, 6, 5], [40, 40, 30])
        hu = int(rng.choice([-1100, -850, -400, -160, -150, -140, 0, 60, 700, 1000, 1600]))
        m = ((x - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((z - c[2]) / r[2]) ** 2 <= 1.0
        v[m] = hu
    v += rng.integers(-2, 3, v.shape)
    return v.astype(np.int16)


def scipy_resize(img, shape):
    import scipy.ndimage as ndi
    factors = np.divide(img.shape, shape)
    lo, hi = img.min(), img.max()
    f = img
    if any(o < i for i, o in zip(img.shape, shape)):
        f = ndi.gaussian_filter(img, np.maximum(0, (factors - 1) / 2), cval=0, mode="mirror")
    out = ndi.zoom(f, [1 / q for q in factors], order=1, mode="mirror", cval=0, grid_mode=True)
    np.clip(out, lo, hi, out=out)
    return out


def make(out_dir):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import luna_prep_reference as R
    vol = phantom()
    logical = R.normalise(vol.transpose(2, 1, 0))
    digests, subs, scores = [], [], []
    for start, src, oshape in CASES:
        crop = logical[start[0]:start[0] + src[0], start[1]:start[1] + src[1], start[2]:start[2] + src[2]]
        assert crop.shape == src, (start, src)
        out = crop if src == (64, 64, 35) else scipy_resize(crop, oshape)
        assert out.shape == oshape
        out = np.ascontiguousarray(out, dtype=np.float64)
        digests.append(np.frombuffer(hashlib.sha256(out.tobytes()).digest(), dtype=np.uint8))
        subs.append(out.reshape(-1)[::SUB])
        scores.append(R.depth_score(out) if oshape == GLOBAL_OUT else -1)
    path = os.path.join(out_dir, "luna_prep_windows.npz")
    np.savez_compressed(path, vol=vol, start=np.array([c[0] for c in CASES]), src=np.array([c[1] for c in CASES]),
                        out_shape=np.array([c[2] for c in CASES]), sha256=np.stack(digests), sub=np.concatenate(subs),
                        sub_len=np.array([len(s) for s in subs]), score=np.array(scores), sub_stride=SUB)
    print(path, os.path.getsize(path), "bytes")
    return path


if __name__ == "__main__":
    make(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden"))
