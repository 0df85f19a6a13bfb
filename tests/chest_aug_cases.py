"""Case tables and input builders for csrc/augment2d.hip at its edges (test_chest_aug_cases_cpu.py, test_chest_augment_edges_gpu.py): the
every-colour image and the table of distinct HSV triples, the hue shifts and blend factors, the resampling boxes, the tall crops that enter
hresample_kernel's grid-stride loop, the blur, contrast, rotation, cut-out and jitter-order records, and one mixed gray / RGB launch.  Not a
test file.  Every input comes from a seed or a formula; the expected values come from tests/chest_aug_reference.py, which
test_chest_aug_cases_cpu.py holds to Pillow itself on these same cases.

Records are int64 [NPARAM] in the layout of pcrlv2_amd/data_chest.py.  Images are uint8 [H, W, C]."""
import functools
import itertools

import numpy as np

import chest_aug_reference as R
from norm_pool_cases import _tokens, read_source
from pcrlv2_amd import data_chest as DC

# ---- the constants of the source, restated (test_chest_aug_cases_cpu.py compares them with the source text token by token) ----
BLUR_RMAX = 4                    # box_line's hist[] holds BLUR_RMAX + 1 overwritten pixels
HRESAMPLE_BLOCKS = 1024          # pcrl_aug2d_hresample's grid cap along x
HRESAMPLE_THREADS = 256
HRESAMPLE_CAP = HRESAMPLE_BLOCKS * HRESAMPLE_THREADS       # 262 144 items in one step of the grid-stride loop
V_MAX, S_MAX = 65535, 4096
PHOTOMETRIC_SIDES = (224, 96)

SOURCE_PINS = [
    ("augment2d.hip", "constexpr int BLUR_RMAX = 4;"),
    ("augment2d.hip", "(work + 255) / 256 < 1024 ? (work + 255) / 256 : 1024"),
    ("augment2d.hip", "hipLaunchKernelGGL(hresample_kernel, dim3(gx, V), dim3(256)"),
    ("augment2d.hip", "V > 0 && V <= 65535 && S > 0 && max_rows > 0"),
    ("augment2d.hip", "V > 0 && V <= 65535 && S > 0 && S <= 4096"),
    ("augment2d.hip", "photometric_kernel<224>"),
    ("augment2d.hip", "photometric_kernel<96>"),
]


def source_pins_missing(pins=None):
    """-> the pins whose token sequence does not occur in their file"""
    missing = []
    for f, text in SOURCE_PINS if pins is None else pins:
        hay, pin = " ".join(_tokens(read_source(f))), " ".join(_tokens(text))
        if f" {pin} " not in f" {hay} ":
            missing.append((f, text))
    return missing


def identity_record(S, **kw):
    """A record that does nothing but the angle-0 rotation; keywords name the P_* fields in lower case (order=..., bri=...)."""
    r = np.zeros(DC.NPARAM, np.int64)
    r[DC.P_A0:DC.P_A5 + 1] = DC.rotate_fixed(0.0, S, S)
    for k, v in kw.items():
        r[getattr(DC, "P_" + k.upper())] = v
    return r


def f32_bits(x):
    return int(np.float32(x).view(np.int32))


def bits_f32(b):
    return float(np.array(b, np.int64).astype(np.int32).view(np.float32))


def source_image(H, W, C, seed, low=0):
    return np.random.default_rng(seed).integers(low, 256, (H, W, C), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------
# Colours
# ---------------------------------------------------------------------------------------------------------------
HUE_SHIFTS = (0, 1, 102, 154, 255)          # DC.hue_shift(+-0.4) = 102 / 154 and their neighbours at the wrap; shift 0 is not an identity
BLEND_FACTORS = {                            # float32 bit patterns
    "0.6": f32_bits(0.6), "1.4": f32_bits(1.4), "1-": 0x3f7fffff, "1+": 0x3f800001, "1": 0x3f800000, "0": 0, "denormal": 1,
}
FULL_FACTORS = ("0.6", "1.4")               # saturation on every colour; the other factors on the pre-image table
COLOUR_SIDE = 224


@functools.lru_cache(maxsize=None)
def every_colour():
    """uint8 [2^24, 3]: colour c is (c >> 16, c >> 8 & 255, c & 255)."""
    c = np.arange(2 ** 24, dtype=np.uint32)
    return np.stack([c >> 16, (c >> 8) & 255, c & 255], -1).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def every_colour_hsv():
    """R._rgb2hsv of every colour, as three uint8 arrays [2^24] (computed once per process)."""
    rgb = every_colour()
    parts = [R._rgb2hsv(rgb[k:k + 2 ** 21][None]) for k in range(0, 2 ** 24, 2 ** 21)]
    return tuple(np.concatenate([p[c][0] for p in parts]).astype(np.uint8) for c in range(3))


@functools.lru_cache(maxsize=None)
def hsv_preimages():
    """-> (uint8 [n, 3] RGB, uint8 [n, 3] HSV): one RGB pre-image (the smallest colour index) of every distinct triple R._rgb2hsv produces."""
    h, s, v = every_colour_hsv()
    key = (h.astype(np.uint32) << 16) | (s.astype(np.uint32) << 8) | v
    _, first = np.unique(key, return_index=True)
    return every_colour()[first], np.stack([h[first], s[first], v[first]], -1)


def colour_views(rgb, S=COLOUR_SIDE):
    """uint8 [n, 3] colours -> uint8 [V, 3, S, S] planar views, the last padded with colour 0."""
    n = rgb.shape[0]
    V = -(-n // (S * S))
    flat = np.zeros((V * S * S, 3), np.uint8)
    flat[:n] = rgb
    return np.ascontiguousarray(flat.reshape(V, S * S, 3).transpose(0, 2, 1)).reshape(V, 3, S, S)


def view_colours(u8):
    """uint8 [V, 3, S, S] -> uint8 [V * S * S, 3]: colour_views undone, the padding kept."""
    V = u8.shape[0]
    return np.ascontiguousarray(u8.reshape(V, 3, -1).transpose(0, 2, 1)).reshape(-1, 3)


def hue_of_hsv(hsv, shift):
    """R.hue from an HSV decomposition that is already there: uint8 [n, 3] HSV -> uint8 [n, 3] RGB."""
    out = np.empty((hsv.shape[0], 3), np.uint8)
    for k in range(0, hsv.shape[0], 2 ** 21):
        h, s, v = (hsv[k:k + 2 ** 21, c].astype(np.int64) for c in range(3))
        out[k:k + 2 ** 21] = R._hsv2rgb((h + shift) % 256, s, v)
    return out


def on_colours(fn, rgb):
    """An image operation of chest_aug_reference on a colour table uint8 [n, 3] (as a 1 x n image, in chunks) -> uint8 [n, 3]."""
    out = np.empty_like(rgb)
    for k in range(0, rgb.shape[0], 2 ** 21):
        out[k:k + 2 ** 21] = fn(rgb[k:k + 2 ** 21][None])[0]
    return out


def normalize_table():
    """float32 [3, 256]: R.normalize of every byte in every plane."""
    return np.ascontiguousarray(R.normalize(np.arange(256, dtype=np.uint8).reshape(1, 256, 1)).reshape(3, 256))


def byte_ramp(C, S=96):
    """uint8 [S, S, C]: every byte value, 36 times; the planes of an RGB ramp are shifted against each other."""
    k = np.arange(S * S, dtype=np.int64).reshape(S, S, 1)
    return ((k + np.arange(C) * 85) % 256).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------
# Resampler
# ---------------------------------------------------------------------------------------------------------------
RESAMPLE_SIDES = (8, 17)


def resample_sizes(S):
    return (1, 2, S - 1, S, S + 1, 4 * S + 3)


def clamp_sizes(S):
    """the sizes at which a pass barely or strongly rescales: some output index has an active xmin or xmax clamp"""
    return (S - 1, S + 1, 4 * S + 3)


def raw_bounds(in_size, out_size):
    """Coeffs' xmin and xmax BEFORE their clamps to [0, in_size], and the tap count after them, per output index."""
    scale = float(np.float32(in_size)) / out_size
    support = max(scale, 1.0)
    lo, hi, n = [], [], []
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        lo.append(int(center - support + 0.5))
        hi.append(int(center + support + 0.5))
        n.append(min(hi[-1], in_size) - max(lo[-1], 0))
    return lo, hi, n


def resample_boxes():
    """-> [(H, W, C, j, i, cw, ch, S)]: every (cw, ch) of resample_sizes(S)^2 for S in RESAMPLE_SIDES (every other box sits inside a larger
    source, so a tap outside the box reads foreign pixels), a crop in each corner of a larger source, and one box of each production side."""
    boxes, k = [], 0
    for S in RESAMPLE_SIDES:
        for ch in resample_sizes(S):
            for cw in resample_sizes(S):
                m = k % 2
                boxes.append((ch + 3 * m, cw + 2 * m, 1 if (k // 2) % 2 == 0 else 3, m, 2 * m, cw, ch, S))
                k += 1
    H, W, cw, ch = 40, 50, 31, 23
    for n, (j, i) in enumerate(((0, 0), (W - cw, 0), (0, H - ch), (W - cw, H - ch))):
        boxes.append((H, W, 1 if n % 2 else 3, j, i, cw, ch, 17))
    boxes.append((157, 183, 3, 20, 11, 140, 120, 96))
    boxes.append((300, 257, 1, 5, 7, 250, 290, 224))
    return boxes


def box_source(box, seed):
    H, W, C = box[:3]
    return source_image(H, W, C, 1000 + seed)


def box_record(box):
    H, W, C, j, i, cw, ch, S = box
    return identity_record(S, h=H, w=W, c=C, j=j, i=i, cw=cw, ch=ch)


# The tall crops: ch * S items against the 262 144 the capped grid covers in one step.  1200 rows overshoot by 6656 = 26 * 256, whole blocks;
# 1203 rows by 7328 = 28 * 256 + 160, so the last block of the second step is a partial one.  Both stay below Pillow's 100 : 1 (see
# TALL_BOUNDARY).  The second view of the launch is short, so max_rows = 40 leaves almost all of the tall view to the stride loop.
TALL_S, TALL_W, TALL_ROWS, TALL_OTHER_ROWS = 224, 16, (1200, 1203), 40


def tall_case(rows):
    """-> (sources, records): a rows x 16 one-plane source, full crop, and a second view of 40 rows, both at S = 224."""
    a, b = source_image(rows, TALL_W, 1, 77), source_image(64, 48, 1, 78)
    recs = np.stack([identity_record(TALL_S, h=rows, w=TALL_W, c=1, cw=TALL_W, ch=rows),
                     identity_record(TALL_S, h=64, w=48, c=1, j=3, i=9, cw=41, ch=TALL_OTHER_ROWS)])
    return [a, b], recs


# Pillow's resize runs the VERTICAL pass first once a crop is more than 100 times as tall as it is wide (and taller than the output);
# R.resize and the kernels always run the horizontal pass first.  (cw, ch, S, horizontal first equals Pillow)
TALL_BOUNDARY = [(cw, 100 * cw + d, S, d == 0) for S in (8, 96, 224) for cw in (3, 4, 7) for d in (0, 1)] + [
    (2, 128 * 2, 8, False), (3, 128 * 3, 224, False), (2, 224, 224, True), (2, 225, 224, False), (16, 1200, 224, True), (16, 1203, 224, True)]


# ---------------------------------------------------------------------------------------------------------------
# Photometric records (S = 96 unless said otherwise)
# ---------------------------------------------------------------------------------------------------------------
PS = 96
BLUR_SIGMAS = (0.1, 1.5, 2.5, 3.5, 4.9)        # DC.blur_params -> radii 0, 1, 2, 3, 4


def blur_images(C, S=PS):
    """-> [(name, uint8 [S, S, C])]: impulses in the first two and last two rows and columns (another amplitude per plane), a random image,
    an all-255 image."""
    amp = np.array([255, 128, 77][:C], np.uint8)
    out = []
    for p in (0, 1, S - 2, S - 1):
        a = np.zeros((S, S, C), np.uint8)
        a[p, S // 2] = a[S // 2, p] = a[p, p] = a[p, S - 1 - p] = amp
        out.append((f"impulse{p}", a))
    out.append(("random", source_image(S, S, C, 31 + C)))
    out.append(("white", np.full((S, S, C), 255, np.uint8)))
    return out


def colour_with_luma(l, r, g):
    """an RGB colour with the given r and g, not gray, whose Convert.c luma is l"""
    for b in range(256):
        if (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16 == l:
            return (r, g, b)
    raise ValueError((l, r, g))


CONTRAST_FACTORS = ("0.6", "1.4")


def contrast_images(C, S=PS):
    """-> [(name, uint8 [S, S, C], the mean contrast must blend with)]: luma 100 everywhere but k scattered pixels of luma 101, k on either
    side of SS / 2 where (2 tot + SS) / (2 SS) steps from 100 to 101; all 0; all 255."""
    SS = S * S
    lo, hi = ((100,), (101,)) if C == 1 else (colour_with_luma(100, 140, 90), colour_with_luma(101, 60, 125))
    out = []
    for k, mean in ((SS // 2 - 1, 100), (SS // 2, 101), (SS // 2 + 1, 101)):
        a = np.empty((SS, C), np.uint8)
        a[:] = lo
        a[np.random.default_rng(k).permutation(SS)[:k]] = hi
        out.append((f"k={k}", a.reshape(S, S, C), mean))
    out.append(("black", np.zeros((S, S, C), np.uint8), 0))
    out.append(("white", np.full((S, S, C), 255, np.uint8), 255))
    return out


ROT_ANGLES = (10.0, -10.0, 9.999999, 1e-9, 0.0, 5.0, 1e-14)      # 1e-14: the sine rounds to zero at 15 digits (rotate_fixed's identity branch)
ROT_SIDES = (8, 17, 96, 224)
ROT_IDENTITY = (1e-9, 0.0, 1e-14)                                  # the 16.16 matrix is the identity: no pixel is fill


def rotation_has_fill(angle, S):
    """Whether a rotation of an S x S image by `angle` must read outside: every angle that is no identity, except 5 degrees at S = 8, where
    the corner pixel's centre (3.5, 3.5) from the middle stays inside (3.5 (cos 5 + sin 5) = 3.79 < 4)."""
    return angle not in ROT_IDENTITY and not (angle == 5.0 and S == 8)


def rotation_cases(S):
    """-> [(angle, flip, C)] for one side; C alternates."""
    return [(a, f, 1 if (n + f) % 2 == 0 else 3) for n, a in enumerate(ROT_ANGLES) for f in (0, 1)]


def rotation_source(S, C):
    return source_image(S, S, C, 500 + S + C, low=1)           # no zero pixel: a 0 in the output is fill


def rotation_record(S, angle, flip, C):
    r = identity_record(S, h=S, w=S, c=C, cw=S, ch=S, flip=flip)
    r[DC.P_A0:DC.P_A5 + 1] = DC.rotate_fixed(angle, S, S)
    return r


def hole_sets(S):
    """-> [[(y0, y1, x0, x1)]]: none; one clipped at each corner; two apart; three overlapping; one over the whole view."""
    return [[], [(0, 10, 0, 7)], [(0, 16, S - 5, S)], [(S - 16, S, 0, 1)], [(S - 1, S, S - 12, S)],
            [(3, 35, 4, 36), (S - 40, S - 8, S - 33, S - 1)],
            [(20, 52, 20, 52), (30, 62, 40, 72), (36, 68, 10, 42)], [(0, S, 0, S)]]


def holes_record(S, holes, **kw):
    r = identity_record(S, nholes=len(holes), **kw)
    for k, h in enumerate(holes):
        r[DC.P_HOLES + 4 * k:DC.P_HOLES + 4 * k + 4] = h
    return r


JITTER_FACTORS = (0.731, 1.262, 0.644)       # brightness, contrast, saturation
JITTER_HUE = 37


def jitter_records(S=PS):
    """-> [(ops, record)]: every permutation of the four operations, cut after nops = 0 .. 4."""
    out = []
    for perm in itertools.permutations(range(4)):
        for nops in range(5):
            order = sum(op << (4 * k) for k, op in enumerate(perm))
            out.append((perm[:nops], identity_record(S, c=3, nops=nops, order=order, bri=f32_bits(JITTER_FACTORS[0]), con=f32_bits(JITTER_FACTORS[1]),
                                                     sat=f32_bits(JITTER_FACTORS[2]), hue=JITTER_HUE)))
    return out


# ---------------------------------------------------------------------------------------------------------------
# One launch of gray and RGB views, interleaved
# ---------------------------------------------------------------------------------------------------------------
LAYOUT_PAD = 1          # bytes in front of the first source: its offset is odd


def layout_case(S=PS):
    """-> (images, sample index per view, records with P_SRC / P_INTER set, packed source bytes).  Four sources (gray, RGB, gray, RGB; the gray
    ones of odd size) behind one pad byte; eight drawn views, gray and RGB alternating, with grayscale, blur, all four jitter operations and
    three cut-out holes each."""
    shapes = ((57, 61, 1), (64, 49, 3), (75, 33, 1), (41, 83, 3))
    imgs = [source_image(*sh, seed=900 + n) for n, sh in enumerate(shapes)]
    sample = np.arange(8) % 4
    rng = np.random.default_rng(12)
    H, W, C = (np.array([shapes[n][k] for n in sample]) for k in range(3))
    rec = DC.draw_views(rng, H, W, C, S, (0.3, 1.0), cutout=True)
    rec[:, DC.P_BLUR] = [1, 1, 0, 0, 1, 1, 0, 0]
    rec[:, DC.P_GRAY] = [0, 1, 1, 0, 0, 0, 1, 1]
    sizes = np.array([a.size for a in imgs])
    offs = LAYOUT_PAD + np.concatenate([[0], np.cumsum(sizes)[:-1]])
    DC.pack_offsets(rec, offs, sample, S)
    src = np.concatenate([np.full(LAYOUT_PAD, 0xEE, np.uint8)] + [a.reshape(-1) for a in imgs])
    return imgs, sample, rec, src
