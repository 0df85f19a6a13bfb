"""Case table, lattice and derived bounds for csrc/seg_augment.hip (test_seg_aug_cpu.py, test_seg_aug_gpu.py).  Not a test file.

pcrl_seg_aug_resample takes its per-sample coefficients (inverse matrix and translation, gain, bias) as INPUTS, so the kernel is judged alone against
seg_aug_reference.ref_resample (float64).  What is compared with what:

  lattice   bits (image) and bytes (label).  inv entries k/8, translations k/8, output centres j/2 and box centres j/2: a sampling coordinate and
            its three fractions are multiples of 1/16 with |s| < 2^10, a corner weight is a multiple of 2^-12 <= 1; the data are integers |v| <= 64
            (exact in float16 too): a product v w and every partial sum of the eight are multiples of 2^-12 below 2^7, 19 bits; gains k/4, k <= 8:
            gain * T is a multiple of 2^-14 <= 128, 21 bits; integer biases |b| <= 16: a multiple of 2^-14 <= 144, 22 bits.  Nothing is ever
            rounded in float32, in any corner order, fused or not (lattice_violations, resample_steps; test_seg_aug_cpu.py).  s + 0.5 is exact as
            well, so the nearest voxel -- ties at .5 included, s = -0.5 -> voxel 0, s = -0.5625 -> outside -- is the float64 one.
  generic   rotations and zooms: generic_bound()'s derived bound on the image; labels where the float64 coordinate is further than D_COORD from a
            tie on every axis (at most 1 % of a case may be excluded; about 6 D_COORD = 0.07 % are).
"""
import itertools

import numpy as np

import aug_cases
import seg_aug_reference as R

U = 2.0 ** -24                   # unit roundoff of float32
D_COORD = 2.0 ** -13             # float32 sampling coordinate against the float64 one, extents <= 128 (generic_bound)
NOT_COUNTED = 0x80

# ========================================================================================================================================
# lattice
# ========================================================================================================================================
TRANSLATION = (1 / 8, -3 / 8, 1 / 2)
LATTICE_EXTENTS = [((9, 11, 7), (5, 7, 3)), ((12, 10, 6), (8, 8, 8)), ((24, 22, 12), (16, 16, 8)), ((6, 6, 70), (4, 4, 66))]   # source -> crop
LATTICE_C = (1, 3, 4)
DATA_MAX, GAIN_DEN, GAIN_MAX_K, BIAS_MAX = 64, 4, 8, 16


def lattice_matrices():
    """[(name, M float64 [3, 3], t float64 [3])]: the identity, the 47 other signed permutations, diag(7/8, 9/8, 5/4), the two shears of
    aug_cases.affine_matrices, 3 I (most of the crop outside the box), and each of them with the translation (1/8, -3/8, 1/2)"""
    eye = np.eye(3)
    ms = [("identity", eye)]
    ms += [(f"signed permutation {k}", m.numpy()) for k, m in enumerate(aug_cases.signed_permutations()) if not np.array_equal(m.numpy(), eye)]
    ms.append(("diag(7/8, 9/8, 5/4)", np.diag([7 / 8, 9 / 8, 5 / 4])))
    ms += [(n, m.numpy()) for n, m in aug_cases.affine_matrices() if n.startswith("shear")]
    ms.append(("zoom out 3", 3.0 * eye))
    assert len(ms) == 52
    zero, t = np.zeros(3), np.array(TRANSLATION)
    return [(n, m.astype(np.float64), zero) for n, m in ms] + [(n + " + t", m.astype(np.float64), t) for n, m in ms]


def lattice_case(extent, crop, C, half, seed=0):
    """-> dict: src [B, C, *extent] float32 / float16 integers, src_lab uint8 [B, *extent] (any byte), inv float32 [B, 12], gain, bias float32 [B, C],
    names.  One sample per matrix: a different matrix, gain, bias and volume per b (a kernel that reads another sample's row gets another result)."""
    ms = lattice_matrices()
    B = len(ms)
    rng = np.random.default_rng([seed, sum(extent), C, int(half)])
    src = rng.integers(-DATA_MAX, DATA_MAX + 1, (B, C) + tuple(extent)).astype(np.float16 if half else np.float32)
    src_lab = rng.integers(0, 256, (B,) + tuple(extent)).astype(np.uint8)
    inv = np.stack([np.concatenate([m, t[:, None]], axis=1).reshape(12) for _, m, t in ms]).astype(np.float32)
    gain = (rng.integers(0, GAIN_MAX_K + 1, (B, C)) / GAIN_DEN).astype(np.float32)
    bias = rng.integers(-BIAS_MAX, BIAS_MAX + 1, (B, C)).astype(np.float32)
    return {"src": src, "src_lab": src_lab, "inv": inv, "gain": gain, "bias": bias, "crop": tuple(crop), "extent": tuple(extent), "names": [n for n, _, _ in ms]}


def lattice_cases():
    """(id, extent, crop, C, half) of every bit-for-bit case"""
    return [(f"{'x'.join(map(str, e))}->{'x'.join(map(str, c))}-C{C}-{'f16' if half else 'f32'}", e, c, C, half)
            for (e, c), C, half in itertools.product(LATTICE_EXTENTS, LATTICE_C, (False, True))]


def _is_f32(v):
    return np.array_equal(v.astype(np.float32).astype(np.float64), v)


def lattice_violations(case):
    """-> the preconditions of the bit-for-bit claim that this case breaks (none: [])"""
    bad = []
    inv = case["inv"].astype(np.float64)
    if not np.array_equal(inv * 8, np.round(inv * 8)):
        bad.append("an inv entry is no multiple of 1/8")
    src = case["src"].astype(np.float64)
    if not (np.array_equal(src, np.round(src)) and np.abs(src).max() <= DATA_MAX and np.array_equal(src.astype(np.float16).astype(np.float64), src)):
        bad.append("the data are not integers |v| <= 64 that float16 holds")
    g, b = case["gain"].astype(np.float64), case["bias"].astype(np.float64)
    if not (np.array_equal(g * GAIN_DEN, np.round(g * GAIN_DEN)) and g.min() >= 0 and g.max() <= GAIN_MAX_K / GAIN_DEN):
        bad.append("a gain is not k/4 with 0 <= k <= 8")
    if not (np.array_equal(b, np.round(b)) and np.abs(b).max() <= BIAS_MAX):
        bad.append("a bias is no integer |b| <= 16")
    s = R.coords(case["inv"], case["extent"], case["crop"])
    if not (np.array_equal(s * 16, np.round(s * 16)) and np.abs(s).max() < 2.0 ** 10):
        bad.append("a coordinate is no multiple of 1/16 below 2^10")
    t = s - np.floor(s)
    B, C = case["src"].shape[:2]
    for reverse in (False, True):
        corners = list(itertools.product((0, 1), repeat=3))
        acc = np.zeros((B, C) + case["crop"])
        f = np.floor(s).astype(np.int64)
        bi = np.arange(B).reshape(B, 1, 1, 1)
        for a in (corners[::-1] if reverse else corners):
            w = np.ones_like(t[:, 0])
            for k in range(3):
                w = w * (t[:, k] if a[k] else 1.0 - t[:, k])
            if not np.array_equal(w * 4096, np.round(w * 4096)):
                bad.append("a corner weight is no multiple of 2^-12")
            idx = [f[:, k] + a[k] for k in range(3)]
            inside = np.ones(idx[0].shape, dtype=bool)
            for k in range(3):
                inside &= (idx[k] >= 0) & (idx[k] < case["extent"][k])
            cl = [np.clip(idx[k], 0, case["extent"][k] - 1) for k in range(3)]
            for ch in range(C):
                term = np.where(inside, src[bi, ch, cl[0], cl[1], cl[2]], 0.0) * w
                acc[:, ch] += term
                if not (_is_f32(term) and _is_f32(acc[:, ch])):
                    bad.append("a product or a partial sum needs more than 24 bits")
        gt = g.reshape(B, C, 1, 1, 1) * acc
        if not (_is_f32(gt) and _is_f32(gt + b.reshape(B, C, 1, 1, 1))):
            bad.append("gain * T or gain * T + bias needs more than 24 bits")
    return sorted(set(bad))


def _fma(a, b, c):
    """float32 fused multiply-add: the product of two float32 values is exact in float64"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def resample_steps(case, reverse=False, fused=False):
    """The image path of seg_aug_kernel operation by operation in numpy float32: `fused` contracts every multiply-add, `reverse` walks the corners
    and the coordinate's terms in the opposite order.  -> y float32 [B, C, *crop]"""
    f = np.float32
    src, inv, crop, ext = case["src"].astype(f), case["inv"].astype(f).reshape(-1, 3, 4), case["crop"], case["extent"]
    B, C = src.shape[:2]
    grid = np.meshgrid(*[(np.arange(n).astype(f) + f(0.5)) - f(0.5) * f(n) for n in crop], indexing="ij")
    c = [np.broadcast_to(g, (B,) + tuple(crop)).astype(f) for g in grid]
    s = []
    for r in range(3):
        m = [inv[:, r, k].reshape(B, 1, 1, 1) for k in range(4)]
        centre = np.full((B,) + tuple(crop), f(0.5) * f(ext[r]) - f(0.5), dtype=f)
        if fused:
            v = _fma(m[2], c[2], _fma(m[1], c[1], (m[0] * c[0]).astype(f)))
            v = ((v + m[3]).astype(f) + centre).astype(f)
        else:
            terms = [(m[k] * c[k]).astype(f) for k in range(3)] + [np.broadcast_to(m[3], centre.shape).astype(f), centre]
            terms = terms[::-1] if reverse else terms
            v = terms[0]
            for tm in terms[1:]:
                v = (v + tm).astype(f)
        s.append(v)
    fl = [np.floor(v) for v in s]
    t = [(v - w).astype(f) for v, w in zip(s, fl)]
    fl = [w.astype(np.int64) for w in fl]
    corners = list(itertools.product((0, 1), repeat=3))
    acc = np.zeros((B, C) + tuple(crop), dtype=f)
    bi = np.arange(B).reshape(B, 1, 1, 1)
    for a in (corners[::-1] if reverse else corners):
        w = (((t[0] if a[0] else f(1) - t[0]) * (t[1] if a[1] else f(1) - t[1])).astype(f) * (t[2] if a[2] else f(1) - t[2])).astype(f)
        idx = [fl[k] + a[k] for k in range(3)]
        inside = np.ones(idx[0].shape, dtype=bool)
        for k in range(3):
            inside &= (idx[k] >= 0) & (idx[k] < ext[k])
        cl = [np.clip(idx[k], 0, ext[k] - 1) for k in range(3)]
        for ch in range(C):
            v = np.where(inside, src[bi, ch, cl[0], cl[1], cl[2]], f(0)).astype(f)
            acc[:, ch] = _fma(v, w, acc[:, ch]) if fused else (acc[:, ch] + (v * w).astype(f)).astype(f)
    g, b = case["gain"].astype(f).reshape(B, C, 1, 1, 1), case["bias"].astype(f).reshape(B, C, 1, 1, 1)
    return _fma(g, acc, np.broadcast_to(b, acc.shape)) if fused else ((g * acc).astype(f) + b).astype(f)


def tie_coordinates(case):
    """-> the set of fractional coordinate values s (as multiples of 1/16, only those within (-1, 0)) and whether an exact .5 tie occurs"""
    s = R.coords(case["inv"], case["extent"], case["crop"])
    near = s[(s > -1) & (s < 0)]
    return set(np.unique(near).tolist()), bool((s - np.floor(s) == 0.5).any())


# ========================================================================================================================================
# generic rotations and zooms
# ========================================================================================================================================
GENERIC_EXTENT, GENERIC_CROP, GENERIC_C, GENERIC_DRAWS = (24, 22, 12), (16, 16, 8), 2, 12
GENERIC_ROTATE, GENERIC_SCALE = 15.0, (0.8, 1.25)        # the extremes of `--augment`'s defaults
MAX_EXCLUDED = 0.01


def _rotation(angles):
    (sa, sb, sg), (ca, cb, cg) = np.sin(angles), np.cos(angles)
    rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    rz = np.array([[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]])
    return rx @ ry @ rz


def generic_case(seed=0):
    """Twelve seeded rotation-plus-zoom draws at the extremes of the defaults: every angle +-15 degrees (the sign drawn), the zoom 0.8 or 1.25
    (alternating), flips drawn; Gaussian data with a raised ellipsoid; gains and biases inside the defaults' ranges.  One sample per draw."""
    rng = np.random.default_rng([seed, 77])
    B, C = GENERIC_DRAWS, GENERIC_C
    inv = []
    for b in range(B):
        angles = np.deg2rad(GENERIC_ROTATE) * rng.choice([-1.0, 1.0], 3)
        flips = np.diag(rng.choice([-1.0, 1.0], 3))
        m = _rotation(angles) @ flips / GENERIC_SCALE[b % 2]
        inv.append(np.concatenate([m, np.zeros((3, 1))], axis=1).reshape(12))
    src = rng.standard_normal((B, C) + GENERIC_EXTENT).astype(np.float32)
    src[:, :, 8:16, 6:15, 3:9] += np.float32(2.5)
    src_lab = rng.integers(0, 8, (B,) + GENERIC_EXTENT).astype(np.uint8)
    src_lab[:, :2] |= NOT_COUNTED
    gain = rng.uniform(0.75, 1.25, (B, C)).astype(np.float32)
    bias = rng.uniform(-0.1, 0.1, (B, C)).astype(np.float32)
    return {"src": src, "src_lab": src_lab, "inv": np.stack(inv).astype(np.float32), "gain": gain, "bias": bias, "crop": GENERIC_CROP,
            "extent": GENERIC_EXTENT}


def neighbour_difference(src):
    """The largest |difference| of two neighbouring voxels along any axis, of every (sample, channel) volume padded with one voxel of 0 (what
    lies outside the box): [B, C]"""
    p = np.pad(np.asarray(src, dtype=np.float64), ((0, 0), (0, 0), (1, 1), (1, 1), (1, 1)))
    return np.max([np.abs(np.diff(p, axis=a)).max(axis=(2, 3, 4)) for a in (2, 3, 4)], axis=0)


def generic_bound(case):
    """-> bound float64 [B, C] on |kernel - ref_resample| for the image.

    Coordinates.  The kernel forms c = i + 0.5 - X / 2 exactly (halves below 2^7) and s = m0 cx + m1 cy + m2 cz + t + (S / 2 - 0.5) in 7 float32
    operations (3 products, 4 sums; a fused multiply-add only removes roundings) on values below 256 for extents <= 128, each off by at most
    2^-24 * 256: |s~ - s| <= 7 * 2^-16 < d = 2^-13 = D_COORD.  The restatement evaluates the same float32 inv in float64.
    Sample.  T is continuous and, along one axis with the other two fixed, piecewise linear with a slope that is a convex combination of
    differences of neighbouring voxels of the zero-padded volume, so |slope| <= L = neighbour_difference: moving the coordinate axis by axis,
        |T(s~) - T(s)| <= 3 d L.
    Arithmetic.  At s~ the fractions t = s~ - floor(s~) are exact; the eight terms v_k w_k are added into one float32 sum: eight roundings, each at
    most u = 2^-24 of a partial sum that never exceeds A = max |v| (the weights are non-negative and sum to 1): 8 u A.  The remaining
    roundings -- five in a weight, gain * T, + bias -- are 7 u (A |gain| + |bias|) at most; this case's extents are <= 32, where the 7 coordinate
    operations err by 7 * 2^-24 * 32 < d / 8, so 3 (d - d / 8) L |gain| of the first term is unused, and the function asserts that it
    covers them.  With the gain and the bias:
        |y~ - y| <= |gain| 3 d L + 8 u (|gain| A + |bias|)."""
    src = np.asarray(case["src"], dtype=np.float64)
    assert max(case["extent"]) <= 32 and max(case["crop"]) <= 32
    L = neighbour_difference(src)
    A = np.abs(src).max(axis=(2, 3, 4))
    g, b = np.abs(case["gain"].astype(np.float64)), np.abs(case["bias"].astype(np.float64))
    rounding = U * (g * A + b)
    assert (7 * rounding <= 3 * (D_COORD - D_COORD / 8) * L * g).all(), "the unused part of the coordinate term does not cover the weights' roundings"
    return g * 3 * D_COORD * L + 8 * rounding


def away_from_ties(s):
    """bool [B, *crop]: the float64 coordinate is further than D_COORD from a tie of the nearest-voxel rule (s + 0.5 an integer) on every axis"""
    h = s + 0.5
    return (np.abs(h - np.round(h)) > D_COORD).all(axis=1)


# ========================================================================================================================================
# label bits
# ========================================================================================================================================
def label_bits_case(seed=0):
    """A source whose labels use every bit 0..6 and 0x80 (bytes k * 17 % 127 and single bits, some with bit 7), under generic_case's geometry"""
    case = generic_case(seed)
    rng = np.random.default_rng([seed, 5])
    pool = np.array([1 << k for k in range(7)] + [0x7F, 0x55, 0x2A, 0x80, 0x81, 0xC0, 0], dtype=np.uint8)
    case["src_lab"] = pool[rng.integers(0, len(pool), case["src_lab"].shape)]
    return case


# ========================================================================================================================================
# the loader of the training-path tests
# ========================================================================================================================================
TRAIN_CROP, TRAIN_B, TRAIN_K = (16, 16, 8), 2, 3
TRAIN_C, TRAIN_SEED = 2, 2          # a seed whose counted voxels are settled (counted_voxels; test_seg_aug_cpu.py asserts it)


def train_batch(seed=TRAIN_SEED):
    """The first batch of CropLoader(synthetic cases, crop (16, 16, 8), b = 2, aug = the defaults with both probabilities 1)"""
    from pcrlv2_amd import data_seg as D
    cases = [D.synthetic_case(seed, i, D.synthetic_shape(TRAIN_CROP), TRAIN_K, TRAIN_C) for i in range(4)]
    cfg = D.AugConfig.defaults(p_spatial=1.0, p_intensity=1.0)
    return next(iter(D.CropLoader(cases, TRAIN_CROP, TRAIN_B, 1, seed, 0, aug=cfg)))


def counted_voxels(batch):
    """-> (the label bytes below 0x80 in the restatement of an augmented batch, settled): settled when every coordinate within D_COORD of the
    float64 one on every axis gives the same count -- the nearest index is monotone in the coordinate, so the eight corners of that box decide --
    and the kernel's float32 coordinates, which lie in the box (generic_bound), must then count the same voxels."""
    src_lab, inv = batch[1].numpy(), batch[2]["inv"].numpy()
    s = R.coords(inv, src_lab.shape[1:], tuple(int(c) for c in batch[2]["crop"]))
    base = R.nearest_labels(src_lab, s) < NOT_COUNTED
    settled = all(np.array_equal(R.nearest_labels(src_lab, s + np.array(d).reshape(1, 3, 1, 1, 1)) < NOT_COUNTED, base)
                  for d in itertools.product((-D_COORD, D_COORD), repeat=3))
    return int(base.sum()), settled
