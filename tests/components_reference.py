"""The reference of the connected-component kernels (csrc/components.hip, ops.label_components / filter_components, train_seg.postprocess_mask):
scipy.ndimage.label, and the mask generators of the tests.  Not a test file.

label_ref        scipy.ndimage.label with generate_binary_structure(3, 1 | 2 | 3) for connectivity 6 | 18 | 26, sizes by np.bincount.  scipy numbers the
                 components by the ascending C-order index of their first voxel; the kernels promise the same numbering, so the comparison is ==.
filter_ref       the two rules on (labels, sizes): keep_largest keeps the FIRST maximum of sizes (the lowest label among equals), min_voxels keeps
                 sizes >= min_voxels, both keeps what passes both; bit `bit` is cleared elsewhere, every other bit is copied.
postprocess_ref  class by class.

The generators return bool [X, Y, Z]; `embed` puts one into bit k of a byte whose other bits are random.
"""
import numpy as np

RANK = {6: 1, 18: 2, 26: 3}


def label_ref(mask, bit, connectivity):
    """-> (labels int32 [X, Y, Z], sizes int32 [n], n)"""
    from scipy import ndimage as ndi
    b = (mask >> bit & 1).astype(bool)
    labels, n = ndi.label(b, structure=ndi.generate_binary_structure(3, RANK[connectivity]))
    sizes = np.bincount(labels.ravel(), minlength=n + 1)[1:]
    return labels.astype(np.int32), sizes.astype(np.int32), int(n)


def filter_ref(mask, labels, sizes, bit, keep_largest=False, min_voxels=0):
    sizes = np.asarray(sizes, dtype=np.int64)
    keep = np.ones(len(sizes), dtype=bool)
    if keep_largest and len(sizes):
        first_max = min(i for i in range(len(sizes)) if sizes[i] == sizes.max())
        keep = np.arange(len(sizes)) == first_max
    if min_voxels > 0:
        keep = keep & (sizes >= min_voxels)
    out = mask.copy()
    drop = np.zeros(mask.shape, dtype=bool)
    on = labels > 0
    drop[on] = ~keep[labels[on] - 1]
    out[drop] &= np.uint8(~(1 << bit) & 0xFF)
    return out


def postprocess_ref(mask, K, keep_largest=(), min_voxels=0, connectivity=6):
    out = mask.copy()
    for k in range(K):
        if k not in keep_largest and min_voxels <= 0:
            continue
        labels, sizes, _ = label_ref(out, k, connectivity)
        out = filter_ref(out, labels, sizes, k, k in keep_largest, min_voxels)
    return out


def embed(b, bit, seed=0):
    """bool [X, Y, Z] -> uint8: bit `bit` from b, every other bit random."""
    rng = np.random.default_rng(seed)
    other = rng.integers(0, 256, b.shape, dtype=np.uint8) & np.uint8(~(1 << bit) & 0xFF)
    return np.ascontiguousarray(other | (b.astype(np.uint8) << bit))


# ---- generators -------------------------------------------------------------------------------------------------------------------------
def blobs(shape, seed=0, n=7):
    """A union of n random balls: a few ragged components, some touching."""
    rng = np.random.default_rng(seed)
    g = np.indices(shape).astype(np.float64)
    out = np.zeros(shape, dtype=bool)
    for _ in range(n):
        c = [rng.uniform(0, s) for s in shape]
        r = rng.uniform(1.0, max(1.5, 0.22 * max(shape)))
        out |= sum((g[a] - c[a]) ** 2 for a in range(3)) <= r * r
    return out


def noise(shape, p, seed=0):
    return np.random.default_rng(seed).random(shape) < p


def checker(shape):
    """(x + y + z) % 2 == 0: ceil(V / 2) single voxels at connectivity 6; one component at 18 and 26 where at least two axes exceed 1."""
    x, y, z = np.indices(shape)
    return (x + y + z) % 2 == 0


def corner_lattice(shape):
    """x = y = z mod 2: every voxel alone at 6 and 18, one component at 26 (where every axis exceeds 1): what separates 18 from 26."""
    x, y, z = np.indices(shape)
    return (x % 2 == y % 2) & (y % 2 == z % 2)


def snake(shape):
    """One one-voxel-wide path: the whole Z-line of every (even x, even y), neighbouring lines joined at alternating ends, so the path runs through
    every tile of at least 2 x 2 columns and crosses every tile face it meets: the longest parent chains.  One component at every connectivity."""
    X, Y, Z = shape
    m = np.zeros(shape, dtype=bool)
    line = 0
    xs = list(range(0, X, 2))
    for xi, x in enumerate(xs):
        ys = list(range(0, Y, 2))
        if xi % 2:
            ys.reverse()
        for yi, y in enumerate(ys):
            m[x, y, :] = True
            z_exit = Z - 1 if line % 2 == 0 else 0
            line += 1
            if yi + 1 < len(ys):
                m[x, (y + ys[yi + 1]) // 2, z_exit] = True
            elif xi + 1 < len(xs):
                m[x + 1, y, z_exit] = True
    return m


def comb(shape):
    """Parallel plates (every even y, all x and z) joined only by the last x-slab, the far end of the raster order: the provisional roots at x = 0 are
    relinked late.  One component at every connectivity."""
    m = np.zeros(shape, dtype=bool)
    m[:, ::2, :] = True
    m[-1, :, :] = True
    return m


def twins(shape):
    """Two components of equal size: the first and the last plane along the longest axis (which must have at least 3 voxels), and from 5 voxels on
    a single voxel between them.  The tie goes to the first plane."""
    axis = int(np.argmax(shape))
    assert shape[axis] >= 3
    m = np.zeros(shape, dtype=bool)
    sl = [slice(None)] * 3
    for i in (0, shape[axis] - 1):
        sl[axis] = i
        m[tuple(sl)] = True
    if shape[axis] >= 5:
        mid = [0, 0, 0]
        mid[axis] = shape[axis] // 2
        m[tuple(mid)] = True
    return m


def empty(shape):
    return np.zeros(shape, dtype=bool)


def full(shape):
    return np.ones(shape, dtype=bool)


def corner(shape, i):
    """A single voxel in corner i (bit 2, 1, 0 of i: the high end of x, y, z)."""
    m = np.zeros(shape, dtype=bool)
    m[tuple((s - 1) if (i >> (2 - a)) & 1 else 0 for a, s in enumerate(shape))] = True
    return m


def expected_count(kind, shape, connectivity):
    """The component counts the issue states for the structured generators (None: not stated)."""
    V = int(np.prod(shape))
    long_axes = sum(s > 1 for s in shape)
    if kind == "checker":
        return (V + 1) // 2 if connectivity == 6 or long_axes < 2 else 1
    if kind == "corner_lattice":
        return 1 if connectivity == 26 and long_axes == 3 else int(corner_lattice(shape).sum())
    if kind in ("snake", "comb", "full"):
        return 1
    if kind == "empty":
        return 0
    if kind == "twins":
        return 3 if max(shape) >= 5 else 2
    return None
