"""csrc/seg_prep.hip, pcrlv2_amd/seg_prep.py and `seg3d.py prepare / restore` on the GPU.  float64 restatement: seg_prep_reference.py; its own
agreement with scipy is checked without a GPU in test_seg_prep_cpu.py.

Bound of the statistics on unit-normal data (u = 2^-53, n masked values, A = mean |x|, m and s the true mean and standard deviation).  A float64
sum of n terms accumulated in ANY order is off by at most gamma_{n-1} sum |x_i| with gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability,
(4.4)); the kernel's order (a strided run per thread, a shuffle tree, four wave partials, the block partials in block order) is one such order.
    mean   the device: |sum error| / n <= gamma_{n-1} A, and the division rounds once: + u |m|.  The reference sums with math.fsum (exact, rounded
           once) and divides: 2 u |m|.          bound_mean = 1.01 u (n A + 3 |m|)
    std    the device forms d = fl(x - mean), fl(d d): (1 + u)^3 per term; the sum: gamma_{n-1}; the division and the square root one rounding
           each, the root halving what is under it: relative (gamma_{n+2} + u) / 2 + u.  Its sum is about ITS mean, off by delta <= bound_mean: sum
           (x - m - delta)^2 = sum (x - m)^2 + n delta^2, relative delta^2 / (2 s^2) after the root.  The reference: three roundings per term, an exact
           sum, a division and a root: at most 3 u, and its own delta^2 term.
                                                bound_std = 1.01 s u ((n + 3) / 2 + 5) + bound_mean^2 / s
The 1.01 covers the second-order terms (n u < 1e-11 here).  On integer data |v| <= 64 whose mean is an integer every partial sum of both
passes is an exact float64 (integers below 2^14 n), so mean and std equal the restatement bit for bit.
"""
import math
import os
import sys

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import seg_prep_reference as R  # noqa: E402
from pcrlv2_amd import data_seg, nifti, seg3d, seg_prep as SP  # noqa: E402
from pcrlv2_amd._lib import PcrlError  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -53
GUARD = 64
REGION = SP.region_table(SP.parse_regions("1,2,4;1,4;4"))      # overlapping sets; 3 and 5 are in no set


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def source(shape, C, kind, seed, pad=None, holes=True):
    """-> (src [C, Z, Y, X] int16 / float32, lab uint8 [Z, Y, X]).  pad = (x, y, z): the data sits at this odd offset inside a larger zero volume.
    holes: a few voxels are 0 in every channel (outside the mask, inside the box) and a few in one channel only."""
    rng = np.random.default_rng(seed)
    X, Y, Z = shape
    if kind == "int16":
        a = rng.integers(-300, 1200, (C, Z, Y, X)).astype(np.int16)
        a[a == 0] = 7
    else:
        a = (rng.standard_normal((C, Z, Y, X)) * 2 + 0.5).astype(np.float32)
    if holes:
        hole = rng.random((Z, Y, X)) < 0.08
        a[:, hole] = 0
        a[0][rng.random((Z, Y, X)) < 0.05] = 0
        a[:, 0, 0, 0] = a[:, -1, -1, -1] = 5          # two opposite corners are inside the mask: its box is the whole extent
    lab = rng.integers(0, 6, (Z, Y, X)).astype(np.uint8)
    if pad is not None:
        px, py, pz = pad
        big = np.zeros((C, Z + pz + 2, Y + py + 1, X + px + 3), dtype=a.dtype)
        big[:, pz:pz + Z, py:py + Y, px:px + X] = a
        blab = rng.integers(0, 6, big.shape[1:]).astype(np.uint8)
        blab[pz:pz + Z, py:py + Y, px:px + X] = lab
        return big, blab
    return a, lab


def guarded(nbytes):
    buf = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    return buf, buf[GUARD:GUARD + nbytes]


def intact(buf, nbytes, whole=False):
    h = buf.cpu().numpy()
    edge = (h[:GUARD] == 0xA5).all() and (h[GUARD + nbytes:] == 0xA5).all()
    return edge and (not whole or (h == 0xA5).all())


def run_resample(src, lab, box, out_shape, stats, clip, use_mask, half, region=REGION, K=3):
    C = src.shape[0]
    OV = int(np.prod(out_shape))
    es = 2 if half else 4
    ibuf, iv = guarded(C * OV * es)
    lbuf, lv = guarded(OV)
    ti, tw = SP.resample_tables(box[3:], out_shape)
    img = iv.view(torch.float16 if half else torch.float32).view(C, *out_shape)
    SP.gpu_resample(up(src), up(lab) if lab is not None else None, box, out_shape, up(ti), up(tw), up(stats) if stats is not None else None,
                    up(clip) if clip is not None else None, up(region) if region is not None else None, K, use_mask, img, lv.view(*out_shape))
    torch.cuda.synchronize()
    assert intact(ibuf, C * OV * es) and intact(lbuf, OV), "a canary around an output was overwritten"
    return img.cpu().numpy(), lv.view(*out_shape).cpu().numpy()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- scan ---------------------------------------------------------------------------------------------------------------------------
def _scan(src):
    rec = SP.gpu_scan(up(src)).cpu().numpy()
    return tuple(int(v) for v in rec)


def test_scan_box_count_and_non_finite():
    X, Y, Z = 13, 6, 5
    zero = np.zeros((2, Z, Y, X), dtype=np.float32)
    assert _scan(zero) == R.scan(zero) == (0x7FFFFFFF, 0, 0x7FFFFFFF, 0, 0x7FFFFFFF, 0, 0, 0)
    for z in (0, Z - 1):
        for y in (0, Y - 1):
            for x in (0, X - 1):
                one = zero.copy()
                one[1, z, y, x] = -0.5
                assert _scan(one) == R.scan(one) == (x, x + 1, y, y + 1, z, z + 1, 1, 0)
    full = np.ones((3, Z, Y, X), dtype=np.int16)
    assert _scan(full) == R.scan(full) == (0, X, 0, Y, 0, Z, X * Y * Z, 0)
    for kind in ("int16", "float32"):
        src, _ = source((9, 11, 7), 3, kind, 1, pad=(1, 3, 5))
        assert _scan(src) == R.scan(src) and _scan(src)[:6] == (1, 10, 3, 14, 5, 12)
    bad, _ = source((300, 9, 7), 2, "float32", 2)      # more than one block
    bad[0, 1, 2, 3], bad[1, 4, 4, 250], bad[1, 0, 0, 0] = np.nan, np.inf, -np.inf
    assert _scan(bad) == R.scan(bad) and _scan(bad)[7] == 3
    neg0 = zero.copy()
    neg0[0, 2, 2, 2] = -0.0
    assert _scan(neg0)[6] == 0


# ---- stats --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,use_mask,C", [("int16", True, 3), ("float32", False, 1), ("float32", True, 4)])
def test_stats_exact_on_integer_data(kind, use_mask, C):
    rng = np.random.default_rng(7)
    X, Y, Z = 41, 9, 8      # 2952 voxels: twelve blocks, the last one partial
    a = rng.integers(-64, 65, (C, Z, Y, X))
    hole = rng.random((Z, Y, X)) < 0.1
    a[:, hole] = 0
    a[0][(a[0] == 0) & ~hole] = 1
    m = (a != 0).any(axis=0) if use_mask else np.ones((Z, Y, X), dtype=bool)
    for c in range(C):      # move single voxels by one until the masked sum is a multiple of n: the mean is an integer
        n = int(m.sum())
        idx = np.argwhere(m & (np.abs(a[c]) < 60) & (a[c] != 0) & (a[c] != -1) & (a[c] != 1))
        need = (-int(a[c][m].sum())) % n
        need = need if need <= n // 2 else need - n
        for k in range(abs(need)):
            z, y, x = idx[k]
            a[c, z, y, x] += 1 if need > 0 else -1
        assert int(a[c][m].sum()) % n == 0
    src = a.astype(np.int16 if kind == "int16" else np.float32)
    assert np.array_equal((src != 0).any(axis=0), (a != 0).any(axis=0))
    d = up(src)
    got = SP.gpu_stats(d, use_mask, SP.gpu_scan(d)).cpu().numpy()
    want = R.stats(src, use_mask)
    assert same_bits(got, want), (got, want)
    clip = np.array([[-10.0, 20.0]] * C)
    assert same_bits(SP.gpu_stats(d, use_mask, SP.gpu_scan(d), up(clip)).cpu().numpy()[:, :1], R.stats(src, use_mask, clip)[:, :1])


def test_stats_unit_normal_within_the_derived_bound():
    rng = np.random.default_rng(8)
    src = rng.standard_normal((3, 9, 21, 37)).astype(np.float32)
    src[:, rng.random((9, 21, 37)) < 0.1] = 0
    d = up(src)
    rec = SP.gpu_scan(d)
    first = SP.gpu_stats(d, True, rec)
    got = first.cpu().numpy()
    assert same_bits(got, SP.gpu_stats(d, True, rec).cpu().numpy())
    want = R.stats(src, True)
    worst = 0.0
    for c in range(3):
        x = R.masked_values(src, c, True).astype(np.float64)
        n, A, m, s = x.size, np.abs(x).mean(), abs(want[c, 0]), want[c, 1]
        b_mean = 1.01 * U * (n * A + 3 * m)
        b_std = 1.01 * s * U * ((n + 3) / 2 + 5) + b_mean ** 2 / s
        e_mean, e_std = abs(got[c, 0] - want[c, 0]), abs(got[c, 1] - want[c, 1])
        print(f"[seg prep stats] channel {c}: n = {n}, mean error {e_mean:.2e} / bound {b_mean:.2e}, std error {e_std:.2e} / bound {b_std:.2e}")
        assert e_mean <= b_mean and e_std <= b_std
        worst = max(worst, e_mean / b_mean, e_std / b_std)
    print(f"[seg prep stats] worst error / bound = {worst:.3g}")


# ---- select -------------------------------------------------------------------------------------------------------------------------
def _select_case(values, ranks):
    """The values as channel 1 of a 2-channel volume whose channel 0 is non-zero everywhere (the mask is everything) -> device order statistics."""
    v = np.asarray(values, dtype=np.float32)
    src = np.stack([np.ones_like(v), v]).reshape(2, 1, 1, -1)
    d = up(src)
    a = SP.gpu_select(d, 1, True, ranks).cpu().numpy()
    b = SP.gpu_select(d, 1, False, ranks).cpu().numpy()
    assert same_bits(a, b)
    return a


@pytest.mark.parametrize("name", ["n1", "n2", "n3", "n4097", "constant", "ties", "negatives", "zeros", "last_byte"])
def test_select_and_percentiles_bit_for_bit(name):
    rng = np.random.default_rng(9)
    values = {"n1": [2.5], "n2": [3.0, -1.0], "n3": [0.5, 0.25, 8.0], "n4097": rng.standard_normal(4097) * 100, "constant": [1.75] * 300,
              "ties": np.repeat([-2.0, 0.5, 0.5, 0.5, 3.0], 40), "negatives": -np.abs(rng.standard_normal(777)) - 1e-3,
              "zeros": rng.permutation(np.array([0.0] * 30 + [-0.0] * 30 + [-1e-30, 1e-30, -5.0, 5.0], dtype=np.float32)),
              # 257 keys (more than one block) that agree in their three leading bytes: only the last pass tells them apart, under one full prefix
              "last_byte": (np.uint32(0x42280000) + (np.arange(257, dtype=np.uint32) * np.uint32(37)) % np.uint32(256)).view(np.float32)}[name]
    v = np.asarray(values, dtype=np.float32)
    n = v.size
    for q_lo, q_hi in ((0.5, 99.5), (0.0, 100.0), (40.0, 60.0)):
        ranks = SP.percentile_ranks(n, q_lo)[:2] + SP.percentile_ranks(n, q_hi)[:2]
        got = _select_case(v, ranks)
        assert same_bits(got, R.order_statistics(v, ranks)), (name, ranks, got)
        for q, pair in ((q_lo, got[:2]), (q_hi, got[2:])):
            p = SP.percentile_from_values(n, q, pair[0], pair[1])
            assert np.float64(p).tobytes() == np.float64(R.percentile(v, q)).tobytes() == np.float64(np.percentile(v.astype(np.float64) + 0.0, q)).tobytes()
    assert same_bits(_select_case(v, (0, n - 1, 0, n - 1)), R.order_statistics(v, (0, n - 1, 0, n - 1)))


def test_select_respects_the_mask_and_int16():
    src, _ = source((37, 9, 8), 3, "int16", 10)
    d = up(src)
    for use_mask in (True, False):
        vals = R.masked_values(src, 2, use_mask)
        ranks = (0, vals.size // 3, vals.size // 2, vals.size - 1)
        assert same_bits(SP.gpu_select(d, 2, use_mask, ranks).cpu().numpy(), R.order_statistics(vals, ranks))


# ---- resample -----------------------------------------------------------------------------------------------------------------------
TX, TZ = 32, 32      # the kernel's output tile where the ratio is about 1 (asserted in the test); one output y per block
CASES = [   # id, source extent (x, y, z), output, C, source type, float16 output, norm, mask, padded (odd box offsets)
    ("9x11x7-none", (9, 11, 7), (13, 8, 7), 1, "float32", False, "none", False, False),
    ("12x10x6-zscore-mask", (12, 10, 6), (5, 23, 9), 3, "int16", False, "zscore", True, True),
    ("6x6x70-percentile", (6, 6, 70), (4, 9, 66), 4, "float32", True, "percentile", True, False),
    ("8x8x8-window", (8, 8, 8), (16, 16, 4), 3, "int16", True, "window", False, True),
    ("7x5x3-zscore", (7, 5, 3), (14, 10, 6), 4, "float32", False, "zscore", False, False),
    ("5x1x4-none-mask", (5, 1, 4), (9, 3, 2), 1, "int16", False, "none", True, True),
    ("24x22x12-percentile-mask", (24, 22, 12), (16, 16, 8), 4, "float32", False, "percentile", True, True),
    ("tile+1", (35, 3, 34), (TX + 1, 2, TZ + 1), 3, "float32", True, "zscore", True, True),
    ("tile+1-down", (70, 2, 69), (TX + 1, 3, TZ + 1), 1, "int16", False, "window", True, False),
    ("7x5x3-percentile-f16", (7, 5, 3), (14, 10, 6), 3, "float32", True, "percentile", False, True),
]


def _norm(src, norm, use_mask):
    """-> (stats, clip) float64 [C, 2] or None, from the restatement (the kernels that make them on the device have their own tests)."""
    C = src.shape[0]
    clip = stats = None
    if norm == "percentile":
        clip = np.array([[R.percentile(R.masked_values(src, c, use_mask), q) for q in (0.5, 99.5)] for c in range(C)])
    if norm == "window":
        clip, stats = np.array([[-100.0, 400.0]] * C), np.array([[50.0, 120.0]] * C)
    if norm in ("zscore", "percentile"):
        stats = R.stats(src, use_mask, clip)
    return stats, clip


@pytest.mark.parametrize("cid,shape,out,C,kind,half,norm,use_mask,padded", CASES, ids=[c[0] for c in CASES])
def test_resample_bits_against_the_restatement(cid, shape, out, C, kind, half, norm, use_mask, padded):
    assert SP.resample_tile(64, 64, 64, 64, True)[:2] == (TX, TZ)
    src, lab = source(shape, C, kind, 11, pad=(1, 3, 5) if padded else None)
    box = (1, 3, 5) + shape if padded else (0, 0, 0) + shape
    if use_mask:
        r = R.scan(src)
        assert (r[0], r[2], r[4], r[1] - r[0], r[3] - r[2], r[5] - r[4]) == box or not padded
        box = (r[0], r[2], r[4], r[1] - r[0], r[3] - r[2], r[5] - r[4])
        if box[3:] != shape:
            pytest.fail(f"the generated case's box {box} is not the planned one")
    stats, clip = _norm(src, norm, use_mask)
    img, got_lab = run_resample(src, lab, box, out, stats, clip, use_mask, half)
    want, want_lab = R.resample(src, lab, box, out, stats, clip, REGION, use_mask)
    want = want.astype(np.float16 if half else np.float32)
    bad = img.view(np.uint16 if half else np.uint32) != want.view(np.uint16 if half else np.uint32)
    assert not bad.any(), f"{int(bad.sum())} image values differ, first at {tuple(np.argwhere(bad)[0])}"
    assert np.array_equal(got_lab, want_lab)
    assert set(np.unique(want_lab)) <= {0, 0b001, 0b011, 0b111} and (want != 0).any()


def test_resample_unlabelled_case_and_two_runs():
    src, _ = source((12, 10, 6), 3, "float32", 12)
    a = run_resample(src, None, (0, 0, 0, 12, 10, 6), (5, 23, 9), None, None, True, False, region=None)
    b = run_resample(src, None, (0, 0, 0, 12, 10, 6), (5, 23, 9), None, None, True, False, region=None)
    assert not a[1].any() and same_bits(a[0], b[0])
    assert same_bits(a[0], R.resample(src, None, (0, 0, 0, 12, 10, 6), (5, 23, 9), None, None, None, True)[0].astype(np.float32))


@pytest.mark.parametrize("shape,out", [((8, 8, 8), (16, 16, 4)), ((7, 5, 3), (14, 10, 6))])
def test_resample_lattice_exact_in_any_order(shape, out):
    """Dyadic ratios, integer data, mean 0, std 1: every product and partial sum is exact, so scipy's own order gives the same bits."""
    rng = np.random.default_rng(13)
    X, Y, Z = shape
    src = rng.integers(-500, 500, (2, Z, Y, X)).astype(np.int16)
    lab = rng.integers(0, 6, (Z, Y, X)).astype(np.uint8)
    img, got_lab = run_resample(src, lab, (0, 0, 0) + shape, out, None, None, False, False)
    zoom = [o / i for i, o in zip(shape, out)]
    for c in range(2):
        want = ndi.zoom(src[c].transpose(2, 1, 0).astype(np.float64), zoom, order=1, mode="nearest", grid_mode=True)
        assert np.array_equal(want.astype(np.float32).astype(np.float64), want) and same_bits(img[c], want.astype(np.float32))
    assert np.array_equal(got_lab, REGION[ndi.zoom(lab.transpose(2, 1, 0), zoom, order=0, mode="nearest", grid_mode=True)])


def test_resample_refusals_leave_the_outputs_untouched():
    src, lab = source((9, 11, 7), 2, "float32", 14)
    d, dl = up(src), up(lab)
    out = (13, 8, 7)
    OV = 13 * 8 * 7
    ti, tw = (up(t) for t in SP.resample_tables((9, 11, 7), out))
    reg = up(REGION)
    ibuf, iv = guarded(2 * OV * 4)
    lbuf, lv = guarded(OV)
    img, labo = iv.view(torch.float32).view(2, *out), lv.view(*out)
    ok = dict(box=(0, 0, 0, 9, 11, 7), out=out, K=3, lab=dl, img=img, labo=labo, src=d)

    def call(**kw):
        a = dict(ok, **kw)
        SP.gpu_resample(a["src"], a["lab"], a["box"], a["out"], ti, tw, None, None, reg, a["K"], True, a["img"], a["labo"])

    for kw, word in [(dict(K=0), "K = 0"), (dict(K=8), "K = 8"), (dict(box=(1, 0, 0, 9, 11, 7)), "box"), (dict(box=(0, 0, 0, 9, 0, 7)), "box"),
                     (dict(out=(13, 0, 7)), "output"), (dict(img=d.view(-1)), "overlaps"), (dict(labo=dl.view(-1)), "overlaps"),
                     (dict(labo=iv[:OV].view(*out)), "overlaps")]:
        with pytest.raises(PcrlError, match=word):
            call(**kw)
    wide = torch.zeros((17, 7, 11, 9), dtype=torch.float32, device=DEV)
    with pytest.raises(PcrlError, match="C = 17"):
        call(src=wide)
    torch.cuda.synchronize()
    assert intact(ibuf, 2 * OV * 4, whole=True) and intact(lbuf, OV, whole=True)
    assert same_bits(d.cpu().numpy(), src) and np.array_equal(dl.cpu().numpy(), lab)
    call()
    torch.cuda.synchronize()
    assert intact(ibuf, 2 * OV * 4) and not intact(ibuf, 2 * OV * 4, whole=True)


# ---- restore ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prep,box,orig,paint", [
    ((13, 8, 7), (1, 3, 5, 9, 11, 7), (13, 15, 14), None), ((5, 23, 9), (0, 0, 0, 12, 10, 6), (12, 10, 6), [2, 1, 4]),
    ((9, 11, 7), (1, 3, 5, 9, 11, 7), (11, 17, 13), [7, 0, 9]), ((33, 2, 33), (3, 1, 1, 70, 2, 69), (75, 4, 70), [2, 1, 4])])
def test_restore_bytes_against_the_restatement(prep, box, orig, paint):
    rng = np.random.default_rng(15)
    pred = rng.integers(0, 8, prep).astype(np.uint8)
    meta = {"prep_shape": np.array(prep), "orig_shape": np.array(orig),
            "box": np.array([box[0], box[0] + box[3], box[1], box[1] + box[4], box[2], box[2] + box[5]])}
    mask, label = SP.restore_case(pred, meta, torch.device(DEV), paint)
    want, want_label = R.restore(pred, box, orig, SP.paint_table(paint) if paint else None)
    assert np.array_equal(mask, want) and mask.shape == orig
    assert (label is None) == (paint is None) and (paint is None or np.array_equal(label, want_label))
    outside = np.ones(orig, dtype=bool)
    outside[box[0]:box[0] + box[3], box[1]:box[1] + box[4], box[2]:box[2] + box[5]] = False
    assert not mask[outside].any()
    if prep == box[3:]:      # --spacing keep: the identity on the box
        assert np.array_equal(mask[~outside].reshape(prep), pred)
    with pytest.raises(SP.PrepError):
        SP.restore_case(pred[:-1], meta, torch.device(DEV))


# ---- prepare_case -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", ["zscore", "percentile", "window", "none"])
@pytest.mark.parametrize("crop_nonzero", [True, False])
def test_prepare_case_every_normalisation(norm, crop_nonzero):
    src, lab = source((24, 22, 12), 3, "float32", 16, pad=(1, 3, 5))
    cfg = SP.PrepConfig(regions=SP.parse_regions("1,2,4;1,4;4"), spacing=(1.5, 1.25, 1.0), crop_nonzero=crop_nonzero, norm=norm, window=(-1.0, 3.0), mean=0.5,
                        std=2.0, float16=(norm == "window"))
    res = SP.prepare_case(list(src), lab, (1.0, 0.9, 1.1), cfg, torch.device(DEV))
    Z, Y, X = src.shape[1:]
    box = (1, 3, 5, 24, 22, 12) if crop_nonzero else (0, 0, 0, X, Y, Z)
    out = tuple(R.n_out(n, si, so) for n, si, so in zip(box[3:], (1.0, 0.9, 1.1), cfg.spacing))
    clip = stats = None
    if norm == "percentile":
        clip = np.array([[R.percentile(R.masked_values(src, c, crop_nonzero), q) for q in (0.5, 99.5)] for c in range(3)])
        assert same_bits(res["meta"]["stats"][:, 2:4].copy(), clip)
    if norm == "window":
        clip, stats = np.array([[-1.0, 3.0]] * 3), np.array([[0.5, 2.0]] * 3)
    if norm in ("zscore", "percentile"):
        stats = res["meta"]["stats"][:, 0:2].copy()      # the device's own, pinned by the stats tests; here: within a few ulp of the restatement's
        assert np.allclose(stats, R.stats(src, crop_nonzero, clip), rtol=1e-12, atol=0)
    want, want_lab = R.resample(src, lab, box, out, stats, clip, REGION, crop_nonzero)
    dt = np.float16 if cfg.float16 else np.float32
    assert res["img"].shape == (3,) + out and same_bits(np.ascontiguousarray(res["img"]), want.astype(dt)) and np.array_equal(res["seg"], want_lab)
    assert np.array_equal(res["meta"]["box"], [box[0], box[0] + box[3], box[1], box[1] + box[4], box[2], box[2] + box[5]])
    assert np.allclose(res["spacing"] * np.array(out), np.array(box[3:]) * np.array([1.0, 0.9, 1.1]), rtol=1e-14)


def test_prepare_case_refuses_non_finite_and_skips_all_zero():
    cfg = SP.PrepConfig(regions=SP.parse_regions("1"))
    src, lab = source((9, 11, 7), 2, "float32", 17)
    bad = src.copy()
    bad[1, 3, 3, 3] = np.nan
    with pytest.raises(SP.PrepError, match="case42.*non-finite"):
        SP.prepare_case(list(bad), lab, (1, 1, 1), cfg, torch.device(DEV), name="case42")
    assert SP.prepare_case(list(np.zeros_like(src)), lab, (1, 1, 1), cfg, torch.device(DEV)) is None
    mixed = SP.prepare_case([src[0], np.ones((7, 11, 9), dtype=np.int16)], None, (1, 1, 1), cfg, torch.device(DEV))      # int16 next to float32: all float32
    assert mixed["img"].shape == (2, 9, 11, 7) and not mixed["seg"].any()
    with pytest.raises(SP.PrepError, match="shape"):
        SP.prepare_case([src[0], src[1][:-1]], None, (1, 1, 1), cfg, torch.device(DEV))


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def test_prepare_train_predict_restore_score_end_to_end(tmp_path, capsys, monkeypatch):
    for k in ("HIP_VISIBLE_DEVICES", "PCRL_LOADER_WORKERS"):          # launch() sets them: monkeypatch puts back what was there
        if k in os.environ:
            monkeypatch.setenv(k, os.environ[k])
        else:
            monkeypatch.delenv(k, raising=False)
    raw, truth = tmp_path / "raw", tmp_path / "truth"
    raw.mkdir()
    truth.mkdir()
    names = ["s0", "s1", "s2"]
    values = np.array([0, 2, 1, 4], dtype=np.uint8)      # BraTS's values: WT = {1, 2, 4}, TC = {1, 4}, ET = {4}
    lines = []
    for i, n in enumerate(names):
        case = data_seg.synthetic_case(3, i, (24, 22, 12), 3, in_channels=2)
        big = np.zeros((2, 28, 26, 14), dtype=np.float32)
        big[:, 3:27, 1:23, 1:13] = case.img
        seg = np.zeros((28, 26, 14), dtype=np.uint8)
        seg[3:27, 1:23, 1:13] = case.seg
        level = (seg & 1) + ((seg >> 1) & 1) + ((seg >> 2) & 1)      # nested ellipsoids: 0..3 classes deep
        level[(seg != 0) & (seg != 1) & (seg != 3) & (seg != 7)] = 1
        for c in range(2):
            nifti.write_nifti(str(raw / f"{n}_c{c}.nii.gz"), np.ascontiguousarray(big[c].transpose(2, 1, 0)), spacing=(1.0, 1.0, 1.0), big_endian=(i == 1))
        nifti.write_nifti(str(raw / f"{n}_seg.nii"), np.ascontiguousarray(values[level].transpose(2, 1, 0)), spacing=(1.0, 1.0, 1.0))
        np.save(truth / f"{n}_seg.npy", REGION[values[level]])
        lines.append(f"{n} {n}_seg.nii {n}_c0.nii.gz {n}_c1.nii.gz\n")
    (tmp_path / "cases.tsv").write_text("".join(reversed(lines)))
    (truth / "cases.txt").write_text("".join(n + "\n" for n in names))

    def prepare(save):
        return seg3d.main(["prepare", "--data", str(raw), "--manifest", str(tmp_path / "cases.tsv"), "--save", str(save), "--regions", "1,2,4;1,4;4",
                           "--spacing", "1,1,1", "--split", "0.34,0.33,0.33", "--seed", "1"])

    res = prepare(tmp_path / "prep")
    assert sorted(res["cases"]) == names and not res["skipped"]
    prepare(tmp_path / "prep2")
    files = sorted(os.listdir(tmp_path / "prep"))
    assert files == sorted(os.listdir(tmp_path / "prep2")) and len([f for f in files if f.endswith(".npy")]) == 9 and "cases.txt" in files
    for f in files:
        assert (tmp_path / "prep" / f).read_bytes() == (tmp_path / "prep2" / f).read_bytes(), f
    listed = sorted(sum(((tmp_path / "prep" / f).read_text().split() for f in ("train.txt", "val.txt", "test.txt")), []))
    assert listed == names
    for n in names:
        case = data_seg.open_case(str(tmp_path / "prep"), n, 3, 2)
        assert case.shape == (24, 22, 12) and np.array_equal(np.asarray(case.seg), np.load(truth / f"{n}_seg.npy")[3:27, 1:23, 1:13])
        with np.load(tmp_path / "prep" / f"{n}_prep.npz") as z:
            assert list(z["box"]) == [3, 27, 1, 23, 1, 13] and list(z["orig_shape"]) == [28, 26, 14] and z["header"].size == 348
    for f, n in (("train.txt", "s0"), ("val.txt", "s1"), ("test.txt", "s2")):      # one case each, whatever the hash drew
        (tmp_path / "prep" / f).write_text(n + "\n")
    out = tmp_path / "model"
    seg3d.main(["train", "--data", str(tmp_path / "prep"), "--phase", "scratch", "--crop", "16,16,8", "--b", "2", "--epochs", "1", "--steps_per_epoch", "2",
                "--n_class", "3", "--in_channels", "2", "--output", str(out)])
    weights = sorted(str(out / f) for f in os.listdir(out) if f.endswith(".pt"))
    assert weights
    seg3d.main(["predict", "--data", str(tmp_path / "prep"), "--list", "cases.txt", "--weights", weights[-1], "--out", str(tmp_path / "pred"), "--crop", "16,16,8",
                "--b", "2"])
    seg3d.main(["restore", "--prep", str(tmp_path / "prep"), "--pred", str(tmp_path / "pred"), "--list", "cases.txt", "--out", str(tmp_path / "orig"),
                "--paint", "2,1,4", "--nifti"])
    for n in names:
        m, p = np.load(tmp_path / "orig" / f"{n}_pred.npy"), np.load(tmp_path / "pred" / f"{n}_pred.npy")
        assert m.shape == (28, 26, 14) and np.array_equal(m[3:27, 1:23, 1:13], p) and int(m.sum()) == int(p.sum())
        assert np.array_equal(np.load(tmp_path / "orig" / f"{n}_label.npy"), SP.paint_table([2, 1, 4])[m])
        vol, sp, _ = nifti.read_nifti(str(tmp_path / "orig" / f"{n}_label.nii.gz"), raw_values=True)
        assert vol.dtype == np.uint8 and np.array_equal(vol.transpose(2, 1, 0), SP.paint_table([2, 1, 4])[m]) and sp == (1.0, 1.0, 1.0)
    capsys.readouterr()
    rows = seg3d.main(["score", "--data", str(truth), "--list", "cases.txt", "--pred", str(tmp_path / "orig"), "--n_class", "3"])
    assert len(rows) == 9 and "Score: 3 cases" in capsys.readouterr().out
