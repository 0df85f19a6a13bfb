"""LUNA16 pre-processing, host side (no GPU): the MetaImage reader, the float64 restatement against scipy (what skimage's resize runs) and
against ITK's resample rules, the draw rules, the skip / pad rules, K-independence and the files the loader reads."""
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import luna_prep_reference as R  # noqa: E402
from pcrlv2_amd import luna_prep as P  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "luna_prep_windows.npz")


# ---- MetaImage -------------------------------------------------------------------------------------------------------------------
def test_metaimage_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    vol = rng.integers(-3000, 3000, (7, 5, 11)).astype(np.int16)
    p = str(tmp_path / "a.b.c.mhd")
    P.write_metaimage(p, vol, (0.7, 0.8, 2.5), offset=(-1.5, 2.0, 3.0))
    got, spacing, hdr = P.read_metaimage(p)
    assert got.dtype == np.int16 and got.shape == (7, 5, 11)
    np.testing.assert_array_equal(got, vol)
    assert spacing == (0.7, 0.8, 2.5)
    assert hdr["Offset"] == [-1.5, 2.0, 3.0] and hdr["TransformMatrix"] == [1, 0, 0, 0, 1, 0, 0, 0, 1]


def test_metaimage_big_endian_and_relative_data_file(tmp_path):
    vol = np.arange(24, dtype=np.int16).reshape(2, 3, 4) - 7
    (tmp_path / "d").mkdir()
    vol.astype(">i2").tofile(str(tmp_path / "d" / "v.raw"))
    (tmp_path / "h.mhd").write_text("NDims = 3\nDimSize = 4 3 2\nElementSpacing = 1 1 1\nBinaryDataByteOrderMSB = True\n"
                                    "ElementType = MET_SHORT\nElementDataFile = d/v.raw\n")
    got, _, _ = P.read_metaimage(str(tmp_path / "h.mhd"))
    np.testing.assert_array_equal(got, vol)


@pytest.mark.parametrize("line,word", [("ElementType = MET_FLOAT", "MET_FLOAT"), ("CompressedData = True", "CompressedData"),
                                       ("ElementDataFile = LIST", "LIST"), ("NDims = 2", "NDims")])
def test_metaimage_rejects(tmp_path, line, word):
    base = {"NDims": "3", "DimSize": "2 2 2", "ElementSpacing": "1 1 1", "ElementType": "MET_SHORT", "CompressedData": "False"}
    k, v = [s.strip() for s in line.split("=")]
    base[k] = v
    text = "".join(f"{a} = {b}\n" for a, b in base.items() if a != "ElementDataFile")
    text += f"ElementDataFile = {base.get('ElementDataFile', 'x.raw')}\n"
    np.zeros(8, np.int16).tofile(str(tmp_path / "x.raw"))
    (tmp_path / "h.mhd").write_text(text)
    with pytest.raises(P.MetaImageError, match=word):
        P.read_metaimage(str(tmp_path / "h.mhd"))


def test_metaimage_short_data_file(tmp_path):
    vol = np.zeros((2, 2, 2), np.int16)
    p = str(tmp_path / "s.mhd")
    P.write_metaimage(p, vol, (1, 1, 1))
    np.zeros(5, np.int16).tofile(str(tmp_path / "s.raw"))
    with pytest.raises(P.MetaImageError, match="voxels"):
        P.read_metaimage(p)


# ---- ITK resample rules ------------------------------------------------------------------------------------------------------------
def test_resample_spacing_one_is_identity():
    v = np.random.default_rng(1).integers(-2000, 2000, (5, 6, 7)).astype(np.int16)
    np.testing.assert_array_equal(R.resample(v, (1.0, 1.0, 1.0)), v)


def test_resample_spacing_two_midpoints_and_truncation():
    v = np.array([[[0, 10, -7]]], dtype=np.int16)       # z = y = 1, x = 3 at spacing 2 -> 6 outputs along x (size 6 + 0.5 -> 6)
    out = R.resample(v, (2.0, 1.0, 1.0))
    assert out.shape == (1, 1, 6)
    # o = 0..5 -> ci = 0, .5, 1, 1.5, 2, 2.5: 0, 5, 10, 1.5 -> 1, -7, then 2.5 >= 3 - 0.5: outside -> 0
    np.testing.assert_array_equal(out[0, 0], [0, 5, 10, 1, -7, 0])
    v = np.array([[[-3, -4]]], dtype=np.int16)
    np.testing.assert_array_equal(R.resample(v, (2.0, 1.0, 1.0), (4, 1, 1))[0, 0], [-3, -3, -4, 0])   # -3.5 truncates to -3


def test_resample_boundary_and_clamp():
    v = np.full((1, 1, 4), 100, dtype=np.int16)
    out = R.resample(v, (0.7, 1.0, 1.0), (6, 1, 1))
    ci = np.arange(6) / 0.7
    np.testing.assert_array_equal(out[0, 0] != 0, ci < 3.5)
    assert R.resample_size((512, 512, 300), (0.7, 0.7, 1.25)) == (358, 358, 375)
    assert P.resample_size((512, 512, 121), (0.703125, 0.703125, 2.5)) == R.resample_size((512, 512, 121), (0.703125, 0.703125, 2.5))


# ---- resize restatement vs scipy -------------------------------------------------------------------------------------------------
def test_gaussian_weights_are_scipys():
    from scipy.ndimage._filters import _gaussian_kernel1d
    for s in (0.03125, 0.25, 0.375, 0.457, 0.5, 0.914, 1.7):
        r, c = P.gaussian_weights(s)
        ref = _gaussian_kernel1d(s, 0, int(4.0 * s + 0.5))
        np.testing.assert_array_equal(c, ref[r:])
        np.testing.assert_array_equal(R.gaussian_weights(s)[1], ref[r:])


def test_resize_restatement_matches_scipy_bitwise():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from make_luna_prep_fixtures import scipy_resize
    rng = np.random.default_rng(2)
    for _ in range(60):
        src = tuple(int(v) for v in rng.integers(1, 48, 3))
        out = tuple(int(v) for v in rng.integers(1, 40, 3))
        img = rng.random(src)
        a, b = R.resize(img, out), scipy_resize(img, out)
        assert a.shape == b.shape == out
        assert np.array_equal(a, b), (src, out, np.abs(a - b).max())


def test_fixture_is_scipys_output_of_every_size_class():
    z = np.load(FIXTURE)
    vol = R.normalise(z["vol"].transpose(2, 1, 0))
    seen = set()
    for i, (s, n, o) in enumerate(zip(z["start"], z["src"], z["out_shape"])):
        crop = vol[s[0]:s[0] + n[0], s[1]:s[1] + n[1], s[2]:s[2] + n[2]]
        out = crop if tuple(n) == (64, 64, 35) else R.resize(crop, tuple(o))
        assert hashlib.sha256(np.ascontiguousarray(out).tobytes()).digest() == z["sha256"][i].tobytes(), tuple(n)
        if z["score"][i] >= 0:
            assert R.depth_score(out) == z["score"][i]
        seen.add(tuple(int(v) for v in n))
    for r, c, d in R.COL_SIZE:
        assert (r, c, d + 3) in seen and (r - 32, c - 32, d + 3) in seen
    for loc in R.LOCAL_COL_SIZE:
        assert loc in seen
    assert (1, 1, 1) in seen
    assert os.path.getsize(FIXTURE) < 1 << 20


def test_window_record_matches_restatement():
    for src, out in (((112, 112, 67), (64, 64, 35)), ((96, 96, 99), (64, 64, 35)), ((32, 32, 35), (64, 64, 35)), ((17, 1, 32), (16, 16, 16))):
        rec, prm = P.window_record((1, 2, 3), src, out, 10, out[2], 20, 0)
        sig = R.resize_sigmas(src, out)
        for a in range(3):
            if sig is None or sig[a] <= 1e-15:
                assert rec[9 + a] == 0
            else:
                r, c = R.gaussian_weights(sig[a])
                assert rec[9 + a] == r
                np.testing.assert_array_equal(prm[a * 9:a * 9 + r + 1], c)
            assert prm[27 + a] == src[a] / out[a]


def test_depth_threshold_in_float32_and_float64_agree():
    """The reference sums d_img in float32 (exact: halves up to 2^17) and compares against a Python float; the exact integer score /
    2 against the float64 limit decides the same for every size class."""
    sizes = {(r - s, c - s, d) for r, c, d in R.COL_SIZE for s in (0, 32)}
    for r, c, d in sizes:
        lim = R.LUNG_MAX * c * d * r
        for sc in range(max(0, int(2 * lim) - 4), int(2 * lim) + 5):
            assert (sc / 2 > lim) == bool(np.float32(sc / 2) > lim) == bool(np.float32(sc) / np.float32(2) > np.float32(lim))


# ---- draws -----------------------------------------------------------------------------------------------------------------------
def test_draw_rules_over_many_seeds():
    for seed in range(150):
        sx = 221 + seed % 40 * 7
        shape = (sx, sx + seed % 13 * 5, 130 + seed % 17 * 11)
        d = P.draw_attempt(np.random.default_rng(seed), shape)
        ref = R.draw_attempt(np.random.default_rng(seed), shape, P.IOU_BLOCK, P.IOU_BLOCKS)
        assert d.kind == ref[0] == "ok"
        assert (d.box1, d.box2, d.size1, d.size2, d.locals) == ref[1:]
        assert R.cal_iou(d.box1, d.box2) > 0.3
        for b, s in ((d.box1, d.size1), (d.box2, d.size2)):
            assert s in {(r - q, c - q, dd) for r, c, dd in R.COL_SIZE for q in (0, 32)}
            assert 70 <= b[0] <= shape[0] - s[0] - 1 - 70 and 70 <= b[2] <= shape[1] - s[1] - 1 - 70
            assert 15 <= b[4] <= shape[2] - s[2] - 3 - 1 - 15
            if s[0] in (32, 80):          # shrunk by 32: only size_x is tested
                assert shape[0] - (s[0] + 32) - 1 - 70 <= 70
            if s[0] in (96, 112):
                assert shape[0] - s[0] - 1 - 70 > 70
        for start, n in d.locals:
            for a, q in enumerate((0, 2, 4)):
                lo = max(min(d.box1[q], d.box2[q]) - 3, 0)
                hi = min(max(d.box1[q + 1], d.box2[q + 1]) + 3, shape[a])
                assert lo <= start[a] < hi
                assert 1 <= n[a] and start[a] + n[a] <= shape[a]


def test_local_windows_truncate_at_the_volume_edge():
    shape = (221, 221, 130)      # boxes reach the last 71 voxels; the union + 3 and a 32-wide window cross the edge
    cut = 0
    for seed in range(400):
        d = P.draw_attempt(np.random.default_rng(seed), shape)
        for start, n in d.locals:
            cut += any(start[a] + n[a] == shape[a] for a in range(3)) and any(n[a] not in (8, 16, 32) for a in range(3))
    assert cut > 0


def test_padded_depth():
    assert P.padded_depth(98) == 98 and P.padded_depth(97) == 99 and P.padded_depth(40) == 99 and P.padded_depth(300) == 300
    assert R.padded_depth(60) == P.padded_depth(60)


def test_empty_start_range_skips_the_series():
    shape = (300, 300, P.padded_depth(80))        # z = 99: a 96-deep window has no start (the reference raises ValueError)
    with pytest.raises(P.SeriesSkipped, match="empty start range on axis z"):
        list(P.series_pairs(shape, "s", 0, 16, 4, lambda ds: (0, ds[0])))
    small = (150, 300, 200)                      # x too small for any size class
    d = P.draw_attempt(np.random.default_rng(0), small)
    assert d.kind == "empty" and d.axis == "x"
    assert R.draw_attempt(np.random.default_rng(0), small, P.IOU_BLOCK, P.IOU_BLOCKS) == ("empty", "x")


def test_attempt_cap_skips_the_series():
    with pytest.raises(P.SeriesSkipped, match="no accepted crop pair in 7 attempts"):
        list(P.series_pairs((260, 260, 200), "s", 0, 2, 3, lambda ds: (-1, None), max_attempts=7))


def _stub(ds):
    for i, d in enumerate(ds):
        if (d.box1[0] + d.box2[2] + d.box1[4]) % 3 == 0:
            return i, (d.box1, d.box2, tuple(d.locals))
    return -1, None


def test_output_does_not_depend_on_attempts_per_launch():
    shape = (240, 250, 160)
    runs = [list(P.series_pairs(shape, "1.3.6.1.4.1.14519", 5, 6, K, _stub)) for K in (1, 2, 5, 16, 64)]
    assert all(r == runs[0] for r in runs[1:]) and len(runs[0]) == 6
    assert list(P.series_pairs(shape, "other", 5, 6, 4, _stub)) != runs[0]
    assert list(P.series_pairs(shape, "1.3.6.1.4.1.14519", 6, 6, 4, _stub)) != runs[0]


def test_stable_hash_is_not_pythons_hash():
    assert P.stable_hash("abc") == int.from_bytes(hashlib.blake2b(b"abc", digest_size=8).digest(), "little")
    a = P.attempt_rng(1, P.stable_hash("n"), 2, 3).integers(0, 1 << 30, 4)
    b = R.attempt_rng(1, "n", 2, 3).integers(0, 1 << 30, 4)
    np.testing.assert_array_equal(a, b)


# ---- files -----------------------------------------------------------------------------------------------------------------------
def test_files_are_what_the_loader_reads(tmp_path):
    import torch
    from pcrlv2_amd.data import LunaCropPairs, luna_file_lists
    rng = np.random.default_rng(3)
    for fold in (0, 8):
        d = tmp_path / f"subset{fold}"
        d.mkdir()
        for k in range(2):
            P.save_pair(str(d), f"1.2.{fold}", k, rng.random((2, 64, 64, 32)), rng.random((6, 16, 16, 16)), float32=(fold == 8))
    names = sorted(os.listdir(tmp_path / "subset0"))
    assert names == ["1.2.0_global_0.npy", "1.2.0_global_1.npy", "1.2.0_local_0.npy", "1.2.0_local_1.npy"]
    g = np.load(tmp_path / "subset0" / "1.2.0_global_1.npy")
    loc = np.load(tmp_path / "subset0" / "1.2.0_local_1.npy")
    assert g.dtype == np.float64 and g.shape == (2, 64, 64, 32) and g.flags.c_contiguous
    assert loc.dtype == np.float64 and loc.shape == (6, 16, 16, 16) and loc.flags.c_contiguous
    assert np.load(tmp_path / "subset8" / "1.2.8_global_0.npy").dtype == np.float32
    tr, va = luna_file_lists(str(tmp_path), 1.0, list_file=str(tmp_path / "absent.txt"))
    assert len(tr) == 2 and len(va) == 2
    pair, lo = LunaCropPairs(tr)[1]
    assert pair.dtype == torch.float32 and tuple(pair.shape) == (2, 64, 64, 32) and tuple(lo.shape) == (6, 16, 16, 16)
    np.testing.assert_array_equal(pair.numpy(), g.astype(np.float32))


def test_cli_rejects_non_default_sizes(tmp_path):
    for flag in ("--input_rows", "--input_deps", "--crop_cols"):
        args = P.build_parser().parse_args(["--data", str(tmp_path), "--save", str(tmp_path / "o"), flag, "48"])
        with pytest.raises(SystemExit, match="hard-codes"):
            P.run(args)
    args = P.build_parser().parse_args(["--data", "d", "--save", "s"])
    assert args.scale == 16 and args.folds == "0,1,2,3,4,5,6,7,8,9" and args.attempts_per_launch == 16 and not args.float32
