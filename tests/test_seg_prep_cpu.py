"""seg3d.py prepare / restore without a GPU: the float64 restatement (seg_prep_reference.py) against scipy, the host arithmetic of
pcrlv2_amd/seg_prep.py against numpy and the restatement, the NIfTI reader / writer, every refused option, and the C ABI's argument checks."""
import argparse
import ctypes
import gzip
import os
import struct
import sys

import numpy as np
import pytest
import scipy.ndimage as ndi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import seg_prep_reference as R  # noqa: E402
from pcrlv2_amd import _lib, data_seg, nifti, seg3d, seg_prep as SP  # noqa: E402

PAIRS = [((9, 11, 7), (13, 8, 7)), ((12, 10, 6), (5, 23, 9)), ((6, 6, 70), (4, 9, 66)), ((8, 8, 8), (16, 16, 4)), ((7, 5, 3), (14, 10, 6)),
         ((5, 1, 4), (9, 3, 2))]
DYADIC = [((8, 8, 8), (16, 16, 4)), ((7, 5, 3), (14, 10, 6))]


def _volume(shape, seed):
    rng = np.random.default_rng(seed)
    X, Y, Z = shape
    return rng.standard_normal((1, Z, Y, X)), rng.integers(0, 6, (Z, Y, X)).astype(np.uint8)


# ---- the restatement against scipy ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,out", PAIRS, ids=[f"{a}->{b}" for a, b in PAIRS])
def test_restatement_matches_scipy_zoom(shape, out):
    src, lab = _volume(shape, 3)
    img, got_lab = R.resample(src, lab, (0, 0, 0) + shape, out, None, None, np.arange(256, dtype=np.uint8), False)
    zoom = [o / i for i, o in zip(shape, out)]
    x64 = src[0].transpose(2, 1, 0)
    want = ndi.zoom(x64, zoom, order=1, mode="nearest", grid_mode=True)
    want_lab = ndi.zoom(lab.transpose(2, 1, 0), zoom, order=0, mode="nearest", grid_mode=True)
    assert want.shape == tuple(out)
    assert np.array_equal(got_lab, want_lab)
    err = np.abs(img[0] - want).max()
    print(f"[seg prep] {shape} -> {out}: image |restatement - scipy| = {err:.2e}")
    assert err <= 1e-12
    if (shape, out) in DYADIC:      # dyadic weights on integer data: every product and sum is exact, so any order gives the same bits
        ints = np.round(src * 8)
        assert np.array_equal(R.resample(ints, None, (0, 0, 0) + shape, out, None, None, None, False)[0][0],
                              ndi.zoom(ints[0].transpose(2, 1, 0), zoom, order=1, mode="nearest", grid_mode=True))


def test_host_tables_equal_the_restatement_bit_for_bit():
    for n_in, n_o in [(9, 13), (12, 5), (70, 66), (8, 16), (1, 4), (5, 1), (33, 34), (300, 300)]:
        i0, i1, nn, w0, w1 = SP.axis_tables(n_in, n_o)
        r0, r1, rw0, rw1, rnn = R.axis(n_in, n_o)
        assert np.array_equal(i0, r0) and np.array_equal(i1, r1) and np.array_equal(nn, rnn)
        assert np.array_equal(w0.view(np.int64), rw0.view(np.int64)) and np.array_equal(w1.view(np.int64), rw1.view(np.int64))
        assert i0.min() >= 0 and i1.max() <= n_in - 1 and nn.min() >= 0 and nn.max() <= n_in - 1


def test_tables_clamp_at_one_input_sample():
    i0, i1, nn, w0, w1 = SP.axis_tables(1, 5)
    assert not i0.any() and not i1.any() and not nn.any() and np.array_equal(w0, np.ones(5)) and np.array_equal(w1, np.zeros(5))


def test_n_out_rounds_half_to_even_and_never_below_one():
    assert SP.n_out(5, 0.5, 1.0) == 2 and SP.n_out(7, 0.5, 1.0) == 4 and SP.n_out(3, 0.5, 1.0) == 2      # 2.5 -> 2, 3.5 -> 4, 1.5 -> 2
    assert SP.n_out(1, 0.1, 5.0) == 1 and SP.n_out(512, 0.7, 1.0) == 358 and SP.n_out(300, 1.5, 1.5) == 300
    for n, a, b in [(5, 0.5, 1.0), (240, 1.0, 1.0), (155, 1.0, 0.33), (1, 0.1, 5.0)]:
        assert SP.n_out(n, a, b) == R.n_out(n, a, b)


# ---- percentiles ----------------------------------------------------------------------------------------------------------------------
def _host_percentile(values, q):
    n = len(values)
    lo, hi, _ = SP.percentile_ranks(n, q)
    s = R.order_statistics(values, (lo, hi))
    return SP.percentile_from_values(n, q, s[0], s[1])


@pytest.mark.parametrize("name,values", [
    ("n1", [3.25]), ("n2", [-1.5, 2.75]), ("equal", [0.1] * 7), ("negatives", [-5.5, -0.3, -7.25, -1e-3, -2.0]),
    ("normal", list(np.random.default_rng(0).standard_normal(4097).astype(np.float32))), ("zeros", [0.0, -0.0, -0.0, 0.0, 1.0, -1.0])])
def test_percentile_formula_equals_numpy_on_float64(name, values):
    """Zeros count as +0.0 on the device (-0.0 shares +0.0's key), so numpy sees the values with -0.0 replaced by +0.0: where the data has no -0.0
    that is np.percentile(values.astype(float64), q) itself."""
    v = np.asarray(values, dtype=np.float32)
    for q in (0.0, 0.5, 25.0, 50.0, 99.5, 100.0, 37.3):
        want = np.percentile(v.astype(np.float64) + 0.0, q)
        got = _host_percentile(v, q)
        assert np.float64(got).tobytes() == np.float64(want).tobytes(), (name, q, got, want)
        assert np.float64(R.percentile(v, q)).tobytes() == np.float64(want).tobytes()
        assert got == np.percentile(v.astype(np.float64), q)


# ---- NIfTI ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("ext", [".nii", ".nii.gz"])
def test_nifti_round_trip_every_datatype(tmp_path, big, ext):
    rng = np.random.default_rng(1)
    for code, dt in nifti.DTYPES.items():
        vol = (rng.standard_normal((3, 4, 5)) * 50).astype(dt) if np.dtype(dt).kind == "f" else rng.integers(0, 100, (3, 4, 5)).astype(dt)
        p = str(tmp_path / f"v{code}{ext}")
        nifti.write_nifti(p, vol, spacing=(0.7, 0.8, 1.5), big_endian=big)
        raw, sp, hdr = nifti.read_nifti(p, raw_values=True)
        assert raw.dtype == np.dtype(dt) and np.array_equal(raw, vol) and len(hdr) == 348
        assert np.allclose(sp, (0.7, 0.8, 1.5), rtol=1e-6)
        assert struct.unpack(">i" if big else "<i", hdr[:4])[0] == 348
        dev, _, _ = nifti.read_nifti(p)
        assert dev.dtype == (np.int16 if code == 4 else np.float32) and np.array_equal(dev, vol.astype(dev.dtype))


def test_nifti_scaling_and_header_reuse(tmp_path):
    vol = np.arange(24, dtype=np.int16).reshape(2, 3, 4)
    p = str(tmp_path / "s.nii.gz")
    nifti.write_nifti(p, vol, spacing=(1, 2, 3), slope=0.5, inter=-1024.0)
    got, sp, hdr = nifti.read_nifti(p)
    assert got.dtype == np.float32 and np.array_equal(got, (vol.astype(np.float64) * 0.5 - 1024.0).astype(np.float32)) and sp == (1.0, 2.0, 3.0)
    q = str(tmp_path / "t.nii")
    nifti.write_nifti(q, np.ones((2, 3, 4), dtype=np.uint8), header=hdr)
    back, sp2, hdr2 = nifti.read_nifti(q, raw_values=True)
    assert back.dtype == np.uint8 and sp2 == sp and hdr2[120:344] == hdr[120:344] and not nifti.scaled(nifti.parse_header(hdr2))
    a, b = str(tmp_path / "a.nii.gz"), str(tmp_path / "b.nii.gz")
    nifti.write_nifti(a, vol)
    nifti.write_nifti(b, vol)
    assert open(a, "rb").read() == open(b, "rb").read()


def test_nifti_refusals_name_the_path(tmp_path):
    vol = np.zeros((2, 3, 4), dtype=np.int16)
    good = str(tmp_path / "g.nii")
    nifti.write_nifti(good, vol)
    raw = bytearray(open(good, "rb").read())

    def variant(name, edit, cut=None):
        b = bytearray(raw)
        edit(b)
        p = str(tmp_path / name)
        with open(p, "wb") as f:
            f.write(bytes(b[:cut]))
        return p

    cases = [(variant("trunc.nii", lambda b: None, cut=352 + 10), "truncated"), (variant("short.nii", lambda b: None, cut=100), "truncated"),
             (variant("dim4.nii", lambda b: struct.pack_into("<8h", b, 40, 4, 4, 3, 2, 2, 1, 1, 1), None), "dim"),
             (variant("dim2.nii", lambda b: struct.pack_into("<h", b, 40, 2), None), "dim"),
             (variant("dt.nii", lambda b: struct.pack_into("<h", b, 70, 128), None), "datatype"),
             (variant("n2.nii", lambda b: struct.pack_into("<i", b, 0, 540), None), "NIfTI-2"),
             (variant("pair.nii", lambda b: b.__setitem__(slice(344, 348), b"ni1\0"), None), "pair"),
             (variant("junk.nii", lambda b: struct.pack_into("<i", b, 0, 1234), None), "sizeof_hdr")]
    for p, word in cases:
        with pytest.raises(nifti.NiftiError) as e:
            nifti.read_nifti(p)
        assert p in str(e.value) and word in str(e.value), str(e.value)
    trailing = variant("ok4.nii", lambda b: struct.pack_into("<8h", b, 40, 4, 4, 3, 2, 1, 1, 1, 1), None)
    assert nifti.read_nifti(trailing)[0].shape == (2, 3, 4)
    gz = str(tmp_path / "cut.nii.gz")
    with open(gz, "wb") as f:
        f.write(gzip.compress(bytes(raw))[:20])
    with pytest.raises(nifti.NiftiError):
        nifti.read_nifti(gz)


# ---- options --------------------------------------------------------------------------------------------------------------------------
def test_regions_and_paint_tables():
    reg = SP.parse_regions("1,2,4;1,4;4")
    tab = SP.region_table(reg)
    assert [int(tab[v]) for v in (0, 1, 2, 3, 4)] == [0, 0b011, 0b001, 0, 0b111] and not tab[5:].any()
    for bad in ("", "1;;2", "1,x", "256", "-1", ";".join("1" * 8)):
        with pytest.raises(SystemExit):
            SP.parse_regions(bad)
    paint = SP.paint_table(SP.parse_paint("2,1,4"))
    assert [int(paint[m]) for m in (0, 1, 2, 3, 4, 5, 7, 0x80)] == [0, 2, 1, 1, 4, 4, 4, 0]
    for bad in ("", "1,2,3,4,5,6,7,8", "300", "a"):
        with pytest.raises(SystemExit):
            SP.parse_paint(bad)
    assert SP.parse_spacing("keep") is None and SP.parse_spacing("1,1,1.5") == (1.0, 1.0, 1.5)
    for bad in ("1,1", "0,1,1", "1,1,-2", "nan,1,1", "x"):
        with pytest.raises(SystemExit):
            SP.parse_spacing(bad)
    assert SP.parse_split("0.7,0.1,0.2") == (0.7, 0.1, 0.2)
    for bad in ("0.7,0.1", "0.7,0.1,0.1", "-0.1,0.6,0.5"):
        with pytest.raises(SystemExit):
            SP.parse_split(bad)


def _raw_dir(tmp_path, names=("a", "b")):
    raw = tmp_path / "raw"
    raw.mkdir()
    for n in names:
        np.save(raw / f"{n}_t1.npy", np.ones((4, 5, 6), dtype=np.float32))
        np.save(raw / f"{n}_seg.npy", np.ones((4, 5, 6), dtype=np.uint8))
    man = tmp_path / "cases.tsv"
    man.write_text("# comment\n" + "".join(f"{n} {n}_seg.npy {n}_t1.npy\n" for n in names[:-1]) + f"{names[-1]} - {names[-1]}_t1.npy\n")
    return str(raw), str(man)


def _prepare_args(tmp_path, *extra):
    raw, man = _raw_dir(tmp_path)
    return seg3d.build_parser().parse_args(["prepare", "--data", raw, "--manifest", man, "--save", str(tmp_path / "out"), "--regions", "1;2", *extra])


def test_prepare_accepts_and_refuses_before_any_gpu(tmp_path):
    cfg, manifest, split = SP.check_prepare(_prepare_args(tmp_path, "--norm", "percentile", "--percentiles", "1,99", "--split", "0.5,0.25,0.25", "--seed", "3"))
    assert cfg.norm == "percentile" and cfg.percentiles == (1.0, 99.0) and cfg.spacing is None and cfg.crop_nonzero and split == (0.5, 0.25, 0.25)
    assert [m[0] for m in manifest] == ["a", "b"] and manifest[1][1] is None and manifest[0][1].endswith("a_seg.npy")
    refused = [["--norm", "median"], ["--percentiles", "1,99"], ["--norm", "percentile", "--percentiles", "99,1"], ["--norm", "window"],
               ["--norm", "window", "--window", "-100,200", "--mean", "0"], ["--norm", "window", "--window", "5,1", "--mean", "0", "--std", "1"],
               ["--norm", "window", "--window", "0,1", "--mean", "0", "--std", "0"], ["--window", "0,1"], ["--mean", "1"], ["--std", "1"], ["--seed", "1"],
               ["--crop_nonzero", "2"], ["--spacing", "1,1"], ["--split", "1,1,1"], ["--regions", "1;;"]]
    for i, extra in enumerate(refused):
        sub = tmp_path / f"r{i}"
        sub.mkdir()
        with pytest.raises(SystemExit):
            SP.check_prepare(_prepare_args(sub, *extra))


def test_manifest_refusals(tmp_path):
    raw, man = _raw_dir(tmp_path)
    for i, text in enumerate(["a a_seg.npy\n", "a - a_t1.npy\na - a_t1.npy\n", "a - missing.npy\n", "a - a_t1.mhd\n", "", "a - a_t1.npy\nb - b_t1.npy b_t1.npy\n"]):
        p = tmp_path / f"m{i}.tsv"
        p.write_text(text)
        with pytest.raises(SystemExit):
            SP.parse_manifest(str(p), raw)
    with pytest.raises(SystemExit):
        SP.parse_manifest(str(tmp_path / "none.tsv"), raw)


def test_split_does_not_depend_on_the_manifest_order():
    names = [f"case{i:03d}" for i in range(200)]
    first = {n: SP.split_of(n, 5, (0.7, 0.1, 0.2)) for n in names}
    again = {n: SP.split_of(n, 5, (0.7, 0.1, 0.2)) for n in reversed(names[::3])}
    assert all(first[n] == s for n, s in again.items())
    counts = [sum(1 for s in first.values() if s == k) for k in ("train", "val", "test")]
    assert counts[0] > counts[2] > counts[1] > 0
    assert any(SP.split_of(n, 6, (0.7, 0.1, 0.2)) != first[n] for n in names)


def test_restore_refusals(tmp_path):
    prep, pred = tmp_path / "prep", tmp_path / "pred"
    prep.mkdir()
    pred.mkdir()
    (prep / "cases.txt").write_text("a\n")
    args = lambda *extra: seg3d.build_parser().parse_args(      # noqa: E731
        ["restore", "--prep", str(prep), "--pred", str(pred), "--list", "cases.txt", "--out", str(tmp_path / "o"), *extra])
    with pytest.raises(SystemExit, match="prep.npz"):
        SP.check_restore(args())
    np.savez(prep / "a_prep.npz", prep_shape=np.array([2, 3, 4]))
    with pytest.raises(SystemExit, match="missing"):
        SP.check_restore(args())
    np.save(pred / "a_pred.npy", np.zeros((2, 3, 5), dtype=np.uint8))
    with pytest.raises(SystemExit, match="prepared shape"):
        SP.check_restore(args())
    np.save(pred / "a_pred.npy", np.zeros((2, 3, 4), dtype=np.uint8))
    assert SP.check_restore(args("--paint", "2,1"))[0] == [2, 1]
    with pytest.raises(SystemExit):
        SP.check_restore(args("--paint", "999"))
    with pytest.raises(SystemExit, match="--out"):
        SP.check_restore(seg3d.build_parser().parse_args(["restore", "--prep", str(prep), "--pred", str(pred), "--list", "cases.txt", "--out", str(pred)]))


# ---- restatement properties -------------------------------------------------------------------------------------------------------------
def test_restore_of_prepare_is_the_identity_on_the_box_with_spacing_keep():
    rng = np.random.default_rng(4)
    X, Y, Z = 9, 7, 6
    src = np.zeros((2, Z, Y, X), dtype=np.float32)
    src[:, 1:5, 2:6, 3:8] = rng.standard_normal((2, 4, 4, 5)).astype(np.float32) + 3.0
    lab = rng.integers(0, 4, (Z, Y, X)).astype(np.uint8)
    x0, x1, y0, y1, z0, z1, n, bad = R.scan(src)
    assert (x0, x1, y0, y1, z0, z1, n, bad) == (3, 8, 2, 6, 1, 5, 80, 0)
    box = (x0, y0, z0, x1 - x0, y1 - y0, z1 - z0)
    region = SP.region_table(SP.parse_regions("1,2;2,3"))
    img, prep = R.resample(src, lab, box, box[3:], None, None, region, True)
    assert np.array_equal(img, src[:, z0:z1, y0:y1, x0:x1].transpose(0, 3, 2, 1).astype(np.float64))
    back, _ = R.restore(prep, box, (X, Y, Z))
    want = np.zeros((X, Y, Z), dtype=np.uint8)
    want[x0:x1, y0:y1, z0:z1] = region[lab.transpose(2, 1, 0)][x0:x1, y0:y1, z0:z1]
    assert np.array_equal(back, want)


def test_open_case_accepts_a_prepared_case(tmp_path):
    rng = np.random.default_rng(5)
    src = rng.standard_normal((2, 6, 8, 10)).astype(np.float32)
    lab = rng.integers(0, 5, (6, 8, 10)).astype(np.uint8)
    cfg = SP.PrepConfig(regions=SP.parse_regions("1,2,4;1,4;4"))
    img, seg = R.resample(src, lab, (0, 0, 0, 10, 8, 6), (8, 8, 8), R.stats(src, True), None, SP.region_table(cfg.regions), True)
    meta = {"orig_shape": np.array([10, 8, 6]), "prep_shape": np.array([8, 8, 8])}
    for dt in (np.float32, np.float16):
        SP.save_case(str(tmp_path), "c", {"img": img.astype(dt), "seg": seg, "spacing": np.array([1.25, 1.0, 0.75]), "meta": meta}, None)
        case = data_seg.open_case(str(tmp_path), "c", 3, 2)
        assert case.shape == (8, 8, 8) and case.img.dtype == dt and case.seg.dtype == np.uint8
    assert np.load(tmp_path / "c_spacing.npy").dtype == np.float64
    with np.load(tmp_path / "c_prep.npz") as z:
        assert set(z.files) == {"header", "orig_shape", "prep_shape"} and z["header"].size == 0
    with pytest.raises(SystemExit):
        data_seg.open_case(str(tmp_path), "c", 2, 2)      # bit 2 is set: three regions need --n_class 3


def test_load_volume_npy_takes_the_spacing_next_to_it(tmp_path):
    a = np.arange(24, dtype=np.int16).reshape(2, 3, 4)
    np.save(tmp_path / "v.npy", a)
    vol, sp, hdr = SP.load_volume(str(tmp_path / "v.npy"))
    assert vol.shape == (4, 3, 2) and vol[3, 2, 1] == a[1, 2, 3] and sp == (1.0, 1.0, 1.0) and hdr is None
    np.save(tmp_path / "v_spacing.npy", np.array([0.5, 0.6, 2.0]))
    assert SP.load_volume(str(tmp_path / "v.npy"))[1] == (0.5, 0.6, 2.0)
    with pytest.raises(SP.PrepError):
        SP.as_labels(np.array([[[300]]], dtype=np.int16), "x")
    with pytest.raises(SP.PrepError):
        SP.as_labels(np.array([[[1.5]]]), "x")
    np.save(tmp_path / "w.npy", np.zeros((2, 3, 5), dtype=np.int16))
    with pytest.raises(SP.PrepError, match="case7"):
        SP.read_case(("case7", None, [str(tmp_path / "v.npy"), str(tmp_path / "w.npy")]))


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------------
SYMBOLS = ("pcrl_segprep_scan", "pcrl_segprep_stats", "pcrl_segprep_stats_ws_bytes", "pcrl_segprep_select", "pcrl_segprep_select_ws_bytes",
           "pcrl_segprep_resample", "pcrl_segprep_resample_tile", "pcrl_segprep_restore")


def test_symbols_declared_and_exported():
    protos = _lib.parse_header()
    cdll = ctypes.CDLL(_lib.LIBPATH)
    for name in SYMBOLS:
        assert name in protos, f"{name} not declared in include/pcrl_hip.h"
        assert hasattr(cdll, name), f"{name} not exported"
    assert [n for _, n in protos["pcrl_segprep_scan"][1]] == ["src", "src_kind", "C", "X", "Y", "Z", "rec", "stream"]
    assert protos["pcrl_segprep_resample"][1][13] == ("const int32_t*", "tab_i") and protos["pcrl_segprep_resample"][1][14] == ("const double*", "tab_w")
    assert protos["pcrl_segprep_select"][1][8] == ("int64_t", "r0")


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """The checks touch neither the device nor the pointers: non-null dummies, no GPU in this process."""
    L = _lib.lib()
    P = 1 << 20      # distinct dummy addresses, far apart
    scan, stats, select = (L.fn[n][0] for n in ("pcrl_segprep_scan", "pcrl_segprep_stats", "pcrl_segprep_select"))
    resample, restore = L.fn["pcrl_segprep_resample"][0], L.fn["pcrl_segprep_restore"][0]

    def refused(rc, word):
        assert rc != 0 and word in L.last_error(), L.last_error()

    refused(scan(P, 2, 1, 4, 4, 4, 2 * P, None), "src_kind")
    refused(scan(P, 0, 0, 4, 4, 4, 2 * P, None), "C = 0")
    refused(scan(P, 0, 17, 4, 4, 4, 2 * P, None), "C = 17")
    refused(scan(P, 0, 1, 0, 4, 4, 2 * P, None), "volume")
    refused(scan(P, 0, 1, 2048, 1024, 1024, 64 * P * P, None), "2^31")
    refused(scan(None, 0, 1, 4, 4, 4, 2 * P, None), "null")
    refused(scan(P, 1, 1, 4, 4, 4, P + 8, None), "overlap")
    refused(stats(P, 0, 1, 4, 4, 4, 1, None, None, 2 * P, 3 * P, 1 << 16, None), "null")
    refused(stats(P, 0, 1, 4, 4, 4, 0, None, None, 2 * P, 3 * P, 0, None), "workspace")
    refused(stats(P, 0, 1, 4, 4, -1, 0, None, None, 2 * P, 3 * P, 1 << 16, None), "volume")
    refused(select(P, 0, 2, 2, 4, 4, 4, 0, 0, 0, 0, 0, 2 * P, 3 * P, 1 << 16, None), "channel")
    refused(select(P, 0, 1, 0, 4, 4, 4, 0, 0, 0, 0, 64, 2 * P, 3 * P, 1 << 16, None), "rank")
    refused(select(P, 0, 1, 0, 4, 4, 4, 0, 0, 0, 0, 0, 2 * P, 3 * P, 8, None), "workspace")
    ok = dict(src=P, kind=0, lab=2 * P, C=1, X=8, Y=8, Z=8, b=(0, 0, 0), n=(8, 8, 8), ti=3 * P, tw=4 * P, st=None, cl=None, reg=5 * P, K=3, m=0, img=6 * P,
              half=0, out=7 * P, o=(4, 4, 4))

    def rs(**kw):
        a = dict(ok, **kw)
        return resample(a["src"], a["kind"], a["lab"], a["C"], a["X"], a["Y"], a["Z"], *a["b"], *a["n"], a["ti"], a["tw"], a["st"], a["cl"], a["reg"], a["K"],
                        a["m"], a["img"], a["half"], a["out"], *a["o"], None)

    refused(rs(K=0), "K = 0")
    refused(rs(K=8), "K = 8")
    refused(rs(C=17), "C = 17")
    refused(rs(o=(4, 0, 4)), "output")
    refused(rs(b=(1, 0, 0)), "box")
    refused(rs(n=(8, 0, 8)), "box")
    refused(rs(img=None), "null")
    refused(rs(reg=None), "null")
    refused(rs(img=P + 16), "overlaps")
    refused(rs(out=6 * P + 8), "overlaps")
    refused(rs(half=2), "out_half")
    refused(restore(P, 4, 4, 4, 2 * P, 0, 0, 0, 9, 4, 4, None, 3 * P, None, 8, 8, 8, None), "box")
    refused(restore(P, 4, 4, 4, 2 * P, 0, 0, 0, 4, 4, 4, None, 3 * P, 4 * P, 8, 8, 8, None), "null")
    refused(restore(P, 4, 4, 4, 2 * P, 0, 0, 0, 4, 4, 4, None, P + 8, None, 8, 8, 8, None), "overlap")
    refused(restore(P, 0, 4, 4, 2 * P, 0, 0, 0, 4, 4, 4, None, 3 * P, None, 8, 8, 8, None), "prepared grid")


def test_resample_tile_is_a_function_of_the_sizes():
    assert SP.resample_tile(64, 64, 64, 64, True)[:2] == (32, 32)
    tx, tz, nb = SP.resample_tile(4096, 4096, 32, 32, True)      # a 128-fold reduction: the tile shrinks until its source span fits
    assert tx < 32 and tz < 32 and 0 < nb <= 40 * 1024
    assert SP.resample_tile(5, 4, 9, 2, False)[2] <= 40 * 1024
