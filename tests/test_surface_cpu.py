"""Surface-distance metrics on the host: the numpy restatement against scipy, hand-computable cases, the crop, the finish and the command line (no GPU).

Bound for the spacing (0.7, 0.7, 2.5) against scipy.ndimage.distance_transform_edt.  Both sides square the same three products tx = fl(fl(sx dx)^2),
ty, tz of the same nearest surface voxel (scipy multiplies the index difference by the sampling and squares it, as the restatement does), and then
    restatement  sqrt(fl(tx + fl(ty + tz)))          scipy  sqrt(fl(fl(tx + ty) + tz))        (np.add.reduce over the axes in order)
Each sum carries two roundings on positive terms, so each lies within a factor (1 +- u)^2 of T = tx + ty + tz, u = 2^-53: the two sums differ by at
most 4 u T to first order; the square root halves a relative error (2 u) and each side adds one rounding of its own (u each): the two distances differ
by at most 4 u d < 4 ulp(d), because ulp(d) > u d.  Where two surface voxels are nearest within that rounding the two sides may pick different
ones; both picks are minima of their own sums, and min is monotone, so the bound holds for the minima as well.  Asserted: 4 ulp.  Measured: 1 ulp.
For (1, 1, 1) and (0.78125, 0.78125, 1.25) every product, square and sum is exact (the spacings have 1, 5 and 3 significant bits, the index
differences at most 6, so a square has at most 22 bits and a sum of three stays below 2^53 units of its last place): both sides round sqrt once
from the same number, and the distances are EQUAL.
"""
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import surface_reference as R  # noqa: E402
from pcrlv2_amd import train_seg as T  # noqa: E402

SHAPES = [(1, 1, 1), (9, 1, 20), (17, 12, 9), (5, 33, 7)]
SPACINGS = [(1.0, 1.0, 1.0), (0.78125, 0.78125, 1.25), (0.7, 0.7, 2.5)]


def _masks(shape, K, seed):
    pred, gt = R.blobs(shape, K, seed), R.sprinkle_not_counted(R.blobs(shape, K, seed + 1), seed + 2)
    return pred, gt


# ---- the restatement against scipy -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_surfaces_are_scipys_erosion_formula_byte_for_byte(shape):
    ndi = pytest.importorskip("scipy.ndimage")
    K = 3
    pred, gt = _masks(shape, K, 11)
    sp, sg, counts = R.surfaces(pred, gt, K)
    P, G = R.effective(pred, gt, K)
    cross = ndi.generate_binary_structure(3, 1)
    for m, s in ((P, sp), (G, sg)):
        want = np.zeros_like(m)
        for k in range(K):
            b = (m >> k & 1).astype(bool)
            want |= ((b & ~ndi.binary_erosion(b, cross)).astype(np.uint8) << k).astype(np.uint8)
        assert np.array_equal(s, want)
    assert not ((sp | sg) & 0x80).any() and not (P[(gt & 0x80) != 0]).any()
    for k in range(K):
        pk, gk = (P >> k & 1).astype(bool), (G >> k & 1).astype(bool)
        assert counts[k].tolist() == [int((pk & gk).sum()), int(pk.sum()), int(gk.sum())]


@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("shape", SHAPES)
def test_separable_d2_is_the_brute_force_minimum_bit_for_bit(shape, spacing):
    surf = (R.surfaces(*_masks(shape, 1, 5), 1)[1] & 1).astype(bool)
    if not surf.any():
        surf[0, 0, 0] = True
    sep, brute = R.edt_sq(surf, spacing), R.brute_d2(surf, spacing)
    assert np.array_equal(sep.view(np.int64), brute.view(np.int64))
    assert np.array_equal(R.edt_sq(np.zeros(shape, dtype=bool), spacing), np.full(shape, np.inf))


@pytest.mark.parametrize("spacing,ulps", list(zip(SPACINGS, (0, 0, 4))))
@pytest.mark.parametrize("shape", SHAPES)
def test_distances_against_scipys_transform(shape, spacing, ulps):
    ndi = pytest.importorskip("scipy.ndimage")
    surf = (R.surfaces(*_masks(shape, 1, 7), 1)[0] & 1).astype(bool)
    if not surf.any():
        surf[0, 0, 0] = True
    sparse = np.zeros(shape, dtype=bool)          # two voxels in opposite corners: long distances with all three terms in play
    sparse[0, 0, 0] = sparse[-1, -1, -1] = True
    for kind, s in (("blobs", surf), ("corners", sparse)):
        mine = np.sqrt(R.edt_sq(s, spacing))
        theirs = ndi.distance_transform_edt(~s, sampling=spacing)
        off = np.abs(mine - theirs) / np.spacing(np.maximum(mine, theirs))
        print(f"[edt vs scipy {shape} {spacing} {kind}] worst {off.max():.0f} ulp, {100.0 * (off > 0).mean():.3f} % of the voxels differ")
        assert off.max() <= ulps


# ---- hand-computable cases -------------------------------------------------------------------------------------------------------------
def test_one_voxel_against_one_voxel():
    pred, gt = np.zeros((6, 7, 8), np.uint8), np.zeros((6, 7, 8), np.uint8)
    pred[1, 2, 3], gt[4, 6, 3] = 1, 1
    m = R.metrics(pred, gt, 1, (2.0, 0.5, 3.0))
    d = math.sqrt(36.0 + 4.0)
    assert m["hd95"][0] == d and m["hd"][0] == d and m["assd"][0] == d and m["n_pred"][0] == 1 and m["n_gt"][0] == 1
    assert m["counts"].tolist() == [[0, 1, 1]]


def test_two_parallel_planes():
    pred, gt = np.zeros((10, 6, 5), np.uint8), np.zeros((10, 6, 5), np.uint8)
    pred[2], gt[7] = 1, 1            # one voxel thick: every voxel of a plane is on its surface
    m = R.metrics(pred, gt, 1, (1.5, 1.0, 1.0))
    assert m["hd95"][0] == 7.5 and m["hd"][0] == 7.5 and m["assd"][0] == 7.5 and m["n_pred"][0] == 30


def test_identical_masks_score_zero_and_empty_masks_follow_the_convention():
    K = 3
    pred = R.blobs((9, 8, 7), K, 3)
    m = R.metrics(pred, pred.copy(), K)
    assert all((m[k] == 0).all() for k in T.SURFACE_KEYS)
    gt = pred & 0x01                  # class 1 and 2: prediction only
    empty_both = R.metrics(pred & 0x01, gt, K)
    assert all((empty_both[k] == 0).all() for k in T.SURFACE_KEYS)
    one = R.metrics(pred, gt, K)
    assert one["hd95"][0] == 0 and all(np.isnan(one[k][1:]).all() for k in T.SURFACE_KEYS)
    assert one["n_gt"].tolist()[1:] == [0, 0] and min(one["n_pred"].tolist()) > 0


# ---- the host's finish -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [0.95, 0.5, 0.0, 1.0, 0.37])
@pytest.mark.parametrize("spacing", SPACINGS)
def test_finish_from_records_is_numpys_percentile_exactly(spacing, q):
    """surface_from_records sees only what the device record holds (three order statistics of d2, two sums, the counts) and must land on np.percentile
    of the distances bit for bit: sqrt is monotone, and _lerp repeats numpy's two formulas."""
    K = 3
    pred, gt = _masks((17, 12, 9), K, 21)
    gt[..., :] &= 0xFB | 0x80          # class 2: no ground truth -> NaN
    per, _ = R.class_stats(pred, gt, K, spacing, q)
    want = R.metrics_of(per, q)
    got = T.surface_from_records(np.stack([R.record_of(st) for st in per]), q)
    for key in T.SURFACE_KEYS:
        assert np.array_equal(got[key].view(np.int64), want[key].view(np.int64)), (key, got[key], want[key])
    assert np.isnan(got["hd95"][2]) and got["n_gt"][2] == 0 and got["n_pred"].tolist() == [st["n_a"] for st in per]


def test_single_distance_and_equal_ranks():
    st = {"n_a": 1, "n_b": 1, "lo": 0, "d2": (4.0, 9.0, 9.0), "sum_a": 3.0, "sum_b": 2.0}
    got = T.surface_from_records(R.record_of(st), 0.95)
    assert got["hd95"][0] == np.percentile([2.0, 3.0], 95) and got["hd"][0] == 3.0 and got["assd"][0] == 2.5


def test_the_bounding_box_crop_leaves_every_metric_unchanged():
    K = 3
    shape, inner = (20, 18, 15), (slice(4, 13), slice(6, 14), slice(2, 9))
    pred, gt = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    p, g = _masks((9, 8, 7), K, 31)
    pred[inner], gt[inner] = p, g
    gt[0, 0, 0] = 0x80                 # a voxel that is not counted does not widen the box
    cut = T.crop_to_masks(pred, gt)
    assert cut[0].shape == cut[1].shape and all(a <= b for a, b in zip(cut[0].shape, (9, 8, 7))) and cut[0].flags.c_contiguous
    full, boxed = R.metrics(pred, gt, K, (0.7, 0.7, 2.5)), R.metrics(cut[0], cut[1], K, (0.7, 0.7, 2.5))
    for key in full:
        assert np.array_equal(full[key], boxed[key], equal_nan=True), key
    assert T.crop_to_masks(np.zeros(shape, np.uint8), np.full(shape, 0x80, np.uint8)) is None


# ---- the C ABI and the command line ----------------------------------------------------------------------------------------------------
NEW = ("pcrl_surf_extract", "pcrl_edt_max_axis", "pcrl_edt_sq_ws_bytes", "pcrl_edt_sq", "pcrl_surf_dist_stats_ws_bytes", "pcrl_surf_dist_stats")


def test_header_declares_the_entry_points_and_the_library_resolves_them():
    from pcrlv2_amd import _lib
    if not os.path.exists(_lib.LIBPATH):
        import __graft_entry__ as g
        g.build()
    protos = _lib.parse_header()
    assert all(n in protos for n in NEW)
    L = _lib.lib()
    top = L.call("pcrl_edt_max_axis")
    assert top >= 1024
    assert L.call("pcrl_surf_dist_stats_ws_bytes", 1000) > 0 and L.call("pcrl_edt_sq_ws_bytes", 8, 8, 8) >= 0
    with pytest.raises(_lib.PcrlError, match=rf"at most {top} voxels"):        # refused before a launch
        L.call("pcrl_edt_sq", 16, 0, 16, 1.0, 1.0, 1.0, None, None, 0, 4, top + 1, 4, None)
    with pytest.raises(_lib.PcrlError, match="1 <= K <= 7"):
        L.call("pcrl_surf_extract", 16, 16, 16, 16, 16, 4, 4, 4, 8, None)
    with pytest.raises(_lib.PcrlError, match="three positive finite numbers"):
        L.call("pcrl_edt_sq", 16, 0, 16, 1.0, float("inf"), 1.0, None, None, 0, 4, 4, 4, None)
    with pytest.raises(_lib.PcrlError, match=r"outside \[0, 1\]"):
        L.call("pcrl_surf_dist_stats", 16, 16, 16, 16, 0, 1.5, 16, 16, 1 << 20, 64, None)


def test_ops_wrappers_refuse_host_tensors_and_bad_arguments():
    import torch
    from pcrlv2_amd import ops
    from pcrlv2_amd._lib import PcrlError
    m = torch.zeros((4, 4, 4), dtype=torch.uint8)
    for call in (lambda: ops.surf_extract(m, m, 3), lambda: ops.edt_sq(m, 0), lambda: ops.surf_dist_stats(m.double(), m, m.double(), m, 0)):
        with pytest.raises(PcrlError, match="on the GPU"):
            call()


def _cli(*argv):
    r = subprocess.run([sys.executable, "seg3d.py", *argv], cwd=ROOT, capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout + r.stderr


def _write_cases(d, with_pred=True, pred_shape=None):
    os.makedirs(d / "data"), os.makedirs(d / "pred")
    for i, name in enumerate(("a", "b")):
        pred, gt = _masks((9, 8, 7), 3, 40 + i)
        np.save(d / "data" / f"{name}_seg.npy", gt)
        if with_pred or i == 0:
            np.save(d / "pred" / f"{name}_pred.npy", pred if pred_shape is None or i == 0 else np.zeros(pred_shape, np.uint8))
    (d / "data" / "list.txt").write_text("a\nb\n")
    return ("score", "--data", str(d / "data"), "--list", "list.txt", "--pred", str(d / "pred"))


@pytest.mark.parametrize("extra,message", [
    (("--spacing", "1,1"), "--spacing 1,1: three positive finite numbers"),
    (("--spacing", "1,0,1"), "--spacing 1,0,1: three positive finite numbers"),
    (("--spacing", "1,inf,1"), "three positive finite numbers"),
    (("--spacing", "1,x,1"), "three positive finite numbers"),
    (("--n_class", "0"), "--n_class 0: 1..7"),
    (("--n_class", "8"), "--n_class 8: 1..7"),
])
def test_score_refuses_bad_flags_before_any_gpu_work(extra, message, tmp_path):
    code, out = _cli(*_write_cases(tmp_path), *extra, "--gpu", "99")
    assert code != 0 and message in out and "Traceback" not in out, out


def test_score_refuses_a_missing_and_a_mis_shaped_prediction(tmp_path):
    code, out = _cli(*_write_cases(tmp_path / "m", with_pred=False), "--gpu", "99")
    assert code != 0 and "b_pred.npy: missing" in out and "Traceback" not in out, out
    code, out = _cli(*_write_cases(tmp_path / "s", pred_shape=(9, 8, 6)), "--gpu", "99")
    assert code != 0 and "b_pred.npy: a prediction is a uint8 array of its label's shape (9, 8, 7), got uint8 (9, 8, 6)" in out and "Traceback" not in out, out


def test_score_plan_takes_a_cases_spacing_file_over_the_flag(tmp_path):
    argv = _write_cases(tmp_path)
    np.save(tmp_path / "data" / "b_spacing.npy", np.array([0.7, 0.7, 2.5]))
    args = types.SimpleNamespace(data=argv[2], list="list.txt", pred=argv[6], n_class=3, spacing="2,2,2")
    K, plan = T.score_plan(args)
    assert K == 3 and [(p[0], p[3]) for p in plan] == [("a", (2.0, 2.0, 2.0)), ("b", (0.7, 0.7, 2.5))]
    np.save(tmp_path / "data" / "a_spacing.npy", np.array([1.0, -1.0, 1.0]))
    with pytest.raises(SystemExit, match="a_spacing.npy: .* three positive finite numbers"):
        T.score_plan(args)


def test_score_writes_the_csv_layout_with_the_device_stubbed_by_the_restatement(tmp_path, monkeypatch):
    """The loop around surface_metrics -- crop, an all-empty case without a device, per-case lines, the means with their case counts, the CSV -- with
    surface_metrics replaced by the restatement (the device path itself: test_surface_gpu.py)."""
    argv = _write_cases(tmp_path)
    shape = (9, 8, 7)
    np.save(tmp_path / "data" / "c_seg.npy", np.zeros(shape, np.uint8)), np.save(tmp_path / "pred" / "c_pred.npy", np.zeros(shape, np.uint8))
    gt_b = np.load(tmp_path / "data" / "b_seg.npy")
    np.save(tmp_path / "data" / "b_seg.npy", gt_b & 0xFB)           # case b: class 2 has no ground truth
    (tmp_path / "data" / "list.txt").write_text("a\nb\nc\n")
    monkeypatch.setattr(T, "surface_metrics", lambda p, g, K, spacing=(1.0, 1.0, 1.0), q=0.95: R.metrics(p.numpy(), g.numpy(), K, spacing, q))
    monkeypatch.setattr(T._ops, "edt_max_axis", lambda: 1024)
    monkeypatch.setattr(T.torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(T.torch, "device", lambda *a: "cpu")
    lines = []
    csv = tmp_path / "s.csv"
    args = types.SimpleNamespace(data=argv[2], list="list.txt", pred=argv[6], n_class=3, spacing="1,1,1", csv=str(csv), gpu=0)
    rows = T.score(args, log=lines.append)
    text = csv.read_text().splitlines()
    assert text[0] == "case,class,dice,hd95,hd,assd,n_pred,n_gt" and len(text) == 1 + 9 and len(rows) == 9
    assert text[7:] == ["c,0,1.0,0.0,0.0,0.0,0,0", "c,1,1.0,0.0,0.0,0.0,0,0", "c,2,1.0,0.0,0.0,0.0,0,0"]
    b2 = text[6].split(",")
    assert b2[:2] == ["b", "2"] and b2[3:6] == ["nan", "nan", "nan"] and float(b2[2]) == 0.0 and b2[7] == "0"
    want = R.metrics(*T.crop_to_masks(np.load(tmp_path / "pred" / "a_pred.npy"), np.load(tmp_path / "data" / "a_seg.npy")), 3)
    a0 = text[1].split(",")
    assert [float(v) for v in a0[3:6]] == [want["hd95"][0], want["hd"][0], want["assd"][0]] and int(a0[6]) == want["n_pred"][0]
    assert len(lines) == 4 and lines[-1].startswith("Score: 3 cases") and "class 2: Dice" in lines[-1]
    tail = lines[-1].split("class 2:")[1]
    assert "HD95" in tail and "(2)" in tail and "(3)" in tail       # class 2: three Dice values, two distances (case b is left out)
