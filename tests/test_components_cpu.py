"""Connected-component clean-up on the host: the generators' component counts under scipy, filter_ref on hand-computable cases, the host functions of
the C ABI, the argument checks of the ops wrappers and every refusal of the command line (no GPU).  The kernels: test_components_gpu.py."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import components_reference as R  # noqa: E402
from pcrlv2_amd import train_seg as T  # noqa: E402

SHAPES = [(1, 1, 1), (1, 1, 9), (4, 4, 64), (5, 3, 65), (9, 10, 7), (1, 6, 5)]
CONNS = (6, 18, 26)


# ---- the generators ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", CONNS)
@pytest.mark.parametrize("kind,shape", [(k, s) for k in ("checker", "corner_lattice", "snake", "comb", "full", "empty", "twins") for s in SHAPES
                                        if k != "twins" or max(s) >= 3])      # twins needs an axis of at least 3 voxels
def test_generators_have_the_stated_component_counts(kind, shape, conn):
    m = getattr(R, kind)(shape)
    labels, sizes, n = R.label_ref(m.astype(np.uint8), 0, conn)
    assert n == R.expected_count(kind, shape, conn) and sizes.sum() == m.sum() and len(sizes) == n
    if kind == "twins":
        assert sizes[0] == sizes[n - 1] == sizes.max()
    if kind == "snake":          # a path: two ends, every other voxel has exactly two face neighbours
        deg = sum(np.roll(np.pad(m, 1), s, a)[1:-1, 1:-1, 1:-1] for a in range(3) for s in (1, -1))[m]
        assert m.sum() == 1 or (sorted(deg.tolist())[:2] == [1, 1] and (deg <= 2).all())


def test_corners_are_single_voxels_and_scipy_numbers_by_first_index():
    shape = (3, 4, 5)
    both = np.zeros(shape, dtype=bool)
    for i in range(8):
        c = R.corner(shape, i)
        assert c.sum() == 1
        both |= c
    labels, sizes, n = R.label_ref(both.astype(np.uint8), 0, 26)
    assert n == 8 and sizes.tolist() == [1] * 8
    first = [int(np.flatnonzero(labels.ravel() == c)[0]) for c in range(1, n + 1)]
    assert first == sorted(first)
    labels, _, n = R.label_ref(R.embed(R.noise((9, 10, 7), 0.3, 1), 3, 2), 3, 6)
    first = [int(np.flatnonzero(labels.ravel() == c)[0]) for c in range(1, n + 1)]
    assert first == sorted(first) and n > 5


# ---- filter_ref on hand-computable cases ------------------------------------------------------------------------------------------------
def _bars():
    """bit 1: bars of 3, 5, 5 and 2 voxels along z at x = 0, 2, 4, 6 (they do not touch at any connectivity); bits 0 and 4 carry something else."""
    m = np.zeros((8, 2, 7), np.uint8)
    m[0, 0, :3] = 2
    m[2, 0, :5] = 2
    m[4, 0, 2:7] = 2
    m[6, 0, 5:] = 2
    m[0, 0, 1:] |= 1
    m[3:5] |= 16
    return m


def test_filter_ref_tie_goes_to_the_lowest_label_and_other_bits_pass_through():
    far = _bars()
    labels, sizes, n = R.label_ref(far, 1, 26)
    assert n == 4 and sizes.tolist() == [3, 5, 5, 2]
    out = R.filter_ref(far, labels, sizes, 1, keep_largest=True)
    assert ((out >> 1 & 1) == (labels == 2)).all(), "of the two bars of 5 the one with the lower label stays"
    assert ((out & 0xFD) == (far & 0xFD)).all(), "bits 0 and 4 are copied"
    both = R.filter_ref(far, labels, sizes, 1, keep_largest=True, min_voxels=6)
    assert not (both >> 1 & 1).any() and ((both & 0xFD) == (far & 0xFD)).all()


def test_filter_ref_min_voxels_at_a_components_size_keeps_it_and_one_more_drops_it():
    far = _bars()
    labels, sizes, _ = R.label_ref(far, 1, 6)
    assert ((R.filter_ref(far, labels, sizes, 1, min_voxels=3) >> 1 & 1) == np.isin(labels, (1, 2, 3))).all()
    assert ((R.filter_ref(far, labels, sizes, 1, min_voxels=4) >> 1 & 1) == np.isin(labels, (2, 3))).all()
    assert ((R.filter_ref(far, labels, sizes, 1, min_voxels=5) >> 1 & 1) == np.isin(labels, (2, 3))).all()
    assert not (R.filter_ref(far, labels, sizes, 1, min_voxels=6) >> 1 & 1).any()
    assert (R.filter_ref(far, labels, sizes, 1) == far).all()
    e = np.zeros((3, 3, 3), np.uint8)
    assert (R.filter_ref(e, *R.label_ref(e, 0, 6)[:2], 0, keep_largest=True, min_voxels=2) == e).all()


def test_kept_components_is_the_references_rule():
    rng = np.random.default_rng(5)
    for _ in range(20):
        sizes = rng.integers(1, 5, rng.integers(0, 9))
        labels = np.arange(1, len(sizes) + 1, dtype=np.int32).reshape(1, 1, -1)
        mask = np.ones(labels.shape, np.uint8)
        for largest, mv in ((True, 0), (False, 3), (True, 3)):
            want = R.filter_ref(mask, labels, sizes, 0, largest, mv).ravel().astype(bool)
            assert T.kept_components(sizes, largest, mv).tolist() == want.tolist()


def test_postprocess_ref_treats_the_classes_independently():
    m = R.embed(R.noise((9, 10, 7), 0.3, 3), 0, 4) & 0x07
    a = R.postprocess_ref(m, 3, keep_largest=(0, 2), min_voxels=0, connectivity=6)
    assert ((a >> 1 & 1) == (m >> 1 & 1)).all() and R.label_ref(a, 0, 6)[2] == 1 and R.label_ref(a, 2, 6)[2] == 1
    b = R.postprocess_ref(m, 3, min_voxels=4, connectivity=26)
    for k in range(3):
        s = R.label_ref(b, k, 26)[1]
        assert (s >= 4).all() and sorted(s.tolist()) == sorted(v for v in R.label_ref(m, k, 26)[1].tolist() if v >= 4)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
NEW = ("pcrl_ccl_tile", "pcrl_ccl_ws_bytes", "pcrl_ccl_label", "pcrl_ccl_filter_ws_bytes", "pcrl_ccl_filter")


def test_header_declares_the_entry_points_and_the_host_queries_answer_without_a_gpu():
    from pcrlv2_amd import _lib, ops
    if not os.path.exists(_lib.LIBPATH):
        import __graft_entry__ as g
        g.build()
    protos = _lib.parse_header()
    assert all(n in protos for n in NEW)
    L = _lib.lib()
    tx, ty, tz = ops.ccl_tile()
    assert tx >= 1 and ty >= 1 and tz >= 1
    V = 33 * 34 * 35
    assert L.call("pcrl_ccl_ws_bytes", 33, 34, 35) >= 8 * V and L.call("pcrl_ccl_filter_ws_bytes") >= 4
    assert L.call("pcrl_ccl_ws_bytes", 2048, 1024, 1024) == 0 and L.call("pcrl_ccl_ws_bytes", 0, 4, 4) == 0
    assert L.call("pcrl_ccl_ws_bytes", 2047, 1024, 1024) > 0
    for thin in ((16384, 16384, 1), (1 << 26, 1, 1), (1, 1, 1 << 30), ((1 << 31) - 1, 1, 1)):      # thin volumes: 2^24 tiles and more, all accepted
        V = thin[0] * thin[1] * thin[2]
        assert L.call("pcrl_ccl_ws_bytes", *thin) == 8 * V + 8 * ((V + 1023) // 1024)
    big = 1 << 40
    with pytest.raises(_lib.PcrlError, match="2\\^31 voxels or more"):        # each refused before a launch
        L.call("pcrl_ccl_label", 16, 0, 6, 16, 16, 16, 16, big, 2048, 1024, 1024, None)
    with pytest.raises(_lib.PcrlError, match="connectivity 8 is not 6, 18 or 26"):
        L.call("pcrl_ccl_label", 16, 0, 8, 16, 16, 16, 16, big, 4, 4, 4, None)
    for bit in (-1, 7):
        with pytest.raises(_lib.PcrlError, match=f"bit {bit} outside 0..6"):
            L.call("pcrl_ccl_label", 16, bit, 6, 16, 16, 16, 16, big, 4, 4, 4, None)
        with pytest.raises(_lib.PcrlError, match=f"bit {bit} outside 0..6"):
            L.call("pcrl_ccl_filter", 16, 16, 16, 16, 32, bit, 1, 0, 16, big, 4, 4, 4, None)
    with pytest.raises(_lib.PcrlError, match="empty volume"):
        L.call("pcrl_ccl_label", 16, 0, 6, 16, 16, 16, 16, big, 4, 0, 4, None)
    with pytest.raises(_lib.PcrlError, match="workspace too small"):
        L.call("pcrl_ccl_label", 16, 0, 6, 16, 16, 16, 16, 8, 4, 4, 4, None)
    with pytest.raises(_lib.PcrlError, match="min_voxels -1 is negative"):
        L.call("pcrl_ccl_filter", 16, 16, 16, 16, 32, 0, 0, -1, 16, big, 4, 4, 4, None)
    with pytest.raises(_lib.PcrlError, match="must not be the input mask"):
        L.call("pcrl_ccl_filter", 16, 16, 16, 16, 16, 0, 1, 0, 16, big, 4, 4, 4, None)


def test_ops_wrappers_refuse_host_tensors_and_bad_arguments():
    import torch
    from pcrlv2_amd import ops
    from pcrlv2_amd._lib import PcrlError
    m = torch.zeros((4, 4, 4), dtype=torch.uint8)
    lab, sizes = torch.zeros((4, 4, 4), dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(PcrlError, match="on the GPU"):
        ops.label_components(m, 0)
    with pytest.raises(PcrlError, match="on the GPU"):
        ops.filter_components(m, lab, sizes, 0, keep_largest=True)
    for conn in (4, 8, 27, "6", None):
        with pytest.raises(PcrlError, match="is not 6, 18 or 26"):
            ops.label_components(m, 0, conn)
    for bit in (-1, 7):
        with pytest.raises(PcrlError, match=f"bit {bit} outside 0..6"):
            ops.label_components(m, bit)
        with pytest.raises(PcrlError, match=f"bit {bit} outside 0..6"):
            ops.filter_components(m, lab, sizes, bit)
    with pytest.raises(PcrlError, match="uint8 \\[X, Y, Z\\] bitmask"):
        ops.label_components(m.int(), 0)
    with pytest.raises(PcrlError, match="uint8 \\[X, Y, Z\\] bitmask"):
        ops.label_components(m[0], 0)


# ---- the command line ---------------------------------------------------------------------------------------------------------------------
def _cli(*argv):
    r = subprocess.run([sys.executable, "seg3d.py", *argv], cwd=ROOT, capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout + r.stderr


def _write_preds(d, second=None):
    os.makedirs(d / "pred")
    np.save(d / "pred" / "a_pred.npy", R.embed(R.blobs((9, 8, 7), 1), 0, 2) & 0x07)
    if second is not None:
        np.save(d / "pred" / "b_pred.npy", second)
    (d / "pred" / "list.txt").write_text("a\nb\n")
    return ("postprocess", "--pred", str(d / "pred"), "--list", "list.txt", "--out", str(d / "out"), "--gpu", "99")


OK_B = np.zeros((9, 8, 7), np.uint8)


@pytest.mark.parametrize("extra,message", [
    ((), "postprocess: no rule given: --keep_largest CLASSES|all and / or --min_voxels N"),
    (("--keep_largest", "0,3"), "--keep_largest 3: the masks have the classes 0..2 (--n_class 3)"),
    (("--keep_largest", "1", "--n_class", "1"), "--keep_largest 1: the masks have the classes 0..0 (--n_class 1)"),
    (("--keep_largest", "0,x"), "--keep_largest 0,x: class numbers separated by commas, or `all`"),
    (("--keep_largest", "-1"), "--keep_largest -1: class numbers separated by commas, or `all`"),
    (("--min_voxels", "-1"), "--min_voxels -1: the smallest volume of a component that stays, in voxels; 0 or more"),
    (("--min_voxels", "4", "--connectivity", "8"), "--connectivity 8: 6 (faces), 18 (faces and edges) or 26 (faces, edges and corners)"),
    (("--keep_largest", "all", "--connectivity", "0"), "--connectivity 0: 6 (faces)"),
    (("--keep_largest", "all", "--n_class", "8"), "--n_class 8: 1..7"),
])
def test_postprocess_refuses_bad_flags_before_any_gpu_work(extra, message, tmp_path):
    code, out = _cli(*_write_preds(tmp_path, OK_B), *extra)
    assert code != 0 and message in out and "Traceback" not in out, out


@pytest.mark.parametrize("second,message", [
    (None, "b_pred.npy: missing"),
    (np.zeros((9, 8, 7), np.int16), "b_pred.npy: a prediction is a non-empty uint8 array [X, Y, Z] of fewer than 2^31 voxels, got int16 (9, 8, 7)"),
    (np.zeros((9, 8), np.uint8), "b_pred.npy: a prediction is a non-empty uint8 array [X, Y, Z] of fewer than 2^31 voxels, got uint8 (9, 8)"),
    (np.zeros((2, 9, 8, 7), np.uint8), "got uint8 (2, 9, 8, 7)"),
])
def test_postprocess_refuses_a_missing_and_a_mis_typed_prediction(second, message, tmp_path):
    code, out = _cli(*_write_preds(tmp_path, second), "--keep_largest", "all")
    assert code != 0 and message in out and "Traceback" not in out, out


def test_postprocess_refuses_to_write_over_its_input(tmp_path):
    argv = list(_write_preds(tmp_path, OK_B))
    argv[argv.index("--out") + 1] = str(tmp_path / "pred" / ".." / "pred")
    code, out = _cli(*argv, "--min_voxels", "2")
    assert code != 0 and "the same directory as --pred" in out and "Traceback" not in out, out
    assert sorted(os.listdir(tmp_path / "pred")) == ["a_pred.npy", "b_pred.npy", "list.txt"]


def test_predict_refuses_bad_clean_up_flags_before_any_gpu_work(tmp_path):
    base = ("predict", "--data", str(tmp_path), "--list", "l.txt", "--weights", str(tmp_path / "none.pt"), "--out", str(tmp_path / "o"), "--gpu", "99")
    for extra, message in ((("--connectivity", "7", "--keep_largest", "all"), "--connectivity 7: 6 (faces)"), (("--min_voxels", "-3"), "--min_voxels -3:"),
                           (("--keep_largest", "a"), "--keep_largest a: class numbers")):
        code, out = _cli(*base, *extra)
        assert code != 0 and message in out and "Traceback" not in out, out


def test_plan_and_rules_on_the_host(tmp_path):
    argv = _write_preds(tmp_path, OK_B)
    args = types.SimpleNamespace(pred=argv[2], list="list.txt", out=argv[6], n_class=3, keep_largest="all", min_voxels=0, connectivity=18)
    K, rules, plan = T.postprocess_plan(args)
    assert K == 3 and rules == ((0, 1, 2), 0, 18) and [p[0] for p in plan] == ["a", "b"] and plan[0][2].endswith(os.path.join("out", "a_pred.npy"))
    assert T.parse_cleanup(types.SimpleNamespace()) is None, "predict without the options: no clean-up"
    assert T.parse_cleanup(types.SimpleNamespace(keep_largest="2,0,2", min_voxels=5)) == ((0, 2), 5, 6)
    assert T.parse_cleanup(types.SimpleNamespace(min_voxels=5, connectivity=26)) == ((), 5, 26)
