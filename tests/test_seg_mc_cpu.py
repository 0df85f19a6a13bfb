"""The host side of the softmax segmentation head (label maps of mutually exclusive classes), without a GPU:
  * the yardstick itself: tests/seg_mc_reference.py's closed-form loss and gradients equal torch's own autograd through log_softmax and the Dice formula in
    float64 to 1e-12 -- float64 round-off of two evaluation orders, not a kernel tolerance;
  * the entry points of csrc/seg_head_mc.hip are declared in include/pcrl_hip.h and exported, and the host-only workspace helper refuses K outside 2..16;
  * the refusals of the wrappers and of Segmenter3d, and the unchanged defaults of the sigmoid head."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from seg_mc_reference import autograd_reference, lowest_argmax, reference  # noqa: E402

MC_SYMBOLS = ("pcrl_seg_mc_head_ws_bytes", "pcrl_seg_mc_head_fwd", "pcrl_seg_mc_head_bwd", "pcrl_seg_mc_head_eval", "pcrl_seg_mc_head_logits",
              "pcrl_seg_labelmap_to_bits", "pcrl_seg_labelmap_keep")


def _case(K, M, seed, kind="mixed30"):
    g = torch.Generator().manual_seed(seed)
    a = torch.relu(torch.randn(M, 64, generator=g))
    w = 0.2 * torch.randn(K, 64, generator=g)
    b = torch.randn(K, generator=g)
    lab = torch.randint(0, K, (M,), generator=g).to(torch.uint8)
    if kind == "mixed30":
        lab = lab | ((torch.rand(M, generator=g) < 0.3).to(torch.uint8) << 7)
    if kind == "all_off":
        lab = lab | 0x80
    if kind == "background":
        lab = torch.zeros(M, dtype=torch.uint8)
    return a, w, b, lab


@pytest.mark.parametrize("K", [2, 3, 8, 9, 16])
def test_reference_equals_autograd_through_log_softmax(K):
    for kind in ("mixed", "mixed30", "background", "all_off"):
        for wc, wd, dloss in ((1.0, 1.0, 1.0), (0.3, 1.7, 0.75), (1.0, 0.0, 1.0), (0.0, 1.0, -2.0)):
            a, w, b, lab = _case(K, 257, seed=100 * K + len(kind), kind=kind)
            ref, ag = reference(a, w, b, lab, dloss, wc, wd), autograd_reference(a, w, b, lab, dloss, wc, wd)
            assert abs(float(ref["loss"] - ag["loss"])) <= 1e-12
            for name in ("dx", "dw", "db"):
                assert float((ref[name] - ag[name]).abs().max()) <= 1e-12, (name, kind, wc, wd)
            if kind == "all_off":
                assert float(ref["loss"]) == 0.0 and not bool(ref["dx"].abs().any())


def test_reference_treats_a_label_outside_the_classes_as_not_counted_and_takes_the_lowest_argmax():
    a, w, b, lab = _case(3, 40, seed=1, kind="mixed")
    bad, off = lab.clone(), lab.clone()
    bad[::4], off[::4] = 5, off[::4] | 0x80
    r0, r1 = reference(a, w, b, off, S=40), reference(a, w, b, bad, S=40)
    assert torch.equal(r0["sums"], r1["sums"]) and torch.equal(r0["dx"], r1["dx"]) and torch.equal(r0["counts"], r1["counts"])
    z = torch.tensor([[1.0, 3.0, 3.0], [2.0, 2.0, 2.0], [0.0, -1.0, 5.0]], dtype=torch.float64)
    assert lowest_argmax(z).tolist() == [1, 0, 2]
    assert int(r0["counts"][0, :, 2].sum()) == r0["Mc"] == int(r0["counts"][0, :, 1].sum())      # every counted voxel has one class and one prediction


def test_symbols_are_declared_and_exported():
    from pcrlv2_amd import _lib
    if not os.path.exists(_lib.LIBPATH):
        import __graft_entry__ as g
        g.build()
    protos = _lib.parse_header()
    cdll = ctypes.CDLL(_lib.LIBPATH)
    for name in MC_SYMBOLS:
        assert name in protos, f"{name} is not declared in include/pcrl_hip.h"
        assert hasattr(cdll, name), f"{name} declared in include/pcrl_hip.h but not exported"
    L = _lib.lib()
    # the workspace helper is a pure host function: 0 for what the entry points refuse, the larger of the two partial layouts otherwise
    assert [L.call("pcrl_seg_mc_head_ws_bytes", 2, 4096, K) for K in (0, 1, 17)] == [0, 0, 0]
    nb = 2 * 128
    assert L.call("pcrl_seg_mc_head_ws_bytes", 2, 4096, 2) == nb * 72 * 8
    assert L.call("pcrl_seg_mc_head_ws_bytes", 2, 4096, 16) == nb * 16 * 65 * 4
    assert L.call("pcrl_seg_head_ws_bytes", 2, 4096, 8) == 0, "the sigmoid head keeps its 1..7"


def test_segmenter_head_option_and_its_refusals():
    from pcrlv2_amd.models import Segmenter3d
    m = Segmenter3d(3)
    assert m.head == "sigmoid" and m.n_class == 3 and m.wc == 1.0
    with pytest.raises(ValueError, match=r"n_class must be in 1\.\.7 \(one bit of the label byte per class"):
        Segmenter3d(8)
    with pytest.raises(ValueError, match="head must be 'sigmoid'"):
        Segmenter3d(3, head="softmx")
    for bad in (1, 17):
        with pytest.raises(ValueError, match=r"n_class must be in 2\.\.16 with the softmax head"):
            Segmenter3d(bad, head="softmax")
    s = Segmenter3d(16, in_channels=2, head="softmax", wc=0.5)
    assert s.head == "softmax" and s.wc == 0.5 and tuple(s.out_tr.final_conv.weight.shape) == (16, 64, 1, 1, 1)
    assert len(s.state_dict()) == 169 and set(s.state_dict()) == set(m.state_dict())


def test_wrappers_refuse_a_class_count_outside_2_to_16_before_the_device_is_touched():
    from pcrlv2_amd import ops
    a = torch.zeros((1, 64, 2, 2, 2)).permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)
    for K in (1, 17):
        with pytest.raises(ops.PcrlError, match="2..16 mutually exclusive classes"):
            ops.seg_mc_head_forward(a, torch.zeros(K, 64), torch.zeros(K), torch.zeros((1, 2, 2, 2), dtype=torch.uint8), torch.float32)
    with pytest.raises(ops.PcrlError, match="1..7 classes inside 0..127"):
        ops.seg_labelmap_to_bits(torch.zeros(4, dtype=torch.uint8), 1, 8)
    with pytest.raises(ops.PcrlError, match="label map on the GPU is expected"):
        ops.seg_labelmap_to_bits(torch.zeros(4, dtype=torch.uint8), 1, 7)


# ---- the command line, the data layer and the metrics ---------------------------------------------------------------------------------------
def _exit_message(fn, *a, **k):
    with pytest.raises(SystemExit) as e:
        fn(*a, **k)
    return str(e.value)


def _train_args(*extra):
    from pcrlv2_amd import seg3d
    ap_args = ["train", "--data", "synthetic", "--phase", "scratch", *extra]
    holder = {}
    orig = seg3d.train
    try:
        seg3d.train = lambda args: holder.setdefault("args", args)
        seg3d.main(ap_args)
    finally:
        seg3d.train = orig
    return holder["args"]


def test_head_and_class_count_refusals_of_train():
    from pcrlv2_amd import seg3d
    assert "--head soft: 'sigmoid'" in _exit_message(seg3d.check_train, _train_args("--head", "soft"))
    for n in ("1", "17"):
        assert f"--n_class {n}: 2..16 with --head softmax" in _exit_message(seg3d.check_train, _train_args("--head", "softmax", "--n_class", n))
    assert _exit_message(seg3d.check_train, _train_args("--n_class", "8")) == "--n_class 8: 1..7 (one bit of the label byte per class; bit 7 means 'not counted')"
    assert "--wc -1.0" in _exit_message(seg3d.check_train, _train_args("--head", "softmax", "--wc", "-1"))
    seg3d.check_train(_train_args("--head", "softmax", "--n_class", "4", "--val_overlap", "0.5", "--val_mirror", "x"))      # both heads slide and mirror
    seg3d.check_train(_train_args("--head", "softmax", "--n_class", "16"))
    seg3d.check_train(_train_args("--n_class", "7"))


def test_train_builds_its_model_with_the_parsed_head_and_ce_weight():
    """`seg3d.py train --head softmax --wc 0.5`: the model train_seg hands to the epoch loop carries that head and that weight (the loop itself and the
    data are replaced: no device is needed to construct the model)."""
    from pcrlv2_amd import train_seg as T
    args = _train_args("--head", "softmax", "--wc", "0.5", "--n_class", "4")
    orig = T._loop.run_epochs, T._data.loaders
    try:
        T._data.loaders = lambda *a, **k: {}
        T._loop.run_epochs = lambda args, loaders, task, distributed: (task.make_model(0), None, False)
        model = T._train_segmenter(args, False)
    finally:
        T._loop.run_epochs, T._data.loaders = orig
    assert (model.head, model.wc, model.wd, model.wb, model.n_class) == ("softmax", 0.5, 1.0, 1.0, 4)
    assert T._loop.run_epochs is orig[0] and T._data.loaders is orig[1]


def test_default_parser_values_are_unchanged():
    a = _train_args()
    assert (a.head, a.wc, a.n_class, a.in_channels, a.crop, a.b, a.val_overlap, a.val_mirror) == ("sigmoid", 1.0, 3, 1, "64,64,32", 8, 0.0, "none")


def test_label_map_case_with_a_value_outside_the_classes_is_refused_by_name(tmp_path):
    import numpy as np
    from pcrlv2_amd import data_seg as D
    D.write_synthetic(str(tmp_path), ["a", "b"], (16, 16, 8), 4, head="softmax")
    seg = np.load(tmp_path / "b_seg.npy")
    seg[3, 3, 3] = 0x80 | 2           # bit 7 above a valid class is fine
    np.save(tmp_path / "b_seg.npy", seg)
    assert D.open_case(str(tmp_path), "b", 4, 1, head="softmax").seg is not None
    seg[1, 2, 3] = 6
    np.save(tmp_path / "b_seg.npy", seg)
    msg = _exit_message(D.open_case, str(tmp_path), "b", 4, 1, head="softmax")
    assert "b_seg.npy: label value 6 but --n_class is 4" in msg
    assert D.open_case(str(tmp_path), "a", 4, 1, head="softmax").shape == (16, 16, 8)


def test_label_map_phantoms_are_disjoint_and_inside_the_classes():
    import numpy as np
    from pcrlv2_amd import data_seg as D
    for K in (2, 4, 16):
        c = D.synthetic_case(7, 3, (48, 36, 20), K, in_channels=2, head="softmax")
        seg = np.asarray(c.seg)
        assert seg.dtype == np.uint8 and int(seg.max()) <= K - 1 and c.img.shape == (2, 48, 36, 20)
        assert set(np.unique(seg).tolist()) == set(range(K)), "every class, the background included, is present (one value per voxel: disjoint by construction)"
        assert np.array_equal(np.asarray(D.synthetic_case(7, 3, (48, 36, 20), K, in_channels=2, head="softmax").seg), seg)
        assert len(c.foreground()) == int((seg != 0).sum())
    old = D.synthetic_case(7, 3, (24, 16, 8), 3)
    assert int(np.asarray(old.seg).max()) <= 7 and np.array_equal(np.asarray(old.seg), np.asarray(D.synthetic_case(7, 3, (24, 16, 8), 3, head="sigmoid").seg))


def test_dice_and_loss_of_a_pass_in_their_softmax_forms():
    from pcrlv2_amd.train_seg import dice_from_counts, loss_from_sums
    counts = [[[90, 100, 95], [5, 10, 10], [0, 0, 0]], [[50, 50, 50], [0, 4, 0], [3, 3, 6]]]
    per, mean = dice_from_counts(counts, first=1)
    assert per == [(0.5 + 0.0) / 2, (1.0 + 6.0 / 9.0) / 2] and mean == sum(per) / 2
    per0, mean0 = dice_from_counts(counts)
    assert len(per0) == 3 and per0[1:] == per and mean0 == sum(per0) / 3
    K = 3
    sums = [4.0, 9.0, 5.0, 1.5, 2.0, 3.0, 4.0, 2.5, 1.0, 2.0, 1.0, 0.5, 10.0]
    want = 0.7 * (1.5 + 2.5 + 0.5) / 10.0 + 1.3 * (1.0 - 0.5 * ((2 * 2.0 + 1) / (3.0 + 4.0 + 1) + (2 * 1.0 + 1) / (2.0 + 1.0 + 1)))
    assert abs(loss_from_sums(sums, K, wd=1.3, head="softmax", wc=0.7) - want) < 1e-15
    assert loss_from_sums([0.0] * 13, K, head="softmax") == 0.0


def test_head_kind_of_a_checkpoint_and_mixed_head_ensembles():
    import types
    from pcrlv2_amd.train_seg import check_ensemble, checkpoint_head
    assert checkpoint_head({"state_dict": {}}) == "sigmoid"
    assert checkpoint_head({"val": {"mean_dice": 0.5}, "opt": types.SimpleNamespace(lr=0.1)}) == "sigmoid"
    assert checkpoint_head({"val": {"mean_dice": 0.5, "head": "softmax"}}) == "softmax"
    assert checkpoint_head({"opt": types.SimpleNamespace(head="softmax")}) == "softmax"
    sd = {"out_tr.final_conv.weight": torch.zeros(4, 64, 1, 1, 1), "down_tr64.ops.0.conv1.weight": torch.zeros(32, 1, 3, 3, 3)}
    assert check_ensemble(["a.pt", "b.pt"], [sd, sd], ["softmax", "softmax"]) == (4, 1)
    msg = _exit_message(check_ensemble, ["a.pt", "b.pt"], [sd, sd], ["softmax", "sigmoid"])
    assert "b.pt was trained with --head sigmoid, a.pt with --head softmax" in msg


def test_classes_table_and_label_map_paint_table_and_their_refusals(tmp_path):
    import types
    import numpy as np
    from pcrlv2_amd import seg3d
    from pcrlv2_amd import seg_prep as SP
    cls = SP.parse_classes("1;2;3,4")
    tab = SP.class_table(cls)
    assert tab.dtype == np.uint8 and tab.shape == (256,)
    assert [int(tab[v]) for v in (0, 1, 2, 3, 4, 5, 255)] == [0, 1, 2, 3, 3, 0, 0], "set i -> class index i + 1, a value in no set -> background"
    assert "label value 2 is in set 1 and in set 3" in _exit_message(SP.parse_classes, "1,2;5;2")
    for bad in ("", "1;;2", "1;x", "256", ";".join(str(i) for i in range(16))):
        assert "--classes" in _exit_message(SP.parse_classes, bad)
    assert len(SP.parse_classes(";".join(str(i) for i in range(1, 16)))) == 15
    paint = SP.labelmap_paint_table(SP.parse_labelmap_paint("0,7,9,200"))
    assert [int(paint[i]) for i in (0, 1, 2, 3, 4, 0x80, 0x81)] == [0, 7, 9, 200, 0, 0, 0], "class index i -> v_i, nothing else"
    for bad in ("5", "1,2,999", ",".join(["1"] * 17), "a,b"):
        assert "with --labelmap 2..16" in _exit_message(SP.parse_labelmap_paint, bad)
    assert [int(SP.paint_table(SP.parse_paint("2,1,4"))[m]) for m in (0, 1, 2, 3, 4)] == [0, 2, 1, 1, 4], "the bitmask builder is unchanged"
    # --classes together with --regions, and neither
    raw = tmp_path / "raw"
    raw.mkdir()
    base = ["prepare", "--data", str(raw), "--manifest", str(raw / "m.tsv"), "--save", str(tmp_path / "out")]
    ap = seg3d.build_parser()
    assert "exactly one of --regions" in _exit_message(SP.check_prepare, ap.parse_args(base + ["--regions", "1;2", "--classes", "1;2"]))
    assert "exactly one of --regions" in _exit_message(SP.check_prepare, ap.parse_args(base))
    assert "label value 1 is in set 1 and in set 2" in _exit_message(SP.check_prepare, ap.parse_args(base + ["--classes", "1;1"]))
    assert ap.parse_args(["restore", "--prep", "a", "--pred", "b", "--list", "c", "--out", "d"]).labelmap is False


def test_score_and_postprocess_refuse_label_maps_without_the_option_and_values_outside_the_classes(tmp_path):
    import types
    import numpy as np
    from pcrlv2_amd import train_seg as T
    data, pred = tmp_path / "data", tmp_path / "pred"
    data.mkdir()
    pred.mkdir()
    seg = np.zeros((8, 8, 8), dtype=np.uint8)
    seg[2:4] = 3
    np.save(data / "c_seg.npy", seg)
    np.save(pred / "c_pred.npy", seg)
    (data / "l.txt").write_text("c\n")
    (pred / "l.txt").write_text("c\n")
    sc = lambda **k: types.SimpleNamespace(data=str(data), list="l.txt", pred=str(pred), n_class=4, spacing="1,1,1", csv="", gpu=0, **k)      # noqa: E731
    assert T.score_plan(sc(labelmap=True))[0] == 4
    assert "c_seg.npy: label value 3 but --n_class is 3 with --labelmap" in _exit_message(T.score_plan, types.SimpleNamespace(**{**vars(sc(labelmap=True)), "n_class": 3}))
    assert "--n_class 17: 2..16" in _exit_message(T.score_plan, types.SimpleNamespace(**{**vars(sc(labelmap=True)), "n_class": 17}))
    bad = seg.copy()
    bad[0, 0, 0] = 9
    np.save(pred / "c_pred.npy", bad)
    assert "c_pred.npy: label value 9 but --n_class is 4" in _exit_message(T.score_plan, sc(labelmap=True))
    np.save(pred / "c_pred.npy", seg)
    # what `predict` of a softmax model leaves next to its label maps makes the bitmask reading impossible
    T.score_plan(sc())                                   # no marker: bitmasks, as before
    T.write_head_kind(str(pred), "softmax")
    assert "pass --labelmap" in _exit_message(T.score_plan, sc())
    pp = types.SimpleNamespace(pred=str(pred), list="l.txt", out=str(tmp_path / "clean"), n_class=4, keep_largest="all", min_voxels=0, connectivity=6)
    assert "pass --labelmap" in _exit_message(T.postprocess_plan, pp)
    assert T.postprocess_plan(types.SimpleNamespace(**vars(pp), labelmap=True))[0] == 4
    T.write_head_kind(str(pred), "sigmoid")              # a sigmoid prediction into the same directory takes the marker away
    T.score_plan(sc())
