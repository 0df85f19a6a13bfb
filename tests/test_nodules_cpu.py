"""LUNA16 nodule classification, host side (no GPU): the two new ABI entry points and their argument checks, the candidates reader, the
world-to-voxel rule, the negative subsample, the --ratio split and the balanced sampler."""
import argparse
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import nodule_reference as R  # noqa: E402
from pcrlv2_amd import _lib  # noqa: E402
from pcrlv2_amd import data as D  # noqa: E402
from pcrlv2_amd import luna_nodules as N  # noqa: E402
from pcrlv2_amd.luna_prep import MetaImageError  # noqa: E402


# ---- ABI ----------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_and_exported():
    protos = _lib.parse_header()
    cdll = ctypes.CDLL(_lib.LIBPATH)
    for name in ("pcrl_prep_cubes", "pcrl_prep_hu_to_unit"):
        assert name in protos, f"{name} not declared in include/pcrl_hip.h"
        assert hasattr(cdll, name), f"{name} not exported"
    assert [n for _, n in protos["pcrl_prep_cubes"][1]] == ["vol", "X", "Y", "Z", "start", "M", "out", "out_kind", "CX", "CY", "CZ", "stream"]
    assert protos["pcrl_prep_cubes"][1][4] == ("const int32_t*", "start")
    assert protos["pcrl_prep_hu_to_unit"][1][2] == ("int64_t", "n")


@pytest.mark.parametrize("cube,M,word", [((12, 16, 16), 1, "12"), ((16, 16, 72), 1, "72"), ((16, 16, 16), -1, "M = -1"), ((0, 16, 16), 1, "cube")])
def test_prep_cubes_rejects_bad_arguments_before_any_launch(cube, M, word):
    """The shape checks come first and touch neither the device nor the pointers: non-null dummies, no GPU in this process."""
    L = _lib.lib()
    f = L.fn["pcrl_prep_cubes"][0]
    rc = f(64, 32, 32, 32, 64, M, 64, 0, cube[0], cube[1], cube[2], None)
    assert rc != 0 and word in L.last_error(), L.last_error()
    assert f(64, 32, 32, 32, 64, 1, 64, 2, 16, 16, 16, None) != 0 and "out_kind" in L.last_error()


def test_prep_cubes_m_zero_and_hu_to_unit_n_zero_are_no_ops():
    L = _lib.lib()
    assert L.fn["pcrl_prep_cubes"][0](None, 32, 32, 32, None, 0, None, 0, 16, 16, 16, None) == 0
    assert L.fn["pcrl_prep_hu_to_unit"][0](None, None, 0, None) == 0
    assert L.fn["pcrl_prep_hu_to_unit"][0](None, None, -1, None) != 0


# ---- candidates -----------------------------------------------------------------------------------------------------------------
CSV = ("seriesuid,coordX,coordY,coordZ,class\n"
       "1.2.3,-56.08,-67.85,-311.92,0\n"
       "1.2.3,53.21,-244.41,-245.17,1\n"
       "9.8.7,0.5,-0.5,10,0\n"
       "1.2.3,1e1,2.25,-3,0\n"
       "9.8.7,68.42,-74.48,-288.7,1\n")


def test_read_candidates(tmp_path):
    p = tmp_path / "c.csv"
    p.write_text(CSV)
    c = N.read_candidates(str(p))
    assert list(c) == ["1.2.3", "9.8.7"]
    world, label = c["1.2.3"][:2]
    assert world.dtype == np.float64 and world.shape == (3, 3) and label.dtype == np.uint8
    np.testing.assert_array_equal(world, [[-56.08, -67.85, -311.92], [53.21, -244.41, -245.17], [10.0, 2.25, -3.0]])
    np.testing.assert_array_equal(label, [0, 1, 0])
    np.testing.assert_array_equal(c["1.2.3"].index, [0, 1, 3])
    np.testing.assert_array_equal(c["9.8.7"].index, [2, 4])
    assert c["1.2.3"].text[2] == ("1e1", "2.25", "-3")            # echoed as written
    (tmp_path / "bad.csv").write_text("1.2.3,1,2,3,0\n")
    with pytest.raises(ValueError, match="header"):
        N.read_candidates(str(tmp_path / "bad.csv"))


def _hdr(matrix, offset=(0.0, 0.0, 0.0)):
    return {"TransformMatrix": [float(v) for v in matrix.split()], "Offset": list(offset)}


def test_world_to_start_identity_flipped_and_half_millimetres():
    cube = (64, 64, 32)
    ident, flip = _hdr("1 0 0 0 1 0 0 0 1", (-10.0, 20.0, -300.0)), _hdr("-1 0 0 0 -1 0 0 0 1", (150.0, 160.0, -300.0))
    w = np.array([[0.0, 30.0, -250.0], [-10.0, 20.0, -300.0]])
    np.testing.assert_array_equal(N.world_to_voxel(w, ident), [[10, 10, 50], [0, 0, 0]])
    np.testing.assert_array_equal(N.world_to_voxel(w, flip), [[150, 130, 50], [160, 140, 0]])
    np.testing.assert_array_equal(N.world_to_start(w, ident, cube), [[10 - 32, 10 - 32, 50 - 16], [-32, -32, -16]])
    assert N.world_to_start(w, ident, cube).dtype == np.int32
    # floor(v + 0.5): halves round UP on both sides of zero (round-half-even and truncation both differ somewhere here)
    zero = _hdr("1 0 0 0 1 0 0 0 1")
    halves = np.array([[0.5, -0.5, 1.5], [-1.5, 2.5, -2.5], [0.49999, -0.50001, -0.49999]])
    np.testing.assert_array_equal(N.world_to_voxel(halves, zero), [[1, 0, 2], [-1, 3, -2], [0, -1, 0]])
    neg = _hdr("-1 0 0 0 -1 0 0 0 1")
    np.testing.assert_array_equal(N.world_to_voxel(halves, neg), [[0, 1, 2], [2, -2, -2], [0, 1, 0]])
    for hdr in (ident, flip, zero, neg):
        d = np.diag(np.array(hdr["TransformMatrix"]).reshape(3, 3))
        np.testing.assert_array_equal(N.world_to_start(halves, hdr, (16, 8, 24)), R.world_to_start(halves, hdr["Offset"], d, (16, 8, 24)))


@pytest.mark.parametrize("matrix", ["0 1 0 1 0 0 0 0 1", "1 0 0 0 0.9 0.1 0 0 1", "1 0 0 0 1 0 0 0 2", "1 0 0 0 1 0"])
def test_world_to_start_rejects_a_matrix_that_is_no_signed_identity(matrix):
    with pytest.raises(MetaImageError, match="TransformMatrix"):
        N.world_to_start(np.zeros((1, 3)), _hdr(matrix))


def test_negative_subsample_is_a_function_of_the_series_and_the_seed():
    rng = np.random.default_rng(5)
    series = {f"1.2.{k}": (rng.random(40 + 7 * k) < 0.1).astype(np.uint8) for k in range(6)}
    first = {s: N.subsample(s, lab, 5, seed=1) for s, lab in series.items()}
    again = {s: N.subsample(s, series[s], 5, seed=1) for s in reversed(list(series))}          # another order of presentation
    for s, lab in series.items():
        keep = first[s]
        np.testing.assert_array_equal(keep, again[s])
        assert np.all(np.diff(keep) > 0)
        assert set(np.flatnonzero(lab)) <= set(keep.tolist())                                   # every positive
        assert int((lab[keep] == 0).sum()) == min(5, int((lab == 0).sum()))
        # the rule itself
        r = np.random.default_rng([1, N.stable_hash(s)])
        neg = np.flatnonzero(lab == 0)
        np.testing.assert_array_equal(keep[lab[keep] == 0], neg[np.sort(r.permutation(neg.size)[:5])])
        np.testing.assert_array_equal(N.subsample(s, lab, -1, seed=1), np.arange(lab.size))     # -1: all
    assert any(not np.array_equal(first[s], N.subsample(s, series[s], 5, seed=2)) for s in series)


# ---- split ----------------------------------------------------------------------------------------------------------------------
def test_ratio_split(tmp_path):
    lst = tmp_path / "luna_train.txt"
    names = [f"1.2.{k}" for k in range(10)]
    lst.write_text("".join(n + "\n" for n in names))
    assert D.luna_finetune_names(0.0, str(lst)) == set(names)
    assert D.luna_finetune_names(0.5, str(lst)) == set(names[5:])
    assert D.luna_finetune_names(0.8, str(lst)) == set(names[8:])
    with pytest.raises(SystemExit) as e:
        D.luna_finetune_names(1.0, str(lst))
    assert "--ratio" in str(e.value.code)
    missing = str(tmp_path / "nope.txt")
    assert D.luna_finetune_names(0.0, missing) is None
    with pytest.raises(SystemExit) as e:
        D.luna_finetune_names(0.8, missing)
    assert "nope.txt" in str(e.value.code) and "--ratio" in str(e.value.code)


def test_balanced_epochs():
    rng = np.random.default_rng(2)
    labels = (rng.random(400) < 0.07).astype(np.uint8)
    pos = set(np.flatnonzero(labels).tolist())
    e0, e1 = D.balanced_epoch(labels, seed=3, epoch=0), D.balanced_epoch(labels, seed=3, epoch=1)
    for e in (e0, e1):
        assert e.dtype == np.int64 and len(e) == 2 * len(pos) and len(set(e.tolist())) == len(e)      # positives once each, negatives unique
        assert set(e[labels[e] == 1].tolist()) == pos and int((labels[e] == 0).sum()) == len(pos)    # equal counts
    assert set(e0[labels[e0] == 0].tolist()) != set(e1[labels[e1] == 0].tolist())                  # another draw per epoch
    assert not np.array_equal(np.flatnonzero(labels[e0]), np.arange(len(pos)))                    # shuffled together, not positives first
    np.testing.assert_array_equal(e0, D.balanced_epoch(labels, seed=3, epoch=0))                  # seeded
    assert not np.array_equal(e0, D.balanced_epoch(labels, seed=4, epoch=0))
    # rank shards: disjoint, equal length, together the epoch cut to a multiple of the world size
    shares = [D.rank_share(e0, r, 3) for r in range(3)]
    assert len({len(s) for s in shares}) == 1 and sorted(np.concatenate(shares).tolist()) == sorted(e0[:len(e0) - len(e0) % 3].tolist())
    few = np.array([1, 1, 1, 0], dtype=np.uint8)                                                  # fewer negatives than positives: all of them
    assert sorted(D.balanced_epoch(few, 0, 0).tolist()) == [0, 1, 2, 3]


def test_candidate_entries_and_mmap_rows(tmp_path):
    import torch
    d = tmp_path / "subset3"
    d.mkdir()
    cubes = np.arange(3 * 8 * 8 * 8, dtype=np.int16).reshape(3, 8, 8, 8)
    np.save(str(d / "1.2.3_cand.npy"), cubes)
    np.savez(str(d / "1.2.3_cand_meta.npz"), world=np.zeros((3, 3)), label=np.array([0, 1, 0], np.uint8), index=np.arange(3))
    entries = D.candidate_entries(str(tmp_path), (2, 3))
    assert [(os.path.basename(p), r, lab) for p, r, lab in entries] == [("1.2.3_cand.npy", 0, 0), ("1.2.3_cand.npy", 1, 1), ("1.2.3_cand.npy", 2, 0)]
    assert D.candidate_entries(str(tmp_path), (3,), keep={"9.9"}) == []
    ds = D.CandidateCubes(entries)
    cube, label = ds[1]
    assert cube.dtype == torch.int16 and label.dtype == torch.int32 and int(label) == 1
    np.testing.assert_array_equal(cube.numpy(), cubes[1])
    table = torch.tensor([2, 0])
    ds = D.CandidateCubes(entries, 2, table)
    assert len(ds) == 2
    np.testing.assert_array_equal(ds[0][0].numpy(), cubes[2])
    table[0] = 1                                                                                  # the next epoch's table shows through
    np.testing.assert_array_equal(ds[0][0].numpy(), cubes[1])


# ---- command line ---------------------------------------------------------------------------------------------------------------
def test_main_py_still_refuses_3d_finetuning():
    from pcrlv2_amd import main as M
    for phase in ("finetune", "scratch"):
        with pytest.raises(SystemExit) as e:
            M.check_route(M.build_parser().parse_args(["--d", "3", "--phase", phase]))
        assert "--d 3" in str(e.value.code) and "not implemented" in str(e.value.code)


def test_train_finetune_needs_encoder_weights(tmp_path):
    with pytest.raises(SystemExit) as e:
        N.main(["train", "--data", "synthetic", "--phase", "finetune", "--output", str(tmp_path / "o")])
    assert "--phase finetune needs --encoder_weights" in str(e.value.code) and "--phase scratch" in str(e.value.code)
    assert not (tmp_path / "o").exists()


def test_parser_defaults():
    ap = N.build_parser()
    a = ap.parse_args(["extract", "--data", "d", "--candidates", "c", "--save", "s"])
    assert (a.cube, a.negatives, a.folds) == ([64, 64, 32], 64, "0,1,2,3,4,5,6,7,8,9")
    a = ap.parse_args(["train", "--data", "d"])
    assert (a.val_folds, a.test_folds, a.n, a.model, a.phase) == ("7", "8,9", "luna_nodules", "pcrlv2", "finetune")
    a = ap.parse_args(["predict", "--data", "d", "--candidates", "c", "--weights", "w", "--out", "o"])
    assert a.b == 256 and isinstance(a, argparse.Namespace)
    with pytest.raises(SystemExit):
        N.check_cube((64, 64, 12))
