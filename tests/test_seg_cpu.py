"""Host side of 3D segmentation fine-tuning (pcrlv2_amd/data_seg.py, train_seg.py, seg3d.py): tiling, the crop sampler, the Dice metric and its
all-reduce, the command line's refusals.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pcrlv2_amd import data_seg as D  # noqa: E402
from pcrlv2_amd.train_seg import dice_from_counts, evaluate, higher_dice, loss_from_sums  # noqa: E402

CROP = (16, 8, 8)


def _case(shape, seed=0, K=3):
    return D.synthetic_case(seed, 0, shape, K)


# ---- tiling -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(32, 16, 8), (33, 17, 9), (16, 8, 8), (40, 5, 20), (10, 8, 9), (17, 24, 7), (1, 1, 1)])
def test_tiles_count_every_voxel_exactly_once(shape):
    case = _case(shape)
    hist = np.zeros(shape, dtype=np.int64)
    seen_img = np.zeros(shape, dtype=np.float32)
    for start, own in D.tiles(shape, CROP):
        assert all(0 <= s and (s + c <= n or s == 0) for s, c, n in zip(start, CROP, shape)), "a tile lies inside the volume (or the volume is shorter)"
        x, lab = D.cut_tile(case, start, own, CROP)
        assert x.shape == (1,) + CROP and lab.shape == CROP and lab.dtype == np.uint8
        counted = (lab & 0x80) == 0
        idx = np.nonzero(counted)
        g = tuple(i + s for i, s in zip(idx, start))
        assert all((gi < n).all() for gi, n in zip(g, shape)), "a counted voxel lies inside the volume"
        np.add.at(hist, g, 1)
        assert np.array_equal(lab[counted], case.seg[g]) and np.array_equal(x[0][counted], case.img[0][g])
        seen_img[g] = x[0][counted]
        # padding: outside the volume the image is 0 and the label exactly 0x80
        outside = np.ones(CROP, dtype=bool)
        outside[tuple(slice(0, max(min(n - s, c), 0)) for s, c, n in zip(start, CROP, shape))] = False
        assert (lab[outside] == 0x80).all() and (x[0][outside] == 0).all()
    assert hist.min() == 1 and hist.max() == 1, "every voxel of the case is counted exactly once"
    assert np.array_equal(seen_img, case.img[0])


def test_tile_loader_shards_cases_and_indexes_the_global_table():
    cases = [D.synthetic_case(1, i, (20, 9, 8), 2) for i in range(5)]
    whole = [int(c) for b in D.TileLoader(cases, CROP, 3) for c in b[2]]
    parts = [[int(c) for b in D.TileLoader(cases, CROP, 3, r, 2) for c in b[2]] for r in range(2)]
    assert whole == parts[0] + parts[1] and set(parts[0]).isdisjoint(parts[1]) and set(whole) == set(range(5))
    b0 = next(iter(D.TileLoader(cases, CROP, 3)))
    assert b0[0].shape == (3, 1) + CROP and b0[0].dtype == torch.float32 and b0[1].dtype == torch.uint8 and b0[2].dtype == torch.int32 and b0[3].shape == (3, 3)


# ---- crop sampler -----------------------------------------------------------------------------------------------------------------
def test_crops_flip_image_and_mask_together_contain_their_voxel_and_stay_inside():
    # the image encodes the mask: img = seg + 0.25 wherever it is inside the volume, so any flip applied to one and not the other shows
    shape = (37, 6, 19)                     # shorter than the crop on y: padded
    case = _case(shape)
    case.img = (case.seg.astype(np.float32) + 0.25)[None]
    rng = np.random.default_rng(3)
    flips_seen = set()
    for i in range(64):
        x, lab, info = D.draw_crop(rng, case, CROP, centred=i % 2 == 0)
        flips_seen.add(info["flips"])
        inside = lab != 0x80
        assert np.array_equal(x[0][inside], lab[inside].astype(np.float32) + 0.25) and (x[0][~inside] == 0).all()
        room = [max(n - c, 0) for n, c in zip(shape, CROP)]
        assert all(0 <= s <= r for s, r in zip(info["start"], room)), "the crop stays inside the padded volume"
        assert int(inside.sum()) == np.prod([min(c, n) for c, n in zip(CROP, shape)])
        # undo the flips: the crop is the box at `start`
        ux, ul = x, lab
        for axis, f in enumerate(info["flips"]):
            if f:
                ux, ul = np.flip(ux, axis + 1), np.flip(ul, axis)
        rx, rl = D.cut(case, info["start"], CROP)
        assert np.array_equal(ux, rx) and np.array_equal(ul, rl)
        if i % 2 == 0:
            v = info["voxel"]
            assert v is not None and case.seg[v] & 0x7F and all(s <= vi < s + c for vi, s, c in zip(v, info["start"], CROP)), "a centred crop contains its voxel"
        else:
            assert info["voxel"] is None
    assert len(flips_seen) == 8


def test_same_seed_same_crops_other_rank_other_crops():
    cases = [D.synthetic_case(2, i, (24, 12, 10), 3) for i in range(3)]
    take = lambda **k: [(x.clone(), l.clone()) for x, l in D.CropLoader(cases, CROP, 4, 3, **k)]      # noqa: E731
    a, b, c = take(seed=5, rank=0), take(seed=5, rank=0), take(seed=5, rank=1)
    assert len(a) == 3 and a[0][0].shape == (4, 1) + CROP and a[0][1].shape == (4,) + CROP and a[0][1].dtype == torch.uint8
    assert all(torch.equal(x1, x2) and torch.equal(l1, l2) for (x1, l1), (x2, l2) in zip(a, b))
    assert not all(torch.equal(x1, x2) for (x1, _), (x2, _) in zip(a, c))
    ld = D.CropLoader(cases, CROP, 4, 3, seed=5)
    ld.set_epoch(1)
    assert not torch.equal(next(iter(ld))[0], a[0][0])


def test_synthetic_phantoms_are_a_function_of_the_seed_and_overlap():
    a, b, c = D.synthetic_case(7, 1, (24, 20, 12), 3), D.synthetic_case(7, 1, (24, 20, 12), 3), D.synthetic_case(8, 1, (24, 20, 12), 3)
    assert np.array_equal(a.img, b.img) and np.array_equal(a.seg, b.seg) and not np.array_equal(a.img, c.img)
    assert a.seg.max() < 8 and all((a.seg >> k & 1).any() for k in range(3))
    assert ((a.seg & 1) & (a.seg >> 1 & 1)).any(), "the classes overlap"


# ---- Dice -------------------------------------------------------------------------------------------------------------------------
def test_dice_from_counts_hand_cases():
    per, mean = dice_from_counts([[[0, 0, 0], [0, 0, 5]], [[3, 4, 4], [2, 2, 2]]])
    assert per == [(1.0 + 0.75) / 2, (0.0 + 1.0) / 2] and mean == (0.875 + 0.5) / 2        # empty / empty scores 1; empty prediction, non-empty truth 0
    assert dice_from_counts(torch.tensor([[[0, 7, 0]]]))[1] == 0.0                          # a prediction against an empty truth
    assert dice_from_counts([])[1] != dice_from_counts([])[1]                               # no cases: NaN
    nan = float("nan")
    assert not higher_dice({"mean_dice": nan}, None) and not higher_dice({"mean_dice": nan}, {"mean_dice": 0.1})
    assert higher_dice({"mean_dice": 0.2}, None) and higher_dice({"mean_dice": 0.2}, {"mean_dice": 0.1}) and not higher_dice({"mean_dice": 0.1}, {"mean_dice": 0.1})
    assert loss_from_sums([0.0] * 9, 2) == 0.0                                              # nothing counted: no division by zero
    assert abs(loss_from_sums([2.0, 3.0, 4.0, 6.0, 5.0], 1, wb=2.0, wd=3.0) - (2.0 * 6.0 / 5.0 + 3.0 * (1.0 - 5.0 / 8.0))) < 1e-15


class _FakeSegmenter:
    """infer() on the host with Segmenter3d's interface: the prediction is `x > 1` per channel-0 threshold k."""
    n_class, wb, wd = 2, 1.0, 1.0

    def parameters(self):
        return iter([torch.zeros(1)])

    def infer(self, x, labels=None, case_index=None, counts=None, want_mask=False):
        K = self.n_class
        counted = (labels & 0x80) == 0
        sums = torch.zeros(4 * K + 1, dtype=torch.float64)
        for k in range(K):
            pred = (x[:, 0] > 1.0 + k) & counted
            gt = ((labels >> k) & 1).bool() & counted
            for n in range(x.shape[0]):
                counts[int(case_index[n]), k] += torch.tensor([int((pred[n] & gt[n]).sum()), int(pred[n].sum()), int(gt[n].sum())])
            sums[4 * k:4 * k + 4] = torch.tensor([float((pred & gt).sum()), float(pred.sum()), float(gt.sum()), float((pred ^ gt).sum())])
        sums[4 * K] = float(counted.sum())
        return counts, None, sums, None


def _cases():
    return [D.synthetic_case(4, i, (20 + i, 9, 8 + i), 2) for i in range(5)]


def _eval_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.save(evaluate(_FakeSegmenter(), D.TileLoader(_cases(), CROP, 3, rank, world)), os.path.join(out_dir, "r%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_sharded_counts_all_reduce_to_the_one_rank_table(tmp_path):
    import socket
    import torch.multiprocessing as mp
    one = evaluate(_FakeSegmenter(), D.TileLoader(_cases(), CROP, 3))
    assert one["cases"] == 5 and 0.0 < one["mean_dice"] < 1.0
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_eval_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        assert torch.load(str(tmp_path / ("r%d.pt" % r))) == one


# ---- command line -----------------------------------------------------------------------------------------------------------------
def _cli(*argv):
    r = subprocess.run([sys.executable, *argv], cwd=ROOT, capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout + r.stderr


@pytest.mark.parametrize("argv,message", [
    (("--data", "synthetic", "--phase", "finetune"), "--phase finetune needs --weights"),
    (("--data", "synthetic", "--phase", "scratch", "--crop", "64,60,32"), "multiples of 8"),
    (("--data", "synthetic", "--phase", "scratch", "--crop", "64,64"), "multiples of 8"),
    (("--data", "synthetic", "--phase", "scratch", "--n_class", "8"), "--n_class 8: 1..7"),
    (("--data", "synthetic", "--phase", "scratch", "--n_class", "0"), "--n_class 0: 1..7"),
    (("--data", "synthetic", "--phase", "scratch", "--weights", "x.pt"), "drop --weights"),
])
def test_refused_combinations_exit_with_their_message(argv, message, tmp_path):
    code, out = _cli("seg3d.py", "train", "--output", str(tmp_path), *argv)
    assert code != 0 and message in out, out


def test_a_label_bit_at_or_above_n_class_is_refused(tmp_path):
    D.write_synthetic(str(tmp_path), ["a"], (16, 8, 8), 3)
    assert D.open_case(str(tmp_path), "a", 3, 1).seg.shape == (16, 8, 8)
    with pytest.raises(SystemExit, match="--n_class is 2"):
        D.open_case(str(tmp_path), "a", 2, 1)
    seg = np.load(str(tmp_path / "a_seg.npy"))
    seg[0, 0, 0] |= 0x80                    # bit 7 is allowed: 'not counted'
    np.save(str(tmp_path / "a_seg.npy"), seg)
    D.open_case(str(tmp_path), "a", 3, 1)
    with pytest.raises(SystemExit, match="--in_channels 2"):
        D.open_case(str(tmp_path), "a", 3, 2)
    with pytest.raises(SystemExit, match="no such case list"):
        D.open_cases(str(tmp_path), "train.txt", 3, 1)


def test_main_py_3d_finetune_still_says_it_is_not_implemented():
    code, out = _cli("main.py", "--d", "3", "--phase", "finetune")
    assert code != 0 and "3D fine-tuning is not implemented" in out, out
