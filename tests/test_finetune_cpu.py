"""CPU: the surface of supervised 2D fine-tuning -- the command line's routing (no combination of --d / --phase falls through silently), the
labelled lists and the split, the label bitmask of the slot record, the evaluation transform's record, the uneven all-gather of scores and the
new C-ABI entry points."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

NEW_SYMBOLS = ("pcrl_cls_head_fwd", "pcrl_cls_head_bwd", "pcrl_cls_head_ws_bytes", "pcrl_auroc_counts")


def test_library_exports_the_finetune_entry_points():
    from pcrlv2_amd import _lib
    protos = _lib.parse_header()
    cdll = ctypes.CDLL(_lib.LIBPATH)
    for name in NEW_SYMBOLS:
        assert name in protos, f"{name} not declared in include/pcrl_hip.h"
        assert hasattr(cdll, name), f"{name} not exported"
    args = protos["pcrl_cls_head_fwd"][1]
    assert [n for _, n in args[:9]] == ["a", "keep", "keep_scale", "w", "b", "labels", "probs", "pooled", "loss"]
    assert [n for _, n in protos["pcrl_cls_head_bwd"][1][7:10]] == ["da", "dw", "db"]
    assert protos["pcrl_auroc_counts"][1][2] == ("int64_t*", "counts")


def test_entry_points_reject_what_they_cannot_compute():
    from pcrlv2_amd import _lib
    L = _lib.lib()
    assert L.call("pcrl_cls_head_ws_bytes", 5) == 40 and L.call("pcrl_cls_head_ws_bytes", 0) == 0
    with pytest.raises(_lib.PcrlError, match="power of two"):
        L.call("pcrl_cls_head_fwd", 16, None, 1.0, 16, 16, None, 16, 16, None, None, 0, 2, 7, 7, 500, 14, 1, None)
    with pytest.raises(_lib.PcrlError, match="classes"):
        L.call("pcrl_cls_head_fwd", 16, None, 1.0, 16, 16, None, 16, 16, None, None, 0, 2, 7, 7, 512, 65, 1, None)
    with pytest.raises(_lib.PcrlError, match="come together"):
        L.call("pcrl_cls_head_fwd", 16, None, 1.0, 16, 16, 16, 16, 16, None, None, 0, 2, 7, 7, 512, 14, 1, None)
    with pytest.raises(_lib.PcrlError, match="null pointer"):
        L.call("pcrl_cls_head_bwd", 16, None, 16, 16, None, 1.0, 16, 16, 16, 16, 2, 7, 7, 512, 14, 1, None)
    with pytest.raises(_lib.PcrlError, match="bad sizes"):
        L.call("pcrl_auroc_counts", 16, 16, 16, 0, 14, None)


# ---- the command line ----
def test_3d_finetune_exits_with_a_message(tmp_path):
    """The parent parsed --phase finetune, built the loaders, printed the arguments and returned with status 0 having trained nothing."""
    from pcrlv2_amd import main as M
    with pytest.raises(SystemExit) as e:
        M.main(["--d", "3", "--phase", "finetune", "--data", "synthetic", "--gpus", "0", "--output", str(tmp_path / "o")])
    assert e.value.code not in (0, None) and "--d 3" in str(e.value.code) and "not implemented" in str(e.value.code)
    with pytest.raises(SystemExit) as e:
        M.main(["--d", "3", "--phase", "scratch", "--data", "synthetic", "--gpus", "0", "--output", str(tmp_path / "o")])
    assert e.value.code not in (0, None)
    assert not (tmp_path / "o").exists()


def test_2d_finetune_without_encoder_weights_points_to_scratch(tmp_path):
    from pcrlv2_amd import main as M
    with pytest.raises(SystemExit) as e:
        M.main(["--d", "2", "--phase", "finetune", "--data", "synthetic", "--gpus", "0", "--output", str(tmp_path / "o")])
    assert e.value.code not in (0, None) and "--encoder_weights" in str(e.value.code) and "--phase scratch" in str(e.value.code)


@pytest.mark.parametrize("argv", [["--phase", "linear"], ["--d", "4"], ["--model", "genesis"], ["--d", "2", "--phase", "scratch", "--n_class", "32"]])
def test_unrouted_combinations_exit_non_zero(argv, tmp_path):
    from pcrlv2_amd import main as M
    with pytest.raises(SystemExit) as e:
        M.main(argv + ["--data", "synthetic", "--gpus", "0", "--output", str(tmp_path / "o")])
    assert e.value.code not in (0, None) and isinstance(e.value.code, str)


def test_parser_has_the_finetune_flags_and_keeps_the_old_defaults():
    from pcrlv2_amd import main as M
    a = M.build_parser().parse_args([])
    assert a.test_list == "./train_val_txt/chest_test.txt" and a.n_class == 14 and a.dropout == 0.2
    assert (a.phase, a.d, a.ratio, a.val_every, a.save_best, a.val_list) == ("pretask", 3, 0.8, 0, False, "./train_val_txt/chest_valid.txt")


def test_synthetic_labels_are_a_function_of_the_image():
    from pcrlv2_amd import main as M
    ld = M.SyntheticLabelledChestLoader(8, 2, 64, 14, seed=3, device="cpu")
    batches = list(ld)
    assert len(batches) == 2
    for x, y in batches:
        assert x.shape == (8, 3, 64, 64) and y.shape == (8, 14) and y.dtype == torch.uint8
        assert torch.equal(y, M.SyntheticLabelledChestLoader.labels_of(x, 14))
    both = torch.cat([y for _, y in batches])
    assert (both.sum(0) > 0).all() and (both.sum(0) < both.shape[0]).all()
    ld.reset_rng()
    assert torch.equal(next(iter(ld))[0], batches[0][0])


# ---- lists, split, bitmask ----
def _write_list(path, n, K, rng):
    lab = rng.integers(0, 2, (n, K))
    names = ["img_%02d.png" % i for i in range(n)]
    with open(path, "w") as f:
        for nm, row in zip(names, lab):
            f.write(nm + " " + " ".join(str(int(v)) for v in row) + "\n")
    return names, lab.astype(np.uint8)


def test_chest_labelled_list(tmp_path):
    from pcrlv2_amd import data_chest as D
    rng = np.random.default_rng(0)
    names, lab = _write_list(tmp_path / "l.txt", 7, 14, rng)
    got_n, got_l = D.chest_labelled_list("/imgs", str(tmp_path / "l.txt"))
    assert got_n == [os.path.join("/imgs", n) for n in names]
    assert got_l.dtype == np.uint8 and got_l.shape == (7, 14) and np.array_equal(got_l, lab)
    with open(tmp_path / "ragged.txt", "w") as f:
        f.write("a.png 0 1 0\nb.png 1 0\n")
    with pytest.raises(ValueError, match="ragged.txt:2"):
        D.chest_labelled_list("/imgs", str(tmp_path / "ragged.txt"))
    with open(tmp_path / "wide.txt", "w") as f:
        f.write("a.png " + " ".join(["1"] * 32) + "\n")
    with pytest.raises(ValueError, match="32 labels"):
        D.chest_labelled_list("/imgs", str(tmp_path / "wide.txt"))
    with pytest.raises(SystemExit):
        D.chest_labelled_list("/imgs", str(tmp_path / "absent.txt"))


@pytest.mark.parametrize("ratio", [0.0, 0.5, 0.95])
def test_finetune_split_is_the_complement_of_the_pretask_split(ratio, tmp_path):
    from pcrlv2_amd import data_chest as D
    rng = np.random.default_rng(1)
    lst = str(tmp_path / "chest_train.txt")
    names, lab = _write_list(lst, 20, 14, rng)
    for n in names:
        (tmp_path / n).write_bytes(b"")
    full = [os.path.join(str(tmp_path), n) for n in names]
    pre = D.chest_file_list(str(tmp_path), ratio, lst)
    fin, fin_lab = D.chest_finetune_split(str(tmp_path), ratio, lst)
    assert pre + fin == full and not set(pre) & set(fin)
    assert len(fin) == 20 - int(20 * ratio) and np.array_equal(fin_lab, lab[int(20 * ratio):])


def test_finetune_split_of_nothing_names_the_flag(tmp_path):
    from pcrlv2_amd import data_chest as D
    lst = str(tmp_path / "chest_train.txt")
    _write_list(lst, 20, 14, np.random.default_rng(2))
    with pytest.raises(SystemExit) as e:
        D.chest_finetune_split(str(tmp_path), 1.0, lst)
    assert "--ratio" in str(e.value.code)


@pytest.mark.parametrize("K", [1, 14, 31])
def test_label_bitmask_round_trip(K):
    from pcrlv2_amd import data_chest as D
    rng = np.random.default_rng(K)
    lab = rng.integers(0, 2, (50, K)).astype(np.uint8)
    lab[0], lab[1] = 0, 1
    m = D.pack_labels(lab)
    assert m.dtype == np.int32 and (m >= 0).all() and m[0] == 0 and m[1] == (1 << K) - 1
    assert np.array_equal(D.unpack_labels(m, K), lab)
    # through the slot record (H, W, C, bitmask) as the workers write it and the augment object reads it
    rec = torch.tensor([[37, 53, 1, int(v)] for v in m], dtype=torch.int32)
    assert np.array_equal(D.unpack_labels(rec.numpy()[:, 3], K), lab)
    with pytest.raises(ValueError):
        D.pack_labels(np.zeros((2, 32), np.uint8))


def test_labelled_kind_keeps_the_loader_contract(tmp_path):
    from PIL import Image
    from pcrlv2_amd import data_chest as D
    rng = np.random.default_rng(5)
    files = []
    for i, (h, w) in enumerate([(37, 53), (64, 64)]):
        p = str(tmp_path / ("i%d.png" % i))
        Image.fromarray(rng.integers(0, 256, (h, w), dtype=np.uint8)).save(p)
        files.append(p)
    lab = np.array([[1, 0, 1], [0, 1, 1]], np.uint8)
    entries = D.labelled_entries(files, lab)
    kind = D.ChestLabelledKind(entries, 3, train=False)
    assert kind.slot_shapes() == [((53 * 53 * 3,), torch.uint8), ((4,), torch.int32)]
    pix, rec = kind.dataset(entries)[0]
    assert rec.tolist() == [37, 53, 1, 0b101] and pix.dtype == torch.uint8 and pix.shape == (53 * 53 * 3,)
    bufs = [torch.zeros((2, 2) + tuple(sh), dtype=dt) for sh, dt in kind.slot_shapes()]
    assert kind.slot_dataset(entries, bufs)[(1, 0, 1)] == (1, 0)
    assert bufs[1][1, 0].tolist() == [64, 64, 1, 0b110]


# ---- the evaluation transform's record ----
@pytest.mark.parametrize("hw", [(37, 53), (64, 64)])
def test_eval_record_is_whole_image_identity_no_flip(hw):
    from pcrlv2_amd import data_chest as D
    H, W = hw
    rec = D.eval_records(np.array([[H, W, 1]]))[0]
    assert (rec[D.P_H], rec[D.P_W], rec[D.P_C]) == (H, W, 1)
    assert (rec[D.P_J], rec[D.P_I], rec[D.P_CW], rec[D.P_CH]) == (0, 0, W, H)
    assert tuple(rec[D.P_A0:D.P_A5 + 1]) == (65536, 0, 32768, 0, 65536, 32768) == D.rotate_fixed(0.0, 224, 224)
    assert rec[D.P_FLIP] == 0 and rec[D.P_NHOLES] == 0 and rec[D.P_GRAY] == 0 and rec[D.P_BLUR] == 0
    # the 16.16 affine is the identity on every output pixel
    a = [int(v) for v in rec[D.P_A0:D.P_A5 + 1]]
    for y in (0, 1, 111, 223):
        for x in (0, 1, 111, 223):
            assert ((a[2] + y * a[1] + x * a[0]) >> 16, (a[5] + y * a[4] + x * a[3]) >> 16) == (x, y)


# ---- gather_scores on two gloo ranks ----
def _gather_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pcrlv2_amd.train_finetune import gather_scores
        g = torch.Generator().manual_seed(0)
        probs, labels = torch.rand(8, 3, generator=g), (torch.rand(8, 3, generator=g) < 0.5).to(torch.uint8)
        lo, hi = (0, 3) if rank == 0 else (3, 8)
        p, y = gather_scores(probs[lo:hi].clone(), labels[lo:hi].clone())
        torch.save((p, y, probs, labels), os.path.join(out_dir, "r%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_gather_scores_uneven_shards_two_gloo_ranks(tmp_path):
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_gather_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        p, y, probs, labels = torch.load(str(tmp_path / ("r%d.pt" % r)))
        assert p.shape == (8, 3) and y.shape == (8, 3) and y.dtype == torch.uint8 and p.dtype == torch.float32
        assert torch.equal(p, probs) and torch.equal(y, labels)


def test_gather_scores_without_a_group_is_the_identity():
    from pcrlv2_amd.train_finetune import gather_scores
    p, y = torch.rand(4, 2), torch.ones(4, 2, dtype=torch.uint8)
    q, z = gather_scores(p, y)
    assert q is p and z is y
