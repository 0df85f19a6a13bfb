"""CPU: the host side of mirror test-time augmentation and checkpoint ensembling -- data_seg.parse_mirror, the two new entry
points in the header and the library, the alignment of tests/seg_mirror_reference.py (what the GPU tests of test_seg_mirror_gpu.py rest on), and the
refusals of `seg3d.py predict` / `train`, none of which touches a GPU."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pcrlv2_amd import data_seg as D  # noqa: E402
from pcrlv2_amd import seg3d  # noqa: E402
from pcrlv2_amd import train_seg as T  # noqa: E402
from seg_mirror_reference import flip_axes, mirror_dims, tta_logits  # noqa: E402


# ---- parse_mirror ---------------------------------------------------------------------------------------------------------------------------
def test_parse_mirror_accepts_every_spelling():
    assert D.parse_mirror("none") == [0] and D.parse_mirror(None) == [0] and D.parse_mirror(" None ") == [0]
    assert D.parse_mirror("all") == list(range(8)) and D.parse_mirror("ALL") == list(range(8))
    bit = {"x": 1, "y": 2, "z": 4}
    seen = 0
    for n in (1, 2, 3):
        for letters in itertools.permutations("xyz", n):
            chosen = sum(bit[c] for c in letters)
            want = [c for c in range(8) if c & ~chosen == 0]
            got = D.parse_mirror("".join(letters))
            assert got == want == sorted(got) and got[0] == 0 and len(got) == 2 ** n, letters
            assert D.mirror_letters(got) == "".join(c for c in "xyz" if c in letters)
            seen += 1
    assert seen == 15
    assert D.parse_mirror("xz") == [0, 1, 4, 5] and D.parse_mirror("zx") == [0, 1, 4, 5] and D.parse_mirror("y") == [0, 2]
    assert D.parse_mirror("xyz") == D.parse_mirror("all") and D.mirror_letters([0]) == "none"


@pytest.mark.parametrize("text", ["", " ", "xx", "xyzx", "w", "x,y", "x y", "0", "7", "nonee", "al", "xyzw", "-x"])
def test_parse_mirror_refuses_the_rest(text):
    with pytest.raises(SystemExit) as e:
        D.parse_mirror(text)
    assert str(e.value).startswith(f"--mirror {text}: none, all, or"), str(e.value)
    with pytest.raises(SystemExit, match="--val_mirror"):
        D.parse_mirror(text, "--val_mirror")


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_and_exported():
    from pcrlv2_amd import _lib
    if not os.path.exists(_lib.LIBPATH):
        import __graft_entry__ as g
        g.build()
    protos = _lib.parse_header()
    cdll = ctypes.CDLL(_lib.LIBPATH)
    want = {"pcrl_seg_cut_patches_mirror": ["img", "src_half", "starts", "out", "n", "C", "X", "Y", "Z", "cx", "cy", "cz", "flip", "stream"],
            "pcrl_seg_head_logits_acc": ["a", "w", "b", "z", "N", "S", "K", "dtype", "cx", "cy", "cz", "flip", "first", "scale", "stream"]}
    for name, args in want.items():
        assert name in protos, f"{name} is not declared in include/pcrl_hip.h"
        assert protos[name][0] == "int" and [a for _, a in protos[name][1]] == args
        assert hasattr(cdll, name), f"{name} is not exported"
    assert dict((a, t) for t, a in protos["pcrl_seg_head_logits_acc"][1])["scale"] == "float"
    # the two existing entry points keep their signatures (that the header is plain C is test_host_cpu.py's)
    assert [a for _, a in protos["pcrl_seg_cut_patches"][1]] == want["pcrl_seg_cut_patches_mirror"][:12] + ["stream"]
    assert [a for _, a in protos["pcrl_seg_head_logits"][1]] == want["pcrl_seg_head_logits_acc"][:8] + ["stream"]


# ---- the restatement's alignment --------------------------------------------------------------------------------------------------------------
def test_mirror_dims_and_flip_axes():
    assert [mirror_dims(c, 1) for c in range(8)] == [[], [1], [2], [1, 2], [3], [1, 3], [2, 3], [1, 2, 3]]
    a = np.arange(2 * 3 * 5 * 7, dtype=np.float32).reshape(2, 3, 5, 7)
    for code in range(8):
        f = flip_axes(a, code, 1)
        fx, fy, fz = code & 1, code >> 1 & 1, code >> 2 & 1
        for i, j, k in ((0, 0, 0), (1, 2, 3), (2, 4, 6)):
            assert np.array_equal(f[:, i, j, k], a[:, 2 - i if fx else i, 4 - j if fy else j, 6 - k if fz else k])
        assert np.array_equal(flip_axes(f, code, 1), a) and f.flags.c_contiguous
        t = flip_axes(torch.from_numpy(a), code, 1)
        assert t.is_contiguous() and np.array_equal(t.numpy(), f)


def test_every_single_pass_unmirrors_to_the_input_and_exact_means_are_the_input():
    """The identity as the 'network': the patch is mirrored, 'inferred' (unchanged) and un-mirrored.  Small integers accumulate exactly in float32
    and M in {2, 4, 8} divides exactly, so the mean over the passes is the input, bit for bit."""
    rng = np.random.default_rng(7)
    x = rng.integers(-64, 65, (2, 3, 5, 7, 3)).astype(np.float32)          # [n, cx, cy, cz, K]
    for code in range(8):
        seen = flip_axes(x, code, 1)                                        # what the network is shown
        assert code == 0 or not np.array_equal(seen, x)
        back = flip_axes(seen, code, 1)
        assert np.array_equal(back, x)
        assert np.array_equal(tta_logits([back], 1.0), x)
    for text in ("z", "xz", "all"):
        codes = D.parse_mirror(text)
        passes = [flip_axes(flip_axes(x, c, 1), c, 1) for c in codes]
        assert len(codes) in (2, 4, 8) and np.array_equal(tta_logits(passes, np.float32(1.0 / len(codes))), x), text
    # one operation at a time, in pass order: float32 addition is not associative, and the restatement keeps the order it is given
    a, b, c = np.float32(1.0), np.float32(2.0 ** -24), np.float32(2.0 ** -24)
    assert tta_logits([np.array([a]), np.array([b]), np.array([c])], 1.0)[0] == np.float32(1.0)
    assert tta_logits([np.array([b]), np.array([c]), np.array([a])], 1.0)[0] == np.float32(1.0 + 2.0 ** -23)
    assert tta_logits([np.array([np.float32(3.0)])], np.float32(1 / 24))[0] == np.float32(3.0) * np.float32(1 / 24)


# ---- the commands' refusals ---------------------------------------------------------------------------------------------------------------------
PREDICT = ["predict", "--data", "d", "--list", "l.txt", "--out", "o"]
TRAIN = ["train", "--data", "synthetic", "--phase", "scratch"]


@pytest.fixture
def no_gpu(monkeypatch):
    """Anything that reaches for the device fails the test."""
    def touched(*a, **k):
        raise AssertionError("the refusal must come before a GPU is touched")
    monkeypatch.setattr(torch.cuda, "set_device", touched)
    monkeypatch.setattr(torch.nn.Module, "to", touched)


@pytest.mark.parametrize("argv,message", [
    (PREDICT + ["--weights", "a.pt", "--mirror", "xx"], "--mirror xx: none, all, or"),
    (PREDICT + ["--weights", "a.pt", "--mirror", "w"], "--mirror w: none, all, or"),
    (PREDICT + ["--weights", "a.pt", "--mirror", ""], "--mirror : none, all, or"),
    (PREDICT + ["--weights", "a.pt", "--probs"], "--probs writes the blended probabilities"),
    (PREDICT + ["--weights", "a.pt", "--probs", "--mirror", "none"], "--probs writes the blended probabilities"),
    (PREDICT + ["--weights", "a.pt,,b.pt"], "--weights a.pt,,b.pt: one checkpoint"),
    (PREDICT + ["--weights", "a.pt,"], "--weights a.pt,: one checkpoint"),
    (PREDICT + ["--weights", ""], "--weights : one checkpoint"),
    (PREDICT + ["--weights", "a.pt", "--mirror", "all", "--overlap", "0.8"], "--overlap 0.8"),
    (TRAIN + ["--val_mirror", "xyx"], "--val_mirror xyx: none, all, or"),
    (TRAIN + ["--val_mirror", "both"], "--val_mirror both: none, all, or"),
    (TRAIN + ["--val_mirror", "x", "--val_window", "hann"], "--val_window hann"),
])
def test_refused_flag_combinations_exit_with_their_message(argv, message, no_gpu):
    with pytest.raises(SystemExit) as e:
        seg3d.main(argv)
    assert str(e.value).startswith(message), str(e.value)


def test_probs_are_allowed_with_a_mirror_or_several_checkpoints():
    parse = seg3d.build_parser().parse_args
    seg3d.check_predict(parse(PREDICT + ["--weights", "a.pt", "--probs", "--mirror", "x"]))
    seg3d.check_predict(parse(PREDICT + ["--weights", "a.pt,b.pt", "--probs"]))
    seg3d.check_predict(parse(PREDICT + ["--weights", "a.pt", "--probs", "--overlap", "0.5"]))
    seg3d.check_predict(parse(PREDICT + ["--weights", "a.pt"]))
    args = parse(PREDICT + ["--weights", "a.pt"])
    assert args.mirror == "none" and parse(TRAIN).val_mirror == "none"
    seg3d.check_train(parse(TRAIN + ["--val_mirror", "zy"]))
    assert T.split_weights("a.pt") == ["a.pt"] and T.split_weights(" a.pt , b/c.pt ") == ["a.pt", "b/c.pt"]


def _tiny_state_dict(n_class, in_channels):
    return {"out_tr.final_conv.weight": torch.zeros(n_class, 64, 1, 1, 1), "down_tr64.ops.0.conv1.weight": torch.zeros(32, in_channels, 3, 3, 3)}


def test_mismatched_checkpoints_exit_naming_both_files(tmp_path, no_gpu):
    a, b, c = (str(tmp_path / n) for n in ("fold0.pt", "fold1.pt", "fold2.pt"))
    torch.save({"state_dict": _tiny_state_dict(3, 1)}, a)
    torch.save({"state_dict": _tiny_state_dict(2, 1)}, b)
    torch.save({"state_dict": _tiny_state_dict(3, 4)}, c)
    assert T.check_ensemble([a, a], [_tiny_state_dict(3, 1), _tiny_state_dict(3, 1)]) == (3, 1)
    for other, what in ((b, "n_class 2 and in_channels 1"), (c, "n_class 3 and in_channels 4")):
        with pytest.raises(SystemExit) as e:
            seg3d.main(PREDICT + ["--weights", f"{a},{other}"])
        msg = str(e.value)
        assert a in msg and other in msg and what in msg and "n_class 3 and in_channels 1" in msg, msg
    with pytest.raises(SystemExit, match="no such file"):
        seg3d.main(PREDICT + ["--weights", f"{a},{tmp_path / 'absent.pt'}"])
