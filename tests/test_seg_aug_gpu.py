"""pcrl_seg_aug_resample (csrc/seg_augment.hip), ops.seg_augment, the augmented training step (train_seg.augment_batch / train_step) and
`seg3d.py train --augment` on the GPU.  Case table, lattice and bounds: seg_aug_cases.py; float64 restatement: seg_aug_reference.py; their
preconditions are checked without a GPU in test_seg_aug_cpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import seg_aug_cases as SC  # noqa: E402
import seg_aug_reference as R  # noqa: E402
from pcrlv2_amd import ops  # noqa: E402
from pcrlv2_amd._lib import PcrlError, lib, stream_handle  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _run(case):
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
    x, lab = ops.seg_augment(up(case["src"]), up(case["src_lab"]), up(case["inv"]), up(case["gain"]), up(case["bias"]), crop=case["crop"])
    torch.cuda.synchronize()
    return x.cpu().numpy(), lab.cpu().numpy()


def _ref(case):
    return R.ref_resample(case["src"], case["src_lab"], case["inv"], case["gain"], case["bias"], case["crop"])


# ---- 1. bit for bit on the lattice -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ext,crop,C,half", SC.lattice_cases(), ids=[c[0] for c in SC.lattice_cases()])
def test_lattice_bit_for_bit(cid, ext, crop, C, half):
    case = SC.lattice_case(ext, crop, C, half)
    x, lab = _run(case)
    y, want_lab, _ = _ref(case)
    want = y.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), y)
    assert x.dtype == np.float32 and x.shape == want.shape and lab.dtype == np.uint8 and lab.shape == want_lab.shape
    for b, name in enumerate(case["names"]):
        bad = x[b].view(np.int32) != want[b].view(np.int32)
        assert not bad.any(), f"{name} (sample {b}): {int(bad.sum())} image voxels differ, first at {tuple(np.argwhere(bad)[0])}"
        bad = lab[b] != want_lab[b]
        assert not bad.any(), f"{name} (sample {b}): {int(bad.sum())} label bytes differ, first at {tuple(np.argwhere(bad)[0])}"
    assert (want_lab == 0x80).any() and (want != 0).any()


# ---- 2. generic matrices ---------------------------------------------------------------------------------------------------------------------
def test_generic_rotations_within_the_derived_bound():
    case = SC.generic_case()
    x, lab = _run(case)
    y, want_lab, s = _ref(case)
    bound = SC.generic_bound(case)
    err = np.abs(x.astype(np.float64) - y).max(axis=(2, 3, 4))
    print("[seg aug generic] worst image error / bound per draw:", " ".join("%.2e/%.2e" % (e, b) for e, b in zip(err.max(axis=1), bound.min(axis=1))))
    assert (err <= bound).all(), (err / bound).max()
    clear = SC.away_from_ties(s)
    share = 1.0 - clear.reshape(clear.shape[0], -1).mean(axis=1)
    assert (share <= SC.MAX_EXCLUDED).all()
    bad = (lab != want_lab) & clear
    print("[seg aug generic] excluded label share: max %.5f; label mismatches among the excluded: %d" % (share.max(), int((lab != want_lab).sum())))
    assert not bad.any(), f"{int(bad.sum())} label bytes away from a tie differ"


# ---- 3. label bits survive -------------------------------------------------------------------------------------------------------------------
def test_label_bits_survive():
    case = SC.label_bits_case()
    _, lab = _run(case)
    for b in range(lab.shape[0]):
        present = set(np.unique(case["src_lab"][b]).tolist()) | {0x80}
        got = set(np.unique(lab[b]).tolist())
        assert got <= present, f"sample {b}: bytes {sorted(got - present)} are in no source voxel"
        assert len(got) > 8, "the crop holds many of the patterns"
    assert int(np.bitwise_or.reduce(lab.reshape(-1))) == 0xFF


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_returns_its_error_and_launches_nothing():
    B, C, ext, crop = 2, 2, (6, 5, 4), (4, 4, 4)
    src = torch.ones((B, C) + ext, device=DEV)
    src_lab = torch.ones((B,) + ext, dtype=torch.uint8, device=DEV)
    y = torch.full((B, C) + crop, -7.0, device=DEV)
    lab = torch.full((B,) + crop, 0x33, dtype=torch.uint8, device=DEV)
    inv = torch.tensor([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]] * B, dtype=torch.float32, device=DEV)
    gain, bias = torch.ones((B, C), device=DEV), torch.zeros((B, C), device=DEV)
    good = [src, 0, src_lab, y, lab, inv, gain, bias, B, C, *ext, *crop]

    def refused(match, **change):
        args = list(good)
        for k, v in change.items():
            args[int(k[1:])] = v
        with pytest.raises(PcrlError, match=match):
            lib().call("pcrl_seg_aug_resample", *args, stream_handle())
        torch.cuda.synchronize()
        assert bool((y == -7.0).all()) and bool((lab == 0x33).all()), f"{change}: something was launched"

    for i in (0, 2, 3, 4, 5, 6, 7):
        refused("null pointer", **{f"a{i}": None})
    refused("overlap", a3=src)                       # y on src
    refused("overlap", a4=src_lab)                   # lab on src_lab
    refused("overlap", a3=src.view(-1)[8:])          # y inside src
    refused("overlap", a4=src.view(torch.uint8))     # lab on src
    big = torch.full((B * C * 64 + 64,), -7.0, device=DEV)
    refused("overlap", a3=big, a4=big[B * C * 64 - 1:].view(torch.uint8))      # lab on the last element of y
    for bad in (0, -1, 65536):
        refused("1 <= B <= 65535", a8=bad)
    for bad in (0, -2, 17):
        refused("1 <= C <= 16", a9=bad)
    for i in range(10, 16):
        for bad in (0, -3):
            refused("empty extent", **{f"a{i}": bad})
    refused("2\\^31 voxels", a10=2048, a11=1024, a12=1024)
    refused("2\\^31 voxels", a13=1024, a14=2048, a15=1024)
    # the largest sizes that pass the checks are refused by nothing: B = 65535 and C = 16 are legal (not launched here: the buffers are small)
    # the wrapper's own refusals
    for change in ({"src": src.cpu()}, {"src": src.double()}, {"src": src[:, :, :, :, ::2]}, {"src_lab": src_lab[:1]}, {"src_lab": src_lab.int()},
                   {"inv": inv[:, :9].contiguous()}, {"gain": gain[:1]}, {"bias": bias.double()}, {"crop": None}, {"crop": (4, 4)}, {"crop": (4, 0, 4)},
                   {"out": (y, lab[:1])}, {"out": (y.double(), lab)}):
        kw = {"src": src, "src_lab": src_lab, "inv": inv, "gain": gain, "bias": bias, "crop": crop}
        kw.update(change)
        if "out" in change:
            kw["crop"] = None
        with pytest.raises(PcrlError, match="seg_augment"):
            ops.seg_augment(kw.pop("src"), kw.pop("src_lab"), kw.pop("inv"), kw.pop("gain"), kw.pop("bias"), **kw)
    # and the good call, into `out`, writes both
    ox, ol = ops.seg_augment(src, src_lab, inv, gain, bias, out=(y, lab))
    torch.cuda.synchronize()
    assert ox is y and ol is lab and bool((y == 1.0).all()) and bool((lab == 1).all())


def test_no_matrix_reads_outside_the_box():
    """Huge, infinite and NaN entries: a coordinate is clamped before it becomes an index and every read is bounds-checked in the kernel, so the result
    is 'outside' (bias, 0x80) or a value of the box.  What the host's source-extent bound promises plays no part."""
    B, C, ext, crop = 6, 1, (5, 4, 3), (4, 4, 4)
    src = torch.full((B, C) + ext, 2.0, device=DEV)
    src_lab = torch.full((B,) + ext, 5, dtype=torch.uint8, device=DEV)
    eye = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    rows = [[v * 1e30 for v in eye], [0, 0, 0, 3e9, 0, 0, 0, -3e9, 0, 0, 0, 1e38], [float("nan")] * 12, [float("inf")] + eye[1:],
            eye[:3] + [float("-inf")] + eye[4:], [v * 2.0 ** 31 for v in eye]]
    inv = torch.tensor(rows, dtype=torch.float32, device=DEV)
    x, lab = ops.seg_augment(src, src_lab, inv, torch.ones((B, C), device=DEV), torch.full((B, C), 0.5, device=DEV), crop=crop)
    torch.cuda.synchronize()
    assert bool(torch.isin(lab, torch.tensor([5, 0x80], dtype=torch.uint8, device=DEV)).all())
    assert bool((lab[1:5] == 0x80).all()) and bool((x[1:5] == 0.5).all()), "a coordinate that is nowhere gives the outside values"
    assert bool(((x >= 0.5) & (x <= 2.5)).all())


# ---- 5. the training path ----------------------------------------------------------------------------------------------------------------------
def test_train_step_on_an_augmented_batch():
    from pcrlv2_amd.models import Segmenter3d
    from pcrlv2_amd.optim import FusedSGD
    from pcrlv2_amd.train_seg import augment_batch, is_augmented, train_step
    batch = SC.train_batch()
    assert is_augmented(batch) and not is_augmented(batch[:2])
    count, settled = SC.counted_voxels(batch)
    assert settled
    with lib().count_calls("pcrl_seg_aug_resample", "pcrl_aug_noise_gamma") as calls:
        x1, lab1 = augment_batch(batch)
        x2, lab2 = augment_batch(batch)
    torch.cuda.synchronize()
    assert calls == {"pcrl_seg_aug_resample": 2, "pcrl_aug_noise_gamma": 2}
    assert x1.dtype == torch.float32 and tuple(x1.shape) == (SC.TRAIN_B, SC.TRAIN_C) + SC.TRAIN_CROP and tuple(lab1.shape) == (SC.TRAIN_B,) + SC.TRAIN_CROP
    assert torch.equal(x1.view(torch.int32), x2.view(torch.int32)) and torch.equal(lab1, lab2), "the same parameters give the same bytes"
    assert bool(torch.isfinite(x1).all()) and int((lab1 < 0x80).sum()) == count
    # neutral intensity: the noise / gamma pass is skipped, and the result is the resampling alone, bit for bit
    p = dict(batch[2], gamma=torch.ones_like(batch[2]["gamma"]), noise_std=torch.zeros_like(batch[2]["noise_std"]))
    with lib().count_calls("pcrl_seg_aug_resample", "pcrl_aug_noise_gamma") as calls:
        x3, lab3 = augment_batch((batch[0], batch[1], p))
    up = lambda t: t.to(DEV)      # noqa: E731
    x4, _ = ops.seg_augment(up(batch[0]), up(batch[1]), up(p["inv"]), up(p["gain"]), up(p["bias"]), crop=SC.TRAIN_CROP)
    assert calls == {"pcrl_seg_aug_resample": 1} and torch.equal(x3.view(torch.int32), x4.view(torch.int32)) and torch.equal(lab3, lab1)
    y, want_lab, s = R.ref_resample(batch[0].numpy(), batch[1].numpy(), p["inv"].numpy(), p["gain"].numpy(), p["bias"].numpy(), SC.TRAIN_CROP)
    clear = SC.away_from_ties(s)
    assert np.array_equal(lab1.cpu().numpy()[clear], want_lab[clear]) and np.abs(x3.cpu().numpy() - y).max() < 1e-2
    # the step itself
    torch.manual_seed(0)
    model = Segmenter3d(SC.TRAIN_K, in_channels=SC.TRAIN_C).cuda().train()
    opt = FusedSGD(model.trainable_parameters(), lr=1e-2, momentum=0.9, weight_decay=1e-4)
    with lib().count_calls("pcrl_seg_aug_resample", "pcrl_aug_noise_gamma") as calls:
        loss, sums = train_step(model, opt, batch)
    assert calls == {"pcrl_seg_aug_resample": 1, "pcrl_aug_noise_gamma": 1}
    assert bool(torch.isfinite(loss)) and float(sums[-1]) == float(count)
    # a two-entry batch takes the path it always took
    with lib().count_calls("pcrl_seg_aug_resample", "pcrl_aug_noise_gamma") as calls:
        loss2, sums2 = train_step(model, opt, (x1.cpu(), lab1.cpu()))
    assert calls == {} and bool(torch.isfinite(loss2)) and float(sums2[-1]) == float(count)


def test_float16_sources_go_to_the_device_as_float16():
    from pcrlv2_amd.train_seg import augment_batch
    batch = SC.train_batch()
    p = dict(batch[2], gamma=torch.ones_like(batch[2]["gamma"]), noise_std=torch.zeros_like(batch[2]["noise_std"]))
    half = batch[0].half()
    x16, lab16 = augment_batch((half, batch[1], p))
    x32, lab32 = augment_batch((half.float(), batch[1], p))
    assert torch.equal(x16.view(torch.int32), x32.view(torch.int32)) and torch.equal(lab16, lab32), "a float16 source is widened exactly"


# ---- 6. end to end -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("augment", [True, False], ids=["augment", "plain"])
def test_seg3d_train_end_to_end(augment, tmp_path, capsys, monkeypatch):
    from pcrlv2_amd import seg3d
    for k in ("HIP_VISIBLE_DEVICES", "PCRL_LOADER_WORKERS"):          # launch() sets them: monkeypatch puts back what was there
        if k in os.environ:
            monkeypatch.setenv(k, os.environ[k])
        else:
            monkeypatch.delenv(k, raising=False)
    argv = ["train", "--data", "synthetic", "--phase", "scratch", "--n_class", "3", "--crop", "16,16,8", "--b", "2", "--epochs", "1", "--steps_per_epoch", "2",
            "--output", str(tmp_path / "out")] + (["--augment"] if augment else [])
    with lib().count_calls("pcrl_seg_aug_resample") as calls:
        model = seg3d.main(argv)
    out = capsys.readouterr().out
    assert out.count("Val: [") == 2 and out.count("Test: (") == 1 and "mean Dice" in out, out[-2000:]       # epochs 0 and 1 (inclusive upper bound)
    assert calls == ({"pcrl_seg_aug_resample": 4} if augment else {})
    assert model.test_metrics["mean_dice"] == model.test_metrics["mean_dice"]
