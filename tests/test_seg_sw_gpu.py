"""Overlap-blended sliding-window inference end to end on the GPU: Segmenter3d.infer_logits, train_seg.sliding_window / evaluate_sliding and the two
commands.  A tiny Segmenter3d from a fixed seed, crop 16 x 16 x 8, K = 3."""
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pcrlv2_amd import data_seg as D  # noqa: E402
from pcrlv2_amd.models import Segmenter3d  # noqa: E402
from pcrlv2_amd.train_seg import evaluate, evaluate_sliding, predict_case, sliding_window  # noqa: E402
from seg_blend_reference import blend32, mask_of  # noqa: E402

pytestmark = pytest.mark.gpu
K, B, CROP = 3, 2, (16, 16, 8)
_DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])


def _model(dtype, seed=0):
    torch.manual_seed(seed)
    return Segmenter3d(K).cuda().eval().set_compute_dtype(dtype)


def _digest(model):
    h = hashlib.sha256()
    for k, v in model.state_dict().items():
        h.update(k.encode())
        h.update(v.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def _pack(z):
    return sum(((z[..., k] >= 0).to(torch.uint8) << k) for k in range(z.shape[-1])).to(torch.uint8)


@_DTYPES
def test_infer_logits_threshold_to_infers_mask_and_leave_the_model_alone(dtype):
    model = _model(dtype).train()                    # whatever self.training says
    before = _digest(model)
    x = torch.randn((2, 1) + CROP, generator=torch.Generator().manual_seed(1)).cuda()
    z = model.infer_logits(x)
    mask = model.infer(x, want_mask=True)[3]
    torch.cuda.synchronize()
    assert z.shape == (2,) + CROP + (K,) and z.dtype == torch.float32
    assert torch.equal(_pack(z), mask) and mask.unique().numel() > 1, "the same mask, and not a constant one"
    assert _digest(model) == before and model.training


@_DTYPES
def test_overlap_0_with_the_constant_window_is_the_tiled_path(dtype):
    """Shape a multiple of the crop, overlap 0, all weights 1: every voxel has one patch, num = z and den = 1 exactly -- the mask and the counts are the
    tiled path's, the loss differs by the order of its float64 sums alone."""
    model = _model(dtype)
    cases = [D.synthetic_case(3, i, (32, 16, 16), K) for i in range(2)]
    counts = torch.zeros((2, K, 3), dtype=torch.int64, device="cuda")
    want_counts = torch.zeros_like(counts)
    for ci, case in enumerate(cases):
        mask, probs, sums = sliding_window(model, case, CROP, B, 0.0, "constant", counts=counts, row=ci)
        assert probs is None and np.array_equal(mask.cpu().numpy(), predict_case(model, case, CROP, B)), case.name
        for x, lab, _, _ in D.TileLoader([case], CROP, B):
            model.infer(x.cuda(), labels=lab.cuda(), case_index=torch.full((x.shape[0],), ci, dtype=torch.int32, device="cuda"), counts=want_counts)
    assert torch.equal(counts, want_counts) and int(counts[:, :, 2].sum()) > 0
    tiled = evaluate(model, D.TileLoader(cases, CROP, B))
    blended = evaluate_sliding(model, cases, CROP, B, 0.0, "constant")
    assert blended["dice"] == tiled["dice"] and blended["mean_dice"] == tiled["mean_dice"] and blended["cases"] == tiled["cases"] == 2
    assert abs(blended["loss"] - tiled["loss"]) <= 1e-12 * abs(tiled["loss"]), (blended["loss"], tiled["loss"])


@_DTYPES
def test_blended_mask_is_the_float32_restatement_of_host_cut_patches(dtype):
    """The cutter, the patch order and the blend in one piece: a phantom that is no multiple of the crop, overlap 0.5, Gaussian window."""
    model = _model(dtype)
    shape = D.synthetic_shape(CROP)
    case = D.synthetic_case(5, 0, shape, K)
    axes, weights = D.windows(shape, CROP, 0.5), D.blend_weights(CROP, "gaussian")
    starts = D.window_starts(axes)
    assert any(n % c for n, c in zip(shape, CROP)) and len(starts) > B
    xs = np.stack([D.cut(case, st, CROP)[0] for st in starts])
    z = torch.cat([model.infer_logits(torch.from_numpy(xs[i:i + B]).cuda()) for i in range(0, len(starts), B)]).cpu().numpy()
    num, den = blend32(z, axes, weights, shape)
    mask, probs, sums = sliding_window(model, case, CROP, B, 0.5, "gaussian", want_probs=True)
    assert np.array_equal(mask.cpu().numpy(), mask_of(num, case.seg)) and 0 < int(mask.count_nonzero())
    assert probs.shape == (K,) + shape and float(sums[4 * K]) == float(np.prod(shape))
    bare = sliding_window(model, D.Case(case.name, case.img), CROP, B, 0.5, "gaussian")       # unlabelled, no counts: nothing to sum
    assert np.array_equal(bare[0].cpu().numpy(), mask_of(num)) and bare[1] is None and bare[2] is None


def _cli(*argv, timeout=300):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "seg3d.py"), *argv], cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


_TODAY_VAL = re.compile(r"^Val: \[\d+\]\tloss \d+\.\d{4}\tmean Dice \d\.\d{4}\t\(2 cases\)$")
_TODAY_TEST = re.compile(r"^Test: \((last|best) epoch \d+\)\tloss \d+\.\d{4}\tmean Dice \d\.\d{4}\t\(2 cases\)\tper class( \d\.\d{4}){3}$")


def test_train_validates_by_sliding_windows_and_predict_writes_probabilities(tmp_path):
    common = ("train", "--data", "synthetic", "--phase", "scratch", "--epochs", "2", "--steps_per_epoch", "3", "--b", "2", "--crop", "16,16,8", "--save_best")
    out_dir = str(tmp_path / "out")
    log = _cli(*common, "--output", out_dir, "--val_overlap", "0.5")
    val = [ln for ln in log.splitlines() if ln.startswith("Val: [")]
    test = [ln for ln in log.splitlines() if ln.startswith("Test: (")]
    assert len(val) == 3 and len(test) == 1, log[-2000:]       # --epochs is the last epoch index: 0, 1, 2
    for ln in val + test:
        assert ln.endswith("\toverlap 0.5 gaussian"), ln
    assert _TODAY_VAL.match(val[0][:-len("\toverlap 0.5 gaussian")]) and _TODAY_TEST.match(test[0][:-len("\toverlap 0.5 gaussian")]), (val, test)
    plain = _cli(*common, "--output", str(tmp_path / "plain"))
    lines = [ln for ln in plain.splitlines() if ln.startswith(("Val: [", "Test: ("))]
    assert len(lines) == 4 and not any("overlap" in ln for ln in lines)
    assert all(_TODAY_VAL.match(ln) for ln in lines[:3]) and _TODAY_TEST.match(lines[3]), lines
    # predict --overlap 0.5 --probs on two cases whose size is no multiple of the crop
    best = os.path.join(out_dir, "pcrlv2_seg3d_scratch_1.0_best.pt")
    data, pred = str(tmp_path / "data"), str(tmp_path / "pred")
    D.write_synthetic(data, ["p0", "p1"], (20, 18, 12), K, seed=9)
    with open(os.path.join(data, "two.txt"), "w") as f:
        f.write("p0\np1\n")
    _cli("predict", "--data", data, "--list", "two.txt", "--weights", best, "--out", pred, "--crop", "16,16,8", "--b", "4", "--overlap", "0.5", "--probs")
    for name in ("p0", "p1"):
        m, p = np.load(os.path.join(pred, name + "_pred.npy")), np.load(os.path.join(pred, name + "_prob.npy"))
        assert m.shape == (20, 18, 12) and m.dtype == np.uint8 and p.shape == (K, 20, 18, 12) and p.dtype == np.float16
        for k in range(K):
            decided = p[k] != np.float16(0.5)
            assert np.array_equal(((m >> k) & 1).astype(bool)[decided], (p[k] > np.float16(0.5))[decided]), (name, k)
