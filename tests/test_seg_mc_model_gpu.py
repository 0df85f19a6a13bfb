"""models.Segmenter3d(head='softmax'), functions.SegSoftmaxHeadFn, train_seg and the seg3d command line on label maps: crop 16x16x8, b = 2, K = 4.
The loss bound is tests/test_seg_mc_head_gpu.py's, derived there, applied to the activation the model's own features() hands to the head."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pcrlv2_amd import data_seg as D  # noqa: E402
from pcrlv2_amd import functions as Fn, ops  # noqa: E402
from pcrlv2_amd.models import PCRLv23d, Segmenter3d  # noqa: E402
from pcrlv2_amd.train_seg import loss_from_sums  # noqa: E402
from seg_mc_reference import lowest_argmax, reference  # noqa: E402
from test_seg_mc_head_gpu import _bounds  # noqa: E402

pytestmark = pytest.mark.gpu
K, B, CROP = 4, 2, (16, 16, 8)
_DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
HEAD_PARTS = (".bn.", ".predictor_head.", ".deep_supervision_head.")


def _model(dtype, seed=0):
    torch.manual_seed(seed)
    return Segmenter3d(K, head="softmax").cuda().train().set_compute_dtype(dtype)


def _batch(seed=0):
    cases = [D.synthetic_case(seed, i, CROP, K, head="softmax") for i in range(B)]
    x = torch.from_numpy(np.stack([c.img for c in cases])).cuda()
    lab = torch.from_numpy(np.stack([c.seg for c in cases]))
    lab[:, :2] |= 0x80
    return x, lab.cuda()


def _rows(a):
    """the logical [N, 64, D, H, W] activation -> its [M, 64] rows on the host"""
    return a.detach().permute(0, 2, 3, 4, 1).reshape(-1, 64).cpu()


@_DTYPES
def test_loss_is_the_reference_on_the_models_features_and_every_trainable_parameter_gets_a_gradient(dtype):
    model = _model(dtype)
    x, lab = _batch()
    assert int((lab.cpu() & 0x7F).max()) == K - 1
    params = dict(model.named_parameters())
    ops.begin_step()
    Fn.reset_parked()
    loss, sums = model.loss(x, lab)
    loss.backward()
    torch.cuda.synchronize()
    got = {n for n, p in params.items() if p.grad is not None}
    assert got == {n for n, p in params.items() if p.requires_grad} and not any(h in n for n in got for h in HEAD_PARTS)
    assert all(bool(torch.isfinite(params[n].grad).all()) for n in got) and bool(params["out_tr.final_conv.weight"].grad.abs().sum() > 0)
    # the same features again (training-mode BatchNorm of the same batch: the same activation), the float64 restatement on them
    ops.begin_step()
    Fn.reset_parked()
    with torch.no_grad():
        a = ops.to_act(model.features(x), dtype)
        ops.end_of_forward_join()
    fc = model.out_tr.final_conv
    l2, s2 = ops.seg_mc_head_forward(a, fc.weight, fc.bias, lab, dtype)
    torch.cuda.synchronize()
    assert torch.equal(l2.cpu(), loss.detach().cpu()) and torch.equal(s2.cpu(), sums.cpu())
    rows, w, b = _rows(a), fc.weight.detach().view(K, 64).cpu(), fc.bias.detach().cpu()
    ref = reference(rows, w, b, lab.cpu().reshape(-1))
    S = CROP[0] * CROP[1] * CROP[2]
    tol = _bounds(rows, w, b, ref, K, B, S, dtype, 1.0)
    for name, g in (("loss", loss.detach().cpu()), ("sums", sums.cpu())):
        err = (g.double() - ref[name]).abs()
        print(f"[seg_mc model {dtype}] {name}: worst error / bound {float((err / tol[name].clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= tol[name]).all()), name


@_DTYPES
def test_the_models_loss_weights_reach_the_training_loss_and_the_eval_loss(dtype):
    """Segmenter3d(head='softmax', wc=0.5, wd=1.5): model.loss is the raw forward with THESE weights on the model's own features bit for bit and the
    float64 restatement with them within tests/test_seg_mc_head_gpu.py's bound (a swap, or the defaults, is far outside it); infer's loss is
    train_seg.loss_from_sums of infer's sums with the model's weights, to the float32 rounding of the device value (the device evaluates the same
    float64 expression, possibly with one fused multiply-add: 8 x 2^-53 of the terms, then half a float32 ulp)."""
    wc, wd = 0.5, 1.5
    torch.manual_seed(0)
    model = Segmenter3d(K, head="softmax", wc=wc, wd=wd).cuda().train().set_compute_dtype(dtype)
    assert (model.wc, model.wd) == (wc, wd)
    x, lab = _batch()
    ops.begin_step()
    Fn.reset_parked()
    loss, sums = model.loss(x, lab)
    loss.backward()
    torch.cuda.synchronize()
    ops.begin_step()
    Fn.reset_parked()
    with torch.no_grad():
        a = ops.to_act(model.features(x), dtype)
        ops.end_of_forward_join()
    fc = model.out_tr.final_conv
    l2, s2 = ops.seg_mc_head_forward(a, fc.weight, fc.bias, lab, dtype, wc, wd)
    torch.cuda.synchronize()
    assert torch.equal(l2.cpu(), loss.detach().cpu()) and torch.equal(s2.cpu(), sums.cpu())
    rows, w, b = _rows(a), fc.weight.detach().view(K, 64).cpu(), fc.bias.detach().cpu()
    flat = lab.cpu().reshape(-1)
    ref = reference(rows, w, b, flat, 1.0, wc, wd)
    tol = _bounds(rows, w, b, ref, K, B, CROP[0] * CROP[1] * CROP[2], dtype, 1.0, wc, wd)
    for name, g in (("loss", loss.detach().cpu()), ("sums", sums.cpu())):
        err = (g.double() - ref[name]).abs()
        print(f"[seg_mc model weights {dtype}] {name}: worst error / bound {float((err / tol[name].clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= tol[name]).all()), name
    for other in (reference(rows, w, b, flat, 1.0, wd, wc), reference(rows, w, b, flat, 1.0, 1.0, 1.0)):
        assert float((ref["loss"] - other["loss"]).abs()) > 100 * float(tol["loss"]), "these weights are told from the swapped and the unit ones"
    # the eval path
    _, eloss, esums, _ = model.infer(x, labels=lab)
    torch.cuda.synchronize()
    host = esums.cpu().tolist()
    want = loss_from_sums(host, K, wd=model.wd, head="softmax", wc=model.wc)
    mc = host[4 * K]
    terms = wc * sum(host[4 * k + 3] for k in range(K)) / mc + wd * 2.0
    assert mc > 0 and abs(float(eloss) - want) <= 2.0 ** -24 * abs(want) + 8 * 2.0 ** -53 * terms
    swapped, unit = loss_from_sums(host, K, wd=wc, head="softmax", wc=wd), loss_from_sums(host, K, head="softmax")
    assert abs(want - swapped) > 100 * 2.0 ** -23 * abs(want) and abs(want - unit) > 100 * 2.0 ** -23 * abs(want)


@_DTYPES
def test_infer_gives_the_label_map_counts_for_all_classes_and_the_argmax_of_its_logits(dtype):
    model = _model(dtype)
    x, lab = _batch()
    ci = torch.tensor([1, 0], dtype=torch.int32, device="cuda")
    counts = torch.zeros((2, K, 3), dtype=torch.int64, device="cuda")
    got, loss, sums, lm = model.infer(x, labels=lab, case_index=ci, counts=counts, want_mask=True)
    z = model.infer_logits(x)
    torch.cuda.synchronize()
    assert got is counts and lm.shape == lab.shape and lm.dtype == torch.uint8 and bool(torch.isfinite(loss)) and z.shape == (B, *CROP, K)
    m, l = lm.cpu(), lab.cpu()
    on = (l & 0x80) == 0
    assert int(m.max()) < K and not bool(m[~on].any()), "class indices, 0 where bit 7 is set"
    assert torch.equal(torch.where(on, lowest_argmax(z.cpu().double()).to(torch.uint8), torch.zeros_like(m)), m)
    want = torch.zeros((2, K, 3), dtype=torch.int64)
    for n in range(B):
        for k in range(K):
            p, g = (m[n] == k) & on[n], ((l[n] & 0x7F) == k) & on[n]
            want[int(ci[n]), k] = torch.tensor([int((p & g).sum()), int(p.sum()), int(g.sum())])
    assert torch.equal(counts.cpu(), want)
    # the accumulating store: twice the same pass, halved, is the plain logits
    buf = torch.empty_like(z)
    model.infer_logits(x, out=buf)
    model.infer_logits(x, out=buf, accumulate=True, scale=0.5)
    assert torch.equal(buf, z)
    with pytest.raises(ValueError, match="`out`, which is required"):
        model.infer_logits(x, flip=1)


def test_state_dict_is_the_reference_models_with_k_output_channels():
    model = Segmenter3d(K, head="softmax")
    assert len(model.state_dict()) == 169
    assert PCRLv23d(n_class=K).load_state_dict(model.state_dict()) is not None          # strict


def _seg3d(*argv, cwd):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "seg3d.py"), *argv], cwd=cwd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def _run(*argv, cwd):
    return subprocess.run([sys.executable, os.path.join(ROOT, "seg3d.py"), *argv], cwd=cwd, capture_output=True, text=True, timeout=300)


def test_train_predict_and_score_from_the_command_line_on_label_map_phantoms(tmp_path):
    """`seg3d.py train --data synthetic --head softmax` runs, its _best.pt names its head and loads into the reference's layout; `predict` takes the head
    from the checkpoint and writes label maps; the tiled prediction equals the sliding-window one at --overlap 0 with the constant window byte for byte
    (the weight is 1, so the argmax of num is the argmax of z); --mirror x and an ensemble run, the ensemble of a checkpoint with itself gives the single
    model's label map; an ensemble with a sigmoid checkpoint is refused; `score --labelmap` of a prediction identical to the ground truth gives Dice 1 and
    distances 0, and `score` without --labelmap refuses the directory."""
    cwd = str(tmp_path)
    out = str(tmp_path / "ck")
    common = ("--data", "synthetic", "--phase", "scratch", "--n_class", "4", "--crop", "16,16,8", "--b", "2", "--epochs", "1", "--steps_per_epoch", "2",
              "--save_best", "--workers", "0")
    log = _seg3d("train", *common, "--head", "softmax", "--output", out, cwd=cwd)
    assert "Test:" in log
    best = [f for f in os.listdir(out) if f.endswith("_best.pt")]
    assert len(best) == 1
    ckpt = os.path.join(out, best[0])
    ck = torch.load(ckpt, map_location="cpu", weights_only=False)
    assert ck["val"]["head"] == "softmax" and len(ck["state_dict"]) == 169 and len(ck["val"]["dice"]) == 3
    assert tuple(ck["state_dict"]["out_tr.final_conv.weight"].shape) == (4, 64, 1, 1, 1)
    data = str(tmp_path / "data")
    shape = (32, 16, 16)          # a multiple of the crop: at --overlap 0 every voxel lies in exactly one window, which is its tile
    D.write_synthetic(data, ["c0", "c1"], shape, 4, head="softmax", seed=5)
    with open(os.path.join(data, "test.txt"), "w") as f:
        f.write("c0\nc1\n")
    base = ("predict", "--data", data, "--list", "test.txt", "--crop", "16,16,8", "--b", "2")

    def predict(tag, weights, *extra):
        d = str(tmp_path / tag)
        _seg3d(*base, "--weights", weights, "--out", d, *extra, cwd=cwd)
        assert open(os.path.join(d, "head.txt")).read().strip() == "softmax"
        return d, [np.load(os.path.join(d, n + "_pred.npy")) for n in ("c0", "c1")]

    tiled_dir, tiled = predict("tiled", ckpt)
    for m in tiled:
        assert m.dtype == np.uint8 and m.shape == shape and int(m.max()) < 4
    # sliding windows at --overlap 0 are reached through an ensemble (or a mirror): a two-file ensemble of the checkpoint with itself
    _, twice = predict("twice", ckpt + "," + ckpt, "--window", "constant")
    _, mirrored = predict("mirror", ckpt, "--mirror", "x", "--probs")
    for a, b, c in zip(tiled, twice, mirrored):
        assert np.array_equal(a, b), "(z + z) * 0.5 == z: the ensemble with itself, blended at overlap 0 with weight 1, is the tiled label map"
        assert c.shape == shape and int(c.max()) < 4
    probs = np.load(os.path.join(str(tmp_path / "mirror"), "c0_prob.npy"))
    assert probs.shape == (4,) + shape and bool(np.all(np.abs(probs.astype(np.float64).sum(0) - 1.0) < 4 * 2.0 ** -11)), "[K,X,Y,Z] softmax probabilities (float16)"
    # a sigmoid checkpoint of the same sizes: mixed head kinds are refused, naming both files
    sig = str(tmp_path / "cksig")
    _seg3d("train", *common, "--output", sig, cwd=cwd)
    sig_ckpt = os.path.join(sig, [f for f in os.listdir(sig) if f.endswith("_best.pt")][0])
    r = _run(*base, "--weights", ckpt + "," + sig_ckpt, "--out", str(tmp_path / "mixed"), cwd=cwd)
    assert r.returncode != 0 and "was trained with --head sigmoid" in r.stderr and os.path.basename(sig_ckpt) in r.stderr
    # score: the ground truth as its own prediction
    same = str(tmp_path / "same")
    os.makedirs(same)
    for n in ("c0", "c1"):
        np.save(os.path.join(same, n + "_pred.npy"), np.load(os.path.join(data, n + "_seg.npy")))
    csv = str(tmp_path / "s.csv")
    _seg3d("score", "--data", data, "--list", "test.txt", "--pred", same, "--n_class", "4", "--labelmap", "--csv", csv, cwd=cwd)
    rows = [ln.strip().split(",") for ln in open(csv)][1:]
    assert [(r[0], r[1]) for r in rows] == [(n, str(k)) for n in ("c0", "c1") for k in (1, 2, 3)], "one row per (case, class 1..K-1)"
    assert all(float(r[2]) == 1.0 and float(r[3]) == 0.0 and float(r[4]) == 0.0 and float(r[5]) == 0.0 and int(r[7]) > 0 for r in rows)
    _seg3d("score", "--data", data, "--list", "test.txt", "--pred", tiled_dir, "--n_class", "4", "--labelmap", cwd=cwd)
    r = _run("score", "--data", data, "--list", "test.txt", "--pred", tiled_dir, "--n_class", "4", cwd=cwd)
    assert r.returncode != 0 and "pass --labelmap" in r.stderr
    r = _run("score", "--data", data, "--list", "test.txt", "--pred", same, "--n_class", "3", "--labelmap", cwd=cwd)
    assert r.returncode != 0 and "label value 3 but --n_class is 3" in r.stderr
    # the clean-up on label maps, from `predict` and from `postprocess`
    clean = str(tmp_path / "clean")
    _seg3d("postprocess", "--pred", tiled_dir, "--list", os.path.join(data, "test.txt"), "--out", clean, "--n_class", "4", "--labelmap", "--keep_largest", "all",
           cwd=cwd)
    _, kept = predict("kept", ckpt, "--keep_largest", "all")
    for n, m in zip(("c0", "c1"), kept):
        assert np.array_equal(np.load(os.path.join(clean, n + "_pred.npy")), m), "predict --keep_largest == predict, then postprocess --labelmap"
