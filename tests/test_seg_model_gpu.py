"""models.Segmenter3d, functions.UpConvsFn / SegHeadFn, train_seg and the seg3d command line on the GPU: crops 16x16x8 and 32x32x16, b = 2, K = 3."""
import hashlib
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
from pcrlv2_amd.optim import FusedSGD  # noqa: E402
from pcrlv2_amd.train_seg import loss_from_sums, train_step  # noqa: E402
from seg_reference import reference  # noqa: E402
from test_seg_head_gpu import _bounds  # noqa: E402

pytestmark = pytest.mark.gpu
K, B = 3, 2
CROPS = [(16, 16, 8), (32, 32, 16)]
_DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
_CROPS = pytest.mark.parametrize("crop", CROPS, ids=["16x16x8", "32x32x16"])
HEAD_PARTS = (".bn.", ".predictor_head.", ".deep_supervision_head.")


def _bits(t):
    return t.detach().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32 if t.dtype == torch.float32 else torch.int64).cpu()


def _model(dtype, seed=0):
    torch.manual_seed(seed)
    return Segmenter3d(K).cuda().train().set_compute_dtype(dtype)


def _batch(crop, seed=0):
    """(x [B,1,*crop] float32, labels uint8 [B,*crop] with some voxels not counted) from the phantoms, on the device."""
    cases = [D.synthetic_case(seed, i, crop, K) for i in range(B)]
    x = torch.from_numpy(np.stack([c.img for c in cases])).cuda()
    lab = torch.from_numpy(np.stack([c.seg for c in cases]))
    lab[:, :2] |= 0x80
    return x, lab.cuda()


def _fresh_step():
    ops.begin_step()
    Fn.reset_parked()


@_CROPS
@_DTYPES
def test_decoder_stage_without_heads_gives_the_stage_output_bit_for_bit(dtype, crop):
    model = _model(dtype)
    g = torch.Generator().manual_seed(1)
    for name, c, shrink in (("up_tr256", 512, 8), ("up_tr128", 256, 4), ("up_tr64", 128, 2)):
        up = getattr(model, name)
        x = ops.to_act(torch.relu(torch.randn((B, c) + tuple(s // shrink for s in crop), generator=g)).cuda(), dtype)
        _fresh_step()
        full = up(x)[0]
        ops.end_of_forward_join()
        lu = lambda m: (m.conv1.weight, m.conv1.bias, m.bn1.weight, m.bn1.bias)      # noqa: E731
        _fresh_step()
        mine = Fn.UpConvsFn.apply(x, up.up_conv.weight, up.up_conv.bias, *lu(up.ops[0]), *lu(up.ops[1]), up)
        torch.cuda.synchronize()
        assert mine.dtype == full.dtype and torch.equal(_bits(mine), _bits(full)), name


@_CROPS
@_DTYPES
def test_decoder_stage_backward_equals_the_full_stage_with_only_its_first_output_used(dtype, crop):
    """UpStageFn's backward with d_pro = d_pre = d_mask = None is the convolutions' backward alone: dx and the ten convolution gradients of
    UpConvsFn must be bit-identical to it."""
    model = _model(dtype)
    for p in model.parameters():
        p.requires_grad_(True)          # the full stage's node takes the head parameters too (they get no gradient: their outputs are unused)
    g = torch.Generator().manual_seed(2)
    lu = lambda m: (m.conv1.weight, m.conv1.bias, m.bn1.weight, m.bn1.bias)      # noqa: E731
    for name, c, shrink in (("up_tr256", 512, 8), ("up_tr128", 256, 4), ("up_tr64", 128, 2)):
        up = getattr(model, name)
        convs = (up.up_conv.weight, up.up_conv.bias) + lu(up.ops[0]) + lu(up.ops[1])
        shape = (B, c) + tuple(s // shrink for s in crop)
        x0 = ops.to_act(torch.relu(torch.randn(shape, generator=g)).cuda(), dtype)
        d = ops.to_act(torch.randn((B, up.ops[1].conv1.out_channels) + tuple(2 * s // shrink for s in crop), generator=g).cuda(), dtype)
        got = []
        for which in ("full", "convs"):
            for p in up.parameters():
                p.grad = None
            x = x0.clone().requires_grad_(True)
            _fresh_step()
            up._pass_idx = ops.next_pass()
            if which == "full":
                out = up(x)[0]
            else:
                out = Fn.UpConvsFn.apply(x, *convs, up)
            ops.end_of_forward_join()
            out.backward(d)
            torch.cuda.synchronize()
            got.append([x.grad.clone()] + [p.grad.clone() for p in convs])
            if which == "full":
                assert all(p.grad is None for n, p in up.named_parameters() if any(h in "." + n for h in HEAD_PARTS)), name
        for i, (a, b) in enumerate(zip(*got)):
            assert a.dtype == b.dtype and torch.equal(_bits(a), _bits(b)), f"{name}: gradient {i} (0 = dx, then up_conv.weight, up_conv.bias, ops.0, ops.1)"


@_CROPS
@_DTYPES
def test_loss_backward_equals_the_seam_done_by_hand(dtype, crop):
    model = _model(dtype)
    x, lab = _batch(crop)
    params = dict(model.named_parameters())
    _fresh_step()
    loss, sums = model.loss(x, lab)
    loss.backward()
    torch.cuda.synchronize()
    first = {n: p.grad.clone() for n, p in params.items() if p.grad is not None}
    assert set(first) == {n for n, p in params.items() if p.requires_grad} and not any(h in n for n in first for h in HEAD_PARTS)
    for p in params.values():
        p.grad = None
    _fresh_step()
    a1 = model.features(x)
    fc = model.out_tr.final_conv
    l2, s2 = ops.seg_head_forward(a1.detach(), fc.weight, fc.bias, lab, dtype)
    dx, dw, db = ops.seg_head_backward(a1.detach(), fc.weight, fc.bias, lab, s2, torch.ones((), device="cuda"), dtype)
    ops.end_of_forward_join()
    a1.backward(dx)
    torch.cuda.synchronize()
    assert torch.equal(_bits(l2), _bits(loss)) and torch.equal(s2.cpu(), sums.cpu())
    for n, p in params.items():
        if n == "out_tr.final_conv.weight":
            got = dw.view(p.shape)
        elif n == "out_tr.final_conv.bias":
            got = db
        else:
            got = p.grad
        if n in first:
            assert got is not None and torch.equal(_bits(got), _bits(first[n])), n
        else:
            assert got is None, n


@_DTYPES
def test_the_models_loss_weights_reach_the_training_loss_and_the_eval_loss(dtype):
    """Segmenter3d(wb=0.25, wd=2.0): model.loss is the raw forward with THESE weights on the model's own features bit for bit and the float64
    restatement with them within tests/test_seg_head_gpu.py's bound (a swap, or the defaults, is far outside it); infer's loss is
    train_seg.loss_from_sums of infer's sums with the model's weights, to the float32 rounding of the device value (the device evaluates the same
    float64 expression, possibly with one fused multiply-add: 8 x 2^-53 of the terms, then half a float32 ulp)."""
    wb, wd, crop = 0.25, 2.0, CROPS[0]
    torch.manual_seed(0)
    model = Segmenter3d(K, wb=wb, wd=wd).cuda().train().set_compute_dtype(dtype)
    assert (model.wb, model.wd) == (wb, wd)
    x, lab = _batch(crop)
    _fresh_step()
    loss, sums = model.loss(x, lab)
    loss.backward()
    torch.cuda.synchronize()
    _fresh_step()
    with torch.no_grad():
        a = ops.to_act(model.features(x), dtype)
        ops.end_of_forward_join()
    fc = model.out_tr.final_conv
    l2, s2 = ops.seg_head_forward(a, fc.weight, fc.bias, lab, dtype, wb, wd)
    torch.cuda.synchronize()
    assert torch.equal(_bits(l2), _bits(loss)) and torch.equal(s2.cpu(), sums.cpu())
    rows, w, b = a.detach().permute(0, 2, 3, 4, 1).reshape(-1, 64).cpu(), fc.weight.detach().view(K, 64).cpu(), fc.bias.detach().cpu()
    flat = lab.cpu().reshape(-1)
    ref = reference(rows, w, b, flat, 1.0, wb, wd)
    tol = _bounds(rows, w, b, ref, K, B, crop[0] * crop[1] * crop[2], dtype, 1.0, wb, wd)
    for name, g in (("loss", loss.detach().cpu()), ("sums", sums.cpu())):
        err = (g.double() - ref[name]).abs()
        print(f"[seg model weights {dtype}] {name}: worst error / bound {float((err / tol[name].clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= tol[name]).all()), name
    for other in (reference(rows, w, b, flat, 1.0, wd, wb), reference(rows, w, b, flat, 1.0, 1.0, 1.0)):
        assert float((ref["loss"] - other["loss"]).abs()) > 100 * float(tol["loss"]), "these weights are told from the swapped and the unit ones"
    # the eval path
    _, eloss, esums, _ = model.infer(x, labels=lab)
    torch.cuda.synchronize()
    host = esums.cpu().tolist()
    want = loss_from_sums(host, K, model.wb, model.wd)
    mc = host[4 * K]
    terms = wb * sum(host[4 * k + 3] for k in range(K)) / (mc * K) + wd * 2.0
    assert mc > 0 and abs(float(eloss) - want) <= 2.0 ** -24 * abs(want) + 8 * 2.0 ** -53 * terms
    assert abs(want - loss_from_sums(host, K, wd, wb)) > 100 * 2.0 ** -23 * abs(want) and abs(want - loss_from_sums(host, K)) > 100 * 2.0 ** -23 * abs(want)


@_CROPS
@_DTYPES
def test_one_step_moves_what_the_loss_reaches_and_nothing_of_the_heads(dtype, crop):
    model = _model(dtype)
    # weight decay > 0: a convolution bias in front of a BatchNorm has an exactly zero gradient and moves by its decay alone
    opt = FusedSGD(model.trainable_parameters(), lr=0.1, momentum=0.9, weight_decay=1e-2)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    x, lab = _batch(crop)
    loss, _ = train_step(model, opt, (x.cpu(), lab.cpu()))
    after = model.state_dict()
    assert bool(torch.isfinite(loss))
    trainable = {n for n, p in model.named_parameters() if p.requires_grad}
    for k, v in before.items():
        is_head = any(h in k for h in HEAD_PARTS)
        if is_head:
            assert torch.equal(v, after[k]), f"{k}: a head's parameter, statistic or counter moved"
        elif k in trainable:
            assert not torch.equal(v, after[k]), f"{k}: a parameter the loss reaches did not change"
        elif k.endswith("num_batches_tracked"):
            assert int(after[k]) == int(v) + 1, k
        else:
            assert not torch.equal(v, after[k]), f"{k}: a running statistic of a layer that ran did not move"
    assert len(trainable) + sum(1 for n, _ in model.named_parameters() if any(h in "." + n for h in HEAD_PARTS)) == len(list(model.parameters()))


def _digest(model):
    h = hashlib.sha256()
    for k, v in model.state_dict().items():
        h.update(k.encode())
        h.update(v.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


@_CROPS
@_DTYPES
def test_infer_leaves_the_model_alone_and_counts_match_its_mask(dtype, crop):
    model = _model(dtype)
    x, lab = _batch(crop)
    before = _digest(model)
    ci = torch.tensor([1, 0], dtype=torch.int32, device="cuda")
    counts = torch.zeros((2, K, 3), dtype=torch.int64, device="cuda")
    got, loss, sums, mask = model.infer(x, labels=lab, case_index=ci, counts=counts, want_mask=True)
    torch.cuda.synchronize()
    assert _digest(model) == before and model.training and got is counts
    assert mask.shape == lab.shape and mask.dtype == torch.uint8 and bool(torch.isfinite(loss))
    m, l = mask.cpu(), lab.cpu()
    assert not bool(m[(l & 0x80) != 0].any()), "the mask is 0 where bit 7 is set"
    want = torch.zeros((2, K, 3), dtype=torch.int64)
    for n in range(B):
        on = (l[n] & 0x80) == 0
        for k in range(K):
            p, g = ((m[n] >> k) & 1).bool() & on, ((l[n] >> k) & 1).bool() & on
            want[int(ci[n]), k] = torch.tensor([int((p & g).sum()), int(p.sum()), int(g.sum())])
    assert torch.equal(counts.cpu(), want)
    assert float(sums[4 * K]) == float(((l & 0x80) == 0).sum())
    # without labels: every voxel counted, nothing labelled
    c2 = model.infer(x)[0].cpu()
    assert int(c2[:, :, 2].sum()) == 0 and c2.shape == (B, K, 3)


def test_state_dict_keys_are_the_reference_manifest():
    keys = [ln.split()[0] for ln in open(os.path.join(ROOT, "tests", "golden", "state_dict_manifest.txt"))]
    model = Segmenter3d(K)
    assert list(model.state_dict().keys()) == keys and len(keys) == 169
    assert PCRLv23d(n_class=K).load_state_dict(model.state_dict()) is not None          # strict
    with pytest.raises(ValueError):
        Segmenter3d(8)
    with pytest.raises(RuntimeError, match="no forward"):
        model(torch.zeros(1, 1, 16, 16, 8))


def test_load_pretrained_takes_a_pretraining_checkpoint_with_two_announced_exceptions(tmp_path, capsys):
    torch.manual_seed(3)
    pre = PCRLv23d()
    sd = pre.state_dict()
    path = str(tmp_path / "pre.pt")
    torch.save({"state_dict": {"module." + k: v for k, v in sd.items()}, "epoch": 0}, path)
    torch.manual_seed(4)
    model = Segmenter3d(K, in_channels=2)
    fresh = {k: v.clone() for k, v in model.state_dict().items()}
    model.load_pretrained(path)
    out = capsys.readouterr().out
    mine = model.state_dict()
    announced = ("out_tr.final_conv.weight", "out_tr.final_conv.bias", "down_tr64.ops.0.conv1.weight")
    for k in announced:
        assert torch.equal(mine[k], fresh[k]) and (k + ":") in out, k
    assert out.count("freshly initialised") == 3
    for k in sd:
        if k not in announced:
            assert torch.equal(mine[k], sd[k]), k
    same = Segmenter3d(1, weights=path)                       # nothing differs: nothing is announced, everything is loaded
    assert all(torch.equal(v, sd[k]) for k, v in same.state_dict().items())
    renamed = dict(sd)
    renamed["up_tr64.ops.1.conv1.wieght"] = renamed.pop("up_tr64.ops.1.conv1.weight")
    torch.save({"state_dict": renamed}, path)
    with pytest.raises(KeyError, match="up_tr64.ops.1.conv1"):
        Segmenter3d(K).load_pretrained(path)
    bad = dict(sd)
    bad["up_tr128.ops.0.conv1.weight"] = bad["up_tr128.ops.0.conv1.weight"][:, :100].clone()
    torch.save({"state_dict": bad}, path)
    with pytest.raises(KeyError, match="up_tr128.ops.0.conv1.weight"):
        Segmenter3d(K).load_pretrained(path)


def test_thirty_steps_on_one_fixed_batch_lower_the_loss():
    model = _model(torch.float32, seed=5)
    opt = FusedSGD(model.trainable_parameters(), lr=1e-2, momentum=0.9, weight_decay=1e-4)
    x, lab = _batch((32, 32, 16), seed=2)
    batch = (x.cpu(), lab.cpu())
    losses = torch.stack([train_step(model, opt, batch)[0] for _ in range(30)]).cpu()
    print("[seg fixed batch] loss", " ".join("%.4f" % v for v in losses.tolist()))
    assert bool(torch.isfinite(losses).all()) and float(losses[-1]) < float(losses[0])


def _cli(*argv, timeout=300):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "seg3d.py"), *argv], cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_train_end_to_end_then_predict(tmp_path):
    out_dir = str(tmp_path / "out")
    log = _cli("train", "--data", "synthetic", "--phase", "scratch", "--epochs", "2", "--steps_per_epoch", "3", "--b", "2", "--crop", "32,32,16", "--save_best",
               "--output", out_dir)
    assert log.count("Val: [") == 3 and "mean Dice" in log and log.count("Test: (") == 1, log[-2000:]       # epochs 0, 1, 2 (inclusive upper bound)
    best = os.path.join(out_dir, "pcrlv2_seg3d_scratch_1.0_best.pt")
    assert os.path.exists(best)
    ckpt = torch.load(best, map_location="cpu", weights_only=False)
    PCRLv23d(n_class=3).load_state_dict(ckpt["state_dict"])               # strict: the reference's class takes the fine-tuned checkpoint
    assert ckpt["val"]["mean_dice"] == ckpt["val"]["mean_dice"]
    # predict on two cases whose size is no multiple of the crop
    data = str(tmp_path / "data")
    D.write_synthetic(data, ["p0", "p1"], (40, 36, 20), 3, seed=9)
    with open(os.path.join(data, "two.txt"), "w") as f:
        f.write("p0\np1\n")
    pred = str(tmp_path / "pred")
    _cli("predict", "--data", data, "--list", "two.txt", "--weights", best, "--out", pred, "--crop", "32,32,16", "--b", "4")
    from pcrlv2_amd.train_seg import load_segmenter
    model = load_segmenter(best, torch.device("cuda"))
    crop = (32, 32, 16)
    for name in ("p0", "p1"):
        m = np.load(os.path.join(pred, name + "_pred.npy"))
        assert m.shape == (40, 36, 20) and m.dtype == np.uint8 and int(m.max()) < 8
        # the stitching, redone another way: every tile predicted whole (no label, nothing masked), laid down in tile order, a voxel keeps the
        # FIRST tile's value -- the tile that counts it
        case = D.open_case(data, name, 3, 1)
        want, written = np.zeros(case.shape, dtype=np.uint8), np.zeros(case.shape, dtype=bool)
        starts = [st for st, _ in D.tiles(case.shape, crop)]
        xs = np.stack([D.cut(case, st, crop)[0] for st in starts])
        masks = torch.cat([model.infer(torch.from_numpy(xs[i:i + 4]).cuda(), want_mask=True)[3] for i in range(0, len(starts), 4)]).cpu().numpy()   # predict's batches
        for start, tile in zip(starts, masks):
            box = tuple(slice(s, min(s + c, n)) for s, c, n in zip(start, crop, case.shape))
            inner = tuple(slice(0, sl.stop - sl.start) for sl in box)
            new = ~written[box]
            want[box][new] = tile[inner][new]
            written[box] = True
        assert written.all() and np.array_equal(m, want), name
    with pytest.raises(SystemExit, match="no such file"):
        load_segmenter(os.path.join(out_dir, "absent.pt"), torch.device("cuda"))
