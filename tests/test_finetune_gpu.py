"""Supervised 2D fine-tuning on the GPU: the evaluation transform against Pillow, ChestClassifier's fused head against the same encoder followed by
torch's head, infer against the eval-mode forward, a learning check, the best-checkpoint round trip and the encoder's key names."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import chest_aug_reference as R  # noqa: E402
from pcrlv2_amd import data_chest as DC  # noqa: E402
from pcrlv2_amd import functions as Fn  # noqa: E402
from pcrlv2_amd import ops  # noqa: E402
from pcrlv2_amd.models import ChestClassifier, PCRLv2  # noqa: E402

pytestmark = pytest.mark.gpu
U, ULP = 2.0 ** -24, 2.0 ** -23
S = DC.GLOBAL_SIZE


# ---------------------------------------------------------------------------------------------------------------
# the evaluation transform: Resize((224, 224)) -> ToTensor -> Normalize through the pre-task's two spatial kernels
# ---------------------------------------------------------------------------------------------------------------
def _sources():
    rng = np.random.default_rng(3)
    smooth = lambda h, w, c: np.clip(np.add.outer(np.arange(h) * 3.1, np.arange(w) * 1.7)[..., None] + rng.integers(0, 90, (h, w, c)), 0, 255).astype(np.uint8)
    return [smooth(37, 53, 1), smooth(64, 64, 1), smooth(45, 61, 3)]


def _pillow_resize(src):
    from PIL import Image
    im = Image.fromarray(src[..., 0] if src.shape[2] == 1 else src)
    return np.array(im.convert("RGB").resize((S, S), Image.BILINEAR), dtype=np.uint8)


@pytest.mark.parametrize("idx", [0, 1, 2], ids=["37x53", "64x64", "45x61x3"])
def test_eval_transform_equals_pillow_resize(idx):
    src = _sources()[idx]
    H, W, C = src.shape
    ref = _pillow_resize(src)                                                          # [S, S, 3]
    # on the CPU first: an angle-0 record is the identity in the restatement, and the restatement's whole-image crop + resize is Pillow's resize
    rec = DC.eval_records(np.array([[H, W, C]]))
    base = R.crop_resize(src, 0, 0, H, W, S)
    assert np.array_equal(R.rotate_nearest(base, rec[0, DC.P_A0:DC.P_A5 + 1]), base)
    assert np.array_equal(np.repeat(base, 3, axis=2) if C == 1 else base, ref)
    DC.pack_offsets(rec, [0], np.zeros(1, np.int64), S)
    dev = torch.device("cuda")
    view, x = DC.apply_spatial(torch.from_numpy(src.reshape(-1).copy()).to(dev), torch.from_numpy(rec.astype(np.int32)).to(dev), rec, S)
    torch.cuda.synchronize()
    got = view[0, :C].cpu().numpy()
    assert np.array_equal(got, np.moveaxis(ref, 2, 0)[:C]), f"{int((got != np.moveaxis(ref, 2, 0)[:C]).sum())} pixels differ from Pillow"
    want = (torch.from_numpy(np.moveaxis(ref, 2, 0).copy()).float() / 255.0 - torch.tensor(R.MEAN).view(3, 1, 1)) / torch.tensor(R.STD).view(3, 1, 1)
    assert torch.equal(x[0].cpu().view(torch.int32), want.view(torch.int32))


def test_labelled_augment_object_eval_and_train():
    srcs = _sources()
    cap = max(s.size for s in srcs)
    pix = torch.zeros((3, cap), dtype=torch.uint8)
    lab = np.array([[1, 0, 1, 1], [0, 0, 0, 0], [1, 1, 1, 1]], np.uint8)
    rec = torch.zeros((3, 4), dtype=torch.int32)
    for n, s in enumerate(srcs):
        pix[n, :s.size] = torch.from_numpy(s.reshape(-1).copy())
        rec[n] = torch.tensor(tuple(s.shape) + (int(DC.pack_labels(lab[n:n + 1])[0]),), dtype=torch.int32)
    ev = DC.GpuChestLabelledAugment("cuda", 0, 4, train=False)
    x, y = ev(pix, rec)
    torch.cuda.synchronize()
    assert x.shape == (3, 3, S, S) and x.dtype == torch.float32 and y.is_cuda and y.dtype == torch.uint8 and np.array_equal(y.cpu().numpy(), lab)
    for n, s in enumerate(srcs):
        assert np.array_equal(x[n].cpu().numpy().view(np.int32), R.normalize(_pillow_resize(s)).view(np.int32))
    # training transform: the pre-task's un-jittered target of the same draws (chest_aug_reference.view), labels untouched
    tr = DC.GpuChestLabelledAugment("cuda", 5, 4, train=True)
    x, y = tr(pix, rec)
    torch.cuda.synchronize()
    assert np.array_equal(y.cpu().numpy(), lab)
    tr.reset_rng(5)
    recs, _, _ = tr.records(rec.numpy()[:, :3])
    for n, s in enumerate(srcs):
        assert np.array_equal(x[n].cpu().numpy().view(np.int32), R.view(s, recs[n], S)[1].view(np.int32))


def test_finetune_loaders_on_a_directory_of_pngs(tmp_path, monkeypatch):
    """chest_finetune_loaders end to end: PNGs decoded by a worker into the shared slots, the labels riding in the slot record, the last 1 - ratio of the
    training list shuffled through the training transform, the held-out lists in order through the evaluation transform; 'test' built on first use."""
    from PIL import Image
    from pcrlv2_amd import main as M
    rng = np.random.default_rng(9)
    (tmp_path / "imgs").mkdir()
    (tmp_path / "train_val_txt").mkdir()
    srcs, lab = {}, {}
    for split, n in (("train", 8), ("valid", 3)):
        with open(tmp_path / "train_val_txt" / f"chest_{split}.txt", "w") as f:
            for i in range(n):
                name = f"{split}_{i}.png"
                a = rng.integers(0, 256, (40 + 3 * i, 48), dtype=np.uint8)
                Image.fromarray(a).save(tmp_path / "imgs" / name)
                y = rng.integers(0, 2, 14)
                y[i % 14] = 1
                f.write(name + " " + " ".join(str(int(v)) for v in y) + "\n")
                srcs[name], lab[name] = a[..., None], y.astype(np.uint8)
    monkeypatch.chdir(tmp_path)
    args = M.build_parser().parse_args(["--data", str(tmp_path / "imgs"), "--d", "2", "--phase", "scratch", "--b", "2", "--workers", "1", "--ratio", "0.5",
                                        "--gpus", "0", "--output", str(tmp_path / "out")])
    loaders = M.get_dataloader(args)
    try:
        train = list(loaders["train"])
        assert len(train) == 2 and all(x.shape == (2, 3, S, S) and x.dtype == torch.float32 and y.dtype == torch.uint8 and y.is_cuda for x, y in train)
        got = sorted(tuple(r) for _, y in train for r in y.cpu().tolist())
        assert got == sorted(tuple(lab[f"train_{i}.png"].tolist()) for i in range(4, 8))          # the LAST half of the list, each image once
        ev = list(loaders["eval"])
        assert [x.shape[0] for x, _ in ev] == [2, 1]
        xs, ys = torch.cat([x for x, _ in ev]).cpu().numpy(), torch.cat([y for _, y in ev]).cpu().numpy()
        for i in range(3):
            name = f"valid_{i}.png"
            assert np.array_equal(ys[i], lab[name])
            assert np.array_equal(xs[i].view(np.int32), R.normalize(_pillow_resize(srcs[name])).view(np.int32))
        with pytest.raises(SystemExit, match="chest_test.txt"):
            loaders["test"]
    finally:
        for k in ("train", "eval"):
            ld = dict.get(loaders, k)
            if ld is not None:
                ld.close()


# ---------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------
def _model(dropout=0.0, seed=0, n_class=14):
    torch.manual_seed(seed)
    m = ChestClassifier(n_class=n_class, dropout=dropout).cuda()
    m.set_compute_dtype(torch.float32)
    with torch.no_grad():          # a head that is not at its all-zero-bias start: every logit differs
        m.classification_head[3].bias.normal_(0.0, 0.5)
    return m


def _batch(b, size, n_class, seed):
    from pcrlv2_amd.main import SyntheticLabelledChestLoader
    ld = SyntheticLabelledChestLoader(b, 1, size, n_class, seed=seed, device="cuda")
    return next(iter(ld))


def _head_bounds(h, w, b, y, probs):
    """The derived bounds of tests/test_cls_head_gpu.py for one side (no dropout) -> (loss bound, dp [N,K], d_a bound [N,C] per pixel, dW bound [K,C])."""
    N, C, H, W = h.shape
    HW, K = H * W, w.shape[0]
    mean_abs = h.double().abs().mean((2, 3))
    e_z = (C + HW + 8) * U * (mean_abs @ w.double().abs().t() + b.double().abs())
    dp = e_z / 4 + 4 * ULP * probs.double()
    c = 1.0 / (N * K)
    dz = (probs.double() - y.double()).abs() * c
    row = ((K + 8) * U * (dz @ w.double().abs()) + (dp * c) @ w.double().abs()) / HW
    pooled = h.double().mean((2, 3)).abs()
    dw = (N + 8) * U * (dz.t() @ pooled) + (dp * c).t() @ pooled + dz.t() @ ((HW + 8) * U * mean_abs)
    return e_z.mean(), dp, row, dw


def test_fused_head_against_the_same_encoder_with_torchs_head():
    """ChestClassifier.loss (one head node) vs encoder.forward_last + torch's mean / linear / sigmoid / binary_cross_entropy on the GPU.  Both sides run
    the same encoder kernels on the same input, so the encoder's output is the same bit for bit and the two differ by the head arithmetic only: each
    side is within the derived bound of the exact value, the difference within twice it.  Convolution weights: the encoder's backward is linear in d_a,
    so the relative difference of d_a in the 2-norm is propagated as a relative bound on the gradient's norm."""
    m = _model()
    m.train()
    x, y = _batch(4, 64, 14, seed=1)
    lin = m.classification_head[3]
    names = ("encoder.conv1.weight", "encoder.layer4.1.conv2.weight", "classification_head.3.weight")
    params = dict(m.named_parameters())

    def grads():
        torch.cuda.synchronize()
        out = {n: params[n].grad.detach().double().clone() for n in names}
        for p in m.parameters():
            p.grad = None
        return out

    ops.begin_step()
    Fn.reset_parked()
    loss, probs = m.loss(x, y)
    loss.backward()
    g_fused = grads()

    ops.begin_step()
    Fn.reset_parked()
    h = m.encoder.forward_last(x)
    h.retain_grad()
    pr = torch.sigmoid(F.linear(h.float().mean((2, 3)), lin.weight, lin.bias))
    loss_t = F.binary_cross_entropy(pr, y.float())
    loss_t.backward()
    d_a = h.grad.detach().double()
    g_torch = grads()

    loss_b, dp, row, dw_b = _head_bounds(h.detach(), lin.weight.detach(), lin.bias.detach(), y, pr.detach())
    d_loss = abs(float(loss) - float(loss_t))
    print(f"[fused vs composed] loss {float(loss):.7f} vs {float(loss_t):.7f}: |d| {d_loss:.3e}, bound {2 * float(loss_b + 4 * ULP * float(loss_t)):.3e}")
    assert d_loss <= 2 * float(loss_b + 4 * ULP * abs(float(loss_t)))
    assert bool(((probs.double() - pr.double()).abs() <= 2 * dp).all())
    n = "classification_head.3.weight"
    err = (g_fused[n] - g_torch[n]).abs()
    print(f"[fused vs composed] dW: worst error / bound {float((err / (2 * dw_b)).max()):.3f}")
    assert bool((err <= 2 * dw_b).all())
    HW = h.shape[2] * h.shape[3]
    rel = 2 * float((row.pow(2).sum() * HW).sqrt()) / float(d_a.norm())
    for n in names[:2]:
        r = float((g_fused[n] - g_torch[n]).norm() / g_torch[n].norm())
        print(f"[fused vs composed] {n}: relative difference {r:.3e}, bound {rel:.3e}")
        assert r <= rel, n


def test_infer_equals_eval_forward_touches_nothing_builds_no_graph():
    m = _model(dropout=0.2)
    x, y = _batch(4, 64, 14, seed=2)
    m.train()
    ops.begin_step()
    Fn.reset_parked()
    m.loss(x, y)                                  # running statistics that are not the initial ones
    m.eval()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with torch.enable_grad():
        p_inf = m.infer(x)
        p_inf2, loss_inf = m.infer(x, labels=y)
    p_fwd = m(x)
    torch.cuda.synchronize()
    assert not p_inf.requires_grad and p_inf.grad_fn is None and not loss_inf.requires_grad
    assert torch.equal(p_inf, p_inf2)
    after = m.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before), "infer or the eval forward changed the model"
    # the bound of the head for the activation this side saw; the two encoder routes (fused epilogues vs separate passes) add their own float32 roundings
    # to that activation, which the bound's 512-term slack is derived to cover only if they are of rounding size -- so measure and report first
    from pcrlv2_amd.models.pcrlv2_model import encoder_eval
    h = encoder_eval(m.encoder, x, torch.float32)
    lin = m.classification_head[3]
    _, dp, _, _ = _head_bounds(h, lin.weight.detach(), lin.bias.detach(), y, p_fwd)
    err = (p_inf.double() - p_fwd.double()).abs()
    print(f"[infer vs eval forward] worst |dp| {float(err.max()):.3e}, worst error / bound {float((err / (2 * dp)).max()):.3f}")
    assert bool((err <= 2 * dp).all())
    ref_loss = F.binary_cross_entropy(p_fwd.double(), y.double())
    assert abs(float(loss_inf) - float(ref_loss)) <= 2 * float(dp.mean() * 4) + 8 * ULP * float(ref_loss)
    m.train()
    assert m.training and m(x).shape == (4, 14)


def test_learning_check_and_evaluate():
    from pcrlv2_amd.optim import FusedSGD
    from pcrlv2_amd.train_finetune import evaluate, train_step
    m = _model(seed=3)
    m.train()
    x, y = _batch(8, 64, 14, seed=4)
    opt = FusedSGD(m.parameters(), lr=1e-2, momentum=0.9, weight_decay=1e-4)
    losses = [train_step(m, opt, (x, y))[0] for _ in range(40)]
    losses = [float(l) for l in losses]
    print(f"[learning check] loss {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert all(math.isfinite(l) for l in losses) and losses[-1] < losses[0]
    out = evaluate(m, [(x, y)])
    assert out["n"] == 8 and math.isfinite(out["loss"]) and len(out["auroc"]) == 14
    both = (y.sum(0) > 0) & (y.sum(0) < 8)
    assert bool(both.any())
    for k in range(14):
        assert math.isfinite(out["auroc"][k]) == bool(both[k]) and (not bool(both[k]) or 0.0 <= out["auroc"][k] <= 1.0)
    assert math.isfinite(out["mean_auroc"])
    assert evaluate(m, [(x, y)]) == out, "two passes on the same weights and data differ"
    assert m.training


def test_best_checkpoint_round_trip(tmp_path, capsys):
    from pcrlv2_amd import main as M
    from pcrlv2_amd.train_finetune import evaluate, train_chest_classifier
    argv = ["--data", "synthetic", "--d", "2", "--phase", "scratch", "--b", "4", "--epochs", "1", "--steps_per_epoch", "3", "--size2d", "64", "--gpus", "0",
            "--save_best", "--lr", "1e-2", "--output", str(tmp_path)]
    args = M.build_parser().parse_args(argv)
    train_chest_classifier(args, M.get_dataloader(args))
    text = capsys.readouterr().out
    vals = re.findall(r"Val: \[(\d+)\]\tloss ([\d.]+)\tmean AUROC ([\d.]+)", text)
    assert [v[0] for v in vals] == ["0", "1"] and re.search(r"Test: \((best|last) epoch \d\)\tloss [\d.]+\tmean AUROC [\d.]+", text), text
    best = tmp_path / "pcrlv2_luna_scratch_0.8_best.pt"
    assert best.exists() and (tmp_path / "pcrlv2_luna_scratch_0.8_1.pt").exists()
    ck = torch.load(str(best), map_location="cpu", weights_only=False)
    assert set(ck) == {"epoch", "state_dict", "val"}
    assert "%.4f" % ck["val"]["mean_auroc"] == vals[ck["epoch"]][2] and float(vals[ck["epoch"]][2]) == max(float(v[2]) for v in vals)
    fresh = ChestClassifier(n_class=14, dropout=0.2).cuda()
    fresh.load_state_dict(ck["state_dict"], strict=True)
    out = evaluate(fresh, M.get_dataloader(args)["eval"])
    assert out["mean_auroc"] == ck["val"]["mean_auroc"] and out["auroc"] == ck["val"]["auroc"] and out["n"] == ck["val"]["n"] == 12


def test_resume_restores_model_momentum_and_epoch(tmp_path, capsys):
    from pcrlv2_amd import main as M
    from pcrlv2_amd.train_finetune import train_chest_classifier
    base = ["--data", "synthetic", "--d", "2", "--phase", "scratch", "--b", "4", "--steps_per_epoch", "2", "--size2d", "64", "--gpus", "0", "--lr", "1e-2",
            "--output", str(tmp_path)]
    args = M.build_parser().parse_args(base + ["--epochs", "1"])
    train_chest_classifier(args, M.get_dataloader(args))
    capsys.readouterr()
    last = str(tmp_path / "pcrlv2_luna_scratch_0.8_1.pt")
    ck = torch.load(last, map_location="cpu", weights_only=False)
    assert ck["epoch"] == 1 and "classification_head.3.weight" in ck["state_dict"]
    bufs = [st["momentum_buffer"] for st in ck["optimizer"]["state"].values()]
    assert len(bufs) == len(ck["optimizer"]["param_groups"][0]["params"]) and any(float(b.abs().max()) > 0 for b in bufs)
    # an untrained model evaluates differently from the resumed one; the resumed run trains epoch 2 only
    args = M.build_parser().parse_args(base + ["--epochs", "2", "--resume", last])
    seen = {}
    import pcrlv2_amd.train_finetune as TF
    real = TF.train_inner

    def spy(a, epoch, loader, model, optimizer, verbose=True):
        if not seen:
            seen["epoch"] = epoch
            sd = model.state_dict()
            seen["model"] = all(torch.equal(sd[k].cpu(), ck["state_dict"][k]) for k in ck["state_dict"])
            i = len(optimizer._plist) - 2                              # classification_head.3.weight
            o, n = optimizer._offsets_host[i], optimizer._plist[i].numel()
            seen["momentum"] = torch.equal(optimizer.flat_buf[o:o + n].cpu(), ck["optimizer"]["state"][i]["momentum_buffer"].reshape(-1))
        return real(a, epoch, loader, model, optimizer, verbose)

    TF.train_inner = spy
    try:
        train_chest_classifier(args, M.get_dataloader(args))
    finally:
        TF.train_inner = real
    text = capsys.readouterr().out
    assert seen == {"epoch": 2, "model": True, "momentum": True}, seen
    assert "continuing with epoch 2" in text and re.findall(r"Val: \[(\d+)\]", text) == ["2"]


def test_encoder_keys_interchange_with_the_2d_pretraining_checkpoint(tmp_path):
    pre = PCRLv2()
    cls = ChestClassifier()
    saved = pre.model.encoder.state_dict()              # what train_2d writes under 'state_dict'
    assert list(cls.encoder.state_dict().keys()) == list(saved.keys())
    assert [k for k in cls.state_dict() if k.startswith("classification_head")] == ["classification_head.3.weight", "classification_head.3.bias"]
    path = str(tmp_path / "pre.pt")
    torch.save({"state_dict": dict(saved, **{"fc.weight": torch.zeros(2, 512)}), "epoch": 0}, path)
    loaded = ChestClassifier(encoder_weights=path)
    assert all(torch.equal(loaded.encoder.state_dict()[k], saved[k]) for k in saved)
    pre.model.encoder.load_state_dict(loaded.encoder.state_dict())      # and back
