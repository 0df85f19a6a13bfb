"""Held-out validation on the GPU: the fused inference convolutions, PCRLv23d.infer, pcrl_val_metrics and train_3d.validate.

Tolerances are `check`'s of tests/test_ops_gpu.py (float32: 2e-5 * max|ref|; bf16 with a rounded output: 1e-2 * max|ref|) wherever a kernel is
compared with float64 torch, and the bounds of test_eval_mode_forward_matches_reference_golden (tests/test_model_gpu.py) wherever the model is
compared with the real reference.  The end-to-end bounds of test_validate_against_reference_fixture are DERIVED from those per-element bounds
(tools/make_val_fixtures.py stores what the derivation needs); nothing here is fitted to what the engine produces.
"""
import math
import os
import random
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import pcrlv2_oracle as O  # noqa: E402
from test_model_gpu import build, samples  # noqa: E402
from test_ops_gpu import act_dev, back, check, q, rnd  # noqa: E402
from pcrlv2_amd import ops, train_3d as T  # noqa: E402
from pcrlv2_amd._lib import ACT_NONE, ACT_RELU, dtype_code, lib, stream_handle  # noqa: E402
from pcrlv2_amd.models import PCRLv23d  # noqa: E402
from pcrlv2_amd.optim import FusedSGD  # noqa: E402

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
F32 = torch.float32


# ---- 1. fused kernels against float64 torch -------------------------------------------------------------------------------------------
def _model_layers(d, h, w):
    """(Ci, Co, D, H, W) of every LUConv of the default PCRLv23d with more than one output channel, for a d x h x w input."""
    out = []
    lv = lambda s: (d >> s, h >> s, w >> s)
    for s, (a, b) in enumerate(((32, 64), (64, 128), (128, 256), (256, 512))):      # encoder stage s: in -> a = 32 * 2^s -> b = 64 * 2^s, in = 1 or the previous b (= a)
        out += [(1 if s == 0 else a, a, *lv(s)), (a, b, *lv(s))]
    for s, c in ((2, 256), (1, 128), (0, 64)):                                     # decoder: 2c (after the up-convolution) -> c -> c
        out += [(2 * c, c, *lv(s)), (c, c, *lv(s))]
    return out


def _classes():
    seen, cases = set(), []
    Ns = (1, 3, 4)
    for vol in ((32, 32, 16), (16, 16, 16)):
        for cls in _model_layers(*vol):
            if cls not in seen:
                seen.add(cls)
                cases.append(cls + (Ns[len(cases) % 3],))
    # the full-resolution layers at 64 x 64 x 32.  One sample each where Ci >= 64: ATen's float64 CPU convolution materialises the im2col
    # matrix of a sample (27 * Ci * voxels * 8 bytes = 3.6 GB for Ci = 128), the kernels treat samples independently and every N of
    # {1, 3, 4} is covered on every kernel family by the classes above
    cases += [(1, 32, 64, 64, 32, 3), (32, 64, 64, 64, 32, 1), (128, 64, 64, 64, 32, 1), (64, 64, 64, 64, 32, 1)]
    return cases


CASES = _classes()


def test_case_list_covers_the_default_model():
    """The class list is derived, not typed in: pin what it must contain."""
    cls = {c[:5] for c in CASES}
    for want in ((1, 32, 32, 32, 16), (32, 64, 32, 32, 16), (64, 64, 16, 16, 8), (64, 128, 16, 16, 8), (128, 128, 8, 8, 4), (128, 256, 8, 8, 4),
                 (256, 256, 4, 4, 2), (256, 512, 4, 4, 2), (512, 256, 8, 8, 4), (256, 256, 8, 8, 4), (256, 128, 16, 16, 8), (128, 128, 16, 16, 8),
                 (128, 64, 32, 32, 16), (64, 64, 32, 32, 16), (1, 32, 16, 16, 16), (256, 512, 2, 2, 2), (128, 64, 16, 16, 16),
                 (32, 64, 64, 64, 32), (128, 64, 64, 64, 32), (64, 64, 64, 64, 32), (1, 32, 64, 64, 32)):
        assert want in cls, want
    assert {c[5] for c in CASES} == {1, 3, 4}


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_fused_conv_affine_against_float64_torch(case):
    """pcrl_conv3d_k3_fwd_affine / pcrl_conv3d_k3_c1_fwd_affine against F.conv3d -> affine -> activation in float64 on the CPU, float32 and bf16,
    ReLU and none, with the tolerance `check` applies to the existing forward convolution of that dtype."""
    Ci, Co, D, H, W, N = case
    L, s = lib(), stream_handle()
    x, w, b = rnd(N, Ci, D, H, W, seed=1), rnd(Co, Ci, 3, 3, 3, seed=2, scale=0.1 if Ci > 1 else 1.0), rnd(Co, seed=3)
    scale, shift = rnd(Co, seed=4) * 0.5 + 1.0, rnd(Co, seed=5) * 0.5
    for dt in DTYPES:
        if Ci == 1:
            brick = dt == torch.bfloat16 and D % 4 == 0 and H % 8 == 0 and W % 8 == 0       # the MFMA first-layer kernel takes x and w as bf16
            y = F.conv3d(q(x, dt) if brick else x, q(w, dt) if brick else w, b, padding=1)
            xd, wd = x.float().to(DEV).contiguous(), w.float().to(DEV)
        else:
            y = F.conv3d(q(x, dt), q(w, dt), b, padding=1)
            xd = act_dev(x, dt)
            wd, _ = ops.PackedWeights("conv3").get(w.float().to(DEV), dt)
        z = y * scale.view(1, -1, 1, 1, 1) + shift.view(1, -1, 1, 1, 1)
        for act in (ACT_RELU, ACT_NONE):
            ref = torch.relu(z) if act == ACT_RELU else z
            a = ops.new_act(N, D, H, W, Co, dt, DEV)
            a.fill_(float("nan"))
            if Ci == 1:
                L.call("pcrl_conv3d_k3_c1_fwd_affine", xd, wd, b.float().to(DEV), scale.float().to(DEV), shift.float().to(DEV), a, N, D, H, W, Co, act,
                       dtype_code(dt), s)
            else:
                nb = L.call("pcrl_conv3d_k3_fwd_affine_ws_bytes", N, D, H, W, Ci, Co, dtype_code(dt))
                L.call("pcrl_conv3d_k3_fwd_affine", xd, wd, b.float().to(DEV), scale.float().to(DEV), shift.float().to(DEV), a,
                       ops.workspace(nb, xd.device) if nb else None, nb, N, D, H, W, Ci, Co, act, dtype_code(dt), s)
            err = check(a, ref, dt, f"fused conv {case} act={act}")
            print(f"fused conv {case} {dt} act={act}: max|d| = {err:.3e}")


def test_fused_route_covers_the_layers_that_carry_the_bytes():
    """Host-only query: every BatchNorm + ReLU LUConv of the default model at full and half resolution is ONE kernel, at b = 32 / 64x64x32 and at
    b = 8 / 128x128x64, in bf16 and float32; GroupNorm / InstanceNorm / PReLU / ELU / sigmoid layers and the 1-channel heads never are."""
    for N, (d, h, w) in ((32, (64, 64, 32)), (8, (128, 128, 64))):
        for Ci, Co, D, H, W in _model_layers(d, h, w):
            if D < d // 2:
                continue
            for dt in DTYPES:
                assert ops.infer_fused_route(N, D, H, W, Ci, Co, ACT_RELU, dt), (N, Ci, Co, D, H, W, dt)
                if Ci > 1:
                    assert lib().call("pcrl_conv3d_k3_fwd_affine_fused", N, D, H, W, Ci, Co, dtype_code(dt)) == 1
    from pcrlv2_amd._lib import ACT_ELU, ACT_SIGMOID, ACT_SILU
    for act in (ACT_ELU, ACT_SIGMOID, ACT_SILU):
        assert not ops.infer_fused_route(32, 64, 64, 32, 32, 64, act, torch.bfloat16)
    assert not ops.infer_fused_route(32, 64, 64, 32, 32, 64, ACT_RELU, torch.bfloat16, norm_is_bn=False)
    assert not ops.infer_fused_route(32, 64, 64, 32, 64, 1, ACT_RELU, torch.bfloat16)


# ---- 2. infer against the real reference ----------------------------------------------------------------------------------------------
def _eval_state(fx):
    b, dhw = int(fx["meta/b"]) if "meta/b" in fx else int(fx["meta/state_b"]), tuple(int(v) for v in fx["meta/dhw"])
    with torch.backends.mkldnn.flags(enabled=False):
        st1, _, _, _ = O.train_steps(O.fill_state(torch.float64), [O.fill_batch(b, dhw, dtype=torch.float64, seed=int(fx["meta/state_batch_seed"]))], 0, 1e-3, 240, 0)
    return {k: v.detach() for k, v in st1.items()}, b, dhw


def _f32_state(st):
    return {k: (v.float() if v.is_floating_point() else v) for k, v in st.items()}


@pytest.mark.parametrize("dt", DTYPES)
def test_infer_matches_reference_golden(dt, golden_dir):
    """PCRLv23d.infer against the REAL reference in .eval() (tests/golden/eval_b2_32x32x16.npz) with the bounds of
    test_eval_mode_forward_matches_reference_golden: float32 maps 5e-5 / features 2e-4 abs; bf16 maps 2e-2 abs, features cosine > 0.995.
    In train AND eval mode; the state dict is unchanged; local=True returns no masks; features_only returns (None, feats, []); in float32
    infer agrees with model.eval()(x) to `check`'s float32 tolerance."""
    fx = np.load(os.path.join(golden_dir, "eval_b2_32x32x16.npz"))
    st1, b, dhw = _eval_state(fx)
    x = O.fill_batch(b, dhw, dtype=torch.float32, seed=int(fx["meta/input_seed"]))[0].to(DEV)
    model = build(dt, _f32_state(st1))
    map_tol = 5e-5 if dt == torch.float32 else 2e-2
    for training in (True, False):
        model.train(training)
        sd_before = {k: v.clone() for k, v in model.state_dict().items()}
        out, feats, masks = model.infer(x)
        assert model.training is training
        assert not out.requires_grad and len(masks) == 3 and out.shape == x.shape
        assert np.abs(samples(out, 512) - fx["out/samples"]).max() < map_tol
        for i in range(3):
            assert np.abs(samples(masks[i], 512) - fx[f"mask{i}/samples"]).max() < map_tol, i
            for j, nm in enumerate(("pro", "pre")):
                a, r = feats[i][j].double().cpu().numpy(), fx[f"{nm}{i}"]
                if dt == torch.float32:
                    np.testing.assert_allclose(a, r, rtol=0, atol=2e-4, err_msg=f"{nm}{i}")
                else:
                    cs = float(a.ravel() @ r.ravel() / (np.linalg.norm(a) * np.linalg.norm(r)))
                    assert cs > 0.995, (nm, i, cs)
        for k, v in model.state_dict().items():
            assert torch.equal(v, sd_before[k]), k
        assert model.infer(x, local=True)[2] == []
        none, feats_only, empty = model.infer(x, features_only=True)
        assert none is None and empty == [] and all(torch.equal(feats_only[i][j], feats[i][j]) for i in range(3) for j in range(2))
    model.eval()
    e_out, e_feats, e_masks = model(x)
    if dt == torch.float32:
        check(out, back(e_out), dt, "infer vs eval out")
        for i in range(3):
            check(masks[i], back(e_masks[i]), dt, f"infer vs eval mask{i}")
            for j in range(2):
                check(feats[i][j], back(e_feats[i][j]), dt, f"infer vs eval feature {i}/{j}")
        print("float32: infer bit-identical to model.eval()(x):", all(torch.equal(a, b_) for a, b_ in ((out, e_out), *zip(masks, e_masks))))


@pytest.mark.parametrize("kw", [dict(norm="gn", act="silu"), dict(act="elu")], ids=["gn-silu", "elu"])
def test_infer_falls_back_to_the_unfused_path(kw):
    """Layers without a fused form take today's path: infer == model.eval()(x) bit for bit."""
    torch.manual_seed(3)
    model = PCRLv23d(**kw).to(DEV)
    model.eval()
    x = O.fill_batch(2, (32, 32, 16), dtype=torch.float32, seed=9)[0].to(DEV)
    with lib().count_calls("pcrl_conv3d_k3_fwd_affine", "pcrl_conv3d_k3_c1_fwd_affine") as n:
        out, feats, masks = model.infer(x)
    assert not n, n
    e_out, e_feats, e_masks = model(x)
    assert torch.equal(out, e_out) and all(torch.equal(a, b) for a, b in zip(masks, e_masks))
    assert all(torch.equal(feats[i][j], e_feats[i][j]) for i in range(3) for j in range(2))


def test_infer_uses_the_fused_kernels():
    """b = 4, 32x32x16, bf16: the first layer and the seven wide-brick LUConvs (full and half resolution) are ONE launch each -- eight
    pcrl_bn_act_apply passes fewer than model.eval()(x); the quarter- and eighth-resolution layers (4x8x8 bricks) keep conv + apply."""
    model = build(torch.bfloat16)
    model.eval()
    x = O.fill_batch(4, (32, 32, 16), dtype=torch.float32, seed=9)[0].to(DEV)
    names = ("pcrl_conv3d_k3_fwd_affine", "pcrl_conv3d_k3_c1_fwd_affine", "pcrl_bn_act_apply", "pcrl_conv3d_k3_fwd_ws", "pcrl_conv3d_k3_c1_fwd")
    with lib().count_calls(*names) as n:
        model.infer(x)
    with lib().count_calls(*names) as e:
        model(x)
    assert n.get("pcrl_conv3d_k3_c1_fwd_affine") == 1 and n.get("pcrl_conv3d_k3_fwd_affine") == 7 and "pcrl_conv3d_k3_c1_fwd" not in n, n
    assert "pcrl_conv3d_k3_fwd_affine" not in e and "pcrl_conv3d_k3_c1_fwd_affine" not in e and e.get("pcrl_conv3d_k3_c1_fwd") == 1, e
    assert e["pcrl_bn_act_apply"] - n["pcrl_bn_act_apply"] == 8 and e["pcrl_conv3d_k3_fwd_ws"] - n["pcrl_conv3d_k3_fwd_ws"] == 7, (n, e)


# ---- 3. bf16 accuracy, reported -------------------------------------------------------------------------------------------------------
def test_bf16_accuracy_of_infer_and_eval_reported(golden_dir):
    """rel-L2 of infer and of model.eval()(x) in bf16 against the float64 oracle forward on the inputs of test 2.  Reported, not asserted: the
    fused path drops one rounding (the pre-normalisation tensor) and is expected to be no worse."""
    fx = np.load(os.path.join(golden_dir, "eval_b2_32x32x16.npz"))
    st1, b, dhw = _eval_state(fx)
    x64 = O.fill_batch(b, dhw, dtype=torch.float64, seed=int(fx["meta/input_seed"]))[0]
    with torch.backends.mkldnn.flags(enabled=False), torch.no_grad():
        o_out, o_feats, o_masks = O.forward(st1, x64, training=False)
    model = build(torch.bfloat16, _f32_state(st1))
    model.eval()
    x = x64.float().to(DEV)
    rel = lambda a, r: float((a.double().cpu() - r).norm() / r.norm())
    rows = []
    for name, (out, feats, masks) in (("infer", model.infer(x)), ("eval", model(x))):
        vals = [rel(out, o_out)] + [rel(masks[i], o_masks[i]) for i in range(3)] + [rel(feats[i][j], o_feats[i][j]) for i in range(3) for j in range(2)]
        rows.append((name, vals))
    names = ["out", "mask0", "mask1", "mask2", "pro0", "pre0", "pro1", "pre1", "pro2", "pre2"]
    for name, vals in rows:
        print(f"bf16 rel-L2 vs float64 oracle, {name:5s}: " + "  ".join(f"{n} {v:.3e}" for n, v in zip(names, vals)))


# ---- 4. pcrl_val_metrics against float64 torch ----------------------------------------------------------------------------------------
def _metrics64(out1, masks, gt, f1, f2, fl, B):
    """The ten batch means in float64 torch on the CPU (mse_loss / CosineSimilarity), from tensors of any float dtype."""
    d = lambda t: t.detach().double().cpu()
    cosine = torch.nn.CosineSimilarity()
    cl = lambda a, b_: -(cosine(d(a[1]), d(b_[0])).mean() + cosine(d(b_[1]), d(a[0])).mean()) * 0.5
    vals = [F.mse_loss(d(out1), d(gt))] + [F.mse_loss(d(m), d(gt)) for m in masks]
    vals += [cl(f1[k], f2[k]) for k in range(3)]
    nl = fl[0][0].shape[0] // B
    for k in range(3):
        tot = 0.0
        for i in range(nl):
            crop = [t[B * i:B * (i + 1)] for t in fl[k]]
            tot = tot + cl(f1[k], crop) + cl(f2[k], crop)
        vals.append(tot / (2 * nl))
    return torch.stack([torch.as_tensor(v, dtype=torch.float64) for v in vals])


def _check_each(got, ref, what):
    """`check`'s float32 tolerance per metric (every value against its OWN magnitude)."""
    errs = []
    for i, k in enumerate(T.VAL_KEYS):
        errs.append(check(torch.as_tensor([float(got[i])], dtype=torch.float64), torch.as_tensor([float(ref[i])], dtype=torch.float64), F32, f"{what}: {k}"))
    return errs


@pytest.mark.parametrize("B", [3, 4])
def test_val_metrics_kernel_against_float64_torch(B):
    g = torch.Generator().manual_seed(100 + B)
    S, nl, C = (16, 16, 8), 6, (256, 128, 64)
    r = lambda *sh: torch.randn(*sh, generator=g).to(DEV)
    out1, gt = torch.rand(B, 1, *S, generator=g).to(DEV), torch.rand(B, 1, *S, generator=g).to(DEV)
    masks = [torch.rand(B, 1, *S, generator=g).to(DEV) for _ in range(3)]
    f1, f2, fl = ([[r(rows, c), r(rows, c)] for c in C] for rows in (B, B, nl * B))
    acc = torch.zeros(11, dtype=torch.float64, device=DEV)
    ops.val_metrics(out1, masks, gt, f1, f2, fl, acc)
    acc2 = torch.zeros(11, dtype=torch.float64, device=DEV)
    ops.val_metrics(out1, masks, gt, f1, f2, fl, acc2)
    assert torch.equal(acc, acc2)                                  # deterministic
    ops.val_metrics(out1, masks, gt, f1, f2, fl, acc2)             # accumulates
    host, host2 = acc.cpu(), acc2.cpu()
    assert host[10] == B and host2[10] == 2 * B and torch.allclose(host2, 2 * host, rtol=1e-14, atol=0)
    ref = _metrics64(out1, masks, gt, f1, f2, fl, B)
    errs = _check_each(host[:10] / B, ref, f"val_metrics B={B}")
    print(f"val_metrics B={B}: max|d| per metric = " + " ".join(f"{e:.1e}" for e in errs))
    # the kernel is float64 throughout: the relative bound test_validate2d_gpu.py asserts for its twin
    got = host[:10] / B
    rel = [abs(float(got[i] - ref[i])) / abs(float(ref[i])) for i in range(10)]
    print(f"val_metrics B={B}: relative distance per metric = " + " ".join(f"{e:.1e}" for e in rel))
    assert max(rel) <= 1e-12, rel


# ---- 5. validate assembly, tight ------------------------------------------------------------------------------------------------------
def _batches(sizes=(4, 4, 3), seeds=(21, 22, 23), dhw=(32, 32, 16), gt_scale=(1.0, 1.0, 1.0)):
    out = []
    for b, seed, sc in zip(sizes, seeds, gt_scale):
        x1, x2, gt, gt2, loc = O.fill_batch(b, dhw, dtype=torch.float32, seed=seed)
        out.append((x1, x2, gt * sc, gt2, loc))
    return out


@pytest.mark.parametrize("epoch", [0, 120])
@pytest.mark.parametrize("dt", DTYPES)
def test_validate_assembles_the_batches_correctly(dt, epoch):
    """validate over a list of three batches (4, 4 and 3 samples) against float64 metrics computed HERE from the engine's own per-batch infer
    outputs: sample weighting, the pairing of the cosine terms, beta(epoch) and the total.  The third batch's gt is scaled so that every MSE
    metric differs between batches by at least 100 x the tolerance -- a batch-weighted (instead of sample-weighted) mean cannot pass."""
    model = build(dt)
    model.eval()
    batches = _batches(gt_scale=(1.0, 1.0, 3.0))
    per, n = [], 0
    for x1, x2, gt, _, loc in batches:
        B = x1.shape[0]
        o, f1, m = model.infer(x1.to(DEV))
        _, f2, _ = model.infer(x2.to(DEV), features_only=True)
        _, fl, _ = model.infer(torch.cat(loc, 0).to(DEV), local=True, features_only=True)
        per.append((B, _metrics64(o, m, gt, f1, f2, fl, B)))
        n += B
    for i in range(4):      # the MSE metrics of the third batch against the first two
        gap = min(abs(float(per[2][1][i] - per[j][1][i])) for j in (0, 1))
        assert gap >= 100 * 2e-5 * max(float(p[1][i]) for p in per), (i, gap)
    ref = sum(B * v for B, v in per) / n
    wrong = sum(v for _, v in per) / len(per)
    assert float((ref[:4] - wrong[:4]).abs().min()) > 10 * 2e-5 * float(ref[:4].max())      # the unweighted mean is out of tolerance
    got = T.validate(model, batches, epoch)
    assert got["n"] == n == 11
    errs = _check_each([got[k] for k in T.VAL_KEYS], ref, f"validate {dt} epoch {epoch}")
    beta = 0.5 * (1.0 + math.cos(math.pi * epoch / 240))
    total = float(ref[0] + ref[4:7].mean() + ref[7:10].mean() + beta * ref[1:4].mean())
    check(torch.as_tensor([got["total"]], dtype=torch.float64), torch.as_tensor([total], dtype=torch.float64), F32, "validate total")
    print(f"validate assembly {dt} epoch {epoch}: max|d| per metric = " + " ".join(f"{e:.1e}" for e in errs))


# ---- 6. validate against the real reference, end to end -------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_validate_against_reference_fixture(dt, golden_dir):
    """tests/golden/val_b4_32x32x16.npz (tools/make_val_fixtures.py: the real reference in .eval(), float64, three batches of 4, 4 and 3).
    Bounds, derived from the per-element envelope of test 2 (d = 5e-5 float32 / 2e-2 bf16 on the maps, 2e-4 on float32 features):
    MSE metrics 2 * max|pred - gt| * d + d^2; float32 cosine metrics the fixture's cos_bound_f32 (see the tool); total = the sum of its
    terms' bounds.  bf16 cosine metrics are printed only (test 2 bounds bf16 features by direction, not per element)."""
    fx = np.load(os.path.join(golden_dir, "val_b4_32x32x16.npz"))
    st1, _, dhw = _eval_state(fx)
    epoch = int(fx["meta/epoch"])
    batches = [O.fill_batch(int(b), dhw, dtype=torch.float32, seed=int(s)) for b, s in zip(fx["meta/sizes"], fx["meta/seeds"])]
    model = build(dt, _f32_state(st1))
    got = T.validate(model, batches, epoch)
    assert model.training and got["n"] == int(fx["meta/sizes"].sum())
    d = 5e-5 if dt == torch.float32 else 2e-2
    mse_bound = 2.0 * float(fx["max_abs_diff"]) * d + d * d
    if dt == torch.float32:
        assert mse_bound <= 1.0e-4
    keys = [str(k) for k in fx["keys"]]
    assert tuple(keys) == T.VAL_KEYS
    dist = {k: abs(got[k] - float(v)) for k, v in zip(keys, fx["values"])}
    dist["total"] = abs(got["total"] - float(fx["total"]))
    report = f"validate vs reference [{dt}]: " + "  ".join(f"{k} {v:.2e}" for k, v in dist.items())
    print(report)
    for k in keys[:4]:
        assert dist[k] <= mse_bound, report
    if dt == torch.float32:
        cb = [float(v) for v in fx["cos_bound_f32"]]
        for k in range(3):
            assert dist[f"cos_global{k}"] <= cb[k] and dist[f"cos_local{k}"] <= cb[k], report
        beta = 0.5 * (1.0 + math.cos(math.pi * epoch / 240))
        assert dist["total"] <= mse_bound + 2.0 * sum(cb) / 3.0 + beta * mse_bound, report


# ---- 7. validation does not disturb training ------------------------------------------------------------------------------------------
def _train_run(validate_after=()):
    random.seed(5)
    torch.manual_seed(5)
    model = build(torch.float32)
    opt = FusedSGD(model.parameters(), lr=1e-2, momentum=0.9, weight_decay=1e-4)
    crit, cosine = T.MSELoss(), T.CosineSimilarityMean()
    val_batches = _batches(sizes=(4, 3), seeds=(61, 62))
    vals = []
    for step in range(6):
        T.train_step(model, opt, O.fill_batch(4, (32, 32, 16), dtype=torch.float32, seed=40 + step), 3, crit, cosine)
        if step + 1 in validate_after:
            vals.append(T.validate(model, val_batches, 3))
    torch.cuda.synchronize()
    return model, opt, vals, val_batches


def test_validation_does_not_disturb_training():
    m0, o0, _, _ = _train_run()
    sd0, buf0, rs0 = {k: v.clone() for k, v in m0.state_dict().items()}, o0.flat_buf.clone(), random.getstate()
    t0 = torch.random.get_rng_state()
    m1, o1, vals, val_batches = _train_run(validate_after=(2, 4))
    assert len(vals) == 2 and m1.training
    for k, v in m1.state_dict().items():
        assert torch.equal(v, sd0[k]), k
    assert torch.equal(o1.flat_buf, buf0) and torch.equal(o1.flat_p, o0.flat_p)
    assert random.getstate() == rs0 and torch.equal(torch.random.get_rng_state(), t0)
    a, b = T.validate(m1, val_batches, 3), T.validate(m1, val_batches, 3)
    assert a == b and a["n"] == 7            # bit-identical on an unchanged model
    assert a != vals[0]                      # ... and the weights moved since the first pass


VAL2_WORKER = r'''
import os, sys, torch, torch.distributed as dist
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "oracle"))
import pcrlv2_oracle as O
from pcrlv2_amd import ddp, train_3d as T
from pcrlv2_amd.models import PCRLv23d
torch.cuda.set_device(0)
model = PCRLv23d().cuda()
model.load_state_dict(O.fill_state(torch.float32))
model.train()
batches = [O.fill_batch(b, (32, 32, 16), dtype=torch.float32, seed=70 + i) for i, b in enumerate((2, 2, 2, 1))]
single = T.validate(model, batches, 7)                        # no group yet: the whole list
rank, world, _ = ddp.init_process_group_from_env("gloo")      # two processes, ONE GPU: gloo moves the CUDA buffer
try:
    both = T.validate(model, batches, 7, group=dist.group.WORLD)
    assert both["n"] == single["n"] == 7, (both["n"], single["n"])
    for k, v in single.items():
        tol = 2e-5 * max(abs(v), 1e-6)
        assert abs(both[k] - v) <= tol, (k, both[k], v)
    dist.barrier()
    print("OK", rank, flush=True)
finally:
    dist.destroy_process_group()      # tear the group down before the interpreter exits
'''


def test_validate_two_ranks_one_gpu_gloo(tmp_path):
    """validate over a world-2 gloo group (both ranks on cuda:0): each rank evaluates a contiguous run of the batches (4 + 3 samples), one
    all_reduce combines the sums; the result equals the single-process pass to `check`'s float32 tolerance on both ranks."""
    script = tmp_path / "val2.py"
    script.write_text(VAL2_WORKER)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29787", WORLD_SIZE="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen(["timeout", "-k", "10", "420", sys.executable, str(script), root], env=dict(env, RANK=str(r), LOCAL_RANK="0"),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [None, None]

    def drain(i):
        outs[i] = procs[i].communicate()[0]

    threads = [threading.Thread(target=drain, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert all(p.returncode == 0 for p in procs), "\n".join((o or "")[-3000:] for o in outs)
    assert all("OK" in o for o in outs)
