"""LUNA16 nodule classification on the GPU: pcrl_prep_cubes / pcrl_prep_hu_to_unit bit for bit against tests/nodule_reference.py, models.NoduleClassifier
against a float64 torch comparator (oracle/pcrlv2_oracle.py's encoder + mean / linear / binary_cross_entropy_with_logits), and
`luna_nodules.py extract | train | predict` end to end on two small series.

Tolerances are other files' and are used as they stand:
  float32 loss 1e-5 abs; per-tensor gradient rel-L2 1.2e-2 for encoder tensors and BatchNorm vectors, 5e-3 for every other weight (here: the head's);
      conv biases in front of a BatchNorm 1e-5 ABSOLUTE (their gradient is analytically zero)      -- tests/test_model_gpu.py at c_small_b4
      (test_fp32_step_matches_reference_golden, _grad_report with LOOSE_GRAD_TENSORS / ZERO_GRAD)
  bf16    loss 3e-2 abs (test_bf16_step_within_stated_tolerance_of_golden); weight tensors of >= 1024 elements: cosine to the float64 gradient > 0.7
      and norm ratio within 25 % (test_restoration_path_gradients_vs_live_oracle); every gradient finite
  head    on an exact input: the derived bounds of tests/test_cls_head_gpu.py (`_bounds`), imported, on `down_tr512`'s layout
  infer   against model.eval()(x): `check` of tests/test_ops_gpu.py (float32 2e-5 max|ref|, bf16 1e-2 max|ref|), what tests/test_validate_gpu.py holds the
      fused eval forward to against the unfused one
"""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import nodule_reference as R  # noqa: E402
import pcrlv2_oracle as O  # noqa: E402
import test_cls_head_gpu as H  # noqa: E402
from test_ops_gpu import check  # noqa: E402
from pcrlv2_amd import data as D  # noqa: E402
from pcrlv2_amd import luna_nodules as N  # noqa: E402
from pcrlv2_amd import luna_prep as P  # noqa: E402
from pcrlv2_amd import functions as Fn  # noqa: E402
from pcrlv2_amd import ops, ops2d  # noqa: E402
from pcrlv2_amd._lib import lib, stream_handle  # noqa: E402
from pcrlv2_amd.models import NoduleClassifier, PCRLv23d  # noqa: E402
from pcrlv2_amd.models import pcrlv2_model_3d as M3  # noqa: E402
from pcrlv2_amd.optim import FusedSGD  # noqa: E402
from pcrlv2_amd.train_finetune import train_step  # noqa: E402

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
SHAPE = (32, 32, 16)            # the golden case's: bottleneck 4 x 4 x 2


# ---- 1. pcrl_prep_cubes ---------------------------------------------------------------------------------------------------------
def _volume(shape, seed=0):
    return np.random.default_rng(seed).integers(-3000, 3001, shape).astype(np.int16)


def _starts(X, Y, Z, cube):
    """13 starts: inside (as far as the cube fits), one across each of the six faces, two corners, two fully outside, x0 = 1 and x0 = 2."""
    CX, CY, CZ = cube
    mid = (max(0, (X - CX) // 2), max(0, (Y - CY) // 2), max(0, (Z - CZ) // 2))
    s = [mid,
         (-3, mid[1], mid[2]), (X - CX + 3 if CX <= X else X - 5, mid[1], mid[2]),
         (mid[0], -5, mid[2]), (mid[0], Y - CY + 2 if CY <= Y else Y - 3, mid[2]),
         (mid[0], mid[1], -1), (mid[0], mid[1], Z - CZ + 7 if CZ <= Z else Z - 2),
         (-2, -3, -4), (X - 4, Y - 3, Z - 2),
         (X + 5, 0, 0), (-CX - 1, 2, 2),
         (1, mid[1], mid[2]), (2, mid[1], mid[2])]
    assert len(s) == 13 and {v[0] % 2 for v in s} == {0, 1}
    return np.array(s, dtype=np.int32)


# [Z, Y, X]: the issue's volume (X odd: the rows' shifts take all four values), X % 4 == 0 (one shift) and X % 4 == 2 (two), x0 over every
# residue, and a volume smaller than the 16^3 cube on every axis
VOLUMES = {"41x29x37": (41, 29, 37), "20x19x40": (20, 19, 40), "20x19x38": (20, 19, 38), "9x11x13": (9, 11, 13)}
CUBES = [(16, 16, 16), (64, 64, 32), (8, 24, 40)]


@pytest.fixture(scope="module")
def volumes():
    return {k: _volume(s, seed=i) for i, (k, s) in enumerate(VOLUMES.items())}


@pytest.mark.parametrize("cube", CUBES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("name", list(VOLUMES))
def test_prep_cubes_equals_the_restatement(volumes, name, cube):
    vol = volumes[name]
    Z, Y, X = vol.shape
    start = _starts(X, Y, Z, cube)
    if name != "41x29x37":
        start[:4, 0] += np.arange(4, dtype=np.int32)          # x0 over every residue modulo 4
    inside = [(0 <= s[0] and s[0] + cube[0] <= X) and (0 <= s[1] and s[1] + cube[1] <= Y) and (0 <= s[2] and s[2] + cube[2] <= Z) for s in start]
    assert any(inside) == all(c <= n for c, n in zip(cube, (X, Y, Z)))
    vd = torch.from_numpy(vol).to(DEV)
    for f32 in (False, True):
        want = R.cubes(vol, start, cube, float32=f32)
        got = N.gpu_cubes(vd, start, cube, float32=f32)
        again = N.gpu_cubes(vd, start, cube, float32=f32)
        assert got.dtype == (torch.float32 if f32 else torch.int16) and tuple(got.shape) == (13,) + cube
        g = got.cpu().numpy()
        bad = np.argwhere(g != want)
        assert bad.size == 0, f"{name} {cube} float32={f32}: {len(bad)} elements differ, first at [m, i, j, k] = {bad[0].tolist()}, start {start[bad[0][0]].tolist()}"
        assert torch.equal(got, again)
    assert np.all(R.cubes(vol, start[9:11], cube) == -1000)          # the two starts outside really are
    if name == "9x11x13":
        assert all(c > n for c, n in zip(CUBES[0], (X, Y, Z)))       # a cube larger than the volume on every axis


def test_prep_cubes_starts_at_the_ends_of_int32_read_air(volumes):
    """A start is whatever an int32 holds: the kernel's coordinates are 64-bit, so the far ends read air and do not wrap into the volume."""
    vol = volumes["41x29x37"]
    lo, hi = -2 ** 31, 2 ** 31 - 1
    start = np.array([(hi, 0, 0), (0, hi, 0), (0, 0, hi), (lo, 0, 0), (0, lo, 0), (0, 0, lo), (hi - 5, hi - 5, hi - 5), (lo, lo, lo), (0, 0, 0)], dtype=np.int32)
    got = N.gpu_cubes(torch.from_numpy(vol).to(DEV), start, (16, 16, 16)).cpu().numpy()
    assert np.all(got[:8] == -1000)
    np.testing.assert_array_equal(got[8], R.cubes(vol, start[8:], (16, 16, 16))[0])


def test_prep_cubes_m_zero_returns(volumes):
    vd = torch.from_numpy(volumes["41x29x37"]).to(DEV)
    out = N.gpu_cubes(vd, np.zeros((0, 3), np.int32), (16, 16, 16))
    assert tuple(out.shape) == (0, 16, 16, 16)
    torch.cuda.synchronize()


def test_prep_cubes_into_a_batch_buffer(volumes):
    """predict's form: a device tensor of starts, the first M rows of a longer buffer."""
    vol = volumes["20x19x40"]
    vd = torch.from_numpy(vol).to(DEV)
    start = _starts(40, 19, 20, (16, 16, 16))
    buf = torch.full((20, 16, 16, 16), -7.0, device=DEV)
    got = N.gpu_cubes(vd, torch.from_numpy(start).to(DEV)[3:10], (16, 16, 16), True, buf)
    assert got.data_ptr() == buf.data_ptr() and got.shape[0] == 7
    np.testing.assert_array_equal(got.cpu().numpy(), R.cubes(vol, start[3:10], (16, 16, 16), float32=True))
    assert bool((buf[7:] == -7.0).all())


def test_balanced_loader_set_epoch_continues_the_sequence(tmp_path):
    """What a resumed run relies on: after set_epoch(k) the next pass draws epoch k's negatives, and the one after it epoch k + 1's."""
    rng = np.random.default_rng(0)
    np.save(tmp_path / "s_cand.npy", rng.integers(-1000, 1000, (12, 8, 8, 8)).astype(np.int16))
    labels = [1, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0]
    entries = [(str(tmp_path / "s_cand.npy"), i, l) for i, l in enumerate(labels)]
    loader = D.BalancedCandidateLoader(entries, 2, 1, torch.device(DEV), seed=5)
    loader.set_epoch(3)
    for k in (3, 4):
        ys = torch.cat([y for _, y in loader]).cpu().view(-1)
        want = D.rank_share(D.balanced_epoch(np.array(labels), 5, k), 0, 1)
        np.testing.assert_array_equal(loader.table[:len(want)].numpy(), want)
        assert len(ys) == 6 and int(ys.sum()) == 3 and loader.epoch == k + 1
    assert not np.array_equal(D.balanced_epoch(np.array(labels), 5, 3), D.balanced_epoch(np.array(labels), 5, 0))


# ---- 2. pcrl_prep_hu_to_unit ----------------------------------------------------------------------------------------------------
def test_hu_to_unit_on_every_int16():
    v = np.arange(-32768, 32768, dtype=np.int16)
    vd = torch.from_numpy(v).to(DEV)
    out = torch.empty(v.size, dtype=torch.float32, device=DEV)
    lib().call("pcrl_prep_hu_to_unit", vd, out, v.size, stream_handle())
    np.testing.assert_array_equal(out.cpu().numpy(), np.float32((v.astype(np.float64) + 1000) / 2000))
    # a length that is no multiple of 8: the tail
    out2 = torch.full((1003,), -1.0, device=DEV)
    lib().call("pcrl_prep_hu_to_unit", vd[32000:], out2, 1001, stream_handle())
    np.testing.assert_array_equal(out2.cpu().numpy()[:1001], R.unit(v[32000:33001]))
    assert out2[1001:].tolist() == [-1.0, -1.0]


# ---- 3. the model ---------------------------------------------------------------------------------------------------------------
def _enc_keys(sd):
    return {k for k in sd if k.startswith("down_tr")}


def test_encoder_keys_and_checkpoint_loading(tmp_path):
    torch.manual_seed(5)
    pre = PCRLv23d()
    cls = NoduleClassifier()
    assert _enc_keys(cls.state_dict()) == _enc_keys(pre.state_dict()) and len(_enc_keys(pre.state_dict())) == 8 * 7
    assert list(cls.state_dict())[-2:] == ["classification_head.3.weight", "classification_head.3.bias"]
    assert tuple(cls.classification_head[3].weight.shape) == (1, 512)
    sd = pre.state_dict()
    for k in sd:                                               # running statistics and counters that differ from a fresh model's
        if k.endswith("running_mean"):
            sd[k] += 0.25
        if k.endswith("num_batches_tracked"):
            sd[k] += 3
    ck = str(tmp_path / "pre.pt")
    torch.save({"epoch": 7, "state_dict": sd, "optimizer": {}}, ck)
    got = NoduleClassifier(encoder_weights=ck).state_dict()
    for k in _enc_keys(sd):
        assert torch.equal(got[k], sd[k]), k
    torch.save({"state_dict": {"module." + k: v for k, v in sd.items()}}, ck)          # saved from under nn.DataParallel
    got = NoduleClassifier(encoder_weights=ck).state_dict()
    assert all(torch.equal(got[k], sd[k]) for k in _enc_keys(sd))
    short = {k: v for k, v in sd.items() if k != "down_tr256.ops.1.bn1.running_var"}
    torch.save({"state_dict": short}, ck)
    with pytest.raises(KeyError, match="down_tr256.ops.1.bn1.running_var"):
        NoduleClassifier(encoder_weights=ck)
    torch.save({"state_dict": dict(sd, **{"down_tr512.ops.2.conv1.weight": torch.zeros(1)})}, ck)
    with pytest.raises(KeyError, match="unexpected"):
        NoduleClassifier(encoder_weights=ck)
    torch.save(sd, ck)
    with pytest.raises(KeyError, match="state_dict"):
        NoduleClassifier(encoder_weights=ck)


def _pretrain_model(dt=torch.float32):
    m = PCRLv23d().to(DEV)
    m.load_state_dict(O.fill_state(torch.float32))
    m.train()
    return m.set_compute_dtype(dt)


def test_pcrlv23d_forward_goes_through_the_shared_encoder():
    """PCRLv23d's training forward on [4, 1, 32, 32, 16]: two runs from the same weights are bit-identical, its `out512` IS what the shared
    encoder function returns when called on a third copy, and the classifier's encoder (same weights) produces the same tensor."""
    x = O.fill_batch(4, SHAPE, dtype=torch.float32, seed=11)[0].to(DEV)
    a, b, c, lazy = _pretrain_model(), _pretrain_model(), _pretrain_model(), _pretrain_model()
    _begin_step()
    ra, rb = a(x), b(x)
    assert torch.equal(ra[0], rb[0]) and all(torch.equal(p, q) for p, q in zip(ra[2], rb[2]))
    assert all(torch.equal(ra[1][i][j], rb[1][i][j]) for i in range(3) for j in range(2))
    h = M3._train_encoder(c, x, lambda: None, False, stash=True)
    ops.end_of_forward_join()
    torch.cuda.synchronize()
    assert torch.equal(h, a.out512) and torch.equal(c.skip_out64, a.skip_out64) and torch.equal(c.skip_out256, b.skip_out256)
    for m in (a, b, c):
        m.flush_counters()
    assert all(torch.equal(v, c.state_dict()[k]) for k, v in a.state_dict().items() if k.startswith("down_tr"))
    # the classifier runs the engine step's form of the same half (lazy_skips: train_3d.step_losses' flag)
    lazy(x, lazy_skips=True)
    cls = NoduleClassifier(dropout=0.0).to(DEV)
    cls.load_state_dict({k: v for k, v in O.fill_state(torch.float32).items() if k.startswith("down_tr")}, strict=False)
    cls.train()
    hc = M3._train_encoder(cls, x, lambda: None, True, stash=False)
    ops.end_of_forward_join()
    torch.cuda.synchronize()
    assert torch.equal(hc, lazy.out512)
    print("[nodule] the lazy-skip encoder output is bit-identical to the stored-skip one:", torch.equal(hc, h))


# ---- 4. the training forward and backward against float64 ------------------------------------------------------------------------
NAMED = ("down_tr64.ops.0.conv1.weight", "down_tr512.ops.1.conv1.weight", "down_tr512.ops.1.bn1.weight", "classification_head.3.weight",
         "classification_head.3.bias")
ZERO = ("down_tr64.ops.0.conv1.bias", "down_tr512.ops.1.conv1.bias")
LOOSE = ("down_tr", ".bn1.weight", ".bn1.bias")             # tests/test_model_gpu.py LOOSE_GRAD_TENSORS


def _state():
    st = {k: v for k, v in O.fill_state(torch.float32).items() if k.startswith("down_tr")}
    g = torch.Generator().manual_seed(12)
    st["classification_head.3.weight"] = 0.05 * torch.randn(1, 512, generator=g)
    st["classification_head.3.bias"] = 0.1 * torch.randn(1, generator=g)
    return st


def _classifier(dt, dropout=0.0):
    m = NoduleClassifier(dropout=dropout).to(DEV)
    m.load_state_dict(_state())
    m.train()
    return m.set_compute_dtype(dt)


def _begin_step():
    """What train_step does in front of a forward: the pass counter and the parked gradients of whatever ran before start clean."""
    ops.begin_step()
    Fn.reset_parked()


def _inputs():
    x = O.fill_batch(4, SHAPE, dtype=torch.float32, seed=11)[0]
    return x, torch.tensor([[1], [0], [0], [1]], dtype=torch.uint8)


def _oracle_encoder(st, x, training=True):
    h = x
    for i, (p, _, _) in enumerate(O.ENCODER):
        if i in (2, 4, 6):
            h = F.max_pool3d(h, 2)
        h = O._luconv(h, st, p, None)
    return h


@pytest.fixture(scope="module")
def reference():
    """float64 on the CPU, computed once: loss, probabilities and the gradient of every parameter."""
    st = {k: (v.double() if v.is_floating_point() else v) for k, v in _state().items()}
    pn = [k for k in st if not O.is_buffer(k)]
    for k in pn:
        st[k].requires_grad_(True)
    x, y = _inputs()
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    with torch.backends.mkldnn.flags(enabled=False):
        z = F.linear(_oracle_encoder(st, x.double()).mean(dim=(2, 3, 4)), st["classification_head.3.weight"], st["classification_head.3.bias"])
        loss = F.binary_cross_entropy_with_logits(z, y.double())
        grads = dict(zip(pn, torch.autograd.grad(loss, [st[k] for k in pn])))
    return {"loss": float(loss.detach()), "probs": torch.sigmoid(z.detach()), "grads": grads}


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "bf16"])
def test_loss_and_gradients_against_float64(reference, dt):
    """In bf16 only weight tensors of >= 1024 elements (the two conv weights) are held to the cosine / norm bounds, as tests/test_model_gpu.py filters;
    `classification_head.3.weight` (512 elements), `.bias` and `down_tr512.ops.1.bn1.weight` are checked for being FINITE only there.  The head's own
    bf16 bounds are asserted on an exact input in test_head_kernels_on_the_ndhwc_view."""
    x, y = _inputs()
    model = _classifier(dt)
    _begin_step()
    loss, probs = model.loss(x.to(DEV), y.to(DEV))
    assert loss.dim() == 0 and tuple(probs.shape) == (4, 1) and not probs.requires_grad
    loss.backward()
    torch.cuda.synchronize()
    d = abs(float(loss.detach()) - reference["loss"])
    dp = float((probs.double().cpu() - reference["probs"]).abs().max())
    print(f"[nodule {dt}] loss {float(loss.detach()):.6f} vs {reference['loss']:.6f} |d| = {d:.2e}, probs max|d| = {dp:.2e}")
    params = dict(model.named_parameters())
    rows = []
    for name in NAMED:
        a, g = params[name].grad.double().cpu().reshape(-1), reference["grads"][name].reshape(-1)
        rows.append((name, float((a - g).norm() / g.norm()), float(a @ g / (a.norm() * g.norm())) if a.numel() > 1 else 1.0, float(a.norm() / g.norm()), a.numel()))
        print(f"[nodule {dt}] {name:34s} rel-L2 {rows[-1][1]:.3e} cos {rows[-1][2]:.4f} norm-ratio {rows[-1][3]:.3f}")
    zeros = {name: float(params[name].grad.abs().max()) for name in ZERO}
    print(f"[nodule {dt}] conv biases in front of a BatchNorm, max|g|: {zeros}")
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params.values())
    for name in ZERO:
        assert float(reference["grads"][name].abs().max()) < 1e-8
    if dt == torch.float32:
        assert d < 1e-5
        assert dp < 5e-5                                     # sigmoid outputs, test_model_gpu's map bound
        for name, rel, _, nr, _ in rows:
            tol = 1.2e-2 if any(k in name for k in LOOSE) else 5e-3
            assert rel < tol and abs(nr - 1) < tol, (name, rel, nr)
        assert all(v <= 1e-5 for v in zeros.values()), zeros
    else:
        assert d < 3e-2 and dp < 3e-2
        big = [r for r in rows if r[4] >= 1024]
        assert big and min(r[2] for r in big) > 0.7 and all(0.75 < r[3] < 1.25 for r in big), big


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "bf16"])
def test_head_kernels_on_the_ndhwc_view(dt):
    """`down_tr512`'s output layout -- [N, 512, 4, 4, 2] in NDHWC memory -- through NoduleClassifier._head_input into pcrl_cls_head_fwd / _bwd, against the
    float64 module chain with the DERIVED bounds of tests/test_cls_head_gpu.py (H = D * H of the volume, W = its W)."""
    N_, p = 4, 0.5
    g = torch.Generator().manual_seed(21)
    a5 = torch.relu(torch.randn(N_, 4, 4, 2, 512, generator=g)).to(dt)                  # NDHWC memory
    w, b = 0.15 * torch.randn(1, 512, generator=g), torch.randn(1, generator=g)
    keep = (torch.rand(N_, 512, generator=g) >= p).to(torch.uint8)
    y = torch.tensor([[1], [0], [1], [0]], dtype=torch.uint8)
    a4 = a5.reshape(N_, 16, 2, 512)                                                     # NHWC with H := D * H
    ref = H._reference(a4, w, b, keep, p, y, H.DLOSS)
    tol = H._bounds(a4, w, b, y, ref, H.DLOSS, dt == torch.bfloat16)
    model = NoduleClassifier().set_compute_dtype(dt)
    a5d = a5.to(DEV)
    view = model._head_input(a5d.permute(0, 4, 1, 2, 3))
    assert tuple(view.shape) == (N_, 512, 16, 2) and view.data_ptr() == a5d.data_ptr()          # a view of the tensor passed in, no copy
    wd, bd, yd, kd = w.to(DEV), b.to(DEV), y.to(DEV), keep.to(DEV)
    probs, pooled, loss = ops2d.cls_head_forward(view, wd, bd, dt, keep=kd, p=p, labels=yd)
    da, dw, db = ops2d.cls_head_backward(probs, yd, torch.tensor(H.DLOSS, device=DEV), pooled, wd, view, dt, keep=kd, p=p)
    got = dict(probs=probs.cpu(), pooled=pooled.cpu(), loss=loss.cpu(), da=da.permute(0, 2, 3, 1).cpu(), dw=dw.cpu(), db=db.cpu())
    for name in ("pooled", "probs", "loss", "dw", "db", "da"):
        err = (got[name].double() - ref[name]).abs()
        assert bool((err <= tol[name]).all()), f"{name}: error / bound = {float((err / tol[name].clamp_min(1e-300)).max()):.3f}"


def test_seeded_dropout_is_reproducible():
    x, y = _inputs()
    runs = []
    for _ in range(2):
        model = _classifier(torch.float32, dropout=0.5)
        model.mask_generator = torch.Generator(device=DEV).manual_seed(77)
        _begin_step()
        loss, probs = model.loss(x.to(DEV), y.to(DEV))
        loss.backward()
        torch.cuda.synchronize()
        runs.append((loss.detach(), probs, [p.grad for p in model.parameters()]))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][2], runs[1][2]))
    plain = _classifier(torch.float32)
    _begin_step()
    assert not torch.equal(plain.loss(x.to(DEV), y.to(DEV))[0].detach(), runs[0][0])        # the mask did something


# ---- 5. infer -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "bf16"])
def test_infer_against_eval_forward(dt):
    x, y = _inputs()
    xd, yd = x.to(DEV), y.to(DEV)
    model = _classifier(dt, dropout=0.2)
    _begin_step()
    model.loss(xd, yd)[0].backward()                        # running statistics that are no longer the initial ones
    for training in (True, False):
        model.train(training)
        before = {k: v.clone() for k, v in model.state_dict().items()}
        probs = model.infer(xd)
        probs2, loss = model.infer(xd, labels=yd)
        assert model.training is training and not probs.requires_grad and tuple(probs.shape) == (4, 1)
        assert torch.equal(probs, probs2)
        want = F.binary_cross_entropy(probs.double().cpu(), y.double())
        assert abs(float(loss) - float(want)) < 1e-5
        after = model.state_dict()
        assert all(torch.equal(after[k], before[k]) for k in before)
    model.eval()
    e = model(xd)
    err = check(probs, e.double().cpu(), dt, "infer vs model.eval()(x)")       # (synchronises every stream)
    print(f"[nodule {dt}] infer vs eval forward: max|d| = {err:.2e}")


# ---- 6. learning ----------------------------------------------------------------------------------------------------------------
def test_training_lowers_the_loss():
    x, y = next(iter(D.SyntheticNoduleLoader(8, 1, SHAPE, seed=4, device=DEV)))
    assert tuple(x.shape) == (8, 1) + SHAPE and y.dtype == torch.uint8 and 0 < int(y.sum()) < 8
    torch.manual_seed(0)
    model = NoduleClassifier(dropout=0.0).to(DEV)
    model.train()
    opt = FusedSGD(model.parameters(), lr=1e-2, momentum=0.9, weight_decay=1e-4)
    losses = [float(v) for v in torch.stack([train_step(model, opt, (x, y))[0] for _ in range(40)]).cpu()]
    print("[nodule] losses:", " ".join(f"{v:.3f}" for v in losses))
    assert np.mean(losses[-5:]) < np.mean(losses[:5])


# ---- 7. end to end --------------------------------------------------------------------------------------------------------------
CUBE = (32, 32, 16)


def _write_series(root):
    """Two series of about 48 x 40 x 44 mm: A at 1 mm with the identity matrix in subset0, B at (0.7, 0.7, 1.25) mm with x and y flipped in subset7.
    -> {name: (offset, diagonal)}"""
    rng = np.random.default_rng(8)
    a = "1.3.6.1.4.1.14519.5.2.1.111"
    b = "1.3.6.1.4.1.14519.5.2.1.222"
    (root / "subset0").mkdir(parents=True)
    (root / "subset7").mkdir()
    P.write_metaimage(str(root / "subset0" / (a + ".mhd")), rng.integers(-2000, 2000, (44, 40, 48)).astype(np.int16), (1.0, 1.0, 1.0), offset=(-20.0, 10.0, -100.0))
    pb = root / "subset7" / (b + ".mhd")
    P.write_metaimage(str(pb), rng.integers(-2000, 2000, (35, 57, 68)).astype(np.int16), (0.7, 0.7, 1.25), offset=(150.0, 160.0, -300.0))
    text = pb.read_text()
    assert "TransformMatrix = 1 0 0 0 1 0 0 0 1" in text
    pb.write_text(text.replace("TransformMatrix = 1 0 0 0 1 0 0 0 1", "TransformMatrix = -1 0 0 0 -1 0 0 0 1"))
    return {a: ((-20.0, 10.0, -100.0), (1, 1, 1)), b: ((150.0, 160.0, -300.0), (-1, -1, 1))}


def _write_candidates(path, series):
    """12 rows, 3 positive, the two series interleaved; voxel centres in the middle, at the edges and outside, some on half millimetres."""
    (a, (oa, da)), (b, (ob, db)) = series.items()
    vox = [(a, (24, 20, 22), 1), (b, (30, 18, 20), 0), (a, (2, 3, 1), 0), (a, (46.5, 38.5, 42.5), 0), (b, (5, 35, 40), 1), (a, (10, 30, 8), 1),
           (b, (44.5, 2.5, 3), 0), (a, (-4, 20, 50), 0), (b, (24, 20, 22), 0), (a, (30.25, 11.75, 30), 0), (b, (47, 39, 43), 0), (a, (16, 16, 8), 0)]
    lines = ["seriesuid,coordX,coordY,coordZ,class\n"]
    for s, v, lab in vox:
        o, d = (oa, da) if s == a else (ob, db)
        w = [o[k] + d[k] * v[k] for k in range(3)]
        lines.append(f"{s},{w[0]:.2f},{w[1]:.2f},{w[2]:.2f},{lab}\n")
    path.write_text("".join(lines))
    assert sum(v[2] for v in vox) == 3 and len(vox) == 12


def test_extract_train_predict_end_to_end(tmp_path, capsys, monkeypatch):
    """`--epochs` is the LAST epoch index (the project's convention): --epochs 1 trains epochs 0 and 1, and --val_every 2 validates after the second --
    one `Val:` line.  --ratio 0 without a series list (the working directory is the temporary one) keeps every series."""
    monkeypatch.chdir(tmp_path)
    raw, cubes_dir, out_dir, csv = tmp_path / "luna", tmp_path / "cubes", tmp_path / "out", tmp_path / "cand.csv"
    series = _write_series(raw)
    _write_candidates(csv, series)
    cands = N.read_candidates(str(csv))

    res = N.main(["extract", "--data", str(raw), "--candidates", str(csv), "--save", str(cubes_dir), "--cube", "32", "32", "16", "--negatives", "2", "--seed", "3"])
    assert res["series"] == 2 and not res["skipped"]
    kept = {}
    for fold, name in zip((0, 7), series):
        c = cands[name]
        cube_file = cubes_dir / f"subset{fold}" / (name + "_cand.npy")
        meta = np.load(str(cubes_dir / f"subset{fold}" / (name + "_cand_meta.npz")))
        got = np.load(str(cube_file))
        # the rule: every positive, rng.permutation(n_neg)[:2] of the negatives, sorted
        neg = np.flatnonzero(c.label == 0)
        r = np.random.default_rng([3, P.stable_hash(name)])
        keep = np.sort(np.concatenate([np.flatnonzero(c.label), neg[np.sort(r.permutation(neg.size)[:2])]]))
        assert got.dtype == np.int16 and got.shape == (len(keep),) + CUBE and len(keep) == int(c.label.sum()) + 2
        np.testing.assert_array_equal(meta["index"], c.index[keep])
        np.testing.assert_array_equal(meta["label"], c.label[keep])
        np.testing.assert_array_equal(meta["world"], c.world[keep])
        vol_zyx, spacing, hdr = P.read_metaimage(str(raw / f"subset{fold}" / (name + ".mhd")))
        vol = P.prepare_volume(vol_zyx, spacing, torch.device(DEV))[0].cpu().numpy()
        assert abs(vol.shape[2] - 48) <= 1 and abs(vol.shape[1] - 40) <= 1 and abs(vol.shape[0] - 44) <= 1
        offset, diag = series[name]
        np.testing.assert_array_equal(got, R.cubes(vol, R.world_to_start(c.world[keep], offset, diag, CUBE), CUBE))
        kept[name] = (c.index[keep], got)
    capsys.readouterr()

    model = N.main(["train", "--data", str(cubes_dir), "--phase", "scratch", "--epochs", "1", "--b", "4", "--val_folds", "7", "--test_folds", "7", "--save_best",
                    "--ratio", "0", "--val_every", "2", "--workers", "1", "--output", str(out_dir), "--gpus", "0"])
    text = capsys.readouterr().out
    best = out_dir / "pcrlv2_luna_nodules_scratch_0.0_best.pt"
    assert len(re.findall(r"^Val: \[1\]", text, re.M)) == 1 and len(re.findall(r"^Val:", text, re.M)) == 1 and len(re.findall(r"^Test: \(best epoch 1\)", text, re.M)) == 1, text
    assert best.exists() and model.test_metrics["n"] == 3
    ck = torch.load(str(best), map_location="cpu", weights_only=False)
    assert "classification_head.3.weight" in ck["state_dict"] and "down_tr64.ops.0.conv1.weight" in ck["state_dict"]

    scores = tmp_path / "scores.csv"
    args = ["predict", "--data", str(raw), "--candidates", str(csv), "--weights", str(best), "--out", str(scores), "--cube", "32", "32", "16", "--b", "5"]
    res = N.main(args)
    assert res["rows"] == 12 and res["series"] == 2
    rows = scores.read_text().splitlines()
    src = csv.read_text().splitlines()
    assert rows[0] == "seriesuid,coordX,coordY,coordZ,probability" and len(rows) == 13
    for got_line, src_line in zip(rows[1:], src[1:]):
        assert got_line.split(",")[:4] == src_line.split(",")[:4]                 # input order, coordinates echoed as text
    probs = np.array([float(line.split(",")[4]) for line in rows[1:]])
    assert np.all((probs > 0) & (probs < 1))
    clf = N.load_classifier(str(best), torch.device(DEV))
    for name, (index, cubes_np) in kept.items():
        p = clf.infer(D.normalise_cubes(torch.from_numpy(cubes_np).to(DEV)))
        check(p[:, 0], torch.from_numpy(probs[index]), torch.float32, f"predict vs infer on the extracted cubes of {name}")
    first = scores.read_bytes()
    N.main(args)
    assert scores.read_bytes() == first
