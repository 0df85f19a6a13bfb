"""pcrl_cls_head_fwd / _bwd (csrc/cls_head.hip) against a float64 torch restatement on the CPU of the literal module chain
adaptive_avg_pool2d -> mask / (1 - p) -> F.linear -> sigmoid -> F.binary_cross_entropy on the same inputs (bf16 inputs upcast exactly); its autograd
gives the three gradients.

Tolerances are derived (u = 2^-24, the float32 unit roundoff; |terms| are the absolute values of the products a sum runs over, taken in float64):
  pooled   (HW + 8) u sum_s |a| / HW                                             a sum of HW float32 values, then one division
  logit    E_z = (C + HW + 8) u (sum_c |W| mean_s|a| keep / (1 - p) + |b|)        a sum of C products of values that are sums of HW
  probs    dp = E_z / 4 + 4 ulp(p)        sigmoid is 1/4-Lipschitz; 4 float32 ulps (2^-23 relative) for exp and the division
  loss     mean(E_z) + 4 ulp(loss)        the loss term is 1-Lipschitz in the logit; 4 ulps for exp / log1p; the sums run in float64
  dW       (N + 8) u sum_n |dz gd| + sum_n (dp c |gd| + |dz| dpool keep / (1 - p))      c = dloss / (N K), dz = (p - y) c, gd = the dropped pooled vector:
                                                                                     a sum of N products + the first-order effect of the forward's own
                                                                                     error in p and in the pooled vector, which the backward reads
  db       (N + 8) u sum_n |dz| + sum_n dp c
  d_a      f ((K + 8) u sum_k |W dz| + sum_k |W| dp c),  f = keep / (1 - p) / HW;  bf16: + 2^-8 |reference| for the one rounding of the output
"""
import itertools
import os
import sys
import types

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import heads_eval_cases as hec  # noqa: E402
from pcrlv2_amd import ops2d  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
ULP = 2.0 ** -23
C = 512
DLOSS = 0.75


def _inputs(N, H, W, K, dtype, p, labels, seed, C=C):
    g = torch.Generator().manual_seed(seed)
    a = torch.relu(torch.randn(N, H, W, C, generator=g)).to(dtype)                 # what layer4 hands over: a ReLU output, NHWC memory
    w = 0.15 * torch.randn(K, C, generator=g)
    b = torch.randn(K, generator=g)
    keep = None if p is None else (torch.rand(N, C, generator=g) >= p).to(torch.uint8)
    y = {"zeros": torch.zeros(N, K), "ones": torch.ones(N, K), "mixed": (torch.rand(N, K, generator=g) < 0.5).float()}[labels].to(torch.uint8)
    return a, w, b, keep, y


def _reference(a, w, b, keep, p, y, dloss, C=C):
    """float64, CPU: the module chain and its autograd.  -> dict of float64 tensors"""
    assert a.shape[-1] == C and w.shape[1] == C
    a64 = a.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)          # [N,C,H,W], exact upcast
    w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
    pooled = F.adaptive_avg_pool2d(a64, 1).flatten(1)
    m = torch.ones_like(pooled) if keep is None else keep.double() / (1.0 - p)
    z = F.linear(pooled * m, w64, b64)
    assert float(z.detach().abs().max()) < 30.0, "the comparator's BCELoss would clamp its logarithm"
    pr = torch.sigmoid(z)
    loss = F.binary_cross_entropy(pr, y.double())
    da, dw, db = torch.autograd.grad(loss, (a64, w64, b64), grad_outputs=torch.tensor(dloss, dtype=torch.float64))
    return dict(pooled=pooled.detach(), z=z.detach(), probs=pr.detach(), loss=loss.detach(), da=da.permute(0, 2, 3, 1), dw=dw, db=db, m=m)


def _bounds(a, w, b, y, ref, dloss, bf16, C=C):
    N, H, W_, _ = a.shape
    assert a.shape[-1] == C
    HW, K = H * W_, w.shape[0]
    A = a.double().abs().reshape(N, HW, C)
    m = ref["m"]
    mean_abs = A.sum(1) / HW
    t = {}
    t["pooled"] = (HW + 8) * U * mean_abs
    e_z = (C + HW + 8) * U * ((mean_abs * m) @ w.double().abs().t() + b.double().abs())
    dp = e_z / 4 + 4 * ULP * ref["probs"]
    t["probs"] = dp
    t["loss"] = e_z.mean() + 4 * ULP * ref["loss"].abs()
    c = abs(dloss) / (N * K)
    dz = (ref["probs"] - y.double()).abs() * c                      # [N,K]
    gd = (ref["pooled"] * m).abs()                                  # [N,C]
    t["dw"] = (N + 8) * U * (dz.t() @ gd) + (dp * c).t() @ gd + dz.t() @ (t["pooled"] * m)
    t["db"] = (N + 8) * U * dz.sum(0) + (dp * c).sum(0)
    row = ((K + 8) * U * (dz @ w.double().abs()) + (dp * c) @ w.double().abs()) * m / HW      # [N,C]
    t["da"] = row.reshape(N, 1, 1, C).expand(N, H, W_, C)
    if bf16:
        t["da"] = t["da"] + 2.0 ** -8 * ref["da"].abs()
    return t


def _run(a, w, b, keep, p, y, dloss, dtype, C=C):
    dev = torch.device("cuda")
    assert a.shape[-1] == C
    ad = a.to(dev).permute(0, 3, 1, 2)                              # logical [N,C,H,W] in NHWC memory
    wd, bd, yd = w.to(dev), b.to(dev), y.to(dev)
    kd = None if keep is None else keep.to(dev)
    pp = 0.0 if p is None else p
    probs, pooled, loss = ops2d.cls_head_forward(ad, wd, bd, dtype, keep=kd, p=pp, labels=yd)
    da, dw, db = ops2d.cls_head_backward(probs, yd, torch.tensor(dloss, device=dev), pooled, wd, ad, dtype, keep=kd, p=pp)
    torch.cuda.synchronize()
    return dict(probs=probs.cpu(), pooled=pooled.cpu(), loss=loss.cpu(), da=da.permute(0, 2, 3, 1).cpu(), dw=dw.cpu(), db=db.cpu())


CASES = list(itertools.product((1, 3, 5), (1, 14, 15), (None, 0.2, 0.5), ("zeros", "ones", "mixed")))


@pytest.mark.parametrize("hw", [(1, 1), (2, 2), (3, 5), (7, 7)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_head_and_loss_against_float64_module_chain(dtype, hw):
    H, W = hw
    worst = {}
    for i, (N, K, p, labels) in enumerate(CASES):
        a, w, b, keep, y = _inputs(N, H, W, K, dtype, p, labels, seed=1000 * H + 10 * i + (dtype == torch.bfloat16))
        ref = _reference(a, w, b, keep, p, y, DLOSS)
        got = _run(a, w, b, keep, p, y, DLOSS, dtype)
        tol = _bounds(a, w, b, y, ref, DLOSS, dtype == torch.bfloat16)
        assert got["da"].dtype == dtype and got["probs"].dtype == torch.float32
        for name in ("pooled", "probs", "loss", "dw", "db", "da"):
            err = (got[name].double() - ref[name]).abs()
            ratio = float((err / tol[name].clamp_min(1e-300)).max())
            worst[name] = max(worst.get(name, 0.0), ratio)
            assert bool((err <= tol[name]).all()), f"{name}: error / bound = {ratio:.3f} at N={N} HW={hw} K={K} p={p} labels={labels} {dtype}"
    print(f"[cls_head {dtype} {hw}] worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_two_runs_are_bit_identical_and_null_labels_give_probabilities_only():
    dev = torch.device("cuda")
    for dtype in (torch.float32, torch.bfloat16):
        a, w, b, keep, y = _inputs(5, 7, 7, 14, dtype, 0.2, "mixed", seed=7)
        r1 = _run(a, w, b, keep, 0.2, y, DLOSS, dtype)
        r2 = _run(a, w, b, keep, 0.2, y, DLOSS, dtype)
        for k in r1:
            assert torch.equal(r1[k].view(torch.int16 if r1[k].dtype == torch.bfloat16 else torch.int32),
                               r2[k].view(torch.int16 if r2[k].dtype == torch.bfloat16 else torch.int32)), k
        ad = a.to(dev).permute(0, 3, 1, 2)
        probs, pooled, loss = ops2d.cls_head_forward(ad, w.to(dev), b.to(dev), dtype, keep=keep.to(dev), p=0.2)
        assert loss is None
        assert torch.equal(probs.cpu(), r1["probs"]) and torch.equal(pooled.cpu(), r1["pooled"])
        # eval: no mask -- the probabilities of the undropped pooled vector
        ref = _reference(a, w, b, None, None, y, DLOSS)
        pe = ops2d.cls_head_forward(ad, w.to(dev), b.to(dev), dtype)[0].cpu()
        tol = _bounds(a, w, b, y, ref, DLOSS, False)["probs"]
        assert bool(((pe.double() - ref["probs"]).abs() <= tol).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_autograd_node_hands_over_the_raw_calls_gradients(dtype):
    from pcrlv2_amd import functions as Fn
    from pcrlv2_amd.functions2d import ClsHeadFn
    dev = torch.device("cuda")
    a, w, b, keep, y = _inputs(3, 3, 5, 14, dtype, 0.5, "mixed", seed=11)
    raw = _run(a, w, b, keep, 0.5, y, 1.0, dtype)
    ad = a.to(dev).permute(0, 3, 1, 2).requires_grad_(True)
    wp, bp = torch.nn.Parameter(w.to(dev)), torch.nn.Parameter(b.to(dev))
    mod = types.SimpleNamespace(compute_dtype=dtype, _pass_idx=1)
    Fn.reset_parked()
    loss, probs = ClsHeadFn.apply(ad, wp, bp, y.to(dev), keep.to(dev), 0.5, mod)
    assert not probs.requires_grad and loss.requires_grad
    loss.backward()
    torch.cuda.synchronize()
    assert torch.equal(loss.detach().cpu(), raw["loss"]) and torch.equal(probs.cpu(), raw["probs"])
    assert torch.equal(ad.grad.permute(0, 2, 3, 1).cpu().float(), raw["da"].float())
    assert torch.equal(wp.grad.cpu(), raw["dw"]) and torch.equal(bp.grad.cpu(), raw["db"])


# ---- the other legal widths, the class and sample loops past their first trips (case lists: heads_eval_cases.py) ------------------------
def _check(N, H, W, K, p, labels, dtype, seed, Cw, worst):
    """one case with the assertions and bounds of test_head_and_loss_against_float64_module_chain; `worst` collects error / bound per output"""
    a, w, b, keep, y = _inputs(N, H, W, K, dtype, p, labels, seed, C=Cw)
    ref = _reference(a, w, b, keep, p, y, DLOSS, C=Cw)
    got = _run(a, w, b, keep, p, y, DLOSS, dtype, C=Cw)
    tol = _bounds(a, w, b, y, ref, DLOSS, dtype == torch.bfloat16, C=Cw)
    assert got["da"].dtype == dtype and got["probs"].dtype == torch.float32
    for name in ("pooled", "probs", "loss", "dw", "db", "da"):
        err = (got[name].double() - ref[name]).abs()
        ratio = float((err / tol[name].clamp_min(1e-300)).max())
        worst[name] = max(worst.get(name, 0.0), ratio)
        assert bool((err <= tol[name]).all()), f"{name}: error / bound = {ratio:.3f} at C={Cw} N={N} HW={(H, W)} K={K} p={p} labels={labels} {dtype}"


@pytest.mark.parametrize("Cw", hec.CLS_WIDTHS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_the_other_legal_widths(dtype, Cw):
    """C = 32 .. 256: NV = C / V vectors per pixel row and G = 256 / NV row groups up to 64 -- HW = 1, 15 and 65 lie below, inside and above G, so
    row groups are empty, partly filled and take a second trip; the `idx < C` loop of the forward takes one short trip."""
    worst = {}
    for i, ((H, W), N, K, p) in enumerate(itertools.product(hec.CLS_HW, (1, 3), (1, 14), (None, 0.5))):
        _check(N, H, W, K, p, "mixed", dtype, 5000 + 100 * Cw + 2 * i + (dtype == torch.bfloat16), Cw, worst)
    print(f"[cls_head {dtype} C={Cw}] worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("K", hec.CLS_WIDE_K)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_the_class_loop_up_to_the_largest_head(dtype, K):
    """K = 4, 5, 63, 64 at C = 512: the per-wave class loop takes one trip in every wave, a second in wave 0 only, sixteen with wave 3 one short,
    sixteen in every wave -- K = 64 = CH_MAX_K fills the backward's dz[]."""
    worst = {}
    for labels in ("mixed", "ones"):
        _check(3, 2, 2, K, 0.2, labels, dtype, 7000 + 10 * K + (dtype == torch.bfloat16), C, worst)
    print(f"[cls_head {dtype} K={K}] worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("Cw", [32, 512])
@pytest.mark.parametrize("N", hec.CLS_LONG_N)
def test_the_sample_loops_past_their_first_trip(N, Cw):
    """N = 65, 256, 257 (float32, HW = 1, K = 3): the stride-64 db sum takes a second trip; the loss kernel's stride-256 walk ends exactly at its
    first trip and takes a second one.  A sample dropped from the loss moves it by about loss / N = 4e-3 relative, the bound is near 1e-5."""
    worst = {}
    for p in (None, 0.5):
        _check(N, 1, 1, 3, p, "mixed", torch.float32, 9000 + N + Cw, Cw, worst)
    print(f"[cls_head N={N} C={Cw}] worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_rejections_launch_nothing():
    """host-side checks of cls_head_check and of the two entry points; H * W = 1 is accepted"""
    from pcrlv2_amd._lib import PcrlError, lib, stream_handle
    dev = torch.device("cuda")
    L, s = lib(), stream_handle()
    for Cw in (16, 48, 1024):
        for dtype in (torch.float32, torch.bfloat16):
            a = torch.zeros(2, 2, 2, Cw, dtype=dtype, device=dev).permute(0, 3, 1, 2)
            w, b = torch.zeros(3, Cw, device=dev), torch.zeros(3, device=dev)
            with pytest.raises(PcrlError, match=rf"cls_head_fwd: C must be a power of two in 32\.\.512 .*got {Cw}"):
                ops2d.cls_head_forward(a, w, b, dtype)
            with pytest.raises(PcrlError, match=rf"cls_head_bwd: C must be a power of two in 32\.\.512 .*got {Cw}"):
                ops2d.cls_head_backward(torch.zeros(2, 3, device=dev), torch.zeros(2, 3, dtype=torch.uint8, device=dev), torch.ones((), device=dev),
                                        torch.zeros(2, Cw, device=dev), w, a, dtype)
    with pytest.raises(PcrlError, match="unsupported activation dtype"):          # the wrapper does not let float16 through ...
        ops2d.cls_head_forward(torch.zeros(2, 2, 2, 32, dtype=torch.float16, device=dev).permute(0, 3, 1, 2), torch.zeros(3, 32, device=dev),
                               torch.zeros(3, device=dev), torch.float16)
    # raw calls: every pointer is a device buffer large enough for any size named below
    N, H, W, Cw = 2, 1, 1, 32
    f = lambda n: torch.full((n,), -7.0, device=dev)
    a, w, b, probs, pooled, loss = torch.zeros(N * Cw, device=dev), torch.zeros(65 * Cw, device=dev), torch.zeros(65, device=dev), f(N * 65), f(N * Cw), f(1)
    labels = torch.zeros(N * 65, dtype=torch.uint8, device=dev)
    nb = L.call("pcrl_cls_head_ws_bytes", N)
    ws = torch.zeros(nb, dtype=torch.uint8, device=dev)
    fwd = lambda K=3, code=0, labels_=labels, loss_=loss: L.call("pcrl_cls_head_fwd", a, None, 1.0, w, b, labels_, probs, pooled, loss_, ws, nb, N, H, W, Cw, K,
                                                                 code, s)
    for K in (0, 65):
        with pytest.raises(PcrlError, match=rf"cls_head_fwd: 1 <= K <= 64 classes, got {K}"):
            fwd(K=K)
        with pytest.raises(PcrlError, match=rf"cls_head_bwd: 1 <= K <= 64 classes, got {K}"):
            L.call("pcrl_cls_head_bwd", probs, labels, loss, pooled, None, 1.0, w, None, f(65 * Cw), f(65), N, H, W, Cw, K, 0, s)
    with pytest.raises(PcrlError, match="cls_head_fwd: labels and loss come together"):
        fwd(loss_=None)
    with pytest.raises(PcrlError, match="cls_head_fwd: labels and loss come together"):
        fwd(labels_=None)
    with pytest.raises(PcrlError, match="cls_head_fwd: dtype must be float32 or bfloat16"):   # ... and the entry point refuses its code (2)
        fwd(code=2)
    torch.cuda.synchronize()
    for name, t in (("probs", probs), ("pooled", pooled), ("loss", loss)):
        assert bool((t == -7.0).all()), f"{name} was written by a rejected call"
    fwd()                                                        # H * W = 1, zero inputs: every probability is sigmoid(0), the loss log 2
    torch.cuda.synchronize()
    assert bool((probs[:N * 3] == 0.5).all()) and bool((probs[N * 3:] == -7.0).all()) and bool((pooled == 0).all())
    assert abs(float(loss) - 0.6931471805599453) <= 2.0 ** -23
