"""pcrl_seg_head_fwd / _bwd / _eval (csrc/seg_head.hip) against tests/seg_reference.py, a float64 torch restatement on the CPU (bf16 inputs upcast exactly).

Tolerances are derived, none is fitted (u = 2^-24, the float32 unit roundoff; ULP = 2^-23; sums of |terms| are taken in float64 from the reference):
  logit   E_z  = (64 + 8) u sum_c |W x| + u |b|                      64 fused multiply-adds and the shuffle sums; the bias add costs u (|d| + |b|), u |d| inside the + 8
  p       dp   = E_z / 4 + 4 ULP p                                   sigmoid is 1/4-Lipschitz; 4 ulps for exp and the division
  P, I    E_P  = sum_v dp, E_I = sum_v g dp (counted voxels)         the sums themselves run in float64 (+ (M + 8) 2^-53 of the sum); G and Mc are exact
  BCE_k   sum_v (E_z + 4 ULP |term|)                                 the loss term is 1-Lipschitz in the logit; 4 ulps for exp / log1p
  loss    wb sum_k E_BCE_k / (Mc K) + (wd / K) sum_k (2 E_I / U + (2 I + eps) E_P / U^2) + 2 ULP |loss|       U = P + G + eps; first order; the float32 result
  dz      the backward recomputes p (error dp again) and takes cA = c wb / (Mc K), e1 = (c wd / K) 2 / U, e0 = (c wd / K) (2 I + eps) / U^2 from the
          forward's sums:  dz = cA (p - g) - p (1 - p) (g e1 - e0)
          E_dz = (|cA| + |g e1 - e0|) dp                             d/dp of both terms, |1 - 2p| <= 1
               + (g de1 + de0) / 4                                   de1 = e1 E_P / U, de0 = |c wd / K| (2 E_I / U^2 + 2 (2 I + eps) E_P / U^3); p (1 - p) <= 1/4
               + 8 u (|cA| + g e1 + e0)                              the float32 casts of the coefficients and the handful of float32 operations
  dx      (K + 8) u sum_k |W dz| + sum_k |W| E_dz;   bf16: + 2^-8 |reference| for the one rounding of the output
  dW      d u sum_v |dz x| + sum_v |x| E_dz                          d = the longest chain of float32 additions a term goes through: the voxels of one
  db      d u sum_v |dz|  + sum_v E_dz                               lane, the shuffle and LDS combination of a block (<= 8 adds), the per-block partials of
                                                                     one range of the second launch and its 4 ranges (+ 8 slack); computed from the launch
                                                                     geometry in _chain() below, which restates the header's description of the grid
Uncounted voxels: exactly zero dx rows; all voxels uncounted: loss == wd * 0 and exactly zero dx, dW, db.
Every class count the dispatch knows, K = 1..7, is launched in both dtypes by the reference, the exact-eval and (tests/test_seg_blend_gpu.py,
tests/test_seg_mirror_gpu.py) the logits, accumulate and blend tests: FULL_KS with the whole shape and label lists, the others with REDUCED_SHAPES and
REDUCED_LABELS.  The loss weights wb, wd enter _bounds exactly as the lines above state them, and test_unequal_loss_weights_* runs the kernels, the eval
entry point and the autograd node with unequal ones: a swapped, dropped or doubled weight is invisible at (1, 1).
The exact part draws a, W, b from exact_lattice's FINER lattice: every logit is exact in float32 in any order, so the integer counts and the predicted
bitmask of the eval kernel must EQUAL the float64 reference's, ties at z = 0 included.
"""
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from exact_lattice import FINER, assert_exactly_summable, lattice, unit  # noqa: E402
from pcrlv2_amd import ops  # noqa: E402
from pcrlv2_amd._lib import dtype_code, lib, stream_handle  # noqa: E402
from seg_reference import reference  # noqa: E402

pytestmark = pytest.mark.gpu
U, ULP = 2.0 ** -24, 2.0 ** -23
C = 64
DLOSS = 0.75
# M in {1, 63, 64, 257, 4099} as N x spatial, then N = 3 samples of S = 70 voxels: three blocks per sample, so both factors of the partial-block index
# blockIdx.y * gridDim.x + blockIdx.x exceed 1
SHAPES = [(1, (1, 1, 1)), (3, (1, 3, 7)), (1, (4, 4, 4)), (1, (1, 1, 257)), (1, (1, 4099, 1)), (3, (2, 5, 7))]
LABELS = ("zeros", "ones", "mixed", "mixed30", "all_off")
ALL_KS = [1, 2, 3, 4, 5, 6, 7]
FULL_KS = (1, 3, 7)         # these run SHAPES x LABELS; the other class counts the lists below
# less than one block's voxels with N = 3; gx = 3 with N = 3; nine blocks, the last one partial
REDUCED_SHAPES = [(3, (1, 3, 7)), (3, (2, 5, 7)), (1, (1, 1, 257))]
REDUCED_LABELS = ("mixed30", "all_off", "ones")
WEIGHTS = [(0.25, 2.0), (2.0, 0.25), (0.0, 1.0), (1.0, 0.0), (0.0, 0.0)]      # all exact in float32
WEIGHT_SHAPES = [(3, (2, 5, 7)), (1, (1, 1, 257))]
_DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])


def _labels(kind, M, K, g):
    full = (1 << K) - 1
    if kind == "zeros":
        return torch.zeros(M, dtype=torch.uint8)
    if kind == "ones":
        return torch.full((M,), full, dtype=torch.uint8)
    lab = torch.randint(0, full + 1, (M,), generator=g).to(torch.uint8)
    if kind == "mixed30":
        lab = lab | ((torch.rand(M, generator=g) < 0.3).to(torch.uint8) << 7)
    if kind == "all_off":
        lab = lab | 0x80
    return lab


def _inputs(N, sp, K, dtype, kind, seed):
    g = torch.Generator().manual_seed(seed)
    M = N * sp[0] * sp[1] * sp[2]
    a = torch.relu(torch.randn(M, C, generator=g)).to(dtype)           # what the last decoder stage hands over: a ReLU output
    w = 0.2 * torch.randn(K, C, generator=g)
    b = torch.randn(K, generator=g)
    return a, w, b, _labels(kind, M, K, g)


def _act(a, N, sp):
    """[M, 64] rows -> the logical [N, 64, D, H, W] activation in NDHWC memory on the device."""
    return a.cuda().view(N, sp[0], sp[1], sp[2], C).permute(0, 4, 1, 2, 3)


def _run(a, w, b, lab, N, sp, dtype, dloss=DLOSS, wb=1.0, wd=1.0):
    ad, wd_, bd, ld = _act(a, N, sp), w.cuda(), b.cuda(), lab.cuda().view(N, *sp)
    loss, sums = ops.seg_head_forward(ad, wd_, bd, ld, dtype, wb, wd)
    dx, dw, db = ops.seg_head_backward(ad, wd_, bd, ld, sums, torch.tensor(dloss, device="cuda"), dtype, wb, wd)
    torch.cuda.synchronize()
    return dict(loss=loss.cpu(), sums=sums.cpu(), dx=dx.permute(0, 2, 3, 4, 1).reshape(-1, C).cpu(), dw=dw.cpu(), db=db.cpu())


def _chain(N, S, dtype):
    gx = min(-(-S // 32), max(1, 1024 // N))
    gpb = 32 if dtype == torch.bfloat16 else 16
    per_lane = -(-(-(-S // gpb)) // gx)
    return per_lane + 8 + -(-(gx * N) // 4) + 4 + 8


def _bounds(a, w, b, ref, K, N, S, dtype, dloss, wb=1.0, wd=1.0):
    """The module docstring's lines; `ref` is the reference computed with the same wb, wd."""
    A, W = a.double().abs(), w.double().abs()
    cnt = ref["counted"].double().unsqueeze(1)
    g, p = ref["g"], ref["p"]
    M = a.shape[0]
    e_z = (C + 8) * U * (A @ W.t()) + U * b.double().abs()
    dp = e_z / 4 + 4 * ULP * p
    E_P, E_I = (dp * cnt).sum(0) + (M + 8) * 2.0 ** -53 * ref["P"], (dp * g * cnt).sum(0) + (M + 8) * 2.0 ** -53 * ref["I"]
    t = {}
    Uk, num = ref["P"] + ref["G"] + 1.0, 2 * ref["I"] + 1.0
    Mc = ref["Mc"]
    e_bce = ((e_z + 4 * ULP * ref["terms"].abs()) * cnt).sum(0)
    t["sums"] = torch.cat([torch.stack([E_I, E_P, torch.zeros(K, dtype=torch.float64), e_bce], dim=1).reshape(-1), torch.zeros(1, dtype=torch.float64)])
    t["loss"] = (abs(wb) * e_bce.sum() / (Mc * K) if Mc else 0.0) + (abs(wd) / K) * (2 * E_I / Uk + num * E_P / Uk ** 2).sum() + 2 * ULP * ref["loss"].abs()
    c = abs(dloss)
    cA = c * abs(wb) / (Mc * K) if Mc else 0.0
    cd = c * abs(wd) / K
    e1, e0 = cd * 2 / Uk, cd * num / Uk ** 2
    de1, de0 = e1 * E_P / Uk, cd * (2 * E_I / Uk ** 2 + 2 * num * E_P / Uk ** 3)
    e_dz = ((cA + (g * e1 - e0).abs()) * dp + (g * de1 + de0) / 4 + 8 * U * (cA + g * e1 + e0)) * cnt          # [M, K]
    # dz of the reference itself: dL/dz, recovered from db's terms is not available per voxel -- restate it
    dz = (cA * (p - g) - p * (1 - p) * (g * e1 - e0)).abs() * cnt
    t["dx"] = (K + 8) * U * (dz @ W) + e_dz @ W
    if dtype == torch.bfloat16:
        t["dx"] = t["dx"] + 2.0 ** -8 * ref["dx"].abs()
    d = _chain(N, S, dtype)
    t["dw"] = d * U * (dz.t() @ A) + e_dz.t() @ A
    t["db"] = d * U * dz.sum(0) + e_dz.sum(0)
    return t


@pytest.mark.parametrize("K", ALL_KS)
@_DTYPES
def test_head_and_loss_against_float64_restatement(dtype, K):
    worst = {}
    shapes, labels = (SHAPES, LABELS) if K in FULL_KS else (REDUCED_SHAPES, REDUCED_LABELS)
    for si, (N, sp) in enumerate(shapes):
        S = sp[0] * sp[1] * sp[2]
        for li, kind in enumerate(labels):
            a, w, b, lab = _inputs(N, sp, K, dtype, kind, seed=10000 * K + 100 * si + 10 * li + (dtype == torch.bfloat16))
            ref = reference(a, w, b, lab, DLOSS)
            got = _run(a, w, b, lab, N, sp, dtype)
            tol = _bounds(a, w, b, ref, K, N, S, dtype, DLOSS)
            assert got["dx"].dtype == dtype and got["sums"].dtype == torch.float64
            assert float(got["sums"][4 * K]) == ref["Mc"] and torch.equal(got["sums"][2:4 * K:4], ref["G"]), "counted voxels and G are exact integers"
            for name in ("sums", "loss", "dx", "dw", "db"):
                err = (got[name].double() - ref[name]).abs()
                ratio = float((err / tol[name].clamp_min(1e-300)).max()) if float(err.max()) > 0 else 0.0
                worst[name] = max(worst.get(name, 0.0), ratio)
                assert bool((err <= tol[name]).all()), f"{name}: error / bound = {ratio:.3f} at N={N} spatial={sp} K={K} labels={kind} {dtype}"
            off = (lab & 0x80) != 0
            assert not bool(got["dx"][off].float().abs().any()), "dx rows of uncounted voxels are exactly zero"
            if kind == "all_off":
                assert float(got["loss"]) == 0.0 and not bool(got["dx"].float().abs().any()) and not bool(got["dw"].abs().any()) and not bool(got["db"].abs().any())
    print(f"[seg_head {dtype} K={K}] worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@_DTYPES
def test_capped_grid_where_a_lane_walks_several_voxels(dtype):
    """S > 32768: the grid is capped at 1024 blocks, every lane takes more than one voxel (the prefetching loop) -- same bounds.  K = 3, and K = 6
    (an instantiation the uncapped lists reach with their reduced shapes only)."""
    N, sp = 1, (3, 7, 1829)
    S = sp[0] * sp[1] * sp[2]
    for K in (3, 6):
        a, w, b, lab = _inputs(N, sp, K, dtype, "mixed30", seed=77 if K == 3 else 77 + K)
        ref = reference(a, w, b, lab, DLOSS)
        got = _run(a, w, b, lab, N, sp, dtype)
        tol = _bounds(a, w, b, ref, K, N, S, dtype, DLOSS)
        for name in ("sums", "loss", "dx", "dw", "db"):
            err = (got[name].double() - ref[name]).abs()
            print(f"[seg_head capped {dtype} K={K}] {name}: worst error / bound {float((err / tol[name].clamp_min(1e-300)).max()):.3f}")
            assert bool((err <= tol[name]).all()), f"{name} K={K}"


def _exact_inputs(N, sp, K, seed, kind="mixed30"):
    g = torch.Generator().manual_seed(seed)
    M = N * sp[0] * sp[1] * sp[2]
    a = lattice((M, C), *FINER["x"], g)
    w = lattice((K, C), *FINER["w"], g)
    b = lattice((K,), *FINER["b"], g)
    b[0] = 0.0
    a[::5] = 0.0                      # whole zero rows: z_0 = 0 exactly, a tie that must be predicted (z >= 0)
    assert_exactly_summable(a.abs() @ w.abs().t() + b.abs(), unit(FINER["x"][1], FINER["w"][1]), "seg head logits")
    return a, w, b, _labels(kind, M, K, g)


EVAL_CASES = [(1, (1, 1, 1), None, 1), (3, (1, 3, 7), [1, 0, 1], 2), (1, (1, 1, 257), [2], 3), (3, (5, 13, 21), [1, 0, 1], 2), (1, (1, 4099, 1), None, 1),
              (3, (2, 5, 7), [1, 0, 1], 2)]
REDUCED_EVAL_CASES = [(3, (1, 3, 7), [1, 0, 1], 2), (3, (2, 5, 7), [1, 0, 1], 2), (1, (1, 1, 257), [2], 3)]


@pytest.mark.parametrize("K", ALL_KS)
@_DTYPES
def test_eval_counts_and_mask_equal_the_reference_on_exactly_summable_operands(dtype, K):
    cases, kinds = (EVAL_CASES, ("mixed30",)) if K in FULL_KS else (REDUCED_EVAL_CASES, REDUCED_LABELS)
    for (N, sp, ci, n_cases), kind in [(c, k) for c in cases for k in kinds]:
        S = sp[0] * sp[1] * sp[2]
        a, w, b, lab = _exact_inputs(N, sp, K, seed=31 * K + S, kind=kind)
        ref = reference(a, w, b, lab, case_index=ci, n_cases=n_cases, S=S)
        assert int((ref["z"] == 0).sum()) > 0 or S == 1, "the case list must contain ties at z = 0"
        cid = None if ci is None else torch.tensor(ci, dtype=torch.int32, device="cuda")
        counts = torch.zeros((n_cases, K, 3), dtype=torch.int64, device="cuda")
        out = ops.seg_head_eval(_act(a.to(dtype), N, sp), w.float().cuda(), b.float().cuda(), dtype, labels=lab.cuda().view(N, *sp), case_index=cid,
                                counts=counts, want_mask=True)
        torch.cuda.synchronize()
        assert out[0] is counts and torch.equal(counts.cpu(), ref["counts"]), f"counts differ at N={N} spatial={sp} K={K} labels={kind}"
        assert torch.equal(out[3].reshape(-1).cpu(), ref["mask"]), f"mask differs at N={N} spatial={sp} K={K} labels={kind}"
        assert torch.equal(out[2].cpu()[2:4 * K:4], ref["G"]) and float(out[2][4 * K]) == ref["Mc"]
        # a second call ADDS to the table
        ops.seg_head_eval(_act(a.to(dtype), N, sp), w.float().cuda(), b.float().cuda(), dtype, labels=lab.cuda().view(N, *sp), case_index=cid, counts=counts)
        assert torch.equal(counts.cpu(), 2 * ref["counts"])
        # the eval loss is the forward's
        loss, sums = ops.seg_head_forward(_act(a.to(dtype), N, sp), w.float().cuda(), b.float().cuda(), lab.cuda().view(N, *sp), dtype)
        assert torch.equal(loss.cpu(), out[1].cpu()) and torch.equal(sums.cpu(), out[2].cpu())


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32 if t.dtype == torch.float32 else torch.int64)


@_DTYPES
def test_two_runs_are_bit_identical(dtype):
    for N, sp in [(3, (1, 3, 7)), (1, (1, 4099, 1)), (2, (8, 24, 100))]:
        a, w, b, lab = _inputs(N, sp, 3, dtype, "mixed30", seed=5)
        r1, r2 = _run(a, w, b, lab, N, sp, dtype), _run(a, w, b, lab, N, sp, dtype)
        for k in r1:
            assert torch.equal(_bits(r1[k]), _bits(r2[k])), k


@_DTYPES
def test_non_finite_activations_of_uncounted_voxels_enter_nothing(dtype):
    N, sp, K = 3, (2, 3, 7), 3
    a, w, b, lab = _inputs(N, sp, K, dtype, "mixed30", seed=21)
    off = (lab & 0x80) != 0
    assert int(off.sum()) > 3
    clean = a.clone()
    clean[off] = 0
    dirty = a.clone()
    dirty[off] = torch.tensor([float("nan"), float("inf"), -float("inf"), 1.0], dtype=dtype).repeat(C // 4)
    r0, r1 = _run(clean, w, b, lab, N, sp, dtype), _run(dirty, w, b, lab, N, sp, dtype)
    for k in r0:
        assert bool(torch.isfinite(r1[k].float()).all()) and torch.equal(_bits(r0[k]), _bits(r1[k])), k
    ad, ld = _act(dirty, N, sp), lab.cuda().view(N, *sp)
    counts, loss, sums, mask = ops.seg_head_eval(ad, w.cuda(), b.cuda(), dtype, labels=ld, want_mask=True)
    c0, l0, s0, m0 = ops.seg_head_eval(_act(clean, N, sp), w.cuda(), b.cuda(), dtype, labels=ld, want_mask=True)
    assert torch.equal(counts, c0) and torch.equal(_bits(loss), _bits(l0)) and torch.equal(sums, s0) and torch.equal(mask, m0)


@_DTYPES
def test_canary_bytes_behind_every_output_are_untouched(dtype):
    N, sp, K = 3, (1, 3, 7), 3
    S, M = 21, 63
    a, w, b, lab = _inputs(N, sp, K, dtype, "mixed30", seed=9)
    dev = torch.device("cuda")
    ad, wd_, bd, ld = _act(a, N, sp).permute(0, 2, 3, 4, 1).contiguous(), w.to(dev), b.to(dev), lab.to(dev)
    PAD = 64

    def padded(n, dt, fill):
        full = torch.full((n + PAD,), fill, dtype=dt, device=dev)
        return full, full[:n]

    sums_f, sums = padded(4 * K + 1, torch.float64, -7.0)
    loss_f, loss = padded(1, torch.float32, -7.0)
    dx_f, dx = padded(M * C, dtype, -7.0)
    dw_f, dw = padded(K * C, torch.float32, -7.0)
    db_f, db = padded(K, torch.float32, -7.0)
    mask_f, mask = padded(M, torch.uint8, 0xAB)
    cnt_f, cnt = padded(2 * K * 3, torch.int64, 0)
    cnt_f[2 * K * 3:] = -7
    nb = lib().call("pcrl_seg_head_ws_bytes", N, S, K)
    ws_f, ws = padded(nb, torch.uint8, 0xAB)
    L, code, s = lib(), dtype_code(dtype), stream_handle()
    ci = torch.tensor([1, 0, 1], dtype=torch.int32, device=dev)
    L.call("pcrl_seg_head_fwd", ad, wd_, bd, ld, sums, loss, 1.0, 1.0, ws, nb, N, S, K, code, s)
    L.call("pcrl_seg_head_bwd", ad, wd_, bd, ld, sums, torch.tensor([DLOSS], device=dev), 1.0, 1.0, dx, dw, db, ws, nb, N, S, K, code, s)
    L.call("pcrl_seg_head_eval", ad, wd_, bd, ld, ci, cnt, 2, mask, sums, loss, 1.0, 1.0, ws, nb, N, S, K, code, s)
    torch.cuda.synchronize()
    for name, full, n, fill in (("sums", sums_f, 4 * K + 1, -7.0), ("loss", loss_f, 1, -7.0), ("dx", dx_f, M * C, -7.0), ("dw", dw_f, K * C, -7.0),
                                ("db", db_f, K, -7.0), ("mask", mask_f, M, 0xAB), ("counts", cnt_f, 2 * K * 3, -7), ("workspace", ws_f, nb, 0xAB)):
        assert bool((full[n:].double() == float(fill)).all()), f"{name}: bytes behind the buffer were written"
    ref = reference(a, w, b, lab, DLOSS, case_index=[1, 0, 1], n_cases=2, S=S)
    assert int(cnt.sum()) > 0 and torch.equal(cnt.view(2, K, 3).cpu()[:, :, 2], ref["counts"][:, :, 2])
    with pytest.raises(RuntimeError):       # a short workspace is refused, not overrun
        L.call("pcrl_seg_head_fwd", ad, wd_, bd, ld, sums, loss, 1.0, 1.0, ws, nb - 1, N, S, K, code, s)
    with pytest.raises(RuntimeError):
        L.call("pcrl_seg_head_fwd", ad, wd_, bd, ld, sums, loss, 1.0, 1.0, ws, nb, N, S, 8, code, s)


@_DTYPES
def test_autograd_node_hands_over_the_raw_calls_gradients(dtype):
    from pcrlv2_amd import functions as Fn
    N, sp, K = 3, (2, 3, 7), 3
    a, w, b, lab = _inputs(N, sp, K, dtype, "mixed30", seed=11)
    seen = []
    for wb, wd in ((1.0, 1.0), (0.25, 2.0)):
        raw = _run(a, w, b, lab, N, sp, dtype, dloss=1.0, wb=wb, wd=wd)
        ad = _act(a, N, sp).requires_grad_(True)
        wp, bp = torch.nn.Parameter(w.cuda().view(K, C, 1, 1, 1)), torch.nn.Parameter(b.cuda())
        mod = types.SimpleNamespace(compute_dtype=dtype, _pass_idx=1)
        Fn.reset_parked()
        loss, sums = Fn.SegHeadFn.apply(ad, wp, bp, lab.cuda().view(N, *sp), wb, wd, mod)
        assert loss.requires_grad and not sums.requires_grad
        loss.backward()
        torch.cuda.synchronize()
        assert torch.equal(loss.detach().cpu(), raw["loss"]) and torch.equal(sums.cpu(), raw["sums"])
        assert torch.equal(_bits(ad.grad.permute(0, 2, 3, 4, 1).reshape(-1, C).cpu()), _bits(raw["dx"]))
        assert torch.equal(wp.grad.view(K, C).cpu(), raw["dw"]) and torch.equal(bp.grad.cpu(), raw["db"])
        seen.append(raw)
    assert not torch.equal(seen[0]["loss"], seen[1]["loss"]) and not torch.equal(seen[0]["dw"], seen[1]["dw"]), "the weights reach the loss and the gradients"


def _gap(x, y, tol):
    """Whether x and y differ by more than 100 x the bound somewhere: the weights under test are far from the ones they could be mistaken for."""
    return bool(((x - y).abs() > 100 * tol).any())


@pytest.mark.parametrize("K", [1, 4, 7])
@_DTYPES
def test_unequal_loss_weights_against_float64_restatement(dtype, K):
    """wb and wd multiply the two loss terms in the second launch of the forward and are folded into cA, e1, e0 of the backward; at (1, 1) a swap, a
    weight left out or one applied twice cannot be seen.  Bounds as above with the weights in them.  On top: the sums do not depend on the weights (bit for
    bit); at (0, 0) everything is exactly zero; the eval entry point's loss is the forward's bit for bit.  The test is not vacuous: at (0.25, 2.0) the
    REFERENCE's loss, dW and db are further than 100 x the bound from the references with the weights swapped and with unit weights."""
    worst = {}
    for si, (N, sp) in enumerate(WEIGHT_SHAPES):
        S = sp[0] * sp[1] * sp[2]
        a, w, b, lab = _inputs(N, sp, K, dtype, "mixed30", seed=20000 * K + 100 * si + (dtype == torch.bfloat16))
        ad, wdev, bdev, ld = _act(a, N, sp), w.cuda(), b.cuda(), lab.cuda().view(N, *sp)
        unit_sums = _run(a, w, b, lab, N, sp, dtype)["sums"]
        for wb, wd in WEIGHTS:
            where = f"at N={N} spatial={sp} K={K} wb={wb} wd={wd} {dtype}"
            ref = reference(a, w, b, lab, DLOSS, wb, wd)
            got = _run(a, w, b, lab, N, sp, dtype, wb=wb, wd=wd)
            tol = _bounds(a, w, b, ref, K, N, S, dtype, DLOSS, wb, wd)
            assert torch.equal(_bits(got["sums"]), _bits(unit_sums)), "the sums do not depend on the weights " + where
            for name in ("sums", "loss", "dx", "dw", "db"):
                err = (got[name].double() - ref[name]).abs()
                ratio = float((err / tol[name].clamp_min(1e-300)).max()) if float(err.max()) > 0 else 0.0
                worst[name] = max(worst.get(name, 0.0), ratio)
                assert bool((err <= tol[name]).all()), f"{name}: error / bound = {ratio:.3f} {where}"
            if (wb, wd) == (0.0, 0.0):
                assert float(got["loss"]) == 0.0 and not bool(got["dx"].float().abs().any()) and not bool(got["dw"].abs().any()) and not bool(got["db"].abs().any())
            if (wb, wd) == (0.25, 2.0):
                for other in (reference(a, w, b, lab, DLOSS, wd, wb), reference(a, w, b, lab, DLOSS, 1.0, 1.0)):
                    for name in ("loss", "dw", "db"):
                        assert _gap(ref[name], other[name], tol[name]), f"{name}: the reference does not tell these weights from others {where}"
            out = ops.seg_head_eval(ad, wdev, bdev, dtype, labels=ld, wb=wb, wd=wd)
            torch.cuda.synchronize()
            assert torch.equal(_bits(out[1].cpu()), _bits(got["loss"])) and torch.equal(_bits(out[2].cpu()), _bits(got["sums"])), "eval " + where
    print(f"[seg_head weights {dtype} K={K}] worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@_DTYPES
def test_bce_alone_still_moves_a_class_without_ground_truth(dtype):
    """wd = 0, K = 1, no voxel of the class anywhere: the Dice term is gone and G = 0, the BCE gradient cA (p - 0) is not."""
    N, sp, K = 3, (2, 5, 7), 1
    S = sp[0] * sp[1] * sp[2]
    a, w, b, lab = _inputs(N, sp, K, dtype, "zeros", seed=23)
    ref = reference(a, w, b, lab, DLOSS, 1.0, 0.0)
    got = _run(a, w, b, lab, N, sp, dtype, wb=1.0, wd=0.0)
    tol = _bounds(a, w, b, ref, K, N, S, dtype, DLOSS, 1.0, 0.0)
    assert float(got["sums"][2]) == 0.0 and float(ref["db"].abs().min()) > 100 * float(tol["db"].max()) and float(got["db"].abs().min()) > 0.0
    for name in ("sums", "loss", "dx", "dw", "db"):
        err = (got[name].double() - ref[name]).abs()
        print(f"[seg_head bce alone {dtype}] {name}: worst error / bound {float((err / tol[name].clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= tol[name]).all()), name


@_DTYPES
def test_backward_without_dx_leaves_dw_and_db_as_they_are(dtype):
    """need_dx=False hands the kernel a null dx: no dx comes back, dW and db are the bytes of the run that wrote one."""
    N, sp, K = 3, (2, 5, 7), 3
    a, w, b, lab = _inputs(N, sp, K, dtype, "mixed30", seed=13)
    ad, wdev, bdev, ld = _act(a, N, sp), w.cuda(), b.cuda(), lab.cuda().view(N, *sp)
    loss, sums = ops.seg_head_forward(ad, wdev, bdev, ld, dtype)
    dl = torch.tensor(DLOSS, device="cuda")
    dx, dw, db = ops.seg_head_backward(ad, wdev, bdev, ld, sums, dl, dtype)
    none, dw2, db2 = ops.seg_head_backward(ad, wdev, bdev, ld, sums, dl, dtype, need_dx=False)
    torch.cuda.synchronize()
    assert none is None and dx is not None and bool(dw.abs().sum() > 0)
    assert torch.equal(_bits(dw), _bits(dw2)) and torch.equal(_bits(db), _bits(db2))
