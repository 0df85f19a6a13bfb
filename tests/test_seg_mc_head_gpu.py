"""pcrl_seg_mc_head_fwd / _bwd / _eval / _logits and the two label-map byte kernels (csrc/seg_head_mc.hip) against tests/seg_mc_reference.py, a float64
torch restatement on the CPU (bf16 inputs upcast exactly).

Tolerances are derived, none is fitted (u = 2^-24, the float32 unit roundoff; ULP = 2^-23; sums of |terms| are taken in float64 from the reference):
  logit   E_z  = (64 + 8) u sum_c |W x| + u |b|              64 fused multiply-adds and the tree's log2(LPV) <= 4 additions; the bias add is inside the + 8
          E    = max_j E_z_j of the voxel
  p       dp_k = 2 p_k (1 - p_k) E + r_k p_k                  sum_j |d p_k / d z_j| = 2 p_k (1 - p_k); the arithmetic's RELATIVE error of p_k = e_k / s is
          r_k  = (d_k + dbar) u + 8 ULP                       d_k = m - z_k: the rounding of the exponent's argument (z_k - m) moves e_k by d_k u
                                                              relatively, dbar = sum_j p_j d_j is the same for s; 8 ULP: expf twice (<= 2 ulp each),
                                                              the <= 5 additions of s (2.5), the division (0.5), 1 spare.  m is one of the computed
                                                              logits and cancels: it carries no error of its own
  P, I    E_P  = sum_v dp, E_I = sum_{y=k} dp (counted)       the sums themselves run in float64 (+ (M + 8) 2^-53 of the sum); G and Mc are exact
  ce      E_ce = 2 E + (d_y + dbar + ce) u + (6 + 2 ln K) ULP logsumexp(z) - z_y is 2-Lipschitz in the max norm; m - z_y and the final add round once
                                                              each; log s inherits s's relative error (dbar u + 4.5 ULP) and logf's 2 ulp of ln K
  CE_k    sum_{y=k} E_ce
  loss    wc sum_k E_CE_k / Mc + (wd / (K-1)) sum_{k>=1} (2 E_I / U + (2 I + 1) E_P / U^2) + 2 ULP |loss|       U = P + G + 1; first order
  dz      the backward recomputes p (error dp again) and takes cA = c wc / Mc, e1_k = (c wd / (K-1)) 2 / U_k, e0_k = (c wd / (K-1)) (2 I_k + 1) / U_k^2
          from the forward's sums; q_k = e0_k - [y=k] e1_k, S = sum_k p_k q_k:   dz_j = cA (p_j - [y=j]) + p_j (q_j - S)
          dq_k = de0_k + [y=k] de1_k + u (e0_k + [y=k] e1_k)  de1 = e1 E_P / U, de0 = |c wd / (K-1)| (2 E_I / U^2 + 2 (2 I + 1) E_P / U^3); the float32 casts
          dS   = sum_k (|q_k| dp_k + p_k dq_k) + 8 u sum_k p_k |q_k|       the products and the <= 5 additions of the butterfly
          E_dz = (|cA| + |q_j - S|) dp_j + p_j (dq_j + dS) + 8 u (|cA| |p_j - [y=j]| + p_j (|q_j| + sum_k p_k |q_k|))
  dx      (K + 8) u sum_k |W dz| + sum_k |W| E_dz;   bf16: + 2^-8 |reference| for the one rounding of the output
  dW      d u sum_v |dz x| + sum_v |x| E_dz                   d = the longest chain of float32 additions a term goes through: the voxels of one lane,
  db      d u sum_v |dz|  + sum_v E_dz                        the shuffle and LDS combination of a block (<= 8 adds), the per-block partials of one range
                                                              of the second launch and its 4 ranges (+ 8 slack); _chain() restates the launch geometry,
                                                              which is the sigmoid head's (tests/test_seg_head_gpu.py)
Uncounted voxels: exactly zero dx rows; all voxels uncounted: loss == 0 and exactly zero dx, dW, db.
Every class count the dispatch knows, K = 2..16, is launched in both dtypes by the reference, the exact-eval, the logits and the mirror tests here and by
tests/test_seg_mc_blend_gpu.py: KS with the whole shape and label lists, the others with REDUCED_SHAPES and REDUCED_LABELS.  The geometry changes with K
(McGeom in csrc/seg_head_mc.hip: KP = K rounded up to a power of two, CPL classes per lane, DUP lanes per class), and the padded classes K..KP-1 stay out
of the max, the sum, the argmin and the partial slots by guards alone, so every padding count matters.  The loss weights wc, wd enter forward_bounds and
_bounds exactly as the lines above state them, and test_unequal_loss_weights_* runs the kernels, the eval entry point and the autograd node with unequal
ones: a swapped, dropped or doubled weight is invisible at (1, 1).
The exact part draws a, W, b from exact_lattice's FINER lattice: every logit is exact in float32 in any order, so the maximum, its ties, the integer
counts and the predicted label map of the eval kernel must EQUAL the float64 reference's (lowest index among the tied classes).
"""
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from exact_lattice import FINER, assert_exactly_summable, lattice, unit  # noqa: E402
from pcrlv2_amd import ops  # noqa: E402
from pcrlv2_amd._lib import dtype_code, lib, stream_handle  # noqa: E402
from seg_mc_reference import lowest_argmax, reference  # noqa: E402

pytestmark = pytest.mark.gpu
U, ULP = 2.0 ** -24, 2.0 ** -23
C = 64
DLOSS = 0.75
KS = [2, 3, 8, 9, 16]       # the minimum, a non-power of two, bf16's lanes per voxel, one above it, the maximum: the whole shape and label lists
ALL_KS = list(range(2, 17))  # every instantiation; those not in KS run the reduced lists: 4 (KP == K, DUP = 4 / 2), 5..7 (KP = 8, padded), 10..15 (KP = 16,
#                              padded; at 15 the one padded class shares a lane with class 14 in bf16, where CPL = 2)
# M in {1, 63, 64, 257, 4099} as N x spatial, then N = 3 samples of S = 70 voxels: three blocks per sample, so both factors of the partial-block index
# blockIdx.y * gridDim.x + blockIdx.x exceed 1
SHAPES = [(1, (1, 1, 1)), (3, (1, 3, 7)), (1, (4, 4, 4)), (1, (1, 1, 257)), (1, (1, 4099, 1)), (3, (2, 5, 7))]
LABELS = ("background", "one_class", "mixed", "mixed30", "all_off")
# less than one block's voxels with N = 3; gx = 3 with N = 3; nine blocks, the last one partial
REDUCED_SHAPES = [(3, (1, 3, 7)), (3, (2, 5, 7)), (1, (1, 1, 257))]
REDUCED_LABELS = ("mixed30", "all_off", "one_class")
WEIGHTS = [(0.25, 2.0), (2.0, 0.25), (0.0, 1.0), (1.0, 0.0), (0.0, 0.0)]      # all exact in float32
WEIGHT_SHAPES = [(3, (2, 5, 7)), (1, (1, 1, 257))]
_DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])


def _labels(kind, M, K, g):
    if kind == "background":
        return torch.zeros(M, dtype=torch.uint8)
    if kind == "one_class":
        return torch.full((M,), K - 1, dtype=torch.uint8)
    lab = torch.randint(0, K, (M,), generator=g).to(torch.uint8)
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


def _run(a, w, b, lab, N, sp, dtype, dloss=DLOSS, wc=1.0, wd=1.0):
    ad, wd_, bd, ld = _act(a, N, sp), w.cuda(), b.cuda(), lab.cuda().view(N, *sp)
    loss, sums = ops.seg_mc_head_forward(ad, wd_, bd, ld, dtype, wc, wd)
    dx, dw, db = ops.seg_mc_head_backward(ad, wd_, bd, ld, sums, torch.tensor(dloss, device="cuda"), dtype, wc, wd)
    torch.cuda.synchronize()
    return dict(loss=loss.cpu(), sums=sums.cpu(), dx=dx.permute(0, 2, 3, 4, 1).reshape(-1, C).cpu(), dw=dw.cpu(), db=db.cpu())


def _chain(N, S, dtype):
    gx = min(-(-S // 32), max(1, 1024 // N))
    gpb = 32 if dtype == torch.bfloat16 else 16
    per_lane = -(-(-(-S // gpb)) // gx)
    return per_lane + 8 + -(-(gx * N) // 4) + 4 + 8


def forward_bounds(e_z, ref, K, M, s_adds=5, wc=1.0, wd=1.0):
    """The docstring's p, P, I, ce, CE and loss lines from the logit bound e_z [M, K].  s_adds: the float32 additions that form s (the head's butterfly: at
    most 5; a serial sum over K classes: K - 1), each worth half an ulp in r_k and in log s.  wc, wd: the weights `ref` was computed with.
    -> dict with dp [M, K], E_P, E_I, E_CE [K], sums, loss"""
    cnt = ref["counted"].double().unsqueeze(1)
    g, p = ref["g"], ref["p"]
    emax = e_z.max(1, keepdim=True).values
    d = ref["m"].unsqueeze(1) - ref["z"]
    dbar = (p * d).sum(1, keepdim=True)
    more = (s_adds - 5) / 2.0
    dp = 2 * p * (1 - p) * emax + ((d + dbar) * U + (8 + more) * ULP) * p
    f64 = (M + 8) * 2.0 ** -53
    E_P, E_I = (dp * cnt).sum(0) + f64 * ref["P"], (dp * g * cnt).sum(0) + f64 * ref["I"]
    d_y = (d * g).sum(1, keepdim=True)
    e_ce = (2 * emax + (d_y + dbar + ref["ce"].unsqueeze(1)) * U + (6 + more + 2 * math.log(K)) * ULP) * cnt
    E_CE = (e_ce * g).sum(0) + f64 * ref["CE"]
    Uk, num = ref["P"] + ref["G"] + 1.0, 2 * ref["I"] + 1.0
    Mc = ref["Mc"]
    t = dict(dp=dp, E_P=E_P, E_I=E_I, E_CE=E_CE)
    t["sums"] = torch.cat([torch.stack([E_I, E_P, torch.zeros(K, dtype=torch.float64), E_CE], dim=1).reshape(-1), torch.zeros(1, dtype=torch.float64)])
    t["loss"] = (abs(wc) * E_CE.sum() / Mc if Mc else 0.0) + (abs(wd) / (K - 1)) * (2 * E_I / Uk + num * E_P / Uk ** 2)[1:].sum() + 2 * ULP * ref["loss"].abs()
    return t


def _bounds(a, w, b, ref, K, N, S, dtype, dloss, wc=1.0, wd=1.0):
    """The module docstring's lines; `ref` is the reference computed with the same wc, wd."""
    cntb = ref["counted"]
    cnt = cntb.double().unsqueeze(1)
    A, W = torch.where(cntb.unsqueeze(1), a.double().abs(), torch.zeros(1, dtype=torch.float64)), w.double().abs()
    g, p = ref["g"], ref["p"]
    M = a.shape[0]
    e_z = (C + 8) * U * (A @ W.t()) + U * b.double().abs()
    t = forward_bounds(e_z, ref, K, M, wc=wc, wd=wd)
    dp, E_P, E_I = t["dp"], t["E_P"], t["E_I"]
    Uk, num = ref["P"] + ref["G"] + 1.0, 2 * ref["I"] + 1.0
    Mc = ref["Mc"]
    c = abs(dloss)
    cA = c * abs(wc) / Mc if Mc else 0.0
    cd = c * abs(wd) / (K - 1)
    e1, e0 = cd * 2 / Uk, cd * num / Uk ** 2
    de1, de0 = e1 * E_P / Uk, cd * (2 * E_I / Uk ** 2 + 2 * num * E_P / Uk ** 3)
    for v in (e1, e0, de1, de0):
        v[0] = 0.0                                      # the background has no Dice term
    q, spq = ref["q"].abs(), ref["spq"]
    dq = de0 + g * de1 + U * (e0 + g * e1)
    sabs = (p * q).sum(1, keepdim=True)
    dS = (q * dp + p * dq).sum(1, keepdim=True) + 8 * U * sabs
    e_dz = ((cA + (ref["q"] - spq).abs()) * dp + p * (dq + dS) + 8 * U * (cA * (p - g).abs() + p * (q + sabs))) * cnt          # [M, K]
    dz = ref["dz"].abs()
    t["dx"] = (K + 8) * U * (dz @ W) + e_dz @ W
    if dtype == torch.bfloat16:
        t["dx"] = t["dx"] + 2.0 ** -8 * ref["dx"].abs()
    dch = _chain(N, S, dtype)
    t["dw"] = dch * U * (dz.t() @ A) + e_dz.t() @ A
    t["db"] = dch * U * dz.sum(0) + e_dz.sum(0)
    return t


def _check(got, ref, tol, K, worst, where):
    assert float(got["sums"][4 * K]) == ref["Mc"] and torch.equal(got["sums"][2:4 * K:4], ref["G"]), f"counted voxels and G are exact integers {where}"
    for name in ("sums", "loss", "dx", "dw", "db"):
        err = (got[name].double() - ref[name]).abs()
        ratio = float((err / tol[name].clamp_min(1e-300)).max()) if float(err.max()) > 0 else 0.0
        worst[name] = max(worst.get(name, 0.0), ratio)
        assert bool((err <= tol[name]).all()), f"{name}: error / bound = {ratio:.3f} {where}"


@pytest.mark.parametrize("K", ALL_KS)
@_DTYPES
def test_head_and_loss_against_float64_restatement(dtype, K):
    worst = {}
    shapes, labels = (SHAPES, LABELS) if K in KS else (REDUCED_SHAPES, REDUCED_LABELS)
    for si, (N, sp) in enumerate(shapes):
        S = sp[0] * sp[1] * sp[2]
        for li, kind in enumerate(labels):
            a, w, b, lab = _inputs(N, sp, K, dtype, kind, seed=10000 * K + 100 * si + 10 * li + (dtype == torch.bfloat16))
            ref = reference(a, w, b, lab, DLOSS)
            got = _run(a, w, b, lab, N, sp, dtype)
            tol = _bounds(a, w, b, ref, K, N, S, dtype, DLOSS)
            assert got["dx"].dtype == dtype and got["sums"].dtype == torch.float64
            _check(got, ref, tol, K, worst, f"at N={N} spatial={sp} K={K} labels={kind} {dtype}")
            off = (lab & 0x80) != 0
            assert not bool(got["dx"][off].float().abs().any()), "dx rows of uncounted voxels are exactly zero"
            if kind == "all_off":
                assert float(got["loss"]) == 0.0 and not bool(got["dx"].float().abs().any()) and not bool(got["dw"].abs().any()) and not bool(got["db"].abs().any())
    print(f"[seg_mc_head {dtype} K={K}] worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("K", [5, 9, 15, 16])
@_DTYPES
def test_capped_grid_where_a_lane_walks_several_voxels(dtype, K):
    """S > 32768: the grid is capped at 1024 blocks, every lane takes more than one voxel (the prefetching loop) -- same bounds.  One padded class count
    per KP range (5 in 8, 9 and 15 in 16) and the maximum."""
    N, sp = 1, (3, 7, 1829)
    S = sp[0] * sp[1] * sp[2]
    a, w, b, lab = _inputs(N, sp, K, dtype, "mixed30", seed=77 + K)
    ref = reference(a, w, b, lab, DLOSS)
    got = _run(a, w, b, lab, N, sp, dtype)
    tol = _bounds(a, w, b, ref, K, N, S, dtype, DLOSS)
    worst = {}
    _check(got, ref, tol, K, worst, f"capped grid K={K} {dtype}")
    print(f"[seg_mc_head capped {dtype} K={K}] worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_a_label_outside_the_classes_is_not_counted():
    """y >= K is the host's to refuse; on the device such a voxel is harmless: it is treated as not counted."""
    N, sp, K, dtype = 2, (2, 3, 7), 3, torch.float32
    a, w, b, lab = _inputs(N, sp, K, dtype, "mixed", seed=3)
    bad = lab.clone()
    bad[::4] = 5
    off = lab.clone()
    off[::4] |= 0x80
    r0, r1 = _run(a, w, b, off, N, sp, dtype), _run(a, w, b, bad, N, sp, dtype)
    for k in r0:
        assert torch.equal(_bits(r0[k]), _bits(r1[k])), k
    # the labels a padded class would answer to: K (the first one), KP - 1 (the last one), 16 (past every KP) and 127 (the largest a byte carries)
    for K in (3, 5, 9, 13):
        KP = 4 if K <= 4 else 8 if K <= 8 else 16
        for dtype in (torch.float32, torch.bfloat16):
            a, w, b, lab = _inputs(N, sp, K, dtype, "mixed", seed=3 + K)
            off = lab.clone()
            off[::4] |= 0x80
            ad, wdev, bdev = _act(a, N, sp), w.cuda(), b.cuda()
            r0 = _run(a, w, b, off, N, sp, dtype)
            e0 = ops.seg_mc_head_eval(ad, wdev, bdev, dtype, labels=off.cuda().view(N, *sp), want_mask=True)
            for y in sorted({v for v in (K, KP - 1, 16, 127) if v >= K}):
                bad = lab.clone()
                bad[::4] = y
                r1 = _run(a, w, b, bad, N, sp, dtype)
                for k in r0:
                    assert torch.equal(_bits(r0[k]), _bits(r1[k])), f"{k}: label {y} at K={K} {dtype}"
                e1 = ops.seg_mc_head_eval(ad, wdev, bdev, dtype, labels=bad.cuda().view(N, *sp), want_mask=True)
                assert torch.equal(e0[0], e1[0]) and torch.equal(e0[2], e1[2]) and torch.equal(e0[3], e1[3]), f"eval: label {y} at K={K} {dtype}"


def _exact_inputs(N, sp, K, seed, kind="mixed30"):
    g = torch.Generator().manual_seed(seed)
    M = N * sp[0] * sp[1] * sp[2]
    a = lattice((M, C), *FINER["x"], g)
    w = lattice((K, C), *FINER["w"], g)
    b = lattice((K,), *FINER["b"], g)
    b[0] = b[1] = 1.0                 # the lattice's largest bias, twice
    a[::5] = 0.0                      # whole zero rows: z = b exactly, the maximum is shared by the classes 0 and 1 -> 0 is predicted
    if K >= 3:                        # classes 1 and 2 are the same function: wherever they lead, 1 is predicted
        w[2], b[2] = w[1], b[1]
    assert_exactly_summable(a.abs() @ w.abs().t() + b.abs(), unit(FINER["x"][1], FINER["w"][1]), "seg mc head logits")
    return a, w, b, _labels(kind, M, K, g)


EVAL_CASES = [(1, (1, 1, 1), None, 1), (3, (1, 3, 7), [1, 0, 1], 2), (1, (1, 1, 257), [2], 3), (3, (5, 13, 21), [1, 5, 1], 2), (1, (1, 4099, 1), None, 1),
              (3, (2, 5, 7), [1, 0, 1], 2)]
REDUCED_EVAL_CASES = [(3, (1, 3, 7), [1, 0, 1], 2), (3, (2, 5, 7), [1, 0, 1], 2), (1, (1, 1, 257), [2], 3)]
EVAL_FULL_KS = (2, 3, 9, 16)


@pytest.mark.parametrize("K", ALL_KS)
@_DTYPES
def test_eval_counts_and_label_map_equal_the_reference_on_exactly_summable_operands(dtype, K):
    cases, kinds = (EVAL_CASES, ("mixed30",)) if K in EVAL_FULL_KS else (REDUCED_EVAL_CASES, REDUCED_LABELS)
    for (N, sp, ci, n_cases), kind in [(c, k) for c in cases for k in kinds]:
        S = sp[0] * sp[1] * sp[2]
        a, w, b, lab = _exact_inputs(N, sp, K, seed=31 * K + S, kind=kind)
        ref = reference(a, w, b, lab, case_index=ci, n_cases=n_cases, S=S)
        tied = (ref["z"] == ref["z"].max(1, keepdim=True).values).sum(1) >= 2
        assert int(tied.sum()) > 0, "the case list must contain voxels whose maximum is shared by two classes"
        if K >= 3 and S > 1 and kind == "mixed30":
            assert int((tied & (ref["pred"] >= 1) & ref["counted"]).sum()) > 0, "... and ties whose lowest class is not the background"
        cid = None if ci is None else torch.tensor(ci, dtype=torch.int32, device="cuda")
        counts = torch.zeros((n_cases, K, 3), dtype=torch.int64, device="cuda")
        out = ops.seg_mc_head_eval(_act(a.to(dtype), N, sp), w.float().cuda(), b.float().cuda(), dtype, labels=lab.cuda().view(N, *sp), case_index=cid,
                                   counts=counts, want_mask=True)
        torch.cuda.synchronize()
        assert out[0] is counts and torch.equal(counts.cpu(), ref["counts"]), f"counts differ at N={N} spatial={sp} K={K} labels={kind}"
        assert torch.equal(out[3].reshape(-1).cpu(), ref["labelmap"]), f"label map differs at N={N} spatial={sp} K={K} labels={kind}"
        assert torch.equal(out[2].cpu()[2:4 * K:4], ref["G"]) and float(out[2][4 * K]) == ref["Mc"]
        # a second call ADDS to the table
        ops.seg_mc_head_eval(_act(a.to(dtype), N, sp), w.float().cuda(), b.float().cuda(), dtype, labels=lab.cuda().view(N, *sp), case_index=cid, counts=counts)
        assert torch.equal(counts.cpu(), 2 * ref["counts"])
        # the eval loss is the forward's
        loss, sums = ops.seg_mc_head_forward(_act(a.to(dtype), N, sp), w.float().cuda(), b.float().cuda(), lab.cuda().view(N, *sp), dtype)
        assert torch.equal(loss.cpu(), out[1].cpu()) and torch.equal(sums.cpu(), out[2].cpu())
        # the logits are the exact ones, and without labels every voxel is predicted
        z = ops.seg_mc_head_logits(_act(a.to(dtype), N, sp), w.float().cuda(), b.float().cuda(), dtype)
        zr = (a @ w.t() + b).float()
        assert torch.equal(z.reshape(-1, K).cpu(), zr)
        free = ops.seg_mc_head_eval(_act(a.to(dtype), N, sp), w.float().cuda(), b.float().cuda(), dtype, want_mask=True)
        assert torch.equal(free[3].reshape(-1).cpu(), lowest_argmax(zr.double()).to(torch.uint8))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32 if t.dtype == torch.float32 else torch.int64)


@pytest.mark.parametrize("K", ALL_KS)
@_DTYPES
def test_argmax_of_the_logits_is_the_eval_label_map(dtype, K):
    for N, sp in [(3, (1, 3, 7)), (2, (3, 5, 7)), (1, (1, 4099, 1)), (3, (2, 5, 7))] if K in KS else REDUCED_SHAPES:
        a, w, b, _ = _inputs(N, sp, K, dtype, "mixed", seed=40 + K)
        ad, wd_, bd = _act(a, N, sp), w.cuda(), b.cuda()
        z = ops.seg_mc_head_logits(ad, wd_, bd, dtype)
        _, _, _, lm = ops.seg_mc_head_eval(ad, wd_, bd, dtype, want_mask=True)
        torch.cuda.synchronize()
        assert z.shape == (N, *sp, K) and torch.equal(lowest_argmax(z.cpu().double()).to(torch.uint8), lm.cpu())
        # the logit is the restatement's within E_z
        zr = a.double() @ w.double().t() + b.double()
        e_z = (C + 8) * U * (a.double().abs() @ w.double().abs().t()) + U * b.double().abs()
        assert bool(((z.cpu().double().reshape(-1, K) - zr).abs() <= e_z).all())


@pytest.mark.parametrize("K", [2, 9, 16])
@_DTYPES
def test_logits_with_a_mirror_are_the_plain_logits_permuted_and_accumulate_as_stated(dtype, K):
    N, sp = 2, (3, 5, 7)
    a, w, b, _ = _inputs(N, sp, K, dtype, "mixed", seed=50 + K)
    ad, wd_, bd = _act(a, N, sp), w.cuda(), b.cuda()
    plain = ops.seg_mc_head_logits(ad, wd_, bd, dtype)
    for flip in range(8):
        dims = [d + 1 for d in range(3) if flip >> d & 1]
        want = plain.flip(dims) if dims else plain
        out = torch.full_like(plain, float("nan"))
        got = ops.seg_mc_head_logits(ad, wd_, bd, dtype, out=out, flip=flip)
        assert got.data_ptr() == out.data_ptr() and torch.equal(_bits(got), _bits(want.contiguous())), f"flip {flip}"
        # first = 0: v = out + z; out = v * scale -- one add, one multiply, plain float32
        prev = torch.randn(plain.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(flip))
        acc = prev.clone()
        ops.seg_mc_head_logits(ad, wd_, bd, dtype, out=acc, flip=flip, first=False, scale=0.375)
        assert torch.equal(_bits(acc), _bits((prev + want) * torch.tensor(0.375, device="cuda"))), f"accumulate, flip {flip}"
        sc = plain.clone()
        ops.seg_mc_head_logits(ad, wd_, bd, dtype, out=sc, flip=flip, first=True, scale=1.0 / 3.0)
        assert torch.equal(_bits(sc), _bits(want * torch.tensor(1.0 / 3.0, device="cuda"))), f"first with a scale, flip {flip}"


@pytest.mark.parametrize("K", [k for k in ALL_KS if k not in (2, 9, 16)])
@_DTYPES
def test_mirrored_and_accumulated_logits_at_the_other_class_counts(dtype, K):
    """The accumulating store of every class count the test above leaves out: one sequence of passes with a z mirror (code 4), an x mirror and a
    non-first pass, the last one scaled -- plain float32, restated on the device with torch (one add per pass, one multiply)."""
    N, sp = 2, (3, 5, 7)
    a, w, b, _ = _inputs(N, sp, K, dtype, "mixed", seed=50 + K)
    ad, wd_, bd = _act(a, N, sp), w.cuda(), b.cuda()
    plain = ops.seg_mc_head_logits(ad, wd_, bd, dtype)
    zr = a.double() @ w.double().t() + b.double()
    e_z = (C + 8) * U * (a.double().abs() @ w.double().abs().t()) + U * b.double().abs()
    assert bool(((plain.cpu().double().reshape(-1, K) - zr).abs() <= e_z).all())
    un = lambda code: plain.flip([d + 1 for d in range(3) if code >> d & 1]).contiguous() if code else plain      # noqa: E731
    out = torch.full_like(plain, float("nan"))
    ops.seg_mc_head_logits(ad, wd_, bd, dtype, out=out, flip=4, first=True)
    assert torch.equal(_bits(out), _bits(un(4))), "a first pass with a z mirror"
    ops.seg_mc_head_logits(ad, wd_, bd, dtype, out=out, flip=1, first=False)
    ops.seg_mc_head_logits(ad, wd_, bd, dtype, out=out, flip=6, first=False, scale=1.0 / 3.0)
    assert torch.equal(_bits(out), _bits(((un(4) + un(1)) + un(6)) * torch.tensor(1.0 / 3.0, device="cuda"))), "three passes, the last one scaled"


@_DTYPES
def test_two_runs_are_bit_identical(dtype):
    for K, N, sp in [(3, 3, (1, 3, 7)), (9, 1, (1, 4099, 1)), (16, 2, (8, 24, 100))]:
        a, w, b, lab = _inputs(N, sp, K, dtype, "mixed30", seed=5)
        r1, r2 = _run(a, w, b, lab, N, sp, dtype), _run(a, w, b, lab, N, sp, dtype)
        for k in r1:
            assert torch.equal(_bits(r1[k]), _bits(r2[k])), k


@pytest.mark.parametrize("K", [3, 16])
@_DTYPES
def test_non_finite_activations_of_uncounted_voxels_enter_nothing(dtype, K):
    N, sp = 3, (2, 3, 7)
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
    counts, loss, sums, lm = ops.seg_mc_head_eval(ad, w.cuda(), b.cuda(), dtype, labels=ld, want_mask=True)
    c0, l0, s0, m0 = ops.seg_mc_head_eval(_act(clean, N, sp), w.cuda(), b.cuda(), dtype, labels=ld, want_mask=True)
    assert torch.equal(counts, c0) and torch.equal(_bits(loss), _bits(l0)) and torch.equal(sums, s0) and torch.equal(lm, m0)


@pytest.mark.parametrize("K", [3, 16])
@_DTYPES
def test_canary_bytes_behind_every_output_are_untouched(dtype, K):
    N, sp = 3, (1, 3, 7)
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
    lm_f, lm = padded(M, torch.uint8, 0xAB)
    z_f, z = padded(M * K, torch.float32, -7.0)
    cnt_f, cnt = padded(2 * K * 3, torch.int64, 0)
    cnt_f[2 * K * 3:] = -7
    nb = lib().call("pcrl_seg_mc_head_ws_bytes", N, S, K)
    ws_f, ws = padded(nb, torch.uint8, 0xAB)
    L, code, s = lib(), dtype_code(dtype), stream_handle()
    ci = torch.tensor([1, 0, 1], dtype=torch.int32, device=dev)
    L.call("pcrl_seg_mc_head_fwd", ad, wd_, bd, ld, sums, loss, 1.0, 1.0, ws, nb, N, S, K, code, s)
    L.call("pcrl_seg_mc_head_bwd", ad, wd_, bd, ld, sums, torch.tensor([DLOSS], device=dev), 1.0, 1.0, dx, dw, db, ws, nb, N, S, K, code, s)
    L.call("pcrl_seg_mc_head_eval", ad, wd_, bd, ld, ci, cnt, 2, lm, sums, loss, 1.0, 1.0, ws, nb, N, S, K, code, s)
    L.call("pcrl_seg_mc_head_logits", ad, wd_, bd, z, N, S, K, code, 1, 3, 7, 5, 1, 1.0, s)
    torch.cuda.synchronize()
    for name, full, n, fill in (("sums", sums_f, 4 * K + 1, -7.0), ("loss", loss_f, 1, -7.0), ("dx", dx_f, M * C, -7.0), ("dw", dw_f, K * C, -7.0),
                                ("db", db_f, K, -7.0), ("labelmap", lm_f, M, 0xAB), ("logits", z_f, M * K, -7.0), ("counts", cnt_f, 2 * K * 3, -7),
                                ("workspace", ws_f, nb, 0xAB)):
        assert bool((full[n:].double() == float(fill)).all()), f"{name}: bytes behind the buffer were written"
    assert not bool((z == -7.0).any()), "every logit is written"
    ref = reference(a, w, b, lab, DLOSS, case_index=[1, 0, 1], n_cases=2, S=S)
    assert int(cnt.sum()) > 0 and torch.equal(cnt.view(2, K, 3).cpu()[:, :, 2], ref["counts"][:, :, 2])
    with pytest.raises(RuntimeError):       # a short workspace is refused, not overrun
        L.call("pcrl_seg_mc_head_fwd", ad, wd_, bd, ld, sums, loss, 1.0, 1.0, ws, nb - 1, N, S, K, code, s)
    for bad_k in (1, 17):
        with pytest.raises(RuntimeError):
            L.call("pcrl_seg_mc_head_fwd", ad, wd_, bd, ld, sums, loss, 1.0, 1.0, ws, nb, N, S, bad_k, code, s)
        assert L.call("pcrl_seg_mc_head_ws_bytes", N, S, bad_k) == 0


@_DTYPES
def test_autograd_node_hands_over_the_raw_calls_gradients(dtype):
    from pcrlv2_amd import functions as Fn
    N, sp, K = 3, (2, 3, 7), 9
    a, w, b, lab = _inputs(N, sp, K, dtype, "mixed30", seed=11)
    seen = []
    for wc, wd in ((1.0, 1.0), (0.25, 2.0)):
        raw = _run(a, w, b, lab, N, sp, dtype, dloss=1.0, wc=wc, wd=wd)
        ad = _act(a, N, sp).requires_grad_(True)
        wp, bp = torch.nn.Parameter(w.cuda().view(K, C, 1, 1, 1)), torch.nn.Parameter(b.cuda())
        mod = types.SimpleNamespace(compute_dtype=dtype, _pass_idx=1)
        Fn.reset_parked()
        loss, sums = Fn.SegSoftmaxHeadFn.apply(ad, wp, bp, lab.cuda().view(N, *sp), wc, wd, mod)
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


@pytest.mark.parametrize("K", [2, 5, 16])
@_DTYPES
def test_unequal_loss_weights_against_float64_restatement(dtype, K):
    """wc and wd multiply the two loss terms in the second launch of the forward and are folded into cA, e1, e0 of the backward; at (1, 1) a swap, a
    weight left out or one applied twice cannot be seen.  Bounds as above with the weights in them.  On top: the sums do not depend on the weights (bit for
    bit); at (0, 0) everything is exactly zero; the eval entry point's loss is the forward's bit for bit.  The test is not vacuous: at (0.25, 2.0) the
    REFERENCE's loss, dW and db are further than 100 x the bound from the references with the weights swapped and with unit weights."""
    worst = {}
    for si, (N, sp) in enumerate(WEIGHT_SHAPES):
        S = sp[0] * sp[1] * sp[2]
        a, w, b, lab = _inputs(N, sp, K, dtype, "mixed30", seed=20000 * K + 100 * si + (dtype == torch.bfloat16))
        ad, wdev, bdev, ld = _act(a, N, sp), w.cuda(), b.cuda(), lab.cuda().view(N, *sp)
        unit_sums = _run(a, w, b, lab, N, sp, dtype)["sums"]
        for wc, wd in WEIGHTS:
            where = f"at N={N} spatial={sp} K={K} wc={wc} wd={wd} {dtype}"
            ref = reference(a, w, b, lab, DLOSS, wc, wd)
            got = _run(a, w, b, lab, N, sp, dtype, wc=wc, wd=wd)
            tol = _bounds(a, w, b, ref, K, N, S, dtype, DLOSS, wc, wd)
            assert torch.equal(_bits(got["sums"]), _bits(unit_sums)), "the sums do not depend on the weights " + where
            _check(got, ref, tol, K, worst, where)
            if (wc, wd) == (0.0, 0.0):
                assert float(got["loss"]) == 0.0 and not bool(got["dx"].float().abs().any()) and not bool(got["dw"].abs().any()) and not bool(got["db"].abs().any())
            if (wc, wd) == (0.25, 2.0):
                for other in (reference(a, w, b, lab, DLOSS, wd, wc), reference(a, w, b, lab, DLOSS, 1.0, 1.0)):
                    for name in ("loss", "dw", "db"):
                        assert _gap(ref[name], other[name], tol[name]), f"{name}: the reference does not tell these weights from others {where}"
            out = ops.seg_mc_head_eval(ad, wdev, bdev, dtype, labels=ld, wc=wc, wd=wd)
            torch.cuda.synchronize()
            assert torch.equal(_bits(out[1].cpu()), _bits(got["loss"])) and torch.equal(_bits(out[2].cpu()), _bits(got["sums"])), "eval " + where
    print(f"[seg_mc_head weights {dtype} K={K}] worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("K", [3, 9])
@_DTYPES
def test_backward_without_dx_leaves_dw_and_db_as_they_are(dtype, K):
    """need_dx=False hands the kernel a null dx: no dx comes back, dW and db are the bytes of the run that wrote one."""
    N, sp = 3, (2, 5, 7)
    a, w, b, lab = _inputs(N, sp, K, dtype, "mixed30", seed=13)
    ad, wdev, bdev, ld = _act(a, N, sp), w.cuda(), b.cuda(), lab.cuda().view(N, *sp)
    loss, sums = ops.seg_mc_head_forward(ad, wdev, bdev, ld, dtype)
    dl = torch.tensor(DLOSS, device="cuda")
    dx, dw, db = ops.seg_mc_head_backward(ad, wdev, bdev, ld, sums, dl, dtype)
    none, dw2, db2 = ops.seg_mc_head_backward(ad, wdev, bdev, ld, sums, dl, dtype, need_dx=False)
    torch.cuda.synchronize()
    assert none is None and dx is not None and bool(dw.abs().sum() > 0)
    assert torch.equal(_bits(dw), _bits(dw2)) and torch.equal(_bits(db), _bits(db2))


def test_label_map_groups_match_numpy():
    """pcrl_seg_labelmap_to_bits / _keep, a group of at most 7 classes at a time: n = 7, and first + n - 1 reaching K - 1."""
    K = 16
    rng = np.random.default_rng(4)
    lab = rng.integers(0, K, size=(5, 7, 13)).astype(np.uint8)
    lab[rng.random(lab.shape) < 0.2] |= 0x80
    labd = torch.from_numpy(lab).cuda()
    for first, n in [(1, 7), (8, 7), (15, 1), (9, 7), (0, 3)]:
        cls = (lab & 0x7F).astype(np.int64) - first
        inside = (cls >= 0) & (cls < n)
        want = (lab & 0x80) | np.where(inside, 1 << np.clip(cls, 0, 6), 0).astype(np.uint8)
        bits = ops.seg_labelmap_to_bits(labd, first, n)
        assert np.array_equal(bits.cpu().numpy(), want), (first, n)
        cleared = want & rng.integers(0, 256, size=lab.shape).astype(np.uint8)          # what a clean-up left of the bitmask
        kept = (cleared >> np.clip(cls, 0, 6)) & 1
        want_lab = np.where(inside & (kept == 0), lab & 0x80, lab).astype(np.uint8)
        got = ops.seg_labelmap_keep(labd, torch.from_numpy(cleared).cuda(), first, n)
        assert np.array_equal(got.cpu().numpy(), want_lab), (first, n)
    with pytest.raises(RuntimeError):
        ops.seg_labelmap_to_bits(labd, 1, 8)
