"""pcrl_seg_head_logits, pcrl_seg_cut_patches and pcrl_seg_blend (csrc/seg_head.hip, csrc/seg_blend.hip).

logits   thresholded, they ARE pcrl_seg_head_eval's mask (both go through sh_logit); against the float64 reference they keep the head test's bound
         E_z = (64 + 8) u sum_c |W x| + u |b| (test_seg_head_gpu.py), and on exact_lattice's FINER operands they equal it.
cutter   byte for byte data_seg.cut's image.
blend    num, den, the mask and the integer counts EQUAL tests/seg_blend_reference.py's float32 restatement, bit for bit.  Derived bounds for the rest
         (u = 2^-24, ULP = 2^-23):
  zbar   |zbar - fl32(num / den)| <= ULP |zbar|                           one division, correctly rounded or 1 ulp off
  p      |p - sigmoid(fl32(num / den))| <= |zbar| ULP / 4 + 4 ULP p         sigmoid is 1/4-Lipschitz; 4 ulps for exp and the division
  sums   the head test's lines with E_z := |fl32(num32 / den32) - num64 / den64| + ULP |zbar|, the float32 restatement's own distance from the float64
         one plus the division: dp = E_z / 4 + 4 ULP p; E_P = sum dp, E_I = sum g dp (+ (M + 8) 2^-53 of the float64 sum); BCE_k: sum (E_z + 4 ULP |term|);
         loss: wb sum_k E_BCE_k / (Mc K) + (wd / K) sum_k (2 E_I / U + (2 I + eps) E_P / U^2) + 2 ULP |loss|.  G and Mc are exact.
Every class count K = 1..7 is launched by the logits and the blend tests (1, 3, 7 with the whole lists, the others with compact ones), and the blend's
loss takes unequal weights wb, wd in test_blend_loss_takes_its_weights_and_the_sums_do_not.
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_seg_head_gpu as H  # noqa: E402
from pcrlv2_amd import data_seg as D  # noqa: E402
from pcrlv2_amd import ops  # noqa: E402
from pcrlv2_amd._lib import PcrlError, dtype_code, lib, stream_handle  # noqa: E402
from seg_blend_reference import blend32, blend64, counts_of, mask_of  # noqa: E402
from seg_reference import reference  # noqa: E402

pytestmark = pytest.mark.gpu
U, ULP = 2.0 ** -24, 2.0 ** -23
CROP = (8, 8, 8)
GRID_CAP, BLOCK = 1024, 256              # csrc/seg_blend.hip: SB_MAX_BLOCKS, SB_THREADS
DEV = "cuda"


def _pack(z):
    """(z >= 0) of [..., K] packed into bits."""
    return sum(((z[..., k] >= 0).to(torch.uint8) << k) for k in range(z.shape[-1])).to(torch.uint8)


# ---- logits -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", H.ALL_KS)
@H._DTYPES
def test_logits_threshold_to_the_eval_mask_and_keep_the_head_bound(dtype, K):
    for si, (N, sp) in enumerate(H.SHAPES if K in H.FULL_KS else H.REDUCED_SHAPES):
        a, w, b, lab = H._inputs(N, sp, K, dtype, "zeros", seed=900 * K + si)
        act = H._act(a, N, sp)
        z = ops.seg_head_logits(act, w.cuda(), b.cuda(), dtype)
        mask = ops.seg_head_eval(act, w.cuda(), b.cuda(), dtype, want_mask=True)[3]
        torch.cuda.synchronize()
        assert z.shape == (N, *sp, K) and z.dtype == torch.float32 and z.is_contiguous()
        assert torch.equal(_pack(z), mask), f"N={N} spatial={sp}"
        ref = reference(a, w, b, lab)
        e_z = (H.C + 8) * U * (a.double().abs() @ w.double().abs().t()) + U * b.double().abs()
        err = (z.reshape(-1, K).cpu().double() - ref["z"]).abs()
        print(f"[logits {dtype} K={K} M={a.shape[0]}] worst error / bound {float((err / e_z.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= e_z).all())


@pytest.mark.parametrize("K", H.ALL_KS)
@H._DTYPES
def test_logits_equal_the_reference_on_exactly_summable_operands(dtype, K):
    for N, sp in H.SHAPES if K in H.FULL_KS else H.REDUCED_SHAPES:
        S = sp[0] * sp[1] * sp[2]
        a, w, b, lab = H._exact_inputs(N, sp, K, seed=31 * K + S)
        z = ops.seg_head_logits(H._act(a.to(dtype), N, sp), w.float().cuda(), b.float().cuda(), dtype)
        assert torch.equal(z.reshape(-1, K).cpu().double(), reference(a, w, b, lab)["z"]), f"N={N} spatial={sp}"


@H._DTYPES
def test_logits_leave_the_bytes_behind_their_output_alone_and_refuse_bad_sizes(dtype):
    N, sp, K = 3, (1, 3, 7), 3
    S, M = 21, 63
    a, w, b, _ = H._inputs(N, sp, K, dtype, "zeros", seed=9)
    ad = H._act(a, N, sp).permute(0, 2, 3, 4, 1).contiguous()
    full = torch.full((M * K + 64,), -7.0, dtype=torch.float32, device=DEV)
    lib().call("pcrl_seg_head_logits", ad, w.cuda(), b.cuda(), full[:M * K], N, S, K, dtype_code(dtype), stream_handle())
    torch.cuda.synchronize()
    assert bool((full[M * K:] == -7.0).all()) and not bool((full[:M * K] == -7.0).any())
    assert torch.equal(full[:M * K].view(N, *sp, K), ops.seg_head_logits(H._act(a, N, sp), w.cuda(), b.cuda(), dtype))
    for bad_k, bad_s in ((8, S), (0, S), (K, 0)):
        with pytest.raises(PcrlError):
            lib().call("pcrl_seg_head_logits", ad, w.cuda(), b.cuda(), full, N, bad_s, bad_k, dtype_code(dtype), stream_handle())
    with pytest.raises(PcrlError, match="out must be"):
        ops.seg_head_logits(H._act(a, N, sp), w.cuda(), b.cuda(), dtype, out=full[:M * K + 1])


# ---- cutter -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", [np.float32, np.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("C", [1, 4])
@pytest.mark.parametrize("shape", [(1, 1, 1), (8, 8, 8), (9, 17, 13), (5, 20, 8)])
def test_cutter_equals_data_seg_cut_byte_for_byte(shape, C, src):
    rng = np.random.default_rng(sum(shape) + C)
    img = rng.standard_normal((C,) + shape).astype(src)
    img.reshape(-1)[::7] = -0.0                      # a copy keeps the sign of zero
    case = D.Case("c", img)
    back = tuple(max(n - c, 0) for n, c in zip(shape, CROP))                    # the shifted-back last start
    out3 = tuple(max(n - 3, 0) for n in shape)                                    # leaves the volume on all three axes at once
    starts = [(0, 0, 0), back, out3, (back[0], 0, out3[2]), tuple(n // 2 for n in shape)]
    want = np.stack([D.cut(case, st, CROP)[0] for st in starts])
    n_out = want.size
    full = torch.full((n_out + 64,), -7.0, dtype=torch.float32, device=DEV)
    got = ops.seg_cut_patches(torch.from_numpy(img).cuda(), torch.tensor(starts, dtype=torch.int32, device=DEV), CROP, out=full[:n_out].view(want.shape))
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and got.cpu().numpy().tobytes() == want.tobytes()
    assert bool((full[n_out:] == -7.0).all())


def test_cutter_refuses_what_it_cannot_cut():
    img = torch.zeros((1, 8, 8, 8), device=DEV)
    st = torch.zeros((1, 3), dtype=torch.int32, device=DEV)
    for bad_img, bad_st, crop in ((img.double(), st, CROP), (img.cpu(), st, CROP), (img, st.long(), CROP), (img, st[:, :2], CROP), (img, st, (8, 8, 6)),
                                  (img, st, (8, 0, 8))):
        with pytest.raises(PcrlError):
            ops.seg_cut_patches(bad_img, bad_st, crop)
    with pytest.raises(PcrlError):
        lib().call("pcrl_seg_cut_patches", img, 0, st, img, 0, 1, 8, 8, 8, 8, 8, 8, stream_handle())
    room = torch.empty(512 + 4, device=DEV)
    for off in (1, 2, 3):       # 16-byte stores: an output at an element offset that is no multiple of 4 is refused by the wrapper and by the library
        view = room[off:off + 512].view(1, 1, 8, 8, 8)
        with pytest.raises(PcrlError, match="16-byte aligned"):
            ops.seg_cut_patches(img, st, CROP, out=view)
        with pytest.raises(PcrlError, match="16-byte aligned"):
            lib().call("pcrl_seg_cut_patches", img, 0, st, view, 1, 1, 8, 8, 8, 8, 8, 8, stream_handle())
    assert ops.seg_cut_patches(img, st, CROP, out=room[4:516].view(1, 1, 8, 8, 8)).data_ptr() == room.data_ptr() + 16


# ---- blend ------------------------------------------------------------------------------------------------------------------------
def _logits(kind, axes, shape, K, rng):
    """'random': N(0, 1).  'ties': a field over the VOLUME of small integers with many zeros, every patch showing it with its own sign: exact zeros
    and sign-symmetric pairs, so num == 0 occurs (and must predict 1)."""
    starts = D.window_starts(axes)
    z = rng.standard_normal((len(starts),) + CROP + (K,)).astype(np.float32)
    if kind == "ties":
        field = rng.integers(-2, 3, tuple(shape) + (K,)).astype(np.float32)
        field[rng.random(tuple(shape)) < 0.3] = 0.0
        for p, st in enumerate(starts):
            vol = tuple(slice(s, min(s + c, n)) for s, c, n in zip(st, CROP, shape))
            box = tuple(slice(0, sl.stop - sl.start) for sl in vol)
            z[p][box] = field[vol] * np.float32(1 if p % 2 == 0 else -1)
    return z


def _labels(kind, shape, K, rng):
    if kind == "none":
        return None
    lab = rng.integers(0, 1 << K, shape).astype(np.uint8)
    if kind == "mixed30":
        lab |= (rng.random(shape) < 0.3).astype(np.uint8) << 7
    if kind == "all_off":
        lab |= 0x80
    return lab


def _dev(axes, weights):
    return ([torch.tensor(a, dtype=torch.int32, device=DEV) for a in axes], [torch.from_numpy(w).to(DEV) for w in weights])


def _sum_bounds(zref32, zbar64, ref, K, M, wb=1.0, wd=1.0):
    """The head test's E_P, E_I, BCE and loss lines with E_z as in the module docstring; flat [M, K] float64 inputs.  wb, wd: the weights of `ref`."""
    e_z = (torch.from_numpy(zref32).double() - zbar64).abs() + ULP * torch.from_numpy(zref32).double().abs()
    cnt = ref["counted"].double().unsqueeze(1)
    g, p = ref["g"], ref["p"]
    dp = e_z / 4 + 4 * ULP * p
    E_P, E_I = (dp * cnt).sum(0) + (M + 8) * 2.0 ** -53 * ref["P"], (dp * g * cnt).sum(0) + (M + 8) * 2.0 ** -53 * ref["I"]
    Uk, num, Mc = ref["P"] + ref["G"] + 1.0, 2 * ref["I"] + 1.0, ref["Mc"]
    e_bce = ((e_z + 4 * ULP * ref["terms"].abs()) * cnt).sum(0)
    sums = torch.cat([torch.stack([E_I, E_P, torch.zeros(K, dtype=torch.float64), e_bce], dim=1).reshape(-1), torch.zeros(1, dtype=torch.float64)])
    loss = (abs(wb) * e_bce.sum() / (Mc * K) if Mc else 0.0) + (abs(wd) / K) * (2 * E_I / Uk + num * E_P / Uk ** 2).sum() + 2 * ULP * ref["loss"].abs()
    return sums, loss


def _check_blend(shape, K, overlap, window, zkind, label_kinds, seed, worst, weight_pairs=()):
    """weight_pairs: further (wb, wd) the labelled runs are repeated with: the loss within its bound against the reference with those weights, the sums
    the unit-weight run's bytes."""
    rng = np.random.default_rng(seed)
    axes, weights = D.windows(shape, CROP, overlap), D.blend_weights(CROP, window)
    z = _logits(zkind, axes, shape, K, rng)
    n32, d32 = blend32(z, axes, weights, shape)
    n64, d64, _, cover = blend64(z, axes, weights, shape)
    assert cover.min() >= 1
    zref32 = n32 / d32[..., None]
    assert zref32.dtype == np.float32
    zbar64 = torch.from_numpy(n64 / d64[..., None]).reshape(-1, K)
    M = int(np.prod(shape))
    sd, wd_ = _dev(axes, weights)
    zd = torch.from_numpy(z).to(DEV)
    if zkind == "ties" and M > 1:
        assert int((n32 == 0).sum()) > 0, "the case list must contain ties at num = 0"
    for kind in label_kinds:
        lab = _labels(kind, shape, K, rng)
        ld = None if lab is None else torch.from_numpy(lab).to(DEV)
        counts = torch.full((3, K, 3), 5, dtype=torch.int64, device=DEV)
        runs = []
        for _ in range(2):
            before = counts.clone()
            mask, probs, sums, loss, nd = ops.seg_blend(zd, sd, wd_, shape, labels=ld, counts=counts, row=1, want_probs=True, want_numden=True)
            torch.cuda.synchronize()
            runs.append((mask.cpu(), probs.cpu(), sums.cpu(), loss.cpu(), nd.cpu(), (counts - before).cpu()))
        for x, y in zip(*runs):
            assert x.numpy().tobytes() == y.numpy().tobytes(), "two runs give identical bytes"
        mask, probs, sums, loss, nd, added = runs[0]
        what = f"volume {shape} K={K} overlap {overlap} {window} logits {zkind} labels {kind}"
        # bit for bit: num, den, mask, counts
        assert nd[:K].numpy().tobytes() == np.ascontiguousarray(np.moveaxis(n32, -1, 0)).tobytes(), "num: " + what
        assert nd[K].numpy().tobytes() == d32.tobytes(), "den: " + what
        want_mask = mask_of(n32, lab)
        assert np.array_equal(mask.numpy(), want_mask), "mask: " + what
        tie = (n32 == 0) & (np.ones(shape, dtype=bool) if lab is None else (lab & 0x80) == 0)[..., None]
        for k in range(K):
            assert bool((((mask.numpy() >> k) & 1)[tie[..., k]] == 1).all()), "num == 0 predicts 1: " + what
        want_counts = torch.zeros((3, K, 3), dtype=torch.int64)
        want_counts[1] = torch.from_numpy(counts_of(want_mask, lab, K))
        assert torch.equal(added, want_counts), "counts are added to row 1 alone: " + what
        assert torch.equal(counts.cpu(), 5 + 2 * want_counts)
        # zbar and the probabilities
        zb = nd[K + 1:].permute(1, 2, 3, 0).double().numpy()
        assert bool((np.abs(zb - zref32) <= ULP * np.abs(zref32) + 1e-44).all()), "zbar: " + what
        p_ref = 1.0 / (1.0 + np.exp(-zref32.astype(np.float64)))
        p_err, p_tol = np.abs(probs.permute(1, 2, 3, 0).double().numpy() - p_ref), np.abs(zref32) * ULP / 4 + 4 * ULP * p_ref
        assert bool((p_err <= p_tol).all()), "probabilities: " + what
        worst["p"] = max(worst.get("p", 0.0), float((p_err / p_tol).max()))
        # sums and loss against the float64 restatement: the head's reference fed with zbar64 as its logits (weight = unit rows, bias = 0)
        a = torch.zeros((M, 64), dtype=torch.float64)
        a[:, :K] = zbar64
        flat = torch.zeros(M, dtype=torch.uint8) if lab is None else torch.from_numpy(lab).reshape(-1)
        ref = reference(a, torch.eye(K, 64, dtype=torch.float64), torch.zeros(K, dtype=torch.float64), flat)
        assert torch.equal(ref["z"], zbar64)
        t_sums, t_loss = _sum_bounds(zref32.reshape(-1, K), zbar64, ref, K, M)
        assert float(sums[4 * K]) == ref["Mc"] and torch.equal(sums[2:4 * K:4], ref["G"]), "counted voxels and G are exact: " + what
        e_sums, e_loss = (sums - ref["sums"]).abs(), (loss.double() - ref["loss"]).abs()
        assert bool((e_sums <= t_sums).all()), "sums: " + what
        assert bool(e_loss <= t_loss), f"loss: error {float(e_loss):.3e} bound {float(t_loss):.3e} " + what
        worst["sums"] = max(worst.get("sums", 0.0), float((e_sums / t_sums.clamp_min(1e-300)).max()))
        worst["loss"] = max(worst.get("loss", 0.0), float(e_loss / t_loss.clamp_min(1e-300)))
        if kind == "all_off":
            assert not bool(mask.any()) and not bool(added.any()) and float(loss) == 0.0
        seen = {}
        for wb, wd in weight_pairs:
            _, _, s_w, l_w, _ = ops.seg_blend(zd, sd, wd_, shape, labels=ld, want_mask=False, wb=wb, wd=wd)
            torch.cuda.synchronize()
            ref_w = reference(a, torch.eye(K, 64, dtype=torch.float64), torch.zeros(K, dtype=torch.float64), flat, 1.0, wb, wd)
            _, t_w = _sum_bounds(zref32.reshape(-1, K), zbar64, ref_w, K, M, wb, wd)
            e_w = (l_w.cpu().double() - ref_w["loss"]).abs()
            assert s_w.cpu().numpy().tobytes() == sums.numpy().tobytes(), f"the sums do not depend on the weights ({wb}, {wd}): " + what
            assert bool(e_w <= t_w), f"loss at weights ({wb}, {wd}): error {float(e_w):.3e} bound {float(t_w):.3e} " + what
            worst["loss_w"] = max(worst.get("loss_w", 0.0), float(e_w / t_w.clamp_min(1e-300)))
            if (wb, wd) == (0.0, 0.0):
                assert float(l_w) == 0.0
            seen[(wb, wd)] = (float(ref_w["loss"]), float(t_w))
        if (0.25, 2.0) in seen and (2.0, 0.25) in seen and kind != "all_off":      # not vacuous: the swapped weights are another loss by far
            assert abs(seen[(0.25, 2.0)][0] - seen[(2.0, 0.25)][0]) > 100 * seen[(0.25, 2.0)][1], what
            assert abs(seen[(0.25, 2.0)][0] - float(ref["loss"])) > 100 * seen[(0.25, 2.0)][1], what


@pytest.mark.parametrize("K", [1, 3, 7])
@pytest.mark.parametrize("shape", [(1, 1, 1), (8, 8, 8), (9, 8, 8), (9, 17, 13), (16, 16, 16)])
def test_blend_equals_the_float32_restatement_bit_for_bit(shape, K):
    worst, i = {}, 0
    for overlap in (0, 0.5, 0.75):
        for window in D.WINDOWS:
            for zkind in ("random", "ties"):
                i += 1
                _check_blend(shape, K, overlap, window, zkind, ("none", "mixed", "mixed30", "all_off"), 1000 * K + 10 * sum(shape) + i, worst)
    print(f"[seg_blend {shape} K={K}] worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("K", [2, 4, 5, 6])
def test_blend_at_the_other_class_counts(K):
    """The instantiations the test above leaves out, compactly: a volume that is no multiple of the crop, overlapping gaussian windows."""
    worst = {}
    for i, zkind in enumerate(("random", "ties")):
        _check_blend((9, 17, 13), K, 0.5, "gaussian", zkind, ("mixed30",), 5000 + 10 * K + i, worst)
    print(f"[seg_blend compact K={K}] worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_blend_loss_takes_its_weights_and_the_sums_do_not():
    """wb, wd are arguments of pcrl_seg_blend (the loss of a blended case): the head test's weight pairs, same bound, the sums bit for bit."""
    worst = {}
    _check_blend((9, 17, 13), 3, 0.5, "gaussian", "random", ("mixed30",), 6003, worst, weight_pairs=H.WEIGHTS)
    print("[seg_blend weights K=3] worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("K,zkind", [(3, "random"), (3, "ties"), (7, "random"), (7, "ties")])
def test_blend_one_voxel_above_the_grid_cap(K, zkind):
    """GRID_CAP * BLOCK + 1 voxels: every thread of the capped grid takes one voxel and one thread a second one (the grid-stride loop), whose terms
    enter the same per-thread sums and counts -- with mixed, partly uncounted and wholly uncounted labels."""
    shape = (65, 37, 109)
    assert shape[0] * shape[1] * shape[2] == GRID_CAP * BLOCK + 1
    worst = {}
    _check_blend(shape, K, 0.5, "gaussian" if zkind == "random" else "constant", zkind, ("mixed30", "all_off"), 4242 + K, worst)
    print(f"[seg_blend above the cap K={K} {zkind}] worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_blend_outputs_are_optional_and_bad_arguments_are_refused():
    shape, K = (9, 17, 13), 3
    axes, weights = D.windows(shape, CROP, 0.5), D.blend_weights(CROP, "gaussian")
    sd, wd_ = _dev(axes, weights)
    P = len(D.window_starts(axes))
    z = torch.randn((P,) + CROP + (K,), device=DEV)
    full = ops.seg_blend(z, sd, wd_, shape, want_probs=True)
    assert full[4] is None and full[0] is not None and full[1] is not None and full[2] is not None
    only_mask = ops.seg_blend(z, sd, wd_, shape, want_sums=False)
    assert torch.equal(only_mask[0], full[0]) and only_mask[1:] == (None, None, None, None)
    only_probs = ops.seg_blend(z, sd, wd_, shape, want_mask=False, want_probs=True, want_sums=False)
    assert only_probs[0] is None and torch.equal(only_probs[1], full[1])
    counts = torch.zeros((1, K, 3), dtype=torch.int64, device=DEV)
    for kw in (dict(counts=counts, row=1), dict(counts=counts, want_sums=False), dict(counts=counts.int()), dict(labels=torch.zeros(5, dtype=torch.uint8, device=DEV))):
        with pytest.raises(PcrlError):
            ops.seg_blend(z, sd, wd_, shape, **kw)
    with pytest.raises(PcrlError, match="patches against start lists"):
        ops.seg_blend(z[:-1], sd, wd_, shape)
    with pytest.raises(PcrlError, match="weight tables"):
        ops.seg_blend(z, sd, [wd_[0], wd_[1], wd_[2][:4]], shape)
    # the library's own error code, past the Python checks
    n = [len(a) for a in axes]
    mask = torch.empty(shape, dtype=torch.uint8, device=DEV)

    def raw(P_, K_, vol):
        lib().call("pcrl_seg_blend", z, P_, *sd, *n, *wd_, *CROP, *vol, K_, None, mask, None, None, None, None, None, 1.0, 1.0, None, 0, stream_handle())

    raw(P, K, shape)
    for P_, K_, vol in ((P, 8, shape), (P, 0, shape), (P, K, (0, 17, 13)), (P + 1, K, shape), (P - 1, K, shape)):
        with pytest.raises(PcrlError):
            raw(P_, K_, vol)
