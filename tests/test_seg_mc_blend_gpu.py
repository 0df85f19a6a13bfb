"""pcrl_seg_mc_blend (csrc/seg_blend.hip), the label-map sibling of the sliding-window blend, against tests/seg_blend_reference.py's numpy restatements.

Bit for bit: num and den equal blend32 (the kernel's float32 arithmetic, one operation at a time in its order: the patch walk is pcrl_seg_blend's own);
the label map is the LOWEST class with the largest num_k of that restatement (0 where the voxel is not counted), the counts {TP, |pred|, |gt|} of all K
classes follow from it, they are added to one row, and two runs give identical bytes.
Derived, none fitted (u = 2^-24, ULP = 2^-23): zbar_k = num_k / den is one correctly rounded division of the restatement's operands, so it is within
ULP |zref32| of zref32 = n32 / d32.  Against the float64 blend zbar64 the logit error is  E_z = |zref32 - zbar64| + ULP |zref32|,  and the probabilities,
sums and loss follow tests/test_seg_mc_head_gpu.py's lines with that E_z (forward_bounds), the sum s taken serially over the K classes (K - 1 additions
instead of the head's butterfly).  The float64 reference is the head's, fed with zbar64 as its logits (unit weight rows, zero bias).
Every class count K = 2..16 is launched (2, 9, 16 with the whole lists, the others compactly), and the blend's loss takes unequal weights wc, wd in
test_label_map_blend_loss_takes_its_weights_and_the_sums_do_not.
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pcrlv2_amd import data_seg as D  # noqa: E402
from pcrlv2_amd import ops  # noqa: E402
from pcrlv2_amd._lib import PcrlError  # noqa: E402
from seg_blend_reference import blend32, blend64  # noqa: E402
from seg_mc_reference import reference  # noqa: E402
from test_seg_mc_head_gpu import ULP, WEIGHTS, forward_bounds  # noqa: E402

pytestmark = pytest.mark.gpu
CROP = (8, 8, 8)
DEV = "cuda"


def _logits(kind, axes, shape, K, rng):
    """'random': N(0, 1).  'ties': a field over the VOLUME of small integers, every patch showing the same values: num_k are exact multiples and many
    voxels have their maximum shared by two classes."""
    starts = D.window_starts(axes)
    z = rng.standard_normal((len(starts),) + CROP + (K,)).astype(np.float32)
    if kind == "ties":
        field = rng.integers(-1, 2, tuple(shape) + (K,)).astype(np.float32)
        for p, st in enumerate(starts):
            vol = tuple(slice(s, min(s + c, n)) for s, c, n in zip(st, CROP, shape))
            box = tuple(slice(0, sl.stop - sl.start) for sl in vol)
            z[p][box] = field[vol]
    return z


def _labels(kind, shape, K, rng):
    if kind == "none":
        return None
    lab = rng.integers(0, K, shape).astype(np.uint8)
    if kind == "mixed30":
        lab |= (rng.random(shape) < 0.3).astype(np.uint8) << 7
    if kind == "all_off":
        lab |= 0x80
    return lab


def _lowest_argmax(num):
    K = num.shape[-1]
    m = num.max(-1, keepdims=True)
    return np.where(num == m, np.arange(K), K).min(-1).astype(np.uint8)


def _counts_of(pred, lab, K):
    labv = np.zeros(pred.shape, dtype=np.uint8) if lab is None else lab
    on = ((labv & 0x80) == 0) & ((labv & 0x7F) < K)
    out = np.zeros((K, 3), dtype=np.int64)
    for k in range(K):
        p, g = (pred == k) & on, ((labv & 0x7F) == k) & on
        out[k] = (int((p & g).sum()), int(p.sum()), int(g.sum()))
    return out


def _check(shape, K, overlap, window, zkind, label_kinds, seed, worst, weight_pairs=()):
    """weight_pairs: further (wc, wd) the labelled runs are repeated with: the loss within its bound against the reference with those weights, the sums
    the unit-weight run's bytes."""
    rng = np.random.default_rng(seed)
    axes, weights = D.windows(shape, CROP, overlap), D.blend_weights(CROP, window)
    z = _logits(zkind, axes, shape, K, rng)
    n32, d32 = blend32(z, axes, weights, shape)
    n64, d64, _, cover = blend64(z, axes, weights, shape)
    assert cover.min() >= 1
    zref32 = n32 / d32[..., None]
    zbar64 = torch.from_numpy(n64 / d64[..., None]).reshape(-1, K)
    M = int(np.prod(shape))
    sd, wd_ = [torch.tensor(a, dtype=torch.int32, device=DEV) for a in axes], [torch.from_numpy(w).to(DEV) for w in weights]
    zd = torch.from_numpy(z).to(DEV)
    pred = _lowest_argmax(n32)
    if zkind == "ties" and M > 1:
        assert int(((n32 == n32.max(-1, keepdims=True)).sum(-1) >= 2).sum()) > 0, "the case list must contain voxels whose maximum is shared"
    for kind in label_kinds:
        lab = _labels(kind, shape, K, rng)
        ld = None if lab is None else torch.from_numpy(lab).to(DEV)
        counts = torch.full((3, K, 3), 5, dtype=torch.int64, device=DEV)
        runs = []
        for _ in range(2):
            before = counts.clone()
            lm, probs, sums, loss, nd = ops.seg_mc_blend(zd, sd, wd_, shape, labels=ld, counts=counts, row=1, want_probs=True, want_numden=True)
            torch.cuda.synchronize()
            runs.append((lm.cpu(), probs.cpu(), sums.cpu(), loss.cpu(), nd.cpu(), (counts - before).cpu()))
        for x, y in zip(*runs):
            assert x.numpy().tobytes() == y.numpy().tobytes(), "two runs give identical bytes"
        lm, probs, sums, loss, nd, added = runs[0]
        what = f"volume {shape} K={K} overlap {overlap} {window} logits {zkind} labels {kind}"
        assert nd[:K].numpy().tobytes() == np.ascontiguousarray(np.moveaxis(n32, -1, 0)).tobytes(), "num: " + what
        assert nd[K].numpy().tobytes() == d32.tobytes(), "den: " + what
        on = np.ones(shape, dtype=bool) if lab is None else ((lab & 0x80) == 0) & ((lab & 0x7F) < K)
        want_lm = np.where(on, pred, 0).astype(np.uint8)
        assert np.array_equal(lm.numpy(), want_lm), "label map: " + what
        want_counts = torch.zeros((3, K, 3), dtype=torch.int64)
        want_counts[1] = torch.from_numpy(_counts_of(pred, lab, K))
        assert torch.equal(added, want_counts), "counts are added to row 1 alone: " + what
        assert torch.equal(counts.cpu(), 5 + 2 * want_counts)
        zb = nd[K + 1:].permute(1, 2, 3, 0).double().numpy()
        assert bool((np.abs(zb - zref32) <= ULP * np.abs(zref32) + 1e-44).all()), "zbar: " + what
        # probabilities, sums and loss against the float64 restatement
        a = torch.zeros((M, 64), dtype=torch.float64)
        a[:, :K] = zbar64
        flat = torch.zeros(M, dtype=torch.uint8) if lab is None else torch.from_numpy(lab).reshape(-1)
        ref = reference(a, torch.eye(K, 64, dtype=torch.float64), torch.zeros(K, dtype=torch.float64), flat)
        free = reference(a, torch.eye(K, 64, dtype=torch.float64), torch.zeros(K, dtype=torch.float64), torch.zeros(M, dtype=torch.uint8))
        z32 = torch.from_numpy(zref32.reshape(-1, K)).double()
        e_z = (z32 - zbar64).abs() + ULP * z32.abs()
        assert torch.equal(free["z"], zbar64)
        p_tol = forward_bounds(e_z, free, K, M, s_adds=K - 1)["dp"]
        p_err = (probs.permute(1, 2, 3, 0).reshape(-1, K).double() - free["p"]).abs()
        assert bool((p_err <= p_tol).all()), "probabilities: " + what
        worst["p"] = max(worst.get("p", 0.0), float((p_err / p_tol).max()))
        tol = forward_bounds(e_z, ref, K, M, s_adds=K - 1)
        assert float(sums[4 * K]) == ref["Mc"] and torch.equal(sums[2:4 * K:4], ref["G"]), "counted voxels and G are exact: " + what
        e_sums, e_loss = (sums - ref["sums"]).abs(), (loss.double() - ref["loss"]).abs()
        assert bool((e_sums <= tol["sums"]).all()), "sums: " + what
        assert bool(e_loss <= tol["loss"]), f"loss: error {float(e_loss):.3e} bound {float(tol['loss']):.3e} " + what
        worst["sums"] = max(worst.get("sums", 0.0), float((e_sums / tol["sums"].clamp_min(1e-300)).max()))
        worst["loss"] = max(worst.get("loss", 0.0), float(e_loss / tol["loss"].clamp_min(1e-300)))
        if kind == "all_off":
            assert not bool(lm.any()) and not bool(added.any()) and float(loss) == 0.0
        seen = {}
        for wc, wd in weight_pairs:
            _, _, s_w, l_w, _ = ops.seg_mc_blend(zd, sd, wd_, shape, labels=ld, want_mask=False, wc=wc, wd=wd)
            torch.cuda.synchronize()
            ref_w = reference(a, torch.eye(K, 64, dtype=torch.float64), torch.zeros(K, dtype=torch.float64), flat, 1.0, wc, wd)
            t_w = forward_bounds(e_z, ref_w, K, M, s_adds=K - 1, wc=wc, wd=wd)["loss"]
            e_w = (l_w.cpu().double() - ref_w["loss"]).abs()
            assert s_w.cpu().numpy().tobytes() == sums.numpy().tobytes(), f"the sums do not depend on the weights ({wc}, {wd}): " + what
            assert bool(e_w <= t_w), f"loss at weights ({wc}, {wd}): error {float(e_w):.3e} bound {float(t_w):.3e} " + what
            worst["loss_w"] = max(worst.get("loss_w", 0.0), float(e_w / t_w.clamp_min(1e-300)))
            if (wc, wd) == (0.0, 0.0):
                assert float(l_w) == 0.0
            seen[(wc, wd)] = (float(ref_w["loss"]), float(t_w))
        if (0.25, 2.0) in seen and (2.0, 0.25) in seen and kind != "all_off":      # not vacuous: the swapped weights are another loss by far
            assert abs(seen[(0.25, 2.0)][0] - seen[(2.0, 0.25)][0]) > 100 * seen[(0.25, 2.0)][1], what
            assert abs(seen[(0.25, 2.0)][0] - float(ref["loss"])) > 100 * seen[(0.25, 2.0)][1], what


@pytest.mark.parametrize("K", [2, 9, 16])
@pytest.mark.parametrize("shape", [(5, 8, 3), (8, 8, 8), (9, 17, 13)])      # smaller than, equal to and no multiple of the crop
def test_label_map_blend_equals_the_float32_restatement_bit_for_bit(shape, K):
    worst, i = {}, 0
    for overlap in (0, 0.5):
        for window in D.WINDOWS:
            for zkind in ("random", "ties"):
                i += 1
                _check(shape, K, overlap, window, zkind, ("none", "mixed", "mixed30", "all_off"), 1000 * K + 10 * sum(shape) + i, worst)
    print(f"[seg_mc_blend {shape} K={K}] worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("K", [k for k in range(2, 17) if k not in (2, 9, 16)])
def test_label_map_blend_at_the_other_class_counts(K):
    """The instantiations the test above leaves out, compactly: a volume that is no multiple of the crop, overlapping gaussian windows."""
    worst = {}
    for i, zkind in enumerate(("random", "ties")):
        _check((9, 17, 13), K, 0.5, "gaussian", zkind, ("mixed30",), 5000 + 10 * K + i, worst)
    print(f"[seg_mc_blend compact K={K}] worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_label_map_blend_loss_takes_its_weights_and_the_sums_do_not():
    """wc, wd are arguments of pcrl_seg_mc_blend (the loss of a blended case): the head test's weight pairs, same bound, the sums bit for bit."""
    worst = {}
    _check((9, 17, 13), 5, 0.5, "gaussian", "random", ("mixed30",), 6005, worst, weight_pairs=WEIGHTS)
    print("[seg_mc_blend weights K=5] worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_outputs_are_optional_and_bad_arguments_are_refused():
    K, shape = 3, (9, 8, 8)
    rng = np.random.default_rng(1)
    axes, weights = D.windows(shape, CROP, 0.5), D.blend_weights(CROP, "gaussian")
    sd, wd_ = [torch.tensor(a, dtype=torch.int32, device=DEV) for a in axes], [torch.from_numpy(w).to(DEV) for w in weights]
    zd = torch.from_numpy(_logits("random", axes, shape, K, rng)).to(DEV)
    lm, probs, sums, loss, nd = ops.seg_mc_blend(zd, sd, wd_, shape, want_sums=False)
    assert lm is not None and probs is None and sums is None and loss is None and nd is None
    full = ops.seg_mc_blend(zd, sd, wd_, shape)
    assert torch.equal(full[0], lm) and full[2].shape == (4 * K + 1,)
    with pytest.raises(PcrlError, match="2 <= K <= 16"):
        ops.seg_mc_blend(zd[..., :1].contiguous(), sd, wd_, shape)
    with pytest.raises(PcrlError, match="patches against start lists"):
        ops.seg_mc_blend(zd[:1], sd, wd_, shape)
