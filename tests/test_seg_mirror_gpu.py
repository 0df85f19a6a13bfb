"""Mirror test-time augmentation and checkpoint ensembling on the GPU: pcrl_seg_cut_patches_mirror (csrc/seg_blend.hip),
pcrl_seg_head_logits_acc (csrc/seg_head.hip), Segmenter3d.infer_logits(flip=, accumulate=, scale=), train_seg.sliding_window(mirror=, models=),
evaluate_sliding(mirror=) and the commands.  EVERYTHING here is bit for bit: the cutter is a copy, a logit is the plain kernel's, and the accumulation is
one float32 addition per pass and one multiplication, which tests/seg_mirror_reference.py restates in that order.

Shapes of the accumulating head (a block handles 16 voxels per iteration in float32 and 32 in bf16; a sample gets at most 1024 / N blocks):
  N = 3,  crop 3 x 5 x 7    three different sizes (a swapped axis shows); S = 105 is no multiple of 16 or 32; one iteration per block
  N = 64, crop 8 x 8 x 16   16 blocks per sample for S = 1024 voxels: every block iterates 4 (float32) or 2 (bf16) times, so the carried (i, j, k) advance
                            and the read-ahead of z are exercised"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pcrlv2_amd import data_seg as D  # noqa: E402
from pcrlv2_amd import ops  # noqa: E402
from pcrlv2_amd._lib import PcrlError, dtype_code, lib, stream_handle  # noqa: E402
from pcrlv2_amd.models import Segmenter3d  # noqa: E402
from pcrlv2_amd.train_seg import dice_from_counts, evaluate_sliding, sliding_window  # noqa: E402
from seg_blend_reference import blend32, counts_of, mask_of  # noqa: E402
from seg_mirror_reference import flip_axes, tta_logits  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
_DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])


def _bytes(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


# ---- the mirrored cutter ------------------------------------------------------------------------------------------------------------------------
CUT_SHAPE, CUT_CROP, PAD = (9, 7, 6), (8, 4, 4), 8
CUT_STARTS = [(0, 0, 0), (-3, -2, -1), (4, 5, 4), (1, 3, 2), (-7, 6, -3), (8, -3, 5)]      # below 0, inside, hanging over the high end, mixed


@pytest.mark.parametrize("src", [np.float32, np.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("C", [1, 2])
def test_mirrored_cutter_is_np_flip_of_data_seg_cut(C, src):
    rng = np.random.default_rng(11 + C)
    img = rng.standard_normal((C,) + CUT_SHAPE).astype(src)
    img.reshape(-1)[::7] = -0.0                                                  # a copy keeps the sign of zero
    # data_seg.cut pads at the high end only: a volume zero-padded by PAD at the low end, cut at start + PAD, is the box of a negative start
    padded = D.Case("c", np.pad(img, ((0, 0),) + ((PAD, 0),) * 3))
    box = np.stack([D.cut(padded, tuple(s + PAD for s in st), CUT_CROP)[0] for st in CUT_STARTS])
    assert box.dtype == np.float32 and any((b == 0).all() for b in box[:, :, 0]) and bool((box != 0).any())
    imgd = torch.from_numpy(img).to(DEV)
    st = torch.tensor(CUT_STARTS, dtype=torch.int32, device=DEV)
    n_out = box.size
    old = ops.seg_cut_patches(imgd, st, CUT_CROP)
    assert _bytes(old) == box.tobytes(), "the un-mirrored cutter at these starts"
    for code in range(8):
        full = torch.full((n_out + 64,), -7.0, dtype=torch.float32, device=DEV)
        got = ops.seg_cut_patches(imgd, st, CUT_CROP, out=full[:n_out].view(box.shape), flip=code)
        torch.cuda.synchronize()
        assert _bytes(got) == flip_axes(box, code, 2).tobytes(), f"code {code}"
        assert bool((full[n_out:] == -7.0).all())
    # code 0 through the NEW entry point gives the old entry point's bytes
    raw = torch.empty_like(old)
    lib().call("pcrl_seg_cut_patches_mirror", imgd, int(src == np.float16), st, raw, len(CUT_STARTS), C, *CUT_SHAPE, *CUT_CROP, 0, stream_handle())
    assert _bytes(raw) == _bytes(old)


def test_mirrored_cutter_refuses_bad_codes_and_what_the_cutter_refuses():
    img = torch.zeros((1, 8, 8, 8), device=DEV)
    st = torch.zeros((1, 3), dtype=torch.int32, device=DEV)
    out = torch.empty((1, 1, 8, 8, 8), device=DEV)
    for bad in (8, -1, 16, True, 1.0, "x"):
        with pytest.raises(PcrlError, match="no mirror code"):
            ops.seg_cut_patches(img, st, (8, 8, 8), flip=bad)
    for bad in (8, -1):
        with pytest.raises(PcrlError, match="no mirror code"):
            lib().call("pcrl_seg_cut_patches_mirror", img, 0, st, out, 1, 1, 8, 8, 8, 8, 8, 8, bad, stream_handle())
    with pytest.raises(PcrlError):
        lib().call("pcrl_seg_cut_patches_mirror", img, 0, st, out, 1, 1, 8, 8, 8, 8, 8, 6, 1, stream_handle())       # cz is no multiple of 4
    with pytest.raises(PcrlError):
        ops.seg_cut_patches(img, st, (8, 8, 6), flip=1)
    room = torch.empty(512 + 4, device=DEV)
    with pytest.raises(PcrlError, match="16-byte aligned"):
        lib().call("pcrl_seg_cut_patches_mirror", img, 0, st, room[1:513], 1, 1, 8, 8, 8, 8, 8, 8, 4, stream_handle())


# ---- the accumulating head on raw activations ---------------------------------------------------------------------------------------------------------
HEAD_SHAPES = [(3, (3, 5, 7)), (64, (8, 8, 16))]


def _head_inputs(N, sp, K, dtype, seed, n_act=3):
    """n_act activations [N, *sp, 64] (a ReLU output, as the decoder hands over) on the device, the weight and the bias."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    acts = [torch.relu(torch.randn((N,) + tuple(sp) + (64,), generator=g, device=DEV)).to(dtype) for _ in range(n_act)]
    w = 0.2 * torch.randn((K, 64), generator=g, device=DEV)
    b = torch.randn((K,), generator=g, device=DEV)
    return acts, w, b


def _ndhwc(rows):
    """[N, D, H, W, 64] contiguous rows -> the logical [N, 64, D, H, W] activation in NDHWC memory."""
    return rows.permute(0, 4, 1, 2, 3)


@pytest.mark.parametrize("K", [1, 3, 7])
@_DTYPES
def test_a_first_pass_unmirrors_to_the_plain_kernels_bytes(dtype, K):
    for N, sp in HEAD_SHAPES:
        (a,), w, b = _head_inputs(N, sp, K, dtype, seed=100 * K + N, n_act=1)
        plain = ops.seg_head_logits(_ndhwc(a), w, b, dtype)
        want = _bytes(plain)
        n = plain.numel()
        for code in range(8):
            full = torch.full((n + 64,), float("nan"), dtype=torch.float32, device=DEV)         # a sentinel that survives neither a read nor a miss
            seen = flip_axes(a, code, 1)                                                             # what the network is shown
            assert code == 0 or not torch.equal(seen, a)
            got = ops.seg_head_logits_acc(_ndhwc(seen), w, b, dtype, full[:n], flip=code, first=True, scale=1.0)
            torch.cuda.synchronize()
            assert got.shape == plain.shape and got.data_ptr() == full.data_ptr()
            assert _bytes(got) == want, f"N={N} crop={sp} code {code}: a first pass overwrites every element with the un-mirrored plain logit"
            assert bool(full[n:].isnan().all()), "the bytes behind z are left alone"


def _sequence(acts, w, b, dtype, codes, scale, z):
    """The passes of one batch into z: pass i shows acts[i % len(acts)] as the patch mirrored by codes[i]."""
    for i, code in enumerate(codes):
        last = i == len(codes) - 1
        ops.seg_head_logits_acc(_ndhwc(acts[i % len(acts)]), w, b, dtype, z, flip=code, first=i == 0, scale=scale if last else 1.0)
    torch.cuda.synchronize()
    return z


@pytest.mark.parametrize("K", [1, 3, 7])
@_DTYPES
def test_a_sequence_of_passes_equals_the_float32_restatement(dtype, K):
    """Codes [0, 3, 4, 7] with the last pass scaled by 1/4 (exact), and all eight with the last scaled by float32(1/24) (what three checkpoints under
    mirror `all` would use on their last pass; it pins the rounding of the one multiplication).  Each pass's un-mirrored logits are the PLAIN kernel's
    output for the activation it was shown, flipped back on the host."""
    for N, sp in HEAD_SHAPES:
        acts, w, b = _head_inputs(N, sp, K, dtype, seed=7 * K + N)
        plain = [ops.seg_head_logits(_ndhwc(a), w, b, dtype) for a in acts]
        for codes, scale in (([0, 3, 4, 7], 0.25), (list(range(8)), np.float32(1 / 24))):
            passes = [flip_axes(plain[i % len(acts)], code, 1).cpu().numpy() for i, code in enumerate(codes)]
            want = tta_logits(passes, scale)
            runs = []
            for _ in range(2):
                z = torch.full(plain[0].shape, -7.0, dtype=torch.float32, device=DEV)
                runs.append(_bytes(_sequence(acts, w, b, dtype, codes, scale, z)))
            assert runs[0] == runs[1], "two runs give identical bytes"
            assert runs[0] == want.tobytes(), f"N={N} crop={sp} codes {codes} scale {scale}"


@pytest.mark.parametrize("K", [2, 4, 5, 6])
@_DTYPES
def test_a_sequence_of_passes_at_the_other_class_counts(dtype, K):
    """The instantiations the two tests above leave out: one sequence with a z mirror (codes 4 and 7) and non-first passes, the last one scaled by
    float32(1/3), on the smaller shape -- the same restatement, bit for bit."""
    N, sp = HEAD_SHAPES[0]
    acts, w, b = _head_inputs(N, sp, K, dtype, seed=7 * K + N)
    plain = [ops.seg_head_logits(_ndhwc(a), w, b, dtype) for a in acts]
    codes, scale = [4, 3, 7], np.float32(1 / 3)
    want = tta_logits([flip_axes(plain[i % len(acts)], code, 1).cpu().numpy() for i, code in enumerate(codes)], scale)
    z = torch.full(plain[0].shape, -7.0, dtype=torch.float32, device=DEV)
    assert _bytes(_sequence(acts, w, b, dtype, codes, scale, z)) == want.tobytes(), f"N={N} crop={sp} codes {codes} K={K}"


@_DTYPES
def test_accumulating_head_refuses_bad_codes_grids_and_buffers(dtype):
    N, sp, K = 3, (3, 5, 7), 3
    S = 105
    (a,), w, b = _head_inputs(N, sp, K, dtype, seed=5, n_act=1)
    z = torch.zeros((N,) + sp + (K,), device=DEV)
    for bad in (8, -1, True, 2.0):
        with pytest.raises(PcrlError, match="no mirror code"):
            ops.seg_head_logits_acc(_ndhwc(a), w, b, dtype, z, flip=bad)
    for out in (None, z.double(), z.reshape(-1)[:-1], z.cpu(), z.permute(0, 2, 1, 3, 4)):
        with pytest.raises(PcrlError, match="out must be"):
            ops.seg_head_logits_acc(_ndhwc(a), w, b, dtype, out, flip=1)
    with pytest.raises(PcrlError, match="not finite"):
        ops.seg_head_logits_acc(_ndhwc(a), w, b, dtype, z, scale=float("nan"))

    def raw(S_, grid, flip, K_=K):
        lib().call("pcrl_seg_head_logits_acc", a, w, b, z, N, S_, K_, dtype_code(dtype), *grid, flip, 1, 1.0, stream_handle())

    raw(S, sp, 7)
    with pytest.raises(PcrlError, match="no mirror code"):
        raw(S, sp, 8)
    for S_, grid in ((S, (3, 5, 8)), (S - 1, sp), (S, (5, 3, 0)), (S, (-3, -5, 7)), (S + 15, sp)):
        with pytest.raises(PcrlError, match="voxels per sample against a grid"):
            raw(S_, grid, 1)
    for K_ in (0, 8):
        with pytest.raises(PcrlError):
            raw(S, sp, 1, K_)
    assert not bool(z.isnan().any())


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------------------
K, B, CROP = 3, 2, (16, 16, 8)                           # the tiny Segmenter3d of test_seg_sw_gpu.py


def _model(dtype, seed=0):
    torch.manual_seed(seed)
    return Segmenter3d(K).cuda().eval().set_compute_dtype(dtype)


def _phantom():
    shape = D.synthetic_shape(CROP)
    case = D.synthetic_case(5, 0, shape, K)
    axes, weights = D.windows(shape, CROP, 0.5), D.blend_weights(CROP, "gaussian")
    starts = D.window_starts(axes)
    assert any(n % c for n, c in zip(shape, CROP)) and len(starts) > B
    xs = np.stack([D.cut(case, st, CROP)[0] for st in starts])                 # host-cut patches [P, C, *crop]
    return shape, case, axes, weights, starts, xs


def _restated_num(models, codes, case, shape, axes, weights, starts, xs):
    """blend32's num of the logits tta_logits forms, per batch, from model.infer_logits(torch.flip(host-cut patches)), un-mirrored on the host;
    passes in sliding_window's order: models in list order, codes ascending."""
    z = []
    for i in range(0, len(starts), B):
        x = torch.from_numpy(xs[i:i + B]).cuda()
        passes = [flip_axes(m.infer_logits(flip_axes(x, code, 2)), code, 1).cpu().numpy() for m in models for code in codes]
        z.append(tta_logits(passes, np.float32(1.0 / len(passes))))
    num, _ = blend32(np.concatenate(z), axes, weights, shape)
    return num


@_DTYPES
def test_mirrored_sliding_window_is_the_restatement_of_host_flipped_patches(dtype):
    model = _model(dtype)
    shape, case, axes, weights, starts, xs = _phantom()
    codes = D.parse_mirror("xz")
    assert codes == [0, 1, 4, 5]
    num = _restated_num([model], codes, case, shape, axes, weights, starts, xs)
    mask, probs, sums = sliding_window(model, case, CROP, B, 0.5, "gaussian", want_probs=True, mirror=codes)
    assert np.array_equal(mask.cpu().numpy(), mask_of(num, case.seg)) and 0 < int(mask.count_nonzero())
    assert probs.shape == (K,) + shape and float(sums[4 * K]) == float(np.prod(shape))
    plain = sliding_window(model, case, CROP, B, 0.5, "gaussian")[0]
    assert not torch.equal(plain, mask), "the mirrored passes change the prediction of a random network"


@_DTYPES
def test_two_models_under_mirror_all_are_the_restatement(dtype):
    models = [_model(dtype, 0), _model(dtype, 1)]
    shape, case, axes, weights, starts, xs = _phantom()
    codes = D.parse_mirror("all")
    num = _restated_num(models, codes, case, shape, axes, weights, starts, xs)
    bare = D.Case(case.name, case.img)
    mask, probs, sums = sliding_window(models[0], bare, CROP, B, 0.5, "gaussian", mirror=codes, models=models)
    assert np.array_equal(mask.cpu().numpy(), mask_of(num)) and probs is None and sums is None
    # `model` is the source of n_class, wb and wd only: the logits come from `models`
    again = sliding_window(models[1], bare, CROP, B, 0.5, "gaussian", mirror=codes, models=models)[0]
    assert torch.equal(again, mask)
    swapped = sliding_window(models[0], bare, CROP, B, 0.5, "gaussian", mirror=codes, models=models[:1])[0]
    assert not torch.equal(swapped, mask)
    with pytest.raises(ValueError):
        sliding_window(models[0], bare, CROP, B, 0.5, "gaussian", mirror=(0, 8))
    with pytest.raises(ValueError):
        sliding_window(models[0], bare, CROP, B, 0.5, "gaussian", models=[])


@_DTYPES
def test_defaults_return_todays_bytes_and_make_todays_calls(dtype):
    model = _model(dtype)
    shape, case, *_ = _phantom()
    want = sliding_window(model, case, CROP, B, 0.5, "gaussian", want_probs=True)
    names = ("pcrl_seg_cut_patches", "pcrl_seg_head_logits", "pcrl_seg_cut_patches_mirror", "pcrl_seg_head_logits_acc")
    with lib().count_calls(*names) as n:
        got = sliding_window(model, case, CROP, B, 0.5, "gaussian", want_probs=True, mirror=(0,), models=None)
    assert n.get("pcrl_seg_cut_patches") == n.get("pcrl_seg_head_logits") == 2 and "pcrl_seg_cut_patches_mirror" not in n and "pcrl_seg_head_logits_acc" not in n
    for a, b in zip(want, got):
        assert _bytes(a) == _bytes(b)
    listed = sliding_window(model, case, CROP, B, 0.5, "gaussian", want_probs=True, mirror=D.parse_mirror("none"), models=[model])
    for a, b in zip(want, listed):
        assert _bytes(a) == _bytes(b)
    with lib().count_calls(*names) as n:
        sliding_window(model, case, CROP, B, 0.5, "gaussian", mirror=D.parse_mirror("y"))
    # two batches x two passes: the first pass of a batch (code 0, overwrite, scale 1) IS infer_logits' default, i.e. the plain kernels
    assert n == {"pcrl_seg_cut_patches": 2, "pcrl_seg_head_logits": 2, "pcrl_seg_cut_patches_mirror": 2, "pcrl_seg_head_logits_acc": 2}, n
    # infer_logits: the defaults are the plain kernel; a first pass of code 0 at scale 1 writes the same bytes through the other one
    x = torch.randn((2, 1) + CROP, generator=torch.Generator().manual_seed(1)).cuda()
    z0 = model.infer_logits(x)
    z1 = model.infer_logits(x, out=torch.empty_like(z0), flip=0, accumulate=False, scale=1.0)
    with lib().count_calls(*names) as n:
        z2 = model.infer_logits(flip_axes(x, 6, 2), out=torch.full_like(z0, float("nan")), flip=6)
    assert n == {"pcrl_seg_head_logits_acc": 1}
    z3 = model.infer_logits(x, out=z0.clone(), accumulate=True, scale=0.5)
    assert _bytes(z0) == _bytes(z1) and not bool(z2.isnan().any()) and _bytes(z3) == _bytes(z0)      # (z + z) * 0.5 is exact
    with pytest.raises(ValueError, match="out"):
        model.infer_logits(x, flip=1)


def test_evaluate_sliding_passes_the_mirror_through():
    model = _model(torch.bfloat16)
    shape = D.synthetic_shape(CROP)
    cases = [D.synthetic_case(3, i, shape, K) for i in range(2)]
    codes = D.parse_mirror("yz")
    table = []
    for case in cases:
        mask = sliding_window(model, case, CROP, B, 0.5, "gaussian", mirror=codes)[0].cpu().numpy()
        table.append(counts_of(mask, case.seg, K).tolist())
    per, mean = dice_from_counts(table)
    got = evaluate_sliding(model, cases, CROP, B, 0.5, "gaussian", mirror=codes)
    assert got["dice"] == per and got["mean_dice"] == mean and got["cases"] == 2 and sum(r[k][2] for r in table for k in range(K)) > 0
    plain = evaluate_sliding(model, cases, CROP, B, 0.5, "gaussian")
    assert plain["dice"] != per, "without the mirror the counts are other counts"


# ---- the commands -------------------------------------------------------------------------------------------------------------------------------------
def _cli(*argv, timeout=300):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "seg3d.py"), *argv], cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


_TODAY_VAL = re.compile(r"^Val: \[\d+\]\tloss \d+\.\d{4}\tmean Dice \d\.\d{4}\t\(2 cases\)$")
_TODAY_TEST = re.compile(r"^Test: \((last|best) epoch \d+\)\tloss \d+\.\d{4}\tmean Dice \d\.\d{4}\t\(2 cases\)\tper class( \d\.\d{4}){3}$")


def test_train_validates_mirrored_and_predict_runs_an_ensemble(tmp_path):
    out_dir = str(tmp_path / "out")
    log = _cli("train", "--data", "synthetic", "--phase", "scratch", "--epochs", "1", "--steps_per_epoch", "2", "--b", "2", "--crop", "16,16,8", "--save_best",
               "--output", out_dir, "--val_overlap", "0.5", "--val_mirror", "x")
    val = [ln for ln in log.splitlines() if ln.startswith("Val: [")]
    test = [ln for ln in log.splitlines() if ln.startswith("Test: (")]
    tail = "\toverlap 0.5 gaussian\tmirror x"
    assert len(val) == 2 and len(test) == 1, log[-2000:]
    for ln in val + test:
        assert ln.endswith(tail), ln
    assert _TODAY_VAL.match(val[0][:-len(tail)]) and _TODAY_TEST.match(test[0][:-len(tail)]), (val, test)
    best = os.path.join(out_dir, "pcrlv2_seg3d_scratch_1.0_best.pt")
    last = os.path.join(out_dir, "pcrlv2_seg3d_scratch_1.0_1.pt")
    assert os.path.isfile(best) and os.path.isfile(last), sorted(os.listdir(out_dir))
    data, pred = str(tmp_path / "data"), str(tmp_path / "pred")
    D.write_synthetic(data, ["p0", "p1"], (20, 18, 12), K, seed=9)
    with open(os.path.join(data, "two.txt"), "w") as f:
        f.write("p0\np1\n")
    _cli("predict", "--data", data, "--list", "two.txt", "--weights", best + "," + last, "--out", pred, "--crop", "16,16,8", "--b", "4", "--mirror", "all",
         "--overlap", "0.5", "--probs")
    for name in ("p0", "p1"):
        m, p = np.load(os.path.join(pred, name + "_pred.npy")), np.load(os.path.join(pred, name + "_prob.npy"))
        assert m.shape == (20, 18, 12) and m.dtype == np.uint8 and p.shape == (K, 20, 18, 12) and p.dtype == np.float16
        for k in range(K):
            decided = p[k] != np.float16(0.5)
            assert np.array_equal(((m >> k) & 1).astype(bool)[decided], (p[k] > np.float16(0.5))[decided]), (name, k)
