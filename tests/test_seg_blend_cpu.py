"""Sliding-window geometry, blending weights, the float32 restatement of the blend against the float64 one, and the refused flags (no GPU)."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pcrlv2_amd import data_seg as D  # noqa: E402
from pcrlv2_amd.train_seg import sliding_window  # noqa: E402
from seg_blend_reference import blend32, blend64, mask_of  # noqa: E402


@pytest.mark.parametrize("overlap", [0, 0.25, 0.5, 0.75])
@pytest.mark.parametrize("crop", [8, 16])
@pytest.mark.parametrize("size", [1, 7, 8, 9, 12, 16, 17, 40])
def test_window_axis_covers_the_axis_with_ascending_patches_inside_it(size, crop, overlap):
    s = D.window_axis(size, crop, overlap)
    assert all(isinstance(v, int) for v in s) and all(a < b for a, b in zip(s, s[1:])), "ascending and distinct"
    end = max(size, crop)
    assert s[0] == 0 and s[-1] + crop == end and all(0 <= v and v + crop <= end for v in s)
    covered = np.zeros(size, dtype=int)
    for v in s:
        covered[v:v + crop] += 1
    assert covered.min() >= 1, "every voxel is covered"
    if size > crop:
        interval = max(1, int(crop * (1 - overlap)))
        assert len(s) <= -(-(size - crop) // interval) + 1 and all(b - a <= interval for a, b in zip(s, s[1:]))
    if overlap == 0 and size % crop == 0:
        assert s == [a for a, _ in D.tile_axis(size, crop)]


def test_windows_run_in_x_major_order():
    axes = D.windows((17, 12, 9), (8, 8, 8), 0.5)
    assert axes == [[0, 4, 8, 9], [0, 4], [0, 1]]
    starts = D.window_starts(axes)
    nx, ny, nz = (len(a) for a in axes)
    for ix in range(nx):
        for iy in range(ny):
            for iz in range(nz):
                assert starts[(ix * ny + iy) * nz + iz] == (axes[0][ix], axes[1][iy], axes[2][iz])


@pytest.mark.parametrize("overlap", [-0.1, 0.76, 1.0, float("nan"), "half"])
def test_overlap_outside_its_range_is_refused(overlap):
    with pytest.raises(SystemExit, match="a fraction of the crop"):
        D.window_axis(16, 8, overlap)


def test_blend_weights_are_positive_symmetric_float32_tables():
    for crop in [(8, 8, 8), (16, 16, 8), (64, 64, 32), (24, 8, 40)]:
        for window in D.WINDOWS:
            ws = D.blend_weights(crop, window)
            assert len(ws) == 3
            for w, c in zip(ws, crop):
                assert w.dtype == np.float32 and w.shape == (c,) and bool((w > 0).all()) and np.array_equal(w, w[::-1])
                if window == "constant":
                    assert bool((w == 1).all())
                else:
                    i = np.arange(c, dtype=np.float64)
                    assert np.array_equal(w, np.exp(-0.5 * ((i - (c - 1) / 2) / (0.125 * c)) ** 2).astype(np.float32))
                    assert w.argmax() in (c // 2 - 1, c // 2) and w[0] < w[c // 2]
    with pytest.raises(SystemExit, match="gaussian, constant"):
        D.blend_weights((8, 8, 8), "hann")


@pytest.mark.parametrize("window", D.WINDOWS)
@pytest.mark.parametrize("overlap", [0.5, 0.75])
def test_float32_restatement_agrees_with_the_float64_one_outside_its_rounding_band(overlap, window):
    """A prediction is the sign of num.  The float32 sum differs from the float64 one by at most (n_cover + 2) 2^-24 sum |w z| to first order (the
    n_cover additions, the product and the two multiplications of the weight), so outside that band the two masks must agree; at most 0.1 % of the
    voxel-classes may lie inside it (with this seed: none)."""
    shape, crop, K = (17, 12, 9), (8, 8, 8), 3
    axes, weights = D.windows(shape, crop, overlap), D.blend_weights(crop, window)
    P = len(D.window_starts(axes))
    z = np.random.default_rng(20240 + int(overlap * 100)).standard_normal((P,) + crop + (K,)).astype(np.float32)
    n32, d32 = blend32(z, axes, weights, shape)
    n64, d64, absum, cover = blend64(z, axes, weights, shape)
    assert cover.min() >= 1 and bool((d32 > 0).all())
    band = (cover[..., None] + 2) * 2.0 ** -24 * absum
    outside = np.abs(n64) > band
    inside = int((~outside).sum())
    print(f"[blend restatements overlap {overlap} {window}] voxel-classes inside the band: {inside} of {outside.size}; covering patches up to {cover.max()}")
    assert inside <= 0.001 * outside.size
    assert np.array_equal((n32 >= 0)[outside], (n64 >= 0)[outside])
    assert bool((np.abs(n32 - n64) <= band).all()), "the band is the float32 sum's error bound"
    assert bool((np.abs(d32 - d64) <= (cover + 2) * 2.0 ** -24 * d64).all())
    m32, m64 = mask_of(n32), mask_of(n64)
    assert np.array_equal(m32, m64) or inside > 0


# ---- command line -----------------------------------------------------------------------------------------------------------------
def _cli(*argv):
    r = subprocess.run([sys.executable, "seg3d.py", *argv], cwd=ROOT, capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout + r.stderr


_TRAIN = ("train", "--data", "synthetic", "--phase", "scratch")
_PREDICT = ("predict", "--data", "nowhere", "--list", "none.txt", "--weights", "absent.pt", "--out", "nowhere_out")


@pytest.mark.parametrize("argv,message", [
    (_TRAIN + ("--val_overlap", "0.8"), "--val_overlap 0.8: a fraction of the crop in [0, 0.75]"),
    (_TRAIN + ("--val_overlap", "-0.5"), "--val_overlap -0.5: a fraction of the crop"),
    (_TRAIN + ("--val_overlap", "0.5", "--val_window", "hann"), "--val_window hann: one of gaussian, constant"),
    (_PREDICT + ("--overlap", "1"), "--overlap 1.0: a fraction of the crop in [0, 0.75]"),
    (_PREDICT + ("--overlap", "-1"), "--overlap -1.0: a fraction of the crop"),
    (_PREDICT + ("--overlap", "0.5", "--window", "box"), "--window box: one of gaussian, constant"),
    (_PREDICT + ("--probs",), "--probs writes the blended probabilities of overlapping windows: it needs --overlap > 0"),
    (_PREDICT + ("--overlap", "0", "--probs"), "it needs --overlap > 0"),
])
def test_refused_flags_exit_with_their_message_before_any_gpu_work(argv, message, tmp_path):
    code, out = _cli(*argv, *(("--output", str(tmp_path)) if argv[0] == "train" else ()))
    assert code != 0 and message in out, out
    assert "Traceback" not in out, out


def test_a_logit_buffer_above_max_bytes_is_refused_with_its_size(tmp_path):
    case = D.synthetic_case(0, 0, (40, 36, 20), 3)
    model = types.SimpleNamespace(n_class=3)         # the refusal comes before the model or a device is looked at
    with pytest.raises(SystemExit, match=r"phantom000: the logits of its \d+ patches at overlap 0.5 need .* GiB, above the limit of .* smaller --overlap"):
        sliding_window(model, case, (16, 16, 8), 2, 0.5, "gaussian", max_bytes=1 << 20)
