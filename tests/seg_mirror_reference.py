"""Restatements of mirror test-time augmentation and checkpoint ensembling (csrc/seg_head.hip's accumulating logits kernel, csrc/seg_blend.hip's
mirrored cutter, train_seg.sliding_window(mirror=..., models=...)) with numpy / torch.  Not a test file.

A mirror code has bit 0 = x, bit 1 = y, bit 2 = z: the first, second and third SPATIAL axis of an array whose spatial axes start at `first_axis`."""
import numpy as np
import torch


def mirror_dims(code, first_axis):
    """The array axes mirror code `code` flips."""
    code = int(code)
    assert 0 <= code <= 7
    return [first_axis + a for a in range(3) if code >> a & 1]


def flip_axes(arr, code, first_axis):
    """`arr` (numpy array or torch tensor) mirrored along the axes of `code`; a copy, contiguous.  Its own inverse."""
    dims = mirror_dims(code, first_axis)
    if torch.is_tensor(arr):
        return torch.flip(arr, dims).contiguous() if dims else arr.clone()
    return np.ascontiguousarray(np.flip(arr, dims)) if dims else np.array(arr, copy=True)


def tta_logits(passes, scale):
    """What the per-case buffer holds after the passes of one batch: `passes` are the UN-MIRRORED float32 logits of each pass in pass order; the first
    overwrites, every later one is added in float32 -- one addition at a time -- and the last pass's sum is multiplied by float32(scale), one
    multiplication.  (Earlier passes multiply by 1.0f, which is exact.)"""
    assert len(passes) >= 1
    acc = np.array(passes[0], dtype=np.float32, copy=True)
    for p in passes[1:]:
        p = np.asarray(p)
        assert p.dtype == np.float32 and p.shape == acc.shape
        acc = acc + p
        assert acc.dtype == np.float32
    out = acc * np.float32(scale)
    assert out.dtype == np.float32
    return out
