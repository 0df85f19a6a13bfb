"""Label maps through the tools around the softmax segmenter, on the GPU: `prepare --classes` and `restore --labelmap` are second builders of the 256-entry
tables of the UNCHANGED kernels pcrl_segprep_resample / pcrl_segprep_restore, and the clean-up takes label maps through pcrl_seg_labelmap_to_bits /
_keep and the bitmask machinery, at most 7 classes at a time.  Everything here is an equality: no tolerance."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import seg_prep_reference as R  # noqa: E402
from pcrlv2_amd import seg_prep as SP  # noqa: E402
from pcrlv2_amd import train_seg as T  # noqa: E402
from test_seg_prep_gpu import source  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_prepare_with_classes_writes_the_label_map_of_the_same_voxels_the_regions_give():
    """Disjoint sets as --regions give one bit per voxel; the same sets as --classes must give that bit's index + 1 at the same voxels, and the same image."""
    src, lab = source((24, 22, 12), 2, "float32", 16, pad=(1, 3, 5))
    assert set(np.unique(lab).tolist()) >= {0, 1, 2, 3, 4}
    common = dict(spacing=(1.5, 1.25, 1.0), crop_nonzero=True, norm="zscore")
    bits = SP.prepare_case(list(src), lab, (1.0, 0.9, 1.1), SP.PrepConfig(regions=SP.parse_regions("1;2;3,4"), **common), torch.device(DEV))
    maps = SP.prepare_case(list(src), lab, (1.0, 0.9, 1.1), SP.PrepConfig(regions=[], classes=SP.parse_classes("1;2;3,4"), **common), torch.device(DEV))
    want = np.zeros_like(bits["seg"])
    for i in range(3):
        want[bits["seg"] == (1 << i)] = i + 1
    assert set(np.unique(bits["seg"]).tolist()) <= {0, 1, 2, 4} and int(maps["seg"].max()) == 3
    assert np.array_equal(maps["seg"], want) and maps["img"].tobytes() == bits["img"].tobytes()


@pytest.mark.parametrize("prep,box,orig", [((13, 8, 7), (1, 3, 5, 9, 11, 7), (13, 15, 14)), ((9, 11, 7), (1, 3, 5, 9, 11, 7), (11, 17, 13))])
def test_restore_paints_class_indices(prep, box, orig):
    rng = np.random.default_rng(3)
    K = 16
    pred = rng.integers(0, K, prep).astype(np.uint8)
    values = [0] + [int(v) for v in rng.permutation(np.arange(20, 20 + K - 1))]
    meta = {"prep_shape": np.array(prep), "orig_shape": np.array(orig),
            "box": np.array([box[0], box[0] + box[3], box[1], box[1] + box[4], box[2], box[2] + box[5]])}
    lm, label = SP.restore_case(pred, meta, torch.device(DEV), values, labelmap=True)
    want, want_label = R.restore(pred, box, orig, SP.labelmap_paint_table(values))
    assert np.array_equal(lm, want) and np.array_equal(label, want_label)
    assert np.array_equal(label, np.asarray(values, dtype=np.uint8)[lm]), "class index i -> v_i"


@pytest.mark.parametrize("K", [4, 9, 16])
def test_clean_up_of_a_label_map_is_the_clean_up_of_each_class_as_a_bitmask(K):
    """postprocess_labelmap against postprocess_mask run on ONE class at a time (K - 1 single-bit masks): the same voxels survive, the background and
    bit 7 stay, the report has a row per class."""
    rng = np.random.default_rng(K)
    shape = (12, 14, 10)
    lab = np.zeros(shape, dtype=np.uint8)
    for _ in range(60):      # small blobs of random classes: several components per class, some of one voxel
        c = [int(rng.integers(0, n - 2)) for n in shape]
        e = [int(rng.integers(1, 4)) for _ in shape]
        lab[c[0]:c[0] + e[0], c[1]:c[1] + e[1], c[2]:c[2] + e[2]] = rng.integers(1, K)
    lab[0, 0, :] |= 0x80
    labd = torch.from_numpy(lab).to(DEV)
    for keep, min_voxels, conn in (((1, K - 1), 0, 6), ((), 3, 26), (tuple(range(1, K)), 2, 18)):
        got, report = T.postprocess_labelmap(labd, K, keep, min_voxels, conn)
        want = lab.copy()
        for k in range(1, K):
            one = torch.from_numpy(((lab & 0x7F) == k).astype(np.uint8)).to(DEV)
            kept, rep = T.postprocess_mask(one, 1, (0,) if k in keep else (), min_voxels, conn)
            gone = (((lab & 0x7F) == k) & (kept.cpu().numpy() == 0))
            want[gone] &= 0x80
            assert report[k] == rep[0], (k, keep, min_voxels, conn)
        assert len(report) == K and report[0]["before"] is None
        assert np.array_equal(got.cpu().numpy(), want), (keep, min_voxels, conn)
        assert np.array_equal(got.cpu().numpy() & 0x80, lab & 0x80)
