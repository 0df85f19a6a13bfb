"""pcrl_auroc_counts (csrc/auroc.hip) against a numpy restatement of its three integers by explicit pairwise comparison (O(M^2), fine at these
sizes), with scipy's average ranks as a second witness: 2 (R+ - P (P + 1) / 2) is the first integer.  Equality is EXACT: there is no tolerance."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pcrlv2_amd import ops2d  # noqa: E402

pytestmark = pytest.mark.gpu


def pair_counts(s, y):
    """numpy: s float32 [M,K], y uint8 [M,K] -> int64 [K,3]"""
    out = np.zeros((s.shape[1], 3), np.int64)
    for k in range(s.shape[1]):
        pos, neg = s[y[:, k] != 0, k], s[y[:, k] == 0, k]
        gt = (pos[:, None] > neg[None, :]).sum(dtype=np.int64)
        eq = (pos[:, None] == neg[None, :]).sum(dtype=np.int64)
        out[k] = (2 * gt + eq, pos.size, neg.size)
    return out


def rank_counts(s, y):
    """scipy.stats.rankdata (average ranks): 2 (R+ - P (P + 1) / 2), an integer because the doubled average ranks are."""
    from scipy.stats import rankdata
    out = []
    for k in range(s.shape[1]):
        r2 = np.rint(2 * rankdata(s[:, k].astype(np.float64), method="average")).astype(np.int64)      # doubled ranks: integers
        P = int((y[:, k] != 0).sum())
        out.append(int(r2[y[:, k] != 0].sum()) - P * (P + 1))
    return np.asarray(out, np.int64)


def _scores(kind, M, K, rng):
    if kind == "continuous":
        return rng.random((M, K), dtype=np.float32)
    if kind == "ties8":
        return (rng.integers(0, 8, (M, K)) / 8.0).astype(np.float32)
    if kind == "equal":
        return np.full((M, K), 0.25, np.float32)
    s = rng.random((M, K), dtype=np.float32) - np.float32(0.5)                 # "zeros": a column holding both signed zeros, among others
    z = np.where(rng.random((M, K)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    s = np.where(rng.random((M, K)) < 0.6, z, s).astype(np.float32)
    if M >= 2:
        s[0, 0], s[1, 0] = np.float32(-0.0), np.float32(0.0)
        assert np.signbit(s[0, 0]) and not np.signbit(s[1, 0])
    return s


def _labels(M, K, rng):
    y = (rng.random((M, K)) < 0.3).astype(np.uint8)
    if K >= 14:
        y[:, 1] = 0                     # no positives
        y[:, 2] = 1                     # no negatives
        y[:, 3] = 0
        y[M // 2, 3] = 1                # a single positive
    return y


def _device(s, y):
    dev = torch.device("cuda")
    return torch.from_numpy(s).to(dev), torch.from_numpy(y).to(dev)


@pytest.mark.parametrize("kind", ["continuous", "ties8", "equal", "zeros"])
@pytest.mark.parametrize("K", [1, 14])
@pytest.mark.parametrize("M", [1, 2, 63, 64, 65, 257, 1025])
def test_counts_are_exact(M, K, kind):
    rng = np.random.default_rng(1000 * M + K)
    s, y = _scores(kind, M, K, rng), _labels(M, K, rng)
    ref = pair_counts(s, y)
    assert np.array_equal(ref[:, 0], rank_counts(s, y)), "the two witnesses disagree"
    sd, yd = _device(s, y)
    got = ops2d.auroc_counts(sd, yd).cpu().numpy()
    assert got.dtype == np.int64 and np.array_equal(got, ref), (got.tolist(), ref.tolist())
    per, mean = ops2d.auroc(sd, yd)
    assert per.dtype == torch.float64 and per.shape == (K,)
    want = np.array([c / (2.0 * p * q) if p and q else np.nan for c, p, q in ref.tolist()], np.float64)
    assert np.array_equal(per.numpy(), want, equal_nan=True)
    valid = want[~np.isnan(want)]
    if valid.size:
        assert mean == math.fsum(valid) / valid.size or abs(mean - float(valid.mean())) <= valid.size * 2.0 ** -53
    else:
        assert math.isnan(mean)
    if K >= 14:
        assert math.isnan(want[1]) and math.isnan(want[2])          # left out of the mean above
        if M > 1:
            assert ref[3, 1] == 1 and not math.isnan(want[3])


def test_label_columns_without_a_class_and_signed_zeros():
    s = np.array([[-0.0, 0.3], [0.0, 0.3], [0.0, 0.1], [-0.0, 0.9]], np.float32)
    y = np.array([[1, 0], [0, 0], [1, 0], [0, 0]], np.uint8)
    got = ops2d.auroc_counts(*_device(s, y)).cpu().tolist()
    assert got == [[4, 2, 2], [0, 0, 4]]                             # all four (positive, negative) pairs of column 0 tie: -0.0 == +0.0
    per, mean = ops2d.auroc(*_device(s, y))
    assert per[0] == 0.5 and math.isnan(per[1]) and mean == 0.5
    per, mean = ops2d.auroc(*_device(s, np.ones_like(y)))
    assert bool(torch.isnan(per).all()) and math.isnan(mean)


def test_more_rows_than_one_block_of_rows_and_one_tile():
    """M past the 1024 rows a block owns and the 1024-row tile, not a multiple of either: the chest validation set's class count."""
    rng = np.random.default_rng(5)
    M, K = 2 * 1024 + 77, 14
    s, y = _scores("ties8", M, K, rng), (rng.random((M, K)) < 0.1).astype(np.uint8)
    assert np.array_equal(ops2d.auroc_counts(*_device(s, y)).cpu().numpy(), pair_counts(s, y))
