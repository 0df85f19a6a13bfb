#!/usr/bin/env python3
"""What data_seg.CropLoader yields WITHOUT augmentation: the sha256 of its first two batches on the synthetic cases, for two (seed, rank, epoch)
triples.

tests/test_seg_aug_cpu.py compares the loader against tests/golden/seg_croploader_default.npz.  The fixture pins the un-augmented loader -- its
code path and its random stream -- against the revision BEFORE augmentation existed, so it is generated from a checkout of the PARENT commit, never
from the code under test:

    git archive HEAD^ | tar -x -C /tmp/parent
    python tools/make_seg_aug_fixtures.py --tree /tmp/parent        # writes tests/golden/seg_croploader_default.npz

(--tree: the checkout whose pcrlv2_amd.data_seg is imported; default: this one.)  Host code only: no GPU and no built library are needed.
"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "seg_croploader_default.npz")
CROP, B, STEPS, K, C, CASES, CASE_SEED = (16, 16, 8), 4, 2, 3, 2, 8, 42
TRIPLES = ((0, 0, 0), (42, 1, 3))          # (seed, rank, epoch)


def digests(data_seg):
    """-> uint8 [triples][STEPS][32]: sha256 over the image bytes, then the label bytes, of every batch"""
    cases = [data_seg.synthetic_case(CASE_SEED, i, data_seg.synthetic_shape(CROP), K, C) for i in range(CASES)]
    out = np.zeros((len(TRIPLES), STEPS, 32), dtype=np.uint8)
    for t, (seed, rank, epoch) in enumerate(TRIPLES):
        loader = data_seg.CropLoader(cases, CROP, B, STEPS, seed, rank)
        loader.set_epoch(epoch)
        for s, batch in enumerate(loader):
            x, lab = batch
            assert x.dtype.is_floating_point and tuple(x.shape) == (B, C) + CROP and tuple(lab.shape) == (B,) + CROP
            h = hashlib.sha256()
            h.update(x.numpy().tobytes())
            h.update(lab.numpy().tobytes())
            out[t, s] = np.frombuffer(h.digest(), dtype=np.uint8)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tree", default=ROOT, help="the checkout whose pcrlv2_amd.data_seg is imported")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    from pcrlv2_amd import data_seg
    assert os.path.abspath(data_seg.__file__).startswith(os.path.abspath(args.tree) + os.sep), data_seg.__file__
    d = digests(data_seg)
    np.savez_compressed(FIXTURE, digests=d, triples=np.array(TRIPLES, dtype=np.int64))
    print(f"{FIXTURE}: {d.shape[0]} triples x {d.shape[1]} batches from {data_seg.__file__} ({os.path.getsize(FIXTURE)} bytes)")


if __name__ == "__main__":
    main()
