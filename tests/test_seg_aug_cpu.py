"""CPU: what the GPU tests of csrc/seg_augment.hip (test_seg_aug_gpu.py) rest on, and the host side of the augmentation (pcrlv2_amd/data_seg.py, seg3d.py)
-- the float64 restatement equals scipy; the lattice cases are exact in float32; source_extent holds every corner; cut_box; the un-augmented
CropLoader is the parent revision's; the augmented draws; the command line's refusals."""
import argparse
import dataclasses
import hashlib
import itertools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import seg_aug_cases as SC  # noqa: E402
import seg_aug_reference as R  # noqa: E402
from pcrlv2_amd import data_seg as D  # noqa: E402
from pcrlv2_amd import seg3d  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_seg_aug_fixtures as FX  # noqa: E402


# ---- 1. the restatement equals scipy -------------------------------------------------------------------------------------------------------
def _generic_inv(seed=3):
    rng = np.random.default_rng(seed)
    m = D.rotation(np.deg2rad([11.0, -7.0, 23.0])) * 1.13
    return np.concatenate([m, np.array([[0.31], [-0.42], [0.17]])], axis=1).reshape(1, 12), rng


def test_restatement_equals_scipy():
    import scipy.ndimage as ndi
    ext, crop = (22, 20, 14), (16, 16, 8)
    inv, rng = _generic_inv()
    src = rng.standard_normal((1, 2) + ext)
    src_lab = rng.integers(0, 128, (1,) + ext).astype(np.uint8)
    y, lab, s = R.ref_resample(src, src_lab, inv, np.ones((1, 2)), np.zeros((1, 2)), crop)
    M, t = inv.reshape(3, 4)[:, :3], inv.reshape(3, 4)[:, 3]
    # s = M (i + 0.5 - crop / 2) + t + ext / 2 - 0.5 = M i + offset
    offset = M @ (0.5 - np.array(crop) / 2.0) + t + np.array(ext) / 2.0 - 0.5
    for ch in range(2):
        want = ndi.affine_transform(src[0, ch], M, offset=offset, output_shape=crop, order=1, mode="grid-constant", cval=0.0)
        assert np.abs(y[0, ch] - want).max() <= 1e-12
    assert (y[0] == 0).any() and (y[0] != 0).any(), "the case has voxels inside and outside the box"
    want = ndi.affine_transform(src_lab[0], M, offset=offset, output_shape=crop, order=0, mode="grid-constant", cval=0x80)
    h = s[0] + 0.5
    clear = (np.abs(h - np.round(h)) > 1e-9).all(axis=0)
    assert clear.mean() > 0.99 and np.array_equal(lab[0][clear], want[clear])
    assert (lab[0] == 0x80).any() and (lab[0] != 0x80).any()


# ---- 2. lattice preconditions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ext,crop,C,half", SC.lattice_cases(), ids=[c[0] for c in SC.lattice_cases()])
def test_lattice_cases_are_exact_in_float32(cid, ext, crop, C, half):
    case = SC.lattice_case(ext, crop, C, half)
    assert SC.lattice_violations(case) == []
    y64 = R.ref_resample(case["src"], case["src_lab"], case["inv"], case["gain"], case["bias"], crop)[0]
    assert np.array_equal(R.ref_resample(case["src"], case["src_lab"], case["inv"], case["gain"], case["bias"], crop, reverse=True)[0], y64)
    for reverse, fused in ((False, False), (True, False), (False, True)):
        y32 = SC.resample_steps(case, reverse=reverse, fused=fused)
        assert y32.dtype == np.float32 and np.array_equal(y32.astype(np.float64), y64), (reverse, fused)


def test_lattice_table_is_the_issue_and_holds_the_ties():
    ms = SC.lattice_matrices()
    assert len(ms) == 104 and len({(m.tobytes(), t.tobytes()) for _, m, t in ms}) == 104
    perms = [m for _, m, t in ms if not t.any() and (np.abs(m) == 1).sum() == 3 and (m != 0).sum() == 3]
    assert len(perms) == 48
    assert len(SC.lattice_cases()) == 4 * 3 * 2 and max(c[2] for _, c in SC.LATTICE_EXTENTS) > 64          # a z row longer than a wave
    near, half = set(), False
    for ext, crop in SC.LATTICE_EXTENTS:
        a, b = SC.tie_coordinates(SC.lattice_case(ext, crop, 1, False))
        near |= a
        half |= b
    assert half and -0.5 in near and -0.5625 in near, "the tie rule's edge (-0.5 inside, -0.5625 outside) is in the table"
    # on those coordinates the rule gives what the issue says
    assert int(np.floor(-0.5 + 0.5)) == 0 and int(np.floor(-0.5625 + 0.5)) == -1


def test_generic_case_excludes_few_labels_and_its_bound_is_small():
    case = SC.generic_case()
    assert case["src"].shape == (12, 2, 24, 22, 12)
    y, lab, s = R.ref_resample(case["src"], case["src_lab"], case["inv"], case["gain"], case["bias"], case["crop"])
    clear = SC.away_from_ties(s)
    excluded = 1.0 - clear.reshape(12, -1).mean(axis=1)
    print("[seg aug generic] excluded label share per draw:", " ".join("%.5f" % e for e in excluded))
    assert (excluded <= SC.MAX_EXCLUDED).all()
    bound = SC.generic_bound(case)
    print("[seg aug generic] image bound per (draw, channel): max %.3e" % bound.max())
    assert bound.max() < 1e-2 and bound.min() > 0
    assert (lab == 0x80).any() and ((lab & 0x80) == 0).any()
    bits = SC.label_bits_case()["src_lab"]
    assert int(np.bitwise_or.reduce(bits.reshape(-1))) == 0xFF


# ---- 3. source_extent ------------------------------------------------------------------------------------------------------------------------
def _corners_stay_inside(crop, ext, angles, scale, flips):
    inv = D.inverse_affine(angles, scale, flips, crop, ext)
    lo, hi = R.corner_range(R.coords(inv[None], ext, crop))
    return (lo >= 0).all() and (hi[0] <= np.array(ext) - 1).all()


@pytest.mark.parametrize("crop", [(8, 8, 8), (16, 16, 8), (64, 64, 32)], ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("cfg", [D.AugConfig.defaults(), D.AugConfig.defaults(rotate=45.0, scale=(0.5, 2.0))], ids=["defaults", "extremes"])
def test_source_extent_holds_every_corner(crop, cfg):
    ext = D.source_extent(crop, cfg)
    assert all(e % 2 == 0 and e >= c + 2 for e, c in zip(ext, crop))
    theta = np.deg2rad(cfg.rotate)
    for signs in itertools.product((-theta, 0.0, theta), repeat=3):           # every vertex of the parameter box (and the mid-planes)
        for scale in (cfg.scale[0], 1.0, cfg.scale[1]):
            for flips in ((False, False, False), (True, False, True), (True, True, True)):
                assert _corners_stay_inside(crop, ext, signs, scale, flips), (signs, scale, flips)
    rng = np.random.default_rng(5)
    for _ in range(200):
        angles = rng.uniform(-theta, theta, 3)
        scale = float(np.exp(rng.uniform(np.log(cfg.scale[0]), np.log(cfg.scale[1]))))
        assert _corners_stay_inside(crop, ext, angles, scale, tuple(bool(v) for v in rng.integers(0, 2, 3))), (angles, scale)


def test_source_extent_is_tight_without_geometry_and_for_row_x():
    assert D.source_extent((16, 16, 8), D.AugConfig()) == (18, 18, 10)
    assert D.source_extent((16, 16, 8), D.AugConfig.defaults(p_spatial=0.0)) == (18, 18, 10)
    # row x's bound is attained: one voxel less on that axis loses a corner at the maximising angles
    cfg, crop = D.AugConfig.defaults(), (64, 64, 32)
    ext = D.source_extent(crop, cfg)
    theta = np.deg2rad(cfg.rotate)
    small = (ext[0] - 4,) + ext[1:]
    assert not _corners_stay_inside(crop, small, (0.0, theta, theta), cfg.scale[0], (False,) * 3)


# ---- 4. cut_box ------------------------------------------------------------------------------------------------------------------------------
def _case(shape=(12, 10, 9), C=2, dtype=np.float32, seed=1):
    rng = np.random.default_rng(seed)
    return D.Case("c", rng.standard_normal((C,) + shape).astype(dtype), rng.integers(0, 8, shape).astype(np.uint8))


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_cut_box_equals_cut_in_range_and_pads_both_sides(dtype):
    case = _case(dtype=dtype)
    for start, ext in (((0, 0, 0), (8, 8, 8)), ((4, 2, 1), (8, 8, 8)), ((6, 5, 4), (8, 8, 8)), ((0, 0, 0), (16, 16, 16))):     # the last two run past the high end
        x, lab = D.cut_box(case, start, ext)
        wx, wl = D.cut(case, start, ext)
        assert x.dtype == dtype and np.array_equal(x.astype(np.float32), wx) and np.array_equal(lab, wl), (start, ext)
    # the low side, the high side, and a volume smaller than the extent on every axis
    for start, ext in (((-3, -1, -2), (8, 8, 8)), ((7, 6, 5), (8, 8, 8)), ((-2, -3, -4), (18, 16, 16)), ((-20, 0, 0), (8, 8, 8)), ((0, 30, 0), (4, 4, 4))):
        x, lab = D.cut_box(case, start, ext)
        want_x = np.zeros((2,) + ext, dtype=dtype)
        want_l = np.full(ext, 0x80, dtype=np.uint8)
        for i, j, k in itertools.product(*[range(e) for e in ext]):
            p = (start[0] + i, start[1] + j, start[2] + k)
            if all(0 <= q < n for q, n in zip(p, case.shape)):
                want_x[:, i, j, k] = case.img[:, p[0], p[1], p[2]]
                want_l[i, j, k] = case.seg[p]
        assert x.dtype == dtype and np.array_equal(x, want_x) and np.array_equal(lab, want_l), (start, ext)
    unlabelled = D.Case("u", case.img)
    assert set(np.unique(D.cut_box(unlabelled, (-1, -1, -1), (4, 4, 4))[1]).tolist()) == {0, 0x80}


# ---- 5. the un-augmented loader is the parent revision's --------------------------------------------------------------------------------------
def test_croploader_without_augmentation_reproduces_the_parent(golden_dir):
    fix = np.load(os.path.join(golden_dir, "seg_croploader_default.npz"))
    assert np.array_equal(fix["triples"], np.array(FX.TRIPLES)) and fix["digests"].shape == (len(FX.TRIPLES), FX.STEPS, 32)
    assert np.array_equal(FX.digests(D), fix["digests"])
    # aug=None, a neutral config and no argument at all are one code path
    cases = [D.synthetic_case(1, i, (24, 16, 10), 3, 1) for i in range(3)]
    plain = [tuple(t.numpy().tobytes() for t in b) for b in D.CropLoader(cases, (16, 16, 8), 2, 2, 7, 0)]
    for aug in (None, D.AugConfig(), D.AugConfig.defaults(p_spatial=0.0, p_intensity=0.0)):
        loader = D.CropLoader(cases, (16, 16, 8), 2, 2, 7, 0, aug=aug)
        assert loader.aug is None and [tuple(t.numpy().tobytes() for t in b) for b in loader] == plain


# ---- 6. the augmented draws --------------------------------------------------------------------------------------------------------------------
def _digest(batch):
    h = hashlib.sha256()
    for t in (batch[0], batch[1]) + tuple(batch[2][k] for k in sorted(batch[2])):
        h.update(t.numpy().tobytes())
    return h.hexdigest()


def test_augmented_draws_are_a_function_of_seed_rank_epoch():
    cases = [D.synthetic_case(2, i, D.synthetic_shape((16, 16, 8)), 3, 2) for i in range(4)]
    cfg = D.AugConfig.defaults(p_spatial=1.0, p_intensity=1.0)

    def run(seed, rank, epoch):
        loader = D.CropLoader(cases, (16, 16, 8), 2, 2, seed, rank, aug=cfg)
        loader.set_epoch(epoch)
        return [_digest(b) for b in loader]

    base = run(3, 0, 1)
    assert run(3, 0, 1) == base and len(set(base)) == 2
    assert run(4, 0, 1) != base and run(3, 1, 1) != base and run(3, 0, 2) != base
    loader = D.CropLoader(cases, (16, 16, 8), 2, 1, 3, 0, aug=cfg)
    src, src_lab, p = next(iter(loader))
    ext = D.source_extent((16, 16, 8), cfg)
    assert loader.extent == ext and tuple(src.shape) == (2, 2) + ext and src.dtype == torch.float32 and tuple(src_lab.shape) == (2,) + ext
    assert set(p) == {"inv", "gain", "bias", "gamma", "noise_std", "seed", "crop"}
    assert tuple(p["inv"].shape) == (2, 12) and p["inv"].dtype == torch.float32 and p["seed"].dtype == torch.int64 and p["seed"].dim() == 0
    for k in ("gain", "bias", "gamma", "noise_std"):
        assert tuple(p[k].shape) == (2, 2) and p[k].dtype == torch.float32
    assert bool((p["gain"] >= 0.75).all() and (p["gain"] <= 1.25).all() and (p["bias"].abs() <= 0.1).all() and (p["gamma"] >= 0.7 - 1e-6).all()
                and (p["gamma"] <= 1.5 + 1e-6).all() and (p["noise_std"] >= 0).all() and (p["noise_std"] <= 0.1).all())
    # float16 cases stay float16 up to the device
    half = [D.Case(c.name, c.img.astype(np.float16), c.seg) for c in cases]
    assert next(iter(D.CropLoader(half, (16, 16, 8), 2, 1, 3, 0, aug=cfg)))[0].dtype == torch.float16
    # the drawn parameters stay inside the config, and the neutral draw is neutral
    rng = np.random.default_rng(0)
    seen = set()
    for _ in range(40):
        _, _, inv, rows, info = D.draw_aug_crop(rng, cases[0], (16, 16, 8), False, D.AugConfig.defaults())
        seen.add(info["spatial"])
        assert all(abs(a) <= np.deg2rad(15.0) for a in info["angles"]) and 0.8 - 1e-12 <= info["scale"] <= 1.25 + 1e-12
        if not info["spatial"]:
            assert np.array_equal(np.abs(inv.reshape(3, 4)[:, :3]), np.eye(3)) and not inv.reshape(3, 4)[:, 3].any()
    assert seen == {True, False}


@pytest.mark.parametrize("shape", [(24, 20, 10), (12, 20, 6)], ids=["larger", "shorter than the crop on two axes"])
def test_identity_config_gives_draw_crops_crop(shape):
    case = D.synthetic_case(4, 0, shape, 3, 2)
    crop = (16, 16, 8)
    ident = D.AugConfig(p_spatial=1.0, p_intensity=1.0)
    assert not ident.enabled
    flips_seen = set()
    for seed, centred in itertools.product(range(6), (True, False)):
        x, lab, info = D.draw_crop(np.random.default_rng(seed), case, crop, centred)
        src, src_lab, inv, rows, info2 = D.draw_aug_crop(np.random.default_rng(seed), case, crop, centred, ident)
        assert {k: info2[k] for k in info} == info and src.shape[1:] == (18, 18, 10)
        assert all(np.array_equal(rows[k], np.full(2, v, dtype=np.float32)) for k, v in (("gain", 1), ("bias", 0), ("gamma", 1), ("noise_std", 0)))
        y, got_lab, _ = R.ref_resample(src[None], src_lab[None], inv[None], rows["gain"][None], rows["bias"][None], crop)
        assert np.array_equal(y[0], x.astype(np.float64)) and np.array_equal(got_lab[0], lab), (seed, centred, info)
        flips_seen.add(info["flips"])
    assert len(flips_seen) > 3


def test_training_batch_of_the_gpu_test_has_a_settled_count():
    """test_seg_aug_gpu.py compares the step's counted voxels with the restatement's: no coordinate of that batch sits so close to a tie that the
    kernel's float32 coordinate could count another voxel."""
    batch = SC.train_batch()
    count, settled = SC.counted_voxels(batch)
    assert settled and 0 < count < 2 * 16 * 16 * 8, "part of the batch lies outside its volume, part inside"
    assert bool((batch[2]["noise_std"] != 0).all()) and bool((batch[2]["gamma"] != 1).all())


def test_odd_extent_difference_takes_the_half_voxel():
    """An odd extent - crop difference (an odd crop under the even extents): the box starts at start - (extent - crop) // 2 and t = -0.5 puts the crop
    back on the voxel grid."""
    case = D.synthetic_case(4, 1, (20, 20, 12), 2, 1)
    crop, ext = (7, 8, 5), (10, 10, 8)
    src, src_lab, inv, rows, info = D.draw_aug_crop(np.random.default_rng(1), case, crop, False, D.AugConfig(), extent=ext)
    assert inv.reshape(3, 4)[:, 3].tolist() == [-0.5, 0.0, -0.5]
    y, lab, _ = R.ref_resample(src[None], src_lab[None], inv[None], rows["gain"][None], rows["bias"][None], crop)
    x, want, _ = D.draw_crop(np.random.default_rng(1), case, crop, False)
    assert np.array_equal(y[0], x.astype(np.float64)) and np.array_equal(lab[0], want)


# ---- 7. the command line ----------------------------------------------------------------------------------------------------------------------
BASE = ["train", "--data", "synthetic", "--phase", "scratch"]


def _parse(*extra):
    return seg3d.build_parser().parse_args(BASE + list(extra))


def test_options_make_the_config():
    assert D.parse_aug(_parse()) is None
    assert D.parse_aug(argparse.Namespace()) is None
    assert D.parse_aug(_parse("--augment")) == D.AugConfig.defaults()
    d = D.AugConfig.defaults()
    assert (d.rotate, d.scale, d.p_spatial, d.gain, d.bias, d.gamma, d.noise_std, d.p_intensity) == (15.0, (0.8, 1.25), 0.5, (0.75, 1.25), 0.1, (0.7, 1.5),
                                                                                                     0.1, 0.15)
    assert d.enabled and not D.AugConfig().enabled
    for flag, value, field, want in (("--aug_rotate", "30", "rotate", 30.0), ("--aug_scale", "0.9,1.1", "scale", (0.9, 1.1)),
                                     ("--aug_gain", "0.5,2", "gain", (0.5, 2.0)), ("--aug_bias", "0.25", "bias", 0.25),
                                     ("--aug_gamma", "1,1", "gamma", (1.0, 1.0)), ("--aug_noise", "0", "noise_std", 0.0),
                                     ("--aug_p_spatial", "1", "p_spatial", 1.0), ("--aug_p_intensity", "0", "p_intensity", 0.0)):
        cfg = D.parse_aug(_parse(flag, value))                                       # an override implies --augment and replaces one default
        assert cfg == dataclasses.replace(d, **{field: want}), flag
    seg3d.check_train(_parse("--augment", "--aug_rotate", "0"))


@pytest.mark.parametrize("flag,value", [
    ("--aug_scale", "1.25,0.8"), ("--aug_gain", "1.5,0.5"), ("--aug_gamma", "1.5,0.7"),            # lo > hi
    ("--aug_scale", "0,1"), ("--aug_scale", "-1,1"), ("--aug_scale", "0.8"), ("--aug_scale", "a,b"),      # scale <= 0, malformed
    ("--aug_rotate", "-1"), ("--aug_rotate", "45.5"), ("--aug_rotate", "x"),
    ("--aug_p_spatial", "-0.1"), ("--aug_p_spatial", "1.5"), ("--aug_p_intensity", "-0.1"), ("--aug_p_intensity", "2"), ("--aug_p_intensity", "nan"),
    ("--aug_gamma", "0,1"), ("--aug_bias", "-0.5"), ("--aug_noise", "-1"),
])
def test_bad_option_values_exit_with_their_message(flag, value):
    args = _parse(flag + "=" + value)
    with pytest.raises(SystemExit) as e:
        seg3d.check_train(args)
    assert str(e.value).startswith(f"{flag} {value}: "), str(e.value)
    with pytest.raises(SystemExit, match=flag):
        D.parse_aug(args)
