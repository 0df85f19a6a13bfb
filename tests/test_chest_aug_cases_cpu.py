"""Preconditions of tests/test_chest_augment_edges_gpu.py, checked without a GPU: the constants chest_aug_cases.py restates are the ones in
augment2d.hip; the tables reach the edges they were built for; and the numpy restatement (tests/chest_aug_reference.py), the GPU tests'
expected value, equals PILLOW on every case of the tables -- Pillow stays the ground truth.  One fact about Pillow is recorded, not fixed:
its resize runs the vertical pass first on crops more than 100 times as tall as wide."""
import numpy as np
import pytest

import chest_aug_cases as cc
import chest_aug_reference as R
from pcrlv2_amd import data_chest as DC


def _pil():
    return pytest.importorskip("PIL.Image")


def _arr(im):
    a = np.asarray(im, dtype=np.uint8)
    return a.reshape(a.shape[0], a.shape[1], -1)


def _img(a):
    return _pil().fromarray(a[..., 0] if a.shape[2] == 1 else a)


# ---------------------------------------------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------------------------------------------
def test_the_constants_of_the_source_are_the_ones_the_tables_were_built_for():
    assert cc.source_pins_missing() == []
    assert cc.source_pins_missing([("augment2d.hip", "constexpr int BLUR_RMAX = 5;")]) == [("augment2d.hip", "constexpr int BLUR_RMAX = 5;")]
    assert (cc.BLUR_RMAX, cc.HRESAMPLE_CAP, cc.V_MAX, cc.S_MAX) == (4, 262144, 65535, 4096)
    assert DC.NPARAM == 40 and DC.P_INTER == DC.P_HOLES + 12


def test_the_tall_cases_cross_the_grid_cap():
    """1200 rows, the case as first written down, overshoot the cap by whole blocks (6656 = 26 * 256); 1203 rows were added so that the
    second step of the stride loop also ends in a partial block."""
    over = {rows: rows * cc.TALL_S - cc.HRESAMPLE_CAP for rows in cc.TALL_ROWS}
    assert over == {1200: 6656, 1203: 7328}
    assert over[1200] % cc.HRESAMPLE_THREADS == 0 and over[1203] % cc.HRESAMPLE_THREADS == 160
    assert all(0 < o < cc.HRESAMPLE_CAP for o in over.values())
    for rows in cc.TALL_ROWS:
        imgs, recs = cc.tall_case(rows)
        assert imgs[0].shape == (rows, 16, 1) and tuple(recs[0, [DC.P_CW, DC.P_CH]]) == (16, rows) and recs[1, DC.P_CH] == cc.TALL_OTHER_ROWS
        assert rows <= 100 * cc.TALL_W                                    # Pillow still runs the horizontal pass first
        assert cc.TALL_OTHER_ROWS * cc.TALL_S < cc.HRESAMPLE_CAP // 16    # max_rows = 40: the tall view takes more than 16 steps


def test_the_resampling_boxes_reach_every_size_and_clamp():
    boxes = cc.resample_boxes()
    for S in cc.RESAMPLE_SIDES:
        assert {(b[5], b[6]) for b in boxes if b[7] == S} >= {(w, h) for w in cc.resample_sizes(S) for h in cc.resample_sizes(S)}
        for n in cc.clamp_sizes(S):
            lo, hi, taps = cc.raw_bounds(n, S)
            assert min(lo) < 0 or max(hi) > n, (n, S)
            assert min(taps) >= 1
        assert max(cc.raw_bounds(4 * S + 3, S)[2]) >= 9 and min(cc.raw_bounds(4 * S + 3, S)[0]) < 0 and max(cc.raw_bounds(4 * S + 3, S)[1]) > 4 * S + 3
        assert cc.raw_bounds(1, S)[2] == [1] * S                                                  # one source pixel
        assert all(sorted(t)[-1] == 1 << R.PRECISION_BITS and not any(sorted(t)[:-1]) for t in R.resample_coeffs(S, S)[1])   # the identity: one tap of weight 1
    assert max(cc.raw_bounds(290, 224)[2]) >= 3 and {b[7] for b in boxes} == {8, 17, 96, 224}
    assert all(0 <= j and j + cw <= W and 0 <= i and i + ch <= H and C in (1, 3) for H, W, C, j, i, cw, ch, S in boxes)
    assert any(H > ch and W > cw for H, W, C, j, i, cw, ch, S in boxes if S in cc.RESAMPLE_SIDES)
    corners = [(b[3] == 0, b[4] == 0, b[3] + b[5] == b[1], b[4] + b[6] == b[0]) for b in boxes if (b[0], b[1]) == (40, 50)]
    assert sorted(corners) == sorted([(True, True, False, False), (False, True, True, False), (True, False, False, True), (False, False, True, True)])
    assert {b[2] for b in boxes if b[7] == 8} == {1, 3} and len(boxes) == 78
    # the restated bounds are the reference's
    for n, S in ((9, 8), (71, 17), (1, 8), (290, 224)):
        xmins, taps = R.resample_coeffs(n, S)
        lo, hi, cnt = cc.raw_bounds(n, S)
        assert xmins == [max(v, 0) for v in lo] and [len(t) for t in taps] == cnt


def test_the_blur_radii_and_the_contrast_means():
    assert [DC.blur_params(s)[0] for s in cc.BLUR_SIGMAS] == [0, 1, 2, 3, 4] and cc.BLUR_RMAX == 4
    assert max(DC.blur_params(s)[0] for s in np.linspace(DC.SIGMA[0], DC.SIGMA[1], 400)) == 1        # what production draws
    for s in cc.BLUR_SIGMAS:
        r, ww, fw = DC.blur_params(s)
        assert 0 <= fw < 2 ** 24 and 0 < ww <= 2 ** 24 and (2 * r + 1) * ww + 2 * fw <= 2 ** 24        # 255 * 2^24 + 2^23 fits the kernel's unsigned
    SS = cc.PS * cc.PS
    for C in (1, 3):
        got = []
        for name, a, mean in cc.contrast_images(C):
            l = R.luma(a) if C == 3 else a[..., 0].astype(np.int64)
            tot = int(l.sum())
            assert (2 * tot + SS) // (2 * SS) == mean, (C, name)
            got.append((name, tot - 100 * SS if name.startswith("k") else None, mean))
            if C == 3 and name.startswith("k"):
                assert set(np.unique(l)) == {100, 101} and not (a[..., 0] == a[..., 1]).any()
        assert got[:3] == [(f"k={SS // 2 - 1}", SS // 2 - 1, 100), (f"k={SS // 2}", SS // 2, 101), (f"k={SS // 2 + 1}", SS // 2 + 1, 101)]
        assert [m for _, _, m in got[3:]] == [0, 255]
    assert 2 * (100 * SS + SS // 2) + SS == 2 * SS * 101          # k = SS / 2: the mean lies exactly on the half


def test_the_rotation_cases_have_fill_and_kept_pixels():
    """Every angle that is no identity reads outside somewhere and keeps pixels elsewhere -- except 5 degrees at S = 8, whose corners stay
    inside; the three identity angles keep every pixel."""
    for S in cc.ROT_SIDES:
        cases = cc.rotation_cases(S)
        assert len(cases) == 2 * len(cc.ROT_ANGLES) and {f for _, f, _ in cases} == {0, 1} and {c for _, _, c in cases} == {1, 3}
        for angle, flip, C in cases:
            src = cc.rotation_source(S, C)
            assert src.min() >= 1
            rec = cc.rotation_record(S, angle, flip, C)
            out = R.rotate_nearest(src, rec[DC.P_A0:DC.P_A5 + 1])
            fill = (out == 0).all(axis=2)
            assert fill.any() == cc.rotation_has_fill(angle, S), (S, angle)
            assert not fill.all()
            if angle in cc.ROT_IDENTITY:
                assert tuple(rec[DC.P_A0:DC.P_A5 + 1]) == DC.rotate_fixed(0.0, S, S) and np.array_equal(out, src)
        assert sum(cc.rotation_has_fill(a, S) for a, _, _ in cases) >= 6


def test_the_colour_tables():
    assert np.array_equal(cc.every_colour()[[0, 1, 256, 65536, 2 ** 24 - 1]], [[0, 0, 0], [0, 0, 1], [0, 1, 0], [1, 0, 0], [255, 255, 255]])
    views = cc.colour_views(cc.every_colour())
    assert views.shape == (335, 3, 224, 224) and 335 * 224 * 224 - 2 ** 24 == 31744
    assert tuple(views[1, :, 0, 1]) == (0, 196, 1) and not views[-1].reshape(3, -1)[:, -31744:].any()        # colour 50177 = 0x00c401
    assert np.array_equal(cc.view_colours(views)[:2 ** 24], cc.every_colour())
    rgb, hsv = cc.hsv_preimages()
    n = rgb.shape[0]
    assert 2 ** 22 < n < 2 ** 23 and len(np.unique(hsv.astype(np.uint32) @ np.array([65536, 256, 1], np.uint32))) == n
    h, s, v = R._rgb2hsv(rgb[None])
    assert np.array_equal(np.stack([h[0], s[0], v[0]], -1), hsv)
    assert (hsv[:, 1] == 0).any() and hsv[:, 0].max() == 254 and (hsv[:, 0] == 0).any()          # h < 1, so int(h * 255) <= 254
    assert cc.HUE_SHIFTS == (0, 1, DC.hue_shift(0.4), DC.hue_shift(-0.4), 255)
    f = {k: cc.bits_f32(b) for k, b in cc.BLEND_FACTORS.items()}
    assert f["0.6"] == float(np.float32(0.6)) and f["1.4"] == float(np.float32(1.4)) and f["1"] == 1.0 and f["0"] == 0.0
    assert f["1-"] == float(np.nextafter(np.float32(1), np.float32(0))) and f["1+"] == float(np.nextafter(np.float32(1), np.float32(2)))
    assert 0 < f["denormal"] < float(np.finfo(np.float32).tiny)
    t = cc.normalize_table()
    assert t.shape == (3, 256) and t.dtype == np.float32 and np.array_equal(t[:, 7], R.normalize(np.full((1, 1, 3), 7, np.uint8)).reshape(3))
    assert all(len(np.unique(cc.byte_ramp(C)[..., c])) == 256 for C in (1, 3) for c in range(C))


def test_the_hole_sets_the_jitter_orders_and_the_mixed_launch():
    for S in cc.PHOTOMETRIC_SIDES:
        sets = cc.hole_sets(S)
        assert {len(h) for h in sets} == {0, 1, 2, 3}
        assert all(0 <= y0 < y1 <= S and 0 <= x0 < x1 <= S for h in sets for y0, y1, x0, x1 in h)
        ones = [h[0] for h in sets if len(h) == 1]
        assert {(y0 == 0, x0 == 0, y1 == S, x1 == S) for y0, y1, x0, x1 in ones} >= {(True, True, False, False), (True, False, False, True),
                                                                                      (False, True, True, False), (False, False, True, True), (True,) * 4}
        three = next(h for h in sets if len(h) == 3)
        m = sum(R.cutout(np.ones((1, S, S), np.float32), [h])[0] == 0 for h in three)
        assert m.max() >= 2 and (m == 1).any()                   # the three overlap, and not everywhere
    recs = cc.jitter_records()
    assert len(recs) == 120 and len({ops for ops, _ in recs if len(ops) == 4}) == 24 and {len(ops) for ops, _ in recs} == {0, 1, 2, 3, 4}
    assert all(tuple((int(r[DC.P_ORDER]) >> (4 * k)) & 15 for k in range(int(r[DC.P_NOPS]))) == ops for ops, r in recs)
    imgs, sample, rec, src = cc.layout_case()
    C = rec[:, DC.P_C]
    assert list(C) == [1, 3] * 4 and src.size == cc.LAYOUT_PAD + sum(a.size for a in imgs)
    assert any(o % 2 == 1 for o in rec[C == 1, DC.P_SRC]) and any(o % 2 == 1 for o in rec[C == 3, DC.P_SRC]) and (rec[:, DC.P_SRC] > 0).all()
    for v, n in enumerate(sample):
        o = int(rec[v, DC.P_SRC])
        assert np.array_equal(src[o:o + imgs[n].size], imgs[n].reshape(-1)) and tuple(rec[v, [DC.P_H, DC.P_W, DC.P_C]]) == imgs[n].shape
    sizes = rec[:, DC.P_CH] * cc.PS * C
    assert np.array_equal(rec[:, DC.P_INTER], np.concatenate([[0], np.cumsum(sizes)[:-1]]))          # packed: no gap between the views
    assert (rec[:, DC.P_NHOLES] == 3).all() and (rec[:, DC.P_NOPS] == 4).all() and {0, 1} == set(rec[:, DC.P_BLUR]) == set(rec[:, DC.P_GRAY])


# ---------------------------------------------------------------------------------------------------------------
# the restatement against Pillow on the tables
# ---------------------------------------------------------------------------------------------------------------
def test_resampling_boxes_equal_pillow():
    Image = _pil()
    for n, box in enumerate(cc.resample_boxes()):
        H, W, C, j, i, cw, ch, S = box
        src = cc.box_source(box, n)
        ref = _arr(_img(src).crop((j, i, j + cw, i + ch)).resize((S, S), Image.BILINEAR))
        assert np.array_equal(R.crop_resize(src, i, j, ch, cw, S), ref), box
    for rows in cc.TALL_ROWS:
        for a, r in zip(*cc.tall_case(rows)):
            j, i, cw, ch = (int(r[k]) for k in (DC.P_J, DC.P_I, DC.P_CW, DC.P_CH))
            ref = _arr(_img(a).crop((j, i, j + cw, i + ch)).resize((cc.TALL_S, cc.TALL_S), Image.BILINEAR))
            assert np.array_equal(R.crop_resize(a, i, j, ch, cw, cc.TALL_S), ref), (rows, ch)


def test_pillow_runs_the_vertical_pass_first_beyond_100_to_1():
    """A fact about Pillow (12.2.0), recorded and not fixed: on a crop with ch > 100 cw (and ch > S) Image.resize gives the result of the
    vertical pass followed by the horizontal one; R.resize and the kernels run the horizontal pass first, as Pillow does up to 100 : 1.  The
    two orders round differently.  RandomResizedCrop's ratio is 3/4 .. 4/3 (its fallback is clamped to it), so no drawn crop comes near."""
    Image = _pil()
    for n, (cw, ch, S, same) in enumerate(cc.TALL_BOUNDARY):
        src = cc.source_image(ch, cw, 1, 300 + n)
        pil = _arr(_img(src).resize((S, S), Image.BILINEAR))
        assert np.array_equal(R.resize(src, S), pil) == same, (cw, ch, S)
        if not same:
            assert np.array_equal(R._pass(R._pass(src, S, 0), S, 1), pil), (cw, ch, S)
    rng = np.random.default_rng(41)                       # wide crops never differ
    for cw, ch in ((600, 1), (999, 3), (1281, 10)):
        src = rng.integers(0, 256, (ch, cw, 1), dtype=np.uint8)
        assert np.array_equal(R.resize(src, 17), _arr(_img(src).resize((17, 17), Image.BILINEAR)))
    i, j, h, w = DC.draw_crops(rng, np.tile([90, 600, 257, 4000], 500), np.tile([600, 90, 300, 30], 500), DC.LOCAL_SCALE)
    assert (h <= 2 * w).all()


def test_rotations_equal_pillow():
    Image = _pil()
    for S in cc.ROT_SIDES:
        for angle, flip, C in cc.rotation_cases(S):
            src = cc.rotation_source(S, C)
            rec = cc.rotation_record(S, angle, flip, C)
            im = _img(src).rotate(angle, Image.NEAREST, expand=False, fillcolor=0 if C == 1 else (0, 0, 0))
            got = R.rotate_nearest(src, rec[DC.P_A0:DC.P_A5 + 1])
            if flip:
                im, got = im.transpose(Image.FLIP_LEFT_RIGHT), R.hflip(got)
            assert np.array_equal(got, _arr(im)), (S, angle, flip, C)


def test_blur_radii_0_to_4_equal_pillow():
    _pil()
    from PIL import ImageFilter
    for C in (1, 3):
        for name, a in cc.blur_images(C):
            for sigma in cc.BLUR_SIGMAS:
                ref = _arr(_img(a).filter(ImageFilter.GaussianBlur(radius=sigma)))
                assert np.array_equal(R.box_blur(a, *DC.blur_params(sigma)), ref), (C, name, sigma)
    line = cc.source_image(3, 2, 1, 5)                     # lines shorter than the radius
    for sigma in cc.BLUR_SIGMAS:
        assert np.array_equal(R.box_blur(line, *DC.blur_params(sigma)), _arr(_img(line).filter(ImageFilter.GaussianBlur(radius=sigma)))), sigma


def test_contrast_means_equal_pillow():
    _pil()
    from PIL import ImageEnhance
    for C in (1, 3):
        for name, a, mean in cc.contrast_images(C):
            for f in cc.CONTRAST_FACTORS:
                f = cc.bits_f32(cc.BLEND_FACTORS[f])
                ref = _arr(ImageEnhance.Contrast(_img(a)).enhance(f))
                assert np.array_equal(R.contrast(a, f), ref), (C, name, f)
                assert np.array_equal(ref, R.blend(np.full_like(a, mean), a, f))


def test_every_blend_factor_equals_pillow_on_every_pair():
    Image = _pil()
    from PIL import ImageEnhance
    a, b = np.mgrid[0:256, 0:256].astype(np.uint8)
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16, 1)
    rgb = cc.hsv_preimages()[0][::997][:4096].reshape(64, 64, 3)
    for name, bits in cc.BLEND_FACTORS.items():
        f = cc.bits_f32(bits)
        assert np.float32(f).view(np.int32) == bits
        assert np.array_equal(R.blend(a, b, f), np.asarray(Image.blend(Image.fromarray(a), Image.fromarray(b), f))), name
        assert np.array_equal(R.brightness(ramp, f), _arr(ImageEnhance.Brightness(_img(ramp)).enhance(f))), name
        assert np.array_equal(R.saturation(rgb, f), _arr(ImageEnhance.Color(_img(rgb)).enhance(f))), name
    below = R.brightness(ramp, cc.bits_f32(cc.BLEND_FACTORS["1-"])).reshape(-1)
    assert np.array_equal(below, np.maximum(np.arange(256) - 1, 0))           # v (1 - 2^-24) rounds below v and is truncated
    assert np.array_equal(R.brightness(ramp, cc.bits_f32(cc.BLEND_FACTORS["denormal"])).reshape(-1), np.zeros(256))


def test_hue_shifts_equal_pillow_on_the_distinct_hsv_triples():
    Image = _pil()
    rgb, hsv = cc.hsv_preimages()
    n = rgb.shape[0]
    side = int(np.ceil(np.sqrt(n)))
    img = np.zeros((side * side, 3), np.uint8)
    img[:n] = rgb
    h, s, v = Image.fromarray(img.reshape(side, side, 3)).convert("HSV").split()
    assert np.array_equal(np.stack([np.asarray(h), np.asarray(s), np.asarray(v)], -1).reshape(-1, 3)[:n], hsv)
    for shift in cc.HUE_SHIFTS:
        nh = Image.fromarray((np.asarray(h).astype(np.int64) + shift).astype(np.uint8))
        ref = np.asarray(Image.merge("HSV", (nh, s, v)).convert("RGB")).reshape(-1, 3)[:n]
        got = cc.hue_of_hsv(hsv, shift)
        assert np.array_equal(got, ref), shift
        assert np.array_equal(got[::4099], R.hue(rgb[::4099][None], shift)[0])
    assert (cc.hue_of_hsv(hsv, 0) != rgb).any(axis=1).any()          # shift 0 is no identity: HSV quantises


def test_grayscale_and_saturation_equal_pillow_on_every_colour():
    Image = _pil()
    from PIL import ImageEnhance
    rgb = cc.every_colour()
    im = Image.fromarray(rgb.reshape(4096, 4096, 3))
    assert np.array_equal(cc.on_colours(R.grayscale, rgb)[:, 0], np.asarray(im.convert("L")).reshape(-1))
    for name in cc.FULL_FACTORS:
        f = cc.bits_f32(cc.BLEND_FACTORS[name])
        assert np.array_equal(cc.on_colours(lambda a: R.saturation(a, f), rgb), np.asarray(ImageEnhance.Color(im).enhance(f)).reshape(-1, 3)), name


def test_whole_views_of_the_mixed_launch_equal_pillow():
    """The layout case's drawn records through Pillow operation by operation, as tools/make_chest_fixtures.py does for the fixtures."""
    Image = _pil()
    from PIL import ImageEnhance, ImageFilter
    imgs, sample, rec, _ = cc.layout_case()
    S = cc.PS
    for v, n in enumerate(sample):
        r = rec[v]
        _, _, sp, ph = R.view(imgs[n], r, S)
        j, i, cw, ch = (int(r[k]) for k in (DC.P_J, DC.P_I, DC.P_CW, DC.P_CH))
        assert np.array_equal(R.crop_resize(imgs[n], i, j, ch, cw, S), _arr(_img(imgs[n]).crop((j, i, j + cw, i + ch)).resize((S, S), Image.BILINEAR)))
        im = _img(sp)
        if r[DC.P_GRAY] and imgs[n].shape[2] == 3:
            im = Image.merge("RGB", [im.convert("L")] * 3)
        if r[DC.P_BLUR]:
            # the record holds (r, ww, fw), not the sigma Pillow would need: the restated blur, held to Pillow by the test above
            im = _img(R.box_blur(_arr(im), int(r[DC.P_BR]), int(r[DC.P_WW]), int(r[DC.P_FW])))
        fac = np.array(r[DC.P_BRI:DC.P_SAT + 1], np.int32).view(np.float32)
        for k in range(int(r[DC.P_NOPS])):
            op = (int(r[DC.P_ORDER]) >> (4 * k)) & 15
            if op == 0:
                im = ImageEnhance.Brightness(im).enhance(float(fac[0]))
            elif op == 1:
                im = ImageEnhance.Contrast(im).enhance(float(fac[1]))
            elif op == 2:
                im = ImageEnhance.Color(im).enhance(float(fac[2]))
            elif im.mode == "RGB":
                h, s, val = im.convert("HSV").split()
                nh = Image.fromarray((np.asarray(h).astype(np.int64) + int(r[DC.P_HUE])).astype(np.uint8))
                im = Image.merge("HSV", (nh, s, val)).convert("RGB")
        assert np.array_equal(_arr(im), ph), v
