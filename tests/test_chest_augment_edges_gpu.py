"""csrc/augment2d.hip (pcrl_aug2d_hresample, pcrl_aug2d_spatial, pcrl_aug2d_photometric) on every colour and at its edges, through the raw
entry points, bit for bit against tests/chest_aug_reference.py -- which test_chest_aug_cases_cpu.py holds to Pillow on these same cases
(tests/chest_aug_cases.py).  uint8 outputs are compared as bytes, float32 outputs through their int32 bit patterns; there is no tolerance in
this file.  Every output lies in a canary-filled buffer with guard bands on both sides; the source and the intermediate do too, so a tap
outside its box reads canary bytes and moves the result.

Trusted, not checked, by the kernels: the record fields the host draws.  P_BR <= BLUR_RMAX = 4 (box_line's history has five slots) and
P_NHOLES <= 3 (the record has room for three boxes) are preconditions of pcrlv2_amd/data_chest.py, as are P_C in {1, 3}, a crop inside its
source and offsets inside their buffers.  The entry points reject only what they can see: null pointers and the launch shape."""
import re
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import chest_aug_cases as cc  # noqa: E402
import chest_aug_reference as R  # noqa: E402
from pcrlv2_amd import data_chest as DC  # noqa: E402
from pcrlv2_amd._lib import PcrlError, lib, stream_handle  # noqa: E402

DEV = "cuda"
GUARD = 4096
CANARY_U8 = 0xA5
CANARY_F32 = -768.0        # Normalize's range is [-2.2, 2.7]
JUNK = 0x5A                # planes 1 and 2 of a one-plane INPUT view: never read


def call(name, *args):
    return lib().call(name, *args, stream_handle())


def guarded(n, dt=torch.uint8):
    """-> (a canary-filled buffer, its view of n elements GUARD elements from either end)"""
    full = torch.full((n + 2 * GUARD,), CANARY_U8 if dt == torch.uint8 else CANARY_F32, dtype=dt, device=DEV)
    return full, full[GUARD:GUARD + n]


def intact(full, what, untouched=False):
    torch.cuda.synchronize()
    canary = CANARY_U8 if full.dtype == torch.uint8 else CANARY_F32
    n = full.numel() - 2 * GUARD
    assert bool((full[:GUARD] == canary).all()) and bool((full[GUARD + n:] == canary).all()), f"{what}: the canaries around the buffer were overwritten"
    if untouched:
        assert bool((full == canary).all()), f"{what}: a rejected call wrote to its output"


def same(got, want, what):
    """numpy arrays equal element by element: bytes as bytes, float32 as bit patterns"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float32:
        got, want = got.view(np.int32), want.view(np.int32)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    if bad.size:
        first = [(int(i), int(got.reshape(-1)[i]), int(want.reshape(-1)[i])) for i in bad[:6]]
        raise AssertionError(f"{what}: {bad.size} of {got.size} elements differ; (flat index, got, want): {first}")


def planes(img):
    """uint8 [S, S, C] -> [C, S, S]"""
    return np.ascontiguousarray(np.moveaxis(img, 2, 0))


def device_records(recs):
    return torch.from_numpy(np.asarray(recs, np.int64).astype(np.int32)).to(DEV).contiguous()


@pytest.fixture(scope="module")
def table():
    """R.normalize of every byte in every plane, float32 [3, 256] on the device"""
    return torch.from_numpy(cc.normalize_table()).to(DEV)


def out_is_normalize_of(out, u8, C, table, what):
    """On the device: out [V, 3, S, S] equals table[c][u8[:, c]] (u8[:, 0] for a one-plane view) as bits.  Together with a launch that puts
    every byte into every plane this pins normalize() for each (u, c)."""
    for c in range(3):
        want = table[c][u8[:, c if C == 3 else 0].long()]
        assert torch.equal(out[:, c].view(torch.int32), want.view(torch.int32)), f"{what}: plane {c} of `out` is not Normalize(ToTensor(u8_out))"


def run_spatial(imgs, recs, S, max_rows=None, target=True, src=None):
    """hresample + spatial over V views.  imgs[v] is view v's source (packed here one after the other) unless `src`, the packed bytes, is
    given and the records carry their offsets already.  -> (view uint8 [V, 3, S, S], target float32 or None, intermediate bytes) as numpy;
    planes 1 and 2 of a one-plane view hold CANARY_U8."""
    recs = np.array(recs, np.int64).reshape(-1, DC.NPARAM)
    V = recs.shape[0]
    if src is None:
        for v, a in enumerate(imgs):
            recs[v, DC.P_H], recs[v, DC.P_W], recs[v, DC.P_C] = a.shape
        sizes = np.array([a.size for a in imgs])
        DC.pack_offsets(recs, np.concatenate([[0], np.cumsum(sizes)[:-1]]), np.arange(V), S)
        src = np.concatenate([a.reshape(-1) for a in imgs])
    total = int((recs[:, DC.P_CH] * S * recs[:, DC.P_C]).sum())
    src_full, src_d = guarded(src.size)
    src_d.copy_(torch.from_numpy(np.ascontiguousarray(src)))
    rec_d = device_records(recs)
    inter_full, inter = guarded(total)
    view_full, view = guarded(V * 3 * S * S)
    tgt_full, tgt = guarded(V * 3 * S * S, torch.float32) if target else (None, None)
    call("pcrl_aug2d_hresample", src_d, rec_d, inter, V, S, int(recs[:, DC.P_CH].max()) if max_rows is None else max_rows)
    call("pcrl_aug2d_spatial", inter, rec_d, view, tgt, V, S)
    for full, what in ((inter_full, "intermediate"), (view_full, "view"), (tgt_full, "target")):
        if full is not None:
            intact(full, what)
    assert bool((inter != CANARY_U8).any())
    cpu = lambda t, shape: None if t is None else t.cpu().numpy().reshape(shape)
    return cpu(view, (V, 3, S, S)), cpu(tgt, (V, 3, S, S)), cpu(inter, (-1,))


def check_spatial(view, tgt, v, want, what):
    """view v against the expected uint8 [S, S, C] image: its C planes, the canary in the others, the target Normalize(ToTensor(want))."""
    C = want.shape[2]
    same(view[v, :C], planes(want), f"{what}: view")
    assert (view[v, C:] == CANARY_U8).all(), f"{what}: a plane of `view` that a {C}-plane source does not own was written"
    if tgt is not None:
        same(tgt[v], R.normalize(want), f"{what}: target")


def run_photometric(view, recs, S):
    """pcrl_aug2d_photometric on a device view uint8 [V, 3, S, S] -> (out float32 [V, 3, S, S], u8_out uint8 [V, 3, S, S]) device views of
    guarded buffers, canaries checked."""
    recs = np.array(recs, np.int64).reshape(-1, DC.NPARAM)
    V = recs.shape[0]
    assert view.shape == (V, 3, S, S) and view.is_contiguous()
    out_full, out = guarded(V * 3 * S * S, torch.float32)
    u8_full, u8 = guarded(V * 3 * S * S)
    call("pcrl_aug2d_photometric", view, device_records(recs), out, u8, V, S)
    intact(out_full, "out")
    intact(u8_full, "u8_out")
    return out.view(V, 3, S, S), u8.view(V, 3, S, S)


def as_views(imgs, S):
    """[uint8 [S, S, C]] -> device uint8 [V, 3, S, S]; the planes a one-plane view does not own hold JUNK"""
    v = np.full((len(imgs), 3, S, S), JUNK, np.uint8)
    for k, a in enumerate(imgs):
        v[k, :a.shape[2]] = planes(a)
    return torch.from_numpy(v).to(DEV)


def check_photometric(out, u8, wants, what, holes=None):
    """Each view against its expected uint8 [S, S, C] image: the C planes of u8_out, the canary in the others, out = cutout(normalize(want))."""
    out, u8 = out.cpu().numpy(), u8.cpu().numpy()
    for v, want in enumerate(wants):
        C = want.shape[2]
        same(u8[v, :C], planes(want), f"{what} [{v}]: u8_out")
        assert (u8[v, C:] == CANARY_U8).all(), f"{what} [{v}]: a plane of `u8_out` that a {C}-plane view does not own was written"
        t = R.normalize(want)
        same(out[v], R.cutout(t, holes[v]) if holes is not None and holes[v] else t, f"{what} [{v}]: out")


# ---------------------------------------------------------------------------------------------------------------
# 1. Every colour
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def colours():
    """the every-colour image as 335 views of side 224 on the device"""
    return torch.from_numpy(cc.colour_views(cc.every_colour())).to(DEV)


@pytest.fixture(scope="module")
def triples():
    """(pre-image views on the device, uint8 [n, 3] RGB, uint8 [n, 3] HSV, n padded to whole views): one colour per distinct HSV triple"""
    rgb, hsv = cc.hsv_preimages()
    n = rgb.shape[0]
    assert n == len(np.unique(hsv.astype(np.uint32) @ np.array([65536, 256, 1], np.uint32)))      # the count the table gives
    views = cc.colour_views(rgb)
    assert views.shape[0] == -(-n // cc.COLOUR_SIDE ** 2)
    pad = views.shape[0] * cc.COLOUR_SIDE ** 2 - rgb.shape[0]
    z = np.zeros((pad, 3), np.uint8)
    return torch.from_numpy(views).to(DEV), np.concatenate([rgb, z]), np.concatenate([hsv, z])


def colour_launch(views, table, what, **fields):
    S = cc.COLOUR_SIDE
    V = views.shape[0]
    out, u8 = run_photometric(views, np.stack([cc.identity_record(S, c=3, **fields)] * V), S)
    out_is_normalize_of(out, u8, 3, table, what)
    return cc.view_colours(u8.cpu().numpy())


def test_hue_at_shift_0_on_every_colour(colours, table):
    """rgb2hsv -> hsv2rgb of all 2^24 colours (shift 0 is no identity: HSV quantises), 335 views in one launch.  The longest test of the file:
    1.6 s of wall time on an MI355X host -- 0.3 s for the launch, the table check on the device and the copy back, 1.3 s for the numpy reference
    (the HSV decomposition of every colour, which the module then shares, and hsv2rgb) -- after 0.3 s to build and upload the image.  The table
    of distinct triples costs its first user a few seconds more (a sort of 2^24 keys); a CPU without that host's speed takes 6 s for the reference."""
    t0 = time.perf_counter()
    got = colour_launch(colours, table, "hue 0", nops=1, order=3, hue=0)
    t1 = time.perf_counter()
    want = cc.hue_of_hsv(np.stack(cc.every_colour_hsv(), -1), 0)
    print(f"  every-colour hue: kernel and copies {t1 - t0:.2f} s, reference {time.perf_counter() - t1:.2f} s")
    assert colours.shape[0] == 335 and not got[2 ** 24:].any()
    same(got[:2 ** 24], want, "hue 0 on every colour")
    assert (want != cc.every_colour()).any()


@pytest.mark.parametrize("shift", cc.HUE_SHIFTS[1:])
def test_hue_shifts_on_every_distinct_hsv_triple(triples, table, shift):
    views, rgb, hsv = triples
    got = colour_launch(views, table, f"hue {shift}", nops=1, order=3, hue=shift)
    same(got, cc.hue_of_hsv(hsv, shift), f"hue {shift} on the distinct HSV triples")


@pytest.mark.parametrize("name", cc.FULL_FACTORS)
def test_saturation_on_every_colour(colours, table, name):
    f = cc.bits_f32(cc.BLEND_FACTORS[name])
    got = colour_launch(colours, table, f"saturation {name}", nops=1, order=2, sat=cc.BLEND_FACTORS[name])
    same(got[:2 ** 24], cc.on_colours(lambda a: R.saturation(a, f), cc.every_colour()), f"saturation {name} on every colour")
    assert not got[2 ** 24:].any()


@pytest.mark.parametrize("name", [k for k in cc.BLEND_FACTORS if k not in cc.FULL_FACTORS])
def test_saturation_at_the_edge_factors(triples, table, name):
    views, rgb, _ = triples
    f = cc.bits_f32(cc.BLEND_FACTORS[name])
    got = colour_launch(views, table, f"saturation {name}", nops=1, order=2, sat=cc.BLEND_FACTORS[name])
    same(got, cc.on_colours(lambda a: R.saturation(a, f), rgb), f"saturation {name} on the pre-image table")


def test_grayscale_on_every_colour(colours, table):
    got = colour_launch(colours, table, "grayscale", gray=1)
    same(got[:2 ** 24], cc.on_colours(R.grayscale, cc.every_colour()), "luma on every colour")


def test_brightness_at_every_factor_on_every_byte(table):
    """Seven factors x (one plane, three planes) in one launch; `out` against the table pins normalize() for every (u, c): the factor-1
    views put every byte into every plane."""
    S = cc.PS
    imgs, recs, wants = [], [], []
    for name, bits in cc.BLEND_FACTORS.items():
        for C in (1, 3):
            a = cc.byte_ramp(C)
            imgs.append(a)
            recs.append(cc.identity_record(S, c=C, nops=1, order=0, bri=bits))
            wants.append(R.brightness(a, cc.bits_f32(bits)))
    out, u8 = run_photometric(as_views(imgs, S), recs, S)
    check_photometric(out, u8, wants, "brightness")
    k = list(cc.BLEND_FACTORS).index("1") * 2 + 1
    assert all(len(torch.unique(u8[k, c])) == 256 for c in range(3))
    out_is_normalize_of(out[k:k + 1], u8[k:k + 1], 3, table, "brightness 1")
    same(out[k].cpu().numpy(), cc.normalize_table()[np.arange(3)[:, None, None], u8[k].cpu().numpy()], "normalize of every (u, c)")


# ---------------------------------------------------------------------------------------------------------------
# 2. The resampler, the rotation and the flip
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", (8, 17, 96, 224))
def test_resampling_boxes(S):
    """Every box of the table with this side in one launch (gray and RGB sources packed one after the other), identity rotation."""
    boxes = [(n, b) for n, b in enumerate(cc.resample_boxes()) if b[7] == S]
    imgs = [cc.box_source(b, n) for n, b in boxes]
    view, tgt, _ = run_spatial(imgs, [cc.box_record(b) for _, b in boxes], S)
    for v, (n, (H, W, C, j, i, cw, ch, _)) in enumerate(boxes):
        check_spatial(view, tgt, v, R.crop_resize(imgs[v], i, j, ch, cw, S), f"box {(H, W, C, j, i, cw, ch, S)}")


@pytest.mark.parametrize("rows", cc.TALL_ROWS)
def test_tall_crop_enters_the_grid_stride_loop(rows):
    """ch * S > 1024 * 256: the capped grid covers the crop in two steps with max_rows = ch, and in 30 with max_rows = 40 (the other view's
    height); the bytes must not depend on it."""
    imgs, recs = cc.tall_case(rows)
    S = cc.TALL_S
    view, tgt, inter = run_spatial(imgs, recs, S, max_rows=rows)
    view40, tgt40, inter40 = run_spatial(imgs, recs, S, max_rows=cc.TALL_OTHER_ROWS)
    for v, (a, r) in enumerate(zip(imgs, recs)):
        j, i, cw, ch = (int(r[k]) for k in (DC.P_J, DC.P_I, DC.P_CW, DC.P_CH))
        want_inter = R._pass(a[i:i + ch, j:j + cw], S, 1)
        off = int(sum(int(q[DC.P_CH]) * S for q in recs[:v]))
        same(inter[off:off + ch * S], want_inter.reshape(-1), f"tall {rows} view {v}: horizontal pass")
        check_spatial(view, tgt, v, R.crop_resize(a, i, j, ch, cw, S), f"tall {rows} view {v}")
    same(inter40, inter, "max_rows = 40: intermediate")
    same(view40, view, "max_rows = 40: view")
    same(tgt40, tgt, "max_rows = 40: target")


@pytest.mark.parametrize("S", cc.ROT_SIDES)
def test_rotation_and_flip_at_their_ends(S):
    cases = cc.rotation_cases(S)
    imgs = [cc.rotation_source(S, C) for _, _, C in cases]
    view, tgt, _ = run_spatial(imgs, [cc.rotation_record(S, a, f, C) for a, f, C in cases], S)
    zero = cc.normalize_table()[:, 0]
    for v, (angle, flip, C) in enumerate(cases):
        want = R.rotate_nearest(imgs[v], DC.rotate_fixed(angle, S, S))
        want = R.hflip(want) if flip else want
        check_spatial(view, tgt, v, want, f"S {S} angle {angle} flip {flip} C {C}")
        fill = (want == 0).all(axis=2)
        assert fill.any() == cc.rotation_has_fill(angle, S)
        assert (view[v, :C][:, fill] == 0).all()
        for c in range(3):
            assert (tgt[v, c][fill].view(np.int32) == zero[c].view(np.int32)).all()
    view_only, none, _ = run_spatial(imgs, [cc.rotation_record(S, a, f, C) for a, f, C in cases], S, target=False)     # a null target is accepted
    assert none is None
    same(view_only, view, "view without a target")


# ---------------------------------------------------------------------------------------------------------------
# 3. The photometric chain
# ---------------------------------------------------------------------------------------------------------------
def test_blur_at_radii_0_to_4():
    S = cc.PS
    imgs, recs, wants, names = [], [], [], []
    for C in (1, 3):
        for name, a in cc.blur_images(C):
            for sigma in cc.BLUR_SIGMAS:
                r, ww, fw = DC.blur_params(sigma)
                imgs.append(a)
                recs.append(cc.identity_record(S, c=C, blur=1, br=r, ww=ww, fw=fw))
                wants.append(R.box_blur(a, r, ww, fw))
                names.append((C, name, r))
    assert {r for _, _, r in names} == set(range(cc.BLUR_RMAX + 1))
    out, u8 = run_photometric(as_views(imgs, S), recs, S)
    check_photometric(out, u8, wants, f"blur {names}")
    assert any((w != a).any() for w, a, (_, name, r) in zip(wants, imgs, names) if r == 0)          # radius 0 still has its two far taps


def test_contrast_where_the_mean_rounds():
    S = cc.PS
    imgs, recs, wants = [], [], []
    for C in (1, 3):
        for name, a, mean in cc.contrast_images(C):
            for f in cc.CONTRAST_FACTORS:
                imgs.append(a)
                recs.append(cc.identity_record(S, c=C, nops=1, order=1, con=cc.BLEND_FACTORS[f]))
                wants.append(R.blend(np.full_like(a, mean), a, cc.bits_f32(cc.BLEND_FACTORS[f])))
                assert np.array_equal(wants[-1], R.contrast(a, cc.bits_f32(cc.BLEND_FACTORS[f])))
    out, u8 = run_photometric(as_views(imgs, S), recs, S)
    check_photometric(out, u8, wants, "contrast")


def test_every_jitter_order_and_length():
    S = cc.PS
    a = cc.source_image(S, S, 3, 61)
    recs = cc.jitter_records()
    wants = [R.jitter(a, ops, cc.JITTER_FACTORS, cc.JITTER_HUE) for ops, _ in recs]
    assert len({w.tobytes() for w in wants}) > 60
    out, u8 = run_photometric(as_views([a] * len(recs), S), [r for _, r in recs], S)
    check_photometric(out, u8, wants, "jitter orders")


@pytest.mark.parametrize("S", cc.PHOTOMETRIC_SIDES)
def test_cutout_hole_sets(S):
    """0 to 3 holes, clipped at every corner, overlapping, covering the view: a masked element is +0.0 or -0.0 as its sign was (bits)."""
    sets = cc.hole_sets(S)
    imgs = [cc.source_image(S, S, 1 if k % 2 else 3, 70 + k) for k in range(len(sets))]
    recs = [cc.holes_record(S, h, c=a.shape[2]) for h, a in zip(sets, imgs)]
    out, u8 = run_photometric(as_views(imgs, S), recs, S)
    check_photometric(out, u8, imgs, f"cutout {S}", holes=sets)
    o = out.cpu().numpy()
    assert (o[-1] == 0).all() and np.signbit(o[-1]).any() and not np.signbit(o[-1]).all()


def test_gray_and_rgb_views_interleaved_in_one_launch():
    """Four sources behind one pad byte (odd offsets for a gray and an RGB one), eight drawn views, gray and RGB alternating: the whole
    chain against R.view, planes 1 and 2 of `view` and `u8_out` left alone for the gray views, a null target accepted."""
    S = cc.PS
    imgs, sample, rec, src = cc.layout_case()
    view, tgt, _ = run_spatial(None, rec, S, src=src)
    wants = [R.view(imgs[n], rec[v], S) for v, n in enumerate(sample)]
    for v, (_, target, sp, _) in enumerate(wants):
        check_spatial(view, tgt, v, sp, f"layout view {v}")
        same(tgt[v], target, f"layout view {v}: target")
    view_only, none, _ = run_spatial(None, rec, S, src=src, target=False)
    assert none is None
    same(view_only, view, "layout: view without a target")
    feed = torch.from_numpy(view).to(DEV)                 # the spatial kernel's own output: the planes a gray view does not own hold the canary
    out, u8 = run_photometric(feed, rec, S)
    holes = [[tuple(int(x) for x in rec[v, DC.P_HOLES + 4 * k:DC.P_HOLES + 4 * k + 4]) for k in range(3)] for v in range(len(sample))]
    check_photometric(out, u8, [w[3] for w in wants], "layout", holes=holes)
    for v, (o, _, _, _) in enumerate(wants):
        same(out[v].cpu().numpy(), o, f"layout view {v}: out")
    V = len(sample)                                        # u8_out is optional
    out_full, out2 = guarded(V * 3 * S * S, torch.float32)
    call("pcrl_aug2d_photometric", feed, device_records(rec), out2, None, V, S)
    intact(out_full, "out without u8_out")
    assert torch.equal(out2.view(torch.int32), out.reshape(-1).view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------
# 4. Rejections
# ---------------------------------------------------------------------------------------------------------------
def test_every_rejection_of_the_three_entry_points():
    S, V = 96, 2
    a = cc.source_image(100, 100, 1, 3)
    recs = np.stack([cc.identity_record(S, h=100, w=100, c=1, cw=100, ch=100)] * V)
    DC.pack_offsets(recs, [0], np.zeros(V, np.int64), S)
    rec = device_records(recs)
    src = torch.from_numpy(a.reshape(-1)).to(DEV)
    inter_full, inter = guarded(V * 100 * S)
    view_full, view = guarded(V * 3 * S * S)
    tgt_full, tgt = guarded(V * 3 * S * S, torch.float32)
    out_full, out = guarded(V * 3 * S * S, torch.float32)
    u8_full, u8 = guarded(V * 3 * S * S)
    vin = torch.zeros(V * 3 * S * S, dtype=torch.uint8, device=DEV)
    bad = [
        ("pcrl_aug2d_hresample", (None, rec, inter, V, S, 100), "aug2d_hresample: null pointer"),
        ("pcrl_aug2d_hresample", (src, None, inter, V, S, 100), "aug2d_hresample: null pointer"),
        ("pcrl_aug2d_hresample", (src, rec, None, V, S, 100), "aug2d_hresample: null pointer"),
        ("pcrl_aug2d_hresample", (src, rec, inter, 0, S, 100), "aug2d_hresample: bad shape"),
        ("pcrl_aug2d_hresample", (src, rec, inter, -1, S, 100), "aug2d_hresample: bad shape"),
        ("pcrl_aug2d_hresample", (src, rec, inter, cc.V_MAX + 1, S, 100), "aug2d_hresample: bad shape"),
        ("pcrl_aug2d_hresample", (src, rec, inter, V, 0, 100), "aug2d_hresample: bad shape"),
        ("pcrl_aug2d_hresample", (src, rec, inter, V, -S, 100), "aug2d_hresample: bad shape"),
        ("pcrl_aug2d_hresample", (src, rec, inter, V, S, 0), "aug2d_hresample: bad shape"),
        ("pcrl_aug2d_hresample", (src, rec, inter, V, S, -100), "aug2d_hresample: bad shape"),
        ("pcrl_aug2d_spatial", (None, rec, view, tgt, V, S), "aug2d_spatial: null pointer"),
        ("pcrl_aug2d_spatial", (inter, None, view, tgt, V, S), "aug2d_spatial: null pointer"),
        ("pcrl_aug2d_spatial", (inter, rec, None, tgt, V, S), "aug2d_spatial: null pointer"),
        ("pcrl_aug2d_spatial", (inter, rec, view, tgt, 0, S), "aug2d_spatial: bad shape"),
        ("pcrl_aug2d_spatial", (inter, rec, view, tgt, -1, S), "aug2d_spatial: bad shape"),
        ("pcrl_aug2d_spatial", (inter, rec, view, tgt, cc.V_MAX + 1, S), "aug2d_spatial: bad shape"),
        ("pcrl_aug2d_spatial", (inter, rec, view, tgt, V, 0), "aug2d_spatial: bad shape"),
        ("pcrl_aug2d_spatial", (inter, rec, view, tgt, V, -S), "aug2d_spatial: bad shape"),
        ("pcrl_aug2d_spatial", (inter, rec, view, tgt, V, cc.S_MAX + 1), "aug2d_spatial: bad shape"),
        ("pcrl_aug2d_photometric", (None, rec, out, u8, V, S), "aug2d_photometric: null pointer"),
        ("pcrl_aug2d_photometric", (vin, None, out, u8, V, S), "aug2d_photometric: null pointer"),
        ("pcrl_aug2d_photometric", (vin, rec, None, u8, V, S), "aug2d_photometric: null pointer"),
        ("pcrl_aug2d_photometric", (vin, rec, out, u8, 0, S), "aug2d_photometric: bad shape"),
        ("pcrl_aug2d_photometric", (vin, rec, out, u8, -1, S), "aug2d_photometric: bad shape"),
    ] + [("pcrl_aug2d_photometric", (vin, rec, out, u8, V, side), f"aug2d_photometric: view side {side} (224 and 96 are built)")
         for side in (0, -96, 8, 95, 97, 223, 225, 448)]
    for name, args, message in bad:
        with pytest.raises(PcrlError, match=re.escape(message)):
            call(name, *args)
    for full, what in ((inter_full, "intermediate"), (view_full, "view"), (tgt_full, "target"), (out_full, "out"), (u8_full, "u8_out")):
        intact(full, what, untouched=True)
    # the same buffers, the limits themselves: accepted
    call("pcrl_aug2d_hresample", src, rec, inter, V, S, 1)
    call("pcrl_aug2d_spatial", inter, rec, view, None, V, S)
    call("pcrl_aug2d_photometric", view, rec, out, None, V, S)
    for full, what in ((inter_full, "intermediate"), (view_full, "view"), (out_full, "out")):
        intact(full, what)
    same(view.view(V, 3, S, S)[:, 0].cpu().numpy(), np.stack([planes(R.resize(a, S))[0]] * V), "after the rejections: view")
