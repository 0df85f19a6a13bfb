"""CPU side of the 2D (chest) pre-task loader (pcrlv2_amd/data_chest.py): the numpy restatement (tests/chest_aug_reference.py) against Pillow
itself, the committed Pillow fixtures, torchvision's draw rules, the file list, the decode workers and the CLI."""
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import chest_aug_reference as R  # noqa: E402
from pcrlv2_amd import data_chest as DC  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def _pil():
    return pytest.importorskip("PIL.Image")


def _arr(im):
    a = np.asarray(im, dtype=np.uint8)
    return a.reshape(a.shape[0], a.shape[1], -1)


def _image(rng, h, w):
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([(x * 255) // w, (y * 255) // h, ((x + y) * 7) % 256], -1)
    a[h // 3:h // 2, w // 4:w // 2] = (200, 30, 90)
    return (a + rng.integers(0, 40, a.shape)).clip(0, 255).astype(np.uint8)


def test_restatement_equals_pillow_for_every_operation():
    Image = _pil()
    from PIL import ImageEnhance, ImageFilter
    rng = np.random.default_rng(3)
    src = _image(rng, 157, 183)
    im = Image.fromarray(src)
    for _ in range(12):
        S = int(rng.choice([224, 96]))
        h, w = int(rng.integers(3, 157)), int(rng.integers(3, 183))
        i, j = int(rng.integers(0, 157 - h + 1)), int(rng.integers(0, 183 - w + 1))
        assert np.array_equal(R.crop_resize(src, i, j, h, w, S), _arr(im.crop((j, i, j + w, i + h)).resize((S, S), Image.BILINEAR)))
    v = R.resize(src, 96)
    vim = Image.fromarray(v)
    for angle in list(rng.uniform(-10, 10, 8)) + [0.0, -0.0, 1e-3, -9.99]:
        ref = _arr(vim.rotate(float(angle), Image.NEAREST, expand=False, fillcolor=(0, 0, 0)))
        assert np.array_equal(R.rotate_nearest(v, DC.rotate_fixed(float(angle), 96, 96)), ref), angle
    assert np.array_equal(R.hflip(v), _arr(vim.transpose(Image.FLIP_LEFT_RIGHT)))
    assert np.array_equal(R.grayscale(v), _arr(Image.merge("RGB", [vim.convert("L")] * 3)))
    for sigma in list(rng.uniform(0.1, 2.0, 6)) + [0.1, 2.0]:
        assert np.array_equal(R.box_blur(v, *DC.blur_params(float(sigma))), _arr(vim.filter(ImageFilter.GaussianBlur(radius=float(sigma))))), sigma
    for f in list(rng.uniform(0.6, 1.4, 6)) + [1.0, 0.6, 1.37]:
        f = float(f)
        assert np.array_equal(R.brightness(v, f), _arr(ImageEnhance.Brightness(vim).enhance(f)))
        assert np.array_equal(R.contrast(v, f), _arr(ImageEnhance.Contrast(vim).enhance(f)))
        assert np.array_equal(R.saturation(v, f), _arr(ImageEnhance.Color(vim).enhance(f)))
    from make_chest_fixtures import pil_jitter_op
    for hue in list(rng.uniform(-0.4, 0.4, 6)) + [-0.4, 0.4, 0.0, -0.001]:
        assert np.array_equal(R.hue(v, DC.hue_shift(float(hue))), _arr(pil_jitter_op(vim, 3, None, float(hue)))), hue


def test_pillow_facts_the_kernels_rely_on():
    Image = _pil()
    from PIL import ImageEnhance, ImageFilter
    a = np.array([[10, 255]], np.uint8)
    assert _arr(ImageEnhance.Brightness(Image.fromarray(a)).enhance(1.37))[0, 0, 0] == 13          # blend truncates
    assert _arr(ImageEnhance.Brightness(Image.fromarray(a)).enhance(0.63))[0, 1, 0] == 160
    imp = np.zeros((1, 21), np.uint8)
    imp[0, 10] = 255
    line = _arr(Image.fromarray(imp).filter(ImageFilter.GaussianBlur(radius=0.5)))[0, 8:13, 0]
    assert list(line) == [1, 27, 199, 27, 1]          # an extended BOX blur, not a true Gaussian
    assert list(R.box_blur(imp[..., None], *DC.blur_params(0.5))[0, 8:13, 0]) == [1, 27, 199, 27, 1]


def test_hsv_conversions_equal_pillow_on_every_colour():
    Image = _pil()
    c = np.arange(2 ** 24, dtype=np.uint32)
    img = np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    hsv = _arr(Image.fromarray(img).convert("HSV"))
    h, s, v = R._rgb2hsv(img)
    assert np.array_equal(hsv[..., 0], h) and np.array_equal(hsv[..., 1], s) and np.array_equal(hsv[..., 2], v)
    back = _arr(Image.fromarray(img, "HSV").convert("RGB"))
    assert np.array_equal(back, R._hsv2rgb(img[..., 0].astype(np.int64), img[..., 1].astype(np.int64), img[..., 2].astype(np.int64)))


def test_gray_plane_equals_rgb_replicated():
    rng = np.random.default_rng(4)
    g = _image(rng, 120, 140)[..., :1]
    g3 = np.repeat(g, 3, axis=2)
    rec = DC.draw_views(rng, np.full(6, 120), np.full(6, 140), np.full(6, 1), 96, DC.LOCAL_SCALE, cutout=True)
    rec[:, DC.P_GRAY] = [0, 1, 0, 1, 0, 1]
    rec[:, DC.P_BLUR] = [1, 0, 1, 1, 0, 0]
    for r in rec:
        o1, t1, _, _ = R.view(g, r, 96)
        r3 = r.copy()
        r3[DC.P_C] = 3
        o3, t3, _, _ = R.view(g3, r3, 96)
        assert np.array_equal(o1.view(np.int32), o3.view(np.int32)) and np.array_equal(t1.view(np.int32), t3.view(np.int32))


@pytest.mark.parametrize("name", ["gray", "rgb", "long"])
def test_restatement_reproduces_the_fixture(name):
    z = np.load(os.path.join(GOLDEN, f"chest_aug_{name}.npz"))
    src = z["src"]
    rep = lambda a: np.repeat(a, 3, axis=2) if a.shape[2] == 1 else a
    for tag, S in (("g", 224), ("l", 96)):
        for k in range(len(z[f"{tag}_rec"])):
            out, tgt, sp, ph = R.view(src, z[f"{tag}_rec"][k], S)
            assert np.array_equal(rep(sp), z[f"{tag}_spatial"][k])
            assert np.array_equal(rep(ph), z[f"{tag}_photo"][k])
            assert np.array_equal(out.view(np.int32), z[f"{tag}_out"][k].view(np.int32))
            assert np.array_equal(tgt.view(np.int32), z[f"{tag}_target"][k].view(np.int32))


@pytest.mark.parametrize("name", ["gray", "rgb", "long"])
def test_fixture_regenerates_bit_identically(name):
    _pil()
    from make_chest_fixtures import make
    z = np.load(os.path.join(GOLDEN, f"chest_aug_{name}.npz"))
    new = make(name)
    assert sorted(new) == sorted(z.files)
    for k in z.files:
        assert new[k].dtype == z[k].dtype and np.array_equal(np.asarray(new[k]).view(np.uint8), z[k].view(np.uint8)), k


def test_fixture_sizes():
    total = sum(os.path.getsize(os.path.join(GOLDEN, f"chest_aug_{n}.npz")) for n in ("gray", "rgb", "long"))
    assert total <= 2 * 2 ** 20


def test_random_resized_crop_rules():
    rng = np.random.default_rng(5)
    N = 4000
    H, W = np.full(N, 257), np.full(N, 300)
    i, j, h, w = DC.draw_crops(rng, H, W, DC.GLOBAL_SCALE)
    assert ((w > 0) & (w <= W) & (h > 0) & (h <= H) & (i >= 0) & (j >= 0) & (i + h <= H) & (j + w <= W)).all()
    area = w * h / (257 * 300)
    assert area.min() > 0.29 and area.max() <= 1.01
    r = w / h
    assert (r > 0.74).all() and (r < 1.35).all()
    assert i.min() == 0 and (i + h).max() == 257           # every offset is reachable
    # elongated source: the global scale is unreachable within the ratio bounds -> the centre crop with the clamped ratio
    i, j, h, w = DC.draw_crops(rng, np.full(50, 90), np.full(50, 600), DC.GLOBAL_SCALE)
    assert (h == 90).all() and (w == 120).all() and (i == 0).all() and (j == 240).all()
    i, j, h, w = DC.draw_crops(rng, np.full(50, 600), np.full(50, 90), DC.GLOBAL_SCALE)
    assert (w == 90).all() and (h == 120).all() and (j == 0).all() and (i == 240).all()
    # the local scale fits in the elongated source: no fallback
    i, j, h, w = DC.draw_crops(rng, np.full(200, 90), np.full(200, 600), DC.LOCAL_SCALE)
    assert (w * h < 0.31 * 90 * 600).all() and (h <= 90).all()


def test_view_draw_probabilities_and_ranges():
    rng = np.random.default_rng(6)
    N = 20000
    raw = {}
    rec = DC.draw_views(rng, np.full(N, 300), np.full(N, 257), np.full(N, 1), 224, DC.GLOBAL_SCALE, cutout=True, raw=raw)
    assert abs(rec[:, DC.P_FLIP].mean() - 0.5) < 0.02
    assert abs(rec[:, DC.P_GRAY].mean() - 0.2) < 0.02
    assert abs(rec[:, DC.P_BLUR].mean() - 0.5) < 0.02
    assert (np.abs(raw["angle"]) <= 10).all() and raw["sigma"].min() >= 0.1 and raw["sigma"].max() <= 2.0
    assert raw["factors"].min() >= 0.6 and raw["factors"].max() <= 1.4 and np.abs(raw["hue"]).max() <= 0.4
    f = rec[:, DC.P_BRI:DC.P_SAT + 1].astype(np.int32).view(np.float32)
    assert np.array_equal(f, raw["factors"].astype(np.float32))
    assert all(DC.hue_shift(float(h)) == rec[n, DC.P_HUE] for n, h in enumerate(raw["hue"][:200]))
    assert DC.hue_shift(-0.001) == 0 and DC.hue_shift(-0.1) == 256 - 25 and DC.hue_shift(0.4) == 102
    perms = [tuple((int(o) >> (4 * k)) & 15 for k in range(4)) for o in rec[:, DC.P_ORDER]]
    assert all(sorted(p) == [0, 1, 2, 3] for p in perms) and len(set(perms)) == 24
    assert (rec[:, DC.P_NOPS] == 4).all()
    assert all(DC.rotate_fixed(float(a), 224, 224) == tuple(rec[n, DC.P_A0:DC.P_A5 + 1]) for n, a in enumerate(raw["angle"][:100]))
    # cutout: clipped squares of at most 32, centres uniform over the image
    holes = rec[:, DC.P_HOLES:DC.P_HOLES + 12].reshape(N, 3, 4)
    assert (rec[:, DC.P_NHOLES] == 3).all()
    assert (holes >= 0).all() and (holes <= 224).all()
    assert ((holes[..., 1] - holes[..., 0]) <= 32).all() and ((holes[..., 3] - holes[..., 2]) <= 32).all()
    assert (holes[..., 0] == 0).any() and (holes[..., 1] == 224).any() and ((holes[..., 1] - holes[..., 0]) < 32).any()
    loc = DC.draw_views(rng, np.full(10, 300), np.full(10, 257), np.full(10, 1), 96, DC.LOCAL_SCALE, cutout=False)
    assert (loc[:, DC.P_NHOLES] == 0).all()


def test_cutout_restatement_zeroes_the_clipped_squares():
    t = np.random.default_rng(7).standard_normal((3, 224, 224)).astype(np.float32)
    o = R.cutout(t, [(0, 16, 200, 224), (100, 132, 5, 37)])
    assert (o[:, :16, 200:] == 0).all() and (o[:, 100:132, 5:37] == 0).all()
    assert np.signbit(o[:, :16, 200:]).any()                       # t * 0 keeps the sign, as torch does
    keep = np.ones((224, 224), bool)
    keep[:16, 200:] = keep[100:132, 5:37] = False
    assert np.array_equal(o[:, keep], t[:, keep])


def _write_pngs(d, n, size=(64, 48), modes=("L",)):
    Image = _pil()
    rng = np.random.default_rng(8)
    names = []
    for k in range(n):
        mode = modes[k % len(modes)]
        shape = (size[1], size[0]) + ((3,) if mode == "RGB" else ())
        Image.fromarray(rng.integers(0, 256, shape, dtype=np.uint8), mode).save(os.path.join(d, f"img_{k:03d}.png"))
        names.append(f"img_{k:03d}.png")
    return names


def test_file_list_ratio_and_list_file(tmp_path, monkeypatch):
    d = tmp_path / "data"
    d.mkdir()
    names = _write_pngs(str(d), 10)
    monkeypatch.chdir(tmp_path)
    assert DC.chest_file_list(str(d), 1.0) == [str(d / n) for n in names]           # no list file: every png, sorted
    assert DC.chest_file_list(str(d), 0.5) == [str(d / n) for n in names[:5]]
    (tmp_path / "train_val_txt").mkdir()
    with open(tmp_path / "train_val_txt" / "chest_train.txt", "w") as f:
        for n in reversed(names[:6]):
            f.write(f"{n} 0 1 0\n")
    assert DC.chest_file_list(str(d), 1.0) == [str(d / n) for n in reversed(names[:6])]
    assert DC.chest_file_list(str(d), 0.5) == [str(d / n) for n in reversed(names[3:6])]
    with open(tmp_path / "train_val_txt" / "chest_train.txt", "a") as f:
        f.write("missing.png 1\n")
    with pytest.raises(FileNotFoundError, match="missing.png"):
        DC.chest_file_list(str(d), 1.0)


def test_equal_shards_and_eval_is_train(tmp_path, monkeypatch):
    d = tmp_path / "data"
    d.mkdir()
    _write_pngs(str(d), 7)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(DC, "AugmentedLoader", lambda files, b, workers, device, shuffle=True, seed=0, drop_last=False, kind=None: (list(files), drop_last, seed))
    lens = []
    for rank in range(2):
        monkeypatch.setenv("RANK", str(rank))
        monkeypatch.setenv("WORLD_SIZE", "2")
        dl = DC.chest_pretask_loaders(types.SimpleNamespace(data=str(d), ratio=1.0, b=2, workers=0, seed=3), device="cpu")
        files, drop, seed = dl["train"]
        assert drop is True and seed == 3 + rank and dl["eval"] is dl["train"]
        lens.append(len(files))
    assert lens == [3, 3]
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setenv("RANK", "0")
    files, drop, _ = DC.chest_pretask_loaders(types.SimpleNamespace(data=str(d), ratio=1.0, b=2, workers=0, seed=0), device="cpu")["train"]
    assert len(files) == 7 and drop is False


def test_decode_workers_write_the_right_pixels_into_the_shared_slots(tmp_path):
    """data_chest._SlotImages under data._SlotBatches: worker processes decode each image into (slot, row) of the shared buffers -- one plane
    for an L image, three for RGB -- with its (H, W, C); an image larger than the slots is an error naming the file."""
    Image = _pil()
    from pcrlv2_amd import data as D
    names = _write_pngs(str(tmp_path), 9, modes=("L", "RGB", "L"))
    files = [str(tmp_path / n) for n in names]
    kind = DC.ChestKind(files)
    assert kind.cap == 64 * 64 * 3
    b, nslots = 4, 2 * 2 + 6
    bufs = [torch.zeros((nslots, b) + sh, dtype=dt).share_memory_() for sh, dt in kind.slot_shapes()]
    sampler = D._SlotBatches(len(files), b, True, False, nslots, seed=5)
    loader = torch.utils.data.DataLoader(kind.slot_dataset(files, bufs), num_workers=2, collate_fn=lambda items: (items[0][0], len(items)),
                                         batch_sampler=sampler, prefetch_factor=2)
    g = torch.Generator()
    g.set_state(sampler.gen.get_state())
    order = torch.randperm(len(files), generator=g).tolist()
    delivered = []
    for k, (slot, rows) in enumerate(loader):
        for r, i in enumerate(order[k * b:(k + 1) * b][:rows]):
            with Image.open(files[i]) as im:
                a = _arr(im)
            assert tuple(bufs[1][slot, r].tolist()) == a.shape
            assert torch.equal(bufs[0][slot, r, :a.size], torch.from_numpy(a.reshape(-1).copy()))
            delivered.append(i)
    assert sorted(delivered) == list(range(len(files)))
    Image.fromarray(np.zeros((70, 70, 3), np.uint8), "RGB").save(tmp_path / "big.png")      # 14 700 bytes > 64 * 64 * 3
    with pytest.raises(ValueError, match="big.png"):
        kind.slot_dataset(files + [str(tmp_path / "big.png")], bufs)[(0, 0, len(files))]


def test_cli_builds_the_chest_loader_for_an_image_directory(tmp_path, monkeypatch):
    from pcrlv2_amd import main as M
    d = tmp_path / "imgs"
    d.mkdir()
    _write_pngs(str(d), 3)
    monkeypatch.chdir(tmp_path)
    seen = {}
    monkeypatch.setattr(DC, "chest_pretask_loaders", lambda args: seen.setdefault("args", args) and {"train": "T", "eval": "T"})
    args = M.build_parser().parse_args(["--data", str(d), "--d", "2", "--n", "chest", "--b", "4"])
    dl = M.get_dataloader(args)
    assert dl == {"train": "T", "eval": "T"} and seen["args"].data == str(d)
    with pytest.raises(SystemExit):
        M.get_dataloader(M.build_parser().parse_args(["--data", str(tmp_path / "nowhere"), "--d", "2"]))


def test_no_cpu_fallback():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DC.GpuChestAugment("cpu")
