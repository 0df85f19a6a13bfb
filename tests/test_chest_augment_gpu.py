"""The pcrl_aug2d_* kernels (csrc/augment2d.hip) against PILLOW's own output (the committed fixtures tests/golden/chest_aug_*.npz, written by
tools/make_chest_fixtures.py), the float32 tensors against torch CPU bit for bit, a whole drawn batch against the numpy restatement, and one
epoch of `main.py --d 2` on a directory of PNGs."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import chest_aug_reference as R  # noqa: E402
from pcrlv2_amd import data_chest as DC  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ("gray", "rgb", "long")


def _call(name, *args):
    from pcrlv2_amd._lib import lib, stream_handle
    lib().call(name, *args, stream_handle())


def _run(src, recs, S, target=True, view_in=None):
    """Kernels on one source image (uint8 [H, W, C]) and records [V, NPARAM] -> (view u8 [V,3,S,S], target, out, photometric u8)."""
    recs = np.array(recs, np.int64).reshape(-1, DC.NPARAM)
    V = recs.shape[0]
    H, W, C = src.shape
    recs[:, DC.P_SRC], recs[:, DC.P_H], recs[:, DC.P_W], recs[:, DC.P_C] = 0, H, W, C
    DC.pack_offsets(recs, [0], np.zeros(V, np.int64), S)
    dev = torch.device("cuda")
    rec_d = torch.from_numpy(recs.astype(np.int32)).to(dev)
    src_d = torch.from_numpy(np.ascontiguousarray(src).reshape(-1)).to(dev)
    if view_in is None:
        inter = torch.empty(int((recs[:, DC.P_CH] * S * C).sum()), dtype=torch.uint8, device=dev)
        _call("pcrl_aug2d_hresample", src_d, rec_d, inter, V, S, int(recs[:, DC.P_CH].max()))
        view = torch.zeros((V, 3, S, S), dtype=torch.uint8, device=dev)
        tgt = torch.empty((V, 3, S, S), dtype=torch.float32, device=dev) if target else None
        _call("pcrl_aug2d_spatial", inter, rec_d, view, tgt, V, S)
    else:
        view, tgt = view_in.to(dev), None
    out = torch.empty((V, 3, S, S), dtype=torch.float32, device=dev)
    u8 = torch.zeros((V, 3, S, S), dtype=torch.uint8, device=dev)
    _call("pcrl_aug2d_photometric", view, rec_d, out, u8, V, S)
    torch.cuda.synchronize()
    cpu = lambda t: None if t is None else t.cpu().numpy()
    return cpu(view), cpu(tgt), cpu(out), cpu(u8)


def _planes(a, C):
    """uint8 [.., H, W, 3] Pillow output -> [.., C, H, W] planes (a gray image: its one plane)."""
    return np.moveaxis(a, -1, -3)[..., :C, :, :]


def _identity_record(S, **kw):
    r = np.zeros(DC.NPARAM, np.int64)
    r[DC.P_A0:DC.P_A5 + 1] = DC.rotate_fixed(0.0, S, S)
    for k, v in kw.items():
        r[getattr(DC, "P_" + k.upper())] = v
    return r


def _mismatch(a, b, what):
    d = np.abs(a.astype(np.int64) - b.astype(np.int64))
    if d.any():
        print(f"[{what}] {int((d > 0).sum())} of {d.size} values differ, at most by {int(d.max())}")
    return d


def _fixture(name):
    return np.load(os.path.join(GOLDEN, f"chest_aug_{name}.npz"))


@pytest.mark.parametrize("name", NAMES)
def test_resize_and_rotation_kernels_equal_pillow(name):
    z = _fixture(name)
    src = z["src"]
    C = src.shape[2]
    flat, pos = z["resize_out"], 0
    for j, i, w, h, S in z["resize_box"]:
        ref = flat[pos:pos + S * S * 3].reshape(S, S, 3)
        pos += S * S * 3
        view, _, _, _ = _run(src, [_identity_record(S, j=j, i=i, cw=w, ch=h)], int(S))
        assert not _mismatch(view[0, :C], _planes(ref, C), f"{name} resize {w}x{h}->{S}").any()
    base = z["base"][..., :C]
    S = base.shape[0]
    for fixed, ref in zip(z["rotate_fixed"], z["rotate_out"]):
        r = _identity_record(S, cw=S, ch=S)
        r[DC.P_A0:DC.P_A5 + 1] = fixed
        view, tgt, _, _ = _run(base, [r], S)
        assert not _mismatch(view[0, :C], _planes(ref, C), f"{name} rotate").any()
        assert np.array_equal(tgt[0].view(np.int32), R.normalize(ref).view(np.int32))


@pytest.mark.parametrize("name", NAMES)
def test_photometric_kernel_equals_pillow_operation_by_operation(name):
    z = _fixture(name)
    C = z["src"].shape[2]
    base = z["base"][..., :C]
    S = base.shape[0]
    view = torch.zeros((1, 3, S, S), dtype=torch.uint8)
    view[0, :C] = torch.from_numpy(np.ascontiguousarray(np.moveaxis(base, -1, 0)))
    cases = [("gray", _identity_record(S, gray=1), z["gray_out"])]
    for (r, ww, fw), ref in zip(z["blur_params"], z["blur_out"]):
        cases.append(("blur", _identity_record(S, blur=1, br=r, ww=ww, fw=fw), ref))
    for op, slot in ((0, "bri"), (1, "con"), (2, "sat")):
        for f, ref in zip(z["jitter_factors"][op], z["jitter_out"][op]):
            cases.append((slot, _identity_record(S, nops=1, order=op, **{slot: int(np.float32(f).view(np.int32))}), ref))
    for h, ref in zip(z["jitter_hue"], z["jitter_out"][3]):
        cases.append(("hue", _identity_record(S, nops=1, order=3, hue=DC.hue_shift(float(h))), ref))
    for what, rec, ref in cases:
        _, _, out, u8 = _run(base, [rec], S, view_in=view)
        assert not _mismatch(u8[0, :C], _planes(ref, C), f"{name} {what}").any()
        assert np.array_equal(out[0].view(np.int32), R.normalize(ref).view(np.int32))


@pytest.mark.parametrize("name", NAMES)
def test_whole_views_equal_pillow_and_torch_cpu(name):
    """Drawn records: the spatial view and the photometric view uint8-identical to Pillow, the float32 outputs and targets bit-identical to
    torch CPU's ToTensor -> Normalize (-> Cutout: its squares exactly zero, in the global views only)."""
    z = _fixture(name)
    src = z["src"]
    C = src.shape[2]
    for tag, S in (("g", 224), ("l", 96)):
        view, tgt, out, u8 = _run(src, z[f"{tag}_rec"], S)
        assert not _mismatch(view[:, :C], _planes(z[f"{tag}_spatial"], C), f"{name} {tag} spatial").any()
        assert not _mismatch(u8[:, :C], _planes(z[f"{tag}_photo"], C), f"{name} {tag} photometric").any()
        assert np.array_equal(out.view(np.int32), z[f"{tag}_out"].view(np.int32))
        assert np.array_equal(tgt.view(np.int32), z[f"{tag}_target"].view(np.int32))
        for k, rec in enumerate(z[f"{tag}_rec"]):
            for h in range(int(rec[DC.P_NHOLES])):
                y0, y1, x0, x1 = rec[DC.P_HOLES + 4 * h:DC.P_HOLES + 4 * h + 4]
                assert (out[k, :, y0:y1, x0:x1] == 0).all()
        assert (z[f"{tag}_rec"][:, DC.P_NHOLES] > 0).all() == (tag == "g")


def _batch_images(b, seed=0):
    rng = np.random.default_rng(seed)
    imgs = []
    for n in range(b):
        H, W = int(rng.integers(200, 320)), int(rng.integers(200, 320))
        y, x = np.mgrid[0:H, 0:W]
        a = np.stack([(x * 255) // W, (y * 255) // H, ((x * y) // 64) % 256], -1)
        a = (a + rng.integers(0, 30, a.shape)).clip(0, 255).astype(np.uint8)
        imgs.append(a[..., :1].copy() if n % 2 == 0 else a)        # mixed gray and RGB sources
    return imgs


def _pack(imgs, cap):
    pix = torch.zeros((len(imgs), cap), dtype=torch.uint8)
    for n, a in enumerate(imgs):
        pix[n, :a.size] = torch.from_numpy(a.reshape(-1))
    return pix, torch.tensor([a.shape for a in imgs], dtype=torch.int32)


def test_batch_from_drawn_parameters_equals_the_restatement():
    b = 8
    imgs = _batch_images(b)
    pix, dims = _pack(imgs, 320 * 320 * 3)
    aug = DC.GpuChestAugment("cuda", seed=4)
    rng0 = copy.deepcopy(aug.rng)
    y1, y2, x, x2, loc = aug(pix, dims)
    torch.cuda.synchronize()
    for t in (y1, y2, x, x2):
        assert t.shape == (b, 3, 224, 224) and t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda
    assert len(loc) == 6 and all(t.shape == (b, 3, 96, 96) and t.dtype == torch.float32 and t.is_contiguous() for t in loc)
    aug.rng = rng0
    rec, _, _ = aug.draw(dims.numpy())
    got = [y1, y2] + list(loc)
    tg = [x, x2]
    for v in range(8 * b):
        k, n = divmod(v, b)
        S = 224 if k < 2 else 96
        out, target, _, _ = R.view(imgs[n], rec[v], S)
        assert np.array_equal(got[k][n].cpu().numpy().view(np.int32), out.view(np.int32)), (k, n)
        if k < 2:
            assert np.array_equal(tg[k][n].cpu().numpy().view(np.int32), target.view(np.int32)), (k, n)


def test_same_seed_same_batch_and_gray_equals_rgb_replicated():
    b = 6
    imgs = _batch_images(b, seed=1)
    pix, dims = _pack(imgs, 320 * 320 * 3)
    a = DC.GpuChestAugment("cuda", seed=9)(pix, dims)
    c = DC.GpuChestAugment("cuda", seed=9)(pix, dims)
    flat = lambda t: [t[0], t[1], t[2], t[3]] + list(t[4])
    assert all(torch.equal(u.view(torch.int32), w.view(torch.int32)) for u, w in zip(flat(a), flat(c)))
    rgb = [np.repeat(i, 3, axis=2) if i.shape[2] == 1 else i for i in imgs]
    pix3, dims3 = _pack(rgb, 320 * 320 * 3)
    aug1, aug3 = DC.GpuChestAugment("cuda", seed=2), DC.GpuChestAugment("cuda", seed=2)
    g1, g3 = aug1(pix, dims), aug3(pix3, dims3)          # the same draws: they depend on H and W only
    assert all(torch.equal(u.view(torch.int32), w.view(torch.int32)) for u, w in zip(flat(g1), flat(g3)))


_E2E = r"""
import math, os, sys
import torch
sys.path.insert(0, sys.argv[1])
from pcrlv2_amd import main as M
M.main(['--data', sys.argv[2], '--d', '2', '--n', 'chest', '--b', '4', '--epochs', '1', '--gpus', '0', '--amp', '--workers', '2',
        '--ratio', '1.0', '--lr', '1e-2', '--output', sys.argv[3]])
ck = torch.load(os.path.join(sys.argv[3], 'pcrlv2_chest_pretask_1.0_0.pt'), map_location='cpu', weights_only=False)
assert all(torch.isfinite(v).all() for v in ck['state_dict'].values() if v.is_floating_point())
print('E2E OK')
"""


def test_main_runs_one_epoch_on_a_directory_of_pngs(tmp_path):
    Image = pytest.importorskip("PIL.Image", reason="Pillow is needed to write the PNGs")
    d = tmp_path / "imgs"
    d.mkdir()
    rng = np.random.default_rng(0)
    for k in range(40):
        H, W = 256 - 8 * (k % 3), 256          # the first file sizes the slots
        y, x = np.mgrid[0:H, 0:W]
        a = ((x + y + 7 * k) % 256).astype(np.uint8)
        a = (a.astype(np.int64) + rng.integers(0, 20, a.shape)).clip(0, 255).astype(np.uint8)
        Image.fromarray(a if k % 8 else np.stack([a, a // 2, 255 - a], -1)).save(d / f"{k:03d}.png")
    script = tmp_path / "e2e.py"
    script.write_text(_E2E)
    out = tmp_path / "out"
    env = dict(os.environ, PYTHONNOUSERSITE="1")
    r = subprocess.run([sys.executable, str(script), ROOT, str(d), str(out)], cwd=str(tmp_path), capture_output=True, text=True, timeout=600, env=env)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "E2E OK" in r.stdout and "nan" not in r.stdout.lower(), tail
