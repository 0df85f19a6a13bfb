"""Writes tests/golden/chest_aug_{gray,rgb,long}.npz: synthetic sources Pillow can make, explicit parameter records of pcrlv2_amd.data_chest,
and PILLOW's output for every operation of the 2D augmentation chain alone and for whole 224 / 96 views, plus the float32 tensors torch CPU
gives for ToTensor -> Normalize -> Cutout.  Deterministic: tests/test_chest_data_cpu.py regenerates the fixtures and compares them bit for bit.

    python tools/make_chest_fixtures.py [OUT_DIR]
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NAMES = ("gray", "rgb", "long")


def source(name):
    """-> PIL image: a gray 300 x 257 L image with edges and gradients, an RGB image whose channels differ (hue matters), and a 600 x 90
    L image whose aspect ratio forces RandomResizedCrop's fallback for the global views."""
    from PIL import Image, ImageDraw
    if name == "gray":
        W, H = 300, 257
        y, x = np.mgrid[0:H, 0:W]
        a = ((x * 200) // W + (y * 55) // H).astype(np.uint8)
        a[(x // 17 + y // 13) % 2 == 0] //= 2
        im = Image.fromarray(a, "L")
        d = ImageDraw.Draw(im)
        d.ellipse((60, 40, 200, 180), fill=240)
        d.rectangle((220, 150, 280, 240), fill=10)
        d.line((0, 256, 299, 0), fill=255, width=3)
        return im
    if name == "rgb":
        W, H = 280, 240
        y, x = np.mgrid[0:H, 0:W]
        a = np.stack([(x * 255) // W, (y * 255) // H, ((x + y) * 255) // (W + H)], -1).astype(np.uint8)
        im = Image.fromarray(a, "RGB")
        d = ImageDraw.Draw(im)
        d.ellipse((30, 30, 150, 130), fill=(220, 40, 90))
        d.rectangle((160, 100, 260, 220), fill=(20, 200, 60))
        d.polygon([(10, 230), (120, 150), (200, 235)], fill=(250, 250, 10))
        return im
    if name == "long":
        W, H = 600, 90
        y, x = np.mgrid[0:H, 0:W]
        a = ((x % 64) * 3 + y).clip(0, 255).astype(np.uint8)
        im = Image.fromarray(a, "L")
        ImageDraw.Draw(im).rectangle((250, 20, 350, 70), fill=200)
        return im
    raise ValueError(name)


def _arr(im):
    a = np.asarray(im, dtype=np.uint8)
    return a.reshape(a.shape[0], a.shape[1], -1).copy()


def pil_spatial(img, rec, angle, S):
    """torchvision's RandomResizedCrop + RandomRotation + RandomHorizontalFlip on a PIL RGB image with the drawn parameters."""
    from PIL import Image
    from pcrlv2_amd import data_chest as DC
    j, i, w, h = (int(rec[k]) for k in (DC.P_J, DC.P_I, DC.P_CW, DC.P_CH))
    v = img.crop((j, i, j + w, i + h)).resize((S, S), Image.BILINEAR)
    v = v.rotate(float(angle), Image.NEAREST, expand=False, fillcolor=(0, 0, 0))
    if rec[DC.P_FLIP]:
        v = v.transpose(Image.FLIP_LEFT_RIGHT)
    return v


def pil_gray(v):
    from PIL import Image
    return Image.merge("RGB", [v.convert("L")] * 3)


def pil_blur(v, sigma):
    from PIL import ImageFilter
    return v.filter(ImageFilter.GaussianBlur(radius=float(sigma)))


def pil_jitter_op(v, op, factors, hue):
    from PIL import Image, ImageEnhance
    if op == 0:
        return ImageEnhance.Brightness(v).enhance(float(factors[0]))
    if op == 1:
        return ImageEnhance.Contrast(v).enhance(float(factors[1]))
    if op == 2:
        return ImageEnhance.Color(v).enhance(float(factors[2]))
    h, s, val = v.convert("HSV").split()
    nh = np.array(h, dtype=np.uint8)
    with np.errstate(over="ignore", invalid="ignore"):
        nh += np.array(float(hue) * 255).astype(np.int64).astype(np.uint8)      # torchvision: truncated toward zero, then wrapped
    return Image.merge("HSV", (Image.fromarray(nh, "L"), s, val)).convert("RGB")


def torch_tensor(v, holes=()):
    """ToTensor -> Normalize -> Cutout on torch CPU, the reference's exact float32 ops."""
    import torch
    t = torch.from_numpy(_arr(v)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    mean = torch.as_tensor([0.485, 0.456, 0.406], dtype=torch.float32)[:, None, None]
    std = torch.as_tensor([0.229, 0.224, 0.225], dtype=torch.float32)[:, None, None]
    t = t.sub(mean).div(std)
    if holes:
        m = np.ones(t.shape[1:], np.float32)
        for y0, y1, x0, x1 in holes:
            m[y0:y1, x0:x1] = 0.
        t = t * torch.from_numpy(m).expand_as(t)
    return t.numpy()


def make(name):
    """-> {array name: array} of one fixture."""
    from pcrlv2_amd import data_chest as DC
    im = source(name)
    src = _arr(im)                               # what the decode worker hands over: one plane for L
    rgb = im.convert("RGB")                      # what the reference's transforms see
    H, W, C = src.shape
    rng = np.random.default_rng({"gray": 11, "rgb": 12, "long": 13}[name])
    out = {"src": src}
    # -- whole views from drawn records: 2 global (with cutout), 2 local --
    for tag, S, scale, n, cut in (("g", DC.GLOBAL_SIZE, DC.GLOBAL_SCALE, 2, True), ("l", DC.LOCAL_SIZE, DC.LOCAL_SCALE, 2, False)):
        raw = {}
        rec = DC.draw_views(rng, np.full(n, H), np.full(n, W), np.full(n, C), S, scale, cutout=cut, raw=raw)
        sp, ph, fl, tg = [], [], [], []
        for k in range(n):
            v = pil_spatial(rgb, rec[k], raw["angle"][k], S)
            sp.append(_arr(v))
            tg.append(torch_tensor(v))
            if rec[k, DC.P_GRAY]:
                v = pil_gray(v)
            if rec[k, DC.P_BLUR]:
                v = pil_blur(v, raw["sigma"][k])
            for o in range(4):
                v = pil_jitter_op(v, (int(rec[k, DC.P_ORDER]) >> (4 * o)) & 15, raw["factors"][k], raw["hue"][k])
            ph.append(_arr(v))
            holes = [tuple(int(x) for x in rec[k, DC.P_HOLES + 4 * h:DC.P_HOLES + 4 * h + 4]) for h in range(int(rec[k, DC.P_NHOLES]))]
            fl.append(torch_tensor(v, holes))
        out.update({f"{tag}_rec": rec.astype(np.int32), f"{tag}_spatial": np.stack(sp), f"{tag}_photo": np.stack(ph),
                    f"{tag}_out": np.stack(fl), f"{tag}_target": np.stack(tg)})
    # -- each operation alone --
    S = DC.LOCAL_SIZE
    crops = DC.draw_crops(rng, np.full(4, H), np.full(4, W), (0.05, 1.0))
    sizes = np.array([DC.GLOBAL_SIZE, S, S, DC.GLOBAL_SIZE])
    out["resize_box"] = np.stack([crops[1], crops[0], crops[3], crops[2], sizes], 1).astype(np.int32)     # j, i, w, h, S
    from PIL import Image
    out["resize_out"] = [_arr(rgb.crop((j, i, j + w, i + h)).resize((s, s), Image.BILINEAR)) for j, i, w, h, s in out["resize_box"]]
    base = rgb.resize((S, S), Image.BILINEAR)      # the view every photometric op and the rotation start from
    out["base"] = _arr(base)
    out["rotate_angle"] = rng.uniform(-10, 10, 3)
    out["rotate_fixed"] = np.array([DC.rotate_fixed(float(a), S, S) for a in out["rotate_angle"]], np.int32)
    out["rotate_out"] = np.stack([_arr(base.rotate(float(a), Image.NEAREST, expand=False, fillcolor=(0, 0, 0))) for a in out["rotate_angle"]])
    out["gray_out"] = _arr(pil_gray(base))
    out["blur_sigma"] = np.array([0.1, 0.5, float(rng.uniform(0.1, 2.0)), 2.0])
    out["blur_params"] = np.array([DC.blur_params(float(s)) for s in out["blur_sigma"]], np.int64)
    out["blur_out"] = np.stack([_arr(pil_blur(base, s)) for s in out["blur_sigma"]])
    fac = rng.uniform(0.6, 1.4, (3, 3))
    out["jitter_factors"] = fac                                       # [op 0..2][draw]
    out["jitter_hue"] = np.concatenate([[-0.4, 0.4], rng.uniform(-0.4, 0.4, 1)])
    out["jitter_out"] = np.stack([np.stack([_arr(pil_jitter_op(base, op, [fac[op, d]] * 3, 0.0)) for d in range(3)]) for op in range(3)]
                                 + [np.stack([_arr(pil_jitter_op(base, 3, [1, 1, 1], h)) for h in out["jitter_hue"]])])
    out["resize_out"] = np.concatenate([a.reshape(-1) for a in out["resize_out"]])      # ragged (224 and 96 views), flattened in order
    return out


def main(out_dir=None):
    out_dir = out_dir or os.path.join(ROOT, "tests", "golden")
    for name in NAMES:
        path = os.path.join(out_dir, f"chest_aug_{name}.npz")
        np.savez_compressed(path, **make(name))
        print(path, os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
