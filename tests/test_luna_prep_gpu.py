"""LUNA16 pre-processing on the GPU: `pcrl_prep_resample` and `pcrl_prep_windows` (csrc/luna_prep.hip) against the float64 restatement
(tests/luna_prep_reference.py) and scipy's committed outputs (tests/golden/luna_prep_windows.npz), bit for bit; then the whole tool,
`luna_preprocess.py`, on synthetic MetaImage series against the restatement pipeline, and one `main.py` epoch on what it wrote."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import luna_prep_reference as R  # noqa: E402
from pcrlv2_amd import luna_prep as P  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(ROOT, "tests", "golden", "luna_prep_windows.npz")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.mark.parametrize("shape,spacing", [((37, 61, 53), (0.703125, 0.703125, 2.5)), ((29, 45, 70), (0.6, 0.6, 1.25)),
                                           ((11, 13, 17), (1.7, 0.9, 3.3))])
def test_resample_matches_restatement(dev, shape, spacing):
    rng = np.random.default_rng(sum(shape))
    vol = rng.integers(-32768, 32768, shape).astype(np.int16)
    vol[:, :, :5] = rng.integers(-1100, 1500, (shape[0], shape[1], 5))
    Z, Y, X = shape
    out_xyz = P.resample_size((X, Y, Z), spacing)
    got = P.gpu_resample(torch.from_numpy(vol).to(dev), spacing, out_xyz).cpu().numpy()
    ref = R.resample(vol, spacing, out_xyz)
    assert got.shape == ref.shape == out_xyz[::-1]
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:5]


def _run_windows(dev, vol_zyx, cases, padded_z=None):
    """cases: (start, src, out shape, score depth) -> ([outputs], stats) with every output depth stored."""
    recs, prms = [], []
    oo = wo = 0
    for start, src, oshape, scored in cases:
        rec, prm = P.window_record(start, src, oshape, oo, oshape[2], wo, scored)
        recs.append(rec)
        prms.append(prm)
        oo += int(np.prod(oshape))
        wo += 2 * int(np.prod(src))
    rec, prm = np.stack(recs), np.stack(prms)
    Z, Y, X = vol_zyx.shape
    out, stats = P.gpu_windows(torch.from_numpy(vol_zyx).to(dev), rec, prm, oo, wo, int(max(np.prod(c[1]) for c in cases)),
                               int(max(c[2][0] * c[2][1] for c in cases)), (X, Y, padded_z or Z))
    out, stats = out.cpu().numpy(), stats.cpu().numpy()
    res = []
    for (start, src, oshape, _), r in zip(cases, rec):
        res.append(out[r[12]:r[12] + int(np.prod(oshape))].reshape(oshape))
    return res, stats


def test_windows_match_scipy_fixture_and_restatement(dev):
    z = np.load(FIXTURE)
    vol = z["vol"]
    logical = R.normalise(vol.transpose(2, 1, 0))
    cases = [(tuple(map(int, s)), tuple(map(int, n)), tuple(map(int, o)), 32 if tuple(o) == (64, 64, 35) else 0)
             for s, n, o in zip(z["start"], z["src"], z["out_shape"])]
    outs, stats = _run_windows(dev, vol, cases)
    sub_off = np.concatenate([[0], np.cumsum(z["sub_len"])])
    for i, ((s, n, o, scored), got) in enumerate(zip(cases, outs)):
        crop = logical[s[0]:s[0] + n[0], s[1]:s[1] + n[1], s[2]:s[2] + n[2]]
        ref = crop if n == (64, 64, 35) else R.resize(crop, o)
        assert np.array_equal(got, ref), (n, np.abs(got - ref).max())
        np.testing.assert_array_equal(got.reshape(-1)[::int(z["sub_stride"])], z["sub"][sub_off[i]:sub_off[i + 1]])
        assert hashlib.sha256(np.ascontiguousarray(got).tobytes()).digest() == z["sha256"][i].tobytes(), n
        raw = vol.transpose(2, 1, 0)[s[0]:s[0] + n[0], s[1]:s[1] + n[1], s[2]:s[2] + n[2]]
        assert (stats[i, 1], stats[i, 2]) == (raw.min(), raw.max())
        if scored:
            assert stats[i, 0] == z["score"][i] == R.depth_score(ref)
        else:
            assert stats[i, 0] == 0


def test_windows_read_the_end_pad_and_many_windows(dev):
    """z beyond the volume reads as HU -1000 (the reference's pad); 40 windows of mixed classes in one launch."""
    rng = np.random.default_rng(9)
    vol = rng.integers(-1200, 1400, (70, 120, 118)).astype(np.int16)      # (z, y, x); padded to 99 in z
    padded = np.concatenate([R.normalise(vol.transpose(2, 1, 0)), np.zeros((118, 120, 29))], axis=2)
    cases = []
    for q in range(40):
        if q % 4 == 0:
            src = (96, 96, 67) if q % 8 == 0 else (64, 64, 35)
            start = (int(rng.integers(0, 118 - src[0] + 1)), int(rng.integers(0, 120 - src[1] + 1)), 99 - src[2] - int(rng.integers(0, 3)))
            cases.append((start, src, (64, 64, 35), 32))
        else:
            start = tuple(int(rng.integers(0, m)) for m in (118, 120, 99))
            n = tuple(min(start[a] + int(rng.choice([8, 16, 32])), (118, 120, 99)[a]) - start[a] for a in range(3))
            cases.append((start, n, (16, 16, 16), 0))
    outs, stats = _run_windows(dev, vol, cases, padded_z=99)
    for (s, n, o, scored), got, st in zip(cases, outs, stats):
        crop = padded[s[0]:s[0] + n[0], s[1]:s[1] + n[1], s[2]:s[2] + n[2]]
        ref = crop if n == (64, 64, 35) else R.resize(crop, o)
        assert np.array_equal(got, ref), (s, n)
        if scored:
            assert st[0] == R.depth_score(ref)


# ---- the tool, end to end ----------------------------------------------------------------------------------------------------------
def _phantom(rng, shape_zyx):
    """CT-like int16: body wall tissue, lungs at about -850 HU, a slab of soft tissue (rejected crops) and vessels."""
    Z, Y, X = shape_zyx
    z, y, x = np.ogrid[0:Z, 0:Y, 0:X]
    v = np.full(shape_zyx, 40, dtype=np.int32)
    v[np.broadcast_to((np.abs(x - X / 2) < 0.42 * X) & (np.abs(y - Y / 2) < 0.42 * Y), shape_zyx)] = -850
    v[np.broadcast_to((x > 0.45 * X) & (x < 0.6 * X), shape_zyx)] = 30
    for _ in range(30):
        c = rng.uniform([0, 0, 0], [X, Y, Z])
        v[np.broadcast_to(((x - c[0]) ** 2 + (y - c[1]) ** 2) < rng.uniform(4, 30), shape_zyx)] = 60
    v += rng.integers(-30, 31, shape_zyx)
    v[:, :4, :] = -3024                          # outside the scanner's field of view
    return v.astype(np.int16)


@pytest.fixture(scope="module")
def luna_tree(tmp_path_factory):
    rng = np.random.default_rng(1234)
    d = tmp_path_factory.mktemp("luna")
    series = {0: [("1.3.6.1.4.1.14519.5.2.1.6279.6001.100", (108, 330, 328), (0.703125, 0.703125, 1.25)),
                  ("1.3.6.1.4.1.14519.5.2.1.6279.6001.101", (90, 390, 380), (0.6, 0.6, 1.5))],
              1: [("1.3.6.1.4.1.14519.5.2.1.6279.6001.102", (36, 330, 330), (0.703125, 0.703125, 2.5))],     # 90 mm: padded, then skipped
              8: [("1.3.6.1.4.1.14519.5.2.1.6279.6001.103", (60, 300, 300), (0.78, 0.78, 2.5))]}
    made = []
    for fold, lst in series.items():
        (d / f"subset{fold}").mkdir()
        for name, shape, spacing in lst:
            vol = _phantom(rng, shape)
            P.write_metaimage(str(d / f"subset{fold}" / f"{name}.mhd"), vol, spacing)
            made.append((fold, name, vol, spacing))
    return d, made


def _preprocess(data, save, *extra):
    cmd = ["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "luna_preprocess.py"), "--data", str(data), "--save", str(save),
           "--scale", "2", "--seed", "7", *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def _tree(save):
    out = {}
    for root, _, files in os.walk(save):
        for f in files:
            with open(os.path.join(root, f), "rb") as fh:
                out[os.path.relpath(os.path.join(root, f), save)] = hashlib.sha256(fh.read()).hexdigest()
    return out


def test_preprocess_matches_restatement_and_is_independent_of_k(luna_tree, tmp_path):
    data, made = luna_tree
    log = _preprocess(data, tmp_path / "k16")
    _preprocess(data, tmp_path / "k1", "--attempts-per-launch", "1")
    _preprocess(data, tmp_path / "k64", "--attempts-per-launch", "64")
    t16 = _tree(tmp_path / "k16")
    assert t16 == _tree(tmp_path / "k1") == _tree(tmp_path / "k64")
    written = 0
    for fold, name, vol, spacing in made:
        ref = R.series(vol, spacing, name, 7, 2)
        g0 = tmp_path / "k16" / f"subset{fold}" / f"{name}_global_0.npy"
        if isinstance(ref, str):
            assert not g0.exists() and f"skip {data}/subset{fold}/{name}.mhd" in log.replace("//", "/")
            continue
        for k, (g, loc) in enumerate(ref):
            got_g = np.load(tmp_path / "k16" / f"subset{fold}" / f"{name}_global_{k}.npy")
            got_l = np.load(tmp_path / "k16" / f"subset{fold}" / f"{name}_local_{k}.npy")
            assert got_g.dtype == np.float64 and got_g.shape == (2, 64, 64, 32) and got_g.flags.c_contiguous
            assert got_l.dtype == np.float64 and got_l.shape == (6, 16, 16, 16)
            assert np.array_equal(got_g, g), (name, k)
            assert np.array_equal(got_l, loc), (name, k)
            written += 1
    assert written >= 4 and len(t16) == 2 * written
    assert not (tmp_path / "k16" / "subset1" / f"{made[2][1]}_global_0.npy").exists()      # the short series


def test_main_trains_one_epoch_on_the_output(luna_tree, tmp_path):
    data, _ = luna_tree
    _preprocess(data, tmp_path / "pre", "--float32")
    cmd = ["timeout", "-k", "10", "900", sys.executable, os.path.join(ROOT, "main.py"), "--d", "3", "--data", str(tmp_path / "pre"),
           "--b", "2", "--epochs", "1", "--gpus", "0", "--workers", "2", "--output", str(tmp_path / "ckpt")]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
