"""pcrl_surf_extract, pcrl_edt_sq, pcrl_surf_dist_stats (csrc/surface_dist.hip), train_seg.surface_metrics and `seg3d.py score` on the device.

EQUAL, bit for bit, to tests/surface_reference.py: the surface bitmasks, the integer counts, d2 (+inf throughout for an empty surface), n_a, n_b, lo
and the three order statistics of d2 (the device selects them on the bit patterns; the restatement sorts).
The two sums of sqrt(d2) against math.fsum: within (n + 2) 2^-53 sum.  The n terms are positive, so ANY order of the n - 1 additions -- per thread,
wave shuffle, per block, block order -- has a relative error of at most (n - 1) u to first order, u = 2^-53 (each partial sum is at most the
total); every term carries the one rounding of its sqrt, at most u of itself, u sum in all; fsum rounds once more: (n - 1) + 1 + 1 <= n + 2.
surface_metrics: hd95 is EXACTLY np.percentile of the restatement's distances -- the host takes sqrt of the two selected d2 (sqrt is monotone, so
they are the distances' order statistics) and repeats numpy's two-sided lerp one operation at a time (test_surface_cpu.py pins that finish against
np.percentile for five quantiles); hd is exact; assd = (sum_a / n_a + sum_b / n_b) / 2 is within the sums' bound, relative, plus two roundings on
each side (a division per term, the addition; the halving is exact): (max(n_a, n_b) + 2 + 4) u assd.
Tile edges (csrc/surface_dist.hip): the extract grid is capped at 1024 blocks x 256 threads x 4 z; a Z-pass tile is min(4096 / Z, 512) lines; a Y- or X-pass tile
is min(8128 / L, 64) inner positions; the statistics grids are capped at 1024 x 256 voxels; an axis has at most 1024 voxels.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import surface_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
EXTRACT_CAP_ITEMS, STATS_CAP, INNER_TILE, INNER_LINES, LDS_TILE, MAX_RUN, MAX_AXIS = 1024 * 256, 1024 * 256, 4096, 512, 8128, 64, 1024
SPACINGS = [(1.0, 1.0, 1.0), (0.78125, 0.78125, 1.25), (0.7, 0.7, 2.5)]
GUARD, CANARY = 64, 0xA5


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(shape, dtype, offset=0):
    """A canary-filled buffer and a contiguous view of `shape` inside it, GUARD + offset elements from its start."""
    n = int(np.prod(shape))
    full = torch.empty(n + 2 * GUARD + offset, dtype=torch.uint8 if dtype == torch.uint8 else torch.int64, device="cuda")
    full.fill_(CANARY if dtype == torch.uint8 else 0x5A5A5A5A5A5A5A5A)
    return full, full[GUARD + offset:GUARD + offset + n].view(dtype).view(shape)


def _intact(full, n, offset=0):
    want = CANARY if full.dtype == torch.uint8 else 0x5A5A5A5A5A5A5A5A
    return bool((full[:GUARD + offset] == want).all()) and bool((full[GUARD + offset + n:] == want).all())


def _mask_pair(kind, shape, K, seed):
    """-> (pred, gt) uint8 bitmasks of one of the issue's mask kinds."""
    full = np.uint8((1 << K) - 1)
    pred, gt = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    if kind == "blobs":
        pred, gt = R.blobs(shape, K, seed), R.sprinkle_not_counted(R.blobs(shape, K, seed + 1), seed + 2)
    elif kind == "voxel":
        pred[tuple(s // 2 for s in shape)] = full
        gt[tuple(0 for _ in shape)] = full
    elif kind == "full":
        pred[:], gt[:] = full, full
        gt[tuple(s // 2 for s in shape)] = 0x80
    elif kind == "empty":
        pass
    elif kind == "equal":
        pred = R.blobs(shape, K, seed)
        gt = pred.copy()
    elif kind == "corners":
        pred[tuple(slice(0, max(1, s // 3)) for s in shape)] = full
        gt[tuple(slice(s - max(1, s // 3), s) for s in shape)] = full
    elif kind == "symmetric":         # gt is pred reflected through the centre: every distance occurs at least twice
        pred = R.blobs(shape, K, seed, level=0.8)
        gt = np.ascontiguousarray(pred[::-1, ::-1, ::-1])
    elif kind == "pred_only":
        pred = R.blobs(shape, K, seed)
    return pred, gt


def _extract_raw(pred, gt, K, prefill, offset=0):
    from pcrlv2_amd._lib import lib, stream_handle
    shape, n = pred.shape, pred.size
    fp, sp = _guarded(shape, torch.uint8, offset)
    fg, sg = _guarded(shape, torch.uint8, offset)
    fc, counts = _guarded((K, 3), torch.int64)
    counts.copy_(_dev(prefill))
    lib().call("pcrl_surf_extract", _dev(pred), _dev(gt), sp, sg, counts, *shape, K, stream_handle())
    torch.cuda.synchronize()
    assert _intact(fp, n, offset) and _intact(fg, n, offset) and _intact(fc, K * 3), "canary bytes around the outputs"
    return sp.cpu().numpy(), sg.cpu().numpy(), counts.cpu().numpy()


# ---- extract ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,K,kind,offset", [
    ((1, 1, 1), 1, "full", 0), ((9, 1, 20), 3, "blobs", 0), ((17, 12, 9), 7, "blobs", 0), ((5, 33, 7), 3, "symmetric", 0),
    ((9, 8, 12), 3, "blobs", 1),                      # Z % 4 == 0 at an odd address: byte stores
    ((6, 5, 8), 7, "full", 0), ((6, 5, 8), 1, "empty", 0), ((7, 6, 5), 3, "corners", 0), ((7, 6, 5), 3, "voxel", 0),
    ((1, EXTRACT_CAP_ITEMS + 1, 3), 3, "blobs", 0),    # one (x, y) row more than the capped grid has threads
    ((2, EXTRACT_CAP_ITEMS // 2 // 2 + 1, 8), 1, "blobs", 0),     # the same through the 32-bit stores
])
def test_surfaces_and_counts_equal_the_restatement(shape, K, kind, offset):
    pred, gt = _mask_pair(kind, shape, K, 100 + K)
    if kind == "blobs":
        pred |= np.uint8(0x80) * (np.arange(pred.size).reshape(shape) % 7 == 0).astype(np.uint8)      # bit 7 of a PREDICTION means nothing
        pred[..., 0] |= np.uint8(1 << K) if K < 7 else np.uint8(0)                                   # nor does a bit >= K
    prefill = np.arange(K * 3, dtype=np.int64).reshape(K, 3) * 1000 + 7
    sp, sg, counts = _extract_raw(pred, gt, K, prefill, offset)
    wp, wg, wc = R.surfaces(pred, gt, K)
    assert np.array_equal(sp, wp) and np.array_equal(sg, wg)
    assert np.array_equal(counts, prefill + wc), "the counts are ADDED to the row"
    assert not ((sp | sg) & 0x80).any()


# ---- the distance transform ------------------------------------------------------------------------------------------------------------
EDT_CASES = [
    ((1, 1, 1), "full", 0), ((9, 1, 20), "blobs", 1), ((17, 12, 9), "blobs", 2), ((5, 33, 7), "symmetric", 2), ((17, 12, 9), "voxel", 1),
    ((17, 12, 9), "corners", 2), ((6, 5, 8), "full", 2),
    ((5, 41, 20), "blobs", 2),             # Z pass: 4096 / 20 = 204 lines per tile, 205 lines
    ((3, 20, MAX_RUN + 1), "voxel", 2),     # Y pass: runs of 64 z, 65 z
    ((9, 5, 13), "corners", 1),            # X pass: runs of 64 (y, z), 65 of them
    ((27, 19, 3), "blobs", 1),             # Z pass: 513 lines of 3, 512 per tile
    ((12, 11, 10), "corners", 2), ((3, 9, 70), "blobs", 0),      # lines and whole tiles without a surface voxel next to ones that have some
    ((MAX_AXIS, 3, 3), "voxel", 2),        # the longest axis: runs of 8128 / 1024 = 7 (y, z), 9 of them
    ((3, MAX_AXIS, 3), "corners", 1), ((2, 2, MAX_AXIS), "voxel", 2), ((1, 5, MAX_AXIS), "blobs", 0),      # Z = 1024: 4 lines per tile, 5 lines
]


@pytest.mark.parametrize("shape,kind,si", EDT_CASES)
def test_d2_equals_the_restatement_bit_for_bit(shape, kind, si):
    from pcrlv2_amd import ops
    spacing = SPACINGS[si]
    pred, gt = _mask_pair(kind, shape, 2, 200)
    surf = R.surfaces(pred, gt, 2)[1]
    n = surf.size
    full, out = _guarded(shape, torch.float64)
    steps = torch.zeros(1, dtype=torch.int64, device="cuda")
    got = ops.edt_sq(_dev(surf), 1, spacing, out=out, steps=steps)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert _intact(full, n), "canary words around d2"
    want = R.edt_sq((surf >> 1 & 1).astype(bool), spacing)
    assert np.array_equal(out.cpu().numpy().view(np.int64), want.view(np.int64))
    assert 0 <= int(steps) <= 3 * n * max(shape)


def test_d2_of_an_empty_surface_is_inf_and_a_longer_axis_is_refused():
    from pcrlv2_amd import ops
    from pcrlv2_amd._lib import PcrlError, lib, stream_handle
    d2 = ops.edt_sq(torch.zeros((5, 9, 7), dtype=torch.uint8, device="cuda"), 0, (0.7, 0.7, 2.5))
    assert bool(torch.isinf(d2).all()) and bool((d2 > 0).all())
    other_bit = ops.edt_sq(torch.full((5, 9, 7), 0x7E, dtype=torch.uint8, device="cuda"), 0)
    assert bool(torch.isinf(other_bit).all())
    assert ops.edt_max_axis() == MAX_AXIS
    big = torch.zeros((2, MAX_AXIS + 1, 2), dtype=torch.uint8, device="cuda")
    with pytest.raises(PcrlError, match=f"at most {MAX_AXIS} voxels"):
        ops.edt_sq(big, 0)
    out = torch.empty(big.shape, dtype=torch.float64, device="cuda")
    with pytest.raises(PcrlError, match=rf"pcrl_edt_sq failed \(-1\).*at most {MAX_AXIS} voxels"):
        lib().call("pcrl_edt_sq", big, 0, out, 1.0, 1.0, 1.0, None, None, 0, *big.shape, stream_handle())


# ---- the statistics --------------------------------------------------------------------------------------------------------------------
def _check_record(rec, st, tag):
    assert int(rec[0]) == st["n_a"] and int(rec[1]) == st["n_b"], tag
    if st["d2"] is None:
        assert not rec[2:].any(), f"{tag}: only the counts are written when a surface is empty"
        return
    assert int(rec[2]) == st["lo"], tag
    assert rec[3:6].tolist() == np.array(st["d2"]).view(np.int64).tolist(), f"{tag}: order statistics {rec[3:6].view(np.float64)} against {st['d2']}"
    for slot, key, n in ((6, "sum_a", st["n_a"]), (7, "sum_b", st["n_b"])):
        got, want = float(rec[slot:slot + 1].view(np.float64)[0]), st[key]
        bound = (n + 2) * U * want
        print(f"[{tag}] {key}: error / bound = {abs(got - want) / bound if bound else 0.0:.3f} (n = {n})")
        assert abs(got - want) <= bound, (tag, key, got, want)


@pytest.mark.parametrize("V,q,levels", [(1000, 0.95, 7), (STATS_CAP + 1, 0.95, 1 << 40), (STATS_CAP + 1, 0.5, 3), (4097, 1.0, 50), (4097, 0.0, 50),
                                        (300, 0.37, 1)])
def test_selection_and_sums_on_synthetic_distances(V, q, levels):
    """The select on its own: d2 drawn from `levels` distinct values (few levels: long runs of equal values that it must count, not skip; 2^40: all
    distinct, every byte of the pattern in play), random masks."""
    from pcrlv2_amd import ops
    rng = np.random.default_rng(V + levels % 97)
    vals = rng.random(min(levels, 4 * V)) * 10.0 ** rng.integers(-3, 6, min(levels, 4 * V))
    d2a, d2b = vals[rng.integers(0, len(vals), V)], vals[rng.integers(0, len(vals), V)]
    ma, mb = (rng.random(V) < 0.3).astype(np.uint8) << 2, (rng.random(V) < 0.2).astype(np.uint8) << 2
    ma |= rng.integers(0, 2, V).astype(np.uint8)              # another class's bit
    shape = (1, 1, V)
    st = R.stats(d2a.reshape(shape), (ma >> 2 & 1).astype(bool).reshape(shape), d2b.reshape(shape), (mb >> 2 & 1).astype(bool).reshape(shape), q)
    full, rec = _guarded((8,), torch.int64)
    rec.zero_()
    args = (_dev(d2a.reshape(shape)), _dev(ma.reshape(shape)), _dev(d2b.reshape(shape)), _dev(mb.reshape(shape)), 2, q)
    ops.surf_dist_stats(*args, record=rec)
    torch.cuda.synchronize()
    assert _intact(full, 8)
    _check_record(rec.cpu().numpy(), st, f"synthetic V={V} q={q}")
    again = ops.surf_dist_stats(*args)
    assert torch.equal(again, rec), "two runs give identical bytes"


def test_two_values_one_value_and_none():
    from pcrlv2_amd import ops
    shape = (2, 3, 4)
    d2a, d2b = np.full(shape, 2.25), np.full(shape, 9.0)
    ma, mb = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    ma[0, 1, 2], mb[1, 2, 3] = 1, 1
    rec = ops.surf_dist_stats(_dev(d2a), _dev(ma), _dev(d2b), _dev(mb), 0, 1.0).cpu().numpy()      # n = 2, q = 1: lo == hi == n - 1 == 1
    assert rec[:3].tolist() == [1, 1, 1] and rec[3:].view(np.float64).tolist() == [9.0, 9.0, 9.0, 1.5, 3.0]
    rec = ops.surf_dist_stats(_dev(d2a), _dev(ma), _dev(d2b), _dev(mb), 0, 0.95).cpu().numpy()
    assert rec[:3].tolist() == [1, 1, 0] and rec[3:6].view(np.float64).tolist() == [2.25, 9.0, 9.0]
    pre = torch.full((8,), 77, dtype=torch.int64, device="cuda")                                   # n = 1: one surface is empty
    rec = ops.surf_dist_stats(_dev(np.full(shape, np.inf)), _dev(ma), _dev(d2b), _dev(np.zeros(shape, np.uint8)), 0, 0.95, record=pre).cpu().numpy()
    assert rec.tolist() == [1, 0, 77, 77, 77, 77, 77, 77]
    rec = ops.surf_dist_stats(_dev(d2a), _dev(mb * 0), _dev(d2b), _dev(mb * 0), 0).cpu().numpy()
    assert not rec.any()
    # 257 keys (more than one block) that agree in their seven leading bytes: only the last pass tells them apart, under one full prefix;
    # q = 0: ranks 0, 1 and n - 1 in one call; q = 1: all three ranks n - 1
    last = (np.uint64(0x4024000000000000) + (np.arange(257, dtype=np.uint64) * np.uint64(37)) % np.uint64(256)).view(np.float64).reshape(1, 1, 257)
    on, third, back = np.ones(last.shape, np.uint8), (np.arange(257) % 3 == 0).astype(np.uint8).reshape(last.shape), last[:, :, ::-1].copy()
    for q in (0.0, 1.0):
        for m_b in (third, on):      # the keys of one side and a third of the other's; every key twice
            st = R.stats(last, on.astype(bool), back, m_b.astype(bool), q)
            rec = ops.surf_dist_stats(_dev(last), _dev(on), _dev(back), _dev(m_b), 0, q).cpu().numpy()
            _check_record(rec, st, f"last byte q={q} n_b={int(m_b.sum())}")
            assert st["d2"][2] == last.max() and st["d2"][0] == (last.max() if q else last.min())


# ---- the chain and surface_metrics -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(shape, K, kind, si, q=0.95):
    pred, gt = _mask_pair(kind, shape, K, 300 + K)
    per, counts = R.class_stats(pred, gt, K, SPACINGS[si], q)
    return pred, gt, per, counts


CHAIN = [((1, 1, 1), 1, "full", 0), ((9, 1, 20), 3, "blobs", 1), ((17, 12, 9), 7, "blobs", 2), ((5, 33, 7), 3, "symmetric", 2),
         ((17, 12, 9), 3, "corners", 1), ((17, 12, 9), 3, "equal", 2), ((17, 12, 9), 1, "empty", 0), ((17, 12, 9), 3, "pred_only", 2),
         ((7, 6, 5), 3, "voxel", 2), ((6, 5, 8), 7, "full", 1), ((65, 64, 64), 1, "symmetric", 2)]


@pytest.mark.parametrize("shape,K,kind,si", CHAIN)
def test_records_of_the_whole_chain(shape, K, kind, si):
    from pcrlv2_amd import ops
    pred, gt, per, counts = _reference(shape, K, kind, si)
    spacing = SPACINGS[si]
    sp, sg, c = ops.surf_extract(_dev(pred), _dev(gt), K)
    assert np.array_equal(c.cpu().numpy(), counts)
    for k in range(K):
        d2g, d2p = ops.edt_sq(sg, k, spacing), ops.edt_sq(sp, k, spacing)
        rec = ops.surf_dist_stats(d2g, sp, d2p, sg, k, 0.95)
        _check_record(rec.cpu().numpy(), per[k], f"{kind} {shape} class {k}")
        assert torch.equal(ops.surf_dist_stats(ops.edt_sq(sg, k, spacing), sp, ops.edt_sq(sp, k, spacing), sg, k, 0.95), rec), "two runs, identical bytes"


@pytest.mark.parametrize("shape,K,kind,si", CHAIN)
def test_surface_metrics_against_the_restatement(shape, K, kind, si):
    from pcrlv2_amd.train_seg import surface_metrics
    pred, gt, per, counts = _reference(shape, K, kind, si)
    want = R.metrics_of(per)
    got = surface_metrics(_dev(pred), _dev(gt), K, SPACINGS[si])
    assert np.array_equal(got["counts"], counts) and got["counts"].dtype == np.int64
    assert got["n_pred"].tolist() == [st["n_a"] for st in per] and got["n_gt"].tolist() == [st["n_b"] for st in per]
    for key in ("hd95", "hd"):
        assert np.array_equal(got[key].view(np.int64), want[key].view(np.int64)), (key, got[key], want[key])
    for k, st in enumerate(per):
        if st["d2"] is None:
            assert (np.isnan(got["assd"][k]) and np.isnan(want["assd"][k])) or got["assd"][k] == want["assd"][k] == 0.0
            continue
        bound = (max(st["n_a"], st["n_b"]) + 2 + 4) * U * want["assd"][k]
        assert abs(got["assd"][k] - want["assd"][k]) <= bound, (k, got["assd"][k], want["assd"][k])
    if kind == "equal":
        assert all((got[key] == 0).all() for key in ("hd95", "hd", "assd"))
    if kind == "pred_only":
        assert all(np.isnan(got[key]).all() for key in ("hd95", "hd", "assd"))
    again = surface_metrics(_dev(pred), _dev(gt), K, SPACINGS[si])
    assert all(np.array_equal(got[key], again[key], equal_nan=True) for key in got)


# ---- seg3d.py score, end to end --------------------------------------------------------------------------------------------------------
def test_score_end_to_end_against_the_restatement(tmp_path):
    K, shape = 3, (17, 12, 9)
    data, pdir = tmp_path / "data", tmp_path / "pred"
    os.makedirs(data), os.makedirs(pdir)
    cases = {}
    for i, name in enumerate(("one", "two", "three")):
        pred, gt = _mask_pair("blobs", shape, K, 400 + 10 * i)
        big_p, big_g = np.zeros((24, 20, 16), np.uint8), np.full((24, 20, 16), 0, np.uint8)
        big_p[3:20, 5:17, 2:11], big_g[3:20, 5:17, 2:11] = pred, gt            # the bounding-box crop has something to cut
        if name == "two":
            big_g &= 0xFD                                                      # class 1: no ground truth
        spacing = (1.0, 1.0, 1.0)
        if name == "three":
            spacing = (0.7, 0.7, 2.5)
            np.save(data / "three_spacing.npy", np.array(spacing))
        np.save(data / f"{name}_seg.npy", big_g), np.save(pdir / f"{name}_pred.npy", big_p)
        cases[name] = (big_p, big_g, spacing)
    (data / "list.txt").write_text("one\ntwo\nthree\n")
    csv = tmp_path / "scores.csv"
    r = subprocess.run([sys.executable, "seg3d.py", "score", "--data", str(data), "--list", "list.txt", "--pred", str(pdir), "--n_class", str(K),
                        "--csv", str(csv)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 4 and lines[-1].startswith("Score: 3 cases") and lines[2].startswith("three\tspacing 0.7,0.7,2.5")
    text = csv.read_text().splitlines()
    assert text[0] == "case,class,dice,hd95,hd,assd,n_pred,n_gt" and len(text) == 1 + 3 * K
    row = 1
    for name, (p, g, spacing) in cases.items():
        want = R.metrics(p, g, K, spacing)
        for k in range(K):
            f = text[row].split(",")
            row += 1
            assert f[:2] == [name, str(k)] and int(f[6]) == want["n_pred"][k] and int(f[7]) == want["n_gt"][k]
            tp, np_, ng = want["counts"][k].tolist()
            assert float(f[2]) == (1.0 if np_ + ng == 0 else 2.0 * tp / (np_ + ng))
            if np.isnan(want["hd95"][k]):
                assert f[3:6] == ["nan", "nan", "nan"] and (name, k) == ("two", 1)
                continue
            assert float(f[3]) == want["hd95"][k] and float(f[4]) == want["hd"][k]
            n = max(want["n_pred"][k], want["n_gt"][k])
            assert abs(float(f[5]) - want["assd"][k]) <= (n + 2 + 4) * U * want["assd"][k]
    assert "class 1: Dice" in lines[-1] and "(2)" in lines[-1].split("class 1:")[1].split("class 2:")[0]
