"""pcrl_ccl_label, pcrl_ccl_filter (csrc/components.hip), ops.label_components / filter_components, train_seg.postprocess_mask, `seg3d.py postprocess`
and the clean-up options of `predict` on the device.

EQUAL, bit for bit, to tests/components_reference.py: labels == scipy.ndimage.label(...)[0] with no canonicalisation (both number the components by
the ascending C-order index of their first voxel), sizes == np.bincount, n; the filtered masks == filter_ref / postprocess_ref.  Everything is
integer, so there is no tolerance anywhere.
Shapes come from the tile (tx, ty, tz) that pcrl_ccl_tile reports (4 x 4 x 64 today): one voxel, one Z-run and one voxel, exactly one tile, one less
and one more than a tile along each axis, two tiles and one voxel along every axis, (33, 34, 35), and (96, 96, 80).
Caps (csrc/components.hip): the tile grid is one block per tile (24 x 24 x 2 = 1152 at the last shape) up to 2^20 blocks, beyond which a block walks
several tiles -- a launch takes fewer than 2^32 threads in all, and a tile of a thin volume holds as few as 4 real voxels: (tx 2^20 + 5, 1, 1) has
two tiles more than the cap, and (2^26, 1, 1), 2^24 tiles, is the size at which an uncapped grid of 256-thread blocks reaches 2^32 threads; the
per-voxel grids are one thread per voxel (fewer than 2^31); the flatten and rank kernels work on chunks of 1024 consecutive voxels (720 at the last shape, against 1 to 39 at the others), and
the one-block scan of the chunk sums walks them in strips of 256 chunks: 720 chunks are three strips, the last one partial.  The winner of
keep_largest is reduced by one block of 256 threads, thread t looking at sizes[t], sizes[t + 256], ...: noise at the last shape has tens of
thousands of components.  Voxel indices are 32-bit: X * Y * Z >= 2^31 is refused on the host (test_components_cpu.py).
"""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import components_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

CONNS = (6, 18, 26)
GUARD = 64
CANARY8, CANARY32 = 0xA5, 0x5A5A5A5A


def _tile():
    """pcrl_ccl_tile is a host function: the parametrisation asks the library (built first where it is not there yet)."""
    from pcrlv2_amd import _lib, ops
    if not os.path.exists(_lib.LIBPATH):
        import __graft_entry__ as g
        g.build()
    return ops.ccl_tile()


def _shapes():
    tx, ty, tz = _tile()
    return [(1, 1, 1), (1, 1, tz + 1), (tx, ty, tz), (tx - 1, ty, tz), (tx + 1, ty, tz), (tx, ty - 1, tz), (tx, ty + 1, tz), (tx, ty, tz - 1),
            (tx, ty, tz + 1), (2 * tx + 1, 2 * ty + 1, 2 * tz + 1), (33, 34, 35), (96, 96, 80)]


SHAPES = _shapes()
SMALL = [SHAPES[2], SHAPES[9], SHAPES[10]]
MAX_BLOCKS = 1 << 20          # CCL_MAX_BLOCKS: the tile grid's cap


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(n, dtype, offset=0):
    """A canary-filled buffer and a view of n elements inside it, GUARD (+ offset, uint8 only) elements from its start."""
    full = torch.empty(n + 2 * GUARD + offset, dtype=dtype, device="cuda")
    full.fill_(CANARY8 if dtype == torch.uint8 else CANARY32)
    return full, full[GUARD + offset:GUARD + offset + n]


def _intact(full, n, offset=0, written=None):
    """The guards on both sides, and (written: elements of the view that may have changed) the rest of the view."""
    want = CANARY8 if full.dtype == torch.uint8 else CANARY32
    lo = GUARD + offset
    return bool((full[:lo] == want).all()) and bool((full[lo + (n if written is None else written):] == want).all())


def _masks(shape):
    """Every generator of the issue -> [(name, bool array, bit)]; the bit rotates through 0, 3, 6, and noise 0.3 runs at all three."""
    out = [("blobs", R.blobs(shape, 1)), ("noise0.1", R.noise(shape, 0.1, 2)), ("noise0.3", R.noise(shape, 0.3, 3)), ("noise0.5", R.noise(shape, 0.5, 4)),
           ("checker", R.checker(shape)), ("corner_lattice", R.corner_lattice(shape)), ("snake", R.snake(shape)), ("comb", R.comb(shape)),
           ("empty", R.empty(shape)), ("full", R.full(shape))]
    if max(shape) >= 3:
        out.append(("twins", R.twins(shape)))
    out += [(f"corner{i}", R.corner(shape, i)) for i in range(8)]
    with_bits = [(name, b, (0, 3, 6)[i % 3]) for i, (name, b) in enumerate(out)]
    return with_bits + [("noise0.3", out[2][1], 0), ("noise0.3", out[2][1], 6)]


def _label_raw(mask, bit, conn, offset=0):
    """pcrl_ccl_label with every output inside canary guards and the mask `offset` bytes off its allocation -> (labels, sizes[:n], n) on the host."""
    from pcrlv2_amd import ops
    from pcrlv2_amd._lib import lib, stream_handle
    shape, V = mask.shape, mask.size
    cap = (V + 1) // 2
    holder = torch.empty(V + offset, dtype=torch.uint8, device="cuda")
    m = holder[offset:]
    m.copy_(_dev(mask).reshape(-1))
    fl, labels = _guarded(V, torch.int32)
    fs, sizes = _guarded(cap, torch.int32)
    fn, n = _guarded(1, torch.int32)
    nb = lib().call("pcrl_ccl_ws_bytes", *shape)
    lib().call("pcrl_ccl_label", m, bit, conn, labels, sizes, n, ops.workspace(nb, m.device), nb, *shape, stream_handle())
    torch.cuda.synchronize()
    count = int(n)
    assert 0 <= count <= cap
    assert _intact(fl, V) and _intact(fn, 1) and _intact(fs, cap, written=count), "canary words around labels, n and sizes, and in sizes from n on"
    return labels.cpu().numpy().reshape(shape), sizes[:count].cpu().numpy(), count


# ---- labelling ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", CONNS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_labels_sizes_and_n_equal_scipy_bit_for_bit(shape, conn):
    counts = []
    for i, (name, b, bit) in enumerate(_masks(shape)):
        mask = R.embed(b, bit, seed=10 + i)
        want_l, want_s, want_n = R.label_ref(mask, bit, conn)
        stated = R.expected_count(name, shape, conn)
        assert stated is None or stated == want_n, (name, stated, want_n)
        offset = (0, 1, 3)[i % 3]
        got_l, got_s, got_n = _label_raw(mask, bit, conn, offset)
        tag = f"{name} {shape} bit {bit} connectivity {conn} offset {offset}"
        assert got_n == want_n, tag
        assert got_s.dtype == np.int32 and np.array_equal(got_s, want_s), tag
        assert got_l.dtype == np.int32 and np.array_equal(got_l, want_l), tag
        again = _label_raw(mask, bit, conn, offset)
        assert again[2] == got_n and np.array_equal(again[0], got_l) and np.array_equal(again[1], got_s), f"{tag}: two runs, identical bytes"
        counts.append(f"{name}/{bit}: {got_n}")
    print(f"[ccl {shape} connectivity {conn}] components " + ", ".join(counts))


@pytest.mark.parametrize("shape,conn", [((_tile()[0] * MAX_BLOCKS + 5, 1, 1), 6), ((_tile()[0] * MAX_BLOCKS + 5, 1, 1), 18),
                                        ((_tile()[0] * MAX_BLOCKS + 5, 1, 1), 26), ((1 << 26, 1, 1), 6)], ids=lambda v: str(v).replace(" ", ""))
def test_thin_volumes_with_more_tiles_than_the_grid_cap(shape, conn):
    from pcrlv2_amd import ops
    tx, ty, tz = _tile()
    assert -(-shape[0] // tx) > MAX_BLOCKS
    mask = R.embed(R.noise(shape, 0.5, 11), 3, 12)
    mask[-3:] |= 8          # the last, partial tile holds a run
    labels, sizes = ops.label_components(_dev(mask), 3, conn)
    want_l, want_s, want_n = R.label_ref(mask, 3, conn)
    assert sizes.numel() == want_n and np.array_equal(sizes.cpu().numpy(), want_s) and np.array_equal(labels.cpu().numpy(), want_l)


@pytest.mark.parametrize("conn", CONNS)
def test_label_components_returns_the_view_of_n_sizes(conn):
    from pcrlv2_amd import ops
    shape = SHAPES[10]
    mask = R.embed(R.noise(shape, 0.3, 7), 3, 8)
    labels, sizes = ops.label_components(_dev(mask), 3, conn)
    want_l, want_s, want_n = R.label_ref(mask, 3, conn)
    assert labels.dtype == torch.int32 and tuple(labels.shape) == shape and sizes.dtype == torch.int32 and tuple(sizes.shape) == (want_n,)
    assert np.array_equal(labels.cpu().numpy(), want_l) and np.array_equal(sizes.cpu().numpy(), want_s)
    l0, s0 = ops.label_components(torch.zeros(shape, dtype=torch.uint8, device="cuda"), 0, conn)
    assert s0.numel() == 0 and not bool(l0.any())


# ---- filtering ----------------------------------------------------------------------------------------------------------------------------
RULES = [(True, 0), (False, 5), (True, 5), (False, 0)]


@pytest.mark.parametrize("conn", CONNS)
@pytest.mark.parametrize("shape", SMALL + [SHAPES[11]], ids=lambda s: "x".join(map(str, s)))
def test_filter_components_equals_the_reference(shape, conn):
    from pcrlv2_amd import ops
    for i, (name, b) in enumerate((("twins", R.twins(shape)), ("noise0.3", R.noise(shape, 0.3, 5)), ("noise0.1", R.noise(shape, 0.1, 6)), ("empty", R.empty(shape)))):
        bit = (0, 3, 6)[i % 3]
        mask = R.embed(b, bit, seed=20 + i)
        want_l, want_s, _ = R.label_ref(mask, bit, conn)
        dm = _dev(mask)
        labels, sizes = ops.label_components(dm, bit, conn)
        for largest, mv in RULES:
            mv = mv if name != "twins" else (int(want_s.max()) + (1 if largest else 0) if mv else 0)      # at the twins' size it keeps them, one more drops them
            got = ops.filter_components(dm, labels, sizes, bit, keep_largest=largest, min_voxels=mv)
            assert got.data_ptr() != dm.data_ptr() and got.dtype == torch.uint8
            want = R.filter_ref(mask, want_l, want_s, bit, largest, mv)
            assert np.array_equal(got.cpu().numpy(), want), (name, shape, conn, largest, mv)
            assert np.array_equal(dm.cpu().numpy(), mask), "the input mask is not written"
        if name == "twins":
            kept = ops.filter_components(dm, labels, sizes, bit, keep_largest=True).cpu().numpy() >> bit & 1
            assert np.array_equal(kept.astype(bool), want_l == 1), "the tie goes to the lowest label"


def test_filter_output_sits_inside_intact_guards_at_an_odd_offset():
    from pcrlv2_amd import ops
    from pcrlv2_amd._lib import lib, stream_handle
    shape = SHAPES[9]
    V = int(np.prod(shape))
    mask = R.embed(R.noise(shape, 0.3, 9), 6, 9)
    labels, sizes = ops.label_components(_dev(mask), 6, 18)
    n = torch.tensor([sizes.numel()], dtype=torch.int32, device="cuda")
    want_l, want_s, _ = R.label_ref(mask, 6, 18)
    for offset in (0, 1):
        holder = torch.empty(V + offset, dtype=torch.uint8, device="cuda")
        holder[offset:].copy_(_dev(mask).reshape(-1))
        full, out = _guarded(V, torch.uint8, offset)
        nb = lib().call("pcrl_ccl_filter_ws_bytes")
        lib().call("pcrl_ccl_filter", holder[offset:], labels, sizes, n, out, 6, 1, 3, ops.workspace(nb, out.device), nb, *shape, stream_handle())
        torch.cuda.synchronize()
        assert _intact(full, V, offset)
        assert np.array_equal(out.cpu().numpy().reshape(shape), R.filter_ref(mask, want_l, want_s, 6, True, 3))


# ---- postprocess_mask and the command line ---------------------------------------------------------------------------------------------------
def _prediction(shape, seed):
    """Three classes: blobs with specks around them."""
    m = np.zeros(shape, np.uint8)
    for k in range(3):
        m |= (R.blobs(shape, seed + k, n=3) | R.noise(shape, 0.02, seed + 10 + k)).astype(np.uint8) << k
    return m


@pytest.mark.parametrize("conn", CONNS)
@pytest.mark.parametrize("keep,mv", [((0, 2), 0), ((0, 2), 4), ((), 3)])
def test_postprocess_mask_equals_the_reference(keep, mv, conn):
    from pcrlv2_amd.train_seg import postprocess_mask
    shape = (33, 34, 35)
    mask = _prediction(shape, 30)
    got, report = postprocess_mask(_dev(mask), 3, keep, mv, conn)
    want = R.postprocess_ref(mask, 3, keep, mv, conn)
    assert np.array_equal(got.cpu().numpy(), want)
    for k in range(3):
        if k not in keep and mv == 0:
            assert report[k] == {"before": None, "after": None, "removed": 0} and np.array_equal(want >> k & 1, mask >> k & 1)
            continue
        assert report[k]["before"] == R.label_ref(mask, k, conn)[2] and report[k]["after"] == R.label_ref(want, k, conn)[2]
        assert report[k]["removed"] == int((mask >> k & 1).sum()) - int((want >> k & 1).sum())


def test_postprocess_end_to_end_against_the_reference(tmp_path):
    pdir, out = tmp_path / "pred", tmp_path / "clean"
    os.makedirs(pdir)
    cases = {name: _prediction(shape, 40 + i) for i, (name, shape) in enumerate((("one", (17, 12, 9)), ("two", (9, 10, 70)), ("three", (5, 5, 5))))}
    cases["three"][:] &= 0x02          # classes 0 and 2 are empty there
    for name, m in cases.items():
        np.save(pdir / f"{name}_pred.npy", m)
    (tmp_path / "list.txt").write_text("one\ntwo\nthree\n")
    r = subprocess.run([sys.executable, "seg3d.py", "postprocess", "--pred", str(pdir), "--list", str(tmp_path / "list.txt"), "--out", str(out), "--n_class", "3",
                        "--keep_largest", "0,2", "--min_voxels", "3", "--connectivity", "18"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 4 and lines[0].startswith("one\tclass 0: components ") and lines[-1].startswith("Postprocess: 3 cases, connectivity 18\tclass 0: ")
    for name, m in cases.items():
        got = np.load(out / f"{name}_pred.npy")
        assert got.dtype == np.uint8 and np.array_equal(got, R.postprocess_ref(m, 3, (0, 2), 3, 18)), name
        assert np.array_equal(np.load(pdir / f"{name}_pred.npy"), m), "the predictions are left alone"


# ---- predict ------------------------------------------------------------------------------------------------------------------------------
def test_predict_cleans_on_request_and_writes_todays_bytes_otherwise(tmp_path):
    from pcrlv2_amd import data_seg as D
    from pcrlv2_amd import train_seg as T
    from pcrlv2_amd.models import Segmenter3d
    data = str(tmp_path / "data")
    D.write_synthetic(data, ["p0", "p1"], (40, 36, 20), 3, seed=9)
    with open(os.path.join(data, "two.txt"), "w") as f:
        f.write("p0\np1\n")
    # a randomly initialised segmenter answers all-or-nothing per class; its output biases are moved to the 50 %, 80 % and 95 % quantiles of its own
    # logits on one patch, so that every class is a ragged mask with specks
    torch.manual_seed(3)
    fresh = Segmenter3d(3).cuda()
    patch = torch.from_numpy(D.cut(D.open_case(data, "p0", 3, 1, need_seg=False), (0, 0, 0), (32, 32, 16))[0][None]).cuda()
    z = fresh.infer_logits(patch).reshape(-1, 3)
    with torch.no_grad():
        fresh.out_tr.final_conv.bias -= torch.stack([torch.quantile(z[:, k], q) for k, q in enumerate((0.5, 0.8, 0.95))])
    weights = str(tmp_path / "random.pt")
    torch.save({"state_dict": {k: v.cpu() for k, v in fresh.state_dict().items()}}, weights)
    changed = 0
    base = dict(data=data, list="two.txt", weights=weights, crop="32,32,16", b=4, amp=False, gpu=0)
    quiet = lambda *a: None      # noqa: E731
    model, crop = T.load_segmenter(weights, torch.device("cuda", 0)), (32, 32, 16)
    for tag, extra in (("tiled", {}), ("blended", {"overlap": 0.5, "window": "gaussian", "probs": False})):
        plain, clean = str(tmp_path / f"{tag}_plain"), str(tmp_path / f"{tag}_clean")
        assert T.predict(types.SimpleNamespace(out=plain, **base, **extra), log=quiet) == 2          # the namespace `predict` got before the options existed
        T.predict(types.SimpleNamespace(out=clean, keep_largest="all", min_voxels=8, connectivity=6, **base, **extra), log=quiet)
        for name in ("p0", "p1"):
            case = D.open_case(data, name, 3, 1, need_seg=False)
            case.seg = None
            before = (T.sliding_window(model, case, crop, 4, 0.5, "gaussian")[0].cpu().numpy() if extra else T.predict_case(model, case, crop, 4))
            raw = np.load(os.path.join(plain, name + "_pred.npy"))
            assert raw.dtype == np.uint8 and np.array_equal(raw, before), f"{tag} {name}: without the options, what predict wrote before they existed"
            got = np.load(os.path.join(clean, name + "_pred.npy"))
            assert got.dtype == np.uint8 and np.array_equal(got, R.postprocess_ref(raw, 3, (0, 1, 2), 8, 6)), (tag, name)
            print(f"[predict {tag} {name}] voxels per class before {[int((raw >> k & 1).sum()) for k in range(3)]} after {[int((got >> k & 1).sum()) for k in range(3)]}")
            changed += int(not np.array_equal(raw, got))
    assert changed == 4, "every prediction had something to clean"
