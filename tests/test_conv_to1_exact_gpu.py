"""3D path: the convolutions with ONE output channel (pcrl_conv3d_to1_fwd, _dgrad, _wgrad: the deep-supervision heads, final_conv and the segmentation
head's per-class products) bit for bit against float64 torch on exactly summable operands.  Method: tests/exact_lattice.py; cases, references and
route mirrors: tests/conv1_cases.py, whose preconditions and constant crossings tests/test_conv1_cases_cpu.py asserts on the CPU.

Every comparison is on bits at every element (float32 outputs against the float64 value, bf16 outputs against its round-to-nearest-even rounding),
outputs are pre-filled with NaN, hooks are restored in `finally`, and every test asserts the route that ran before it compares.  Statistics rows
are compared ROW BY ROW against the float64 sums of the row's own voxels (a 4x8x8 brick, or 1024 consecutive voxels): sum y on both lattices,
sum y^2 on the ternary one."""
import pytest
import torch

import conv1_cases as K
import exact_lattice as X

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
DEV = "cuda"
BRICK = {"d": 4, "h": 8, "w": 8}
NAN = float("nan")


def _act(t, dt):
    from pcrlv2_amd import ops
    return ops.to_act(t.to(dt).to(DEV), dt)


def _f32(t):
    return t.float().to(DEV).contiguous()


def _nan(shape, dt=F32):
    return torch.full(tuple(shape) if not isinstance(shape, int) else (shape,), NAN, dtype=dt, device=DEV)


def _nan_act(N, D, H, W, C, dt):
    from pcrlv2_amd import ops
    a = ops.new_act(N, D, H, W, C, dt, DEV)
    a.fill_(NAN)
    return a


def _ws(nb):
    return torch.empty(max(int(nb), 1), dtype=torch.uint8, device=DEV)


def _untouched(*outs):
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs), "a rejected call wrote its output"


# ---------------------------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------------------------
def _run_fwd(c, R, with_stats=True):
    """-> (y [M] float32, statistics rows [rows, 2]); the route is asserted from the row count, the workspace and the mirrored predicates"""
    from pcrlv2_amd._lib import dtype_code, lib, stream_handle
    L, dc, M = lib(), dtype_code(c.dt), K.voxels(c.vol)
    L.debug_set_conv_impl(c.impl)
    try:
        rows = L.call("pcrl_conv3d_to1_stats_rows", *c.vol, c.C, c.taps, dc)
        brick = c.route in (K.FWD_BRICK, K.FWD_BRICK_PACKED)
        assert rows == K.to1_stats_rows(c.vol, c.C, c.taps, c.dt, c.impl) == (K.nbricks(c.vol) if brick else -(-M // K.TO1_VOX))
        nb = L.call("pcrl_conv3d_to1_fwd_ws_bytes", *c.vol, c.C, c.taps) if c.ws else 0
        assert not c.ws or nb > 0
        assert c.route == K.to1_fwd_route(c.vol, c.C, c.taps, c.dt, nb > 0, c.impl), f"expected {c.route}"
        y, part = _nan(M), _nan(rows * 2)
        L.call("pcrl_conv3d_to1_fwd", _act(R.x, c.dt), _f32(R.w), _f32(R.b) if c.bias else None, y, part if with_stats else None,
               _ws(nb) if c.ws else None, nb, *c.vol, c.C, c.taps, dc, stream_handle())
        torch.cuda.synchronize()
    finally:
        L.debug_set_conv_impl(0)
    return y, part.view(rows, 2)


@pytest.mark.parametrize("c", K.fwd_cases(), ids=K.fwd_id)
def test_to1_fwd(c):
    """Output and statistics rows of every forward kernel: the direct gather (general loop: lanes striding over the channel vectors with and without a
    remainder, lpv = 1 and the cap of 64; the 1-tap fast path through a second, partial block), the two-pass form (pack, pointwise planes, shifted sum;
    one row and a second row of 56 voxels), the brick kernel with and without the packed weight image, and the two-pass form on the brick volumes
    under conv_impl = 1."""
    brick = c.route in (K.FWD_BRICK, K.FWD_BRICK_PACKED)
    for lat in ("fine", "ternary"):
        R = K.to1_reference(c.vol, c.C, c.taps, lat, c.bias)
        y, st = _run_fwd(c, R)
        what = f"to1 fwd {K.fwd_id(c)} [{lat}] route: {c.route}"
        X.assert_bit_equal(y.view(c.vol[0], 1, *c.vol[1:]), R.y, F32, what, brick=BRICK if brick else None)
        S = K.stats_reference(R, brick)
        X.assert_bit_equal(st[:, 0], S[:, 0], F32, what + " statistics rows: sum y")
        if lat == "ternary":
            X.assert_bit_equal(st[:, 1], S[:, 1], F32, what + " statistics rows: sum y^2")
        else:
            assert not bool(torch.isnan(st).any()), what + ": a statistics row was not written"
    y2, _ = _run_fwd(c, R, with_stats=False)      # stats_partial = NULL
    assert torch.equal(y2, y), f"to1 fwd {K.fwd_id(c)}: the output without statistics differs"


@pytest.mark.parametrize("vol", K.BRICK_VOLS, ids=K.vid)
@pytest.mark.parametrize("C", [32, 96, 128, 160, 512])
def test_to1_brick_forms_agree(vol, C):
    """The brick kernel with the packed weight image (staged once per call) and without it (converted in every block): the same MFMAs in the same order --
    outputs and BOTH statistics columns equal in bits on the fine lattice too, where sum y^2 has no exact reference."""
    cs = [c for c in K.fwd_cases() if (c.vol, c.C, c.impl) == (vol, C, 0)]
    assert sorted(c.route for c in cs) == sorted([K.FWD_BRICK, K.FWD_BRICK_PACKED])
    R = K.to1_reference(vol, C, 27, "fine")
    (y0, s0), (y1, s1) = (_run_fwd(c, R) for c in cs)
    assert torch.equal(y0, y1) and torch.equal(s0, s1)


@pytest.mark.parametrize("dt", [F32, BF], ids=K.dname)
def test_to1_fwd_rejections(dt):
    """Host-side checks only, nothing is launched: taps, channel multiples, the LDS limit (27 taps x C float32 weights must fit the 64 KiB a launch gets
    without opting in: C <= 606), dtype, null pointers."""
    from pcrlv2_amd._lib import PcrlError, dtype_code, lib, stream_handle
    L, dc, st = lib(), dtype_code(dt), stream_handle()
    vol, C = (1, 3, 5, 7), 1024
    M = K.voxels(vol)
    x, w, b = torch.zeros(M * C, dtype=dt, device=DEV), torch.zeros(27 * C, dtype=F32, device=DEV), torch.zeros(1, dtype=F32, device=DEV)
    y, dx = _nan(M), _nan(M * C, dt)
    dy = torch.zeros(M, dtype=F32, device=DEV)
    bad = [dict(taps=3), dict(C=K.vec(dt) // 2 * 3), dict(C=0), dict(C=1024 + K.vec(dt)), dict(C=608), dict(C=1024), dict(dtype=7)]
    for kw in bad + [dict(x=None), dict(w=None), dict(y=None)]:
        a = dict(x=x, w=w, y=y, C=64, taps=27, dtype=dc)
        a.update(kw)
        assert kw not in bad or "dtype" in kw or not K.to1_accepts(a["C"], a["taps"], dt), kw
        with pytest.raises(PcrlError):
            L.call("pcrl_conv3d_to1_fwd", a["x"], a["w"], b, a["y"], None, None, 0, *vol, a["C"], a["taps"], a["dtype"], st)
    for kw in bad + [dict(dy=None), dict(w=None), dict(dx=None)]:
        a = dict(dy=dy, w=w, dx=dx, C=64, taps=27, dtype=dc)
        a.update(kw)
        with pytest.raises(PcrlError):
            L.call("pcrl_conv3d_to1_dgrad", a["dy"], a["w"], None, a["dx"], *vol, a["C"], a["taps"], a["dtype"], st)
    _untouched(y, dx)
    assert K.to1_accepts(1024, 1, dt) and K.to1_accepts(600, 27, dt)      # what stays accepted runs in test_to1_fwd / test_to1_dgrad (C = 600) and below
    L.call("pcrl_conv3d_to1_fwd", x, w, b, y, None, None, 0, *vol, 1024, 1, dc, st)
    torch.cuda.synchronize()
    assert bool((y == 0).all())


# ---------------------------------------------------------------------------------------------------------------------------------------
# data gradient
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", K.dgrad_cases(), ids=K.dgrad_id)
def test_to1_dgrad(c):
    """dx = add_src + sum_t dy[m - delta_t] w[c][t] with add_src NULL, another tensor, and dx itself (the documented in-place form); 27 taps and 1;
    channel-vector counts that are no power of two; and M C / vec past 8192 * 256, where the grid-stride loop takes a second pass."""
    from pcrlv2_amd._lib import dtype_code, lib, stream_handle
    N, D, H, W = c.vol
    R = K.to1_dgrad_reference(c.vol, c.C, c.taps)
    blocks, passes = K.dgrad_passes(c.vol, c.C, c.dt)
    assert (passes > 1) == (c.vol == K.V_DGRAD_CAP)
    dx = _act(R.add, c.dt).clone() if c.add == "inplace" else _nan_act(N, D, H, W, c.C, c.dt)
    add = None if c.add == "none" else dx if c.add == "inplace" else _act(R.add, c.dt)
    lib().call("pcrl_conv3d_to1_dgrad", _f32(R.dy), _f32(R.w), add, dx, N, D, H, W, c.C, c.taps, dtype_code(c.dt), stream_handle())
    X.assert_bit_equal(dx, R.dx if c.add == "none" else R.dx_add, c.dt, f"to1 dgrad {K.dgrad_id(c)} ({blocks} blocks, {passes} grid-stride passes)")


# ---------------------------------------------------------------------------------------------------------------------------------------
# weight and bias gradient
# ---------------------------------------------------------------------------------------------------------------------------------------
def _wgrad_need(L, c):
    """bytes the route that runs asks for (pcrl_conv3d_to1_wgrad_ws_bytes sizes for the largest form of the shape)"""
    M = K.voxels(c.vol)
    if c.route == K.WG_BRICK:
        return K.scalar_brick_ws_bytes(c.vol, c.C)
    if c.route == K.WG_POINTWISE:
        return 8192 + L.call("pcrl_colsum_ws_bytes", M, c.C)
    return K.plain_ws_bytes(M, c.C, 2 if c.dt == BF else 4)


def _run_wgrad(c, x, dy):
    """-> (dw [C, taps], db [1]) under the case's hooks; the route query is asserted, and a workspace one byte short of what the route needs is rejected first"""
    from pcrlv2_amd._lib import PcrlError, dtype_code, lib, stream_handle
    L, dc = lib(), dtype_code(c.dt)
    L.debug_set_wgrad_impl(c.impl)
    L.debug_set_wgrad_tr(c.tr)
    try:
        route = L.call("pcrl_conv3d_to1_wgrad_route", *c.vol[1:], c.C, c.taps, dc)
        assert route == c.route == K.scalar_wgrad_route(c.vol, c.C, c.taps, c.dt, c.impl, c.tr), f"route {route}, expected {c.route}"
        nb, need = L.call("pcrl_conv3d_to1_wgrad_ws_bytes", *c.vol, c.C, c.taps), _wgrad_need(L, c)
        assert need <= nb
        dw, db, ws = _nan((c.C, c.taps)), _nan(1), _ws(nb)
        with pytest.raises(PcrlError):
            L.call("pcrl_conv3d_to1_wgrad", x, dy, dw, db, ws, need - 1, *c.vol, c.C, c.taps, dc, stream_handle())
        _untouched(dw, db)
        L.call("pcrl_conv3d_to1_wgrad", x, dy, dw, db, ws, nb, *c.vol, c.C, c.taps, dc, stream_handle())
        torch.cuda.synchronize()
    finally:
        L.debug_set_wgrad_impl(0)
        L.debug_set_wgrad_tr(1)
    return dw, db


@pytest.mark.parametrize("c", K.wgrad_cases(), ids=K.wgrad_id)
def test_to1_wgrad(c):
    """dw[c][t] = sum_m x[m][c] dy[m - delta_t] and db = sum dy: the scalar brick kernel with one and two bricks per block and an uneven last block;
    the im2col + plain GEMM route under wgrad_impl = 1, under wgrad_tr = 0, in float32 and on a non-brick volume; the 1-tap weighted column sum --
    all against the same reference."""
    R = K.to1_reference(c.vol, c.C, c.taps, "fine")
    dw, db = _run_wgrad(c, _act(R.x, c.dt), _f32(R.dy).view(-1))
    what = f"to1 wgrad {K.wgrad_id(c)} route {c.route}"
    X.assert_bit_equal(dw, R.dw.reshape(c.C, c.taps), F32, what)
    X.assert_bit_equal(db, R.db, F32, what + " bias gradient")


@pytest.mark.parametrize("c", K.BIG_WG, ids=K.wgrad_id)
def test_to1_wgrad_past_the_block_caps(c):
    """vecsum_partial_kernel past its 1024 blocks (M > 1024 * 4096, through the 1-tap column sum) and im2col27_kernel past its 16384 blocks
    (M > 16384 * 256 / 4 in bf16): generated on the device on the ternary lattice, restated there in float64."""
    N, D, H, W = c.vol
    M = K.voxels(c.vol)
    assert N == 1 and (K.vecsum_passes(M)[0] == K.VECSUM_CAP if c.taps == 1 else K.im2col_passes(M, c.dt)[1] == 2)
    lat = X.TERNARY
    x = K.device_lattice((M, c.C), *lat["x"], c.dt, 11, DEV)
    dy = K.device_lattice((M,), *lat["dy"], F32, 12, DEV)
    dw, db = _run_wgrad(c, x, dy)
    want_dw, want_db = K.to1_wgrad_restated(x, dy.view(D, H, W), c.taps)
    X.assert_exactly_summable(K.to1_wgrad_restated(x.abs(), dy.abs().view(D, H, W), c.taps)[0], 1.0, f"to1 wgrad {K.wgrad_id(c)}")
    X.assert_bit_equal(dw, want_dw.cpu(), F32, f"to1 wgrad {K.wgrad_id(c)} route {c.route}")
    X.assert_bit_equal(db, want_db.cpu(), F32, f"to1 wgrad {K.wgrad_id(c)} bias gradient")


@pytest.mark.parametrize("dt", [F32, BF], ids=K.dname)
def test_to1_wgrad_rejections(dt):
    from pcrlv2_amd._lib import PcrlError, dtype_code, lib, stream_handle
    L, dc, st = lib(), dtype_code(dt), stream_handle()
    vol, C = (1, 3, 5, 7), 64
    M = K.voxels(vol)
    x, dy = torch.zeros(M * C, dtype=dt, device=DEV), torch.zeros(M, dtype=F32, device=DEV)
    dw, db = _nan(C * 27), _nan(1)
    nb = L.call("pcrl_conv3d_to1_wgrad_ws_bytes", *vol, C, 27)
    ws = _ws(nb)
    for kw in (dict(taps=3), dict(C=12), dict(C=0), dict(dtype=7), dict(x=None), dict(dy=None), dict(dw=None), dict(db=None), dict(ws=None), dict(nb=0)):
        a = dict(x=x, dy=dy, dw=dw, db=db, ws=ws, nb=nb, C=C, taps=27, dtype=dc)
        a.update(kw)
        with pytest.raises(PcrlError):
            L.call("pcrl_conv3d_to1_wgrad", a["x"], a["dy"], a["dw"], a["db"], a["ws"], a["nb"], *vol, a["C"], a["taps"], a["dtype"], st)
    _untouched(dw, db)
