"""3D path: the 2x2x2 / stride-2 transposed convolution (pcrl_convt3d_k2s2_fwd, _dgrad, _wgrad: every up-sampling step that is not taken by the composed
up-convolution, and both inference forwards) bit for bit against float64 torch on exactly summable operands.  Method: tests/exact_lattice.py; cases,
references and route mirrors: tests/conv1_cases.py, whose preconditions and constant crossings tests/test_conv1_cases_cpu.py asserts on the CPU.

Every comparison is on bits at every element, outputs are pre-filled with NaN, hooks are restored in `finally`, and every test asserts the kernel /
route the library names (pcrl_convt3d_k2s2_fwd_kernel, pcrl_convt3d_k2s2_wgrad_route) before it compares."""
import pytest
import torch

import conv1_cases as K
import exact_lattice as X

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
DEV = "cuda"
NAN = float("nan")


def _act(t, dt):
    from pcrlv2_amd import ops
    return ops.to_act(t.to(dt).to(DEV), dt)


def _nan_act(N, D, H, W, C, dt):
    from pcrlv2_amd import ops
    a = ops.new_act(N, D, H, W, C, dt, DEV)
    a.fill_(NAN)
    return a


def _packed(w, dt):
    """(forward pack, data-gradient pack) of a [Ci, Co, 2, 2, 2] weight on the device"""
    from pcrlv2_amd import ops
    return ops.PackedWeights("convt").get(w, dt)


def _fwd(x, wf, bias, vol, Ci, Co, dt, impl, expect):
    from pcrlv2_amd._lib import dtype_code, lib, stream_handle
    L, (N, D, H, W) = lib(), vol
    L.debug_set_conv_impl(impl)
    try:
        kernel = L.call("pcrl_convt3d_k2s2_fwd_kernel", Ci, Co, dtype_code(dt))
        assert kernel == expect == K.convt_fwd_kernel(Ci, Co, dt, impl), f"kernel {kernel}, expected {expect}"
        y = _nan_act(N, 2 * D, 2 * H, 2 * W, Co, dt)
        L.call("pcrl_convt3d_k2s2_fwd", x, wf, bias, y, N, D, H, W, Ci, Co, dtype_code(dt), stream_handle())
        torch.cuda.synchronize()
    finally:
        L.debug_set_conv_impl(0)
    return y


def run_id(r):
    return "-".join([K.ct_id(r[0]), K.dname(r[1])] + [str(v) for v in r[2:]])


@pytest.mark.parametrize("run", K.convt_fwd_runs(), ids=run_id)
def test_convt_fwd(run):
    """The implicit-GEMM forward (float32, bf16, and every streaming shape again under conv_impl = 1) and the streaming kernel: one block whose last wave
    is partly and wholly out of range, a tail block, the three K / 128 instances, the column tiles split eight ways; with and without bias."""
    s, dt, impl, bias = run
    R = K.convt_reference(s.vol, s.Ci, s.Co)
    wf, _ = _packed(R.w.float().to(DEV), dt)
    expect = K.convt_fwd_kernel(s.Ci, s.Co, dt, impl)
    y = _fwd(_act(R.x, dt), wf, R.b.float().to(DEV) if bias else None, s.vol, s.Ci, s.Co, dt, impl, expect)
    X.assert_bit_equal(y, R.y if bias else R.y_nobias, dt, f"convT fwd {run_id(run)} kernel {expect} ({s.why})")


@pytest.mark.parametrize("impl", [0, 1], ids=["impl0", "impl1"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("s", K.CT_BIG, ids=K.ct_id)
def test_convt_fwd_at_scale(s, bias, impl):
    """The streaming kernel where only a large volume reaches: column tiles that cross a tap inside one block at three tiles per tap (split = 4), one
    split (768 row blocks), the non-temporal stores (an output of exactly 192 MiB) and one row block fewer (plain stores); and the implicit GEMM on the
    same volumes under conv_impl = 1.  Generated on the device, compared there against a chunked float64 product."""
    N, D, H, W = s.vol
    M, lat = K.voxels(s.vol), X.fine_for(s.Ci)
    p = K.up2_plan(M, s.Co)
    x = K.device_lattice((M, s.Ci), *lat["x"], BF, 21, DEV)
    w = K.device_lattice((s.Ci, s.Co, 2, 2, 2), *lat["w"], F32, 22, DEV)
    b = K.device_lattice((s.Co,), *lat["b"], F32, 23, DEV) if bias else None
    wf, _ = _packed(w, BF)
    kernel = K.CT_STREAM if impl == 0 else K.CT_IGEMM
    y = _fwd(x.view(N, D, H, W, s.Ci).permute(0, 4, 1, 2, 3), wf, b, s.vol, s.Ci, s.Co, BF, impl, kernel)
    rows = K.convt_rows_view(y, s.vol)
    got = rows.view(torch.int16)
    what = f"convT fwd {K.ct_id(s)} kernel {kernel}" + (f", split {p.split}, {p.tiles_per_block} tiles per block, non-temporal {p.nt} ({s.why})" if impl == 0 else "")
    worst = 0.0
    for r0, r1 in K.chunks(M):
        want = K.convt_rows_restated(x[r0:r1], w, b)
        worst = max(worst, float(K.convt_rows_restated(x[r0:r1].abs(), w.abs(), None if b is None else b.abs()).max()))
        bad = got[r0:r1] != want.to(BF).view(torch.int16)
        if bool(bad.any()):
            m, t, co = (int(v) for v in bad.nonzero()[0])
            raise AssertionError(f"{what}: {int(bad.sum())} elements of rows {r0}..{r1} differ; first at input voxel {r0 + m} (row block {(r0 + m) // K.UP2_ROWS}, "
                                 f"lane voxel {(r0 + m) % K.UP2_ROWS}), tap {t}, channel {co}: got {float(rows[r0 + m, t, co])}, "
                                 f"want {float(want[m, t, co])}")
    X.assert_exactly_summable(worst, X.unit(lat["x"][1], lat["w"][1]), what)


@pytest.mark.parametrize("dt", [F32, BF], ids=K.dname)
@pytest.mark.parametrize("s", K.CT_SHAPES, ids=K.ct_id)
def test_convt_dgrad(s, dt):
    """dx[n, ci, d, h, w] = sum over the eight taps and Co of dy[n, co, 2d+kd, 2h+kh, 2w+kw] w[ci, co, kd, kh, kw]: one K = 8 Co gather GEMM"""
    from pcrlv2_amd._lib import dtype_code, lib, stream_handle
    N, D, H, W = s.vol
    R = K.convt_reference(s.vol, s.Ci, s.Co)
    _, wd = _packed(R.w.float().to(DEV), dt)
    dx = _nan_act(N, D, H, W, s.Ci, dt)
    lib().call("pcrl_convt3d_k2s2_dgrad", _act(R.dy, dt), wd, dx, N, D, H, W, s.Ci, s.Co, dtype_code(dt), stream_handle())
    X.assert_bit_equal(dx, R.dx, dt, f"convT dgrad {K.ct_id(s)} {K.dname(dt)}")


@pytest.mark.parametrize("dt", [F32, BF], ids=K.dname)
@pytest.mark.parametrize("s", K.CT_BIG[:2], ids=K.ct_id)
def test_convt_dgrad_at_scale(s, dt):
    """The data gradient on the large volumes of the forward (all but the two largest): K = 8 Co = 1536 and 512, 192 and 768 row tiles.  Generated on
    the device, compared there against a chunked float64 product."""
    from pcrlv2_amd._lib import dtype_code, lib, stream_handle
    N, D, H, W = s.vol
    M, lat = K.voxels(s.vol), X.fine_for(8 * s.Co)
    dy_rows = K.device_lattice((M, 8, s.Co), *lat["dy"], dt, 31, DEV)
    w = K.device_lattice((s.Ci, s.Co, 2, 2, 2), *lat["w"], F32, 32, DEV)
    _, wd = _packed(w, dt)
    dy = K.convt_rows_unview(dy_rows, s.vol)
    dx = _nan_act(N, D, H, W, s.Ci, dt)
    lib().call("pcrl_convt3d_k2s2_dgrad", dy, wd, dx, N, D, H, W, s.Ci, s.Co, dtype_code(dt), stream_handle())
    torch.cuda.synchronize()
    got = dx.permute(0, 2, 3, 4, 1).reshape(M, s.Ci)
    what, worst = f"convT dgrad {K.ct_id(s)} {K.dname(dt)}", 0.0
    for r0, r1 in K.chunks(M):
        want = K.convt_dgrad_rows_restated(dy_rows[r0:r1], w)
        worst = max(worst, float(K.convt_dgrad_rows_restated(dy_rows[r0:r1].abs(), w.abs()).max()))
        bad = got[r0:r1].view(torch.int16 if dt == BF else torch.int32) != want.to(dt).view(torch.int16 if dt == BF else torch.int32)
        if bool(bad.any()):
            m, ci = (int(v) for v in bad.nonzero()[0])
            raise AssertionError(f"{what}: {int(bad.sum())} elements of rows {r0}..{r1} differ; first at voxel {r0 + m}, channel {ci}: got {float(got[r0 + m, ci])}, want {float(want[m, ci])}")
    X.assert_exactly_summable(worst, X.unit(lat["dy"][1], lat["w"][1]), what)


@pytest.mark.parametrize("run", K.convt_wgrad_runs(), ids=run_id)
def test_convt_wgrad(run):
    """dw[ci, co, tap] = sum over the input voxels of x[m][ci] dy[2m + tap][co]: the all-taps kernel (one split with a K tail; five splits with a K tail
    in the last) and the gather kernel under wgrad_impl = 1, under wgrad_tr = 0, in float32 and for channel counts the all-taps kernel does not take.
    A workspace one byte short of what the route asks for is rejected."""
    from pcrlv2_amd._lib import PcrlError, dtype_code, lib, stream_handle
    s, dt, impl, tr = run
    N, D, H, W = s.vol
    L, dc = lib(), dtype_code(dt)
    R = K.convt_reference(s.vol, s.Ci, s.Co)
    xa, dya = _act(R.x, dt), _act(R.dy, dt)
    L.debug_set_wgrad_impl(impl)
    L.debug_set_wgrad_tr(tr)
    try:
        route = L.call("pcrl_convt3d_k2s2_wgrad_route", s.Ci, s.Co, dc)
        assert route == K.convt_wgrad_route(s.Ci, s.Co, dt, impl, tr), route
        nb, need = L.call("pcrl_convt3d_k2s2_wgrad_ws_bytes", N, D, H, W, s.Ci, s.Co), K.convt_wgrad_need(K.voxels(s.vol), s.Ci, s.Co, route)
        assert need <= nb
        dw, ws = torch.full((s.Ci, s.Co, 2, 2, 2), NAN, dtype=F32, device=DEV), torch.empty(nb, dtype=torch.uint8, device=DEV)
        with pytest.raises(PcrlError):
            L.call("pcrl_convt3d_k2s2_wgrad", xa, dya, dw, ws, need - 1, N, D, H, W, s.Ci, s.Co, dc, stream_handle())
        torch.cuda.synchronize()
        assert bool(torch.isnan(dw).all()), "a rejected call wrote its output"
        L.call("pcrl_convt3d_k2s2_wgrad", xa, dya, dw, ws, nb, N, D, H, W, s.Ci, s.Co, dc, stream_handle())
    finally:
        L.debug_set_wgrad_impl(0)
        L.debug_set_wgrad_tr(1)
    plan = K.plan_up2(K.voxels(s.vol), s.Ci, s.Co) if route == K.CT_WG_ALLTAPS else K.plan_splits(K.voxels(s.vol), s.Ci, s.Co, 8)
    X.assert_bit_equal(dw, R.dw, F32, f"convT wgrad {run_id(run)} route {route} (splits, chunk) = {plan}")


@pytest.mark.parametrize("dt", [F32, BF], ids=K.dname)
def test_convt_rejections(dt):
    """Host-side checks only, nothing is launched: channel multiples, extents, dtype, null pointers"""
    from pcrlv2_amd._lib import PcrlError, dtype_code, lib, stream_handle
    L, dc, st = lib(), dtype_code(dt), stream_handle()
    N, D, H, W, Ci, Co = 1, 2, 2, 2, 64, 64
    x, dy = torch.zeros(8 * Ci, dtype=dt, device=DEV), torch.zeros(64 * Co, dtype=dt, device=DEV)
    wp = torch.zeros(8 * Ci * Co, dtype=dt, device=DEV)
    y, dx = torch.full((64 * Co,), NAN, dtype=dt, device=DEV), torch.full((8 * Ci,), NAN, dtype=dt, device=DEV)
    dw = torch.full((8 * Ci * Co,), NAN, dtype=F32, device=DEV)
    nb = L.call("pcrl_convt3d_k2s2_wgrad_ws_bytes", N, D, H, W, Ci, Co)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    dims = [dict(Ci=48), dict(Co=16), dict(Ci=0), dict(D=0)]
    for kw in dims + [dict(dtype=7), dict(a=None), dict(wp=None), dict(out=None)]:
        a = dict(N=N, D=D, H=H, W=W, Ci=Ci, Co=Co, dtype=dc, a=x, wp=wp, out=y)
        a.update(kw)
        with pytest.raises(PcrlError):
            L.call("pcrl_convt3d_k2s2_fwd", a["a"], a["wp"], None, a["out"], a["N"], a["D"], a["H"], a["W"], a["Ci"], a["Co"], a["dtype"], st)
        a = dict(N=N, D=D, H=H, W=W, Ci=Ci, Co=Co, dtype=dc, a=dy, wp=wp, out=dx)
        a.update(kw)
        with pytest.raises(PcrlError):
            L.call("pcrl_convt3d_k2s2_dgrad", a["a"], a["wp"], a["out"], a["N"], a["D"], a["H"], a["W"], a["Ci"], a["Co"], a["dtype"], st)
    for kw in dims[:3] + [dict(dtype=7), dict(x=None), dict(dy=None), dict(dw=None), dict(ws=None), dict(nb=0)]:
        a = dict(N=N, D=D, H=H, W=W, Ci=Ci, Co=Co, dtype=dc, x=x, dy=dy, dw=dw, ws=ws, nb=nb)
        a.update(kw)
        with pytest.raises(PcrlError):
            L.call("pcrl_convt3d_k2s2_wgrad", a["x"], a["dy"], a["dw"], a["ws"], a["nb"], a["N"], a["D"], a["H"], a["W"], a["Ci"], a["Co"], a["dtype"], st)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in (y, dx, dw)), "a rejected call wrote its output"
