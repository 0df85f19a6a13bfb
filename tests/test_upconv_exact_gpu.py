"""3D path: the composed ConvTranspose3d(k2, s2) -> Conv3d(3x3x3) operator (pcrl_upconv_compose, _fwd, _dgrad, _dgrad_ws, _wgrad_accum, _wgrad_finish,
_wgrad; ops.upconv_luconv_forward / _backward) bit for bit against float64 torch on exactly summable operands.  Method: tests/exact_lattice.py;
cases, lattices, references, layout decoders and route mirrors: tests/upconv_cases.py, whose preconditions tests/test_upconv_cases_cpu.py asserts on
the CPU.  A sparse transposed convolution keeps the composed 8-tap weights on a lattice of bf16 values, so every sum of the operator is exact in
float32 in any order and over any split: no tolerance anywhere in this file.

Every comparison is on bits at every element, outputs are pre-filled with NaN, hooks are restored in `finally`, and every run asserts the kernel family
the library names for it before it compares."""
import functools
import os
import subprocess
import sys
import types

import pytest
import torch

import exact_lattice as X
import upconv_cases as K

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
DEV = "cuda"
NAN = float("nan")
LATS = ("fine", "stats")
FAMILY = {K.GATHER: 0, K.B8: 1, K.B8_P: 1, K.B8_32: 1, K.B8_32_P: 1, K.B8_64: 1, K.WIDE: 2, K.WIDE_P: 2}      # pcrl_conv3d_k3_fwd_kernel's codes
COMPOSE_SHAPES = [(32, 32, 64), (64, 96, 32), (64, 64, 64)]      # Ci, Cm, Co: Ci != Co both ways, Cm = 32 and 96


def _lib():
    from pcrlv2_amd._lib import dtype_code, lib, stream_handle
    return lib(), dtype_code, stream_handle()


def _act(t, dt):
    from pcrlv2_amd import ops
    return ops.to_act(t.to(dt).to(DEV), dt)


def _nan_act(N, D, H, W, C, dt):
    from pcrlv2_amd import ops
    a = ops.new_act(N, D, H, W, C, dt, DEV)
    a.fill_(NAN)
    return a


def _f32(t):
    return t.float().to(DEV).contiguous()


def _nan(n, dt=F32):
    return torch.full((n,), NAN, dtype=dt, device=DEV)


def _ws(nb):
    return torch.empty(max(int(nb), 16), dtype=torch.uint8, device=DEV)


def _fine_brick(route):
    b = K.brick_of(route)
    return {"d": 2 * b[0], "h": 2 * b[1], "w": 2 * b[2]} if b else None


def _coarse_brick(route):
    b = K.brick_of(route)
    return {"d": b[0], "h": b[1], "w": b[2]} if b else None


def _compose(w_up, b_up, w0, b0, dt):
    """pcrl_upconv_compose with all four layouts and the bias table, every output pre-filled with NaN"""
    L, dtype_code, st = _lib()
    Ci, Cm, Co = w_up.shape[0], w_up.shape[1], w0.shape[0]
    W = types.SimpleNamespace(wf=_nan(64 * Ci * Co, dt), wd=_nan(64 * Ci * Co, dt), w3f=_nan(216 * Ci * Co, dt), wd3=_nan(216 * Ci * Co, dt), tab=_nan(27 * Co))
    nb = L.call("pcrl_upconv_compose_ws_bytes", Ci, Cm, Co, dtype_code(dt))
    L.call("pcrl_upconv_compose", _f32(w_up), _f32(b_up), _f32(w0), _f32(b0), W.wf, W.wd, W.w3f, W.wd3, W.tab, _ws(nb), nb, Ci, Cm, Co, dtype_code(dt), st)
    torch.cuda.synchronize()
    return W


@functools.lru_cache(maxsize=None)
def _composed(c, lat, dt):
    R = K.reference(c, lat)
    return _compose(R.w_up, R.b_up, R.w0, R.b0, dt)


# ---- routes -----------------------------------------------------------------------------------------------------------------------------
def _assert_routes(L, dtype_code, c, dt, conv_impl, wgrad_impl):
    """Under the hooks in force: the library's answers agree with the mirrors of upconv_cases.py -> (fwd, dgrad, wgrad) route names"""
    g, dc = (c.N, c.D, c.H, c.W), dtype_code(dt)
    fwd, dgrad, wgrad = K.fwd_route(c, dt, conv_impl), K.dgrad_route(c, dt, conv_impl), K.wgrad_route(c, dt, wgrad_impl)
    f = L.call("pcrl_upconv_fwd_uses_brick", *g, c.Ci, c.Co, dc)
    fam = L.call("pcrl_conv3d_k3_fwd_kernel", *g, c.Ci, 8 * c.Co, dc) if f else 0
    assert fam == FAMILY[fwd], (K.case_id(c), dt, "forward", fam, fwd)
    d = L.call("pcrl_upconv_dgrad_uses_brick", *g, c.Ci, c.Co, dc)
    fam = (2 if (L.call("pcrl_conv3d_k3_fwd_kernel", *g, 8 * c.Co, c.Ci, dc) == 2 and c.Ci % 64 == 0) else 1) if d else 0
    assert fam == FAMILY[dgrad], (K.case_id(c), dt, "data gradient", fam, dgrad)
    assert L.call("pcrl_upconv_wgrad_uses_brick", *g, c.Ci, c.Co, dc) == (wgrad != K.WG_GATHER), (K.case_id(c), dt, "weight gradient", wgrad)
    assert L.call("pcrl_upconv_stats_rows", *g, c.Ci, c.Co, dc) == K.stats_rows(c, dt, conv_impl)
    nbd = L.call("pcrl_upconv_dgrad_ws_bytes", *g, c.Ci, c.Co, dc)
    splits = K.dgrad_splits(c) if dgrad == K.GATHER else 1
    assert nbd == (splits * c.N * c.D * c.H * c.W * c.Ci * 4 if splits > 1 else 0), (K.case_id(c), nbd, splits)
    return fwd, dgrad, wgrad, splits


def test_run_lists_reach_every_route():
    """Host only (no launch): over the run lists below, the (pass, route) pairs the LIBRARY names are the full expected set -- gather, wide brick on both
    axis orders, the 4 x 8 x 8 brick on both axis orders with both data-gradient tile widths, both weight-gradient routes (and the weight-gradient
    brick with two ranges), and the split-K data gradient."""
    L, dtype_code, _ = _lib()
    got = set()
    try:
        for c, dt, impl in K.fwd_runs():
            L.debug_set_conv_impl(impl)
            fwd, dgrad, _, splits = _assert_routes(L, dtype_code, c, dt, impl, 0)
            got |= {("fwd", fwd), ("dgrad", dgrad)} | ({("dgrad", "gather-splitk")} if splits > 1 else set())
        L.debug_set_conv_impl(0)
        for c, dt, impl in K.wgrad_runs():
            L.debug_set_wgrad_impl(impl)
            wgrad = _assert_routes(L, dtype_code, c, dt, 0, impl)[2]
            got |= {("wgrad", wgrad)} | ({("wgrad", "brick-splits")} if wgrad != K.WG_GATHER and K.wgrad_brick_splits(c) > 1 else set())
    finally:
        L.debug_set_conv_impl(0)
        L.debug_set_wgrad_impl(0)
    assert got == K.EXPECTED_REACHED, (got ^ K.EXPECTED_REACHED)
    assert L.call("pcrl_upconv_dgrad_ws_bytes", *K.SPLITK_DGRAD_CASE[:4], K.SPLITK_DGRAD_CASE.Ci, K.SPLITK_DGRAD_CASE.Co, dtype_code(BF)) > 0


# ---- compose ----------------------------------------------------------------------------------------------------------------------------
def check_compose(Ci, Cm, Co, dt, lat):
    """The four layouts decode to the float64 Weff of the impulse response bit for bit, the embedded forms are zero everywhere else, bias_tab equals
    the two calls' response to x = 0"""
    w_up, b_up, w0, b0 = K.weights(Ci, Cm, Co, lat, 100 + Ci + 2 * Cm + 3 * Co)
    weff, tab = K.impulse_weff(w_up, w0), K.impulse_bias_tab(w_up, b_up, w0, b0)
    u = K.units(K.LATTICES[lat])
    what = f"compose {Ci}x{Cm}x{Co} {K.dname(dt)} [{lat}]"
    assert torch.equal(weff.to(BF).double(), weff), what
    X.assert_exactly_summable(K.compose_from_pairs(w_up.abs(), w0.abs()), u.weff, what + " composed weights")
    X.assert_exactly_summable(K.impulse_bias_tab(w_up.abs(), b_up.abs(), w0.abs(), b0.abs()), u.weff / K.LATTICES[lat]["b"][1], what + " bias table")
    W = _compose(w_up, b_up, w0, b0, dt)
    X.assert_bit_equal(K.decode_wf(W.wf.cpu(), Ci, Co), weff, dt, what + " wf")
    X.assert_bit_equal(K.decode_wd(W.wd.cpu(), Ci, Co), weff, dt, what + " wd")
    for name, t, dec in (("w3f", W.w3f, K.decode_w3f), ("wd3", W.wd3, K.decode_wd3)):
        got, rest = dec(t.cpu(), Ci, Co)
        X.assert_bit_equal(got, weff, dt, f"{what} {name}")
        assert float(rest.float().abs().max()) == 0, f"{what} {name}: {int((rest.float() != 0).sum())} entries outside the embedded taps are not zero"
    X.assert_bit_equal(W.tab.view(27, Co), tab, F32, what + " bias_tab")


def run_compose_checks():
    n = 0
    for Ci, Cm, Co in COMPOSE_SHAPES:
        for dt in (F32, BF):
            for lat in LATS:
                check_compose(Ci, Cm, Co, dt, lat)
                n += 1
    return n


def test_compose_tiled():
    assert run_compose_checks() == 12


def test_compose_untiled():
    """The same checks in a child process with PCRL_UPC_PACK_TILED=0 (read once per process): upc_pack_kernel instead of upc_pack_tiled_kernel"""
    here = os.path.dirname(os.path.abspath(__file__))
    prog = "import sys; sys.path[:0] = [%r, %r]; import test_upconv_exact_gpu as T; print('COMPOSE-OK', T.run_compose_checks())" % (os.path.dirname(here), here)
    r = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, env=dict(os.environ, PCRL_UPC_PACK_TILED="0"), timeout=600)
    assert r.returncode == 0 and "COMPOSE-OK 12" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---- forward and data gradient ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", K.fwd_runs(), ids=K.run_id)
def test_forward(run):
    """pcrl_upconv_fwd: y0 at every element on both lattices, the (sum, sum^2) rows on the stats lattice"""
    c, dt, impl = run
    L, dtype_code, st = _lib()
    g, dc = (c.N, c.D, c.H, c.W), dtype_code(dt)
    L.debug_set_conv_impl(impl)
    try:
        route = _assert_routes(L, dtype_code, c, dt, impl, 0)[0]
        rows = K.stats_rows(c, dt, impl)
        for lat in LATS:
            R, W = K.reference(c, lat), _composed(c, lat, dt)
            y, part = _nan_act(c.N, 2 * c.D, 2 * c.H, 2 * c.W, c.Co, dt), _nan(rows * c.Co * 2)
            L.call("pcrl_upconv_fwd", _act(R.x, dt), W.wf, W.w3f, W.tab, y, part, *g, c.Ci, c.Co, dc, st)
            what = f"upconv fwd {K.run_id(run)} [{lat}] route {route} ({c.why})"
            X.assert_bit_equal(y, R.y, dt, what, brick=_fine_brick(route))
            if lat == "stats" and c.stats:
                rows_ = part.view(rows, c.Co, 2)
                X.assert_rows_exact(rows_[:, :, 0], R.sum_y, what + " statistics: sum y")
                X.assert_rows_exact(rows_[:, :, 1], R.sum_y2, what + " statistics: sum y^2")
    finally:
        L.debug_set_conv_impl(0)


@pytest.mark.parametrize("run", K.fwd_runs(), ids=K.run_id)
def test_dgrad(run):
    """pcrl_upconv_dgrad and pcrl_upconv_dgrad_ws at every element; the workspace form (split-K partial sums and a finish pass on the gather route) and
    the one-pass form are bit-identical"""
    c, dt, impl = run
    L, dtype_code, st = _lib()
    g, dc = (c.N, c.D, c.H, c.W), dtype_code(dt)
    L.debug_set_conv_impl(impl)
    try:
        _, route, _, splits = _assert_routes(L, dtype_code, c, dt, impl, 0)
        nbd = L.call("pcrl_upconv_dgrad_ws_bytes", *g, c.Ci, c.Co, dc)
        for lat in LATS:
            R, W = K.reference(c, lat), _composed(c, lat, dt)
            dya = _act(R.dy, dt)
            dx1, dx2 = _nan_act(*g, c.Ci, dt), _nan_act(*g, c.Ci, dt)
            L.call("pcrl_upconv_dgrad", dya, W.wd, W.wd3, dx1, *g, c.Ci, c.Co, dc, st)
            L.call("pcrl_upconv_dgrad_ws", dya, W.wd, W.wd3, dx2, _ws(nbd) if nbd else None, nbd, *g, c.Ci, c.Co, dc, st)
            what = f"upconv dgrad {K.run_id(run)} [{lat}] route {route}, {splits} K split(s) with a workspace ({c.why})"
            X.assert_bit_equal(dx1, R.dx, dt, what + " one pass", brick=_coarse_brick(route))
            X.assert_bit_equal(dx2, R.dx, dt, what + " workspace form", brick=_coarse_brick(route))
    finally:
        L.debug_set_conv_impl(0)


# ---- weight gradient --------------------------------------------------------------------------------------------------------------------
def _accum(L, dtype_code, st, c, dt, x, dy, flags, dweff, box):
    g, dc = (c.N, c.D, c.H, c.W), dtype_code(dt)
    nb = L.call("pcrl_upconv_wgrad_accum_ws_bytes", *g, c.Ci, c.Co, dc)
    L.call("pcrl_upconv_wgrad_accum", _act(x, dt), _act(dy, dt), dweff, box, flags, _ws(nb), nb, *g, c.Ci, c.Co, dc, st)


def _check_acc(c, dweff, box, ref_dweff, ref_box, what):
    torch.cuda.synchronize()
    X.assert_bit_equal(K.decode_dweff(dweff.cpu(), c.Ci, c.Co), ref_dweff, F32, what + " dweff_acc [p][q][ci][co]")
    X.assert_bit_equal(box.view(27, c.Co), ref_box, F32, what + " box_acc")


@pytest.mark.parametrize("run", K.wgrad_runs(), ids=K.run_id)
def test_wgrad_accum(run):
    """pcrl_upconv_wgrad_accum: dweff_acc and box_acc equal float64 exactly under both weight-gradient routes; flags 1 and 3 on a zero-sum dy; and the
    add-to-accumulator mode every training step uses on its second and third pass: flags 1 then 0, flags 3 then 2.  NaN-filled buffers are fully
    overwritten by every flags-bit-0 call."""
    c, dt, impl = run
    L, dtype_code, st = _lib()
    n_w, n_b = 64 * c.Ci * c.Co, 27 * c.Co
    L.debug_set_wgrad_impl(impl)
    try:
        route = _assert_routes(L, dtype_code, c, dt, 0, impl)[2]
        what = f"upconv wgrad_accum {K.run_id(run)} route {route}, {K.wgrad_brick_splits(c) if route != K.WG_GATHER else 1} brick range(s)"
        for lat in LATS:
            R, Z = K.reference(c, lat), K.zero_sum_reference(c, lat)
            dweff, box = _nan(n_w), _nan(n_b)
            _accum(L, dtype_code, st, c, dt, R.x, R.dy, 1, dweff, box)
            _check_acc(c, dweff, box, R.dweff, R.box, f"{what} [{lat}] flags 1")
            for flags in (1, 3):
                dweff, box = _nan(n_w), _nan(n_b)
                _accum(L, dtype_code, st, c, dt, R.x, Z.dy, flags, dweff, box)
                _check_acc(c, dweff, box, Z.dweff, Z.box, f"{what} [{lat}] zero-sum dy, flags {flags}")
        (R1, Z1), (R2, Z2) = [(K.reference(c, lat), K.zero_sum_reference(c, lat)) for lat in LATS]
        u = min(R1.u.dweff, R2.u.dweff)
        X.assert_exactly_summable(R1.dweff_abs + R2.dweff_abs, u, what + " two passes: dWeff")
        X.assert_exactly_summable(R1.box_abs + R2.box_abs, min(R1.u.box, R2.u.box), what + " two passes: box sums")
        for first, (dy1, dy2), (rw, rb) in ((1, (R1.dy, R2.dy), (R1.dweff + R2.dweff, R1.box + R2.box)), (3, (Z1.dy, Z2.dy), (Z1.dweff + Z2.dweff, Z1.box + Z2.box))):
            dweff, box = _nan(n_w), _nan(n_b)
            _accum(L, dtype_code, st, c, dt, R1.x, dy1, first, dweff, box)
            _accum(L, dtype_code, st, c, dt, R2.x, dy2, first & 2, dweff, box)
            _check_acc(c, dweff, box, rw, rb, f"{what} flags {first} then {first & 2}")
    finally:
        L.debug_set_wgrad_impl(0)


@pytest.mark.parametrize("dt", [F32, BF], ids=K.dname)
@pytest.mark.parametrize("shape", COMPOSE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_wgrad_finish_alone(shape, dt):
    """pcrl_upconv_wgrad_finish on accumulators that do not come from data: integers up to 256 in bf16 mode (upc_chain_pack_kernel<bf16> rounds dWeff),
    i/64 with |i| <= 2^12 in float32 mode; weights on the fine lattice.  Against the float64 chain rule of upconv_cases.py."""
    Ci, Cm, Co = shape
    L, dtype_code, st = _lib()
    w_up, b_up, w0, _ = K.weights(Ci, Cm, Co, "fine", 300 + Ci + Cm + Co)
    g = torch.Generator().manual_seed(7 + Ci + Co)
    mx, den = (256, 1) if dt == BF else (1 << 12, 64)
    dweff = torch.randint(-mx, mx + 1, (8, 8, Ci, Co), generator=g).double() / den
    box = torch.randint(-mx, mx + 1, (27, Co), generator=g).double() / den
    if dt == BF:
        assert torch.equal(dweff.to(BF).double(), dweff)
    assert torch.equal(dweff.float().double(), dweff) and torch.equal(box.float().double(), box)
    ref = K.chain_rule(dweff, box, w_up, b_up, w0)
    ab = K.chain_rule(dweff.abs(), box.abs(), w_up.abs(), b_up.abs(), w0.abs())
    what = f"upconv wgrad_finish {shape} {K.dname(dt)}"
    # units: dweff 1/den, w0 1/8, w_up 1/2, b_up 1/4, box 1/den
    X.assert_exactly_summable(ab[0], X.unit(den, 8), what + " dw_up")
    X.assert_exactly_summable(ab[1], X.unit(den, 8), what + " db_up")
    X.assert_exactly_summable(ab[2], X.unit(den, 4), what + " dw0")
    dwu, dbu, dwc = _nan(Ci * Cm * 8), _nan(Cm), _nan(Co * Cm * 27)
    nb = L.call("pcrl_upconv_wgrad_finish_ws_bytes", Ci, Cm, Co, dtype_code(dt))
    L.call("pcrl_upconv_wgrad_finish", _f32(K.encode_dweff(dweff)), _f32(box), _f32(w_up), _f32(b_up), _f32(w0), dwu, dbu, dwc, _ws(nb), nb, Ci, Cm, Co,
           dtype_code(dt), st)
    X.assert_bit_equal(dwu.view(w_up.shape), ref[0], F32, what + " dw_up")
    X.assert_bit_equal(dbu, ref[1], F32, what + " db_up")
    X.assert_bit_equal(dwc.view(w0.shape), ref[2], F32, what + " dw0")


def _e2e_runs():
    """(case, dtype, lattice): float32 on both lattices, bf16 where dWeff passed the bf16 round trip (upconv_cases.reference asserts it)"""
    return [(c, dt, lat) for c in K.ACCUM_CASES for dt in (F32, BF) for lat in LATS if dt == F32 or (lat == "stats" and c.chain)]


@pytest.mark.parametrize("run", _e2e_runs(), ids=lambda r: f"{K.case_id(r[0])}-{K.dname(r[1])}-{r[2]}")
def test_wgrad_end_to_end(run):
    """pcrl_upconv_wgrad against autograd's dw_up, db_up, dw0 of the two aten calls: float32 outputs, exactly equal"""
    c, dt, lat = run
    L, dtype_code, st = _lib()
    g, dc = (c.N, c.D, c.H, c.W), dtype_code(dt)
    R = K.reference(c, lat)
    assert dt == F32 or R.chain_bf16
    route = _assert_routes(L, dtype_code, c, dt, 0, 0)[2]
    dwu, dbu, dwc = _nan(R.w_up.numel()), _nan(c.Cm), _nan(R.w0.numel())
    nb = L.call("pcrl_upconv_wgrad_ws_bytes", *g, c.Ci, c.Cm, c.Co, dc)
    L.call("pcrl_upconv_wgrad", _act(R.x, dt), _act(R.dy, dt), _f32(R.w_up), _f32(R.b_up), _f32(R.w0), dwu, dbu, dwc, _ws(nb), nb, *g, c.Ci, c.Cm, c.Co, dc, st)
    what = f"upconv wgrad {K.case_id(c)} {K.dname(dt)} [{lat}] route {route}"
    X.assert_bit_equal(dwu.view(R.w_up.shape), R.dw_up, F32, what + " dw_up")
    X.assert_bit_equal(dbu, R.db_up, F32, what + " db_up")
    X.assert_bit_equal(dwc.view(R.w0.shape), R.dw0, F32, what + " dw0")


# ---- the Python path ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF], ids=K.dname)
def test_stage_head_through_ops(dt):
    """ops.upconv_luconv_forward / _backward on the stats lattice (a case with 2^k voxels per channel, so the mean is a lattice value too): what the
    Python path hands to BatchNorm -- the convolution output and the batch mean from its statistics rows -- equals the reference; a second forward
    reuses the ComposedUpConv cache; and the backward pass (side stream, accumulators, chain rule) delivers the very bits of the direct library calls
    on the same BatchNorm gradient.  The BatchNorm arithmetic itself stays with its own tests."""
    from pcrlv2_amd import config, ops
    from pcrlv2_amd._lib import ACT_RELU
    L, dtype_code, st = _lib()
    c = K.CASES[13]
    assert (c.N, c.D, c.H, c.W) == (1, 2, 8, 8) and c.stats
    g, dc = (c.N, c.D, c.H, c.W), dtype_code(dt)
    M = 8 * c.N * c.D * c.H * c.W
    assert M & (M - 1) == 0
    R = K.reference(c, "stats")
    wu, bu, wc, bc = (_f32(t) for t in (R.w_up, R.b_up, R.w0, R.b0))
    gen = torch.Generator().manual_seed(11)
    gamma, beta = _f32(1 + X.lattice((c.Co,), 2, 8, gen)), _f32(X.lattice((c.Co,), 4, 4, gen))
    rm, rv = torch.zeros(c.Co, device=DEV), torch.ones(c.Co, device=DEV)
    comp = ops.ComposedUpConv()
    xa = _act(R.x, dt)
    a, sv = ops.upconv_luconv_forward(xa, wu, bu, wc, bc, gamma, beta, rm, rv, comp, ACT_RELU, dt)
    what = f"ops.upconv_luconv_forward {K.case_id(c)} {K.dname(dt)}"
    X.assert_bit_equal(sv.y, R.y, dt, what + " convolution output")
    X.assert_bit_equal(sv.mean, R.sum_y / M, F32, what + " batch mean")
    wf_ptr = comp.wf.data_ptr()
    a2, sv2 = ops.upconv_luconv_forward(xa, wu, bu, wc, bc, gamma, beta, rm.clone(), rv.clone(), comp, ACT_RELU, dt)
    torch.cuda.synchronize()
    assert comp.wf.data_ptr() == wf_ptr, "the composed weights were rebuilt for unchanged parameters"
    assert torch.equal(sv2.y, sv.y) and torch.equal(a2, a)

    da = _act(X.lattice(R.dy.shape, 4, 4, gen), dt)
    dx, dwu, dbu, dwc, dbc, dg, dbe = ops.upconv_luconv_backward(sv, da.clone(), wu, bu, wc, bc, gamma, comp, dt)
    torch.cuda.synchronize()
    dy, dg2, dbe2 = ops.bn_act_backward(da.clone(), sv.y, gamma, sv.mean, sv.rstd, sv.scale, sv.shift, M, c.Co, sv.act, dt)
    W = _composed(c, "stats", dt)
    dx2 = _nan_act(*g, c.Ci, dt)
    nbd = L.call("pcrl_upconv_dgrad_ws_bytes", *g, c.Ci, c.Co, dc)
    L.call("pcrl_upconv_dgrad_ws", dy, W.wd, W.wd3, dx2, _ws(nbd) if nbd else None, nbd, *g, c.Ci, c.Co, dc, st)
    dweff, box = _nan(64 * c.Ci * c.Co), _nan(27 * c.Co)
    nb = L.call("pcrl_upconv_wgrad_accum_ws_bytes", *g, c.Ci, c.Co, dc)
    L.call("pcrl_upconv_wgrad_accum", xa, dy, dweff, box, 1 | (2 if config.UPC_ZERO_SUM else 0), _ws(nb), nb, *g, c.Ci, c.Co, dc, st)
    dwu2, dbu2, dwc2 = _nan(wu.numel()), _nan(c.Cm), _nan(wc.numel())
    nb = L.call("pcrl_upconv_wgrad_finish_ws_bytes", c.Ci, c.Cm, c.Co, dc)
    L.call("pcrl_upconv_wgrad_finish", dweff, box, wu, bu, wc, dwu2, dbu2, dwc2, _ws(nb), nb, c.Ci, c.Cm, c.Co, dc, st)
    torch.cuda.synchronize()
    for name, got, want in (("dx", dx, dx2), ("dw_up", dwu, dwu2.view(wu.shape)), ("db_up", dbu, dbu2), ("dw0", dwc, dwc2.view(wc.shape)), ("dgamma", dg, dg2),
                            ("dbeta", dbe, dbe2)):
        assert not bool(torch.isnan(want.float()).any()), name
        assert torch.equal(got.contiguous().view(-1), want.contiguous().view(-1)) if name != "dx" else torch.equal(got, want), \
            f"ops.upconv_luconv_backward {K.dname(dt)}: {name} differs from the direct library calls on the same BatchNorm gradient"
    assert float(dbc.abs().max()) == 0.0
