"""2D path: every convolution kernel bit for bit against float64 torch on exactly summable operands (tests/exact_lattice.py), through the C ABI.

The operands lie on a dyadic lattice, the precondition (sum |terms| < 2^24 units, asserted per case from the float64 reference alone) makes every
float32 accumulation exact in any order, so a float32 output equals the float64 reference and a bf16 output its round-to-nearest-even rounding at
EVERY element: a missing tap at one corner pixel, a halo row off by one, a parity class stored one pixel off or one wrong tail channel fails, where
the relative-L2 bound of tests/test_ops2d_gpu.py (which stays, as the random-Gaussian coverage) sees nothing below 6e-3 of the whole tensor.

Each case runs on two lattices: FINE (x = i/4, w = j/8; FINER, x = i/8, w = j/32, for sums of fewer than 512 products: the sums land between bf16
values, mostly on ties -- the output rounding is exercised) for the
outputs and the sum rows of the statistics, TERNARY (x, w in {-1, 0, 1}) where in addition the sum-of-squares rows are exactly summable.  With the
ternary pass no case needs the per-channel 2^-23 * sum y^2 bound: every statistics row of every case is held exactly.

The case lists and their float64 references are plain CPU code: tests/test_exact_lattice_cpu.py imports them and checks, without a GPU, that every
precondition holds and that torch's own float32 convolution reproduces the float64 one on them."""
import collections
import functools
import types

import pytest
import torch
import torch.nn.functional as F

import exact_lattice as X

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
GATHER, BRICK8, NARROW, BRICK16 = 0, 1, 2, 3      # pcrl_conv2d_fwd_kind / _dgrad_kind
BRICKS = {GATHER: None, BRICK8: {"n": 4, "h": 8, "w": 8}, NARROW: {"h": 8, "w": 32}, BRICK16: {"n": 4, "h": 8, "w": 16}}

# kind: the route pcrl_conv2d_fwd_kind answers for the case in bf16 under conv2d impl 0 (asserted); Ci = 3 is the image zero-padded to 8 channels
Case = collections.namedtuple("Case", "N Ci Co K stride pad up H W bias out_f32 kind")
C = Case
CASES = [
    # ---- gather kernel: N = 3, odd extents, stride 2 (3x3 and 1x1, odd and even extents), the stem on the 8-padded image, the 512-channel bottleneck
    C(3, 3, 64, 7, 2, 3, 0, 33, 21, 0, 0, GATHER),
    C(3, 64, 64, 3, 1, 1, 0, 15, 9, 0, 0, GATHER),
    C(3, 64, 128, 3, 2, 1, 0, 15, 9, 0, 0, GATHER),
    C(3, 128, 256, 3, 2, 1, 0, 8, 12, 0, 0, GATHER),
    C(3, 64, 128, 1, 2, 0, 0, 15, 9, 0, 0, GATHER),
    C(3, 128, 256, 1, 2, 0, 0, 8, 12, 0, 0, GATHER),
    C(3, 512, 256, 3, 1, 1, 1, 2, 2, 0, 0, GATHER),       # first decoder block: 2 x 2 behind the fused x2 upsample
    C(3, 512, 512, 3, 1, 1, 0, 2, 2, 0, 0, GATHER),
    C(3, 512, 512, 3, 1, 1, 0, 3, 3, 0, 0, GATHER),
    C(3, 64, 32, 3, 1, 1, 1, 8, 16, 0, 0, GATHER),        # 64 -> 32 behind the upsample: W % 32 == 0 but 64 source channels
    C(3, 32, 16, 3, 1, 1, 1, 5, 7, 0, 0, GATHER),         # upsampled source at odd coarse extents: data gradient + upsample backward as two kernels
    C(2, 16, 3, 1, 1, 0, 0, 16, 24, 1, 1, GATHER),        # float32 output, 1x1 -> 3 and 3x3 -> 3
    C(2, 16, 3, 3, 1, 1, 0, 16, 24, 1, 1, GATHER),
    # ---- right-sized narrow kernel: H % 8 == 0, W % 32 == 0, <= 32 channels on both sides
    C(3, 16, 16, 3, 1, 1, 0, 16, 32, 1, 0, NARROW),
    C(3, 32, 16, 3, 1, 1, 1, 8, 16, 0, 0, NARROW),
    C(3, 32, 32, 3, 1, 1, 0, 8, 64, 0, 0, NARROW),
    C(3, 16, 32, 3, 1, 1, 0, 24, 32, 0, 0, NARROW),
    C(3, 16, 16, 1, 1, 0, 0, 8, 32, 1, 0, NARROW),
    C(2, 16, 3, 1, 1, 0, 0, 16, 32, 1, 1, NARROW),
    C(2, 16, 3, 3, 1, 1, 0, 16, 32, 1, 1, NARROW),
    # ---- 4 images x 8 x 8 brick kernel: both channel-tile forms (Co % 64 == 0, Co = 32), the upsampled source
    C(4, 32, 128, 3, 1, 1, 0, 24, 8, 0, 0, BRICK8),
    C(4, 64, 32, 3, 1, 1, 0, 24, 8, 1, 0, BRICK8),
    C(4, 128, 64, 3, 1, 1, 1, 8, 8, 0, 0, BRICK8),
    C(8, 64, 32, 3, 1, 1, 1, 4, 8, 0, 0, BRICK8),
    # ---- wide brick (4 images x 8 x 16, and its permuted axes H % 16 == 0, W % 8 == 0): edge bricks in every direction, N = 4 and 8, both tile forms
    C(4, 64, 64, 3, 1, 1, 0, 16, 32, 0, 0, BRICK16),
    C(8, 32, 64, 3, 1, 1, 0, 24, 48, 0, 0, BRICK16),
    C(4, 64, 128, 3, 1, 1, 0, 32, 8, 0, 0, BRICK16),
    C(4, 128, 128, 3, 1, 1, 0, 8, 16, 1, 0, BRICK16),
    C(4, 128, 32, 3, 1, 1, 0, 16, 16, 0, 0, BRICK16),
    C(4, 64, 64, 3, 1, 1, 0, 8, 128, 0, 0, BRICK16),
]
STEM_CASES = [C(2, 3, 64, 7, 2, 3, 0, 32, 128, 0, 0, GATHER), C(3, 3, 64, 7, 2, 3, 0, 48, 64, 0, 0, GATHER)]     # pcrl_stem7_ok: H/2 % 8 == W/2 % 32 == 0
SMALL_BWD_CASES = [(16, 2, 32, 32), (32, 3, 21, 19), (128, 1, 5, 7)]      # Ci, N, H, W of pcrl_conv2d_1x1_small_bwd: two and one rows of 1024 pixels, odd


def case_id(c):
    return "x".join(str(int(v)) for v in c)


def runs(cases=None):
    """(case, dtype, conv2d impl): float32 and bf16 under impl 0; the brick shapes also under 2 (no wide brick) and 1 (gather kernel)."""
    out = []
    for c in (CASES if cases is None else cases):
        out += [(c, F32, 0), (c, BF, 0)]
        if c.kind in (BRICK8, BRICK16):
            out += [(c, BF, 2), (c, BF, 1)]
    return out


def run_id(r):
    return f"{case_id(r[0])}-{'bf16' if r[1] == BF else 'f32'}-impl{r[2]}"


def expected_kind(c, dt, impl):
    if dt != BF or impl == 1:
        return GATHER
    return BRICK8 if (impl == 2 and c.kind == BRICK16) else c.kind


def cip(c):
    return 8 if c.Ci < 8 else c.Ci


def cop(c):
    p = 8
    while p < c.Co:
        p *= 2
    return p


def out_dims(c):
    Hl, Wl = (2 * c.H, 2 * c.W) if c.up else (c.H, c.W)
    return (Hl + 2 * c.pad - c.K) // c.stride + 1, (Wl + 2 * c.pad - c.K) // c.stride + 1


def dgrad_path(c):
    """The branch of ops2d.conv2d_backward a case takes, as far as the host decides it: 's2' parity classes, 'up' (fused or two kernels: the library's
    pcrl_conv2d_dgrad_up_ok decides), 'plain'."""
    if c.stride == 2 and not c.up and c.H % 2 == 0 and c.W % 2 == 0 and ((c.K == 3 and c.pad == 1) or (c.K == 1 and c.pad == 0)):
        return "s2"
    return "up" if c.up else "plain"


# ---------------------------------------------------------------------------------------------------------------------------------------
# float64 references (CPU; computed once per case and lattice, shared by every test, never modified)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _conv(c, x, w, b):
    xin = F.interpolate(x, scale_factor=2, mode="nearest") if c.up else x
    return xin, F.conv2d(xin, w, b, c.stride, c.pad)


@functools.lru_cache(maxsize=None)
def reference(c, lat_name):
    """Operands on the lattice, float64 forward / data gradient / weight gradient by torch autograd, and the preconditions: every output's
    sum |terms| from the same graph on the absolute values."""
    lat = X.fine_for(c.Ci * c.K * c.K) if lat_name == "fine" else X.TERNARY
    g = torch.Generator().manual_seed(sum((k + 1) * int(v) for k, v in enumerate(c)) + (0 if lat_name == "fine" else 7919))
    x = X.lattice((c.N, c.Ci, c.H, c.W), *lat["x"], g)
    w = X.lattice((c.Co, c.Ci, c.K, c.K), *lat["w"], g)
    b = X.lattice((c.Co,), *lat["b"], g) if c.bias else None
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    xin, y = _conv(c, xr, wr, b)
    xin.retain_grad()
    dy = X.lattice(y.shape, *lat["dy"], g)
    y.backward(dy)
    xa, wa = x.abs().requires_grad_(True), w.abs().requires_grad_(True)
    xina, ya = _conv(c, xa, wa, None if b is None else b.abs())
    xina.retain_grad()
    ya.backward(dy.abs())
    R = types.SimpleNamespace(x=x, w=w, b=b, y=y.detach(), dy=dy, dx=xr.grad, dw=wr.grad, dx_fine=xin.grad.detach(), lat=lat_name, u_fwd=X.unit(lat["x"][1], lat["w"][1]),
                              y_abs=ya.detach(), dx_abs=xa.grad, dw_abs=wa.grad)
    u_fwd, u_dx, u_dw = X.unit(lat["x"][1], lat["w"][1]), X.unit(lat["dy"][1], lat["w"][1]), X.unit(lat["x"][1], lat["dy"][1])
    what = f"{case_id(c)} [{lat_name}]"
    R.headroom = max(X.assert_exactly_summable(R.y_abs, u_fwd, what + " forward"),
                     X.assert_exactly_summable(R.dx_abs, u_dx, what + " data gradient"),
                     X.assert_exactly_summable(R.dw_abs, u_dw, what + " weight gradient"),
                     X.assert_exactly_summable(R.y.abs().sum((0, 2, 3)), u_fwd, what + " statistics: sum y over the channel"))
    if lat_name == "ternary":
        X.assert_exactly_summable((R.y * R.y).sum((0, 2, 3)), u_fwd * u_fwd, what + " statistics: sum y^2 over the channel")
    return R


@functools.lru_cache(maxsize=None)
def affine_reference(c):
    """scale in {0.5, 1, 2}, shift and residual on the lattice: z = scale * y + shift (+ residual) stays on multiples of half the forward's unit and exactly summable."""
    R = reference(c, "fine")
    g = torch.Generator().manual_seed(1000 + sum((k + 1) * int(v) for k, v in enumerate(c)))
    scale = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (c.Co,), generator=g)]
    shift = X.lattice((c.Co,), 4, 4, g)
    res = X.lattice(R.y.shape, 4, 4, g)
    sv, hv = scale.view(1, -1, 1, 1), shift.view(1, -1, 1, 1)
    X.assert_exactly_summable(sv * R.y_abs + hv.abs() + res.abs(), R.u_fwd / 2, f"{case_id(c)} affine epilogue")
    return types.SimpleNamespace(scale=scale, shift=shift, res=res, z=sv * R.y + hv)


def route_sets(L):
    """Host only (no launch): the kernel kinds the case list reaches, per query.  L: pcrlv2_amd._lib.lib()."""
    from pcrlv2_amd._lib import dtype_code
    fwd, forms, dgrad, wgrad = set(), set(), set(), set()
    try:
        for c, dt, impl in runs():
            L.debug_set_conv2d_impl(impl)
            Ho, Wo = out_dims(c)
            k = L.call("pcrl_conv2d_fwd_kind", c.N, c.H, c.W, cip(c), c.Co, c.K, c.K, c.stride, c.pad, c.up, c.out_f32, dtype_code(dt))
            assert k == expected_kind(c, dt, impl), (c, dt, impl, k)
            fwd.add(k)
            forms.add((k, c.Co % 64 == 0))
            if dgrad_path(c) != "s2":
                Hl, Wl = (2 * c.H, 2 * c.W) if c.up else (c.H, c.W)
                dgrad.add(L.call("pcrl_conv2d_dgrad_kind", c.N, Hl, Wl, c.Ci, Ho, Wo, cop(c), c.K, c.K, c.stride, c.pad, dtype_code(dt)))
            for wimpl in (0, 1):
                L.debug_set_wgrad_impl(wimpl)
                wgrad.add((wimpl, L.call("pcrl_conv2d_wgrad_kind", c.N, c.H, c.W, cip(c), Ho, Wo, cop(c), c.K, c.K, c.stride, c.pad, c.up, dtype_code(dt))))
    finally:
        L.debug_set_conv2d_impl(0)
        L.debug_set_wgrad_impl(0)
    return fwd, forms, dgrad, wgrad


def assert_route_sets(L):
    fwd, forms, dgrad, wgrad = route_sets(L)
    assert fwd == {GATHER, BRICK8, NARROW, BRICK16}, fwd
    for kind in (BRICK8, BRICK16):       # both channel-tile forms (64 and 32 output channels per block) of both brick kernels
        assert {f[1] for f in forms if f[0] == kind} == {True, False}, (kind, forms)
    assert dgrad == {GATHER, BRICK8, NARROW, BRICK16}, dgrad
    # weight gradient: 0 gather, 1 narrow, 2 brick, 3 one kernel row per block under impl 0; the gather kernel alone under impl 1
    assert wgrad == {(0, 0), (0, 1), (0, 2), (0, 3), (1, 0)}, wgrad


# ---------------------------------------------------------------------------------------------------------------------------------------
def _dev():
    return torch.device("cuda:0")


def _act(t, dt, pad_to=0):
    from pcrlv2_amd import ops2d
    return ops2d.to_act2(t.to(dt).to(_dev()), dt, pad_to=pad_to)


class _impl:
    """conv2d / wgrad test hooks for the block; always back to 0"""

    def __init__(self, conv2d=0, wgrad=0):
        self.c, self.w = conv2d, wgrad

    def __enter__(self):
        from pcrlv2_amd._lib import lib
        lib().debug_set_conv2d_impl(self.c)
        lib().debug_set_wgrad_impl(self.w)

    def __exit__(self, *a):
        from pcrlv2_amd._lib import lib
        lib().debug_set_conv2d_impl(0)
        lib().debug_set_wgrad_impl(0)


def _check_stats(partial, rows, Co, R, what):
    st = partial.view(rows, Co, 2)
    X.assert_rows_exact(st[:, :, 0], R.y.sum((0, 2, 3)), what + " statistics: sum y")
    if R.lat == "ternary":
        X.assert_rows_exact(st[:, :, 1], (R.y * R.y).sum((0, 2, 3)), what + " statistics: sum y^2")


def test_case_list_reaches_every_route():
    """Forward kinds {0, 1, 2, 3} with both channel-tile forms of both brick kernels, data-gradient kinds {0, 1, 2, 3}, and every answer of the
    weight gradient's route under its impl 0 and 1 (no launch: the queries the dispatchers themselves go through)."""
    from pcrlv2_amd._lib import lib
    assert_route_sets(lib())


@pytest.mark.parametrize("run", runs(), ids=run_id)
def test_conv2d_fwd(run):
    """pcrl_conv2d_fwd: y (bf16, float32, `out_f32`) and the statistics rows, summed over the rows in float64, bit for bit; the route asserted."""
    from pcrlv2_amd import ops2d
    from pcrlv2_amd._lib import dtype_code, lib
    c, dt, impl = run
    with _impl(impl):
        kind = lib().call("pcrl_conv2d_fwd_kind", c.N, c.H, c.W, cip(c), c.Co, c.K, c.K, c.stride, c.pad, c.up, c.out_f32, dtype_code(dt))
        assert kind == expected_kind(c, dt, impl)
        for lat in ("fine", "ternary"):
            R = reference(c, lat)
            xa = _act(R.x, dt, pad_to=8 if c.Ci < 8 else 0)
            y, partial, rows = ops2d.conv2d_forward(xa, R.w.float().to(_dev()), None if R.b is None else R.b.float().to(_dev()), ops2d.PackedConv2d(),
                                                    c.stride, c.pad, c.up, dt, want_stats=not c.out_f32, out_f32=bool(c.out_f32))
            what = f"conv2d fwd {run_id(run)} [{lat}] kind {kind}"
            X.assert_bit_equal(y, R.y, F32 if c.out_f32 else dt, what, brick=BRICKS[kind])
            if not c.out_f32:
                _check_stats(partial, rows, c.Co, R, what)


@pytest.mark.parametrize("run", runs([c for c in CASES if not c.out_f32]), ids=run_id)
def test_conv2d_fwd_affine(run):
    """pcrl_conv2d_fwd_affine on the same routes: ReLU and none, with and without residual (a wide-brick call WITH a residual is computed by the gather
    kernel), scale in {0.5, 1, 2}, shift and residual on the lattice -- the epilogue is exact too.  The output buffer is pre-filled with NaN."""
    from pcrlv2_amd import ops2d
    from pcrlv2_amd._lib import ACT_NONE, ACT_RELU, dtype_code, lib, stream_handle
    c, dt, impl = run
    R, A = reference(c, "fine"), affine_reference(c)
    Ho, Wo = out_dims(c)
    L = lib()
    xa = _act(R.x, dt, pad_to=8 if c.Ci < 8 else 0)
    wf, _ = ops2d.PackedConv2d().get(R.w.float().to(_dev()), dt, cip(c))
    bias = None if R.b is None else R.b.float().to(_dev())
    scale, shift, ra = A.scale.float().to(_dev()), A.shift.float().to(_dev()), _act(A.res, dt)
    with _impl(impl):
        kind = L.call("pcrl_conv2d_fwd_kind", c.N, c.H, c.W, cip(c), c.Co, c.K, c.K, c.stride, c.pad, c.up, 0, dtype_code(dt))
        assert kind == expected_kind(c, dt, impl)
        for act in (ACT_RELU, ACT_NONE):
            for with_res in (False, True):
                fused = L.call("pcrl_conv2d_fwd_affine_fused", c.N, c.H, c.W, cip(c), c.Co, c.K, c.K, c.stride, c.pad, c.up, int(with_res), dtype_code(dt))
                assert fused == int(not (kind == BRICK16 and with_res))
                ref = A.z + A.res if with_res else A.z
                ref = torch.relu(ref) if act == ACT_RELU else ref
                a = ops2d.new_act2(c.N, Ho, Wo, c.Co, dt, _dev())
                a.fill_(float("nan"))
                L.call("pcrl_conv2d_fwd_affine", xa, wf, bias, scale, shift, ra if with_res else None, a, c.N, c.H, c.W, cip(c), c.Co, c.K, c.K,
                       c.stride, c.pad, c.up, act, dtype_code(dt), stream_handle())
                X.assert_bit_equal(a, ref, dt, f"conv2d fwd_affine {run_id(run)} act={act} residual={with_res} kind {kind if fused else GATHER}",
                                   brick=BRICKS[kind if fused else GATHER])


@pytest.mark.parametrize("run", runs(), ids=run_id)
def test_conv2d_backward(run):
    """ops2d.conv2d_backward: the data gradient by the route the case takes -- pcrl_conv2d_dgrad (kind asserted), the four parity classes of
    pcrl_conv2d_dgrad_s2 (3x3; class (0, 0) over a zero-filled dx for 1x1), pcrl_conv2d_dgrad_up -- and pcrl_conv2d_wgrad under wgrad impl 0 and 1.

    An upsampled source WITHOUT pcrl_conv2d_dgrad_up runs two kernels with a stored intermediate: pcrl_conv2d_dgrad writes the fine-resolution
    gradient in the activation dtype, pcrl_upsample2d_nearest2_bwd sums its 2 x 2 blocks.  In bf16 that path rounds TWICE (the reference rounds the
    fine-resolution gradient to bf16 before the 2 x 2 sum); the fused pcrl_conv2d_dgrad_up rounds ONCE, after the sum ("Exact-lattice pins")."""
    from pcrlv2_amd import ops2d
    from pcrlv2_amd._lib import dtype_code, lib
    c, dt, impl = run
    L = lib()
    R = reference(c, "fine")
    Ho, Wo = out_dims(c)
    Hl, Wl = (2 * c.H, 2 * c.W) if c.up else (c.H, c.W)
    xa = _act(R.x, dt, pad_to=8 if c.Ci < 8 else 0)
    dya = _act(R.dy, dt, pad_to=8 if c.Co < 8 else 0)
    wd = R.w.float().to(_dev())
    names = ("pcrl_conv2d_dgrad", "pcrl_conv2d_dgrad_s2", "pcrl_conv2d_dgrad_up", "pcrl_upsample2d_nearest2_bwd", "pcrl_zero")
    for wimpl in (0, 1):
        with _impl(impl, wimpl):
            wkind = L.call("pcrl_conv2d_wgrad_kind", c.N, c.H, c.W, cip(c), Ho, Wo, cop(c), c.K, c.K, c.stride, c.pad, c.up, dtype_code(dt))
            dkind = L.call("pcrl_conv2d_dgrad_kind", c.N, Hl, Wl, c.Ci, Ho, Wo, cop(c), c.K, c.K, c.stride, c.pad, dtype_code(dt))
            up_ok = bool(c.up) and bool(L.call("pcrl_conv2d_dgrad_up_ok", c.N, c.H, c.W, c.Ci, cop(c), dtype_code(dt)))
            with L.count_calls(*names) as n:
                dx, dw = ops2d.conv2d_backward(xa, dya, wd, ops2d.PackedConv2d(), c.stride, c.pad, c.up, dt, need_dx=wimpl == 0)
            ops2d.ops.join_side_stream()
        assert wimpl == 0 or wkind == 0
        X.assert_bit_equal(dw, R.dw, F32, f"conv2d wgrad {run_id(run)} wgrad impl {wimpl} kind {wkind}")
        if wimpl:
            continue
        path = dgrad_path(c)
        dx_ref, brick = R.dx, None
        if path == "s2":
            assert dict(n) == ({"pcrl_conv2d_dgrad_s2": 4} if c.K == 3 else {"pcrl_conv2d_dgrad_s2": 1, "pcrl_zero": 1}), dict(n)
        elif path == "up" and up_ok:
            assert dict(n) == {"pcrl_conv2d_dgrad_up": 1}, dict(n)
            brick = BRICKS[NARROW]
        elif path == "up":
            assert dict(n) == {"pcrl_conv2d_dgrad": 1, "pcrl_upsample2d_nearest2_bwd": 1}, dict(n)
            fine = R.dx_fine.to(dt).double()          # the stored intermediate: rounded to the activation dtype
            dx_ref = fine.view(c.N, c.Ci, c.H, 2, c.W, 2).sum((3, 5))
        else:
            assert dict(n) == {"pcrl_conv2d_dgrad": 1}, dict(n)
            brick = BRICKS[dkind]
        X.assert_bit_equal(dx[:, :c.Ci], dx_ref, dt, f"conv2d dgrad {run_id(run)} path {path} dgrad kind {dkind}", brick=brick)


@pytest.mark.parametrize("c", [c for c in CASES if c.kind == BRICK16], ids=case_id)
def test_conv2d_dgrad_bnred_dx(c):
    """The dx of pcrl_conv2d_dgrad_bnred (wide brick, bf16) bit for bit; its reduction rows stay with tests/test_dgrad_bnred_gpu.py."""
    from pcrlv2_amd import ops2d
    from pcrlv2_amd._lib import ACT_RELU, dtype_code, lib, stream_handle
    L, R = lib(), reference(c, "fine")
    rows = L.call("pcrl_conv2d_dgrad_bnred_rows", c.N, c.H, c.W, c.Ci, c.Co, ACT_RELU, dtype_code(BF))
    assert rows == c.N * c.H * c.W // 512
    g = torch.Generator().manual_seed(c.H)
    _, wd = ops2d.PackedConv2d().get(R.w.float().to(_dev()), BF, c.Ci)
    coef = [(torch.rand(c.Ci, generator=g) + 0.5).to(_dev()) for _ in range(4)]       # scale, shift, mean, rstd of the layer below: they do not enter dx
    dx = ops2d.new_act2(c.N, c.H, c.W, c.Ci, BF, _dev())
    dx.fill_(float("nan"))
    part = torch.empty(rows * c.Ci * 2, dtype=F32, device=_dev())
    L.call("pcrl_conv2d_dgrad_bnred", _act(R.dy, BF), wd, dx, _act(R.x, BF), coef[0], coef[1], coef[2], coef[3], part, c.N, c.H, c.W, c.Ci, c.Co,
           ACT_RELU, dtype_code(BF), stream_handle())
    X.assert_bit_equal(dx, R.dx, BF, f"conv2d dgrad_bnred dx {case_id(c)}", brick=BRICKS[BRICK16])


@pytest.mark.parametrize("c", STEM_CASES, ids=case_id)
def test_stem7_fwd_and_wgrad(c):
    """pcrl_stem7_fwd (output and statistics rows) and pcrl_stem7_wgrad on the float32 NCHW image, and the gather kernel on the image padded to 8
    channels: all three against the same float64 reference, bit for bit."""
    from pcrlv2_amd import ops2d
    for lat in ("fine", "ternary"):
        R = reference(c, lat)
        xd, wd = R.x.float().to(_dev()), R.w.float().to(_dev())
        assert ops2d.stem_ok(xd, wd, BF)
        y, partial, rows = ops2d.stem_forward(xd, wd, ops2d.PackedStem(), BF)
        X.assert_bit_equal(y, R.y, BF, f"stem7 fwd {case_id(c)} [{lat}]", brick={"h": 8, "w": 32})
        _check_stats(partial, rows, 64, R, f"stem7 fwd {case_id(c)} [{lat}]")
        dw = ops2d.stem_wgrad(xd, _act(R.dy, BF), wd, BF)
        ops2d.ops.join_side_stream()
        X.assert_bit_equal(dw, R.dw, F32, f"stem7 wgrad {case_id(c)} [{lat}]")
        y2, partial2, rows2 = ops2d.conv2d_forward(ops2d.image_to_act(xd, BF, 8), wd, None, ops2d.PackedConv2d(), 2, 3, 0, BF)
        X.assert_bit_equal(y2, R.y, BF, f"stem through the gather kernel {case_id(c)} [{lat}]")
        _check_stats(partial2, rows2, 64, R, f"stem through the gather kernel {case_id(c)} [{lat}]")


@functools.lru_cache(maxsize=None)
def small_bwd_reference(Ci, N, H, W):
    g = torch.Generator().manual_seed(Ci + H)
    x, w, dy = X.lattice((N, Ci, H, W), 4, 4, g), X.lattice((3, Ci, 1, 1), 2, 8, g), X.lattice((N, 3, H, W), 4, 4, g)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    br = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    F.conv2d(xr, wr, br).backward(dy)
    what = f"1x1 -> 3 backward {(Ci, N, H, W)}"
    X.assert_exactly_summable(F.conv_transpose2d(dy.abs(), w.abs()), X.unit(4, 8), what + " dx")
    X.assert_exactly_summable(torch.einsum("nchw,nkhw->kc", x.abs(), dy.abs()), X.unit(4, 4), what + " dw")
    X.assert_exactly_summable(dy.abs().sum((0, 2, 3)), X.unit(4), what + " db")
    return types.SimpleNamespace(x=x, w=w, dy=dy, dx=xr.grad, dw=wr.grad, db=br.grad)


@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SMALL_BWD_CASES, ids=lambda s: "x".join(map(str, s)))
def test_conv1x1_small_backward(shape, dt):
    """pcrl_conv2d_1x1_small_bwd: dx (activation dtype), dw and db (float32, block partials + pcrl_colsum) bit for bit."""
    from pcrlv2_amd import ops2d
    R = small_bwd_reference(*shape)
    dx, dw, db = ops2d.conv1x1_small_backward(_act(R.x, dt), _act(R.dy, F32), R.w.float().to(_dev()), dt)
    X.assert_bit_equal(dx, R.dx, dt, f"1x1 -> 3 dx {shape}")
    X.assert_bit_equal(dw, R.dw, F32, f"1x1 -> 3 dw {shape}")
    X.assert_bit_equal(db, R.db, F32, f"1x1 -> 3 db {shape}")
