"""3D path: the 3x3x3 convolution kernels bit for bit against float64 torch on exactly summable operands (tests/exact_lattice.py; the 2D counterpart
is tests/test_conv2d_exact_gpu.py, which explains the method).  pcrl_conv3d_k3_fwd and the data gradient (the same entry with the transposed pack)
under every conv test-hook code defined for the shape, pcrl_conv3d_k3_fwd_affine, the first layer (pcrl_conv3d_k3_c1_fwd, _c1_fwd_affine, _c1_wgrad)
and pcrl_conv3d_k3_wgrad under the impl / tr pairs of tests/test_ops_gpu.py::test_conv3d_fwd_stats_dgrad_wgrad.

The one-channel convolutions and the transposed convolution are pinned the same way by tests/test_conv_to1_exact_gpu.py and
tests/test_convt_exact_gpu.py (cases: tests/conv1_cases.py), and the composed up-convolution by tests/test_upconv_exact_gpu.py (cases:
tests/upconv_cases.py): its phase weights are sums of products of the two layers' weights, and a sparse transposed convolution keeps them on a lattice
of bf16 values."""
import collections
import functools
import types

import pytest
import torch
import torch.nn.functional as F

import exact_lattice as X

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
DEV = "cuda"
GATHER, BRICK8, BRICK16 = 0, 1, 2      # pcrl_conv3d_k3_fwd_kernel

# auto: the kernel pcrl_conv3d_k3_fwd_kernel names in bf16 under conv impl 0; b8: under impl 4 (the 4x8x8-brick kernel wherever it is eligible).  Both asserted.
Shape = collections.namedtuple("Shape", "N D H W Ci Co auto b8")
SHAPES = [
    Shape(3, 6, 5, 7, 32, 64, GATHER, GATHER),         # generic gather: M not a multiple of 128
    Shape(2, 8, 16, 8, 64, 64, BRICK16, BRICK8),       # 4x8x8 bricks under impl 3 / 4 (two bricks in d and h); the wide brick's permuted axes under 0 / 5 / 6
    Shape(1, 8, 16, 32, 32, 64, BRICK16, BRICK8),      # wide brick: two bricks in every direction
    Shape(3, 4, 16, 8, 64, 64, BRICK16, BRICK8),       # wide brick on permuted axes (H % 16 == 0, W % 8 == 0), D % 8 != 0
    Shape(2, 8, 8, 4, 64, 128, BRICK8, BRICK8),        # innermost 4-deep axis
    Shape(2, 8, 16, 16, 64, 128, BRICK16, BRICK8),     # several channel tiles
    Shape(40, 2, 2, 2, 64, 64, GATHER, GATHER),        # voxel-major gather
    Shape(33, 2, 2, 1, 64, 32, GATHER, GATHER),        # voxel-major gather, tiles of one and two voxels
]
WGRAD_HOOKS = ((0, 1), (6, 1), (2, 1), (1, 1), (1, 0))      # (wgrad impl, tr) of test_conv3d_fwd_stats_dgrad_wgrad; float32: (0, 1) only
# first layer (Ci = 1): N, D, H, W, Co -- the float32-FMA kernel (any shape) and the bf16 MFMA brick kernel (D % 4 == H % 8 == W % 8 == 0), Co 32 and 64
C1_SHAPES = [(3, 6, 5, 7, 32), (2, 8, 16, 24, 32), (2, 8, 16, 24, 64)]


def shape_id(s):
    return "x".join(str(int(v)) for v in s[:6])


def impl_codes(s, dt):
    if dt != BF:
        return [0, 1]
    return [0, 1] + ([3, 4] if s.b8 == BRICK8 else []) + ([5, 6] if s.auto == BRICK16 else [])


def expected_kernel(s, dt, impl):
    if dt != BF or impl == 1:
        return GATHER
    return s.b8 if impl in (3, 4) else s.auto


def runs():
    return [(s, dt, impl) for s in SHAPES for dt in (F32, BF) for impl in impl_codes(s, dt)]


def run_id(r):
    return f"{shape_id(r[0])}-{'bf16' if r[1] == BF else 'f32'}-impl{r[2]}"


@functools.lru_cache(maxsize=None)
def reference(N, D, H, W, Ci, Co, lat_name):
    """Operands on the lattice, the float64 forward / data gradient / weight gradient (torch autograd), and the preconditions from the same graph on
    the absolute values.  Ci = 1: the first layer."""
    lat = X.fine_for(27 * Ci) if lat_name == "fine" else X.TERNARY
    g = torch.Generator().manual_seed(N * 7 + D * 5 + H * 3 + W + Ci + Co + (0 if lat_name == "fine" else 7919))
    x = X.lattice((N, Ci, D, H, W), *lat["x"], g)
    w = X.lattice((Co, Ci, 3, 3, 3), *lat["w"], g)
    b = X.lattice((Co,), *lat["b"], g)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv3d(xr, wr, b, padding=1)
    dy = X.lattice(y.shape, *lat["dy"], g)
    y.backward(dy)
    xa, wa = x.abs().requires_grad_(True), w.abs().requires_grad_(True)
    ya = F.conv3d(xa, wa, b.abs(), padding=1)
    ya.backward(dy.abs())
    R = types.SimpleNamespace(x=x, w=w, b=b, y=y.detach(), dy=dy, dx=xr.grad, dw=wr.grad, y_abs=ya.detach(), dx_abs=xa.grad, dw_abs=wa.grad, lat=lat_name,
                              u_fwd=X.unit(lat["x"][1], lat["w"][1]))
    u_fwd, u_dx, u_dw = X.unit(lat["x"][1], lat["w"][1]), X.unit(lat["dy"][1], lat["w"][1]), X.unit(lat["x"][1], lat["dy"][1])
    what = f"{(N, D, H, W, Ci, Co)} [{lat_name}]"
    X.assert_exactly_summable(R.y_abs, u_fwd, what + " forward")
    X.assert_exactly_summable(R.dx_abs, u_dx, what + " data gradient")
    X.assert_exactly_summable(R.dw_abs, u_dw, what + " weight gradient")
    X.assert_exactly_summable(R.y.abs().sum((0, 2, 3, 4)), u_fwd, what + " statistics: sum y over the channel")
    if lat_name == "ternary":
        X.assert_exactly_summable((R.y * R.y).sum((0, 2, 3, 4)), u_fwd * u_fwd, what + " statistics: sum y^2 over the channel")
    return R


@functools.lru_cache(maxsize=None)
def affine_reference(N, D, H, W, Ci, Co):
    """scale in {0.5, 1, 2}, shift on the lattice: z = scale * y + shift stays on multiples of half the forward's unit and exactly summable."""
    R = reference(N, D, H, W, Ci, Co, "fine")
    g = torch.Generator().manual_seed(1000 + N + D + H + W + Ci + Co)
    scale = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (Co,), generator=g)]
    shift = X.lattice((Co,), 4, 4, g)
    sv, hv = scale.view(1, -1, 1, 1, 1), shift.view(1, -1, 1, 1, 1)
    X.assert_exactly_summable(sv * R.y_abs + hv.abs(), R.u_fwd / 2, f"{(N, D, H, W, Ci, Co)} affine epilogue")
    return types.SimpleNamespace(scale=scale, shift=shift, z=sv * R.y + hv)


def kernel_sets(L):
    """Host only (no launch): (impl codes, kernels) the run list reaches; every run's kernel equals the case list's expectation, for the forward and
    for the data gradient (channels exchanged).  L: pcrlv2_amd._lib.lib()."""
    from pcrlv2_amd._lib import dtype_code
    codes, kernels = set(), set()
    try:
        for s, dt, impl in runs():
            L.debug_set_conv_impl(impl)
            k = L.call("pcrl_conv3d_k3_fwd_kernel", s.N, s.D, s.H, s.W, s.Ci, s.Co, dtype_code(dt))
            kd = L.call("pcrl_conv3d_k3_fwd_kernel", s.N, s.D, s.H, s.W, s.Co, s.Ci, dtype_code(dt))
            assert k == kd == expected_kernel(s, dt, impl), (s, dt, impl, k, kd)
            codes.add(impl)
            kernels.add((impl, k))
    finally:
        L.debug_set_conv_impl(0)
    return codes, kernels


def assert_kernel_sets(L):
    codes, kernels = kernel_sets(L)
    assert codes == {0, 1, 3, 4, 5, 6}, codes
    assert kernels == {(0, GATHER), (0, BRICK8), (0, BRICK16), (1, GATHER), (3, BRICK8), (4, BRICK8), (5, BRICK16), (6, BRICK16)}, kernels


# ---------------------------------------------------------------------------------------------------------------------------------------
def _act(t, dt):
    from pcrlv2_amd import ops
    return ops.to_act(t.to(dt).to(DEV), dt)


def _brick(kernel):
    return {GATHER: None, BRICK8: {"d": 4, "h": 8, "w": 8}, BRICK16: {"d": 4, "h": 8, "w": 16}}[kernel]


def _check_stats(part, rows, Co, R, what):
    st = part.view(rows, Co, 2)
    X.assert_rows_exact(st[:, :, 0], R.y.sum((0, 2, 3, 4)), what + " statistics: sum y")
    if R.lat == "ternary":
        X.assert_rows_exact(st[:, :, 1], (R.y * R.y).sum((0, 2, 3, 4)), what + " statistics: sum y^2")


def test_run_list_reaches_every_kernel_code():
    from pcrlv2_amd._lib import lib
    assert_kernel_sets(lib())


@pytest.mark.parametrize("run", runs(), ids=run_id)
def test_conv3d_fwd_and_dgrad(run):
    """pcrl_conv3d_k3_fwd: output (with bias), statistics rows and the data gradient bit for bit; the kernel that runs is asserted."""
    from pcrlv2_amd import ops
    from pcrlv2_amd._lib import dtype_code, lib, stream_handle
    s, dt, impl = run
    N, D, H, W, Ci, Co = s[:6]
    L, st, dc = lib(), stream_handle(), dtype_code(dt)
    L.debug_set_conv_impl(impl)
    try:
        kernel = L.call("pcrl_conv3d_k3_fwd_kernel", N, D, H, W, Ci, Co, dc)
        assert kernel == expected_kernel(s, dt, impl) == L.call("pcrl_conv3d_k3_fwd_kernel", N, D, H, W, Co, Ci, dc)
        for lat in ("fine", "ternary"):
            R = reference(N, D, H, W, Ci, Co, lat)
            wf, wd = ops.PackedWeights("conv3").get(R.w.float().to(DEV), dt)
            rows = L.call("pcrl_conv3d_k3_stats_rows", N, D, H, W, Ci, Co, dc)
            y = ops.new_act(N, D, H, W, Co, dt, DEV)
            y.fill_(float("nan"))
            part = torch.full((rows * Co * 2,), float("nan"), dtype=F32, device=DEV)
            L.call("pcrl_conv3d_k3_fwd", _act(R.x, dt), wf, R.b.float().to(DEV), y, part, N, D, H, W, Ci, Co, dc, st)
            what = f"conv3d fwd {run_id(run)} [{lat}] kernel {kernel}"
            X.assert_bit_equal(y, R.y, dt, what, brick=_brick(kernel))
            _check_stats(part, rows, Co, R, what)
            dx = ops.new_act(N, D, H, W, Ci, dt, DEV)
            dx.fill_(float("nan"))
            L.call("pcrl_conv3d_k3_fwd", _act(R.dy, dt), wd, None, dx, None, N, D, H, W, Co, Ci, dc, st)
            X.assert_bit_equal(dx, R.dx, dt, f"conv3d dgrad {run_id(run)} [{lat}] kernel {kernel}", brick=_brick(kernel))
    finally:
        L.debug_set_conv_impl(0)


@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("s", SHAPES, ids=shape_id)
def test_conv3d_fwd_affine(s, dt):
    """pcrl_conv3d_k3_fwd_affine (wide brick where the forward takes it, else the gather kernel in one pass; impl 1: the gather kernel everywhere):
    ReLU and none, scale in {0.5, 1, 2} and shift on the lattice -- the epilogue is exact too."""
    from pcrlv2_amd import ops
    from pcrlv2_amd._lib import ACT_NONE, ACT_RELU, dtype_code, lib, stream_handle
    N, D, H, W, Ci, Co = s[:6]
    L, dc = lib(), dtype_code(dt)
    R, A = reference(N, D, H, W, Ci, Co, "fine"), affine_reference(N, D, H, W, Ci, Co)
    wf, _ = ops.PackedWeights("conv3").get(R.w.float().to(DEV), dt)
    xa, bias, scale, shift = _act(R.x, dt), R.b.float().to(DEV), A.scale.float().to(DEV), A.shift.float().to(DEV)
    try:
        for impl in ((0, 1) if (dt == BF and s.auto == BRICK16) else (0,)):
            L.debug_set_conv_impl(impl)
            kernel = L.call("pcrl_conv3d_k3_fwd_kernel", N, D, H, W, Ci, Co, dc)
            for act in (ACT_RELU, ACT_NONE):
                a = ops.new_act(N, D, H, W, Co, dt, DEV)
                a.fill_(float("nan"))
                L.call("pcrl_conv3d_k3_fwd_affine", xa, wf, bias, scale, shift, a, None, 0, N, D, H, W, Ci, Co, act, dc, stream_handle())
                X.assert_bit_equal(a, torch.relu(A.z) if act == ACT_RELU else A.z, dt, f"conv3d fwd_affine {shape_id(s)} {dt} impl {impl} act {act}",
                                   brick=_brick(kernel if kernel == BRICK16 else GATHER))
    finally:
        L.debug_set_conv_impl(0)


@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("s", SHAPES, ids=shape_id)
def test_conv3d_wgrad(s, dt):
    """pcrl_conv3d_k3_wgrad (float32 out: split-K partials + a fixed-order second pass, all exact) under every (impl, tr) pair."""
    from pcrlv2_amd import ops
    from pcrlv2_amd._lib import dtype_code, lib, stream_handle
    N, D, H, W, Ci, Co = s[:6]
    L = lib()
    R = reference(N, D, H, W, Ci, Co, "fine")
    xa, dya = _act(R.x, dt), _act(R.dy, dt)
    nb = L.call("pcrl_conv3d_k3_wgrad_ws_bytes", N, D, H, W, Ci, Co)
    try:
        for impl, tr in (WGRAD_HOOKS if dt == BF else ((0, 1),)):
            L.debug_set_wgrad_impl(impl)
            L.debug_set_wgrad_tr(tr)
            dw = torch.full((Co, Ci, 3, 3, 3), float("nan"), dtype=F32, device=DEV)
            L.call("pcrl_conv3d_k3_wgrad", xa, dya, dw, ops.workspace(nb, xa.device), nb, N, D, H, W, Ci, Co, dtype_code(dt), stream_handle())
            X.assert_bit_equal(dw, R.dw, F32, f"conv3d wgrad {shape_id(s)} {dt} impl={impl} tr={tr}")
    finally:
        L.debug_set_wgrad_tr(1)
        L.debug_set_wgrad_impl(0)


@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", C1_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_first_layer_c1(shape, dt):
    """pcrl_conv3d_k3_c1_fwd (output, statistics rows), _c1_fwd_affine and _c1_wgrad on the float32 scalar field: the float32-FMA kernel and, in bf16
    on brick volumes, the MFMA brick kernel (one statistics row per 4x8x8 brick)."""
    from pcrlv2_amd import ops
    from pcrlv2_amd._lib import ACT_NONE, ACT_RELU, dtype_code, lib, stream_handle
    N, D, H, W, Co = shape
    L, dc, st = lib(), dtype_code(dt), stream_handle()
    brick = dt == BF and D % 4 == 0 and H % 8 == 0 and W % 8 == 0
    rows = L.call("pcrl_conv3d_k3_c1_stats_rows", N, D, H, W, Co, dc)
    assert rows == (N * (D // 4) * (H // 8) * (W // 8) if brick else (N * D * H * W + 127) // 128)
    bk = {"d": 4, "h": 8, "w": 8} if brick else None
    for lat in ("fine", "ternary"):
        R = reference(N, D, H, W, 1, Co, lat)
        xd, wd, bd = R.x.float().to(DEV).contiguous(), R.w.float().to(DEV), R.b.float().to(DEV)
        y = ops.new_act(N, D, H, W, Co, dt, DEV)
        y.fill_(float("nan"))
        part = torch.full((rows * Co * 2,), float("nan"), dtype=F32, device=DEV)
        L.call("pcrl_conv3d_k3_c1_fwd", xd, wd, bd, y, part, N, D, H, W, Co, dc, st)
        what = f"c1 fwd {shape} {dt} [{lat}]"
        X.assert_bit_equal(y, R.y, dt, what, brick=bk)
        _check_stats(part, rows, Co, R, what)
        nb = L.call("pcrl_conv3d_k3_c1_wgrad_ws_bytes", N, D, H, W, Co)
        dw = torch.full((Co, 1, 3, 3, 3), float("nan"), dtype=F32, device=DEV)
        L.call("pcrl_conv3d_k3_c1_wgrad", xd, _act(R.dy, dt), dw, ops.workspace(nb, xd.device), nb, N, D, H, W, Co, dc, st)
        X.assert_bit_equal(dw, R.dw, F32, f"c1 wgrad {shape} {dt} [{lat}]")
    R, A = reference(N, D, H, W, 1, Co, "fine"), affine_reference(N, D, H, W, 1, Co)
    xd, wd, bd = R.x.float().to(DEV).contiguous(), R.w.float().to(DEV), R.b.float().to(DEV)
    for act in (ACT_RELU, ACT_NONE):
        a = ops.new_act(N, D, H, W, Co, dt, DEV)
        a.fill_(float("nan"))
        L.call("pcrl_conv3d_k3_c1_fwd_affine", xd, wd, bd, A.scale.float().to(DEV), A.shift.float().to(DEV), a, N, D, H, W, Co, act, dc, st)
        X.assert_bit_equal(a, torch.relu(A.z) if act == ACT_RELU else A.z, dt, f"c1 fwd_affine {shape} {dt} act {act}", brick=bk)
