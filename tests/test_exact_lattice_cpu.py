"""CPU: what the bit-for-bit GPU tests (test_conv2d_exact_gpu.py, test_conv3d_exact_gpu.py) rest on, checked without a GPU for every one of their
cases -- the preconditions hold, torch's own float32 convolution reproduces the float64 one on the lattice operands (forward, data gradient, weight
gradient: the claim "exactly summable => any float32 summation order gives the float64 value"), the case lists reach every route -- and a planted
one-ulp error that assert_bit_equal catches while the old relative-L2 figure stays far below its bound."""
import pytest
import torch
import torch.nn.functional as F

import exact_lattice as X
import test_conv2d_exact_gpu as T2
import test_conv3d_exact_gpu as T3

CASES2 = T2.CASES + T2.STEM_CASES
CASES3 = [tuple(s[:6]) for s in T3.SHAPES] + [(N, D, H, W, 1, Co) for N, D, H, W, Co in T3.C1_SHAPES]


def _f32_equals_f64(conv, R):
    """float32 torch on the same operands: forward, data gradient and weight gradient identical to float64"""
    x, w = R.x.float().requires_grad_(True), R.w.float().requires_grad_(True)
    y = conv(x, w, None if R.b is None else R.b.float())
    y.backward(R.dy.float())
    for got, ref, what in ((y.detach(), R.y, "forward"), (x.grad, R.dx, "data gradient"), (w.grad, R.dw, "weight gradient")):
        assert torch.equal(got.double(), ref), f"float32 {what} differs from float64 at {int((got.double() != ref).sum())} elements"


@pytest.mark.parametrize("lat", ["fine", "ternary"])
@pytest.mark.parametrize("c", CASES2, ids=T2.case_id)
def test_conv2d_cases_are_exactly_summable(c, lat):
    R = T2.reference(c, lat)         # asserts the preconditions: forward, data gradient, weight gradient, statistics rows (sum y; ternary: sum y^2)
    assert R.headroom < 1.0
    _f32_equals_f64(lambda x, w, b: T2._conv(c, x, w, b)[1], R)
    if lat == "fine":
        if not c.out_f32:
            T2.affine_reference(c)
        if not c.out_f32 and c.K == 3:
            # the point of the fine lattice: bf16 rounding changes outputs, and (sums of multiples of 1/32) mostly on ties
            changed = R.y.to(torch.bfloat16).double() != R.y
            assert changed.any(), "no output of this case is changed by bf16 rounding: the rounding mode would go unexercised"
        if c.up:      # the two-kernel path's reference differs from the single rounding somewhere in the list (checked over the list below)
            assert R.dx_fine.shape[-2:] == (2 * c.H, 2 * c.W)


def test_two_roundings_differ_from_one_somewhere():
    """The upsampled-source data gradient as two kernels (bf16 fine-resolution gradient stored, then 2 x 2 sums) against one rounding after the sum:
    the two references differ on the case list, so the GPU test does tell the paths apart."""
    n = 0
    for c in T2.CASES:
        if c.up:
            R = T2.reference(c, "fine")
            twice = R.dx_fine.to(torch.bfloat16).double().view(c.N, c.Ci, c.H, 2, c.W, 2).sum((3, 5)).to(torch.bfloat16)
            n += int((twice != R.dx.to(torch.bfloat16)).sum())
    assert n > 0


@pytest.mark.parametrize("shape", T2.SMALL_BWD_CASES, ids=lambda s: "x".join(map(str, s)))
def test_conv1x1_small_backward_cases_are_exactly_summable(shape):
    R = T2.small_bwd_reference(*shape)
    x, w = R.x.float().requires_grad_(True), R.w.float().requires_grad_(True)
    F.conv2d(x, w).backward(R.dy.float())
    assert torch.equal(x.grad.double(), R.dx) and torch.equal(w.grad.double(), R.dw)


@pytest.mark.parametrize("lat", ["fine", "ternary"])
@pytest.mark.parametrize("shape", CASES3, ids=lambda s: "x".join(map(str, s)))
def test_conv3d_cases_are_exactly_summable(shape, lat):
    R = T3.reference(*shape, lat)
    _f32_equals_f64(lambda x, w, b: F.conv3d(x, w, b, padding=1), R)
    if lat == "fine":
        T3.affine_reference(*shape)
        if shape[1] * shape[2] * shape[3] >= 8:      # (a 2 x 2 x 1 volume sums 4 taps only: its outputs are all bf16 values)
            assert (R.y.to(torch.bfloat16).double() != R.y).any(), "no output of this case is changed by bf16 rounding"


def test_case_lists_reach_every_route():
    """The route queries are host code: the forward / data-gradient kinds {0, 1, 2, 3}, both channel-tile forms of both brick kernels, every
    weight-gradient route and every listed 3D kernel code are reached by the case lists (the GPU files assert the same before they launch)."""
    from pcrlv2_amd import _lib
    import os
    if not os.path.exists(_lib.LIBPATH):
        import __graft_entry__ as g
        g.build()
    L = _lib.lib()
    T2.assert_route_sets(L)
    T3.assert_kernel_sets(L)


def test_lattice_and_precondition_helpers():
    g = torch.Generator().manual_seed(0)
    t = X.lattice((1000,), 4, 4, g)
    assert t.dtype == torch.float64 and set((t * 4).tolist()) == set(range(-4, 5))
    with pytest.raises(AssertionError):
        X.lattice((1000,), 300, 1, g)                    # 257 ... 300 are not bf16 values
    X.assert_exactly_summable(torch.tensor([2.0 ** 24 - 1]), 1.0)
    with pytest.raises(AssertionError, match="not exactly summable"):
        X.assert_exactly_summable(torch.tensor([2.0 ** 24]), 1.0)
    with pytest.raises(AssertionError, match="not exactly summable"):
        X.assert_exactly_summable(torch.tensor([1.0, 2.0 ** 19]), 1 / 32)


def test_one_planted_ulp_is_caught_where_relative_l2_sees_nothing():
    """One single element of a 4 x 64 x 24 x 48 tensor (test_conv2d_brick_path's size) moved by one bf16 ulp: assert_bit_equal raises and names the
    element; the old assertion's figure, rel-L2 against the float64 reference, stays far below its 6e-3 bound -- and ten completely wrong elements
    still pass it."""
    c = T2.Case(4, 32, 64, 3, 1, 1, 0, 24, 48, 0, 0, T2.BRICK16)
    R = T2.reference(c, "fine")
    good = R.y.to(torch.bfloat16)
    X.assert_bit_equal(good, R.y, torch.bfloat16, "unchanged")
    idx = (3, 63, 23, 47)          # the last channel of the corner pixel of the last brick
    bad = good.clone()
    bits = bad.view(torch.int16)
    bits[idx] += 1                 # one ulp away from zero
    with pytest.raises(AssertionError) as e:
        X.assert_bit_equal(bad, R.y, torch.bfloat16, "planted", brick={"n": 4, "h": 8, "w": 16})
    msg = str(e.value)
    assert "1 of 294912 elements differ" in msg and "(n=3, c=63, h=23, w=47)" in msg and "tensor border: h,w" in msg and "brick border: n,h,w" in msg, msg
    rel = float((bad.double() - R.y).norm() / R.y.norm())
    clean = float((good.double() - R.y).norm() / R.y.norm())
    assert rel < 6e-3 / 2 and rel - clean < 1e-5, (rel, clean)       # invisible to the old bound
    worse = good.clone()
    worse[0, :10, 0, 0] = 0.0                                          # ten outputs lost outright
    with pytest.raises(AssertionError, match="elements differ"):
        X.assert_bit_equal(worse, R.y, torch.bfloat16, "ten wrong")
    assert float((worse.double() - R.y).norm() / R.y.norm()) < 6e-3
    # float32 outputs and NaN (a never-written element) are caught the same way
    f = R.y.float()
    f[1, 2, 3, 4] = float("nan")
    with pytest.raises(AssertionError, match="NaN"):
        X.assert_bit_equal(f, R.y, torch.float32, "nan")
