"""csrc/encoder2d.hip, csrc/ops2d.hip and csrc/heads2d.hip at their edges: the fused BasicBlock tail and its backward mask, the fused stem
pool and both pool backwards, the two upsamplers, the 3-channel MSE, its padded backward, the one-pass backward of the 1x1 convolution to
3 channels and the image transpose -- at the sizes where a kernel changes path: rc_grid()'s 2048 blocks for every slot count, grid_for()'s
16 384 blocks, the 65 536 blocks of the transpose, ROWS_PER_BLOCK = 1024, the `i + 768 < blocks` unroll of the MSE finish, the unroll-4 /
unroll-2 row loops and pcrl_streaming()'s 192 MiB.

The case table, the lattices and the restatements are in ops2d_cases.py, their preconditions are asserted by test_ops2d_cases_cpu.py.
Every comparison is on BITS at every element against the float64 restatement (or its round-to-nearest-even rounding to bf16), with these
exceptions and no other:
  zero sign   where the reference is a matrix product (bilinear, conv1x1 dx) a zero of either sign equals a zero
  derived     odd-scale bilinear forward: 8 * 2^-24 * sum |w x| per element; the float32 column partials of pcrl_mse2d_bwd_pad:
              (rows - 1) * 2^-24 * sum |stored| per block and column (the any-order bound of a float32 sum)
Inputs sit in front of poison rows, outputs in front of a sentinel that must survive.  Cases above a few MB are generated, restated and
compared on the device.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import ops2d_cases as oc  # noqa: E402
from ops2d_cases import BF16, F32  # noqa: E402
from pcrlv2_amd import ops, ops2d  # noqa: E402
from pcrlv2_amd._lib import ACT_NONE, ACT_RELU, PcrlError, dtype_code, lib, stream_handle  # noqa: E402

DEV = "cuda"
SENT = -768.0          # a bf16 value no case reaches
POISON = 96.0          # finite, a bf16 value, far outside the lattices: a row read past the end moves a sum or an output
TAIL = 64
DTYPES = [F32, BF16]
NC = lambda dt: ((1, oc.vec(dt)), (3, 64))      # noqa: E731  (N, C): one channel vector, and 64 channels in three images


def call(name, *args):
    return lib().call(name, *args, stream_handle())


def outbuf(n, dt):
    return torch.full((n + TAIL,), SENT, dtype=dt, device=DEV)


def tail_kept(buf, n, what):
    torch.cuda.synchronize()
    assert bool((buf[n:] == SENT).all()), f"{what}: the elements behind the output were written"


def guarded(t, extra=4096):
    """a contiguous copy of t followed in memory by `extra` elements of POISON"""
    buf = torch.full((t.numel() + extra,), POISON, dtype=t.dtype, device=DEV)
    buf[:t.numel()] = t.reshape(-1).to(DEV)
    return buf[:t.numel()].view(t.shape)


def eq(got, want, what, bits=True):
    """device comparison on the bit views (NaN equals NaN); bits=False: zeros of either sign are equal.  Only the count and the first
    mismatches come back."""
    torch.cuda.synchronize()
    got, want = got.reshape(-1), want.reshape(-1).to(got.device)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    it = {BF16: torch.int16, F32: torch.int32, torch.uint8: torch.uint8}[got.dtype]
    if torch.equal(got.view(it), want.view(it)):
        return
    same = got.view(it) == want.view(it)
    if got.dtype != torch.uint8:
        same |= got.isnan() & want.isnan()
        if not bits:
            same |= (got == 0) & (want == 0)
    bad = (~same).nonzero().flatten()
    if bad.numel():
        first = [(int(i), float(got[i]), float(want[i])) for i in bad[:6]]
        raise AssertionError(f"{what}: {bad.numel()} of {got.numel()} elements differ; (flat index, got, want): {first}")


def rejected(out, name, *args):
    with pytest.raises(PcrlError):
        call(name, *args)
    torch.cuda.synchronize()
    assert bool((out == SENT).all()), f"{name}: a rejected call wrote its output"


def chunks(M, step=1 << 19):
    return [(r, min(r + step, M)) for r in range(0, M, step)]


def nchw(t):
    """[N, H, W, C] memory -> the logical [N, C, H, W] view the wrappers take"""
    return t.permute(0, 3, 1, 2)


# ----------------------------------------------------------------------------------------------------------------------------------------
# pcrl_bn_add_relu_fwd
# ----------------------------------------------------------------------------------------------------------------------------------------
def k_bar(y, r, co, down, M, C, dt):
    out = outbuf(M * C, dt)
    call("pcrl_bn_add_relu_fwd", y, co.scale, co.shift, r, co.rscale if down else None, co.rshift if down else None, out, M, C, dtype_code(dt))
    tail_kept(out, M * C, "bn_add_relu_fwd")
    return out[:M * C].view(M, C)


def chain_bar(y, r, co, down, M, C, dt):
    """the project's unfused chain: BatchNorm apply (twice with the downsample branch), then add + ReLU"""
    t = ops.bn_act_apply(y, co.scale, co.shift, M, C, ACT_NONE, dt)
    i = ops.bn_act_apply(r, co.rscale, co.rshift, M, C, ACT_NONE, dt) if down else r
    return ops2d.add_relu_forward(t, i, dt)


def check_bar(dt, C, M, y, r, co):
    for down in (False, True):
        got = k_bar(y, r, co, down, M, C, dt)
        what = f"bn_add_relu_fwd {dt} C={C} M={M} downsample={down}"
        for r0, r1 in chunks(M):
            want = oc.ref_bn_add_relu(y[r0:r1], co.scale, co.shift, r[r0:r1], co.rscale if down else None, co.rshift if down else None, dt)
            eq(got[r0:r1], want, f"{what} rows {r0}..{r1}")
        eq(got, chain_bar(y, r, co, down, M, C, dt), what + " against the unfused chain")
    return got


@pytest.mark.parametrize("dt,C,M", oc.BAR_CASES, ids=oc.ids)
def test_bn_add_relu_through_the_grid_wrap_and_the_unroll(dt, C, M):
    """Exact, with and without the downsample branch, against the restatement with its three roundings AND against bn_act_apply (once or
    twice) + add_relu_forward.  rc_grid() caps the launch at 2048 blocks of nslots = 256 / (C / vec) rows: M = 2048 nslots + 2 nslots + r
    wraps the grid for every slot count (C = one vector .. 256 vectors); M = 1 and 37 leave slots without a row; M = 3, 4, 5 strides + a
    remainder put 3 / 4 / 5 rows through the unroll-4 loop of a thread.  y, r = i/4, scale = j/4 up to 10, shift = j/8: z is exact in
    float32 and needs more than the 8 bits of bf16, so the intermediate roundings decide bits (test_ops2d_cases_cpu.py)."""
    y, r, co = oc.bar_inputs(dt, C, M, DEV)
    check_bar(dt, C, M, guarded(y), guarded(r), co)


@pytest.mark.parametrize("dt,C,M", oc.BAR_NT, ids=oc.ids)
def test_bn_add_relu_non_temporal_twin(dt, C, M):
    """bn_add_relu_body<NT = true>: M C esize = 201 326 592 bytes is the first size with pcrl_streaming() true (bf16 and float32), one row
    less takes the plain body.  Generated, restated in float64 chunks and compared on the device."""
    y, r, co = oc.bar_inputs(dt, C, M, DEV)
    check_bar(dt, C, M, y, r, co)


@pytest.mark.parametrize("dt", DTYPES, ids=oc.ids)
def test_bn_add_relu_special_values(dt):
    """NaN, +-inf, +-0 in y and r (all 49 pairs, inf - inf included), identity and lattice coefficients: both the fused kernel and the chain
    are `s > 0 ? s : 0`, so NaN, -inf and -0 store +0 and nothing stores NaN."""
    C = oc.vec(dt)
    y1, r1 = oc.special_pairs(dt)
    M = y1.numel()
    y, r = guarded(y1.unsqueeze(1).repeat(1, C)), guarded(r1.unsqueeze(1).repeat(1, C))
    ident = oc.Coef2(C, 3, DEV)
    ident.scale[:], ident.shift[:], ident.rscale[:], ident.rshift[:] = 1.0, 0.0, 1.0, 0.0
    for co in (ident, oc.Coef2(C, 4, DEV)):
        got = check_bar(dt, C, M, y, r, co)
        assert not bool(got.isnan().any())
    got = k_bar(y, r, ident, False, M, C, dt)
    nan_rows = (y1 != y1) | (r1 != r1)
    assert bool((got[nan_rows.to(DEV)].view(torch.int16 if dt == BF16 else torch.int32) == 0).all()), "a NaN must store +0"


@pytest.mark.parametrize("dt", DTYPES, ids=oc.ids)
def test_bn_add_relu_rejections(dt):
    C, M = 64, 16
    y, r, co = oc.bar_inputs(dt, C, M, DEV)
    out = outbuf(M * 2048, dt)
    code = dtype_code(dt)
    ok = (y, co.scale, co.shift, r, None, None, out, M, C, code)

    def with_(**kw):
        names = ("y", "scale", "shift", "r", "rscale", "rshift", "out", "M", "C", "dtype")
        return tuple(kw.get(n, v) for n, v in zip(names, ok))

    rejected(out, "pcrl_bn_add_relu_fwd", *with_(C=24 if dt == F32 else 48))          # 6 channel vectors: do not divide 256
    rejected(out, "pcrl_bn_add_relu_fwd", *with_(C=oc.vec(dt) + 2))                   # no multiple of the vector
    rejected(out, "pcrl_bn_add_relu_fwd", *with_(C=0))
    rejected(out, "pcrl_bn_add_relu_fwd", *with_(dtype=7))
    rejected(out, "pcrl_bn_add_relu_fwd", *with_(M=0))
    rejected(out, "pcrl_bn_add_relu_fwd", *with_(rscale=co.rscale))
    rejected(out, "pcrl_bn_add_relu_fwd", *with_(rshift=co.rshift))
    for k in ("y", "scale", "shift", "r"):
        rejected(out, "pcrl_bn_add_relu_fwd", *with_(**{k: None}))
    with pytest.raises(PcrlError):
        call("pcrl_bn_add_relu_fwd", *with_(out=None))
    call("pcrl_bn_add_relu_fwd", *ok)
    tail_kept(out, M * C, "bn_add_relu_fwd")


# ----------------------------------------------------------------------------------------------------------------------------------------
# pcrl_relu_mask_sum_bwd, pcrl_relu_mask_bwd, pcrl_add_relu_fwd
# ----------------------------------------------------------------------------------------------------------------------------------------
def k_elementwise(name, ins, n, dt):
    out = outbuf(n, dt)
    call(name, *ins, out, n, dtype_code(dt))
    tail_kept(out, n, name)
    return out[:n]


@pytest.mark.parametrize("nvec", oc.MASK_NVEC)
@pytest.mark.parametrize("dt", DTYPES, ids=oc.ids)
def test_relu_masks_and_add_relu_through_the_grid_stride(dt, nvec):
    """Exact.  n / vec = 1, 255, 256, 257 are around one block; 16 384 x 256 + 302 is past grid_for()'s cap: 302 threads take a second
    grid-stride step.  da = i/4 and db = 4 k are bf16 values whose sum has up to 12 significant bits: exact in float32, rounded in bf16."""
    n = nvec * oc.vec(dt)
    da, db = (guarded(t) for t in oc.wide_pair((n,), dt, nvec % 1000, DEV))
    a = guarded(oc.lat((n,), 8, 4, dt, nvec % 1000 + 7, DEV))
    eq(k_elementwise("pcrl_relu_mask_sum_bwd", (da, db, a), n, dt), oc.ref_relu_mask_sum(da, db, a, dt), f"relu_mask_sum_bwd {dt} nvec={nvec}")
    eq(k_elementwise("pcrl_relu_mask_bwd", (da, a), n, dt), oc.ref_relu_mask(da, a), f"relu_mask_bwd {dt} nvec={nvec}")
    eq(k_elementwise("pcrl_add_relu_fwd", (da, db), n, dt), oc.ref_add_relu(da, db, dt), f"add_relu_fwd {dt} nvec={nvec}")


@pytest.mark.parametrize("dt", DTYPES, ids=oc.ids)
def test_relu_masks_decide_on_the_float_value_and_round_ties_to_even(dt):
    """The mask is `a > 0.f` on the float value: the smallest positive subnormal of T and the smallest normal pass, +0, -0, a negative
    subnormal, NaN and -inf do not, +inf does.  Then 512 pairs whose sum is exactly halfway between two bf16 values: ties go to even.
    add_relu of (a, +0) stores a positive subnormal as it is and +0 for NaN, -0, -inf."""
    a10 = oc.mask_values(dt)
    a = torch.cat([a10, torch.ones(6, dtype=dt)]).to(DEV)
    da, db = torch.full((16,), 1.5, dtype=dt, device=DEV), torch.full((16,), 0.25, dtype=dt, device=DEV)
    passes = torch.tensor(oc.MASK_PASSES + [True] * 6, device=DEV)
    got = k_elementwise("pcrl_relu_mask_sum_bwd", (da, db, a), 16, dt)
    eq(got, torch.where(passes, 1.75, 0.0).to(dt), f"relu_mask_sum_bwd {dt}: special values of a")
    eq(got, oc.ref_relu_mask_sum(da.cpu(), db.cpu(), a.cpu(), dt), "the same against the restatement on the CPU")
    eq(k_elementwise("pcrl_relu_mask_bwd", (da, a), 16, dt), torch.where(passes, 1.5, 0.0).to(dt), f"relu_mask_bwd {dt}: special values of a")
    zero = torch.zeros(16, dtype=dt, device=DEV)
    eq(k_elementwise("pcrl_add_relu_fwd", (a, zero), 16, dt), oc.ref_add_relu(a.cpu(), zero.cpu(), dt), f"add_relu_fwd {dt}: special values")
    da, db = oc.tie_pair(512, dt, DEV)
    one = torch.ones(512, dtype=dt, device=DEV)
    want = (da.cpu().double() + db.cpu().double()).to(dt)
    eq(k_elementwise("pcrl_relu_mask_sum_bwd", (da, db, one), 512, dt), want, f"relu_mask_sum_bwd {dt}: ties")
    eq(k_elementwise("pcrl_add_relu_fwd", (da, db), 512, dt), want, f"add_relu_fwd {dt}: ties")


@pytest.mark.parametrize("dt", DTYPES, ids=oc.ids)
def test_relu_masks_reject_a_ragged_length(dt):
    n = oc.vec(dt) * 3 + 1
    t = torch.ones(64, dtype=dt, device=DEV)
    out = outbuf(64, dt)
    rejected(out, "pcrl_relu_mask_sum_bwd", t, t, t, out, n, dtype_code(dt))
    rejected(out, "pcrl_relu_mask_bwd", t, t, out, n, dtype_code(dt))
    rejected(out, "pcrl_add_relu_fwd", t, t, out, n, dtype_code(dt))
    rejected(out, "pcrl_relu_mask_sum_bwd", t, t, t, out, 0, dtype_code(dt))


# ----------------------------------------------------------------------------------------------------------------------------------------
# pcrl_bn_relu_maxpool2d_3s2_fwd, pcrl_maxpool2d_3s2_fwd / _bwd / _bwd_sum
# ----------------------------------------------------------------------------------------------------------------------------------------
def k_pool_fused(y, sc, sh, dt):
    N, H, W, C = y.shape
    n = N * oc.pool_out(H) * oc.pool_out(W) * C
    p, idx = outbuf(n, dt), torch.full((n + TAIL,), 200, dtype=torch.uint8, device=DEV)
    call("pcrl_bn_relu_maxpool2d_3s2_fwd", y, sc, sh, p, idx, N, H, W, C, dtype_code(dt))
    tail_kept(p, n, "bn_relu_maxpool2d_3s2_fwd: p")
    assert bool((idx[n:] == 200).all()), "bn_relu_maxpool2d_3s2_fwd: the bytes behind idx were written"
    shape = (N, oc.pool_out(H), oc.pool_out(W), C)
    return p[:n].view(shape), idx[:n].view(shape)


def k_pool_bwd(name, grads, idx, N, H, W, C, dt):
    dx = outbuf(N * H * W * C, dt)
    call(name, *grads, idx, dx, N, H, W, C, dtype_code(dt))
    tail_kept(dx, N * H * W * C, name)
    return dx[:N * H * W * C].view(N, H, W, C)


@pytest.mark.parametrize("kind", oc.POOL_KINDS)
@pytest.mark.parametrize("H,W", oc.POOL_EXTENTS, ids=oc.ids)
@pytest.mark.parametrize("dt", DTYPES, ids=oc.ids)
def test_bn_relu_maxpool_values_and_indices(dt, H, W, kind):
    """p AND idx byte for byte against (1) the restatement, (2) F.max_pool2d(return_indices=True) in float64 on the rounded activation
    T(relu(scale y + shift)) with torch's flat index converted to kh * 3 + kw, (3) bn_act_apply(ReLU) + maxpool_forward.  The extents hold
    every combination of odd / even / unit and every first-in-bounds code 0, 1, 3, 4; N = 1 with one channel vector and N = 3 with 64
    channels.  three-level: most windows hold ties (first maximum wins); negative: every activation is +0, the first in-bounds position
    wins; rounded-tie: z = 101 + r/128 differs before the rounding to bf16 and ties after it -- the argmax is taken on the stored value."""
    for N, C in NC(dt):
        y, sc, sh = oc.pool_inputs(kind, dt, N, H, W, C, DEV)
        y = guarded(y)
        p, idx = k_pool_fused(y, sc, sh, dt)
        what = f"bn_relu_maxpool2d {dt} {kind} N={N} {H}x{W} C={C}"
        a = oc.ref_bn_relu(y, sc, sh, dt)
        rp, ri = oc.ref_maxpool(a)
        eq(p, rp, what + ": p")
        eq(idx, ri, what + ": idx")
        ap, ai = oc.aten_maxpool(a.cpu())
        eq(p, ap.to(dt), what + ": p against aten")
        eq(idx, ai, what + ": idx against aten")
        act = ops.bn_act_apply(y.view(-1, C), sc, sh, N * H * W, C, ACT_RELU, dt)
        cp, ci = ops2d.maxpool_forward(nchw(act.view(N, H, W, C)), dt)
        eq(p, cp.permute(0, 2, 3, 1), what + ": p against the unfused chain")
        eq(idx, ci, what + ": idx against the unfused chain")
        if kind == "rounded-tie" and dt == BF16 and H * W > 1:
            assert not torch.equal(oc.ref_maxpool(oc.ref_bn_relu(y, sc, sh, dt, mid=False))[1], ri)


@pytest.mark.parametrize("dt", DTYPES, ids=oc.ids)
def test_maxpool_forward_lets_a_nan_win(dt):
    """pcrl_maxpool2d_3s2_fwd on images with NaN, +-inf, all -inf and signed zeros against aten (values as bits, NaN = NaN): a NaN takes
    the window (the last one of several), an all -inf window keeps its first in-bounds position."""
    C = oc.vec(dt)
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-2, 3, (2, 7, 6, C), generator=g).double()
    k = torch.randint(0, 10, (2, 7, 6, C), generator=g)
    x[k == 0], x[k == 1], x[k == 2] = float("nan"), float("-inf"), float("inf")
    x[0, ..., 1] = float("-inf")
    x[1, ..., 1] = torch.where(k[1, ..., 1] % 2 == 0, 0.0, -0.0)
    xd = guarded(x.to(dt))
    y, idx = ops2d.maxpool_forward(nchw(xd), dt)
    ap, ai = oc.aten_maxpool(x)
    eq(idx, ai, f"maxpool2d_3s2_fwd {dt}: idx with NaN / inf")
    eq(y.permute(0, 2, 3, 1).contiguous(), ap.to(dt), f"maxpool2d_3s2_fwd {dt}: values with NaN / inf")
    eq(idx, oc.ref_maxpool(x)[1], "the same against the restatement")
    assert bool(y.isnan().any())


def check_pool_backward(dt, N, H, W, C, a, idx, what, adjoint=True):
    shape = tuple(idx.shape)
    g = oc.lat(shape, 8, 4, dt, H + W, DEV)
    dx = k_pool_bwd("pcrl_maxpool2d_3s2_bwd", (guarded(g),), idx, N, H, W, C, dt)
    eq(dx, oc.ref_maxpool_bwd(g.double(), idx, H, W).to(dt), what + ": maxpool2d_3s2_bwd")
    if adjoint:      # sums of at most four i/4 with |i| <= 8 are bf16 values: dx is exact in either type, and so is the identity
        p = oc.ref_maxpool(a)[0]
        assert float((dx.double() * a.double()).sum()) == float((g.double() * p.double()).sum()), what + ": adjoint identity"
    dy, dy2 = oc.wide_pair(shape, dt, H * 3 + W, DEV)
    dxs = k_pool_bwd("pcrl_maxpool2d_3s2_bwd_sum", (guarded(dy), guarded(dy2)), idx, N, H, W, C, dt)
    eq(dxs, oc.ref_maxpool_bwd_sum(dy, dy2, idx, H, W, dt), what + ": maxpool2d_3s2_bwd_sum")


@pytest.mark.parametrize("H,W", oc.POOL_EXTENTS, ids=oc.ids)
@pytest.mark.parametrize("dt", DTYPES, ids=oc.ids)
def test_maxpool_backward_and_its_sum_form(dt, H, W):
    """Exact.  idx is the forward's on the three-level images, so a pixel is the argmax of 0, 1, 2 and 4 windows; an even extent's last
    row / column meets the `oh >= Ho` / `ow >= Wo` skip, an odd extent's does not.  The sum form rounds T(dy + dy2) BEFORE it accumulates:
    dy = i/4, dy2 = 4 k need 12 bits together, and pixels with several windows tell the two orders apart (test_ops2d_cases_cpu.py).
    Second check: <maxpool_bwd(g), a> = <g, take(a, idx)> in float64, exact on these values."""
    for N, C in NC(dt):
        y, sc, sh = oc.pool_inputs("three-level", dt, N, H, W, C, DEV)
        p, idx = k_pool_fused(y, sc, sh, dt)
        a = oc.ref_bn_relu(y, sc, sh, dt)
        eq(idx, oc.ref_maxpool(a)[1], "the forward's idx")
        check_pool_backward(dt, N, H, W, C, a, idx, f"{dt} N={N} {H}x{W} C={C}")


def test_pools_past_the_grid_cap():
    """bf16 C = 8, (4, 2050, 2052): 4 206 600 pooled vectors and 16 826 400 input vectors, both past grid_for()'s 4 194 304: the forward
    (values and idx), the backward and its sum form, generated, restated and compared on the device."""
    dt, C, N, H, W = oc.POOL_BIG
    y, sc, sh = oc.pool_inputs("three-level", dt, N, H, W, C, DEV)
    p, idx = k_pool_fused(y, sc, sh, dt)
    a = oc.ref_bn_relu(y, sc, sh, dt)
    rp, ri = oc.ref_maxpool(a)
    eq(p, rp, "bn_relu_maxpool2d past the cap: p")
    eq(idx, ri, "bn_relu_maxpool2d past the cap: idx")
    del rp, ri
    check_pool_backward(dt, N, H, W, C, a, idx, "past the cap", adjoint=False)


# ----------------------------------------------------------------------------------------------------------------------------------------
# upsamplers
# ----------------------------------------------------------------------------------------------------------------------------------------
def check_nearest(dt, N, H, W, C):
    dy = guarded(oc.lat((N, 2 * H, 2 * W, C), 127, 4, dt, H + W, DEV))
    dx = outbuf(N * H * W * C, dt)
    call("pcrl_upsample2d_nearest2_bwd", dy, dx, N, H, W, C, dtype_code(dt))
    tail_kept(dx, N * H * W * C, "upsample2d_nearest2_bwd")
    eq(dx[:N * H * W * C], oc.ref_nearest2_bwd(dy, dt), f"upsample2d_nearest2_bwd {dt} N={N} {H}x{W} C={C}")


@pytest.mark.parametrize("H,W", oc.UP_EXTENTS, ids=oc.ids)
@pytest.mark.parametrize("dt", DTYPES, ids=oc.ids)
def test_nearest_upsample_backward(dt, H, W):
    """pcrl_upsample2d_nearest2_bwd, exact: dx = T((a + b) + (c + d)), dy = i/4 with |i| <= 127, so the 2x2 sum needs 9 bits and is rounded
    in bf16."""
    for N, C in NC(dt):
        check_nearest(dt, N, H, W, C)


def test_nearest_upsample_backward_past_the_grid_cap():
    """bf16 C = 8, (1, 2049, 2050): 4 200 450 vectors, past grid_for()'s 4 194 304; generated, restated and compared on the device."""
    dt, C, N, H, W = oc.UP_BIG
    check_nearest(dt, N, H, W, C)


def k_bilinear(name, x, N, H, W, C, s, n_out):
    out = outbuf(n_out, F32)
    call(name, x, out, N, H, W, C, s)
    tail_kept(out, n_out, name)
    return out[:n_out]


@pytest.mark.parametrize("s", oc.BIL_POW2)
@pytest.mark.parametrize("H,W", oc.BIL_EXTENTS, ids=oc.ids)
def test_bilinear_power_of_two_scales_are_exact(H, W, s):
    """pcrl_upsample2d_bilinear_fwd / _bwd for s = 1, 2, 4, 8, 16: source index and weights are dyadic, x = i/4 and dy = i/4 (|i| <= 8), so
    forward and backward are exact: bits against the float64 restatement of torch's align_corners=False rule and against F.interpolate in
    float64; the backward against the float64 adjoint.  The extents have the clamp at 0, the clamp of i1 at the far edge and one-pixel
    axes; C = 1, 3, 4, 5.  (Zero sign: the references are matrix products.)"""
    N = 2
    for C in oc.BIL_C:
        x = guarded(oc.lat((N, H, W, C), 8, 4, F32, H * 7 + W + C, DEV))
        n_out = N * H * s * W * s * C
        y = k_bilinear("pcrl_upsample2d_bilinear_fwd", x, N, H, W, C, s, n_out)
        what = f"bilinear s={s} {H}x{W} C={C}"
        eq(y, oc.ref_bilinear_fwd(x, s).float(), what + ": forward", bits=False)
        ya = F.interpolate(x.cpu().double().permute(0, 3, 1, 2), scale_factor=s, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
        eq(y, ya.float().contiguous(), what + ": forward against F.interpolate", bits=False)
        dy = guarded(oc.lat((N, H * s, W * s, C), oc.BIL_DY_INT, 4, F32, s + C, DEV))
        dx = k_bilinear("pcrl_upsample2d_bilinear_bwd", dy, N, H, W, C, s, N * H * W * C)
        eq(dx, oc.ref_bilinear_bwd(dy, s).float(), what + ": backward", bits=False)


@pytest.mark.parametrize("s", oc.BIL_ODD)
@pytest.mark.parametrize("H,W", oc.BIL_EXTENTS, ids=oc.ids)
def test_bilinear_odd_scales_within_the_derived_bound(H, W, s):
    """s = 3, 5 (accepted by the ABI, unused by the model): 1/s and the weights are rounded.  The restatement takes src, i0 and l1 in
    float32 exactly as the compiled bilinear_src does (one fused multiply-add) and the lerp in float64.  Derived bound per element:
    8 * 2^-24 * sum |w x| -- at most five float32 roundings lie on any path of the two-level lerp (1 - l, two products and their sum per
    level, the last sum), each at most 2^-24 of a partial result bounded by sum |w x|; three more for contraction choices."""
    N = 2
    for C in oc.BIL_C:
        x = guarded(oc.lat((N, H, W, C), 8, 4, F32, H * 7 + W + C, DEV))
        y = k_bilinear("pcrl_upsample2d_bilinear_fwd", x, N, H, W, C, s, N * H * s * W * s * C).view(N, H * s, W * s, C)
        ref, scale = oc.ref_bilinear_fwd(x, s), oc.ref_bilinear_fwd(x, s, absolute=True)
        err, bound = (y.double() - ref).abs(), 8 * 2.0 ** -24 * scale
        bad = (err > bound).nonzero()
        print(f"bilinear s={s} {H}x{W} C={C}: max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bad.numel() == 0, f"bilinear s={s} {H}x{W} C={C}: {bad.shape[0]} elements past the bound, first {bad[0].tolist()}: err {float(err[tuple(bad[0])]):.3e}"


# ----------------------------------------------------------------------------------------------------------------------------------------
# heads2d.hip
# ----------------------------------------------------------------------------------------------------------------------------------------
def ws_of(nbytes):
    return torch.full((int(nbytes) // 4 + 2048,), POISON, dtype=F32, device=DEV)


@pytest.mark.parametrize("N,HW,C", oc.MSE_FWD, ids=oc.ids)
def test_mse_forward(N, HW, C):
    """pcrl_mse2d_fwd, exact: p, gt = i/4, so every thread's float32 sum of d^2 is exact, the float64 block and finish sums are exact in any
    order, and the loss is (float)(sum * (1.0 / (M C))) restated as exactly that.  M around a quarter block and a block (255 .. 1025);
    768 / 769 / 1024 / 1025 / 1030 blocks around the four-way unroll `i + 768 < blocks` of the finish and its tail; N = 3 with HW no
    multiple of 256: blocks straddle samples.  The workspace and the rows behind p and gt hold poison."""
    M = N * HW
    p, gt = guarded(oc.lat((M, C), 8, 4, F32, M % 1000 + 1, DEV)), guarded(oc.lat((N, C, HW), 8, 4, F32, M % 1000 + 2, DEV))
    nb = lib().call("pcrl_mse2d_ws_bytes", M)
    assert nb == oc.rows1024(M) * 8
    loss = outbuf(1, F32)
    call("pcrl_mse2d_fwd", p, gt, loss, ws_of(nb), nb, N, HW, C)
    tail_kept(loss, 1, "mse2d_fwd")
    eq(loss[:1], oc.ref_mse(p, gt, N, C, HW).view(1), f"mse2d_fwd N={N} HW={HW} C={C} ({oc.rows1024(M)} blocks)")


def test_mse_forward_rejections():
    N, HW = 3, 343
    p, gt = oc.lat((N * HW, 3), 8, 4, F32, 1, DEV), oc.lat((N, 3, HW), 8, 4, F32, 2, DEV)
    nb = lib().call("pcrl_mse2d_ws_bytes", N * HW)
    loss = outbuf(1, F32)
    rejected(loss, "pcrl_mse2d_fwd", p, gt, loss, ws_of(nb), nb - 1, N, HW, 3)          # one byte short
    rejected(loss, "pcrl_mse2d_fwd", p, gt, loss, None, nb, N, HW, 3)
    rejected(loss, "pcrl_mse2d_fwd", p, gt, loss, ws_of(nb), nb, N, HW, 2)
    rejected(loss, "pcrl_mse2d_fwd", p, gt, loss, ws_of(nb), nb, 0, HW, 3)


@pytest.mark.parametrize("N,HW", oc.MSE_BWD, ids=oc.ids)
@pytest.mark.parametrize("dt,CP", oc.MSE_FORMS, ids=oc.ids)
def test_mse_backward_padded(dt, CP, N, HW):
    """pcrl_mse2d_bwd_pad (bf16 CP 8, float32 CP 8, float32 CP 3).  dy: bits against float32 g * (p - gt) with g = float32(dloss) *
    float32(2 / (3 M)) -- one product that no contraction can change -- then RNE to bf16; padding channels exactly +0.
    Column partials (row pitch CP, one row per 1024 pixels): in the bf16 form |p - gt| = i/4 with |i| <= 15, the stored values span fewer
    than 2^12 units and a partial is exact in any order: bits against the float64 sum of the STORED values.  In the float32 forms the
    partial depends on the order: derived any-order bound (rows - 1) * 2^-24 * sum |stored| per block and column."""
    M = N * HW
    p, gt = oc.mse_bwd_inputs(N, HW, dt, DEV)
    p, gt = guarded(p), guarded(gt)
    dloss = torch.tensor([oc.MSE_DLOSS], dtype=F32, device=DEV)
    rows = oc.rows1024(M)
    assert lib().call("pcrl_rows1024", M) == rows
    dy, col = outbuf(M * CP, dt), outbuf(rows * CP, F32)
    call("pcrl_mse2d_bwd_pad", p, gt, dloss, dy, col, N, HW, 3, CP, dtype_code(dt))
    tail_kept(dy, M * CP, "mse2d_bwd_pad: dy")
    tail_kept(col, rows * CP, "mse2d_bwd_pad: colpart")
    what = f"mse2d_bwd_pad {dt} CP={CP} N={N} HW={HW}"
    stored = dy[:M * CP].view(M, CP)
    eq(stored, oc.ref_mse_bwd(p, gt, oc.MSE_DLOSS, N, HW, CP, dt), what + ": dy")
    got = col[:rows * CP].view(rows, CP)
    sums = oc.block_sums64(stored)
    if CP == 8:
        assert bool((got[:, 3:].contiguous().view(torch.int32) == 0).all()), what + ": padding columns of the partials"
    if dt == BF16:
        eq(got, sums.float(), what + ": column partials")
    else:
        n_rows = torch.full((rows,), 1024.0, dtype=torch.float64, device=DEV)
        n_rows[-1] = M - 1024 * (rows - 1)
        bound = (n_rows - 1).view(-1, 1) * 2.0 ** -24 * oc.block_sums64(stored.abs())
        err = (got.double() - sums).abs()
        print(f"{what}: max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), what + f": column partials off by up to {float(err.max()):.3e}"


def test_mse_backward_rejections():
    N, HW = 1, 257
    p, gt = oc.mse_bwd_inputs(N, HW, BF16, DEV)
    dloss = torch.ones(1, dtype=F32, device=DEV)
    dy, col = outbuf(HW * 8, BF16), outbuf(8, F32)
    rejected(dy, "pcrl_mse2d_bwd_pad", p, gt, dloss, dy, col, N, HW, 3, 3, dtype_code(BF16))          # the unpadded form is float32 only
    rejected(dy, "pcrl_mse2d_bwd_pad", p, gt, dloss, dy, col, N, HW, 3, 4, dtype_code(BF16))
    rejected(dy, "pcrl_mse2d_bwd_pad", p, gt, dloss, dy, col, N, HW, 1, 8, dtype_code(BF16))
    rejected(dy, "pcrl_mse2d_bwd_pad", p, gt, None, dy, col, N, HW, 3, 8, dtype_code(BF16))
    tail_kept(col, 0, "mse2d_bwd_pad: colpart of a rejected call")


@pytest.mark.parametrize("dt,Ci,M", oc.C11_CASES, ids=oc.ids)
def test_conv1x1_small_backward(dt, Ci, M):
    """pcrl_conv2d_1x1_small_bwd, exact: x = i/4, dy = i/4, w = j/8 (|j| <= 16).  dx equals the float64 value / its RNE to bf16 (up to 384
    units of 1/32: rounded in bf16); every row of `part` equals the float64 sums over its 1024 pixels (4096 units of 1/16: exact in any
    order), the three bias sums at offset 3 Ci, the padding out to PW exactly zero -- with PW = 3 Ci + 3 and with the wrapper's 4 * 2^k.
    Ci from one channel vector (256 row slots) to 256 vectors (one slot); M = 1, nslots - 1, 2 nslots + 1 and around one and two blocks.
    (Zero sign of dx: the reference is a matrix product.)"""
    x, dy = guarded(oc.lat((M, Ci), 8, 4, dt, M + Ci, DEV)), guarded(oc.lat((M, 3), 8, 4, F32, M + Ci + 1, DEV))
    w = oc.lat((3, Ci), 16, 8, F32, Ci, DEV)
    rdx, rpart = oc.ref_conv1x1_small_bwd(x, dy, w, dt)
    rows, width = oc.rows1024(M), 3 * Ci + 3
    pw2 = 4
    while pw2 < width:
        pw2 *= 2
    for PW in (width, pw2, width + 5):
        dx, part = outbuf(M * Ci, dt), outbuf(rows * PW, F32)
        call("pcrl_conv2d_1x1_small_bwd", x, dy, w, dx, part, M, Ci, 3, PW, dtype_code(dt))
        tail_kept(dx, M * Ci, "conv2d_1x1_small_bwd: dx")
        tail_kept(part, rows * PW, "conv2d_1x1_small_bwd: part")
        what = f"conv2d_1x1_small_bwd {dt} Ci={Ci} M={M} PW={PW}"
        eq(dx[:M * Ci], rdx, what + ": dx", bits=False)
        got = part[:rows * PW].view(rows, PW)
        eq(got[:, :width].contiguous(), rpart.float(), what + ": partial rows", bits=False)
        if PW > width:
            assert bool((got[:, width:].contiguous().view(torch.int32) == 0).all()), what + ": the row pitch padding is not zero"


@pytest.mark.parametrize("dt", DTYPES, ids=oc.ids)
def test_conv1x1_small_backward_rejections(dt):
    M, Ci = 16, 64
    x, dy, w = oc.lat((M, Ci), 8, 4, dt, 1, DEV), oc.lat((M, 4), 8, 4, F32, 2, DEV), oc.lat((4, Ci), 16, 8, F32, 3, DEV)
    dx, part = outbuf(M * Ci, dt), outbuf(512, F32)
    code = dtype_code(dt)
    rejected(dx, "pcrl_conv2d_1x1_small_bwd", x, dy, w, dx, part, M, Ci, 4, 512, code)                       # Co = 4
    rejected(dx, "pcrl_conv2d_1x1_small_bwd", x, dy, w, dx, part, M, 24 if dt == F32 else 48, 3, 512, code)  # six channel vectors
    rejected(dx, "pcrl_conv2d_1x1_small_bwd", x, dy, w, dx, part, M, Ci, 3, 3 * Ci + 2, code)                # PW too small
    rejected(dx, "pcrl_conv2d_1x1_small_bwd", x, dy, w, dx, part, 0, Ci, 3, 512, code)
    tail_kept(part, 0, "conv2d_1x1_small_bwd: part of a rejected call")


@pytest.mark.parametrize("dt,C,N,HW", oc.PAD_CASES + [oc.PAD_BIG], ids=oc.ids)
def test_image_transpose_and_pad(dt, C, N, HW):
    """pcrl_nchw_to_nhwc_pad, bits against the transpose-and-pad restatement: C = 1, 2, 3 float32 planes -> [N HW][8] in float32 or bf16
    (normal deviates: the bf16 values need a rounding), channels C .. 7 exactly +0.  (1, 16 777 216 + 300) in bf16 C = 3 is 300 pixels past
    the 65 536 x 256 threads of the capped grid; generated and compared on the device."""
    g = torch.Generator(device=DEV).manual_seed(HW % 1000 + C)
    x = guarded(torch.randn((N, C, HW), generator=g, device=DEV, dtype=F32))
    out = outbuf(N * HW * 8, dt)
    call("pcrl_nchw_to_nhwc_pad", x, out, N, C, HW, 8, dtype_code(dt))
    tail_kept(out, N * HW * 8, "nchw_to_nhwc_pad")
    eq(out[:N * HW * 8], oc.ref_nchw_to_nhwc_pad(x, N, C, HW, dt), f"nchw_to_nhwc_pad {dt} C={C} N={N} HW={HW}")
