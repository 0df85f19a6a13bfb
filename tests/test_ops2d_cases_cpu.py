"""Preconditions of tests/test_ops2d_exact_gpu.py, checked without a GPU: the constants the case table of ops2d_cases.py was built for are
the ones in the source text; the table crosses each of them; every "exact" case is exactly summable (asserted analytically from the
lattice bounds); the restatements agree with aten on the CPU; and where a kernel places a rounding on purpose, the restatement without
that rounding differs from the one with it on the inputs of the case -- the case can tell the two apart."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_pool_cases as npc
import ops2d_cases as oc
from exact_lattice import EXACT_LIMIT, assert_exactly_summable
from ops2d_cases import BF16, F32


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32 if t.dtype == F32 else torch.int64)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---- source pins ----
def test_the_constants_of_the_source_are_the_ones_the_case_table_was_built_for():
    assert oc.source_pins_hold() == []
    assert (oc.RC_CAP, oc.GRID_CAP, oc.ROWS_PER_BLOCK, oc.PAD_CAP, oc.ADD_CAP, oc.FINISH_LEAD, oc.NT_BYTES) == (2048, 16384, 1024, 65536, 4096, 768, 192 << 20)


@pytest.mark.parametrize("f,old,new", [
    ("encoder2d.hip", "b > 2048", "b > 4096"), ("encoder2d.hip", "b > 16384 ? 16384", "b > 16384 ? 8192"), ("encoder2d.hip", "#pragma unroll 4", "#pragma unroll 8"),
    ("ops2d.hip", "b > 16384 ? 16384", "b > 32768 ? 32768"), ("heads2d.hip", "ROWS_PER_BLOCK = 1024", "ROWS_PER_BLOCK = 512"),
    ("heads2d.hip", "b > 65536", "b > 32768"), ("heads2d.hip", "blocks > 4096", "blocks > 2048"), ("heads2d.hip", "i + 768 < blocks", "i + 768 <= blocks"),
    ("heads2d.hip", "#pragma unroll 2", "#pragma unroll 4"), ("common.h", "(int64_t)192 << 20", "(int64_t)256 << 20")])
def test_source_pins_notice_a_changed_constant_and_ignore_spacing(f, old, new):
    text = npc.read_source(f)
    assert old in text
    assert [p[0] for p in oc.source_pins_hold(read=lambda n: text.replace(old, new) if n == f else npc.read_source(n))] == [f]
    assert oc.source_pins_hold(read=lambda n: npc.read_source(n).replace(" < ", "<\n   ")) == []


# ---- the table crosses every constant ----
def test_bn_add_relu_cases_cross_the_grid_cap_the_unroll_and_the_streaming_threshold():
    for dt in (F32, BF16):
        wrapped = {oc.nslots(C, dt) for d, C, M in oc.BAR_CASES if d == dt and oc.rc_blocks(M, C, dt)[1] > oc.RC_CAP}
        assert wrapped == {256 // (C // oc.vec(dt)) for C in oc.BAR_C[dt]} and {1, 4, 8, 16, 256} <= wrapped
        for C in oc.BAR_C[dt]:
            M, ns = oc.wrap_rows(C, dt), oc.nslots(C, dt)
            assert npc.rc_ok(C, dt) and M > oc.RC_CAP * ns + 2 * ns and (ns == 1 or M % ns)
        assert any(d == dt and M == 1 for d, C, M in oc.BAR_CASES)
    assert {4, 1024} <= set(oc.BAR_C[F32]) and {8, 2048} <= set(oc.BAR_C[BF16])          # one channel vector and 256 of them: the extremes
    counts = set().union(*(oc.thread_rows(M, C, dt) for dt, C, M in oc.BAR_CASES))
    assert {0, 1, 2, 3, 4, 5} <= counts, counts
    (d0, C0, M0), (d1, C1, M1), (d2, C2, M2) = oc.BAR_NT
    assert M0 * C0 * oc.esize(d0) == oc.NT_BYTES == 201326592 and oc.streaming(M0 * C0 * oc.esize(d0))
    assert M1 == M0 - 1 and not oc.streaming(M1 * C1 * oc.esize(d1))
    assert d2 == F32 and M2 * C2 * 4 == oc.NT_BYTES
    assert all(not oc.streaming(M * C * oc.esize(dt)) for dt, C, M in oc.BAR_CASES)
    assert not npc.rc_ok(24, F32) and not npc.rc_ok(48, BF16) and 24 % 4 == 0 and 48 % 8 == 0            # the two rejected widths


def test_grid_stride_cases_wrap_once():
    assert oc.MASK_NVEC == [1, 255, 256, 257, 16384 * 256 + 302]
    assert oc.CAP_ITEMS < oc.WRAP_VECS < 2 * oc.CAP_ITEMS
    dt, C, N, H, W = oc.POOL_BIG
    assert oc.CAP_ITEMS < N * oc.pool_out(H) * oc.pool_out(W) * (C // oc.vec(dt)) < 2 * oc.CAP_ITEMS
    assert N * H * W * (C // oc.vec(dt)) > oc.CAP_ITEMS
    dt, C, N, H, W = oc.UP_BIG
    assert oc.CAP_ITEMS < N * H * W * (C // oc.vec(dt)) < 2 * oc.CAP_ITEMS
    dt, C, N, HW = oc.PAD_BIG
    assert oc.PAD_CAP * 256 < N * HW < 2 * oc.PAD_CAP * 256 and (N * HW) % 256 and (dt, C) == (BF16, 3)
    assert all(N * HW <= oc.PAD_CAP * 256 for _, _, N, HW in oc.PAD_CASES)
    assert {HW for _, _, _, HW in oc.PAD_CASES} == {1, 255, 257} and {C for _, C, _, _ in oc.PAD_CASES} == {1, 2, 3}


def test_pool_extents_reach_every_start_code_and_both_sides_of_the_last_row_skip():
    """first in-bounds code of a window: 4 (top-left window of an image), 3 / 1 (first row / column further on), 0 (interior); H = 1 or
    W = 1 leave windows of one row / column.  An even extent's last row has oh1 = (ih + 1) >> 1 = Ho (the `oh >= Ho` skip), an odd
    extent's last row does not."""
    first, sizes = set(), set()
    for H, W in oc.POOL_EXTENTS:
        _, valid = oc.windows9(torch.zeros(1, H, W, 1))
        first |= set(valid.squeeze(0).squeeze(-1).int().argmax(2).flatten().tolist())
        sizes |= set(valid.sum(3).flatten().tolist())
    assert first == {0, 1, 3, 4} and {1, 2, 3, 4, 6, 9} <= sizes
    ext = [h for hw in oc.POOL_EXTENTS for h in hw]
    assert any(h % 2 == 0 and (h - 1 + 1) >> 1 >= oc.pool_out(h) for h in ext) and any(h % 2 == 1 and h > 1 and h >> 1 < oc.pool_out(h) for h in ext)
    assert {(H % 2, W % 2) for H, W in oc.POOL_EXTENTS if H > 1 and W > 1} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert (1, 1) in oc.POOL_EXTENTS and any(H == 1 < W for H, W in oc.POOL_EXTENTS) and any(W == 1 < H for H, W in oc.POOL_EXTENTS)


def test_heads_cases_cross_the_row_blocks_the_finish_unroll_and_every_slot_count():
    assert {N * HW for N, HW, _ in oc.MSE_FWD} >= set(oc.MSE_M) and {N * HW for N, HW in oc.MSE_BWD} >= set(oc.MSE_M)
    assert {oc.rows1024(N * HW) for N, HW, _ in oc.MSE_FWD} >= set(oc.MSE_BLOCKS)
    # thread 0 of the finish kernel: the unrolled pass runs while i + 768 < blocks: not at 768, once from 769 on, and 1025 / 1030 leave a tail
    assert not 0 + oc.FINISH_LEAD < 768 and 0 + oc.FINISH_LEAD < 769 and 1025 - 1024 == 1 and 1030 - 1024 == 6
    assert any(N == 3 and HW % 256 and oc.rows1024(N * HW) > 1 for N, HW, _ in oc.MSE_FWD) and {C for _, _, C in oc.MSE_FWD} == {1, 3}
    assert any(N == 3 and HW % 256 and oc.rows1024(N * HW) > 1 for N, HW in oc.MSE_BWD)
    assert oc.MSE_FORMS == [(BF16, 8), (F32, 8), (F32, 3)]
    for dt in (F32, BF16):
        ns = {oc.nslots(Ci, dt) for Ci in oc.C11_CI[dt]}
        assert {1, 256} <= ns and len(ns) == 4
        for Ci in oc.C11_CI[dt]:
            assert npc.rc_ok(Ci, dt) and (256 // (Ci // oc.vec(dt))) * 3 * Ci * 4 <= 64 * 1024
            n = oc.nslots(Ci, dt)
            assert set(oc.c11_ms(Ci, dt)) == {m for m in (1, n - 1, 2 * n + 1, 1023, 1024, 1025, 2049) if m > 0}
    # `#pragma unroll 2` over m = slot, slot + nslots, ...: a block of 1024 rows gives a slot 1024 / nslots rows, the tails 1, 2 or 3
    assert {len(range(0, min(M, 1024), oc.nslots(Ci, dt))) % 2 for dt, Ci, M in oc.C11_CASES} == {0, 1}


# ---- exactness ----
def test_elementwise_results_fit_24_bits_and_exceed_8():
    z_units = oc.SC_INT * oc.Y_INT + 2 * oc.SH_INT                           # (j/4)(i/4) + k/8 in units of 1/16
    assert 256 < z_units < EXACT_LIMIT and 2 * z_units < EXACT_LIMIT        # t + i as well
    assert 127 + 16 * 127 < EXACT_LIMIT and 127 + 16 * 127 > 256            # wide_pair sums, units of 1/4: rounded in bf16
    assert 4 * (127 + 16 * 127) < EXACT_LIMIT                                # at most four windows meet in a pixel
    assert 4 * 127 > 256 and 4 * 127 < EXACT_LIMIT                           # nearest2: 2x2 sum of i/4, |i| <= 127


def test_bilinear_backward_is_exactly_summable():
    """weights are multiples of 1/(2s), dy of 1/4: every term is a multiple of 1/(16 s^2); an input pixel collects at most 1.5 s of weight
    per axis (s in the interior, the clamped border half a pixel more), so |dx| <= (1.5 s)^2 max|dy|"""
    for s in oc.BIL_POW2:
        unit = 1.0 / (16 * s * s)
        assert_exactly_summable((1.5 * s) ** 2 * oc.BIL_DY_INT / 4, unit, f"bilinear backward s={s}")
        assert s * s * oc.BIL_DY_INT / 4 / unit < EXACT_LIMIT
        for n in (1, 2, 3, 5, 6, 7):
            A = oc.bilinear_matrix(n, s)
            assert float(A.sum(0).max()) <= 1.5 * s and torch.equal(A * 2 * s, (A * 2 * s).round())
            assert torch.equal(A, oc.bilinear_matrix(n, s, fused=False))


def test_partial_rows_are_exactly_summable():
    assert_exactly_summable(1024 * (oc.Y_INT / 4) ** 2, 1 / 16, "conv1x1 small: sum dy x over a 1024-pixel block")
    assert_exactly_summable(1024 * oc.Y_INT / 4, 1 / 4, "conv1x1 small: sum dy")
    assert_exactly_summable(3 * (oc.Y_INT / 4) * 2.0, 1 / 32, "conv1x1 small: dx")
    assert 3 * 2 * 2 * 32 > 256, "dx never leaves the bf16 grid"
    assert_exactly_summable(4 * 3 * 16.0, 1 / 16, "mse2d: a thread's sum of d^2 (4 rows x 3 channels, |d| <= 4)")
    # bf16 backward: stored values T(g i/4), 1 <= |i| <= 15: the smallest is g/4 with ulp(g/4) >= |g/4| 2^-8, the largest below 16 |g/4|
    # = 2^12 such ulps; 1024 of them stay below 2^22 units, and every stored value is a multiple of the smallest one's ulp
    assert 1024 * 2 ** 12 < EXACT_LIMIT


# ---- placed roundings: the cases tell the restatement with the rounding from the one without ----
def test_bn_add_relu_cases_see_the_intermediate_roundings():
    """bf16: T(scale y + shift) and T(rscale r + rshift) are rounded before the sum.  (In float32 every value of the lattice is a float32
    value and the roundings are the identity: there the case pins the arithmetic, not the place of a rounding.)"""
    for dt, C, M in [c for c in oc.BAR_CASES if c[0] == BF16 and c[2] * c[1] < 1 << 20]:
        y, r, co = oc.bar_inputs(dt, C, M, "cpu")
        for rs, rh in ((None, None), (co.rscale, co.rshift)):
            a, b = oc.ref_bn_add_relu(y, co.scale, co.shift, r, rs, rh, dt), oc.ref_bn_add_relu(y, co.scale, co.shift, r, rs, rh, dt, mid=False)
            assert not same_bits(a, b), (C, M)
    y, r, co = oc.bar_inputs(F32, 64, 37, "cpu")
    z = co.scale * y + co.shift
    assert torch.equal(z.double(), co.scale.double() * y.double() + co.shift.double()) and not torch.equal(z.to(BF16).float(), z)


def test_special_values_through_bn_add_relu():
    y, r = oc.special_pairs(F32)
    one, zero = torch.ones(1), torch.zeros(1)
    out = oc.ref_bn_add_relu(y, one, zero, r, None, None, F32)
    assert not bool(out.isnan().any()) and bool((bits(out[out == 0]) == 0).all()), "NaN, -inf, inf - inf and -0 store +0"
    assert float(out[(y == math.inf) & (r == 1)][0]) == math.inf and float(out[(y == math.inf) & (r == -math.inf)][0]) == 0.0


def test_pool_cases_see_the_argmax_on_the_rounded_activation_and_hold_ties():
    mult = set()
    for H, W in oc.POOL_EXTENTS:
        for N, C in ((1, 8), (3, 64)):
            y, sc, sh = oc.pool_inputs("rounded-tie", BF16, N, H, W, C, "cpu")
            a, z = oc.ref_bn_relu(y, sc, sh, BF16), oc.ref_bn_relu(y, sc, sh, BF16, mid=False)
            assert bool((a == 101).all()) and torch.equal(z, 101 + (y.double() - 1))
            _, idx = oc.ref_maxpool(a)
            _, valid = oc.windows9(a)
            assert torch.equal(idx.long(), valid.int().argmax(3).expand_as(idx)), "all tied: the first in-bounds position"
            if H * W > 1:
                assert not torch.equal(oc.ref_maxpool(z)[1], idx)
            y, sc, sh = oc.pool_inputs("negative", BF16, N, H, W, C, "cpu")
            a = oc.ref_bn_relu(y, sc, sh, BF16)
            assert bool((bits(a) == 0).all()) and torch.equal(oc.ref_maxpool(a)[1], idx)
            y, sc, sh = oc.pool_inputs("three-level", BF16, N, H, W, C, "cpu")
            _, idx3 = oc.ref_maxpool(oc.ref_bn_relu(y, sc, sh, BF16))
            mult |= set(oc.argmax_multiplicity(idx3, H, W).flatten().tolist())
    assert mult == {0, 1, 2, 3, 4} or {0, 1, 2, 4} <= mult, mult


def test_maxpool_backward_sum_cases_see_the_rounding_of_the_sum():
    """bf16: T(dy + dy2) before the accumulation.  Only a pixel that is the argmax of two or more windows can tell (one term: the same single
    rounding either way), so the N = 3, C = 64 case of every extent that has such pixels must differ; the (1, 1) image has none."""
    for H, W in oc.POOL_EXTENTS:
        y, sc, sh = oc.pool_inputs("three-level", BF16, 3, H, W, 64, "cpu")
        _, idx = oc.ref_maxpool(oc.ref_bn_relu(y, sc, sh, BF16))
        dy, dy2 = oc.wide_pair(idx.shape, BF16, H + W, "cpu")
        assert not torch.equal((dy.double() + dy2.double()).to(BF16).double(), dy.double() + dy2.double())
        a, b = oc.ref_maxpool_bwd_sum(dy, dy2, idx, H, W, BF16), oc.ref_maxpool_bwd_sum(dy, dy2, idx, H, W, BF16, pre=False)
        assert same_bits(a, b) == (int(oc.argmax_multiplicity(idx, H, W).max()) <= 1), (H, W)
    assert any(int(oc.argmax_multiplicity(oc.ref_maxpool(oc.ref_bn_relu(*oc.pool_inputs("three-level", BF16, 1, H, W, 8, "cpu"), BF16))[1], H, W).max()) > 1
               for H, W in oc.POOL_EXTENTS)


def test_tie_pairs_are_halfway_and_go_to_even():
    da, db = oc.tie_pair(512, BF16, "cpu")
    s = da.double() + db.double()
    assert bool((s % 1 == 0.5).all()) and bool((s > 128).all()) and bool((s < 256).all())
    r = s.to(BF16).double()
    assert bool(((r - s).abs() == 0.5).all()) and bool((r % 2 == 0).all())
    assert bool((r > s).any()) and bool((r < s).any())


def test_mask_values():
    for dt in (F32, BF16):
        a = oc.mask_values(dt)
        assert (a.double() > 0).tolist() == oc.MASK_PASSES
        sub, nrm = oc.tiny(dt)
        assert float(a[2].double()) == sub > 0 and float(a[3].double()) == nrm and bits(a)[2].item() == 1
        g = oc.ref_relu_mask_sum(torch.ones(10, dtype=dt), torch.ones(10, dtype=dt), a, dt)
        assert g.tolist() == [2.0 if p else 0.0 for p in oc.MASK_PASSES]


@pytest.mark.parametrize("N,HW", oc.MSE_BWD, ids=oc.ids)
def test_mse_backward_cases_see_the_float32_coefficient(N, HW):
    """float32 forms: g = dloss * (float)(2.0 / (3 M)) and ONE float32 product against the float64 product rounded once.  In the bf16 form
    the rounding to 8 bits hides the difference except next to a tie; that form is pinned by the bits of T(float32 product) alone."""
    M = N * HW
    p, gt = oc.mse_bwd_inputs(N, HW, F32, "cpu")
    a, b = oc.ref_mse_bwd(p, gt, oc.MSE_DLOSS, N, HW, 3, F32), oc.ref_mse_bwd(p, gt, oc.MSE_DLOSS, N, HW, 3, F32, k32=False)
    assert not same_bits(a, b)
    g = oc.mse_g(oc.MSE_DLOSS, M)
    assert g.dtype == np.float32 and float(g) != float(oc.mse_g(oc.MSE_DLOSS, M, k32=False))
    d = (p - oc.nchw_to_rows(gt, N, 3, HW)).numpy()
    assert same_bits(a, torch.from_numpy((g * d).astype(np.float32)))


def test_odd_scale_bilinear_source_index_depends_on_the_contraction():
    """s = 3, 5: inv = (float)(1/s) is rounded and so is src; the fused form (one rounding, what the compiled kernel does) and the
    two-rounding form differ at some dst -- the restatement has to pick the kernel's.  s a power of two: equal (and exact)."""
    for s in oc.BIL_ODD:
        a, b = oc.bilinear_axis(7 * s, 7, s), oc.bilinear_axis(7 * s, 7, s, fused=False)
        assert not torch.equal(a[2], b[2])
        assert bool(((a[2] - b[2]).abs() <= 2.0 ** -21).all())
    for s in oc.BIL_POW2:
        for n in (1, 6, 7):
            a, b = oc.bilinear_axis(n * s, n, s), oc.bilinear_axis(n * s, n, s, fused=False)
            assert all(torch.equal(u, v) for u, v in zip(a, b))
            assert int(a[0].min()) == 0 and int(a[1].max()) == n - 1 and bool((a[1] - a[0] <= 1).all())
            if n > 1:
                assert bool(((a[0] == n - 1) & (a[1] == n - 1)).any()), "the far edge: i1 clamped"
                assert bool((a[2][:max(s // 2, 1)] == 0).all()), "the near edge: src clamped at 0"


# ---- the restatements against aten ----
def special_image(H, W):
    g = torch.Generator().manual_seed(H * 13 + W)
    x = torch.randint(-2, 3, (2, H, W, 4), generator=g).double()
    k = torch.randint(0, 12, (2, H, W, 4), generator=g)
    x[k == 0], x[k == 1], x[k == 2] = math.nan, -math.inf, math.inf
    x[0, ..., 3] = -math.inf
    x[1, ..., 3] = math.nan
    x[0, ..., 2] = torch.where(k[0, ..., 2] % 2 == 0, 0.0, -0.0)
    return x


@pytest.mark.parametrize("H,W", oc.POOL_EXTENTS + [(6, 6)], ids=oc.ids)
def test_pool_restatement_against_aten(H, W):
    """ref_maxpool / ref_maxpool_bwd against F.max_pool2d(return_indices=True) and its autograd in float64: lattice, tie-heavy, and images
    with NaN (the LAST NaN of a window wins), all -inf (the first in-bounds position keeps the index), +-inf and signed zeros."""
    for x in (oc.lat((3, H, W, 4), 8, 4, F32, H + W, "cpu").double(), oc.three_level((3, H, W, 4), F32, H * W, "cpu").double(), special_image(H, W)):
        p, idx = oc.ref_maxpool(x)
        pa, ia = oc.aten_maxpool(x)
        assert torch.equal(idx, ia)
        assert torch.equal(p.isnan(), pa.isnan()) and same_bits(p.nan_to_num(nan=0.0), pa.nan_to_num(nan=0.0))
        xn = x.nan_to_num(nan=0.0, posinf=9.0, neginf=-9.0).permute(0, 3, 1, 2).clone().requires_grad_(True)
        out, flat = F.max_pool2d(xn, 3, 2, 1, return_indices=True)
        g = oc.lat(tuple(idx.shape), 8, 4, F32, 5, "cpu").double()
        out.backward(g.permute(0, 3, 1, 2))
        _, idn = oc.ref_maxpool(xn.detach().permute(0, 2, 3, 1))
        dx = oc.ref_maxpool_bwd(g, idn, H, W)
        assert torch.equal(dx, xn.grad.permute(0, 2, 3, 1))
        # the adjoint identity <bwd(g), x> = <g, take(x, idx)> in float64 on exact values
        xf = xn.detach().permute(0, 2, 3, 1)
        assert float((dx * xf).sum()) == float((g * oc.ref_maxpool(xf)[0]).sum())


@pytest.mark.parametrize("H,W", oc.BIL_EXTENTS, ids=oc.ids)
def test_bilinear_and_nearest_restatements_against_aten(H, W):
    for C in oc.BIL_C:
        x = oc.lat((2, H, W, C), 8, 4, F32, H * 7 + W + C, "cpu").double()
        for s in oc.BIL_POW2 + oc.BIL_ODD:
            xn = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
            ya = F.interpolate(xn, scale_factor=s, mode="bilinear", align_corners=False)
            y = oc.ref_bilinear_fwd(x, s)
            dy = oc.lat(tuple(y.shape), oc.BIL_DY_INT, 4, F32, s, "cpu").double()
            ya.backward(dy.permute(0, 3, 1, 2))
            if s in oc.BIL_POW2:
                assert torch.equal(y, ya.detach().permute(0, 2, 3, 1)), (s, C)
                assert torch.equal(oc.ref_bilinear_bwd(dy, s), xn.grad.permute(0, 2, 3, 1)), (s, C)
                assert torch.equal(y.float().double(), y), "the forward is a float32 value"
            else:
                assert torch.allclose(y, ya.detach().permute(0, 2, 3, 1), rtol=0, atol=1e-5)
                assert bool((oc.ref_bilinear_fwd(x, s, absolute=True) >= y.abs() - 1e-12).all())
    x = oc.lat((2, 2 * H, 2 * W, 8), 127, 4, BF16, H + W, "cpu")
    xn = torch.zeros(2, 8, H, W, dtype=torch.float64, requires_grad=True)
    F.interpolate(xn, scale_factor=2, mode="nearest").backward(x.double().permute(0, 3, 1, 2))
    assert torch.equal(oc.ref_nearest2_bwd(x, F32).double(), xn.grad.permute(0, 2, 3, 1))
    if H * W > 1:
        assert not torch.equal(oc.ref_nearest2_bwd(x, BF16).double(), xn.grad.permute(0, 2, 3, 1)), "the bf16 2x2 sums need a rounding"


def test_heads_restatements_against_aten():
    N, HW, Ci = 3, 343, 16
    M = N * HW
    gt = oc.lat((N, 3, HW), 8, 4, F32, 1, "cpu")
    p = oc.lat((M, 3), 8, 4, F32, 2, "cpu").requires_grad_(True)
    loss = F.mse_loss(p.double().view(N, HW, 3).permute(0, 2, 1), gt.double())
    assert float(oc.ref_mse(p.detach(), gt, N, 3, HW)) == float(loss.float())
    loss.backward()
    dy = oc.ref_mse_bwd(p.detach(), gt, 1.0, N, HW, 8, F32)
    assert torch.allclose(dy[:, :3].double(), p.grad.double(), rtol=1e-6, atol=0) and bool((bits(dy[:, 3:]) == 0).all())
    x = oc.lat((M, Ci), 8, 4, BF16, 3, "cpu")
    g = oc.lat((M, 3), 8, 4, F32, 4, "cpu")
    w = oc.lat((3, Ci), 16, 8, F32, 5, "cpu")
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    (xd @ wd.t()).backward(g.double())
    dx, part = oc.ref_conv1x1_small_bwd(x, g, w, BF16)
    assert torch.equal(dx, xd.grad.to(BF16)) and part.shape == (2, 3 * Ci + 3)
    assert torch.equal(part.sum(0)[:3 * Ci].view(3, Ci), wd.grad) and torch.equal(part.sum(0)[3 * Ci:], g.double().sum(0))
    assert torch.equal(part[1, 3 * Ci:], g[1024:].double().sum(0))
    assert not torch.equal(dx.double(), xd.grad), "dx needs more than 8 bits somewhere"
    img = torch.randn(2, 3, 257, generator=torch.Generator().manual_seed(6))
    out = oc.ref_nchw_to_nhwc_pad(img, 2, 3, 257, BF16)
    assert torch.equal(out.view(2, 257, 8)[..., :3], img.permute(0, 2, 1).to(BF16)) and bool((bits(out[:, 3:]) == 0).all())
    assert not torch.equal(out[:, :3].float(), oc.nchw_to_rows(img, 2, 3, 257))
    assert torch.equal(oc.block_sums64(g)[0], g[:1024].double().sum(0)) and oc.block_sums64(g).shape == (2, 3)
