"""Preconditions of tests/test_norm_pool_gpu.py, checked without a GPU: the case table of norm_pool_cases.py reaches every tile size, both
sides of every cap, both ra_tile states and the non-temporal threshold; every "exact" case is exactly summable (asserted analytically from
the lattice bounds, no large tensor is built); the restatements agree with aten on the CPU."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_pool_cases as npc
from exact_lattice import EXACT_LIMIT, assert_exactly_summable
from norm_pool_cases import BF16, F32

# largest magnitudes, in lattice integers
GIN_MAX = 3 * 8                         # |da| + |da2| + |row term|, units of 1/4
GIN_UNIT = 1 / 4
RSTD_MIN, RSTD_MAX = 2.0 ** npc.RSTD_EXP[0], 2.0 ** npc.RSTD_EXP[1]
K1_MIN, K1_MAX = 2.0 ** npc.K1_EXP[0], 2.0 ** npc.K1_EXP[1]


def test_the_constants_of_the_source_are_the_ones_the_case_table_was_built_for():
    assert npc.source_pins_hold() == []


def test_elementwise_results_fit_24_bits_and_exceed_8():
    """z = scale y + shift in units of 1/16; dy = k1 dz + kB y + kA in units of k1_min/4 .. 1/16; dz (y - mean) rstd in units of 2^-6."""
    z_units = npc.SC_INT * npc.Y_INT + 2 * npc.SH_INT                       # (j/4)(i/4) + k/8 = (ij + 2k) / 16
    assert z_units < EXACT_LIMIT
    assert z_units > 256, "the forward never leaves the bf16 grid: the output rounding would not be exercised"
    unit = min(K1_MIN * GIN_UNIT, 1 / 16, 1 / 8)
    dy_max = K1_MAX * GIN_MAX * GIN_UNIT + (npc.KB_INT / 4) * (npc.Y_INT / 4) + npc.SH_INT / 8
    assert dy_max / unit < EXACT_LIMIT and dy_max / unit > 256
    s2_unit = GIN_UNIT * (1 / 8) * RSTD_MIN
    s2_max = GIN_MAX * GIN_UNIT * (npc.Y_INT / 4 + npc.MU_INT / 8) * RSTD_MAX
    assert s2_max / s2_unit < EXACT_LIMIT


def test_every_first_stage_partial_is_exactly_summable():
    """(rows of one first-stage partial) x (max |term| in units) < 2^24 for sum dz and for sum dz (y - mean) rstd, every reduce and pool case;
    for the column sums (rows of a tile) x max |a|."""
    s2_unit = GIN_UNIT * (1 / 8) * RSTD_MIN
    s2_max = GIN_MAX * GIN_UNIT * (npc.Y_INT / 4 + npc.MU_INT / 8) * RSTD_MAX
    for dt, C, M, row in npc.REDUCE_CASES + [(npc.NT_CASE[0], npc.NT_CASE[1], npc.NT_CASE[2] * npc.NT_CASE[3], None)]:
        rows = npc.bn_bwd_tile_rows(M)
        assert_exactly_summable(rows * GIN_MAX * GIN_UNIT, GIN_UNIT, f"sum dz, M={M}")
        assert_exactly_summable(rows * s2_max, s2_unit, f"sum dz xhat, M={M}")
    for dt, C, dims in npc.POOL_CASES + [npc.POOL_BIG]:
        rows = npc.bn_pool_tile(npc.pool_mp(dims))
        assert_exactly_summable(rows * s2_max, s2_unit, f"pooled sum dz xhat, {dims}")
    a_max = (npc.SC_INT * npc.Y_INT + 2 * npc.SH_INT) / 16
    for dt, C, N, S in npc.COL_CASES + [npc.NT_CASE]:
        assert_exactly_summable(min(S, npc.coltile_rows(N, S)) * a_max, 1 / 16, f"column tile, N={N} S={S}")
    assert_exactly_summable(1024 * 4.0, 1 / 16, "weighted column tile: x dy = (i/4)(j/4)")
    # second stages: float64 over at most 16 384 exact float32 partials of at most 2^24 units each: 2^38 < 2^53


def test_enumerated_and_special_window_cases_are_exact():
    """The pool-fusion cases on the enumerated windows use y = 1 + r/128 (r <= 7) with (scale, shift) = (1, 0), (1, 100), (-1, 0) or the lattice
    coefficients; those on the special windows use integers |y| <= 5 (next to NaN, inf and zeros) with the lattice coefficients.  Every finite
    elementwise result fits 24 bits, and a first-stage partial (at most bn_pool_tile() = 4 windows at these sizes) is exactly summable."""
    for y_max, y_unit, sh_max in ((1 + 7 / 128, 1 / 128, 100.0), (5.0, 1.0, npc.SH_INT / 8)):
        z_unit = y_unit / npc.SC_DEN if y_unit < 1 else 1 / 8                    # (j/4) y + k/8
        z_max = (npc.SC_INT / 4) * y_max + sh_max
        assert z_max / z_unit < EXACT_LIMIT
        dy_unit = min(K1_MIN * GIN_UNIT, y_unit / npc.KB_DEN, 1 / 8)
        dy_max = K1_MAX * (npc.Y_INT / 4) + (npc.KB_INT / 4) * y_max + npc.SH_INT / 8
        assert dy_max / dy_unit < EXACT_LIMIT
        s2_unit = GIN_UNIT * min(y_unit, 1 / 8) * RSTD_MIN
        s2_max = (npc.Y_INT / 4) * (y_max + npc.MU_INT / 8) * RSTD_MAX
        windows = max(npc.enumerated_windows().shape[0], npc.special_windows().shape[0])
        assert npc.bn_pool_tile(windows) == 4
        assert_exactly_summable(4 * s2_max, s2_unit, "pooled sum dz xhat, enumerated / special windows")
    assert float(npc.enumerated_windows().max()) == 7 and float(npc.special_windows().nan_to_num(nan=0.0, posinf=0.0, neginf=0.0).abs().max()) == 5


def test_pool_fusion_restatement_on_the_special_windows():
    """ref_pool_fused on channel 0 of the special windows through the identity, no activation: the all -inf window pools to -inf, keeps
    position 0 and enters the statistics with ybest = 0; a NaN window pools to NaN and its LAST NaN takes the gradient."""
    w = npc.special_windows().unsqueeze(-1)
    co = npc.Coef(1, 1, "cpu")
    co.scale[0], co.shift[0], co.kB[0], co.k1[0], co.kA[0], co.mean[0], co.rstd[0] = 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0
    gp = torch.arange(1, w.shape[0] + 1, dtype=F32).view(-1, 1)
    aw, p, s1, s2, dyw = npc.ref_pool_fused(w.float(), gp, co, npc.ACT_NONE, F32)
    assert float(p[0]) == -math.inf and bool(p[1:10].isnan().all())
    # kB = kA = 0, k1 = 1: dy is the routed gradient; it goes to a NaN position (0 * NaN + dp: NaN), so NO finite position carries it
    assert torch.equal(dyw[9, :, 0].nan_to_num(nan=-1.0), torch.tensor([-1.0, 0, 0, -1, 0, 0, 0, 0]))
    for k in range(8):
        assert torch.equal(dyw[1 + k, :, 0].nan_to_num(nan=-1.0), torch.tensor([-1.0 if t == k else 0.0 for t in range(8)]))
    assert torch.equal(npc.pool_arg(aw)[1:10, 0], torch.tensor([0, 1, 2, 3, 4, 5, 6, 7, 3]))
    assert float(s1[0]) == float(gp.sum())
    aw, p, s1, s2, dyw = npc.ref_pool_fused(w[:1].float(), gp[:1], co, npc.ACT_NONE, F32)
    assert float(s2[0]) == 0.0, "an all -inf window enters sum dz xhat with ybest = 0"


def test_source_pins_ignore_spacing_and_notice_a_changed_constant():
    text = npc.read_source("norm_pool.hip")
    hay = " ".join(npc._tokens(text.replace("r + 768 < rows", "r+768   <\n rows")))
    assert " ".join(npc._tokens("for (; r + 768 < rows; r += 1024)")) in hay
    assert " ".join(npc._tokens("for (; r + 768 < rows; r += 1024)")) not in " ".join(npc._tokens(text.replace("r + 768 < rows", "r + 769 < rows")))


def test_the_row_term_of_the_apply_cases_is_inexact():
    """g = i/8 times (float)(1.0 / S) at S = 1000 and 5000: most products are rounded, so the apply cases observe the kernel's rounding points"""
    for S in (1000, 5000):
        g = np.arange(-100, 101, dtype=np.float64) / 8
        prod64 = g * np.float64(np.float32(1.0 / S))
        assert ((g.astype(np.float32) * np.float32(1.0 / S)).astype(np.float64) != prod64).mean() > 0.5
        assert ((g.astype(np.float32) * np.float32(1.0 / S)).astype(np.float64) != g / S).mean() > 0.5


def test_the_row_term_lands_on_the_lattice_for_every_sample_size_of_the_table():
    """g = S m/4 and (float)(1.0 / S): the float32 product is m/4 exactly, so the sums of the reduce cases with a row term stay exact also
    where 1/S is not a power of two (61 696).  (The apply cases at S = 1000 and 5000 do not need this: there the float32 restatement of
    the row term determines the bits, and k1 is a power of two.)"""
    sizes = {row[1] for _, _, _, row in npc.REDUCE_CASES if row} | {npc.NT_CASE[3]}
    m = np.array(npc.ROW_M, dtype=np.float64)
    for S in sorted(sizes):
        g = (m * S / 4).astype(np.float32)
        assert (g.astype(np.float64) == m * S / 4).all(), S
        add = g * np.float32(1.0 / S)
        assert add.dtype == np.float32 and (add.astype(np.float64) == m / 4).all(), (S, add)


def test_the_case_table_reaches_every_constant():
    tiles = {npc.bn_bwd_tile_rows(M) for _, _, M, _ in npc.REDUCE_CASES}
    assert tiles == {32, 64, 128, 256, 512, 1024}
    assert {npc.bn_bwd_tile_rows(65535), npc.bn_bwd_tile_rows(65536)} == {32, 64}
    assert npc.bn_bwd_tile_rows((1 << 20) - 1) == 512 and npc.bn_bwd_tile_rows((1 << 20) + 37) == 1024 and ((1 << 20) + 37) % 1024 == 37
    passes = {npc.u4_passes(M, C, dt) for dt, C, M, _ in npc.REDUCE_CASES}
    assert {0, 1, 2, 4} <= passes
    assert (BF16, 8, (1 << 20) + 37, None) in npc.REDUCE_CASES and npc.u4_passes((1 << 20) + 37, 8, BF16) == 1
    # a last tile whose row count lies in (2 nslots, 3 nslots]: the unrolled loop must not start a pass whose fourth row is missing
    assert any(2 * npc.nslots(C, dt) < M % npc.bn_bwd_tile_rows(M) <= 3 * npc.nslots(C, dt) and npc.u4_passes(M, C, dt) >= 1
               for dt, C, M, _ in npc.REDUCE_CASES if C > 1)
    ra = {(S % npc.bn_bwd_tile_rows(M) == 0) for _, _, M, row in npc.REDUCE_CASES if row for S in [row[1]]}
    assert ra == {True, False}
    for _, _, M, row in npc.REDUCE_CASES:
        assert row is None or row[0] * row[1] == M
    ptiles = {npc.bn_pool_tile(npc.pool_mp(d)) for _, _, d in npc.POOL_CASES}
    assert ptiles == {4, 8, 16, 32, 64, 128}
    mps = sorted(npc.pool_mp(d) for _, _, d in npc.POOL_CASES)
    assert 8190 in mps and 8192 in mps and 16380 in mps and 16384 in mps
    assert any(mp >= 131072 and mp % 128 for mp in mps)
    # register-cached grid: both sides of 2048 blocks, every slot count, a remainder that is no multiple of the slots
    seen = set()
    for dt, C, M in npc.RC_CASES:
        assert npc.rc_ok(C, dt)
        ns = npc.nslots(C, dt)
        blocks, want = npc.rc_blocks(M, C, dt)
        seen.add((dt, ns, want > npc.RC_CAP))
        if want > npc.RC_CAP:
            assert ns == 1 or M % ns != 0
    for dt in (F32, BF16):
        assert {1, 4, 32, 128, 256} <= {ns for d, ns, wrapped in seen if d == dt and wrapped}
        assert any(d == dt and not wrapped for d, ns, wrapped in seen)
    for dt, C, N, S in npc.ROW_WRAP_CASES[:6]:
        assert npc.RC_CAP * npc.nslots(C, dt) == 4096 and N * S > 4096
    assert 4096 // 1000 == 4 and 4096 % 1000 == 96 and 4096 // 5000 == 0 and 4096 % 1024 == 0
    # generic kernels and grid_for
    for dt, C, M in npc.GENERIC_CASES + [npc.GENERIC_BIG]:
        assert not npc.rc_ok(C, dt) and (M * C) % npc.vec(dt) == 0
    dt, C, M = npc.GENERIC_BIG
    assert M * C // 4 > npc.CAP_ITEMS and (M * C // 4) % 256 != 0 and (npc.CAP_ITEMS * 4) % C != 0
    assert all(M * C // npc.vec(dt) < npc.CAP_ITEMS for dt, C, M in npc.GENERIC_CASES)
    dt, C, N, S = npc.GAP_BWD_BIG
    assert N * S * C // npc.vec(dt) > npc.CAP_ITEMS
    # column sums
    assert {npc.coltile_rows(N, S) for _, _, N, S in npc.COL_CASES} >= {32, 1024}
    counts = {npc.coltile_tiles(N, S) for _, _, N, S in npc.COL_CASES}
    assert {1, 7, 8, 9, 24, 25, 32, 33, 57, 4096} <= counts
    for S in (1023, 1024, 1025):
        assert npc.coltile_rows(512, S) == 1024
    assert {C for _, C, _, _ in npc.COL_CASES} >= {8, 16, 1024} and {N for _, _, N, _ in npc.COL_CASES} >= {1, 3}
    # non-temporal threshold
    dt, C, N, S = npc.NT_CASE
    assert N * S * C * npc.esize(dt) == npc.NT_BYTES == 201326592
    assert npc.streaming(N * S * C * npc.esize(dt)) and not npc.streaming((N * S - 1) * C * npc.esize(dt))
    dt, C, dims = npc.POOL_BIG
    assert npc.streaming(8 * npc.pool_mp(dims) * C * npc.esize(dt)) and npc.pool_mp(dims) * C // npc.vec(dt) > npc.CAP_ITEMS
    assert 8 * npc.pool_mp(dims) * C * npc.esize(dt) >= 512 << 20
    assert all(not npc.streaming(8 * npc.pool_mp(d) * C * npc.esize(dt)) for dt, C, d in npc.POOL_CASES)


def test_pool_restatement_against_aten_on_the_enumerated_windows():
    """pool_arg / ref_maxpool_bwd against F.max_pool3d float64 autograd on the CPU: single maxima, the 28 ties, all equal, all -inf, a NaN at
    each position, signed zeros."""
    w = torch.cat([npc.enumerated_windows(), npc.special_windows()]).unsqueeze(-1)
    x5 = npc.windows_to_volume(w)                                   # [1, 2, 2, 2 Wn, 1]
    assert torch.equal(npc.windows(x5).nan_to_num(nan=77.0), w.nan_to_num(nan=77.0))
    x = x5.permute(0, 4, 1, 2, 3).clone().requires_grad_(True)
    out = F.max_pool3d(x, 2)
    gy = torch.arange(1, w.shape[0] + 1, dtype=torch.float64).view(1, 1, 1, 1, -1)
    out.backward(gy)
    arg = npc.pool_arg(w)
    p = npc.take(w, arg)
    ref_p = out.detach().reshape(-1, 1)
    assert torch.equal(p.isnan(), ref_p.isnan()) and torch.equal(p.nan_to_num(nan=0.0), ref_p.nan_to_num(nan=0.0))
    dx = npc.unwindows(npc.ref_maxpool_bwd(arg, gy.reshape(-1, 1)), 1, 2, 2, 2 * w.shape[0])
    assert torch.equal(dx, x.grad.permute(0, 2, 3, 4, 1))
    assert int(arg[0]) == 0 and arg[:8, 0].tolist() == list(range(8))


def test_bf16_windows_that_differ_before_rounding_and_tie_after_it():
    """y = 1 + r/128 (bf16 values), scale 1, shift 100: z = 101 + r/128 is exact in float32 and rounds to 101 in bf16 for every r <= 7, so
    the argmax on the rounded activation is position 0 where the one on z is the position of the largest rank."""
    r = npc.enumerated_windows().unsqueeze(-1)
    y = (1 + r / 128).to(BF16)
    assert torch.equal(y.double(), 1 + r / 128)
    z = y.float() * 1.0 + 100.0
    assert torch.equal(z.double(), 101 + r / 128)
    a = z.to(BF16)
    assert bool((a.float() == 101).all())
    assert bool((npc.pool_arg(a) == 0).all())
    assert not bool((npc.pool_arg(z) == 0).all())


def test_the_clamp_case_is_negative_in_float64():
    s1, s2, count = npc.clamp_partials()
    mu = s1.double() / count
    assert bool((s2.double() / count - mu * mu < 0).all())


def test_finalize_restatement_against_aten():
    """finalize64 / bwd_finalize64 against float64 F.batch_norm autograd on a small tensor (the restatement is the reference of the 1-ulp
    tests, so it is itself checked here)."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(50, 4, generator=g, dtype=torch.float64).requires_grad_(True)
    gamma, beta = torch.randn(4, generator=g, dtype=torch.float64).requires_grad_(True), torch.randn(4, generator=g, dtype=torch.float64)
    rm, rv = torch.zeros(4, dtype=torch.float64), torch.ones(4, dtype=torch.float64)
    out = F.batch_norm(x, rm, rv, gamma, beta, training=True, momentum=0.1, eps=1e-5)
    dz = torch.randn(50, 4, generator=g, dtype=torch.float64)
    out.backward(dz)
    xd = x.detach()
    f = npc.finalize64(xd.sum(0), (xd * xd).sum(0), 50.0, gamma.detach(), beta, torch.zeros(4, dtype=torch.float64), torch.ones(4, dtype=torch.float64), 0.1, 1e-5)
    assert torch.allclose(f["running_mean"], rm, rtol=1e-12, atol=1e-14) and torch.allclose(f["running_var"], rv, rtol=1e-12)
    assert torch.allclose(f["scale"] * xd + f["shift"], out.detach(), rtol=1e-10, atol=1e-12)
    xhat = (xd - f["mean"]) * f["rstd"]
    b = npc.bwd_finalize64(dz.sum(0), (dz * xhat).sum(0), 50.0, gamma.detach(), f["mean"], f["rstd"])
    assert torch.allclose(b["k1"] * dz + b["kB"] * xd + b["kA"], x.grad, rtol=1e-9, atol=1e-11)
    assert torch.allclose(b["dgamma"], gamma.grad, rtol=1e-10)
    assert math.isfinite(float(b["kA"].sum()))


@pytest.mark.parametrize("dt", [F32, BF16])
def test_elementwise_restatements_on_a_small_lattice(dt):
    """ref_apply / ref_bwd_apply / ref_reduce: float32 evaluation in ANY association equals the float64 one on the lattice (CPU, small)."""
    C, M = 16, 300
    co = npc.Coef(C, 5, "cpu")
    y, da, da2 = (npc.lat((M, C), 8, 4, dt, s, "cpu") for s in (1, 2, 3))
    g = npc.row_term(3, C, 100, 4, "cpu")
    z32 = co.scale * y.float() + co.shift
    assert torch.equal(torch.relu(z32).to(dt), npc.ref_apply(y, co, npc.ACT_RELU, dt))
    gin = npc.ref_gin(M, C, "cpu", da, da2, g, 100)
    dz32 = torch.where(z32 > 0, gin, torch.zeros_like(gin))
    dy32 = co.kA + (co.kB * y.float() + co.k1 * dz32)                # another association than the kernel's
    assert torch.equal(dy32.to(dt), npc.ref_bwd_apply(gin, y, co, npc.ACT_RELU, dt))
    s1, s2 = npc.ref_reduce(gin, y, co, npc.ACT_RELU)
    assert torch.equal(dz32.sum(0).double(), s1)
    assert torch.equal(((y.float() - co.mean) * dz32 * co.rstd).flip(0).sum(0).double(), s2)
