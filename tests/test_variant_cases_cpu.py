"""Preconditions of tests/test_variants_edges_gpu.py, checked without a GPU: the constants that variant_cases.py restates are the ones in
extras_groupnorm.hip / variants.hip; the case table reaches both sides of each of them; every "exact" case is exact in float32 in any order
and under any contraction (asserted analytically from the lattice bounds); the hand-made finalize partials are well conditioned; and the
float64 restatements agree with F.group_norm, F.instance_norm and F.prelu under float64 autograd to 1e-12 -- the only place where torch's
own operators are the judge."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import variant_cases as vc
from exact_lattice import EXACT_LIMIT, assert_exactly_summable
from variant_cases import ACT_ELU, ACT_NONE, BF16, F32, F64


def test_the_constants_of_the_sources_are_the_ones_the_case_table_was_built_for():
    assert vc.source_pins_missing() == []
    assert (vc.GN_TILE_ROWS, vc.PRELU_TILE_ROWS, vc.PRELU_GRID_CAP, vc.GN_C_MAX, vc.FINALIZE_STRIDE) == (512, 256, 4096, 1024, 256)


def test_source_pins_ignore_spacing_and_notice_a_changed_constant():
    assert vc.source_pins_missing([("extras_groupnorm.hip", "constexpr  int GN_TILE_ROWS=512 ;")]) == []
    for f, text, old, new in (("extras_groupnorm.hip", "constexpr int GN_TILE_ROWS = 512;", "512", "256"),
                              ("extras_groupnorm.hip", "for (int g = threadIdx.x; g < G; g += 256)", "256", "128"),
                              ("variants.hip", "(nv + 255) / 256 < 4096 ? (nv + 255) / 256 : 4096", "4096", "2048")):
        assert (f, text) in vc.SOURCE_PINS
        assert vc.source_pins_missing([(f, text.replace(old, new))]) == [(f, text.replace(old, new))]


def test_the_case_table_reaches_every_constant():
    pairs = set(vc.CG_PAIRS)
    assert {(C, G) for C in (32, 64, 128, 256, 512) for G in (8, C)} <= pairs                      # the model's own
    assert {(4, 1), (4, 4), (8, 8), (1024, 1024), (1024, 512), (1024, 1)} <= pairs
    assert (4, 4, F32) in vc.CG_DT and (8, 8, BF16) in vc.CG_DT and (4, 4, BF16) not in vc.CG_DT
    assert vc.nslots(4, F32) == 256 and vc.nslots(8, BF16) == 256 and vc.nslots(1024, F32) == 1     # one channel vector; one row slot
    assert all(vc.c_ok(C, dt) and C <= vc.GN_C_MAX and C % G == 0 for C, G, dt in vc.CG_DT)
    assert sum(G > vc.FINALIZE_STRIDE for C, G in pairs) >= 2 and any(G > vc.FINALIZE_STRIDE and G < C for C, G in pairs)
    assert {vc.gn_tiles(S) for S in vc.S_VALUES} == {1, 2, 3} and 1025 % vc.GN_TILE_ROWS == 1 and 513 % vc.GN_TILE_ROWS == 1
    assert {511, 512, 513} <= set(vc.S_VALUES) and vc.N_VALUES == [1, 3]
    for C, G in pairs:
        sn = vc.sn_of(C, G)
        assert ((1, 1) in sn) == (C // G > 1) and (2, 3) in sn and (1025, 3) in sn
    # a tile with fewer rows than slots: S = 1 / 2 / the one-row last tile against at least 2 slots
    assert any(vc.nslots(C, dt) > 2 for C, dt in vc.C_DT)
    # finalize / bwd_finalize: G > 256, several tiles / rows, N = 3
    assert any(G > 256 for _, _, G, _ in vc.FINALIZE_CASES) and any(vc.gn_tiles(S) == 3 for _, _, _, S in vc.FINALIZE_CASES)
    assert any(G > 256 and N == 3 for N, _, G, _, _ in vc.BWD_FINALIZE_CASES) and any(r > 1 for *_, r in vc.BWD_FINALIZE_CASES)
    for N, C, G, S, rows_b in vc.BWD_FINALIZE_CASES:
        cnt = S * (C // G)
        assert cnt & (cnt - 1) == 0, "S * cpg must be a power of two"
    N, C, G, S, rows_b = vc.BWD_FINALIZE_RANDOM
    assert (S * (C // G)) & (S * (C // G) - 1) != 0
    # PReLU: both sides of a tile, of two tiles, and of the forward grid cap
    assert {vc.prelu_rows(M) for M in vc.PRELU_M} == {1, 2, 3} and {255, 256, 257} <= set(vc.PRELU_M)
    assert all(vc.c_ok(C, dt) for dt, C in vc.PRELU_C) and {vc.nslots(C, dt) for dt, C in vc.PRELU_C} >= {1, 2, 32, 256}
    dt, C, M = vc.PRELU_BIG
    blocks, want = vc.prelu_grid(M, C, dt)
    nv = M * C // vc.vec(dt)
    assert blocks == vc.PRELU_GRID_CAP < want and (nv - vc.PRELU_GRID_CAP * 256) % 256 != 0 and nv > vc.PRELU_GRID_CAP * 256
    assert M * C * 4 <= 17 << 20
    assert all(vc.prelu_grid(m, c, d)[1] <= vc.PRELU_GRID_CAP for d, c in vc.PRELU_C for m in vc.PRELU_M)


def test_the_stats_lattice_is_exactly_summable_over_a_tile():
    """y = i/4, |i| <= 8: sum |y| over 512 rows in units of 1/4 and sum y^2 in units of 1/16 stay below 2^24; the values are bf16 values"""
    y_max = vc.Y_INT / vc.Y_DEN
    assert_exactly_summable(vc.GN_TILE_ROWS * y_max, 1 / vc.Y_DEN, "sum y of a tile")
    assert_exactly_summable(vc.GN_TILE_ROWS * y_max * y_max, 1 / vc.Y_DEN ** 2, "sum y^2 of a tile")
    t = vc.lat((64, 8), vc.Y_INT, vc.Y_DEN, F64, 1)
    assert torch.equal(t.to(BF16).double(), t) and float(t.abs().max()) == y_max and bool((t == 0).any())
    # a sample's sums in float64 over at most 3 tiles: trivially exact


def test_the_bwd_finalize_lattice_fits_24_bits():
    """m = K / (16 cnt) with K an integer: |K| < 2^24 makes m1, m2 float32 values; kB = -r^2 m2 only moves the exponent; kA is a multiple of
    1 / (16 cnt * 32) bounded by kA_units(), and so are its two terms and the intermediate (r r m2) mu.  k1 = r gamma is a power of two
    times a 4-bit integer."""
    for N, C, G, S, rows_b in vc.BWD_FINALIZE_CASES:
        cpg = C // G
        pi = vc.partial_int(cpg, rows_b)
        assert 1 <= pi <= vc.Y_INT
        assert cpg * vc.GAMMA_INT * pi * rows_b < EXACT_LIMIT
        assert vc.kA_units(cpg, rows_b, pi) < EXACT_LIMIT, (C, G, rows_b)
        # the double accumulations: integers below 2^53 in units of 1/16
        assert rows_b * pi < 2 ** 24
    assert vc.partial_int(1024, 1) == 8 and vc.partial_int(1024, 3) < 8
    # ... and numerically: float32 evaluation in another association and with products kept apart equals the float64 one
    for N, C, G, S, rows_b in vc.BWD_FINALIZE_CASES:
        la = vc.BwdLattice(N, C, G, rows_b, seed=C + G + rows_b)
        s = vc.serial_sum64(la.partial)
        ref = vc.gn_bwd_coef_ref(s[..., 0], s[..., 1], S, G, la.gamma, la.mean_c, la.rstd_c)
        s32 = la.partial.sum(1)
        got = vc.gn_bwd_coef_ref(s32[..., 0], s32[..., 1], S, G, la.gamma, la.mean_c, la.rstd_c, prec=F32)
        for k, (a, b) in enumerate(zip(got, ref)):
            assert a.dtype == F32 and torch.equal(a.double(), b), (C, G, S, rows_b, k)


def test_the_prelu_lattice_is_exact():
    """w da = (j/8)(i/4) and da z = (i/4)(k/4) are exact; a tile of 256 rows and the whole column (M rows, float32 column sums of float32
    partials) stay below 2^24 units of 1/16"""
    term = (vc.Y_INT / vc.Y_DEN) ** 2
    assert vc.W_INT * vc.Y_INT < 2 ** 8, "w da is a bf16 value: the bf16 output of the lattice cases is not rounded"
    for M in vc.PRELU_M + [vc.PRELU_BIG[2]]:
        assert_exactly_summable(M * term, 1 / vc.Y_DEN ** 2, f"slope gradient, M={M}")
    z = vc.lat((513, 8), vc.Y_INT, vc.Y_DEN, F32, 3)
    assert bool((z == 0).any()) and bool((z > 0).any()) and bool((z < 0).any())


@pytest.mark.parametrize("case", vc.FINALIZE_CASES)
def test_the_finalize_partials_are_well_conditioned(case):
    """mu^2 / var <= 2^20 for every group (the cancellation of b / cnt - mu^2 then amplifies the last float64 bit to less than 2^-32) and no
    cancellation in the mean: sum |s1| = |sum s1| for every group"""
    N, C, G, S = case
    partial, gamma, beta = vc.finalize_partials(N, C, G, S, seed=C + G + S)
    assert partial.shape == (N, vc.gn_tiles(S), C, 2) and partial.dtype == F32
    s = vc.serial_sum64(partial)
    mu, rstd, scale, shift = vc.gn_finalize_ref(s[..., 0], s[..., 1], S, G, gamma, beta)
    var = 1.0 / (rstd * rstd) - vc.EPS32
    assert float((mu * mu / var).max()) <= 2.0 ** 20 and float((mu * mu / var).max()) < 100
    assert torch.equal(vc.group_sum(s[..., 0].abs(), G), vc.group_sum(s[..., 0], G).abs())
    assert float(gamma.abs().min()) >= 0.5


def test_the_clamp_case_is_negative_in_float64():
    p = vc.clamp_partials(4).double()
    mu = p[0, 0, :, 0] / 3.0
    assert bool((p[0, 0, :, 1] / 3.0 - mu * mu < 0).all())
    mu, rstd, scale, shift = vc.gn_finalize_ref(p[:, 0, :, 0], p[:, 0, :, 1], 3, 4, torch.ones(4), torch.zeros(4))
    assert torch.equal(rstd, torch.full_like(rstd, 1.0 / np.sqrt(vc.EPS32)))


def close12(got, ref, what):
    err = float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)
    assert err <= 1e-12, f"{what}: relative error {err:.2e}"


@pytest.mark.parametrize("act", [ACT_NONE, ACT_ELU])
@pytest.mark.parametrize("C,G", [(32, 8), (8, 8), (4, 1), (12, 3)])
def test_groupnorm_restatement_against_aten(C, G, act):
    """gn_ref (and through it gn_forward_ref, gn_finalize_ref, gn_bwd_coef_ref) against F.group_norm -- F.instance_norm where G == C -- and
    F.elu with float64 autograd"""
    N, S = 3, 37
    g = torch.Generator().manual_seed(C + G)
    y = (torch.randn(N, S, C, generator=g, dtype=F64) + 0.3).requires_grad_(True)
    gamma = (torch.rand(C, generator=g, dtype=F64) + 0.5).requires_grad_(True)
    beta = (torch.rand(C, generator=g, dtype=F64) - 0.5).requires_grad_(True)
    da = torch.randn(N, S, C, generator=g, dtype=F64)
    x = y.permute(0, 2, 1)                                   # [N, C, S]
    z = F.instance_norm(x, weight=gamma, bias=beta, eps=vc.EPS32) if G == C else F.group_norm(x, G, gamma, beta, eps=vc.EPS32)
    a = F.elu(z) if act == ACT_ELU else z
    a.backward(da.permute(0, 2, 1))
    r = vc.gn_ref(y.detach(), da, gamma.detach(), beta.detach(), G, act)
    close12(r["out"], a.detach().permute(0, 2, 1), "output")
    close12(r["dx"], y.grad, "dx")
    close12(r["dgamma"], gamma.grad, "dgamma")
    close12(r["dbeta"], beta.grad, "dbeta")
    yd = y.detach()
    close12(r["mean"], yd.view(N, S, G, C // G).mean(dim=(1, 3)), "mean")
    close12(r["rstd"], 1 / torch.sqrt(yd.view(N, S, G, C // G).var(dim=(1, 3), unbiased=False) + vc.EPS32), "rstd")


def test_prelu_restatement_against_aten():
    g = torch.Generator().manual_seed(5)
    M, C = 41, 8
    z = torch.randn(M, C, generator=g, dtype=F64)
    z[::5] = 0.0
    zr = z.clone().requires_grad_(True)
    w = (torch.randn(C, generator=g, dtype=F64) * 0.5).requires_grad_(True)
    da = torch.randn(M, C, generator=g, dtype=F64)
    a = F.prelu(zr.t().unsqueeze(0), w)                      # [1, C, M]
    a.backward(da.t().unsqueeze(0))
    close12(vc.prelu_fwd_ref(z, w.detach()), a.detach()[0].t(), "prelu")
    dz, dw = vc.prelu_bwd_ref(da, z, w.detach())
    close12(dz, zr.grad, "prelu dz")
    close12(dw, w.grad, "prelu dslope")
    assert torch.equal(dz[::5], w.detach() * da[::5]), "a row with z == 0 takes w * da"


def test_the_float32_yardstick_is_the_same_formula():
    """prec=float32 evaluates the same expressions in float32 (the yardstick of the ill-conditioned cases): on a well-conditioned input it
    is within float32 rounding of the float64 one, on a group of two values it is not"""
    g = torch.Generator().manual_seed(9)
    y = torch.randn(2, 64, 8, generator=g).double()
    da = torch.randn(2, 64, 8, generator=g).double()
    gamma, beta = torch.ones(8), torch.zeros(8)
    r64, r32 = vc.gn_ref(y, da, gamma, beta, 2, ACT_NONE), vc.gn_ref(y, da, gamma, beta, 2, ACT_NONE, prec=F32)
    assert r32["out"].dtype == F32 and float((r32["out"].double() - r64["out"]).abs().max()) < 1e-5 * float(r64["out"].abs().max())
    assert vc.ill_conditioned(512, 512, 2) and vc.ill_conditioned(1024, 512, 1) and not vc.ill_conditioned(32, 8, 2) and not vc.ill_conditioned(1024, 1, 1)


@pytest.mark.parametrize("C,G", vc.CG_PAIRS)
def test_the_groupnorm_inputs_are_well_conditioned_in_every_group(C, G):
    """variant_cases.gn_inputs: mean^2 / var <= 16 in every group of every (S, N) of the table, in either storage type -- the forward is
    well conditioned everywhere, and only dx of a two-value group needs the yardstick"""
    for dt in vc.dtypes_of(C):
        for S, N in vc.sn_of(C, G):
            y, da, gamma, beta = vc.gn_inputs(N, S, C, G, dt, seed=S + N)
            assert torch.equal(y.to(dt).double(), y) and torch.equal(da.to(dt).double(), da) and y.shape == (N, S, C)
            yg = y.view(N, S, G, C // G)
            mu, var = yg.mean(dim=(1, 3)), yg.var(dim=(1, 3), unbiased=False)
            assert float(var.min()) >= 0.2 and float((mu * mu / var).max()) <= 16, (C, G, dt, S, N, float(var.min()))
