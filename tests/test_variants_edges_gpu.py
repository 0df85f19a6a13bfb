"""csrc/extras_groupnorm.hip and csrc/variants.hip at their edges: the coefficient kernels of norm='gn' / norm='in' (pcrl_gn_stats,
pcrl_gn_finalize, pcrl_gn_bwd_finalize), the two PReLU passes of act='prelu' (pcrl_prelu_fwd, pcrl_prelu_bwd), and the Python composition
around them in ops.py: the per-sample slicing of gn_forward_rows / gn_backward_rows, prelu_backward's slope reduction, and the one-channel
InstanceNorm head of luconv_forward / luconv_backward.  The activation codes inside the streaming kernels are pinned by
test_norm_pool_gpu.py and not repeated here.

The case table, the lattices and the restatements are in variant_cases.py; the preconditions are asserted by test_variant_cases_cpu.py.
Three kinds of bound, nothing else:
  exact    lattice operands, or a single float32 operation: the output equals the float64 value (or the float32 CPU value of the one
           operation), rounded to nearest even for bf16, at EVERY element
  derived  the derivation is in the test's docstring
  project  tests/test_ops_gpu.py, each times max|ref|: 1e-5 forward, 2e-4 dx, 1e-4 dgamma / dbeta, 1e-2 for a bf16 output (check())
Where a shape is ill-conditioned in float32 itself the bound is the larger of the project tolerance and 4 x the error of a plain float32
CPU evaluation of the same scale-and-shift formula against the same float64 reference (`yard=`, the rule of test_step_tail_gpu.py).
Raw entry points write into views of canary-filled buffers; inputs a kernel must not read past are followed in memory by poison.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import variant_cases as vc  # noqa: E402
from variant_cases import ACT_ELU, ACT_NONE, BF16, F32, F64  # noqa: E402
from pcrlv2_amd import ops  # noqa: E402
from pcrlv2_amd._lib import ACT_SIGMOID, PcrlError, dtype_code, lib, stream_handle  # noqa: E402

DEV = "cuda"
GUARD = 64
CANARY = -768.0        # a bf16 value that no case produces
POISON = 96.0          # finite, a bf16 value, far outside the lattices: a row read past the end moves every sum
U32 = 2.0 ** -24       # float32 unit roundoff


def call(name, *args):
    return lib().call(name, *args, stream_handle())


def guarded(n, dt=F32):
    """-> (a canary-filled buffer, its view of n elements GUARD elements from either end)"""
    full = torch.full((n + 2 * GUARD,), CANARY, dtype=dt, device=DEV)
    return full, full[GUARD:GUARD + n]


def intact(full, n, what, untouched=False):
    torch.cuda.synchronize()
    ok = bool((full[:GUARD] == CANARY).all()) and bool((full[GUARD + n:] == CANARY).all())
    assert ok, f"{what}: the canaries around the output were overwritten"
    if untouched:
        assert bool((full == CANARY).all()), f"{what}: a rejected call wrote to its output"


def padded(t, rows=600):
    """a contiguous device view holding t, followed in memory by `rows` rows (of t's trailing shape) of POISON"""
    t = t.to(DEV)
    flat = t.reshape(-1, t.shape[-1])
    buf = torch.full((flat.shape[0] + rows, flat.shape[1]), POISON, dtype=t.dtype, device=DEV)
    buf[:flat.shape[0]] = flat
    return buf[:flat.shape[0]].view(t.shape)


def same(got, want, what, bits=False):
    """every element equal in bits; NaN equals NaN; zeros of either sign are equal unless `bits`"""
    if got.is_cuda:
        torch.cuda.synchronize()
    got, want = got.detach().reshape(-1), want.detach().to(got.device).reshape(-1)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    it = torch.int16 if got.dtype == BF16 else torch.int32
    ok = (got.view(it) == want.view(it)) | (got.isnan() & want.isnan())
    if not bits:
        ok |= (got == 0) & (want == 0)
    bad = (~ok).nonzero().flatten()
    if bad.numel():
        first = [(int(i), float(got[i]), float(want[i])) for i in bad[:6]]
        raise AssertionError(f"{what}: {bad.numel()} of {got.numel()} elements differ; (flat index, got, want): {first}")


def back(t):
    torch.cuda.synchronize()
    return t.detach().double().cpu().contiguous()


def check(got, ref, tol, what, yard=None, log=None):
    """max|got - ref| <= tol * max|ref| (the convention of tests/test_ops_gpu.py), on whatever device ref is.  yard: the float32 CPU
    evaluation of the same formula; the bound becomes max(that, 4 x its own error against ref)."""
    torch.cuda.synchronize()
    ref = ref.detach().double()
    got = got.detach().double().to(ref.device).reshape(ref.shape)
    scale = max(float(ref.abs().max()), 1e-6)
    bound, y_err = tol * scale, None
    if yard is not None:
        y_err = float((yard.detach().double().to(ref.device).reshape(ref.shape) - ref).abs().max())
        bound = max(bound, 4 * y_err)
    err = float((got - ref).abs().max())
    line = f"  {what}: max|d|={err:.3e} bound={bound:.3e} (project {tol * scale:.3e}" + (f", float32 yardstick {y_err:.3e})" if yard is not None else ")")
    if log is None:
        print(line)
    else:
        log.append(line)
    assert err <= bound, f"{what}: max|d|={err:.3e} > {bound:.3e} (ref max {scale:.3e})" + (f", float32 yardstick {y_err:.3e}" if yard is not None else "")
    return err


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g, dtype=F64) * 2 - 1) * scale


# ----------------------------------------------------------------------------------------------------------------------------------------
# 1. pcrl_gn_stats
# ----------------------------------------------------------------------------------------------------------------------------------------
def tile_sums64(y, S):
    """[N, S, C] -> float64 [N, tiles, C, 2]: (sum, sum of squares) over the rows of each 512-row tile"""
    N, _, C = y.shape
    tiles = vc.gn_tiles(S)
    y64 = torch.cat([y.double(), torch.zeros(N, tiles * vc.GN_TILE_ROWS - S, C, dtype=F64, device=y.device)], 1).view(N, tiles, vc.GN_TILE_ROWS, C)
    return torch.stack([y64.sum(2), (y64 * y64).sum(2)], dim=3)


@pytest.mark.parametrize("C,dt", vc.C_DT)
def test_gn_stats_partials_on_the_lattice(C, dt):
    """pcrl_gn_stats, exact.  y = i/4, |i| <= 8: every float32 sum of a 512-row tile is exact in any order, so each
    partial[n][tile][c][{0, 1}] equals the float64 sum bit for bit.  S = 1, 2 and the one-row last tiles of 513 / 1025 leave row slots idle
    (256 slots at C = 4 float32 and C = 8 bf16), which must contribute 0; 511 / 512 / 513 sit around GN_TILE_ROWS; N = 3 puts a sample's rows
    behind another's; C = 1024 float32 has a single row slot that walks all 512 rows.  Nothing outside the N * tiles * C * 2 floats is
    written, and the rows behind the input hold poison."""
    for S in vc.S_VALUES:
        for N in vc.N_VALUES:
            what = f"gn_stats C={C} {dt} S={S} N={N}"
            y = padded(vc.lat((N, S, C), vc.Y_INT, vc.Y_DEN, dt, seed=S + N + C, device=DEV))
            tiles = lib().call("pcrl_gn_stats_tiles", S)
            assert tiles == vc.gn_tiles(S)
            n = N * tiles * C * 2
            full, out = guarded(n)
            call("pcrl_gn_stats", y, out, N, S, C, dtype_code(dt))
            intact(full, n, what)
            same(out, tile_sums64(y, S).float(), what)


def badly_centred(ratio, dt, N=3, S=1025, C=512):
    """CPU float64 [N, S, C] holding dt values: uniform(-1, 1) moved to `ratio` (+-10 %) standard deviations per (sample, channel)"""
    y0 = rnd(N, S, C, seed=1)
    return (y0 + ratio * y0.std(dim=1, keepdim=True) * (1 + 0.1 * rnd(N, 1, C, seed=3))).to(dt).double()


@pytest.mark.parametrize("dt", [F32, BF16])
def test_gn_stats_partials_are_float64_sums_rounded_once(dt):
    """pcrl_gn_stats, derived, on data that is NOT exactly summable in float32 (mean at 100 standard deviations, C = 512, S = 1025, N = 3:
    squares near 3300, tile sums near 1.7e6).  The kernel adds a tile's rows in float64 -- 512 terms: a relative error below 512 * 2^-53
    = 6e-14, a 10^-6 of a float32 ulp -- and rounds once, so each partial is the float32 rounding of the float64 sum or, where that sum
    lies within 6e-14 of a rounding boundary, its neighbour: at most ONE float32 ulp from the float64 reference.  (A float32 running
    sum is some tens of ulps off here.)"""
    N, S, C = 3, 1025, 512
    y = badly_centred(100.0, dt).to(dt).to(DEV)
    tiles = vc.gn_tiles(S)
    n = N * tiles * C * 2
    full, out = guarded(n)
    call("pcrl_gn_stats", padded(y), out, N, S, C, dtype_code(dt))
    intact(full, n, "gn_stats")
    ref = tile_sums64(y, S).reshape(-1)
    err = (out.double() - ref).abs()
    worst = float((err / vc.ulp32(ref)).max())
    print(f"  gn_stats {dt}: worst partial {worst:.3f} float32 ulp from the float64 sum")
    assert worst <= 1.0


# ----------------------------------------------------------------------------------------------------------------------------------------
# 2. pcrl_gn_finalize
# ----------------------------------------------------------------------------------------------------------------------------------------
def run_finalize(partial, N, C, G, S, gamma, beta, what):
    tiles = partial.shape[1]
    full, out = guarded(4 * N * C)
    o = [out[k * N * C:(k + 1) * N * C] for k in range(4)]
    call("pcrl_gn_finalize", padded(partial), tiles, N, S, C, G, gamma.to(DEV), beta.to(DEV), 1e-5, *o)
    intact(full, 4 * N * C, what)
    return [back(t).view(N, C) for t in o]


def check_finalize(got, partial, N, C, G, S, gamma, beta, what):
    mean_d, rstd_d, scale_d, shift_d = got
    s = vc.serial_sum64(partial)
    mu, rstd, _, _ = vc.gn_finalize_ref(s[..., 0], s[..., 1], S, G, gamma, beta)
    mu_c, rstd_c = vc.per_channel(mu, C), vc.per_channel(rstd, C)
    assert bool(((mean_d - mu_c).abs() <= 2.0 ** -23 * mu_c.abs()).all()), f"{what}: mean_c, worst {float(((mean_d - mu_c).abs() / mu_c.abs()).max()):.3e}"
    assert bool(((rstd_d - rstd_c).abs() <= 2.0 ** -23 * rstd_c).all()), f"{what}: rstd_c, worst {float(((rstd_d - rstd_c).abs() / rstd_c).max()):.3e}"
    same(scale_d.float(), (gamma.double() * rstd_d).float(), f"{what}: scale = fl32(gamma * rstd_c)")
    p = mean_d * scale_d
    bound = 2 * vc.ulp32(torch.maximum(beta.double().abs().expand_as(p), p.abs()))
    err = (shift_d - (beta.double() - p)).abs()
    assert bool((err <= bound).all()), f"{what}: shift, worst {float((err / bound).max()):.3f} of the bound"


@pytest.mark.parametrize("case", vc.FINALIZE_CASES)
def test_gn_finalize_on_hand_made_partials(case):
    """pcrl_gn_finalize, derived + exact, on the float32 partials of variant_cases.finalize_partials (poison behind them): G > 256 -- the
    `g += 256` loop takes a second trip, with one and with two channels per group --, one to three tiles, one group of 1024 channels, N = 3.
    mean_c, rstd_c: within 2^-23 relative of the float64 restatement on the same partials: 2^-24 for the final rounding to float32 and as
    much again for the float64 evaluation, whose cancellation in b / cnt - mu^2 amplifies a last-bit difference by mu^2 / var + 1 < 100
    (asserted on the CPU, where 2^20 would still do), and whose sums may be taken in another order (no cancellation: asserted on the CPU).
    scale: ONE float32 multiply of gamma and the stored rstd_c, hence bit for bit fl32(gamma * rstd_c) of the device's own rstd_c.
    shift = beta - mean * scale, as two roundings or one (FMA): |p - mean scale| <= ulp(p) / 2 and the subtraction's rounding is at most
    ulp(2 max(|beta|, |p|)) / 2 = ulp(max): 1.5 ulp of max(|beta|, |mean scale|) at most; the bound is 2 ulp."""
    N, C, G, S = case
    partial, gamma, beta = vc.finalize_partials(N, C, G, S, seed=C + G + S)
    what = f"gn_finalize N={N} C={C} G={G} S={S}"
    got = run_finalize(partial, N, C, G, S, gamma, beta, what)
    check_finalize(got, partial, N, C, G, S, gamma, beta, what)
    mean_d = got[0].view(N, G, C // G)
    assert torch.equal(mean_d, mean_d[:, :, :1].expand_as(mean_d)), f"{what}: mean_c differs within a group"


def test_gn_finalize_clamps_a_negative_variance():
    """`if (var < 0.0) var = 0.0`: three rows of the constant 1000 with a sum of squares one float32 step below 3e6: b / cnt - mu^2 = -1/12 in
    float64.  rstd must be fl32(1 / sqrt(eps)) (within the 2^-23 of the finalize test; eps the float32 value), not NaN."""
    C = 4
    partial = vc.clamp_partials(C)
    gamma, beta = torch.tensor([1.0, -2.0, 0.5, 1.5]), torch.tensor([0.0, 0.25, -0.5, 1.0])
    mean_d, rstd_d, scale_d, shift_d = run_finalize(partial, 1, C, C, 3, gamma, beta, "gn_finalize clamp")
    want = float(np.float32(1.0 / math.sqrt(vc.EPS32)))
    assert not bool(rstd_d.isnan().any()) and bool(((rstd_d - want).abs() <= 2.0 ** -23 * want).all()), (rstd_d, want)
    assert bool((mean_d == 1000.0).all())
    check_finalize((mean_d, rstd_d, scale_d, shift_d), partial, 1, C, C, 3, gamma, beta, "gn_finalize clamp")


# ----------------------------------------------------------------------------------------------------------------------------------------
# 3. pcrl_gn_bwd_finalize
# ----------------------------------------------------------------------------------------------------------------------------------------
def run_bwd_finalize(partial, N, C, G, S, gamma, mean_c, rstd_c, what):
    rows_b = partial.shape[1]
    full, out = guarded(5 * N * C)
    o = [out[k * N * C:(k + 1) * N * C] for k in range(5)]
    call("pcrl_gn_bwd_finalize", padded(partial), rows_b, N, S, C, G, gamma.to(DEV), mean_c.to(DEV), rstd_c.to(DEV), *o)
    intact(full, 5 * N * C, what)
    torch.cuda.synchronize()
    return [t.detach().cpu().view(N, C) for t in o]       # k1, kB, kA, dgamma_n, dbeta_n (float32)


@pytest.mark.parametrize("case", vc.BWD_FINALIZE_CASES)
def test_gn_bwd_finalize_on_the_lattice(case):
    """pcrl_gn_bwd_finalize, exact.  Dyadic partials, gamma = j/4, S * cpg a power of two, rstd in {1/2, 1, 2}, mean = j/8, the partials
    sized so that m1, m2, k1, kB, kA and (r r m2) mu have at most 24 significant bits (test_variant_cases_cpu.py): every float32 product and
    sum is exact with or without FMA contraction, and all five outputs equal the float64 restatement bit for bit.  G > 256 (1024 groups
    of one, 512 groups of two channels), rows_b > 1 (the [N][rows_b][C][2] stride), N = 3 (the n * C offsets of all eight vectors), one
    group of 1024 channels."""
    N, C, G, S, rows_b = case
    la = vc.BwdLattice(N, C, G, rows_b, seed=C + G + rows_b)
    what = f"gn_bwd_finalize N={N} C={C} G={G} S={S} rows_b={rows_b}"
    got = run_bwd_finalize(la.partial, N, C, G, S, la.gamma, la.mean_c, la.rstd_c, what)
    s = vc.serial_sum64(la.partial)
    ref = vc.gn_bwd_coef_ref(s[..., 0], s[..., 1], S, G, la.gamma, la.mean_c, la.rstd_c)
    for name, g, r in zip(("k1", "kB", "kA", "dgamma_n", "dbeta_n"), got, ref):
        same(g, r.float(), f"{what}: {name}")


def test_gn_bwd_finalize_on_random_operands():
    """pcrl_gn_bwd_finalize, derived, nothing a power of two (C = 96, G = 12, S = 77, rows_b = 3, N = 3).  u = 2^-24.
    dgamma_n, dbeta_n: the float64 sum of the rows in the kernel's order, rounded once: bit for bit.  k1 = r * gamma: one multiply: bit for bit.
    kB = (-r * r) * m2 with m2 = fl32(float64 value): three roundings, |error| <= 4u |kB|.
    kA = ((r * r) * m2) * mu - r * m1 =: T1 - T2: T1 carries the rounding of m2 and three multiplies (4u |T1|), T2 that of m1 and one
    multiply (2u |T2|), the subtraction u |T1 - T2| (none of it lost if contracted): |error| <= 5u |T1| + 3u |T2| <= 6u (|T1| + |T2|)."""
    N, C, G, S, rows_b = vc.BWD_FINALIZE_RANDOM
    g = torch.Generator().manual_seed(11)
    partial = torch.randn(N, rows_b, C, 2, generator=g)
    gamma = (torch.rand(C, generator=g) + 0.5) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1).float()
    mean_c = vc.per_channel(torch.randn(N, G, generator=g), C).contiguous()
    rstd_c = vc.per_channel(torch.rand(N, G, generator=g) + 0.5, C).contiguous()
    what = "gn_bwd_finalize random"
    k1, kB, kA, dg, db = run_bwd_finalize(partial, N, C, G, S, gamma, mean_c, rstd_c, what)
    s = vc.serial_sum64(partial)
    r_k1, r_kB, r_kA, r_dg, r_db = vc.gn_bwd_coef_ref(s[..., 0], s[..., 1], S, G, gamma, mean_c, rstd_c)
    same(dg, r_dg.float(), f"{what}: dgamma_n")
    same(db, r_db.float(), f"{what}: dbeta_n")
    same(k1, r_k1.float(), f"{what}: k1")
    assert bool(((kB.double() - r_kB).abs() <= 4 * U32 * r_kB.abs()).all()), f"{what}: kB, worst {float(((kB.double() - r_kB).abs() / r_kB.abs()).max() / U32):.2f} u"
    cnt = float(S * (C // G))
    r, mu = rstd_c.double(), mean_c.double()
    T1 = r * r * vc.per_channel(vc.group_sum(gamma.double() * s[..., 1], G) / cnt, C) * mu
    T2 = r * vc.per_channel(vc.group_sum(gamma.double() * s[..., 0], G) / cnt, C)
    assert torch.allclose(T1 - T2, r_kA, rtol=1e-12, atol=0)
    bound = 6 * U32 * (T1.abs() + T2.abs())
    assert bool(((kA.double() - r_kA).abs() <= bound).all()), f"{what}: kA, worst {float(((kA.double() - r_kA).abs() / bound).max()):.3f} of the bound"


# ----------------------------------------------------------------------------------------------------------------------------------------
# 4. pcrl_prelu_fwd
# ----------------------------------------------------------------------------------------------------------------------------------------
SPECIALS = (0.0, -0.0, math.inf, -math.inf, math.nan)


def prelu_random(M, C, dt, seed):
    """-> (z [M, C] in dt with +-0, +-inf and NaN sprinkled in, slopes float32 [C] of both signs (and one 0 where C allows))  -- CPU"""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(M, C, generator=g)
    flat = z.view(-1)
    for k in range(min(3 * len(SPECIALS), max(flat.numel() // 2, 1))):
        flat[(k * 7919 + k // len(SPECIALS)) % flat.numel()] = SPECIALS[k % len(SPECIALS)]
    w = torch.randn(C, generator=g) * 0.5
    w[0] = -0.75                     # +0 and -0 under a negative slope: w * z is the zero of the OTHER sign
    z[0, 0], z[M - 1, 0] = 0.0, (-0.0 if M > 1 else 0.0)
    if C > 4:
        w[3] = 0.0
    return z.to(dt), w


def prelu_fwd32(z, w):
    """the float32 CPU evaluation: one multiply, then the rounding to nearest even of the storage type"""
    zf = z.float()
    return torch.where(zf > 0, zf, w * zf).to(z.dtype)


def run_prelu_fwd(z, w, M, C, dt, what):
    full, out = guarded(M * C, dt)
    call("pcrl_prelu_fwd", z.to(DEV), w.to(DEV), out, M, C, dtype_code(dt))
    intact(full, M * C, what)
    return out.cpu().view(M, C)


@pytest.mark.parametrize("dt,C", vc.PRELU_C)
def test_prelu_forward_bit_for_bit(dt, C):
    """pcrl_prelu_fwd, exact: a = z > 0 ? z : w[c] * z is a select and ONE float32 multiply, so the output equals the float32 CPU
    torch.where(z > 0, z, w * z), rounded to nearest even for bf16, in bits -- signed zeros included (-0 and +0 both take w * z), NaN as NaN
    (NaN > 0 is false, w * NaN is NaN; 0 * inf is NaN on both sides).  M = 1, 255, 256, 257, 513; slopes of both signs."""
    for M in vc.PRELU_M:
        z, w = prelu_random(M, C, dt, seed=M + C)
        what = f"prelu_fwd {dt} C={C} M={M}"
        same(run_prelu_fwd(z, w, M, C, dt, what), prelu_fwd32(z, w), what, bits=True)


def test_prelu_forward_past_the_grid_cap():
    """`< 4096 ? ... : 4096`: C = 32 float32 with M = 131 075 rows is 1 048 600 channel vectors, 24 past 4096 blocks x 256 threads: the
    grid-stride loop takes a second step for the first 24 threads of block 0 only, whose channel offset (i % nvec) * VEC must be that of
    vector 1 048 576 + t, not of t.  16 MB; the canaries behind the output catch a step too many."""
    dt, C, M = vc.PRELU_BIG
    z, w = prelu_random(M, C, dt, seed=1)
    same(run_prelu_fwd(z, w, M, C, dt, "prelu_fwd past the cap"), prelu_fwd32(z, w), "prelu_fwd past the cap", bits=True)


# ----------------------------------------------------------------------------------------------------------------------------------------
# 5. pcrl_prelu_bwd + pcrl_colsum through ops.prelu_backward
# ----------------------------------------------------------------------------------------------------------------------------------------
def as_act(t):
    """[M, C] -> the [1, C, M, 1, 1] activation (NDHWC memory) on the device"""
    M, C = t.shape
    return t.to(DEV).contiguous().view(1, M, 1, 1, C).permute(0, 4, 1, 2, 3)


def rows_of(a):
    torch.cuda.synchronize()
    return a.permute(0, 2, 3, 4, 1).reshape(-1, a.shape[1]).cpu()


@pytest.mark.parametrize("dt,C", vc.PRELU_C)
def test_prelu_backward_on_the_lattice(dt, C):
    """pcrl_prelu_bwd and the slope reduction (ops.prelu_backward: per-tile partials, then pcrl_colsum), exact.  z, da = i/4, |i| <= 8
    with z = 0 present, w = j/8: w * da and da * z are exact and a column sum of M <= 131 075 rows stays below 2^24 units of 1/16, so dz
    and dslope equal the float64 restatement of aten::prelu_backward bit for bit: a row with z == 0 takes w * da and adds 0 to the slope
    gradient.  M = 1, 255, 256, 257, 513 around PRELU_TILE_ROWS; in float32 at C = 32 also the 131 075 rows of the grid-cap case (513 tiles)."""
    Ms = vc.PRELU_M + ([vc.PRELU_BIG[2]] if (dt, C) == vc.PRELU_BIG[:2] else [])
    for M in Ms:
        z, da = (vc.lat((M, C), vc.Y_INT, vc.Y_DEN, dt, seed=M + C + k) for k in (0, 1))
        w = vc.lat((C,), vc.W_INT, vc.W_DEN, F32, seed=C)
        what = f"prelu_bwd lattice {dt} C={C} M={M}"
        dz, dslope = ops.prelu_backward(as_act(da), as_act(z), w.to(DEV), dt)
        r_dz, r_dw = vc.prelu_bwd_ref(da, z, w)
        same(rows_of(dz), r_dz.to(dt), f"{what}: dz")
        same(dslope.cpu(), r_dw.float(), f"{what}: dslope")
        if M >= 255:
            zero = (z == 0)
            assert bool(zero.any()) and torch.equal(rows_of(dz)[zero].double(), (w.double() * da.double())[zero]), f"{what}: rows with z == 0"


@pytest.mark.parametrize("dt,C", vc.PRELU_C)
def test_prelu_backward_on_random_data(dt, C):
    """dz = z > 0 ? da : w[c] * da is one multiply: bit for bit against the float32 CPU evaluation (rounded to nearest even for bf16).
    dslope: the project's 1e-4 x max|ref| of dgamma / dbeta (tests/test_ops_gpu.py) against the float64 restatement."""
    for M in vc.PRELU_M:
        g = torch.Generator().manual_seed(M + C)
        z, da = torch.randn(M, C, generator=g).to(dt), torch.randn(M, C, generator=g).to(dt)
        z[M // 2, :] = 0.0
        w = torch.randn(C, generator=g) * 0.5
        what = f"prelu_bwd random {dt} C={C} M={M}"
        dz, dslope = ops.prelu_backward(as_act(da), as_act(z), w.to(DEV), dt)
        same(rows_of(dz), torch.where(z.float() > 0, da.float(), w * da.float()).to(dt), f"{what}: dz", bits=True)
        log = []
        check(dslope.cpu(), vc.prelu_bwd_ref(da, z, w)[1], 1e-4, f"{what}: dslope", log=log)


# ----------------------------------------------------------------------------------------------------------------------------------------
# 6. ops.gn_forward_rows / ops.gn_backward_rows
# ----------------------------------------------------------------------------------------------------------------------------------------
def gn_device(y, da, gamma, beta, G, act, dt):
    a, saved = ops.gn_forward_rows(y.to(dt).to(DEV).contiguous(), gamma.to(DEV), beta.to(DEV), G, act, dt)
    dy, dg, db = ops.gn_backward_rows(da.to(dt).to(DEV).contiguous(), saved, gamma.to(DEV), G, act, dt)
    return a, dy, dg, db, saved


def check_gn(got, ref, dt, what, yard=None, log=None):
    a, dy, dg, db = got[:4]
    out_tol, dx_tol = (1e-2, 1e-2) if dt == BF16 else (1e-5, 2e-4)
    y = yard or {}
    check(a, ref["out"], out_tol, f"{what}: output", y.get("out"), log)
    check(dy, ref["dx"], dx_tol, f"{what}: dx", y.get("dx"), log)
    check(dg, ref["dgamma"], 1e-4, f"{what}: dgamma", y.get("dgamma"), log)
    check(db, ref["dbeta"], 1e-4, f"{what}: dbeta", y.get("dbeta"), log)


@pytest.mark.parametrize("C,G,dt", vc.CG_DT)
def test_groupnorm_rows_against_the_restatement(C, G, dt):
    """ops.gn_forward_rows / ops.gn_backward_rows, project bounds, for every (S, N) of the table and ACT_NONE / ACT_ELU: output, dx,
    dgamma, dbeta against the float64 restatement (on the device) of the float32- or bf16-rounded inputs of variant_cases.gn_inputs.
    N = 3: samples 1 and 2 take their coefficient rows from scale[n * C:], k1[n * C:], ... and write their partials at
    partial_b[n * rows_b * C * 2:]; the samples have different statistics, so a wrong offset moves the output by its own size.
    The inputs keep every group's variance above 1/5 (test_variant_cases_cpu.py), so the forward is well conditioned at every shape.  dx of
    a group of TWO values (variant_cases.ill_conditioned: S = 2 with G = C, S = 1 at (1024, 512)) is the residue of eps alone: terms of
    order 1 cancel to order eps / var in float32 whatever evaluates k1 dz + kB y + kA.  There the bound is the larger of the project tolerance
    and 4 x the float32 CPU yardstick.  Measured yardsticks of dx at those shapes: float32 30 .. 140 x the project tolerance
    (0.6 .. 2.8 % of max|dx|, which is itself of order 1e-5; 1e-7 .. 6e-7 absolute), bf16 0.4 .. 1.7 x; the kernels' own error there is
    0.2 .. 1 x the yardstick.  Output, dgamma and dbeta: 3 % of their tolerance at most."""
    for S, N in vc.sn_of(C, G):
        y, da, gamma, beta = vc.gn_inputs(N, S, C, G, dt, seed=S + N)
        yd, dad, gd, bd = y.to(DEV), da.to(DEV), gamma.to(DEV), beta.to(DEV)
        for act in (ACT_NONE, ACT_ELU):
            what = f"C={C} G={G} {dt} S={S} N={N} act={act}"
            ref = vc.gn_ref(yd, dad, gd, bd, G, act)
            yard = vc.gn_ref(y, da, gamma, beta, G, act, prec=F32) if vc.ill_conditioned(C, G, S) else None
            log = []
            try:
                check_gn(gn_device(y, da, gamma, beta, G, act, dt), ref, dt, what, yard, log)
            finally:
                if yard is not None:
                    print("\n".join(log))


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("ratio", [10.0, 100.0])
def test_groupnorm_statistics_of_a_badly_centred_group(ratio, dt):
    """InstanceNorm at C = G = 512, S = 1025, N = 3 with every channel's mean at `ratio` standard deviations: var = E[y^2] - mean^2 cancels.
    The relative error of rstd is reported and bounded as test_batch_statistics_on_badly_centred_channels (tests/test_ops_gpu.py) bounds
    BatchNorm's at the same ratio: 2e-5 (ratio 10) / 2e-3 (ratio 100), mean within 1e-4 standard deviations -- unless 4 x the float32 CPU
    yardstick (the same formula with torch's float32 sums) is larger.  Output and gradients: project bounds with the same yardstick rule.
    Measured, relative rstd error (float32 yardstick): with float32 running sums in pcrl_gn_stats, where one thread added up to 256 rows of
    a tile serially, float32 4.67e-5 (2.64e-5) at ratio 10 and 4.63e-3 (2.14e-3) at ratio 100 -- past BatchNorm's bounds, inside 4 x the
    yardstick; bf16 3.0e-6 (1.3e-5) and 4.3e-4 (1.2e-3).  The kernel now takes a tile's sums in float64 and rounds them once
    (test_gn_stats_partials_are_float64_sums_rounded_once): float32 6.7e-6 and 8.6e-4, bf16 3.0e-6 and 3.2e-4, inside BatchNorm's bounds."""
    N, S, C = 3, 1025, 512
    y = badly_centred(ratio, dt)
    da = rnd(N, S, C, seed=2).to(dt).double()
    gamma, beta = (1 + 0.3 * rnd(C, seed=4)).float(), (0.3 * rnd(C, seed=5)).float()
    ref = vc.gn_ref(y.to(DEV), da.to(DEV), gamma.to(DEV), beta.to(DEV), C, ACT_NONE)
    yard = vc.gn_ref(y, da, gamma, beta, C, ACT_NONE, prec=F32)
    got = gn_device(y, da, gamma, beta, C, ACT_NONE, dt)
    mean_d, rstd_d = back(got[4][1]).view(N, C), back(got[4][2]).view(N, C)
    mean_r, rstd_r = ref["mean"].cpu(), ref["rstd"].cpu()
    e_mean = float(((mean_d - mean_r).abs() * rstd_r).max())
    e_rstd = float(((rstd_d - rstd_r).abs() / rstd_r).max())
    y_rstd = float(((yard["rstd"].double() - rstd_r).abs() / rstd_r).max())
    bound = max(2e-5 if ratio <= 10 else 2e-3, 4 * y_rstd)
    print(f"  mean/std = {ratio:g} [{dt}]: max |mean - ref| / std = {e_mean:.2e}, max relative rstd error = {e_rstd:.2e} "
          f"(bound {bound:.2e}, float32 yardstick {y_rstd:.2e})")
    assert e_mean < 1e-4 and e_rstd <= bound
    check_gn(got, ref, dt, f"badly centred, ratio {ratio:g} {dt}", yard)


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("C,G", [(32, 8), (32, 32)])
def test_groupnorm_of_a_constant_group(C, G, dt):
    """y[n] = c_n, a lattice constant per sample (7/4, -2, 1/4): the sums are exact, var is exactly 0, rstd = 1 / sqrt(eps) = 316 and
    scale = gamma * 316.  Derived bound for the output against beta: with P = c * scale, shift = fl(beta - fl(P)) and out = fl(fl(P) + shift)
    (or either as an FMA): |out - beta| <= 2u |P| + u |beta - P| + u |out| <= 4u (|P| + |beta|) =: e, u = 2^-24 -- of the order of
    ulp(|c gamma| / sqrt(eps)).  A bf16 output adds its rounding, at most 2^-8 (|beta| + e): bf16 keeps 8 significant bits, half an ulp
    is up to 2^-8 of the value.  xhat is 0, every gradient must be finite."""
    N, S = 3, 513
    c = torch.tensor([1.75, -2.0, 0.25], dtype=F64)
    y = c.view(N, 1, 1).expand(N, S, C).contiguous()
    da = rnd(N, S, C, seed=7).to(dt).double()
    gamma, beta = (1 + 0.3 * rnd(C, seed=4)).float(), (0.3 * rnd(C, seed=5)).float()
    a, dy, dg, db, saved = gn_device(y, da, gamma, beta, G, ACT_NONE, dt)
    rstd = 1.0 / math.sqrt(vc.EPS32)
    assert bool(((back(saved[2]) - rstd).abs() <= 2.0 ** -23 * rstd).all()), "rstd of a constant group is not 1 / sqrt(eps)"
    P = c.view(N, 1) * back(saved[3]).view(N, C)             # the device's own scale
    bound = 4 * U32 * (P.abs() + beta.double().abs())
    if dt == BF16:
        bound = bound + 2.0 ** -8 * (beta.double().abs() + bound)
    err = (back(a) - beta.double()).abs().amax(1)
    print(f"  constant group C={C} G={G} {dt}: worst |out - beta| = {float(err.max()):.3e}, {float((err / bound).max()):.3f} of the bound")
    assert bool((err <= bound).all())
    for name, t in (("dx", dy), ("dgamma", dg), ("dbeta", db)):
        assert bool(torch.isfinite(back(t)).all()), f"constant group: {name} is not finite"


# ----------------------------------------------------------------------------------------------------------------------------------------
# 7. the one-channel InstanceNorm head
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [ACT_NONE, ACT_SIGMOID])
@pytest.mark.parametrize("vol", [(2, 2, 2), (6, 18, 19)])
def test_instancenorm_head(vol, act):
    """norm='in' deep-supervision head: ops.luconv_forward(..., inorm=True) with Co = 1 views the float32 map as [N][S / 4][4] with ONE group
    over four pseudo-channels; luconv_backward sums the four pseudo-channels' dgamma / dbeta.  N = 3, Ci = 32; D*H*W = 8 (two rows of the view)
    and 2052 = 4 * 513 (one 512-row tile and a last tile of ONE row).  Reference: float64 F.instance_norm on the float64 F.conv3d, autograd.
    float32 mode (the map and everything behind it is float32 in either mode; the bf16 convolutions are pinned by test_conv_to1_exact_gpu.py).
    Tolerances: the map 2e-5 (test_conv_to_one_channel, test_batchnorm_one_channel_sigmoid: check default); dx, dw, dgamma, dbeta 1e-4
    (test_batchnorm_one_channel_sigmoid's backward; test_conv_to_one_channel's 2e-5 / 3e-5 hold for an exact dy, here dy comes out of the
    normalisation's backward); the conv-bias gradient is exactly zero."""
    N, Ci = 3, 32
    D, H, W = vol
    x, w, b = rnd(N, Ci, D, H, W, seed=1), rnd(1, Ci, 3, 3, 3, seed=2, scale=0.2), rnd(1, seed=3)
    gamma, beta = torch.tensor([1.2], dtype=F64), torch.tensor([-0.1], dtype=F64)
    da = rnd(N, 1, D, H, W, seed=4)
    xq = x.float().double().requires_grad_(True)
    wr, br = w.float().double().requires_grad_(True), b.float().double().requires_grad_(True)
    gr, btr = gamma.float().double().requires_grad_(True), beta.float().double().requires_grad_(True)
    z = F.instance_norm(F.conv3d(xq, wr, br, padding=1), weight=gr, bias=btr, eps=vc.EPS32)
    ref = torch.sigmoid(z) if act == ACT_SIGMOID else z
    ref.backward(da.float().double())
    dev = lambda t: t.float().to(DEV).contiguous()
    packed = ops.PackedWeights("conv3")
    wd, gd = dev(w), dev(gamma)
    a, sv = ops.luconv_forward(ops.to_act(dev(x), F32), wd, dev(b), gd, dev(beta), None, None, packed, act, F32, inorm=True)
    assert a.shape == (N, 1, D, H, W) and a.dtype == F32
    check(a, ref.detach(), 2e-5, f"IN head {vol}: map")
    dx, dw, db, dg, dbeta = ops.luconv_backward(sv, dev(da), wd, gd, packed, F32)
    check(dx, xq.grad, 1e-4, f"IN head {vol}: dx")
    check(dw, wr.grad, 1e-4, f"IN head {vol}: dw")
    check(dg, gr.grad, 1e-4, f"IN head {vol}: dgamma")
    check(dbeta, btr.grad, 1e-4, f"IN head {vol}: dbeta")
    assert dg.shape == (1,) and dbeta.shape == (1,)
    assert bool((back(db) == 0).all()) and float(br.grad.abs().max()) < 1e-12, "the conv bias in front of InstanceNorm has a zero gradient"


def test_instancenorm_head_rejects_a_volume_that_is_no_multiple_of_four():
    N, Ci, D, H, W = 3, 32, 1, 2, 3
    dev = lambda t: t.float().to(DEV).contiguous()
    x, w = rnd(N, Ci, D, H, W, seed=1), rnd(1, Ci, 3, 3, 3, seed=2)
    with pytest.raises(PcrlError, match="multiple of 4"):
        ops.luconv_forward(ops.to_act(dev(x), F32), dev(w), dev(rnd(1)), dev(torch.ones(1)), dev(torch.zeros(1)), None, None,
                           ops.PackedWeights("conv3"), ACT_NONE, F32, inorm=True)


# ----------------------------------------------------------------------------------------------------------------------------------------
# 8. rejections
# ----------------------------------------------------------------------------------------------------------------------------------------
BAD_C = [(12, vc.PCRL_F32, "three channel vectors do not divide 256"), (6, vc.PCRL_F32, "no whole channel vector"),
         (2048, vc.PCRL_F32, "512 channel vectors"), (32, 7, "bad dtype code")]


@pytest.mark.parametrize("C,code,why", BAD_C)
def test_stats_and_prelu_reject_bad_channels_and_types(C, code, why):
    """C = 12 / 6 / 2048 in float32 and a dtype code of 7: PcrlError with the entry point's message, the canary-filled outputs untouched"""
    M = 8
    src = torch.zeros(M * max(C, 8), dtype=F32, device=DEV)
    w = torch.zeros(max(C, 8), dtype=F32, device=DEV)
    msg = "bad dtype 7" if code == 7 else None
    full, out = guarded(M * C * 2)
    with pytest.raises(PcrlError, match=msg or rf"gn_stats: C={C}: channel vectors must divide 256"):
        call("pcrl_gn_stats", src, out, 1, M, C, code)
    intact(full, M * C * 2, f"gn_stats {why}", untouched=True)
    with pytest.raises(PcrlError, match=msg or rf"prelu_fwd: M={M} C={C}: channel vectors of 4 must divide 256"):
        call("pcrl_prelu_fwd", src, w, out, M, C, code)
    intact(full, M * C * 2, f"prelu_fwd {why}", untouched=True)
    full2, part = guarded(C)
    with pytest.raises(PcrlError, match=msg or rf"prelu_bwd: M={M} C={C}: channel vectors of 4 must divide 256"):
        call("pcrl_prelu_bwd", src, src, w, out, part, M, C, code)
    intact(full, M * C * 2, f"prelu_bwd {why}", untouched=True)
    intact(full2, C, f"prelu_bwd {why}: partial", untouched=True)


def test_stats_and_prelu_reject_empty_tensors():
    """M or S of 0 (and N of 0 for the statistics)"""
    C = 32
    src, w = torch.zeros(8 * C, dtype=F32, device=DEV), torch.zeros(C, dtype=F32, device=DEV)
    full, out = guarded(8 * C)
    with pytest.raises(PcrlError, match="gn_stats: bad arguments"):
        call("pcrl_gn_stats", src, out, 1, 0, C, vc.PCRL_F32)
    with pytest.raises(PcrlError, match="gn_stats: bad arguments"):
        call("pcrl_gn_stats", src, out, 0, 8, C, vc.PCRL_F32)
    with pytest.raises(PcrlError, match=r"prelu_fwd: M=0 C=32"):
        call("pcrl_prelu_fwd", src, w, out, 0, C, vc.PCRL_F32)
    with pytest.raises(PcrlError, match=r"prelu_bwd: M=0 C=32"):
        call("pcrl_prelu_bwd", src, src, w, out, out, 0, C, vc.PCRL_F32)
    intact(full, 8 * C, "empty tensors", untouched=True)


@pytest.mark.parametrize("C,G,why", [(2048, 8, "C > 1024"), (32, 0, "G = 0"), (32, 5, "G does not divide C")])
def test_finalize_kernels_reject_bad_groups(C, G, why):
    """gn_check(): C = 2048 (the LDS rows hold 1024 channels), G = 0, G not dividing C: PcrlError `bad sizes ... (C <= 1024, G | C)`, outputs untouched"""
    N, S = 1, 8
    src = torch.zeros(N * C * 2, dtype=F32, device=DEV)
    full, out = guarded(5 * N * C)
    o = [out[k * N * C:(k + 1) * N * C] for k in range(5)]
    with pytest.raises(PcrlError, match=rf"gn_finalize: bad sizes N=1 S=8 C={C} G={G} \(C <= 1024, G \| C\)"):
        call("pcrl_gn_finalize", src, 1, N, S, C, G, src, src, 1e-5, *o[:4])
    with pytest.raises(PcrlError, match=rf"gn_bwd_finalize: bad sizes N=1 S=8 C={C} G={G} \(C <= 1024, G \| C\)"):
        call("pcrl_gn_bwd_finalize", src, 1, N, S, C, G, src, src, src, *o)
    intact(full, 5 * N * C, why, untouched=True)
