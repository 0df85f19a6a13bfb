"""csrc/norm_pool.hip at its edges: the 3D BatchNorm statistics finalizes, apply and backward, the row-term / second-gradient /
global-average-pool / MaxPool fusions, MaxPool3d(2) itself and the tiled column sums -- at the sizes where a kernel changes path: the grid
caps of rc_grid() (2048 blocks) and grid_for() (16 384 blocks), every first-stage tile size, the four-way unrolls of the second stages, the
`c < C` guard, and the non-temporal twins that every full-resolution pass of a real step takes (pcrl_streaming(): 192 MiB per tensor).

Every test names the constant and the shape that crosses it; the case table, the lattices and the restatements are in norm_pool_cases.py, the
preconditions are asserted by test_norm_pool_cases_cpu.py.  Three kinds of bound, nothing else:
  exact    lattice operands (the coefficients are inputs of the ABI, so they sit on the lattice too): the output equals the float64 value, or
           its round-to-nearest-even rounding to bf16, at EVERY element; zeros compare equal whatever their sign, except where the operation
           only moves bits (MaxPool forward and backward); partial rows through assert_rows_exact
  derived  the two finalize kernels, one float32 ulp against a float64 restatement (derivation in the test's docstring)
  project  ELU, SiLU, sigmoid (expf): 2e-5 / 1e-2 x max|ref| as `check` of tests/test_ops_gpu.py
Inputs that a kernel must not read past are views into a larger buffer filled with a poison value; outputs are views into a buffer filled with
a sentinel that must survive behind them.  The large cases are generated, restated (float64, in chunks) and compared on the device.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import norm_pool_cases as npc  # noqa: E402
from exact_lattice import assert_bit_equal, assert_rows_exact  # noqa: E402
from norm_pool_cases import ACT_ELU, ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SILU, BF16, F32  # noqa: E402
from pcrlv2_amd import ops  # noqa: E402
from pcrlv2_amd._lib import PcrlError, dtype_code, lib, stream_handle  # noqa: E402

DEV = "cuda"
SENT = -768.0          # a bf16 value no lattice result reaches
POISON = 96.0          # finite, a bf16 value, far outside the lattice: a row read past the end moves every sum and every output
TAIL = 64
DTYPES = [F32, BF16]


def call(name, *args):
    return lib().call(name, *args, stream_handle())


def outbuf(n, dt):
    return torch.full((n + TAIL,), SENT, dtype=dt, device=DEV)


def tail_kept(buf, n, what):
    torch.cuda.synchronize()
    assert bool((buf[n:] == SENT).all()), f"{what}: the elements behind the output were written"


def padded(t, rows=2048):
    """a contiguous view holding t, followed in memory by `rows` rows of POISON"""
    buf = torch.full((t.shape[0] + rows,) + tuple(t.shape[1:]), POISON, dtype=t.dtype, device=t.device)
    buf[:t.shape[0]] = t
    return buf[:t.shape[0]]


def eq(got, want, what, bits=False):
    """device comparison on the bit views; zeros of either sign are equal unless `bits`; NaN equals NaN"""
    torch.cuda.synchronize()
    got, want = got.reshape(-1), want.reshape(-1)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    it = torch.int16 if got.dtype == BF16 else torch.int32
    if torch.equal(got.view(it), want.view(it)):
        return
    same = (got.view(it) == want.view(it)) | (got.isnan() & want.isnan())
    if not bits:
        same |= (got == 0) & (want == 0)
    bad = (~same).nonzero().flatten()
    if bad.numel():
        first = [(int(i), float(got[i]), float(want[i])) for i in bad[:6]]
        raise AssertionError(f"{what}: {bad.numel()} of {got.numel()} elements differ; (flat index, got, want): {first}")


def within_one_ulp(got, ref64, what):
    """|got - float32(ref64)| <= one float32 step: got is the rounding of ref64 or one of its two neighbours"""
    torch.cuda.synchronize()
    got, r = got.detach().cpu().float(), ref64.detach().cpu().float()
    up, dn = torch.nextafter(r, torch.full_like(r, math.inf)), torch.nextafter(r, torch.full_like(r, -math.inf))
    ok = (got >= dn) & (got <= up)
    assert bool(ok.all()), f"{what}: more than one float32 ulp off at {[(int(i), float(got[i]), float(ref64.cpu()[i])) for i in (~ok).nonzero().flatten()[:6]]}"


def inputs(M, C, dt, seed, n=3):
    return [npc.lat((M, C), 8, 4, dt, seed + k, DEV) for k in range(n)]


def chunks(M, step=1 << 19):
    return [(r, min(r + step, M)) for r in range(0, M, step)]


# ----------------------------------------------------------------------------------------------------------------------------------------
# launch wrappers
# ----------------------------------------------------------------------------------------------------------------------------------------
def k_apply(y, co, M, C, act, dt):
    out = outbuf(M * C, dt)
    call("pcrl_bn_act_apply", y, out, co.scale, co.shift, M, C, act, dtype_code(dt))
    tail_kept(out, M * C, "bn_act_apply")
    return out[:M * C].view(M, C)


VARIANTS = {   # name -> (entry, da, da2, row)
    "plain": ("", 1, 0, 0), "rowadd: da + row": ("_rowadd", 1, 0, 1), "rowadd: row only": ("_rowadd", 0, 0, 1), "sum: da only": ("_sum", 1, 0, 0),
    "sum: row only": ("_sum", 0, 0, 1), "sum: da + da2 + row": ("_sum", 1, 1, 1), "sum: da + da2": ("_sum", 1, 1, 0),
}


def grads_of(variant, da, da2, g, N, S, M):
    entry, u1, u2, ug = VARIANTS[variant]
    da, da2, g = da if u1 else None, da2 if u2 else None, g if ug else None
    if entry == "":
        head = (da,)
    elif entry == "_rowadd":
        head = (da, g, N, S)
    else:
        head = (da, da2, g, N if ug else 1, S if ug else M)
    return entry, head, da, da2, g


def k_bwd_apply(variant, da, da2, g, N, S, y, co, M, C, act, dt):
    entry, head, *_ = grads_of(variant, da, da2, g, N, S, M)
    out = outbuf(M * C, dt)
    call("pcrl_bn_act_bwd_apply" + entry, *head, y, out, co.scale, co.shift, co.k1, co.kB, co.kA, M, C, act, dtype_code(dt))
    tail_kept(out, M * C, "bn_act_bwd_apply" + entry)
    return out[:M * C].view(M, C)


def k_reduce(variant, da, da2, g, N, S, y, co, M, C, act, dt):
    entry, head, *_ = grads_of(variant, da, da2, g, N, S, M)
    rows = lib().call("pcrl_bn_bwd_partial_rows", M)
    assert rows == -(-M // npc.bn_bwd_tile_rows(M))
    out = outbuf(rows * C * 2, F32)
    call("pcrl_bn_act_bwd_reduce" + entry, *head, y, co.scale, co.shift, co.mean, co.rstd, out, M, C, act, dtype_code(dt))
    tail_kept(out, rows * C * 2, "bn_act_bwd_reduce" + entry)
    return out[:rows * C * 2].view(rows, C, 2), rows


def ref_gin_of(variant, da, da2, g, S, r0, r1, C):
    _, u1, u2, ug = VARIANTS[variant]
    return npc.ref_gin(r1 - r0, C, DEV, da[r0:r1] if u1 else None, da2[r0:r1] if u2 else None, g if ug else None, S, r0)


def check_bwd_finalize(partial, rows, C, M, co, s1, s2, what):
    """the second stage on the kernel's own partials: dbeta / dgamma are the float64 sums rounded ONCE to float32 (exact), k1 / kB / kA within
    one ulp of the float64 restatement of lines 101-107"""
    out = outbuf(5 * C, F32)
    o = [out[i * C:(i + 1) * C] for i in range(5)]
    call("pcrl_bn_bwd_finalize", partial, rows, C, float(M), co.gamma, co.mean, co.rstd, *o)
    tail_kept(out, 5 * C, what)
    assert_bit_equal(o[1], s1.cpu(), F32, f"{what}: dbeta")
    assert_bit_equal(o[0], s2.cpu(), F32, f"{what}: dgamma")
    ref = npc.bwd_finalize64(s1.cpu(), s2.cpu(), float(M), co.gamma.double().cpu(), co.mean.double().cpu(), co.rstd.double().cpu())
    for k, t in (("k1", o[2]), ("kB", o[3]), ("kA", o[4])):
        within_one_ulp(t, ref[k], f"{what}: {k}")


# ----------------------------------------------------------------------------------------------------------------------------------------
# 1. partial_pair_sum and the two finalizes
# ----------------------------------------------------------------------------------------------------------------------------------------
STAT_ROWS = [1, 255, 256, 257, 768, 769, 1024, 1025, 1793, 16384]
MOM32, EPS32 = float(np.float32(ops.BN_MOMENTUM)), float(np.float32(ops.BN_EPS))


def stat_partials(rows, C, seed):
    """[rows, C, 2] lattice pairs: s1 = i/4 with |i| <= 8, s2 = j/4 with 16 <= j <= 48 (so s2 / count > mu^2 at count = 4 rows), followed
    in memory by poison rows"""
    g = torch.Generator().manual_seed(seed)
    s1 = torch.randint(-8, 9, (rows, C), generator=g).float() / 4
    s2 = torch.randint(16, 49, (rows, C), generator=g).float() / 4
    p = torch.stack([s1, s2], dim=2).contiguous()
    return padded(p.to(DEV), rows=1100), p.double().sum(0)


def run_finalize(partial, rows, C, count, gamma, beta, rm, rv):
    out = outbuf(4 * C, F32)
    o = [out[i * C:(i + 1) * C] for i in range(4)]
    call("pcrl_bn_finalize", partial, rows, C, float(count), gamma, beta, rm, rv, ops.BN_MOMENTUM, ops.BN_EPS, *o)
    tail_kept(out, 4 * C, "bn_finalize")
    return dict(mean=o[0], rstd=o[1], scale=o[2], shift=o[3])


def affine(C, seed):
    g = torch.Generator().manual_seed(seed)
    t = [(torch.rand(C, generator=g) + 0.5).float(), (torch.rand(C, generator=g) - 0.5).float(), (torch.rand(C, generator=g) - 0.5).float(),
         (torch.rand(C, generator=g) + 0.5).float()]
    return t      # gamma, beta, running_mean, running_var (CPU float32)


def check_finalize(got, rm, rv, sums, count, gamma, beta, rm0, rv0, what):
    ref = npc.finalize64(sums[:, 0], sums[:, 1], float(count), gamma.double(), beta.double(), None if rm0 is None else rm0.double(),
                         None if rv0 is None else rv0.double(), MOM32, EPS32)
    for k in ("mean", "rstd", "scale", "shift"):
        within_one_ulp(got[k], ref[k], f"{what}: {k}")
    if rm is not None:
        within_one_ulp(rm, ref["running_mean"], f"{what}: running_mean")
        within_one_ulp(rv, ref["running_var"], f"{what}: running_var")
    return ref


@pytest.mark.parametrize("C", [1, 3, 32])
@pytest.mark.parametrize("rows", STAT_ROWS)
def test_finalize_statistics_rows(rows, C):
    """pcrl_bn_finalize / pcrl_bn_bwd_finalize, derived + exact.  partial_pair_sum (lines 39-57): a thread takes rows t, t + 256, ..., four at a
    time while `r + 768 < rows`: 768 / 769 sit on either side of the first unrolled pass for thread 0, 1024 / 1025 and 1793 leave tails of
    0 / 1 / several rows behind one or two passes, 255 / 256 / 257 are around one row per thread, 16 384 is the most a step produces.  The
    partial pairs are lattice values, the sums are float64 over exact float32 values, hence exact: dbeta and dgamma must be the float64 sums
    rounded once (bit-equal).  Derived bound for mean, rstd, scale, shift, the running statistics, k1, kB, kA: ONE float32 ulp against the
    numpy / torch float64 restatement of lines 73-85 and 101-107 on the same sums: both sides evaluate the same float64 formula, whose
    sqrt, divisions and products may differ in the last float64 bit between the device and the host, which can flip the final rounding to
    float32 to the neighbouring value but no further.  The rows behind the partials hold poison."""
    partial, sums = stat_partials(rows, C, seed=rows + C)
    gamma, beta, rm0, rv0 = affine(C, seed=C)
    rm, rv = rm0.to(DEV), rv0.to(DEV)
    count = 4 * rows
    got = run_finalize(partial, rows, C, count, gamma.to(DEV), beta.to(DEV), rm, rv)
    ref = check_finalize(got, rm, rv, sums, count, gamma, beta, rm0, rv0, f"bn_finalize rows={rows} C={C}")
    co = npc.Coef(C, 7, DEV)
    co.gamma, co.mean, co.rstd = gamma.to(DEV), ref["mean"].float().to(DEV), ref["rstd"].float().to(DEV)
    check_bwd_finalize(partial, rows, C, count, co, sums[:, 0], sums[:, 1], f"bn_bwd_finalize rows={rows} C={C}")


def test_finalize_variance_clamp_count_one_and_null_running_statistics():
    """pcrl_bn_finalize, derived (one ulp, as above) + exact where stated.
    `if (var < 0.0) var = 0.0` (line 75): channel 0 has s1 = 3000, s2 = one float32 step below 3e6 at count 3, so s2 / 3 - mu^2 = -1/12 in
    float64; rstd must be 1 / sqrt(eps) (without the clamp var + eps is negative and rstd NaN), the running variance takes 0.
    `count > 1.0 ? ... : var` (line 84): count = 1 with (s1, s2) = (1.5, 2.5): var = 0.25 and the running variance takes the BIASED value
    (the unbiased factor would be 1 / 0).
    running_mean / running_var null: the four coefficient vectors as before, nothing else written."""
    s1, s2, count = npc.clamp_partials()
    p = torch.tensor([[[float(s1), float(s2)], [3.0, 9.0]]], dtype=F32)          # channel 1: ordinary (mu = 1, var = 2)
    gamma, beta, rm0, rv0 = affine(2, seed=1)
    rm, rv = rm0.to(DEV), rv0.to(DEV)
    got = run_finalize(p.to(DEV), 1, 2, count, gamma.to(DEV), beta.to(DEV), rm, rv)
    check_finalize(got, rm, rv, p.double().sum(0), count, gamma, beta, rm0, rv0, "bn_finalize, clamped channel")
    within_one_ulp(got["rstd"][:1], torch.tensor([1.0 / math.sqrt(EPS32)], dtype=torch.float64), "rstd of the clamped channel")
    assert float(got["mean"][0]) == 1000.0
    p1 = torch.tensor([[[1.5, 2.5]]], dtype=F32)
    rm, rv = rm0[:1].to(DEV), rv0[:1].to(DEV)
    got = run_finalize(p1.to(DEV), 1, 1, 1.0, gamma[:1].to(DEV), beta[:1].to(DEV), rm, rv)
    check_finalize(got, rm, rv, p1.double().sum(0), 1.0, gamma[:1], beta[:1], rm0[:1], rv0[:1], "bn_finalize, count = 1")
    within_one_ulp(rv, (1.0 - MOM32) * rv0[:1].double() + MOM32 * 0.25, "running_var at count = 1 (biased)")
    partial, sums = stat_partials(300, 3, seed=9)
    gamma, beta, _, _ = affine(3, seed=2)
    got = run_finalize(partial, 300, 3, 1200, gamma.to(DEV), beta.to(DEV), None, None)
    check_finalize(got, None, None, sums, 1200, gamma, beta, None, None, "bn_finalize, no running statistics")


@pytest.mark.parametrize("rows,C,prepass", [(20000, 16, False), (20001, 16, True), (20001, 3, False)])
def test_ops_bn_finalize_column_sum_prepass(rows, C, prepass):
    """ops.bn_finalize (ops.py: `rows > 20000 and C % 2 == 0`), exact: from 20 001 statistics rows on an even C is first summed by the tiled
    column sums (pcrl_colsum over [rows][2 C] float32: coltile_rows(1, 20 001) = 32, so 626 tiles, and the finish kernel's unrolled loop runs)
    and finalized from ONE row; 20 000 rows and an odd C stay on
    the direct route.  The lattice partials sum exactly in float32 (20 001 x 48 units < 2^24), so both routes see the same (s1, s2) and
    must produce the same bits in all six outputs."""
    partial, sums = stat_partials(rows, C, seed=rows)
    gamma, beta, rm0, rv0 = affine(C, seed=3)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    rm_a, rv_a, rm_b, rv_b = rm0.to(DEV), rv0.to(DEV), rm0.to(DEV), rv0.to(DEV)
    direct = run_finalize(partial, rows, C, 4 * rows, gd, bd, rm_a, rv_a)
    with lib().count_calls("pcrl_colsum") as calls:
        mean, rstd, scale, shift = ops.bn_finalize(partial, rows, C, 4 * rows, gd, bd, rm_b, rv_b)
    assert calls.get("pcrl_colsum", 0) == (1 if prepass else 0)
    for a, b, what in ((mean, direct["mean"], "mean"), (rstd, direct["rstd"], "rstd"), (scale, direct["scale"], "scale"),
                       (shift, direct["shift"], "shift"), (rm_b, rm_a, "running_mean"), (rv_b, rv_a, "running_var")):
        eq(a, b, f"ops.bn_finalize rows={rows} C={C}: {what}", bits=True)
    check_finalize(direct, rm_a, rv_a, sums, 4 * rows, gamma, beta, rm0, rv0, f"bn_finalize rows={rows} C={C}")


# ----------------------------------------------------------------------------------------------------------------------------------------
# 2. apply forward and backward, register-cached path
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,C,M", npc.RC_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_apply_register_cached_through_the_grid_wrap(dt, C, M):
    """pcrl_bn_act_apply / pcrl_bn_act_bwd_apply, bn_apply_rc_kernel / bn_bwd_apply_rc_kernel, exact, ReLU and no activation.  rc_grid() caps
    the launch at 2048 blocks of nslots = 256 / (C / vec) rows: M = 2048 nslots + 2 nslots + a remainder that is no multiple of nslots, so
    every slot takes a second step of `r += stride` and some a third; every nslots of the kernel (1, 2, 4, 32, 128, 256).  Two small shapes
    stay below the cap."""
    co = npc.Coef(C, C, DEV)
    y, da = inputs(M, C, dt, seed=M % 1000, n=2)
    for act in (ACT_RELU, ACT_NONE):
        eq(k_apply(y, co, M, C, act, dt), npc.ref_apply(y, co, act, dt), f"bn_act_apply C={C} M={M} act={act}")
        got = k_bwd_apply("plain", da, None, None, 1, M, y, co, M, C, act, dt)
        eq(got, npc.ref_bwd_apply(da.float(), y, co, act, dt), f"bn_act_bwd_apply C={C} M={M} act={act}")


# ----------------------------------------------------------------------------------------------------------------------------------------
# 3. row term through the wrap
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", npc.GRAD_VARIANTS)
@pytest.mark.parametrize("dt,C,N,S", npc.ROW_WRAP_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_bwd_apply_row_term_through_the_grid_wrap(dt, C, N, S, variant):
    """pcrl_bn_act_bwd_apply_rowadd / _sum, exact restatement.  With C = 512 float32 (C = 1024 bf16) a block holds 2 rows and the stride is
    4096 rows, so the incremental sample walk (`n += dn; rem += drem; if (rem >= S) ...`, lines 212-231) does something:
      (9, 1000): dn = 4, drem = 96, `rem` wraps on some steps and not on others;   (2, 5000): dn = 0, the sample changes only through the wrap;
      (9, 1024): S divides the stride, drem = 0;   (5, 8) with one channel vector: below the cap, a block spans 32 samples.
    Gradient = da + row, row alone, da alone, da + da2 + row, da + da2.  The row term is g[n][c] * (float)(1.0 / S) in float32, added as
    (da + da2) + add.  g = i/8 with |i| <= 100 is NOT chosen to make that exact: at S = 1000 and 5000 the product is rounded and so is the
    sum, and the restatement makes the same two roundings in torch float32 -- a kernel that divided by S, kept 1/S in double, contracted
    the product into the sum or added in another order would differ in the last bit of many elements.  k1 is a power of two, so k1 * dz is
    exact, kB * y too, and (k1 dz + kB y) + kA has the two roundings the restatement makes (a contraction of either product into that sum
    changes nothing: both products are exact)."""
    M = N * S
    co = npc.Coef(C, C + 1, DEV)
    y, da, da2 = inputs(M, C, dt, seed=S % 1000)
    g = npc.row_term_general(N, C, 5, DEV)
    got = k_bwd_apply(variant, da, da2, g, N, S, y, co, M, C, ACT_RELU, dt)
    want = npc.ref_bwd_apply(ref_gin_of(variant, da, da2, g, S, 0, M, C), y, co, ACT_RELU, dt)
    eq(got, want, f"bn_act_bwd_apply {variant} C={C} N={N} S={S}")


# ----------------------------------------------------------------------------------------------------------------------------------------
# 4. generic kernels
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,C,M", npc.GENERIC_CASES + [npc.GENERIC_BIG], ids=lambda v: str(v).replace("torch.", ""))
def test_apply_generic_kernels(dt, C, M):
    """pcrl_bn_act_apply / pcrl_bn_act_bwd_apply, bn_apply_kernel / bn_bwd_apply_kernel, exact: a channel-vector count that does not divide
    256 (C = 12, 24, 96) and C = 1 (float32 only) take the generic kernels, which look the coefficients up per element from
    `c0 = (i * VEC) % C`.  The large shape has 4 194 606 vectors, 302 more than grid_for()'s 16 384 x 256, so a few threads take a second
    grid-stride step; the stride of 16 777 216 elements is 16 mod 24: c0 must be recomputed, not carried."""
    co = npc.Coef(C, C + 2, DEV)
    y, da = inputs(M, C, dt, seed=C, n=2)
    acts = (ACT_RELU,) if M > 100000 else (ACT_RELU, ACT_NONE)
    for act in acts:
        eq(k_apply(y, co, M, C, act, dt), npc.ref_apply(y, co, act, dt), f"generic bn_act_apply C={C} M={M} act={act}")
        got = k_bwd_apply("plain", da, None, None, 1, M, y, co, M, C, act, dt)
        eq(got, npc.ref_bwd_apply(da.float(), y, co, act, dt), f"generic bn_act_bwd_apply C={C} M={M} act={act}")


# ----------------------------------------------------------------------------------------------------------------------------------------
# 5. backward first stage
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,C,M,row", npc.REDUCE_CASES, ids=lambda v: str(v).replace("torch.", "").replace(" ", ""))
def test_bwd_reduce_tiles(dt, C, M, row):
    """pcrl_bn_act_bwd_reduce / _rowadd / _sum + pcrl_bn_bwd_finalize, exact.  bn_bwd_tile_rows() gives 32-row tiles below M = 65 536 and
    doubles up to 1024 at 2^20: one case per tile size, on both sides of 65 536 and of 2^20 (2^20 + 37 leaves a last tile of 37 rows: `rend`
    clipped; the rows behind the tensors hold poison).  The four-rows-in-flight loop (lines 301-321) runs tile / (4 nslots) times: zero,
    exactly once (bf16 C = 8: 256 slots, tile 1024), twice, four times.  With a row term: S a multiple of the tile (`ra_tile`: one sample per
    tile, unrolled loop taken) against S = 61 696 = 60 x 1024 + 256 and S = 32 < tile (a tile straddles samples: per-row lookup, unrolled
    loop skipped).  C = 1 float32: a "row" is four voxels, rows_total = M / 4.
    Every first-stage partial is a float32 sum of lattice terms below 2^24 units (test_norm_pool_cases_cpu.py), hence exact in any order: the
    partial rows summed in float64 equal the float64 reference (assert_rows_exact), dbeta / dgamma are that sum rounded once."""
    N, S = row if row else (1, M)
    co = npc.Coef(C, C + 3, DEV)
    y, da, da2 = (padded(t) for t in inputs(M, C, dt, seed=M % 997))
    g = npc.row_term(N, C, S, 6, DEV) if row else None
    if row:
        todo = [("rowadd: da + row", ACT_RELU), ("sum: da + da2 + row", ACT_RELU), ("rowadd: row only", ACT_NONE)]
    elif C == 1:
        todo = [("plain", ACT_RELU), ("plain", ACT_NONE)]
    else:
        todo = [("plain", ACT_RELU), ("plain", ACT_NONE), ("sum: da + da2", ACT_RELU)]
    for variant, act in todo:
        partial, rows = k_reduce(variant, da, da2, g, N, S, y, co, M, C, act, dt)
        s1 = torch.zeros(C, dtype=torch.float64, device=DEV)
        s2 = torch.zeros(C, dtype=torch.float64, device=DEV)
        for r0, r1 in chunks(M):
            a, b = npc.ref_reduce(ref_gin_of(variant, da, da2, g, S, r0, r1, C), y[r0:r1], co, act)
            s1, s2 = s1 + a, s2 + b
        what = f"bn_act_bwd_reduce {variant} act={act} C={C} M={M}"
        assert_rows_exact(partial[:, :, 0], s1.cpu(), what + ": sum dz")
        assert_rows_exact(partial[:, :, 1], s2.cpu(), what + ": sum dz xhat")
        check_bwd_finalize(partial, rows, C, M, co, s1, s2, what)


# ----------------------------------------------------------------------------------------------------------------------------------------
# 6. column sums and global average pool
# ----------------------------------------------------------------------------------------------------------------------------------------
def ws_of(nbytes):
    """a workspace of nbytes, poison before the launch and followed by 8 KiB of poison: a partial read past it moves the result"""
    return torch.full((int(nbytes) // 4 + 2048,), POISON, dtype=F32, device=DEV)


@pytest.mark.parametrize("dt,C,N,S", npc.COL_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_column_sums_and_global_average_pool(dt, C, N, S):
    """pcrl_colsum (N = 1), pcrl_gap_fwd, pcrl_bn_act_apply_gap, exact.  coltile_rows() halves the 1024-row tile down to 32 while the grid has
    fewer than 512 blocks: S = tile - 1, tile, tile + 1 for tile 32 (N = 1, 3) and tile 1024 (N = 512).  coltile_finish_kernel sums 8 tile
    slices per channel, four tiles in flight while `t + 24 < tiles`: 1, 7, 8, 9 tiles are around one tile per slice, 24 / 25 around the first
    unrolled pass of slice 0, 32 / 33 / 57 leave tails behind it, 4096 is a full-resolution tensor.  C = 8 and 16 leave channels of the
    32-channel block without work (`c < C`), C = 1024 is 32 blocks.  Tile sums are float32 sums of at most 1024 lattice values, the finish
    is float64: colsum equals the float64 sum rounded once, the average is (float)(sum * (1.0 / S)) restated in float64 exactly so.  For
    apply + gap the stored activation must be bit-equal to pcrl_bn_act_apply's and to the restatement, and g is the average of the ROUNDED
    activation.  The rows behind the input hold poison."""
    M = N * S
    co = npc.Coef(C, C + 4, DEV)
    v = padded(inputs(M, C, dt, seed=S % 991, n=1)[0])
    tiles = npc.coltile_tiles(N, S)
    sums = torch.stack([v[n * S:(n + 1) * S].double().sum(0) for n in range(N)])
    nb = lib().call("pcrl_gap_ws_bytes", N, S, C)
    assert nb == N * tiles * C * 4
    if N == 1:
        assert lib().call("pcrl_colsum_ws_bytes", M, C) == nb
        out = outbuf(C, F32)
        call("pcrl_colsum", v, out, ws_of(nb), nb, M, C, dtype_code(dt))
        tail_kept(out, C, "colsum")
        assert_bit_equal(out[:C], sums[0].cpu(), F32, f"colsum C={C} M={M} ({tiles} tiles)")
    out = outbuf(N * C, F32)
    call("pcrl_gap_fwd", v, out, ws_of(nb), nb, N, S, C, dtype_code(dt))
    tail_kept(out, N * C, "gap_fwd")
    eq(out[:N * C], (sums * (1.0 / S)).float().reshape(-1), f"gap_fwd C={C} N={N} S={S} ({tiles} tiles)")
    a, gout = outbuf(M * C, dt), outbuf(N * C, F32)
    call("pcrl_bn_act_apply_gap", v, a, gout, co.scale, co.shift, ws_of(nb), nb, N, S, C, ACT_RELU, dtype_code(dt))
    tail_kept(a, M * C, "bn_act_apply_gap: a")
    tail_kept(gout, N * C, "bn_act_apply_gap: g")
    want = npc.ref_apply(v, co, ACT_RELU, dt)
    eq(a[:M * C], want, f"bn_act_apply_gap a C={C} N={N} S={S}")
    eq(a[:M * C], k_apply(v, co, M, C, ACT_RELU, dt), "bn_act_apply_gap a against bn_act_apply", bits=True)
    asum = torch.stack([want[n * S:(n + 1) * S].double().sum(0) for n in range(N)])
    eq(gout[:N * C], (asum * (1.0 / S)).float().reshape(-1), f"bn_act_apply_gap g C={C} N={N} S={S}")


@pytest.mark.parametrize("dt,C,N,S", [(F32, 8, 3, 37), (BF16, 16, 2, 1000), npc.GAP_BWD_BIG], ids=lambda v: str(v).replace("torch.", ""))
def test_gap_backward(dt, C, N, S):
    """pcrl_gap_bwd with and without add_src, exact: da = round(add + dg[n][c] * (float)(1.0 / S)).  dg is zero or a signed power of two, so
    the product with the (inexact) float32 1/S is exact and the sum is rounded once, whether or not the compiler contracts the two.  (3, 349 999) in bf16 C = 32 is 4 199 988 vectors, past grid_for()'s
    4 194 304: the sample index `(i / nvec) / S` must hold across the second grid-stride step."""
    M = N * S
    add = inputs(M, C, dt, seed=3, n=1)[0]
    dg = npc.pow2_lat((N, C), 4, DEV)
    term = (dg * npc.inv_s32(S).to(DEV)).repeat_interleave(S, dim=0)
    for src, want in ((None, term.to(dt)), (add, (add.float() + term).to(dt))):
        out = outbuf(M * C, dt)
        call("pcrl_gap_bwd", dg, src, out, N, S, C, dtype_code(dt))
        tail_kept(out, M * C, "gap_bwd")
        eq(out[:M * C], want, f"gap_bwd C={C} N={N} S={S} add_src={'yes' if src is not None else 'no'}")


@pytest.mark.parametrize("dt", DTYPES)
def test_weighted_column_sum_through_the_pointwise_weight_gradient(dt):
    """pcrl_conv3d_to1_wgrad with taps = 1 (coltile_sum_kernel<T, true>), exact: dw[c] = sum_m x[m][c] dy[m] on a (1, 1, 3, 11) volume = 33
    rows: two 32-row tiles, the second of ONE row; x = i/4, dy = j/4, products in units of 1/16.  db = sum dy in float64, rounded once."""
    N, D, H, W, C = 1, 1, 3, 11, 8
    M = N * D * H * W
    x = padded(inputs(M, C, dt, seed=8, n=1)[0])
    dy = padded(npc.lat((M,), 8, 4, F32, 9, DEV))
    nb = lib().call("pcrl_conv3d_to1_wgrad_ws_bytes", N, D, H, W, C, 1)
    dw, db = outbuf(C, F32), outbuf(1, F32)
    call("pcrl_conv3d_to1_wgrad", x, dy, dw, db, ws_of(nb), nb, N, D, H, W, C, 1, dtype_code(dt))
    tail_kept(dw, C, "conv3d_to1_wgrad: dw")
    assert_bit_equal(dw[:C], (x.double() * dy.double().unsqueeze(1)).sum(0).cpu(), F32, "weighted column sum")
    assert_bit_equal(db[:1], dy.double().sum().view(1).cpu(), F32, "bias gradient")


# ----------------------------------------------------------------------------------------------------------------------------------------
# 7. MaxPool and the pool fusions
# ----------------------------------------------------------------------------------------------------------------------------------------
def k_maxpool(x, gy, dims, C, dt):
    N, D, H, W = dims
    Mp = npc.pool_mp(dims)
    p, dx = outbuf(Mp * C, dt), outbuf(8 * Mp * C, dt)
    call("pcrl_maxpool3d_2_fwd", x, p, N, D, H, W, C, dtype_code(dt))
    call("pcrl_maxpool3d_2_bwd", x, gy, dx, N, D, H, W, C, dtype_code(dt))
    tail_kept(p, Mp * C, "maxpool fwd")
    tail_kept(dx, 8 * Mp * C, "maxpool bwd")
    return p[:Mp * C].view(Mp, C), dx[:8 * Mp * C].view(N, D, H, W, C)


def k_pool_fused(y, gp, co, dims, C, act, dt, want_a=True):
    N, D, H, W = dims
    Mp = npc.pool_mp(dims)
    a, p, dy = outbuf(8 * Mp * C, dt), outbuf(Mp * C, dt), outbuf(8 * Mp * C, dt)
    call("pcrl_bn_act_apply_pool", y, a if want_a else None, p, co.scale, co.shift, N, D, H, W, C, act, dtype_code(dt))
    rows = lib().call("pcrl_bn_act_bwd_pool_partial_rows", N, D, H, W)
    assert rows == -(-Mp // npc.bn_pool_tile(Mp))
    part = outbuf(rows * C * 2, F32)
    call("pcrl_bn_act_bwd_reduce_pool", gp, y, co.scale, co.shift, co.mean, co.rstd, part, N, D, H, W, C, act, dtype_code(dt))
    call("pcrl_bn_act_bwd_apply_pool", gp, y, dy, co.scale, co.shift, co.k1, co.kB, co.kA, N, D, H, W, C, act, dtype_code(dt))
    for buf, n, what in ((a, 8 * Mp * C, "a"), (p, Mp * C, "p"), (dy, 8 * Mp * C, "dy"), (part, rows * C * 2, "partial")):
        tail_kept(buf, n, f"pool fusion: {what}")
    if not want_a:
        torch.cuda.synchronize()
        assert bool((a == SENT).all()), "bn_act_apply_pool with a null activation pointer wrote an activation"
    return a[:8 * Mp * C].view(N, D, H, W, C), p[:Mp * C].view(Mp, C), part[:rows * C * 2].view(rows, C, 2), dy[:8 * Mp * C].view(N, D, H, W, C)


def rows_exact(rows, ref64, what, nan_ok):
    """assert_rows_exact; with nan_ok a channel whose reference sum is NaN (a NaN or inf met 0, or infs of both signs) must be NaN too"""
    if not nan_ok:
        return assert_rows_exact(rows, ref64, what)
    torch.cuda.synchronize()
    got = rows.detach().double().cpu().sum(0)
    bad = ((got != ref64) & ~(got.isnan() & ref64.isnan())).nonzero().flatten().tolist()
    assert not bad, f"{what}: {len(bad)} of {got.numel()} channels differ; first {[(c, float(got[c]), float(ref64[c])) for c in bad[:6]]}"


def check_pool_fused(y5, gp, co, dims, C, act, dt, what, nan_ok=False):
    N, D, H, W = dims
    a, p, part, dy = k_pool_fused(y5, gp, co, dims, C, act, dt)
    aw, pw, s1, s2, dyw = npc.ref_pool_fused(npc.windows(y5), gp, co, act, dt)
    eq(a, npc.unwindows(aw, N, D, H, W).contiguous(), f"{what}: bn_act_apply_pool a")
    eq(p, pw, f"{what}: bn_act_apply_pool p")
    eq(dy, npc.unwindows(dyw, N, D, H, W).contiguous(), f"{what}: bn_act_bwd_apply_pool dy")
    rows_exact(part[:, :, 0], s1.cpu(), f"{what}: bn_act_bwd_reduce_pool sum dz", nan_ok)
    rows_exact(part[:, :, 1], s2.cpu(), f"{what}: bn_act_bwd_reduce_pool sum dz xhat", nan_ok)
    _, p2, _, _ = k_pool_fused(y5, gp, co, dims, C, act, dt, want_a=False)
    eq(p2, pw, f"{what}: bn_act_apply_pool p (a null)")


@pytest.mark.parametrize("dt", DTYPES)
def test_maxpool_enumerated_windows_against_aten(dt):
    """pcrl_maxpool3d_2_fwd / _bwd, exact (bits, zeros included: the operation only moves values) against F.max_pool3d float64 autograd on the
    CPU, on a tensor whose windows enumerate: each of the 8 positions as the single maximum, each of the 28 pairs as a tie (the FIRST in
    scan order takes the gradient: strict `>`, line 558), an all-equal window, a descending and an ascending run, an all -inf window
    (position 0 keeps the gradient), a NaN at each position and two NaNs in one window (the last NaN wins, as in aten), (+0, -0) in both
    orders among negatives.  Channel c sees the windows rotated by c, so every window meets every lane of a vector."""
    C = npc.vec(dt)
    w = torch.cat([npc.enumerated_windows(), npc.special_windows()])
    Wn = w.shape[0]
    wc = torch.stack([w.roll(c, 0) for c in range(C)], dim=2)                     # [Wn, 8, C]
    x5 = npc.windows_to_volume(wc).contiguous()                                   # [1, 2, 2, 2 Wn, C] float64
    assert torch.equal(x5.to(dt).double().nan_to_num(nan=7.0), x5.nan_to_num(nan=7.0))
    x = x5.permute(0, 4, 1, 2, 3).clone().requires_grad_(True)
    out = F.max_pool3d(x, 2)
    gy = (torch.arange(1, Wn * C + 1, dtype=torch.float64).view(Wn, C) / 4).to(dt).double()
    out.backward(gy.t().reshape(1, C, 1, 1, Wn))
    ref_p = out.detach().permute(0, 2, 3, 4, 1).reshape(Wn, C).to(dt).to(DEV)
    ref_dx = x.grad.permute(0, 2, 3, 4, 1).contiguous().to(dt).to(DEV)
    p, dx = k_maxpool(x5.to(dt).to(DEV), gy.to(dt).to(DEV), (1, 2, 2, 2 * Wn), C, dt)
    eq(p, ref_p, f"maxpool fwd, enumerated windows {dt}", bits=True)
    eq(dx, ref_dx, f"maxpool bwd, enumerated windows {dt}", bits=True)
    # the restatement used by the large cases gives the same
    arg = npc.pool_arg(wc)
    eq(dx, npc.unwindows(npc.ref_maxpool_bwd(arg, gy), 1, 2, 2, 2 * Wn).contiguous().to(dt).to(DEV), "maxpool bwd against the restatement", bits=True)


def enumerated_coef(C):
    """channel c % 4 == 0: (scale, shift) = (1, 0): a = y;  1: (1, 100): in bf16 every y = 1 + r/128 rounds to a = 101 -- values that differ
    before the rounding tie after it;  2: (-1, 0): the order is reversed (ReLU: all zero, all tied);  3: the lattice coefficients"""
    co = npc.Coef(C, 11, DEV)
    for c in range(C):
        if c % 4 == 0:
            co.scale[c], co.shift[c] = 1.0, 0.0
        elif c % 4 == 1:
            co.scale[c], co.shift[c] = 1.0, 100.0
        elif c % 4 == 2:
            co.scale[c], co.shift[c] = -1.0, 0.0
    return co


@pytest.mark.parametrize("act", [ACT_RELU, ACT_NONE])
@pytest.mark.parametrize("dt", DTYPES)
def test_pool_fusions_enumerated_windows(dt, act):
    """pcrl_bn_act_apply_pool (a stored and a null), pcrl_bn_act_bwd_reduce_pool, pcrl_bn_act_bwd_apply_pool, exact against the restatement
    (not against the three-kernel route) on the enumerated windows: y = 1 + r/128 for the ranks r of test_maxpool_enumerated_windows (single
    maxima, the 28 ties, runs), rotated over the channels.  pool_argmax decides on the activation ROUNDED to the storage type (line 603):
    with (scale, shift) = (1, 100), z = 101 + r/128 is exact in float32 and in bf16 every element of a window rounds to 101, so position 0
    takes the gradient -- and `ybest`, so the statistics and dy -- where an argmax on z would take the largest rank.  y - mean, the products
    with rstd, kB and k1 stay exact (units of 2^-10, values below 2^7)."""
    C = 2 * npc.vec(dt)
    r = npc.enumerated_windows()
    Wn = r.shape[0]
    yw = torch.stack([1 + r.roll(c, 0) / 128 for c in range(C)], dim=2).to(dt)
    assert torch.equal(yw.double(), torch.stack([1 + r.roll(c, 0) / 128 for c in range(C)], dim=2))
    dims = (1, 2, 2, 2 * Wn)
    y5 = npc.windows_to_volume(yw).contiguous().to(DEV)
    gp = npc.lat((Wn, C), 8, 4, dt, 12, DEV)
    co = enumerated_coef(C)
    if dt == BF16 and act == ACT_NONE:
        aw = npc.ref_apply(yw.to(DEV), co, act, dt)
        assert bool((aw[:, :, 1] == 101).all()) and bool((npc.pool_arg(aw)[:, 1] == 0).all())
    check_pool_fused(y5, gp, co, dims, C, act, dt, f"enumerated windows {dt} act={act}")


@pytest.mark.parametrize("act", [ACT_RELU, ACT_NONE])
@pytest.mark.parametrize("dt", DTYPES)
def test_pool_fusions_special_values(dt, act):
    """pcrl_bn_act_apply_pool (a stored and a null), pcrl_bn_act_bwd_reduce_pool, pcrl_bn_act_bwd_apply_pool on the special windows -- all -inf,
    a NaN at each position, two NaNs, (+0, -0) in both orders, -inf with one finite value -- rotated over the channels, with the lattice
    coefficients (scales of both signs), exact against the restatement; NaN compares equal to NaN, inf to inf of the same sign.
    Without activation a NaN pre-activation is a NaN activation and `a != a` (line 604) hands the window to the LAST NaN: dy is NaN exactly
    at the NaN inputs (kB * NaN, also for kB = 0) and NO finite position carries k1 * dp -- a kernel that ignored the NaN would route it
    to the largest finite element; the statistics of such a channel are NaN.  With ReLU a NaN pre-activation becomes 0 (`z > 0.f ? z : 0.f`) and ties with the other zeros.  A window whose activations are all
    -inf (no activation, -inf inputs under a positive scale) never satisfies `a > m` from m = -inf: position 0 keeps the gradient and the
    statistics take zb = ybest = 0, the start values of pool_argmax (the three-kernel route would put y = -inf into sum dz xhat there;
    both are statistics of a tensor that is already lost).  Sums that meet infs of both signs or 0 * inf are NaN in any order."""
    C = 2 * npc.vec(dt)
    w = npc.special_windows()
    Wn = w.shape[0]
    yw = torch.stack([w.roll(c, 0) for c in range(C)], dim=2).to(dt)
    dims = (1, 2, 2, 2 * Wn)
    y5 = npc.windows_to_volume(yw).contiguous().to(DEV)
    gp = npc.lat((Wn, C), 8, 4, dt, 14, DEV)
    co = npc.Coef(C, 12, DEV)
    co.scale[0], co.shift[0], co.kB[0] = 1.0, 0.0, 0.5        # channel 0 sees the windows unrotated, through the identity
    assert bool((co.scale < 0).any()) and bool((co.scale > 0).any())
    check_pool_fused(y5, gp, co, dims, C, act, dt, f"special windows {dt} act={act}", nan_ok=True)
    aw, pw, s1, s2, dyw = npc.ref_pool_fused(npc.windows(y5), gp, co, act, dt)
    if act == ACT_NONE:                                       # what the restatement says about channel 0, spelled out
        assert bool(pw[0, 0].isinf()) and bool(pw[1:10, 0].isnan().all())
        for k in range(8):                                    # window 1 + k has its NaN at position k: dy = k1 dp + kB NaN there, kB NaN elsewhere: NaN at k only
            assert dyw[1 + k, :, 0].isnan().tolist() == [t == k for t in range(8)]
        assert dyw[9, :, 0].isnan().tolist() == [True, False, False, True, False, False, False, False]
        assert bool(s2[0].isnan()) and not bool(s1[0].isnan())
    else:
        assert not bool(aw.isnan().any())


@pytest.mark.parametrize("dt,C,dims", npc.POOL_CASES, ids=lambda v: str(v).replace("torch.", "").replace(" ", ""))
def test_pool_fusions_tiles(dt, C, dims):
    """The three pool-fused kernels and pcrl_maxpool3d_2_fwd / _bwd on lattice tensors (17 values: most windows hold ties), ReLU, exact.
    bn_pool_tile() gives 4 pooled voxels per partial below Mp = 8192 and doubles up to 128 at 131 072: Mp = 8190 / 8192 and 16 380 / 16 384
    on both sides of the first two steps, one case per tile size, Mp = 135 135 with a last tile of 95 (`pend` clipped), and three samples in
    one block."""
    N, D, H, W = dims
    Mp = npc.pool_mp(dims)
    co = npc.Coef(C, C + 5, DEV)
    y5 = npc.lat((N, D, H, W, C), 8, 4, dt, Mp % 983, DEV)
    gp = npc.lat((Mp, C), 8, 4, dt, 13, DEV)
    check_pool_fused(y5, gp, co, dims, C, ACT_RELU, dt, f"pool fusions {dims} C={C}")
    p, dx = k_maxpool(y5, gp, dims, C, dt)
    yw = npc.windows(y5)
    arg = npc.pool_arg(yw)
    eq(p, npc.take(yw, arg), f"maxpool fwd {dims} C={C}", bits=True)
    eq(dx, npc.unwindows(npc.ref_maxpool_bwd(arg, gp), N, D, H, W).contiguous(), f"maxpool bwd {dims} C={C}", bits=True)


# ----------------------------------------------------------------------------------------------------------------------------------------
# 8. non-temporal twins
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nt():
    """y, da, coefficients and row term of the first size with pcrl_streaming() true (bf16 C = 32, M = 3 145 728: 201 326 592 bytes per
    tensor), built once for the tests of this section, never modified, released when the module is done"""
    dt, C, N, S = npc.NT_CASE
    y, da = inputs(N * S, C, dt, seed=21, n=2)
    yield y, da, npc.Coef(C, 22, DEV), npc.row_term(N, C, S, 23, DEV)
    del y, da


def test_nt_apply_and_backward_apply(nt):
    """bn_apply_rc_kernel_body<NT = true> and bn_bwd_apply_rc_kernel_body<NT = true> (plain and with the row term), exact against the device
    float64 restatement in chunks.  A second call on the first M - 1 rows is one row below the threshold and takes the plain path: its
    output must be bit-equal to the first M - 1 rows of the large call."""
    dt, C, N, S = npc.NT_CASE
    M = N * S
    y, da, co, g = nt
    a = k_apply(y, co, M, C, ACT_RELU, dt)
    dy = k_bwd_apply("plain", da, None, None, 1, M, y, co, M, C, ACT_RELU, dt)
    dyr = k_bwd_apply("rowadd: da + row", da, None, g, N, S, y, co, M, C, ACT_RELU, dt)
    for r0, r1 in chunks(M):
        eq(a[r0:r1], npc.ref_apply(y[r0:r1], co, ACT_RELU, dt), f"NT bn_act_apply rows {r0}..{r1}")
        eq(dy[r0:r1], npc.ref_bwd_apply(da[r0:r1].float(), y[r0:r1], co, ACT_RELU, dt), f"NT bn_act_bwd_apply rows {r0}..{r1}")
        gin = npc.ref_gin(r1 - r0, C, DEV, da[r0:r1], None, g, S, r0)
        eq(dyr[r0:r1], npc.ref_bwd_apply(gin, y[r0:r1], co, ACT_RELU, dt), f"NT bn_act_bwd_apply_rowadd rows {r0}..{r1}")
    eq(k_apply(y, co, M - 1, C, ACT_RELU, dt), a[:M - 1], "bn_act_apply: plain path on M - 1 rows against the NT call", bits=True)
    eq(k_bwd_apply("plain", da, None, None, 1, M - 1, y, co, M - 1, C, ACT_RELU, dt), dy[:M - 1], "bn_act_bwd_apply: plain path on M - 1 rows", bits=True)


def test_nt_backward_reduce(nt):
    """bn_bwd_reduce_kernel_body<NT = true>, plain and with the row term (S = 2^20: ra_tile), exact: partial rows and dbeta / dgamma.  The
    call on M - 1 rows (plain path, same tile size) must give the same partial rows but the last."""
    dt, C, N, S = npc.NT_CASE
    M = N * S
    y, da, co, g = nt
    for variant in ("plain", "rowadd: da + row"):
        partial, rows = k_reduce(variant, da, None, g, N, S, y, co, M, C, ACT_RELU, dt)
        s1 = torch.zeros(C, dtype=torch.float64, device=DEV)
        s2 = torch.zeros(C, dtype=torch.float64, device=DEV)
        for r0, r1 in chunks(M):
            a, b = npc.ref_reduce(ref_gin_of(variant, da, None, g, S, r0, r1, C), y[r0:r1], co, ACT_RELU)
            s1, s2 = s1 + a, s2 + b
        assert_rows_exact(partial[:, :, 0], s1.cpu(), f"NT bn_act_bwd_reduce {variant}: sum dz")
        assert_rows_exact(partial[:, :, 1], s2.cpu(), f"NT bn_act_bwd_reduce {variant}: sum dz xhat")
        check_bwd_finalize(partial, rows, C, M, co, s1, s2, f"NT bn_act_bwd_reduce {variant}")
        if variant == "plain":
            small, rows_s = k_reduce("plain", da, None, None, 1, M - 1, y, co, M - 1, C, ACT_RELU, dt)
            assert rows_s == rows
            eq(small[:rows - 1], partial[:rows - 1], "bn_act_bwd_reduce: plain path on M - 1 rows against the NT call", bits=True)


def test_nt_apply_gap_and_gap_backward(nt):
    """bn_apply_gap_body<NT = true> and gap_bwd_kernel<T, NT = true> at N = 3, S = 2^20, exact: the activation against the restatement and
    bit-equal to pcrl_bn_act_apply's, g = (float)(sum * (1.0 / S)); gap_bwd with add_src (also past grid_for()'s cap: 12 582 912 vectors)."""
    dt, C, N, S = npc.NT_CASE
    M = N * S
    y, da, co, g = nt
    nb = lib().call("pcrl_gap_ws_bytes", N, S, C)
    a, gout = outbuf(M * C, dt), outbuf(N * C, F32)
    call("pcrl_bn_act_apply_gap", y, a, gout, co.scale, co.shift, ws_of(nb), nb, N, S, C, ACT_RELU, dtype_code(dt))
    tail_kept(a, M * C, "NT bn_act_apply_gap")
    asum = torch.zeros(N, C, dtype=torch.float64, device=DEV)
    av = a[:M * C].view(M, C)
    for r0, r1 in chunks(M):
        want = npc.ref_apply(y[r0:r1], co, ACT_RELU, dt)
        eq(av[r0:r1], want, f"NT bn_act_apply_gap a rows {r0}..{r1}")
        asum[r0 // S] += want.double().sum(0)
    eq(gout[:N * C], (asum * (1.0 / S)).float().reshape(-1), "NT bn_act_apply_gap g")
    dg = npc.lat((N, C), 64, 1, F32, 24, DEV) * 1024.0
    out = outbuf(M * C, dt)
    call("pcrl_gap_bwd", dg, da, out, N, S, C, dtype_code(dt))
    tail_kept(out, M * C, "NT gap_bwd")
    term = dg * npc.inv_s32(S).to(DEV)
    ov = out[:M * C].view(M, C)
    for r0, r1 in chunks(M):
        eq(ov[r0:r1], (da[r0:r1].float() + term[r0 // S]).to(dt), f"NT gap_bwd rows {r0}..{r1}")


def test_nt_pool_kernels_past_the_grid_stride_cap():
    """maxpool_fwd / maxpool_bwd_kernel<T, NT = true> and the NT bodies of the three pool-fused kernels on (1, 128, 256, 258) x 32 bf16:
    541 065 216 bytes (non-temporal) and 4 227 072 work items, 32 768 past grid_for()'s 16 384 x 256, so threads take a second grid-stride
    step.  Exact against the device restatement, in chunks of 8 input planes."""
    dt, C, dims = npc.POOL_BIG
    N, D, H, W = dims
    Mp = npc.pool_mp(dims)
    co = npc.Coef(C, 31, DEV)
    y5 = npc.lat((N, D, H, W, C), 8, 4, dt, 32, DEV)
    gp = npc.lat((Mp, C), 8, 4, dt, 33, DEV)
    code = dtype_code(dt)
    per = (H // 2) * (W // 2)                 # pooled voxels per pooled plane
    rows = lib().call("pcrl_bn_act_bwd_pool_partial_rows", N, D, H, W)
    assert rows == -(-Mp // 128)
    p, pf, part = outbuf(Mp * C, dt), outbuf(Mp * C, dt), outbuf(rows * C * 2, F32)
    dx, a, dy = outbuf(8 * Mp * C, dt), outbuf(8 * Mp * C, dt), outbuf(8 * Mp * C, dt)
    call("pcrl_maxpool3d_2_fwd", y5, p, N, D, H, W, C, code)
    call("pcrl_maxpool3d_2_bwd", y5, gp, dx, N, D, H, W, C, code)
    call("pcrl_bn_act_apply_pool", y5, a, pf, co.scale, co.shift, N, D, H, W, C, ACT_RELU, code)
    call("pcrl_bn_act_bwd_reduce_pool", gp, y5, co.scale, co.shift, co.mean, co.rstd, part, N, D, H, W, C, ACT_RELU, code)
    call("pcrl_bn_act_bwd_apply_pool", gp, y5, dy, co.scale, co.shift, co.k1, co.kB, co.kA, N, D, H, W, C, ACT_RELU, code)
    for buf, n, what in ((p, Mp * C, "maxpool fwd"), (pf, Mp * C, "apply_pool p"), (part, rows * C * 2, "reduce_pool"), (dx, 8 * Mp * C, "maxpool bwd"),
                         (a, 8 * Mp * C, "apply_pool a"), (dy, 8 * Mp * C, "bwd_apply_pool")):
        tail_kept(buf, n, "NT " + what)

    def full(buf):
        return buf[:8 * Mp * C].view(N, D, H, W, C)

    s1 = torch.zeros(C, dtype=torch.float64, device=DEV)
    s2 = torch.zeros(C, dtype=torch.float64, device=DEV)
    step = 4
    for d0 in range(0, D // 2, step):
        d1 = min(d0 + step, D // 2)
        sl, pl, Dc = slice(d0 * per, d1 * per), slice(2 * d0, 2 * d1), 2 * (d1 - d0)
        yw, gs = npc.windows(y5[:, pl]), gp[sl]
        arg = npc.pool_arg(yw)
        eq(p[:Mp * C].view(Mp, C)[sl], npc.take(yw, arg), f"NT maxpool fwd planes {d0}..{d1}", bits=True)
        eq(full(dx)[:, pl], npc.unwindows(npc.ref_maxpool_bwd(arg, gs), N, Dc, H, W), f"NT maxpool bwd planes {d0}..{d1}", bits=True)
        aw, pw, a1, a2, dyw = npc.ref_pool_fused(yw, gs, co, ACT_RELU, dt)
        eq(full(a)[:, pl], npc.unwindows(aw, N, Dc, H, W), f"NT bn_act_apply_pool a planes {d0}..{d1}")
        eq(pf[:Mp * C].view(Mp, C)[sl], pw, f"NT bn_act_apply_pool p planes {d0}..{d1}")
        eq(full(dy)[:, pl], npc.unwindows(dyw, N, Dc, H, W), f"NT bn_act_bwd_apply_pool dy planes {d0}..{d1}")
        s1, s2 = s1 + a1, s2 + a2
    pv = part[:rows * C * 2].view(rows, C, 2)
    assert_rows_exact(pv[:, :, 0], s1.cpu(), "NT bn_act_bwd_reduce_pool sum dz")
    assert_rows_exact(pv[:, :, 1], s2.cpu(), "NT bn_act_bwd_reduce_pool sum dz xhat")


# ----------------------------------------------------------------------------------------------------------------------------------------
# 9. ELU, SiLU, sigmoid
# ----------------------------------------------------------------------------------------------------------------------------------------
def act_torch(z, act):
    return {ACT_ELU: F.elu, ACT_SILU: F.silu, ACT_SIGMOID: torch.sigmoid}[act](z)


def check_project(got, ref, dt, what, rounded=True):
    """`check` of tests/test_ops_gpu.py: max|got - ref| <= (1e-2 for a bf16-rounded output, else 2e-5) x max|ref|"""
    torch.cuda.synchronize()
    got, ref = got.detach().double().cpu(), ref.detach().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = max(ref.abs().max().item(), 1e-6)
    tol = (1e-2 if (dt == BF16 and rounded) else 2e-5) * scale
    err = (got - ref).abs().max().item()
    print(f"  {what} [{dt}]: max|d|={err:.3e} bound={tol:.3e}")
    assert err <= tol, f"{what} [{dt}]: max|d|={err:.3e} > {tol:.3e} (ref max {scale:.3e})"


ACT_CASES = [(F32, 32, 777), (BF16, 32, 777), (F32, 1, 1000), (F32, 24, 777)]


@pytest.mark.parametrize("act", [ACT_ELU, ACT_SILU, ACT_SIGMOID], ids=["elu", "silu", "sigmoid"])
@pytest.mark.parametrize("dt,C,M", ACT_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_elu_silu_sigmoid_forward_and_backward(dt, C, M, act):
    """pcrl_bn_act_apply, pcrl_bn_act_bwd_reduce + pcrl_bn_bwd_finalize, pcrl_bn_act_bwd_apply with ELU / SiLU / sigmoid against float64
    torch autograd of act(batch_norm(y)) on the dtype-rounded y and da; project bound (2e-5 x max|ref|; 1e-2 for the bf16-rounded a and dy).
    C = 32 takes the register-cached kernels, C = 1 and C = 24 (float32) the generic ones; C = 24 has no first stage (six channel vectors do
    not divide 256), so there only the two apply kernels run.  The coefficients the kernels take are the float32 roundings of the float64
    statistics (k1, kB, kA from the reference's own dgamma, dbeta where the first stage is not available); uniform(-1, 1) inputs over
    several hundred rows are well conditioned, no yardstick is needed."""
    g = torch.Generator().manual_seed(100 * act + C)
    y = ((torch.rand(M, C, generator=g, dtype=torch.float64) * 2 - 1) * 1.5 + 0.25).to(dt).double().requires_grad_(True)
    da = (torch.rand(M, C, generator=g, dtype=torch.float64) * 2 - 1).to(dt).double()
    gamma = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5).float().double().requires_grad_(True)
    beta = (torch.rand(C, generator=g, dtype=torch.float64) - 0.5).float().double().requires_grad_(True)
    a_ref = act_torch(F.batch_norm(y, None, None, gamma, beta, training=True, eps=ops.BN_EPS), act)
    a_ref.backward(da)
    yd = y.detach()
    mean = yd.mean(0)
    rstd = 1.0 / torch.sqrt(yd.var(0, unbiased=False) + ops.BN_EPS)
    co = npc.Coef(C, 1, DEV)
    gm, bt = gamma.detach(), beta.detach()
    co.gamma, co.mean, co.rstd = gm.float().to(DEV), mean.float().to(DEV), rstd.float().to(DEV)
    co.scale, co.shift = (gm * rstd).float().to(DEV), (bt - mean * gm * rstd).float().to(DEV)
    ydev, dadev = yd.to(dt).to(DEV), da.to(dt).to(DEV)
    check_project(k_apply(ydev, co, M, C, act, dt), a_ref, dt, f"bn_act_apply act={act} C={C}")
    f = npc.bwd_finalize64(beta.grad, gamma.grad, float(M), gm, mean, rstd)
    if C != 24:
        partial, rows = k_reduce("plain", dadev, None, None, 1, M, ydev, co, M, C, act, dt)
        out = torch.empty(5 * C, dtype=F32, device=DEV)
        o = [out[i * C:(i + 1) * C] for i in range(5)]
        call("pcrl_bn_bwd_finalize", partial, rows, C, float(M), co.gamma, co.mean, co.rstd, *o)
        check_project(o[0], gamma.grad, dt, f"dgamma act={act} C={C}", rounded=False)
        check_project(o[1], beta.grad, dt, f"dbeta act={act} C={C}", rounded=False)
        co.k1, co.kB, co.kA = o[2], o[3], o[4]
    else:
        co.k1, co.kB, co.kA = (f[k].float().to(DEV) for k in ("k1", "kB", "kA"))
    dy = k_bwd_apply("plain", dadev, None, None, 1, M, ydev, co, M, C, act, dt)
    check_project(dy, y.grad, dt, f"bn_act_bwd_apply act={act} C={C}")


# ----------------------------------------------------------------------------------------------------------------------------------------
# 10. rejections
# ----------------------------------------------------------------------------------------------------------------------------------------
def test_rejections_leave_the_outputs_untouched():
    """Each of these raises PcrlError and leaves a sentinel-filled output untouched: the first stage with a channel-vector count that does not
    divide 256; the row term, the second gradient, apply + gap and the pool entries at such a C; C = 1 in bf16; M * C no multiple of the
    vector; odd D, H or W; N * S != M; a workspace one byte short (PCRL_EWORKSPACE = -3); no gradient at all for _sum."""
    M = 48
    out = torch.full((M * 96 * 8,), SENT, dtype=F32, device=DEV)
    t = torch.zeros(M * 96 * 8, dtype=F32, device=DEV)
    co = npc.Coef(96, 1, DEV)
    f, b = dtype_code(F32), dtype_code(BF16)
    coef2 = (co.scale, co.shift)
    coef4 = (co.scale, co.shift, co.mean, co.rstd)
    coef5 = (co.scale, co.shift, co.k1, co.kB, co.kA)
    g = torch.zeros(4 * 96, dtype=F32, device=DEV)
    ws = ws_of(1 << 16)
    cases = [
        ("reduce, C = 24", "pcrl_bn_act_bwd_reduce", (t, t, *coef4, out, M, 24, ACT_RELU, f)),
        ("reduce, C = 96 bf16", "pcrl_bn_act_bwd_reduce", (t, t, *coef4, out, M, 96, ACT_RELU, b)),
        ("row term apply, C = 24", "pcrl_bn_act_bwd_apply_rowadd", (t, g, 4, 12, t, out, *coef5, M, 24, ACT_RELU, f)),
        ("row term reduce, C = 24", "pcrl_bn_act_bwd_reduce_rowadd", (t, g, 4, 12, t, *coef4, out, M, 24, ACT_RELU, f)),
        ("second gradient apply, C = 24", "pcrl_bn_act_bwd_apply_sum", (t, t, None, 1, M, t, out, *coef5, M, 24, ACT_RELU, f)),
        ("second gradient reduce, C = 24", "pcrl_bn_act_bwd_reduce_sum", (t, t, None, 1, M, t, *coef4, out, M, 24, ACT_RELU, f)),
        ("apply + gap, C = 24", "pcrl_bn_act_apply_gap", (t, out, out, *coef2, ws, 1 << 16, 4, 12, 24, ACT_RELU, f)),
        ("apply + pool, C = 24", "pcrl_bn_act_apply_pool", (t, out, out, *coef2, 1, 2, 2, 2, 24, ACT_RELU, f)),
        ("reduce + pool, C = 24", "pcrl_bn_act_bwd_reduce_pool", (t, t, *coef4, out, 1, 2, 2, 2, 24, ACT_RELU, f)),
        ("backward apply + pool, C = 24", "pcrl_bn_act_bwd_apply_pool", (t, t, out, *coef5, 1, 2, 2, 2, 24, ACT_RELU, f)),
        ("apply, C = 1 bf16", "pcrl_bn_act_apply", (t, out, *coef2, M, 1, ACT_RELU, b)),
        ("backward apply, C = 1 bf16", "pcrl_bn_act_bwd_apply", (t, t, out, *coef5, M, 1, ACT_RELU, b)),
        ("apply, C = 1, M = 1001", "pcrl_bn_act_apply", (t, out, *coef2, 1001, 1, ACT_RELU, f)),
        ("backward apply, C = 1, M = 1001", "pcrl_bn_act_bwd_apply", (t, t, out, *coef5, 1001, 1, ACT_RELU, f)),
        ("reduce, C = 1, M = 1001", "pcrl_bn_act_bwd_reduce", (t, t, *coef4, out, 1001, 1, ACT_RELU, f)),
        ("maxpool fwd, odd D", "pcrl_maxpool3d_2_fwd", (t, out, 1, 3, 4, 4, 8, f)),
        ("maxpool bwd, odd H", "pcrl_maxpool3d_2_bwd", (t, t, out, 1, 4, 3, 4, 8, f)),
        ("maxpool fwd, odd W", "pcrl_maxpool3d_2_fwd", (t, out, 1, 4, 4, 5, 8, b)),
        ("apply + pool, odd W", "pcrl_bn_act_apply_pool", (t, out, out, *coef2, 1, 4, 4, 5, 8, ACT_RELU, f)),
        ("reduce + pool, odd D", "pcrl_bn_act_bwd_reduce_pool", (t, t, *coef4, out, 1, 3, 4, 4, 8, ACT_RELU, f)),
        ("backward apply + pool, odd H", "pcrl_bn_act_bwd_apply_pool", (t, t, out, *coef5, 1, 4, 3, 4, 8, ACT_RELU, f)),
        ("row term apply, N S != M", "pcrl_bn_act_bwd_apply_rowadd", (t, g, 3, 5, t, out, *coef5, 16, 8, ACT_RELU, f)),
        ("row term reduce, N S != M", "pcrl_bn_act_bwd_reduce_rowadd", (t, g, 3, 5, t, *coef4, out, 16, 8, ACT_RELU, f)),
        ("sum apply with a row term, N S != M", "pcrl_bn_act_bwd_apply_sum", (t, None, g, 3, 5, t, out, *coef5, 16, 8, ACT_RELU, f)),
        ("sum apply, no gradient", "pcrl_bn_act_bwd_apply_sum", (None, None, None, 1, M, t, out, *coef5, M, 8, ACT_RELU, f)),
        ("sum reduce, no gradient", "pcrl_bn_act_bwd_reduce_sum", (None, None, None, 1, M, t, *coef4, out, M, 8, ACT_RELU, f)),
    ]
    for what, name, args in cases:
        with pytest.raises(PcrlError):
            call(name, *args)
            pytest.fail(f"{what}: accepted")
    for what, name, args, need in [
        ("colsum", "pcrl_colsum", lambda nb: (t, out, ws, nb, 100, 8, f), lib().call("pcrl_colsum_ws_bytes", 100, 8)),
        ("gap_fwd", "pcrl_gap_fwd", lambda nb: (t, out, ws, nb, 3, 100, 8, f), lib().call("pcrl_gap_ws_bytes", 3, 100, 8)),
        ("apply + gap", "pcrl_bn_act_apply_gap", lambda nb: (t, out, out, *coef2, ws, nb, 3, 100, 8, ACT_RELU, f), lib().call("pcrl_gap_ws_bytes", 3, 100, 8)),
    ]:
        with pytest.raises(PcrlError, match=r"\(-3\)"):
            call(name, *args(need - 1))
    torch.cuda.synchronize()
    assert bool((out == SENT).all()), "a refused call wrote to its output"
