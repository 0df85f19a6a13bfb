"""Case table, lattices and float64 restatements for csrc/extras_groupnorm.hip and csrc/variants.hip (test_variant_cases_cpu.py,
test_variants_edges_gpu.py): the coefficient kernels of norm='gn' / norm='in', the two PReLU passes of act='prelu'.  Not a test file.

Three lattices make a float32 result independent of the summation order and of whether the compiler contracts a product into a following
addition (these two files are not built with -ffp-contract=off); the preconditions are asserted analytically by test_variant_cases_cpu.py:
  stats         y = i/4, |i| <= 8 (bf16 values): every float32 sum and sum of squares over the 512 rows of a tile is exact
  bwd_finalize  partials = i/4, |i| <= partial_int(cpg, rows_b) <= 8; gamma = j/4, |j| <= 8; S * cpg a power of two; rstd in {1/2, 1, 2};
                mean = j/8, |j| <= 8: m1, m2, k1, kB, kA and every intermediate have at most 24 significant bits
  prelu         z, da = i/4, |i| <= 8 (z = 0 included); slope w = j/8, |j| <= 8: w * da and da * z are exact, a column sum stays below 2^24 units

The restatements take `prec`: torch.float64 is the reference; torch.float32 is the plain float32 evaluation of the same scale-and-shift
formula that serves as the yardstick of the ill-conditioned cases.  They work on CPU and device tensors alike.
"""
import math

import numpy as np
import torch

from norm_pool_cases import _tokens, read_source

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
ACT_NONE, ACT_ELU = 0, 4
PCRL_F32, PCRL_BF16 = 0, 1

# ---- the constants of the two sources, restated (test_variant_cases_cpu.py compares them with the source text token by token) ----
GN_TILE_ROWS = 512               # rows of one (sum, sum of squares) partial of pcrl_gn_stats
PRELU_TILE_ROWS = 256            # rows of one slope-gradient partial of pcrl_prelu_bwd
PRELU_GRID_CAP = 4096            # blocks of pcrl_prelu_fwd: 4096 x 256 channel vectors in one grid-stride pass
GN_C_MAX = 1024                  # gn_check(): the finalize kernels keep a sample's channel sums in LDS
FINALIZE_STRIDE = 256            # `g += 256`: groups per trip of the two finalize kernels
EPS32 = float(np.float32(1e-5))  # the kernel widens a float32 eps

SOURCE_PINS = [
    ("extras_groupnorm.hip", "constexpr int GN_TILE_ROWS = 512;"),
    ("extras_groupnorm.hip", "C <= 0 || C > 1024 || G <= 0 || C % G != 0"),
    ("extras_groupnorm.hip", "C % vec == 0 && (C / vec) <= 256 && 256 % (C / vec) == 0"),
    ("extras_groupnorm.hip", "for (int g = threadIdx.x; g < G; g += 256)"),
    ("extras_groupnorm.hip", "__shared__ double cs[1024][2];"),
    ("variants.hip", "constexpr int PRELU_TILE_ROWS = 256;"),
    ("variants.hip", "(nv + 255) / 256 < 4096 ? (nv + 255) / 256 : 4096"),
    ("variants.hip", "C % vec != 0 || C / vec > 256 || 256 % (C / vec) != 0"),
]


def source_pins_missing(pins=None):
    """-> the pins whose token sequence does not occur in their file"""
    missing = []
    for f, text in SOURCE_PINS if pins is None else pins:
        hay, pin = " ".join(_tokens(read_source(f))), " ".join(_tokens(text))
        if f" {pin} " not in f" {hay} ":
            missing.append((f, text))
    return missing


def vec(dt):
    return 8 if dt == BF16 else 4


def c_ok(C, dt):
    """the `256 % (C / vec)` rule of pcrl_gn_stats and prelu_check()"""
    v = vec(dt)
    return C > 0 and C % v == 0 and C // v <= 256 and 256 % (C // v) == 0


def nslots(C, dt):
    return 256 // (C // vec(dt))


def gn_tiles(S):
    return -(-S // GN_TILE_ROWS)


def prelu_rows(M):
    return -(-M // PRELU_TILE_ROWS)


def prelu_grid(M, C, dt):
    """-> (blocks of the launch, blocks the channel vectors ask for)"""
    want = -(-(M * C // vec(dt)) // 256)
    return min(want, PRELU_GRID_CAP), want


# ---- restatements ----
def group_sum(t, G):
    """[N, C] -> [N, G]: the sum over the C / G channels of a group"""
    N, C = t.shape
    return t.view(N, G, C // G).sum(2)


def per_channel(t, C):
    """[N, G] -> [N, C]"""
    return t.repeat_interleave(C // t.shape[1], dim=1)


def gn_finalize_ref(s1, s2, S, G, gamma, beta, eps=EPS32, prec=F64):
    """gn_finalize_kernel on per-(sample, channel) sums s1, s2 [N, C], in its order: a / cnt, b / cnt - mu * mu, the clamp at 0,
    1 / sqrt(var + eps).  -> mean [N, G], rstd [N, G], scale [N, C], shift [N, C]"""
    N, C = s1.shape
    cnt = float(S * (C // G))
    a, b = group_sum(s1.to(prec), G), group_sum(s2.to(prec), G)
    mu = a / cnt
    var = b / cnt - mu * mu
    var = torch.where(var < 0, torch.zeros_like(var), var)
    rstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma.to(prec) * per_channel(rstd, C)
    shift = beta.to(prec) - per_channel(mu, C) * scale
    return mu, rstd, scale, shift


def gn_forward_ref(y, gamma, beta, G, eps=EPS32, prec=F64):
    """GroupNorm(G) without activation of y [N, S, C] -> (mean [N, G], rstd [N, G], scale [N, C], shift [N, C], output [N, S, C])"""
    yp = y.to(prec)
    mu, rstd, scale, shift = gn_finalize_ref(yp.sum(1), (yp * yp).sum(1), y.shape[1], G, gamma, beta, eps, prec)
    return mu, rstd, scale, shift, scale.unsqueeze(1) * yp + shift.unsqueeze(1)


def gn_bwd_coef_ref(A, B, S, G, gamma, mean_c, rstd_c, prec=F64):
    """gn_bwd_finalize_kernel: A = sum dz, B = sum dz * xhat per (sample, channel) [N, C]; mean_c, rstd_c [N, C]
    -> k1, kB, kA, dgamma_n, dbeta_n, all [N, C]:  dx = k1 dz + kB y + kA"""
    N, C = A.shape
    cnt = float(S * (C // G))
    g, r, mu = gamma.to(prec), rstd_c.to(prec), mean_c.to(prec)
    m1 = per_channel(group_sum(g * A.to(prec), G) / cnt, C)
    m2 = per_channel(group_sum(g * B.to(prec), G) / cnt, C)
    return r * g, -r * r * m2, r * r * m2 * mu - r * m1, B.to(prec), A.to(prec)


def act_ref(z, act):
    if act == ACT_ELU:
        return torch.where(z > 0, z, torch.expm1(z))
    assert act == ACT_NONE
    return z


def dact_ref(z, da, act):
    if act == ACT_ELU:
        return torch.where(z > 0, da, da * torch.exp(z))
    assert act == ACT_NONE
    return da


def gn_ref(y, da, gamma, beta, G, act, eps=EPS32, prec=F64):
    """forward and backward of act(GroupNorm(G)(y)) on [N, S, C] tensors, by the scale-and-shift formulation of the kernels
    -> dict(mean, rstd [N, G]; out, dx [N, S, C]; dgamma, dbeta [C])"""
    N, S, C = y.shape
    mu, rstd, scale, shift, z = gn_forward_ref(y, gamma, beta, G, eps, prec)
    yp = y.to(prec)
    dz = dact_ref(z, da.to(prec), act)
    mean_c, rstd_c = per_channel(mu, C), per_channel(rstd, C)
    xhat = (yp - mean_c.unsqueeze(1)) * rstd_c.unsqueeze(1)
    k1, kB, kA, dg_n, db_n = gn_bwd_coef_ref(dz.sum(1), (dz * xhat).sum(1), S, G, gamma, mean_c, rstd_c, prec)
    dx = k1.unsqueeze(1) * dz + kB.unsqueeze(1) * yp + kA.unsqueeze(1)
    return dict(mean=mu, rstd=rstd, out=act_ref(z, act), dx=dx, dgamma=dg_n.sum(0), dbeta=db_n.sum(0))


def prelu_fwd_ref(z, w, prec=F64):
    """aten::prelu on [M, C]: z > 0 ? z : w[c] * z"""
    zp = z.to(prec)
    return torch.where(zp > 0, zp, w.to(prec) * zp)


def prelu_bwd_ref(da, z, w, prec=F64):
    """aten::prelu_backward on [M, C] -> (dz [M, C], dslope [C]): a row with z == 0 takes w * da and adds da * 0 to the slope gradient"""
    zp, dp = z.to(prec), da.to(prec)
    return torch.where(zp > 0, dp, w.to(prec) * dp), torch.where(zp > 0, torch.zeros_like(dp), dp * zp).sum(0)


# ---- lattices ----
Y_INT, Y_DEN = 8, 4              # stats and prelu: y, z, da = i/4
W_INT, W_DEN = 8, 8              # prelu slope j/8
GAMMA_INT, GAMMA_DEN = 8, 4      # bwd_finalize: gamma j/4
MU_INT, MU_DEN = 8, 8            # bwd_finalize: mean j/8
RSTD_EXP = (-1, 1)               # bwd_finalize: rstd = 2^e
PART_DEN = 4                     # bwd_finalize: partials i/4


def lat(shape, max_int, den, dt, seed, device="cpu"):
    """randint(-max_int, max_int) / den in `dt`"""
    g = torch.Generator(device=device).manual_seed(seed)
    t = torch.randint(-max_int, max_int + 1, tuple(shape), generator=g, device=device, dtype=torch.int32)
    return t.to(F32).div_(den).to(dt)


def kA_units(cpg, rows_b, part_int):
    """largest |r^2 m2 mu| + |r m1| in units of the finest one: m = K / (16 cnt) with |K| <= cpg * GAMMA_INT * part_int * rows_b;
    r^2 mu is a multiple of 1/32 at most 4, r a multiple of 1/2 at most 2: the unit is 1 / (16 cnt * 32)"""
    K = cpg * GAMMA_INT * part_int * rows_b
    rr_mu = (2.0 ** (2 * RSTD_EXP[1])) * MU_INT / MU_DEN
    return K * 32 * rr_mu + K * 32 * 2.0 ** RSTD_EXP[1]


def partial_int(cpg, rows_b):
    """the largest |i| <= 8 of the partials i/4 at which kA of a group of `cpg` channels over `rows_b` partial rows still fits 24 bits"""
    i = Y_INT
    while i > 1 and not kA_units(cpg, rows_b, i) < 2.0 ** 24:
        i -= 1
    return i


class BwdLattice:
    """inputs of pcrl_gn_bwd_finalize on the lattice (CPU float32 tensors): partial_b [N, rows_b, C, 2], gamma [C], mean_c, rstd_c [N, C]
    (constant within a group, as gn_finalize_kernel writes them)"""

    def __init__(self, N, C, G, rows_b, seed):
        g = torch.Generator().manual_seed(seed)
        cpg = C // G
        pi = partial_int(cpg, rows_b)
        self.partial = torch.randint(-pi, pi + 1, (N, rows_b, C, 2), generator=g).float() / PART_DEN
        self.gamma = torch.randint(-GAMMA_INT, GAMMA_INT + 1, (C,), generator=g).float() / GAMMA_DEN
        mean = torch.randint(-MU_INT, MU_INT + 1, (N, G), generator=g).float() / MU_DEN
        rstd = 2.0 ** torch.randint(RSTD_EXP[0], RSTD_EXP[1] + 1, (N, G), generator=g).float()
        self.mean_c, self.rstd_c = per_channel(mean, C).contiguous(), per_channel(rstd, C).contiguous()


def serial_sum64(partial):
    """[N, rows, C, 2] float32 -> float64 [N, C, 2]: the rows added one after the other, the order of both finalize kernels"""
    acc = torch.zeros(partial.shape[0], partial.shape[2], 2, dtype=F64, device=partial.device)
    for t in range(partial.shape[1]):
        acc = acc + partial[:, t].double()
    return acc


def finalize_partials(N, C, G, S, seed):
    """hand-made partials of pcrl_gn_finalize: the float32-rounded per-tile (sum, sum of squares) of y = off[n][g] + uniform(-1/2, 1/2) with
    1 <= |off| <= 2: no value is nearer to 0 than 1/2 (the mean has no cancellation), mu^2 / var is about 12 .. 48 (far below 2^20)
    -> (partial float32 [N, tiles, C, 2], gamma, beta float32 [C])"""
    g = torch.Generator().manual_seed(seed)
    off = (1 + torch.rand(N, G, generator=g, dtype=F64)) * (torch.randint(0, 2, (N, G), generator=g) * 2 - 1)
    y = per_channel(off, C).unsqueeze(1) + torch.rand(N, S, C, generator=g, dtype=F64) - 0.5
    tiles = gn_tiles(S)
    pad = torch.zeros(N, tiles * GN_TILE_ROWS - S, C, dtype=F64)
    yt = torch.cat([y, pad], 1).view(N, tiles, GN_TILE_ROWS, C)
    partial = torch.stack([yt.sum(2), (yt * yt).sum(2)], dim=3).float().contiguous()
    gamma = (torch.rand(C, generator=g) + 0.5) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1)
    beta = torch.rand(C, generator=g) - 0.5
    return partial, gamma.float(), beta.float()


def clamp_partials(C):
    """a constant group x = 1000 over three rows: s1 = 3000, s2 one float32 step below 3e6: s2 / 3 - mu^2 = -1/12 in float64
    -> partial [1, 1, C, 2] for S = 3, G = C"""
    s1 = torch.full((C,), 3000.0, dtype=F32)
    s2 = torch.nextafter(torch.full((C,), 3.0e6, dtype=F32), torch.zeros(C, dtype=F32))
    return torch.stack([s1, s2], dim=1).view(1, 1, C, 2).contiguous()


def ulp32(x):
    """float64 tensor -> the float32 unit in the last place of |x| (of the smallest normal number for smaller |x|)"""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126)))
    return torch.pow(torch.full_like(x, 2.0), e - 23)


# ---- case tables ----
# (C, G): the model's own pairs (norm='gn': G = 8; norm='in': G = C), the head's [S/4][4] view with one group, and the edges: one channel
# vector with 256 row slots; G > 256 (a second trip of `g += 256`) with one row slot in float32; one group of 1024 channels
CG_PAIRS = [(C, G) for C in (32, 64, 128, 256, 512) for G in (8, C)] + [(4, 1), (4, 4), (8, 8), (1024, 1024), (1024, 512), (1024, 1)]
S_VALUES = [1, 2, 511, 512, 513, 1025]       # around one tile of 512 rows; 1025: a third tile of ONE row.  S = 1 only where cpg > 1
N_VALUES = [1, 3]                            # sample 2: the slices scale[n * C:] and partial_b[n * rows_b * C * 2:] are not at offset 0


def dtypes_of(C):
    return [dt for dt in (F32, BF16) if c_ok(C, dt)]


CG_DT = [(C, G, dt) for C, G in CG_PAIRS for dt in dtypes_of(C)]
C_DT = sorted({(C, dt) for C, G, dt in CG_DT}, key=lambda t: (t[0], t[1] == BF16))


def sn_of(C, G):
    return [(S, N) for S in S_VALUES for N in N_VALUES if S > 1 or C // G > 1]


def ill_conditioned(C, G, S):
    """a group of TWO values: xhat = +-1 / sqrt(1 + eps / var) whatever the data, and dx = k1 dz + kB y + kA is the residue of eps alone --
    terms of order 1 that cancel to order eps / var in whatever evaluates the formula in float32.  There the float32 yardstick may replace
    the project tolerance."""
    return S * (C // G) == 2


def gn_inputs(N, S, C, G, dt, seed):
    """CPU float64 tensors holding dt values: y[n][s][c] = off[n][g] + (-1)^(s + c) * a with a = 1 + uniform(-1/2, 1/2) and off in (-1, 1) per
    (sample, group): every group of two or more values has members on either side of its offset, at least 1/2 away from it -- a group's
    variance is at least about 1/4 against mean^2 < 4, small groups included, and the samples' statistics differ.  da = uniform(-1, 1);
    gamma = 1 + 0.3 uniform, beta = 0.3 uniform (float32)"""
    def rnd(*shape, k):
        g = torch.Generator().manual_seed(seed + k)
        return torch.rand(*shape, generator=g, dtype=F64) * 2 - 1

    sign = 1.0 - 2.0 * ((torch.arange(S).view(1, S, 1) + torch.arange(C).view(1, 1, C)) % 2).double()
    off = per_channel(rnd(N, G, k=1), C).unsqueeze(1)
    y = (off + sign * (1.0 + 0.5 * rnd(N, S, C, k=0))).to(dt).double()
    da = rnd(N, S, C, k=2).to(dt).double()
    return y, da, (1 + 0.3 * rnd(C, k=3)).float(), (0.3 * rnd(C, k=4)).float()


# pcrl_gn_finalize with hand-made partials: (N, C, G, S)
FINALIZE_CASES = [(3, 32, 8, 513), (3, 4, 1, 1025), (1, 8, 8, 64), (3, 1024, 1024, 64), (1, 1024, 512, 1025), (3, 1024, 1, 513), (3, 512, 512, 600)]
# pcrl_gn_bwd_finalize on its lattice: (N, C, G, S, rows_b), S * cpg a power of two
BWD_FINALIZE_CASES = [(1, 32, 8, 64, 1), (3, 32, 32, 128, 3), (3, 4, 1, 256, 33), (3, 1024, 1024, 32, 2), (1, 1024, 512, 16, 3), (3, 1024, 1, 4, 1),
                      (3, 512, 8, 1, 1), (3, 256, 256, 2, 1)]
BWD_FINALIZE_RANDOM = (3, 96, 12, 77, 3)     # nothing a power of two

# PReLU: M around one and two tiles of 256 rows; C / vec in {1, 8, 128, 256}
PRELU_M = [1, 255, 256, 257, 513]
PRELU_C = [(F32, 4), (F32, 32), (F32, 1024), (BF16, 8), (BF16, 64), (BF16, 1024)]
PRELU_BIG = (F32, 32, 131072 + 3)            # 1 048 600 channel vectors: 24 past 4096 x 256; 16 MB
