"""Case table, lattices and float64 restatements for csrc/norm_pool.hip (test_norm_pool_cases_cpu.py, test_norm_pool_gpu.py).  Not a test file.

The apply / reduce entry points of the 3D BatchNorm take their per-channel coefficients (scale, shift, mean, rstd, k1, kB, kA) as INPUTS, so a
test can put them on a dyadic lattice next to the activations:
  y, da, da2, dp = i/4, |i| <= 8      scale = j/4, 0 < |j| <= 40      shift, kA = j/8, |j| <= 16      mean = j/8, |j| <= 8      kB = j/4, |j| <= 8
  rstd in {1/2, 1, 2}                 k1 in {1/2, 1, 2, 4}            row term g[n][c] = S * m/4, m = 0, +-1, +-2, +-4, +-8 (times (float)(1/S): m/4 again)
Every product and every sum of the kernels is then exact in float32 in any order (the preconditions are asserted analytically by
test_norm_pool_cases_cpu.py), and an output must equal the float64 value, or its round-to-nearest-even rounding to bf16, at every element.
scale reaches 10, so z = scale * y + shift reaches 352/16: more than the 8 significant bits of bf16, the output rounding is exercised.

The restatements work on CPU and device tensors alike (the large cases never leave the device) and mirror the kernels' rounding points where
the lattice does not make them moot: the row term is g * (float)(1.0 / S) in float32 added as (da + da2) + add; the pooling argmax is taken on
the activation ROUNDED to the storage type; the global average is (float)(sum * (1.0 / S)) in float64.
"""
import math
import os
import re

import torch

F32, BF16 = torch.float32, torch.bfloat16
ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SILU, ACT_ELU = 0, 1, 2, 3, 4

# ---- the constants of the source, restated (test_norm_pool_cases_cpu.py checks them against the text of norm_pool.hip / common.h) ----
TILE_ROWS = 1024                 # rows of a first-stage partial at full size
RC_CAP = 2048                    # rc_grid(): blocks of the register-cached kernels
GRID_CAP = 16384                 # grid_for(): blocks of the grid-stride kernels
CAP_ITEMS = GRID_CAP * 256       # 4 194 304 work items in one grid-stride pass
NT_BYTES = 192 << 20             # pcrl_streaming(): non-temporal twins from this many bytes per tensor on
SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pcrlv2_amd", "csrc")

SOURCE_PINS = [                  # (file, source text, compared token by token: spacing and line breaks do not matter): a change of a constant
    ("norm_pool.hip", "constexpr int TILE_ROWS = 1024;"),                      # must be noticed by the case table
    ("norm_pool.hip", "if (b > 16384) b = 16384;"),
    ("norm_pool.hip", "if (b > 2048) b = 2048;"),
    ("norm_pool.hip", "while (t > 32 && M / t < 1024) t >>= 1;"),
    ("norm_pool.hip", "int t = TILE_ROWS / 8;"),
    ("norm_pool.hip", "while (t > 4 && Mp / t < 1024) t >>= 1;"),
    ("norm_pool.hip", "while (t > 32 && (int64_t)N * ((S + t - 1) / t) < 512) t >>= 1;"),
    ("norm_pool.hip", "for (; r + 768 < rows; r += 1024)"),
    ("norm_pool.hip", "for (; t + 24 < tiles; t += 32)"),
    ("norm_pool.hip", "#define BN_RED_U 4"),
    ("common.h", "return bytes >= ((int64_t)192 << 20);"),
]


def vec(dt):
    return 8 if dt == BF16 else 4


def esize(dt):
    return 2 if dt == BF16 else 4


def streaming(nbytes):
    return nbytes >= NT_BYTES


def rc_ok(C, dt):
    v = vec(dt)
    return C % v == 0 and C // v <= 256 and 256 % (C // v) == 0


def nslots(C, dt):
    return 256 if C == 1 else 256 // (C // vec(dt))


def rc_blocks(M, C, dt):
    """-> (blocks of the launch, blocks the rows ask for): the grid wraps when the second exceeds RC_CAP"""
    want = -(-M // nslots(C, dt))
    return min(want, RC_CAP), want


def bn_bwd_tile_rows(M):
    t = TILE_ROWS
    while t > 32 and M // t < 1024:
        t >>= 1
    return t


def bn_pool_tile(Mp):
    t = TILE_ROWS // 8
    while t > 4 and Mp // t < 1024:
        t >>= 1
    return t


def coltile_rows(N, S):
    t = TILE_ROWS
    while t > 32 and N * (-(-S // t)) < 512:
        t >>= 1
    return t


def coltile_tiles(N, S):
    return -(-S // coltile_rows(N, S))


def u4_passes(M, C, dt):
    """how often the four-rows-in-flight loop of bn_bwd_reduce runs for slot 0 of a FULL tile"""
    tile, ns = bn_bwd_tile_rows(M), nslots(C, dt)
    if C == 1:
        tile //= vec(dt)
    n, r = 0, 0
    while r + 3 * ns < tile:
        n, r = n + 1, r + 4 * ns
    return n


# ---- lattice bounds, in the integers of the module docstring ----
Y_INT, Y_DEN = 8, 4
SC_INT, SC_DEN = 40, 4
SH_INT, SH_DEN = 16, 8
MU_INT, MU_DEN = 8, 8
KB_INT, KB_DEN = 8, 4
RSTD_EXP = (-1, 1)
K1_EXP = (-1, 2)


class Coef:
    """per-channel lattice coefficients: float32 tensors on `device`"""

    def __init__(self, C, seed, device):
        g = torch.Generator().manual_seed(seed)

        def ri(m):
            return torch.randint(-m, m + 1, (C,), generator=g).double()

        sc = ri(SC_INT)
        sc[sc == 0] = 1.0
        self.scale = sc / SC_DEN
        self.shift = ri(SH_INT) / SH_DEN
        self.mean = ri(MU_INT) / MU_DEN
        self.rstd = 2.0 ** torch.randint(RSTD_EXP[0], RSTD_EXP[1] + 1, (C,), generator=g).double()
        self.k1 = 2.0 ** torch.randint(K1_EXP[0], K1_EXP[1] + 1, (C,), generator=g).double()
        self.kB = ri(KB_INT) / KB_DEN
        self.kA = ri(SH_INT) / SH_DEN
        self.gamma = ri(8) / 4
        for k in ("scale", "shift", "mean", "rstd", "k1", "kB", "kA", "gamma"):
            setattr(self, k, getattr(self, k).float().to(device).contiguous())


ROW_M = (0.0, 1.0, -1.0, 2.0, -2.0, 4.0, -4.0, 8.0, -8.0)


def lat(shape, max_int, den, dt, seed, device):
    """randint(-max_int, max_int) / den in `dt`, generated on `device` (the large cases never cross to the host)"""
    g = torch.Generator(device=device).manual_seed(seed)
    t = torch.randint(-max_int, max_int + 1, tuple(shape), generator=g, device=device, dtype=torch.int8)
    return t.to(F32).div_(den).to(dt)


def row_term(N, C, S, seed, device):
    """g[n][c] = S * m/4 with m in ROW_M (zero and the signed powers of two up to 8): float32, exact (S * 8 < 2^24 for every S of the table),
    and g * (float)(1/S) is m/4 again for every S of the reduce cases, 61 696 included: S * (float)(1/S) rounds to 1 and a power of two only
    moves the exponent (test_norm_pool_cases_cpu.py evaluates that in float32 for every (S, m); m = 3, 5, 6, 7 do NOT land on m/4 there)"""
    return pow2_lat((N, C), seed, device) * (S / 4.0)


def row_term_general(N, C, seed, device):
    """g[n][c] = i/8, |i| <= 100, for the APPLY cases: its float32 product with (float)(1.0 / S) is inexact for S = 1000 and 5000 and so is the
    sum with da + da2 -- the restatement has to make the kernel's roundings at the kernel's places"""
    return lat((N, C), 100, 8, F32, seed, device)


def pow2_lat(shape, seed, device):
    """float32 values of ROW_M: a product with ANY float32 factor is exact, whether or not it is contracted into a following addition"""
    g = torch.Generator(device=device).manual_seed(seed)
    k = torch.randint(0, len(ROW_M), tuple(shape), generator=g, device=device)
    return torch.tensor(ROW_M, dtype=F32, device=device)[k]


def inv_s32(S):
    return torch.tensor(1.0 / S, dtype=torch.float64).float()


# ---- restatements ----
def act64(z, act):
    if act == ACT_RELU:
        return torch.where(z > 0, z, torch.zeros_like(z))
    assert act == ACT_NONE
    return z


def dact64(z, gin, act):
    if act == ACT_RELU:
        return torch.where(z > 0, gin, torch.zeros_like(gin))
    assert act == ACT_NONE
    return gin


def ref_apply(y, co, act, dt):
    """a = act(scale * y + shift): exact in float64, rounded once to dt"""
    return act64(co.scale.double() * y.double() + co.shift.double(), act).to(dt)


def ref_gin(rows, C, device, da=None, da2=None, g=None, S=1, row0=0):
    """float32 ((da + da2) + g[n] * (float)(1.0 / S)) for the rows row0 .. row0 + rows, the kernel's order and rounding points (line 237)"""
    t = torch.zeros((rows, C), dtype=F32, device=device)
    if da is not None:
        t = t + da.float()
    if da2 is not None:
        t = t + da2.float()
    if g is not None:
        add = g.float() * inv_s32(S).to(device)
        n = torch.arange(row0, row0 + rows, device=device) // S
        t = t + add[n]
    return t


def ref_bwd_apply(gin, y, co, act, dt):
    """dy = (k1 * dz + kB * y) + kA with float32 roundings after the sum of the two (exact) products and after the last addition"""
    y64 = y.double()
    dz = dact64(co.scale.double() * y64 + co.shift.double(), gin.double(), act)
    t = (co.k1.double() * dz + co.kB.double() * y64).float().double() + co.kA.double()
    return t.float().to(dt)


def ref_reduce(gin, y, co, act):
    """-> float64 (sum dz, sum dz * (y - mean) * rstd) per channel"""
    y64 = y.double()
    dz = dact64(co.scale.double() * y64 + co.shift.double(), gin.double(), act)
    return dz.sum(0), (dz * (y64 - co.mean.double()) * co.rstd.double()).sum(0)


def windows(x5):
    """[N, D, H, W, C] -> [Mp, 8, C]: window position t = 4 dd + 2 hh + ww, the kernels' scan order"""
    N, D, H, W, C = x5.shape
    return x5.reshape(N, D // 2, 2, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(-1, 8, C)


def unwindows(w, N, D, H, W):
    C = w.shape[-1]
    return w.reshape(N, D // 2, H // 2, W // 2, 2, 2, 2, C).permute(0, 1, 4, 2, 5, 3, 6, 7).reshape(N, D, H, W, C)


def pool_arg(aw):
    """[Mp, 8, C] -> [Mp, C]: `if (f > m || f != f)` from m = -inf: the FIRST maximum in scan order; a NaN takes over wherever it stands, so
    the LAST NaN of a window wins; an all -inf window keeps position 0.  (aten's max_pool3d rule.)"""
    aw = aw.float()
    nan = aw != aw
    m = torch.where(nan, torch.full_like(aw, -math.inf), aw).amax(1, keepdim=True)
    ismax = (aw == m) & ~nan
    down = torch.arange(8, 0, -1, device=aw.device).view(1, 8, 1)
    up = torch.arange(1, 9, device=aw.device).view(1, 8, 1)
    first = (ismax * down).argmax(1)
    last_nan = (nan * up).argmax(1)
    return torch.where(nan.any(1), last_nan, first)


def take(w, arg):
    return w.gather(1, arg.unsqueeze(1)).squeeze(1)


def ref_maxpool_bwd(arg, gy):
    """[Mp, C] argmax and pooled gradient -> [Mp, 8, C]: the gradient's bits at the argmax, +0 elsewhere"""
    dxw = torch.zeros((gy.shape[0], 8, gy.shape[1]), dtype=gy.dtype, device=gy.device)
    return dxw.scatter_(1, arg.unsqueeze(1), gy.unsqueeze(1))


def ref_pool_fused(yw, gp, co, act, dt):
    """yw [Mp, 8, C] (dt), gp [Mp, C] (dt) -> a windows (dt), pooled p (dt), s1, s2 (float64 [C]), dy windows (dt): the argmax on the
    activation rounded to dt (line 603), dz and the statistics from the pre-activation of THAT element.  NaN and inf go through float64 as
    through float32 (0 * inf = NaN included): ReLU maps a NaN pre-activation to 0 (`z > 0.f ? z : 0.f`), without activation the last NaN of
    a window takes the gradient"""
    aw = ref_apply(yw, co, act, dt)
    arg = pool_arg(aw)
    p = take(aw, arg)
    yb = take(yw.double(), arg)
    zb = co.scale.double() * yb + co.shift.double()
    # a window whose rounded activations are ALL -inf never satisfies `a > m || a != a` from m = -inf: arg, zb and ybest keep their start 0
    start = (aw.float() == -math.inf).all(1)
    yb, zb = torch.where(start, torch.zeros_like(yb), yb), torch.where(start, torch.zeros_like(zb), zb)
    dz = dact64(zb, gp.double(), act)
    s1, s2 = dz.sum(0), (dz * (yb - co.mean.double()) * co.rstd.double()).sum(0)
    dzw = torch.zeros(yw.shape, dtype=torch.float64, device=yw.device).scatter_(1, arg.unsqueeze(1), dz.unsqueeze(1))
    t = (co.k1.double() * dzw + co.kB.double() * yw.double()).float().double() + co.kA.double()
    return aw, p, s1, s2, t.float().to(dt)


def finalize64(s1, s2, count, gamma, beta, rm, rv, momentum, eps):
    """bn_finalize_kernel lines 73-85 in float64 (inputs float64 tensors [C], eps and momentum the float32 values) -> float64 results"""
    mu = s1 / count
    var = s2 / count - mu * mu
    var = torch.where(var < 0, torch.zeros_like(var), var)
    rs = 1.0 / torch.sqrt(var + eps)
    sc = gamma * rs
    out = dict(mean=mu, rstd=rs, scale=sc, shift=beta - mu * sc)
    if rm is not None:
        out["running_mean"] = (1.0 - momentum) * rm + momentum * mu
        unb = var * count / (count - 1.0) if count > 1.0 else var
        out["running_var"] = (1.0 - momentum) * rv + momentum * unb
    return out


def clamp_partials():
    """three values of a constant channel x = 1000: s1 = 3000 and s2 one float32 step below 3e6: s2 / 3 - mu^2 = -1/12 in float64"""
    s1 = torch.tensor([3000.0], dtype=F32)
    s2 = torch.nextafter(torch.tensor([3.0e6], dtype=F32), torch.tensor([0.0], dtype=F32))
    return s1, s2, 3.0


def bwd_finalize64(s1, s2, count, gamma, mean, rstd):
    """bn_bwd_finalize_kernel lines 101-107 in float64"""
    g1 = gamma * rstd
    b = -g1 * rstd * s2 / count
    return dict(dbeta=s1, dgamma=s2, k1=g1, kB=b, kA=-g1 * s1 / count - b * mean)


# ---- case tables ----
def _wrap_rows(C, dt):
    ns = nslots(C, dt)
    return RC_CAP * ns + 2 * ns + max(ns // 3, 1)


# 2. register-cached apply: every nslots (C / vec in {1, 2, 8, 64, 256}), M = 2048 * nslots + a remainder that is no multiple of nslots
RC_CASES = [(dt, C, _wrap_rows(C, dt)) for dt, Cs in ((F32, (4, 8, 32, 256, 512, 1024)), (BF16, (8, 16, 64, 512, 2048))) for C in Cs]
RC_CASES += [(F32, 32, 100), (BF16, 64, 33)]           # below the cap: one row per thread at most

# 3. row term through the wrap: stride = 2048 * nslots rows = 4096 for C = 512 float32 / C = 1024 bf16
ROW_WRAP_CASES = [(dt, C, N, S) for dt, C in ((F32, 512), (BF16, 1024)) for N, S in ((9, 1000), (2, 5000), (9, 1024))]
ROW_WRAP_CASES += [(F32, 8, 5, 8), (BF16, 16, 5, 8)]
GRAD_VARIANTS = ["rowadd: da + row", "rowadd: row only", "sum: da only", "sum: row only", "sum: da + da2 + row", "sum: da + da2"]

# 4. generic kernels: channel-vector counts that do not divide 256, and C = 1
GENERIC_CASES = [(F32, 1, 4100), (F32, 12, 777), (F32, 24, 777), (F32, 96, 333), (BF16, 24, 777), (BF16, 96, 333)]
GENERIC_BIG = (F32, 24, 699101)   # 4 194 606 vectors: 302 past grid_for()'s cap; the stride 16 777 216 elements is 16 mod 24

# 5. backward first stage: (dt, C, M, row term (N, S) or None)
REDUCE_CASES = [
    (F32, 32, 65535, None),               # tile 32, 32 slots: the U = 4 loop runs zero times
    (F32, 32, 65536 + 5, None),           # tile 64, last tile of 5 rows
    (F32, 8, (1 << 17) + 3, None),        # tile 128 = one slot pass short of U = 4 (128 slots)
    (F32, 32, (1 << 17) + 91, None),      # tile 128 = 4 x 32 slots: once; the last tile has 91 rows, in (2, 3] x 32: three of four rows in flight exist
    (BF16, 8, (1 << 18) + 3, None),       # tile 256 = exactly the 256 slots
    (BF16, 16, (1 << 19) + 3, None),      # tile 512, 128 slots: U = 4 loop once
    (BF16, 8, (1 << 20) - 1, None),       # tile 512, 256 slots: zero times
    (BF16, 8, (1 << 20) + 37, None),      # tile 1024, 256 slots: exactly once; last tile of 37 rows
    (F32, 16, (1 << 20) + 37, None),      # tile 1024, 64 slots: four times
    (BF16, 16, 16 * 65536, (16, 65536)),  # S a multiple of the tile: ra_tile, U = 4 loop taken (twice)
    (BF16, 16, 17 * 61696, (17, 61696)),  # 61 696 = 60 * 1024 + 256: tiles straddle two samples, per-row lookup, unrolled loop skipped
    (F32, 32, 2048 * 32, (2048, 32)),     # tile 64 holds two samples of 32 rows
    (F32, 32, 8 * 8192, (8, 8192)),       # tile 64 divides S: ra_tile with a small tile
    (F32, 1, 4100, None),                 # C = 1: rows_total = M / 4 = 1025 "rows", tile 32 / 4 = 8: 129 partials, the last of one row
]

# 6. column sums / global average pool: (dt, C, N, S)
FINISH_TILES = [1, 7, 8, 9, 24, 25, 32, 33, 57]
COL_CASES = [((F32, BF16)[k % 2], (8, 16)[k % 2], (1, 3)[(k // 2) % 2], 32 * t - 5) for k, t in enumerate(FINISH_TILES)]
COL_CASES += [(F32, 16, 1, 31), (F32, 16, 1, 32), (F32, 16, 1, 33), (BF16, 8, 3, 31), (BF16, 8, 3, 33)]
COL_CASES += [(BF16, 8, 512, 1023), (BF16, 8, 512, 1024), (BF16, 8, 512, 1025)]          # tile 1024: S = tile - 1, tile, tile + 1
COL_CASES += [(BF16, 8, 1, 4096 * 1024 - 3)]                                             # 4096 tiles of 1024
COL_CASES += [(F32, 1024, 3, 32 * 9 - 5), (BF16, 1024, 1, 100), (BF16, 16, 3, 250), (F32, 8, 1, 32 * 57)]
GAP_BWD_BIG = (BF16, 32, 3, 349999)   # 4 199 988 vectors

# 7. pool fusions: (dt, C, (N, D, H, W)) -- Mp = N D H W / 8
POOL_CASES = [
    (BF16, 8, (1, 28, 30, 78)),     # Mp = 8190: tile 4, ragged
    (F32, 4, (1, 32, 32, 64)),      # Mp = 8192: tile 8
    (F32, 32, (1, 28, 30, 156)),    # Mp = 16380: tile 8, ragged
    (BF16, 16, (1, 32, 64, 64)),    # Mp = 16384: tile 16
    (BF16, 8, (1, 64, 64, 66)),     # Mp = 33792: tile 32
    (F32, 8, (1, 64, 66, 130)),     # Mp = 68640: tile 64, ragged
    (BF16, 8, (3, 22, 126, 130)),   # Mp = 135135: tile 128, Mp % 128 = 95
    (F32, 32, (3, 2, 6, 10)),       # Mp = 45: three samples, one block
]
POOL_BIG = (BF16, 32, (1, 128, 256, 258))   # 541 065 216 bytes: non-temporal, and 4 227 072 work items, past grid_for()'s cap

# 8. non-temporal twins: the first size at which pcrl_streaming() is true
NT_CASE = (BF16, 32, 3, 1 << 20)      # N = 3, S = 2^20: M = 3 145 728 rows of 64 bytes = 201 326 592 bytes


def pool_mp(dims):
    N, D, H, W = dims
    return N * (D // 2) * (H // 2) * (W // 2)


# ---- the enumerated pooling windows ----
def enumerated_windows():
    """[W, 8] integer ranks: each position as the single maximum, each of the 28 pairs as a tie, all equal, a descending and an ascending run"""
    rows = []
    for p in range(8):
        rows.append([1 if t == p else 0 for t in range(8)])
    for p in range(8):
        for q in range(p + 1, 8):
            rows.append([2 if t in (p, q) else 0 for t in range(8)])
    rows.append([3] * 8)
    rows.append(list(range(7, -1, -1)))
    rows.append(list(range(8)))
    return torch.tensor(rows, dtype=torch.float64)


def special_windows():
    """[W, 8] float64 for the plain pool: all -inf, a NaN at each position (others finite, one larger than the NaN's neighbours), two NaNs,
    (+0, -0, ...) and (-0, +0, ...) among negatives, -inf with one finite"""
    inf, nan = math.inf, math.nan
    rows = [[-inf] * 8]
    for p in range(8):
        r = [float(t % 3) for t in range(8)]
        r[p] = nan
        rows.append(r)
    rows.append([nan, 1.0, 2.0, nan, 5.0, 0.0, 0.0, 0.0])
    rows.append([0.0, -0.0, -1.0, -1.0, -2.0, -1.0, -0.0, 0.0])
    rows.append([-0.0, 0.0, -1.0, -1.0, -2.0, -1.0, 0.0, -0.0])
    rows.append([-inf, -inf, -inf, -5.0, -inf, -inf, -inf, -inf])
    return torch.tensor(rows, dtype=torch.float64)


def windows_to_volume(w):
    """[Wn, 8, C] -> [1, 2, 2, 2 Wn, C]: the windows side by side along W"""
    Wn, _, C = w.shape
    return unwindows(w, 1, 2, 2, 2 * Wn)


def read_source(name):
    return open(os.path.join(SOURCE, name)).read()


def _tokens(text):
    return re.findall(r"\w+|[^\w\s]", text)


def source_pins_hold():
    """-> the pins whose token sequence does not occur in their file"""
    missing = []
    for f, text in SOURCE_PINS:
        hay, pin = " ".join(_tokens(read_source(f))), " ".join(_tokens(text))
        if f" {pin} " not in f" {hay} ":
            missing.append((f, text))
    return missing
