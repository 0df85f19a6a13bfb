"""Case tables, lattices, float64 restatements and route mirrors for the one-channel convolutions (pcrl_conv3d_to1_fwd / _dgrad / _wgrad:
csrc/conv_c1.hip, conv_to1_brick.hip, conv_wgrad.hip) and the 2x2x2 / stride-2 transposed convolution (pcrl_convt3d_k2s2_fwd / _dgrad / _wgrad:
csrc/conv_up2.hip, conv_igemm.hip, conv_wgrad.hip).  Read by test_conv1_cases_cpu.py, test_conv_to1_exact_gpu.py and test_convt_exact_gpu.py.
Not a test file.

Method: tests/exact_lattice.py.  Every output here is a sum of products of two lattice values (plus a lattice bias / add term), so a float32
accumulator is exact in any order while the sum of the absolute values of the terms stays below 2^24 units; a float32 output then equals the
float64 value and a bf16 output its round-to-nearest-even rounding, at every element.  The references are F.conv3d / F.conv_transpose3d and
torch autograd in float64 on the CPU; the preconditions come from the same graph on the absolute values.  The four cases too large for that are
generated and restated on the device (chunked float64 products); their preconditions are bounded analytically (worst_units)."""
import collections
import functools
import os
import re
import types

import torch
import torch.nn.functional as F

import exact_lattice as X

F32, BF16 = torch.float32, torch.bfloat16

# ---- the constants of the source, restated (test_conv1_cases_cpu.py checks them against the text of the kernels' files) ----
TO1_VOX = 1024                   # conv_c1.hip TO1_VOX: voxels of a block of to1_fwd_kernel / shift_sum27_kernel = one statistics row
TO1_UNROLL = 4                   # conv_c1.hip U: voxels in flight per lane in the 1-tap fast path
LPV_CAP = 64                     # conv_c1.hip: lanes per voxel of to1_fwd_kernel
DGRAD_CAP = 8192                 # conv_c1.hip: blocks of to1_dgrad_kernel (grid-stride past 8192 * 256 work items)
LDS_NO_OPT_IN = 65536            # conv_c1.hip to1_check: taps * C * 4 bytes of dynamic LDS at most
IM2COL_CAP = 16384               # conv_wgrad.hip im2col_launch: blocks of im2col27_kernel
VECSUM_CAP, VECSUM_VOX = 1024, 4096     # conv_wgrad.hip: blocks of vecsum_partial_kernel, voxels a block is sized for
SCALAR_BRICK_BLOCKS = 512        # conv_wgrad.hip scalar_brick_blocks: blocks over all 64-channel tiles
BRICK = (4, 8, 8)                # conv_to1_brick.hip TD, TH, TW (the scalar weight-gradient brick kernel uses the same bricks)
UP2_ROWS = 128                   # conv_up2.hip UM: input voxels of a block of convt_up2_fwd_kernel
UP2_FILL = 768                   # conv_up2.hip: row blocks x splits the launch wants before it stops splitting the column tiles
UP2_WG_BLOCKS, UP2_WG_STEPS = 512, 16   # conv_wgrad.hip plan_up2: blocks of a round, least K-steps (of 32 voxels) per block
NT_BYTES = 192 << 20             # common.h pcrl_streaming(): non-temporal stores from this many bytes per tensor on
SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pcrlv2_amd", "csrc")

SOURCE_PINS = [                  # (file, source text, compared token by token): a changed constant must be noticed by the case tables
    ("conv_c1.hip", "constexpr int TO1_VOX = 1024;"),
    ("conv_c1.hip", "constexpr int U = 4;"),
    ("conv_c1.hip", "if (taps == 1 && nvec == lpv)"),
    ("conv_c1.hip", "if (lpv > 64) lpv = 64;"),
    ("conv_c1.hip", "if (blocks > 8192) blocks = 8192;"),
    ("conv_c1.hip", "if ((size_t)taps * C * sizeof(float) > 65536)"),
    ("conv_c1.hip", "if (taps == 27 && C % 32 == 0 && M % 4 == 0 && ws && ws_bytes >= pcrl_conv3d_to1_fwd_ws_bytes(N, D, H, W, C, taps))"),
    ("conv_c1.hip", "return g_hooks.conv_impl == 0 && pcrl_to1_brick_eligible(N, D, H, W, C, taps, dtype);"),
    ("conv_to1_brick.hip", "constexpr int TD = 4, TH = 8, TW = 8;"),
    ("conv_to1_brick.hip", "return dtype == PCRL_BF16 && taps == 27 && D % TD == 0 && H % TH == 0 && W % TW == 0 && C % 32 == 0 && C <= 512 &&"),
    ("conv_wgrad.hip", "if (blocks > 16384) blocks = 16384;"),
    ("conv_wgrad.hip", "int64_t blocks = (M * (dtype == PCRL_BF16 ? 4 : 8) + 255) / 256;"),
    ("conv_wgrad.hip", "int blocks = (int)((M + 4095) / 4096);"),
    ("conv_wgrad.hip", "if (blocks > 1024) blocks = 1024;"),
    ("conv_wgrad.hip", "int64_t nb = 512 / ytiles;"),
    ("conv_wgrad.hip", "return dtype == PCRL_BF16 && g_hooks.wgrad_tr && taps == 27 && D % 4 == 0 && H % 8 == 0 && W % 8 == 0 && C % 8 == 0;"),
    ("conv_wgrad.hip", "return taps == 1 && C % (dtype == PCRL_BF16 ? 8 : 4) == 0 && C <= 512 ? SCALAR_WG_POINTWISE : SCALAR_WG_PLAIN;"),
    ("conv_wgrad.hip", "int64_t splits = 512 / tiles;"),
    ("conv_wgrad.hip", "if (splits > (steps + 15) / 16) splits = (steps + 15) / 16;"),
    ("conv_wgrad.hip", "int64_t splits = 2048 / tiles;"),
    ("conv_wgrad.hip", "return g_hooks.wgrad_impl == 0 && dtype == PCRL_BF16 && g_hooks.wgrad_tr && Ci % 64 == 0 && Co % 64 == 0 ? CONVT_WG_ALLTAPS : CONVT_WG_GATHER;"),
    ("conv_up2.hip", "constexpr int UM = 128;"),
    ("conv_up2.hip", "while (mblocks * split < 768 && split * 2 <= ntiles && ntiles % (split * 2) == 0) split *= 2;"),
    ("conv_up2.hip", "return dtype == PCRL_BF16 && (Ci == 128 || Ci == 256 || Ci == 512) && Co % 64 == 0;"),
    ("common.h", "return bytes >= ((int64_t)192 << 20);"),
]


def _tokens(text):
    return re.findall(r"\w+|[^\w\s]", text)


def source_pins_missing():
    """-> the pins whose token sequence does not occur in their file"""
    missing = []
    for f, text in SOURCE_PINS:
        hay, pin = " ".join(_tokens(open(os.path.join(SOURCE, f)).read())), " ".join(_tokens(text))
        if f" {pin} " not in f" {hay} ":
            missing.append((f, text))
    return missing


def vec(dt):
    return 8 if dt == BF16 else 4


def dname(dt):
    return "bf16" if dt == BF16 else "f32"


def voxels(vol):
    N, D, H, W = vol
    return N * D * H * W


def vid(vol):
    return "x".join(str(v) for v in vol)


def is_brick_volume(vol):
    return vol[1] % BRICK[0] == 0 and vol[2] % BRICK[1] == 0 and vol[3] % BRICK[2] == 0


def nbricks(vol):
    return vol[0] * (vol[1] // BRICK[0]) * (vol[2] // BRICK[1]) * (vol[3] // BRICK[2])


# =======================================================================================================================================
# Route mirrors: one-channel convolutions
# =======================================================================================================================================
FWD_GATHER, FWD_FAST, FWD_TWOPASS, FWD_BRICK, FWD_BRICK_PACKED = "gather loop", "gather 1-tap fast path", "two-pass", "brick", "brick + packed image"
WG_PLAIN, WG_BRICK, WG_POINTWISE = 0, 1, 2      # pcrl_conv3d_to1_wgrad_route (ScalarWgradRoute)


def lpv(C, dt):
    """lanes per voxel of to1_fwd_kernel: pow2_floor(C / vec), at most LPV_CAP"""
    p = 1
    while p * 2 <= C // vec(dt):
        p *= 2
    return min(p, LPV_CAP)


def to1_accepts(C, taps, dt):
    """to1_check"""
    return taps in (1, 27) and C > 0 and C % vec(dt) == 0 and C <= 1024 and taps * C * 4 <= LDS_NO_OPT_IN


def to1_brick_eligible(vol, C, taps, dt):
    return dt == BF16 and taps == 27 and is_brick_volume(vol) and C % 32 == 0 and C <= 512 and voxels(vol) < 2 ** 31


def to1_fwd_route(vol, C, taps, dt, ws, conv_impl):
    """pcrl_conv3d_to1_fwd's dispatch"""
    if conv_impl == 0 and to1_brick_eligible(vol, C, taps, dt):
        return FWD_BRICK_PACKED if ws else FWD_BRICK
    if taps == 27 and C % 32 == 0 and voxels(vol) % 4 == 0 and ws:
        return FWD_TWOPASS
    return FWD_FAST if taps == 1 and C // vec(dt) == lpv(C, dt) else FWD_GATHER


def to1_stats_rows(vol, C, taps, dt, conv_impl):
    if conv_impl == 0 and to1_brick_eligible(vol, C, taps, dt):
        return nbricks(vol)
    return -(-voxels(vol) // TO1_VOX)


def dgrad_passes(vol, C, dt):
    """-> (blocks launched, grid-stride passes of the busiest thread) of to1_dgrad_kernel"""
    total = voxels(vol) * (C // vec(dt))
    blocks = min(-(-total // 256), DGRAD_CAP)
    return blocks, -(-total // (blocks * 256))


def scalar_wgrad_route(vol, C, taps, dt, impl, tr):
    if impl != 0:
        return WG_PLAIN
    if dt == BF16 and tr and taps == 27 and is_brick_volume(vol) and C % 8 == 0:
        return WG_BRICK
    return WG_POINTWISE if taps == 1 and C % vec(dt) == 0 and C <= 512 else WG_PLAIN


def scalar_brick_plan(vol, C):
    """scalar_brick_launch -> (bricks per block, blocks used, bricks of the last block)"""
    nb = max(1, min(SCALAR_BRICK_BLOCKS // (-(-C // 64)), nbricks(vol)))
    per = -(-nbricks(vol) // nb)
    blocks = -(-nbricks(vol) // per)
    return per, blocks, nbricks(vol) - (blocks - 1) * per


def plan_splits(M, Cu, Cv, taps):
    """conv_wgrad.hip plan_splits -> (splits, chunk)"""
    tiles = (-(-Cu // 64)) * (-(-Cv // 64)) * taps
    steps = -(-M // 32)
    splits = max(1, min(max(1, 2048 // tiles), -(-steps // 8)))
    per = -(-steps // splits)
    return -(-steps // per), per * 32


def scalar_brick_ws_bytes(vol, C):
    nb = max(1, min(SCALAR_BRICK_BLOCKS // (-(-C // 64)), nbricks(vol)))
    return 8192 + nb * C * 32 * 4


def plain_ws_bytes(M, C, esize):
    return M * 32 * esize + 8192 + plan_splits(M, C, 32, 1)[0] * C * 32 * 4


def im2col_passes(M, dt):
    total = M * (4 if dt == BF16 else 8)
    blocks = min(-(-total // 256), IM2COL_CAP)
    return blocks, -(-total // (blocks * 256))


def vecsum_passes(M):
    blocks = min(-(-M // VECSUM_VOX), VECSUM_CAP)
    return blocks, -(-M // (blocks * 256))


# =======================================================================================================================================
# Route mirrors: transposed convolution
# =======================================================================================================================================
CT_IGEMM, CT_STREAM = 0, 1       # pcrl_convt3d_k2s2_fwd_kernel
CT_WG_GATHER, CT_WG_ALLTAPS = 0, 1      # pcrl_convt3d_k2s2_wgrad_route


def convt_fwd_kernel(Ci, Co, dt, conv_impl):
    return CT_STREAM if conv_impl == 0 and dt == BF16 and Ci in (128, 256, 512) and Co % 64 == 0 else CT_IGEMM


def up2_plan(M, Co):
    """pcrl_convt_up2_launch -> row blocks, splits of the column tiles (grid.y), column tiles per block, column tiles per tap, non-temporal stores"""
    ntiles, mblocks, split = 8 * (Co // 64), -(-M // UP2_ROWS), 1
    while mblocks * split < UP2_FILL and split * 2 <= ntiles and ntiles % (split * 2) == 0:
        split *= 2
    return types.SimpleNamespace(mblocks=mblocks, split=split, tiles_per_block=ntiles // split, ct_per_tap=Co // 64, nt=M * 8 * Co * 2 >= NT_BYTES)


def convt_wgrad_route(Ci, Co, dt, impl, tr):
    return CT_WG_ALLTAPS if impl == 0 and dt == BF16 and tr and Ci % 64 == 0 and Co % 64 == 0 else CT_WG_GATHER


def plan_up2(M, Cu, Cv):
    """conv_wgrad.hip plan_up2 -> (splits, chunk)"""
    tiles = (Cu // 64) * (Cv // 64)
    steps = -(-M // 32)
    splits = max(1, min(max(1, UP2_WG_BLOCKS // tiles), -(-steps // UP2_WG_STEPS)))
    per = -(-steps // splits)
    return -(-steps // per), per * 32


def convt_wgrad_need(M, Ci, Co, route):
    """bytes the route that runs asks for (pcrl_convt3d_k2s2_wgrad_ws_bytes sizes for the larger of the two)"""
    splits = plan_up2(M, Ci, Co)[0] if route == CT_WG_ALLTAPS else plan_splits(M, Ci, Co, 8)[0]
    return splits * 8 * Co * Ci * 4


# =======================================================================================================================================
# Case tables: one-channel forward
# =======================================================================================================================================
V_ODD = (2, 5, 6, 7)             # M = 420: no brick, one block, M % 4 == 0
V_ROW = (2, 5, 6, 4)             # M = 240: one row
V_ROW2 = (1, 3, 20, 18)          # M = 1080: a second row of 56 voxels
V_M105 = (1, 3, 5, 7)            # M = 105: M % 4 != 0
V_BLK2 = (1, 3, 17, 21)          # M = 1071: a second block of 47 voxels, partial groups of the 4-deep unroll
BRICK_VOLS = [(1, 4, 8, 8), (3, 4, 8, 16), (2, 8, 16, 24)]      # one brick; bricks along n and w; along d, h, w

Fwd = collections.namedtuple("Fwd", "vol C taps dt ws impl bias route why")


def _fwd(vol, C, taps, dt, ws=False, impl=0, bias=True, why=""):
    return Fwd(vol, C, taps, dt, ws, impl, bias, to1_fwd_route(vol, C, taps, dt, ws, impl), why)


def fwd_cases():
    c = []
    for dt, C, why in ((BF16, 8, "lpv = 1"), (BF16, 96, "12 vectors over 8 lanes"), (BF16, 520, "lpv capped at 64, one vector left over"),
                       (BF16, 600, "the widest 27-tap layer to1_check accepts: 64 800 bytes of LDS"), (F32, 4, "lpv = 1"),
                       (F32, 260, "lpv capped at 64, one vector left over"), (BF16, 64, ""), (F32, 64, "")):
        c.append(_fwd(V_ODD, C, 27, dt, why=why))
    for dt in (F32, BF16):
        for C in (32, 96, 256):
            c.append(_fwd(V_ROW, C, 27, dt, ws=True, why="one row"))
            c.append(_fwd(V_ROW2, C, 27, dt, ws=True, why="second row of 56 voxels"))
        for C in (64, 96):
            c.append(_fwd(V_ODD, C, 27, dt, ws=True, why="equals the gather kernel at the same C"))
        c.append(_fwd(V_M105, 64, 27, dt, ws=True, why="M % 4 != 0: the gather kernel although a workspace is given"))
    for vol in BRICK_VOLS:
        for C in (32, 96, 128, 160, 512):
            c.append(_fwd(vol, C, 27, BF16, ws=False))
            c.append(_fwd(vol, C, 27, BF16, ws=True, why="packed weight image"))
            c.append(_fwd(vol, C, 27, BF16, ws=True, impl=1, why="conv_impl = 1: the two-pass form on a brick volume"))
    for vol in (V_ROW, V_BLK2):
        for dt, C in ((BF16, 8), (BF16, 64), (BF16, 512), (BF16, 96), (F32, 64), (F32, 12)):
            c.append(_fwd(vol, C, 1, dt))
    c.append(_fwd(V_BLK2, 64, 1, BF16, bias=False, why="bias = NULL"))
    c.append(_fwd(V_ODD, 64, 27, BF16, bias=False, why="bias = NULL"))
    return c


def fwd_id(c):
    return f"{vid(c.vol)}-C{c.C}-t{c.taps}-{dname(c.dt)}-{'ws' if c.ws else 'nows'}-impl{c.impl}" + ("" if c.bias else "-nobias")


# ---- data gradient ----
Dgrad = collections.namedtuple("Dgrad", "vol C taps dt add why")      # add: "none" | "other" | "inplace"
V_DGRAD_CAP = (1, 17, 32, 32)    # M = 17 408: at C = 512 float32, 2 228 224 work items against 8192 * 256 = 2 097 152


def dgrad_cases():
    c = []
    for taps in (27, 1):
        for dt, C in ((BF16, 8), (BF16, 96), (BF16, 520), (F32, 4), (F32, 260)):
            for add in ("none", "other", "inplace"):
                c.append(Dgrad(V_ODD, C, taps, dt, add, ""))
    c.append(Dgrad(V_ODD, 600, 27, BF16, "none", "the widest 27-tap layer to1_check accepts"))
    c.append(Dgrad(V_DGRAD_CAP, 512, 27, F32, "other", "past the 8192-block cap: a second grid-stride pass"))
    return c


def dgrad_id(c):
    return f"{vid(c.vol)}-C{c.C}-t{c.taps}-{dname(c.dt)}-{c.add}"


# ---- weight and bias gradient ----
Wgrad = collections.namedtuple("Wgrad", "vol C taps dt impl tr route why")
V_PER2 = (1, 4, 8, 528)          # 66 bricks over 512 / 8 = 64 blocks at C = 512: two bricks per block, 33 blocks
V_UNEVEN = (1, 4, 8, 520)        # 65 bricks: 33 blocks, the last with one brick
WG_HOOKS = ((0, 1), (1, 1), (0, 0))     # (wgrad impl, tr): defaults, the gather hook, the non-transposed fragment fetch


def _wg(vol, C, taps, dt, impl=0, tr=1, why=""):
    return Wgrad(vol, C, taps, dt, impl, tr, scalar_wgrad_route(vol, C, taps, dt, impl, tr), why)


def wgrad_cases():
    c = []
    for vol, C, why in [((2, 8, 16, 24), C, "24 bricks, one per block") for C in (8, 64, 96, 512)] + [
            (V_PER2, 512, "two bricks per block"), (V_UNEVEN, 512, "uneven last block")]:
        for impl, tr in WG_HOOKS:
            c.append(_wg(vol, C, 27, BF16, impl, tr, why))
        c.append(_wg(vol, C, 27, F32, why=why))
    for C in (8, 64):
        for impl, tr in WG_HOOKS:
            c.append(_wg(V_ODD, C, 27, BF16, impl, tr, "non-brick volume"))
        c.append(_wg(V_ODD, C, 27, F32, why="non-brick volume"))
    for dt in (F32, BF16):
        c.append(_wg(V_ODD, 64, 1, dt, why="1 tap: weighted column sum"))
        c.append(_wg(V_ODD, 64, 1, dt, impl=1, why="1 tap through im2col"))
    return c


def wgrad_id(c):
    return f"{vid(c.vol)}-C{c.C}-t{c.taps}-{dname(c.dt)}-impl{c.impl}-tr{c.tr}"


# ---- past the caps: generated and restated on the device ----
V_DB_CAP = (1, 257, 128, 128)    # M = 4 210 688 > 1024 * 4096: vecsum_partial_kernel strides; taps = 1, C = 8, bf16 -> weighted column sum
V_IM2COL_CAP = (1, 65, 127, 128)        # M = 1 056 640 > 16384 * 256 / 4: im2col27_kernel<bf16> strides; H % 8 != 0 -> im2col route
BIG_WG = [Wgrad(V_DB_CAP, 8, 1, BF16, 0, 1, WG_POINTWISE, "bias gradient past 1024 blocks"),
          Wgrad(V_IM2COL_CAP, 8, 27, BF16, 0, 1, WG_PLAIN, "im2col past 16384 blocks")]


# =======================================================================================================================================
# Case tables: transposed convolution (vol = N, D, H, W of the INPUT)
# =======================================================================================================================================
CT = collections.namedtuple("CT", "vol Ci Co why")
CT_SHAPES = [
    CT((2, 3, 4, 5), 64, 64, "implicit GEMM"),
    CT((3, 2, 2, 2), 32, 32, "implicit GEMM, Ci = 32"),
    CT((1, 3, 5, 7), 96, 32, "implicit GEMM, Co not a multiple of 64"),
    CT((1, 3, 5, 7), 128, 64, "M = 105: one block, wave 3 has 9 valid voxels"),
    CT((2, 5, 6, 7), 256, 128, "M = 420: tail block of 36"),
    CT((1, 3, 3, 3), 512, 192, "split = 8: three column tiles (one tap) per block"),
    CT((3, 5, 11, 13), 128, 64, "M = 2145: weight gradient in five splits with a K tail (M % 32 = 1)"),
]
# restated on the device
CT_BIG = [
    CT((1, 24, 32, 32), 128, 192, "M = 24 576: split = 4, six column tiles per block cross a tap at three tiles per tap"),
    CT((2, 32, 48, 32), 128, 64, "M = 98 304: 768 row blocks, split = 1"),
    CT((3, 32, 64, 32), 128, 64, "M = 196 608: the output is 192 MiB, non-temporal stores"),
    CT((1, 307, 20, 32), 128, 64, "M = 196 480: one row block fewer, plain stores"),
]
CT_WG_SHAPES = [s for s in CT_SHAPES]


def ct_id(s):
    return f"{vid(s.vol)}-{s.Ci}-{s.Co}"


def convt_fwd_runs():
    """(shape, dtype, conv impl, bias)"""
    r = []
    for s in CT_SHAPES:
        for dt in (F32, BF16):
            for impl in ((0, 1) if convt_fwd_kernel(s.Ci, s.Co, dt, 0) == CT_STREAM else (0,)):
                for bias in (True, False):
                    r.append((s, dt, impl, bias))
    return r


def convt_wgrad_runs():
    """(shape, dtype, wgrad impl, tr)"""
    r = []
    for s in CT_WG_SHAPES:
        for impl, tr in WG_HOOKS:
            r.append((s, BF16, impl, tr))
        r.append((s, F32, 0, 1))
    return r


# =======================================================================================================================================
# Lattices and float64 restatements
# =======================================================================================================================================
def lattice_of(name, terms):
    return X.fine_for(terms) if name == "fine" else X.TERNARY


def rows_of(v, brick):
    """[N, 1, D, H, W] -> [rows, voxels of a row]: the voxel set of every statistics row -- the 4x8x8 bricks in the kernel's brick order (n, d / 4,
    h / 8, w / 8), or 1024 consecutive voxels (the last row zero padded)."""
    N, _, D, H, W = v.shape
    if brick:
        bd, bh, bw = BRICK
        return v.view(N, D // bd, bd, H // bh, bh, W // bw, bw).permute(0, 1, 3, 5, 2, 4, 6).reshape(-1, bd * bh * bw)
    flat = v.reshape(-1)
    return F.pad(flat, (0, -flat.numel() % TO1_VOX)).view(-1, TO1_VOX)


@functools.lru_cache(maxsize=None)
def to1_reference(vol, C, taps, lat_name, bias=True):
    """Operands on the lattice; the float64 forward, weight and bias gradient; the preconditions from the same graph on the absolute values,
    asserted here: every caller gets a checked reference.  (The data gradient has its own lattice: to1_dgrad_reference.)"""
    N, D, H, W = vol
    k = 3 if taps == 27 else 1
    lat = lattice_of(lat_name, taps * C)
    g = torch.Generator().manual_seed(N * 7 + D * 5 + H * 3 + W + C + taps + (0 if lat_name == "fine" else 7919))
    x = X.lattice((N, C, D, H, W), *lat["x"], g)
    w = X.lattice((1, C, k, k, k), *lat["w"], g)
    b = X.lattice((1,), *lat["b"], g) if bias else None
    wr = w.clone().requires_grad_(True)
    y = F.conv3d(x, wr, b, padding=k // 2)
    dy = X.lattice(y.shape, *lat["dy"], g)
    y.backward(dy)
    wa = w.abs().requires_grad_(True)
    ya = F.conv3d(x.abs(), wa, None if b is None else b.abs(), padding=k // 2)
    ya.backward(dy.abs())
    u_fwd, u_dw = X.unit(lat["x"][1], lat["w"][1]), X.unit(lat["x"][1], lat["dy"][1])
    R = types.SimpleNamespace(x=x, w=w, b=b, y=y.detach(), dy=dy, dw=wr.grad, db=dy.sum().reshape(1), lat=lat_name, u_fwd=u_fwd,
                              margins={})
    what = f"to1 {vid(vol)} C={C} taps={taps} [{lat_name}]"
    R.margins["fwd"] = X.assert_exactly_summable(ya.detach(), u_fwd, what + " forward")
    R.margins["wgrad"] = X.assert_exactly_summable(wa.grad, u_dw, what + " weight gradient")
    assert torch.equal(R.db.float().double(), R.db), what + ": the bias gradient is not a float32 value"
    for brick in ((False, True) if is_brick_volume(vol) else (False,)):      # per statistics row, for both row layouts the shape can get
        R.margins[f"sum y rows brick={brick}"] = X.assert_exactly_summable(rows_of(R.y.abs(), brick).sum(1), u_fwd, what + f" statistics rows (brick={brick}): sum y")
        if lat_name == "ternary":
            R.margins[f"sum y^2 rows brick={brick}"] = X.assert_exactly_summable(rows_of(R.y * R.y, brick).sum(1), u_fwd * u_fwd,
                                                                               what + f" statistics rows (brick={brick}): sum y^2")
    return R


@functools.lru_cache(maxsize=None)
def to1_dgrad_reference(vol, C, taps):
    """dx[m][c] = add[m][c] + sum_t dy[m - delta_t] w[c][t] in float64.  At most 27 products: on the finer lattice (dy = i/8, w = j/32, add = i/8)
    the sums pass 256 units of 1/256, so a bf16 output is rounded; on the fine one every value would be a bf16 value."""
    N, D, H, W = vol
    k = 3 if taps == 27 else 1
    lat = X.FINER
    g = torch.Generator().manual_seed(N * 7 + D * 5 + H * 3 + W + C + taps + 104729)
    w = X.lattice((1, C, k, k, k), *lat["w"], g)
    dy = X.lattice((N, 1, D, H, W), *lat["dy"], g)
    add = X.lattice((N, C, D, H, W), *lat["x"], g)
    x0 = torch.zeros(N, C, D, H, W, dtype=torch.float64, requires_grad=True)
    F.conv3d(x0, w, None, padding=k // 2).backward(dy)
    xa = torch.zeros(N, C, D, H, W, dtype=torch.float64, requires_grad=True)
    F.conv3d(xa, w.abs(), None, padding=k // 2).backward(dy.abs())
    u = X.unit(lat["dy"][1], lat["w"][1])      # 1/256; the add term's 1/8 is a multiple of it
    R = types.SimpleNamespace(w=w, dy=dy, add=add, dx=x0.grad, dx_add=x0.grad + add)
    R.margin = X.assert_exactly_summable(xa.grad + add.abs(), u, f"to1 dgrad {vid(vol)} C={C} taps={taps}: data gradient + add term")
    return R


def stats_reference(R, brick):
    """-> float64 [rows, 2]: sum y and sum y^2 of every row's own voxel set"""
    return torch.stack([rows_of(R.y, brick).sum(1), rows_of(R.y * R.y, brick).sum(1)], 1)


@functools.lru_cache(maxsize=None)
def convt_reference(vol, Ci, Co):
    """y[n, co, 2d+kd, 2h+kh, 2w+kw] = b[co] + sum_ci x[n, ci, d, h, w] w[ci, co, kd, kh, kw] and its gradients, float64, with the preconditions."""
    N, D, H, W = vol
    lat = X.fine_for(Ci)
    g = torch.Generator().manual_seed(N * 7 + D * 5 + H * 3 + W + Ci * 11 + Co)
    x = X.lattice((N, Ci, D, H, W), *lat["x"], g)
    w = X.lattice((Ci, Co, 2, 2, 2), *lat["w"], g)
    b = X.lattice((Co,), *lat["b"], g)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv_transpose3d(xr, wr, b, stride=2)
    dy = X.lattice(y.shape, *lat["dy"], g)
    y.backward(dy)
    xa, wa = x.abs().requires_grad_(True), w.abs().requires_grad_(True)
    ya = F.conv_transpose3d(xa, wa, b.abs(), stride=2)
    ya.backward(dy.abs())
    y0 = F.conv_transpose3d(x, w, None, stride=2)
    u_fwd, u_dx, u_dw = X.unit(lat["x"][1], lat["w"][1]), X.unit(lat["dy"][1], lat["w"][1]), X.unit(lat["x"][1], lat["dy"][1])
    R = types.SimpleNamespace(x=x, w=w, b=b, y=y.detach(), y_nobias=y0, dy=dy, dx=xr.grad, dw=wr.grad, margins={})
    what = f"convT {vid(vol)} {Ci}->{Co}"
    R.margins["fwd"] = X.assert_exactly_summable(ya.detach(), u_fwd, what + " forward")
    R.margins["dgrad"] = X.assert_exactly_summable(xa.grad, u_dx, what + " data gradient")
    R.margins["wgrad"] = X.assert_exactly_summable(wa.grad, u_dw, what + " weight gradient")
    return R


def worst_units(terms, lat, a, b, extra=None):
    """Analytic bound for the cases restated on the device: `terms` products of the largest magnitudes of operand lattices a and b (plus the largest
    `extra` value), in units of the sum -- holds for every draw."""
    (ma, da), (mb, db_) = lat[a], lat[b]
    m = terms * ma * mb
    if extra:
        me, de = lat[extra]
        assert (da * db_) % de == 0
        m += me * (da * db_ // de)
    return m


def device_lattice(shape, max_int, den, dtype, seed, device):
    """the lattice drawn on the device (the large cases never visit the host)"""
    g = torch.Generator(device=device).manual_seed(seed)
    return (torch.randint(-max_int, max_int + 1, tuple(shape), generator=g, device=device, dtype=torch.int8).to(torch.float32) / den).to(dtype)


# ---- restatements of the large cases: chunked float64 products, on whatever device the operands live on (checked against the CPU references above
# by test_conv1_cases_cpu.py) ----
def chunks(M, step=1 << 16):
    return [(r, min(r + step, M)) for r in range(0, M, step)]


def to1_wgrad_restated(x_rows, dy_vol, taps):
    """x_rows [M, C], dy_vol [D, H, W] (one sample), any float dtype -> (dw float64 [C, taps], db float64 [1]):
    dw[c][t] = sum_m x[m][c] dy[m - delta_t] over the voxels whose neighbour lies inside the volume; db = sum dy"""
    D, H, W = dy_vol.shape
    dy64 = dy_vol.double()
    dw = torch.zeros(x_rows.shape[1], taps, dtype=torch.float64, device=x_rows.device)
    P = F.pad(dy64, (1, 1, 1, 1, 1, 1))
    for t in range(taps):
        kd, kh, kw = (t // 9 - 1, (t // 3) % 3 - 1, t % 3 - 1) if taps == 27 else (0, 0, 0)
        s = P[1 - kd:1 - kd + D, 1 - kh:1 - kh + H, 1 - kw:1 - kw + W].reshape(-1)
        for r0, r1 in chunks(x_rows.shape[0], 1 << 20):
            dw[:, t] += x_rows[r0:r1].double().t() @ s[r0:r1]
    return dw, dy64.sum().reshape(1)


def convt_rows_restated(x_rows, w, b):
    """x_rows [m, Ci], w [Ci, Co, 2, 2, 2], b [Co] or None -> float64 [m, 8, Co]: the eight output voxels (tap = kd * 4 + kh * 2 + kw) of every input voxel"""
    Ci, Co = w.shape[:2]
    y = x_rows.double() @ w.double().permute(0, 2, 3, 4, 1).reshape(Ci, 8 * Co)
    y = y.view(-1, 8, Co)
    return y if b is None else y + b.double().view(1, 1, Co)


def convt_rows_view(y, vol):
    """the transposed convolution's output, logical [N, Co, 2D, 2H, 2W] in NDHWC memory -> [M, 8, Co] in the order of convt_rows_restated (a copy)"""
    N, D, H, W = vol
    Co = y.shape[1]
    return y.permute(0, 2, 3, 4, 1).reshape(N, D, 2, H, 2, W, 2, Co).permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(N * D * H * W, 8, Co)


def convt_rows_unview(rows, vol):
    """the inverse of convt_rows_view: [M, 8, Co] -> the logical [N, Co, 2D, 2H, 2W] tensor in NDHWC memory (a copy)"""
    N, D, H, W = vol
    Co = rows.shape[2]
    return rows.view(N, D, H, W, 2, 2, 2, Co).permute(0, 1, 4, 2, 5, 3, 6, 7).reshape(N, 2 * D, 2 * H, 2 * W, Co).permute(0, 4, 1, 2, 3)


def convt_dgrad_rows_restated(dy_rows, w):
    """dy_rows [m, 8, Co] (convt_rows_view order), w [Ci, Co, 2, 2, 2] -> float64 [m, Ci]: dx[m][ci] = sum over tap and co of dy[m][tap][co] w[ci][co][tap]"""
    Ci, Co = w.shape[:2]
    return dy_rows.reshape(-1, 8 * Co).double() @ w.double().permute(2, 3, 4, 1, 0).reshape(8 * Co, Ci)
