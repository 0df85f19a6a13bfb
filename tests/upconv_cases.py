"""Case table, lattices, float64 references, layout decoders and route mirrors for the composed ConvTranspose3d(k2, s2) -> Conv3d(3x3x3) operator
(pcrl_upconv_*: csrc/upconv_fused.hip with kernels in conv_igemm.hip, conv_brick.hip, conv_brick16_upc.hip, conv_wgrad.hip, wgrad_brick.hip).
Read by test_upconv_cases_cpu.py and test_upconv_exact_gpu.py.  Not a test file.

Method: tests/exact_lattice.py.  The composed weights are sums of products of the two layers' weights, so the operands must keep THEM on a lattice
of bf16 values: the transposed convolution is sparse (one or two non-zero intermediate channels per (input channel, sub-position)), which bounds
every composed weight by a small multiple of the unit.  On top of that x, dy and the biases are lattice values, every product is exact in float32
and every sum stays below 2^24 units of its lattice: a float32 result equals the float64 value, a bf16 result its rounding, at every element,
whatever the order and the split of the sums.

    fine  : x, dy = i/4, |i| <= 4;  w0 = j/8, |j| <= 2;  w_up: two non-zero intermediate channels per (ci, s), values in {+-1, +-1/2};
            b_up, b0 = i/4.  Composed weights are k/16, |k| <= 16 terms * 2 * 2 = 64.  Outputs (unit 1/64) pass 256 units: the bf16 rounding works.
    stats : x = +-1 with half the entries zero; w_up: one non-zero (+-1) intermediate channel per (ci, s); w0 = +-1 with half the entries zero;
            b_up: two non-zero entries (+-1); b0, dy ternary.  Everything is an integer, small enough that sum y^2 over a channel is exact too.
            (A dense b_up alone pushes sum y^2 past 2^24: every fine voxel would carry 27 Cm / 2 bias terms.)

The references are torch autograd of the two aten calls in float64 on the CPU; the composed weights come from the impulse response of those two
calls and the bias table from their response to x = 0 -- not from the (t, s) -> (p, q) tables of the kernel file.  The index algebra used here
(`pq_of_ts`, `e_of_pq`) is derived in the comments from f = 2 v + p alone."""
import collections
import functools
import os
import re
import types

import torch
import torch.nn.functional as F

import exact_lattice as X

F32, BF16 = torch.float32, torch.bfloat16
SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pcrlv2_amd", "csrc")

# ---- lattices: (max_int, den) per operand, `nnz` non-zero intermediate channels of w_up per (ci, s) and their values ----
FINE_UP = dict(name="fine", x=(4, 4), dy=(4, 4), w0=(2, 8), b=(4, 4), nnz=2, up_values=(1.0, -1.0, 0.5, -0.5), up_den=2)
STATS_UP = dict(name="stats", x=(1, 1), dy=(1, 1), w0=(1, 1), b=(1, 1), nnz=1, up_values=(1.0, -1.0), up_den=1)
LATTICES = {"fine": FINE_UP, "stats": STATS_UP}


def units(lat):
    """The unit of every sum of the operator on this lattice"""
    weff = X.unit(lat["up_den"], lat["w0"][1])
    return types.SimpleNamespace(
        weff=weff, y=X.unit(lat["x"][1]) * weff, dx=X.unit(lat["dy"][1]) * weff, dweff=X.unit(lat["x"][1], lat["dy"][1]), box=X.unit(lat["dy"][1]),
        dw0=X.unit(lat["x"][1], lat["dy"][1], lat["up_den"]), dw_up=X.unit(lat["x"][1], lat["dy"][1], lat["w0"][1]), db_up=X.unit(lat["dy"][1], lat["w0"][1]))


# ---- routes (bf16, no hook set; float32 and conv_impl = 1 / wgrad_impl = 1 always take the gather kernels) ----
GATHER, WIDE, WIDE_P, B8, B8_P = "gather", "wide", "wide-perm", "brick8", "brick8-perm"
B8_32, B8_32_P, B8_64 = "brick8-bn32", "brick8-bn32-perm", "brick8-bn64"
WG_GATHER, WG_BRICK, WG_BRICK_P = "gather", "brick", "brick-perm"
CONV_BM = 128            # include/pcrl_hip.h PCRL_CONV_BM: rows of a gather tile = rows of one statistics partial

SOURCE_PINS = [          # (file, source text, compared token by token): a changed routing rule must be noticed by the mirrors below
    ("conv_brick16.h", "constexpr int TD = 4, TH = 8, TW = 16;"),
    ("conv_brick16.h", "if (D % TD == 0 && W % TH == 0 && H % TW == 0) return 2;"),
    ("conv_brick.hip", "constexpr int TD = 4, TH = 8, TW = 8;"),
    ("conv_brick.hip", "static bool brick_permuted(int D, int H, int W) { return W % TD == 0 && D % TH == 0 && H % TW == 0; }"),
    ("conv_brick.hip", "return pcrl_brick_conv_eligible(N, D, H, W, Ci, 8 * Co, dtype) && Co % 64 == 0 && (int64_t)N * D * H * W * 8 < ((int64_t)1 << 29);"),
    ("conv_brick.hip", "const int BN = (Ci % 64 == 0 && bricks * (Ci / 64) > 192) ? 64 : 32;"),
    ("conv_brick16_upc.hip", "return pcrl_brick16_conv_eligible(N, D, H, W, Ci, 8 * Co, dtype) && Co % 64 == 0 && (int64_t)N * D * H * W * 8 < ((int64_t)1 << 29);"),
    ("conv_brick16_upc.hip", "return upc_cshift(Co) >= 0 && Ci % 64 == 0 && pcrl_brick16_conv_eligible(N, D, H, W, 8 * Co, Ci, dtype) && (int64_t)N * D * H * W * 8 < ((int64_t)1 << 29);"),
    ("conv_igemm.hip", "if (blocks >= 512) return SplitPlan{1, steps};"),
    ("conv_igemm.hip", "int splits = (int)((1024 + blocks - 1) / blocks);"),
    ("conv_igemm.hip", "if (splits > steps / 16) splits = steps / 16;"),
    ("wgrad_brick.hip", "constexpr int BD = 2, BH = 8, BW = 8;"),
    ("wgrad_brick.hip", "static bool wb_permuted(int D, int H, int W) { return W % BD == 0 && D % BH == 0 && H % BW == 0; }"),
    ("wgrad_brick.hip", "return pcrl_wgrad_brick_eligible(N, D, H, W, Ci, 8 * Co, dtype) && Co % 64 == 0 && (int64_t)N * D * H * W * 8 * Co < ((int64_t)1 << 31);"),
    ("wgrad_brick.hip", "const int ntile = 4 * (Co / 64) * ((Ci + 63) / 64);"),
    ("wgrad_brick.hip", "int s = 512 / ntile;"),
    ("wgrad_brick.hip", "if (s > nbricks / 16) s = nbricks / 16;"),
    ("upconv_fused.hip", "return g_hooks.wgrad_impl == 0 && g_hooks.wgrad_tr && pcrl_wgrad_brick_upc_eligible(N, D, H, W, Ci, Co, dtype) ? UPC_WG_BRICK : UPC_WG_GATHER;"),
]


def _tokens(text):
    return re.findall(r"\w+|[^\w\s]", text)


def source_has(fname, text):
    with open(os.path.join(SOURCE, fname)) as f:
        hay, needle = _tokens(f.read()), _tokens(text)
    return any(hay[i:i + len(needle)] == needle for i in range(len(hay) - len(needle) + 1))


def _pow2_32(Co):
    return Co >= 32 and Co % 32 == 0 and (Co // 32) & (Co // 32 - 1) == 0


def _wide_perm(D, H, W):
    return 1 if (D % 4 == 0 and H % 8 == 0 and W % 16 == 0) else 2 if (D % 4 == 0 and W % 8 == 0 and H % 16 == 0) else 0


def _b8_perm(D, H, W):
    return 1 if (D % 4 == 0 and H % 8 == 0 and W % 8 == 0) else 2 if (W % 4 == 0 and D % 8 == 0 and H % 8 == 0) else 0


def _wb_perm(D, H, W):
    return 1 if (D % 2 == 0 and H % 8 == 0 and W % 8 == 0) else 2 if (W % 2 == 0 and D % 8 == 0 and H % 8 == 0) else 0


def fwd_route(c, dt=BF16, conv_impl=0):
    if dt != BF16 or conv_impl != 0 or c.Co % 64:
        return GATHER
    w, b = _wide_perm(c.D, c.H, c.W), _b8_perm(c.D, c.H, c.W)
    return (WIDE, WIDE_P)[w - 1] if w else (B8, B8_P)[b - 1] if b else GATHER


def dgrad_route(c, dt=BF16, conv_impl=0):
    if dt != BF16 or conv_impl != 0 or not _pow2_32(c.Co):
        return GATHER
    w, b = _wide_perm(c.D, c.H, c.W), _b8_perm(c.D, c.H, c.W)
    if w and c.Ci % 64 == 0:
        return (WIDE, WIDE_P)[w - 1]
    if not b:
        return GATHER
    bricks = c.N * c.D * c.H * c.W // 256
    if c.Ci % 64 == 0 and bricks * (c.Ci // 64) > 192:
        assert b == 1, "no case reaches the 64-channel tile on permuted axes"
        return B8_64
    return (B8_32, B8_32_P)[b - 1]


def dgrad_splits(c):
    """upc_dgrad_plan of conv_igemm.hip: K splits of the gather data gradient when it is given a workspace (pcrl_upconv_dgrad_ws)"""
    M = c.N * c.D * c.H * c.W
    bn = 128 if c.Ci % 128 == 0 else 64 if c.Ci % 64 == 0 else 32
    blocks, steps = -(-M // CONV_BM) * (c.Ci // bn), 64 * (c.Co // 32)
    if blocks >= 512:
        return 1
    splits = min(-(-1024 // blocks), 16, steps // 16)
    if splits < 2:
        return 1
    per = -(-steps // splits)
    return -(-steps // per)


def wgrad_route(c, dt=BF16, wgrad_impl=0):
    if dt != BF16 or wgrad_impl != 0 or c.Co % 64:
        return WG_GATHER
    b = _wb_perm(c.D, c.H, c.W)
    return (WG_BRICK, WG_BRICK_P)[b - 1] if b else WG_GATHER


def wgrad_brick_splits(c):
    """upc2_plan of wgrad_brick.hip: brick ranges (splits) of the two-phases-per-block kernel"""
    if wgrad_route(c) == WG_GATHER:
        return 1
    nbricks = c.N * c.D * c.H * c.W // 128
    ntile = 4 * (c.Co // 64) * ((c.Ci + 63) // 64)
    s = max(1, min(max(1, 512 // ntile), nbricks // 16))
    if s >= 8:
        s &= ~7
    per = -(-nbricks // s)
    used = -(-nbricks // per)
    return s if (s >= 8 and used & 7) else used


def stats_rows(c, dt=BF16, conv_impl=0):
    r = fwd_route(c, dt, conv_impl)
    M = c.N * c.D * c.H * c.W
    return 8 * (M // 512 if r in (WIDE, WIDE_P) else M // 256 if r in (B8, B8_P) else -(-M // CONV_BM))


def brick_of(route):
    """Brick extents on the tensor a pass WRITES, for assert_bit_equal's messages (forward: fine voxels = 2 x the coarse brick)"""
    return {WIDE: (4, 8, 16), WIDE_P: (4, 16, 8), B8: (4, 8, 8), B8_P: (8, 8, 4), B8_32: (4, 8, 8), B8_32_P: (8, 8, 4), B8_64: (4, 8, 8)}.get(route)


# ---- the cases: N, D, H, W (coarse), Ci, Cm, Co; the kernel each pass runs in bf16 with no hook set; chain: the bf16 chain rule is pinned
#      on the stats lattice (its dWeff passes the bf16 round trip -- asserted, see reference()); stats: the (sum, sum^2) rows of the forward are
#      pinned on the stats lattice (sum |y| and sum y^2 over a whole channel stay below 2^24 -- asserted).  The 25-sample case has neither: with
#      102 400 fine voxels of 256-channel sums per channel its sum y^2 is 1.7e8 on the stats lattice.  It is in the list for the 64-channel tile
#      of the data gradient; its forward runs on the gather kernel, whose statistics rows the four gather cases pin. ----
Case = collections.namedtuple("Case", "N D H W Ci Cm Co fwd dgrad wgrad chain stats why")
CASES = [
    # gather kernels (conv_igemm.hip GEOM_UPC_FWD / GEOM_UPC_DGRAD, conv_wgrad.hip)
    Case(2, 3, 4, 5, 32, 32, 32, GATHER, GATHER, WG_GATHER, True, True, "odd extents: 120 rows of a 128-row tile"),
    Case(1, 1, 1, 1, 32, 64, 32, GATHER, GATHER, WG_GATHER, True, True, "one coarse voxel: every fine voxel is a corner"),
    Case(2, 1, 2, 3, 64, 32, 64, GATHER, GATHER, WG_GATHER, True, True, "fine extent 2 along d: first and last class only"),
    Case(3, 2, 2, 2, 64, 64, 32, GATHER, GATHER, WG_GATHER, True, True, "split-K data gradient with its finish pass"),
    # wide brick (conv_brick16_upc.hip), forward and data gradient
    Case(1, 4, 8, 16, 64, 64, 64, WIDE, WIDE, WG_BRICK, True, True, "one wide brick: every border class on its faces"),
    Case(1, 4, 16, 8, 64, 64, 64, WIDE_P, WIDE_P, WG_BRICK, True, True, "wide brick along (D, W, H)"),
    Case(1, 4, 8, 16, 32, 32, 128, WIDE, B8_32, WG_BRICK, True, True, "two 64-channel tiles per phase; Ci = 32 sends the data gradient to the 4x8x8 brick"),
    Case(1, 4, 8, 16, 64, 64, 32, GATHER, WIDE, WG_GATHER, True, True, "Co = 32: one 32-channel chunk per parity, forward on the gather kernel"),
    Case(1, 4, 8, 16, 64, 64, 128, WIDE, WIDE, WG_BRICK, True, True, "Co = 128: four chunks per parity"),
    # 4 x 8 x 8 brick (conv_brick.hip composed modes)
    Case(1, 8, 8, 8, 64, 64, 64, B8, B8_32, WG_BRICK, True, True, "two bricks along d"),
    Case(1, 8, 8, 4, 64, 64, 64, B8_P, B8_32_P, WG_BRICK_P, True, True, "brick axes (W, D, H)"),
    Case(1, 16, 8, 4, 64, 32, 32, GATHER, B8_32_P, WG_GATHER, True, True, "Co = 32: 32-channel data-gradient tiles on permuted axes"),
    Case(25, 8, 8, 8, 256, 32, 32, GATHER, B8_64, WG_GATHER, False, False, "bricks * Ci / 64 = 200 > 192: the 64-channel data-gradient tile"),
    # brick weight gradient (wgrad_brick.hip composed mode)
    Case(1, 2, 8, 8, 64, 64, 64, GATHER, GATHER, WG_BRICK, True, True, "one weight-gradient brick"),
    Case(1, 8, 8, 2, 64, 64, 64, GATHER, GATHER, WG_BRICK_P, True, True, "weight-gradient brick axes (W, D, H)"),
    Case(3, 2, 8, 8, 32, 64, 64, GATHER, GATHER, WG_BRICK, True, True, "Ci = 32 tiles"),
    Case(1, 2, 8, 16, 64, 64, 128, GATHER, GATHER, WG_BRICK, True, True, "two 64-channel tiles inside a phase"),
    # upc2_plan: s = min(512 / ntile, nbricks / 16) in integer division, so a second split needs nbricks >= 32 bricks of 2 x 8 x 8 = 4096 coarse
    # voxels whatever the channels; Ci = 32, Cm = 32, Co = 64 are the smallest channels the brick route takes (ntile = 4 <= 256).  16^3 = 4096.
    Case(1, 16, 16, 16, 32, 32, 64, WIDE, B8_32, WG_BRICK, True, True, "the smallest shape with two brick ranges in the weight gradient"),
]
SPLIT_WGRAD_CASE = CASES[-1]
SPLITK_DGRAD_CASE = CASES[3]


def case_id(c):
    return "x".join(str(v) for v in c[:7])


def dname(dt):
    return "bf16" if dt == BF16 else "f32"


# ---- index algebra, from f = 2 v + p alone ----
# Per axis a fine voxel f = 2 v + p (phase p) reads up[f + t - 1] through tap t of the 3-tap window; up[g] with g = 2 u + s was written from x[u]
# through sub-position s of the transposed convolution.  g = 2 v + p + t - 1 gives s = (p + t - 1) mod 2 and u = v + floor((p + t - 1) / 2); the
# composed operator names that coarse voxel u = v + p - 1 + q, so q = floor((p + t - 1) / 2) - p + 1.  Given (t, s): p = (s - t + 1) mod 2.
def pq_of_ts(t, s):
    p = (s - t + 1) % 2
    return p, (p + t - 1) // 2 - p + 1


# The data gradient of coarse voxel u reads the fine voxels g = 2 u - 1 + e, e = 0..3: with g = 2 v + p and u = v + p - 1 + q, e = 3 - p - 2 q.
def e_of_pq(p, q):
    return 3 - p - 2 * q


def _axes(i):
    return (i >> 2) & 1, (i >> 1) & 1, i & 1


def ts_pairs(p, q):
    """(t, s) triples -- t = 0..26, s = 0..7 -- that lead from offset q to phase p (p, q = 0..7)"""
    out = []
    for t in range(27):
        for s in range(8):
            ta, sa = (t // 9, (t // 3) % 3, t % 3), _axes(s)
            if all(pq_of_ts(ta[k], sa[k]) == (_axes(p)[k], _axes(q)[k]) for k in range(3)):
                out.append((t, s))
    return out


def compose_from_pairs(w_up, w0, pairs=None):
    """Weff[p][q][ci][co] = sum over the (t, s) of (p, q) of sum_cm w_up[ci][cm][s] w0[co][cm][t]; `pairs`: {(p, q): [(t, s)]} overrides"""
    Ci, Cm = w_up.shape[:2]
    Co = w0.shape[0]
    wu, wc = w_up.reshape(Ci, Cm, 8), w0.reshape(Co, Cm, 27)
    out = torch.zeros(8, 8, Ci, Co, dtype=torch.float64)
    for p in range(8):
        for q in range(8):
            for t, s in (pairs or {}).get((p, q), ts_pairs(p, q)):
                out[p, q] += wu[:, :, s] @ wc[:, :, t].t()
    return out


# ---- layouts of include/pcrl_hip.h <-> Weff[p][q][ci][co] ----
def _e_index(p, q):
    return sum(e_of_pq(_axes(p)[k], _axes(q)[k]) << (4 - 2 * k) for k in range(3))


def encode_wf(weff):                 # [8][Co][8][Ci]
    return weff.permute(0, 3, 1, 2).contiguous()


def decode_wf(wf, Ci, Co):
    return wf.reshape(8, Co, 8, Ci).permute(0, 2, 3, 1).contiguous()


def encode_wd(weff):                 # [Ci][64][Co], e = fine offset triple
    Ci, Co = weff.shape[2:]
    out = torch.zeros(Ci, 64, Co, dtype=weff.dtype)
    for p in range(8):
        for q in range(8):
            out[:, _e_index(p, q)] = weff[p, q]
    return out


def decode_wd(wd, Ci, Co):
    wd = wd.reshape(Ci, 64, Co)
    return torch.stack([torch.stack([wd[:, _e_index(p, q)] for q in range(8)]) for p in range(8)])


def _tap3(p, q):                     # the zero-embedded forward form: tap = p + q per axis
    return sum((_axes(p)[k] + _axes(q)[k]) * (9, 3, 1)[k] for k in range(3))


def encode_w3f(weff):                # [8 * Co][27][Ci], zero outside a phase's eight taps
    Ci, Co = weff.shape[2:]
    out = torch.zeros(8, Co, 27, Ci, dtype=weff.dtype)
    for p in range(8):
        for q in range(8):
            out[p, :, _tap3(p, q)] = weff[p, q].t()
    return out.reshape(8 * Co, 27, Ci)


def decode_w3f(w3f, Ci, Co):
    """-> (Weff, the entries outside the embedded taps)"""
    w = w3f.reshape(8, Co, 27, Ci)
    rest = w.clone()
    for p in range(8):
        for q in range(8):
            rest[p, :, _tap3(p, q)] = 0
    return torch.stack([torch.stack([w[p, :, _tap3(p, q)].t() for q in range(8)]) for p in range(8)]), rest


def _kpar(p, q):                     # space-to-depth view of dy0: g = 2 u - 1 + e = 2 (u + k - 1) + par, so e + 1 = 2 k + par per axis
    e = [e_of_pq(_axes(p)[k], _axes(q)[k]) for k in range(3)]
    return sum(((e[k] + 1) >> 1) * (9, 3, 1)[k] for k in range(3)), sum(((e[k] + 1) & 1) << (2 - k) for k in range(3))


def encode_wd3(weff):                # [Ci][27][8 * Co], channel = parity * Co + co
    Ci, Co = weff.shape[2:]
    out = torch.zeros(Ci, 27, 8, Co, dtype=weff.dtype)
    for p in range(8):
        for q in range(8):
            k, par = _kpar(p, q)
            out[:, k, par] = weff[p, q]
    return out.reshape(Ci, 27, 8 * Co)


def decode_wd3(wd3, Ci, Co):
    w = wd3.reshape(Ci, 27, 8, Co)
    rest = w.clone()
    for p in range(8):
        for q in range(8):
            k, par = _kpar(p, q)
            rest[:, k, par] = 0
    return torch.stack([torch.stack([w[:, _kpar(p, q)[0], _kpar(p, q)[1]] for q in range(8)]) for p in range(8)]), rest


def encode_dweff(dweff):             # [Co][Ci][64], index p * 8 + q
    Ci, Co = dweff.shape[2:]
    return dweff.permute(3, 2, 0, 1).reshape(Co, Ci, 64).contiguous()


def decode_dweff(acc, Ci, Co):
    return acc.reshape(Co, Ci, 8, 8).permute(2, 3, 1, 0).contiguous()


# ---- operands ----
def _signs(shape, g):
    return (torch.randint(0, 2, tuple(shape), generator=g) * 2 - 1).double()


def _half_zero(shape, g):
    return _signs(shape, g) * (torch.rand(tuple(shape), generator=g) < 0.5).double()


def sparse_up(Ci, Cm, lat, g):
    """w_up [Ci][Cm][2][2][2] with exactly lat['nnz'] non-zero intermediate channels per (ci, s)"""
    nnz, vals = lat["nnz"], torch.tensor(lat["up_values"], dtype=torch.float64)
    idx = torch.rand(Ci, 8, Cm, generator=g).topk(nnz, dim=2).indices
    w = torch.zeros(Ci, 8, Cm, dtype=torch.float64).scatter_(2, idx, vals[torch.randint(0, len(vals), (Ci, 8, nnz), generator=g)])
    assert int((w != 0).sum()) == Ci * 8 * nnz
    return w.permute(0, 2, 1).reshape(Ci, Cm, 2, 2, 2).contiguous()


def weights(Ci, Cm, Co, lat_name, seed):
    lat, g = LATTICES[lat_name], torch.Generator().manual_seed(seed)
    w_up = sparse_up(Ci, Cm, lat, g)
    if lat_name == "fine":
        w0 = X.lattice((Co, Cm, 3, 3, 3), *lat["w0"], g)
        b_up, b0 = X.lattice((Cm,), *lat["b"], g), X.lattice((Co,), *lat["b"], g)
    else:
        w0 = _half_zero((Co, Cm, 3, 3, 3), g)
        b_up = torch.zeros(Cm, dtype=torch.float64)
        b_up[torch.randperm(Cm, generator=g)[:2]] = _signs((2,), g)
        b0 = X.lattice((Co,), *lat["b"], g)
    return w_up, b_up, w0, b0


def zero_sum_dy(shape, lat, g):
    """dy [N][Co][FD][FH][FW] whose sum over (n, voxels) is exactly zero per channel: the second half of a channel's voxels is the negated
    permutation of the first half"""
    N, Co = shape[:2]
    vox = shape[2] * shape[3] * shape[4]
    half = N * vox // 2
    a = X.lattice((Co, half), *lat["dy"], g)
    flat = pz(torch.cat([a, -a[:, torch.randperm(half, generator=g)]], dim=1))        # [Co][N * vox]
    dy = flat.reshape(Co, N, *shape[2:]).permute(1, 0, 2, 3, 4).contiguous()
    assert bool((dy.sum((0, 2, 3, 4)) == 0).all())
    return dy


# ---- float64 references ----
def pz(t):
    """Zeros of either sign -> +0.  A reference sum of one term (one coarse voxel, one voxel of a border class) can be 0 * (-a) = -0, while an
    accumulator that starts at +0 -- every kernel's -- ends at +0: the sign of a zero sum is the reference's artefact, and the bit comparison
    would report it.  After this a kernel that writes -0 is still reported."""
    return t + 0.0


def two_calls(x, w_up, b_up, w0, b0):
    return F.conv3d(F.conv_transpose3d(x, w_up, b_up, stride=2), w0, b0, padding=1)


def impulse_weff(w_up, w0):
    """Weff[p][q][ci][co] from the two aten calls: a one-hot coarse voxel at the centre c = 1 of a 3^3 grid, one input channel per batch entry, no
    biases.  x[v + p - 1 + q] is the impulse for v = 2 - p - q, so the weight appears at the fine voxel 2 v + p = 4 - p - 2 q (per axis)."""
    Ci, Co = w_up.shape[0], w0.shape[0]
    x = torch.zeros(Ci, Ci, 3, 3, 3, dtype=torch.float64)
    x[torch.arange(Ci), torch.arange(Ci), 1, 1, 1] = 1
    y = two_calls(x, w_up, None, w0, None)                # [Ci][Co][6][6][6]
    f = lambda p, q, k: 4 - _axes(p)[k] - 2 * _axes(q)[k]
    return torch.stack([torch.stack([y[:, :, f(p, q, 0), f(p, q, 1), f(p, q, 2)] for q in range(8)]) for p in range(8)])


def impulse_bias_tab(w_up, b_up, w0, b0):
    """bias_tab[27][Co] from the two aten calls on x = 0 over a 2^3 coarse grid: fine voxel 0 is of the first class, 1 of the inside one, 3 of the last"""
    y = two_calls(torch.zeros(1, w_up.shape[0], 2, 2, 2, dtype=torch.float64), w_up, b_up, w0, b0)[0]      # [Co][4][4][4]
    at = (0, 1, 3)
    return torch.stack([y[:, at[c // 9], at[(c // 3) % 3], at[c % 3]] for c in range(27)])


def classes(F_):
    """border class of each fine index along an axis of extent F_: 0 first, 1 inside, 2 last"""
    c = torch.ones(F_, dtype=torch.long)
    c[0], c[-1] = 0, 2
    return c


def class_map(D, H, W):
    cd, ch, cw = classes(2 * D), classes(2 * H), classes(2 * W)
    return cd.view(-1, 1, 1) * 9 + ch.view(1, -1, 1) * 3 + cw.view(1, 1, -1)


def composed_forward(x, weff, bias_tab, cls=None):
    """y[2 v + p] = bias_tab[class] + sum_q x[v + p - 1 + q] Weff[p][q] on the zero-padded coarse grid"""
    N, Ci, D, H, W = x.shape
    Co = weff.shape[3]
    xp = F.pad(x, (1, 1, 1, 1, 1, 1))
    y = torch.zeros(N, Co, 2 * D, 2 * H, 2 * W, dtype=torch.float64)
    for p in range(8):
        pa = _axes(p)
        acc = 0
        for q in range(8):
            o = [pa[k] + _axes(q)[k] for k in range(3)]             # v + p - 1 + q, + 1 for the padding
            acc = acc + torch.einsum("nidhw,io->nodhw", xp[:, :, o[0]:o[0] + D, o[1]:o[1] + H, o[2]:o[2] + W], weff[p, q])
        y[:, :, pa[0]::2, pa[1]::2, pa[2]::2] = acc
    cls = class_map(D, H, W) if cls is None else cls
    return y + bias_tab[cls].permute(3, 0, 1, 2).unsqueeze(0)


def dweff_of(x, dy):
    """dWeff[p][q][ci][co] = sum_v x[v + p - 1 + q][ci] dy[2 v + p][co]: shifted slices of the zero-padded x against the stride-2 phases of dy"""
    N, Ci, D, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1, 1, 1))
    out = torch.zeros(8, 8, Ci, dy.shape[1], dtype=torch.float64)
    for p in range(8):
        pa = _axes(p)
        dp = dy[:, :, pa[0]::2, pa[1]::2, pa[2]::2]
        for q in range(8):
            o = [pa[k] + _axes(q)[k] for k in range(3)]
            out[p, q] = torch.einsum("nidhw,nodhw->io", xp[:, :, o[0]:o[0] + D, o[1]:o[1] + H, o[2]:o[2] + W], dp)
    return pz(out)


def box_of(dy, zero_sum=False):
    """box[t][co] = sum of dy over the fine voxels from which tap t stays inside the grid.  zero_sum: the sum over the voxels of the fully interior
    class is taken as minus the sum over all others, as the kernel does under flags bit 1."""
    FD, FH, FW = dy.shape[2:]
    if zero_sum:
        cls = class_map(FD // 2, FH // 2, FW // 2)
        S = torch.stack([(dy * (cls == c)).sum((0, 2, 3, 4)) for c in range(27)])
        S[13] = -(S.sum(0) - S[13])
        inside = lambda t, c: not (t == 0 and c == 0) and not (t == 2 and c == 2)
        return pz(torch.stack([sum(S[c] for c in range(27) if inside(t // 9, c // 9) and inside((t // 3) % 3, (c // 3) % 3) and inside(t % 3, c % 3))
                               for t in range(27)]))
    sl = lambda k, n_: slice(max(0, -k), n_ - max(0, k))
    return pz(torch.stack([dy[:, :, sl(t // 9 - 1, FD), sl((t // 3) % 3 - 1, FH), sl(t % 3 - 1, FW)].sum((0, 2, 3, 4)) for t in range(27)]))


def chain_rule(dweff, box, w_up, b_up, w0):
    """-> (dw_up, db_up, dw0) from the gradient of the composed weights and the box sums (float64)"""
    Ci, Cm = w_up.shape[:2]
    Co = w0.shape[0]
    wu, wc = w_up.reshape(Ci, Cm, 8), w0.reshape(Co, Cm, 27)
    dw_up, dw0 = torch.zeros_like(wu), torch.zeros_like(wc)
    for p in range(8):
        for q in range(8):
            for t, s in ts_pairs(p, q):
                dw0[:, :, t] += dweff[p, q].t() @ wu[:, :, s]           # [Co][Ci] x [Ci][Cm]
                dw_up[:, :, s] += dweff[p, q] @ wc[:, :, t]             # [Ci][Co] x [Co][Cm]
    dw0 += b_up.view(1, Cm, 1) * box.t().unsqueeze(1)                   # box [27][Co] -> [Co][1][27]
    db_up = torch.einsum("omt,to->m", wc, box)
    return pz(dw_up.reshape(w_up.shape)), pz(db_up), pz(dw0.reshape(w0.shape))


def _seed(c, lat_name):
    return c.N * 7 + c.D * 5 + c.H * 3 + c.W + c.Ci + 2 * c.Cm + 3 * c.Co + (0 if lat_name == "fine" else 7919)


@functools.lru_cache(maxsize=None)
def reference(c, lat_name):
    """Operands on the lattice, the float64 references and every precondition (asserted: a violation is an error of the case list).  R.headroom:
    {name: largest sum of |terms| as a fraction of 2^24}."""
    lat, u = LATTICES[lat_name], units(LATTICES[lat_name])
    w_up, b_up, w0, b0 = weights(c.Ci, c.Cm, c.Co, lat_name, _seed(c, lat_name))
    g = torch.Generator().manual_seed(_seed(c, lat_name) + 1)
    shape_x, shape_y = (c.N, c.Ci, c.D, c.H, c.W), (c.N, c.Co, 2 * c.D, 2 * c.H, 2 * c.W)
    x = _half_zero(shape_x, g) if lat_name == "stats" else X.lattice(shape_x, *lat["x"], g)
    dy = X.lattice(shape_y, *lat["dy"], g)
    leaves = [t.clone().requires_grad_(True) for t in (x, w_up, b_up, w0)]
    y = two_calls(leaves[0], leaves[1], leaves[2], leaves[3], b0)
    y.backward(dy)
    ab = [t.abs().requires_grad_(True) for t in (x, w_up, b_up, w0)]
    ya = two_calls(ab[0], ab[1], ab[2], ab[3], b0.abs())
    ya.backward(dy.abs())
    weff, tab = impulse_weff(w_up, w0), impulse_bias_tab(w_up, b_up, w0, b0)
    dweff, dweff_abs = dweff_of(x, dy), dweff_of(x.abs(), dy.abs())
    R = types.SimpleNamespace(case=c, lat=lat_name, u=u, x=x, dy=dy, w_up=w_up, b_up=b_up, w0=w0, b0=b0, y=pz(y.detach()), dx=pz(leaves[0].grad), dw_up=pz(leaves[1].grad),
                              db_up=pz(leaves[2].grad), dw0=pz(leaves[3].grad), weff=weff, bias_tab=tab, dweff=dweff, dweff_abs=dweff_abs, box=box_of(dy),
                              box_abs=dy.abs().sum((0, 2, 3, 4)), y_abs=ya.detach(), sum_y=y.detach().sum((0, 2, 3, 4)),
                              sum_y2=(y.detach() ** 2).sum((0, 2, 3, 4)))
    what = f"{case_id(c)} [{lat_name}]"
    h = R.headroom = {}
    h["forward"] = X.assert_exactly_summable(R.y_abs, u.y, what + " forward")
    h["data gradient"] = X.assert_exactly_summable(ab[0].grad, u.dx, what + " data gradient")
    h["dWeff"] = X.assert_exactly_summable(dweff_abs, u.dweff, what + " gradient of the composed weights")
    h["box"] = X.assert_exactly_summable(R.box_abs, u.box, what + " box sums: sum |dy| per channel")
    # The chain rule starts from FINISHED values of dWeff and of the box sums (both exact by the two preconditions above), so the terms of its
    # sums are dWeff * w and w0 * box: the absolute-value graph of that stage.
    ca = chain_rule(dweff.abs(), R.box.abs(), w_up.abs(), b_up.abs(), w0.abs())
    h["chain rule dw_up"] = X.assert_exactly_summable(ca[0], u.dw_up, what + " chain rule product dWeff * w0")
    h["chain rule dw0"] = X.assert_exactly_summable(ca[2], u.dw0, what + " chain rule product dWeff * w_up (+ b_up * box)")
    h["db_up"] = X.assert_exactly_summable(ca[1], u.db_up, what + " db_up: sum |w0| |box|")
    assert torch.equal(weff.to(BF16).double(), weff), what + ": a composed weight is not a bf16 value"
    assert float(weff.abs().max()) / u.weff <= 64
    if lat_name == "stats" and c.stats:
        h["sum |y|"] = X.assert_exactly_summable(R.y.abs().sum((0, 2, 3, 4)), u.y, what + " statistics: sum |y| over the channel")
        h["sum y^2"] = X.assert_exactly_summable(R.sum_y2, u.y * u.y, what + " statistics: sum y^2 over the channel")
    if lat_name == "stats" and c.chain:     # upc_chain_pack_kernel<bf16> rounds dWeff to bf16 before the chain-rule GEMMs
        assert torch.equal(dweff.to(BF16).double(), dweff), what + ": dWeff is not a bf16 value (max |dWeff| = %g): not a bf16 chain-rule case" % float(dweff.abs().max())
    R.chain_bf16 = lat_name == "stats" and c.chain
    return R


@functools.lru_cache(maxsize=None)
def zero_sum_reference(c, lat_name):
    """The same x with a zero-sum dy: dWeff and the box sums (both ways: they agree exactly on this dy)"""
    R, lat = reference(c, lat_name), LATTICES[lat_name]
    g = torch.Generator().manual_seed(_seed(c, lat_name) + 2)
    dy = zero_sum_dy(R.dy.shape, lat, g)
    Z = types.SimpleNamespace(dy=dy, dweff=dweff_of(R.x, dy), box=box_of(dy), box_zs=box_of(dy, zero_sum=True))
    what = f"{case_id(c)} [{lat_name}] zero-sum dy"
    X.assert_exactly_summable(dweff_of(R.x.abs(), dy.abs()), R.u.dweff, what + " gradient of the composed weights")
    X.assert_exactly_summable(dy.abs().sum((0, 2, 3, 4)), R.u.box, what + " box sums: sum |dy| per channel")
    return Z


# ---- run lists of the GPU tests ----
ACCUM_CASES = [c for c in CASES if c.N * c.D * c.H * c.W <= 4096]          # every case but the 25-sample one (it is there for the data-gradient tile)


def fwd_runs():
    """(case, dtype, conv_impl): float32 once (always the gather kernels), bf16 under the default route and under conv_impl = 1"""
    out = []
    for c in CASES:
        out.append((c, F32, 0))
        out.append((c, BF16, 0))
        if (c.fwd, c.dgrad) != (GATHER, GATHER):
            out.append((c, BF16, 1))
    return out


def wgrad_runs():
    """(case, dtype, wgrad_impl)"""
    out = []
    for c in ACCUM_CASES:
        out.append((c, F32, 0))
        out.append((c, BF16, 0))
        if c.wgrad != WG_GATHER:
            out.append((c, BF16, 1))
    return out


def run_id(r):
    return f"{case_id(r[0])}-{dname(r[1])}-impl{r[2]}"


# the (pass, route) pairs the run lists must reach (asserted on the CPU from the mirrors and on the GPU from the library's answers)
EXPECTED_REACHED = {("fwd", r) for r in (GATHER, WIDE, WIDE_P, B8, B8_P)} | \
                   {("dgrad", r) for r in (GATHER, "gather-splitk", WIDE, WIDE_P, B8_32, B8_32_P, B8_64)} | \
                   {("wgrad", r) for r in (WG_GATHER, WG_BRICK, WG_BRICK_P, "brick-splits")}


def reached_from_mirrors():
    got = set()
    for c, dt, impl in fwd_runs():
        got.add(("fwd", fwd_route(c, dt, impl)))
        d = dgrad_route(c, dt, impl)
        got.add(("dgrad", d))
        if d == GATHER and dgrad_splits(c) > 1:
            got.add(("dgrad", "gather-splitk"))
    for c, dt, impl in wgrad_runs():
        w = wgrad_route(c, dt, impl)
        got.add(("wgrad", w))
        if w != WG_GATHER and wgrad_brick_splits(c) > 1:
            got.add(("wgrad", "brick-splits"))
    return got


def case_table():
    """Markdown: per case the kernel each pass runs in bf16 with no hook set, and per lattice the headroom of each precondition -- the largest sum of
    |terms| as a fraction of 2^24, from the float64 reference (docs/upconv_exact_cases.md; `python tests/upconv_cases.py` prints it)"""
    keys = ["forward", "data gradient", "dWeff", "box", "chain rule dw_up", "chain rule dw0", "db_up", "sum |y|", "sum y^2"]
    lines = ["| case (N D H W Ci Cm Co) | forward | data gradient (workspace form) | weight gradient | lattice | " + " | ".join(keys) + " |",
             "|---|---|---|---|---|" + "---|" * len(keys)]
    for c in CASES:
        for lat in ("fine", "stats"):
            R = reference(c, lat)
            d = c.dgrad + (f", {dgrad_splits(c)} K splits" if c.dgrad == GATHER and dgrad_splits(c) > 1 else "")
            w = c.wgrad + (f", {wgrad_brick_splits(c)} range(s)" if c.wgrad != WG_GATHER else "")
            cells = [("%.2g" % R.headroom[k]) if k in R.headroom else "-" for k in keys]
            lines.append(f"| {' '.join(map(str, c[:7]))} | {c.fwd} | {d} | {w} | {lat} | " + " | ".join(cells) + " |")
    return "\n".join(lines)


if __name__ == "__main__":
    print(case_table())
