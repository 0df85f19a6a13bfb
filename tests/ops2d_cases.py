"""Case table, lattices and float64 restatements for the HBM-bound passes of the 2D path: csrc/encoder2d.hip, csrc/ops2d.hip and
csrc/heads2d.hip (test_ops2d_cases_cpu.py, test_ops2d_exact_gpu.py).  Not a test file.

Operands sit on a dyadic lattice (activations and gradients i/4, coefficients j/4 or j/8), so every float32 product and sum of these
kernels is exact in any order and under any contraction, and an output must equal the float64 value (float32 outputs) or its
round-to-nearest-even rounding to bf16 at EVERY element.  Where a kernel places a rounding on purpose the restatement places the same one
(`mid=True`, `pre=True`, `k32=True`) and the CPU test shows that the case's inputs tell the two apart:
  bn_add_relu        t = T(scale y + shift) and i = T(rscale r + rshift) are rounded to the storage type before the addition
  bn_relu_maxpool    the argmax is taken on T(relu(scale y + shift))
  maxpool_bwd_sum    T(dy + dy2) is rounded before it is accumulated
  mse2d_bwd_pad      g = dloss * (float)(2.0 / (M C)) in float32, ONE float32 product g * (p - gt), then the rounding to T
  mse2d_fwd          (float)(sum * (1.0 / (M C))) in float64
The restatements work on CPU and device tensors alike; the large cases never leave the device.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import norm_pool_cases as npc
from norm_pool_cases import BF16, F32, GRID_CAP, NT_BYTES, esize, lat, nslots, rc_blocks, streaming, vec  # noqa: F401

RC_CAP = npc.RC_CAP
CAP_ITEMS = npc.CAP_ITEMS            # 4 194 304 work items in one pass of a grid_for() launch
ROWS_PER_BLOCK = 1024                # heads2d.hip: pixels per first-stage block
PAD_CAP = 65536                      # pcrl_nchw_to_nhwc_pad: blocks
ADD_CAP = 4096                       # pcrl_add_f32: blocks (pinned by test_step_tail_gpu.py; its constant is read here with the others)
FINISH_LEAD = 768                    # mse2d_finish_kernel: four partials in flight while i + 768 < blocks

SOURCE_PINS = [
    ("encoder2d.hip", "if (b > 2048) b = 2048;"),
    ("encoder2d.hip", "return (unsigned)(b < 1 ? 1 : (b > 16384 ? 16384 : b));"),
    ("encoder2d.hip", "#pragma unroll 4 for (int64_t m = (int64_t)blockIdx.x * nslots + slot; m < M; m += stride)"),
    ("ops2d.hip", "return (unsigned)(b < 1 ? 1 : (b > 16384 ? 16384 : b));"),
    ("heads2d.hip", "constexpr int ROWS_PER_BLOCK = 1024;"),
    ("heads2d.hip", "if (b > 65536) b = 65536;"),
    ("heads2d.hip", "if (blocks > 4096) blocks = 4096;"),
    ("heads2d.hip", "for (; i + 768 < blocks; i += 1024)"),
    ("heads2d.hip", "#pragma unroll 2 for (int64_t m = beg + slot; m < end; m += nslots)"),
    ("common.h", "return bytes >= ((int64_t)192 << 20);"),
]


def source_pins_hold(pins=None, read=npc.read_source):
    """-> the pins whose token sequence does not occur in their file (norm_pool_cases' tokenizer: spacing and line breaks do not matter)"""
    missing = []
    for f, text in (SOURCE_PINS if pins is None else pins):
        hay, pin = " ".join(npc._tokens(read(f))), " ".join(npc._tokens(text))
        if f" {pin} " not in f" {hay} ":
            missing.append((f, text))
    return missing


def rows1024(M):
    return -(-M // ROWS_PER_BLOCK)


def pool_out(h):
    return (h + 2 - 3) // 2 + 1


# ---------------------------------------------------------------------------------------------------------------------------------------
# lattices
# ---------------------------------------------------------------------------------------------------------------------------------------
Y_INT, SC_INT, SH_INT = 8, 40, 16          # y, r = i/4; scale, rscale = j/4 (up to 10); shift, rshift = j/8


class Coef2:
    """scale, shift, rscale, rshift: float32 [C] on `device`, lattice values; no scale is zero"""

    def __init__(self, C, seed, device):
        g = torch.Generator().manual_seed(seed)

        def ri(m):
            return torch.randint(-m, m + 1, (C,), generator=g).double()

        for k, m, den in (("scale", SC_INT, 4), ("shift", SH_INT, 8), ("rscale", SC_INT, 4), ("rshift", SH_INT, 8)):
            v = ri(m)
            if den == 4:
                v[v == 0] = 1.0
            setattr(self, k, (v / den).float().to(device).contiguous())


def wide_pair(shape, dt, seed, device):
    """(da, db): da = i/4 with |i| <= 127 and db = 4 k with |k| <= 127, both bf16 values; da + db = (i + 16 k)/4 has up to 12 significant
    bits: exact in float32, rounded in bf16"""
    return lat(shape, 127, 4, dt, seed, device), (lat(shape, 127, 4, F32, seed + 1, device) * 16).to(dt)


def tie_pair(n, dt, device):
    """(da, db) whose sums are exactly halfway between two bf16 values: da = 129 .. 255 (ulp 1 in bf16), db = +-1/2.  Ties go to even."""
    i = torch.arange(n, device=device)
    da = (129 + i % 127).to(F32)
    db = torch.where((i // 128) % 2 == 0, 0.5, -0.5).to(F32)
    return da.to(dt), db.to(dt)


def tiny(dt):
    """(smallest positive subnormal, smallest normal) of dt as float64"""
    return (2.0 ** -133, 2.0 ** -126) if dt == BF16 else (2.0 ** -149, 2.0 ** -126)


def mask_values(dt):
    """the values of `a` the ReLU masks must decide: +0, -0, the smallest positive subnormal of dt, the smallest normal, -subnormal, +inf,
    NaN, -inf, 1, -1 -- as dt (built from float64 through float32: every one is a dt value)"""
    sub, nrm = tiny(dt)
    v = torch.tensor([0.0, -0.0, sub, nrm, -sub, math.inf, math.nan, -math.inf, 1.0, -1.0], dtype=torch.float64)
    t = v.float().to(dt)
    assert torch.equal(t.double().nan_to_num(nan=7.0), v.nan_to_num(nan=7.0))
    return t


MASK_PASSES = [False, False, True, True, False, True, False, False, True, False]      # a > 0.f on the float value


def special_pairs(dt):
    """(y, r) covering NaN, +-inf and +-0 on either side and inf - inf, as dt [n]"""
    inf, nan = math.inf, math.nan
    s = [0.0, -0.0, inf, -inf, nan, 1.0, -1.0]
    y = torch.tensor([a for a in s for _ in s], dtype=torch.float64)
    r = torch.tensor([b for _ in s for b in s], dtype=torch.float64)
    return y.float().to(dt), r.float().to(dt)


# ---------------------------------------------------------------------------------------------------------------------------------------
# restatements: encoder2d.hip, and the element-wise kernels of ops2d.hip
# ---------------------------------------------------------------------------------------------------------------------------------------
def relu64(s):
    """`s > 0.f ? s : 0.f`: NaN, -inf and -0 store +0"""
    return torch.where(s > 0, s, torch.zeros_like(s))


def ref_bn_add_relu(y, sc, sh, r, rsc, rsh, dt, mid=True):
    """out = T(relu(T(sc y + sh) + (rsc given ? T(rsc r + rsh) : r)))  (mid=False: without the two intermediate roundings)"""
    t = sc.double() * y.double() + sh.double()
    i = r.double() if rsc is None else rsc.double() * r.double() + rsh.double()
    if mid:
        t = t.to(dt).double()
        if rsc is not None:
            i = i.to(dt).double()
    return relu64(t + i).to(dt)


def ref_add_relu(t, r, dt):
    return relu64(t.double() + r.double()).to(dt)


def ref_relu_mask(da, a):
    """g = da's bits where a > 0 else +0"""
    return torch.where(a.double() > 0, da, torch.zeros_like(da))


def ref_relu_mask_sum(da, db, a, dt):
    return torch.where(a.double() > 0, (da.double() + db.double()).to(dt), torch.zeros_like(da))


def ref_bn_relu(y, sc, sh, dt, mid=True):
    """the stem's activation T(relu(sc y + sh)) (mid=False: unrounded, float64)"""
    a = relu64(sc.double() * y.double() + sh.double())
    return a.to(dt) if mid else a


def windows9(a, fill=-math.inf):
    """[N, H, W, C] -> values [N, Ho, Wo, 9, C] of the 3x3 stride-2 pad-1 windows in scan order (code = kh * 3 + kw) and the in-bounds mask
    [1, Ho, Wo, 9, 1]"""
    N, H, W, C = a.shape
    Ho, Wo = pool_out(H), pool_out(W)
    pad = F.pad(a, (0, 0, 1, 2, 1, 2), value=fill)
    v = torch.stack([pad[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2] for kh in range(3) for kw in range(3)], dim=3)
    oh = torch.arange(Ho, device=a.device).view(Ho, 1, 1)
    ow = torch.arange(Wo, device=a.device).view(1, Wo, 1)
    k = torch.arange(9, device=a.device).view(1, 1, 9)
    ih, iw = 2 * oh - 1 + k // 3, 2 * ow - 1 + k % 3
    valid = (ih >= 0) & (ih < H) & (iw >= 0) & (iw < W)
    return v, valid.view(1, Ho, Wo, 9, 1)


def pool_arg9(v, valid):
    """-> uint8 codes [N, Ho, Wo, C].  The kernels' rule (aten's): from m = -inf and the first in-bounds position, `f > m || f != f` takes
    over: the FIRST maximum in scan order; a NaN takes over wherever it stands, so the LAST NaN wins; an all -inf window keeps its first
    in-bounds position"""
    v = v.float()
    nan = (v != v) & valid
    m = torch.where(nan | ~valid, torch.full_like(v, -math.inf), v).amax(3, keepdim=True)
    ismax = (v == m) & valid & ~nan
    down = torch.arange(9, 0, -1, device=v.device).view(1, 1, 1, 9, 1)
    up = torch.arange(1, 10, device=v.device).view(1, 1, 1, 9, 1)
    first = (ismax * down).argmax(3)
    last_nan = (nan * up).argmax(3)
    return torch.where(nan.any(3), last_nan, first).to(torch.uint8)


def ref_maxpool(a):
    """[N, H, W, C] -> (p [N, Ho, Wo, C] with a's bits, idx uint8)"""
    v, valid = windows9(a)
    code = pool_arg9(v, valid)
    return v.gather(3, code.long().unsqueeze(3)).squeeze(3), code


def aten_maxpool(a):
    """the same from F.max_pool2d(return_indices=True) in float64 on [N, H, W, C]: torch's flat index h * W + w -> kh * 3 + kw"""
    N, H, W, C = a.shape
    p, flat = F.max_pool2d(a.double().permute(0, 3, 1, 2), 3, 2, 1, return_indices=True)
    Ho, Wo = p.shape[2], p.shape[3]
    oh = torch.arange(Ho, device=a.device).view(1, 1, Ho, 1)
    ow = torch.arange(Wo, device=a.device).view(1, 1, 1, Wo)
    code = (flat // W - (2 * oh - 1)) * 3 + (flat % W - (2 * ow - 1))
    assert int(code.min()) >= 0 and int(code.max()) <= 8
    return p.permute(0, 2, 3, 1).contiguous(), code.permute(0, 2, 3, 1).contiguous().to(torch.uint8)


def ref_maxpool_bwd(g64, idx, H, W):
    """float64 [N, Ho, Wo, C] gradient and the stored codes -> float64 dx [N, H, W, C]: a pixel sums the windows whose argmax it is"""
    N, Ho, Wo, C = g64.shape
    code = idx.long()
    oh = torch.arange(Ho, device=g64.device).view(1, Ho, 1, 1)
    ow = torch.arange(Wo, device=g64.device).view(1, 1, Wo, 1)
    ih, iw = 2 * oh - 1 + code // 3, 2 * ow - 1 + code % 3
    assert bool(((ih >= 0) & (ih < H) & (iw >= 0) & (iw < W)).all()), "a stored code points outside the image"
    n = torch.arange(N, device=g64.device).view(N, 1, 1, 1)
    c = torch.arange(C, device=g64.device).view(1, 1, 1, C)
    flat = ((n * H + ih) * W + iw) * C + c
    dx = torch.zeros(N * H * W * C, dtype=torch.float64, device=g64.device)
    dx.scatter_add_(0, flat.reshape(-1), g64.reshape(-1))
    return dx.view(N, H, W, C)


def ref_maxpool_bwd_sum(dy, dy2, idx, H, W, dt, pre=True):
    """dx = T(sum over the windows of T(dy + dy2))  (pre=False: the sum of the two is not rounded before it is accumulated)"""
    s = dy.double() + dy2.double()
    if pre:
        s = s.to(dt).double()
    return ref_maxpool_bwd(s, idx, H, W).to(dt)


def argmax_multiplicity(idx, H, W):
    """how many windows each pixel is the argmax of: int64 [N, H, W, C]"""
    return ref_maxpool_bwd(torch.ones(idx.shape, dtype=torch.float64, device=idx.device), idx, H, W).long()


def ref_nearest2_bwd(dy, dt):
    """[N, 2H, 2W, C] -> [N, H, W, C]: the 2x2 sum, rounded once"""
    d = dy.double()
    return (d[:, 0::2, 0::2] + d[:, 0::2, 1::2] + d[:, 1::2, 0::2] + d[:, 1::2, 1::2]).to(dt)


def three_level(shape, dt, seed, device):
    """values in {-1/4, 1/2, 3/4}: most 3x3 windows hold ties"""
    g = torch.Generator(device=device).manual_seed(seed)
    k = torch.randint(0, 3, tuple(shape), generator=g, device=device)
    return torch.tensor([-0.25, 0.5, 0.75], dtype=F32, device=device)[k].to(dt)


# ---------------------------------------------------------------------------------------------------------------------------------------
# bilinear
# ---------------------------------------------------------------------------------------------------------------------------------------
def bilinear_axis(out_size, in_size, s, fused=True):
    """bilinear_src (ops2d.hip) for dst = 0 .. out_size - 1 -> (i0, i1 int64, l1 float64 holding the float32 value).  inv = 1.0f / (float)s
    is the correctly rounded float32 quotient; src = ((float)dst + 0.5f) * inv - 0.5f is ONE fused multiply-add in the compiled kernel
    (the compiler contracts it), restated as the float64 product -- exact: 24 x 12 bits -- minus 0.5 rounded once to float32; fused=False
    rounds the product first (what the source text says without contraction).  For s a power of two both are exact and equal."""
    dst = np.arange(out_size, dtype=np.float64)
    inv = np.float64(np.float32(1.0) / np.float32(s))
    if fused:
        src = ((dst + 0.5) * inv - 0.5).astype(np.float32)
    else:
        src = ((dst + 0.5) * inv).astype(np.float32) - np.float32(0.5)
    src = np.maximum(src, np.float32(0.0)).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), in_size - 1)
    i1 = i0 + (i0 < in_size - 1)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    return torch.from_numpy(i0), torch.from_numpy(i1.astype(np.int64)), torch.from_numpy(l1.astype(np.float64))


def bilinear_matrix(in_size, s, fused=True):
    """float64 [in_size * s, in_size]: row dst holds (1 - l1) at i0 plus l1 at i1"""
    out = in_size * s
    i0, i1, l1 = bilinear_axis(out, in_size, s, fused)
    A = torch.zeros(out, in_size, dtype=torch.float64)
    r = torch.arange(out)
    A[r, i0] += 1.0 - l1
    A[r, i1] += l1
    return A


def ref_bilinear_fwd(x, s, absolute=False, fused=True):
    """float64 [N, H s, W s, C] from x [N, H, W, C]; absolute=True: the same with |weights| |x| (the scale of the derived bound)"""
    Ah, Aw = bilinear_matrix(x.shape[1], s, fused).to(x.device), bilinear_matrix(x.shape[2], s, fused).to(x.device)
    xx = x.double().abs() if absolute else x.double()
    return torch.einsum("oh,nhwc,pw->nopc", Ah, xx, Aw)


def ref_bilinear_bwd(dy, s):
    """float64 adjoint of ref_bilinear_fwd: dy [N, H s, W s, C] -> [N, H, W, C]"""
    H, W = dy.shape[1] // s, dy.shape[2] // s
    Ah, Aw = bilinear_matrix(H, s).to(dy.device), bilinear_matrix(W, s).to(dy.device)
    return torch.einsum("oh,nopc,pw->nhwc", Ah, dy.double(), Aw)


# ---------------------------------------------------------------------------------------------------------------------------------------
# heads2d.hip
# ---------------------------------------------------------------------------------------------------------------------------------------
def nchw_to_rows(gt, N, C, HW):
    """[N, C, HW] -> [N HW, C]"""
    return gt.view(N, C, HW).permute(0, 2, 1).reshape(N * HW, C)


def ref_mse(p, gt, N, C, HW):
    """(float)(sum * (1.0 / (M C))): p [M, C] float32, gt [N, C, HW] float32 -> float32 0-d tensor (CPU).  The sum is exact in float64."""
    d = p.double() - nchw_to_rows(gt, N, C, HW).double()
    total = float((d * d).sum())
    return torch.tensor(total * (1.0 / (float(N * HW) * C)), dtype=torch.float64).float()


def mse_g(dloss, M, k32=True):
    """the kernel's g = dloss * (float)(2.0 / (M 3)) as a float32 numpy scalar (k32=False: the float64 product, never rounded)"""
    if not k32:
        return np.float64(np.float32(dloss)) * (2.0 / (float(M) * 3))
    return np.float32(dloss) * np.float32(2.0 / (float(M) * 3))


def ref_mse_bwd(p, gt, dloss, N, HW, CP, dt, k32=True):
    """dy [M, CP] in dt: T(g * (p - gt)) with ONE float32 product, +0 in the padding channels (k32=False: g and the product in float64,
    rounded once to float32 and then to T)"""
    M = N * HW
    d = p - nchw_to_rows(gt, N, 3, HW)                                      # exact in float32 on the lattice
    if k32:
        v = d * torch.tensor(float(mse_g(dloss, M)), dtype=F32, device=p.device)
    else:
        v = (d.double() * float(mse_g(dloss, M, k32=False))).float()
    out = torch.zeros((M, CP), dtype=dt, device=p.device)
    out[:, :3] = v.to(dt)
    return out


def block_sums64(v, rows=ROWS_PER_BLOCK):
    """[M, K] -> float64 [ceil(M / rows), K]: the sums of each block of `rows` rows"""
    M, K = v.shape
    nb = -(-M // rows)
    buf = torch.zeros((nb * rows, K), dtype=torch.float64, device=v.device)
    buf[:M] = v.double()
    return buf.view(nb, rows, K).sum(1)


def ref_conv1x1_small_bwd(x, dy, w, dt):
    """x [M, Ci] (dt), dy [M, 3] float32, w [3, Ci] float32 -> dx (dt) and the float64 partial rows [blocks, 3 Ci + 3] of 1024 pixels"""
    M, Ci = x.shape
    dx = (dy.double() @ w.double()).to(dt)
    nb = rows1024(M)
    xb = torch.zeros((nb * ROWS_PER_BLOCK, Ci), dtype=torch.float64, device=x.device)
    gb = torch.zeros((nb * ROWS_PER_BLOCK, 3), dtype=torch.float64, device=x.device)
    xb[:M], gb[:M] = x.double(), dy.double()
    xb, gb = xb.view(nb, ROWS_PER_BLOCK, Ci), gb.view(nb, ROWS_PER_BLOCK, 3)
    part = torch.cat([torch.einsum("bmo,bmi->boi", gb, xb).reshape(nb, 3 * Ci), gb.sum(1)], dim=1)
    return dx, part


def ref_nchw_to_nhwc_pad(x, N, C, HW, dt):
    out = torch.zeros((N * HW, 8), dtype=dt, device=x.device)
    out[:, :C] = nchw_to_rows(x, N, C, HW).to(dt)
    return out


def mse_diff(shape, seed, device, dt=BF16):
    """p - gt of the backward cases: i/4 with |i| <= 15 (zero included) for the bf16 form, whose column partials must be exact; |i| <= 127 for
    the float32 forms, so that many different products meet the float32 coefficient"""
    return lat(shape, 15 if dt == BF16 else 127, 4, F32, seed, device)


def mse_bwd_inputs(N, HW, dt, device):
    """-> p [M, 3] float32 (NHWC rows), gt [N, 3, HW] float32"""
    M = N * HW
    gt = lat((N, 3, HW), 8, 4, F32, M + 1, device)
    return nchw_to_rows(gt, N, 3, HW) + mse_diff((M, 3), M, device, dt), gt


# ---------------------------------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------------------------------
def ids(v):
    return str(v).replace("torch.", "").replace(" ", "")


def wrap_rows(C, dt):
    ns = nslots(C, dt)
    return RC_CAP * ns + 2 * ns + max(ns // 3, 1)


def thread_rows(M, C, dt):
    """the set of row counts the threads of a bn_add_relu launch see (how often each runs the unroll-4 loop's body)"""
    ns = nslots(C, dt)
    blocks, _ = rc_blocks(M, C, dt)
    stride = blocks * ns
    lo, hi = M // stride, -(-M // stride)
    return {lo, hi} if M % stride else {lo}


BAR_C = {F32: (4, 64, 128, 256, 512, 1024), BF16: (8, 64, 128, 256, 512, 2048)}
# (dt, C, M): the grid wrap for every slot count; M = 1; thread row counts {0, 1}, {3, 4}, {4, 5} around the unroll of four
BAR_CASES = [(dt, C, wrap_rows(C, dt)) for dt in (F32, BF16) for C in BAR_C[dt]]
BAR_CASES += [(F32, 1024, 1), (BF16, 2048, 1), (F32, 256, 37), (BF16, 512, 37)]
BAR_CASES += [(F32, 512, 3 * 4096 + 11), (F32, 512, 4 * 4096 + 7), (BF16, 2048, 3 * 2048 + 5), (BF16, 2048, 4 * 2048 + 3), (F32, 1024, 5 * 2048)]
BAR_NT = [(BF16, 64, 1572864), (BF16, 64, 1572863), (F32, 64, 786432)]      # M C esize = 201 326 592 = 192 MiB: on, one row below: off, float32 on

WRAP_VECS = GRID_CAP * 256 + 302                                             # 302 vectors past one pass of grid_for()'s 16 384 blocks
MASK_NVEC = [1, 255, 256, 257, WRAP_VECS]

POOL_EXTENTS = [(1, 1), (1, 7), (2, 2), (2, 5), (3, 4), (7, 1), (15, 9), (16, 24)]
POOL_KINDS = ["lattice", "three-level", "negative", "rounded-tie"]
POOL_BIG = (BF16, 8, 4, 2050, 2052)      # N Ho Wo = 4 * 1025 * 1026 = 4 206 600 vectors; the backward has N H W = 16 826 400

UP_EXTENTS = [(1, 1), (1, 5), (5, 1), (3, 4), (8, 12)]
UP_BIG = (BF16, 8, 1, 2049, 2050)        # N H W = 4 200 450 vectors
BIL_EXTENTS = [(1, 1), (1, 6), (6, 1), (2, 3), (5, 7)]
BIL_POW2 = [1, 2, 4, 8, 16]
BIL_ODD = [3, 5]
BIL_C = [1, 3, 4, 5]
BIL_DY_INT = 8

# (N, HW, C) of pcrl_mse2d_fwd; M = N HW
MSE_M = [1, 255, 256, 257, 1023, 1024, 1025]
MSE_FWD = [(1, m, c) for m in MSE_M for c in (1, 3)] + [(3, 85, 3), (3, 341, 3), (3, 343, 3), (3, 343, 1)]
MSE_FWD += [(1, 768 * 1024 - 5, 3), (1, 768 * 1024 + 1, 3), (1, 1024 * 1024, 1), (1, 1024 * 1024 + 1, 3), (3, 351403, 3)]
MSE_BLOCKS = [768, 769, 1024, 1025, 1030]
MSE_BWD = [(1, m) for m in MSE_M] + [(3, 85), (3, 341), (3, 343), (3, 1365)]      # (N, HW); 3 x 1365 = 4095 rows: four blocks, the last of 1023
MSE_FORMS = [(BF16, 8), (F32, 8), (F32, 3)]
MSE_DLOSS = 1.3

C11_CI = {F32: (4, 16, 64, 1024), BF16: (8, 16, 128, 2048)}


def c11_ms(Ci, dt):
    ns = nslots(Ci, dt)
    return sorted({m for m in (1, ns - 1, 2 * ns + 1, 1023, 1024, 1025, 2049) if m > 0})


C11_CASES = [(dt, Ci, M) for dt in (F32, BF16) for Ci in C11_CI[dt] for M in c11_ms(Ci, dt)]

PAD_CASES = [(dt, C, N, HW) for dt in (F32, BF16) for C in (1, 2, 3) for N, HW in ((1, 1), (2, 255), (3, 257))]
PAD_BIG = (BF16, 3, 1, 16777216 + 300)


# ---------------------------------------------------------------------------------------------------------------------------------------
# inputs of the cases (the CPU test evaluates the restatements on exactly these)
# ---------------------------------------------------------------------------------------------------------------------------------------
def bar_inputs(dt, C, M, device):
    """-> y, r [M, C] (dt) and the coefficients of a pcrl_bn_add_relu_fwd case"""
    return lat((M, C), Y_INT, 4, dt, M % 1000 + 1, device), lat((M, C), Y_INT, 4, dt, M % 1000 + 2, device), Coef2(C, C, device)


def pool_inputs(kind, dt, N, H, W, C, device):
    """-> y [N, H, W, C] (dt), scale, shift (float32 [C]) of a pcrl_bn_relu_maxpool2d_3s2_fwd case"""
    one, zero = torch.ones(C, dtype=F32, device=device), torch.zeros(C, dtype=F32, device=device)
    seed = 31 * H + W + N
    if kind == "lattice":
        co = Coef2(C, seed, device)
        return lat((N, H, W, C), Y_INT, 4, dt, seed, device), co.scale, co.shift
    if kind == "three-level":                 # a in {0, 1/2, 3/4}
        return three_level((N, H, W, C), dt, seed, device), one, zero
    if kind == "negative":                    # z in [-6, -2]: every activation is +0 and the first in-bounds position wins
        return lat((N, H, W, C), Y_INT, 4, dt, seed, device), one, zero - 4.0
    assert kind == "rounded-tie"              # z = 101 + r/128: distinct in float32, all 101 in bf16
    g = torch.Generator(device=device).manual_seed(seed)
    r = torch.randint(0, 8, (N, H, W, C), generator=g, device=device)
    return (1 + r.to(F32) / 128).to(dt), one, zero + 100.0
