"""Case lists, lattices and float64 restatements for csrc/heads_fused.hip, csrc/val_metrics.hip, csrc/val_metrics2d.hip and csrc/cls_head.hip
(test_heads_eval_cases_cpu.py, test_head_bwd_stage_gpu.py, test_val_metrics_edges_gpu.py, test_cls_head_gpu.py).  Not a test file.

The restatements run on the CPU in float64 and are written from the formulas in the kernels' header comments:
  head_bwd_stage   t = add + dy W;  ReLU mask where ybn <= 0 (-0.0 included);  xh = (xbn - mean) rstd;  dbeta = sum_n t;  dgamma = sum_n t xh;
                   dx = gamma rstd (t - dbeta / N - xh dgamma / N);  dW = dy^T xin;  db = sum_n dy
  val_metrics      acc[0] += sum (out1 - gt)^2 / S;  acc[1 + k] likewise for mask_k;  a cosine term is dot / (max(|x|, eps) max(|y|, eps));
                   acc[4 + k] += -1/2 sum_r (cos(pre1[r], pro2[r]) + cos(pre2[r], pro1[r]));
                   acc[7 + k] += -1 / (4 nlocal) sum over local views i, rows r of cos(pre1[r], proL[iB + r]) + cos(preL[iB + r], pro1[r])
                                                                                 + cos(pre2[r], proL[iB + r]) + cos(preL[iB + r], pro2[r])
  val2d_metrics    the same with five scales, three channels (S = 3 H W) and mask_k upsampled by 2^(4 - k) inside the reduction: align_corners=False,
                   src = (dst + 1/2) / s - 1/2 clamped at 0, i0 = floor(src) clamped to the last index, i1 = i0 + 1 clamped likewise, l1 = src - i0

Lattices (exact_lattice.py): dy, xin, xbn, add = i/4, |i| <= 4; W = j/8, |j| <= 2; mean = j/8, |j| <= 8; rstd in {1/2, 1, 2}; gamma in +-{1/2, 1, 2};
ybn a mix of positive values, negative values, +0.0 and -0.0; the validation maps i/8, |i| <= 8.  On them every float32 product and sum of
pcrl_head_bwd_stage is exact in any order (test_heads_eval_cases_cpu.py asserts the preconditions), and every square, every interpolation product
(the weights of a power-of-two scale are multiples of 1/32) and every float64 sum of the validation kernels' first stages is exact.
"""
import os
import re

import numpy as np
import torch

from exact_lattice import lattice

SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pcrlv2_amd", "csrc")

# ---- the constants of the sources, restated (test_heads_eval_cases_cpu.py checks them against the text of the .hip files) ----
RMAX = 8                          # rows per lane of role A: N <= 64 * RMAX
HEAD_MAX_N = 64 * RMAX
VM_CHUNK = 4096                   # elements per first-stage block of pcrl_val_metrics
V2_SCALES, V2_PX = 5, 1024        # scales, pixels per first-stage block of pcrl_val2d_metrics
FINISH_THREADS = 256              # stride of the finishing kernels' walks over `blocks` and over the R term rows
COS_WAVES = 4                     # term rows (waves) per block of val_cos_rows_kernel / val2d_cos_rows_kernel
CH_THREADS, CH_MAX_C, CH_MAX_K = 256, 512, 64
EPS = float(np.float32(1e-8))     # eps is a `float` argument of both validation entry points: the kernels see the float32 value of 1e-8

SOURCE_PINS = [                   # (file, source text), compared token by token: spacing and line breaks do not matter
    ("heads_fused.hip", "constexpr int RMAX = 8;"),
    ("heads_fused.hip", "const int kq = ((K / 4 + 3) / 4) * 4;"),
    ("heads_fused.hip", "const int k0 = wv * kq, k1 = min(K, k0 + kq);"),
    ("heads_fused.hip", "nBx = (C + 255) / 256"),
    ("heads_fused.hip", "const int n = lane + 64 * i;"),
    ("heads_fused.hip", "for (int n = lane; n < N; n += 64)"),
    ("val_metrics.hip", "constexpr int VM_CHUNK = 4096;"),
    ("val_metrics.hip", "for (int i = threadIdx.x; i < blocks; i += 256)"),
    ("val_metrics.hip", "for (int j = threadIdx.x; j < R; j += 256)"),
    ("val_metrics.hip", "const int j = blockIdx.x * 4 + (threadIdx.x >> 6);"),
    ("val_metrics2d.hip", "constexpr int V2_SCALES = 5, V2_PX = 1024;"),
    ("val_metrics2d.hip", "for (int i = threadIdx.x; i < blocks; i += 256)"),
    ("val_metrics2d.hip", "for (int j = threadIdx.x; j < R; j += 256)"),
    ("val_metrics2d.hip", "const int j = blockIdx.x * 4 + (threadIdx.x >> 6);"),
    ("cls_head.hip", "constexpr int CH_THREADS = 256, CH_MAX_C = 512, CH_MAX_K = 64;"),
    ("cls_head.hip", "for (int i = threadIdx.x; i < N; i += CH_THREADS)"),
    ("cls_head.hip", "for (int64_t n = threadIdx.x; n < N; n += 64)"),
    ("cls_head.hip", "for (int k = wid; k < K; k += CH_THREADS / 64)"),
]


def read_source(name):
    return open(os.path.join(SOURCE, name)).read()


def _tokens(text):
    return re.findall(r"\w+|[^\w\s]", text)


def source_pins_hold(pins=None):
    """-> the pins whose token sequence does not occur in their file"""
    missing = []
    for f, text in SOURCE_PINS if pins is None else pins:
        hay, pin = " ".join(_tokens(read_source(f))), " ".join(_tokens(text))
        if f" {pin} " not in f" {hay} ":
            missing.append((f, text))
    return missing


# ---- pcrl_head_bwd_stage: the splits of the launch, from the restated rules ----
def head_quarters(K):
    """[k0, k1) of the four waves of role A: kq = ((K / 4 + 3) / 4) * 4, k0 = wave * kq, k1 = min(K, k0 + kq); an empty quarter has k1 <= k0"""
    kq = ((K // 4 + 3) // 4) * 4
    return [(w * kq, min(K, w * kq + kq)) for w in range(4)]


def head_empty_waves(K):
    return sum(1 for k0, k1 in head_quarters(K) if k1 <= k0)


def head_short_waves(K):
    """waves whose quarter is not empty and shorter than kq"""
    kq = ((K // 4 + 3) // 4) * 4
    return sum(1 for k0, k1 in head_quarters(K) if 0 < k1 - k0 < kq)


def head_nbx(C):
    return (C + 255) // 256


def head_idle_b_lanes(C):
    """lanes of role B's last x-block whose four columns lie at or beyond C (c = ((b % nBx) * 64 + lane) * 4 >= C)"""
    return head_nbx(C) * 64 - C // 4


def head_rows_per_lane(N):
    """(rows of lane 0, rows of lane 63) in n = lane + 64 i"""
    return -(-N // 64), max(0, -(-(N - 63) // 64))


HEAD_N = (2, 63, 64, 65, 128, 449, 511, 512)
HEAD_K = (4, 8, 12, 16, 20, 36, 64, 132)
HEAD_C = (4, 60, 64, 252, 256, 260, 516)

HEAD_CASES = [      # (N, K, C, why)
    (2, 4, 4, "corner: two rows, one k-quad (waves 1..3 of role A idle), one column quad"),
    (512, 132, 516, "corner: RMAX rows in every lane, kq = 36 with a 24-long last quarter, three x-blocks of role B"),
]
# every K with N = 65 (lane 0 owns two rows, every other lane one); C walks the axis
HEAD_CASES += [(65, K, C, f"K = {K}: quarters {head_quarters(K)}")
               for K, C in zip(HEAD_K, (4, 60, 64, 252, 256, 260, 516, 252))]
# every N with K = 20 (quarters 8, 8, 4, empty) and C = 260 (role B: second x-block, one live lane in it)
HEAD_CASES += [(N, 20, 260, f"N = {N}: rows per lane (lane 0, lane 63) = {head_rows_per_lane(N)}") for N in HEAD_N if N != 65]
HEAD_CASES += [(65, 20, 260, "N = 65 at the C = 260 / K = 20 point of the canary set")]
HEAD_CASES += [
    (63, 4, 252, "canary set: C = 252 ends one lane before the first x-block of role B does; lane 63 has no row"),
    (449, 20, 252, "canary set: K = 20, C = 252; N = 449 = 7 x 64 + 1: only lane 0 has an eighth row"),
    (64, 4, 260, "canary set: K = 4, C = 260; every lane exactly one row"),
    (511, 4, 260, "lane 63 is the only one without an eighth row"),
    (128, 8, 256, "C = 256: role B's single x-block exactly full; K = 8: waves 2 and 3 idle"),
    (2, 132, 60, "two rows against the longest K walk"),
    (512, 12, 64, "K = 12: one idle wave; every lane RMAX rows"),
    (449, 36, 516, "K = 36: kq = 12, the fourth quarter empty; C = 516: third x-block of role B with one live lane"),
    (511, 64, 4, "K = 64: four full quarters; one column quad"),
    (63, 16, 516, "K = 16: four quarters of one k-quad"),
    (128, 132, 256, "K = 132 at a power-of-two N: dx bit for bit on the longest walk"),
    (64, 36, 60, "power-of-two N with an empty fourth quarter"),
    (2, 8, 516, "two rows, three x-blocks"),
    (512, 64, 260, "power-of-two N, full quarters, second x-block"),
    (449, 12, 4, "odd rows, three live waves, one column quad"),
    (63, 132, 64, "lane 63 idle on the longest walk"),
    (128, 4, 60, "C = 60: the last lane group of role B idle"),
    (511, 16, 256, "N = 511, four one-quad quarters, full x-block"),
    (64, 64, 252, "N = 64 with full quarters at C = 252"),
    (512, 36, 4, "RMAX rows, empty fourth quarter, one column quad"),
    (2, 20, 64, "two rows at K = 20"),
]
HEAD_ADD_ONLY = [(N, C) for N in (2, 65, 512) for C in (4, 260)]      # dy = W = xin = dW = db = NULL
HEAD_LARGEST = (512, 132, 516)
HEAD_CANARY = [(N, K, C) for N, K, C, _ in HEAD_CASES if C in (252, 260) and K in (4, 20)]

DY_LAT, W_LAT, MEAN_LAT = (4, 4), (2, 8), (8, 8)      # (max_int, den)
RSTD_VALUES = (0.5, 1.0, 2.0)
GAMMA_VALUES = (-2.0, -1.0, -0.5, 0.5, 1.0, 2.0)
YBN_VALUES = (1.5, 0.25, -0.75, -2.0, 0.0, -0.0)       # the ReLU mask `ybn <= 0` holds for the last four


def head_inputs(N, K, C, seed):
    """float64 CPU tensors on the lattices -> dict(dy [N,K], W [K,C], add [N,C], xin [N,C], xbn [N,C], ybn [N,C], gamma, mean, rstd [C])"""
    g = torch.Generator().manual_seed(seed)
    pick = lambda values, shape: torch.tensor(values, dtype=torch.float64)[torch.randint(0, len(values), shape, generator=g)]
    return dict(dy=lattice((N, K), *DY_LAT, g), W=lattice((K, C), *W_LAT, g), add=lattice((N, C), *DY_LAT, g), xin=lattice((N, C), *DY_LAT, g),
                xbn=lattice((N, C), *DY_LAT, g), ybn=pick(YBN_VALUES, (N, C)), gamma=pick(GAMMA_VALUES, (C,)), mean=lattice((C,), *MEAN_LAT, g),
                rstd=pick(RSTD_VALUES, (C,)))


def head_bwd_stage_ref(dy, W, add, xin, xbn, ybn, gamma, mean, rstd, relu):
    """float64 -> dx [N,C], dgamma [C], dbeta [C], dW [K,C] | None, db [K] | None (the formulas of the module docstring; dy or add may be None)"""
    N = xbn.shape[0]
    t = torch.zeros_like(xbn)
    if dy is not None:
        t = t + dy @ W
    if add is not None:
        t = t + add
    if relu:
        t = torch.where(ybn <= 0, torch.zeros_like(t), t)          # -0.0 <= 0 holds
    xh = (xbn - mean) * rstd
    dbeta = t.sum(0)
    dgamma = (t * xh).sum(0)
    dx = gamma * rstd * (t - dbeta / N - xh * dgamma / N)
    if dy is None:
        return dx, dgamma, dbeta, None, None
    return dx, dgamma, dbeta, dy.t() @ xin, dy.sum(0)


def head_dx_slack(dy, W, add, xbn, ybn, gamma, mean, rstd, relu):
    """|gamma rstd| (|t| + |dbeta| / N + |xh dgamma| / N): what the 2^-50 term of the bound on dx multiplies when N is no power of two"""
    N = xbn.shape[0]
    t = torch.zeros_like(xbn)
    if dy is not None:
        t = t + dy @ W
    if add is not None:
        t = t + add
    if relu:
        t = torch.where(ybn <= 0, torch.zeros_like(t), t)
    xh = (xbn - mean) * rstd
    dbeta, dgamma = t.sum(0), (t * xh).sum(0)
    return (gamma * rstd).abs() * (t.abs() + dbeta.abs() / N + (xh * dgamma).abs() / N)


def ulp_f32(x64):
    """the float32 spacing at |x| (float64 tensor)"""
    a = x64.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def is_pow2(n):
    return n > 0 and n & (n - 1) == 0


# ---- pcrl_val_metrics / pcrl_val2d_metrics ----
MAP_LAT = (8, 8)
VAL_BIG_S = 257 * VM_CHUNK + 77           # the smallest S that gives B = 1 more than 256 first-stage blocks with a ragged last chunk
VAL2D_BIG = (1, 544, 496)                 # 263.5 blocks of 1024 pixels: H != W, more than 256 blocks, a ragged last block
C3_A, C3_B = (1, 63, 200), (65, 64, 130)  # channel widths that differ between the scales: one lane live, one lane idle, four trips with a short one
C5 = (1, 63, 64, 65, 200)

VAL3D_CASES = [     # (B, S, nlocal, widths, why)
    (1, 1, 1, C3_A, "one element, one sample, R = 6: the last block of the cosine rows has two live waves"),
    (1, 255, 6, C3_B, "S one short of a block's 256 threads; R = 26"),
    (1, 257, 1, C3_A, "S one past the 256 threads: thread 0 takes a second element"),
    (3, 4096, 6, C3_B, "n = 3 chunks exactly; B = 3, nlocal = 6: R = 78"),
    (1, 4097, 1, C3_B, "a second chunk of one element"),
    (2, 6000, 1, C3_A, "the boundary between the samples lies inside a chunk; R = 12 = three full blocks of rows"),
    (1, VAL_BIG_S, 1, C3_A, "258 first-stage blocks: the finishing kernel's walk over `blocks` takes its second trip; ragged last chunk of 77"),
    (10, 17, 6, C3_B, "R = 260: the finishing kernel's walk over the term rows takes its second trip (in the local part)"),
    (43, 5, 1, C3_A, "R = 258 with 2B = 86 global rows: second trip, R % 4 = 2"),
    (5, 257, 2, C3_B, "R = 50: B = 5 rows per term, two local views"),
]
VAL2D_CASES = [     # (B, H, W, nlocal, why)
    (1, 16, 16, 1, "the smallest legal image: the coarsest map is one pixel, both interpolation indices clamp; 256 pixels: a ragged only block"),
    (1, 16, 48, 6, "H < W: the coarsest map is 1 x 3"),
    (1, 48, 16, 1, "H > W: the coarsest map is 3 x 1"),
    (2, 32, 80, 1, "H != W, five blocks of pixels exactly, the sample boundary inside a block"),
    (3, 64, 64, 6, "twelve blocks; B = 3, nlocal = 6: R = 78"),
    (VAL2D_BIG[0], VAL2D_BIG[1], VAL2D_BIG[2], 1, "264 first-stage blocks, the last one half full, H != W"),
    (10, 16, 16, 6, "R = 260: second trip of the finishing kernel's walk over the term rows"),
    (43, 16, 16, 1, "R = 258, R % 4 = 2"),
    (5, 16, 32, 2, "R = 50; 2560 pixels: a ragged last block"),
]


def val_blocks(B, S):
    return -(-(B * S) // VM_CHUNK)


def val2d_blocks(B, H, W):
    return -(-(B * H * W) // V2_PX)


def val_rows(B, nlocal):
    return B * (2 + 4 * nlocal)


def val_maps3d(B, S, seed):
    """-> out1, [mask0, mask1, mask2], gt: float64 [B, 1, 1, 1, S] on the i/8 lattice"""
    g = torch.Generator().manual_seed(seed)
    m = [lattice((B, 1, 1, 1, S), *MAP_LAT, g) for _ in range(5)]
    return m[0], m[1:4], m[4]


def val_maps2d(B, H, W, seed):
    """-> out1 [B,3,H,W], [mask_k [B,3,H >> (4-k),W >> (4-k)]], gt [B,3,H,W]: float64 on the i/8 lattice (logical NCHW)"""
    g = torch.Generator().manual_seed(seed)
    out1 = lattice((B, 3, H, W), *MAP_LAT, g)
    masks = [lattice((B, 3, H >> (V2_SCALES - 1 - k), W >> (V2_SCALES - 1 - k)), *MAP_LAT, g) for k in range(V2_SCALES)]
    return out1, masks, lattice((B, 3, H, W), *MAP_LAT, g)


def val_feats(B, nlocal, widths, seed):
    """per scale [pro1, pre1, pro2, pre2, proL, preL]: float32 CPU tensors from torch.randn; proL / preL have nlocal * B rows, view-major"""
    g = torch.Generator().manual_seed(seed)
    return [[torch.randn(rows, C, generator=g) for rows in (B, B, B, B, nlocal * B, nlocal * B)] for C in widths]


def cos_rows(x, y, eps=EPS):
    """dot / (max(|x|, eps) max(|y|, eps)) per row pair, float64"""
    x, y = x.double(), y.double()
    nx, ny = (x * x).sum(1).sqrt().clamp_min(eps), (y * y).sum(1).sqrt().clamp_min(eps)
    return (x * y).sum(1) / (nx * ny)


def cos_terms(f, B, nlocal, eps=EPS):
    """-> (global terms [2B], local terms [4 nlocal B]) of one scale, in the row order of the kernels' comments"""
    pro1, pre1, pro2, pre2, proL, preL = f
    glob = torch.cat([cos_rows(pre1, pro2, eps), cos_rows(pre2, pro1, eps)])
    loc = []
    for i in range(nlocal):
        pl, ql = proL[i * B:(i + 1) * B], preL[i * B:(i + 1) * B]
        loc += [cos_rows(pre1, pl, eps), cos_rows(ql, pro1, eps), cos_rows(pre2, pl, eps), cos_rows(ql, pro2, eps)]
    return glob, torch.cat(loc)


def _cos_entries(feats, B, nlocal, eps):
    g_val, g_abs, l_val, l_abs = [], [], [], []
    for f in feats:
        glob, loc = cos_terms(f, B, nlocal, eps)
        g_val.append(-0.5 * glob.sum())
        g_abs.append(0.5 * glob.abs().sum())
        l_val.append(-loc.sum() / (4.0 * nlocal))
        l_abs.append(loc.abs().sum() / (4.0 * nlocal))
    return g_val, g_abs, l_val, l_abs


def val_metrics_ref(out1, masks, gt, feats, B, nlocal, eps=EPS):
    """What ONE call adds to acc[0..9] and, per entry, the same weighted sum over the absolute values of its terms: float64 [10] each.
    out1, masks[k], gt: [B, ...] of S elements per sample; feats: per scale the six tensors of val_feats."""
    S = out1[0].numel()
    g = gt.double()
    mse = [((m.double() - g) ** 2).sum() / S for m in (out1, *masks)]
    g_val, g_abs, l_val, l_abs = _cos_entries(feats, B, nlocal, eps)
    return torch.stack(mse + g_val + l_val), torch.stack(mse + g_abs + l_abs)


def bilinear_index(n_out, scale, n_in):
    """-> i0, i1 (int64 [n_out]), l1 (float64 [n_out]) by the rule of the module docstring"""
    src = ((torch.arange(n_out, dtype=torch.float64) + 0.5) / scale - 0.5).clamp_min(0.0)
    i0 = src.floor().long().clamp_max(n_in - 1)
    i1 = (i0 + 1).clamp_max(n_in - 1)
    return i0, i1, src - i0.double()


def bilinear_up(m, scale):
    """[B,C,h,w] float64 -> [B,C,h * scale,w * scale]"""
    h, w = m.shape[-2:]
    h0, h1, lh = bilinear_index(h * scale, scale, h)
    w0, w1, lw = bilinear_index(w * scale, scale, w)
    lh = lh.view(-1, 1)
    top = (1.0 - lw) * m[..., h0, :][..., w0] + lw * m[..., h0, :][..., w1]
    bot = (1.0 - lw) * m[..., h1, :][..., w0] + lw * m[..., h1, :][..., w1]
    return (1.0 - lh) * top + lh * bot


def val2d_metrics_ref(out1, masks, gt, feats, B, nlocal, eps=EPS):
    """What ONE call adds to acc[0..15] and the weighted sums of absolute values: float64 [16] each.  Logical NCHW inputs; masks[k] at its own size."""
    S = out1[0].numel()                               # 3 H W
    g = gt.double()
    mse = [((out1.double() - g) ** 2).sum() / S]
    for k, m in enumerate(masks):
        mse.append(((bilinear_up(m.double(), 1 << (V2_SCALES - 1 - k)) - g) ** 2).sum() / S)
    g_val, g_abs, l_val, l_abs = _cos_entries(feats, B, nlocal, eps)
    return torch.stack(mse + g_val + l_val), torch.stack(mse + g_abs + l_abs)


# ---- pcrl_cls_head_fwd / _bwd ----
def cls_groups(C, bf16):
    """-> (NV vectors per pixel row, G row groups) of the forward's thread mapping: NV = C / V, G = 256 / NV, V = 16 bytes of the element type"""
    nv = C // (8 if bf16 else 4)
    return nv, CH_THREADS // nv


CLS_WIDTHS = (32, 64, 128, 256)
CLS_HW = ((1, 1), (3, 5), (5, 13))            # HW = 1, 15, 65: below, inside and above G (8 .. 64 for these widths)
CLS_WIDE_K = (4, 5, 63, 64)                   # the per-wave class loop: one trip each, a second trip for wave 0, 16 trips with wave 3 one short, 16 full
CLS_LONG_N = (65, 256, 257)                   # db's stride-64 walk takes a second trip; the loss kernel's stride-256 walk exactly one, then a second
