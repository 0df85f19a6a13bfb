"""Case table, lattices and restatements for csrc/augment.hip (test_aug_cases_cpu.py, test_augment_exact_gpu.py).  Not a test file.

Every pcrl_aug_* entry point takes its per-volume coefficients (inverse matrix, flip, fill, sigma, noise std, gamma, seed, mean, rstd, patch
corners) as INPUTS, so each kernel is judged alone.  What is compared with what:

  volume_min   bits.  The minimum is fminf's: a NaN operand is ignored (IEEE minNum), the sign of a zero minimum is not defined.
  affine       bits against aug_reference.ref_spatial (float64) on a dyadic lattice: inverse-matrix entries k/8, voxel centres j/2, so the
               sampling coordinates and the three fractions are multiples of 1/16, a corner weight is a multiple of 2^-12 <= 1, the data
               are integers |v| <= 64: every product and the 8-term sum are exact in float32 in any order, fused or not.
  blur_axis    bits where the pass is the identity (radius 0, sigma under the floor); otherwise blur_axis_bound()'s derived bound.
  noise_gamma  the integer hash is restated bit for bit (numpy uint32); logf / cosf / powf are the device library's, so the float result is
               held to 4 x the error of a float32 numpy evaluation of the same formula (the project's yardstick custom).
  meanstd      mean: the float32 rounding of the float64 mean; rstd: meanstd_bounds()'s derived bound.
  znorm        bits against float32 (x - m) * r.
  swap         bits against aug_reference.ref_swap.
"""
import itertools
import math
import os

import numpy as np
import torch


U = 2.0 ** -24                   # unit roundoff of float32
EPS = 2.0 ** -53                 # unit roundoff of float64

# ---- the constants of the source, restated (test_aug_cases_cpu.py checks them against the text of augment.hip) ----
GRID_CAP = 1024                  # blocks of noise_gamma_kernel / znorm_kernel
CAP_ITEMS = GRID_CAP * 256       # 262 144 elements in one grid-stride pass
RED_THREADS = 1024               # threads of vol_min_kernel / meanstd_kernel: 16 waves
SWAP_THREADS = 256
MAX_RADIUS = 32
SIGMA_FLOOR = np.float32(1e-3)
SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pcrlv2_amd", "csrc", "augment.hip")
SOURCE_PINS = [
    "if (gx > 1024) gx = 1024;",
    "hipLaunchKernelGGL(noise_gamma_kernel, dim3(gx, B), dim3(256)",
    "hipLaunchKernelGGL(znorm_kernel, dim3(gx, B), dim3(256)",
    "hipLaunchKernelGGL(vol_min_kernel, dim3(B), dim3(1024)",
    "hipLaunchKernelGGL(meanstd_kernel, dim3(B), dim3(1024)",
    "hipLaunchKernelGGL(swap_kernel, dim3(B), dim3(256)",
    "__shared__ float wt[65];",
    "radius >= 0 && radius <= 32",
    "fmaxf(sigma[b], 1e-3f)",
    "v ^= v >> 16; v *= 0x7feb352du; v ^= v >> 15; v *= 0x846ca68bu; v ^= v >> 16;",
    "const uint32_t k0 = mix32((uint32_t)seed ^ mix32(vol * 0x9e3779b9u + 0x85ebca6bu));",
    "const uint32_t k1 = mix32((uint32_t)(seed >> 32) ^ mix32(vol * 0x85ebca6bu + 0xc2b2ae35u));",
    "const uint32_t a = mix32(mix32((uint32_t)idx ^ k0) + k1);",
    "const uint32_t b2 = mix32(((uint32_t)(idx >> 32) + 0x632be5abu + a) ^ k1);",
    "const uint32_t c = mix32(a + 0x9e3779b9u + b2);",
    "const float u1 = ((float)(a >> 8) + 1.0f) * (1.0f / 16777216.0f);",
    "const float u2 = (float)(c >> 8) * (1.0f / 16777216.0f);",
    "return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);",
]


def source_pins_hold():
    """-> the pins whose token sequence does not occur in augment.hip"""
    import re

    def tok(s):
        return " " + " ".join(re.findall(r"\w+|[^\w\s]", s)) + " "
    hay = tok(open(SOURCE).read())
    return [p for p in SOURCE_PINS if tok(p) not in hay]


# ========================================================================================================================================
# noise: the counter hash
# ========================================================================================================================================
_M1, _M2 = np.uint32(0x7feb352d), np.uint32(0x846ca68b)
_M1_INV, _M2_INV = np.uint32(pow(0x7feb352d, -1, 1 << 32)), np.uint32(pow(0x846ca68b, -1, 1 << 32))
_u32 = np.uint32


def mix32(v):
    v = np.array(v, dtype=np.uint32)
    v ^= v >> _u32(16)
    v *= _M1
    v ^= v >> _u32(15)
    v *= _M2
    v ^= v >> _u32(16)
    return v


def unmix32(v):
    """the inverse permutation of mix32"""
    v = np.array(v, dtype=np.uint32)
    v ^= v >> _u32(16)
    v *= _M2_INV
    v ^= v >> _u32(15)
    v ^= v >> _u32(30)
    v *= _M1_INV
    v ^= v >> _u32(16)
    return v


def _words(seed):
    seed = int(seed) & ((1 << 64) - 1)
    return _u32(seed & 0xffffffff), _u32(seed >> 32)


def _split(idx):
    idx = np.asarray(idx, dtype=np.uint64)
    return (idx & np.uint64(0xffffffff)).astype(np.uint32), (idx >> np.uint64(32)).astype(np.uint32)


def keys_v1(seed, vol):
    """the ONE volume key of the hash before the fix: it enters as an XOR on the index and nowhere else"""
    lo, _ = _words(seed)
    with np.errstate(over="ignore"):
        return mix32(lo ^ mix32(np.asarray(vol, dtype=np.uint32) * _u32(0x9e3779b9) + _u32(0x85ebca6b)))


def draws_v1(seed, vol, idx):
    """(a, c) of normal_at BEFORE the fix (kept to show the defect: test_aug_cases_cpu.py reproduces the collisions with it)"""
    _, hi = _words(seed)
    ilo, ihi = _split(idx)
    with np.errstate(over="ignore"):
        a = mix32(ilo ^ keys_v1(seed, vol))
        b2 = mix32((ihi + _u32(0x632be5ab) + a) ^ hi)
        c = mix32(a + _u32(0x9e3779b9) + b2)
    return a, c


def keys(seed, vol):
    """-> (k0, k1): k0 permutes the index (XOR), k1 is added after the first mixing round.  For one seed, k1 is a bijection of the volume."""
    lo, hi = _words(seed)
    vol = np.asarray(vol, dtype=np.uint32)
    with np.errstate(over="ignore"):
        k0 = mix32(lo ^ mix32(vol * _u32(0x9e3779b9) + _u32(0x85ebca6b)))
        k1 = mix32(hi ^ mix32(vol * _u32(0x85ebca6b) + _u32(0xc2b2ae35)))
    return k0, k1


def draws(seed, vol, idx):
    """(a, c) of normal_at: a = mix32(mix32(idx_lo ^ k0) + k1), c = mix32(a + golden + mix32((idx_hi + const + a) ^ k1))"""
    k0, k1 = keys(seed, vol)
    ilo, ihi = _split(idx)
    with np.errstate(over="ignore"):
        a = mix32(mix32(ilo ^ k0) + k1)
        b2 = mix32((ihi + _u32(0x632be5ab) + a) ^ k1)
        c = mix32(a + _u32(0x9e3779b9) + b2)
    return a, c


TWO_PI_F32 = np.float32(6.28318530717958647692)


def uniforms(a, c):
    """u1 in (0, 1], u2 in [0, 1) and the angle, formed in float32 exactly as the kernel forms them (the first two are exact: 24-bit integers
    times 2^-24; the angle is one float32 product)"""
    u1 = ((a >> _u32(8)).astype(np.float32) + np.float32(1.0)) * np.float32(1.0 / 16777216.0)
    u2 = (c >> _u32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return u1, u2, (TWO_PI_F32 * u2).astype(np.float32)


def deviate64(a, c):
    u1, _, ang = uniforms(a, c)
    return np.sqrt(-2.0 * np.log(u1.astype(np.float64))) * np.cos(ang.astype(np.float64))


def deviate32(a, c):
    """the float32 yardstick: the same formula, operation by operation, in numpy float32"""
    u1, _, ang = uniforms(a, c)
    return (np.sqrt(np.float32(-2.0) * np.log(u1)) * np.cos(ang)).astype(np.float32)


def noise_field(seed, B, S, v1=False):
    """-> (a, c) uint32 [B, S] of one call"""
    idx = np.arange(S, dtype=np.uint64)
    f = draws_v1 if v1 else draws
    out = [f(seed, b, idx) for b in range(B)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def shared_fields_v1(seeds, B, S):
    """[(seed, i, j, K)]: volumes of one call whose keys differ by less than S (a power of two) -- the same field, permuted by idx ^ K"""
    assert S & (S - 1) == 0
    vol = np.arange(B, dtype=np.uint32)
    hits = []
    for seed in seeds:
        k = keys_v1(seed, vol)
        x = k[:, None] ^ k[None, :]
        for i, j in zip(*np.nonzero((x < S) & (vol[:, None] < vol[None, :]))):
            hits.append((seed, int(i), int(j), int(x[i, j])))
    return hits


def shared_fields(seeds, B, sizes, probes=4):
    """[(seed, i, j, S)]: ordered pairs of volumes of one call whose sets of `a` over idx < S could be equal.  A set equality needs EVERY
    element of volume i to be in volume j's set; a(i, idx) = mix32(m) with m = mix32(idx ^ k0_i) + k1_i lies in volume j's set iff
    unmix32(m - k1_j) ^ k0_j < S, which costs one inverse round per pair.  Index 0 settles all but about S / 2^32 of the pairs, the few left
    are asked about index 1, 2, ...; a pair that survives `probes` indices is reported (none does).  c is a function of (a, k1, idx_hi)."""
    vol = np.arange(B, dtype=np.uint32)
    iu, ju = np.triu_indices(B, 1)                                   # equality is symmetric: i < j is enough
    smax = max(sizes)
    hits = []
    seeds = list(seeds)
    for s0 in range(0, len(seeds), 128):
        chunk = seeds[s0:s0 + 128]
        k0 = np.stack([keys(s, vol)[0] for s in chunk])             # [n, B]
        k1 = np.stack([keys(s, vol)[1] for s in chunk])
        with np.errstate(over="ignore"):
            m = mix32(_u32(0) ^ k0) + k1                             # element 0 of every volume, before the last round
            back = unmix32(m[:, iu] - k1[:, ju]) ^ k0[:, ju]         # [n, pair]: the index at which volume j would hold it
        for n, p in zip(*np.nonzero(back < smax)):
            i, j = iu[p], ju[p]
            for S in sizes:
                alive = True
                for p in range(probes):
                    with np.errstate(over="ignore"):
                        mp = mix32(_u32(p) ^ k0[n, i]) + k1[n, i]
                        alive = alive and int(unmix32(mp - k1[n, j]) ^ k0[n, j]) < S
                if alive:
                    hits.append((chunk[n], int(i), int(j), S))
    return hits


# (S, B, seed): 4096 = 16 blocks; CAP_ITEMS - 1, CAP_ITEMS, CAP_ITEMS + 77: one element short of the cap, the cap, 77 elements in a second stride
NOISE_SEEDS = [0, 1 << 31, 1 << 32, (1 << 61) + 5, 5]               # 0 / 2^32 and 5 / 2^61 + 5 differ in the high word only
NOISE_CASES = [(4096, 5, s) for s in NOISE_SEEDS] + [(4096, 1, 5)]
NOISE_CASES += [(CAP_ITEMS - 1, 1, 0), (CAP_ITEMS, 1, (1 << 61) + 5), (CAP_ITEMS + 77, 1, 1 << 32), (CAP_ITEMS + 77, 5, 1 << 31)]
COLLISIONS_V1 = [(262, 64, 4096, 14, 60, 638), (4, 64, 131072, 0, 40, 77283)]            # (seed, B, S, i, j, K) of the hash before the fix

# the gamma map alone (std = 0): negative, both zeros, one, tiny and large (no subnormal and no infinite result: 2^-120 .. 2^80 with gamma = 2)
GAMMA_X = np.array([-3.5, -1.0, -0.0, 0.0, 1.0, 2.0 ** -60, 1.0e-15, 0.37, 1.7, 1.0e15, -2.0 ** 40, 255.0], dtype=np.float32)
GAMMA_G = np.array([0.7408182, 1.0, 1.3498588, 0.5, 2.0], dtype=np.float32)


def gamma64(v, g):
    v = v.astype(np.float64)
    return np.copysign(np.abs(v) ** g.astype(np.float64), v)


def gamma32(v, g):
    return np.copysign(np.power(np.abs(v), g, dtype=np.float32), v).astype(np.float32)


# ========================================================================================================================================
# volume minimum
# ========================================================================================================================================
MIN_SIZES = [1, 63, 64, 1023, 1024, 1025, 2049]


def min_positions(S):
    """where the minimum is put, one volume each: an element of every wave that owns one (thread t = i % 1024 reads element i, wave t / 64;
    the lane walks with the wave), the first and the last element"""
    pos = {0, S - 1}
    for w in range(RED_THREADS // 64):
        p = w * 64 + (7 * w + 3) % 64
        if p < S:
            pos.add(p)
        if p + RED_THREADS < S:
            pos.add(p + RED_THREADS)               # the same wave's second stride
    return sorted(pos)


def min_volumes(S, seed=0):
    """[len(positions), S] float32: distinct values 1 .. S in a random order, -5 at the volume's position"""
    pos = min_positions(S)
    g = torch.Generator().manual_seed(seed + S)
    x = torch.stack([torch.randperm(S, generator=g).float() + 1 for _ in pos])
    for b, p in enumerate(pos):
        x[b, p] = -5.0
    return x


# ========================================================================================================================================
# affine
# ========================================================================================================================================
AFFINE_EXTENTS = [(4, 6, 8), (5, 7, 3), (12, 10, 6), (16, 16, 16)]
DATA_MAX = 64                    # |v| <= 64, integers
FILL_BASE = -100                 # fill[b] = -100 - b: negative, distinct from every voxel and from every other volume's


def signed_permutations():
    out = []
    for p in itertools.permutations(range(3)):
        for s in itertools.product((1.0, -1.0), repeat=3):
            m = torch.zeros(3, 3, dtype=torch.float64)
            for r in range(3):
                m[r, p[r]] = s[r]
            out.append(m)
    return out


def affine_matrices():
    """[(name, [3,3] float64)]: every entry a multiple of 1/8"""
    eye = torch.eye(3, dtype=torch.float64)
    ms = [("identity", eye)]
    ms += [(f"signed permutation {k}", m) for k, m in enumerate(signed_permutations()) if not torch.equal(m, eye)]
    ms.append(("diag(7/8, 9/8, 5/4)", torch.diag(torch.tensor([7 / 8, 9 / 8, 5 / 4], dtype=torch.float64))))
    ms.append(("shear 1/8", torch.tensor([[1, 1 / 8, 0], [0, 1, 1 / 8], [1 / 8, 0, 1]], dtype=torch.float64)))
    ms.append(("shear -1/8, 3/8", torch.tensor([[1, 0, -1 / 8], [3 / 8, 1, 0], [0, -1 / 8, 7 / 8]], dtype=torch.float64)))
    ms.append(("scale 2^20", eye * 2.0 ** 20))
    ms.append(("zoom out 3", eye * 3.0))
    return ms


def affine_case(dhw, seed=0):
    """-> x [B,D,H,W] float32 integers, flip int32 [B], inv float32 [B,3,3], fill float32 [B]: every matrix with flip 0 and with flip 1, a
    different matrix, fill and volume per b (a kernel that reads inv, flip or fill of another volume gets another result)"""
    ms = affine_matrices()
    B = 2 * len(ms)
    g = torch.Generator().manual_seed(seed + sum(dhw))
    x = torch.randint(-DATA_MAX, DATA_MAX + 1, (B,) + tuple(dhw), generator=g).float()
    inv = torch.stack([m for _, m in ms] * 2).float().contiguous()
    flip = torch.cat([torch.zeros(len(ms)), torch.ones(len(ms))]).to(torch.int32)
    fill = (FILL_BASE - torch.arange(B)).float()
    names = [f"{n}, flip {f}" for f in (0, 1) for n, _ in ms]
    return x, flip, inv, fill, names


def affine_f32(x, flip, inv, fill, reverse=False):
    """affine_kernel operation by operation in numpy float32, WITHOUT fused multiply-adds; `reverse` walks the corners and the three coordinate
    products in the opposite order.  On the lattice it equals the float64 reference in both orders."""
    f = np.float32
    x, inv, fill = x.numpy().astype(f), inv.numpy().astype(f), fill.numpy().astype(f)
    B, D, H, W = x.shape
    d, h, w = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    cd, ch, cw = (d.astype(f) + f(0.5) - f(0.5) * f(D)), (h.astype(f) + f(0.5) - f(0.5) * f(H)), (w.astype(f) + f(0.5) - f(0.5) * f(W))
    out = np.zeros_like(x)
    for b in range(B):
        m = inv[b].reshape(9)
        rows = []
        for r, ext in enumerate((D, H, W)):
            terms = [m[3 * r] * cd, m[3 * r + 1] * ch, m[3 * r + 2] * cw, np.full_like(cd, f(0.5) * f(ext) - f(0.5))]
            if reverse:
                terms = terms[::-1]
            s = terms[0]
            for t in terms[1:]:
                s = (s + t).astype(f)
            rows.append(s)
        sd, sh, sw = rows
        if flip[b]:
            sd = (f(D - 1) - sd).astype(f)
        fd, fh, fw = np.floor(sd), np.floor(sh), np.floor(sw)
        td, th, tw = sd - fd, sh - fh, sw - fw
        acc = np.zeros_like(sd)
        corners = list(itertools.product((0, 1), repeat=3))
        for a, bb, c in (corners[::-1] if reverse else corners):
            dd, hh, ww = fd.astype(np.int64) + a, fh.astype(np.int64) + bb, fw.astype(np.int64) + c
            inside = (dd >= 0) & (dd < D) & (hh >= 0) & (hh < H) & (ww >= 0) & (ww < W)
            val = np.where(inside, x[b][dd.clip(0, D - 1), hh.clip(0, H - 1), ww.clip(0, W - 1)], fill[b]).astype(f)
            t = (val * (td if a else f(1) - td)).astype(f)
            t = (t * (th if bb else f(1) - th)).astype(f)
            t = (t * (tw if c else f(1) - tw)).astype(f)
            acc = (acc + t).astype(f)
        out[b] = acc
    return out


# ========================================================================================================================================
# blur
# ========================================================================================================================================
BLUR_EXTENTS = [(6, 5, 4), (33, 3, 2), (2, 40, 3), (3, 2, 33), (16, 16, 16)]
BLUR_RADII = [0, 8, 32]
BLUR_SIGMAS = [0.0, 1e-4, 0.4, 1.0, 1.9, 7.3]            # one per volume: the first two are under the 1e-3 floor (identity)
EXP_ULPS = 3                                             # the OpenCL C bound for exp, which the device library documents to meet


def blur_data(dhw, seed=0):
    """[B,D,H,W] float32: signed, a few voxels 100 times larger, so the bound is not flat"""
    g = torch.Generator().manual_seed(seed + 7 * sum(dhw))
    x = torch.randn((len(BLUR_SIGMAS),) + tuple(dhw), generator=g)
    big = torch.rand(x.shape, generator=g) < 0.03
    return torch.where(big, x * 100.0, x).float()


def _gather_taps(x, axis, r):
    """x [B,D,H,W] numpy -> [2r+1, B,D,H,W]: x at pos + k along axis, reflected as the kernel reflects (edge value repeated once)"""
    n = x.shape[axis + 1]
    pos = np.arange(n)
    out = []
    for k in range(-r, r + 1):
        q = pos + k
        q = np.where(q < 0, -1 - q, np.where(q >= n, 2 * n - 1 - q, q))
        out.append(np.take(x, q, axis=axis + 1))
    return np.stack(out)


def blur_axis_f32(x, sigma, axis, radius):
    """blur_axis_kernel operation by operation in numpy float32 (no fused multiply-add): the yardstick"""
    f = np.float32
    x = x.numpy().astype(f)
    n = x.shape[axis + 1]
    r = min(radius, n)
    s = np.maximum(sigma.numpy().astype(f), SIGMA_FLOOR)                               # [B]
    t = np.arange(-r, r + 1).astype(f)[:, None]
    q = (t / s[None, :]).astype(f)
    wt = np.exp(((f(-0.5) * q).astype(f) * q).astype(f)).astype(f)                      # [2r+1, B]
    norm = np.zeros_like(s)
    for k in range(2 * r + 1):
        norm = (norm + wt[k]).astype(f)
    taps = _gather_taps(x, axis, r)
    acc = np.zeros_like(x)
    for k in range(2 * r + 1):
        acc = (acc + (wt[k].reshape(-1, 1, 1, 1) * taps[k]).astype(f)).astype(f)
    return (acc / norm.reshape(-1, 1, 1, 1)).astype(f)


def blur_axis_bound(x, sigma, axis, radius):
    """-> (y64, bound, A): the float64 value of one pass, the bound on |kernel - y64| per element, and A = sum_k |w_k v_q| / sum_k w_k.

    The kernel computes w~_k = expf(fl(fl(-0.5 q~) q~)), q~ = fl(t / s), then N~ = sum_k w~_k v_q and D~ = sum_k w~_k in float32 (any order,
    fused or not) and y~ = fl(N~ / D~).  With u = 2^-24:
      q~ = q (1 + d1), the exponent z~ = z (1 + d1)^2 (1 + d2) has relative error <= 3u, so exp(z~) = w_k exp(z * 3u'): relative error
      |z| 3u = 1.5 q^2 u; expf adds EXP_ULPS ulp <= 2 EXP_ULPS u.   w~_k = w_k (1 + e_k u'), e_k = 1.5 q_k^2 + 2 EXP_ULPS   (+ 2^-149 absolute
      where the weight is subnormal).  w_k e_k is largest at q^2 = 2, where q^2 exp(-q^2 / 2) peaks: the weight term never exceeds 1.11 u |v|
      per tap next to the centre tap's weight 1.
      A sum of n = 2r + 1 terms carries (1 + th_k), |th_k| <= n u per term (products included when fused, n + 1 when not: n + 1 is used).
      y~ - y = [sum_k w_k v_q (e_k + n + 1) u'] / D  -  y [sum_k w_k (e_k + n) u''] / D  +  y u'''      (first order)
      |y~ - y| <= u ( sum_k |w_k v_q| (e_k + n + 1) / D  +  A (sum_k w_k e_k / D + n + 1) ),   |y| <= A.
    The second-order terms are below (100 u)^2; the bound is multiplied by 1 + 2^-10 for them."""
    x = x.numpy().astype(np.float64)
    n_ext = x.shape[axis + 1]
    r = min(radius, n_ext)
    n = 2 * r + 1
    s = np.maximum(sigma.numpy().astype(np.float32), SIGMA_FLOOR).astype(np.float64)
    q = np.arange(-r, r + 1, dtype=np.float64)[:, None] / s[None, :]
    w = np.exp(-0.5 * q * q)                                                            # [n, B]
    e = 1.5 * q * q + 2 * EXP_ULPS
    we = w * e + 2.0 ** -149 / U
    Dn = w.sum(0).reshape(-1, 1, 1, 1)
    taps = _gather_taps(x, axis, r)
    sh = (n, -1, 1, 1, 1)
    y = (w.reshape(sh) * taps).sum(0) / Dn
    A = (w.reshape(sh) * np.abs(taps)).sum(0) / Dn
    first = ((we + w * (n + 1)).reshape(sh) * np.abs(taps)).sum(0) / Dn
    second = A * (we.sum(0).reshape(-1, 1, 1, 1) / Dn + n + 1)
    return y, U * (first + second) * (1 + 2.0 ** -10), A


def blur_is_identity(sigma, radius):
    """per volume: radius 0, or sigma under the floor (exp(-0.5 / 1e-6) = 0 in float32 and in float64)"""
    return (sigma <= 1e-3) | (radius == 0)


def scipy_tail_mass(sigma, radius=8):
    """2 sum_{R < t <= radius} w(t) / sum_{|t| <= radius} w(t), R = int(4 sigma + 0.5): the weight the kernel's fixed radius keeps and scipy's
    truncation at 4 sigma drops.  The two results differ by at most this times the data range, per axis:
      y8 - yR = (T / W8) (mean of v over the tail taps, weighted - yR), both in [min v, max v]."""
    t = np.arange(-radius, radius + 1, dtype=np.float64)
    w = np.exp(-0.5 * (t / max(float(sigma), 1e-3)) ** 2)
    Rs = int(4.0 * float(sigma) + 0.5)
    return float(w[np.abs(t) > Rs].sum() / w.sum())


SCIPY_STEPS = [(k - 0.5) / 4 for k in range(1, 9)]        # sigma at which int(4 sigma + 0.5) becomes k


# ========================================================================================================================================
# mean / rstd, z-normalisation
# ========================================================================================================================================
def meanstd_cases():
    """[(name, x [B, S] float32)]"""
    g = torch.Generator().manual_seed(11)
    rn = lambda *s: torch.randn(*s, generator=g)
    return [
        ("S = 1", torch.tensor([[0.3], [-7.25], [1e10]])),
        ("S = 2", rn(3, 2)),
        ("S = 63", rn(3, 63) * 3 + 1),
        ("S = 1025", rn(3, 1025) * 0.1 - 2),
        ("constant 0.75, S = 1025", torch.full((3, 1025), 0.75)),          # dyadic: every double sum is exact, the variance is exactly 0
        ("constant -3, S = 63", torch.full((1, 63), -3.0)),
        ("mean / std = 1000, S = 1025", 1000.0 + rn(3, 1025)),
        ("mean / std = 1000, S = 4096 + 5", 250.0 + 0.25 * rn(1, 4101)),
        ("B = 1, S = 1024", rn(1, 1024)),
    ]


def meanstd_one_pass64(x):
    """meanstd_kernel in numpy float64 (sequential sums): what the bound is checked against on the CPU"""
    x = x.numpy().astype(np.float64)
    S = x.shape[1]
    s1, s2 = np.zeros(x.shape[0]), np.zeros(x.shape[0])
    for i in range(S):
        s1 += x[:, i]
        s2 += x[:, i] * x[:, i]
    m = s1 / S
    var = (s2 - s1 * m) / max(S - 1, 1)
    return m.astype(np.float32), (1.0 / np.maximum(np.sqrt(np.maximum(var, 0.0)), 1e-12)).astype(np.float32)


def meanstd_bounds(x):
    """-> (mean64, tau, rstd64, rel): the exactly rounded float64 mean (math.fsum), the relative slack tau of the kernel's double mean, the
    float64 1 / std from a two-pass evaluation, and the relative bound on the kernel's rstd.

    mean: s1^ = s1 + g_S sum|x| (any order, g_n = n eps), m^ = s1^ / S (1 + eps): |m^ - m| <= tau |m|, tau = (S + 1) eps sum|x| / |sum x|.  The
      kernel's float32 mean is the float32 rounding of some value within tau of m: the float32 rounding of m itself unless m sits within tau
      of a rounding boundary, where the neighbour is as good.
    rstd: s2^ = s2 + (S + 1) eps sum x^2 (the squares of float32 values are exact in double), s1^ m^ = s1 m + (2S + 2) eps (sum|x|)^2 / S
      <= (2S + 2) eps sum x^2 (Cauchy-Schwarz), one more eps for the subtraction (none when fused): the numerator (S - 1) var is off by at most
      (3S + 4) eps sum x^2, var relatively by k = (3S + 4) eps sum x^2 / ((S - 1) var), rstd by k / 2 (first order; (1 - k)^-1/2 - 1 is
      used), then sqrt, the reciprocal and the division by S - 1 (3 eps) and ONE float32 rounding (2^-24).
      A variance of exactly 0 (S = 1, a dyadic constant) gives 1e12."""
    x64 = x.numpy().astype(np.float64)
    B, S = x64.shape
    mean, tau, rstd, rel = [], [], [], []
    for b in range(B):
        v = x64[b]
        s = math.fsum(v)
        m = s / S
        sabs, ssq = math.fsum(np.abs(v)), math.fsum(v * v)
        mean.append(m)
        tau.append((S + 1) * EPS * sabs / abs(s) if s != 0 else math.inf)
        var = math.fsum((v - m) ** 2) / max(S - 1, 1)
        if var == 0.0:
            rstd.append(1e12)
            rel.append(U)
            continue
        k = (3 * S + 4) * EPS * ssq / (max(S - 1, 1) * var)
        assert k < 0.5, "the case is too ill-conditioned for a first-order bound"
        rstd.append(1.0 / math.sqrt(var))
        rel.append(((1 - k) ** -0.5 - 1) + 3 * EPS + U * (1 + 2.0 ** -10))
    return np.array(mean), np.array(tau), np.array(rstd), np.array(rel)


ZNORM_SIZES = [(1, 3), (257, 3), (CAP_ITEMS + 77, 2)]      # (S, B)


# ========================================================================================================================================
# swap
# ========================================================================================================================================
def swap_cases():
    """[(name, dhw, patch, origins [iters][B][2][3])]; disjoint patches only, or equal corners (the host's contract)"""
    O = lambda *its: torch.tensor(its, dtype=torch.int32)
    cases = [
        ("corners equal: no-op", (8, 8, 8), (2, 3, 4), O([[[1, 2, 3], [1, 2, 3]]], [[[0, 0, 0], [0, 0, 0]]])),
        ("touching in d", (8, 8, 8), (2, 3, 4), O([[[0, 1, 2], [2, 1, 2]]])),
        ("touching in h", (8, 8, 8), (2, 3, 4), O([[[3, 0, 1], [3, 3, 1]]])),
        ("touching in w", (8, 8, 8), (2, 3, 4), O([[[5, 4, 0], [5, 4, 4]]])),
        ("touching at the far corner", (10, 12, 10), (5, 6, 5), O([[[0, 0, 0], [5, 6, 5]]])),
        ("patch = whole volume (corners can only be equal)", (8, 8, 8), (8, 8, 8), O([[[0, 0, 0], [0, 0, 0]]])),
        ("P = 255", (6, 5, 17), (3, 5, 17), O([[[0, 0, 0], [3, 0, 0]]])),
        ("P = 256", (8, 8, 8), (4, 8, 8), O([[[4, 0, 0], [0, 0, 0]]])),
        ("P = 257", (2, 1, 257), (1, 1, 257), O([[[0, 0, 0], [1, 0, 0]]])),
        ("P = 600", (10, 12, 10), (5, 12, 10), O([[[0, 0, 0], [5, 0, 0]]])),
        ("P = 300, three steps", (10, 12, 10), (3, 10, 10), O([[[0, 0, 0], [3, 1, 0]]], [[[3, 1, 0], [7, 2, 0]]], [[[7, 2, 0], [3, 1, 0]]])),
        # step 2 moves the voxels step 1 placed at B on to C, step 3 brings them back; then A <-> B again restores the input
        ("chain A<->B, B<->C, C<->B", (8, 8, 8), (2, 2, 2), O([[[0, 0, 0], [4, 4, 4]]], [[[4, 4, 4], [6, 1, 2]]], [[[6, 1, 2], [4, 4, 4]]])),
        ("B = 3, different corners, a no-op in the middle", (10, 12, 10), (2, 3, 4),
         O([[[0, 0, 0], [2, 0, 0]], [[8, 9, 6], [0, 0, 0]], [[4, 4, 4], [4, 4, 4]]],
           [[[2, 0, 0], [2, 3, 0]], [[1, 1, 1], [1, 1, 1]], [[0, 9, 0], [8, 0, 6]]],
           [[[1, 1, 1], [5, 5, 5]], [[3, 3, 3], [3, 6, 3]], [[0, 0, 0], [0, 0, 4]]])),
    ]
    return cases


def boxes_overlap(a, b, patch):
    """two patches share a voxel: on every axis the half-open intervals [a, a + p) and [b, b + p) intersect (max of the starts < min of the ends)"""
    return all(max(int(a[k]), int(b[k])) < min(int(a[k]), int(b[k])) + patch[k] for k in range(3))
