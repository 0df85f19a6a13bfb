"""GPU: every kernel of csrc/augment.hip alone, through its pcrl_aug_* entry point with its coefficients as inputs, at the sizes where its loops
turn over (tests/aug_cases.py holds the case table, the lattices and the restatements; tests/test_aug_cases_cpu.py their preconditions).

  entry           compared with                                                   bound                      measured on gfx950
  aug_volume_min  the minimum (fminf: a NaN is ignored, zeros of either sign)      bits                       equal in every case
  aug_affine      aug_reference.ref_spatial, float64, dyadic lattice                bits                       equal in every case
  aug_blur_axis   aug_reference.ref_blur, float64                                   bits (identity, radius 0)  equal
                                                                                    else blur_axis_bound()     <= 0.123 x the bound
  aug_noise_gamma float64 Box-Muller on the bit-exact hash                          4 x float32 yardstick      1.02 .. 1.34 x the yardstick
                  float64 sign(v) |v|^gamma                                         4 x float32 yardstick      0.90 x the yardstick
  aug_meanstd     exactly rounded float64 mean; two-pass float64 1 / std            meanstd_bounds()           mean exact; rstd <= 4.5e-8 relative
  aug_znorm       numpy float32 (x - m) * r                                         bits                       equal in every case
  aug_swap        aug_reference.ref_swap                                            bits                       equal in every case
  refusals (53)   PcrlError, the outputs keep their sentinel

Parity with torchio's affine and its random streams stays unpinned; the blur's definition is held to scipy's within the tail mass on the CPU."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import aug_cases as A  # noqa: E402
import aug_reference as R  # noqa: E402
from exact_lattice import assert_bit_equal  # noqa: E402
from pcrlv2_amd._lib import PcrlError, lib, stream_handle  # noqa: E402

DEV = "cuda"
SENTINEL = 7.0


def call(name, *args):
    lib().call(name, *args, stream_handle())


def sentinel(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.float32, device=DEV)


def same_bits(got, want, what, zeros_of_either_sign=False):
    """got (device float32) equals want (CPU float32 tensor or array) in bits"""
    got = got.detach().cpu().contiguous()
    want = torch.as_tensor(np.asarray(want)).contiguous()
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, f"{what}: {got.shape} {got.dtype} against {want.shape} {want.dtype}"
    bad = got.view(torch.int32) != want.view(torch.int32)
    if zeros_of_either_sign:
        bad &= ~((got == 0) & (want == 0))
    n = int(bad.sum())
    if n:
        idx = bad.nonzero()[:6].tolist()
        raise AssertionError(f"{what}: {n} of {got.numel()} elements differ; first " + ", ".join(f"{tuple(i)}: got {got[tuple(i)].item()!r} want {want[tuple(i)].item()!r}" for i in idx))


# ----------------------------------------------------------------------------------------------------------------------------------------
# 1. volume minimum
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", A.MIN_SIZES)
def test_volume_min_at_every_owner_of_the_minimum(S):
    """vol_min_kernel: one block of 1024 threads per volume, thread t reads elements t, t + 1024, ...; 16 wave minima meet in LDS.  S = 1, 63, 64:
    fewer elements than threads (idle lanes and idle waves hold +inf); 1023, 1024, 1025, 2049: the last partial stride.  One volume per place
    the minimum can sit (an element of each wave, in the first and in the second stride, element 0, element S - 1); then B = 1 and B = 3;
    zeros of both signs; one NaN among finite values.  Measured: bits in every case."""
    x = A.min_volumes(S)
    Bp = x.shape[0]
    out = sentinel(Bp + 2)
    call("pcrl_aug_volume_min", x.to(DEV), out, Bp, S)
    same_bits(out[:Bp], torch.full((Bp,), -5.0), f"minimum at {A.min_positions(S)}, S={S}")
    assert (out[Bp:] == SENTINEL).all()
    for B in (1, 3):
        g = torch.Generator().manual_seed(S + B)
        v = torch.randn(B, S, generator=g)
        out = sentinel(B + 1)
        call("pcrl_aug_volume_min", v.to(DEV), out, B, S)
        same_bits(out[:B], v.amin(1), f"B={B} S={S}")
        assert out[B].item() == SENTINEL
    if S < 2:
        return
    pos = A.min_positions(S)
    z = torch.zeros(2 * len(pos), S)
    for k, p in enumerate(pos):
        z[k, p] = -0.0                                  # -0 among +0
        z[len(pos) + k] = -0.0
        z[len(pos) + k, p] = 0.0                        # +0 among -0
    out = sentinel(z.shape[0])
    call("pcrl_aug_volume_min", z.to(DEV), out, z.shape[0], S)
    same_bits(out, torch.zeros(z.shape[0]), f"zeros S={S}", zeros_of_either_sign=True)
    n = A.min_volumes(S, seed=1)
    for k, p in enumerate(pos):
        n[k, (p + 1) % S] = float("nan")               # next to the minimum: same wave
        n[k, (p + S // 2) % S if (p + S // 2) % S != p else (p + 1) % S] = float("nan")
    out = sentinel(n.shape[0])
    call("pcrl_aug_volume_min", n.to(DEV), out, n.shape[0], S)
    same_bits(out, np.fmin.reduce(n.numpy(), axis=1), f"NaN among finite values S={S}")


# ----------------------------------------------------------------------------------------------------------------------------------------
# 2. affine
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dhw", A.AFFINE_EXTENTS)
def test_affine_bit_for_bit_on_the_dyadic_lattice(dhw):
    """affine_kernel on inverse matrices with entries k/8 and integer data: identity, the 47 other signed axis permutations (unequal extents
    mapped onto each other: large outside regions), diag(7/8, 9/8, 5/4), two shears, scale 2^20 (everything outside but the centre voxel of
    an odd volume), zoom-out 3; each with flip 0 and 1; fill[b] = -100 - b (negative, distinct from every voxel and per volume); one call of
    B = 106 with a different matrix per volume, then B = 3 and B = 1.  Even extents put the centre on a half-integer.  S = 192, 105, 720 are
    no multiples of 256.  Measured: bits in every case."""
    x, flip, inv, fill, names = A.affine_case(dhw)
    B = x.shape[0]
    ref = R.ref_spatial(x, flip, inv, fill)
    xd = x.to(DEV)
    y = sentinel(B + 1, *dhw)
    call("pcrl_aug_affine", xd, y, inv.to(DEV), flip.to(DEV), fill.to(DEV), B, *dhw)
    assert (y[B] == SENTINEL).all() and torch.equal(xd.cpu(), x)
    got = y[:B].cpu()
    for b in range(B):                                                       # per volume: the message names the transform
        assert_bit_equal(got[b], ref[b], torch.float32, f"affine {dhw} volume {b}: {names[b]}")
    half = B // 2
    for pick in ([half + 3, 1, B - 3], [B - 4]):                              # B = 3 (flip 1 first) and B = 1
        n = len(pick)
        y = sentinel(n + 1, *dhw)
        call("pcrl_aug_affine", x[pick].to(DEV), y, inv[pick].to(DEV), flip[pick].to(DEV), fill[pick].to(DEV), n, *dhw)
        assert_bit_equal(y[:n], ref[pick], torch.float32, f"affine {dhw} B={n} volumes {pick}")
        assert (y[n] == SENTINEL).all()


# ----------------------------------------------------------------------------------------------------------------------------------------
# 3. blur
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("dhw", A.BLUR_EXTENTS)
def test_blur_axis_alone(dhw, axis):
    """blur_axis_kernel, one axis, radius 0, 8 and 32, six volumes with sigma 0, 1e-4 (under the 1e-3 floor: identity), 0.4, 1, 1.9 and 7.3.
    Three unequal extents per shape catch an extent or stride taken from another axis; n = 33 and n = 40 at radius 32 use all 65 weights;
    n = 2 .. 6 clip the radius to n, where every tap of a border voxel is a reflected one.
    Identity volumes and radius 0: bits.  Otherwise |y - ref_blur| <= blur_axis_bound() (derived there: float32 accumulation of 2r + 1 products
    and of the norm, the division, expf within 3 ulp and the rounding of t / s before squaring), which is at most 156 x 2^-24 x sum|w v| / norm
    (radius 32, sigma 7.3).  Measured on gfx950: err / bound at most 0.123 over the 45 launches (0.064 .. 0.123 per shape and axis;
    CPU float32 yardstick: 0.130)."""
    x = A.blur_data(dhw)
    sig = torch.tensor(A.BLUR_SIGMAS, dtype=torch.float32)
    B = x.shape[0]
    xd, sd = x.to(DEV), sig.to(DEV)
    worst = 0.0
    for radius in A.BLUR_RADII:
        y = sentinel(B + 1, *dhw)
        call("pcrl_aug_blur_axis", xd, y, sd, B, *dhw, axis, radius)
        assert (y[B] == SENTINEL).all()
        got = y[:B].cpu()
        sigma3 = torch.zeros(3, B)
        sigma3[axis] = sig
        ref = R.ref_blur(x, sigma3, radius=radius).numpy()
        _, bound, _ = A.blur_axis_bound(x, sig, axis, radius)
        ident = A.blur_is_identity(sig.numpy(), radius)
        same_bits(got[ident], x[ident], f"blur {dhw} axis {axis} radius {radius}: identity volumes")
        err = np.abs(got.numpy().astype(np.float64) - ref)
        ratio = float((err / bound).max())
        worst = max(worst, ratio)
        print(f"  blur {dhw} axis {axis} radius {radius}: max err {err.max():.3e}, err / bound {ratio:.3f}")
        assert (err <= bound).all(), f"blur {dhw} axis {axis} radius {radius}: err / bound = {ratio:.3f} at {np.unravel_index((err / bound).argmax(), err.shape)}"
    assert torch.equal(xd.cpu(), x)
    print(f"  blur {dhw} axis {axis}: worst err / bound {worst:.3f}")


# ----------------------------------------------------------------------------------------------------------------------------------------
# 4. noise and gamma
# ----------------------------------------------------------------------------------------------------------------------------------------
def _noise(S, B, seed, x=None, std=None, gamma=None):
    x = torch.zeros(B, S, device=DEV) if x is None else x
    std = torch.ones(B, device=DEV) if std is None else std
    gamma = torch.ones(B, device=DEV) if gamma is None else gamma
    y = sentinel(B * S + 1)
    call("pcrl_aug_noise_gamma", x, y, std, gamma, B, S, seed)
    assert y[B * S].item() == SENTINEL
    return y[:B * S].view(B, S)


@pytest.mark.parametrize("S,B,seed", A.NOISE_CASES)
def test_the_deviate_alone(S, B, seed):
    """x = 0, std = 1, gamma = 1: y is the deviate.  Reference: float64 sqrt(-2 log u1) cos(angle) on the restated hash (u1, u2 and the float32
    angle formed as the kernel forms them).  Bound: 4 x the error of the float32 numpy evaluation, both scaled by max(1, |n|).  A wrong hash
    constant, shift or operand gives differences of order 1.  S = 262 143, 262 144, 262 221: one short of the 1024-block cap, the cap, and 77
    elements into the second grid stride; seeds 0, 2^31, 2^32, 2^61 + 5 and 5.
    Measured on gfx950: err 1.8e-7 .. 2.5e-7 against yardsticks of 1.6e-7 .. 2.0e-7 (ratio 1.02 .. 1.34, bound 4): logf, cosf and
    sqrtf of the device library are as good as numpy's float32 ones here."""
    got = _noise(S, B, seed).cpu().numpy().astype(np.float64)
    a, c = A.noise_field(seed, B, S)
    n64 = A.deviate64(a, c)
    scale = np.maximum(1.0, np.abs(n64))
    yard = float((np.abs(A.deviate32(a, c).astype(np.float64) - n64) / scale).max())
    err = float((np.abs(got - n64) / scale).max())
    print(f"  deviate S={S} B={B} seed={seed}: err {err:.3e}, float32 yardstick {yard:.3e}, ratio {err / yard:.2f}")
    assert err <= 4 * yard, f"S={S} B={B} seed={seed}: {err:.3e} > 4 x {yard:.3e}"


def test_seeds_that_differ_in_the_high_word_give_other_fields():
    for lo, hi in ((0, 1 << 32), (5, (1 << 61) + 5)):
        y0, y1 = _noise(4096, 5, lo), _noise(4096, 5, hi)
        assert (y0 == y1).float().mean().item() < 0.01
        assert not torch.equal(y0.abs().sort(1).values, y1.abs().sort(1).values)


@pytest.mark.parametrize("seed,B,S,i,j,K", A.COLLISIONS_V1)
def test_no_two_volumes_of_a_call_get_the_same_field(seed, B, S, i, j, K):
    """The calls at which the one-key hash gave volumes i and j the same deviates, permuted by idx ^ K (seed 262: 14 and 60 at S = 4096; seed 4:
    0 and 40 at S = 131 072).  With the second key no two of the 64 volumes share their sorted values."""
    y = _noise(S, B, seed)
    s = y.sort(1).values
    assert not torch.equal(s[i], s[j]), f"volumes {i} and {j} hold the same deviates"
    assert not torch.equal(y[i], y[j][(torch.arange(S, device=DEV) ^ K)])
    assert torch.unique(s[:, :: max(S // 64, 1)], dim=0).shape[0] == B                    # 64 order statistics tell all volumes apart
    c = torch.corrcoef(torch.stack([y[i], y[j], y[j][(torch.arange(S, device=DEV) ^ K)]]))
    assert c[0, 1].abs().item() < 0.08 and c[0, 2].abs().item() < 0.08


def test_the_gamma_map_alone():
    """std = 0: y = sign(x) |x|^gamma, gamma per volume (0.74, 1, 1.35, 0.5, 2), x negative, -0, +0, 1, 2^-60, 1e-15, 1e15, -2^40 (no subnormal
    or infinite result), S = 300 (two blocks).  Reference float64; bound 4 x the relative error of numpy's float32 power (8.7e-8); a zero stays a
    zero (0 * n may be -0 and -0 + 0 is +0: either sign).  Measured on gfx950: 7.8e-8 relative (0.90 x the yardstick)."""
    B, S = len(A.GAMMA_G), 300
    xr = np.tile(A.GAMMA_X, S // len(A.GAMMA_X))[None, :].repeat(B, 0)
    g = A.GAMMA_G[:, None]
    got = _noise(S, B, 99, x=torch.from_numpy(xr).to(DEV), std=torch.zeros(B, device=DEV), gamma=torch.from_numpy(A.GAMMA_G).to(DEV)).cpu().numpy()
    r64 = A.gamma64(xr, g)
    nz = r64 != 0
    yard = float((np.abs(A.gamma32(xr, g).astype(np.float64) - r64)[nz] / np.abs(r64[nz])).max())
    err = float((np.abs(got.astype(np.float64) - r64)[nz] / np.abs(r64[nz])).max())
    print(f"  gamma map: relative err {err:.3e}, float32 yardstick {yard:.3e}, ratio {err / yard:.2f}")
    assert (got[~nz] == 0).all() and (np.signbit(got[nz]) == np.signbit(r64[nz])).all()
    assert err <= 4 * yard


# ----------------------------------------------------------------------------------------------------------------------------------------
# 5. mean and 1 / std
# ----------------------------------------------------------------------------------------------------------------------------------------
def test_meanstd_to_the_derived_bounds():
    """meanstd_kernel: double one-pass sums over 1024 threads.  S = 1 (variance 0: rstd = 1e12, finite), 2, 63, 1025, dyadic constants (the
    variance clamps at exactly 0), mean / std = 1000 (the cancellation in s2 - s1 m), B = 1 and 3.
    mean: the float32 rounding of the exactly rounded float64 mean (or its neighbour where that mean is within the double round-off
    (S + 1) 2^-53 sum|x| / |sum x| of a rounding boundary).  rstd: relative 2^-24 + k / 2 + 3 x 2^-53, k = (3S + 4) 2^-53 sum x^2 / ((S - 1) var):
    the one-pass formula's double round-off in any summation order, plus one float32 rounding (derivation: aug_cases.meanstd_bounds).
    Measured on gfx950: the mean is the rounded float64 mean in every case; rstd relative error 2.8e-9 .. 4.4e-8 against bounds of 6.0e-8 (well
    conditioned), 2.4e-7 (mean / std = 1000, S = 1025) and 7.5e-7 (S = 4101)."""
    for name, x in A.meanstd_cases():
        B, S = x.shape
        m64, tau, r64, rel = A.meanstd_bounds(x)
        mean, rstd = sentinel(B + 1), sentinel(B + 1)
        call("pcrl_aug_meanstd", x.to(DEV), mean, rstd, B, S)
        assert mean[B].item() == SENTINEL and rstd[B].item() == SENTINEL
        m, r = mean[:B].cpu().numpy(), rstd[:B].cpu().numpy()
        lo, hi = (m64 - np.abs(m64) * tau).astype(np.float32), (m64 + np.abs(m64) * tau).astype(np.float32)
        assert ((m >= np.minimum(lo, hi)) & (m <= np.maximum(lo, hi))).all(), f"{name}: mean {m} against {m64}"
        rerr = np.abs(r.astype(np.float64) - r64) / r64
        print(f"  meanstd {name}: mean exact, rstd relative err {rerr.max():.3e}, bound {rel.max():.3e}")
        assert np.isfinite(r).all() and (rerr <= rel).all(), f"{name}: rstd {r} against {r64}: {rerr} > {rel}"
        if name == "S = 1" or name.startswith("constant"):
            assert (r == np.float32(1e12)).all(), name
        if B > 1:                                                                          # B = 1 on the last volume
            call("pcrl_aug_meanstd", x[B - 1:].to(DEV), mean, rstd, 1, S)
            assert mean[0].item() == m[B - 1] and rstd[0].item() == r[B - 1] and mean[1].item() == m[1]


# ----------------------------------------------------------------------------------------------------------------------------------------
# 6. z-normalisation
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,B", A.ZNORM_SIZES)
def test_znorm_bit_for_bit(S, B):
    """znorm_kernel with arbitrary float32 mean and rstd (inputs, not the volume's own): a subtraction, then a product, nothing to contract.
    S = 1, 257 and 262 144 + 77 (past the grid cap); the last volume is a constant with rstd = 1e12: exact zeros.  Measured: bits."""
    g = torch.Generator().manual_seed(S)
    x = torch.randn(B, S, generator=g) * 3 + 1
    x[B - 1] = 0.3
    m = torch.tensor([0.37, -2.5, 1000.0][:B - 1] + [0.3])
    r = torch.tensor([1.7, 0.003, 12345.678][:B - 1] + [1e12])
    y = sentinel(B * S + 1)
    call("pcrl_aug_znorm", x.to(DEV), y, m.to(DEV), r.to(DEV), B, S)
    want = ((x.numpy() - m.numpy()[:, None]) * r.numpy()[:, None]).astype(np.float32)
    same_bits(y[:B * S].view(B, S), want, f"znorm S={S} B={B}")
    assert y[B * S].item() == SENTINEL and (y[(B - 1) * S:B * S] == 0).all()


# ----------------------------------------------------------------------------------------------------------------------------------------
# 7. swap
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", A.swap_cases(), ids=lambda c: c[0])
def test_swap_bit_for_bit(case):
    """swap_kernel: one block of 256 threads per volume walks the patch with t += 256.  P = 24 (under the block), 255, 256, 257, 300, 600;
    patches that touch in each axis; equal corners; a chain in which a later exchange moves voxels an earlier one placed; B = 3 with its own
    corners per volume.  A swap is a permutation: the sorted voxels are the input's (what lets apply_intensity take mean and std before it).
    Measured: bits."""
    name, dhw, patch, o = case
    B = o.shape[1]
    x = (torch.arange(B * dhw[0] * dhw[1] * dhw[2], dtype=torch.float32) * 0.5 - 100).view(B, *dhw)
    y = torch.cat([x.flatten(), torch.full((1,), SENTINEL)]).to(DEV)
    call("pcrl_aug_swap", y, o.to(DEV), B, *dhw, *patch, o.shape[0])
    want = R.ref_swap(x, o, patch)
    same_bits(y[:-1].view(B, *dhw), want, name)
    assert y[-1].item() == SENTINEL
    assert torch.equal(y[:-1].cpu().view(B, -1).sort(1).values, x.view(B, -1).sort(1).values)
    assert torch.equal(want, x) == all(bool((p[0] == p[1]).all()) for p in o.reshape(-1, 2, 3))      # only equal corners leave the volume alone
    y0 = x.to(DEV).clone()
    call("pcrl_aug_swap", y0, o.to(DEV), B, *dhw, *patch, 0)                              # iters = 0
    assert torch.equal(y0.cpu(), x)


# ----------------------------------------------------------------------------------------------------------------------------------------
# 8. refusals
# ----------------------------------------------------------------------------------------------------------------------------------------
def _refusals():
    """[(what, entry, args builder(t) -> args)]; t: dict of small device tensors; the output tensors hold the sentinel"""
    c = []
    V = ("pcrl_aug_volume_min", lambda t, x="x", o="o1", B=2, S=64: (t[x], t[o], B, S))
    c += [("min: null x", V[0], lambda t: V[1](t, x=None)), ("min: null out", V[0], lambda t: V[1](t, o=None)),
          ("min: B = 0", V[0], lambda t: V[1](t, B=0)), ("min: S = 0", V[0], lambda t: V[1](t, S=0))]
    Af = lambda t, x="x", y="y", inv="inv", flip="flip", fill="fill", B=2, D=4, H=4, W=4: (t[x], t[y], t[inv], t[flip], t[fill], B, D, H, W)
    c += [(f"affine: null {k}", "pcrl_aug_affine", (lambda k: lambda t: Af(t, **{k: None}))(k)) for k in ("x", "y", "inv", "flip", "fill")]
    c += [("affine: in place", "pcrl_aug_affine", lambda t: Af(t, x="y")), ("affine: B = 0", "pcrl_aug_affine", lambda t: Af(t, B=0)),
          ("affine: B = 65536", "pcrl_aug_affine", lambda t: Af(t, B=65536)), ("affine: D = 0", "pcrl_aug_affine", lambda t: Af(t, D=0)),
          ("affine: W = -1", "pcrl_aug_affine", lambda t: Af(t, W=-1))]
    Bl = lambda t, x="x", y="y", s="sig", B=2, D=4, H=4, W=4, axis=0, radius=8: (t[x], t[y], t[s], B, D, H, W, axis, radius)
    c += [(f"blur: null {k}", "pcrl_aug_blur_axis", (lambda k: lambda t: Bl(t, **{k: None}))(k)) for k in ("x", "y", "s")]
    c += [("blur: in place", "pcrl_aug_blur_axis", lambda t: Bl(t, x="y")), ("blur: B = 0", "pcrl_aug_blur_axis", lambda t: Bl(t, B=0)),
          ("blur: B = 65536", "pcrl_aug_blur_axis", lambda t: Bl(t, B=65536)), ("blur: axis 3", "pcrl_aug_blur_axis", lambda t: Bl(t, axis=3)),
          ("blur: axis -1", "pcrl_aug_blur_axis", lambda t: Bl(t, axis=-1)), ("blur: radius -1", "pcrl_aug_blur_axis", lambda t: Bl(t, radius=-1)),
          ("blur: radius 33", "pcrl_aug_blur_axis", lambda t: Bl(t, radius=33)), ("blur: H = 0", "pcrl_aug_blur_axis", lambda t: Bl(t, H=0))]
    N = lambda t, x="x", y="y", s="sig", g="gam", B=2, S=64: (t[x], t[y], t[s], t[g], B, S, 1)
    c += [(f"noise: null {k}", "pcrl_aug_noise_gamma", (lambda k: lambda t: N(t, **{k: None}))(k)) for k in ("x", "y", "s", "g")]
    c += [("noise: B = 0", "pcrl_aug_noise_gamma", lambda t: N(t, B=0)), ("noise: B = 65536", "pcrl_aug_noise_gamma", lambda t: N(t, B=65536)),
          ("noise: S = 0", "pcrl_aug_noise_gamma", lambda t: N(t, S=0))]
    M = lambda t, x="x", m="o1", r="o2", B=2, S=64: (t[x], t[m], t[r], B, S)
    c += [(f"meanstd: null {k}", "pcrl_aug_meanstd", (lambda k: lambda t: M(t, **{k: None}))(k)) for k in ("x", "m", "r")]
    c += [("meanstd: B = 0", "pcrl_aug_meanstd", lambda t: M(t, B=0)), ("meanstd: S = 0", "pcrl_aug_meanstd", lambda t: M(t, S=0))]
    Z = lambda t, x="x", y="y", m="sig", r="gam", B=2, S=64: (t[x], t[y], t[m], t[r], B, S)
    c += [(f"znorm: null {k}", "pcrl_aug_znorm", (lambda k: lambda t: Z(t, **{k: None}))(k)) for k in ("x", "y", "m", "r")]
    c += [("znorm: B = 0", "pcrl_aug_znorm", lambda t: Z(t, B=0)), ("znorm: B = 65536", "pcrl_aug_znorm", lambda t: Z(t, B=65536)),
          ("znorm: S = 0", "pcrl_aug_znorm", lambda t: Z(t, S=0))]
    Sw = lambda t, y="y", o="org", B=2, D=4, H=4, W=4, p=(2, 2, 2), iters=1: (t[y], t[o], B, D, H, W, *p, iters)
    c += [("swap: null x", "pcrl_aug_swap", lambda t: Sw(t, y=None)), ("swap: null origins", "pcrl_aug_swap", lambda t: Sw(t, o=None)),
          ("swap: B = 0", "pcrl_aug_swap", lambda t: Sw(t, B=0)), ("swap: iters -1", "pcrl_aug_swap", lambda t: Sw(t, iters=-1))]
    c += [(f"swap: patch {p}", "pcrl_aug_swap", (lambda p: lambda t: Sw(t, p=p))(p)) for p in ((5, 2, 2), (2, 5, 2), (2, 2, 5), (0, 2, 2), (2, 2, -1))]
    return c


def test_every_entry_point_refuses_what_it_cannot_run():
    """Null pointers, an in-place affine or blur, B = 0, B = 65 536 where the grid's y carries B, axis 3 and -1, radius -1 and 33, an empty or
    negative extent, S = 0, a patch larger than the volume or empty, iters < 0: PcrlError before any launch, the outputs keep their sentinel;
    the next valid call works."""
    t = dict(x=torch.ones(2, 4, 4, 4, device=DEV), y=sentinel(2, 4, 4, 4), o1=sentinel(2), o2=sentinel(2), sig=torch.ones(2, device=DEV),
             gam=torch.ones(2, device=DEV), inv=torch.eye(3, device=DEV).repeat(2, 1, 1).contiguous(), flip=torch.zeros(2, dtype=torch.int32, device=DEV),
             fill=torch.zeros(2, device=DEV), org=torch.tensor([[[[0, 0, 0], [2, 2, 2]]] * 2], dtype=torch.int32, device=DEV))
    t[None] = None
    cases = _refusals()
    assert len(cases) == 53
    for what, entry, build in cases:
        with pytest.raises(PcrlError):
            call(entry, *build(t))
            torch.cuda.synchronize()
            pytest.fail(f"{what}: accepted")
        torch.cuda.synchronize()
        for k in ("y", "o1", "o2"):
            assert (t[k] == SENTINEL).all(), f"{what}: {k} was written"
        assert (t["x"] == 1).all(), what
    call("pcrl_aug_znorm", t["x"], t["y"], t["sig"], t["gam"], 2, 64)
    assert (t["y"] == 0).all()
