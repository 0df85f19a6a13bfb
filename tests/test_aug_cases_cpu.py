"""Preconditions of tests/test_augment_exact_gpu.py, checked without a GPU: the constants the case table was built for are the source's; the
affine lattice is exactly summable (a float32 evaluation in either operand order equals the float64 reference in bits); the hash restatement
reproduces the collisions of the one-key hash and finds none in the two-key one; the derived bounds of the blur and of mean / rstd hold for a
float32 (float64 for the one-pass statistics) operation-by-operation numpy evaluation with room; the blur's definition agrees with
scipy.ndimage.gaussian_filter up to the tail mass its fixed radius keeps; draw_swap's overlap rule."""
import numpy as np
import pytest
import torch

import aug_cases as A
import aug_reference as R
from exact_lattice import EXACT_LIMIT, assert_bit_equal
from pcrlv2_amd import data as D


def test_the_constants_of_the_source_are_the_ones_the_case_table_was_built_for():
    assert A.source_pins_hold() == []
    assert A.CAP_ITEMS == 262144 and D.BLUR_RADIUS == 8 and D.BLUR_RADIUS <= A.MAX_RADIUS


# ---- the hash ----
def test_mix32_is_a_permutation_with_the_restated_inverse():
    with np.errstate(over="ignore"):
        x = np.arange(1 << 16, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(12345)
    assert np.array_equal(A.unmix32(A.mix32(x)), x) and np.array_equal(A.mix32(A.unmix32(x)), x)


@pytest.mark.parametrize("seed,B,S,i,j,K", A.COLLISIONS_V1)
def test_the_one_key_hash_gave_two_volumes_of_a_call_the_same_field(seed, B, S, i, j, K):
    """The defect this hash was changed for: n_i[idx] == n_j[idx ^ K], deviate for deviate."""
    k = A.keys_v1(seed, np.arange(B, dtype=np.uint32))
    assert int(k[i] ^ k[j]) == K and K < S
    idx = np.arange(S, dtype=np.uint64)
    ai, ci = A.draws_v1(seed, i, idx)
    aj, cj = A.draws_v1(seed, j, idx ^ np.uint64(K))
    assert np.array_equal(ai, aj) and np.array_equal(ci, cj)
    ni, nj = A.deviate64(ai, ci), A.deviate64(*A.draws_v1(seed, j, idx))
    assert np.array_equal(np.sort(ni), np.sort(nj))
    # the two-key hash on the same call: the two volumes hold other values of `a`
    a2i, _ = A.draws(seed, i, idx)
    a2j, _ = A.draws(seed, j, idx)
    assert np.intersect1d(a2i, a2j).size < 64          # chance hits: S^2 / 2^32 = 0.004 (S = 4096), 4 (S = 2^17) expected
    assert not np.array_equal(np.sort(a2i), np.sort(a2j))


def test_the_one_key_hash_collided_at_the_rate_the_issue_reports():
    assert [h[0] for h in A.shared_fields_v1(range(13), 64, 131072)] == [4, 7, 12]
    assert [h[0] for h in A.shared_fields_v1(range(512), 64, 4096)] == [262, 435, 511]
    idx = np.arange(4096, dtype=np.uint64)
    a_lo, c_lo = A.draws_v1(5, 3, idx)
    a_hi, c_hi = A.draws_v1((1 << 61) + 5, 3, idx)
    assert np.array_equal(a_lo, a_hi) and not np.array_equal(c_lo, c_hi)      # the radius ignored the seed's high word


def test_no_two_volumes_of_a_call_share_a_field():
    """seeds 0 .. 4095, B = 256, S = 4096 and 131 072: no pair of volumes whose sets of `a` (and with them of (a, c)) are equal"""
    assert A.shared_fields(range(4096), 256, (4096, 131072)) == []
    for seed in (0, 4, 262, (1 << 61) + 5):
        _, k1 = A.keys(seed, np.arange(65535, dtype=np.uint32))
        assert np.unique(k1).size == 65535                                       # k1 is a bijection of the volume
    # the search does find a planted equality: volume j given volume i's keys
    real = A.keys

    def planted(seed, v):
        k0, k1 = real(seed, v)
        t0, t1 = real(seed, np.uint32(1))
        return np.where(np.asarray(v) == 3, t0, k0), np.where(np.asarray(v) == 3, t1, k1)
    try:
        A.keys = planted
        assert A.shared_fields([9], 4, (4096,)) == [(9, 1, 3, 4096)]
    finally:
        A.keys = real


def test_both_draws_depend_on_all_64_seed_bits_and_on_the_volume():
    idx = np.arange(4096, dtype=np.uint64)
    base = A.draws(5, 3, idx)
    for seed, vol in (((1 << 61) + 5, 3), ((1 << 32) + 5, 3), (4, 3), (5, 2), (5 + (1 << 31), 3)):
        a, c = A.draws(seed, vol, idx)
        assert (a == base[0]).mean() < 0.01 and (c == base[1]).mean() < 0.01
        assert (a >> np.uint32(8) == base[0] >> np.uint32(8)).mean() < 0.01      # the radius draw itself
    hi = A.draws(5, 3, idx + (np.uint64(1) << np.uint64(32)))
    assert (hi[0] == base[0]).all() and (hi[1] == base[1]).mean() < 0.01         # past 2^32 elements the angle still changes


def test_the_deviates_are_standard_normal_and_uncorrelated_between_volumes():
    a, c = A.noise_field(1234, 4, 1 << 16)
    n = A.deviate64(a, c)
    assert np.isfinite(n).all()
    for b in range(4):
        v = n[b]
        assert abs(v.mean()) < 0.02 and abs(v.std() - 1) < 0.02 and abs((v ** 3).mean()) < 0.05 and abs((v ** 4).mean() - 3) < 0.15
    cc = np.corrcoef(n)
    assert np.abs(cc - np.eye(4)).max() < 0.02
    assert abs(np.corrcoef(n[0, :-1], n[0, 1:])[0, 1]) < 0.02


def test_the_float32_yardstick_of_the_deviate_and_of_the_gamma_map():
    """What 4 x the yardstick means in numbers (printed; the GPU test computes it again for its own inputs)."""
    a, c = A.noise_field(5, 2, 4096)
    n64, n32 = A.deviate64(a, c), A.deviate32(a, c).astype(np.float64)
    y = (np.abs(n32 - n64) / np.maximum(1.0, np.abs(n64))).max()
    x, g = np.meshgrid(A.GAMMA_X, A.GAMMA_G)
    r64, r32 = A.gamma64(x, g), A.gamma32(x, g).astype(np.float64)
    nz = r64 != 0
    yg = (np.abs(r32 - r64)[nz] / np.abs(r64[nz])).max()
    print(f"  deviate yardstick {y:.3e}, gamma yardstick {yg:.3e} (relative)")
    assert 0 < y < 1e-6 and 0 < yg < 2e-7
    assert np.isfinite(r64).all() and (np.abs(r64[nz]) >= 2.0 ** -120).all() and (np.abs(r64) < 2.0 ** 120).all()      # no subnormal, no overflow


# ---- affine ----
def test_the_affine_lattice_is_exactly_summable_in_any_order():
    for name, m in A.affine_matrices():
        assert torch.equal(m * 8, (m * 8).round()), name
    for dhw in A.AFFINE_EXTENTS:
        x, flip, inv, fill, names = A.affine_case(dhw)
        half = (max(dhw) - 1) / 2                                                 # the largest centred coordinate
        # coordinates: multiples of 1/16 (1/2 where the matrix is integral), |s| <= sum|m| half + half; weights: multiples of 2^-12, <= 1;
        # terms: |v| <= 64, or the fill
        for m in inv.double():
            unit = 1 / 2 if torch.equal(m, m.round()) else 1 / 16
            smax = float(m.abs().sum(1).max()) * half + half
            assert smax / unit < EXACT_LIMIT and smax < 2 ** 31, (dhw, m)
        assert max(A.DATA_MAX, float(fill.abs().max())) * 8 * 4096 < EXACT_LIMIT
        assert len(set(fill.tolist())) == len(fill) and fill.max() < -A.DATA_MAX
        ref = R.ref_spatial(x, flip, inv, fill)
        for rev in (False, True):
            assert_bit_equal(torch.from_numpy(A.affine_f32(x, flip, inv, fill, reverse=rev)), ref, torch.float32, f"float32 affine {dhw} reverse={rev}")
        # the cases do what they are there for
        k = {n: i for i, n in enumerate(names)}
        assert torch.equal(ref[k["identity, flip 0"]], x[k["identity, flip 0"]].double())
        assert torch.equal(ref[k["identity, flip 1"]], x[k["identity, flip 1"]].flip(0).double())
        b = k["scale 2^20, flip 0"]
        inside = (ref[b] != fill[b].double()).sum().item()
        assert inside == (1 if all(e % 2 for e in dhw) else 0)                    # odd extents: the centre voxel maps onto itself
        if len(set(dhw)) == 3:
            outside = [(ref[i] == fill[i].double()).float().mean().item() for n, i in k.items() if n.startswith("signed permutation")]
            assert max(outside) > 0.25
        frac = ref[k["shear 1/8, flip 0"]]
        assert (frac != frac.round()).any()                                       # fractional weights are exercised


# ---- blur ----
def _blur_cases():
    for dhw in A.BLUR_EXTENTS:
        for axis in range(3):
            for radius in A.BLUR_RADII:
                yield dhw, axis, radius


def test_the_blur_bound_holds_for_the_float32_yardstick_with_room():
    worst, cmax = 0.0, 0.0
    sig = torch.tensor(A.BLUR_SIGMAS, dtype=torch.float32)
    for dhw, axis, radius in _blur_cases():
        x = A.blur_data(dhw)
        y64, bound, Aabs = A.blur_axis_bound(x, sig, axis, radius)
        sigma3 = torch.zeros(3, len(sig))
        sigma3[axis] = sig
        ref = R.ref_blur(x, sigma3, radius=radius).numpy()
        assert np.abs(ref - y64).max() <= 1e-13 * np.abs(x.numpy()).max()          # the bound is built around ref_blur's value
        y32 = A.blur_axis_f32(x, sig, axis, radius).astype(np.float64)
        ident = A.blur_is_identity(sig.numpy(), radius)
        assert np.array_equal(y32[ident], x.numpy()[ident].astype(np.float64)), (dhw, axis, radius)
        err = np.abs(y32 - ref)
        assert (err <= 0.5 * bound).all(), (dhw, axis, radius, float((err / bound).max()))
        worst = max(worst, float((err / bound).max()))
        cmax = max(cmax, float((bound[~ident] / (A.U * Aabs[~ident])).max()) if (~ident).any() else 0.0)
        assert bound.max() > 20 * np.median(bound)                                # not flat
    print(f"  float32 yardstick / bound: at most {worst:.3f}; the bound is at most {cmax:.1f} x 2^-24 x sum|w v| / norm")
    assert 0.01 < worst and cmax < 3 * (2 * A.MAX_RADIUS + 2) + 40


def test_the_blur_cases_reach_the_last_weight_and_the_clipped_radius():
    cases = list(_blur_cases())
    n_of = lambda dhw, axis: dhw[axis]
    assert any(min(r, n_of(d, a)) == 32 and n_of(d, a) == 33 for d, a, r in cases)      # wt[64]
    assert any(min(r, n_of(d, a)) == 32 and n_of(d, a) == 40 for d, a, r in cases)
    assert {(n_of(d, a), r) for d, a, r in cases} >= {(4, 8), (4, 32), (5, 8), (5, 32)}  # radius clipped to n
    assert all(any(a == ax and len(set(d)) == 3 for d, a, r in cases) for ax in range(3))


def test_blur_definition_against_scipy_up_to_the_tail_mass():
    """ref_blur (radius 8, renormalised) against scipy.ndimage.gaussian_filter (truncate 4 sigma, mode reflect: what torchio's RandomBlur is
    understood to call).  The two differ in truncation only: at most the tail mass per axis times the data range.  Parity with torchio stays
    unpinned for everything else."""
    import scipy.ndimage as ndi
    g = torch.Generator().manual_seed(3)
    below = [s - 1e-6 for s in A.SCIPY_STEPS]
    worst = (0.0, None)
    for dhw in ((64, 64, 32), (16, 16, 16)):
        triples = [(below[k], below[(k + 3) % 8], below[(k + 5) % 8]) for k in range(8)]
        triples += [tuple(A.SCIPY_STEPS[k] + 1e-6 for k in (0, 3, 7)), (1.11, 1.11, 1.11), (0.05, 1.999, 0.7)]
        triples += [tuple((torch.rand(3, generator=g) * 1.99 + 0.005).tolist()) for _ in range(3)]
        x = torch.rand((len(triples),) + dhw, generator=g, dtype=torch.float64)
        sigma = torch.tensor(triples, dtype=torch.float64).t().contiguous()        # [3, B]
        ref = R.ref_blur(x, sigma).numpy()
        for b, tr in enumerate(triples):
            sp = ndi.gaussian_filter(x[b].numpy(), sigma=tr, mode="reflect", truncate=4.0)
            rng = float(x[b].max() - x[b].min())
            bound = sum(A.scipy_tail_mass(s) for s in tr) * rng + 1e-13
            d = float(np.abs(ref[b] - sp).max())
            assert d <= bound, (dhw, tr, d, bound)
            if d > worst[0]:
                worst = (d, tr)
    print(f"  largest |ref_blur - gaussian_filter| = {worst[0]:.3e} at sigma {worst[1]}")
    assert 1e-6 < worst[0] < 2e-4
    assert max(A.scipy_tail_mass(s - 1e-6) for s in A.SCIPY_STEPS) < 4.9e-5       # the known deviation, per axis, of a unit range (sigma just under 1.625)


# ---- mean / rstd ----
def test_the_meanstd_bounds_hold_for_the_one_pass_formula_in_float64():
    for name, x in A.meanstd_cases():
        m64, tau, r64, rel = A.meanstd_bounds(x)
        m, r = A.meanstd_one_pass64(x)
        lo, hi = (m64 - np.abs(m64) * tau).astype(np.float32), (m64 + np.abs(m64) * tau).astype(np.float32)
        assert ((m >= np.minimum(lo, hi)) & (m <= np.maximum(lo, hi))).all(), name
        assert (np.abs(r.astype(np.float64) - r64) <= rel * r64).all(), (name, np.abs(r - r64) / r64, rel)
        assert np.isfinite(r).all() and rel.max() < 1e-6, name
        if name == "S = 1" or name.startswith("constant"):
            assert (r == np.float32(1e12)).all(), name


# ---- swap ----
def test_the_swap_cases_keep_the_host_contract_and_cross_the_thread_loop():
    ps = set()
    for name, dhw, patch, o in A.swap_cases():
        assert all(p <= e for p, e in zip(patch, dhw)), name
        assert (o >= 0).all() and (o + torch.tensor(patch) <= torch.tensor(dhw)).all(), name
        for pair in o.reshape(-1, 2, 3):
            assert torch.equal(pair[0], pair[1]) or not A.boxes_overlap(pair[0], pair[1], patch), name
        ps.add(patch[0] * patch[1] * patch[2])
    assert ps >= {255, 256, 257, 600} and min(ps) < A.SWAP_THREADS
    name, dhw, patch, o = [c for c in A.swap_cases() if c[0].startswith("chain")][0]
    x = torch.arange(512.0).view(1, 8, 8, 8)
    y = R.ref_swap(x, o, patch)
    assert torch.equal(y[0, 6:8, 1:3, 2:4], x[0, 6:8, 1:3, 2:4]) and torch.equal(y[0, 4:6, 4:6, 4:6], x[0, 0:2, 0:2, 0:2])


def test_a_swap_is_a_permutation_so_mean_and_std_can_be_taken_before_it():
    """apply_intensity measures mean and std BEFORE the swaps and normalises after them: a permutation of the voxels leaves both alone."""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(3, 10, 12, 10, generator=g)
    o = D.draw_swap(g, 3, (10, 12, 10), "cpu", patch=(2, 3, 4), iterations=40)
    y = R.ref_swap(x, o, (2, 3, 4))
    assert not torch.equal(x, y) and torch.equal(x.flatten(1).sort(1).values, y.flatten(1).sort(1).values)


@pytest.mark.parametrize("dhw,patch", [((64, 64, 32), (8, 4, 4)), ((16, 16, 16), (8, 4, 4)), ((6, 5, 4), (2, 2, 2))])
def test_draw_swap_keeps_disjoint_pairs_and_only_those(dhw, patch):
    """10^4 draws: no kept pair overlaps, no discarded pair is disjoint, a kept pair is the drawn one."""
    it, B = 100, 100
    o = D.draw_swap(torch.Generator().manual_seed(5), B, dhw, "cpu", patch=patch, iterations=it)
    r = torch.rand(it, B, 2, 3, generator=torch.Generator().manual_seed(5))
    raw = (r * torch.tensor([dhw[k] - patch[k] + 1 for k in range(3)])).long()
    assert o.dtype == torch.int32 and (o >= 0).all() and (o + torch.tensor(patch) <= torch.tensor(dhw)).all()
    kept = disc = 0
    for got, drawn in zip(o.reshape(-1, 2, 3).tolist(), raw.reshape(-1, 2, 3).tolist()):
        if got[0] == got[1]:
            disc += 1
            assert got[0] == drawn[0] and A.boxes_overlap(drawn[0], drawn[1], patch)
        else:
            kept += 1
            assert got == drawn and not A.boxes_overlap(got[0], got[1], patch)
    assert kept > 100 and disc > 30
