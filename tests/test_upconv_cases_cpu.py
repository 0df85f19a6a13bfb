"""CPU only: the case table of tests/upconv_cases.py (composed ConvTranspose3d -> Conv3d operator) is sound before any kernel runs -- every case
passes its exact-summability preconditions on both lattices, the float64 references agree with each other exactly (they are all lattice values),
the bf16-rounded references have the power to notice a wrong weight, border class or (t, s) pairing, the layout decoders round-trip, and the route
mirrors restate the source and reach every kernel the GPU file claims to reach."""
import pytest
import torch

import exact_lattice as X
import upconv_cases as K

BF = torch.bfloat16
LATS = ("fine", "stats")


@pytest.mark.parametrize("lat", LATS)
@pytest.mark.parametrize("c", K.CASES, ids=K.case_id)
def test_preconditions_and_references_agree(c, lat):
    """reference() asserts every precondition.  Then, exactly: the composed form bias_tab[class] + sum_q x * Weff equals the two-call y; the weights
    composed from the derived (t, s) tables equal the impulse response; the chain rule applied to dWeff and box equals autograd's dw_up, db_up,
    dw0; the box sums with and without the zero-sum shortcut agree on the zero-sum dy."""
    R = K.reference(c, lat)
    assert all(0 <= v < 1 for v in R.headroom.values()), R.headroom
    assert torch.equal(K.compose_from_pairs(R.w_up, R.w0), R.weff)
    assert torch.equal(K.composed_forward(R.x, R.weff, R.bias_tab), R.y)
    dw_up, db_up, dw0 = K.chain_rule(R.dweff, R.box, R.w_up, R.b_up, R.w0)
    assert torch.equal(dw_up, R.dw_up) and torch.equal(db_up, R.db_up) and torch.equal(dw0, R.dw0)
    if c in K.ACCUM_CASES:
        Z = K.zero_sum_reference(c, lat)
        assert torch.equal(Z.box, Z.box_zs)
        assert bool((Z.dy.sum((0, 2, 3, 4)) == 0).all()) and float(Z.dy.abs().max()) > 0


@pytest.mark.parametrize("c", K.CASES, ids=K.case_id)
def test_fine_lattice_exercises_the_output_rounding(c):
    """Outputs above 256 units (a bf16 value holds 8 bits), and outputs exactly half way between two bf16 values"""
    R = K.reference(c, "fine")
    for t, u in ((R.y, R.u.y),):
        k = (t.abs() / u).round()
        assert torch.equal(k * u, t.abs())
        assert int((k > 256).sum()) > 0
        assert int(((k > 256) & (k < 512) & (k % 2 == 1)).sum()) > 0, "no exact tie"
        assert not torch.equal(t.to(BF).double(), t)


@pytest.mark.parametrize("c", [K.CASES[0], K.CASES[2], K.CASES[4]], ids=K.case_id)
def test_power_of_the_bf16_rounded_reference(c):
    """The bf16 rounding of the reference changes in at least one element under: one composed weight bumped by one lattice unit; one fine border voxel
    given the neighbouring border class's bias; the two (t, s) pairs of one (p, q) swapped"""
    R = K.reference(c, "fine")
    y16 = R.y.to(BF)
    w = R.weff.clone()
    w[5, 2, 3, 7] += R.u.weff
    assert not torch.equal(K.composed_forward(R.x, w, R.bias_tab).to(BF), y16)
    cls = K.class_map(c.D, c.H, c.W).clone()
    assert int(cls[0, 0, 0]) == 0
    cls[0, 0, 0] = 1 if 2 * c.W > 2 else 2           # its neighbour along w
    changed = K.composed_forward(R.x, R.weff, R.bias_tab, cls).to(BF) != y16
    assert bool(changed.any()) and bool((changed.sum((0, 1)).nonzero() == 0).all()), "only voxel (0, 0, 0) may change"
    # per axis (p, q) = (0, 1) has the pairs (t, s) = (1, 0), (2, 1); swapped: (1, 1), (2, 0).  On the w axis of p = (1, 1, 0), q = (0, 0, 1), whose
    # coarse voxel v + p - 1 + q = v lies inside every grid:
    pairs = K.ts_pairs(6, 1)
    assert len(pairs) == 8 and sorted({(t % 3, s & 1) for t, s in pairs}) == [(1, 0), (2, 1)]
    swapped = K.compose_from_pairs(R.w_up, R.w0, {(6, 1): [(t, s ^ 1) for t, s in pairs]})
    assert not torch.equal(K.composed_forward(R.x, swapped, R.bias_tab).to(BF), y16)
    dx16 = R.dx.to(BF)
    # the data gradient is the adjoint of the weight part: the same three changes move it too (through autograd of the composed form)
    x = R.x.clone().requires_grad_(True)
    K.composed_forward(x, w, R.bias_tab).backward(R.dy)
    assert not torch.equal(x.grad.to(BF), dx16)
    x = R.x.clone().requires_grad_(True)
    K.composed_forward(x, R.weff, R.bias_tab).backward(R.dy)
    assert torch.equal(x.grad, R.dx)


def test_index_algebra():
    """Every (t, s) belongs to exactly one (p, q); (p, q) has 1, 2, 4 or 8 pairs (27 * 8 = 216 in all); e = 3 - p - 2 q is a bijection per axis"""
    seen = []
    for p in range(8):
        for q in range(8):
            prs = K.ts_pairs(p, q)
            assert len(prs) in (1, 2, 4, 8)
            seen += prs
    assert sorted(seen) == [(t, s) for t in range(27) for s in range(8)]
    assert sorted(K.e_of_pq(p, q) for p in (0, 1) for q in (0, 1)) == [0, 1, 2, 3]
    assert [K.pq_of_ts(t, s) for t, s in ((0, 1), (1, 0), (2, 1), (0, 0), (1, 1), (2, 0))] == [(0, 0), (0, 1), (0, 1), (1, 0), (1, 0), (1, 1)]


@pytest.mark.parametrize("Ci,Co", [(32, 64), (64, 32)])
def test_layout_decoders_round_trip(Ci, Co):
    """encode, then decode, on a tensor of distinct values; the embedded forms hold 8 of 27 taps per phase / parity and zero elsewhere"""
    weff = torch.arange(1, 64 * Ci * Co + 1, dtype=torch.float64).reshape(8, 8, Ci, Co)
    assert torch.equal(K.decode_wf(K.encode_wf(weff).flatten(), Ci, Co), weff) and K.encode_wf(weff).shape == (8, Co, 8, Ci)
    assert torch.equal(K.decode_wd(K.encode_wd(weff).flatten(), Ci, Co), weff) and K.encode_wd(weff).shape == (Ci, 64, Co)
    for enc, dec, shape in ((K.encode_w3f, K.decode_w3f, (8 * Co, 27, Ci)), (K.encode_wd3, K.decode_wd3, (Ci, 27, 8 * Co))):
        e = enc(weff)
        assert e.shape == shape and int((e != 0).sum()) == weff.numel() and e.numel() == 216 * Ci * Co
        got, rest = dec(e.flatten(), Ci, Co)
        assert torch.equal(got, weff) and float(rest.abs().max()) == 0
        got, rest = dec((e + 1).flatten(), Ci, Co)
        assert int((rest != 0).sum()) == e.numel() - weff.numel()
    assert torch.equal(K.decode_dweff(K.encode_dweff(weff).flatten(), Ci, Co), weff) and K.encode_dweff(weff).shape == (Co, Ci, 64)
    # each encoder scatters to distinct places: the five flat forms are permutations of the same values
    for enc in (K.encode_wf, K.encode_wd, K.encode_dweff):
        assert torch.equal(enc(weff).flatten().sort().values, weff.flatten())


def test_route_mirrors_restate_the_source_and_reach_every_kernel():
    for fname, text in K.SOURCE_PINS:
        assert K.source_has(fname, text), f"{fname} no longer contains `{text}`: the route mirrors of upconv_cases.py restate it"
    for c in K.CASES:
        assert (K.fwd_route(c), K.dgrad_route(c), K.wgrad_route(c)) == (c.fwd, c.dgrad, c.wgrad), K.case_id(c)
        for dt, impl in ((K.F32, 0), (K.BF16, 1)):
            assert (K.fwd_route(c, dt, impl), K.dgrad_route(c, dt, impl), K.wgrad_route(c, dt, impl)) == (K.GATHER, K.GATHER, K.WG_GATHER)
    assert K.reached_from_mirrors() == K.EXPECTED_REACHED
    assert K.dgrad_splits(K.SPLITK_DGRAD_CASE) > 1
    # the smallest shape with two brick ranges: one brick fewer along any axis, or the next smaller channel counts the route takes, leave one
    c = K.SPLIT_WGRAD_CASE
    assert K.wgrad_brick_splits(c) == 2 and (c.Ci, c.Cm, c.Co) == (32, 32, 64) and c.N * c.D * c.H * c.W == 32 * 128
    for smaller in (c._replace(D=8), c._replace(H=8), c._replace(W=8), c._replace(D=14)):
        assert K.wgrad_brick_splits(smaller) == 1
    assert all(K.wgrad_brick_splits(o) == 1 for o in K.CASES if o is not c)
    assert [o for o in K.CASES if o.dgrad == K.B8_64] == [K.CASES[12]]


def test_zero_sum_dy_is_on_the_lattice():
    g = torch.Generator().manual_seed(1)
    dy = K.zero_sum_dy((3, 32, 2, 4, 6), K.FINE_UP, g)
    assert torch.equal(dy.to(BF).double(), dy) and torch.equal((dy * 4).round(), dy * 4) and float(dy.abs().max()) <= 1
    assert bool((dy.sum((0, 2, 3, 4)) == 0).all())
    assert X.assert_exactly_summable(dy.abs().sum((0, 2, 3, 4)), 0.25, "zero-sum dy") < 1
