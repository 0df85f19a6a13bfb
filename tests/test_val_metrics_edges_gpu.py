"""ops.val_metrics (csrc/val_metrics.hip) and ops2d.val2d_metrics (csrc/val_metrics2d.hip) at their edges: more than 256 first-stage blocks and
more than 256 term rows (the second trip of the finishing kernels' stride-256 walks -- the real workload's 16 crops of 64 x 64 x 32 are 512
chunks), a ragged last chunk / block of pixels, H != W, the 16 x 16 image whose coarsest map is one pixel, channel widths that are no multiple
of 64 and differ between the scales, a last block of cosine rows with fewer than four live waves, B = 1, nlocal = 1, rows below eps.

The case lists, lattices and float64 restatements are in heads_eval_cases.py (preconditions: test_heads_eval_cases_cpu.py).  Bounds:
  MSE entries   the maps sit on the i/8 lattice (and the interpolation weights of a power-of-two scale are dyadic), so every square and every
                float64 sum of the kernels is exact in any order; what is left is the multiplication by the rounded 1.0 / S:
                3D   bit for bit where S is a power of two, else within 1 ulp of float64 (one multiplication by a rounded reciprocal against one
                     correctly rounded division: the two differ by less than 1 ulp of the result)
                2D   within 2 ulps of float64 (inv_S = 1 / (3 H W) is rounded once, then one multiplication)
  cosine        features from torch.randn:  |acc[q] / B - ref[q]| <= 2^-44 x (the weighted sum of |cos_j| of that entry).  A term has at most
                C / 64 + 6 rounded float64 additions per sum, then a square root, a product and a division: for C <= 1024 a relative error below
                2^-47 per term; the bound leaves a factor 8 over that (it covers the restatement's own roundings and the final sums).  It is far
                below the effect of one dropped or doubled row, about |cos| / R.
"""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import heads_eval_cases as hec  # noqa: E402
from pcrlv2_amd import ops, ops2d  # noqa: E402
from pcrlv2_amd._lib import PcrlError, lib, stream_handle  # noqa: E402

DEV = "cuda"
F32 = torch.float32
COS_REL = 2.0 ** -44


def _split(feats):
    """per scale six tensors -> feats1, feats2, feats_loc of the wrappers ([projection, prediction] per scale), on the device"""
    d = [[t.to(DEV) for t in f] for f in feats]
    return [[f[0], f[1]] for f in d], [[f[2], f[3]] for f in d], [[f[4], f[5]] for f in d]


def run3d(out1, masks, gt, feats, acc=None):
    acc = torch.zeros(11, dtype=torch.float64, device=DEV) if acc is None else acc
    dev = lambda t: t.to(F32).to(DEV)
    ops.val_metrics(dev(out1), [dev(m) for m in masks], dev(gt), *_split(feats), acc)
    return acc


def run2d(out1, masks, gt, feats, acc=None):
    acc = torch.zeros(17, dtype=torch.float64, device=DEV) if acc is None else acc
    nhwc = lambda t: ops2d.to_act2(t.to(F32).to(DEV), F32)
    ops2d.val2d_metrics(nhwc(out1), [nhwc(m) for m in masks], gt.to(F32).to(DEV).contiguous(), *_split(feats), acc)
    return acc


def check_mse(got, ref, ulps, what):
    for q, (g, r) in enumerate(zip(got.tolist(), ref.tolist())):
        assert r > 0.0 and abs(g - r) <= ulps * math.ulp(r), f"{what}: MSE entry {q}: got {g!r}, float64 {r!r}: {abs(g - r) / math.ulp(r):.1f} ulps, allowed {ulps}"


def check_cos(got, ref, absw, B, first, what):
    """-> worst error / bound over the cosine entries acc[first:]"""
    worst = 0.0
    for q in range(first, ref.numel()):
        err, bound = abs(float(got[q]) / B - float(ref[q]) / B), COS_REL * float(absw[q]) / B
        worst = max(worst, err / bound)
        assert err <= bound, f"{what}: cosine entry {q}: |{float(got[q]) / B!r} - {float(ref[q]) / B!r}| = {err:.3e} > {bound:.3e}"
    return worst


def accumulates_and_repeats(run, args, first, B, n):
    """two calls into one accumulator give exactly twice the first; the count entry is 2 B; a second fresh run is bit-identical"""
    again = run(*args)
    assert torch.equal(again.cpu().view(torch.int64), first.view(torch.int64)), "a second fresh run differs"
    twice = run(*args, acc=again).cpu()
    assert torch.equal(twice, 2.0 * first), "two calls into one accumulator are not twice the first"
    assert float(first[n]) == B and float(twice[n]) == 2 * B


@pytest.mark.parametrize("case", hec.VAL3D_CASES, ids=lambda c: f"B{c[0]}-S{c[1]}-nl{c[2]}-C{c[3][0]}")
def test_val_metrics_at_its_edges(case):
    B, S, nl, widths, why = case
    out1, masks, gt = hec.val_maps3d(B, S, seed=31 * B + S % 1000)
    feats = hec.val_feats(B, nl, widths, seed=7 * B + nl)
    ref, absw = hec.val_metrics_ref(out1, masks, gt, feats, B, nl)
    got = run3d(out1, masks, gt, feats).cpu()
    check_mse(got[:4], ref[:4], 0 if hec.is_pow2(S) else 1, f"val_metrics B={B} S={S} ({why})")
    worst = check_cos(got, ref, absw, B, 4, f"val_metrics B={B} nlocal={nl} C={widths} ({why})")
    accumulates_and_repeats(run3d, (out1, masks, gt, feats), got, B, 10)
    print(f"[val_metrics B={B} S={S} nlocal={nl} C={widths}] MSE within {0 if hec.is_pow2(S) else 1} ulp; cosine worst error / bound {worst:.4f}")


@pytest.mark.parametrize("case", hec.VAL2D_CASES, ids=lambda c: f"B{c[0]}-{c[1]}x{c[2]}-nl{c[3]}")
def test_val2d_metrics_at_its_edges(case):
    B, H, W, nl, why = case
    out1, masks, gt = hec.val_maps2d(B, H, W, seed=13 * B + H + 3 * W)
    feats = hec.val_feats(B, nl, hec.C5, seed=5 * B + nl)
    ref, absw = hec.val2d_metrics_ref(out1, masks, gt, feats, B, nl)
    got = run2d(out1, masks, gt, feats).cpu()
    check_mse(got[:6], ref[:6], 2, f"val2d_metrics B={B} {H}x{W} ({why})")
    worst = check_cos(got, ref, absw, B, 6, f"val2d_metrics B={B} nlocal={nl} ({why})")
    accumulates_and_repeats(run2d, (out1, masks, gt, feats), got, B, 16)
    print(f"[val2d_metrics B={B} {H}x{W} nlocal={nl}] MSE within 2 ulps; cosine worst error / bound {worst:.4f}")


# ---- degenerate rows ----
def _all_pairs_zero(f, scale, names):
    """zero the named tensors of one scale entirely"""
    idx = dict(pro1=0, pre1=1, pro2=2, pre2=3, proL=4, preL=5)
    for n in names:
        f[scale][idx[n]].zero_()


def _degenerate(feats, B, nl):
    """a zero row in each of the six tensors of scale 0 (different rows), rows of norm about 1e-9 < eps in each tensor of scale 1"""
    for q, r in enumerate((0, 1, 2, 0, 1, B * (nl - 1) + 2)):
        feats[0][q][r].zero_()
    for q, r in enumerate((2, 0, 1, 1, B * (nl - 1), 2)):
        feats[1][q][r].mul_(1e-10)
    feats[1][0][0].mul_(1e-10)       # the rows above meet rows of ordinary norm; here BOTH rows of the pair cos(pre2[0], pro1[0]) lie below eps
    feats[1][3][0].mul_(1e-10)


@pytest.mark.parametrize("dim", [3, 2])
def test_rows_below_eps_follow_the_explicit_formula(dim):
    B, nl = 3, 2
    widths = hec.C3_B if dim == 3 else hec.C5
    feats = hec.val_feats(B, nl, widths, seed=90 + dim)
    _degenerate(feats, B, nl)
    norms = [float(t.double().norm(dim=1).min()) for t in feats[1]]
    assert all(0.0 < n < hec.EPS for n in norms), norms
    if dim == 3:
        out1, masks, gt = hec.val_maps3d(B, 100, seed=1)
        ref, absw = hec.val_metrics_ref(out1, masks, gt, feats, B, nl)
        got, first = run3d(out1, masks, gt, feats).cpu(), 4
    else:
        out1, masks, gt = hec.val_maps2d(B, 16, 16, seed=1)
        ref, absw = hec.val2d_metrics_ref(out1, masks, gt, feats, B, nl)
        got, first = run2d(out1, masks, gt, feats).cpu(), 6
    assert bool(torch.isfinite(got).all())
    worst = check_cos(got, ref, absw, B, first, f"degenerate rows, {dim}D")
    # the terms with a zero row are exactly 0 in the restatement; dropping those pairs from it altogether changes nothing
    glob, loc = hec.cos_terms(feats[0], B, nl)
    assert int((glob == 0).sum()) >= 3 and int((loc == 0).sum()) >= 6
    print(f"[val metrics {dim}D, rows below eps] cosine worst error / bound {worst:.4f}")


@pytest.mark.parametrize("dim", [3, 2])
def test_a_zero_row_in_every_pair_gives_exactly_zero(dim):
    """B = 1, nlocal = 1: six terms per scale.  Scale 0: pro1, pre1, pro2 and proL are zero; scale 1: pre2, preL, pro1 and pre1 -- each of the
    six tensors is zero somewhere and every pair of both scales holds a zero row: their four entries must be exactly 0 (no 0 / 0)."""
    widths = hec.C3_A if dim == 3 else hec.C5
    feats = hec.val_feats(1, 1, widths, seed=60 + dim)
    _all_pairs_zero(feats, 0, ("pro1", "pre1", "pro2", "proL"))
    _all_pairs_zero(feats, 1, ("pre2", "preL", "pro1", "pre1"))
    if dim == 3:
        out1, masks, gt = hec.val_maps3d(1, 10, seed=2)
        got, g0, l0 = run3d(out1, masks, gt, feats).cpu(), 4, 7
    else:
        out1, masks, gt = hec.val_maps2d(1, 16, 16, seed=2)
        got, g0, l0 = run2d(out1, masks, gt, feats).cpu(), 6, 11
    for q in (g0, g0 + 1, l0, l0 + 1):
        assert float(got[q]) == 0.0, (q, float(got[q]))
    for q in (g0 + 2, l0 + 2):
        assert float(got[q]) != 0.0 and math.isfinite(float(got[q]))


# ---- rejections: host-side checks, nothing is launched ----
def test_val_metrics_rejections():
    L, s = lib(), stream_handle()
    B, S, nl, C = 2, 64, 2, 8
    m = [torch.zeros(B * S, dtype=F32, device=DEV) for _ in range(5)]
    f = [torch.zeros(nl * B * C, dtype=F32, device=DEV) for _ in range(18)]
    acc = torch.full((11,), -7.0, dtype=torch.float64, device=DEV)
    nb = L.call("pcrl_val_metrics_ws_bytes", B * S, B, nl)
    assert nb == (hec.val_blocks(B, S) * 4 + 3 * hec.val_rows(B, nl)) * 8
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    call = lambda nb_=nb, B_=B, nl_=nl, C0=C: L.call("pcrl_val_metrics", *m, *f, acc, ws, nb_, B_, S, nl_, C0, C, C, 1e-8, s)
    with pytest.raises(PcrlError, match=r"val_metrics: bad sizes B=0 "):
        call(B_=0)
    with pytest.raises(PcrlError, match=r"val_metrics: bad sizes B=2 S=64 nlocal=0 "):
        call(nl_=0)
    with pytest.raises(PcrlError, match=r"val_metrics: bad sizes B=2 S=64 nlocal=2 C=0,8,8"):
        call(C0=0)
    with pytest.raises(PcrlError, match="val_metrics: workspace too small"):
        call(nb_=nb - 8)
    torch.cuda.synchronize()
    assert bool((acc == -7.0).all()), "a rejected call wrote the accumulator"
    acc.zero_()
    call()
    assert float(acc.cpu()[10]) == B


def test_val2d_metrics_rejections():
    """(H = 24 is rejected in test_validate2d_cpu.py)"""
    L, s = lib(), stream_handle()
    B, H, W, nl, C = 2, 16, 32, 2, 8
    out1, gt = (torch.zeros(B * 3 * H * W, dtype=F32, device=DEV) for _ in range(2))
    masks = [torch.zeros(B * 3 * H * W, dtype=F32, device=DEV) for _ in range(5)]
    feats = [torch.zeros(nl * B * C, dtype=F32, device=DEV) for _ in range(30)]
    acc = torch.full((17,), -7.0, dtype=torch.float64, device=DEV)
    nb = L.call("pcrl_val2d_metrics_ws_bytes", B, H, W, nl)
    assert nb == (hec.val2d_blocks(B, H, W) * 6 + 5 * hec.val_rows(B, nl)) * 8
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    mp, fp = (ctypes.c_void_p * 5)(*[t.data_ptr() for t in masks]), (ctypes.c_void_p * 30)(*[t.data_ptr() for t in feats])

    def call(nb_=nb, B_=B, nl_=nl, C0=C):
        Cs = (ctypes.c_int * 5)(C0, C, C, C, C)
        L.call("pcrl_val2d_metrics", out1, ctypes.addressof(mp), gt, ctypes.addressof(fp), ctypes.addressof(Cs), acc, ws, nb_, B_, H, W, nl_, 1e-8, s)

    with pytest.raises(PcrlError, match=r"val2d_metrics: bad sizes B=0 "):
        call(B_=0)
    with pytest.raises(PcrlError, match=r"val2d_metrics: bad sizes B=2 H=16 W=32 nlocal=0"):
        call(nl_=0)
    with pytest.raises(PcrlError, match="val2d_metrics: null map or bad channel count at scale 0"):
        call(C0=0)
    with pytest.raises(PcrlError, match="val2d_metrics: workspace too small"):
        call(nb_=nb - 8)
    torch.cuda.synchronize()
    assert bool((acc == -7.0).all()), "a rejected call wrote the accumulator"
    acc.zero_()
    call()
    assert float(acc.cpu()[16]) == B
