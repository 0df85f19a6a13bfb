"""Preconditions of test_head_bwd_stage_gpu.py, test_val_metrics_edges_gpu.py and the widened test_cls_head_gpu.py, checked without a GPU:
the constants heads_eval_cases.py restates are the ones in the sources; its case lists stand on both sides of every loop and split boundary
(the predicates are computed from the restated constants); every bit-for-bit case of pcrl_head_bwd_stage is exactly summable (asserted
analytically from the lattice bounds); the float64 restatements agree with float64 torch where torch states the same thing; the prototypes
have the argument order the GPU tests rely on."""
import pytest
import torch
import torch.nn.functional as F

import heads_eval_cases as hec
from exact_lattice import EXACT_LIMIT, assert_exactly_summable, unit


def test_the_constants_of_the_sources_are_the_ones_the_case_lists_were_built_for():
    assert hec.source_pins_hold() == []


def test_source_pins_ignore_spacing_and_notice_a_changed_constant():
    text = hec.read_source("heads_fused.hip")
    pin = " ".join(hec._tokens("const int kq = ((K / 4 + 3) / 4) * 4;"))
    assert pin in " ".join(hec._tokens(text.replace("((K / 4 + 3) / 4) * 4", "((K/4+3)\n  / 4)*4")))
    assert pin not in " ".join(hec._tokens(text.replace("((K / 4 + 3) / 4) * 4", "(K / 16) * 4")))
    assert hec.source_pins_hold([("val_metrics.hip", "constexpr int VM_CHUNK = 2048;")]) != []
    assert hec.source_pins_hold([("cls_head.hip", "constexpr int CH_THREADS = 256, CH_MAX_C = 512, CH_MAX_K = 32;")]) != []


# ---- 2. both sides of every boundary ----
def test_head_cases_stand_on_both_sides_of_every_split():
    cases = [(N, K, C) for N, K, C, why in hec.HEAD_CASES]
    assert all(why for _, _, _, why in hec.HEAD_CASES) and len(set(cases)) == len(cases) and 35 <= len(cases) <= 48
    assert {N for N, _, _ in cases} == set(hec.HEAD_N) and {K for _, K, _ in cases} == set(hec.HEAD_K) and {C for _, _, C in cases} == set(hec.HEAD_C)
    assert (2, 4, 4) in cases and (512, 132, 516) in cases and hec.HEAD_LARGEST in cases
    assert {K for N, K, _ in cases if N == 65} == set(hec.HEAD_K)
    assert {N for N, K, C in cases if K == 20 and C == 260} == set(hec.HEAD_N)
    for N, K, C in cases:
        assert 2 <= N <= hec.HEAD_MAX_N and K % 4 == 0 and C % 4 == 0
        q = hec.head_quarters(K)
        assert sorted(k for k0, k1 in q for k in range(k0, k1)) == list(range(K)) and all(k0 % 4 == 0 for k0, _ in q)
    Ks = {K for _, K, _ in cases}
    # the four-wave split: three, two, one and no empty quarter; a non-empty quarter shorter than kq; and K % 16 != 0 next to K % 16 == 0
    assert {hec.head_empty_waves(K) for K in Ks} == {0, 1, 2, 3}
    assert hec.head_empty_waves(4) == 3 and hec.head_empty_waves(8) == 2 and hec.head_empty_waves(12) == 1 and hec.head_empty_waves(36) == 1
    assert hec.head_quarters(20) == [(0, 8), (8, 16), (16, 20), (24, 20)] and hec.head_empty_waves(20) == 1 and hec.head_short_waves(20) == 1
    assert hec.head_quarters(132)[3] == (108, 132) and hec.head_short_waves(132) == 1
    assert any(K % 16 for K in Ks) and any(K % 16 == 0 and hec.head_empty_waves(K) == 0 and hec.head_short_waves(K) == 0 for K in Ks)
    # role B: one, two and three x-blocks; the last lane group beyond C, and exactly full
    assert {hec.head_nbx(C) for _, _, C in cases} == {1, 2, 3}
    assert any(hec.head_nbx(C) == 2 and hec.head_idle_b_lanes(C) > 0 for _, _, C in cases)
    assert hec.head_nbx(260) == 2 and hec.head_idle_b_lanes(260) == 63 and hec.head_nbx(516) == 3 and hec.head_idle_b_lanes(516) == 63
    assert hec.head_idle_b_lanes(256) == 0 and hec.head_idle_b_lanes(252) == 1 and hec.head_idle_b_lanes(4) == 63
    # rows n = lane + 64 i: fewer rows than lanes, lane 63 with and without a row, a lone row in the next trip, RMAX rows in all lanes / all but one
    rows = {N: hec.head_rows_per_lane(N) for N in hec.HEAD_N}
    assert rows[2] == (1, 0) and rows[63] == (1, 0) and rows[64] == (1, 1) and rows[65] == (2, 1) and rows[128] == (2, 2)
    assert rows[449] == (8, 7) and rows[511] == (8, 7) and rows[512] == (hec.RMAX, hec.RMAX)
    # dx bit for bit (N a power of two) and by the derived bound (any other N)
    assert {hec.is_pow2(N) for N in hec.HEAD_N} == {True, False}
    # canaries: C in {252, 260} x K in {4, 20}
    assert {(K, C) for _, K, C in hec.HEAD_CANARY} == {(4, 252), (20, 252), (4, 260), (20, 260)}
    assert set(hec.HEAD_ADD_ONLY) == {(N, C) for N in (2, 65, 512) for C in (4, 260)}


def test_validation_cases_stand_on_both_sides_of_every_boundary():
    c3 = [(B, S, nl, Cs) for B, S, nl, Cs, why in hec.VAL3D_CASES]
    c2 = [(B, H, W, nl) for B, H, W, nl, why in hec.VAL2D_CASES]
    assert all(c[-1] for c in hec.VAL3D_CASES + hec.VAL2D_CASES)
    for want in ((1, 1), (1, 255), (1, 257), (3, 4096), (1, 4097), (2, 6000), (1, 257 * 4096 + 77)):
        assert want in {(B, S) for B, S, _, _ in c3}, want
    for want in ((1, 16, 16), (1, 16, 48), (1, 48, 16), (2, 32, 80), (3, 64, 64), (1, 544, 496)):
        assert want in {(B, H, W) for B, H, W, _ in c2}, want
    for want in ((1, 1), (1, 6), (3, 6), (10, 6), (43, 1), (5, 2)):
        assert want in {(B, nl) for B, _, nl, _ in c3}, want
        assert want in {(B, nl) for B, _, _, nl in c2}, want
    # the finishing kernels' stride over the first-stage blocks: second trip taken / not taken, by one large case each
    big3 = [c for c in c3 if hec.val_blocks(c[0], c[1]) > hec.FINISH_THREADS]
    big2 = [c for c in c2 if hec.val2d_blocks(*c[:3]) > hec.FINISH_THREADS]
    assert len(big3) == 1 and len(big2) == 1 and any(hec.val_blocks(B, S) == 1 for B, S, _, _ in c3)
    B, S, nl, _ = big3[0]
    assert hec.val_blocks(B, S) == 258 and (B * S) % hec.VM_CHUNK == 77 and hec.val_blocks(1, 256 * hec.VM_CHUNK + 77) == 257
    assert hec.val_rows(B, nl) == 6, "the large map case runs with the smallest feature case"
    B, H, W, nl = big2[0]
    assert hec.val2d_blocks(B, H, W) == 264 and (B * H * W) % hec.V2_PX == 512 and H != W and hec.val_rows(B, nl) == 6
    # ... and over the term rows R = B (2 + 4 nlocal)
    for rows in ([hec.val_rows(B, nl) for B, _, nl, _ in c3], [hec.val_rows(B, nl) for B, _, _, nl in c2]):
        assert 260 in rows and 258 in rows and any(r <= hec.FINISH_THREADS for r in rows)
        assert any(r % hec.COS_WAVES for r in rows) and any(r % hec.COS_WAVES == 0 for r in rows)
    assert all(B * S <= 2 * hec.VM_CHUNK for B, S, nl, _ in c3 if hec.val_rows(B, nl) > hec.FINISH_THREADS), "the large feature cases run on small maps"
    assert all(B * H * W <= 12 * hec.V2_PX for B, H, W, nl in c2 if hec.val_rows(B, nl) > hec.FINISH_THREADS)
    # first stage, 3D: S below / at / above the 256 threads and the chunk; a sample boundary inside a chunk
    n3 = {B * S for B, S, _, _ in c3}
    assert 1 in n3 and 255 in n3 and 257 in n3 and 4097 in n3 and 3 * hec.VM_CHUNK in n3 and 12000 in n3 and 6000 % hec.VM_CHUNK != 0
    # first stage, 2D: the smallest legal image, H < W and H > W, a ragged last block and none
    assert (1, 16, 16) in {c[:3] for c in c2} and any(H < W for _, H, W, _ in c2) and any(H > W for _, H, W, _ in c2)
    assert any((B * H * W) % hec.V2_PX for B, H, W, _ in c2) and any((B * H * W) % hec.V2_PX == 0 for B, H, W, _ in c2)
    assert all(H % 16 == 0 and W % 16 == 0 for _, H, W, _ in c2)
    # channel widths: no multiple of 64, below 64, above 64, different at every scale; B = 1 and nlocal = 1
    widths = {C for _, _, _, Cs in c3 for C in Cs} | set(hec.C5)
    assert {1, 63, 64, 65, 130, 200} <= widths and len(set(hec.C3_A)) == 3 and len(set(hec.C3_B)) == 3 and len(set(hec.C5)) == 5
    assert {Cs for _, _, _, Cs in c3} == {hec.C3_A, hec.C3_B}
    assert any(B == 1 for B, _, _, _ in c3) and any(nl == 1 for _, _, nl, _ in c3) and any(nl > 1 for _, _, nl, _ in c3)
    assert max(C for C in widths) <= 1024, "the cosine bound of test_val_metrics_edges_gpu.py is derived for C <= 1024"


def test_cls_head_cases_stand_on_both_sides_of_every_boundary():
    hws = [h * w for h, w in hec.CLS_HW]
    for C in hec.CLS_WIDTHS:
        assert hec.CH_THREADS >= C >= 32 and C & (C - 1) == 0         # the `idx < C` loop takes one short trip (C < 256 threads) ...
        for bf16 in (False, True):
            nv, G = hec.cls_groups(C, bf16)
            assert nv * G == hec.CH_THREADS
            assert any(hw < G for hw in hws) and any(hw > G for hw in hws), (C, bf16, G)
    assert 256 in hec.CLS_WIDTHS and hec.cls_groups(256, False)[1] == 4   # ... or exactly one full trip
    assert max(hec.cls_groups(C, True)[1] for C in hec.CLS_WIDTHS) == 64 and min(hws) == 1 and max(hws) == 65 and 15 in hws
    assert hec.cls_groups(hec.CH_MAX_C, False) == (128, 2) and hec.cls_groups(hec.CH_MAX_C, True) == (64, 4)
    waves = hec.CH_THREADS // 64
    trips = {K: [len(range(w, K, waves)) for w in range(waves)] for K in hec.CLS_WIDE_K}
    assert trips[4] == [1, 1, 1, 1] and trips[5] == [2, 1, 1, 1] and trips[63] == [16, 16, 16, 15] and trips[64] == [16] * 4
    assert max(hec.CLS_WIDE_K) == hec.CH_MAX_K
    assert any(N > hec.CH_THREADS for N in hec.CLS_LONG_N) and hec.CH_THREADS in hec.CLS_LONG_N and any(64 < N < hec.CH_THREADS for N in hec.CLS_LONG_N)


# ---- 3. the exact cases are exactly summable ----
def test_every_head_case_is_exactly_summable():
    dy_max, w_max, mean_max = hec.DY_LAT[0] / hec.DY_LAT[1], hec.W_LAT[0] / hec.W_LAT[1], hec.MEAN_LAT[0] / hec.MEAN_LAT[1]
    rs_min, rs_max = min(hec.RSTD_VALUES), max(hec.RSTD_VALUES)
    for N, K, C, _ in hec.HEAD_CASES:
        t_max = K * dy_max * w_max + dy_max
        assert_exactly_summable(t_max, unit(hec.DY_LAT[1], hec.W_LAT[1]), f"t = sum_k dy W + add, K={K}")
        assert unit(hec.DY_LAT[1], hec.W_LAT[1]) == 1 / 32
        assert_exactly_summable(N * dy_max * dy_max, unit(hec.DY_LAT[1], hec.DY_LAT[1]), f"dW = sum_n dy xin, N={N}")
        assert_exactly_summable(N * dy_max, unit(hec.DY_LAT[1]), f"db = sum_n dy, N={N}")
        # xh = (xbn - mean) rstd is a float32 of the kernel: unit 1/8 * min rstd, a few bits
        xh_unit, xh_max = unit(hec.MEAN_LAT[1]) * rs_min, (dy_max + mean_max) * rs_max
        assert xh_max / xh_unit < EXACT_LIMIT
        # s1, s2: float64 sums of exact terms; dx's float64 products t - s1/N - xh s2/N and gamma rstd (...) for N a power of two
        s2_unit = unit(hec.DY_LAT[1], hec.W_LAT[1]) * xh_unit
        assert N * t_max / (1 / 32) < 2.0 ** 53 and N * t_max * xh_max / s2_unit < 2.0 ** 53
        if hec.is_pow2(N):
            dx_unit = s2_unit * xh_unit / N * min(abs(v) for v in hec.GAMMA_VALUES) * rs_min
            dx_max = max(hec.GAMMA_VALUES) * rs_max * (2 * t_max + xh_max * xh_max * t_max)
            assert dx_max / dx_unit < 2.0 ** 53, (N, K)
    # the lattice values themselves, and that the drawn ybn holds every kind of value the mask must tell apart
    x = hec.head_inputs(65, 20, 260, seed=1)
    for k in ("dy", "W", "add", "xin", "xbn", "ybn", "gamma", "mean", "rstd"):
        assert torch.equal(x[k].float().double(), x[k]), k
    y = x["ybn"]
    neg_zero = (y == 0) & torch.signbit(y)
    assert bool(neg_zero.any()) and bool(((y == 0) & ~torch.signbit(y)).any()) and bool((y > 0).any()) and bool((y < 0).any())
    assert bool(torch.signbit(y.float()[neg_zero]).all()), "-0.0 survives the conversion to float32"
    assert set(x["rstd"].tolist()) == set(hec.RSTD_VALUES) and set(x["gamma"].tolist()) == set(hec.GAMMA_VALUES)


def test_validation_map_sums_are_exact_in_float64():
    """(a - g)^2 on the i/8 lattice is a multiple of 1/64 below 4; through the interpolation (weights multiples of 1/32 per axis) a multiple of
    2^-26: sums over every element of the largest cases stay below 2^53 units."""
    assert 4 * 64 * hec.VAL_BIG_S < 2.0 ** 53
    B, H, W = hec.VAL2D_BIG
    assert 4 * 2.0 ** 26 * 3 * B * H * W < 2.0 ** 53
    for s in (2, 4, 8, 16):
        i0, i1, l1 = hec.bilinear_index(16 * s, s, 16)
        assert torch.equal(l1 * 32, (l1 * 32).round()) and int(i1.max()) == 15 and float(l1.min()) == 0.0
    i0, i1, l1 = hec.bilinear_index(16, 16, 1)
    assert int(i0.max()) == 0 and int(i1.max()) == 0, "the one-pixel map: both indices clamp"


# ---- 4. the restatements against float64 torch ----
@pytest.mark.parametrize("relu", [0, 1])
def test_head_restatement_against_autograd(relu):
    """xbn -> F.batch_norm (batch statistics) = ybn -> [ReLU] = xin -> F.linear(W, b) = y; loss = sum y dy + sum xin add."""
    g = torch.Generator().manual_seed(5 + relu)
    N, K, C, eps = 37, 12, 20, 1e-5
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    xbn, gamma, beta, W, b = r(N, C).requires_grad_(True), r(C).requires_grad_(True), r(C).requires_grad_(True), r(K, C).requires_grad_(True), r(K).requires_grad_(True)
    dy, add = r(N, K), r(N, C)
    ybn = F.batch_norm(xbn, None, None, gamma, beta, training=True, eps=eps)
    xin = torch.relu(ybn) if relu else ybn
    y = F.linear(xin, W, b)
    ((y * dy).sum() + (xin * add).sum()).backward()
    mean = xbn.detach().mean(0)
    rstd = 1.0 / torch.sqrt(xbn.detach().var(0, unbiased=False) + eps)
    dx, dgamma, dbeta, dW, db = hec.head_bwd_stage_ref(dy, W.detach(), add, xin.detach(), xbn.detach(), ybn.detach(), gamma.detach(), mean, rstd, relu)
    for got, want, name in ((dx, xbn.grad, "dx"), (dgamma, gamma.grad, "dgamma"), (dbeta, beta.grad, "dbeta"), (dW, W.grad, "dW"), (db, b.grad, "db")):
        assert torch.allclose(got, want, rtol=1e-10, atol=1e-11), name
    # the "add only" form: the same chain without the Linear
    dx2, dgamma2, dbeta2, none1, none2 = hec.head_bwd_stage_ref(None, None, add, None, xbn.detach(), ybn.detach(), gamma.detach(), mean, rstd, relu)
    xb = xbn.detach().clone().requires_grad_(True)
    gm = gamma.detach().clone().requires_grad_(True)
    yb = F.batch_norm(xb, None, None, gm, beta.detach(), training=True, eps=eps)
    ((torch.relu(yb) if relu else yb) * add).sum().backward()
    assert none1 is None and none2 is None and torch.allclose(dx2, xb.grad, rtol=1e-10, atol=1e-11) and torch.allclose(dgamma2, gm.grad, rtol=1e-10, atol=1e-11)
    assert torch.allclose(dbeta2, (add * (ybn.detach() > 0) if relu else add).sum(0), rtol=1e-12, atol=1e-12)


def test_head_restatement_masks_both_zeros():
    z = torch.zeros(4, 4, dtype=torch.float64)
    ybn = torch.tensor([[1.0, -1.0, 0.0, -0.0]] * 4, dtype=torch.float64)
    one = torch.ones(4, dtype=torch.float64)
    dx, dgamma, dbeta, _, _ = hec.head_bwd_stage_ref(None, None, z + 1.0, None, z, ybn, one, one * 0, one, 1)
    assert dbeta.tolist() == [4.0, 0.0, 0.0, 0.0]


def _cos_mean(a, b):
    return torch.nn.CosineSimilarity()(a.double(), b.double()).mean()


def _torch_cos_entries(feats, B, nlocal):
    cl = lambda pre_a, pro_a, pre_b, pro_b: -(_cos_mean(pre_a, pro_b) + _cos_mean(pre_b, pro_a)) * 0.5
    glob, loc = [], []
    for pro1, pre1, pro2, pre2, proL, preL in feats:
        glob.append(cl(pre1, pro1, pre2, pro2))
        tot = 0.0
        for i in range(nlocal):
            pl, ql = proL[B * i:B * (i + 1)], preL[B * i:B * (i + 1)]
            tot = tot + cl(pre1, pro1, ql, pl) + cl(pre2, pro2, ql, pl)
        loc.append(tot / (2 * nlocal))
    return glob + loc


def test_validation_restatements_against_float64_torch():
    B, nl = 3, 2
    out1, masks, gt = hec.val_maps3d(B, 50, seed=1)
    feats = hec.val_feats(B, nl, hec.C3_B, seed=2)
    acc, absw = hec.val_metrics_ref(out1, masks, gt, feats, B, nl)
    want = torch.stack([F.mse_loss(m, gt) for m in (out1, *masks)] + _torch_cos_entries(feats, B, nl))
    assert torch.allclose(acc / B, want, rtol=1e-12, atol=1e-15)
    assert bool((absw >= acc.abs() * (1 - 1e-12)).all()) and torch.equal(absw[:4], acc[:4])
    H, W = 32, 48
    out1, masks, gt = hec.val_maps2d(B, H, W, seed=3)
    feats = hec.val_feats(B, nl, hec.C5, seed=4)
    acc, absw = hec.val2d_metrics_ref(out1, masks, gt, feats, B, nl)
    up = lambda m: m if m.shape[-1] == W else F.interpolate(m, scale_factor=W // m.shape[-1], mode="bilinear")
    want = torch.stack([F.mse_loss(out1, gt)] + [F.mse_loss(up(m), gt) for m in masks] + _torch_cos_entries(feats, B, nl))
    assert acc.shape == (16,) and torch.allclose(acc / B, want, rtol=1e-12, atol=1e-15)
    for k, m in enumerate(masks):          # the interpolation itself, element by element (dyadic weights: torch's float64 result is exact too)
        assert torch.equal(hec.bilinear_up(m, 1 << (4 - k)), up(m)), k
    one = torch.ones(1, 3, 1, 1, dtype=torch.float64) * 0.375
    assert torch.equal(hec.bilinear_up(one, 16), one.expand(1, 3, 16, 16))


def test_cosine_restatement_on_degenerate_rows():
    """rows below eps: the explicit formula divides by eps, not by the norm; a zero row gives exactly 0"""
    x = torch.tensor([[3e-10, 4e-10], [0.0, 0.0], [3.0, 4.0]])
    y = torch.tensor([[1.0, 0.0], [1.0, 1.0], [3.0, 4.0]])
    c = hec.cos_rows(x, y)
    assert float(c[1]) == 0.0 and abs(float(c[2]) - 1.0) < 1e-15
    assert abs(float(c[0]) - float(x[0, 0].double()) / hec.EPS) < 1e-15 and hec.EPS != 1e-8 and abs(hec.EPS - 1e-8) < 1e-15


# ---- 5. prototypes ----
def test_prototypes_have_the_argument_order_the_gpu_tests_rely_on():
    from pcrlv2_amd import _lib
    protos = _lib.parse_header()
    names = lambda f: [n for _, n in protos[f][1]]
    assert names("pcrl_head_bwd_stage") == ["dy", "W", "add", "xin", "xbn", "ybn", "gamma", "mean", "rstd", "dx", "dgamma", "dbeta", "dW", "db",
                                            "N", "K", "C", "relu", "stream"]
    feats = [f"{t}_{k}" for k in range(3) for t in ("pro1", "pre1", "pro2", "pre2", "proL", "preL")]
    assert names("pcrl_val_metrics") == ["out1", "mask0", "mask1", "mask2", "gt"] + feats + ["acc", "ws", "ws_bytes", "B", "S", "nlocal", "C0", "C1", "C2",
                                                                                         "eps", "stream"]
    assert names("pcrl_val_metrics_ws_bytes") == ["n", "B", "nlocal"]
    assert names("pcrl_val2d_metrics") == ["out1", "masks", "gt", "feats", "C", "acc", "ws", "ws_bytes", "B", "H", "W", "nlocal", "eps", "stream"]
    assert names("pcrl_val2d_metrics_ws_bytes") == ["B", "H", "W", "nlocal"]
    assert names("pcrl_cls_head_fwd") == ["a", "keep", "keep_scale", "w", "b", "labels", "probs", "pooled", "loss", "ws", "ws_bytes", "N", "H", "W", "C", "K",
                                          "dtype", "stream"]
    assert names("pcrl_cls_head_bwd") == ["probs", "labels", "dloss", "pooled", "keep", "keep_scale", "w", "da", "dw", "db", "N", "H", "W", "C", "K", "dtype",
                                          "stream"]
    assert dict((n, t) for t, n in protos["pcrl_val_metrics"][1])["eps"] == "float" and dict((n, t) for t, n in protos["pcrl_val_metrics"][1])["S"] == "int64_t"
    assert dict((n, t) for t, n in protos["pcrl_val2d_metrics"][1])["eps"] == "float"
