"""CPU: the case tables of tests/conv1_cases.py hold what the GPU tests (test_conv_to1_exact_gpu.py, test_convt_exact_gpu.py) rely on -- every
precondition of exact summation (never skipped, no tolerance), the route each case expects from the mirrored predicates and from the library's own
host-side queries, the constant each case names is really crossed, and the tables together reach every route and every hook pair."""
import os

import pytest
import torch

import conv1_cases as K
import exact_lattice as X

BF16, F32 = K.BF16, K.F32


@pytest.fixture(scope="module")
def L():
    from pcrlv2_amd import _lib
    if not os.path.exists(_lib.LIBPATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.lib()
    yield lib
    lib.debug_set_conv_impl(0)
    lib.debug_set_wgrad_impl(0)
    lib.debug_set_wgrad_tr(1)


def code(dt):
    return 1 if dt == BF16 else 0


def test_constants_match_the_source():
    assert K.source_pins_missing() == []


# ---- preconditions -------------------------------------------------------------------------------------------------------------------------
def _to1_problems():
    p = {(c.vol, c.C, c.taps, c.bias) for c in K.fwd_cases()}
    p |= {(c.vol, c.C, c.taps, True) for c in K.wgrad_cases()}
    return sorted(p)


@pytest.mark.parametrize("vol,C,taps,bias", _to1_problems(), ids=lambda v: K.vid(v) if isinstance(v, tuple) else str(v))
def test_to1_preconditions(vol, C, taps, bias):
    """to1_reference asserts forward, weight gradient, the bias gradient's float32 value and every statistics row (sum y
    on both lattices, sum y^2 on the ternary one, for the brick rows and the 1024-voxel rows).  The outputs are float32: no output rounding to exercise."""
    for lat in ("fine", "ternary"):
        R = K.to1_reference(vol, C, taps, lat, bias)
        assert all(0 <= m < 1 for m in R.margins.values()), R.margins
        assert K.to1_accepts(C, taps, BF16) or K.to1_accepts(C, taps, F32)


@pytest.mark.parametrize("vol,C,taps", sorted({(c.vol, c.C, c.taps) for c in K.dgrad_cases()}), ids=lambda v: K.vid(v) if isinstance(v, tuple) else str(v))
def test_to1_dgrad_preconditions(vol, C, taps):
    """summable with the add term; and the lattice is fine enough that a bf16 output is rounded (27 taps: already without the add term)"""
    R = K.to1_dgrad_reference(vol, C, taps)
    assert 0 <= R.margin < 1
    assert not torch.equal(R.dx_add.to(BF16).double(), R.dx_add)
    assert taps == 1 or not torch.equal(R.dx.to(BF16).double(), R.dx)


def test_to1_margins_named_by_the_design_note():
    """the largest fractions of 2^24, as DESIGN.md quotes them"""
    R = K.to1_reference((2, 8, 16, 24), 512, 27, "fine")
    assert R.margins["fwd"] < 0.01
    T = K.to1_reference((2, 8, 16, 24), 512, 27, "ternary")
    assert T.margins["sum y^2 rows brick=False"] < 0.5 and T.margins["sum y^2 rows brick=True"] < 0.5
    whole = float((T.y * T.y).sum()) / X.EXACT_LIMIT
    assert whole > 1, f"sum y^2 over the whole tensor is {whole:.2f} of the limit: it would be summable as one row; the per-row rule is not needed"


@pytest.mark.parametrize("s", K.CT_SHAPES, ids=K.ct_id)
def test_convt_preconditions(s):
    R = K.convt_reference(s.vol, s.Ci, s.Co)
    assert all(0 <= m < 1 for m in R.margins.values()), R.margins
    assert not torch.equal(R.y.to(BF16).double(), R.y), "the forward never needs rounding to bf16 on this lattice"
    assert not torch.equal(R.dx.to(BF16).double(), R.dx), "the data gradient never needs rounding to bf16 on this lattice"


def test_device_side_cases_are_summable_for_every_draw():
    """worst-case bounds (largest magnitudes everywhere) of the cases that are generated on the device"""
    for s in K.CT_BIG:
        assert K.worst_units(s.Ci, X.fine_for(s.Ci), "x", "w", extra="b") < X.EXACT_LIMIT, s
        assert K.worst_units(8 * s.Co, X.fine_for(8 * s.Co), "dy", "w") < X.EXACT_LIMIT, s       # data gradient: K = 8 Co
    for c in K.BIG_WG:
        assert K.worst_units(K.voxels(c.vol), X.TERNARY, "x", "dy") < X.EXACT_LIMIT, c      # dw[c][t]: at most M products of magnitude one
        assert K.voxels(c.vol) < X.EXACT_LIMIT                                               # db: an integer of magnitude <= M is a float32 value
    assert not K.worst_units(K.voxels(K.V_IM2COL_CAP), X.FINE, "x", "dy") < X.EXACT_LIMIT, "the fine lattice would do: use it"


# ---- routes --------------------------------------------------------------------------------------------------------------------------------
def test_to1_forward_routes(L):
    routes, impls = set(), set()
    for c in K.fwd_cases():
        assert K.to1_accepts(c.C, c.taps, c.dt), c
        assert c.route == K.to1_fwd_route(c.vol, c.C, c.taps, c.dt, c.ws, c.impl)
        L.debug_set_conv_impl(c.impl)
        try:
            rows = L.call("pcrl_conv3d_to1_stats_rows", *c.vol, c.C, c.taps, code(c.dt))
            nb = L.call("pcrl_conv3d_to1_fwd_ws_bytes", *c.vol, c.C, c.taps)
        finally:
            L.debug_set_conv_impl(0)
        assert rows == K.to1_stats_rows(c.vol, c.C, c.taps, c.dt, c.impl), c
        assert rows == (K.nbricks(c.vol) if c.route in (K.FWD_BRICK, K.FWD_BRICK_PACKED) else -(-K.voxels(c.vol) // K.TO1_VOX)), c
        if c.route == K.FWD_TWOPASS:
            assert nb > 0 and K.voxels(c.vol) % 4 == 0 and c.C % 32 == 0, c
        if c.ws and c.taps == 27 and c.C % 32 == 0:
            assert nb >= (c.C // 32) * 2048, "the two-pass workspace also holds the brick kernel's packed image"
        routes.add((c.route, c.dt))
        impls.add(c.impl)
    assert impls == {0, 1}
    assert routes == {(K.FWD_GATHER, BF16), (K.FWD_GATHER, F32), (K.FWD_FAST, BF16), (K.FWD_FAST, F32), (K.FWD_TWOPASS, BF16), (K.FWD_TWOPASS, F32),
                      (K.FWD_BRICK, BF16), (K.FWD_BRICK_PACKED, BF16)}, routes


def test_to1_forward_cases_cross_their_constants():
    by = {}
    for c in K.fwd_cases():
        by.setdefault(c.route, []).append(c)
    g27 = [c for c in by[K.FWD_GATHER] if c.taps == 27]
    assert any(K.lpv(c.C, c.dt) == 1 for c in g27 if c.dt == BF16) and any(K.lpv(c.C, c.dt) == 1 for c in g27 if c.dt == F32)
    for dt in (BF16, F32):      # lanes stride over the vectors with a remainder; the cap of 64 lanes with a vector left over
        assert any((c.C // K.vec(dt)) % K.lpv(c.C, dt) != 0 and K.lpv(c.C, dt) < K.LPV_CAP for c in g27 if c.dt == dt) or dt == F32
        assert any(K.lpv(c.C, dt) == K.LPV_CAP and c.C // K.vec(dt) > K.LPV_CAP for c in g27 if c.dt == dt)
    assert any(c.vol == K.V_M105 and c.ws and K.voxels(c.vol) % 4 != 0 for c in g27), "a workspace with M % 4 != 0 must reach the gather kernel"
    assert max(c.C for c in g27) == 600 and 27 * 600 * 4 <= K.LDS_NO_OPT_IN < 27 * 608 * 4
    assert not K.to1_accepts(608, 27, BF16) and K.to1_accepts(608, 1, BF16) and K.to1_accepts(1024, 1, BF16)
    tp = by[K.FWD_TWOPASS]
    assert any(K.voxels(c.vol) <= K.TO1_VOX for c in tp) and any(K.TO1_VOX < K.voxels(c.vol) < 2 * K.TO1_VOX for c in tp)
    assert {c.C for c in tp if c.impl == 0} >= {32, 96, 256} and any(c.impl == 1 and K.is_brick_volume(c.vol) for c in tp)
    assert any(c.vol == K.V_ODD and c.ws for c in tp) and any(c.vol == K.V_ODD and not c.ws and c.C in (64, 96) and c.dt == BF16 for c in g27)
    for route in (K.FWD_BRICK, K.FWD_BRICK_PACKED):
        assert {(c.vol, c.C) for c in by[route]} == {(v, C) for v in K.BRICK_VOLS for C in (32, 96, 128, 160, 512)}
    assert any(c.C <= 128 for c in by[K.FWD_BRICK_PACKED]) and any(c.C > 128 for c in by[K.FWD_BRICK_PACKED])
    assert {K.nbricks(v) for v in K.BRICK_VOLS} == {1, 6, 24} and any(K.nbricks(v) % 8 == 0 for v in K.BRICK_VOLS)      # the XCD block map and the plain one
    fast, loop1 = by[K.FWD_FAST], [c for c in by[K.FWD_GATHER] if c.taps == 1]
    assert {(c.C, c.dt) for c in fast} == {(8, BF16), (64, BF16), (512, BF16), (64, F32)} and {(c.C, c.dt) for c in loop1} == {(96, BF16), (12, F32)}
    for cs in (fast, loop1):
        M2 = K.voxels(K.V_BLK2)
        assert any(c.vol == K.V_ROW for c in cs) and any(c.vol == K.V_BLK2 for c in cs) and K.TO1_VOX < M2 < 2 * K.TO1_VOX
    for c in fast:      # second block: whole and partial groups of the 4-deep unroll, and lanes whose voxel is past the end inside a group
        if c.vol == K.V_BLK2:
            vpp, tail = 256 // K.lpv(c.C, c.dt), K.voxels(c.vol) - K.TO1_VOX
            groups = -(-tail // vpp)
            assert tail % vpp != 0 or groups % K.TO1_UNROLL != 0, c
    assert any(not c.bias for c in fast) and any(not c.bias for c in g27)


def test_to1_dgrad_cases_cross_their_constants():
    cs = K.dgrad_cases()
    assert {(c.taps, c.dt, c.add) for c in cs} >= {(t, dt, a) for t in (27, 1) for dt in (F32, BF16) for a in ("none", "other", "inplace")}
    over = [c for c in cs if K.dgrad_passes(c.vol, c.C, c.dt)[1] > 1]
    assert len(over) == 1 and over[0].vol == K.V_DGRAD_CAP and over[0].add == "other" and over[0].taps == 27
    c = over[0]
    assert K.voxels(c.vol) * c.C // K.vec(c.dt) == 2228224 > K.DGRAD_CAP * 256 == 2097152
    assert all(K.to1_accepts(c.C, c.taps, c.dt) for c in cs)
    assert any((c.C // K.vec(c.dt)) & (c.C // K.vec(c.dt) - 1) for c in cs), "C / vec a power of two everywhere: idx % nvec never leaves a remainder pattern"


def test_to1_wgrad_routes_and_constants(L):
    seen = set()
    try:
        for c in K.wgrad_cases() + K.BIG_WG:
            L.debug_set_wgrad_impl(c.impl)
            L.debug_set_wgrad_tr(c.tr)
            assert c.route == K.scalar_wgrad_route(c.vol, c.C, c.taps, c.dt, c.impl, c.tr) == L.call("pcrl_conv3d_to1_wgrad_route", *c.vol[1:], c.C, c.taps, code(c.dt)), c
            M, need = K.voxels(c.vol), L.call("pcrl_conv3d_to1_wgrad_ws_bytes", *c.vol, c.C, c.taps)
            if c.route == K.WG_BRICK:
                assert K.scalar_brick_ws_bytes(c.vol, c.C) <= need
            elif c.route == K.WG_PLAIN:
                assert K.plain_ws_bytes(M, c.C, 2 if c.dt == BF16 else 4) <= need
            else:
                assert 8192 + L.call("pcrl_colsum_ws_bytes", M, c.C) <= need
            seen.add((c.route, c.dt, c.impl, c.tr, c.taps))
    finally:
        L.debug_set_wgrad_impl(0)
        L.debug_set_wgrad_tr(1)
    assert seen == {(K.WG_BRICK, BF16, 0, 1, 27), (K.WG_PLAIN, BF16, 1, 1, 27), (K.WG_PLAIN, BF16, 0, 0, 27), (K.WG_PLAIN, F32, 0, 1, 27),
                    (K.WG_PLAIN, BF16, 0, 1, 27), (K.WG_POINTWISE, BF16, 0, 1, 1), (K.WG_POINTWISE, F32, 0, 1, 1), (K.WG_PLAIN, BF16, 1, 1, 1),
                    (K.WG_PLAIN, F32, 1, 1, 1)}, seen
    bricks = {(c.vol, c.C): K.scalar_brick_plan(c.vol, c.C) for c in K.wgrad_cases() if c.route == K.WG_BRICK}
    assert {C for (v, C) in bricks if v == (2, 8, 16, 24)} == {8, 64, 96, 512} and all(bricks[(2, 8, 16, 24), C][0] == 1 for C in (8, 64, 96, 512))
    assert bricks[K.V_PER2, 512] == (2, 33, 2) and K.nbricks(K.V_PER2) == 66 > K.SCALAR_BRICK_BLOCKS // 8       # per = 2, 33 blocks, even
    assert bricks[K.V_UNEVEN, 512] == (2, 33, 1) and K.nbricks(K.V_UNEVEN) == 65                                 # the last block has one brick
    db, col = K.BIG_WG
    assert K.vecsum_passes(K.voxels(db.vol))[0] == K.VECSUM_CAP and K.voxels(db.vol) > K.VECSUM_CAP * K.VECSUM_VOX
    assert all(K.vecsum_passes(K.voxels(c.vol))[0] < K.VECSUM_CAP for c in K.wgrad_cases())
    assert K.im2col_passes(K.voxels(col.vol), col.dt) == (K.IM2COL_CAP, 2) and K.voxels(col.vol) > K.IM2COL_CAP * 256 // 4 and not K.is_brick_volume(col.vol)
    assert all(K.im2col_passes(K.voxels(c.vol), c.dt)[1] == 1 for c in K.wgrad_cases())


def test_convt_routes_and_constants(L):
    kernels, wg = set(), set()
    try:
        for s, dt, impl, bias in K.convt_fwd_runs():
            L.debug_set_conv_impl(impl)
            k = L.call("pcrl_convt3d_k2s2_fwd_kernel", s.Ci, s.Co, code(dt))
            assert k == K.convt_fwd_kernel(s.Ci, s.Co, dt, impl), (s, dt, impl)
            kernels.add((k, dt, impl, bias))
        L.debug_set_conv_impl(0)
        for s in K.CT_BIG:
            assert L.call("pcrl_convt3d_k2s2_fwd_kernel", s.Ci, s.Co, 1) == K.CT_STREAM
        for s, dt, impl, tr in K.convt_wgrad_runs():
            L.debug_set_wgrad_impl(impl)
            L.debug_set_wgrad_tr(tr)
            r = L.call("pcrl_convt3d_k2s2_wgrad_route", s.Ci, s.Co, code(dt))
            assert r == K.convt_wgrad_route(s.Ci, s.Co, dt, impl, tr), (s, dt, impl, tr)
            assert K.convt_wgrad_need(K.voxels(s.vol), s.Ci, s.Co, r) <= L.call("pcrl_convt3d_k2s2_wgrad_ws_bytes", *s.vol, s.Ci, s.Co)
            wg.add((r, dt, impl, tr, s.Ci % 64 == 0 and s.Co % 64 == 0))
    finally:
        L.debug_set_conv_impl(0)
        L.debug_set_wgrad_impl(0)
        L.debug_set_wgrad_tr(1)
    assert kernels == {(k, dt, impl, b) for b in (True, False) for k, dt, impl in
                       ((K.CT_STREAM, BF16, 0), (K.CT_IGEMM, BF16, 0), (K.CT_IGEMM, BF16, 1), (K.CT_IGEMM, F32, 0))}, kernels
    A, G = K.CT_WG_ALLTAPS, K.CT_WG_GATHER
    assert wg == {(A, BF16, 0, 1, True), (G, BF16, 0, 1, False), (G, BF16, 1, 1, True), (G, BF16, 1, 1, False), (G, BF16, 0, 0, True), (G, BF16, 0, 0, False),
                  (G, F32, 0, 1, True), (G, F32, 0, 1, False)}, wg
    plans = {K.ct_id(s): (K.voxels(s.vol), K.up2_plan(K.voxels(s.vol), s.Co)) for s in K.CT_SHAPES + K.CT_BIG if K.convt_fwd_kernel(s.Ci, s.Co, BF16, 0)}
    M, p = plans["1x3x5x7-128-64"]      # one block; wave 3 (voxels 96..127) has 9 valid voxels: fragment 0 partly, fragment 1 wholly out of range
    assert (M, p.mblocks) == (105, 1) and M - 96 == 9
    M, p = plans["2x5x6x7-256-128"]
    assert p.mblocks == 4 and M - 3 * K.UP2_ROWS == 36
    M, p = plans["1x3x3x3-512-192"]
    assert (p.split, p.tiles_per_block, p.ct_per_tap) == (8, 3, 3)
    M, p = plans["1x24x32x32-128-192"]    # a block's six column tiles cover two taps at three tiles per tap: tile / ct_per_tap and tile % ct_per_tap both move
    assert (p.split, p.tiles_per_block, p.ct_per_tap, p.nt) == (4, 6, 3, False)
    M, p = plans["2x32x48x32-128-64"]
    assert (p.mblocks, p.split, p.nt) == (K.UP2_FILL, 1, False)
    M, p = plans["3x32x64x32-128-64"]
    assert p.split == 1 and p.nt and M * 8 * 64 * 2 == K.NT_BYTES
    M2, p2 = plans["1x307x20x32-128-64"]
    assert p2.split == 1 and not p2.nt and p2.mblocks == p.mblocks - 1 and M2 % K.UP2_ROWS == 0
    assert {s.Ci for s in K.CT_SHAPES if K.convt_fwd_kernel(s.Ci, s.Co, BF16, 0)} == {128, 256, 512}      # the three K / 128 instances of the kernel
    # the all-taps weight gradient: one split with a K tail, and several splits with a K tail in the last one
    at = {K.ct_id(s): (K.voxels(s.vol), K.plan_up2(K.voxels(s.vol), s.Ci, s.Co)) for s in K.CT_WG_SHAPES if s.Ci % 64 == 0 and s.Co % 64 == 0}
    assert at["1x3x5x7-128-64"] == (105, (1, 128)) and 105 % 32 != 0
    M, (splits, chunk) = at["3x5x11x13-128-64"]
    assert splits > 1 and M % 32 != 0 and (splits, chunk) == (5, 448) and (M - 4 * chunk) % 32 == 1
    assert "2x5x6x7-256-128" in at and any(s.Ci == 32 for s in K.CT_WG_SHAPES)


# ---- the restatements of the large cases agree with the references of the small ones -----------------------------------------------------------
@pytest.mark.parametrize("taps", [27, 1])
def test_to1_wgrad_restatement_is_the_autograd_gradient(taps):
    vol, C = (1, 3, 5, 7), 64
    R = K.to1_reference(vol, C, taps, "ternary")
    dw, db = K.to1_wgrad_restated(R.x[0].permute(1, 2, 3, 0).reshape(-1, C), R.dy[0, 0], taps)
    assert torch.equal(dw, R.dw.reshape(C, taps)) and torch.equal(db, R.db)


def test_convt_restatement_is_conv_transpose3d():
    s = K.CT_SHAPES[2]
    R = K.convt_reference(s.vol, s.Ci, s.Co)
    rows = R.x.permute(0, 2, 3, 4, 1).reshape(-1, s.Ci)
    for b, y in ((R.b, R.y), (None, R.y_nobias)):
        got = K.convt_rows_restated(rows, R.w, b)
        ndhwc = y.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)      # the kernels' memory layout
        assert torch.equal(got, K.convt_rows_view(ndhwc, s.vol))
    dy_rows = K.convt_rows_view(R.dy.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3), s.vol)
    assert torch.equal(K.convt_rows_unview(dy_rows, s.vol), R.dy)
    assert torch.equal(K.convt_dgrad_rows_restated(dy_rows, R.w), R.dx.permute(0, 2, 3, 4, 1).reshape(-1, s.Ci))
