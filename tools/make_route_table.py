#!/usr/bin/env python3
"""The routing table of the convolution dispatchers: what every host-side query of the 3D conv, composed up-conv, transposed-conv, to-1, c1,
2D conv and stem families answers for the model's layer shapes and a set of awkward ones, under every test-hook setting.

tests/test_routes_cpu.py compares the library against tests/golden/route_table.npz (integers only).  The fixture pins the dispatchers against
the revision BEFORE a change, so it is generated from a build of the PARENT commit, never from the code under test:

    git archive HEAD^ | tar -x -C /tmp/parent && (cd /tmp/parent && python -m pcrlv2_amd.build)
    PCRL_LIB=/tmp/parent/pcrlv2_amd/lib/libpcrl_hip.so python tools/make_route_table.py        # writes tests/golden/route_table.npz

(PCRL_LIB: pcrlv2_amd/_lib.py loads that library instead of the tree's own.)  Every query is a pure host function: no GPU is needed.  The
environment switches the dispatchers read (PCRL_DGRAD_BNRED, PCRL_IGEMM_VMAJOR, PCRL_UPC_PACK_TILED) must be unset: the table holds their defaults.
"""
import hashlib
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "route_table.npz")
ENV_SWITCHES = ("PCRL_DGRAD_BNRED", "PCRL_IGEMM_VMAJOR", "PCRL_UPC_PACK_TILED")
F32, BF16 = 0, 1
ACT_NONE, ACT_RELU = 0, 1


def settings():
    """(conv impl, wgrad impl, wgrad tr, conv2d impl): every value of one hook with the others at their defaults."""
    out = [(c, 0, 1, 0) for c in range(7)]
    out += [(0, w, tr, 0) for w in (0, 1, 2, 4, 5, 6) for tr in (1, 0) if (w, tr) != (0, 1)]
    out += [(0, 0, 1, c2) for c2 in (1, 2)]
    return out


def apply_setting(L, s):
    L.debug_set_conv_impl(s[0])
    L.debug_set_wgrad_impl(s[1])
    L.debug_set_wgrad_tr(s[2])
    L.debug_set_conv2d_impl(s[3])


def reset_hooks(L):
    apply_setting(L, (0, 0, 1, 0))
    L.fn["pcrl_debug_set_reduce_repeat"][0](1)


def _levels(n, dhw):
    d, h, w = dhw
    return [(n, d >> k, h >> k, w >> k) for k in range(4)]


def model3d(n, dhw):
    """The launches of PCRLv23d on a batch of n crops of dhw: (kind, N, D, H, W, channels...)."""
    lv = _levels(n, dhw)
    out = []
    for k, g in enumerate(lv):                       # encoder stage k: in -> 32 * 2^k -> 64 * 2^k
        out.append(("c1", *g, 32) if k == 0 else ("conv", *g, 32 << k, 32 << k))
        out.append(("conv", *g, 32 << k, 64 << k))
    for k in (2, 1, 0):                              # decoder stage k: up-conv from level k + 1, two convolutions, the deep-supervision head
        c = 128 << k
        out.append(("upc", *lv[k + 1], c, c, c // 2))
        out.append(("convt", *lv[k + 1], c, c))
        out.append(("conv", *lv[k], c, c // 2))      # the uncomposed form of the stage's first convolution
        out.append(("conv", *lv[k], c // 2, c // 2))
        out.append(("to1", *lv[k], c // 2, 27))
    out.append(("to1", *lv[0], 64, 1))
    return out


AWKWARD_3D = [
    (4, 16, 16, 24), (4, 16, 16, 8), (4, 8, 16, 24), (2, 16, 24, 40), (3, 6, 16, 16), (2, 10, 8, 8), (5, 4, 8, 16), (1, 4, 8, 8), (2, 12, 12, 12),
    (7, 3, 5, 7), (64, 2, 2, 2), (16, 1, 1, 1), (2, 32, 32, 48), (1, 128, 128, 128),
]
AWKWARD_CH = [(32, 32), (64, 96), (96, 96), (96, 64), (128, 64), (256, 512), (48, 64), (64, 40), (20, 20)]
DEGENERATE_3D = [(0, 16, 16, 16), (4, 0, 16, 16), (4, 16, 16, 0), (-1, 16, 16, 16), (4, 16, -16, 16)]
# the queries that guard their extents themselves; the others divide by what the extents make of a plan and are asked valid shapes only
GUARDED_3D = ("pcrl_conv3d_k3_fwd_ws_bytes", "pcrl_conv3d_k3_fwd_affine_fused", "pcrl_conv3d_k3_fwd_affine_ws_bytes", "pcrl_conv3d_k3_dgrad_bnred_rows",
              "pcrl_upconv_dgrad_ws_bytes", "pcrl_upconv_wgrad_accum_ws_bytes", "pcrl_upconv_wgrad_ws_bytes")


def conv3_queries(g, ci, co, only=None):
    q = []
    for dt in (F32, BF16):
        for name in ("pcrl_conv3d_k3_stats_rows", "pcrl_conv3d_k3_fwd_kernel", "pcrl_conv3d_k3_fwd_ws_bytes", "pcrl_conv3d_k3_fwd_affine_fused",
                     "pcrl_conv3d_k3_fwd_affine_ws_bytes"):
            q.append((name, (*g, ci, co, dt)))
        for act in (ACT_RELU, ACT_NONE):
            q.append(("pcrl_conv3d_k3_dgrad_bnred_rows", (*g, ci, co, act, dt)))
    q.append(("pcrl_conv3d_k3_wgrad_ws_bytes", (*g, ci, co)))
    return [x for x in q if only is None or x[0] in only]


def upc_queries(g, ci, cm, co, only=None):
    q = []
    for dt in (F32, BF16):
        for name in ("pcrl_upconv_fwd_uses_brick", "pcrl_upconv_stats_rows", "pcrl_upconv_dgrad_uses_brick", "pcrl_upconv_dgrad_ws_bytes",
                     "pcrl_upconv_wgrad_uses_brick", "pcrl_upconv_wgrad_accum_ws_bytes"):
            q.append((name, (*g, ci, co, dt)))
        q.append(("pcrl_upconv_wgrad_ws_bytes", (*g, ci, cm, co, dt)))
        if only is None:
            q.append(("pcrl_upconv_compose_ws_bytes", (ci, cm, co, dt)))
            q.append(("pcrl_upconv_wgrad_finish_ws_bytes", (ci, cm, co, dt)))
    return [x for x in q if only is None or x[0] in only]


def c1_queries(g, co):
    return [("pcrl_conv3d_k3_c1_stats_rows", (*g, co, dt)) for dt in (F32, BF16)] + [("pcrl_conv3d_k3_c1_wgrad_ws_bytes", (*g, co))]


def to1_queries(g, c, taps):
    return ([("pcrl_conv3d_to1_stats_rows", (*g, c, taps, dt)) for dt in (F32, BF16)]
            + [("pcrl_conv3d_to1_fwd_ws_bytes", (*g, c, taps)), ("pcrl_conv3d_to1_wgrad_ws_bytes", (*g, c, taps))])


def cases3d():
    q = []
    launches = []
    for n, dhw in ((32, (64, 64, 32)), (192, (16, 16, 16)), (8, (128, 128, 64)), (48, (16, 16, 16))):     # C2 and C4: global views, local views
        launches += model3d(n, dhw)
    for la in dict.fromkeys(launches):
        kind, g, ch = la[0], la[1:5], la[5:]
        if kind == "conv":
            q += conv3_queries(g, *ch)
        elif kind == "c1":
            for co in (16, 32, 64):
                q += c1_queries(g, co)
        elif kind == "to1":
            q += to1_queries(g, *ch)
        elif kind == "convt":
            q.append(("pcrl_convt3d_k2s2_wgrad_ws_bytes", (*g, *ch)))
        else:
            q += upc_queries(g, *ch)
    for g, (ci, co) in itertools.product(AWKWARD_3D, AWKWARD_CH):
        if ci % 32 == 0 and co % 32 == 0:
            q += conv3_queries(g, ci, co) + upc_queries(g, ci, ci, co)
            q.append(("pcrl_convt3d_k2s2_wgrad_ws_bytes", (*g, ci, co)))
        else:
            q += conv3_queries(g, ci, co, GUARDED_3D) + upc_queries(g, ci, ci, co, GUARDED_3D)     # channel counts no kernel takes
            q += conv3_queries(g, ci, co, ("pcrl_conv3d_k3_stats_rows", "pcrl_conv3d_k3_fwd_kernel"))
    for g in AWKWARD_3D:
        q += c1_queries(g, 32) + to1_queries(g, 64, 27) + to1_queries(g, 96, 27) + to1_queries(g, 64, 1) + to1_queries(g, 520, 1)
    for g in DEGENERATE_3D:
        q += conv3_queries(g, 64, 64, GUARDED_3D) + upc_queries(g, 128, 128, 64, GUARDED_3D)
    return q


def model2d(n, size):
    """Convolutions of the ResNet-18 U-Net (PCRLv2) on n images of size^2: (N, Hi, Wi, Ci, Co, K, stride, up, out_f32)."""
    out = []
    h = size // 4                                     # behind the stem and the max pool
    cin = 64
    for c in (64, 128, 256, 512):                     # layer1..4: two BasicBlocks each
        s = 1 if c == 64 else 2
        out.append((n, h, h, cin, c, 3, s, 0, 0))
        if s == 2:
            out.append((n, h, h, cin, c, 1, 2, 0, 0))
            h //= 2
        out += [(n, h, h, c, c, 3, 1, 0, 0)] * 3
        cin = c
    for cin, c in ((512, 256), (256, 128), (128, 64), (64, 32), (32, 16)):      # decoder blocks: upsample + conv1, conv2, deep-supervision head
        out.append((n, h, h, cin, c, 3, 1, 1, 0))
        h *= 2
        out.append((n, h, h, c, c, 3, 1, 0, 0))
        out.append((n, h, h, c, c, 3, 1, 0, 0))
        out.append((n, h, h, c, 3, 1, 1, 0, 1))
    out.append((n, h, h, 16, 3, 3, 1, 0, 1))          # segmentation head
    return out


AWKWARD_2D = [
    (4, 24, 40, 32, 32, 3, 1, 0, 0), (3, 32, 32, 64, 64, 3, 1, 0, 0), (4, 20, 20, 64, 64, 3, 1, 0, 0), (4, 32, 48, 96, 96, 3, 1, 0, 0),
    (8, 16, 16, 8, 8, 3, 1, 0, 0), (8, 16, 16, 8, 24, 1, 1, 0, 0), (8, 16, 16, 40, 16, 3, 1, 1, 0), (4, 32, 32, 64, 64, 5, 1, 0, 0),
    (4, 32, 32, 64, 64, 3, 2, 0, 0), (4, 32, 32, 32, 32, 3, 1, 0, 1), (4, 64, 64, 64, 32, 3, 1, 1, 0), (4, 7, 9, 16, 16, 3, 1, 0, 0),
]


def _pad8(c):
    return (c + 7) // 8 * 8


def cases2d():
    q = []
    layers = model2d(64, 512) + model2d(384, 96) + AWKWARD_2D       # the C5 per-GPU step: global views 512^2 b = 64, six local views 96^2 per image
    for n, hi, wi, ci, co, k, stride, up, f32 in dict.fromkeys(layers):
        pad = (k - 1) // 2
        hl, wl = (2 * hi, 2 * wi) if up else (hi, wi)
        ho, wo = (hl + 2 * pad - k) // stride + 1, (wl + 2 * pad - k) // stride + 1
        cip, cop = _pad8(ci), _pad8(co)
        q.append(("pcrl_conv2d_packed_elems", (co, k * k, cip)))
        q.append(("pcrl_conv2d_packed_elems", (ci, k * k, cop)))
        q.append(("pcrl_conv2d_stats_rows", (n, ho, wo)))
        q.append(("pcrl_conv2d_wgrad_ws_bytes", (n, ho, wo, cip, cop, k, k)))
        for dt in (F32, BF16):
            for name in ("pcrl_conv2d_fwd_stats_rows", "pcrl_conv2d_fwd_stats_only_ok", "pcrl_conv2d_fwd_kind"):
                q.append((name, (n, hi, wi, cip, co, k, k, stride, pad, up, f32, dt)))
            q.append(("pcrl_conv2d_dgrad_kind", (n, hl, wl, ci, ho, wo, cop, k, k, stride, pad, dt)))
            q.append(("pcrl_conv2d_dgrad_up_ok", (n, hi, wi, ci, cop, dt)))
            for act in (ACT_RELU, ACT_NONE):
                q.append(("pcrl_conv2d_dgrad_bnred_rows", (n, hl, wl, ci, cop, act, dt)))
    q.append(("pcrl_conv2d_dgrad_bnred_rows", (0, 32, 32, 64, 64, ACT_RELU, BF16)))
    q.append(("pcrl_conv2d_dgrad_bnred_rows", (4, 32, -32, 64, 64, ACT_RELU, BF16)))
    q.append(("pcrl_stem7_packed_elems", ()))
    for n, h, w in ((64, 512, 512), (384, 96, 96), (4, 224, 224), (4, 64, 64), (2, 130, 128), (2, 48, 80), (1, 16, 64)):
        q += [("pcrl_stem7_ok", (n, h, w, dt)) for dt in (F32, BF16)]
        q += [("pcrl_stem7_stats_rows", (n, h, w)), ("pcrl_stem7_wgrad_ws_bytes", (n, h, w))]
    return q


def cases():
    return list(dict.fromkeys(cases3d() + cases2d()))


def case_digest(q):
    return np.frombuffer(hashlib.sha256(repr(q).encode()).digest(), dtype=np.uint8).astype(np.int64)


def evaluate(L, q):
    """-> int64 [settings][cases]; leaves every hook at its default."""
    table = np.zeros((len(settings()), len(q)), dtype=np.int64)
    try:
        for i, s in enumerate(settings()):
            apply_setting(L, s)
            for j, (name, args) in enumerate(q):
                v = int(L.fn[name][0](*args))
                assert 0 <= v < 1 << 62, (name, args, v)
                table[i, j] = v
    finally:
        reset_hooks(L)
    return table


def main():
    set_ = [k for k in ENV_SWITCHES if k in os.environ]
    if set_:
        sys.exit(f"unset {', '.join(set_)}: the table holds the dispatchers' defaults")
    sys.path.insert(0, ROOT)
    from pcrlv2_amd import _lib
    L = _lib.lib()
    q = cases()
    table = evaluate(L, q)
    np.savez_compressed(FIXTURE, table=table, settings=np.array(settings(), dtype=np.int64), digest=case_digest(q))
    print(f"{FIXTURE}: {table.shape[0]} settings x {table.shape[1]} queries from {_lib.LIBPATH} ({os.path.getsize(FIXTURE)} bytes)")


if __name__ == "__main__":
    main()
