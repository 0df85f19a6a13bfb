"""csrc/optim.hip and pcrlv2_amd.optim's FusedAdam / FusedAdamW / max_grad_norm on the GPU, bit for bit against tests/optim_reference.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import optim_reference as R  # noqa: E402
from pcrlv2_amd import data_seg as D  # noqa: E402
from pcrlv2_amd._lib import lib, stream_handle  # noqa: E402
from pcrlv2_amd.models import Segmenter3d  # noqa: E402
from pcrlv2_amd.optim import FusedAdam, FusedAdamW, FusedSGD  # noqa: E402
from pcrlv2_amd.train_seg import train_step  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
LR, WD, BETAS, EPS = 1e-2, 1e-2, (0.9, 0.999), 1e-8
SMALL = [5, 1, 7, 64, 3, 130, 2]             # the unpadded arena of test_sgd_kernel_on_an_unpadded_arena: groups of four straddle tensors


def _cap():
    cap = lib().fn["pcrl_optim_grid_cap"][0]()
    assert cap == R.GRID_CAP
    return cap


def _wrap_sizes():
    """One group past the grid cap (cap * 256 * 4 + 5 elements): the grid-stride loop wraps once, with a tail of 5."""
    return SMALL + [_cap() * 256 * 4 + 5 - sum(SMALL)]


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _bytes(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def _dev(a, shift=0):
    """numpy -> device; shift = 1: through a pointer one float past a 16-byte boundary (the unaligned path)."""
    t = torch.zeros(len(a) + shift, dtype=torch.from_numpy(a[:0]).dtype, device=DEV)
    t[shift:].copy_(torch.from_numpy(a))
    return t[shift:]


def _gradients(rng, n):
    """2^-10 <= |g| <= 1 with random signs, the CPU test's range: g / (|g| + eps) is well conditioned."""
    return (np.exp2(rng.uniform(-10.0, 0.0, n)) * rng.choice((-1.0, 1.0), n)).astype(F)


class _Tables:
    def __init__(self, n):
        self.ref = R.AdamTables(n)
        self.steps = torch.zeros(n, dtype=torch.int32, device=DEV)
        self.prods = torch.ones(2 * n, dtype=torch.float64, device=DEV)
        self.coefs = torch.zeros(2 * n, dtype=torch.float32, device=DEV)

    def check(self):
        assert np.array_equal(self.steps.cpu().numpy(), self.ref.steps)
        assert self.prods.cpu().numpy().tobytes() == self.ref.prods.tobytes()
        assert self.coefs.cpu().numpy().tobytes() == self.ref.coefs.tobytes()


def _adam_call(p, g, m, v, offs, flags, tab, n, total, decoupled, gs, clip):
    L, s = lib(), stream_handle()
    L.call("pcrl_adam_prepare", flags, tab.steps, tab.prods, tab.coefs, n, LR, BETAS[0], BETAS[1], s)
    L.call("pcrl_adam_step", p, g, m, v, offs, flags, tab.coefs, n, total, (1.0 - LR * WD) if decoupled else WD, int(decoupled),
           1.0 - BETAS[0], BETAS[1], 1.0 - BETAS[1], EPS, gs, clip, s)


@pytest.mark.parametrize("clip", [None, 1.0, 0.25], ids=["noclip", "clip1", "clip0.25"])
@pytest.mark.parametrize("decoupled", [True, False], ids=["adamw", "adam"])
@pytest.mark.parametrize("case", ["unpadded", "unaligned", "wrap"])
def test_adam_step_kernel_bit_for_bit(case, decoupled, clip):
    """pcrl_adam_prepare + pcrl_adam_step through the C ABI, two steps with different has-gradient flags, against the restatement: p, m, v and the
    step / product / coefficient tables bit for bit; a tensor with flag 0 keeps all of them."""
    sizes = _wrap_sizes() if case == "wrap" else SMALL
    shift = 1 if case == "unaligned" else 0
    offs, n = _offsets(sizes), len(sizes)
    total = int(offs[-1])
    rng = np.random.default_rng(21)
    p, m = rng.standard_normal(total).astype(F), (0.1 * rng.standard_normal(total)).astype(F)
    v = (0.01 * rng.random(total)).astype(F)
    pd, md, vd = _dev(p, shift), _dev(m, shift), _dev(v, shift)
    assert pd.data_ptr() % 16 == 4 * shift
    od = torch.from_numpy(offs).to(DEV)
    tab = _Tables(n)
    clip_d = None if clip is None else torch.tensor([clip], dtype=torch.float32, device=DEV)
    for step, flags in enumerate(([1, 1, 0, 1, 1, 0, 1, 1][:n], [1, 0, 1, 1, 0, 0, 1, 1][:n])):
        g = _gradients(rng, total)
        fd = torch.tensor(flags, dtype=torch.int32, device=DEV)
        before = (p.copy(), m.copy(), v.copy(), tab.ref.copy())
        _adam_call(pd, _dev(g, shift), md, vd, od, fd, tab, n, total, decoupled, 0.5, clip_d)
        R.adam_prepare(tab.ref, flags, LR, *BETAS)
        R.adam_step(p, g, m, v, offs, flags, tab.ref, LR, WD, BETAS[0], BETAS[1], EPS, decoupled, 0.5, clip)
        for name, dev, want in (("p", pd, p), ("m", md, m), ("v", vd, v)):
            got = dev.cpu().numpy()
            bad = np.flatnonzero(got.view(np.int32) != want.view(np.int32))
            assert bad.size == 0, f"step {step} {name}: {bad.size} elements differ, first at {bad[:4]}: {got[bad[:4]]} vs {want[bad[:4]]}"
        tab.check()
        for t, f in enumerate(flags):
            if not f:
                sl = slice(int(offs[t]), int(offs[t + 1]))
                assert all(np.array_equal(a[sl].view(np.int32), b[sl].view(np.int32)) for a, b in zip((p, m, v), before[:3]))
                assert tab.ref.steps[t] == before[3].steps[t] and np.array_equal(tab.ref.prods[t], before[3].prods[t])
    assert not np.array_equal(p, before[0])


SHAPES = [(32, 1, 3, 3, 3), (32,), (7,), (64, 32, 3, 3, 3), (5, 3), (1,), (3,)]      # test_fused_sgd_matches_torch_sgd's, plus a 1- and a 3-element parameter


def _no_grad(step, i):
    return i == 2 and step in (0, 2)


def _feed(opt, params, grads, step):
    for i, p in enumerate(params):
        p.grad = None if _no_grad(step, i) else torch.from_numpy(grads[step][i]).to(p.device, p.dtype)
    opt.step()


def _optimizer_inputs(nsteps=4):
    rng = np.random.default_rng(0)
    p0 = [rng.standard_normal(s).astype(F) for s in SHAPES]
    grads = [[_gradients(rng, int(np.prod(s))).reshape(s) for s in SHAPES] for _ in range(nsteps)]
    return p0, grads


def _restate_arena(opt, p0, grads, steps, decoupled, state=None):
    """The restatement on the optimiser's own padded arena layout -> (p, m, v, tables)."""
    offs = np.array(opt._offsets_host, np.int64)
    total = int(offs[-1])
    if state is None:
        p, m, v, tab = np.zeros(total, F), np.zeros(total, F), np.zeros(total, F), R.AdamTables(len(SHAPES))
        for o, x in zip(offs, p0):
            p[o:o + x.size] = x.reshape(-1)
    else:
        p, m, v, tab = state
    for step in steps:
        g = np.zeros(total, F)
        flags = []
        for i, o in enumerate(offs[:-1]):
            flags.append(0 if _no_grad(step, i) else 1)
            if flags[-1]:
                g[o:o + grads[step][i].size] = grads[step][i].reshape(-1)
        R.adam_prepare(tab, flags, LR, *BETAS)
        R.adam_step(p, g, m, v, offs, flags, tab, LR, WD, BETAS[0], BETAS[1], EPS, decoupled)
    return p, m, v, tab


@pytest.mark.parametrize("cls", [FusedAdamW, FusedAdam], ids=["adamw", "adam"])
def test_fused_adam_matches_the_restatement_and_torch(cls):
    """Four steps, one parameter without a gradient on steps 0 and 2: the arenas equal the restatement bit for bit, and the parameters stay within
    the CPU test's bound of float64 torch -- twice stock float32 torch's own distance from it on the same inputs (measured on an MI355X: both 7.7e-7 for
    AdamW, both 3.9e-7 for Adam).  The 1- and 3-element parameters sit in 4-float slots whose padding stays zero in every arena."""
    decoupled = cls is FusedAdamW
    stock = torch.optim.AdamW if decoupled else torch.optim.Adam
    p0, grads = _optimizer_inputs()
    mine = [torch.nn.Parameter(torch.from_numpy(x).to(DEV)) for x in p0]
    opt = cls(mine, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)
    refs = {}
    for dt in (torch.float64, torch.float32):
        ps = [torch.nn.Parameter(torch.from_numpy(x).to(dt).clone()) for x in p0]          # a copy: float32 would alias p0
        o = stock(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, foreach=False)
        for step in range(4):
            _feed(o, ps, grads, step)
        refs[dt] = np.concatenate([p.detach().double().numpy().reshape(-1) for p in ps])
    for step in range(4):
        _feed(opt, mine, grads, step)
    p, m, v, tab = _restate_arena(opt, p0, grads, range(4), decoupled)
    for name, arena, want in (("p", opt.flat_p, p), ("m", opt.flat_m, m), ("v", opt.flat_v, v)):
        assert _bytes(arena) == want.tobytes(), name
    assert np.array_equal(opt._steps.cpu().numpy(), tab.steps) and list(tab.steps) == opt._step_host == [4, 4, 2, 4, 4, 4, 4]
    assert _bytes(opt._prods) == tab.prods.tobytes() and _bytes(opt._coefs) == tab.coefs.tobytes()
    got = np.concatenate([q.detach().double().cpu().numpy().reshape(-1) for q in mine])
    d_torch, d_mine = np.abs(refs[torch.float32] - refs[torch.float64]).max(), np.abs(got - refs[torch.float64]).max()
    print(f"{cls.__name__}: float32 torch vs float64 {d_torch:.3e}, fused vs float64 {d_mine:.3e}")
    assert d_torch > 0 and d_mine <= 2 * d_torch
    for arena in (opt.flat_p, opt.flat_g, opt.flat_m, opt.flat_v):           # slot padding: zero everywhere
        a = arena.cpu().numpy()
        for i, s in enumerate(SHAPES):
            o, n = opt._offsets_host[i], int(np.prod(s))
            assert not a[o + n:opt._offsets_host[i + 1]].any(), (i, s)
    assert opt._offsets_host[6] - opt._offsets_host[5] == 4 and opt._total - opt._offsets_host[6] == 4
    sd = opt.state_dict()
    assert set(sd["state"][0].keys()) == {"step", "exp_avg", "exp_avg_sq"} and sd["state"][2]["step"].dtype == torch.float32
    assert float(sd["state"][2]["step"]) == 2.0 and sd["state"][2]["step"].dim() == 0 and sd["param_groups"][0]["betas"] == BETAS


def test_refused_options():
    ps = [torch.nn.Parameter(torch.zeros(4, device=DEV))]
    for kw, text in ((dict(amsgrad=True), "amsgrad"), (dict(maximize=True), "maximize"), (dict(capturable=True), "capturable")):
        with pytest.raises(ValueError, match=text):
            FusedAdamW(ps, **kw)
    with pytest.raises(ValueError, match="single param group"):
        FusedAdam([{"params": [torch.nn.Parameter(torch.zeros(4, device=DEV))]}, {"params": [torch.nn.Parameter(torch.zeros(4, device=DEV))]}])
    opt = FusedAdamW([torch.nn.Parameter(torch.zeros(4, device=DEV))])
    opt.skip_flag = torch.zeros(1, device=DEV)
    with pytest.raises(RuntimeError, match="the pre-task stays on SGD"):
        opt.step()
    assert opt.grad_norm is None and FusedSGD([torch.nn.Parameter(torch.zeros(4, device=DEV))], lr=0.1).grad_norm is None


# ---- the gradient norm ---------------------------------------------------------------------------------------------------------------
NORM_SIZES = [1, 63, 64, 65, 255, 256, 257, 1025]
NORM_FLAGS = [1, 1, 0, 1, 1, 0, 1, 1, 1]


def _norm_call(g, od, nd, fd, n, total, gs, max_norm):
    parts = torch.zeros(_cap(), dtype=torch.float64, device=DEV)
    norm, coef = torch.zeros(1, dtype=torch.float64, device=DEV), torch.zeros(1, dtype=torch.float32, device=DEV)
    lib().call("pcrl_grad_norm", g, od, nd, fd, n, total, gs, max_norm, parts, norm, coef, stream_handle())
    return norm, coef


@pytest.mark.parametrize("gs", [1.0, 0.5])
@pytest.mark.parametrize("case", ["small", "unaligned", "wrap"])
def test_grad_norm_bit_for_bit_on_exactly_summable_gradients(case, gs):
    """Tensors of 1 .. 1 025 elements (and one that makes the grid-stride loop wrap): norm and coefficient equal the restatement and the exact
    sum's square root bit for bit; tensors with flag 0 hold 1e30 and do not count; a max_norm above the norm gives exactly 1.0f."""
    sizes = NORM_SIZES + ([_cap() * 256 * 4 + 5] if case == "wrap" else [7])
    shift = 1 if case == "unaligned" else 0
    offs, n = _offsets(sizes), len(sizes)
    total = int(offs[-1])
    g = R.summable_grads(total, 31)
    clean = g.copy()
    for t, f in enumerate(NORM_FLAGS):
        if not f:
            g[offs[t]:offs[t + 1]] = 1e30
            clean[offs[t]:offs[t + 1]] = 0
    exact = R.assert_summable(clean, gs)
    gd, od, fd = _dev(g, shift), torch.from_numpy(offs).to(DEV), torch.tensor(NORM_FLAGS, dtype=torch.int32, device=DEV)
    for max_norm in (1.0, 1e9):
        norm, coef = _norm_call(gd, od, None, fd, n, total, gs, max_norm)
        want_norm, want_coef = R.grad_norm(g, offs, NORM_FLAGS, gs, max_norm)
        assert want_norm == np.sqrt(exact)
        assert norm.cpu().numpy().tobytes() == np.float64(want_norm).tobytes(), (float(norm), want_norm)
        assert coef.cpu().numpy().tobytes() == F(want_coef).tobytes(), (float(coef), want_coef)
        assert (float(coef) == 1.0) == (max_norm > want_norm)


def test_grad_norm_leaves_the_slot_padding_out():
    sizes, numels = [4, 4, 8], [3, 1, 5]
    offs = _offsets(sizes)
    g = R.summable_grads(16, 2)
    for t, k in enumerate(numels):
        g[offs[t] + k:offs[t + 1]] = 1e30
    nd = torch.tensor(numels, dtype=torch.int64, device=DEV)
    norm, coef = _norm_call(_dev(g), torch.from_numpy(offs).to(DEV), nd, torch.tensor([1, 1, 1], dtype=torch.int32, device=DEV), 3, 16, 1.0, 0.5)
    want = R.grad_norm(g, offs, [1, 1, 1], 1.0, 0.5, numels=numels)
    assert float(norm) == want[0] < 1e3 and coef.cpu().numpy()[0] == want[1]


@pytest.mark.parametrize("decoupled", [True, False], ids=["adamw", "adam"])
def test_a_coefficient_of_one_leaves_the_adam_step_unchanged(decoupled):
    sizes = NORM_SIZES + [7]
    offs, n = _offsets(sizes), len(sizes)
    total = int(offs[-1])
    rng = np.random.default_rng(8)
    g, p = R.summable_grads(total, 32), rng.standard_normal(total).astype(F)
    od, fd = torch.from_numpy(offs).to(DEV), torch.tensor(NORM_FLAGS, dtype=torch.int32, device=DEV)
    norm, coef = _norm_call(_dev(g), od, None, fd, n, total, 0.5, 1e9)
    assert float(coef) == 1.0
    outs = []
    for clip in (None, coef):
        pd, md, vd, tab = _dev(p), _dev(np.zeros(total, F)), _dev(np.zeros(total, F)), _Tables(n)
        _adam_call(pd, _dev(g), md, vd, od, fd, tab, n, total, decoupled, 0.5, clip)
        outs.append(_bytes(pd) + _bytes(md) + _bytes(vd))
    assert outs[0] == outs[1] and outs[0][:4 * total] != p.tobytes()


@pytest.mark.parametrize("gs", [0.5, 1.0 / 3.0], ids=["half", "third"])
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "unaligned"])
def test_sgd_step_clipped_with_a_coefficient_of_one_has_sgd_steps_bits(shift, gs):
    """pcrl_sgd_step_clipped against pcrl_sgd_step (the kernels of heads_loss.hip, untouched) on the unpadded arena -- 16-byte groups, straddling
    groups and, through pointers one float off, the all-scalar kernel; momentum buffers initialised and not.  And with 0.25 it is pcrl_sgd_step on
    gradients scaled beforehand (a power of two: exact)."""
    L, s = lib(), stream_handle()
    sizes, flags = SMALL + [1025], [1, 3, 0, 3, 1, 2, 3, 3]
    offs, n = _offsets(sizes), len(sizes)
    total = int(offs[-1])
    rng = np.random.default_rng(4)
    p, g, b = (rng.standard_normal(total).astype(F) for _ in range(3))
    od, fd = torch.from_numpy(offs).to(DEV), torch.tensor(flags, dtype=torch.int32, device=DEV)
    lr, mom, wd = 0.05, 0.9, 1e-2

    def run(name, grad, *extra):
        pd, bd = _dev(p, shift), _dev(b, shift)
        L.call(name, pd, _dev(grad, shift), bd, od, fd, n, total, lr, mom, wd, gs, *extra, s)
        return _bytes(pd) + _bytes(bd)

    one, quarter = (torch.tensor([c], dtype=torch.float32, device=DEV) for c in (1.0, 0.25))
    plain = run("pcrl_sgd_step", g)
    assert run("pcrl_sgd_step_clipped", g, one) == plain and plain[:4 * total] != p.tobytes()
    if gs == 0.5:
        assert run("pcrl_sgd_step_clipped", g, quarter) == run("pcrl_sgd_step", g * F(0.25)) != plain


def test_fused_sgd_with_max_grad_norm():
    """FusedSGD(max_grad_norm=...) runs pcrl_grad_norm + pcrl_sgd_step_clipped; a norm below the bound leaves FusedSGD's bytes, a bound below
    the norm scales the update.  Without max_grad_norm the step is pcrl_sgd_step alone."""
    p0, grads = _optimizer_inputs(2)
    outs, calls = {}, {}
    for bound in (None, 1e9, 0.5):
        ps = [torch.nn.Parameter(torch.from_numpy(x).to(DEV)) for x in p0]
        opt = FusedSGD(ps, lr=0.05, momentum=0.9, weight_decay=1e-2, max_grad_norm=bound)
        with lib().count_calls("pcrl_sgd_step", "pcrl_sgd_step_clipped", "pcrl_grad_norm", "pcrl_adam_step") as n:
            for step in range(2):
                _feed(opt, ps, grads, step)
        outs[bound], calls[bound] = _bytes(opt.flat_p) + _bytes(opt.flat_buf), dict(n)
        if bound is not None:
            counted = torch.cat([v.reshape(-1) for i, v in enumerate(opt._gviews) if not _no_grad(1, i)]).double()
            want = float(torch.linalg.vector_norm(counted))
            assert abs(float(opt.grad_norm) - want) <= 1e-12 * want
    assert calls[None] == {"pcrl_sgd_step": 2} and calls[1e9] == calls[0.5] == {"pcrl_grad_norm": 2, "pcrl_sgd_step_clipped": 2}
    assert outs[None] == outs[1e9] != outs[0.5]


# ---- state ------------------------------------------------------------------------------------------------------------------------------
def test_state_round_trip_through_stock_adamw():
    p0, grads = _optimizer_inputs()
    runs = {}
    for name in ("straight", "resumed"):
        ps = [torch.nn.Parameter(torch.from_numpy(x).to(DEV)) for x in p0]
        opt = FusedAdamW(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)
        for step in range(2):
            _feed(opt, ps, grads, step)
        if name == "resumed":
            sd = opt.state_dict()
            cpu = [torch.nn.Parameter(q.detach().cpu().clone()) for q in ps]
            stock = torch.optim.AdamW(cpu, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)
            stock.load_state_dict(sd)                                     # torch accepts the layout
            assert float(stock.state[cpu[0]]["step"]) == 2 and float(stock.state[cpu[2]]["step"]) == 1
            assert torch.equal(stock.state[cpu[3]]["exp_avg"], opt.state[ps[3]]["exp_avg"].cpu())
            ps = [torch.nn.Parameter(q.detach().clone()) for q in ps]
            opt = FusedAdamW(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)
            opt.load_state_dict(stock.state_dict())                       # and a stock state comes back
            assert opt._step_host == [2, 2, 1, 2, 2, 2, 2]
        for step in range(2, 4):
            _feed(opt, ps, grads, step)
        runs[name] = b"".join(_bytes(t) for t in (opt.flat_p, opt.flat_m, opt.flat_v, opt._steps, opt._prods, opt._coefs))
    assert runs["straight"] == runs["resumed"]
    sgd = FusedSGD([torch.nn.Parameter(torch.from_numpy(x).to(DEV)) for x in p0], lr=0.1, momentum=0.9)
    _feed(sgd, sgd._plist, grads, 1)
    with pytest.raises(SystemExit, match="holds the state of optimizer 'sgd', but 'adamw' was asked for"):
        opt.load_state_dict(sgd.state_dict())
    with pytest.raises(SystemExit, match="holds the state of optimizer 'adam', but 'sgd' was asked for"):
        sgd.load_state_dict(opt.state_dict())


# ---- the segmenter -------------------------------------------------------------------------------------------------------------------------
K, B, CROP = 3, 2, (16, 16, 8)
HEAD_PARTS = (".bn.", ".predictor_head.", ".deep_supervision_head.")


def _seg_batch(seed):
    cases = [D.synthetic_case(seed, i, CROP, K) for i in range(B)]
    return torch.from_numpy(np.stack([c.img for c in cases])), torch.from_numpy(np.stack([c.seg for c in cases]))


def _seg_run(dtype):
    torch.manual_seed(0)
    model = Segmenter3d(K).cuda().train().set_compute_dtype(dtype)
    opt = FusedAdamW(model.trainable_parameters(), lr=1e-3, weight_decay=1e-2, max_grad_norm=1.0)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    losses, norms = [], []
    for step in range(3):
        losses.append(train_step(model, opt, _seg_batch(step))[0])
        counted = torch.cat([v.reshape(-1) for p, v in zip(opt._plist, opt._gviews) if p.grad is not None]).double()
        norms.append((float(opt.grad_norm), float(torch.linalg.vector_norm(counted))))
    return model, opt, before, torch.stack([l.float() for l in losses]).cpu(), norms


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_segmenter_steps_with_adamw_and_clipping(dtype):
    model, opt, before, losses, norms = _seg_run(dtype)
    assert bool(torch.isfinite(losses).all())
    after = model.state_dict()
    trainable = {n for n, p in model.named_parameters() if p.requires_grad}
    for k, v in before.items():
        if any(h in k for h in HEAD_PARTS):
            assert torch.equal(v, after[k]), f"{k}: a frozen head's bytes changed"
        elif k in trainable:
            assert not torch.equal(v, after[k]), f"{k}: a trainable parameter did not move"
    for got, want in norms:
        assert want > 0 and abs(got - want) <= 1e-12 * want, (got, want)
    again = _seg_run(dtype)[1]
    for a, b in ((opt.flat_p, again.flat_p), (opt.flat_m, again.flat_m), (opt.flat_v, again.flat_v), (opt.grad_norm, again.grad_norm)):
        assert _bytes(a) == _bytes(b)


DDP2_WORKER = r'''
import os, sys, hashlib, numpy as np, torch, torch.distributed as dist
root = sys.argv[1]
sys.path.insert(0, root)
from pcrlv2_amd import data_seg as D, ddp, optim, optim_cli, seg3d
from pcrlv2_amd.models import Segmenter3d
from pcrlv2_amd.train_seg import train_step
rank, world, _ = ddp.init_process_group_from_env("gloo")     # two processes, ONE GPU: gloo moves the CUDA buffers
torch.cuda.set_device(0)
args = seg3d.build_parser().parse_args(["train", "--data", "synthetic", "--phase", "scratch", "--optimizer", "adamw", "--clip_grad", "1.0"])
seg3d.check_train(args)
torch.manual_seed(0)
model = Segmenter3d(3).cuda().train()
opt = optim.make(model.trainable_parameters(), lr=1e-3, momentum=args.momentum, weight_decay=1e-2, **optim_cli.options(args))
assert type(opt).__name__ == "FusedAdamW" and opt.max_grad_norm == 1.0
dp = ddp.DataParallel(model, opt)
assert dp._active and opt.grad_scale == 0.5
for step in range(2):
    cases = [D.synthetic_case(100 * rank + step, i, (16, 16, 8), 3) for i in range(2)]          # different crops per rank
    loss = train_step(model, opt, (torch.from_numpy(np.stack([c.img for c in cases])), torch.from_numpy(np.stack([c.seg for c in cases]))))[0]
    assert bool(torch.isfinite(loss))
h = hashlib.sha256()
for t in (opt.flat_p, opt.flat_m, opt.flat_v, opt.grad_norm):
    h.update(t.cpu().numpy().tobytes())
mine = torch.tensor(list(h.digest()), dtype=torch.uint8)
both = [torch.zeros(32, dtype=torch.uint8) for _ in range(world)]
dist.all_gather(both, mine)
assert torch.equal(both[0], both[1]), "the ranks ended with different parameter, m, v or grad_norm bytes"
assert float(opt.grad_norm) > 0 and opt._step_host.count(2) > 0
dist.barrier()
print("OK", rank, flush=True)
dist.destroy_process_group()
'''


def test_two_ranks_adamw_clipped_end_with_identical_bytes(tmp_path):
    """Two processes (gloo, both on cuda:0) run the segmenter with --optimizer adamw --clip_grad 1.0 for 2 steps on different crops: the norm is
    taken after the all-reduce, so both ranks end with identical parameter, m, v and grad_norm bytes."""
    script = tmp_path / "ddp2_adamw.py"
    script.write_text(DDP2_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29767", WORLD_SIZE="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, str(script), ROOT], env=dict(env, RANK=str(r), LOCAL_RANK="0"),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = []
    try:
        for p in procs:                                  # each child under its own time limit; the first failure ends the test
            outs.append(p.communicate(timeout=240)[0])
            assert p.returncode == 0, outs[-1][-3000:]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.communicate()
    assert all("OK" in o for o in outs)


def test_command_line_adamw_writes_its_state_and_refuses_an_sgd_resume(tmp_path):
    out_dir = str(tmp_path / "out")
    base = [sys.executable, os.path.join(ROOT, "seg3d.py"), "train", "--data", "synthetic", "--phase", "scratch", "--crop", "16,16,8", "--b", "2",
            "--epochs", "1", "--steps_per_epoch", "2", "--output", out_dir]
    r = subprocess.run(base + ["--optimizer", "adamw", "--clip_grad", "1"], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    path = os.path.join(out_dir, "pcrlv2_seg3d_scratch_1.0_1.pt")
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    assert ckpt["opt"].optimizer == "adamw" and "exp_avg" in ckpt["optimizer"]["state"][0] and float(ckpt["optimizer"]["state"][0]["step"]) == 4
    r = subprocess.run(base + ["--optimizer", "sgd", "--resume", path], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode != 0 and "holds the state of optimizer 'adamw', but 'sgd' was asked for" in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
