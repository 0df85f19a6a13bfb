"""The fine-tuning optimisers without a GPU: the numpy restatement of csrc/optim.hip (tests/optim_reference.py) against stock torch, the
exactly summable inputs of the norm tests, the C ABI and the command lines' optimiser options."""
import ctypes
import os

import numpy as np
import pytest
import torch

import optim_reference as R
from pcrlv2_amd import _lib, optim_cli

F = np.float32
SIZES = (1000, 96, 3000)            # 4 096 elements; the middle tensor has no gradient on steps 0 and 2
LR, WD, BETAS, EPS, STEPS = 1e-2, 1e-2, (0.9, 0.999), 1e-8, 8


def _inputs():
    rng = np.random.default_rng(11)
    p0 = [rng.standard_normal(n) for n in SIZES]
    grads = []
    for _ in range(STEPS):
        # 2^-10 <= |g| <= 1, random signs: |g| stays far above eps, so g / (|g| + eps) is well conditioned
        grads.append([np.exp2(rng.uniform(-10.0, 0.0, n)) * rng.choice((-1.0, 1.0), n) for n in SIZES])
    return [x.astype(F) for x in p0], [[g.astype(F) for g in gs] for gs in grads]


def _has(step, t):
    return not (t == 1 and step in (0, 2))


def _torch_run(cls, dtype, p0, grads):
    ps = [torch.nn.Parameter(torch.tensor(x, dtype=dtype)) for x in p0]
    opt = cls(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, foreach=False)
    for step in range(STEPS):
        for t, p in enumerate(ps):
            p.grad = torch.tensor(grads[step][t], dtype=dtype) if _has(step, t) else None
        opt.step()
    return np.concatenate([p.detach().double().numpy() for p in ps]), opt


def _restatement_run(decoupled, p0, grads):
    offs = np.concatenate([[0], np.cumsum(SIZES)])
    p = np.concatenate(p0).astype(F)
    m, v = np.zeros_like(p), np.zeros_like(p)
    tab = R.AdamTables(len(SIZES))
    for step in range(STEPS):
        flags = [1 if _has(step, t) else 0 for t in range(len(SIZES))]
        g = np.concatenate(grads[step]).astype(F)
        R.adam_prepare(tab, flags, LR, *BETAS)
        R.adam_step(p, g, m, v, offs, flags, tab, LR, WD, BETAS[0], BETAS[1], EPS, decoupled)
    return p, m, v, tab


@pytest.mark.parametrize("decoupled", [True, False], ids=["adamw", "adam"])
def test_restatement_against_stock_torch(decoupled):
    """8 steps on 4 096 elements.  The yardstick is stock float32 torch's own distance (largest |difference| of a parameter) from float64 torch on
    the same inputs; the restatement stays within 2x of it (the margin: the two round in different places).  Measured on the CPU this was written
    on: 9.8e-7 for both with AdamW, 4.7e-7 for both with Adam.  Against float32 torch the restatement differs by at most 1 ulp of p (not a target)."""
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    p0, grads = _inputs()
    ref64, _ = _torch_run(cls, torch.float64, p0, grads)
    ref32, opt32 = _torch_run(cls, torch.float32, p0, grads)
    p, m, v, tab = _restatement_run(decoupled, p0, grads)
    d_torch = np.abs(ref32 - ref64).max()
    d_mine = np.abs(p.astype(np.float64) - ref64).max()
    print(f"{cls.__name__}: float32 torch vs float64 {d_torch:.3e}, restatement vs float64 {d_mine:.3e}, "
          f"restatement vs float32 torch {np.abs(p.astype(np.float64) - ref32).max():.3e}")
    assert d_torch > 0 and d_mine <= 2 * d_torch
    assert list(tab.steps) == [STEPS, STEPS - 2, STEPS]                      # torch's per-parameter `step`
    assert [int(opt32.state[q]["step"]) for q in opt32.param_groups[0]["params"]] == [STEPS, STEPS - 2, STEPS]


def test_running_products_are_plain_multiplies():
    from pcrlv2_amd.optim import running_product
    tab = R.AdamTables(2)
    for _ in range(5):
        R.adam_prepare(tab, [1, 0], LR, *BETAS)
    x = 1.0
    for _ in range(5):
        x = x * 0.999
    assert tab.prods[0, 1] == x == running_product(0.999, 5) and tab.steps[1] == 0 and tab.prods[1, 0] == 1.0
    assert tab.coefs[0, 0] == F(LR / (1.0 - running_product(0.9, 5))) and tab.coefs[0, 1] == F(np.sqrt(1.0 - x))


def _clip_with_torch(parts, max_norm):
    ps = [torch.nn.Parameter(torch.zeros(len(g), dtype=torch.float64)) for g in parts]
    for p, g in zip(ps, parts):
        p.grad = torch.tensor(g, dtype=torch.float64)
    ps[0].grad[0] = 1.0                   # this element becomes the coefficient itself
    norm = torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False)
    return float(norm), float(ps[0].grad[0])


@pytest.mark.parametrize("max_norm", [1.0, 1e6])
def test_norm_restatement_against_clip_grad_norm(max_norm):
    """clip_grad_norm_'s total_norm and coefficient in float64, within 1e-14 relative: torch takes the norm of the per-tensor norms, a few
    roundings more than one sum.  On exactly summable gradients the restatement's norm is the square root of the exact sum."""
    sizes = [5, 1, 7, 64, 3, 130, 2, 1025]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    flags = [1, 1, 0, 1, 1, 0, 1, 1]
    for exact in (True, False):
        g = R.summable_grads(offs[-1], 3) if exact else np.random.default_rng(5).standard_normal(offs[-1]).astype(F)
        g[0] = 1.0
        counted = [g[offs[t]:offs[t + 1]] for t in range(len(sizes)) if flags[t]]
        norm_t, coef_t = _clip_with_torch(counted, max_norm)
        g[offs[2]:offs[3]] = 1e30          # tensors without a gradient do not count
        norm, coef = R.grad_norm(g, offs, flags, 1.0, max_norm)
        assert abs(norm - norm_t) <= 1e-14 * norm_t and abs(float(coef) - coef_t) <= 6e-8 * coef_t      # float32 rounding of the coefficient
        if exact:
            g[offs[2]:offs[3]] = 0
            g[offs[5]:offs[6]] = 0
            assert norm == np.sqrt(R.assert_summable(g))
        assert (coef == F(1.0)) == (max_norm > norm_t)


def test_norm_restatement_nonfinite_and_padding():
    offs, g = np.array([0, 4, 8]), np.array([1, 2, 2, 7, 3, 0, 0, 0], F)
    assert R.grad_norm(g, offs, [1, 1], 1.0, 1.0, numels=[3, 1])[0] == np.sqrt(18.0)        # the 7 lies in the first slot's padding
    g[0] = np.inf
    norm, coef = R.grad_norm(g, offs, [1, 1], 1.0, 1.0)
    assert np.isinf(norm) and coef == 0
    g[0] = np.nan
    norm, coef = R.grad_norm(g, offs, [1, 1], 1.0, 1.0)
    assert np.isnan(norm) and np.isnan(coef)


def test_exactly_summable_clip_inputs():
    """The precondition of the GPU norm tests, at their largest size (2^23 + 5 elements) and both gradient scales: every square is a multiple of
    2^-18 and the sum stays far below 2^53 * 2^-18, so any summation order gives the same float64.  For 2^20 elements: three orders, same bits."""
    g = R.summable_grads(2 ** 23 + 5, 9)
    assert np.abs(g).max() <= 4 and np.array_equal(g * 256, np.rint(g * 256))
    for gs in (1.0, 0.5):
        assert R.assert_summable(g, gs) < 2.0 ** 53 * 2.0 ** -18
    h = g[:2 ** 20]
    want = R.assert_summable(h, 0.5)
    sq = (h.astype(np.float64) * 0.5) ** 2
    seq = 0.0
    for chunk in np.sort(sq).reshape(1024, 1024):          # ascending, chunk by chunk, one running sum
        seq = seq + float(np.add.reduce(chunk))
    offs = np.array([0, len(h)])
    assert np.sum(sq) == want == seq == np.sum(sq[::-1])
    assert R.grad_norm(h, offs, [1], 0.5, 1.0)[0] == np.sqrt(want)


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------
NEW_ENTRY_POINTS = ("pcrl_optim_grid_cap", "pcrl_adam_prepare", "pcrl_adam_step", "pcrl_grad_norm", "pcrl_sgd_step_clipped")


def test_entry_points_declared_and_exported():
    protos = _lib.parse_header()
    cdll = ctypes.CDLL(_lib.LIBPATH)
    for name in NEW_ENTRY_POINTS:
        assert name in protos, name
        assert hasattr(cdll, name), name
    assert [t for t, _ in protos["pcrl_adam_prepare"][1]][:4] == ["const int32_t*", "int32_t*", "double*", "float*"]
    assert [n for _, n in protos["pcrl_adam_step"][1]][-2:] == ["clip_coef", "stream"]
    assert [n for _, n in protos["pcrl_sgd_step_clipped"][1]][:11] == [n for _, n in protos["pcrl_sgd_step"][1]][:11]
    assert cdll.pcrl_optim_grid_cap() == R.GRID_CAP


def test_optim_file_is_built_without_contraction():
    from pcrlv2_amd import build
    assert build.FILE_FLAGS["optim.hip"] == ["-ffp-contract=off"]
    assert os.path.exists(os.path.join(build.CSRC, "optim.hip"))


# ---- command lines ----------------------------------------------------------------------------------------------------------------
def _parsers():
    from pcrlv2_amd import luna_nodules, main, seg3d
    return {"main": (main.build_parser(), ["--d", "2", "--phase", "scratch", "--data", "synthetic"]),
            "nodules": (luna_nodules.build_parser(), ["train", "--data", "synthetic", "--phase", "scratch"]),
            "seg3d": (seg3d.build_parser(), ["train", "--data", "synthetic", "--phase", "scratch"])}


@pytest.mark.parametrize("which", ["main", "nodules", "seg3d"])
def test_command_lines_parse_the_optimiser_options(which):
    ap, base = _parsers()[which]
    a = ap.parse_args(base)
    assert (a.optimizer, a.betas, a.eps, a.clip_grad) == ("sgd", "0.9,0.999", 1e-8, 0.0)
    optim_cli.check(a)
    assert optim_cli.options(a) == {}                  # plain SGD: make_optimizer is called as it always was
    a = ap.parse_args(base + ["--optimizer", "adamw", "--betas", "0.8, 0.99", "--eps", "1e-6", "--clip_grad", "2.5", "--lr", "3e-4", "--weight_decay", "0.05"])
    optim_cli.check(a)
    assert optim_cli.options(a) == {"kind": "adamw", "betas": (0.8, 0.99), "eps": 1e-6, "max_grad_norm": 2.5}
    assert (a.lr, a.weight_decay) == (3e-4, 0.05)
    a = ap.parse_args(base + ["--clip_grad", "1"])
    assert optim_cli.options(a) == {"max_grad_norm": 1.0}
    for bad, text in ((["--optimizer", "lamb"], "sgd, adam or adamw"), (["--clip_grad", "-1"], "--clip_grad"), (["--eps", "-1"], "--eps")):
        with pytest.raises(SystemExit, match=text):
            optim_cli.check(ap.parse_args(base + bad))


def test_checks_run_in_front_of_the_loops():
    from pcrlv2_amd import luna_nodules, main, seg3d
    with pytest.raises(SystemExit, match="sgd, adam or adamw"):
        seg3d.check_train(seg3d.build_parser().parse_args(["train", "--data", "synthetic", "--phase", "scratch", "--optimizer", "rmsprop"]))
    with pytest.raises(SystemExit, match="sgd, adam or adamw"):
        luna_nodules.train(luna_nodules.build_parser().parse_args(["train", "--data", "synthetic", "--phase", "scratch", "--optimizer", "rmsprop"]))
    with pytest.raises(SystemExit, match="--betas"):
        main.check_route(main.build_parser().parse_args(["--d", "2", "--phase", "scratch", "--optimizer", "adam", "--betas", "0.9"]))
    main.check_route(main.build_parser().parse_args(["--d", "2", "--phase", "scratch", "--optimizer", "adam", "--clip_grad", "1"]))


@pytest.mark.parametrize("d", ["2", "3"])
def test_pretask_refuses_other_optimisers_and_clipping(d):
    from pcrlv2_amd import main
    ap = main.build_parser()
    main.check_route(ap.parse_args(["--d", d, "--phase", "pretask"]))
    for kind in ("adam", "adamw"):
        with pytest.raises(SystemExit, match="--phase pretask trains with the reference's SGD: --optimizer " + kind):
            main.check_route(ap.parse_args(["--d", d, "--phase", "pretask", "--optimizer", kind]))
    with pytest.raises(SystemExit, match="--phase pretask does not clip gradients"):
        main.check_route(ap.parse_args(["--d", d, "--phase", "pretask", "--clip_grad", "1.0"]))


def test_betas_parser_messages():
    assert optim_cli.parse_betas("0.9,0.999") == (0.9, 0.999)
    assert optim_cli.parse_betas(" 0 , 0.5 ") == (0.0, 0.5)
    for text, msg in (("0.9", "two numbers B1,B2"), ("0.9,0.99,0.999", "two numbers B1,B2"), ("a,b", "B1 and B2 are numbers"),
                      ("0.9,1.0", r"B2 = 1 is outside \[0, 1\)"), ("-0.1,0.9", r"B1 = -0.1 is outside \[0, 1\)"), ("nan,0.9", "B1 = nan is outside")):
        with pytest.raises(SystemExit, match=msg):
            optim_cli.parse_betas(text)


def test_state_kind_refusals():
    """A checkpoint's optimiser state of another kind ends the run with a message (no torch state is touched before it)."""
    from pcrlv2_amd import optim

    class _O:
        kind = "adamw"
    sgd = {"state": {0: {"momentum_buffer": None}}, "param_groups": [{"momentum": 0.9}]}
    adam = {"state": {0: {"exp_avg": None}}, "param_groups": [{"betas": (0.9, 0.999)}]}
    assert optim.state_kind(sgd) == "sgd" and optim.state_kind(adam) == "adam"
    assert optim.state_kind({"state": {}, "param_groups": [{"betas": (0.9, 0.999)}]}) == "adam"
    with pytest.raises(SystemExit, match="holds the state of optimizer 'sgd', but 'adamw' was asked for"):
        optim.require_state_kind(_O, sgd)
    optim.require_state_kind(_O, adam)                       # the state alone cannot tell adam from adamw ...
    with pytest.raises(SystemExit, match="holds the state of optimizer 'adam', but 'adamw' was asked for"):
        optim.require_state_kind(_O, adam, saved="adam")     # ... the checkpoint's own --optimizer can
    _O.kind = "sgd"
    with pytest.raises(SystemExit, match="holds the state of optimizer 'adam', but 'sgd' was asked for"):
        optim.require_state_kind(_O, adam)
    optim.require_state_kind(_O, sgd, saved="sgd")
