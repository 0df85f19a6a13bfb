"""pcrl_head_bwd_stage (csrc/heads_fused.hip) called directly, at the edges of its three roles: the four-wave split of the K range of role A
(empty and short quarters), the row lanes n = lane + 64 i up to RMAX rows per lane, the x-blocks of role B and its `c >= C` exit, the wave
walk of role C, the ReLU mask on +0.0 and -0.0, and the "add only" form.  ops.heads_backward keeps its own test (test_ops2d_gpu.py).

mean, rstd and gamma are INPUTS of the entry point, so they sit on a dyadic lattice next to the activations (heads_eval_cases.py); the
preconditions are asserted by test_heads_eval_cases_cpu.py.  Two kinds of bound, nothing measured:
  exact    dW, db, dbeta, dgamma always, and dx where N is a power of two: every float32 product and sum is exact in any order, s1 and s2 are
           exact float64 sums, both divisions by N are exact, so only the final cast to float32 rounds: the output equals the float32 rounding of
           the float64 restatement at EVERY element (assert_bit_equal)
  derived  dx for any other N: |dx - ref| <= 2 ulp_f32(|ref|) + 2^-50 |gamma rstd| (|t| + |dbeta| / N + |xh dgamma| / N) -- the two float64
           quotients by N are rounded before a subtraction that may cancel, then one float32 rounding follows (the restatement rounds the same
           quotients, so each side is within 2^-51 of the second term of the true value, and half a float32 ulp of its own rounding)
Every output lies between two runs of 64 words of a fixed bit pattern, which must survive every call.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import heads_eval_cases as hec  # noqa: E402
from exact_lattice import assert_bit_equal  # noqa: E402
from pcrlv2_amd._lib import PcrlError, lib, stream_handle  # noqa: E402

DEV = "cuda"
F32 = torch.float32
PAD = 64
PATTERN = 0x7FA5A5A5          # a NaN payload no computation produces


def guarded(n):
    full = torch.empty(n + 2 * PAD, dtype=torch.int32, device=DEV).fill_(PATTERN).view(F32)
    return full, full[PAD:PAD + n]


def guards_kept(full, n, what):
    bits = full.view(torch.int32)
    assert bool((bits[:PAD] == PATTERN).all()), f"{what}: the words in front of the output were written"
    assert bool((bits[PAD + n:] == PATTERN).all()), f"{what}: the words behind the output were written"


def run(x, N, K, C, with_dy, with_add, relu):
    """one call on guarded outputs -> dict of float32 CPU tensors (dW / db only with dy)"""
    d = {k: v.to(F32).to(DEV).contiguous() for k, v in x.items()}
    bufs = dict(dx=guarded(N * C), dgamma=guarded(C), dbeta=guarded(C))
    if with_dy:
        bufs.update(dW=guarded(K * C), db=guarded(K))
    out = {k: v[1] for k, v in bufs.items()}
    lib().call("pcrl_head_bwd_stage", d["dy"] if with_dy else None, d["W"] if with_dy else None, d["add"] if with_add else None,
               d["xin"] if with_dy else None, d["xbn"], d["ybn"] if relu else None, d["gamma"], d["mean"], d["rstd"], out["dx"], out["dgamma"], out["dbeta"],
               out.get("dW"), out.get("db"), N, K, C, relu, stream_handle())
    torch.cuda.synchronize()
    for k, (full, view) in bufs.items():
        guards_kept(full, view.numel(), f"{k} N={N} K={K} C={C}")
    shapes = dict(dx=(N, C), dgamma=(C,), dbeta=(C,), dW=(K, C), db=(K,))
    return {k: v.cpu().view(shapes[k]) for k, v in out.items()}


def compare(x, got, N, K, C, with_dy, with_add, relu, what):
    """-> worst error / bound of dx (0 where dx is compared bit for bit)"""
    args = (x["dy"] if with_dy else None, x["W"] if with_dy else None, x["add"] if with_add else None, x["xin"] if with_dy else None, x["xbn"], x["ybn"],
            x["gamma"], x["mean"], x["rstd"], relu)
    dx, dgamma, dbeta, dW, db = hec.head_bwd_stage_ref(*args)
    assert_bit_equal(got["dbeta"], dbeta + 0.0, F32, f"{what}: dbeta")
    assert_bit_equal(got["dgamma"], dgamma + 0.0, F32, f"{what}: dgamma")
    if with_dy:
        assert_bit_equal(got["dW"], dW + 0.0, F32, f"{what}: dW")          # + 0.0: a sum that starts at +0 never ends at -0
        assert_bit_equal(got["db"], db + 0.0, F32, f"{what}: db")
    if hec.is_pow2(N):
        assert_bit_equal(got["dx"], dx, F32, f"{what}: dx")
        return 0.0
    slack = hec.head_dx_slack(args[0], args[1], args[2], x["xbn"], x["ybn"], x["gamma"], x["mean"], x["rstd"], relu)
    bound = 2.0 * hec.ulp_f32(dx) + 2.0 ** -50 * slack
    err = (got["dx"].double() - dx).abs()
    ratio = float((err / bound).max())
    assert bool((err <= bound).all()), f"{what}: dx error / bound = {ratio:.3f} at {int((err / bound).argmax())}"
    return ratio


@pytest.mark.parametrize("case", hec.HEAD_CASES, ids=lambda c: f"N{c[0]}-K{c[1]}-C{c[2]}")
def test_full_form_against_the_float64_restatement(case):
    N, K, C, why = case
    x = hec.head_inputs(N, K, C, seed=1000 * N + 10 * K + C)
    worst = 0.0
    for with_add in (True, False):
        for relu in (0, 1):
            got = run(x, N, K, C, True, with_add, relu)
            worst = max(worst, compare(x, got, N, K, C, True, with_add, relu, f"N={N} K={K} C={C} add={with_add} relu={relu} ({why})"))
    print(f"[head_bwd_stage N={N} K={K} C={C}] dx " + ("bit for bit" if hec.is_pow2(N) else f"worst error / bound {worst:.3f}"))


@pytest.mark.parametrize("case", hec.HEAD_ADD_ONLY, ids=lambda c: f"N{c[0]}-C{c[1]}")
def test_add_only_form_against_the_float64_restatement(case):
    """dy = W = xin = dW = db = NULL; K is ignored (a value that the full form would reject is passed)"""
    N, C = case
    x = hec.head_inputs(N, 4, C, seed=77 * N + C)
    worst = 0.0
    for relu in (0, 1):
        got = run(x, N, 6, C, False, True, relu)
        worst = max(worst, compare(x, got, N, 4, C, False, True, relu, f"add only N={N} C={C} relu={relu}"))
    print(f"[head_bwd_stage add only N={N} C={C}] dx " + ("bit for bit" if hec.is_pow2(N) else f"worst error / bound {worst:.3f}"))


def test_the_mask_treats_both_zeros_as_not_positive():
    """ybn = +0.0 and -0.0 everywhere except one positive row: t survives in that row only, so dbeta is that row of add."""
    N, C = 65, 8
    x = hec.head_inputs(N, 4, C, seed=3)
    ybn = torch.zeros(N, C, dtype=torch.float64)
    ybn[::2] = -0.0
    ybn[7] = 0.5
    x["ybn"] = ybn
    got = run(x, N, 4, C, False, True, 1)
    assert torch.equal(got["dbeta"].double(), x["add"][7])
    compare(x, got, N, 4, C, False, True, 1, "zeros mask")


def test_two_runs_of_the_largest_case_are_bit_identical():
    N, K, C = hec.HEAD_LARGEST
    x = hec.head_inputs(N, K, C, seed=9)
    a, b = run(x, N, K, C, True, True, 1), run(x, N, K, C, True, True, 1)
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


def test_the_canary_cases_are_in_the_list():
    """run() checks the guard words of every output in every call; the cases the float4 stores of role B end inside a lane group are among them."""
    ran = {(K, C) for _, K, C, _ in hec.HEAD_CASES}
    assert {(4, 252), (20, 252), (4, 260), (20, 260)} <= ran


def test_rejections_launch_nothing():
    z = lambda *s: torch.zeros(*s, dtype=F32, device=DEV)
    R, Q = 520, 8                                              # every buffer holds 520 rows of 8: large enough for any size a call below names
    dy, W, add, xin, xbn, ybn = z(R, Q), z(Q, Q), z(R, Q), z(R, Q), z(R, Q), z(R, Q)
    gamma, mean, rstd = z(Q), z(Q), z(Q)
    dx, dgamma, dbeta, dW, db = z(R, Q), z(Q), z(Q), z(Q, Q), z(Q)
    sent = dict(dx=dx, dgamma=dgamma, dbeta=dbeta, dW=dW, db=db)
    for t in sent.values():
        t.fill_(-7.0)

    def call(N=4, K=4, C=4, relu=0, **kw):
        a = dict(dy=dy, W=W, add=add, xin=xin, xbn=xbn, ybn=ybn, gamma=gamma, mean=mean, rstd=rstd, dx=dx, dgamma=dgamma, dbeta=dbeta, dW=dW, db=db)
        a.update(kw)
        lib().call("pcrl_head_bwd_stage", *(a[k] for k in ("dy", "W", "add", "xin", "xbn", "ybn", "gamma", "mean", "rstd", "dx", "dgamma", "dbeta", "dW", "db")),
                   N, K, C, relu, stream_handle())

    rows = r"N=%d \(2\.\.512 rows\) C=%d \(a multiple of 4\)"
    with pytest.raises(PcrlError, match=rows % (1, 4)):
        call(N=1)
    with pytest.raises(PcrlError, match=rows % (513, 4)):
        call(N=513)
    with pytest.raises(PcrlError, match=rows % (4, 6)):
        call(C=6)
    with pytest.raises(PcrlError, match=r"the Linear part needs W, xin, dW, db and K % 4 == 0 \(K=6\)"):
        call(K=6)
    with pytest.raises(PcrlError, match="the ReLU mask needs the normalisation's output"):
        call(relu=1, ybn=None)
    with pytest.raises(PcrlError, match=r"the Linear part needs W, xin, dW, db and K % 4 == 0 \(K=4\)"):
        call(dW=None)
    with pytest.raises(PcrlError, match="head_bwd_stage: null pointer"):
        call(dy=None, add=None)
    off = z(R * Q + 4)[1:1 + R * Q].view(R, Q)
    assert off.data_ptr() % 16 == 4
    with pytest.raises(PcrlError, match="dy, xin and dW must be 16-byte aligned"):
        call(dy=off)
    torch.cuda.synchronize()
    for k, t in sent.items():
        assert bool((t == -7.0).all()), f"{k} was written by a rejected call"
    call()                                                      # the same buffers are accepted once the sizes are legal (N = 4 zero rows)
    torch.cuda.synchronize()
    assert bool((dW.flatten()[:16] == 0).all()) and bool((dW.flatten()[16:] == -7.0).all()) and bool((db[:4] == 0).all()) and bool((db[4:] == -7.0).all())
