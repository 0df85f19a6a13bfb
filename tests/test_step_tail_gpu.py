"""The latency-bound tail of the training step (csrc/heads_loss.hip, pcrl_add_f32 in csrc/heads2d.hip) at the sizes where its kernels change
path: past one block, one reduction chunk, one wave pass, one grid-stride step; unaligned operands; degenerate rows; the rejections.

Every test names the constant in the source and the shape that crosses it.  References are float64 CPU computations on the float32-rounded
inputs.  Three kinds of bound, nothing else:
  exact    data movement and float32 additions in a stated order: bit patterns compared through .view(torch.int32)
  derived  the derivation is in the test's docstring
  project  tests/test_ops_gpu.py: 2e-5 * max|ref| (check default); BatchNorm1d 1e-5 forward / statistics, 2e-4 dx, 1e-4 dgamma, dbeta;
           2e-6 for the Linear products and SGD
Where a shape is ill-conditioned in float32 itself (a cancellation the formula has, whatever evaluates it), the bound is the larger of the
project tolerance and 4 x the error of a plain float32 CPU evaluation of the same formula against the same float64 reference (`yard=`); the
measured yardstick is written next to the case.

grid_for() in heads_loss.hip caps a launch at 8192 blocks x 256 threads = 2 097 152 work items (8 388 608 floats for the kernels that work on
groups of four); "past the cap" = the cap plus a remainder that is no multiple of 256.
"""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from pcrlv2_oracle import cosine_similarity  # noqa: E402
from pcrlv2_amd import functions, ops  # noqa: E402
from pcrlv2_amd._lib import PcrlError, lib, stream_handle  # noqa: E402

DEV = "cuda"
F32 = torch.float32
CAP_ITEMS = 8192 * 256            # grid_for(): work items of one grid-stride pass
CAP4 = 4 * CAP_ITEMS              # the same in floats for kernels that take four per work item
U = 2.0 ** -24                    # float32 unit roundoff


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * scale


def rnd32(n, seed):
    """large inputs: float32 uniform(-1, 1) straight away"""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, generator=g, dtype=F32) * 2 - 1


def back(t):
    torch.cuda.synchronize()
    return t.detach().double().cpu().contiguous()


def check(got, ref, what, tol=2e-5, yard=None):
    """max|got - ref| <= tol * max|ref| (the convention of tests/test_ops_gpu.py).  yard: a float32 CPU evaluation of the same formula; the
    bound becomes max(that, 4 x its own error against ref)."""
    got = back(got) if got.is_cuda else got.double()
    ref = ref.detach().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = max(ref.abs().max().item(), 1e-6)
    bound, y_err = tol * scale, None
    if yard is not None:
        y_err = (yard.detach().double() - ref).abs().max().item()
        bound = max(bound, 4 * y_err)
    err = (got - ref).abs().max().item()
    print(f"  {what}: max|d|={err:.3e} bound={bound:.3e} (project {tol * scale:.3e}" + (f", float32 yardstick {y_err:.3e})" if yard is not None else ")"))
    assert err <= bound, f"{what}: max|d|={err:.3e} > {bound:.3e} (ref max {scale:.3e})"
    return err


def same_bits(got, ref, what):
    """bit-for-bit: float32 device tensor against a float32 CPU tensor"""
    torch.cuda.synchronize()
    got, ref = got.detach().cpu().contiguous(), ref.detach().contiguous()
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    it = torch.int32 if got.element_size() == 4 else torch.int16
    bad = (got.view(it) != ref.view(it)).flatten().nonzero()
    assert bad.numel() == 0, f"{what}: {bad.numel()} elements differ, first at flat index {bad[0].item()}"


def dev(t):
    return t.to(F32).to(DEV).contiguous()


def off4(t):
    """a contiguous device copy of the float32 tensor t that starts 4 bytes into its buffer (not 16-byte aligned)"""
    buf = torch.empty(t.numel() + 1, dtype=F32, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t.to(F32))
    assert v.data_ptr() % 16 == 4
    return v


# ----------------------------------------------------------------------------------------------------------------------------------------
# 1. pcrl_grad_sum
# ----------------------------------------------------------------------------------------------------------------------------------------
SENT = -777.25
SIZES = [1, 1, 2, 3, 4, 5, 7, 8, 64, 130, 864]
PATTERNS = ("all", "first", "last", "mid", "none")


class Arena:
    """A gradient arena laid out like FusedSGD's: slots rounded up to 4 floats; offsets / numels on the device, offsets on the host as well."""

    def __init__(self, sizes):
        self.sizes = list(sizes)
        offs = [0]
        for n in sizes:
            offs.append(offs[-1] + (n + 3) // 4 * 4)
        self.offs, self.total = offs, offs[-1]
        self.dst = torch.full((self.total,), SENT, dtype=F32, device=DEV)
        self.offsets = torch.tensor(offs, dtype=torch.int64, device=DEV)
        self.numels = torch.tensor(self.sizes, dtype=torch.int64, device=DEV)
        self.offsets_c = (ctypes.c_int64 * len(offs))(*offs)
        self.expect = torch.full((self.total,), SENT, dtype=F32)

    def run(self, srcs, nsrc, t0=0):
        """srcs[i][k]: (cpu float32, device float32) of source k of tensor t0 + i, or None.  Launches, and records what must come out:
        ((s0 + s1) + ...) over the non-null sources in order, in float32; everything else keeps the sentinel."""
        arr = (ctypes.c_void_p * (len(srcs) * nsrc))()
        for i, row in enumerate(srcs):
            assert len(row) == nsrc
            acc = None
            for k, s in enumerate(row):
                if s is None:
                    continue
                arr[i * nsrc + k] = s[1].data_ptr()
                acc = s[0].clone() if acc is None else acc + s[0]
            if acc is not None:
                o = self.offs[t0 + i]
                self.expect[o:o + self.sizes[t0 + i]] = acc
        lib().call("pcrl_grad_sum", self.dst, self.offsets, self.numels, ctypes.addressof(self.offsets_c), ctypes.addressof(arr), t0, len(srcs), nsrc,
                   stream_handle())

    def verify(self, what):
        same_bits(self.dst, self.expect, what)


class Pool:
    """Random float32 sources carved out of ONE host buffer and its ONE device copy (one upload per test instead of one per source); every
    piece starts on a 16-byte boundary unless asked to start 4 bytes past one."""

    def __init__(self, nfloats, seed):
        self.cpu = rnd32(nfloats, seed)
        self.gpu = self.cpu.to(DEV)
        assert self.gpu.data_ptr() % 16 == 0
        self.at = 0

    def take(self, n, unaligned=False):
        o = (self.at + 3) // 4 * 4 + (1 if unaligned else 0)
        self.at = o + n
        assert self.at <= self.cpu.numel()
        d = self.gpu[o:o + n]
        assert d.data_ptr() % 16 == (4 if unaligned else 0)
        return self.cpu[o:o + n], d


def present(pattern, nsrc):
    if pattern == "all":
        return [True] * nsrc
    if pattern == "first":
        return [k == 0 for k in range(nsrc)]
    if pattern == "last":
        return [k == nsrc - 1 for k in range(nsrc)]
    if pattern == "mid":          # a null source between two present ones (needs three)
        return [not (nsrc >= 3 and k == nsrc // 2) for k in range(nsrc)]
    return [False] * nsrc


@pytest.mark.parametrize("nsrc", [1, 2, 3, 4, 5, 6, 7, 8])
def test_grad_sum_source_patterns(nsrc):
    """pcrl_grad_sum, exact.  Tensor sizes 1 .. 864 cross the kernel's `e + 4 <= n` test (a ragged last group of a slot takes the scalar loop,
    full groups the float4 one) and `e >= n` (nothing to do in a slot's padding).  Per tensor the sources are all present / only the first /
    only the last / a null between two others / all null (the pattern rotates over the tensors in five rounds, so every size meets every
    pattern): the sum is ((s0 + s1) + ...) over the non-null ones in order, a tensor without sources and every padding float keep the sentinel
    the arena was filled with."""
    for shift in range(len(PATTERNS)):
        ar, pool = Arena(SIZES), Pool(1 << 14, seed=10 * nsrc + shift)
        srcs = []
        for t, n in enumerate(SIZES):
            pr = present(PATTERNS[(t + shift) % len(PATTERNS)], nsrc)
            srcs.append([pool.take(n) if p else None for p in pr])
        ar.run(srcs, nsrc)
        ar.verify(f"grad_sum nsrc={nsrc} shift={shift}")


@pytest.mark.parametrize("which", ["every source of a tensor", "one source of a tensor", "the source of a 1-element tensor"])
def test_grad_sum_unaligned_sources(which):
    """pcrl_grad_sum, exact: a source that starts 4 bytes past a 16-byte boundary (a slice of a (gamma, beta) pair).  The kernel's
    `vec = vec && (pointer & 15) == 0` sends the WHOLE tensor down the scalar loop as soon as one of its sources is unaligned; its aligned
    neighbours stay on the float4 path."""
    nsrc = 3
    ar, pool = Arena(SIZES), Pool(1 << 14, seed=77)
    srcs = []
    for t, n in enumerate(SIZES):
        if which == "every source of a tensor":
            un = [n in (130, 864, 8)] * nsrc
        elif which == "one source of a tensor":
            un = [n in (64, 864, 5) and k == 1 for k in range(nsrc)]
        else:
            un = [n == 1 and k == 0 for k in range(nsrc)]
        srcs.append([pool.take(n, unaligned=u) for u in un])
    ar.run(srcs, nsrc)
    ar.verify(f"grad_sum, unaligned: {which}")


def test_grad_sum_sub_range_leaves_its_neighbours_alone():
    """pcrl_grad_sum, exact: t0 = 3, cnt = 5 -- the kernel's index space starts at offsets[t0] and its table search at t0; tensors 0 .. 2 and
    8 .. 10 (and all padding) keep the sentinel."""
    ar, pool = Arena(SIZES), Pool(1 << 14, seed=5)
    ar.run([[pool.take(n), None, pool.take(n)] for n in SIZES[3:8]], 3, t0=3)
    ar.verify("grad_sum t0=3 cnt=5")
    o3, o8 = ar.offs[3], ar.offs[8]
    torch.cuda.synchronize()
    assert bool((ar.dst[:o3] == SENT).all()) and bool((ar.dst[o8:] == SENT).all())


@pytest.mark.parametrize("ntens,nsrc,null_chunk", [(130, 8, None), (130, 8, 1), (70, 7, None), (70, 7, 0)])
def test_grad_sum_launch_split(ntens, nsrc, null_chunk):
    """pcrl_grad_sum, exact: the source pointers travel as kernel arguments, GS_MAX = 480 per launch, so a call is split after 480 / nsrc
    tensors: 130 tensors with 8 sources = launches of 60, 60, 10; 70 tensors with 7 sources = launches of 68 and 2.  With `null_chunk` the
    tensors of that whole launch have no source at all (the launcher skips it: `if (!any) continue`) and the launch after it must still take
    its own pointers and offsets."""
    per = 480 // nsrc
    sizes = [SIZES[t % len(SIZES)] for t in range(ntens)]
    ar, pool = Arena(sizes), Pool(1 << 18, seed=ntens + nsrc)
    srcs = []
    for t, n in enumerate(sizes):
        if null_chunk is not None and t // per == null_chunk:
            srcs.append([None] * nsrc)
        else:
            pr = present(PATTERNS[t % 4], nsrc)        # no all-null tensors outside the null chunk
            srcs.append([pool.take(n) if p else None for p in pr])
    ar.run(srcs, nsrc)
    ar.verify(f"grad_sum {ntens} tensors x {nsrc} sources")
    if null_chunk is not None:
        lo, hi = ar.offs[null_chunk * per], ar.offs[min(ntens, (null_chunk + 1) * per)]
        assert bool((ar.dst[lo:hi] == SENT).all())


def test_grad_sum_past_the_grid_stride_cap():
    """pcrl_grad_sum, exact: one tensor of 8 388 608 + 1028 floats = 2 097 152 + 257 groups of four, more than grid_for()'s 8192 x 256 work
    items, so threads take a second grid-stride step (`q += gridDim.x * 256`); three small tensors follow it in the same launch."""
    sizes = [CAP4 + 1028, 5, 1, 64]
    ar = Arena(sizes)
    big = [rnd32(sizes[0], seed=s) for s in (1, 2)]
    pool = Pool(1 << 10, seed=3)
    srcs = [[(b, b.to(DEV)) for b in big]] + [[pool.take(n), pool.take(n)] for n in sizes[1:]]
    ar.run(srcs, 2)
    ar.verify("grad_sum past the cap")


def test_grad_sum_rejections():
    """pcrl_grad_sum refuses nsrc = 0, nsrc = 9 (the ABI takes 1 .. 8) and a source pointer that is not 4-byte aligned."""
    ar, pool = Arena([8, 8]), Pool(64, seed=1)
    a, b = pool.take(8)[1], pool.take(8)[1]
    L, s = lib(), stream_handle()

    def call(ptrs, nsrc):
        arr = (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)
        L.call("pcrl_grad_sum", ar.dst, ar.offsets, ar.numels, ctypes.addressof(ar.offsets_c), ctypes.addressof(arr), 0, 2, nsrc, s)

    with pytest.raises(PcrlError):
        call([a.data_ptr(), b.data_ptr()], 0)
    with pytest.raises(PcrlError):
        call([a.data_ptr()] * 18, 9)
    with pytest.raises(PcrlError):
        call([a.data_ptr() + 2, b.data_ptr()], 1)
    torch.cuda.synchronize()
    assert bool((ar.dst == SENT).all())


# ----------------------------------------------------------------------------------------------------------------------------------------
# 2. pcrl_concat / ops.concat_batch
# ----------------------------------------------------------------------------------------------------------------------------------------
CAT_BYTES = [16, 48, 4096 + 16, 32, 1600, 16, 256, 4096 + 16]


def concat_abi(pieces, out, nbytes=None, n=None):
    n = len(pieces) if n is None else n
    m = max(len(pieces), 1)
    src = (ctypes.c_void_p * m)(*[p if isinstance(p, int) else p.data_ptr() for p in pieces])
    nb = (ctypes.c_int64 * m)(*(nbytes if nbytes is not None else [p.numel() * p.element_size() for p in pieces]))
    lib().call("pcrl_concat", ctypes.addressof(src), ctypes.addressof(nb), n, out, stream_handle())


@pytest.mark.parametrize("order", ["as listed", "reversed"])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8])
def test_concat_unequal_pieces(n, order):
    """pcrl_concat, exact against torch.cat: 1 .. 8 pieces of unequal byte counts -- a 16-byte piece (ONE vector: `i >= vec_end[q]` moves on
    after a single element), 48 bytes, 4 KiB + 16 (one vector past a block of 256) -- through the kernel's 7-step piece search
    (`q + 1 < c.n`: unused table entries must not be looked at).  Four floats behind the destination keep their sentinel."""
    sizes = (CAT_BYTES if order == "as listed" else CAT_BYTES[::-1])[:n]
    cpu = [rnd32(b // 4, seed=100 + k) for k, b in enumerate(sizes)]
    pieces = [t.to(DEV) for t in cpu]
    total = sum(sizes) // 4
    out = torch.full((total + 4,), SENT, dtype=F32, device=DEV)
    concat_abi(pieces, out)
    same_bits(out, torch.cat(cpu + [torch.full((4,), SENT, dtype=F32)]), f"concat of {sizes} bytes")


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", [6, 8])
def test_concat_batch_equal_pieces(n, dt):
    """ops.concat_batch, exact against torch.cat: the models' call (six equal pieces, train_3d.py:121) and the ABI's maximum of eight, in
    both activation types; one pcrl_concat launch each."""
    cpu = [rnd(2, 3, 8, seed=k).to(dt) for k in range(n)]
    with lib().count_calls("pcrl_concat") as calls:
        out = ops.concat_batch([t.to(DEV) for t in cpu])
    assert calls.get("pcrl_concat") == 1
    same_bits(out, torch.cat(cpu), f"concat_batch {n} x {dt}")


@pytest.mark.parametrize("why", ["bytes not a multiple of 16", "pointer not 16-byte aligned"])
def test_concat_batch_falls_back_for_what_the_kernel_refuses(why):
    """ops.concat_batch hands what pcrl_concat does not take (60-byte pieces; pieces that start 4 bytes past a 16-byte boundary) to torch.cat:
    same result, no pcrl_concat launch."""
    if why == "bytes not a multiple of 16":
        cpu = [rnd(3, 5, seed=k).float() for k in range(6)]
        pieces = [t.to(DEV) for t in cpu]
    else:
        cpu = [rnd(2, 3, 8, seed=k).float() for k in range(6)]
        pieces = [t.to(DEV) for t in cpu[:3]] + [off4(t) for t in cpu[3:]]
    with lib().count_calls("pcrl_concat") as calls:
        out = ops.concat_batch(pieces)
    assert not calls
    same_bits(out, torch.cat(cpu), f"concat_batch fallback ({why})")


def test_concat_past_the_grid_stride_cap():
    """pcrl_concat, exact: eight pieces of 4 194 816 bytes = 2 097 408 vectors of 16 bytes, 256 more than grid_for()'s 8192 x 256 work items,
    so the first block's threads take a second grid-stride step, inside the LAST piece.  The pieces are rows of one buffer taken in
    reverse order (a kernel that ignored the piece table would copy them in the buffer's order)."""
    per = 4194816 // 4
    cpu = rnd32(8 * per, seed=9).view(8, per)
    buf = cpu.to(DEV)
    out = ops.concat_batch([buf[k] for k in range(7, -1, -1)])
    assert out.numel() * 4 // 16 == CAP_ITEMS + 256
    same_bits(out, cpu.flip(0).reshape(-1), "concat past the cap")


def test_concat_rejections():
    """pcrl_concat refuses 0 and 9 pieces, a byte count that is no multiple of 16, and a source or destination that is not 16-byte aligned."""
    a = torch.zeros(16, dtype=F32, device=DEV)
    out = torch.full((64,), SENT, dtype=F32, device=DEV)
    for pieces, kw in (([a], dict(n=0)), ([a] * 9, dict()), ([a], dict(nbytes=[24])), ([a[1:5]], dict())):
        with pytest.raises(PcrlError):
            concat_abi(pieces, out, **kw)
    with pytest.raises(PcrlError):
        concat_abi([a], out[1:])
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


# ----------------------------------------------------------------------------------------------------------------------------------------
# 3. MSE
# ----------------------------------------------------------------------------------------------------------------------------------------
MSE_N = [1, 255, 4095, 4096, 4097, 4096 * 256 + 1, CAP_ITEMS + 300]
_mse_cache = {}


def mse_inputs(n):
    """random p, gt with a difference of 1000 planted at the last element and at the first element of the last RED_CHUNK: dropping either
    moves the loss by far more than any bound below.  Built once per n, shared by forward and backward, never modified."""
    if n not in _mse_cache:
        _mse_cache.clear()           # one size at a time: the largest is 2 x 8 MB on either side
        p, gt = rnd32(n, seed=n % 1000 + 1), rnd32(n, seed=n % 1000 + 2)
        for i in {n - 1, (n - 1) // 4096 * 4096}:
            p[i] = gt[i] + 1000.0
        _mse_cache[n] = (p, gt, p.to(DEV), gt.to(DEV))
    return _mse_cache[n]


@pytest.mark.parametrize("n", MSE_N)
def test_mse_forward_chunks(n):
    """pcrl_mse_fwd.  RED_CHUNK = 4096 elements per first-stage block: n = 4095 / 4096 / 4097 sit on either side of one chunk (4097: a last
    chunk of ONE element), 4096 * 256 + 1 gives 257 partials, so mse_finish_kernel's loop `i += 256` runs twice for thread 0, and
    2 097 152 + 300 gives 513 blocks with a ragged last chunk of 300.
    Derived bound, relative 4 * 2^-24 against float64 on the same float32 inputs: d = p - gt is rounded once and squared (2 u), the square is
    rounded once (u), all terms are non-negative and accumulated in double, the mean is rounded to float32 once (u)."""
    p, gt, pd, gd = mse_inputs(n)
    ref = ((p.double() - gt.double()) ** 2).mean().item()
    got = ops.mse_forward(pd, gd).double().item()
    rel = abs(got - ref) / ref
    print(f"  mse fwd n={n}: rel err {rel:.3e} (bound {4 * U:.3e})")
    assert rel <= 4 * U, (n, got, ref, rel)


@pytest.mark.parametrize("n", MSE_N)
def test_mse_backward_grid_stride(n):
    """pcrl_mse_bwd: dp = g * (p - gt), g = dloss * (float)(2 / n).  n = 2 097 152 + 300 is past grid_for()'s cap: 300 threads take a second
    grid-stride step.  Derived bound per element, relative 4 * 2^-24 (+ 1e-12 absolute) against float64 dloss * (2 / n) * (p - gt) on the same
    inputs: one rounding each for (float)(2 / n), g, the difference and the product."""
    p, gt, pd, gd = mse_inputs(n)
    dl = torch.tensor(0.7, dtype=F32)
    ref = dl.double() * (2.0 / n) * (p.double() - gt.double())
    got = back(ops.mse_backward(pd, gd, dl.to(DEV)))
    excess = ((got - ref).abs() - (4 * U * ref.abs() + 1e-12)).max().item()
    print(f"  mse bwd n={n}: max rel err {((got - ref).abs() / ref.abs().clamp_min(1e-30)).max().item():.3e} (bound {4 * U:.3e})")
    assert excess <= 0, (n, excess)


# ----------------------------------------------------------------------------------------------------------------------------------------
# 4. cosine
# ----------------------------------------------------------------------------------------------------------------------------------------
def cos_grad_f32(x, y, g, eps=1e-8):
    """The float32 yardstick: cosine_bwd_kernel's formula, operation by operation, in float32 on the CPU: g * (y / (nx' ny') - (x.y) x / (nx'^3 ny')),
    the second term only where |x| > eps."""
    x, y = x.float(), y.float()
    dot, nx, ny = (x * y).sum(1, keepdim=True), (x * x).sum(1, keepdim=True).sqrt(), (y * y).sum(1, keepdim=True).sqrt()
    nxc, nyc = nx.clamp_min(eps), ny.clamp_min(eps)
    v = y / (nxc * nyc)
    v = torch.where(nx > eps, v - dot * x / (nxc * nxc * nxc * nyc), v)
    return torch.as_tensor(g, dtype=F32) * v


def degenerate_rows(x, y):
    """row 0: x all zero; row 1: |x| = 5e-9 < eps; row 2: |y| = 5e-9 < eps (float64 in, float32-rounded float64 out)"""
    x, y = x.clone(), y.clone()
    x[0] = 0.0
    x[1] *= 5e-9 / x[1].norm()
    y[2] *= 5e-9 / y[2].norm()
    return x.float().double(), y.float().double()


def check_rows(got, ref, what, tol=2e-5):
    """per row, relative to that row's own max|ref| (the gradients of the clamped rows are ~1e8 times the others)"""
    got, ref = back(got), ref.double()
    scale = ref.abs().amax(dim=1).clamp_min(1e-30)
    rel = ((got - ref).abs().amax(dim=1) / scale)
    print(f"  {what}: per-row max|d| / max|ref| = {[f'{v:.1e}' for v in rel.tolist()]}")
    assert bool((rel <= tol).all()), (what, rel.tolist())


@pytest.mark.parametrize("C", [1, 5, 64, 65, 512])
@pytest.mark.parametrize("rows", [1, 3, 17, 64, 192])
def test_cosine_mean_rows_and_widths(rows, C):
    """pcrl_cosine_mean_fwd / _bwd against float64 autograd of the oracle's cosine_similarity(x, y).mean(), dout = -0.5.  The forward is ONE
    block of 4 waves, a wave per row at a time (`r += 4`): rows 1 and 3 leave waves without a row, 17 and 192 are ragged / many passes; lanes
    stride over the channels (`c += 64`): C = 1 and 5 leave lanes idle, 65 is one element into a second pass, 512 is eight passes.  The
    backward is one thread per element (rows * C up to 98 304 = 384 blocks).
    Project tolerance 2e-5 * max|ref|.  C = 1 is the exception: the gradient is y/(|x||y|) - (xy) x/(|x|^3 |y|) = 0 exactly, what is left in
    float32 is the rounding of two equal terms of size 1/|x| (float32 yardstick measured on the CPU for these inputs: 7e-9 .. 1.6e-7, where
    the float64 reference is 0 and the project bound 2e-11), so the bound there is 4 x the yardstick."""
    x, y = rnd(rows, C, seed=3).float().double().requires_grad_(True), rnd(rows, C, seed=4).float().double()
    c = cosine_similarity(x, y).mean()
    c.backward(torch.tensor(-0.5, dtype=torch.float64))
    xd, yd = dev(x.detach()), dev(y)
    out, saved = ops.cosine_mean_forward(xd, yd)
    check(out.view(1), c.detach().view(1), f"cosine_mean fwd rows={rows} C={C}")
    dx = ops.cosine_mean_backward(xd, yd, saved, torch.tensor(-0.5, device=DEV))
    check(dx, x.grad, f"cosine_mean bwd rows={rows} C={C}", yard=cos_grad_f32(x.detach(), y, -0.5 / rows) if C == 1 else None)


@pytest.mark.parametrize("C", [5, 64])
def test_cosine_mean_degenerate_rows(C):
    """pcrl_cosine_mean_*: an all-zero x row, an x row of norm 5e-9 and a y row of norm 5e-9 (eps = 1e-8), next to two ordinary rows; compared
    per row, relative to the row's own max|ref|, at the project tolerance.  The reference is the oracle's definition
    x.y / (max(|x|, eps) max(|y|, eps)), which the kernels implement: where a clamp is active it is a constant, so a clamped x row gets
    y / (eps |y|) and no projection term (`if (nx > eps)` in cosine_bwd_kernel).  The installed ATen differs from this for 0 < |x| <= eps: it
    applies the clamp under no-grad and differentiates through the norm (measured on the CPU with torch 2.10: about 2 % on such a row;
    identical on an all-zero row and on ordinary rows).  The oracle's definition is the pinned one."""
    x, y = degenerate_rows(rnd(5, C, seed=5), rnd(5, C, seed=6))
    x.requires_grad_(True)
    c = cosine_similarity(x, y).mean()
    c.backward(torch.tensor(-0.5, dtype=torch.float64))
    xd, yd = dev(x.detach()), dev(y)
    out, saved = ops.cosine_mean_forward(xd, yd)
    check(out.view(1), c.detach().view(1), f"cosine_mean fwd, degenerate rows, C={C}")
    check_rows(ops.cosine_mean_backward(xd, yd, saved, torch.tensor(-0.5, device=DEV)), x.grad, f"cosine_mean bwd, degenerate rows, C={C}")


def terms_reference(spec, rows, ngroups, tensors, dout):
    ts = [t.clone().requires_grad_(True) for t in tensors]
    out = [torch.zeros((), dtype=torch.float64) for _ in range(ngroups)]
    for xi, xr, yi, yr, w, g in spec:
        out[g] = out[g] + w * cosine_similarity(ts[xi][xr:xr + rows], ts[yi][yr:yr + rows].detach()).mean()
    out = torch.stack(out)
    (out * dout).sum().backward()
    return out.detach(), [t.grad for t in ts]


def terms_device(spec, rows, ngroups, tensors, dout):
    ts = [dev(t).requires_grad_(True) for t in tensors]
    out = functions.cosine_terms(spec, rows, ngroups, ts)
    out.backward(dev(dout))
    return out.detach(), [t.grad for t in ts]


def _terms_cases():
    W = [-0.5, 0.25, 1.5, -0.125, 0.75, -2.0, 0.375, 1.0]          # exact in float32; negative and fractional
    cases = {}
    # ONE term, rows = 3: a backward block of 4 rows with one row idle
    cases["one term"] = (3, 1, [(3, 5), (3, 5)], [(0, 0, 1, 0, -0.5, 0)])
    # COS_MAX_TERMS = 32 terms over four x tensors (eight terms share each gradient buffer: `first` = 0 for seven of them, accumulated in
    # term order); rows = 17 > the forward block's 16 waves (`r += nw` runs twice for wave 0)
    cases["32 terms, 2 groups"] = (17, 2, [(17, 64)] * 8, [(k % 4, 0, 4 + (3 * k) % 4, 0, W[k % 8] * (1 + k // 8), k % 2) for k in range(32)])
    # 8 groups (the ABI's maximum), widths 5 / 64 / 576 / 1030 in ONE call, rows = 40 (three passes of the forward's 16 waves); 576 and 1030 run
    # the backward's `cb += 512` loop two and three times; tensor 1 is x of one term and y of three
    spec = [(2 * (k % 4), 0, 2 * (k % 4) + 1, 0, W[k % 8], k % 8) for k in range(12)] + [(1, 0, 0, 0, 0.75, 3)]
    cases["8 groups, widths 5..1030"] = (40, 8, [(40, 5), (40, 5), (40, 64), (40, 64), (40, 576), (40, 576), (40, 1030), (40, 1030)], spec)
    # row blocks of taller tensors (the local views): tensor 0 has three blocks of 17 rows, block 1 is written by no term and must come back
    # zero, block 0 by two terms; tensor 2 has both of its blocks written (no zero fill)
    spec = [(0, 0, 1, 17, -0.5, 0), (0, 34, 1, 0, 0.25, 1), (0, 0, 1, 34, 1.5, 1), (2, 0, 3, 0, -0.125, 0), (2, 17, 3, 0, 0.5, 1)]
    cases["row blocks"] = (17, 2, [(51, 576), (51, 576), (34, 5), (17, 5)], spec)
    # C = 1030 with rows = 3: three `cb` passes, the last of 6 channels, in a block with an idle row
    cases["C=1030, rows=3"] = (3, 1, [(3, 1030), (3, 1030), (3, 1030)], [(0, 0, 1, 0, 1.5, 0), (0, 0, 2, 0, -0.5, 0)])
    return cases


TERMS_CASES = _terms_cases()


@pytest.mark.parametrize("name", list(TERMS_CASES))
def test_cosine_terms_against_float64(name):
    """functions.cosine_terms (pcrl_cosine_terms_fwd / _bwd) against float64 autograd of sum_t w_t * cosine_similarity(x_t, y_t.detach()).mean()
    per group, project tolerance 2e-5 * max|ref| on the group vector and on every gradient tensor.  What each case reaches is written next to
    it in _terms_cases(): 1 and COS_MAX_TERMS = 32 terms; 1, 2 and 8 groups; terms that share an x (first = 0, term-order accumulation);
    row blocks with an unwritten block that must read zero; rows 3 / 17 / 40 against the forward's 16 waves and the backward's 4-row blocks;
    C = 5 / 64 / 576 / 1030 against the backward's 512-channel `cb` loop.  Tensors that are no term's x get no gradient."""
    rows, ngroups, shapes, spec = TERMS_CASES[name]
    tensors = [rnd(*s, seed=20 + i).float().double() for i, s in enumerate(shapes)]
    dout = (rnd(ngroups, seed=7) + 1.5).float().double()
    out_ref, g_ref = terms_reference(spec, rows, ngroups, tensors, dout)
    out, g = terms_device(spec, rows, ngroups, tensors, dout)
    check(out, out_ref, f"cosine_terms fwd ({name})")
    xs = {s[0] for s in spec}
    for i, (a, b) in enumerate(zip(g, g_ref)):
        if i not in xs:
            assert a is None and b is None, (name, i)
            continue
        check(a, b, f"cosine_terms d tensor {i} ({name})")
    if name == "row blocks":
        torch.cuda.synchronize()
        assert bool((g[0][17:34] == 0).all()), "the row block no term writes must be zero"


def test_cosine_terms_degenerate_rows():
    """functions.cosine_terms on the degenerate rows of test_cosine_mean_degenerate_rows (all-zero x, |x| = 5e-9, |y| = 5e-9; same reference,
    same note on ATen), two terms sharing the x so that the clamped rows also pass through the accumulation; per row at the project
    tolerance."""
    x, y = degenerate_rows(rnd(5, 64, seed=5), rnd(5, 64, seed=6))
    y2 = rnd(5, 64, seed=8).float().double()
    spec = [(0, 0, 1, 0, 1.0, 0), (0, 0, 2, 0, -0.5, 0)]
    dout = torch.tensor([-0.5], dtype=torch.float64)
    out_ref, g_ref = terms_reference(spec, 5, 1, [x, y, y2], dout)
    out, g = terms_device(spec, 5, 1, [x, y, y2], dout)
    check(out, out_ref, "cosine_terms fwd, degenerate rows")
    check_rows(g[0], g_ref[0], "cosine_terms bwd, degenerate rows")
    assert g[1] is None and g[2] is None


# ----------------------------------------------------------------------------------------------------------------------------------------
# 5. trilinear
# ----------------------------------------------------------------------------------------------------------------------------------------
def tri_lds_bytes(H, W, s):
    """pcrl_upsample_trilinear_bwd's request for the planes kernel: an [H s][W s] and an [H][W s] float image"""
    return (H * s * W * s + H * W * s) * 4


def tri_planes_limit():
    """the launcher's LDS threshold, read from the source so that a change of it is noticed here"""
    src = open(os.path.join(os.path.dirname(ops.__file__), "csrc", "heads_loss.hip")).read()
    m = re.search(r"scale > 1 && lds <= (\d+) \* 1024", src)
    assert m, "pcrl_upsample_trilinear_bwd no longer selects its kernel by `scale > 1 && lds <= K * 1024`: revisit the shapes of this file"
    return int(m.group(1)) * 1024


PLANES = [((2, 3, 5, 7), 2), ((2, 3, 5, 7), 3), ((2, 3, 5, 7), 4),
          ((2, 1, 1, 1), 2), ((2, 1, 1, 1), 4), ((1, 1, 6, 1), 2), ((1, 1, 6, 1), 4), ((1, 4, 1, 5), 2), ((1, 4, 1, 5), 4),
          ((1, 2, 40, 64), 2)]
GATHER = [((1, 2, 32, 32), 4), ((1, 3, 64, 48), 2), ((2, 3, 5, 7), 1)]


@pytest.mark.parametrize("shape,s,kernel", [(sh, s, "planes") for sh, s in PLANES] + [(sh, s, "gather") for sh, s in GATHER])
def test_trilinear_both_backward_kernels(shape, s, kernel):
    """pcrl_upsample_trilinear_fwd / _bwd against float64 F.interpolate(mode="trilinear") autograd, project tolerance 2e-5 * max|ref|, and the
    adjoint identity <dy, up(x)> = <bwd(dy), x>.
    The backward takes tri_bwd_planes_kernel when scale > 1 and (H s W s + H W s) * 4 <= 60 KiB of LDS, else the gather tri_bwd_kernel:
      planes  (2,3,5,7) at s = 2, 3, 4 (3: the only odd scale; weights 1/6, 3/6, 5/6); size-1 axes (2,1,1,1), (1,1,6,1), (1,4,1,5) where
              i1 == i0 and a voxel collects both weights; (1,2,40,64) at s = 2 asks for exactly 61 440 bytes, the most the branch may request
      gather  (1,2,32,32) at s = 4 would need 81 920 bytes, (1,3,64,48) at s = 2 73 728; s = 1 is the identity in both directions (compared
              bit for bit)
    Adjoint bound 1e-5 relative to the larger inner product, both evaluated in float64 from the float32 outputs: each side carries the
    float32 interpolation error of one kernel, about 5 x the per-element 2e-5 * max would allow on a sum of same-signed terms; the inputs are
    uniform(-0.5, 1.5) so that neither inner product cancels."""
    N, D, H, W = shape
    lds, limit = tri_lds_bytes(H, W, s), tri_planes_limit()
    assert (s > 1 and lds <= limit) == (kernel == "planes"), (shape, s, lds, limit)
    if (shape, s) == ((1, 2, 40, 64), 2):
        assert lds == 61440 == limit
    if (shape, s) == ((1, 3, 64, 48), 2):
        assert lds == 73728 > limit
    x = (rnd(N, 1, D, H, W, seed=1) + 0.5).float().double().requires_grad_(True)
    ref = F.interpolate(x, scale_factor=s, mode="trilinear")
    dy = (rnd(*ref.shape, seed=2) + 0.5).float().double()
    ref.backward(dy)
    xd, dyd = dev(x.detach()), dev(dy)
    y = ops.upsample_forward(xd, s)
    dx = ops.upsample_backward(dyd, tuple(x.shape), s)
    if s == 1:
        same_bits(y, x.detach().float(), "trilinear fwd, scale 1")
        same_bits(dx, dy.float(), "trilinear bwd, scale 1")
    check(y, ref.detach(), f"trilinear fwd {shape} x{s}")
    check(dx, x.grad, f"trilinear bwd ({kernel}) {shape} x{s}")
    a, b = (dy * back(y)).sum().item(), (back(dx) * x.detach()).sum().item()
    print(f"  adjoint {shape} x{s}: <dy, up x> = {a:.9e}, <bwd dy, x> = {b:.9e}, rel {abs(a - b) / max(abs(a), abs(b)):.2e}")
    assert abs(a - b) <= 1e-5 * max(abs(a), abs(b))


def test_trilinear_rejections():
    """the ABI takes scale 1 .. 4 (TRI_MAXW = 16 weights per axis cover 3 s <= 12 outputs): 0 and 5 are refused in both directions"""
    x = torch.zeros(1, 1, 2, 2, 2, dtype=F32, device=DEV)
    for s in (0, 5):
        with pytest.raises(PcrlError):
            lib().call("pcrl_upsample_trilinear_fwd", x, x, 1, 2, 2, 2, s, stream_handle())
        with pytest.raises(PcrlError):
            lib().call("pcrl_upsample_trilinear_bwd", x, x, 1, 2, 2, 2, s, stream_handle())


# ----------------------------------------------------------------------------------------------------------------------------------------
# 6. BatchNorm1d of the heads
# ----------------------------------------------------------------------------------------------------------------------------------------
def bn1d_reference(x, g, b, dy, relu, dt=torch.float64):
    x, g, b = (t.to(dt).clone().requires_grad_(True) for t in (x, g, b))
    C = x.shape[1]
    rm, rv = torch.zeros(C, dtype=dt), torch.ones(C, dtype=dt)
    z = F.batch_norm(x, rm, rv, g, b, training=True, momentum=0.1, eps=1e-5)
    y = torch.relu(z) if relu else z
    y.backward(dy.to(dt))
    return y.detach(), rm, rv, x.grad, g.grad, b.grad


def bn1d_device(x, g, b, dy, relu):
    C = x.shape[1]
    rmd, rvd = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    xd, gd, bd = dev(x), dev(g), dev(b)
    yd, mean, rstd = ops.bn1d_forward(xd, gd, bd, rmd, rvd, relu)
    dx, dg, db = ops.bn1d_backward(dev(dy), xd, yd, gd, mean, rstd, relu)
    return yd, rmd, rvd, dx, dg, db


BN1D_WHAT = ("fwd", "running_mean", "running_var", "dx", "dgamma", "dbeta")
BN1D_TOL = (1e-5, 1e-5, 1e-5, 2e-4, 1e-4, 1e-4)        # test_heads_bn1d_linear's


def bn1d_compare(x, g, b, dy, relu, tag, yard=False):
    ref = bn1d_reference(x, g, b, dy, relu)
    f32 = bn1d_reference(x, g, b, dy, relu, dt=F32) if yard else (None,) * 6
    got = bn1d_device(x, g, b, dy, relu)
    for what, tol, a, r, y in zip(BN1D_WHAT, BN1D_TOL, got, ref, f32):
        check(a, r, f"bn1d {what} {tag} relu={relu}", tol=tol, yard=y if what == "dx" else None)
    return got, ref


@pytest.mark.parametrize("C", [1, 3, 6, 64])
@pytest.mark.parametrize("rows", [2, 63, 64, 65, 192, 384])
def test_bn1d_rows_and_channels(rows, C):
    """pcrl_bn1d_fwd / _bwd (ReLU off and on) against float64 F.batch_norm autograd with test_heads_bn1d_linear's tolerances: 1e-5 forward and
    running statistics (unbiased variance), 2e-4 dx, 1e-4 dgamma / dbeta.  One wave per channel, lanes stride over the rows (`r += 64`):
    rows = 63 / 64 / 65 sit around one pass, 192 and 384 (the local views' row counts) are three and six passes, 2 is the smallest the ABI
    takes; four channels per block (`c = blockIdx.x * 4 + wave`, `if (c >= C) return`): C = 1, 3 and 6 leave waves of the last block without a
    channel.
    rows = 2 is ill-conditioned for dx in any float32 storage of the statistics: dx = gamma rstd (dy0 - dy1)/2 * eps / (var + eps), the
    factor eps / (var + eps) ~ 1e-4 is 1 - xhat^2 and an error of 1e-7 in rstd is 1e-3 of it.  There the dx bound is the larger of the project
    tolerance and 4 x the error of torch's own float32 CPU batch_norm autograd against the same float64 reference.  Measured on the CPU for
    these inputs: C = 1 yardstick 4.2e-7 = 6e-4 of max|ref| (project 2e-4 = 1.4e-7; the kernel's arithmetic -- float32 mean / rstd, the rest
    in double -- evaluated on the CPU gives 5.1e-7); C = 3 yardstick 1.7e-7 / 4.3e-7 (ReLU off / on) against a project bound of 7e-7; C = 6
    and 64 yardsticks 30 x and more below the project bound, which a column of small variance sets."""
    x = rnd(rows, C, seed=1)
    g, b = 1 + 0.2 * rnd(C, seed=2), 0.2 * rnd(C, seed=3)
    dy = rnd(rows, C, seed=4)
    x, g, b, dy = (t.float().double() for t in (x, g, b, dy))
    for relu in (False, True):
        bn1d_compare(x, g, b, dy, relu, f"rows={rows} C={C}", yard=rows == 2)


@pytest.mark.parametrize("rows", [63, 65, 192, 384])
def test_bn1d_zero_variance_and_exact_zero_columns(rows):
    """pcrl_bn1d_fwd / _bwd on two special columns among six (same tolerances):
    column 1 is constant: var = 0, rstd = 1 / sqrt(eps), the output is beta exactly;
    column 4 has beta = 0 and x = (-a, 0, +a, -a, 0, +a, ..., 0 for what is left): its mean is exactly 0 in any summation order, so the rows
    with x = 0 normalise to exactly 0 and the ReLU output there is exactly 0.  Those rows must get zero gradient, as aten's
    threshold_backward gives (`y <= 0` in bn1d_bwd_kernel, not `y < 0`): asserted through the float64 reference and, separately, through
    dbeta of that column = the sum of dy over the rows with x = +a alone (dy is uniform(-0.75, 1.25): the x = 0 rows would add a third more)."""
    C, a = 6, 0.75
    x = rnd(rows, C, seed=11)
    x[:, 1] = 0.3125
    col = torch.zeros(rows, dtype=torch.float64)
    k = rows // 3 * 3
    col[:k] = torch.tensor([-a, 0.0, a], dtype=torch.float64).repeat(rows // 3)
    x[:, 4] = col
    g, b = 1 + 0.2 * rnd(C, seed=12), 0.2 * rnd(C, seed=13)
    b[4] = 0.0
    dy = rnd(rows, C, seed=14) + 0.25
    x, g, b, dy = (t.float().double() for t in (x, g, b, dy))
    for relu in (False, True):
        got, ref = bn1d_compare(x, g, b, dy, relu, f"special columns rows={rows}")
        y = back(got[0])
        assert bool((y[:, 1] == (b[1].clamp_min(0) if relu else b[1])).all()), "a constant column must come out as beta"
        assert bool((y[col == 0, 4] == 0).all()), "x = mean must normalise to exactly 0"
        if relu:
            # dbeta of column 4 = the sum of dy over the rows the ReLU passes: the x = 0 rows (output exactly 0) are not among them
            passed = dy[col > 0, 4].sum().item()
            assert abs(back(got[5])[4].item() - passed) <= 1e-4 * abs(passed)
            assert abs(ref[5][4].item() - passed) <= 1e-12 * abs(passed)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("C", [3, 64])
@pytest.mark.parametrize("rows", [1, 5, 192])
def test_bn1d_eval(rows, C, relu):
    """ops.bn1d_eval (eval-mode BatchNorm1d of the heads, + ReLU) against float64 F.batch_norm(training=False), check's default 2e-5 * max|ref|.
    C = 64 runs the vectorised per-channel apply kernel; C = 3 (rows * C = 3, 15, 576: no multiple of the 4-float vector, and rows = 1 is a
    single row, which eval mode takes and training mode refuses) runs the scalar bn1d_eval_kernel."""
    x, g, b = rnd(rows, C, seed=1, scale=2.0), 1 + 0.2 * rnd(C, seed=2), 0.2 * rnd(C, seed=3)
    rm, rv = 0.5 * rnd(C, seed=4), 0.25 + (rnd(C, seed=5) + 1)
    x, g, b, rm, rv = (t.float().double() for t in (x, g, b, rm, rv))
    ref = F.batch_norm(x, rm, rv, g, b, training=False, eps=1e-5)
    ref = torch.relu(ref) if relu else ref
    got = ops.bn1d_eval(dev(x), dev(g), dev(b), dev(rm), dev(rv), relu)
    check(got, ref, f"bn1d_eval rows={rows} C={C} relu={relu}")


# ----------------------------------------------------------------------------------------------------------------------------------------
# 7. small pieces
# ----------------------------------------------------------------------------------------------------------------------------------------
def test_sigmoid_saturation():
    """pcrl_sigmoid_fwd / _bwd at x = 0, +-1e-8, +-20, +-88, +-100, +-inf: expf overflows to inf from x = -88.8 down and 1 / (1 + inf) must be 0,
    not NaN.  Results finite, in [0, 1], equal to the float64 sigmoid to 2e-7 absolute (derived: one expf, one add, one divide, each within
    an ulp or two of a value in [0, 1]); the backward dout * a * (1 - a) against float64 on the forward's own float32 output, same bound
    (two products of values in [0, 1])."""
    inf = float("inf")
    x = torch.tensor([0.0, 1e-8, -1e-8, 20, -20, 88, -88, 100, -100, inf, -inf], dtype=F32)
    L, s = lib(), stream_handle()
    xd, yd = x.to(DEV), torch.full((x.numel(),), SENT, dtype=F32, device=DEV)
    L.call("pcrl_sigmoid_fwd", xd, yd, x.numel(), s)
    y = back(yd)
    assert bool(torch.isfinite(y).all()) and bool(((y >= 0) & (y <= 1)).all()), y
    err = (y - torch.sigmoid(x.double())).abs().max().item()
    print(f"  sigmoid fwd at the saturation points: max|d| = {err:.3e}")
    assert err <= 2e-7
    assert y[-2].item() == 1.0 and y[-1].item() == 0.0 and y[0].item() == 0.5
    dout = (rnd(x.numel(), seed=1) + 1.5).float()
    dpre = torch.full_like(yd, SENT)
    L.call("pcrl_sigmoid_bwd", dout.to(DEV), yd, dpre, x.numel(), s)
    d = back(dpre)
    assert bool(torch.isfinite(d).all())
    assert (d - dout.double() * y * (1 - y)).abs().max().item() <= 2e-7


def test_sigmoid_past_the_grid_stride_cap():
    """pcrl_sigmoid_fwd / _bwd on 2 097 152 + 300 elements, uniform(-8, 8): 300 threads take a second grid-stride step.  Same 2e-7 absolute."""
    n = CAP_ITEMS + 300
    x, dout = rnd32(n, seed=1) * 8, rnd32(n, seed=2)
    L, s = lib(), stream_handle()
    xd, yd = x.to(DEV), torch.full((n + 4,), SENT, dtype=F32, device=DEV)
    L.call("pcrl_sigmoid_fwd", xd, yd, n, s)
    y = back(yd)
    assert bool((y[n:] == SENT).all())
    y = y[:n]
    assert (y - torch.sigmoid(x.double())).abs().max().item() <= 2e-7
    dpre = torch.full((n + 4,), SENT, dtype=F32, device=DEV)
    L.call("pcrl_sigmoid_bwd", dout.to(DEV), yd, dpre, n, s)
    d = back(dpre)
    assert bool((d[n:] == SENT).all())
    assert (d[:n] - dout.double() * y * (1 - y)).abs().max().item() <= 2e-7


def test_guard_flag_at_the_threshold():
    """pcrl_guard_flag at threshold 1000: `loss > threshold` exactly as the reference's `if loss > 1000` -- 999.99 -> 0, 1000 -> 0, the float32
    successor of 1000 -> 1, +inf -> 1, -inf -> 0, NaN -> 0 (NaN > x is false: the reference would not skip such a step either)."""
    nxt = torch.nextafter(torch.tensor(1000.0, dtype=F32), torch.tensor(2000.0, dtype=F32)).item()
    cases = [(999.99, 0.0), (1000.0, 0.0), (nxt, 1.0), (float("inf"), 1.0), (float("-inf"), 0.0), (float("nan"), 0.0)]
    assert nxt > 1000.0
    for v, want in cases:
        flag = torch.full((1,), SENT, dtype=F32, device=DEV)
        lib().call("pcrl_guard_flag", torch.tensor([v], dtype=F32, device=DEV), 1000.0, flag, stream_handle())
        assert flag.item() == want, (v, flag.item(), want)


@pytest.mark.parametrize("n", [1, 255, 257, 4096 * 256 + 77])
def test_add_f32(n):
    """ops.add2_small (pcrl_add_f32, csrc/heads2d.hip), exact against torch float32 a + b: one thread, one block less one, one block plus
    one, and 4096 * 256 + 77 -- past this launcher's own cap of 4096 blocks, so 77 threads take a second grid-stride step."""
    a, b = rnd32(n, seed=1), rnd32(n, seed=2)
    same_bits(ops.add2_small(a.to(DEV), b.to(DEV)), a + b, f"add_f32 n={n}")


@pytest.mark.parametrize("rows,Cin,Cout", [(33, 64, 12), (192, 256, 128)])
def test_linear_products_on_operands_that_are_not_16_byte_aligned(rows, Cin, Cout):
    """pcrl_linear_fwd / _bwd with x and w as views that start 4 bytes into a buffer (parameters are slices of the optimizer's arena; a
    caller of the C ABI need not pad them).  Cin is a multiple of 4 in both cases, so only the launcher's al16() test keeps the float4
    kernels (linear_fwd / _dx / _dw_kernel) away: all three products must take sgemm_small_kernel.  (33, 64, 12): ragged 32 x 32 tiles in
    both directions, K = one chunk of 64; (192, 256, 128): a head's size, four K chunks.  Against float64 at test_linear_products' 2e-6."""
    x, w, b = rnd(rows, Cin, seed=1), rnd(Cout, Cin, seed=2, scale=0.1), rnd(Cout, seed=3)
    dy = rnd(rows, Cout, seed=4)
    xd, wd = off4(x), off4(w)
    bd, dyd = dev(b), dev(dy)
    x64, w64, dy64 = (t.float().double() for t in (x, w, dy))
    check(ops.linear_forward(xd, wd, bd), x64 @ w64.T + b.float().double(), "linear fwd, unaligned", tol=2e-6)
    dx, dw, db = ops.linear_backward(dyd, xd, wd)
    check(dx, dy64 @ w64, "linear dx, unaligned", tol=2e-6)
    check(dw, dy64.T @ x64, "linear dw, unaligned", tol=2e-6)
    check(db, dy64.sum(0), "linear db, unaligned", tol=2e-6)


def sgd_reference(p0, gr, b0, offs, sizes, flags, lr, mom, wd, gs):
    ep, eb = p0.clone(), b0.clone()
    for t, (o, n) in enumerate(zip(offs, sizes)):
        if not flags[t] & 1:
            continue
        sl = slice(o, o + n)
        gg = gr[sl] * gs + wd * p0[sl]
        bb = mom * b0[sl] + gg if flags[t] & 2 else gg
        eb[sl] = bb
        ep[sl] = p0[sl] - lr * bb
    return ep, eb


def test_sgd_step_past_the_grid_stride_cap():
    """pcrl_sgd_step on one arena of 5 + (8 388 608 + 1028) + 7 + 64 + 3 floats: 2 097 152 + 277 groups of four, more than grid_for()'s
    8192 x 256, so sgd4_kernel's threads take a second grid-stride step inside the big tensor and into the small ones behind it.  The slots
    are unpadded, so the groups at the tensor borders straddle tensors with different flags (bit 0 has a gradient, bit 1 has momentum) and
    take the kernel's scalar branch.  Against the float64 update at test_sgd_kernel_on_an_unpadded_arena's 2e-6."""
    sizes = [5, CAP4 + 1028, 7, 64, 3]
    flags = [1, 3, 0, 2, 1]
    offs = [0]
    for n in sizes:
        offs.append(offs[-1] + n)
    total = offs[-1]
    p32, g32, b32 = (rnd32(total, seed=s) for s in (1, 2, 3))
    lr, mom, wd, gs = 0.05, 0.9, 1e-2, 0.5
    ep, eb = sgd_reference(p32.double(), g32.double(), b32.double(), offs, sizes, flags, lr, mom, wd, gs)
    pd, gd, bd = p32.to(DEV), g32.to(DEV), b32.to(DEV)
    lib().call("pcrl_sgd_step", pd, gd, bd, torch.tensor(offs, dtype=torch.int64, device=DEV), torch.tensor(flags, dtype=torch.int32, device=DEV),
               len(sizes), total, lr, mom, wd, gs, stream_handle())
    check(pd, ep, "sgd parameters past the cap", tol=2e-6)
    check(bd, eb, "sgd momentum buffers past the cap", tol=2e-6)
    # the tensors without a gradient are untouched bit for bit
    for t in (2, 3):
        sl = slice(offs[t], offs[t + 1])
        same_bits(pd[sl], p32[sl], f"sgd: parameter of tensor {t} (no gradient)")
        same_bits(bd[sl], b32[sl], f"sgd: momentum of tensor {t} (no gradient)")


def test_sgd_step_guarded_against_the_plain_entry_point():
    """pcrl_sgd_step_guarded: with skip = 0 bit-equal to pcrl_sgd_step on copies of the same arenas; with skip = 1 parameters, gradients and
    momentum buffers are bit-unchanged (`if (skip && *skip != 0.f) return`); a null flag is refused."""
    L, s = lib(), stream_handle()
    sizes = [5, 1, 7, 64, 3, 130, 2]
    flags = [1, 3, 0, 3, 1, 2, 3]
    offs = [0]
    for n in sizes:
        offs.append(offs[-1] + n)
    total = offs[-1]
    p0, g0, b0 = (rnd32(total, seed=s_) for s_ in (4, 5, 6))
    od, fd = torch.tensor(offs, dtype=torch.int64, device=DEV), torch.tensor(flags, dtype=torch.int32, device=DEV)
    hp = (0.05, 0.9, 1e-2, 0.5)
    plain = [t.to(DEV) for t in (p0, g0, b0)]
    L.call("pcrl_sgd_step", *plain, od, fd, len(sizes), total, *hp, s)
    assert not torch.equal(plain[0].cpu(), p0)
    go = [t.to(DEV) for t in (p0, g0, b0)]
    L.call("pcrl_sgd_step_guarded", *go, od, fd, len(sizes), total, *hp, torch.zeros(1, device=DEV), s)
    for a, b, what in zip(go, plain, ("parameters", "gradients", "momentum")):
        same_bits(a, b.cpu(), f"guarded, skip = 0: {what}")
    held = [t.to(DEV) for t in (p0, g0, b0)]
    L.call("pcrl_sgd_step_guarded", *held, od, fd, len(sizes), total, *hp, torch.ones(1, device=DEV), s)
    for a, b, what in zip(held, (p0, g0, b0), ("parameters", "gradients", "momentum")):
        same_bits(a, b, f"guarded, skip = 1: {what}")
    with pytest.raises(PcrlError):
        L.call("pcrl_sgd_step_guarded", *held, od, fd, len(sizes), total, *hp, None, s)
