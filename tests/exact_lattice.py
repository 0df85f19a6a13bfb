"""Exactly summable operands: the helper of the bit-for-bit convolution tests (test_exact_lattice_cpu.py, test_conv2d_exact_gpu.py,
test_conv3d_exact_gpu.py, test_conv_to1_exact_gpu.py, test_convt_exact_gpu.py, test_upconv_exact_gpu.py).  Not a test file.

Operands drawn from a small dyadic lattice (integers / a power of two) are exactly representable in bf16, every product of two of them is exact in
float32, and every partial sum of such products -- in any order, over any split -- is an integer multiple of one fixed unit.  While the sum of the
ABSOLUTE values of all terms of an output stays below 2^24 units, every partial sum in every order does too, so a float32 accumulation is exact
whatever the summation order: the accumulator equals the float64 value.  A float32 output must then equal the float64 reference exactly, a bf16 output
its round-to-nearest-even rounding, at every element.  No measured number enters."""
import torch

EXACT_LIMIT = float(2 ** 24)      # float32 holds every integer of magnitude <= 2^24

# the lattices of the convolution cases: (max_int, den) of the source, of the weight (and of the bias, the gradient, shift and residual)
#   fine   : x = i/4, |i| <= 4; w = j/8, |j| <= 2 -- sums land between bf16 values (and often on ties): the output rounding is exercised
#   ternary: x, w in {-1, 0, 1} -- small enough that the per-channel sums of SQUARES of the outputs (unit 1) stay exactly summable
#   finer  : x = i/8, |i| <= 8; w = j/32, |j| <= 8 -- for short sums (few source channels), whose values on the fine lattice would all be bf16 values
FINE = dict(x=(4, 4), w=(2, 8), b=(4, 4), dy=(4, 4))
FINER = dict(x=(8, 8), w=(8, 32), b=(4, 4), dy=(8, 8))
TERNARY = dict(x=(1, 1), w=(1, 1), b=(1, 1), dy=(1, 1))


def fine_for(terms):
    """The rounding-exercising lattice for sums of `terms` products: a bf16 output is only rounded once |y| exceeds 256 units."""
    return FINE if terms >= 512 else FINER


def lattice(shape, max_int, den, generator):
    """float64 CPU tensor of randint(-max_int, max_int) / den (both ends included); its bf16 round trip is the identity."""
    t = torch.randint(-max_int, max_int + 1, tuple(shape), generator=generator).double() / den
    assert torch.equal(t.to(torch.bfloat16).double(), t), f"lattice {max_int}/{den} is not representable in bf16"
    return t


def unit(*dens):
    """The unit every sum of products of lattice values with these denominators is a multiple of."""
    u = 1.0
    for d in dens:
        u /= d
    return u


def assert_exactly_summable(terms_abs_sum, unit, what=""):
    """The precondition of every bit-for-bit assertion: max of sum |terms| (a float64 tensor or number: F.conv(|x|, |w|, |b|) for a convolution,
    sum |x||dy| for a weight gradient, sum |y| and sum y^2 over the whole channel for a statistics row), in units of `unit`, is < 2^24.  The sum of
    absolute values bounds every partial sum in every order.  A violation is an error of the case list -- never skipped, never given a tolerance."""
    m = float(torch.as_tensor(terms_abs_sum, dtype=torch.float64).abs().max()) / unit
    if not m < EXACT_LIMIT:
        raise AssertionError(f"{what}: sum |terms| = {m:.4g} units of {unit:g} is not below 2^24: this case is not exactly summable (fix the case list)")
    return m / EXACT_LIMIT


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32 if t.dtype == torch.float32 else torch.int64)


def _where(idx, shape, names, brick):
    """'(n=.., c=.., h=.., w=..) tensor border: h; brick border: w' for one coordinate"""
    tb, bb = [], []
    for k, (i, ext, nm) in enumerate(zip(idx, shape, names)):
        if nm == "c":
            continue
        if nm != "n" and (i == 0 or i == ext - 1):
            tb.append(nm)
        b = (brick or {}).get(nm)
        if b and (i % b == 0 or i % b == b - 1):
            bb.append(nm)
    s = "(" + ", ".join(f"{nm}={i}" for nm, i in zip(names, idx)) + ")"
    s += " tensor border: " + (",".join(tb) if tb else "no")
    if brick:
        s += "; brick border: " + (",".join(bb) if bb else "no")
    return s


def assert_bit_equal(got, ref64, dtype, what, brick=None, show=6):
    """Every element of `got` (any device, dtype `dtype`, logical [N,C,H,W] / [N,C,D,H,W] or any other shape) equals ref64.to(dtype) in bits.
    The message names the number of differing elements and the first few coordinates, and for each whether it lies on a tensor border (first / last
    index of a spatial axis) or on a brick border (`brick`: {axis name: brick extent}, e.g. {"n": 4, "h": 8, "w": 16})."""
    if got.is_cuda:
        torch.cuda.synchronize()      # results of every engine stream (weight gradients are produced on a side stream)
    got = got.detach().cpu()
    assert got.dtype == dtype, f"{what}: output is {got.dtype}, expected {dtype}"
    assert ref64.dtype == torch.float64 and tuple(got.shape) == tuple(ref64.shape), f"{what}: shape {tuple(got.shape)} against reference {tuple(ref64.shape)}"
    want = ref64.to(dtype)
    bad = _bits(got) != _bits(want)
    n = int(bad.sum())
    if n == 0:
        return
    names = {4: "nchw", 5: "ncdhw"}.get(got.dim(), "".join(chr(ord("i") + k) for k in range(got.dim())))
    idx = bad.nonzero()[:show].tolist()
    zero_sign = bool(((got.double() == 0) & (want.double() == 0))[bad].all())
    lines = [f"{what}: {n} of {got.numel()} elements differ from the {dtype} rounding of the float64 reference"
             + (" (all of them zeros of the other sign)" if zero_sign else "")]
    for i in idx:
        i = tuple(i)
        lines.append(f"  {_where(i, got.shape, names, brick)}: got {float(got[i]):.10g}, want {float(want[i]):.10g} (float64 {float(ref64[i]):.17g})")
    nan = int(torch.isnan(got.double()).sum())
    if nan:
        lines.append(f"  {nan} elements are NaN (never written?)")
    raise AssertionError("\n".join(lines))


def assert_rows_exact(rows_f32, ref64, what):
    """Partial rows [rows][C] (float32, each exact by the precondition) summed over the rows in float64 equal the float64 reference [C] exactly."""
    if rows_f32.is_cuda:
        torch.cuda.synchronize()
    got = rows_f32.detach().double().cpu().sum(0)
    bad = (got != ref64).nonzero().flatten().tolist()
    assert not bad, f"{what}: {len(bad)} of {got.numel()} channels differ; first {[(c, float(got[c]), float(ref64[c])) for c in bad[:6]]}"
