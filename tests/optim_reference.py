"""numpy restatement of csrc/optim.hip, operation by operation: pcrl_adam_prepare (float64 running products), pcrl_adam_step (float32, one
rounding per operation, torch.optim.Adam / AdamW's single-tensor order) and pcrl_grad_norm (float64, the kernel's own summation order).

The arena is a flat float32 array; `offsets` (ntensors + 1) and `flags` (bit 0: the tensor has a gradient) are the kernels' tables."""
import numpy as np

F = np.float32
GRID_CAP = 2048          # pcrl_optim_grid_cap(): asserted equal by the GPU tests


class AdamTables:
    """Per-tensor step counts, products beta^t and the two float32 coefficients."""

    def __init__(self, ntensors):
        self.steps = np.zeros(ntensors, np.int32)
        self.prods = np.ones((ntensors, 2), np.float64)
        self.coefs = np.zeros((ntensors, 2), np.float32)

    def copy(self):
        t = AdamTables(len(self.steps))
        t.steps, t.prods, t.coefs = self.steps.copy(), self.prods.copy(), self.coefs.copy()
        return t


def adam_prepare(tab, flags, lr, beta1, beta2):
    for t, f in enumerate(flags):
        if not f & 1:
            continue
        tab.steps[t] += 1
        b1 = np.float64(tab.prods[t, 0]) * np.float64(beta1)
        b2 = np.float64(tab.prods[t, 1]) * np.float64(beta2)
        tab.prods[t] = (b1, b2)
        tab.coefs[t, 0] = F(np.float64(lr) / (np.float64(1.0) - b1))
        tab.coefs[t, 1] = F(np.sqrt(np.float64(1.0) - b2))


def adam_step(p, g, m, v, offsets, flags, tab, lr, wd, beta1, beta2, eps, decoupled, grad_scale=1.0, clip_coef=None):
    """In place on float32 arrays p, m, v.  The scalars reach the kernel as float32: decay = (float)(1 - lr * wd) or (float)wd,
    (float)(1 - beta1), (float)beta2, (float)(1 - beta2), (float)eps."""
    gs, eps32 = F(grad_scale), F(eps)
    decay = F(1.0 - lr * wd) if decoupled else F(wd)
    omb1, b2, omb2 = F(1.0 - beta1), F(beta2), F(1.0 - beta2)
    for t, f in enumerate(flags):
        if not f & 1:
            continue
        sl = slice(int(offsets[t]), int(offsets[t + 1]))
        pp, mm, vv = p[sl], m[sl], v[sl]
        gg = g[sl] * gs
        if clip_coef is not None:
            gg = gg * F(clip_coef)
        if decoupled:
            pp = pp * decay
        else:
            gg = gg + decay * pp
        mm = mm + (gg - mm) * omb1
        vv = vv * b2 + (gg * gg) * omb2
        pp = pp - tab.coefs[t, 0] * (mm / (np.sqrt(vv) / tab.coefs[t, 1] + eps32))
        assert pp.dtype == F and mm.dtype == F and vv.dtype == F
        p[sl], m[sl], v[sl] = pp, mm, vv


def summable_grads(n, seed):
    """float32 gradients that are integer multiples of 2^-8 with |g| <= 4: their squares sum exactly in float64 in ANY order (assert_summable)."""
    k = np.random.default_rng(seed).integers(-1024, 1025, size=n)
    return (k.astype(np.float64) / 256.0).astype(F)


def assert_summable(g, grad_scale=1.0):
    """The precondition of the order-free norm tests: every (g * grad_scale)^2 is an integer multiple of one power of two `u`, and their sum stays
    below 2^53 * u -- so every partial sum in every order is exact.  -> the exact sum of squares."""
    d = (np.asarray(g, F) * F(grad_scale)).astype(np.float64)
    assert np.array_equal(d, np.asarray(g, np.float64) * np.float64(grad_scale)), "g * grad_scale is not exact in float32"
    u = 2.0 ** -18                       # (2^-8 * 2^-1)^2: grad_scale 1 and 0.5
    q = d * d / u
    assert np.array_equal(q, np.rint(q)), "a square is not a multiple of 2^-18"
    total = int(np.sum(q.astype(np.int64)))          # exact integer arithmetic: each q <= 16 * 2^18 = 2^22
    assert total < 2 ** 53
    return total * u


def _tree64(a):
    """The wave's xor-butterfly sum over the last axis (64 lanes): halves added pairwise, 32 .. 1."""
    n = a.shape[-1]
    while n > 1:
        n //= 2
        a = a[..., :n] + a[..., n:2 * n]
    return a[..., 0]


def _block_sum(a):
    """block_sum_256 over the last axis (256 threads): four wave sums added in order."""
    w = _tree64(a.reshape(a.shape[:-1] + (4, 64)))
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def grad_norm(g, offsets, flags, grad_scale, max_norm, numels=None):
    """-> (norm float64, coef float32), summed in pcrl_grad_norm's order: thread `b * 256 + t` of `grid` blocks takes the groups of four
    q = b * 256 + t, + grid * 256, ... one element after the other; block sums, then one block over the partials."""
    total = int(offsets[-1])
    counted = np.zeros(total, bool)
    for t, f in enumerate(flags):
        if f & 1:
            n = int(offsets[t + 1] - offsets[t]) if numels is None else int(numels[t])
            counted[int(offsets[t]):int(offsets[t]) + n] = True
    d = (np.asarray(g[:total], F) * F(grad_scale)).astype(np.float64)
    sq = np.where(counted, d * d, 0.0)          # an element that does not count is not added; adding +0.0 to a sum of squares is the same bits
    ngroups = (total + 3) // 4
    grid = min(max((ngroups + 255) // 256, 1), GRID_CAP)
    iters = (ngroups + grid * 256 - 1) // (grid * 256)
    pad = np.zeros(iters * grid * 256 * 4, np.float64)
    pad[:total] = sq
    pad = pad.reshape(iters, grid, 256, 4)
    acc = np.zeros((grid, 256), np.float64)
    for k in range(iters):
        for c in range(4):
            acc = acc + pad[k, :, :, c]
    partials = _block_sum(acc)
    acc2 = np.zeros(256, np.float64)
    for k in range(0, grid, 256):
        chunk = np.zeros(256, np.float64)
        chunk[:min(256, grid - k)] = partials[k:k + 256]
        acc2 = acc2 + chunk
    norm = np.sqrt(_block_sum(acc2))
    with np.errstate(invalid="ignore"):
        c = np.float64(max_norm) / (norm + np.float64(1e-6))
    if c > 1.0:
        c = np.float64(1.0)
    return np.float64(norm), F(c)
