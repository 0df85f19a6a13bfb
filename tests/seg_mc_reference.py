"""Float64 CPU restatement of the softmax segmentation head and its loss (csrc/seg_head_mc.hip) with torch, and of the label-map blend's fixed-order
float32 accumulation (csrc/seg_blend.hip) in numpy.  The gradients are the CLOSED FORM the kernels implement, not autograd: tests/test_seg_mc_cpu.py
checks them against torch's own autograd through log_softmax.  Not a test file.

    z = W a + b;  p = softmax(z);  ce = logsumexp(z) - z_y           y = label & 0x7F; counted: bit 7 clear and y < K
    I_k = sum_{y=k} p_k, P_k = sum p_k, G_k = #{y=k}, CE_k = sum_{y=k} ce        over the counted voxels
    loss = wc sum_k CE_k / Mc + wd (1 - 1/(K-1) sum_{k=1}^{K-1} (2 I_k + 1) / (P_k + G_k + 1))         (CE term 0 when Mc = 0)
    q_0 = 0, q_k = -(c wd / (K-1)) (2 [y=k] / U_k - (2 I_k + 1) / U_k^2), U_k = P_k + G_k + 1
    dz_j = c wc / Mc (p_j - [y=j]) + p_j (q_j - sum_k p_k q_k)"""
import torch

EPS = 1.0


def lowest_argmax(z):
    """The LOWEST index of the maximum of every row (torch.argmax's tie rule is restated, not relied upon)."""
    K = z.shape[-1]
    m = z.max(-1, keepdim=True).values
    idx = torch.arange(K, dtype=torch.int64).expand_as(z)
    return torch.where(z == m, idx, torch.full_like(idx, K)).min(-1).values


def reference(a, w, b, labels, dloss=1.0, wc=1.0, wd=1.0, case_index=None, n_cases=None, S=None):
    """a [M, 64] (any float dtype; upcast exactly), w [K, 64], b [K], labels uint8 [M] (a label map).  -> dict of float64 / integer CPU tensors.
    With S (voxels per sample): counts int64 [n_cases, K, 3] = {TP, |pred|, |gt|} of sample n at row case_index[n] for all K classes."""
    K = w.shape[0]
    x, w64, b64 = a.double(), w.double(), b.double()
    z = x @ w64.t() + b64
    lab = labels.to(torch.int64)
    y = lab & 0x7F
    counted = ((lab & 0x80) == 0) & (y < K)
    z = torch.where(counted.unsqueeze(1), z, torch.zeros_like(z))          # an uncounted voxel's activations, finite or not, enter nothing
    m = z.max(1, keepdim=True).values
    e = torch.exp(z - m)
    s = e.sum(1, keepdim=True)
    p = e / s
    g = torch.zeros_like(z)
    g[counted, y[counted]] = 1.0
    c = counted.double().unsqueeze(1)
    ce = ((m - (z * g).sum(1, keepdim=True)) + torch.log(s)) * c           # [M, 1]
    Mc = int(counted.sum())
    I, P, G, CE = (p * g * c).sum(0), (p * c).sum(0), g.sum(0), (ce * g).sum(0)
    U, num = P + G + EPS, 2 * I + EPS
    dice = num[1:] / U[1:]
    loss = (wc * CE.sum() / Mc if Mc > 0 else torch.zeros((), dtype=torch.float64)) + wd * (1.0 - dice.sum() / (K - 1))
    cd = float(dloss) * wd / (K - 1)
    e1, e0 = cd * 2 / U, cd * num / U ** 2
    e1[0] = e0[0] = 0.0
    q = e0 - g * e1
    spq = (p * q).sum(1, keepdim=True)
    cA = float(dloss) * wc / Mc if Mc > 0 else 0.0
    dz = (cA * (p - g) + p * (q - spq)) * c
    x0 = torch.where(counted.unsqueeze(1), x, torch.zeros_like(x))
    out = dict(z=z, p=p, g=g, y=y, counted=counted, Mc=Mc, I=I, P=P, G=G, CE=CE, ce=ce.squeeze(1), m=m.squeeze(1), loss=loss, dz=dz, q=q, spq=spq, cA=cA,
               e0=e0, e1=e1, dx=dz @ w64, dw=dz.t() @ x0, db=dz.sum(0),
               sums=torch.cat([torch.stack([I, P, G, CE], dim=1).reshape(-1), torch.tensor([float(Mc)], dtype=torch.float64)]))
    pred = lowest_argmax(z)
    out["pred"] = pred
    out["labelmap"] = torch.where(counted, pred, torch.zeros_like(pred)).to(torch.uint8)
    if S is not None:
        N = a.shape[0] // S
        ci = list(range(N)) if case_index is None else [int(v) for v in case_index]
        counts = torch.zeros((n_cases if n_cases is not None else N, K, 3), dtype=torch.int64)
        ks = torch.arange(K).unsqueeze(0)
        pr = (pred.unsqueeze(1) == ks) & counted.unsqueeze(1)
        gt = g > 0
        for n in range(N):
            if not 0 <= ci[n] < counts.shape[0]:
                continue
            sl = slice(n * S, (n + 1) * S)
            counts[ci[n], :, 0] += (pr[sl] & gt[sl]).sum(0)
            counts[ci[n], :, 1] += pr[sl].sum(0)
            counts[ci[n], :, 2] += gt[sl].sum(0)
        out["counts"] = counts
    return out


def autograd_reference(a, w, b, labels, dloss=1.0, wc=1.0, wd=1.0):
    """The same loss through torch.log_softmax and torch.autograd (float64): the check OF reference(), used by the CPU test only."""
    import torch.nn.functional as F
    K = w.shape[0]
    x = a.double().clone().requires_grad_(True)
    w64, b64 = w.double().clone().requires_grad_(True), b.double().clone().requires_grad_(True)
    lab = labels.to(torch.int64)
    y = lab & 0x7F
    counted = ((lab & 0x80) == 0) & (y < K)
    z = F.linear(x, w64, b64)[counted]
    yc = y[counted]
    logp = F.log_softmax(z, dim=1)
    p = logp.exp()
    g = F.one_hot(yc, K).double()
    Mc = int(counted.sum())
    ce = F.nll_loss(logp, yc, reduction="sum") / Mc if Mc > 0 else z.sum() * 0.0
    dice = (2 * (p * g).sum(0) + EPS) / (p.sum(0) + g.sum(0) + EPS)
    loss = wc * ce + wd * (1.0 - dice[1:].mean())
    grads = torch.autograd.grad(loss, (x, w64, b64), grad_outputs=torch.tensor(float(dloss), dtype=torch.float64), allow_unused=True)
    dx, dw, db = (torch.zeros_like(t) if gr is None else gr for gr, t in zip(grads, (x, w64, b64)))
    return dict(loss=loss.detach(), dx=dx, dw=dw, db=db)
