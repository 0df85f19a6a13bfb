"""Float64 CPU restatement of the segmentation head and its loss (csrc/seg_head.hip) with torch: F.linear over the channels -> sigmoid ->
wb * BCE + wd * (1 - mean_k Dice_k) with the voxels whose label has bit 7 masked out; torch.autograd.grad gives dx, dW, db.  Not a test file."""
import torch
import torch.nn.functional as F

EPS = 1.0


def reference(a, w, b, labels, dloss=1.0, wb=1.0, wd=1.0, case_index=None, n_cases=None, S=None):
    """a [M, 64] (any float dtype; upcast exactly), w [K, 64], b [K], labels uint8 [M].  -> dict of float64 / integer CPU tensors.
    With S (voxels per sample): counts int64 [n_cases, K, 3] = {TP, |pred|, |gt|} of sample n at row case_index[n], pred = (z >= 0)."""
    K = w.shape[0]
    x = a.double().clone().requires_grad_(True)
    w64, b64 = w.double().clone().requires_grad_(True), b.double().clone().requires_grad_(True)
    z = F.linear(x, w64, b64)                                                   # [M, K]
    p = torch.sigmoid(z)
    lab = labels.to(torch.int64)
    counted = ((lab & 0x80) == 0)
    g = torch.stack([((lab >> k) & 1) for k in range(K)], dim=1).double()       # [M, K]
    c = counted.double().unsqueeze(1)
    Mc = int(counted.sum())
    I, P, G = (p * g * c).sum(0), (p * c).sum(0), (g * c).sum(0)
    terms = torch.clamp(z, min=0) - g * z + torch.log1p(torch.exp(-z.abs()))
    bce_k = (terms * c).sum(0)
    bce = bce_k.sum() / (Mc * K) if Mc > 0 else z.sum() * 0.0
    dice = (2 * I + EPS) / (P + G + EPS)
    loss = wb * bce + wd * (1.0 - dice.mean())
    dx, dw, db = torch.autograd.grad(loss, (x, w64, b64), grad_outputs=torch.tensor(float(dloss), dtype=torch.float64), allow_unused=True)
    zero = lambda t, like: torch.zeros_like(like) if t is None else t          # noqa: E731
    out = dict(z=z.detach(), p=p.detach(), g=g, counted=counted, Mc=Mc, I=I.detach(), P=P.detach(), G=G.detach(), bce_k=bce_k.detach(), terms=terms.detach(),
               loss=loss.detach(), dx=zero(dx, x), dw=zero(dw, w64), db=zero(db, b64),
               sums=torch.cat([torch.stack([I, P, G, bce_k], dim=1).reshape(-1).detach(), torch.tensor([float(Mc)], dtype=torch.float64)]))
    pred = (z.detach() >= 0) & counted.unsqueeze(1)
    out["mask"] = sum((pred[:, k].to(torch.int64) << k) for k in range(K)).to(torch.uint8)
    if S is not None:
        N = a.shape[0] // S
        ci = list(range(N)) if case_index is None else [int(v) for v in case_index]
        counts = torch.zeros((n_cases if n_cases is not None else N, K, 3), dtype=torch.int64)
        gt = (g > 0) & counted.unsqueeze(1)
        for n in range(N):
            sl = slice(n * S, (n + 1) * S)
            counts[ci[n], :, 0] += (pred[sl] & gt[sl]).sum(0)
            counts[ci[n], :, 1] += pred[sl].sum(0)
            counts[ci[n], :, 2] += gt[sl].sum(0)
        out["counts"] = counts
    return out
