"""Writes tests/golden/val2d_b4_64.npz: one held-out 2D validation pass (train_2d.validate's sixteen metrics and their total) in float64 on the CPU.

    python tools/make_val2d_fixtures.py

What is the reference's and what is not.  Every cosine term goes through the reference's own `train_2d.cos_loss` (train_2d.py:111-117), imported
the way oracle/make_golden.py::make_loss2d imports it (`_stub_modules()`), called on ONE-scale lists so that its `random.randint(0, 0)` picks the
scale we ask for; the MSE terms are torch.nn.MSELoss as train_2d.py:78 builds it; the local term is train_2d.py:148-163 around the imported
function.  The FORWARD is oracle/pcrlv2_2d_oracle.model_forward(training=False) in float64: the 2D model stays PARITY-UNPINNED -- the reference's
class needs segmentation_models_pytorch and torchvision, which are absent -- so this fixture pins the metric assembly and the draw-free expectation,
not the network.  State and batches: tests/val2d_state.py (shared with the GPU test, which rebuilds the state without the reference and checks
the digest stored here): 4 + 4 + 3 samples at 64^2 with 32^2 local views, epoch 0.

Besides the values the fixture stores what the test's bounds are derived from (nothing measured on the engine):
  max_abs_diff   max |prediction - gt| over the six full-resolution maps and all batches: an engine whose maps are within d of the oracle's
                 (d = 2e-4 of the largest entry of the map, the envelope test_eval_mode_forward_uses_the_running_statistics_2d holds the float32 eval
                 forward to; the bilinear interpolation is a convex combination and does not widen it) has every MSE metric within
                 2 * max_abs_diff * d + d^2.  mse_bound_f32 is that, with d from the largest map entry seen.
  cos_bound_f32  per scale k, exactly as tools/make_val_fixtures.py derives it: with every feature element within e = 2e-4 of the oracle's, a feature
                 vector of C_k elements moves by at most r = e sqrt(C_k) / |x| relative to its norm, its direction by at most r / (1 - r), and a
                 cosine of two such vectors by at most the sum of the two: the bound uses the SMALLEST feature norm of the scale; every cosine metric
                 is an average of cosines with total weight one.  (The 2D envelope is 2e-4 of the LARGEST entry of a tensor; max_feat_entry records
                 those entries: where they are below one the absolute e is the looser of the two readings, above one the stricter.)
CPU numbers of this recipe (printed and stored by every run): smallest feature norms per scale 2.61, 1.84, 1.32, 0.98, 0.62, so r = 1.16e-3 ... 1.30e-3
(all < 0.002: the derivation is valid) and the cosine bounds are 2.3e-3 ... 2.6e-3; max |pred - gt| = 5.298 and the largest map entry 5.468 give
d = 1.09e-3 and an MSE bound of 1.16e-2; the same oracle in float32 differs from the float64 one by <= 4.4e-7 on every metric -- a correct float32
engine sits orders of magnitude inside the bounds; tests/test_validate2d_gpu.py's weighting test, not the fixture, is what catches assembly
errors."""
import math
import os
import random
import sys
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_golden as G  # noqa: E402
import pcrlv2_2d_oracle as O2  # noqa: E402
import val2d_state as V  # noqa: E402

TAG, NS, FEAT_TOL_F32 = "val2d_b4_64", 5, 2e-4
KEYS = (("mse_out",) + tuple(f"mse_mid{k}" for k in range(NS)) + tuple(f"cos_global{k}" for k in range(NS)) + tuple(f"cos_local{k}" for k in range(NS)))


def batch_metrics(ref2d, criterion, cosine, out1, masks1, gt, feats1, feats2, feats_loc, nlocal):
    """The sixteen batch means, each cosine term through the reference's own cos_loss at a fixed scale index."""
    b = out1.shape[0]
    m = OrderedDict(mse_out=criterion(out1, gt))
    for k in range(NS):
        m[f"mse_mid{k}"] = criterion(masks1[k], gt)
    for k in range(NS):
        m[f"cos_global{k}"] = ref2d.cos_loss(cosine, [feats1[k]], [feats2[k]])[0]
    for k in range(NS):
        stacked = torch.stack(feats_loc[k])                    # train_2d.py:147
        local = 0.0
        for i in range(nlocal):                                # train_2d.py:148-163 at index k
            crop = [stacked[:, b * i: b * (i + 1)]]
            local = local + ref2d.cos_loss(cosine, [feats1[k]], crop)[0] + ref2d.cos_loss(cosine, [feats2[k]], crop)[0]
        m[f"cos_local{k}"] = local / (2 * nlocal)
    return OrderedDict((k, float(v)) for k, v in m.items())


def run(sd, ref2d, dtype):
    criterion, cosine = torch.nn.MSELoss(), torch.nn.CosineSimilarity()
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    sums = OrderedDict((k, 0.0) for k in KEYS)
    per_batch, max_abs_diff, max_map, min_norm, max_feat = [], 0.0, 0.0, [math.inf] * NS, [0.0] * NS
    with torch.backends.mkldnn.flags(enabled=False), torch.no_grad():
        for x1, x2, gt, _gt2, local_views in V.batches():
            b = x1.shape[0]
            x1, x2, gt, loc = x1.to(dtype), x2.to(dtype), gt.to(dtype), torch.cat(local_views, dim=0).to(dtype)
            feats1, out1, masks1 = O2.model_forward(x1, sd, training=False)
            feats2, _, _ = O2.model_forward(x2, sd, training=False)
            feats_loc, none, _ = O2.model_forward(loc, sd, local=True, training=False)
            assert none is None
            m = batch_metrics(ref2d, criterion, cosine, out1, masks1, gt, feats1, feats2, feats_loc, len(local_views))
            per_batch.append([m[k] for k in KEYS])
            for k in KEYS:
                sums[k] += b * m[k]
            max_abs_diff = max(max_abs_diff, *(float((t - gt).abs().max()) for t in (out1, *masks1)))
            max_map = max(max_map, *(float(t.abs().max()) for t in (out1, *masks1)))
            for k in range(NS):
                for fs in (feats1, feats2, feats_loc):
                    for t in fs[k]:
                        min_norm[k] = min(min_norm[k], float(t.norm(dim=1).min()))
                        max_feat[k] = max(max_feat[k], float(t.abs().max()))
    n = sum(V.BATCH_SIZES)
    vals = OrderedDict((k, sums[k] / n) for k in KEYS)
    return vals, per_batch, max_abs_diff, max_map, min_norm, max_feat


def total_of(vals, epoch):
    mean = lambda name: sum(vals[name + str(k)] for k in range(NS)) / NS
    beta = 0.5 * (1.0 + math.cos(math.pi * epoch / O2.BETA_PERIOD))
    return vals["mse_out"] + mean("cos_global") + mean("cos_local") + beta * mean("mse_mid")


def main():
    G._stub_modules()
    sys.path.insert(0, G.REF)
    try:
        import train_2d as ref2d        # the reference's module: cos_loss
    finally:
        sys.path.remove(G.REF)
    torch.set_num_threads(8)
    random.seed(0)                      # cos_loss draws randint(0, 0): nothing depends on it
    sd = V.build_state()
    vals, per_batch, max_abs_diff, max_map, min_norm, max_feat = run(sd, ref2d, torch.float64)
    vals32 = run(sd, ref2d, torch.float32)[0]
    f32_gap = max(abs(vals[k] - vals32[k]) for k in KEYS)
    total = total_of(vals, V.EPOCH)
    widths = list(O2.DECODER_CHANNELS)
    cos_bound, rs = [], []
    for k in range(NS):
        r = FEAT_TOL_F32 * math.sqrt(widths[k]) / min_norm[k]
        assert r < 0.5, (k, r)
        rs.append(r)
        cos_bound.append(2.0 * r / (1.0 - r))
    d = FEAT_TOL_F32 * max_map
    mse_bound = 2.0 * max_abs_diff * d + d * d
    fx = OrderedDict()
    fx["meta/size"], fx["meta/local"], fx["meta/state_seed"], fx["meta/state_batch_seeds"] = np.int64(V.SIZE), np.int64(V.LOCAL), np.int64(V.SEED), np.array(V.STATE_SEEDS)
    fx["meta/seeds"], fx["meta/sizes"], fx["meta/epoch"] = np.array(V.BATCH_SEEDS), np.array(V.BATCH_SIZES), np.int64(V.EPOCH)
    fx["state_digest"] = V.state_digest(sd)
    fx["keys"] = np.array(KEYS)
    fx["values"] = np.array([vals[k] for k in KEYS], dtype=np.float64)
    fx["total"] = np.float64(total)
    fx["per_batch"] = np.array(per_batch, dtype=np.float64)
    fx["max_abs_diff"], fx["max_map_entry"] = np.float64(max_abs_diff), np.float64(max_map)
    fx["feat_widths"], fx["min_feat_norm"], fx["max_feat_entry"] = np.array(widths), np.array(min_norm, dtype=np.float64), np.array(max_feat, dtype=np.float64)
    fx["feat_tol_f32"], fx["cos_bound_f32"], fx["mse_bound_f32"] = np.float64(FEAT_TOL_F32), np.array(cos_bound, dtype=np.float64), np.float64(mse_bound)
    fx["f32_oracle_gap"] = np.float64(f32_gap)
    os.makedirs(G.OUT, exist_ok=True)
    np.savez_compressed(os.path.join(G.OUT, TAG + ".npz"), **fx)
    for k in KEYS:
        print(f"{k:12s} {vals[k]:.9f}")
    print(f"total        {total:.9f}   (n = {sum(V.BATCH_SIZES)})")
    print(f"max|pred - gt| = {max_abs_diff:.6f}, largest map entry {max_map:.4f} -> MSE bound {mse_bound:.3e}")
    print(f"smallest feature norms {min_norm}; largest entries {max_feat}; r {rs}; float32 cosine bounds {cos_bound}")
    print(f"float32 oracle vs float64 oracle: largest metric difference {f32_gap:.3e}")
    print(f"[{TAG}] wrote fixture")


if __name__ == "__main__":
    main()
