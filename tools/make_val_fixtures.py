"""Writes tests/golden/val_b4_32x32x16.npz: one held-out validation pass (train_3d.validate's metrics) computed by the REAL reference.

    python tools/make_val_fixtures.py

Needs the reference checkout that oracle/make_golden.py loads (its `load_reference`); runs on the CPU in float64, oneDNN off.  The reference's own
model class in .eval(), its own `cos_loss` (called on one-scale lists, so that its `random.randint(0, 0)` picks the scale we ask for), torch's
MSELoss / CosineSimilarity as train_3d.py:56-57 builds them.  State: the oracle's deterministic initial state moved by one oracle training step
(oracle/make_golden.py make_eval's recipe -- batch seed 31 -- with a 4-sample batch); data: O.fill_batch seeds 77, 78, 79 with 4, 4 and 3 samples; epoch 0.
The deterministic oracle's eval forward is asserted equal to the reference's on every batch, so the tests can rebuild the state without the
reference.

Besides the eleven float64 values the fixture stores what the test's bounds are derived from (nothing measured on the engine):
  max_abs_diff   max |prediction - gt| over the four maps and all batches: an engine whose maps are within d of the reference's has every MSE
                 metric within 2 * max_abs_diff * d + d^2
  cos_bound_f32  per scale k: with every feature element within e = 2e-4 of the reference's (the float32 feature bound of
                 test_eval_mode_forward_matches_reference_golden), a feature vector of C_k elements moves by at most r = e sqrt(C_k) / |x| relative to
                 its norm, its direction by at most r / (1 - r), and a cosine of two such vectors by at most the sum of the two: the bound uses the
                 SMALLEST feature norm of the scale; every cosine metric is an average of cosines with total weight one.
"""
import math
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_golden as G  # noqa: E402
import pcrlv2_oracle as O  # noqa: E402

TAG, DHW, STATE_B, STATE_SEED, SEEDS, SIZES, EPOCH = "val_b4_32x32x16", (32, 32, 16), 4, 31, (77, 78, 79), (4, 4, 3), 0
FEAT_TOL_F32 = 2e-4
KEYS = ("mse_out", "mse_mid0", "mse_mid1", "mse_mid2", "cos_global0", "cos_global1", "cos_global2", "cos_local0", "cos_local1", "cos_local2")


def batch_metrics(ref_train, criterion, cosine, out1, masks1, gt, feats1, feats2, feats_loc, nlocal):
    """The ten batch means, each term through the reference's own loss code at a fixed scale index."""
    b = out1.shape[0]
    m = OrderedDict(mse_out=criterion(out1, gt))
    for k in range(3):
        m[f"mse_mid{k}"] = criterion(masks1[k], gt)
    for k in range(3):
        m[f"cos_global{k}"] = ref_train.cos_loss(cosine, [feats1[k]], [feats2[k]])[0]
    for k in range(3):
        stacked = torch.stack(feats_loc[k])                    # train_3d.py:124
        local = 0.0
        for i in range(nlocal):                                # train_3d.py:127-134 at index k
            crop = [stacked[:, b * i: b * (i + 1)]]
            local = local + ref_train.cos_loss(cosine, [feats1[k]], crop)[0] + ref_train.cos_loss(cosine, [feats2[k]], crop)[0]
        m[f"cos_local{k}"] = local / (2 * nlocal)
    return OrderedDict((k, float(v)) for k, v in m.items())


def main():
    refmod, ref_train, _ref_utils = G.load_reference()
    dt = torch.float64
    criterion, cosine = torch.nn.MSELoss(), torch.nn.CosineSimilarity()
    sums = OrderedDict((k, 0.0) for k in KEYS)
    per_batch, max_abs_diff, min_norm = [], 0.0, [math.inf] * 3
    with torch.backends.mkldnn.flags(enabled=False), torch.no_grad():
        with torch.enable_grad():
            st1, _, _, _ = O.train_steps(O.fill_state(dt), [O.fill_batch(STATE_B, DHW, dtype=dt, seed=STATE_SEED)], 0, 1e-3, 240, 0)
        st1 = {k: v.detach() for k, v in st1.items()}
        model = refmod.PCRLv23d().double()
        model.load_state_dict(st1, strict=True)
        model.eval()
        for seed, b in zip(SEEDS, SIZES):
            x1, x2, gt, _gt2, local_views = O.fill_batch(b, DHW, dtype=dt, seed=seed)
            loc = torch.cat(local_views, dim=0)
            out1, feats1, masks1 = model(x1)
            _, feats2, _ = model(x2)
            _, feats_loc, masks_loc = model(loc, local=True)
            assert masks_loc == []
            for x, local, got in ((x1, False, (out1, feats1, masks1)), (x2, False, (None, feats2, None)), (loc, True, (None, feats_loc, None))):
                o_out, o_feats, o_masks = O.forward(st1, x, local=local, training=False)
                if got[0] is not None:
                    G.close(o_out, got[0], 1e-10, "val out")
                    for i in range(3):
                        G.close(o_masks[i], got[2][i], 1e-10, f"val mask{i}")
                for i in range(3):
                    G.close(o_feats[i][0], got[1][i][0], 1e-9, f"val pro{i}")
                    G.close(o_feats[i][1], got[1][i][1], 1e-9, f"val pre{i}")
            m = batch_metrics(ref_train, criterion, cosine, out1, masks1, gt, feats1, feats2, feats_loc, len(local_views))
            per_batch.append([m[k] for k in KEYS])
            for k in KEYS:
                sums[k] += b * m[k]
            max_abs_diff = max(max_abs_diff, *(float((t - gt).abs().max()) for t in (out1, *masks1)))
            for k in range(3):
                for fs in (feats1, feats2, feats_loc):
                    for t in fs[k]:
                        min_norm[k] = min(min_norm[k], float(t.norm(dim=1).min()))
    n = sum(SIZES)
    vals = OrderedDict((k, sums[k] / n) for k in KEYS)
    mean3 = lambda name: sum(vals[name + str(k)] for k in range(3)) / 3.0
    beta = 0.5 * (1.0 + math.cos(math.pi * EPOCH / 240))
    total = vals["mse_out"] + mean3("cos_global") + mean3("cos_local") + beta * mean3("mse_mid")
    widths = [int(model.up_tr256.bn.num_features), int(model.up_tr128.bn.num_features), int(model.up_tr64.bn.num_features)]
    cos_bound = []
    for k in range(3):
        r = FEAT_TOL_F32 * math.sqrt(widths[k]) / min_norm[k]
        assert r < 0.5, (k, r)
        cos_bound.append(2.0 * r / (1.0 - r))
    fx = OrderedDict()
    fx["meta/dhw"], fx["meta/state_b"], fx["meta/state_batch_seed"] = np.array(DHW), np.int64(STATE_B), np.int64(STATE_SEED)
    fx["meta/seeds"], fx["meta/sizes"], fx["meta/epoch"] = np.array(SEEDS), np.array(SIZES), np.int64(EPOCH)
    fx["keys"] = np.array(KEYS)
    fx["values"] = np.array([vals[k] for k in KEYS], dtype=np.float64)
    fx["total"] = np.float64(total)
    fx["per_batch"] = np.array(per_batch, dtype=np.float64)
    fx["max_abs_diff"] = np.float64(max_abs_diff)
    fx["feat_widths"], fx["min_feat_norm"] = np.array(widths), np.array(min_norm, dtype=np.float64)
    fx["feat_tol_f32"], fx["cos_bound_f32"] = np.float64(FEAT_TOL_F32), np.array(cos_bound, dtype=np.float64)
    np.savez_compressed(os.path.join(G.OUT, TAG + ".npz"), **fx)
    for k in KEYS:
        print(f"{k:12s} {vals[k]:.9f}")
    print(f"total        {total:.9f}   (n = {n}, beta = {beta})")
    print(f"max|pred - gt| = {max_abs_diff:.6f}; smallest feature norms {min_norm}; float32 cosine bounds {cos_bound}")
    print(f"[{TAG}] oracle eval == reference eval on every batch; wrote fixture")


if __name__ == "__main__":
    main()
