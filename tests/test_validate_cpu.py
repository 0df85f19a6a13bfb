"""CPU: the surface of held-out validation -- new C-ABI entry points, the host-only route queries, the command-line flags, the training loop's
use of the 'eval' loader and the best-checkpoint rule (stand-in model / step / validate: no GPU here), and the validation file shards."""
import ctypes
import os
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pcrl_conv3d_k3_fwd_affine", "pcrl_conv3d_k3_fwd_affine_ws_bytes", "pcrl_conv3d_k3_fwd_affine_fused", "pcrl_conv3d_k3_c1_fwd_affine",
               "pcrl_val_metrics", "pcrl_val_metrics_ws_bytes")


def test_library_exports_the_inference_and_validation_entry_points():
    from pcrlv2_amd import _lib
    protos = _lib.parse_header()
    cdll = ctypes.CDLL(_lib.LIBPATH)
    for name in NEW_SYMBOLS:
        assert name in protos, f"{name} not declared in include/pcrl_hip.h"
        assert hasattr(cdll, name), f"{name} not exported"
    assert [t for t, _ in protos["pcrl_conv3d_k3_fwd_affine"][1]].count("const float*") == 3       # bias, scale, shift
    assert protos["pcrl_val_metrics"][1][23] == ("double*", "acc")


def test_route_queries_answer_without_a_gpu():
    """pcrl_conv3d_k3_fwd_affine_fused: 1 for the layers that carry the bytes (full and half resolution, b = 32 / 64x64x32 and b = 8 / 128x128x64,
    bf16 and float32), 0 where the unfused convolution runs on a family without the epilogue; `_ws_bytes` answers too."""
    from pcrlv2_amd import _lib
    L = _lib.lib()
    fused = lambda *a: L.call("pcrl_conv3d_k3_fwd_affine_fused", *a)
    for dt in (0, 1):
        for N, (D, H, W) in ((32, (64, 64, 32)), (8, (128, 128, 64))):
            for Ci, Co in ((32, 64), (128, 64), (64, 64)):
                assert fused(N, D, H, W, Ci, Co, dt) == 1, (N, D, H, W, Ci, Co, dt)
            for Ci, Co in ((64, 64), (64, 128), (256, 128), (128, 128)):
                assert fused(N, D // 2, H // 2, W // 2, Ci, Co, dt) == 1, (N, Ci, Co, dt)
            assert L.call("pcrl_conv3d_k3_fwd_affine_ws_bytes", N, D, H, W, 64, 64, dt) == 0
    assert fused(32, 8, 8, 4, 256, 256, 1) == 0       # bf16 bottleneck level: the 4x8x8-brick kernel has no fused form
    assert fused(32, 8, 8, 4, 256, 256, 0) == 0       # float32: split-K
    assert fused(192, 2, 2, 2, 256, 256, 1) == 0      # voxel-major rows
    assert fused(32, 64, 64, 32, 48, 64, 1) == 0 and fused(0, 64, 64, 32, 64, 64, 1) == 0
    assert L.call("pcrl_val_metrics_ws_bytes", 4 * 32 * 32 * 16, 4, 6) == ((4 * 32 * 32 * 16 // 4096) * 4 + 3 * 4 * 26) * 8
    with pytest.raises(_lib.PcrlError, match="ReLU or none"):
        L.call("pcrl_conv3d_k3_fwd_affine", 16, 16, 16, 16, 16, 16, None, 0, 1, 8, 8, 16, 32, 32, 2, 1, None)


def test_parser_has_the_validation_flags():
    from pcrlv2_amd import main as M
    a = M.build_parser().parse_args([])
    assert a.val_every == 0 and a.save_best is False
    a = M.build_parser().parse_args(["--val_every", "5", "--save_best"])
    assert a.val_every == 5 and a.save_best is True


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(3))

    def cuda(self, *a, **k):
        return self

    def set_compute_dtype(self, dt):
        return self


class _Opt(torch.optim.SGD):
    def __init__(self, params, lr, momentum, weight_decay):
        super().__init__(params, lr=lr, momentum=momentum, weight_decay=weight_decay)


class _Crit:
    def cuda(self):
        return self


class _Loaders(dict):
    """{'train', 'eval'} that records who reads 'eval'."""

    def __init__(self):
        super().__init__(train=[0, 1], eval="EVAL")
        self.eval_reads = 0

    def __getitem__(self, k):
        if k == "eval":
            self.eval_reads += 1
        return super().__getitem__(k)


def _stub_loop(monkeypatch, tmp_path, **kw):
    from pcrlv2_amd import config, train_3d as T
    monkeypatch.setattr(T, "PCRLv23d", _Net)
    monkeypatch.setattr(T, "FusedSGD", _Opt)
    monkeypatch.setattr(T, "MSELoss", _Crit)
    monkeypatch.setattr(T, "CosineSimilarityMean", _Crit)
    monkeypatch.setattr(config, "EMPTY_CACHE_PER_EPOCH", False)
    epochs_run = []
    monkeypatch.setattr(T, "train_pcrlv2_inner", lambda args, epoch, loader, model, opt, crit, cos, verbose=True: epochs_run.append((epoch, loader)))
    args = types.SimpleNamespace(lr=1e-3, momentum=0.9, weight_decay=1e-4, epochs=5, output=str(tmp_path), model="pcrlv2", n="luna", phase="pretask", ratio=0.8,
                                 seed=1, amp=False, resume="", lr_decay_epochs=None, **kw)
    return T, args, epochs_run


def test_val_every_0_never_touches_the_eval_loader(monkeypatch, tmp_path):
    T, args, epochs_run = _stub_loop(monkeypatch, tmp_path, val_every=0, save_best=True)
    monkeypatch.setattr(T, "validate", lambda *a, **k: pytest.fail("validate called with --val_every 0"))
    loaders = _Loaders()
    T._train_pcrlv2_3d(args, loaders, False)
    assert [e for e, _ in epochs_run] == [0, 1, 2, 3, 4, 5] and loaders.eval_reads == 0
    assert not [f for f in os.listdir(tmp_path) if f.endswith("_best.pt")]
    # a namespace without the new flags (callers of the library entry point that predate them) behaves the same
    del args.val_every, args.save_best
    T._train_pcrlv2_3d(args, loaders, False)
    assert loaders.eval_reads == 0


def test_val_every_and_the_best_checkpoint_rule(monkeypatch, tmp_path, capsys):
    """--val_every 2 over epochs 0..5: validate after epochs 1, 3 and 5 on data_loader['eval']; --save_best writes
    <model>_<n>_<phase>_<ratio>_best.pt in the checkpoint layout + 'val' on STRICT improvement of `total` only."""
    T, args, _ = _stub_loop(monkeypatch, tmp_path, val_every=2, save_best=True)
    totals = iter([0.5, 0.5, 0.25])
    calls = []

    def fake_validate(model, loader, epoch, group=None):
        calls.append((loader, epoch))
        t = next(totals)
        out = {k: t / 4 for k in T.VAL_KEYS}
        out.update(total=t, n=11)
        return out

    monkeypatch.setattr(T, "validate", fake_validate)
    saved = []
    real_save = torch.save
    monkeypatch.setattr(torch, "save", lambda obj, path: (saved.append((path, obj["epoch"])), real_save(obj, path)))
    loaders = _Loaders()
    T._train_pcrlv2_3d(args, loaders, False)
    assert calls == [("EVAL", 1), ("EVAL", 3), ("EVAL", 5)] and loaders.eval_reads == 3
    best = os.path.join(str(tmp_path), "pcrlv2_luna_pretask_0.8_best.pt")
    assert [(p, e) for p, e in saved if p.endswith("_best.pt")] == [(best, 1), (best, 5)]       # 0.5 (first), not 0.5 again, then 0.25
    ck = torch.load(best, map_location="cpu", weights_only=False)
    assert set(ck) == {"opt", "state_dict", "optimizer", "epoch", "val"} and ck["epoch"] == 5 and ck["val"]["total"] == 0.25 and ck["val"]["n"] == 11
    assert list(ck["state_dict"]) == ["w"]
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Val: [")]
    assert len(lines) == 3 and lines[0].startswith("Val: [1]\ttotal 0.5000\tmg ") and "cos " in lines[0] and "local " in lines[0]
    # without --save_best nothing is written
    T2, args2, _ = _stub_loop(monkeypatch, tmp_path / "other", val_every=3, save_best=False)
    os.makedirs(args2.output)
    totals = iter([0.1, 0.05])
    T2._train_pcrlv2_3d(args2, _Loaders(), False)
    assert not [f for f in os.listdir(args2.output) if f.endswith("_best.pt")]


def test_val_total_is_the_expected_training_loss():
    from pcrlv2_amd import train_3d as T
    m = dict(mse_out=1.0, mse_mid0=3.0, mse_mid1=6.0, mse_mid2=9.0, cos_global0=-0.3, cos_global1=-0.6, cos_global2=-0.9, cos_local0=0.1, cos_local1=0.2, cos_local2=0.3)
    assert T.val_total(m, 0) == pytest.approx(1.0 - 0.6 + 0.2 + 1.0 * 6.0, abs=1e-12)
    assert T.val_total(m, 120) == pytest.approx(1.0 - 0.6 + 0.2 + 0.5 * 6.0, abs=1e-12)
    assert T.val_total(m, 240) == pytest.approx(1.0 - 0.6 + 0.2, abs=1e-12)


def test_validation_file_shards_are_disjoint_and_cover_folds_7_to_9(tmp_path, monkeypatch):
    from test_data_cpu import _make_tree
    from pcrlv2_amd import data as D
    _make_tree(tmp_path, series_per_fold=3, pairs=1)
    _, x_valid = D.luna_file_lists(str(tmp_path), 1.0, str(tmp_path / "no_list.txt"))
    assert len(x_valid) == 9 and {os.path.basename(os.path.dirname(p)) for p in x_valid} == {"subset7", "subset8", "subset9"}
    s0, s1 = D.eval_shard(x_valid, 0, 2), D.eval_shard(x_valid, 1, 2)
    assert s0 + s1 == x_valid and not set(s0) & set(s1) and {len(s0), len(s1)} == {4, 5}
    assert D.eval_shard(x_valid, 0, 1) == x_valid
    # the 'eval' loader of luna_pretask_loaders is this rank's shard, and it is not built until somebody asks for it
    built = []
    monkeypatch.setattr(D, "AugmentedLoader", lambda files, b, workers, device, shuffle=True, seed=0, drop_last=False: built.append(list(files)) or list(files))
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("WORLD_SIZE", "2")
    got = []
    for rank in range(2):
        monkeypatch.setenv("RANK", str(rank))
        loaders = D.luna_pretask_loaders(types.SimpleNamespace(data=str(tmp_path), ratio=1.0, b=2, workers=0, seed=0), device="cpu")
        assert set(loaders) == {"train", "eval"} and len(built) == 1 + 2 * rank          # the training loader only
        got.append(loaders["eval"])
        assert len(built) == 2 + 2 * rank and loaders["eval"] is got[-1] and len(built) == 2 + 2 * rank      # built once
    assert got == [s0, s1]


def test_synthetic_eval_loader_is_a_second_stream(monkeypatch):
    from pcrlv2_amd import main as M
    made = []
    monkeypatch.setattr(M.SyntheticLunaLoader, "__init__", lambda self, b, steps, seed=0, device=None: made.append(seed))
    monkeypatch.delenv("RANK", raising=False)
    dl = M.get_dataloader(M.build_parser().parse_args(["--data", "synthetic", "--seed", "5", "--val_every", "1"]))
    assert made[0] != made[1] and 5 in made and dl["eval"] is not None and dl["eval"].sharded is True and set(dl) == {"train", "eval"}
