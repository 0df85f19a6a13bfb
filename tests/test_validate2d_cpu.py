"""CPU: the surface of 2D held-out validation -- new C-ABI entry points and the host-only route query, the command-line flags, the 2D training
loop's use of the 'eval' loader and the best-checkpoint rule (stand-in model / step / validate: no GPU here), the held-out chest loader and the
chest augmentation's reset."""
import ctypes
import os
import sys
import types
from collections import Counter

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import val2d_state as V  # noqa: E402

NEW_SYMBOLS = ("pcrl_conv2d_fwd_affine", "pcrl_conv2d_fwd_affine_fused", "pcrl_val2d_metrics", "pcrl_val2d_metrics_ws_bytes")
BF16, F32 = 1, 0


def test_library_exports_the_2d_inference_and_validation_entry_points():
    from pcrlv2_amd import _lib
    protos = _lib.parse_header()
    cdll = ctypes.CDLL(_lib.LIBPATH)
    for name in NEW_SYMBOLS:
        assert name in protos, f"{name} not declared in include/pcrl_hip.h"
        assert hasattr(cdll, name), f"{name} not exported"
    args = protos["pcrl_conv2d_fwd_affine"][1]
    assert [n for _, n in args[:7]] == ["x", "wp", "bias", "scale", "shift", "residual", "a"] and args[-3][1] == "act"
    assert protos["pcrl_val2d_metrics"][1][5] == ("double*", "acc")


# routes of the ResNet-18 U-Net's Conv2d + BatchNorm2d layers (val2d_state.model_layers), bf16: kernel family counts (0 gather, 1 4x8x8 brick, 2 narrow,
# 3 wide brick) and the layers pcrl_conv2d_fwd_affine_fused answers 0 for -- (Ci, Co, up, input side, residual); the same at b = 4 and b = 64
ROUTES = {
    64: ({0: 16, 1: 8, 3: 6, 2: 5}, {(64, 64, 0, 16, 1)}),
    96: ({0: 22, 1: 8, 2: 3, 3: 2}, set()),
    224: ({0: 22, 1: 8, 2: 3, 3: 2}, set()),
    512: ({3: 19, 0: 7, 2: 5, 1: 4}, {(64, 64, 0, 128, 1), (128, 128, 0, 64, 1), (256, 256, 0, 32, 1), (512, 512, 0, 16, 1)}),
}


@pytest.mark.parametrize("b", [4, 64])
@pytest.mark.parametrize("side", sorted(ROUTES))
def test_affine_fused_query_answers_through_the_route(side, b):
    """pcrl_conv2d_fwd_affine_fused, host only: 1 on the gather, narrow and 4x8x8-brick routes and on the wide-brick route without a residual, 0 for a
    wide-brick layer with a residual -- and it IS the route pcrl_conv2d_fwd_kind reports.  float32 runs the gather kernel only."""
    from pcrlv2_amd import _lib
    L = _lib.lib()
    kinds, unfused = Counter(), set()
    for Ci, Co, K, s, p, up, H, _bias, res, _relu in V.model_layers(side):
        kind = L.call("pcrl_conv2d_fwd_kind", b, H, H, Ci, Co, K, K, s, p, up, 0, BF16)
        fused = L.call("pcrl_conv2d_fwd_affine_fused", b, H, H, Ci, Co, K, K, s, p, up, int(res), BF16)
        assert fused == int(kind != 3 or not res), (side, b, Ci, Co, K, s, up, H, res, kind, fused)
        kinds[kind] += 1
        if not fused:
            unfused.add((Ci, Co, up, H, int(res)))
        assert L.call("pcrl_conv2d_fwd_kind", b, H, H, Ci, Co, K, K, s, p, up, 0, F32) == 0
        assert L.call("pcrl_conv2d_fwd_affine_fused", b, H, H, Ci, Co, K, K, s, p, up, int(res), F32) == 1
    assert dict(kinds) == ROUTES[side][0] and unfused == ROUTES[side][1], (dict(kinds), unfused)


def test_affine_entry_point_rejects_what_it_cannot_compute():
    from pcrlv2_amd import _lib
    L = _lib.lib()
    assert L.call("pcrl_conv2d_fwd_affine_fused", 0, 16, 16, 64, 64, 3, 3, 1, 1, 0, 0, BF16) == 0
    with pytest.raises(_lib.PcrlError, match="ReLU or none"):
        L.call("pcrl_conv2d_fwd_affine", 16, 16, None, 16, 16, None, 16, 4, 16, 16, 64, 64, 3, 3, 1, 1, 0, 2, BF16, None)       # sigmoid
    with pytest.raises(_lib.PcrlError, match="null pointer"):
        L.call("pcrl_conv2d_fwd_affine", 16, 16, None, None, 16, None, 16, 4, 16, 16, 64, 64, 3, 3, 1, 1, 0, 1, BF16, None)
    R = 4 * 26
    assert L.call("pcrl_val2d_metrics_ws_bytes", 4, 64, 64, 6) == ((4 * 64 * 64 // 1024) * 6 + 5 * R) * 8
    with pytest.raises(_lib.PcrlError, match="multiples of 16"):
        L.call("pcrl_val2d_metrics", 16, 16, 16, 16, 16, 16, 16, 1 << 20, 4, 24, 24, 6, 1e-8, None)


def test_parser_has_the_2d_validation_flags():
    from pcrlv2_amd import main as M
    a = M.build_parser().parse_args(["--d", "2"])
    assert a.val_every == 0 and a.save_best is False and a.val_list == "./train_val_txt/chest_valid.txt"
    a = M.build_parser().parse_args(["--d", "2", "--val_every", "5", "--save_best", "--val_list", "lists/held_out.txt"])
    assert a.val_every == 5 and a.save_best is True and a.val_list == "lists/held_out.txt"
    text = M.build_parser().format_help()
    assert "only with --d 3: held-out" not in text


class _Enc(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(3))


class _Net(torch.nn.Module):
    """Stand-in for PCRLv2: .model.encoder is what the 2D checkpoint layout saves."""

    def __init__(self, encoder_weights=None):
        super().__init__()
        self.model = torch.nn.Module()
        self.model.encoder = _Enc()
        self.head = torch.nn.Parameter(torch.zeros(2))

    def cuda(self, *a, **k):
        return self

    def set_compute_dtype(self, dt):
        return self

    def flush_counters(self):
        pass


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
    from pcrlv2_amd import config, train_2d as T
    monkeypatch.setattr(T, "PCRLv2", _Net)
    monkeypatch.setattr(T, "FusedSGD", _Opt)
    monkeypatch.setattr(T, "MSELoss2d", _Crit)
    monkeypatch.setattr(T, "CosineSimilarityMean", _Crit)
    monkeypatch.setattr(config, "EMPTY_CACHE_PER_EPOCH", False)
    epochs_run = []
    monkeypatch.setattr(T, "train_pcrlv2_inner", lambda args, epoch, loader, model, opt, crit, cos, verbose=True: epochs_run.append((epoch, loader)))
    args = types.SimpleNamespace(lr=1e-3, momentum=0.9, weight_decay=1e-4, epochs=5, output=str(tmp_path), model="pcrlv2", n="chest", phase="pretask", ratio=0.8,
                                 seed=1, amp=False, resume="", encoder_weights="", lr_decay_epochs=None, **kw)
    return T, args, epochs_run


def test_val_every_0_never_touches_the_eval_loader_2d(monkeypatch, tmp_path):
    T, args, epochs_run = _stub_loop(monkeypatch, tmp_path, val_every=0, save_best=True)
    monkeypatch.setattr(T, "validate", lambda *a, **k: pytest.fail("validate called with --val_every 0"))
    loaders = _Loaders()
    T._train_pcrlv2(args, loaders, False)
    assert [e for e, _ in epochs_run] == [0, 1, 2, 3, 4, 5] and loaders.eval_reads == 0
    assert not [f for f in os.listdir(tmp_path) if f.endswith("_best.pt")]
    # a namespace without the flags (callers of the library entry point that predate them) behaves the same
    del args.val_every, args.save_best
    T._train_pcrlv2(args, loaders, False)
    assert loaders.eval_reads == 0


def test_val_every_and_the_best_checkpoint_rule_2d(monkeypatch, tmp_path, capsys):
    """--val_every 2 over epochs 0..5: validate after epochs 1, 3 and 5 on data_loader['eval']; --save_best writes
    <model>_<n>_<phase>_<ratio>_best.pt in the 2D checkpoint layout (the ENCODER's state_dict) + 'val' on STRICT improvement of `total` only."""
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
    T._train_pcrlv2(args, loaders, False)
    assert calls == [("EVAL", 1), ("EVAL", 3), ("EVAL", 5)] and loaders.eval_reads == 3
    best = os.path.join(str(tmp_path), "pcrlv2_chest_pretask_0.8_best.pt")
    assert [(p, e) for p, e in saved if p.endswith("_best.pt")] == [(best, 1), (best, 5)]       # 0.5 (first), not 0.5 again, then 0.25
    ck = torch.load(best, map_location="cpu", weights_only=False)
    assert set(ck) == {"opt", "state_dict", "optimizer", "epoch", "val"} and ck["epoch"] == 5 and ck["val"]["total"] == 0.25 and ck["val"]["n"] == 11
    assert list(ck["state_dict"]) == ["w"]                                                      # the encoder only: train_2d.py:96-107
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Val: [")]
    assert len(lines) == 3 and lines[0].startswith("Val: [1]\ttotal 0.5000\tmg ") and "cos " in lines[0] and "local " in lines[0] and "mid " in lines[0]
    # without --save_best nothing is written
    T2, args2, _ = _stub_loop(monkeypatch, tmp_path / "other", val_every=3, save_best=False)
    os.makedirs(args2.output)
    totals = iter([0.1, 0.05])
    T2._train_pcrlv2(args2, _Loaders(), False)
    assert not [f for f in os.listdir(args2.output) if f.endswith("_best.pt")]


def test_val_total_2d_is_the_expected_training_loss():
    from pcrlv2_amd import train_2d as T
    assert len(T.VAL_KEYS) == 16 and T.VAL_KEYS[0] == "mse_out" and T.VAL_KEYS[1] == "mse_mid0" and T.VAL_KEYS[6] == "cos_global0" and T.VAL_KEYS[11] == "cos_local0"
    m = dict(mse_out=1.0)
    for k in range(5):
        m[f"mse_mid{k}"], m[f"cos_global{k}"], m[f"cos_local{k}"] = 3.0 * (k + 1), -0.1 * (k + 1), 0.05 * (k + 1)
    assert T.val_total(m, 0) == pytest.approx(1.0 - 0.3 + 0.15 + 1.0 * 9.0, abs=1e-12)
    assert T.val_total(m, 120) == pytest.approx(1.0 - 0.3 + 0.15 + 0.5 * 9.0, abs=1e-12)
    assert T.val_total(m, 240) == pytest.approx(1.0 - 0.3 + 0.15, abs=1e-12)


def test_held_out_chest_loader_is_lazy_sharded_and_needs_its_list(tmp_path, monkeypatch):
    from test_chest_data_cpu import _write_pngs
    from pcrlv2_amd import data as D, data_chest as DC
    d = tmp_path / "data"
    d.mkdir()
    names = _write_pngs(str(d), 12)
    (tmp_path / "lists").mkdir()
    held = tmp_path / "lists" / "held_out.txt"
    held.write_text("".join(f"{n} 0 1\n" for n in names[7:]))           # five held-out images; `name label...` lines
    train_list = tmp_path / "train_val_txt"
    train_list.mkdir()
    (train_list / "chest_train.txt").write_text("".join(f"{n} 0\n" for n in names[:7]))
    monkeypatch.chdir(tmp_path)
    built = []
    monkeypatch.setattr(DC, "AugmentedLoader", lambda files, b, workers, device, shuffle=True, seed=0, drop_last=False, kind=None:
                        built.append((list(files), shuffle, seed)) or types.SimpleNamespace(files=list(files), shuffle=shuffle))
    valid = [str(d / n) for n in names[7:]]
    got = []
    for rank in range(2):
        monkeypatch.setenv("RANK", str(rank))
        monkeypatch.setenv("WORLD_SIZE", "2")
        args = types.SimpleNamespace(data=str(d), ratio=1.0, b=2, workers=0, seed=3, val_every=1, val_list=str(held))
        n0 = len(built)
        dl = DC.chest_pretask_loaders(args, device="cpu")
        assert isinstance(dl, D._LazyLoaders) and set(dl) == {"train", "eval"} and len(built) == n0 + 1           # the training loader only
        assert not set(dl["train"].files) & set(valid)                                                             # never carved out of the training list
        ev = dl["eval"]
        assert len(built) == n0 + 2 and dl["eval"] is ev and len(built) == n0 + 2                                  # built once, on first use
        assert ev is not dl["train"] and ev.shuffle is False and ev.sharded is True and built[-1][2] == 3
        got.append(ev.files)
    assert got == [D.eval_shard(valid, 0, 2), D.eval_shard(valid, 1, 2)] and got[0] + got[1] == valid and {len(g) for g in got} == {2, 3}
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setenv("RANK", "0")
    # a missing list is an error that says so; nothing is carved out of the training list instead
    with pytest.raises(SystemExit, match="no_such_list.txt"):
        DC.chest_pretask_loaders(types.SimpleNamespace(data=str(d), ratio=1.0, b=2, workers=0, seed=3, val_every=1, val_list=str(tmp_path / "no_such_list.txt")), device="cpu")
    # --val_every 0 (or args that predate the flag): the reference's dict, 'eval' IS the training loader and no list is looked for
    for args in (types.SimpleNamespace(data=str(d), ratio=1.0, b=2, workers=0, seed=3, val_every=0, val_list=str(tmp_path / "no_such_list.txt")),
                 types.SimpleNamespace(data=str(d), ratio=1.0, b=2, workers=0, seed=3)):
        dl = DC.chest_pretask_loaders(args, device="cpu")
        assert type(dl) is dict and dl["eval"] is dl["train"]


def test_synthetic_2d_eval_loader_is_a_second_stream(monkeypatch):
    from pcrlv2_amd import main as M
    made = []
    monkeypatch.setattr(M.SyntheticChestLoader, "__init__", lambda self, b, steps, size, seed=0, device=None: made.append(seed))
    monkeypatch.delenv("RANK", raising=False)
    dl = M.get_dataloader(M.build_parser().parse_args(["--data", "synthetic", "--d", "2", "--seed", "5"]))
    assert made == [5] and dl["eval"] is None and set(dl) == {"train", "eval"}                 # --val_every 0: unchanged
    made.clear()
    monkeypatch.setenv("RANK", "1")
    dl = M.get_dataloader(M.build_parser().parse_args(["--data", "synthetic", "--d", "2", "--seed", "5", "--val_every", "1"]))
    assert sorted(made) == [6, 5 + 7919 + 1] and dl["eval"] is not None and dl["eval"].sharded is True and dl["eval"] is not dl["train"]


def test_chest_augment_reset_reproduces_the_draw_records():
    """AugmentedLoader.reset_rng reaches GpuChestAugment's numpy Generator (it used to reset only `gen` / `host_rng`, which the chest augmentation
    does not have: a chest validation pass did not repeat); the LUNA augmentation's reset is what it was."""
    from pcrlv2_amd import data as D, data_chest as DC
    aug = object.__new__(DC.GpuChestAugment)            # the constructor wants a GPU; the draws are host arithmetic
    aug.rng = np.random.default_rng(11)
    dims = np.array([[64, 48, 1], [40, 72, 3], [64, 64, 1]])
    loader = object.__new__(D.AugmentedLoader)
    loader.augment, loader.seed = aug, 11
    first = [aug.draw(dims)[0] for _ in range(2)]
    assert not np.array_equal(first[0], first[1])
    loader.reset_rng()
    again = [aug.draw(dims)[0] for _ in range(2)]
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    # LUNA-style augmentation (a device generator and a host companion, no reset of its own): unchanged behaviour
    calls = []
    luna = types.SimpleNamespace(gen=types.SimpleNamespace(manual_seed=lambda s: calls.append(("gen", s))),
                                 host_rng=types.SimpleNamespace(seed=lambda s: calls.append(("host", s))))
    loader.augment, loader.seed = luna, 7
    loader.reset_rng()
    assert calls == [("gen", 7), ("host", 7)]


def test_fixture_state_recipe_matches_its_digest():
    """tests/golden/val2d_b4_64.npz stores a digest of the state the GPU test rebuilds without the reference."""
    fx = np.load(os.path.join(ROOT, "tests", "golden", "val2d_b4_64.npz"))
    sd = V.build_state()
    np.testing.assert_allclose(V.state_digest(sd), fx["state_digest"], rtol=1e-6, atol=1e-9)
    assert tuple(int(v) for v in fx["meta/sizes"]) == V.BATCH_SIZES and tuple(int(v) for v in fx["meta/seeds"]) == V.BATCH_SEEDS
    assert float(fx["f32_oracle_gap"]) < 1e-6 and all(0 < float(c) < 5e-3 for c in fx["cos_bound_f32"])
