"""The recorded number of DESIGN.md section 21: tools/seg_sw_dice.py's short phantom run (`seg3d.py train --data synthetic`, five epochs of 20 steps,
crop 32 x 32 x 16, bf16), then the validation and test Dice of the SAME weights by blended sliding windows (overlap 0.5, Gaussian) un-mirrored, with
mirror `z` and with mirror `all` -- one JSON line per split.  A record of one run, not an assertion.

    python tools/seg_tta_dice.py
"""
import json
import os
import subprocess
import sys
import tempfile
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
out = tempfile.mkdtemp(prefix="seg_tta_dice_")
argv = ["train", "--data", "synthetic", "--phase", "scratch", "--n_class", "3", "--crop", "32,32,16", "--b", "4", "--epochs", "5", "--steps_per_epoch", "20", "--amp",
        "--output", out]
r = subprocess.run([sys.executable, os.path.join(ROOT, "seg3d.py"), *argv], cwd=ROOT, capture_output=True, text=True, timeout=280)
print("\n".join(ln for ln in r.stdout.splitlines() if ln.startswith(("Val:", "Test:"))))
if r.returncode:
    print(r.stdout[-2000:], r.stderr[-2000:])
    sys.exit(r.returncode)
from pcrlv2_amd import data_seg as D  # noqa: E402
from pcrlv2_amd.train_seg import evaluate_sliding, load_segmenter  # noqa: E402
ckpt = [f for f in os.listdir(out) if f.endswith(".pt")]
last = max(ckpt, key=lambda f: int(f[:-3].rsplit("_", 1)[1]))       # pcrlv2_seg3d_scratch_1.0_<epoch>.pt: the last epoch's weights
print(last)
model = load_segmenter(os.path.join(out, last), torch.device("cuda"), amp=True)
crop = (32, 32, 16)
args = types.SimpleNamespace(crop="32,32,16", n_class=3, in_channels=1, data="synthetic", seed=42, steps_per_epoch=20, b=4)
L = D.loaders(args)
for split in ("eval", "test"):
    cases = L[split].cases
    rec = {"split": split}
    for mirror in ("none", "z", "all"):
        rec[f"gaussian_0.5_mirror_{mirror}"] = evaluate_sliding(model, cases, crop, 4, 0.5, "gaussian", mirror=D.parse_mirror(mirror))
    print(json.dumps(rec))
