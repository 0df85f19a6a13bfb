"""The deterministic 2D model state and batches behind tests/golden/val2d_b4_64.npz -- shared by tools/make_val2d_fixtures.py (CPU, float64, with the
reference's loss code) and tests/test_validate2d_gpu.py (which rebuilds the state WITHOUT the reference and checks it against the fixture's digest).

State: PCRLv2() initialised on the CPU under torch.manual_seed(5) with the non-trivial affine parameters of tests/test_model2d_gpu._build, then two
training-mode forwards of the float64 2D oracle (view 1 of O2.synthetic_batch(4, 64, 32, seed=40 / 41)) move every BatchNorm's running statistics;
the result is rounded to float32 -- what a GPU model holds after load_state_dict -- so the oracle and the engine start from the same numbers.
(The 2D MODEL is parity-unpinned -- smp / torchvision are absent, the oracle is a restatement: the fixture pins the metric assembly and the
draw-free expectation, not the network.)"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))

SEED, SIZE, LOCAL, STATE_B, STATE_SEEDS = 5, 64, 32, 4, (40, 41)
BATCH_SEEDS, BATCH_SIZES, EPOCH = (77, 78, 79), (4, 4, 3), 0


def build_state():
    """-> OrderedDict name -> CPU tensor (floating entries float32-representable float64; counters as they are)."""
    import pcrlv2_2d_oracle as O2
    from pcrlv2_amd.models import PCRLv2
    rng = torch.random.get_rng_state()
    try:
        torch.manual_seed(SEED)
        model = PCRLv2()
        g = torch.Generator().manual_seed(SEED + 1)
        with torch.no_grad():
            for n, p in model.named_parameters():
                if p.dim() == 1:
                    p.copy_(torch.rand(p.shape, generator=g) * 0.5 + (0.75 if n.endswith("weight") else -0.25))
    finally:
        torch.random.set_rng_state(rng)
    sd = {k: (v.detach().double() if v.is_floating_point() else v.clone()) for k, v in torch.nn.Module.state_dict(model).items()}
    with torch.no_grad(), torch.backends.mkldnn.flags(enabled=False):
        for s in STATE_SEEDS:
            so = {}
            O2.model_forward(O2.synthetic_batch(STATE_B, SIZE, LOCAL, seed=s, dtype=torch.float64)[0], sd, so=so)
            sd.update(so)
    return {k: (v.float().double() if v.is_floating_point() else v) for k, v in sd.items()}


def state_digest(sd):
    """float64 [n, 2]: (sum, sum of magnitudes) of every floating tensor in key order -- compared with a relative tolerance (the oracle's float64
    convolutions may differ in the last bits between CPUs before the rounding to float32)."""
    return np.array([[float(v.double().sum()), float(v.double().abs().sum())] for k, v in sorted(sd.items()) if v.is_floating_point()], dtype=np.float64)


def batches(dtype=torch.float32):
    import pcrlv2_2d_oracle as O2
    return [O2.synthetic_batch(b, SIZE, LOCAL, seed=s, dtype=dtype) for s, b in zip(BATCH_SEEDS, BATCH_SIZES)]


def model_layers(side):
    """Every Conv2d that sits in front of a BatchNorm2d in the ResNet-18 U-Net (models/pcrlv2_model.py) for a side x side input, as the engine calls
    it: (Ci as stored, Co, K, stride, pad, up, input side, bias, residual, relu).  The stem's 3 channels are stored zero-padded to 8."""
    out = [(8, 64, 7, 2, 3, 0, side, False, False, True)]
    h, cin = side // 4, 64
    for planes, stride in ((64, 1), (128, 2), (256, 2), (512, 2)):
        for blk in range(2):
            s = stride if blk == 0 else 1
            out.append((cin, planes, 3, s, 1, 0, h, False, False, True))                 # conv1 + bn1 + relu
            if s != 1 or cin != planes:
                out.append((cin, planes, 1, s, 0, 0, h, False, False, False))            # downsample
            h //= s
            out.append((planes, planes, 3, 1, 1, 0, h, False, True, True))               # conv2 + bn2 + identity + relu
            cin = planes
    for cout in (256, 128, 64, 32, 16):
        out.append((cin, cout, 3, 1, 1, 1, h, False, False, True))                       # decoder conv1 behind the nearest x2 upsample
        h *= 2
        out.append((cout, cout, 3, 1, 1, 0, h, False, False, True))                      # decoder conv2
        out.append((cout, cout, 3, 1, 1, 0, h, True, False, True))                       # deep-supervision head conv (bias) + bn + relu
        cin = cout
    return out
