"""PCRLv23d on the MI355X engine -- drop-in for the reference's models/pcrlv2_model_3d.py.

Same public classes, constructor arguments, forward signatures, return tuples, attribute names and state_dict
(169 entries in the same order); the arithmetic runs in libpcrl_hip.so (hand-written gfx950 kernels)
through `pcrlv2_amd.functions`.  torch.nn layers appear here ONLY as parameter containers: they provide the reference's
parameter names / shapes / default initialisation (so an identical `torch.manual_seed` yields identical initial
weights); their forward() is never called.  There is no CPU / eager fallback: non-GPU inputs raise.
`model.eval()` runs the same kernels on the running statistics (inference; `_forward_eval`).

Constructor variants the reference accepts but train_3d.py:45 never instantiates -- act in {'elu','prelu'}, norm='in',
in_channels != 1, n_class != 1 (models/pcrlv2_model_3d.py:15-16,22-25,98) -- run on the same library through general-purpose routes
(ELU as an activation code of the fused BatchNorm kernels; PReLU as a streaming pass behind the normalisation; InstanceNorm3d as
GroupNorm with one channel per group; the first layer zero-padded to 32 input channels; one C -> 1 pass per output class) and are
pinned against the real reference built with the same arguments (tests/golden/v_*.npz, tests/test_variants_gpu.py).  They are not
tuned: the pre-training path is PCRLv23d() with its defaults.  norm='gn' crashes in the reference; here it is the optional
GroupNorm + SiLU mode described below.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import config, functions as Fn, ops
from .._lib import ACT_ELU, ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SILU

# 'silu' and norm='gn' are OPTIONAL, NON-REFERENCE modes (BASELINE.json's north_star names GroupNorm + SiLU; the reference rejects
# 'silu' and crashes on 'gn'): PCRLv23d(norm='gn', act='silu') runs conv -> GroupNorm(8) -> SiLU in every LUConv except
# the 1-channel deep-supervision heads, which keep BatchNorm + sigmoid (GroupNorm(8, 1) cannot exist).  Default = the reference.
_ACTS = {"relu": ACT_RELU, "sigmoid": ACT_SIGMOID, "silu": ACT_SILU, "elu": ACT_ELU, "prelu": ACT_NONE}   # prelu: a pass of its own behind the normalisation


class _Counted:
    """`num_batches_tracked` bookkeeping done lazily: bumped on the host per forward, written to the device buffers
    only when somebody looks (state_dict / flush_counters)."""

    def _init_counter(self, bns):
        self._bns, self._pending = bns, 0

    def _count_batch(self):
        self._pending += 1

    def flush_counters(self):
        if self._pending:
            for bn in self._bns:
                bn.num_batches_tracked += self._pending
            self._pending = 0


class LUConv(nn.Module, _Counted):
    """conv3x3x3(pad 1, bias) -> BatchNorm3d(batch statistics) -> activation      [reference :6-34]"""

    def __init__(self, in_chan, out_chan, act, norm):
        super().__init__()
        if norm not in ("bn", "gn", "in"):
            raise ValueError('normalization type {} is not supported'.format(norm))
        if act not in _ACTS or (act == "silu" and norm != "gn"):    # the reference rejects 'silu' (:30); only the optional 'gn' mode takes it
            raise ValueError('activation type {} is not supported'.format(act))
        self.conv1 = nn.Conv3d(in_chan, out_chan, 3, padding=1)               # container: weight [Co,Ci,3,3,3], bias [Co]
        self._inorm = norm == "in"
        # per-sample statistics pooled over channel groups: GroupNorm(8) (optional mode) or one channel per group = InstanceNorm3d (:15-16);
        # the 1-channel heads keep BatchNorm in 'gn' mode (GroupNorm(8, 1) cannot exist) and take ops.luconv_forward's InstanceNorm route in 'in' mode
        self._gn_groups = (8 if norm == "gn" else out_chan) if (norm in ("gn", "in") and out_chan > 1) else 0
        if norm == "in":
            self.bn1 = nn.InstanceNorm3d(out_chan, momentum=ops.BN_MOMENTUM, affine=True)   # container: affine only (no running statistics, :16)
        elif self._gn_groups:
            self.bn1 = nn.GroupNorm(8, out_chan)                              # the reference's attribute name for either norm (:13-14)
        else:
            self.bn1 = nn.BatchNorm3d(out_chan, momentum=ops.BN_MOMENTUM)      # container: affine + running statistics
        self._prelu = act == "prelu"
        if self._prelu:
            self.activation = nn.PReLU(out_chan)                              # container: the slope vector, registered after bn1 like the reference (:23)
        # first layer of a multi-channel model (in_channels != 1, :98): zero-padded to the implicit-GEMM kernels' 32-channel granule
        self._ci_pad = 32 * ((in_chan + 31) // 32) if (in_chan != 1 and in_chan % 32) else 0
        self._act = _ACTS[act]
        self.compute_dtype = config.default_compute_dtype()
        self._packed = ops.PackedWeights("conv3")
        self._init_counter([] if (self._gn_groups or self._inorm) else [self.bn1])

    def forward(self, x):
        if self._ci_pad:
            x = x.float()
        else:
            x = x.float().contiguous() if self.conv1.in_channels == 1 else ops.to_act(x, self.compute_dtype)
        c, n = self.conv1, self.bn1
        return Fn.LUConvFn.apply(x, c.weight, c.bias, n.weight, n.bias, self)

    def forward_pooled(self, x, pool_only=False):
        """-> (act(bn1(conv1(x))), MaxPool3d(2) of it) as one autograd node (Fn.LUConvPoolFn): what PCRLv23d.forward asks of the second
        LUConv of an encoder stage.  BatchNorm layers with more than one input channel only.  pool_only (the engine's training step): the unpooled
        activation is not stored -- (a _LazySkip that builds it from the saved pre-normalisation tensor on demand, the pooled tensor)."""
        c, n = self.conv1, self.bn1
        out = Fn.LUConvPoolFn.apply(ops.to_act(x, self.compute_dtype), c.weight, c.bias, n.weight, n.bias, self, pool_only)
        if isinstance(out, tuple):
            return out
        return _LazySkip(self._last_saved, self.compute_dtype), out


class _LazySkip:
    """The unpooled output of an encoder stage when the training step did not store it: `PCRLv23d.skip_out64` (etc.) hands out
    act(scale * y + shift) computed from the stage's saved pre-normalisation tensor the first time somebody reads the attribute -- the values the
    stored tensor would have held, detached (the reference's attribute is a graph node; nothing in train_3d.py reads it)."""

    def __init__(self, sv, dt):
        self.sv, self.dt, self.value = sv, dt, None

    def materialize(self):
        if self.value is None:
            sv = self.sv
            N, D, H, W, _, Co = sv.geom
            with torch.no_grad():
                self.value = ops.bn_act_apply(sv.y, sv.scale, sv.shift, N * D * H * W, Co, sv.act, self.dt)
            self.sv = None
        return self.value


def _make_nConv(in_channel, depth, act, norm, double_chnnel=False):
    """Two LUConvs.  Encoder stage d: in -> 32*2^d -> 64*2^d; decoder stage (double_chnnel): in -> 64*2^d -> 64*2^d   [:37-45]"""
    wide = 64 << depth
    mid = wide if double_chnnel else wide // 2
    first, second = LUConv(in_channel, mid, act, norm), LUConv(mid, wide, act, norm)
    # engine hint, not a submodule (no state_dict entry): `first`'s activation has `second` as its only consumer, so `second`'s data gradient may take
    # the first pass of `first`'s BatchNorm backward from its own output tiles (functions.LUConvFn / ops.luconv_backward `bnred`)
    object.__setattr__(second, "_below", first)
    return nn.Sequential(first, second)


class UpTransition(nn.Module, _Counted):
    """ConvTranspose3d(k2,s2) -> two LUConvs -> {global-average projection head, predictor MLP, deep-supervision map}   [:48-72]"""

    def __init__(self, inChans, outChans, depth, act, norm):
        super().__init__()
        c = 64 << depth
        self.depth = depth
        self.up_conv = nn.ConvTranspose3d(inChans, outChans, 2, stride=2)
        self.ops = _make_nConv(outChans, depth, act, norm, double_chnnel=True)
        self.bn = nn.BatchNorm1d(c)
        self.predictor_head = nn.Sequential(nn.Linear(c, 2 * c), nn.BatchNorm1d(2 * c), nn.ReLU(inplace=True), nn.Linear(2 * c, c))
        self.deep_supervision_head = LUConv(c, 1, "sigmoid", norm)
        self._act = _ACTS[act]
        self.compute_dtype = config.default_compute_dtype()
        self._packed_up = ops.PackedWeights("convt")
        self._composed_up = ops.ComposedUpConv()
        self._init_counter([self.bn, self.predictor_head[1]])

    def _count_batch_heads(self):
        self._count_batch()

    def _stage_params(self):
        lu = lambda m: (m.conv1.weight, m.conv1.bias, m.bn1.weight, m.bn1.bias)
        ph = self.predictor_head
        return ((self.up_conv.weight, self.up_conv.bias) + lu(self.ops[0]) + lu(self.ops[1]) + (self.bn.weight, self.bn.bias)
                + (ph[0].weight, ph[0].bias, ph[1].weight, ph[1].bias, ph[3].weight, ph[3].bias) + lu(self.deep_supervision_head))

    def forward(self, x):
        """-> (x, x_pro, x_pre, x_mask)"""
        return Fn.UpStageFn.apply(x, *self._stage_params(), self)


class OutputTransition(nn.Module):
    """sigmoid(conv1x1x1)   [:75-83]"""

    def __init__(self, inChans, n_labels):
        super().__init__()
        self.final_conv = nn.Conv3d(inChans, n_labels, 1)
        self.sigmoid = nn.Sigmoid()   # kept for attribute parity; the sigmoid is fused into the kernel path
        self.compute_dtype = config.default_compute_dtype()

    def forward(self, x):
        return Fn.OutFn.apply(x, self.final_conv.weight, self.final_conv.bias, self)


class DownTransition(nn.Module):
    """encoder stage   [:86-92]"""

    def __init__(self, in_channel, depth, act, norm):
        super().__init__()
        self.ops = _make_nConv(in_channel, depth, act, norm)

    def forward(self, x):
        return self.ops(x)


class _MaxPool3d2(nn.MaxPool3d):
    """`self.maxpool` of the reference (:100) routed to the gfx950 kernel."""

    def __init__(self):
        super().__init__(2)
        self.compute_dtype = config.default_compute_dtype()

    def forward(self, x):
        return Fn.MaxPoolFn.apply(ops.to_act(x, self.compute_dtype), self.compute_dtype)


_ENCODER = (("down_tr64", None, 0), ("down_tr128", 64, 1), ("down_tr256", 128, 2), ("down_tr512", 256, 3))   # name, Cin, depth
_DECODER = (("up_tr256", 512, 2), ("up_tr128", 256, 1), ("up_tr64", 128, 0))                                  # name, C, depth
_SKIPS = ("skip_out64", "skip_out128", "skip_out256", "out512")                                               # attributes stashed by forward (:114-117)
_UPSAMPLE = (4, 2, 1)                                                                                         # trilinear factors of the three masks (:125-127)


# The encoder half of the two forwards, shared by PCRLv23d and NoduleClassifier (both hold the four `down_tr*` stages and `maxpool` under the
# same names): one sequence of launches, whichever model asks.
def _eval_luconv(m, h, dt, fused):
    """One LUConv on its running statistics: the inference kernel (fused) or the module chain's two passes."""
    c, n, gn = m.conv1, m.bn1, m._gn_groups
    w = c.weight
    if m._ci_pad:
        h, w = ops.pad_first_layer(h, w, m._ci_pad, dt)
    rm, rv = (None, None) if gn else (n.running_mean, n.running_var)
    if fused:
        return ops.luconv_infer(h, w, c.bias, n.weight, n.bias, rm, rv, m._packed, m._act, dt, gn_groups=gn, prelu=Fn._slope(m), inorm=m._inorm)
    return ops.luconv_forward(h, w, c.bias, n.weight, n.bias, rm, rv,
                              m._packed, m._act, dt, training=False, gn_groups=gn, prelu=Fn._slope(m), inorm=m._inorm)[0]


def _eval_encoder(model, x, dt, fused, stash):
    """-> `down_tr512`'s output on the running statistics.  stash: the stage outputs are kept as `skip_out64` ... `out512` (the reference's attributes)."""
    h = x.float().contiguous()
    for i, ((name, _, _), attr) in enumerate(zip(_ENCODER, _SKIPS)):
        if i:
            h = ops.maxpool_forward(ops.to_act(h, dt), dt)
        st = getattr(model, name)
        h = _eval_luconv(st.ops[1], _eval_luconv(st.ops[0], h, dt, fused), dt, fused)
        if stash:
            setattr(model, attr, h)
    return h


def _train_encoder(model, x, mine, lazy_skips, stash):
    """-> `down_tr512`'s output in training mode.  `mine()` marks the stage modules with the pass number before every stage; lazy_skips: the
    unpooled outputs of the first three stages are not stored (_LazySkip)."""
    h, pooled = x, None
    for i, ((name, _, _), attr) in enumerate(zip(_ENCODER, _SKIPS)):
        stage = getattr(model, name)
        mine()
        h = h if i == 0 else (pooled if pooled is not None else model.maxpool(h))
        last = stage.ops[1]
        if config.FOLD_POOL_GRAD and i + 1 < len(_ENCODER) and not last._gn_groups:
            # stage output and `self.maxpool` of it (:115-117) as one node: the pool's backward folds into the BatchNorm backward
            a = stage.ops[0](h)
            h, pooled = last.forward_pooled(a, pool_only=lazy_skips)     # lazy_skips: h is a _LazySkip (the stage output is not stored)
        else:
            h, pooled = stage(h), None
        if stash:
            setattr(model, attr, h)          # the reference keeps these alive as attributes; the skips are never consumed (D6)
    return h


class PCRLv23d(nn.Module):
    """reference: models/pcrlv2_model_3d.py:95-133"""

    def __init__(self, n_class=1, act='relu', norm='bn', in_channels=1, low_dim=128, student=False):
        super().__init__()
        self.compute_dtype = config.default_compute_dtype()
        # registration order == the reference's, so state_dict() enumerates the same 169 keys in the same order
        self.maxpool = _MaxPool3d2()
        for name, cin, depth in _ENCODER:
            setattr(self, name, DownTransition(in_channels if cin is None else cin, depth, act, norm))
        self.avg_pool = nn.AdaptiveAvgPool3d((1, 1, 1))     # unused in the reference too (:105)
        for name, c, depth in _DECODER:
            setattr(self, name, UpTransition(c, c, depth, act, norm))
        self.out_tr = OutputTransition(64, n_class)
        self.sigmoid = nn.Sigmoid()                         # unused in the reference too (:110)

    # ---- engine controls (not in the reference) ----
    def set_compute_dtype(self, dt):
        """float32 (exact parity mode) or bfloat16 (MFMA throughput mode) for activations / packed weights."""
        dt = {"fp32": torch.float32, "bf16": torch.bfloat16}.get(dt, dt) if isinstance(dt, str) else dt
        if dt not in (torch.float32, torch.bfloat16):
            raise ValueError("compute dtype must be float32 or bfloat16")
        for m in self.modules():
            if hasattr(m, "compute_dtype"):
                m.compute_dtype = dt
        return self

    def flush_counters(self):
        for m in self.modules():
            if isinstance(m, _Counted):
                m.flush_counters()

    def _stage_modules(self):
        if not hasattr(self, "_stages"):
            object.__setattr__(self, "_stages", [m for m in self.modules() if isinstance(m, (LUConv, UpTransition, OutputTransition))])
        return self._stages

    def state_dict(self, *args, **kwargs):
        self.flush_counters()
        return super().state_dict(*args, **kwargs)

    def load_state_dict(self, state_dict, *args, **kwargs):
        """In-place copy like nn.Module's (parameters may live in FusedSGD's flat arena), plus the two things the engine caches:
        pending `num_batches_tracked` bumps are dropped (the loaded counters win) and packed weights are invalidated."""
        for m in self.modules():
            if isinstance(m, _Counted):
                m._pending = 0
        out = super().load_state_dict(state_dict, *args, **kwargs)
        ops.bump_weights_epoch()
        return out

    @torch.no_grad()
    def _forward_eval(self, x, local):
        """`model.eval()` forward (what a consumer of the checkpoint runs for validation, README.md:48-55): the same kernels with every
        BatchNorm on its RUNNING statistics, nothing updated, no autograd graph (inference only: fine-tuning runs in train mode)."""
        return self._eval_stages(x, local, fused=False)

    @torch.no_grad()
    def infer(self, x, local=False, *, features_only=False):
        """The eval-mode forward on the inference kernels (engine extension): the values of `model.eval()(x, local)` -- in bf16 up to the one
        rounding of the pre-normalisation tensor that this path does not perform -- with every BatchNorm + ReLU LUConv as ONE launch
        (ops.luconv_infer: normalisation and activation in the convolution's epilogue).  Whatever `self.training` says; no parameter, running
        statistic, counter or attribute of the model is touched.  features_only: (None, features, []) -- the reconstruction, the deep-supervision
        maps and their upsampling are skipped (the second view and the local views of train_3d.validate)."""
        if not x.is_cuda:
            raise RuntimeError("PCRLv23d (pcrlv2_amd) runs on the GPU only: input is on %s and there is no CPU fallback" % x.device)
        return self._eval_stages(x, local, fused=True, features_only=features_only)

    def _eval_stages(self, x, local, fused, features_only=False):
        dt = self.compute_dtype
        lu = lambda m, h: _eval_luconv(m, h, dt, fused)     # noqa: E731
        h = _eval_encoder(self, x, dt, fused, stash=not fused)
        feats, masks = [], []
        for (name, _, _), factor in zip(_DECODER, _UPSAMPLE):
            up = getattr(self, name)
            h = lu(up.ops[1], lu(up.ops[0], ops.convt_forward(ops.to_act(h, dt), up.up_conv.weight, up.up_conv.bias, up._packed_up, dt)))
            ph = up.predictor_head
            pro = ops.bn1d_eval(ops.gap_forward(h, dt), up.bn.weight, up.bn.bias, up.bn.running_mean, up.bn.running_var, relu=False)
            hid = ops.bn1d_eval(ops.linear_forward(pro, ph[0].weight, ph[0].bias), ph[1].weight, ph[1].bias, ph[1].running_mean, ph[1].running_var, relu=True)
            feats.append([pro, ops.linear_forward(hid, ph[3].weight, ph[3].bias)])
            if not local and not features_only:
                mask = lu(up.deep_supervision_head, h)
                masks.append(mask if factor == 1 else ops.upsample_forward(mask, factor))
        if features_only:
            return None, feats, []
        return ops.conv1x1_to1_forward(ops.to_act(h, dt), self.out_tr.final_conv.weight, self.out_tr.final_conv.bias, dt), feats, masks

    def _train_stages(self, x, local, pass_idx, features_only=False, lazy_skips=False):
        """The training-mode forward.  (Rounds 3-4 had this as a generator so that several passes could be advanced stage by stage in rotation,
        each on its own stream, with one matrix kernel at a time -- measured slower, 33.5 -> 34.4 / 37.1 ms, DESIGN section 5 -- removed.)
        features_only: the caller discards the reconstruction and the deep-supervision maps (the second view and the local views of a
        training step, train_3d.py:117,123 -- SURVEY Q3): `out_tr` (no state) and the trilinear upsampling are skipped and None / [] are
        returned in their place; everything that has STATE -- the deep-supervision heads' BatchNorm running statistics -- still runs."""
        mods = self._stage_modules()

        def mine():          # the stage Functions read the pass number off their module at forward time
            for m in mods:
                m._pass_idx = pass_idx

        h = _train_encoder(self, x, mine, lazy_skips, stash=True)
        middle_features, middle_masks = [], []
        for (name, _, _), factor in zip(_DECODER, _UPSAMPLE):
            mine()
            h, pro, pre, mask = getattr(self, name)(h)
            middle_features.append([pro, pre])
            if not local and not features_only:
                middle_masks.append(mask if factor == 1 else Fn.TrilinearFn.apply(mask, factor))
        if features_only:
            return None, middle_features, middle_masks
        mine()
        out = self.out_tr(h)
        return out, middle_features, middle_masks

    def forward(self, x, local=False, *, features_only=False, lazy_skips=False):
        """-> (out [b,1,D,H,W], [[pro, pre] x 3 scales], [mask x 3] or [] when local).  `features_only` (engine extension, keyword only):
        (None, features, []) -- see _train_stages.  `lazy_skips` (engine extension, keyword only; train_3d.step_losses sets it): the encoder stages'
        unpooled outputs -- which the reference stashes as `self.skip_out64 / 128 / 256` (:114-117) and never reads -- are not written to HBM; the
        attributes still answer, computing the tensor from the stage's saved pre-normalisation values when read (detached)."""
        if not x.is_cuda:
            raise RuntimeError("PCRLv23d (pcrlv2_amd) runs on the GPU only: input is on %s and there is no CPU fallback" % x.device)
        if not self.training:
            return self._forward_eval(x, local)
        result = self._train_stages(x, local, ops.next_pass(), features_only, lazy_skips)     # pass 0 = first forward since the last optimizer step (its backward runs last)
        ops.end_of_forward_join()           # the stages' side branches (config.FWD_BRANCH_STREAM) are complete when the outputs are handed out
        return result


def _skip_attribute(name):
    """`model.skip_out64` etc.: plain attributes as in the reference (:114-117), except that a _LazySkip stored by the engine's training step is
    turned into its tensor when read."""
    def get(self):
        store = self.__dict__.get("_skip_store")
        if store is None or name not in store:
            raise AttributeError(f"'{type(self).__name__}' object has no attribute '{name}' (set by forward())")
        v = store[name]
        if isinstance(v, _LazySkip):
            v = store[name] = v.materialize()
        return v

    def put(self, v):
        self.__dict__.setdefault("_skip_store", {})[name] = v
    return property(get, put)


for _n in _SKIPS[:3]:
    setattr(PCRLv23d, _n, _skip_attribute(_n))



class NoduleClassifier(nn.Module):
    """The downstream model of the 3D encoder: LUNA16 nodule false-positive reduction, the paper's 3D classification task (the reference's fine-tune
    branch is not public).  `down_tr64 / 128 / 256 / 512` and `maxpool` are PCRLv23d's, under PCRLv23d's names -- the encoder keys of a 3D pre-training
    checkpoint are this model's -- and `classification_head` = Sequential(AdaptiveAvgPool3d(1), Flatten, Dropout(p), Linear(512, n_class), Sigmoid), a
    parameter container laid out as ChestClassifier's (the linear layer is `classification_head.3`).  `encoder_weights`: a 3D pre-training checkpoint
    ({'state_dict': PCRLv23d's}); its `down_tr*` entries must be exactly the encoder's, everything else in it is ignored.

    loss(x, labels) is the training step's path (the encoder half of PCRLv23d's training forward -> functions2d.ClsHeadFn on `down_tr512`'s NDHWC output
    viewed as NHWC [N, D/8 * H/8, W/8, 512]), infer(x) the eval-mode one (the encoder on running statistics through the inference kernels, the head
    without dropout); forward(x) returns probabilities in either mode.  The interface is ChestClassifier's."""

    def __init__(self, n_class=1, dropout=0.2, encoder_weights=None, act='relu', norm='bn', in_channels=1):
        super().__init__()
        if not 0.0 <= dropout < 1.0:
            raise ValueError("dropout must be in [0, 1)")
        self.compute_dtype = config.default_compute_dtype()
        self.maxpool = _MaxPool3d2()
        for name, cin, depth in _ENCODER:
            setattr(self, name, DownTransition(in_channels if cin is None else cin, depth, act, norm))
        self.classification_head = nn.Sequential(nn.AdaptiveAvgPool3d(1), nn.Flatten(), nn.Dropout(p=dropout, inplace=True),
                                                 nn.Linear(512, n_class, bias=True), nn.Sigmoid())
        nn.init.xavier_uniform_(self.classification_head[3].weight)        # as ChestClassifier's head (smp's initialize_head)
        nn.init.constant_(self.classification_head[3].bias, 0)
        self.n_class, self.dropout = n_class, float(dropout)
        self._pass_idx = 1
        self.mask_generator = None        # a torch.Generator on the model's device: seeded dropout masks (None: torch's default generator)
        if encoder_weights is not None:
            self.load_encoder(encoder_weights)

    def load_encoder(self, path):
        """The `down_tr*` entries of a 3D pre-training checkpoint's 'state_dict' -> the encoder, strictly: a missing or an unknown encoder key raises."""
        ckpt = torch.load(path, map_location="cpu", weights_only=False)
        if not isinstance(ckpt, dict) or "state_dict" not in ckpt:
            raise KeyError(f"{path}: no 'state_dict' entry (a 3D pre-training checkpoint is expected)")
        strip = lambda k: k[len("module."):] if k.startswith("module.") else k      # noqa: E731  (a checkpoint saved from under nn.DataParallel)
        enc = {strip(k): v for k, v in ckpt["state_dict"].items() if strip(k).startswith("down_tr")}
        own = {k for k in self.state_dict() if k.startswith("down_tr")}
        if set(enc) != own:
            raise KeyError(f"{path}: encoder keys differ from the model's: missing {sorted(own - set(enc))[:4]}, unexpected {sorted(set(enc) - own)[:4]}")
        self.load_state_dict(enc, strict=False)

    # ---- engine controls: PCRLv23d's (they walk self.modules()) ----
    set_compute_dtype = PCRLv23d.set_compute_dtype
    flush_counters = PCRLv23d.flush_counters
    _stage_modules = PCRLv23d._stage_modules

    def state_dict(self, *args, **kwargs):
        self.flush_counters()
        return super().state_dict(*args, **kwargs)

    def load_state_dict(self, state_dict, *args, **kwargs):
        for m in self.modules():
            if isinstance(m, _Counted):
                m._pending = 0
        out = super().load_state_dict(state_dict, *args, **kwargs)
        ops.bump_weights_epoch()
        return out

    def _check(self, x):
        if not x.is_cuda:
            raise RuntimeError("NoduleClassifier (pcrlv2_amd) runs on the GPU only: input is on %s and there is no CPU fallback" % x.device)

    def draw_keep(self, n, device):
        """The dropout keep mask of a training step: uint8 [n, 512], P(keep) = 1 - p, drawn on the device (`mask_generator` seeds it); None at p = 0."""
        if self.dropout == 0.0:
            return None
        return (torch.rand((n, 512), device=device, generator=self.mask_generator) >= self.dropout).to(torch.uint8)

    def _head_input(self, h):
        """`down_tr512`'s output [N,512,D,H,W] (NDHWC memory) as the NHWC activation [N, D * H, W, 512] the head kernels take: a view."""
        h = ops.to_act(h, self.compute_dtype)
        N, D, H, W, C = ops.dims(h)
        return h.permute(0, 2, 3, 4, 1).reshape(N, D * H, W, C).permute(0, 3, 1, 2)

    def loss(self, x, labels, keep=None):
        """Training mode: -> (BCE loss 0-d, probabilities float32 [N, n_class] (no gradient)).  labels: uint8 [N, n_class] on the device.  `keep`: a
        given dropout mask instead of a drawn one (tests)."""
        self._check(x)
        if not self.training:
            raise RuntimeError("NoduleClassifier.loss is the TRAINING step's path; in eval mode call infer")
        from .. import functions2d as Fn2
        pass_idx = ops.next_pass()
        self._pass_idx = pass_idx
        mods = self._stage_modules()

        def mine():
            for m in mods:
                m._pass_idx = pass_idx

        h = _train_encoder(self, x, mine, lazy_skips=True, stash=False)
        if keep is None:
            keep = self.draw_keep(x.shape[0], x.device)
        lin = self.classification_head[3]
        out = Fn2.ClsHeadFn.apply(self._head_input(h), lin.weight, lin.bias, labels, keep, self.dropout if keep is not None else 0.0, self)
        ops.end_of_forward_join()
        return out

    def _eval_probs(self, x, fused, labels=None):
        from .. import ops2d
        dt = self.compute_dtype
        h = _eval_encoder(self, x, dt, fused, stash=False)
        lin = self.classification_head[3]
        probs, _, loss = ops2d.cls_head_forward(self._head_input(h), lin.weight, lin.bias, dt, labels=labels)
        return probs if labels is None else (probs, loss)

    @torch.no_grad()
    def infer(self, x, labels=None):
        """Eval-mode probabilities float32 [N, n_class], whatever `self.training` says: nothing of the model is touched, no autograd graph.  With
        labels (uint8 [N, n_class]) -> (probabilities, mean BCE loss 0-d) from the same launch."""
        self._check(x)
        return self._eval_probs(x, True, labels)

    @torch.no_grad()
    def _forward_eval(self, x):
        """model.eval()(x): the module chain pass by pass on the running statistics, then the head without dropout."""
        self._check(x)
        return self._eval_probs(x, False)

    def forward(self, x):
        if not self.training:
            return self._forward_eval(x)
        labels = torch.zeros((x.shape[0], self.n_class), dtype=torch.uint8, device=x.device)
        return self.loss(x, labels)[1]


class Segmenter3d(PCRLv23d):
    """The downstream model of the whole pre-trained 3D network, decoder included: voxel-wise segmentation (BraTS / LiTS in the paper; the reference's
    README loads the whole PCRLv23d for it, its fine-tune branch is not public).  It IS a PCRLv23d(n_class, in_channels): the same modules under the
    same names, so `state_dict()` has the 169 keys of a pre-training checkpoint and a fine-tuned one loads into the reference's
    PCRLv23d(n_class=K, in_channels=C).  `weights`: a 3D pre-training checkpoint (load_pretrained).

    loss(x, labels) is the training step's path: the encoder half of the training forward, each decoder stage as up_conv -> ops.0 -> ops.1 only
    (functions.UpConvsFn), then the output head and the Dice/BCE loss as one operator (functions.SegHeadFn, csrc/seg_head.hip).  The projection,
    predictor and deep-supervision heads are NOT run: their parameters have requires_grad = False here and their running statistics and counters do
    not move; `trainable_parameters()` is what the optimiser gets.  infer(x, ...) is the eval-mode forward on the inference kernels followed by
    pcrl_seg_head_eval, infer_logits(x) the same forward followed by pcrl_seg_head_logits.  labels: uint8 [N, D, H, W], bit k = class k (classes may overlap), bit 7 = the voxel is not counted.

    head='softmax' (the default is 'sigmoid', everything above): n_class = K in 2..16 mutually exclusive classes, the background (class 0) counted in K;
    labels are a LABEL MAP (bits 0..6: the class index, bit 7: not counted) and the loss is wc * cross-entropy + wd * (1 - mean Dice of the classes
    1..K-1) on functions.SegSoftmaxHeadFn (csrc/seg_head_mc.hip).  loss, infer and infer_logits dispatch on `self.head`; infer then returns the predicted
    label map where the sigmoid head returns the bitmask, and counts rows for all K classes.  Everything below the head is shared."""

    _HEADS = ("bn.", "predictor_head.", "deep_supervision_head.")

    HEADS = ("sigmoid", "softmax")

    def __init__(self, n_class, in_channels=1, weights=None, act='relu', norm='bn', wb=1.0, wd=1.0, head='sigmoid', wc=1.0):
        if head not in self.HEADS:
            raise ValueError("head must be 'sigmoid' (overlapping regions, a bitmask) or 'softmax' (mutually exclusive classes, a label map), got %r" % (head,))
        if head == 'softmax' and not 2 <= int(n_class) <= 16:
            raise ValueError("n_class must be in 2..16 with the softmax head (mutually exclusive classes, the background counted; a label byte holds the "
                             "class index in bits 0..6), got %r" % (n_class,))
        if head == 'sigmoid' and not 1 <= int(n_class) <= 7:
            raise ValueError("n_class must be in 1..7 (one bit of the label byte per class; bit 7 means 'not counted'), got %r" % (n_class,))
        super().__init__(n_class=int(n_class), act=act, norm=norm, in_channels=in_channels)
        self.n_class, self.in_channels, self.wb, self.wd = int(n_class), int(in_channels), float(wb), float(wd)
        self.head, self.wc = head, float(wc)
        for name, p in self.named_parameters():
            if self._is_head(name):
                p.requires_grad_(False)
        if weights is not None:
            self.load_pretrained(weights)

    @classmethod
    def _is_head(cls, key):
        parts = key.split(".", 1)
        return parts[0].startswith("up_tr") and len(parts) > 1 and parts[1].startswith(cls._HEADS)

    def trainable_parameters(self):
        """The parameters loss() reaches, in registration order."""
        return [p for p in self.parameters() if p.requires_grad]

    def load_pretrained(self, path):
        """A 3D pre-training checkpoint's 'state_dict', strictly, with two announced exceptions that keep their fresh initialisation:
        `out_tr.final_conv.*` when n_class != the checkpoint's, `down_tr64.ops.0.conv1.weight` when in_channels differs.  Any other missing,
        unexpected or mis-shaped key raises KeyError."""
        ckpt = torch.load(path, map_location="cpu", weights_only=False)
        if not isinstance(ckpt, dict) or "state_dict" not in ckpt:
            raise KeyError(f"{path}: no 'state_dict' entry (a 3D pre-training checkpoint is expected)")
        strip = lambda k: k[len("module."):] if k.startswith("module.") else k      # noqa: E731
        sd = {strip(k): v for k, v in ckpt["state_dict"].items()}
        own = self.state_dict()
        if set(sd) != set(own):
            raise KeyError(f"{path}: keys differ from the model's: missing {sorted(set(own) - set(sd))[:4]}, unexpected {sorted(set(sd) - set(own))[:4]}")
        may_differ = {"out_tr.final_conv.weight": "n_class", "out_tr.final_conv.bias": "n_class", "down_tr64.ops.0.conv1.weight": "in_channels"}
        for k in list(sd):
            if tuple(sd[k].shape) != tuple(own[k].shape):
                if k not in may_differ:
                    raise KeyError(f"{path}: {k} has shape {tuple(sd[k].shape)}, the model's is {tuple(own[k].shape)}")
                print(f"==> {k}: checkpoint {tuple(sd[k].shape)} != model {tuple(own[k].shape)} ({may_differ[k]} differs): freshly initialised")
                sd[k] = own[k]
        self.load_state_dict(sd)

    def _check(self, x, labels):
        if not x.is_cuda:
            raise RuntimeError("Segmenter3d (pcrlv2_amd) runs on the GPU only: input is on %s and there is no CPU fallback" % x.device)
        if x.dim() != 5 or x.shape[1] != self.in_channels or any(int(s) % 8 for s in x.shape[2:]):
            raise ValueError(f"Segmenter3d: input must be [N, {self.in_channels}, D, H, W] with D, H, W multiples of 8, got {tuple(x.shape)}")
        if labels is not None and (labels.dtype != torch.uint8 or tuple(labels.shape) != (x.shape[0],) + tuple(x.shape[2:])):
            raise ValueError(f"Segmenter3d: labels must be a uint8 bitmask of shape {(x.shape[0],) + tuple(x.shape[2:])}, got {labels.dtype} {tuple(labels.shape)}")

    def forward(self, x, *args, **kwargs):
        raise RuntimeError("Segmenter3d has no forward(): PCRLv23d's would run the pre-training heads, which are frozen here.  Call loss(x, labels) in "
                           "training and infer(x, ...) for evaluation; the pre-training forward of these weights is PCRLv23d(n_class, in_channels)'s")

    def features(self, x):
        """Training mode: the last decoder stage's activation [N, 64, D, H, W] (NDHWC memory) -- the encoder half of the training forward, then each
        decoder stage without its heads.  One forward pass of the step (ops.next_pass)."""
        pass_idx = ops.next_pass()
        mods = self._stage_modules()

        def mine():
            for m in mods:
                m._pass_idx = pass_idx

        lu = lambda m: (m.conv1.weight, m.conv1.bias, m.bn1.weight, m.bn1.bias)      # noqa: E731
        h = _train_encoder(self, x, mine, lazy_skips=True, stash=False)
        for name, _, _ in _DECODER:
            mine()
            up = getattr(self, name)
            h = Fn.UpConvsFn.apply(h, up.up_conv.weight, up.up_conv.bias, *lu(up.ops[0]), *lu(up.ops[1]), up)
        mine()
        return h

    def loss(self, x, labels):
        """Training mode: -> (loss 0-d, sums float64 [4 K + 1] (no gradient): {I, P, G, BCE} per class, then the counted voxels)."""
        self._check(x, labels)
        if not self.training:
            raise RuntimeError("Segmenter3d.loss is the TRAINING step's path; in eval mode call infer")
        fc = self.out_tr.final_conv
        if self.head == 'softmax':      # sums: {I, P, G, CE} per class
            out = Fn.SegSoftmaxHeadFn.apply(self.features(x), fc.weight, fc.bias, labels.contiguous(), self.wc, self.wd, self.out_tr)
        else:
            out = Fn.SegHeadFn.apply(self.features(x), fc.weight, fc.bias, labels.contiguous(), self.wb, self.wd, self.out_tr)
        ops.end_of_forward_join()
        return out

    @torch.no_grad()
    def infer(self, x, labels=None, case_index=None, counts=None, want_mask=False):
        """The eval-mode forward on the inference kernels, whatever `self.training` says; nothing of the model is touched.  Prediction: z_k >= 0.
        counts int64 [cases, K, 3] (device) gets {TP, |pred|, |gt|} of sample n added at row case_index[n] (int32 [N]; None: row n of a fresh table).
        -> (counts, loss 0-d, sums float64 [4 K + 1], predicted bitmask uint8 [N, D, H, W] | None)
        Softmax head: prediction = the lowest class with the largest logit, counts rows for all K classes, and the label map in the bitmask's place."""
        self._check(x, labels)
        dt = self.compute_dtype
        fc = self.out_tr.final_conv
        if self.head == 'softmax':
            return ops.seg_mc_head_eval(self._infer_features(x, dt), fc.weight, fc.bias, dt, labels=None if labels is None else labels.contiguous(),
                                        case_index=case_index, counts=counts, want_mask=want_mask, wc=self.wc, wd=self.wd)
        return ops.seg_head_eval(self._infer_features(x, dt), fc.weight, fc.bias, dt, labels=None if labels is None else labels.contiguous(),
                                 case_index=case_index, counts=counts, want_mask=want_mask, wb=self.wb, wd=self.wd)

    def _infer_features(self, x, dt):
        """The last decoder stage's activation of the eval-mode forward on the inference kernels, NDHWC memory in `dt`."""
        h = _eval_encoder(self, x, dt, True, stash=False)
        for name, _, _ in _DECODER:
            up = getattr(self, name)
            h = ops.convt_forward(ops.to_act(h, dt), up.up_conv.weight, up.up_conv.bias, up._packed_up, dt)
            h = _eval_luconv(up.ops[1], _eval_luconv(up.ops[0], h, dt, True), dt, True)
        return ops.to_act(h, dt)

    @torch.no_grad()
    def infer_logits(self, x, out=None, *, flip=0, accumulate=False, scale=1.0):
        """infer's forward followed by the head's logits alone (pcrl_seg_head_logits), whatever `self.training` says; nothing of the model is touched.
        -> float32 [N, D, H, W, K] (written into `out` when given): thresholding it at 0 (softmax head: its lowest-index argmax) is infer's mask, bit for bit.  What overlap-blended
        sliding windows average (train_seg.sliding_window).
        With any of flip / accumulate / scale off its default the head is pcrl_seg_head_logits_acc and `out` is required: `x` is the ALREADY mirrored
        patch and `flip` (bit 0 = D, bit 1 = H, bit 2 = W) names the mirroring to undo, so each logit lands on its un-mirrored voxel of `out`;
        accumulate=False overwrites `out` (the first pass), True adds to what it holds; the result is multiplied by `scale` (float32)."""
        self._check(x, None)
        dt = self.compute_dtype
        fc = self.out_tr.final_conv
        if self.head == 'softmax':      # one entry point for the plain and the accumulating store
            if out is None and (flip != 0 or accumulate or float(scale) != 1.0):
                raise ValueError("Segmenter3d.infer_logits: flip / accumulate / scale write into the buffer `out`, which is required with them")
            return ops.seg_mc_head_logits(self._infer_features(x, dt), fc.weight, fc.bias, dt, out=out, flip=flip, first=not accumulate, scale=scale)
        if flip == 0 and not accumulate and float(scale) == 1.0:
            return ops.seg_head_logits(self._infer_features(x, dt), fc.weight, fc.bias, dt, out=out)
        if out is None:
            raise ValueError("Segmenter3d.infer_logits: flip / accumulate / scale write into the buffer `out`, which is required with them")
        return ops.seg_head_logits_acc(self._infer_features(x, dt), fc.weight, fc.bias, dt, out, flip=flip, first=not accumulate, scale=scale)
