"""Fused optimisers over a flat parameter arena, one step kernel launch per step.

`FusedSGD` is torch.optim.SGD as configured at train_3d.py:48-51 (momentum, weight decay on every parameter, dampening 0, no nesterov): the
pre-training optimiser.  It subclasses torch.optim.SGD so `param_groups` (what utils.adjust_learning_rate edits) and
the checkpoint's `optimizer.state_dict()` layout ('momentum_buffer' per parameter) stay those of the
reference.  Parameters are re-homed into one contiguous float32 arena (values preserved; the
nn.Parameter objects stay the same), momentum buffers into a second arena, and gradients are
summed into a third (which is also the buffer the data-parallel all-reduce works on).
Parameters whose .grad is None are skipped, like torch.optim.SGD does after zero_grad(set_to_none=True).

`FusedAdam` / `FusedAdamW` (the decoupled form) are the fine-tuning optimisers over the same arenas: torch.optim.Adam / AdamW's
single-tensor arithmetic in float32 (csrc/optim.hip), 'exp_avg' / 'exp_avg_sq' in two state arenas, and torch's per-parameter `step` as
device-resident tables that a tiny launch advances in front of the step -- nothing is uploaded or read back per step.

All of them take `max_grad_norm`: torch.nn.utils.clip_grad_norm_ over the parameters that have a gradient, computed after the gradient
all-reduce by one extra read of the gradient arena; the coefficient stays on the device and is folded into the step kernel, the gradients
are not rewritten.  `optimizer.grad_norm` (float64[1] on the device) holds the last step's norm.
"""
from __future__ import annotations

import torch

from . import ops
from ._lib import lib, stream_handle


def _zeros(n, dtype, dev):
    """Zero-filled by the library's own entry point (a runtime memset): no ATen fill kernel even at set-up."""
    a = torch.empty(n, dtype=dtype, device=dev)
    lib().call("pcrl_zero", a, a.element_size() * n, stream_handle())
    return a


def state_kind(state_dict):
    """'sgd' | 'adam' | None: which family an optimizer.state_dict() belongs to (by its per-parameter state, else by its param group)."""
    for st in state_dict.get("state", {}).values():
        if "exp_avg" in st:
            return "adam"
        if "momentum_buffer" in st:
            return "sgd"
    for g in state_dict.get("param_groups", []):
        if "betas" in g:
            return "adam"
        if "momentum" in g:
            return "sgd"
    return None


def require_state_kind(optimizer, state_dict, saved=None):
    """Exit with a message when a checkpoint's optimiser state is not of the kind of `optimizer` (`saved`: the checkpoint's own --optimizer,
    which tells Adam from AdamW where the state alone cannot)."""
    want, have = getattr(optimizer, "kind", None), state_kind(state_dict)
    if want is None:          # not one of this module's optimisers: torch's own load_state_dict decides
        return
    if saved in ("sgd", "adam", "adamw") and have in (None, "sgd" if saved == "sgd" else "adam"):
        have = saved
    if have is None or have == want or (have == "adam" and want == "adamw" and saved is None):
        return
    raise SystemExit("the checkpoint holds the state of optimizer '{}', but '{}' was asked for: resume with --optimizer {}".format(
        have, want, "adam|adamw" if have == "adam" else have))


class _FlatArenas:
    """What the fused optimisers share: the arenas and their slots, the gradient gather, the cached flags table, the optional clip
    coefficient, and the tail of a step.  Mixed in FRONT of the torch.optim class."""

    def _init_arenas(self, name, nstate):
        """Re-home the single param group into flat_p; -> the `nstate` zeroed state arenas."""
        self._plist = [p for p in self.param_groups[0]["params"]]
        dev = self._plist[0].device
        if dev.type != "cuda":
            raise RuntimeError(name + " needs parameters on the GPU (no CPU fallback)")
        sizes = [p.numel() for p in self._plist]
        # every parameter starts on a 16-byte boundary of the arena (slots rounded up to 4 floats; the padding stays zero in all the
        # arenas): the kernels that read weights with 16-byte loads (the heads' Linear products) take them as they lie -- the model has
        # 1-element parameters (the deep-supervision heads' 1-channel convolutions and norms) in front of them
        self._slot_sizes = [(n + 3) // 4 * 4 for n in sizes]
        offs = [0]
        for n in self._slot_sizes:
            offs.append(offs[-1] + n)
        self._offsets_host = offs
        self._total = offs[-1]
        arenas = [_zeros(self._total, torch.float32, dev) for _ in range(2 + nstate)]
        self.flat_p, self.flat_g = arenas[:2]
        with torch.no_grad():
            for p, o, n in zip(self._plist, offs, sizes):
                if p.dtype != torch.float32:
                    raise ValueError(name + ": parameters must be float32")
                self.flat_p[o:o + n].copy_(p.detach().reshape(-1))
                p.data = self.flat_p[o:o + n].view(p.shape)
        self._offsets = torch.tensor(offs, dtype=torch.int64, device=dev)
        self._gviews = [self.flat_g[o:o + n].view(p.shape) for p, o, n in zip(self._plist, offs, sizes)]
        self._numels = torch.tensor(sizes, dtype=torch.int64, device=dev)
        import ctypes
        self._offsets_c = (ctypes.c_int64 * len(offs))(*offs)       # pcrl_grad_sum reads the offsets on the host as well
        for i, (p, v) in enumerate(zip(self._plist, self._gviews)):
            p._pcrl_gview = v      # pcrlv2_amd.functions.flush_param_grads sums the step's gradients straight into the arena
            p._pcrl_gslot = (self, i)
        self._initialised = [False] * len(self._plist)
        self._flag_cache = {}
        self._flag_ring = None
        self.grad_scale = 1.0          # set to 1/world_size by the data-parallel wrapper
        self.pre_step = None           # optional callable(self, None) -> has-grad list: replaces the gradient gather (ddp.DataParallel)
        self.skip_flag = None          # float32[1] on the device, consumed by the NEXT step(): non-zero = leave parameters and momentum untouched
        return arenas[2:]

    def _init_clip(self, max_grad_norm):
        self.max_grad_norm = None if not max_grad_norm else float(max_grad_norm)
        self.grad_norm = None
        if self.max_grad_norm is not None:
            if not self.max_grad_norm > 0:
                raise ValueError("max_grad_norm must be positive (None or 0: no clipping)")
            dev = self.flat_p.device
            self._norm_partials = _zeros(lib().fn["pcrl_optim_grid_cap"][0](), torch.float64, dev)
            self.grad_norm = _zeros(1, torch.float64, dev)
            self._clip_coef = _zeros(1, torch.float32, dev)

    def _state_view(self, arena, i):
        o = self._offsets_host[i]
        return arena[o:o + self._plist[i].numel()].view(self._plist[i].shape)

    # ------------------------------------------------------------------
    def gather_grads(self):
        """Gradients that do not already live in the flat arena (set by hand, or produced by autograd's own accumulation)
        are copied into it; returns the has-grad list."""
        has = [p.grad is not None for p in self._plist]
        todo = [(v, p.grad) for v, p, h in zip(self._gviews, self._plist, has) if h and p.grad.data_ptr() != v.data_ptr()]
        if todo:
            torch._foreach_copy_([v for v, _ in todo], [g for _, g in todo])
        return has

    def _flags(self, has):
        """int32 per parameter (bit 0: has a gradient, bit 1: momentum buffer initialised) on the device.  Patterns are cached; a NEW pattern
        (the 2D step has 160 of them: which scales the 13 draws picked) is staged in a pinned host slot and copied asynchronously on the
        current stream -- `torch.tensor(vals, device=...)` is a pageable-memory copy, which the runtime completes only after everything
        queued before it: a host stall of the whole backward (14 ms per 2D step, tools/host_probe_2d.py).  A slot is reused after
        `len(ring)` further misses; the host never runs more than config.MAX_STEPS_AHEAD steps ahead of the device, and the ring is deeper."""
        key = (tuple(has), tuple(self._initialised))
        t = self._flag_cache.get(key)
        if t is None:
            vals = [(1 if h else 0) | (2 if i else 0) for h, i in zip(has, self._initialised)]
            if self._flag_ring is None:
                self._flag_ring = [torch.empty(len(vals), dtype=torch.int32).pin_memory() for _ in range(8)]
                self._flag_ring_ev = [None] * 8
                self._flag_ring_pos = 0
            k = self._flag_ring_pos = (self._flag_ring_pos + 1) % len(self._flag_ring)
            if self._flag_ring_ev[k] is not None:
                self._flag_ring_ev[k].synchronize()       # the copy that last read this slot (long done: 8 misses ago)
            self._flag_ring[k].copy_(torch.tensor(vals, dtype=torch.int32))
            t = self._flag_ring[k].to(self.flat_p.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._flag_ring_ev[k] = ev
            if len(self._flag_cache) > 256:
                self._flag_cache.clear()
            self._flag_cache[key] = t
        return t

    def _gather(self):
        """Head of a step: the side stream joined, the gradients in the arena (all-reduced under data parallelism) -> the has-grad list."""
        ops.join_side_stream()
        if self.pre_step is not None:
            return self.pre_step(self, None)       # the data-parallel wrapper gathers (bucket by bucket) and all-reduces
        return self.gather_grads()

    def _clip(self, flags):
        """-> the device clip coefficient of this step's gradients (None without max_grad_norm: nothing is launched)."""
        if self.max_grad_norm is None:
            return None
        lib().call("pcrl_grad_norm", self.flat_g, self._offsets, self._numels, flags, len(self._plist), self._total, float(self.grad_scale),
                   self.max_grad_norm, self._norm_partials, self.grad_norm, self._clip_coef, stream_handle())
        return self._clip_coef


class FusedSGD(_FlatArenas, torch.optim.SGD):
    kind = "sgd"

    def __init__(self, params, lr=1e-3, momentum=0.0, weight_decay=0.0, max_grad_norm=None, **kw):
        # the reference's argparse leaves --momentum / --weight_decay as strings when given on the CLI
        super().__init__(params, lr=float(lr), momentum=float(momentum), weight_decay=float(weight_decay), **kw)
        if len(self.param_groups) != 1:
            raise ValueError("FusedSGD supports a single param group (the reference uses one)")
        g = self.param_groups[0]
        if g["dampening"] != 0 or g["nesterov"] or g.get("maximize", False):
            raise ValueError("FusedSGD implements dampening=0, nesterov=False, maximize=False")
        self.flat_buf, = self._init_arenas("FusedSGD", 1)
        self._init_clip(max_grad_norm)
        ops.bump_weights_epoch()

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """torch.optim.SGD layout in ('momentum_buffer' per parameter, e.g. from a checkpoint written by the reference or by
        this class, train_3d.py:71-82); the buffers are copied into the flat arena the kernel updates."""
        require_state_kind(self, state_dict)
        super().load_state_dict(state_dict)
        if len(self.param_groups) != 1:
            raise ValueError("FusedSGD supports a single param group")
        for i, p in enumerate(self._plist):
            buf = self.state.get(p, {}).get("momentum_buffer")
            o, n = self._offsets_host[i], p.numel()
            view = self.flat_buf[o:o + n].view(p.shape)
            if buf is None:
                view.zero_()
                self._initialised[i] = False
                self.state.pop(p, None)
            else:
                view.copy_(buf.to(device=view.device, dtype=torch.float32))
                self.state[p]["momentum_buffer"] = view
                self._initialised[i] = True
        self._flag_cache.clear()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        g = self.param_groups[0]
        has = self._gather()
        flags = self._flags(has)
        skip, self.skip_flag = self.skip_flag, None
        clip = self._clip(flags)
        if clip is not None:
            if skip is not None:
                raise RuntimeError("FusedSGD: max_grad_norm and the device-decided skip flag (the pre-task's divergence guard) do not combine")
            lib().call("pcrl_sgd_step_clipped", self.flat_p, self.flat_g, self.flat_buf, self._offsets, flags, len(self._plist),
                       self._total, float(g["lr"]), float(g["momentum"]), float(g["weight_decay"]), float(self.grad_scale), clip,
                       stream_handle())
        elif skip is None:
            lib().call("pcrl_sgd_step", self.flat_p, self.flat_g, self.flat_buf, self._offsets, flags, len(self._plist),
                       self._total, float(g["lr"]), float(g["momentum"]), float(g["weight_decay"]), float(self.grad_scale),
                       stream_handle())
        else:
            # the divergence guard decided on the device (train_3d.train_step): a skipped update leaves the arenas bit-unchanged.  The host-side
            # "momentum initialised" marks below are set either way; the buffers start as zeros, so momentum * 0 + g == g and a first update
            # that happens one step later is the same arithmetic.
            lib().call("pcrl_sgd_step_guarded", self.flat_p, self.flat_g, self.flat_buf, self._offsets, flags, len(self._plist),
                       self._total, float(g["lr"]), float(g["momentum"]), float(g["weight_decay"]), float(self.grad_scale), skip,
                       stream_handle())
        for i, (p, h) in enumerate(zip(self._plist, has)):
            if h and not self._initialised[i]:
                self._initialised[i] = True
                o, n = self._offsets_host[i], p.numel()
                self.state[p]["momentum_buffer"] = self.flat_buf[o:o + n].view(p.shape)
        ops.bump_weights_epoch()
        ops.begin_step()
        return loss


def running_product(beta, steps):
    """beta^steps the way pcrl_adam_prepare builds it: one IEEE double multiply per step."""
    x = 1.0
    for _ in range(int(steps)):
        x = x * beta
    return x


class _FusedAdamBase(_FlatArenas):
    """torch.optim.Adam / AdamW, single-tensor order, over the arenas (module docstring).  `flat_m` / `flat_v` are 'exp_avg' / 'exp_avg_sq';
    `_steps` (int32[n]), `_prods` (float64[2n]: beta1^t, beta2^t) and `_coefs` (float32[2n]: lr / (1 - beta1^t), sqrt(1 - beta2^t)) live
    on the device and are advanced there; `_step_host` mirrors the counts, because the host knows which parameters had a gradient."""
    _decoupled = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, max_grad_norm=None, **kw):
        name = type(self).__name__
        for opt in ("maximize", "capturable", "differentiable"):
            if kw.get(opt):
                raise ValueError("{} does not implement {}=True".format(name, opt))
        if amsgrad:
            raise ValueError("{} does not implement amsgrad=True".format(name))
        super().__init__(params, lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps), weight_decay=float(weight_decay), **kw)
        if len(self.param_groups) != 1:
            raise ValueError(name + " supports a single param group")
        self.flat_m, self.flat_v = self._init_arenas(name, 2)
        n, dev = len(self._plist), self.flat_p.device
        self._step_host = [0] * n
        self._steps = _zeros(n, torch.int32, dev)
        self._coefs = _zeros(2 * n, torch.float32, dev)
        self._prods = torch.tensor([1.0] * (2 * n), dtype=torch.float64, device=dev)
        self._state_tensors = (self.flat_m, self.flat_v, self._steps, self._prods, self._coefs)      # what a resumed data-parallel run broadcasts
        self._init_clip(max_grad_norm)
        ops.bump_weights_epoch()

    def _attach_state(self, i):
        p = self._plist[i]
        self.state[p]["step"] = torch.tensor(float(self._step_host[i]), dtype=torch.float32)
        self.state[p]["exp_avg"] = self._state_view(self.flat_m, i)
        self.state[p]["exp_avg_sq"] = self._state_view(self.flat_v, i)
        self._initialised[i] = True

    def state_dict(self):
        """torch's layout: 'step' (float32 0-d, from the host mirror of the counts: no device read-back), 'exp_avg', 'exp_avg_sq'."""
        for i, p in enumerate(self._plist):
            if self._initialised[i]:
                self.state[p]["step"] = torch.tensor(float(self._step_host[i]), dtype=torch.float32)
        return super().state_dict()

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """A state of this class or of stock torch.optim.Adam / AdamW: the moments are copied into the arenas, the step counts into the tables,
        and the products beta^step are rebuilt by the same running multiply the device uses."""
        name = type(self).__name__
        require_state_kind(self, state_dict)
        super().load_state_dict(state_dict)
        if len(self.param_groups) != 1:
            raise ValueError(name + " supports a single param group")
        g = self.param_groups[0]
        for opt in ("amsgrad", "maximize", "capturable", "differentiable"):
            if g.get(opt):
                raise ValueError("{} does not implement {}=True (the loaded state asks for it)".format(name, opt))
        b1, b2 = (float(b) for b in g["betas"])
        steps, prods, cache = [], [], {0: (1.0, 1.0)}
        for i, p in enumerate(self._plist):
            st = self.state.get(p, {})
            m, v = self._state_view(self.flat_m, i), self._state_view(self.flat_v, i)
            if "exp_avg" not in st:
                m.zero_()
                v.zero_()
                self._step_host[i] = 0
                self._initialised[i] = False
                self.state.pop(p, None)
            else:
                m.copy_(st["exp_avg"].to(device=m.device, dtype=torch.float32))
                v.copy_(st["exp_avg_sq"].to(device=v.device, dtype=torch.float32))
                self._step_host[i] = int(float(st["step"]))
                self._attach_state(i)
            k = self._step_host[i]
            if k not in cache:
                cache[k] = (running_product(b1, k), running_product(b2, k))
            steps.append(k)
            prods.extend(cache[k])
        dev = self.flat_p.device
        self._steps.copy_(torch.tensor(steps, dtype=torch.int32, device=dev))
        self._prods.copy_(torch.tensor(prods, dtype=torch.float64, device=dev))
        self._flag_cache.clear()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.skip_flag is not None:
            raise RuntimeError("{}: the device-decided skip flag (the pre-task's divergence guard) is FusedSGD's; the pre-task stays on SGD".format(
                type(self).__name__))
        g = self.param_groups[0]
        lr, wd, (b1, b2) = float(g["lr"]), float(g["weight_decay"]), (float(b) for b in g["betas"])
        has = self._gather()
        flags = self._flags(has)
        n = len(self._plist)
        lib().call("pcrl_adam_prepare", flags, self._steps, self._prods, self._coefs, n, lr, b1, b2, stream_handle())
        clip = self._clip(flags)
        lib().call("pcrl_adam_step", self.flat_p, self.flat_g, self.flat_m, self.flat_v, self._offsets, flags, self._coefs, n, self._total,
                   (1.0 - lr * wd) if self._decoupled else wd, int(self._decoupled), 1.0 - b1, b2, 1.0 - b2, float(g["eps"]),
                   float(self.grad_scale), clip, stream_handle())
        for i, h in enumerate(has):
            if h:
                self._step_host[i] += 1
                if not self._initialised[i]:
                    self._attach_state(i)
        ops.bump_weights_epoch()
        ops.begin_step()
        return loss


class FusedAdam(_FusedAdamBase, torch.optim.Adam):
    """torch.optim.Adam: weight decay added to the gradient (L2)."""
    kind = "adam"
    _decoupled = False


class FusedAdamW(_FusedAdamBase, torch.optim.AdamW):
    """torch.optim.AdamW: decoupled weight decay, p *= 1 - lr * wd in front of the update."""
    kind = "adamw"
    _decoupled = True


def restore(optimizer, ckpt):
    """`--resume`: the checkpoint's optimiser state into `optimizer`; a state of another kind (by the state itself and, where the checkpoint's
    own options name it, by --optimizer) ends the run with a message."""
    require_state_kind(optimizer, ckpt["optimizer"], getattr(ckpt.get("opt"), "optimizer", None))
    optimizer.load_state_dict(ckpt["optimizer"])


def for_task(sgd, params, **kw):
    """loop.Task.make_optimizer of the fine-tuning loops: plain SGD (no optimiser options) is the task module's own `sgd(params, lr=, momentum=,
    weight_decay=)`, the call it always was; anything else goes through make()."""
    if not set(kw) - {"lr", "momentum", "weight_decay"}:
        return sgd(params, **kw)
    return make(params, **kw)


def make(params, lr, momentum=0.0, weight_decay=0.0, kind="sgd", betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None):
    """What loop.Task.make_optimizer builds for the fine-tuning loops: the optimiser --optimizer / --betas / --eps / --clip_grad ask for
    (optim_cli.options); without them FusedSGD, as ever."""
    if kind == "sgd":
        return FusedSGD(params, lr=lr, momentum=momentum, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
    if kind in ("adam", "adamw"):
        return (FusedAdam if kind == "adam" else FusedAdamW)(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                                             max_grad_norm=max_grad_norm)
    raise ValueError("unknown optimizer '{}' (sgd, adam or adamw)".format(kind))
