"""SmartOptimizer - drop-in for kod.nn.optim.smart.SmartOptimizer (kod/nn/optim/smart.py:11-60).

Same constructor and call: ``SmartOptimizer(optimizer=partial(torch.optim.SGD, lr=.01, momentum=.937, nesterov=True),
weight_decay=5e-4)(net)`` (kod/configs/nn/optimizers/smart_sgd.yaml) returns a ``torch.optim.Optimizer`` whose
``param_groups`` are the reference's three named groups - bias_params | decay_params | norm_params, parameters in
module-walk order - so OptimizerWarmupUpdater (warmup.py:39-58), LambdaLR schedulers and Lightning checkpoints see
exactly what they see with the reference.  When ``net`` is the HIP ``Yolov5Network`` the returned optimizer is
``FusedSGD``: ``step()`` is ONE launch of ``sgd_nesterov_kernel`` (csrc/misc_ops.hip) over the engine's flat
parameter / gradient / momentum arenas instead of torch's foreach update over 189 tensors.  ``torch.optim.Adam`` /
``torch.optim.AdamW`` map to ``FusedAdam`` / ``FusedAdamW`` the same way (``adam_kernel``, csrc/adam.hip).
"""
from __future__ import annotations

from functools import partial
from typing import Callable, Optional

import torch
import torch.nn as nn


CLIP_ALGORITHMS = ("norm", "value")


def split_param_groups(net: nn.Module):
    """smart.py:20-35: (bias, decay, no-decay norm weights) in module-walk order."""
    bias_params, no_decay_params, decay_params = [], [], []
    bn = tuple(v for k, v in nn.__dict__.items() if "Norm" in k and isinstance(v, type))
    for v in net.modules():
        for p_name, p in v.named_parameters(recurse=False):
            if p_name == "bias":
                bias_params.append(p)
            elif p_name == "weight" and isinstance(v, bn):
                no_decay_params.append(p)
            else:
                decay_params.append(p)
    return bias_params, decay_params, no_decay_params


class FusedSGD(torch.optim.Optimizer):
    """torch.optim.SGD (momentum with or without Nesterov, dampening, maximize) over a HIP Yolov5Network: same
    param_groups / state_dict layout, the update itself is the engine's fused multi-tensor kernel.  lr / momentum /
    weight_decay are read from ``param_groups`` at every ``step()`` (so warm-up and LR schedulers work unchanged);
    dampening, nesterov and maximize are the constructor's (one value for all groups, as SmartOptimizer builds them).
    gradient_clip_val / gradient_clip_algorithm / skip_nonfinite: gradient clipping fused into ``step()`` (see __init__)."""

    def __init__(self, params, lr: float = 1e-3, momentum: float = 0.0, dampening: float = 0.0,
                 weight_decay: float = 0.0, nesterov: bool = False, *, net: nn.Module, world_size: int = 1,
                 maximize: bool = False, foreach=None, differentiable: bool = False,
                 gradient_clip_val: Optional[float] = None, gradient_clip_algorithm: str = "norm",
                 skip_nonfinite: bool = False, track_grad_norm: bool = False):
        if gradient_clip_algorithm not in CLIP_ALGORITHMS:            # (Lightning: MisconfigurationException at Trainer())
            raise ValueError(f"gradient_clip_algorithm {gradient_clip_algorithm!r}: expected one of {CLIP_ALGORITHMS}")
        if nesterov and (momentum <= 0 or dampening != 0):            # torch.optim.SGD.__init__
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        if foreach is False or differentiable:
            raise NotImplementedError("FusedSGD is the fused multi-tensor update (foreach=False / differentiable=True have no HIP form)")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                        maximize=maximize, foreach=foreach, differentiable=differentiable)
        super().__init__(params, defaults)
        self.net = net
        self.world_size = world_size
        self._nesterov = bool(nesterov)
        self._dampening, self._maximize = float(dampening), bool(maximize)
        self.steps_taken = 0          # torch keeps no momentum_buffer before the first step (checkpoint layout)
        # Lightning's Trainer(gradient_clip_val, gradient_clip_algorithm): applied inside step() - the norm reduction
        # and the SGD form that consumes its coefficient, after the 1 / world_size scale (torch's order).  Plain attributes:
        # an experiment sets them on the optimizer it gets back from a partial(torch.optim.SGD, ...), as it sets world_size
        self.gradient_clip_val, self.gradient_clip_algorithm = gradient_clip_val, gradient_clip_algorithm
        self.skip_nonfinite, self.track_grad_norm = bool(skip_nonfinite), bool(track_grad_norm)

    def _by_name(self):
        g = {pg.get("name"): pg for pg in self.param_groups}
        try:
            return [g["bias_params"], g["decay_params"], g["norm_params"]]
        except KeyError:
            raise RuntimeError("FusedSGD expects SmartOptimizer's groups bias_params / decay_params / norm_params")

    def hyper(self):
        eng = self.net.engine()                                # (the engine's device-side hyper block carries the flags)
        eng.sgd_nesterov, eng.sgd_dampening, eng.sgd_maximize = self._nesterov, self._dampening, self._maximize
        eng.sgd_steps = self.steps_taken
        g = self._by_name()
        return ([float(x["lr"]) for x in g], [float(x["momentum"]) for x in g], [float(x["weight_decay"]) for x in g])

    def clip_config(self):
        """(algorithm or None, skip_nonfinite, track_grad_norm): Engine.configure_clip's arguments"""
        if self.gradient_clip_algorithm not in CLIP_ALGORITHMS:
            raise ValueError(f"gradient_clip_algorithm {self.gradient_clip_algorithm!r}: expected one of {CLIP_ALGORITHMS}")
        return (self.gradient_clip_algorithm if self.gradient_clip_val is not None else None, self.skip_nonfinite,
                self.track_grad_norm)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lr, mom, wd = self.hyper()
        eng = self.net.engine()
        eng.configure_clip(*self.clip_config())
        eng.set_clip(self.gradient_clip_val)
        eng.sgd_step(lr, mom, wd, 1.0 / self.world_size)
        self.steps_taken += 1
        return loss

    def state_dict(self):
        """torch.optim.SGD.state_dict() layout, momentum buffers read from the engine's arena (lightning/checkpoint.py)."""
        from ...lightning.checkpoint import optimizer_state_dict
        return optimizer_state_dict(self.net, self)

    def load_state_dict(self, sd):
        from ...lightning.checkpoint import load_optimizer_state_dict
        load_optimizer_state_dict(self.net, self, sd)


class FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam (and, with decoupled_weight_decay=True, AdamW) over a HIP Yolov5Network: torch's constructor
    keywords, param_groups and state_dict layout; the update is ONE launch of adam_kernel (csrc/adam.hip) over the engine's
    flat parameter / gradient / exp_avg / exp_avg_sq arenas.  lr / betas / eps / weight_decay are read from ``param_groups``
    at every ``step()`` (warm-up and LR schedulers work unchanged); maximize and the decoupled form are the constructor's.
    The arithmetic is torch's single-tensor, non-capturable path with every operation rounded once (include/kodhip.h).

    Limits, each raised for:
    * ``0.5 <= beta1 < 1`` (ValueError otherwise): torch's ``lerp_`` takes another branch for a weight ``1 - beta1 > 0.5``,
      which the kernel has no form for; ``0 <= beta2 < 1``;
    * amsgrad=True, capturable=True, differentiable=True, foreach=False, fused=True: NotImplementedError;
    * skip_nonfinite=True: ValueError.  The step count lives on the host (the bias corrections come from
      ``steps_taken + 1``), and a step skipped on the device would not hold that count back;
    * one step count serves all tensors, so the freeze set (requires_grad) may not change once the first step has run:
      RuntimeError.  Tensors frozen from the start are supported and own no state, as with torch."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 amsgrad: bool = False, *, net: nn.Module, world_size: int = 1, foreach=None, maximize: bool = False,
                 capturable: bool = False, differentiable: bool = False, fused=None, decoupled_weight_decay: bool = False,
                 gradient_clip_val: Optional[float] = None, gradient_clip_algorithm: str = "norm",
                 skip_nonfinite: bool = False, track_grad_norm: bool = False):
        if gradient_clip_algorithm not in CLIP_ALGORITHMS:
            raise ValueError(f"gradient_clip_algorithm {gradient_clip_algorithm!r}: expected one of {CLIP_ALGORITHMS}")
        if isinstance(lr, torch.Tensor) or any(isinstance(b, torch.Tensor) for b in betas):
            raise NotImplementedError("FusedAdam takes Python floats for lr and betas (tensor values belong to capturable=True)")
        if not 0.0 <= lr:                                               # torch.optim.Adam.__init__
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        self._check_betas(betas)
        if amsgrad or capturable or differentiable or foreach is False or fused:
            raise NotImplementedError("FusedAdam is the fused multi-tensor update over the engine's arenas (amsgrad=True / "
                                      "capturable=True / differentiable=True / foreach=False / fused=True have no HIP form)")
        if skip_nonfinite:
            raise ValueError("skip_nonfinite with Adam is not supported: the bias corrections come from the host's step "
                             "count, which a step skipped on the device would not hold back")
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=maximize,
                        foreach=foreach, capturable=False, differentiable=False, fused=None)
        if self._TORCH_HAS_DECOUPLED:
            defaults["decoupled_weight_decay"] = bool(decoupled_weight_decay)
        super().__init__(params, defaults)
        self.net = net
        self.world_size = world_size
        self._maximize, self._decoupled = bool(maximize), bool(decoupled_weight_decay)
        self.steps_taken = 0          # the host's step count: the next step's bias corrections use steps_taken + 1
        self.gradient_clip_val, self.gradient_clip_algorithm = gradient_clip_val, gradient_clip_algorithm
        self.skip_nonfinite, self.track_grad_norm = False, bool(track_grad_norm)

    _TORCH_HAS_DECOUPLED = "decoupled_weight_decay" in torch.optim.Adam([torch.zeros(1)]).defaults

    @staticmethod
    def _check_betas(betas):
        b1, b2 = float(betas[0]), float(betas[1])
        if not 0.5 <= b1 < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {b1}: FusedAdam accepts 0.5 <= beta1 < 1 (torch's lerp_ takes "
                             "another branch for a weight 1 - beta1 above 0.5)")
        if not 0.0 <= b2 < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {b2}")

    def _by_name(self):
        g = {pg.get("name"): pg for pg in self.param_groups}
        try:
            return [g["bias_params"], g["decay_params"], g["norm_params"]]
        except KeyError:
            raise RuntimeError("FusedAdam expects SmartOptimizer's groups bias_params / decay_params / norm_params")

    def hyper(self):
        """What the next step uploads - Engine.set_adam_hyper's keywords (GraphedTrainStep.__call__(adam=...)): per group lr,
        betas, eps, weight_decay as they stand in param_groups, the flags, and the 1-based count of the step about to run."""
        g = self._by_name()
        for x in g:
            self._check_betas(x["betas"])
        return dict(lr=[float(x["lr"]) for x in g], betas=[(float(x["betas"][0]), float(x["betas"][1])) for x in g],
                    eps=[float(x["eps"]) for x in g], weight_decay=[float(x["weight_decay"]) for x in g],
                    step=self.steps_taken + 1, maximize=self._maximize, decoupled=self._decoupled)

    def clip_config(self):
        """(algorithm or None, skip_nonfinite, track_grad_norm): Engine.configure_clip's arguments"""
        if self.gradient_clip_algorithm not in CLIP_ALGORITHMS:
            raise ValueError(f"gradient_clip_algorithm {self.gradient_clip_algorithm!r}: expected one of {CLIP_ALGORITHMS}")
        if self.skip_nonfinite:
            raise ValueError("skip_nonfinite with Adam is not supported (the step count lives on the host)")
        return (self.gradient_clip_algorithm if self.gradient_clip_val is not None else None, False, self.track_grad_norm)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        h = self.hyper()
        eng = self.net.engine()
        eng.configure_clip(*self.clip_config())
        eng.set_clip(self.gradient_clip_val)
        eng.adam_step(**h, grad_scale=1.0 / self.world_size)
        self.steps_taken += 1
        return loss

    def state_dict(self):
        """torch.optim.Adam.state_dict() layout, the moments read from the engine's arenas (lightning/checkpoint.py)."""
        from ...lightning.checkpoint import optimizer_state_dict
        return optimizer_state_dict(self.net, self)

    def load_state_dict(self, sd):
        from ...lightning.checkpoint import load_optimizer_state_dict
        load_optimizer_state_dict(self.net, self, sd)


class FusedAdamW(FusedAdam):
    """torch.optim.AdamW: FusedAdam in its decoupled form, weight_decay default 1e-2."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 amsgrad: bool = False, **kw):
        if kw.pop("decoupled_weight_decay", True) is not True:
            raise ValueError("FusedAdamW is the decoupled form; use FusedAdam for decoupled_weight_decay=False")
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, decoupled_weight_decay=True, **kw)


class SmartOptimizer(object):
    def __init__(self, optimizer: Callable[..., torch.optim.Optimizer], weight_decay: float):
        self.partial_opt = optimizer
        self.weight_decay = weight_decay

    def _factory(self, net: nn.Module):
        """torch.optim.SGD / Adam / AdamW asked for a HIP network -> FusedSGD / FusedAdam / FusedAdamW with the same keyword
        arguments."""
        from ..networks.yolov5 import Yolov5Network
        opt = self.partial_opt
        func = getattr(opt, "func", opt)
        fused = {torch.optim.SGD: FusedSGD, FusedSGD: FusedSGD, torch.optim.Adam: FusedAdam, FusedAdam: FusedAdam,
                 torch.optim.AdamW: FusedAdamW, FusedAdamW: FusedAdamW}.get(func)
        if isinstance(net, Yolov5Network) and fused is not None:
            kw = dict(getattr(opt, "keywords", {}) or {})
            kw.pop("net", None)
            return partial(fused, *getattr(opt, "args", ()), **kw, net=net)
        return opt

    def __call__(self, net: nn.Module) -> torch.optim.Optimizer:
        bias_params, decay_params, no_decay_params = split_param_groups(net)
        optimizer = self._factory(net)(params=bias_params)                      # smart.py:36-58
        optimizer.param_groups[0]["name"] = "bias_params"
        optimizer.add_param_group(dict(params=decay_params, weight_decay=self.weight_decay, name="decay_params"))
        optimizer.add_param_group(dict(params=no_decay_params, weight_decay=0.0, name="norm_params"))
        return optimizer


def SmartSGD(net, lr: float = 0.01, momentum: float = 0.937, weight_decay: float = 5e-4, nesterov: bool = True,
             world_size: int = 1) -> FusedSGD:
    """The reference's configured optimizer (smart_sgd.yaml) in one call; `initial_lr` is pre-set like LambdaLR does."""
    opt = SmartOptimizer(partial(FusedSGD, lr=lr, momentum=momentum, nesterov=nesterov, net=net, world_size=world_size),
                         weight_decay)(net)
    for pg in opt.param_groups:
        pg.setdefault("initial_lr", pg["lr"])
    return opt


def SmartAdamW(net, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
               world_size: int = 1) -> FusedAdamW:
    """AdamW over the reference's three groups in one call (decay on decay_params only, as SmartOptimizer builds them);
    `initial_lr` is pre-set like LambdaLR does."""
    opt = SmartOptimizer(partial(FusedAdamW, lr=lr, betas=betas, eps=eps, weight_decay=0.0, net=net, world_size=world_size),
                         weight_decay)(net)
    for pg in opt.param_groups:
        pg.setdefault("initial_lr", pg["lr"])
    return opt
