"""Checkpoint wire format: Lightning `.ckpt` envelopes with the reference's layout.

The reference trains a LightningModule `DefaultYolov5Experiment` whose network is the attribute `net`
(kod/lightning/experiments/yv5_baseline/exp.py:36-58) and checkpoints it with lightning's ModelCheckpoint
(kod/configs/callbacks/model_checkpoint.yaml, kod/lightning/tasks/trainer.py:122-137).  A `.ckpt` is a
`torch.save`d dict; the entries a resume / README eval command needs are

    state_dict         {"net." + key: tensor}  - the network's 360 keys (yv5s), fp32
    optimizer_states   [torch.optim.SGD.state_dict()] for the optimizer SmartOptimizer builds
                       (kod/nn/optim/smart.py:20-60): groups bias_params | decay_params | norm_params, parameters
                       numbered consecutively group by group in module-walk order, state[i]["momentum_buffer"];
                       for FusedAdam / FusedAdamW torch.optim.Adam.state_dict(): state[i] = {"step" (float32 scalar
                       tensor), "exp_avg", "exp_avg_sq"}
    lr_schedulers      [LambdaLR.state_dict()]
    epoch, global_step, pytorch-lightning_version

Here the parameters / momentum live in the engine's flat arenas, so this module maps between the two.
Host-only Python (checkpoint I/O stays Python per the north star).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

GROUP_NAMES = ("bias_params", "decay_params", "norm_params")
NET_PREFIX = "net."
LIGHTNING_VERSION = "2.0.9"


def optimizer_param_order(net: nn.Module) -> Tuple[List[str], List[str], List[str]]:
    """Parameter names per optimizer group in the order SmartOptimizer.__call__ collects them (smart.py:20-35)."""
    norm_types = tuple(v for k, v in nn.__dict__.items() if "Norm" in k and isinstance(v, type))
    bias, decay, norm = [], [], []
    for mod_name, m in net.named_modules():
        for p_name, _ in m.named_parameters(recurse=False):
            full = f"{mod_name}.{p_name}" if mod_name else p_name
            if p_name == "bias":
                bias.append(full)
            elif p_name == "weight" and isinstance(m, norm_types):
                norm.append(full)
            else:
                decay.append(full)
    return bias, decay, norm


def _is_adam(optimizer) -> bool:
    from ..nn.optim.smart import FusedAdam
    return isinstance(optimizer, FusedAdam)


def adam_param_group(g: Dict, ids: List[int]) -> Dict:
    """One param_groups entry with the keys of the installed torch.optim.Adam(...).state_dict(), plus name and initial_lr."""
    ref = torch.optim.Adam([torch.zeros(1)]).state_dict()["param_groups"][0]
    out = {}
    for k, default in ref.items():
        if k != "params":
            out[k] = g.get(k, default)
    out["lr"], out["eps"], out["weight_decay"] = float(g["lr"]), float(g["eps"]), float(g["weight_decay"])
    out["betas"] = (float(g["betas"][0]), float(g["betas"][1]))
    out["name"] = g["name"]
    out["initial_lr"] = float(g.get("initial_lr", g["lr"]))
    out["params"] = ids
    return out


def adam_state_dict(groups, param_groups, shapes: Dict, layout: Dict, exp_avg, exp_avg_sq, steps_taken: int, frozen=()) -> Dict:
    """torch.optim.Adam.state_dict() layout from flat arenas (any device; a test may pass CPU tensors): per stepped tensor
    {"step": float32 scalar tensor, "exp_avg", "exp_avg_sq"}; before the first step, and for a tensor frozen from the start,
    no state - as with torch.  groups: parameter names per group (optimizer_param_order), layout: name -> (offset, numel)."""
    state, pgs, idx = {}, [], 0
    for names, g in zip(groups, param_groups):
        ids = []
        for n in names:
            if steps_taken > 0 and n not in frozen:
                off, numel = layout[n]
                state[idx] = {"step": torch.tensor(float(steps_taken), dtype=torch.float32),
                              "exp_avg": exp_avg[off:off + numel].view(shapes[n]).detach().clone().cpu(),
                              "exp_avg_sq": exp_avg_sq[off:off + numel].view(shapes[n]).detach().clone().cpu()}
            ids.append(idx)
            idx += 1
        pgs.append(adam_param_group(g, ids))
    return {"state": state, "param_groups": pgs}


def _adam_optimizer_state_dict(net, optimizer) -> Dict:
    groups = optimizer_param_order(net)
    shapes = {n: tuple(p.shape) for n, p in net.named_parameters()}
    steps = int(getattr(optimizer, "steps_taken", 0))
    if steps == 0:
        return adam_state_dict(groups, optimizer.param_groups, shapes, {}, None, None, 0)
    eng = net.engine()
    return adam_state_dict(groups, optimizer.param_groups, shapes, eng.layout, eng.m_arena, eng.v_arena, steps,
                           eng.adam_frozen or ())


def _load_adam_optimizer_state_dict(net, optimizer, sd: Dict):
    """The reverse of adam_state_dict: moments into the arenas, the step count into the optimizer.  One count serves all
    tensors, so the stepped tensors must agree on it; tensors without state are the set frozen from the start."""
    groups = optimizer_param_order(net)
    params = dict(net.named_parameters())
    assert len(sd["param_groups"]) == 3, "expected SmartOptimizer's three parameter groups"
    eng = net.engine()
    eng.configure_adam()
    eng.m_arena.zero_()
    eng.v_arena.zero_()
    steps, got = set(), set()
    for names, g_saved, g in zip(groups, sd["param_groups"], optimizer.param_groups):
        assert len(names) == len(g_saved["params"]), (g_saved.get("name"), len(names), len(g_saved["params"]))
        for key in ("lr", "betas", "eps", "weight_decay", "initial_lr"):
            if key in g_saved:
                g[key] = tuple(g_saved[key]) if key == "betas" else g_saved[key]
        for n, i in zip(names, g_saved["params"]):
            st = sd["state"].get(i, sd["state"].get(str(i)))
            if not st:
                continue
            off, numel = eng.layout[n]
            for key, arena in (("exp_avg", eng.m_arena), ("exp_avg_sq", eng.v_arena)):
                buf = st[key]
                assert tuple(buf.shape) == tuple(params[n].shape), (n, key, buf.shape, params[n].shape)
                arena[off:off + numel].copy_(buf.reshape(-1).to(arena.device, torch.float32))
            steps.add(int(float(st["step"])))
            got.add(n)
    if len(steps) > 1:
        raise RuntimeError(f"the Adam state holds different step counts {sorted(steps)}: the fused Adam keeps one count for all "
                           "tensors (a freeze set that changed during training is not supported)")
    optimizer.steps_taken = steps.pop() if steps else 0
    eng.adam_steps = optimizer.steps_taken
    eng.adam_frozen = frozenset(n for n in eng.layout if n not in got) if got else None
    eng._adam_vals = None
    return len(got)


def optimizer_state_dict(net, optimizer) -> Dict:
    """torch.optim.SGD.state_dict() layout for a SmartSGD over `net` (momentum read from the engine's arena); for a FusedAdam
    / FusedAdamW torch.optim.Adam's (both moments and the step count)."""
    if _is_adam(optimizer):
        return _adam_optimizer_state_dict(net, optimizer)
    groups = optimizer_param_order(net)
    params = dict(net.named_parameters())
    eng = net.engine() if getattr(optimizer, "steps_taken", 0) > 0 else None
    state, pgs, idx = {}, [], 0
    for names, g in zip(groups, optimizer.param_groups):
        ids = []
        for n in names:
            if eng is not None and (eng.stepped is None or n in eng.stepped):      # (torch: frozen = never stepped, no state)
                off, numel = eng.layout[n]
                state[idx] = {"momentum_buffer": eng.m_arena[off:off + numel].view(params[n].shape).detach().clone().cpu()}
            ids.append(idx)
            idx += 1
        # (dampening / nesterov / maximize are the optimizer's own: a plain torch.optim.SGD that loads this steps the same way)
        pgs.append(dict(lr=float(g["lr"]), momentum=float(g["momentum"]), dampening=g.get("dampening", 0),
                        weight_decay=float(g["weight_decay"]), nesterov=bool(g.get("nesterov", True)),
                        maximize=bool(g.get("maximize", False)), foreach=None, differentiable=False, name=g["name"],
                        initial_lr=float(g.get("initial_lr", g["lr"])), params=ids))
    return {"state": state, "param_groups": pgs}


def load_optimizer_state_dict(net, optimizer, sd: Dict):
    if _is_adam(optimizer):
        return _load_adam_optimizer_state_dict(net, optimizer, sd)
    groups = optimizer_param_order(net)
    params = dict(net.named_parameters())
    assert len(sd["param_groups"]) == 3, "expected SmartOptimizer's three parameter groups"
    eng = net.engine()
    eng.m_arena.zero_()
    loaded = 0
    for names, g_saved, g in zip(groups, sd["param_groups"], optimizer.param_groups):
        assert len(names) == len(g_saved["params"]), (g_saved.get("name"), len(names), len(g_saved["params"]))
        for key in ("lr", "momentum", "weight_decay", "initial_lr"):
            if key in g_saved:
                g[key] = g_saved[key]
        for n, i in zip(names, g_saved["params"]):
            st = sd["state"].get(i, sd["state"].get(str(i)))
            if st is None or st.get("momentum_buffer") is None:
                continue
            buf = st["momentum_buffer"]
            assert tuple(buf.shape) == tuple(params[n].shape), (n, buf.shape, params[n].shape)
            off, numel = eng.layout[n]
            eng.m_arena[off:off + numel].copy_(buf.reshape(-1).to(eng.m_arena.device, torch.float32))
            loaded += 1
    optimizer.steps_taken = 1 if loaded else 0
    keys = [n for names in groups for n in names]
    got = {n for names, g_saved in zip(groups, sd["param_groups"]) for n, i in zip(names, g_saved["params"])
           if (sd["state"].get(i, sd["state"].get(str(i))) or {}).get("momentum_buffer") is not None}
    eng.stepped = None if len(got) == len(keys) else got        # the same state layout is written back
    eng._stepped_key = None
    return loaded


MULTI_SCALE_KEY = "multi_scale_schedule"
EMA_KEY = "ema"


def save_checkpoint(path: str, net, optimizer=None, epoch: int = 0, global_step: int = 0,
                    lr_scheduler_state: Optional[Dict] = None, extra: Optional[Dict] = None,
                    multi_scale_state: Optional[Dict] = None, ema_state: Optional[Dict] = None) -> Dict:
    """multi_scale_state: the multi-scale size schedule's state_dict (MultiScaleSchedule / MultiScaleTrainStep /
    DefaultYolov5Experiment.multi_scale_state_dict), stored under MULTI_SCALE_KEY; left out, the file has no such key.
    ema_state: the weight EMA's state (ModelEMA.ema_state_dict / DefaultYolov5Experiment.ema_state_dict: updates, decay, tau and
    the EMA's own state dict), stored under EMA_KEY; left out, the file has no such key."""
    ckpt = {
        "epoch": int(epoch), "global_step": int(global_step), "pytorch-lightning_version": LIGHTNING_VERSION,
        "state_dict": {NET_PREFIX + k: v.detach().clone().cpu() for k, v in net.state_dict().items()},
        "loops": {}, "callbacks": {},
        "optimizer_states": [optimizer_state_dict(net, optimizer)] if optimizer is not None else [],
        "lr_schedulers": [lr_scheduler_state] if lr_scheduler_state is not None else [],
    }
    if multi_scale_state is not None:
        ckpt[MULTI_SCALE_KEY] = dict(multi_scale_state)
    if ema_state is not None:
        ckpt[EMA_KEY] = dict(ema_state)
    if extra:
        ckpt.update(extra)
    torch.save(ckpt, path)
    return ckpt


def load_checkpoint(path: str, net, optimizer=None, strict: bool = True, multi_scale=None, ema=None) -> Dict:
    """Loads the network (and optimizer) from a reference-layout `.ckpt`; returns the remaining entries.
    multi_scale: an object with load_state_dict (MultiScaleSchedule, MultiScaleTrainStep) or a DefaultYolov5Experiment
    (load_multi_scale_state_dict) that takes the size schedule's state when the file carries one; a file without the key
    loads as before and leaves it untouched.
    ema: a ModelEMA or a DefaultYolov5Experiment(ema=True) (both have load_ema_state_dict) that takes the weight EMA's state
    when the file carries one; a file without the key leaves it untouched."""
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    if multi_scale is not None and ckpt.get(MULTI_SCALE_KEY) is not None:
        load = getattr(multi_scale, "load_multi_scale_state_dict", None) or multi_scale.load_state_dict
        load(ckpt[MULTI_SCALE_KEY])
    if ema is not None and ckpt.get(EMA_KEY) is not None:
        ema.load_ema_state_dict(ckpt[EMA_KEY])
    sd = ckpt["state_dict"]
    net_sd = {k[len(NET_PREFIX):]: v for k, v in sd.items() if k.startswith(NET_PREFIX)}
    if not net_sd:                      # a bare network state_dict (README-style weight files)
        net_sd = sd
    net.load_state_dict(net_sd, strict=strict)
    if optimizer is not None and ckpt.get("optimizer_states"):
        load_optimizer_state_dict(net, optimizer, ckpt["optimizer_states"][0])
    return {k: v for k, v in ckpt.items() if k not in ("state_dict", "optimizer_states")}
