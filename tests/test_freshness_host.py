"""engine/freshness.py on CPU tensors: the key that decides when the weight packs and the eval-mode BatchNorm constants
are rebuilt moves after every way torch code edits a Parameter or a BatchNorm buffer that was re-pointed into an arena
the way Engine._build_arenas does it, and stays put when nothing was edited."""
import copy

import pytest
import torch
import torch.nn as nn

from object_detection_cib_amd.engine.freshness import freshness_key, track_data_edits


class _Bound:
    """conv + BatchNorm holders bound into flat arenas as in engine/arenas.py _build_arenas"""

    def __init__(self):
        torch.manual_seed(0)
        self.mod = nn.Sequential(nn.Conv2d(4, 8, 3, bias=True), nn.BatchNorm2d(8))
        self.p_arena = torch.zeros(1024)
        self.rm_arena, self.rv_arena = torch.zeros(16), torch.ones(16)
        off = 0
        with torch.no_grad():
            for p in self.mod.parameters():
                k = p.numel()
                self.p_arena[off:off + k].copy_(p.detach().reshape(-1))
                p.data = self.p_arena[off:off + k].view(p.shape)
                track_data_edits(p)
                off += (k + 63) // 64 * 64
            bn = self.mod[1]
            for b, arena in ((bn.running_mean, self.rm_arena), (bn.running_var, self.rv_arena)):
                arena[:8].copy_(b)
                b.data = arena[:8]
        self.param_version = self.stats_version = 0
        self.params = [self.p_arena] + list(self.mod.parameters())
        self.stats = [self.rm_arena, self.rv_arena, bn.running_mean, bn.running_var]

    def key(self):
        return freshness_key(self.param_version, self.stats_version, self.params, self.stats)


def _sgd_step(s):
    for p in s.mod.parameters():
        p.grad = torch.ones_like(p)
    torch.optim.SGD(s.mod.parameters(), lr=0.1).step()


def _no_grad_mul(s):
    with torch.no_grad():
        s.mod[0].weight.mul_(1.5)


def _load_state_dict(s):
    s.mod.load_state_dict({k: v.clone() + 1 for k, v in s.mod.state_dict().items()})


PARAM_EDITS = {
    "no_grad_mul": _no_grad_mul,
    "data_mul": lambda s: s.mod[0].weight.data.mul_(2),
    "data_copy": lambda s: s.mod[0].bias.data.copy_(torch.ones(8)),
    "init_normal": lambda s: nn.init.normal_(s.mod[0].weight, std=0.05),
    "torch_sgd": _sgd_step,
    "load_state_dict": _load_state_dict,
    "arena_copy": lambda s: s.p_arena.copy_(torch.ones(1024)),
    "engine_counter": lambda s: setattr(s, "param_version", s.param_version + 1),
}
STAT_EDITS = {
    "reset_running_stats": lambda s: s.mod[1].reset_running_stats(),
    "running_var_copy": lambda s: s.mod[1].running_var.copy_(torch.full((8,), 2.0)),
    "rm_arena_copy": lambda s: s.rm_arena.copy_(torch.ones(16)),
    "engine_counter": lambda s: setattr(s, "stats_version", s.stats_version + 1),
}


@pytest.mark.parametrize("name", sorted(PARAM_EDITS))
def test_parameter_edit_moves_the_parameter_half(name):
    s = _Bound()
    k0 = s.key()
    before = s.p_arena.clone()
    PARAM_EDITS[name](s)
    if name != "engine_counter":
        assert not torch.equal(s.p_arena, before), "the edit must reach the arena, or the case is vacuous"
    k1 = s.key()
    assert k1[0] > k0[0], (name, k0, k1)
    assert s.key() == k1                              # reading the key moves nothing


@pytest.mark.parametrize("name", sorted(STAT_EDITS))
def test_statistic_edit_moves_the_statistics_half_only(name):
    s = _Bound()
    s.rm_arena[:8] = 0.5                              # (so that reset_running_stats changes something)
    k0 = s.key()
    before = torch.cat((s.rm_arena, s.rv_arena)).clone()
    STAT_EDITS[name](s)
    if name != "engine_counter":
        assert not torch.equal(torch.cat((s.rm_arena, s.rv_arena)), before)
    k1 = s.key()
    assert k1[1] > k0[1] and k1[0] == k0[0], (name, k0, k1)


def test_no_op_keeps_the_key():
    s = _Bound()
    k0 = s.key()
    w = s.mod[0].weight
    _ = w.detach().clone(), w.data.sum(), (w * 2).sum(), s.p_arena[:8] + 1, s.mod.state_dict(), w.data.shape
    s.mod.train(); s.mod.eval(); s.mod.requires_grad_(False); s.mod.requires_grad_(True)
    s.mod.zero_grad(set_to_none=True)
    assert s.key() == k0


def test_tracked_parameter_stays_a_parameter():
    """track_data_edits changes what `.data` hands out and nothing else a module, an optimizer or a checkpoint relies on"""
    s = _Bound()
    w = s.mod[0].weight
    assert isinstance(w, nn.Parameter) and w.requires_grad and w.is_leaf
    d = w.data
    assert type(d) is torch.Tensor and not d.requires_grad and d.data_ptr() == w.data_ptr()
    assert dict(s.mod.named_parameters())["0.weight"] is w
    new = torch.full_like(w, 3.0)
    w.data = new                                      # rebinding still goes through torch's setter
    assert w.data_ptr() == new.data_ptr() and torch.equal(w.detach(), new)
    c = copy.deepcopy(s.mod)
    assert torch.equal(c[0].weight.detach(), new) and c[0].weight.data_ptr() != new.data_ptr()
    assert isinstance(c[0].weight, nn.Parameter) and c[0].weight.requires_grad
    import io
    buf = io.BytesIO()
    torch.save({"sd": s.mod.state_dict(), "p": w}, buf)
    buf.seek(0)
    back = torch.load(buf, weights_only=False)
    assert type(back["sd"]["0.weight"]) is torch.Tensor and torch.equal(back["sd"]["0.weight"], new)
    assert isinstance(back["p"], nn.Parameter) and torch.equal(back["p"].detach(), new)
    # an edit through .data under autograd: the loss below saves no parameter-dependent tensor of w itself
    (s.mod[0].bias * 2).sum().backward()
    s.mod[0].bias.data.add_(1.0)
    assert torch.equal(s.mod[0].bias.grad, torch.full((8,), 2.0))
    b = torch.zeros(3)
    assert track_data_edits(b) is b and type(b) is torch.Tensor          # only exact Parameters are touched
