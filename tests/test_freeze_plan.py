"""CPU checks of the freeze plan (engine/freeze.py): which gradients a training step forms when parameters are frozen."""
import pytest

from object_detection_cib_amd.engine.graph import build_graph, head_param
from object_detection_cib_amd.engine.freeze import build_freeze_plan, trainable_span, unit_param_names, HEAD_KEYS
from object_detection_cib_amd.engine.ddp import plan_buckets


def _g():
    return build_graph(3, 10, 0.5, 0.33)           # yv5s


def _names(g):
    out = []
    for u in g.units:
        out.extend(unit_param_names(u))
    for h in g.heads:
        out.extend(head_param(h, k, w) for w in ("weight", "bias") for k in HEAD_KEYS)
    return out


def _plan(g, frozen=lambda n: False):
    return build_freeze_plan(g, {n: not frozen(n) for n in _names(g)})


def _layout(g):
    """the engine's own arena layout (engine/arenas.py arena_layout) over the network's parameters"""
    from object_detection_cib_amd.engine.arenas import arena_layout
    from object_detection_cib_amd.nn.networks.yolov5 import Yolov5Network
    net = Yolov5Network(3, 10, widen_factor=0.5, deepen_factor=0.33)
    layout, _gid, n, starts = arena_layout(g, {k: p.numel() for k, p in net.named_parameters()})
    return layout, starts, n


def test_default_plan():
    g = _g()
    p = _plan(g)
    assert p.is_default and not p.frozen
    assert all(f.needs_out_grad for f in p.units.values())
    assert all(f.needs_in_grad for u in g.units if not u.stem for f in [p.units[u.name]])
    assert not p.units["backbone.stem"].needs_in_grad
    assert all(h.needs_out_grad and h.needs_in_grad for h in p.heads.values())
    assert _plan(g).key == p.key


def test_frozen_backbone_is_the_no_grad_region():
    g = _g()
    p = _plan(g, lambda n: n.startswith("backbone."))
    assert not p.is_default
    for u in g.units:
        f = p.units[u.name]
        if u.name.startswith("backbone."):
            assert not f.needs_out_grad and not f.needs_in_grad and not f.trainable, u.name
            assert not p.unit_runs(u), u.name
        else:
            assert f.needs_out_grad and f.w_trainable, u.name
    # the neck's CSP entries read concat buffers holding a backbone output and a neck value: they still need dX
    assert p.units["neck.top_down_layers.0.0.main_conv"].needs_in_grad
    assert p.units["neck.top_down_layers.1.main_conv"].needs_in_grad
    # the 1x1 reduce conv reads P5 (backbone only): no data gradient
    assert not p.units["neck.reduce_layers.2"].needs_in_grad
    # SPPF pools sit in the backbone: nothing upstream needs their gradient
    assert not any(ok for op, ok in zip(g.ops, p.op_in_grad) if op.kind == "pool")
    assert all(ok for op, ok in zip(g.ops, p.op_in_grad) if op.kind == "up")


def test_only_stem_frozen():
    g = _g()
    p = _plan(g, lambda n: n.startswith("backbone.stem."))
    f = p.units["backbone.stem"]
    assert not f.w_trainable and not f.needs_out_grad and not f.needs_in_grad
    # the first 3x3 s2 conv is trainable but its input (the stem's output) needs no gradient
    s1 = p.units["backbone.stages.stage1.blocks.0"]
    assert s1.needs_out_grad and s1.w_trainable and not s1.needs_in_grad
    for u in g.units:
        if u.name not in ("backbone.stem", "backbone.stages.stage1.blocks.0"):
            assert p.units[u.name] == _plan(g).units[u.name], u.name


def test_frozen_neck_keeps_data_gradients():
    g = _g()
    p = _plan(g, lambda n: n.startswith("neck."))
    for u in g.units:
        f = p.units[u.name]
        if u.name.startswith("neck."):
            assert not f.w_trainable and f.bn_trainable == (False, False) and f.needs_out_grad and f.needs_in_grad, u.name
        else:
            assert f.needs_out_grad and f.trainable
    assert all(ok for op, ok in zip(g.ops, p.op_in_grad) if not (op.kind == "conv" and op.unit.stem))


def test_single_head_cls_frozen():
    g = _g()
    name = head_param(g.heads[1], "cls", "weight")
    p = _plan(g, lambda n: n == name)
    assert p.frozen == (name,)
    h = p.heads[g.heads[1].name]
    assert h.w_trainable == (True, True, False) and h.b_trainable == (True, True, True) and h.needs_out_grad
    assert all(f == _plan(g).units[n] for n, f in p.units.items())
    assert p.key != _plan(g).key


def test_mid_conv_weight_and_bn_affine():
    g = _g()
    w = "backbone.stages.stage2.blocks.1.blocks.0.conv1.0.weight"
    p = _plan(g, lambda n: n == w)
    f = p.units["backbone.stages.stage2.blocks.1.blocks.0.conv1"]
    assert not f.w_trainable and f.bn_trainable == (True, True) and f.needs_out_grad and f.needs_in_grad
    b = "neck.reduce_layers.2.1.bias"
    f = _plan(g, lambda n: n == b).units["neck.reduce_layers.2"]
    assert f.w_trainable and f.bn_trainable == (True, False) and f.needs_out_grad


def test_all_frozen_raises_on_backward():
    g = _g()
    p = _plan(g, lambda n: True)
    assert not p.any_trainable and not any(f.needs_out_grad for f in p.units.values())
    with pytest.raises(RuntimeError, match="does not require grad"):
        p.require_trainable()
    _plan(g).require_trainable()


def test_buckets_tile_the_trainable_span():
    g = _g()
    layout, starts, n = _layout(g)
    p = _plan(g, lambda n_: n_.startswith("backbone."))
    first = trainable_span(starts, p, layout)
    lo_train = min(layout[x][0] for x in p.trainable)
    assert starts[first] == lo_train == layout["neck.reduce_layers.2.0.weight"][0]
    for elems in (1, 4096, 1 << 16, 1 << 30):
        bk = plan_buckets(starts, n, elems, first)
        assert bk[0][2] == n and bk[-1][1] == lo_train and bk[-1][0] == first
        for (_, lo, _), (_, _, hi) in zip(bk, bk[1:]):
            assert lo == hi                                 # contiguous, back to front
        assert all(t >= first for t, _, _ in bk)
    # the default tiles the whole arena, as before
    assert plan_buckets(starts, n, 4096) == plan_buckets(starts, n, 4096, trainable_span(starts, _plan(g), layout))
    assert plan_buckets(starts, n, 4096)[-1][1] == 0
    assert trainable_span(starts, _plan(g, lambda n_: True), layout) == -1


# ---------------------------------------------------------------------------------------------- group_launches
def _groups(g, dual, pair_all=False):
    """backward's unit groups: reversed op list, [short_conv, main_conv] where the pair shares a launch (a dual data
    gradient; pair_all: every sibling pair, as under RCCL SyncBN)"""
    rops, ri, out = list(reversed(g.ops)), 0, []
    while ri < len(rops):
        op = rops[ri]
        ri += 1
        if op.kind != "conv":
            continue
        grp = [op.unit]
        if ri < len(rops) and rops[ri].kind == "conv" and rops[ri].unit.sibling is op.unit and \
                (pair_all or rops[ri].unit.name in dual):
            grp.append(rops[ri].unit)
            ri += 1
        out.append(grp)
    return out


def _launches(g, plan, dual, grp, wg_dual=True):
    """group_launches with the partner written as its name"""
    from object_detection_cib_amd.engine.freeze import group_launches
    out = group_launches(grp, plan, dual, wg_dual and len(grp) == 2)
    return [None if ln is None else (ln.dgrad, ln.partner.name if ln.partner is not None else None, ln.dual_w, ln.w_grad,
                                     ln.res_grad) for ln in out]


@pytest.mark.parametrize("dual_on", [True, False])
@pytest.mark.parametrize("pair_all", [False, True])
@pytest.mark.parametrize("wg_dual", [True, False])
def test_group_launches_without_a_plan_equal_the_default_plan(dual_on, pair_all, wg_dual):
    from object_detection_cib_amd.engine.plan import plan_dual_dgrads
    g = _g()
    dual = set(plan_dual_dgrads(g)) if dual_on else set()
    default = _plan(g)
    assert default.is_default
    groups = _groups(g, dual, pair_all)
    assert sum(len(grp) for grp in groups) == len([op for op in g.ops if op.kind == "conv"])
    for grp in groups:
        got = _launches(g, None, dual, grp, wg_dual)
        assert got == _launches(g, default, dual, grp, wg_dual), [u.name for u in grp]
        assert all(ln is not None and ln[3] for ln in got)                    # every unit runs, every weight gradient
        if len(grp) == 2 and grp[1].name in dual:
            assert [ln[0] for ln in got] == ["skip", "dual"] and got[1][1] == grp[0].name
            assert got[0][2] == got[1][2] == wg_dual
        else:
            assert [ln[0] for ln in got] == ["none" if u.stem else "own" for u in grp]
            assert not any(ln[2] for ln in got)


def test_group_launches_under_freeze_plans():
    """Where a plan's answer differs from the default's, written out; the values are what the engine's separate
    freeze-plan path handed to the unit launches for the same plans before the default and the freeze path became one."""
    from object_detection_cib_amd.engine.plan import plan_dual_dgrads
    g = _g()
    dual = set(plan_dual_dgrads(g))
    default = _plan(g)
    groups = _groups(g, dual)
    bb = [tuple(u.name for u in grp) for grp in groups if grp[0].name.startswith("backbone.")]
    S1 = "backbone.stages.stage1.blocks.1."
    TD = "neck.top_down_layers.1."
    cases = {
        # no data gradient where needs_in_grad is false, nothing at all in the no-grad region (the tick stays: None)
        "backbone": (lambda n: n.startswith("backbone."),
                     {("neck.reduce_layers.2",): [("none", None, False, True, False)],
                      **{names: [None] * len(names) for names in bb}}),
        "stem": (lambda n: n.startswith("backbone.stem."),
                 {("backbone.stages.stage1.blocks.0",): [("none", None, False, True, False)],
                  ("backbone.stem",): [None]}),
        "mid_conv_weight": (lambda n: n == "backbone.stages.stage2.blocks.1.blocks.0.conv1.0.weight",
                            {("backbone.stages.stage2.blocks.1.blocks.0.conv1",): [("own", None, False, False, False)]}),
        # one weight of a pair frozen: the dual data gradient stays, the dual weight gradient does not
        "short_weight": (lambda n: n == TD + "short_conv.0.weight",
                         {(TD + "short_conv", TD + "main_conv"): [("skip", None, False, False, False),
                                                                  ("dual", TD + "short_conv", False, True, False)]}),
        # one partner of a pair outside the grad region: the other takes the single forms
        "entry_and_short": (lambda n: n.startswith(("backbone.stem.", "backbone.stages.stage1.blocks.0.", S1 + "short_conv.")),
                            {(S1 + "short_conv", S1 + "main_conv"): [None, ("none", None, False, True, False)],
                             ("backbone.stages.stage1.blocks.0",): [None], ("backbone.stem",): [None]}),
    }
    assert len(bb) == 29
    for key, (frozen, want) in cases.items():
        plan = _plan(g, frozen)
        differs = {}
        for grp in groups:
            got = _launches(g, plan, dual, grp)
            if got != _launches(g, default, dual, grp):
                differs[tuple(u.name for u in grp)] = got
        assert differs == want, key
