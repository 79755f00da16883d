"""CPU checks of the BatchNorm mode plan (engine/bn_mode.py): which units of a training forward normalise with their
running statistics, and how backward forms their coefficients; plus the argument checks of the eval-mode exports."""
import pytest

from object_detection_cib_amd.engine.graph import build_graph
from object_detection_cib_amd.engine.freeze import build_freeze_plan, unit_param_names
from object_detection_cib_amd.engine.bn_mode import (build_bn_mode_plan, coef_kind, coef_launches, conv_units,
                                                     eval_constant_units, TRAIN, EVAL, NONE)


def _g():
    return build_graph(3, 10, 0.5, 0.33)           # yv5s


def _modes(g, eval_=lambda n: False):
    return build_bn_mode_plan(g, {n: not eval_(n) for n in conv_units(g)})


def _frozen(g, frozen):
    names = [n for u in g.units for n in unit_param_names(u)]
    return build_freeze_plan(g, {n: not frozen(n) for n in names})


def _pair(g):
    main = next(op.unit for op in g.ops if op.kind == "conv" and op.unit.sibling is not None)
    return main, main.sibling


def test_default_plan_for_an_empty_eval_set():
    g = _g()
    p = _modes(g)
    assert p.is_default and p.key == () and not p.eval_units
    assert p.any_train and p.train_mask() == (1,) * len(conv_units(g))
    assert build_bn_mode_plan(g, {}).is_default            # no modules registered: every unit in train mode
    assert p.key == _modes(g).key


def test_key_changes_with_the_eval_set():
    g = _g()
    bb = _modes(g, lambda n: n.startswith("backbone."))
    stem = _modes(g, lambda n: n == "backbone.stem")
    assert not bb.is_default and not stem.is_default
    assert len({(), bb.key, stem.key}) == 3
    assert stem.key == ("backbone.stem",)
    assert all(n.startswith("backbone.") for n in bb.key)
    assert list(bb.key) == [n for n in conv_units(g) if n.startswith("backbone.")]      # program order
    mask = bb.train_mask()
    assert [m for n, m in zip(conv_units(g), mask)] == [0 if n.startswith("backbone.") else 1 for n in conv_units(g)]
    every = _modes(g, lambda n: True)
    assert not every.any_train and sum(every.train_mask()) == 0


def test_forward_statistic_groups_drop_eval_units():
    g = _g()
    main, short = _pair(g)
    p = _modes(g, lambda n: n == short.name)
    assert p.stat_group([main, short]) == [main]
    assert p.stat_group([short]) == []
    assert _modes(g).stat_group([main, short]) == [main, short]


def test_sibling_pair_with_mixed_modes():
    g = _g()
    main, short = _pair(g)
    names = [short.name, main.name]                        # backward order: short_conv first
    p = _modes(g, lambda n: n == short.name)
    # one two-unit launch with a mode per job without SyncBN
    assert coef_launches(p, None, names, sync=False) == [("mode2", tuple(names), (1, 0))]
    # under SyncBN: the eval unit alone, the train unit through the exchange
    assert coef_launches(p, None, names, sync=True) == [("eval", (short.name,), (1,)), ("train", (main.name,), (0,))]
    both = _modes(g, lambda n: n in names)
    assert coef_launches(both, None, names, sync=False) == [("mode2", tuple(names), (1, 1))]
    assert coef_launches(both, None, names, sync=True) == [("eval", (names[0],), (1,)), ("eval", (names[1],), (1,))]
    # the default grouping stays the train pair
    assert coef_launches(_modes(g, lambda n: n == "backbone.stem"), None, names, sync=False) == \
        [("train", tuple(names), (0, 0))]


def test_frozen_affine_eval_units_launch_no_coefficients():
    g = _g()
    main, short = _pair(g)
    names = [short.name, main.name]
    p = _modes(g, lambda n: n.startswith("backbone."))
    fz = _frozen(g, lambda n: n.startswith("backbone."))
    assert coef_kind(p, fz, short.name) == NONE and coef_kind(p, None, short.name) == EVAL
    neck = next(n for n in conv_units(g) if not n.startswith("backbone."))
    assert coef_kind(p, fz, neck) == TRAIN
    assert coef_launches(p, fz, names, sync=False) == []
    assert coef_launches(p, fz, names, sync=True) == []
    # gamma frozen, beta trainable: the eval-mode kernel still forms dbeta
    fz_g = _frozen(g, lambda n: n == short.name + ".1.weight")
    assert coef_kind(p, fz_g, short.name) == EVAL
    # a frozen-affine eval unit beside a train unit: the train unit's own launch only
    p1 = _modes(g, lambda n: n == short.name)
    fz1 = _frozen(g, lambda n: n.startswith(short.name + ".1."))
    assert coef_launches(p1, fz1, names, sync=False) == [("train", (main.name,), (0,))]
    # the forward's eval-constants launch writes the coefficients of exactly those units
    ev = dict(eval_constant_units(p, fz))
    assert set(ev) == set(p.key) and all(ev.values())
    ev = dict(eval_constant_units(p, fz_g))
    assert not ev[short.name] and not ev[main.name]


@pytest.fixture(scope="module")
def lib():
    from object_detection_cib_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


def test_eval_exports_validate_arguments(lib):
    assert lib.kodhip_bn_eval_desc_bytes() == 64
    rc = lib.kodhip_bn_eval_constants(None, 3, 1e-3, None)
    assert rc < 0 and b"bn_eval_constants" in lib.kodhip_last_error()
    rc = lib.kodhip_bn_eval_constants(16, 0, 1e-3, None)
    assert rc < 0 and b"bn_eval_constants" in lib.kodhip_last_error()
    rc = lib.kodhip_bn_bwd_coeffs_eval_partials(None, 4, None, None, None, None, None, None, 8, 0, None)
    assert rc < 0 and b"bn_bwd_coeffs_eval_partials" in lib.kodhip_last_error()
    job = [16, 4, 0.0, 16, 16, 16, 16, 16, 16, 8, 0]
    # count is needed by a train-mode job only
    rc = lib.kodhip_bn_bwd_coeffs_eval_partials2(*job, 0, *job, 1, None)
    assert rc < 0 and b"bn_bwd_coeffs_eval_partials2" in lib.kodhip_last_error()
    rc = lib.kodhip_bn_bwd_coeffs_eval_partials2(*(job[:9] + [0, 0]), 1, *job, 1, None)
    assert rc < 0 and b"bn_bwd_coeffs_eval_partials2" in lib.kodhip_last_error()
