"""The numpy restatement of the fused Adam / AdamW update (tests/adam_reference.py) against CPU torch.optim.Adam / AdamW
(foreach=False), and the Adam state-dict writer against the installed torch's own layout.  No GPU.

Pins (the states are re-synchronised to torch's before every step, so one step's arithmetic is compared at a time):
(b) exp_avg and exp_avg_sq equal torch's bit for bit;
(c) the parameters lie within one ulp of torch's everywhere and differ in at most 1e-4 of the element-steps.  The cap is a
    condition on the inputs, not a measurement.  What differs is torch's side: its CPU sqrt over a large tensor is off by one
    ulp in a share of the elements that depends on the host's math library (0.7 % measured on one host), the denominator
    inherits it, and the difference reaches the parameter with probability ~|update| / |parameter|.  Measured with learning
    rates ten times these: 0 to 1 of 360 891 element-steps on one host, 26 to 32 (up to 8.9e-5) on another - too close to
    the cap to rely on, so the inputs keep |update| / |parameter| near 1e-4 (see _inputs)."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import adam_reference as ar

N, STEPS = 40099, 9
SIZES = (1031, 30004, 9064)                       # bias | decay | norm groups: odd sizes, 40099 elements together
# per group, cycled over the steps.  ~1e-4 against parameters of magnitude ~1: see _inputs
LRS = ((2e-4, 1e-4, 5e-5), (1.7e-4, 1.1e-4, 4e-5), (1.3e-4, 9e-5, 3.3e-5))
BETAS, EPS = (0.937, 0.999), 1e-8


def _inputs(seed):
    rng = np.random.default_rng(seed)
    # parameter magnitudes in [0.25, 2) and learning rates ~1e-4: an update of ~lr then never cancels its parameter.  Where it does (|p| ~ lr), a one-ulp
    # difference in the update - torch's CPU sqrt over a large tensor is not correctly rounded on every build - shows as many
    # ulps of the small result, which says nothing about the order of operations pinned here.  Small and zero parameters are
    # covered bit for bit by pin (a), the kernel against this restatement (tests/test_hip_adam.py).
    ps = [(rng.choice([-1.0, 1.0], n) * rng.uniform(0.25, 2.0, n)).astype(np.float32) for n in SIZES]
    gs = [[(rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 2, n)).astype(np.float32) for n in SIZES] for _ in range(STEPS)]
    return ps, gs


@pytest.mark.parametrize("maximize", [False, True])
@pytest.mark.parametrize("wds", [(0.0, 0.0, 0.0), (0.0, 5e-4, 1e-2)])
@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_restatement_against_cpu_torch(decoupled, wds, maximize):
    assert sum(SIZES) == N
    ps, gs = _inputs(11)
    params = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in ps]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([dict(params=[p], lr=LRS[0][k], weight_decay=wds[k]) for k, p in enumerate(params)], betas=BETAS, eps=EPS,
              foreach=False, maximize=maximize)
    differ = worst = 0
    for step in range(1, STEPS + 1):
        before = []
        for k, p in enumerate(params):
            st = opt.state.get(p, {})
            before.append((p.detach().numpy().copy(),
                           st["exp_avg"].numpy().copy() if st else np.zeros(SIZES[k], np.float32),
                           st["exp_avg_sq"].numpy().copy() if st else np.zeros(SIZES[k], np.float32)))
            p.grad = torch.from_numpy(gs[step - 1][k].copy())
            opt.param_groups[k]["lr"] = LRS[step % 3][k]
        opt.step()
        for k, p in enumerate(params):
            c = ar.host_constants(LRS[step % 3][k], BETAS[0], BETAS[1], EPS, wds[k], step)
            p2, m2, v2 = ar.adam_ref(*before[k][:1], gs[step - 1][k], *before[k][1:], c, maximize=maximize, decoupled=decoupled)
            st = opt.state[p]
            assert float(st["step"]) == step
            assert np.array_equal(m2.view(np.int32), st["exp_avg"].numpy().view(np.int32)), (step, k)             # (b)
            assert np.array_equal(v2.view(np.int32), st["exp_avg_sq"].numpy().view(np.int32)), (step, k)          # (b)
            d = ar.ulp_distance(p2, p.detach().numpy())
            differ += int((d != 0).sum())
            worst = max(worst, int(d.max()))
    print(f"parameters: {differ} of {N * STEPS} element-steps differ from torch, worst {worst} ulp")
    assert worst <= 1                                                                                                   # (c)
    assert differ <= 1e-4 * N * STEPS                                                                                   # (c)


def test_fma32_is_a_single_rounding():
    """a case where fp32(fp64(a) * b + c) rounds twice, and random cancelling cases against exact rational arithmetic"""
    from fractions import Fraction
    # a * b = 2^-24 - 2^-70; with c = 1 + 2^-23 the exact sum lies just BELOW the fp32 tie 1 + 2^-23 + 2^-24 and rounds down to
    # c; fp64 rounds the sum onto the tie, and ties-to-even then goes up to 1 + 2^-22
    a = np.float32(2.0 ** -12 * (1 + 2.0 ** -23))
    b = np.float32(2.0 ** -12 * (1 - 2.0 ** -23))
    c = np.float32(1 + 2.0 ** -23)
    assert np.float32(np.float64(a) * np.float64(b) + np.float64(c)) == np.float32(1 + 2.0 ** -22)       # the bare shortcut is wrong
    assert ar.fma32(a, b, c) == c
    assert ar.fma32(-a, b, -c) == -c
    rng = np.random.default_rng(5)
    n = 3000
    x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(np.float32)
    y = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(np.float32)
    z = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(np.float32)
    z[: n // 2] = (-(x[: n // 2].astype(np.float64) * y[: n // 2]) * (1 + rng.uniform(-1e-6, 1e-6, n // 2))).astype(np.float32)
    got = ar.fma32(x, y, z)
    for i in range(n):
        exact = Fraction(float(x[i])) * Fraction(float(y[i])) + Fraction(float(z[i]))
        near = np.float32(float(exact))            # (Fraction -> double is correctly rounded; the fp32 answer is among its neighbours)
        cands = [np.nextafter(near, np.float32(-np.inf)), near, np.nextafter(near, np.float32(np.inf))]
        best = min(cands, key=lambda t: (abs(Fraction(float(t)) - exact), int(np.float32(t).view(np.int32)) & 1))
        assert got[i] == best, (i, x[i], y[i], z[i], got[i], best)


def _fake_net_state(steps_taken, frozen=()):
    """the writer over CPU 'arenas': three groups, five tensors"""
    from object_detection_cib_amd.lightning.checkpoint import adam_state_dict
    shapes = OrderedDict([("a.bias", (5,)), ("b.bias", (3,)), ("a.weight", (5, 4)), ("b.weight", (3, 5, 1, 1)), ("n.weight", (7,))])
    groups = (["a.bias", "b.bias"], ["a.weight", "b.weight"], ["n.weight"])
    layout, off = {}, 0
    for n, s in shapes.items():
        layout[n] = (off, int(np.prod(s)))
        off += (int(np.prod(s)) + 63) // 64 * 64
    g = torch.Generator().manual_seed(3)
    m, v = torch.randn(off, generator=g), torch.rand(off, generator=g)
    pgs = [dict(lr=1e-3 * (k + 1), betas=(0.9, 0.999), eps=1e-8, weight_decay=w, name=nm, initial_lr=1e-3)
           for k, (nm, w) in enumerate((("bias_params", 0.0), ("decay_params", 5e-4), ("norm_params", 0.0)))]
    return adam_state_dict(groups, pgs, shapes, layout, m, v, steps_taken, frozen), shapes, groups, layout, m, v


@pytest.mark.parametrize("cls", [torch.optim.Adam, torch.optim.AdamW])
def test_state_dict_keys_and_types_match_installed_torch(cls):
    sd, shapes, groups, layout, m, v = _fake_net_state(4)
    params = [torch.nn.Parameter(torch.zeros(shapes[n])) for names in groups for n in names]
    opt = torch.optim.Adam([dict(params=params[0:2]), dict(params=params[2:4]), dict(params=params[4:5])])
    for p in params:
        p.grad = torch.ones_like(p)
    opt.step()
    ref = opt.state_dict()
    assert set(sd) == set(ref)
    for got, want in zip(sd["param_groups"], ref["param_groups"]):
        assert set(got) == set(want) | {"name", "initial_lr"}
        assert got["params"] == want["params"]
        for k in want:
            number = lambda x: isinstance(x, (int, float)) and not isinstance(x, bool)      # (torch's own default weight_decay is the int 0)
            assert type(got[k]) is type(want[k]) or (number(got[k]) and number(want[k])), (k, got[k], want[k])
    assert set(sd["state"]) == set(ref["state"])
    for i, st in ref["state"].items():
        assert set(sd["state"][i]) == set(st)
        for k, t in st.items():
            assert sd["state"][i][k].dtype == t.dtype and sd["state"][i][k].shape == t.shape, (i, k)
    assert float(sd["state"][0]["step"]) == 4.0
    # the installed torch optimizer loads it, and the tensors arrive where they belong
    opt2 = cls([dict(params=params[0:2]), dict(params=params[2:4]), dict(params=params[4:5])], foreach=False)
    opt2.load_state_dict(sd)
    flat = [n for names in groups for n in names]
    for n, p in zip(flat, params):
        o, k = layout[n]
        assert torch.equal(opt2.state[p]["exp_avg"].reshape(-1), m[o:o + k])
        assert torch.equal(opt2.state[p]["exp_avg_sq"].reshape(-1), v[o:o + k])
        assert float(opt2.state[p]["step"]) == 4.0
    assert [g["lr"] for g in opt2.param_groups] == [1e-3, 2e-3, 3e-3]
    for p in params:
        p.grad = torch.ones_like(p)
    opt2.step()                                    # and steps on from it
    assert float(opt2.state[params[0]]["step"]) == 5.0


def test_state_dict_before_the_first_step_and_with_frozen_tensors():
    sd, *_ = _fake_net_state(0)
    assert sd["state"] == {} and [g["params"] for g in sd["param_groups"]] == [[0, 1], [2, 3], [4]]
    sd, *_ = _fake_net_state(2, frozen=("b.bias", "a.weight"))
    assert sorted(sd["state"]) == [0, 3, 4]        # frozen from the start: no state, as with torch


def test_host_block_matches_the_restatement_constants():
    from object_detection_cib_amd.engine.arenas import ADAM_HYPER_FLOATS, adam_hyper_values
    lr, wd = (1e-3, 2e-3, 3e-4), (0.0, 5e-4, 1e-2)
    for step in (1, 2, 7, 1000):
        vals = np.array(adam_hyper_values(lr, [BETAS] * 3, [EPS] * 3, wd, step, 0.25, True, True), dtype=np.float64).astype(np.float32)
        want = ar.hyper_block([ar.host_constants(lr[k], *BETAS, EPS, wd[k], step) for k in range(3)], 0.25, True, True, ADAM_HYPER_FLOATS)
        assert np.array_equal(vals.view(np.int32), want.view(np.int32)), step
    with pytest.raises(ValueError, match="step"):
        adam_hyper_values(lr, [BETAS] * 3, [EPS] * 3, wd, 0)
