"""CPU checks of tests/conv_reference.py: the bf16 round-to-nearest-even helper, the tie test and the single- / double-
rounding formulas on hand-computed values, and the float64 convolution reference against autograd."""
import torch
import torch.nn.functional as F

from conv_reference import (U16, U32, accumulate_bf16, bf16_rne, conv_abs, conv_ref, double_rounding, first_mismatch, gamma,
                            int_tensor, is_bf16, is_rne_tie, single_rounding)


def t(*v):
    return torch.tensor(v, dtype=torch.float64)


def test_bf16_rne_on_hand_computed_values():
    # bf16 keeps 8 significant bits: spacing 1 in [128, 256), 2 in [256, 512), 4 in [512, 1024), 2^-7 in [1, 2)
    x = t(0, 1, 255, 256, 257, 258, 259, 261, 263, 513, 514, 515, 518, -257, -259, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 0.5, 2.0 ** 100)
    want = t(0, 1, 255, 256, 256, 258, 260, 260, 264, 512, 512, 516, 520, -256, -260, 1, 1 + 2.0 ** -6, 0.5, 2.0 ** 100)
    assert torch.equal(bf16_rne(x), want)
    tie = t(0, 0, 0, 0, 1, 0, 1, 1, 1, 0, 1, 0, 1, 1, 1, 1, 1, 0, 0).bool()
    assert torch.equal(is_rne_tie(x), tie)
    assert torch.equal(is_bf16(x), bf16_rne(x) == x)
    assert U16 == 2.0 ** -8 and U32 == 2.0 ** -24
    assert gamma(1) == U32 / (1 - U32) and abs(gamma(576) / (576 * U32) - 1) < 1e-4


def test_bf16_rne_agrees_with_torch_conversion():
    g = torch.Generator().manual_seed(0)
    x = torch.cat([torch.randn(20000, generator=g) * 300, torch.randint(-70000, 70000, (20000,), generator=g).float(),
                   torch.randint(-4096, 4096, (20000,), generator=g).float() / 64])
    assert torch.equal(bf16_rne(x.double()), x.to(torch.bfloat16).double())
    # every error is within half a spacing, i.e. the unit roundoff 2^-8 relative to the value
    assert bool(((bf16_rne(x.double()) - x.double()).abs() <= U16 * x.double().abs()).all())


def test_single_and_double_rounding_formulas():
    S, prior = t(261, 259, 257, 300), t(1, 1, 257, 0.5)
    # 261 + 1 = 262 is a bf16 number; rounding 261 first gives 260, and 260 + 1 = 261 ties back to 260
    assert torch.equal(single_rounding(S, prior), t(262, 260, 512, 300))
    assert torch.equal(double_rounding(S, prior), t(260, 260, 512, 300))
    # the read-modify-write form rounds the partial, then the sum with the (bf16) content of dx
    assert torch.equal(accumulate_bf16(S, t(1, 1, 257, 2)), t(260, 260, 512, 302))
    assert torch.equal(accumulate_bf16(t(261), t(3)), t(264))               # 260 + 3 = 263 -> 264; single rounding: 264 too
    assert torch.equal(single_rounding(t(259), t(3)), t(262)) and torch.equal(accumulate_bf16(t(259), t(3)), t(264))


def test_conv_reference_matches_autograd_and_a_hand_example():
    x = torch.tensor([[[[1., 2.], [3., 4.]]]])
    w = torch.tensor([[[[2.]]], [[[-1.]]]])
    y, _, _ = conv_ref(x, w, 1, 0)
    assert torch.equal(y, torch.tensor([[[[2., 4.], [6., 8.]], [[-1., -2.], [-3., -4.]]]], dtype=torch.float64))
    g = torch.Generator().manual_seed(1)
    for (k, s, p) in ((1, 1, 0), (3, 1, 1), (3, 2, 1), (6, 2, 2)):
        x, w = int_tensor((2, 5, 9, 8), 16, g), int_tensor((4, 5, k, k), 8, g)
        dy = int_tensor(F.conv2d(x, w, None, s, p).shape, 8, g)
        y, dx, dw = conv_ref(x, w, s, p, dy)
        assert y.dtype == torch.float64 and torch.equal(y, F.conv2d(x, w, None, s, p).double())      # small integers: fp32 is exact too
        assert torch.equal(dx, torch.nn.grad.conv2d_input(x.shape, w.double(), dy.double(), s, p))
        assert torch.equal(dw, torch.nn.grad.conv2d_weight(x.double(), w.shape, dy.double(), s, p))
        ya, _, _ = conv_abs(x, w, s, p)
        assert bool((ya >= y.abs()).all())


def test_first_mismatch_names_position_and_tile():
    a = torch.zeros(2, 16, 16, 40)
    b = a.clone()
    assert first_mismatch(a, b) == "equal"
    b[1, 2, 3, 37] = 5.0
    msg = first_mismatch(a, b, 128, 32)
    assert "(image 1, row 2, column 3, channel 37)" in msg and "pixel 291 = tile 2 row 35, channel tile 1 column 5, lane 35" in msg
