"""tests/small_ops_reference.py against torch on the CPU: the reference the GPU tests (tests/test_hip_small_ops.py) hold
the layout, pack, pool and upsample kernels to is itself pinned to torch.Tensor.to(bfloat16), F.conv2d, F.max_pool2d,
F.interpolate and float64 autograd - from first principles, so that it cannot restate a kernel's own index arithmetic."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import small_ops_reference as S


def _torch_bf16_bits(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def _cl(t):
    """NCHW torch -> channels-last numpy"""
    return t.detach().permute(0, 2, 3, 1).contiguous().numpy()


# ---------------------------------------------------------------- bf16
def test_bf16_bits_equals_torch():
    rng = np.random.default_rng(0)
    half = S.halfway_values()
    lows = half.view(np.uint32) & 0xFFFF
    uppers = (half.view(np.uint32) >> 16) & 1
    for low in (0x7FFF, 0x8000, 0x8001):
        for odd in (0, 1):
            assert ((lows == low) & (uppers == odd)).any()          # exact halves and their neighbours, even and odd upper half
    rand = rng.integers(0, 2 ** 32, size=200000, dtype=np.uint64).astype(np.uint32)
    expo = (rand >> 23) & 0xFF
    rand = rand[(expo != 0) & (expo != 0xFF)].view(np.float32)        # finite normal values of every exponent
    vals = np.concatenate([S.special_values(), rand, (rng.standard_normal(50000) * 3).astype(np.float32)])
    vals = vals[~np.isnan(vals)]
    assert np.array_equal(S.bf16_bits(vals), _torch_bf16_bits(vals))
    assert S.bf16_bits(np.float32(np.finfo(np.float32).max)) == 0x7F80
    assert S.bf16_bits(np.float32(-0.0)) == 0x8000
    # ties to even: 1 + 2^-8 is halfway between 1 and 1 + 2^-7 and goes down, 1 + 3 * 2^-8 goes up
    assert S.bf16_bits(np.float32(1 + 2.0 ** -8)) == 0x3F80 and S.bf16_bits(np.float32(1 + 3 * 2.0 ** -8)) == 0x3F82
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0xFF80FFFF], dtype=np.uint32).view(np.float32)
    assert S.bits_is_nan(S.bf16_bits(nans)).all()                   # a NaN maps to some NaN, never to inf
    assert np.array_equal(S.bits_to_f32(S.bf16_bits(vals)), torch.from_numpy(vals).to(torch.bfloat16).float().numpy())


def test_nhwc4():
    rng = np.random.default_rng(1)
    for C in (1, 2, 3, 4):
        x = rng.standard_normal((2, C, 3, 5)).astype(np.float32)
        y = S.nhwc4(x)
        assert y.shape == (2, 3, 5, 4) and y.dtype == np.uint16
        assert np.array_equal(y[..., :C], _torch_bf16_bits(x.transpose(0, 2, 3, 1)))
        assert (y[..., C:] == 0).all()
    with pytest.raises(ValueError):
        S.nhwc4(np.zeros((1, 5, 2, 2), np.float32))


# ---------------------------------------------------------------- weight packs
def _up(n, a=32):
    return (n + a - 1) // a * a


def _materialise(master, gather):
    return np.where(gather >= 0, master[np.maximum(gather, 0)], 0.0)


@pytest.mark.parametrize("cin,k", [(3, 1), (3, 3), (8, 1), (8, 3), (48, 1), (48, 3)])
def test_pack_gather_plain_is_a_conv(cin, k):
    """forward pack row . equally packed im2col patch = F.conv2d; dgrad pack row . packed dY patch = autograd's dX (fp64).
    The weight shares its packs with a neighbour through n_off / Ntot, like a head does."""
    g = torch.Generator().manual_seed(cin * 10 + k)
    N, N2, H, W, p = 5, 3, 4, 5, k // 2
    w = torch.randn(N + N2, cin, k, k, generator=g, dtype=torch.float64)
    x = torch.randn(1, cin, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(1, N + N2, H, W, generator=g, dtype=torch.float64)
    cs, Ntot = _up(cin), N + N2
    ns = _up(Ntot)
    Kp, Kdp = k * k * cs, k * k * ns
    pre = 7                                                         # the masters do not start at 0
    master = np.concatenate([np.full(pre, 1e9), w.numpy().reshape(-1)])
    descs = [[pre, 0, 0, N, cin, k, k, Kp, Kdp, Ntot, 0, 0, 0],
             [pre + N * cin * k * k, N * Kp, 0, N2, cin, k, k, Kp, Kdp, Ntot, N, 0, 1]]
    fg, dg = S.pack_gather(descs, Ntot * Kp, cin * Kdp)
    assert (fg >= 0).sum() == (dg >= 0).sum() == w.numel()
    fp = _materialise(master, fg).reshape(Ntot, Kp)
    dp = _materialise(master, dg).reshape(cin, Kdp)
    y = F.conv2d(x, w, padding=p)
    y.backward(dy)
    xp = F.pad(x.detach(), (p, p, p, p)).numpy()[0]
    dyp = F.pad(dy, (p, p, p, p)).numpy()[0]
    for oy in range(H):
        for ox in range(W):
            patch = np.zeros(Kp)
            gpatch = np.zeros(Kdp)
            for kh in range(k):
                for kw in range(k):
                    t = kh * k + kw
                    patch[t * cs:t * cs + cin] = xp[:, oy + kh, ox + kw]
                    # dX[i] = sum over taps of w[tap] dY[i + p - tap]
                    gpatch[t * ns:t * ns + Ntot] = dyp[:, oy + 2 * p - kh, ox + 2 * p - kw]
            np.testing.assert_allclose(fp @ patch, y.detach().numpy()[0, :, oy, ox], rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(dp @ gpatch, x.grad.numpy()[0, :, oy, ox], rtol=1e-12, atol=1e-12)


def test_pack_gather_stem_is_the_6x6_conv():
    """stem rows against F.conv2d(x, w, stride 2, padding 2): the patch of an output pixel is 6 image rows of 4 pixel
    pairs x (2 pixels x 4 channels), starting at pixel 2 ox - 2 (the layout kodhip_nchw_to_nhwc4 writes, read in pairs)"""
    g = torch.Generator().manual_seed(3)
    N, H, W = 4, 8, 12
    w = torch.randn(N, 3, 6, 6, generator=g, dtype=torch.float64)
    x = torch.randn(1, 3, H, W, generator=g, dtype=torch.float64)
    fg, dg = S.pack_gather([[0, 0, -1, N, 3, 6, 6, 192, 0, 0, 0, 1, 0]], N * 192, 8)
    assert (dg < 0).all() and (fg >= 0).sum() == w.numel()
    fp = _materialise(w.numpy().reshape(-1), fg).reshape(N, 192)
    y = F.conv2d(x, w, stride=2, padding=2).numpy()[0]
    x4 = np.zeros((H + 8, W + 8, 4))                               # channels-last, C padded to 4, zero border
    x4[4:4 + H, 4:4 + W, :3] = x.numpy()[0].transpose(1, 2, 0)
    for oy in range(H // 2):
        for ox in range(W // 2):
            rows = [x4[4 + 2 * oy - 2 + kh, 4 + 2 * ox - 2:4 + 2 * ox - 2 + 8].reshape(-1) for kh in range(6)]
            np.testing.assert_allclose(fp @ np.concatenate(rows), y[:, oy, ox], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("N", [8, 40])
@pytest.mark.parametrize("form", [S.S2_CLASSES, S.S2_FOLDED])
def test_pack_gather_stride2_forms_are_the_transposed_conv(form, N):
    """dX of F.conv2d(x, w, stride=2, padding=1) assembled from the packs per output-pixel parity equals autograd (fp64).
    Input pixel (iy, ix) of parity (py, px) sits in the 2 x 2 block (iy >> 1, ix >> 1); tap kh along an axis brings
    dY[(i + 1 - kh) / 2]."""
    g = torch.Generator().manual_seed(N + form)
    Cin, H, W = 8, 6, 6
    w = torch.randn(N, Cin, 3, 3, generator=g, dtype=torch.float64)
    x = torch.randn(1, Cin, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, stride=2, padding=1)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    ns = _up(N)
    d_size = Cin * (16 if form == S.S2_FOLDED else 9) * ns
    Kp = 9 * _up(Cin)
    fg, dg = S.pack_gather([[0, 0, 0, N, Cin, 3, 3, Kp, 9 * ns, N, 0, form, 0]], N * Kp, d_size)
    assert (fg >= 0).sum() == w.numel() and (dg >= 0).sum() == w.numel()
    dp = _materialise(w.numpy().reshape(-1), dg)
    Ho, Wo = y.shape[2:]
    dyz = np.zeros((N, Ho + 1, Wo + 1))                             # (one zero row / column: the neighbour past the edge)
    dyz[:, :Ho, :Wo] = dy.numpy()[0]
    want = x.grad.numpy()[0]
    got = np.zeros_like(want)
    base = 0
    for py in (0, 1):
        for px in (0, 1):
            cls = 2 * py + px
            if form == S.S2_CLASSES:
                taps = S.s2_class_taps(py, px)
                assert len(taps) == (1, 2, 2, 4)[cls]
                pack = dp[base:base + Cin * len(taps) * ns].reshape(Cin, len(taps) * ns)
                base += pack.size
                for iy in range(py, H, 2):
                    for ix in range(px, W, 2):
                        vec = np.zeros(len(taps) * ns)
                        for t, (kh, kw) in enumerate(taps):
                            vec[t * ns:t * ns + N] = dyz[:, (iy + 1 - kh) // 2, (ix + 1 - kw) // 2]
                        got[:, iy, ix] = pack @ vec
            else:
                pack = dp.reshape(4 * Cin, 4 * ns)[cls * Cin:(cls + 1) * Cin]
                for iy in range(py, H, 2):
                    for ix in range(px, W, 2):
                        vec = np.zeros(4 * ns)                      # the 2 x 2 dY neighbourhood of the block, row-major
                        for a in (0, 1):
                            for b in (0, 1):
                                vec[(2 * a + b) * ns:(2 * a + b) * ns + N] = dyz[:, (iy >> 1) + a, (ix >> 1) + b]
                        got[:, iy, ix] = pack @ vec
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)


def test_pack_gather_refuses_overlap_and_overflow():
    ok = [0, 0, 0, 4, 8, 1, 1, 32, 32, 4, 0, 0, 0]
    S.pack_gather([ok], 4 * 32, 8 * 32)
    with pytest.raises(ValueError):
        S.pack_gather([ok, [32, 0, -1, 4, 8, 1, 1, 32, 32, 4, 0, 0, 1]], 8 * 32, 8 * 32)       # same forward rows
    with pytest.raises(ValueError):
        S.pack_gather([ok, [32, 4 * 32, 0, 4, 8, 1, 1, 32, 32, 4, 0, 0, 1]], 8 * 32, 8 * 32)   # same dgrad columns
    with pytest.raises(ValueError):
        S.pack_gather([ok], 3 * 32 + 7, 8 * 32)                                               # past the arena's end


# ---------------------------------------------------------------- pools
@pytest.mark.parametrize("K", S.POOL_WINDOWS)
def test_maxpool_vs_torch(K):
    """values and argmax against F.max_pool2d(return_indices=True), gradient against float64 autograd, on the GPU test's
    own inputs (tie-heavy, +-inf) and on the same with a NaN per image; the backward sum on the dyadic gradients is the
    same in fp32 and fp64 (every fp32 sum is exact, whatever its order) and at least 1 % of the totals are no bf16 values"""
    for si, (B, H, W, C) in enumerate(S.POOL_SHAPES):
        x0, dy, base = S.pool_case(K, si)
        assert not np.isnan(x0).any() and np.array_equal(S.bits_to_f32(S.bf16_bits(x0)), x0)
        for with_nan in (False, True):
            x = x0.copy()
            if with_nan:
                if H * W < 9:
                    continue
                x[:, H // 2, W // 2, 0] = np.nan
            xt = torch.from_numpy(x).double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
            yt, it = F.max_pool2d(xt, K, 1, K // 2, return_indices=True)
            val, idx = S.maxpool_fwd(x, K)
            assert np.array_equal(val, _cl(yt).astype(np.float32), equal_nan=True)
            # idx byte -> flat input index, as torch reports it
            oy, ox = np.indices((H, W))
            flat = ((oy[None, :, :, None] + (idx >> 4).astype(np.int64) - K // 2) * W
                    + ox[None, :, :, None] + (idx & 15).astype(np.int64) - K // 2)
            assert np.array_equal(flat, _cl(it))
            yt.backward(torch.from_numpy(dy).double().permute(0, 3, 1, 2))
            s32 = S.maxpool_bwd_sum(dy, idx, K, base, np.float32)
            s64 = S.maxpool_bwd_sum(dy, idx, K, base, np.float64)
            assert np.array_equal(s32.astype(np.float64), s64)
            assert np.array_equal(s64, base.astype(np.float64) + _cl(xt.grad))
            assert np.array_equal(S.maxpool_bwd(dy, idx, K, base), S.bf16_bits(s64.astype(np.float32)))
            if not with_nan:
                assert S.rounded_share(s32) >= 0.01, (K, si)


def test_dyadic_inputs_are_bf16_values():
    d = S.dyadic((4096,), np.random.default_rng(0))
    assert np.array_equal(S.bits_to_f32(S.bf16_bits(d)), d) and d.min() >= -4 and d.max() <= 4
    assert np.array_equal(d * 64, np.round(d * 64))


# ---------------------------------------------------------------- upsample
def test_upsample_vs_torch():
    rng = np.random.default_rng(5)
    for si, (B, H, W, C) in enumerate(S.UPSAMPLE_SHAPES):
        x = rng.standard_normal((B, H, W, C))
        xt = torch.from_numpy(x).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        yt = F.interpolate(xt, scale_factor=2, mode="nearest")
        assert np.array_equal(S.upsample_fwd(x), _cl(yt))
        bits = rng.integers(0, 2 ** 16, size=(B, H, W, C)).astype(np.uint16)       # any bit pattern is copied
        up = S.upsample_fwd(bits)
        assert up.dtype == np.uint16 and np.array_equal(up[:, 1::2, 0::2], bits) and np.array_equal(up[:, 0::2, 1::2], bits)
        dy, old, shadow = S.upsample_case(si)
        yt.backward(torch.from_numpy(dy).double().permute(0, 3, 1, 2))
        grad = _cl(xt.grad)
        for acc, sh, start in ((0, None, 0.0), (0, shadow, 0.0), (1, None, old), (1, shadow, shadow)):
            s32 = S.upsample_bwd_sum(dy, acc, old, sh, np.float32)
            s64 = S.upsample_bwd_sum(dy, acc, old, sh, np.float64)
            assert np.array_equal(s32.astype(np.float64), s64)
            assert np.array_equal(s64, grad + start)
            assert np.array_equal(S.upsample_bwd(dy, acc, old, sh), S.bf16_bits(s64.astype(np.float32)))
            assert S.rounded_share(s32) >= 0.01, (si, acc)


# ---------------------------------------------------------------- SPPF
def test_sppf_grad_forms():
    """an int is the cascade of three pools, a sequence reads x with every pool; the two route tied gradients differently
    although the pooled VALUES of (k, 2k - 1, 3k - 2) equal the cascade's.  On the GPU test's inputs every sum is a small
    integer: exact in bf16 whatever the order of the launches."""
    for ks in S.SPPF_FORMS:
        x, dcat = S.sppf_case(ks)
        C = x.shape[-1]
        cat, g = S.sppf_grad(x, ks, dcat)
        assert np.array_equal(cat[..., :C], x) and np.abs(g).max() <= 25
        if isinstance(ks, int):
            cat_c, g_c = S.sppf_cascade_grad(x, ks, 3, dcat)
            assert np.array_equal(cat, cat_c) and np.array_equal(g, g_c)
            continue
        # the sequence form, pool by pool through this module's own forward / backward
        want = dcat[..., :C].astype(np.float64)
        for q, kk in enumerate(ks):
            val, idx = S.maxpool_fwd(x, kk)
            assert np.array_equal(val, cat[..., C * (q + 1):C * (q + 2)].astype(np.float32))
            want = S.maxpool_bwd_sum(dcat[..., C * (q + 1):C * (q + 2)], idx, kk, want, np.float64)
        assert np.array_equal(want, g)
        if len(ks) == 3 and all(k == (j + 1) * (ks[0] - 1) + 1 for j, k in enumerate(ks)):
            cat_c, g_c = S.sppf_cascade_grad(x, ks[0], 3, dcat)
            assert np.array_equal(cat_c, cat)                         # same values ...
            assert np.mean(g_c != g) >= 0.01                          # ... other routing
