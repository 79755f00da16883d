"""The small kernels at both ends of the training step (csrc/misc_ops.hip) against tests/small_ops_reference.py, BIT FOR BIT:
image re-layout, weight packing (descriptor tables built here, and the engine's own), pool backward with real bf16
rounding and the fp32 shadow, every form of the x2 upsample backward, the SPPF pool plan against the reference module's
gradient routing, fill and host pull, and the argument checks.

Every device buffer sits between two sentinel-filled margins, every channel slice between sentinel guard channels; both
must come back untouched.  Comparisons are np.array_equal on the bf16 bit patterns (where a NaN is expected, any NaN
will do).  The backward inputs are dyadic (multiples of 2^-6 in [-4, 4]), so every fp32 sum is exact in any order and
only the final rounding to bf16 remains - which at least 1 % of the elements of every case need
(tests/test_small_ops_reference.py asserts both on the same inputs)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from object_detection_cib_amd import _lib  # noqa: E402
import small_ops_reference as S  # noqa: E402
from hip_helpers import stream  # noqa: E402

MARGIN = 64                                    # elements on either side of a buffer (a multiple of 16 bytes for every type)
SENTINEL = {torch.int16: 0x5A5A, torch.uint8: 0x5A, torch.int32: 0x5A5A5A5A}
NP_OF = {torch.int16: np.int16, torch.uint8: np.uint8, torch.int32: np.int32}
NAN16 = 0xFFFF                                 # a bf16 NaN: what a kernel must not read
NAN32 = 0x7FC00000


class Buf:
    """A device buffer of integer words (bf16 bits: int16, fp32 bits: int32, bytes: uint8) inside one fresh allocation
    whose margins hold a sentinel.  skew: extra elements in front, to misalign the data."""

    def __init__(self, shape, dtype, init=None, skew=0):
        self.shape, self.dtype = tuple(shape), dtype
        self.n = int(np.prod(shape))
        self.lo = MARGIN + skew
        self.full = torch.full((self.lo + self.n + MARGIN,), SENTINEL[dtype], dtype=dtype, device="cuda")
        self.t = self.full[self.lo:self.lo + self.n].view(self.shape)
        if init is not None:
            self.put(init)

    def put(self, a):
        a = np.asarray(a)
        assert a.dtype.itemsize == self.t.element_size() and a.shape == self.shape, (a.dtype, a.shape, self.shape)
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(a).view(NP_OF[self.dtype])))
        return self

    @property
    def ptr(self):
        return self.t.data_ptr()

    def get(self, as_dtype):
        torch.cuda.synchronize()
        return self.t.cpu().numpy().view(as_dtype)

    def margins_untouched(self):
        torch.cuda.synchronize()
        s = SENTINEL[self.dtype]
        return bool((self.full[:self.lo] == s).all()) and bool((self.full[self.lo + self.n:] == s).all())


def bf16_buf(shape, bits=None):
    return Buf(shape, torch.int16, None if bits is None else np.asarray(bits, dtype=np.uint16))


def f32_buf(shape, vals=None, skew=0):
    return Buf(shape, torch.int32, None if vals is None else np.asarray(vals, dtype=np.float32), skew)


def fill_bits(buf, word):
    buf.t.fill_(int(np.array(word, dtype=np.uint32 if buf.dtype == torch.int32 else np.uint16)
                    .view(np.int32 if buf.dtype == torch.int32 else np.int16)))
    return buf


def assert_bits(got, want, what=""):
    """bit patterns equal; where a NaN is expected any NaN will do"""
    got, want = np.asarray(got, dtype=np.uint16), np.asarray(want, dtype=np.uint16)
    assert got.shape == want.shape, what
    nan = S.bits_is_nan(want)
    assert S.bits_is_nan(got)[nan].all(), f"{what}: a NaN was expected"
    bad = (got != want) & ~nan
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {np.argwhere(bad)[0].tolist()}"


def sliced(C, bits, guard=8, lead=8):
    """bf16 bits [B, H, W, C] as the channel slice [lead, lead + C) of a wider sentinel-filled buffer (ld = lead + C + guard)"""
    B, H, W, _ = bits.shape
    wide = bf16_buf((B, H, W, lead + C + guard))
    wide.t[..., lead:lead + C].copy_(torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)))
    return wide, lead + C + guard, lead


def guards_untouched(wide, slices):
    """every channel of `wide` outside the (coff, C) slices still holds the sentinel"""
    torch.cuda.synchronize()
    keep = torch.ones(wide.shape[-1], dtype=torch.bool)
    for coff, C in slices:
        keep[coff:coff + C] = False
    return bool((wide.t[..., keep.cuda()] == SENTINEL[wide.dtype]).all()) and wide.margins_untouched()


# ---------------------------------------------------------------- a. image re-layout
NHWC4_SHAPES = [(2, 2, 2, False),           # one pixel quad per image
                (1, 3, 5, False),           # HW % 4 != 0: the scalar kernel
                (3, 16, 20, False),
                (5, 16, 16, False),         # 320 quads: the second block partly filled
                (2, 1, 4, False),
                (3, 16, 20, True)]          # x starts 4 bytes into its allocation: the scalar kernel with HW % 4 == 0


@pytest.mark.parametrize("C", [1, 2, 3, 4])
@pytest.mark.parametrize("B,H,W,misaligned", NHWC4_SHAPES)
def test_nchw_to_nhwc4(B, H, W, misaligned, C):
    """kodhip_nchw_to_nhwc4, both kernels: values at exact bf16 halfway points (even and odd upper half) and their
    neighbours, +-0, +-inf, the largest finite fp32 (-> inf), a NaN and every k / 255; the padding channels are zero and
    nothing is written past the end."""
    lib = _lib.lib()
    rng = np.random.default_rng(1000 * C + 100 * B + H * W + int(misaligned))
    pool = rng.permutation(S.special_values())
    n = B * C * H * W
    x = np.resize(pool, n).reshape(B, C, H, W)
    xd = f32_buf((B, C, H, W), x, skew=1 if misaligned else 0)
    assert xd.ptr % 16 == (4 if misaligned else 0)
    y = bf16_buf((B, H, W, 4))                                     # (its own fresh allocation, sentinel-filled)
    assert y.ptr % 16 == 0
    _lib.check(lib.kodhip_nchw_to_nhwc4(xd.ptr, y.ptr, B, C, H, W, stream()), "nchw_to_nhwc4")
    want = S.nhwc4(x)
    got = y.get(np.uint16)
    assert_bits(got, want, "nhwc4")
    assert (got[..., C:] == 0).all()
    assert y.margins_untouched() and xd.margins_untouched()
    assert np.array_equal(xd.get(np.uint32), x.view(np.uint32))


# ---------------------------------------------------------------- b. weight packs by tables built here
def _up(n, a=32):
    return (n + a - 1) // a * a


def _pack_table():
    """one launch's descriptors: (rows, master size, forward pack size, dgrad pack size, blocks)"""
    rows = []
    st = dict(w=0, f=0, d=0, blk=0)

    def row(N, Cin, KH, KW, f_off, d_off, Kp, Kdp, Ntot, n_off, form):
        rows.append([st["w"], f_off, d_off, N, Cin, KH, KW, Kp, Kdp, Ntot, n_off, form, st["blk"]])
        st["blk"] += (N * Cin * KH * KW + 255) // 256
        st["w"] += N * Cin * KH * KW

    def conv(N, Cin, k, form=S.PLAIN, gap=0):
        Kp, Kdp = k * k * _up(Cin), k * k * _up(N)
        row(N, Cin, k, k, st["f"], st["d"], Kp, Kdp, N, 0, form)
        st["f"] += N * Kp
        st["d"] += Cin * {S.PLAIN: Kdp, S.S2_CLASSES: 9 * _up(N), S.S2_FOLDED: 16 * _up(N)}[form]
        st["w"] += gap                                            # (masters need not be packed tightly)

    conv(16, 16, 1)                          # exactly 256 elements: one full block
    conv(1, 1, 1, gap=5)                     # one element
    conv(8, 48, 3)                           # Cin = 48: taps padded to 64 channels
    row(16, 3, 6, 6, st["f"], -1, 192, 0, 0, 0, S.STEM)
    st["f"] += 16 * 192
    A, nc, cin = 3, 3, 40                    # a head: three weights in one forward pack and one dgrad pack
    Ntot = (A * (5 + nc) + 7) // 8 * 8
    Kp, Kdp = _up(cin), _up(Ntot)
    n_off = 0
    for n in (4 * A, A, nc * A):
        row(n, cin, 1, 1, st["f"] + n_off * Kp, st["d"], Kp, Kdp, Ntot, n_off, S.PLAIN)
        n_off += n
    st["f"] += Ntot * Kp
    st["d"] += cin * Kdp
    st["w"] += 3
    conv(16, 8, 3, S.S2_CLASSES)
    conv(40, 8, 3, S.S2_FOLDED, gap=1)       # N = 40: columns padded to 64
    conv(10, 30, 1)                          # 300 elements: the last block partly filled
    return np.array(rows, dtype=np.int64), st["w"], st["f"], st["d"], st["blk"]


@pytest.mark.parametrize("prefill", ["zero", "sentinel"])
def test_pack_weights_descriptor_table(prefill):
    """kodhip_pack_weights over a table holding every form and the block edges (a 256-element layer, a 1-element layer,
    a partly filled last block): into zeroed arenas the packs are bf16(master)[gather] with zero padding; into
    sentinel-filled arenas exactly the gathered positions change."""
    lib = _lib.lib()
    assert lib.kodhip_pack_desc_bytes() == 13 * 8
    rows, n_master, f_size, d_size, blocks = _pack_table()
    fg, dg = S.pack_gather(rows, f_size, d_size)                  # (raises if two descriptors overlap)
    rng = np.random.default_rng(7)
    pool = np.concatenate([S.halfway_values(), rng.standard_normal(1000).astype(np.float32)])
    master = pool[rng.integers(0, pool.size, size=n_master)].astype(np.float32)
    used = np.zeros(n_master, dtype=bool)
    used[fg[fg >= 0]] = True
    master[~used] = np.float32(1e9)                               # the gaps between masters: never read into a pack
    assert used.sum() == (fg >= 0).sum() == sum(int(r[3] * r[4] * r[5] * r[6]) for r in rows)
    md = f32_buf((n_master,), master)
    desc = torch.from_numpy(rows).cuda()
    fpack, dpack = bf16_buf((f_size,)), bf16_buf((d_size,))
    if prefill == "zero":
        fpack.t.zero_(); dpack.t.zero_()
        rest = 0
    else:
        rest = SENTINEL[torch.int16]
    _lib.check(lib.kodhip_pack_weights(md.ptr, fpack.ptr, dpack.ptr, desc.data_ptr(), rows.shape[0], blocks, stream()), "pack")
    bits = S.bf16_bits(master)
    for name, buf, g in (("forward pack", fpack, fg), ("dgrad pack", dpack, dg)):
        want = np.where(g >= 0, bits[np.maximum(g, 0)], rest).astype(np.uint16)
        assert (g < 0).sum() > 0
        assert_bits(buf.get(np.uint16), want, f"{name} ({prefill})")
        assert buf.margins_untouched()
    assert md.margins_untouched() and np.array_equal(md.get(np.float32).view(np.uint32), master.view(np.uint32))


# ---------------------------------------------------------------- c. weight packs by the engine's own table
def test_pack_weights_engine_table():
    """Engine.pack_weights() over the engine's descriptor table (engine/arenas.py): every conv unit, the three head
    weights per level, the stem form, both stride-2 forms - packs equal the reference gather of pack_descs over p_arena,
    padding stays zero over two steps, no element is claimed twice and pack_blocks is the table's block count."""
    from object_detection_cib_amd.nn.networks.yolov5 import Yolov5Network
    net = Yolov5Network(3, 3, widen_factor=0.25, deepen_factor=0.33).cuda()
    eng = net.engine()
    rows = eng.pack_descs.cpu().numpy()
    assert rows.shape[1] == 13
    assert {0, 1, 2, 3} <= set(int(v) for v in rows[:, 11]), "the table must hold every pack form"
    counts = rows[:, 3] * rows[:, 4] * rows[:, 5] * rows[:, 6]
    nblk = (counts + 255) // 256
    assert eng.pack_blocks == int(nblk.sum())
    assert np.array_equal(rows[:, 12], np.concatenate([[0], np.cumsum(nblk)[:-1]]))
    assert rows.shape[0] == len(eng.exec_units) + 3 * len(eng.g.heads)
    fg, dg = S.pack_gather(rows, eng.fpack.numel(), eng.dpack.numel())        # (raises on a double claim / overflow)
    assert (fg >= 0).sum() == int(counts.sum())
    assert (dg >= 0).sum() == int(counts[rows[:, 2] >= 0].sum())
    assert (fg < 0).any() and (dg < 0).any()
    g = torch.Generator().manual_seed(11)
    for step in range(2):                      # the second time as a later optimizer step would: other masters, same packs
        vals = torch.randn(eng.p_arena.numel(), generator=g) * (0.5 + step)
        eng.p_arena.copy_(vals)
        eng.pack_weights()
        torch.cuda.synchronize()
        m = vals.numpy()
        for name, pack, gat in (("fpack", eng.fpack, fg), ("dpack", eng.dpack, dg)):
            got = pack.view(torch.int16).cpu().numpy().view(np.uint16)
            assert_bits(got, S.gather_bits(m, gat), f"{name} step {step}")
            assert (got[gat < 0] == 0).all()


# ---------------------------------------------------------------- d. pool backward with rounding and the shadow
def _pool(lib, fwd, *a):
    _lib.check((lib.kodhip_maxpool_fwd if fwd else lib.kodhip_maxpool_bwd)(*a), "maxpool")


@pytest.mark.parametrize("si", range(len(S.POOL_SHAPES)))
@pytest.mark.parametrize("K", S.POOL_WINDOWS)
def test_maxpool_bwd_rounding_shadow_and_slices(K, si):
    """kodhip_maxpool_fwd's idx and kodhip_maxpool_bwd for every window (K = 5: the tuned kernels) on tie-heavy inputs
    with +-inf: (i) base in the bf16 dx; (ii) base in the fp32 shadow, dx full of NaN (not read); (iii) dy and dx as two
    channel slices of one buffer between guard channels; (iv) the same with a shadow in the slice's own indexing."""
    lib = _lib.lib()
    B, H, W, C = S.POOL_SHAPES[si]
    x, dy, base = S.pool_case(K, si)
    val, idx_ref = S.maxpool_fwd(x, K)
    total = S.maxpool_bwd_sum(dy, idx_ref, K, base)
    assert S.rounded_share(total) >= 0.01                          # the final rounding really happens
    want = S.bf16_bits(total)
    xb, yb = bf16_buf(x.shape, S.bf16_bits(x)), bf16_buf(x.shape)
    idx = Buf(x.shape, torch.uint8)
    _pool(lib, True, xb.ptr, C, 0, yb.ptr, C, 0, idx.ptr, B, H, W, C, K, stream())
    assert_bits(yb.get(np.uint16), S.bf16_bits(val), "pool values")
    assert np.array_equal(idx.get(np.uint8), idx_ref)
    assert xb.margins_untouched() and yb.margins_untouched() and idx.margins_untouched()
    gb = bf16_buf(x.shape, S.bf16_bits(dy))
    # (i) the old bf16 dx is the base
    dx = bf16_buf(x.shape, S.bf16_bits(base))
    _pool(lib, False, gb.ptr, C, 0, idx.ptr, dx.ptr, C, 0, B, H, W, C, K, None, stream())
    assert_bits(dx.get(np.uint16), want, "(i) bf16 base")
    assert dx.margins_untouched()
    # (ii) the fp32 shadow is the base; dx is only written
    dx = fill_bits(bf16_buf(x.shape), NAN16)
    shadow = f32_buf(x.shape, base)
    _pool(lib, False, gb.ptr, C, 0, idx.ptr, dx.ptr, C, 0, B, H, W, C, K, shadow.ptr, stream())
    assert_bits(dx.get(np.uint16), want, "(ii) shadow")
    assert dx.margins_untouched() and shadow.margins_untouched()
    assert np.array_equal(shadow.get(np.float32), base)
    # (iii) / (iv) slices of one buffer: guard | dx | guard | dy | guard
    ld, xo, yo = 2 * C + 24, 8, 16 + C
    for form, with_shadow in (("(iii) slices", False), ("(iv) slices + shadow", True)):
        wide = bf16_buf((B, H, W, ld))
        wide.t[..., yo:yo + C].copy_(gb.t)
        sh = None
        if with_shadow:
            wide.t[..., xo:xo + C].fill_(-1)                       # 0xffff: NaN
            sh = fill_bits(f32_buf((B, H, W, ld)), NAN32)
            sh.t[..., xo:xo + C].copy_(torch.from_numpy(base.view(np.int32)))
        else:
            wide.t[..., xo:xo + C].copy_(torch.from_numpy(S.bf16_bits(base).view(np.int16)))
        _pool(lib, False, wide.ptr, ld, yo, idx.ptr, wide.ptr, ld, xo, B, H, W, C, K, None if sh is None else sh.ptr, stream())
        got = wide.get(np.uint16)
        assert_bits(got[..., xo:xo + C], want, form)
        assert np.array_equal(got[..., yo:yo + C], S.bf16_bits(dy))
        assert guards_untouched(wide, [(xo, C), (yo, C)])
        if sh is not None:
            assert sh.margins_untouched()
    assert gb.margins_untouched() and idx.margins_untouched() and np.array_equal(idx.get(np.uint8), idx_ref)


# ---------------------------------------------------------------- e. upsample
@pytest.mark.parametrize("si", range(len(S.UPSAMPLE_SHAPES)))
def test_upsample_fwd_copies_bits_between_slices(si):
    lib = _lib.lib()
    B, H, W, C = S.UPSAMPLE_SHAPES[si]
    rng = np.random.default_rng(70 + si)
    bits = rng.integers(0, 2 ** 16, size=(B, H, W, C)).astype(np.uint16)      # NaN payloads, -0, subnormals: all copied
    bits.reshape(-1)[:4] = (0x8000, 0x7FC1, 0xFFFF, 0x0001)
    src, lds, so = sliced(C, bits, guard=8, lead=8)
    dst, ldd, do = sliced(C, np.full((B, 2 * H, 2 * W, C), SENTINEL[torch.int16], np.uint16), guard=8, lead=16)
    _lib.check(lib.kodhip_upsample2x_fwd(src.ptr, lds, so, dst.ptr, ldd, do, B, H, W, C, stream()), "upsample fwd")
    assert np.array_equal(dst.get(np.uint16)[..., do:do + C], S.upsample_fwd(bits))
    assert guards_untouched(dst, [(do, C)]) and guards_untouched(src, [(so, C)])
    assert np.array_equal(src.get(np.uint16)[..., so:so + C], bits)


@pytest.mark.parametrize("accumulate,with_shadow", [(0, False), (0, True), (1, False), (1, True)])
@pytest.mark.parametrize("si", range(len(S.UPSAMPLE_SHAPES)))
def test_upsample_bwd_every_form(si, accumulate, with_shadow):
    """kodhip_upsample2x_bwd: the four forms of (accumulate, fp32 shadow).  What a form does not read holds NaN: dx
    without accumulate, dx when the shadow carries the partial sum, the shadow without accumulate."""
    lib = _lib.lib()
    B, H, W, C = S.UPSAMPLE_SHAPES[si]
    dy, old, shadow = S.upsample_case(si)
    total = S.upsample_bwd_sum(dy, accumulate, old, shadow if with_shadow else None)
    assert S.rounded_share(total) >= 0.01
    g, ldy, yo = sliced(C, S.bf16_bits(dy), guard=16, lead=8)
    reads_dx = accumulate and not with_shadow
    dx, ldx, xo = sliced(C, S.bf16_bits(old) if reads_dx else np.full(old.shape, NAN16, np.uint16), guard=8, lead=16)
    sh = None
    if with_shadow:
        sh = fill_bits(f32_buf((B, H, W, ldx)), NAN32)
        if accumulate:
            sh.t[..., xo:xo + C].copy_(torch.from_numpy(shadow.view(np.int32)))
    _lib.check(lib.kodhip_upsample2x_bwd(g.ptr, ldy, yo, dx.ptr, ldx, xo, accumulate, B, H, W, C,
                                         None if sh is None else sh.ptr, stream()), "upsample bwd")
    assert_bits(dx.get(np.uint16)[..., xo:xo + C], S.bf16_bits(total), f"upsample bwd acc={accumulate} shadow={with_shadow}")
    assert guards_untouched(dx, [(xo, C)]) and guards_untouched(g, [(yo, C)])
    assert np.array_equal(g.get(np.uint16)[..., yo:yo + C], S.bf16_bits(dy))
    if sh is not None:
        assert sh.margins_untouched()


# ---------------------------------------------------------------- f. the pool plan against the reference module
def run_pool_plan(plan, x, dcat):
    """the engine's pool launches for `plan` on a concat buffer [B, H, W, (n + 1) C]: forward in order, backward last to
    first, each pool adding its routed gradient into the gradient slice of its source.  Returns (concat bits, bits of
    the gradient of slice 0)."""
    lib = _lib.lib()
    B, H, W, C = x.shape
    ld = (len(plan) + 1) * C
    cat = bf16_buf((B, H, W, ld))
    cat.t[..., :C].copy_(torch.from_numpy(S.bf16_bits(x).view(np.int16)))
    idx = [Buf(x.shape, torch.uint8) for _ in plan]
    for q, (sq, k) in enumerate(plan):
        _pool(lib, True, cat.ptr, ld, sq * C, cat.ptr, ld, (q + 1) * C, idx[q].ptr, B, H, W, C, k, stream())
    gcat = bf16_buf((B, H, W, ld), S.bf16_bits(dcat))
    for q in reversed(range(len(plan))):
        sq, k = plan[q]
        _pool(lib, False, gcat.ptr, ld, (q + 1) * C, idx[q].ptr, gcat.ptr, ld, sq * C, B, H, W, C, k, None, stream())
    out = cat.get(np.uint16), gcat.get(np.uint16)[..., :C]
    assert cat.margins_untouched() and gcat.margins_untouched() and all(i.margins_untouched() for i in idx)
    return out


def _is_arithmetic_cascade(ks):
    return not isinstance(ks, int) and len(ks) > 1 and ks[0] > 1 and all(k == (j + 1) * (ks[0] - 1) + 1 for j, k in enumerate(ks))


@pytest.mark.parametrize("ks", S.SPPF_FORMS, ids=lambda ks: "k" + "_".join(str(k) for k in (ks if isinstance(ks, tuple) else (ks,))))
def test_sppf_pool_plan_routes_like_the_reference_module(ks):
    """sppf_pool_plan(kernel_sizes) run with the library's pools against the reference module's pooling stage by fp64
    autograd (an int: three cascaded pools; a sequence: every pool reads x): concat values and input gradient, bit for
    bit.  Gradients are -1 / 0 / 1 and every sum stays below 25, exact in bf16 at every step.  A sequence (k, 2k - 1,
    3k - 2) has the cascade's VALUES but not its gradient routing under ties: the cascade's gradient differs from the
    reference's on 3.3 % ((5, 9, 13)) and 5.9 % ((3, 5, 7)) of the elements of this input."""
    from object_detection_cib_amd.engine.graph import sppf_pool_plan
    x, dcat = S.sppf_case(ks)
    C = x.shape[-1]
    cat_ref, g_ref = S.sppf_grad(x, ks, dcat)
    assert np.abs(g_ref).max() <= 25 and np.array_equal(g_ref, np.round(g_ref))
    # every partial sum of the launches, in the reference's own form (last pool first): integers below 25
    if isinstance(ks, int):
        srcs = [x]
        for _ in range(2):
            srcs.append(S.maxpool_fwd(srcs[-1], ks)[0])
        part = dcat[..., 3 * C:].astype(np.float64)
        for q in (2, 1, 0):                    # the gradient of slice q + 1 goes into slice q
            part = S.maxpool_bwd_sum(part, S.maxpool_fwd(srcs[q], ks)[1], ks, dcat[..., q * C:(q + 1) * C], np.float64)
            assert np.abs(part).max() <= 25
    else:
        part = dcat[..., :C].astype(np.float64)
        for q in reversed(range(len(ks))):     # every pool adds into slice 0
            part = S.maxpool_bwd_sum(dcat[..., (q + 1) * C:(q + 2) * C], S.maxpool_fwd(x, ks[q])[1], ks[q], part, np.float64)
            assert np.abs(part).max() <= 25
    assert np.array_equal(part, g_ref)
    if _is_arithmetic_cascade(ks):
        g_casc = S.sppf_cascade_grad(x, ks[0], len(ks), dcat)[1]
        assert np.mean(g_casc != g_ref) >= 0.01                    # this input tells the two routings apart
    cat, g = run_pool_plan(sppf_pool_plan(ks), x, dcat)
    assert_bits(cat, S.bf16_bits(cat_ref.astype(np.float32)), f"concat of {ks}")
    want = S.bf16_bits(g_ref.astype(np.float32))
    print(f"sppf {ks}: input gradient differs from the reference module's on {np.mean(g != want) * 100:.2f} % of elements")
    assert_bits(g, want, f"input gradient of {ks}")


# ---------------------------------------------------------------- g. fill, h. host pull
@pytest.mark.parametrize("n", [1, 255, 256, 257, 70000])
def test_fill_u32(n):
    lib = _lib.lib()
    buf = Buf((n,), torch.int32)
    _lib.check(lib.kodhip_fill_u32(buf.ptr, 0xDEADBEEF, n, stream()), "fill_u32")
    assert (buf.get(np.uint32) == 0xDEADBEEF).all() and buf.margins_untouched()


@pytest.mark.parametrize("nbytes", [16, 4096, 1048592])
def test_pull_from_host(nbytes):
    """kodhip_pull_from_host from a pin_memory() tensor; 1 048 592 bytes = 65 537 sixteen-byte pieces, one more than the
    256 blocks x 256 lanes of the capped grid cover in one pass"""
    lib = _lib.lib()
    rng = np.random.default_rng(nbytes)
    host = torch.from_numpy(rng.integers(0, 256, size=nbytes, dtype=np.uint8)).pin_memory()
    assert host.data_ptr() % 16 == 0
    dst = Buf((nbytes,), torch.uint8)
    assert dst.ptr % 16 == 0
    _lib.check(lib.kodhip_pull_from_host(dst.ptr, host.data_ptr(), nbytes, stream()), "pull_from_host")
    assert np.array_equal(dst.get(np.uint8), host.numpy()) and dst.margins_untouched()


# ---------------------------------------------------------------- i. refusals
def test_bad_arguments_are_refused_before_any_launch():
    """non-zero return and a message in kodhip_last_error for: C, ld or coff that is no multiple of 8, an even window
    or one above 15, more than 4 image channels, a pull that is no multiple of 16 bytes.  Every call gets real buffers,
    and they come back untouched."""
    lib = _lib.lib()
    B, H, W, C = 1, 4, 4, 8
    a, b = bf16_buf((B, 2 * H, 2 * W, 32)), bf16_buf((B, 2 * H, 2 * W, 32))
    idx = Buf((B, H, W, 32), torch.uint8)
    xin = f32_buf((1, 8, 4, 4))
    host = torch.zeros(64, dtype=torch.uint8).pin_memory()
    s = stream()

    def refused(rc, name):
        msg = lib.kodhip_last_error().decode(errors="replace")
        assert rc != 0 and name in msg, (name, rc, msg)

    for K, name in ((3, "maxpool"), (5, "maxpool5")):
        for (c, ldx, xo, ldy, yo) in ((12, 16, 0, 16, 0), (4, 16, 0, 16, 0), (C, 12, 0, 16, 0), (C, 16, 0, 20, 0),
                                      (C, 16, 4, 16, 0), (C, 16, 0, 16, 4)):
            refused(lib.kodhip_maxpool_fwd(a.ptr, ldx, xo, b.ptr, ldy, yo, idx.ptr, B, H, W, c, K, s), name + "_fwd")
            refused(lib.kodhip_maxpool_bwd(a.ptr, ldy, yo, idx.ptr, b.ptr, ldx, xo, B, H, W, c, K, None, s), name + "_bwd")
    for K in (0, 2, 4, 14, 16, 17):
        refused(lib.kodhip_maxpool_fwd(a.ptr, 16, 0, b.ptr, 16, 0, idx.ptr, B, H, W, C, K, s), "maxpool_fwd")
        refused(lib.kodhip_maxpool_bwd(a.ptr, 16, 0, idx.ptr, b.ptr, 16, 0, B, H, W, C, K, None, s), "maxpool_bwd")
    for (c, ldx, xo, ldy, yo) in ((12, 16, 0, 16, 0), (C, 12, 0, 16, 0), (C, 16, 0, 20, 0), (C, 16, 4, 16, 0), (C, 16, 0, 16, 4)):
        refused(lib.kodhip_upsample2x_fwd(a.ptr, ldx, xo, b.ptr, ldy, yo, B, H, W, c, s), "upsample2x_fwd")
        for acc in (0, 1):
            refused(lib.kodhip_upsample2x_bwd(b.ptr, ldy, yo, a.ptr, ldx, xo, acc, B, H, W, c, None, s), "upsample2x_bwd")
    refused(lib.kodhip_nchw_to_nhwc4(xin.ptr, a.ptr, 1, 5, 4, 4, s), "nchw_to_nhwc4")
    refused(lib.kodhip_nchw_to_nhwc4(xin.ptr, a.ptr, 1, 0, 4, 4, s), "nchw_to_nhwc4")
    for nbytes in (24, 8, 17):
        refused(lib.kodhip_pull_from_host(a.ptr, host.data_ptr(), nbytes, s), "pull_from_host")
    for buf in (a, b, idx, xin):
        assert buf.margins_untouched() and bool((buf.t == SENTINEL[buf.dtype]).all())
