"""Gradient norm, clipping and the clipped fused SGD (csrc/misc_ops.hip) against torch on the same data.

Yardstick for every norm: torch.linalg.vector_norm over the counted elements of the fp32 product g * grad_scale, widened
to fp64, rounded once to fp32.  The kernel squares and sums in fp64 too: n <= 2^25 squares accumulate a relative error
below 1e-8, far under half an fp32 ulp (6e-8), so only the final rounding is left - the bar is 1 fp32 ulp.  torch's own fp32
clip_grad_norm_ is NOT the yardstick (its foreach norm is tens of ulp away on millions of elements); where a test compares
with it, the bar is torch's own measured distance to the fp64 value plus that 1 ulp.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hip_helpers import stream  # noqa: E402
from object_detection_cib_amd import _lib  # noqa: E402

LR, MOM, WD = (0.1, 0.01, 0.02), (0.8, 0.9, 0.937), (0.0, 5e-4, 0.0)


def ulps(got: torch.Tensor, ref64: torch.Tensor) -> int:
    """distance in fp32 ulps between got (fp32) and the fp64 reference rounded to fp32"""
    a = got.detach().cpu().float().reshape(-1).view(torch.int32).long()
    b = ref64.detach().cpu().double().float().reshape(-1).view(torch.int32).long()
    return int((a - b).abs().max())


def make_arena(granules: int, seed: int, decades: float = 3.0, masked: bool = True):
    """A synthetic arena as the engine lays it out: a group id per 64-element granule (all three groups and padding
    granules), a per-element count mask with partially masked granules, magnitudes spread over `decades` decades."""
    g = torch.Generator().manual_seed(seed)
    n = 64 * granules
    gid = torch.randint(0, 3, (granules,), generator=g).to(torch.uint8)
    gid[torch.rand(granules, generator=g) < 0.1] = 255
    gid[:7] = torch.tensor([0, 1, 2, 1, 255, 0, 2], dtype=torch.uint8)
    gr = torch.randn(n, generator=g) * torch.pow(10.0, (torch.rand(n, generator=g) - 0.5) * decades)
    p = torch.randn(n, generator=g)
    keep = torch.ones(n, dtype=torch.uint8)
    if masked:
        keep.view(granules, 64)[torch.rand(granules, generator=g) < 0.2] = 0              # whole granules (frozen tensors)
        part = torch.rand(granules, generator=g) < 0.3                                    # partially masked granules
        tail = torch.randint(1, 64, (granules,), generator=g)
        cols = torch.arange(64).expand(granules, 64)
        keep.view(granules, 64)[part[:, None] & (cols >= tail[:, None])] = 0
    return SimpleArena(p, gr, gid, keep if masked else None)


class SimpleArena:
    def __init__(self, p, gr, gid, keep):
        self.n = p.numel()
        self.p0, self.gr, self.gid, self.keep = p, gr, gid, keep
        self.group = self.gid.repeat_interleave(64)                      # group id per element
        self.counted = (self.group <= 2) & (keep.bool() if keep is not None else torch.ones(self.n, dtype=torch.bool))
        self.gid_d = gid.cuda()
        self.keep_d = keep.cuda() if keep is not None else None
        lib = _lib.lib()
        self.clip = torch.zeros(lib.kodhip_clip_block_bytes() // 4, device="cuda")
        self.ws = torch.zeros(lib.kodhip_grad_norm_workspace_bytes() // 8, dtype=torch.float64, device="cuda")

    def keep_ptr(self):
        return None if self.keep_d is None else self.keep_d.data_ptr()

    def ref_norms(self, gr, scale):
        """[total, bias, decay, norm] in fp64 over the counted elements of the fp32 product"""
        prod = (gr.float() * torch.tensor(scale, dtype=torch.float32)).double()
        parts = [torch.linalg.vector_norm(prod[self.counted & (self.group == k)]) for k in range(3)]
        return torch.stack([torch.linalg.vector_norm(prod[self.counted])] + parts)

    def norm(self, gr_d, hyper, max_norm=float("inf"), skip=0, nt=0):
        self.clip[8] = max_norm
        _lib.check(_lib.lib().kodhip_grad_norm(gr_d.data_ptr(), self.gid_d.data_ptr(), self.keep_ptr(), self.n,
                                               hyper.data_ptr(), self.clip.data_ptr(), self.ws.data_ptr(), skip, nt,
                                               stream()), "grad_norm")

    def sgd_clipped(self, p, gr_d, buf, hyper, mode, skip=0):
        _lib.check(_lib.lib().kodhip_sgd_nesterov_clipped(p.data_ptr(), gr_d.data_ptr(), buf.data_ptr(), self.gid_d.data_ptr(),
                                                          self.keep_ptr(), self.n, hyper.data_ptr(), self.clip.data_ptr(),
                                                          mode, skip, stream()), "sgd_clipped")

    def sgd_plain(self, p, gr_d, buf, hyper):
        lib = _lib.lib()
        if self.keep_d is None:
            _lib.check(lib.kodhip_sgd_nesterov(p.data_ptr(), gr_d.data_ptr(), buf.data_ptr(), self.gid_d.data_ptr(), self.n,
                                               hyper.data_ptr(), stream()), "sgd")
        else:
            _lib.check(lib.kodhip_sgd_nesterov_masked(p.data_ptr(), gr_d.data_ptr(), buf.data_ptr(), self.gid_d.data_ptr(),
                                                      self.keep_d.data_ptr(), self.n, hyper.data_ptr(), stream()), "sgd_masked")

    def torch_sgd(self, nesterov):
        """torch.optim.SGD over the updated elements, one Parameter per optimizer group (the update is elementwise)"""
        idx = [torch.nonzero(self.counted & (self.group == k)).flatten() for k in range(3)]
        refs = [torch.nn.Parameter(self.p0[i].clone()) for i in idx]
        opt = torch.optim.SGD([dict(params=[refs[k]], lr=LR[k], momentum=MOM[k], weight_decay=WD[k]) for k in range(3)],
                              lr=0.1, nesterov=nesterov, momentum=0.5)
        return idx, refs, opt


def hyper_block(scale, nesterov=True):
    return torch.tensor([*LR, *MOM, *WD, scale, 1.0 if nesterov else 0.0, 0.0], dtype=torch.float32, device="cuda")


def torch_coef(total32: torch.Tensor, max_norm: float) -> torch.Tensor:
    """the coefficient exactly as torch.nn.utils.clip_grad_norm_ forms it, in fp32"""
    return torch.clamp(max_norm / (total32 + 1e-6), max=1.0)


@pytest.mark.parametrize("granules,decades,masked", [(7, 1.0, True), (40, 3.0, True), (40, 3.0, False),
                                                     (3 * 2 ** 15, 6.0, True)])          # the last: 6.3 M elements
def test_grad_norm_vs_fp64_one_ulp_and_same_bits(granules, decades, masked):
    """total and group norms within 1 fp32 ulp of the fp64 value; two runs, non-temporal loads and a graph replay give the
    same bits; 1e30 / NaN in padding granules and masked elements change nothing."""
    A = make_arena(granules, seed=granules, decades=decades, masked=masked)
    scale = 0.37
    hyper = hyper_block(scale)
    ref = A.ref_norms(A.gr, scale)
    gr_d = A.gr.cuda()
    A.norm(gr_d, hyper, max_norm=0.5 * float(ref[0]))
    first = A.clip.clone()
    d = [ulps(first[k], ref[k]) for k in range(4)]
    print(f"n = {A.n}: ulp distance of [total, bias, decay, norm] to the fp64 norms: {d}; total = {float(ref[0]):.9g}")
    assert max(d) <= 1, (d, first[:4].tolist(), ref.tolist())
    want_coef = torch_coef(ref[0].float(), 0.5 * float(ref[0]))
    print(f"coefficient {float(first[4]):.9g}, torch forms {float(want_coef):.9g} from the fp64-reference norm")
    assert abs(float(first[4]) - float(want_coef)) <= 2.0 ** -22 * float(want_coef)       # the norm's 1 ulp, the product's 1
    assert first[5].item() == 0.0 and first[6].item() == 0.0
    A.norm(gr_d, hyper, max_norm=0.5 * float(ref[0]))
    assert torch.equal(A.clip.view(torch.int32), first.view(torch.int32))
    A.norm(gr_d, hyper, max_norm=0.5 * float(ref[0]), nt=1)
    assert torch.equal(A.clip.view(torch.int32), first.view(torch.int32))
    # what must not count: padding granules and masked elements
    poison = A.gr.clone()
    dead = ~A.counted
    poison[dead] = torch.where(torch.arange(int(dead.sum())) % 2 == 0, torch.tensor(1e30), torch.tensor(float("nan")))
    assert dead.any()
    gp = poison.cuda()
    A.norm(gp, hyper, max_norm=0.5 * float(ref[0]))
    assert torch.equal(A.clip.view(torch.int32), first.view(torch.int32)), (A.clip[:7].tolist(), first[:7].tolist())
    # a captured graph, replayed twice on changed clip-block inputs
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        A.norm(gp, hyper, max_norm=0.5 * float(ref[0]))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _lib.check(_lib.lib().kodhip_grad_norm(gp.data_ptr(), A.gid_d.data_ptr(), A.keep_ptr(), A.n, hyper.data_ptr(),
                                               A.clip.data_ptr(), A.ws.data_ptr(), 0, 0, stream()), "grad_norm")
    for _ in range(2):
        A.clip[:6].fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(A.clip[:6].view(torch.int32), first[:6].view(torch.int32))
    A.clip[8] = 2.0 * float(ref[0])                   # max_norm is device data: a replay sees the new value
    graph.replay()
    assert A.clip[4].item() == 1.0 and torch.equal(A.clip[:4].view(torch.int32), first[:4].view(torch.int32))


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("nesterov", [True, False])
def test_clipped_sgd_norm_mode_vs_torch(nesterov, masked):
    """(g * scale) * coef, then the existing update: torch.optim.SGD over the fp32 gradients times the coefficient formed in
    fp32 from the fp64-reference norm; test_sgd_nesterov's bars, three steps with new gradients each."""
    A = make_arena(40, seed=11, masked=masked)
    scale = 0.5
    hyper = hyper_block(scale, nesterov)
    idx, refs, opt = A.torch_sgd(nesterov)
    p, buf = A.p0.clone().cuda(), torch.zeros(A.n, device="cuda")
    g = torch.Generator().manual_seed(3)
    for step in range(3):
        gr = A.gr * (1.0 + step) + 0.1 * torch.randn(A.n, generator=g)
        ref = A.ref_norms(gr, scale)
        max_norm = 0.3 * float(ref[0])
        gr_d = gr.cuda()
        A.norm(gr_d, hyper, max_norm=max_norm)
        A.sgd_clipped(p, gr_d, buf, hyper, 0)
        assert ulps(A.clip[0], ref[0]) <= 1
        coef = torch_coef(ref[0].float(), max_norm)
        assert 0.29 < float(coef) < 0.31
        for k in range(3):
            refs[k].grad = (gr[idx[k]] * scale) * coef
        opt.step()
    got = p.cpu()
    for k in range(3):
        err = (got[idx[k]] - refs[k].detach()).abs().max().item()
        print(f"group {k}: max |HIP - torch| = {err:.3g}")
        torch.testing.assert_close(got[idx[k]], refs[k].detach(), rtol=1e-6, atol=1e-6)
    assert torch.equal(got[~A.counted], A.p0[~A.counted])            # masked and padding elements untouched


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("nesterov", [True, False])
def test_coefficient_one_is_bit_identical_to_the_unclipped_kernels(nesterov, masked):
    A = make_arena(40, seed=5, masked=masked)
    hyper = hyper_block(0.5, nesterov)
    gr_d = A.gr.cuda()
    pa, ba = A.p0.clone().cuda(), torch.zeros(A.n, device="cuda")
    pb, bb = A.p0.clone().cuda(), torch.zeros(A.n, device="cuda")
    for step in range(3):
        A.norm(gr_d, hyper, max_norm=10.0 * float(A.ref_norms(A.gr, 0.5)[0]))
        assert A.clip[4].item() == 1.0
        A.sgd_clipped(pa, gr_d, ba, hyper, 0)
        A.sgd_plain(pb, gr_d, bb, hyper)
    assert torch.equal(pa.view(torch.int32), pb.view(torch.int32))
    assert torch.equal(ba.view(torch.int32), bb.view(torch.int32))
    assert not torch.equal(pa.cpu(), A.p0)


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("nesterov", [True, False])
def test_value_mode_vs_clip_grad_value(nesterov, masked):
    """clamp(g * scale, -v, +v) then the update: torch.nn.utils.clip_grad_value_ + torch.optim.SGD; a NaN gradient stays NaN"""
    A = make_arena(40, seed=7, masked=masked)
    scale, v = 0.5, 0.2
    hyper = hyper_block(scale, nesterov)
    gr = A.gr.clone()
    nan_at = int(torch.nonzero(A.counted)[17])
    gr[nan_at] = float("nan")
    idx, refs, opt = A.torch_sgd(nesterov)
    p, buf = A.p0.clone().cuda(), torch.zeros(A.n, device="cuda")
    gr_d = gr.cuda()
    A.clip[8] = v
    for step in range(3):
        A.sgd_clipped(p, gr_d, buf, hyper, 1)
        for k in range(3):
            refs[k].grad = gr[idx[k]] * scale
        torch.nn.utils.clip_grad_value_(refs, v)
        opt.step()
    got = p.cpu()
    assert torch.isnan(got[nan_at]) and int(torch.isnan(got).sum()) == 1
    clipped = int(((gr * scale).abs() > v)[A.counted].sum())
    assert 0 < clipped < int(A.counted.sum())
    for k in range(3):
        torch.testing.assert_close(got[idx[k]], refs[k].detach(), rtol=1e-6, atol=1e-6, equal_nan=True)
    assert torch.equal(got[A.group > 2], A.p0[A.group > 2])


@pytest.mark.parametrize("mode", [0, 1])
def test_skip_nonfinite(mode):
    """one Inf in a counted gradient: parameters and momentum unchanged bit for bit, count = 1; the same Inf in a masked or
    a padding element: a normal step, count = 0.  Without the option the NaN coefficient reaches the parameters (torch's
    error_if_nonfinite=False)."""
    A = make_arena(40, seed=9, masked=True)
    hyper = hyper_block(0.5)
    p0 = A.p0.cuda()
    b0 = torch.randn(A.n, generator=torch.Generator().manual_seed(1)).cuda()
    ref = A.ref_norms(A.gr, 0.5)

    def run(gr, skip):
        p, buf = p0.clone(), b0.clone()
        gr_d = gr.cuda()
        A.norm(gr_d, hyper, max_norm=0.5 * float(ref[0]), skip=skip)
        A.sgd_clipped(p, gr_d, buf, hyper, mode, skip)
        return p, buf

    A.clip.zero_()
    clean_p, clean_b = run(A.gr, 1)
    assert A.clip[6].item() == 0.0 and not torch.equal(clean_p, p0)
    bad = A.gr.clone()
    bad[int(torch.nonzero(A.counted)[5])] = float("inf")
    p, buf = run(bad, 1)
    assert A.clip[5].item() == 1.0 and A.clip[6].item() == 1.0 and torch.isinf(A.clip[0])
    assert torch.equal(p.view(torch.int32), p0.view(torch.int32)) and torch.equal(buf.view(torch.int32), b0.view(torch.int32))
    p, buf = run(bad, 1)
    assert A.clip[6].item() == 2.0                                  # the count accumulates over steps
    A.clip.zero_()
    for where in (int(torch.nonzero((A.group <= 2) & ~A.counted)[3]), int(torch.nonzero(A.group > 2)[3])):
        masked_inf = A.gr.clone()
        masked_inf[where] = float("inf")
        p, buf = run(masked_inf, 1)
        assert A.clip[5].item() == 0.0 and A.clip[6].item() == 0.0
        assert torch.equal(p.view(torch.int32), clean_p.view(torch.int32))
        assert torch.equal(buf.view(torch.int32), clean_b.view(torch.int32))
    if mode == 0:                                                   # default off: NaN norm -> NaN coefficient -> NaN parameters
        bad[int(torch.nonzero(A.counted)[5])] = float("nan")
        p, buf = run(bad, 0)
        assert A.clip[6].item() == 0.0 and torch.isnan(A.clip[4]) and torch.isnan(p.cpu()[A.counted]).all()


def test_inplace_scale_and_clamp():
    """the eager path's g *= coef (and the clamp) over the counted elements only"""
    A = make_arena(40, seed=13, masked=True)
    hyper = hyper_block(1.0)
    ref = A.ref_norms(A.gr, 1.0)
    gr_d = A.gr.cuda()
    A.norm(gr_d, hyper, max_norm=0.25 * float(ref[0]))
    coef = A.clip[4].cpu()
    lib = _lib.lib()
    _lib.check(lib.kodhip_grad_clip_inplace(gr_d.data_ptr(), A.gid_d.data_ptr(), A.keep_ptr(), A.n, A.clip.data_ptr(), 0,
                                            stream()), "scale")
    want = torch.where(A.counted, A.gr * coef, A.gr)
    assert torch.equal(gr_d.cpu().view(torch.int32), want.view(torch.int32))
    gr_d = A.gr.cuda()
    A.clip[8] = 0.3
    _lib.check(lib.kodhip_grad_clip_inplace(gr_d.data_ptr(), A.gid_d.data_ptr(), A.keep_ptr(), A.n, A.clip.data_ptr(), 1,
                                            stream()), "clamp")
    want = torch.where(A.counted, A.gr.clamp(-0.3, 0.3), A.gr)
    assert torch.equal(gr_d.cpu().view(torch.int32), want.view(torch.int32))
