"""Float64 reference of the YOLOv5 loss (assignment rows -> CIoU-family box loss, objectness and class BCE) and its
gradient, plus the per-row diagnostics and the comparison scheme that the loss tests (tests/test_hip_loss_edges.py) use.

The arithmetic is oracle/detection.py's `level_losses` / `iou_family` (dtype-agnostic) evaluated in float64 with
autograd, on the SAME fp32 logits and the SAME assignment rows: `gt_boxes` / `anchors` come from `D.assign` in fp32 (the
assigner is pinned bit-exactly elsewhere and stays out of the comparison) and are widened to fp64.  torch's CPU
`index_put_` runs single-threaded here ("last row wins" on cells that several rows write, the reference's small-batch
behaviour and the device's).  tests/test_loss_reference.py pins this module to tests/golden/loss.npz (vectors from the
model project) and to `D.yolo_loss` in fp32, so the GPU tests compare the kernels with torch's semantics and the
golden vectors, not with a transcription of the kernel sources.

Comparison scheme.  A kernel value is accepted when |kernel - fp64| <= K * E + floor per (level, group, matched /
unmatched cells), where E is the max error of the fp32 CPU oracle (`D.yolo_loss` in fp32) against this reference on the
same group - the yardstick is the reference arithmetic in the kernel's number format, never the kernel - and the floor
is FLOOR_ULPS fp32 ulps of the group's max |reference|: the kernel's result is itself rounded to fp32 and E can be
accidentally tiny on a group of a few elements.
"""
from __future__ import annotations

import contextlib
import math
from typing import NamedTuple, Sequence

import torch

from oracle import detection as D, synth
from oracle.network import HeadOut, NetOut

LEVELS = ("ll", "ml", "hl")
GROUPS = (("box", slice(0, 4)), ("obj", slice(4, 5)), ("cls", slice(5, None)))
FLOOR_ULPS = 4            # "a few ulps": the result's own rounding, the chain rule's 3-4 rounded factors
BAND = 1e-5               # decision guard band (relative), see `near_decision`


@contextlib.contextmanager
def single_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


class RowDiag(NamedTuple):
    """Per assignment row of one level, all fp64 (bool where said)."""
    cell: torch.Tensor          # flat cell index ((sample * A + anchor) * fh + gy) * fw + gx
    pred: torch.Tensor          # [m,4] predicted box xyxy, grid units relative to the cell
    gt: torch.Tensor            # [m,4] target box xyxy
    ties: torch.Tensor          # [m,4] bool: x1 == x1g, y1 == y1g, x2 == x2g, y2 == y2g (the min / max operands)
    iw: torch.Tensor            # unclamped overlap width  min(x2, x2g) - max(x1, x1g)
    ih: torch.Tensor
    iou: torch.Tensor           # the value of the chosen IoU kind (`ciou` for the shipped configuration)
    rows_per_cell: torch.Tensor  # how many rows of the level write this row's cell
    is_last: torch.Tensor       # bool: this row is the cell's highest row (its objectness target survives)
    near: torch.Tensor          # bool: inside the decision guard band (see `near_decision`)


class LossRef(NamedTuple):
    losses: torch.Tensor        # [3] localization, objectness, classification (fp64)
    total: torch.Tensor         # B * (loc + cls + obj)
    means: torch.Tensor         # [3 levels][3]: box mean, balance * obj mean, cls mean (NaN on a level without rows)
    grads: list                 # per level [B,A,h,w,5+nc] fp64: d total / d logits
    matched: list               # per level [B,A,h,w] bool: cells that at least one row writes
    rows: list                  # per level RowDiag
    asg: tuple                  # D.assign output (fp32)


def _widen(a: D.Assigned) -> D.Assigned:
    return a._replace(gt_boxes=a.gt_boxes.double(), anchors=a.anchors.double())


def near_decision(pred, gt, iw, ih, iou, band=BAND):
    """Rows where an fp64 comparison that the loss branches on is closer than `band` relative WITHOUT being an exact
    tie: the operands of the four min / max pairs, the clamp arguments iw / ih against 0 (relative to the operands they
    are a difference of), the IoU value against 0 (relative to 1, its scale).  fp32 may take the other branch there."""
    scale = torch.maximum(pred.abs(), gt.abs())
    d = (pred - gt).abs()
    near = ((d != 0) & (d <= band * scale)).any(1)
    sx = torch.maximum(scale[:, 0], scale[:, 2])
    sy = torch.maximum(scale[:, 1], scale[:, 3])
    near |= (iw != 0) & (iw.abs() <= band * sx)
    near |= (ih != 0) & (ih.abs() <= band * sy)
    near |= (iou != 0) & (iou.abs() <= band)
    return near


def row_diagnostics(raw64: torch.Tensor, a: D.Assigned, iou_kind: str, iou_eps: float) -> RowDiag:
    B, A, fh, fw, _ = raw64.shape
    idx = (a.samples, a.anchors_idx, a.grid_y, a.grid_x)
    cell = ((a.samples * A + a.anchors_idx) * fh + a.grid_y) * fw + a.grid_x
    with torch.no_grad():
        p = raw64[idx][:, :4]
        pxy = p[:, :2].sigmoid() * 2 - 0.5
        pwh = (p[:, 2:4].sigmoid() * 2) ** 2 * a.anchors.double()
        pred = D._to_xyxy(torch.cat((pxy, pwh), 1))
        gt = D._to_xyxy(a.gt_boxes.double())
        iw = torch.min(pred[:, 2], gt[:, 2]) - torch.max(pred[:, 0], gt[:, 0])
        ih = torch.min(pred[:, 3], gt[:, 3]) - torch.max(pred[:, 1], gt[:, 1])
        iou = D.iou_family(pred, gt, iou_kind, iou_eps).reshape(-1)
    m = cell.numel()
    counts = torch.bincount(cell, minlength=B * A * fh * fw)
    last = torch.full((B * A * fh * fw,), -1, dtype=torch.long)
    if m:
        last.scatter_reduce_(0, cell, torch.arange(m), "amax", include_self=True)
    return RowDiag(cell, pred, gt, pred == gt, iw, ih, iou, counts[cell], last[cell] == torch.arange(m),
                   near_decision(pred, gt, iw, ih, iou))


def loss_reference(img_w: int, img_h: int, raws: Sequence[torch.Tensor], targets, pos_weight=None,
                   iou_kind: str = "ciou", iou_eps: float = 1e-7) -> LossRef:
    """raws: three fp32 [B,A,h,w,5+nc] logit tensors; targets: [(boxes f64 [n,4], labels i64 [n])]."""
    B = raws[0].shape[0]
    nc = raws[0].shape[-1] - 5
    scale, dtype = B, torch.float64
    asg = D.assign(img_w, img_h, [D.Target(b, l) for b, l in targets])
    leaves = [r.detach().to(dtype).clone().requires_grad_(True) for r in raws]
    pw = None if pos_weight is None else torch.as_tensor(pos_weight, dtype=dtype)
    means = []
    with single_thread():
        lb = lo = lc = 0.0
        for x, a, bal in zip(leaves, asg, D.OBJ_BALANCE):
            b, o, c, _ = D.level_losses(x[..., :4], x[..., 4:5], x[..., 5:], _widen(a), bal, pw, iou_kind, iou_eps)
            means.append(torch.stack((b, o, c)).detach())
            lb, lo, lc = lb + b, lo + o, lc + c
        losses = (D.LAMBDA_BOX * lb, D.LAMBDA_OBJ * (img_w / 640) ** 2 * lo, D.LAMBDA_CLS * (nc / 80) * lc)
        total = scale * (losses[0] + losses[2] + losses[1])
        # a level without rows makes box / cls (and the total) NaN - 0 / 0 means - but NaN values do not enter the
        # backward pass: the other levels' gradients and every objectness gradient stay defined
        total.backward()
    grads = [x.grad for x in leaves]
    matched, rows = [], []
    for x, a in zip(leaves, asg):
        Bx, A, fh, fw, _ = x.shape
        mk = torch.zeros(Bx, A, fh, fw, dtype=torch.bool)
        mk[a.samples, a.anchors_idx, a.grid_y, a.grid_x] = True
        matched.append(mk)
        rows.append(row_diagnostics(x.detach().double(), a, iou_kind, iou_eps))
    return LossRef(torch.stack([l.detach() for l in losses]), total.detach(), torch.stack(means), grads, matched, rows, asg)


def oracle_fp32(img_w: int, img_h: int, raws, targets, pos_weight=None, iou_kind="ciou", iou_eps=1e-7):
    """`D.yolo_loss` in fp32 with autograd, unchanged: (losses [3] fp32, total, [grad per level] fp32, means [3][3])."""
    B = raws[0].shape[0]
    leaves = [r.detach().float().clone().requires_grad_(True) for r in raws]
    out = NetOut(*[HeadOut(x[..., :4], x[..., 4:5], x[..., 5:]) for x in leaves])
    pw = None if pos_weight is None else torch.as_tensor(pos_weight, dtype=torch.float32)
    with single_thread():
        res = D.yolo_loss(img_w, img_h, out, [D.Target(b, l) for b, l in targets], pos_weight=pw, iou_kind=iou_kind,
                          iou_eps=iou_eps)
        total = D.train_step_total(res, B)
        total.backward()
        means = []
        with torch.no_grad():
            asg = D.assign(img_w, img_h, [D.Target(b, l) for b, l in targets])
            for x, a, bal in zip(leaves, asg, D.OBJ_BALANCE):
                means.append(torch.stack(D.level_losses(x[..., :4], x[..., 4:5], x[..., 5:], a, bal, pw, iou_kind, iou_eps)[:3]))
    return (torch.stack([res.localization, res.objectness, res.classification]).detach(), total.detach(),
            [x.grad for x in leaves], torch.stack(means))


def ulp32(x: float) -> float:
    """Spacing of fp32 numbers at |x|."""
    x = abs(float(x))
    return 2.0 ** (math.floor(math.log2(x)) - 23) if x >= 2.0 ** -126 else 2.0 ** -149


def group_report(got, ref: LossRef, yard, drop=None):
    """got / yard: per-level gradients of the code under test / of the fp32 oracle.  Yields one record per (level, group,
    matched | unmatched): (level, group, where, err, E, max|ref|, floor) with err = max |got - ref|, E = max |yard - ref|
    over the group.  drop: per level, a bool mask over cells left out of the matched groups (guard band)."""
    for li, lvl in enumerate(LEVELS):
        r = ref.grads[li]
        g = got[li].detach().cpu().double()
        y = yard[li].double()
        for where in ("matched", "unmatched"):
            mk = ref.matched[li] if where == "matched" else ~ref.matched[li]
            if drop is not None and where == "matched":
                mk = mk & ~drop[li]
            for nm, sl in GROUPS:
                rr = r[..., sl][mk]
                if rr.numel() == 0:
                    continue
                err = (g[..., sl][mk] - rr).abs().max().item()
                E = (y[..., sl][mk] - rr).abs().max().item()
                mx = rr.abs().max().item()
                yield lvl, nm, where, err, E, mx, (FLOOR_ULPS * ulp32(mx) if mx > 0 else 0.0)


def band_cells(ref: LossRef, constructed_rows=None):
    """Cells that a guard-band row writes, per level, and the share of such rows over the case.  constructed_rows: per
    level a bool mask of rows that the case constructed on purpose - those are never left out (asserted)."""
    drop, n_near, n_rows = [], 0, 0
    for li, (rd, mk) in enumerate(zip(ref.rows, ref.matched)):
        near = rd.near
        if constructed_rows is not None:
            assert not bool((near & constructed_rows[li]).any()), "a constructed row sits in the decision guard band"
        d = torch.zeros(mk.numel(), dtype=torch.bool)
        d[rd.cell[near]] = True
        drop.append(d.view(mk.shape))
        n_near += int(near.sum())
        n_rows += near.numel()
    return drop, (n_near / n_rows if n_rows else 0.0)


# ---------------------------------------------------------------- constructed cases
class Case(NamedTuple):
    width: int
    height: int
    nc: int
    raws: list                  # three fp32 [B,A,h,w,5+nc] logit tensors
    targets: list               # [(boxes f64 [n,4] xyxy px, labels i64 [n])]
    constructed: tuple          # images whose rows are constructed on purpose (never left to the guard band)
    events: tuple               # names of the events (see `events`) that the case exists for: asserted to occur


def _raws(B, w, h, nc, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for s in D.STRIDES:
        t = torch.randn(B, 3, h // s, w // s, 5 + nc, generator=g) * scale
        t[..., 4] -= 2.0
        out.append(t)
    return out


def _random_targets(B, size, nc, seed, nmin=3, nmax=9):
    return synth.targets(B, size, nc, seed=seed, nmin=nmin, nmax=nmax)


def _boxes(rows, nc):
    b = torch.tensor([r[:4] for r in rows], dtype=torch.float64).reshape(-1, 4)
    return b, torch.arange(b.shape[0], dtype=torch.int64) % nc


def _anchor0_ciou(gcx, gw, gh, aw=10 / 8, ah=13 / 8):
    """ciou of the zero-logit anchor-0 prediction of a stride-8 cell against a target at (gcx, 0.5, gw, gh)."""
    pred = D._to_xyxy(torch.tensor([[0.5, 0.5, aw, ah]], dtype=torch.float64))
    gt = D._to_xyxy(torch.tensor([[gcx, 0.5, gw, gh]], dtype=torch.float64))
    return float(D.iou_family(pred, gt, "ciou", 1e-7))


def ties_case(nc=10, seed=31) -> Case:
    """160 px, two images.  Image 0 has zero box logits, so every prediction sits exactly on its anchor centred in its
    cell (sigmoid(0) = 0.5: px = 0.5, pw = the anchor's width, exact in fp32), and targets built around that:
    four-edge and one-edge ties on each level (anchors 10x13 @ 8, 62x45 @ 16, 116x90 @ 32), a target whose left
    neighbour's row touches the prediction (iw == 0 exactly, ciou = -0.137: the false side of the `ciou >= 0` objectness
    gate), one that is disjoint from it (iw < 0) and one overlapping just enough for a ciou slightly above 0.
    Image 1: Gaussian logits and random targets."""
    size, B = 160, 2
    raws = _raws(B, size, size, nc, seed)
    for r in raws:
        r[0, ..., :4] = 0.0
    # the smallest overlap (in steps of 1/256 cell) of a 4 x 13 px target with its left neighbour's anchor-0 prediction
    # that gives a positive ciou
    d = next(k / 256 for k in range(1, 96) if _anchor0_ciou(1.375 - k / 256, 0.5, 13 / 8) > 0)
    rows = [
        (39, 53.5, 49, 66.5),                     # stride 8, cell (5, 7): all four edges of anchor 10 x 13
        (95, 23, 109, 34),                        # stride 8, cell (12, 3): left edge only
        (41, 65.5, 103, 110.5),                   # stride 16, cell (4, 5): all four edges of anchor 62 x 45
        (22, 35, 138, 125),                       # stride 32, cell (2, 2): all four edges of anchor 116 x 90
        (89, 20.5, 159, 60.5),                    # stride 16, cell (7, 2): left edge only
        (22, 72.5, 152, 152.5),                   # stride 32, cell (2, 3): left edge only
        (121, 93.5, 125, 106.5),                  # stride 8: centre x (14 + 1.375) * 8, 4 x 13 px -> cell 14 sees x1g == x2
        (26, 117.5, 29, 130.5),                   # stride 8: centre x (2 + 1.4375) * 8, 3 px wide -> cell 2 is disjoint
        ((9.375 - d) * 8 - 2, 133.5, (9.375 - d) * 8 + 2, 146.5),     # stride 8, cell 8: ciou just above 0
    ]
    tg = [_boxes(rows, nc)] + _random_targets(1, size, nc, seed)
    return Case(size, size, nc, raws, tg, (0,), ("tie4@ll", "tie4@ml", "tie4@hl", "tie1@ll", "tie1@ml", "tie1@hl",
                                                "iw==0", "iw<0", "ciou<0", "ciou>0 small"))


def crowded_case(nc=20, seed=32) -> Case:
    """160 px.  Image 0: a 20 x 20 px box (passes the ratio filter of all three stride-8 anchors) 9 and 17 times with
    different labels, 11 and 8 times with the size growing by 1/4 px per copy (same cells, different IoU per row, so
    that WHICH row's objectness target survives is visible), and 3, 2 and 1 times - at centres far enough apart that
    the stride-8 cells of different groups are disjoint.  Image 1: Gaussian logits, random targets."""
    size, B = 160, 2
    raws = _raws(B, size, size, nc, seed)
    rows = []
    for (cx, cy), n, jitter in (((21, 21), 9, 0.0), ((69, 29), 17, 0.0), ((117, 21), 11, 0.25), ((29, 77), 8, 0.25),
                                ((77, 85), 3, 0.0), ((125, 77), 2, 0.0), ((37, 133), 1, 0.0)):
        for i in range(n):
            hw = 10 + jitter * i / 2
            rows.append((cx - hw, cy - hw, cx + hw, cy + hw))
    tg = [_boxes(rows, nc)] + _random_targets(1, size, nc, seed)
    return Case(size, size, nc, raws, tg, (0,), ("rows/cell 1", "rows/cell 2", "rows/cell 3", "rows/cell 8",
                                                "rows/cell 9", "rows/cell 11", "rows/cell 17", "last row differs"))


def saturated_case(nc=3, seed=33, wh_scale=1.5, size=128, B=2) -> Case:
    """xy logits x 30, objectness and class logits x 40 (sigmoid exactly 0 or 1 in fp32 on most of them), wh logits x
    `wh_scale`, and on the first rows of every level logits planted at +-100 and +-1e4 (expf overflows to inf).
    wh_scale = 30 saturates the box size too: w1 / (h1 + eps) with w1, h1 -> 0 makes the function itself
    ill-conditioned (the fp32 oracle is 13 % of max away from fp64 there), which is only checked for finiteness."""
    raws = _raws(B, size, size, nc, seed)
    tg = _random_targets(B, size, nc, seed)
    tg[0] = (torch.cat((tg[0][0], torch.tensor([[20.0, 24.0, 100.0, 110.0]], dtype=torch.float64))),     # rows on every level
             torch.cat((tg[0][1], torch.tensor([nc - 1]))))
    for r in raws:
        r[..., 0:2] *= 30.0
        r[..., 2:4] *= wh_scale
        r[..., 4:] *= 40.0
    plant = ((0, 100.0), (1, -100.0), (0, -1e4), (1, 1e4), (4, 1e4), (4, -1e4), (4, 100.0), (5, 1e4), (5, -1e4),
             (5 + nc - 1, -100.0), (5 + nc - 1, 100.0))
    for r, a in zip(raws, D.assign(size, size, [D.Target(b, l) for b, l in tg])):
        for i, (slot, v) in enumerate(plant):
            if i < a.samples.numel():
                r[a.samples[i], a.anchors_idx[i], a.grid_y[i], a.grid_x[i], slot] = v
    return Case(size, size, nc, raws, tg, (), ("sigmoid == 1", "sigmoid == 0", "planted 1e4"))


def random_case(B, w, h, nc, seed) -> Case:
    """Gaussian logits, random targets: the class-count / ragged-chunk sweep."""
    tg = synth.targets(B, min(w, h), nc, seed=seed, nmin=2, nmax=7)
    return Case(w, h, nc, _raws(B, w, h, nc, seed), tg, (), ())


def empty_case(kind: str, nc=10, seed=34) -> Case:
    """'level': one tiny box, no row on the coarse level (NaN box / cls loss there); 'batch': no box at all."""
    size, B = 128, 2
    e = (torch.zeros((0, 4), dtype=torch.float64), torch.zeros(0, dtype=torch.int64))
    tg = [(torch.tensor([[10, 10, 18, 19]], dtype=torch.float64), torch.tensor([3])), e] if kind == "level" else [e, e]
    return Case(size, size, nc, _raws(B, size, size, nc, seed), tg, (), ("empty level",))


def events(case: Case, ref: LossRef) -> dict:
    """name -> number of rows (or cells) of the case on which the event occurs, from the fp64 diagnostics."""
    ev = {}
    con = torch.tensor(case.constructed, dtype=torch.long)
    allrows = []
    for lvl, rd, a in zip(LEVELS, ref.rows, ref.asg):
        c = torch.isin(a.samples, con)
        nt = rd.ties.sum(1)
        ev[f"tie4@{lvl}"] = int(((nt == 4) & c).sum())
        ev[f"tie1@{lvl}"] = int(((nt == 1) & c).sum())
        allrows.append((rd, c))
        ev[f"rows@{lvl}"] = rd.cell.numel()
    cat = lambda f: torch.cat([f(rd)[c] for rd, c in allrows]) if allrows else torch.zeros(0)
    iw, ih, iou, rpc = cat(lambda r: r.iw), cat(lambda r: r.ih), cat(lambda r: r.iou), cat(lambda r: r.rows_per_cell)
    ev["iw==0"] = int(((iw == 0) | (ih == 0)).sum())
    ev["iw<0"] = int(((iw < 0) | (ih < 0)).sum())
    ev["ciou<0"] = int((iou < 0).sum())
    ev["ciou>0 small"] = int(((iou > 0) & (iou < 0.02)).sum())
    for n in (1, 2, 3, 8, 9, 11, 17):
        ev[f"rows/cell {n}"] = int((rpc == n).sum())
    ev["rows/cell max"] = int(rpc.max()) if rpc.numel() else 0
    # crowded cells on which the surviving (last) row's IoU differs visibly from the first row's
    differs = 0
    for rd, c in allrows:
        for cell in torch.unique(rd.cell[c & (rd.rows_per_cell > 8)]).tolist():
            v = rd.iou[rd.cell == cell].clamp(0)
            differs += int((v[-1] - v[0]).abs() > 1e-3)
    ev["last row differs"] = differs
    s = torch.cat([r[..., [0, 1, 4]].reshape(-1) for r in case.raws] + [r[..., 5:].reshape(-1) for r in case.raws])
    sg = torch.sigmoid(s)
    ev["sigmoid == 1"], ev["sigmoid == 0"] = int((sg == 1).sum()), int((sg == 0).sum())
    ev["planted 1e4"] = int((s.abs() == 1e4).sum())
    ev["empty level"] = sum(int(rd.cell.numel() == 0) for rd in ref.rows)
    return ev


def constructed_rows(case: Case, ref: LossRef):
    con = torch.tensor(case.constructed, dtype=torch.long)
    return [torch.isin(a.samples, con) for a in ref.asg]


NC_SWEEP = (1, 2, 3, 7, 20, 59, 80, 91, 123)
SWEEP_SHAPES = ((1, 96, 96), (3, 160, 160), (2, 160, 96))       # B, width, height: no level's cell count is a multiple of 64


def cases() -> dict:
    """name -> thunk building the Case: everything tests/test_hip_loss_edges.py runs against the kernels (and
    tests/test_loss_reference.py checks on the CPU: events occur, guard band within its cap)."""
    c = {"ties": ties_case, "crowded": crowded_case,
         "saturated_nc3": lambda: saturated_case(3, 33), "saturated_nc80": lambda: saturated_case(80, 35),
         "empty_level": lambda: empty_case("level"), "empty_batch": lambda: empty_case("batch")}
    for nc in NC_SWEEP:
        for B, w, h in SWEEP_SHAPES:
            c[f"nc{nc}_b{B}_{w}x{h}"] = (lambda B=B, w=w, h=h, nc=nc: random_case(B, w, h, nc, seed=100 + nc + B))
    return c


def pos_weight_for(nc: int):
    """A fixed, uneven per-class weight vector (1 .. 9)."""
    return [1.0 + 8.0 * ((7 * i) % 11) / 10.0 for i in range(nc)]


BAND_SHARE = 0.005        # at most this share of a case's rows may sit in the decision guard band


def expected_events(case: Case, kind: str, eps: float):
    """The case's events that exist under this IoU kind: plain IoU is never negative, and the 'just above 0' row is
    placed by the shipped CIoU's value."""
    out = []
    for e in case.events:
        if e == "ciou<0" and kind == "iou":
            continue
        if e == "ciou>0 small" and kind != "ciou":
            continue
        out.append(e)
    return out
