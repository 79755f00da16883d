"""Reference of the YOLOv5 loss with its remaining hyper-parameters - focal modulation of both BCE terms (`fl_gamma`,
`fl_alpha`), smoothed class targets (`label_smoothing`) and an objectness pos_weight (`obj_pos_weight`) - for
tests/test_focal_reference.py (CPU) and tests/test_hip_focal.py (GPU).

The model project has none of these options, so the definition is a torch program: oracle/detection.py's `level_losses`
with YOLOv5's `FocalLoss` wrapper around its two `binary_cross_entropy_with_logits` calls and YOLOv5's `smooth_BCE`
targets, dtype-agnostic like the function it restates.  Autograd on it in fp64 defines the gradients (`reference`); the
same program in fp32 is the yardstick (`oracle_fp32`).  Everything else - `D.assign`, `D.iou_family`, `D._to_xyxy`, the
constructed cases, the row diagnostics and the comparison scheme - is tests/loss_reference.py's, unchanged.  At neutral
options `level_losses` here equals `D.level_losses` bit for bit (tests/test_focal_reference.py), which ties this module
to the reference already pinned to the golden vectors.

The objectness target stays clamp(iou, 0) scattered into zeros, last row wins, NOT detached.  Under focal modulation the
target's gradient depends on the target itself, so every row that wrote a cell receives d loss / d t evaluated at the
LAST row's value (torch's index_put_ backward), gated by its own iou >= 0.
"""
from __future__ import annotations

from typing import NamedTuple

import torch
import torch.nn.functional as F

import loss_reference as R
from loss_reference import D


class Options(NamedTuple):
    gamma: float = 0.0          # fl_gamma: 0 = plain BCE
    alpha: float = 0.25         # fl_alpha
    smoothing: float = 0.0      # label_smoothing
    obj_pw: float = 1.0         # obj_pos_weight

    @property
    def neutral(self) -> bool:
        return self.gamma == 0 and self.smoothing == 0 and self.obj_pw == 1


# what tests/test_hip_focal.py runs on the GPU: (gamma, alpha, smoothing, obj_pw)
OPTION_SETS = (Options(1.5, 0.25, 0.0, 1.0), Options(2.0, 0.25, 0.1, 0.7), Options(1.0, 0.5, 0.1, 2.0),
               Options(0.0, 0.25, 0.1, 1.0), Options(0.0, 0.25, 0.0, 2.0))
CONSTRUCTED = ("ties", "crowded", "saturated_nc3", "saturated_nc80", "empty_level", "empty_batch")
SWEEP = {"nc1_b1_96x96": (0, 1), "nc7_b3_160x160": (1, 3), "nc59_b2_160x96": (2, 4), "nc123_b3_160x160": (0, 2)}


def focal_bce(x, t, pos_weight, gamma, alpha):
    """YOLOv5's FocalLoss(BCEWithLogitsLoss(pos_weight), gamma, alpha), mean over all elements as the reference reduces.
    gamma == 0 is the reference's own call (reduction="mean"): the same function as reduction="none" + mean(), but torch's
    fused mean backward rounds (sigmoid - t) * g / N in another order, and neutral options must give the oracle's bits."""
    if not gamma > 0:
        return F.binary_cross_entropy_with_logits(x, t, reduction="mean", pos_weight=pos_weight)
    l = F.binary_cross_entropy_with_logits(x, t, reduction="none", pos_weight=pos_weight)
    p = torch.sigmoid(x)
    p_t = t * p + (1 - t) * (1 - p)
    l = l * (t * alpha + (1 - t) * (1 - alpha)) * (1.0 - p_t) ** gamma
    return l.mean()


def level_losses(box, obj, cls, a, balance, options: Options = Options(), pos_weight=None, iou_kind="ciou", iou_eps=1e-7):
    """`D.level_losses` with the options; returns (box_mean, obj_scaled, cls_mean, iou)."""
    idx = (a.samples, a.anchors_idx, a.grid_y, a.grid_x)
    p = box[idx]
    pxy = p[:, :2].sigmoid() * 2 - 0.5
    pwh = (p[:, 2:4].sigmoid() * 2) ** 2 * a.anchors
    iou = D.iou_family(D._to_xyxy(torch.cat((pxy, pwh), 1)), D._to_xyxy(a.gt_boxes), iou_kind, iou_eps).squeeze()
    l_box = (1 - iou).mean()
    tobj = torch.zeros_like(obj).squeeze(-1)
    tobj[idx] = iou.clamp(0).type(tobj.dtype)            # NOT detached
    # (a pos_weight of one is no pos_weight: torch's target gradient takes another route when one is given)
    opw = None if options.obj_pw == 1 else torch.tensor([options.obj_pw], dtype=obj.dtype)
    l_obj = balance * focal_bce(obj, tobj.unsqueeze(-1), opw, options.gamma, options.alpha)
    pc = cls[idx]
    t = torch.full_like(pc, 0.5 * options.smoothing)
    t[range(t.shape[0]), a.labels] = 1 - 0.5 * options.smoothing
    l_cls = focal_bce(pc, t, pos_weight, options.gamma, options.alpha)
    return l_box, l_obj, l_cls, iou


def _program(case: R.Case, options: Options, pos_weight, kind, eps, dtype):
    """The whole loss and its backward in `dtype`: (losses [3], total, leaves, means [3][3], asg)."""
    B = case.raws[0].shape[0]
    asg = D.assign(case.width, case.height, [D.Target(b, l) for b, l in case.targets])
    leaves = [r.detach().to(dtype).clone().requires_grad_(True) for r in case.raws]
    pw = None if pos_weight is None else torch.as_tensor(pos_weight, dtype=dtype)
    means = []
    with R.single_thread():
        lb = lo = lc = 0.0
        for x, a, bal in zip(leaves, asg, D.OBJ_BALANCE):
            a = a._replace(gt_boxes=a.gt_boxes.to(dtype), anchors=a.anchors.to(dtype))
            b, o, c, _ = level_losses(x[..., :4], x[..., 4:5], x[..., 5:], a, bal, options, pw, kind, eps)
            means.append(torch.stack((b, o, c)).detach())
            lb, lo, lc = lb + b, lo + o, lc + c
        losses = (D.LAMBDA_BOX * lb, D.LAMBDA_OBJ * (case.width / 640) ** 2 * lo, D.LAMBDA_CLS * (case.nc / 80) * lc)
        total = B * (losses[0] + losses[2] + losses[1])
        total.backward()
    return torch.stack([l.detach() for l in losses]), total.detach(), leaves, torch.stack(means), asg


def reference(case: R.Case, options: Options, pos_weight=None, kind="ciou", eps=1e-7) -> R.LossRef:
    """fp64 with autograd, as `R.loss_reference` (same record, same diagnostics)."""
    losses, total, leaves, means, asg = _program(case, options, pos_weight, kind, eps, torch.float64)
    matched, rows = [], []
    for x, a in zip(leaves, asg):
        Bx, A, fh, fw, _ = x.shape
        mk = torch.zeros(Bx, A, fh, fw, dtype=torch.bool)
        mk[a.samples, a.anchors_idx, a.grid_y, a.grid_x] = True
        matched.append(mk)
        rows.append(R.row_diagnostics(x.detach().double(), a, kind, eps))
    return R.LossRef(losses, total, means, [x.grad for x in leaves], matched, rows, asg)


def oracle_fp32(case: R.Case, options: Options, pos_weight=None, kind="ciou", eps=1e-7):
    """The same program in fp32, as `R.oracle_fp32`: (losses [3] fp32, total, [grad per level] fp32, means [3][3])."""
    losses, total, leaves, means, _ = _program(case, options, pos_weight, kind, eps, torch.float32)
    return losses, total, [x.grad for x in leaves], means


# ---------------------------------------------------------------- the closed forms that the kernels evaluate
def closed_forms(x, t, pw, g, al):
    """numpy fp64, element-wise: (L, dL/dx, dL/dt) of  L = bce * af * q^g  (g == 0: L = bce)."""
    import numpy as np
    sp = np.log1p(np.exp(-np.abs(x))) + np.maximum(-x, 0.0)
    e = np.exp(-np.abs(x))
    p = np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    omp = np.where(x >= 0, e / (1.0 + e), 1.0 / (1.0 + e))
    w = 1.0 + (pw - 1.0) * t
    bce = (1.0 - t) * x + w * sp
    dbx, dbt = (1.0 - t) - w * omp, -x + (pw - 1.0) * sp
    if g == 0:
        return bce, dbx, dbt
    q = t * omp + (1.0 - t) * p
    af = t * al + (1.0 - t) * (1.0 - al)
    qg1 = np.power(q, g - 1.0)
    mf = qg1 * q
    return (bce * af * mf, af * (dbx * mf - bce * g * qg1 * (2.0 * t - 1.0) * p * omp),
            dbt * af * mf + bce * (2.0 * al - 1.0) * mf - bce * af * g * qg1 * (2.0 * p - 1.0))
