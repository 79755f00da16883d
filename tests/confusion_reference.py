"""Plain reference of the detection confusion matrix (csrc/confusion.hip, DeviceConfusionMatrix) and the inputs that
tests/test_confusion_reference.py (CPU) and tests/test_hip_confusion.py (GPU) run.  Nothing here touches the HIP library.

The rule is YOLOv5's ConfusionMatrix.process_batch made deterministic; matching is class-agnostic, boxes are fp64.  Per image:
1  a detection is kept when score > conf_thres (fp32, strict); a kept detection whose class, or a ground truth whose
   label, is outside [0, nc) takes no part and is counted nowhere;
2  IoU = inter / (area_d + area_g - inter), width / height of the intersection clamped at 0, no +1; a pair is a candidate
   when IoU > iou_thres (strict; NaN never);
3  every kept detection picks its candidate of largest IoU, equal IoUs -> the lower ground-truth index;
4  every ground truth takes, among the detections that picked it, the one of largest IoU, equal IoUs -> the lower
   detection index; a detection that loses is NOT offered another ground truth;
5  matched pair -> M[class][label]; ground truth nobody took -> M[nc][label]; kept detection not taken -> M[class][nc].

Exactness.  Every coordinate of every case is a multiple of 1/4 below 2048: areas, intersections and unions are exact in
fp64 with or without fused multiply-adds, the IoU is one correctly rounded division on either side, so matrices are compared
with integer equality and a mismatch is a bug.  Ties in the hand cases are real ties.

`confusion_ref` is loops over per-image lists; like `val_reference.match_ref` it counts what happened into an `events` dict
(tie3 / tie4: equal-IoU choices in step 3 / 4; lost: detections that picked a ground truth and lost it; offdiag: matches
with class != label; exact_thr: pairs with IoU == iou_thres; exact_conf: scores == conf_thres; matched, bg_fp, missed), and
the CPU test asserts those, which keeps a GPU test from passing on inputs that no longer reach what they were built for.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

from val_reference import _f32, _grid_boxes, evaluator_batches, random_scene

EVENT_KEYS = ("tie3", "tie4", "lost", "offdiag", "exact_thr", "exact_conf", "matched", "bg_fp", "missed")
# the scenes at 80 and 81 classes lie on either side of the kernel's on-chip / direct-atomic switch-over
# (kodhip_confusion_lds_classes() == 80: asserted in tests/test_confusion_reference.py)
SWITCH_NC = (80, 81)


def _iou(d, g):
    """fp64 IoU of two xyxy boxes; 0 / 0 -> NaN"""
    x1, y1, x2, y2 = (np.float64(v) for v in d)
    gx1, gy1, gx2, gy2 = (np.float64(v) for v in g)
    w = min(x2, gx2) - max(x1, gx1)
    h = min(y2, gy2) - max(y1, gy1)
    w = w if w > 0 else np.float64(0)
    h = h if h > 0 else np.float64(0)
    inter = w * h
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / ((x2 - x1) * (y2 - y1) + (gx2 - gx1) * (gy2 - gy1) - inter)


def det_class(value) -> Optional[int]:
    """class id of a detection row's last column (fp32, truncated toward zero); None when outside [0, nc) is decided by the caller"""
    v = np.float32(value)
    return None if np.isnan(v) or np.isinf(v) else int(np.trunc(v))


def confusion_ref(dets, gts, nc, conf_thres=0.25, iou_thres=0.45, events=None):
    """dets: per image [n, 6] fp32 (x1 y1 x2 y2 score class, descending score); gts: per image ([m, 4] fp64, [m] int64).
    -> int64 [nc+1, nc+1], row = predicted, column = true, index nc = background."""
    M = np.zeros((nc + 1, nc + 1), np.int64)
    ev = events if events is not None else {}
    for k in EVENT_KEYS:
        ev.setdefault(k, 0)
    conf = np.float32(conf_thres)
    thr = np.float64(iou_thres)
    for d_img, (g_box, g_lab) in zip(dets, gts):
        d_img = _f32(d_img).reshape(-1, 6)
        g_box = np.asarray(g_box, dtype=np.float64).reshape(-1, 4)
        g_lab = np.asarray(g_lab, dtype=np.int64).reshape(-1)
        g_ok = [0 <= int(l) < nc for l in g_lab]
        # step 1
        kept = []                                          # (detection index, class)
        for i, row in enumerate(d_img):
            ev["exact_conf"] += int(row[4] == conf)
            if not row[4] > conf:
                continue
            c = det_class(row[5])
            if c is None or not 0 <= c < nc:
                continue
            kept.append((i, c))
        # steps 2, 3
        pick = {}                                          # detection index -> (ground-truth index, IoU)
        for i, _ in kept:
            best, m = thr, -1
            for g in range(len(g_lab)):
                if not g_ok[g]:
                    continue
                v = _iou(d_img[i, :4], g_box[g])
                ev["exact_thr"] += int(v == thr)
                if m >= 0 and v == best:
                    ev["tie3"] += 1
                if v > best:
                    best, m = v, g
            if m >= 0:
                pick[i] = (m, best)
        # step 4
        taken = set()
        for g in range(len(g_lab)):
            if not g_ok[g]:
                continue
            win, best = -1, None
            for i, _ in kept:
                if i not in pick or pick[i][0] != g:
                    continue
                if win >= 0 and pick[i][1] == best:
                    ev["tie4"] += 1
                if win < 0 or pick[i][1] > best:
                    win, best = i, pick[i][1]
            if win >= 0:
                taken.add(win)
                c = dict(kept)[win]
                M[c, g_lab[g]] += 1
                ev["matched"] += 1
                ev["offdiag"] += int(c != g_lab[g])
            else:
                M[nc, g_lab[g]] += 1
                ev["missed"] += 1
        # step 5
        for i, c in kept:
            if i not in taken:
                M[c, nc] += 1
                ev["bg_fp"] += 1
                ev["lost"] += int(i in pick)
    return M


class ConfCase(NamedTuple):
    nc: int
    conf: float
    iou: float
    dets: list                 # per image [n, 6] fp32
    gts: list                  # per image ([m, 4] fp64, [m] int64)
    expected: Optional[dict]   # hand cases: {(row, column): count}, every other cell 0


def snap(dets, gts, step=0.25):
    """every coordinate to the nearest multiple of `step` (scores and classes untouched)"""
    out_d, out_g = [], []
    for d, (g, l) in zip(dets, gts):
        d = _f32(d).reshape(-1, 6).copy()
        d[:, :4] = np.round(d[:, :4] / np.float32(step)) * np.float32(step)
        g = np.round(np.asarray(g, dtype=np.float64).reshape(-1, 4) / step) * step
        out_d.append(d); out_g.append((g, np.asarray(l, dtype=np.int64)))
    return out_d, out_g


def on_lattice(case: ConfCase, step=0.25) -> bool:
    """every coordinate a multiple of `step` with magnitude below 2048"""
    for d, (g, _) in zip(case.dets, case.gts):
        for a in (np.asarray(d, dtype=np.float64)[:, :4], np.asarray(g, dtype=np.float64)):
            if a.size and (np.any(a / step != np.round(a / step)) or np.abs(a).max() >= 2048):
                return False
    return True


def _case(nc, conf, iou, det_rows, gt_boxes, gt_labels, expected):
    return ConfCase(nc, conf, iou, [_f32(det_rows).reshape(-1, 6)],
                    [(np.asarray(gt_boxes, dtype=np.float64).reshape(-1, 4), np.asarray(gt_labels, dtype=np.int64))], expected)


def hand_cases():
    """name -> ConfCase, one image each, nc = 3 (index 3 = background)"""
    out = {}
    # A: IoU 1/3 with both ground truths -> the lower index wins, the other is missed
    out["A_equal_iou_lower_gt"] = _case(3, 0.25, 0.3, [[10, 0, 20, 10, 0.9, 2]], [[5, 0, 15, 10], [15, 0, 25, 10]], [0, 1],
                                        {(2, 0): 1, (3, 1): 1})
    # B: two detections on one box -> the lower detection index wins, the loser is a background false positive
    out["B_equal_iou_lower_det"] = _case(3, 0.25, 0.45, [[0, 0, 10, 10, 0.9, 1], [0, 0, 10, 10, 0.8, 2]], [[0, 0, 10, 8]], [0],
                                         {(1, 0): 1, (2, 3): 1})
    # C: IoU exactly 0.45 is no candidate; a score exactly 0.25 is dropped
    out["C_exact_thresholds"] = _case(3, 0.25, 0.45, [[0, 0, 10, 4.5, 0.9, 1], [20, 0, 30, 10, 0.25, 2]],
                                      [[0, 0, 10, 10], [20, 0, 30, 10]], [1, 2], {(1, 3): 1, (3, 1): 1, (3, 2): 1})
    # D: the second detection picks the first ground truth (0.905 against 0.739), loses it and is not re-matched
    out["D_loser_not_rematched"] = _case(3, 0.25, 0.45, [[0, 0, 10, 10, 0.9, 0], [0, 0.5, 10, 10.5, 0.8, 1]],
                                         [[0, 0, 10, 10], [0, 2, 10, 12]], [0, 1], {(0, 0): 1, (1, 3): 1, (3, 1): 1})
    # E: 300 ground truths; exact-fit detections on 0, 255, 256, 299 and a lower-scoring duplicate of each
    g = _grid_boxes(300).astype(np.float64)
    lab = (np.arange(300) % 3).astype(np.int64)
    hit = (0, 255, 256, 299)
    rows = [[*g[k], 0.9 - 0.01 * i, lab[k]] for i, k in enumerate(hit)] + [[*g[k], 0.5 - 0.01 * i, lab[k]] for i, k in enumerate(hit)]
    exp = {}
    for k in hit:
        exp[(int(lab[k]), int(lab[k]))] = exp.get((int(lab[k]), int(lab[k])), 0) + 1
        exp[(int(lab[k]), 3)] = exp.get((int(lab[k]), 3), 0) + 1
    for c in range(3):
        exp[(3, c)] = int((lab == c).sum()) - sum(1 for k in hit if lab[k] == c)
    out["E_300_ground_truths"] = _case(3, 0.25, 0.45, rows, g, lab, exp)
    out["gt_no_det"] = _case(3, 0.25, 0.45, [], [[0, 0, 10, 10], [20, 20, 40, 40]], [0, 2], {(3, 0): 1, (3, 2): 1})
    out["det_no_gt"] = _case(3, 0.25, 0.45, [[0, 0, 10, 10, 0.9, 0], [20, 20, 40, 40, 0.8, 2], [50, 50, 60, 60, 0.1, 1]], [], [],
                             {(0, 3): 1, (2, 3): 1})
    out["neither"] = _case(3, 0.25, 0.45, [], [], [], {})
    # class id nc and label -1 are ignored: the in-range pair next to them is all that is counted
    out["ignored_classes"] = _case(3, 0.25, 0.45, [[0, 0, 10, 10, 0.9, 3], [50, 50, 60, 60, 0.8, 1]],
                                   [[0, 0, 10, 10], [50, 50, 60, 60]], [-1, 1], {(1, 1): 1})
    return out


def expected_matrix(case: ConfCase) -> np.ndarray:
    M = np.zeros((case.nc + 1, case.nc + 1), np.int64)
    for (r, c), v in case.expected.items():
        M[r, c] = v
    return M


RANDOM_SCENES = (("nc1", 1, 31), ("nc5", 5, 32), ("nc80", SWITCH_NC[0], 33), ("nc81", SWITCH_NC[1], 34), ("nc200", 200, 35))


def random_cases():
    """name -> ConfCase of 16 images: val_reference.random_scene snapped to 1/4 pixel at nc = 1, 5, 80, 81, 200, and one scene
    on an 8-pixel lattice at size 160 (genuine IoU ties, zero-area boxes)."""
    out = {}
    for name, nc, seed in RANDOM_SCENES:
        dets, gts = snap(*random_scene(np.random.default_rng(seed), nc, 16))
        out[name] = ConfCase(nc, 0.25, 0.45, dets, gts, None)
    dets, gts = snap(*random_scene(np.random.default_rng(36), 5, 16, size=160), step=8.0)
    out["lattice8"] = ConfCase(5, 0.25, 0.45, dets, gts, None)
    return out


def evaluator_cases(nc=5):
    """val_reference.evaluator_batches snapped to 1/4 pixel, then a batch whose detections are all empty and a batch without
    any ground truth -> list of (dets, gts)"""
    batches, _, _ = evaluator_batches()
    out = [snap(d, g) for d, g in batches]
    d0, g0 = out[0]
    out.append(([np.zeros((0, 6), np.float32) for _ in d0], g0))
    out.append((out[1][0], [(np.zeros((0, 4)), np.zeros(0, np.int64)) for _ in g0]))
    return out


def pack(dets, gts, max_det=None):
    """per-image lists -> (det [B, max_det, 6] fp32, ndet [B] i32, gt [n, 4] f64, labels [n] i64, start [B+1] i32)"""
    B = len(dets)
    max_det = max_det or max([len(d) for d in dets] + [1])
    det = np.zeros((B, max_det, 6), np.float32)
    for b, d in enumerate(dets):
        det[b, :len(d)] = d
    nd = np.asarray([len(d) for d in dets], dtype=np.int32)
    gt = np.concatenate([np.asarray(g, dtype=np.float64).reshape(-1, 4) for g, _ in gts])
    lab = np.concatenate([np.asarray(l, dtype=np.int64).reshape(-1) for _, l in gts])
    start = np.concatenate(([0], np.cumsum([len(l) for _, l in gts]))).astype(np.int32)
    return det, nd, gt, lab, start
