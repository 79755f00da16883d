"""Plain numpy restatement of the second-stage crops (csrc/crops.hip, core/crops.py): YOLOv5's save_one_box / apply_classifier
rectangle in np.float32, one rounding per operation; the resize geometry in Python floats (double); the crop itself as
slice -> oracle resize_linear_u8 (cv2.resize INTER_LINEAR of the cutout alone) -> paste on 114 -> / 255, normalise, channel order.
For YUV sources the caller hands in `frames_reference.yuv420_to_rgb`'s image of the whole frame."""
import numpy as np

from oracle.datapath import resize_linear_u8

F = np.float32


def crop_rects(rows, shapes, square=True, gain=1.3, pad=30):
    """rows [N, >= 4] (x1, y1, x2, y2 first), shapes: one (h, w) for all rows or one per row -> (int32 [N, 4] x0, y0, cw, ch,
    bool [N] valid).  An empty crop (cw < 1 or ch < 1, a non-finite coordinate, a NaN edge) has the rectangle (0, 0, 0, 0)."""
    rows = np.asarray(rows, dtype=F).reshape(-1, np.shape(rows)[-1])
    shapes = np.asarray(shapes).reshape(-1, 2)
    if len(shapes) == 1:
        shapes = np.repeat(shapes, len(rows), axis=0)
    rects, valid = np.zeros((len(rows), 4), np.int32), np.zeros(len(rows), bool)
    gain, pad, two = F(gain), F(pad), F(2)
    with np.errstate(all="ignore"):
        for n, (row, (H, W)) in enumerate(zip(rows, shapes)):
            x1, y1, x2, y2 = (F(v) for v in row[:4])
            if not np.isfinite([x1, y1, x2, y2]).all():
                continue
            cx, cy = F(F(x1 + x2) / two), F(F(y1 + y2) / two)            # xyxy2xywh
            w, h = F(x2 - x1), F(y2 - y1)
            if square:
                w = h = max(w, h)
            w, h = F(F(w * gain) + pad), F(F(h * gain) + pad)
            ax, bx = F(cx - F(w / two)), F(cx + F(w / two))              # xywh2xyxy
            ay, by = F(cy - F(h / two)), F(cy + F(h / two))
            if np.isnan([ax, bx, ay, by]).any():
                continue
            ax, bx = (min(max(v, F(0)), F(W)) for v in (ax, bx))         # clip_boxes
            ay, by = (min(max(v, F(0)), F(H)) for v in (ay, by))
            x0, y0 = int(ax), int(ay)
            cw, ch = int(bx) - x0, int(by) - y0
            if cw >= 1 and ch >= 1:
                rects[n], valid[n] = (x0, y0, cw, ch), True
    return rects, valid


def crop_geometry(cw, ch, out_h, out_w, mode="stretch"):
    """(nh, nw, top, left, scale_x, scale_y) of a cw x ch cutout in an out_h x out_w output"""
    cw, ch = int(cw), int(ch)
    nh, nw, top, left = out_h, out_w, 0, 0
    if mode == "letterbox":
        r = min(out_h / float(ch), out_w / float(cw))
        nh, nw = min(max(round(ch * r), 1), out_h), min(max(round(cw * r), 1), out_w)     # round(): half to even
        top, left = (out_h - nh) // 2, (out_w - nw) // 2
    return nh, nw, top, left, 1.0 / (nw / float(cw)), 1.0 / (nh / float(ch))


def crop_ref(img, rect, valid, out_h, out_w, mode="stretch", bgr=False, mean=None, std=None):
    """img: the source as RGB uint8 [H, W, 3] -> (fp32 [3, out_h, out_w], uint8 [out_h, out_w, 3]) of one crop"""
    canvas = np.full((out_h, out_w, 3), 114, dtype=np.uint8)
    if valid:
        x0, y0, cw, ch = (int(v) for v in rect)
        cut = img[y0:y0 + ch, x0:x0 + cw]
        assert cut.shape[:2] == (ch, cw)
        nh, nw, top, left = crop_geometry(cw, ch, out_h, out_w, mode)[:4]
        canvas[top:top + nh, left:left + nw] = resize_linear_u8(cut, nw, nh) if (nh, nw) != (ch, cw) else cut
    if bgr:
        canvas = np.ascontiguousarray(canvas[..., ::-1])
    x = canvas.astype(F) / F(255)
    if mean is not None:
        x = (x - np.asarray(mean, F)) / np.asarray(std, F)
    return np.ascontiguousarray(x.transpose(2, 0, 1)), canvas


def crops_ref(images, rows, frame_index, out_h, out_w, mode="stretch", square=True, gain=1.3, pad=30, bgr=False, mean=None, std=None):
    """every row of `rows` cut out of images[frame_index[n]] -> (rects, valid, fp32 [N, 3, h, w], uint8 [N, h, w, 3])"""
    rects, valid = crop_rects(rows, [images[k].shape[:2] for k in frame_index], square, gain, pad)
    outs = [crop_ref(images[k], r, v, out_h, out_w, mode, bgr, mean, std) for k, r, v in zip(frame_index, rects, valid)]
    return (rects, valid, np.stack([o[0] for o in outs]) if outs else np.zeros((0, 3, out_h, out_w), F),
            np.stack([o[1] for o in outs]) if outs else np.zeros((0, out_h, out_w, 3), np.uint8))
