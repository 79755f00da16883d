"""Second-stage crops: what cutting and resizing detections on the device costs.  Diagnostic; nothing asserts a time.

1. The kernels alone: kodhip_crop_plan + kodhip_crop_batch for --frames 1280 x 720 frames with --boxes boxes each (16 x 20 = 320
   crops of 224 x 224, fp32 output, apply_classifier's options) against kodhip_letterbox_frames producing the same number of fp32
   output pixels in the same run: one record per crop, a view of the frame at the rectangle the plan chose (fetched once, before
   the timing), stretched to 224 x 224 - the same taps and the same bytes written, but with the rectangles known on the host.
   Device events around --reps launches per window after --warm launches, the two alternated, for RGB24 frames and for NV12
   surfaces (NV12 views start and end on even pixels, so there the letterbox reads rectangles rounded outward to even).
   ALLOWANCE, written before the first run: plan + crop may take the letterbox launch's time per output pixel, plus that
   launch's own window spread (max - min), plus 25 % - for the per-crop record and source reads scattered over many small
   regions; nobody had measured that 25 %.  The tool reports the figure and which side of the allowance it lands on.
2. End to end: `Detector.detect_crops` against `Detector.__call__` (rectangular, graphed) on the same --images frames, host clock
   around windows of --calls calls that end in a device synchronise, alternated; the added time per call.  No gate.

usage: python tools/bench_crops.py [--frames 16] [--boxes 20] [--crop 224] [--rounds 7] [--reps 50] [--warm 5] [--images 128] [--calls 4]
       [--rows 20] [--skip-kernels] [--skip-detector] [--json PATH]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import bench
from object_detection_cib_amd import _lib; _lib.limit_host_threads()
from object_detection_cib_amd.core.anchors.info import voc_anchor_info
from object_detection_cib_amd.core.crops import CROP_DESC, CropOptions
from object_detection_cib_amd.data.frames import FRAME_DESC, Frame, frame_records
from object_detection_cib_amd.inference import Detector
from object_detection_cib_amd.lightning.experiments.yv5_baseline.type_defs import LayerwiseAnchorInfo

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=16); ap.add_argument("--boxes", type=int, default=20); ap.add_argument("--crop", type=int, default=224)
ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--reps", type=int, default=50); ap.add_argument("--warm", type=int, default=5)
ap.add_argument("--images", type=int, default=128); ap.add_argument("--calls", type=int, default=4); ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--size", type=int, default=640); ap.add_argument("--nc", type=int, default=80); ap.add_argument("--rows", type=int, default=20)
ap.add_argument("--json", default=None); ap.add_argument("--skip-detector", action="store_true"); ap.add_argument("--skip-kernels", action="store_true")
a = ap.parse_args()
ALLOWANCE_EXTRA = 0.25                                  # (see the text above: fixed before the first run)
H0, W0, C = 720, 1280, a.crop
dev = torch.device("cuda", 0)
lib, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
assert lib.kodhip_crop_desc_bytes() == CROP_DESC.itemsize and lib.kodhip_frame_desc_bytes() == FRAME_DESC.itemsize


def med(v):
    v = np.sort(np.asarray(v, dtype=np.float64))
    return f"{np.median(v):.4f} ({v[0]:.4f} - {v[-1]:.4f})"


def window_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(forms, measure):
    """{name: callable} -> {name: [one figure per round]}, the forms alternated from round to round after a warm-up each"""
    out = {k: [] for k in forms}
    for fn in forms.values():
        measure(fn, warm=True)
    for r in range(a.rounds):
        for k in (list(forms) if r % 2 == 0 else list(forms)[::-1]):
            out[k].append(measure(forms[k], warm=False))
    return out


def upload(arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).to(dev)


rng = np.random.default_rng(0)
F, N = a.frames, a.frames * a.boxes
pitch = (W0 + 255) // 256 * 256
rgb = [torch.from_numpy(rng.integers(0, 256, (H0, W0, 3), dtype=np.uint8)).to(dev) for _ in range(F)]
nv12 = [torch.from_numpy(rng.integers(0, 256, pitch * H0 * 3 // 2, dtype=np.uint8)).to(dev) for _ in range(F)]
# boxes 60 - 360 pixels wide and high anywhere in the frame: squared, * 1.3 + 30, clipped, they become 108 - 498 pixel cutouts
wh = rng.uniform(60, 360, (N, 2))
cxy = rng.uniform(0, 1, (N, 2)) * (W0, H0)
rows = torch.from_numpy(np.float32(np.concatenate((cxy - wh / 2, cxy + wh / 2, np.full((N, 1), 0.5), np.zeros((N, 1))), axis=1))).to(dev)
row_index, frame_index = upload(np.arange(N, dtype=np.int32)), upload(np.repeat(np.arange(F, dtype=np.int32), a.boxes))
opts = CropOptions((C, C))
recs = torch.empty(N * CROP_DESC.itemsize, dtype=torch.uint8, device=dev)
rects = torch.empty((N, 4), dtype=torch.int32, device=dev)
out = torch.empty((N, 3, C, C), dtype=torch.float32, device=dev)
result = {"frames": F, "boxes": a.boxes, "crop": C, "rounds": a.rounds, "reps": a.reps, "source": [H0, W0], "output_pixels": N * C * C,
          "allowance_extra": ALLOWANCE_EXTRA}


def kernels(tag, frames, even):
    f_dev = upload(frame_records(frames))

    def plan_crop():
        _lib.check(lib.kodhip_crop_plan(f_dev.data_ptr(), F, rows.data_ptr(), 6, row_index.data_ptr(), frame_index.data_ptr(), N, C, C,
                                        opts.mode, int(opts.square), opts.gain, opts.pad, recs.data_ptr(), rects.data_ptr(), stream), "crop_plan")
        _lib.check(lib.kodhip_crop_batch(f_dev.data_ptr(), F, recs.data_ptr(), N, out.data_ptr(), None, C, C, 0, None, stream), "crop_batch")

    def crop_only():
        _lib.check(lib.kodhip_crop_batch(f_dev.data_ptr(), F, recs.data_ptr(), N, out.data_ptr(), None, C, C, 0, None, stream), "crop_batch")
    plan_crop()
    r = rects.cpu().numpy()
    assert (r[:, 2] > 0).all()
    got = out.clone()
    # the same rectangles as letterbox records: a view of the frame per crop, stretched to C x C
    views = []
    for (x0, y0, cw, ch), k in zip(r.tolist(), np.repeat(np.arange(F), a.boxes)):
        if even:
            x1, y1 = min(W0, (x0 + cw + 1) & ~1), min(H0, (y0 + ch + 1) & ~1)
            x0, y0 = x0 & ~1, y0 & ~1
            buf = nv12[k]
            yy = buf.as_strided((y1 - y0, x1 - x0), (pitch, 1), y0 * pitch + x0)
            uv = buf.as_strided(((y1 - y0) // 2, x1 - x0), (pitch, 1), pitch * H0 + (y0 // 2) * pitch + x0)
            views.append(Frame.nv12(yy, uv))
        else:
            views.append(Frame.rgb(rgb[k][y0:y0 + ch, x0:x0 + cw]))
    vd = frame_records(views)
    for d, f in zip(vd, views):
        d["nh"], d["nw"], d["top"], d["left"] = C, C, 0, 0
        d["scale_x"], d["scale_y"] = 1.0 / (C / float(f.w)), 1.0 / (C / float(f.h))
    v_dev = upload(vd)

    def letterbox():
        _lib.check(lib.kodhip_letterbox_frames(v_dev.data_ptr(), out.data_ptr(), None, N, C, C, stream), "letterbox_frames")
    letterbox()
    same = bool(torch.equal(out, got))
    assert same or even, "RGB24: the letterbox of the rectangles' views must give the crops bit for bit"
    forms = {f"{tag} crop_plan + crop_batch": plan_crop, f"{tag} crop_batch alone": crop_only, f"{tag} letterbox_frames on the same rectangles": letterbox}
    ms = alternate(forms, lambda fn, warm: window_ms(fn, a.warm if warm else a.reps))
    for k, v in ms.items():
        result[k + " ms"] = [round(t, 5) for t in v]
        print(f"{k:58s}: {med(v)} ms per launch, {np.median(v) * 1e6 / (N * C * C):.4f} ns per output pixel", flush=True)
    lb, pc = np.asarray(ms[f"{tag} letterbox_frames on the same rectangles"]), np.asarray(ms[f"{tag} crop_plan + crop_batch"])
    allowance = float(np.median(lb) * (1 + ALLOWANCE_EXTRA) + (lb.max() - lb.min()))
    verdict = "inside" if np.median(pc) <= allowance else "OUTSIDE"
    result[f"{tag} allowance ms"], result[f"{tag} verdict"], result[f"{tag} bit equal to letterbox"] = round(allowance, 5), verdict, same
    cut = float((r[:, 2] * r[:, 3]).sum())
    print(f"{tag}: {N} crops of {C} x {C} from cutouts of {r[:, 2].min()} - {r[:, 2].max()} x {r[:, 3].min()} - {r[:, 3].max()} pixels "
          f"({cut / 1e6:.1f} M source pixels, {N * C * C / 1e6:.1f} M output pixels); plan + crop {np.median(pc):.4f} ms = x "
          f"{np.median(pc) / np.median(lb):.3f} of the letterbox launch; allowance {allowance:.4f} ms (median x 1.25 + spread "
          f"{lb.max() - lb.min():.4f}): {verdict}; bit-equal outputs: {same}", flush=True)


if not a.skip_kernels:
    kernels("RGB24", [Frame.rgb(t) for t in rgb], even=False)
    kernels("NV12", [Frame.nv12_surface(b, H0, W0, pitch) for b in nv12], even=True)

if not a.skip_detector:
    B, S = a.batch, a.size
    ANCH = LayerwiseAnchorInfo(voc_anchor_info(8), voc_anchor_info(16), voc_anchor_info(32))
    net, _ = bench.build(a.nc, dev)
    with torch.no_grad():                                   # a fresh network scores nothing above 0.001: head biases that give rows
        for name, p in net.named_parameters():              # (objectness 0.73 x class 0.5, boxes 0.29 of an anchor wide)
            if name.endswith("obj_head.conv.bias"):
                p.fill_(1.0)
            elif name.endswith("cls_head.conv.bias"):
                p.zero_()
            elif name.endswith("box_head.conv.bias"):
                p.copy_(torch.tensor([0.0, 0.0, -1.0, -1.0], device=p.device).repeat(p.numel() // 4))
    x, _ = bench.synth_batch(B, S, a.nc, 1, dev)
    for _ in range(2):                                      # a few training-mode forwards so that BN running stats are sane
        net(x.to(dev))
    net.eval()
    n = a.images // B * B
    images = [rng.integers(0, 256, (H0, W0, 3), dtype=np.uint8) for _ in range(n)]
    # a threshold that leaves about --rows rows per image in the first chunk
    probe = Detector(net, ANCH, image_size=S, batch_size=B, conf_thres=0.001, graphed=True).rectangular()(images[:B])
    scores = np.sort(np.concatenate([p[:, 4].cpu().numpy() for p in probe]))[::-1]
    conf = float(scores[min(len(scores) - 1, a.rows * B)]) if len(scores) else 0.25
    det = Detector(net, ANCH, image_size=S, batch_size=B, conf_thres=conf, graphed=True).rectangular()
    ref = det(images)
    got = det.detect_crops(images, size=(C, C))
    assert all(torch.equal(g, r) for g, r in zip(got, ref))
    total = sum(len(r) for r in ref)
    del got

    def call(fn, warm):
        calls = 1 if warm else a.calls
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / calls * 1e3

    ms = alternate({"Detector.__call__": lambda: det(images), "Detector.detect_crops": lambda: det.detect_crops(images, size=(C, C))}, call)
    for k, v in ms.items():
        result[k + " ms"] = [round(t, 3) for t in v]
        print(f"{k:24s}: {med(v)} ms per call of {n} frames", flush=True)
    added = float(np.median(ms["Detector.detect_crops"]) - np.median(ms["Detector.__call__"]))
    result["detector rows per call"], result["detector conf"], result["detector added ms per call"] = total, conf, round(added, 3)
    print(f"detect_crops adds {added:.3f} ms per call of {n} frames ({total} rows, {total / n:.1f} per frame, conf {conf:.4g}; "
          f"{total * C * C * 12 / 1e6:.0f} MB of fp32 crops per call)", flush=True)
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    json.dump(result, open(a.json, "w"), indent=1)
