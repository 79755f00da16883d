"""Rectangular inference: what the minimum-padding canvas buys.  Diagnostic; nothing asserts a time.

1. Detector (upload of original-size u8 images -> letterbox -> graphed eval forward + decode -> best-class NMS -> boxes in image
   pixels) in img/s with rect=False and rect=True on the SAME images, for 4:3 (480 x 640) and 16:9 (720 x 1280) inputs: host
   clock around windows of --calls calls over --images images each that end in a device synchronise, the two detectors
   alternated from window to window in this one process, --rounds windows each after a warm-up call (which captures the graphs).
2. One replay of each detector's captured forward (GraphedEvalForward: eval forward + decode) on its canvas: device events around
   --reps replays per window, alternated.  This is the part the pixel share (0.75 for 4:3, 0.60 for 16:9) is about; the rest of a
   Detector call (the upload of the source images, the NMS) does not shrink with the canvas.
3. kodhip_letterbox_batch (kodhip_val_prep_batch is the same launch with H = W = S) on the square canvas and on the rectangular
   canvas of the same images, fp32 output as the Detector asks for it and the bf16 pair output: device events around --reps
   launches per window, alternated.

usage: python tools/bench_rect.py [--batch 16] [--size 640] [--nc 80] [--rounds 7] [--reps 50] [--images 128] [--calls 16] [--json PATH]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import bench
from object_detection_cib_amd import _lib; _lib.limit_host_threads()
from object_detection_cib_amd.core.anchors.info import voc_anchor_info
from object_detection_cib_amd.data.device_pipeline import ImagePool
from object_detection_cib_amd.engine.rect import rect_canvas
from object_detection_cib_amd.inference import Detector, letterbox_table
from object_detection_cib_amd.lightning.experiments.yv5_baseline.type_defs import LayerwiseAnchorInfo

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16); ap.add_argument("--size", type=int, default=640)
ap.add_argument("--nc", type=int, default=80); ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--images", type=int, default=128); ap.add_argument("--calls", type=int, default=16); ap.add_argument("--json", default=None)
ap.add_argument("--conf", type=float, default=0.25); ap.add_argument("--iou", type=float, default=0.45)
a = ap.parse_args()
B, S = a.batch, a.size
dev = torch.device("cuda", 0)
ANCH = LayerwiseAnchorInfo(voc_anchor_info(8), voc_anchor_info(16), voc_anchor_info(32))
INPUTS = {"4:3": (480, 640), "16:9": (720, 1280)}                     # h x w


def med(v):
    v = np.sort(np.asarray(v, dtype=np.float64))
    return f"{np.median(v):.3f} ({v[0]:.3f} - {v[-1]:.3f})"


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


def kernel_forms(images, canvas):
    """launches of the letterbox kernel over one chunk's records on the two canvases -> {name: callable}; the buffers stay alive in `keep`"""
    lib, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    pool = ImagePool(images, dev)
    shapes = [im.shape[:2] for im in images]
    forms, keep = {}, [pool]
    for name, (H, W), table in (("square", (S, S), letterbox_table(shapes, S)), ("rect", canvas, letterbox_table(shapes, S, canvas=canvas))):
        descs = table[0]
        descs["off"] = pool.offsets
        d_dev = torch.from_numpy(descs.view(np.uint8).copy()).to(dev)
        x = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
        p = torch.empty((B, H, W // 2, 8), dtype=torch.bfloat16, device=dev)
        keep += [d_dev, x, p]
        for out, (xp, pp) in (("f32", (x.data_ptr(), None)), ("pairs", (None, p.data_ptr()))):
            base = (pool.data.data_ptr(), d_dev.data_ptr(), xp, pp, B)
            forms[f"letterbox_batch {name} {H}x{W} {out}"] = lambda base=base, H=H, W=W: _lib.check(      # noqa: E731
                lib.kodhip_letterbox_batch(*base, H, W, stream), "letterbox_batch")
    return forms, keep


net, _ = bench.build(a.nc, dev)
x, _ = bench.synth_batch(B, S, a.nc, 1, dev)
for _ in range(2):                                      # a few training-mode forwards so that BN running stats are sane
    net(x.to(dev))
net.eval()
result = {"batch": B, "size": S, "nc": a.nc, "rounds": a.rounds, "reps": a.reps, "images": a.images, "calls": a.calls, "inputs": {}}
n = a.images // B * B
rng = np.random.default_rng(0)
for tag, (h, w) in INPUTS.items():
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(n)]
    canvas = rect_canvas([(h, w)], S)
    share = canvas[0] * canvas[1] / float(S * S)
    dets = {"rect=False": Detector(net, ANCH, image_size=S, batch_size=B, conf_thres=a.conf, iou_thres=a.iou, graphed=True),
            "rect=True": Detector(net, ANCH, image_size=S, batch_size=B, conf_thres=a.conf, iou_thres=a.iou, graphed=True).rectangular()}

    def call(d, warm):
        calls = 1 if warm else a.calls
        t0 = time.perf_counter()
        for _ in range(calls):
            d(images)
        torch.cuda.synchronize()
        return calls * n / (time.perf_counter() - t0)
    rates = alternate(dets, call)
    entry = {"source": [h, w], "canvas": list(canvas), "pixel_share": share}
    for k, v in rates.items():
        entry[f"detector {k} img_s"] = [round(t, 1) for t in v]
        print(f"{tag} B {B} Detector {k:10s}: {med(v)} img/s over {a.rounds} windows of {a.calls} x {n} images", flush=True)
    print(f"{tag} Detector rect=True / rect=False: x {np.median(rates['rect=True']) / np.median(rates['rect=False']):.3f} "
          f"(canvas {canvas[0]} x {canvas[1]}, pixel share {share:.2f})", flush=True)
    graphs = {"rect=False": dets["rect=False"]._geval[(B, 3, S, S)], "rect=True": dets["rect=True"]._geval[(B, 3, *canvas)]}
    ms = alternate({k: g.graph.replay for k, g in graphs.items()}, lambda fn, warm: window_ms(fn, 3 if warm else a.reps))
    for k, v in ms.items():
        entry[f"replay {k} ms"] = [round(t, 4) for t in v]
        print(f"{tag} B {B} forward + decode replay {k:10s}: {med(v)} ms ({graphs[k].det.shape[1]} rows)", flush=True)
    print(f"{tag} replay rect=True / rect=False: x {np.median(ms['rect=True']) / np.median(ms['rect=False']):.3f}", flush=True)
    forms, keep = kernel_forms(images[:B], canvas)
    kms = alternate(forms, lambda fn, warm: window_ms(fn, 3 if warm else a.reps))
    for k, v in kms.items():
        entry[k + " ms"] = [round(t, 5) for t in v]
        print(f"{tag} B {B} {k:40s}: {med(v)} ms per launch", flush=True)
    result["inputs"][tag] = entry
    del dets, graphs, forms, keep
    torch.cuda.empty_cache()
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    json.dump(result, open(a.json, "w"), indent=1)
