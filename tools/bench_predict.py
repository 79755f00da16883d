"""Inference post-process and Detector throughput.  Diagnostic; nothing asserts a time.

1. kodhip_nms (multi-label: rows * nc sort keys per image) against kodhip_nms_ex with best_class = 1 (rows keys per image) on the
   SAME decoded detections of a random-init yv5s at conf_thres = 0.001 - the many-candidates worst case - for each --nc.  Device
   events around --reps calls per window, the two forms alternated from window to window in this one process, --rounds windows
   each after a warm-up window; median (min - max) in ms per call.
2. Detector (upload of original-size u8 images -> letterbox -> graphed eval forward + decode -> best-class NMS -> boxes in image
   pixels) in img/s beside the validation loop's `make_batch` + `validation_step` (pool resident in HBM, multi-label NMS) on the
   same images, same batch size, host clock around windows that end in a device synchronise.

--augment runs only this instead: AugmentedDetector - test-time augmentation, three views per batch in one hipGraph
(GraphedAugmentedForward) and one NMS over the merged rows - beside the plain Detector on the same images in the same window
scheme, and the time of one replay of the augmented graph beside one replay of the plain GraphedEvalForward (device events
around --reps replays per window, alternated).

usage: python tools/bench_predict.py [--batch 16] [--size 640] [--nc 10,80] [--rounds 7] [--reps 20] [--images 256] [--json PATH]
                                     [--augment]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from oracle import synth
import bench
from object_detection_cib_amd import _lib; _lib.limit_host_threads()
from object_detection_cib_amd.core.anchors.info import voc_anchor_info
from object_detection_cib_amd.core.types import FeatureShape
from object_detection_cib_amd.data.device_pipeline import DeviceValPipeline
from object_detection_cib_amd.inference import AugmentedDetector, Detector
from object_detection_cib_amd.lightning.experiments.yv5_baseline.exp import DefaultYolov5Experiment
from object_detection_cib_amd.lightning.experiments.yv5_baseline.layers import get_detections
from object_detection_cib_amd.lightning.experiments.yv5_baseline.type_defs import LayerwiseAnchorInfo

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16); ap.add_argument("--size", type=int, default=640)
ap.add_argument("--nc", default="10,80"); ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--images", type=int, default=256); ap.add_argument("--json", default=None)
ap.add_argument("--conf", type=float, default=0.001); ap.add_argument("--iou", type=float, default=0.6)
ap.add_argument("--augment", action="store_true")
a = ap.parse_args()
B, S = a.batch, a.size
dev = torch.device("cuda", 0)
ANCH = LayerwiseAnchorInfo(voc_anchor_info(8), voc_anchor_info(16), voc_anchor_info(32))
MAX_WH, MAX_DET, MAX_NMS = 4096.0, 300, 30000


def cap_for(n):
    cap = 64
    while cap < n:
        cap <<= 1
    return cap


def med(v):
    v = np.sort(np.asarray(v, dtype=np.float64))
    return f"{np.median(v):.3f} ({v[0]:.3f} - {v[-1]:.3f})"


def nms_forms(det):
    """the two launch sequences on one detections tensor -> {name: (callable, key_cap, ncand, nout)}"""
    Bd, rows, P = det.shape
    nc = P - 5
    lib, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    forms = {}
    for name, cap, best in (("multi_label", cap_for(rows * nc), 0), ("best_class", cap_for(rows), 1)):
        keys = torch.empty(Bd * cap, dtype=torch.int64, device=dev)
        ncand = torch.empty(Bd, dtype=torch.int32, device=dev); nout = torch.empty(Bd, dtype=torch.int32, device=dev)
        out = torch.empty((Bd, MAX_DET, 6), dtype=torch.float32, device=dev)
        base = (det.data_ptr(), keys.data_ptr(), cap, ncand.data_ptr(), out.data_ptr(), nout.data_ptr(), Bd, rows, nc, a.conf, a.iou,
                MAX_DET, MAX_NMS, MAX_WH)
        if best:
            fn = lambda base=base: _lib.check(lib.kodhip_nms_ex(*base, 1, None, None, stream), "nms_ex")      # noqa: E731
        else:
            fn = lambda base=base: _lib.check(lib.kodhip_nms(*base, stream), "nms")                           # noqa: E731
        forms[name] = (fn, cap, ncand, nout, keys)
    return forms


def augment_entry(net, nc):
    """Detector with and without test-time augmentation on the same images, and one graph replay of each forward"""
    cache = synth.coco_zipf_like(a.images, 500, 3, nc)
    images = [c[0] for c in cache]
    n = len(images) // B * B
    dets = {"detector_plain": Detector(net, ANCH, image_size=S, batch_size=B, conf_thres=a.conf, iou_thres=a.iou, graphed=True),
            "detector_augment": AugmentedDetector(net, ANCH, image_size=S, batch_size=B, conf_thres=a.conf, iou_thres=a.iou, graphed=True)}
    rates = {k: [] for k in dets}
    for d in dets.values():
        d(images[:n]); torch.cuda.synchronize()
    for r in range(a.rounds):
        for k in (list(dets) if r % 2 == 0 else list(dets)[::-1]):
            t0 = time.perf_counter(); dets[k](images[:n]); torch.cuda.synchronize()
            rates[k].append(n / (time.perf_counter() - t0))
    entry = {}
    for k, v in rates.items():
        entry[k + "_img_s"] = [round(t, 1) for t in v]
        print(f"nc {nc} B {B} {k:17s}: {med(v)} img/s over {a.rounds} windows of {n} images", flush=True)
    graphs = {k: d._geval[(B, 3, S, S)] for k, d in dets.items()}
    entry["merged_rows"] = int(graphs["detector_augment"].det.shape[1]); entry["rows"] = int(graphs["detector_plain"].det.shape[1])
    ms = {k: [] for k in graphs}
    for g in graphs.values():
        window_ms(g.graph.replay, 3)
    for r in range(a.rounds):
        for k in (list(graphs) if r % 2 == 0 else list(graphs)[::-1]):
            ms[k].append(window_ms(graphs[k].graph.replay, a.reps))
    for k, v in ms.items():
        entry[k.replace("detector", "replay") + "_ms"] = [round(t, 4) for t in v]
        print(f"nc {nc} B {B} {k.replace('detector', 'replay'):17s}: {med(v)} ms per graph replay ({entry['merged_rows' if 'augment' in k else 'rows']} rows)", flush=True)
    print(f"nc {nc} B {B} augmented / plain replay: x {np.median(ms['detector_augment']) / np.median(ms['detector_plain']):.2f}", flush=True)
    return entry


def window_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / reps


result = {"batch": B, "size": S, "conf_thres": a.conf, "iou_thres": a.iou, "rounds": a.rounds, "reps": a.reps, "nc": {}}
for nc in [int(v) for v in a.nc.split(",")]:
    net, loss = bench.build(nc, dev)
    x, _ = bench.synth_batch(B, S, nc, 1, dev)
    x = x.to(dev)
    for _ in range(2):                                  # a few training-mode forwards so that BN running stats are sane
        net(x)
    net.eval()
    if a.augment:
        result["nc"][str(nc)] = augment_entry(net, nc)
        del net
        torch.cuda.empty_cache()
        continue
    with torch.no_grad():
        det = get_detections(FeatureShape(width=S, height=S), net(x), ANCH).contiguous()
    forms = nms_forms(det)
    times = {k: [] for k in forms}
    for fn, *_ in forms.values():
        window_ms(fn, 3)
    order = list(forms)
    for r in range(a.rounds):
        for name in (order if r % 2 == 0 else order[::-1]):
            times[name].append(window_ms(forms[name][0], a.reps))
    rows = det.shape[1]
    entry = {"rows": rows}
    for name, (fn, cap, ncand, nout, keys) in forms.items():
        entry[name] = {"key_cap": cap, "workspace_MB": B * cap * 8 / 1e6, "candidates_mean": float(ncand.float().mean()),
                       "kept_mean": float(nout.float().mean()), "ms": [round(t, 4) for t in times[name]]}
        print(f"nc {nc} B {B} rows {rows} {name:11s}: key_cap {cap:8d} ({B * cap * 8 / 1e6:7.1f} MB) candidates/img {entry[name]['candidates_mean']:9.0f} "
              f"kept/img {entry[name]['kept_mean']:5.0f}  {med(times[name])} ms/call", flush=True)
    del forms
    # end to end on original-size images
    cache = synth.coco_zipf_like(a.images, 500, 3, nc)
    images = [c[0] for c in cache]
    n = len(images) // B * B
    detector = Detector(net, ANCH, image_size=S, batch_size=B, conf_thres=a.conf, iou_thres=a.iou, graphed=True)
    multi = Detector(net, ANCH, image_size=S, batch_size=B, conf_thres=a.conf, iou_thres=a.iou, multi_label=True, graphed=True)
    pipe = DeviceValPipeline(images, [c[1] for c in cache], [c[2] for c in cache], S, dev)
    exp = DefaultYolov5Experiment(net, loss, ANCH, val_nms_conf_threshold=a.conf, val_nms_iou_threshold=a.iou, graphed=True)

    def val_loop():
        for i in range(0, n, B):
            img, _, t = pipe.make_batch(list(range(i, i + B)))
            exp.validation_step((img, t, None))
    loops = {"detector_best_class": lambda: detector(images[:n]), "detector_multi_label": lambda: multi(images[:n]), "validation_step": val_loop}
    rates = {k: [] for k in loops}
    for k, fn in loops.items():
        fn(); torch.cuda.synchronize()
    for r in range(a.rounds):
        for k in (list(loops) if r % 2 == 0 else list(loops)[::-1]):
            t0 = time.perf_counter(); loops[k](); torch.cuda.synchronize()
            rates[k].append(n / (time.perf_counter() - t0))
    for k, v in rates.items():
        entry[k + "_img_s"] = [round(t, 1) for t in v]
        print(f"nc {nc} B {B} {k:21s}: {med(v)} img/s over {a.rounds} windows of {n} images", flush=True)
    result["nc"][str(nc)] = entry
    del net, detector, multi, exp, pipe
    torch.cuda.empty_cache()
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    json.dump(result, open(a.json, "w"), indent=1)
