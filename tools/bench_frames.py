"""Video frames as Detector input: what reading frames where they lie buys over the numpy path.  Diagnostic; nothing asserts a time.

1. Detector (rectangular, graphed) in img/s on the SAME 1280 x 720 content given four ways: (a) numpy RGB arrays - ImagePool upload
   + kodhip_letterbox_batch, the path every call took before Frames; (b) `Frame.rgb` of uint8 tensors on the device; (c) NV12
   decoder surfaces on the device with a 256-aligned pitch; (d) host NV12 arrays through `Frame.from_host_yuv` (1.5 B / pixel
   through pinned memory).  Host clock around windows of --calls calls over --images frames each that end in a device synchronise,
   the variants alternated from window to window in this one process, --rounds windows each after a warm-up call.
2. The kernels alone on one chunk of that content, fp32 output on the rectangular canvas: kodhip_letterbox_frames in RGB24 and NV12
   mode against kodhip_letterbox_batch - device events around --reps launches per window after --warm launches, alternated.

usage: python tools/bench_frames.py [--batch 16] [--size 640] [--nc 80] [--rounds 7] [--reps 200] [--warm 20] [--images 128] [--calls 16] [--json PATH]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import bench
from object_detection_cib_amd import _lib; _lib.limit_host_threads()
from object_detection_cib_amd.core.anchors.info import voc_anchor_info
from object_detection_cib_amd.data.device_pipeline import ImagePool
from object_detection_cib_amd.data.frames import Frame, frame_table, matrix_coeffs
from object_detection_cib_amd.engine.rect import rect_canvas
from object_detection_cib_amd.inference import Detector, letterbox_table
from object_detection_cib_amd.lightning.experiments.yv5_baseline.type_defs import LayerwiseAnchorInfo

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16); ap.add_argument("--size", type=int, default=640)
ap.add_argument("--nc", type=int, default=80); ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--warm", type=int, default=20); ap.add_argument("--images", type=int, default=128); ap.add_argument("--calls", type=int, default=16)
ap.add_argument("--json", default=None); ap.add_argument("--conf", type=float, default=0.25); ap.add_argument("--iou", type=float, default=0.45)
a = ap.parse_args()
B, S = a.batch, a.size
H0, W0 = 720, 1280
dev = torch.device("cuda", 0)
ANCH = LayerwiseAnchorInfo(voc_anchor_info(8), voc_anchor_info(16), voc_anchor_info(32))


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


def to_rgb(y, uv):
    """OpenCV's fixed-point NV12 -> RGB (BT.601) in numpy: the image the device conversion stands for"""
    yoff, cy, cvr, cvg, cug, cub = matrix_coeffs("bt601")
    c = np.repeat(np.repeat(uv.reshape(H0 // 2, W0 // 2, 2).astype(np.int32) - 128, 2, axis=0), 2, axis=1)
    l = np.maximum(0, y.astype(np.int32) - yoff) * cy + (1 << 19)
    return np.stack([np.clip(s >> 20, 0, 255) for s in (l + cvr * c[..., 1], l + cvg * c[..., 1] + cug * c[..., 0], l + cub * c[..., 0])],
                    axis=-1).astype(np.uint8)


net, _ = bench.build(a.nc, dev)
x, _ = bench.synth_batch(B, S, a.nc, 1, dev)
for _ in range(2):                                      # a few training-mode forwards so that BN running stats are sane
    net(x.to(dev))
net.eval()
n = a.images // B * B
rng = np.random.default_rng(0)
pitch = (W0 + 255) // 256 * 256
host_nv12 = [rng.integers(0, 256, (H0 * 3 // 2, W0), dtype=np.uint8) for _ in range(n)]
images = [to_rgb(f[:H0], f[H0:]) for f in host_nv12]
rgb_dev = [torch.from_numpy(im).to(dev) for im in images]
surfaces = []
for f in host_nv12:
    buf = torch.zeros(pitch * H0 * 3 // 2, dtype=torch.uint8, device=dev)
    buf.view(H0 * 3 // 2, pitch)[:, :W0] = torch.from_numpy(f).to(dev)
    surfaces.append(buf)
inputs = {"(a) numpy RGB": images,
          "(b) Frame.rgb on the device": [Frame.rgb(t) for t in rgb_dev],
          "(c) NV12 surfaces on the device": [Frame.nv12_surface(s, H0, W0, pitch) for s in surfaces],
          "(d) host NV12, from_host_yuv": [Frame.from_host_yuv(f, "nv12") for f in host_nv12]}
canvas = rect_canvas([(H0, W0)], S)
result = {"batch": B, "size": S, "nc": a.nc, "rounds": a.rounds, "reps": a.reps, "images": n, "calls": a.calls, "source": [H0, W0],
          "canvas": list(canvas), "pitch": pitch}
det = Detector(net, ANCH, image_size=S, batch_size=B, conf_thres=a.conf, iou_thres=a.iou, graphed=True).rectangular()
ref = det(images[:B])
for k, items in inputs.items():                         # the four inputs are one content: same rows out
    got = det(items[:B])
    assert all(torch.equal(g, r) for g, r in zip(got, ref)), k


def call(items, warm):
    calls = 1 if warm else a.calls
    t0 = time.perf_counter()
    for _ in range(calls):
        det(items)
    torch.cuda.synchronize()
    return calls * n / (time.perf_counter() - t0)


rates = alternate(inputs, call)
for k, v in rates.items():
    result[f"detector {k} img_s"] = [round(t, 1) for t in v]
    print(f"B {B} Detector {k:34s}: {med(v)} img/s over {a.rounds} windows of {a.calls} x {n} frames, x "
          f"{np.median(v) / np.median(rates['(a) numpy RGB']):.3f} of (a)", flush=True)

# the kernels alone, one chunk, fp32 output on the canvas
lib, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
Hc, Wc = canvas
pool = ImagePool(images[:B], dev)
vd = letterbox_table([(H0, W0)] * B, S, canvas=canvas)[0]
vd["off"] = pool.offsets
vd_dev = torch.from_numpy(vd.view(np.uint8).copy()).to(dev)
out = torch.empty((B, 3, Hc, Wc), dtype=torch.float32, device=dev)
forms = {"letterbox_batch (pool, 4-byte taps)": lambda: _lib.check(
    lib.kodhip_letterbox_batch(pool.data.data_ptr(), vd_dev.data_ptr(), out.data_ptr(), None, B, Hc, Wc, stream), "letterbox_batch")}
keep = []
for name, frames in (("letterbox_frames RGB24", inputs["(b) Frame.rgb on the device"][:B]), ("letterbox_frames NV12", inputs["(c) NV12 surfaces on the device"][:B])):
    fd_dev = torch.from_numpy(frame_table(frames, S, 0, canvas)[0].view(np.uint8).copy()).to(dev)
    keep.append(fd_dev)
    forms[name] = lambda fd_dev=fd_dev: _lib.check(lib.kodhip_letterbox_frames(fd_dev.data_ptr(), out.data_ptr(), None, B, Hc, Wc, stream),
                                                   "letterbox_frames")
kms = alternate(forms, lambda fn, warm: window_ms(fn, a.warm if warm else a.reps))
for k, v in kms.items():
    result[k + " ms"] = [round(t, 5) for t in v]
    print(f"B {B} {k:40s}: {med(v)} ms per launch ({Hc} x {Wc} canvas, fp32 output)", flush=True)
# bytes per OUTPUT pixel inside the letterboxed frame (360 x 640 of the canvas): 4 taps x (1 Y + 2 UV) = 12 requested, distinct
# source bytes per output pixel = 1.5 B x (720 x 1280) / (360 x 640) = 6; written: 12 (three fp32 planes)
px_out, src = B * Hc * Wc, B * H0 * W0
nv12_ms = float(np.median(kms["letterbox_frames NV12"]))
moved = src * 1.5 + px_out * 12
result["nv12 bytes moved"] = moved
print(f"NV12: {src * 1.5 / px_out:.2f} distinct source bytes read + 12 written per canvas pixel, {moved / 1e6:.1f} MB per launch, "
      f"{moved / nv12_ms / 1e9:.3f} TB/s = {moved / nv12_ms / 1e9 / 6.3:.3f} of the achievable 6.3 TB/s", flush=True)
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    json.dump(result, open(a.json, "w"), indent=1)
