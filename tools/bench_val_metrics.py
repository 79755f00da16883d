"""One validation epoch's batches through the two metric consumers.  Diagnostic; nothing asserts a time.

DeviceDetectionMetrics (csrc/val_metrics.hip: add_batch per batch + compute once) beside DeviceMAPEvaluator (csrc/map_match.hip:
add_batch with its host hand-off per batch + get_report) on the SAME batches: --images images in batches of --batch, the NMS
output as it lies on the device (PackedDetections [B, 300, 6] with device-side counts) and BatchedTargets.  The epoch is
synthetic: 2 - 15 ground truths per image, jittered detections of them and false positives up to 300 rows per image (what
validation at conf_thres 0.001 hands over), --distinct different batches cycled.  A host clock around the whole epoch, ending
in the consumer's read-back (compute() / get_report() return host values: the device has finished); the two consumers
alternated, --rounds epochs each after a warm-up epoch; median (min - max).

usage: python tools/bench_val_metrics.py [--images 5000] [--batch 64] [--nc 80] [--rounds 5] [--distinct 8] [--json PATH]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from object_detection_cib_amd import _lib; _lib.limit_host_threads()
from object_detection_cib_amd.core.label_assignment.yv5 import BatchedTargets
from object_detection_cib_amd.core.nms import PackedDetections
from object_detection_cib_amd.data.detection import DetectionTarget
from object_detection_cib_amd.lightning.callbacks.map_eval import DeviceMAPEvaluator
from object_detection_cib_amd.lightning.callbacks.val_metrics import DeviceDetectionMetrics

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=5000); ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--nc", type=int, default=80); ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--distinct", type=int, default=8); ap.add_argument("--json", default=None)
a = ap.parse_args()
dev = torch.device("cuda", 0)
MAX_DET = 300


def make_batch(rng, B, nc, size=640):
    packed = np.zeros((B, MAX_DET, 6), np.float32)
    counts = np.zeros(B, np.int32)
    targets = []
    for b in range(B):
        n = int(rng.integers(2, 16))
        c = rng.uniform(40, size - 40, (n, 2)); wh = rng.uniform(16, 240, (n, 2))
        gt = np.concatenate((c - wh / 2, c + wh / 2), 1)
        lab = rng.integers(0, nc, n)
        rows = []
        for box, l in zip(gt, lab):
            for _ in range(int(rng.integers(0, 4))):
                rows.append([*(box + rng.normal(0, 0.04, 4) * np.tile(box[2:] - box[:2], 2)), rng.uniform(0.05, 1.0),
                             l if rng.random() < 0.85 else rng.integers(0, nc)])
        k = MAX_DET - len(rows) if rng.random() < 0.8 else int(rng.integers(0, MAX_DET - len(rows)))
        c2 = rng.uniform(0, size, (k, 2)); wh2 = rng.uniform(8, 160, (k, 2))
        fp = np.concatenate((c2 - wh2 / 2, c2 + wh2 / 2, rng.uniform(0.001, 0.5, (k, 1)), rng.integers(0, nc, (k, 1))), 1)
        d = np.concatenate((np.asarray(rows, np.float64).reshape(-1, 6), fp)).astype(np.float32)
        d = d[np.argsort(-d[:, 4], kind="mergesort")][:MAX_DET]
        packed[b, :len(d)] = d; counts[b] = len(d)
        targets.append(DetectionTarget(torch.from_numpy(gt), torch.from_numpy(lab.astype(np.int64))))
    p = torch.from_numpy(packed).to(dev)
    dets = PackedDetections([p[b, :int(n)] for b, n in enumerate(counts)], p, torch.from_numpy(counts).to(dev))
    return BatchedTargets.from_targets(tuple(targets), dev), dets, int(counts.sum())


rng = np.random.default_rng(7)
distinct = [make_batch(rng, a.batch, a.nc) for _ in range(a.distinct)]
n_batches = -(-a.images // a.batch)
epoch = [distinct[i % a.distinct] for i in range(n_batches)]
records = sum(e[2] for e in epoch)


def run_metrics():
    vm = DeviceDetectionMetrics(a.nc)
    t0 = time.perf_counter()
    for tg, dets, _ in epoch:
        vm.add_batch(tg, dets)
    t1 = time.perf_counter()                         # enqueue only: add_batch never waits
    res = vm.compute()
    t2 = time.perf_counter()
    return {"total_ms": 1e3 * (t2 - t0), "enqueue_ms": 1e3 * (t1 - t0), "value": res["map"], "n": int(res["n_p"].sum())}


def run_map():
    ev = DeviceMAPEvaluator(a.nc)
    t0 = time.perf_counter()
    for tg, dets, _ in epoch:
        ev.add_batch(tg, dets)
    t1 = time.perf_counter()
    rep = ev.get_report()
    t2 = time.perf_counter()
    return {"total_ms": 1e3 * (t2 - t0), "enqueue_ms": 1e3 * (t1 - t0), "value": rep["map"], "n": records}


def med(v):
    v = np.sort(np.asarray(v, dtype=np.float64))
    return f"{np.median(v):.1f} ({v[0]:.1f} - {v[-1]:.1f})"


forms = {"DeviceDetectionMetrics add_batch + compute": run_metrics, "DeviceMAPEvaluator add_batch + get_report": run_map}
for fn in forms.values():
    fn(); torch.cuda.synchronize()
out = {k: [] for k in forms}
for _ in range(a.rounds):
    for k, fn in forms.items():
        torch.cuda.synchronize()
        out[k].append(fn())
print(f"{n_batches} batches of {a.batch} images x {MAX_DET} rows, nc {a.nc}: {records} detections per epoch")
summary = {"batches": n_batches, "batch": a.batch, "nc": a.nc, "records": records, "forms": {}}
for k, runs in out.items():
    tot, enq = [r["total_ms"] for r in runs], [r["enqueue_ms"] for r in runs]
    print(f"{k:46s} epoch {med(tot)} ms = {np.median(tot) / n_batches:.3f} ms per batch; of it the add_batch loop {med(enq)} ms; "
          f"records {runs[0]['n']}, value {runs[0]['value']:.6f}")
    summary["forms"][k] = {"epoch_ms": tot, "add_batch_loop_ms": enq, "records": runs[0]["n"], "value": runs[0]["value"]}
if a.json:
    json.dump(summary, open(a.json, "w"), indent=1)
