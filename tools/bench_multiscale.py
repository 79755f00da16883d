"""Multi-scale training: what the resize launch and the per-size captured steps cost.  Diagnostic; nothing asserts a time.

1. kodhip_multiscale_batch alone, --batch images of --size px resized to 0.5, 1 and 1.5 of the size from both sources (fp32 NCHW,
   bf16 pixel pairs), and next to kodhip_tta_view on the same fp32 source at --size -> 0.8 x --size, where the two kernels do the
   same work.  Device events around --reps launches per window after --warm launches, the forms alternated from window to window
   in this one process, --rounds windows each.
2. Per size (0.5, 1, 1.5 of --size): MultiScaleTrainStep pinned to that size (`sizes=[sz]`: the resize launch + the replay) against a
   plain GraphedTrainStep captured at that size, in img/s - host clock around windows of --calls steps that end in a device
   synchronise, alternated; the cost of a miss (capture + first replay, host clock); and the device memory the captured size adds
   (torch.cuda.memory_allocated before and after, graph pools included via memory_reserved).

usage: python tools/bench_multiscale.py [--batch 64] [--size 640] [--nc 80] [--widen 0.5] [--rounds 7] [--reps 100] [--warm 10]
                                        [--calls 10] [--no-steps] [--json PATH]"""
import argparse, gc, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import bench
from object_detection_cib_amd import _lib; _lib.limit_host_threads()
from object_detection_cib_amd.engine.graphed import GraphedTrainStep
from object_detection_cib_amd.engine.multiscale import MultiScaleTrainStep, resize_batch

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64); ap.add_argument("--size", type=int, default=640); ap.add_argument("--nc", type=int, default=80)
ap.add_argument("--widen", type=float, default=0.5); ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--reps", type=int, default=100)
ap.add_argument("--warm", type=int, default=10); ap.add_argument("--calls", type=int, default=10); ap.add_argument("--no-steps", action="store_true")
ap.add_argument("--json", default=None)
a = ap.parse_args()
B, S = a.batch, a.size
dev = torch.device("cuda", 0)
lib, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
SIZES = [S // 2 // 32 * 32, S, S * 3 // 2 // 32 * 32]
result = {"batch": B, "size": S, "nc": a.nc, "widen": a.widen, "rounds": a.rounds, "reps": a.reps, "calls": a.calls, "sizes": SIZES}


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
        measure(fn, True)
    for r in range(a.rounds):
        for k in (list(forms) if r % 2 == 0 else list(forms)[::-1]):
            out[k].append(measure(forms[k], False))
    return out


# ---------------------------------------------------------------------------------------------------- 1. the kernel alone
x, targets = bench.synth_batch(B, S, a.nc, 1, dev)
xp = torch.empty((B, S, S // 2, 8), dtype=torch.bfloat16, device=dev)
resize_batch(lib, x, xp, S, S)                                       # the pairs form of the same batch (identity resize)
boxes = torch.zeros((4096, 4), dtype=torch.float64, device=dev)
boxes[:targets.n] = targets.boxes
boxes_out = torch.empty_like(boxes)
forms, keep = {}, []
for sz in SIZES:
    out = torch.empty((B, sz, sz // 2, 8), dtype=torch.bfloat16, device=dev)
    keep.append(out)
    for name, src in (("f32", x), ("pairs", xp)):
        forms[f"multiscale_batch {S} -> {sz} from {name}"] = lambda src=src, out=out, sz=sz: resize_batch(
            lib, src, out, sz, sz, boxes_in=boxes, boxes_out=boxes_out, n=targets.n)
v = int(S * 0.8) // 32 * 32
out_v = torch.empty((B, v, v // 2, 8), dtype=torch.bfloat16, device=dev)
forms[f"multiscale_batch {S} -> {v} from f32 (no boxes)"] = lambda: resize_batch(lib, x, out_v, v, v)
forms[f"tta_view {S} -> {v} from f32"] = lambda: _lib.check(
    lib.kodhip_tta_view(x.data_ptr(), out_v.data_ptr(), None, B, S, S, v, v, v, v, 0, 0.447, stream), "tta_view")
kms = alternate(forms, lambda fn, warm: window_ms(fn, a.warm if warm else a.reps))
for k, t in kms.items():
    result[k + " ms"] = [round(u, 5) for u in t]
    print(f"B {B} {k:52s}: {med(t)} ms per launch", flush=True)
del forms, keep, out_v, xp
torch.cuda.empty_cache()

# ------------------------------------------------------------------------------------------- 2. steps, misses and memory
if not a.no_steps:
    net, loss = bench.build(a.nc, dev, widen=a.widen)
    hyper = ((0.01, 0.01, 0.01), (0.9, 0.9, 0.9), (0.0, 5e-4, 0.0))
    for sz in SIZES:
        gc.collect(); torch.cuda.empty_cache(); torch.cuda.synchronize()
        m0, r0 = torch.cuda.memory_allocated(), torch.cuda.memory_reserved()
        ms = MultiScaleTrainStep(net, loss, B, S, S, sizes=[sz])
        m1 = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        ms(x, targets, *hyper)
        torch.cuda.synchronize()
        miss = time.perf_counter() - t0
        m2, r2 = torch.cuda.memory_allocated(), torch.cuda.memory_reserved()
        xs, ts = bench.synth_batch(B, sz, a.nc, 1, dev)
        plain = GraphedTrainStep(net, loss, B, sz, sz).capture(xs, ts)

        def run(step, batch, warm):
            calls = 2 if warm else a.calls
            t0 = time.perf_counter()
            for _ in range(calls):
                step(*batch, *hyper)
            torch.cuda.synchronize()
            return calls * B / (time.perf_counter() - t0)
        rates = alternate({"wrapper": lambda warm: run(ms, (x, targets), warm), "plain": lambda warm: run(plain, (xs, ts), warm)},
                          lambda fn, warm: fn(warm))
        result[f"size {sz}"] = {"wrapper img_s": [round(u, 1) for u in rates["wrapper"]], "plain img_s": [round(u, 1) for u in rates["plain"]],
                                "miss_s": round(miss, 3), "staging_bytes": m1 - m0, "captured_size_allocated_bytes": m2 - m1,
                                "captured_size_reserved_bytes": r2 - r0}
        print(f"B {B} size {sz}: wrapper {med(rates['wrapper'])} img/s, plain GraphedTrainStep {med(rates['plain'])} img/s "
              f"(x {np.median(rates['wrapper']) / np.median(rates['plain']):.4f}); miss (capture + first replay) {miss:.2f} s; "
              f"the captured size adds {(m2 - m1) / 2**30:.2f} GiB allocated, {(r2 - r0) / 2**30:.2f} GiB reserved (staging {(m1 - m0) / 2**30:.2f} GiB)",
              flush=True)
        torch.cuda.synchronize()
        for st in list(ms.steps.values()) + [plain]:
            st.release()
        del ms, plain, xs, ts
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    json.dump(result, open(a.json, "w"), indent=1)
