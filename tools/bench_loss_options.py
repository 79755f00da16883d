"""Cost of the loss options (focal modulation, label smoothing, objectness pos_weight: the extended instantiations of
loss_rows_kernel / loss_cells_kernel, csrc/loss.hip) on the flagship workload, one process, alternated windows, default
loss against Yolov5Loss(fl_gamma=1.5, fl_alpha=.25, label_smoothing=.1, obj_pos_weight=1) in the same run:
(a) the Yolov5Loss.value_and_grad call on Gaussian head tensors of the step's shapes with a precomputed assignment (the loss
    kernels alone: memsets, mark, rows, cells, scatter, finalize): device events around --reps back-to-back calls per
    window, us per call;
(b) the replayed step (hipGraph), two captured programs over one network, ms per step over windows of --steps steps (both
    run with lr 0: the same launches and bytes, and neither program's updates disturb the other's).
The extended path moves the same bytes through the same launches, so the yardstick is the default call of the same run.
Allowance, written down before the first measurement: the default's own window spread (max - min) plus 30 us per call -
  rows kernel: one lane per assignment row walks its nc class logits serially; per element the extended body adds one powf
    (~100 dependent VALU instructions with its log2 / exp2) and ~25 multiply-adds to the default's ~60: 80 elements x ~125
    instructions x ~5 cycles of dependent issue at 2.4 GHz = ~20 us on the launch's critical path (few blocks, latency-bound);
  cells kernel: the same ~125 instructions once per cell, 1.6 M cells over 1024 x 4 waves = ~6 passes of 64 cells per wave
    beside a P-float strided load and a 64 P-float store per pass: <= 10 us if none of it hides under the memory traffic.
Diagnostic; nothing asserts a time.
usage: python tools/bench_loss_options.py [--variant yv5s] [--nc 80] [--batch 64] [--size 640] [--rounds 7] [--reps 50] [--steps 30]
                                          [--no-step] [--json PATH]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R]
import bench  # noqa: E402
from object_detection_cib_amd import _lib  # noqa: E402
from object_detection_cib_amd.core.types import FeatureShape  # noqa: E402
from object_detection_cib_amd.engine.graphed import GraphedTrainStep  # noqa: E402
from object_detection_cib_amd.lightning.experiments.yv5_baseline.loss import Yolov5Loss  # noqa: E402

OPTIONS = dict(fl_gamma=1.5, fl_alpha=0.25, label_smoothing=0.1, obj_pos_weight=1.0)
ALLOWANCE_US = 30.0


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n          # us per call


def alternate(forms, rounds, measure):
    res = {k: [] for k in forms}
    for r in range(rounds):
        for k in (list(forms) if r % 2 == 0 else list(forms)[::-1]):
            res[k].append(measure(forms[k]))
    return res


def report(res, unit, base_key, result, scale=1.0):
    base = res[base_key]
    spread = max(base) - min(base)
    for k, v in res.items():
        med = float(np.median(v))
        result[f"{k} {unit}"] = [round(u, 4) for u in v]
        print(f"  {k:28s} median {med:9.3f} (min {min(v):9.3f} - max {max(v):9.3f}) {unit}", flush=True)
    return float(np.median(base)), spread


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="yv5s", choices=sorted(bench.VARIANTS))
    ap.add_argument("--nc", type=int, default=80)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--no-step", action="store_true", help="the loss call only")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    _lib.limit_host_threads()
    dev = torch.device("cuda", 0)
    widen, deepen = bench.VARIANTS[a.variant]
    nc, B, S = a.nc, a.batch, a.size
    x, tg = bench.synth_batch(B, S, nc, 2023, dev)
    shape = FeatureShape(width=S, height=S)
    net, loss = bench.build(nc, dev, widen=widen, deepen=deepen)
    focal = Yolov5Loss(loss.assigner, loss.hparams, loss.iou_calculator, None, **OPTIONS)
    result = {"variant": a.variant, "nc": nc, "batch": B, "size": S, "rounds": a.rounds, "reps": a.reps, "steps": a.steps,
              "options": OPTIONS, "allowance_us": ALLOWANCE_US}

    # ---- (a) the loss call on head tensors of the step's shapes
    g = torch.Generator(device=dev).manual_seed(2023)
    raws = [torch.randn(B, 3, S // s, S // s, 5 + nc, generator=g, device=dev) for s in (8, 16, 32)]
    for r in raws:
        r[..., 4] -= 2.0
    asg = loss.assigner.assign_device(shape, tg, dev)
    up = (float(B),) * 3
    forms = {"value_and_grad, default": lambda: loss.value_and_grad(shape, raws, tg, up, assignment=asg),
             "value_and_grad, options": lambda: focal.value_and_grad(shape, raws, tg, up, assignment=asg)}
    for fn in forms.values():
        for _ in range(5):
            fn()
    res = alternate(forms, a.rounds, lambda fn: timed(fn, a.reps))
    print(f"(a) {a.variant} nc {nc} B={B} / {S} px: us per value_and_grad call over {a.rounds} alternated windows of {a.reps} calls")
    base, spread = report(res, "us", "value_and_grad, default", result)
    extra = float(np.median(res["value_and_grad, options"])) - base
    result["call_extra_us"], result["call_spread_us"] = round(extra, 2), round(spread, 2)
    print(f"  options - default = {extra:+.1f} us; allowance {spread:.1f} (default's spread) + {ALLOWANCE_US:.0f} = {spread + ALLOWANCE_US:.1f} us: "
          f"{'inside' if extra <= spread + ALLOWANCE_US else 'OUTSIDE'}")

    # ---- (b) the replayed step with either loss, two captured programs over one network, alternated
    if not a.no_step:
        hyper = ((0.0, 0.0, 0.0), (0.9, 0.9, 0.9), (0.0, 0.0, 0.0))
        gd = GraphedTrainStep(net, loss, B, S, S, max_targets=4096).capture(x, tg)
        gf = GraphedTrainStep(net, focal, B, S, S, max_targets=4096).capture(x, tg)
        forms = {"step, default": lambda: gd(x, tg, *hyper, 1.0), "step, options": lambda: gf(x, tg, *hyper, 1.0)}
        for fn in forms.values():
            for _ in range(5):
                fn()
        res = alternate(forms, a.rounds, lambda fn: timed(fn, a.steps) / 1e3)
        print(f"(b) replayed {a.variant} B={B} / {S} px step, ms per step over {a.rounds} alternated windows of {a.steps} steps")
        base, spread = report(res, "ms", "step, default", result)
        extra = (float(np.median(res["step, options"])) - base) * 1e3
        result["step_extra_us"], result["step_spread_us"] = round(extra, 2), round(spread * 1e3, 2)
        result["step_rate_ratio"] = round(base / float(np.median(res["step, options"])), 4)
        print(f"  options - default = {extra:+.1f} us per step (rate x {result['step_rate_ratio']:.4f}); allowance {spread * 1e3:.1f} "
              f"(default's spread) + {ALLOWANCE_US:.0f} = {spread * 1e3 + ALLOWANCE_US:.1f} us: "
              f"{'inside' if extra <= spread * 1e3 + ALLOWANCE_US else 'OUTSIDE'}")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(result, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
