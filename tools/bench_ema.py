"""Cost of the weight EMA (engine/ema.py, csrc/ema.hip) on the flagship workload, one process, alternated windows:
(a) the kodhip_ema_update launch over the network's three arenas and the swap launch, beside the SGD launch on the same
    arenas in the same run: device events around --reps back-to-back calls per window, us per call and GB/s of the bytes each
    moves (update 3 x 4 bytes per element, SGD 5 x 4, swap 4 x 4).  Back to back the arenas stay in the Infinity Cache for
    all of them, as in tools/bench_clip.py: the comparison is between launches under the same conditions;
(b) the replayed step (hipGraph) alone and followed by ModelEMA.update(), ms per step over windows of --steps steps.
Diagnostic; nothing asserts a time.
usage: python tools/bench_ema.py [--variant yv5s] [--nc 80] [--batch 64] [--size 640] [--rounds 7] [--reps 50] [--steps 30] [--no-step]
                                 [--json PATH]"""
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
from object_detection_cib_amd.engine.ema import ModelEMA  # noqa: E402
from object_detection_cib_amd.engine.graphed import GraphedTrainStep  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="yv5s", choices=sorted(bench.VARIANTS))
    ap.add_argument("--nc", type=int, default=80)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--no-step", action="store_true", help="launches only")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    _lib.limit_host_threads()
    dev = torch.device("cuda", 0)
    widen, deepen = bench.VARIANTS[a.variant]
    nc, B, S = a.nc, a.batch, a.size
    x, tg = bench.synth_batch(B, S, nc, 2023, dev)
    hyper = ((0.01, 0.01, 0.01), (0.9, 0.9, 0.9), (0.0, 5e-4, 0.0))
    result = {"variant": a.variant, "nc": nc, "batch": B, "size": S, "rounds": a.rounds, "reps": a.reps, "steps": a.steps}

    # ---- (a) the launches, on the arenas of a network that has run one backward
    net, loss = bench.build(nc, dev, widen=widen, deepen=deepen)
    eng = net.engine()
    from object_detection_cib_amd.core.types import FeatureShape
    net.train_step(x, loss, FeatureShape(width=S, height=S), tg, float(B))
    eng.wait_grads()
    eng.set_hyper(*hyper, 1.0)
    eng.configure_clip(None)
    ema = ModelEMA(net)
    n_p, n_s = eng.n_arena, eng.rm_arena.numel()
    n_ema = n_p + 2 * n_s
    keep = [t.clone() for t in (eng.p_arena, eng.m_arena)]
    legs = {"ema update": (ema.update, 12 * n_ema), "sgd": (eng.sgd_step_device, 20 * n_p),
            "ema swap (twice)": (lambda: (ema._swap(), ema._swap()), 2 * (16 * n_ema + 32 * eng.nbt_arena.numel()))}
    for fn, _ in legs.values():
        for _ in range(5):
            fn()
    res = alternate(legs, a.rounds, lambda leg: timed(leg[0], a.reps))
    print(f"(a) {a.variant} nc {nc}: parameter arena {n_p} floats, statistics 2 x {n_s}; the update moves {12 * n_ema / 1e6:.1f} MB, the SGD "
          f"launch {20 * n_p / 1e6:.1f} MB; us per call over {a.rounds} alternated windows of {a.reps} calls")
    for k, v in res.items():
        med = float(np.median(v))
        result[k + " us"] = [round(u, 2) for u in v]
        print(f"  {k:18s} median {med:7.1f}  min {min(v):7.1f}  max {max(v):7.1f}  | {legs[k][1] / med * 1e-3:6.0f} GB/s of its bytes", flush=True)
    ratio = float(np.median(res["ema update"]) / np.median(res["sgd"]))
    result["update_over_sgd"] = round(ratio, 3)
    print(f"  ema update / sgd = {ratio:.3f} (expected <= 1: the update moves {12 * n_ema / (20 * n_p):.2f} of the SGD launch's bytes)")
    for t, k in zip((eng.p_arena, eng.m_arena), keep):
        t.copy_(k)
    eng.mark_params_changed()

    # ---- (b) the replayed step alone and with the update behind it, one captured program, alternated
    if not a.no_step:
        gs = GraphedTrainStep(net, loss, B, S, S, max_targets=4096).capture(x, tg)
        ema = ModelEMA(net)
        forms = {"step": lambda: gs(x, tg, *hyper, 1.0), "step + ema.update()": lambda: (gs(x, tg, *hyper, 1.0), ema.update())}
        for fn in forms.values():
            for _ in range(5):
                fn()
        res = alternate(forms, a.rounds, lambda fn: timed(fn, a.steps) / 1e3)
        base = float(np.median(res["step"]))
        print(f"(b) replayed {a.variant} B={B} / {S} px step, ms per step over {a.rounds} alternated windows of {a.steps} steps")
        for k, v in res.items():
            med = float(np.median(v))
            result[k + " ms"] = [round(u, 4) for u in v]
            print(f"  {k:20s} median {med:7.3f}  min {min(v):7.3f}  max {max(v):7.3f}  | rate x {base / med:.4f} of the plain step", flush=True)
        result["step_rate_ratio"] = round(base / float(np.median(res["step + ema.update()"])), 4)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(result, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
