"""Cost of gradient accumulation (engine/accumulate.py, csrc/accumulate.hip) on the flagship workload, one process, alternated
windows:
(a) the kodhip_grad_accumulate launch (mode 2, the form a captured step holds; flag 0 = add, flag 1 = copy) over the gradient
    arena, beside the SGD launch on the same arenas in the same run: device events around --reps back-to-back calls per window,
    us per call and GB/s of the bytes each moves (accumulate add 3 x 4 bytes per element, copy 2 x 4, SGD 5 x 4).  Back to back
    the arenas stay in the Infinity Cache for all of them, as in tools/bench_ema.py: the comparison is between launches under the
    same conditions;
(b) the replayed plain step (hipGraph, update inside) and GraphedTrainStep(accumulate_grad_batches=N) - accumulate launch inside,
    update behind every N-th replay - ms per micro-batch and images/s over windows of --steps micro-batches.  The micro-step's
    graph trades the update launch for the accumulate launch, so the allowance over the plain step's own min - max spread is
    the measured time of the per-window update divided by N.
Diagnostic; nothing asserts a time.
usage: python tools/bench_accumulate.py [--variant yv5s] [--nc 80] [--batch 64] [--size 640] [--accumulate 4] [--rounds 7] [--reps 50]
                                        [--steps 32] [--no-step] [--json PATH]"""
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
    ap.add_argument("--accumulate", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--no-step", action="store_true", help="launches only")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    _lib.limit_host_threads()
    dev = torch.device("cuda", 0)
    widen, deepen = bench.VARIANTS[a.variant]
    nc, B, S, N = a.nc, a.batch, a.size, a.accumulate
    steps = max(a.steps // N, 1) * N              # whole windows
    x, tg = bench.synth_batch(B, S, nc, 2023, dev)
    hyper = ((0.01, 0.01, 0.01), (0.9, 0.9, 0.9), (0.0, 5e-4, 0.0))
    result = {"variant": a.variant, "nc": nc, "batch": B, "size": S, "accumulate": N, "rounds": a.rounds, "reps": a.reps, "steps": steps}

    # ---- (a) the launches, on the arenas of a network that has run one backward
    net, loss = bench.build(nc, dev, widen=widen, deepen=deepen)
    eng = net.engine()
    from object_detection_cib_amd.core.types import FeatureShape
    net.train_step(x, loss, FeatureShape(width=S, height=S), tg, float(B))
    eng.wait_grads()
    eng.set_hyper(*hyper, 1.0)
    eng.configure_clip(None)
    eng.configure_accumulation(N)
    n_p = eng.n_arena
    keep = [t.clone() for t in (eng.p_arena, eng.m_arena)]

    def accumulate(first):
        def run():
            eng.set_accumulate_first(first)       # (uploads only when the flag changes: once per window of calls)
            eng.accumulate_grads_device()
        return run
    legs = {"accumulate (add)": (accumulate(False), 12 * n_p), "accumulate (copy)": (accumulate(True), 8 * n_p),
            "sgd": (eng.sgd_step_device, 20 * n_p), "sgd on the accumulator": (lambda: eng.step_accumulated_device("sgd"), 20 * n_p)}
    for fn, _ in legs.values():
        for _ in range(5):
            fn()
    res = alternate(legs, a.rounds, lambda leg: timed(leg[0], a.reps))
    print(f"(a) {a.variant} nc {nc}: parameter arena {n_p} floats ({4 * n_p / 1e6:.1f} MB); the accumulate launch moves {12 * n_p / 1e6:.1f} MB, "
          f"the SGD launch {20 * n_p / 1e6:.1f} MB; us per call over {a.rounds} alternated windows of {a.reps} calls")
    for k, v in res.items():
        med = float(np.median(v))
        result[k + " us"] = [round(u, 2) for u in v]
        print(f"  {k:24s} median {med:7.1f}  min {min(v):7.1f}  max {max(v):7.1f}  | {legs[k][1] / med * 1e-3:6.0f} GB/s of its bytes", flush=True)
    ratio = float(np.median(res["accumulate (add)"]) / np.median(res["sgd"]))
    result["accumulate_over_sgd"] = round(ratio, 3)
    print(f"  accumulate (add) / sgd = {ratio:.3f} (expected <= 1: it moves 0.60 of the SGD launch's bytes)")
    update_us = float(np.median(res["sgd on the accumulator"]))
    for t, k in zip((eng.p_arena, eng.m_arena), keep):
        t.copy_(k)
    eng.mark_params_changed()
    eng.accumulation.reset()

    # ---- (b) the plain replayed step and the accumulating one, alternated
    if not a.no_step:
        plain = GraphedTrainStep(net, loss, B, S, S, max_targets=4096).capture(x, tg)
        accum = GraphedTrainStep(net, loss, B, S, S, max_targets=4096, accumulate_grad_batches=N).capture(x, tg)
        forms = {"plain step": lambda: plain(x, tg, *hyper, 1.0), f"accumulate_grad_batches={N}": lambda: accum(x, tg, *hyper, 1.0)}
        for fn in forms.values():
            for _ in range(2 * N):
                fn()
        assert not eng.accumulation.flush_needed
        res = alternate(forms, a.rounds, lambda fn: timed(fn, steps) / 1e3)
        base = res["plain step"]
        bmed = float(np.median(base))
        print(f"(b) replayed {a.variant} B={B} / {S} px, ms per micro-batch over {a.rounds} alternated windows of {steps} micro-batches")
        for k, v in res.items():
            med = float(np.median(v))
            result[k + " ms"] = [round(u, 4) for u in v]
            print(f"  {k:26s} median {med:7.3f}  min {min(v):7.3f}  max {max(v):7.3f}  | {B / med * 1e3:8.1f} images/s, rate x {bmed / med:.4f} "
                  f"of the plain step", flush=True)
        amed = float(np.median(res[f"accumulate_grad_batches={N}"]))
        allowance = update_us / 1e3 / N
        spread_hi = max(base)
        result.update(step_rate_ratio=round(bmed / amed, 4), update_us=round(update_us, 2), allowance_ms=round(allowance, 5),
                      within_allowance=bool(amed <= spread_hi + allowance))
        print(f"  allowance: the per-window update ({update_us:.1f} us) / {N} = {allowance * 1e3:.1f} us over the plain step's own spread "
              f"({min(base):.3f} - {spread_hi:.3f} ms): median {amed:.3f} ms is {'inside' if amed <= spread_hi + allowance else 'OUTSIDE'} "
              f"{spread_hi + allowance:.3f} ms")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(result, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
