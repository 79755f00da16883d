"""Cost of gradient clipping on the flagship workload, one process, alternating order:
(a) the norm launches (partials + finalize; plain and non-temporal loads) and the SGD launch on the network's own arenas,
    device events, us per call and GB/s of the bytes each reads / writes;
(b) the replayed step (hipGraph) with clipping off, with track_grad_norm and with norm clipping, ms per step.
usage: python tools/bench_clip.py [--variant yv5s] [--batch 64] [--size 640] [--rounds 5] [--steps 30] [--no-step]"""
import argparse
import os
import sys

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="yv5s", choices=sorted(bench.VARIANTS))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--no-step", action="store_true", help="kernels only")
    a = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    widen, deepen = bench.VARIANTS[a.variant]
    nc, B, S = 10, a.batch, a.size
    x, tg = bench.synth_batch(B, S, nc, 2023, dev)
    hyper = ((0.01, 0.01, 0.01), (0.9, 0.9, 0.9), (0.0, 5e-4, 0.0))

    # ---- (a) kernels on the arena of a network that has run one backward
    net, loss = bench.build(nc, dev, widen=widen, deepen=deepen)
    eng = net.engine()
    from object_detection_cib_amd.core.types import FeatureShape
    net.train_step(x, loss, FeatureShape(width=S, height=S), tg, float(B))
    eng.wait_grads()
    eng.set_hyper(*hyper, 1.0)
    n = eng.n_arena
    keep = [t.clone() for t in (eng.p_arena, eng.m_arena)]
    legs = {
        "norm (plain loads)": (lambda: (setattr(eng, "norm_nontemporal", False), eng.grad_norm_device()), 5 * n),
        "norm (non-temporal)": (lambda: (setattr(eng, "norm_nontemporal", True), eng.grad_norm_device()), 5 * n),
        "sgd": (lambda: (eng.configure_clip(None), eng.sgd_step_device()), 20 * n),
        "norm + clipped sgd": (lambda: (setattr(eng, "norm_nontemporal", False), eng.configure_clip("norm"),
                                        eng.sgd_step_device()), 25 * n),
        "norm(nt) + clipped sgd": (lambda: (setattr(eng, "norm_nontemporal", True), eng.configure_clip("norm"),
                                            eng.sgd_step_device()), 25 * n),
    }
    eng.set_clip(1.0)
    for fn, _ in legs.values():
        for _ in range(5):
            fn()
    res = {k: [] for k in legs}
    for r in range(a.rounds):
        order = list(legs) if r % 2 == 0 else list(legs)[::-1]
        for k in order:
            res[k].append(timed(legs[k][0], 50))
    print(f"(a) {a.variant}: arena {n} floats ({4 * n / 1e6:.1f} MB); us per call over {a.rounds} alternating rounds of 50 calls")
    for k, v in res.items():
        med = sorted(v)[len(v) // 2]
        print(f"  {k:24s} median {med:7.1f}  min {min(v):7.1f}  max {max(v):7.1f}  | {legs[k][1] / med * 1e-3:6.0f} GB/s of its bytes")
    eng.norm_nontemporal = False
    eng.configure_clip(None)
    for t, k in zip((eng.p_arena, eng.m_arena), keep):
        t.copy_(k)
    if a.no_step:
        return

    # ---- (b) the replayed step, three captured programs on one network, alternating
    steps = {}
    for name, kw in (("off", {}), ("track_grad_norm", dict(track_grad_norm=True)), ("clip norm", dict(gradient_clip_val=1.0))):
        steps[name] = GraphedTrainStep(net, loss, B, S, S, max_targets=4096, **kw).capture(x, tg)
    res = {k: [] for k in steps}
    for k, gs in steps.items():
        for _ in range(5):
            gs(x, tg, *hyper, 1.0)
    for r in range(a.rounds):
        order = list(steps) if r % 2 == 0 else list(steps)[::-1]
        for k in order:
            res[k].append(timed(lambda: steps[k](x, tg, *hyper, 1.0), a.steps) / 1e3)
    print(f"(b) replayed {a.variant} B={B} / {S} px step, ms per step over {a.rounds} alternating rounds of {a.steps} steps")
    base = sorted(res["off"])[len(res["off"]) // 2]
    for k, v in res.items():
        med = sorted(v)[len(v) // 2]
        print(f"  {k:18s} median {med:7.3f}  min {min(v):7.3f}  max {max(v):7.3f}  | {100 * (med / base - 1):+5.2f} % vs off")


if __name__ == "__main__":
    main()
