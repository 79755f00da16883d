"""Cost of the fused Adam / AdamW update (csrc/adam.hip) on the flagship workload, one process, alternated windows:
(a) the kodhip_adam_step launch beside the SGD launch on the same arenas in the same run: device events around --reps
    back-to-back calls per window, us per call and GB/s of the bytes each moves (Adam 7 x 4 bytes per element, SGD 5 x 4).  Back
    to back the arenas stay in the Infinity Cache for both, as in tools/bench_ema.py: the comparison is between launches under
    the same conditions.  Expectation: the byte ratio 7 / 5 = 1.4; allowance 15 % over 1.4 x the SGD launch's median;
(b) the replayed step (hipGraph) with optimizer="adam" against optimizer="sgd", ms per step over windows of --steps steps
    (two captured programs over one network; the Adam one uploads its hyper block before every replay.  The two share
    m_arena - momentum for one, exp_avg for the other - so the Adam program runs with lr 0 here: the same launches and bytes,
    and the other program's momentum cannot throw the parameters off).
Diagnostic; nothing asserts a time.
usage: python tools/bench_adam.py [--variant yv5s] [--nc 80] [--batch 64] [--size 640] [--rounds 7] [--reps 50] [--steps 30] [--no-step]
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
    sgd_hyper = ((0.01, 0.01, 0.01), (0.9, 0.9, 0.9), (0.0, 5e-4, 0.0))
    count = [0]

    def adam_hyper(lr=1e-3):
        """AdamW with the step count moving, as FusedAdam.hyper() hands it over"""
        count[0] += 1
        return dict(lr=[lr] * 3, betas=[(0.9, 0.999)] * 3, eps=[1e-8] * 3, weight_decay=[0.0, 5e-4, 0.0], step=count[0],
                    maximize=False, decoupled=True)

    result = {"variant": a.variant, "nc": nc, "batch": B, "size": S, "rounds": a.rounds, "reps": a.reps, "steps": a.steps}

    # ---- (a) the launches, on the arenas of a network that has run one backward
    net, loss = bench.build(nc, dev, widen=widen, deepen=deepen)
    eng = net.engine()
    from object_detection_cib_amd.core.types import FeatureShape
    net.train_step(x, loss, FeatureShape(width=S, height=S), tg, float(B))
    eng.wait_grads()
    eng.set_hyper(*sgd_hyper, 1.0)
    eng.set_adam_hyper(**adam_hyper())
    eng.configure_clip(None)
    n_p = eng.n_arena
    keep = [t.clone() for t in (eng.p_arena, eng.m_arena, eng.v_arena)]
    legs = {"adam": (eng.adam_step_device, 28 * n_p), "sgd": (eng.sgd_step_device, 20 * n_p)}
    for fn, _ in legs.values():
        for _ in range(5):
            fn()
    res = alternate(legs, a.rounds, lambda leg: timed(leg[0], a.reps))
    print(f"(a) {a.variant} nc {nc}: parameter arena {n_p} floats; the Adam launch moves {28 * n_p / 1e6:.1f} MB, the SGD launch "
          f"{20 * n_p / 1e6:.1f} MB; us per call over {a.rounds} alternated windows of {a.reps} calls")
    for k, v in res.items():
        med = float(np.median(v))
        result[k + " us"] = [round(u, 2) for u in v]
        print(f"  {k:6s} median {med:7.1f}  min {min(v):7.1f}  max {max(v):7.1f}  | {legs[k][1] / med * 1e-3:6.0f} GB/s of its bytes", flush=True)
    ratio = float(np.median(res["adam"]) / np.median(res["sgd"]))
    result["adam_over_sgd"] = round(ratio, 3)
    print(f"  adam / sgd = {ratio:.3f} (byte ratio 1.400; allowance 1.15 x 1.4 = 1.610)")
    for t, k in zip((eng.p_arena, eng.m_arena, eng.v_arena), keep):
        t.copy_(k)
    eng.mark_params_changed()
    eng.adam_steps = 0

    # ---- (b) the replayed step with either update, two captured programs over one network, alternated
    if not a.no_step:
        gs = GraphedTrainStep(net, loss, B, S, S, max_targets=4096).capture(x, tg)
        ga = GraphedTrainStep(net, loss, B, S, S, max_targets=4096, optimizer="adam").capture(x, tg, adam=adam_hyper(0.0))
        forms = {"step, sgd": lambda: gs(x, tg, *sgd_hyper, 1.0), "step, adam": lambda: ga(x, tg, adam=adam_hyper(0.0))}
        for fn in forms.values():
            for _ in range(5):
                fn()
        res = alternate(forms, a.rounds, lambda fn: timed(fn, a.steps) / 1e3)
        base = float(np.median(res["step, sgd"]))
        print(f"(b) replayed {a.variant} B={B} / {S} px step, ms per step over {a.rounds} alternated windows of {a.steps} steps")
        for k, v in res.items():
            med = float(np.median(v))
            result[k + " ms"] = [round(u, 4) for u in v]
            print(f"  {k:12s} median {med:7.3f}  min {min(v):7.3f}  max {max(v):7.3f}  | rate x {base / med:.4f} of the SGD step", flush=True)
        result["step_rate_ratio"] = round(base / float(np.median(res["step, adam"])), 4)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(result, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
