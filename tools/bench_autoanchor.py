"""Auto-anchor kernels (csrc/anchors.hip) at a dataset-sized input.  Diagnostic; nothing asserts a time.

N synthetic log-normal box sizes (default 2^20, clipped to [2, 640]), n = 9 anchors:
1. kodhip_anchor_evolve: ms per generation (one fitness launch + one select launch) at population 1 (YOLOv5's schedule) and at
   the largest population; device events around one call of --gens generations, --rounds calls after a warm-up call;
   median (min - max).
2. kodhip_anchor_kmeans_step: ms per Lloyd step of --restarts restarts (one launch pair), events around --steps steps.
3. The host baseline: the wall time of the numpy reference the tests compare against (tests/autoanchor_reference.py) on the
   same inputs - one generation at each population (64 candidates = 64 calls of its metric) and one Lloyd step (restart by
   restart, to bound its memory).  --no-host skips it.

usage: python tools/bench_autoanchor.py [--n-boxes 1048576] [--anchors 9] [--restarts 30] [--gens 200] [--steps 10] [--rounds 5]
                                        [--no-host] [--json PATH]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import autoanchor_reference as R
from object_detection_cib_amd import _lib; _lib.limit_host_threads()
from object_detection_cib_amd.core.anchors import autoanchor as A

ap = argparse.ArgumentParser()
ap.add_argument("--n-boxes", type=int, default=1 << 20); ap.add_argument("--anchors", type=int, default=9)
ap.add_argument("--restarts", type=int, default=30); ap.add_argument("--gens", type=int, default=200)
ap.add_argument("--steps", type=int, default=10); ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--no-host", action="store_true"); ap.add_argument("--json", default=None)
a = ap.parse_args()
_lib.require_gpu()
lib, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
N, n, Rn = a.n_boxes, a.anchors, a.restarts
PMAX = lib.kodhip_anchor_max_population()
T = float(R.threshold(4.0))


def stats(v):
    v = np.sort(np.asarray(v, dtype=np.float64))
    return {"median": float(np.median(v)), "min": float(v[0]), "max": float(v[-1])}


def fmt(s):
    return f"{s['median']:.4f} ({s['min']:.4f} - {s['max']:.4f})"


def timed(fn, per):
    """device events around fn() -> ms / per, --rounds times after one warm-up"""
    out = []
    for i in range(a.rounds + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        if i:
            out.append(e0.elapsed_time(e1) / per)
    return stats(out)


rng = np.random.default_rng(0)
wh = R.lognormal_wh(rng, N)
k0 = np.maximum(R.uniform_anchors(rng, n), np.float32(2.0))
d_wh = torch.from_numpy(wh).cuda()
ws = torch.empty(lib.kodhip_anchor_workspace_bytes(N, max(PMAX, Rn)), dtype=torch.uint8, device="cuda")
res = {"n_boxes": N, "anchors": n, "restarts": Rn, "device": torch.cuda.get_device_name(0)}

tables = {}
for P in (1, PMAX):
    gens = a.gens if P == 1 else max(a.gens // 10, 4)
    table = tables[P] = A.mutation_table(np.random.default_rng(P), gens, P, n)
    d_v = torch.from_numpy(table).cuda()
    d_k0 = torch.from_numpy(k0).cuda()
    d_k, d_f = d_k0.clone(), torch.zeros(1, dtype=torch.float64, device="cuda")
    trace = torch.empty(gens * lib.kodhip_anchor_trace_bytes(), dtype=torch.uint8, device="cuda")

    def evolve():
        d_k.copy_(d_k0); d_f.zero_()
        _lib.check(lib.kodhip_anchor_evolve(d_wh.data_ptr(), N, d_k.data_ptr(), d_f.data_ptr(), d_v.data_ptr(), gens, P, n, T,
                                            trace.data_ptr(), ws.data_ptr(), stream), "anchor_evolve")
    res[f"evolve_ms_per_generation_P{P}"] = s = timed(evolve, gens)
    print(f"evolve     N {N} n {n} P {P:2d}: {fmt(s)} ms per generation ({gens} generations per call)")

std = wh.astype(np.float64).std(0).astype(np.float32)
pts = np.ascontiguousarray(wh / std)
cent0 = np.stack([pts[rng.choice(N, n, replace=False)] for _ in range(Rn)])
d_pts, d_c = torch.from_numpy(pts).cuda(), torch.from_numpy(cent0).cuda()
d_dist = torch.empty(Rn, dtype=torch.float64, device="cuda"); d_cnt = torch.empty((Rn, n), dtype=torch.int64, device="cuda")


def lloyd():
    for _ in range(a.steps):
        _lib.check(lib.kodhip_anchor_kmeans_step(d_pts.data_ptr(), N, d_c.data_ptr(), Rn, n, ws.data_ptr(), d_dist.data_ptr(),
                                                 d_cnt.data_ptr(), None, stream), "anchor_kmeans_step")
res["kmeans_ms_per_step"] = s = timed(lloyd, a.steps)
print(f"k-means    N {N} n {n} R {Rn:2d}: {fmt(s)} ms per step ({a.steps} steps per window)")

if not a.no_host:
    host = {}
    for P in (1, PMAX):
        cand = R.candidates(k0, tables[P][0])
        t0 = time.perf_counter()
        sums = [R.metric(wh, c, T)[0] for c in cand]
        host[f"evolve_ms_per_generation_P{P}"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    for r in range(Rn):
        R.lloyd_step(pts, cent0[r:r + 1])
    host["kmeans_ms_per_step"] = 1e3 * (time.perf_counter() - t0)
    res["numpy_reference"] = host
    for key, v in host.items():
        print(f"numpy reference {key}: {v:.1f} ms  (x {v / res[key]['median']:.0f} the device)")
print(json.dumps(res))
if a.json:
    json.dump(res, open(a.json, "w"), indent=1)
