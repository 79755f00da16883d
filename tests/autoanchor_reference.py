"""Plain numpy reference of csrc/anchors.hip and core/anchors/autoanchor.py: YOLOv5's anchor metric, its genetic evolution
and one Lloyd step of k-means.  Per-box values are float32 in the kernels' operation order (so they agree bit for bit);
every sum is float64 (the kernels sum the same terms in another order: tests allow N * 2^-52 relative there).  No scipy."""
from __future__ import annotations

import numpy as np

F32 = np.float32


def threshold(thr) -> np.float32:
    return F32(1.0 / float(thr))


def per_box(wh, k):
    """wh [N, 2], k [n, 2] float32 -> x [N, n] float32: min(min(r_w, 1 / r_w), min(r_h, 1 / r_h)), r = wh / k"""
    wh, k = np.asarray(wh, dtype=F32), np.asarray(k, dtype=F32)
    r = wh[:, None, :] / k[None, :, :]
    inv = F32(1.0) / r
    m = np.minimum(r, inv)
    return np.minimum(m[..., 0], m[..., 1])


def metric(wh, k, t):
    """-> (fitness_sum float64, n_recalled int, n_pairs int); strict comparisons against t (float32)"""
    x = per_box(wh, k)
    best = x.max(1)
    hit = best > F32(t)
    return float(best[hit].astype(np.float64).sum()), int(hit.sum()), int((x > F32(t)).sum())


def candidates(k, v):
    """k [n, 2], v [P, n, 2] float32 -> max(k * v, 2) float32 [P, n, 2]: one multiply, then a max"""
    return np.maximum(np.asarray(k, dtype=F32)[None] * np.asarray(v, dtype=F32), F32(2.0))


def evolve(wh, k, fitness, table, t):
    """The evolution loop.  table [gen, P, n, 2] -> (anchors, fitness_sum, trace [(winner, accepted, winner_sum)], gap):
    gap is the smallest distance met between a generation's best and second-best candidate sum and between its best
    candidate and the current fitness (a device sum reordered by less than that takes the same decisions)."""
    k = np.asarray(k, dtype=F32).copy()
    fitness = float(fitness)
    trace, gap = [], np.inf
    for v in np.asarray(table, dtype=F32):
        cand = candidates(k, v)
        sums = np.array([metric(wh, c, t)[0] for c in cand])
        win = int(np.argmax(sums))                       # first maximum: equal sums go to the lower index
        if len(sums) > 1:
            gap = min(gap, float(sums[win] - np.delete(sums, win).max()))
        gap = min(gap, abs(float(sums[win]) - fitness))
        acc = bool(sums[win] > fitness)
        if acc:
            k, fitness = cand[win].copy(), float(sums[win])
        trace.append((win, int(acc), float(sums[win])))
    return k, fitness, trace, gap


def mutation_table(rng, gen, population, n, mp=0.9, sigma=0.1, lo=0.3, hi=3.0):
    """The documented draw order of autoanchor.mutation_table, restated."""
    out = np.empty((gen, population, n, 2), dtype=F32)
    for g in range(gen):
        for p in range(population):
            while True:
                mask = rng.random((n, 2)) < mp
                u = rng.random()
                z = rng.standard_normal((n, 2))
                v = np.clip(mask * u * z * sigma + 1.0, lo, hi).astype(F32)
                if not (v == 1).all():
                    break
            out[g, p] = v
    return out


def lloyd_step(pts, cent):
    """pts [N, 2], cent [R, n, 2] float32 -> (new centroids float32 [R, n, 2], labels int32 [R, N], counts int64 [R, n],
    distortion float64 [R], sums float64 [R, n, 2])"""
    pts, cent = np.asarray(pts, dtype=F32), np.asarray(cent, dtype=F32)
    R, n, _ = cent.shape
    dx = pts[None, :, None, 0] - cent[:, None, :, 0]
    dy = pts[None, :, None, 1] - cent[:, None, :, 1]
    d = dx * dx + dy * dy                                 # float32 [R, N, n]
    labels = d.argmin(2).astype(np.int32)                 # first minimum: equal distances go to the lower index
    win = np.take_along_axis(d, labels[..., None].astype(np.int64), 2)[..., 0]
    distortion = win.astype(np.float64).sum(1)
    new = cent.copy()
    counts = np.zeros((R, n), dtype=np.int64)
    sums = np.zeros((R, n, 2), dtype=np.float64)
    for r in range(R):
        for j in range(n):
            m = labels[r] == j
            counts[r, j] = int(m.sum())
            if counts[r, j]:
                sums[r, j] = pts[m].astype(np.float64).sum(0)
                new[r, j] = (sums[r, j] / counts[r, j]).astype(F32)
    return new, labels, counts, distortion, sums


def filter_wh(wh):
    wh = np.asarray(wh, dtype=F32).reshape(-1, 2)
    return wh[(wh >= 2.0).any(1)]


def lognormal_wh(rng, N, mean=4.0, sigma=0.8):
    """log-normal box sizes clipped to [2, 640], float32 [N, 2]"""
    return np.clip(rng.lognormal(mean, sigma, (N, 2)), 2.0, 640.0).astype(F32)


def uniform_anchors(rng, n, image_size=640):
    """YOLOv5's sorted-uniform initialisation"""
    return (np.sort(rng.random(n * 2)).reshape(n, 2) * image_size).astype(F32)


# (N, gen, P, n): the evolution cases of tests/test_hip_autoanchor.py; the gap condition is asserted on the CPU too
EVOLVE_SHAPES = ((500, 40, 8, 9), (257, 40, 1, 9), (1000, 30, 4, 12))
_EVOLVE = {}


def evolve_case(shape):
    """inputs and the reference run of one evolution case, computed once and shared: dict(wh, k0, f0, table, t, k, f, trace, gap)"""
    if shape not in _EVOLVE:
        N, gen, P, n = shape
        rng = np.random.default_rng(1000 + N)
        wh = lognormal_wh(rng, N)
        k0 = np.maximum(uniform_anchors(rng, n), F32(2.0))
        table = mutation_table(rng, gen, P, n)
        t = threshold(4.0)
        f0 = metric(wh, k0, t)[0]
        k, f, trace, gap = evolve(wh, k0, f0, table, t)
        _EVOLVE[shape] = dict(wh=wh, k0=k0, f0=f0, table=table, t=t, k=k, f=f, trace=trace, gap=gap)
    return _EVOLVE[shape]
