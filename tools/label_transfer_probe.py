#!/usr/bin/env python3
"""Annotation transfer onto a predicted segmentation (prep.nearest_points, scan.transfer_labels) on synthetic rooms of 10^5 and
5 x 10^5 points per cloud: the annotated cloud is points on the faces of boxes standing in a 10 x 10 x 3 m room, the predicted
cloud a jittered resample of it whose segments cut every instance in two.  Times, medians over ``--reps`` after a warm-up:
``nearest_points`` alone (HIP events; device tensors in and out), the whole ``transfer_labels`` from host arrays to the mapping
(host clock, ends in the read-back of the per-segment arrays), and the host path of the nearest-point query -- scipy's cKDTree
(build + query, float64, not bit-compatible with the rule) when scipy is importable, else ``prep.nearest_points_host`` at the
smaller size only.  Prints one JSON line per size."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vlsat_amd  # noqa: E402,F401
from vlsat_amd import prep, scan  # noqa: E402


def room(n_points, seed, n_obj=60):
    rng = np.random.default_rng(seed)
    centre = rng.uniform([0.5, 0.5, 0.3], [9.5, 9.5, 2.0], size=(n_obj, 3))
    half = rng.uniform(0.15, 0.6, size=(n_obj, 3))
    inst = rng.integers(1, n_obj + 1, size=n_points)
    p = rng.uniform(-1, 1, size=(n_points, 3))
    axis = rng.integers(0, 3, size=n_points)
    p[np.arange(n_points), axis] = np.sign(p[np.arange(n_points), axis])            # onto a face
    gt = (centre[inst - 1] + half[inst - 1] * p).astype(np.float32)
    src = rng.integers(0, n_points, size=n_points)
    pd = (gt[src] + rng.normal(scale=0.01, size=(n_points, 3))).astype(np.float32)
    seg = 2 * inst[src] - (gt[src, 0] < centre[inst[src] - 1, 0])                   # every instance in two segments
    return ({"points": pd, "instances": seg.astype(np.int64)}, {"points": gt, "instances": inst.astype(np.int64)},
            {i: "object" for i in range(1, n_obj + 1)})


def median_ms(fn, reps, events):
    ts = []
    for it in range(reps + 2):
        if events:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            t = a.elapsed_time(b)
        else:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t = 1e3 * (time.perf_counter() - t0)
        if it >= 2:
            ts.append(t)
    return round(statistics.median(ts), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sizes", type=int, nargs="+", default=[100000, 500000])
    ap.add_argument("--max-sq-dist", type=float, default=0.1)
    a = ap.parse_args()
    dev = "cuda:0"
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
    for n in a.sizes:
        pd, gt, labels = room(n, 41)
        d_pd, d_gt = torch.from_numpy(pd["points"]).to(dev), torch.from_numpy(gt["points"]).to(dev)
        out = {"probe": "label_transfer", "points_per_cloud": n, "max_sq_dist": a.max_sq_dist, "reps": a.reps}
        out["nearest_points_ms"] = median_ms(lambda: prep.nearest_points(d_pd, d_gt, a.max_sq_dist), a.reps, True)
        t = scan.transfer_labels(pd, gt, labels, max_sq_dist=a.max_sq_dist, device=dev)
        out["segments"], out["matched"], out["without_correspondence"] = len(t.segment_ids), len(t.segment_to_gt), t.n_without_correspondence
        out["transfer_labels_ms"] = median_ms(lambda: scan.transfer_labels(pd, gt, labels, max_sq_dist=a.max_sq_dist, device=dev), a.reps, False)
        if cKDTree is not None:
            def host():
                d, i = cKDTree(gt["points"].astype(np.float64)).query(pd["points"].astype(np.float64), k=1)
                return i
            out["host"] = "scipy.spatial.cKDTree build + query (float64)"
        elif n <= min(a.sizes):
            def host():
                return prep.nearest_points_host(pd["points"], gt["points"], a.max_sq_dist)[0]
            out["host"] = "prep.nearest_points_host (numpy)"
        else:
            host = None
        if host is not None:
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                host()
                ts.append(1e3 * (time.perf_counter() - t0))
            out["host_nearest_ms"] = round(statistics.median(ts), 1)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
