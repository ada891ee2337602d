#!/usr/bin/env python3
"""Time of the object segmenter -- prep.cloud_planes (vlsat_cloud_planes), prep.cloud_clusters (vlsat_cloud_clusters) and the whole of
scan.segment_objects -- next to the numpy restatements, on two walled rooms (synth.make_walled_room(12, step, 3, height 2.5) plus
N(0, 0.002) on every coordinate) of about 10^5 and 5 x 10^5 points: dist 0.02, 1024 hypotheses, up to 8 planes, share 0.02,
outside_frac 0.01, cluster radius 1.6 x step, K = 16, min_points 50.  Device time: wall clock around one call including allocation of
outputs and scratch, device idle before and synchronised after, median of --reps after --warmup.  Each restatement runs ONCE on the
same arrays (the clusters' on the device's own neighbour table; the whole host route only on rooms below --host-route-below points: its
neighbour search is a numpy sweep that takes minutes beyond that).  There is no earlier device code to compare with: the restatement
beside it is the yardstick, and every device output is compared with it for equality of bits.  Recorded too: the planes found, the
clusters, dropped points, and evaluate.merge_quality of the clusters against the generating boxes over the points that got a cluster.
Synthetic boxes say nothing about real scans.  No threshold is set: what is measured is recorded.  Prints one JSON line per room and
writes them to --out."""
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
from vlsat_amd import evaluate as EV, lib as L, prep, scan, synth  # noqa: E402


def timed(fn, reps, warmup, sync):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        sync()
        t = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(out), 4), round(min(out), 4)


def once(fn):
    t = time.perf_counter()
    out = fn()
    return out, round((time.perf_counter() - t) * 1e3, 1)


def same(got, want):
    for g, w in zip(got, want):
        g, w = np.ascontiguousarray(g.cpu().numpy() if torch.is_tensor(g) else g), np.ascontiguousarray(w)
        if g.dtype != w.dtype or g.shape != w.shape or g.tobytes() != w.tobytes():
            return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=float, nargs="+", default=[0.045, 0.022])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n-hyp", type=int, default=1024)
    ap.add_argument("--host-route-below", type=int, default=200000)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "objects_probe.txt"))
    a = ap.parse_args()
    dev, sync = "cuda:0", torch.cuda.synchronize
    lines = []
    for step in a.steps:
        room = synth.make_walled_room(12, step, 3, height=2.5)
        pts = np.ascontiguousarray(room["points"] + np.random.default_rng(1).normal(0, 0.002, room["points"].shape), dtype=np.float32)
        d_p = torch.from_numpy(pts).to(dev)
        v = len(pts)
        min_inliers, radius = int(np.ceil(0.02 * v)), 1.6 * step
        r2 = float(np.float32(radius) ** 2)
        planes_kw = dict(n_hyp=a.n_hyp, max_planes=8, dist=0.02, min_inliers=min_inliers, outside_ppm=10000, seed=0)
        row = {"probe": "segment_objects", "step": step, "points": v, "n_hyp": a.n_hyp, "reps": a.reps, "lib_sha256": L.identity()["lib_sha256"][:16]}
        found = prep.cloud_planes(d_p, **planes_kw)
        row["planes"] = int(found.n_planes[0])
        row["plane_inliers"] = found.counts[:row["planes"], 0].tolist()
        row["planes_ms_median"], row["planes_ms_min"] = timed(lambda: prep.cloud_planes(d_p, **planes_kw), a.reps, a.warmup, sync)
        h_found, row["planes_host_ms"] = once(lambda: prep.cloud_planes_host(pts, **planes_kw))
        row["planes_equal_host"] = bool(same(found, h_found))
        row["planes_two_runs_equal"] = bool(same(prep.cloud_planes(d_p, **planes_kw), [x.cpu().numpy() for x in found]))
        rest = torch.nonzero(found.plane_id == 0).reshape(-1)
        table = prep.knn_points(d_p[rest], 16, r2)
        mask = torch.ones(len(rest), dtype=torch.int32, device=dev)
        grown = prep.cloud_clusters(table.index, table.sqdist, mask, r2, 50)
        row["rest_points"], row["clusters"] = len(rest), int(grown.n_clusters[0])
        row["clusters_ms_median"], row["clusters_ms_min"] = timed(lambda: prep.cloud_clusters(table.index, table.sqdist, mask, r2, 50), a.reps,
                                                                  a.warmup, sync)
        h_grown, row["clusters_host_ms"] = once(lambda: prep.cloud_clusters_host(table.index.cpu().numpy(), table.sqdist.cpu().numpy(),
                                                                                 np.ones(len(rest), np.int32), r2, 50))
        row["clusters_equal_host"] = bool(same(grown, h_grown))
        route = lambda device: scan.segment_objects({"points": pts}, 0.02, radius, n_hyp=a.n_hyp, device=device)   # noqa: E731
        out = route(dev)
        row["segment_objects_ms_median"], row["segment_objects_ms_min"] = timed(lambda: route(dev), max(3, a.reps // 6), 1, sync)
        if v < a.host_route_below:
            h_out, row["segment_objects_host_ms"] = once(lambda: route(None))
            row["segment_objects_equal_host"] = bool(np.array_equal(out["instances"], h_out["instances"]) and np.array_equal(out["seg_size"], h_out["seg_size"]))
        lab, gen = out["instances"], room["instances"]
        use = (lab > out["n_planes"]) & ~room["structural"]
        q = EV.merge_quality(lab[use], gen[use])
        row["segments"], row["dropped_points"] = int(out["n_segments"]), int((lab == 0).sum())
        row["structural_points_on_planes"] = round(float((lab[room["structural"]] > 0).mean() if out["n_planes"] else 0.0), 6)
        row["box_points_on_planes"] = int(((lab > 0) & (lab <= out["n_planes"]) & ~room["structural"]).sum())
        row["cluster_quality_vs_boxes"] = {k: (round(x, 6) if isinstance(x, float) else x) for k, x in q.items()}
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
