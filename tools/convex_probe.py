#!/usr/bin/env python3
"""Time of the convexity clusters -- prep.convex_clusters (vlsat_convex_clusters) -- beside prep.cloud_clusters on the SAME neighbour
table at the earlier rule, and the numpy restatement once, on synth.make_stacked_boxes tiled to about 10^5 and 5 x 10^5 points: every
tile is the scene with its own jitter (seed = tile), moved by 2.0 along x and 1.6 along y so that tiles do not touch; K = 16 within
0.06, normals estimated on the device and turned to a viewpoint far away in the scene's viewing direction (every tile then shows the
same faces), links up to 0.03, tau = sin 10 deg, min_points 20, 8 absorption rounds.  The method is tools/objects_probe.py's: wall
clock around one call including allocation of outputs and scratch, device idle before and synchronised after, median of --reps after
--warmup.  Recorded too: the clusters, the states, the unlabelled points, equality of bits with the restatement and between two runs,
and evaluate.merge_quality of both clusterings against the generating boxes.  There is no time gate: the number to read is
ratio_to_cloud_clusters, whatever it is.  Synthetic boxes say nothing about real scans.  Prints one JSON line per cloud and writes
them to --out."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vlsat_amd  # noqa: E402,F401
from vlsat_amd import evaluate as EV, lib as L, prep, synth  # noqa: E402


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


def same(got, want):
    for g, w in zip(got, want):
        g, w = np.ascontiguousarray(g.cpu().numpy() if torch.is_tensor(g) else g), np.ascontiguousarray(w)
        if g.dtype != w.dtype or g.shape != w.shape or g.tobytes() != w.tobytes():
            return False
    return True


def tiled(tiles):
    """-> (points f32 [V,3], generating body int64 [V], unique per tile and box)"""
    side = int(math.ceil(math.sqrt(tiles)))
    pts, gen = [], []
    for t in range(tiles):
        scene = synth.make_stacked_boxes(seed=t)
        pts.append(scene["points"] + np.array([2.0 * (t % side), 1.6 * (t // side), 0.0]))
        gen.append(scene["instances"] + 8 * t)
    return np.ascontiguousarray(np.concatenate(pts), dtype=np.float32), np.concatenate(gen)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, nargs="+", default=[14, 70])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "convex_probe.txt"))
    a = ap.parse_args()
    dev, sync = "cuda:0", torch.cuda.synchronize
    view = tuple(1000.0 * x for x in (3.0, -2.5, 2.5))
    reach2, link2, tau = float(np.float32(0.06) ** 2), float(np.float32(0.03) ** 2), float(np.float32(math.sin(math.radians(10.0))))
    lines = []
    for tiles in a.tiles:
        pts, gen = tiled(tiles)
        v = len(pts)
        d_p = torch.from_numpy(pts).to(dev)
        table = prep.knn_points(d_p, 16, reach2)
        normals = prep.cloud_normals(d_p, table.index, table.count, 5, view)[0]
        mask = torch.ones(v, dtype=torch.int32, device=dev)
        row = {"probe": "convex_clusters", "tiles": tiles, "points": v, "k": 16, "reps": a.reps, "lib_sha256": L.identity()["lib_sha256"][:16]}
        convex = lambda: prep.convex_clusters(d_p, normals, table.index, table.sqdist, mask, link2, tau, 20, 8)       # noqa: E731
        near = lambda: prep.cloud_clusters(table.index, table.sqdist, mask, link2, 20)                                 # noqa: E731
        out, grown = convex(), near()
        row["convex_ms_median"], row["convex_ms_min"] = timed(convex, a.reps, a.warmup, sync)
        row["cloud_clusters_ms_median"], row["cloud_clusters_ms_min"] = timed(near, a.reps, a.warmup, sync)
        row["ratio_to_cloud_clusters"] = round(row["convex_ms_median"] / row["cloud_clusters_ms_median"], 3)
        t = time.perf_counter()
        host = prep.convex_clusters_host(pts, normals.cpu().numpy(), table.index.cpu().numpy(), table.sqdist.cpu().numpy(), np.ones(v, np.int32),
                                         link2, tau, 20, 8)
        row["convex_host_ms"] = round((time.perf_counter() - t) * 1e3, 1)
        row["equal_host"] = bool(same(out, host))
        row["two_runs_equal"] = bool(same(convex(), [x.cpu().numpy() for x in out]))
        lab, old = out.labels.cpu().numpy(), grown.labels.cpu().numpy()
        row["bodies"], row["clusters"], row["cloud_clusters"] = 5 * tiles, int(out.n_clusters[0]), int(grown.n_clusters[0])
        row["states"] = np.bincount(out.state.cpu().numpy(), minlength=5).tolist()
        row["unlabelled_points"], row["cloud_clusters_dropped_points"] = int((lab == 0).sum()), int((old == 0).sum())
        for name, labels in (("quality_vs_boxes", lab), ("cloud_clusters_quality_vs_boxes", old)):
            q = EV.merge_quality(labels[labels > 0], gen[labels > 0])
            row[name] = {k: (round(x, 6) if isinstance(x, float) else x) for k, x in q.items()}
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
