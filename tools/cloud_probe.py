#!/usr/bin/env python3
"""Time of the point-cloud front end -- prep.knn_points (vlsat_cloud_knn), prep.cloud_normals (vlsat_cloud_normals), prep.segment_cloud
(vlsat_segment_cloud) and the whole scan.segment_cloud -- next to the numpy restatements and, if scipy is installed, next to
scipy.spatial.cKDTree.query for the neighbour search alone, on synth.make_box_mesh rooms of about 10^5 and 5 x 10^5 vertices with the
faces dropped (a floor and 12 boxes), radius = 3 x step, K = 16, 10 degrees, min_verts 20, max_curvature 0.02.  Device time: wall clock
around one call including allocation of outputs and scratch (and, for segment_cloud, the read-back of the segment count; for
scan.segment_cloud, the upload and every read-back), device idle before and synchronised after, median of --reps after --warmup.  The
host routes run ONCE each on the same arrays (the restated neighbour search takes about a minute on the larger room).  Also reported:
whether every device output equals the restatement bit for bit, the segment count, and evaluate.merge_quality with the segment as
"object" and the room's planar face as "instance" over the non-crease points that got a segment -- a box's bottom face and the floor it
lies in count as one plane, since no cloud can tell them apart -- once over all of them and once over the flat ones alone (curvature <=
max_curvature: the points within a radius of a crease are handed to a neighbouring segment by design).  Synthetic boxes say nothing
about real scans.  No threshold is set: what is measured is recorded.  Prints one JSON line per room and writes them to --out."""
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


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=float, nargs="+", default=[0.038, 0.017], help="grid spacing per room: 10 m / step squared is the floor")
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "cloud_probe.txt"))
    a = ap.parse_args()
    dev, sync = "cuda:0", torch.cuda.synchronize
    w = float(np.float32(1.0 - math.cos(math.radians(10.0))))
    lines = []
    for step in a.steps:
        room = synth.make_box_mesh(12, step, 77)
        pts = np.ascontiguousarray(room["points"], dtype=np.float32)
        radius = 3.0 * step
        m = float(np.float32(radius) ** 2)
        d_p = torch.from_numpy(pts).to(dev)
        row = {"probe": "segment_cloud", "points": len(pts), "radius": round(radius, 4), "k": a.k, "max_angle_deg": 10.0, "min_verts": 20,
               "max_curvature": 0.02, "reps": a.reps, "lib_sha256": L.identity()["lib_sha256"][:16]}
        # each stage on the device, on the previous stage's device output
        table = prep.knn_points(d_p, a.k, m)
        normals, curv = prep.cloud_normals(d_p, table.index, table.count, 5)
        masked = torch.where((curv > float(np.float32(0.02)))[:, None], torch.zeros_like(normals), normals)
        seg = prep.segment_cloud(masked, table.index, w, 20)
        row["knn_ms_median"], row["knn_ms_min"] = timed(lambda: prep.knn_points(d_p, a.k, m), a.reps, a.warmup, sync)
        row["normals_ms_median"], row["normals_ms_min"] = timed(lambda: prep.cloud_normals(d_p, table.index, table.count, 5), a.reps, a.warmup, sync)
        row["segment_ms_median"], row["segment_ms_min"] = timed(lambda: prep.segment_cloud(masked, table.index, w, 20), a.reps, a.warmup, sync)
        cloud = {"points": room["points"]}
        whole = lambda: scan.segment_cloud(cloud, radius, k=a.k, device=dev)     # noqa: E731
        out = whole()
        row["scan_segment_cloud_ms_median"], row["scan_segment_cloud_ms_min"] = timed(whole, a.reps, a.warmup, sync)
        # the restatements, once each, and equality stage by stage
        h_table, row["knn_host_ms"] = once(lambda: prep.knn_points_host(pts, a.k, m))
        (h_n, h_c), row["normals_host_ms"] = once(lambda: prep.cloud_normals_host(pts, h_table.index, h_table.count, 5))
        h_masked = np.where((h_c > np.float32(0.02))[:, None], np.float32(0), h_n)
        h_seg, row["segment_host_ms"] = once(lambda: prep.segment_mesh_host(h_masked, prep.knn_edges(h_table.index), w, 20, unsigned=True))
        row["knn_equals_host"] = bool(all(same_bits(g.cpu().numpy(), h) for g, h in zip(table, h_table)))
        row["normals_equal_host"] = bool(same_bits(normals.cpu().numpy(), h_n) and same_bits(curv.cpu().numpy(), h_c))
        row["segments_equal_host"] = bool(torch.equal(seg.labels.cpu(), h_seg.labels) and seg.n_segments == h_seg.n_segments
                                          and torch.equal(seg.seg_size.cpu(), h_seg.seg_size))
        row["scan_equals_stages"] = bool(np.array_equal(out["instances"], h_seg.labels.numpy()) and same_bits(out["curvature"], h_c))
        try:
            from scipy.spatial import cKDTree
            tree, row["ckdtree_build_ms"] = once(lambda: cKDTree(pts))
            _, row["ckdtree_query_ms"] = once(lambda: tree.query(pts, k=a.k + 1, distance_upper_bound=radius))
        except ImportError:
            row["ckdtree_query_ms"] = None
        lab = out["instances"]
        plane = room["plane"].copy()
        plane[(plane > 0) & ((plane - 1) % 6 == 4)] = 0                            # a box's bottom face lies in the floor
        use = (plane >= 0) & (lab > 0)
        q = EV.merge_quality(lab[use], plane[use])
        flat = use & (h_c <= np.float32(0.02))                                     # without the points the flatness mask hands to a neighbour
        qf = EV.merge_quality(lab[flat], plane[flat])
        row.update({"neighbours_mean": round(float(h_table.count.mean()), 2), "points_above_max_curvature": int((h_c > np.float32(0.02)).sum()),
                    "segments": int(out["n_segments"]), "planes": int(len(np.unique(plane[plane >= 0]))),
                    "dropped_points": int((lab == 0).sum()), "precision": round(q["precision"], 6), "recall": round(q["recall"], 6),
                    "f1": round(q["f1"], 6), "segments_over_two_planes": q["over_merged"], "planes_in_pieces": q["split"],
                    "flat_points": int(flat.sum()), "flat_precision": round(qf["precision"], 6), "flat_recall": round(qf["recall"], 6),
                    "flat_segments_over_two_planes": qf["over_merged"], "flat_planes_in_pieces": qf["split"]})
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
