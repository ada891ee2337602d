#!/usr/bin/env python3
"""Time of prep.segment_mesh (vlsat_segment_mesh) next to its numpy restatement and next to scipy.sparse.csgraph.connected_components for
step 2 ALONE (the link graph's components; no absorb rounds, no numbering), on synth.make_box_mesh rooms of about 10^5 and 5 x 10^5
vertices (a floor and 12 boxes; normal_noise 0.05), at 10 degrees and min_verts 20.  Device time: wall clock around one call including
allocation of outputs and scratch and the read-back of the segment count (trim=True), device idle before and synchronised after, median
of --reps after --warmup; the two host routes are timed on CPU copies of the same arrays (fewer repetitions: they are slow).  On the
smaller room it also reports, for 5 / 10 / 15 / 20 degrees, how the segments relate to the room's planar faces: segments per face and
evaluate.merge_quality with the segment as "object" and the planar face as "instance" over the non-crease vertices (precision: a
segment stays inside one face; recall: a face is one segment).  Synthetic boxes say nothing about real scans.  No threshold is set:
what is measured is recorded.  Prints one JSON line per row and writes them to --out."""
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
    return statistics.median(out), min(out)


def max_weight(deg):
    return float(np.float32(1.0 - math.cos(math.radians(deg))))


def scipy_step2(normals, edges, w_max):
    """connected components of the link graph, weights computed in numpy as the restatement computes them"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    a, b = edges[:, 0], edges[:, 1]
    link = prep.segment_weights_host(normals, a, b) <= np.float32(w_max)
    v = len(normals)
    return connected_components(coo_matrix((np.ones(int(link.sum()), np.int8), (a[link], b[link])), shape=(v, v)), directed=False)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=float, nargs="+", default=[0.038, 0.017], help="grid spacing per room: 10 m / step squared is the floor")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "segment_probe.txt"))
    a = ap.parse_args()
    dev = "cuda:0"
    lines = []
    for n_room, step in enumerate(a.steps):
        room = synth.make_box_mesh(12, step, 77, normal_noise=0.05)
        normals = np.ascontiguousarray(room["normals"], dtype=np.float32)
        edges = prep.mesh_edges(room["faces"])
        d_n, d_e = torch.from_numpy(normals).to(dev), torch.from_numpy(edges).to(dev)
        w = max_weight(10.0)
        hip = lambda: prep.segment_mesh(d_n, d_e, w, 20)
        host = lambda: prep.segment_mesh_host(normals, edges, w, 20)
        g, h = hip(), host()
        same = torch.equal(g.labels.cpu(), h.labels) and g.n_segments == h.n_segments and torch.equal(g.seg_size.cpu(), h.seg_size)
        row = {"probe": "segment_mesh", "vertices": len(normals), "edges": len(edges), "max_angle_deg": 10.0, "min_verts": 20,
               "rounds": prep.segment_rounds(20), "segments": g.n_segments, "dropped_vertices": int((g.labels == 0).sum()),
               "link_components_scipy": int(scipy_step2(normals, edges, w)), "hip_equals_host": bool(same), "reps": a.reps,
               "lib_sha256": L.identity()["lib_sha256"][:16]}
        row["hip_ms_median"], row["hip_ms_min"] = (round(x, 4) for x in timed(hip, a.reps, a.warmup, torch.cuda.synchronize))
        few = max(3, a.reps // 10)
        row["host_ms_median"], row["host_ms_min"] = (round(x, 2) for x in timed(host, few, 1, lambda: None))
        row["scipy_step2_ms_median"], row["scipy_step2_ms_min"] = (round(x, 2) for x in timed(lambda: scipy_step2(normals, edges, w), few, 1, lambda: None))
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
        if n_room:
            continue
        flat = room["plane"] >= 0
        n_faces = len(np.unique(room["plane"][flat]))
        for deg in (5.0, 10.0, 15.0, 20.0):
            s = prep.segment_mesh(d_n, d_e, max_weight(deg), 20)
            lab = s.labels.cpu().numpy()
            use = flat & (lab > 0)                                                 # (dropped vertices are counted, not scored)
            q = EV.merge_quality(lab[use], room["plane"][use])
            lines.append(json.dumps({"probe": "segments_per_planar_face", "vertices": len(normals), "normal_noise": 0.05, "max_angle_deg": deg,
                                     "segments": s.n_segments, "planar_faces": n_faces, "segments_per_face": round(s.n_segments / n_faces, 3),
                                     "dropped_vertices": int((lab == 0).sum()), "precision": round(q["precision"], 6),
                                     "recall": round(q["recall"], 6), "f1": round(q["f1"], 6), "segments_over_two_faces": q["over_merged"],
                                     "faces_in_pieces": q["split"]}))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
