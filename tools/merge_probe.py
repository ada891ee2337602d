#!/usr/bin/env python3
"""Time of metrics.merge_segments (vlsat_merge_segments) next to its host restatement on the same inputs: synth.make_room rooms
whose objects are cut into about 5 segments each, proximity edges between the segments (prep.proximity_edges on the segments'
boxes), random class probabilities, and as "same part" probability 0.9 for an edge between two segments of one object and 0.1
otherwise (no trained checkpoint predicts the relation: the inputs exercise the step, they say nothing about accuracy).  At 200 and
1 000 segments.  Device time: wall clock around one call including allocation of outputs and scratch and the read-back of the two
totals (trim=True), device idle before and synchronised after, median of --reps after --warmup; the host restatement is timed on
CPU copies of the same tensors.  Prints one JSON line per size and writes them to --out."""
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
from vlsat_amd import lib as L, metrics as M, prep, synth  # noqa: E402


def room(n_segments: int, per_object: int, seed: int, dev):
    n_obj = max(1, n_segments // per_object)
    pts, inst = synth.make_room(n_obj, 64 * per_object, seed)
    g = np.random.default_rng(seed)
    # cut every object along x into `per_object` slabs of equal point count: segment ids 1..n_obj * per_object
    seg = np.zeros_like(inst)
    for o in range(n_obj):
        idx = np.nonzero(inst == o + 1)[0]
        order = idx[np.argsort(pts[idx, 0], kind="stable")]
        seg[order] = o * per_object + 1 + np.arange(len(order)) // 64
    ids = np.arange(1, n_obj * per_object + 1, dtype=np.int32)
    d = lambda a: torch.from_numpy(a).to(dev)
    boxes = prep.instance_boxes(d(pts), d(seg.astype(np.int32)), d(ids))
    edges = prep.proximity_edges(boxes, [len(ids)], padding=0.25, max_neighbors=16)[0].t().contiguous()
    n, e = len(ids), edges.shape[0]
    obj_of = torch.from_numpy((ids - 1) // per_object).to(dev)
    same = obj_of[edges[:, 0]] == obj_of[edges[:, 1]]
    rel = torch.from_numpy(g.random((e, 26), dtype=np.float32)).to(dev)
    rel[:, 25] = torch.where(same, 0.9, 0.1)
    probs = torch.softmax(torch.from_numpy(g.standard_normal((n, 160)).astype(np.float32) * 4).to(dev), -1)
    w = torch.full((n,), 64.0, device=dev)
    return probs, rel, edges, w, n_obj


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, nargs="+", default=[200, 1000])
    ap.add_argument("--per-object", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "merge_probe.txt"))
    a = ap.parse_args()
    dev = "cuda:0"
    lines = []
    for n_seg in a.segments:
        probs, rel, edges, w, n_obj = room(n_seg, a.per_object, 77, dev)
        args = (None, 1, 25, 0.5)
        hip = lambda mutual: M.merge_segments(probs, rel, edges, *args, mutual, w, obj_probs=probs, rel_probs=rel)
        cpu = [t.cpu() for t in (probs, rel, edges, w)]
        host = lambda mutual: M.merge_segments_host(cpu[0], cpu[1], cpu[2], *args, mutual, cpu[3], obj_probs=cpu[0], rel_probs=cpu[1])
        g, h = hip(False), host(False)
        same = all(torch.equal(getattr(g, k).cpu(), getattr(h, k)) for k in M._MG_FIELDS)
        row = {"probe": "merge_segments", "segments": int(probs.shape[0]), "objects_cut": n_obj, "edges": int(edges.shape[0]),
               "objects_found": int(g.totals[0]), "merged_edges": int(g.totals[1]), "hip_equals_host": same, "reps": a.reps,
               "lib_sha256": L.identity()["lib_sha256"][:16]}
        for mutual in (False, True):
            k = "mutual" if mutual else "plain"
            row[f"hip_{k}_ms_median"], row[f"hip_{k}_ms_min"] = (round(x, 4) for x in timed(lambda: hip(mutual), a.reps, a.warmup, torch.cuda.synchronize))
            row[f"host_{k}_ms_median"], row[f"host_{k}_ms_min"] = (round(x, 4) for x in timed(lambda: host(mutual), max(3, a.reps // 5), 1, lambda: None))
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
