#!/usr/bin/env python3
"""Time of scan.split_scan (vlsat_split_seeds + vlsat_split_groups) and of metrics.fuse_splits (vlsat_fuse_splits) next to their numpy
restatements on the same inputs: synth.make_room rooms of 10^5 and 5 x 10^5 vertices (1 000 points per object, 10 x 10 x 3 m), the
reference's defaults (distance 1.0, box 0.75, at least 5 segments).  The fusion input is what the split yields: one row per (group,
instance), fully connected edges inside every group, random probabilities (no trained checkpoint: the inputs exercise the step, they
say nothing about accuracy).  Device time: wall clock around one call including the upload of the mesh (split_scan takes a host mesh),
allocation of outputs and scratch and the read-backs (the seed count and the bit table; the two totals), device idle before and
synchronised after, median of --reps after --warmup; the host restatements are timed on the same arrays.  Prints one JSON line per
size and writes them to --out."""
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
from vlsat_amd import lib as L, metrics as M, prep, scan, synth  # noqa: E402


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


def fusion_input(groups, seed, dev):
    g = np.random.default_rng(seed)
    rows = [i for grp in groups for i in grp]
    edges, off = [], 0
    for grp in groups:
        n = len(grp)
        a, b = np.nonzero(~np.eye(n, dtype=bool))
        edges.append(np.stack([a + off, b + off], 1))
        off += n
    edges = np.concatenate(edges) if edges else np.zeros((0, 2), np.int64)
    probs = torch.softmax(torch.from_numpy(g.standard_normal((len(rows), 160)).astype(np.float32) * 4), -1)
    rel = torch.from_numpy(g.random((len(edges), 26), dtype=np.float32))
    w = torch.from_numpy(g.integers(100, 2000, len(rows)).astype(np.float32))
    return rows, [t.to(dev) for t in (probs, rel, torch.from_numpy(edges), w)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vertices", type=int, nargs="+", default=[100_000, 500_000])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "split_probe.txt"))
    a = ap.parse_args()
    dev = "cuda:0"
    lines = []
    for v in a.vertices:
        pts, inst = synth.make_room(v // 1000, 1000, 77)
        mesh = {"points": pts, "instances": inst}
        hip = lambda: scan.split_scan(mesh, seed=7, device=dev)
        host = lambda: scan.split_scan(mesh, seed=7, device=None)
        s, h = hip(), host()
        row = {"probe": "split_scan", "vertices": int(len(pts)), "segments": int(len(np.unique(inst))), "seeds": int(len(s.seeds)),
               "seed_cap": prep.split_seed_cap(pts, 1.0), "groups_kept": len(s.groups), "group_sizes": [len(g) for g in s.groups],
               "hip_equals_host": s.groups == h.groups and s.seeds.tolist() == h.seeds.tolist(), "reps": a.reps,
               "lib_sha256": L.identity()["lib_sha256"][:16]}
        few = max(3, a.reps // 5)
        row["split_hip_ms_median"], row["split_hip_ms_min"] = (round(x, 4) for x in timed(hip, a.reps, a.warmup, torch.cuda.synchronize))
        row["split_host_ms_median"], row["split_host_ms_min"] = (round(x, 4) for x in timed(host, few, 1, lambda: None))
        rows, (probs, rel, edges, w) = fusion_input(s.groups, 78, dev)
        cpu = [t.cpu() for t in (probs, rel, edges, w)]
        f_hip = lambda: M.fuse_splits(probs, rel, edges, rows, w, obj_probs=probs, rel_probs=rel)
        f_host = lambda: M.fuse_splits_host(cpu[0], cpu[1], cpu[2], rows, cpu[3], obj_probs=cpu[0], rel_probs=cpu[1])
        g, gh = f_hip(), f_host()
        row.update({"fuse_rows": len(rows), "fuse_edges": int(edges.shape[0]), "fused_objects": int(g.totals[0]), "fused_pairs": int(g.totals[1]),
                    "fuse_hip_equals_host": all(torch.equal(getattr(g, k).cpu(), getattr(gh, k)) for k in M.FusedGraph._FIELDS)})
        row["fuse_hip_ms_median"], row["fuse_hip_ms_min"] = (round(x, 4) for x in timed(f_hip, a.reps, a.warmup, torch.cuda.synchronize))
        row["fuse_host_ms_median"], row["fuse_host_ms_min"] = (round(x, 4) for x in timed(f_host, few, 1, lambda: None))
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
