#!/usr/bin/env python3
"""Time of the voxel-grid filter -- prep.voxel_downsample (vlsat_voxel_assign + vlsat_voxel_reduce) -- next to its numpy restatement, on
two clouds: the FUSED room (synth.make_box_mesh(12, 0.05, 3) without faces, every point jittered by N(0, 0.002) and the half x < 5 seen
eight more times with N(0, 0.005) noise: synth.make_fused_cloud, 311 605 points) and a uniform room of about 5 x 10^5 points
(synth.make_box_mesh(12, 0.017, 77)), both on a grid of edge 0.05, bare and with normals and colours.  Device time: wall clock around one
call including allocation of outputs and scratch and the read-back of the voxel count, device idle before and synchronised after,
median of --reps after --warmup.  The restatement runs ONCE on the same arrays.  There is no earlier device code to compare with: the
restatement beside it is the yardstick, and every device output is compared with it for equality of bits.  Recorded too: M, the
largest count, and -- for the fused room -- what the filter is for: scan.segment_cloud on the device over the uniform room, over the raw
fused cloud and over the fused cloud with voxel = step (radius 3 x step, K = 16, the defaults otherwise): segments, dropped points and
evaluate.merge_quality against the room's planes over the points that got a segment (a box's bottom face counted with the floor), with
the time of each route.  Synthetic boxes say nothing about real scans.  No threshold is set: what is measured is recorded.  Prints one
JSON line per cloud and writes them to --out."""
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
        if (g is None) != (w is None):
            return False
        if w is not None:
            g, w = np.ascontiguousarray(g.cpu().numpy()), np.ascontiguousarray(w)
            if g.dtype != w.dtype or g.shape != w.shape or g.tobytes() != w.tobytes():
                return False
    return True


def quality(out, plane):
    lab = out["instances"]
    plane = plane.copy()
    plane[(plane > 0) & ((plane - 1) % 6 == 4)] = 0                                # a box's bottom face lies in the floor
    use = (plane >= 0) & (lab > 0)
    q = EV.merge_quality(lab[use], plane[use])
    return {"segments": int(out["n_segments"]), "dropped_points": int((lab == 0).sum()), "precision": round(q["precision"], 6),
            "recall": round(q["recall"], 6)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxel", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "voxel_probe.txt"))
    a = ap.parse_args()
    dev, sync = "cuda:0", torch.cuda.synchronize
    fused_room = synth.make_box_mesh(12, 0.05, 3)
    big_room = synth.make_box_mesh(12, 0.017, 77)
    clouds = [("fused_room", synth.make_fused_cloud(fused_room["points"], seed=7)), ("uniform_room", big_room["points"])]
    lines = []
    for name, points in clouds:
        pts = np.ascontiguousarray(points, dtype=np.float32)
        g = np.random.default_rng(1)
        nrm = g.normal(0, 1, pts.shape).astype(np.float32)
        col = g.integers(0, 256, pts.shape).astype(np.uint8)
        d_p, d_n, d_c = (torch.from_numpy(x).to(dev) for x in (pts, nrm, col))
        row = {"probe": "voxel_downsample", "cloud": name, "points": len(pts), "voxel": a.voxel, "reps": a.reps,
               "lib_sha256": L.identity()["lib_sha256"][:16]}
        bare = prep.voxel_downsample(d_p, a.voxel)
        full = prep.voxel_downsample(d_p, a.voxel, normals=d_n, colors=d_c)
        row["voxels"], row["largest_count"] = len(bare.count), int(bare.count.max())
        row["ms_median"], row["ms_min"] = timed(lambda: prep.voxel_downsample(d_p, a.voxel), a.reps, a.warmup, sync)
        row["with_normals_colors_ms_median"], row["with_normals_colors_ms_min"] = timed(
            lambda: prep.voxel_downsample(d_p, a.voxel, normals=d_n, colors=d_c), a.reps, a.warmup, sync)
        h_bare, row["host_ms"] = once(lambda: prep.voxel_downsample_host(pts, a.voxel))
        h_full, row["with_normals_colors_host_ms"] = once(lambda: prep.voxel_downsample_host(pts, a.voxel, normals=nrm, colors=col))
        row["equals_host"] = bool(same(bare, h_bare) and same(full, h_full))
        again = prep.voxel_downsample(d_p, a.voxel, normals=d_n, colors=d_c)
        row["two_runs_equal"] = bool(same(again, [None if x is None else x.cpu().numpy() for x in full]))
        if name == "fused_room":
            step, plane = 0.05, fused_room["plane"]
            fused_plane = plane[synth.make_fused_index(fused_room["points"])]
            routes = {"uniform": (lambda: scan.segment_cloud({"points": fused_room["points"]}, 3 * step, k=16, device=dev), plane),
                      "fused_raw": (lambda: scan.segment_cloud({"points": points}, 3 * step, k=16, device=dev), fused_plane),
                      "fused_resampled": (lambda: scan.segment_cloud({"points": points}, 3 * step, k=16, device=dev, voxel=step), fused_plane)}
            for route, (fn, pl) in routes.items():
                out = fn()
                row[route] = quality(out, pl)
                row[route]["segment_cloud_ms_median"], _ = timed(fn, 5, 1, sync)
                if "resampled" in out:
                    row[route]["resampled_points"] = len(out["resampled"]["points"])
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
