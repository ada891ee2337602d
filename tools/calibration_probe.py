#!/usr/bin/env python3
"""Time of metrics.score_histograms (vlsat_score_hist) next to ONE metrics.decode_counts call on the same tensors -- the comparator:
a histogram call stands in for `bins` of them.  Three cases: the 64-scene batch shape (E = 99 840, R = 26, N = 2 560), the
200-object scene (E = 39 800, N = 200), both with rand ** 4 scores (most near 0, as a trained multi-label head's) and 10 % hot cells,
and the worst case of the batch shape where every score is equal (every cell of a predicate on one counter).  Each at bins = 1024 and
4096.  Device time: wall clock around one call with the probabilities given and the tables / counts preallocated (tables= /
counts=: the accumulating form an evaluation loop uses), device idle before and synchronised after, median of --reps after --warmup.
Random inputs exercise the kernel; they say nothing about accuracy.  Prints one JSON line per case and writes them to --out."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vlsat_amd  # noqa: E402,F401
from vlsat_amd import lib as L, metrics as M  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out), min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "calibration_probe.txt"))
    a = ap.parse_args()
    dev, r, c = "cuda:0", 26, 160
    g = torch.Generator().manual_seed(0)
    lines = []
    for name, n, e, equal in (("batch_64x40", 2560, 99840, False), ("scene_200", 200, 39800, False), ("batch_64x40_all_equal", 2560, 99840, True)):
        rp = (torch.full((e, r), 0.3) if equal else torch.rand(e, r, generator=g) ** 4).to(dev)
        gt_rel = (torch.rand(e, r, generator=g) < 0.1).long().to(dev)
        probs = torch.softmax(torch.randn(n, c, generator=g) * 3, -1).to(dev)
        gt_cls = torch.randint(0, c, (n,), generator=g).to(dev)
        counts = torch.zeros(M.decode_counts_width(r), dtype=torch.int64, device=dev)
        dec = lambda: M.decode_counts(probs, rp, gt_cls, gt_rel, True, 0.5, obj_probs=probs, rel_probs=rp, counts=counts)
        row = {"probe": "score_histograms", "case": name, "nodes": n, "edges": e, "predicates": r, "reps": a.reps,
               "lib_sha256": L.identity()["lib_sha256"][:16]}
        row["decode_counts_ms_median"], row["decode_counts_ms_min"] = (round(x, 4) for x in timed(dec, a.reps, a.warmup))
        for bins in (1024, 4096):
            t = M.ScoreTables(r, c, bins, dev)
            hist = lambda: M.score_histograms(probs, rp, gt_cls, gt_rel, True, bins, obj_probs=probs, rel_probs=rp, tables=t)
            fresh = M.score_histograms(probs, rp, gt_cls, gt_rel, True, bins, obj_probs=probs, rel_probs=rp)
            one = M.decode_counts(probs, rp, gt_cls, gt_rel, True, 0.5, obj_probs=probs, rel_probs=rp)
            row[f"bins{bins}_counts_equal_decode_counts"] = bool(torch.equal(fresh.counts_at(bins // 2), one[:3 * r]))
            med, low = timed(hist, a.reps, a.warmup)
            row[f"bins{bins}_ms_median"], row[f"bins{bins}_ms_min"] = round(med, 4), round(low, 4)
            row[f"bins{bins}_over_one_decode_counts"] = round(med / row["decode_counts_ms_median"], 2)
            row[f"bins{bins}_sweep_of_decode_counts_over_hist"] = round(bins * row["decode_counts_ms_median"] / med, 1)
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
