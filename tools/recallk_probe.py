#!/usr/bin/env python3
"""Time of the scene-graph Recall@K counts (metrics.recallk_counts -> vlsat_eval_recallk) on the benchmark's batch shape:
64 fully connected scenes of 40 objects (E = 99 840), all four variants (PredCls / SGCls, GC / NGC) on both branches, i.e.
two library calls per batch, with the object softmax and the scratch allocation included.  Prints one JSON line
(median / min of the timed repetitions, ms per batch, and each variant alone on one branch)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vlsat_amd  # noqa: E402,F401
from vlsat_amd import metrics as M  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=64)
    ap.add_argument("--objects", type=int, default=40)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    dev = "cuda:0"
    g = torch.Generator().manual_seed(5)
    n = a.scenes * a.objects
    ei = [(s * a.objects + i, s * a.objects + j) for s in range(a.scenes) for i in range(a.objects) for j in range(a.objects) if i != j]
    edges = torch.tensor(ei, dtype=torch.int64, device=dev)
    e = edges.shape[0]
    bid = torch.arange(a.scenes).repeat_interleave(a.objects).to(dev)
    gt_cls = torch.randint(0, 160, (n,), generator=g).to(dev)
    gt_rel = (torch.rand(e, 26, generator=g) < 0.05).long().to(dev)
    branches = [((torch.randn(n, 160, generator=g) * 6).to(dev), torch.sigmoid(torch.randn(e, 26, generator=g) * 2).to(dev))
                for _ in range(2)]

    def run(variants=M.RECALL_VARIANTS, brs=branches):
        for obj, rel in brs:
            M.recallk_counts(obj, rel, gt_cls, gt_rel, edges, bid, a.scenes, True, variants=variants)

    def timed(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            ts.append(t0.elapsed_time(t1))
        ts.sort()
        return round(ts[len(ts) // 2], 4), round(ts[0], 4)

    med, best = timed(run)
    out = {"probe": "recallk", "scenes": a.scenes, "objects": a.objects, "edges": e, "reps": a.reps,
           "all_variants_both_branches_ms": med, "min_ms": best}
    for v in M.RECALL_VARIANTS:
        out[f"{v}_one_branch_ms"] = timed(lambda: run((v,), branches[:1]))[0]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
