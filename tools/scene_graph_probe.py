#!/usr/bin/env python3
"""Time of the predicted scene graph (metrics.scene_graph_topk -> vlsat_scene_graph_topk) on the benchmark's batch shape -- 64
fully connected scenes of 40 objects (E = 99 840), one branch, top_k = 100, object softmax and scratch allocation included
-- next to the Recall@K call of the matching variant on the same inputs (tools/recallk_probe.py's method and batch;
eval_recall.hip does the same per-edge selection on 32-bit keys), the two interleaved repetition by repetition.  Then, without
a gate, VLSATModel.predict_graph against forward alone on 40-object scenes, one call in flight.  Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vlsat_amd  # noqa: E402,F401
from vlsat_amd import metrics as M  # noqa: E402


def interleaved(fns, reps, warm=5):
    """Median ms of every function, the functions taking turns inside each repetition (HIP events)."""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            ts[k].append(t0.elapsed_time(t1))
    return [round(sorted(t)[len(t) // 2], 4) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=64)
    ap.add_argument("--objects", type=int, default=40)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--forward-scenes", type=int, default=40)
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
    obj, rel = (torch.randn(n, 160, generator=g) * 6).to(dev), torch.sigmoid(torch.randn(e, 26, generator=g) * 2).to(dev)
    out = {"probe": "scene_graph", "scenes": a.scenes, "objects": a.objects, "edges": e, "reps": a.reps, "top_k": 100}
    for each, variant in ((100, "sgcls_ngc"), (1, "sgcls_gc")):
        graph = lambda: M.scene_graph_topk(obj, rel, edges, bid, a.scenes, True, 100, each, "triplet")
        recall = lambda: M.recallk_counts(obj, rel, gt_cls, gt_rel, edges, bid, a.scenes, True, variants=(variant,))
        tg, tr = interleaved([graph, recall], a.reps)
        out[f"triplet_each{each}_ms"], out[f"{variant}_one_branch_ms"], out[f"triplet_each{each}_ratio"] = tg, tr, round(tg / tr, 3)
    out["rels_each100_ms"] = interleaved([lambda: M.scene_graph_topk(obj, rel, edges, bid, a.scenes, True, 100, 100, "rels")], a.reps)[0]
    out["triplet_each100_top1024_ms"] = interleaved(
        [lambda: M.scene_graph_topk(obj, rel, edges, bid, a.scenes, True, 1024, 100, "triplet")], a.reps)[0]

    # one 40-object scene per call, one in flight: forward alone and forward + graph of both branches in one library call
    from vlsat_amd import VLSATConfig, synth
    from vlsat_amd.model import VLSATModel
    cfg = VLSATConfig(N_LAYERS=3)
    model = VLSATModel(cfg, dev).load_state(synth.make_weights(cfg)).eval()
    scenes = []
    for s in range(a.forward_scenes):
        b = synth.collate([synth.make_scene(a.objects, 256, 7000 + s)])
        scenes.append({k: torch.from_numpy(v).to(dev) for k, v in b.items()})

    def fwd():
        for b in scenes:
            model(b["obj_points"], b["obj_2d_feats"], b["edge_indices"], b["descriptor"], b["batch_ids"], fc_sizes=[a.objects])

    def pred():
        for b in scenes:
            model.predict_graph(b["obj_points"], b["obj_2d_feats"], b["edge_indices"], b["descriptor"], b["batch_ids"],
                                fc_sizes=[a.objects])

    tf, tp = interleaved([fwd, pred], max(5, a.reps // 5), warm=2)
    out.update(forward_ms_per_scene=round(tf / len(scenes), 4), predict_graph_ms_per_scene=round(tp / len(scenes), 4),
               graph_adds_ms_per_scene=round((tp - tf) / len(scenes), 4))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
