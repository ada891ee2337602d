#!/usr/bin/env python3
"""Time of the decoded scene graph (metrics.decode_graph -> vlsat_graph_decode) on the benchmark's batch shape -- 64 fully
connected scenes of 40 objects (E = 99 840), one branch, threshold 0.5, probabilities handed in, scratch and output allocation
included -- interleaved repetition by repetition with the top-K list in rels mode at topk_each = 26 on the same tensors
(tools/scene_graph_probe.py's method and batch).  Then, without a gate, VLSATModel.decode_graph (both branches, and 3D-only)
against forward / forward_3d alone on 40-object scenes, one call in flight.  Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vlsat_amd  # noqa: E402,F401
from vlsat_amd import metrics as M  # noqa: E402

from scene_graph_probe import interleaved  # noqa: E402


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
    obj, rel = (torch.randn(n, 160, generator=g) * 6).to(dev), torch.sigmoid(torch.randn(e, 26, generator=g) * 2).to(dev)
    probs = M.softmax_rows(obj)
    out = {"probe": "graph_decode", "scenes": a.scenes, "objects": a.objects, "edges": e, "reps": a.reps}
    topk = lambda: M.scene_graph_topk(obj, rel, edges, bid, a.scenes, True, 1024, 26, "rels", obj_probs=probs)
    for name, kw in (("rel_max1024", dict(score="rel", max_rel=1024)), ("triplet_max1024", dict(score="triplet", max_rel=1024)),
                     ("rel_max4096", dict(score="rel", max_rel=4096)), ("rel_thr0.9_max1024", dict(score="rel", max_rel=1024, threshold=0.9))):
        dec = lambda: M.decode_graph(obj, rel, edges, bid, a.scenes, True, obj_probs=probs, **dict(dict(threshold=0.5, n_labels=3), **kw))
        td, tt = interleaved([dec, topk], a.reps)
        out[f"decode_{name}_ms"], out[f"topk_rels_each26_top1024_ms__{name}"] = td, tt
    gph = M.decode_graph(obj, rel, edges, bid, a.scenes, True, 0.5, "rel", 3, 1024, obj_probs=probs)
    out["asserted_per_scene_at_0.5"] = round(float(gph.n_total.float().mean()), 1)

    # one 40-object scene per call, one in flight: forward alone and forward + decode in one library call
    from vlsat_amd import VLSATConfig, synth
    from vlsat_amd.model import VLSATModel
    cfg = VLSATConfig(N_LAYERS=3)
    model = VLSATModel(cfg, dev).load_state(synth.make_weights(cfg)).eval()
    scenes = []
    for s in range(a.forward_scenes):
        b = synth.collate([synth.make_scene(a.objects, 256, 7000 + s)])
        scenes.append({k: torch.from_numpy(v).to(dev) for k, v in b.items()})
    thr = float(model(scenes[0]["obj_points"], scenes[0]["obj_2d_feats"], scenes[0]["edge_indices"], scenes[0]["descriptor"],
                      scenes[0]["batch_ids"], fc_sizes=[a.objects])[2].median())      # synthetic weights: about half of the pairs pass

    def fwd():
        for b in scenes:
            model(b["obj_points"], b["obj_2d_feats"], b["edge_indices"], b["descriptor"], b["batch_ids"], fc_sizes=[a.objects])

    def dec():
        for b in scenes:
            model.decode_graph(b["obj_points"], b["obj_2d_feats"], b["edge_indices"], b["descriptor"], b["batch_ids"], threshold=thr,
                               fc_sizes=[a.objects])

    def fwd3():
        for b in scenes:
            model.forward_3d(b["obj_points"], b["edge_indices"], b["descriptor"], b["batch_ids"], fc_sizes=[a.objects])

    def dec3():
        for b in scenes:
            model.decode_graph(b["obj_points"], None, b["edge_indices"], b["descriptor"], b["batch_ids"], threshold=thr, fc_sizes=[a.objects])

    tf, td, tf3, td3 = interleaved([fwd, dec, fwd3, dec3], max(5, a.reps // 5), warm=2)
    k = len(scenes)
    out.update(forward_ms_per_scene=round(tf / k, 4), decode_graph_ms_per_scene=round(td / k, 4),
               decode_adds_ms_per_scene=round((td - tf) / k, 4), forward_3d_ms_per_scene=round(tf3 / k, 4),
               decode_graph_3d_ms_per_scene=round(td3 / k, 4), decode_3d_adds_ms_per_scene=round((td3 - tf3) / k, 4))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
