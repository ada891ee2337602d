#!/usr/bin/env python3
"""Proximity-pruned edge lists against the fully connected one, on rooms with spatial structure (synth.make_room): one room of 200
objects x 1024 points (the stress shape) and one of 40 objects x 256 points.  Per room: E fully connected and E at padding 0.2 with
max_neighbors 0 / 8 / 16; the time of boxes + count + fill (the host wait on the edge total included); and the forward per scene
in fp32 and bf16_mixed on every list -- same process, the lists taking turns inside each repetition, HIP events, medians
(tools/scene_graph_probe.py's method).  The fully connected list runs through its own fast path (fc_sizes); the pruned lists run
through the general-edge path (as does ``fc_nohint``, the fully connected list handed in without the hint).  No trained
checkpoint: the accuracy effect of pruning is not measured here.  Prints one JSON line per room."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vlsat_amd  # noqa: E402,F401
from vlsat_amd import VLSATConfig, prep, synth  # noqa: E402
from vlsat_amd.model import VLSATModel  # noqa: E402

from scene_graph_probe import interleaved  # noqa: E402


def room(n_obj, n_pts, seed, dev):
    pts, inst = synth.make_room(n_obj, n_pts, seed)
    d_pts, d_inst = torch.from_numpy(pts).to(dev), torch.from_numpy(inst).to(dev)
    ids = torch.arange(1, n_obj + 1, dtype=torch.int32, device=dev)
    choice, _ = prep.sample_objects(d_inst, ids, n_pts, seed)
    obj_points, desc = prep.prepare_objects(d_pts, choice)
    g = torch.Generator().manual_seed(seed)
    f2d = torch.nn.functional.normalize(torch.randn(n_obj, 512, generator=g), dim=-1).to(dev)
    return d_pts, d_inst, ids, obj_points, desc, f2d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--padding", type=float, default=0.2)
    a = ap.parse_args()
    dev = "cuda:0"
    cfg = VLSATConfig(N_LAYERS=3)
    w = synth.make_weights(cfg)
    models = {p: VLSATModel(cfg, dev).load_state(w).eval().set_gemm_precision(p) for p in ("fp32", "bf16_mixed")}
    for n_obj, n_pts in ((200, 1024), (40, 256)):
        d_pts, d_inst, ids, obj_points, desc, f2d = room(n_obj, n_pts, 31, dev)
        out = {"probe": "proximity", "objects": n_obj, "points_per_object": n_pts, "padding": a.padding, "reps": a.reps,
               "E_fully_connected": n_obj * (n_obj - 1)}
        lists = {"fc": prep.fc_edges([n_obj], dev)}
        lists["fc_nohint"] = tuple(t.clone() for t in lists["fc"])         # the same list without fc_sizes: what the plan makes of it
        for k in (0, 8, 16):
            def build(k=k):
                boxes = prep.instance_boxes(d_pts, d_inst, ids, n_obj + 1)
                return prep.proximity_edges(boxes, [n_obj], a.padding, k)
            e, bids, _ = build()
            lists[f"k{k}"] = (e, bids)
            deg = torch.bincount(e[0], minlength=n_obj)
            out[f"E_k{k}"], out[f"max_out_degree_k{k}"] = int(e.shape[1]), int(deg.max())
            out[f"isolated_nodes_k{k}"] = int((deg == 0).sum())
            out[f"boxes_count_fill_ms_k{k}"] = interleaved([build], 30)[0]
        for prec, m in models.items():
            def fwd(name):
                e, bids = lists[name]
                return lambda: m(obj_points, f2d, e, desc, bids, fc_sizes=[n_obj] if name == "fc" else None)
            names = list(lists)
            ts = interleaved([fwd(nm) for nm in names], a.reps, warm=2)
            for nm, t in zip(names, ts):
                out[f"forward_{prec}_ms_{nm}"] = t
                out[f"forward_{prec}_us_per_edge_{nm}"] = round(1e3 * t / lists[nm][0].shape[1], 4)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
