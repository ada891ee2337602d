#!/usr/bin/env python3
"""Largest |A| the split-fp16 kernels of the fp32 mode see, from the CPU oracle (no GPU): the inputs of PointNet's conv2 / conv3 (H1, H2),
of the Linears on node rows, of the Linears on edge rows and of the two layers of the edge gate (its kproj rows KP and its hidden vector) -- on the bench weights and on the x 3 / x 4 stress weights, three scenes of
40 objects x 256 points.  The operand domain is +-65504 (beyond it the operand saturates).

    python tools/f16s_domain.py
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "cvpr2023-vlsat_amd"))

import vlsat_amd  # noqa: E402,F401
from vlsat_amd import VLSATConfig, synth  # noqa: E402
from oracle import vlsat_oracle as O  # noqa: E402


def main():
    cfg = VLSATConfig(N_LAYERS=3)
    n_obj, scenes = 40, 3
    b = {k: torch.from_numpy(v) for k, v in synth.collate([synth.make_scene(n_obj, 256, 1000 + s) for s in range(scenes)]).items()}
    n_nodes, n_edges = n_obj * scenes, b["edge_indices"].shape[1]
    inner = O.lin
    for label, w in (("bench weights", synth.make_weights(cfg)), ("stress x 3", synth.make_weights_stress(cfg, 3.0)),
                     ("stress x 4", synth.make_weights_stress(cfg, 4.0))):
        seen = {}

        def lin(x, wt, name):
            rows = x.reshape(-1, x.shape[-1]).shape[0]
            per_scene = {n_obj: "node rows", n_obj * (n_obj - 1): "edge rows", n_obj * 256: "point rows"}
            cls = ("PointNet H1" if name.endswith("obj_encoder.conv2") else "PointNet H2" if name.endswith("obj_encoder.conv3") else
                   per_scene.get(rows) or {n_nodes: "node rows", n_edges: "edge rows", n_nodes * 256: "point rows"}.get(rows, f"{rows} rows"))
            v = float(x.abs().max())
            if v > seen.get(cls, (0.0, ""))[0]:
                seen[cls] = (v, name)
            return inner(x, wt, name)

        inner_gate = O.edge_atten

        def edge_atten(x, e, ei, wt, prefix, n_heads, taps=None):
            # the operands of the gate's two layers (edge_gate_f16s.hip): KP = proj_edge(e), hidden = relu(nn.0([q | k]) + b0)
            p = prefix + ".edgeatten."
            xi, _ = O.gen_index(x, ei, "target_to_source")
            E = e.shape[0]
            q = inner(xi, wt, p + "proj_query.0")
            k = inner(e, wt, p + "proj_edge.0")
            q, k = q.view(E, q.shape[1] // n_heads, n_heads), k.view(E, k.shape[1] // n_heads, n_heads)
            w0, b0 = wt[p + "nn.0.weight"][:, :, 0], wt[p + "nn.0.bias"]
            z = torch.cat([q, k], 1) if w0.shape[1] == q.shape[1] + k.shape[1] else q
            hid = torch.relu(torch.einsum("oc,ech->eoh", w0, z) + b0[None, :, None])
            for cls, v in (("gate KP", float(k.abs().max())), ("gate hidden", float(hid.max()))):
                if v > seen.get(cls, (0.0, ""))[0]:
                    seen[cls] = (v, prefix)
            return inner_gate(x, e, ei, wt, prefix, n_heads, taps)

        O.lin = lin
        O.edge_atten = edge_atten
        try:
            O.forward(O.to_torch(w, torch.float32), cfg, b["obj_points"], b["obj_2d_feats"], b["edge_indices"], b["descriptor"], b["batch_ids"])
        finally:
            O.lin = inner
            O.edge_atten = inner_gate
        print(label + ": " + "; ".join(f"{c} {v:.4g} ({n})" for c, (v, n) in sorted(seen.items())))


if __name__ == "__main__":
    main()
