#!/usr/bin/env python3
"""Cost of the zero-shot split in a one-scene-per-call validation loop: evaluate.validation(workers=K) on scenes of a fixed size,
with and without ``zero_shot`` (one extra launch per scene, vlsat_eval_triplet_split inside vlsat_process_val_counts_split).
Best of ``--reps`` timed passes per mode, modes interleaved, plans warm.  Prints one line per mode and a JSON record
(``--out``).  Under ``rocprofv3 --kernel-trace --stats`` the split kernel's own time shows as eval_triplet_split_kernel.

    python tools/zeroshot_probe.py [--scenes 120] [--objects 40] [--workers 1,4] [--out profiles/zeroshot_probe.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vlsat_amd  # noqa: E402
from vlsat_amd import VLSATConfig, synth, evaluate as EV  # noqa: E402
from vlsat_amd.model import VLSATModel  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=120)
    ap.add_argument("--objects", type=int, default=40)
    ap.add_argument("--points", type=int, default=256)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--workers", default="1,4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = "cuda:0"
    cfg = VLSATConfig(N_LAYERS=a.layers)
    model = VLSATModel(cfg, dev).load_state(synth.make_weights(cfg)).eval()
    g = np.random.default_rng(11)
    items = []
    for i in range(a.scenes):
        b = synth.collate([synth.make_scene(a.objects, a.points, seed=300 + i)])
        n, e = b["obj_points"].shape[0], b["edge_indices"].shape[1]
        it = {k: torch.from_numpy(v).to(dev) for k, v in b.items() if k != "edge_indices"}
        it.update(gt_class=torch.from_numpy(g.integers(0, 160, n)).to(dev),
                  gt_rel_cls=torch.from_numpy((g.random((e, 26)) < 0.04).astype(np.int64)).to(dev),
                  edge_indices=torch.from_numpy(b["edge_indices"]).t().contiguous().to(dev), fc_sizes=[n])
        items.append(it)
    table = torch.from_numpy((g.random(160 * 160 * 26) < 0.5).astype(np.uint8)).to(dev)
    modes = [(k, zs) for k in [int(x) for x in a.workers.split(",")] for zs in (False, True)]
    best = {m: 1e9 for m in modes}
    out = {}
    for m in modes:                                    # warm: plans, replicas, code objects
        out[m] = EV.validation(model, items, device=dev, workers=m[0], zero_shot=table if m[1] else None)
    for _ in range(a.reps):
        for m in modes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            EV.validation(model, items, device=dev, workers=m[0], zero_shot=table if m[1] else None)
            torch.cuda.synchronize()
            best[m] = min(best[m], time.perf_counter() - t0)
    rec = {"scenes": a.scenes, "objects": a.objects, "edges_per_scene": a.objects * (a.objects - 1), "layers": a.layers,
           "points": a.points, "reps": a.reps, "device": torch.cuda.get_device_name(0), "modes": []}
    print(f"{a.scenes} scenes x {a.objects} objects, L={a.layers}, one scene per call, best of {a.reps}")
    for k in sorted({m[0] for m in modes}):
        off, on = best[(k, False)], best[(k, True)]
        over = (on - off) / off * 100
        print(f"  workers={k}: {off / a.scenes * 1e3:7.3f} ms/scene without, {on / a.scenes * 1e3:7.3f} with zero_shot "
              f"({over:+.2f} %)   zero_shot_recall@100_3d = {out[(k, True)]['zero_shot_recall@100_3d']:.3f}")
        rec["modes"].append({"workers": k, "ms_per_scene": off / a.scenes * 1e3, "ms_per_scene_zero_shot": on / a.scenes * 1e3,
                             "overhead_pct": over})
        assert {q: out[(k, True)][q] for q in out[(k, False)]} == out[(k, False)]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    model.close()


if __name__ == "__main__":
    main()
