#!/usr/bin/env python3
"""evaluate.validation(use_2d=False) beside use_2d=True, one scene per item: the README's "one scene per call" workload (synthetic
scenes of 9..80 objects, every scene a different graph; forward + ranking + counts per scene) at 1, 2 and 4 scenes in flight and with
16 items collated per call, in fp32 and bf16_mixed.  The two loops are timed in interleaved pairs (full, 3D-only, full, ...) after a
warm-up pass of each; a pass starts with the device idle and ends with a synchronise; the figure is the median of the repeats.
The use_2d=True column is the baseline -- that path is what it was -- and the 3D values of the two summaries must be equal.

    python tools/validation_3d_probe.py [--scenes 120] [--repeats 7] [--out profiles/validation_3d_probe.txt]
    python tools/validation_3d_probe.py --lib OTHER/libvlsat_hip.so --full-only --label parent --append     another build, same box:
                                                                                                            the full loop only"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vlsat_amd  # noqa: E402,F401
from vlsat_amd import VLSATConfig, synth, evaluate as EV, lib as L  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=120)
    ap.add_argument("--points", type=int, default=256)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--objects", default="9,80")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--precisions", default="fp32,bf16_mixed")
    ap.add_argument("--settings", default="1:1,2:1,4:1,2:16", help="workers:merge pairs")
    ap.add_argument("--lib", default="", help="another build of the library (same-box A/B)")
    ap.add_argument("--full-only", action="store_true", help="time use_2d=True only (a build from before the 3D-only loops)")
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "validation_3d_probe.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("validation_3d_probe: no GPU visible; nothing is measured without one")
    if a.lib:
        L.LIB_PATH = os.path.abspath(a.lib)
    from vlsat_amd.model import VLSATModel
    dev = "cuda:0"
    cfg = VLSATConfig(N_LAYERS=a.layers)
    weights = synth.make_weights(cfg)
    lo, hi = ([int(x) for x in a.objects.split(",")] * 2)[:2]
    sizes = np.random.default_rng(5).integers(lo, hi + 1, a.scenes)
    items = []
    for i, n in enumerate(sizes):
        b = synth.collate([synth.make_scene(int(n), a.points, seed=100 + i)])
        e = b["edge_indices"].shape[1]
        g = np.random.default_rng([int(n), e, 7])
        it = {k: torch.from_numpy(v).to(dev) for k, v in b.items() if k != "edge_indices"}
        it.update(gt_class=torch.from_numpy(g.integers(0, 160, int(n))).to(dev),
                  gt_rel_cls=torch.from_numpy((g.random((e, 26)) < 0.04).astype(np.int64)).to(dev),
                  edge_indices=torch.from_numpy(b["edge_indices"]).t().contiguous().to(dev), fc_sizes=[int(n)])
        items.append(it)
    ident = L.identity(L.LIB_PATH)
    lines = [f"# validation_3d_probe [{a.label}]: {a.scenes} scenes of {lo}..{hi} objects (mean {sizes.mean():.1f}) x {a.points} points, L={a.layers}, "
             f"fc_sizes hint; one warm-up pass per loop, then {a.repeats} interleaved pairs, median; scenes/s",
             f"# library {os.path.relpath(L.LIB_PATH, ROOT)} lib_sha256 {ident['lib_sha256']} source_sha256 {ident['source_sha256']}",
             f"# device {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
             f"{'precision':<11} {'workers':>7} {'merge':>5} {'use_2d=True':>12} {'use_2d=False':>13} {'ratio':>6}   spread of the repeats (min..max scenes/s): full | 3D-only"]
    flags = (True,) if a.full_only else (True, False)
    for prec in a.precisions.split(","):
        model = VLSATModel(cfg, dev).load_state(weights).eval().set_gemm_precision(prec)
        for setting in a.settings.split(","):
            workers, merge = (int(x) for x in setting.split(":"))
            run = lambda use_2d: (EV.validation(model, items, device=dev, workers=workers, merge=merge, use_2d=use_2d) if not a.full_only
                                  else EV.validation(model, items, device=dev, workers=workers, merge=merge))
            out = {f: run(f) for f in flags}                       # warm-up: plans, replicas, allocator, code objects
            if not a.full_only:
                same = {k: out[False][k] == out[True][k] for k in out[False]}
                assert all(same.values()) and set(out[False]) == {k for k in out[True] if not k.endswith("_2d")}, \
                    ("3D values differ", [k for k, v in same.items() if not v][:8])
            times = {f: [] for f in flags}
            for _ in range(a.repeats):
                for f in flags:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    run(f)
                    torch.cuda.synchronize()
                    times[f].append(time.perf_counter() - t0)
            rate = {f: a.scenes / statistics.median(times[f]) for f in flags}
            spread = {f: f"{a.scenes / max(times[f]):.0f}..{a.scenes / min(times[f]):.0f}" for f in flags}
            if a.full_only:
                lines.append(f"{prec:<11} {workers:>7} {merge:>5} {rate[True]:>12.1f} {'-':>13} {'-':>6}   {spread[True]}")
            else:
                lines.append(f"{prec:<11} {workers:>7} {merge:>5} {rate[True]:>12.1f} {rate[False]:>13.1f} {rate[False] / rate[True]:>6.2f}   "
                             f"{spread[True]} | {spread[False]}")
            print(lines[-1], flush=True)
        model.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
