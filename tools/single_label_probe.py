#!/usr/bin/env python3
"""evaluate.validation of a SINGLE-LABEL model (MODEL.multi_rel_outputs = false, 27 relation classes), one scene per item, on this build
beside the parent commit's library on the same box: the "one scene per call" workload of tools/validation_3d_probe.py (synthetic scenes
of 9..80 objects, every scene a different graph; forward + ranking + counts per scene) at 1, 2 and 4 scenes in flight and with 16 items
collated per call, two-branch and use_2d=False, in fp32 and bf16_mixed.  The multi-label loop (26 classes, two-branch) is timed beside
it in the same runs: its path did not change, so its pair shows what the box's own spread is.

A process loads one library.  The two builds are therefore timed in interleaved PAIRS OF PROCESSES: round r starts a worker on the
parent's library, then one on this tree's; each worker builds the scenes, and for every configuration runs one warm-up pass (plans,
replicas, allocator, code objects) and one timed pass that starts with the device idle and ends with a synchronise.  The figure of a
configuration is the median over the rounds; `spread` is min..max of the rounds, `pairs` the min..max of the per-round ratio.

The parent's library refuses the one call for a single-label model, and the parent's metrics.process_val_counts never tried it: it
took forward + 2 rank_tables (two vlsat_eval_ranks passes each, an exp between them) + eval_counts.  On the parent's library the
worker takes exactly that route (--separate: the model's process_val_counts answers False for a single-label model, as a permuted
plan does), on this tree's library the one call.  A worker stops at the first failure and the driver starts nothing after it.

    python tools/single_label_probe.py --parent-lib OTHER/libvlsat_hip.so [--scenes 120] [--rounds 7] [--out profiles/single_label_probe.txt]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def configs(a):
    out = []
    for prec in a.precisions.split(","):
        for setting in a.settings.split(","):
            workers, merge = (int(x) for x in setting.split(":"))
            out += [("single", prec, workers, merge, True), ("single", prec, workers, merge, False), ("multi", prec, workers, merge, True)]
    return out


def name(c):
    return f"{c[0]}|{c[1]}|{c[2]}|{c[3]}|{int(c[4])}"


def worker(a):
    import numpy as np
    import torch
    import vlsat_amd  # noqa: F401
    from vlsat_amd import VLSATConfig, synth, evaluate as EV, lib as L
    if not torch.cuda.is_available():
        sys.exit("single_label_probe: no GPU visible; nothing is measured without one")
    if a.lib:
        L.LIB_PATH = os.path.abspath(a.lib)
    from vlsat_amd.model import VLSATModel
    dev = "cuda:0"
    lo, hi = ([int(x) for x in a.objects.split(",")] * 2)[:2]
    sizes = np.random.default_rng(5).integers(lo, hi + 1, a.scenes)
    items = {"single": [], "multi": []}
    for i, n in enumerate(sizes):
        b = synth.collate([synth.make_scene(int(n), a.points, seed=100 + i)])
        e = b["edge_indices"].shape[1]
        g = np.random.default_rng([int(n), e, 7])
        it = {k: torch.from_numpy(v).to(dev) for k, v in b.items() if k != "edge_indices"}
        it.update(gt_class=torch.from_numpy(g.integers(0, 160, int(n))).to(dev),
                  edge_indices=torch.from_numpy(b["edge_indices"]).t().contiguous().to(dev), fc_sizes=[int(n)])
        multi = torch.from_numpy((g.random((e, 26)) < 0.04).astype(np.int64)).to(dev)
        labels = g.integers(1, 27, e)
        labels[g.random(e) < 0.5] = 0                                     # half of the edges 'none'
        items["multi"].append(dict(it, gt_rel_cls=multi))
        items["single"].append(dict(it, gt_rel_cls=torch.from_numpy(labels).to(dev)))

    class SeparateCalls(VLSATModel):                                      # the parent's route for a single-label model
        def process_val_counts(self, *args, **kw):
            return False

        def replicas(self, k):
            reps = super().replicas(k)
            for r in reps:
                r.__class__ = SeparateCalls
            return reps

    times, summaries = {}, {}
    models = {}
    for c in configs(a):
        kind, prec, workers, merge, use_2d = c
        if (kind, prec) not in models:
            if any(p != prec for _, p in models):                         # (both models of a precision stay alive, with their replicas and plans)
                for m in models.values():
                    m.close()
                models.clear()
            cfg = VLSATConfig(N_LAYERS=a.layers) if kind == "multi" else VLSATConfig(N_LAYERS=a.layers, multi_rel_outputs=False, num_rel_class=27)
            cls = SeparateCalls if (kind == "single" and a.separate) else VLSATModel
            models[(kind, prec)] = cls(cfg, dev).load_state(synth.make_weights(cfg)).eval().set_gemm_precision(prec)
        model = models[(kind, prec)]
        run = lambda: EV.validation(model, items[kind], device=dev, workers=workers, merge=merge, use_2d=use_2d)
        summaries[name(c)] = run()                                        # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        times[name(c)] = time.perf_counter() - t0
    for m in models.values():
        m.close()
    ident = L.identity(L.LIB_PATH)
    print("RESULT " + json.dumps({"times": times, "summaries": summaries, "lib": os.path.relpath(L.LIB_PATH, ROOT), "lib_sha256": ident["lib_sha256"],
                                  "source_sha256": ident["source_sha256"], "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
                                  "mean_objects": float(sizes.mean())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=120)
    ap.add_argument("--points", type=int, default=256)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--objects", default="9,80")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--precisions", default="fp32,bf16_mixed")
    ap.add_argument("--settings", default="1:1,2:1,4:1,2:16", help="workers:merge pairs")
    ap.add_argument("--parent-lib", default="", help="the parent commit's build of the library")
    ap.add_argument("--timeout", type=int, default=240, help="seconds a worker process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "single_label_probe.txt"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--lib", default="", help=argparse.SUPPRESS)
    ap.add_argument("--separate", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("single_label_probe: --parent-lib, the parent commit's libvlsat_hip.so, is required")
    common = [sys.executable, os.path.abspath(__file__), "--worker", "--scenes", str(a.scenes), "--points", str(a.points), "--layers", str(a.layers),
              "--objects", a.objects, "--precisions", a.precisions, "--settings", a.settings]
    builds = {"parent": common + ["--lib", os.path.abspath(a.parent_lib), "--separate"], "this": common}
    res = {b: [] for b in builds}
    for r in range(a.rounds):
        for b, cmd in builds.items():
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
            if p.returncode or not line:                                  # stop here: nothing more is started on the device
                sys.exit(f"single_label_probe: worker [{b}] of round {r} failed with status {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
            res[b].append(json.loads(line[0][7:]))
            print(f"round {r} [{b}] done", flush=True)
    first = {b: res[b][0] for b in builds}
    # the two builds count the same: every summary of every configuration equal, NaN = NaN
    same = lambda x, y: x == y or (x != x and y != y)
    for key, s in first["this"]["summaries"].items():
        p = first["parent"]["summaries"][key]
        bad = [k for k in s if not same(s[k], p[k])]
        if list(s) != list(p) or bad:
            sys.exit(f"single_label_probe: {key}: the summaries of the two builds differ: {bad[:8]}")
    lines = [f"# single_label_probe: {a.scenes} scenes of {a.objects.replace(',', '..')} objects (mean {first['this']['mean_objects']:.1f}) x {a.points} points, "
             f"L={a.layers}, fc_sizes hint; {a.rounds} interleaved pairs of processes (parent, this tree), each one warm-up pass and one timed pass per row; "
             "median, scenes/s",
             "# single: multi_rel_outputs = false, 27 classes, half of the edges 'none'; parent = its library on the separate calls (what it ran), "
             "this tree = the one call.  multi: 26 classes, the one call on both (the path did not change: its pair is the box's spread)",
             "# every summary of every row is equal between the two builds"]
    for b in builds:                                                      # (the source digest is this tree's: it says nothing about the parent's library)
        lines.append(f"# {b}: library {first[b]['lib']} lib_sha256 {first[b]['lib_sha256']}" + (f" source_sha256 {first[b]['source_sha256']}" if b == "this" else ""))
    lines.append(f"# device {first['this']['device']}; torch {first['this']['torch']}")
    lines.append(f"{'model':<7} {'precision':<11} {'workers':>7} {'merge':>5} {'use_2d':>6} {'parent':>9} {'this tree':>10} {'ratio':>6}   "
                 "spread (min..max scenes/s): parent | this tree | pairs (ratio min..max)")
    for c in configs(a):
        k = name(c)
        t = {b: [x["times"][k] for x in res[b]] for b in builds}
        rate = {b: a.scenes / statistics.median(t[b]) for b in builds}
        spread = {b: f"{a.scenes / max(t[b]):.0f}..{a.scenes / min(t[b]):.0f}" for b in builds}
        ratios = [p / q for p, q in zip(t["parent"], t["this"])]
        lines.append(f"{c[0]:<7} {c[1]:<11} {c[2]:>7} {c[3]:>5} {str(c[4]):>6} {rate['parent']:>9.1f} {rate['this']:>10.1f} {rate['this'] / rate['parent']:>6.2f}   "
                     f"{spread['parent']} | {spread['this']} | {min(ratios):.2f}..{max(ratios):.2f}")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
