#!/usr/bin/env python3
"""Per-launch table of the matrix kernels (GEMMs, attention, LayerNorm, edge gate and its aggregation launches) of one forward from two SERIAL kernel traces (`rocprofv3 --kernel-trace --stats -d DIR -o NAME --
python bench.py ... --no-profile --debug-option dual_stream=0`, one per build; rocpd databases), side by side: the launches of a
forward in stream order, each averaged over the traced forwards after the first two.  Both builds launch the same sequence, so row i
is the same stage in both (profiles/edge_pairs_ab.txt).

    python tools/launch_table.py parent_results.db new_results.db
"""
import re, sqlite3, sys

def launches(db):
    c = sqlite3.connect(db)
    cols = [r[1] for r in c.execute("pragma table_info(kernels)")]
    start = "start" if "start" in cols else [x for x in cols if "start" in x][0]
    rows = list(c.execute(f"select name, duration, grid_x / workgroup_x from kernels order by {start}"))
    fw, cur = [], None
    for name, dur, blocks in rows:
        if "pointnet" in name:
            cur = []
            fw.append(cur)
        if cur is not None and ("gemm_" in name or "flash_" in name or "layernorm" in name or "edge_gate" in name or "agg" in name):
            m = re.search(r"(gemm_\w+|flash_\w+|layernorm\w*|edge_gate\w*|agg\w*)(<[^>]*>)?", name)
            cur.append(((m.group(1) + (m.group(2) or "")) if m else name[:60], blocks, dur))
    fw = [f for f in fw if len(f) == len(fw[-1])][2:]           # drop the warm-up forwards
    out = []
    for i in range(len(fw[0])):
        out.append((fw[0][i][0], fw[0][i][1], sum(f[i][2] for f in fw) / len(fw) / 1e3))
    return out, len(fw)

a, na = launches(sys.argv[1])
b, nb = launches(sys.argv[2])
print(f"forwards averaged: {na} / {nb}; launches per forward: {len(a)} / {len(b)}")
assert len(a) == len(b)
ta = tb = 0.0
for i, (x, y) in enumerate(zip(a, b)):
    big = "p8s" in x[0] or "flash" in x[0] or "gate" in x[0] or "agg" in x[0] or x[2] > 15
    if big:
        print(f"{i:4d}  {x[0]:50s} {x[1]:5d} {x[2]:8.1f}   {y[0]:50s} {y[2]:8.1f}  {y[2] - x[2]:+7.1f}")
    ta += x[2]; tb += y[2]
print(f"sum of all gemm / flash / layernorm / gate / aggregation launches per forward: {ta / 1e3:.3f} ms -> {tb / 1e3:.3f} ms")
