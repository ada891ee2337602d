"""Shared by test_split_cpu.py and test_hip_split.py: the three rules of include/vlsat_split.h written a second time as plain Python
loops -- seeds from ``math`` on Python floats, box membership per vertex, fusion through dictionaries and one np.float32 scalar operation
at a time -- the cases, and the comparisons.  No comparison uses a tolerance."""
import math

import numpy as np
import torch

F = np.float32
M64 = (1 << 64) - 1
FUSED_TABLES = ("root", "object", "n_objects", "totals", "member_ptr", "members", "obj_weight", "obj_batch_ids", "edge_to_pair", "pair_edges",
                "pair_count", "pair_probs", "obj_probs", "obj_ids")


def draw(seed, k, n):
    """splitmix64 of (seed, k), the top 32 bits scaled to n (include/vlsat.h, vlsat_sample_objects)."""
    z = (seed + 0x9E3779B97F4A7C15 * (k + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return ((z >> 32) * n) >> 32


def brute_seeds(points, distance=1.0, seed=0, ranks=None):
    """-> list of seed indices.  Python floats are fp64 and ``a * a + b * b`` rounds each operation on its own."""
    pts = [[float(c) for c in p] for p in np.asarray(points, dtype=F).tolist()]
    v = len(pts)
    finite = [all(math.isfinite(c) for c in p) for p in pts]
    take = (lambda k, n: ranks[k]) if ranks is not None else (lambda k, n: draw(seed, k, n))
    seeds = [int(take(0, v))]
    dmin2 = [math.nan] * v
    while True:
        sx, sy = pts[seeds[-1]][0], pts[seeds[-1]][1]
        for i, p in enumerate(pts):
            dx, dy = p[0] - sx, p[1] - sy
            d = dx * dx + dy * dy
            if len(seeds) == 1:
                dmin2[i] = d if finite[i] else math.nan
            elif d < dmin2[i]:
                dmin2[i] = d
        selectable = [i for i in range(v) if dmin2[i] > distance * distance]
        if not selectable:
            return seeds
        seeds.append(selectable[int(take(len(seeds), len(selectable)))])


def brute_groups(points, segments, segment_ids, seeds, bbox_distance=0.75, min_seg_per_group=5):
    """-> (groups as ascending id lists, counts, keep)."""
    pts = [[float(c) for c in p] for p in np.asarray(points, dtype=F).tolist()]
    seg = [int(s) for s in np.asarray(segments).tolist()]
    listed = set(int(i) for i in np.asarray(segment_ids).tolist())
    groups = []
    for sv in np.asarray(seeds).tolist():
        lo = [c - bbox_distance for c in pts[sv]]
        hi = [c + bbox_distance for c in pts[sv]]
        found = set()
        for p, s in zip(pts, seg):
            if s in listed and all(lo[a] < p[a] < hi[a] for a in range(3)):
                found.add(s)
        groups.append(sorted(found))
    counts = [len(g) for g in groups]
    return groups, counts, [c >= min_seg_per_group for c in counts]


def brute_fuse(c, map_size=1 << 24):
    """The fusion rule as loops -> dict of numpy tables, trimmed to M / E' rows."""
    probs, rp, edges = c["obj_probs"].numpy(), c["rel_probs"].numpy(), c["edges"].numpy().reshape(-1, 2).tolist()
    inst = [int(i) for i in np.asarray(c["row_instance"]).tolist()]
    n, k = probs.shape
    r = rp.shape[1]
    w = [F(1)] * n if c["weights"] is None else [F(x) for x in c["weights"].tolist()]
    rows_of = {}
    for i, ident in enumerate(inst):
        if 0 <= ident < map_size:
            rows_of.setdefault(ident, []).append(i)
    ids = sorted(rows_of)
    slot = {ident: m for m, ident in enumerate(ids)}
    obj = [slot.get(ident, -1) if 0 <= ident < map_size else -1 for ident in inst]
    root = [rows_of[ident][0] if o >= 0 else -1 for ident, o in zip(inst, obj)]
    m = len(ids)
    out_p, out_w = np.zeros((m, k), dtype=F), np.zeros(m, dtype=F)
    for o, ident in enumerate(ids):
        for i in rows_of[ident]:
            out_w[o] = F(out_w[o] + w[i])
        for col in range(k):
            s = F(0)
            for i in rows_of[ident]:
                s = F(s + F(w[i] * probs[i, col]))
            out_p[o, col] = F(s / out_w[o])
    pairs = {}
    for i, (a, b) in enumerate(edges):
        if not (0 <= a < n and 0 <= b < n) or obj[a] < 0 or obj[b] < 0 or obj[a] == obj[b]:
            continue
        p = pairs.setdefault((obj[a], obj[b]), [0, np.zeros(r, dtype=F), []])
        p[0] += 1
        p[1] = np.maximum(p[1], rp[i])
        p[2].append(i)
    keys = sorted(pairs)
    e2p = [-1] * len(edges)
    for q, key in enumerate(keys):
        for i in pairs[key][2]:
            e2p[i] = q
    members = [i for ident in ids for i in rows_of[ident]]
    members += [-1] * (n - len(members))
    return {"root": np.asarray(root, dtype=np.int64), "object": np.asarray(obj, dtype=np.int64), "n_objects": np.asarray([m]),
            "totals": np.asarray([m, len(keys)]), "member_ptr": np.cumsum([0] + [len(rows_of[i]) for i in ids]),
            "members": np.asarray(members, dtype=np.int64), "obj_probs": out_p, "obj_weight": out_w, "obj_batch_ids": np.zeros(m, dtype=np.int64),
            "obj_ids": np.asarray(ids, dtype=np.int64), "edge_to_pair": np.asarray(e2p, dtype=np.int64),
            "pair_edges": np.asarray(keys, dtype=np.int64).reshape(-1, 2), "pair_count": np.asarray([pairs[q][0] for q in keys], dtype=np.int64),
            "pair_probs": np.stack([pairs[q][1] for q in keys]) if keys else np.zeros((0, r), dtype=F)}


def assert_fused(got, want, what=""):
    """``got``: a FusedGraph (any device); ``want``: a FusedGraph or the dict of ``brute_fuse``.  Integers equal, floats bit for bit."""
    for k in FUSED_TABLES:
        a = getattr(got, k).cpu().numpy()
        b = want[k] if isinstance(want, dict) else getattr(want, k).cpu().numpy()
        assert a.shape == tuple(b.shape), (what, k, a.shape, b.shape)
        if a.dtype == np.float32:
            assert np.array_equal(a.view(np.uint32), np.asarray(b, dtype=F).view(np.uint32)), (what, k)
        else:
            assert np.array_equal(a.astype(np.int64), np.asarray(b).astype(np.int64)), (what, k)


def fuse_case(row_instance, edges, c=5, r=3, weights=None, seed=0):
    g = np.random.default_rng(seed)
    n = len(row_instance)
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    probs = g.random((n, c), dtype=F)
    probs = (probs / probs.sum(1, keepdims=True)).astype(F) if n else probs
    w = None
    if weights == "mixed":                                                      # point counts of very different magnitude
        w = torch.from_numpy(np.where(g.random(n) < 0.5, g.integers(1, 9, n), g.integers(20000, 3000000, n)).astype(F))
    elif weights is not None:
        w = torch.as_tensor(weights, dtype=torch.float32)
    return {"obj_probs": torch.from_numpy(probs), "rel_probs": torch.from_numpy(g.random((len(edges), r), dtype=F)),
            "edges": torch.from_numpy(edges), "row_instance": [int(i) for i in row_instance], "weights": w}


def random_splits(n_splits, n_ids, rows_per_split, n_edges, seed, ids=None, **kw):
    """``n_splits`` splits of ``rows_per_split`` rows, each a sample without replacement of ``n_ids`` scan-level ids (so an id recurs in
    several splits); ``n_edges`` random row pairs INSIDE a split, duplicates and self loops included, plus a few that are out of range."""
    g = np.random.default_rng(seed)
    ids = np.asarray(ids if ids is not None else g.choice(np.arange(0, 5000), n_ids, replace=False))
    inst, a, b = [], [], []
    for s in range(n_splits):
        inst.extend(g.choice(ids, rows_per_split, replace=False).tolist())
    per = n_edges // n_splits
    for s in range(n_splits):
        a.extend((s * rows_per_split + g.integers(0, rows_per_split, per)).tolist())
        b.extend((s * rows_per_split + g.integers(0, rows_per_split, per)).tolist())
    a += [-1, 0, len(inst)]
    b += [0, len(inst) + 3, 1]
    return fuse_case(inst, np.stack([a, b], 1), seed=seed, **kw)


def cloud(v, seed, extent=(4.0, 3.0, 2.5), ids=None):
    """``v`` vertices uniform in a box; the segment of a vertex is the cell of a coarse grid it lies in, mapped onto ``ids``."""
    g = np.random.default_rng(seed)
    pts = (g.random((v, 3)) * np.asarray(extent)).astype(F)
    ids = np.asarray(ids if ids is not None else [0] + list(range(1, 30)) + [4097, 4500, 4999, 5000, 4100, 4200, 4300])
    cell = (np.floor(pts[:, 0] / extent[0] * 7).astype(np.int64) * 6 + np.floor(pts[:, 1] / extent[1] * 6).astype(np.int64)) % len(ids)
    return pts, ids[cell].astype(np.int32)
