"""Shared by test_segment_merge_cpu.py and test_hip_segment_merge.py: the merge rule of include/vlsat.h (vlsat_merge_segments) written
a second time as plain Python -- breadth-first search over the link set, a dictionary of pairs, one np.float32 scalar operation at a
time -- the cases, and the comparison.  No comparison uses a tolerance."""
from collections import deque

import numpy as np
import torch

F = np.float32
TABLES = ("root", "object", "n_objects", "totals", "member_ptr", "members", "obj_weight", "obj_batch_ids", "edge_to_pair", "pair_edges",
          "pair_count", "pair_probs", "obj_probs")


def brute(c):
    """The rule as loops -> dict of numpy tables, trimmed to M / E' rows."""
    probs, rp, edges = c["obj_probs"].numpy(), c["rel_probs"].numpy(), c["edges"].numpy().reshape(-1, 2).tolist()
    n, k = probs.shape
    e, r = rp.shape
    bid = [0] * n if c["batch_ids"] is None else c["batch_ids"].tolist()
    w = [F(1)] * n if c["weights"] is None else [F(x) for x in c["weights"].tolist()]
    thr, sp = F(c["threshold"]), c["same_part"]
    ok = [a != b and bid[a] == bid[b] for a, b in edges]
    passed = {(a, b) for i, (a, b) in enumerate(edges) if ok[i] and rp[i, sp] >= thr}
    links = {(a, b) for a, b in passed if not c["mutual"] or (b, a) in passed}
    nb = [[] for _ in range(n)]
    for a, b in links:
        nb[a].append(b)
        nb[b].append(a)
    root = [-1] * n
    for start in range(n):                                                      # ascending: the first row of a component is its root
        if root[start] >= 0:
            continue
        root[start], todo = start, deque([start])
        while todo:
            for y in nb[todo.popleft()]:
                if root[y] < 0:
                    root[y] = start
                    todo.append(y)
    roots = sorted(set(root))
    number = {x: i for i, x in enumerate(roots)}
    obj = [number[x] for x in root]
    m = len(roots)
    groups = [[i for i in range(n) if obj[i] == o] for o in range(m)]
    out_p, out_w = np.zeros((m, k), dtype=F), np.zeros(m, dtype=F)
    for o, g in enumerate(groups):
        for i in g:
            out_w[o] = F(out_w[o] + w[i])
        for col in range(k):
            s = F(0)
            for i in g:
                s = F(s + F(w[i] * probs[i, col]))
            out_p[o, col] = F(s / out_w[o])
    pairs, e2p = {}, []
    for i, (a, b) in enumerate(edges):
        if not ok[i] or obj[a] == obj[b]:
            e2p.append(-1)
            continue
        key = (obj[a], obj[b])
        if key not in pairs:                                                    # rows ascend: first seen = lowest contributing row
            pairs[key] = [len(pairs), 0, np.zeros(r, dtype=F)]
        p = pairs[key]
        p[1] += 1
        p[2] = np.maximum(p[2], rp[i])
        e2p.append(p[0])
    n_scenes = c["n_scenes"]
    member_ptr = np.cumsum([0] + [len(g) for g in groups])
    return {"root": np.asarray(root, dtype=np.int64), "object": np.asarray(obj, dtype=np.int64),
            "n_objects": np.asarray([sum(bid[x] == s for x in roots) for s in range(n_scenes)], dtype=np.int64),
            "totals": np.asarray([m, len(pairs)]), "member_ptr": member_ptr, "members": np.asarray([i for g in groups for i in g], dtype=np.int64),
            "obj_probs": out_p, "obj_weight": out_w, "obj_batch_ids": np.asarray([bid[x] for x in roots], dtype=np.int64),
            "edge_to_pair": np.asarray(e2p, dtype=np.int64), "pair_edges": np.asarray(list(pairs), dtype=np.int64).reshape(-1, 2),
            "pair_count": np.asarray([p[1] for p in pairs.values()], dtype=np.int64),
            "pair_probs": np.stack([p[2] for p in pairs.values()]) if pairs else np.zeros((0, r), dtype=F)}


def assert_tables(got, want, what=""):
    """``got``: a MergedGraph (any device); ``want``: a MergedGraph or the dict of ``brute``.  Integers equal, floats bit for bit."""
    for k in TABLES:
        a = getattr(got, k).cpu().numpy()
        b = want[k] if isinstance(want, dict) else getattr(want, k).cpu().numpy()
        assert a.shape == tuple(b.shape), (what, k, a.shape, b.shape)
        if a.dtype == np.float32:
            assert np.array_equal(a.view(np.uint32), np.asarray(b, dtype=F).view(np.uint32)), (what, k)
        else:
            assert np.array_equal(a.astype(np.int64), np.asarray(b).astype(np.int64)), (what, k)


def _case(n, edges, link_prob, c=5, r=3, same_part=1, threshold=0.5, mutual=False, batch_ids=None, n_scenes=1, weights=None, seed=0):
    """``link_prob[e]`` goes into column same_part; the other entries are random probabilities."""
    g = np.random.default_rng(seed)
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    probs = g.random((n, c), dtype=F)
    probs = (probs / probs.sum(1, keepdims=True)).astype(F) if n else probs
    rp = g.random((len(edges), r), dtype=F)
    rp[:, same_part] = np.asarray(link_prob, dtype=F)
    w = None
    if weights == "mixed":                                                      # point counts of very different magnitude
        w = torch.from_numpy(np.where(g.random(n) < 0.5, g.integers(1, 9, n), g.integers(20000, 3000000, n)).astype(F))
    elif weights is not None:
        w = torch.as_tensor(weights, dtype=torch.float32)
    return {"obj_probs": torch.from_numpy(probs), "rel_probs": torch.from_numpy(rp), "edges": torch.from_numpy(edges),
            "batch_ids": None if batch_ids is None else torch.as_tensor(batch_ids, dtype=torch.int64), "n_scenes": n_scenes,
            "same_part": same_part, "threshold": threshold, "mutual": mutual, "weights": w}


def path(n, descending=True, step=1, **kw):
    """Nodes joined i -- i + step (``step`` interleaved paths), the links listed from the far end when ``descending``; plus one unlinked
    edge between the two ends so that a merged edge exists when step > 1."""
    links = [(i + step, i) for i in range(n - step)]
    if descending:
        links = links[::-1]
    edges = links + [(0, n - 1), (n - 1, 0)]
    return _case(n, edges, [1.0] * len(links) + [0.0, 0.0], **kw)


def random_groups(n, n_groups, n_edges, seed, scenes=None, **kw):
    """``n_edges`` random ordered pairs over n nodes, half of them inside one of ``n_groups`` groups (those link), duplicates and self
    loops included.  ``scenes``: node counts per scene (groups never span scenes because only same-scene edges link)."""
    g = np.random.default_rng(seed)
    group = g.integers(0, n_groups, n)
    bid = None
    if scenes is not None:
        bid = np.repeat(np.arange(len(scenes)), scenes)
        assert len(bid) == n
    a = g.integers(0, n, n_edges)
    b = g.integers(0, n, n_edges)
    inside = np.nonzero(g.random(n_edges) < 0.5)[0]
    for i in inside:                                                            # redraw b inside a's group
        same = np.nonzero(group == group[a[i]])[0]
        b[i] = same[g.integers(0, len(same))]
    link = np.where(group[a] == group[b], 0.5 + 0.5 * g.random(n_edges), 0.49 * g.random(n_edges)).astype(F)
    return _case(n, np.stack([a, b], 1), link, batch_ids=bid, n_scenes=1 if scenes is None else len(scenes), seed=seed, **kw)
