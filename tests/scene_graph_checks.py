"""Brute-force check of the output contract of the predicted scene graph (include/vlsat.h, vlsat_scene_graph_topk), shared by
the CPU and the GPU tests.  It forms the full [edges, C, C, R] product with torch in chunks and takes ``topk`` per edge: no
dominance table, so it does not share the selection's argument."""
import torch


def edge_candidates(probs, rp, edges, mode, each=100, budget=1 << 27):
    """[E, min(each, #entries)] the largest entries of every edge, descending: fl(fl(s_i * o_j) * r_k), or r_k in rels mode."""
    e, r = rp.shape
    if mode == "rels":
        return rp.sort(1, descending=True).values[:, :min(each, r)]
    c = probs.shape[1]
    lim = min(each, c * c * r)
    out = torch.empty(e, lim, dtype=torch.float32, device=rp.device)
    chunk = max(1, budget // (c * c * r))
    for e0 in range(0, e, chunk):
        sl = slice(e0, min(e, e0 + chunk))
        so = probs[edges[sl, 0]][:, :, None] * probs[edges[sl, 1]][:, None, :]
        full = so[:, :, :, None] * rp[sl][:, None, None, :]
        out[sl] = full.reshape(full.shape[0], -1).topk(lim, 1).values
    return out


def check_contract(graph, probs, rp, edges, scene_of_edge, n_scenes, top_k, each, mode, cand=None):
    """Points 1-4 for every scene; ``cand`` = edge_candidates(..., each=100) may be passed in (its first columns are the
    candidates of a smaller topk_each)."""
    e, r = rp.shape
    c = probs.shape[1] if mode == "triplet" else 1
    if cand is None:
        cand = edge_candidates(probs, rp, edges, mode, each)
    lim = min(each, r if mode == "rels" else c * c * r)
    cand = cand[:, :lim]
    assert graph.score.shape == (n_scenes, top_k) and graph.edge.shape == (n_scenes, top_k) and graph.n_valid.shape == (n_scenes,)
    for s in range(n_scenes):
        idx = torch.nonzero(scene_of_edge == s).view(-1)
        n = min(top_k, idx.numel() * lim)
        assert int(graph.n_valid[s]) == n, (s, int(graph.n_valid[s]), n)
        ed, sc, oc, pr, val = (t[s].long() if t.dtype != torch.float32 else t[s]
                               for t in (graph.edge, graph.sub_cls, graph.obj_cls, graph.pred, graph.score))
        assert bool((ed[n:] == -1).all() and (sc[n:] == -1).all() and (oc[n:] == -1).all() and (pr[n:] == -1).all()), s
        assert bool((val[n:] == 0).all()), s
        if n == 0:
            continue
        ed, sc, oc, pr, val = ed[:n], sc[:n], oc[:n], pr[:n], val[:n]
        # 1. the scores are the n largest candidate values of the scene, bit for bit
        want = cand[idx].reshape(-1).sort(descending=True).values[:n]
        assert torch.equal(val, want), (s, "scores", int((val != want).sum()))
        # nothing out of range
        assert bool(((ed >= idx.min()) & (ed <= idx.max()) & (scene_of_edge[ed] == s)).all()), (s, "edge range")
        assert bool(((pr >= 0) & (pr < r)).all()), (s, "predicate range")
        if mode == "triplet":
            assert bool(((sc >= 0) & (sc < c) & (oc >= 0) & (oc < c)).all()), (s, "class range")
            prod = (probs[edges[ed, 0], sc] * probs[edges[ed, 1], oc]) * rp[ed, pr]
            code = (sc * c + oc) * r + pr
        else:
            assert bool(((sc == -1) & (oc == -1)).all()), s
            prod = rp[ed, pr]
            code = pr
        # 2. a row's score is the product at its indices; rows are distinct; at most topk_each per edge, each a candidate of its edge
        assert torch.equal(prod, val), (s, "row product", int((prod != val).sum()))
        full = ed * (c * c * r) + code
        assert full.unique().numel() == n, (s, "duplicate rows")
        per_edge = torch.bincount(ed - idx.min(), minlength=int(idx.max() - idx.min()) + 1)
        assert int(per_edge.max()) <= each, (s, "rows per edge", int(per_edge.max()))
        assert bool((val >= cand[ed, lim - 1]).all()), (s, "a row is not among its edge's candidates")
        # 3. every candidate strictly greater than the last kept score is present
        last = val[-1]
        rows_above = torch.bincount((ed - idx.min())[val > last], minlength=per_edge.numel())
        cand_above = torch.zeros_like(rows_above)
        cand_above[idx - idx.min()] = (cand[idx] > last).sum(1)
        assert torch.equal(rows_above, cand_above), (s, "a candidate above the last kept score is missing")
        # 4. score descending, then edge, subject class, object class, predicate ascending
        if n > 1:
            assert bool(((val[:-1] > val[1:]) | ((val[:-1] == val[1:]) & (full[:-1] < full[1:]))).all()), (s, "row order")


def graphs_equal(a, b):
    return all(torch.equal(getattr(a, k), getattr(b, k)) for k in ("edge", "sub_cls", "obj_cls", "pred", "score", "n_valid"))


def three_valued_scene(p50, p75, seed=0, n=34, r=26, c=12):
    """(probs [n, c], rel [E, r], edges [E, 2]) of one fully connected scene of 34 objects -- E = 1 122: one 1024-edge chunk of the
    scene kernels plus 98 edges -- whose relation scores are 0.75 (probability p75), 0.5 (p50) or 0.25 only, so that equal scores
    lie on both sides of edge 1024 and a cap falls inside a run of them."""
    g = torch.Generator().manual_seed(seed)
    edges = torch.tensor([(a, b) for a in range(n) for b in range(n) if a != b])
    u = torch.rand(edges.shape[0], r, generator=g)
    rel = torch.full_like(u, 0.25)
    rel[u < p50 + p75] = 0.5
    rel[u < p75] = 0.75
    return torch.softmax(torch.randn(n, c, generator=g), -1), rel, edges
