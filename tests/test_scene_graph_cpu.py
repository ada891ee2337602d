"""The predicted scene graph without a GPU: the host path (metrics.scene_graph_topk_host) against the reference's own
pred_triplets (tests/golden/scene_graph_cases.npz, made by make_golden_scene_graph.py), against a brute force over the full
product on cases with ties, and against the pinned Recall@K counts; the labelled export; the C surface; no blocking HIP call
in csrc/scene_graph.hip."""
import json
import os
import re

import numpy as np
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import lib as L, metrics as M, scene_graph as SG

from scene_graph_checks import check_contract, graphs_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "scene_graph_cases.npz")
VARIANTS = (("triplet", 1), ("triplet", 100), ("rels", 1), ("rels", 100))
GAP = 1e-6                                    # the margin make_golden_scene_graph.py asserted at every boundary


def golden_case(z, i, br, dev="cpu"):
    t = lambda k: torch.from_numpy(z[f"c{i}_{k}"]).to(dev)
    return t(f"obj_logits_{br}"), t(f"rel_{br}"), t("edges"), t(f"probs_{br}"), bool(z[f"c{i}_multi"])


def golden_probs(z, i, br, rel, multi, dev="cpu"):
    """The predicate probabilities the reference scored with: rel itself, or its np.exp of a single-label model's output."""
    return rel if multi else torch.from_numpy(z[f"c{i}_relp_{br}"]).to(dev)


def golden_rows(z, i, br, evaluate, each, edges):
    """(edge row, sub, obj, pred) [n, 4] and scores [n] of the reference's list (its tuples name the edge by its two nodes)."""
    rows, score = z[f"c{i}_{evaluate}_{each}_{br}_rows"], z[f"c{i}_{evaluate}_{each}_{br}_score"]
    pos = {(int(a), int(b)): e for e, (a, b) in enumerate(edges.tolist())}
    assert len(pos) == edges.shape[0]
    ed = np.array([pos[(int(a), int(b))] for a, b in rows[:, :2]], dtype=np.int64)
    return np.concatenate([ed[:, None], rows[:, 2:].astype(np.int64)], 1), score


def assert_golden(g, want_rows, want_score, exact):
    n = len(want_score)
    assert int(g.n_valid[0]) == n
    got = torch.stack([g.edge[0, :n], g.sub_cls[0, :n], g.obj_cls[0, :n], g.pred[0, :n]], 1).cpu().numpy().astype(np.int64)
    np.testing.assert_array_equal(got, want_rows)
    sc = g.score[0, :n].cpu().numpy()
    if exact:
        np.testing.assert_array_equal(sc, want_score)
    else:
        np.testing.assert_allclose(sc, want_score, rtol=GAP, atol=0)


@pytest.mark.parametrize("br", ["3d", "2d"])
def test_host_path_equals_reference_pred_triplets(br):
    z = np.load(GOLD)
    for i in range(int(z["n_cases"])):
        obj, rel, edges, probs, multi = golden_case(z, i, br)
        for evaluate, each in VARIANTS:
            rows, score = golden_rows(z, i, br, evaluate, each, edges)
            relp = golden_probs(z, i, br, rel, multi)
            g = M.scene_graph_topk(obj, relp, edges, None, 1, True, 100, each, evaluate, obj_probs=probs)
            assert_golden(g, rows, score, exact=True)
            g = M.scene_graph_topk(obj, rel, edges, None, 1, multi, 100, each, evaluate)          # softmax of the logits, exp here
            assert_golden(g, rows, score, exact=False)
            g20 = M.scene_graph_topk(obj, relp, edges, None, 1, True, 20, each, evaluate, obj_probs=probs)
            assert_golden(g20, rows[:20], score[:20], exact=True)


def hits_from_graph(g, s, gt_cls, hot, edges, mode):
    """Edges of scene s with a correct row among the first 20 / 50 / 100 (evaluate_triplet_recallk's count)."""
    n = int(g.n_valid[s])
    ed, sc, oc, pr = (t[s, :n].long() for t in (g.edge, g.sub_cls, g.obj_cls, g.pred))
    ok = hot[ed, pr]
    if mode == "triplet":
        ok &= (sc == gt_cls[edges[ed, 0]]) & (oc == gt_cls[edges[ed, 1]])
    return [int(ed[:k][ok[:k]].unique().numel()) for k in (20, 50, 100)]


@pytest.mark.parametrize("br", ["3d", "2d"])
def test_emitted_lists_reproduce_the_pinned_recall_counts(br):
    z = np.load(GOLD)
    names = {("triplet", 1): "sgcls_gc", ("triplet", 100): "sgcls_ngc", ("rels", 1): "predcls_gc", ("rels", 100): "predcls_ngc"}
    for i in range(int(z["n_cases"])):
        obj, rel, edges, probs, multi = golden_case(z, i, br)
        gt_cls, gt_rel = torch.from_numpy(z[f"c{i}_gt_cls"]), torch.from_numpy(z[f"c{i}_gt_rel"])
        hot = M.multihot_targets(gt_rel, rel.shape[1]) == 1
        counts = M.recallk_counts_host(obj, rel, gt_cls, gt_rel, edges, None, 1, multi, obj_probs=probs)[0]
        for (evaluate, each), name in names.items():
            g = M.scene_graph_topk(obj, rel, edges, None, 1, multi, 100, each, evaluate, obj_probs=probs)
            base = M.recallk_offset(name, rel.shape[1])
            assert hits_from_graph(g, 0, gt_cls, hot, edges, evaluate) == counts[base:base + 3].tolist(), (i, name)
            with np.errstate(invalid="ignore", divide="ignore"):
                rec = np.array(counts[base:base + 3].tolist()) / int(counts[0])
            np.testing.assert_array_equal(rec, z[f"c{i}_{evaluate}_{each}_{br}_recall"])


def tie_cases(dev="cpu"):
    """(name, probs [N, C], rel probabilities [E, R], edges, batch ids, scenes): ties on purpose and odd graphs, small classes."""
    g = torch.Generator().manual_seed(5)
    c, r = 6, 5
    fc = lambda n, off=0: [(a + off, b + off) for a in range(n) for b in range(n) if a != b]
    out = []
    p = torch.full((4, c), 1.0 / c)
    out.append(("uniform object rows", p, torch.rand(12, r, generator=g), fc(4), [0] * 4, 1))
    p = torch.softmax(torch.randn(5, c, generator=g) * 2, -1)
    p[1] = p[0]
    rel = torch.rand(20, r, generator=g)
    rel[4:8] = rel[0:4]
    out.append(("two identical nodes", p, rel, fc(5), [0] * 5, 1))
    rel = torch.sigmoid(torch.randn(12, r, generator=g) * 3)
    rel[:, :3] = 1.0
    out.append(("saturated sigmoids", torch.softmax(torch.randn(4, c, generator=g), -1), rel, fc(4), [0] * 4, 1))
    p = torch.softmax(torch.randn(4, c, generator=g) * 60, -1)
    out.append(("underflow to zero", p * 1e-30, torch.rand(12, r, generator=g) * 1e-20, fc(4), [0] * 4, 1))
    p = torch.softmax(torch.randn(9, c, generator=g) * 2, -1)
    ed = fc(3) + fc(3, 6)                                         # scene 1 (nodes 3..5) has no edge
    out.append(("empty scene in the middle", p, torch.rand(12, r, generator=g), ed, [0] * 3 + [1] * 3 + [2] * 3, 3))
    ed = [(0, 0), (0, 1), (0, 1), (1, 0), (2, 2), (1, 0)]
    out.append(("self loops and duplicate edges", p[:3], torch.rand(6, r, generator=g), ed, [0] * 3, 1))
    out.append(("fewer candidates than K", p[:2], torch.rand(2, r, generator=g), fc(2), [0] * 2, 1))
    t = lambda x, dt: torch.as_tensor(x, dtype=dt).to(dev)
    return [(n, t(p, torch.float32), t(rl, torch.float32), t(e, torch.int64).view(-1, 2), t(b, torch.int64), s)
            for n, p, rl, e, b, s in out]


@pytest.mark.parametrize("evaluate", ["triplet", "rels"])
def test_host_path_keeps_the_contract_with_ties(evaluate):
    for name, probs, rel, edges, bid, n_sc in tie_cases():
        scene = bid[edges[:, 0]]
        for top_k in (1, 7, 100, 1024):
            for each in (1, 3, 100):
                g = M.scene_graph_topk_host(probs, rel, edges, bid, n_sc, True, top_k, each, evaluate, obj_probs=probs)
                check_contract(g, probs, rel, edges, scene, n_sc, top_k, each, evaluate)
                again = M.scene_graph_topk_host(probs, rel, edges, bid, n_sc, True, top_k, each, evaluate, obj_probs=probs)
                assert graphs_equal(g, again), name


def test_arguments_out_of_range_are_refused():
    p, rel, ed = torch.rand(3, 4), torch.rand(2, 5), torch.tensor([[0, 1], [1, 2]])
    for kw in (dict(top_k=0), dict(top_k=1025), dict(topk_each=0), dict(topk_each=101)):
        with pytest.raises(L.VlsatError, match="must be in"):
            M.scene_graph_topk(p, rel, ed, None, 1, **kw)
    with pytest.raises(NotImplementedError):
        M.scene_graph_topk(p, rel, ed, None, 1, evaluate="sgdet")
    with pytest.raises(L.VlsatError, match="batch_ids"):
        M.scene_graph_topk(p, rel, ed, None, 2)
    with pytest.raises(L.VlsatError, match=r"\[E,2\]"):
        M.scene_graph_topk(p, rel, ed[:1], None, 1)


def test_records_round_trip(tmp_path, golden_dir):
    """to_records / write_json on the scan_small fixture scene: its instance ids and label names."""
    from vlsat_amd import scan as S
    e = json.load(open(os.path.join(golden_dir, "scan_small_expect.json")))
    rel, objs, scans = S.read_relationships(os.path.join(golden_dir, "scan_small_relationships.json"), ["scan-a"])
    key = scans[0]
    mesh = S.read_ply(os.path.join(golden_dir, "scan_small.ply"))
    nodes = S.scene_nodes(mesh["instances"], objs[key])
    edges = torch.from_numpy(S.edge_list(nodes, rel[key]))
    classes, relations = e["classes"], e["relations"]
    g = torch.Generator().manual_seed(3)
    logits, rp = torch.randn(len(nodes), len(classes), generator=g) * 3, torch.rand(edges.shape[0], len(relations), generator=g)
    graph = M.scene_graph_topk(logits, rp, edges, None, 1, True, top_k=10, topk_each=2)
    recs = SG.to_records(graph, 0, edges, nodes, classes, relations)
    assert len(recs) == int(graph.n_valid[0]) == min(10, 2 * edges.shape[0])
    probs = torch.softmax(logits, -1)
    for k, rec in enumerate(recs):
        a, b = edges[int(graph.edge[0, k])].tolist()
        assert rec["subject"] == nodes[a] and rec["object"] == nodes[b]
        assert rec["subject_label"] == classes[int(graph.sub_cls[0, k])] and rec["object_label"] == classes[int(graph.obj_cls[0, k])]
        assert rec["predicate"] == relations[int(graph.pred[0, k])]
        assert np.float32(rec["score"]) == graph.score[0, k].numpy()
    assert [r["score"] for r in recs] == sorted((r["score"] for r in recs), reverse=True)
    best = recs[0]
    assert best["score"] == float((probs.max(1).values[edges[:, 0]] * probs.max(1).values[edges[:, 1]] * rp.max(1).values).max())
    path = tmp_path / "graphs.json"
    SG.write_json(path, {key: recs})
    assert SG.read_json(path) == {key: recs}
    rels = SG.to_records(M.scene_graph_topk(logits, rp, edges, None, 1, True, 5, 1, "rels"), 0, edges, nodes, classes, relations)
    assert len(rels) == 5 and all(r["subject_label"] is None and r["object_label"] is None for r in rels)


def test_the_source_is_in_the_build_list():
    from vlsat_amd import build as B
    assert "scene_graph.hip" in B.SOURCES


BLOCKING = re.compile(r"\b(hipDeviceSynchronize|hipStreamSynchronize|hipMemcpy\w*|hipMemset\w*|hipMalloc\w*|hipFree\w*|hipHostMalloc|"
                      r"hipEventSynchronize|atomic\w+)\s*\(")


def test_scene_graph_kernels_have_no_blocking_call_fill_or_atomic():
    def code_of(name):
        txt = open(os.path.join(ROOT, "cvpr2023-vlsat_amd", "csrc", name)).read()
        txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
        return "\n".join(l.split("//")[0] for l in txt.splitlines())
    code = code_of("scene_graph.hip")
    assert not BLOCKING.findall(code) and not BLOCKING.findall(code_of("select_core.h"))
    # five launches: four here, and the per-node sort it shares with the ranking step (eval_ranks.hip launch_sort_probs)
    assert code.count("hipLaunchKernelGGL") == 4 and code.count("launch_sort_probs(") == 1
    ranks = code_of("eval_ranks.hip")
    sort = ranks[ranks.index("int launch_sort_probs("):ranks.index("int launch_softmax_rows(")]
    assert sort.count("hipLaunchKernelGGL") == 1 and not BLOCKING.findall(sort)
    kernel = ranks[ranks.index("void sort_probs_kernel("):ranks.index("void tri_rank_kernel(")]
    assert not BLOCKING.findall(kernel)
    api = open(os.path.join(ROOT, "cvpr2023-vlsat_amd", "csrc", "engine_api.hip")).read()
    body = api[api.index("int vlsat_scene_graph_topk("):api.index("int vlsat_scene_checksums(")]
    assert not BLOCKING.findall("\n".join(l.split("//")[0] for l in body.splitlines()))
