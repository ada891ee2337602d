"""Segments merged into objects along "same part" edges, on the host (vlsat_amd/metrics.py::merge_segments_host, the numpy restatement
of csrc/segment_merge.hip; include/vlsat.h states the rule): against the rule written a second time as loops
(segment_merge_checks.brute), one case per clause of the rule, the scan -> transfer -> inherit -> merge route on a small box scan, the
exports, and the build list (the bindings: test_c_abi_cpu.py).  No comparison uses a tolerance.  No GPU."""
import numpy as np
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import evaluate as EV, lib as L, metrics as M, scan as S, scene_graph as SG

from segment_merge_checks import F, _case, assert_tables, brute, path, random_groups


def host(c, trim=True):
    return M.merge_segments_host(c["obj_probs"], c["rel_probs"], c["edges"], c["batch_ids"], c["n_scenes"], c["same_part"], c["threshold"],
                                 c["mutual"], c["weights"], obj_probs=c["obj_probs"], rel_probs=c["rel_probs"], trim=trim)


def components(g):
    ptr, mem = g.member_ptr.tolist(), g.members.tolist()
    return [mem[ptr[o]:ptr[o + 1]] for o in range(int(g.totals[0]))]


CASES = {
    "chain": lambda: path(9, descending=True),
    "chain_ascending": lambda: path(9, descending=False, weights="mixed"),
    "cycle": lambda: _case(6, [(0, 1), (1, 2), (2, 0), (3, 4), (5, 3), (2, 3), (5, 0)], [1, 1, 1, .9, .9, .1, .2]),
    "star": lambda: _case(7, [(6, k) for k in range(5)] + [(5, 6), (6, 5)], [1] * 5 + [0, 0], weights="mixed"),
    "duplicates_and_self_loops": lambda: _case(5, [(0, 1), (0, 1), (1, 0), (2, 2), (3, 2), (3, 2), (2, 3), (4, 4), (0, 3), (0, 3), (1, 2)],
                                               [.9, .1, .2, 1, 0, 0, 0, 1, .3, .4, .1]),
    "cross_scene_edge": lambda: _case(6, [(0, 1), (2, 3), (3, 2), (1, 4), (4, 5), (0, 2)], [1, 1, 1, 1, 1, 0], batch_ids=[0, 0, 0, 1, 1, 1],
                                      n_scenes=2),
    "mutual_one_direction": lambda: _case(5, [(0, 1), (1, 0), (2, 3), (3, 4), (3, 4), (4, 3), (0, 2)], [1, 1, 1, .2, 1, 1, 0], mutual=True),
    "ties_at_threshold": lambda: _case(4, [(0, 1), (2, 3), (1, 2)], [0.25, np.nextafter(F(0.25), F(0)), 0.25], threshold=0.25),
    "no_links": lambda: _case(6, [(a, b) for a in range(6) for b in range(6) if a != b], [0.1] * 30, weights="mixed"),
    "all_linked": lambda: _case(7, [(a, b) for s in ((0, 3), (3, 7)) for a in range(*s) for b in range(*s) if a != b], [1.0] * (6 + 12),
                                batch_ids=[0] * 3 + [1] * 4, n_scenes=2, weights="mixed"),
    "no_nodes": lambda: _case(0, [], [], n_scenes=1),
    "no_scenes": lambda: _case(0, [], [], n_scenes=0),
    "no_edges": lambda: _case(4, [], [], batch_ids=[0, 0, 1, 1], n_scenes=2),
    "empty_scene_between": lambda: _case(5, [(0, 1), (3, 4), (4, 2), (1, 0)], [1, 1, 0, 0], batch_ids=[0, 0, 2, 2, 2], n_scenes=3),
    "random_mutual": lambda: random_groups(60, 9, 500, 3, mutual=True, weights="mixed"),
    "random_scenes": lambda: random_groups(70, 8, 600, 4, scenes=[30, 0, 40]),
}


@pytest.mark.parametrize("name", list(CASES))
def test_host_rule_equals_the_loops(name):
    c = CASES[name]()
    assert_tables(host(c), brute(c), name)


def test_what_the_cases_assert():
    """The cases do what their names say (so that the comparison above compares something)."""
    g = host(CASES["chain"]())
    assert g.totals.tolist() == [1, 0] and g.root.tolist() == [0] * 9 and g.edge_to_pair.tolist() == [-1] * 10
    g = host(CASES["cross_scene_edge"]())
    assert components(g) == [[0, 1], [2], [3], [4, 5]] and g.n_objects.tolist() == [2, 2]
    assert g.edge_to_pair.tolist() == [-1, -1, -1, -1, -1, 0] and g.pair_edges.tolist() == [[0, 1]]      # (2,3), (3,2), (1,4) are dropped
    g = host(CASES["mutual_one_direction"]())
    assert components(g) == [[0, 1], [2], [3, 4]]                                     # 2 -> 3 has no partner; one of the two 3 -> 4 passes: enough
    g = host(CASES["ties_at_threshold"]())
    assert components(g) == [[0, 1, 2], [3]]                                          # equality passes, one ulp below does not
    c = CASES["no_links"]()
    g = host(c)
    assert g.totals.tolist() == [6, 30] and g.object.tolist() == list(range(6)) and torch.equal(g.pair_probs, c["rel_probs"])
    assert torch.equal(g.pair_edges, c["edges"]) and g.pair_count.tolist() == [1] * 30
    g = host(CASES["all_linked"]())
    assert g.totals.tolist() == [2, 0] and g.n_objects.tolist() == [1, 1] and g.pair_probs.shape == (0, 3)
    g = host(CASES["empty_scene_between"]())
    assert g.n_objects.tolist() == [1, 0, 2] and g.obj_batch_ids.tolist() == [0, 2, 2]
    g = host(CASES["duplicates_and_self_loops"]())
    assert components(g) == [[0, 1], [2], [3], [4]] and g.pair_count.tolist() == [2, 1, 2, 1]   # (3,2) x 2; (2,3); (0,3) x 2; (1,2)
    assert g.pair_edges.tolist() == [[2, 1], [1, 2], [0, 2], [0, 1]]                  # ordered pairs, by their first edge row


def test_untrimmed_tables_are_full_size_and_padded():
    c = CASES["random_scenes"]()
    full, cut = host(c, trim=False), host(c)
    m, e = cut.totals.tolist()
    n, ne = c["obj_probs"].shape[0], c["edges"].shape[0]
    assert not full.trimmed and full.obj_probs.shape[0] == n and full.pair_probs.shape[0] == ne and full.member_ptr.shape[0] == n + 1
    assert_tables(full.trim(), cut)
    assert not full.obj_probs[m:].any() and not full.pair_probs[e:].any() and not full.pair_count[e:].any()
    assert (full.pair_edges[e:] == -1).all() and (full.obj_batch_ids[m:] == -1).all() and (full.member_ptr[m:] == n).all()


def test_scene_slices_and_decode():
    c = CASES["random_scenes"]()
    g = host(c)
    first = torch.searchsorted(c["batch_ids"][c["edges"][:, 0]].contiguous(), torch.arange(4))
    assert first.tolist()[0] == 0                                                     # (edges of this case are NOT grouped: only row counts)
    d = g.decode(threshold=0.5, n_labels=2, max_rel=64)
    assert d.labels.shape == (int(g.totals[0]), 2) and d.n_valid.shape == (3,)
    s2 = g.scene(2)
    o0 = int(g.n_objects[0])
    assert s2.totals[0] == g.n_objects[2] and torch.equal(s2.obj_probs, g.obj_probs[o0:]) and int(s2.members.min()) == 0
    assert g.scene(1).totals.tolist() == [0, 0]
    assert torch.equal(s2.pair_edges + o0, g.pair_edges[g.pair_edges[:, 0] >= o0])


def test_bad_arguments_raise():
    c = CASES["chain"]()
    args = lambda **kw: {**dict(obj_logits=c["obj_probs"], rel=c["rel_probs"], edges=c["edges"], batch_ids=None, n_scenes=1, same_part=1), **kw}
    for bad in (dict(same_part=3), dict(same_part=-1), dict(n_scenes=2), dict(n_scenes=-1), dict(threshold=float("nan")),
                dict(edges=c["edges"][:-1]), dict(weights=torch.ones(3))):
        with pytest.raises(L.VlsatError):
            M.merge_segments(**args(**bad))


# ---- scan -> transfer -> inherit -> merge -----------------------------------------------------------------------------------------------
NAMES = ["none", "left", "standing on", "same part"]


def box_scan(seed=0):
    """Four annotated boxes of 600 points, well apart; the predicted cloud is the same points with every box cut into 2-4 slabs along x
    (segment ids 1..), 200+ points each."""
    g = np.random.default_rng(seed)
    pts, inst, seg, next_id = [], [], [], 1
    for k, cuts in enumerate((2, 3, 4, 2)):
        p = g.random((600, 3)) * [1.2, 0.5, 0.5] + [3.0 * k, 0.0, 0.0]
        slab = np.minimum((p[:, 0] - 3.0 * k) / 1.2 * cuts, cuts - 1).astype(np.int64)
        pts.append(p)
        inst.append(np.full(600, k + 1))
        seg.append(next_id + slab)
        next_id += cuts
    pts = np.concatenate(pts)
    return ({"points": pts, "instances": np.concatenate(seg)}, {"points": pts.copy(), "instances": np.concatenate(inst)},
            {1: "chair", 2: "table", 3: "sofa", 4: "lamp"}, [[1, 2, 1, "left"], [4, 3, 2, "standing on"]])


def test_box_scan_merges_back_into_its_annotated_objects():
    pd_mesh, gt_mesh, labels, rel = box_scan()
    t = S.transfer_labels(pd_mesh, gt_mesh, labels, max_sq_dist=0.01, min_seg_size=20, device=None)
    assert sorted(len(v) for v in t.gt_to_segments.values()) == [2, 2, 3, 4]
    ids = sorted(t.segment_to_gt)                                                     # node rows = ascending segment id
    row = {s: i for i, s in enumerate(ids)}
    rel_seg = S.inherit_relationships(t, rel, NAMES)
    same_part = NAMES.index("same part") - 1                                          # a multi-label model drops the leading 'none'
    edges = torch.tensor([(a, b) for a in range(len(ids)) for b in range(len(ids)) if a != b])
    at = {(int(a), int(b)): i for i, (a, b) in enumerate(edges.tolist())}
    hot = torch.zeros(len(edges), len(NAMES) - 1)
    for a, b, k, _ in rel_seg:
        hot[at[row[a], row[b]], k - 1] = 1.0
    probs = torch.from_numpy(np.random.default_rng(1).random((len(ids), 6), dtype=F))
    w = torch.tensor([float((pd_mesh["instances"] == s).sum()) for s in ids])
    run = lambda h, mutual: M.merge_segments(probs, h, edges, None, 1, same_part, 0.5, mutual, w, obj_probs=probs, rel_probs=h)
    want = [[row[s] for s in segs] for segs in sorted(t.gt_to_segments.values())]
    gt_of = [t.segment_to_gt[s] for s in ids]
    for mutual in (False, True):
        g = run(hot, mutual)
        assert components(g) == want
        q = EV.merge_quality(g.root, gt_of)
        assert q["f1"] == 1.0 and q["precision"] == 1.0 and q["recall"] == 1.0 and q["over_merged"] == 0 and q["split"] == 0
    # the merged graph: 'left' between every slab of box 1 and every slab of box 2 folds into one pair
    o = {tuple(c): k for k, c in enumerate(want)}
    chair, table = o[tuple(row[s] for s in t.gt_to_segments[1])], o[tuple(row[s] for s in t.gt_to_segments[2])]
    p = g.pair_edges.tolist().index([chair, table])
    assert g.pair_count[p] == 2 * 3 == (g.edge_to_pair == p).sum() and g.pair_probs[p].tolist() == [1.0, 0.0, 0.0]
    # exports
    node_ids = SG.merged_node_ids(g, ids)
    assert node_ids == [min(v) for v in sorted(t.gt_to_segments.values())]
    entry = SG.add_segments({"scan": "box"}, g, ids)
    assert entry["segments"] == {str(min(v)): v for v in sorted(t.gt_to_segments.values())}
    ann = SG.to_annotation(g.decode(threshold=0.5), 0, g.pair_edges, node_ids, [f"c{k}" for k in range(6)], NAMES, "box")
    assert [node_ids[chair], node_ids[table], 1, "left"] in ann["relationships"]
    assert not any(r[3] == "same part" for r in ann["relationships"])                 # no same-part edge survives between objects
    per_vertex = S.merge_instances(pd_mesh["instances"], ids, g)
    assert sorted(set(per_vertex.tolist())) == node_ids
    assert all(len(set(gt_mesh["instances"][per_vertex == i].tolist())) == 1 for i in node_ids)
    # one direction of one same-part pair missing: the mutual rule splits that object, the plain rule does not
    a, b = (row[s] for s in t.gt_to_segments[1])
    one_way = hot.clone()
    one_way[at[a, b], same_part] = 0.0
    assert components(run(one_way, False)) == want
    split = run(one_way, True)
    assert [a] in components(split) and [b] in components(split) and int(split.totals[0]) == len(want) + 1
    q = EV.merge_quality(split.root, gt_of)
    assert q["split"] == 1 and q["over_merged"] == 0 and q["precision"] == 1.0 and q["recall"] < 1.0


def test_merge_quality_counts():
    q = EV.merge_quality([0, 0, 0, 3, 3, 5], [7, 7, 8, 8, None, -1])
    # matched: rows 0..3.  predicted pairs {01, 02, 12}; annotated pairs {01, 23}; both {01}
    assert (q["segments"], q["pairs_same_pred"], q["pairs_same_gt"], q["pairs_both"]) == (4, 3, 2, 1)
    assert q["precision"] == 1 / 3 and q["recall"] == 1 / 2 and q["f1"] == 2 / 5 and q["over_merged"] == 1 and q["split"] == 1
    assert EV.merge_quality([0, 1], [4, 5])["f1"] == 1.0


def test_the_source_is_built_with_fp_contract_off():
    from vlsat_amd import build as B
    assert "segment_merge.hip" in B.SOURCES and B.PER_SOURCE_FLAGS["segment_merge.hip"] == ["-ffp-contract=off"]
