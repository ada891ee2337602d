"""The decoded scene graph without a GPU: the decision rule pinned to the reference's own run (metrics_small.npz), the host
restatement (metrics.decode_graph_host) against a brute-force loop, the export in the dataset's annotation layout read back by
scan.read_relationships, the C surface, and arguments out of range."""
import numpy as np
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import evaluate as EV, lib as L, metrics as M, scan as S, scene_graph as SG

from graph_decode_checks import METRICS_GOLD, SG_GOLD, assert_equal, brute, case, indicator


@pytest.mark.parametrize("br", ["", "_2d"])
def test_decision_rule_is_the_reference_no_relation_rank(br):
    """An edge without gt relation gets, from the reference's evaluate_topk_predicate, the rank 1 + #(predicates >= 0.5), or
    topk + 1 = 7 when no predicate is below the threshold: its top_k_rel entry counts what the decode asserts."""
    z = np.load(METRICS_GOLD)
    seen, rows_checked = set(), 0
    for c in "abc":
        obj, rel = torch.from_numpy(z[f"{c}.obj_logits{br}"]), torch.from_numpy(z[f"{c}.rel{br}"])
        edges, gt_rel = torch.from_numpy(z[f"{c}.edges"]), z[f"{c}.gt_rel"]
        e, r = rel.shape
        g = M.decode_graph_host(obj, rel, edges, None, 1, True, 0.5, "rel", 1, 4096)
        assert int(g.n_total[0]) == int(g.n_valid[0])
        asserted = indicator(g, 0, e, r).sum(1).numpy()
        first = np.concatenate([[0], np.cumsum(np.maximum(1, (gt_rel == 1).sum(1)))])[:-1]       # first cls_matrix row of an edge
        cm, top = z[f"{c}.cls_matrix"], z[f"{c}.top_k_rel{br}"]
        for j in range(e):
            if (gt_rel[j] == 1).any():
                continue
            assert cm[first[j], 4] == -1
            assert top[first[j]] == (7 if asserted[j] == r else 1 + asserted[j]), (c, j)
            seen.add(int(asserted[j]))
            rows_checked += 1
        assert (cm[:, 4] == -1).sum() == (~(gt_rel == 1).any(1)).sum()
    assert rows_checked == 40 and len(seen) > 5, (rows_checked, sorted(seen))
    if br == "":                                                                      # the 3D outputs hold both extremes
        assert 0 in seen and 26 in seen, sorted(seen)
    assert min(float(np.abs(z[f"{c}.rel{br}"] - 0.5).min()) for c in "abc") > 1e-5          # no value near the threshold


@pytest.mark.parametrize("i", [0, 3, 6, 4])
@pytest.mark.parametrize("br", ["3d", "2d"])
def test_host_path_equals_the_brute_force(i, br):
    z = np.load(SG_GOLD)
    obj, rel, edges, probs, multi, rp = case(z, i, br)
    e, r = rel.shape
    scene = np.zeros(e, np.int64)
    totals = set()
    for score in ("rel", "triplet"):
        for n_labels in (1, 8):
            n_total = int(M.decode_graph_host(obj, rel, edges, None, 1, multi, 0.5, score, 1, 4096, probs, rp).n_total[0])
            assert n_total > 2
            for max_rel in (1, n_total - 1, 4096):
                g = M.decode_graph_host(obj, rel, edges, None, 1, multi, 0.5, score, n_labels, max_rel, obj_probs=probs, rel_probs=rp)
                assert_equal(g, brute(probs, rp, edges, scene, 1, 0.5, multi, score, n_labels, max_rel), (i, br, score, n_labels, max_rel))
                totals.add(n_total)
    # the library's own softmax / exp restatement (no probabilities handed in) decides the same pairs on these cases
    g = M.decode_graph(obj, rel, edges, None, 1, multi, 0.5, "rel", 3, 4096)
    want = M.decode_graph_host(obj, rel, edges, None, 1, multi, 0.5, "rel", 3, 4096, probs, rp)
    assert torch.equal(indicator(g, 0, e, r), indicator(want, 0, e, r)) and torch.equal(g.labels, want.labels)


def test_host_path_batch_threshold_vector_and_empty_scene():
    g = torch.Generator().manual_seed(11)
    n_obj = [4, 1, 3]
    ed, bid, off = [], [], 0
    for s, n in enumerate(n_obj):
        ed += [(off + a, off + b) for a in range(n) for b in range(n) if a != b]
        bid += [s] * n
        off += n
    edges, bid = torch.tensor(ed), torch.tensor(bid)
    e, r, c = edges.shape[0], 7, 9
    probs = torch.softmax(torch.randn(off, c, generator=g) * 2, -1)
    rp = torch.randint(0, 9, (e, r), generator=g).float() / 8
    thr = torch.tensor([0.5, 1.5, -1.0, 0.25, 0.5, 1.0, 0.0])
    for multi in (True, False):
        for score in ("rel", "triplet"):
            for max_rel in (3, 4096):
                got = M.decode_graph_host(probs, rp, edges, bid, 3, multi, thr, score, 2, max_rel, obj_probs=probs, rel_probs=rp)
                assert_equal(got, brute(probs, rp, edges, bid[edges[:, 0]].numpy(), 3, thr.numpy(), multi, score, 2, max_rel))
                assert int(got.n_total[1]) == 0 and int(got.edge[1].max()) == -1
    got = M.decode_graph_host(probs, rp, edges, bid, 3, True, thr, "rel", 2, 4096, obj_probs=probs, rel_probs=rp)
    hot = torch.cat([indicator(got, s, e, r)[None] for s in range(3)]).any(0)
    assert not hot[:, 1].any() and hot[:, 2].all() and hot[:, 6].all()
    assert torch.equal(hot[:, 3], rp[:, 3] >= 0.25) and (rp[:, 3] == 0.25).any()             # equality passes
    one = got.scene(2, 12, (5, 8))
    assert one.labels.shape[0] == 3 and int(one.edge[0, :int(one.n_valid[0])].min()) >= 0
    assert int(one.edge[0, :int(one.n_valid[0])].max()) < 6


@pytest.mark.parametrize("i", [0, 3, 6, 4])
def test_annotation_round_trip(i, tmp_path):
    """to_annotation -> write_annotations -> scan.read_relationships -> edge_list + ground_truth gives back the decoded graph."""
    z = np.load(SG_GOLD)
    obj, rel, edges, probs, multi, rp = case(z, i, "3d")
    e, r = rel.shape
    n = obj.shape[0]
    g = M.decode_graph_host(obj, rel, edges, None, 1, multi, 0.5, "rel", 3, 4096, probs, rp)
    assert int(g.n_valid[0]) == int(g.n_total[0]) > 0                                 # the cap was not hit
    classes = [f"class {k}" for k in range(obj.shape[1])]
    full = ["none"] + [f"relation {k}" for k in range(1, r + 1 if multi else r)]
    ids = [7 + 3 * k for k in range(n)]
    entry = SG.to_annotation(g, 0, edges, ids, classes, full, "scan-x", split=2, multi_rel_outputs=multi)
    assert entry["objects"] == {str(ids[k]): classes[int(g.labels[k, 0])] for k in range(n)}
    assert len(entry["relationships"]) == int(g.n_valid[0])
    path = tmp_path / "relationships_predicted.json"
    SG.write_annotations(path, [entry])
    rels, objs, scans = S.read_relationships(str(path), ["scan-x"])
    assert scans == ["scan-x_2"]
    nodes = list(objs["scan-x_2"].keys())
    assert nodes == ids
    fc = S.edge_list(nodes, rels["scan-x_2"])
    names = full[1:] if multi else full
    gt_cls, gt_rel = S.ground_truth(nodes, fc, objs["scan-x_2"], classes, rels["scan-x_2"], names, multi)
    np.testing.assert_array_equal(gt_cls, g.labels[:, 0].numpy().astype(np.int64))
    pos = {(int(a), int(b)): j for j, (a, b) in enumerate(fc.tolist())}
    rows = torch.tensor([pos[(int(a), int(b))] for a, b in edges.tolist()])
    hot = indicator(g, 0, e, r)
    if multi:
        want = np.zeros((fc.shape[0], r), np.float32)
        want[rows] = hot.numpy()
        np.testing.assert_array_equal(gt_rel, want)
    else:
        want = np.zeros(fc.shape[0], np.int64)
        want[rows] = (hot.long() * torch.arange(r)[None]).sum(1).numpy()
        assert gt_rel.dtype == np.int64
        np.testing.assert_array_equal(gt_rel, want)


def test_counts_host_and_graph_quality():
    z = np.load(SG_GOLD)
    for i in (0, 4):
        obj, rel, edges, probs, multi, rp = case(z, i, "3d")
        e, r = rel.shape
        gt_cls, gt_rel = torch.from_numpy(z[f"c{i}_gt_cls"]), torch.from_numpy(z[f"c{i}_gt_rel"])
        if not multi and gt_rel.dim() == 2:
            gt_rel = (gt_rel * torch.arange(r)[None]).max(1).values
        cnt = M.decode_counts(obj, rel, gt_cls, gt_rel, multi, 0.5, obj_probs=probs, rel_probs=rp)
        hot = indicator(M.decode_graph_host(obj, rel, edges, None, 1, multi, 0.5, "rel", 1, 4096, probs, rp), 0, e, r)
        gt = (gt_rel == 1) if multi else ((gt_rel[:, None] == torch.arange(r)[None]) & (torch.arange(r)[None] != 0))
        for k in range(r):
            assert cnt[3 * k:3 * k + 3].tolist() == [int((hot[:, k] & gt[:, k]).sum()), int((hot[:, k] & ~gt[:, k]).sum()),
                                                     int((gt[:, k] & ~hot[:, k]).sum())]
        assert cnt[3 * r:].tolist() == [obj.shape[0], int((probs.argmax(1) == gt_cls).sum())]
        if not multi:
            assert cnt[:3].tolist() == [0, 0, 0]
        q = EV.graph_quality(cnt, r)
        tp, fp, fn = (float(cnt[j:3 * r:3].sum()) for j in range(3))
        assert q["micro_precision"] == tp / (tp + fp) and q["micro_recall"] == tp / (tp + fn)
        assert q["node_acc"] == float(cnt[3 * r + 1]) / obj.shape[0] and q["nodes"] == obj.shape[0]
        both = EV.graph_quality({"3d": cnt, "2d": cnt}, r)
        assert both["micro_f1_3d"] == both["micro_f1_2d"] == q["micro_f1"]
    v = np.zeros(3 * 2 + 2)
    v[:] = [3, 1, 0, 0, 0, 2, 4, 3]
    q = EV.graph_quality(v, 2)
    assert q["micro_precision"] == 0.75 and q["micro_recall"] == 0.6 and q["macro_recall"] == 0.5 and q["node_acc"] == 0.75


def test_the_source_is_in_the_build_list():
    from vlsat_amd import build as B
    assert "graph_decode.hip" in B.SOURCES


def test_arguments_out_of_range_are_refused_not_clamped():
    p, rel, ed = torch.rand(3, 9), torch.rand(2, 5), torch.tensor([[0, 1], [1, 2]])
    for kw in (dict(n_labels=0), dict(n_labels=9), dict(max_rel=0), dict(max_rel=4097)):
        for fn in (M.decode_graph, M.decode_graph_host):
            with pytest.raises(L.VlsatError, match="must be in"):
                fn(p, rel, ed, None, 1, **kw)
    with pytest.raises(L.VlsatError, match="n_labels"):
        M.decode_graph(p[:, :4], rel, ed, None, 1, n_labels=5)                          # more labels than classes
    with pytest.raises(NotImplementedError):
        M.decode_graph(p, rel, ed, None, 1, score="sgdet")
    with pytest.raises(L.VlsatError, match="batch_ids"):
        M.decode_graph(p, rel, ed, None, 2)
    with pytest.raises(L.VlsatError, match="threshold"):
        M.decode_graph(p, rel, ed, None, 1, threshold=[0.5, 0.5])
    g = M.decode_graph(p, rel, ed, None, 1, n_labels=8, max_rel=4096)
    assert g.labels.shape == (3, 8) and g.edge.shape == (1, 4096)
