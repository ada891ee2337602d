"""Annotation transfer onto a predicted segmentation on the host (vlsat_amd/prep.py::nearest_points_host / segment_overlap_host and
vlsat_amd/scan.py::transfer_labels(device=None) / inherit_relationships / read_semseg -- the numpy restatement of
csrc/label_transfer.hip): against a restatement written here as the reference's own loops (data_processing/gen_data.py:242-349: one
point at a time, dictionaries, Python floats), one case per quirk of the rule, and the build list.  No comparison uses a tolerance.
No GPU.  The reference program itself cannot be run (open3d, trimesh and two of its own modules are absent), so nothing here is a
recorded output of it."""
import json

import numpy as np
import pytest

import vlsat_amd  # noqa: F401
from vlsat_amd import lib as L, prep, scan as S, scene_graph as SG

F = np.float32
DEFAULTS = dict(min_seg_size=512, corr_thres=0.5, occ_thres=0.75, occ_min_candidates=3)


# ---- the rule as the reference writes it ---------------------------------------------------------------------------------------------
def loops_nearest(pd_points, gt_points, max_sq_dist):
    """Per predicted point the first annotated point with the smallest d2 (every operation one np.float32 scalar operation), or -1."""
    m = F(max_sq_dist)
    out = []
    for q in pd_points:
        best, best_d = -1, None
        if all(np.isfinite(q)):
            for k, r in enumerate(gt_points):
                if not all(np.isfinite(r)):
                    continue
                dx, dy, dz = F(q[0] - r[0]), F(q[1] - r[1]), F(q[2] - r[2])
                d = F(F(F(dx * dx) + F(dy * dy)) + F(dz * dz))
                if best_d is None or d < best_d:
                    best, best_d = k, d
        out.append(best if best >= 0 and best_d <= m else -1)
    return out


def loops_decide(pd_segments, nn, gt_instances, instance2label, segment_ids, min_seg_size, corr_thres, occ_thres, occ_min_candidates):
    """gen_data.py:254-281 and :315-346 with the issue's reading of its two size tests and of the tie -> (mapping, sizes, counts)."""
    sizes, counts = {}, {}
    for seg_id in segment_ids:
        idx = [i for i, s in enumerate(pd_segments) if s == seg_id]
        sizes[seg_id] = len(idx)
        for i in idx:
            if nn[i] < 0:
                continue
            g = int(gt_instances[nn[i]])
            if g not in instance2label or instance2label[g] == "none":
                continue
            counts.setdefault(seg_id, {}).setdefault(g, 0)
            counts[seg_id][g] += 1
    mapping = {}
    for seg_id, counter in counts.items():
        if not sizes[seg_id] > min_seg_size:
            continue
        max_ratio, max_seg, ratios = -1, -1, []
        for g in sorted(counter):                                    # ascending instance id: a tie stays with the lower one
            ratio = counter[g] / sizes[seg_id]
            ratios.append(ratio)
            if ratio > max_ratio:
                max_ratio, max_seg = ratio, g
        if len(ratios) >= occ_min_candidates:
            ratios = sorted(ratios, reverse=True)
            occ = ratios[1] / ratios[0]
        else:
            occ = 0
        if max_ratio > corr_thres and occ < occ_thres:
            mapping[seg_id] = max_seg
    return mapping, sizes, counts


def assert_overlap_is_loops(out, case, params):
    """``out``: the dict of prep.segment_overlap(_host) as numpy arrays; ``case``: the inputs."""
    seg_ids, gt_ids = list(case["segment_ids"]), list(case["gt_ids"])
    labels = case["instance2label"]
    mapping, sizes, counts = loops_decide(case["pd_segments"].tolist(), case["nn_index"].tolist(), case["gt_instances"], labels, seg_ids, **params)
    assert out["size"].tolist() == [sizes[s] for s in seg_ids]
    assert out["counts"].tolist() == [[counts.get(s, {}).get(g, 0) for g in gt_ids] for s in seg_ids]
    got = {s: gt_ids[m] for s, m in zip(seg_ids, out["match"].tolist()) if m >= 0}
    assert got == mapping
    for k, s in enumerate(seg_ids):
        c = sorted(counts.get(s, {}).values(), reverse=True)
        assert out["best"][k] == (c[0] if c else 0) and out["second"][k] == (c[1] if len(c) > 1 else 0) and out["n_candidates"][k] == len(c)
    return mapping


# ---- inputs shared with tests/test_hip_label_transfer.py -----------------------------------------------------------------------------
def random_clouds(seed, n_gt_pts=260, n_pd_pts=330):
    """A few hundred points: 3-8 annotated instances (one labelled 'none', one without a label), 5-15 predicted segments that mostly
    follow the instances; some predicted points far from every annotated one."""
    rng = np.random.default_rng(seed)
    n_inst, n_seg = int(rng.integers(3, 9)), int(rng.integers(5, 16))
    centres = rng.uniform(-2, 2, size=(n_inst, 3))
    gt_inst = rng.integers(1, n_inst + 1, size=n_gt_pts)
    gt_points = (centres[gt_inst - 1] + rng.normal(scale=0.25, size=(n_gt_pts, 3))).astype(np.float32)
    src = rng.integers(0, n_gt_pts, size=n_pd_pts)
    pd_points = (gt_points[src] + rng.normal(scale=0.05, size=(n_pd_pts, 3))).astype(np.float32)
    far = rng.random(n_pd_pts) < 0.1
    pd_points[far] += np.float32(5.0)
    seg_of_inst = rng.integers(1, n_seg + 1, size=(n_inst + 1, 2))
    pd_seg = seg_of_inst[gt_inst[src], rng.integers(0, 2, size=n_pd_pts)]
    noise = rng.random(n_pd_pts) < 0.15
    pd_seg[noise] = rng.integers(0, n_seg + 1, size=int(noise.sum()))          # (0 = background)
    labels = {i: f"class{i % 4}" for i in range(1, n_inst + 1)}
    labels[1] = "none"
    del labels[n_inst]
    return {"pd_points": pd_points, "pd_segments": pd_seg.astype(np.int64), "gt_points": gt_points, "gt_instances": gt_inst.astype(np.int64),
            "instance2label": labels}


def _overlap_case(rows, instance2label, gt_instances=None):
    """rows: [(segment id, annotated instance id or None for 'no correspondence', number of points)] -> inputs of segment_overlap.
    The annotated cloud has one point per instance id 1..9 (index = id - 1) unless given."""
    gt_instances = np.arange(1, 10, dtype=np.int64) if gt_instances is None else gt_instances
    first = {int(g): k for k, g in reversed(list(enumerate(gt_instances)))}
    seg, nn = [], []
    for s, g, n in rows:
        seg += [s] * n
        nn += [-1 if g is None else first[g]] * n
    order = np.random.default_rng(len(seg)).permutation(len(seg))
    return {"pd_segments": np.asarray(seg, dtype=np.int64)[order], "nn_index": np.asarray(nn, dtype=np.int64)[order],
            "gt_instances": gt_instances, "segment_ids": sorted({r[0] for r in rows}),
            "gt_ids": sorted(i for i, n in instance2label.items() if n != "none"), "instance2label": instance2label}


LABELS = {1: "chair", 2: "table", 3: "lamp", 4: "none", 5: "floor"}          # 4 is 'none'; 6..9 have no label


def quirk_case():
    """One segment per quirk of the decision, min_seg_size = 100.  Expected with the defaults otherwise:
    10 size == min_seg_size -> dropped;  11 size == min_seg_size + 1 -> instance 1;  20 two candidates 51 % : 49 % -> instance 2
    (rejected with occ_min_candidates = 2);  30 / 31 three candidates, second / best = 299 / 400 (accepted) and 301 / 400 (rejected);
    40 half of the points on a 'none' and an unlabelled instance (they count in size, not in count: 40 % -> rejected; 100 % if they
    did not);  50 no point has a correspondence;  60 a tie of the two best (never accepted)."""
    rows = [(10, 1, 100), (11, 1, 101),
            (20, 2, 102), (20, 3, 98),
            (30, 1, 400), (30, 2, 299), (30, 3, 1), (31, 1, 400), (31, 2, 301), (31, 3, 1),
            (40, 5, 80), (40, 4, 60), (40, 7, 60),
            (50, None, 150),
            (60, 3, 120), (60, 2, 120)]
    return _overlap_case(rows, LABELS), dict(DEFAULTS, min_seg_size=100)


def as_np(out):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in out.items()}


# ---- nearest points ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_host_nearest_points_equal_the_loops(seed):
    c = random_clouds(seed)
    c["gt_points"][5] = np.nan                                        # never returned
    c["pd_points"][7, 1] = np.inf                                     # no correspondence
    c["gt_points"][11] = c["gt_points"][3]                            # a duplicate: the lower index wins
    for m in (0.1, 0.01):
        idx, d = prep.nearest_points_host(c["pd_points"], c["gt_points"], m)
        want = loops_nearest(c["pd_points"], c["gt_points"], m)
        assert idx.dtype == np.int32 and d.dtype == np.float32 and idx.tolist() == want
        assert -1 in want and 11 not in want and 5 not in want and want[7] == -1
        for q, k in enumerate(want):
            if k < 0:
                assert np.isposinf(d[q])
            else:
                dx, dy, dz = (F(c["pd_points"][q, a] - c["gt_points"][k, a]) for a in range(3))
                assert d[q].tobytes() == F(F(F(dx * dx) + F(dy * dy)) + F(dz * dz)).tobytes()


def test_the_distance_bound_is_a_squared_distance_and_is_inclusive():
    ref = np.zeros((1, 3), dtype=np.float32)
    at, above = F(0.5), np.nextafter(F(0.5), F(1))
    assert F(at * at) == F(0.25) and F(above * above) > F(0.25)
    q = np.array([[at, 0, 0], [above, 0, 0], [0, -at, 0], [0, 0, -above]], dtype=np.float32)
    idx, d = prep.nearest_points_host(q, ref, 0.25)
    assert idx.tolist() == [0, -1, 0, -1] and d.tolist() == [0.25, np.inf, 0.25, np.inf]
    assert prep.nearest_points_host(q, ref, 0.5)[0].tolist() == [0, 0, 0, 0]          # (as a distance, 0.5 would stop at 0.25 squared)
    idx0, d0 = prep.nearest_points_host(np.array([[0, 0, 0], [1e-3, 0, 0]], dtype=np.float32), ref, 0.0)
    assert idx0.tolist() == [0, -1] and d0[0] == 0                                     # exact coincidence only
    for bad in (-1.0, float("nan")):
        with pytest.raises(L.VlsatError):
            prep.nearest_points_host(q, ref, bad)
    e_idx, e_d = prep.nearest_points_host(q, np.zeros((0, 3), dtype=np.float32), 1.0)
    assert e_idx.tolist() == [-1] * 4 and np.isposinf(e_d).all()
    assert prep.nearest_points_host(np.zeros((0, 3), dtype=np.float32), ref, 1.0)[0].shape == (0,)


def test_cpu_tensors_take_the_host_path():
    import torch
    c = random_clouds(4)
    idx, d = prep.nearest_points(torch.from_numpy(c["pd_points"]), torch.from_numpy(c["gt_points"]), 0.1)
    want = prep.nearest_points_host(c["pd_points"], c["gt_points"], 0.1)
    assert np.array_equal(idx.numpy(), want[0]) and idx.dtype == torch.int32 and d.numpy().tobytes() == want[1].tobytes()


# ---- counts and decision -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_host_overlap_equals_the_loops_on_random_clouds(seed):
    c = random_clouds(seed)
    nn, _ = prep.nearest_points_host(c["pd_points"], c["gt_points"], 0.1)
    seg_ids = [int(s) for s in np.unique(c["pd_segments"]) if s != 0]
    gt_ids = sorted(i for i, n in c["instance2label"].items() if n != "none")
    case = dict(c, nn_index=nn.astype(np.int64), segment_ids=seg_ids, gt_ids=gt_ids)
    accepted = 0
    for params in (dict(DEFAULTS, min_seg_size=12), dict(DEFAULTS, min_seg_size=25, occ_min_candidates=2, corr_thres=0.4)):
        out = prep.segment_overlap_host(c["pd_segments"], nn, c["gt_instances"], seg_ids, gt_ids, **params)
        accepted += len(assert_overlap_is_loops(out, case, params))
    assert accepted > 0


def test_every_quirk_of_the_decision():
    case, params = quirk_case()
    run = lambda **kw: prep.segment_overlap_host(case["pd_segments"], case["nn_index"], case["gt_instances"], case["segment_ids"],   # noqa: E731
                                                 case["gt_ids"], **dict(params, **kw))
    out = run()
    assert_overlap_is_loops(out, case, params)
    ids, gt_ids = case["segment_ids"], case["gt_ids"]
    got = {s: (gt_ids[m] if m >= 0 else None) for s, m in zip(ids, out["match"].tolist())}
    assert got == {10: None, 11: 1, 20: 2, 30: 1, 31: None, 40: None, 50: None, 60: None}
    k = ids.index(40)
    assert out["size"][k] == 200 and out["counts"][k].sum() == 80 and out["n_candidates"][k] == 1
    k = ids.index(50)
    assert out["size"][k] == 150 and out["counts"][k].sum() == 0 and out["n_candidates"][k] == 0 and out["best"][k] == 0
    k = ids.index(60)
    assert out["best"][k] == out["second"][k] == 120
    two = run(occ_min_candidates=2)
    assert_overlap_is_loops(two, case, dict(params, occ_min_candidates=2))
    assert two["match"][ids.index(20)] == -1 and two["match"][ids.index(30)] == out["match"][ids.index(30)]
    assert run(min_seg_size=99)["match"][ids.index(10)] == gt_ids.index(1)                     # the size test alone dropped it
    for name in ("segment_ids", "gt_ids"):
        with pytest.raises(L.VlsatError):
            prep.segment_overlap_host(case["pd_segments"], case["nn_index"], case["gt_instances"],
                                      **{"segment_ids": ids, "gt_ids": gt_ids, name: [3, 3]})


# ---- transfer_labels on the host -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 5])
def test_transfer_labels_on_the_host_equals_the_loops(seed):
    c = random_clouds(seed)
    pd_mesh = {"points": c["pd_points"].astype(np.float64), "instances": c["pd_segments"]}
    gt_mesh = {"points": c["gt_points"].astype(np.float64), "instances": c["gt_instances"]}
    t = S.transfer_labels(pd_mesh, gt_mesh, c["instance2label"], max_sq_dist=0.1, min_seg_size=12, device=None)
    nn = loops_nearest(c["pd_points"], c["gt_points"], 0.1)
    seg_ids = [int(s) for s in np.unique(c["pd_segments"]) if s != 0]
    mapping, sizes, _ = loops_decide(c["pd_segments"].tolist(), nn, c["gt_instances"], c["instance2label"], seg_ids,
                                     **dict(DEFAULTS, min_seg_size=12))
    assert mapping and t.segment_to_gt == mapping and list(t.segment_to_gt) == sorted(mapping)
    assert t.instance2label == {s: c["instance2label"][g] for s, g in sorted(mapping.items())}
    assert t.gt_to_segments == {g: [s for s in sorted(mapping) if mapping[s] == g] for g in dict.fromkeys(mapping[s] for s in sorted(mapping))}
    assert t.segment_ids.tolist() == seg_ids and t.size.tolist() == [sizes[s] for s in seg_ids]
    assert t.n_without_correspondence == sum(k < 0 for k in nn) > 0
    assert "none" not in t.instance2label.values()
    assert t.matched_gt.tolist() == [mapping.get(s, -1) for s in seg_ids]


# ---- inherited relationships ---------------------------------------------------------------------------------------------------------
RELS26 = ["supported by", "left", "right", "front", "behind", "close by", "inside", "bigger than", "smaller than", "higher than",
          "lower than", "same symmetry as", "same as", "attached to", "standing on", "lying on", "hanging on", "connected to",
          "leaning against", "part of", "belonging to", "build in", "standing in", "cover", "lying in", "hanging in"]


def test_inherited_relationships():
    gt_to_segments = {7: [3, 9], 2: [4], 5: [6, 8, 11]}               # instance 1 has no accepted segment
    names = ["none", "left", "same part", "standing on"]
    rel = [[7, 2, 1, "left"], [2, 5, 14, "standing on"], [7, 5, 3, "close by"], [1, 2, 1, "left"], [2, 1, 1, "left"], [5, 7, 1, "left"]]
    out = S.inherit_relationships(gt_to_segments, rel, names)
    want = [[3, 4, 1, "left"], [9, 4, 1, "left"],                                                   # the cartesian product, in order
            [4, 6, 3, "standing on"], [4, 8, 3, "standing on"], [4, 11, 3, "standing on"],          # re-indexed by name
            [6, 3, 1, "left"], [6, 9, 1, "left"], [8, 3, 1, "left"], [8, 9, 1, "left"], [11, 3, 1, "left"], [11, 9, 1, "left"],
            [3, 9, 2, "same part"], [9, 3, 2, "same part"],
            [6, 8, 2, "same part"], [8, 6, 2, "same part"], [6, 11, 2, "same part"], [11, 6, 2, "same part"], [8, 11, 2, "same part"],
            [11, 8, 2, "same part"]]
    assert out == want                                                # 'close by' dropped (not in the list), instance 1 dropped
    no_same = S.inherit_relationships(gt_to_segments, rel, ["left", "standing on"])
    assert no_same == [[a, b, {"left": 0, "standing on": 1}[n], n] for a, b, _, n in want if n != "same part"]
    assert "same part" not in RELS26 and all(r[3] != "same part" for r in S.inherit_relationships(gt_to_segments, rel, RELS26))
    other = S.inherit_relationships(gt_to_segments, rel, ["left", "one object"], same_part="one object")
    assert [r for r in other if r[3] == "one object"] == [[a, b, 1, "one object"] for a, b, _, n in want if n == "same part"]

    class T:                                                          # a LabelTransfer is accepted as well
        pass
    T.gt_to_segments = gt_to_segments
    assert S.inherit_relationships(T, rel, names) == want


def test_inherited_relationships_read_back_as_a_relationship_file(tmp_path):
    gt_to_segments = {7: [3, 9], 2: [4]}
    labels = {3: "chair", 4: "table", 9: "chair"}
    rel = S.inherit_relationships(gt_to_segments, [[7, 2, 1, "left"], [2, 7, 2, "right"]], ["none", "left", "right", "same part"])
    entry = {"scan": "scan-q", "split": 0, "objects": {str(k): v for k, v in labels.items()}, "relationships": rel}
    path = str(tmp_path / "relationships_segments.json")
    SG.write_annotations(path, [entry])
    back_rel, back_objs, scans = S.read_relationships(path, ["scan-q"])
    assert scans == ["scan-q_0"] and back_rel["scan-q_0"] == rel and back_objs["scan-q_0"] == labels
    nodes = [3, 4, 9]
    edges = S.edge_list(nodes, rel, all_edge=True)
    gt_class, gt_rel = S.ground_truth(nodes, edges, back_objs["scan-q_0"], ["chair", "table"], back_rel["scan-q_0"],
                                      ["left", "right", "same part"], True)
    assert gt_class.tolist() == [0, 1, 0] and gt_rel.sum() == len(rel) == 6


def test_read_semseg(tmp_path):
    doc = {"scan_id": "x", "segGroups": [{"objectId": 4, "id": 4, "label": "Sofa Chair", "segments": [1, 2]},
                                         {"objectId": 1, "id": 1, "label": "floor", "segments": [3]},
                                         {"objectId": 12, "id": 12, "label": "none", "segments": []}]}
    path = tmp_path / "semseg.v2.json"
    path.write_text(json.dumps(doc))
    got = S.read_semseg(str(path))
    assert got == {4: "Sofa Chair", 1: "floor", 12: "none"} and list(got) == [4, 1, 12]       # unmapped, the file's order
    assert S.read_semseg(doc) == got
    with pytest.raises(S.ScanError):
        S.read_semseg({"scan_id": "x"})


def test_the_source_is_built_with_fp_contract_off():
    from vlsat_amd import build as B
    assert "label_transfer.hip" in B.SOURCES and "-ffp-contract=off" in B.PER_SOURCE_FLAGS["label_transfer.hip"]
