"""csrc/label_transfer.hip on the GPU: nearest points and the segment / instance overlap against the host restatement (prep.*_host) and a
brute force written here, element for element with no tolerance; then a segmentation of a synthetic scan scored end to end
(transfer_labels -> inherit_relationships -> prepare_scan -> validation, decode, export)."""
import numpy as np
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import VLSATConfig, evaluate as EV, lib as L, prep, scan as S, scene_graph as SG, synth
from test_label_transfer_cpu import DEFAULTS, RELS26, as_np, assert_overlap_is_loops, quirk_case, random_clouds

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path cannot run and there is no fallback")


def brute(q, r, m):
    """All pairs, a block of queries at a time; argmin takes the first (= lowest-index) minimum."""
    m = F(m)
    keep = np.nonzero(np.isfinite(r).all(1))[0]
    rr = r[keep]
    idx, d = np.full(len(q), -1, dtype=np.int32), np.full(len(q), np.inf, dtype=np.float32)
    if not len(rr):
        return idx, d
    rx, ry, rz = (np.ascontiguousarray(rr[:, a])[None, :] for a in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        for c0 in range(0, len(q), 64):
            qc = q[c0:c0 + 64]
            d2 = qc[:, 0:1] - rx
            np.multiply(d2, d2, out=d2)
            t = qc[:, 1:2] - ry
            np.multiply(t, t, out=t)
            np.add(d2, t, out=d2)
            t = qc[:, 2:3] - rz
            np.multiply(t, t, out=t)
            np.add(d2, t, out=d2)
            j = d2.argmin(1)
            dm = d2[np.arange(len(qc)), j]
            ok = np.isfinite(qc).all(1) & (dm <= m)
            idx[c0:c0 + 64] = np.where(ok, keep[j], -1)
            d[c0:c0 + 64] = np.where(ok, dm, np.inf)
    return idx, d


def check_nearest(q, r, m, what):
    """device == host path == brute force, indices and distance bits."""
    q, r = np.ascontiguousarray(q, dtype=np.float32).reshape(-1, 3), np.ascontiguousarray(r, dtype=np.float32).reshape(-1, 3)
    gi, gd = prep.nearest_points(torch.from_numpy(q).to(DEV), torch.from_numpy(r).to(DEV), m)
    assert gi.is_cuda and gi.dtype == torch.int32 and gd.dtype == torch.float32 and gi.shape == gd.shape == (len(q),)
    gi, gd = gi.cpu().numpy(), gd.cpu().numpy()
    for name, (wi, wd) in (("host", prep.nearest_points_host(q, r, m)), ("brute force", brute(q, r, m))):
        assert np.array_equal(gi, wi), (what, name, "index")
        assert gd.tobytes() == wd.tobytes(), (what, name, "distance bits")
    return gi, gd


# ---- nearest points --------------------------------------------------------------------------------------------------------------
def test_one_point_against_one_point():
    _need_gpu()
    assert check_nearest([[0.1, 0.2, 0.3]], [[0.1, 0.2, 0.5]], 0.1, "1x1")[0].tolist() == [0]
    assert check_nearest([[0.1, 0.2, 0.3]], [[0.1, 0.2, 0.7]], 0.1, "1x1 too far")[0].tolist() == [-1]


def test_sizes_that_are_no_multiple_of_the_wave():
    _need_gpu()
    rng = np.random.default_rng(10)
    r = rng.uniform(-1, 1, size=(193, 3)).astype(np.float32)
    q = rng.uniform(-1.2, 1.2, size=(257, 3)).astype(np.float32)
    r[17] = np.nan
    r[40, 2] = -np.inf
    q[3, 0] = np.inf
    q[200] = np.nan
    for m in (0.1, 0.01, 10.0, float("inf")):
        gi, _ = check_nearest(q, r, m, f"257x193 m={m}")
        assert gi[3] == gi[200] == -1 and 17 not in gi and 40 not in gi
    assert (check_nearest(q, r, 0.01, "")[0] < 0).sum() > 2


def _grid_cells(ref, max_sq_dist):
    """The cell count of the grid rule in include/vlsat.h (nearest_points), when the first cell edge fits: edge = fl(sqrt(max_sq_dist)
    (1 + 2^-6)), floor(extent / edge) + 1 cells per axis, in fp32."""
    f = np.float32
    inv = f(1) / f(np.sqrt(f(max_sq_dist)) * f(1.015625))
    n = [int(f(f(hi - lo) * inv)) + 1 for lo, hi in zip(ref.min(0), ref.max(0))]
    assert max(n) <= 1024 and n[0] * n[1] * n[2] <= 1 << 21, n
    return n[0] * n[1] * n[2]


def test_a_room_of_many_blocks():
    _need_gpu()
    rng = np.random.default_rng(11)
    ext = np.array([6.0, 6.0, 3.0])
    r = (rng.uniform(0, 1, size=(30000, 3)) * ext).astype(np.float32)
    q = (rng.uniform(-0.05, 1.05, size=(20000, 3)) * ext).astype(np.float32)
    # the scan of the cell counts walks tiles of 4096: less than one tile at 0.1, 101 tiles and a ragged one at 0.004
    assert _grid_cells(r, 0.1) == 19 * 19 * 10 and _grid_cells(r, 0.004) == 94 * 94 * 47 == 101 * 4096 + 1596
    gi, _ = check_nearest(q, r, 0.1, "20000x30000")
    assert (gi >= 0).mean() > 0.9
    gi, _ = check_nearest(q[:4000], r, 0.004, "4000x30000, small radius")
    assert 0.05 < (gi >= 0).mean() < 0.95


def test_no_queries_and_no_annotated_points():
    _need_gpu()
    e = np.zeros((0, 3), dtype=np.float32)
    pts = np.random.default_rng(12).normal(size=(70, 3)).astype(np.float32)
    assert check_nearest(e, pts, 0.1, "Q=0")[0].shape == (0,)
    gi, gd = check_nearest(pts, e, 0.1, "G=0")
    assert (gi == -1).all() and np.isposinf(gd).all()
    assert check_nearest(e, e, 0.1, "both empty")[0].shape == (0,)


def test_negative_coordinates_on_cell_boundaries():
    """max_sq_dist = 0.25: the cell edge is 0.5 * (1 + 2^-6) exactly, the grid starts at the smallest annotated coordinate; annotated
    points on the lattice of cell corners, queries exactly at the distance bound from them and one float beyond."""
    _need_gpu()
    h = F(0.5) * F(1.015625)
    k = np.arange(-4, 5, dtype=np.float32)
    r = np.stack(np.meshgrid(k * h, k * h, k[:3] * h, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    assert r.min() < 0
    at, above = F(0.5), np.nextafter(F(0.5), F(1))
    offs = np.array([[at, 0, 0], [-at, 0, 0], [0, at, 0], [0, 0, -at], [above, 0, 0], [0, -above, 0], [0, 0, above], [0, 0, 0]], dtype=np.float32)
    q = (r[:, None, :] + offs[None, :, :]).reshape(-1, 3)
    gi, gd = check_nearest(q, r, 0.25, "lattice")
    assert (gi >= 0).any() and (gi < 0).any() and (gd[gi >= 0] <= 0.25).all()


def test_duplicates_coincident_points_and_a_zero_radius():
    _need_gpu()
    rng = np.random.default_rng(13)
    r0 = rng.uniform(-1, 1, size=(500, 3)).astype(np.float32)
    q = np.concatenate([r0[::3] + F(0.01), r0[:50]])
    gi, _ = check_nearest(q, np.concatenate([r0, r0, r0[::-1]]), 0.1, "duplicates")
    assert (gi >= 0).all() and gi.max() < 500                                        # ties go to the lower index
    gi, gd = check_nearest(np.concatenate([r0[:40], r0[40:80] + F(1e-3)]), r0, 0.0, "max_sq_dist = 0")
    assert gi[:40].tolist() == list(range(40)) and (gi[40:] == -1).all() and (gd[:40] == 0).all()
    # one overfull cell: 5000 annotated points at one place, a few elsewhere
    r = np.concatenate([rng.uniform(-1, 1, size=(30, 3)), np.tile([[0.25, -0.5, 0.125]], (5000, 1)), rng.uniform(-1, 1, size=(30, 3))]).astype(np.float32)
    q = np.concatenate([np.array([[0.25, -0.5, 0.125], [0.26, -0.5, 0.125]]), rng.uniform(-1, 1, size=(300, 3))]).astype(np.float32)
    gi, _ = check_nearest(q, r, 0.1, "5000 coincident")
    assert gi[0] == gi[1] == 30
    gi, _ = check_nearest(q[:64], np.tile([[0.25, -0.5, 0.125]], (5000, 1)), 0.1, "every annotated point coincides")
    assert set(gi.tolist()) <= {0, -1} and gi[0] == 0


def test_a_cloud_far_wider_than_the_cell_cap_allows():
    """10^4 m across with max_sq_dist = 1e-4: 10^6 cells of 0.01 m per axis would be needed; the edge grows instead."""
    _need_gpu()
    rng = np.random.default_rng(14)
    r = rng.uniform(-5e3, 5e3, size=(4000, 3)).astype(np.float32)
    r = np.concatenate([r, r[:500] + rng.uniform(-3e-3, 3e-3, size=(500, 3)).astype(np.float32)])
    q = np.concatenate([r[::2] + rng.uniform(-4e-3, 4e-3, size=(len(r[::2]), 3)).astype(np.float32),
                        rng.uniform(-5e3, 5e3, size=(300, 3)).astype(np.float32)])
    gi, _ = check_nearest(q, r, 1e-4, "wide cloud")
    assert 0.2 < (gi >= 0).mean() < 0.98


def test_a_bad_distance_bound_is_an_error_code():
    _need_gpu()
    lib = L.load()
    p = torch.zeros(4, 3, device=DEV)
    scratch = torch.empty(int(lib.vlsat_nearest_points_scratch_bytes(4, 4)), dtype=torch.uint8, device=DEV)
    idx = torch.full((4,), 7, dtype=torch.int32, device=DEV)
    d = torch.zeros(4, device=DEV)
    for bad in (-1.0, float("nan")):
        rc = lib.vlsat_nearest_points(p.data_ptr(), 4, p.data_ptr(), 4, bad, scratch.data_ptr(), idx.data_ptr(), d.data_ptr(), L.stream_ptr())
        assert rc != 0 and "max_sq_dist" in lib.vlsat_last_error().decode()
        with pytest.raises(L.VlsatError):
            prep.nearest_points(p, p, bad)
    torch.cuda.synchronize()
    assert idx.tolist() == [7] * 4                                                    # refused: nothing written


# ---- counts and decision ---------------------------------------------------------------------------------------------------------
def dev_overlap(case, params):
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).to(DEV)   # noqa: E731
    out = prep.segment_overlap(d(case["pd_segments"]), d(case["nn_index"]), d(case["gt_instances"]), case["segment_ids"], case["gt_ids"], **params)
    assert all(v.is_cuda and v.dtype == torch.int32 for v in out.values())
    return as_np(out)


def assert_dev_is_host(case, params):
    got = dev_overlap(case, params)
    want = prep.segment_overlap_host(case["pd_segments"], case["nn_index"], case["gt_instances"], case["segment_ids"], case["gt_ids"], **params)
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    return got


def test_overlap_on_the_quirk_cases():
    _need_gpu()
    case, params = quirk_case()
    for extra in ({}, {"occ_min_candidates": 2}, {"min_seg_size": 99}, {"corr_thres": 0.39, "occ_thres": 0.76}):
        p = dict(params, **extra)
        assert_overlap_is_loops(assert_dev_is_host(case, p), case, p)
    ids, gt_ids = case["segment_ids"], case["gt_ids"]
    got = dev_overlap(case, params)
    assert {s: (gt_ids[m] if m >= 0 else None) for s, m in zip(ids, got["match"].tolist())} == \
        {10: None, 11: 1, 20: 2, 30: 1, 31: None, 40: None, 50: None, 60: None}


@pytest.mark.parametrize("seed", [1, 2])
def test_overlap_on_random_clouds(seed):
    _need_gpu()
    c = random_clouds(seed)
    nn, _ = prep.nearest_points(torch.from_numpy(c["pd_points"]).to(DEV), torch.from_numpy(c["gt_points"]).to(DEV), 0.1)
    seg_ids = [int(s) for s in np.unique(c["pd_segments"]) if s != 0]
    gt_ids = sorted(i for i, n in c["instance2label"].items() if n != "none")
    case = dict(c, nn_index=nn.cpu().numpy().astype(np.int64), segment_ids=seg_ids, gt_ids=gt_ids)
    p = dict(DEFAULTS, min_seg_size=12)
    assert len(assert_overlap_is_loops(assert_dev_is_host(case, p), case, p)) > 0


def test_overlap_of_many_segments_with_large_ids():
    """300 segments x 200 instances, segment ids up to 60 000 (not ascending in the list), instance ids up to 5 000; a no-segment call."""
    _need_gpu()
    rng = np.random.default_rng(15)
    seg_ids = rng.choice(np.arange(1, 60001), size=300, replace=False)
    seg_ids[0] = 60000
    gt_all = rng.choice(np.arange(1, 5001), size=260, replace=False)
    gt_ids = gt_all[:200]                                              # 60 instances without a label
    G, Q = 5000, 120000
    gt_inst = gt_all[rng.integers(0, 260, size=G)]
    home = rng.integers(0, G, size=300)                                # a segment's points mostly land near one annotated point's instance
    seg_slot = rng.integers(0, 330, size=Q)                            # slots 300.. are segments that are not asked for
    nn = np.where(rng.random(Q) < 0.6, home[np.minimum(seg_slot, 299)], rng.integers(-1, G, size=Q))
    pd_seg = np.where(seg_slot < 300, seg_ids[np.minimum(seg_slot, 299)], 60001 + seg_slot)
    case = {"pd_segments": pd_seg, "nn_index": nn, "gt_instances": gt_inst, "segment_ids": seg_ids.tolist(), "gt_ids": gt_ids.tolist()}
    got = assert_dev_is_host(case, dict(DEFAULTS, min_seg_size=300))
    assert 20 < (got["match"] >= 0).sum() < 300 and got["size"].sum() == (seg_slot < 300).sum() and got["n_candidates"].max() > 64
    none = assert_dev_is_host(dict(case, segment_ids=[]), DEFAULTS)
    assert none["match"].shape == (0,) and none["counts"].shape == (0, 200)
    no_gt = assert_dev_is_host(dict(case, gt_ids=[]), DEFAULTS)
    assert (no_gt["match"] == -1).all() and no_gt["counts"].shape == (300, 0) and np.array_equal(no_gt["size"], got["size"])


# ---- a segmentation of one's own, scored ----------------------------------------------------------------------------------------------
CLASSES = ["chair", "table", "lamp", "floor"]


def _boxes_scan():
    """12 annotated boxes of 2400 points, 1.5 m apart.  The predicted cloud: 1800 jittered points of each, cut in two segments
    (100 + 2 i, 101 + 2 i) at the median x; of instance 10 the second segment keeps 300 points (below min_seg_size); the second
    halves of instances 11 and 12 share segment 900 evenly (rejected); instance 9 is labelled 'none'."""
    rng = np.random.default_rng(16)
    gt_pts, gt_inst, pd_pts, pd_seg = [], [], [], []
    for i in range(1, 13):
        centre = np.array([1.5 * ((i - 1) % 4), 1.5 * ((i - 1) // 4), 0.4])
        p = centre + rng.uniform(-0.3, 0.3, size=(2400, 3))
        gt_pts.append(p)
        gt_inst += [i] * 2400
        sub = p[rng.permutation(2400)[:1800]] + rng.normal(scale=0.004, size=(1800, 3))
        sub = sub[np.argsort(sub[:, 0])]
        first, second = sub[:900], sub[900:]
        if i == 10:
            second = second[:300]
        pd_pts += [first, second]
        pd_seg += [100 + 2 * i] * len(first) + [900 if i >= 11 else 101 + 2 * i] * len(second)
    order = rng.permutation(len(pd_seg))
    pd_mesh = {"points": np.concatenate(pd_pts)[order], "instances": np.asarray(pd_seg, dtype=np.int64)[order], "colors": None, "normals": None}
    order = rng.permutation(len(gt_inst))
    gt_mesh = {"points": np.concatenate(gt_pts)[order], "instances": np.asarray(gt_inst, dtype=np.int64)[order], "colors": None, "normals": None}
    labels = {i: CLASSES[i % 4] for i in range(1, 13)}
    labels[9] = "none"
    return pd_mesh, gt_mesh, labels


def test_a_segmentation_is_scored_end_to_end(tmp_path):
    _need_gpu()
    from vlsat_amd.model import VLSATModel
    pd_mesh, gt_mesh, labels = _boxes_scan()
    t = S.transfer_labels(pd_mesh, gt_mesh, labels, device=DEV)
    h = S.transfer_labels(pd_mesh, gt_mesh, labels, device=None)
    for name in ("instance2label", "segment_to_gt", "gt_to_segments", "n_without_correspondence"):
        assert getattr(t, name) == getattr(h, name), name
    for name in ("segment_ids", "size", "best", "second", "n_candidates", "counts", "matched_gt"):
        assert np.array_equal(getattr(t, name), getattr(h, name)), name
    # by hand: both halves of 1..8, the first half of 10, 11 and 12; nothing of 9 ('none'), not 121 (300 points), not 900 (a tie)
    by_hand = {100 + 2 * i + k: i for i in range(1, 9) for k in (0, 1)}
    by_hand.update({120: 10, 122: 11, 124: 12})
    assert t.segment_to_gt == by_hand and list(t.instance2label) == sorted(by_hand) and t.n_without_correspondence == 0
    assert t.instance2label == {s: labels[g] for s, g in sorted(by_hand.items())}
    k = t.segment_ids.tolist().index(900)
    assert t.size[k] == 1800 and t.best[k] == t.second[k] == 900 and t.n_candidates[k] == 2 and t.matched_gt[k] == -1
    k = t.segment_ids.tolist().index(121)
    assert t.size[k] == 300 and t.best[k] == 300 and t.matched_gt[k] == -1
    k = t.segment_ids.tolist().index(118)
    assert t.size[k] == 900 and t.best[k] == 0 and t.n_candidates[k] == 0            # on the 'none' instance: in size, not in count

    gt_rel = [[1, 2, 2, "left"], [2, 1, 3, "right"], [3, 9, 2, "left"], [10, 11, 6, "close by"], [12, 4, 15, "standing on"], [5, 6, 99, "same part"]]
    rel = S.inherit_relationships(t, gt_rel, RELS26)
    assert len(rel) == 4 + 4 + 0 + 1 + 2 + 0 and all(r[3] != "same part" for r in rel)
    assert [120, 122, RELS26.index("close by"), "close by"] in rel

    b = S.prepare_scan(pd_mesh, t.instance2label, CLASSES, rel, RELS26, num_points=64, seed=3, device=DEV)
    nodes = b["instance_ids"]
    assert nodes == sorted(by_hand)
    assert b["gt_class"].tolist() == [CLASSES.index(labels[by_hand[s]]) for s in nodes]
    edges = b["edge_indices"].cpu().numpy()
    want_rel = np.zeros((len(edges), len(RELS26)), dtype=np.float32)
    pos = {(nodes[a], nodes[c]): e for e, (a, c) in enumerate(edges.tolist())}
    for a, c, k, _ in rel:
        want_rel[pos[(a, c)], k] = 1
    assert np.array_equal(b["gt_rel_cls"].cpu().numpy(), want_rel) and want_rel.sum() == len(rel)
    sparse = S.prepare_scan(pd_mesh, t.instance2label, CLASSES, rel, RELS26, num_points=64, seed=3, device=DEV, edge_mode="proximity")
    assert sparse["instance_ids"] == nodes and 0 < len(sparse["edge_indices"]) < len(edges)

    cfg = VLSATConfig(N_LAYERS=2)
    m = VLSATModel(cfg, DEV).load_state(synth.make_weights(cfg)).eval()
    res = EV.validation(m, [b], device=DEV, workers=1)
    assert res == EV.validation(m, [b]) and len(res) > 0
    assert len(EV.validation(m, [sparse], device=DEV, workers=1)) > 0
    g3, g2 = m.decode_graph(b["obj_points"], b["obj_2d_feats"], b["edge_indices"].t().contiguous(), b["descriptor"], b["batch_ids"],
                            threshold=0.5, fc_sizes=b["fc_sizes"])
    entry = SG.to_annotation(g3, 0, b["edge_indices"], nodes, CLASSES + [f"c{i}" for i in range(4, cfg.num_obj_class)], ["none"] + RELS26, "scan-q")
    assert list(entry["objects"]) == [str(s) for s in nodes] and len(entry["relationships"]) == int(g3.n_valid[0]) and g2 is not None
    path = str(tmp_path / "relationships_segments.json")
    SG.write_annotations(path, [entry])
    assert S.read_relationships(path, ["scan-q"])[0]["scan-q_0"] == entry["relationships"]
