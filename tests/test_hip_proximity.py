"""Proximity-pruned edge lists on the device (csrc/proximity.hip: vlsat_instance_boxes, vlsat_proximity_count / _fill) against the
host restatement of the rule (prep.proximity_edges_host, itself checked against a brute force in test_proximity_cpu.py), element
for element -- no tolerance anywhere -- and the proximity batch through prepare_scan, decode, export and validation.  Needs an MI355X."""
import json
import os

import numpy as np
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import VLSATConfig, evaluate as EV, lib as L, prep, scan as S, scene_graph as SG, synth
from test_proximity_cpu import boxes_of, room_boxes, tie_boxes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path cannot run and there is no fallback")


def dev_edges(boxes, sizes, padding, k):
    out = prep.proximity_edges(torch.from_numpy(boxes).to(DEV), sizes, padding, k)
    assert all(t.is_cuda and t.dtype == torch.int64 for t in out)
    return tuple(t.cpu().numpy() for t in out)


def assert_same(got, want, what):
    for g, w, name in zip(got, want, ("edge_indices", "batch_ids", "edge_ptr")):
        assert g.shape == w.shape and np.array_equal(g, w), (what, name)


def dev_boxes(pts, inst, ids, map_size):
    b = prep.instance_boxes(torch.from_numpy(pts).to(DEV), torch.from_numpy(inst.astype(np.int32)).to(DEV),
                            torch.tensor(list(ids), dtype=torch.int32), map_size)
    assert b.is_cuda and b.dtype == torch.float32 and b.shape == (len(ids), 6)
    return b.cpu().numpy()


# ---- boxes -----------------------------------------------------------------------------------------------------------------------
def test_instance_boxes_equal_numpy_min_and_max():
    """make_room(70, 50): point order shuffled, background points (id 0), ids the map cannot hold (negative, >= map_size), the ids
    requested in another order than they occur, and one requested id without points (+inf / -inf)."""
    _need_gpu()
    pts, inst = synth.make_room(70, 50, 11)
    g = np.random.default_rng(3)
    extra = g.uniform(-50, 50, (300, 3)).astype(np.float32)             # far outside every object: would widen a box if counted
    pts = np.concatenate([pts, extra])
    inst = np.concatenate([inst, np.repeat(np.array([0, -3, 128, 100000], dtype=np.int32), 75)])
    pts[0, 0] = -0.0                                                    # (a signed zero: boxes compare with array_equal, -0.0 == 0.0)
    order = g.permutation(len(pts))
    pts, inst = np.ascontiguousarray(pts[order]), inst[order]
    ids = [int(i) for i in g.permutation(np.arange(1, 71))] + [99]
    want = boxes_of(pts, inst, ids)
    got = dev_boxes(pts, inst, ids, map_size=128)
    assert np.array_equal(got, want)
    assert np.all(np.isposinf(got[-1, :3])) and np.all(np.isneginf(got[-1, 3:]))


def test_instance_boxes_above_the_lds_table():
    """More objects than the block's LDS table holds: every point sends its own atomics (the other branch of the kernel)."""
    _need_gpu()
    n = prep.proximity_lds_boxes() + 1
    pts, inst = synth.make_room(n, 5, 12)
    order = np.random.default_rng(4).permutation(len(pts))
    pts, inst = np.ascontiguousarray(pts[order]), inst[order]
    ids = list(range(1, n + 1))
    assert np.array_equal(dev_boxes(pts, inst, ids, map_size=n + 1), boxes_of(pts, inst, ids))


def test_instance_boxes_equal_the_reference_on_the_fixture_mesh(golden_dir):
    _need_gpu()
    z = np.load(os.path.join(golden_dir, "proximity_cases.npz"))
    mesh = S.read_ply(os.path.join(golden_dir, "scan_small.ply"))
    got = dev_boxes(mesh["points"].astype(np.float32), mesh["instances"], z["nodes"].tolist(), map_size=65536)
    pad = np.float32(float(z["padding"]))
    assert np.array_equal(got[:, :3] - pad, z["box_lo"]) and np.array_equal(got[:, 3:] + pad, z["box_hi"])


# ---- edges -----------------------------------------------------------------------------------------------------------------------
def _crowded(n, seed):
    side = max(2.0, 0.5 * np.sqrt(n))                                   # about four objects per square metre: the caps bite
    return room_boxes(n, seed, extent=(side, side, 2.0))


@pytest.mark.parametrize("n_obj", [1, 2, 63, 64, 65, 257, 300, 600, 601])
def test_edges_equal_the_host_rule_on_one_scene(n_obj):
    """Wave boundary (63 / 64 / 65 targets), 300 objects (38 blocks of 8 rows, five lane passes per row); no cap, a cap that bites
    (3, 8), a cap of N and one above N; padding 0 and 0.2.  The 256 threads of the row-count scan own runs of two at 257 and 300 rows
    (thread 128 owns the odd row of 257; the threads after it, and from 150 on, own nothing) and runs of three at 600 and 601 (200
    threads, then one ragged run of a single row)."""
    _need_gpu()
    boxes = _crowded(n_obj, 400 + n_obj)
    sizes = {}
    for padding in (0.0, 0.2):
        for k in (0, 3, 8, n_obj, n_obj + 7):
            want = prep.proximity_edges_host(boxes, [n_obj], padding, k)
            assert_same(dev_edges(boxes, [n_obj], padding, k), want, (n_obj, padding, k))
            sizes[padding, k] = want[0].shape[1]
    if n_obj >= 63:
        assert sizes[0.2, 3] < sizes[0.2, 8] < sizes[0.2, 0] == sizes[0.2, n_obj] == sizes[0.2, n_obj + 7]


@pytest.mark.parametrize("sizes", ["above", "straddle"])
def test_edges_equal_the_host_rule_without_lds_staging(sizes):
    """One scene above the staging limit (every block reads global memory), and two scenes whose border blocks need a span above
    the limit while all other blocks stage theirs: both branches in one launch."""
    _need_gpu()
    limit = prep.proximity_lds_boxes()
    sizes = [limit + 1] if sizes == "above" else [limit - 4, 10]
    boxes = np.concatenate([room_boxes(n, 500 + n, extent=(16.0, 16.0, 2.0)) for n in sizes])
    for k in (0, 4):
        want = prep.proximity_edges_host(boxes, sizes, 0.2, k)
        assert want[0].shape[1] > sum(sizes)
        assert_same(dev_edges(boxes, sizes, 0.2, k), want, (sizes, k))


@pytest.mark.parametrize("k", [0, 2, 5])
def test_edges_equal_the_host_rule_on_a_batch_with_an_empty_and_a_one_object_scene(k):
    _need_gpu()
    sizes = [7, 0, 1, 65, 30]
    boxes = np.concatenate([_crowded(n, 600 + s) for s, n in enumerate(sizes) if n])
    for padding in (0.0, 0.2):
        want = prep.proximity_edges_host(boxes, sizes, padding, k)
        assert_same(dev_edges(boxes, sizes, padding, k), want, (padding, k))
    assert want[2][1] == want[2][2] == want[2][3] and want[2][4] > want[2][3]
    trailing = prep.proximity_edges_host(boxes[:7], [7, 0], 0.2, k)     # the empty scene last
    assert_same(dev_edges(boxes[:7], [7, 0], 0.2, k), trailing, "trailing empty scene")


def test_ties_and_empty_boxes_follow_the_host_rule():
    _need_gpu()
    boxes = tie_boxes()
    for k in (1, 2, 3):
        assert_same(dev_edges(boxes, [7], 5.0, k), prep.proximity_edges_host(boxes, [7], 5.0, k), ("ties", k))
    got = dev_edges(boxes, [7], 5.0, 2)[0]
    assert got[1][got[0] == 0].tolist() == [1, 2, 6] and got[1][got[0] == 1].tolist() == [0, 2, 3, 4, 5, 6]
    holes = _crowded(20, 77)
    holes[[0, 7, 19], :3], holes[[0, 7, 19], 3:] = np.inf, -np.inf      # instances without points
    for k in (0, 3):
        want = prep.proximity_edges_host(holes, [20], 0.2, k)
        assert not np.isin(want[0], [0, 7, 19]).any() and want[0].shape[1] > 0
        assert_same(dev_edges(holes, [20], 0.2, k), want, ("empty boxes", k))
    touch = np.array([[0, 0, 0, 1, 1, 1], [1, 0, 0, 2, 1, 1], [0.5, 0.5, 0.5, 1.5, 1.5, 1.5]], dtype=np.float32)
    assert sorted(zip(*dev_edges(touch, [3], 0.0, 0)[0].tolist())) == [(0, 2), (1, 2), (2, 0), (2, 1)]      # strict inequality


def test_a_large_padding_without_a_cap_is_fc_edges():
    _need_gpu()
    sizes = [7, 1, 12, 65]
    boxes = np.concatenate([room_boxes(n, 700 + n) for n in sizes])
    e, bids, ptr = prep.proximity_edges(torch.from_numpy(boxes).to(DEV), sizes, 1e3, 0)
    fe, fb = prep.fc_edges(sizes, DEV)
    assert torch.equal(e, fe) and torch.equal(bids, fb)
    assert ptr.tolist() == np.cumsum([0] + [n * (n - 1) for n in sizes]).tolist()


def test_fill_refuses_a_capacity_below_the_count_and_stays_inside_a_larger_one():
    _need_gpu()
    lib = L.load()
    n = 65
    boxes = torch.from_numpy(_crowded(n, 800)).to(DEV)
    node_ptr = torch.tensor([0, n], dtype=torch.int32, device=DEV)
    scratch = torch.empty(int(lib.vlsat_proximity_scratch_bytes(n)), dtype=torch.uint8, device=DEV)
    edge_ptr = torch.empty(2, dtype=torch.int64, device=DEV)
    bids = torch.empty(n, dtype=torch.int64, device=DEV)
    args = (boxes.data_ptr(), node_ptr.data_ptr(), 1, n, 0.2, 3)
    L.check(lib.vlsat_proximity_count(*args, scratch.data_ptr(), edge_ptr.data_ptr(), bids.data_ptr(), L.stream_ptr()))
    count = int(edge_ptr[1])
    want = prep.proximity_edges_host(boxes.cpu().numpy(), [n], 0.2, 3)[0]
    assert count == want.shape[1] and count > n
    guard = -7
    small = torch.full((2 * count + 64,), guard, dtype=torch.int64, device=DEV)
    rc = lib.vlsat_proximity_fill(*args, scratch.data_ptr(), count, count - 1, small.data_ptr(), L.stream_ptr())
    assert rc != 0 and "capacity" in lib.vlsat_last_error().decode()
    torch.cuda.synchronize()
    assert bool((small == guard).all())                                 # refused: nothing written, the guard after `capacity` included
    cap = count + 5
    big = torch.full((2 * cap + 64,), guard, dtype=torch.int64, device=DEV)
    L.check(lib.vlsat_proximity_fill(*args, scratch.data_ptr(), count, cap, big.data_ptr(), L.stream_ptr()))
    big = big.cpu().numpy()
    assert np.array_equal(big[:count], want[0]) and np.array_equal(big[cap:cap + count], want[1])       # row stride = capacity
    assert np.all(big[count:cap] == guard) and np.all(big[cap + count:] == guard)


# ---- the proximity batch through the pipeline ------------------------------------------------------------------------------------------
def test_a_proximity_batch_runs_through_decode_export_and_validation(golden_dir, tmp_path):
    """prepare_scan(edge_mode="proximity") on the fixture mesh == the fully connected preparation of the same seed with the edge list
    and its labels replaced by the host-built ones; the batch is decoded, exported and read back; validation on it equals validation
    on the host-built batch exactly."""
    _need_gpu()
    from vlsat_amd.model import VLSATModel
    e = json.load(open(os.path.join(golden_dir, "scan_small_expect.json")))
    ply = os.path.join(golden_dir, "scan_small.ply")
    rel, objs, _ = S.read_relationships(os.path.join(golden_dir, "scan_small_relationships.json"), ["scan-a"])
    rel, objs = rel["scan-a_0"], objs["scan-a_0"]
    classes, relations = e["classes"], e["relations"]
    feats = np.random.default_rng(0).normal(size=(100, 512)).astype(np.float32)
    kw = dict(num_points=32, seed=4, device=DEV, feature_loader=lambda i, name: feats[i])
    b = S.prepare_scan(ply, objs, classes, rel, relations, edge_mode="proximity", padding=0.2, **kw)
    full = S.prepare_scan(ply, objs, classes, rel, relations, **kw)
    mesh = S.read_ply(ply)
    nodes = b["instance_ids"]
    boxes = boxes_of(mesh["points"].astype(np.float32), mesh["instances"], nodes)
    edges = np.ascontiguousarray(prep.proximity_edges_host(boxes, [len(nodes)], 0.2, 0)[0].T)
    assert 0 < len(edges) < len(nodes) * (len(nodes) - 1)                # the fixture is really pruned (12 of 20 pairs)
    gt_class, gt_rel = S.ground_truth(nodes, edges, objs, classes, rel, relations, True)
    host = dict(full, edge_indices=torch.from_numpy(edges).to(DEV), gt_rel_cls=torch.from_numpy(gt_rel).to(DEV))
    del host["fc_sizes"]
    assert "fc_sizes" not in b and np.array_equal(b["boxes"].cpu().numpy(), boxes)
    for name in ("obj_points", "obj_2d_feats", "descriptor", "edge_indices", "batch_ids", "gt_class", "gt_rel_cls", "choice"):
        assert b[name].dtype == host[name].dtype and torch.equal(b[name], host[name]), name
    assert S.annotation_coverage(nodes, edges, rel) == S.annotation_coverage(nodes, b["edge_indices"].cpu().numpy(), rel)
    capped = S.prepare_scan(ply, objs, classes, rel, relations, edge_mode="proximity", padding=0.2, max_neighbors=1, **kw)
    want1 = prep.proximity_edges_host(boxes, [len(nodes)], 0.2, 1)[0].T
    assert np.array_equal(capped["edge_indices"].cpu().numpy(), want1) and len(want1) < len(edges)

    cfg = VLSATConfig(N_LAYERS=2)
    m = VLSATModel(cfg, DEV).load_state(synth.make_weights(cfg)).eval()
    r3 = m.forward_3d(b["obj_points"], b["edge_indices"].t().contiguous(), b["descriptor"], b["batch_ids"])[1]
    assert r3.shape == (len(edges), len(relations)) and bool(torch.isfinite(r3).all())
    (g3, g2), = list(EV.decode(m, [b], threshold=float(r3.median()), n_labels=3, max_rel=1024))
    assert int(g3.n_valid[0]) > 0 and g2 is not None
    full_names = ["none"] + list(relations)
    entry = SG.to_annotation(g3, 0, b["edge_indices"], nodes, classes, full_names, "scan-p")
    path = str(tmp_path / "relationships_predicted.json")
    SG.write_annotations(path, [entry])
    back_rel, back_objs, back_scans = S.read_relationships(path, ["scan-p"])
    assert back_scans == ["scan-p_0"] and list(back_objs["scan-p_0"]) == nodes
    assert back_rel["scan-p_0"] == entry["relationships"] and len(entry["relationships"]) == int(g3.n_valid[0])
    pairs = {(a, c) for a, c in edges.tolist()}
    pos = {i: k for k, i in enumerate(nodes)}
    assert all((pos[r[0]], pos[r[1]]) in pairs for r in entry["relationships"])      # every asserted relation lies on a kept edge
    (h3, _), = list(EV.decode(m, [host], threshold=float(r3.median()), n_labels=3, max_rel=1024))
    assert SG.to_annotation(h3, 0, host["edge_indices"], nodes, classes, full_names, "scan-p") == entry

    assert EV.validation(m, [b, b], device=DEV, workers=1) == EV.validation(m, [host, host], device=DEV, workers=1)     # counts on the device
    assert EV.validation(m, [b, b]) == EV.validation(m, [host, host])                                                   # reference-compatible loop
