"""The proximity edge rule on the host (vlsat_amd/prep.py::proximity_edges_host, the numpy restatement of csrc/proximity.hip):
against a brute force written here independently, its stated properties, the reference's own padded boxes
(tests/golden/proximity_cases.npz, made by make_golden_proximity.py from data_preparation's ``instances_box``), and the annotation
coverage (the bindings: test_c_abi_cpu.py).  No comparison uses a tolerance.  No GPU."""
import os
import struct

import numpy as np
import pytest

import vlsat_amd  # noqa: F401
from vlsat_amd import lib as L, prep, scan as S, synth

F = np.float32


def boxes_of(pts, inst, ids):
    """lo.xyz, hi.xyz over all points of every id; an id without points gets +inf / -inf."""
    out = np.empty((len(ids), 6), dtype=np.float32)
    for k, i in enumerate(ids):
        p = pts[inst == i]
        out[k, :3] = p.min(0) if len(p) else np.inf
        out[k, 3:] = p.max(0) if len(p) else -np.inf
    return out


def room_boxes(n_obj, seed, pts_per_obj=6, extent=(4.0, 4.0, 2.0)):
    """Boxes of a small, crowded room: most objects have more candidates than the caps under test."""
    pts, inst = synth.make_room(n_obj, pts_per_obj, seed, extent)
    return boxes_of(pts, inst, range(1, n_obj + 1))


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def brute(boxes, n_per_scene, padding, max_neighbors):
    """Section 1 of the rule, pair by pair, every operation one np.float32 scalar operation."""
    pad = F(padding)
    edges, bids, ptr, off = [], [], [0], 0
    for s, n in enumerate(n_per_scene):
        cand = [[False] * n for _ in range(n)]
        key = [[None] * n for _ in range(n)]
        for i in range(n):
            for j in range(n):
                if i == j:
                    continue
                bi, bj = boxes[off + i], boxes[off + j]
                ok, gaps = True, []
                for a in range(3):
                    lo_i, hi_i, lo_j, hi_j = F(bi[a]), F(bi[3 + a]), F(bj[a]), F(bj[3 + a])
                    if not (F(lo_i - pad) < F(hi_j + pad) and F(lo_j - pad) < F(hi_i + pad)):
                        ok = False
                    gaps.append((lo_i, hi_i, lo_j, hi_j))
                cand[i][j] = ok
                if ok:
                    g = [max(F(0), max(F(lo_i - hi_j), F(lo_j - hi_i))) for lo_i, hi_i, lo_j, hi_j in gaps]
                    d = F(F(F(g[0] * g[0]) + F(g[1] * g[1])) + F(g[2] * g[2]))
                    key[i][j] = (_bits(d) << 32) | j
        keep = [[False] * n for _ in range(n)]
        for i in range(n):
            mine = sorted(key[i][j] for j in range(n) if cand[i][j])
            if max_neighbors > 0:
                mine = mine[:max_neighbors]
            for k in mine:
                keep[i][k & 0xFFFFFFFF] = True
        for i in range(n):
            for j in range(n):
                if cand[i][j] and (keep[i][j] or keep[j][i]):
                    edges.append((off + i, off + j))
        bids += [s] * n
        ptr.append(len(edges))
        off += n
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2).T
    return e, np.asarray(bids, dtype=np.int64).reshape(-1, 1), np.asarray(ptr, dtype=np.int64)


def assert_same(got, want):
    for g, w, name in zip(got, want, ("edge_indices", "batch_ids", "edge_ptr")):
        assert g.dtype == np.int64 and g.shape == w.shape and np.array_equal(g, w), name


@pytest.mark.parametrize("n_obj", [1, 2, 7, 65])
@pytest.mark.parametrize("padding", [0.0, 0.2])
def test_host_equals_the_brute_force_on_rooms(n_obj, padding):
    boxes = room_boxes(n_obj, 100 + n_obj)
    sizes = []
    for k in (0, 1, 3, n_obj):
        got = prep.proximity_edges_host(boxes, [n_obj], padding, k)
        assert_same(got, brute(boxes, [n_obj], padding, k))
        sizes.append(got[0].shape[1])
    if n_obj == 65 and padding == 0.2:
        assert sizes[1] < sizes[2] < sizes[0] == sizes[3]          # the caps bite; a cap of N is no cap


@pytest.mark.parametrize("padding", [0.0, 0.2])
@pytest.mark.parametrize("k", [0, 1, 3, 9])
def test_host_equals_the_brute_force_on_a_mixed_batch_with_an_empty_scene(padding, k):
    sizes = [7, 0, 1, 9, 2]
    boxes = np.concatenate([room_boxes(n, 200 + s) for s, n in enumerate(sizes) if n])
    got = prep.proximity_edges_host(boxes, sizes, padding, k)
    assert_same(got, brute(boxes, sizes, padding, k))
    assert got[2][1] == got[2][2] == got[2][3]                      # the empty scene and the one-object scene own no edge
    assert got[1].reshape(-1).tolist() == [0] * 7 + [2] + [3] * 9 + [4] * 2


@pytest.mark.parametrize("k", [0, 1, 3])
def test_the_list_is_symmetric_and_source_major_ascending(k):
    boxes = np.concatenate([room_boxes(65, 7), room_boxes(30, 8)])
    e, _, ptr = prep.proximity_edges_host(boxes, [65, 30], 0.2, k)
    pairs = list(zip(e[0].tolist(), e[1].tolist()))
    assert len(pairs) > 0 and set(pairs) == {(b, a) for a, b in pairs}
    assert pairs == sorted(pairs)                                   # source-major, targets ascending, scenes in node order
    assert all((a < 65) == (b < 65) and a != b for a, b in pairs)   # no edge between scenes, no self loop
    if k:
        n = np.array([65, 30])
        per_scene = np.diff(ptr)
        assert np.all(per_scene <= np.minimum(n * (n - 1), 2 * n * k))
    if k == 1:
        assert np.bincount(e[0]).max() > 1                          # an out-degree above the cap: the list is the union, made symmetric


def test_a_huge_padding_without_a_cap_is_the_fully_connected_list():
    sizes = [7, 1, 12]
    boxes = np.concatenate([room_boxes(n, 300 + n) for n in sizes])
    e, bids, ptr = prep.proximity_edges_host(boxes, sizes, 1e3, 0)
    want, off = [], 0
    for n in sizes:
        want.append(S.edge_list(list(range(n)), [], all_edge=True) + off)
        off += n
    assert np.array_equal(e.T, np.concatenate(want))
    assert ptr.tolist() == [0, 42, 42, 42 + 132]
    both = prep.proximity_edges(boxes, sizes, 1e3, 0)               # no device tensor: the same host path, as torch tensors
    assert np.array_equal(both[0].numpy(), e) and np.array_equal(both[1].numpy(), bids) and np.array_equal(both[2].numpy(), ptr)


def test_touching_boxes_are_not_neighbours_at_zero_padding():
    boxes = np.array([[0, 0, 0, 1, 1, 1], [1, 0, 0, 2, 1, 1], [0.5, 0.5, 0.5, 1.5, 1.5, 1.5]], dtype=np.float32)
    e = prep.proximity_edges_host(boxes, [3], 0.0, 0)[0]
    assert sorted(zip(*e.tolist())) == [(0, 2), (1, 2), (2, 0), (2, 1)]          # 0 and 1 share a face only: strict inequality
    e = prep.proximity_edges_host(boxes, [3], np.nextafter(F(0), F(1)), 0)[0]    # the smallest padding is absorbed by the rounding ...
    assert e.shape[1] == 4
    assert prep.proximity_edges_host(boxes, [3], 1e-3, 0)[0].shape[1] == 6       # ... a real one connects them


def test_an_instance_without_points_has_no_edges():
    pts, inst = synth.make_room(6, 5, 1)
    boxes = boxes_of(pts, inst, [1, 2, 99, 3, 4, 5, 6])
    assert np.all(np.isposinf(boxes[2, :3])) and np.all(np.isneginf(boxes[2, 3:]))
    for k in (0, 2):
        e = prep.proximity_edges_host(boxes, [7], 1e3, k)[0]
        assert 2 not in e and e.shape[1] > 0
        assert_same(prep.proximity_edges_host(boxes, [7], 1e3, k), brute(boxes, [7], 1e3, k))
    assert prep.proximity_edges_host(boxes, [7], 1e3, 0)[0].shape[1] == 6 * 5


def tie_boxes():
    """Node 0 and five identical boxes at the same distance from it, then one farther away: every distance from 0 ties."""
    same = [2.0, 0.0, 0.0, 3.0, 1.0, 1.0]
    return np.array([[0, 0, 0, 1, 1, 1]] + [same] * 5 + [[0, 3.0, 0, 1, 4.0, 1]], dtype=np.float32)


def test_ties_keep_the_lowest_indices():
    boxes = tie_boxes()
    e = prep.proximity_edges_host(boxes, [7], 5.0, 2)[0]
    assert_same(prep.proximity_edges_host(boxes, [7], 5.0, 2), brute(boxes, [7], 5.0, 2))
    # from 0 the five identical boxes are at d = 1 and node 6 at d = 4: 0 keeps the lowest two indices, 1 and 2.  The identical boxes
    # are at d = 0 from each other: each keeps the lowest two of the others.  Node 6 has 0 at d = 4 and the five at d = 5: it keeps 0
    # and, of the tie, 1.  The emitted list is the union made symmetric.
    assert e[1][e[0] == 0].tolist() == [1, 2, 6]                    # keeps 1, 2; kept by 6
    assert e[1][e[0] == 6].tolist() == [0, 1]
    assert e[1][e[0] == 3].tolist() == [1, 2]                       # keeps 1, 2; nobody else ranks 3 that 3 does not keep
    assert e[1][e[0] == 5].tolist() == [1, 2]
    assert e[1][e[0] == 1].tolist() == [0, 2, 3, 4, 5, 6]           # keeps 2, 3; kept by 0, 2, 3, 4, 5 and 6: six edges under a cap of two


def test_padded_boxes_and_candidates_equal_the_reference(golden_dir):
    z = np.load(os.path.join(golden_dir, "proximity_cases.npz"))
    mesh = S.read_ply(os.path.join(golden_dir, "scan_small.ply"))
    rel, objs, _ = S.read_relationships(os.path.join(golden_dir, "scan_small_relationships.json"), ["scan-a"])
    nodes = S.scene_nodes(mesh["instances"], objs["scan-a_0"])
    assert nodes == z["nodes"].tolist()
    boxes = boxes_of(mesh["points"].astype(np.float32), mesh["instances"], nodes)
    pad = F(float(z["padding"]))
    lo, hi = boxes[:, :3] - pad, boxes[:, 3:] + pad                # one fp32 operation per side, as instances_box
    assert lo.dtype == np.float32 and np.array_equal(lo, z["box_lo"]) and np.array_equal(hi, z["box_hi"])
    n = len(nodes)
    e = prep.proximity_edges_host(boxes, [n], float(z["padding"]), 0)[0]
    got = np.zeros((n, n), dtype=bool)
    got[e[0], e[1]] = True
    want = z["intersect"] & ~np.eye(n, dtype=bool)
    assert np.array_equal(got, want) and 0 < want.sum() < n * (n - 1)


def test_annotation_coverage_on_the_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "proximity_cases.npz"))
    rel, objs, _ = S.read_relationships(os.path.join(golden_dir, "scan_small_relationships.json"), ["scan-a"])
    rel, nodes = rel["scan-a_0"], z["nodes"].tolist()              # [5, 1, 9, 2, 40]
    # annotated pairs between nodes: (5,1) twice, (9,1), (5,9) twice, (2,1), (40,5), (1,40); 77 owns no point -> 6 distinct
    full = S.edge_list(nodes, rel, all_edge=True)
    assert S.annotation_coverage(nodes, full, rel) == (6, 6)
    assert S.annotation_coverage(nodes, S.edge_list(nodes, rel, all_edge=False), rel) == (6, 6)
    assert S.annotation_coverage(nodes, np.zeros((0, 2), dtype=np.int64), rel) == (0, 6)
    assert S.annotation_coverage(nodes, np.array([[0, 1], [1, 0], [3, 1]]), rel) == (2, 6)       # (5,1) and (2,1); (1,5) is not annotated
    n = len(nodes)
    inter = z["intersect"] & ~np.eye(n, dtype=bool)
    kept, total = S.annotation_coverage(nodes, np.argwhere(inter), rel)
    pos = {i: k for k, i in enumerate(nodes)}
    want = len({(r[0], r[1]) for r in rel if r[0] in pos and r[1] in pos and inter[pos[r[0]], pos[r[1]]]})
    assert total == 6 and kept == want


def test_bad_arguments_are_refused():
    boxes = room_boxes(3, 1)
    with pytest.raises(L.VlsatError):
        prep.proximity_edges_host(boxes, [2], 0.2, 0)
    with pytest.raises(L.VlsatError):
        prep.proximity_edges_host(boxes, [3], -0.1, 0)
    with pytest.raises(S.ScanError, match="edge_mode"):
        S.prepare_scan({"instances": np.array([1]), "points": np.zeros((1, 3))}, {1: "chair"}, ["chair"], [], ["left"], 4, 0,
                       device="cpu", edge_mode="nearest")


def test_make_room_is_deterministic_and_has_spatial_structure():
    a, ia = synth.make_room(40, 16, 5)
    b, ib = synth.make_room(40, 16, 5)
    assert a.dtype == np.float32 and a.shape == (640, 3) and ia.dtype == np.int32 and np.array_equal(a, b) and np.array_equal(ia, ib)
    assert not np.array_equal(a, synth.make_room(40, 16, 6)[0])
    assert sorted(set(ia.tolist())) == list(range(1, 41))
    e = prep.proximity_edges_host(boxes_of(a, ia, range(1, 41)), [40], 0.2, 0)[0]
    assert 0 < e.shape[1] < 40 * 39 // 4                            # far from fully connected
