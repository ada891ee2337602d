"""A scan split into sub-scenes and the per-split graphs fused, on the GPU (csrc/scene_split.hip via vlsat_split_seeds /
vlsat_split_groups / vlsat_fuse_splits): every index, mask, count, pooled fp32 probability and maximum equal, bit for bit, to the host
restatement AND to the rules written as loops (split_checks) -- several blocks and a ragged last one, 37 segment ids across a mask word
with 0 and ids above 4096, one vertex, one seed, the reference's recorded runs, the fusion clauses, two calls in a row, and the whole
route split -> prepare -> forward -> fuse -> decode -> annotation."""
import os

import numpy as np
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import evaluate as EV, lib as L, metrics as M, prep as P, scan as S, scene_graph as SG

from split_checks import assert_fused, brute_fuse, brute_groups, brute_seeds, cloud, fuse_case, random_splits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "split_cases.npz")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path cannot run and there is no fallback")


def _split(pts, seg, ids, distance=1.0, bbox=0.75, min_seg=5, seed=0, ranks=None):
    """device seeds and groups, each checked against the host restatement -> (seeds, groups, counts, keep)."""
    d_pts, d_seg = torch.from_numpy(pts).to(DEV), torch.from_numpy(np.asarray(seg, dtype=np.int32)).to(DEV)
    seeds = P.split_seeds(d_pts, distance, seed, ranks)
    assert seeds.is_cuda and seeds.dtype == torch.int32
    want = P.split_seeds_host(pts, distance, seed, ranks)
    assert seeds.cpu().numpy().tolist() == want.tolist()
    got = P.split_groups(d_pts, d_seg, ids, seeds, bbox, min_seg)
    ref = P.split_groups_host(pts, seg, ids, want, bbox, min_seg)
    assert got[0] == ref[0] and got[1].tolist() == ref[1].tolist() and got[2].tolist() == ref[2].tolist() and np.array_equal(got[3], ref[3])
    return want.tolist(), got[0], got[1].tolist(), got[2].tolist()


def test_4099_vertices_37_ids_equal_host_and_loops():
    _need_gpu()
    pts, seg = cloud(4099, 11)                                                    # 5 blocks of 1024, the last one ragged
    ids = np.unique(seg)
    assert len(ids) == 37 and ids[0] == 0 and (ids > 4096).sum() >= 5
    seeds, groups, counts, keep = _split(pts, seg, ids, seed=11)
    assert 8 <= len(seeds) <= 20 and seeds == brute_seeds(pts, 1.0, 11)
    assert (groups, counts, keep) == brute_groups(pts, seg, ids, seeds)
    assert any(0 in g for g in groups) and any(g and g[-1] > 4096 for g in groups)
    again = _split(pts, seg, ids, seed=11)                                        # two calls in a row: identical
    assert again == (seeds, groups, counts, keep)
    other = _split(pts, seg, ids[::-1].copy(), distance=0.7, bbox=0.4, min_seg=9, seed=12)            # other slots, a dropped group
    assert not all(other[3]) and other[0] == brute_seeds(pts, 0.7, 12)


def test_one_vertex_one_seed_and_non_finite():
    _need_gpu()
    one = np.asarray([[3, 4, 5]], dtype=np.float32)
    assert _split(one, [4], [4], min_seg=1) == ([0], [[4]], [1], [True])
    near, seg = cloud(1500, 2, extent=(0.6, 0.5, 0.4))                            # all within the distance: K = 1, two blocks
    seeds, groups, _, _ = _split(near, seg, np.unique(seg), seed=2)
    assert len(seeds) == 1 and groups == brute_groups(near, seg, np.unique(seg), seeds)[0]
    bad, seg = cloud(1300, 6)
    bad[10, 0], bad[1200, 2], bad[30, 1] = np.nan, np.inf, -np.inf
    seeds = _split(bad, seg, np.unique(seg), seed=1)[0]
    assert seeds == brute_seeds(bad, 1.0, 1) and not {10, 1200, 30} & set(seeds[1:])
    assert _split(bad, seg, np.unique(seg), ranks=[10])[0] == [10]


def test_seeds_with_two_blocks_per_thread_of_the_pick():
    """1024 * 1024 + 1025 vertices are 1026 blocks of 1024: the 1024 threads of the pick own runs of two blocks (thread 512 the last
    full block and the one-vertex block after it, the threads after it nothing).  Three clusters far apart give three seeds; the ranks
    put the second seed into block 1, the second block of thread 0's run, and the third into the last, partial block."""
    _need_gpu()
    v = 1024 * 1024 + 1025
    g = np.random.default_rng(21)
    cluster = g.integers(0, 3, v)
    cluster[0], cluster[-1] = 0, 2
    pts = (np.asarray([[0, 0, 0], [10, 0, 0], [0, 10, 0]], dtype=np.float32)[cluster] + g.random((v, 3)) * 0.1).astype(np.float32)
    other = np.nonzero(cluster != 0)[0]
    r1 = int((other < 1024).sum()) + 5                                            # the sixth selectable vertex of block 1
    second = int(other[r1])
    assert 1024 <= second < 2048 and cluster[second] == 1                         # (seed 21 draws it so; then cluster 2 is what is left)
    ranks = [0, r1, int((cluster == 2).sum()) - 1]
    want = P.split_seeds_host(pts, 1.0, 0, ranks)
    assert want.tolist() == [0, second, v - 1]
    got = P.split_seeds(torch.from_numpy(pts).to(DEV), 1.0, 0, ranks, max_seeds=5)
    assert got.cpu().numpy().tolist() == want.tolist()


def test_golden_reference_runs_replay_on_the_device():
    _need_gpu()
    z = np.load(GOLDEN)
    for k in range(int(z["n_cases"])):
        pts, seg = z[f"pts_{k}"], z[f"seg_{k}"]
        distance, bbox, min_seg = z[f"params_{k}"].tolist()
        seeds, groups, _, keep = _split(pts, seg, np.unique(seg), distance, bbox, int(min_seg), ranks=z[f"ranks_{k}"])
        ptr, flat = z[f"group_ptr_{k}"].tolist(), z[f"group_ids_{k}"].tolist()
        assert seeds == z[f"seeds_{k}"].tolist(), k
        assert [g for g, kept in zip(groups, keep) if kept] == [flat[a:b] for a, b in zip(ptr, ptr[1:])], k


def test_rank_errors_are_reported_not_faults():
    _need_gpu()
    pts, _ = cloud(2100, 1)
    d = torch.from_numpy(pts).to(DEV)
    first = int(P.split_seeds_host(pts, 1.0, 1)[0])
    for ranks, word in (([first, 0], "ran out"), ([2100], "rank"), ([first, 5000], "rank")):
        with pytest.raises(L.VlsatError, match=word):
            P.split_seeds(d, 1.0, 0, ranks)
    with pytest.raises(L.VlsatError, match="max_seeds"):
        P.split_seeds(d, 1.0, 1, max_seeds=2)
    lib = L.load()
    assert lib.vlsat_split_seeds(d.data_ptr(), 2100, 0.0, 0, None, 0, 4, d.data_ptr(), d.data_ptr(), d.data_ptr(), L.stream_ptr()) == -1
    assert "distance" in lib.vlsat_last_error().decode() and int(lib.vlsat_split_seeds_scratch_bytes(0)) == 0
    assert int(lib.vlsat_fuse_splits_scratch_bytes(20000, 3, 5, 2, 64)) == 0 and int(lib.vlsat_fuse_splits_scratch_bytes(4, 3, 5, 33, 64)) == 0
    torch.cuda.synchronize()


# ---- fusion -------------------------------------------------------------------------------------------------------------------------------
def _both(c, trim=True, device_ids=False, **kw):
    d = lambda t: None if t is None else t.to(DEV)
    ids = torch.tensor(c["row_instance"], dtype=torch.int32, device=DEV) if device_ids else c["row_instance"]
    got = M.fuse_splits(d(c["obj_probs"]), d(c["rel_probs"]), d(c["edges"]), ids, d(c["weights"]), obj_probs=d(c["obj_probs"]),
                        rel_probs=d(c["rel_probs"]), trim=trim, **kw)
    want = M.fuse_splits_host(c["obj_probs"], c["rel_probs"], c["edges"], c["row_instance"] if not device_ids else ids.cpu(), c["weights"],
                              obj_probs=c["obj_probs"], rel_probs=c["rel_probs"], trim=trim, **kw)
    return got, want


FUSE = {
    "150_rows_6_splits_60_ids": lambda: random_splits(6, 60, 25, 1000, 21, weights="mixed", c=160, r=26),
    "id_in_three_splits": lambda: fuse_case([5, 9, 2, 9, 7, 5, 9, 40], [(0, 1), (1, 0), (3, 4), (5, 6), (6, 7), (2, 0)], weights="mixed"),
    "edge_in_two_splits": lambda: fuse_case([3, 8, 8, 3, 1], [(0, 1), (3, 2), (1, 0), (4, 3), (0, 1)]),
    "weights": lambda: fuse_case([4, 4, 4, 2, 2], [(0, 3), (4, 1)], c=7, weights=[1, 250000, 3, 0.5, 12]),
    "dropped_edges": lambda: fuse_case([6, 6, 1, 0], [(0, 0), (0, 1), (1, 0), (2, 9), (-1, 2), (4, 0), (3, 2), (2, 3)]),
    "no_rows": lambda: fuse_case([], []),
    "no_edges": lambda: fuse_case([3, 1, 3], []),
    "one_class_one_predicate_70_rows_one_id": lambda: fuse_case([77] * 70 + [3], [(0, 70), (70, 69), (5, 6)], c=1, r=1, weights="mixed"),
    "1024_classes_32_predicates": lambda: random_splits(4, 50, 33, 600, 22, c=1024, r=32),
}


@pytest.mark.parametrize("name", list(FUSE))
def test_fusion_equals_host_and_loops(name):
    _need_gpu()
    c = FUSE[name]()
    got, want = _both(c)
    assert_fused(got, want, name)
    assert_fused(got, brute_fuse(c), name)
    assert_fused(_both(c)[0], got, name)                                          # two calls in a row: identical


def test_fusion_untrimmed_and_ids_on_the_device():
    _need_gpu()
    c = FUSE["150_rows_6_splits_60_ids"]()
    got, want = _both(c, trim=False)
    assert not got.trimmed and got.obj_probs.shape == want.obj_probs.shape and got.obj_ids.shape[0] == 150
    assert_fused(got, want)
    c = fuse_case([3, 70000, 3, 5, 64], [(0, 1), (1, 3), (0, 3), (4, 0)])
    got, want = _both(c, device_ids=True, map_size=64)                            # 70000 and 64 are outside a table of 64: no object
    assert_fused(got, want)
    assert_fused(got, brute_fuse(c, map_size=64))
    assert got.object.tolist() == [0, -1, 0, 1, -1] and got.edge_to_pair.tolist() == [-1, -1, 0, -1]


# ---- the whole route ----------------------------------------------------------------------------------------------------------------------
def test_split_prepare_forward_fuse_decode_annotation(tmp_path):
    _need_gpu()
    from vlsat_amd import VLSATConfig, synth
    from vlsat_amd.model import VLSATModel
    pts, inst = synth.make_room(40, 48, 3, extent=(4.0, 3.0, 2.5))
    mesh = {"points": pts.astype(np.float64), "instances": inst.astype(np.int64)}
    sp = S.split_scan(mesh, seed=5, device=DEV)
    host = S.split_scan(mesh, seed=5, device=None)
    assert sp.groups == host.groups and sp.seeds.tolist() == host.seeds.tolist() and len(sp.groups) >= 2
    cfg = VLSATConfig(N_LAYERS=1)
    classes = [f"c{k}" for k in range(cfg.num_obj_class)]
    names_full = ["none"] + [f"r{k}" for k in range(cfg.num_rel_class)]
    labels = {i: classes[i % 7] for i in range(1, 41)}
    batches = [S.prepare_scan(mesh, {i: labels[i] for i in g if i in labels}, classes, [], names_full[1:], 32, seed=k, device=DEV)
               for k, g in enumerate(sp.groups)]
    assert [b["instance_ids"] for b in batches] == sp.groups
    b = EV.merge_batches(batches)
    row_instance = [i for x in batches for i in x["instance_ids"]]
    weights = torch.cat([x["points_per_instance"] for x in batches]).float()
    m = VLSATModel(cfg, DEV).load_state(synth.make_weights(cfg)).eval()
    obj3, rel3 = m.forward_3d(b["obj_points"], b["edge_indices"].t().contiguous(), b["descriptor"], b["batch_ids"])
    thr = float(rel3.float().quantile(0.98))                                      # synthetic weights: nothing is calibrated
    g = M.fuse_splits(obj3, rel3, b["edge_indices"], row_instance, weights)
    want = M.fuse_splits_host(obj3.cpu(), rel3.cpu(), b["edge_indices"].cpu(), row_instance, weights.cpu(), obj_probs=M.softmax_rows(obj3).cpu())
    assert_fused(g, want)
    ids = sorted(set(row_instance))
    assert g.node_ids() == ids and len(ids) < len(row_instance) and int(g.pair_count.max()) >= 2          # ids and pairs recur across splits
    d = g.decode(threshold=thr, n_labels=2, max_rel=512)
    entry = SG.add_segments(SG.to_annotation(d, 0, g.pair_edges, g.node_ids(), classes, names_full, "room"), g, row_instance)
    assert len(entry["relationships"]) == int(d.n_valid[0]) > 0 and set(entry["objects"]) == {str(i) for i in ids}
    path = tmp_path / "relationships_fused.json"
    SG.write_annotations(path, [entry])
    rel, objs, scans = S.read_relationships(str(path), ["room"])
    assert scans == ["room_0"] and rel["room_0"] == entry["relationships"] and objs["room_0"] == {int(k): v for k, v in entry["objects"].items()}
