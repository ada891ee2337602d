"""A scan split into sub-scenes and the per-split graphs fused, on the host (vlsat_amd/prep.py::split_seeds_host / split_groups_host,
vlsat_amd/metrics.py::fuse_splits_host, the numpy restatements of csrc/scene_split.hip; include/vlsat_split.h states the rules): against
the rules written a second time as loops (split_checks), against what the reference's generate_groups returned
(tests/golden/split_cases.npz), one case per clause, and the build list (the exports: test_c_abi_cpu.py).  No comparison uses
a tolerance.  No GPU."""
import os

import numpy as np
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import lib as L, metrics as M, prep as P, scan as S, scene_graph as SG

from split_checks import F, assert_fused, brute_fuse, brute_groups, brute_seeds, cloud, draw, fuse_case, random_splits

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "split_cases.npz")


def groups_host(pts, seg, ids, seeds, bbox=0.75, min_seg=5):
    groups, counts, keep, mask = P.split_groups_host(pts, seg, ids, seeds, bbox, min_seg)
    return groups, counts.tolist(), keep.tolist(), mask


# ---- seeds and groups ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v,seed", [(700, 0), (333, 7), (64, 3)])
def test_host_rules_equal_the_loops(v, seed):
    pts, seg = cloud(v, seed)
    seeds = P.split_seeds_host(pts, 1.0, seed)
    assert seeds.tolist() == brute_seeds(pts, 1.0, seed) and seeds.dtype == np.int32
    assert seeds[0] == draw(seed, 0, v) == P.split_draw(seed, 0, v) and len(set(seeds.tolist())) == len(seeds) > 3
    ids = np.unique(seg)
    got = groups_host(pts, seg, ids, seeds)
    assert got[:3] == brute_groups(pts, seg, ids, seeds)
    assert all(sorted(g) == g for g in got[0]) and any(got[2]) and got[1] == [len(g) for g in got[0]]
    words = got[3]                                                                # the bit table says the same as the lists
    assert words.shape == (len(seeds), (len(ids) + 31) // 32) and words.dtype == np.uint32
    assert [[int(ids[s]) for s in range(len(ids)) if words[k, s >> 5] >> (s & 31) & 1] for k in range(len(seeds))] == got[0]


def test_golden_reference_run_replays():
    """What the reference's generate_groups drew and returned (make_golden_split.py), replayed through ``ranks``."""
    z = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 200_000 and int(z["n_cases"]) >= 3
    for k in range(int(z["n_cases"])):
        pts, seg = z[f"pts_{k}"], z[f"seg_{k}"]
        distance, bbox, min_seg = z[f"params_{k}"].tolist()
        seeds = P.split_seeds_host(pts, distance, 0, ranks=z[f"ranks_{k}"])
        assert seeds.tolist() == z[f"seeds_{k}"].tolist(), k
        assert brute_seeds(pts, distance, ranks=z[f"ranks_{k}"].tolist()) == seeds.tolist()
        groups, _, keep, _ = groups_host(pts, seg, np.unique(seg), seeds, bbox, int(min_seg))
        ptr, flat = z[f"group_ptr_{k}"].tolist(), z[f"group_ids_{k}"].tolist()
        assert [g for g, kept in zip(groups, keep) if kept] == [flat[a:b] for a, b in zip(ptr, ptr[1:])], k
        mesh = {"points": pts, "instances": seg}
        sp = S.split_scan(mesh, distance, bbox, int(min_seg), device=None, ranks=z[f"ranks_{k}"])
        assert sp.groups == [flat[a:b] for a, b in zip(ptr, ptr[1:])] and sp.seeds.tolist() == seeds.tolist()
        assert np.array_equal(sp.seed_points, pts[seeds]) and len(sp.kept) == len(sp.groups)
    assert len(z["seeds_3"]) == 1                                                 # the cloud inside one distance: one seed


def test_strict_inequalities_on_representable_coordinates():
    one_up = float(np.nextafter(F(1.0), F(2.0)))
    pts = np.asarray([[0, 0, 0], [1, 0, 0], [0, -1, 9], [0.6, 0.8, 0], [one_up, 0, 0]], dtype=F)      # |(0.6, 0.8)| is not exactly 1 in fp32
    assert P.split_seeds_host(pts[:3], 1.0, ranks=[0]).tolist() == [0]            # exactly at distance: not selectable (z is ignored)
    assert P.split_seeds_host(pts[[0, 1, 2, 4]], 1.0, ranks=[0, 0]).tolist() == [0, 3]                 # one ulp beyond: selectable
    assert P.split_seeds_host(pts, 1.0, ranks=[0, 0]).tolist() == brute_seeds(pts, 1.0, ranks=[0, 0])
    box = np.asarray([[0, 0, 0], [0.75, 0, 0], [0.5, 0.5, -0.5], [0, -0.75, 0], [0, 0, 0.75], [0.7499999, 0.7, -0.7]], dtype=F)
    seg = np.asarray([1, 2, 3, 4, 5, 6], dtype=np.int32)
    groups, counts, keep, _ = groups_host(box, seg, [1, 2, 3, 4, 5, 6], [0], 0.75, 3)
    assert groups == [[1, 3, 6]] and counts == [3] and keep == [True]             # a vertex on a face is outside, on every axis
    assert groups_host(box, seg, [1, 2, 3, 4, 5, 6], [0], 0.75, 4)[2] == [False]  # ... and one segment short: the group is dropped


def test_ids_zero_sparse_ids_and_a_mask_word_crossed():
    ids = [0, 7, 4999, 5000] + list(range(100, 3400, 100))                       # 37 ids, not contiguous, up to 5000, 0 included
    assert len(ids) == 37
    pts, seg = cloud(900, 5, ids=ids)
    seeds = P.split_seeds_host(pts, 1.0, 5)
    groups, counts, keep, mask = groups_host(pts, seg, np.unique(seg), seeds, 1.4, 5)
    assert (groups, counts, keep) == brute_groups(pts, seg, np.unique(seg), seeds, 1.4, 5)
    assert mask.shape[1] == 2 and (mask[:, 1] != 0).any() and any(0 in g for g in groups) and any(5000 in g for g in groups)
    only = groups_host(pts, seg, [5000, 7], seeds, 1.4, 1)                        # unlisted ids are ignored; slots follow the caller's order
    assert only[0] == [[i for i in g if i in (7, 5000)] for g in groups]
    with pytest.raises(L.VlsatError):
        P.split_groups_host(pts, seg, [7, 7], seeds)


def test_one_vertex_one_seed_duplicates_and_non_finite():
    one = np.asarray([[3, 4, 5]], dtype=F)
    assert P.split_seeds_host(one, 1.0, 9).tolist() == [0] == brute_seeds(one, 1.0, 9)
    assert groups_host(one, [4], [4], [0], 0.75, 1)[:3] == ([[4]], [1], [True])
    near, seg = cloud(200, 2, extent=(0.6, 0.5, 0.4))                             # all within the distance: K = 1
    assert len(P.split_seeds_host(near, 1.0, 2)) == 1
    dup = np.repeat(cloud(50, 3)[0], 3, axis=0)                                   # every vertex three times: a seed's copies are never selectable
    seeds = P.split_seeds_host(dup, 1.0, 4)
    assert seeds.tolist() == brute_seeds(dup, 1.0, 4) and len({tuple(dup[s]) for s in seeds}) == len(seeds)
    bad, seg = cloud(300, 6)
    bad[10, 0], bad[20, 2], bad[30, 1] = np.nan, np.inf, -np.inf
    for seed in range(4):
        seeds = P.split_seeds_host(bad, 1.0, seed)
        assert seeds.tolist() == brute_seeds(bad, 1.0, seed) and not {10, 20, 30} & set(seeds[1:].tolist())
    assert P.split_seeds_host(bad, 1.0, ranks=[10]).tolist() == [10] == brute_seeds(bad, 1.0, ranks=[10])   # NaN seed: nothing is selectable
    got = groups_host(bad, seg, np.unique(seg), [10, 20, 0])
    assert got[:3] == brute_groups(bad, seg, np.unique(seg), [10, 20, 0]) and got[0][0] == [] and got[0][1] == []


def test_ranks_errors():
    pts, _ = cloud(300, 1)
    full = P.split_seeds_host(pts, 1.0, 1)
    ranks = [int(full[0])] + [0] * 40
    with pytest.raises(L.VlsatError, match="ran out"):
        P.split_seeds_host(pts, 1.0, ranks=ranks[:2])
    with pytest.raises(L.VlsatError, match="rank"):
        P.split_seeds_host(pts, 1.0, ranks=[300])
    with pytest.raises(L.VlsatError, match="rank"):
        P.split_seeds_host(pts, 1.0, ranks=[0, 300])
    with pytest.raises(L.VlsatError):
        P.split_seeds_host(pts, 0.0)
    assert P.split_seeds_host(pts, 1.0, ranks=ranks).tolist() == brute_seeds(pts, 1.0, ranks=ranks)
    assert 1 <= len(full) <= P.split_seed_cap(pts, 1.0) <= 300 and P.split_seed_cap(pts[:1], 1.0) == 1


def test_split_scan_feeds_prepare_scan_shapes():
    pts, seg = cloud(1200, 8)
    sp = S.split_scan({"points": pts.astype(np.float64), "instances": seg.astype(np.int64)}, seed=3, device="cpu")
    groups, seeds, seed_points = sp
    assert groups == sp.groups and len(groups) >= 2 and all(len(g) >= 5 for g in groups) and seed_points.shape == (len(seeds), 3)
    assert seeds.tolist() == brute_seeds(pts, 1.0, 3)
    want = brute_groups(pts, seg, np.unique(seg), seeds)
    assert groups == [g for g, k in zip(want[0], want[2]) if k] and sp.counts.tolist() == want[1]


# ---- fusion -------------------------------------------------------------------------------------------------------------------------------
def host(c, trim=True, **kw):
    return M.fuse_splits_host(c["obj_probs"], c["rel_probs"], c["edges"], c["row_instance"], c["weights"], obj_probs=c["obj_probs"],
                              rel_probs=c["rel_probs"], trim=trim, **kw)


FUSE = {
    "id_in_three_splits": lambda: fuse_case([5, 9, 2, 9, 7, 5, 9, 40], [(0, 1), (1, 0), (3, 4), (5, 6), (6, 7), (2, 0)], weights="mixed"),
    "edge_in_two_splits": lambda: fuse_case([3, 8, 8, 3, 1], [(0, 1), (3, 2), (1, 0), (4, 3), (0, 1)]),
    "weights": lambda: fuse_case([4, 4, 4, 2, 2], [(0, 3), (4, 1)], c=7, weights=[1, 250000, 3, 0.5, 12]),
    "dropped_edges": lambda: fuse_case([6, 6, 1, 0], [(0, 0), (0, 1), (1, 0), (2, 9), (-1, 2), (4, 0), (3, 2), (2, 3)]),
    "no_rows": lambda: fuse_case([], []),
    "no_edges": lambda: fuse_case([3, 1, 3], []),
    "random_150_rows": lambda: random_splits(6, 60, 25, 1000, 21, weights="mixed", c=20, r=7),
}


@pytest.mark.parametrize("name", list(FUSE))
def test_fusion_host_equals_the_loops(name):
    c = FUSE[name]()
    assert_fused(host(c), brute_fuse(c), name)


def test_what_the_fusion_cases_assert():
    g = host(FUSE["id_in_three_splits"]())
    assert g.obj_ids.tolist() == [2, 5, 7, 9, 40] and g.root.tolist() == [0, 1, 2, 1, 4, 0, 1, 7]
    assert g.members[g.member_ptr[3]:g.member_ptr[4]].tolist() == [1, 3, 6] and g.n_objects.tolist() == [5]
    c = FUSE["edge_in_two_splits"]()
    g = host(c)
    rp = c["rel_probs"]
    assert g.pair_edges.tolist() == [[0, 1], [1, 2], [2, 1]] and g.pair_count.tolist() == [1, 3, 1]    # ids 1, 3, 8 -> slots 0, 1, 2
    assert torch.equal(g.pair_probs[1], torch.maximum(torch.maximum(rp[0], rp[1]), rp[4])) and not torch.equal(rp[0], rp[1])
    assert g.edge_to_pair.tolist() == [1, 1, 2, 0, 1]
    c = FUSE["weights"]()
    g = host(c)
    w, p = c["weights"].numpy(), c["obj_probs"].numpy()
    s = F(F(F(w[0] * p[0, 0]) + F(w[1] * p[1, 0])) + F(w[2] * p[2, 0]))
    assert g.obj_probs[1, 0].item() == float(F(s / F(F(w[0] + w[1]) + w[2]))) and g.obj_weight.tolist() == [12.5, 250004.0]
    g = host(FUSE["dropped_edges"]())
    assert g.edge_to_pair.tolist() == [-1, -1, -1, -1, -1, -1, 0, 1] and g.pair_edges.tolist() == [[0, 1], [1, 0]]
    g = host(FUSE["no_rows"]())
    assert g.totals.tolist() == [0, 0] and g.member_ptr.tolist() == [0]


def test_ids_outside_the_table_belong_to_no_object():
    c = fuse_case([3, 70000, 3, 5], [(0, 1), (1, 3), (0, 3)])
    ids = torch.tensor(c["row_instance"], dtype=torch.int32)
    small = M.fuse_splits_host(c["obj_probs"], c["rel_probs"], c["edges"], ids, obj_probs=c["obj_probs"], rel_probs=c["rel_probs"])
    assert small.obj_ids.tolist() == [3, 5, 70000]                                # host ids size the table
    assert_fused(small, brute_fuse(c))
    c = fuse_case([3, 70000, 3, 5, 64], [(0, 1), (1, 3), (0, 3), (4, 0)])
    for ids in (c["row_instance"], torch.tensor(c["row_instance"], dtype=torch.int32)):             # an explicit table holds for host ids too
        cut = M.fuse_splits_host(c["obj_probs"], c["rel_probs"], c["edges"], ids, obj_probs=c["obj_probs"], rel_probs=c["rel_probs"], map_size=64)
        assert_fused(cut, brute_fuse(c, map_size=64))
        assert cut.object.tolist() == [0, -1, 0, 1, -1] and cut.root.tolist() == [0, -1, 0, 3, -1] and cut.edge_to_pair.tolist() == [-1, -1, 0, -1]
    with pytest.raises(L.VlsatError):
        host(fuse_case([1, -2], []))


def test_untrimmed_tables_and_the_merged_route():
    c = FUSE["random_150_rows"]()
    full, cut = host(c, trim=False), host(c)
    m, e = cut.totals.tolist()
    n, ne = c["obj_probs"].shape[0], c["edges"].shape[0]
    assert isinstance(cut, M.FusedGraph) and isinstance(cut, M.MergedGraph) and cut.trimmed and not full.trimmed
    assert full.obj_probs.shape[0] == n and full.pair_probs.shape[0] == ne and full.member_ptr.shape[0] == n + 1 and full.obj_ids.shape[0] == n
    assert_fused(full.trim(), cut)
    assert not full.obj_probs[m:].any() and not full.pair_probs[e:].any() and not full.pair_count[e:].any()
    assert (full.pair_edges[e:] == -1).all() and (full.obj_ids[m:] == -1).all() and (full.member_ptr[m:] == n).all()
    assert 50 <= m <= 60 and int(cut.pair_count.max()) >= 2 and (np.diff(cut.pair_edges[:, 0].numpy() * n + cut.pair_edges[:, 1].numpy()) > 0).all()
    # decode_graph, to_annotation, add_segments on the fused graph, as on a merged one
    node_ids = cut.node_ids()
    assert node_ids == SG.merged_node_ids(cut, c["row_instance"]) == sorted(set(c["row_instance"]))
    d = cut.decode(threshold=0.5, n_labels=2, max_rel=4000)
    names = ["none"] + [f"r{k}" for k in range(7)]
    ann = SG.to_annotation(d, 0, cut.pair_edges, node_ids, [f"c{k}" for k in range(20)], names, "scan-x")
    assert set(ann["objects"]) == {str(i) for i in node_ids} and len(ann["relationships"]) == int(d.n_valid[0]) > 0
    entry = SG.add_segments(ann, cut, c["row_instance"])
    assert all(set(v) == {int(k)} for k, v in entry["segments"].items())
    rel, objs, scans = S.read_relationships({"scans": [ann]}, ["scan-x"])
    assert scans == ["scan-x_0"] and rel["scan-x_0"] == ann["relationships"] and objs["scan-x_0"] == {int(k): v for k, v in ann["objects"].items()}
    assert cut.scene(0) is cut


def test_bad_fusion_arguments_raise():
    c = FUSE["weights"]()
    args = lambda **kw: {**dict(obj_logits=c["obj_probs"], rel=c["rel_probs"], edges=c["edges"], row_instance=c["row_instance"]), **kw}
    for bad in (dict(row_instance=[1, 2]), dict(edges=c["edges"][:1]), dict(weights=torch.ones(3)), dict(rel=torch.zeros(2, 33)),
                dict(row_instance=[1 << 24] * 5)):
        with pytest.raises(L.VlsatError):
            M.fuse_splits(**args(**bad))


# ---- the build list -----------------------------------------------------------------------------------------------------------------------
def test_the_source_is_built_with_fp_contract_off():
    from vlsat_amd import build as B
    assert "scene_split.hip" in B.SOURCES and B.PER_SOURCE_FLAGS["scene_split.hip"] == ["-ffp-contract=off"]
