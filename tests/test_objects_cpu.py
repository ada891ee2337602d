"""The object segmenter without a GPU (include/vlsat_objects.h): csrc/plane_core.h on the host against the numpy restatement, bit for
bit, plain and under ASan + UBSan; the restatement against an independent scalar brute force, against answers derived by hand on
dyadic coordinates, and end to end on the box rooms and the walled room; the cluster rule; scan.segment_objects on the host route; the
arguments that are refused; synth.make_walled_room; the build list and the scratch sizes (the header and its table: test_c_abi_cpu.py)."""
import numpy as np
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import build as B, lib as L, prep, scan, synth

import objects_checks as OC
import plane_core_host
from cloud_checks import assert_bit_equal


def _f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


# ---- csrc/plane_core.h on the host ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_plane_core_header_equals_the_restatement(sanitize):
    """the stand-alone program (its own main, g++ -ffp-contract=off; with -fsanitize=address,undefined in the second case) runs its
    in-place checks and prints rows; every row equals the numpy restatement bit for bit"""
    rows = plane_core_host.run(sanitize)
    assert len(rows["d"]) == 200 and len(rows["p"]) == 400 and len(rows["s"]) > 2000 and len(rows["e"]) == 300 and len(rows["k"]) == 300
    for seed, k, n, rank in rows["d"]:
        assert prep.split_draw(seed, k, n) == rank == OC.draw(seed, k, n)
        assert int(prep.plane_draws(seed, np.array([k], dtype=np.uint64), n)[0]) == rank
    pts = _f32([r[0] for r in rows["p"]]).reshape(-1, 3, 3)
    planes, ok = prep.plane_from_points_host(pts[:, 0], pts[:, 1], pts[:, 2])
    assert ok.tolist() == [bool(r[1]) for r in rows["p"]] and 300 < ok.sum() < 400          # the void triples are among them
    assert_bit_equal(planes, _f32([r[2] for r in rows["p"]]).reshape(-1, 4), "planes")
    for i in np.nonzero(ok)[0][:60]:                                                         # and the scalar statement agrees
        assert_bit_equal(np.array(OC.scalar_plane(*pts[i])), planes[i], ("scalar plane", i))
    s_in = _f32([r[0] for r in rows["s"]]).reshape(-1, 8)
    with np.errstate(all="ignore"):
        s = np.array([prep.plane_scores_host(row[None, :4], row[None, 4:7])[0, 0] for row in s_in], dtype=np.float32)
        klass = np.where(np.abs(s) <= s_in[:, 7], 0, np.where(s > s_in[:, 7], 1, 2))
    assert_bit_equal(s, _f32([r[1] for r in rows["s"]]), "scores")
    assert klass.tolist() == [r[2] for r in rows["s"]] and set(klass.tolist()) == {0, 1, 2}
    for (inliers, above, n, min_inliers, ppm), eligible in rows["e"]:
        assert bool(eligible) == (inliers >= min_inliers and min(above, n - inliers - above) <= (n * ppm) // 1000000)
    assert {e for _, e in rows["e"]} == {0, 1}
    for inliers, h, key in rows["k"]:
        assert key == (inliers << 32) | (0xFFFFFFFF - h)


# ---- the restatement against an independent scalar statement ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", OC.SMALL_CASES)
def test_restatement_equals_the_scalar_brute_force(name):
    p, kw = OC.case(name)
    OC.assert_same_planes(OC.host_planes(name), OC.brute_planes(p, **kw), name)


def test_restatement_equals_the_scalar_brute_force_on_a_thinned_room():
    p = OC.boxes()[0][::40]                                                                  # 282 points: a floor and a few box points
    kw = dict(n_hyp=12, max_planes=2, dist=0.02, min_inliers=20, outside_ppm=10000, seed=6)
    got = prep.cloud_planes_host(p, **kw)
    assert int(got.n_planes[0]) == 1 and got.counts[0, 0] > 200
    OC.assert_same_planes(got, OC.brute_planes(p, **kw))


# ---- answers derived by hand ------------------------------------------------------------------------------------------------------------
def _layers():
    """a z = 0 grid of 20 x 20 points at spacing 0.25, a z = 1 plate of 10 x 10 above its middle, 30 points on a line at z = 2: dyadic
    coordinates, so fp32 and every product with a normal (0, 0, 1) are exact"""
    i, j = (x.ravel() for x in np.meshgrid(np.arange(20), np.arange(20), indexing="ij"))
    floor = np.stack([i * 0.25, j * 0.25, np.zeros(400)], 1)
    i, j = (x.ravel() for x in np.meshgrid(np.arange(10), np.arange(10), indexing="ij"))
    plate = np.stack([1.0 + i * 0.25, 1.0 + j * 0.25, np.ones(100)], 1)
    top = np.stack([np.arange(30) * 0.125, np.full(30, 2.0), np.full(30, 2.0)], 1)
    return np.concatenate([floor, plate, top]).astype(np.float32)


def test_hand_derived_floor_plate_and_top():
    """530 points: 400 at z = 0, 100 at z = 1, 30 at z = 2; dist 0.125, min_inliers 50, 1024 hypotheses (one in 150 lies in the plate).
    Round 1, n = 530.  The plane through three floor points is (0, 0, 1, 0): s = z exactly, so inliers = 400, above = 130, below = 0 and
    min(above, below) = 0 <= (530 * 10000) / 10^6 = 5: eligible.  The plane through three plate points is (0, 0, 1, -1): inliers = 100 >=
    50, above = 30, below = 400, min = 30 > 5: NOT eligible although it has enough inliers -- a table top.  A plane through the z = 2
    line and anything else has at most 30 + 20 + 10 inliers only if it is vertical and then has points on both sides; no plane has more
    than 400 inliers.  So round 1 extracts (0, 0, 1, 0) with counts (400, 130, 0), and with max_planes = 1 exactly one plane comes out.
    With outside_ppm = 500000 the bound is 265: the plate is eligible in round 1 too, loses to the floor's 400 inliers, and is extracted in
    round 2 (n = 130: inliers 100, above 30, below 0).
    The rule as include/vlsat_objects.h states it has one more consequence, asserted last: once the floor is gone NOTHING lies below
    the plate, so with max_planes >= 2 it is extracted in round 2 under outside_ppm = 10000 as well (bound (130 * 10000) / 10^6 = 1,
    min(30, 0) = 0).  What keeps a table top out in a room is min_inliers (a share of the whole cloud) and whatever stands below it."""
    p = _layers()
    one = prep.cloud_planes_host(p, 1024, 1, 0.125, 50, 10000, seed=0)
    assert int(one.n_planes[0]) == 1 and one.planes[0].tolist() == [0.0, 0.0, 1.0, 0.0] and one.counts[0].tolist() == [400, 130, 0]
    assert (one.plane_id[:400] == 1).all() and (one.plane_id[400:] == 0).all()
    plate, ok = prep.plane_from_points_host(p[400:401], p[409:410], p[490:491])              # three corners of the plate
    assert ok[0] and plate[0].tolist() == [0.0, 0.0, 1.0, -1.0]
    s = prep.plane_scores_host(plate, p)[0]
    inliers, above = int((np.abs(s) <= 0.125).sum()), int((s > 0.125).sum())
    assert (inliers, above, 530 - inliers - above) == (100, 30, 400) and inliers >= 50
    assert min(above, 400) > (530 * 10000) // 1000000 and min(above, 400) <= (530 * 500000) // 1000000
    # the draws do try the plate in round 1: some hypothesis takes three distinct plate points that are not collinear
    tried = [[prep.split_draw(0, h * 3 + j, 530) for j in range(3)] for h in range(1024)]
    assert any(all(400 <= r < 500 for r in t) and prep.plane_from_points_host(*(p[r:r + 1] for r in t))[1][0] for t in tried)
    two = prep.cloud_planes_host(p, 1024, 2, 0.125, 50, 500000, seed=0)
    assert int(two.n_planes[0]) == 2 and two.planes.tolist() == [[0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 1.0, -1.0]]
    assert two.counts.tolist() == [[400, 130, 0], [100, 30, 0]] and (two.plane_id[400:500] == 2).all() and (two.plane_id[500:] == 0).all()
    later = prep.cloud_planes_host(p, 1024, 4, 0.125, 50, 10000, seed=0)
    assert int(later.n_planes[0]) == 2 and later.counts[:2].tolist() == [[400, 130, 0], [100, 30, 0]] and (later.planes[2:] == 0).all()


def test_points_at_exactly_dist_are_inliers_and_the_next_float_is_not():
    """a z = 0 grid of 100 points, then points at z = +dist, -dist (inliers: |s| <= dist with s = z exactly) and at the next float
    beyond either (above and below); dist = 0.1f is no dyadic number, the comparison is between equal or neighbouring floats"""
    dist = np.float32(0.1)
    up = np.nextafter(dist, np.float32(1))
    i, j = (x.ravel() for x in np.meshgrid(np.arange(10), np.arange(10), indexing="ij"))
    z = np.concatenate([np.zeros(100, np.float32), [dist, -dist, up, -up, dist, -up]])
    p = np.stack([np.concatenate([i, [1, 2, 3, 4, 5, 6]]) * 0.5, np.concatenate([j, [1, 2, 3, 4, 5, 6]]) * 0.5, z], 1).astype(np.float32)
    out = prep.cloud_planes_host(p, 64, 1, float(dist), 50, 100000, seed=1)
    assert out.planes[0].tolist() == [0.0, 0.0, 1.0, 0.0] and out.counts[0].tolist() == [103, 1, 2]
    assert out.plane_id[100:].tolist() == [1, 1, 0, 0, 1, 0] and (out.plane_id[:100] == 1).all()


def test_equal_inlier_counts_go_to_the_lower_hypothesis():
    """the four corners of a tetrahedron, min_inliers 3, outside_ppm 500000 (the bound is 2): every hypothesis of three distinct draws
    is a face with exactly 3 inliers and one point off it, so every key has the same inlier count and the LOWEST such h must win; which
    face that is follows from the draws, computed here in Python integers"""
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)
    for seed in range(6):
        tried = [[OC.draw(seed, h * 3 + j, 4) for j in range(3)] for h in range(16)]
        first = next(t for t in tried if len(set(t)) == 3)
        later = [t for t in tried if len(set(t)) == 3 and set(t) != set(first)]
        assert later                                                                         # another face was on offer
        out = prep.cloud_planes_host(p, 16, 1, 0.125, 3, 500000, seed=seed)
        assert int(out.n_planes[0]) == 1 and out.counts[0, 0] == 3
        assert sorted(np.nonzero(out.plane_id == 1)[0].tolist()) == sorted(first)
        assert_bit_equal(out.planes[0], np.array(OC.scalar_plane(*p[first])), seed)
    n3 = prep.cloud_planes_host(p[:3], 16, 2, 0.125, 3, 0, seed=0)                           # an alive list of n = 3: one plane, then n = 0
    assert int(n3.n_planes[0]) == 1 and n3.plane_id.tolist() == [1, 1, 1] and n3.counts.tolist() == [[3, 0, 0], [0, 0, 0]]


def test_coincident_points_give_no_plane_and_few_points_end_the_rounds():
    out = OC.host_planes("coincident")
    assert int(out.n_planes[0]) == 0 and not out.plane_id.any() and not out.planes.any() and not out.counts.any()
    # four coplanar points and one far off: round 1 takes the four, round 2 has n = 1 < 3 and stops
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0.5, 0.5, 9.0]], dtype=np.float32)
    out = prep.cloud_planes_host(p, 32, 4, 0.125, 3, 500000, seed=2)
    assert int(out.n_planes[0]) == 1 and out.plane_id.tolist() == [1, 1, 1, 1, 0] and out.counts[0].tolist() == [4, 1, 0]
    # invalid points are never alive: two finite points are fewer than three
    p = np.array([[0, 0, 0], [np.nan, 0, 0], [1, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]], dtype=np.float32)
    out = prep.cloud_planes_host(p, 32, 4, 0.125, 3, 500000)
    assert int(out.n_planes[0]) == 0 and not out.plane_id.any()


def test_cases_of_the_device_tests_stop_where_they_should():
    """what the GPU test compares against: the counts here are the restatement's own"""
    n = {name: int(OC.host_planes(name).n_planes[0]) for name in OC.PLANE_CASES}
    assert n["boxes_h65"] == n["boxes_h256"] == n["boxes_h300"] == n["boxes_one_plane"] == 1         # the floor, then an early stop
    assert n["plates"] == 2 and n["walled"] == 5 and n["boxes_tops"] == 6 and n["nonfinite"] == 1 and n["boxes_h1"] == 0
    assert n["v3"] == 1 and n["v64"] >= 1 and n["v65"] >= 1 and n["v257"] >= 1
    bad = ~np.isfinite(OC.case("nonfinite")[0]).all(1)
    assert bad.sum() > 100 and not OC.host_planes("nonfinite").plane_id[bad].any()
    plates = OC.host_planes("plates")
    assert sorted(plates.counts[:2, 0].tolist()) == [420, 441] and (plates.plane_id > 0).all()


# ---- clusters ---------------------------------------------------------------------------------------------------------------------------
def _clusters(index, sqdist, mask, max_sq_dist, min_points):
    got = prep.cloud_clusters_host(index, sqdist, mask, max_sq_dist, min_points)
    OC.assert_same_clusters(got, OC.brute_clusters(index, sqdist, mask, max_sq_dist, min_points))
    return got


def test_two_blobs_and_a_bridge():
    r2 = float(np.float32(0.6) ** 2)
    p, mask = OC.blobs(0)
    t = OC.knn(p, 8, 0.6)
    apart = _clusters(t.index, t.sqdist, mask, r2, 5)
    assert int(apart.n_clusters[0]) == 2 and apart.cluster_size[:3].tolist() == [30, 30, 0]
    assert apart.labels.tolist() == [1] * 30 + [2] * 30 + [0]                                # the bridge has mask 0: no label, no link
    joined = _clusters(t.index, t.sqdist, OC.blobs(1)[1], r2, 5)
    assert int(joined.n_clusters[0]) == 1 and joined.cluster_size[0] == 61 and (joined.labels == 1).all()
    near = _clusters(t.index, t.sqdist, OC.blobs(1)[1], float(np.float32(0.45) ** 2), 1)     # a smaller radius: the bridge is alone
    assert int(near.n_clusters[0]) == 3 and near.labels[-1] == 3 and near.cluster_size[:3].tolist() == [30, 30, 1]


def test_small_components_get_zero_and_numbering_follows_the_lowest_point():
    p = np.concatenate([OC.blobs(0)[0][:30], OC.blobs(0)[0][30:49]])                         # 30 and 19 points
    t = OC.knn(p, 8, 0.6)
    mask = np.ones(len(p), dtype=np.int32)
    r2 = float(np.float32(0.6) ** 2)
    assert _clusters(t.index, t.sqdist, mask, r2, 19).cluster_size[:2].tolist() == [30, 19]
    out = _clusters(t.index, t.sqdist, mask, r2, 20)                                         # min_points - 1 = 19 points: 0
    assert int(out.n_clusters[0]) == 1 and out.labels.tolist() == [1] * 30 + [0] * 19
    perm = np.random.default_rng(3).permutation(len(p))                                      # numbering: by the lowest point of each cluster
    tp = OC.knn(p[perm], 8, 0.6)
    shuffled = _clusters(tp.index, tp.sqdist, mask, r2, 1)
    first = {int(shuffled.labels[i]): i for i in range(len(p) - 1, -1, -1)}
    assert first[1] < first[2] and int(shuffled.n_clusters[0]) == 2
    assert sorted(shuffled.cluster_size[:2].tolist()) == [19, 30] and shuffled.cluster_size[shuffled.labels[0] - 1] == (30 if perm[0] < 30 else 19)


def test_pads_and_entries_out_of_range_are_ignored():
    index = np.array([[1, -1, 7], [0, 5, -3], [3, 2, 1 << 30], [2, -1, -1], [4, 4, 4]], dtype=np.int32)
    sqdist = np.array([[0.1, np.inf, 0.0], [0.1, 0.0, 0.0], [0.2, 0.0, 0.0], [np.nan, np.inf, np.inf], [0.0, 0.0, 0.0]], dtype=np.float32)
    out = _clusters(index, sqdist, np.ones(5, np.int32), 0.5, 1)
    # 0-1 by both rows; 2-3 by row 2 only (row 3 holds a NaN distance); 2 -> 2 and 4 -> 4 are no edges; 5, 7, -3 and 2^30 name no point
    assert out.labels.tolist() == [1, 1, 2, 2, 3] and out.cluster_size.tolist() == [2, 2, 1, 0, 0]
    none = _clusters(index, sqdist, np.zeros(5, np.int32), 0.5, 1)
    assert int(none.n_clusters[0]) == 0 and not none.labels.any() and not none.cluster_size.any()
    far = _clusters(index, sqdist, np.array([1, 1, 1, 1, 0], np.int32), 0.15, 2)             # 0.2 > 0.15: 2 and 3 stay alone, below 2 points
    assert far.labels.tolist() == [1, 1, 0, 0, 0] and int(far.n_clusters[0]) == 1


# ---- end to end on the restatement ------------------------------------------------------------------------------------------------------
def _padded_boxes_meet(room, a, b, pad):
    pa, pb = (room["points"][room["instances"] == x] for x in (a, b))
    return bool(((pa.min(0) - pad <= pb.max(0) + pad) & (pb.min(0) - pad <= pa.max(0) + pad)).all())


@pytest.mark.parametrize("which,radius,n_planes,n_clusters", [("big", 0.075, 1, 10), ("small", 0.15, 2, 3)])
def test_box_rooms_end_to_end(which, radius, n_planes, n_clusters):
    """the issue's rooms with the project's own draws and kNN edges: dist 0.02, H 256, share 0.02, outside_frac 0.01, min_points 20.
    The counts are the restatement's own.  59 429 points: one plane, the floor, of 43 668 inliers and 10 clusters of 12 boxes, as the
    issue's prototype found with numpy's draws and all pairs within the radius.  11 245 points: the floor of 10 456 inliers and 3
    clusters as there, but under these draws a SECOND plane: the three boxes are 0.6, 0.6 and 0.7 high, and a plane tilted by 0.03 through
    their tops holds 239 >= 225 of the 789 remaining points with one point above it -- structural by the rule, as a ceiling is.  Each
    box keeps its sides, which still hang together."""
    pts, room = OC.big_boxes() if which == "big" else (OC.boxes()[0].astype(np.float64), OC.boxes()[1])
    out = scan.segment_objects({"points": pts}, 0.02, radius, n_hyp=256, min_plane_share=0.02, outside_frac=0.01, min_points=20, device=None)
    inst, gen = out["instances"], room["instances"]
    assert out["n_planes"] == n_planes and out["planes"].shape == (n_planes, 4) and out["planes"][0, 2] > 0.9999
    floorish = np.abs(pts[:, 2].astype(np.float32)) <= np.float32(0.02)
    assert (inst[floorish] == 1).all() and (inst[gen == 1] == 1).all()                       # no floor point is left alive
    assert int((inst == 1).sum()) == int(out["seg_size"][0]) == {"big": 43668, "small": 10456}[which]
    assert out["n_segments"] == n_planes + n_clusters and not (inst == 0).any()              # no point is dropped
    if which == "small":
        assert out["seg_size"][1] == 239 and (room["plane"][inst == 2] % 6 == 0).sum() >= 149   # plane 2: the tops (face +z) and their rims
    members = {}
    for box in np.unique(gen[gen > 1]):
        labels = np.unique(inst[(gen == box) & (inst > n_planes)])
        assert len(labels) == 1, (box, labels)                                               # no box is split
        members.setdefault(int(labels[0]), []).append(int(box))
    assert len(members) == n_clusters
    for boxes in members.values():                                                           # a cluster spans two boxes only where they touch
        for a in boxes:
            assert len(boxes) == 1 or any(_padded_boxes_meet(room, a, b, radius / 2) for b in boxes if b != a), boxes
    assert np.array_equal(out["seg_size"], np.bincount(inst, minlength=out["n_segments"] + 1)[1:])


def test_walled_room_gives_five_planes_and_no_box_top():
    """floor and four walls come out, and the top of 100 points does not although min_inliers is 60: walls stand above it on every
    side.  Share 0.012 of 4995 points; the restatement alone decides"""
    pts, room = OC.walled()
    tops = [int((room["plane"] == 1 + 6 * b + 5).sum()) for b in range(3)]
    out = scan.segment_objects({"points": pts}, 0.02, 0.15, n_hyp=256, max_planes=8, min_plane_share=0.012, outside_frac=0.01, min_points=20,
                               device=None)
    assert max(tops) == 100 > 60 == int(np.ceil(0.012 * len(pts)))
    assert out["n_planes"] == 5
    normals = np.abs(np.round(out["planes"][:, :3])).tolist()
    assert sorted(normals) == sorted([[0, 0, 1], [1, 0, 0], [1, 0, 0], [0, 1, 0], [0, 1, 0]])
    inst = out["instances"]
    assert (inst[room["structural"]] >= 1).all() and (inst[room["structural"]] <= 5).all()   # every floor and wall point is on a plane
    for wall in range(room["n_obj"] + 2, room["n_obj"] + 6):
        assert len(np.unique(inst[room["instances"] == wall])) == 1
    for b in range(3):                                                                       # no top, and no other interior face, is a plane
        top = room["plane"] == 1 + 6 * b + 5
        assert (inst[top] > 5).all()
    assert out["n_segments"] > 5 and np.array_equal(out["seg_size"], np.bincount(inst, minlength=out["n_segments"] + 1)[1:])
    assert np.array_equal(OC.host_planes("walled").plane_id > 0, (inst >= 1) & (inst <= 5))  # the device test's case is this room


# ---- scan.segment_objects on the host route ---------------------------------------------------------------------------------------------
def test_segment_objects_voxel_gathers_back_to_every_input_point(tmp_path):
    p = OC.boxes()[0].astype(np.float64)
    twice = np.concatenate([p, p[:4000] + 0.003, [[np.nan, 0.0, 0.0]]])                      # the first 4000 points seen twice, one bad row
    out = scan.segment_objects({"points": twice}, 0.02, 0.15, n_hyp=128, min_plane_share=0.02, min_points=20, voxel=0.05, device=None)
    small = out["resampled"]
    assert len(out["instances"]) == len(twice) and len(small["points"]) < len(twice) and out["instances"][-1] == 0
    of = small["voxel_of_point"]
    assert (of[:-1] >= 0).all() and np.array_equal(out["instances"][:-1], small["instances"][of[:-1]])
    assert out["n_planes"] == small["n_planes"] >= 1 and out["n_segments"] == small["n_segments"] == out["n_planes"] + 3
    assert np.array_equal(out["seg_size"], np.bincount(out["instances"], minlength=out["n_segments"] + 1)[1:])
    assert out["seg_size"].sum() == len(twice) - 1
    path = str(tmp_path / "objects.ply")                                                     # and from a file, into a file
    scan.write_ply(path, {"points": p})
    again = scan.segment_objects(path, 0.02, 0.15, n_hyp=128, min_plane_share=0.02, min_points=20, device=None)
    assert again["n_segments"] == again["n_planes"] + 3 and (again["instances"] > 0).all()
    scan.write_ply(path, again)
    assert np.array_equal(scan.read_ply(path)["instances"], again["instances"])


def test_refused_arguments_on_the_host():
    p = np.zeros((5, 3), dtype=np.float32)
    good = dict(n_hyp=8, max_planes=2, dist=0.1, min_inliers=3, outside_ppm=1000)
    for change in (dict(n_hyp=0), dict(n_hyp=4097), dict(max_planes=0), dict(max_planes=33), dict(dist=0.0), dict(dist=-1.0),
                   dict(dist=float("nan")), dict(dist=float("inf")), dict(dist=1e39), dict(min_inliers=2), dict(outside_ppm=-1),
                   dict(outside_ppm=500001)):
        with pytest.raises(L.VlsatError):
            prep.cloud_planes_host(p, **{**good, **change})
    with pytest.raises(L.VlsatError):
        prep.cloud_planes_host(p[:2], **good)
    index, sqdist, mask = np.zeros((4, 2), np.int32), np.zeros((4, 2), np.float32), np.ones(4, np.int32)
    for args in ((index, sqdist, mask, float("nan"), 1), (index, sqdist, mask, 1.0, 0), (index, sqdist[:, :1], mask, 1.0, 1),
                 (index, sqdist, mask[:3], 1.0, 1), (np.zeros((4, 33), np.int32), np.zeros((4, 33), np.float32), mask, 1.0, 1)):
        with pytest.raises(L.VlsatError):
            prep.cloud_clusters_host(*args)
    for kw in (dict(cluster_radius=-1.0), dict(min_plane_share=0.0), dict(outside_frac=0.6), dict(dist=0.0)):
        with pytest.raises(scan.ScanError):
            scan.segment_objects({"points": np.zeros((5, 3))}, **{**dict(dist=0.1, cluster_radius=0.1, device=None), **kw})
    with pytest.raises(scan.ScanError):
        scan.segment_objects({"points": np.zeros((2, 3))}, 0.1, 0.1, device=None)
    cpu = prep.cloud_planes(torch.from_numpy(OC.case("v64")[0]), **OC.case("v64")[1])          # CPU tensors run the restatement
    OC.assert_same_planes([x.numpy() for x in cpu], OC.host_planes("v64"))


def test_make_walled_room():
    room = synth.make_walled_room(3, 0.1, 3, height=2.0, extent=(3.0, 3.0))
    base = synth.make_box_mesh(3, 0.1, 3, extent=(3.0, 3.0))
    n = len(base["points"])
    assert np.array_equal(room["points"][:n], base["points"]) and np.array_equal(room["instances"][:n], base["instances"])
    assert np.array_equal(room["plane"][:n], base["plane"]) and "faces" not in room
    walls = room["points"][n:]
    assert len(walls) == 2 * 31 * 20 + 2 * 29 * 20 and len(np.unique(walls, axis=0)) == len(walls)   # corner columns are sampled once
    assert np.isclose(walls[:, 2].min(), 0.1) and np.isclose(walls[:, 2].max(), 2.0)
    on = [np.isclose(walls[:, 0], 0.0), np.isclose(walls[:, 0], 3.0), np.isclose(walls[:, 1], 0.0), np.isclose(walls[:, 1], 3.0)]
    for w in range(4):
        sel = room["instances"][n:] == 5 + w
        assert sel.sum() == (31 if w < 2 else 29) * 20 and on[w][sel].all() and (room["plane"][n:][sel] == 19 + w).all()
    assert room["structural"].sum() == (base["instances"] == 1).sum() + len(walls) and room["height"] == 2.0


# ---- the build list and the scratch sizes -----------------------------------------------------------------------------------------------
def test_objects_source_is_built_with_fp_contract_off_and_scratch_sizes_need_no_device():
    lib = L.load()
    assert "objects.hip" in B.SOURCES and B.PER_SOURCE_FLAGS["objects.hip"] == ["-ffp-contract=off"]
    # the scratch sizes need no device: 0 for what is out of range, the layout's bytes otherwise
    assert lib.vlsat_cloud_planes_scratch_bytes(2, 8) == 0 and lib.vlsat_cloud_planes_scratch_bytes(3, 4097) == 0
    assert lib.vlsat_cloud_planes_scratch_bytes((1 << 24) + 1, 8) == 0 and lib.vlsat_cloud_clusters_scratch_bytes(0) == 0
    assert lib.vlsat_cloud_planes_scratch_bytes(1000, 300) >= 8 * 1000 + 28 * 300 and lib.vlsat_cloud_clusters_scratch_bytes(1000) >= 16000
