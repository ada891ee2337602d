"""The convexity clusters without a GPU (include/vlsat_convex.h): csrc/convex_core.h on the host against the numpy predicate, bit for bit,
plain and under ASan + UBSan; the restatement against an independent brute force (Python loops, a breadth-first search) on tables made
by hand, one and two points, the two plates seen from either side, the absorption rounds and a dissolved component; the stacked boxes
with the conditions the feature exists for and the restatement's own counts; scan.segment_objects on the host route;
synth.make_stacked_boxes; the arguments that are refused; the build list and the scratch size (header and table: test_c_abi_cpu.py)."""
import numpy as np
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import build as B, lib as L, prep, scan, synth

import convex_checks as CC
import convex_core_host
import objects_checks as OC
from cloud_checks import assert_bit_equal


def _f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


# ---- csrc/convex_core.h on the host -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_convex_core_header_equals_the_restatement(sanitize):
    """the stand-alone program (its own main, g++ -ffp-contract=off; with -fsanitize=address,undefined in the second case) runs its
    in-place checks and prints 3800 rows: random triples, d = 0, zero / NaN / inf normals, tau = 0 and 1, values near the largest float;
    c, c seen from the other end and the four predicates equal the numpy restatement bit for bit"""
    rows = convex_core_host.run(sanitize)
    assert len(rows) == 3800
    x = _f32([r[0] for r in rows]).reshape(-1, 14)
    xi, ni, xj, nj, tau, q = x[:, 0:3], x[:, 3:6], x[:, 6:9], x[:, 9:12], x[:, 12], x[:, 13]
    c_cpp, back_cpp = _f32([r[1] for r in rows]), _f32([r[2] for r in rows])
    concave = np.zeros(len(rows), dtype=bool)
    c = np.zeros(len(rows), dtype=np.float32)
    for t in np.unique(tau.view(np.uint32)):           # convex_evidence_host takes one tau
        sel = tau.view(np.uint32) == t
        c[sel], concave[sel] = prep.convex_evidence_host(xi[sel], ni[sel], xj[sel], nj[sel], q[sel], tau[sel][0])
    back = prep.convex_evidence_host(xj, nj, xi, ni, q, 0.0)[0]
    real = ~np.isnan(c)
    assert (np.isnan(c_cpp) == ~real).all() and (np.isnan(back_cpp) == ~real).all() and (np.isnan(back) == ~real).all()
    assert 3000 < real.sum() < 3800                    # (a NaN has no stated payload)
    assert_bit_equal(c[real], c_cpp[real], "c")
    assert ((back == 0) == (c == 0)).all() and ((back_cpp == 0) == (c == 0)).all() and (c == 0).sum() >= 5
    real &= c != 0                                     # (x + -x is +0 from both ends: a zero c may change its sign, and nothing sees it)
    assert_bit_equal(back[real], c[real], "c seen from j, numpy")
    assert_bit_equal(back_cpp[real], c[real], "c seen from j, header")
    assert concave.tolist() == [bool(r[6]) for r in rows] and 400 < concave.sum() < 3000
    usable = lambda n: np.isfinite(n).all(1) & (n != 0).any(1)      # noqa: E731
    assert usable(ni).tolist() == [bool(r[3]) for r in rows] and usable(nj).tolist() == [bool(r[4]) for r in rows]
    with np.errstate(invalid="ignore"):
        assert (np.isfinite(q) & (q >= 0)).tolist() == [bool(r[5]) for r in rows]
    assert not usable(ni).all() and not (np.isfinite(q) & (q >= 0)).all()
    for i in list(range(0, 3000, 97)) + list(range(3000, 3800, 13)):                          # and the scalar statement agrees
        s = CC.scalar_c(xi[i], ni[i], xj[i], nj[i])
        assert (np.isnan(s) and not real[i]) or s.view(np.uint32) == c[i].view(np.uint32)
        assert CC.scalar_concave(s, tau[i], q[i]) == bool(concave[i])


# ---- the restatement against the brute force --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CC.HAND_CASES + ("v1_k1", "v1_k16", "v2_k1", "v2_k32", "v64_k16", "v65_k32") + CC.PLATE_CASES)
def test_restatement_equals_the_brute_force(name):
    CC.assert_same(CC.host(name), CC.brute_convex(**CC.case(name)), name)


def test_hand_made_table_step_by_step():
    """the floor line and the wall line of convex_checks.hand(): c = 2 between points 0 and 4 (q = 2, tau = 0.5: 4 > 0.5) and nowhere
    else, so 0 and 4 are boundary; the floor's cores 1, 2, 3, 9 and the wall's 5, 6 are the two components; 7 has no normal, 8 no place"""
    r0, r1, r2, r8, r64 = (CC.host(f"hand_r{r}") for r in (0, 1, 2, 8, 64))
    assert r0.state.tolist() == [2, 1, 1, 1, 2, 1, 1, 3, 0, 1] and r0.n_clusters.tolist() == [2]
    assert r0.labels.tolist() == [0, 1, 1, 1, 0, 2, 2, 0, 0, 1] and r0.cluster_size.tolist() == [4, 2] + [0] * 8
    # round 1: 0 passes its first entry (4, unlabelled) and takes the floor from 1; 4 passes 0 and takes the wall from 5; every entry of 7
    # is unlabelled at the end of round 0 -- it waits, although 0 and 4 get their labels in this very round
    assert r1.labels.tolist() == [1, 1, 1, 1, 2, 2, 2, 0, 0, 1] and r1.cluster_size.tolist() == [5, 3] + [0] * 8
    assert r2.labels.tolist() == [1, 1, 1, 1, 2, 2, 2, 1, 0, 1] and r2.cluster_size.tolist() == [6, 3] + [0] * 8       # 7 takes its FIRST entry's
    for later in (r8, r64):
        CC.assert_same(later, r2, "nothing is left to absorb")
    assert all((r.state == r0.state).all() for r in (r1, r2))                                 # an absorbed point keeps its state
    # min_points 3: the wall's two cores are dissolved (state 4) and the floor takes them through the junction, one ring per round
    m3 = CC.host("hand_min3")
    assert m3.state.tolist() == [2, 1, 1, 1, 2, 4, 4, 3, 0, 1] and m3.n_clusters.tolist() == [1]
    assert m3.labels.tolist() == [1] * 8 + [0, 1] and m3.cluster_size[0] == 9
    masks = CC.host("hand_masks")                                                             # 7 and -1 are non-zero; point 1 is out
    assert masks.state.tolist() == [2, 0, 1, 1, 2, 1, 1, 3, 0, 1]
    # 0 sees the wall's 4 (labelled in round 1) before anybody of the floor, whose nearest point is out: round 2, and 7 follows 4 then too
    assert masks.labels.tolist() == [2, 0, 1, 1, 2, 2, 2, 2, 0, 1] and masks.cluster_size[:2].tolist() == [3, 5]
    assert CC.host("hand_tau1").state.tolist() == r0.state.tolist()                           # 2^2 > 1 x 2 still
    assert CC.host("hand_tau0").state.tolist() == r0.state.tolist()                           # one plane: c = 0 is not > 0


@pytest.mark.parametrize("name", ["hand_r1", "plates_concave", "stacked_r1"])
def test_round_one_reaches_exactly_the_points_with_a_labelled_entry(name):
    a = CC.case(name)
    before = prep.convex_clusters_host(**{**a, "absorb_rounds": 0})
    after = prep.convex_clusters_host(**{**a, "absorb_rounds": 1})
    index = a["knn_index"].astype(np.int64)
    v = len(index)
    valid = (index >= 0) & (index < v) & (index != np.arange(v)[:, None])
    sees = (valid & (before.labels[np.where(valid, index, 0)] > 0)).any(1)
    assert ((after.labels > 0) == ((before.labels > 0) | ((before.state > 0) & sees))).all()
    assert (after.labels[before.labels > 0] == before.labels[before.labels > 0]).all() and 0 < ((after.labels > 0) & (before.labels == 0)).sum()


def test_plates_convex_from_outside_concave_from_inside():
    """two perpendicular plates: with the normals turned to a viewpoint behind both the crease is the convex edge of a box and the
    plates are ONE cluster; turned to a viewpoint between them it is the junction of a floor and a wall: TWO clusters and a band of
    boundary points along the crease"""
    from vlsat_amd import synth as S
    plate = S.make_plates(0.05, 0.002, 1)["plate"]
    one, two = CC.host("plates_convex"), CC.host("plates_concave")
    assert one.n_clusters.tolist() == [1] and (one.labels == 1).all() and one.cluster_size[0] == 861
    assert two.n_clusters.tolist() == [2] and (two.labels > 0).all()
    band = two.state == 2
    p = CC.plates()[0]
    assert 60 <= band.sum() <= 300 and (np.minimum(np.abs(p[band, 0]), np.abs(p[band, 2])) < 0.16).all()
    for k in (0, 1):                                                                          # each plate in a cluster of its own
        members = two.labels[plate == k]
        assert (members == np.bincount(members).argmax()).mean() > 0.9
    assert np.bincount(two.labels[plate == 0]).argmax() != np.bincount(two.labels[plate == 1]).argmax()


# ---- the stacked boxes ------------------------------------------------------------------------------------------------------------------
def _quality(labels, instances):
    own = [np.bincount(labels[instances == b], minlength=1).max() / (instances == b).sum() for b in np.unique(instances)]
    foreign = [1.0 - np.bincount(instances[labels == c]).max() / (labels == c).sum() for c in np.unique(labels[labels > 0])]
    return min(own), max(foreign)


def test_stacked_boxes_are_separated():
    """the prototype's setting on make_stacked_boxes(): K = 16 within 0.06, normals estimated and turned to the viewpoint, links up to
    0.03, tau = sin 10 deg = 0.17, min_points 20, 8 rounds.  The conditions, then the restatement's own counts: five bodies and the pocket
    of table top that three boxes enclose"""
    p, scene, table, est, exact = CC.stacked()
    out = CC.host("stacked")
    inst = scene["instances"]
    assert len(p) == 7211 and np.bincount(inst).tolist() == [0, 4271, 736, 1076, 401, 727]
    own, foreign = _quality(out.labels, inst)
    print("stacked boxes: the worst body keeps", own, "of its points in one cluster; the worst cluster holds", foreign, "foreign points")
    assert own >= 0.9
    assert foreign <= 0.05
    assert (out.labels > 0).all()
    near = prep.cloud_clusters_host(table.index, table.sqdist, np.ones(len(p), np.int32), CC._sq(0.03), 20)
    assert near.n_clusters.tolist() == [1]                                                   # proximity alone: one blob
    assert out.n_clusters.tolist() == [6] and out.cluster_size[:7].tolist() == [4156, 114, 740, 1076, 400, 725, 0]
    assert np.bincount(out.state, minlength=5).tolist() == [0, 6293, 914, 0, 4]
    assert own > 0.97 and foreign < 0.012
    pocket = p[out.labels == 2]                                                               # on the table top, between the boxes
    assert (np.abs(pocket[:, 2] - 0.5) < 0.01).all() and (inst[out.labels == 2] == 1).all()
    ex = CC.host("stacked_exact")                                                             # exact normals: the pocket stays with the table
    assert ex.n_clusters.tolist() == [5] and ex.cluster_size[:5].tolist() == [4274, 726, 1076, 399, 736] and (ex.labels > 0).all()
    own, foreign = _quality(ex.labels, inst)
    assert own >= 0.9 and foreign <= 0.05


@pytest.mark.parametrize("name", ["stacked_min1", "stacked_r0", "stacked_r64", "stacked_masked", "stacked_nonfinite"])
def test_stacked_variants_hold_together(name):
    """what the GPU test compares against, checked for sense: sizes add up to the labelled points, states and labels agree"""
    a, out = CC.case(name), CC.host(name)
    s = int(out.n_clusters[0])
    assert s >= 5 and out.cluster_size[:s].tolist() == np.bincount(out.labels, minlength=s + 1)[1:].tolist() and not out.cluster_size[s:].any()
    eligible = (a["mask"] != 0) & np.isfinite(a["points"]).all(1)
    assert ((out.state == 0) == ~eligible).all() and not out.labels[~eligible].any() and (out.labels[out.state == 1] > 0).all()
    if name == "stacked_r0":
        assert ((out.labels > 0) == (out.state == 1)).all()
    if name == "stacked_masked":
        assert (~eligible).sum() == 727
    if name == "stacked_nonfinite":
        assert (out.state == 3).sum() > 400 and (~eligible).sum() == 1031


def test_make_stacked_boxes():
    a = synth.make_stacked_boxes()
    assert a["points"].shape == a["normals"].shape == (7211, 3) and a["instances"].shape == (7211,) and a["viewpoint"] == (3.0, -2.5, 2.5)
    assert set(map(tuple, a["normals"].tolist())) == {(1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0)}      # the faces the viewpoint sees
    clean = synth.make_stacked_boxes(jitter=0.0)
    assert np.array_equal(clean["instances"], a["instances"]) and np.abs(a["points"] - clean["points"]).max() < 0.005
    top = clean["points"][(clean["instances"] == 5) & (clean["normals"][:, 2] == 1)]           # 22.5 steps high: the sides end at 0.94
    assert np.allclose(top[:, 2], 0.95) and np.isclose(clean["points"][(clean["instances"] == 5) & (clean["normals"][:, 2] == 0)][:, 2].max(), 0.94)
    for b, (lo, hi) in enumerate(synth.STACKED_BOXES):                                        # on its own box, inside no other
        mine = clean["points"][clean["instances"] == 1 + b]
        assert (mine >= np.asarray(lo) - 1e-9).all() and (mine <= np.asarray(hi) + 1e-9).all()
        others = clean["points"][clean["instances"] != 1 + b]
        assert not ((others >= np.asarray(lo) - 1e-9) & (others <= np.asarray(hi) + 1e-9)).all(1).any()
    assert not (clean["points"][clean["instances"] == 1][:, 2] < -1e-9).any()
    big = synth.make_stacked_boxes(step=0.05, jitter=0.0, viewpoint=(7.5, -6.25, 6.25))      # another step scales the boxes
    assert np.array_equal(big["instances"], clean["instances"]) and np.allclose(big["points"], clean["points"] * 2.5)
    assert not np.array_equal(synth.make_stacked_boxes(seed=1)["points"], a["points"])
    behind = synth.make_stacked_boxes(jitter=0.0, viewpoint=(-3.0, 2.5, 2.5))
    assert set(map(tuple, behind["normals"].tolist())) == {(-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)}


# ---- scan.segment_objects ---------------------------------------------------------------------------------------------------------------
def test_segment_objects_without_concavity_is_what_it_was():
    walls = OC.walled()[0]
    kw = dict(dist=0.02, cluster_radius=0.15, n_hyp=256, max_planes=8, min_plane_share=0.012, outside_frac=0.01, min_points=20, device=None)
    old = scan.segment_objects({"points": walls}, **kw)
    new = scan.segment_objects({"points": walls}, concavity_deg=None, viewpoint=(1.5, 1.5, 1.0), normal_radius=0.3, absorb_rounds=3,
                               recompute_normals=True, **kw)
    assert set(old) == set(new) and "concave" not in new
    for key in old:
        assert np.array_equal(old[key], new[key]), key
    assert old["n_planes"] == 5


def test_segment_objects_with_concavity_on_the_host():
    """the stacked boxes on a floor: the floor is found and removed as a plane, and what stood on it comes apart"""
    points, view = CC.floor_scene()
    kw = dict(dist=0.01, cluster_radius=0.03, n_hyp=64, max_planes=2, min_plane_share=0.3, min_points=20, device=None)
    near = scan.segment_objects({"points": points}, **kw)
    assert near["n_planes"] == 1 and near["n_segments"] == 2                                  # proximity: one blob on the floor
    out = scan.segment_objects({"points": points}, concavity_deg=10, viewpoint=view, **kw)
    assert out["n_planes"] == 1 and out["n_segments"] - out["n_planes"] >= 5
    assert out["concave"].dtype == bool and out["concave"].shape == (len(points),) and 300 < out["concave"].sum() < 2000
    assert out["seg_size"].tolist() == np.bincount(out["instances"], minlength=out["n_segments"] + 1)[1:].tolist()
    inst = synth.make_stacked_boxes()["instances"]
    own, foreign = _quality(out["instances"][:len(inst)] * (out["instances"][:len(inst)] > 1), inst)
    assert own >= 0.85 and foreign <= 0.05                                                    # the floor takes the bodies' lowest rows
    carried = scan.segment_objects({"points": points, "normals": np.concatenate([synth.make_stacked_boxes()["normals"] * 3.0,
                                                                                 np.tile([0.0, 0.0, 1.0], (len(points) - len(inst), 1))])},
                                   concavity_deg=10, **kw)                                    # carried normals: no viewpoint needed
    assert carried["n_segments"] - carried["n_planes"] >= 5
    with pytest.raises(scan.ScanError, match="needs a side"):
        scan.segment_objects({"points": points}, concavity_deg=10, **kw)
    with pytest.raises(scan.ScanError, match="needs a side"):
        scan.segment_objects({"points": points, "normals": np.ones_like(points)}, concavity_deg=10, recompute_normals=True, **kw)
    with pytest.raises(scan.ScanError):
        scan.segment_objects({"points": points}, concavity_deg=100, viewpoint=view, **kw)
    with pytest.raises(scan.ScanError):
        scan.segment_objects({"points": points}, concavity_deg=10, viewpoint=view, absorb_rounds=65, **kw)
    vox = scan.segment_objects({"points": points}, concavity_deg=10, viewpoint=view, voxel=0.02, **kw)
    assert vox["concave"].shape == (len(points),) and vox["n_segments"] == vox["resampled"]["n_segments"]
    of = vox["resampled"]["voxel_of_point"]
    assert np.array_equal(vox["concave"], (of >= 0) & vox["resampled"]["concave"][np.maximum(of, 0)]) and vox["concave"].any()


# ---- arguments, the header and the build ------------------------------------------------------------------------------------------------
def test_refused_arguments_on_the_host():
    a = CC.case("hand_r8")
    good = prep.convex_clusters(**{k: (torch.from_numpy(np.array(x)) if isinstance(x, np.ndarray) else x) for k, x in a.items()})
    assert isinstance(good, prep.ConvexClusters) and all(isinstance(x, torch.Tensor) and not x.is_cuda for x in good)
    CC.assert_same([x.numpy() for x in good], CC.host("hand_r8"))
    for change in (dict(link_sq_dist=float("nan")), dict(concavity=-0.01), dict(concavity=1.01), dict(concavity=float("nan")), dict(min_points=0),
                   dict(absorb_rounds=-1), dict(absorb_rounds=65), dict(points=a["points"][:5]), dict(normals=a["normals"][:, :2]),
                   dict(knn_sqdist=a["knn_sqdist"][:, :2]), dict(mask=a["mask"][:3]), dict(knn_index=np.zeros((10, 33), np.int32)),
                   dict(knn_index=np.zeros((0, 4), np.int32))):
        with pytest.raises(L.VlsatError, match="convex_clusters:"):
            prep.convex_clusters_host(**{**a, **change})
    for fine in (dict(link_sq_dist=float("inf")), dict(link_sq_dist=-1.0), dict(concavity=0.0), dict(concavity=1.0), dict(absorb_rounds=64)):
        prep.convex_clusters_host(**{**a, **fine})


def test_convex_source_is_built_with_fp_contract_off_and_the_scratch_size_needs_no_device():
    lib = L.load()
    assert "convex.hip" in B.SOURCES and B.PER_SOURCE_FLAGS["convex.hip"] == ["-ffp-contract=off"]
    # the scratch size needs no device: 0 for what is out of range, the layout's bytes otherwise
    assert lib.vlsat_convex_clusters_scratch_bytes(0) == 0 and lib.vlsat_convex_clusters_scratch_bytes((1 << 24) + 1) == 0
    assert lib.vlsat_convex_clusters_scratch_bytes(-1) == 0
    assert 28000 <= lib.vlsat_convex_clusters_scratch_bytes(1000) <= 28000 + 4 * 5 + 9 * 256
    assert lib.vlsat_convex_clusters_scratch_bytes(1 << 24) >= 28 << 24
