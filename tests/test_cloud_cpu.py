"""The point-cloud front end on the host (the rules are stated in include/vlsat_cloud.h): the numpy restatement of the neighbour search
against a brute force, csrc/cloud_core.h through g++ (with ASan + UBSan in the stand-alone program) against the restatements bit for
bit, the restated normals against np.linalg.eigh, the segmenter on the plate cases, scan.segment_cloud on the host, and what the
entry points refuse without a device (the header's symbols: test_c_abi_cpu.py)."""
import numpy as np
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import lib as L, prep, scan, synth

import cloud_core_host
from cloud_checks import assert_bit_equal, brute_knn, cloud, host_knn, small_room


# ---- neighbours ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["grid", "duplicates", "nonfinite", "density", "radius0", "single"])
def test_restated_neighbours_equal_the_brute_force(name):
    p, m = cloud(name)
    p = p[:140]
    for k in (1, 9, 32):
        got = prep.knn_points_host(p, k, m)
        index, sqdist, count = brute_knn(p, k, m)
        assert_bit_equal(got.index, index, (name, k, "index"))
        assert_bit_equal(got.sqdist, sqdist, (name, k, "sqdist"))
        assert_bit_equal(got.count, count, (name, k, "count"))


def test_neighbour_table_properties():
    p, m = cloud("density")
    t = host_knn("density", 16)
    assert int(t.count.min()) == 0 and int(t.count.max()) == 16 and 0 < ((t.count > 0) & (t.count < 16)).sum()
    slot = np.arange(16)[None, :]
    assert ((t.index >= 0) == (slot < t.count[:, None])).all() and (np.isinf(t.sqdist) == (t.index < 0)).all()
    assert (t.index != np.arange(len(p))[:, None]).all()
    d = np.where(t.index >= 0, t.sqdist, np.float32(0))
    assert (t.sqdist[:, 1:] >= t.sqdist[:, :-1]).all() and (d <= np.float32(m)).all()
    assert_bit_equal(host_knn("density", 8).index, t.index[:, :8])                 # the first 8 of 16 are the 8
    bad = ~np.isfinite(cloud("nonfinite")[0]).all(1)
    t = host_knn("nonfinite", 8)
    assert bad.sum() > 50 and (t.count[bad] == 0).all() and not np.isin(t.index, np.nonzero(bad)[0]).any()
    t = host_knn("radius0", 8)
    assert int(t.count.max()) == 2 and int(t.count.min()) == 0 and (t.sqdist[t.index >= 0] == 0).all()   # only the other copies of a point


def test_cpu_tensors_take_the_host_route():
    p, m = cloud("v257")
    t = prep.knn_points(torch.from_numpy(p.copy()), 9, m)
    want = host_knn("v257", 9)
    assert isinstance(t, prep.KnnTable) and all(torch.is_tensor(x) and not x.is_cuda for x in t)
    for got, w in zip(t, want):
        assert_bit_equal(got.numpy(), w)
    n, c = prep.cloud_normals(torch.from_numpy(p.copy()), t.index, t.count, 5)
    wn, wc = prep.cloud_normals_host(p, want.index, want.count, 5)
    assert_bit_equal(n.numpy(), wn)
    assert_bit_equal(c.numpy(), wc)


def test_refused_arguments():
    p = np.zeros((4, 3), np.float32)
    for bad in (lambda: prep.knn_points_host(p, 0, 1.0), lambda: prep.knn_points_host(p, 33, 1.0), lambda: prep.knn_points_host(p, 4, -1.0),
                lambda: prep.knn_points_host(p, 4, float("nan")), lambda: prep.knn_points_host(np.zeros((0, 3), np.float32), 4, 1.0),
                lambda: prep.cloud_normals_host(p, np.zeros((4, 2), np.int32), np.zeros(4, np.int32), 2),
                lambda: prep.cloud_normals_host(p, np.zeros((3, 2), np.int32), np.zeros(4, np.int32), 3),
                lambda: prep.cloud_normals_host(p, np.zeros((4, 2), np.int32), np.zeros(4, np.int32), 3, (0.0, float("nan"), 0.0))):
        with pytest.raises(L.VlsatError):
            bad()
    with pytest.raises(scan.ScanError):
        scan.segment_cloud({"points": p}, -1.0, device=None)
    with pytest.raises(TypeError):
        scan.segment_cloud({"points": p})                                          # no radius: none is free of units


# ---- cloud_core.h through g++ against the restatements ----------------------------------------------------------------------------------
def test_core_distances_keys_and_weights_equal_the_restatements():
    rows = cloud_core_host.run(sanitize=True)
    assert len(rows["d"]) > 1000 and len(rows["u"]) > 2000
    pts = np.array([r[0] for r in rows["d"]], dtype=np.uint32).view(np.float32).reshape(-1, 2, 3)
    with np.errstate(over="ignore", invalid="ignore"):
        dx, dy, dz = (pts[:, 0, c] - pts[:, 1, c] for c in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.view(np.uint32).tolist() == [r[2] for r in rows["d"]]
    assert [(int(b) << 32) | r[1] for b, r in zip(d2.view(np.uint32), rows["d"])] == [r[3] for r in rows["d"]]
    nrm = np.array([r[0] for r in rows["u"]], dtype=np.uint32).view(np.float32).reshape(-1, 3)
    idx = np.arange(len(rows["u"]))
    want = prep.segment_weights_host(nrm, 2 * idx, 2 * idx + 1, unsigned=True)
    assert want.view(np.uint32).tolist() == [r[1] for r in rows["u"]]
    assert {int(x) for x in want.view(np.uint32)} >= {0, 0x3f800000, 0x40000000}   # 0, 1 and 2 all occur
    assert rows == cloud_core_host.run(sanitize=False)


def test_core_normals_equal_the_restatement_bit_for_bit():
    """every neighbourhood of tests/cloud_core_check.cpp -- planar, collinear, isotropic, coincident, too few, 1e-6 and 1e+6 scale,
    random; every sign rule -- as a table of one point each: the restatement gives the fp64 bits cloud_core.h gives"""
    rows = cloud_core_host.run(sanitize=True)["n"]
    assert len(rows) > 900
    none = (0, 0, 0, np.float64(1.0).view(np.uint64))
    n_none = n_zero_dot = 0
    for use_vp, vp, min_points, members, want in rows:
        m = np.array(members, dtype=np.uint32).view(np.float32).reshape(-1, 3)
        count = len(m) - 1
        k = max(count, 1)
        index = np.full((len(m), k), -1, dtype=np.int32)
        index[0, :count] = np.arange(1, count + 1)
        cnt = np.zeros(len(m), dtype=np.int32)
        cnt[0] = count
        view = tuple(np.array(vp, dtype=np.uint64).view(np.float64)) if use_vp else None
        n, c = prep.cloud_normals_host(m, index, cnt, min_points, view, rounded=False)
        got = tuple(int(x) for x in n[0].view(np.uint64)) + (int(c[:1].view(np.uint64)[0]),)
        assert got == want, (use_vp, vp, min_points, m.tolist(), got, want)
        n_none += want == none
        n_zero_dot += bool(use_vp) and view == tuple(float(x) for x in m[0].astype(np.float64))
        n32, c32 = prep.cloud_normals_host(m, index, cnt, min_points, view)
        assert_bit_equal(n32[0], n[0].astype(np.float32))
        assert_bit_equal(c32[:1], c[:1].astype(np.float32))
        assert (n32[1:] == 0).all() and (c32[1:] == 1).all()                         # the other rows list nobody: no estimate
    assert n_none > 100 and n_zero_dot > 50 and n_none < len(rows) // 2


# ---- normals against another solver ---------------------------------------------------------------------------------------------------
def test_restated_normals_equal_eigh():
    """the box room (step 0.1, 3 boxes, 3 x 3 m), radius 0.15, K = 12: wherever the two smallest eigenvalues are apart by at least 0.05 of
    the largest, the Jacobi normal and LAPACK's eigenvector span the same line to |sin| <= 1e-12 (eps / gap with two orders of margin)"""
    p = small_room()["points"].astype(np.float32)
    t = prep.knn_points_host(p, 12, float(np.float32(0.15) ** 2))
    n, curv = prep.cloud_normals_host(p, t.index, t.count, 3, rounded=False)      # min_points 3: every point the filter lets through has a normal
    p64 = p.astype(np.float64)
    checked, worst, worst_curv = 0, 0.0, 0.0
    for i in range(len(p)):
        q = p64[np.concatenate([[i], t.index[i, :t.count[i]]])]
        d = q - q.mean(0)
        lam, vec = np.linalg.eigh(d.T @ d)
        if not lam[2] > 0 or (lam[1] - lam[0]) / lam[2] < 0.05:
            continue
        checked += 1
        worst = max(worst, float(np.linalg.norm(np.cross(vec[:, 0], n[i]))))
        worst_curv = max(worst_curv, abs(max(lam[0], 0.0) / lam.sum() - curv[i]))
    print(f"gap filter passed by {checked / len(p):.4f}, worst |sin| {worst:.2e}, worst curvature difference {worst_curv:.2e}")
    assert checked >= 0.9 * len(p)
    assert worst <= 1e-12 and worst_curv <= 1e-12
    assert np.abs(np.linalg.norm(n[(n != 0).any(1)], axis=1) - 1.0).max() < 1e-14  # V stays orthonormal: no renormalisation needed


def test_sign_rules():
    p = small_room()["points"].astype(np.float32)
    t = prep.knn_points_host(p, 12, float(np.float32(0.15) ** 2))
    free, _ = prep.cloud_normals_host(p, t.index, t.count, 5)
    have = (free != 0).any(1)
    big = np.take_along_axis(free, np.abs(free).argmax(1)[:, None], 1)[:, 0]
    assert have.sum() > 1900 and (big[have] > 0).all()                            # no viewpoint: the largest component is positive
    eye = (1.5, 1.5, 10.0)
    seen, _ = prep.cloud_normals_host(p, t.index, t.count, 5, eye)
    dot = (seen.astype(np.float64) * (np.array(eye) - p.astype(np.float64))).sum(1)
    assert (dot[have] >= -1e-6).all() and ((seen == free) | (seen == -free)).all() and (seen != free).any()


# ---- segments ------------------------------------------------------------------------------------------------------------------------
def _plates(max_curvature):
    pl = synth.make_plates(0.05, 0.002, 0)
    out = scan.segment_cloud({"points": pl["points"]}, 0.15, k=32, max_angle_deg=10.0, min_verts=20, max_curvature=max_curvature, device=None)
    return pl, out


def test_plates_with_the_flatness_mask_give_three_segments_none_spanning():
    pl, out = _plates(0.02)
    assert len(pl["points"]) == 861 and sorted(np.bincount(pl["plate"]).tolist()) == [420, 441]
    assert out["n_segments"] == 3 and int(out["seg_size"].sum()) == 861 and (out["instances"] > 0).all()
    flat = out["curvature"] <= np.float32(0.02)
    assert 700 <= flat.sum() < 861
    for s in (1, 2, 3):
        assert len(np.unique(pl["plate"][(out["instances"] == s) & flat])) <= 1, s # no segment holds flat points of both plates
    with_flat = [s for s in (1, 2, 3) if ((out["instances"] == s) & flat).any()]
    assert len(with_flat) == 2                                                     # the third is the crease
    assert out["normals"].shape == (861, 3) and out["normals"].dtype == np.float64 and (out["normals"] != 0).any(1).all()


def test_one_flat_plate_is_one_segment():
    pl = synth.make_plates(0.05, 0.0, 0)
    one = pl["points"][pl["plate"] == 0]
    out = scan.segment_cloud({"points": one}, 0.15, k=32, device=None)
    assert out["n_segments"] == 1 and out["seg_size"].tolist() == [441] and (out["instances"] == 1).all()
    assert (np.abs(out["normals"]) == [0, 0, 1]).all() and (out["curvature"] == 0).all()


def test_segment_cloud_equals_segment_mesh_host_on_the_edge_list():
    p = small_room()["points"].astype(np.float32)
    t = prep.knn_points_host(p, 12, float(np.float32(0.15) ** 2))
    n, c = prep.cloud_normals_host(p, t.index, t.count, 5)
    edges = prep.knn_edges(t.index)
    assert edges.shape == (len(p) * 12, 2) and edges.dtype == np.int32 and (edges[:, 0] == np.repeat(np.arange(len(p)), 12)).all()
    for unsigned in (True, False):
        got = prep.segment_cloud(torch.from_numpy(n), torch.from_numpy(t.index), 0.015, 20, unsigned=unsigned)
        want = prep.segment_mesh_host(n, edges, 0.015, 20, unsigned=unsigned)
        assert got.n_segments == want.n_segments >= 4 and torch.equal(got.labels, want.labels) and torch.equal(got.seg_size, want.seg_size)
    flipped = n * np.where(np.arange(len(n)) % 2, -1, 1).astype(np.float32)[:, None]
    a = prep.segment_mesh_host(n, edges, 0.015, 20, unsigned=True)
    b = prep.segment_mesh_host(flipped, edges, 0.015, 20, unsigned=True)
    assert torch.equal(a.labels, b.labels)                                         # the unsigned weight does not see a sign
    assert not torch.equal(prep.segment_mesh_host(flipped, edges, 0.015, 20).labels, a.labels)


def test_scan_segment_cloud_on_the_host_feeds_write_ply(tmp_path):
    room = small_room()
    path = str(tmp_path / "cloud.ply")
    scan.write_ply(path, {"points": room["points"]})                               # no faces, no normals, no ids
    assert scan.read_mesh(path)["faces"].shape == (0, 3) and scan.read_mesh(path)["normals"] is None
    out = scan.segment_cloud(path, 0.15, k=12, device=None)
    assert out["n_segments"] >= 4 and out["instances"].shape == (len(room["points"]),) and out["curvature"].dtype == np.float32
    assert int(out["seg_size"].sum()) == int((out["instances"] > 0).sum())
    kept = scan.segment_cloud({"points": room["points"], "normals": room["normals"], "faces": room["faces"]}, 0.15, k=12, device=None)
    assert np.array_equal(kept["normals"], room["normals"].astype(np.float32).astype(np.float64))    # the cloud's own normals are kept
    again = scan.segment_cloud({"points": room["points"], "normals": room["normals"]}, 0.15, k=12, device=None, recompute_normals=True)
    assert np.array_equal(again["normals"], out["normals"]) and np.array_equal(again["instances"], out["instances"])
    scan.write_ply(path, out)
    back = scan.read_mesh(path)
    assert np.array_equal(back["instances"], out["instances"]) and back["normals"] is not None
    with pytest.raises(scan.ScanError):
        scan.segment_scan({"points": room["points"]}, device=None)                 # the mesh entry still wants faces


# ---- the entry points without a device ---------------------------------------------------------------------------------------------------
def test_cloud_entry_points_refuse_what_is_out_of_range_without_a_device():
    lib = L.load()
    size = lib.vlsat_cloud_knn_scratch_bytes
    assert size(0, 8) == 0 and size((1 << 24) + 1, 8) == 0 and size(10, 0) == 0 and size(10, 33) == 0
    assert size(1, 1) > 0 and size(1000, 32) - size(1, 32) == 999 * 16 + 4000 - 16 and size(1 << 24, 32) > 20 << 24
    assert lib.vlsat_cloud_knn(0, 0, 8, 1.0, 0, 0, 0, 0, 0) != 0 and b"cloud_knn" in lib.vlsat_last_error()
    assert lib.vlsat_cloud_knn(0, 10, 8, -1.0, 0, 0, 0, 0, 0) != 0 and b"cloud_knn" in lib.vlsat_last_error()
    assert lib.vlsat_cloud_knn(0, 10, 8, 1.0, 0, 0, 0, 0, 0) != 0 and b"cloud_knn" in lib.vlsat_last_error()
    assert lib.vlsat_cloud_normals(0, 0, 0, 10, 8, 2, 0, 0.0, 0.0, 0.0, 0, 0, 0) != 0 and b"cloud_normals" in lib.vlsat_last_error()
    assert lib.vlsat_cloud_normals(0, 0, 0, 10, 33, 5, 0, 0.0, 0.0, 0.0, 0, 0, 0) != 0 and b"cloud_normals" in lib.vlsat_last_error()
    assert lib.vlsat_cloud_normals(0, 0, 0, 10, 8, 5, 1, float("nan"), 0.0, 0.0, 0, 0, 0) != 0 and b"cloud_normals" in lib.vlsat_last_error()
    assert lib.vlsat_segment_cloud(0, 0, 10, 8, 0.1, 20, 1, 0, 0, 0, 0, 0) != 0 and b"segment_cloud" in lib.vlsat_last_error()
    assert lib.vlsat_segment_cloud(0, 0, 10, 0, 0.1, 20, 1, 0, 0, 0, 0, 0) != 0 and b"segment_cloud" in lib.vlsat_last_error()
    assert lib.vlsat_segment_cloud(0, 0, 10, 8, float("nan"), 20, 1, 0, 0, 0, 0, 0) != 0 and b"segment_cloud" in lib.vlsat_last_error()
