"""The convexity clusters on the GPU (csrc/convex.hip): every output -- labels, n_clusters, cluster_size, state -- EQUAL to the host
restatement on the tables made by hand (pads, entries out of range, self entries, NaN / inf distances, masks 0 / 7 / -1), on 1, 2, 64, 65
and 257 points with 1, 16 and 32 neighbours, on the two plates seen from either side, on the stacked boxes with estimated and with
exact normals, with rows of NaN coordinates and normals, with a mask that removes a body, with 0, 1, 8 and 64 absorption rounds and
min_points 1 and 20; two runs bit-equal; every entry of every output written; refused arguments refused before any launch;
scan.segment_objects with concavity_deg on the device equal to the host, with voxel=, and on into prepare_scan."""
import numpy as np
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import lib as L, prep, scan

import convex_checks as CC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path cannot run and there is no fallback")


def _device(**a):
    put = lambda x: torch.from_numpy(np.array(x)).to(DEV) if isinstance(x, np.ndarray) else x       # noqa: E731
    out = prep.convex_clusters(**{k: put(x) for k, x in a.items()})
    assert isinstance(out, prep.ConvexClusters) and all(x.is_cuda and x.dtype == torch.int32 for x in out)
    return [x.cpu().numpy() for x in out]


@pytest.mark.parametrize("name", CC.CASES)
def test_equal_to_the_restatement(name):
    _need_gpu()
    got = _device(**CC.case(name))
    CC.assert_same(got, CC.host(name), name)
    if name in ("hand_wild", "v257_k16", "plates_concave", "stacked", "stacked_nonfinite"):
        CC.assert_same(_device(**CC.case(name)), got, (name, "second run"))


def test_on_the_device_table_and_device_normals():
    """the route of scan.segment_objects piece by piece: the device's own table and normals (test_hip_cloud.py compares both with their
    restatements) give what the host's give"""
    _need_gpu()
    p, scene, table, est, exact = CC.stacked()
    d_p = torch.from_numpy(np.array(p)).to(DEV)
    t = prep.knn_points(d_p, 16, CC._sq(0.06))
    n = prep.cloud_normals(d_p, t.index, t.count, 5, scene["viewpoint"])[0]
    out = prep.convex_clusters(d_p, n, t.index, t.sqdist, torch.ones(len(p), dtype=torch.int32, device=DEV), CC._sq(0.03), 0.17, 20, 8)
    CC.assert_same([x.cpu().numpy() for x in out], CC.host("stacked"))
    assert out.n_clusters.tolist() == [6]


def test_every_output_entry_is_written_and_errors_touch_nothing():
    """the C entry point directly: outputs pre-filled with a pattern; a good call leaves none of it, a refused call leaves all of it and
    returns VLSAT_EINVAL before anything is launched"""
    _need_gpu()
    lib = L.load()
    a = CC.case("plates_concave")
    v, k = a["knn_index"].shape
    d = {key: torch.from_numpy(np.array(a[key])).to(DEV) for key in ("points", "normals", "knn_index", "knn_sqdist", "mask")}
    scratch = torch.empty(int(lib.vlsat_convex_clusters_scratch_bytes(v)), dtype=torch.uint8, device=DEV)
    fill = 0x5A5A5A5A

    def outputs():
        return [torch.full((n,), fill, dtype=torch.int32, device=DEV) for n in (v, 1, v, v)]

    def call(out, null=None, **change):
        c = {**dict(v=v, k=k, link=a["link_sq_dist"], tau=a["concavity"], min_points=a["min_points"], rounds=a["absorb_rounds"]), **change}
        ptr = [d["points"].data_ptr(), d["normals"].data_ptr(), d["knn_index"].data_ptr(), d["knn_sqdist"].data_ptr(), d["mask"].data_ptr(),
               scratch.data_ptr(), *(x.data_ptr() for x in out)]
        if null is not None:
            ptr[null] = 0
        return lib.vlsat_convex_clusters(*ptr[:5], c["v"], c["k"], c["link"], c["tau"], c["min_points"], c["rounds"], *ptr[5:], L.stream_ptr())

    out = outputs()
    assert call(out) == 0
    CC.assert_same([x.cpu().numpy() for x in out], CC.host("plates_concave"))
    assert not any(bool((x == fill).any()) for x in out)
    for change in (dict(v=0), dict(v=(1 << 24) + 1), dict(k=0), dict(k=33), dict(link=float("nan")), dict(tau=-0.01), dict(tau=1.01),
                   dict(tau=float("nan")), dict(min_points=0), dict(rounds=-1), dict(rounds=65), *(dict(null=i) for i in range(10))):
        out = outputs()
        assert call(out, **change) == -1, change
        assert lib.vlsat_last_error().decode().startswith("convex_clusters:")
        torch.cuda.synchronize()
        assert all(bool((x == fill).all()) for x in out), change
    for bad in (lambda: prep.convex_clusters(d["points"][:5], d["normals"], d["knn_index"], d["knn_sqdist"], d["mask"], 0.01, 0.17),
                lambda: prep.convex_clusters(d["points"], d["normals"], d["knn_index"], d["knn_sqdist"][:, :2], d["mask"], 0.01, 0.17),
                lambda: prep.convex_clusters(d["points"], d["normals"], d["knn_index"], d["knn_sqdist"], d["mask"], 0.01, 1.5),
                lambda: prep.convex_clusters(d["points"], d["normals"], d["knn_index"], d["knn_sqdist"], d["mask"], 0.01, 0.17, absorb_rounds=65)):
        with pytest.raises(L.VlsatError):
            bad()


def _same(dev, host):
    assert dev["n_planes"] == host["n_planes"] and dev["n_segments"] == host["n_segments"]
    assert np.array_equal(dev["instances"], host["instances"]) and np.array_equal(dev["seg_size"], host["seg_size"])
    assert np.array_equal(dev["planes"].view(np.uint32), host["planes"].view(np.uint32)) and np.array_equal(dev["concave"], host["concave"])


def test_segment_objects_device_equals_host():
    """the stacked boxes on a floor: a plane is found and removed first; plain, with carried normals and with voxel="""
    _need_gpu()
    points, view = CC.floor_scene()
    kw = dict(dist=0.01, cluster_radius=0.03, n_hyp=64, max_planes=2, min_plane_share=0.3, min_points=20, concavity_deg=10)
    dev = scan.segment_objects({"points": points}, viewpoint=view, device=DEV, **kw)
    _same(dev, scan.segment_objects({"points": points}, viewpoint=view, device=None, **kw))
    assert dev["n_planes"] == 1 and dev["n_segments"] >= 6 and dev["concave"].any()
    normals = np.tile([0.0, 0.0, 2.0], (len(points), 1))
    from vlsat_amd import synth
    normals[:7211] = synth.make_stacked_boxes()["normals"]
    _same(scan.segment_objects({"points": points, "normals": normals}, device=DEV, **kw),
          scan.segment_objects({"points": points, "normals": normals}, device=None, **kw))
    twice = np.concatenate([points, points[:3000] + 0.001, [[np.nan, 0.0, 0.0]]])             # voxel=: gathered back to every input point
    dev = scan.segment_objects({"points": twice}, viewpoint=view, voxel=0.02, device=DEV, **kw)
    host = scan.segment_objects({"points": twice}, viewpoint=view, voxel=0.02, device=None, **kw)
    _same(dev, host)
    _same(dev["resampled"], host["resampled"])
    assert len(dev["instances"]) == len(twice) and dev["instances"][-1] == 0 and not dev["concave"][-1] and dev["n_segments"] >= 6


def test_segment_objects_with_concavity_into_prepare_scan(tmp_path):
    """a faceless PLY -> segment_objects(concavity_deg=10) -> prepare_scan on the device: one node per plane and cluster"""
    _need_gpu()
    points, view = CC.floor_scene()
    path = str(tmp_path / "cloud.ply")
    scan.write_ply(path, {"points": points})
    cloud = scan.segment_objects(path, 0.01, 0.03, n_hyp=64, max_planes=2, min_plane_share=0.3, min_points=20, concavity_deg=10, viewpoint=view,
                                 device=DEV)
    s = cloud["n_segments"]
    assert cloud["n_planes"] == 1 and s >= 6 and (cloud["seg_size"] > 0).all()
    from vlsat_amd import VLSATConfig
    cfg = VLSATConfig(N_LAYERS=1)
    relations = [f"r{k}" for k in range(cfg.num_rel_class)]
    b = scan.prepare_scan(cloud, {i: "?" for i in range(1, s + 1)}, ["?"], [], relations, num_points=32, seed=0, device=DEV)
    assert b["instance_ids"] == list(range(1, s + 1)) and b["points_per_instance"].tolist() == cloud["seg_size"].tolist()
    assert b["obj_points"].shape[0] == s
