"""The object segmenter on the GPU (csrc/objects.hip): every output EQUAL bit for bit to the host restatement -- plane_id, the bits of
planes, plane_counts and n_planes on the jittered box room (11 245 points) with 1, 65, 256 and 300 hypotheses (a lone lane, a block with
a tail, a full block, two hypotheses per thread), the two plates, the walled room, 3, 64, 65 and 257 points, rows with NaN / inf,
coordinates near the largest float, coincident points, max_planes beyond the planes present (the later rounds return at once) and
max_planes = 1, 1024 hypotheses (four per thread); labels, n_clusters and cluster_size on tables made by hand and on the rooms' own
tables, with and without a mask; two runs bit-equal; every entry of every output written; refused arguments refused before any launch;
scan.segment_objects on the device equal to the host, with voxel=, and on into prepare_scan."""
import ctypes

import numpy as np
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import lib as L, prep, scan

import objects_checks as OC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path cannot run and there is no fallback")


def _planes(points, **kw):
    out = prep.cloud_planes(torch.from_numpy(np.array(points)).to(DEV), **kw)
    assert isinstance(out, prep.CloudPlanes) and all(x.is_cuda for x in out)
    return [x.cpu().numpy() for x in out]


def _clusters(index, sqdist, mask, max_sq_dist, min_points):
    put = lambda x: torch.from_numpy(np.array(x)).to(DEV)       # noqa: E731
    out = prep.cloud_clusters(put(index), put(sqdist), put(mask), max_sq_dist, min_points)
    assert isinstance(out, prep.CloudClusters) and all(x.is_cuda for x in out)
    return [x.cpu().numpy() for x in out]


@pytest.mark.parametrize("name", OC.PLANE_CASES)
def test_planes_equal_the_restatement(name):
    _need_gpu()
    p, kw = OC.case(name)
    got = _planes(p, **kw)
    OC.assert_same_planes(got, OC.host_planes(name), name)
    if name in ("boxes_h300", "walled", "v65"):
        OC.assert_same_planes(_planes(p, **kw), got, (name, "second run"))


def test_four_hypotheses_per_thread_and_two_groups():
    """1024 and 1100 hypotheses: four per thread, and a second hypothesis group with a tail, on a thinned room (2249 points: three tiles)"""
    _need_gpu()
    p = OC.boxes()[0][::5]
    for n_hyp in (1024, 1100):
        kw = dict(n_hyp=n_hyp, max_planes=2, dist=0.02, min_inliers=45, outside_ppm=10000, seed=n_hyp)
        want = prep.cloud_planes_host(p, **kw)
        assert int(want.n_planes[0]) >= 1
        OC.assert_same_planes(_planes(p, **kw), want, n_hyp)


def test_every_output_entry_is_written_and_errors_touch_nothing():
    """the C entry points directly: outputs pre-filled with a pattern; a good call leaves none of it, a refused call leaves all of it
    and returns VLSAT_EINVAL before anything is launched"""
    _need_gpu()
    lib = L.load()
    p, kw = OC.case("plates")
    v, h, planes_max = len(p), kw["n_hyp"], kw["max_planes"]
    d_p = torch.from_numpy(np.array(p)).to(DEV)
    scratch = torch.empty(int(lib.vlsat_cloud_planes_scratch_bytes(v, h)), dtype=torch.uint8, device=DEV)
    fill = 0x5A5A5A5A

    def outputs():
        return [torch.full(shape, fill, dtype=torch.int32, device=DEV) for shape in ((v,), (planes_max, 4), (planes_max, 3), (1,))]

    def call(out, **change):
        a = {**dict(v=v, **kw), **change}
        return lib.vlsat_cloud_planes(d_p.data_ptr(), a["v"], a["n_hyp"], a["max_planes"], a["dist"], a["min_inliers"], a["outside_ppm"],
                                      a["seed"], scratch.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                      out[3].data_ptr(), L.stream_ptr())

    out = outputs()
    assert call(out) == 0
    want = OC.host_planes("plates")
    assert np.array_equal(out[0].cpu().numpy(), want.plane_id) and np.array_equal(out[1].cpu().numpy().view(np.float32).view(np.uint32),
                                                                                  want.planes.view(np.uint32))
    assert np.array_equal(out[2].cpu().numpy(), want.counts) and out[3].tolist() == [2]
    for change in (dict(v=2), dict(v=(1 << 24) + 1), dict(n_hyp=0), dict(n_hyp=4097), dict(max_planes=0), dict(max_planes=33), dict(dist=0.0),
                   dict(dist=float("nan")), dict(dist=float("inf")), dict(dist=-0.5), dict(min_inliers=2), dict(outside_ppm=-1),
                   dict(outside_ppm=500001)):
        out = outputs()
        assert call(out, **change) == -1, change
        assert lib.vlsat_last_error().decode().startswith("cloud_planes:")
        torch.cuda.synchronize()
        assert all(bool((x == fill).all()) for x in out), change
    assert lib.vlsat_cloud_planes(0, v, h, 1, 0.1, 3, 0, 0, scratch.data_ptr(), 0, 0, 0, 0, L.stream_ptr()) == -1         # null pointers
    # clusters
    t = OC.knn(OC.blobs(1)[0], 8, 0.6)
    n, k = t.index.shape
    d_i, d_d = torch.from_numpy(t.index).to(DEV), torch.from_numpy(t.sqdist).to(DEV)
    d_m = torch.ones(n, dtype=torch.int32, device=DEV)
    cs = torch.empty(int(lib.vlsat_cloud_clusters_scratch_bytes(n)), dtype=torch.uint8, device=DEV)

    def couts():
        return [torch.full(shape, fill, dtype=torch.int32, device=DEV) for shape in ((n,), (1,), (n,))]

    def ccall(out, **change):
        a = {**dict(n=n, k=k, r2=0.36, min_points=1), **change}
        return lib.vlsat_cloud_clusters(d_i.data_ptr(), d_d.data_ptr(), d_m.data_ptr(), a["n"], a["k"], a["r2"], a["min_points"], cs.data_ptr(),
                                        out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), L.stream_ptr())

    out = couts()
    assert ccall(out) == 0
    want = prep.cloud_clusters_host(t.index, t.sqdist, np.ones(n, np.int32), float(ctypes.c_float(0.36).value), 1)
    OC.assert_same_clusters([x.cpu().numpy() for x in out], want)
    for change in (dict(n=0), dict(n=(1 << 24) + 1), dict(k=0), dict(k=33), dict(r2=float("nan")), dict(min_points=0)):
        out = couts()
        assert ccall(out, **change) == -1, change
        torch.cuda.synchronize()
        assert all(bool((x == fill).all()) for x in out), change
    for bad in (lambda: prep.cloud_planes(d_p.double(), **kw), lambda: prep.cloud_planes(d_p[:2], **kw),
                lambda: prep.cloud_planes(d_p, **{**kw, "dist": 1e39}), lambda: prep.cloud_clusters(d_i, d_d[:, :1], d_m, 0.36, 1),
                lambda: prep.cloud_clusters(d_i, d_d, d_m[:3], 0.36, 1)):
        with pytest.raises(L.VlsatError):
            bad()


def test_clusters_on_tables_made_by_hand():
    _need_gpu()
    r2 = float(np.float32(0.6) ** 2)
    p, mask0 = OC.blobs(0)
    t = OC.knn(p, 8, 0.6)
    apart = _clusters(t.index, t.sqdist, mask0, r2, 5)
    OC.assert_same_clusters(apart, OC.brute_clusters(t.index, t.sqdist, mask0, r2, 5))
    assert apart[1].tolist() == [2] and apart[0].tolist() == [1] * 30 + [2] * 30 + [0]       # a bridge of mask 0 joins nothing
    joined = _clusters(t.index, t.sqdist, OC.blobs(1)[1], r2, 5)
    assert joined[1].tolist() == [1] and (joined[0] == 1).all() and joined[2][0] == 61        # the same point with mask 1 does
    both = np.concatenate([p[:30], p[30:49]])                                                # 30 and 19 points: min_points 20 drops the 19
    tb = OC.knn(both, 8, 0.6)
    ones = np.ones(len(both), dtype=np.int32)
    for min_points in (19, 20):
        want = OC.brute_clusters(tb.index, tb.sqdist, ones, r2, min_points)
        OC.assert_same_clusters(_clusters(tb.index, tb.sqdist, ones, r2, min_points), want, min_points)
    assert want[0].tolist() == [1] * 30 + [0] * 19
    perm = np.random.default_rng(3).permutation(len(both))                                   # numbering by lowest point under a permutation
    tp = OC.knn(both[perm], 8, 0.6)
    got = _clusters(tp.index, tp.sqdist, ones, r2, 1)
    OC.assert_same_clusters(got, OC.brute_clusters(tp.index, tp.sqdist, ones, r2, 1))
    assert got[0][0] == 1 and got[1].tolist() == [2]
    index = np.array([[1, -1, 7], [0, 5, -3], [3, 2, 1 << 30], [2, -1, -1], [4, 4, 4]], dtype=np.int32)      # pads and entries out of range
    sqdist = np.array([[0.1, np.inf, 0.0], [0.1, 0.0, 0.0], [0.2, 0.0, 0.0], [np.nan, np.inf, np.inf], [0.0, 0.0, 0.0]], dtype=np.float32)
    for mask, limit, min_points in ((np.ones(5, np.int32), 0.5, 1), (np.zeros(5, np.int32), 0.5, 1), (np.array([1, 1, 1, 1, 0], np.int32), 0.15, 2),
                                    (np.array([7, -1, 1, 1, 1], np.int32), np.inf, 1)):
        OC.assert_same_clusters(_clusters(index, sqdist, mask, limit, min_points), OC.brute_clusters(index, sqdist, mask, limit, min_points))
    assert _clusters(index, sqdist, np.ones(5, np.int32), 0.5, 1)[0].tolist() == [1, 1, 2, 2, 3]


@pytest.mark.parametrize("name,radius,k", [("boxes_h256", 0.15, 16), ("walled", 0.15, 16), ("nonfinite", 0.3, 4), ("v257", 0.4, 32)])
def test_clusters_on_the_rooms_equal_the_restatement(name, radius, k):
    """the table of the WHOLE cloud (the device's own, which test_hip_cloud.py compares with its restatement) and the mask "no plane took
    this point": components of several thousand points down to single points, invalid rows, several blocks; two runs bit-equal"""
    _need_gpu()
    p = OC.case(name)[0]
    r2 = float(np.float32(radius) ** 2)
    table = prep.knn_points(torch.from_numpy(np.array(p)).to(DEV), k, r2)
    index, sqdist = table.index.cpu().numpy(), table.sqdist.cpu().numpy()
    mask = ((OC.host_planes(name).plane_id == 0) & np.isfinite(p).all(1)).astype(np.int32)
    assert 0 < mask.sum() < len(p)
    for m, min_points in ((mask, 20), (mask, 1), (np.ones(len(p), np.int32), 3)):
        want = prep.cloud_clusters_host(index, sqdist, m, r2, min_points)
        got = _clusters(index, sqdist, m, r2, min_points)
        OC.assert_same_clusters(got, want, (name, min_points))
        OC.assert_same_clusters(_clusters(index, sqdist, m, r2, min_points), got, (name, "second run"))
    assert int(want.n_clusters[0]) >= 1


def _same(dev, host):
    assert dev["n_planes"] == host["n_planes"] and dev["n_segments"] == host["n_segments"]
    assert np.array_equal(dev["instances"], host["instances"]) and np.array_equal(dev["seg_size"], host["seg_size"])
    assert np.array_equal(dev["planes"].view(np.uint32), host["planes"].view(np.uint32))


def test_segment_objects_device_equals_host():
    _need_gpu()
    p = OC.boxes()[0].astype(np.float64)
    kw = dict(dist=0.02, cluster_radius=0.15, n_hyp=256, min_plane_share=0.02, outside_frac=0.01, min_points=20)
    host = scan.segment_objects({"points": p}, device=None, **kw)
    dev = scan.segment_objects({"points": p}, device=DEV, **kw)
    _same(dev, host)
    assert dev["n_segments"] == dev["n_planes"] + 3 and (dev["instances"] > 0).all()
    walls = OC.walled()[0]
    kw = dict(dist=0.02, cluster_radius=0.15, n_hyp=256, max_planes=8, min_plane_share=0.012, outside_frac=0.01, min_points=20)
    dev = scan.segment_objects({"points": walls}, device=DEV, **kw)
    _same(dev, scan.segment_objects({"points": walls}, device=None, **kw))
    assert dev["n_planes"] == 5
    twice = np.concatenate([p, p[:4000] + 0.003, [[np.nan, 0.0, 0.0]]])                      # voxel=: gathered back to every input point
    kw = dict(dist=0.02, cluster_radius=0.15, n_hyp=128, min_plane_share=0.02, min_points=20, voxel=0.05)
    dev = scan.segment_objects({"points": twice}, device=DEV, **kw)
    host = scan.segment_objects({"points": twice}, device=None, **kw)
    _same(dev, host)
    _same(dev["resampled"], host["resampled"])
    assert len(dev["instances"]) == len(twice) and dev["instances"][-1] == 0 and (dev["instances"][:-1] > 0).all()


def test_segment_objects_into_prepare_scan_and_a_decoded_graph(tmp_path):
    """a faceless PLY -> segment_objects -> prepare_scan -> decode_graph -> to_annotation on the device: one node per plane and cluster"""
    _need_gpu()
    from vlsat_amd import VLSATConfig, scene_graph as SG, synth
    from vlsat_amd.model import VLSATModel
    path = str(tmp_path / "cloud.ply")
    scan.write_ply(path, {"points": OC.boxes()[0]})
    cloud = scan.segment_objects(path, 0.02, 0.15, n_hyp=256, min_points=20, device=DEV)
    s = cloud["n_segments"]
    assert s == cloud["n_planes"] + 3
    cfg = VLSATConfig(N_LAYERS=1)
    relations = [f"r{k}" for k in range(cfg.num_rel_class)]
    b = scan.prepare_scan(cloud, {i: "?" for i in range(1, s + 1)}, ["?"], [], relations, num_points=32, seed=0, device=DEV)
    assert b["instance_ids"] == list(range(1, s + 1)) and b["points_per_instance"].tolist() == cloud["seg_size"].tolist()
    assert b["obj_points"].shape[0] == s
    m = VLSATModel(cfg, DEV).load_state(synth.make_weights(cfg)).eval()
    g3d, none = m.decode_graph(b["obj_points"], None, b["edge_indices"].t().contiguous(), b["descriptor"], threshold=0.5, n_labels=3, max_rel=256)
    assert none is None and g3d.labels.shape == (s, 3)
    classes = [f"c{k}" for k in range(cfg.num_obj_class)]
    entry = SG.to_annotation(g3d, 0, b["edge_indices"], b["instance_ids"], classes, ["none"] + relations, "room")
    assert set(entry["objects"]) == {str(i) for i in range(1, s + 1)}
