"""The point-cloud front end on the GPU (csrc/cloud.hip, vlsat_segment_cloud in csrc/mesh_segment.hip): every output EQUAL bit for bit
to the host restatement, each stage on that stage's own inputs -- the neighbour tables for K = 1, 8, 9, 16, 32 (all three register
capacities, K below a capacity) on clouds with distance ties, duplicates, non-finite rows, one point, 257 points, counts below and above
K, radius 0, one cell and many cells; the normals on those tables with and without a viewpoint; the segments, signed and unsigned,
against segment_mesh_host on the explicit edge list; the mesh entry unchanged; two runs bit-equal; scan.segment_cloud on the device
equal to the host; and the whole route from a faceless PLY to a written graph."""
import numpy as np
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import lib as L, prep, scan

from cloud_checks import CLOUDS, KS, VIEWPOINT, assert_bit_equal, cloud, host_knn, host_normals, small_room
from mesh_segment_checks import assert_same, host_result, room_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path cannot run and there is no fallback")


def _device_knn(name, k):
    p, m = cloud(name)
    return prep.knn_points(torch.from_numpy(p.copy()).to(DEV), k, m)


def _assert_table(got, want, what):
    assert got.index.is_cuda and got.index.dtype == torch.int32 and got.sqdist.dtype == torch.float32 and got.count.dtype == torch.int32
    for g, w, part in zip(got, want, ("index", "sqdist", "count")):
        assert_bit_equal(g.cpu().numpy(), w, (what, part))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", list(CLOUDS))
def test_neighbours_equal_the_restatement(name, k):
    _need_gpu()
    _assert_table(_device_knn(name, k), host_knn(name, k), (name, k))


def test_the_clouds_cover_what_they_claim():
    assert host_knn("single", 8).count.tolist() == [0] and len(cloud("v257")[0]) == 257
    c = host_knn("density", 32).count
    assert c.min() == 0 and c.max() == 32 and ((c > 0) & (c < 32)).any()
    assert host_knn("one_cell", 32).count.min() == 32 and host_knn("grid", 32).count.max() == 18   # 6 at 1/8 and 12 at sqrt(2)/8
    d = host_knn("grid", 8).sqdist
    assert (d[:, 0] == d[:, 2]).all()                                               # ties: three or more neighbours at the nearest distance
    assert (host_knn("duplicates", 8).sqdist[:, :2] == 0).all() and (host_knn("nonfinite", 8).count == 0).sum() >= 72
    assert set(np.unique(host_knn("radius0", 9).count)) == {0, 1, 2}


@pytest.mark.parametrize("name", list(CLOUDS))
def test_normals_equal_the_restatement(name):
    _need_gpu()
    p = torch.from_numpy(cloud(name)[0].copy()).to(DEV)
    for k in KS:
        t = host_knn(name, k)
        index, count = torch.from_numpy(t.index).to(DEV), torch.from_numpy(t.count).to(DEV)
        for with_viewpoint in (False, True):
            n, c = prep.cloud_normals(p, index, count, 5, VIEWPOINT if with_viewpoint else None)
            wn, wc = host_normals(name, k, with_viewpoint)
            assert_bit_equal(n.cpu().numpy(), wn, (name, k, with_viewpoint, "normals"))
            assert_bit_equal(c.cpu().numpy(), wc, (name, k, with_viewpoint, "curvature"))
    assert name in ("single", "radius0") or (host_normals(name, 16, False)[0] != 0).any()


def test_normals_of_a_foreign_table():
    """a table nobody made with knn_points: counts outside [0, K], entries outside [0, V) in the listed part, min_points 3"""
    _need_gpu()
    p, _ = cloud("v257")
    g = np.random.default_rng(11)
    index = g.integers(-3, 260, (257, 9)).astype(np.int32)
    count = g.integers(-2, 12, 257).astype(np.int32)
    n, c = prep.cloud_normals(torch.from_numpy(p.copy()).to(DEV), torch.from_numpy(index).to(DEV), torch.from_numpy(count).to(DEV), 3, (0.0, 0.0, 9.0))
    wn, wc = prep.cloud_normals_host(p, index, count, 3, (0.0, 0.0, 9.0))
    assert_bit_equal(n.cpu().numpy(), wn)
    assert_bit_equal(c.cpu().numpy(), wc)
    assert (wn != 0).any() and (wc == 1).any()


def _segment_case(name, k, mask):
    """(normals, table, max_weight, min_verts): restated normals on the restated table, optionally with the flatness mask's zero normals"""
    t = host_knn(name, k)
    n, c = host_normals(name, k, False)
    if mask:
        n = np.where((c > np.float32(0.02))[:, None], np.float32(0), n)
    return n, t.index, float(np.float32(1.0 - np.cos(np.radians(10.0)))), 20


@pytest.mark.parametrize("unsigned", [True, False])
@pytest.mark.parametrize("name,k,mask", [("grid", 16, False), ("density", 9, True), ("many_cells", 8, True), ("nonfinite", 32, False)])
def test_segments_equal_segment_mesh_host_on_the_edge_list(name, k, mask, unsigned):
    _need_gpu()
    n, index, max_weight, min_verts = _segment_case(name, k, mask)
    got = prep.segment_cloud(torch.from_numpy(n).to(DEV), torch.from_numpy(index).to(DEV), max_weight, min_verts, unsigned=unsigned)
    want = prep.segment_mesh_host(n, prep.knn_edges(index), max_weight, min_verts, unsigned=unsigned)
    assert_same(got, want, (name, k, mask, unsigned))
    listed = prep.segment_mesh(torch.from_numpy(n).to(DEV), prep.knn_edges(torch.from_numpy(index).to(DEV)), max_weight, min_verts)
    if not unsigned:
        assert_same(listed, want, "the list entry on the same edges")


def test_room_cloud_segments_and_untrimmed():
    _need_gpu()
    p = small_room()["points"].astype(np.float32)
    t = prep.knn_points_host(p, 12, float(np.float32(0.15) ** 2))
    n, _ = prep.cloud_normals_host(p, t.index, t.count, 5)
    dn, di = torch.from_numpy(n).to(DEV), torch.from_numpy(t.index).to(DEV)
    want = prep.segment_mesh_host(n, prep.knn_edges(t.index), 0.015, 20, unsigned=True)
    assert want.n_segments >= 4
    assert_same(prep.segment_cloud(dn, di, 0.015, 20), want)
    full = prep.segment_cloud(dn, di, 0.015, 20, trim=False)
    assert not full.trimmed and full.n_segments.is_cuda and full.seg_size.shape == full.labels.shape
    assert_same(full.trim(), want)


def test_the_mesh_entry_is_unchanged():
    """vlsat_segment_mesh shares its kernels with vlsat_segment_cloud as template instances: the box room through its own restatement"""
    _need_gpu()
    normals, edges, max_weight, min_verts = room_case(0.05)
    assert_same(prep.segment_mesh(normals.to(DEV), edges.to(DEV), max_weight, min_verts), host_result(("room", 0.05)))


def test_two_runs_are_bit_equal():
    _need_gpu()
    a, b = _device_knn("many_cells", 16), _device_knn("many_cells", 16)
    for x, y in zip(a, b):
        assert_bit_equal(x.cpu().numpy(), y.cpu().numpy())
    p = torch.from_numpy(cloud("many_cells")[0].copy()).to(DEV)
    na, nb = prep.cloud_normals(p, a.index, a.count), prep.cloud_normals(p, b.index, b.count)
    assert_bit_equal(na[0].cpu().numpy(), nb[0].cpu().numpy())
    assert_bit_equal(na[1].cpu().numpy(), nb[1].cpu().numpy())
    sa, sb = prep.segment_cloud(na[0], a.index, 0.015, 20), prep.segment_cloud(nb[0], b.index, 0.015, 20)
    assert_same(sa, sb)


def _same_result(got, want):
    assert got["n_segments"] == want["n_segments"] and np.array_equal(got["instances"], want["instances"])
    assert np.array_equal(got["seg_size"], want["seg_size"])
    assert_bit_equal(got["normals"], want["normals"], "normals")
    assert_bit_equal(got["curvature"], want["curvature"], "curvature")


def test_scan_segment_cloud_device_equals_host():
    _need_gpu()
    room = small_room()
    for given in ({"points": room["points"], "normals": room["normals"]}, {"points": room["points"]}):     # faces removed
        for viewpoint in (None, (1.5, 1.5, 4.0)):
            host = scan.segment_cloud(given, 0.15, k=12, viewpoint=viewpoint, device=None)
            dev = scan.segment_cloud(given, 0.15, k=12, viewpoint=viewpoint, device=DEV)
            _same_result(dev, host)
            assert host["n_segments"] >= 4


def test_refused_arguments():
    _need_gpu()
    p = torch.zeros(4, 3, device=DEV)
    with pytest.raises(L.VlsatError):
        prep.knn_points(p.double(), 4, 1.0)
    with pytest.raises(L.VlsatError):
        prep.knn_points(p, 33, 1.0)
    with pytest.raises(L.VlsatError):
        prep.knn_points(p, 4, float("nan"))
    t = prep.knn_points(p, 4, 1.0)
    assert t.count.tolist() == [3, 3, 3, 3] and t.index[0].tolist() == [1, 2, 3, -1]   # coincident points are each other's neighbours
    with pytest.raises(L.VlsatError):
        prep.cloud_normals(p, t.index, t.count, 2)
    with pytest.raises(L.VlsatError):
        prep.segment_cloud(p, t.index[:3], 0.1)
    with pytest.raises(L.VlsatError):
        prep.segment_cloud(p, t.index, float("nan"))
    lib = L.load()
    out = torch.zeros(64, dtype=torch.int32, device=DEV)
    scratch = torch.empty(int(lib.vlsat_cloud_knn_scratch_bytes(4, 4)), dtype=torch.uint8, device=DEV)
    args = lambda **k: [k.get("points", p.data_ptr()), k.get("v", 4), k.get("k", 4), k.get("m", 1.0), k.get("scratch", scratch.data_ptr()),
                        out.data_ptr(), out.data_ptr(), out.data_ptr(), L.stream_ptr()]
    for bad in (dict(points=0), dict(scratch=0), dict(v=0), dict(v=(1 << 24) + 1), dict(k=0), dict(k=33), dict(m=-1.0), dict(m=float("nan"))):
        assert lib.vlsat_cloud_knn(*args(**bad)) != 0, bad
        assert b"cloud_knn" in lib.vlsat_last_error()


def test_faceless_ply_to_decoded_graph(tmp_path):
    """the 3-box room as a cloud: write_ply without faces -> segment_cloud -> prepare_scan -> decode_graph(obj_2d_feats=None) ->
    to_annotation, on the device"""
    _need_gpu()
    from vlsat_amd import VLSATConfig, scene_graph as SG, synth
    from vlsat_amd.model import VLSATModel
    room = small_room()
    path = str(tmp_path / "cloud.ply")
    scan.write_ply(path, {"points": room["points"]})
    cloud_ = scan.segment_cloud(path, 0.15, k=12, device=DEV)
    _same_result(cloud_, scan.segment_cloud(path, 0.15, k=12, device=None))
    s = cloud_["n_segments"]
    assert s >= 4
    cfg = VLSATConfig(N_LAYERS=1)
    relations = [f"r{k}" for k in range(cfg.num_rel_class)]
    b = scan.prepare_scan(cloud_, {i: "?" for i in range(1, s + 1)}, ["?"], [], relations, num_points=32, seed=0, device=DEV)
    assert b["instance_ids"] == list(range(1, s + 1)) and b["points_per_instance"].tolist() == cloud_["seg_size"].tolist()
    m = VLSATModel(cfg, DEV).load_state(synth.make_weights(cfg)).eval()
    g3d, none = m.decode_graph(b["obj_points"], None, b["edge_indices"].t().contiguous(), b["descriptor"], threshold=0.5, n_labels=3, max_rel=256)
    assert none is None and g3d.labels.shape == (s, 3)
    classes = [f"c{k}" for k in range(cfg.num_obj_class)]
    entry = SG.to_annotation(g3d, 0, b["edge_indices"], b["instance_ids"], classes, ["none"] + relations, "room")
    assert set(entry["objects"]) == {str(i) for i in range(1, s + 1)}
