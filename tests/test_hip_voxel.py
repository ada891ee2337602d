"""The voxel-grid filter on the GPU (csrc/voxel.hip): every output EQUAL bit for bit to the host restatement -- eight clouds at three
cell edges each (one voxel for all: every atomic hits one destination; a voxel per point; in between, about a thousand voxels on
many_cells and so probe collisions), min_count 1, 2 and above every count (M = 0: empty outputs, nothing launched), with and without
normals and colours, a non-zero origin, points on cell faces, both signs, points and cells out of range, normals that cancel or are not
finite, 65 and 257 points for the wave and block edges of the scan, 300 000, 262 144 and 262 145 points for the scan of the per-block counts, two runs
bit-equal; scan.downsample_cloud and scan.segment_cloud(voxel=...) on the device equal to the host; and the route from a faceless PLY
through resampling and segmentation to a written graph."""
import numpy as np
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import lib as L, prep, scan

import voxel_checks as VC
from cloud_checks import assert_bit_equal, cloud, small_room

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path cannot run and there is no fallback")


def _device(points, voxel, origin=(0.0, 0.0, 0.0), min_count=1, normals=None, colors=None):
    put = lambda x: None if x is None else torch.from_numpy(np.array(x)).to(DEV)       # noqa: E731
    out = prep.voxel_downsample(put(points), voxel, origin, min_count, put(normals), put(colors))
    assert isinstance(out, prep.VoxelCloud) and all(x is None or x.is_cuda for x in out)
    assert out.points.shape == (len(out.count), 3) and out.first_point.shape == out.count.shape and out.voxel_of_point.shape == (len(points),)
    return [None if x is None else x.cpu().numpy() for x in out]


@pytest.mark.parametrize("size", VC.SIZES)
@pytest.mark.parametrize("name", VC.NAMES)
def test_device_equals_the_restatement(name, size):
    _need_gpu()
    p = cloud(name)[0]
    voxel, origin = VC.setting(name, size)
    n, c = VC.attributes(name)
    VC.assert_same_cloud(_device(p, voxel, origin), VC.host_case(name, size), (name, size))
    for min_count in (1, 2, 10 ** 6):
        want = VC.host_case(name, size, min_count, True)
        VC.assert_same_cloud(_device(p, voxel, origin, min_count, n, c), want, (name, size, min_count, "normals and colours"))
    assert len(VC.host_case(name, size, 10 ** 6, True).points) == 0                  # M = 0: empty outputs


@pytest.mark.parametrize("name", VC.SPECIAL)
def test_device_equals_the_restatement_on_the_further_settings(name):
    _need_gpu()
    VC.assert_same_cloud(_device(*VC.special(name)), VC.host_special(name), name)


def test_normals_alone_and_colours_alone():
    _need_gpu()
    p = cloud("density")[0]
    n, c = VC.attributes("density")
    both = VC.host_case("density", "between", 1, True)
    only_n, only_c = _device(p, 0.5, normals=n), _device(p, 0.5, colors=c)
    assert only_n[2] is None and only_c[1] is None
    assert_bit_equal(only_n[1], both.normals)
    assert_bit_equal(only_c[2], both.colors)
    assert_bit_equal(only_c[0], both.points)


def test_the_scan_of_the_block_counts():
    """300 000 points are 1172 blocks of 256: the one-block scan of the per-block head counts takes two counts per thread; then the
    thread count itself, 1024 blocks, and one block more"""
    _need_gpu()
    g = np.random.default_rng(8)
    p = (g.uniform(0, 1, (300000, 3)) * np.array([8.0, 8.0, 0.5])).astype(np.float32)
    for voxel, min_count in ((0.05, 1), (0.05, 3), (2.0 ** -12, 1)):
        want = VC.host(p, voxel, (0, 0, 0), min_count)
        assert len(want.points) > 20000
        VC.assert_same_cloud(_device(p, voxel, (0, 0, 0), min_count), want, (voxel, min_count))
    # 1024 blocks give every thread of the scan one count; 1025 give runs of two and leave half the block idle.  The scan is in place
    # and sees zeros: the second half of these clouds repeats the first, so no voxel opens there.
    for n_points in (262144, 262145):
        half = p[:(n_points + 1) // 2]
        twice = np.concatenate([half, half[:n_points - len(half)]])
        for min_count in (1, 3):
            want = VC.host(twice, 0.05, (0, 0, 0), min_count)
            heads = np.bincount(want.first_point // 256, minlength=(n_points + 255) // 256)
            assert len(heads) == (n_points + 255) // 256 and (heads[:400] > 0).all() and (heads[520:] == 0).all() and len(want.points) > 20000
            VC.assert_same_cloud(_device(twice, 0.05, (0, 0, 0), min_count), want, (n_points, min_count))


def test_two_runs_are_bit_equal():
    _need_gpu()
    p = cloud("many_cells")[0]
    n, c = VC.attributes("many_cells")
    a, b = _device(p, 0.075, (0.01, 0.02, 0.03), 1, n, c), _device(p, 0.075, (0.01, 0.02, 0.03), 1, n, c)
    VC.assert_same_cloud(a, b)
    VC.assert_same_cloud(a, VC.host(p, 0.075, (0.01, 0.02, 0.03), 1, n, c))


def test_refused_arguments():
    _need_gpu()
    p = torch.zeros(4, 3, device=DEV)
    for bad in (lambda: prep.voxel_downsample(p.double(), 1.0), lambda: prep.voxel_downsample(p, 0.0), lambda: prep.voxel_downsample(p, float("nan")),
                lambda: prep.voxel_downsample(p, 1e-39), lambda: prep.voxel_downsample(p, 1.0, min_count=0),
                lambda: prep.voxel_downsample(p, 1.0, normals=torch.zeros(4, 3)), lambda: prep.voxel_downsample(p, 1.0, colors=p),
                lambda: prep.voxel_downsample(p, 1.0, normals=torch.zeros(3, 3, device=DEV))):
        with pytest.raises(L.VlsatError):
            bad()
    out = prep.voxel_downsample(p, 1.0)
    assert out.count.tolist() == [4] and out.voxel_of_point.tolist() == [0, 0, 0, 0] and out.points.tolist() == [[0.0, 0.0, 0.0]]
    none = prep.voxel_downsample(p, 1.0, min_count=5, normals=p, colors=torch.zeros(4, 3, dtype=torch.uint8, device=DEV))
    assert none.points.shape == (0, 3) and none.normals.shape == (0, 3) and none.colors.shape == (0, 3) and none.count.shape == (0,)
    assert none.voxel_of_point.tolist() == [-1] * 4


def _same_dict(got, want, keys):
    for k in keys:
        if want[k] is None:
            assert got[k] is None, k
        elif np.asarray(want[k]).dtype.kind == "f":
            assert_bit_equal(got[k], want[k], k)
        else:
            assert np.array_equal(got[k], want[k]), k


def test_scan_downsample_and_segment_device_equal_host(tmp_path):
    _need_gpu()
    room = small_room()
    given = {"points": room["points"], "normals": room["normals"], "instances": room["instances"],
             "colors": (np.arange(len(room["points"]) * 3).reshape(-1, 3) % 251).astype(np.uint8)}
    fields = ("points", "normals", "colors", "instances", "voxel_of_point", "first_point", "voxel_count")
    _same_dict(scan.downsample_cloud(given, 0.25, (0.1, 0.0, -0.05), 2, device=DEV),
               scan.downsample_cloud(given, 0.25, (0.1, 0.0, -0.05), 2, device=None), fields)
    pts = np.concatenate([room["points"], room["points"][:700] + 0.003, [[np.nan, 0.0, 0.0]]])
    for cloud_ in ({"points": pts}, {"points": room["points"], "normals": room["normals"]}):
        host = scan.segment_cloud(cloud_, 0.3, k=12, device=None, voxel=0.1)
        dev = scan.segment_cloud(cloud_, 0.3, k=12, device=DEV, voxel=0.1)
        assert dev["n_segments"] == host["n_segments"] >= 4
        _same_dict(dev, host, ("instances", "normals", "curvature", "seg_size"))
        _same_dict(dev["resampled"], host["resampled"], fields + ("curvature", "seg_size"))


def test_faceless_ply_resampled_to_decoded_graph(tmp_path):
    """the 3-box room seen twice as a cloud: write_ply without faces -> segment_cloud(voxel=...) -> prepare_scan -> decode_graph ->
    to_annotation, on the device"""
    _need_gpu()
    from vlsat_amd import VLSATConfig, scene_graph as SG, synth
    from vlsat_amd.model import VLSATModel
    room = small_room()
    path = str(tmp_path / "cloud.ply")
    scan.write_ply(path, {"points": np.concatenate([room["points"], room["points"] + 0.002])})
    cloud_ = scan.segment_cloud(path, 0.3, k=12, device=DEV, voxel=0.1)
    assert np.array_equal(cloud_["instances"], scan.segment_cloud(path, 0.3, k=12, device=None, voxel=0.1)["instances"])
    s = cloud_["n_segments"]
    assert s >= 4 and len(cloud_["instances"]) == 2 * len(room["points"]) and (cloud_["instances"] > 0).all()
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
