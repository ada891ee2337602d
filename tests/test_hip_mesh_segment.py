"""The mesh segmenter on the GPU (csrc/mesh_segment.hip via vlsat_segment_mesh): labels, count and sizes EQUAL to the host
restatement -- the hand-made meshes with their typed-in answers, a shuffled chain (path halving under contention), a grid whose weights
tie exactly (five rounds), random normals, a box room of 54 thousand vertices with and without noise (many blocks, the multi-block
numbering, the hot floor root), trim=False, two runs bit-equal, refused arguments, and the whole route from a bare mesh to a decoded graph."""
import numpy as np
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import lib as L, prep, scan

from mesh_segment_checks import HAND_CASES, assert_same, box_room, check_hand_case, grid_mesh, hand_case, host_result, room_case, shuffled_chain

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path cannot run and there is no fallback")


def _device(case, trim=True):
    normals, edges, max_weight, min_verts = case
    return prep.segment_mesh(normals.to(DEV), edges.to(DEV), max_weight, min_verts, trim=trim)


@pytest.mark.parametrize("name", list(HAND_CASES))
def test_hand_cases(name):
    _need_gpu()
    check_hand_case(prep.segment_mesh, name, DEV)
    assert_same(_device(hand_case(name)[:4]), prep.segment_mesh_host(*hand_case(name)[:4]), name)


def test_shuffled_chain_is_one_segment():
    _need_gpu()
    got = _device(shuffled_chain())
    assert got.n_segments == 1 and got.seg_size.tolist() == [8192]
    assert_same(got, host_result(("chain",)))


@pytest.mark.parametrize("kind", ["axes", "random"])
def test_grid_rounds_and_ties(kind):
    _need_gpu()
    case = grid_mesh(kind)
    assert prep.segment_rounds(case[3]) == 5
    want = host_result(("grid", kind))
    assert want.n_segments >= 2 and int(want.seg_size.min()) >= 20
    assert_same(_device(case), want, kind)


@pytest.mark.parametrize("noise", [0.0, 0.05])
def test_box_room(noise):
    _need_gpu()
    case = room_case(noise)
    assert 30000 <= case[0].shape[0] <= 60000
    want = host_result(("room", noise))
    got = _device(case)
    assert_same(got, want, f"noise {noise}")
    assert int(got.seg_size[0]) >= 40000 and got.n_segments >= 49                 # the floor is segment 1; past 1024 vertices: many tiles
    assert_same(_device(case), got, "second run")                                 # repeatability: bit-equal


def test_untrimmed_reads_nothing_back_and_equals_trimmed():
    _need_gpu()
    case = room_case(0.05)
    full = _device(case, trim=False)
    assert not full.trimmed and full.n_segments.is_cuda and full.n_segments.shape == (1,) and full.seg_size.shape == full.labels.shape
    want = host_result(("room", 0.05))
    assert_same(full, prep.segment_mesh_host(*case, trim=False))
    cut = full.trim()
    assert_same(cut, want)
    assert not bool(full.seg_size[cut.n_segments:].any())


def test_refused_arguments():
    _need_gpu()
    n, e = torch.zeros(4, 3, device=DEV), torch.zeros(2, 2, dtype=torch.int32, device=DEV)
    with pytest.raises(L.VlsatError):
        prep.segment_mesh(n.double(), e, 0.1)
    with pytest.raises(L.VlsatError):
        prep.segment_mesh(n, e, float("nan"))
    lib = L.load()
    out = torch.zeros(8, dtype=torch.int32, device=DEV)
    scratch = torch.empty(int(lib.vlsat_segment_mesh_scratch_bytes(4, 2)), dtype=torch.uint8, device=DEV)
    args = lambda **k: [k.get("normals", n.data_ptr()), k.get("edges", e.data_ptr()), k.get("v", 4), k.get("m", 2), k.get("w", 0.1), 20,
                        k.get("scratch", scratch.data_ptr()), out.data_ptr(), out.data_ptr(), out.data_ptr(), L.stream_ptr()]
    for bad in (dict(normals=0), dict(edges=0), dict(scratch=0), dict(v=0), dict(v=(1 << 24) + 1), dict(m=-1), dict(m=1 << 31), dict(w=float("nan"))):
        assert lib.vlsat_segment_mesh(*args(**bad)) != 0, bad
        assert b"segment_mesh" in lib.vlsat_last_error()
    assert lib.vlsat_segment_mesh(*args(edges=0, m=0)) == 0                        # no edge: the list may be null


def test_bare_mesh_to_decoded_graph(tmp_path):
    """an 8-box room: write_ply -> segment_scan -> prepare_scan -> decode_graph; transfer_labels against the generating boxes"""
    _need_gpu()
    from vlsat_amd import VLSATConfig, scene_graph as SG, synth
    from vlsat_amd.model import VLSATModel
    room = box_room()
    path = str(tmp_path / "room.ply")
    scan.write_ply(path, {k: room[k] for k in ("points", "normals", "faces")})    # a bare mesh: no ids
    mesh = scan.segment_scan(path, max_angle_deg=10.0, min_verts=20, device=DEV)
    want = host_result(("room", 0.0))
    s = mesh["n_segments"]
    assert s == want.n_segments and np.array_equal(mesh["instances"], want.labels.numpy()) and np.array_equal(mesh["seg_size"], want.seg_size.numpy())
    cfg = VLSATConfig(N_LAYERS=1)
    relations = [f"r{k}" for k in range(cfg.num_rel_class)]
    b = scan.prepare_scan(mesh, {i: "?" for i in range(1, s + 1)}, ["?"], [], relations, num_points=32, seed=0, device=DEV)
    sampled = [i + 1 for i, c in enumerate(mesh["seg_size"].tolist()) if c > 0]
    assert b["instance_ids"] == sampled == list(range(1, s + 1)) and b["points_per_instance"].tolist() == mesh["seg_size"].tolist()
    m = VLSATModel(cfg, DEV).load_state(synth.make_weights(cfg)).eval()
    g3d, none = m.decode_graph(b["obj_points"], None, b["edge_indices"].t().contiguous(), b["descriptor"], threshold=0.5, n_labels=3, max_rel=256)
    assert none is None and g3d.labels.shape == (s, 3)                           # the graph's nodes are exactly the segments
    classes = [f"c{k}" for k in range(cfg.num_obj_class)]
    entry = SG.to_annotation(g3d, 0, b["edge_indices"], b["instance_ids"], classes, ["none"] + relations, "room")
    assert set(entry["objects"]) == {str(i) for i in range(1, s + 1)}
    out = tmp_path / "relationships_predicted.json"
    SG.write_annotations(out, [entry])
    rel, objs, scans = scan.read_relationships(str(out), ["room"])
    assert scans == ["room_0"] and rel["room_0"] == entry["relationships"] and sorted(objs["room_0"]) == list(range(1, s + 1))
    gt = {"points": room["points"], "instances": room["instances"]}
    match = scan.transfer_labels(mesh, gt, {i: f"box{i}" for i in range(1, 10)}, max_sq_dist=0.01, min_seg_size=100, device=DEV)
    assert match.counts.shape == (s, 9) and int(match.counts.sum()) == len(room["points"]) and match.n_without_correspondence == 0
    assert match.segment_to_gt[1] == 1 and len(match.gt_to_segments) >= 2         # the floor, and some box faces above 100 vertices
