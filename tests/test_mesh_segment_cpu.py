"""The mesh segmenter on the host (the rule is stated in include/vlsat_segment.h): the numpy restatement against answers typed in by
hand, its invariances, synth.make_box_mesh and what the rule makes of it, the mesh reader and writer, what the entry points
refuse without a device, and csrc/segment_core.h under ASan + UBSan in a stand-alone program against the restatement and the library."""
import math

import numpy as np
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import lib as L, prep, scan, synth

import segment_core_host
from mesh_segment_checks import (HAND_CASES, assert_same, box_room, check_hand_case, grid_mesh, hand_case, host_result, room_case,
                                 same_partition, shuffled_chain)


@pytest.mark.parametrize("name", list(HAND_CASES))
def test_host_gives_the_hand_answer(name):
    check_hand_case(prep.segment_mesh_host, name)


def test_cpu_tensors_take_the_host_route():
    n, e, w, mv, labels, sizes = hand_case("island_kept")
    got = prep.segment_mesh(n, e, w, mv)
    assert got.labels.tolist() == labels and got.seg_size.tolist() == sizes and list(got)[1] == 2


def test_mesh_edges_lists_the_three_sides_of_every_triangle():
    f = np.array([[0, 1, 2], [2, 1, 3]])
    want = [[0, 1], [1, 2], [2, 0], [2, 1], [1, 3], [3, 2]]
    assert prep.mesh_edges(f).tolist() == want and prep.mesh_edges(f).dtype == np.int32
    t = prep.mesh_edges(torch.from_numpy(f))
    assert t.tolist() == want and t.dtype == torch.int32
    with pytest.raises(L.VlsatError):
        prep.mesh_edges(np.zeros((2, 4), np.int32))


@pytest.mark.parametrize("key", [("grid", "random"), ("room", 0.05)])
def test_relabelled_vertices_give_the_same_partition(key):
    """(random normals: a tie between two neighbours goes to the lower ROOT, which a renumbering changes -- the axis grid is all ties)"""
    normals, edges, max_weight, min_verts = {"grid": grid_mesh, "room": room_case}[key[0]](*key[1:])
    want = host_result(key)
    v = normals.shape[0]
    perm = torch.from_numpy(np.random.default_rng(7).permutation(v))               # old vertex i becomes vertex perm[i]
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(v)
    shuffled = prep.segment_mesh_host(normals[inv], perm[edges.long()].to(torch.int32), max_weight, min_verts)
    assert shuffled.n_segments == want.n_segments
    assert sorted(shuffled.seg_size.tolist()) == sorted(want.seg_size.tolist())
    assert same_partition(shuffled.labels[perm].numpy(), want.labels.numpy())
    assert_same(prep.segment_mesh_host(normals, edges, max_weight, min_verts), want, "second run")


def test_axis_grid_takes_five_rounds_and_ties():
    normals, edges, max_weight, min_verts = grid_mesh("axes")
    assert prep.segment_rounds(min_verts) == 5 and max_weight == 0.0
    w = prep.segment_weights_host(normals.numpy(), edges[:, 0].numpy(), edges[:, 1].numpy())
    assert set(np.unique(w).tolist()) == {0.0, 1.0, 2.0}                          # exact: every absorb choice is a tie of many
    got = host_result(("grid", "axes"))
    assert got.n_segments >= 2 and int(got.seg_size.min()) >= min_verts and int(got.seg_size.sum()) == 64 * 64 == int((got.labels > 0).sum())


def test_chain_is_one_segment():
    got = host_result(("chain",))
    assert got.n_segments == 1 and got.seg_size.tolist() == [8192] and bool((got.labels == 1).all())


def test_box_mesh_layout():
    m = box_room()
    v = len(m["points"])
    assert 30000 <= v <= 60000 and m["faces"].dtype == np.int32 and m["faces"].min() == 0 and m["faces"].max() == v - 1
    assert m["plane"].shape == m["instances"].shape == (v,) and m["normals"].shape == (v, 3)
    assert np.allclose(np.linalg.norm(m["normals"], axis=1), 1.0)
    assert sorted(np.unique(m["instances"]).tolist()) == list(range(1, 10)) and int((m["plane"] == 0).sum()) == 201 * 201
    planes = np.unique(m["plane"][m["plane"] >= 0])
    assert planes.tolist() == list(range(0, 1 + 6 * 8)) and all(int((m["plane"] == p).sum()) >= 25 for p in planes)
    crease = m["plane"] < 0
    assert crease.any() and (m["instances"][crease] >= 2).all()
    # every triangle is wound along its vertices' normals, and an interior vertex's computed normal is its face's
    p, f = m["points"], m["faces"]
    cross = np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
    assert (np.einsum("ij,ij->i", cross, m["normals"][f[:, 0]]) > 0).all()
    vn = scan.vertex_normals(p, f)
    assert np.abs(vn[~crease] - m["normals"][~crease]).max() < 1e-9
    again = synth.make_box_mesh(8, 0.05, 3)
    assert all(np.array_equal(again[k], m[k]) for k in ("points", "normals", "faces", "plane", "instances"))
    noisy = box_room(0.05)
    assert np.array_equal(noisy["faces"], m["faces"]) and np.abs(noisy["normals"] - m["normals"]).max() > 0.05


def test_box_mesh_segments_are_planar_faces():
    m = box_room()
    got = host_result(("room", 0.0))
    labels, plane = got.labels.numpy(), m["plane"]
    assert (labels > 0).all() and got.n_segments >= 1 + 6 * 8
    for s in range(1, got.n_segments + 1):                                         # a segment: vertices of ONE planar face, plus crease vertices
        assert len(np.unique(plane[(labels == s) & (plane >= 0)])) <= 1, s
    for p in np.unique(plane[plane >= 0]):                                         # a face of >= min_verts interior vertices: ONE segment
        assert len(np.unique(labels[plane == p])) == 1, p
    assert int(got.seg_size[0]) == 201 * 201                                       # the floor: vertex 0 is its lowest


def test_vertex_normals_of_lonely_and_cancelling_vertices_are_zero():
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5]], dtype=np.float64)
    vn = scan.vertex_normals(pts, np.array([[0, 1, 2]]))
    assert vn[:3].tolist() == [[0, 0, 1]] * 3 and vn[3].tolist() == [0, 0, 0]
    assert scan.vertex_normals(pts, np.array([[0, 1, 2], [0, 2, 1]])).tolist() == [[0, 0, 0]] * 4
    with pytest.raises(scan.ScanError):
        scan.vertex_normals(pts, np.array([[0, 1, 4]]))


# ---- reader and writer -----------------------------------------------------------------------------------------------------------------
def test_read_mesh_returns_the_face_of_the_golden_scan():
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scan_small_ascii.ply")
    mesh, ref = scan.read_mesh(path), scan.read_ply(path)
    assert mesh["faces"].tolist() == [[0, 1, 2]] and mesh["faces"].dtype == np.int32
    assert all(np.array_equal(mesh[k], ref[k]) and mesh[k].dtype == ref[k].dtype for k in ref)
    binary = scan.read_mesh(path.replace("_ascii", ""))
    ref = scan.read_ply(path.replace("_ascii", ""))
    assert all(np.array_equal(binary[k], ref[k]) for k in ref) and binary["faces"].shape[1] == 3


@pytest.mark.parametrize("ascii", [False, True])
def test_write_ply_round_trips(tmp_path, ascii):
    g = np.random.default_rng(5)
    mesh = {"points": g.standard_normal((40, 3)), "normals": g.standard_normal((40, 3)), "instances": g.integers(0, 70000, 40),
            "faces": g.integers(0, 40, (25, 3)).astype(np.int32)}
    path = str(tmp_path / "m.ply")
    scan.write_ply(path, mesh, ascii=ascii)
    assert open(path, "rb").read(40).split(b"\n")[1] == (b"format ascii 1.0" if ascii else b"format binary_little_endian 1.0")
    back, plain = scan.read_mesh(path), scan.read_ply(path)
    for got in (back, plain):
        assert np.array_equal(got["points"], mesh["points"].astype(np.float32).astype(np.float64))
        assert np.array_equal(got["normals"], mesh["normals"].astype(np.float32).astype(np.float64))
        assert np.array_equal(got["instances"], mesh["instances"]) and got["colors"] is None
    assert np.array_equal(back["faces"], mesh["faces"])
    scan.write_ply(path, {"points": mesh["points"]}, ascii=ascii)                  # nothing but points: no normals, zero ids, no face element
    bare = scan.read_mesh(path)
    assert bare["normals"] is None and not bare["instances"].any() and bare["faces"].shape == (0, 3)


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian"])
def test_a_ply_without_labels_loads_with_zero_instances(tmp_path, fmt):
    path = str(tmp_path / "bare.ply")
    header = f"ply\nformat {fmt} 1.0\ncomment a reconstruction\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n" \
             "element face 2\nproperty list uchar int vertex_indices\nend_header\n"
    pts = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], dtype="<f4")
    with open(path, "wb") as f:
        f.write(header.encode())
        if fmt == "ascii":
            f.write(b"0 0 0\n1 0 0\n1 1 0\n0 1 0\n3 0 1 2\n3 0 2 3\n")
        else:
            f.write(pts.tobytes() + b"".join(bytes([3]) + np.array(t, dtype="<i4").tobytes() for t in ([0, 1, 2], [0, 2, 3])))
    mesh = scan.read_mesh(path)
    assert mesh["instances"].tolist() == [0, 0, 0, 0] and mesh["faces"].tolist() == [[0, 1, 2], [0, 2, 3]]
    assert np.array_equal(mesh["points"], pts.astype(np.float64)) and mesh["normals"] is None
    with pytest.raises(scan.ScanError, match="neither objectId nor label"):
        scan.read_ply(path)
    seg = scan.segment_scan(path, min_verts=2, device=None)                        # no normals in the file: computed; one flat square
    assert seg["instances"].tolist() == [1, 1, 1, 1] and seg["n_segments"] == 1 and seg["seg_size"].tolist() == [4]


def test_read_mesh_refuses_what_it_cannot_hold(tmp_path):
    path = str(tmp_path / "quad.ply")
    head = "ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\nelement face 1\n" \
           "property list uchar int vertex_indices\nend_header\n0 0 0\n1 0 0\n1 1 0\n0 1 0\n"
    open(path, "w").write(head + "4 0 1 2 3\n")
    with pytest.raises(scan.ScanError):
        scan.read_mesh(path)
    open(path, "w").write(head + "3 0 1 4\n")
    with pytest.raises(scan.ScanError, match="outside"):
        scan.read_mesh(path)


def test_segment_scan_on_the_host_fills_the_mesh_dict():
    m = box_room()
    out = scan.segment_scan(m, max_angle_deg=10.0, min_verts=20, device=None)
    want = host_result(("room", 0.0))
    assert out is not m and (m["instances"] <= 9).all()                            # a copy: the input keeps its own ids
    assert out["n_segments"] == want.n_segments and np.array_equal(out["instances"], want.labels.numpy()) and out["instances"].dtype == np.int64
    assert np.array_equal(out["seg_size"], want.seg_size.numpy())
    assert scan.scene_nodes(out["instances"], {i: "?" for i in range(1, out["n_segments"] + 1)}) == list(range(1, out["n_segments"] + 1))
    with pytest.raises(scan.ScanError):
        scan.segment_scan({"points": m["points"]}, device=None)


def test_refused_arguments():
    n, e = torch.zeros(4, 3), torch.zeros(2, 2, dtype=torch.int32)
    for bad in (lambda: prep.segment_mesh_host(torch.zeros(4, 2), e, 0.1), lambda: prep.segment_mesh_host(torch.zeros(0, 3), e, 0.1),
                lambda: prep.segment_mesh_host(n, torch.zeros(2, 3, dtype=torch.int32), 0.1), lambda: prep.segment_mesh_host(n, e, float("nan"))):
        with pytest.raises(L.VlsatError):
            bad()


# ---- the entry points without a device, the core under sanitizers --------------------------------------------------------------------
def test_segment_entry_points_refuse_what_is_out_of_range_without_a_device():
    lib = L.load()
    assert lib.vlsat_segment_mesh_scratch_bytes(0, 0) == 0 and lib.vlsat_segment_mesh_scratch_bytes((1 << 24) + 1, 0) == 0
    assert lib.vlsat_segment_mesh_scratch_bytes(10, -1) == 0 and lib.vlsat_segment_mesh_scratch_bytes(10, 1 << 31) == 0
    assert lib.vlsat_segment_mesh(0, 0, 0, 0, 0.1, 20, 0, 0, 0, 0, 0) != 0 and b"segment_mesh" in lib.vlsat_last_error()


def test_core_under_host_sanitizers_equals_the_restatement_and_the_library():
    rows = segment_core_host.run(sanitize=True)
    assert len(rows["w"]) > 5000 and len(rows["k"]) == 77 and len(rows["s"]) == 14
    bits = np.array([r[0] for r in rows["w"]], dtype=np.uint32)
    normals = bits.view(np.float32).reshape(-1, 3)                                 # rows 2 i and 2 i + 1 are the pair i
    idx = np.arange(len(rows["w"]))
    want = prep.segment_weights_host(normals, 2 * idx, 2 * idx + 1)
    assert want.view(np.uint32).tolist() == [r[1] for r in rows["w"]]
    assert {int(x) for x in want.view(np.uint32)} >= {0, 0x3f800000, 0x40000000}   # 0, 1 and 2 all occur
    for wbits, root, key in rows["k"]:
        assert key == (wbits << 32) | root
    for min_verts, rounds in rows["r"]:
        assert rounds == prep.segment_rounds(min_verts) == (0 if min_verts <= 1 else math.ceil(math.log2(min_verts))), min_verts
    lib = L.load()
    for v, nbytes in rows["s"]:
        assert lib.vlsat_segment_mesh_scratch_bytes(v, 3 * v) == nbytes and 24 * v <= nbytes <= 24 * v + 8 * (v // 1024 + 2) + 7 * 16
    assert rows == segment_core_host.run(sanitize=False)
