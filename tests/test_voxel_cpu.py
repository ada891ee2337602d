"""The voxel-grid filter on the host (the rule is stated in include/vlsat_voxel.h): the numpy restatement against an independent brute
force, csrc/voxel_core.h through g++ (with ASan + UBSan in the stand-alone program) against the restatement bit for bit, the refused
arguments of the C entry points, the permutation property, scan.downsample_cloud through write_ply / read_mesh, scan.segment_cloud
with and without `voxel`, and the density case (the header's symbols: test_c_abi_cpu.py).  Every comparison is of bits:
nothing here has a tolerance."""
import ctypes

import numpy as np
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import lib as L, prep, scan, synth

import voxel_checks as VC
import voxel_core_host
from cloud_checks import assert_bit_equal, cloud, small_room


# ---- the restatement against the brute force --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", VC.SIZES)
@pytest.mark.parametrize("name", VC.NAMES)
def test_restatement_equals_the_brute_force(name, size):
    p = cloud(name)[0]
    voxel, origin = VC.setting(name, size)
    n, c = VC.attributes(name)
    for min_count in (1, 2, 10 ** 6):
        want = VC.brute_voxels(p, voxel, origin, min_count, n, c)
        VC.assert_same_cloud(VC.host(p, voxel, origin, min_count, n, c), want[:6], (name, size, min_count))
    assert VC.host_case(name, size).normals is None and VC.host_case(name, size).colors is None
    VC.assert_same_cloud(VC.host_case(name, size), VC.brute_voxels(p, voxel, origin)[:6], (name, size, "bare"))


@pytest.mark.parametrize("name", VC.SPECIAL)
def test_restatement_equals_the_brute_force_on_the_further_settings(name):
    VC.assert_same_cloud(VC.host_special(name), VC.brute_voxels(*VC.special(name))[:6], name)


def test_the_cases_cover_what_they_claim():
    for name in VC.NAMES:
        valid = int((np.abs(cloud(name)[0]) < 32768).all(1).sum())
        one, each, mid = (VC.host_case(name, s) for s in VC.SIZES)
        assert len(one.points) == 1 and one.count.tolist() == [valid], name         # every atomic hits one destination
        assert (one.voxel_of_point >= 0).sum() == valid
        assert each.count.max() <= 3 and len(each.points) >= valid // 3, name       # a voxel per point (coincident points share one)
        assert len(each.points) >= len(mid.points) >= 1
    assert VC.host_case("v257", "each").count.max() == 1 and VC.host_case("duplicates", "each").count.tolist() == [3] * 300
    assert 700 <= len(VC.host_case("many_cells", "between").points) <= 1300         # about a thousand voxels
    assert (VC.host_case("nonfinite", "between").voxel_of_point == -1).sum() == 72
    assert len(VC.host_case("many_cells", "between", 10 ** 6).points) == 0          # min_count above every count: M = 0
    out = VC.host_special("out_of_range")
    assert 0 < len(out.points) < 400 and (out.voxel_of_point == -1).sum() > 300     # cells beyond 2^20 with a tiny voxel
    assert (out.voxel_of_point[::7] == -1).all() and (out.voxel_of_point[1::7] == -1).all()
    cancel = VC.host_special("cancel")
    zero = (cancel.normals == 0).all(1)
    assert zero.all() and cancel.count.tolist() == [2] * 150                        # opposite normals, and NaN ones, give (0, 0, 0)
    both = VC.host_special("faces_and_signs")
    p = VC.special("faces_and_signs")[0]
    assert (p < 0).any() and (p > 0).any() and ((p * 8) == np.round(p * 8)).all(1).sum() >= 480
    assert len(both.points) > 300 and both.first_point.tolist() == sorted(both.first_point.tolist())
    assert VC.host_special("v65").count.tolist() == [1] * 65 and VC.host_special("v257_pairs").voxel_of_point[-1] == -1
    n, _ = VC.attributes("density")
    assert not np.isfinite(n).all() and (np.abs(n) >= 32768).any()


def test_numbering_means_and_map_properties():
    p = cloud("many_cells")[0]
    n, c = VC.attributes("many_cells")
    got = VC.host_case("many_cells", "between", 1, True)
    of = got.voxel_of_point
    assert got.points.dtype == np.float32 and got.normals.dtype == np.float32 and got.colors.dtype == np.uint8
    assert of.dtype == got.first_point.dtype == got.count.dtype == np.int32
    assert (np.diff(got.first_point) > 0).all() and (of[got.first_point] == np.arange(len(got.points))).all()
    assert np.array_equal(np.bincount(of, minlength=len(got.points)), got.count)
    first_seen = np.full(len(got.points), len(p))
    np.minimum.at(first_seen, of, np.arange(len(p)))
    assert np.array_equal(first_seen, got.first_point)
    for m in (0, 17, len(got.points) - 1):
        member = p[of == m].astype(np.float64)
        assert np.abs(member.mean(0) - got.points[m]).max() < 1e-6                   # a plausibility check beside the exact ones above
        assert np.abs(got.points[m] - member.mean(0)).max() <= np.ptp(member, axis=0).max() + 1e-6
    length = np.linalg.norm(got.normals.astype(np.float64), axis=1)
    assert ((np.abs(length - 1) < 1e-6) | (length == 0)).all()
    two = VC.host_case("many_cells", "between", 2, True)
    keep = got.count >= 2
    assert_bit_equal(two.points, got.points[keep])                                   # a dropped voxel changes nobody else's mean
    assert_bit_equal(two.first_point, got.first_point[keep])
    assert ((two.voxel_of_point >= 0) == keep[of]).all()


def test_permutation_gives_the_same_voxels_numbered_by_the_new_first_points():
    p = cloud("density")[0]
    n, c = VC.attributes("density")
    voxel, origin = VC.setting("density", "between")
    a = VC.host(p, voxel, origin, 1, n, c)
    perm = np.random.default_rng(5).permutation(len(p))
    b = VC.host(p[perm], voxel, origin, 1, n[perm], c[perm])
    key_a, _ = prep.voxel_keys_host(p, voxel, origin)
    key_b, _ = prep.voxel_keys_host(p[perm], voxel, origin)

    def rows(v, key):
        return {(int(key[f]), v.points[m].tobytes(), v.normals[m].tobytes(), v.colors[m].tobytes(), int(v.count[m]))
                for m, f in enumerate(v.first_point)}
    assert rows(a, key_a) == rows(b, key_b) and len(rows(a, key_a)) == len(a.points)
    assert (np.diff(b.first_point) > 0).all()
    # the voxel of input point perm[j] is the same cell, under its new number
    assert np.array_equal(key_a[a.first_point][a.voxel_of_point[perm]], key_b[b.first_point][b.voxel_of_point])


def test_two_clouds_in_one_frame_share_cells():
    p = cloud("many_cells")[0]
    a, _ = prep.voxel_keys_host(p[:1500], 0.075)
    b, _ = prep.voxel_keys_host(p[1500:], 0.075)
    whole, _ = prep.voxel_keys_host(p, 0.075)
    assert np.array_equal(np.concatenate([a, b]), whole) and len(np.intersect1d(a, b)) > 100


def test_cpu_tensors_take_the_host_route():
    p = cloud("v257")[0]
    n, c = VC.attributes("v257")
    got = prep.voxel_downsample(torch.from_numpy(p.copy()), 0.25, normals=torch.from_numpy(n.copy()), colors=torch.from_numpy(c.copy()))
    assert isinstance(got, prep.VoxelCloud) and all(torch.is_tensor(x) and not x.is_cuda for x in got)
    VC.assert_same_cloud([x.numpy() for x in got], VC.host(p, 0.25, (0, 0, 0), 1, n, c))
    bare = prep.voxel_downsample(p, 0.25)
    assert bare.normals is None and bare.colors is None
    assert_bit_equal(bare.points.numpy(), got.points.numpy())


# ---- voxel_core.h through g++ against the restatement ------------------------------------------------------------------------------------
def test_core_equals_the_restatement():
    rows = voxel_core_host.run(sanitize=True)
    assert len(rows["k"]) > 1000 and len(rows["q"]) > 300 and len(rows["m"]) == len(rows["n"]) == len(rows["c"]) == 300
    out_of_range = 0
    groups = {}
    for bits, key in rows["k"]:
        groups.setdefault(bits[3:], []).append((bits[:3], key))
    for (ox, oy, oz, voxel), members in groups.items():
        f = lambda *u: np.array(u, dtype=np.uint32).view(np.float32)        # noqa: E731
        pts = np.array([m[0] for m in members], dtype=np.uint32).view(np.float32).reshape(-1, 3)
        keys, ok = prep.voxel_keys_host(pts, f(voxel)[0], tuple(f(ox, oy, oz)))
        assert [int(k) for k in keys] == [m[1] for m in members]
        out_of_range += int((~ok).sum())
    assert out_of_range >= 45 and len(groups) == 15
    x = np.array([r[0] for r in rows["q"]], dtype=np.uint32).view(np.float32)
    assert np.rint(x.astype(np.float64) * 2.0 ** 24).astype(np.int64).tolist() == [r[1] for r in rows["q"]]
    assert np.rint(x.astype(np.float64) * 2.0 ** 20).astype(np.int64).tolist() == [r[2] for r in rows["q"]]
    s, n = (np.array([r[k] for r in rows["m"]], dtype=np.int64) for k in (0, 1))
    mean = (s.astype(np.float64) / n.astype(np.float64) * 2.0 ** -24).astype(np.float32)
    assert mean.view(np.uint32).tolist() == [r[2] for r in rows["m"]]
    v = np.array([r[0] for r in rows["n"]], dtype=np.int64).astype(np.float64)
    length = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    assert (length > 0).all()
    assert (v / length[:, None]).astype(np.float32).view(np.uint32).tolist() == [list(r[1]) for r in rows["n"]]
    cs, cn = (np.array([r[k] for r in rows["c"]], dtype=np.int64) for k in (0, 1))
    assert ((2 * cs + cn) // (2 * cn)).tolist() == [r[2] for r in rows["c"]] and max(r[2] for r in rows["c"]) <= 255
    assert rows == voxel_core_host.run(sanitize=False)


# ---- refused arguments --------------------------------------------------------------------------------------------------------------------
def test_refused_arguments_of_the_python_layer():
    p = np.zeros((4, 3), np.float32)
    for bad in (lambda: prep.voxel_downsample_host(p, 0.0), lambda: prep.voxel_downsample_host(p, -1.0),
                lambda: prep.voxel_downsample_host(p, float("nan")), lambda: prep.voxel_downsample_host(p, float("inf")),
                lambda: prep.voxel_downsample_host(p, 1e-39), lambda: prep.voxel_downsample_host(np.zeros((0, 3), np.float32), 1.0),
                lambda: prep.voxel_downsample_host(p, 1.0, min_count=0), lambda: prep.voxel_downsample_host(p, 1.0, origin=(0.0, 0.0)),
                lambda: prep.voxel_downsample_host(p, 1.0, origin=(0.0, float("nan"), 0.0)),
                lambda: prep.voxel_downsample_host(p, 1.0, normals=np.zeros((3, 3), np.float32)),
                lambda: prep.voxel_downsample_host(p, 1.0, colors=np.zeros((5, 3), np.uint8))):
        with pytest.raises(L.VlsatError):
            bad()
    with pytest.raises(scan.ScanError):
        scan.downsample_cloud({"points": p}, 0.0, device=None)
    with pytest.raises(scan.ScanError):
        scan.downsample_cloud({"points": np.zeros((0, 3))}, 1.0, device=None)


def test_refused_arguments_of_the_c_entry_points():
    """every limit is checked before anything is launched, so the refusals need no device: the pointers are never followed"""
    lib = L.load()
    assert lib.vlsat_voxel_scratch_bytes(0) == 0 and lib.vlsat_voxel_scratch_bytes((1 << 24) + 1) == 0 and lib.vlsat_voxel_scratch_bytes(-1) == 0
    assert lib.vlsat_voxel_scratch_bytes(1) > 0
    big = lib.vlsat_voxel_scratch_bytes(1 << 24)
    assert (16 << 25) + (8 + 60) * (1 << 24) <= big <= (16 << 25) + (8 + 60) * (1 << 24) + (1 << 20)
    buf = (ctypes.c_char * 4096)()
    ptr = ctypes.addressof(buf)
    assign = lambda **k: lib.vlsat_voxel_assign(k.get("points", ptr), k.get("v", 4), k.get("voxel", 1.0), 0.0, k.get("oy", 0.0), 0.0,   # noqa: E731
                                                k.get("min_count", 1), k.get("scratch", ptr), k.get("of", ptr), k.get("first", ptr),
                                                k.get("count", ptr), k.get("n", ptr), None)
    for bad in (dict(voxel=0.0), dict(voxel=-0.5), dict(voxel=float("nan")), dict(voxel=float("inf")), dict(voxel=1e-39), dict(v=0),
                dict(v=(1 << 24) + 1), dict(min_count=0), dict(min_count=-3), dict(points=None), dict(scratch=None), dict(of=None),
                dict(first=None), dict(count=None), dict(n=None), dict(oy=float("nan"))):
        assert assign(**bad) == -1, bad
        assert b"voxel" in lib.vlsat_last_error(), bad
    reduce = lambda **k: lib.vlsat_voxel_reduce(k.get("points", ptr), k.get("normals", None), k.get("colors", None), k.get("of", ptr),   # noqa: E731
                                                k.get("count", ptr), k.get("v", 4), k.get("m", 2), k.get("scratch", ptr),
                                                k.get("out", ptr), k.get("out_normals", None), k.get("out_colors", None), None)
    for bad in (dict(v=0), dict(v=(1 << 24) + 1), dict(m=-1), dict(m=5), dict(points=None), dict(of=None), dict(count=None),
                dict(scratch=None), dict(out=None), dict(normals=ptr), dict(colors=ptr)):
        assert reduce(**bad) == -1, bad
        assert b"voxel" in lib.vlsat_last_error(), bad
    assert reduce(m=0, out=None) == 0                                               # no voxel: nothing to launch, nothing to refuse


# ---- scan ---------------------------------------------------------------------------------------------------------------------------------
def test_downsample_cloud_round_trips_through_ply(tmp_path):
    room = small_room()
    given = {"points": room["points"], "normals": room["normals"], "instances": room["instances"], "faces": room["faces"],
             "colors": (np.arange(len(room["points"]) * 3).reshape(-1, 3) % 251).astype(np.uint8), "plane": room["plane"]}
    out = scan.downsample_cloud(given, 0.25, device=None)
    want = VC.host(room["points"].astype(np.float32), 0.25, (0, 0, 0), 1, room["normals"].astype(np.float32), given["colors"])
    m = len(want.points)
    assert 50 < m < len(room["points"]) // 3 and out["faces"].shape == (0, 3)
    assert out["points"].dtype == np.float64 and np.array_equal(out["points"], want.points.astype(np.float64))
    assert np.array_equal(out["normals"], want.normals.astype(np.float64)) and np.array_equal(out["colors"], want.colors)
    assert np.array_equal(out["voxel_of_point"], want.voxel_of_point) and np.array_equal(out["voxel_count"], want.count)
    assert np.array_equal(out["first_point"], want.first_point)
    assert np.array_equal(out["instances"], room["instances"][want.first_point])     # integer fields: the value at the first point
    assert np.array_equal(out["plane"], room["plane"][want.first_point])
    path = str(tmp_path / "small.ply")
    scan.write_ply(path, out)
    back = scan.read_mesh(path)
    assert np.array_equal(back["points"], out["points"]) and np.array_equal(back["normals"], out["normals"])
    assert np.array_equal(back["instances"], out["instances"]) and back["faces"].shape == (0, 3)
    again = scan.downsample_cloud(path, 0.25, device=None)                            # a resampled cloud resampled on its own grid
    assert len(again["points"]) <= m and int(again["voxel_count"].sum()) == m
    bare = scan.downsample_cloud({"points": room["points"]}, 0.25, origin=(0.1, 0.0, -0.05), min_count=3, device=None)
    assert bare["normals"] is None and bare["colors"] is None and (bare["instances"] == 0).all() and (bare["voxel_count"] >= 3).all()
    assert (bare["voxel_of_point"] == -1).any()


def _stages(points, radius, k):
    """what scan.segment_cloud does without `voxel`, stage by stage"""
    p = np.ascontiguousarray(points, dtype=np.float32)
    t = prep.knn_points_host(p, k, float(np.float32(radius) ** 2))
    n, c = prep.cloud_normals_host(p, t.index, t.count, 5)
    masked = np.where((c > np.float32(0.02))[:, None], np.float32(0), n)
    seg = prep.segment_mesh_host(masked, prep.knn_edges(t.index), float(np.float32(1.0 - np.cos(np.radians(10.0)))), 20, unsigned=True)
    return n, c, seg


def test_segment_cloud_without_voxel_is_what_it_was():
    room = small_room()
    n, c, seg = _stages(room["points"], 0.15, 12)
    for out in (scan.segment_cloud({"points": room["points"]}, 0.15, k=12, device=None),
                scan.segment_cloud({"points": room["points"]}, 0.15, k=12, device=None, voxel=None)):
        assert "resampled" not in out and out["n_segments"] == seg.n_segments >= 4
        assert np.array_equal(out["instances"], seg.labels.numpy().astype(np.int64)) and np.array_equal(out["seg_size"], seg.seg_size.numpy())
        assert_bit_equal(out["normals"], n.astype(np.float64))
        assert_bit_equal(out["curvature"], c)


def test_segment_cloud_with_voxel_returns_the_input_cloud():
    room = small_room()
    pts = np.concatenate([room["points"], room["points"][:700] + 0.003, [[np.nan, 0.0, 0.0], [1e6, 0.0, 0.0]]])
    out = scan.segment_cloud({"points": pts, "plane": np.arange(len(pts))}, 0.3, k=12, device=None, voxel=0.1)
    small = out["resampled"]
    of = small["voxel_of_point"]
    assert len(out["points"]) == len(pts) and of.shape == (len(pts),) and of[-2:].tolist() == [-1, -1] and (of[:-2] >= 0).all()
    want = scan.segment_cloud(scan.downsample_cloud({"points": pts, "plane": np.arange(len(pts))}, 0.1, device=None), 0.3, k=12, device=None)
    assert np.array_equal(small["instances"], want["instances"]) and small["n_segments"] == want["n_segments"] == out["n_segments"] >= 4
    assert np.array_equal(small["plane"], small["first_point"])
    assert np.array_equal(out["instances"][:-2], want["instances"][of[:-2]]) and out["instances"][-2:].tolist() == [0, 0]
    assert_bit_equal(out["normals"][:-2], want["normals"][of[:-2]])
    assert (out["normals"][-2:] == 0).all() and np.isinf(out["curvature"][-2:]).all() and out["curvature"].dtype == np.float32
    assert_bit_equal(out["curvature"][:-2], want["curvature"][of[:-2]])
    assert out["seg_size"].dtype == np.int32 and len(out["seg_size"]) == out["n_segments"]
    assert np.array_equal(out["seg_size"], np.bincount(out["instances"], minlength=out["n_segments"] + 1)[1:])
    assert out["seg_size"].sum() > want["seg_size"].sum()                            # recounted over the input points
    carried = scan.segment_cloud({"points": room["points"], "normals": room["normals"]}, 0.3, k=12, device=None, voxel=0.1)
    averaged = VC.host(room["points"].astype(np.float32), 0.1, (0, 0, 0), 1, room["normals"].astype(np.float32)).normals
    assert np.array_equal(carried["resampled"]["normals"], averaged.astype(np.float64))   # the input's normals, averaged and kept


@pytest.mark.parametrize("step", [0.1])
def test_resampling_a_fused_cloud_restores_the_uniform_segmentation(step):
    """the density case: a room sampled at `step`, then every point jittered and the half x < 5 seen eight more times with more
    noise.  Resampled on a grid of edge `step` the fused cloud drops no point and has at most 1.25 times the segments of the uniform
    room.  (The raw fused cloud is not run here: its restated neighbour search takes minutes; README.md quotes a one-off run.)"""
    uniform, fused = VC.fused_room(step)
    assert len(fused) > 4 * len(uniform)
    base = scan.segment_cloud({"points": uniform}, 3 * step, k=16, device=None)
    out = scan.segment_cloud({"points": fused}, 3 * step, k=16, device=None, voxel=step)
    print("uniform", len(uniform), base["n_segments"], "fused", len(fused), "resampled", len(out["resampled"]["points"]), out["n_segments"],
          "dropped", int((out["instances"] == 0).sum()))
    assert (out["instances"] > 0).all() and (out["resampled"]["instances"] > 0).all()
    assert out["n_segments"] <= 1.25 * base["n_segments"]
