"""Shared by test_mesh_segment_cpu.py and test_hip_mesh_segment.py: the hand-made meshes of the mesh segmenter with their answers typed in
(the rule is stated in include/vlsat_segment.h), the larger generated cases, and the comparison of two results."""
import functools
import math

import numpy as np
import torch

X, Y, Z = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
NAN = (float("nan"), 0.0, 0.0)


def _xz(deg):
    return (math.cos(math.radians(deg)), 0.0, math.sin(math.radians(deg)))


def _path(n):
    return [(i, i + 1) for i in range(n - 1)]


def _grid_faces(rows, cols):
    """two triangles per cell of a rows x cols vertex grid (vertex r * cols + c): sides, and the diagonal (r, c) - (r + 1, c + 1)"""
    f = []
    for r in range(rows - 1):
        for c in range(cols - 1):
            a = r * cols + c
            f += [(a, a + cols, a + cols + 1), (a, a + cols + 1, a + 1)]
    return np.asarray(f, dtype=np.int32)


def faces_to_edges(faces):
    return np.asarray(faces, dtype=np.int32)[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2)


_ISLAND = [Z] * 16
for _v in (5, 6, 9):
    _ISLAND[_v] = X
_ISLAND_EDGES = faces_to_edges(_grid_faces(4, 4)).tolist()

# name -> (normals, edges, max_weight, min_verts, labels, seg_size); every answer worked out by hand from the rule
HAND_CASES = {
    # two planes (z: vertices 0-2, y: 4-6) and a crease vertex 3 between them.  w(3, z side) = 1 - 0.8, w(3, y side) = 1 - 0.6: to z
    "crease_to_lower_weight": ([Z, Z, Z, (0.0, 0.6, 0.8), Y, Y, Y], _path(7), 0.1, 2, [1, 1, 1, 1, 2, 2, 2], [4, 3]),
    # ... the lower weight on the side of the HIGHER root: the weight decides before the root does
    "crease_to_lower_weight_higher_root": ([Z, Z, Z, (0.0, 0.8, 0.6), Y, Y, Y], _path(7), 0.1, 2, [1, 1, 1, 2, 2, 2, 2], [3, 4]),
    # (0, 0.5, 0.5): both weights are exactly 0.5 -> the lower root, which is the z side (root 0)
    "crease_exact_tie_to_lower_root": ([Z, Z, Z, (0.0, 0.5, 0.5), Y, Y, Y], _path(7), 0.1, 2, [1, 1, 1, 1, 2, 2, 2], [4, 3]),
    # the same tie with the crease as vertex 0 and the edge to the higher root listed FIRST: still root 1 (the y side), not root 4
    "crease_exact_tie_edge_order": ([(0.0, 0.5, 0.5), Y, Y, Y, Z, Z, Z], [(0, 4), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6)], 0.1, 2,
                                    [1, 1, 1, 1, 2, 2, 2], [4, 3]),
    # a 4 x 4 grid mesh facing z with the island {5, 6, 9} facing x: three vertices, absorbed when min_verts = 4 ...
    "island_absorbed": (_ISLAND, _ISLAND_EDGES, 0.1, 4, [1] * 16, [16]),
    # ... and a segment of its own when min_verts = 3
    "island_kept": (_ISLAND, _ISLAND_EDGES, 0.1, 3, [1, 1, 1, 1, 1, 2, 2, 1, 1, 2, 1, 1, 1, 1, 1, 1], [13, 3]),
    # four single vertices in a row at 0, 40, 100, 140 degrees: weights 0.23, 0.5, 0.23.  Round 1 pairs {0,1} and {2,3}, still below
    # min_verts = 4; round 2 joins the pairs.  One round alone would leave two pieces of 2, which step 4 would drop.
    "chain_needs_two_rounds": ([_xz(0), _xz(40), _xz(100), _xz(140)], _path(4), 0.1, 4, [1, 1, 1, 1], [4]),
    # {5, 6} are linked to each other and to nobody else, 7 has no edge at all: islands below min_verts get id 0
    "isolated_small_component": ([Z] * 8, _path(5) + [(5, 6)], 0.1, 3, [1, 1, 1, 1, 1, 0, 0, 0], [5]),
    # crease_to_lower_weight plus duplicate, reversed, degenerate (a == b) and out-of-range edges: the same answer
    "junk_edges_change_nothing": ([Z, Z, Z, (0.0, 0.6, 0.8), Y, Y, Y],
                                  [(-1, 3), (3, 7)] + _path(7) + [(1, 0), (0, 1), (2, 2), (100, 0), (3, 2), (4, 3), (0, -5), (6, 6)], 0.1, 2,
                                  [1, 1, 1, 1, 2, 2, 2], [4, 3]),
    # three interleaved components: ids follow the lowest vertex of each
    "ids_in_order_of_lowest_vertex": ([Z, X, Y] * 3, [(0, 3), (3, 6), (1, 4), (4, 7), (2, 5), (5, 8), (0, 1), (1, 2), (7, 8)], 0.1, 3,
                                      [1, 2, 3, 1, 2, 3, 1, 2, 3], [3, 3, 3]),
    # {0, 1} linked, 2 hangs on 1 at a right angle, 3 has no edge.  min_verts 0 and 1: no round, nothing dropped
    "min_verts_0": ([Z, Z, X, Z], [(0, 1), (1, 2)], 0.1, 0, [1, 1, 2, 3], [2, 1, 1]),
    "min_verts_1": ([Z, Z, X, Z], [(0, 1), (1, 2)], 0.1, 1, [1, 1, 2, 3], [2, 1, 1]),
    # min_verts 2: one round absorbs 2, and 3 is an island
    "min_verts_2": ([Z, Z, X, Z], [(0, 1), (1, 2)], 0.1, 2, [1, 1, 1, 0], [3]),
    # a NaN normal weighs 2 on every edge: it cuts the path ...
    "nan_normal_cuts": ([Z, Z, NAN, Z, Z], _path(5), 0.1, 1, [1, 1, 2, 3, 3], [2, 1, 2]),
    # ... and when absorbed, both of its edges tie at 2: the lower root
    "nan_normal_absorbed": ([Z, Z, NAN, Z, Z], _path(5), 0.1, 2, [1, 1, 1, 2, 2], [3, 2]),
    # no edge at all: every vertex is an island
    "no_edges_all_dropped": ([Z] * 5, [], 0.1, 2, [0] * 5, []),
    "no_edges_all_kept": ([Z] * 5, [], 0.1, 1, [1, 2, 3, 4, 5], [1] * 5),
}


def hand_case(name):
    normals, edges, max_weight, min_verts, labels, sizes = HAND_CASES[name]
    return (torch.tensor(normals, dtype=torch.float32).reshape(-1, 3), torch.tensor(edges, dtype=torch.int32).reshape(-1, 2), max_weight,
            min_verts, labels, sizes)


def check_hand_case(fn, name, device=None):
    """``fn``: prep.segment_mesh or prep.segment_mesh_host"""
    normals, edges, max_weight, min_verts, labels, sizes = hand_case(name)
    assert normals.shape[0] <= 64
    if device is not None:
        normals, edges = normals.to(device), edges.to(device)
    got = fn(normals, edges, max_weight, min_verts)
    assert got.labels.dtype == torch.int32 and got.seg_size.dtype == torch.int32
    assert got.labels.tolist() == labels, (name, got.labels.tolist())
    assert got.n_segments == len(sizes) and got.seg_size.tolist() == sizes, (name, got.n_segments, got.seg_size.tolist())
    full = fn(normals, edges, max_weight, min_verts, trim=False)
    assert full.seg_size.tolist() == sizes + [0] * (len(labels) - len(sizes)) and full.n_segments.tolist() == [len(sizes)], name


def assert_same(got, want, what=""):
    """two MeshSegments, entry for entry"""
    assert got.trimmed == want.trimmed, what
    if got.trimmed:
        assert got.n_segments == want.n_segments, (what, got.n_segments, want.n_segments)
    else:
        assert got.n_segments.cpu().tolist() == want.n_segments.cpu().tolist(), what
    assert got.labels.shape == want.labels.shape and got.seg_size.shape == want.seg_size.shape, what
    bad = torch.nonzero(got.labels.cpu() != want.labels.cpu()).reshape(-1)
    assert bad.numel() == 0, (what, "labels differ at", bad[:8].tolist())
    assert torch.equal(got.seg_size.cpu(), want.seg_size.cpu()), what


def same_partition(a, b):
    """two label vectors describe the same partition (the ids may be numbered differently; 0 = dropped in both)"""
    a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    if a.shape != b.shape or ((a == 0) != (b == 0)).any():
        return False
    pairs = np.unique(np.stack([a, b], 1), axis=0)
    return len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))


# ---- generated cases (each built once) ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shuffled_chain(n=8192, seed=1):
    """one chain through all n vertices in shuffled vertex order, equal normals: one segment; long parent paths under contention"""
    order = np.random.default_rng(seed).permutation(n).astype(np.int32)
    edges = np.stack([order[:-1], order[1:]], 1)
    return torch.tensor([Z] * n, dtype=torch.float32), torch.from_numpy(edges), 0.0, 20


_AXES = np.asarray([X, Y, Z, (-1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, -1.0)], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def grid_mesh(kind, side=64, seed=2):
    """a side x side grid mesh.  "axes": normals drawn from the six axis directions, so weights are exactly 0, 1 or 2 and tie all over;
    max_weight = 0 links equal neighbours only and min_verts = 20 gives five rounds.  "random": random unit normals, max_weight 0.3."""
    g = np.random.default_rng(seed)
    if kind == "axes":
        normals, max_weight = _AXES[g.integers(0, 6, side * side)], 0.0
    else:
        n = g.standard_normal((side * side, 3))
        normals, max_weight = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32), 0.3
    return torch.from_numpy(np.ascontiguousarray(normals)), torch.from_numpy(faces_to_edges(_grid_faces(side, side))), max_weight, 20


@functools.lru_cache(maxsize=None)
def box_room(normal_noise=0.0, n_obj=8, step=0.05, seed=3):
    """synth.make_box_mesh: about 54 thousand vertices, of which the floor -- one component, the hot root -- holds 40 401"""
    from vlsat_amd import synth
    return synth.make_box_mesh(n_obj, step, seed, normal_noise=normal_noise)


def room_case(normal_noise=0.0, max_angle_deg=10.0):
    from vlsat_amd import prep
    m = box_room(normal_noise)
    return (torch.from_numpy(m["normals"].astype(np.float32)), torch.from_numpy(prep.mesh_edges(m["faces"])),
            float(np.float32(1.0 - math.cos(math.radians(max_angle_deg)))), 20)


@functools.lru_cache(maxsize=None)
def host_result(key):
    """the host restatement of a generated case, computed once per process: key = ("chain",) | ("grid", kind) | ("room", noise)"""
    from vlsat_amd import prep
    case = {"chain": shuffled_chain, "grid": grid_mesh, "room": room_case}[key[0]](*key[1:])
    return prep.segment_mesh_host(*case)
