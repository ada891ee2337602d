"""Deterministic synthetic weights and 3RScan-shaped scenes (numpy only).

Both generators are pure functions of (name/seed) so that this container (where the
golden vectors are made from the real reference) and the GPU box (which never sees the
reference) regenerate bit-identical tensors without shipping >100 MB of fixtures.

Scene semantics restate the reference input contract:
  * per-object descriptor = ``gen_descriptor`` on the raw sampled points
    (reference ``src/utils/op_utils.py:47-64``: mean, unbiased std, max-min, volume, max dim),
  * points are then zero-meaned per object (reference ``src/dataset/dataset_3dssg.py:291-293``),
  * fully-connected directed edges, source-major, no self loops
    (reference ``src/dataset/dataset_3dssg.py:264-266``),
  * a batch is the concatenation of scenes with node-index offsets and ``batch_ids [N,1]``
    (reference ``src/dataset/DataLoader.py:153-176``),
  * ``obj_points`` is handed to the model as ``[N,3,P]`` (reference ``src/model/model.py:79``).
"""
from __future__ import annotations

import zlib
from collections import OrderedDict

import numpy as np

from .config import VLSATConfig, param_shapes


def _rng(name: str, seed: int) -> np.random.Generator:
    return np.random.default_rng([int(seed) & 0x7FFFFFFF, zlib.crc32(name.encode())])


def make_weights(cfg: VLSATConfig, seed: int = 0) -> "OrderedDict[str, np.ndarray]":
    """Formula weights: xavier-uniform matrices, small non-zero biases and deliberately
    non-trivial LayerNorm / BatchNorm statistics (default init would hide BN-folding and
    LN-affine bugs)."""
    out: "OrderedDict[str, np.ndarray]" = OrderedDict()
    for name, shape in param_shapes(cfg).items():
        g = _rng(name, seed)
        leaf = name.rsplit(".", 1)[1]
        is_norm = (".layer_norm." in name or name.startswith("mlp_3d.1.") or any(f".bn{i}." in name for i in range(1, 6))
                   or name.startswith("mmg.self_attn_fc.2.") or name.startswith("mmg.self_attn_fc.5."))
        if is_norm:
            if leaf == "weight":
                w = g.uniform(0.9, 1.1, shape)
            elif leaf == "bias":
                w = g.uniform(-0.05, 0.05, shape)
            elif leaf == "running_mean":
                w = g.uniform(-0.1, 0.1, shape)
            else:  # running_var
                w = g.uniform(0.5, 1.5, shape)
        elif leaf == "bias":
            w = g.uniform(-0.05, 0.05, shape)
        else:
            fan_out, fan_in = shape[0], int(np.prod(shape[1:]))
            a = np.sqrt(6.0 / (fan_in + fan_out))
            w = g.uniform(-a, a, shape)
        out[name] = np.ascontiguousarray(w, dtype=np.float32)
    return out


def make_weights_stress(cfg: VLSATConfig, scale: float, seed: int = 0) -> "OrderedDict[str, np.ndarray]":
    """Trained-scale stress weights: the formula weights with every GCN matrix (nn_edge, proj_*, the gate MLP, prop)
    multiplied by ``scale`` and LayerNorm gains drawn from U(0.3, 3).  Exercises the node-side hoisting of
    nn_edge.0 / proj_query / gate layer 1 (reference network_MMG.py:84-112) away from Xavier scale, where a
    summation-order slip would hide below the tolerance."""
    w = make_weights(cfg, seed)
    for name in list(w):
        if ".layer_norm.weight" in name:
            w[name] = _rng(name + "/stress", seed).uniform(0.3, 3.0, w[name].shape).astype(np.float32)
        elif (".gcn_2ds." in name or ".gcn_3ds." in name) and name.endswith(".weight"):
            w[name] = (w[name] * np.float32(scale)).astype(np.float32)
    return w


def fc_edges(n: int) -> np.ndarray:
    """[2,E] source-major fully-connected pairs without self loops, E = n(n-1)."""
    src = np.repeat(np.arange(n, dtype=np.int64), n)
    dst = np.tile(np.arange(n, dtype=np.int64), n)
    keep = src != dst
    return np.stack([src[keep], dst[keep]], 0)


def gen_descriptor(raw: np.ndarray) -> np.ndarray:
    """raw [N,P,3] float32 -> [N,11] (centroid, unbiased std, dims, volume, max dim)."""
    raw64 = raw.astype(np.float64)
    mean = raw64.mean(1)
    std = raw64.std(1, ddof=1)
    dims = raw64.max(1) - raw64.min(1)
    vol = dims.prod(-1, keepdims=True)
    length = dims.max(-1, keepdims=True)
    return np.concatenate([mean, std, dims, vol, length], -1).astype(np.float32)


def make_scene(n_obj: int, n_pts: int, seed: int, clip_dim: int = 512) -> dict:
    """One scene: dict of numpy arrays in the reference's model-input layout."""
    g = np.random.default_rng([int(seed) & 0x7FFFFFFF, 0x3D55])
    centre = g.uniform(0.0, 4.0, (n_obj, 1, 3))
    ext = g.uniform(0.2, 1.0, (n_obj, 1, 3))
    raw = (centre + g.uniform(-0.5, 0.5, (n_obj, n_pts, 3)) * ext).astype(np.float32)
    desc = gen_descriptor(raw)
    pts = raw - raw.mean(1, keepdims=True, dtype=np.float64).astype(np.float32)
    f2d = g.standard_normal((n_obj, clip_dim))
    f2d = (f2d / np.linalg.norm(f2d, axis=-1, keepdims=True)).astype(np.float32)
    return {
        "obj_points": np.ascontiguousarray(pts.transpose(0, 2, 1)),   # [N,3,P]
        "obj_2d_feats": f2d,                                           # [N,512]
        "edge_indices": fc_edges(n_obj),                               # [2,E] int64
        "descriptor": desc,                                            # [N,11]
        "batch_ids": np.zeros((n_obj, 1), dtype=np.int64),            # [N,1]
    }


def collate(scenes: list) -> dict:
    """Concatenate scenes the way ``collate_fn_mmg`` does (reference DataLoader.py:153-176):
    node tensors stacked, edge indices offset by the running node count, batch_ids = scene id."""
    off, ei, bid = 0, [], []
    for s, sc in enumerate(scenes):
        n = sc["obj_points"].shape[0]
        ei.append(sc["edge_indices"] + off)
        bid.append(np.full((n, 1), s, dtype=np.int64))
        off += n
    return {
        "obj_points": np.concatenate([s["obj_points"] for s in scenes], 0),
        "obj_2d_feats": np.concatenate([s["obj_2d_feats"] for s in scenes], 0),
        "edge_indices": np.concatenate(ei, 1),
        "descriptor": np.concatenate([s["descriptor"] for s in scenes], 0),
        "batch_ids": np.concatenate(bid, 0),
    }


def make_batch(n_scenes: int, n_obj: int, n_pts: int, seed0: int = 1000) -> dict:
    """Batch of ``n_scenes`` scenes with seeds seed0, seed0+1, ...."""
    return collate([make_scene(n_obj, n_pts, seed0 + s) for s in range(n_scenes)])


# ---- config-switch parity cases (tests/golden/make_golden_switches.py makes their goldens from the real reference) ----
SWITCH_CASES = {
    "switch_with_bn": dict(N_LAYERS=2, WITH_BN=True),
    "switch_no_gcn_edge": dict(N_LAYERS=2, USE_GCN_EDGE=False),
    "switch_single_rel": dict(N_LAYERS=2, multi_rel_outputs=False, num_rel_class=27),
    "switch_rgb_normal": dict(N_LAYERS=2, USE_RGB=True, USE_NORMAL=True),
    "switch_feature_transform": dict(N_LAYERS=1, feature_transform=True),
    "switch_all": dict(feature_transform=True, N_LAYERS=1, GCN_AGGR="mean", WITH_BN=True, USE_GCN_EDGE=False, multi_rel_outputs=False,
                       num_rel_class=27, USE_RGB=True, USE_NORMAL=True),
}


def switch_scenes(cfg: VLSATConfig) -> list:
    """The ragged pair of scenes (4 and 6 objects x 32 points) every switch case runs on; colour / normal channels
    (cfg.dim_point > 3) are seeded uniform values in [-1, 1] appended after xyz."""
    out = []
    for i, n in enumerate((4, 6)):
        sc = make_scene(n, 32, 5000 + i)
        if cfg.dim_point > 3:
            g = np.random.default_rng([5000 + i, cfg.dim_point])
            extra = g.uniform(-1, 1, (n, cfg.dim_point - 3, 32)).astype(np.float32)
            sc["obj_points"] = np.concatenate([sc["obj_points"], extra], 1)
        out.append(sc)
    return out


def make_room(n_obj: int, pts_per_obj: int, seed: int, extent=(10.0, 10.0, 3.0)):
    """A room with spatial structure (``make_scene`` has none: its objects all overlap): ``n_obj`` small boxes scattered over
    ``extent`` metres, ``pts_per_obj`` points each -> (scene_points f32[n_obj * pts_per_obj, 3], instances i32[...] with ids
    1..n_obj, object-major).  Objects are 0.2-1.2 m wide and up to 1 m tall, centres uniform in the room (the lower half in z)."""
    g = np.random.default_rng([int(seed) & 0x7FFFFFFF, 0x200F])
    ext = np.asarray(extent, dtype=np.float64)
    centre = g.uniform(0.0, 1.0, (n_obj, 1, 3)) * ext * np.array([1.0, 1.0, 0.5])
    size = g.uniform(0.2, 1.2, (n_obj, 1, 3)) * np.array([1.0, 1.0, 1.0 / 1.2])
    pts = (centre + g.uniform(-0.5, 0.5, (n_obj, pts_per_obj, 3)) * size).astype(np.float32)
    inst = np.repeat(np.arange(1, n_obj + 1, dtype=np.int32), pts_per_obj)
    return np.ascontiguousarray(pts.reshape(-1, 3)), inst


def _grid_triangles(idx: np.ndarray, pts: np.ndarray, outward: np.ndarray) -> np.ndarray:
    """Two triangles per cell of the vertex-index grid ``idx`` [A+1, B+1], wound so that their normal points along ``outward``."""
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    tri = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)])
    t0 = tri[0]
    if np.dot(np.cross(pts[t0[1]] - pts[t0[0]], pts[t0[2]] - pts[t0[0]]), outward) < 0:
        tri = tri[:, ::-1]
    return tri


def make_box_mesh(n_obj: int, step: float, seed: int, normal_noise: float = 0.0, extent=(10.0, 10.0)) -> dict:
    """A room as a triangle MESH, for the mesh segmenter: a floor of ``extent`` metres plus ``n_obj`` closed axis-aligned boxes standing
    on it (separate surfaces: nothing connects a box to the floor), every surface tessellated on a grid of spacing ``step``, two
    triangles per cell.  A box is 0.4-1.2 m along each axis and at least 6 cells, so each of its faces has at least 25 interior
    vertices.  The vertices on a box's edges and corners are SHARED between its faces and carry the normalised average of the faces'
    normals, as a reconstruction's vertex normals do at a crease.  ``normal_noise`` > 0 adds that many standard normals to every
    component of every normal and renormalises.

    -> the dict of ``scan.read_mesh``: ``points`` f64 [V,3], ``normals`` f64 [V,3], ``colors`` None, ``faces`` i32 [F,3], ``instances``
    i64 [V] = the GENERATING object (1 = floor, 2 + k = box k), plus ``plane`` i32 [V]: the planar face a vertex belongs to (0 = floor,
    1 + 6 k + f = face f of box k in the order -x, +x, -y, +y, -z, +z) or -1 for a crease vertex, which belongs to several."""
    g = np.random.default_rng([int(seed) & 0x7FFFFFFF, 0xB0C5])
    step = float(step)
    pts, nrm, plane, inst, faces = [], [], [], [], []
    nx, ny = (max(2, int(round(e / step))) for e in extent)
    ii, jj = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="ij")
    floor = np.stack([ii.ravel() * step, jj.ravel() * step, np.zeros(ii.size)], 1)
    pts.append(floor)
    nrm.append(np.tile([0.0, 0.0, 1.0], (len(floor), 1)))
    plane.append(np.zeros(len(floor), np.int32))
    inst.append(np.ones(len(floor), np.int64))
    faces.append(_grid_triangles(np.arange(len(floor)).reshape(nx + 1, ny + 1), floor, np.array([0.0, 0.0, 1.0])))
    base = len(floor)
    for k in range(n_obj):
        cells = np.maximum(6, np.rint(g.uniform(0.4, 1.2, 3) / step).astype(np.int64))
        origin = np.array([*(g.uniform(0.0, max(extent[d] - cells[d] * step, 0.0)) for d in range(2)), 0.0])
        lat = np.stack(np.meshgrid(*(np.arange(c + 1) for c in cells), indexing="ij"), -1)           # [a+1, b+1, c+1, 3]
        side = (lat == cells).astype(np.int64) - (lat == 0).astype(np.int64)                            # outward direction per axis
        on = (side != 0).any(-1)
        vid = np.full(on.shape, -1, np.int64)
        vid[on] = base + np.arange(int(on.sum()))
        s = side[on]
        p = origin + lat[on] * step
        n_faces_at = (s != 0).sum(1)
        axis = np.argmax(s != 0, 1)
        pl = np.where(n_faces_at == 1, 1 + 6 * k + 2 * axis + (s[np.arange(len(s)), axis] > 0), -1)
        pts.append(p)
        nrm.append(s / np.linalg.norm(s, axis=1, keepdims=True))
        plane.append(pl.astype(np.int32))
        inst.append(np.full(len(p), 2 + k, np.int64))
        allp = np.concatenate(pts)
        for d in range(3):
            for end, sign in ((0, -1.0), (int(cells[d]), 1.0)):
                out = np.zeros(3)
                out[d] = sign
                faces.append(_grid_triangles(np.take(vid, end, axis=d), allp, out))
        base += len(p)
    points, normals = np.concatenate(pts), np.concatenate(nrm)
    if normal_noise > 0:
        normals = normals + float(normal_noise) * g.standard_normal(normals.shape)
        normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    return {"points": points, "colors": None, "normals": normals, "instances": np.concatenate(inst),
            "faces": np.ascontiguousarray(np.concatenate(faces), dtype=np.int32), "plane": np.concatenate(plane)}


def make_plates(step: float, jitter: float, seed: int) -> dict:
    """Two perpendicular unit plates that share an edge -- an L -- as a CLOUD without faces, for the cloud segmenter: plate 0 is z = 0
    over x, y in [0, 1], plate 1 is x = 0 over y, z in [0, 1], both sampled on a grid of spacing ``step``; the shared line x = z = 0
    is sampled once and belongs to plate 0.  ``jitter`` > 0 adds that many standard normals to every coordinate.
    -> {"points": f64 [V,3], "plate": i32 [V]}, plate 0 first, each plate in the order of the coordinate that leaves the crease."""
    g = np.random.default_rng([int(seed) & 0x7FFFFFFF, 0x91A7E5])
    n = max(1, int(round(1.0 / float(step))))
    i, j = (x.ravel() for x in np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij"))
    zero = np.zeros(i.size)
    a = np.stack([i / n, j / n, zero], 1)
    keep = i > 0
    b = np.stack([zero, j / n, i / n], 1)[keep]
    points = np.concatenate([a, b])
    if jitter > 0:
        points = points + float(jitter) * g.standard_normal(points.shape)
    return {"points": points, "plate": np.concatenate([np.zeros(len(a), np.int32), np.ones(len(b), np.int32)])}


def make_fused_cloud(points, seed: int = 7, jitter: float = 0.002, views: int = 8, view_noise: float = 0.005, x_below: float = 5.0) -> np.ndarray:
    """A cloud of uneven density, as fusing overlapping frames leaves it: every point of ``points`` with N(0, ``jitter``) added to each
    coordinate, then the points with x < ``x_below`` ``views`` more times, each time with fresh N(0, ``view_noise``) noise, one view
    after the other.  -> f64 [V + views * H, 3]; row i < V belongs to input point i, and ``make_fused_index`` names the input point of
    every row."""
    g = np.random.default_rng(int(seed))
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    half = p[p[:, 0] < x_below]
    parts = [p + g.normal(0.0, jitter, p.shape)]
    parts += [half + g.normal(0.0, view_noise, half.shape) for _ in range(int(views))]
    return np.concatenate(parts)


def make_fused_index(points, views: int = 8, x_below: float = 5.0) -> np.ndarray:
    """The input point behind every row of ``make_fused_cloud``: int64 [V + views * H]."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    return np.concatenate([np.arange(len(p))] + [np.nonzero(p[:, 0] < x_below)[0]] * int(views))


def make_walled_room(n_obj: int, step: float, seed: int, height: float = 2.0, extent=(10.0, 10.0)) -> dict:
    """A room with WALLS as a cloud without faces, for the object segmenter: the points and ``instances`` of ``make_box_mesh(n_obj,
    step, seed, extent=extent)`` plus four walls of ``height`` metres on the floor's border -- x = 0, x = extent[0], y = 0, y =
    extent[1] -- sampled on the same grid of spacing ``step`` from z = step upwards (the row z = 0 is the floor's; a corner column
    belongs to the x wall).  -> {"points": f64 [V,3], "instances": i64 [V] (1 = floor, 2 + k = box k, n_obj + 2 + w = wall w in the
    order above), "plane": i32 [V] (``make_box_mesh``'s numbering, then 1 + 6 n_obj + w for wall w), "structural": bool [V] (floor and
    walls), "n_obj", "step", "height", "extent"}."""
    room = make_box_mesh(n_obj, step, seed, extent=extent)
    step = float(step)
    nx, ny = (max(2, int(round(e / step))) for e in extent)
    nz = max(1, int(round(float(height) / step)))
    pts, inst, plane = [room["points"]], [room["instances"]], [room["plane"]]
    for w in range(4):
        along = np.arange((ny if w < 2 else nx) + 1)
        if w >= 2:
            along = along[1:-1]
        a, z = (x.ravel() for x in np.meshgrid(along, np.arange(1, nz + 1), indexing="ij"))
        fixed = np.full(a.size, (0, nx, 0, ny)[w] * step)
        p = np.stack([fixed, a * step, z * step], 1) if w < 2 else np.stack([a * step, fixed, z * step], 1)
        pts.append(p)
        inst.append(np.full(len(p), n_obj + 2 + w, np.int64))
        plane.append(np.full(len(p), 1 + 6 * n_obj + w, np.int32))
    instances = np.concatenate(inst)
    return {"points": np.concatenate(pts), "instances": instances, "plane": np.concatenate(plane),
            "structural": (instances == 1) | (instances >= n_obj + 2), "n_obj": int(n_obj), "step": step, "height": nz * step,
            "extent": (nx * step, ny * step)}


STACKED_BOXES = (((0.0, 0.0, 0.0), (1.0, 1.0, 0.5)), ((0.3, 0.3, 0.5), (0.6, 0.6, 0.8)), ((1.0, 0.2, 0.0), (1.4, 0.6, 0.3)),
                 ((0.05, 0.62, 0.5), (0.35, 0.92, 0.7)), ((0.35, 0.62, 0.5), (0.55, 0.9, 0.95)))


def make_stacked_boxes(step: float = 0.02, jitter: float = 0.0008, seed: int = 0, viewpoint=(3.0, -2.5, 2.5)) -> dict:
    """Bodies that TOUCH, as one scan sees them, for the convexity clusters: a table (box 0), three boxes standing on it -- boxes 3 and 4
    touch each other and their fronts y = 0.62 are coplanar -- and a lower box against the table's side (``STACKED_BOXES``, (lo, hi) in
    metres at ``step`` = 0.02; another ``step`` scales the boxes by step / 0.02, so the number of points does not change; ``jitter``
    and ``viewpoint`` are taken as given).  Of every box only the faces whose outward normal faces ``viewpoint`` (from the face's
    centre) are sampled, on a grid of ``step`` that starts at the box's lower corner -- an extent that is no whole number of steps
    (box 4 is 22.5 high) leaves the last half step empty -- so an edge between two visible faces is sampled once by each, with that
    face's normal.  Every point inside or on ANOTHER box (closed, widened by 1e-6) is removed: a scan has no hidden surfaces.
    ``jitter`` > 0 then adds that many standard normals to every coordinate.
    -> {"points": f64 [V,3], "normals": f64 [V,3] (the exact face normals), "instances": i64 [V] (1 + box), "viewpoint": (x, y, z)};
    box by box, face by face in the order -x, +x, -y, +y, -z, +z."""
    g = np.random.default_rng([int(seed) & 0x7FFFFFFF, 0x57AC4ED])
    step = float(step)
    view = np.asarray([float(x) for x in viewpoint], dtype=np.float64)
    boxes = [(np.asarray(lo) * (step / 0.02), np.asarray(hi) * (step / 0.02)) for lo, hi in STACKED_BOXES]
    pts, nrm, inst = [], [], []
    for b, (lo, hi) in enumerate(boxes):
        grid = [lo[a] + step * np.arange(int(np.floor((hi[a] - lo[a]) / step + 1e-6)) + 1) for a in range(3)]
        for axis in range(3):
            for sign, end in ((-1.0, lo[axis]), (1.0, hi[axis])):
                if sign * (view[axis] - end) <= 0.0:
                    continue
                u, v = (a for a in range(3) if a != axis)
                uu, vv = (x.ravel() for x in np.meshgrid(grid[u], grid[v], indexing="ij"))
                p = np.zeros((uu.size, 3))
                p[:, axis], p[:, u], p[:, v] = end, uu, vv
                n = np.zeros((uu.size, 3))
                n[:, axis] = sign
                pts.append(p)
                nrm.append(n)
                inst.append(np.full(uu.size, 1 + b, np.int64))
    points, normals, instances = np.concatenate(pts), np.concatenate(nrm), np.concatenate(inst)
    keep = np.ones(len(points), dtype=bool)
    for b, (lo, hi) in enumerate(boxes):
        keep &= ~(((points >= lo - 1e-6) & (points <= hi + 1e-6)).all(1) & (instances != 1 + b))
    points = points[keep]
    if jitter > 0:
        points = points + float(jitter) * g.standard_normal(points.shape)
    return {"points": points, "normals": normals[keep], "instances": instances[keep], "viewpoint": tuple(float(x) for x in view)}
