#!/usr/bin/env python3
"""Golden vectors for the scan-splitting rule (vlsat_amd/prep.py::split_seeds* / split_groups*), made by the REAL reference function:

    data_processing/gen_data.py   generate_groups (:56-183), BBOX method (:108-122)

Run once where the reference is available:  python tests/golden/make_golden_split.py

gen_data.py imports modules this image lacks (``trimesh``, ``open3d``, ``tqdm``) and two that are not in the reference's tree
(``utils.util_label``, ``utils.util_search``); ``generate_groups`` uses none of them on the BBOX path, so empty stand-ins are installed
(``trimesh.points.PointCloud`` exists only because the function's annotation names it).  Its module-level ``args`` (the argument
parser's result, read for ``verbose`` and ``split_method``) is set to a namespace with the defaults.  The cloud handed over is an
object with the two attributes the function reads: ``vertices`` (float64, as trimesh hands them over; the values are float32 values)
and ``metadata['ply_raw']['vertex']['data']`` with a ``label`` or an ``objectId`` column.

``np.random.choice`` is wrapped to RECORD every draw: the vertex it returned and its RANK in the array it was drawn from (the
selectable vertices; for the first draw all vertices) -- the ranks replay the run through ``split_seeds(ranks=...)``.

The product compares squared distances (dmin2 > distance^2) where the reference compares sqrt(dmin2) > distance, and both compare box
faces strictly; this script ASSERTS that no vertex of any case comes within 1e-9 (relative) of the distance threshold at any step, or
within 1e-9 of a box face, so that the two forms cannot differ on these cases.

Written: split_cases.npz -- per case k: pts_k f32 [V,3], seg_k i32 [V], params_k f64 [distance, bbox_distance, min_seg_per_group],
seeds_k / ranks_k i64 [K] (the reference's draws), group_ptr_k i64 [G+1] + group_ids_k i64 (the returned groups, flattened).
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("VLSAT_REFERENCE", "/root/reference")
MARGIN = 1e-9


def install_standins():
    tm = types.ModuleType("trimesh")
    tm.points = types.SimpleNamespace(PointCloud=object)
    sys.modules["trimesh"] = tm
    for name in ("open3d", "tqdm", "utils.util_label", "utils.util_search"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["tqdm"].tqdm = lambda it, *a, **k: it
    sys.modules["utils.util_search"].SAMPLE_METHODS = None
    sys.modules["utils.util_search"].find_neighbors = None
    sys.path[:0] = [REF]


class Cloud:
    def __init__(self, pts, seg, column):
        self.vertices = pts.astype(np.float64)
        self.metadata = {"ply_raw": {"vertex": {"data": {column: seg.reshape(-1, 1)}}}}


def make_cloud(v, seed, extent, ids):
    g = np.random.default_rng(seed)
    pts = (g.random((v, 3)) * np.asarray(extent)).astype(np.float32)
    ids = np.asarray(ids)
    cell = (np.floor(pts[:, 0] / extent[0] * 5).astype(np.int64) * 4 + np.floor(pts[:, 1] / extent[1] * 4).astype(np.int64)) % len(ids)
    return pts, ids[cell].astype(np.int32)


CASES = [   # (V, seed, extent, ids, column, distance, bbox_distance, min_seg_per_group)
    (400, 1, (4.0, 3.0, 2.5), list(range(1, 21)), "label", 1.0, 0.75, 5),
    (600, 2, (5.0, 2.0, 2.0), [0] + list(range(3, 40, 3)) + [4097, 5000], "objectId", 1.0, 0.75, 5),
    (350, 3, (3.0, 3.0, 1.0), list(range(1, 36)), "label", 0.8, 0.5, 3),
    (200, 4, (0.6, 0.5, 0.4), list(range(1, 9)), "label", 1.0, 0.75, 5),           # every vertex within the distance: one seed
]


def check_margins(pts, seeds, distance, bbox):
    p = pts.astype(np.float64)
    dmin = None
    for s in seeds:
        d = np.linalg.norm(p[:, :2] - p[s, :2], axis=1)
        dmin = d if dmin is None else np.minimum(d, dmin)
        assert (np.abs(dmin - distance) > MARGIN * distance).all(), "a vertex lies within the margin of the seed distance"
    for s in seeds:
        for face in (p[s] - bbox, p[s] + bbox):
            assert (np.abs(p - face) > MARGIN).all(), "a vertex lies within the margin of a box face"


def main():
    install_standins()
    from data_processing import gen_data as GD
    GD.args = types.SimpleNamespace(verbose=False, split_method="BBOX")
    out = {}
    real_choice = np.random.choice
    for k, (v, seed, extent, ids, column, distance, bbox, min_seg) in enumerate(CASES):
        pts, seg = make_cloud(v, seed, extent, ids)
        drawn, ranks = [], []

        def choice(a, size=None, *args, **kw):
            got = real_choice(a, size, *args, **kw)
            arr = np.asarray(a)
            assert np.size(got) == 1 and (np.diff(arr) > 0).all()
            drawn.append(int(np.ravel(got)[0]))
            ranks.append(int(np.searchsorted(arr, drawn[-1])))
            assert arr[ranks[-1]] == drawn[-1]
            return got

        np.random.seed(1000 + k)
        np.random.choice = choice
        try:
            groups = GD.generate_groups(Cloud(pts, seg, column), distance=distance, bbox_distance=bbox, min_seg_per_group=min_seg)
        finally:
            np.random.choice = real_choice
        check_margins(pts, drawn, distance, bbox)
        groups = [[int(i) for i in g] for g in groups]
        out[f"pts_{k}"], out[f"seg_{k}"] = pts, seg
        out[f"params_{k}"] = np.asarray([distance, bbox, min_seg], dtype=np.float64)
        out[f"seeds_{k}"], out[f"ranks_{k}"] = np.asarray(drawn, dtype=np.int64), np.asarray(ranks, dtype=np.int64)
        out[f"group_ptr_{k}"] = np.cumsum([0] + [len(g) for g in groups]).astype(np.int64)
        out[f"group_ids_{k}"] = np.asarray([i for g in groups for i in g], dtype=np.int64)
        print(f"case {k}: V={v} seeds={len(drawn)} groups kept={len(groups)} sizes={[len(g) for g in groups]}")
    out["n_cases"] = np.asarray(len(CASES))
    path = os.path.join(HERE, "split_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
