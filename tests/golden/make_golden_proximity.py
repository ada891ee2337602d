#!/usr/bin/env python3
"""Golden vectors for the proximity edge rule (vlsat_amd/prep.py::proximity_edges*), made by the REAL reference dataset code:

    src/dataset/dataset_3dssg.py   load_mesh (:38-58), SSGDatasetGraph.data_preparation (:244-367) -- its local ``instances_box``
                                   (:286-288: min - padding, max + padding of ALL points of an instance)

Run once where the reference is available:  python tests/golden/make_golden_proximity.py

The committed label mesh tests/golden/scan_small.ply is read by the reference's ``load_mesh`` through the trimesh stand-in of
make_golden_scan.py; ``data_preparation`` runs on it with the annotations of scan_small_relationships.json, and a profile hook
reads its local ``instances_box`` at the return (as make_golden_scene_graph.py reads locals).  ``load_mesh`` hands the vertices
over as float64; the PLY stores float32, so they are passed on as the float32 values they are, which makes the reference's
``min - padding`` ONE float32 operation -- the operation the product's rule is stated in.  The float64 result is recorded as well.

Written: proximity_cases.npz -- nodes, padding, box_lo / box_hi (the reference's padded boxes, float32), box_lo64 / box_hi64 (the same
from float64 vertices) and intersect (bool [N,N]: the reference's padded boxes of i and j overlap strictly on all three axes).
"""
import copy
import json
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402
import make_golden_scan as GS  # noqa: E402


def run_reference(ds, D, points, instances, objs, classes, rel, relations, padding):
    """data_preparation's local ``instances_box`` at its return."""
    seen = {}

    def hook(frame, event, arg):
        if event == "return" and frame.f_code is D.SSGDatasetGraph.data_preparation.__code__:
            seen["instances_box"] = dict(frame.f_locals["instances_box"])

    np.random.seed(1234)
    sys.setprofile(hook)
    try:
        ds.data_preparation(points, instances, 16, 8, scene_id="scan-a", instance2labelName=objs, classNames=classes,
                            rel_json=copy.deepcopy(rel), relationships=list(relations), multi_rel_outputs=True, padding=padding,
                            all_edge=True)
    finally:
        sys.setprofile(None)
    if "instances_box" not in seen:
        raise RuntimeError("the profile hook did not see the reference's locals")
    return seen["instances_box"]


def main():
    G.install_standins()
    GS.install_trimesh_stub()
    from src.dataset import dataset_3dssg as D
    from utils import util

    classes = util.read_txt_to_list(os.path.join(HERE, "3dssg_classes.txt"))
    relations = util.read_relationships(os.path.join(HERE, "3dssg_relations.txt"))
    doc = json.load(open(os.path.join(HERE, "scan_small_relationships.json")))
    tmp = tempfile.mkdtemp(prefix="vlsat_proximity_golden_")
    try:
        scan_dir = os.path.join(tmp, "3RScan", "scan-a")
        os.makedirs(scan_dir)
        shutil.copy(os.path.join(HERE, "scan_small.ply"), os.path.join(scan_dir, GS.LABEL_FILE))
        mesh = D.load_mesh(scan_dir, GS.LABEL_FILE, False, False)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    import types
    ds = object.__new__(D.SSGDatasetGraph)
    ds.mconfig = types.SimpleNamespace(label_file=GS.LABEL_FILE)
    rel, objs, scans = ds.read_relationship_json(copy.deepcopy(doc), ["scan-a"])
    key = "scan-a_0"
    padding = 0.2
    pts64 = np.asarray(mesh["points"], dtype=np.float64)
    pts32 = pts64.astype(np.float32)
    assert np.array_equal(pts32.astype(np.float64), pts64)            # the PLY's float32 values, exactly
    inst = np.asarray(mesh["instances"])
    box32 = run_reference(ds, D, pts32, inst, objs[key], classes, rel[key], relations, padding)
    box64 = run_reference(ds, D, pts64, inst, objs[key], classes, rel[key], relations, padding)
    nodes = list(box32.keys())
    assert nodes == list(box64.keys())
    lo = np.stack([box32[i][0] for i in nodes])
    hi = np.stack([box32[i][1] for i in nodes])
    assert lo.dtype == np.float32 and hi.dtype == np.float32
    n = len(nodes)
    inter = np.zeros((n, n), dtype=bool)
    for a in range(n):
        for b in range(n):
            inter[a, b] = bool(np.all(lo[a] < hi[b]) and np.all(lo[b] < hi[a]))
    np.savez_compressed(os.path.join(HERE, "proximity_cases.npz"), nodes=np.asarray(nodes, dtype=np.int64), padding=np.float64(padding),
                        box_lo=lo, box_hi=hi, box_lo64=np.stack([box64[i][0] for i in nodes]), box_hi64=np.stack([box64[i][1] for i in nodes]),
                        intersect=inter)
    print("written proximity_cases.npz: nodes", nodes, "intersecting ordered pairs", int(inter.sum()) - n, "of", n * (n - 1))


if __name__ == "__main__":
    main()
