"""Real-data entry of the hot path (".ply -> tensors when 3RScan is available"): what the reference's dataset
class does on the host before ``Mmgnet.forward`` sees a scene, without trimesh --

* ``read_ply``                 the vertex element of a 3RScan label mesh (``labels.instances.align.annotated.v2.ply``): xyz, colours,
                               normals, instance id per vertex -- what ``load_mesh`` takes from trimesh (reference
                               ``src/dataset/dataset_3dssg.py:38-58``, ``utils/util_ply.py:8-14``);
* ``read_relationships``       ``relationships_*.json`` -> per-scan relationship lists and object-name maps
                               (``dataset_3dssg.py:215-243``, including the one scan the reference skips for the v2 label file);
* ``scene_nodes`` / ``edge_list`` / ``ground_truth``   the node order, the edge list and the labels of
                               ``data_preparation`` (``dataset_3dssg.py:248-266,281-283,300-336``);
* ``prepare_scan``             all of it + the per-object point selection, zero-mean, descriptor on the DEVICE (``prep.py``; reference
                               ``:279-294``) -> one batch dict in the layout ``evaluate.validation`` and ``VLSATModel.forward`` take;
* ``read_mesh`` / ``write_ply`` / ``vertex_normals`` / ``segment_scan``   a bare mesh with its faces, and the over-segmentation (on the
                               DEVICE, ``prep.segment_mesh``) that stands in for the instance ids when nobody has made any;
* ``segment_objects``          a bare cloud to OBJECT-level instances on the device: structural planes removed, the rest clustered.

The union point sets (``rel_points``, ``:337-359``) are not produced: ``Mmgnet.forward`` never reads them.  The host-side
functions are plain numpy; ``prepare_scan`` needs the GPU library.  Parity: PINNED to the reference's own dataset code --
``tests/golden/make_golden_scan.py`` imports ``dataset_3dssg`` / ``DataLoader`` / ``util`` / ``util_ply`` (with a stand-in for the
absent ``trimesh`` that only hands over the vertex table) and records what ``load_mesh``, ``read_relationship_json``,
``data_preparation`` (every combination of ``all_edge`` x ``multi_rel_outputs``, colour / normal channels, the draws of
``np.random.choice``), ``__getitem__`` + ``collate_fn_mmg`` and the name-list readers return; ``tests/test_scan_golden_cpu.py``
compares every function of this module with those fixtures, ``tests/test_hip_scan.py`` the device half on the recorded draws."""
from __future__ import annotations

import json
import os
from itertools import product
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}
# the scan whose segments and ply mismatch in 3RScan v2 (reference dataset_3dssg.py:219-226)
_BAD_V2_SCAN = "fa79392f-7766-2d5c-869a-f5d6cfb62fc6"


class ScanError(ValueError):
    pass


def read_ply(path: str) -> Dict[str, Optional[np.ndarray]]:
    """-> {"points": f64[V,3], "colors": u8[V,3] | None, "normals": f64[V,3] | None, "instances": i64[V]}.
    ASCII and binary_little_endian PLY; only the vertex element is read (faces are skipped by never reaching them).  The instance id
    of a vertex is its ``objectId`` property, else ``label`` (reference utils/util_ply.py:8-14)."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ScanError(f"{path}: not a PLY file")
        fmt, elements = None, []          # elements: [name, count, [(prop, dtype) | (prop, None) for lists]]
        while True:
            line = f.readline()
            if not line:
                raise ScanError(f"{path}: header without end_header")
            tok = line.decode("ascii", "replace").split()
            if not tok or tok[0] in ("comment", "obj_info"):
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                elements.append([tok[1], int(tok[2]), []])
            elif tok[0] == "property":
                if not elements:
                    raise ScanError(f"{path}: property before any element")
                if tok[1] == "list":
                    elements[-1][2].append((tok[-1], None))
                else:
                    if tok[1] not in _PLY_TYPES:
                        raise ScanError(f"{path}: unknown property type {tok[1]}")
                    elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]]))
            elif tok[0] == "end_header":
                break
        if fmt not in ("ascii", "binary_little_endian"):
            raise ScanError(f"{path}: format {fmt!r} is not supported (ascii, binary_little_endian)")
        vert = None
        for name, count, props in elements:
            scalar = all(t is not None for _, t in props)
            if name == "vertex":
                if not scalar:
                    raise ScanError(f"{path}: list property inside the vertex element")
                if fmt == "ascii":
                    vals = b" ".join(f.readline() for _ in range(count)).split()
                    if len(vals) != count * len(props):
                        raise ScanError(f"{path}: vertex rows do not hold {count} x {len(props)} values")
                    try:
                        table = np.array(vals, dtype=np.float64).reshape(count, len(props))
                    except ValueError:
                        raise ScanError(f"{path}: a vertex value is not a number") from None
                    # a value is parsed INTO its declared property type (a float32 written in decimal is that float32 again), as a
                    # PLY reader that fills the element's record does; integer columns go through int64 first
                    vert = {p: (table[:, i].astype(t) if t[0] == "f" else table[:, i].astype(np.int64).astype(t)) for i, (p, t) in enumerate(props)}
                else:
                    dt = np.dtype([(p, "<" + t) for p, t in props])
                    raw = f.read(dt.itemsize * count)
                    if len(raw) != dt.itemsize * count:
                        raise ScanError(f"{path}: vertex data truncated")
                    rec = np.frombuffer(raw, dtype=dt, count=count)
                    vert = {p: rec[p] for p, _ in props}
                break
            # an element in front of the vertices: skip it (scalar properties only -- a list would need parsing row by row)
            if not scalar:
                raise ScanError(f"{path}: element {name!r} with list properties precedes the vertices")
            if fmt == "ascii":
                for _ in range(count):
                    f.readline()
            else:
                f.seek(sum(np.dtype(t).itemsize for _, t in props) * count, os.SEEK_CUR)
        if vert is None:
            raise ScanError(f"{path}: no vertex element")
    for k in ("x", "y", "z"):
        if k not in vert:
            raise ScanError(f"{path}: vertex element has no {k}")
    out = {"points": np.stack([vert["x"], vert["y"], vert["z"]], 1).astype(np.float64)}
    out["colors"] = (np.stack([vert["red"], vert["green"], vert["blue"]], 1).astype(np.uint8)
                     if all(k in vert for k in ("red", "green", "blue")) else None)
    out["normals"] = (np.stack([vert["nx"], vert["ny"], vert["nz"]], 1).astype(np.float64)
                      if all(k in vert for k in ("nx", "ny", "nz")) else None)
    if "objectId" in vert:
        lab = vert["objectId"]
    elif "label" in vert:
        lab = vert["label"]
    else:
        raise ScanError(f"{path}: vertex element has neither objectId nor label")
    out["instances"] = np.asarray(lab).astype(np.int64).reshape(-1)
    return out


def scene_points(mesh: Dict[str, Optional[np.ndarray]], use_rgb: bool = False, use_normal: bool = False) -> np.ndarray:
    """xyz [+ rgb / 255] [+ normal] per vertex, the channel order of ``load_mesh`` (dataset_3dssg.py:43-52)."""
    pts = mesh["points"]
    if use_rgb:
        if mesh["colors"] is None:
            raise ScanError("USE_RGB: the mesh has no vertex colours")
        pts = np.concatenate([pts, mesh["colors"].astype(np.float64) / 255.0], 1)
    if use_normal:
        if mesh["normals"] is None:
            raise ScanError("USE_NORMAL: the mesh has no vertex normals")
        pts = np.concatenate([pts, mesh["normals"][:, :3]], 1)
    return pts


def read_name_list(path: str) -> List[str]:
    """classes.txt / relationships.txt: one name per line, exactly as the reference reads them (utils/util.py:15-21 ``read_txt_to_list``,
    :34-40 ``read_relationships``): trailing white space stripped, lower-cased, EVERY line kept -- an empty line is an entry (it
    takes an index), leading blanks stay."""
    with open(path, "r") as f:
        return [ln.rstrip().lower() for ln in f]


def read_relationships(path_or_data, selected_scans: Sequence[str],
                       label_file: str = "labels.instances.align.annotated.v2.ply") -> Tuple[dict, dict, list]:
    """relationships_{train,validation}.json -> (rel, objs, scans) keyed by ``<scan>_<split>`` exactly as the reference builds them
    (dataset_3dssg.py:215-243): rel[key] = list of [subject id, object id, relation id, relation name]; objs[key] = {instance id: label
    name} in the file's order (the node order of a scene follows it)."""
    data = path_or_data
    if isinstance(path_or_data, (str, os.PathLike)):
        with open(path_or_data) as f:
            data = json.load(f)
    selected = set(selected_scans)
    rel, objs, scans = {}, {}, []
    for scan_i in data["scans"]:
        if scan_i["scan"] == _BAD_V2_SCAN and label_file == "labels.instances.align.annotated.v2.ply":
            continue
        if scan_i["scan"] not in selected:
            continue
        key = scan_i["scan"] + "_" + str(scan_i["split"])
        rel[key] = [list(r) for r in scan_i["relationships"]]
        objs[key] = {int(i): name for i, name in scan_i["objects"].items()}
        scans.append(key)
    return rel, objs, scans


def scene_nodes(instances: np.ndarray, instance2label: Dict[int, str]) -> List[int]:
    """Instance ids of the scene's nodes, in the order of the object map, restricted to ids that own points; 0 is background
    (dataset_3dssg.py:251-261)."""
    present = set(int(i) for i in np.unique(instances))
    present.discard(0)
    return [int(i) for i in instance2label.keys() if int(i) in present]


def edge_list(nodes: Sequence[int], rel_json: Sequence[Sequence], all_edge: bool = True) -> np.ndarray:
    """i64[E,2] node-index pairs: every ordered pair i != j (source-major), or the annotated pairs only (dataset_3dssg.py:263-270)."""
    if all_edge:
        e = [(i, j) for i, j in product(range(len(nodes)), range(len(nodes))) if i != j]
    else:
        pos = {n: k for k, n in enumerate(nodes)}
        e = [(pos[r[0]], pos[r[1]]) for r in rel_json if r[0] in pos and r[1] in pos]
    return np.asarray(e, dtype=np.int64).reshape(-1, 2)


def ground_truth(nodes: Sequence[int], edges: np.ndarray, instance2label: Dict[int, str], class_names: Sequence[str],
                 rel_json: Sequence[Sequence], relation_names: Sequence[str], multi_rel_outputs: bool = True):
    """-> gt_class i64[N], gt_rel f32[E,R] (multi-label) | i64[E] (single label; 0 = none, a later annotation of a pair replaces
    an earlier one) -- dataset_3dssg.py:281-283,300-336.  Unknown names raise, as the reference's ``index`` / assert do."""
    class_pos = {n: k for k, n in enumerate(class_names)}
    rel_pos = {n: k for k, n in enumerate(relation_names)}
    try:
        gt_class = np.asarray([class_pos[instance2label[i]] for i in nodes], dtype=np.int64)
    except KeyError as e:
        raise ScanError(f"object label {e.args[0]!r} is not in the class list") from None
    pos = {n: k for k, n in enumerate(nodes)}
    n = len(nodes)
    adj = np.zeros((n, n, len(relation_names)), dtype=np.float32) if multi_rel_outputs else np.zeros((n, n), dtype=np.int64)
    for r in rel_json:
        if r[0] not in pos or r[1] not in pos:
            continue
        if r[3] not in rel_pos:
            raise ScanError(f"invalid relation name {r[3]!r}")
        k = rel_pos[r[3]]                  # (re-indexed by name: custom relation lists, :309)
        if multi_rel_outputs:
            adj[pos[r[0]], pos[r[1]], k] = 1.0
        else:
            adj[pos[r[0]], pos[r[1]]] = k
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    gt_rel = adj[edges[:, 0], edges[:, 1]] if len(edges) else np.zeros((0,) + adj.shape[2:], dtype=adj.dtype)   # (a one-object scan: no edge)
    return gt_class, gt_rel


def multi_view_feature_path(root: str, scene_id: str, instance_id: int, label: str) -> str:
    """Where the reference keeps an object's CLIP feature (dataset_3dssg.py:296-297)."""
    return os.path.join(root, f"data/3RScan/{scene_id}/multi_view/instance_{instance_id}_class_{label}_origin_view_mean.npy")


def prepare_scan(mesh_or_path, instance2label: Dict[int, str], class_names: Sequence[str], rel_json: Sequence[Sequence],
                 relation_names: Sequence[str], num_points: int, seed: int, device="cuda:0", multi_rel_outputs: bool = True,
                 all_edge: bool = True, use_rgb: bool = False, use_normal: bool = False, multi_view_root: Optional[str] = None,
                 scene_id: str = "", feature_loader: Optional[Callable[[int, str], np.ndarray]] = None,
                 edge_mode: Optional[str] = None, padding: float = 0.2, max_neighbors: int = 0) -> dict:
    """One scene, from the label mesh to the batch dict of ``evaluate.validation`` / ``VLSATModel.forward``: obj_points [N,C,P],
    obj_2d_feats [N,512], descriptor [N,11], edge_indices [E,2] (the loader's layout: ``forward`` takes its transpose, like the
    reference's ``process_val``), batch_ids [N,1], gt_class [N], gt_rel_cls [E,R] | [E], plus
    ``fc_sizes`` when the edge list is the fully connected one (and, for inspection, ``instance_ids``, ``points_per_instance``, ``choice``
    = the selected vertex indices [N,P]).  Points are selected, centred and described on the device
    (``prep.sample_objects`` / ``prep.prepare_objects``); extra channels (rgb, normals) are gathered with the same selection and are
    not centred (dataset_3dssg.py:291-293 centres xyz only).  ``feature_loader(instance id, label) -> f32[512]`` overrides the
    reference's file layout; without it and without ``multi_view_root`` the 2D features are zeros (as in the reference).

    ``edge_mode=None`` leaves the edge list to ``all_edge``.  ``edge_mode="proximity"`` builds a sparse list on the device instead
    (``prep.instance_boxes`` + ``prep.proximity_edges``: pairs whose boxes, padded by ``padding``, intersect; with ``max_neighbors > 0``
    only pairs in which one node is among the other's ``max_neighbors`` nearest -- the list is symmetric, so an out-degree can exceed
    the cap), computes the labels on that list, returns the unpadded ``boxes`` [N,6] too and omits ``fc_sizes``.  A pruned graph
    changes the model's outputs (edge attention and aggregation see fewer edges); ``annotation_coverage`` tells how many annotated
    pairs a setting keeps."""
    import torch

    from . import prep

    mesh = read_ply(mesh_or_path) if isinstance(mesh_or_path, (str, os.PathLike)) else mesh_or_path
    nodes = scene_nodes(mesh["instances"], instance2label)
    if not nodes:
        raise ScanError("no annotated instance owns a point of this mesh")
    if edge_mode not in (None, "proximity"):
        raise ScanError(f"edge_mode {edge_mode!r}: None (all_edge decides) or 'proximity'")
    proximity = edge_mode == "proximity"
    pts = scene_points(mesh, use_rgb, use_normal)
    dev = torch.device(device)
    d_inst = torch.from_numpy(mesh["instances"].astype(np.int32)).to(dev)
    d_ids = torch.tensor(nodes, dtype=torch.int32, device=dev)
    if len(set(nodes)) != len(nodes) or min(nodes) < 0 or max(nodes) >= (1 << 24):
        raise ScanError("instance ids of the scene's nodes must be distinct integers in [0, 2^24)")
    map_size = max(65536, max(nodes) + 1)
    d_xyz = torch.from_numpy(np.ascontiguousarray(pts[:, :3], dtype=np.float32)).to(dev)
    if proximity:
        boxes = prep.instance_boxes(d_xyz, d_inst, d_ids, map_size)
        d_edges = prep.proximity_edges(boxes, [len(nodes)], padding, max_neighbors)[0].t().contiguous()      # the loader's [E,2]
        edges = d_edges.cpu().numpy()
    else:
        edges = edge_list(nodes, rel_json, all_edge)
        d_edges = torch.from_numpy(edges).to(dev)
    gt_class, gt_rel = ground_truth(nodes, edges, instance2label, class_names, rel_json, relation_names, multi_rel_outputs)
    choice, counts = prep.sample_objects(d_inst, d_ids, num_points, seed, map_size=map_size)
    obj_points, descriptor = prep.prepare_objects(d_xyz, choice)
    if pts.shape[1] > 3:                 # colour / normal channels ride along with the same selection
        extra = torch.from_numpy(np.ascontiguousarray(pts[:, 3:], dtype=np.float32)).to(dev)
        obj_points = torch.cat([obj_points, extra[choice.long()].permute(0, 2, 1).contiguous()], 1)
    feats = np.zeros((len(nodes), 512), dtype=np.float32)
    if feature_loader is not None or multi_view_root is not None:
        for k, i in enumerate(nodes):
            name = instance2label[i]
            feats[k] = (feature_loader(i, name) if feature_loader is not None
                        else np.load(multi_view_feature_path(multi_view_root, scene_id, i, name)))
    n = len(nodes)
    batch = {"obj_points": obj_points, "obj_2d_feats": torch.from_numpy(feats).to(dev), "descriptor": descriptor,
             "edge_indices": d_edges,
             "batch_ids": torch.zeros(n, 1, dtype=torch.int64, device=dev),
             "gt_class": torch.from_numpy(gt_class).to(dev), "gt_rel_cls": torch.from_numpy(gt_rel).to(dev),
             "n_scenes": 1, "instance_ids": nodes, "points_per_instance": counts, "choice": choice}
    if proximity:
        batch["boxes"] = boxes
    elif all_edge:
        batch["fc_sizes"] = [n]
    return batch


def annotation_coverage(nodes: Sequence[int], edges: np.ndarray, rel_json: Sequence[Sequence]) -> Tuple[int, int]:
    """(kept, total): the annotated ordered pairs between the scene's ``nodes`` (instance ids, node order; distinct pairs, whatever
    number of relations a pair carries) that are present in ``edges`` (i64[E,2] node-index pairs), against all of them -- what a
    pruned edge list can still be right about; the number to tune ``padding`` and ``max_neighbors`` with."""
    pos = {n: k for k, n in enumerate(nodes)}
    annotated = {(pos[r[0]], pos[r[1]]) for r in rel_json if r[0] in pos and r[1] in pos}
    present = {(int(a), int(b)) for a, b in np.asarray(edges, dtype=np.int64).reshape(-1, 2)}
    return len(annotated & present), len(annotated)


# ---- scoring a segmentation of one's own: which predicted segment is which annotated object --------------------------------------------
def read_semseg(path_or_data) -> Dict[int, str]:
    """3RScan ``semseg.v2.json`` -> {objectId: label} from ``segGroups`` in the file's order, unmapped (the reference's ``load_semseg``
    without a label mapping, utils/util.py:44-61).  Mapping the names onto a class list is the caller's."""
    data = path_or_data
    if isinstance(path_or_data, (str, os.PathLike)):
        with open(path_or_data) as f:
            data = json.load(f)
    if "segGroups" not in data:
        raise ScanError("semseg: no segGroups")
    return {int(g["objectId"]): g["label"] for g in data["segGroups"]}


class LabelTransfer:
    """What ``transfer_labels`` found.  ``instance2label`` {segment id: label} (ascending segment id; what ``prepare_scan`` takes for the
    predicted mesh), ``segment_to_gt`` {segment id: annotated instance id}, ``gt_to_segments`` {instance id: [segment ids]} (instances
    in the order of their first segment), and per considered-or-not segment of ``segment_ids`` (ascending, 0 excluded) the arrays
    ``size``, ``best``, ``second``, ``n_candidates`` and ``matched_gt`` (instance id or -1); ``counts`` [S, len(gt_ids)] is the table
    they come from, ``n_without_correspondence`` the number of predicted points with no annotated point within the distance."""

    def __init__(self, **fields):
        self.__dict__.update(fields)

    def __repr__(self):
        return (f"LabelTransfer({len(self.segment_to_gt)} of {len(self.segment_ids)} segments matched to {len(self.gt_to_segments)} instances, "
                f"{self.n_without_correspondence} points without a correspondence)")


def transfer_labels(pd_mesh, gt_mesh, gt_instance2label: Dict[int, str], max_sq_dist: float = 0.1, min_seg_size: int = 512,
                    corr_thres: float = 0.5, occ_thres: float = 0.75, occ_min_candidates: int = 3, device="cuda:0") -> LabelTransfer:
    """Which annotated object is each segment of a predicted segmentation?  ``pd_mesh`` / ``gt_mesh``: a path or the dict of
    ``read_ply`` (``instances`` = the segment id per vertex of the predicted cloud, the annotators' instance id per vertex of the label
    mesh); ``gt_instance2label`` {instance id: label}, already mapped to the class list (``read_semseg`` gives the raw names); an
    instance that is absent or labelled ``'none'`` takes no part.

    The rule of the reference's data_processing/gen_data.py:196-349, stated in include/vlsat.h: every predicted point looks up its
    nearest annotated point (``prep.nearest_points``; ``max_sq_dist`` is a SQUARED distance, as the reference's ``--max_dist`` is
    compared with a squared distance), a segment with more than ``min_seg_size`` points takes the instance most of its points land on
    when that share is above ``corr_thres`` and the runner-up is below ``occ_thres`` of it (``prep.segment_overlap``, where
    ``occ_min_candidates`` is explained).  Segment 0 is background.  ``device=None`` (or "cpu") runs the numpy restatement, which gives
    the same result.  The reference program cannot be run here, so agreement with it is by reading."""
    import torch

    from . import prep

    pd = read_ply(pd_mesh) if isinstance(pd_mesh, (str, os.PathLike)) else pd_mesh
    gt = read_ply(gt_mesh) if isinstance(gt_mesh, (str, os.PathLike)) else gt_mesh
    pd_seg = np.asarray(pd["instances"]).astype(np.int64).reshape(-1)
    gt_inst = np.asarray(gt["instances"]).astype(np.int64).reshape(-1)
    segment_ids = np.unique(pd_seg)
    segment_ids = segment_ids[segment_ids != 0]
    gt_ids = np.asarray(sorted(int(i) for i, name in gt_instance2label.items() if name != "none"), dtype=np.int64)
    for ids in (segment_ids, gt_ids):
        if len(ids) and (ids.min() < 0 or ids.max() >= (1 << 24)):
            raise ScanError("segment and instance ids must be integers in [0, 2^24)")
    arrays = [np.ascontiguousarray(pd["points"][:, :3], dtype=np.float32), np.ascontiguousarray(gt["points"][:, :3], dtype=np.float32),
              np.clip(pd_seg, -1, 1 << 24).astype(np.int32), np.clip(gt_inst, -1, 1 << 24).astype(np.int32)]
    on_host = device is None or torch.device(device).type == "cpu"
    d_pd, d_gt, d_seg, d_inst = (torch.from_numpy(a) if on_host else torch.from_numpy(a).to(device) for a in arrays)
    nn_index, _ = prep.nearest_points(d_pd, d_gt, max_sq_dist)
    ov = prep.segment_overlap(d_seg, nn_index, d_inst, segment_ids, gt_ids, min_seg_size, corr_thres, occ_thres, occ_min_candidates)
    n_without = int((nn_index < 0).sum())
    ov = {k: v.cpu().numpy() for k, v in ov.items()}
    segment_to_gt, gt_to_segments, instance2label = {}, {}, {}
    for s, slot in zip(segment_ids, ov["match"]):
        if slot >= 0:
            g = int(gt_ids[slot])
            segment_to_gt[int(s)] = g
            gt_to_segments.setdefault(g, []).append(int(s))
            instance2label[int(s)] = gt_instance2label[g]
    matched = np.where(ov["match"] >= 0, gt_ids[np.maximum(ov["match"], 0)] if len(gt_ids) else -1, -1).astype(np.int64)
    return LabelTransfer(instance2label=instance2label, segment_to_gt=segment_to_gt, gt_to_segments=gt_to_segments,
                         segment_ids=segment_ids, gt_ids=gt_ids, size=ov["size"], best=ov["best"], second=ov["second"],
                         n_candidates=ov["n_candidates"], counts=ov["counts"], matched_gt=matched, n_without_correspondence=n_without)


def inherit_relationships(match, rel_json: Sequence[Sequence], relation_names: Sequence[str], same_part: str = "same part") -> List[list]:
    """The annotated relationships, carried over to the segments (gen_data.py:426-481) -> a ``rel_json`` for the predicted mesh.
    ``match``: a ``LabelTransfer`` (or its ``gt_to_segments``).  Every annotated ``[src, tgt, k, name]`` whose two instances both have
    accepted segments becomes one entry per (segment of src x segment of tgt), in the annotation's order; ``k`` is the name's index in
    ``relation_names`` and a name outside the list is dropped.  When ``same_part`` is in ``relation_names`` every ordered pair of
    distinct segments of one instance gets that relation; when it is not (the 26-name list), none is added -- the reference would
    raise there."""
    gt_to_segments = match if isinstance(match, dict) else match.gt_to_segments
    pos = {n: k for k, n in enumerate(relation_names)}
    out = []
    for r in rel_json:
        src, tgt, name = int(r[0]), int(r[1]), r[3]
        if name not in pos or src not in gt_to_segments or tgt not in gt_to_segments:
            continue
        out.extend([int(a), int(b), pos[name], name] for a in gt_to_segments[src] for b in gt_to_segments[tgt])
    if same_part in pos:
        for group in gt_to_segments.values():
            for i in range(len(group)):
                for j in range(i + 1, len(group)):
                    out.append([int(group[i]), int(group[j]), pos[same_part], same_part])
                    out.append([int(group[j]), int(group[i]), pos[same_part], same_part])
    return out



def merge_instances(instances: np.ndarray, instance_ids: Sequence[int], merged) -> np.ndarray:
    """The per-vertex object id of a merged label mesh: every vertex whose segment id is ``instance_ids[n]`` takes the id of the
    object segment n was merged into -- the instance id of that object's root segment (``scene_graph.merged_node_ids``); a vertex of
    any other segment (background, segments that are no node) keeps 0.  ``merged``: a one-scene ``metrics.MergedGraph``."""
    instances = np.asarray(instances).astype(np.int64).reshape(-1)
    ids = np.asarray(list(instance_ids), dtype=np.int64)
    root = np.asarray(merged.root.cpu() if hasattr(merged.root, "cpu") else merged.root).astype(np.int64).reshape(-1)
    if root.shape != ids.shape:
        raise ScanError("merge_instances: the graph's segments and instance_ids differ in length")
    out = np.zeros_like(instances)
    if not ids.size:
        return out
    order = np.argsort(ids, kind="stable")
    pos = np.clip(np.searchsorted(ids[order], instances), 0, ids.size - 1)
    hit = ids[order][pos] == instances
    out[hit] = ids[root[order[pos[hit]]]]
    return out


# ---- a scan split into the sub-scenes the models were trained on ---------------------------------------------------------------------
class ScanSplits:
    """What ``split_scan`` found.  ``groups``: the kept sub-scenes as lists of ascending instance ids; ``kept``: the seed number of each
    kept group; ``seeds`` int32 [K] / ``seed_points`` float32 [K,3]: the vertex index and position of EVERY seed, in creation order;
    ``counts`` int32 [K]: segments per seed's box (a group below ``min_seg_per_group`` is dropped, as the reference drops it)."""

    def __init__(self, **fields):
        self.__dict__.update(fields)

    def __iter__(self):                      # groups, seeds, seed_points = split_scan(...)
        return iter((self.groups, self.seeds, self.seed_points))

    def __repr__(self):
        return f"ScanSplits({len(self.groups)} groups kept of {len(self.seeds)} seeds, sizes {[len(g) for g in self.groups]})"


def split_scan(mesh_or_path, distance: float = 1.0, bbox_distance: float = 0.75, min_seg_per_group: int = 5, seed: int = 0,
               device="cuda:0", ranks=None) -> ScanSplits:
    """A scan split into sub-scenes as the reference's ``generate_groups`` splits it (data_processing/gen_data.py:56-183, BBOX method;
    every entry of its relationships_*.json is one such split): seed vertices more than ``distance`` apart in xy, drawn until no vertex
    is further than that from all of them, and per seed the segments with a vertex strictly inside the box ``seed -/+ bbox_distance``;
    a group of fewer than ``min_seg_per_group`` segments is dropped.  The rules are stated in include/vlsat_split.h; both steps run on
    the device (``prep.split_seeds`` / ``prep.split_groups``; ``device=None`` or "cpu": their numpy restatements, same result).  The
    draws come from the counter-based generator of ``prep.sample_objects`` under ``seed`` -- not numpy's stream -- or from ``ranks``
    (a recorded run: the rank of every seed among the selectable vertices).

    Like the reference's np.unique, a group lists id 0 (unlabelled vertices) when the box holds such a vertex.  Feed a group to
    ``prepare_scan`` as ``{i: instance2label[i] for i in group if i in instance2label}``: ids without a label are ignored there."""
    import torch

    from . import prep

    mesh = read_ply(mesh_or_path) if isinstance(mesh_or_path, (str, os.PathLike)) else mesh_or_path
    pts = np.ascontiguousarray(np.asarray(mesh["points"])[:, :3], dtype=np.float32)
    seg = np.asarray(mesh["instances"]).astype(np.int64).reshape(-1)
    if len(pts) < 1 or len(seg) != len(pts):
        raise ScanError("split_scan: the mesh needs at least one vertex and one segment id per vertex")
    segment_ids = np.unique(seg)
    if segment_ids.min() < 0 or segment_ids.max() >= (1 << 24):
        raise ScanError("segment ids must be integers in [0, 2^24)")
    on_host = device is None or torch.device(device).type == "cpu"
    d_pts = torch.from_numpy(pts) if on_host else torch.from_numpy(pts).to(device)
    d_seg = torch.from_numpy(seg.astype(np.int32)) if on_host else torch.from_numpy(seg.astype(np.int32)).to(device)
    seeds = prep.split_seeds(d_pts, distance, seed, ranks, max_seeds=None if on_host else prep.split_seed_cap(pts, distance))
    groups, counts, keep, _ = prep.split_groups(d_pts, d_seg, segment_ids, seeds, bbox_distance, min_seg_per_group)
    seeds = seeds.cpu().numpy().astype(np.int32)
    kept = [k for k in range(len(seeds)) if keep[k]]
    return ScanSplits(groups=[groups[k] for k in kept], kept=kept, seeds=seeds, seed_points=pts[seeds], counts=counts)


# ---- a bare mesh: faces, normals, and the segmentation every function above takes as given -------------------------------------------
def _ply_header(f, path):
    """-> (format, [[element name, count, [(property, dtype) | (property, (count dtype, item dtype)) for a list]]])"""
    if f.readline().strip() != b"ply":
        raise ScanError(f"{path}: not a PLY file")
    fmt, elements = None, []
    while True:
        line = f.readline()
        if not line:
            raise ScanError(f"{path}: header without end_header")
        tok = line.decode("ascii", "replace").split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append([tok[1], int(tok[2]), []])
        elif tok[0] == "property":
            if not elements:
                raise ScanError(f"{path}: property before any element")
            types = tok[2:4] if tok[1] == "list" else tok[1:2]
            if len(tok) < (5 if tok[1] == "list" else 3) or any(t not in _PLY_TYPES for t in types):
                raise ScanError(f"{path}: unknown property type in {' '.join(tok)!r}")
            elements[-1][2].append((tok[-1], tuple(_PLY_TYPES[t] for t in types) if tok[1] == "list" else _PLY_TYPES[types[0]]))
        elif tok[0] == "end_header":
            break
    if fmt not in ("ascii", "binary_little_endian"):
        raise ScanError(f"{path}: format {fmt!r} is not supported (ascii, binary_little_endian)")
    return fmt, elements


def _ply_rows(f, path, fmt, name, count, props):
    """One element -> {property: column}; a list property becomes an int64 [count, 3] table (every row must hold three entries)."""
    lists = [p for p, t in props if isinstance(t, tuple)]
    if len(lists) > 1:
        raise ScanError(f"{path}: element {name!r} has more than one list property")
    if fmt == "ascii":
        vals = b" ".join(f.readline() for _ in range(count)).split()
        width = len(props) + (3 if lists else 0)
        if len(vals) != count * width:
            raise ScanError(f"{path}: {name} rows do not hold {count} x {width} values" + (" (triangles only)" if lists else ""))
        try:
            table = np.array(vals, dtype=np.float64).reshape(count, width)
        except ValueError:
            raise ScanError(f"{path}: a {name} value is not a number") from None
        out, col = {}, 0
        for p, t in props:
            if isinstance(t, tuple):
                if count and not (table[:, col] == 3).all():
                    raise ScanError(f"{path}: a {name} row is not a triangle")
                out[p] = table[:, col + 1:col + 4].astype(np.int64)
                col += 4
            else:                          # parsed INTO the declared type, as read_ply does
                out[p] = table[:, col].astype(t) if t[0] == "f" else table[:, col].astype(np.int64).astype(t)
                col += 1
        return out
    fields = []                            # a list row as (count, three items): rows of another length fail the count check below
    for p, t in props:
        fields += [("#" + p, "<" + t[0]), (p, "<" + t[1], (3,))] if isinstance(t, tuple) else [(p, "<" + t)]
    dt = np.dtype(fields)
    raw = f.read(dt.itemsize * count)
    if len(raw) != dt.itemsize * count:
        raise ScanError(f"{path}: {name} data truncated" + (" (triangles only)" if lists else ""))
    rec = np.frombuffer(raw, dtype=dt, count=count)
    if lists and count and not (rec["#" + lists[0]] == 3).all():
        raise ScanError(f"{path}: a {name} row is not a triangle")
    return {p: (rec[p].astype(np.int64) if isinstance(t, tuple) else rec[p]) for p, t in props}


def read_mesh(path: str) -> Dict[str, Optional[np.ndarray]]:
    """``read_ply`` plus the triangles: -> {"points", "colors", "normals", "instances", "faces": i32[F,3]}.  ASCII and
    binary_little_endian; the face element's list property (``vertex_indices`` / ``vertex_index``, any integer count and index type:
    ``uchar`` / ``int`` is the usual pair) must hold triangles.  A file without a face element has F = 0.  A vertex element without
    ``objectId`` / ``label`` -- a plain reconstructed mesh -- is accepted: ``instances`` is all zeros, for ``segment_scan`` to fill."""
    with open(path, "rb") as f:
        fmt, elements = _ply_header(f, path)
        vert, faces = None, np.zeros((0, 3), dtype=np.int32)
        for name, count, props in elements:
            if name not in ("vertex", "face") and vert is not None and faces.size:
                break
            rows = _ply_rows(f, path, fmt, name, count, props)
            if name == "vertex":
                if any(isinstance(t, tuple) for _, t in props):
                    raise ScanError(f"{path}: list property inside the vertex element")
                vert = rows
            elif name == "face":
                lists = [p for p, t in props if isinstance(t, tuple)]
                if not lists:
                    raise ScanError(f"{path}: the face element has no list property")
                faces = rows[lists[0]]
    if vert is None:
        raise ScanError(f"{path}: no vertex element")
    for k in ("x", "y", "z"):
        if k not in vert:
            raise ScanError(f"{path}: vertex element has no {k}")
    n = len(vert["x"])
    if faces.size and (faces.min() < 0 or faces.max() >= n):
        raise ScanError(f"{path}: a face names a vertex outside [0, {n})")
    out = {"points": np.stack([vert["x"], vert["y"], vert["z"]], 1).astype(np.float64)}
    out["colors"] = (np.stack([vert["red"], vert["green"], vert["blue"]], 1).astype(np.uint8)
                     if all(k in vert for k in ("red", "green", "blue")) else None)
    out["normals"] = (np.stack([vert["nx"], vert["ny"], vert["nz"]], 1).astype(np.float64)
                      if all(k in vert for k in ("nx", "ny", "nz")) else None)
    lab = vert["objectId"] if "objectId" in vert else vert.get("label")
    out["instances"] = np.zeros(n, dtype=np.int64) if lab is None else np.asarray(lab).astype(np.int64).reshape(-1)
    out["faces"] = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    return out


def write_ply(path: str, mesh: Dict[str, Optional[np.ndarray]], ascii: bool = False) -> None:
    """A minimal PLY writer (binary_little_endian, or ASCII): float x y z, float nx ny nz when ``mesh["normals"]`` is there, int
    ``objectId`` from ``mesh["instances"]`` (zeros when absent) and, when ``mesh["faces"]`` holds any, ``property list uchar int
    vertex_indices`` -- enough to save a segmentation, view it, and read it back with ``read_ply`` / ``read_mesh`` /
    ``transfer_labels``.  Coordinates are stored as float32; ASCII prints them with nine significant digits, which reads back as the
    same float32."""
    pts = np.asarray(mesh["points"], dtype=np.float32).reshape(-1, 3)
    nrm = mesh.get("normals")
    cols = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    data = [pts[:, 0], pts[:, 1], pts[:, 2]]
    if nrm is not None:
        nrm = np.asarray(nrm, dtype=np.float32).reshape(-1, 3)
        if len(nrm) != len(pts):
            raise ScanError("write_ply: one normal per vertex")
        cols += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        data += [nrm[:, 0], nrm[:, 1], nrm[:, 2]]
    inst = mesh.get("instances")
    inst = np.zeros(len(pts), dtype=np.int64) if inst is None else np.asarray(inst).astype(np.int64).reshape(-1)
    if len(inst) != len(pts) or (len(inst) and (inst.min() < -(1 << 31) or inst.max() >= 1 << 31)):
        raise ScanError("write_ply: one int32 instance id per vertex")
    cols.append(("objectId", "<i4"))
    data.append(inst)
    faces = mesh.get("faces")
    faces = np.zeros((0, 3), np.int32) if faces is None else np.asarray(faces).astype(np.int32).reshape(-1, 3)
    header = ["ply", f"format {'ascii' if ascii else 'binary_little_endian'} 1.0", f"element vertex {len(pts)}"]
    header += [f"property {'int' if t == '<i4' else 'float'} {p}" for p, t in cols]
    if len(faces):
        header += [f"element face {len(faces)}", "property list uchar int vertex_indices"]
    header.append("end_header")
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        if ascii:
            for row in zip(*data):
                f.write((" ".join(str(int(x)) if isinstance(x, (int, np.integer)) else f"{float(x):.9g}" for x in row) + "\n").encode("ascii"))
            for a, b, c in faces.tolist():
                f.write(f"3 {a} {b} {c}\n".encode("ascii"))
            return
        rec = np.empty(len(pts), dtype=np.dtype(cols))
        for (p, _), col in zip(cols, data):
            rec[p] = col
        f.write(rec.tobytes())
        if len(faces):
            frec = np.empty(len(faces), dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
            frec["n"], frec["v"] = 3, faces
            f.write(frec.tobytes())


def vertex_normals(points: np.ndarray, faces: np.ndarray) -> np.ndarray:
    """Area-weighted vertex normals f64 [V,3], on the host in float64, for meshes that carry none: the sum over a vertex's triangles of
    (p1 - p0) x (p2 - p0) (twice the area times the face normal), normalised; a vertex of no triangle, or whose triangles cancel,
    gets (0, 0, 0) -- its edges then weigh 1, as a right angle does."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    faces = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    if faces.size and (faces.min() < 0 or faces.max() >= len(pts)):
        raise ScanError("vertex_normals: a face names a vertex outside the mesh")
    cross = np.cross(pts[faces[:, 1]] - pts[faces[:, 0]], pts[faces[:, 2]] - pts[faces[:, 0]])
    acc = np.zeros_like(pts)
    for k in range(3):
        np.add.at(acc, faces[:, k], cross)
    length = np.linalg.norm(acc, axis=1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(length > 0, acc / length, 0.0)


def segment_scan(mesh_or_path, max_angle_deg: float = 10.0, min_verts: int = 20, device="cuda:0") -> Dict[str, Optional[np.ndarray]]:
    """A bare mesh over-segmented into segments on the device: -> a copy of the mesh dict with ``instances`` filled (int64 [V]: 0 =
    dropped, else 1..S), ``n_segments`` = S and ``seg_size`` int32 [S].  ``mesh_or_path``: a PLY path (``read_mesh``) or a dict with
    ``points``, ``faces`` and optionally ``normals`` (absent or None: ``vertex_normals``).  Vertices joined by a mesh edge whose normals
    differ by at most ``max_angle_deg`` grow into regions; a region of fewer than ``min_verts`` vertices joins its most similar
    neighbour (``prep.segment_mesh``; the rule is stated in include/vlsat_segment.h).  ``max_weight = np.float32(1 - cos(angle))`` is
    computed once here, on the host.  ``device=None`` (or "cpu") runs the numpy restatement, which gives the same result.

    The result is an OVER-segmentation -- a flat wall, a table top and each of its sides come out as separate segments -- which is what
    ``merge_graph`` expects: feed it to ``prepare_scan(mesh, {i: "?" for i in range(1, S + 1)}, ["?"], [], relations, ...)``.  Both
    defaults are starting values, not tuned operating points: no scan data and no checkpoint is available to this project, so the
    accuracy of the rule on real reconstructions is unmeasured."""
    import math

    import torch

    from . import prep

    mesh = dict(read_mesh(mesh_or_path) if isinstance(mesh_or_path, (str, os.PathLike)) else mesh_or_path)
    faces = mesh.get("faces")
    if faces is None:
        raise ScanError("segment_scan: the mesh has no faces (prep.segment_mesh takes any edge list, for a cloud with kNN edges)")
    pts = np.asarray(mesh["points"])[:, :3]
    if not 1 <= len(pts) <= prep.SEG_MAX_VERTS:
        raise ScanError("segment_scan: 1 .. 2^24 vertices")
    faces = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    if faces.size and (faces.min() < 0 or faces.max() >= len(pts)):
        raise ScanError("segment_scan: a face names a vertex outside the mesh")
    normals = mesh.get("normals")
    if normals is None:
        normals = mesh["normals"] = vertex_normals(pts, faces)
    if not 0.0 <= float(max_angle_deg) <= 180.0:
        raise ScanError("segment_scan: max_angle_deg must be in [0, 180]")
    max_weight = np.float32(1.0 - math.cos(math.radians(float(max_angle_deg))))
    on_host = device is None or torch.device(device).type == "cpu"
    d_normals = torch.from_numpy(np.ascontiguousarray(np.asarray(normals)[:, :3], dtype=np.float32))
    d_edges = torch.from_numpy(prep.mesh_edges(faces))
    if not on_host:
        d_normals, d_edges = d_normals.to(device), d_edges.to(device)
    seg = prep.segment_mesh(d_normals, d_edges, float(max_weight), min_verts)      # trim=True: the one host wait
    mesh["instances"] = seg.labels.cpu().numpy().astype(np.int64)
    mesh["n_segments"] = int(seg.n_segments)
    mesh["seg_size"] = seg.seg_size.cpu().numpy()
    return mesh


def segment_cloud(cloud_or_path, radius: float, k: int = 16, max_angle_deg: float = 10.0, min_verts: int = 20, max_curvature: float = 0.02,
                  min_points: int = 5, viewpoint=None, device="cuda:0", recompute_normals: bool = False,
                  voxel: Optional[float] = None) -> Dict[str, Optional[np.ndarray]]:
    """A point cloud WITHOUT faces over-segmented into segments on the device: -> a copy of the dict with ``normals`` f64 [V,3],
    ``curvature`` f32 [V], ``instances`` (int64 [V]: 0 = dropped, else 1..S), ``n_segments`` = S and ``seg_size`` int32 [S] filled.
    ``cloud_or_path``: a PLY path (``read_mesh``) or a dict with ``points``; faces, if any, are ignored.

    ``radius`` has no default because none is free of units: it is the distance, in the cloud's units, within which two points count
    as neighbours -- about three times the sampling distance is a start.  ``max_sq_dist = np.float32(radius) ** 2`` is computed once
    here, on the host.  Every point gets its ``k`` nearest neighbours within ``radius`` (``prep.knn_points``), from them a normal and the
    surface variation ``curvature`` (``prep.cloud_normals``; fewer than ``min_points`` members: no normal), and the rule of
    ``segment_scan`` runs over the neighbour pairs (``prep.segment_cloud``; include/vlsat_cloud.h states all three).  Normals the cloud
    already carries are kept, and weighed with their sign, unless ``recompute_normals``; computed ones are turned towards ``viewpoint``
    (x, y, z) when there is one and weighed with their sign, else weighed by 1 - |dot|.

    The flatness mask: a point whose curvature exceeds ``max_curvature`` is handed to the segmenter with a zero normal.  It then weighs
    1 against everyone, links to nobody and is absorbed by a neighbouring segment (or by other such points).  Without it the normals
    of a neighbourhood estimate turn gradually across a crease, and a chain of small steps joins two faces.  The returned ``normals`` are
    the unmasked ones.

    ``device=None`` (or "cpu") runs the numpy restatements, which give the same result bit for bit.  The output goes straight into
    ``write_ply`` and ``prepare_scan``, as ``segment_scan``'s does.  ``k``, ``max_curvature`` and the angle are starting values, not
    tuned operating points: no scan data and no checkpoint is available to this project, so accuracy on real scans is unmeasured.

    ``voxel`` (default None: nothing changes): the cloud is first resampled on a grid of that edge (``downsample_cloud``, origin 0,
    ``min_count`` 1) and the RESAMPLED cloud is segmented -- for a cloud of uneven density, where the ``k`` nearest neighbours of a
    densely sampled point lie within the sensor noise.  ``radius``, ``k`` and ``min_verts`` then speak of resampled points (about
    three times ``voxel`` is a start for the radius).  The result is still the INPUT cloud: ``instances``, ``normals`` and ``curvature``
    are gathered through ``voxel_of_point`` (a point without a voxel: 0, a zero normal, +inf), ``n_segments`` is the segmenter's,
    ``seg_size`` is recounted over the input points, and ``resampled`` holds the ``downsample_cloud`` dict with the segmenter's
    fields filled in.  Normals the input carries are averaged per voxel and kept, as without ``voxel``."""
    import math

    import torch

    from . import prep

    cloud = dict(read_mesh(cloud_or_path) if isinstance(cloud_or_path, (str, os.PathLike)) else cloud_or_path)
    if voxel is not None:
        small = segment_cloud(downsample_cloud(cloud, voxel, device=device), radius, k, max_angle_deg, min_verts, max_curvature, min_points,
                              viewpoint, device, recompute_normals)
        of = small["voxel_of_point"].astype(np.int64)
        has, at = of >= 0, np.maximum(of, 0)
        cloud["instances"] = np.where(has, small["instances"][at], 0).astype(np.int64)
        cloud["normals"] = np.where(has[:, None], small["normals"][at], 0.0)
        cloud["curvature"] = np.where(has, small["curvature"][at], np.float32(np.inf)).astype(np.float32)
        cloud["n_segments"] = small["n_segments"]
        cloud["seg_size"] = np.bincount(cloud["instances"][cloud["instances"] > 0] - 1, minlength=small["n_segments"]).astype(np.int32)
        cloud["resampled"] = small
        return cloud
    pts = np.ascontiguousarray(np.asarray(cloud["points"])[:, :3], dtype=np.float32)
    if not 1 <= len(pts) <= prep.SEG_MAX_VERTS:
        raise ScanError("segment_cloud: 1 .. 2^24 points")
    if not float(radius) >= 0.0:
        raise ScanError("segment_cloud: radius must be >= 0")
    if not 0.0 <= float(max_angle_deg) <= 180.0:
        raise ScanError("segment_cloud: max_angle_deg must be in [0, 180]")
    max_sq_dist = float(np.float32(radius) ** 2)
    max_weight = np.float32(1.0 - math.cos(math.radians(float(max_angle_deg))))
    on_host = device is None or torch.device(device).type == "cpu"
    d_pts = torch.from_numpy(pts) if on_host else torch.from_numpy(pts).to(device)
    table = prep.knn_points(d_pts, k, max_sq_dist)
    normals, curvature = prep.cloud_normals(d_pts, table.index, table.count, min_points, viewpoint)
    given = cloud.get("normals")
    unsigned = viewpoint is None
    if given is not None and not recompute_normals:
        normals = torch.from_numpy(np.ascontiguousarray(np.asarray(given)[:, :3], dtype=np.float32)).to(normals.device)
        if len(normals) != len(pts):
            raise ScanError("segment_cloud: one normal per point")
        unsigned = False
    masked = torch.where((curvature > float(np.float32(max_curvature)))[:, None], torch.zeros_like(normals), normals)
    seg = prep.segment_cloud(masked, table.index, float(max_weight), min_verts, unsigned=unsigned)     # trim=True: the one host wait
    cloud["normals"] = normals.cpu().numpy().astype(np.float64)
    cloud["curvature"] = curvature.cpu().numpy()
    cloud["instances"] = seg.labels.cpu().numpy().astype(np.int64)
    cloud["n_segments"] = int(seg.n_segments)
    cloud["seg_size"] = seg.seg_size.cpu().numpy()
    return cloud


def downsample_cloud(cloud_or_path, voxel: float, origin=(0.0, 0.0, 0.0), min_count: int = 1, device="cuda:0") -> Dict[str, Optional[np.ndarray]]:
    """A point cloud resampled on a voxel grid on the device (``prep.voxel_downsample``; include/vlsat_voxel.h states the rule): -> the
    dict ``read_mesh`` returns and ``write_ply`` takes, one point per occupied cell of edge ``voxel`` that holds at least ``min_count``
    points, in the order in which the cells first occur in the input.  ``points`` f64 [M,3] are the cell means (float32 values),
    ``normals`` the normalised means and ``colors`` the rounded means where the input has them; ``instances``, and every other
    one-dimensional integer array of one entry per point, take the value at the cell's first point; ``faces`` are dropped.  Added:
    ``voxel_of_point`` int32 [V] (the resampled point each input point went into, -1 for none: a non-finite or out-of-range point, or
    a cell below ``min_count``), ``first_point`` int32 [M] and ``voxel_count`` int32 [M].  ``origin`` anchors the grid to the frame, not
    to the cloud, so two clouds in one frame share cells.  ``device=None`` (or "cpu") runs the numpy restatement, with equal bits."""
    import torch

    from . import prep

    cloud = dict(read_mesh(cloud_or_path) if isinstance(cloud_or_path, (str, os.PathLike)) else cloud_or_path)
    pts = np.ascontiguousarray(np.asarray(cloud["points"])[:, :3], dtype=np.float32)
    if not 1 <= len(pts) <= prep.SEG_MAX_VERTS:
        raise ScanError("downsample_cloud: 1 .. 2^24 points")
    nrm, col = cloud.get("normals"), cloud.get("colors")
    nrm = None if nrm is None else np.ascontiguousarray(np.asarray(nrm)[:, :3], dtype=np.float32)
    col = None if col is None else np.ascontiguousarray(np.asarray(col)[:, :3], dtype=np.uint8)
    if any(x is not None and len(x) != len(pts) for x in (nrm, col)):
        raise ScanError("downsample_cloud: one normal and one colour per point")
    on_host = device is None or torch.device(device).type == "cpu"
    put = lambda x: None if x is None else (torch.from_numpy(x) if on_host else torch.from_numpy(x).to(device))      # noqa: E731
    try:
        vc = prep.voxel_downsample(put(pts), voxel, origin, min_count, put(nrm), put(col))
    except prep.L.VlsatError as e:
        raise ScanError(f"downsample_cloud: {e}") from e
    get = lambda x: None if x is None else x.cpu().numpy()      # noqa: E731
    first = get(vc.first_point)
    out = {}
    for name, value in cloud.items():                          # every integer field of one entry per point: the value at the first point
        if name in ("points", "normals", "colors", "faces") or value is None or isinstance(value, (str, bytes, dict)):
            continue
        value = np.asarray(value)
        if value.dtype.kind in "iu" and value.shape == (len(pts),):
            out[name] = value[first]
    out["points"] = get(vc.points).astype(np.float64)
    out["colors"] = get(vc.colors)
    out["normals"] = None if vc.normals is None else get(vc.normals).astype(np.float64)
    out.setdefault("instances", np.zeros(len(first), dtype=np.int64))
    out["faces"] = np.zeros((0, 3), dtype=np.int32)
    out["voxel_of_point"] = get(vc.voxel_of_point)
    out["first_point"] = first
    out["voxel_count"] = get(vc.count)
    return out


def segment_objects(cloud_or_path, dist: float, cluster_radius: float, k: int = 16, n_hyp: int = 1024, max_planes: int = 8,
                    min_plane_share: float = 0.02, outside_frac: float = 0.01, min_points: int = 50, voxel: Optional[float] = None,
                    seed: int = 0, device="cuda:0", concavity_deg: Optional[float] = None, viewpoint=None,
                    normal_radius: Optional[float] = None, absorb_rounds: int = 8,
                    recompute_normals: bool = False) -> Dict[str, Optional[np.ndarray]]:
    """A point cloud segmented into OBJECT-level instances on the device, without a trained model: -> a copy of the dict with
    ``instances`` (int64 [V]: the structural planes are 1..P, the clusters P+1..P+S, 0 = dropped), ``n_planes`` = P, ``planes`` f32
    [P,4] = (nx, ny, nz, d), ``n_segments`` = P + S and ``seg_size`` int32 [P + S] filled.  ``cloud_or_path``: a PLY path
    (``read_mesh``) or a dict with ``points``; faces, if any, are ignored.

    First the room's structural planes -- floor, walls, ceiling -- are found and removed (``prep.cloud_planes``): a plane drawn through
    three points is structural when at least ``min_plane_share`` of the valid points lie within ``dist`` of it AND at most
    ``outside_frac`` of the remaining points lie on one of its sides, which is true of a floor and not of a table top;
    ``min_inliers = ceil(min_plane_share x valid points)``, ``outside_ppm = round(outside_frac x 10^6)``, ``n_hyp`` planes are tried
    per round.  Then the points no plane took are clustered by proximity (``prep.knn_points`` over THOSE points, ``k`` neighbours
    within ``cluster_radius``, then ``prep.cloud_clusters``); a cluster of fewer than ``min_points`` points is dropped.
    include/vlsat_objects.h states both rules.  ``dist`` and ``cluster_radius`` have no defaults because none is free of units: the
    sensor noise, and about one and a half times the sampling distance, are a start.

    ``voxel``: as in ``segment_cloud`` -- the cloud is resampled first (``downsample_cloud``, origin 0, ``min_count`` 1), the RESAMPLED
    cloud is segmented (all parameters then speak of resampled points) and ``instances`` are gathered back through
    ``voxel_of_point`` (a point without a voxel: 0); ``seg_size`` is recounted over the input points and ``resampled`` holds the small
    cloud's result.  ``device=None`` (or "cpu") runs the numpy restatements, which give the same result bit for bit.  The output goes
    straight into ``write_ply`` and ``prepare_scan``, as ``segment_scan``'s does.

    Objects that touch -- closer than ``cluster_radius`` -- come out as ONE cluster, and an object standing against a wall loses the
    points within ``dist`` of it to the wall.  Every default is a starting value, not a tuned operating point: no scan data and no
    checkpoint is available to this project, so accuracy on real scans is unmeasured.

    ``concavity_deg`` (default None: nothing changes, the same calls and the same outputs): the points no plane took are clustered by
    LOCAL CONVEXITY instead (``prep.convex_clusters``; include/vlsat_convex.h states the rule), which cuts bodies that touch where their
    surfaces meet in a concave junction -- a box on a table, a cupboard against a desk.  One table ``prep.knn_points(rest, k,
    normal_radius^2)`` serves the normals and the clusters, ``normal_radius`` defaulting to 2 x ``cluster_radius``; the link distance
    stays ``cluster_radius`` and the tolerance is sin(``concavity_deg``): 10 is a start.  Convexity needs ORIENTED normals: the ones the
    cloud carries are taken (normalised in fp32) unless there are none or ``recompute_normals``; then they are estimated over that
    table and turned towards ``viewpoint`` (x, y, z) (``prep.cloud_normals``).  With neither, ``ScanError``.  A point that lost its
    place at a concave junction is handed to the nearest cluster within ``absorb_rounds`` rings.  The result also carries ``concave``
    bool [V]: the points that showed concave evidence.  What this does NOT do: one viewpoint orients only the surfaces seen from it;
    bodies whose faces are coplanar and closer than ``cluster_radius`` can still merge; a patch of surface enclosed by concave
    junctions becomes a cluster of its own."""
    import math

    import torch

    from . import prep

    cloud = dict(read_mesh(cloud_or_path) if isinstance(cloud_or_path, (str, os.PathLike)) else cloud_or_path)
    if voxel is not None:
        small = segment_objects(downsample_cloud(cloud, voxel, device=device), dist, cluster_radius, k, n_hyp, max_planes, min_plane_share,
                                outside_frac, min_points, None, seed, device, concavity_deg, viewpoint, normal_radius, absorb_rounds,
                                recompute_normals)
        of = small["voxel_of_point"].astype(np.int64)
        cloud["instances"] = np.where(of >= 0, small["instances"][np.maximum(of, 0)], 0).astype(np.int64)
        cloud["n_planes"], cloud["planes"], cloud["n_segments"] = small["n_planes"], small["planes"], small["n_segments"]
        cloud["seg_size"] = np.bincount(cloud["instances"][cloud["instances"] > 0] - 1, minlength=small["n_segments"]).astype(np.int32)
        cloud["resampled"] = small
        if concavity_deg is not None:
            cloud["concave"] = (of >= 0) & small["concave"][np.maximum(of, 0)]
        return cloud
    pts = np.ascontiguousarray(np.asarray(cloud["points"])[:, :3], dtype=np.float32)
    if not 3 <= len(pts) <= prep.SEG_MAX_VERTS:
        raise ScanError("segment_objects: 3 .. 2^24 points")
    given = None
    if concavity_deg is not None:
        if not 0.0 <= float(concavity_deg) <= 90.0:
            raise ScanError("segment_objects: concavity_deg must be in [0, 90]")
        if normal_radius is not None and not float(normal_radius) >= 0.0:
            raise ScanError("segment_objects: normal_radius must be >= 0")
        given = None if recompute_normals else cloud.get("normals")
        if given is None and viewpoint is None:
            raise ScanError("segment_objects: convexity needs a side -- normals the cloud carries, or a viewpoint to turn estimated ones to")
        if given is not None:
            given = np.ascontiguousarray(np.asarray(given)[:, :3], dtype=np.float32)
            if len(given) != len(pts):
                raise ScanError("segment_objects: one normal per point")
    if not float(cluster_radius) >= 0.0:
        raise ScanError("segment_objects: cluster_radius must be >= 0")
    if not (0.0 < float(min_plane_share) <= 1.0 and 0.0 <= float(outside_frac) <= 0.5):
        raise ScanError("segment_objects: min_plane_share must be in (0, 1] and outside_frac in [0, 0.5]")
    n_valid = int(np.isfinite(pts).all(1).sum())
    min_inliers = max(3, int(math.ceil(float(min_plane_share) * n_valid)))
    outside_ppm = int(round(float(outside_frac) * 1e6))
    max_sq_dist = float(np.float32(cluster_radius) ** 2)
    on_host = device is None or torch.device(device).type == "cpu"
    d_pts = torch.from_numpy(pts) if on_host else torch.from_numpy(pts).to(device)
    try:
        found = prep.cloud_planes(d_pts, n_hyp, max_planes, dist, min_inliers, outside_ppm, seed)
    except prep.L.VlsatError as e:
        raise ScanError(f"segment_objects: {e}") from e
    n_planes = int(found.n_planes.reshape(-1)[0])                                    # the first host wait
    plane_id = found.plane_id.cpu().numpy().astype(np.int64)
    instances = plane_id.copy()
    rest = np.nonzero((plane_id == 0) & np.isfinite(pts).all(1))[0]
    sizes = [found.counts[:n_planes, 0].cpu().numpy().astype(np.int32)]
    n_clusters = 0
    if len(rest) and concavity_deg is not None:
        d_rest = d_pts[torch.from_numpy(rest).to(d_pts.device)]
        reach = 2.0 * float(cluster_radius) if normal_radius is None else float(normal_radius)
        table = prep.knn_points(d_rest, k, float(np.float32(reach) ** 2))
        if given is None:
            normals = prep.cloud_normals(d_rest, table.index, table.count, viewpoint=viewpoint)[0]
        else:
            with np.errstate(all="ignore"):
                g = given[rest]
                normals = torch.from_numpy(g / np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])[:, None]).to(d_pts.device)
        mask = torch.ones(len(rest), dtype=torch.int32, device=d_pts.device)
        try:
            grown = prep.convex_clusters(d_rest, normals, table.index, table.sqdist, mask, max_sq_dist,
                                         float(np.float32(math.sin(math.radians(float(concavity_deg))))), min_points, absorb_rounds)
        except prep.L.VlsatError as e:
            raise ScanError(f"segment_objects: {e}") from e
        n_clusters = int(grown.n_clusters.reshape(-1)[0])
        labels = grown.labels.cpu().numpy().astype(np.int64)
        instances[rest] = np.where(labels > 0, labels + n_planes, 0)
        sizes.append(grown.cluster_size[:n_clusters].cpu().numpy().astype(np.int32))
        cloud["concave"] = np.zeros(len(pts), dtype=bool)
        cloud["concave"][rest] = grown.state.cpu().numpy() == 2
    elif len(rest):
        d_rest = d_pts[torch.from_numpy(rest).to(d_pts.device)]
        table = prep.knn_points(d_rest, k, max_sq_dist)
        mask = torch.ones(len(rest), dtype=torch.int32, device=d_pts.device)
        grown = prep.cloud_clusters(table.index, table.sqdist, mask, max_sq_dist, min_points)
        n_clusters = int(grown.n_clusters.reshape(-1)[0])
        labels = grown.labels.cpu().numpy().astype(np.int64)
        instances[rest] = np.where(labels > 0, labels + n_planes, 0)
        sizes.append(grown.cluster_size[:n_clusters].cpu().numpy().astype(np.int32))
    if concavity_deg is not None and not len(rest):
        cloud["concave"] = np.zeros(len(pts), dtype=bool)
    cloud["instances"] = instances
    cloud["n_planes"] = n_planes
    cloud["planes"] = found.planes[:n_planes].cpu().numpy()
    cloud["n_segments"] = n_planes + n_clusters
    cloud["seg_size"] = np.concatenate(sizes)
    return cloud
