"""The predicted scene graph as labelled records: what ``VLSATModel.predict_graph`` / ``metrics.scene_graph_topk`` return
(class and edge indices on the device) turned into instance ids and names, and written as JSON; and the decoded graph
(``VLSATModel.decode_graph`` / ``metrics.decode_graph``) written in the dataset's own annotation layout."""
from __future__ import annotations

import json
from typing import Dict, List, Sequence


def to_records(graph, scene: int, edges, node_ids: Sequence[int], class_names: Sequence[str],
               relation_names: Sequence[str]) -> List[dict]:
    """Rows of scene ``scene`` of a ``metrics.SceneGraph`` in rank order:
    ``{"subject": instance id, "subject_label", "object": instance id, "object_label", "predicate", "score"}``.
    ``edges`` is the [E, 2] (from, to) list the graph's edge rows index, ``node_ids[n]`` the instance id of node n
    (``scan.prepare_scan``'s ``instance_ids``).  ``relation_names`` are the names of the model's predicate classes: for a
    multi-label model ``relationships.txt`` without its first line ``none`` (the reference drops it, dataset_3dssg.py:95-96);
    a single-label model keeps ``none`` as class 0 and reports it like any other predicate.  Labels of a ``rels`` graph
    (classes -1) are None.  Reads the scene's rows back from the device."""
    n = int(graph.n_valid[scene])
    rows = [t[scene, :n].tolist() for t in (graph.edge, graph.sub_cls, graph.obj_cls, graph.pred, graph.score)]
    edges = edges.tolist() if hasattr(edges, "tolist") else list(edges)
    out = []
    for e, sc, oc, p, v in zip(*rows):
        a, b = edges[e]
        if not 0 <= p < len(relation_names) or max(sc, oc) >= len(class_names):
            raise ValueError("to_records: class index outside the name lists")
        out.append({"subject": int(node_ids[a]), "subject_label": class_names[sc] if sc >= 0 else None,
                    "object": int(node_ids[b]), "object_label": class_names[oc] if oc >= 0 else None,
                    "predicate": relation_names[p], "score": float(v)})
    return out


def to_annotation(graph, scene: int, edges, node_ids: Sequence[int], class_names: Sequence[str],
                  relation_names_full: Sequence[str], scan: str, split: int = 0, multi_rel_outputs: bool = True) -> dict:
    """Scene ``scene`` of a ``metrics.DecodedGraph`` as one entry of the dataset's ``relationships*.json``:
    ``{"scan", "split", "objects": {instance id: top-1 label}, "relationships": [[subject id, object id, index in
    relation_names_full, name], ...]}`` in the graph's rank order -- what ``scan.read_relationships`` (and the reference's own
    loader) reads back unchanged.  ``edges`` is the [E, 2] list the graph's edge rows index and ``node_ids[n]`` the instance id of
    the scene's node n (``scan.prepare_scan``'s ``instance_ids``); the graph's node tables must be the scene's own (one-scene
    call, or ``DecodedGraph.scene(s, offset, nodes)``).  ``relation_names_full`` is ``relationships.txt`` INCLUDING its first
    line ``none``: the predicate k of a multi-label model is ``relation_names_full[k + 1]`` (the reference drops the leading
    ``none``, dataset_3dssg.py:95-96); a single-label model's k indexes the list directly (0 = none is never asserted).  Reads the
    scene's rows back from the device."""
    n = int(graph.n_valid[scene])
    if graph.labels.shape[0] != len(node_ids):
        raise ValueError("to_annotation: the graph's node tables and node_ids differ in length")
    edges = edges.tolist() if hasattr(edges, "tolist") else list(edges)
    top1 = graph.labels[:, 0].tolist()
    if top1 and max(top1) >= len(class_names):
        raise ValueError("to_annotation: class index outside the name list")
    shift = 1 if multi_rel_outputs else 0
    rels = []
    for e, p in zip(graph.edge[scene, :n].tolist(), graph.pred[scene, :n].tolist()):
        a, b = edges[e]
        if not 0 <= p + shift < len(relation_names_full):
            raise ValueError("to_annotation: predicate index outside the name list")
        rels.append([int(node_ids[a]), int(node_ids[b]), p + shift, relation_names_full[p + shift]])
    return {"scan": str(scan), "split": int(split), "objects": {str(int(i)): class_names[c] for i, c in zip(node_ids, top1)},
            "relationships": rels}


def merged_node_ids(merged, instance_ids: Sequence[int]) -> List[int]:
    """The ids of the objects of a one-scene ``metrics.MergedGraph``: an object is named by the instance id of its root segment
    (``instance_ids[n]`` = the id of segment row n, ``scan.prepare_scan``'s ``instance_ids``).  What ``to_annotation`` takes as
    ``node_ids`` with ``merged.decode()`` and ``merged.pair_edges``."""
    ptr, members = merged.member_ptr.tolist(), merged.members.tolist()
    if len(members) != len(instance_ids):
        raise ValueError("merged_node_ids: the graph's segments and instance_ids differ in length")
    return [int(instance_ids[members[ptr[o]]]) for o in range(int(merged.totals[0]))]


def add_segments(entry: dict, merged, instance_ids: Sequence[int]) -> dict:
    """Writes ``"segments": {object id: [segment ids]}`` (members in ascending row) into an annotation entry of a one-scene
    ``metrics.MergedGraph`` and returns the entry."""
    ptr, members = merged.member_ptr.tolist(), merged.members.tolist()
    ids = merged_node_ids(merged, instance_ids)
    entry["segments"] = {str(ids[o]): [int(instance_ids[n]) for n in members[ptr[o]:ptr[o + 1]]] for o in range(len(ids))}
    return entry


def write_annotations(path, entries) -> None:
    """``{"scans": [entries]}``: the layout of ``relationships_{train,validation}.json``."""
    with open(path, "w") as f:
        json.dump({"scans": list(entries)}, f, indent=1)


def write_json(path, graphs: Dict[str, List[dict]]) -> None:
    """``{scan_id: records}`` as one JSON document (scores are fp32 values: they read back exactly)."""
    with open(path, "w") as f:
        json.dump({"scans": {str(k): v for k, v in graphs.items()}}, f, indent=1)


def read_json(path) -> Dict[str, List[dict]]:
    with open(path) as f:
        return json.load(f)["scans"]
