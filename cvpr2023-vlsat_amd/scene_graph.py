"""The predicted scene graph as labelled records: what ``VLSATModel.predict_graph`` / ``metrics.scene_graph_topk`` return
(class and edge indices on the device) turned into instance ids and names, and written as JSON."""
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


def write_json(path, graphs: Dict[str, List[dict]]) -> None:
    """``{scan_id: records}`` as one JSON document (scores are fp32 values: they read back exactly)."""
    with open(path, "w") as f:
        json.dump({"scans": {str(k): v for k, v in graphs.items()}}, f, indent=1)


def read_json(path) -> Dict[str, List[dict]]:
    with open(path) as f:
        return json.load(f)["scans"]
