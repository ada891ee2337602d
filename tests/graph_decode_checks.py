"""Helpers shared by the decoded-graph tests (not a test module): the fixtures' cases, a brute-force numpy statement of the decode
that shares no code with metrics.decode_graph_host, and a field-by-field comparison."""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SG_GOLD = os.path.join(ROOT, "tests", "golden", "scene_graph_cases.npz")
METRICS_GOLD = os.path.join(ROOT, "tests", "golden", "metrics_small.npz")
FIELDS = ("labels", "label_probs", "edge", "pred", "score", "n_valid", "n_total")


def case(z, i, br):
    """(obj logits, rel output, edges, obj probs, multi, predicate probabilities) of case i of scene_graph_cases.npz, CPU tensors;
    the probabilities are the reference's own (its softmax; its np.exp for a single-label case)."""
    t = lambda k: torch.from_numpy(z[f"c{i}_{k}"])
    multi = bool(z[f"c{i}_multi"])
    rel = t(f"rel_{br}")
    return t(f"obj_logits_{br}"), rel, t("edges"), t(f"probs_{br}"), multi, (rel if multi else t(f"relp_{br}"))


def brute(probs, rp, edges, scene, n_scenes, thr, multi, score, n_labels, max_rel):
    """The decode as nested Python loops over numpy fp32 scalars -> dict of numpy arrays named like DecodedGraph's fields."""
    probs, rp, edges = np.asarray(probs, np.float32), np.asarray(rp, np.float32), np.asarray(edges, np.int64).reshape(-1, 2)
    n, c = probs.shape
    e, r = rp.shape
    thr = np.broadcast_to(np.asarray(thr, np.float32), (r,))
    labels, lp = np.zeros((n, n_labels), np.int32), np.zeros((n, n_labels), np.float32)
    for i in range(n):
        order = sorted(range(c), key=lambda k: (-float(probs[i, k]), k))[:n_labels]
        labels[i], lp[i] = order, probs[i, order]
    rows = [[] for _ in range(n_scenes)]
    for j in range(e):
        if multi:
            ks = [k for k in range(r) if rp[j, k] >= thr[k]]
        else:
            best = min(k for k in range(r) if rp[j, k] == rp[j].max())
            ks = [best] if best != 0 and rp[j, best] >= thr[best] else []
        for k in ks:
            v = rp[j, k]
            if score == "triplet":
                v = np.float32(np.float32(lp[edges[j, 0], 0] * lp[edges[j, 1], 0]) * rp[j, k])
            rows[int(scene[j])].append((-float(v), j, k, v))
    out = {"labels": labels, "label_probs": lp, "edge": np.full((n_scenes, max_rel), -1, np.int32),
           "pred": np.full((n_scenes, max_rel), -1, np.int32), "score": np.zeros((n_scenes, max_rel), np.float32),
           "n_valid": np.zeros(n_scenes, np.int32), "n_total": np.zeros(n_scenes, np.int32)}
    for s in range(n_scenes):
        keep = sorted(rows[s])[:max_rel]
        out["n_total"][s], out["n_valid"][s] = len(rows[s]), len(keep)
        for q, (_, j, k, v) in enumerate(keep):
            out["edge"][s, q], out["pred"][s, q], out["score"][s, q] = j, k, v
    return out


def assert_equal(got, want, what=""):
    """Every field of two decoded graphs (DecodedGraph or brute()'s dict), bit for bit: fp32 fields compared as their bits."""
    for f in FIELDS:
        a, b = (x[f] if isinstance(x, dict) else getattr(x, f) for x in (got, want))
        a, b = (np.ascontiguousarray(x.cpu().numpy() if torch.is_tensor(x) else x) for x in (a, b))
        assert a.shape == b.shape and a.dtype == b.dtype, (what, f, a.shape, b.shape, a.dtype, b.dtype)
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        np.testing.assert_array_equal(a, b, err_msg=f"{what}: {f}")


def indicator(g, s, e, r):
    """bool [e, r]: the (edge, predicate) pairs scene s of a decoded graph keeps."""
    n = int(g.n_valid[s])
    hot = torch.zeros(e, r, dtype=torch.bool)
    hot[g.edge[s, :n].long().cpu(), g.pred[s, :n].long().cpu()] = True
    return hot
