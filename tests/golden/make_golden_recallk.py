#!/usr/bin/env python3
"""Golden vectors for the scene-graph Recall@K / mR@K of the reference (src/utils/eval_utils_recall.py:
evaluate_triplet_recallk / evaluate_triplet_mrecallk, called per scene by process_val2 / process_val3 of
src/model/SGFN_MMG/model_in21k.py:439-500), with get_gt of src/utils/eva_utils_acc.py, called directly (the modules import
only numpy / torch).  Every scene is run through the four variants (PredCls / SGCls, topk_each 1 / 100) on the inputs of
both branches (3D and 2D logits).  Inputs are small and stored with the outputs in recallk_cases.npz.

The counting kernels resolve ties at the K boundary optimistically (include/vlsat.h); the reference's order among equal
scores is torch.topk's.  The generator therefore asserts that no case has a tie -- or a near-tie a last-bit difference of the
softmax could flip -- at any K boundary or between an edge's best correct entry and its maximum."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
from src.utils import eva_utils_acc as A  # noqa: E402
from src.utils import eval_utils_recall as RR  # noqa: E402

C, K_LIST = 160, [20, 50, 100]
VARIANTS = (("predcls_gc", "rels", 1), ("predcls_ngc", "rels", 100), ("sgcls_gc", "triplet", 1), ("sgcls_ngc", "triplet", 100))
GAP = 1e-6                      # relative margin required at every decision boundary


def candidates(obj_logits, rel, edges, multi, evaluate, topk_each):
    """Per edge its topk_each largest entries (values, computed as the reference does), the object and predicate probabilities."""
    probs = torch.softmax(obj_logits, -1)
    r = rel if multi else torch.as_tensor(np.exp(rel))
    out = []
    for e in range(len(edges)):
        if evaluate == "triplet":
            m = torch.einsum("nl,m->nlm", torch.einsum("n,m->nm", probs[edges[e][0]], probs[edges[e][1]]), r[e]).reshape(-1)
        else:
            m = r[e]
        out.append(m.topk(min(topk_each, m.shape[0])).values)
    return out, probs, r


def check_margins(obj_logits, rel, gt_cls, gt_rel, edges, multi):
    hot = gt_rel == 1 if multi else torch.nn.functional.one_hot(gt_rel.long(), rel.shape[1]).bool() & (gt_rel[:, None] > 0)
    for name, evaluate, each in VARIANTS:
        cand, probs, r = candidates(obj_logits, rel, edges, multi, evaluate, each)
        allc = torch.cat(cand).sort(descending=True).values
        for k in K_LIST:
            if allc.numel() > k:
                a, b = float(allc[k - 1]), float(allc[k])
                assert a - b > GAP * a, (name, k, a, b)
        if each == 1:                 # the GC check compares an edge's best correct entry with its maximum
            for e in range(len(edges)):
                if not hot[e].any():
                    continue
                if evaluate == "triplet":
                    corr = (probs[edges[e][0], gt_cls[edges[e][0]]] * probs[edges[e][1], gt_cls[edges[e][1]]]) * r[e][hot[e]]
                else:
                    corr = r[e][hot[e]]
                g, m = float(corr.max()), float(cand[e][0])
                assert g == m or m - g > GAP * m, (name, e, g, m)


def make_case(seed, n, n_edges, multi, no_gt=False, Rn=26, sharp=5.0):
    g = torch.Generator().manual_seed(seed)
    gt_cls = torch.randint(0, C, (n,), generator=g)
    pairs = [(a, b) for a in range(n) for b in range(n) if a != b]
    pick = torch.randperm(len(pairs), generator=g)[:n_edges].tolist()
    edges = torch.tensor([pairs[i] for i in sorted(pick)], dtype=torch.long)
    E = edges.shape[0]
    case = {"edges": edges.numpy(), "gt_cls": gt_cls.numpy(), "multi": np.array(int(multi))}
    if multi:
        gt_rel = torch.zeros(E, Rn, dtype=torch.long)
        if not no_gt:
            for e in range(E):
                k = int(torch.randint(0, 4, (1,), generator=g))
                if k:
                    gt_rel[e, torch.randperm(Rn, generator=g)[:k]] = 1
    else:
        gt_rel = torch.randint(0, Rn, (E,), generator=g)
        gt_rel[torch.rand(E, generator=g) < 0.3] = 0
    case["gt_rel"] = gt_rel.numpy()
    for br in ("3d", "2d"):
        obj_logits = torch.randn(n, C, generator=g) * sharp
        right = torch.rand(n, generator=g) < 0.6            # sharp and often right: hits fall at several K
        obj_logits[right, gt_cls[right]] += 4 * sharp
        z = torch.randn(E, Rn, generator=g) * 1.5
        if multi:
            hot = gt_rel == 1
            z = z + hot * (torch.rand(E, Rn, generator=g) * 4)
            rel = torch.sigmoid(z)
        else:
            z[torch.arange(E), gt_rel] += torch.rand(E, generator=g) * 4
            rel = torch.log_softmax(z, -1)
        check_margins(obj_logits, rel, gt_cls, gt_rel, edges, multi)
        gt_edges = A.get_gt(gt_cls, gt_rel, edges, multi)
        case[f"obj_logits_{br}"] = obj_logits.numpy()
        case[f"rel_{br}"] = rel.numpy()
        for name, evaluate, each in VARIANTS:
            with np.errstate(invalid="ignore", divide="ignore"):
                rec = RR.evaluate_triplet_recallk(obj_logits, rel, gt_edges, edges, multi, K_LIST, each, use_clip=True,
                                                  evaluate=evaluate)
            mrec = RR.evaluate_triplet_mrecallk(obj_logits, rel, gt_edges, edges, multi, K_LIST, each, use_clip=True,
                                                evaluate=evaluate)
            case[f"R_{name}_{br}"] = np.asarray(rec, dtype=np.float64)
            case[f"mR_{name}_{br}"] = np.array([[float(x) for x in row] for row in mrec], dtype=np.float64)
    return case


def main():
    specs = [  # (seed, objects, edges, multi-label, no gt edge)
        (11, 8, 15, True, False),       # E < 20
        (12, 12, 132, True, False),
        (13, 25, 600, True, False),     # >= 600 edges
        (14, 6, 30, True, True),        # no gt edge: recall NaN, mR all -1
        (15, 10, 90, False, False),     # single-label (log-probabilities, 0 = none)
        (16, 15, 150, False, False),
        (17, 9, 72, True, False),
    ]
    out = {}
    for i, (seed, n, e, multi, no_gt) in enumerate(specs):
        for attempt in range(50):            # the first seed of the series whose case has clear margins everywhere
            try:
                case = make_case(seed + 1000 * attempt, n, e, multi, no_gt)
                break
            except AssertionError as ex:
                print("  seed", seed + 1000 * attempt, "has a near-tie:", ex)
        else:
            raise RuntimeError(f"no case without near-ties for {seed}")
        for k, v in case.items():
            out[f"c{i}_{k}"] = v
        print("case", i, "nodes", n, "edges", e, "multi", multi, "sgcls_ngc 3d", out[f"c{i}_R_sgcls_ngc_3d"])
    out["n_cases"] = np.array(len(specs))
    path = os.path.join(HERE, "recallk_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
