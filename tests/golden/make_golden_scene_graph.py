#!/usr/bin/env python3
"""Golden vectors for the predicted scene graph: the list ``pred_triplets = ((from, to), (sub cls, obj cls, rel), conf)`` and
the kept scores ``all_topk_conf_matrix`` that the reference's evaluate_triplet_recallk (src/utils/eval_utils_recall.py) builds
and does not return.  The function is called as it is, on the seven scenes of recallk_cases.npz (both branches), for
(triplet, topk_each 1), (triplet, 100), (rels, 1), (rels, 100) with topk = [20, 50, 100]; a profile hook reads its locals
``pred_triplets``, ``all_topk_conf_matrix``, ``objs_pred`` (its F.softmax output) and ``rels_pred`` (its np.exp of a single-label
model's log-probabilities) from the frame when it returns.

    python tests/golden/make_golden_scene_graph.py <reference checkout>      (or VLSAT_REFERENCE=<reference checkout>)

Which of several equal candidates is kept is torch.topk's choice in the reference and unspecified in the library
(include/vlsat.h), so the generator asserts that consecutive kept scores, the last kept one and the next candidate, and -- for an
edge whose topk_each-th entry is kept -- that entry and the edge's next one differ by more than the relative GAP of
make_golden_recallk.py.  A scene of recallk_cases.npz that fails is replaced by the next seed of that script's series
(make_case(seed + 1000 * attempt)) that passes both scripts' margins; scene_graph_cases.npz therefore stores its own inputs
(same names as recallk_cases.npz) next to the outputs, and ``from_recallk`` says which scenes are the stored ones."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("VLSAT_REFERENCE", "")
if not REF:
    sys.exit(__doc__)
sys.path.insert(0, REF)
sys.path.insert(1, HERE)
from src.utils import eva_utils_acc as A  # noqa: E402
from src.utils import eval_utils_recall as RR  # noqa: E402
import make_golden_recallk as G  # noqa: E402  (make_case: the recipe and the seed series of recallk_cases.npz)

K_LIST = [20, 50, 100]
VARIANTS = (("triplet", 1), ("triplet", 100), ("rels", 1), ("rels", 100))
GAP = 1e-6                      # relative margin required at every decision boundary (make_golden_recallk.py)


def run_reference(obj_logits, rel, gt_edges, edges, multi, evaluate, each):
    """evaluate_triplet_recallk's return value and its locals at the return."""
    seen = {}

    def hook(frame, event, arg):
        if event == "return" and frame.f_code is RR.evaluate_triplet_recallk.__code__:
            loc = frame.f_locals
            for k in ("pred_triplets", "all_topk_conf_matrix", "objs_pred", "rels_pred"):
                seen[k] = loc[k]

    sys.setprofile(hook)
    try:
        with np.errstate(invalid="ignore", divide="ignore"):
            rec = RR.evaluate_triplet_recallk(obj_logits, rel, gt_edges, edges, multi, K_LIST, each, use_clip=True, evaluate=evaluate)
    finally:
        sys.setprofile(None)
    if set(seen) != {"pred_triplets", "all_topk_conf_matrix", "objs_pred", "rels_pred"}:
        raise RuntimeError("the profile hook did not see the reference's locals")
    return rec, seen


def check_margins(probs, r, edges, evaluate, each, kept):
    """Gaps between consecutive kept scores, to the next candidate, and below an edge's topk_each-th entry when it is kept."""
    kept = kept.double()
    if kept.numel() > 1:
        d = kept[:-1] - kept[1:]
        assert bool((d > GAP * kept[:-1]).all()), ("kept", evaluate, each, float(d.min()))
    last = float(kept[-1])
    cand = []
    for e in range(len(edges)):
        if evaluate == "triplet":
            m = torch.einsum("nl,m->nlm", torch.einsum("n,m->nm", probs[edges[e][0]], probs[edges[e][1]]), r[e]).reshape(-1)
        else:
            m = r[e]
        top = m.topk(min(each + 1, m.shape[0])).values
        cand.append(top[:each])
        if top.numel() > each and float(top[each - 1]) >= last:
            a, b = float(top[each - 1]), float(top[each])
            assert a - b > GAP * a, ("edge boundary", evaluate, each, e, a, b)
    allc = torch.cat(cand).sort(descending=True).values
    assert torch.equal(allc[:kept.numel()].double(), kept), "the kept scores are not the largest candidates"
    if allc.numel() > kept.numel():
        nxt = float(allc[kept.numel()])
        assert last - nxt > GAP * last, ("next candidate", evaluate, each, last, nxt)


SPECS = [(11, 8, 15, True, False), (12, 12, 132, True, False), (13, 25, 600, True, False), (14, 6, 30, True, True),
         (15, 10, 90, False, False), (16, 15, 150, False, False), (17, 9, 72, True, False)]     # make_golden_recallk.main's


def graphs_of(case):
    """The reference's lists for one scene (raises AssertionError on a near-tie)."""
    multi = bool(case["multi"])
    edges = torch.from_numpy(case["edges"])
    gt_cls, gt_rel = torch.from_numpy(case["gt_cls"]), torch.from_numpy(case["gt_rel"])
    gt_edges = A.get_gt(gt_cls, gt_rel, edges, multi)
    out = {}
    for br in ("3d", "2d"):
        obj_logits, rel = torch.from_numpy(case[f"obj_logits_{br}"]), torch.from_numpy(case[f"rel_{br}"])
        for evaluate, each in VARIANTS:
            rec, seen = run_reference(obj_logits, rel, gt_edges, edges, multi, evaluate, each)
            probs = torch.as_tensor(seen["objs_pred"])
            r = rel if multi else torch.as_tensor(np.exp(rel))
            kept = torch.as_tensor(seen["all_topk_conf_matrix"]).float()
            check_margins(probs, r, edges, evaluate, each, kept)
            rows = [[int(t[0][0]), int(t[0][1]), int(t[1][0]), int(t[1][1]), int(t[1][2])] for t in seen["pred_triplets"]]
            assert len(rows) == kept.numel()
            if evaluate == "triplet":             # the tuples carry the score; in rels mode they do not
                assert [float(t[2]) for t in seen["pred_triplets"]] == kept.tolist()
            key = f"{evaluate}_{each}_{br}"
            out[key + "_rows"] = np.asarray(rows, dtype=np.int32).reshape(-1, 5)
            out[key + "_score"] = kept.numpy()
            out[key + "_recall"] = np.asarray(rec, dtype=np.float64)
            out[f"probs_{br}"] = probs.numpy()
            if not multi:                         # the reference's np.exp of the log-probabilities
                out[f"relp_{br}"] = np.asarray(seen["rels_pred"], dtype=np.float32)
    return out


class _NoReference:
    """Stands in for the reference module while a seed is only screened for near-ties (make_case's own margins and the ones
    above need no reference run); the accepted seed then goes through the real functions."""
    @staticmethod
    def evaluate_triplet_recallk(*a, **k):
        return np.zeros(len(K_LIST))

    @staticmethod
    def evaluate_triplet_mrecallk(*a, **k):
        return [[0.0] * len(K_LIST) for _ in range(26)]


def screen(args):
    """Does this seed of the series pass both scripts' margins?  (Pure tensor arithmetic: run in worker processes.)"""
    seed, n, e, multi, no_gt = args
    torch.set_num_threads(1)
    real, G.RR = G.RR, _NoReference
    try:
        case = G.make_case(seed, n, e, multi, no_gt)
        edges = torch.from_numpy(case["edges"])
        for br in ("3d", "2d"):
            probs = torch.softmax(torch.from_numpy(case[f"obj_logits_{br}"]), -1)
            rel = torch.from_numpy(case[f"rel_{br}"])
            r = rel if multi else torch.as_tensor(np.exp(rel))
            for evaluate, each in VARIANTS:
                cand, _, _ = G.candidates(torch.from_numpy(case[f"obj_logits_{br}"]), rel, edges, multi, evaluate, each)
                kept = torch.cat(cand).sort(descending=True).values[:max(K_LIST)]
                check_margins(probs, r, edges, evaluate, each, kept)
        return seed, ""
    except AssertionError as ex:
        return seed, str(ex)
    finally:
        G.RR = real


def main():
    import multiprocessing as mp
    z = np.load(os.path.join(HERE, "recallk_cases.npz"))
    out, stored = {"n_cases": np.array(len(SPECS))}, []
    workers = min(8, os.cpu_count() or 1)
    with mp.get_context("fork").Pool(workers) as pool:
        for i, (seed, n, e, multi, no_gt) in enumerate(SPECS):
            good = None
            for a0 in range(0, 50, workers):              # the first seed of make_golden_recallk's series that passes
                res = pool.map(screen, [(seed + 1000 * a, n, e, multi, no_gt) for a in range(a0, min(50, a0 + workers))])
                for sd, why in res:
                    if why:
                        print("  seed", sd, "has a near-tie:", why, flush=True)
                    elif good is None:
                        good = sd
                if good is not None:
                    break
            if good is None:
                raise RuntimeError(f"no case without near-ties for {seed}")
            case = G.make_case(good, n, e, multi, no_gt)
            case.update(graphs_of(case))
            same = all(np.array_equal(case[k], z[f"c{i}_{k}"]) for k in ("edges", "gt_cls", "gt_rel", "obj_logits_3d", "obj_logits_2d",
                                                                          "rel_3d", "rel_2d"))
            stored.append(int(same))
            for k, v in case.items():
                if not k.startswith(("R_", "mR_")):
                    out[f"c{i}_{k}"] = v
            print("case", i, "seed", good, "nodes", n, "edges", e, "multi", multi, "as in recallk_cases.npz:", same, flush=True)
    out["from_recallk"] = np.asarray(stored)
    path = os.path.join(HERE, "scene_graph_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
