"""Eval ranking step on the GPU: host-side mirror of what ``Mmgnet.process_val`` does with the
forward's outputs (reference ``src/model/SGFN_MMG/model.py:458-480``) and of the accuracy
summaries ``MMGNet.validation`` derives from the rank lists (reference ``src/model/model.py:227-242,
364-388``).  Ranks come from counting kernels in libvlsat_hip.so (``csrc/eval_ranks.hip``); the
reference does four ``.cpu()`` syncs and per-edge 665 600-element sorts here."""
from __future__ import annotations

import ctypes as C
from typing import Dict

import numpy as np
import torch

from . import lib as L
from .zeroshot import get_zero_shot_recall, table_shape, zero_shot_table  # noqa: F401  (get_zero_shot_recall: drop-in of eva_utils_acc's)

TOPK_OBJ, TOPK_REL, TOPK_TRIPLET, THRESHOLD = 11, 6, 101, 0.5     # process_val's constants (:463-472)


def softmax_rows(x: torch.Tensor) -> torch.Tensor:
    lib = L.load()
    x = x.contiguous()
    out = torch.empty_like(x)
    L.check(lib.vlsat_k_softmax_rows(x.data_ptr(), x.stride(0), x.shape[0], x.shape[1], out.data_ptr(), L.stream_ptr()))
    return out


def multihot_targets(gt_rel: torch.Tensor, n_rel: int) -> torch.Tensor:
    """The relation target as the multi-hot [E,R] matrix the ranking kernels take.  multi_rel_outputs=True: it
    already is one.  Single-label setting (gt_rel [E] int, 0 = 'none'): get_gt keeps only labels > 0
    (reference eva_utils_acc.py:19-22), i.e. a one-hot row with column 0 cleared."""
    if gt_rel.dim() == 2:
        return gt_rel
    hot = torch.nn.functional.one_hot(gt_rel.long().view(-1), n_rel)
    hot[:, 0] = 0
    return hot


def eval_ranks(obj_logits: torch.Tensor, rel_probs: torch.Tensor, gt_class: torch.Tensor, gt_rel: torch.Tensor,
               edges: torch.Tensor, obj_probs: torch.Tensor | None = None,
               multi_rel_outputs: bool = True, rel_exp: torch.Tensor | None = None) -> Dict[str, torch.Tensor]:
    """Device tensors in, device tensors out (no sync).  ``edges`` is [E,2] (from, to) like the
    ``edge_indices`` the reference hands to process_val; ``gt_rel`` the multi-hot [E,R] target, or the [E] label
    vector of the single-label setting (multi_rel_outputs=False: ``rel_probs`` are then log-probabilities, ranked
    as they are by evaluate_topk_predicate and exponentiated by evaluate_triplet_topk, eva_utils_acc.py:146-147).
    Returns flat rank tensors in the reference's order plus ``cnt`` (ranks per edge)."""
    lib = L.load()
    n, c = obj_logits.shape
    e, r = rel_probs.shape
    dev = obj_logits.device
    obj_logits, rel_probs = obj_logits.contiguous(), rel_probs.contiguous()
    gt_class = gt_class.to(torch.int64).contiguous().view(-1)
    gt_rel = multihot_targets(gt_rel, r).to(torch.int64).contiguous()
    edges = edges.to(torch.int64).contiguous()
    if edges.shape != (e, 2) or gt_rel.shape != (e, r) or gt_class.numel() != n:
        raise L.VlsatError("eval_ranks: edges must be [E,2], gt_rel [E,R], gt_class [N]")
    if obj_probs is None:
        obj_probs = softmax_rows(obj_logits)
    obj_rank = torch.empty(n, dtype=torch.int32, device=dev)
    rel_rank = torch.empty(e, r, dtype=torch.int32, device=dev)
    tri_rank = torch.empty(e, r, dtype=torch.int32, device=dev)
    cnt = torch.empty(e, dtype=torch.int32, device=dev)
    scratch = torch.empty(max(int(lib.vlsat_eval_ranks_scratch_floats(n, c, TOPK_TRIPLET)), 1), dtype=torch.float32, device=dev)
    L.check(lib.vlsat_eval_ranks(obj_logits.data_ptr(), obj_probs.data_ptr(), rel_probs.data_ptr(), gt_class.data_ptr(),
                                 gt_rel.data_ptr(), edges.data_ptr(), n, e, c, r, TOPK_OBJ, TOPK_REL, TOPK_TRIPLET,
                                 THRESHOLD, obj_rank.data_ptr(), rel_rank.data_ptr(), tri_rank.data_ptr(), cnt.data_ptr(),
                                 scratch.data_ptr(), L.stream_ptr()))
    if not multi_rel_outputs:            # triplet scores use exp(log_softmax); predicate ranks above used the raw values
        tri_rank = torch.empty(e, r, dtype=torch.int32, device=dev)
        rel_exp = (rel_probs.exp() if rel_exp is None else rel_exp).contiguous()
        L.check(lib.vlsat_eval_ranks(obj_logits.data_ptr(), obj_probs.data_ptr(), rel_exp.data_ptr(), gt_class.data_ptr(),
                                     gt_rel.data_ptr(), edges.data_ptr(), n, e, c, r, TOPK_OBJ, TOPK_REL, TOPK_TRIPLET,
                                     THRESHOLD, obj_rank.data_ptr(), torch.empty_like(rel_rank).data_ptr(),
                                     tri_rank.data_ptr(), torch.empty_like(cnt).data_ptr(), scratch.data_ptr(), L.stream_ptr()))
    used = torch.arange(r, device=dev)[None, :] < cnt[:, None]          # first cnt[e] slots of each edge row
    return {"top_k_obj": obj_rank, "top_k_rel": rel_rank[used], "top_k_triplet": tri_rank[used], "cnt": cnt,
            "obj_probs": obj_probs}


def rank_tables(obj_logits: torch.Tensor, rel_probs: torch.Tensor, gt_class: torch.Tensor, gt_rel: torch.Tensor,
                edges: torch.Tensor, multi_rel_outputs: bool = True) -> Dict[str, torch.Tensor]:
    """``eval_ranks`` without its variable-length outputs: the rank TABLES as the kernels write them -- obj_rank [N],
    rel_rank / tri_rank [E,R] (first cnt[e] slots of row e used), cnt [E] -- all on the device, nothing that depends on
    their values (no boolean indexing, hence no host synchronisation).  Inputs must already be contiguous, gt_rel the
    multi-hot int64 [E,R] target, edges int64 [E,2].  What ``eval_counts`` consumes."""
    lib = L.load()
    n, c = obj_logits.shape
    e, r = rel_probs.shape
    dev = obj_logits.device
    obj_probs = softmax_rows(obj_logits)
    obj_rank = torch.empty(n, dtype=torch.int32, device=dev)
    rel_rank = torch.empty(e, r, dtype=torch.int32, device=dev)
    tri_rank = torch.empty(e, r, dtype=torch.int32, device=dev)
    cnt = torch.empty(e, dtype=torch.int32, device=dev)
    scratch = torch.empty(max(int(lib.vlsat_eval_ranks_scratch_floats(n, c, TOPK_TRIPLET)), 1), dtype=torch.float32, device=dev)
    L.check(lib.vlsat_eval_ranks(obj_logits.data_ptr(), obj_probs.data_ptr(), rel_probs.data_ptr(), gt_class.data_ptr(),
                                 gt_rel.data_ptr(), edges.data_ptr(), n, e, c, r, TOPK_OBJ, TOPK_REL, TOPK_TRIPLET,
                                 THRESHOLD, obj_rank.data_ptr(), rel_rank.data_ptr(), tri_rank.data_ptr(), cnt.data_ptr(),
                                 scratch.data_ptr(), L.stream_ptr()))
    if not multi_rel_outputs:            # triplet scores use exp(log_softmax); the predicate ranks above used the raw values
        tri_rank = torch.empty(e, r, dtype=torch.int32, device=dev)
        rel_exp = rel_probs.exp()
        L.check(lib.vlsat_eval_ranks(obj_logits.data_ptr(), obj_probs.data_ptr(), rel_exp.data_ptr(), gt_class.data_ptr(),
                                     gt_rel.data_ptr(), edges.data_ptr(), n, e, c, r, TOPK_OBJ, TOPK_REL, TOPK_TRIPLET,
                                     THRESHOLD, torch.empty_like(obj_rank).data_ptr(), torch.empty_like(rel_rank).data_ptr(),
                                     tri_rank.data_ptr(), torch.empty_like(cnt).data_ptr(), scratch.data_ptr(), L.stream_ptr()))
    return {"obj_rank": obj_rank, "rel_rank": rel_rank, "tri_rank": tri_rank, "cnt": cnt}


def eval_counts(counts: torch.Tensor, t3: Dict[str, torch.Tensor], t2: Dict[str, torch.Tensor] | None, gt_class: torch.Tensor,
                gt_rel: torch.Tensor, edges: torch.Tensor, n_scenes: int) -> torch.Tensor:
    """counts (device int64 [len(evaluate.fields())], zeroed once by the caller) += the additive counts of one batch, from the
    rank tables of its 3D (``t3``) and 2D (``t2``) outputs: ``vlsat_eval_counts`` -- the device twin of
    ``evaluate.accumulate`` (integer atomics: exact, order-independent, safe from several streams).  No synchronisation.
    ``t2=None``: the 3D branch alone -- ``scenes``, ``cm_ge*`` and the ``_3d`` fields get what the two-branch call adds, the
    ``_2d`` fields are not touched."""
    lib = L.load()
    e, r = t3["rel_rank"].shape
    n = t3["obj_rank"].numel()
    if counts.dtype != torch.int64 or counts.numel() != 1 + r + 2 * (11 + 6 * r) or not counts.is_contiguous():
        raise L.VlsatError("eval_counts: counts must be a contiguous int64 vector of 1 + R + 2 (11 + 6 R) entries")
    o2, r2, tr2 = (None, None, None) if t2 is None else (t2["obj_rank"], t2["rel_rank"], t2["tri_rank"])
    L.check(lib.vlsat_eval_counts(t3["obj_rank"].data_ptr(), L.ptr(o2), t3["rel_rank"].data_ptr(), L.ptr(r2),
                                  t3["tri_rank"].data_ptr(), L.ptr(tr2), t3["cnt"].data_ptr(), gt_class.data_ptr(),
                                  gt_rel.data_ptr(), edges.data_ptr(), n, e, r, int(n_scenes), counts.data_ptr(), L.stream_ptr()))
    return counts


def eval_triplet_split(split_counts: torch.Tensor, t3: Dict[str, torch.Tensor], t2: Dict[str, torch.Tensor] | None, gt_class: torch.Tensor,
                       gt_rel: torch.Tensor, edges: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """split_counts (device int64 [12], zeroed once by the caller) += the zero-shot split of one batch's triplet ranks, from the
    rank tables of its 3D (``t3``) and 2D (``t2``) outputs (``rank_tables``) and the uint8 [C*C*R] table of
    ``zeroshot.zero_shot_table``: ``vlsat_eval_triplet_split`` (layout: ``evaluate.split_fields``).  No synchronisation.
    ``t2=None``: the 3D half alone; the ``_2d`` half is not touched."""
    lib = L.load()
    e, r = t3["tri_rank"].shape
    c = table_shape(table, r)
    if split_counts.dtype != torch.int64 or split_counts.numel() != 12 or not split_counts.is_contiguous():
        raise L.VlsatError("eval_triplet_split: split_counts must be a contiguous int64 vector of 12 entries")
    if (table.dtype != torch.uint8 or not table.is_contiguous() or not split_counts.is_cuda or table.device != split_counts.device
            or t3["tri_rank"].device != split_counts.device):
        raise L.VlsatError("eval_triplet_split: the table must be a contiguous uint8 tensor on the device of the counts and ranks")
    L.check(lib.vlsat_eval_triplet_split(t3["tri_rank"].data_ptr(), L.ptr(None if t2 is None else t2["tri_rank"]), t3["cnt"].data_ptr(), gt_class.data_ptr(),
                                         gt_rel.data_ptr(), edges.data_ptr(), table.data_ptr(), e, c, r, split_counts.data_ptr(),
                                         L.stream_ptr()))
    return split_counts


@torch.no_grad()
def process_val_counts(model, counts: torch.Tensor, obj_points, obj_2d_feats, gt_cls, descriptor, gt_rel_cls, edge_indices,
                       batch_ids=None, n_scenes: int = 1, fc_sizes=None, recall: torch.Tensor | None = None,
                       split_table: torch.Tensor | None = None, split_counts: torch.Tensor | None = None):
    """``process_val`` for an evaluation LOOP: forward + both ranking passes + the counts, all enqueued on the current stream,
    nothing read back (``Mmgnet.process_val`` returns numpy rank lists, i.e. four host round trips per scene, reference
    SGFN_MMG/model.py:463-480; ``validation()`` only ever turns them into the counts accumulated here).
    ``edge_indices`` is [E,2] as the data loader yields it, on the device.  ``recall``: a device fp64 vector of
    ``evaluate.recall_fields()`` that additionally accumulates the Recall@K / mR@K of both branches (``recallk_counts``).
    ``split_table`` / ``split_counts``: the device uint8 zero-shot table (``zeroshot.zero_shot_table``) and the device int64 [12]
    vector of ``evaluate.split_fields()`` that additionally accumulates the zero-shot split of the triplet ranks.
    ``obj_2d_feats=None``: the 3D branch alone, on both routes -- the one call runs its 3D-only step, the separate calls are
    ``forward_3d`` + one ``rank_tables`` + one ``recallk_counts``; the ``_2d`` entries of every vector are not touched.
    Single-label models (``multi_rel_outputs=False``, ``gt_rel_cls`` the [E] label vector) take the one call like multi-label ones;
    the separate calls serve ``recall=`` and plans that had to permute the edges, for both settings."""
    if (split_table is None) != (split_counts is None):
        raise ValueError("process_val_counts: give both split_table and split_counts, or neither")
    multi = bool(getattr(getattr(model, "config", None), "multi_rel_outputs", True))
    edges = edge_indices.to(torch.int64).contiguous()
    # one library call: forward + ranking + counts in the plan's scratch; a single-label model rides it too (its triplet kernel takes
    # exp of the log-probabilities on load), with the one-hot target, column 0 cleared, that multihot_targets makes of its labels
    if recall is None and hasattr(model, "process_val_counts"):
        r = model.config.num_rel_class
        extra = {} if split_table is None else {"split_table": split_table, "split_counts": split_counts}
        if not multi:                               # (the method keeps its earlier refusal of such a model for callers that do not say so)
            extra["single_label"] = True
        if model.process_val_counts(counts, obj_points, obj_2d_feats, gt_cls.to(torch.int64).contiguous().view(-1), descriptor,
                                    multihot_targets(gt_rel_cls, r).to(torch.int64).contiguous(), edges, batch_ids, n_scenes, fc_sizes,
                                    **extra):
            return counts
    # with the fully-connected hint the plan never reads the edge list: the [2,E] view is enough (no transpose kernel)
    ei_t = edges.t() if fc_sizes is not None else edges.t().contiguous()
    use_2d = obj_2d_feats is not None
    if use_2d:
        obj3, obj2, rel3, rel2 = model(obj_points, obj_2d_feats, ei_t, descriptor, batch_ids, istrain=False, fc_sizes=fc_sizes)
    else:
        obj3, rel3 = model.forward_3d(obj_points, ei_t, descriptor, batch_ids, fc_sizes=fc_sizes)
    gt_rel = multihot_targets(gt_rel_cls, rel3.shape[1]).to(torch.int64).contiguous()
    gt_cls = gt_cls.to(torch.int64).contiguous().view(-1)
    t3 = rank_tables(obj3, rel3, gt_cls, gt_rel, edges, multi)
    t2 = rank_tables(obj2, rel2, gt_cls, gt_rel, edges, multi) if use_2d else None
    if recall is not None:
        from . import evaluate as EV
        bid = None if batch_ids is None else batch_ids.view(-1)
        c3 = recallk_counts(obj3, rel3, gt_cls, gt_rel, edges, bid, n_scenes, multi)
        c2 = recallk_counts(obj2, rel2, gt_cls, gt_rel, edges, bid, n_scenes, multi) if use_2d else None
        recall += EV.recall_vector(c3, c2, rel3.shape[1])
    if split_table is not None:
        eval_triplet_split(split_counts, t3, t2, gt_cls, gt_rel, edges, split_table)
    return eval_counts(counts, t3, t2, gt_cls, gt_rel, edges, n_scenes)


def cls_matrix(gt_class: torch.Tensor, gt_rel: torch.Tensor, edges: torch.Tensor, obj_topk: torch.Tensor) -> torch.Tensor:
    """[n,5] rows (sub_gt, sub_pred_rank, obj_gt, obj_pred_rank, predicate | -1) in the order
    evaluate_triplet_topk appends them (eva_utils_acc.py:185-199): per edge its gt predicates in
    ascending class order, or one row with -1 when the edge has no gt relation."""
    if gt_rel.dim() == 1:
        raise L.VlsatError("cls_matrix: pass the multi-hot target (metrics.multihot_targets)")
    e, r = gt_rel.shape
    has = gt_rel == 1
    none = ~has.any(1)
    slot = torch.cat([none[:, None], has], 1)                             # column 0 = the "-1" row
    ei, ki = torch.nonzero(slot, as_tuple=True)                           # row-major = edge order, ascending class
    a, b = edges[ei, 0], edges[ei, 1]
    gt_class = gt_class.view(-1)
    return torch.stack([gt_class[a], obj_topk[a].long(), gt_class[b], obj_topk[b].long(), ki - 1], 1)


def _forward_eval(model, obj_points, obj_2d_feats, descriptor, edge_indices, batch_ids, use_2d=True):
    """(obj3, obj2, rel3, rel2) of the forward; ``use_2d=False``: ``forward_3d``, ``obj_2d_feats`` not read, the 2D outputs None."""
    ei_t = edge_indices.t().contiguous()
    if not use_2d:
        obj3, rel3 = model.forward_3d(obj_points, ei_t, descriptor, batch_ids)
        return obj3, None, rel3, None
    return model(obj_points, obj_2d_feats, ei_t, descriptor, batch_ids, istrain=False)


@torch.no_grad()
def process_val(model, obj_points, obj_2d_feats, gt_cls, descriptor, gt_rel_cls, edge_indices, batch_ids=None,
                use_triplet=True):
    """Same call and 10-tuple as ``Mmgnet.process_val`` (reference SGFN_MMG/model.py:458-480);
    ``edge_indices`` is [E,2] as the data loader yields it.  Rank arrays are numpy int64 like the
    reference's; the score lists come back stacked as tensors.  ``obj_2d_feats=None``: the 3D-only forward; the three 2D rank
    slots of the tuple (``top_k_obj_2d``, ``top_k_rel_2d``, ``top_k_triplet_2d``) are None."""
    outs = _forward_eval(model, obj_points, obj_2d_feats, descriptor, edge_indices, batch_ids, use_2d=obj_2d_feats is not None)
    return _process_val_from(model, outs, gt_cls, gt_rel_cls, edge_indices, use_triplet)


def _process_val_from(model, outs, gt_cls, gt_rel_cls, edge_indices, use_triplet):
    obj3, obj2, rel3, rel2 = outs
    multi = bool(getattr(getattr(model, "config", None), "multi_rel_outputs", True))     # self.mconfig.multi_rel_outputs
    gt_rel_cls = multihot_targets(gt_rel_cls, rel3.shape[1])
    r3 = eval_ranks(obj3, rel3, gt_cls, gt_rel_cls, edge_indices, multi_rel_outputs=multi)
    np64 = lambda t: None if t is None else t.cpu().numpy().astype(np.int64)
    if obj2 is None:                                                       # 3D-only: the 2D rank slots stay None
        r2 = {"top_k_obj": None, "top_k_rel": None, "top_k_triplet": None}
    else:
        r2 = eval_ranks(obj2, rel2, gt_cls, gt_rel_cls, edge_indices, multi_rel_outputs=multi)
    cm = cls_matrix(gt_cls, gt_rel_cls, edge_indices, r3["top_k_obj"])     # obj_topk = 3D ranks for both (:469-470)
    if not use_triplet:
        return np64(r3["top_k_obj"]), np64(r2["top_k_obj"]), np64(r3["top_k_rel"]), np64(r2["top_k_rel"]), [101], None, None, None, None, None
    has = (gt_rel_cls == 1)
    ei, _ = torch.nonzero(has, as_tuple=True)
    sub_scores = r3["obj_probs"][edge_indices[ei, 0]]
    obj_scores = r3["obj_probs"][edge_indices[ei, 1]]
    rel_scores = rel3[ei] if multi else rel3[ei].exp()
    return (np64(r3["top_k_obj"]), np64(r2["top_k_obj"]), np64(r3["top_k_rel"]), np64(r2["top_k_rel"]),
            np64(r3["top_k_triplet"]), np64(r2["top_k_triplet"]), cm.cpu().numpy(), sub_scores, obj_scores, rel_scores)


def summarize(top_k_obj, top_k_rel, top_k_triplet, cls_mat=None) -> Dict[str, float]:
    """Accuracy summaries of validation() (reference src/model/model.py:267-282) and
    get_mean_recall (eva_utils_acc.py:224-237) from the rank arrays."""
    o, r, t = np.asarray(top_k_obj), np.asarray(top_k_rel), np.asarray(top_k_triplet)
    pct = lambda a, k: float((a <= k).sum() * 100 / max(len(a), 1))
    out = {"obj_acc@1": pct(o, 1), "obj_acc@5": pct(o, 5), "obj_acc@10": pct(o, 10),
           "rel_acc@1": pct(r, 1), "rel_acc@3": pct(r, 3), "rel_acc@5": pct(r, 5),
           "triplet_acc@50": pct(t, 50), "triplet_acc@100": pct(t, 100)}
    if cls_mat is not None and len(cls_mat):
        cm = np.asarray(cls_mat)
        rec = [[], []]
        for i in range(int(cm.max())):
            sel = t[cm[:, -1] == i]
            if len(sel):
                rec[0].append((sel <= 50).sum() * 100 / len(sel))
                rec[1].append((sel <= 100).sum() * 100 / len(sel))
        if rec[0]:
            out["mean_recall@50"], out["mean_recall@100"] = float(np.mean(rec[0])), float(np.mean(rec[1]))
    return out


# ---- Recall@K / mR@K (reference src/utils/eval_utils_recall.py, process_val2 / process_val3 of SGFN_MMG/model_in21k.py) ----
RECALL_K = (20, 50, 100)
RECALL_VARIANTS = ("predcls_gc", "predcls_ngc", "sgcls_gc", "sgcls_ngc")     # bits 1, 2, 4, 8 of vlsat_eval_recallk's mask
_NGC_CAP = 100                                                               # topk_each of the NGC variants


def recallk_width(n_rel: int) -> int:
    """Fields per scene of the counts ``recallk_counts`` returns: gt_edges, gt_per_class[R], then per variant (in
    RECALL_VARIANTS order) hit@{20,50,100} and class_hit@{20,50,100}[R]."""
    return 1 + n_rel + len(RECALL_VARIANTS) * (3 + 3 * n_rel)


def recallk_offset(variant: str, n_rel: int) -> int:
    """Index of ``variant``'s hit@20 in a counts row; hit@K, then class_hit@K[R] for K = 20, 50, 100 follow."""
    return 1 + n_rel + RECALL_VARIANTS.index(variant) * (3 + 3 * n_rel)


def _variant_mask(variants) -> int:
    m = 0
    for v in variants:
        if v not in RECALL_VARIANTS:
            raise ValueError(f"recallk: unknown variant {v!r} (one of {RECALL_VARIANTS})")
        m |= 1 << RECALL_VARIANTS.index(v)
    return m


def _recallk_inputs(obj_logits, rel, gt_cls, gt_rel, edges, batch_ids, multi_rel_outputs, obj_probs):
    e, r = rel.shape
    gt_cls = gt_cls.to(torch.int64).contiguous().view(-1)
    gt_rel = multihot_targets(gt_rel, r).to(torch.int64).contiguous()
    edges = edges.to(torch.int64).contiguous().view(-1, 2)
    if batch_ids is not None:
        batch_ids = batch_ids.to(torch.int64).contiguous().view(-1)
    r_probs = (rel if multi_rel_outputs else rel.exp()).float().contiguous()
    if edges.shape[0] != e or gt_rel.shape != (e, r) or gt_cls.numel() != obj_logits.shape[0]:
        raise L.VlsatError("recallk: edges must be [E,2], gt_rel [E,R] (or [E]), gt_cls [N]")
    return gt_cls, gt_rel, edges, batch_ids, r_probs, obj_probs


def recallk_counts(obj_logits: torch.Tensor, rel: torch.Tensor, gt_cls: torch.Tensor, gt_rel: torch.Tensor,
                   edges: torch.Tensor, batch_ids: torch.Tensor | None, n_scenes: int, multi_rel_outputs: bool = True,
                   variants=RECALL_VARIANTS, obj_probs: torch.Tensor | None = None) -> torch.Tensor:
    """Per-scene Recall@K counts, int64 [n_scenes, recallk_width(R)] (layout: ``recallk_width``), of the four variants
    PredCls / SGCls x graph constraint (topk_each = 1) / none (topk_each = 100) at K = 20, 50, 100.
    ``obj_logits`` [N, C] (the object probabilities are their softmax -- use_clip=True -- unless ``obj_probs`` is given),
    ``rel`` [E, R] predicate probabilities (log-probabilities when ``multi_rel_outputs`` is False), ``gt_rel`` the
    multi-hot [E, R] or single-label [E] target, ``edges`` [E, 2] grouped by scene in ascending order, the scene of an edge
    being ``batch_ids[edges[e, 0]]`` (None: one scene).  Counting rule and tie convention: include/vlsat.h
    (vlsat_eval_recallk).  Device tensors: the HIP kernels (csrc/eval_recall.hip), asynchronous, no host round trip.
    CPU tensors: ``recallk_counts_host``.  Variants left out of ``variants`` are zeros."""
    if not obj_logits.is_cuda:
        return recallk_counts_host(obj_logits, rel, gt_cls, gt_rel, edges, batch_ids, n_scenes, multi_rel_outputs, variants,
                                   obj_probs)
    lib = L.load()
    n, c = obj_logits.shape
    e, r = rel.shape
    n_scenes = int(n_scenes)
    gt_cls, gt_rel, edges, batch_ids, r_probs, obj_probs = _recallk_inputs(obj_logits, rel, gt_cls, gt_rel, edges, batch_ids,
                                                                          multi_rel_outputs, obj_probs)
    mask = _variant_mask(variants)
    if obj_probs is None:
        obj_probs = softmax_rows(obj_logits.float())
    obj_probs = obj_probs.float().contiguous()
    dev = obj_logits.device
    out = torch.empty(n_scenes, recallk_width(r), dtype=torch.int64, device=dev)
    nbytes = int(lib.vlsat_eval_recallk_scratch_bytes(n, e, c, r, n_scenes))
    scratch = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    L.check(lib.vlsat_eval_recallk(obj_probs.data_ptr(), r_probs.data_ptr(), gt_cls.data_ptr(), gt_rel.data_ptr(), edges.data_ptr(),
                                   L.ptr(batch_ids), n, e, c, r, n_scenes, mask, scratch.data_ptr(), out.data_ptr(), L.stream_ptr()))
    return out


def _tri_table(ks: int, r: int, dev) -> torch.Tensor:
    """Index triples (i, j, k) of sorted positions with (i+1)(j+1)(k+1) <= 100: an entry outside is dominated by at least
    100 others, so an edge's 100 largest products lie inside (eval_recall.hip)."""
    t = [(a - 1, b - 1, q - 1) for a in range(1, ks + 1) for b in range(1, min(ks, _NGC_CAP // a) + 1)
         for q in range(1, min(r, _NGC_CAP // (a * b)) + 1)]
    return torch.tensor(t, dtype=torch.int64, device=dev).view(-1, 3)


@torch.no_grad()
def recallk_counts_host(obj_logits, rel, gt_cls, gt_rel, edges, batch_ids, n_scenes, multi_rel_outputs=True,
                        variants=RECALL_VARIANTS, obj_probs=None, chunk: int = 8192) -> torch.Tensor:
    """The counting definition of ``recallk_counts`` stated directly in PyTorch, on whatever device the inputs are:
    every correct entry c of an edge is tested for (1) being one of the edge's topk_each candidates and (2) having fewer than K
    candidates of its scene strictly above it.  The candidates of an SGCls NGC edge (its 100 largest products) are taken
    from the dominance-pruned index set (``_tri_table``) instead of the 665 600 products.  Exact, slow; for CPU tests and
    devices without the HIP library."""
    n, c = obj_logits.shape
    e, r = rel.shape
    n_scenes = int(n_scenes)
    dev = obj_logits.device
    gt_cls, gt_rel, edges, batch_ids, rp, obj_probs = _recallk_inputs(obj_logits, rel, gt_cls, gt_rel, edges, batch_ids,
                                                                      multi_rel_outputs, obj_probs)
    mask = _variant_mask(variants)
    probs = (torch.softmax(obj_logits.float(), -1) if obj_probs is None else obj_probs.float()).contiguous()
    out = torch.zeros(n_scenes, recallk_width(r), dtype=torch.int64, device=dev)
    if e == 0 or n_scenes == 0:
        return out
    a, b = edges[:, 0], edges[:, 1]
    scene = batch_ids[a] if batch_ids is not None else torch.zeros(e, dtype=torch.int64, device=dev)
    hot = gt_rel == 1
    has = hot.any(1)
    out[:, 0] = torch.bincount(scene[has], minlength=n_scenes)[:n_scenes]
    out[:, 1:1 + r].index_add_(0, scene, hot.long())
    neg = torch.tensor(-float("inf"), device=dev)
    for vi, name in enumerate(RECALL_VARIANTS):
        if not (mask >> vi) & 1:
            continue
        sg, gc = name.startswith("sgcls"), name.endswith("_gc")
        if sg:
            corr = (probs[a, gt_cls[a]] * probs[b, gt_cls[b]])[:, None] * rp          # fl(fl(s*o)*r), the correct entries
            n_entries = c * c * r
        else:
            corr = rp
            n_entries = r
        corr = torch.where(hot, corr, neg)
        if gc:                                                                       # one candidate: the edge's maximum
            if sg:
                smax = probs.max(1).values
                cand = ((smax[a] * smax[b]) * rp.max(1).values)[:, None]
            else:
                cand = rp.max(1, keepdim=True).values
        elif not sg:
            cand = rp                                                                 # R < 100: every entry is a candidate
        else:
            ks = min(c, _NGC_CAP)
            ss = probs.topk(ks, 1).values
            rs = rp.sort(1, descending=True).values
            tri = _tri_table(ks, r, dev)
            cand = torch.empty(e, min(_NGC_CAP, n_entries), dtype=torch.float32, device=dev)
            for e0 in range(0, e, chunk):
                sl = slice(e0, min(e, e0 + chunk))
                vals = (ss[a[sl]][:, tri[:, 0]] * ss[b[sl]][:, tri[:, 1]]) * rs[sl][:, tri[:, 2]]
                cand[sl] = vals.topk(cand.shape[1], 1).values
        cap = 1 if gc else _NGC_CAP
        if cap < n_entries:                                                           # (1) #{entries of e > c} < topk_each
            kth = cand[:, cap - 1:cap]
            cond1 = corr >= kth
        else:
            cond1 = torch.ones_like(hot)
        base = recallk_offset(name, r)
        for s in range(n_scenes):
            sel = scene == s
            if not bool(sel.any()):
                continue
            cs = cand[sel].reshape(-1).sort().values                                  # ascending
            cc = corr[sel]
            above = cs.numel() - torch.searchsorted(cs, cc.contiguous(), right=True)  # #{candidates of the scene > c}
            for q, k in enumerate(RECALL_K):
                hit = (hot[sel] & cond1[sel] & (above < k)).any(1)                    # (2)
                out[s, base + q] = hit.sum()
                out[s, base + 3 + q * r: base + 3 + (q + 1) * r] = (hot[sel] & hit[:, None]).sum(0)
    return out


# ---- the predicted scene graph: per-scene top-K triplets with their indices (csrc/scene_graph.hip) ----
SG_MAX_TOP_K, SG_MAX_EACH = 1024, 100
_SG_MODES = {"triplet": 0, "rels": 1}


class SceneGraph:
    """Top-K triplets of every scene of a batch: ``edge`` (row of the batch's edge list), ``sub_cls``, ``obj_cls``, ``pred``
    int32 [S, K], ``score`` float32 [S, K], ``n_valid`` int32 [S]; rows past ``n_valid[s]`` hold -1 / 0.  Rows are ordered by
    score descending, then edge, subject class, object class, predicate ascending (include/vlsat.h, vlsat_scene_graph_topk)."""
    __slots__ = ("edge", "sub_cls", "obj_cls", "pred", "score", "n_valid")

    def __init__(self, triplets: torch.Tensor, score: torch.Tensor, n_valid: torch.Tensor):
        self.edge, self.sub_cls, self.obj_cls, self.pred = (triplets[..., i] for i in range(4))
        self.score, self.n_valid = score, n_valid

    def scene(self, s: int, edge_offset: int = 0) -> "SceneGraph":
        """Scene ``s`` as a one-scene graph; ``edge_offset`` is subtracted from its edge rows (the scene's first row in the batch)."""
        g = SceneGraph.__new__(SceneGraph)
        for k in ("sub_cls", "obj_cls", "pred", "score"):
            setattr(g, k, getattr(self, k)[s:s + 1])
        e = self.edge[s:s + 1]
        g.edge = torch.where(e >= 0, e - edge_offset, e) if edge_offset else e
        g.n_valid = self.n_valid[s:s + 1]
        return g

    def cpu(self) -> "SceneGraph":
        g = SceneGraph.__new__(SceneGraph)
        for k in self.__slots__:
            setattr(g, k, getattr(self, k).cpu())
        return g


def exp_probs(log_probs: torch.Tensor) -> torch.Tensor:
    """exp of a single-label model's log-probabilities by the library's kernel (``vlsat_k_exp``), the one ``predict_graph`` uses."""
    x = log_probs.float().contiguous()
    out = torch.empty_like(x)
    L.check(L.load().vlsat_k_exp(x.data_ptr(), x.numel(), out.data_ptr(), L.stream_ptr()))
    return out


def _sg_args(rel, edges, batch_ids, n_scenes, top_k, topk_each, evaluate):
    if evaluate not in _SG_MODES:
        raise NotImplementedError("evaluate type", evaluate)
    top_k, topk_each, n_scenes = int(top_k), int(topk_each), int(n_scenes)
    if not 1 <= top_k <= SG_MAX_TOP_K:
        raise L.VlsatError(f"scene_graph_topk: top_k must be in 1..{SG_MAX_TOP_K}")
    if not 1 <= topk_each <= SG_MAX_EACH:
        raise L.VlsatError(f"scene_graph_topk: topk_each must be in 1..{SG_MAX_EACH}")
    if n_scenes < 0 or (n_scenes > 1 and batch_ids is None):
        raise L.VlsatError("scene_graph_topk: batch_ids is required for more than one scene")
    edges = edges.to(torch.int64).contiguous().view(-1, 2)
    if rel.dim() != 2 or edges.shape[0] != rel.shape[0]:
        raise L.VlsatError("scene_graph_topk: rel must be [E,R] and edges [E,2]")
    if batch_ids is not None:
        batch_ids = batch_ids.to(torch.int64).contiguous().view(-1)
    return edges, batch_ids, n_scenes, top_k, topk_each, _SG_MODES[evaluate]


def scene_graph_topk(obj_logits: torch.Tensor, rel: torch.Tensor, edges: torch.Tensor, batch_ids: torch.Tensor | None,
                     n_scenes: int, multi_rel_outputs: bool = True, top_k: int = 100, topk_each: int = 100,
                     evaluate: str = "triplet", obj_probs: torch.Tensor | None = None) -> SceneGraph:
    """The predicted graph of every scene: its ``top_k`` (subject, predicate, object) triplets out of each edge's ``topk_each``
    best -- the reference's ``pred_triplets`` (evaluate_triplet_recallk, eval_utils_recall.py:24-96), without labels.
    ``obj_logits`` [N, C] (the object probabilities are their softmax unless ``obj_probs`` is given), ``rel`` [E, R] predicate
    probabilities (log-probabilities when ``multi_rel_outputs`` is False), ``edges`` [E, 2] grouped by scene in ascending order,
    the scene of an edge being ``batch_ids[edges[e, 0]]`` (None: one scene).  ``evaluate`` = "triplet" scores
    fl(fl(s_i * o_j) * r_k); "rels" scores r_k and reports subject / object class as -1.  Output contract and tie rule:
    include/vlsat.h (vlsat_scene_graph_topk).  Device tensors: the HIP kernels, asynchronous, no host round trip.  CPU tensors:
    ``scene_graph_topk_host``."""
    if not obj_logits.is_cuda:
        return scene_graph_topk_host(obj_logits, rel, edges, batch_ids, n_scenes, multi_rel_outputs, top_k, topk_each, evaluate,
                                     obj_probs)
    lib = L.load()
    n, c = obj_logits.shape
    e, r = rel.shape
    edges, batch_ids, n_scenes, top_k, topk_each, mode = _sg_args(rel, edges, batch_ids, n_scenes, top_k, topk_each, evaluate)
    r_probs = rel.float().contiguous() if multi_rel_outputs else exp_probs(rel)
    if obj_probs is None and mode == 0:
        obj_probs = softmax_rows(obj_logits.float())
    if obj_probs is not None:
        obj_probs = obj_probs.float().contiguous()
    dev = obj_logits.device
    trip = torch.empty(n_scenes, top_k, 4, dtype=torch.int32, device=dev)
    score = torch.empty(n_scenes, top_k, dtype=torch.float32, device=dev)
    n_valid = torch.empty(n_scenes, dtype=torch.int32, device=dev)
    if c > 1024 or r > 32 or c < 1 or r < 1:
        raise L.VlsatError("scene_graph_topk: 1..1024 object and 1..32 relation classes")
    nbytes = int(lib.vlsat_scene_graph_scratch_bytes(n, e, c, r, n_scenes, top_k, topk_each))
    scratch = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    L.check(lib.vlsat_scene_graph_topk(L.ptr(obj_probs), r_probs.data_ptr(), edges.data_ptr(), L.ptr(batch_ids), n, e, c, r, n_scenes,
                                       mode, top_k, topk_each, scratch.data_ptr(), trip.data_ptr(), score.data_ptr(),
                                       n_valid.data_ptr(), L.stream_ptr()))
    return SceneGraph(trip, score, n_valid)


@torch.no_grad()
def scene_graph_topk_host(obj_logits, rel, edges, batch_ids, n_scenes, multi_rel_outputs=True, top_k=100, topk_each=100,
                          evaluate="triplet", obj_probs=None, chunk: int = 8192) -> SceneGraph:
    """``scene_graph_topk`` stated in PyTorch on whatever device the inputs are: per edge its min(topk_each, #entries) largest
    entries with their classes (triplet mode: out of the dominance-pruned positions of ``_tri_table``, never the C x C x R
    products), per scene the top_k of them in the contract's order.  Among candidates equal to a boundary value it keeps the
    smallest (edge, subject class, object class, predicate).  Exact, slow; for CPU tests and devices without the HIP library."""
    n, c = obj_logits.shape
    e, r = rel.shape
    dev = obj_logits.device
    edges, batch_ids, n_scenes, top_k, topk_each, mode = _sg_args(rel, edges, batch_ids, n_scenes, top_k, topk_each, evaluate)
    rp = (rel if multi_rel_outputs else rel.exp()).float().contiguous()
    trip = torch.full((n_scenes, top_k, 4), -1, dtype=torch.int32, device=dev)
    score = torch.zeros(n_scenes, top_k, dtype=torch.float32, device=dev)
    n_valid = torch.zeros(n_scenes, dtype=torch.int32, device=dev)
    if e == 0 or n_scenes == 0:
        return SceneGraph(trip, score, n_valid)
    a, b = edges[:, 0], edges[:, 1]
    scene = batch_ids[a] if batch_ids is not None else torch.zeros(e, dtype=torch.int64, device=dev)
    rs, ri = rp.sort(dim=1, descending=True, stable=True)
    if mode == 1:
        lim = min(topk_each, r)
        cand, pack = rs[:, :lim], ri[:, :lim]                                         # pack: the predicate
    else:
        probs = (torch.softmax(obj_logits.float(), -1) if obj_probs is None else obj_probs.float()).contiguous()
        ks = min(c, _NGC_CAP)
        ss, si = probs.sort(dim=1, descending=True, stable=True)
        ss, si = ss[:, :ks], si[:, :ks]
        lim = min(topk_each, c * c * r)
        tri = _tri_table(ks, r, dev)
        tri = tri[(tri[:, 0] + 1) * (tri[:, 1] + 1) * (tri[:, 2] + 1) <= lim]
        cand = torch.empty(e, lim, dtype=torch.float32, device=dev)
        pack = torch.empty(e, lim, dtype=torch.int64, device=dev)
        for e0 in range(0, e, chunk):
            sl = slice(e0, min(e, e0 + chunk))
            vals = (ss[a[sl]][:, tri[:, 0]] * ss[b[sl]][:, tri[:, 1]]) * rs[sl][:, tri[:, 2]]     # fl(fl(s*o)*r)
            pk = (si[a[sl]][:, tri[:, 0]] * c + si[b[sl]][:, tri[:, 1]]) * r + ri[sl][:, tri[:, 2]]
            o1 = pk.argsort(dim=1, stable=True)                                           # (value descending, classes ascending)
            o2 = vals.gather(1, o1).argsort(dim=1, descending=True, stable=True)
            order = o1.gather(1, o2)[:, :lim]
            cand[sl], pack[sl] = vals.gather(1, order), pk.gather(1, order)
    eid = torch.arange(e, device=dev)[:, None].expand(-1, lim)
    for s in range(n_scenes):
        sel = scene == s
        if not bool(sel.any()):
            continue
        v, ed, pk = cand[sel].reshape(-1), eid[sel].reshape(-1), pack[sel].reshape(-1)
        o1 = (ed * (c * c * r if mode == 0 else r) + pk).argsort(stable=True)
        o2 = v[o1].argsort(descending=True, stable=True)
        order = o1[o2][:top_k]
        k = order.numel()
        n_valid[s] = k
        score[s, :k] = v[order]
        trip[s, :k, 0] = ed[order].int()
        p = pk[order]
        if mode == 0:
            trip[s, :k, 1], trip[s, :k, 2], trip[s, :k, 3] = (p // (c * r)).int(), ((p // r) % c).int(), (p % r).int()
        else:
            trip[s, :k, 3] = p.int()
    return SceneGraph(trip, score, n_valid)


# ---- the decoded scene graph: labels per object, asserted predicates per pair (csrc/graph_decode.hip) ----
GD_MAX_LABELS, GD_MAX_REL = 8, 4096
_GD_SCORES = {"rel": 0, "triplet": 1}


class DecodedGraph:
    """The graph a model asserts for every scene of a batch.  Nodes: ``labels`` int32 / ``label_probs`` float32 [N, n_labels], the
    most probable classes of every object, descending.  Relations: ``edge`` (row of the batch's edge list) and ``pred`` int32
    [S, max_rel], ``score`` float32 [S, max_rel], ordered by score descending, then edge, predicate ascending; ``n_total`` int32
    [S] asserted (edge, predicate) pairs, ``n_valid`` = min(n_total, max_rel) rows kept; rows past ``n_valid[s]`` hold -1 / 0
    (include/vlsat.h, vlsat_graph_decode)."""
    __slots__ = ("labels", "label_probs", "edge", "pred", "score", "n_valid", "n_total")

    def __init__(self, labels, label_probs, rels, score, n_valid, n_total):
        self.labels, self.label_probs = labels, label_probs
        self.edge, self.pred = rels[..., 0], rels[..., 1]
        self.score, self.n_valid, self.n_total = score, n_valid, n_total

    def scene(self, s: int, edge_offset: int = 0, nodes=None) -> "DecodedGraph":
        """Scene ``s`` as a one-scene graph; ``edge_offset`` is subtracted from its edge rows (the scene's first row in the batch);
        ``nodes`` = (first, end) node rows of the scene (None: the node tables stay the batch's)."""
        g = DecodedGraph.__new__(DecodedGraph)
        for k in ("pred", "score", "n_valid", "n_total"):
            setattr(g, k, getattr(self, k)[s:s + 1])
        e = self.edge[s:s + 1]
        g.edge = torch.where(e >= 0, e - edge_offset, e) if edge_offset else e
        sl = slice(None) if nodes is None else slice(int(nodes[0]), int(nodes[1]))
        g.labels, g.label_probs = self.labels[sl], self.label_probs[sl]
        return g

    def cpu(self) -> "DecodedGraph":
        g = DecodedGraph.__new__(DecodedGraph)
        for k in self.__slots__:
            setattr(g, k, getattr(self, k).cpu())
        return g


def decode_thresholds(threshold, n_rel: int, device) -> torch.Tensor:
    """``threshold`` (a float, or a length-R sequence / tensor) as the float32 [R] device vector the kernels compare with."""
    if torch.is_tensor(threshold):
        t = threshold.detach().to(device=device, dtype=torch.float32).reshape(-1)
    elif isinstance(threshold, (int, float)):
        t = torch.full((n_rel,), float(threshold), dtype=torch.float32, device=device)
    else:
        t = torch.tensor([float(x) for x in threshold], dtype=torch.float32, device=device)
    if t.numel() == 1 and n_rel != 1:
        t = t.expand(n_rel)
    if t.numel() != n_rel:
        raise L.VlsatError(f"decode_graph: threshold must be a number or hold one value per predicate ({n_rel})")
    return t.contiguous()


def _gd_args(obj_logits, rel, edges, batch_ids, n_scenes, score, n_labels, max_rel):
    if score not in _GD_SCORES:
        raise NotImplementedError("score type", score)
    n_labels, max_rel, n_scenes = int(n_labels), int(max_rel), int(n_scenes)
    if obj_logits.dim() != 2 or rel.dim() != 2:
        raise L.VlsatError("decode_graph: obj_logits must be [N,C] and rel [E,R]")
    c, r = obj_logits.shape[1], rel.shape[1]
    if not 1 <= c <= 1024 or not 1 <= r <= 32:
        raise L.VlsatError("decode_graph: 1..1024 object and 1..32 relation classes")
    if not 1 <= n_labels <= GD_MAX_LABELS or n_labels > c:
        raise L.VlsatError(f"decode_graph: n_labels must be in 1..{GD_MAX_LABELS} (and at most the object class count)")
    if not 1 <= max_rel <= GD_MAX_REL:
        raise L.VlsatError(f"decode_graph: max_rel must be in 1..{GD_MAX_REL}")
    if n_scenes < 0 or (n_scenes > 1 and batch_ids is None):
        raise L.VlsatError("decode_graph: batch_ids is required for more than one scene")
    edges = edges.to(torch.int64).contiguous().view(-1, 2)
    if edges.shape[0] != rel.shape[0]:
        raise L.VlsatError("decode_graph: rel must be [E,R] and edges [E,2]")
    if batch_ids is not None:
        batch_ids = batch_ids.to(torch.int64).contiguous().view(-1)
    return edges, batch_ids, n_scenes, _GD_SCORES[score], n_labels, max_rel


def decode_graph(obj_logits: torch.Tensor, rel: torch.Tensor, edges: torch.Tensor, batch_ids: torch.Tensor | None, n_scenes: int,
                 multi_rel_outputs: bool = True, threshold=0.5, score: str = "rel", n_labels: int = 3, max_rel: int = 1024,
                 obj_probs: torch.Tensor | None = None, rel_probs: torch.Tensor | None = None) -> DecodedGraph:
    """The graph the outputs assert, per scene: for every object its ``n_labels`` most probable classes, and the (edge,
    predicate) pairs that pass the reference's decision rule (eva_utils_acc.py:42-63, 176-181; get_gt :19-22) -- multi-label:
    every predicate with probability >= its threshold; single label (``rel`` holds log-probabilities): the arg-max predicate
    unless it is class 0 = none or below its threshold.  ``score`` = "rel" ranks by the predicate probability, "triplet" by
    fl(fl(s * o) * r) with the two nodes' top-1 probabilities; at most ``max_rel`` pairs per scene are kept, in (score
    descending, edge, predicate ascending) order.  ``threshold``: a float or one value per predicate.  Inputs as for
    ``scene_graph_topk``; ``rel_probs`` [E, R], when given, are the predicate probabilities themselves (``rel`` is then not read).  Device tensors: the HIP kernels, asynchronous, no host round trip.  CPU tensors: ``decode_graph_host``."""
    if not obj_logits.is_cuda:
        return decode_graph_host(obj_logits, rel, edges, batch_ids, n_scenes, multi_rel_outputs, threshold, score, n_labels, max_rel,
                                 obj_probs, rel_probs)
    lib = L.load()
    n, c = obj_logits.shape
    edges, batch_ids, n_scenes, mode, n_labels, max_rel = _gd_args(obj_logits, rel, edges, batch_ids, n_scenes, score, n_labels, max_rel)
    e, r = rel.shape
    dev = obj_logits.device
    thr = decode_thresholds(threshold, r, dev)
    r_probs = _rel_probs(rel, rel_probs, multi_rel_outputs, exp_probs)
    obj_probs = softmax_rows(obj_logits.float()) if obj_probs is None else obj_probs.float().contiguous()
    labels = torch.empty(n, n_labels, dtype=torch.int32, device=dev)
    label_probs = torch.empty(n, n_labels, dtype=torch.float32, device=dev)
    rels = torch.empty(n_scenes, max_rel, 2, dtype=torch.int32, device=dev)
    sc = torch.empty(n_scenes, max_rel, dtype=torch.float32, device=dev)
    n_valid = torch.empty(n_scenes, dtype=torch.int32, device=dev)
    n_total = torch.empty(n_scenes, dtype=torch.int32, device=dev)
    nbytes = int(lib.vlsat_graph_decode_scratch_bytes(e, c, r, n_scenes, n_labels, max_rel))
    scratch = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    L.check(lib.vlsat_graph_decode(obj_probs.data_ptr(), r_probs.data_ptr(), edges.data_ptr(), L.ptr(batch_ids), thr.data_ptr(), n, e, c,
                                   r, n_scenes, int(bool(multi_rel_outputs)), mode, n_labels, max_rel, scratch.data_ptr(),
                                   labels.data_ptr(), label_probs.data_ptr(), rels.data_ptr(), sc.data_ptr(), n_valid.data_ptr(),
                                   n_total.data_ptr(), L.stream_ptr()))
    return DecodedGraph(labels, label_probs, rels, sc, n_valid, n_total)


def _rel_probs(rel, rel_probs, multi_rel_outputs, exp):
    if rel_probs is not None:
        if rel_probs.shape != rel.shape:
            raise L.VlsatError("decode_graph: rel_probs must have the shape of rel")
        return rel_probs.float().contiguous()
    return rel.float().contiguous() if multi_rel_outputs else exp(rel)


def _eligible(rp: torch.Tensor, multi_rel_outputs: bool) -> torch.Tensor:
    """bool [E, R]: the cells the decode can assert at some threshold -- all of them for a multi-label model, the arg-max predicate
    of the row unless it is class 0 for a single-label one."""
    pick = torch.ones_like(rp, dtype=torch.bool)
    if not multi_rel_outputs and rp.shape[0]:
        best = rp.sort(dim=1, descending=True, stable=True).indices[:, 0]                # lowest index of the row maximum
        pick = torch.zeros_like(pick)
        pick[torch.arange(rp.shape[0], device=rp.device), best] = True
        pick[:, 0] = False                                                            # class 0 = none
    return pick


def _asserted(rp: torch.Tensor, thr: torch.Tensor, multi_rel_outputs: bool) -> torch.Tensor:
    """bool [E, R]: the decisions of the decode on predicate probabilities ``rp``."""
    on = rp >= thr[None, :]
    if not multi_rel_outputs and rp.shape[0]:
        on = on & _eligible(rp, False)
    return on


@torch.no_grad()
def decode_graph_host(obj_logits, rel, edges, batch_ids, n_scenes, multi_rel_outputs=True, threshold=0.5, score="rel", n_labels=3,
                      max_rel=1024, obj_probs=None, rel_probs=None) -> DecodedGraph:
    """``decode_graph`` stated in PyTorch on whatever device the inputs are (the role ``scene_graph_topk_host`` plays for the
    top-K list).  Exact; for CPU tests and devices without the HIP library."""
    n, c = obj_logits.shape
    edges, batch_ids, n_scenes, mode, n_labels, max_rel = _gd_args(obj_logits, rel, edges, batch_ids, n_scenes, score, n_labels, max_rel)
    e, r = rel.shape
    dev = obj_logits.device
    thr = decode_thresholds(threshold, r, dev)
    rp = _rel_probs(rel, rel_probs, multi_rel_outputs, lambda x: x.float().exp().contiguous())
    probs = (torch.softmax(obj_logits.float(), -1) if obj_probs is None else obj_probs.float()).contiguous()
    sv, si = probs.sort(dim=1, descending=True, stable=True)                             # equal values: ascending class
    labels, label_probs = si[:, :n_labels].to(torch.int32).contiguous(), sv[:, :n_labels].contiguous()
    rels = torch.full((n_scenes, max_rel, 2), -1, dtype=torch.int32, device=dev)
    sc = torch.zeros(n_scenes, max_rel, dtype=torch.float32, device=dev)
    n_valid = torch.zeros(n_scenes, dtype=torch.int32, device=dev)
    n_total = torch.zeros(n_scenes, dtype=torch.int32, device=dev)
    if e == 0 or n_scenes == 0:
        return DecodedGraph(labels, label_probs, rels, sc, n_valid, n_total)
    a, b = edges[:, 0], edges[:, 1]
    scene = batch_ids[a] if batch_ids is not None else torch.zeros(e, dtype=torch.int64, device=dev)
    val = rp if mode == 0 else (label_probs[a, 0] * label_probs[b, 0])[:, None] * rp      # fl(fl(s * o) * r)
    on = _asserted(rp, thr, multi_rel_outputs)
    ed, pr = on.nonzero(as_tuple=True)                                                # (edge, predicate) ascending
    v = val[ed, pr]
    for s in range(n_scenes):
        sel = scene[ed] == s
        es, ps, vs = ed[sel], pr[sel], v[sel]
        order = vs.argsort(descending=True, stable=True)[:max_rel]
        k = order.numel()
        n_total[s], n_valid[s] = es.numel(), k
        rels[s, :k, 0], rels[s, :k, 1], sc[s, :k] = es[order].int(), ps[order].int(), vs[order]
    return DecodedGraph(labels, label_probs, rels, sc, n_valid, n_total)


def decode_counts_width(n_rel: int) -> int:
    """Fields of the decode counts: per predicate tp, fp, fn, then nodes, nodes whose top-1 label is right."""
    return 3 * n_rel + 2


def _gt_hot(gt_rel: torch.Tensor, e: int, r: int, multi_rel_outputs: bool) -> torch.Tensor:
    """bool [E, R] ground truth of the counts: the multi-hot target (== 1), or a single label's one-hot with 0 = none."""
    if multi_rel_outputs:
        if gt_rel.shape != (e, r):
            raise L.VlsatError("decode_counts: gt_rel must be the multi-hot [E,R] target")
        return gt_rel == 1
    if gt_rel.shape != (e,):
        raise L.VlsatError("decode_counts: gt_rel must be the [E] label vector of a single-label model")
    k = torch.arange(r, device=gt_rel.device)[None, :]
    return (gt_rel[:, None] == k) & (k != 0)


def decode_counts(obj_logits: torch.Tensor, rel: torch.Tensor, gt_cls: torch.Tensor, gt_rel: torch.Tensor,
                  multi_rel_outputs: bool = True, threshold=0.5, obj_probs: torch.Tensor | None = None,
                  counts: torch.Tensor | None = None, rel_probs: torch.Tensor | None = None) -> torch.Tensor:
    """The decisions of ``decode_graph`` before its cap, counted against ground truth: int64 [3 R + 2] -- per predicate tp, fp, fn
    at 3 k + {0, 1, 2}, then nodes and nodes whose top-1 label is ``gt_cls``.  ``gt_rel``: the int64 multi-hot [E, R] target, or
    int64 [E] (0 = none) for a single-label model.  Additive: pass ``counts`` (device int64, zeroed once) to accumulate over
    batches, from several streams if need be.  ``evaluate.graph_quality`` turns the sums into precision / recall / F1."""
    if not obj_logits.is_cuda:
        out = decode_counts_host(obj_logits, rel, gt_cls, gt_rel, multi_rel_outputs, threshold, obj_probs, rel_probs)
        return out if counts is None else counts.add_(out)
    lib = L.load()
    n, c = obj_logits.shape
    e, r = rel.shape
    dev = obj_logits.device
    thr = decode_thresholds(threshold, r, dev)
    gt_rel = gt_rel.to(torch.int64).contiguous()
    if gt_rel.shape != ((e, r) if multi_rel_outputs else (e,)):
        raise L.VlsatError("decode_counts: gt_rel must be multi-hot [E,R] (multi-label) or [E] (single label)")
    gt_cls = gt_cls.to(torch.int64).contiguous().view(-1)
    if gt_cls.numel() != n:
        raise L.VlsatError("decode_counts: gt_cls must hold one class per node")
    r_probs = _rel_probs(rel, rel_probs, multi_rel_outputs, exp_probs)
    obj_probs = softmax_rows(obj_logits.float()) if obj_probs is None else obj_probs.float().contiguous()
    if counts is None:
        counts = torch.zeros(decode_counts_width(r), dtype=torch.int64, device=dev)
    elif counts.dtype != torch.int64 or counts.numel() != decode_counts_width(r) or not counts.is_contiguous() or counts.device != dev:
        raise L.VlsatError(f"decode_counts: counts must be a contiguous int64 [{decode_counts_width(r)}] tensor on the inputs' device")
    L.check(lib.vlsat_graph_decode_counts(obj_probs.data_ptr(), r_probs.data_ptr(), gt_cls.data_ptr(), gt_rel.data_ptr(), thr.data_ptr(),
                                          n, e, c, r, int(bool(multi_rel_outputs)), counts.data_ptr(), L.stream_ptr()))
    return counts


@torch.no_grad()
def decode_counts_host(obj_logits, rel, gt_cls, gt_rel, multi_rel_outputs=True, threshold=0.5, obj_probs=None,
                       rel_probs=None) -> torch.Tensor:
    """``decode_counts`` stated in PyTorch."""
    n, c = obj_logits.shape
    e, r = rel.shape
    dev = obj_logits.device
    thr = decode_thresholds(threshold, r, dev)
    rp = _rel_probs(rel, rel_probs, multi_rel_outputs, lambda x: x.float().exp())
    probs = torch.softmax(obj_logits.float(), -1) if obj_probs is None else obj_probs.float()
    on = _asserted(rp, thr, multi_rel_outputs)
    hot = _gt_hot(gt_rel.to(torch.int64), e, r, multi_rel_outputs)
    out = torch.zeros(decode_counts_width(r), dtype=torch.int64, device=dev)
    out[0:3 * r:3], out[1:3 * r:3], out[2:3 * r:3] = (on & hot).sum(0), (on & ~hot).sum(0), (hot & ~on).sum(0)
    top1 = probs.sort(dim=1, descending=True, stable=True).indices[:, 0] if n else torch.zeros(0, dtype=torch.int64, device=dev)
    out[3 * r], out[3 * r + 1] = n, (top1 == gt_cls.to(torch.int64).view(-1)).sum()
    return out


# ---- score histograms: the counts of every threshold k / bins at once (csrc/calibration.hip, include/vlsat_calib.h) ----
CALIB_MIN_BINS, CALIB_MAX_BINS = 16, 4096


def _check_bins(bins) -> int:
    bins = int(bins)
    if not CALIB_MIN_BINS <= bins <= CALIB_MAX_BINS or bins & (bins - 1):
        raise L.VlsatError(f"score_histograms: bins must be a power of two in {CALIB_MIN_BINS}..{CALIB_MAX_BINS}")
    return bins


class ScoreTables:
    """The additive int64 tables of ``score_histograms`` (rule: include/vlsat_calib.h), views of ONE contiguous ``buffer`` so that a
    single all-reduce takes them whole: ``rel`` [R, 2, bins + 1] (predicate, ground truth not-hot / hot, column), ``obj``
    [2, bins + 1] (top-1 wrong / right, column of the top-1 probability), ``confusion`` [C, C] ([gt_cls, top-1]).  Column b < bins
    holds the scores in [b / bins, (b + 1) / bins) (the last one everything from there up); column ``bins`` the cells the decode
    asserts at no threshold (NaN, negative, or not the pick of a single-label row)."""
    __slots__ = ("buffer", "rel", "obj", "confusion", "bins")

    def __init__(self, n_rel: int, n_obj: int, bins: int = 1024, device=None, buffer: torch.Tensor | None = None):
        self.bins = _check_bins(bins)
        w, n_rel, n_obj = self.bins + 1, int(n_rel), int(n_obj)
        sizes = (n_rel * 2 * w, 2 * w, n_obj * n_obj)
        if buffer is None:
            buffer = torch.zeros(sum(sizes), dtype=torch.int64, device=device)
        if buffer.dtype != torch.int64 or buffer.dim() != 1 or buffer.numel() != sum(sizes) or not buffer.is_contiguous():
            raise L.VlsatError(f"ScoreTables: the buffer must be a contiguous int64 vector of {sum(sizes)} entries")
        self.buffer = buffer
        a, b, c = buffer.split(sizes)
        self.rel, self.obj, self.confusion = a.view(n_rel, 2, w), b.view(2, w), c.view(n_obj, n_obj)

    def cpu(self) -> "ScoreTables":
        return ScoreTables(self.rel.shape[0], self.confusion.shape[0], self.bins, buffer=self.buffer.cpu())

    def suffix_sums(self) -> torch.Tensor:
        """int64 [R, 2, bins]: entry [r, h, k] = the cells of predicate r and ground truth h in columns k..bins - 1, i.e. the cells
        the decode asserts at threshold k / bins (h = 1: tp, h = 0: fp)."""
        return self.rel[:, :, :self.bins].flip(-1).cumsum(-1).flip(-1)

    def k_vector(self, k_or_thresholds) -> torch.Tensor:
        """``k_or_thresholds`` as the int64 [R] vector of columns (on the host): an integer k or one per predicate, or floating
        point thresholds that are multiples of 1 / bins (anything else cannot be read off the table and raises)."""
        r = self.rel.shape[0]
        t = torch.as_tensor(k_or_thresholds).detach().cpu().reshape(-1)
        if t.is_floating_point():
            x = t.double() * self.bins
            if not bool((x == x.round()).all()):
                raise ValueError(f"ScoreTables: a threshold must be a multiple of 1 / {self.bins}")
            t = x.round()
        t = t.to(torch.int64)
        if t.numel() == 1 and r != 1:
            t = t.expand(r)
        if t.numel() != r or not bool(((t >= 0) & (t < self.bins)).all()):
            raise ValueError(f"ScoreTables: one column in 0..{self.bins - 1} (or threshold in [0, 1)) per predicate ({r})")
        return t.contiguous()

    def counts_at(self, k_or_thresholds) -> torch.Tensor:
        """int64 [3 R], tp / fp / fn of predicate r at 3 r + {0, 1, 2}: exactly what ``decode_counts`` counts at threshold
        k / bins (its first 3 R fields)."""
        k = self.k_vector(k_or_thresholds).to(self.rel.device)
        s = self.suffix_sums().gather(2, k[:, None, None].expand(-1, 2, 1))[:, :, 0]                # [R, 2]
        tp, fp = s[:, 1], s[:, 0]
        return torch.stack([tp, fp, self.rel[:, 1].sum(-1) - tp], 1).reshape(-1)


def _score_columns(p: torch.Tensor, eligible, bins: int) -> torch.Tensor:
    """int64 columns of fp32 scores ``p`` under the bin rule of include/vlsat_calib.h (one fp32 multiply, floor, clamp)."""
    ok = (p >= 0) & eligible
    x = torch.where(ok, p, torch.zeros_like(p)) * bins
    return torch.where(ok, x.floor().clamp(max=bins - 1).to(torch.int64), torch.full_like(x, bins, dtype=torch.int64))


def score_histograms(obj_logits: torch.Tensor, rel: torch.Tensor, gt_cls: torch.Tensor, gt_rel: torch.Tensor,
                     multi_rel_outputs: bool = True, bins: int = 1024, obj_probs: torch.Tensor | None = None,
                     rel_probs: torch.Tensor | None = None, tables: ScoreTables | None = None) -> ScoreTables:
    """Histograms of a batch's scores against ground truth (``ScoreTables``): the tp / fp / fn of ``decode_counts`` at EVERY
    threshold k / bins in one pass (``tables.counts_at(k)``, exact), the reliability table of the object head and its confusion
    matrix.  ``bins``: a power of two in 16..4096.  Inputs exactly as for ``decode_counts``: ``rel`` holds log-probabilities for a
    single-label model, ``rel_probs`` overrides it, ``gt_rel`` is the int64 multi-hot [E, R] target or int64 [E] (0 = none).  A node
    whose ``gt_cls`` is outside [0, C) is in neither node table.  Additive: pass ``tables`` (zeroed once) to accumulate over batches,
    from several streams if need be.  ``evaluate.operating_points`` turns the sums into PR curves, AP, per-predicate thresholds
    and calibration figures.  Device tensors: the HIP kernel, asynchronous, no host round trip.  CPU tensors:
    ``score_histograms_host``."""
    bins = _check_bins(bins)
    n, c = obj_logits.shape
    e, r = rel.shape
    if tables is not None and (tables.bins != bins or tables.rel.shape[0] != r or tables.confusion.shape[0] != c
                               or tables.buffer.device != obj_logits.device):
        raise L.VlsatError("score_histograms: tables must have the call's bins, predicate and class counts and live on its device")
    if not obj_logits.is_cuda:
        out = score_histograms_host(obj_logits, rel, gt_cls, gt_rel, multi_rel_outputs, bins, obj_probs, rel_probs)
        if tables is None:
            return out
        tables.buffer.add_(out.buffer)
        return tables
    lib = L.load()
    if not 1 <= c <= 1024 or not 1 <= r <= 32:
        raise L.VlsatError("score_histograms: 1..1024 object and 1..32 relation classes")
    gt_rel = gt_rel.to(torch.int64).contiguous()
    if gt_rel.shape != ((e, r) if multi_rel_outputs else (e,)):
        raise L.VlsatError("score_histograms: gt_rel must be multi-hot [E,R] (multi-label) or [E] (single label)")
    gt_cls = gt_cls.to(torch.int64).contiguous().view(-1)
    if gt_cls.numel() != n:
        raise L.VlsatError("score_histograms: gt_cls must hold one class per node")
    r_probs = _rel_probs(rel, rel_probs, multi_rel_outputs, exp_probs)
    obj_probs = softmax_rows(obj_logits.float()) if obj_probs is None else obj_probs.float().contiguous()
    if tables is None:
        tables = ScoreTables(r, c, bins, obj_logits.device)
    L.check(lib.vlsat_score_hist(obj_probs.data_ptr(), r_probs.data_ptr(), gt_cls.data_ptr(), gt_rel.data_ptr(), n, e, c, r,
                                 int(bool(multi_rel_outputs)), bins, tables.rel.data_ptr(), tables.obj.data_ptr(),
                                 tables.confusion.data_ptr(), L.stream_ptr()))
    return tables


@torch.no_grad()
def score_histograms_host(obj_logits, rel, gt_cls, gt_rel, multi_rel_outputs=True, bins=1024, obj_probs=None,
                          rel_probs=None) -> ScoreTables:
    """``score_histograms`` stated in PyTorch, with the ground truth (``_gt_hot``), the probabilities (``_rel_probs``) and the
    single-label pick (``_eligible``) of the decode's own restatement."""
    bins = _check_bins(bins)
    n, c = obj_logits.shape
    e, r = rel.shape
    dev = obj_logits.device
    w = bins + 1
    rp = _rel_probs(rel, rel_probs, multi_rel_outputs, lambda x: x.float().exp())
    probs = torch.softmax(obj_logits.float(), -1) if obj_probs is None else obj_probs.float()
    hot = _gt_hot(gt_rel.to(torch.int64), e, r, multi_rel_outputs)
    out = ScoreTables(r, c, bins, dev)
    col = _score_columns(rp, _eligible(rp, multi_rel_outputs), bins)
    cell = (torch.arange(r, device=dev)[None, :] * 2 + hot.to(torch.int64)) * w + col
    out.rel.view(-1).add_(torch.bincount(cell.reshape(-1), minlength=r * 2 * w))
    gt = gt_cls.to(torch.int64).view(-1)
    top1 = probs.sort(dim=1, descending=True, stable=True).indices[:, 0]                 # lowest index of the row maximum
    conf = probs.gather(1, top1[:, None])[:, 0]
    valid = (gt >= 0) & (gt < c)
    ocell = (top1 == gt).to(torch.int64) * w + _score_columns(conf, True, bins)
    out.obj.view(-1).add_(torch.bincount(ocell[valid], minlength=2 * w))
    out.confusion.view(-1).add_(torch.bincount((gt * c + top1)[valid], minlength=c * c))
    return out


# ---- segments of an over-segmentation merged into objects along "same part" edges ------------------------------------------------------
_MG_FIELDS = ("root", "object", "n_objects", "totals", "member_ptr", "members", "obj_probs", "obj_weight", "obj_batch_ids",
              "edge_to_pair", "pair_edges", "pair_count", "pair_probs")


class MergedGraph:
    """The objects an over-segmentation's "same part" links assert, and the batch's graph folded onto them (include/vlsat.h,
    vlsat_merge_segments).  Per segment (node row): ``root`` int32 [N] the lowest row of its component, ``object`` int32 [N] its
    object.  Per scene ``n_objects`` int32 [S]; ``totals`` int32 [2] = (M, E').  ``member_ptr`` int32 / ``members`` int32 [N]: CSR
    of the segments of every object in ascending row.  Per object ``obj_probs`` float32 [M, C] (weighted mean of the members'
    class probabilities), ``obj_weight`` float32 [M], ``obj_batch_ids`` int64 [M].  Per input edge ``edge_to_pair`` int32 [E] (-1:
    inside one object, or dropped).  Per merged edge ``pair_edges`` int64 [E', 2] (object rows), ``pair_count`` int32 [E'],
    ``pair_probs`` float32 [E', R] (maximum over the folded edges).  ``trimmed``: the per-object / per-pair tables are cut to
    M / E' rows (``member_ptr`` to M + 1); otherwise they are full size ([N] / [E] rows; rows past the end hold 0 / -1,
    ``member_ptr`` N) and nothing was read back."""
    __slots__ = _MG_FIELDS + ("trimmed",)
    _FIELDS = _MG_FIELDS
    _OBJECT_TABLES = ("obj_probs", "obj_weight", "obj_batch_ids")

    def __init__(self, trimmed=False, **tables):
        for k in self._FIELDS:
            setattr(self, k, tables[k])
        self.trimmed = bool(trimmed)

    def trim(self) -> "MergedGraph":
        """The tables cut to M objects and E' merged edges.  Reads ``totals`` back: ONE host synchronisation."""
        if self.trimmed:
            return self
        m, e = (int(x) for x in self.totals.tolist())
        t = {k: getattr(self, k) for k in self._FIELDS}
        for k in self._OBJECT_TABLES:
            t[k] = t[k][:m]
        t["member_ptr"] = t["member_ptr"][:m + 1]
        for k in ("pair_edges", "pair_count", "pair_probs"):
            t[k] = t[k][:e]
        return type(self)(True, **t)

    def cpu(self) -> "MergedGraph":
        return type(self)(self.trimmed, **{k: getattr(self, k).cpu() for k in self._FIELDS})

    def scene(self, s: int, edges=None) -> "MergedGraph":
        """Scene ``s`` as a one-scene graph with its own segment, object and pair rows counted from 0.  ``edges`` = (first, end)
        rows of the scene in the batch's edge list (None: ``edge_to_pair`` is left empty).  Reads the counts back."""
        g = self.trim()
        n_obj = g.n_objects.tolist()
        o0 = sum(n_obj[:s])
        o1 = o0 + n_obj[s]
        ptr = g.member_ptr.tolist()
        n0, n1 = (ptr[o0], ptr[o1]) if len(ptr) > 1 else (0, 0)
        src = g.pair_edges[:, 0] if g.pair_edges.numel() else g.pair_edges.new_zeros(0)
        rows = ((src >= o0) & (src < o1)).nonzero().view(-1)
        p0 = int(rows[0]) if rows.numel() else 0
        e2p = g.edge_to_pair[0:0] if edges is None else g.edge_to_pair[int(edges[0]):int(edges[1])]
        dev = g.totals.device
        return MergedGraph(True, root=g.root[n0:n1] - n0, object=g.object[n0:n1] - o0, n_objects=g.n_objects[s:s + 1],
                           totals=torch.tensor([o1 - o0, rows.numel()], dtype=torch.int32, device=dev),
                           member_ptr=g.member_ptr[o0:o1 + 1] - n0, members=g.members[n0:n1] - n0, obj_probs=g.obj_probs[o0:o1],
                           obj_weight=g.obj_weight[o0:o1], obj_batch_ids=torch.zeros_like(g.obj_batch_ids[o0:o1]),
                           edge_to_pair=torch.where(e2p >= 0, e2p - p0, e2p), pair_edges=g.pair_edges[rows] - o0,
                           pair_count=g.pair_count[rows], pair_probs=g.pair_probs[rows])

    def decode(self, multi_rel_outputs: bool = True, **decode_args) -> "DecodedGraph":
        """``decode_graph`` on the merged tables (``obj_probs=`` / ``rel_probs=``): one label per object, the asserted predicates per
        merged edge; ``threshold``, ``score``, ``n_labels``, ``max_rel`` as there.  The graph's ``edge`` rows index ``pair_edges``.
        Merged edges keep the input's scene order, so an edge list grouped by scene gives pairs grouped by scene."""
        g = self.trim()
        fn = decode_graph if g.obj_probs.is_cuda else decode_graph_host
        return fn(g.obj_probs, g.pair_probs, g.pair_edges, g.obj_batch_ids, int(g.n_objects.numel()), multi_rel_outputs,
                  obj_probs=g.obj_probs, rel_probs=g.pair_probs, **decode_args)


def _mg_args(obj_logits, rel, edges, batch_ids, n_scenes, same_part, threshold, weights):
    if obj_logits.dim() != 2 or rel.dim() != 2:
        raise L.VlsatError("merge_segments: obj_logits must be [N,C] and rel [E,R]")
    n, c = obj_logits.shape
    e, r = rel.shape
    n_scenes, same_part, threshold = int(n_scenes), int(same_part), float(threshold)
    if not 1 <= c <= 1024 or not 1 <= r <= 32:
        raise L.VlsatError("merge_segments: 1..1024 object and 1..32 relation classes")
    if not 0 <= same_part < r:
        raise L.VlsatError(f"merge_segments: same_part must be a predicate class in [0, {r})")
    if threshold != threshold:
        raise L.VlsatError("merge_segments: threshold is NaN")
    if n_scenes < 0 or (n_scenes > 1 and batch_ids is None) or (n > 0 and n_scenes < 1):
        raise L.VlsatError("merge_segments: batch_ids is required for more than one scene (and nodes need a scene)")
    edges = edges.to(torch.int64).contiguous().view(-1, 2)
    if edges.shape[0] != e:
        raise L.VlsatError("merge_segments: rel must be [E,R] and edges [E,2]")
    if batch_ids is not None:
        batch_ids = batch_ids.to(torch.int64).contiguous().view(-1)
        if batch_ids.numel() != n:
            raise L.VlsatError("merge_segments: batch_ids must hold one scene per node")
    if weights is not None:
        weights = weights.to(device=obj_logits.device, dtype=torch.float32).contiguous().view(-1)
        if weights.numel() != n:
            raise L.VlsatError("merge_segments: weights must hold one value per node")
    return edges, batch_ids, n_scenes, same_part, threshold, weights


def merge_segments(obj_logits: torch.Tensor, rel: torch.Tensor, edges: torch.Tensor, batch_ids: torch.Tensor | None, n_scenes: int,
                   same_part: int, threshold: float = 0.5, mutual: bool = False, weights: torch.Tensor | None = None,
                   multi_rel_outputs: bool = True, obj_probs: torch.Tensor | None = None, rel_probs: torch.Tensor | None = None,
                   trim: bool = True) -> MergedGraph:
    """The segments of an over-segmentation merged into objects: segments joined by an edge whose predicate ``same_part`` has
    probability >= ``threshold`` (``mutual``: in both directions) form one object -- connected components, the lowest row as root
    -- the members' class probabilities are pooled as a mean weighted by ``weights`` (``points_per_instance``; None: all 1), and
    every edge between two objects folds onto the ordered pair of objects with the maximum of the predicate probabilities
    (include/vlsat.h, vlsat_merge_segments, states the rule and its orders).  Probabilities are derived as ``decode_graph``
    derives them.  Device tensors: the HIP kernels, asynchronous; ``trim=True`` then reads the two totals back -- the ONE host
    synchronisation -- and cuts the tables to M objects / E' merged edges, ``trim=False`` leaves them full size and reads nothing.
    CPU tensors: ``merge_segments_host``."""
    if not obj_logits.is_cuda:
        return merge_segments_host(obj_logits, rel, edges, batch_ids, n_scenes, same_part, threshold, mutual, weights, multi_rel_outputs,
                                   obj_probs, rel_probs, trim)
    lib = L.load()
    n, c = obj_logits.shape
    e, r = rel.shape
    edges, batch_ids, n_scenes, same_part, threshold, weights = _mg_args(obj_logits, rel, edges, batch_ids, n_scenes, same_part, threshold,
                                                                         weights)
    dev = obj_logits.device
    r_probs = _rel_probs(rel, rel_probs, multi_rel_outputs, exp_probs)
    probs = softmax_rows(obj_logits.float()) if obj_probs is None else obj_probs.float().contiguous()
    i32 = dict(dtype=torch.int32, device=dev)
    t = {"root": torch.empty(n, **i32), "object": torch.empty(n, **i32), "n_objects": torch.empty(n_scenes, **i32),
         "totals": torch.empty(2, **i32), "member_ptr": torch.empty(n + 1, **i32), "members": torch.empty(n, **i32),
         "obj_probs": torch.empty(n, c, dtype=torch.float32, device=dev), "obj_weight": torch.empty(n, dtype=torch.float32, device=dev),
         "obj_batch_ids": torch.empty(n, dtype=torch.int64, device=dev), "edge_to_pair": torch.empty(e, **i32),
         "pair_edges": torch.empty(e, 2, dtype=torch.int64, device=dev), "pair_count": torch.empty(e, **i32),
         "pair_probs": torch.empty(e, r, dtype=torch.float32, device=dev)}
    nbytes = int(lib.vlsat_merge_segments_scratch_bytes(n, e, c, r, n_scenes))
    if nbytes == 0:
        raise L.VlsatError("merge_segments: sizes out of range (E <= 2^26, E * R and N * C below 2^31)")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    L.check(lib.vlsat_merge_segments(probs.data_ptr(), r_probs.data_ptr(), edges.data_ptr(), L.ptr(batch_ids), L.ptr(weights), n, e, c, r,
                                     n_scenes, same_part, threshold, int(bool(mutual)), scratch.data_ptr(),
                                     *(t[k].data_ptr() for k in _MG_FIELDS), L.stream_ptr()))
    g = MergedGraph(False, **t)
    return g.trim() if trim else g


@torch.no_grad()
def merge_segments_host(obj_logits, rel, edges, batch_ids, n_scenes, same_part, threshold=0.5, mutual=False, weights=None,
                        multi_rel_outputs=True, obj_probs=None, rel_probs=None, trim=True) -> MergedGraph:
    """``merge_segments`` stated in numpy float32 with the kernel's operations and orders: every table equal, the pooled
    probabilities bit for bit (the role ``decode_graph_host`` plays for ``decode_graph``).  Returns CPU tensors."""
    edges, batch_ids, n_scenes, same_part, threshold, weights = _mg_args(obj_logits, rel, edges, batch_ids, n_scenes, same_part, threshold,
                                                                         weights)
    n, c = obj_logits.shape
    e, r = rel.shape
    rp = _rel_probs(rel, rel_probs, multi_rel_outputs, lambda x: x.float().exp().contiguous()).cpu().numpy()
    probs = (torch.softmax(obj_logits.float(), -1) if obj_probs is None else obj_probs.float()).contiguous().cpu().numpy()
    ed = edges.cpu().numpy()
    bid = np.zeros(n, dtype=np.int64) if batch_ids is None else batch_ids.cpu().numpy()
    w = np.ones(n, dtype=np.float32) if weights is None else weights.cpu().numpy().astype(np.float32)
    a, b = (ed[:, 0], ed[:, 1]) if e else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    ok = (a >= 0) & (b >= 0) & (a < n) & (b < n) & (a != b)
    ok[ok] &= bid[a[ok]] == bid[b[ok]]                                          # an edge across scenes never links and is dropped
    link = ok & (rp[:, same_part] >= np.float32(threshold)) if e else ok
    if mutual and e:
        passed = set(zip(a[link].tolist(), b[link].tolist()))
        link = link & np.fromiter(((y, x) in passed for x, y in zip(a.tolist(), b.tolist())), dtype=bool, count=e)
    root = np.arange(n, dtype=np.int64)
    la, lb = a[link], b[link]
    while True:                                                                 # minimum label over links, to the fixed point
        new = root.copy()
        np.minimum.at(new, la, root[lb])
        np.minimum.at(new, lb, root[la])
        new = new[new]
        if (new == root).all():
            break
        root = new
    is_root = root == np.arange(n)
    number = np.cumsum(is_root) - 1
    obj = number[root] if n else np.zeros(0, np.int64)
    m = int(is_root.sum())
    order = np.argsort(obj, kind="stable")                                      # members: by object, ascending row inside
    count = np.bincount(obj, minlength=n) if n else np.zeros(0, np.int64)
    member_ptr = np.concatenate([[0], np.cumsum(count)]).astype(np.int32)
    out_probs = np.zeros((n, c), dtype=np.float32)
    out_w = np.zeros(n, dtype=np.float32)
    for k in range(int(count.max()) if n else 0):                               # the k-th member of every object that has one
        objs = np.nonzero(count > k)[0]
        i = order[member_ptr[objs] + k]
        out_probs[objs] = out_probs[objs] + w[i][:, None] * probs[i]            # fl(s + fl(w p))
        out_w[objs] = out_w[objs] + w[i]
    with np.errstate(invalid="ignore", divide="ignore"):
        out_probs[:m] = out_probs[:m] / out_w[:m, None]
    obj_bid = np.full(n, -1, dtype=np.int64)
    obj_bid[:m] = bid[np.nonzero(is_root)[0]]
    n_objects = np.bincount(obj_bid[:m], minlength=n_scenes)[:n_scenes].astype(np.int32) if n_scenes else np.zeros(0, np.int32)
    edge_to_pair = np.full(e, -1, dtype=np.int32)
    pair_edges = np.full((e, 2), -1, dtype=np.int64)
    pair_count = np.zeros(e, dtype=np.int32)
    pair_probs = np.zeros((e, r), dtype=np.float32)
    n_pairs = 0
    if e:
        oa, ob = obj[np.where(ok, a, 0)], obj[np.where(ok, b, 0)]
        rows = np.nonzero(ok & (oa != ob))[0]
        if rows.size:
            key = oa[rows] * np.int64(n) + ob[rows]
            _, first, inv = np.unique(key, return_index=True, return_inverse=True)
            rank = np.empty(first.size, dtype=np.int64)
            rank[np.argsort(first, kind="stable")] = np.arange(first.size)     # pairs in the order of their lowest edge row
            pair = rank[inv.reshape(-1)]
            n_pairs = first.size
            edge_to_pair[rows] = pair
            reps = rows[first]
            pair_edges[rank, 0], pair_edges[rank, 1] = oa[reps], ob[reps]
            np.add.at(pair_count, pair, 1)
            np.maximum.at(pair_probs, pair, rp[rows])
    t = {"root": root.astype(np.int32), "object": obj.astype(np.int32), "n_objects": n_objects,
         "totals": np.asarray([m, n_pairs], dtype=np.int32), "member_ptr": member_ptr, "members": order.astype(np.int32),
         "obj_probs": out_probs, "obj_weight": out_w, "obj_batch_ids": obj_bid, "edge_to_pair": edge_to_pair, "pair_edges": pair_edges,
         "pair_count": pair_count, "pair_probs": pair_probs}
    g = MergedGraph(False, **{k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in t.items()})
    return g.trim() if trim else g


# ---- the rows of a batch of splits fused into one graph per scan (csrc/scene_split.hip; the rule is stated in include/vlsat_split.h) ----
class FusedGraph(MergedGraph):
    """One graph per scan from the predictions of its splits (``fuse_splits``): the fields of ``MergedGraph`` with the same ``trim``
    semantics -- an "object" is a scan-level instance, its members the rows (of any split) that carry its id, ``root`` the lowest such
    row, objects in ascending id, ``pair_edges`` sorted by (source, target) -- plus ``obj_ids`` int32 [M], the instance id of every
    object (what ``scene_graph.to_annotation`` takes as ``node_ids``; ``scene_graph.merged_node_ids(g, row_instance)`` gives the same
    list).  ``n_objects`` int32 [1]; ``obj_batch_ids`` zeros.  A row whose id is outside the id table has ``root = object = -1``."""
    __slots__ = ("obj_ids",)
    _FIELDS = _MG_FIELDS + ("obj_ids",)
    _OBJECT_TABLES = MergedGraph._OBJECT_TABLES + ("obj_ids",)

    def scene(self, s: int = 0, edges=None) -> "FusedGraph":
        if int(s) != 0:
            raise L.VlsatError("FusedGraph: one scan per graph")
        return self.trim()

    def node_ids(self) -> list:
        return [int(i) for i in self.trim().obj_ids.tolist()]


def _fs_args(obj_logits, rel, edges, row_instance, weights, map_size):
    if obj_logits.dim() != 2 or rel.dim() != 2:
        raise L.VlsatError("fuse_splits: obj_logits must be [N,C] and rel [E,R]")
    n, c = obj_logits.shape
    e, r = rel.shape
    if not 1 <= c <= 1024 or not 1 <= r <= 32:
        raise L.VlsatError("fuse_splits: 1..1024 object and 1..32 relation classes")
    if n > 16384:
        raise L.VlsatError("fuse_splits: at most 16384 rows per call")
    edges = edges.to(torch.int64).contiguous().view(-1, 2)
    if edges.shape[0] != e:
        raise L.VlsatError("fuse_splits: rel must be [E,R] and edges [E,2]")
    if torch.is_tensor(row_instance) and row_instance.is_cuda:                    # device ids: never read back; the table bounds them
        ids = row_instance.to(torch.int32).contiguous().view(-1)
        map_size = 65536 if map_size is None else map_size
    else:
        host = np.asarray(row_instance.cpu() if torch.is_tensor(row_instance) else list(row_instance), dtype=np.int64).reshape(-1)
        if map_size is None:                                                      # host ids: checked, and the table sized from them
            if host.size and (host.min() < 0 or host.max() >= (1 << 24)):
                raise L.VlsatError("fuse_splits: instance ids must be integers in [0, 2^24)")
            map_size = max(65536, int(host.max()) + 1 if host.size else 1)
        ids = torch.from_numpy(np.clip(host, -1, 1 << 24).astype(np.int32))       # (an explicit map_size is taken as given)
    if ids.numel() != n:
        raise L.VlsatError("fuse_splits: row_instance must hold one id per row")
    if not 1 <= int(map_size) <= (1 << 24):
        raise L.VlsatError("fuse_splits: map_size must be in 1..2^24")
    if weights is not None:
        weights = weights.to(device=obj_logits.device, dtype=torch.float32).contiguous().view(-1)
        if weights.numel() != n:
            raise L.VlsatError("fuse_splits: weights must hold one value per row")
    return edges, ids, weights, int(map_size)


_FG_FIELDS = FusedGraph._FIELDS


def fuse_splits(obj_logits: torch.Tensor, rel: torch.Tensor, edges: torch.Tensor, row_instance, weights: torch.Tensor | None = None,
                multi_rel_outputs: bool = True, obj_probs: torch.Tensor | None = None, rel_probs: torch.Tensor | None = None,
                trim: bool = True, map_size: int | None = None) -> FusedGraph:
    """The predictions of a scan's splits (``scan.split_scan`` -> ``prepare_scan`` per group -> one batched forward) fused into one
    graph: the rows that carry the same scan-level instance id (``row_instance`` [N]: the batches' ``instance_ids`` concatenated) are
    one object, objects in ascending id; the rows' class probabilities are pooled as a mean weighted by ``weights``
    (``points_per_instance``; None: all 1) in ascending row order; every edge folds onto the ordered pair of objects with the maximum
    of the predicate probabilities over all occurrences, whatever split they come from; pairs are listed by (source, target)
    ascending, each with its number of occurrences (include/vlsat_split.h, vlsat_fuse_splits).  Probabilities are derived as
    ``merge_segments`` derives them.  Device tensors: the HIP kernels, asynchronous; ``trim=True`` then reads the two totals back --
    the ONE host synchronisation -- ``trim=False`` leaves the tables full size and reads nothing.  ``map_size=None``:
    ``row_instance`` on the host is range-checked and sizes the id table, on the device the table has 65536 entries; an explicit
    ``map_size`` is taken as given, and an id outside [0, ``map_size``) belongs to no object, wherever the ids live.  CPU tensors:
    ``fuse_splits_host``."""
    if not obj_logits.is_cuda:
        return fuse_splits_host(obj_logits, rel, edges, row_instance, weights, multi_rel_outputs, obj_probs, rel_probs, trim, map_size)
    lib = L.load()
    n, c = obj_logits.shape
    e, r = rel.shape
    edges, ids, weights, map_size = _fs_args(obj_logits, rel, edges, row_instance, weights, map_size)
    dev = obj_logits.device
    ids = ids.to(dev)
    r_probs = _rel_probs(rel, rel_probs, multi_rel_outputs, exp_probs)
    probs = softmax_rows(obj_logits.float()) if obj_probs is None else obj_probs.float().contiguous()
    i32 = dict(dtype=torch.int32, device=dev)
    t = {"root": torch.empty(n, **i32), "object": torch.empty(n, **i32), "n_objects": torch.empty(1, **i32),
         "totals": torch.empty(2, **i32), "member_ptr": torch.empty(n + 1, **i32), "members": torch.empty(n, **i32),
         "obj_probs": torch.empty(n, c, dtype=torch.float32, device=dev), "obj_weight": torch.empty(n, dtype=torch.float32, device=dev),
         "obj_batch_ids": torch.empty(n, dtype=torch.int64, device=dev), "edge_to_pair": torch.empty(e, **i32),
         "pair_edges": torch.empty(e, 2, dtype=torch.int64, device=dev), "pair_count": torch.empty(e, **i32),
         "pair_probs": torch.empty(e, r, dtype=torch.float32, device=dev), "obj_ids": torch.empty(n, **i32)}
    nbytes = int(lib.vlsat_fuse_splits_scratch_bytes(n, e, c, r, map_size))
    if nbytes == 0:
        raise L.VlsatError("fuse_splits: sizes out of range (N <= 16384, E <= 2^26, E * R and N * C below 2^31)")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    L.check(lib.vlsat_fuse_splits(probs.data_ptr(), r_probs.data_ptr(), edges.data_ptr(), ids.data_ptr(), L.ptr(weights), n, e, c, r, map_size,
                                  scratch.data_ptr(), *(t[k].data_ptr() for k in _FG_FIELDS), L.stream_ptr()))
    g = FusedGraph(False, **t)
    return g.trim() if trim else g


@torch.no_grad()
def fuse_splits_host(obj_logits, rel, edges, row_instance, weights=None, multi_rel_outputs=True, obj_probs=None, rel_probs=None, trim=True,
                     map_size=None) -> FusedGraph:
    """``fuse_splits`` stated in numpy float32 with the kernel's operations and orders: every table equal, the pooled probabilities
    bit for bit.  Returns CPU tensors."""
    edges, ids, weights, map_size = _fs_args(obj_logits, rel, edges, row_instance, weights, map_size)
    n, c = obj_logits.shape
    e, r = rel.shape
    rp = _rel_probs(rel, rel_probs, multi_rel_outputs, lambda x: x.float().exp().contiguous()).cpu().numpy()
    probs = (torch.softmax(obj_logits.float(), -1) if obj_probs is None else obj_probs.float()).contiguous().cpu().numpy()
    ed = edges.cpu().numpy()
    inst = ids.cpu().numpy().astype(np.int64)
    w = np.ones(n, dtype=np.float32) if weights is None else weights.cpu().numpy().astype(np.float32)
    valid = (inst >= 0) & (inst < map_size)
    uniq, first, inv = np.unique(inst[valid], return_index=True, return_inverse=True)     # ascending ids; first = lowest row of each
    rows = np.nonzero(valid)[0]
    m = len(uniq)
    obj = np.full(n, -1, dtype=np.int64)
    obj[rows] = inv.reshape(-1)
    root = np.full(n, -1, dtype=np.int64)
    root[rows] = rows[first][inv.reshape(-1)]
    order = rows[np.argsort(obj[rows], kind="stable")]                                    # members: by object, ascending row inside
    count = np.bincount(obj[rows], minlength=n) if n else np.zeros(0, np.int64)
    member_ptr = np.concatenate([[0], np.cumsum(count)]).astype(np.int32)
    members = np.full(n, -1, dtype=np.int32)
    members[:len(order)] = order
    out_probs = np.zeros((n, c), dtype=np.float32)
    out_w = np.zeros(n, dtype=np.float32)
    for k in range(int(count.max()) if n else 0):                                         # the k-th member of every object that has one
        objs = np.nonzero(count > k)[0]
        i = order[member_ptr[objs] + k]
        out_probs[objs] = out_probs[objs] + w[i][:, None] * probs[i]                      # fl(s + fl(w p))
        out_w[objs] = out_w[objs] + w[i]
    with np.errstate(invalid="ignore", divide="ignore"):
        out_probs[:m] = out_probs[:m] / out_w[:m, None]
    obj_bid = np.full(n, -1, dtype=np.int64)
    obj_bid[:m] = 0
    obj_ids = np.full(n, -1, dtype=np.int32)
    obj_ids[:m] = uniq
    edge_to_pair = np.full(e, -1, dtype=np.int32)
    pair_edges = np.full((e, 2), -1, dtype=np.int64)
    pair_count = np.zeros(e, dtype=np.int32)
    pair_probs = np.zeros((e, r), dtype=np.float32)
    n_pairs = 0
    if e and n:
        a, b = ed[:, 0], ed[:, 1]
        ok = (a >= 0) & (b >= 0) & (a < n) & (b < n)
        oa, ob = obj[np.where(ok, a, 0)], obj[np.where(ok, b, 0)]
        hit = np.nonzero(ok & (oa >= 0) & (ob >= 0) & (oa != ob))[0]
        if hit.size:
            key, pair = np.unique(oa[hit] * np.int64(n) + ob[hit], return_inverse=True)   # sorted keys: (a, b) ascending
            pair = pair.reshape(-1)
            n_pairs = key.size
            edge_to_pair[hit] = pair
            pair_edges[:n_pairs, 0], pair_edges[:n_pairs, 1] = key // n, key % n
            np.add.at(pair_count, pair, 1)
            np.maximum.at(pair_probs, pair, rp[hit])
    t = {"root": root.astype(np.int32), "object": obj.astype(np.int32), "n_objects": np.asarray([m], dtype=np.int32),
         "totals": np.asarray([m, n_pairs], dtype=np.int32), "member_ptr": member_ptr, "members": members,
         "obj_probs": out_probs, "obj_weight": out_w, "obj_batch_ids": obj_bid, "edge_to_pair": edge_to_pair, "pair_edges": pair_edges,
         "pair_count": pair_count, "pair_probs": pair_probs, "obj_ids": obj_ids}
    g = FusedGraph(False, **{k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in t.items()})
    return g.trim() if trim else g


def _edges_list(edges):
    return [(int(x[0]), int(x[1])) for x in (edges.tolist() if torch.is_tensor(edges) else np.asarray(edges).tolist())]


def _recall_call(objs_pred, rels_pred, gt_rel, edges, multi_rel_outputs, topk, topk_each, use_clip, evaluate):
    """The counts row of one reference-style call (one scene, get_gt's list of (sub, obj, [predicates]))."""
    topk_list = list(topk) if isinstance(topk, (list, tuple)) else [topk]
    if any(k not in RECALL_K for k in topk_list):
        raise NotImplementedError(f"recallk: K must be among {RECALL_K}")
    if evaluate not in ("triplet", "rels"):
        raise NotImplementedError("evaluate type", evaluate)
    if topk_each == 1:
        gc = True
    elif topk_each >= max(topk_list):                                  # the candidate cap never binds
        gc = False
    else:
        raise NotImplementedError("recallk: topk_each must be 1 or at least max(topk)")
    variant = ("sgcls" if evaluate == "triplet" else "predcls") + ("_gc" if gc else "_ngc")
    objs_pred = torch.as_tensor(objs_pred)
    dev = objs_pred.device
    n, _ = objs_pred.shape
    if multi_rel_outputs:
        rel = torch.as_tensor(rels_pred).float()
    elif dev.type == "cpu":
        rel = torch.as_tensor(np.exp(np.asarray(rels_pred, dtype=np.float32)))  # the reference's np.exp
    else:
        rel = torch.as_tensor(rels_pred).float().exp()
    e, r = rel.shape
    el = _edges_list(edges)
    gt_cls = torch.zeros(n, dtype=torch.int64)
    hot = torch.zeros(e, r, dtype=torch.int64)
    for i, (sub, obj, rels) in enumerate(gt_rel):
        gt_cls[el[i][0]], gt_cls[el[i][1]] = int(sub), int(obj)
        for k in rels:
            hot[i, int(k)] = 1
    probs = torch.softmax(objs_pred.float(), -1) if use_clip else objs_pred.float().exp()
    ed = torch.tensor(el, dtype=torch.int64).view(-1, 2)
    row = recallk_counts(objs_pred.float(), rel.to(dev), gt_cls.to(dev), hot.to(dev), ed.to(dev), None, 1, True,
                         variants=(variant,), obj_probs=probs)[0].cpu().numpy()
    return row, variant, topk_list, r


def _row_recall(row, variant, r, topk_list):
    base = recallk_offset(variant, r)
    return [int(row[base + RECALL_K.index(k)]) for k in topk_list], int(row[0])


def evaluate_triplet_recallk(objs_pred, rels_pred, gt_rel, edges, multi_rel_outputs, topk, topk_each, use_clip=False,
                             evaluate='triplet'):
    """Drop-in for the reference's ``evaluate_triplet_recallk`` (eval_utils_recall.py): same arguments (``gt_rel`` is
    get_gt's list), same result -- numpy ``hits / #edges with a gt predicate`` per K (NaN when there is none)."""
    row, variant, topk_list, r = _recall_call(objs_pred, rels_pred, gt_rel, edges, multi_rel_outputs, topk, topk_each, use_clip,
                                              evaluate)
    correct_number, all_number = _row_recall(row, variant, r, topk_list)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.array(correct_number) / all_number


def evaluate_triplet_mrecallk(objs_pred, rels_pred, gt_rel, edges, multi_rel_outputs, topk, topk_each, use_clip=False,
                              evaluate='triplet'):
    """Drop-in for the reference's ``evaluate_triplet_mrecallk``: 26 rows of 3 per-predicate recalls (a hit edge counts for
    every predicate of its gt set; -1 for a predicate no edge has), the reference's fixed 26 x 3 shape included."""
    row, variant, topk_list, r = _recall_call(objs_pred, rels_pred, gt_rel, edges, multi_rel_outputs, topk, topk_each, use_clip,
                                              evaluate)
    base = recallk_offset(variant, r)
    correct = np.zeros((26, len(topk_list)), dtype=np.int64)
    all_pc = [0] * 26
    for j in range(min(26, r)):
        all_pc[j] = int(row[1 + j])
        for i, k in enumerate(topk_list):
            correct[j][i] = row[base + 3 + RECALL_K.index(k) * r + j]
    return [[correct[j][i] / all_pc[j] if all_pc[j] != 0 else -1 for i in range(3)] for j in range(26)]


def _process_val_recall(model, obj_points, obj_2d_feats, gt_cls, descriptor, gt_rel_cls, edge_indices, batch_ids, use_triplet,
                        mean: bool):
    outs = _forward_eval(model, obj_points, obj_2d_feats, descriptor, edge_indices, batch_ids)
    obj3, _, rel3, _ = outs
    multi = bool(getattr(getattr(model, "config", None), "multi_rel_outputs", True))
    r = rel3.shape[1]
    gt_hot = multihot_targets(gt_rel_cls, r)
    rk = eval_ranks(obj3, rel3, gt_cls, gt_hot, edge_indices, multi_rel_outputs=multi)
    np64 = lambda t: t.cpu().numpy().astype(np.int64)
    top_k_obj, top_k_rel = np64(rk["top_k_obj"]), np64(rk["top_k_rel"])
    if not use_triplet:
        z = np.array([0, 0, 0])
        return top_k_obj, top_k_obj, top_k_rel, top_k_rel, z, z, z, z
    # the whole call is ONE scene, as the reference's functions see it
    row = recallk_counts(obj3, rel3, gt_cls, gt_hot, edge_indices, None, 1, multi, obj_probs=rk["obj_probs"])[0].cpu().numpy()
    res = []
    for v in RECALL_VARIANTS:
        base = recallk_offset(v, r)
        if mean:
            res.append([[row[base + 3 + i * r + j] / row[1 + j] if j < r and row[1 + j] != 0 else -1 for i in range(3)]
                        for j in range(26)])
        else:
            with np.errstate(invalid="ignore", divide="ignore"):
                res.append(np.array([int(row[base + q]) for q in range(3)]) / int(row[0]))
    return (top_k_obj, top_k_obj, top_k_rel, top_k_rel, *res)


@torch.no_grad()
def process_val2(model, obj_points, obj_2d_feats, gt_cls, descriptor, gt_rel_cls, edge_indices, batch_ids=None, with_log=False,
                 use_triplet=False):
    """``Mmgnet.process_val2`` (reference SGFN_MMG/model_in21k.py:439-468): 3D object / predicate ranks (each twice, as the
    reference returns them) and the Recall@{20,50,100} of predcls_gc, predcls_ngc, sgcls_gc, sgcls_ngc on the 3D branch."""
    return _process_val_recall(model, obj_points, obj_2d_feats, gt_cls, descriptor, gt_rel_cls, edge_indices, batch_ids,
                               use_triplet, mean=False)


@torch.no_grad()
def process_val3(model, obj_points, obj_2d_feats, gt_cls, descriptor, gt_rel_cls, edge_indices, batch_ids=None, with_log=False,
                 use_triplet=False):
    """``Mmgnet.process_val3`` (model_in21k.py:470-500): as process_val2 with the per-predicate recalls of
    evaluate_triplet_mrecallk (26 x 3, -1 for absent predicates) in place of the recalls."""
    return _process_val_recall(model, obj_points, obj_2d_feats, gt_cls, descriptor, gt_rel_cls, edge_indices, batch_ids,
                               use_triplet, mean=True)
