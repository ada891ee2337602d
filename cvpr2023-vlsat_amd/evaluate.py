"""Scene-sharded evaluation loop: the MI355X counterpart of ``MMGNet.validation`` (reference
``src/model/model.py:181-362``) for the part that sits on top of the hot path.

Each rank walks its contiguous shard of the scene list, runs forward + ranking on its GPU
(``metrics.process_val``), and accumulates a fixed-length vector of hit COUNTS.  Counts are
additive over scenes, so ONE all-reduce(SUM) at the end (RCCL over xGMI; gloo in the CPU test)
gives exactly the numbers a single process would get from the concatenated rank lists
(``validation()`` concatenates and thresholds them, :214-242, :267-282); the per-predicate
counts reproduce ``get_mean_recall`` (eva_utils_acc.py:224-237) and ``compute_mean_predicate``
(model.py:364-388)."""
from __future__ import annotations

import contextlib
import itertools
from typing import Dict, Iterable, Optional

import numpy as np
import torch

from . import dist as vdist
from .metrics import RECALL_K as _RK_K, RECALL_VARIANTS as _RK_VARIANTS, recallk_offset

N_REL = 26
# layout of the metrics vector (fp64): see fields()
_OBJ_K, _REL_K, _TRI_K = (1, 5, 10), (1, 3, 5), (50, 100)


def fields(n_rel: int = N_REL):
    f = ["scenes"]
    # get_mean_recall loops `range(int(cls_matrix.max()))` with the max taken over the WHOLE matrix
    # (object classes and ranks included): class c counts iff some entry >= c+1.  Kept additive:
    f += [f"cm_ge{k}" for k in range(1, n_rel + 1)]
    for br in ("3d", "2d"):
        f += [f"obj_n_{br}"] + [f"obj_hit@{k}_{br}" for k in _OBJ_K]
        f += [f"rel_n_{br}"] + [f"rel_hit@{k}_{br}" for k in _REL_K]
        f += [f"tri_n_{br}"] + [f"tri_hit@{k}_{br}" for k in _TRI_K]
        for c in range(n_rel):
            f += [f"cls{c}_n_{br}"] + [f"cls{c}_tri@{k}_{br}" for k in _TRI_K] + [f"cls{c}_rel@{k}_{br}" for k in _REL_K]
    return f


_IDX_CACHE: Dict[int, Dict[str, int]] = {}


def _index(n_rel: int) -> Dict[str, int]:
    if n_rel not in _IDX_CACHE:
        _IDX_CACHE[n_rel] = {k: i for i, k in enumerate(fields(n_rel))}
    return _IDX_CACHE[n_rel]


def accumulate(vec: np.ndarray, ranks: Dict[str, np.ndarray], cls_matrix: np.ndarray, n_scenes: int, n_rel: int = N_REL):
    """Add one batch's rank arrays (process_val outputs) into the counts vector (in place).  Histogram form
    (bincount per predicate class) of the per-class loops of get_mean_recall / compute_mean_predicate.  A branch whose
    ``top_k_obj*`` entry is missing or None (the 2D one of a 3D-only run) is skipped: its fields stay as they are."""
    idx = _index(n_rel)
    vec[idx["scenes"]] += n_scenes
    cm = np.asarray(cls_matrix, dtype=np.int64).reshape(-1, 5) if len(cls_matrix) else np.zeros((0, 5), np.int64)
    pred = cm[:, -1]
    if len(cm):                                      # #entries >= k for k = 1..n_rel, from one histogram of the matrix
        h = np.bincount(np.clip(cm.ravel(), 0, n_rel), minlength=n_rel + 1)
        ge = np.cumsum(h[::-1])[::-1]                # ge[k] = #entries >= k (entries above n_rel were clipped to n_rel)
        for k in range(1, n_rel + 1):
            vec[idx[f"cm_ge{k}"]] += int(ge[k])
    has = pred >= 0
    pc = pred[has]
    for br, sfx in (("3d", ""), ("2d", "_2d")):
        if ranks.get("top_k_obj" + sfx) is None:
            continue
        o, r, t = (np.asarray(ranks[name + sfx]) for name in ("top_k_obj", "top_k_rel", "top_k_triplet"))
        vec[idx[f"obj_n_{br}"]] += len(o)
        vec[idx[f"rel_n_{br}"]] += len(r)
        vec[idx[f"tri_n_{br}"]] += len(t)
        for k in _OBJ_K:
            vec[idx[f"obj_hit@{k}_{br}"]] += int((o <= k).sum())
        for k in _REL_K:
            vec[idx[f"rel_hit@{k}_{br}"]] += int((r <= k).sum())
        for k in _TRI_K:
            vec[idx[f"tri_hit@{k}_{br}"]] += int((t <= k).sum())
        # rows of cls_matrix align with the rank lists entry by entry; predicate -1 = "no relation" rows
        n_c = np.bincount(pc, minlength=n_rel)
        tri_c = {k: np.bincount(pc, weights=(t[has] <= k), minlength=n_rel) for k in _TRI_K}
        rel_c = {k: np.bincount(pc, weights=(r[has] <= k), minlength=n_rel) for k in _REL_K}
        for c in np.nonzero(n_c)[0]:
            if c >= n_rel:
                continue
            vec[idx[f"cls{c}_n_{br}"]] += int(n_c[c])
            for k in _TRI_K:
                vec[idx[f"cls{c}_tri@{k}_{br}"]] += int(tri_c[k][c])
            for k in _REL_K:
                vec[idx[f"cls{c}_rel@{k}_{br}"]] += int(rel_c[k][c])
    return vec


def _branches(use_2d: bool):
    return ("3d", "2d") if use_2d else ("3d",)


def summarize(vec: np.ndarray, n_rel: int = N_REL, use_2d: bool = True) -> Dict[str, float]:
    """Percentages validation() prints, from the (all-reduced) counts.  ``use_2d=False``: ``scenes`` and the 3D branch's keys only."""
    idx = _index(n_rel)
    out = {"scenes": float(vec[idx["scenes"]])}
    for br in _branches(use_2d):
        for name, ks in (("obj", _OBJ_K), ("rel", _REL_K), ("tri", _TRI_K)):
            n = max(vec[idx[f"{name}_n_{br}"]], 1)
            for k in ks:
                out[f"{name}_acc@{k}_{br}"] = float(vec[idx[f"{name}_hit@{k}_{br}"]] * 100 / n)
        present = [c for c in range(n_rel) if vec[idx[f"cls{c}_n_{br}"]] > 0]
        for k in _TRI_K:                             # classes c < cls_matrix.max() (reference quirk, kept)
            rec = [vec[idx[f"cls{c}_tri@{k}_{br}"]] * 100 / vec[idx[f"cls{c}_n_{br}"]] for c in present
                   if vec[idx[f"cm_ge{c + 1}"]] > 0]
            out[f"mean_recall@{k}_{br}"] = float(np.mean(np.array(rec, dtype=np.float32))) if rec else 0.0
        for k in _REL_K:                             # compute_mean_predicate: all 26 classes with samples
            acc = [vec[idx[f"cls{c}_rel@{k}_{br}"]] / vec[idx[f"cls{c}_n_{br}"]] for c in present]
            out[f"mean_rel_acc@{k}_{br}"] = float(np.mean(acc) * 100) if acc else 0.0
    return out


# ---- Recall@K / mR@K (validation(recall_k=True)): a second additive vector, concatenated onto fields() for the one all-reduce ----
def recall_fields(n_rel: int = N_REL):
    """Layout of the Recall@K vector (fp64, additive over scenes and ranks): rk_scenes (scenes with >= 1 gt edge), rk_gt_edges,
    rk_gt_cls{c}; then per branch, variant and K: the pooled hit count, the sum over scenes of the per-scene recall
    (rsum) and of the per-scene mean recall over the scene's predicate classes (mrsum), and the pooled per-class hits."""
    f = ["rk_scenes", "rk_gt_edges"] + [f"rk_gt_cls{c}" for c in range(n_rel)]
    for br in ("3d", "2d"):
        for v in _RK_VARIANTS:
            for k in _RK_K:
                f += [f"{v}_hit@{k}_{br}", f"{v}_rsum@{k}_{br}", f"{v}_mrsum@{k}_{br}"]
                f += [f"{v}_cls{c}_hit@{k}_{br}" for c in range(n_rel)]
    return f


def recall_vector(c3: torch.Tensor, c2: torch.Tensor | None, n_rel: int = N_REL) -> torch.Tensor:
    """The recall_fields() vector (fp64, on the counts' device, no synchronisation) of one batch from the per-scene counts
    ``metrics.recallk_counts`` returned for its 3D (``c3``) and 2D (``c2``) outputs.  ``c2=None``: the 2D entries are zero."""
    r = n_rel
    gt = c3[:, 0].double()
    gtc = c3[:, 1:1 + r].double()
    valid = gt > 0
    cls_on = gtc > 0
    n_cls = cls_on.sum(1).clamp(min=1).double()
    parts = [valid.sum().double().view(1), gt.sum().view(1), gtc.sum(0)]
    for c in (c3, c2):
        if c is None:                                   # (same layout and length: the branch's block adds nothing)
            parts.append(torch.zeros(len(_RK_VARIANTS) * 3 * (3 + r), dtype=torch.float64, device=c3.device))
            continue
        for v in _RK_VARIANTS:
            base = recallk_offset(v, r)
            hits = c[:, base:base + 3].double()                                        # [S, 3]
            ch = c[:, base + 3:base + 3 + 3 * r].double().view(-1, 3, r)              # [S, 3, R]
            rsum = (hits / gt.clamp(min=1)[:, None] * valid[:, None]).sum(0)
            mr = (ch / gtc.clamp(min=1)[:, None, :] * cls_on[:, None, :]).sum(2) / n_cls[:, None]
            mrsum = (mr * valid[:, None]).sum(0)
            parts.append(torch.cat([hits.sum(0)[:, None], rsum[:, None], mrsum[:, None], ch.sum(0)], 1).reshape(-1))
    return torch.cat(parts)


def recall_summarize(vec: np.ndarray, n_rel: int = N_REL, use_2d: bool = True) -> Dict[str, float]:
    """Percentages from the (all-reduced) recall_fields() vector.  ``{v}_R@{K}_{br}`` / ``{v}_mR@{K}_{br}``: the per-scene
    Recall@K / mR@K (what evaluate_triplet_recallk / _mrecallk return for one scene; mR = mean over the scene's predicate
    classes) averaged over the scenes with at least one gt edge.  ``..._pooled``: hits over gt edges of all scenes, and the
    mean over predicate classes of the pooled per-class recall.  The reference never aggregates across scenes; both are given.
    ``use_2d=False``: the 3D branch's keys only."""
    idx = {k: i for i, k in enumerate(recall_fields(n_rel))}
    n_sc, n_gt = vec[idx["rk_scenes"]], vec[idx["rk_gt_edges"]]
    gtc = np.array([vec[idx[f"rk_gt_cls{c}"]] for c in range(n_rel)])
    out = {}
    for br in _branches(use_2d):
        for v in _RK_VARIANTS:
            for k in _RK_K:
                ch = np.array([vec[idx[f"{v}_cls{c}_hit@{k}_{br}"]] for c in range(n_rel)])
                out[f"{v}_R@{k}_{br}"] = float(vec[idx[f"{v}_rsum@{k}_{br}"]] * 100 / n_sc) if n_sc else float("nan")
                out[f"{v}_mR@{k}_{br}"] = float(vec[idx[f"{v}_mrsum@{k}_{br}"]] * 100 / n_sc) if n_sc else float("nan")
                out[f"{v}_R@{k}_{br}_pooled"] = float(vec[idx[f"{v}_hit@{k}_{br}"]] * 100 / n_gt) if n_gt else float("nan")
                on = gtc > 0
                out[f"{v}_mR@{k}_{br}_pooled"] = float(np.mean(ch[on] / gtc[on]) * 100) if on.any() else float("nan")
    return out


# ---- zero-shot split of the triplet recall (validation(zero_shot=table)): a third additive vector, concatenated like the others ----
def split_fields():
    """Layout of the zero-shot split vector (additive over scenes and ranks; vlsat_eval_triplet_split's counts): per branch
    (3D, 2D) the triplet rows with a predicate (zs_all_n), their hits at 50 / 100, then the same over the zero-shot rows.
    Non-zero-shot = all - zero-shot."""
    f = []
    for br in ("3d", "2d"):
        f += [f"zs_all_n_{br}", f"zs_all_hit@50_{br}", f"zs_all_hit@100_{br}", f"zs_n_{br}", f"zs_hit@50_{br}", f"zs_hit@100_{br}"]
    return f


def accumulate_split(vec: np.ndarray, top_k_triplet, top_k_triplet_2d, cls_matrix, table, n_rel: int = N_REL):
    """Add one batch's zero-shot split counts (the split_fields() vector) from process_val's triplet ranks of both branches
    (``out[4]``, ``out[5]``) and its ``cls_matrix`` (``out[6]``), in place; ``table`` from zeroshot.zero_shot_table.
    ``top_k_triplet_2d=None``: the 2D half stays as it is."""
    from .zeroshot import split_counts_host
    vec[0:6] += split_counts_host(top_k_triplet, cls_matrix, table, n_rel)
    if top_k_triplet_2d is not None:
        vec[6:12] += split_counts_host(top_k_triplet_2d, cls_matrix, table, n_rel)
    return vec


def split_summarize(vec: np.ndarray, use_2d: bool = True) -> Dict[str, float]:
    """``zero_shot_recall@K_{br}``, ``non_zero_shot_recall@K_{br}`` and ``all_zero_shot_recall@K_{br}`` (K = 50, 100) from the
    (all-reduced) split_fields() vector: what get_zero_shot_recall returns (reference eva_utils_acc.py:267-333; NaN for an empty
    group).  The reference reports the 3D branch; the 2D values, the same definition on the 2D triplet ranks, are an extension
    (``use_2d=False``: left out)."""
    from .zeroshot import recall_from_counts
    out = {}
    for b, br in enumerate(_branches(use_2d)):
        an, a50, a100, zn, z50, z100 = (int(x) for x in vec[6 * b:6 * b + 6])
        for k, ah, zh in ((50, a50, z50), (100, a100, z100)):
            out[f"zero_shot_recall@{k}_{br}"] = recall_from_counts(zn, zh)
            out[f"non_zero_shot_recall@{k}_{br}"] = recall_from_counts(an - zn, ah - zh)
            out[f"all_zero_shot_recall@{k}_{br}"] = recall_from_counts(an, ah)
    return out


_warned_sync = False


def _n_scenes(b) -> int:
    """Scenes in a batch.  ``n_scenes`` / ``fc_sizes`` are what the pipelined loop (validation(workers >= 1)) needs to stay free
    of host round trips: without either the count is read back from ``batch_ids`` on the device -- a blocking copy per batch on
    the worker's stream (and the forward then also reads the edge list back to key its plan).  Correct, but the loop runs at the
    latency of every scene; said once."""
    if "n_scenes" in b:
        return int(b["n_scenes"])
    if "fc_sizes" in b:
        return len(b["fc_sizes"])
    if not b["batch_ids"].numel():
        return 0
    if b["batch_ids"].is_cuda:
        global _warned_sync
        if not _warned_sync:
            _warned_sync = True
            import warnings
            warnings.warn("evaluate: batch without 'n_scenes' / 'fc_sizes' -- the scene count (and the plan key) are read back from "
                          "the device for every batch, which serialises the loop; add one of the hints to the loader's items",
                          RuntimeWarning, stacklevel=3)
    return int(b["batch_ids"].max().item()) + 1


def merge_batches(bs, use_2d: bool = True) -> dict:
    """Consecutive batches (the reference loader's item names) collated into ONE on the device: node offsets applied to
    ``edge_indices``, scene offsets to ``batch_ids``, ``fc_sizes`` hints concatenated when every batch carries one (what
    collate_fn_mmg does for a bigger batch_size, reference DataLoader.py:160-172).  Counts are additive over scenes, so a loop
    may hand the library several of its one-scene batches at a time.  ``use_2d=False``: ``obj_2d_feats`` is neither read nor
    part of the result."""
    if len(bs) == 1:
        return bs[0]
    ei, bid, n_off, s_off = [], [], 0, 0
    for b in bs:
        n = b["obj_points"].shape[0]
        ids = b.get("batch_ids")
        ids = torch.zeros(n, 1, dtype=torch.int64, device=b["obj_points"].device) if ids is None else ids.view(-1, 1)
        ei.append(b["edge_indices"] + n_off)
        bid.append(ids + s_off)
        n_off += n
        s_off += _n_scenes(b)
    keys = ("obj_points", "obj_2d_feats", "descriptor", "gt_class", "gt_rel_cls") if use_2d else ("obj_points", "descriptor", "gt_class", "gt_rel_cls")
    out = {k: torch.cat([b[k] for b in bs]) for k in keys}
    out["edge_indices"], out["batch_ids"], out["n_scenes"] = torch.cat(ei), torch.cat(bid), s_off
    if all("fc_sizes" in b for b in bs):
        out["fc_sizes"] = [int(x) for b in bs for x in b["fc_sizes"]]
    return out


@contextlib.contextmanager
def _worker_stream(dev, own: bool):
    """What a worker of ``_run_pool`` runs its items in: the device set for its thread and a stream -- a new one (``own``) or the
    thread's current one -- synchronised after the last item.  An exception leaves without the synchronise."""
    torch.cuda.set_device(dev)
    stream = torch.cuda.Stream(device=dev) if own else torch.cuda.current_stream(dev)
    with torch.cuda.stream(stream):
        yield
    stream.synchronize()


def _run_pool(model, items, dev, workers: int, job, context=None):
    """``job(k, model_k, item)`` for every item of the iterator ``items``, ``workers`` of them in flight: worker k owns a replica of
    the model (its own library handle: a handle is driven by one host thread and one stream at a time; kept by the model:
    building one uploads and prepares every weight) and a stream, and takes the next item under a lock until the iterator ends or
    any worker has failed.  One worker runs in the caller's thread on its current stream; more run on daemon threads with a stream
    each, after ONE synchronise of the caller's stream: what it produced -- inputs, zeroed tables -- is complete before they read
    it.  The first exception of a job is re-raised here after every thread has joined.  ``context``: the ``_worker_stream`` of
    a run without a GPU (the tests pass ``contextlib.nullcontext``)."""
    import threading
    models = [model] + model.replicas(workers - 1)
    items, lock, errors, end = iter(items), threading.Lock(), [], object()

    def work(k):
        try:
            with (context or _worker_stream)(dev, workers > 1):
                while not errors:
                    with lock:
                        item = next(items, end)
                    if item is end:
                        break
                    job(k, models[k], item)
        except BaseException as ex:             # (re-raised in the caller's thread)
            errors.append(ex)

    if workers == 1:
        work(0)
    else:
        if context is None:
            torch.cuda.current_stream(dev).synchronize()
        ts = [threading.Thread(target=work, args=(k,), daemon=True) for k in range(workers)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
    if errors:
        raise errors[0]


def _in_order(model, batches, dev, workers: int, one, split):
    """``split(one(model, b), b)`` of every batch, in input order.  workers <= 0: one batch after the other on the current stream,
    batch i + 1 untouched before the scenes of batch i are out.  workers >= 1: every batch through ``_run_pool`` first."""
    if workers <= 0:
        for b in batches:
            yield from split(one(model, b), b)
        return
    results = {}

    def job(k, m, item):
        results[item[0]] = one(m, item[1]), item[1]

    _run_pool(model, enumerate(batches), torch.device(dev), workers, job)
    for i in sorted(results):
        yield from split(*results[i])


def _scene_starts(b: dict, n_sc: int, nodes: bool = True):
    """Where every scene of a batch starts: (first node row, first edge row), two lists of ``n_sc`` + 1 entries, the last the
    end.  ``batch_ids`` ascend and the edges are grouped by scene, so both are a ``searchsorted`` -- a scene without edges gets an
    empty range.  One read-back per list; ``nodes=False`` spares the first (None)."""
    ids = b["batch_ids"].view(-1).contiguous()
    arange = torch.arange(n_sc + 1, device=ids.device)
    node = torch.searchsorted(ids, arange).tolist() if nodes else None
    return node, torch.searchsorted(ids[b["edge_indices"][:, 0]].contiguous(), arange).tolist()


def _split_scene_graphs(pair, b):
    g3, g2 = pair
    n_sc = g3.n_valid.numel()
    if n_sc == 1:
        yield g3, g2
        return
    _, start = _scene_starts(b, n_sc, nodes=False)
    for s in range(n_sc):
        yield g3.scene(s, start[s]), (None if g2 is None else g2.scene(s, start[s]))


def _split_decoded(pair, b):
    g3, g2 = pair
    n_sc = g3.n_valid.numel()
    if n_sc == 1:
        yield g3, g2
        return
    node, start = _scene_starts(b, n_sc)
    for s in range(n_sc):
        nodes = (node[s], node[s + 1])
        yield g3.scene(s, start[s], nodes), (None if g2 is None else g2.scene(s, start[s], nodes))


def _split_merged(pairs, b):
    n_sc = pairs[0][0].n_objects.numel()
    if n_sc == 1:
        yield pairs
        return
    _, start = _scene_starts(b, n_sc, nodes=False)
    first = [None if pair is None else [0] + list(itertools.accumulate(pair[0].n_objects.tolist())) for pair in pairs]
    for s in range(n_sc):
        out = []
        for pair, o in zip(pairs, first):                 # o: first object row of every scene of this branch
            if pair is None:
                out.append(None)
                continue
            g, d = pair
            src = g.pair_edges[:, 0]
            rows = ((src >= o[s]) & (src < o[s + 1])).nonzero().view(-1)
            out.append((g.scene(s, (start[s], start[s + 1])), d.scene(s, int(rows[0]) if rows.numel() else 0, (o[s], o[s + 1]))))
        yield tuple(out)


def _model_n_rel(model) -> int:
    """relation classes of the model's heads (the layout of the additive vectors); a model without a config: the reference's 26"""
    return int(getattr(getattr(model, "config", None), "num_rel_class", N_REL))


@torch.no_grad()
def _validation_pipelined(model, batches: Iterable[dict], device, workers: int, merge: int = 1, recall_k: bool = False,
                          zero_shot=None, use_2d: bool = True):
    """The counts vector of this rank's batches with NO host round trip per batch and ``workers`` batches in flight
    (``_run_pool``); forward, ranking and counting of a batch are enqueued back to back
    (``metrics.process_val_counts``) and the counts accumulate on the device with integer atomics.  One scene per batch --
    validation()'s own pattern (batch_size = 1, reference src/model/model.py:185,201-211) -- leaves most of the 256 CUs idle
    when scenes run one after the other (a 40-object forward is ~115 dependent kernels of 5-20 us); several in flight fill
    them.  The host side scales too: the library call that enqueues a forward releases the GIL (ctypes).
    ``merge`` > 1: every worker takes that many consecutive batches at a time and collates them on the device into one call
    (``merge_batches``): the forward then runs at its batched rate.  Counts are additive, so the summary is the same up to
    near-ties (a batched forward differs from a one-scene forward in the last bits: a rank may move by one).
    Single-label models (``multi_rel_outputs=False``) ride the same path: one library call per batch, the vectors laid out for the
    model's own ``num_rel_class``.
    ``use_2d=False``: every batch takes the 3D-only step (``obj_2d_feats`` is not read); the 2D entries of the vectors stay zero.
    Returns the counts vector; with ``recall_k`` or ``zero_shot`` (the device uint8 table) the tuple (counts, recall vector or
    None, split vector or None)."""
    from . import metrics as M
    dev = torch.device(device)
    n_rel = _model_n_rel(model)
    counts = [torch.zeros(len(fields(n_rel)), dtype=torch.int64, device=dev) for _ in range(workers)]
    recall = [torch.zeros(len(recall_fields(n_rel)), dtype=torch.float64, device=dev) if recall_k else None for _ in range(workers)]
    split = [torch.zeros(len(split_fields()), dtype=torch.int64, device=dev) if zero_shot is not None else None for _ in range(workers)]

    def groups(it, n):                          # (the pool takes an item under its lock: a whole group is read there)
        while group := list(itertools.islice(it, n)):
            yield group

    def one(k, m, group):
        b = merge_batches(group, use_2d)
        M.process_val_counts(m, counts[k], b["obj_points"], b["obj_2d_feats"] if use_2d else None, b["gt_class"], b["descriptor"],
                             b["gt_rel_cls"], b["edge_indices"], b.get("batch_ids"), _n_scenes(b), b.get("fc_sizes"),
                             recall=recall[k], split_table=zero_shot, split_counts=split[k])

    _run_pool(model, groups(iter(batches), max(1, merge)), dev, workers, one)
    vec = torch.stack(counts).sum(0).cpu().numpy().astype(np.float64)
    if recall_k or zero_shot is not None:
        return (vec, torch.stack(recall).sum(0).cpu().numpy() if recall_k else None,
                torch.stack(split).sum(0).cpu().numpy().astype(np.float64) if zero_shot is not None else None)
    return vec


@torch.no_grad()
def predict(model, batches: Iterable[dict], device=None, workers: int = 0, use_2d: bool = True, **graph_args):
    """The predicted scene graph of every scene of ``batches`` (the loader's dicts; no labels are read), in input order: yields
    one ``(graph_3d, graph_2d)`` pair of one-scene ``metrics.SceneGraph`` per scene, edge rows counted within the scene's own
    edge list.  ``use_2d=False`` takes the 3D-only forward (``obj_2d_feats`` is not read; ``graph_2d`` is None).
    ``graph_args``: ``top_k``, ``topk_each``, ``evaluate`` of ``VLSATModel.predict_graph``.  workers = 0: one batch
    after the other on the current stream.  workers >= 1: as the pipelined validation loop -- every worker thread owns a replica
    of the model and a stream and takes the next batch; nothing is read back per batch."""
    workers = int(workers)
    if workers > 0 and device is None:
        raise ValueError("predict(workers > 0) needs the device")

    def one(m, b):
        return m.predict_graph(b["obj_points"], b["obj_2d_feats"] if use_2d else None, b["edge_indices"].t(), b["descriptor"], b.get("batch_ids"),
                               fc_sizes=b.get("fc_sizes"), **graph_args)

    yield from _in_order(model, batches, device, workers, one, _split_scene_graphs)


@torch.no_grad()
def decode(model, batches: Iterable[dict], device=None, workers: int = 0, use_2d: bool = True, **decode_args):
    """The decoded scene graph of every scene of ``batches`` (the loader's dicts; no labels are read), in input order: yields one
    ``(graph_3d, graph_2d)`` pair of one-scene ``metrics.DecodedGraph`` per scene -- its own node rows, edge rows counted within
    the scene's own edge list.  ``use_2d=False`` takes the 3D-only forward (``obj_2d_feats`` is not read; ``graph_2d`` is None):
    the route of unlabelled scans.  ``decode_args``: ``threshold``, ``score``, ``n_labels``, ``max_rel``, ``multi_rel_outputs`` of
    ``VLSATModel.decode_graph``.  workers = 0: one batch after the other on the current stream.  workers >= 1: as ``predict`` --
    every worker thread owns a replica of the model and a stream and takes the next batch; nothing is read back per batch."""
    workers = int(workers)
    if workers > 0 and device is None:
        raise ValueError("decode(workers > 0) needs the device")

    def one(m, b):
        return m.decode_graph(b["obj_points"], b["obj_2d_feats"] if use_2d else None, b["edge_indices"].t(), b["descriptor"],
                              b.get("batch_ids"), fc_sizes=b.get("fc_sizes"), **decode_args)

    yield from _in_order(model, batches, device, workers, one, _split_decoded)


@torch.no_grad()
def merged(model, batches: Iterable[dict], device=None, workers: int = 0, use_2d: bool = True, same_part: Optional[int] = None,
           threshold: float = 0.5, mutual: bool = False, **decode_args):
    """Over-segmented scans as graphs of objects, in input order: yields per scene ``((merged_3d, decoded_3d), (merged_2d,
    decoded_2d))`` -- one-scene ``metrics.MergedGraph`` / ``metrics.DecodedGraph``, rows counted within the scene (segments,
    objects, merged edges) -- from ``VLSATModel.merge_graph``; the second pair is None with ``use_2d=False``.  ``same_part``: the
    index of the "same part" predicate among the model's classes.  The weights of the pooled class probabilities are the batch's
    ``weights`` or, without, its ``points_per_instance`` (None: all 1).  workers as for ``decode``; the merge reads two totals back
    per batch and branch."""
    workers = int(workers)
    if workers > 0 and device is None:
        raise ValueError("merged(workers > 0) needs the device")

    def one(m, b):
        w = b.get("weights", b.get("points_per_instance"))
        return m.merge_graph(b["obj_points"], b["obj_2d_feats"] if use_2d else None, b["edge_indices"].t(), b["descriptor"],
                             b.get("batch_ids"), same_part=same_part, weights=w, threshold=threshold, mutual=mutual,
                             fc_sizes=b.get("fc_sizes"), **decode_args)

    yield from _in_order(model, batches, device, workers, one, _split_merged)


def merge_quality(root, gt_of_segment) -> Dict[str, float]:
    """How well merged objects agree with the annotation, on the host.  ``root[i]``: any id of the merged object of segment i
    (``MergedGraph.root`` or ``.object``); ``gt_of_segment[i]``: the annotated instance of segment i, negative or None for a
    segment without one (from ``LabelTransfer.segment_to_gt``).  Over the pairs of matched segments: ``pairs_same_pred`` /
    ``pairs_same_gt`` / ``pairs_both`` and the pairwise ``precision`` = both / pred, ``recall`` = both / gt and ``f1`` of "same
    object" (NaN where the denominator is 0; all 1 when neither side joins any pair).  ``over_merged`` = merged objects whose
    matched segments belong to more than one instance; ``split`` = instances whose segments ended in more than one object."""
    root = np.asarray(root.cpu() if torch.is_tensor(root) else root).astype(np.int64).reshape(-1)
    gt = np.asarray([-1 if g is None else int(g) for g in (gt_of_segment.tolist() if hasattr(gt_of_segment, "tolist") else gt_of_segment)],
                    dtype=np.int64)
    if root.shape != gt.shape:
        raise ValueError("merge_quality: one object and one instance per segment")
    keep = gt >= 0
    r, g = root[keep], gt[keep]

    def pairs(*keys):
        if not r.size:
            return 0
        _, cnt = np.unique(np.stack(keys, 1), axis=0, return_counts=True)
        return int((cnt * (cnt - 1) // 2).sum())

    pred, true, both = pairs(r), pairs(g), pairs(r, g)
    nan = float("nan")
    if pred == 0 and true == 0:
        prec = rec = f1 = 1.0
    else:
        prec, rec = (both / pred if pred else nan), (both / true if true else nan)
        f1 = 2 * both / (pred + true)
    cells = np.unique(np.stack([r, g], 1), axis=0) if r.size else np.zeros((0, 2), np.int64)
    over = int((np.unique(cells[:, 0], return_counts=True)[1] > 1).sum()) if cells.size else 0
    split = int((np.unique(cells[:, 1], return_counts=True)[1] > 1).sum()) if cells.size else 0
    return {"segments": int(keep.sum()), "pairs_same_pred": pred, "pairs_same_gt": true, "pairs_both": both, "precision": prec,
            "recall": rec, "f1": f1, "over_merged": over, "split": split}


def graph_quality(counts, n_rel: int = N_REL) -> Dict[str, float]:
    """Precision, recall and F1 of the decoded relations and the accuracy of the decoded labels, from the (all-reduced) counts of
    ``metrics.decode_counts``: one vector [3 R + 2], or the vectors of several branches stacked ([B, 3 R + 2] -> keys suffixed
    ``_0``, ``_1``, ...; a dict maps branch names to vectors).  micro: over the summed tp / fp / fn.  macro: the mean over the
    predicates that occur (tp + fp + fn > 0) of the per-predicate value, a value whose denominator is 0 counting as 0.  An empty
    group is NaN.  ``per_class_{precision,recall,f1}`` hold the per-predicate values (NaN where the denominator is 0)."""
    if isinstance(counts, dict):
        out = {}
        for name, v in counts.items():
            out.update({f"{k}_{name}": x for k, x in graph_quality(v, n_rel).items()})
        return out
    v = np.asarray(counts.cpu() if torch.is_tensor(counts) else counts, dtype=np.float64)
    if v.ndim == 2:
        return graph_quality({str(i): row for i, row in enumerate(v)}, n_rel)
    if v.shape != (3 * n_rel + 2,):
        raise ValueError(f"graph_quality: expected {3 * n_rel + 2} counts")
    tp, fp, fn = v[0:3 * n_rel:3], v[1:3 * n_rel:3], v[2:3 * n_rel:3]
    with np.errstate(invalid="ignore", divide="ignore"):
        def prf(t, p, n):
            pr, rc, f1 = t / (t + p), t / (t + n), 2 * t / (2 * t + p + n)
            return pr, rc, f1
        micro = prf(tp.sum(), fp.sum(), fn.sum())
        per = prf(tp, fp, fn)
        seen = (tp + fp + fn) > 0
        macro = [float(np.nan_to_num(x[seen]).mean()) if seen.any() else float("nan") for x in per]
        acc = v[3 * n_rel + 1] / v[3 * n_rel]
    out = {"rel_asserted": float(tp.sum() + fp.sum()), "rel_gt": float(tp.sum() + fn.sum()), "nodes": float(v[3 * n_rel]),
           "node_acc": float(acc)}
    for name, m, M_, p in zip(("precision", "recall", "f1"), micro, macro, per):
        out[f"micro_{name}"], out[f"macro_{name}"], out[f"per_class_{name}"] = float(m), M_, p
    return out


def operating_points(tables, default: float = 0.5) -> Dict[str, object]:
    """PR curves, average precision, per-predicate thresholds and the calibration of the object head, on the host, from the
    (all-reduced) ``metrics.ScoreTables`` of ``metrics.score_histograms`` / ``calibrate``.  B = ``tables.bins``; threshold k / B.
    Predicate head -- ``precision`` / ``recall`` / ``f1`` float64 [R, B] at every k (NaN where the denominator is 0);
    ``k`` int64 [R] and ``threshold`` float32 [R] (a tensor ready for ``decode_graph(threshold=...)``): the k of the best F1, the
    lowest k among equals; a predicate without ground truth keeps ``default`` (which must be a multiple of 1 / B in [0, 1): nothing
    else can be read off the table); ``tp`` / ``fp`` / ``fn`` int64 [R] at that choice (``counts`` [3 R]: the same in
    ``decode_counts`` order) -- ``decode_counts(threshold=threshold)`` over the same data reproduces them exactly;
    ``ap`` float64 [R]: non-interpolated average precision at bin resolution, sum over k of (recall_k - recall_{k+1}) precision_k
    with recall_B = 0 (NaN without ground truth), ``mean_ap`` over the predicates that occur; ``micro_f1`` / ``macro_f1`` at the
    chosen vector beside ``micro_f1_default`` / ``macro_f1_default`` at ``default``, as ``graph_quality`` defines them (macro:
    over the predicates with tp + fp + fn > 0, a value whose denominator is 0 counting as 0).
    Object head -- ``obj_bin_count`` int64 [B] and ``obj_bin_acc`` float64 [B] (NaN for an empty bin): the reliability diagram of the
    top-1 probability; ``ece`` = sum over the bins of count / total * |accuracy - (b + 0.5) / B|: the table holds counts and no sums of
    confidences, so a bin's confidence is its MIDPOINT (off by at most 1 / (2 B) per bin; nodes whose top-1 probability is NaN
    are left out); ``obj_acc``; ``per_class_acc`` float64 [C] (NaN for a class without nodes) and ``mean_class_acc`` over the classes
    that occur; ``confusion`` int64 [C, C]."""
    t = tables.cpu()
    b, rel = t.bins, t.rel.numpy()
    r = rel.shape[0]
    kd = t.k_vector(float(default))[:1].item()
    suf = t.suffix_sums().numpy().astype(np.float64)                                   # [R, 2, B]
    tp, fp = suf[:, 1], suf[:, 0]
    n_gt = rel[:, 1].sum(-1).astype(np.float64)
    fn = n_gt[:, None] - tp
    with np.errstate(invalid="ignore", divide="ignore"):
        prec, rec, f1 = tp / (tp + fp), tp / (tp + fn), 2 * tp / (2 * tp + fp + fn)
        occurs = n_gt > 0
        k = np.where(occurs, np.argmax(np.nan_to_num(f1, nan=-1.0), axis=1), kd).astype(np.int64)       # (argmax: the first maximum)
        rec_next = np.concatenate([rec[:, 1:], np.zeros((r, 1))], 1)
        ap = np.where(occurs, np.nan_to_num((rec - rec_next) * np.nan_to_num(prec)).sum(1), np.nan)
        counts = t.counts_at(torch.from_numpy(k))
        both = {"": counts, "_default": t.counts_at(kd)}
        out = {"bins": b, "precision": prec, "recall": rec, "f1": f1, "k": k,
               "threshold": torch.from_numpy(k.astype(np.float32) / np.float32(b)), "counts": counts,
               "tp": counts[0::3].clone(), "fp": counts[1::3].clone(), "fn": counts[2::3].clone(), "ap": ap,
               "mean_ap": float(ap[occurs].mean()) if occurs.any() else float("nan")}
        for name, c in both.items():
            q = graph_quality(torch.cat([c, torch.zeros(2, dtype=torch.int64)]), r)
            out["micro_f1" + name], out["macro_f1" + name] = q["micro_f1"], q["macro_f1"]
        obj = t.obj.numpy()[:, :b].astype(np.float64)
        cnt = obj.sum(0)
        acc = obj[1] / cnt
        total = cnt.sum()
        mid = (np.arange(b) + 0.5) / b
        out["obj_bin_count"], out["obj_bin_acc"] = cnt.astype(np.int64), acc
        out["ece"] = float((cnt[cnt > 0] / total * np.abs(acc - mid)[cnt > 0]).sum()) if total else float("nan")
        cm = t.confusion.numpy()
        per = cm.sum(1).astype(np.float64)
        out["obj_acc"] = float(np.trace(cm) / per.sum()) if per.sum() else float("nan")
        out["per_class_acc"] = np.diag(cm) / per
        out["mean_class_acc"] = float(out["per_class_acc"][per > 0].mean()) if (per > 0).any() else float("nan")
        out["confusion"] = cm
    return out


@torch.no_grad()
def calibrate(model, batches: Iterable[dict], device=None, workers: int = 0, use_2d: bool = True, bins: int = 1024,
              multi_rel_outputs: Optional[bool] = None) -> Dict[str, object]:
    """The score histograms of this rank's ``batches`` (the loader's dicts, with ``gt_class`` and ``gt_rel_cls``), all-reduced:
    ``{"3d": metrics.ScoreTables, "2d": metrics.ScoreTables | None}`` -- what ``operating_points`` reads.  Per batch the forward
    (``forward_3d`` with ``use_2d=False``: ``obj_2d_feats`` is not read and "2d" is None) and ``metrics.score_histograms`` per
    branch are enqueued back to back; nothing is read back per batch.  workers = 0: one batch after the other on the current
    stream.  workers >= 1: as ``decode`` -- every worker thread owns a replica of the model and a stream and takes the next batch;
    all of them add into the same table per branch (integer atomics: the sums do not depend on the order).  ONE collective at the
    end (``dist.allreduce_metrics`` over both branches' buffers); it sums in fp64, so the counts are exact as long as every entry of
    the summed tables stays below 2^53.  ``multi_rel_outputs`` (default: the model's) selects the rule."""
    from . import metrics as M
    workers = int(workers)
    if workers > 0 and device is None:
        raise ValueError("calibrate(workers > 0) needs the device")
    cfg = model.config
    multi = bool(cfg.multi_rel_outputs if multi_rel_outputs is None else multi_rel_outputs)
    dev = torch.device(model.device if device is None else device)
    tabs = [M.ScoreTables(cfg.num_rel_class, cfg.num_obj_class, bins, dev) for _ in range(2 if use_2d else 1)]

    def one(k, m, b):
        edges = b["edge_indices"]
        ei_t = edges.t() if b.get("fc_sizes") is not None else edges.t().contiguous()
        if use_2d:
            obj3, obj2, rel3, rel2 = m(b["obj_points"], b["obj_2d_feats"], ei_t, b["descriptor"], b.get("batch_ids"), istrain=False,
                                       fc_sizes=b.get("fc_sizes"))
            outs = ((obj3, rel3), (obj2, rel2))
        else:
            outs = (m.forward_3d(b["obj_points"], ei_t, b["descriptor"], b.get("batch_ids"), fc_sizes=b.get("fc_sizes")),)
        for (obj, rel), t in zip(outs, tabs):
            M.score_histograms(obj, rel, b["gt_class"], b["gt_rel_cls"], multi, bins, tables=t)

    _run_pool(model, batches, dev, max(workers, 1), one)
    vec = vdist.allreduce_metrics(torch.cat([t.buffer for t in tabs]).double())
    parts = vec.to(torch.int64).split([t.buffer.numel() for t in tabs])
    out = [M.ScoreTables(cfg.num_rel_class, cfg.num_obj_class, bins, buffer=p.contiguous()) for p in parts]
    return {"3d": out[0], "2d": out[1] if use_2d else None}


@torch.no_grad()
def validation(model, batches: Iterable[dict], device=None, workers: int = 0, merge: int = 1,
               recall_k: bool = False, zero_shot=None, use_2d: bool = True) -> Dict[str, float]:
    """``batches`` yields this rank's dicts with the reference loader's item names
    (obj_points [N,3,P], obj_2d_feats, gt_class, gt_rel_cls, edge_indices [E,2], descriptor, batch_ids; optionally
    ``fc_sizes``: objects per scene when edge_indices is the canonical fully-connected list, which spares the graph plan a
    read-back of the edge list).  One collective at the very end.
    workers = 0: the reference-compatible path -- ``process_val`` per batch (numpy rank lists on the host, like
    ``Mmgnet.process_val``) and host-side accumulation.  workers >= 1: counts accumulated on the device, no host round trip
    per batch, ``workers`` batches in flight on as many streams and model replicas (for one-scene-per-call loops);
    ``merge`` = B > 1 additionally collates B consecutive batches into one call (``merge_batches``).
    recall_k = True: the result also holds the scene-graph Recall@K / mR@K of both branches (recall_summarize: PredCls /
    SGCls, with and without graph constraint, K = 20, 50, 100), from a recall_fields() vector concatenated onto the counts
    so that the run still does one all-reduce.
    zero_shot = the uint8 [C*C*R] table of zeroshot.zero_shot_table (built once per run from the training and validation
    annotations): the result also holds the zero-shot split of the triplet recall (split_summarize: zero_shot_recall@K,
    non_zero_shot_recall@K, all_zero_shot_recall@K, K = 50, 100) of both branches -- get_zero_shot_recall, reference
    src/model/model.py:253; the reference reports the 3D branch, the ``_2d`` values are an extension -- from a split_fields()
    vector concatenated onto the others, still one all-reduce.  None: the result and the work are unchanged.
    use_2d = False: the model as deployed -- every batch takes the 3D-only forward and one ranking pass, ``obj_2d_feats`` is not
    read (a batch may lack the key).  The vectors keep their layout and length (the 2D entries stay zero: the same one all-reduce)
    and the result holds ``scenes`` and the 3D branch's keys only, with the values of the two-branch run.
    Single-label models (``multi_rel_outputs=False``, ``gt_rel_cls`` the [E] label vector) take every path above, the pipelined one
    included: one library call per batch, like multi-label models.  The vectors are laid out for the model's ``num_rel_class``."""
    from . import metrics as M
    n_rel = _model_n_rel(model)
    if zero_shot is not None:
        if workers > 0:
            zero_shot = torch.as_tensor(zero_shot, dtype=torch.uint8).to(device).contiguous()
        else:                                   # (host accumulation: read the table once, not per batch)
            zero_shot = zero_shot.cpu().numpy() if isinstance(zero_shot, torch.Tensor) else np.asarray(zero_shot)
    if workers > 0:
        if device is None:
            raise ValueError("validation(workers > 0) needs the device")
        vec = _validation_pipelined(model, batches, device, int(workers), int(merge), bool(recall_k), zero_shot, bool(use_2d))
        if recall_k or zero_shot is not None:
            vec = np.concatenate([v for v in vec if v is not None])
            return _summaries(vdist.allreduce_metrics(torch.from_numpy(vec).to(device)).cpu().numpy(), recall_k, zero_shot is not None,
                              use_2d, n_rel)
        t = vdist.allreduce_metrics(torch.from_numpy(vec).to(device))
        return summarize(t.cpu().numpy(), n_rel, use_2d=use_2d)
    vec = np.zeros(len(fields(n_rel)), dtype=np.float64)
    rvec = np.zeros(len(recall_fields(n_rel)), dtype=np.float64) if recall_k else None
    svec = np.zeros(len(split_fields()), dtype=np.float64) if zero_shot is not None else None
    for b in batches:
        # process_val, with the forward's outputs kept for the recall counts
        outs = M._forward_eval(model, b["obj_points"], b["obj_2d_feats"] if use_2d else None, b["descriptor"], b["edge_indices"],
                               b["batch_ids"], use_2d=use_2d)
        out = M._process_val_from(model, outs, b["gt_class"], b["gt_rel_cls"], b["edge_indices"], True)
        ranks = dict(top_k_obj=out[0], top_k_obj_2d=out[1], top_k_rel=out[2], top_k_rel_2d=out[3],
                     top_k_triplet=out[4], top_k_triplet_2d=out[5])
        n_scenes = int(b["batch_ids"].max().item()) + 1 if b["batch_ids"].numel() else 0
        accumulate(vec, ranks, out[6], n_scenes, n_rel)
        if recall_k:
            multi = bool(getattr(getattr(model, "config", None), "multi_rel_outputs", True))
            bid = b["batch_ids"].view(-1)
            c3, c2 = (None if o is None else M.recallk_counts(o, rl, b["gt_class"], b["gt_rel_cls"], b["edge_indices"], bid, n_scenes, multi)
                      for o, rl in ((outs[0], outs[2]), (outs[1], outs[3])))
            rvec += recall_vector(c3, c2, outs[2].shape[1]).cpu().numpy()
        if svec is not None:
            accumulate_split(svec, out[4], out[5], out[6], zero_shot, n_rel)
    t = torch.from_numpy(np.concatenate([v for v in (vec, rvec, svec) if v is not None]))
    if device is not None:
        t = t.to(device)
    t = vdist.allreduce_metrics(t)
    if recall_k or svec is not None:
        return _summaries(t.cpu().numpy(), recall_k, svec is not None, use_2d, n_rel)
    return summarize(t.cpu().numpy(), n_rel, use_2d=use_2d)


def _summaries(v: np.ndarray, recall_k: bool = True, split: bool = False, use_2d: bool = True, n_rel: int = N_REL) -> Dict[str, float]:
    n = len(fields(n_rel))
    out = summarize(v[:n], n_rel, use_2d=use_2d)
    if recall_k:
        m = n + len(recall_fields(n_rel))
        out.update(recall_summarize(v[n:m], n_rel, use_2d=use_2d))
        n = m
    if split:
        out.update(split_summarize(v[n:n + len(split_fields())], use_2d))
    return out
