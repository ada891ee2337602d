"""Zero-shot split of the triplet recall: the host side of ``get_zero_shot_recall`` (reference
``src/utils/eva_utils_acc.py:267-333``, called by ``MMGNet.validation`` at ``src/model/model.py:253``).

A gt triplet (subject class, object class, predicate) is ZERO-SHOT when its key occurs in the validation annotations and
never in the training annotations; every other triplet -- one in neither file included -- is non-zero-shot.  The set is a
uint8 table over all keys, flat index ``(s * C + o) * R + p`` (665 600 bytes for C = 160, R = 26), built once per run by
``zero_shot_table`` and read by the counting kernel (``vlsat_eval_triplet_split``, csrc/eval_ranks.hip) or by
``split_counts_host`` / ``get_zero_shot_recall`` here."""
from __future__ import annotations

import json
import os
from typing import Sequence

import numpy as np
import torch


def _load(path_or_data) -> dict:
    if isinstance(path_or_data, (str, os.PathLike)):
        with open(path_or_data) as f:
            return json.load(f)
    return path_or_data


def _index(names: Sequence[str], name, scan: str, what: str) -> int:
    try:
        return names.index(name)                 # list.index: the first occurrence, as the reference
    except ValueError:
        raise ValueError(f"zero_shot_table: {what} {name!r} of scan {scan!r} is not in the {what} name list") from None


def zero_shot_table(train, val, obj_names: Sequence[str], rel_names: Sequence[str], device=None) -> torch.Tensor:
    """uint8 [C*C*R], 1 at ``(s*C + o)*R + p`` for every zero-shot key.  ``train`` / ``val``: relationships_train.json /
    relationships_validation.json as a path or the loaded dict.  As the reference builds it (eva_utils_acc.py:269-292):
    every scan of both files counts (no scan list, no skipped scan); a training relationship whose subject or object id is not
    among its scan's objects is skipped; in the validation file such a relationship is an error (the reference raises
    KeyError); an unknown class or predicate name raises ValueError.  ``rel_names`` is the dataset's relationNames: without
    'none' under multi_rel_outputs, the full list in single-label mode."""
    obj_names, rel_names = list(obj_names), list(rel_names)
    c, r = len(obj_names), len(rel_names)

    def key(scan, objs, rel):
        s = _index(obj_names, objs[str(rel[0])], scan, "object class")
        o = _index(obj_names, objs[str(rel[1])], scan, "object class")
        return (s * c + o) * r + _index(rel_names, rel[-1], scan, "predicate")

    seen = np.zeros(c * c * r, dtype=bool)
    for sc in _load(train)["scans"]:
        objs = sc["objects"]
        for rel in sc["relationships"]:
            if str(rel[0]) not in objs or str(rel[1]) not in objs:
                continue
            seen[key(sc.get("scan"), objs, rel)] = True
    table = np.zeros(c * c * r, dtype=np.uint8)
    for sc in _load(val)["scans"]:
        objs = sc["objects"]
        for rel in sc["relationships"]:
            for i in rel[:2]:
                if str(i) not in objs:
                    raise KeyError(f"zero_shot_table: validation scan {sc.get('scan')!r} has a relationship with object id {i} "
                                   "that is not among its objects")
            k = key(sc.get("scan"), objs, rel)
            if not seen[k]:
                table[k] = 1
    out = torch.from_numpy(table)
    return out if device is None else out.to(device)


def table_shape(table, n_rel: int) -> int:
    """The object class count C of a flat [C*C*R] table."""
    n = int(table.numel() if isinstance(table, torch.Tensor) else np.asarray(table).size)
    c = int(round((n // max(n_rel, 1)) ** 0.5)) if n_rel > 0 else 0
    if n_rel <= 0 or c * c * n_rel != n:
        raise ValueError(f"zero-shot table of {n} entries is not C*C*R for R = {n_rel}")
    return c


def row_membership(cls_matrix, table, n_rel: int):
    """(rows with a predicate: bool [n], zero-shot: bool [n]) of a cls_matrix (5 columns: keys on 0, 2, 4; 3 columns: 0, 1, 2)."""
    cm = np.asarray(cls_matrix)
    if cm.size == 0:
        return np.zeros(0, bool), np.zeros(0, bool)
    if cm.ndim != 2 or cm.shape[1] not in (3, 5):
        raise RuntimeError("unknown triplet length:", cm.shape[-1] if cm.ndim else 0)
    cm = cm.astype(np.int64)
    s, o, p = (cm[:, 0], cm[:, 2], cm[:, 4]) if cm.shape[1] == 5 else (cm[:, 0], cm[:, 1], cm[:, 2])
    tab = (table.cpu().numpy() if isinstance(table, torch.Tensor) else np.asarray(table)).reshape(-1)
    c = table_shape(tab, n_rel)
    used = p != -1
    inr = used & (s >= 0) & (s < c) & (o >= 0) & (o < c) & (p >= 0) & (p < n_rel)
    zs = np.zeros(len(cm), bool)
    zs[inr] = tab[((s[inr] * c + o[inr]) * n_rel + p[inr])] != 0
    return used, zs


def split_counts_host(triplet_rank, cls_matrix, table, n_rel: int) -> np.ndarray:
    """int64 [6]: all_n, all_hit@50, all_hit@100, zs_n, zs_hit@50, zs_hit@100 of one branch's triplet ranks (rows aligned with
    cls_matrix, as process_val returns them)."""
    used, zs = row_membership(cls_matrix, table, n_rel)
    t = np.asarray(triplet_rank).reshape(-1)[:len(used)]
    out = np.zeros(6, np.int64)
    for base, m in ((0, used), (3, used & zs)):
        out[base] = int(m.sum())
        out[base + 1] = int((m & (t <= 50)).sum())
        out[base + 2] = int((m & (t <= 100)).sum())
    return out


def recall_from_counts(n, hit) -> float:
    """``(ranks <= K).mean() * 100`` from counts; NaN for an empty group, as numpy's mean of an empty array."""
    return float(hit / n * 100) if n else float("nan")


def get_zero_shot_recall(triplet_rank, cls_matrix, obj_names, rel_name, *, train=None, val=None, table=None):
    """Drop-in for the reference's ``get_zero_shot_recall(triplet_rank, cls_matrix, obj_names, rel_name)``: returns
    ``(zero_shot@50, @100), (non_zero_shot@50, @100), (all@50, @100)`` in percent (NaN for an empty group).  The reference reads
    its two annotation files from fixed paths: pass them as ``train`` / ``val`` (paths or dicts), or a prebuilt ``table``."""
    r = len(rel_name)
    if table is None:
        if train is None or val is None:
            raise ValueError("get_zero_shot_recall: give train and val, or a prebuilt table")
        table = zero_shot_table(train, val, obj_names, rel_name)
    a = split_counts_host(triplet_rank, cls_matrix, table, r)
    zs = (recall_from_counts(a[3], a[4]), recall_from_counts(a[3], a[5]))
    nz = (recall_from_counts(a[0] - a[3], a[1] - a[4]), recall_from_counts(a[0] - a[3], a[2] - a[5]))
    al = (recall_from_counts(a[0], a[1]), recall_from_counts(a[0], a[2]))
    return zs, nz, al
