#!/usr/bin/env python3
"""Golden vectors for the zero-shot split of the triplet recall: get_zero_shot_recall of the reference
(src/utils/eva_utils_acc.py:267-333, called by MMGNet.validation at src/model/model.py:253), called directly.

The reference reads relationships_train.json / relationships_validation.json from fixed paths through the module-level
read_json; the generator replaces that function with one returning two fixtures, written next to this script:
  zeroshot_val.json    20 scans cut from data/3DSSG_subset/relationships_validation.json (at most 30 relationships each)
  zeroshot_train.json  synthetic: about half of the validation keys, some of them only on relationships whose subject or object
                       id is missing from the scan (the reference skips those, so their keys stay zero-shot), and keys of
                       triplets that never occur in the validation scans
Names: 3dssg_classes.txt / 3dssg_relations.txt (relationNames without 'none': the multi_rel_outputs list).

zeroshot_cases.npz holds, per case, the cls_matrix, the triplet ranks and the reference's three tuples (5-column and
3-column matrices, -1 rows, ranks on both sides of 50 and 100, a case without zero-shot rows (NaN), one with no row at all),
and the reference's membership of every row of a matrix that lists every validation key plus others: one call per row with
rank 1 on that row and 101 elsewhere, membership = zero_shot[0] > 0."""
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
from src.utils import eva_utils_acc as A  # noqa: E402

VAL_SRC = "/root/reference/data/3DSSG_subset/relationships_validation.json"


def names(f):
    with open(os.path.join(HERE, f)) as fh:
        return [l.rstrip().lower() for l in fh if l.strip()]


def main():
    obj_names, rel_names = names("3dssg_classes.txt"), names("3dssg_relations.txt")
    rng = np.random.default_rng(2023)
    src = json.load(open(VAL_SRC))["scans"]
    pick = np.linspace(0, len(src) - 1, 20).astype(int)
    val_scans = []
    for i in pick:
        sc = src[int(i)]
        rels = sc["relationships"][:30]
        used = {str(r[0]) for r in rels} | {str(r[1]) for r in rels}
        val_scans.append({"scan": sc["scan"], "split": sc["split"], "objects": {k: v for k, v in sc["objects"].items() if k in used},
                          "relationships": rels})
    val = {"scans": val_scans}
    key = lambda s, o, p: (obj_names.index(s), obj_names.index(o), rel_names.index(p))
    vkeys = sorted({key(sc["objects"][str(r[0])], sc["objects"][str(r[1])], r[-1]) for sc in val_scans for r in sc["relationships"]})
    perm = rng.permutation(len(vkeys))
    seen = [vkeys[i] for i in perm[:len(vkeys) // 2]]
    dropped = [vkeys[i] for i in perm[len(vkeys) // 2:len(vkeys) // 2 + 12]]        # only behind missing ids: stay zero-shot
    vset = set(vkeys)
    other = []
    while len(other) < 40:
        k = (int(rng.integers(len(obj_names))), int(rng.integers(len(obj_names))), int(rng.integers(len(rel_names))))
        if k not in vset and k not in other:
            other.append(k)
    train_scans = []
    todo = [(k, False) for k in seen + other] + [(k, True) for k in dropped]
    order = rng.permutation(len(todo))
    for t in range(0, len(order), 9):
        objs, rels = {}, []
        for j in order[t:t + 9]:
            (s, o, p), missing = todo[j]
            a, b = str(len(objs) + 1), str(len(objs) + 2)
            objs[a], objs[b] = obj_names[s], obj_names[o]
            if missing:
                rels.append([int(a), 900 + len(rels), p + 1, rel_names[p]] if len(rels) % 2 else [900 + len(rels), int(b), p + 1, rel_names[p]])
            else:
                rels.append([int(a), int(b), p + 1, rel_names[p]])
        train_scans.append({"scan": f"synthetic-train-{t // 9:02d}", "split": t % 3, "objects": objs, "relationships": rels})
    train = {"scans": train_scans}
    with open(os.path.join(HERE, "zeroshot_val.json"), "w") as f:
        json.dump(val, f, separators=(",", ":"))
    with open(os.path.join(HERE, "zeroshot_train.json"), "w") as f:
        json.dump(train, f, separators=(",", ":"))

    A.read_json = lambda split: {"train": train, "val": val}[split]
    zs_keys = [k for k in vkeys if k not in set(seen)]
    ns_keys = seen

    def rows(n, keys_zs, keys_nz, n_none, n_other, width):
        out = []
        for _ in range(n):
            pool = rng.integers(4)
            if pool == 0 and keys_zs:
                s, o, p = keys_zs[int(rng.integers(len(keys_zs)))]
            elif pool == 1 and n_other:
                s, o, p = other[int(rng.integers(len(other)))] if rng.random() < 0.5 else \
                    (int(rng.integers(160)), int(rng.integers(160)), int(rng.integers(26)))
            else:
                s, o, p = keys_nz[int(rng.integers(len(keys_nz)))]
            out.append([s, int(rng.integers(1, 12)), o, int(rng.integers(1, 12)), p])
        for _ in range(n_none):
            out.insert(int(rng.integers(len(out) + 1)), [int(rng.integers(160)), 1, int(rng.integers(160)), 2, -1])
        cm = np.array(out, dtype=np.int64).reshape(-1, 5)
        return cm if width == 5 else cm[:, [0, 2, 4]]

    def ranks(n):
        r = rng.integers(1, 160, n)
        fixed = [49, 50, 51, 99, 100, 101, 102, 1]
        r[:min(n, len(fixed))] = fixed[:n]
        return rng.permutation(r).astype(np.int64)

    cases = {"c5": rows(220, zs_keys, ns_keys, 30, 1, 5), "c3": rows(180, zs_keys, ns_keys, 25, 1, 3),
             "nozs": rows(60, [], ns_keys, 5, 0, 5), "none": rows(0, [], ns_keys, 4, 0, 5)}
    out = {"case_names": np.array(list(cases))}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)              # mean of an empty array
        for name, cm in cases.items():
            t = ranks(len(cm))
            zs, nz, al = A.get_zero_shot_recall(t, cm, obj_names, rel_names)
            out[f"{name}_cm"], out[f"{name}_rank"] = cm, t
            out[f"{name}_zs"], out[f"{name}_nz"], out[f"{name}_all"] = np.array(zs), np.array(nz), np.array(al)
        assert np.isnan(out["nozs_zs"]).all() and np.isnan(out["none_all"]).all() and not np.isnan(out["c5_zs"]).any()
        member = np.array([list(k) for k in vkeys + other + [(0, 0, 0), (159, 159, 25)]], dtype=np.int64)
        got = []
        for i in range(len(member)):
            t = np.full(len(member), 101, np.int64)
            t[i] = 1
            got.append(A.get_zero_shot_recall(t, member, obj_names, rel_names)[0][0] > 0)
    out["member_cm"], out["member_zs"] = member, np.array(got)
    assert 0 < int(out["member_zs"].sum()) < len(vkeys)
    np.savez_compressed(os.path.join(HERE, "zeroshot_cases.npz"), **out)
    print({k: (v.shape, v.dtype) for k, v in out.items()}, "zero-shot keys", int(out["member_zs"].sum()), "of", len(vkeys))


if __name__ == "__main__":
    main()
