"""Zero-shot split of the triplet recall on the host (zeroshot.py, evaluate.accumulate_split): equal to what the reference's
get_zero_shot_recall returned on the golden cases (tests/golden/make_golden_zeroshot.py), NaN included; the table builder's
membership equal to the reference's per-row membership; the builder's quirks; and the split vector all-reduced over two gloo
ranks equal to one process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import evaluate as EV, zeroshot as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GDIR = os.path.join(ROOT, "tests", "golden")
GOLD = os.path.join(GDIR, "zeroshot_cases.npz")
TRAIN, VAL = os.path.join(GDIR, "zeroshot_train.json"), os.path.join(GDIR, "zeroshot_val.json")


def _names(f):
    with open(os.path.join(GDIR, f)) as fh:
        return [l.rstrip().lower() for l in fh if l.strip()]


OBJ, REL = _names("3dssg_classes.txt"), _names("3dssg_relations.txt")


def _same(got, want):
    np.testing.assert_array_equal(np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64))   # (NaN == NaN here)


def test_table_shape_and_size():
    t = Z.zero_shot_table(TRAIN, VAL, OBJ, REL)
    assert t.dtype == torch.uint8 and t.numel() == 665600
    assert 0 < int(t.sum()) < 665600


def test_drop_in_equals_reference_goldens():
    z = np.load(GOLD)
    table = Z.zero_shot_table(TRAIN, VAL, OBJ, REL)
    for name in z["case_names"]:
        t, cm = z[f"{name}_rank"], z[f"{name}_cm"]
        for kw in ({"train": TRAIN, "val": VAL}, {"table": table},
                   {"train": json.load(open(TRAIN)), "val": json.load(open(VAL))}):
            zs, nz, al = Z.get_zero_shot_recall(t, cm, OBJ, REL, **kw)
            _same(zs, z[f"{name}_zs"])
            _same(nz, z[f"{name}_nz"])
            _same(al, z[f"{name}_all"])
    assert np.isnan(z["nozs_zs"]).all() and np.isnan(z["none_all"]).all()


def test_table_membership_equals_reference_per_row():
    z = np.load(GOLD)
    table = Z.zero_shot_table(TRAIN, VAL, OBJ, REL).numpy()
    cm = z["member_cm"]
    got = np.array([table[(s * 160 + o) * 26 + p] == 1 for s, o, p in cm])
    np.testing.assert_array_equal(got, z["member_zs"])
    used, zs = Z.row_membership(cm, table, 26)
    assert used.all()
    np.testing.assert_array_equal(zs, z["member_zs"])


def _scan(name, objs, rels):
    return {"scan": name, "split": 0, "objects": objs, "relationships": rels}


def test_builder_quirks():
    objs = {"1": "chair", "2": "floor"}
    val = {"scans": [_scan("v", objs, [[1, 2, 15, "standing on"], [2, 1, 1, "attached to"]])]}
    k = lambda s, o, p: (OBJ.index(s) * 160 + OBJ.index(o)) * 26 + REL.index(p)
    # a training relationship whose ids are missing from its scan is skipped: the key stays zero-shot
    train = {"scans": [_scan("t", objs, [[1, 7, 15, "standing on"], [9, 2, 15, "standing on"]])]}
    t = Z.zero_shot_table(train, val, OBJ, REL).numpy()
    assert t[k("chair", "floor", "standing on")] == 1 and t[k("floor", "chair", "attached to")] == 1 and t.sum() == 2
    # every training scan counts (no scan list, whatever its name or split)
    train = {"scans": [_scan("not-in-any-list", objs, [[1, 2, 15, "standing on"]]) | {"split": 7}]}
    t = Z.zero_shot_table(train, val, OBJ, REL).numpy()
    assert t[k("chair", "floor", "standing on")] == 0 and t[k("floor", "chair", "attached to")] == 1 and t.sum() == 1
    # a key in neither file is not zero-shot; a key in train only is not either
    assert t[k("wall", "floor", "attached to")] == 0
    # a missing id in the validation file is an error (the reference: KeyError)
    bad = {"scans": [_scan("v-bad", objs, [[1, 5, 15, "standing on"]])]}
    with pytest.raises(KeyError, match="v-bad"):
        Z.zero_shot_table(train, bad, OBJ, REL)
    # unknown names: ValueError naming the scan and the label, in either file
    with pytest.raises(ValueError, match="unicorn") as e:
        Z.zero_shot_table({"scans": [_scan("t-unk", {"1": "unicorn", "2": "floor"}, [[1, 2, 15, "standing on"]])]}, val, OBJ, REL)
    assert "t-unk" in str(e.value)
    with pytest.raises(ValueError, match="flying over") as e:
        Z.zero_shot_table(train, {"scans": [_scan("v-unk", objs, [[1, 2, 3, "flying over"]])]}, OBJ, REL)
    assert "v-unk" in str(e.value)
    # the first occurrence of a duplicated name
    dup = ["chair", "floor", "chair"]
    t = Z.zero_shot_table({"scans": []}, val, dup, REL).numpy()
    assert t[(0 * 3 + 1) * 26 + REL.index("standing on")] == 1 and t.sum() == 2
    # the single-label list (with 'none' first) shifts every predicate index by one
    t = Z.zero_shot_table({"scans": []}, val, OBJ, ["none"] + REL).numpy()
    assert t[(OBJ.index("chair") * 160 + OBJ.index("floor")) * 27 + 1 + REL.index("standing on")] == 1


def test_row_forms():
    table = np.zeros(4 * 4 * 3, np.uint8)
    table[(1 * 4 + 2) * 3 + 0] = 1
    cm5 = np.array([[1, 9, 2, 9, 0], [1, 9, 2, 9, -1], [2, 9, 1, 9, 0], [5, 9, 2, 9, 0], [1, 9, 2, 9, 2]])
    used, zs = Z.row_membership(cm5, table, 3)
    assert used.tolist() == [True, False, True, True, True] and zs.tolist() == [True, False, False, False, False]
    used3, zs3 = Z.row_membership(cm5[:, [0, 2, 4]], table, 3)
    assert used3.tolist() == used.tolist() and zs3.tolist() == zs.tolist()
    with pytest.raises(RuntimeError):
        Z.row_membership(cm5[:, :4], table, 3)
    with pytest.raises(ValueError):
        Z.get_zero_shot_recall([1], cm5[:1], OBJ, REL)            # neither files nor a table


def _split_case(z, name):
    """(3D ranks, 2D ranks, cls_matrix): the golden ranks, and a shifted copy standing in for the 2D branch."""
    t = z[f"{name}_rank"]
    return t, np.minimum(t + 7, 200), z[f"{name}_cm"]


def test_accumulate_split_and_summary_equal_goldens():
    z = np.load(GOLD)
    table = Z.zero_shot_table(TRAIN, VAL, OBJ, REL)
    for name in z["case_names"]:
        t3, t2, cm = _split_case(z, name)
        v = EV.accumulate_split(np.zeros(len(EV.split_fields())), t3, t2, cm, table)
        s = EV.split_summarize(v)
        _same([s["zero_shot_recall@50_3d"], s["zero_shot_recall@100_3d"]], z[f"{name}_zs"])
        _same([s["non_zero_shot_recall@50_3d"], s["non_zero_shot_recall@100_3d"]], z[f"{name}_nz"])
        _same([s["all_zero_shot_recall@50_3d"], s["all_zero_shot_recall@100_3d"]], z[f"{name}_all"])
        want2 = Z.get_zero_shot_recall(t2, cm, OBJ, REL, table=table)
        _same([s["zero_shot_recall@50_2d"], s["zero_shot_recall@100_2d"]], want2[0])
        _same([s["all_zero_shot_recall@100_2d"]], [want2[2][1]])
    assert EV.split_fields()[0] == "zs_all_n_3d" and len(EV.split_fields()) == 12


_WORKER = r"""
import os, sys, numpy as np, torch
sys.path.insert(0, os.environ["VLSAT_ROOT"])
import vlsat_amd
from vlsat_amd import evaluate as EV, dist as vdist, zeroshot as Z
rank, local, world = vdist.init("gloo")
g = os.environ["VLSAT_GDIR"]
names = lambda f: [l.rstrip().lower() for l in open(os.path.join(g, f)) if l.strip()]
table = Z.zero_shot_table(os.path.join(g, "zeroshot_train.json"), os.path.join(g, "zeroshot_val.json"),
                          names("3dssg_classes.txt"), names("3dssg_relations.txt"))
z = np.load(os.path.join(g, "zeroshot_cases.npz"))
cases = list(z["case_names"])
vec = np.zeros(len(EV.split_fields()))
for i in vdist.shard(len(cases), rank, world):
    t = z[f"{cases[i]}_rank"]
    EV.accumulate_split(vec, t, np.minimum(t + 7, 200), z[f"{cases[i]}_cm"], table)
t = vdist.allreduce_metrics(torch.from_numpy(vec))
if rank == 0:
    print("VEC", " ".join(repr(float(x)) for x in t.tolist()))
"""


def test_two_rank_allreduce_equals_single_process(tmp_path):
    script = tmp_path / "w.py"
    script.write_text(_WORKER)
    env = dict(os.environ, VLSAT_ROOT=ROOT, VLSAT_GDIR=GDIR, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", "--master-port", "29643", str(script)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.array([float(x) for x in [l for l in r.stdout.splitlines() if l.startswith("VEC")][0].split()[1:]])
    z = np.load(GOLD)
    table = Z.zero_shot_table(TRAIN, VAL, OBJ, REL)
    vec = np.zeros(len(EV.split_fields()))
    for name in z["case_names"]:
        EV.accumulate_split(vec, *_split_case(z, name), table)
    assert np.array_equal(got, vec) and vec[0] > 0
