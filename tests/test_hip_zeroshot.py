"""GPU zero-shot split of the triplet recall (vlsat_eval_triplet_split, csrc/eval_ranks.hip): equal to the host counts
(zeroshot.split_counts_host, pinned to the reference's get_zero_shot_recall by tests/test_zeroshot_cpu.py) on the golden cases,
on a 64-scene x 40-object batch and on a configs[4]-sized scene; vlsat_process_val_counts_split equal to the separate calls;
validation(zero_shot=...) the same on the one-scene loop, the pipelined loop and the merged one, and without effect on the
summary it already returned."""
import os

import numpy as np
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import evaluate as EV, metrics as M, zeroshot as Z

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GDIR = os.path.join(ROOT, "tests", "golden")
GOLD = os.path.join(GDIR, "zeroshot_cases.npz")
C, R = 160, 26


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path cannot run and there is no fallback")


def _names(f):
    with open(os.path.join(GDIR, f)) as fh:
        return [l.rstrip().lower() for l in fh if l.strip()]


def _golden_table():
    return Z.zero_shot_table(os.path.join(GDIR, "zeroshot_train.json"), os.path.join(GDIR, "zeroshot_val.json"),
                             _names("3dssg_classes.txt"), _names("3dssg_relations.txt"))


def _tables_from_rows(cm, t3, t2):
    """A cls_matrix and its rank lists as the rank tables the kernels write: one edge (two nodes) per run of consecutive rows with
    the same (subject, object) and ascending predicates, slot j = the edge's j-th predicate; a -1 row is an edge without gt."""
    cm = np.asarray(cm)
    s_col, o_col = (0, 2) if cm.shape[1] == 5 else (0, 1)
    edges, cls, rel, tr3, tr2, cnt = [], [], [], [], [], []
    i = 0
    while i < len(cm):
        s, o, p = int(cm[i, s_col]), int(cm[i, o_col]), int(cm[i, -1])
        hot, r3, r2 = np.zeros(R, np.int64), np.zeros(R, np.int32), np.zeros(R, np.int32)
        if p < 0:
            r3[0], r2[0], n = t3[i], t2[i], 1
            i += 1
        else:
            n = 0
            while i < len(cm) and int(cm[i, s_col]) == s and int(cm[i, o_col]) == o and int(cm[i, -1]) >= 0 and not hot[int(cm[i, -1])] \
                    and (n == 0 or int(cm[i, -1]) > last):
                last = int(cm[i, -1])
                hot[last], r3[n], r2[n] = 1, t3[i], t2[i]
                n += 1
                i += 1
        edges.append((len(cls), len(cls) + 1))
        cls += [s, o]
        rel.append(hot); tr3.append(r3); tr2.append(r2); cnt.append(n)
    d = lambda x, t: torch.tensor(np.array(x), dtype=t, device=DEV)
    return (d(tr3, torch.int32), d(tr2, torch.int32), d(cnt, torch.int32), d(cls, torch.int64), d(rel, torch.int64),
            d(edges, torch.int64))


def _device_split(tr3, tr2, cnt, cls, rel, edges, table):
    out = torch.zeros(12, dtype=torch.int64, device=DEV)
    M.eval_triplet_split(out, {"tri_rank": tr3, "cnt": cnt}, {"tri_rank": tr2, "cnt": cnt}, cls, rel, edges,
                         table.to(DEV).contiguous())
    return out.cpu().numpy()


def test_kernel_equals_host_on_golden_cases():
    _need_gpu()
    z = np.load(GOLD)
    table = _golden_table()
    total = np.zeros(12, np.int64)
    for name in z["case_names"]:
        cm, t3 = z[f"{name}_cm"], z[f"{name}_rank"]
        t2 = np.minimum(t3 + 7, 200)
        got = _device_split(*_tables_from_rows(cm, t3, t2), table)
        want = np.concatenate([Z.split_counts_host(t3, cm, table, R), Z.split_counts_host(t2, cm, table, R)])
        np.testing.assert_array_equal(got, want, err_msg=str(name))
        total += got
        if name == "c5":                              # the kernel's counts give the reference's numbers
            s = EV.split_summarize(got.astype(np.float64))
            np.testing.assert_array_equal([s["zero_shot_recall@50_3d"], s["zero_shot_recall@100_3d"]], z["c5_zs"])
            np.testing.assert_array_equal([s["non_zero_shot_recall@50_3d"], s["non_zero_shot_recall@100_3d"]], z["c5_nz"])
            np.testing.assert_array_equal([s["all_zero_shot_recall@50_3d"], s["all_zero_shot_recall@100_3d"]], z["c5_all"])
    assert total[3] > 0 and total[0] > total[3]
    # classes outside [0, C): non-zero-shot rows, the table is not read past its end
    cm = np.array([[C, 1, 0, 1, 3], [-1, 1, 5, 1, 2], [3, 1, C + 40, 1, 25], [C - 1, 1, C - 1, 1, 25]], dtype=np.int64)
    tab = torch.ones(C * C * R, dtype=torch.uint8)
    t = np.array([10, 60, 120, 5])
    got = _device_split(*_tables_from_rows(cm, t, t), tab)
    assert got[:6].tolist() == [4, 2, 3, 1, 1, 1] and got[6:].tolist() == got[:6].tolist()


def _synth(n_scenes, n_obj, seed):
    g = torch.Generator().manual_seed(seed)
    n = n_scenes * n_obj
    ei = [(s * n_obj + a, s * n_obj + b) for s in range(n_scenes) for a in range(n_obj) for b in range(n_obj) if a != b]
    edges = torch.tensor(ei, dtype=torch.int64)
    e = edges.shape[0]
    gt_cls = torch.randint(0, C, (n,), generator=g)
    gt_rel = (torch.rand(e, R, generator=g) < 0.05).long()
    tabs = []
    for _ in range(2):
        obj = torch.randn(n, C, generator=g) * 6 * torch.rand(n, 1, generator=g)
        right = torch.rand(n, generator=g) < 0.5
        obj[right, gt_cls[right]] += 12
        rel = torch.sigmoid(torch.randn(e, R, generator=g) * 2)
        tabs.append((obj.to(DEV), rel.to(DEV)))
    table = (torch.rand(C * C * R, generator=g) < 0.4).to(torch.uint8)
    return tabs, gt_cls.to(DEV), gt_rel.to(DEV), edges.to(DEV), table


def _check_rank_tables(n_scenes, n_obj, seed):
    ((o3, r3), (o2, r2)), gt_cls, gt_rel, edges, table = _synth(n_scenes, n_obj, seed)
    t3 = M.rank_tables(o3, r3, gt_cls, gt_rel, edges, True)
    t2 = M.rank_tables(o2, r2, gt_cls, gt_rel, edges, True)
    got = _device_split(t3["tri_rank"], t2["tri_rank"], t3["cnt"], gt_cls, gt_rel, edges, table)
    cm = M.cls_matrix(gt_cls, gt_rel, edges, t3["obj_rank"]).cpu().numpy()
    used = torch.arange(R, device=DEV)[None, :] < t3["cnt"][:, None]
    want = np.concatenate([Z.split_counts_host(t["tri_rank"][used].cpu().numpy(), cm, table, R) for t in (t3, t2)])
    np.testing.assert_array_equal(got, want)
    assert got[3] > 0 and got[0] > got[3] and got[4] > 0 and got[1] > got[4]
    return edges.shape[0]


def test_kernel_equals_host_on_the_bench_batch_shape():
    """configs[1] shape: 64 scenes x 40 objects, E = 99 840, random labels and table, ranks from the ranking kernels."""
    _need_gpu()
    assert _check_rank_tables(64, 40, 61) == 99840


def test_kernel_equals_host_on_a_configs4_scene():
    _need_gpu()
    assert _check_rank_tables(1, 200, 62) == 39800


def _label_batches(n_batches, seed):
    from vlsat_amd import VLSATConfig, synth
    cfg = VLSATConfig(N_LAYERS=1)
    w = synth.make_weights(cfg)
    g = torch.Generator().manual_seed(seed)
    batches = []
    for s in range(n_batches):
        n = int(torch.randint(3, 12, (1,), generator=g))
        b = synth.collate([synth.make_scene(n, 32, 9500 + s)])
        e = b["edge_indices"].shape[1]
        item = {k: torch.from_numpy(v).to(DEV) for k, v in b.items() if k != "edge_indices"}
        item.update(gt_class=torch.randint(0, C, (n,), generator=g).to(DEV),
                    gt_rel_cls=(torch.rand(e, R, generator=g) < 0.15).long().to(DEV),
                    edge_indices=torch.from_numpy(b["edge_indices"]).t().contiguous().to(DEV), fc_sizes=[n])
        batches.append(item)
    table = (torch.rand(C * C * R, generator=g) < 0.5).to(torch.uint8)
    return cfg, w, batches, table


def test_process_val_counts_split_equals_the_separate_calls():
    _need_gpu()
    from vlsat_amd.model import VLSATModel
    cfg, w, batches, table = _label_batches(6, 41)
    model = VLSATModel(cfg, DEV).load_state(w).eval()
    tab = table.to(DEV)
    one, plain, sep = (torch.zeros(len(EV.fields()), dtype=torch.int64, device=DEV) for _ in range(3))
    split_one, split_sep = (torch.zeros(12, dtype=torch.int64, device=DEV) for _ in range(2))
    for b in batches:
        gt_cls, gt_rel, edges = b["gt_class"].contiguous(), b["gt_rel_cls"].contiguous(), b["edge_indices"].contiguous()
        args = (b["obj_points"], b["obj_2d_feats"], gt_cls, b["descriptor"], gt_rel, edges, b["batch_ids"], 1, b["fc_sizes"])
        assert model.process_val_counts(one, *args, split_table=tab, split_counts=split_one) is True
        assert model.process_val_counts(plain, *args) is True
        obj3, obj2, rel3, rel2 = model(b["obj_points"], b["obj_2d_feats"], edges.t().contiguous(), b["descriptor"], b["batch_ids"])
        t3 = M.rank_tables(obj3, rel3, gt_cls, gt_rel, edges, True)
        t2 = M.rank_tables(obj2, rel2, gt_cls, gt_rel, edges, True)
        M.eval_counts(sep, t3, t2, gt_cls, gt_rel, edges, 1)
        M.eval_triplet_split(split_sep, t3, t2, gt_cls, gt_rel, edges, tab)
    torch.cuda.synchronize()
    assert torch.equal(one, plain) and torch.equal(one, sep)
    assert torch.equal(split_one, split_sep) and int(split_one[3]) > 0, split_one.tolist()
    with pytest.raises(Exception):
        model.process_val_counts(one, *args, split_table=tab[:-1].contiguous(), split_counts=split_one)
    model.close()


def test_validation_zero_shot_agrees_between_loops():
    """validation(zero_shot=table): the one-scene host loop (workers=0), the pipelined loop (workers=4) and the merged one
    (workers=4, merge=16; compared with the host loop over the same merged batches, since merging changes the forward's last
    bits) report the same zero-shot split; every summary key that existed without it is unchanged."""
    _need_gpu()
    from vlsat_amd.model import VLSATModel
    cfg, w, batches, table = _label_batches(40, 43)
    model = VLSATModel(cfg, DEV).load_state(w).eval()
    zs_keys = [f"{g}_recall@{k}_{br}" for g in ("zero_shot", "non_zero_shot", "all_zero_shot") for k in (50, 100) for br in ("3d", "2d")]
    for kw in ({}, {"workers": 4}, {"workers": 4, "merge": 16}):
        plain = EV.validation(model, batches, device=DEV, **kw)
        got = EV.validation(model, batches, device=DEV, zero_shot=table, **kw)
        assert set(got) == set(plain) | set(zs_keys)
        assert {k: got[k] for k in plain} == plain, kw
        if not kw:
            s0 = got
        elif "merge" not in kw:
            assert {k: got[k] for k in zs_keys} == {k: s0[k] for k in zs_keys}
        else:
            merged = [EV.merge_batches(batches[i:i + 16]) for i in range(0, len(batches), 16)]
            host = EV.validation(model, merged, device=DEV, zero_shot=table)
            assert {k: got[k] for k in zs_keys} == {k: host[k] for k in zs_keys}
    assert all(np.isfinite(s0[k]) for k in zs_keys) and 0 < s0["zero_shot_recall@100_3d"] <= 100
    # with the Recall@K counts as well (the separate calls): the same split, both result groups present
    both = EV.validation(model, batches, device=DEV, workers=4, recall_k=True, zero_shot=table)
    assert {k: both[k] for k in zs_keys} == {k: s0[k] for k in zs_keys} and "sgcls_ngc_R@100_3d" in both
    both0 = EV.validation(model, batches, device=DEV, recall_k=True, zero_shot=table)
    assert both0 == pytest.approx(both, rel=1e-12, abs=1e-12, nan_ok=True)
