"""Scene-graph Recall@K / mR@K (metrics.recallk_counts and the drop-ins of the reference's evaluate_triplet_recallk /
evaluate_triplet_mrecallk) on the host path: equal to the reference goldens (tests/golden/make_golden_recallk.py), to a
literal materialisation of the 160 x 160 x 26 products, additive over shards; validation(recall_k=False) unchanged."""
import os

import numpy as np
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import evaluate as EV, metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "recallk_cases.npz")
VARIANTS = (("predcls_gc", "rels", 1), ("predcls_ngc", "rels", 100), ("sgcls_gc", "triplet", 1), ("sgcls_ngc", "triplet", 100))


def _load():
    z = np.load(GOLD)
    return z, int(z["n_cases"])


def _inputs(z, i, br):
    t = lambda k: torch.from_numpy(z[f"c{i}_{k}"])
    return t(f"obj_logits_{br}"), t(f"rel_{br}"), t("gt_cls"), t("gt_rel"), t("edges"), bool(z[f"c{i}_multi"])


def _gt_list(gt_cls, gt_rel, edges, multi):
    out = []
    for e, (a, b) in enumerate(edges.tolist()):
        if multi:
            rels = [k for k in range(gt_rel.shape[1]) if int(gt_rel[e, k]) == 1]
        else:
            rels = [int(gt_rel[e])] if int(gt_rel[e]) > 0 else []
        out.append((int(gt_cls[a]), int(gt_cls[b]), rels))
    return out


def golden_from_counts(row, r, name):
    """(recall[3], mrecall[26][3]) of one scene's counts row, with the reference's NaN / -1."""
    base = M.recallk_offset(name, r)
    with np.errstate(invalid="ignore", divide="ignore"):
        rec = np.array([row[base + q] for q in range(3)], dtype=np.int64) / int(row[0])
    mrec = np.array([[row[base + 3 + q * r + j] / row[1 + j] if row[1 + j] else -1 for q in range(3)] for j in range(26)],
                    dtype=np.float64)
    return rec, mrec


@pytest.mark.parametrize("br", ["3d", "2d"])
def test_host_counts_equal_reference_goldens(br):
    z, n = _load()
    for i in range(n):
        obj, rel, gt_cls, gt_rel, edges, multi = _inputs(z, i, br)
        row = M.recallk_counts(obj, rel, gt_cls, gt_rel, edges, None, 1, multi)[0].numpy()
        for name, _, _ in VARIANTS:
            rec, mrec = golden_from_counts(row, rel.shape[1], name)
            np.testing.assert_array_equal(rec, z[f"c{i}_R_{name}_{br}"], err_msg=f"case {i} {name}")
            np.testing.assert_array_equal(mrec, z[f"c{i}_mR_{name}_{br}"], err_msg=f"case {i} {name}")


def test_dropins_return_what_the_reference_returned():
    z, n = _load()
    for i in range(n):
        obj, rel, gt_cls, gt_rel, edges, multi = _inputs(z, i, "3d")
        gt = _gt_list(gt_cls, gt_rel, edges, multi)
        for name, ev, each in VARIANTS:
            rec = M.evaluate_triplet_recallk(obj, rel, gt, edges, multi, [20, 50, 100], each, use_clip=True, evaluate=ev)
            mrec = M.evaluate_triplet_mrecallk(obj, rel, gt, edges, multi, [20, 50, 100], each, use_clip=True, evaluate=ev)
            assert isinstance(rec, np.ndarray) and rec.dtype == np.float64
            np.testing.assert_array_equal(rec, z[f"c{i}_R_{name}_3d"])
            assert len(mrec) == 26 and all(len(row) == 3 for row in mrec)
            np.testing.assert_array_equal(np.array(mrec, dtype=np.float64), z[f"c{i}_mR_{name}_3d"])
            assert all(x == -1 and isinstance(x, int) for row in mrec for x in row if not isinstance(x, np.floating))


def _brute_counts(obj, rel, gt_cls, gt_rel, edges, multi):
    """The counting definition over the MATERIALISED products of a one-scene case: candidates = each edge's topk_each largest
    entries; hit at K when a correct candidate has fewer than K candidates of the scene strictly above it."""
    probs = torch.softmax(obj, -1)
    r = rel if multi else rel.exp()
    hot = M.multihot_targets(gt_rel, r.shape[1]) == 1
    out = {}
    for name, ev, each in VARIANTS:
        cands, corrs = [], []
        for e, (a, b) in enumerate(edges.tolist()):
            if ev == "triplet":
                full = ((probs[a][:, None] * probs[b][None, :])[:, :, None] * r[e][None, None, :]).reshape(-1)
                corr = (probs[a, gt_cls[a]] * probs[b, gt_cls[b]]) * r[e][hot[e]]
            else:
                full, corr = r[e], r[e][hot[e]]
            top = full.topk(min(each, full.numel())).values
            cands.append(top)
            corrs.append(corr[corr >= top[-1]])                  # correct entries that are candidates
        allc = torch.cat(cands)
        hits = []
        for k in (20, 50, 100):
            hits.append(sum(1 for c in corrs if len(c) and bool(((allc[None, :] > c[:, None]).sum(1) < k).any())))
        out[name] = hits
    return out


def test_host_counts_equal_materialised_products():
    z, _ = _load()
    for i in (0, 4, 6):                                          # small cases: 15, 90, 72 edges (665 600 products each)
        obj, rel, gt_cls, gt_rel, edges, multi = _inputs(z, i, "2d")
        row = M.recallk_counts(obj, rel, gt_cls, gt_rel, edges, None, 1, multi)[0].numpy()
        want = _brute_counts(obj, rel, gt_cls, gt_rel, edges, multi)
        r = rel.shape[1]
        for name, _, _ in VARIANTS:
            base = M.recallk_offset(name, r)
            assert list(row[base:base + 3]) == want[name], (i, name)


def _batch(z, cases, br):
    """Multi-label cases collated as one batch (node offsets on the edges, scene ids per node)."""
    objs, rels, gcls, grel, edges, bids, off = [], [], [], [], [], [], 0
    for s, i in enumerate(cases):
        obj, rel, gt_cls, gt_rel, e, multi = _inputs(z, i, br)
        assert multi
        objs.append(obj); rels.append(rel); gcls.append(gt_cls); grel.append(gt_rel); edges.append(e + off)
        bids.append(torch.full((obj.shape[0],), s, dtype=torch.int64))
        off += obj.shape[0]
    return torch.cat(objs), torch.cat(rels), torch.cat(gcls), torch.cat(grel), torch.cat(edges), torch.cat(bids)


MULTI_CASES = (0, 1, 3, 6)


def test_batch_equals_one_scene_calls_and_shards_add_up():
    z, _ = _load()
    obj, rel, gt_cls, gt_rel, edges, bid = _batch(z, MULTI_CASES, "3d")
    whole = M.recallk_counts(obj, rel, gt_cls, gt_rel, edges, bid, len(MULTI_CASES), True)
    for s, i in enumerate(MULTI_CASES):
        o, r_, gc, gr, e, _ = _inputs(z, i, "3d")
        assert torch.equal(whole[s], M.recallk_counts(o, r_, gc, gr, e, None, 1, True)[0]), i
    # two shards of the scene list: their recall vectors add up to the one-process vector
    obj2, rel2, *_ = _batch(z, MULTI_CASES, "2d")
    whole2 = M.recallk_counts(obj2, rel2, gt_cls, gt_rel, edges, bid, len(MULTI_CASES), True)
    v = EV.recall_vector(whole, whole2, 26)
    parts = EV.recall_vector(whole[:2], whole2[:2], 26) + EV.recall_vector(whole[2:], whole2[2:], 26)
    assert v.shape == (len(EV.recall_fields()),)
    torch.testing.assert_close(v, parts, rtol=1e-14, atol=0)
    s = EV.recall_summarize(v.numpy())
    # per-scene average over the scenes with a gt edge == the mean of the reference's per-scene recalls
    for name, _, _ in VARIANTS:
        want = np.mean([z[f"c{i}_R_{name}_3d"] for i in MULTI_CASES if not np.isnan(z[f"c{i}_R_{name}_3d"][0])], 0) * 100
        got = [s[f"{name}_R@{k}_3d"] for k in (20, 50, 100)]
        np.testing.assert_allclose(got, want, rtol=1e-12)
        assert f"{name}_R@20_2d_pooled" in s and f"{name}_mR@100_3d" in s


def test_validation_without_recall_is_unchanged():
    """recall_k=False (the default): the same keys and values as the loop always returned, and fields() unchanged."""
    assert len(EV.fields()) == 1 + 26 + 2 * (11 + 6 * 26)
    assert not set(EV.fields()) & set(EV.recall_fields())

    class Fake:                                                   # a model with fixed outputs, no GPU needed
        class config:
            multi_rel_outputs = True

        def __init__(self, z):
            self.o = [torch.from_numpy(z[f"c1_{k}"]) for k in ("obj_logits_3d", "obj_logits_2d", "rel_3d", "rel_2d")]

        def __call__(self, *a, **k):
            return self.o

    z, _ = _load()
    model = Fake(z)
    edges = torch.from_numpy(z["c1_edges"])
    b = dict(obj_points=None, obj_2d_feats=None, descriptor=None, gt_class=torch.from_numpy(z["c1_gt_cls"]),
             gt_rel_cls=torch.from_numpy(z["c1_gt_rel"]), edge_indices=edges,
             batch_ids=torch.zeros(12, 1, dtype=torch.int64))
    calls = []

    def fake_process_val(model_, *a, **k):                        # the rank lists come from the GPU kernels; fixed here
        calls.append(1)
        e = edges.shape[0]
        ranks = [np.ones(12, np.int64), np.ones(12, np.int64), np.ones(e, np.int64), np.ones(e, np.int64),
                 np.full(e, 7, np.int64), np.full(e, 7, np.int64), np.zeros((e, 5), np.int64)]
        return tuple(ranks) + (None, None, None)

    orig_from = M._process_val_from
    M._process_val_from = lambda model_, outs, *a: fake_process_val(model_)
    try:
        plain = EV.validation(model, [b])
        with_rk = EV.validation(model, [b], recall_k=True)
    finally:
        M._process_val_from = orig_from
    vec = EV.accumulate(np.zeros(len(EV.fields())), dict(zip(("top_k_obj", "top_k_obj_2d", "top_k_rel", "top_k_rel_2d",
                                                              "top_k_triplet", "top_k_triplet_2d"), fake_process_val(None)[:6])),
                        np.zeros((edges.shape[0], 5), np.int64), 1)
    assert plain == EV.summarize(vec)
    assert set(with_rk) == set(plain) | set(EV.recall_summarize(np.zeros(len(EV.recall_fields()))))
    assert {k: with_rk[k] for k in plain} == plain
    assert with_rk["sgcls_ngc_R@100_3d"] == pytest.approx(z["c1_R_sgcls_ngc_3d"][2] * 100, rel=1e-12)
