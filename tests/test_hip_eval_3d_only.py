"""3D-only evaluation (a NULL / None 2D input on vlsat_eval_counts, vlsat_eval_triplet_split, vlsat_process_val_counts[_split],
vlsat_forward_scene_graph and everything above them): the 3D outputs of the 3D-only forward are bit-identical to those of the full
forward, so EVERY comparison here is exact -- integers equal, floats bit-equal -- against the two-branch call on the same inputs; the
2D entries of the additive vectors are not touched (zero from zero, a sentinel stays a sentinel).

Two conventions:
  * a "2D key" ends in ``_2d`` or, for recall_summarize's pooled values, in ``_2d_pooled``: both belong to the 2D branch and are left
    out of a 3D-only summary (``_is_2d``).
  * validation(recall_k=True) with three workers: the per-scene recall SUMS (fp64, ``{v}_R@K`` / ``{v}_mR@K``) are added in the order
    the worker threads happened to take the scenes, which differs between any two runs, 3D-only or not; exact equality with the
    full run is asked of them with 0 and 1 worker (one summation order) and, with 3 workers, of every key that is a function of
    integer counts (all the others)."""
import ctypes

import numpy as np
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import VLSATConfig, evaluate as EV, lib as L, metrics as M, synth
from vlsat_amd.model import VLSATModel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 160
P = 32


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path cannot run and there is no fallback")


def _is_2d(name: str) -> bool:
    return name.endswith("_2d") or name.endswith("_2d_pooled")


def _check_vector(names, only3, full, what, in_2d=0):
    """only3 == full outside the 2D fields, == in_2d inside them; bit for bit (the float vectors hold sums of the same terms)"""
    only3, full = np.asarray(only3.cpu()), np.asarray(full.cpu())
    assert len(names) == len(only3) == len(full), what
    bad = [(f, a, b) for f, a, b in zip(names, only3.tolist(), full.tolist()) if a != (in_2d if _is_2d(f) else b)]
    assert not bad, (what, bad[:8])


# ---- 1. rank-table level, no model -----------------------------------------------------------------------------------------
def _random_tables(n, e, r, seed):
    g = torch.Generator().manual_seed(seed)
    gt_rel = (torch.rand(e, r, generator=g) < (0.5 if r == 1 else 0.08)).long()
    cnt = gt_rel.sum(1).clamp(min=1).int()
    tabs = []
    for _ in range(2):
        tabs.append({"obj_rank": torch.randint(1, 13, (n,), generator=g).int().to(DEV),
                     "rel_rank": torch.randint(1, 8, (e, r), generator=g).int().to(DEV),
                     "tri_rank": torch.randint(1, 103, (e, r), generator=g).int().to(DEV), "cnt": cnt.to(DEV)})
    gt_cls = torch.randint(0, C, (n,), generator=g).to(DEV)
    edges = torch.randint(0, n, (e, 2), generator=g).to(DEV)
    table = (torch.rand(C * C * r, generator=g) < 0.4).to(torch.uint8).to(DEV)
    return tabs[0], tabs[1], gt_cls, gt_rel.to(DEV), edges, table


@pytest.mark.parametrize("n,e,r", [(70, 300, 26), (300, 70, 26), (5, 0, 26), (40, 200, 1), (40, 200, 32)])
def test_rank_tables_without_the_2d_tables(n, e, r):
    _need_gpu()
    t3, t2, gt_cls, gt_rel, edges, table = _random_tables(n, e, r, 100 + n + e + r)
    F, S = EV.fields(r), EV.split_fields()
    tag = "tables"
    full = M.eval_counts(torch.zeros(len(F), dtype=torch.int64, device=DEV), t3, t2, gt_cls, gt_rel, edges, 3)
    zero = M.eval_counts(torch.zeros(len(F), dtype=torch.int64, device=DEV), t3, None, gt_cls, gt_rel, edges, 3)
    start = torch.tensor([7 if _is_2d(f) else 0 for f in F], dtype=torch.int64, device=DEV)
    kept = M.eval_counts(start.clone(), t3, None, gt_cls, gt_rel, edges, 3)
    sfull = M.eval_triplet_split(torch.zeros(12, dtype=torch.int64, device=DEV), t3, t2, gt_cls, gt_rel, edges, table)
    szero = M.eval_triplet_split(torch.zeros(12, dtype=torch.int64, device=DEV), t3, None, gt_cls, gt_rel, edges, table)
    sstart = torch.tensor([7 if _is_2d(f) else 0 for f in S], dtype=torch.int64, device=DEV)
    skept = M.eval_triplet_split(sstart.clone(), t3, None, gt_cls, gt_rel, edges, table)
    torch.cuda.synchronize()
    _check_vector(F, zero, full, (tag, "counts", n, e, r))
    _check_vector(F, kept, full, (tag, "counts, sentinel", n, e, r), in_2d=7)
    _check_vector(S, szero, sfull, (tag, "split", n, e, r))
    _check_vector(S, skept, sfull, (tag, "split, sentinel", n, e, r), in_2d=7)
    assert int(full[0]) == 3 and int(full[F.index("obj_n_3d")]) == n and int(full[F.index("obj_n_2d")]) == n
    if e and r > 1:
        assert int(sfull[0]) > 0 and int(sfull[3]) > 0


# ---- the model-level cases ---------------------------------------------------------------------------------------------------
def _batch(sizes, seed, n_rel=26, single=False, shuffle=False):
    """One batch of len(sizes) scenes on the device with random labels: multi-hot [E, R] with an edge without any relation and an edge
    with two, or (``single``) [E] labels with 0 = none.  ``shuffle``: the edges of every scene in random order, no fc_sizes hint."""
    b = synth.collate([synth.make_scene(n, P, seed * 100 + i) for i, n in enumerate(sizes)])
    g = torch.Generator().manual_seed(seed)
    n, e = b["obj_points"].shape[0], b["edge_indices"].shape[1]
    item = {k: torch.from_numpy(v).to(DEV) for k, v in b.items() if k != "edge_indices"}
    edges = torch.from_numpy(b["edge_indices"]).t().contiguous()
    if shuffle:
        start = 0
        for k in sizes:
            m = k * (k - 1)
            edges[start:start + m] = edges[start:start + m][torch.randperm(m, generator=g)]
            start += m
    else:
        item["fc_sizes"] = list(sizes)
    if single:
        gt_rel = torch.randint(0, n_rel, (e,), generator=g)
        gt_rel[::3] = 0
    else:
        gt_rel = (torch.rand(e, n_rel, generator=g) < 0.1).long()
        if e >= 2:
            gt_rel[0] = 0
            gt_rel[1] = 0
            gt_rel[1, [2, 11]] = 1
    item.update(gt_class=torch.randint(0, C, (n,), generator=g).to(DEV), gt_rel_cls=gt_rel.to(DEV), edge_indices=edges.to(DEV),
                n_scenes=len(sizes))
    return item


def _cases(**kw):
    return {"5+1+7": _batch([5, 1, 7], 31, **kw), "shuffled": _batch([5, 1, 7], 32, shuffle=True, **kw), "E=0": _batch([1, 1, 1], 33, **kw)}


@pytest.fixture(scope="module")
def multi_model():
    _need_gpu()
    cfg = VLSATConfig(N_LAYERS=1)
    m = VLSATModel(cfg, DEV).load_state(synth.make_weights(cfg)).eval()
    yield m
    m.close()


@pytest.fixture(scope="module")
def single_model():
    _need_gpu()
    cfg = VLSATConfig(N_LAYERS=1, multi_rel_outputs=False, num_rel_class=27)
    m = VLSATModel(cfg, DEV).load_state(synth.make_weights(cfg)).eval()
    yield m
    m.close()


@pytest.fixture(scope="module")
def zs_table():
    return (torch.rand(C * C * 26, generator=torch.Generator().manual_seed(9)) < 0.5).to(torch.uint8)


def _plan_info(model, b):
    plan = model._plan(b["edge_indices"].t(), b["batch_ids"], b["obj_points"].shape[0], P, b.get("fc_sizes"))
    s, ws, fc = ctypes.c_int32(), ctypes.c_size_t(), ctypes.c_int32()
    L.check(L.load().vlsat_plan_info(plan.handle, ctypes.byref(s), ctypes.byref(ws), ctypes.byref(fc)))
    return s.value, ws.value, fc.value


def _counts_pair(model, b, what, table=None, recall=False):
    """metrics.process_val_counts with and without the 2D features into fresh vectors; every vector compared"""
    r = model.config.num_rel_class
    F, RF, S = EV.fields(r), EV.recall_fields(r), EV.split_fields()
    out = []
    for f2d in (b["obj_2d_feats"], None):
        counts = torch.zeros(len(F), dtype=torch.int64, device=DEV)
        rec = torch.zeros(len(RF), dtype=torch.float64, device=DEV) if recall else None
        split = torch.zeros(len(S), dtype=torch.int64, device=DEV) if table is not None else None
        got = M.process_val_counts(model, counts, b["obj_points"], f2d, b["gt_class"], b["descriptor"], b["gt_rel_cls"], b["edge_indices"],
                                   b["batch_ids"], b["n_scenes"], b.get("fc_sizes"), recall=rec, split_table=table, split_counts=split)
        assert got is counts
        out.append((counts, rec, split))
    torch.cuda.synchronize()
    (cf, rf, sf), (c3, r3, s3) = out
    tag = what[0]
    _check_vector(F, c3, cf, (tag, "counts") + what)
    assert int(cf[0]) == b["n_scenes"]
    if recall:
        _check_vector(RF, r3, rf, (tag, "recall") + what)
    if table is not None:
        _check_vector(S, s3, sf, (tag, "split") + what)


@pytest.mark.parametrize("precision", ["fp32", "bf16_mixed"])
def test_one_call_step_without_2d_features(multi_model, zs_table, precision):
    """vlsat_process_val_counts[_split] with obj_2d_feats NULL (raises on the library before this feature)"""
    model = multi_model
    model.set_gemm_precision(precision)
    try:
        tab = zs_table.to(DEV)
        for name, b in _cases().items():
            before = _plan_info(model, b)
            _counts_pair(model, b, (name, precision))
            _counts_pair(model, b, (name, precision, "split"), table=tab)
            assert _plan_info(model, b) == before and before[0] == 3, (name, before)
            # the method itself took the one call (True), not the separate calls
            counts = torch.zeros(len(EV.fields()), dtype=torch.int64, device=DEV)
            assert model.process_val_counts(counts, b["obj_points"], None, b["gt_class"], b["descriptor"], b["gt_rel_cls"], b["edge_indices"],
                                            b["batch_ids"], 3, b.get("fc_sizes")) is True
    finally:
        model.set_gemm_precision("fp32")


def test_separate_call_route_without_2d_features(multi_model, single_model, zs_table):
    tab = zs_table.to(DEV)
    for name, b in _cases().items():
        _counts_pair(multi_model, b, (name, "recall"), recall=True)
        _counts_pair(multi_model, b, (name, "recall, split"), table=tab, recall=True)
    tab27 = (torch.rand(C * C * 27, generator=torch.Generator().manual_seed(10)) < 0.5).to(torch.uint8).to(DEV)
    for name, b in _cases(n_rel=27, single=True).items():
        _counts_pair(single_model, b, (name, "single-label"))
        _counts_pair(single_model, b, (name, "single-label, recall, split"), table=tab27, recall=True)
    # the one call stays refused for a single-label model, with or without the features
    b = _batch([5, 1, 7], 31, n_rel=27, single=True)
    counts = torch.zeros(len(EV.fields(27)), dtype=torch.int64, device=DEV)
    for f2d in (b["obj_2d_feats"], None):
        with pytest.raises(L.VlsatError, match="multi_rel_outputs"):
            single_model.process_val_counts(counts, b["obj_points"], f2d, b["gt_class"], b["descriptor"],
                                            M.multihot_targets(b["gt_rel_cls"], 27).contiguous(), b["edge_indices"], b["batch_ids"], 3, b["fc_sizes"])
    torch.cuda.synchronize()
    assert int(counts.sum()) == 0


def test_host_route_returns_none_in_the_2d_slots(multi_model):
    b = _batch([5, 1, 7], 31)
    args = (b["gt_class"], b["descriptor"], b["gt_rel_cls"], b["edge_indices"], b["batch_ids"])
    full = M.process_val(multi_model, b["obj_points"], b["obj_2d_feats"], *args, use_triplet=True)
    only = M.process_val(multi_model, b["obj_points"], None, *args, use_triplet=True)
    assert len(only) == len(full) == 10
    for i in (1, 3, 5):
        assert only[i] is None and full[i] is not None
    for i in (0, 2, 4, 6):
        np.testing.assert_array_equal(only[i], full[i])
    for i in (7, 8, 9):
        assert torch.equal(only[i].view(torch.int32), full[i].view(torch.int32))


def _assert_graph_equal(a, b, what):
    for k in M.SceneGraph.__slots__:
        x, y = getattr(a, k), getattr(b, k)
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k)
        if x.dtype == torch.float32:
            x, y = x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)
        assert torch.equal(x, y), (what, k)


@pytest.mark.parametrize("evaluate", ["triplet", "rels"])
def test_predicted_graph_without_2d_features(multi_model, single_model, evaluate):
    for model, kw in ((multi_model, {}), (single_model, dict(n_rel=27, single=True))):
        for name, b in _cases(**kw).items():
            args = (b["edge_indices"].t(), b["descriptor"], b["batch_ids"])
            opts = dict(top_k=20, topk_each=5, evaluate=evaluate, fc_sizes=b.get("fc_sizes"))
            g3, g2 = model.predict_graph(b["obj_points"], b["obj_2d_feats"], *args, **opts)
            only, none = model.predict_graph(b["obj_points"], None, *args, **opts)
            torch.cuda.synchronize()
            assert none is None and g2 is not None
            _assert_graph_equal(only, g3, (name, evaluate, kw))
            assert only.n_valid.numel() == 3 and (name == "E=0") == (int(only.n_valid.sum()) == 0)


# ---- the loops ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_batches():
    _need_gpu()
    return [_batch([n], 50 + i) for i, n in enumerate([5, 1, 7, 3, 9, 4])]


def _without_2d(batches, lacking=2):
    """the same dicts for the 3D-only run, one of them without the obj_2d_feats key"""
    return [{k: v for k, v in b.items() if not (i == lacking and k == "obj_2d_feats")} for i, b in enumerate(batches)]


def _check_summary(only, full, what, exact=lambda k: True):
    assert set(only) == {k for k in full if not _is_2d(k)}, (what, sorted(set(only) ^ {k for k in full if not _is_2d(k)})[:8])
    assert "scenes" in only and not [k for k in only if "_2d" in k]
    for k, v in only.items():
        if exact(k):
            assert np.array([v], np.float64).tobytes() == np.array([full[k]], np.float64).tobytes(), (what, k, v, full[k])


@pytest.mark.parametrize("workers", [0, 1, 3])
def test_validation_without_the_2d_branch(multi_model, scene_batches, zs_table, workers):
    only_batches = _without_2d(scene_batches)
    assert "obj_2d_feats" not in only_batches[2]
    for merge in (1, 2):
        for extra in ({}, {"zero_shot": zs_table}, {"recall_k": True}, {"recall_k": True, "zero_shot": zs_table}):
            kw = dict(device=DEV, workers=workers, merge=merge, **extra)
            full = EV.validation(multi_model, scene_batches, **kw)
            only = EV.validation(multi_model, only_batches, use_2d=False, **kw)
            assert full["scenes"] == 6
            # (see the module docstring: with several workers the fp64 per-scene recall sums have no fixed order in either run)
            order_free = (lambda k: not (("_R@" in k or "_mR@" in k) and not k.endswith("_pooled"))) if workers > 1 else (lambda k: True)
            _check_summary(only, full, (workers, merge, sorted(extra)), order_free)
            if "recall_k" in extra:
                assert "sgcls_ngc_R@100_3d" in only and "predcls_gc_mR@20_3d_pooled" in only
            if "zero_shot" in extra:
                assert "zero_shot_recall@100_3d" in only


def test_predict_loop_without_the_2d_branch(multi_model, scene_batches):
    opts = dict(top_k=20, topk_each=5, evaluate="triplet")
    want = [multi_model.predict_graph(b["obj_points"], None, b["edge_indices"].t(), b["descriptor"], b["batch_ids"], fc_sizes=b["fc_sizes"],
                                      **opts) for b in scene_batches]
    got = list(EV.predict(multi_model, _without_2d(scene_batches), device=DEV, workers=2, use_2d=False, **opts))
    serial = list(EV.predict(multi_model, _without_2d(scene_batches), use_2d=False, **opts))
    torch.cuda.synchronize()
    assert len(got) == len(serial) == len(want) == 6
    for i, ((w3, wn), (g3, g2), (s3, s2)) in enumerate(zip(want, got, serial)):
        assert wn is None and g2 is None and s2 is None
        _assert_graph_equal(g3, w3, ("workers=2", i))
        _assert_graph_equal(s3, w3, ("workers=0", i))
    # a merged batch comes back one scene at a time
    merged = EV.merge_batches(scene_batches[:3])
    per_scene = list(EV.predict(multi_model, [merged], use_2d=False, **opts))
    assert len(per_scene) == 3 and all(g2 is None and g3.n_valid.numel() == 1 for g3, g2 in per_scene)


# ---- 7. the C entry points: what goes together ----------------------------------------------------------------------------------
def test_c_level_refusals_and_all_null_forms(multi_model, zs_table):
    lib = L.load()
    err = lambda: lib.vlsat_last_error().decode()
    n, e, r = 70, 300, 26
    t3, t2, gt_cls, gt_rel, edges, table = _random_tables(n, e, r, 5)
    counts = torch.zeros(len(EV.fields(r)), dtype=torch.int64, device=DEV)
    two = (t2["obj_rank"].data_ptr(), t2["rel_rank"].data_ptr(), t2["tri_rank"].data_ptr())

    def eval_counts(mask):
        o2, r2, tr2 = (p if mask >> i & 1 else None for i, p in enumerate(two))
        return lib.vlsat_eval_counts(t3["obj_rank"].data_ptr(), o2, t3["rel_rank"].data_ptr(), r2, t3["tri_rank"].data_ptr(), tr2,
                                     t3["cnt"].data_ptr(), gt_cls.data_ptr(), gt_rel.data_ptr(), edges.data_ptr(), n, e, r, 1,
                                     counts.data_ptr(), L.stream_ptr())

    for mask in range(1, 7):                                            # one or two of the three NULL
        assert eval_counts(mask) != 0, mask
        assert "2D" in err(), (mask, err())
    torch.cuda.synchronize()
    assert int(counts.abs().sum()) == 0
    assert eval_counts(0) == 0 and eval_counts(7) == 0
    split = torch.zeros(12, dtype=torch.int64, device=DEV)
    assert lib.vlsat_eval_triplet_split(t3["tri_rank"].data_ptr(), None, t3["cnt"].data_ptr(), gt_cls.data_ptr(), gt_rel.data_ptr(),
                                        edges.data_ptr(), table.data_ptr(), e, C, r, split.data_ptr(), L.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert int(counts[0]) == 2 and int(split[0]) > 0 and int(split[6:].sum()) == 0

    # vlsat_forward_scene_graph: the features and the three 2D outputs, all or none; vlsat_process_val_counts[_split]: NULL features
    m, b = multi_model, _batch([5, 1, 7], 31)
    plan = m._plan(b["edge_indices"].t(), b["batch_ids"], b["obj_points"].shape[0], P, b["fc_sizes"])
    k = 16
    outs = [torch.zeros(3, k, 4, dtype=torch.int32, device=DEV), torch.zeros(3, k, device=DEV), torch.zeros(3, dtype=torch.int32, device=DEV),
            torch.zeros(3, k, 4, dtype=torch.int32, device=DEV), torch.zeros(3, k, device=DEV), torch.zeros(3, dtype=torch.int32, device=DEV)]
    e2 = b["edge_indices"].contiguous()

    def scene_graph(mask):                                              # bit 0: the features, bits 1..3: the 2D outputs
        f2d = b["obj_2d_feats"].data_ptr() if mask & 1 else None
        o2 = [t.data_ptr() if mask >> (i + 1) & 1 else None for i, t in enumerate(outs[3:])]
        return lib.vlsat_forward_scene_graph(m._h, plan.handle, b["obj_points"].data_ptr(), f2d, b["descriptor"].data_ptr(), e2.data_ptr(), 3, 0,
                                             k, 5, *[t.data_ptr() for t in outs[:3]], *o2, L.stream_ptr())

    for mask in range(1, 15):
        assert scene_graph(mask) != 0, mask
        assert "2D" in err(), (mask, err())
    torch.cuda.synchronize()
    assert all(int((t != 0).sum()) == 0 for t in outs)
    assert scene_graph(0) == 0
    torch.cuda.synchronize()
    assert int(outs[2].sum()) > 0 and all(int((t != 0).sum()) == 0 for t in outs[3:])
    assert scene_graph(15) == 0
    torch.cuda.synchronize()
    assert torch.equal(outs[2], outs[5]) and int(outs[5].sum()) > 0

    cnt, sp = torch.zeros(len(EV.fields()), dtype=torch.int64, device=DEV), torch.zeros(12, dtype=torch.int64, device=DEV)
    head = (m._h, plan.handle, b["obj_points"].data_ptr(), None, b["descriptor"].data_ptr(), b["gt_class"].data_ptr(),
            b["gt_rel_cls"].contiguous().data_ptr(), e2.data_ptr(), 3, cnt.data_ptr())
    assert lib.vlsat_process_val_counts(*head, L.stream_ptr()) == 0
    assert lib.vlsat_process_val_counts_split(*head, zs_table.to(DEV).data_ptr(), sp.data_ptr(), L.stream_ptr()) == 0
    torch.cuda.synchronize()
    F = EV.fields()
    assert int(cnt[0]) == 6 and int(cnt[F.index("obj_n_3d")]) == 26 and not [f for f, v in zip(F, cnt.tolist()) if _is_2d(f) and v]
    assert int(sp[0]) > 0 and int(sp[6:].sum()) == 0
