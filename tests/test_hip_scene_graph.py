"""The predicted scene graph on the GPU (csrc/scene_graph.hip via vlsat_scene_graph_topk / vlsat_forward_scene_graph): equal
to the reference's pred_triplets on the goldens, the output contract against a brute force over the full product at the
benchmark's batch shape and on a configs[4]-sized scene, ties and odd graphs, agreement with the pinned Recall@K counts, and
predict_graph / evaluate.predict equal to the separate calls."""
import os

import numpy as np
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import evaluate as EV, lib as L, metrics as M

from scene_graph_checks import check_contract, edge_candidates, graphs_equal, three_valued_scene
from test_scene_graph_cpu import GOLD, VARIANTS, assert_golden, golden_case, golden_probs, golden_rows, hits_from_graph, tie_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path cannot run and there is no fallback")


@pytest.mark.parametrize("br", ["3d", "2d"])
def test_hip_equals_reference_pred_triplets(br):
    _need_gpu()
    z = np.load(GOLD)
    for i in range(int(z["n_cases"])):
        obj, rel, edges, probs, multi = golden_case(z, i, br, DEV)
        for evaluate, each in VARIANTS:
            rows, score = golden_rows(z, i, br, evaluate, each, edges.cpu())
            relp = golden_probs(z, i, br, rel, multi, DEV)
            g = M.scene_graph_topk(obj, relp, edges, None, 1, True, 100, each, evaluate, obj_probs=probs)
            assert_golden(g, rows, score, exact=True)
            g = M.scene_graph_topk(obj, rel, edges, None, 1, multi, 100, each, evaluate)          # the device softmax and exp
            assert_golden(g, rows, score, exact=False)
            g50 = M.scene_graph_topk(obj, relp, edges, None, 1, True, 50, each, evaluate, obj_probs=probs)
            assert_golden(g50, rows[:50], score[:50], exact=True)


@pytest.mark.parametrize("br", ["3d", "2d"])
def test_hip_lists_reproduce_the_pinned_recall_counts(br):
    _need_gpu()
    z = np.load(GOLD)
    names = {("triplet", 1): "sgcls_gc", ("triplet", 100): "sgcls_ngc", ("rels", 1): "predcls_gc", ("rels", 100): "predcls_ngc"}
    for i in range(int(z["n_cases"])):
        obj, rel, edges, probs, multi = golden_case(z, i, br, DEV)
        gt_cls, gt_rel = torch.from_numpy(z[f"c{i}_gt_cls"]).to(DEV), torch.from_numpy(z[f"c{i}_gt_rel"]).to(DEV)
        hot = M.multihot_targets(gt_rel, rel.shape[1]) == 1
        counts = M.recallk_counts(obj, rel, gt_cls, gt_rel, edges, None, 1, multi, obj_probs=probs)[0]
        for (evaluate, each), name in names.items():
            g = M.scene_graph_topk(obj, rel, edges, None, 1, multi, 100, each, evaluate, obj_probs=probs)
            base = M.recallk_offset(name, rel.shape[1])
            assert hits_from_graph(g, 0, gt_cls, hot, edges, evaluate) == counts[base:base + 3].tolist(), (i, name)


def _synth(n_scenes, n_obj, multi, seed, sharp):
    """The recipe of tests/test_hip_recallk.py: a fully connected batch with random outputs, logits whose scale varies per object."""
    g = torch.Generator().manual_seed(seed)
    n = n_scenes * n_obj
    ei = [(s * n_obj + a, s * n_obj + b) for s in range(n_scenes) for a in range(n_obj) for b in range(n_obj) if a != b]
    edges = torch.tensor(ei, dtype=torch.int64)
    e = edges.shape[0]
    bid = torch.arange(n_scenes).repeat_interleave(n_obj)
    gt_cls = torch.randint(0, 160, (n,), generator=g)
    gt_rel = (torch.rand(e, 26, generator=g) < 0.05).long() if multi else torch.randint(0, 26, (e,), generator=g)
    outs = []
    for _ in range(2):
        obj = torch.randn(n, 160, generator=g) * sharp * torch.rand(n, 1, generator=g)
        right = torch.rand(n, generator=g) < 0.5
        obj[right, gt_cls[right]] += 2 * sharp
        zz = torch.randn(e, 26, generator=g) * 2
        rel = torch.sigmoid(zz) if multi else torch.log_softmax(zz, -1)
        outs.append((obj, rel))
    to = lambda t: t.to(DEV)
    return [(to(o), to(r)) for o, r in outs], to(edges), to(bid)


def _scale_check(n_scenes, n_obj, seed, multi=True):
    outs, edges, bid = _synth(n_scenes, n_obj, multi, seed, sharp=6.0)
    obj, rel = outs[0]
    probs = M.softmax_rows(obj)
    rp = rel if multi else M.exp_probs(rel)             # the probabilities the selection scores with
    scene = bid[edges[:, 0]]
    bids = bid if n_scenes > 1 else None
    for evaluate in ("triplet", "rels"):
        cand = edge_candidates(probs, rp, edges, evaluate, 100)
        for top_k in (1, 20, 100, 1024):
            for each in (1, 7, 100):
                g = M.scene_graph_topk(obj, rel, edges, bids, n_scenes, multi, top_k, each, evaluate, obj_probs=probs)
                check_contract(g, probs, rp, edges, scene, n_scenes, top_k, each, evaluate, cand=cand)
    return obj, rel, probs, edges, bid


def test_hip_contract_on_the_bench_batch_shape():
    """configs[1] shape: 64 scenes x 40 objects, E = 99 840; a batch equals its scenes called one at a time; two calls agree."""
    _need_gpu()
    obj, rel, probs, edges, bid = _scale_check(64, 40, 52)
    assert edges.shape[0] == 99840
    whole = M.scene_graph_topk(obj, rel, edges, bid, 64, True, 100, 100, "triplet", obj_probs=probs)
    assert graphs_equal(whole, M.scene_graph_topk(obj, rel, edges, bid, 64, True, 100, 100, "triplet", obj_probs=probs))
    for s in (0, 17, 63):
        sl = slice(s * 1560, (s + 1) * 1560)
        one = M.scene_graph_topk(obj[s * 40:(s + 1) * 40], rel[sl], edges[sl] - s * 40, None, 1, True, 100, 100, "triplet",
                                 obj_probs=probs[s * 40:(s + 1) * 40])
        assert graphs_equal(whole.scene(s, s * 1560), one), s


def test_hip_contract_single_label_batch():
    _need_gpu()
    _scale_check(8, 40, 53, multi=False)


def test_hip_configs4_scene_within_its_scratch():
    """One configs[4]-sized scene: 200 objects, 39 800 edges; the scratch is what vlsat_scene_graph_scratch_bytes states, at most
    the recall entry's formula with an index beside every key: 4 (2 N min(C, 100) + E (2 R + 2 topk_each + 8)) bytes."""
    _need_gpu()
    n, e, c, r = 200, 39800, 160, 26
    for each in (1, 7, 100):
        nbytes = int(L.load().vlsat_scene_graph_scratch_bytes(n, e, c, r, 1, 100, each))
        assert 0 < nbytes <= 4 * (2 * n * min(c, 100) + e * (2 * r + 2 * each + 8)), (each, nbytes)
    assert int(L.load().vlsat_scene_graph_scratch_bytes(99840 // 39, 99840, c, r, 64, 100, 100)) <= 4 * (2 * 2560 * 100 + 99840 * 260)
    _scale_check(1, 200, 77)


@pytest.mark.parametrize("evaluate", ["triplet", "rels"])
def test_hip_ties_and_odd_graphs(evaluate):
    _need_gpu()
    for name, probs, rel, edges, bid, n_sc in tie_cases(DEV):
        scene = bid[edges[:, 0]]
        for top_k in (1, 7, 100, 1024):
            for each in (1, 3, 100):
                g = M.scene_graph_topk(probs, rel, edges, bid, n_sc, True, top_k, each, evaluate, obj_probs=probs)
                check_contract(g, probs, rel, edges, scene, n_sc, top_k, each, evaluate)
                assert graphs_equal(g, M.scene_graph_topk(probs, rel, edges, bid, n_sc, True, top_k, each, evaluate, obj_probs=probs)), name
        if n_sc == 1:
            g0 = M.scene_graph_topk(probs, rel, edges, None, 1, True, 100, 100, evaluate, obj_probs=probs)       # batch_ids = None
            assert graphs_equal(g0, M.scene_graph_topk(probs, rel, edges, bid, 1, True, 100, 100, evaluate, obj_probs=probs)), name
        else:                                                                    # the empty scene leaves its neighbours unchanged
            g = M.scene_graph_topk(probs, rel, edges, bid, 3, True, 100, 100, evaluate, obj_probs=probs)
            assert int(g.n_valid[1]) == 0 and int(g.edge[1].max()) == -1 and float(g.score[1].abs().max()) == 0.0
            a = M.scene_graph_topk(probs[:3], rel[:6], edges[:6], None, 1, True, 100, 100, evaluate, obj_probs=probs[:3])
            b = M.scene_graph_topk(probs[6:], rel[6:], edges[6:] - 6, None, 1, True, 100, 100, evaluate, obj_probs=probs[6:])
            assert graphs_equal(g.scene(0), a) and graphs_equal(g.scene(2, 6), b)
    # no edge at all
    g = M.scene_graph_topk(probs, rel[:0], edges[:0], None, 1, True, 5, 5, evaluate, obj_probs=probs)
    assert int(g.n_valid[0]) == 0 and int(g.edge.max()) == -1


@pytest.mark.parametrize("top_k", [100, 1024])
@pytest.mark.parametrize("each", [1, 3])
def test_hip_equal_scores_across_the_cap_and_the_edge_chunk(each, top_k):
    """Ties that straddle both the cap and the 1024-edge chunk of the scene kernel's gather (select_core.h select_topk_lists: the
    running base of a chunk meets the number of ties still needed).  Scores 0.25 / 0.5 / 0.75 only, 1 122 edges.  P(edge has a
    0.75) = 0.30 and P(edge has a score >= 0.5) = 0.93, so with topk_each = 1 and top_k = 1024 about 337 candidates lie above the
    boundary value 0.5 and the first 1024 edges hold fewer ties (about 645) than are still needed: the kept ties run past edge
    1024 and stop short of the last one.  Equal to the host statement field for field."""
    _need_gpu()
    probs, rel, edges = three_valued_scene(p50=0.0836, p75=0.0136)
    want = M.scene_graph_topk_host(probs, rel, edges, None, 1, True, top_k, each, "rels", obj_probs=probs)
    n_v = int(want.n_valid[0])
    cand = edge_candidates(probs, rel, edges, "rels", each)
    t = want.score[0, n_v - 1]                                               # the boundary value
    assert cand.numel() > top_k and n_v == top_k
    assert bool((cand[:1024] == t).any()) and bool((cand[1024:] == t).any())
    if (each, top_k) == (1, 1024):
        kept = want.edge[0, :n_v][want.score[0, :n_v] == t]
        assert float(t) == 0.5 and int(kept.max()) >= 1024 and int((kept >= 1024).sum()) < int((cand[1024:] == t).sum())
    got = M.scene_graph_topk(probs.to(DEV), rel.to(DEV), edges.to(DEV), None, 1, True, top_k, each, "rels", obj_probs=probs.to(DEV))
    for k in ("edge", "sub_cls", "obj_cls", "pred", "score", "n_valid"):
        assert torch.equal(getattr(got, k).cpu(), getattr(want, k)), (each, top_k, k)


def test_hip_arguments_out_of_range_are_refused_with_a_message():
    _need_gpu()
    lib = L.load()
    p, rel = torch.rand(3, 4, device=DEV), torch.rand(2, 5, device=DEV)
    ed = torch.tensor([[0, 1], [1, 2]], device=DEV)
    out = torch.zeros(4096, dtype=torch.int32, device=DEV)
    sc = torch.zeros(1024, dtype=torch.float32, device=DEV)
    scratch = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    nv = torch.zeros(4, dtype=torch.int32, device=DEV)

    def call(c=4, r=5, n_scenes=1, mode=0, top_k=10, each=10, bid=0):
        return lib.vlsat_scene_graph_topk(p.data_ptr(), rel.data_ptr(), ed.data_ptr(), bid, 3, 2, c, r, n_scenes, mode, top_k, each,
                                          scratch.data_ptr(), out.data_ptr(), sc.data_ptr(), nv.data_ptr(), L.stream_ptr())

    assert call() == 0
    for kw, word in ((dict(top_k=0), "top_k"), (dict(top_k=1025), "top_k"), (dict(each=0), "topk_each"), (dict(each=101), "topk_each"),
                     (dict(c=1025), "classes"), (dict(r=33), "classes"), (dict(mode=2), "mode"), (dict(n_scenes=2), "batch_ids")):
        assert call(**kw) != 0, kw
        assert word in lib.vlsat_last_error().decode(), (kw, lib.vlsat_last_error())
    assert int(lib.vlsat_scene_graph_scratch_bytes(3, 2, 4, 5, 1, 0, 10)) == 0
    assert int(lib.vlsat_scene_graph_scratch_bytes(3, 2, 4, 5, 1, 10, 101)) == 0
    torch.cuda.synchronize()


def _model(prec=None, multi=True):
    from vlsat_amd import VLSATConfig, synth
    from vlsat_amd.model import VLSATModel
    cfg = VLSATConfig(N_LAYERS=1, multi_rel_outputs=multi)
    m = VLSATModel(cfg, DEV).load_state(synth.make_weights(cfg)).eval()
    if prec:
        m.set_gemm_precision(prec)
    return m


def _batches(n_batches, seed):
    from vlsat_amd import synth
    g = torch.Generator().manual_seed(seed)
    out = []
    for s in range(n_batches):
        n = int(torch.randint(3, 12, (1,), generator=g))
        b = synth.collate([synth.make_scene(n, 32, 9400 + s)])
        item = {k: torch.from_numpy(v).to(DEV) for k, v in b.items() if k != "edge_indices"}
        item.update(edge_indices=torch.from_numpy(b["edge_indices"]).t().contiguous().to(DEV), fc_sizes=[n], n_scenes=1)
        out.append(item)
    return out


def _separate(m, b, multi, **kw):
    o3, o2, r3, r2 = m(b["obj_points"], b["obj_2d_feats"], b["edge_indices"].t().contiguous(), b["descriptor"], b.get("batch_ids"),
                       fc_sizes=b.get("fc_sizes"))
    bid = None if b.get("batch_ids") is None else b["batch_ids"].view(-1)
    ns = int(b.get("n_scenes", 1))
    return tuple(M.scene_graph_topk(o, r, b["edge_indices"], bid if ns > 1 else None, ns, multi, obj_probs=M.softmax_rows(o), **kw)
                 for o, r in ((o3, r3), (o2, r2)))


@pytest.mark.parametrize("prec,multi", [(None, True), ("bf16_mixed", True), (None, False)])
def test_predict_graph_equals_the_separate_calls(prec, multi):
    """vlsat_forward_scene_graph == forward + softmax_rows + scene_graph_topk bit for bit: one-scene plans (paired schedule) and a
    merged batch, both modes."""
    _need_gpu()
    m = _model(prec, multi)
    bs = _batches(5, 41)
    merged = EV.merge_batches([dict(b, gt_class=b["descriptor"][:, 0], gt_rel_cls=b["edge_indices"][:, 0]) for b in bs])
    for b in bs + [merged]:
        for kw in (dict(top_k=100, topk_each=100, evaluate="triplet"), dict(top_k=20, topk_each=1, evaluate="triplet"),
                   dict(top_k=50, topk_each=100, evaluate="rels")):
            got = m.predict_graph(b["obj_points"], b["obj_2d_feats"], b["edge_indices"].t(), b["descriptor"], b.get("batch_ids"),
                                  fc_sizes=b.get("fc_sizes"), **kw)
            want = _separate(m, b, multi, **kw)
            assert graphs_equal(got[0], want[0]) and graphs_equal(got[1], want[1]), (prec, multi, kw)
            assert int(got[0].n_valid.min()) > 0
    with pytest.raises(L.VlsatError, match="top_k"):
        b = bs[0]
        m.predict_graph(b["obj_points"], b["obj_2d_feats"], b["edge_indices"].t(), b["descriptor"], top_k=2000)
    m.close()


def test_evaluate_predict_pipelined_equals_serial_and_exports(tmp_path):
    _need_gpu()
    from vlsat_amd import scene_graph as SG
    m = _model()
    bs = _batches(9, 43)
    serial = list(EV.predict(m, bs, top_k=30, topk_each=5))
    piped = list(EV.predict(m, bs, device=DEV, workers=2, top_k=30, topk_each=5))
    assert len(serial) == len(piped) == 9
    for (a3, a2), (b3, b2) in zip(serial, piped):
        assert graphs_equal(a3, b3) and graphs_equal(a2, b2)
    merged = EV.merge_batches([dict(b, gt_class=b["descriptor"][:, 0], gt_rel_cls=b["edge_indices"][:, 0]) for b in bs[:3]])
    per_scene = list(EV.predict(m, [merged], top_k=30, topk_each=5))
    assert len(per_scene) == 3 and all(int(g3.n_valid[0]) == 30 and int(g3.edge.min()) >= 0 for g3, _ in per_scene)
    names_c, names_r = [f"c{i}" for i in range(160)], [f"r{i}" for i in range(26)]
    recs = SG.to_records(serial[0][0], 0, bs[0]["edge_indices"], list(range(100, 100 + bs[0]["obj_points"].shape[0])), names_c, names_r)
    assert len(recs) == 30 and recs[0]["score"] >= recs[-1]["score"] and recs[0]["subject"] >= 100
    SG.write_json(tmp_path / "g.json", {"scan-0": recs})
    assert SG.read_json(tmp_path / "g.json")["scan-0"] == recs
    m.close()
