"""The decoded scene graph on the GPU (csrc/graph_decode.hip via vlsat_graph_decode / vlsat_graph_decode_counts /
vlsat_forward_graph): every field equal, bit for bit, to the host restatement fed the same probabilities -- the fixtures' cases,
a collated batch with an empty scene, ties at the cap, a threshold vector, the triplet score, a scene of 104 832 candidates,
the counts, the fused call with and without the 2D branch, evaluate.decode, and the plan's arena."""
import ctypes as C

import numpy as np
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import evaluate as EV, lib as L, metrics as M

from graph_decode_checks import SG_GOLD, assert_equal, brute, case, indicator
from scene_graph_checks import three_valued_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path cannot run and there is no fallback")


def _both(probs, rp, edges, bid, n_scenes, multi, thr, score, n_labels, max_rel):
    """(device graph, host graph) from the same probabilities; logits are not read when both probability tensors are given."""
    d = lambda t: None if t is None else t.to(DEV)
    thr_d = thr.to(DEV) if torch.is_tensor(thr) else thr
    got = M.decode_graph(d(probs), d(rp), d(edges), d(bid), n_scenes, multi, thr_d, score, n_labels, max_rel, obj_probs=d(probs),
                         rel_probs=d(rp))
    want = M.decode_graph_host(probs, rp, edges, bid, n_scenes, multi, thr, score, n_labels, max_rel, obj_probs=probs, rel_probs=rp)
    return got, want


@pytest.mark.parametrize("br", ["3d", "2d"])
@pytest.mark.parametrize("i", range(7))
def test_hip_equals_host_on_the_golden_cases(i, br):
    _need_gpu()
    z = np.load(SG_GOLD)
    obj, rel, edges, probs, multi, rp = case(z, i, br)
    for score in ("rel", "triplet"):
        for n_labels, max_rel in ((3, 4096), (8, 1024), (1, 100)):
            got, want = _both(probs, rp, edges, None, 1, multi, 0.5, score, n_labels, max_rel)
            assert_equal(got, want, (i, br, score, n_labels, max_rel))
    if br == "3d" and i in (1, 2):                       # more than one block of threads; the cap bites at 4 096
        assert int(want.n_total[0]) == {1: 1732, 2: 7976}[i]
    # the device softmax / exp in front of the decode: the same decisions on these cases (no probability within 1e-5 of 0.5)
    got = M.decode_graph(obj.to(DEV), rel.to(DEV), edges.to(DEV), None, 1, multi, 0.5, "rel", 3, 4096)
    want = M.decode_graph_host(obj, rel, edges, None, 1, multi, 0.5, "rel", 3, 4096, probs, rp)
    assert int(got.n_total[0]) == int(want.n_total[0]) and torch.equal(got.labels[:, 0].cpu(), want.labels[:, 0])
    if int(want.n_total[0]) <= 4096:
        assert torch.equal(indicator(got, 0, *rel.shape), indicator(want, 0, *rel.shape))


def test_hip_collated_batch_with_an_empty_scene():
    _need_gpu()
    z = np.load(SG_GOLD)
    g = torch.Generator().manual_seed(2)
    parts = [case(z, 0, "3d"), None, case(z, 3, "3d"), case(z, 6, "3d")]
    probs, rps, eds, bid, node0, edge0, off = [], [], [], [], [], [], 0
    for s, c in enumerate(parts):
        p = torch.softmax(torch.randn(1, 160, generator=g), -1) if c is None else c[3]
        node0.append(off)
        edge0.append(sum(x.shape[0] for x in eds))
        if c is not None:
            eds.append(c[2] + off)
            rps.append(c[5])
        probs.append(p)
        bid += [s] * p.shape[0]
        off += p.shape[0]
    node0.append(off)
    probs, rp, edges, bid = torch.cat(probs), torch.cat(rps), torch.cat(eds), torch.tensor(bid)
    for score in ("rel", "triplet"):
        for max_rel in (4096, 50):
            got, want = _both(probs, rp, edges, bid, 4, True, 0.5, score, 3, max_rel)
            assert_equal(got, want, (score, max_rel))
            assert int(got.n_total[1]) == 0 and int(got.edge[1].max()) == -1 and float(got.score[1].abs().max()) == 0.0
            for s, c in enumerate(parts):
                if c is None:
                    continue
                one, _ = _both(c[3], c[5], c[2], None, 1, True, 0.5, score, 3, max_rel)
                assert_equal(got.scene(s, edge0[s], (node0[s], node0[s + 1])), one, (score, max_rel, s))


def _eighths(seed, n=9, e=70, r=26, c=12):
    g = torch.Generator().manual_seed(seed)
    edges = torch.tensor([(a, b) for a in range(n) for b in range(n) if a != b][:e])
    rp = torch.randint(0, 9, (e, r), generator=g).float() / 8
    probs = torch.randint(0, 9, (n, c), generator=g).float() / 8
    return probs, rp, edges


@pytest.mark.parametrize("multi", [True, False])
def test_hip_ties_at_the_cap_follow_the_total_order(multi):
    _need_gpu()
    probs, rp, edges = _eighths(7)
    for score in ("rel", "triplet"):
        full = M.decode_graph_host(probs, rp, edges, None, 1, multi, 0.5, score, 2, 4096, obj_probs=probs, rel_probs=rp)
        sc, n = full.score[0], int(full.n_total[0])
        cuts = [k for k in range(2, n - 1) if sc[k - 1] == sc[k] and sc[k - 2] == sc[k + 1]]      # inside a run of equal scores
        assert len(cuts) > 4
        for max_rel in (cuts[0], cuts[len(cuts) // 2], cuts[-1]):
            got, want = _both(probs, rp, edges, None, 1, multi, 0.5, score, 2, max_rel)
            assert_equal(got, want, (multi, score, max_rel))
            assert_equal(got, brute(probs, rp, edges, np.zeros(70, np.int64), 1, 0.5, multi, score, 2, max_rel))
            n_v = int(got.n_valid[0])
            assert n_v == max_rel and torch.equal(got.edge[0, :n_v].cpu(), full.edge[0, :n_v])


@pytest.mark.parametrize("max_rel", [1024, 4096])
def test_hip_equal_scores_across_the_cap_and_the_edge_chunk(max_rel):
    """Ties that straddle both the cap and the 1024-edge chunk of the scene kernel's gather (select_core.h select_topk_lists).
    Multi-label at threshold 0.5 on scores 0.25 / 0.5 / 0.75, 1 122 edges, about 0.95 asserted pairs per edge: n_total is a
    little above 1024 while the first 1024 edges assert fewer than 1024 pairs, so at max_rel = 1024 the kept pairs equal to the
    boundary value 0.5 run past edge 1024 and stop short of the last one; at 4096 nothing is cut (no bisection) and the pairs
    of the second chunk land behind the first chunk's.  Equal to the host statement field for field."""
    _need_gpu()
    probs, rp, edges = three_valued_scene(p50=0.0245, p75=0.012)
    got, want = _both(probs, rp, edges, None, 1, True, 0.5, "rel", 3, max_rel)
    n_t, n_v = int(want.n_total[0]), int(want.n_valid[0])
    assert n_t > 1024 and n_v == min(n_t, max_rel)
    t = want.score[0, n_v - 1]                                               # the boundary value
    assert bool((rp[:1024] == t).any()) and bool((rp[1024:] == t).any())
    if max_rel == 1024:
        kept = want.edge[0, :n_v][want.score[0, :n_v] == t]
        assert float(t) == 0.5 and int(kept.max()) >= 1024 and int((kept >= 1024).sum()) < int((rp[1024:] == t).sum())
    assert_equal(got, want, max_rel)


def test_hip_threshold_vector():
    _need_gpu()
    probs, rp, edges = _eighths(9)
    thr = torch.full((26,), 0.5)
    thr[1], thr[2], thr[3], thr[6] = 1.5, -1.0, 0.25, 0.0
    for multi in (True, False):
        got, want = _both(probs, rp, edges, None, 1, multi, thr, "rel", 3, 4096)
        assert_equal(got, want, multi)
        assert_equal(got, brute(probs, rp, edges, np.zeros(70, np.int64), 1, thr.numpy(), multi, "rel", 3, 4096))
    hot = indicator(got := _both(probs, rp, edges, None, 1, True, thr, "rel", 3, 4096)[0], 0, 70, 26)
    assert not hot[:, 1].any() and hot[:, 2].all() and hot[:, 6].all()                  # > 1 never, <= 0 always
    assert torch.equal(hot[:, 3], rp[:, 3] >= 0.25) and int((rp[:, 3] == 0.25).sum()) > 0      # equality passes
    assert int(got.n_total[0]) == int(hot.sum())


def test_hip_triplet_score_is_two_fp32_roundings():
    _need_gpu()
    g = torch.Generator().manual_seed(21)
    n = 12
    edges = torch.tensor([(a, b) for a in range(n) for b in range(n) if a != b])
    probs = torch.softmax(torch.randn(n, 160, generator=g) * 3, -1)
    rp = torch.sigmoid(torch.randn(edges.shape[0], 26, generator=g) * 2)
    got, want = _both(probs, rp, edges, None, 1, True, 0.5, "triplet", 1, 4096)
    assert_equal(got, want)
    nv = int(got.n_valid[0])
    ed, pr = got.edge[0, :nv].long().cpu(), got.pred[0, :nv].long().cpu()
    top = probs.max(1).values.numpy()
    s, o, r = top[edges[ed, 0]], top[edges[ed, 1]], rp.numpy()[ed, pr]
    two = ((s * o).astype(np.float32) * r).astype(np.float32)
    np.testing.assert_array_equal(got.score[0, :nv].cpu().numpy().view(np.uint32), two.view(np.uint32))
    fused = (s.astype(np.float64) * o * r).astype(np.float32)                       # one rounding: differs somewhere
    assert (fused.view(np.uint32) != two.view(np.uint32)).any()


def test_hip_one_larger_scene():
    """N = 64 fully connected: E = 4 032, 104 832 candidates -- every loop of the scene block runs more than once."""
    _need_gpu()
    g = torch.Generator().manual_seed(33)
    n = 64
    edges = torch.tensor([(a, b) for a in range(n) for b in range(n) if a != b])
    probs = torch.softmax(torch.randn(n, 160, generator=g) * 4, -1)
    rp = torch.sigmoid(torch.randn(edges.shape[0], 26, generator=g) * 2)
    rp[::5] = (rp[::5] * 16).round() / 16                                           # ties across edges
    for score, max_rel in (("rel", 4096), ("triplet", 1000), ("rel", 1)):
        got, want = _both(probs, rp, edges, None, 1, True, 0.5, score, 8, max_rel)
        assert_equal(got, want, (score, max_rel))
    assert int(want.n_total[0]) > 40000
    got, want = _both(probs, rp, edges, None, 1, False, 0.3, "triplet", 3, 4096)
    assert_equal(got, want, "single label")
    assert 1024 < int(want.n_total[0]) < 4032


def test_hip_counts_equal_host_and_add_over_scenes():
    _need_gpu()
    g = torch.Generator().manual_seed(5)
    n_sc, n_obj = 5, 9
    n = n_sc * n_obj
    edges = torch.tensor([(s * n_obj + a, s * n_obj + b) for s in range(n_sc) for a in range(n_obj) for b in range(n_obj) if a != b])
    e = edges.shape[0]
    obj = torch.randn(n, 160, generator=g) * 3
    gt_cls = torch.where(torch.rand(n, generator=g) < 0.5, obj.argmax(1), torch.randint(0, 160, (n,), generator=g))
    for multi in (True, False):
        zz = torch.randn(e, 26, generator=g) * 2
        rel = torch.sigmoid(zz) if multi else torch.log_softmax(zz, -1)
        gt_rel = (torch.rand(e, 26, generator=g) < 0.1).long() if multi else torch.randint(0, 26, (e,), generator=g)
        probs = M.softmax_rows(obj.to(DEV))
        rp = rel.to(DEV) if multi else M.exp_probs(rel.to(DEV))
        thr = torch.rand(26, generator=g) * 0.6
        got = M.decode_counts(obj.to(DEV), rel.to(DEV), gt_cls.to(DEV), gt_rel.to(DEV), multi, thr, obj_probs=probs, rel_probs=rp)
        want = M.decode_counts_host(obj, rel, gt_cls, gt_rel, multi, thr, obj_probs=probs.cpu(), rel_probs=rp.cpu())
        assert got.dtype == torch.int64 and got.cpu().tolist() == want.tolist()
        assert int(want[:78:3].sum()) > 0 and int(want[1:78:3].sum()) > 0 and int(want[2:78:3].sum()) > 0 and 0 < int(want[79]) < n
        acc = torch.zeros(80, dtype=torch.int64, device=DEV)
        per = e // n_sc
        for s in range(n_sc):
            ns, es = slice(s * n_obj, (s + 1) * n_obj), slice(s * per, (s + 1) * per)
            M.decode_counts(obj[ns].to(DEV), rel[es].to(DEV), gt_cls[ns].to(DEV), gt_rel[es].to(DEV), multi, thr, obj_probs=probs[ns],
                            rel_probs=rp[es], counts=acc)
        assert acc.cpu().tolist() == want.tolist()
        if not multi:
            assert want[:3].tolist() == [0, 0, 0]


def _model(multi=True):
    from vlsat_amd import VLSATConfig, synth
    from vlsat_amd.model import VLSATModel
    cfg = VLSATConfig(N_LAYERS=1, multi_rel_outputs=multi)
    return VLSATModel(cfg, DEV).load_state(synth.make_weights(cfg)).eval()


def _scene(n_obj, seed):
    from vlsat_amd import synth
    b = synth.collate([synth.make_scene(n_obj, 32, seed)])
    item = {k: torch.from_numpy(v).to(DEV) for k, v in b.items() if k != "edge_indices"}
    item.update(edge_indices=torch.from_numpy(b["edge_indices"]).t().contiguous().to(DEV), fc_sizes=[n_obj], n_scenes=1)
    return item


def _merged(bs):
    return EV.merge_batches([dict(b, gt_class=b["descriptor"][:, 0], gt_rel_cls=b["edge_indices"][:, 0]) for b in bs])


def _separate(m, b, multi, use_2d=True, **kw):
    ei_t = b["edge_indices"].t().contiguous()
    if use_2d:
        o3, o2, r3, r2 = m(b["obj_points"], b["obj_2d_feats"], ei_t, b["descriptor"], b.get("batch_ids"), fc_sizes=b.get("fc_sizes"))
        pairs = ((o3, r3), (o2, r2))
    else:
        pairs = (m.forward_3d(b["obj_points"], ei_t, b["descriptor"], b.get("batch_ids"), fc_sizes=b.get("fc_sizes")),)
    ns = int(b.get("n_scenes", 1))
    bid = b["batch_ids"].view(-1) if ns > 1 else None
    return tuple(M.decode_graph(o, r, b["edge_indices"], bid, ns, multi, obj_probs=M.softmax_rows(o), **kw) for o, r in pairs)


KW = (dict(score="rel", n_labels=3, max_rel=1024), dict(score="triplet", n_labels=8, max_rel=40))


def _median_threshold(m, b, multi):
    """A threshold about half of the decisions pass, from the model's own outputs (synthetic weights: nothing is calibrated)."""
    r3 = m.forward_3d(b["obj_points"], b["edge_indices"].t().contiguous(), b["descriptor"], b.get("batch_ids"), fc_sizes=b.get("fc_sizes"))[1]
    return float(r3.median()) if multi else float(M.exp_probs(r3).max(1).values.median())


@pytest.mark.parametrize("multi", [True, False])
def test_fused_call_equals_forward_plus_decode(multi):
    """vlsat_forward_graph == forward + softmax_rows + decode_graph field for field on a 3-scene batch (8 objects x 32 points), the
    3D-only call == its 3D half == forward_3d + decode_graph, and the plan's arena does not grow."""
    _need_gpu()
    m = _model(multi)
    b = _merged([_scene(8, 9500 + s) for s in range(3)])
    ei_t = b["edge_indices"].t()
    info0 = m.plan_info(ei_t, b["batch_ids"], b["obj_points"].shape[0], 32)
    thr0 = _median_threshold(m, b, multi)
    for kw in KW:
        kw = dict(kw, threshold=thr0)
        g3, g2 = m.decode_graph(b["obj_points"], b["obj_2d_feats"], ei_t, b["descriptor"], b["batch_ids"], fc_sizes=b["fc_sizes"], **kw)
        w3, w2 = _separate(m, b, multi, **kw)
        assert_equal(g3, w3, ("3d", kw))
        assert_equal(g2, w2, ("2d", kw))
        assert int(g3.n_total.sum()) > 0 and g3.n_valid.numel() == 3
        only3, none = m.decode_graph(b["obj_points"], None, ei_t, b["descriptor"], b["batch_ids"], fc_sizes=b["fc_sizes"], **kw)
        assert none is None
        assert_equal(only3, g3, ("3d-only", kw))
        assert_equal(only3, _separate(m, b, multi, use_2d=False, **kw)[0], ("forward_3d", kw))
    info1 = m.plan_info(ei_t, b["batch_ids"], b["obj_points"].shape[0], 32)
    assert info0 == info1 and info0["n_scenes"] == 3
    with pytest.raises(L.VlsatError, match="max_rel"):
        m.decode_graph(b["obj_points"], None, ei_t, b["descriptor"], b["batch_ids"], max_rel=5000)
    # the C entry: 2D features and 2D outputs go together; the top-K sibling still refuses a NULL 2D input
    lib, plan = L.load(), m._plan(ei_t, b["batch_ids"], b["obj_points"].shape[0], 32, b["fc_sizes"])
    thr = torch.full((26,), 0.5, device=DEV)
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=DEV)
    f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=DEV)
    n, e2 = b["obj_points"].shape[0], b["edge_indices"].contiguous()
    outs = [i32(n, 3), f32(n, 3), i32(3, 16, 2), f32(3, 16), i32(3), i32(3)]
    ptrs = [t.data_ptr() for t in outs]
    head = (m._h, plan.handle, b["obj_points"].data_ptr())
    mid = (b["descriptor"].data_ptr(), e2.data_ptr(), 3, int(multi), 0, 3, 16, thr.data_ptr())
    assert lib.vlsat_forward_graph(*head, b["obj_2d_feats"].data_ptr(), *mid, *ptrs, *([None] * 6), L.stream_ptr()) != 0
    assert "2D" in lib.vlsat_last_error().decode()
    assert lib.vlsat_forward_graph(*head, None, *mid, *ptrs, *ptrs[:1], *([None] * 5), L.stream_ptr()) != 0
    assert lib.vlsat_forward_graph(*head, None, *mid, *ptrs, *([None] * 6), L.stream_ptr()) == 0
    assert lib.vlsat_forward_scene_graph(*head, None, b["descriptor"].data_ptr(), e2.data_ptr(), 3, 1, 16, 5, *([ptrs[0]] * 6),
                                         L.stream_ptr()) != 0
    torch.cuda.synchronize()
    m.close()


def test_evaluate_decode_pipelined_equals_per_scene_calls():
    _need_gpu()
    m = _model()
    g = torch.Generator().manual_seed(47)
    bs = [_scene(int(torch.randint(3, 12, (1,), generator=g)), 9600 + s) for s in range(7)]
    kw = dict(threshold=_median_threshold(m, bs[0], True), score="triplet", n_labels=2, max_rel=64)
    want = [m.decode_graph(b["obj_points"], b["obj_2d_feats"], b["edge_indices"].t(), b["descriptor"], fc_sizes=b["fc_sizes"], **kw)
            for b in bs]
    piped = list(EV.decode(m, bs, device=DEV, workers=2, **kw))
    serial = list(EV.decode(m, bs, **kw))
    assert len(piped) == len(serial) == 7
    for (a3, a2), (b3, b2), (c3, c2) in zip(want, piped, serial):
        assert_equal(b3, a3), assert_equal(b2, a2), assert_equal(c3, a3), assert_equal(c2, a2)
    only3 = list(EV.decode(m, bs, device=DEV, workers=2, use_2d=False, **kw))
    for (a3, _), (b3, b2) in zip(want, only3):
        assert b2 is None
        assert_equal(b3, a3)
    # a merged batch comes back one scene at a time, with the scene's own node rows and edge rows
    per_scene = list(EV.decode(m, [_merged(bs[:3])], **kw))
    assert len(per_scene) == 3
    for (g3, g2), b in zip(per_scene, bs[:3]):
        n, e = b["obj_points"].shape[0], b["edge_indices"].shape[0]
        assert g3.labels.shape == (n, 2) and g2.labels.shape == (n, 2)
        rows = g3.edge[0, :int(g3.n_valid[0])]
        assert rows.numel() == 0 or (0 <= int(rows.min()) and int(rows.max()) < e)
    assert sum(int(g3.n_valid[0]) for g3, _ in per_scene) > 0
    m.close()


def test_hip_arguments_out_of_range_are_refused_with_a_message():
    _need_gpu()
    lib = L.load()
    p, rel = torch.rand(3, 9, device=DEV), torch.rand(2, 5, device=DEV)
    ed = torch.tensor([[0, 1], [1, 2]], device=DEV)
    thr = torch.full((5,), 0.5, device=DEV)
    lab, lp = torch.zeros(3 * 8, dtype=torch.int32, device=DEV), torch.zeros(3 * 8, device=DEV)
    out, sc = torch.zeros(2 * 4096, dtype=torch.int32, device=DEV), torch.zeros(4096, device=DEV)
    scratch = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    nv, nt = torch.zeros(4, dtype=torch.int32, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)

    def call(c=9, r=5, n_scenes=1, multi=1, mode=0, n_labels=3, max_rel=10, bid=0):
        return lib.vlsat_graph_decode(p.data_ptr(), rel.data_ptr(), ed.data_ptr(), bid, thr.data_ptr(), 3, 2, c, r, n_scenes, multi, mode,
                                      n_labels, max_rel, scratch.data_ptr(), lab.data_ptr(), lp.data_ptr(), out.data_ptr(),
                                      sc.data_ptr(), nv.data_ptr(), nt.data_ptr(), L.stream_ptr())

    assert call() == 0
    for kw, word in ((dict(n_labels=0), "n_labels"), (dict(n_labels=9), "n_labels"), (dict(max_rel=0), "max_rel"),
                     (dict(max_rel=4097), "max_rel"), (dict(c=1025), "classes"), (dict(r=33), "classes"), (dict(mode=2), "score_mode"),
                     (dict(multi=2), "multi_label"), (dict(n_scenes=2), "batch_ids")):
        assert call(**kw) != 0, kw
        assert word in lib.vlsat_last_error().decode(), (kw, lib.vlsat_last_error())
    assert int(lib.vlsat_graph_decode_scratch_bytes(2, 9, 5, 1, 3, 0)) == 0
    assert int(lib.vlsat_graph_decode_scratch_bytes(2, 9, 5, 1, 9, 10)) == 0
    assert 0 < int(lib.vlsat_graph_decode_scratch_bytes(99840, 160, 26, 64, 3, 1024)) <= 99840 * (5 * 26 + 4) + 4 * 256 + 65 * 4
    torch.cuda.synchronize()
