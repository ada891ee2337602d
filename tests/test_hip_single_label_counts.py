"""The one-call evaluation step (vlsat_process_val_counts[_split], VLSATModel.process_val_counts) for a SINGLE-LABEL model
(MODEL.multi_rel_outputs = false: log_softmax head, class 0 = 'none', an [E] label vector), and the pipelined validation loop on it.

The triplet-rank kernel of the one call takes exp of each log-probability on load; the separate calls rank an exp'd copy of the
tensor in a second pass.  Both form the same fp32 products on the same forward outputs, so every comparison here is EXACT: int64
vectors entry for entry, summary dicts key for key.

The batch: four fully connected scenes of 1, 3, 5 and 6 objects (0, 6, 20 and 30 edges: one scene without any edge), P = 16 points.
Objects 1 and 4 of the 6-object scene are one object twice -- the same points and descriptor, and the same 2D feature so that the
3D outputs, which attend to the 2D branch, are equal too: equal class probabilities and equal triplet scores occur.  Half of the edges
are labelled 'none' (0); the others carry every predicate 1 .. R-1 in turn (26 predicates on 28 edges, or 8 on 28).
Two class geometries: (C, R) = (160, 27), the reference's, and (20, 9) -- C below the triplet top-k of 101 (the sorted rows are the
whole rows), R far below the 32 lanes of an edge.

The loop test compares the host loop (one-scene forwards) with a merged loop (four scenes per forward): a merged forward differs from
a one-scene forward in the last bits, so it needs scenes without near-ties at the counted thresholds, other than the planted exact
duplicate.  The seeds below were checked on the CPU oracle for both geometries: the counts vector of the oracle's outputs does not move
under twenty independent relative perturbations of 1e-5 of every logit and log-probability (a hundred times a forward's last-bit
differences).  No seed had to be passed over; the first one tried (SEED = 4100) held."""
import numpy as np
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import VLSATConfig, evaluate as EV, lib as L, metrics as M, synth
from vlsat_amd.model import VLSATModel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = 16
SIZES = [1, 3, 5, 6]
SEED = 4100
GEOMETRIES = [(160, 27), (20, 9)]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path cannot run and there is no fallback")


def _is_2d(name: str) -> bool:
    return name.endswith("_2d")


def make_scene(n, seed):
    """a synth scene; with six objects, object 4 is object 1 again"""
    sc = synth.make_scene(n, P, seed)
    if n == 6:
        for k in ("obj_points", "descriptor", "obj_2d_feats"):
            sc[k][4] = sc[k][1]
    return sc


def make_labels(sizes, seed, n_obj, n_rel):
    """(gt_class [N], labels [E]): half of the edges 'none', the others every predicate 1 .. n_rel-1 in turn, at random places; the
    duplicated objects of a 6-object scene carry different classes (the mirrored triple of their edge ties with the gt triple)"""
    g = torch.Generator().manual_seed(seed)
    n, e = sum(sizes), sum(k * (k - 1) for k in sizes)
    gt_cls = torch.randint(0, n_obj, (n,), generator=g)
    off = 0
    for k in sizes:
        if k == 6:
            gt_cls[off + 4] = (gt_cls[off + 1] + 1) % n_obj
        off += k
    labels = torch.zeros(e, dtype=torch.int64)
    on = torch.randperm(e, generator=g)[:e // 2]
    labels[on] = torch.arange(len(on)) % (n_rel - 1) + 1
    return gt_cls, labels


def make_item(sizes, seed, n_obj, n_rel, device=DEV):
    b = synth.collate([make_scene(k, seed + 10 * i) for i, k in enumerate(sizes)])
    gt_cls, labels = make_labels(sizes, seed, n_obj, n_rel)
    item = {k: torch.from_numpy(v).to(device) for k, v in b.items() if k != "edge_indices"}
    item.update(gt_class=gt_cls.to(device), gt_rel_cls=labels.to(device), fc_sizes=list(sizes), n_scenes=len(sizes),
                edge_indices=torch.from_numpy(b["edge_indices"]).t().contiguous().to(device))
    return item


def loop_items(n_obj, n_rel, device=DEV):
    """eight one-scene batches of the four shapes"""
    return [make_item([k], SEED + 100 * (i + 1), n_obj, n_rel, device) for i, k in enumerate(SIZES + SIZES)]


class Case:
    """one geometry: the model, the merged batch and -- computed once, left unchanged -- the separate-call reference on the same plan"""

    def __init__(self, n_obj, n_rel, multi=False):
        self.C, self.R, self.multi = n_obj, n_rel, multi
        cfg = VLSATConfig(N_LAYERS=1, multi_rel_outputs=multi, num_rel_class=n_rel, num_obj_class=n_obj)
        self.model = VLSATModel(cfg, DEV).load_state(synth.make_weights(cfg)).eval()
        b = self.b = make_item(SIZES, SEED, n_obj, n_rel)
        if multi:                                   # the labels as a multi-hot target; every fifth labelled edge carries a second predicate
            hot = M.multihot_targets(b["gt_rel_cls"], n_rel).clone()
            rows = torch.nonzero(b["gt_rel_cls"] > 0).view(-1)[::5]
            hot[rows, (b["gt_rel_cls"][rows] % (n_rel - 1)) + 1] = 1
            b["gt_rel_cls"] = hot
        self.F = EV.fields(n_rel)
        self.hot = M.multihot_targets(b["gt_rel_cls"], n_rel).to(torch.int64).contiguous()
        self.edges = b["edge_indices"]
        ei_t = self.edges.t()
        self.outs = self.model(b["obj_points"], b["obj_2d_feats"], ei_t, b["descriptor"], b["batch_ids"], istrain=False, fc_sizes=b["fc_sizes"])
        obj3, obj2, rel3, rel2 = self.outs
        self.t3 = M.rank_tables(obj3, rel3, b["gt_class"], self.hot, self.edges, multi)
        self.t2 = M.rank_tables(obj2, rel2, b["gt_class"], self.hot, self.edges, multi)
        self.want = M.eval_counts(self.zeros(), self.t3, self.t2, b["gt_class"], self.hot, self.edges, len(SIZES))
        torch.cuda.synchronize()

    def zeros(self):
        return torch.zeros(len(self.F), dtype=torch.int64, device=DEV)

    def one_call(self, counts, use_2d=True, **split):
        """VLSATModel.process_val_counts; a single-label model is named as one (without ``single_label=True`` the method keeps its
        earlier refusal: tests/test_hip_eval_3d_only.py)"""
        b = self.b
        if not self.multi:
            split["single_label"] = True
        return self.model.process_val_counts(counts, b["obj_points"], b["obj_2d_feats"] if use_2d else None, b["gt_class"], b["descriptor"], self.hot,
                                             self.edges, b["batch_ids"], len(SIZES), b["fc_sizes"], **split)

    def close(self):
        self.model.close()


@pytest.fixture(scope="module", params=GEOMETRIES, ids=lambda g: f"C{g[0]}-R{g[1]}")
def case(request):
    _need_gpu()
    c = Case(*request.param)
    yield c
    c.close()


def _assert_vector(names, got, want, what, in_2d=None):
    got, want = got.cpu().tolist(), want.cpu().tolist()
    assert len(names) == len(got) == len(want), what
    bad = [(f, a, b) for f, a, b in zip(names, got, want) if a != (in_2d if in_2d is not None and _is_2d(f) else b)]
    assert not bad, (what, bad[:8])


# ---- 1. the call is taken (the parent raises here: it knows no single_label, and its library refuses the model) --------------------
def test_one_call_is_taken_for_a_single_label_model(case):
    counts = case.zeros()
    assert case.one_call(counts) is True
    b = case.b                                                            # unnamed, the model is answered as before: nothing enqueued
    with pytest.raises(L.VlsatError, match="multi_rel_outputs"):
        case.model.process_val_counts(case.zeros(), b["obj_points"], b["obj_2d_feats"], b["gt_class"], b["descriptor"], case.hot, case.edges,
                                      b["batch_ids"], len(SIZES), b["fc_sizes"])
    torch.cuda.synchronize()
    F = case.F
    assert int(counts[0]) == 4 and int(counts[F.index("obj_n_3d")]) == 15 and int(counts[F.index("rel_n_2d")]) == 56
    labels = case.b["gt_rel_cls"].cpu()
    assert int((labels == 0).sum()) == 28 and set(labels[labels > 0].tolist()) == set(range(1, case.R))       # the batch is what the docstring says
    assert torch.equal(case.b["obj_points"][10], case.b["obj_points"][13])


# ---- 2. exact equality with the separate calls -------------------------------------------------------------------------------------
def test_one_call_counts_equal_the_separate_calls(case):
    got = case.zeros()
    assert case.one_call(got) is True
    torch.cuda.synchronize()
    assert got.dtype == case.want.dtype == torch.int64
    _assert_vector(case.F, got, case.want, ("two branches", case.C, case.R))
    # the planted duplicate: equal probabilities did occur
    p = M.softmax_rows(case.outs[0])
    assert torch.equal(p[10], p[13])
    # 3D-only, into a vector pre-filled with a sentinel in its 2D block
    start = torch.tensor([7 if _is_2d(f) else 0 for f in case.F], dtype=torch.int64, device=DEV)
    only = start.clone()
    assert case.one_call(only, use_2d=False) is True
    b = case.b
    obj3, rel3 = case.model.forward_3d(b["obj_points"], case.edges.t(), b["descriptor"], b["batch_ids"], fc_sizes=b["fc_sizes"])
    sep = M.eval_counts(case.zeros(), M.rank_tables(obj3, rel3, b["gt_class"], case.hot, case.edges, False), None, b["gt_class"], case.hot, case.edges,
                        len(SIZES))
    torch.cuda.synchronize()
    _assert_vector(case.F, only, sep + start, ("3D only against the separate 3D-only calls", case.C, case.R))
    _assert_vector(case.F, only, case.want, ("3D only, sentinel", case.C, case.R), in_2d=7)


# ---- 3. against the oracle ---------------------------------------------------------------------------------------------------------
def test_one_call_counts_equal_the_oracle_on_the_forward_outputs(case):
    from oracle import metrics_oracle as MO
    got = case.zeros()
    assert case.one_call(got) is True
    torch.cuda.synchronize()
    gt_cls, hot, edges = case.b["gt_class"].cpu(), case.hot.cpu(), case.edges.cpu()
    ranks = {}
    obj3 = None
    for sfx, logits, logp in (("", case.outs[0], case.outs[2]), ("_2d", case.outs[1], case.outs[3])):
        probs = M.softmax_rows(logits).cpu()
        logits, logp = logits.cpu(), logp.cpu()
        o = MO.topk_object(logits, gt_cls, M.TOPK_OBJ)
        obj3 = o if obj3 is None else obj3                                   # obj_topk of the cls_matrix: the 3D ranks for both branches
        ranks["top_k_obj" + sfx] = o
        ranks["top_k_rel" + sfx] = MO.topk_predicate(logp, hot, M.TOPK_REL)                  # the raw log-probabilities
        ranks["top_k_triplet" + sfx], cm = MO.triplet_topk(logits, logp.exp(), gt_cls, hot, edges, M.TOPK_TRIPLET, obj3, obj_probs=probs)    # their exp
    vec = EV.accumulate(np.zeros(len(case.F)), ranks, cm, len(SIZES), n_rel=case.R)
    assert (logp <= 0).all() and float(logp.exp().sum(1).sub(1).abs().max()) < 1e-4             # log-probabilities indeed
    bad = [(f, a, b) for f, a, b in zip(case.F, got.cpu().tolist(), vec.tolist()) if a != b]
    assert not bad, bad[:8]
    assert vec[case.F.index("tri_n_3d")] == 56 and vec[case.F.index("tri_hit@100_3d")] > 0


# ---- 4. the zero-shot split --------------------------------------------------------------------------------------------------------
def test_zero_shot_split_of_the_one_call(case):
    b, C, R = case.b, case.C, case.R
    labels, gt_cls, edges = b["gt_rel_cls"].cpu(), b["gt_class"].cpu(), case.edges.cpu()
    rows = torch.nonzero(labels > 0).view(-1)
    marked = rows[::2]                                                        # the keys of every other labelled edge are zero-shot
    key = (gt_cls[edges[:, 0]] * C + gt_cls[edges[:, 1]]) * R + labels
    table = torch.zeros(C * C * R, dtype=torch.uint8)
    table[key[marked]] = 1
    n_zs = int(torch.isin(key[rows], key[marked]).sum())
    table = table.to(DEV)
    S = EV.split_fields()
    for use_2d in (True, False):
        want = M.eval_triplet_split(torch.zeros(12, dtype=torch.int64, device=DEV), case.t3, case.t2 if use_2d else None, b["gt_class"], case.hot,
                                    case.edges, table)
        got, counts = torch.zeros(12, dtype=torch.int64, device=DEV), case.zeros()
        assert case.one_call(counts, use_2d=use_2d, split_table=table, split_counts=got) is True
        torch.cuda.synchronize()
        _assert_vector(S, got, want, ("split", use_2d, C, R))
        _assert_vector(case.F, counts, case.want, ("counts beside the split", use_2d, C, R), in_2d=None if use_2d else 0)
        assert int(got[S.index("zs_all_n_3d")]) == len(rows) == 28 and int(got[S.index("zs_n_3d")]) == n_zs and 14 <= n_zs < 28
        assert int(got[S.index("zs_n_2d")]) == (n_zs if use_2d else 0)


# ---- 5. the loop -------------------------------------------------------------------------------------------------------------------
def test_pipelined_validation_of_a_single_label_model(case):
    """workers=2 and workers=2, merge=4 (four one-scene batches collated per call: a merged forward) give the host loop's dict exactly;
    the seeds carry no near-tie other than the planted exact duplicate (module docstring)"""
    batches = loop_items(case.C, case.R)
    want = EV.validation(case.model, batches, device=DEV, workers=0)
    assert want["scenes"] == 8 and any(k.endswith("_2d") for k in want)
    for kw in (dict(workers=2), dict(workers=2, merge=4)):
        got = EV.validation(case.model, batches, device=DEV, **kw)
        assert list(got) == list(want), kw
        bad = [(k, got[k], want[k]) for k in want if np.array([got[k]]).tobytes() != np.array([want[k]]).tobytes()]
        assert not bad, (kw, bad[:8])


# ---- 6. multi-label models are untouched (the rel_is_log = false instantiation) ------------------------------------------------------
@pytest.mark.parametrize("n_obj,n_rel", GEOMETRIES)
def test_multi_label_one_call_still_equals_the_separate_calls(n_obj, n_rel):
    _need_gpu()
    c = Case(n_obj, n_rel, multi=True)
    try:
        assert int((c.hot.sum(1) == 2).sum()) > 0 and int((c.hot.sum(1) == 0).sum()) == 28
        got = c.zeros()
        assert c.one_call(got) is True
        only = c.zeros()
        assert c.one_call(only, use_2d=False) is True
        torch.cuda.synchronize()
        _assert_vector(c.F, got, c.want, ("multi-label", n_obj, n_rel))
        _assert_vector(c.F, only, c.want, ("multi-label, 3D only", n_obj, n_rel), in_2d=0)
    finally:
        c.close()
