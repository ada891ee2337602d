"""GPU Recall@K / mR@K counts (csrc/eval_recall.hip via vlsat_eval_recallk): equal to the reference goldens, to the host path
bit for bit on batches of the benchmark's shape and on a configs[4]-sized scene, batch == one-scene calls, and
validation(recall_k=True) the same on the one-scene loop and the pipelined, merged one."""
import os

import numpy as np
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import evaluate as EV, lib as L, metrics as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "recallk_cases.npz")
VARIANTS = ("predcls_gc", "predcls_ngc", "sgcls_gc", "sgcls_ngc")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path cannot run and there is no fallback")


def _case(z, i, br):
    t = lambda k: torch.from_numpy(z[f"c{i}_{k}"]).to(DEV)
    return t(f"obj_logits_{br}"), t(f"rel_{br}"), t("gt_cls"), t("gt_rel"), t("edges"), bool(z[f"c{i}_multi"])


def _golden(row, r, name):
    base = M.recallk_offset(name, r)
    with np.errstate(invalid="ignore", divide="ignore"):
        rec = np.array([row[base + q] for q in range(3)], dtype=np.int64) / int(row[0])
    mrec = np.array([[row[base + 3 + q * r + j] / row[1 + j] if row[1 + j] else -1 for q in range(3)] for j in range(26)])
    return rec, mrec


@pytest.mark.parametrize("br", ["3d", "2d"])
def test_hip_counts_equal_reference_goldens(br):
    _need_gpu()
    z = np.load(GOLD)
    for i in range(int(z["n_cases"])):
        obj, rel, gt_cls, gt_rel, edges, multi = _case(z, i, br)
        row = M.recallk_counts(obj, rel, gt_cls, gt_rel, edges, None, 1, multi)[0].cpu().numpy()
        for name in VARIANTS:
            rec, mrec = _golden(row, rel.shape[1], name)
            np.testing.assert_array_equal(rec, z[f"c{i}_R_{name}_{br}"], err_msg=f"case {i} {name}")
            np.testing.assert_array_equal(mrec, z[f"c{i}_mR_{name}_{br}"], err_msg=f"case {i} {name}")
        gt = []
        for e, (a, b) in enumerate(edges.tolist()):                       # the drop-in on device tensors
            rels = [k for k in range(26) if int(gt_rel[e, k]) == 1] if multi else ([int(gt_rel[e])] if int(gt_rel[e]) else [])
            gt.append((int(gt_cls[a]), int(gt_cls[b]), rels))
        got = M.evaluate_triplet_recallk(obj, rel, gt, edges, multi, [20, 50, 100], 100, use_clip=True, evaluate="triplet")
        np.testing.assert_array_equal(got, z[f"c{i}_R_sgcls_ngc_{br}"])


def _synth(n_scenes, n_obj, multi, seed, sharp):
    """A fully connected batch with random outputs of both branches: logits whose scale varies per object, some gt labels."""
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
        z = torch.randn(e, 26, generator=g) * 2
        rel = torch.sigmoid(z) if multi else torch.log_softmax(z, -1)
        outs.append((obj, rel))
    to = lambda t: t.to(DEV)
    return [(to(o), to(r)) for o, r in outs], to(gt_cls), to(gt_rel), to(edges), to(bid)


def _host_equal(outs, gt_cls, gt_rel, edges, bid, n_scenes, multi):
    for obj, rel in outs:
        probs = M.softmax_rows(obj)                      # the same probabilities for both paths
        got = M.recallk_counts(obj, rel, gt_cls, gt_rel, edges, bid, n_scenes, multi, obj_probs=probs)
        want = M.recallk_counts_host(obj, rel, gt_cls, gt_rel, edges, bid, n_scenes, multi, obj_probs=probs)
        assert torch.equal(got, want), (got - want).abs().sum(0).nonzero().view(-1).tolist()
        assert int(got[:, 1 + 26 + 2:1 + 26 + 3].sum()) > 0                  # predcls_gc hits at 100 exist


@pytest.mark.parametrize("multi", [True, False])
def test_hip_equals_host_on_the_bench_batch_shape(multi):
    """configs[1] shape: 64 scenes x 40 objects, E = 99 840, both branches."""
    _need_gpu()
    outs, gt_cls, gt_rel, edges, bid = _synth(64, 40, multi, 51 + multi, sharp=6.0)
    assert edges.shape[0] == 99840
    _host_equal(outs, gt_cls, gt_rel, edges, bid, 64, multi)
    # the batch equals its scenes called one at a time
    obj, rel = outs[0]
    whole = M.recallk_counts(obj, rel, gt_cls, gt_rel, edges, bid, 64, multi)
    for s in (0, 17, 63):
        sl = slice(s * 1560, (s + 1) * 1560)
        one = M.recallk_counts(obj[s * 40:(s + 1) * 40], rel[sl], gt_cls[s * 40:(s + 1) * 40], gt_rel[sl], edges[sl] - s * 40,
                               None, 1, multi)
        assert torch.equal(whole[s], one[0]), s


def test_hip_batch_equals_one_scene_calls_on_goldens():
    _need_gpu()
    z = np.load(GOLD)
    cases = [i for i in range(int(z["n_cases"])) if bool(z[f"c{i}_multi"])]
    parts = [_case(z, i, "2d") for i in cases]
    off, objs, rels, gc, gr, ed, bids = 0, [], [], [], [], [], []
    for s, (obj, rel, gt_cls, gt_rel, edges, _) in enumerate(parts):
        objs.append(obj); rels.append(rel); gc.append(gt_cls); gr.append(gt_rel); ed.append(edges + off)
        bids.append(torch.full((obj.shape[0],), s, dtype=torch.int64, device=DEV))
        off += obj.shape[0]
    whole = M.recallk_counts(torch.cat(objs), torch.cat(rels), torch.cat(gc), torch.cat(gr), torch.cat(ed), torch.cat(bids),
                             len(parts), True)
    for s, (obj, rel, gt_cls, gt_rel, edges, _) in enumerate(parts):
        assert torch.equal(whole[s], M.recallk_counts(obj, rel, gt_cls, gt_rel, edges, None, 1, True)[0]), s
    # a scene without edges in the middle of a batch: zero counts, the neighbours unchanged
    b2 = torch.cat([bids[0], torch.full((3,), 1, device=DEV, dtype=torch.int64), bids[1] + 1])
    o2 = torch.cat([objs[0], torch.zeros(3, 160, device=DEV), objs[1]])
    g2 = torch.cat([gc[0], torch.zeros(3, dtype=gc[0].dtype, device=DEV), gc[1]])
    e2 = torch.cat([ed[0], ed[1] + 3])
    r2 = torch.cat(rels[:2])
    t2 = torch.cat(gr[:2])
    got = M.recallk_counts(o2, r2, g2, t2, e2, b2, 3, True)
    assert torch.equal(got[0], whole[0]) and int(got[1].abs().sum()) == 0 and torch.equal(got[2], whole[1])


def test_hip_configs4_scene_within_its_scratch():
    """One configs[4]-sized scene: 200 objects, 39 800 edges; the scratch is what vlsat_eval_recallk_scratch_bytes states."""
    _need_gpu()
    outs, gt_cls, gt_rel, edges, bid = _synth(1, 200, True, 77, sharp=6.0)
    assert edges.shape[0] == 39800
    nbytes = int(L.load().vlsat_eval_recallk_scratch_bytes(200, 39800, 160, 26, 1))
    assert nbytes < 24 << 20, nbytes
    _host_equal(outs[:1], gt_cls, gt_rel, edges, bid, 1, True)


def _label_batches(n_batches, seed):
    from vlsat_amd import VLSATConfig, synth
    cfg = VLSATConfig(N_LAYERS=1)
    w = synth.make_weights(cfg)
    g = torch.Generator().manual_seed(seed)
    batches = []
    for s in range(n_batches):
        n = int(torch.randint(3, 12, (1,), generator=g))
        b = synth.collate([synth.make_scene(n, 32, 9300 + s)])
        e = b["edge_indices"].shape[1]
        item = {k: torch.from_numpy(v).to(DEV) for k, v in b.items() if k != "edge_indices"}
        item.update(gt_class=torch.randint(0, 160, (n,), generator=g).to(DEV),
                    gt_rel_cls=(torch.rand(e, 26, generator=g) < 0.1).long().to(DEV),
                    edge_indices=torch.from_numpy(b["edge_indices"]).t().contiguous().to(DEV), fc_sizes=[n])
        batches.append(item)
    return cfg, w, batches


def test_validation_recall_agrees_between_loops():
    """validation(recall_k=True): the one-scene host loop (workers=0), the pipelined loop (workers=2) and the merged one
    (workers=2, merge=4) give the same recalls; merging changes the forward's last bits, so those agree up to near-ties."""
    _need_gpu()
    from vlsat_amd.model import VLSATModel
    cfg, w, batches = _label_batches(13, 31)
    model = VLSATModel(cfg, DEV).load_state(w).eval()
    plain = EV.validation(model, batches, device=DEV)
    s0 = EV.validation(model, batches, device=DEV, recall_k=True)
    assert {k: s0[k] for k in plain} == plain
    rk = [k for k in s0 if k not in plain]
    assert len(rk) == 2 * 4 * 3 * 4 and all(np.isfinite(s0[k]) for k in rk)
    s2 = EV.validation(model, batches, device=DEV, workers=2, recall_k=True)
    for k in rk:
        assert s2[k] == pytest.approx(s0[k], rel=1e-12, abs=1e-12), k
    s4 = EV.validation(model, batches, device=DEV, workers=2, merge=4, recall_k=True)
    assert set(s4) == set(s0)
    for k in rk:
        assert abs(s4[k] - s0[k]) <= 100 / 13 + 1e-9, (k, s0[k], s4[k])       # at most one scene's hit moved
