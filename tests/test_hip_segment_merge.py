"""Segments merged into objects on the GPU (csrc/segment_merge.hip via vlsat_merge_segments): every table equal to the host
restatement fed the same probabilities, the pooled probabilities bit for bit -- paths that cross a wave and a block, interleaved
paths, thousands of edges folding onto few pairs, an empty scene, the class-count extremes, both link rules, with and without
weights, a forward's own outputs through VLSATModel.merge_graph, and the refused arguments."""
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import evaluate as EV, lib as L, metrics as M

from segment_merge_checks import assert_tables, brute, path, random_groups

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path cannot run and there is no fallback")


def _both(c, trim=True):
    d = lambda t: None if t is None else t.to(DEV)
    args = (c["n_scenes"], c["same_part"], c["threshold"], c["mutual"])
    got = M.merge_segments(d(c["obj_probs"]), d(c["rel_probs"]), d(c["edges"]), d(c["batch_ids"]), *args, d(c["weights"]),
                           obj_probs=d(c["obj_probs"]), rel_probs=d(c["rel_probs"]), trim=trim)
    want = M.merge_segments_host(c["obj_probs"], c["rel_probs"], c["edges"], c["batch_ids"], *args, c["weights"], obj_probs=c["obj_probs"],
                                 rel_probs=c["rel_probs"], trim=trim)
    return got, want


CASES = {
    "path70_descending": lambda: path(70, descending=True, weights="mixed"),                   # crosses a wave; repeated jumping
    "path300_descending": lambda: path(300, descending=True),                                  # crosses a block
    "path300_ascending_mutual": lambda: path(300, descending=False, mutual=True),              # no reverse edge: nothing links
    "two_interleaved_paths": lambda: path(257, descending=True, step=2, weights="mixed"),
    "random_5000_over_300": lambda: random_groups(300, 40, 5000, 11, c=160, r=26, same_part=25),
    "random_5000_mutual_weights": lambda: random_groups(300, 40, 5000, 12, c=160, r=26, same_part=0, mutual=True, weights="mixed"),
    "three_scenes_empty_middle": lambda: random_groups(150, 12, 1200, 13, scenes=[70, 0, 80], weights="mixed"),
    "one_class_one_predicate": lambda: random_groups(130, 10, 900, 14, c=1, r=1, same_part=0, weights="mixed"),
    "1024_classes_32_predicates": lambda: random_groups(90, 7, 700, 15, c=1024, r=32, same_part=31, mutual=True),
    # the one-block scans (1024 threads) past one element per thread: 1025 nodes are runs of 2 and threads 513.. own nothing; 2500
    # nodes are runs of 3 with a ragged last one (thread 833 owns one node), 6000 edges runs of 6
    "path1025_descending": lambda: path(1025, descending=True),
    "random_6000_over_2500": lambda: random_groups(2500, 200, 6000, 16),
}
LONG_RUNS = ("path1025_descending", "random_6000_over_2500")                                 # also against the rule as loops


@pytest.mark.parametrize("name", list(CASES))
def test_hip_equals_host(name):
    _need_gpu()
    c = CASES[name]()
    got, want = _both(c)
    assert_tables(got, want, name)
    if name in LONG_RUNS:
        assert_tables(got, brute(c), name)


def test_what_the_cases_exercise():
    """(host only) the sizes the cases are there for."""
    c = CASES["random_5000_over_300"]()
    g = M.merge_segments_host(c["obj_probs"], c["rel_probs"], c["edges"], None, 1, c["same_part"], obj_probs=c["obj_probs"], rel_probs=c["rel_probs"])
    assert 38 <= int(g.totals[0]) <= 45 and int(g.pair_count.max()) >= 4 and int(g.totals[1]) < 45 * 45
    c = CASES["path300_ascending_mutual"]()
    g = M.merge_segments_host(c["obj_probs"], c["rel_probs"], c["edges"], None, 1, c["same_part"], mutual=True, obj_probs=c["obj_probs"],
                              rel_probs=c["rel_probs"])
    assert g.totals.tolist() == [300, 301]
    c = CASES["two_interleaved_paths"]()
    g = M.merge_segments_host(c["obj_probs"], c["rel_probs"], c["edges"], None, 1, c["same_part"], obj_probs=c["obj_probs"], rel_probs=c["rel_probs"])
    assert g.totals.tolist() == [2, 0] and g.root.tolist() == [0, 1] * 128 + [0]          # (both ends are even: the extra edges fold away)


def test_untrimmed_call_writes_every_field_and_reads_nothing_back():
    _need_gpu()
    got, want = _both(CASES["three_scenes_empty_middle"](), trim=False)
    assert not got.trimmed and got.pair_probs.shape == want.pair_probs.shape
    assert_tables(got, want)


def test_empty_inputs():
    _need_gpu()
    from segment_merge_checks import _case
    for c in (_case(0, [], [], n_scenes=1), _case(4, [], [], batch_ids=[0, 0, 1, 1], n_scenes=2), _case(0, [], [], n_scenes=0)):
        for trim in (True, False):
            got, want = _both(c, trim)
            assert_tables(got, want)


def test_merge_graph_on_a_forwards_own_outputs():
    _need_gpu()
    from vlsat_amd import VLSATConfig, synth
    from vlsat_amd.model import VLSATModel
    cfg = VLSATConfig(N_LAYERS=1)
    m = VLSATModel(cfg, DEV).load_state(synth.make_weights(cfg)).eval()
    b = synth.collate([synth.make_scene(9, 32, 5), synth.make_scene(12, 32, 6)])
    t = {k: torch.from_numpy(v).to(DEV) for k, v in b.items()}
    ei, bid = t["edge_indices"], t["batch_ids"]
    o3, o2, r3, r2 = m(t["obj_points"], t["obj_2d_feats"], ei, t["descriptor"], bid)
    same_part = 7
    thr = float(r3[:, same_part].float().quantile(0.9))                               # synthetic weights: nothing is calibrated
    w = torch.arange(1, o3.shape[0] + 1, dtype=torch.float32) * 37.0
    pairs = m.merge_graph(t["obj_points"], t["obj_2d_feats"], ei, t["descriptor"], bid, same_part=same_part, weights=w, threshold=thr,
                          n_labels=2, max_rel=50)
    for (g, d), o, r in zip(pairs, (o3, o2), (r3, r2)):
        probs = M.softmax_rows(o).cpu()
        want = M.merge_segments_host(o.cpu(), r.cpu(), ei.t().cpu(), bid.view(-1).cpu(), 2, same_part, thr, False, w, obj_probs=probs)
        assert_tables(g, want)
        assert 2 <= int(want.totals[0]) < o.shape[0]                                  # some segments merged, not all
        dw = want.decode(n_labels=2, max_rel=50)
        for k in ("labels", "label_probs", "edge", "pred", "score", "n_valid", "n_total"):
            assert torch.equal(getattr(d, k).cpu(), getattr(dw, k)), k
    only3d = m.merge_graph(t["obj_points"], None, ei, t["descriptor"], bid, same_part=same_part, weights=w, threshold=thr, n_labels=2, max_rel=50)
    assert only3d[1] is None
    assert_tables(only3d[0][0], pairs[0][0])
    item = dict(t, edge_indices=ei.t().contiguous(), n_scenes=2, weights=w)
    per_scene = list(EV.merged(m, [item], same_part=same_part, threshold=thr, n_labels=2, max_rel=50))
    assert len(per_scene) == 2
    g0 = pairs[0][0]
    assert [int(s[0][0].totals[0]) for s in per_scene] == g0.n_objects.tolist()
    assert sum(int(s[0][0].totals[1]) for s in per_scene) == int(g0.totals[1])


def test_evaluate_merged_pipelined_equals_the_serial_loop():
    """EV.merged(workers=2) -- replicas, streams, results put back in input order, a two-scene item split per scene -- against the
    serial loop: the same graphs, scene by scene and branch by branch."""
    _need_gpu()
    from vlsat_amd import VLSATConfig, synth
    from vlsat_amd.model import VLSATModel
    cfg = VLSATConfig(N_LAYERS=1)
    m = VLSATModel(cfg, DEV).load_state(synth.make_weights(cfg)).eval()

    def item(sizes, seed):
        b = synth.collate([synth.make_scene(n, 32, seed + i) for i, n in enumerate(sizes)])
        t = {k: torch.from_numpy(v).to(DEV) for k, v in b.items()}
        n = t["obj_points"].shape[0]
        return dict(t, edge_indices=t["edge_indices"].t().contiguous(), n_scenes=len(sizes),
                    weights=torch.arange(1, n + 1, dtype=torch.float32) * 37.0)

    items = [item([n], 40 + 10 * i) for i, n in enumerate((3, 11, 5, 8, 6))]
    items.insert(3, item([7, 4], 100))
    two = items[3]
    same_part = 7
    r3 = m(two["obj_points"], two["obj_2d_feats"], two["edge_indices"].t(), two["descriptor"], two["batch_ids"])[2]
    kw = dict(same_part=same_part, threshold=float(r3[:, same_part].float().quantile(0.9)), n_labels=2, max_rel=50)
    serial = list(EV.merged(m, items, **kw))
    piped = list(EV.merged(m, items, device=DEV, workers=2, **kw))
    assert len(serial) == len(piped) == 7
    assert [s[0][0].root.numel() for s in piped] == [3, 11, 5, 7, 4, 8, 6]          # input order, the pair split in two
    for want, got in zip(serial, piped):
        for (gw, dw), (gg, dg) in zip(want, got):
            assert_tables(gg, gw)
            for k in dw.__slots__:
                assert torch.equal(getattr(dg, k), getattr(dw, k)), k
    only3 = list(EV.merged(m, items, device=DEV, workers=2, use_2d=False, **kw))
    assert len(only3) == 7
    for want, got in zip(serial, only3):
        assert got[1] is None
        assert_tables(got[0][0], want[0][0])
        for k in want[0][1].__slots__:
            assert torch.equal(getattr(got[0][1], k), getattr(want[0][1], k)), k
    m.close()


def test_bad_arguments_are_errors_not_faults():
    _need_gpu()
    lib = L.load()
    n, e, c, r = 4, 3, 5, 2
    i32 = dict(dtype=torch.int32, device=DEV)
    probs, rp = torch.rand(n, c, device=DEV), torch.rand(e, r, device=DEV)
    edges = torch.tensor([[0, 1], [1, 2], [2, 3]], device=DEV)
    outs = [torch.empty(n, **i32), torch.empty(n, **i32), torch.empty(2, **i32), torch.empty(2, **i32), torch.empty(n + 1, **i32),
            torch.empty(n, **i32), torch.empty(n, c, device=DEV), torch.empty(n, device=DEV), torch.empty(n, dtype=torch.int64, device=DEV),
            torch.empty(e, **i32), torch.empty(e, 2, dtype=torch.int64, device=DEV), torch.empty(e, **i32), torch.empty(e, r, device=DEV)]
    scratch = torch.empty(int(lib.vlsat_merge_segments_scratch_bytes(n, e, c, r, 2)), dtype=torch.uint8, device=DEV)
    bid = torch.tensor([0, 0, 1, 1], device=DEV)

    def call(n_=n, e_=e, n_scenes=1, same_part=1, batch_ids=None):
        return lib.vlsat_merge_segments(probs.data_ptr(), rp.data_ptr(), edges.data_ptr(), L.ptr(batch_ids), None, n_, e_, c, r, n_scenes,
                                        same_part, 0.5, 0, scratch.data_ptr(), *(t.data_ptr() for t in outs), L.stream_ptr())

    assert scratch.numel() > 0 and call() == 0 and call(n_scenes=2, batch_ids=bid) == 0
    for kw, word in ((dict(same_part=2), "same_part"), (dict(same_part=-1), "same_part"), (dict(n_scenes=2), "batch_ids"),
                     (dict(n_=-1), "negative"), (dict(e_=-1), "negative"), (dict(n_scenes=-1), "negative")):
        assert call(**kw) == -1, kw
        assert word in lib.vlsat_last_error().decode(), kw
    assert int(lib.vlsat_merge_segments_scratch_bytes(-1, 3, 5, 2, 1)) == 0 and int(lib.vlsat_merge_segments_scratch_bytes(4, 3, 5, 33, 1)) == 0
    torch.cuda.synchronize()
