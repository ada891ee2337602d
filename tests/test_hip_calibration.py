"""Score histograms on the GPU (csrc/calibration.hip via vlsat_score_hist): every table equal, entry for entry, to the host
restatement fed the same probabilities -- sizes on either side of a block iteration and of the persistent grid's wrap, every
predicate grouping the LDS budget produces, the values at which the bin rule can go wrong, the all-equal worst case, accumulation
from two calls and two streams, skipped outputs, and evaluate.calibrate with the thresholds it promises."""
import ctypes as C

import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import evaluate as EV, lib as L, metrics as M

from calibration_checks import assert_counts_match, assert_tables_equal, device_tables, host_tables, make_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HEADS = [(1, True), (26, True), (32, True), (27, False)]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path cannot run and there is no fallback")


def _geometry(r, bins):
    a, b = C.c_int32(), C.c_int32()
    L.load().vlsat_score_hist_geometry(r, bins, C.byref(a), C.byref(b))
    return a.value, b.value


def test_geometry_is_what_the_shapes_below_assume():
    _need_gpu()
    for r, _ in HEADS:
        for bins in (16, 1024, 4096):
            step, sweep = _geometry(r, bins)
            assert step == 16 and sweep % step == 0 and step < sweep <= 8192, (r, bins, step, sweep)
    assert _geometry(26, 1024)[1] < _geometry(26, 16)[1]           # more predicate groups, fewer edge chunks each
    assert _geometry(33, 1024) == (0, 0) and _geometry(26, 1000) == (0, 0)


@pytest.mark.parametrize("bins", [16, 1024, 4096])
@pytest.mark.parametrize("r,multi", HEADS)
def test_hip_equals_host_around_every_boundary(r, multi, bins):
    """E = 1, one below / at / one above a block iteration and the grid's wrap, two wraps and a bit, and the 72 + 132 edges of a
    ragged two-scene batch (9 and 12 objects); N and C walk through {1, 5, 257} x {1, 160, 1024}."""
    _need_gpu()
    step, sweep = _geometry(r, bins)
    sizes = [1, step - 1, step, step + 1, sweep - 1, sweep, sweep + 1, 2 * sweep + step + 3, 9 * 8 + 12 * 11]
    nodes = [(1, 1), (5, 160), (257, 1024), (21, 160)]
    for i, e in enumerate(sizes):
        n, c = nodes[-1] if e == 204 else nodes[i % 3]
        case = make_case(e, r, bins, multi, seed=1000 * r + bins + e, n=n, c=c)
        got, want = device_tables(case, DEV), host_tables(case)
        assert_tables_equal(got, want, f"E={e} N={n} C={c}")
        if e in (sweep + 1, 204):
            assert_counts_match(got.cpu(), case)


def test_nothing_to_do_launches_nothing_and_leaves_the_tables():
    _need_gpu()
    case = make_case(0, 26, 1024, True, seed=1, n=0)
    t = M.ScoreTables(26, 160, 1024, DEV)
    t.buffer.fill_(7)
    device_tables(case, DEV, tables=t)
    assert bool((t.buffer == 7).all())
    fresh = device_tables(case, DEV)
    assert int(fresh.buffer.abs().sum()) == 0


@pytest.mark.parametrize("bins", [1024, 4096])
def test_worst_case_every_score_equal(bins):
    """70 000 edges x 26 predicates on ONE column per predicate (mid-bin, exactly 1.0, NaN), then two values alternating by
    predicate and by edge: a narrow or packed counter, a lost flush or a wrong combine of equal keys shows as a wrong total."""
    _need_gpu()
    e, r = 70000, 26
    g = torch.Generator().manual_seed(5)
    case = make_case(8, r, bins, True, seed=2, n=5)
    case["gt_rel"] = (torch.rand(e, r, generator=g) < 0.1).long()
    lane = torch.arange(r)[None, :].expand(e, r)
    edge = torch.arange(e)[:, None].expand(e, r)
    mid = (37 + 0.5) / bins
    fills = [("mid", torch.full((e, r), mid), 37), ("one", torch.full((e, r), 1.0), bins - 1), ("nan", torch.full((e, r), float("nan")), bins),
             ("by predicate", torch.where(lane % 2 == 0, 0.25, mid).float(), None), ("by edge", torch.where(edge % 2 == 0, 0.25, mid).float(), None),
             ("by both", torch.where((edge + lane) % 2 == 0, 0.25, mid).float(), None)]
    for name, rp, col in fills:
        case["rp"] = rp.contiguous()
        got = device_tables(case, DEV).cpu()
        assert_tables_equal(got, host_tables(case), name)
        if col is not None:
            assert got.rel[:, :, col].sum(1).tolist() == [e] * r, name
        else:
            assert int(got.rel[:, :, [bins // 4, 37]].sum()) == e * r, name


def test_accumulation_two_calls_two_streams_and_skipped_outputs():
    _need_gpu()
    case = make_case(5000, 26, 1024, True, seed=9, n=257)
    one = device_tables(case, DEV)
    twice = device_tables(case, DEV, tables=device_tables(case, DEV))
    assert torch.equal(twice.buffer, 2 * one.buffer)
    # two streams into one table
    other = make_case(3001, 26, 1024, True, seed=10, n=5)
    shared = M.ScoreTables(26, 160, 1024, DEV)
    dcases = [{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in c.items()} for c in (case, other)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=DEV) for _ in range(2)]
    for s, c in zip(streams, dcases):
        with torch.cuda.stream(s):
            for _ in range(3):
                M.score_histograms(c["probs"], c["rp"], c["gt_cls"], c["gt_rel"], True, 1024, obj_probs=c["probs"], rel_probs=c["rp"], tables=shared)
    for s in streams:
        s.synchronize()
    assert torch.equal(shared.buffer.cpu(), 3 * (one.buffer.cpu() + host_tables(other).buffer))
    # a NULL output is skipped and the others are what they are with all three
    lib, c = L.load(), dcases[0]
    for skip in range(3):
        t = M.ScoreTables(26, 160, 1024, DEV)
        t.buffer.fill_(3)
        ptrs = [t.rel.data_ptr(), t.obj.data_ptr(), t.confusion.data_ptr()]
        ptrs[skip] = None
        L.check(lib.vlsat_score_hist(c["probs"].data_ptr(), c["rp"].data_ptr(), c["gt_cls"].data_ptr(), c["gt_rel"].data_ptr(), 257, 5000, 160,
                                     26, 1, 1024, *ptrs, L.stream_ptr()))
        for i, f in enumerate(("rel", "obj", "confusion")):
            want = torch.full_like(getattr(one, f), 3) + (0 if i == skip else getattr(one, f))
            assert torch.equal(getattr(t, f), want), (skip, f)


def test_limits_are_checked_before_any_launch():
    _need_gpu()
    lib = L.load()
    t = M.ScoreTables(26, 160, 1024, DEV)
    x = torch.zeros(64, device=DEV)
    for n, e, c, r, multi, bins in ((1, 1, 160, 33, 1, 1024), (1, 1, 1025, 26, 1, 1024), (1, 1, 160, 26, 1, 1000), (1, 1, 160, 26, 1, 8192),
                                    (1, 1, 160, 26, 2, 1024), (-1, 1, 160, 26, 1, 1024), (1, (1 << 26) + 1, 160, 26, 1, 1024),
                                    (1, 1 << 26, 160, 32, 1, 1024)):
        rc = lib.vlsat_score_hist(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), n, e, c, r, multi, bins, t.rel.data_ptr(),
                                  t.obj.data_ptr(), t.confusion.data_ptr(), L.stream_ptr())
        assert rc < 0 and b"score_hist" in lib.vlsat_last_error(), (n, e, c, r, multi, bins)
    assert lib.vlsat_score_hist(None, None, None, None, 1, 1, 160, 26, 1, 1024, t.rel.data_ptr(), None, None, L.stream_ptr()) < 0
    torch.cuda.synchronize()
    assert int(t.buffer.abs().sum()) == 0
    with pytest.raises(L.VlsatError):
        M.score_histograms(torch.zeros(2, 160, device=DEV), torch.zeros(3, 26, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV),
                           torch.zeros(3, dtype=torch.int64, device=DEV), True)


def _model():
    from vlsat_amd import VLSATConfig, synth
    from vlsat_amd.model import VLSATModel
    cfg = VLSATConfig(N_LAYERS=1)
    return VLSATModel(cfg, DEV).load_state(synth.make_weights(cfg)).eval()


def _scene(n_obj, seed):
    from vlsat_amd import synth
    b = synth.collate([synth.make_scene(n_obj, 32, seed)])
    item = {k: torch.from_numpy(v).to(DEV) for k, v in b.items() if k != "edge_indices"}
    ei = torch.from_numpy(b["edge_indices"]).t().contiguous().to(DEV)
    g = torch.Generator().manual_seed(seed)
    item.update(edge_indices=ei, fc_sizes=[n_obj], n_scenes=1, gt_class=torch.randint(0, 160, (n_obj,), generator=g).to(DEV),
                gt_rel_cls=(torch.rand(ei.shape[0], 26, generator=g) < 0.05).long().to(DEV))
    return item


def test_calibrate_keeps_its_promise():
    """evaluate.calibrate: the same tables with and without worker threads, equal to the host restatement on the forward's own
    outputs; the thresholds operating_points picks give, through the existing decode_counts, exactly the tp / fp / fn it states."""
    _need_gpu()
    m = _model()
    bs = [_scene(9, 31), _scene(12, 32)]
    bins = 1024
    serial = EV.calibrate(m, bs, bins=bins)
    piped = EV.calibrate(m, bs, device=DEV, workers=2, bins=bins)
    only3 = EV.calibrate(m, bs, device=DEV, workers=2, use_2d=False, bins=bins)
    assert only3["2d"] is None
    assert_tables_equal(only3["3d"], serial["3d"], "3D only")
    outs = []
    for b in bs:
        o3, o2, r3, r2 = m(b["obj_points"], b["obj_2d_feats"], b["edge_indices"].t(), b["descriptor"], b.get("batch_ids"), fc_sizes=b["fc_sizes"])
        outs.append(((o3, M.softmax_rows(o3), r3), (o2, M.softmax_rows(o2), r2)))
    torch.cuda.synchronize()
    for i, br in enumerate(("3d", "2d")):
        assert_tables_equal(piped[br], serial[br], br)
        want = M.ScoreTables(26, 160, bins)
        for b, o in zip(bs, outs):
            obj, probs, rel = (x.cpu() for x in o[i])
            M.score_histograms(obj, rel, b["gt_class"].cpu(), b["gt_rel_cls"].cpu(), True, bins, obj_probs=probs, tables=want)
        assert_tables_equal(serial[br], want, br + " against the host")
        assert int(serial[br].rel.sum()) == (72 + 132) * 26 and int(serial[br].obj.sum()) == 21
        ops = EV.operating_points(serial[br])
        counts = torch.zeros(M.decode_counts_width(26), dtype=torch.int64, device=DEV)
        for b, o in zip(bs, outs):
            obj, probs, rel = o[i]
            M.decode_counts(obj, rel, b["gt_class"], b["gt_rel_cls"], True, ops["threshold"], obj_probs=probs, counts=counts)
        assert torch.equal(counts[:78].cpu(), ops["counts"]), br
        q = EV.graph_quality(counts.cpu(), 26)
        assert ops["micro_f1"] == q["micro_f1"] and ops["macro_f1"] == q["macro_f1"] >= ops["macro_f1_default"]
    m.close()
