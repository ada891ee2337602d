"""fp32 mode, "edge_pairs_e2": the 2D chain tensor E2, as the LayerNorm of the edge attention and conv3 of rel_encoder_2d write it, travels
to its readers (nn_edge.0 and proj_edge of gcn_2ds, the first Linear of the 2D relation head) as GEMM pair words; what nn_edge.2 writes
into the same buffer stays fp32 (csrc/edge_pairs.h, EdgePairs::e2).  The split depends on the word alone, so no MFMA operand changes:
every test here compares the four outputs with the option on (the default) against the option off -- the forward of the release before --
BIT FOR BIT.  On which plans E2 pairs is decided by edge_pairs_plan; tests/test_e2_pairs_cpu.py pins that on the host, and the cases
below that must NOT pair read the same program's answer.
A plan of at most "pair_max_edges" = 4096 edges runs the paired schedule by default, on which nothing pairs -- and every batch here is that
small.  The models of this file therefore run with "pair_twins" 0 (the schedule of the large plans: E2 pairs, as the program's "E = 720"
line says, and test_e2_buffer_holds_the_pair_words_of_the_fp32_forward looks at the tensor itself); test_e2_pairs_paired_schedule
switches the paired schedule back on.  Needs an MI355X:  pytest -m gpu"""
import numpy as np
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import VLSATConfig, synth
import host_check
import e2_pairs_pack as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("obj3d", "obj2d", "rel3d", "rel2d")
TIGHT = 1e-4

# what an option is set back to: the library's defaults, except "pair_twins" (see above)
DEFAULTS = {"edge_pairs": 1, "edge_pairs_e2": 1, "gemm_p8_part_min": 0, "gemm_splitk": 1, "pair_twins": 0, "gemm_exact": -1,
            "gemm_small_exact": -1, "flash_exact": -1, "dual_stream": 2, "sched": -1}


def _dev(b):
    return {k: torch.from_numpy(v).to(DEV) for k, v in b.items()}


def _args(d):
    return (d["obj_points"], d["obj_2d_feats"], d["edge_indices"], d["descriptor"], d["batch_ids"])


def _run(m, d, **kw):
    out = m(*_args(d), **kw)
    torch.cuda.synchronize()
    return [o.clone().cpu() for o in out if torch.is_tensor(o)]


class _Options:
    def __init__(self, m, **options):
        self.m, self.options = m, options

    def __enter__(self):
        for k, v in self.options.items():
            self.m.debug_option(k, v)
        return self.m

    def __exit__(self, *exc):
        for k in self.options:
            self.m.debug_option(k, DEFAULTS[k])


def _same(got, ref, what):
    assert len(got) == len(ref), what
    for i, (a, c) in enumerate(zip(got, ref)):
        assert a.shape == c.shape, (what, i)
        assert torch.isfinite(a).all(), (what, i)
        assert torch.equal(a, c), (what, i, float((a - c).abs().max()) if a.numel() else 0.0)


def _on_off(m, batch, what, run=_run, **options):
    d = _dev(batch)
    with _Options(m, **options):
        got = run(m, d)
        with _Options(m, edge_pairs_e2=0):
            ref = run(m, d)
    _same(got, ref, what)
    return got


def _decisions():
    return {name: right.split(" | ")[0] for name, right in host_check.lines("e2_pairs_check")}


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path cannot run and there is no fallback")
    from vlsat_amd.model import VLSATModel
    # 3 scenes x 16 objects x 64 points: E = 720 = two full 256-row panels and a cut one
    main = synth.collate([synth.make_scene(16, 64, 7500 + j) for j in range(3)])
    cfgs = {3: VLSATConfig(N_LAYERS=3), 1: VLSATConfig(N_LAYERS=1)}
    models = {}
    for L, cfg in cfgs.items():
        models[L, "bench"] = VLSATModel(cfg, DEV).load_state(synth.make_weights(cfg)).eval()
        models[L, "stress x 4"] = VLSATModel(cfg, DEV).load_state(synth.make_weights_stress(cfg, 4.0)).eval()
    for m in models.values():
        m.debug_option("pair_twins", DEFAULTS["pair_twins"])
    yield cfgs, models, main
    for m in models.values():
        m.close()


@pytest.mark.parametrize("weights", ["bench", "stress x 4"])
@pytest.mark.parametrize("route", ["persistent", "8-phase"])
@pytest.mark.parametrize("layers", [3, 1])
def test_e2_pairs_on_equals_off(setup, layers, route, weights):
    """L = 3: conv3 -> layer 1, LayerNorm + ReLU -> layers 2 and 3, LayerNorm without ReLU -> the 2D head; L = 1: conv3 -> the layer,
    LayerNorm + ReLU -> the head.  The persistent kernel takes every launch of 720 rows by default, the 8-phase kernel with
    gemm_p8_part_min = 1; the x 4 stress weights put |E2| in the thousands and lo parts into fp16's subnormal range."""
    _, models, main = setup
    options = {"gemm_p8_part_min": 1} if route == "8-phase" else {}
    _on_off(models[layers, weights], main, (layers, route, weights), **options)


def test_e2_buffer_holds_the_pair_words_of_the_fp32_forward(setup):
    """the option really changes the tensor: after a forward E2 holds what the last LayerNorm wrote -- pack(the fp32 forward's E2) with the
    option on, on both kernel routes"""
    _, models, main = setup
    m, d = models[3, "bench"], _dev(main)
    n, p = d["obj_points"].shape[0], d["obj_points"].shape[2]
    assert _decisions()["E = 720"] == "E2 pairs" and _decisions()["E = 720, gemm_p8_part_min 1"] == "E2 pairs"
    for options in ({}, {"gemm_p8_part_min": 1}):
        with _Options(m, **options):
            _run(m, d)
            on = m.debug_buffer(d["edge_indices"], d["batch_ids"], n, p, "E2").cpu().numpy()
            with _Options(m, edge_pairs_e2=0):
                _run(m, d)
                off = m.debug_buffer(d["edge_indices"], d["batch_ids"], n, p, "E2").cpu().numpy()
        assert np.isfinite(off).all() and off.shape == (720, 512)
        assert (on.view(np.uint32) == P.pack(off)).all(), options
        assert (on.view(np.uint32) != off.view(np.uint32)).any()


def test_e2_pairs_mixed_scenes_and_edgeless(setup):
    """scenes of 5, 1 and 7 objects (E = 62: every launch is small enough for the split-K kernel, nothing pairs), the same with split-K off
    (the persistent kernel on one cut tile: E2 pairs), and a batch without edges"""
    _, models, _ = setup
    mixed = synth.collate([synth.make_scene(n, 64, 7600 + j) for j, n in enumerate((5, 1, 7))])
    assert _decisions()["scenes of 5, 1 and 7 objects (E = 62)"].startswith("E2 fp32 (")
    _on_off(models[3, "bench"], mixed, "5 | 1 | 7")
    _on_off(models[3, "bench"], mixed, "5 | 1 | 7, no split-K", gemm_splitk=0)
    _on_off(models[1, "stress x 4"], mixed, "5 | 1 | 7, no split-K, 8-phase", gemm_splitk=0, gemm_p8_part_min=1)
    single = synth.collate([synth.make_scene(1, 64, 7700), synth.make_scene(1, 64, 7701)])
    got = _on_off(models[3, "bench"], single, "E = 0")
    assert got[2].shape[0] == 0


def test_e2_pairs_paired_schedule(setup):
    """the paired schedule (twin launches of two problems: a one-scene plan, and the three scenes of the main batch, by default): nothing
    pairs, E2 is the fp32 tensor after the forward, nothing changes; a one-scene plan with pair_twins 0 is split-K launches: the same"""
    _, models, main = setup
    m = models[3, "bench"]
    one = synth.collate([synth.make_scene(9, 64, 7800)])
    assert "paired schedule" in _decisions()["one scene of 9 objects, paired schedule"]
    _on_off(m, one, "one scene", pair_twins=1)
    paired = _on_off(m, main, "three scenes, paired schedule", pair_twins=1)
    _same(paired, _run(m, _dev(main)), "paired schedule against pair_twins 0")
    d = _dev(main)
    n, p = d["obj_points"].shape[0], d["obj_points"].shape[2]
    with _Options(m, pair_twins=1):
        _run(m, d)
        e2 = m.debug_buffer(d["edge_indices"], d["batch_ids"], n, p, "E2").cpu()
        with _Options(m, edge_pairs_e2=0):
            _run(m, d)
            assert torch.equal(e2, m.debug_buffer(d["edge_indices"], d["batch_ids"], n, p, "E2").cpu()) and torch.isfinite(e2).all()
    _on_off(m, one, "one scene, pair_twins 0")
    _on_off(m, one, "one scene, pair_twins 0, no split-K", gemm_splitk=0)


def test_e2_pairs_3d_only_forward(setup):
    """forward_3d: no 2D branch, E2 is never written or read -- the 3D outputs equal those of the full forward either way"""
    _, models, main = setup
    m, d = models[3, "bench"], _dev(main)
    full = _run(m, d)

    def run3d(m, d):
        out = m.forward_3d(d["obj_points"], d["edge_indices"], d["descriptor"], d["batch_ids"])
        torch.cuda.synchronize()
        return [o.clone().cpu() for o in out]
    got = _on_off(m, main, "forward_3d", run=run3d)
    assert len(got) == 2 and torch.equal(got[0], full[0]) and torch.equal(got[1], full[2])


def test_e2_pairs_debug_stop(setup):
    """a debug stop refuses the pair form (the caller may read E2): the tap after the first layer's edge attention is the fp32 tensor with
    the option on and off, and after the stop is lifted the forward is the paired one again"""
    _, models, main = setup
    m, d = models[3, "bench"], _dev(main)
    n, p = d["obj_points"].shape[0], d["obj_points"].shape[2]
    assert "debug stop" in _decisions()["bench batch, debug stop"]
    ref = _run(m, d)
    taps = {}
    for stage in (3, 13, 14):               # E2 of conv3, of nn_edge.2 and of the LayerNorm
        for on in (1, 0):
            with _Options(m, edge_pairs_e2=on):
                m.debug_stop_after(stage)
                try:
                    m(*_args(d))
                    taps[stage, on] = m.debug_buffer(d["edge_indices"], d["batch_ids"], n, p, "E2").cpu()
                finally:
                    m.debug_stop_after(-1)
        assert torch.isfinite(taps[stage, 1]).all() and torch.equal(taps[stage, 1], taps[stage, 0]), stage
    assert float(taps[14, 1].min()) == 0.0 and float(taps[14, 1].max()) > 0.1          # (LayerNorm + ReLU of plain fp32 values)
    _same(_run(m, d), ref, "after the stops")


def test_e2_pairs_training_outputs_and_feature_transform():
    """forward(istrain=True) reads E2 in triplet_projector_2d, feature_transform copies E2 out of the encoder's fp32 rows: E2 stays fp32
    (the decision says so) and all outputs, the training extras included, are those of the option off"""
    from vlsat_amd.model import VLSATModel
    dec = _decisions()
    assert "training outputs" in dec["bench batch, training outputs"] and "feature_transform" in dec["bench batch, feature_transform"]
    main = synth.collate([synth.make_scene(16, 64, 7500 + j) for j in range(3)])
    for what, cfg, kw in (("training outputs", VLSATConfig(N_LAYERS=2, train_outputs=True), {"istrain": True}),
                          ("feature_transform", VLSATConfig(N_LAYERS=2, feature_transform=True), {})):
        m = VLSATModel(cfg, DEV).load_state(synth.make_weights(cfg)).eval()
        try:
            got = _on_off(m, main, what, run=lambda m, d: _run(m, d, **kw))
            assert len(got) >= 4
            if kw:                           # (the same model's plain forward pairs E2: its four outputs are the training call's first four)
                _same(_run(m, _dev(main)), got[:4], "istrain=False against istrain=True")
        finally:
            m.close()


def test_e2_pairs_exact_kernel_options(setup):
    """gemm_exact / gemm_small_exact (a part of every launch on an exact kernel: the decision reports E2 as fp32) and flash_exact (the
    attention only: E2 still pairs), one at a time: the forward runs and equals the option off"""
    _, models, main = setup
    dec = _decisions()
    for opt, pairs in (("gemm_exact", False), ("gemm_small_exact", False), ("flash_exact", True)):
        assert (dec[f"E = 720, {opt} 1"] == "E2 pairs") == pairs and (pairs or "exact" in dec[f"E = 720, {opt} 1"]), opt
        _on_off(models[3, "bench"], main, opt, **{opt: 1})
        _on_off(models[3, "bench"], main, opt + ", 8-phase", gemm_p8_part_min=1, **{opt: 1})


def test_e2_pairs_schedules_and_second_forward(setup):
    """one stream, fork / join and the dependency-exact schedule: the same launches on the same operands; a second forward on the same
    plan starts from buffers that hold the first one's pair words"""
    _, models, main = setup
    m, d = models[3, "bench"], _dev(main)
    ref = None
    for options in ({"dual_stream": 0}, {"sched": 0}, {"sched": 1}, {}):
        with _Options(m, **options):
            got = _run(m, d)
            got2 = _run(m, d)
        _same(got2, got, (options, "second forward"))
        if ref is None:
            ref = got
        _same(got, ref, options)


def test_e2_pairs_vs_cpu_oracle(setup):
    cfgs, models, main = setup
    from oracle import vlsat_oracle as O
    c = {k: torch.from_numpy(v) for k, v in main.items()}
    ref = O.forward(O.to_torch(synth.make_weights(cfgs[3]), torch.float32), cfgs[3], c["obj_points"], c["obj_2d_feats"], c["edge_indices"],
                    c["descriptor"], c["batch_ids"])
    got = _run(models[3, "bench"], _dev(main))
    for n, a, r in zip(NAMES, got, ref):
        err = float((a - torch.as_tensor(r).float()).abs().max())
        print(f"{n}: {err:.2e}")
        assert err <= TIGHT, (n, err)
