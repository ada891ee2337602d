"""fp32 mode, "edge_pairs": Hbig, R1, the 3D chain tensor E3 and the edge attention's output Oe travel between the split-fp16 kernels as
GEMM pair words, its K | V as attention pair words (the two halves of the split operand, made once by the kernel that writes the
tensor; csrc/gemm_f16s_planes.h, csrc/edge_pairs.h).  The split depends on the
word alone, so no MFMA operand changes: every test here compares the four outputs with the option on (the default) against the option
off -- the forward of the releases before -- BIT FOR BIT.  Which tensors pair on the plans used here is pinned on the host by
tests/test_edge_pairs_cpu.py (the same eligibility function, compiled by g++).  Needs an MI355X:  pytest -m gpu"""
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import VLSATConfig, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("obj3d", "obj2d", "rel3d", "rel2d")


def _dev(b):
    return {k: torch.from_numpy(v).to(DEV) for k, v in b.items()}


def _run(m, d):
    out = m(d["obj_points"], d["obj_2d_feats"], d["edge_indices"], d["descriptor"], d["batch_ids"])
    torch.cuda.synchronize()
    return [o.clone().cpu() for o in out]


# the library's defaults of the options the tests switch (one model per weight set serves every case: an option holds until it is set back)
DEFAULTS = {"edge_pairs": 1, "gemm_p8_part_min": 0, "gemm_splitk": 1, "pair_twins": 1, "gemm_exact": -1, "gemm_small_exact": -1,
            "flash_exact": -1, "flash_split": 1, "dual_stream": 2, "sched": -1}


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
    for n, a, c in zip(NAMES, got, ref):
        assert a.shape == c.shape, (what, n)
        assert torch.isfinite(a).all(), (what, n)
        assert torch.equal(a, c), (what, n, float((a - c).abs().max()) if a.numel() else 0.0)


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path cannot run and there is no fallback")
    cfg = VLSATConfig(N_LAYERS=2)
    # 3 scenes x 16 objects x 64 points: E = 720 = two full 256-row panels and a cut one; layer 2 has a pending ReLU on E3
    main = synth.collate([synth.make_scene(16, 64, 7100 + j) for j in range(3)])
    from vlsat_amd.model import VLSATModel
    ws = {"bench": synth.make_weights(cfg), "stress x 4": synth.make_weights_stress(cfg, 4.0)}
    models = {k: VLSATModel(cfg, DEV).load_state(w).eval() for k, w in ws.items()}
    yield cfg, models, main
    for m in models.values():
        m.close()


def _on_off(cfg, m, batch, what, **options):
    d = _dev(batch)
    with _Options(m, **options):
        got = _run(m, d)
        with _Options(m, edge_pairs=0):
            ref = _run(m, d)
    _same(got, ref, what)
    return got


@pytest.mark.parametrize("weights", ["bench", "stress x 4"])
@pytest.mark.parametrize("route", ["persistent", "8-phase", "persistent, no split-K", "8-phase, no split-K"])
def test_edge_pairs_on_equals_off(setup, weights, route):
    """Hbig, E3, K | V (and Oe where the plan does not split its keys) pair on both routes, R1 of the 3D head once the relation head's
    second Linear (48 tiles) is kept off the split-K kernel: the 8-phase
    kernel takes the launches with gemm_p8_part_min = 1, the persistent kernel without; the x 4 stress weights put |A| in the thousands
    and lo parts into fp16's subnormal range."""
    cfg, ws, main = setup
    options = {}
    if route.startswith("8-phase"):
        options["gemm_p8_part_min"] = 1
    if route.endswith("no split-K"):
        options["gemm_splitk"] = 0
    _on_off(cfg, ws[weights], main, (weights, route), **options)


def test_edge_pairs_mixed_scenes_and_edgeless(setup):
    """scenes of 5, 1 and 7 objects (E = 62: every launch is small enough for the split-K kernel, so nothing pairs and nothing may change
    or fault), the same with split-K off (the persistent kernel: everything pairs, on 62 rows = one cut tile), and a batch without edges"""
    cfg, ws, _ = setup
    mixed = synth.collate([synth.make_scene(n, 64, 7200 + j) for j, n in enumerate((5, 1, 7))])
    _on_off(cfg, ws["bench"], mixed, "5 | 1 | 7")
    _on_off(cfg, ws["bench"], mixed, "5 | 1 | 7, no split-K", gemm_splitk=0)
    _on_off(cfg, ws["stress x 4"], mixed, "5 | 1 | 7, no split-K, 8-phase", gemm_splitk=0, gemm_p8_part_min=1)
    single = synth.collate([synth.make_scene(1, 64, 7300), synth.make_scene(1, 64, 7301)])
    got = _on_off(cfg, ws["bench"], single, "E = 0")
    assert got[2].shape[0] == 0


def test_edge_pairs_ineligible_plans_and_options(setup):
    """a one-scene plan (the paired schedule: twin launches, nothing pairs), the same with pair_twins = 0 (split-K: nothing pairs), the exact
    kernels (gemm_exact / gemm_small_exact: nothing pairs; flash_exact: K | V and Oe stay fp32, the GEMM tensors pair), and the split-key
    attention off (one key part: Oe leaves the attention as pair words, on a last query tile with idle waves) and on (Oe stays fp32 where
    the plan splits its keys, K | V pair either way)"""
    cfg, ws, main = setup
    one = synth.collate([synth.make_scene(9, 64, 7400)])
    _on_off(cfg, ws["bench"], one, "one scene")
    _on_off(cfg, ws["bench"], one, "one scene, pair_twins 0", pair_twins=0)
    _on_off(cfg, ws["bench"], one, "one scene, pair_twins 0, no split-K", pair_twins=0, gemm_splitk=0)
    for opt in ("gemm_exact", "gemm_small_exact", "flash_exact"):
        _on_off(cfg, ws["bench"], main, opt, **{opt: 1})
    _on_off(cfg, ws["bench"], main, "flash_split 0", flash_split=0)
    _on_off(cfg, ws["bench"], main, "flash_split 1", flash_split=1)


def test_edge_pairs_3d_only_forward(setup):
    """forward_3d: no 2D branch, no edge attention -- E3 still pairs for nn_edge.0, proj_edge and the relation head"""
    cfg, ws, main = setup
    d = _dev(main)
    m = ws["bench"]
    full = _run(m, d)
    for options in ({}, {"gemm_p8_part_min": 1, "gemm_splitk": 0}):
        with _Options(m, **options):
            got = [o.clone() for o in m.forward_3d(d["obj_points"], d["edge_indices"], d["descriptor"], d["batch_ids"])]
            with _Options(m, edge_pairs=0):
                ref = m.forward_3d(d["obj_points"], d["edge_indices"], d["descriptor"], d["batch_ids"])
            torch.cuda.synchronize()
            assert len(got) == len(ref) == 2
            for a, c in zip(got, ref):
                assert torch.isfinite(a).all() and torch.equal(a.cpu(), c.cpu()), options
        if not options:                             # (the 3D outputs of the full forward, as the 3D-only forward promises)
            assert torch.equal(got[0].cpu(), full[0]) and torch.equal(got[1].cpu(), full[2])


def test_edge_pairs_schedules_are_bit_identical(setup):
    """one stream, fork / join and the dependency-exact schedule with the option on: the same launches on the same operands"""
    cfg, ws, main = setup
    d = _dev(main)
    ref = None
    m = ws["bench"]
    for options in ({"dual_stream": 0}, {"sched": 0}, {"sched": 1}, {}):
        with _Options(m, **options):
            got = _run(m, d)
            got2 = _run(m, d)                       # (a second forward on the same plan: the formats of the buffers left by the first)
        _same(got2, got, (options, "second forward"))
        if ref is None:
            ref = got
        _same(got, ref, options)
