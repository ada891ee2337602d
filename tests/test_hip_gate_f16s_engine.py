"""The fp32 forward with the edge gate on the split-fp16 kernel (the default; csrc/edge_gate_f16s.hip) next to the same model with
"gate_exact" = 1 (the exact fp32-MFMA gate, as before): both against the CPU oracle, the default against itself under every form of the
gate launch (row maps, fused and separate aggregation, twin launch, schedules, a second forward, a replica), the x 4 stress weights, and
the 16-bit modes, which the option does not reach.  Needs an MI355X:  pytest -m gpu"""
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import VLSATConfig, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("obj3d", "obj2d", "rel3d", "rel2d")
TIGHT = 1e-4          # the bound of test_hip_fp32_small_f16s_engine.py


def _dev(b):
    return {k: torch.from_numpy(v).to(DEV) for k, v in b.items()}


def _run(m, d):
    out = m(d["obj_points"], d["obj_2d_feats"], d["edge_indices"], d["descriptor"], d["batch_ids"])
    torch.cuda.synchronize()
    return [o.clone().cpu() for o in out]


def _oracle(cfg, w, b, dtype=torch.float32):
    from oracle import vlsat_oracle as O
    c = {k: torch.from_numpy(v) for k, v in b.items()}
    f = (lambda t: t.to(dtype)) if dtype != torch.float32 else (lambda t: t)
    return O.forward(O.to_torch(w, dtype), cfg, f(c["obj_points"]), f(c["obj_2d_feats"]), c["edge_indices"], f(c["descriptor"]), c["batch_ids"])


def _same(got, ref, what):
    for n, a, c in zip(NAMES, got, ref):
        assert a.shape == c.shape and torch.isfinite(a).all(), (what, n)
        assert torch.equal(a, c), (what, n, float((a - c).abs().max()) if a.numel() else 0.0)


@pytest.fixture(scope="module")
def setup():
    from vlsat_amd.model import VLSATModel
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path cannot run and there is no fallback")
    cfg = VLSATConfig(N_LAYERS=2)
    w = synth.make_weights(cfg)
    batches = [("ragged 9 | 14 | 5 | 23", synth.collate([synth.make_scene(n, 64, 8100 + j) for j, n in enumerate((9, 14, 5, 23))])),
               ("3 x 16", synth.collate([synth.make_scene(16, 64, 8200 + j) for j in range(3)])),
               ("5 | 1 | 7", synth.collate([synth.make_scene(n, 64, 8300 + j) for j, n in enumerate((5, 1, 7))])),
               ("E = 0", synth.collate([synth.make_scene(1, 64, 8400), synth.make_scene(1, 64, 8401)]))]
    refs = {name: [torch.as_tensor(r).float() for r in _oracle(cfg, w, b)] for name, b in batches}       # computed once, shared, never changed
    new = VLSATModel(cfg, DEV).load_state(w).eval()
    exact = VLSATModel(cfg, DEV).load_state(w).eval().debug_option("gate_exact", 1)
    yield cfg, w, batches, refs, new, exact
    new.close()
    exact.close()


def test_engine_default_and_gate_exact_vs_oracle(setup):
    """both within 1e-4 of the CPU oracle on every output; they differ wherever there are edges: the option governs a kernel that runs"""
    cfg, _, batches, refs, new, exact = setup
    for name, b in batches:
        d = _dev(b)
        got_new, got_exact = _run(new, d), _run(exact, d)
        same = True
        for n, a, e, r in zip(NAMES, got_new, got_exact, refs[name]):
            assert torch.isfinite(a).all() and torch.isfinite(e).all(), (name, n)
            ea, ee = (float((x - r).abs().max()) if x.numel() else 0.0 for x in (a, e))
            print(f"{name} {n}: default {ea:.2e}, gate_exact {ee:.2e}")
            assert ea <= TIGHT and ee <= TIGHT, (name, n, ea, ee)
            same = same and torch.equal(a, e)
        if b["edge_indices"].shape[0] * b["edge_indices"].shape[1] > 0:
            assert not same, (name, "the default equals gate_exact = 1 bit for bit: the split-fp16 gate never ran")
        else:
            assert same, name


def test_engine_every_form_of_the_gate_launch_gives_the_same_bits(setup):
    """With the default kernel: both row maps, the aggregation fused and separate, the twin launch of a one-scene plan and its single
    launches, the three schedules, one stream, a second forward on the same plan and a replica -- a row's bits depend on the row alone."""
    from vlsat_amd.model import VLSATModel
    cfg, w, batches, _, new, _ = setup
    one = ("one scene of 9", synth.collate([synth.make_scene(9, 64, 8500)]))
    defaults = {"gate_row_map": 1, "gate_fuse_agg": 1, "pair_twins": 1, "sched": -1, "dual_stream": 2}
    m = VLSATModel(cfg, DEV).load_state(w).eval()
    replica = new.replicate()
    try:
        for name, b in batches + [one]:
            d = _dev(b)
            ref = _run(new, d)
            _same(_run(new, d), ref, (name, "second forward"))
            _same(_run(replica, d), ref, (name, "replica"))
            for opts in ({"gate_row_map": 0}, {"gate_fuse_agg": 0}, {"gate_fuse_agg": 2}, {"gate_fuse_agg": 2, "gate_row_map": 0},
                         {"pair_twins": 0}, {"pair_twins": 0, "gate_fuse_agg": 2}, {"sched": 0}, {"sched": 1}, {"dual_stream": 0},
                         {"dual_stream": 0, "gate_fuse_agg": 2}):
                for k, v in opts.items():
                    m.debug_option(k, v)
                try:
                    _same(_run(m, d), ref, (name, opts))
                finally:
                    for k in opts:
                        m.debug_option(k, defaults[k])
    finally:
        m.close()
        replica.close()


def test_engine_gate_grid_is_a_lab_switch_of_the_experiments_build(setup):
    """"gate_grid" sizes the persistent grid of the gate kernels.  Where the library accepts it (build.py --experiments) two grid sizes must
    give the default's bits; the release library answers it with VLSAT_EINVAL (tests/test_host_cpu.py pins that), and there the
    independence of a row from the block that owns it is what tests/test_hip_gate_f16s.py shows at kernel level (a list moved by five
    edges) and the twin / single and row-map comparisons above show in the engine."""
    from vlsat_amd import lib as L
    from vlsat_amd.model import VLSATModel
    cfg, w, batches, _, new, _ = setup
    name, b = batches[0]
    d = _dev(b)
    ref = _run(new, d)
    m = VLSATModel(cfg, DEV).load_state(w).eval()
    try:
        for grid in (3, 41):
            try:
                m.debug_option("gate_grid", grid)
            except L.VlsatError as e:
                assert e.code == -1 and "lab switch" in str(e), e
                return
            _same(_run(m, d), ref, (name, "gate_grid", grid))
    finally:
        m.close()


def test_engine_stress_x4_weights_stay_finite(setup):
    """the x 4 stress weights (|kproj| and |hidden| in the thousands, tools/f16s_domain.py): finite outputs with both gates -- the check
    tests/test_hip_edge_pairs.py makes on them -- and the gate's contribution printed next to both errors against the fp64 oracle"""
    from vlsat_amd.model import VLSATModel
    cfg, _, batches, _, _, _ = setup
    w = synth.make_weights_stress(cfg, 4.0)
    name, b = batches[1]
    d = _dev(b)
    ref = [torch.as_tensor(r) for r in _oracle(cfg, w, b, torch.float64)]
    new = VLSATModel(cfg, DEV).load_state(w).eval()
    exact = VLSATModel(cfg, DEV).load_state(w).eval().debug_option("gate_exact", 1)
    try:
        got_new, got_exact = _run(new, d), _run(exact, d)
        for n, a, e, r in zip(NAMES, got_new, got_exact, ref):
            assert torch.isfinite(a).all() and torch.isfinite(e).all(), n
            scale = max(1.0, float(r.abs().max()))
            print(f"stress x 4 {n}: max |ref| {scale:.3g}; default {float((a.double() - r).abs().max()):.2e}, gate_exact "
                  f"{float((e.double() - r).abs().max()):.2e}, default against gate_exact {float((a - e).abs().max()):.2e}")
        assert not all(torch.equal(a, e) for a, e in zip(got_new, got_exact))
    finally:
        new.close()
        exact.close()


@pytest.mark.parametrize("mode", ["bf16_mixed", "bf16x3"])
def test_engine_gate_exact_does_not_reach_the_16_bit_modes(setup, mode):
    from vlsat_amd.model import VLSATModel
    cfg, w, batches, _, _, _ = setup
    name, b = batches[0]
    d = _dev(b)
    m = VLSATModel(cfg, DEV).load_state(w).eval().set_gemm_precision(mode)
    try:
        ref = _run(m, d)
        m.debug_option("gate_exact", 1)
        _same(_run(m, d), ref, (mode, "gate_exact 1"))
        m.debug_option("gate_exact", -1)
        _same(_run(m, d), ref, (mode, "gate_exact -1"))
    finally:
        m.close()
