"""The fp32 forward with the split-fp16 PointNet and the split-fp16 siblings of the persistent GEMM kernel (the default) next to the same
model with "gemm_small_exact" = 1 and "pointnet_exact" = 1 (those launches on the exact fp32-MFMA kernels, as before): both against the CPU
oracle, and the default against itself under every schedule.  Needs an MI355X:  pytest -m gpu"""
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import VLSATConfig, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("obj3d", "obj2d", "rel3d", "rel2d")
TIGHT = 1e-4
BIG = "14 scenes of 40 nodes"


def _dev(b):
    return {k: torch.from_numpy(v).to(DEV) for k, v in b.items()}


def _run(m, d):
    out = m(d["obj_points"], d["obj_2d_feats"], d["edge_indices"], d["descriptor"], d["batch_ids"])
    torch.cuda.synchronize()
    return [o.clone().cpu() for o in out]


def _oracle(cfg, b):
    from oracle import vlsat_oracle as O
    c = {k: torch.from_numpy(v) for k, v in b.items()}
    return O.forward(O.to_torch(synth.make_weights(cfg), torch.float32), cfg, c["obj_points"], c["obj_2d_feats"], c["edge_indices"],
                     c["descriptor"], c["batch_ids"])


@pytest.fixture(scope="module")
def batches():
    import plan_cases
    out = [(name, synth.collate([synth.make_scene(n, plan_cases.POINTS, 9300 + 10 * i + j) for j, n in enumerate(sizes)]))
           for i, (name, sizes, _) in enumerate(plan_cases.CASES)]
    out.append((BIG, synth.collate([synth.make_scene(40, 32, 9400 + j) for j in range(14)])))
    return out


@pytest.fixture(scope="module")
def models():
    from vlsat_amd.model import VLSATModel
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path cannot run and there is no fallback")
    cfg = VLSATConfig()
    w = synth.make_weights(cfg)
    new = VLSATModel(cfg, DEV).load_state(w).eval()
    exact = VLSATModel(cfg, DEV).load_state(w).eval().debug_option("gemm_small_exact", 1).debug_option("pointnet_exact", 1)
    yield cfg, w, new, exact
    new.close()
    exact.close()


def test_engine_fp32_default_and_small_exact_vs_oracle(models, batches):
    cfg, _, new, exact = models
    for name, b in batches:
        d = _dev(b)
        ref = _oracle(cfg, b)
        got_new, got_exact = _run(new, d), _run(exact, d)
        same = True
        for n, a, e, r in zip(NAMES, got_new, got_exact, ref):
            r = torch.as_tensor(r).float()
            assert torch.isfinite(a).all() and torch.isfinite(e).all(), (name, n)
            ea, ee = (float((x - r).abs().max()) if x.numel() else 0.0 for x in (a, e))
            print(f"{name} {n}: default {ea:.2e}, gemm_small_exact + pointnet_exact {ee:.2e}")
            assert ea <= TIGHT and ee <= TIGHT, (name, n, ea, ee)
            same = same and torch.equal(a, e)
        assert not same, (name, "the default equals the exact setting bit for bit: the new kernels never ran")


def test_engine_each_option_alone_changes_the_result(models, batches):
    """"pointnet_exact" and "gemm_small_exact" each govern kernels that run: switching one on alone moves the outputs of the large batch
    away from the default's and from the other's"""
    from vlsat_amd.model import VLSATModel
    cfg, w, new, exact = models
    name, b = batches[-1]
    d = _dev(b)
    base, both = _run(new, d), _run(exact, d)
    for opt in ("pointnet_exact", "gemm_small_exact"):
        m = VLSATModel(cfg, DEV).load_state(w).eval().debug_option(opt, 1)
        try:
            got = _run(m, d)
            assert not all(torch.equal(a, c) for a, c in zip(got, base)), opt
            assert not all(torch.equal(a, c) for a, c in zip(got, both)), opt
        finally:
            m.close()


def test_engine_schedules_are_bit_identical_under_the_new_default(models, batches):
    """Replica, one stream, the two two-stream schedules, the paired schedule off, and set_batch_mode('reference') across those variants:
    the same kernels on the same data (a sibling is chosen by the launch's shape and flags alone), so every output equals the one-stream
    forward's bit for bit."""
    from vlsat_amd.model import VLSATModel
    cfg, w, new, _ = models
    single = VLSATModel(cfg, DEV).load_state(w).eval().debug_option("dual_stream", 0)
    variants = {"replica": new.replicate(), "sched 1": VLSATModel(cfg, DEV).load_state(w).eval().debug_option("sched", 1),
                "sched 0": VLSATModel(cfg, DEV).load_state(w).eval().debug_option("sched", 0),
                "pair_twins 0": VLSATModel(cfg, DEV).load_state(w).eval().debug_option("pair_twins", 0), "default": new}
    try:
        for name, b in batches:
            d = _dev(b)
            ref = _run(single, d)
            for vn, m in variants.items():
                for n, a, c in zip(NAMES, _run(m, d), ref):
                    assert torch.equal(a, c), (name, vn, n, float((a - c).abs().max()))
        name, b = batches[-2]
        d = _dev(b)
        single.set_batch_mode("reference")
        ref = _run(single, d)
        for vn, m in variants.items():
            m.set_batch_mode("reference")
            got = _run(m, d)
            m.set_batch_mode("per_scene")
            for n, a, c in zip(NAMES, got, ref):
                assert torch.isfinite(a).all()
                assert torch.equal(a, c), (name, vn, "reference batch mode", n, float((a - c).abs().max()))
    finally:
        single.close()
        for vn, m in variants.items():
            if vn != "default":
                m.close()
