"""The split-fp16 edge attention of the fp32 precision mode (flash_attn_f16x3_kernel: fp32 tensors, every product as three f16 MFMAs)
through its kernel-level entry, next to the exact fp32-MFMA kernel on the same inputs, both against an fp64 softmax; and the engine's
fp32 forward with the new default and with "flash_exact" = 1.  Head dim 64, 8 heads.  Needs an MI355X:  pytest -m gpu

Shapes: the smallest at which the kernel takes another path -- one token; 63 / 64 / 65 tokens (the 64-key tile's edge); 129 (the
128-query tile's edge: a second block with one live row); two scenes of 200 and 37 tokens in one launch; split keys (300 tokens in two
parts with the boundary inside a 64-key tile; 65 tokens in five parts of its three 32-key tiles, where one part is empty and another
has a single 64-key tile that is masked throughout, so its running maximum stays -inf).

Bounds: at unit scale the project's own bound for the exact kernel, 2e-5 absolute (5e-5 for the forced rescale,
test_hip_kernels.py); with K and V scaled by 2^-8 and 2^4, error over max |ref| at most 4 x the exact kernel's on the same inputs (the
ratio of the unit roundoffs, 2^-22 / 2^-24)."""
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import VLSATConfig, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("obj3d", "obj2d", "rel3d", "rel2d")
TIGHT = 1e-4


@pytest.fixture(scope="module")
def lib():
    from vlsat_amd import lib as L
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path cannot run and there is no fallback")
    return L


def _x3(L, q, k, v, tok_ptr, scale, parts=1, use_tr=1):
    o = torch.full_like(q, float("nan"))
    tp = torch.tensor(tok_ptr, dtype=torch.int64)
    L.check(L.load().vlsat_k_flash_attn_f16x3(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), q.stride(0), tp.data_ptr(),
                                              len(tok_ptr) - 1, 8, scale, parts, use_tr, L.stream_ptr()))
    torch.cuda.synchronize()
    return o.cpu()


def _exact(L, q, k, v, tok_ptr, scale):
    o = torch.full_like(q, float("nan"))
    tp = torch.tensor(tok_ptr, dtype=torch.int64)
    L.check(L.load().vlsat_k_flash_attn(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), q.stride(0), tp.data_ptr(),
                                        len(tok_ptr) - 1, 8, scale, L.stream_ptr()))
    torch.cuda.synchronize()
    return o.cpu()


def _ref(q, k, v, tok_ptr, scale):
    q, k, v = q.double().cpu(), k.double().cpu(), v.double().cpu()
    out = torch.zeros_like(q)
    for s in range(len(tok_ptr) - 1):
        a, b = tok_ptr[s], tok_ptr[s + 1]
        qq = q[a:b].view(b - a, 8, 64).permute(1, 0, 2)
        kk = k[a:b].view(b - a, 8, 64).permute(1, 2, 0)
        vv = v[a:b].view(b - a, 8, 64).permute(1, 0, 2)
        out[a:b] = (torch.softmax(qq @ kk * scale, -1) @ vv).permute(1, 0, 2).reshape(b - a, 512)
    return out


def _inputs(tok_ptr, kv_scale=1.0):
    g = torch.Generator().manual_seed(sum(tok_ptr) + 17)
    T = tok_ptr[-1]
    q, k, v = (torch.randn(T, 512, generator=g) for _ in range(3))
    v = v * 3 + torch.arange(512)[None, :] * 0.01                  # column-asymmetric values: a transposed or shifted V fragment shows
    return q.to(DEV), (k * kv_scale).to(DEV), (v * kv_scale).to(DEV)


SHAPES = [[0, 1], [0, 63], [0, 64], [0, 65], [0, 129], [0, 200, 237]]


@pytest.mark.parametrize("tok_ptr", SHAPES)
def test_f16x3_vs_softmax_unit_scale(lib, tok_ptr):
    q, k, v = _inputs(tok_ptr)
    ref = _ref(q, k, v, tok_ptr, 0.125)
    tr = _x3(lib, q, k, v, tok_ptr, 0.125, 1, 1)
    ga = _x3(lib, q, k, v, tok_ptr, 0.125, 1, 0)
    ex = _exact(lib, q, k, v, tok_ptr, 0.125)
    assert torch.isfinite(tr).all() and torch.isfinite(ga).all()
    err, err_ex = float((tr.double() - ref).abs().max()), float((ex.double() - ref).abs().max())
    print(f"{tok_ptr}: split-fp16 {err:.2e}, exact {err_ex:.2e}")
    assert err_ex < 2e-5, f"exact {tok_ptr}: {err_ex:.3e}"
    assert err < 2e-5, f"split-fp16 {tok_ptr}: {err:.3e}"
    assert torch.equal(tr, ga), f"transpose-read path differs from the gather path by {float((tr - ga).abs().max()):.3e}"


@pytest.mark.parametrize("log2_scale", [-8, 4])
@pytest.mark.parametrize("tok_ptr", [[0, 129], [0, 200, 237]])
def test_f16x3_scaled_operands_within_4x_of_exact(lib, tok_ptr, log2_scale):
    """K and V times 2^-8 (without the kernel's factor on V their lo planes would be subnormal fp16 throughout: the case that decided
    the pre-scale) and 2^4 (scores of tens: a peaked softmax)."""
    q, k, v = _inputs(tok_ptr, 2.0 ** log2_scale)
    ref = _ref(q, k, v, tok_ptr, 0.125)
    den = float(ref.abs().max())
    tr = _x3(lib, q, k, v, tok_ptr, 0.125, 1, 1)
    ex = _exact(lib, q, k, v, tok_ptr, 0.125)
    err, err_ex = float((tr.double() - ref).abs().max()) / den, float((ex.double() - ref).abs().max()) / den
    print(f"{tok_ptr} x 2^{log2_scale}: split-fp16 {err:.2e}, exact {err_ex:.2e} ({err / err_ex:.2f} x) of max |ref| {den:.2e}")
    assert torch.isfinite(tr).all()
    assert err <= 4 * err_ex, (err, err_ex)
    assert torch.equal(tr, _x3(lib, q, k, v, tok_ptr, 0.125, 1, 0))


@pytest.mark.parametrize("tok_ptr,parts", [([0, 300], 2), ([0, 65], 5), ([0, 200, 237], 3)])
def test_f16x3_split_keys(lib, tok_ptr, parts):
    q, k, v = _inputs(tok_ptr)
    ref = _ref(q, k, v, tok_ptr, 0.125)
    tr = _x3(lib, q, k, v, tok_ptr, 0.125, parts, 1)
    err = float((tr.double() - ref).abs().max())
    print(f"{tok_ptr} in {parts} key parts: {err:.2e}")
    assert torch.isfinite(tr).all()
    assert err < 2e-5, f"{err:.3e}"
    assert torch.equal(tr, _x3(lib, q, k, v, tok_ptr, 0.125, parts, 0))


def test_f16x3_forced_rescale(lib):
    """The inputs of test_flash_attn_forced_rescale: one late key dominates one query, another query has huge logits -- scores grow
    tile by tile and the running-maximum rescale is taken."""
    g = torch.Generator().manual_seed(9)
    T = 300
    q = torch.randn(T, 512, generator=g)
    k = torch.randn(T, 512, generator=g)
    v = torch.randn(T, 512, generator=g)
    k[257] = q[5] * 4.0
    k[31] = -q[100] * 6.0
    q[200] *= 30.0
    q, k, v = q.to(DEV), k.to(DEV), v.to(DEV)
    ref = _ref(q, k, v, [0, T], 0.125)
    got, ex = _x3(lib, q, k, v, [0, T], 0.125), _exact(lib, q, k, v, [0, T], 0.125)
    err, err_ex = float((got.double() - ref).abs().max()), float((ex.double() - ref).abs().max())
    print(f"forced rescale: split-fp16 {err:.2e}, exact {err_ex:.2e}")
    assert torch.isfinite(got).all()
    assert err_ex < 5e-5 and err < 5e-5, (err, err_ex)


def test_f16x3_large_key_row_inside_the_clamp_domain(lib):
    """One K row at 3e4 (inside +-65504, where the fp16 hi part has an ulp of 16): its scores are +-thousands, so it takes the whole
    softmax of the queries it agrees with and none of the others'."""
    tok_ptr = [0, 129]
    q, k, v = _inputs(tok_ptr)
    k[77] = 3e4 * torch.sign(torch.randn(512, generator=torch.Generator().manual_seed(4))).to(DEV)
    ref = _ref(q, k, v, tok_ptr, 0.125)
    got, ex = _x3(lib, q, k, v, tok_ptr, 0.125), _exact(lib, q, k, v, tok_ptr, 0.125)
    err, err_ex = float((got.double() - ref).abs().max()), float((ex.double() - ref).abs().max())
    print(f"K row at 3e4: split-fp16 {err:.2e}, exact {err_ex:.2e}")
    assert torch.isfinite(got).all()
    # the other rows are at unit scale (2e-5, as above); where the large key competes, both kernels round scores of 1e5 in fp32, and
    # the split one may be off by the ratio of the unit roundoffs
    assert err <= max(4 * err_ex, 2e-5), (err, err_ex)


# ---- the engine: fp32 forward with the split-fp16 attention (default) and with the exact kernel ("flash_exact" 1) ----
def _dev(b):
    return {k: torch.from_numpy(v).to(DEV) for k, v in b.items()}


def _args(d):
    return (d["obj_points"], d["obj_2d_feats"], d["edge_indices"], d["descriptor"], d["batch_ids"])


def _run(m, d):
    out = m(*_args(d))
    torch.cuda.synchronize()
    return [o.clone().cpu() for o in out]


def _oracle(cfg, b):
    from oracle import vlsat_oracle as O
    c = {k: torch.from_numpy(v) for k, v in b.items()}
    return O.forward(O.to_torch(synth.make_weights(cfg), torch.float32), cfg, c["obj_points"], c["obj_2d_feats"], c["edge_indices"],
                     c["descriptor"], c["batch_ids"])


def _batches():
    import plan_cases
    out = [(name, synth.collate([synth.make_scene(n, plan_cases.POINTS, 8800 + 10 * i + j) for j, n in enumerate(sizes)]))
           for i, (name, sizes, _) in enumerate(plan_cases.CASES)]
    out.append(("two scenes of 9 and 40 nodes", synth.collate([synth.make_scene(9, 32, 8900), synth.make_scene(40, 32, 8901)])))
    return out


@pytest.fixture(scope="module")
def models():
    from vlsat_amd.model import VLSATModel
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path cannot run and there is no fallback")
    cfg = VLSATConfig()
    w = synth.make_weights(cfg)
    new = VLSATModel(cfg, DEV).load_state(w).eval()
    exact = VLSATModel(cfg, DEV).load_state(w).eval().debug_option("flash_exact", 1)
    yield cfg, w, new, exact
    new.close()
    exact.close()


def test_engine_fp32_default_and_flash_exact_vs_oracle(models):
    cfg, _, new, exact = models
    for name, b in _batches():
        d = _dev(b)
        ref = _oracle(cfg, b)
        got_new, got_exact = _run(new, d), _run(exact, d)
        for n, a, e, r in zip(NAMES, got_new, got_exact, ref):
            r = torch.as_tensor(r).float()
            assert torch.isfinite(a).all() and torch.isfinite(e).all(), (name, n)
            ea, ee = (float((x - r).abs().max()) if x.numel() else 0.0 for x in (a, e))
            print(f"{name} {n}: split-fp16 {ea:.2e}, flash_exact {ee:.2e}")
            assert ea <= TIGHT and ee <= TIGHT, (name, n, ea, ee)
            if n in ("obj3d", "rel3d"):          # the 3D outputs never read the edge cross-attention
                assert torch.equal(a, e), (name, n, float((a - e).abs().max()))


def test_engine_schedules_are_bit_identical_under_the_new_default(models):
    """Replica, one stream, the two two-stream schedules, the paired schedule off, and set_batch_mode('reference') against itself on
    one stream: the same kernels on the same data, so every output equals the one-stream forward's bit for bit."""
    from vlsat_amd.model import VLSATModel
    cfg, w, new, _ = models
    single = VLSATModel(cfg, DEV).load_state(w).eval().debug_option("dual_stream", 0)
    variants = {"replica": new.replicate(), "sched 1": VLSATModel(cfg, DEV).load_state(w).eval().debug_option("sched", 1),
                "sched 0": VLSATModel(cfg, DEV).load_state(w).eval().debug_option("sched", 0),
                "pair_twins 0": VLSATModel(cfg, DEV).load_state(w).eval().debug_option("pair_twins", 0), "default": new}
    try:
        for name, b in _batches():
            d = _dev(b)
            ref = _run(single, d)
            for vn, m in variants.items():
                for n, a, c in zip(NAMES, _run(m, d), ref):
                    assert torch.equal(a, c), (name, vn, n, float((a - c).abs().max()))
        name, b = _batches()[-1]
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
