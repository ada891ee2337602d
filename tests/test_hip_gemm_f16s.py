"""The split-fp16 form of the 8-phase GEMM (gemm_p8s_kernel: fp32 tensors, every product as three f16 MFMAs; the fp32 precision mode runs
the full rounds of its large edge-row launches on it) through its kernel-level entry vlsat_k_gemm_f16s, next to the exact fp32 kernels
(vlsat_k_gemm) on the same inputs, both against an fp64 product; and the engine's fp32 forward with the new default and with
"gemm_exact" = 1.  Needs an MI355X:  pytest -m gpu

Shapes.  N in {256, 512, 1024} x K in {128, 512, 1024} (K = 128 is the shortest tile the kernel takes: four K-tiles of 32) with
M = 3 * 256 + 33 and p8_part_min = 1: a partial round of four row panels whose last one has 33 live rows -- every (additive operands,
ReLU-on-A) form the fp32 forward launches, bias on and off, output ReLU, ldc > N with a guard band.  Three shapes with one FULL round of the
chip's tiles plus two panels and 33 rows, twice: with the built-in bound the rows behind the round are a tail launch of the exact kernels
(bit-equal to vlsat_k_gemm), with p8_part_min = 1 they ride along as balanced rounds with the ragged last panel.

Bound.  On the rows the 8-phase launch covers, max |got - fp64| <= max(4 x the exact kernel's on those rows, 2^-23 max |ref|): 4 is the
ratio of the unit roundoffs (2^-22 per split operand, 2^-24 fp32), the rule of test_hip_flash_f16x3.py; the numpy emulation
(test_gemm_f16s_emulation_cpu.py) stays below 1 x."""
import math

import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import VLSATConfig, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("obj3d", "obj2d", "rel3d", "rel2d")
TIGHT = 1e-4
FORMS = [(0, 0), (0, 1), (1, 0), (6, 0), (6, 1)]          # (additive operands, ReLU-on-A): VLSAT_GEMM_P8S_VARIANTS


@pytest.fixture(scope="module")
def lib():
    from vlsat_amd import lib as L
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path cannot run and there is no fallback")
    return L


def _g1():
    return max(8, 2 * torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8) // 2


def _p8_rows(M, N, part_min):
    """Rows of the first launch when it is the 8-phase kernel's (plan_gemm, exact fp32): full rounds of G1 = one tile per CU; less than a
    round runs as a partial round from part_min tiles on; a remainder behind full rounds rides along from part_min tiles on."""
    g1 = _g1()
    nbn, full = N // 256, M // 256
    panels = full + (1 if M % 256 else 0)
    bound = part_min if part_min > 0 else g1 * 5 // 8
    rounds = full * nbn // g1
    main = rounds * g1 // nbn
    if main == 0:
        return M if panels * nbn >= bound else 0
    if main < panels and (panels - main) * nbn >= bound:
        return M
    return min(main * 256, M)


class Case:
    """One problem on the device, its fp64 reference and the exact kernels' result (made once, shared by the checks of a test)."""

    def __init__(self, L, M, N, K, add, relu_a, bias, act, pad=0, a_scale=1.0, seed=0):
        g = torch.Generator().manual_seed(1000 * N + K + 7 * add + relu_a + seed)
        self.L, self.M, self.N, self.K, self.add, self.relu_a, self.act, self.ldc = L, M, N, K, add, relu_a, act, N + pad
        self.A = (torch.randn(M, K, generator=g) * a_scale).to(DEV)
        self.W = ((torch.rand(N, K, generator=g) * 2 - 1) * math.sqrt(6.0 / (K + 512))).to(DEV)      # Xavier: about 0.05
        self.b = torch.randn(N, generator=g).to(DEV) if bias else None
        self.R = torch.randn(M, N, generator=g).to(DEV) if add == 1 else None
        if add == 6:
            self.gbuf = torch.randn(77, 2 * N, generator=g).to(DEV)
            self.gi0 = torch.randint(0, 77, (M,), generator=g, dtype=torch.int32).to(DEV)
            self.gi1 = torch.randint(0, 77, (M,), generator=g, dtype=torch.int32).to(DEV)

    def ref(self, A=None):
        A = self.A if A is None else A
        r = (torch.relu(A) if self.relu_a else A).double() @ self.W.double().t()
        if self.b is not None:
            r = r + self.b.double()
        if self.add == 1:
            r = r + 0.5 * self.R.double()
        if self.add == 6:
            r = r + self.gbuf.double()[self.gi0.long(), :self.N] + self.gbuf.double()[self.gi1.long(), self.N:]
        return (torch.relu(r) if self.act else r).cpu()

    def run(self, f16s, part_min=0, A=None):
        L, N = self.L, self.N
        A = self.A if A is None else A
        C = torch.full((self.M, self.ldc), float("nan"), device=DEV)
        six = self.add == 6
        args = [A.data_ptr(), self.K, self.W.data_ptr(), self.K, C.data_ptr(), self.ldc, self.M, N, self.K,
                self.b.data_ptr() if self.b is not None else 0, 0, self.R.data_ptr() if self.add == 1 else 0, N if self.add == 1 else 0, 0.5,
                self.gbuf.data_ptr() if six else 0, self.gi0.data_ptr() if six else 0, 2 * N if six else 0,
                self.gbuf.data_ptr() + 4 * N if six else 0, self.gi1.data_ptr() if six else 0, 2 * N if six else 0, self.relu_a, self.act]
        if f16s:
            L.check(L.load().vlsat_k_gemm_f16s(*args, part_min, L.stream_ptr()))
        else:
            L.check(L.load().vlsat_k_gemm(*args, L.stream_ptr()))
        torch.cuda.synchronize()
        C = C.cpu()
        assert bool(torch.isnan(C[:, N:]).all()), "the guard band behind the N columns was written"
        return C[:, :N]


def _check(c, got, exact, ref, rows, what):
    """The bound of the module docstring on rows [0, rows); the rows behind them are the exact kernels', bit for bit."""
    assert torch.isfinite(got).all(), what
    den = float(ref.abs().max())
    err = float((got[:rows].double() - ref[:rows]).abs().max())
    err_ex = float((exact[:rows].double() - ref[:rows]).abs().max())
    print(f"{what}: rows {rows}/{c.M}, split-fp16 {err / den:.2e}, exact {err_ex / den:.2e} of max |ref| {den:.2e} ({err / max(err_ex, 1e-300):.2f} x)")
    assert err <= max(4 * err_ex, 2.0 ** -23 * den), (what, err, err_ex, den)
    assert torch.equal(got[rows:], exact[rows:]), (what, "tail rows differ from vlsat_k_gemm")
    return err, err_ex


@pytest.mark.parametrize("add,relu_a", FORMS)
@pytest.mark.parametrize("N", [256, 512, 1024])
@pytest.mark.parametrize("K", [128, 512, 1024])
def test_f16s_partial_round_every_form(lib, N, K, add, relu_a):
    M = 3 * 256 + 33
    i = FORMS.index((add, relu_a)) + N // 256 + K // 128
    c = Case(lib, M, N, K, add, relu_a, bias=i % 2 == 0, act=1 if i % 3 == 0 else 0, pad=64 if i % 2 else 0)
    assert _p8_rows(M, N, 1) == M
    got, exact, ref = c.run(True, 1), c.run(False), c.ref()
    _check(c, got, exact, ref, M, f"N {N} K {K} add {add} relu_a {relu_a}")
    assert torch.equal(got, c.run(True, 1)), "two launches differ"
    if add == 0:                                  # the same launch stays on the exact kernels where the planner keeps it off the 8-phase kernel
        assert _p8_rows(M, N, 0) == 0 and torch.equal(c.run(True, 0), exact)


@pytest.mark.parametrize("N,K,add,relu_a", [(1024, 1024, 0, 0), (512, 512, 6, 1), (256, 128, 1, 0)])
def test_f16s_full_round_with_tail_and_with_balanced_rounds(lib, N, K, add, relu_a):
    one_round = _g1() // (N // 256) * 256            # rows of one tile per CU
    M = one_round + 2 * 256 + 33
    c = Case(lib, M, N, K, add, relu_a, bias=True, act=0, pad=32)
    exact, ref = c.run(False), c.ref()
    assert _p8_rows(M, N, 0) == one_round and _p8_rows(M, N, 1) == M
    _check(c, c.run(True, 0), exact, ref, one_round, f"N {N} K {K} add {add} relu_a {relu_a}, round + tail")
    _check(c, c.run(True, 1), exact, ref, M, f"N {N} K {K} add {add} relu_a {relu_a}, balanced rounds")


@pytest.mark.parametrize("relu_a", [0, 1])
@pytest.mark.parametrize("scale", [2.0 ** -8, 2.0 ** 4, 1000.0])
def test_f16s_scaled_activations(lib, scale, relu_a):
    """A times 2^-8 (unscaled, the fp16 lo parts of activations and Xavier weights would be subnormal: what decided the scheme), 2^4, 1000."""
    M, N, K = 3 * 256 + 33, 512, 512
    c = Case(lib, M, N, K, 0, relu_a, bias=False, act=0, a_scale=scale)
    _check(c, c.run(True, 1), c.run(False), c.ref(), M, f"A x {scale:g} relu_a {relu_a}")


def test_f16s_edge_inputs(lib):
    """+-1e5 (outside +-65504: the operand saturates, nothing becomes Inf or NaN), an all-zero A panel, -0.0 under ReLU-on-A."""
    M, N, K = 3 * 256 + 33, 512, 512
    c = Case(lib, M, N, K, 0, 0, bias=True, act=0)
    A = c.A.clone()
    A[5, 17], A[300, 400] = 1e5, -1e5
    A[256:512] = 0.0
    got = c.run(True, 1, A)
    sat = A.clamp(-65504.0, 65504.0)
    _check(c, got, c.run(False, 0, sat), c.ref(sat), M, "A with +-1e5 against the saturated operand")
    assert torch.equal(got[256:512], c.b.cpu()[None, :].expand(256, N)), "an all-zero panel must give the bias exactly"
    r = Case(lib, M, N, K, 0, 1, bias=True, act=0)
    A = r.A.clone()
    A[256:512] = -0.0
    A[700:] = -A[700:].abs()
    got = r.run(True, 1, A)
    _check(r, got, r.run(False, 0, A), r.ref(A), M, "-0.0 and negative rows under ReLU-on-A")
    assert torch.equal(got[256:512], r.b.cpu()[None, :].expand(256, N)) and torch.equal(got[700:], r.b.cpu()[None, :].expand(M - 700, N))


def test_f16s_plane_maker_matches_its_definition(lib):
    """vlsat_k_split_f16s: k = 13 - ceil(log2 max |w|); hi + lo within 2^-22 of w 2^k; the exponent of an all-zero tensor is 0."""
    import ctypes
    for n, scale in ((4099, 0.05), (257, 3e4), (64, 0.0), (1000, 2.0 ** -20)):
        w = (torch.randn(n, generator=torch.Generator().manual_seed(n)) * scale).to(DEV)
        planes = torch.zeros(2, n, dtype=torch.int16, device=DEV)
        k = ctypes.c_int32(99)
        lib.check(lib.load().vlsat_k_split_f16s(w.data_ptr(), n, planes[0].data_ptr(), planes[1].data_ptr(), ctypes.byref(k), lib.stream_ptr()))
        torch.cuda.synchronize()
        mx = float(w.abs().max())
        assert k.value == (13 - math.ceil(math.log2(mx)) if mx > 0 else 0), (k.value, mx)
        hi, lo = (p.view(torch.float16).double().cpu() for p in planes)
        x = w.double().cpu() * 2.0 ** k.value
        assert float(hi.abs().max()) <= 2.0 ** 13 and bool(((hi + lo - x).abs() <= 2.0 ** -22 * x.abs() + 2.0 ** -25).all())
        assert torch.equal(hi.half(), x.half())


# ---- the engine: fp32 forward with the split-fp16 GEMM (default) and with the exact kernels ("gemm_exact" 1) ----
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


BIG = "14 scenes of 40 nodes"          # 21 840 edge rows: 172 tiles at N = 512 (a partial round), a full round plus a tail at N = 1024


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
    exact = VLSATModel(cfg, DEV).load_state(w).eval().debug_option("gemm_exact", 1)
    yield cfg, w, new, exact
    new.close()
    exact.close()


def test_engine_fp32_default_and_gemm_exact_vs_oracle(models, batches):
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
            print(f"{name} {n}: split-fp16 GEMM {ea:.2e}, gemm_exact {ee:.2e}")
            assert ea <= TIGHT and ee <= TIGHT, (name, n, ea, ee)
            same = same and torch.equal(a, e)
        # too small for the 8-phase kernel: both settings launch the same kernels; the large batch must differ somewhere, or the new kernel never ran
        assert same == (name != BIG), (name, same)


def test_engine_schedules_are_bit_identical_under_the_new_default(models, batches):
    """Replica, one stream, the two two-stream schedules, the paired schedule off, and set_batch_mode('reference') against itself on
    one stream: the same kernels on the same data (the sibling is chosen by the launch's shape alone), so every output equals the
    one-stream forward's bit for bit."""
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
