"""The split-fp16 siblings of the persistent GEMM kernel (gemm_f16s_kernel: fp32 tensors in and out, every product as three f16 MFMAs; the
fp32 precision mode runs tails, small launches and node rows on them) through vlsat_k_gemm_f16s(..., -1), next to the exact fp32 kernels
(vlsat_k_gemm) on the same inputs, both against an fp64 product.  Problems are built by test_hip_gemm_f16s.Case (Xavier weights, bias on
and off, output ReLU, ldc > N with a NaN guard band).  Needs an MI355X:  pytest -m gpu

Shapes: tests/gemm_f16s_tiled_shapes.py -- all on the persistent kernel, every one of its five tiles, ragged last tiles, main launch plus
tail; tests/test_gemm_f16s_tiled_shapes_cpu.py holds the list against the planner.  Forms: (additive operands, ReLU-on-A) in
{(0,0), (0,1), (1,0), (6,0), (6,1)}.

Bound, the rule of test_hip_gemm_f16s.py and test_hip_flash_f16x3.py: on all rows, max |got - fp64| <= max(4 x the exact kernel's error
on the same rows, 2^-23 max |ref|) -- 4 is the ratio of the unit roundoffs (2^-22 per split operand, 2^-24 fp32)."""
import pytest
import torch

import vlsat_amd  # noqa: F401
import test_hip_gemm_f16s as P8
from gemm_f16s_tiled_shapes import FORMS, SHAPES

pytestmark = pytest.mark.gpu
TILED = -1                # p8_part_min of vlsat_k_gemm_f16s: f16s = 2, the built-in bound of the 8-phase kernel


@pytest.fixture(scope="module")
def lib():
    from vlsat_amd import lib as L
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path cannot run and there is no fallback")
    return L


def _check(c, got, exact, ref, what):
    """the bound of the module docstring on all rows -> (error, the exact kernel's error)"""
    assert torch.isfinite(got).all(), what
    den = float(ref.abs().max())
    err, err_ex = float((got.double() - ref).abs().max()), float((exact.double() - ref).abs().max())
    print(f"{what}: split-fp16 {err / den:.2e}, exact {err_ex / den:.2e} of max |ref| {den:.2e} ({err / max(err_ex, 1e-300):.2f} x)")
    assert err <= max(4 * err_ex, 2.0 ** -23 * den), (what, err, err_ex, den)
    return err, err_ex


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_tiled_every_shape_and_form(lib, M, N, K):
    for i, (add, relu_a) in enumerate(FORMS):
        j = i + N // 64 + K // 32 + M
        c = P8.Case(lib, M, N, K, add, relu_a, bias=j % 2 == 0, act=1 if j % 3 == 0 else 0, pad=64 if j % 2 else 0)
        got, exact, ref = c.run(True, TILED), c.run(False), c.ref()
        _check(c, got, exact, ref, f"M {M} N {N} K {K} add {add} relu_a {relu_a}")
        assert not torch.equal(got, exact), "bit-equal to vlsat_k_gemm: the sibling never ran"
        if i == j % 5:
            assert torch.equal(got, c.run(True, TILED)), "two launches differ"


@pytest.mark.parametrize("relu_a", [0, 1])
@pytest.mark.parametrize("scale", [2.0 ** -8, 2.0 ** 4, 1000.0])
def test_tiled_scaled_activations(lib, scale, relu_a):
    """A times 2^-8 (unscaled, the fp16 lo parts of activations and Xavier weights would be subnormal), 2^4, 1000."""
    M, N, K = 2560 + 33, 512, 512
    c = P8.Case(lib, M, N, K, 0, relu_a, bias=False, act=0, a_scale=scale)
    _check(c, c.run(True, TILED), c.run(False), c.ref(), f"A x {scale:g} relu_a {relu_a}")


def test_tiled_edge_inputs(lib):
    """+-1e5 (outside +-65504: the operand saturates, nothing becomes Inf or NaN; compared against the clamped operand), an all-zero row
    block, -0.0 and negative rows under ReLU-on-A: the bias exactly."""
    M, N, K = 2560 + 33, 512, 512
    c = P8.Case(lib, M, N, K, 0, 0, bias=True, act=0)
    A = c.A.clone()
    A[5, 17], A[300, 400] = 1e5, -1e5
    A[256:512] = 0.0
    got = c.run(True, TILED, A)
    sat = A.clamp(-65504.0, 65504.0)
    _check(c, got, c.run(False, 0, sat), c.ref(sat), "A with +-1e5 against the saturated operand")
    assert torch.equal(got[256:512], c.b.cpu()[None, :].expand(256, N)), "an all-zero row block must give the bias exactly"
    r = P8.Case(lib, M, N, K, 0, 1, bias=True, act=0)
    A = r.A.clone()
    A[256:512] = -0.0
    A[700:] = -A[700:].abs()
    got = r.run(True, TILED, A)
    _check(r, got, r.run(False, 0, A), r.ref(A), "-0.0 and negative rows under ReLU-on-A")
    assert torch.equal(got[256:512], r.b.cpu()[None, :].expand(256, N)) and torch.equal(got[700:], r.b.cpu()[None, :].expand(M - 700, N))


@pytest.mark.parametrize("M,N,K,add", [(2560, 26, 512, 0), (65, 26, 32, 1), (2560 + 33, 40, 128, 0)])
def test_tiled_refused_shapes_run_the_exact_kernel(lib, M, N, K, add):
    """fewer than 64 output columns (the relation classifier's 26): gemm_f16s_tiled_pick refuses, the launch is vlsat_k_gemm's bit for bit"""
    c = P8.Case(lib, M, N, K, add, 0, bias=True, act=0, pad=6)
    assert torch.equal(c.run(True, TILED), c.run(False))


def test_p8_part_min_zero_or_more_keeps_the_exact_tails(lib):
    """p8_part_min >= 0 is f16s = 1 as before: one full round of the 8-phase kernel's tiles on its split-fp16 form, the rows behind it a
    tail launch of the exact kernels, bit-equal to vlsat_k_gemm; the same call with -1 runs the tail on the siblings too."""
    N, K = 256, 128
    one_round = P8._g1() // (N // 256) * 256
    M = one_round + 2 * 256 + 33
    c = P8.Case(lib, M, N, K, 1, 0, bias=True, act=0, pad=32)
    exact, ref = c.run(False), c.ref()
    assert P8._p8_rows(M, N, 0) == one_round
    got = c.run(True, 0)
    assert torch.equal(got[one_round:], exact[one_round:]), "f16s = 1: tail rows differ from vlsat_k_gemm"
    assert not torch.equal(got[:one_round], exact[:one_round])
    both = c.run(True, TILED)
    _check(c, both, exact, ref, "full round + tail, both on the split-fp16 forms")
    assert torch.equal(both[:one_round], got[:one_round]) and not torch.equal(both[one_round:], exact[one_round:])
