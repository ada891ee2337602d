"""The number scheme of the split-fp16 8-phase GEMM (csrc/gemm_p8_kernel.h, FS), emulated with numpy float16 -- no library, no device.

Every product w.a is three fp16 x fp16 products into one fp32 accumulator: weights as Wh = f16(W 2^k), Wl = f16(W 2^k - Wh) with
k = 13 - ceil(log2 max |W|) per tensor, activations as Ah = f16(x), Al = f16((x - Ah) 2^11), and the terms (Wh 2^-11).Al, Wl.Ah, Wh.Ah.
The emulation forms the three products exactly (fp16 x fp16 fits fp32, summed in fp64 per 16-wide k-step) and rounds the accumulator to
fp32 once per k-step and term, which is at least as coarse as the matrix pipe.  The emulated exact kernel is the fp32 product accumulated
in fp32 per k-step of its own instruction (v_mfma_f32_32x32x2_f32: two k).  Yardstick: the fp64 product of the same inputs; errors over max |ref|.

Cases (the issue's): M = 128, N = 64, K in {512, 1024}; W ~ U(+-sqrt(6 / (K + 512))); A = N(0, 1) s, s in {2^-8, 2^-3, 1, 16, 1000}, signed
and after ReLU: 20 cases, three seeds.  Asserted: the scheme stays within 2 x the emulated exact kernel's error everywhere (it measures
0.5 to 1.2 x), and the UNSCALED split (fp16 hi + lo of W and A as they are) exceeds 4 x at s = 2^-8 -- so neither scale can be dropped
without this test noticing."""
import math

import numpy as np
import pytest

F16_MAX = 65504.0


def _f16(x):
    return np.asarray(x, dtype=np.float32).astype(np.float16)


def _acc(terms, K, step=16):
    """fp32 accumulation: per k-step of one matrix instruction (16 wide on the 16-bit pipe, 2 on the fp32 pipe), the terms in the order
    given, each k-step's partial product summed exactly and added to the accumulator in fp32"""
    M, N = terms[0][0].shape[0], terms[0][1].shape[0]
    acc = np.zeros((M, N), dtype=np.float32)
    for k0 in range(0, K, step):
        for a, w in terms:
            part = a[:, k0:k0 + step].astype(np.float64) @ w[:, k0:k0 + step].astype(np.float64).T
            acc = (acc.astype(np.float64) + part).astype(np.float32)
    return acc


def _scheme(A, W):
    k = 13 - math.ceil(math.log2(float(np.abs(W).max())))
    Ws = (W.astype(np.float64) * 2.0 ** k).astype(np.float32)                   # exact
    Wh = _f16(Ws)
    Wl = _f16(Ws - Wh.astype(np.float32))
    Wt = _f16(Wh.astype(np.float32) * np.float32(2.0 ** -11))                   # the third operand, made from Wh
    assert np.array_equal(Wt.astype(np.float64) * 2048.0, Wh.astype(np.float64)) or float(np.abs(Wh[Wh != 0]).min()) < 0.125
    x = np.clip(A, -F16_MAX, F16_MAX).astype(np.float32)
    Ah = _f16(x)
    Al = _f16((x - Ah.astype(np.float32)) * np.float32(2048.0))
    acc = _acc([(Al, Wt), (Ah, Wl), (Ah, Wh)], A.shape[1])
    return (acc.astype(np.float64) * 2.0 ** -k).astype(np.float32)


def _unscaled(A, W):
    Wh = _f16(W)
    Wl = _f16(W - Wh.astype(np.float32))
    Ah = _f16(A)
    Al = _f16(A - Ah.astype(np.float32))
    return _acc([(Al, Wh), (Ah, Wl), (Ah, Wh)], A.shape[1])


def _exact(A, W):
    return _acc([(A, W)], A.shape[1], 2)


CASES = [(K, s, relu) for K in (512, 1024) for s in (2.0 ** -8, 2.0 ** -3, 1.0, 16.0, 1000.0) for relu in (False, True)]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_scheme_within_2x_of_exact_and_unscaled_split_is_not(seed):
    assert len(CASES) == 20
    rng = np.random.default_rng(seed)
    worst, unscaled_small = 0.0, []
    for K, s, relu in CASES:
        bound = math.sqrt(6.0 / (K + 512))
        W = rng.uniform(-bound, bound, size=(64, K)).astype(np.float32)
        A = (rng.standard_normal((128, K)) * s).astype(np.float32)
        if relu:
            A = np.maximum(A, 0)
        ref = A.astype(np.float64) @ W.astype(np.float64).T
        den = float(np.abs(ref).max())
        e_exact = float(np.abs(_exact(A, W) - ref).max()) / den
        e_new = float(np.abs(_scheme(A, W) - ref).max()) / den
        e_old = float(np.abs(_unscaled(A, W) - ref).max()) / den
        print(f"K {K} s {s:g} relu {relu}: exact {e_exact:.2e}, scheme {e_new / e_exact:.2f} x, unscaled split {e_old / e_exact:.2f} x")
        assert e_new <= 2 * e_exact, (K, s, relu, e_new, e_exact)
        worst = max(worst, e_new / e_exact)
        if s == 2.0 ** -8:
            unscaled_small.append(e_old / e_exact)
    assert min(unscaled_small) > 4, unscaled_small
    print(f"seed {seed}: scheme at most {worst:.2f} x the emulated exact kernel; unscaled split at 2^-8: {min(unscaled_small):.1f} - {max(unscaled_small):.1f} x")


def test_saturation_and_small_values():
    """|A| beyond 65504 saturates (finite results); Ah + Al 2^-11 gives x back to 2^-22 relative down to |x| = 2^-13."""
    x = np.array([1e5, -1e5, 65504.0, 70000.0, 2.0 ** -13 * 1.0001, -2.0 ** -13 * 1.37, 0.0, -0.0], dtype=np.float32)
    c = np.clip(x, -F16_MAX, F16_MAX)
    Ah = _f16(c)
    Al = _f16((c - Ah.astype(np.float32)) * np.float32(2048.0))
    assert np.isfinite(Ah.astype(np.float32)).all() and np.isfinite(Al.astype(np.float32)).all()
    assert float(Ah[0]) == F16_MAX and float(Ah[1]) == -F16_MAX and float(Al[0]) == 0.0
    back = Ah.astype(np.float64) + Al.astype(np.float64) / 2048.0
    assert (np.abs(back - c.astype(np.float64)) <= 2.0 ** -22 * np.abs(c.astype(np.float64))).all()      # 2^-22 relative down to |x| = 2^-13
