"""The number scheme of the split-fp16 PointNet (csrc/pointnet_bf16.hip, TERMS = 5) over its two matrix layers, emulated with numpy
float16 -- no library, no device.

The chain: H1 [points, 64] >= 0 -> conv2 (W2 [128, 64]) + b2 -> ReLU -> split again -> conv3 (W3 [n_out, 128]) + b3.  Each layer is the
scheme of tests/test_gemm_f16s_emulation_cpu.py: weights as Wh = f16(W 2^k), Wl = f16(W 2^k - Wh), k = 13 - ceil(log2 max |W|) per tensor;
activations clamped to [0, 65504] as Ah = f16(x), Al = f16((x - Ah) 2^11); the terms (Wh 2^-11).Al, Wl.Ah, Wh.Ah into one fp32 accumulator
per 16-wide k-step (each product exact, a k-step's partial sum exact, one fp32 rounding per k-step and term: at least as coarse as the
matrix pipe); the accumulator times 2^-k, then bias and ReLU in fp32.  Next to it the exact kernel's chain: fp32 products accumulated in
fp32 per k-step of v_mfma_f32_32x32x2_f32 (two k).  Yardstick: the fp64 chain of the same inputs; errors over max |ref|.

Asserted: the scheme's error stays below 4 x the emulated exact chain's (the bound of the kernel test), and the UNSCALED split (fp16 hi +
lo of W and the activations as they are) exceeds 4 x at activations x 2^-8 -- the re-split H2 of the second layer needs both scales as much
as a GEMM operand does."""
import math

import numpy as np
import pytest

F16_MAX = 65504.0


def _f16(x):
    return np.asarray(x, dtype=np.float32).astype(np.float16)


def _acc(terms, K, step):
    M, N = terms[0][0].shape[0], terms[0][1].shape[0]
    acc = np.zeros((M, N), dtype=np.float32)
    for k0 in range(0, K, step):
        for a, w in terms:
            part = a[:, k0:k0 + step].astype(np.float64) @ w[:, k0:k0 + step].astype(np.float64).T
            acc = (acc.astype(np.float64) + part).astype(np.float32)
    return acc


def _layer_scheme(A, W, b):
    k = 13 - math.ceil(math.log2(float(np.abs(W).max())))
    Ws = (W.astype(np.float64) * 2.0 ** k).astype(np.float32)                   # exact
    Wh = _f16(Ws)
    Wl = _f16(Ws - Wh.astype(np.float32))
    Wt = _f16(Wh.astype(np.float32) * np.float32(2.0 ** -11))
    x = np.clip(A, 0.0, F16_MAX).astype(np.float32)
    Ah = _f16(x)
    Al = _f16((x - Ah.astype(np.float32)) * np.float32(2048.0))
    acc = _acc([(Al, Wt), (Ah, Wl), (Ah, Wh)], A.shape[1], 16)
    return np.maximum((acc.astype(np.float64) * 2.0 ** -k).astype(np.float32) + b, np.float32(0))


def _layer_unscaled(A, W, b):
    Wh = _f16(W)
    Wl = _f16(W - Wh.astype(np.float32))
    Ah = _f16(A)
    Al = _f16(A - Ah.astype(np.float32))
    return np.maximum(_acc([(Al, Wh), (Ah, Wl), (Ah, Wh)], A.shape[1], 16) + b, np.float32(0))


def _layer_exact(A, W, b):
    return np.maximum(_acc([(A, W)], A.shape[1], 2) + b, np.float32(0))


def _chain(layer, H1, W2, b2, W3, b3):
    return layer(layer(H1, W2, b2), W3, b3)


SCALES = (2.0 ** -8, 1.0, 16.0, 1000.0)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_chain_within_4x_of_exact_and_unscaled_split_is_not(seed):
    rng = np.random.default_rng(seed)
    worst, unscaled_small = 0.0, []
    for s in SCALES:
        b2w, b3w = math.sqrt(6.0 / (64 + 128)), math.sqrt(6.0 / (128 + 256))
        W2 = rng.uniform(-b2w, b2w, size=(128, 64)).astype(np.float32)
        W3 = rng.uniform(-b3w, b3w, size=(256, 128)).astype(np.float32)
        H1 = np.maximum(rng.standard_normal((128, 64)) * s, 0).astype(np.float32)
        b2 = (rng.standard_normal(128) * 0.1 * s).astype(np.float32)               # biases on the activations' scale: the chain is
        b3 = (rng.standard_normal(256) * 0.1 * s).astype(np.float32)               # homogeneous in s, no bias hides a product's error
        h = np.maximum(H1.astype(np.float64) @ W2.astype(np.float64).T + b2, 0)
        ref = np.maximum(h @ W3.astype(np.float64).T + b3, 0)
        den = float(np.abs(ref).max())
        e_exact = float(np.abs(_chain(_layer_exact, H1, W2, b2, W3, b3) - ref).max()) / den
        e_new = float(np.abs(_chain(_layer_scheme, H1, W2, b2, W3, b3) - ref).max()) / den
        e_old = float(np.abs(_chain(_layer_unscaled, H1, W2, b2, W3, b3) - ref).max()) / den
        print(f"s {s:g}: exact chain {e_exact:.2e}, scheme {e_new / e_exact:.2f} x, unscaled split {e_old / e_exact:.2f} x")
        assert e_new < 4 * e_exact, (s, e_new, e_exact)
        worst = max(worst, e_new / e_exact)
        if s == 2.0 ** -8:
            unscaled_small.append(e_old / e_exact)
    assert min(unscaled_small) > 4, unscaled_small
    print(f"seed {seed}: scheme at most {worst:.2f} x the emulated exact chain; unscaled split at 2^-8: {min(unscaled_small):.1f} x")
