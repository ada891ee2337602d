"""The number scheme of the split-fp16 edge gate (csrc/edge_gate_f16s.hip), emulated with numpy float16 -- no library, no device.

The gate's two layers as one chain per (edge, head) row, at the shipped geometry (W0k [128 x 64], W3 [32 x 128]):
  acc1 = W0k 2^k0 . kproj        three fp16 products per k-step of 16: (Wh 2^-11).Al, Wl.Ah, Wh.Ah into one fp32 accumulator
  hidden = relu(acc1 2^-k0 + Gq) one fp32 rounding (the multiply by a power of two is exact); split again: Ah = f16(clamp), Al = f16((x - Ah) 2^11)
  logits = (b3 2^k3 + W3 2^k3 . hidden) 2^-k3
with k = 13 - ceil(log2 max |W|) per tensor and Wh = f16(W 2^k), Wl = f16(W 2^k - Wh).  The emulation forms every product exactly and
rounds the accumulator to fp32 once per k-step and term (at least as coarse as the matrix pipe).  The emulated exact kernel is the same
chain with fp32 products accumulated per k-step of two (v_mfma_f32_32x32x2_f32).  Yardstick: the chain in fp64 on the same fp32 inputs;
errors of the logits over max |logits|.

Cases: weights as tests/test_hip_gcn_kernels.py draws them (N(0, 1.5 / sqrt(128)) and N(0, 2 / sqrt(128)), b3 N(0, 0.2)), 256 rows,
max |kproj| of 1, 500 and 3000 (Gq of the same scale), three seeds.  Measured ratio scheme / exact over the nine cases: 0.60 - 0.98
(one layer of the GEMM measured 0.5 - 1.2, tests/test_gemm_f16s_emulation_cpu.py).  Asserted: at most 1.96 = twice the largest measured
ratio.  The same scheme WITHOUT the weight scale (k = 0) on weights of 2^-8 (Gq and b3 shrunk with them) measures 78 - 114 x the exact
chain, the scaled scheme 0.71 - 0.88 x; asserted: k = 0 stays above 4 x -- the scale cannot be dropped without this test noticing."""
import math

import numpy as np
import pytest

F16_MAX = 65504.0
BOUND = 1.96


def _f16(x):
    return np.asarray(x, dtype=np.float32).astype(np.float16)


def _acc(terms, K, step, init=None):
    """fp32 accumulation: per k-step of one matrix instruction, the terms in the order given, each k-step's partial product summed
    exactly and added to the accumulator in fp32"""
    M, N = terms[0][0].shape[0], terms[0][1].shape[0]
    acc = np.zeros((M, N), dtype=np.float32) if init is None else np.broadcast_to(init.astype(np.float32), (M, N)).copy()
    for k0 in range(0, K, step):
        for a, w in terms:
            part = a[:, k0:k0 + step].astype(np.float64) @ w[:, k0:k0 + step].astype(np.float64).T
            acc = (acc.astype(np.float64) + part).astype(np.float32)
    return acc


def _exponent(W, scaled):
    return 13 - math.ceil(math.log2(float(np.abs(W).max()))) if scaled else 0


def _planes(W, k):
    Ws = (W.astype(np.float64) * 2.0 ** k).astype(np.float32)                   # exact
    Wh = _f16(Ws)
    return Wh, _f16(Ws - Wh.astype(np.float32)), _f16(Wh.astype(np.float32) * np.float32(2.0 ** -11))


def _split(x, lower):
    x = np.clip(x, lower, F16_MAX).astype(np.float32)
    Ah = _f16(x)
    return Ah, _f16((x - Ah.astype(np.float32)) * np.float32(2048.0))


def _layer(A, W, k, lower, init=None):
    Wh, Wl, Wt = _planes(W, k)
    Ah, Al = _split(A, lower)
    return _acc([(Al, Wt), (Ah, Wl), (Ah, Wh)], A.shape[1], 16, init)


def _scheme(Z, Gq, W0, W3, b3, scaled=True):
    k0, k3 = _exponent(W0, scaled), _exponent(W3, scaled)
    acc1 = _layer(Z, W0, k0, -F16_MAX)
    hid = (acc1.astype(np.float64) * 2.0 ** -k0 + Gq.astype(np.float64)).astype(np.float32)      # one fma
    acc2 = _layer(hid, W3, k3, 0.0, (b3.astype(np.float64) * 2.0 ** k3).astype(np.float32))     # the lower bound of the split is the ReLU
    return (acc2.astype(np.float64) * 2.0 ** -k3).astype(np.float32)


def _exact(Z, Gq, W0, W3, b3):
    acc1 = _acc([(Z, W0)], Z.shape[1], 2)
    hid = np.maximum((acc1.astype(np.float64) + Gq.astype(np.float64)).astype(np.float32), 0)
    return _acc([(hid, W3)], hid.shape[1], 2, b3)


def _ref(Z, Gq, W0, W3, b3):
    d = lambda x: x.astype(np.float64)
    return np.maximum(d(Z) @ d(W0).T + d(Gq), 0) @ d(W3).T + d(b3)


def _case(rng, s, wmax=None):
    W0 = (rng.standard_normal((128, 64)) * 1.5 / math.sqrt(128)).astype(np.float32)
    W3 = (rng.standard_normal((32, 128)) * 2.0 / math.sqrt(128)).astype(np.float32)
    f0 = f3 = 1.0
    if wmax is not None:            # small weights: Gq (a product with the other half of W0) and b3 shrink with them, or they hide the products
        f0, f3 = wmax / float(np.abs(W0).max()), wmax / float(np.abs(W3).max())
        W0, W3 = (W0 * f0).astype(np.float32), (W3 * f3).astype(np.float32)
    b3 = (rng.standard_normal(32) * 0.2 * f0 * f3).astype(np.float32)
    Z = rng.standard_normal((256, 64))
    Z = (Z * (s / np.abs(Z).max())).astype(np.float32)
    Gq = (rng.standard_normal((256, 128)) * (s / 4) * f0).astype(np.float32)
    return Z, Gq, W0, W3, b3


def _errors(fn, args, ref):
    return float(np.abs(fn(*args) - ref).max()) / float(np.abs(ref).max())


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_gate_chain_within_twice_the_measured_ratio_of_the_exact_chain(seed):
    rng = np.random.default_rng(seed)
    for s in (1.0, 500.0, 3000.0):
        args = _case(rng, s)
        ref = _ref(*args)
        e_exact, e_new = _errors(_exact, args, ref), _errors(_scheme, args, ref)
        print(f"seed {seed} max |kproj| {s:g}: exact chain {e_exact:.2e}, split-fp16 chain {e_new:.2e} = {e_new / e_exact:.2f} x")
        assert e_new <= BOUND * e_exact, (seed, s, e_new, e_exact)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_unscaled_split_is_visibly_worse_at_small_weights(seed):
    rng = np.random.default_rng(seed)
    args = _case(rng, 1.0, wmax=2.0 ** -8)
    ref = _ref(*args)
    e_exact, e_new = _errors(_exact, args, ref), _errors(_scheme, args, ref)
    e_k0 = _errors(lambda *a: _scheme(*a, scaled=False), args, ref)
    print(f"seed {seed} weights of 2^-8: exact chain {e_exact:.2e}, scaled {e_new / e_exact:.2f} x, k = 0 {e_k0 / e_exact:.1f} x")
    assert e_new <= BOUND * e_exact and e_k0 > 4 * e_exact, (e_new, e_k0, e_exact)
