"""The arithmetic of the split-fp16 edge attention (csrc/flash_attn_16bit_kernel.h with X3, the fp32 mode's attention kernel), emulated
in torch on the CPU: the same split (hi = fp16(x) round-to-nearest after the clamp to +-65504, lo = fp16(x - hi), subnormal lo parts
kept), the same three terms per product in the kernel's order (lo.hi, hi.lo, hi.hi per 16-wide k-step, fp32 accumulation), the same
online softmax over 64-key tiles in exp2 with Q pre-multiplied by scale * log2 e, P split without a clamp; and the pre-scale that ships:
V times 2^3 and P times 2^14, K as it is (without the factor on V the lo plane of every value below 2^-3 is a
subnormal fp16 with an absolute error of 2^-25, and the 2^-8 case below misses its bound at 6 to 8 x).

Held against the same loop with exact fp32 products (the exact kernel's arithmetic) on the same inputs, both against an fp64 softmax:
one head of 1560 tokens x 64, Q ~ N(0, 2^2), K and V ~ N(0, 2^2) times 2^-8, 1 and 2^4.  Bound: 4 x the emulated exact-fp32 error, the
ratio of the unit roundoffs 2^-22 / 2^-24.  Needs no GPU and no library."""
import numpy as np
import pytest
import torch

T, D, KV = 1560, 64, 64
LOG2E = np.float32(1.4426950408889634)


def split_f16(x, clamp):
    """(hi, lo) as fp32 tensors holding fp16 values"""
    if clamp:
        x = x.clamp(-65504.0, 65504.0)
    hi = x.half().float()
    lo = (x - hi).half().float()
    return hi, lo


def _product(x, y, split):
    """x [M, K] (Q or P: the MFMA's B operand), y [N, K] (K or V^T: its A operand) -> x . y^T [M, N] in fp32, k-steps of 16 in order;
    split: x and y are (hi, lo) pairs and a step is y_lo . x_hi + y_hi . x_lo + y_hi . x_hi, small terms first"""
    if not split:
        x, y = (x, None), (y, None)
    (xh, xl), (yh, yl) = x, y
    acc = torch.zeros(xh.shape[0], yh.shape[0], dtype=torch.float32)
    for k0 in range(0, xh.shape[1], 16):
        s = slice(k0, k0 + 16)
        if split:
            acc = acc + xh[:, s] @ yl[:, s].t()
            acc = acc + xl[:, s] @ yh[:, s].t()
        acc = acc + xh[:, s] @ yh[:, s].t()
    return acc


VS, PBIAS = np.float32(8.0), np.float32(14.0)        # the kernel's pre-scale of V and its exponent bias of P


def attend(q, k, v, scale, split):
    """one head, fp32 [T, 64] each: the kernel's loop over 64-key tiles.  split: V times 2^3 before the split (exact; the factor leaves
    with the final 1 / l), P carries 2^14 (added to the exponent where the running maximum is subtracted), which l carries too"""
    qs = q * (np.float32(scale) * LOG2E)
    qo = split_f16(qs, True) if split else qs
    vs = VS if split else np.float32(1.0)
    bias = PBIAS if split else np.float32(0.0)
    o = torch.zeros(T, D, dtype=torch.float32)
    m = torch.full((T,), -float("inf"), dtype=torch.float32)
    l = torch.zeros(T, dtype=torch.float32)
    for t0 in range(0, T, KV):
        kt, vt = k[t0:t0 + KV], v[t0:t0 + KV]
        s = _product(qo, split_f16(kt, True) if split else kt, split)                    # [T, keys]
        m_new = torch.maximum(m, s.max(1).values)
        alpha = torch.exp2(m - m_new)
        p = torch.exp2(s - (m_new - bias)[:, None])                                      # (m - 14 is rounded, then s - that: as in the kernel)
        l = l * alpha + p.sum(1)
        m = m_new
        o = o * alpha[:, None]
        vtt = vt.t().contiguous()                                                        # [64 d, keys]
        o = o + _product(split_f16(p, False) if split else p, split_f16(vtt * vs, True) if split else vtt, split)
    return o * ((1.0 / l) * (np.float32(1.0) / vs))[:, None]


@pytest.fixture(scope="module")
def qkv():
    g = torch.Generator().manual_seed(1560)
    return tuple(torch.randn(T, D, generator=g) * 2 for _ in range(3))


@pytest.mark.parametrize("log2_scale", [-8, 0, 4])
def test_split_fp16_attention_is_fp32_grade(qkv, log2_scale):
    q, k0, v0 = qkv
    sc = float(2.0 ** log2_scale)
    k, v = k0 * sc, v0 * sc
    ref = torch.softmax(q.double() @ k.double().t() * 0.125, -1) @ v.double()
    den = float(ref.abs().max())
    err_exact = float((attend(q, k, v, 0.125, False).double() - ref).abs().max()) / den
    err_split = float((attend(q, k, v, 0.125, True).double() - ref).abs().max()) / den
    print(f"K, V scale 2^{log2_scale}: exact fp32 {err_exact:.2e}, split-fp16 x3 {err_split:.2e} ({err_split / err_exact:.2f} x)")
    assert err_exact < 1e-4, err_exact                  # the emulation itself is sane
    assert err_split <= 4 * err_exact, (err_split, err_exact)


def test_split_is_exact_to_2_pow_minus_22_and_clamps():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(4096, generator=g) * torch.tensor(2.0) ** torch.randint(-10, 14, (4096,), generator=g).float()
    hi, lo = split_f16(x, True)
    err = ((hi + lo) - x).abs()
    # 11 + 11 bits and the sign of lo: 2^-22 |x|; a lo part below 2^-14 is a subnormal fp16 with an absolute error of 2^-25
    assert bool((err <= torch.maximum(x.abs() * 2.0 ** -22, torch.tensor(2.0 ** -25))).all()), float((err / x.abs()).max())
    big = torch.tensor([1e6, -1e6, 65504.0, 70000.0])
    hi, lo = split_f16(big, True)
    assert torch.isfinite(hi).all() and torch.isfinite(lo).all()
    assert torch.equal(hi + lo, torch.tensor([65504.0, -65504.0, 65504.0, 65504.0]))
