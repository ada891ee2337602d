"""The GEMM pair word (csrc/gemm_f16s_planes.h f16s_pair_pack) in numpy float16, independent of the header's integer code:
word = Ah << 16 | Al,  Ah = f16(xc),  Al = f16((xc - Ah) 2^11),  xc = x clamped to +-65504.  The difference and the product with 2^11 are
exact in fp32; the only roundings are the two conversions to fp16 (round to nearest even, subnormals kept).
tests/test_e2_pairs_cpu.py checks it against the header, tests/test_hip_layernorm_pairs.py checks the LayerNorm kernel against it."""
import numpy as np

# values a test plants: -0.0, |x| below 2^-13 (hi parts that are fp16 subnormals, lo parts below fp16's normal range even times 2^11),
# the clamp at +-65504 and beyond, zeros
PLANTED = np.array([0.0, -0.0, 1.0, -1.0, 2.0 ** -13, -2.0 ** -13, 1.2e-4, -1.2e-4, 6.1e-5, -6.1e-5, 3e-5, 6e-8, 2.9e-8, -2.9e-8, 1e-12, -1e-12,
                    65504.0, -65504.0, 65519.0, 65520.0, 7e4, -7e4, 1e9, -1e9, 3e38, -3e38, 0.1, -0.3333, 1234.5678, -4097.3], np.float32)


def pack(x):
    """fp32 array -> uint32 array of pair words"""
    x = np.asarray(x, np.float32)
    xc = np.clip(x, np.float32(-65504.0), np.float32(65504.0))
    hi = xc.astype(np.float16)
    lo = ((xc - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return (hi.view(np.uint16).astype(np.uint32) << np.uint32(16)) | lo.view(np.uint16).astype(np.uint32)
