"""CPU restatement (torch) of the number formats and rounding points of the 16-bit kernels -- the yardstick the GPU tests
of those kernels compare against, and the host side of the tensor formats the tests hand over.

Formats (csrc/common.h, csrc/pointnet_bf16.hip, csrc/small_ops.hip):
  split pairs   one 32-bit word per element: bf16 hi = rne(x) in the upper half, bf16 lo = rne(x - hi) in the lower half
  half rows     fp32-pitched rows carrying 16-bit values (bf16 or fp16) at byte 2 * column
  fp16          rne after a clamp to +-65504 (never inf)

`pointnet_model` restates where pointnet_bf16.hip rounds: conv1 in full precision; h1 and h2 rounded to the operand format
after the ReLU; W2 and W3 rounded the same way; a split product is ah.wh + al.wh + ah.wl (no lo.lo term); bias, ReLU and the
max over points in the accumulation type.  With acc_dtype = float64 it is the kernel's arithmetic with exact accumulation,
so its distance from the exact fp64 PointNet is the error the FORMAT costs -- the figure a kernel is measured against.
"""
import functools

import numpy as np
import torch

F16_MAX = 65504.0


# ---- tensor formats ------------------------------------------------------------------------------------------------------
def pack_split(x):
    """Host restatement of common.h pack_split: (bf16 rne(x) << 16) | bf16 rne(x - hi), as float32 bit patterns."""
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    w = (hi.view(torch.int16).to(torch.int32) << 16) | (lo.view(torch.int16).to(torch.int32) & 0xFFFF)
    return w.view(torch.float32)


def unpack_split(w):
    u = w.view(torch.int32)
    return (u & -65536).view(torch.float32) + (u << 16).view(torch.float32)


def to_half_rows(x):
    """fp32-pitched rows carrying bf16 values at byte 2 * column (the half-row format of the single-rounding modes)."""
    M, N = x.shape
    out = torch.zeros(M, N, dtype=torch.float32)
    out.view(torch.bfloat16).view(M, 2 * N)[:, :N] = x.to(torch.bfloat16)
    return out


def from_half_rows(w, N):
    return w.view(torch.bfloat16).view(w.shape[0], -1)[:, :N].float()


def to_f16(x):
    """fp16 as the kernels store it: rne of the value clamped to the finite range."""
    return x.clamp(-F16_MAX, F16_MAX).to(torch.float16)


def to_half_rows_f16(x):
    """fp32-pitched rows carrying fp16 values at byte 2 * column (precision mode fp16_mixed)."""
    M, N = x.shape
    out = torch.zeros(M, N, dtype=torch.float32)
    out.view(torch.float16).view(M, 2 * N)[:, :N] = to_f16(x)
    return out


def from_half_rows_f16(w, N):
    return w.view(torch.float16).view(w.shape[0], -1)[:, :N].float()


# ---- operand rounding ----------------------------------------------------------------------------------------------------
def _chop(x, keep_mask):
    """round toward zero by clearing low fp32 mantissa bits (the deliberately wrong rounding of the yardstick's own tests)"""
    return (x.float().contiguous().view(torch.int32) & keep_mask).view(torch.float32)


def quantise(x, fmt, rounding="rne"):
    """The planes an operand of format `fmt` is multiplied as: [x16] for bf16 / fp16, [hi, lo] for split -- in x's dtype, each
    value exactly representable in the 16-bit format.  rounding = "trunc" rounds toward zero instead of to nearest even."""
    if fmt == "bf16" or fmt == "split":
        if rounding == "rne":
            hi = x.to(torch.bfloat16).to(x.dtype)
        else:
            hi = _chop(x, -65536).to(x.dtype)
        if fmt == "bf16":
            return [hi]
        r = x - hi                                # exact: hi holds the leading bits of x
        lo = r.to(torch.bfloat16).to(x.dtype) if rounding == "rne" else _chop(r, -65536).to(x.dtype)
        return [hi, lo]
    if fmt == "fp16":
        c = x.clamp(-F16_MAX, F16_MAX)
        if rounding == "rne":
            return [c.to(torch.float16).to(x.dtype)]
        return [_chop(c, -8192).to(x.dtype)]      # (10 mantissa bits; exact for fp16 normals, which is all a wrong model needs)
    raise ValueError(f"fmt must be bf16, fp16 or split, got {fmt!r}")


SPLIT_TERMS = ("hh", "lh", "hl")                  # (activation plane, weight plane): ah.wh + al.wh + ah.wl


def qlinear(a_planes, w_planes, terms=SPLIT_TERMS):
    """sum of the plane products a . w^T in the planes' dtype (the accumulation type)"""
    if len(a_planes) == 1:
        return a_planes[0] @ w_planes[0].t()
    idx = {"h": 0, "l": 1}
    out = None
    for t in terms:
        p = a_planes[idx[t[0]]] @ w_planes[idx[t[1]]].t()
        out = p if out is None else out + p
    return out


def pointnet_exact(pts, weights):
    """fp64 PointNet: pts [N,C,P], weights = (w1 [64,C], b1, w2 [128,64], b2, w3 [n_out,128], b3) -> [N,n_out] float64"""
    w1, b1, w2, b2, w3, b3 = (t.double() for t in weights)
    out = []
    for o in range(0, pts.shape[0], 64):
        h = pts[o:o + 64].double().transpose(1, 2)
        h = torch.relu(h @ w1.t() + b1)
        h = torch.relu(h @ w2.t() + b2)
        out.append(torch.relu(h @ w3.t() + b3).amax(1))
    return torch.cat(out)


def pointnet_model(pts, weights, fmt, acc_dtype=torch.float64, rounding="rne", terms=SPLIT_TERMS, w_fmt=None):
    """The PointNet of pointnet_bf16.hip with its rounding points (module docstring) -> [N,n_out] in acc_dtype.
    fmt: bf16 | fp16 | split (the kernel's terms 1 | 2 | 3).  rounding, terms and w_fmt (format of the weight planes when it is to
    differ from fmt) exist to build deliberately wrong models."""
    w1, b1, w2, b2, w3, b3 = (t.to(acc_dtype) for t in weights)
    w2p, w3p = quantise(w2, w_fmt or fmt, rounding), quantise(w3, w_fmt or fmt, rounding)
    out = []
    for o in range(0, pts.shape[0], 64):
        h = pts[o:o + 64].to(acc_dtype).transpose(1, 2)
        h = torch.relu(h @ w1.t() + b1)
        h = torch.relu(qlinear(quantise(h, fmt, rounding), w2p, terms) + b2)
        out.append(torch.relu(qlinear(quantise(h, fmt, rounding), w3p, terms) + b3).amax(1))
    return torch.cat(out)


def rel_rms(a, ref):
    """rms(a - ref) / rms(ref)"""
    a, ref = a.double(), ref.double()
    return float(((a - ref) ** 2).mean().sqrt() / (ref ** 2).mean().sqrt())


# ---- the PointNet inputs of the kernel tests ---------------------------------------------------------------------------------
# Every input meets the two conditions of test_quant_model_cpu.py (a correct fp32-accumulating implementation is within 1 % of
# E_m and at most half as far from the model as the model is from the exact result).  The split format leaves little room for
# the second one -- an fp32 rounding of h can flip a lo plane's last bit -- so the seed of an input that missed a condition
# was replaced; the conditions were not touched.
#    name              P  n_obj cin weights  seed
POINTNET_CASES = {
    "p300_n1":         (300,   1, 3, "cfg",     8),        # one object over several blocks, merged atomically
    "p300_n600":       (300, 600, 3, "cfg",     0),        # one block per object
    "p1_n3":           (1,     3, 3, "cfg",     0),
    "p127_n3_c6":      (127,   3, 6, "cfg",     1),
    "p128_n1_c9":      (128,   1, 9, "cfg",     4),
    "p129_n3_c9":      (129,   3, 9, "cfg",     4),
    "p129_n1_c6_o128": (129,   1, 6, "rand128", 8),
    "p300_n3_o384":    (300,   3, 3, "rand384", 0),
}
FMT_OF_TERMS = {1: "bf16", 2: "fp16", 3: "split"}


@functools.lru_cache(maxsize=None)
def pointnet_weights(kind, cin):
    """(w1, b1, w2, b2, w3, b3) float32: the object encoder of synth.make_weights for a config with `cin` point channels, or a
    random set with n_out 128 / 384"""
    if kind == "cfg":
        from vlsat_amd import VLSATConfig, synth
        w = synth.make_weights(VLSATConfig(USE_RGB=cin >= 6, USE_NORMAL=cin >= 9))
        t = [torch.from_numpy(np.ascontiguousarray(w[f"obj_encoder.conv{i}.{k}"])) for i in (1, 2, 3) for k in ("weight", "bias")]
        return tuple(x.reshape(x.shape[0], -1) if x.dim() == 3 else x for x in t)
    n_out = {"rand128": 128, "rand384": 384}[kind]
    g = torch.Generator().manual_seed(1000 * n_out + cin)
    return ((torch.randn(64, cin, generator=g) / cin ** 0.5), torch.randn(64, generator=g) * 0.1,
            (torch.randn(128, 64, generator=g) / 8), torch.randn(128, generator=g) * 0.1,
            (torch.randn(n_out, 128, generator=g) / 128 ** 0.5), torch.randn(n_out, generator=g) * 0.1)


@functools.lru_cache(maxsize=None)
def pointnet_points(P, n_obj, cin, seed=0):
    """[n_obj, cin, P] float32: the first P object points of a synth.make_batch scene (of at least 32 points per object: a
    one-point object would be its own mean, all zeros), colour / normal channels uniform in [-1, 1]"""
    from vlsat_amd import synth
    pts = torch.from_numpy(synth.make_batch(1, n_obj, max(P, 32), seed0=4000 + P + 100 * seed)["obj_points"][:, :, :P])
    if cin > 3:
        g = torch.Generator().manual_seed(P * 10 + cin + 1000 * seed)
        pts = torch.cat([pts, torch.rand(n_obj, cin - 3, P, generator=g) * 2 - 1], 1)
    return pts.contiguous()


def pointnet_case(name):
    P, n_obj, cin, kind, seed = POINTNET_CASES[name]
    return pointnet_points(P, n_obj, cin, seed), pointnet_weights(kind, cin)


@functools.lru_cache(maxsize=None)
def pointnet_case_exact(name):
    return pointnet_exact(*pointnet_case(name))


@functools.lru_cache(maxsize=None)
def pointnet_case_model(name, fmt):
    """fp64-accumulating model of one case (computed once, shared, never modified)"""
    return pointnet_model(*pointnet_case(name), fmt)
