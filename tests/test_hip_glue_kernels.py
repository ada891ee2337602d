"""Direct tests of the kernels that otherwise run only inside a whole forward, each through its C entry point against a plain
fp64 reference or, for the 16-bit PointNet, against the CPU model of its rounding points (tests/quant_model.py, validated by
tests/test_quant_model_cpu.py): every PointNet kernel and operand form, every form of the LayerNorm kernel, the glue kernels of
small_ops.hip / stn.hip, the weight split, and the node attention at several key chunks, odd pitches and hard biases.
Every output buffer is pre-filled with NaN; what a kernel does not promise to write must still hold the fill afterwards.
Needs an MI355X:  pytest -m gpu"""
import math

import numpy as np
import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import VLSATConfig, synth
from oracle import vlsat_oracle as O
import quant_model as Q

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN_BITS = 0x7FC00000


@pytest.fixture(scope="module")
def lib():
    from vlsat_amd import lib as L
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path cannot run and there is no fallback")
    return L


def _sync():
    torch.cuda.synchronize()


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _untouched(t):
    """every word still holds the NaN the buffer was filled with"""
    return bool((t.contiguous().view(torch.int32) == NAN_BITS).all())


# ---- PointNet: every kernel and operand form -------------------------------------------------------------------------------
def _pointnet_ex(L, pts, w, terms):
    """pts [n, cin, P] (device), w = (w1, b1, w2, b2, w3, b3) (device) -> [n, n_out] on the CPU; the words behind the output
    must come back untouched"""
    n, cin, P = pts.shape
    n_out = w[4].shape[0]
    buf = _nan(n * n_out + 128)
    L.check(L.load().vlsat_k_pointnet_ex(pts.data_ptr(), n, P, cin, *(t.data_ptr() for t in w[:6]), n_out, terms, buf.data_ptr(),
                                         L.stream_ptr()))
    _sync()
    assert _untouched(buf[n * n_out:]), "pointnet wrote behind its [n, n_out] block"
    return buf[:n * n_out].view(n, n_out).cpu()


_PN_GOT = {}


def _pn_case(L, name, terms):
    """the kernel's output for one input of quant_model.POINTNET_CASES, computed once per (input, terms)"""
    if (name, terms) not in _PN_GOT:
        pts, w = Q.pointnet_case(name)
        _PN_GOT[name, terms] = _pointnet_ex(L, pts.to(DEV), tuple(t.contiguous().to(DEV) for t in w), terms)
    return _PN_GOT[name, terms]


@pytest.mark.parametrize("name", sorted(Q.POINTNET_CASES))
def test_pointnet_fp32_all_channel_counts_and_widths(lib, name):
    """terms 0: the fp32 kernel at 3 / 6 / 9 point channels and 128 / 384 / 768 outputs, against fp64 at test_pointnet_vs_oracle's
    tolerance"""
    got = _pn_case(lib, name, 0)
    err = float((got.double() - Q.pointnet_case_exact(name)).abs().max())
    assert err < 2e-5, f"pointnet fp32 {name}: {err:.3e}"


@pytest.mark.parametrize("terms", [1, 2, 3])
@pytest.mark.parametrize("name", sorted(Q.POINTNET_CASES))
def test_pointnet_16bit_error_matches_its_format(lib, name, terms):
    """E_k = relative RMS error of the kernel against exact fp64, E_m = that of the fp64-accumulating model of the kernel's
    rounding points: 2/3 <= E_k / E_m <= 3/2 (a correct fp32-accumulating implementation sits at 1.00 +- 0.01, the nearest wrong
    behaviour -- truncation, a dropped split term, another format -- at x 3 or more, a more precise variant than asked for at
    x 0.14 or less: tests/test_quant_model_cpu.py), and the kernel is no farther from its model than the model is from the truth."""
    fmt = Q.FMT_OF_TERMS[terms]
    got = _pn_case(lib, name, terms).double()
    exact, model = Q.pointnet_case_exact(name), Q.pointnet_case_model(name, fmt)
    assert torch.isfinite(got).all()
    ek, em = Q.rel_rms(got, exact), Q.rel_rms(model, exact)
    d_model, d_exact = float((got - model).abs().max()), float((model - exact).abs().max())
    print(f"pointnet {name} terms {terms} ({fmt}): E_k {ek:.3e}  E_m {em:.3e}  E_k / E_m {ek / em:.4f}  "
          f"max|got - model| {d_model:.3e}  max|model - exact| {d_exact:.3e}")
    assert 2.0 / 3.0 <= ek / em <= 3.0 / 2.0, f"{name} terms {terms}: E_k / E_m = {ek / em:.4f}"
    assert d_model <= d_exact, f"{name} terms {terms}: max|got - model| {d_model:.3e} > max|model - exact| {d_exact:.3e}"


TERMS = [0, 1, 2, 3]


@pytest.mark.parametrize("terms", TERMS)
def test_pointnet_object_alone_equals_object_in_batch(lib, terms):
    """An object computed alone (its chunks spread over several blocks that merge with atomicMax) equals, bit for bit, the same
    object inside the 600-object batch (one block per object, plain stores)."""
    pts, w = Q.pointnet_case("p300_n600")
    wd = tuple(t.contiguous().to(DEV) for t in w)
    batch = _pn_case(lib, "p300_n600", terms)
    for i in (0, 17, 599):
        alone = _pointnet_ex(lib, pts[i:i + 1].contiguous().to(DEV), wd, terms)
        assert torch.equal(alone[0], batch[i]), f"terms {terms} object {i}: {float((alone[0] - batch[i]).abs().max()):.3e}"


@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("name", ["p300_n1", "p129_n3_c9", "p127_n3_c6"])
def test_pointnet_point_order_does_not_matter(lib, name, terms):
    pts, w = Q.pointnet_case(name)
    perm = torch.randperm(pts.shape[2], generator=torch.Generator().manual_seed(5))
    got = _pointnet_ex(lib, pts[:, :, perm].contiguous().to(DEV), tuple(t.contiguous().to(DEV) for t in w), terms)
    assert torch.equal(got, _pn_case(lib, name, terms))


@pytest.mark.parametrize("terms", TERMS)
def test_pointnet_last_chunk_clamp(lib, terms):
    """P = 129 equals P = 200 with the 129th point repeated 71 times: the rows of the last chunk past P repeat the last point"""
    pts, w = Q.pointnet_case("p129_n3_c9")
    padded = torch.cat([pts, pts[:, :, 128:129].expand(-1, -1, 71)], 2).contiguous()
    got = _pointnet_ex(lib, padded.to(DEV), tuple(t.contiguous().to(DEV) for t in w), terms)
    assert torch.equal(got, _pn_case(lib, "p129_n3_c9", terms))


@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("name", ["p300_n1", "p129_n3_c9", "p300_n600", "p129_n1_c6_o128"])
def test_pointnet_all_negative_preactivations_give_plus_zero(lib, name, terms):
    """with b3 = -1e3 every conv3 output is negative: the ReLU folded into the max leaves exactly +0.0 everywhere"""
    pts, w = Q.pointnet_case(name)
    w = tuple(t.contiguous().to(DEV) for t in w[:5]) + (torch.full_like(w[5], -1e3).to(DEV),)
    got = _pointnet_ex(lib, pts.to(DEV), w, terms)
    assert torch.equal(got.view(torch.int32), torch.zeros_like(got, dtype=torch.int32))


def test_pointnet_ex_rejects_bad_arguments(lib):
    pts, w = Q.pointnet_case("p1_n3")
    wd = tuple(t.contiguous().to(DEV) for t in w)
    for terms in (-1, 4):
        with pytest.raises(lib.VlsatError):
            _pointnet_ex(lib, pts.to(DEV), wd, terms)
    for terms in TERMS:                                   # 4 point channels: no such kernel
        with pytest.raises(lib.VlsatError):
            _pointnet_ex(lib, torch.zeros(3, 4, 1, device=DEV), wd, terms)


# ---- LayerNorm: every input, residual and output form ------------------------------------------------------------------------
LD, LDY, LDR = 520, 768, 640
LN_ROWS = [1, 3, 4, 5, 4099]
RESID_FORMS = ["none", "f32", "split", "bf16", "f16"]
RESID_FMT = {"none": 0, "f32": 0, "split": 1, "bf16": 2, "f16": 4}
_LN_DATA = {}


def _pitched(t, ld):
    """t [rows, 512] -> device buffer [rows, ld] holding it in the leading columns, NaN behind"""
    buf = _nan(t.shape[0], ld)
    buf[:, :512] = t.to(DEV)
    return buf


def _ln_data(rows):
    """x, residual, gamma, beta of one row count: values every format under test represents exactly (x: fp16 values; residual:
    multiples of 1/32 below 4, exact in bf16 and fp16), each handed over in every format"""
    if rows not in _LN_DATA:
        g = torch.Generator().manual_seed(100 + rows)
        x = (torch.randn(rows, 512, generator=g) * 3 + 1).to(torch.float16).float()
        r = torch.randint(-127, 128, (rows, 512), generator=g).float() / 32
        gamma = (torch.randn(512, generator=g)).to(torch.bfloat16).float()
        beta = (torch.randn(512, generator=g)).to(torch.bfloat16).float()
        assert torch.equal(r.to(torch.bfloat16).float(), r) and torch.equal(r.to(torch.float16).float(), r)
        assert torch.equal(Q.unpack_split(Q.pack_split(r)), r)
        _LN_DATA[rows] = dict(
            x=x, r=r, gamma=gamma.to(DEV), beta=beta.to(DEV),
            x_in={0: _pitched(x, LD), 1: _pitched(Q.to_half_rows_f16(x), LD)},
            r_in={"f32": _pitched(r, LDR), "split": _pitched(Q.pack_split(r), LDR), "bf16": _pitched(Q.to_half_rows(r), LDR),
                  "f16": _pitched(Q.to_half_rows_f16(r), LDR)})
    return _LN_DATA[rows]


def _ln(L, d, rows, relu=0, out_fmt=0, resid="none", x_f16=0, gamma=None, y=None, ldy=LDY, x=None):
    """one vlsat_k_layernorm_to call on the data of _ln_data -> the whole output buffer [rows + 1, ldy] (device)"""
    if y is None:
        y = _nan(rows + 1, ldy)
    rb = None if resid == "none" else d["r_in"][resid]
    xb = d["x_in"][x_f16] if x is None else x
    L.check(L.load().vlsat_k_layernorm_to(xb.data_ptr(), xb.stride(0), y.data_ptr(), ldy, rows, 512,
                                          (d["gamma"] if gamma is None else gamma).data_ptr(), d["beta"].data_ptr(), relu, out_fmt,
                                          L.ptr(rb), 0 if rb is None else LDR, RESID_FMT[resid], x_f16, L.stream_ptr()))
    _sync()
    return y


def _ln_values(y, rows, out_fmt):
    """the [rows, 512] values an output buffer holds, as fp32 on the CPU; asserts that the rest of the buffer kept its fill: the
    pitch gap, the row behind the last and, for a half-row output, everything beyond byte 1024 of each row"""
    used = 512 if out_fmt in (0, 1) else 256
    assert _untouched(y[:rows, used:]) and _untouched(y[rows:]), f"layernorm (output format {out_fmt}) wrote outside its rows"
    w = y[:rows, :used].contiguous().cpu()
    if out_fmt == 0:
        return w
    if out_fmt == 1:
        return Q.unpack_split(w)
    return w.view(torch.bfloat16 if out_fmt == 2 else torch.float16).float()


@pytest.mark.parametrize("rows", LN_ROWS)
def test_layernorm_fp32_form_vs_fp64(lib, rows):
    d = _ln_data(rows)
    for relu in (0, 1):
        for resid in ("none", "f32"):
            got = _ln_values(_ln(lib, d, rows, relu=relu, resid=resid), rows, 0)
            xin = d["x"].double() + (d["r"].double() if resid != "none" else 0)
            ref = torch.nn.functional.layer_norm(xin, (512,), d["gamma"].double().cpu(), d["beta"].double().cpu(), 1e-5)
            if relu:
                ref = ref.clamp_min(0)
            err = float((got.double() - ref).abs().max())
            assert err < 2e-5, f"rows {rows} relu {relu} resid {resid}: {err:.3e}"


@pytest.mark.parametrize("rows", LN_ROWS)
def test_layernorm_input_formats_are_bit_identical_to_fp32_input(lib, rows):
    """residual {none, fp32, split pairs, bf16 half rows, fp16 half rows} x x as fp32 / fp16 half rows x ReLU: the same numbers
    in another format give the same bits"""
    d = _ln_data(rows)
    for relu in (0, 1):
        base = {"none": _ln_values(_ln(lib, d, rows, relu=relu), rows, 0),
                "f32": _ln_values(_ln(lib, d, rows, relu=relu, resid="f32"), rows, 0)}
        assert not torch.equal(base["none"], base["f32"])
        for resid in RESID_FORMS:
            for x_f16 in (0, 1):
                got = _ln_values(_ln(lib, d, rows, relu=relu, resid=resid, x_f16=x_f16), rows, 0)
                want = base["none" if resid == "none" else "f32"]
                assert torch.isfinite(got).all()
                assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"rows {rows} relu {relu} resid {resid} x_f16 {x_f16}"


@pytest.mark.parametrize("rows", LN_ROWS)
def test_layernorm_output_formats(lib, rows):
    """each output format holds the format's rounding of the fp32-output result of the same call"""
    d = _ln_data(rows)
    for relu, resid, x_f16 in ((0, "none", 0), (1, "split", 0), (0, "bf16", 1), (1, "f16", 1), (0, "f32", 0)):
        f32 = _ln_values(_ln(lib, d, rows, relu=relu, resid=resid, x_f16=x_f16), rows, 0)
        kw = dict(relu=relu, resid=resid, x_f16=x_f16)
        y1 = _ln(lib, d, rows, out_fmt=1, **kw)
        _ln_values(y1, rows, 1)
        assert torch.equal(y1[:rows, :512].cpu().view(torch.int32), Q.pack_split(f32).view(torch.int32)), f"split pairs {kw}"
        y2 = _ln_values(_ln(lib, d, rows, out_fmt=2, **kw), rows, 2)
        assert torch.equal(y2.view(torch.int32), f32.to(torch.bfloat16).float().view(torch.int32)), f"bf16 half rows {kw}"
        y4 = _ln_values(_ln(lib, d, rows, out_fmt=4, **kw), rows, 4)
        assert torch.equal(y4.view(torch.int32), Q.to_f16(f32).float().view(torch.int32)), f"fp16 half rows {kw}"


@pytest.mark.parametrize("rows", [5, 4099])
def test_layernorm_residual_and_output_in_one_buffer(lib, rows):
    """as the forward does with the edge rows: y = resid, same pitch, same format"""
    d = _ln_data(rows)
    for form, fmt in (("f32", 0), ("split", 1), ("bf16", 2), ("f16", 4)):
        for x_f16 in (0, 1):
            want = _ln_values(_ln(lib, d, rows, relu=1, out_fmt=fmt, resid=form, x_f16=x_f16, ldy=LDR), rows, fmt)
            buf = torch.cat([d["r_in"][form], _nan(1, LDR)])
            L = lib
            L.check(L.load().vlsat_k_layernorm_to(d["x_in"][x_f16].data_ptr(), LD, buf.data_ptr(), LDR, rows, 512, d["gamma"].data_ptr(),
                                                  d["beta"].data_ptr(), 1, fmt, buf.data_ptr(), LDR, fmt, x_f16, L.stream_ptr()))
            _sync()
            used = 512 if fmt in (0, 1) else 256
            assert _untouched(buf[rows:]) and _untouched(buf[:rows, 512:])
            got = buf[:rows, :used].contiguous().cpu()
            got = got if fmt == 0 else Q.unpack_split(got) if fmt == 1 else got.view(torch.bfloat16 if fmt == 2 else torch.float16).float()
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"rows {rows} format {fmt} x_f16 {x_f16}"


def test_layernorm_constant_row_gives_beta_exactly(lib):
    """a row of 512 equal values: the sum and the x 1/512 are exact, so the centred row is exactly zero and y = beta (max(beta, 0)
    with the ReLU) to the bit"""
    d = _ln_data(5)
    consts = torch.tensor([3.5, -2.25, 1000.0, 0.0, 0.001953125])
    x = consts[:, None].expand(5, 512).contiguous()
    assert torch.equal(x.to(torch.float16).float(), x)
    beta = d["beta"].cpu()
    for x_f16, xb in ((0, _pitched(x, LD)), (1, _pitched(Q.to_half_rows_f16(x), LD))):
        for relu in (0, 1):
            got = _ln_values(_ln(lib, d, 5, relu=relu, x_f16=x_f16, x=xb), 5, 0)
            want = (beta.clamp_min(0) if relu else beta)[None].expand(5, 512)
            assert torch.equal(got, want), f"x_f16 {x_f16} relu {relu}: {float((got - want).abs().max()):.3e}"


def test_layernorm_fp16_output_saturates(lib):
    """gamma = 1e5: results beyond the fp16 range are stored as +-65504, never inf"""
    rows = 4
    d = _ln_data(rows)
    gamma = torch.full((512,), 1e5, device=DEV)
    f32 = _ln_values(_ln(lib, d, rows, gamma=gamma), rows, 0)
    got = _ln_values(_ln(lib, d, rows, gamma=gamma, out_fmt=4), rows, 4)
    assert float(f32.max()) > 65504 and float(f32.min()) < -65504
    assert torch.isfinite(got).all() and float(got.max()) == 65504.0 and float(got.min()) == -65504.0
    assert torch.equal(got, Q.to_f16(f32).float())


def test_layernorm_variance_of_an_offset_row(lib):
    """mean 1000, sigma 1: within 2e-5 * |mean| / sigma of fp64.  A two-pass fp32 LayerNorm measures 4.5e-4 here and a one-pass
    variance (E[x^2] - mean^2) 1.0, so this pins the variance algorithm."""
    rows = 3
    d = _ln_data(rows)
    x = 1000 + torch.randn(rows, 512, generator=torch.Generator().manual_seed(8))
    one, zero = torch.ones(512, device=DEV), torch.zeros(512, device=DEV)
    y = _nan(rows + 1, LDY)
    xb = _pitched(x, LD)
    lib.check(lib.load().vlsat_k_layernorm_to(xb.data_ptr(), LD, y.data_ptr(), LDY, rows, 512, one.data_ptr(), zero.data_ptr(), 0, 0, 0, 0, 0, 0,
                                              lib.stream_ptr()))
    _sync()
    got = _ln_values(y, rows, 0)
    ref = torch.nn.functional.layer_norm(x.double(), (512,), None, None, 1e-5)
    err = float((got.double() - ref).abs().max())
    print(f"layernorm offset row: max err {err:.3e}")
    assert err <= 2e-5 * 1000 / 1.0


@pytest.mark.parametrize("out_fmt,x_f16", [(3, 0), (5, 0), (-1, 0), (8, 0), (0, 2), (0, -1), (2, 3)])
def test_layernorm_refuses_unknown_formats(lib, out_fmt, x_f16):
    """an out_fmt outside {0, 1, 2, 4} used to fall through to the fp32 store; now it is refused, and nothing is written"""
    d = _ln_data(4)
    y = _nan(5, LDY)
    with pytest.raises(lib.VlsatError, match="layernorm"):
        lib.check(lib.load().vlsat_k_layernorm_to(d["x_in"][0].data_ptr(), LD, y.data_ptr(), LDY, 4, 512, d["gamma"].data_ptr(), d["beta"].data_ptr(),
                                                  0, out_fmt, 0, 0, 0, x_f16, lib.stream_ptr()))
    _sync()
    assert _untouched(y)


# ---- glue kernels ---------------------------------------------------------------------------------------------------------
def _rel_conv1():
    w = synth.make_weights(VLSATConfig())
    w1 = np.concatenate([w["rel_encoder_3d.conv1.weight"][:, :, 0], w["rel_encoder_2d.conv1.weight"][:, :, 0]], 0)
    b1 = np.concatenate([w["rel_encoder_3d.conv1.bias"], w["rel_encoder_2d.conv1.bias"]], 0)
    return torch.from_numpy(np.ascontiguousarray(w1)), torch.from_numpy(np.ascontiguousarray(b1))


@pytest.mark.parametrize("source", ["synth", "random"])
@pytest.mark.parametrize("E", [1, 63, 64, 65, 129, 1560])
def test_edge_embed_vs_oracle(lib, E, source):
    if source == "synth":
        b = synth.make_batch(1, 40, 32, seed0=900)
        desc, ei = torch.from_numpy(b["descriptor"]), torch.from_numpy(b["edge_indices"])[:, :E]
    else:
        g = torch.Generator().manual_seed(E)
        desc = torch.rand(23, 11, generator=g) * 5 + 0.05
        ei = torch.randint(0, 23, (2, E), generator=g)
    assert ei.shape[1] == E and bool((desc[:, 6:] > 0).all())
    w1, b1 = _rel_conv1()
    ref = torch.relu(O.edge_descriptor(desc.double(), ei) @ w1.double().t() + b1.double())
    h1 = _nan(E + 3, 128)
    dd, src, dst = desc.to(DEV), ei[0].to(torch.int32).to(DEV), ei[1].to(torch.int32).to(DEV)
    w1d, b1d = w1.to(DEV), b1.to(DEV)
    lib.check(lib.load().vlsat_k_edge_embed(dd.data_ptr(), src.data_ptr(), dst.data_ptr(), E, w1d.data_ptr(), b1d.data_ptr(), h1.data_ptr(),
                                            lib.stream_ptr()))
    _sync()
    assert _untouched(h1[E:]), "edge_embed wrote rows >= E"
    err = float((h1[:E].cpu().double() - ref).abs().max())
    assert err <= 2e-5 * max(1.0, float(ref.abs().max())), f"edge_embed E={E} {source}: {err:.3e}"


@pytest.mark.parametrize("N", [1, 31, 32, 33])
def test_desc_tail(lib, N):
    g = torch.Generator().manual_seed(N)
    desc = torch.rand(N, 11, generator=g) * 5 + 0.05
    desc[:, 3:9] -= 2.0                                       # the copied columns may hold anything
    x = _nan(N + 1, 520)
    dd = desc.to(DEV)
    lib.check(lib.load().vlsat_k_desc_tail(dd.data_ptr(), N, x.data_ptr(), 520, 504, lib.stream_ptr()))
    _sync()
    assert _untouched(x[:N, :504]) and _untouched(x[:N, 512:]) and _untouched(x[N:]), "desc_tail wrote outside its 8 columns"
    got = x[:N, 504:512].cpu()
    assert torch.equal(got[:, :6].view(torch.int32), desc[:, 3:9].contiguous().view(torch.int32))
    err = float((got[:, 6:].double() - desc[:, 9:11].double().log()).abs().max())
    assert err <= 2e-5, f"desc_tail log columns: {err:.3e}"


def _invnorm(L, x, rows, scale, x2=None):
    out, out2 = _nan(rows + 2), (None if x2 is None else _nan(rows + 2))
    L.check(L.load().vlsat_k_row_invnorm(x.data_ptr(), x.stride(0), rows, 512, scale, out.data_ptr(), L.ptr(x2), L.ptr(out2), L.stream_ptr()))
    _sync()
    assert _untouched(out[rows:]) and (out2 is None or _untouched(out2[rows:]))
    return (out[:rows].cpu(), None if out2 is None else out2[:rows].cpu())


@pytest.mark.parametrize("rows", [1, 4, 5, 2561])
def test_row_invnorm(lib, rows):
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, 768, generator=g) * (torch.rand(rows, 1, generator=g) * 10 + 0.01)
    x2 = torch.randn(rows, 768, generator=g)
    scale = 1.0 / 0.07
    xd, x2d = x.to(DEV), x2.to(DEV)
    a, _ = _invnorm(lib, xd, rows, scale)
    b, _ = _invnorm(lib, x2d, rows, scale)
    for got, src in ((a, x), (b, x2)):
        ref = float(np.float32(scale)) / src[:, :512].double().norm(dim=1)
        rel = float(((got.double() - ref).abs() / ref).max())
        assert rel <= 2e-6, f"row_invnorm rows {rows}: {rel:.3e}"
    ta, tb = _invnorm(lib, xd, rows, scale, x2d)
    assert torch.equal(ta, a) and torch.equal(tb, b), "twin launch differs from two single launches"


def test_row_invnorm_refuses_half_a_twin(lib):
    x = torch.randn(4, 768).to(DEV)
    out, out2 = _nan(4), _nan(4)
    l = lib.load()
    with pytest.raises(lib.VlsatError):
        lib.check(l.vlsat_k_row_invnorm(x.data_ptr(), 768, 4, 512, 1.0, out.data_ptr(), x.data_ptr(), 0, lib.stream_ptr()))
    with pytest.raises(lib.VlsatError):
        lib.check(l.vlsat_k_row_invnorm(x.data_ptr(), 768, 4, 512, 1.0, out.data_ptr(), 0, out2.data_ptr(), lib.stream_ptr()))
    _sync()
    assert _untouched(out) and _untouched(out2)


@pytest.mark.parametrize("rows,cols,dst_ld,src_ld,dst_off,src_off",
                         [(37, 512, 640, 768, 0, 0),         # 16-byte accesses
                          (8200, 512, 516, 520, 0, 0),       # ... more vectors than one pass of the grid
                          (37, 510, 640, 768, 0, 0),         # scalar: columns
                          (37, 512, 640, 768, 1, 0),         # scalar: destination 4 bytes off
                          (37, 512, 640, 768, 0, 1),         # scalar: source 4 bytes off
                          (5, 512, 642, 768, 0, 0),          # scalar: pitch
                          (1, 1, 8, 8, 0, 0)])
def test_copy_rows(lib, rows, cols, dst_ld, src_ld, dst_off, src_off):
    g = torch.Generator().manual_seed(rows + cols)
    src = torch.randn(rows * src_ld + 4, generator=g).to(DEV)
    dst = _nan(rows * dst_ld + 4)
    lib.check(lib.load().vlsat_k_copy_rows(dst.data_ptr() + 4 * dst_off, dst_ld, src.data_ptr() + 4 * src_off, src_ld, cols, rows, lib.stream_ptr()))
    _sync()
    d = dst[dst_off:dst_off + rows * dst_ld].view(rows, dst_ld)
    s = src[src_off:src_off + rows * src_ld].view(rows, src_ld)
    assert torch.equal(d[:, :cols], s[:, :cols])
    assert _untouched(d[:, cols:]) and _untouched(dst[:dst_off]) and _untouched(dst[dst_off + rows * dst_ld:]), "copy_rows wrote into the pitch gap"


@pytest.mark.parametrize("cin", [3, 6, 9])
def test_pts_conv1_rows(lib, cin):
    n, P = 3, 37
    pts, w = Q.pointnet_points(P, n, cin), Q.pointnet_weights("cfg", cin)
    ref = torch.relu(pts.double().transpose(1, 2) @ w[0].double().t() + w[1].double()).reshape(n * P, 64)
    rows = _nan(n * P + 1, 64)
    pd, w1, b1 = pts.to(DEV), w[0].contiguous().to(DEV), w[1].to(DEV)
    lib.check(lib.load().vlsat_k_pts_conv1_rows(pd.data_ptr(), n, P, cin, w1.data_ptr(), b1.data_ptr(), rows.data_ptr(), lib.stream_ptr()))
    _sync()
    assert _untouched(rows[n * P:])
    err = float((rows[:n * P].cpu().double() - ref).abs().max())
    assert err <= 2e-5, f"pts_conv1_rows cin {cin}: {err:.3e}"


@pytest.mark.parametrize("n,P,cols,ld,ldo", [(3, 37, 64, 72, 80), (5, 1, 50, 52, 56), (2, 300, 1024, 1024, 1028)])
def test_rowmax(lib, n, P, cols, ld, ldo):
    g = torch.Generator().manual_seed(P)
    x = torch.randn(n * P, ld, generator=g)
    out = _nan(n + 1, ldo)
    xd = x.to(DEV)
    lib.check(lib.load().vlsat_k_rowmax(xd.data_ptr(), ld, n, P, cols, out.data_ptr(), ldo, lib.stream_ptr()))
    _sync()
    assert _untouched(out[:n, cols:]) and _untouched(out[n:])
    assert torch.equal(out[:n, :cols].cpu(), x.view(n, P, ld)[:, :, :cols].amax(1))


def test_apply_stn(lib):
    """out[r] = h[r] . T[r // P] with a non-symmetric T per object (a transposed T would show), a row count that is no multiple of
    the 4 rows of a block"""
    n, P, ldh, ldo = 3, 37, 72, 80
    g = torch.Generator().manual_seed(4)
    h = torch.randn(n * P, ldh, generator=g)
    T = torch.randn(n, 64, 64, generator=g) / 8 + torch.triu(torch.ones(64, 64), 1) * 0.25
    assert (n * P) % 4 and float((T - T.transpose(1, 2)).abs().amax((1, 2)).min()) > 0.1
    ref = torch.bmm(h.view(n, P, ldh)[:, :, :64].double(), T.double()).reshape(n * P, 64)
    out = _nan(n * P + 1, ldo)
    hd, Td = h.to(DEV), T.contiguous().to(DEV)
    lib.check(lib.load().vlsat_k_apply_stn(hd.data_ptr(), ldh, Td.data_ptr(), n * P, P, out.data_ptr(), ldo, lib.stream_ptr()))
    _sync()
    assert _untouched(out[:n * P, 64:]) and _untouched(out[n * P:])
    err = float((out[:n * P, :64].cpu().double() - ref).abs().max())
    wrong = float((torch.bmm(h.view(n, P, ldh)[:, :, :64].double(), T.double().transpose(1, 2)).reshape(n * P, 64) - ref).abs().max())
    assert err <= 2e-5 * max(1.0, float(ref.abs().max())) < wrong, f"apply_stn: {err:.3e}"


def test_split_bf16_planes(lib):
    """hi / lo of vlsat_k_split_bf16 equal the host split bit for bit: random values over many binades, exact round-to-nearest
    ties (low half 0x8000 under an even and under an odd upper half, both signs), +-0 and residuals that are denormal"""
    g = torch.Generator().manual_seed(6)
    ties = torch.tensor([0x3F808000, 0x3F818000, 0x40FE8000, 0x40FF8000, 0x3F807FFF, 0x3F808001], dtype=torch.int32)
    special = torch.cat([ties, ties | -2147483648, torch.tensor([0, -2147483648], dtype=torch.int32)]).view(torch.float32)
    tiny = torch.tensor([2.0 ** -120 * (1 + 2.0 ** -10), -(2.0 ** -118) * (1 + 2.0 ** -9 + 2.0 ** -15), 2.0 ** -126 * 1.00390625, 2.0 ** -130, 2.0 ** -149])
    x = torch.cat([special, tiny, torch.randn(1000, generator=g) * torch.exp2(torch.randint(-30, 30, (1000,), generator=g).float())])
    n = x.numel()
    assert n % 256
    hi = torch.full((n + 64,), 0x5555, dtype=torch.int16, device=DEV)
    lo = torch.full((n + 64,), 0x5555, dtype=torch.int16, device=DEV)
    xd = x.to(DEV)
    lib.check(lib.load().vlsat_k_split_bf16(xd.data_ptr(), n, hi.data_ptr(), lo.data_ptr(), lib.stream_ptr()))
    _sync()
    assert bool((hi[n:] == 0x5555).all()) and bool((lo[n:] == 0x5555).all())
    w = Q.pack_split(x).view(torch.int32)
    want_hi, want_lo = (w >> 16).to(torch.int16), (w & 0xFFFF).to(torch.int16)
    assert torch.equal(hi[:n].cpu(), want_hi), "hi plane"
    assert torch.equal(lo[:n].cpu(), want_lo), "lo plane"
    # the ties went to the even neighbour
    assert hi[:4].cpu().tolist() == [0x3F80, 0x3F82, 0x40FE, 0x4100]


# ---- node attention: several key chunks, unequal pitches, hard biases -------------------------------------------------------
NA_SIZES = [2, 3, 64, 65, 129, 257]
LDQ, LDK, LDV, LDO = 512, 640, 768, 576


def _node_attn(L, q, k, v, bias, sizes, H, lanes):
    """q, k, v [N, 512] and bias (flat, [H][n][n] per scene) on the CPU -> O [N, 512] on the CPU through buffers of pitch 512 / 640 /
    768 / 576; O's pitch gap must keep its fill"""
    N = q.shape[0]
    bufs = []
    for t, ld in ((q, LDQ), (k, LDK), (v, LDV)):
        b = _nan(N, ld)
        b[:, :512] = t.to(DEV)
        bufs.append(b)
    o = _nan(N + 1, LDO)
    node_ptr = torch.tensor([0] + list(np.cumsum(sizes)), dtype=torch.int64)
    bd = None if bias is None else bias.to(DEV)
    L.check(L.load().vlsat_k_node_attn(bufs[0].data_ptr(), LDQ, bufs[1].data_ptr(), LDK, bufs[2].data_ptr(), LDV, o.data_ptr(), LDO, L.ptr(bd),
                                       node_ptr.data_ptr(), len(sizes), H, 1.0 / math.sqrt(512 // H), lanes, L.stream_ptr()))
    _sync()
    assert _untouched(o[:N, 512:]) and _untouched(o[N:]), "node_attn wrote into O's pitch gap"
    got = o[:N, :512].cpu()
    assert torch.isfinite(got).all()
    return got


def _ref_node_attn(q, k, v, biases, sizes, H):
    """fp64 softmax attention per scene; biases: list of [H, n, n]"""
    dk = 512 // H
    out, lo = [], 0
    for n, b in zip(sizes, biases):
        qs, ks, vs = (t[lo:lo + n].double().view(n, H, dk).permute(1, 0, 2) for t in (q, k, v))
        att = torch.softmax(qs @ ks.transpose(1, 2) / math.sqrt(dk) + b.double(), -1)
        out.append((att @ vs).permute(1, 0, 2).reshape(n, 512))
        lo += n
    return torch.cat(out)


def _na_inputs(H, seed):
    g = torch.Generator().manual_seed(seed)
    N = sum(NA_SIZES)
    q, k, v = (torch.randn(N, 512, generator=g) for _ in range(3))
    biases = [torch.randn(H, n, n, generator=g) for n in NA_SIZES]
    return q, k, v, biases


def _flat(biases):
    return torch.cat([b.reshape(-1) for b in biases])


@pytest.mark.parametrize("lanes", [1, 16])
@pytest.mark.parametrize("H", [4, 8, 16])
def test_node_attn_many_chunks_random_bias(lib, H, lanes):
    """scenes of 2 .. 257 nodes (up to five 64-key chunks; with 2 or 3 nodes some key phases of the sixteen-lane kernel see no
    key), head dims 128 / 64 / 32, a random bias, and one late key that dominates a query (online rescale)"""
    q, k, v, biases = _na_inputs(H, 10 * H + lanes)
    lo = 0
    for n in NA_SIZES:                        # the last key of every scene = 3 x one of its queries: in the last chunk
        k[lo + n - 1] = 3.0 * q[lo + (n // 2)]
        lo += n
    got = _node_attn(lib, q, k, v, _flat(biases), NA_SIZES, H, lanes)
    ref = _ref_node_attn(q, k, v, biases, NA_SIZES, H)
    tol = 1e-5 * max(1.0, float(v.abs().max()))
    lo = 0
    for n in NA_SIZES:
        err = float((got[lo:lo + n].double() - ref[lo:lo + n]).abs().max())
        assert err < tol, f"H={H} lanes={lanes} scene of {n}: {err:.2e} (tolerance {tol:.2e})"
        lo += n


@pytest.mark.parametrize("lanes", [1, 16])
@pytest.mark.parametrize("H", [4, 8, 16])
def test_node_attn_strongly_negative_bias_removes_keys(lib, H, lanes):
    """a bias of -1e4 on a third of the keys: they contribute exactly nothing -- the result equals, at the usual tolerance (the
    chunking differs, so not to the bit), the run on scenes from which those nodes were removed"""
    q, k, v, biases = _na_inputs(H, 20 * H + lanes)
    keep_rows, kept_sizes, kept_biases = [], [], []
    lo = 0
    for n, b in zip(NA_SIZES, biases):
        drop = torch.arange(n) % 3 == 1
        b[:, :, drop] = -1e4
        keep = (~drop).nonzero()[:, 0]
        keep_rows.append(lo + keep)
        kept_sizes.append(len(keep))
        kept_biases.append(b[:, keep][:, :, keep].contiguous())
        lo += n
    rows = torch.cat(keep_rows)
    full = _node_attn(lib, q, k, v, _flat(biases), NA_SIZES, H, lanes)
    kept = _node_attn(lib, q[rows], k[rows], v[rows], _flat(kept_biases), kept_sizes, H, lanes)
    tol = 1e-5 * max(1.0, float(v.abs().max()))
    err = float((full[rows] - kept).abs().max())
    assert err < tol, f"H={H} lanes={lanes}: masked keys leak {err:.2e}"
    ref = _ref_node_attn(q[rows], k[rows], v[rows], kept_biases, kept_sizes, H)
    err = float((full[rows].double() - ref).abs().max())
    assert err < tol, f"H={H} lanes={lanes}: {err:.2e}"
