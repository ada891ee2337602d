"""The split-fp16 PointNet of the fp32 precision mode (csrc/pointnet_bf16.hip, TERMS = 5) through vlsat_k_pointnet_ex(terms = 5): conv2 /
conv3 as three fp16 MFMAs per product on the planes of gemm_f16s_planes.h, fp32 tensors in and out, fp32-grade error.  Inputs: every case
of quant_model.POINTNET_CASES (3 / 6 / 9 channels, 128 / 384 / 768 outputs, 1 / 127 / 128 / 129 / 300 points).
Bound, the rule of the two other split-fp16 tests: max |got - fp64| <= max(4 x the exact kernel's (terms = 0) error on the same input,
2^-23 max |ref|).  Every output buffer is pre-filled with NaN; the words behind the [n, n_out] block must still hold it.
Needs an MI355X:  pytest -m gpu"""
import pytest
import torch

import vlsat_amd  # noqa: F401
import quant_model as Q

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN_BITS = 0x7FC00000
FS = 5                    # terms of the split-fp16 form


@pytest.fixture(scope="module")
def lib():
    from vlsat_amd import lib as L
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path cannot run and there is no fallback")
    return L


def _pointnet_ex(L, pts, w, terms):
    """pts [n, cin, P] (device), w = (w1, b1, w2, b2, w3, b3) (device) -> [n, n_out] on the CPU; asserts that the 128 words behind the
    output block come back untouched"""
    n, cin, P = pts.shape
    n_out = w[4].shape[0]
    buf = torch.full((n * n_out + 128,), float("nan"), device=DEV)
    L.check(L.load().vlsat_k_pointnet_ex(pts.data_ptr(), n, P, cin, *(t.data_ptr() for t in w[:6]), n_out, terms, buf.data_ptr(),
                                         L.stream_ptr()))
    torch.cuda.synchronize()
    assert bool((buf[n * n_out:].view(torch.int32) == NAN_BITS).all()), "pointnet wrote behind its [n, n_out] block"
    return buf[:n * n_out].view(n, n_out).cpu()


def _dev(w):
    return tuple(t.contiguous().to(DEV) for t in w)


_GOT = {}


def _case(L, name, terms):
    """the kernel's output for one input of quant_model.POINTNET_CASES, computed once per (input, terms)"""
    if (name, terms) not in _GOT:
        pts, w = Q.pointnet_case(name)
        _GOT[name, terms] = _pointnet_ex(L, pts.to(DEV), _dev(w), terms)
    return _GOT[name, terms]


@pytest.mark.parametrize("name", sorted(Q.POINTNET_CASES))
def test_error_within_4x_of_the_exact_kernel(lib, name):
    ref = Q.pointnet_case_exact(name)
    got, exact = _case(lib, name, FS), _case(lib, name, 0)
    assert torch.isfinite(got).all()
    e_new, e_exact = float((got.double() - ref).abs().max()), float((exact.double() - ref).abs().max())
    floor = 2.0 ** -23 * float(ref.abs().max())
    print(f"pointnet split-fp16 {name}: {e_new:.3e} against the exact kernel's {e_exact:.3e} ({e_new / max(e_exact, 1e-30):.2f} x), "
          f"2^-23 max|ref| {floor:.3e}")
    assert e_new <= max(4 * e_exact, floor), f"{name}: {e_new:.3e} > max(4 x {e_exact:.3e}, {floor:.3e})"


def test_object_alone_equals_object_in_batch(lib):
    """An object computed alone (its chunks spread over several blocks that merge with atomicMax) equals, bit for bit, the same object
    inside the 600-object batch (one block per object, plain stores)."""
    pts, w = Q.pointnet_case("p300_n600")
    wd = _dev(w)
    batch = _case(lib, "p300_n600", FS)
    for i in (0, 17, 599):
        alone = _pointnet_ex(lib, pts[i:i + 1].contiguous().to(DEV), wd, FS)
        assert torch.equal(alone[0], batch[i]), f"object {i}: {float((alone[0] - batch[i]).abs().max()):.3e}"


@pytest.mark.parametrize("name", ["p300_n1", "p129_n3_c9", "p127_n3_c6"])
def test_point_order_does_not_matter(lib, name):
    pts, w = Q.pointnet_case(name)
    perm = torch.randperm(pts.shape[2], generator=torch.Generator().manual_seed(5))
    got = _pointnet_ex(lib, pts[:, :, perm].contiguous().to(DEV), _dev(w), FS)
    assert torch.equal(got, _case(lib, name, FS))


def test_two_launches_are_bit_equal(lib):
    pts, w = Q.pointnet_case("p300_n3_o384")
    again = _pointnet_ex(lib, pts.to(DEV), _dev(w), FS)
    assert torch.equal(again, _case(lib, "p300_n3_o384", FS))


@pytest.mark.parametrize("name", ["p300_n1", "p129_n1_c6_o128", "p300_n600"])
def test_all_zero_weights_give_zeros(lib, name):
    """every weight and bias zero (plane exponent 0, all planes zero): exactly +0.0 everywhere, nothing behind the block"""
    pts, w = Q.pointnet_case(name)
    got = _pointnet_ex(lib, pts.to(DEV), tuple(torch.zeros_like(t).to(DEV) for t in w), FS)
    assert torch.equal(got.view(torch.int32), torch.zeros_like(got, dtype=torch.int32))


def test_zero_conv_weights_give_the_bias(lib):
    """conv2 / conv3 weights zero: the output is relu(b3) exactly, whatever the points are (2^-k of an all-zero tensor is 1)"""
    pts, w = Q.pointnet_case("p129_n3_c9")
    w = (w[0], w[1], torch.zeros_like(w[2]), w[3], torch.zeros_like(w[4]), w[5])
    got = _pointnet_ex(lib, pts.to(DEV), _dev(w), FS)
    assert torch.equal(got, torch.relu(w[5]).expand_as(got))


def test_activations_beyond_the_fp16_range_saturate(lib):
    """points x 1e6: H1 reaches 1e5 and more, the operand saturates at 65504 -- finite results, no NaN"""
    pts, w = Q.pointnet_case("p129_n3_c9")
    got = _pointnet_ex(lib, (pts * 1e6).to(DEV), _dev(w), FS)
    assert torch.isfinite(got).all()
