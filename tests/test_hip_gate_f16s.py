"""The split-fp16 edge gate of the fp32 mode (csrc/edge_gate_f16s.hip; vlsat_k_edge_gate variant 5: three fp16 MFMAs per product)
against the fp64 reference that tests/test_hip_gcn_kernels.py builds for the fp32 kernels, at THEIR tolerance (2e-5 relative), with the
error of the exact kernel (variant 0) on the same inputs printed next to it; then zero and -0.0 rows, inputs beyond the fp16 domain,
the geometries it refuses, and that a row's bits depend on the row alone.  Needs an MI355X:  pytest -m gpu"""
import pytest
import torch

import vlsat_amd  # noqa: F401
from oracle import vlsat_oracle as O
from test_hip_gcn_kernels import _dev, _gate_weights, _random_edges

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
H, A, DK, DOX = 8, 256, 64, 32
TOL = 2e-5          # test_hip_gcn_kernels.VARIANTS: the bound of the fp32 kernels


@pytest.fixture(scope="module")
def lib():
    from vlsat_amd import lib as L
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path cannot run and there is no fallback")
    return L


def _operands(kind, use_edge, seed, n, e):
    """reference-layout tensors in fp64 -> the prepared operands of the gate, as _gate_case makes them"""
    g = torch.Generator().manual_seed(1000 * H + A + seed)
    w = _gate_weights(g, H, A, use_edge)
    ei = _random_edges(g, n, e, kind)
    E = ei.shape[1]
    x = torch.randn(n, 512, generator=g, dtype=F64)
    ed = torch.randn(E, 512, generator=g, dtype=F64)
    p = "g.edgeatten."
    q = O.lin(x, w, p + "proj_query.0").view(n, DK, H)
    k = O.lin(ed, w, p + "proj_edge.0").view(E, DK, H).permute(0, 2, 1).reshape(E, H * DK)
    v = O.lin(x, w, p + "proj_value.0").view(n, DOX, H).permute(0, 2, 1).reshape(n, H * DOX)
    W0, b0 = w[p + "nn.0.weight"][:, :, 0], w[p + "nn.0.bias"]
    W3, b3 = w[p + "nn.3.weight"][:, :, 0], w[p + "nn.3.bias"]
    gq = (torch.einsum("oc,nch->nho", W0[:, :DK], q) + b0[None, None, :]).reshape(n, H * 2 * DK)
    w0k = W0[:, DK:] if use_edge else torch.zeros(2 * DK, DK, dtype=F64)
    ops = dict(k=k, gq=gq, v=v, w0k=w0k, w3=W3, b3=b3, ei=ei, n=n, use_edge=use_edge)
    return ops, (x, ed, ei, w)


def _launch(L, ops, variant):
    """-> gated [E, A] head-major, prob [E, d_o, H], both as the kernel wrote them (fp32, on the host)"""
    n, ei = ops["n"], ops["ei"]
    E = ei.shape[1]
    node = torch.cat([ops["gq"], ops["v"], torch.zeros(n, 4, dtype=F64)], 1)
    d_node, d_k = _dev(node), _dev(ops["k"])
    d_src, d_dst = ei[0].to(torch.int32).to(DEV), ei[1].to(torch.int32).to(DEV)
    d_w0k, d_w3, d_b3 = _dev(ops["w0k"]), _dev(ops["w3"]), _dev(ops["b3"])
    gated = torch.full((E, A), float("nan"), device=DEV)
    prob = torch.full((E, DOX, H), float("nan"), device=DEV)
    L.check(L.load().vlsat_k_edge_gate(d_k.data_ptr(), d_node.data_ptr(), node.shape[1], 0, H * 2 * DK, d_src.data_ptr(), d_dst.data_ptr(),
                                       d_w0k.data_ptr(), d_w3.data_ptr(), d_b3.data_ptr(), gated.data_ptr(), prob.data_ptr(), E, H, DK, DOX,
                                       1 if ops["use_edge"] else 0, variant, L.stream_ptr()))
    torch.cuda.synchronize()
    return gated.cpu(), prob.cpu()


def _ref_from_operands(ops):
    """the gate in fp64 on the fp32-rounded prepared operands (gate_core.h: per (edge, head) row)"""
    f = lambda t: t.to(torch.float32).double()
    ei = ops["ei"]
    E = ei.shape[1]
    k = f(ops["k"]).view(E, H, DK)
    gq = f(ops["gq"]).view(-1, H, 2 * DK)[ei[0]]
    hid = gq.clone()
    if ops["use_edge"]:
        hid = hid + torch.einsum("oc,ehc->eho", f(ops["w0k"]), k)
    hid = hid.clamp_min(0)
    logits = torch.einsum("mo,eho->ehm", f(ops["w3"]), hid) + f(ops["b3"])
    prob = torch.softmax(logits, -1)                                   # [E, H, d_o]
    gated = prob * f(ops["v"]).view(-1, H, DOX)[ei[1]]
    return gated.permute(0, 2, 1).reshape(E, A), prob.permute(0, 2, 1)          # the reference's layouts: channel m * H + h; [E, d_o, H]


def _errors(L, ops, ref_gated, ref_prob, variant):
    gated, prob = _launch(L, ops, variant)
    E = gated.shape[0]
    got = gated.double().view(E, H, DOX).permute(0, 2, 1).reshape(E, A)      # head-major -> the reference's m * H + h
    assert torch.isfinite(got).all() and torch.isfinite(prob).all()
    scale = max(1.0, float(ref_gated.abs().max()))
    return float((got - ref_gated).abs().max()) / scale, float((prob.double() - ref_prob).abs().max()), prob


CASES = [("random", True, n, e) for n in (9, 23) for e in (1, 31, 32, 33, 65, 777)] + \
        [("fc", True, 9, 0), ("fc", True, 23, 0), ("random", False, 9, 33), ("random", False, 23, 777), ("fc", False, 23, 0)]


@pytest.mark.parametrize("kind,use_edge,n,e", CASES)
def test_gate_f16s_vs_fp64_reference(lib, kind, use_edge, n, e):
    """gated rows and the prob tap of variant 5 within 2e-5 (relative to max(1, max |reference|)) of oracle.edge_atten in fp64"""
    ops, (x, ed, ei, w) = _operands(kind, use_edge, seed=e, n=n, e=e)
    ref_gated, _, ref_prob = O.edge_atten(x, ed, ei, w, "g", H)
    err0, perr0, _ = _errors(lib, ops, ref_gated, ref_prob, 0)
    err5, perr5, prob = _errors(lib, ops, ref_gated, ref_prob, 5)
    print(f"{kind} use_edge={use_edge} n={n} E={ei.shape[1]}: split-fp16 gated {err5:.2e} prob {perr5:.2e} | exact gated {err0:.2e} prob {perr0:.2e}")
    assert err5 < TOL and perr5 < TOL, (err5, perr5)
    assert float((prob.double().sum(1) - 1).abs().max()) < 1e-5


def test_gate_f16s_zero_and_negative_zero_rows(lib):
    """kproj rows of +0.0 and of -0.0 (hidden = relu(Gq) exactly: both halves of a split zero are zero), among ordinary rows"""
    ops, _ = _operands("random", True, seed=3, n=9, e=65)
    k = ops["k"].clone()
    k[5] = 0.0
    k[6] = -0.0
    k[40:50] = 0.0
    k[64] = -0.0
    ops["k"] = k
    ref_gated, ref_prob = _ref_from_operands(ops)
    err5, perr5, _ = _errors(lib, ops, ref_gated, ref_prob, 5)
    err0, perr0, _ = _errors(lib, ops, ref_gated, ref_prob, 0)
    print(f"zero rows: split-fp16 gated {err5:.2e} prob {perr5:.2e} | exact gated {err0:.2e} prob {perr0:.2e}")
    assert err5 < TOL and perr5 < TOL, (err5, perr5)
    g5, _ = _launch(lib, ops, 5)
    neg = dict(ops, k=torch.where(k == 0, torch.full_like(k, -0.0), k))        # every zero as -0.0: the same rows bit for bit
    g5n, _ = _launch(lib, neg, 5)
    assert torch.equal(g5, g5n)


def test_gate_f16s_inputs_beyond_the_fp16_domain_saturate(lib):
    """kproj, Gq and value times 1e5 (|kproj| up to ~4e5 > 65504: the split clamps): finite outputs, probabilities that sum to one"""
    ops, _ = _operands("random", True, seed=4, n=23, e=777)
    big = dict(ops, k=ops["k"] * 1e5, gq=ops["gq"] * 1e5, v=ops["v"] * 1e5)
    gated, prob = _launch(lib, big, 5)
    assert torch.isfinite(gated).all() and torch.isfinite(prob).all()
    assert float((prob.double().sum(1) - 1).abs().max()) < 1e-5


def test_gate_f16s_refuses_other_head_geometries(lib):
    """variant 5 is the kernel of 8 heads x (64, 32): (16, 32, 8) is VLSAT_EINVAL, not a launch of another kernel"""
    node = torch.zeros(4, 16 * 64 + 128 + 4, device=DEV)
    k = torch.zeros(8, 512, device=DEV)
    idx = torch.zeros(8, dtype=torch.int32, device=DEV)
    w0k, w3, b3 = torch.zeros(64, 32, device=DEV), torch.zeros(8, 64, device=DEV), torch.zeros(8, device=DEV)
    gated = torch.zeros(8, 128, device=DEV)
    L = lib
    with pytest.raises(L.VlsatError) as ei:
        L.check(L.load().vlsat_k_edge_gate(k.data_ptr(), node.data_ptr(), node.shape[1], 0, 16 * 64, idx.data_ptr(), idx.data_ptr(), w0k.data_ptr(),
                                           w3.data_ptr(), b3.data_ptr(), gated.data_ptr(), None, 8, 16, 32, 8, 1, 5, L.stream_ptr()))
    assert ei.value.code == -1, ei.value           # VLSAT_EINVAL (include/vlsat.h)
    assert float(gated.abs().max()) == 0.0
    with pytest.raises(L.VlsatError):           # ... and 6 is no variant
        L.check(L.load().vlsat_k_edge_gate(k.data_ptr(), node.data_ptr(), node.shape[1], 0, 16 * 64, idx.data_ptr(), idx.data_ptr(), w0k.data_ptr(),
                                           w3.data_ptr(), b3.data_ptr(), gated.data_ptr(), None, 8, 16, 32, 8, 1, 6, L.stream_ptr()))


def test_gate_f16s_is_deterministic_and_a_row_depends_on_the_row_alone(lib):
    """Two calls give equal bits; and the rows of a list that is moved five edges down (other lanes, other waves, other blocks own
    every row) keep their bits -- what the engine's bit-identity tests of row maps, grids and twin launches rest on."""
    ops, _ = _operands("random", True, seed=7, n=23, e=777)
    g1, p1 = _launch(lib, ops, 5)
    g2, p2 = _launch(lib, ops, 5)
    assert torch.equal(g1, g2) and torch.equal(p1, p2)
    ei, k = ops["ei"], ops["k"]
    moved = dict(ops, ei=torch.cat([ei[:, 100:105], ei], 1), k=torch.cat([k[100:105], k], 0))
    g3, p3 = _launch(lib, moved, 5)
    assert torch.equal(g3[5:], g1) and torch.equal(p3[5:], p1)
    assert torch.equal(g3[:5], g1[100:105])
