"""LayerNorm kernel, output format 6: the row leaves as GEMM pair words (csrc/gemm_f16s_planes.h f16s_pair_pack: Ah << 16 | Al), packed
after scale, shift and the optional ReLU with the GEMM epilogues' own code -- what the fp32 mode's edge attention writes into E2 when its
only readers are split-fp16 A operands (csrc/edge_pairs.h, EdgePairs::e2).  Every word must equal pack(y32) BIT FOR BIT, y32 being the
fp32-format output of the same call and pack an independent numpy float16 implementation (tests/e2_pairs_pack.py, itself checked against
the header by tests/test_e2_pairs_cpu.py and once more here on the values the kernel produced).  Every output buffer is pre-filled with
NaN; what the kernel does not promise to write must still hold the fill afterwards.  Needs an MI355X:  pytest -m gpu"""
import numpy as np
import pytest
import torch

import vlsat_amd  # noqa: F401
import host_check
import e2_pairs_pack as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN_BITS = 0x7FC00000
LD, LDY, LDR = 520, 768, 640
ROWS = [1, 5, 4099]
# columns with planted scale / shift: gamma 0 with beta -0.0 (y = -0.0 wherever the centred value is negative), gamma 1e-5 and 1e-9 with
# beta 0 (|y| far below 2^-13: subnormal fp16 hi parts, lo parts below fp16's normal range even times 2^11), gamma 0 with beta 2^-14
COL_NEG0, COL_TINY, COL_TINIER, COL_SUB = (3, 258), (7, 300), (8, 511), (0, 260)


@pytest.fixture(scope="module")
def lib():
    from vlsat_amd import lib as L
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path cannot run and there is no fallback")
    return L


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _untouched(t):
    return bool((t.contiguous().view(torch.int32) == NAN_BITS).all())


def _pitched(t, ld):
    buf = _nan(t.shape[0], ld)
    buf[:, :512] = t.to(DEV)
    return buf


_DATA = {}


def _data(rows):
    if rows not in _DATA:
        g = torch.Generator().manual_seed(300 + rows)
        x = torch.randn(rows, 512, generator=g) * 3 + 1
        r = torch.randn(rows, 512, generator=g)
        x[0, COL_NEG0[0]] = -20.0                 # (a centred value that is negative with and without the residual: y = -0.0 there)
        gamma = torch.randn(512, generator=g)
        beta = torch.randn(512, generator=g)
        for c in COL_NEG0:
            gamma[c], beta[c] = 0.0, -0.0
        for c in COL_TINY:
            gamma[c], beta[c] = 1e-5, 0.0
        for c in COL_TINIER:
            gamma[c], beta[c] = 1e-9, 0.0
        for c in COL_SUB:
            gamma[c], beta[c] = 0.0, 2.0 ** -14
        _DATA[rows] = dict(x=x, r=r, gamma=gamma.to(DEV), beta=beta.to(DEV), xb=_pitched(x, LD), rb=_pitched(r, LDR))
    return _DATA[rows]


def _call(L, x, ldx, y, ldy, rows, gamma, beta, relu, out_fmt, resid=None, ldr=0):
    L.check(L.load().vlsat_k_layernorm_to(x.data_ptr(), ldx, y.data_ptr(), ldy, rows, 512, gamma.data_ptr(), beta.data_ptr(), relu, out_fmt,
                                          L.ptr(resid), ldr, 0, 0, L.stream_ptr()))
    torch.cuda.synchronize()


def _words(y, rows):
    """the [rows, 512] words of an output buffer as uint32 on the CPU; the pitch gap and the row behind the last keep their fill"""
    assert _untouched(y[:rows, 512:]) and _untouched(y[rows:]), "layernorm wrote outside its rows"
    return y[:rows, :512].contiguous().cpu().numpy().view(np.uint32)


def _both(L, d, rows, relu, resid, gamma=None, xb=None):
    """the same call with output format 0 and 6 -> (y32 as float32, words as uint32)"""
    gamma = d["gamma"] if gamma is None else gamma
    xb = d["xb"] if xb is None else xb
    rb = d["rb"] if resid else None
    out = []
    for fmt in (0, 6):
        y = _nan(rows + 1, LDY)
        _call(L, xb, LD, y, LDY, rows, gamma, d["beta"], relu, fmt, rb, LDR if resid else 0)
        out.append(_words(y, rows))
    return out[0].view(np.float32), out[1]


@pytest.mark.parametrize("resid", [False, True], ids=["no residual", "fp32 residual"])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("rows", ROWS)
def test_pair_words_are_pack_of_the_fp32_output(lib, rows, relu, resid):
    d = _data(rows)
    y32, words = _both(lib, d, rows, relu, resid)
    assert np.isfinite(y32).all()
    assert (words == P.pack(y32)).all(), (rows, relu, resid, y32[words != P.pack(y32)][:5])
    # the planted columns hold what they were planted for
    tiny = np.abs(y32[:, list(COL_TINY + COL_TINIER)])
    assert tiny.max() < 2.0 ** -13 and (relu or tiny.min() > 0)
    assert (y32[:, list(COL_SUB)] == np.float32(2.0 ** -14)).all() and (words[:, list(COL_SUB)] == 0x04000000).all()
    neg0 = y32[:, list(COL_NEG0)]
    assert (neg0 == 0).all()
    if not relu:
        assert neg0.view(np.uint32)[0, 0] == 0x80000000 and (words[:, list(COL_NEG0)] == neg0.view(np.uint32)).all()
    if relu:                                      # nothing negative is left: no word has its sign bit set, except that of a kept -0.0
        assert ((words >> 31) == 0)[y32 != 0].all()


def test_numpy_pack_is_the_headers_pack_on_kernel_values(lib):
    """the numpy packer against f16s_pair_pack (g++, tests/e2_pairs_check.cpp) on values the kernel produced: the planted columns and a
    stretch of ordinary ones of five rows"""
    d = _data(5)
    y32, _ = _both(lib, d, 5, 0, True)
    cols = sorted(set(COL_NEG0 + COL_TINY + COL_TINIER + COL_SUB) | set(range(64, 128)))
    v = y32[:, cols].reshape(-1)
    rows = host_check.lines("e2_pairs_check", "pack", *(f"{b:08x}" for b in v.view(np.uint32)))
    assert (np.array([int(r[1], 16) for r in rows], np.uint32) == P.pack(v)).all()


@pytest.mark.parametrize("rows", [5, 4099])
def test_in_place_and_into_the_residual(lib, rows):
    """y == x (as the fp32 forward does: the out-projection has written E2, the LayerNorm packs it where it stands) and y == resid, same pitch"""
    d = _data(rows)
    for relu in (0, 1):
        _, want = _both(lib, d, rows, relu, False)
        buf = torch.cat([d["xb"], _nan(1, LD)])
        _call(lib, buf, LD, buf, LD, rows, d["gamma"], d["beta"], relu, 6)
        assert (_words(buf, rows) == want).all(), ("y == x", rows, relu)
        _, want = _both(lib, d, rows, relu, True)
        buf = torch.cat([d["rb"], _nan(1, LDR)])
        _call(lib, d["xb"], LD, buf, LDR, rows, d["gamma"], d["beta"], relu, 6, buf, LDR)
        assert (_words(buf, rows) == want).all(), ("y == resid", rows, relu)
        buf = torch.cat([d["xb"], _nan(1, LD)])                       # both at once: x, resid and y one buffer (y = LN(2 x))
        ref = _nan(rows + 1, LDY)
        _call(lib, d["xb"], LD, ref, LDY, rows, d["gamma"], d["beta"], relu, 6, d["xb"], LD)
        _call(lib, buf, LD, buf, LD, rows, d["gamma"], d["beta"], relu, 6, buf, LD)
        assert (_words(buf, rows) == _words(ref, rows)).all(), ("y == x == resid", rows, relu)


def test_results_beyond_the_fp16_range_store_the_words_of_65504(lib):
    """gamma = 1e5: |y| beyond 65504 is clamped before the split, so the word is that of +-65504 (Ah = +-65504, Al = 0), never an infinity"""
    rows = 5
    d = _data(rows)
    gamma = torch.full((512,), 1e5, device=DEV)
    y32, words = _both(lib, d, rows, 0, False, gamma=gamma)
    assert float(y32.max()) > 65504 and float(y32.min()) < -65504
    assert (words[y32 > 65504] == 0x7BFF0000).all() and (words[y32 < -65504] == 0xFBFF0000).all()
    assert (words == P.pack(y32)).all()
    assert ((words >> 26) & 31 != 31).all() and ((words >> 10) & 31 != 31).all()           # no half is an infinity or a NaN


def test_constant_row_gives_the_words_of_beta(lib):
    """a row of 512 equal values: the centred row is exactly zero, so y = beta (max(beta, 0) with the ReLU) and the words are pack(beta)"""
    d = _data(5)
    consts = torch.tensor([3.5, -2.25, 1000.0, 0.0, 0.001953125])
    xb = _pitched(consts[:, None].expand(5, 512).contiguous(), LD)
    beta = d["beta"].cpu().numpy()
    for relu in (0, 1):
        y32, words = _both(lib, d, 5, relu, False, xb=xb)
        want = np.broadcast_to(np.maximum(beta, np.float32(0)) if relu else beta, (5, 512))
        assert (y32 == want).all()
        assert (words == P.pack(y32)).all()
        live = want != 0                                               # (the sign of a zero: 0 * gamma + (-0.0) depends on the sign of gamma)
        assert (words[live] == P.pack(want)[live]).all()


@pytest.mark.parametrize("out_fmt", [3, 5, -1, 8])
def test_other_format_codes_stay_refused(lib, out_fmt):
    d = _data(5)
    y = _nan(6, LDY)
    with pytest.raises(lib.VlsatError, match="layernorm"):
        _call(lib, d["xb"], LD, y, LDY, 5, d["gamma"], d["beta"], 0, out_fmt)
    torch.cuda.synchronize()
    assert _untouched(y)
