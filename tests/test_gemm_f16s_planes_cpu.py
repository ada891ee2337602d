"""csrc/gemm_f16s_planes.h (the weight planes of the split-fp16 8-phase GEMM) and the sibling list of csrc/gemm_plan.h, compiled by g++
(tests/gemm_f16s_planes_check.cpp through tests/gemm_f16s_host.py): no HIP header, no library, no device; and the C header and
signature table of the kernel's test entry."""
import pytest

import gemm_f16s_host


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_planes_siblings_and_planner(sanitize):
    """to_half: the header's integer fp32 -> fp16 against the definition on every fp16 value, every midpoint (ties to even), their
    neighbours and 200 000 random bit patterns.  planes: 47 tensors -- random at scales 2^-30 .. 2^48, tiny, huge, zero, negative-zero,
    denormal -- k = 13 - ceil(log2 max |w|) (cut off at +-100), max |w 2^k| in (2^12, 2^13], hi + lo within 2^-22 relative of w 2^k,
    hi 2^-11 exact for |hi| >= 2^-3, nothing infinite.  siblings: with GemmArgs::f16s every exact-fp32 row of the 8-phase list (the
    five (additive operands, ReLU-on-A) forms of the fp32 forward) has its sibling and no other row, no row without the flag, has one.
    planner: 90 problems plan the same with and without f16s; f16s without planes, beside another precision or with |w_exp| > 100 is
    refused.  "asan_ubsan": the same stand-alone binary under ASan + UBSan."""
    rows = gemm_f16s_host.run(sanitize)
    assert set(rows) == {"to_half", "planes", "siblings", "planner"}, rows
    assert all(v.split()[0] == "ok" for v in rows.values()), rows
    assert rows["planes"] == "ok 47 tensors, 0 violations"
    assert rows["siblings"].startswith("ok 5 rows with a sibling")
    assert rows["planner"] == "ok 90 plans compared, 0 wrong"


def test_gemm_header_symbols_are_bound_and_disjoint():
    from vlsat_amd import lib as L
    names = {"vlsat_k_split_f16s", "vlsat_k_gemm_f16s"}
    assert names == set(L.declared_gemm_symbols()) == set(L._SIGNATURES_GEMM)
    for other in (L.declared_symbols(), L._SIGNATURES, L.declared_flash_symbols(), L._SIGNATURES_FLASH, L.declared_convex_symbols(), L._SIGNATURES_CONVEX):
        assert not names & set(other)
    assert len(L.declared_symbols()) == len(L._SIGNATURES) == 81              # include/vlsat.h keeps its entries
    # the arguments of vlsat_k_gemm plus p8_part_min
    assert L._SIGNATURES_GEMM["vlsat_k_gemm_f16s"][1] == L._SIGNATURES["vlsat_k_gemm"][1][:-1] + [L._i32, L._vp]
    lib = L.load()
    assert all(hasattr(lib, n) and getattr(lib, n).argtypes is not None for n in names)
    assert "GEMM_HEADER_PATH" in open(L.__file__).read().split("def identity")[1].split("def _declared")[0]
