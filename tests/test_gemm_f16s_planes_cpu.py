"""csrc/gemm_f16s_planes.h (the weight planes of the split-fp16 8-phase GEMM) and the sibling list of csrc/gemm_plan.h, compiled by g++
(tests/gemm_f16s_planes_check.cpp through tests/host_check.py): no HIP header, no library, no device."""
import pytest

import host_check


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_planes_siblings_and_planner(sanitize):
    """to_half: the header's integer fp32 -> fp16 against the definition on every fp16 value, every midpoint (ties to even), their
    neighbours and 200 000 random bit patterns.  planes: 47 tensors -- random at scales 2^-30 .. 2^48, tiny, huge, zero, negative-zero,
    denormal -- k = 13 - ceil(log2 max |w|) (cut off at +-100), max |w 2^k| in (2^12, 2^13], hi + lo within 2^-22 relative of w 2^k,
    hi 2^-11 exact for |hi| >= 2^-3, nothing infinite.  siblings: with GemmArgs::f16s every exact-fp32 row of the 8-phase list (the
    five (additive operands, ReLU-on-A) forms of the fp32 forward) has its sibling and no other row, no row without the flag, has one.
    planner: 90 problems plan the same with and without f16s; f16s without planes, beside another precision or with |w_exp| > 100 is
    refused.  "asan_ubsan": the same stand-alone binary under ASan + UBSan."""
    rows = dict(host_check.lines("gemm_f16s_planes_check", sanitize=sanitize))
    assert set(rows) == {"to_half", "planes", "siblings", "planner"}, rows
    assert all(v.split()[0] == "ok" for v in rows.values()), rows
    assert rows["planes"] == "ok 47 tensors, 0 violations"
    assert rows["siblings"].startswith("ok 5 rows with a sibling")
    assert rows["planner"] == "ok 90 plans compared, 0 wrong"
