"""csrc/gemm_plan.h: the list of the persistent kernel's split-fp16 siblings and its pick function, and the shape list of
tests/test_hip_gemm_f16s_tiled.py against the planner -- compiled by g++ (tests/gemm_f16s_tiled_shapes_check.cpp through
tests/host_check.py): no HIP header, no library, no device."""
import pytest

import host_check
from gemm_f16s_tiled_shapes import FORMS, SHAPES


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_shape_list_stays_on_the_persistent_kernel_and_reaches_every_tile(sanitize):
    """At 256 CUs, as vlsat_k_gemm_f16s(..., -1) hands the problems in: every launch and tail of every shape x form is in the TILED family
    and gets a sibling, the five tiles are all reached, at least one shape pairs as a twin on a sibling, and the pick refuses N = 26,
    f16s = 1, no_dma, a single gathered-row operand, c_scale != 1 and a missing row.  "asan_ubsan": the same stand-alone binary under
    ASan + UBSan."""
    out = host_check.lines("gemm_f16s_tiled_shapes_check", *(f"{M},{N},{K}" for M, N, K in SHAPES), sanitize=sanitize)
    launches = [l for l in out if l[0].startswith("launch | ")]
    rows = dict(l for l in out if len(l) == 2)
    assert set(rows) == {"families", "siblings", "tiles", "twin", "refused"}, rows
    assert all(v.split()[0] == "ok" for v in rows.values()), rows
    assert len(launches) >= len(SHAPES) * len(FORMS)
    assert rows["families"] == f"ok {len(launches)} launches, all TILED" and rows["tiles"].startswith("ok 5 of 5")
    assert rows["refused"] == "ok 6"
