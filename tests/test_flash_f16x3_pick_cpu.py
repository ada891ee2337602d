"""csrc/flash_pick.h, the split-fp16 list and its pick function, compiled by g++ (tests/flash_f16x3_pick_check.cpp through
tests/host_check.py): no HIP header, no library, no device."""
import pytest

import host_check


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_flash_f16x3_pick_lists_two_kernels_and_refuses_everything_else(sanitize):
    """Head dim {0, 32, 48, 64, 128} x use_tr -1..4 x io 0..3 x bq {64, 128, 256} x qg {0, 1, 2} x ablate {0, 1, 4, 64} = 4320 calls: the
    two listed forms (fp32 tensors, head dim 64, 128-query tiles, 32 queries per wave, no ablation; gather or transpose read) get their
    row of kFlashF16x3Variants, every other call gets -1 and an error text that names the kernel family, both rows are reached, no row
    is listed twice, and flash_f16x3_supports is the pick with the defaults.  "asan_ubsan": the same stand-alone binary under ASan +
    UBSan."""
    rows = dict(host_check.lines("flash_f16x3_pick_check", sanitize=sanitize))
    assert set(rows) == {"listed", "unlisted", "reachable", "supports", "rows"}, rows
    assert all(v.split()[0] == "ok" for v in rows.values()), rows
    assert rows["listed"] == "ok 4320 cases, 2 launches"
    assert rows["unlisted"] == "ok 4318 errors"
    assert rows["reachable"] == "ok 2" and rows["rows"] == "ok 2"
