"""Parses what tests/cloud_core_check.cpp prints: the host-only check of csrc/cloud_core.h, built by host_check with -ffp-contract=off,
optionally with ASan + UBSan in the stand-alone binary."""
import functools

import host_check


@functools.lru_cache(maxsize=None)
def run(sanitize=False):
    """{"d": [(six point bit patterns, j, d2 bits, key)], "u": [(six normal bit patterns, weight bits)],
    "n": [(use_viewpoint, three viewpoint fp64 bit patterns, min_points, member bit patterns (3 per member), four fp64 result bit patterns)]}"""
    out = {"d": [], "u": [], "n": []}
    for head, tail in host_check.lines("cloud_core_check", sanitize=sanitize, fp_strict=True):
        kind, *left = head.split()
        right = tail.split()
        if kind == "d":
            out["d"].append((tuple(int(x, 16) for x in left[:6]), int(left[6]), int(right[0], 16), int(right[1], 16)))
        elif kind == "u":
            out["u"].append((tuple(int(x, 16) for x in left), int(right[0], 16)))
        else:
            count = int(left[5])
            assert len(left) == 6 + 3 * count
            out["n"].append((int(left[0]), tuple(int(x, 16) for x in left[1:4]), int(left[4]), tuple(int(x, 16) for x in left[6:]),
                             tuple(int(x, 16) for x in right)))
    return out
