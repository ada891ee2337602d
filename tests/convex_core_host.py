"""Parses what tests/convex_core_check.cpp prints: the host-only check of csrc/convex_core.h, built by host_check with -ffp-contract=off,
optionally with ASan + UBSan in the stand-alone binary."""
import functools

import host_check


@functools.lru_cache(maxsize=None)
def run(sanitize=False):
    """-> [(fourteen fp32 bit patterns: x_i, n_i, x_j, n_j, tau, q; c bits; c bits seen from j; usable_i, usable_j, q_ok, concave)]"""
    rows = []
    for head, tail in host_check.lines("convex_core_check", sanitize=sanitize, fp_strict=True):
        kind, *left = head.split()
        right = tail.split()
        assert kind == "t"
        rows.append((tuple(int(x, 16) for x in left), int(right[0], 16), int(right[1], 16), *(int(x) for x in right[2:])))
    return rows
