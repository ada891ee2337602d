"""Parses what tests/segment_core_check.cpp prints: the host-only check of csrc/segment_core.h, built by host_check with
-ffp-contract=off, optionally with ASan + UBSan in the stand-alone binary."""
import functools

import host_check


@functools.lru_cache(maxsize=None)
def run(sanitize=False):
    """{"w": [(six input bit patterns, weight bits)], "k": [(weight bits, root, key)], "r": [(min_verts, rounds)], "s": [(V, bytes)]}"""
    out = {"w": [], "k": [], "r": [], "s": []}
    for head, right in host_check.lines("segment_core_check", sanitize=sanitize, fp_strict=True):
        kind, *left = head.split()
        if kind == "w":
            out["w"].append((tuple(int(x, 16) for x in left), int(right, 16)))
        elif kind == "k":
            out["k"].append((int(left[0], 16), int(left[1]), int(right, 16)))
        else:
            (only,) = left
            out[kind].append((int(only), int(right)))
    return out
