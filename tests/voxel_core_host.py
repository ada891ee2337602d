"""Parses what tests/voxel_core_check.cpp prints: the host-only check of csrc/voxel_core.h, built by host_check with -ffp-contract=off,
optionally with ASan + UBSan in the stand-alone binary."""
import functools

import host_check


@functools.lru_cache(maxsize=None)
def run(sanitize=False):
    """{"k": [(seven fp32 bit patterns: x y z ox oy oz voxel, key)], "q": [(fp32 bits, as position, as normal component)],
    "m": [(sum, count, fp32 bits)], "n": [(three sums, three fp32 bit patterns)], "c": [(sum, count, value)]}"""
    out = {"k": [], "q": [], "m": [], "n": [], "c": []}
    for head, tail in host_check.lines("voxel_core_check", sanitize=sanitize, fp_strict=True):
        kind, *left = head.split()
        right = tail.split()
        if kind == "k":
            out["k"].append((tuple(int(x, 16) for x in left), int(right[0], 16)))
        elif kind == "q":
            out["q"].append((int(left[0], 16), int(right[0]), int(right[1])))
        elif kind == "m":
            out["m"].append((int(left[0]), int(left[1]), int(right[0], 16)))
        elif kind == "n":
            out["n"].append((tuple(int(x) for x in left), tuple(int(x, 16) for x in right)))
        else:
            out["c"].append((int(left[0]), int(left[1]), int(right[0])))
    return out
