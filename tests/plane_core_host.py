"""Parses what tests/plane_core_check.cpp prints: the host-only check of csrc/plane_core.h, built by host_check with -ffp-contract=off,
optionally with ASan + UBSan in the stand-alone binary."""
import functools

import host_check


@functools.lru_cache(maxsize=None)
def run(sanitize=False):
    """{"d": [(seed, k, n, rank)], "p": [(nine fp32 bit patterns, ok, four fp32 bit patterns)], "s": [(eight fp32 bit patterns: plane,
    point, dist; score bits; class)], "e": [((inliers, above, n, min_inliers, ppm), eligible)], "k": [(inliers, h, key)]}"""
    out = {"d": [], "p": [], "s": [], "e": [], "k": []}
    for head, tail in host_check.lines("plane_core_check", sanitize=sanitize, fp_strict=True):
        kind, *left = head.split()
        right = tail.split()
        if kind == "d":
            out["d"].append((int(left[0]), int(left[1]), int(left[2]), int(right[0])))
        elif kind == "p":
            out["p"].append((tuple(int(x, 16) for x in left), int(right[0]), tuple(int(x, 16) for x in right[1:])))
        elif kind == "s":
            out["s"].append((tuple(int(x, 16) for x in left), int(right[0], 16), int(right[1])))
        elif kind == "e":
            out["e"].append((tuple(int(x) for x in left), int(right[0])))
        else:
            out["k"].append((int(left[0]), int(left[1]), int(right[0], 16)))
    return out
