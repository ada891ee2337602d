"""Builds and runs tests/plane_core_check.cpp, the host-only check of csrc/plane_core.h, the way voxel_core_host.py builds its program:
g++ only, -ffp-contract=off, optionally with ASan + UBSan in the stand-alone binary; no HIP header, no library, no device."""
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _exe(sanitize=False):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    exe = os.path.join(tempfile.mkdtemp(prefix="plane_core_"), "plane_core_check")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *extra, "-I",
                    os.path.join(ROOT, "cvpr2023-vlsat_amd", "csrc"), os.path.join(ROOT, "tests", "plane_core_check.cpp"), "-o", exe], check=True)
    return exe


@functools.lru_cache(maxsize=None)
def run(sanitize=False):
    """{"d": [(seed, k, n, rank)], "p": [(nine fp32 bit patterns, ok, four fp32 bit patterns)], "s": [(eight fp32 bit patterns: plane,
    point, dist; score bits; class)], "e": [((inliers, above, n, min_inliers, ppm), eligible)], "k": [(inliers, h, key)]}"""
    r = subprocess.run([_exe(sanitize)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    out = {"d": [], "p": [], "s": [], "e": [], "k": []}
    for line in r.stdout.splitlines():
        kind, rest = line.split(" ", 1)
        left, right = (x.split() for x in rest.split(" -> "))
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
