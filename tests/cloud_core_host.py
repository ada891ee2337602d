"""Builds and runs tests/cloud_core_check.cpp, the host-only check of csrc/cloud_core.h, the way segment_core_host.py builds its
program: g++ only, -ffp-contract=off, optionally with ASan + UBSan in the stand-alone binary; no HIP header, no library, no device."""
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
    exe = os.path.join(tempfile.mkdtemp(prefix="cloud_core_"), "cloud_core_check")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *extra, "-I",
                    os.path.join(ROOT, "cvpr2023-vlsat_amd", "csrc"), os.path.join(ROOT, "tests", "cloud_core_check.cpp"), "-o", exe], check=True)
    return exe


@functools.lru_cache(maxsize=None)
def run(sanitize=False):
    """{"d": [(six point bit patterns, j, d2 bits, key)], "u": [(six normal bit patterns, weight bits)],
    "n": [(use_viewpoint, three viewpoint fp64 bit patterns, min_points, member bit patterns (3 per member), four fp64 result bit patterns)]}"""
    r = subprocess.run([_exe(sanitize)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    out = {"d": [], "u": [], "n": []}
    for line in r.stdout.splitlines():
        kind, rest = line.split(" ", 1)
        left, right = (x.split() for x in rest.split(" -> "))
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
