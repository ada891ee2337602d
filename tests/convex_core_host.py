"""Builds and runs tests/convex_core_check.cpp, the host-only check of csrc/convex_core.h, the way plane_core_host.py builds its program:
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
    exe = os.path.join(tempfile.mkdtemp(prefix="convex_core_"), "convex_core_check")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *extra, "-I",
                    os.path.join(ROOT, "cvpr2023-vlsat_amd", "csrc"), os.path.join(ROOT, "tests", "convex_core_check.cpp"), "-o", exe], check=True)
    return exe


@functools.lru_cache(maxsize=None)
def run(sanitize=False):
    """-> [(fourteen fp32 bit patterns: x_i, n_i, x_j, n_j, tau, q; c bits; c bits seen from j; usable_i, usable_j, q_ok, concave)]"""
    r = subprocess.run([_exe(sanitize)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    rows = []
    for line in r.stdout.splitlines():
        kind, rest = line.split(" ", 1)
        assert kind == "t"
        left, right = (x.split() for x in rest.split(" -> "))
        rows.append((tuple(int(x, 16) for x in left), int(right[0], 16), int(right[1], 16), *(int(x) for x in right[2:])))
    return rows
