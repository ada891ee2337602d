"""Builds and runs tests/voxel_core_check.cpp, the host-only check of csrc/voxel_core.h, the way cloud_core_host.py builds its program:
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
    exe = os.path.join(tempfile.mkdtemp(prefix="voxel_core_"), "voxel_core_check")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *extra, "-I",
                    os.path.join(ROOT, "cvpr2023-vlsat_amd", "csrc"), os.path.join(ROOT, "tests", "voxel_core_check.cpp"), "-o", exe], check=True)
    return exe


@functools.lru_cache(maxsize=None)
def run(sanitize=False):
    """{"k": [(seven fp32 bit patterns: x y z ox oy oz voxel, key)], "q": [(fp32 bits, as position, as normal component)],
    "m": [(sum, count, fp32 bits)], "n": [(three sums, three fp32 bit patterns)], "c": [(sum, count, value)]}"""
    r = subprocess.run([_exe(sanitize)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    out = {"k": [], "q": [], "m": [], "n": [], "c": []}
    for line in r.stdout.splitlines():
        kind, rest = line.split(" ", 1)
        left, right = (x.split() for x in rest.split(" -> "))
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
