"""Builds and runs tests/segment_core_check.cpp, the host-only check of csrc/segment_core.h, the way calib_host.py builds its program:
g++ only, optionally with ASan + UBSan in the stand-alone binary; no HIP header, no library, no device."""
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
    exe = os.path.join(tempfile.mkdtemp(prefix="segment_core_"), "segment_core_check")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *extra, "-I",
                    os.path.join(ROOT, "cvpr2023-vlsat_amd", "csrc"), os.path.join(ROOT, "tests", "segment_core_check.cpp"), "-o", exe], check=True)
    return exe


@functools.lru_cache(maxsize=None)
def run(sanitize=False):
    """{"w": [(six input bit patterns, weight bits)], "k": [(weight bits, root, key)], "r": [(min_verts, rounds)], "s": [(V, bytes)]}"""
    r = subprocess.run([_exe(sanitize)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    out = {"w": [], "k": [], "r": [], "s": []}
    for line in r.stdout.splitlines():
        kind, rest = line.split(" ", 1)
        left, right = rest.split(" -> ")
        if kind == "w":
            out["w"].append((tuple(int(x, 16) for x in left.split()), int(right, 16)))
        elif kind == "k":
            out["k"].append((int(left.split()[0], 16), int(left.split()[1]), int(right, 16)))
        else:
            out[kind].append((int(left), int(right)))
    return out
