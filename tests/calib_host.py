"""Builds and runs tests/calib_host_check.cpp, the host-only check of the bin rule in csrc/calib_core.h, the way select_host.py builds
its programs: g++ only, optionally with ASan + UBSan in the stand-alone binary; no HIP header, no library, no device."""
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
    exe = os.path.join(tempfile.mkdtemp(prefix="calib_host_"), "calib_host_check")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "cvpr2023-vlsat_amd", "csrc"),
                    os.path.join(ROOT, "tests", "calib_host_check.cpp"), "-o", exe], check=True)
    return exe


def run(sanitize=False):
    """rows (bins, fp32 bit pattern, eligible, column) the program printed"""
    r = subprocess.run([_exe(sanitize)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    rows = []
    for line in r.stdout.splitlines():
        left, col = line.split(" -> ", 1)
        bins, bits, eligible = left.split(":")
        rows.append((int(bins), int(bits, 16), int(eligible), int(col)))
    return rows
