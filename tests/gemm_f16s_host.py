"""Builds and runs tests/gemm_f16s_planes_check.cpp, the host-only check of csrc/gemm_f16s_planes.h and of the sibling list of
csrc/gemm_plan.h, the way flash_f16x3_core_host.py builds its program: g++ only, optionally with ASan + UBSan in the stand-alone
binary; no HIP header, no library, no device."""
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
    exe = os.path.join(tempfile.mkdtemp(prefix="gemm_f16s_"), "gemm_f16s_planes_check")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "cvpr2023-vlsat_amd", "csrc"),
                    os.path.join(ROOT, "tests", "gemm_f16s_planes_check.cpp"), "-o", exe], check=True)
    return exe


@functools.lru_cache(maxsize=None)
def run(sanitize=False):
    """{name: text right of ' -> '} of the program's lines"""
    r = subprocess.run([_exe(sanitize)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return dict(l.split(" -> ", 1) for l in r.stdout.splitlines())
