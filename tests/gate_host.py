"""Builds and runs tests/gate_host_check.cpp: a host-only program on csrc/kernels.h (gate_select) and libvlsat_hip.so (launch_gate's
argument checks).  It opens no device; the child process is also started with no GPU visible, so that a check that failed to refuse
could not launch anything either."""
import functools
import os
import shutil
import subprocess
import tempfile

from vlsat_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _exe():
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    assert os.path.exists(B.LIB), "libvlsat_hip.so is not built"
    lib_dir = os.path.dirname(B.LIB)
    exe = os.path.join(tempfile.mkdtemp(prefix="gate_host_"), "gate_host_check")
    subprocess.run([gxx, "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "cvpr2023-vlsat_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "gate_host_check.cpp"),
                    "-L", lib_dir, "-lvlsat_hip", "-L", "/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{lib_dir}:/opt/rocm/lib", "-o", exe],
                   check=True)
    return exe


def run(what):
    """lines of `gate_host_check <what>` as (left, right) of ' -> '"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([_exe(), what], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return [tuple(l.split(" -> ", 1)) for l in r.stdout.splitlines()]
