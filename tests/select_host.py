"""Builds and runs the host-only check programs of tests/: select_host_check.cpp on the integer helpers of csrc/select_core.h (the float
key, count_ge, the dominance-triple table), eval_scratch_check.cpp on the evaluation-scratch layout of csrc/engine.h, flash_pick_check.cpp
on the kernel selector of csrc/flash_pick.h, gemm_plan_check.cpp on the GEMM planner and variant lists of csrc/gemm_plan.h, plan_graph_check.cpp
on the graph analysis and the workspace list of csrc/plan_graph.h.  g++ only: no HIP header, no library, no device."""
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _exe(sanitize=False, name="select_host_check", defines=()):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    exe = os.path.join(tempfile.mkdtemp(prefix="select_host_"), name)
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-Werror", *extra, *("-D" + d for d in defines), "-I", os.path.join(ROOT, "cvpr2023-vlsat_amd", "csrc"),
                    os.path.join(ROOT, "tests", name + ".cpp"), "-o", exe], check=True)
    return exe


def run(sanitize=False, name="select_host_check", defines=()):
    """lines of the program `name` as (left, right) of ' -> '; sanitize: the stand-alone binary built with ASan + UBSan; defines: -D macros"""
    r = subprocess.run([_exe(sanitize, name, tuple(defines))], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return [tuple(l.split(" -> ", 1)) for l in r.stdout.splitlines()]
