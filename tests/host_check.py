"""Builds and runs the stand-alone host check programs of tests/ (tests/<name>.cpp): g++ only, on the host-only headers of csrc/; no HIP
header, no library, no device -- except with link_library, which links libvlsat_hip.so for a program that calls into it without opening
a device.  The sanitizers, where asked for, are compiled into the stand-alone binary; nothing is preloaded anywhere."""
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def exe(name, sanitize=False, fp_strict=False, defines=(), link_library=False):
    """path of the program built from tests/<name>.cpp; fp_strict: -ffp-contract=off; sanitize: ASan + UBSan in the binary; defines: a
    tuple of -D macros; link_library: against libvlsat_hip.so and the HIP runtime, with the library's include directories and without
    -Wall -Werror"""
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    csrc, src = os.path.join(ROOT, "cvpr2023-vlsat_amd", "csrc"), os.path.join(ROOT, "tests", name + ".cpp")
    out = os.path.join(tempfile.mkdtemp(prefix=name + "_"), name)
    if link_library:
        from vlsat_amd import build as B
        assert not (sanitize or fp_strict or defines), "a program linked to the library is built plain"
        assert os.path.exists(B.LIB), "libvlsat_hip.so is not built"
        lib_dir = os.path.dirname(B.LIB)
        flags = ["-D__HIP_PLATFORM_AMD__", "-I", csrc, "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", src,
                 "-L", lib_dir, "-lvlsat_hip", "-L", "/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{lib_dir}:/opt/rocm/lib"]
    else:
        flags = ["-Wall", "-Werror", *(["-ffp-contract=off"] if fp_strict else []),
                 *(["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []), *("-D" + d for d in defines),
                 "-I", csrc, src]
    subprocess.run([gxx, "-O1", "-std=c++17", *flags, "-o", out], check=True)
    return out


def lines(name, *args, env=None, **build_options):
    """lines of the program `name` run with `args`, as (left, right) of ' -> '; build_options: those of exe"""
    r = subprocess.run([exe(name, **build_options), *args], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return [tuple(l.split(" -> ", 1)) for l in r.stdout.splitlines()]
