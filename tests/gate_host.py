"""Runs tests/gate_host_check.cpp: a host-only program on csrc/kernels.h (gate_select) and libvlsat_hip.so (launch_gate's argument
checks), built by host_check against the library.  It opens no device; the child process is also started with no GPU visible, so that
a check that failed to refuse could not launch anything either."""
import os

import host_check


def run(what):
    """lines of `gate_host_check <what>` as (left, right) of ' -> '"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    return host_check.lines("gate_host_check", what, env=env, link_library=True)
