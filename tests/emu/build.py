"""Builds tests/emu/libmpc_emu.so -- the CPU emulation harness of the HIP kernels (test infrastructure)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SRC = os.path.join(HERE, "emu.cpp")
LIB = os.path.join(HERE, "libmpc_emu.so")
DEPS = [SRC,
        os.path.join(HERE, "emu_solve.h"),
        os.path.join(ROOT, "motion-planning-for-autonomous-driving-with-mpc_amd", "csrc", "mpc_stage_math.h"),
        os.path.join(ROOT, "motion-planning-for-autonomous-driving-with-mpc_amd", "csrc", "mpc_host_common.h"),
        os.path.join(ROOT, "motion-planning-for-autonomous-driving-with-mpc_amd", "csrc", "mpc_solve_plan.h"),
        os.path.join(ROOT, "motion-planning-for-autonomous-driving-with-mpc_amd", "csrc", "mpc_stamps.h"),
        os.path.join(ROOT, "include", "mpcgpu.h"),
        os.path.join(ROOT, "motion-planning-for-autonomous-driving-with-mpc_amd", "csrc", "mpc_closed_loop.h"),
        os.path.join(ROOT, "motion-planning-for-autonomous-driving-with-mpc_amd", "csrc", "mpc_forces_qp.h")]


def build(force=False):
    stale = (not os.path.exists(LIB)) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in DEPS)
    if force or stale:
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", LIB, SRC])
    return LIB


if __name__ == "__main__":
    print(build(force=True))
