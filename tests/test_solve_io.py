"""The rows of a solve as the host solve chain passes them (csrc/mpc_solve_plan.h: SolveIo) -- the width of every member, in elements per
instance, and the slice of instances off .. off + n - 1 that a chunk of a large batch receives -- on the CPU through the emulation harness
(tests/emu: emu_solve_io_rows).  The widths below are written out here, not read from the code under test."""
import ctypes as C

import numpy as np
import pytest

from helpers import emu_lib

MEMBERS = ("x0", "p", "obst", "x_out", "status", "iters", "kkt", "lam_g", "lam_x", "snap")
SNAP_LEN = 1237                                       # passed in: any length will do


def widths(N, nx):
    n_w = 2 * N + nx * (N + 1)
    n_g = 1 + (14 if nx == 5 else 15) * (N + 1)
    return dict(x0=n_w, p=n_w, obst=6, x_out=n_w, status=1, iters=1, kkt=1, lam_g=n_g, lam_x=n_w, snap=SNAP_LEN)


@pytest.mark.parametrize("N,nx", [(10, 5), (30, 6)])
@pytest.mark.parametrize("absent", [("obst", "iters", "lam_x"), ()])
@pytest.mark.parametrize("off,n", [(128, 44), (0, 64)])
def test_a_slice_moves_every_member_by_its_width_and_keeps_nulls(N, nx, absent, off, n):
    L = emu_lib()
    i64p = C.POINTER(C.c_int64)
    L.emu_solve_io_rows.argtypes = [C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, i64p, C.c_int64, C.c_int32, i64p]
    L.emu_solve_io_rows.restype = C.c_int
    base = np.zeros(4096)                              # the members point into it at known offsets; nothing is read or written
    at = np.array([-1 if m in absent else 64 * (i + 1) for i, m in enumerate(MEMBERS)], dtype=np.int64)
    out = np.full(11, -7, dtype=np.int64)
    assert L.emu_solve_io_rows(N, nx, SNAP_LEN, 172, base.ctypes.data, at.ctypes.data_as(i64p), off, n, out.ctypes.data_as(i64p)) == 0
    assert out[0] == n
    w = widths(N, nx)
    for i, m in enumerate(MEMBERS):
        assert out[1 + i] == (-1 if m in absent else off * w[m]), m
    assert not np.any(base)
