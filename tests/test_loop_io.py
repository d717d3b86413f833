"""The arrays of a closed loop as the host loop chain passes them (csrc/mpc_solve_plan.h: LoopIo) -- the size of every member in bytes, which is
what the host-pointer forms stage -- and the refusals every loop of the NLP shares (loop_refusal), on the CPU through the emulation harness
(tests/emu: emu_loop_io_arrays, emu_loop_refusal).  The sizes and the words below are written out here, not read from the code under test."""
import ctypes as C

import numpy as np
import pytest

from helpers import emu_lib

MEMBERS = ("init_state", "path", "orient", "vdes", "track", "offsets", "traj", "ctrl", "step_status", "clearance", "nearest", "chosen", "kgain",
           "wgain", "ogain")
INPUTS = ("init_state", "path", "orient", "vdes", "track", "offsets")
I64P, I32P = C.POINTER(C.c_int64), C.POINTER(C.c_int32)


def place(absent=()):
    """the members at known offsets of one dummy buffer (nothing is read or written through them); -1: null"""
    return np.array([-1 if m in absent else 64 * (i + 1) for i, m in enumerate(MEMBERS)], dtype=np.int64)


def dims(B=3, L=5, Lp=7, Lt=0, M=0, per_ego=0, noise_mode=0, tracked=0):
    return np.array([B, L, Lp, Lt, M, per_ego, noise_mode, tracked], dtype=np.int32)


def sizes(B, L, Lp, N, Lt, M, per_ego):
    nT = ((B if per_ego else 1) * M) if M > 0 else B
    return dict(init_state=B * 5 * 8, path=B * Lp * 2 * 8, orient=B * Lp * 8, vdes=B * 8, track=nT * Lt * 3 * 8, offsets=nT * 8,
                traj=B * L * 5 * 8, ctrl=B * L * 2 * 8, step_status=B * L * 4, clearance=B * L * 8, nearest=B * L * 4,
                chosen=B * L * (N + 1) * 3 * 4, kgain=B * L * 2 * 5 * 8, wgain=B * L * 2 * 7 * 8, ogain=B * L * 2 * 3 * 8)


OPTIONAL = ("step_status", "track", "offsets", "clearance", "nearest", "chosen", "kgain", "wgain", "ogain")


@pytest.mark.parametrize("M,per_ego", [(0, 0), (2, 0), (2, 1)])         # one track per ego; traffic shared by all egos; traffic per ego
@pytest.mark.parametrize("absent", [(), OPTIONAL])
def test_every_array_has_the_size_written_out_here_and_nulls_stay_null(M, per_ego, absent):
    L = emu_lib()
    L.emu_loop_io_arrays.argtypes = [I32P, C.c_int32, C.c_void_p, I64P, I64P, I64P, I32P]
    L.emu_loop_io_arrays.restype = C.c_int
    B, steps, Lp, N, Lt = 3, 5, 7, 4, 6
    base = np.zeros(4096)
    at, d = place(absent), dims(B, steps, Lp, Lt, M, per_ego, 0, 1)
    where, nbytes, written = np.full(32, -7, np.int64), np.full(32, -7, np.int64), np.full(32, -7, np.int32)
    assert L.emu_loop_io_arrays(d.ctypes.data_as(I32P), N, base.ctypes.data, at.ctypes.data_as(I64P), where.ctypes.data_as(I64P),
                                nbytes.ctypes.data_as(I64P), written.ctypes.data_as(I32P)) == len(MEMBERS)
    want = sizes(B, steps, Lp, N, Lt, M, per_ego)
    if M > 0:                                          # the figures of the issue, once more in full
        assert want["track"] == (B if per_ego else 1) * M * Lt * 3 * 8 and want["offsets"] == (B if per_ego else 1) * M * 8
    else:
        assert want["track"] == B * Lt * 3 * 8
    for i, m in enumerate(MEMBERS):
        assert where[i] == at[i], m                                    # (every member once, each with its own row of the table; null stays null)
        assert nbytes[i] == (0 if m in absent else want[m]), m         # (null: no room is taken)
        assert written[i] == (0 if m in INPUTS else 1), m
    assert not np.any(base)


def refusal(d, N=4, sigma=0.0, offset=0.0, absent=()):
    L = emu_lib()
    L.emu_loop_refusal.argtypes = [I32P, C.c_double, C.c_double, C.c_void_p, I64P, C.c_int32, C.c_char_p, C.c_int32]
    L.emu_loop_refusal.restype = C.c_int
    base, at, out = np.zeros(4096), place(absent), C.create_string_buffer(512)
    n = L.emu_loop_refusal(d.ctypes.data_as(I32P), sigma, offset, base.ctypes.data, at.ctypes.data_as(I64P), N, out, 512)
    assert 0 <= n < 512
    return out.value.decode() if n else None


NO_TRACK = ("track", "offsets", "clearance", "nearest", "chosen", "kgain", "wgain", "ogain")
REFUSED = {
    "B = 0": (dict(B=0), {}, "B > 0"),
    "L = 0": (dict(L=0), {}, "L >= N"),
    "Lp = L - 1": (dict(L=5, Lp=4), {}, "Lp >= L"),
    "L = N - 1": (dict(L=3), {}, "L >= N"),
    **{f"{m} null": (dict(), dict(absent=NO_TRACK + (m,)), m) for m in ("init_state", "path", "orient", "vdes", "traj", "ctrl")},
    "noise_mode = -1": (dict(noise_mode=-1), {}, "noise_mode"),
    "noise_mode = 3": (dict(noise_mode=3), {}, "noise_mode"),
    "sigma = -1 with noise": (dict(noise_mode=1), dict(sigma=-1.0), "sigma >= 0"),
    "sigma NaN with noise": (dict(noise_mode=2), dict(sigma=float("nan")), "sigma >= 0"),
    "Lt = 0": (dict(L=6, Lt=0, tracked=1), {}, "obst_track"),
    "Lt = 2": (dict(L=6, Lt=2, tracked=1), {}, "obst_track"),
    "Lt = L - 1": (dict(L=6, Lt=5, tracked=1), {}, "obst_track"),
    "null track with Lt = 1": (dict(L=6, Lt=1, tracked=1), dict(absent=("track",)), "obst_track"),
    "offset inf": (dict(L=6, Lt=1, tracked=1), dict(offset=float("inf")), "obst_offset"),
    "offset NaN": (dict(L=6, Lt=6, tracked=1), dict(offset=float("nan")), "obst_offset"),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_what_every_loop_refuses(case):
    d, kw, word = REFUSED[case]
    text = refusal(dims(**d), **kw)
    assert text is not None and text.startswith("closed loop:") and word in text, (case, text)


@pytest.mark.parametrize("Lt", [1, 6, 9])              # standing still, a row per step, rows to spare (L = 6)
@pytest.mark.parametrize("noise_mode,sigma", [(0, -1.0), (1, 0.0), (2, 0.1)])       # (sigma is not read with the noise off)
def test_valid_loops_are_not_refused(Lt, noise_mode, sigma):
    assert refusal(dims(L=6, Lt=Lt, tracked=1, noise_mode=noise_mode), sigma=sigma, offset=1.0) is None
    assert refusal(dims(L=6, noise_mode=noise_mode), sigma=sigma, absent=NO_TRACK) is None          # the plain loop
    assert refusal(dims(L=4, Lp=4), absent=("step_status",) + NO_TRACK) is None                    # L = N = Lp, no step_status
