"""
ctypes view of include/mpcgpu.h -- the C-ABI of libmpcgpu.so (hand-written HIP kernels for gfx950).

This is the only place the package touches the shared library.  There is NO CPU fallback: if the library is
missing or cannot be loaded, `load_library()` raises and every solver object fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = "libmpcgpu.so"
LIB_PATH = os.path.join(PKG_DIR, "csrc", LIB_NAME)

MPC_STATUS_CONVERGED = 1
MPC_STATUS_MAXITER = 0
MPC_STATUS_NAN = -6
MPC_STATUS_NOPROGRESS = -7

MPC_OK = 0
MPC_ERR_INVALID = -1
MPC_ERR_HIP = -2
MPC_ERR_BOUNDS = -3
MPC_ERR_STATE = -4

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


class MpcProblemDesc(C.Structure):
    """mirror of `mpc_problem_desc` (include/mpcgpu.h)."""
    _fields_ = [
        ("N", C.c_int32), ("nx", C.c_int32), ("nu", C.c_int32), ("formulation", C.c_int32),
        ("max_iter", C.c_int32), ("fixed_iters", C.c_int32), ("obst_mult", C.c_int32), ("device", C.c_int32),
        ("dt", C.c_double), ("wheelbase", C.c_double), ("friction_div", C.c_double), ("ego_offset", C.c_double),
        ("tol", C.c_double),
        ("Q", C.c_double * 8), ("R", C.c_double * 2), ("P", C.c_double * 8), ("obstacle", C.c_double * 6),
    ]


_vp, _i32, _f64, _u64 = C.c_void_p, C.c_int32, C.c_double, C.c_uint64
_desc_p = C.POINTER(MpcProblemDesc)
_rows = [_dp, _dp, _dp, _dp, _ip, _ip, _dp]          # x0, p, obst, x_out, status, iters, kkt of a host-pointer solve
_loop_tail = [_i32, _f64, _u64]                      # noise_mode, sigma, seed

# the prototypes of include/mpcgpu.h: name -> argument types (device-pointer forms take void*; the last void* of a _dev form is the stream)
PROTOTYPES = {
    "mpc_default_desc": [_desc_p, _i32, _i32],
    "mpc_create": [C.POINTER(_vp), _desc_p],
    "mpc_destroy": [_vp],
    "mpc_last_error": [_vp],
    "mpc_abi_version": [],
    "mpc_set_bounds": [_vp, _dp, _dp, _dp, _dp],
    "mpc_get_bounds": [_vp, _dp, _dp, _dp, _dp],
    "mpc_set_weights": [_vp, _dp, _dp],
    "mpc_set_profiling": [_vp, _i32],
    "mpc_set_option": [_vp, C.c_char_p, C.c_char_p],
    "mpc_get_option": [_vp, C.c_char_p, C.POINTER(C.c_int64)],
    "mpc_get_profile": [_vp, _dp],
    "mpc_get_pipeline_profile": [_vp, _dp],
    "mpc_get_resident_profile": [_vp, _dp],
    "mpc_measure_copy_bandwidth": [_vp, C.c_size_t, _i32, _dp],
    "mpc_last_rescued": [_vp],
    "mpc_last_loop_replayed": [_vp],
    "mpc_solve_batch": [_vp, _i32] + _rows,
    "mpc_solve_batch_dev": [_vp, _i32] + [_vp] * 8,
    "mpc_solve_batch_trace": [_vp, _i32] + _rows + [_dp, _i32, _ip],
    "mpc_eval_nlp_batch": [_vp, _i32] + [_dp] * 5,
    "mpc_eval_nlp_batch_dev": [_vp, _i32] + [_vp] * 6,
    "mpc_solve_batch_ex": [_vp, _i32] + _rows + [_dp] * 4,
    "mpc_solve_batch_dev_ex": [_vp, _i32] + [_vp] * 12,
    "mpc_solve_batch_stages": [_vp, _i32] + _rows + [_dp] * 4,
    "mpc_solve_batch_stages_dev": [_vp, _i32] + [_vp] * 12,
    "mpc_eval_nlp_batch_stages": [_vp, _i32] + [_dp] * 5,
    "mpc_eval_nlp_batch_stages_dev": [_vp, _i32] + [_vp] * 6,
    "mpc_solve_batch_sized": [_vp, _i32] + _rows[:3] + [_dp] + _rows[3:] + [_dp] * 4,          # _stages with rsum behind obst
    "mpc_solve_batch_sized_dev": [_vp, _i32] + [_vp] * 13,
    "mpc_solve_batch_sens": [_vp, _i32] + _rows + [_dp] * 5 + [_i32, _dp, _dp],
    "mpc_solve_batch_sens_dev": [_vp, _i32] + [_vp] * 12 + [_i32, _vp, _vp, _vp],
    "mpc_sens_adjoint": [_vp, _i32, _dp, _dp],
    "mpc_sens_adjoint_dev": [_vp, _i32, _vp, _vp, _vp],
    "mpc_sens_obst": [_vp, _i32, _i32, _dp, _dp, _dp, _dp, _dp],
    "mpc_sens_obst_dev": [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp],
    "mpc_sens_weights": [_vp, _i32, _dp, _i32, _dp, _dp, _dp, _dp, _dp],
    "mpc_sens_weights_dev": [_vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp],
    "mpc_sens_bounds": [_vp, _i32, _i32, _dp, _dp, _dp, _dp, _dp],
    "mpc_sens_bounds_dev": [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp],
    "mpc_plant_step": [_vp, _i32, _i32, _dp, _dp, _dp],
    "mpc_plant_step_dev": [_vp, _i32, _i32] + [_vp] * 4,
    "mpc_closed_loop_batch": [_vp, _i32, _i32, _i32] + [_dp] * 6 + [_ip],
    "mpc_closed_loop_batch_dev": [_vp, _i32, _i32, _i32] + [_vp] * 8,
    "mpc_closed_loop_batch_ex": [_vp, _i32, _i32, _i32] + [_dp] * 4 + _loop_tail + [_dp, _dp, _ip],
    "mpc_closed_loop_batch_dev_ex": [_vp, _i32, _i32, _i32] + [_vp] * 4 + _loop_tail + [_vp] * 4,
    "mpc_closed_loop_batch_obst": [_vp, _i32, _i32, _i32] + [_dp] * 4 + [_i32, _dp, _f64] + _loop_tail + [_dp, _dp, _ip, _dp],
    "mpc_closed_loop_batch_obst_dev": [_vp, _i32, _i32, _i32] + [_vp] * 4 + [_i32, _vp, _f64] + _loop_tail + [_vp] * 5,
    "mpc_closed_loop_batch_pred": [_vp, _i32, _i32, _i32] + [_dp] * 4 + [_i32, _dp, _f64, _i32] + _loop_tail + [_dp, _dp, _ip, _dp],
    "mpc_closed_loop_batch_pred_dev": [_vp, _i32, _i32, _i32] + [_vp] * 4 + [_i32, _vp, _f64, _i32] + _loop_tail + [_vp] * 5,
    "mpc_closed_loop_batch_traffic": [_vp, _i32, _i32, _i32] + [_dp] * 4 + [_i32, _i32, _i32, _dp, _dp, _i32] + _loop_tail + [_dp, _dp, _ip, _dp, _ip, _ip],
    "mpc_closed_loop_batch_traffic_dev": [_vp, _i32, _i32, _i32] + [_vp] * 4 + [_i32, _i32, _i32, _vp, _vp, _i32] + _loop_tail + [_vp] * 7,
    "mpc_closed_loop_batch_traffic_sized": [_vp, _i32, _i32, _i32] + [_dp] * 4 + [_i32, _i32, _i32, _dp, _dp, _dp, _i32] + _loop_tail + [_dp, _dp, _ip, _dp, _ip, _ip],
    "mpc_closed_loop_batch_traffic_sized_dev": [_vp, _i32, _i32, _i32] + [_vp] * 4 + [_i32, _i32, _i32, _vp, _vp, _vp, _i32] + _loop_tail + [_vp] * 7,
    "mpc_session_begin": [_vp, _i32, _i32, _i32] + [_dp] * 4 + [_i32, _i32, _dp, _i32],
    "mpc_session_begin_dev": [_vp, _i32, _i32, _i32] + [_vp] * 4 + [_i32, _i32, _vp, _i32, _vp],
    "mpc_session_step": [_vp, _dp, _dp, _dp, _dp, _ip, _dp, _ip, _ip],
    "mpc_session_step_dev": [_vp] + [_vp] * 8 + [_vp],
    "mpc_session_begin_sized": [_vp, _i32, _i32, _i32] + [_dp] * 4 + [_i32, _i32, _dp, _dp, _i32],                  # rsums behind offsets
    "mpc_session_begin_sized_dev": [_vp, _i32, _i32, _i32] + [_vp] * 4 + [_i32, _i32, _vp, _vp, _i32, _vp],
    "mpc_session_step_pred": [_vp, _dp, _dp, _dp, _dp, _ip, _dp, _ip, _ip],                                         # pred in the place of obs
    "mpc_session_step_pred_dev": [_vp] + [_vp] * 8 + [_vp],
    "mpc_session_record": [_vp, _dp, _dp, _ip],
    "mpc_session_record_dev": [_vp] + [_vp] * 3 + [_vp],
    "mpc_session_steps_done": [_vp],
    "mpc_session_end": [_vp],
    "mpc_closed_loop_batch_lin": [_vp, _i32, _i32, _i32] + [_dp] * 4 + [_i32, _dp, _f64] + _loop_tail + [_dp, _dp, _ip, _dp] + [_dp] * 3,
    "mpc_closed_loop_batch_lin_dev": [_vp, _i32, _i32, _i32] + [_vp] * 4 + [_i32, _vp, _f64] + _loop_tail + [_vp] * 8,
    "mpc_loop_tangent": [_vp, _i32, _i32, _i32] + [_dp] * 5 + [_i32] + [_dp] * 5,
    "mpc_loop_tangent_dev": [_vp, _i32, _i32, _i32] + [_vp] * 5 + [_i32] + [_vp] * 6,
    "mpc_loop_adjoint": [_vp, _i32, _i32] + [_dp] * 5 + [_i32] + [_dp] * 5,
    "mpc_loop_adjoint_dev": [_vp, _i32, _i32] + [_vp] * 5 + [_i32] + [_vp] * 6,
    "mpc_metrics_batch": [_vp, _i32, _i32, _i32, _dp, _dp, _dp, _f64, _i32, _dp, _dp, _dp],
    "mpc_metrics_batch_dev": [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _f64, _i32] + [_vp] * 4,
    "mpc_validity_batch": [_vp, _i32, _i32, _dp, _f64, _f64, _i32, _dp, _i32, _dp, _i32, _dp, _ip, _ip],
    "mpc_validity_batch_dev": [_vp, _i32, _i32, _vp, _f64, _f64, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp],
    "mpc_validity_batch_ego": [_vp, _i32, _i32, _dp, _f64, _f64, _i32, _dp, _i32, _dp, _i32, _dp, _ip, _ip],
    "mpc_validity_batch_ego_dev": [_vp, _i32, _i32, _vp, _f64, _f64, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp],
    "mpc_forces_stage_eval": [_vp, _i32, _i32] + [_dp] * 8,
    "mpc_forces_solve_batch": [_vp, _i32] + [_dp] * 7 + [_i32, _dp, _ip, _ip, _dp],
    "mpc_forces_solve_batch_dev": [_vp, _i32, _vp, _vp, _vp, _dp, _dp, _dp, _dp, _i32] + [_vp] * 5,
    "mpc_forces_closed_loop_batch": [_vp, _i32, _i32, _i32] + [_dp] * 9 + [_i32] + _loop_tail + [_dp, _dp, _ip],
    "mpc_forces_closed_loop_batch_dev": [_vp, _i32, _i32, _i32] + [_vp] * 5 + [_dp] * 4 + [_i32] + _loop_tail + [_vp] * 4,
    "mpc_forces_closed_loop_batch_obst": [_vp, _i32, _i32, _i32] + [_dp] * 9 + [_i32, _i32, _i32, _dp, _f64, _i32, _f64] + _loop_tail + [_dp, _dp, _ip, _dp],
    "mpc_forces_closed_loop_batch_obst_dev": [_vp, _i32, _i32, _i32] + [_vp] * 5 + [_dp] * 4 + [_i32, _i32, _i32, _vp, _f64, _i32, _f64] + _loop_tail + [_vp] * 5,
}
RESTYPES = {"mpc_default_desc": None, "mpc_last_error": C.c_char_p, "mpc_abi_version": C.c_int}       # every other entry point returns an int code
EXPORTS = list(PROTOTYPES)


class MpcLibraryError(RuntimeError):
    pass


_lib = None


def load_library(path: str | None = None):
    """dlopen libmpcgpu.so and declare the prototypes of include/mpcgpu.h; raises if it is not there."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or LIB_PATH
    if os.environ.get("MPCGPU_NO_TORCH") != "1":
        # torch wheels bundle their own libamdhip64.so.7 / libhsa-runtime64; a process must hold ONE HIP runtime
        # (and stream handles passed to mpc_solve_batch_dev must belong to it), so let torch load its copy first
        # and libmpcgpu.so binds to the same SONAME.  Loading in the other order leaves torch without a GPU.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    if not os.path.exists(path):
        raise MpcLibraryError(
            f"{path} not found: the HIP extension is not built. Run `python __graft_entry__.py build` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    try:
        L = C.CDLL(path)
    except OSError as e:  # pragma: no cover
        raise MpcLibraryError(f"cannot load {path}: {e}") from e
    for name, argtypes in PROTOTYPES.items():
        fn = getattr(L, name)
        fn.argtypes, fn.restype = argtypes, RESTYPES.get(name, C.c_int)
    if path == LIB_PATH:
        _lib = L
    return L


def as_dp(a):
    return None if a is None else a.ctypes.data_as(_dp)


def as_ip(a):
    return None if a is None else a.ctypes.data_as(_ip)


def f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a
