"""Shared by tests/test_session_sized_cpu.py and tests/test_gpu_session_sized.py (TEST INFRASTRUCTURE): what the sized session and the session stepped
with predicted poses (include/mpcgpu.h, mpc_session_begin_sized / mpc_session_step_pred) need beyond tests/session_ref.py, tests/traffic_ref.py and
tests/sized_ref.py -- the poses a caller would predict from a track, and the step-by-step host loop a caller would have to write without the session:
CasadiOptimizer's shift / warm_start / reference window, tests/sized_ref.py's selection by clearance on the predicted poses, one
solve(obst=[B, N+1, 6], rsum=[B, N+1, 3]) per step."""
import types

import numpy as np

import session_ref as sref
import sized_ref as zref

opt = sref.opt


def predicted(tracks, i, N):
    """tracks [..., Lt, 3] -> pred [..., N+1, 3] of step i: row k is track row min(i + k, Lt - 1), the row the loops show stage k of step i"""
    tracks = np.asarray(tracks, dtype=np.float64)
    return np.ascontiguousarray(tracks[..., np.minimum(i + np.arange(N + 1), tracks.shape[-2] - 1), :])


def observed(tracks, i, dt):
    """tracks [..., Lt, 3] -> obs [..., 5] at step i: the pose of row min(i, Lt - 1) and the finite difference to the next row as velocity (0 beyond
    the track's end)"""
    tracks = np.asarray(tracks, dtype=np.float64)
    Lt = tracks.shape[-2]
    a, b = min(i, Lt - 1), min(i + 1, Lt - 1)
    vel = (tracks[..., b, :2] - tracks[..., a, :2]) / dt
    return np.ascontiguousarray(np.concatenate([tracks[..., a, :], vel], axis=-1))


def host_loop_sized(backend, init, path, orient, vdes, L, N, dt, predict, offsets, rsums, r_handle, pairing, ego_offset, desc_obst):
    """The loop of a sized session stepped with predicted poses, on the host, one ego (nx = 5), measured None: predict(i) -> pred [M, N+1, 3] of
    step i; per step the selection by clearance (tests/sized_ref.py, select_sized) from the state at step 0 and from the shifted last plan
    afterwards, and `backend.solve(x0, p, obst=, rsum=)`.
    -> dict(traj [L, 5], ctrl [L, 2], status [L], chosen [L, N+1, 3])"""
    x_now = np.asarray(init, dtype=np.float64).reshape(5).copy()
    ego = types.SimpleNamespace(iter_length=L, predict_horizon=N, resampled_path_points=np.asarray(path), desired_velocity=float(vdes),
                                orientation=np.asarray(orient))
    plan_u, plan_x = np.zeros((2, N)), np.tile(x_now[:, None], (1, N + 1))
    window = np.tile(x_now, (N + 1, 1))
    out = dict(traj=np.empty((L, 5)), ctrl=np.empty((L, 2)), status=np.empty(L, np.int32), chosen=np.empty((L, N + 1, 3), np.int64))
    for i in range(L):
        window[0] = x_now
        p = np.concatenate((np.zeros(2 * N), window.ravel()))[None]
        w0 = opt.CasadiOptimizer.warm_start(plan_u, plan_x, first=(i == 0)).ravel()[None]
        poses = (np.tile(x_now[[0, 1, 4]], (N + 1, 1)) if i == 0 else plan_x[[0, 1, 4]].T)[None]
        rows, rad, chosen, _ = zref.select_sized(0, poses, predict(i), offsets, rsums, r_handle, pairing, ego_offset, desc_obst)
        r = backend.solve(w0, p, obst=rows, rsum=rad)
        out["traj"][i], out["status"][i], out["chosen"][i] = x_now, r.status[0], chosen[0]
        plan_u, plan_x = r.x[0, :2 * N].reshape(N, 2).T, r.x[0, 2 * N:].reshape(N + 1, 5).T
        u = plan_u[:, 0].copy()
        out["ctrl"][i] = u
        x_now = x_now + dt * np.asarray(opt.VehicleDynamics.KS_casadi(x_now, u), dtype=np.float64).ravel()
        plan_u, plan_x = opt.CasadiOptimizer.shift(plan_u), opt.CasadiOptimizer.shift(plan_x)
        window, _ = opt.CasadiOptimizer.desired_command_and_trajectory(ego, i, x_now, N)
        window = np.array(window, dtype=np.float64)
    return out
