"""Shared by tests/test_session_cpu.py and tests/test_gpu_session.py (TEST INFRASTRUCTURE): numpy restatement of the two device pieces of the stepping
session (include/mpcgpu.h, mpc_session_step; csrc/mpc_closed_loop.h, session_ingest_instance and session_traffic_stage) -- the selection itself is
tests/traffic_ref.py's, on the observed poses moved on at constant velocity -- and the step-by-step host loop a caller would have to write without the
session: CasadiOptimizer's shift / warm_start / reference window, optimizer.nearest_obstacle_centres on the extrapolated poses, one solve(obst=[B, N+1, 6])
per step and a plant of the caller's."""
import types

import numpy as np

import loop_obst_ref as lref
import traffic_ref as tref

opt = lref.opt


def ingest(measured, state, p, N, nx):
    """(state', p') after the measured states [B, 5] have been taken in: a row whose x is not finite changes nothing"""
    measured, state, p = np.asarray(measured, dtype=np.float64), np.array(state, dtype=np.float64), np.array(p, dtype=np.float64)
    ok = np.isfinite(measured[:, 0])
    state[ok, :5] = measured[ok]
    p[ok, 2 * N: 2 * N + 5] = measured[ok]
    return state, p


def extrapolate(obs, N, dt):
    """obs [..., M, 5] = (x, y, heading, vx, vy) now -> [..., M, N+1, 3]: row k = the pose k dt ahead at constant velocity; a velocity that is not
    finite counts as 0, an x that is not finite stays so (absent)"""
    obs = np.asarray(obs, dtype=np.float64)
    ahead = np.arange(N + 1) * dt
    v = np.where(np.isfinite(obs[..., 3:5]), obs[..., 3:5], 0.0)
    xy = obs[..., None, 0:2] + ahead[:, None] * v[..., None, :]
    return np.concatenate([xy, np.broadcast_to(obs[..., None, 2:3], xy.shape[:-1] + (1,))], axis=-1)


def select(step, state, x0, obs, offsets, pairing, ego_offset, desc_obst, N, nx, dt):
    """(rows [B, N+1, 6], chosen [B, N+1, 3], margin [B, N+1, 3]) of the solve of session step `step`"""
    poses = tref.ego_poses(step, state, x0, N, nx)
    return tref.select(0, poses, extrapolate(obs, N, dt), offsets, pairing, ego_offset, desc_obst)


def clearance(state, obs, offsets, ego_offset, r_sum):
    """(clearance [B], nearest [B], margin [B]) of the states against the observed poses, all nine pairs"""
    return tref.clearance(0, state, np.asarray(obs, dtype=np.float64)[..., None, :3], offsets, ego_offset, r_sum)


def host_loop(backend, init, path, orient, vdes, L, N, dt, observe=None, offsets=None, pairing=0, ego_offset=0.0, desc_obst=tref.DESC_OBST, plant=None,
              before_step=None):
    """The loop of the session on the host, nx = 5: `backend.solve(x0, p[, obst])` per step for all B egos at once.
    observe(i) -> obs [M, 5] at step i (None: no obstacles, plain solves); plant(i, x [B, 5], u [B, 2]) -> the measured states of step i + 1 (None: the
    model's forward-Euler step); before_step(i) runs first in step i.
    -> dict(traj [B, L, 5], ctrl [B, L, 2], status [B, L], plan [L, B, n_w], chosen [L, B, N+1, 3])"""
    init = np.atleast_2d(np.asarray(init, dtype=np.float64))
    B = init.shape[0]
    vdes = np.broadcast_to(np.asarray(vdes, dtype=np.float64), (B,))
    egos = [types.SimpleNamespace(iter_length=L, predict_horizon=N, resampled_path_points=np.asarray(path[b]), desired_velocity=vdes[b],
                                  orientation=np.asarray(orient[b])) for b in range(B)]
    x_now = init.copy()
    plan_u = [np.zeros((2, N)) for _ in range(B)]
    plan_x = [np.tile(x_now[b][:, None], (1, N + 1)) for b in range(B)]
    window = [np.tile(x_now[b], (N + 1, 1)) for b in range(B)]
    out = dict(traj=np.empty((B, L, 5)), ctrl=np.empty((B, L, 2)), status=np.empty((B, L), np.int32), plan=[], chosen=[])
    for i in range(L):
        if before_step is not None:
            before_step(i)
        for b in range(B):
            window[b][0] = x_now[b]                                   # (the measured state: row 0 of X_ref)
        p = np.stack([np.concatenate((np.zeros(2 * N), window[b].ravel())) for b in range(B)])
        w0 = np.stack([opt.CasadiOptimizer.warm_start(plan_u[b], plan_x[b], first=(i == 0)).ravel() for b in range(B)])
        kw = {}
        if observe is not None:
            tracks = extrapolate(observe(i), N, dt)                   # [M, N+1, 3]
            picked = [opt.nearest_obstacle_centres(np.tile(x_now[b][[0, 1, 4]], (N + 1, 1)) if i == 0 else plan_x[b][[0, 1, 4]].T, tracks, offsets,
                                                   np.arange(N + 1), ego_offset, pairing, desc_obst) for b in range(B)]
            kw = dict(obst=np.stack([c for c, _ in picked]))
            out["chosen"].append(np.stack([m for _, m in picked]))
        r = backend.solve(w0, p, **kw)
        out["plan"].append(np.array(r.x))
        out["status"][:, i] = r.status
        out["traj"][:, i] = x_now
        for b in range(B):
            plan_u[b] = r.x[b, :2 * N].reshape(N, 2).T
            plan_x[b] = r.x[b, 2 * N:].reshape(N + 1, 5).T
        u = np.stack([plan_u[b][:, 0] for b in range(B)])
        out["ctrl"][:, i] = u
        predicted = np.stack([x_now[b] + dt * opt.VehicleDynamics.KS_casadi(x_now[b], u[b]) for b in range(B)])
        for b in range(B):
            plan_u[b], plan_x[b] = opt.CasadiOptimizer.shift(plan_u[b]), opt.CasadiOptimizer.shift(plan_x[b])
            window[b], _ = opt.CasadiOptimizer.desired_command_and_trajectory(egos[b], i, predicted[b], N)
        x_now = predicted if plant is None else np.asarray(plant(i, x_now, u), dtype=np.float64).reshape(B, 5)
    out["plan"], out["chosen"] = np.array(out["plan"]), np.array(out["chosen"])
    return out


# ---- the scene no existing loop can express: the obstacle ahead halves its speed at step BRAKE_AT, the plant integrates with RK4 -------------------------
# The ego swerves 0.24 m and is beside the obstacle's rear when the loop ends.  The speed is chosen for the plant: an obstacle at 4 m/s is passed
# within the 40 steps, and while the ego turns back beside it the state of an RK4 plant lies 3 mm inside the distance the Euler model's plan
# kept; stage 0 is pinned to the measurement, so that NLP is infeasible whatever the radius (host loop and session alike, steps 33 - 35).
BRAKE_AT = 15
BRAKE_LATERAL, BRAKE_SPEED = -2.9, 6.0


def braking_obs(i, knows=True):
    """obs [1, 5] at step i: the obstacle of the scenes, AHEAD of the ego at BRAKE_SPEED until step BRAKE_AT, at half of it afterwards; knows=False: the
    pose is the true one, the reported speed stays the old one"""
    t_fast, t_slow = min(i, BRAKE_AT) * lref.DT, max(i - BRAKE_AT, 0) * lref.DT
    v = BRAKE_SPEED if (i < BRAKE_AT or not knows) else BRAKE_SPEED / 2
    return np.array([[lref.AHEAD + BRAKE_SPEED * t_fast + BRAKE_SPEED / 2 * t_slow, BRAKE_LATERAL, 0.0, v, 0.0]])
