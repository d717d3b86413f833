"""Shared by tests/test_forces_loop_obst_cpu.py and tests/test_gpu_forces_loop_obst.py (TEST INFRASTRUCTURE): a numpy host loop of the FORCES-mode
closed loop past per-ego obstacles (include/mpcgpu.h, mpc_forces_closed_loop_batch_obst) over any `solve(zbar, params, xinit) -> (z_out, exitflag)`
callable -- the bookkeeping (parameter rows, guess, plant, noise, clearance) restated in numpy, independent of csrc/mpc_closed_loop.h --, the scenes
and the ego families of the tests, and the emulated solver (the kernel's own QP code on the CPU, tests/emu)."""
import numpy as np

import forces_families as FF
from helpers import emu_forces_solve, pkg
from oracle import forces_model_numpy as FM

nz = __import__("importlib").import_module(pkg.__name__ + ".noise")

LB, UB, HL, HU = FF.LB, FF.UB, FF.HL, FF.HU
WEIGHTS = FM.WEIGHTS_MODEL_C
DT, WHEELBASE, FRICTION_DIV, EGO_OFFSET = 0.1, FM.WHEELBASE_ODE, FM.WHEELBASE_FRICTION, FM.EGO_OFFSET
OBST_OFFSET, R_SUM = 1.0, 3.3
STEPS = 40                                   # the steps the conditions refer to: none of their stages sees the velocity ramp


def run_length(N):
    """(L, Lp) of the scenes at horizon N"""
    L = STEPS + 2 * N
    return L, L + N + 1


# ---- the bookkeeping, in numpy ---------------------------------------------------------------------------------------------------------------
def centres(pose, offset):
    """[..., 3] poses (x, y, heading) -> [..., 6] circle centres: the centre, then +- offset along the heading"""
    p = np.asarray(pose, dtype=np.float64)
    cs, sn = np.cos(p[..., 2]), np.sin(p[..., 2])
    return np.stack([p[..., 0], p[..., 1], p[..., 0] + offset * cs, p[..., 1] + offset * sn, p[..., 0] - offset * cs, p[..., 1] - offset * sn], axis=-1)


def clearance9(state, c6, ego_offset=EGO_OFFSET, r_sum=R_SUM):
    """min over all nine circle pairs of distance - r_sum (rows 1..9 of forces_model_numpy.stage_functions); state [..., 5], c6 [..., 6]"""
    s, c = np.asarray(state, dtype=np.float64), np.asarray(c6, dtype=np.float64)
    d = []
    for sg in (0.0, 1.0, -1.0):
        ex, ey = s[..., 0] + sg * ego_offset * np.cos(s[..., 4]), s[..., 1] + sg * ego_offset * np.sin(s[..., 4])
        for j in range(3):
            d.append(np.hypot(ex - c[..., 2 * j], ey - c[..., 2 * j + 1]))
    return np.min(d, axis=0) - r_sum


def pose_rows(k, N, Lt, predict):
    """the track row that stage j = 0..N-1 of step k sees"""
    return np.minimum(k + np.arange(N) if predict else np.full(N, k), Lt - 1)


def param_rows(k, N, L, path, orient, vdes, track=None, offset=OBST_OFFSET, predict=0, obstacle=None):
    """all_parameters [B,N,10] of step k: path point / orientation k + 1 + j (replenished with the last one), the desired velocity ramping to 0 over
    the last N indices of the run, six circle centres -- of the track's pose row, or `obstacle` [6] without a track"""
    B, Lp = path.shape[:2]
    idx = k + 1 + np.arange(N)
    ip = np.minimum(idx, Lp - 1)
    out = np.empty((B, N, 10))
    out[:, :, 0:2] = path[:, ip]
    out[:, :, 3] = orient[:, ip]
    for b in range(B):
        v_all = np.hstack((np.ones(L - N) * vdes[b], np.linspace(vdes[b], 0, N)))
        out[b, :, 2] = v_all[np.minimum(idx, L - 1)]
    if track is None:
        out[:, :, 4:] = np.asarray(obstacle, dtype=np.float64)
    else:
        out[:, :, 4:] = centres(track[:, pose_rows(k, N, track.shape[1], predict)], offset)
    return out


def next_guess(zbar, z_out, flag, guess_mode):
    """the guess after a solve: the solution shifted by one stage where the exitflag is 1 (guess_mode 1), left alone otherwise"""
    out = zbar.copy()
    if guess_mode == 1:
        ok = np.asarray(flag) == 1
        out[ok] = np.concatenate((z_out[ok, 1:], z_out[ok, -1:]), axis=1)
    return out


def rk4(x, u, dt=DT, l=WHEELBASE):
    def f(s):
        return np.stack([s[:, 3] * np.cos(s[:, 4]), s[:, 3] * np.sin(s[:, 4]), u[:, 0], u[:, 1], s[:, 3] / l * np.tan(s[:, 2])], axis=1)
    k1 = f(x)
    k2 = f(x + 0.5 * dt * k1)
    k3 = f(x + 0.5 * dt * k2)
    k4 = f(x + dt * k3)
    return x + dt / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4)


def host_loop(solve, init_state, path, orient, vdes, L, N, track=None, offset=OBST_OFFSET, predict=0, guess_mode=0, obstacle=None, steps=None,
              init_acc=None, sigma=0.0, seed=None, r_sum=R_SUM, ego_offset=EGO_OFFSET, log=None, dt=DT, wheelbase=WHEELBASE):
    """the loop of B egos: dict(traj [B,S,5], ctrl [B,S,2], flag [B,S], clearance [B,S] | None) over the first S = `steps` (default L) steps of a run
    of L.  seed: the applied-input noise of noise mode 2.  log: a list that receives (zbar, params, xinit) of every solve.  dt, wheelbase: the plant's
    (RK4), ego_offset / r_sum: the clearance's."""
    init_state = np.asarray(init_state, dtype=np.float64)
    B = init_state.shape[0]
    S = L if steps is None else steps
    x = init_state.copy()
    x[:, 2] = 0.0
    z0 = np.zeros((B, 7))
    z0[:, 1] = 0.0 if init_acc is None else init_acc
    z0[:, 2], z0[:, 3], z0[:, 5], z0[:, 6] = init_state[:, 0], init_state[:, 1], init_state[:, 3], init_state[:, 4]
    zbar = np.repeat(z0[:, None, :], N, axis=1)
    traj, ctrl, flag = np.empty((B, S, 5)), np.empty((B, S, 2)), np.empty((B, S), np.int32)
    cl = None if track is None else np.empty((B, S))
    for k in range(S):
        par = param_rows(k, N, L, path, orient, vdes, track, offset, predict, obstacle)
        if cl is not None:
            cl[:, k] = clearance9(x, centres(track[:, min(k, track.shape[1] - 1)], offset), ego_offset, r_sum)
        if log is not None:
            log.append((zbar.copy(), par.copy(), x.copy()))
        z_out, fl = solve(zbar, par, x)
        u = z_out[:, 0, 0:2].copy()
        if seed is not None:
            u += np.array([nz.applied_noise(seed, b, k, sigma) for b in range(B)])
        traj[:, k], ctrl[:, k], flag[:, k] = x, u, fl
        zbar = next_guess(zbar, z_out, fl, guess_mode)
        x = rk4(x, u, dt, wheelbase)
    return dict(traj=traj, ctrl=ctrl, flag=flag, clearance=cl)


def emu_solver(N, hessian_mode=0):
    """solve(zbar, params, xinit) on the emulated kernel (tests/emu: forces_qp_instance, instance after instance)"""
    def solve(zbar, params, xinit):
        zo, _, st, _ = emu_forces_solve(zbar, params, xinit, WEIGHTS, LB, UB, HL, HU, hessian_mode, dt=DT, wheelbase=WHEELBASE, friction_div=FRICTION_DIV,
                                        ego_offset=EGO_OFFSET)
        return zo, st
    return solve


def backend_solver(be):
    """solve(zbar, params, xinit) on a BatchedMPCSolver: mpc_forces_solve_batch, the kernel the device loop launches"""
    def solve(zbar, params, xinit):
        x, fl, _, _ = be.forces_solve(zbar, xinit, params, LB, UB, HL, HU)
        return x, fl
    return solve


# ---- scenes (one ego) and families (B egos) --------------------------------------------------------------------------------------------------
def ego_inputs(B, N, v0, y0=None, dt=DT):
    """init_state [B,5] on the path (v0 dt i, 0), path [B,Lp,2], orient [B,Lp], vdes [B]"""
    L, Lp = run_length(N)
    init = np.tile([0.0, 0.0, 0.0, v0, 0.0], (B, 1))
    if y0 is not None:
        init[:, 1] = y0
    path = np.zeros((B, Lp, 2))
    path[:, :, 0] = v0 * dt * np.arange(Lp)
    return init, path, np.zeros((B, Lp)), np.full(B, float(v0))


def scene(name, N=10):
    """dict(init, path, orient, vdes, track [1,Lt,3], L, N) of 'overtake' (v0 = 10, the obstacle at (15 + 0.4 i, -2.5, 0) at step i) or 'parked'
    (v0 = 6, the obstacle standing at (14, -2.2, 0): Lt = 1)"""
    L, _ = run_length(N)
    if name == "overtake":
        v0 = 10.0
        i = np.arange(L)
        track = np.stack([15.0 + 0.4 * i, np.full(L, -2.5), np.zeros(L)], axis=1)[None]
    elif name == "parked":
        v0 = 6.0
        track = np.array([[[14.0, -2.2, 0.0]]])
    else:
        raise KeyError(name)
    init, path, orient, vdes = ego_inputs(1, N, v0)
    return dict(init=init, path=path, orient=orient, vdes=vdes, track=np.ascontiguousarray(track), L=L, N=N)


MODES = {"today": (0, 0), "shifted": (1, 0), "predicted": (1, 1)}       # name -> (guess_mode, predict): the rows of the table in DESIGN.md section 11


def run_scene(solve, sc, guess_mode, predict, steps=STEPS, **kw):
    return host_loop(solve, sc["init"], sc["path"], sc["orient"], sc["vdes"], sc["L"], sc["N"], track=sc["track"], predict=predict,
                     guess_mode=guess_mode, steps=steps, **kw)


def overtake_family(B, N, seed=7, dt=DT):
    """B egos at 10 m/s, each past its own obstacle: speed U(3.5, 4.5) m/s, lateral U(-2.7, -2.3), start U(14, 17)"""
    rng = np.random.default_rng(seed)
    L, _ = run_length(N)
    speed, lat, start = rng.uniform(3.5, 4.5, B), rng.uniform(-2.7, -2.3, B), rng.uniform(14.0, 17.0, B)
    i = np.arange(L)
    track = np.stack([start[:, None] + speed[:, None] * dt * i, np.repeat(lat[:, None], L, axis=1), np.zeros((B, L))], axis=2)
    return ego_inputs(B, N, 10.0, dt=dt) + (np.ascontiguousarray(track),)


def parked_family(B, N, seed=7):
    """B egos at 6 m/s, each past its own standing obstacle (Lt = 1): at x U(13, 15), lateral U(-2.4, -2.2)"""
    rng = np.random.default_rng(seed)
    track = np.stack([rng.uniform(13.0, 15.0, B), rng.uniform(-2.4, -2.2, B), np.zeros(B)], axis=1)[:, None, :]
    return ego_inputs(B, N, 6.0) + (np.ascontiguousarray(track),)


def weaving_family(B, N, seed=7):
    """B egos at 10 m/s with lateral starts U(-0.2, 0.2), the obstacle of each at lateral -6 with heading 0.3 sin(0.1 i + phase): far enough to stay
    inactive, near enough for its centres to matter to the linearisation"""
    rng = np.random.default_rng(seed)
    L, _ = run_length(N)
    start, phase = rng.uniform(14.0, 17.0, B), rng.uniform(0.0, 2 * np.pi, B)
    i = np.arange(L)
    track = np.stack([start[:, None] + 0.4 * i, np.full((B, L), -6.0), 0.3 * np.sin(0.1 * i + phase[:, None])], axis=2)
    return ego_inputs(B, N, 10.0, y0=rng.uniform(-0.2, 0.2, B)) + (np.ascontiguousarray(track),)
