"""Shared by tests/test_loop_lin_cpu.py and tests/test_gpu_loop_lin.py (TEST INFRASTRUCTURE): the numpy chained reference of the linearised
closed loop (mpc_closed_loop_batch_lin, mpc_loop_tangent, mpc_loop_adjoint).

The closed loop on the C oracle (the numpy mirror of csrc/mpc_closed_loop.h around OracleSolver.solve, one solve per step that sees the step's
obstacle); at every step the multipliers of the oracle's optimum by least squares (sens_ref.ls_multipliers) and the three active-set derivatives
(sens_ref / sens_weights_ref / sens_obst_ref .sensitivity_matrix), reduced to the per-step gains of the first control; the tangent and adjoint
recursions over them through the plant Jacobian; and central differences of the oracle loop itself, relative steps FD_REL.
"""
import dataclasses
import functools

import numpy as np

import loop_obst_ref as obst_ref
import sens_obst_ref
import sens_ref
import sens_weights_ref
from helpers import WEIGHTS_ZAM_LF, NLPConfig
from oracle.binding import OracleSolver
from oracle.nlp_numpy import circle_centers

FD_REL = 1e-5
TOL_FD = 1e-3                     # reference against central differences, max|delta| / max|FD| per direction (worst measured: LF 8.6e-7, OB 1.8e-5)
FD_FLOOR = 1e-6                   # directions whose FD scale is below this are skipped (symmetric scenes), MAX_SKIPPED per scene at most
MAX_SKIPPED = 2
# per-step gains against this reference: the per-family bounds the single-solve derivatives are held to (the math is the same)
TOL_K = 1e-5                      # the p family: TOL_DW of tests/test_gpu_sensitivities.py
TOL_W = sens_weights_ref.TOL_DW   # the weights
TOL_O = 1e-5                      # the obstacle centres: TOL_DW of tests/test_gpu_sens_obst.py
# the tangent over the whole loop, CPU harness (tests/looplinx) against this reference, max|delta| / max|reference| per direction
HARNESS_WORST_LOOP = 1.94e-5      # OB (the weakly active steps' gains included); LF 1.12e-7 (test_loop_lin_cpu.py::test_harness_against_reference prints them);
                                  # the device tangent against central differences of the device loop, worst ego: 4.0e-7
TOL_LOOP = min(10 * HARNESS_WORST_LOOP, 1e-3)

DT = 0.1
N_STATE, N_WT, N_POSE = 5, 7, 3


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Scene:
    cfg: NLPConfig                # weights, bounds, radii (the obstacle of a solve is the step's pose)
    L: int
    init: tuple                   # (x, y, delta, v, psi)
    vdes: float
    curv: float = 0.0
    lateral: float = None         # OB: the obstacle's lateral position; None: lane following, no track
    speed: float = 0.0

    def path(self):
        """path [L,2], orient [L]: the cumulative sum of vdes dt (cos, sin)(curv vdes dt k), dt the configuration's"""
        dt = self.cfg.dt
        th = self.curv * self.vdes * dt * np.arange(self.L)
        return np.cumsum(self.vdes * dt * np.stack([np.cos(th), np.sin(th)], axis=1), axis=0), th

    def track(self):
        return None if self.lateral is None else obst_ref.track_of((self.lateral, self.speed))[:self.L]


LF_CFG = NLPConfig(N=10, nx=5, **WEIGHTS_ZAM_LF)
LF_L = 24
LF_SCENES = [Scene(LF_CFG, LF_L, (0.0, lat, 0.0, v0, hd), 10.0, curv) for lat, hd, v0, curv in
             ((0.8, 0.0, 8.0, 0.0), (-1.5, 0.05, 12.0, 0.0), (0.3, -0.1, 10.0, 0.02), (2.5, 0.0, 6.0, -0.01))]
# the lane-following scenes away from the default descriptor (tests/descriptor_families.py: the closed loops at dt = 0.05, wheelbase = 3.1).  The
# starts are milder than LF_SCENES' and at or below the desired speed: with those starts at this dt the oracle loop passes through changes of the
# active set (a step of scene 2 is 1.8e-2 from central differences of the loop, a start above the desired speed brakes on a weakly active friction
# bound at step 0), where no active-set derivative is a reference.  With these, the reference is within 2.7e-5 of central differences of the oracle
# loop (bound TOL_FD), one step of scene 1 is weakly active and left out.
# tests/test_descriptor_cpu.py::test_loop_lin_harness_against_the_reference_off_the_default_descriptor measures the CPU harness (tests/looplinx)
# against this reference there (no kernel involved): gains k 1.63e-6, w 3.32e-6, the tangent over the loop 3.89e-6; the bounds at this point:
LFD_CFG = NLPConfig(N=10, nx=5, dt=0.05, wheelbase=3.1, **WEIGHTS_ZAM_LF)
LFD_SCENES = [Scene(LFD_CFG, LF_L, (0.0, lat, 0.0, v0, hd), 10.0, curv) for lat, hd, v0, curv in
              ((0.8, 0.0, 9.5, 0.0), (-1.0, 0.05, 9.8, 0.0), (0.3, -0.05, 10.0, 0.01), (1.2, 0.0, 9.0, -0.01))]
LFD_HARNESS_WORST = dict(k=1.63e-6, w=3.32e-6, loop=3.89e-6)
TOL_LFD = dict(k=min(10 * LFD_HARNESS_WORST["k"], TOL_K), w=min(10 * LFD_HARNESS_WORST["w"], TOL_W), loop=min(10 * LFD_HARNESS_WORST["loop"], TOL_LOOP))
OB_LATERALS = (-3.1, -2.9, -2.5, 2.5, 2.9, 3.2)


OB_SCENES = [Scene(obst_ref.CFG, obst_ref.L, (0.0, 0.0, 0.0, obst_ref.V_EGO, 0.0), obst_ref.V_EGO, 0.0, lat, 2.0) for lat in OB_LATERALS]


def scenes_of(kind):
    return {"LF": LF_SCENES, "OB": OB_SCENES, "LFD": LFD_SCENES}[kind]


def scene_path(scene):
    """(path [L,2], orient [L]); the OB scenes run on the straight path of tests/loop_obst_ref.py (its first point is the origin)"""
    return obst_ref.straight_path(scene.L, 0.0, 0.0, 0.0, scene.vdes) if scene.lateral is not None else scene.path()


def batch_inputs(scenes):
    """init [B,5], path [B,L,2], orient [B,L], vdes [B], track [B,L,3] | None of a list of scenes of one kind"""
    pts = [scene_path(s) for s in scenes]
    track = None if scenes[0].lateral is None else np.ascontiguousarray(np.stack([s.track() for s in scenes]))
    return (np.array([s.init for s in scenes], dtype=np.float64), np.ascontiguousarray(np.stack([p for p, _ in pts])),
            np.ascontiguousarray(np.stack([o for _, o in pts])), np.array([s.vdes for s in scenes], dtype=np.float64), track)


def cfg_at(cfg, pose):
    """cfg with its obstacle at pose (x, y, heading)"""
    return dataclasses.replace(cfg, obstacle=(pose[0], pose[1], cfg.obstacle[2], cfg.obstacle[3], pose[2]))


def centres_of(cfg, pose):
    return circle_centers(pose[0], pose[1], cfg.obstacle[2], cfg.obstacle[3], pose[2]).ravel()


def pose_jacobian(pose, offset):
    """d c6 / d (x, y, heading) [6, 3] of loop_obstacle_centres"""
    cs, sn = np.cos(pose[2]), np.sin(pose[2])
    J = np.zeros((6, 3))
    J[0::2, 0] = 1.0
    J[1::2, 1] = 1.0
    J[2:, 2] = [-offset * sn, offset * cs, offset * sn, -offset * cs]
    return J


# ---- the oracle loop (csrc/mpc_closed_loop.h: loop_setup_instance, loop_advance_instance, loop_write_reference; no noise) ---------------------
def oracle_loop(cfg, init, path, orient, vdes, L, track=None):
    """dict(traj [L,5], ctrl [L,2], status [L], w [L,n_w], p [L,n_w]) of one ego; track [Lt,3] | None (the configuration's own obstacle)"""
    N, nx, nw = cfg.N, cfg.nx, cfg.n_w
    assert nx == 5
    o = OracleSolver(cfg)
    cur = np.array(init, dtype=np.float64)
    x0, p = np.zeros(nw), np.zeros(nw)
    p[2 * N:] = np.tile(cur, N + 1)
    x0[2 * N:] = np.repeat(cur, N + 1)                      # (the transposed tile the reference really produces at step 0)
    out = dict(traj=np.zeros((L, 5)), ctrl=np.zeros((L, 2)), status=np.zeros(L, np.int32), w=np.zeros((L, nw)), p=np.zeros((L, nw)))
    for i in range(L):
        if track is not None:
            c6 = centres_of(cfg, track[min(i, len(track) - 1)])
            for q in range(6):
                o.desc.obst[q] = c6[q]
        r = o.solve(x0, p)
        w = r["x"]
        out["traj"][i], out["ctrl"][i], out["status"][i], out["w"][i], out["p"][i] = cur, w[:2], r["status"], w, p
        cur = o.plant_step(cur, w[:2])
        U, X = w[:2 * N].reshape(N, 2), w[2 * N:].reshape(N + 1, nx)
        src = np.minimum(np.arange(N) + 1, N - 1)
        x0 = np.concatenate([U[src, 0], U[src, 1], X[np.minimum(np.arange(N + 1) + 1, N)].ravel()])
        p = np.zeros(nw)
        p[2 * N: 2 * N + nx] = cur
        for k in range(N):
            idx = i + k + 1 - ((i - (L - N) + 1) if i >= L - N else 0)
            p[2 * N + nx * (k + 1): 2 * N + nx * (k + 2)] = [path[idx, 0], path[idx, 1], 0.0, vdes, orient[idx]]
    return out


def run_scene(scene, init=None, wt=None, track=None):
    cfg = scene.cfg if wt is None else sens_weights_ref.with_weights(scene.cfg, wt)
    path, orient = scene_path(scene)
    return oracle_loop(cfg, scene.init if init is None else init, path, orient, scene.vdes, scene.L, scene.track() if track is None else track)


# ---- per-step gains --------------------------------------------------------------------------------------------------------------------------
def step_gains(cfg, w, p, step0, pose=None, offset=0.0):
    """(K [2,5], W [2,7], O [2,3] | None, weak) at the optimum w of the solve with parameters p; pose: the obstacle's at this step"""
    N, nx = cfg.N, cfg.nx
    c = cfg if pose is None else cfg_at(cfg, pose)
    lam_g, lam_x = sens_ref.ls_multipliers(c, w, p)
    Sp, weak = sens_ref.sensitivity_matrix(c, w, p, lam_g, lam_x)
    cols = Sp[:2, 2 * N:].reshape(2, N + 1, nx)
    K = cols.sum(axis=1) if step0 else cols[:, 0]
    W = sens_weights_ref.sensitivity_matrix(c, w, p, lam_g, lam_x)[0][:2]
    O = None
    if pose is not None:
        So = sens_obst_ref.sensitivity_matrix(cfg, centres_of(cfg, pose), w, p, lam_g, lam_x)[0]
        O = So[:2] @ pose_jacobian(pose, offset)
    return K[:, :5], W, O, weak


def loop_gains(scene, run):
    """dict(kgain [L,2,5], wgain [L,2,7], ogain [L,2,3] | None, weak [L]) along the oracle loop `run` of the scene"""
    L, track = scene.L, scene.track()
    kg, wg, weak = np.zeros((L, 2, 5)), np.zeros((L, 2, 7)), np.zeros(L, bool)
    og = None if track is None else np.zeros((L, 2, 3))
    for i in range(L):
        K, W, O, weak[i] = step_gains(scene.cfg, run["w"][i], run["p"][i], i == 0, None if track is None else track[i], obst_ref.OFFSET)
        kg[i], wg[i] = K, W
        if og is not None:
            og[i] = O
    return dict(kgain=kg, wgain=wg, ogain=og, weak=weak)


# ---- the sweeps --------------------------------------------------------------------------------------------------------------------------
def plant_A(x, dt, wheelbase):
    """I + dt d f / d x of the kinematic bicycle at x (sens_stage_A)"""
    A = np.eye(5)
    A[0, 3], A[0, 4] = dt * np.cos(x[4]), -dt * x[3] * np.sin(x[4])
    A[1, 3], A[1, 4] = dt * np.sin(x[4]), dt * x[3] * np.cos(x[4])
    A[4, 2], A[4, 3] = dt * x[3] / (np.cos(x[2]) ** 2 * wheelbase), dt * np.tan(x[2]) / wheelbase
    return A


def tangent(traj, kgain, wgain, ogain, Lt, dinit, dwt, dtrack, dt, wheelbase, mag=False):
    """one ego, one direction: (dtraj [L,5], dctrl [L,2]).  None = zero.  mag=True: the recursion on absolute values, the sum of the absolute
    terms of every entry (the scale of its rounding error)"""
    f = np.abs if mag else (lambda a: a)
    L = traj.shape[0]
    ds = np.zeros(5) if dinit is None else f(np.array(dinit, dtype=np.float64))
    dtraj, dctrl = np.zeros((L, 5)), np.zeros((L, 2))
    Bu = np.zeros((5, 2))
    Bu[2, 0] = Bu[3, 1] = dt
    for i in range(L):
        du = np.zeros(2)
        if kgain is not None:
            du = du + f(kgain[i]) @ ds
        if wgain is not None and dwt is not None:
            du = du + f(wgain[i]) @ f(np.asarray(dwt))
        if ogain is not None and dtrack is not None:
            du = du + f(ogain[i]) @ f(np.asarray(dtrack)[min(i, Lt - 1)])
        dtraj[i], dctrl[i] = ds, du
        ds = f(plant_A(traj[i], dt, wheelbase)) @ ds + Bu @ du
    return dtraj, dctrl


def adjoint(traj, kgain, wgain, ogain, Lt, seed_traj, seed_ctrl, dt, wheelbase, mag=False):
    """one ego: (grad_init [5], grad_wt [7], grad_track [Lt,3])"""
    f = np.abs if mag else (lambda a: a)
    L = traj.shape[0]
    lam, gw, gt = np.zeros(5), np.zeros(7), np.zeros((max(Lt, 1), 3))
    for i in range(L - 1, -1, -1):
        gu = dt * lam[2:4] + (0.0 if seed_ctrl is None else f(seed_ctrl[i]))
        if wgain is not None:
            gw = gw + f(wgain[i]).T @ gu
        if ogain is not None:
            gt[min(i, Lt - 1)] += f(ogain[i]).T @ gu
        lam = f(plant_A(traj[i], dt, wheelbase)).T @ lam + (0.0 if seed_traj is None else f(seed_traj[i]))
        if kgain is not None:
            lam = lam + f(kgain[i]).T @ gu
    return lam, gw, gt[:Lt]


# ---- directions and central differences of the oracle loop ---------------------------------------------------------------------------------------
def directions(scene):
    """the unit directions of a scene: 5 of the initial state, 7 of the weights, and with a track 3 of the pose (every row of the track shifted
    alike): list of (name, dinit [5], dwt [7], dtrack [L,3] | None)"""
    out = []
    for q in range(N_STATE):
        out.append((f"s{q}", np.eye(5)[q], np.zeros(7), None))
    for q in range(N_WT):
        out.append((f"w{q}", np.zeros(5), np.eye(7)[q], None))
    if scene.lateral is not None:
        for q in range(N_POSE):
            out.append((f"o{q}", np.zeros(5), np.zeros(7), np.tile(np.eye(3)[q], (scene.L, 1))))
    return out


def fd_direction(scene, d):
    """central difference of (traj | ctrl) [L,7] of the oracle loop along direction d, step FD_REL relative to the entry moved"""
    _, dinit, dwt, dtrack = d
    init, wt, track = np.array(scene.init, dtype=np.float64), sens_weights_ref.weights_of(scene.cfg), scene.track()
    if dinit.any():
        h = FD_REL * max(1.0, abs(float(init @ dinit)))
    elif dwt.any():
        h = FD_REL * float(wt @ dwt)
    else:
        h = FD_REL * max(1.0, float(np.abs(track * dtrack).max()))
    runs = []
    for sg in (1.0, -1.0):
        r = run_scene(scene, init + sg * h * dinit, wt + sg * h * dwt, None if track is None else track + sg * h * (0.0 if dtrack is None else dtrack))
        assert np.all(r["status"] == 1)
        runs.append(np.concatenate([r["traj"], r["ctrl"]], axis=1))
    return (runs[0] - runs[1]) / (2 * h)


def ref_direction(scene, run, gains, d):
    _, dinit, dwt, dtrack = d
    cfg = scene.cfg
    dtraj, dctrl = tangent(run["traj"], gains["kgain"], gains["wgain"], gains["ogain"], scene.L, dinit, dwt, dtrack, cfg.dt, cfg.wheelbase)
    return np.concatenate([dtraj, dctrl], axis=1)


@functools.lru_cache(maxsize=None)
def reference(kind, index):
    """the oracle loop of scene `index` of LF_SCENES / OB_SCENES and its gains, computed once: (scene, run, gains); read-only"""
    scene = scenes_of(kind)[index]
    run = run_scene(scene)
    gains = loop_gains(scene, run)
    for dct in (run, gains):
        for v in dct.values():
            if v is not None:
                v.setflags(write=False)
    return scene, run, gains


# ---- the comparisons the CPU harness and the GPU share -----------------------------------------------------------------------------------------
def gain_errors(scenes, kind, got):
    """worst error of every family's gains over the steps of every scene that are strictly complementary (sens_ref's weak flag), in the measure
    of the family's single-solve test: p and obstacle max|delta| / max(1, max|want|) per step, weights max|delta| / max|want| over the rollout"""
    worst, n_weak = dict(k=0.0, w=0.0, o=0.0), 0
    n_ref = len(scenes_of(kind))
    for b in range(len(scenes)):
        _, _, g = reference(kind, b % n_ref)
        ok = ~g["weak"]
        n_weak += int(g["weak"].sum())
        for i in np.flatnonzero(ok):
            worst["k"] = max(worst["k"], np.abs(got["kgain"][b, i] - g["kgain"][i]).max() / max(1.0, np.abs(g["kgain"][i]).max()))
            if g["ogain"] is not None:
                worst["o"] = max(worst["o"], np.abs(got["ogain"][b, i] - g["ogain"][i]).max() / max(1.0, np.abs(g["ogain"][i]).max()))
        worst["w"] = max(worst["w"], np.abs(got["wgain"][b, ok] - g["wgain"][ok]).max() / np.abs(g["wgain"]).max())
    return worst, n_weak


def tangent_errors(scenes, kind, sweep):
    """worst max|delta| / max|reference| over the directions of every scene: `sweep(b, dinit, dwt, dtrack) -> (dtraj, dctrl)` on the gains under
    test against the reference's tangent"""
    worst = 0.0
    for b, scene in enumerate(scenes):
        _, run, g = reference(kind, b)
        for d in directions(scene):
            want = ref_direction(scene, run, g, d)
            if np.abs(want).max() < FD_FLOOR:
                continue
            dtraj, dctrl = sweep(b, *d[1:])
            worst = max(worst, rel_err(np.concatenate([dtraj, dctrl], axis=1), want))
    return worst


def rel_err(got, want):
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
