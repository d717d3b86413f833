"""Shared by tests/test_loop_traffic_cpu.py and tests/test_gpu_loop_traffic.py (TEST INFRASTRUCTURE): numpy restatement of the selection and the
clearance of the loop through traffic (include/mpcgpu.h, mpc_closed_loop_batch_traffic; csrc/mpc_closed_loop.h, loop_traffic_stage), with the
margin between the best candidate and the runner-up of every choice, and scene S: two obstacles the ego has to pass one after the other, with the
reference loops around it: the numpy host loop over the emulated per-stage solve."""
import functools

import numpy as np

import loop_obst_ref as lref
from helpers import pkg

MARGIN = 1e-9              # metres between the best candidate and the runner-up below which an index is not compared
DESC_OBST = np.array([-100.0, 0.0] * 3)


def centres(rows, offset):
    """[..., 3] poses, offset broadcast against [...] -> [..., 3, 2]: the centre, then +- offset along the heading (loop_obstacle_centres)"""
    rows, offset = np.asarray(rows, dtype=np.float64), np.asarray(offset, dtype=np.float64)
    cs, sn = np.cos(rows[..., 2]), np.sin(rows[..., 2])
    x, y = rows[..., 0], rows[..., 1]
    return np.stack([np.stack([x, y], -1), np.stack([x + offset * cs, y + offset * sn], -1), np.stack([x - offset * cs, y - offset * sn], -1)], -2)


def _as4(tracks, offsets, B):
    """tracks [M,Lt,3] / [B,M,Lt,3], offsets [M] / [B,M] -> [B,M,Lt,3], [B,M]"""
    t, o = np.asarray(tracks, dtype=np.float64), np.asarray(offsets, dtype=np.float64)
    if t.ndim == 3:
        t, o = np.broadcast_to(t, (B,) + t.shape), np.broadcast_to(o, (B,) + o.shape)
    return t, o


def _two_smallest(d):
    """d [..., n] (inf: no candidate) -> (argmin with ties to the lowest index or -1, margin to the runner-up, inf where there is none)"""
    order = np.sort(d, axis=-1)
    best = np.argmin(d, axis=-1)
    none = ~np.isfinite(order[..., 0])
    with np.errstate(invalid="ignore"):                      # (inf - inf where nothing is present: masked below)
        margin = (order[..., 1] - order[..., 0]) if d.shape[-1] > 1 else np.full(best.shape, np.inf)
    return np.where(none, -1, best), np.where(none, np.inf, margin)


def ego_poses(i, state, x0, N, nx):
    """predicted pose (x, y, psi) [B, N+1, 3] of every stage before the solve of step i: the measured state at step 0, else the stages of the warm start"""
    state = np.asarray(state, dtype=np.float64)
    B = state.shape[0]
    if i == 0:
        return np.repeat(state[:, None, [0, 1, 4]], N + 1, axis=1)
    X = np.asarray(x0, dtype=np.float64)[:, 2 * N:].reshape(B, N + 1, nx)
    return X[:, :, [0, 1, 4]]


def distances(poses, tracks, offsets, rows, ego_offset):
    """poses [B,K,3], tracks [B,M,Lt,3], rows [K] -> (D [B,K,M,3 (ego circle j),3 (obstacle circle c)], inf where obstacle m is absent; O [B,K,M,3,2])"""
    E = centres(poses, ego_offset)                                              # [B,K,3,2]
    tr = np.moveaxis(tracks[:, :, rows], 1, 2)                                  # [B,K,M,3]
    O = centres(tr, offsets[:, None, :])                                        # [B,K,M,3,2]
    with np.errstate(invalid="ignore"):
        D = np.hypot(E[:, :, None, :, None, 0] - O[:, :, :, None, :, 0], E[:, :, None, :, None, 1] - O[:, :, :, None, :, 1])
    present = np.isfinite(tr[..., 0])
    return np.where(present[..., None, None], D, np.inf), O


def select(i, poses, tracks, offsets, pairing, ego_offset, desc_obst=DESC_OBST):
    """rows [B,N+1,6], chosen [B,N+1,3], margin [B,N+1,3] of the solve of step i for the predicted ego poses [B,N+1,3]"""
    B, K = poses.shape[:2]
    tracks, offsets = _as4(tracks, offsets, B)
    M, Lt = tracks.shape[1:3]
    rows = np.minimum(i + np.arange(K), Lt - 1)
    D, O = distances(poses, tracks, offsets, rows, ego_offset)
    out = np.tile(np.asarray(desc_obst, dtype=np.float64).reshape(3, 2), (B, K, 1, 1))
    chosen, margin = np.empty((B, K, 3), np.int64), np.empty((B, K, 3))
    bi, ki = np.meshgrid(np.arange(B), np.arange(K), indexing="ij")
    if pairing == 0:
        score = np.min(np.stack([D[..., j, j] for j in range(3)], -1), -1)     # [B,K,M]
        m, mg = _two_smallest(score)
        have = m >= 0
        out[have] = O[bi[have], ki[have], m[have]]
        chosen[:], margin[:] = m[..., None], mg[..., None]
    else:
        for j in range(3):
            m, mg = _two_smallest(D[:, :, :, j, :].reshape(B, K, 3 * M))         # (m-major: ties to the lowest m, then the lowest c)
            have = m >= 0
            out[bi[have], ki[have], j] = O[bi[have], ki[have], m[have] // 3, m[have] % 3]
            chosen[..., j], margin[..., j] = np.where(have, m // 3, -1), mg
    return out.reshape(B, K, 6), chosen, margin


def clearance(i, state, tracks, offsets, ego_offset, r_sum):
    """(clearance [B], nearest [B], margin [B]) of the states [B, >=5] before step i: all nine pairs of every obstacle present at row min(i, Lt - 1)"""
    state = np.asarray(state, dtype=np.float64)
    B = state.shape[0]
    tracks, offsets = _as4(tracks, offsets, B)
    D, _ = distances(state[:, None, [0, 1, 4]], tracks, offsets, np.array([min(i, tracks.shape[2] - 1)]), ego_offset)
    flat = D.reshape(B, -1)
    m, mg = _two_smallest(flat)
    return np.where(m >= 0, flat.min(-1) - r_sum, np.inf), np.where(m >= 0, m // 9, -1), mg


def clearance_of_run(traj, tracks, offsets, ego_offset, r_sum):
    """[B, L] clearance and nearest of a returned trajectory [B, L, 5]"""
    out = [clearance(i, traj[:, i], tracks, offsets, ego_offset, r_sum) for i in range(traj.shape[1])]
    return np.stack([o[0] for o in out], 1), np.stack([o[1] for o in out], 1), np.stack([o[2] for o in out], 1)


# ---- scene S ----------------------------------------------------------------------------------------------------------------------------------
# Two standing obstacles of the size of tests/loop_obst_ref.py on either side of the ego's straight path (its own scenes put one 25 m ahead at the
# lateral offsets -3.3 .. 3.2): A 25 m ahead at -2.9, B 55 m ahead at +2.9.  Each reaches 0.4 m into the ego's circles, so the ego swerves left past
# A and right past B.  N, the ego, the weights and the radii are loop_obst_ref's; its L = 40 steps at 10 m/s end 15 m short of B, so the scene runs
# S_L = 75 steps, which passes both.
N, L = lref.N, lref.L
S_L = 75
POSE_A, POSE_B = (25.0, -2.9, 0.0), (55.0, 2.9, 0.0)
S_TRACKS = np.array([[POSE_A], [POSE_B]])                   # [M = 2, Lt = 1, 3]
S_OFFSETS = np.array([lref.OFFSET, lref.OFFSET])
UNDERCUT = 0.1                                              # a loop that is given one obstacle only drives this far into the other one


def clearance_nine(traj, m):
    """[L] distance - r_sum of a trajectory [L, 5] against obstacle m of scene S, all nine circle pairs"""
    return clearance_of_run(traj[None], S_TRACKS[m:m + 1], S_OFFSETS[m:m + 1], lref.CFG.ego_offset, lref.CFG.r_sum)[0][0]


def clearance_pairs(traj, m):
    """... over the three pairs (j, j) that the reference's NLP constrains"""
    c6 = centres(S_TRACKS[m, 0], S_OFFSETS[m]).reshape(6)
    return lref.clearance_numpy(traj, np.tile(c6, (len(traj), 1)), lref.CFG.ego_offset, lref.CFG.r_sum)


def emu_solve_stages(cfg, x0, p, stages, bounds=None):
    """the kernels' solve stepped on the CPU (tests/emu: EmuSolve) with obstacle centres per stage, stages [B, N+1, 6] (tests/trafx)"""
    import ctypes as C
    from helpers import BicycleNLP, abi, emu_desc, harness_lib
    L = C.CDLL(harness_lib("trafx"))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L.trafx_solve_stages.argtypes = [C.POINTER(abi.MpcProblemDesc), dp, dp, dp, dp, C.c_int32, dp, dp, dp, dp, ip, ip, dp]
    x0, p, stages = (np.ascontiguousarray(a, dtype=np.float64) for a in (x0, p, stages))
    lbg, ubg, lbx, ubx = (np.ascontiguousarray(a, dtype=np.float64) for a in (BicycleNLP(cfg).bounds() if bounds is None else bounds))
    B = x0.shape[0]
    out, st, it, kkt = np.zeros_like(x0), np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B)
    d = emu_desc(cfg)
    rc = L.trafx_solve_stages(C.byref(d), abi.as_dp(lbx), abi.as_dp(ubx), abi.as_dp(lbg), abi.as_dp(ubg), B, abi.as_dp(x0), abi.as_dp(p), abi.as_dp(stages),
                              abi.as_dp(out), abi.as_ip(st), abi.as_ip(it), abi.as_dp(kkt))
    assert rc == 0, rc
    return pkg.SolveResult(out, st, it, kkt)


class EmuStagedBackend:
    """TEST ONLY: solve(x0, p, obst [B, N+1, 6]) by the emulated per-stage solve, under the bounds last given to set_bounds; a solve without `obst`
    (the second chance of solver.rescue_failed, which the library runs on the device) keeps the centres of the solve before it"""

    def __init__(self, cfg):
        self.cfg, self.n_w, self.n_g, self.N = cfg, cfg.n_w, cfg.n_g, cfg.N
        self._bounds, self._stages = None, None

    def set_bounds(self, lbx, ubx, lbg, ubg):
        self._bounds = (lbg, ubg, lbx, ubx)

    def solve(self, x0, p, obst=None):
        if obst is not None:
            self._stages = np.asarray(obst, dtype=np.float64).reshape(-1, self.cfg.N + 1, 6)
        return emu_solve_stages(self.cfg, np.atleast_2d(x0), np.atleast_2d(p), self._stages, self._bounds)


class _LoggingHandle(lref.opt.NlpSolverHandle):
    """keeps the status of every step (after its second chance)"""

    def __call__(self, **kw):
        out = super().__call__(**kw)
        self.steps = getattr(self, "steps", []) + [int(self._stats["status"][0])]
        return out


class _LoggingOptimizer(lref.opt.CasadiOptimizer):
    """keeps the predicted ego poses [N+1, 3] every selection was made from"""

    def traffic_centres(self, step, poses):
        self.poses = getattr(self, "poses", []) + [np.array(poses)]
        return super().traffic_centres(step, poses)


def host_loop(backend, tracks, offsets, pairing, L=S_L, noise_seed=None, device=False):
    """CasadiOptimizer's step-by-step host loop through the obstacles `tracks` [M, Lt, 3] with `backend` behind sol(...) -- device=True: its device
    loop on `backend` instead --: (states [L,5], controls [L,2], chosen [L, N+1, 3], status [L] of every step of the host loop)"""
    from helpers import WEIGHTS_YAML_ZAM_LF, make_configuration, straight_path
    path, orient = straight_path(L, 0.0, 0.0, 0.0, lref.V_EGO)
    first = tracks[0, 0]
    conf = make_configuration(path, orient, lref.V_EGO, WEIGHTS_YAML_ZAM_LF, use_case="collision_avoidance", noised=noise_seed is not None,
                              obstacle=dict(position_x=first[0], position_y=first[1], length=lref.OBST_LW[0], width=lref.OBST_LW[1], orientation=first[2]))
    conf.obstacle_tracks = np.asarray(tracks, dtype=np.float64)
    conf.obstacle_sizes = np.tile(lref.OBST_LW, (len(tracks), 1))
    conf.obstacle_pairing = pairing
    if noise_seed is not None:
        conf.noise_seed = noise_seed
    o = _LoggingOptimizer(configuration=conf, init_values=(np.array([0.0, 0.0]), lref.V_EGO, 0.0, 0.0), predict_horizon=N)
    o.use_device_loop = device                             # (True: the optimizer's device path, BatchedMPCSolver.closed_loop_traffic)
    o._sol = _LoggingHandle(backend)
    states, controls, _ = o.optimize()
    host_loop.poses = np.array(getattr(o, "poses", []))                     # [L, N+1, 3]: what the last loop's selections were made from
    return states, controls, o.chosen, np.array(getattr(o._sol, "steps", []))


@functools.lru_cache(maxsize=None)
def scene_s(which, pairing):
    """the reference loop through scene S given both obstacles ("AB"), A only or B only: dict(traj [L,5], ctrl [L,2], status [L], clearance [2, L] of the
    trajectory against A and against B, all nine pairs), S_L steps"""
    tr = {"AB": S_TRACKS, "A": S_TRACKS[:1], "B": S_TRACKS[1:]}[which]
    be = EmuStagedBackend(lref.CFG)
    x, u, _, status = host_loop(be, tr, S_OFFSETS[:len(tr)], pairing)
    cl = np.stack([clearance_of_run(x[None], S_TRACKS[m:m + 1], S_OFFSETS[m:m + 1], lref.CFG.ego_offset, lref.CFG.r_sum)[0][0] for m in range(2)])
    res = dict(traj=x, ctrl=u, status=status, clearance=cl)
    for v in res.values():
        v.setflags(write=False)
    return res
