"""Shared by tests/test_loop_obstacles_cpu.py and tests/test_gpu_loop_obstacles.py (TEST INFRASTRUCTURE): the scenes of a closed loop past a
moving obstacle, the reference loop around them -- the host mirror of CasadiOptimizer.optimize with one solve per step that sees the step's
obstacle, on the C oracle or on any backend with solve(x0, p, obst) --, and numpy restatements of the circle centres and the clearance."""
import functools

import numpy as np

from helpers import WEIGHTS_YAML_ZAM_LF, WEIGHTS_ZAM_CA, NLPConfig, OracleBackend, make_configuration, pkg, straight_path
from oracle.nlp_numpy import approximating_circle_radius, circle_centers

opt = __import__("importlib").import_module(pkg.__name__ + ".optimizer")

N, L, V_EGO, DT = 10, 40, 10.0, 0.1
OBST_LW = (6.0, 3.5)
AHEAD = 25.0
LATERAL = (-3.3, -3.1, -2.9, 2.9, 3.2)
SPEED = (2.0, 4.0)
SCENES = [(lat, v) for v in SPEED for lat in LATERAL]                 # the ten scenes, in batch order
OFFSET = approximating_circle_radius(*OBST_LW)[1] / 4                  # front / rear circle centres along the heading


def cfg_for(pose):
    """the NLP of one solve: the obstacle at `pose` (x, y, heading)"""
    return NLPConfig(N=N, nx=5, obstacle=(pose[0], pose[1], OBST_LW[0], OBST_LW[1], pose[2]), **WEIGHTS_ZAM_CA)


CFG = cfg_for((AHEAD, LATERAL[0], 0.0))                                # (weights, radii, ego circles: the same in every scene)


def track_of(scene, moving=True):
    """[L, 3] poses of the scene's obstacle at the loop steps; moving=False: held at its start pose"""
    lat, v = scene
    k = np.arange(L) if moving else np.zeros(L)
    return np.stack([AHEAD + v * DT * k, np.full(L, lat), np.zeros(L)], axis=1)


def loop_inputs():
    """init_state [B,5], path [B,L,2], orient [B,L], vdes [B] of the ten scenes"""
    B = len(SCENES)
    path, orient = straight_path(L, 0.0, 0.0, 0.0, V_EGO)
    return np.tile([0.0, 0.0, 0.0, V_EGO, 0.0], (B, 1)), np.tile(path, (B, 1, 1)), np.tile(orient, (B, 1)), np.full(B, V_EGO)


def centres_numpy(track):
    """[..., 3] poses -> [..., 6] circle centres (oracle.nlp_numpy.circle_centers, configuration.py:69-93)"""
    t = np.asarray(track, dtype=np.float64)
    out = np.empty(t.shape[:-1] + (6,))
    for idx in np.ndindex(*t.shape[:-1]):
        out[idx] = circle_centers(t[idx][0], t[idx][1], OBST_LW[0], OBST_LW[1], t[idx][2]).ravel()
    return out


def clearance_numpy(states, c6, ego_offset, r_sum):
    """min over the three constrained pairs (ego circle j, obstacle circle j) of distance - r_sum; states [..., 5], c6 [..., 6]"""
    s, c = np.asarray(states, dtype=np.float64), np.asarray(c6, dtype=np.float64)
    d = []
    for j, sg in enumerate((0.0, 1.0, -1.0)):
        ex = s[..., 0] + sg * ego_offset * np.cos(s[..., 4])
        ey = s[..., 1] + sg * ego_offset * np.sin(s[..., 4])
        d.append(np.hypot(ex - c[..., 2 * j], ey - c[..., 2 * j + 1]))
    return np.min(d, axis=0) - r_sum


class OracleObstBackend(OracleBackend):
    """TEST ONLY: the C oracle with this solve's obstacle centres; keeps the status and iteration count of every solve"""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.log = []

    def solve(self, x0, p, obst=None):
        if obst is not None:
            for i, v in enumerate(np.asarray(obst, dtype=np.float64).ravel()[:6]):
                self._o.desc.obst[i] = v
        r = super().solve(x0, p)
        self.log.append((int(r.status[0]), int(r.iters[0])))
        return r


def host_loop(backend, track):
    """CasadiOptimizer's step-by-step host loop for one ego of the scenes with `backend` behind `sol(...)`: (states [L,5], controls [L,2])"""
    path, orient = straight_path(L, 0.0, 0.0, 0.0, V_EGO)
    conf = make_configuration(path, orient, V_EGO, WEIGHTS_YAML_ZAM_LF, use_case="collision_avoidance",
                              obstacle=dict(position_x=track[0, 0], position_y=track[0, 1], length=OBST_LW[0], width=OBST_LW[1], orientation=track[0, 2]))
    conf.obstacle_track = track
    o = opt.CasadiOptimizer(configuration=conf, init_values=(np.array([0.0, 0.0]), V_EGO, 0.0, 0.0), predict_horizon=N)
    o.use_device_loop = False
    o._sol = opt.NlpSolverHandle(backend)              # (the weights of the solves are the backend's: WEIGHTS_ZAM_CA)
    states, controls, _ = o.optimize()
    return states, controls


@functools.lru_cache(maxsize=None)
def oracle_loops(moving):
    """the ten scenes on the C oracle: dict(traj [10,L,5], ctrl [10,L,2], status [10,L], iters [10,L], clearance [10,L])"""
    out = dict(traj=[], ctrl=[], status=[], iters=[], clearance=[])
    for scene in SCENES:
        track = track_of(scene, moving)
        be = OracleObstBackend(CFG)
        x, u = host_loop(be, track)
        out["traj"].append(x)
        out["ctrl"].append(u)
        out["status"].append([s for s, _ in be.log])
        out["iters"].append([i for _, i in be.log])
        out["clearance"].append(clearance_numpy(x, centres_numpy(track), CFG.ego_offset, CFG.r_sum))
    res = {k: np.array(v) for k, v in out.items()}
    for v in res.values():
        v.setflags(write=False)
    return res
