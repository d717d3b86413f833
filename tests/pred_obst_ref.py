"""Shared by tests/test_pred_obst_cpu.py, tests/test_gpu_solve_stages.py and tests/test_gpu_loop_pred.py (TEST INFRASTRUCTURE): the NLP with
obstacle centres per stage as a subclass of the oracle's BicycleNLP, the instance families of the per-stage solve and their reference solutions
by the oracle's dense interior-point method, unchanged, on that subclass."""
import functools
import os

import numpy as np

from helpers import WEIGHTS_ZAM_CA, BicycleNLP, NLPConfig
from oracle.ipm_numpy import DenseIPM
from oracle.nlp_numpy import circle_centers

OBST_LW = (6.0, 3.5)                     # the obstacle rectangle: r_sum 3.3; circle_centers puts the outer two +- 1.0 along the heading
SEEDS = 16
MIN_CONVERGED = 12                       # of SEEDS, per (family, N) a test uses
# the reference's optima of the families that take the dense method minutes (N = 30: 5 s per instance), recorded by
# tests/golden/make_pred_obst_ref.py: <family>_n<N>_nx<nx>__seeds [n], __x_ref [n, n_w]; tests/test_pred_obst_cpu.py checks the record
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pred_obst_ref.npz")


class StagedNLP(BicycleNLP):
    """BicycleNLP with obstacle centres per stage, stages [N+1, 3, 2].  g, jac and hess_lag of the parent call obstacle_rows once per stage, in
    stage order: a counter, reset by each of the three, picks the stage's centres."""

    def __init__(self, cfg, stages):
        super().__init__(cfg)
        self.stages = np.asarray(stages, dtype=np.float64).reshape(cfg.N + 1, 3, 2)
        self._k = 0

    def obstacle_rows(self, x, want_hess=False):
        self.obst = self.stages[self._k]
        self._k += 1
        return super().obstacle_rows(x, want_hess)

    def g(self, w, p):
        self._k = 0
        return super().g(w, p)

    def jac(self, w, p):
        self._k = 0
        return super().jac(w, p)

    def hess_lag(self, w, p, sigma, lam):
        self._k = 0
        return super().hess_lag(w, p, sigma, lam)


def cfg_for(N, nx=5):
    return NLPConfig(N=N, nx=nx, obstacle=(0.0, 0.0, OBST_LW[0], OBST_LW[1], 0.0), **WEIGHTS_ZAM_CA)


def centres(poses):
    """[..., 3] poses (x, y, heading) of the obstacle rectangle -> [..., 3, 2] circle centres"""
    t = np.asarray(poses, dtype=np.float64)
    out = np.empty(t.shape[:-1] + (3, 2))
    for idx in np.ndindex(*t.shape[:-1]):
        out[idx] = circle_centers(t[idx][0], t[idx][1], OBST_LW[0], OBST_LW[1], t[idx][2])
    return out


def clearance(cfg, X, stages):
    """min over the three constrained pairs of distance - r_sum, per stage: X [N+1, >=5] states, stages [N+1, 3, 2]"""
    d = []
    for j, sg in enumerate((0.0, 1.0, -1.0)):
        ex = X[:, 0] + sg * cfg.ego_offset * np.cos(X[:, 4])
        ey = X[:, 1] + sg * cfg.ego_offset * np.sin(X[:, 4])
        d.append(np.hypot(ex - stages[:, j, 0], ey - stages[:, j, 1]))
    return np.min(d, axis=0) - cfg.r_sum


def instance(family, N, seed, nx=5):
    """(x0 [n_w], p [n_w], stages [N+1, 3, 2]) of one instance: the ego on a straight reference along x at 6 .. 12 m/s, the state guess the
    reference rollout.
    lead:   a vehicle in the lane, 2 .. 5 m/s slower; without braking the ego is 0.1 .. 0.3 x 2 ((N - 1) dt)^2 short of the distance at the
            last stage (a constant deceleration of 0.4 .. 1.2 m/s^2 from the first stage that moves the position on makes it up)
    drift:  a vehicle beside the lane at the ego's speed that drifts towards it: 0.5 m clear at stage 0, 0.1 .. 0.4 m inside at the last
    beside: clear by 0.2 .. 0.8 m at every stage, and moving: every stage's centres differ (short horizons, where no control reaches the
            position before stage 2 / 4 and an active row cannot be answered)"""
    cfg = cfg_for(N, nx)
    rng = np.random.default_rng(7000 + 100 * N + seed + {"lead": 0, "drift": 31, "beside": 67}[family] * 1000)
    v, dt = rng.uniform(6.0, 12.0), cfg.dt
    k = np.arange(N + 1)
    Xr = np.zeros((N + 1, nx))
    Xr[:, 0], Xr[:, 3] = v * dt * k, v
    p = np.concatenate([np.zeros(2 * N), Xr.ravel()])
    x0 = p.copy()
    ego = np.array([[0.0, 0.0, 0.0, 0.0, 0.0]])

    def place(target, along, heading=0.0):
        """the obstacle's offset from the ego along `along` (a unit vector) at which its clearance against an ego at the origin is
        `target`: bisection, the clearance grows with the offset beyond the point where the rectangles' circles coincide"""
        lo, hi = 0.5, 20.0
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            c = clearance(cfg, ego, centres([[mid * along[0], mid * along[1], heading]]))[0]
            lo, hi = (mid, hi) if c < target else (lo, mid)
        return 0.5 * (lo + hi)

    if family == "lead":
        dv, short = rng.uniform(2.0, 5.0), rng.uniform(0.1, 0.3) * 2.0 * ((N - 1) * dt) ** 2
        gap_last = place(-short, (1.0, 0.0))
        poses = np.stack([Xr[N, 0] + gap_last - (v - dv) * dt * (N - k), np.zeros(N + 1), np.zeros(N + 1)], axis=1)
    elif family == "drift":
        side, inside = rng.choice([-1.0, 1.0]), rng.uniform(0.1, 0.4)
        y0, y1 = place(0.5, (0.0, 1.0)), place(-inside, (0.0, 1.0))
        poses = np.stack([Xr[:, 0], side * (y0 + (y1 - y0) * k / N), np.zeros(N + 1)], axis=1)
    else:
        side, clear, hd = rng.choice([-1.0, 1.0]), rng.uniform(0.2, 0.8, N + 1), rng.uniform(-0.05, 0.05, N + 1)
        poses = np.stack([Xr[:, 0], side * np.array([place(c, (0.0, 1.0), h) for c, h in zip(clear, hd)]), hd], axis=1)
    return x0, p, centres(poses)


def reference_solve(name, N, seed, nx=5):
    """the oracle's dense interior-point method on the instance: its optimum [n_w], or None where it does not converge"""
    x0, p, st = instance(name, N, seed, nx)
    r = DenseIPM(StagedNLP(cfg_for(N, nx), st)).solve(x0, p)
    return r["x"] if r["status"] == 1 else None


@functools.lru_cache(maxsize=None)
def family(name, N, nx=5, n=SEEDS, recorded=True):
    """the instances of (family, N) on which the reference converges, with its optima: dict(x0 [n, n_w], p, stages [n, N+1, 3, 2], x_ref,
    active [n] (a circle row within 1e-6 of its bound at the optimum), seeds [n], tried = SEEDS); arrays read-only.  recorded: take the
    optima from GOLDEN where it has the family"""
    cfg = cfg_for(N, nx)
    keep = dict(x0=[], p=[], stages=[], x_ref=[], active=[], seeds=[])
    key = f"{name}_n{N}_nx{nx}"
    rec = np.load(GOLDEN) if recorded and n == SEEDS and os.path.exists(GOLDEN) else {}
    have = {int(s_): x for s_, x in zip(rec[key + "__seeds"], rec[key + "__x_ref"])} if key + "__seeds" in rec else None
    for seed in range(n):
        x0, p, st = instance(name, N, seed, nx)
        x = have.get(seed) if have is not None else reference_solve(name, N, seed, nx)
        if x is None:
            continue
        X = x[2 * N:].reshape(N + 1, nx)
        for k_, v in zip(keep, (x0, p, st, x, clearance(cfg, X, st).min() <= 1e-6, seed)):
            keep[k_].append(v)
    out = {key: np.array(v) for key, v in keep.items()}
    for v in out.values():
        v.setflags(write=False)
    out["tried"] = n
    return out


def batch(parts):
    """families interleaved into one batch: parts = [(name, N), ...] of one N -> dict(x0, p, stages [B, N+1, 6], x_ref, fam [B] index into
    parts)"""
    fams = [family(*q) for q in parts]
    rows = sorted((i, f) for f, d in enumerate(fams) for i in range(len(d["x0"])))
    pick = lambda key: np.ascontiguousarray(np.array([fams[f][key][i] for i, f in rows]))      # noqa: E731
    B = len(rows)
    return dict(x0=pick("x0"), p=pick("p"), stages=pick("stages").reshape(B, -1, 6), x_ref=pick("x_ref"), active=pick("active"),
                fam=np.array([f for _, f in rows]))
