"""Points of `mpc_problem_desc` away from its defaults, with the inputs that make each changed field matter -- a plain module, no tests in it.

Every other GPU test builds its handle at dt = 0.1, wheelbase = 2.5789128, friction_div = 2.578, ego_offset = 0.75, tol = 1e-8, obst_mult = 3.
The points below move those six; tests/test_descriptor_cpu.py asserts from the oracle alone that each point moves the optimum (a point that
does not would not notice a kernel that ignores the field), tests/test_gpu_descriptor.py holds every kernel path to the oracle at them.

  point  inputs                      N, nx   fields changed
  D1     lane following              10, 5   dt = 0.05
  D2     lane following              10, 6   dt = 0.2
  D3     lane following              10, 5   wheelbase = 3.4
  D4     steered, v in (15, 25)      10, 5   friction_div = 4.0
  D5     steered, v in (12, 22)      12, 5   dt = 0.16, wheelbase = 3.1, friction_div = 3.3
  D6     collision avoidance         30, 5   ego 3.6 x 1.5 m: ego_offset = 0.6, r_sum = 3.1
  D30    D5's scalars                30, 6   (the pipeline tests)

Lane following: synthetic_batch.  Steered: synthetic_batch with the steering angle +-U(0.02, 0.08) in every stage of the guess and in X_ref[0]
-- every synthetic family starts at delta_0 = 0, where tan(delta_0) = 0 and the stage-0 friction row does not see friction_div at all.
Collision avoidance: ca_batch (helpers.py).  tol in {1e-6, 1e-10} is crossed with D1 and D5, obst_mult in {1, 2} with D5 and D6."""
import functools
from dataclasses import dataclass, field, replace

import numpy as np

from helpers import CA_CFG, ca_batch
from oracle.binding import OracleSolver
from oracle.nlp_numpy import WEIGHTS_ZAM_LF, NLPConfig, synthetic_batch

D5_SCALARS = dict(dt=0.16, wheelbase=3.1, friction_div=3.3)
STEER_SEED = 7700001


def steered_batch(cfg, B, start=0, v_range=(12.0, 22.0)):
    """synthetic_batch whose start state (every stage of the guess, X_ref[0]) has the steering angle +-U(0.02, 0.08); instance start + b is the
    same whatever the batch around it"""
    x0, p = synthetic_batch(cfg, B, start=start, v_range=v_range)
    N, nx = cfg.N, cfg.nx
    for b in range(B):
        rng = np.random.default_rng(STEER_SEED + start + b)
        delta = rng.choice([-1.0, 1.0]) * rng.uniform(0.02, 0.08)
        x0[b, 2 * N + 2:: nx] = delta
        p[b, 2 * N + 2] = delta
    return x0, p


@dataclass(frozen=True)
class Point:
    name: str
    kind: str                                   # "lane" | "steered" | "ca"
    cfg: NLPConfig = field(compare=False)
    changed: tuple = field(compare=False)       # names of the NLPConfig fields that differ from the default descriptor
    kw: tuple = field(default=(), compare=False)

    @property
    def cfg_default(self):
        """the point's cfg with the changed fields back at their defaults"""
        d = NLPConfig()
        return replace(self.cfg, **{k: getattr(d, k) for k in self.changed})

    def inputs(self, B, start=0):
        """(x0, p) of instances start .. start + B - 1, generated for the point's own cfg (its dt, its horizon)"""
        if self.kind == "ca":
            return ca_batch(self.cfg, B, start=start)
        if self.kind == "steered":
            return steered_batch(self.cfg, B, start=start, **dict(self.kw))
        return synthetic_batch(self.cfg, B, start=start, **dict(self.kw))

    def at(self, N, nx=None, **kw):
        """the point's scalars and inputs at another horizon / state count (kw: other arguments for the input generator)"""
        return replace(self, name=f"{self.name}_n{N}_nx{nx or self.cfg.nx}" + "".join(f"_{k}{v}" for k, v in sorted(kw.items())),
                       cfg=replace(self.cfg, N=N, nx=nx or self.cfg.nx), kw=tuple({**dict(self.kw), **kw}.items()))


def _lane(N, nx, **fields):
    return NLPConfig(N=N, nx=nx, **WEIGHTS_ZAM_LF, **fields)


D6_CFG = replace(CA_CFG, ego_length=3.6, ego_width=1.5)
POINTS = {
    "D1": Point("D1", "lane", _lane(10, 5, dt=0.05), ("dt",)),
    "D2": Point("D2", "lane", _lane(10, 6, dt=0.2), ("dt",)),
    "D3": Point("D3", "lane", _lane(10, 5, wheelbase=3.4), ("wheelbase",)),
    "D4": Point("D4", "steered", _lane(10, 5, friction_div=4.0), ("friction_div",), (("v_range", (15.0, 25.0)),)),
    "D5": Point("D5", "steered", _lane(12, 5, **D5_SCALARS), tuple(D5_SCALARS), (("v_range", (12.0, 22.0)),)),
    "D6": Point("D6", "ca", D6_CFG, ("ego_length", "ego_width")),
}
POINTS["D30"] = replace(POINTS["D5"], name="D30", cfg=_lane(30, 6, **D5_SCALARS))
assert D6_CFG.ego_offset == 0.6 and abs(D6_CFG.r_sum - 3.1) < 1e-15

# (point, tol, obst_mult): the six points, tol crossed with D1 and D5, obst_mult with D5 and D6
CASES = [(n, 1e-8, 3) for n in ("D1", "D2", "D3", "D4", "D5", "D6")] + [(n, t, 3) for n in ("D1", "D5") for t in (1e-6, 1e-10)] + \
        [(n, 1e-8, m) for n in ("D5", "D6") for m in (1, 2)]
GUARD_B = {"D1": 32, "D2": 32, "D3": 32, "D4": 32, "D5": 32, "D6": 64, "D30": 32, "N64": 66}
# D5's scalars on the horizons where the kernels change shape.  N = 64 (the 512-thread kernels): at v in (12, 22) the oracle itself leaves 3 of
# 66 rows of the 10 s horizon at the iteration limit; at v in (6, 12), the speeds tests/test_gpu_solve_stages.py uses there, all 66 converge
SHORT_HORIZONS = (1, 2, 3, 31, 32)
# the second handle of the two-handle test: D5's horizon and weights at the default descriptor (lane-following inputs: steered ones leave rows
# unconverged at friction_div = 2.578, the kink of the friction row)
D5_AT_DEFAULTS = Point("D5_at_the_defaults", "lane", POINTS["D5"].cfg_default, ())
N64 = POINTS["D5"].at(64, v_range=(6.0, 12.0))
# D30 batches of the pipeline tests: name -> (B, first instance).  The oracle stalls on instances 173, 851, 962, 1169, 1591 of D30's first 2112;
# none is among the evenly spaced rows compared (every 17th of 0 .. 1087, every 37th of 1 .. 2305), and the abandoned launch takes 200 .. 399
D30_BATCHES = {"pipeline": (1088, 0), "hybrid": (2305, 1), "abort": (200, 200)}
# collision-avoidance rows that stall from their cold start at D6's ego (oracle and emulated solve alike; none of instances 0 .. 255 does, and
# instance 94, which stalls at the default ego, converges): the batch of the second-chance test is instances 256 .. 511
D6_STALL_START, D6_STALLED = 256, (311, 371, 420, 502, 503)


def step64(B):
    """stride that leaves at most 64 evenly spaced rows of B"""
    return -(-B // 64)


def assert_ca_rule(cfg, x, status, kkt, p, ro, tol=1e-8):
    """the rule of test_collision_avoidance_batch (tests/test_gpu_parity.py) for rows x against the oracle's rows ro of the same instances:
    the family is nonconvex (pass left / right), so two correct solvers may end in different optima -- at least 85 % of the rows converged on
    both sides agree within 1e-6, and every other row is a KKT point of the numpy NLP of ITS cfg (ego_offset, r_sum) by the certificate of
    helpers.py at 1e-6 / 1e-6"""
    from helpers import kkt_certificate
    from oracle.nlp_numpy import BicycleNLP
    both = (status == 1) & (ro["status"] == 1)
    dist = np.abs(x - ro["x"]).max(axis=1)
    same = both & (dist < 1e-6)
    print(f"converged on both {int(both.sum())} of {len(status)}, same optimum {int(same.sum())}, worst distance among them {dist[same].max():.2e}")
    assert same.sum() >= 0.85 * both.sum() and both.sum() >= 0.85 * len(status)
    assert kkt[status == 1].max() <= tol
    nlp = BicycleNLP(cfg)
    for b in np.flatnonzero(~same):
        assert status[b] == 1, b
        cert = kkt_certificate(nlp, x[b], p[b])
        assert cert["stationarity"] <= 1e-6 and cert["feasibility"] <= 1e-6, (b, cert)


def case_id(c):
    return f"{c[0]}-tol{c[1]:g}-m{c[2]}"


@functools.lru_cache(maxsize=None)
def _oracle(point, B, start, step, tol, obst_mult, default):
    x0, p = point.inputs(B, start)
    r = OracleSolver(point.cfg_default if default else point.cfg, tol=tol, obst_mult=obst_mult).solve_batch(x0[::step], p[::step], nthreads=8)
    for a in r.values():
        a.setflags(write=False)
    return r


def oracle_rows(point, B, start=0, step=1, tol=1e-8, obst_mult=3, default=False):
    """the C oracle on rows 0, step, 2 step .. of point.inputs(B, start): dict(x, status, iters, kkt), computed once per session and read-only.
    default=True: the same inputs solved with the point's changed fields at their defaults (the guard of tests/test_descriptor_cpu.py)"""
    return _oracle(point, int(B), int(start), int(step), float(tol), int(obst_mult), bool(default))


# ---- the closed loop (mpc_closed_loop_batch_ex) at dt = 0.05, wheelbase = 3.1 -----------------------------------------------------------------
LOOP_CFG = _lane(10, 5, dt=0.05, wheelbase=3.1)
LOOP_L, LOOP_B = 24, 65


def loop_inputs(cfg=LOOP_CFG, B=LOOP_B, L=LOOP_L, seed=11):
    """init [B,5], path [B,L,2], orient [B,L], vdes [B]: egos beside an arc of their own (lateral offset, heading error, speed error), path points
    vdes dt apart"""
    rng = np.random.default_rng(seed)
    vdes = np.full(B, 10.0)
    curv = rng.uniform(-0.02, 0.02, B)
    th = curv[:, None] * vdes[:, None] * cfg.dt * np.arange(L)[None, :]
    path = np.cumsum(vdes[:, None, None] * cfg.dt * np.stack([np.cos(th), np.sin(th)], axis=2), axis=1)
    init = np.stack([np.zeros(B), rng.uniform(-1.5, 1.5, B), np.zeros(B), rng.uniform(7.0, 12.0, B), rng.uniform(-0.1, 0.1, B)], axis=1)
    return init, np.ascontiguousarray(path), np.ascontiguousarray(th), vdes


def host_loop(solve, plant, cfg, init, path, orient, vdes, L):
    """the closed loop of B egos as numpy bookkeeping (csrc/mpc_closed_loop.h: loop_setup_instance, loop_advance_instance, loop_write_reference;
    tests/loop_lin_ref.py: oracle_loop, for a batch) around solve(x0, p) -> (x [B,n_w], status [B]) and plant(x [B,5], u [B,2]) -> x_next:
    (traj [B,L,5], ctrl [B,L,2], status [B,L])"""
    N, nx, nw = cfg.N, cfg.nx, cfg.n_w
    assert nx == 5
    B = init.shape[0]
    cur = np.array(init, dtype=np.float64)
    x0, p = np.zeros((B, nw)), np.zeros((B, nw))
    p[:, 2 * N:] = np.tile(cur, (1, N + 1))
    x0[:, 2 * N:] = np.repeat(cur, N + 1, axis=1)           # (the transposed tile the reference really produces at step 0)
    traj, ctrl, status = np.zeros((B, L, 5)), np.zeros((B, L, 2)), np.zeros((B, L), np.int32)
    for i in range(L):
        w, st = solve(x0, p)
        traj[:, i], ctrl[:, i], status[:, i] = cur, w[:, :2], st
        cur = plant(cur, np.ascontiguousarray(w[:, :2]))
        U, X = w[:, :2 * N].reshape(B, N, 2), w[:, 2 * N:].reshape(B, N + 1, nx)
        src = np.minimum(np.arange(N) + 1, N - 1)
        x0 = np.ascontiguousarray(np.concatenate([U[:, src, 0], U[:, src, 1], X[:, np.minimum(np.arange(N + 1) + 1, N)].reshape(B, -1)], axis=1))
        p = np.zeros((B, nw))
        p[:, 2 * N: 2 * N + nx] = cur
        for k in range(N):
            idx = i + k + 1 - ((i - (L - N) + 1) if i >= L - N else 0)
            p[:, 2 * N + nx * (k + 1): 2 * N + nx * (k + 2)] = np.stack([path[:, idx, 0], path[:, idx, 1], np.zeros(B), vdes, orient[:, idx]], axis=1)
    return traj, ctrl, status


@functools.lru_cache(maxsize=None)
def oracle_loop():
    """host_loop of loop_inputs() over the C oracle's solve and its Euler plant step: computed once, read-only"""
    o = OracleSolver(LOOP_CFG)

    def solve(x0, p):
        r = o.solve_batch(x0, p, nthreads=8)
        return r["x"], r["status"]

    out = host_loop(solve, lambda x, u: np.array([o.plant_step(a, b) for a, b in zip(x, u)]), LOOP_CFG, *loop_inputs(), LOOP_L)
    for a in out:
        a.setflags(write=False)
    return out


# ---- FP: the FORCES point -----------------------------------------------------------------------------------------------------------------
FP = dict(dt=0.08, wheelbase=3.1, friction_div=3.3, ego_offset=0.6)
FP_WEIGHTS = dict(Q=(3.0, 1.5, 40.0, 0.3, 8.0), R=(1.2, 0.5), P=(5.0, 6.0, 80.0, 0.4, 12.0))
FP_LOOP_N, FP_LOOP_L, FP_LOOP_B = 10, 12, 33


def fp_loop_inputs(shift=7.0):
    """(init, path, orient, vdes, track) of floop_ref.overtake_family at FP's dt, every obstacle `shift` metres nearer: the linearised circle rows
    bind within the first FP_LOOP_L steps.  Measured on the emulated solver (tests/floop_ref.py: emu_solver): 30 of the 33 egos keep exitflag 1
    throughout, and ego_offset = 0.75 in place of 0.6 moves every one of their trajectories by 0.02 .. 0.03 (8 m nearer: 19 clean, 9 m: 10)"""
    import floop_ref
    init, path, orient, vdes, track = floop_ref.overtake_family(FP_LOOP_B, FP_LOOP_N, dt=FP["dt"])
    track = track.copy()
    track[:, :, 0] -= shift
    return init, path, orient, vdes, np.ascontiguousarray(track)


# ---- derivatives of the optimum at D5 / D6: p (mpc_solve_batch_sens), weights, bounds, obstacle centres (mpc_sens_*) -----------------------------
# Rows compared: SENS_ROWS of the point's first SENS_B instances, on the CPU harness and on the GPU alike.  The figures the bounds are made of stand
# in the reference modules (DESC_HARNESS_WORST / DESC_TOL of tests/sens_ref.py, sens_weights_ref.py, sens_bounds_ref.py, sens_obst_ref.py).
SENS_B, SENS_ROWS = 64, slice(0, 64, 4)
SENS_FAMILIES = ("p", "weights", "bounds", "obst")
SENS_OUTLIER = {"D5": (12,), "D6": ()}         # instances held to the "outlier" bound of the reference modules, every other row to "rest"


def _sens_ref(fam):
    import importlib
    return importlib.import_module({"p": "sens_ref", "weights": "sens_weights_ref", "bounds": "sens_bounds_ref", "obst": "sens_obst_ref"}[fam])


def sens_seeds(cfg, B, seed=1, n_rand=2):
    """directions dp [B, n_rand + nx, n_w]: random ones and the nx unit seeds of xref_0 (tests/test_sensitivities_cpu.py: seeds_for)"""
    rng = np.random.default_rng(seed)
    dps = np.zeros((B, n_rand + cfg.nx, cfg.n_w))
    dps[:, :n_rand] = rng.normal(size=(B, n_rand, cfg.n_w))
    for i in range(cfg.nx):
        dps[:, n_rand + i, cfg.nu * cfg.N + i] = 1.0
    return dps


def sens_directions(fam, cfg, B):
    """the directions of the family's own CPU test, [B, n_dir, n]: p -- two random and the nx unit seeds of xref_0; weights -- the seven
    log-directions and a random relative one; bounds -- the nine level directions and a random one; obst -- the six unit directions and a random one"""
    if fam == "p":
        return sens_seeds(cfg, B)
    if fam == "weights":
        wref = _sens_ref(fam)
        wt = wref.weights_of(cfg)
        d = np.zeros((B, 8, wref.N_WT))
        d[:, :7] = np.diag(wt)
        d[:, 7] = wt * np.random.default_rng(41).normal(size=(B, wref.N_WT))
        return d
    if fam == "bounds":
        bref = _sens_ref(fam)
        d = np.zeros((B, 10, bref.n_b(cfg)))
        d[:, :9] = bref.level_directions(cfg)
        d[:, 9] = np.random.default_rng(61).uniform(-1.0, 1.0, size=(B, bref.n_b(cfg)))
        return d
    d = np.zeros((B, 7, 6))
    d[:, :6] = np.eye(6)
    d[:, 6] = np.random.default_rng(21).normal(size=(B, 6))
    return d


def sens_obst_rows(cfg, B):
    """the descriptor's centres shifted by a few decimetres per instance (tests/test_sens_obst_cpu.py: obst_rows)"""
    c0 = cfg.obstacle_centers.ravel()
    sh = np.array([[0.15 * (b % 4) - 0.2, 0.1 * ((b * 3) % 5) - 0.2] for b in range(B)])
    return np.ascontiguousarray(c0[None, :] + np.tile(sh, (1, 3)))


def sens_row_errors(fam, cfg, x, p, lam_g, lam_x, dw, dirs, rows, obst=None):
    """{row: error of dw[row] against the family's numpy reference, in the measure of the family's own tests; None where the reference flags the
    row weakly active}"""
    ref = _sens_ref(fam)
    out = {}
    for b in rows:
        S, weak = ref.sensitivity_matrix(cfg, obst[b], x[b], p[b], lam_g[b], lam_x[b]) if fam == "obst" else ref.sensitivity_matrix(cfg, x[b], p[b], lam_g[b], lam_x[b])
        if weak:
            out[b] = None
            continue
        d = np.where(np.isfinite(ref.bounds_vector(cfg)), dirs[b], 0.0) if fam == "bounds" else dirs[b]      # (an absent bound's entry is not read)
        want = np.einsum("ij,dj->di", S, d)
        if fam in ("p", "obst"):
            out[b] = float(np.max(np.abs(dw[b] - want)) / max(1.0, np.max(np.abs(want))))
        elif fam == "weights":
            out[b] = max(float(np.max(np.abs(dw[b, q] - want[q])) / np.max(np.abs(want[q]))) for q in range(d.shape[0]))
        else:
            out[b] = max(float(np.max(np.abs(dw[b, q] - want[q])) / max(np.max(np.abs(want[q])), 0.1)) for q in range(d.shape[0]))
    return out


def sens_split(fam, name, errs, instances):
    """(worst error over the rows held to the "rest" bound, over the "outlier" rows, rows compared) of {row: error}; instances[row] is the
    instance number of a row; the rows the family's reference module leaves out and the weakly active ones are dropped"""
    ref = _sens_ref(fam)
    left_out = getattr(ref, "DESC_LEFT_OUT", {}).get(name, ())
    outliers = SENS_OUTLIER[name] if "outlier" in ref.DESC_TOL[name] else ()          # (a family without an outlier bound holds every row to "rest")
    rest = [e for b, e in errs.items() if e is not None and instances[b] not in outliers and instances[b] not in left_out]
    outl = [e for b, e in errs.items() if e is not None and instances[b] in outliers and instances[b] not in left_out]
    return max(rest, default=0.0), max(outl, default=0.0), len(rest) + len(outl)


def assert_sens(fam, name, errs, instances, harness=False):
    """the rows against the bounds of the family's reference module (harness=True: against 1.02 x the recorded figures themselves)"""
    ref = _sens_ref(fam)
    rest, outl, n = sens_split(fam, name, errs, instances)
    bound = {k: 1.02 * v for k, v in ref.DESC_HARNESS_WORST[name].items()} if harness else ref.DESC_TOL[name]
    print(f"{name} {fam}: worst {rest:.3e} (bound {bound['rest']:.2e})" + (f", instance {SENS_OUTLIER[name]}: {outl:.3e} (bound {bound['outlier']:.2e})" if "outlier" in bound else "")
          + f" over {n} rows")
    assert n >= len(errs) // 2
    assert rest <= bound["rest"] and outl <= bound.get("outlier", 0.0)


_sensx = None


def sens_harness(fam, cfg, x0, p, dirs, seeds, obst=None):
    """the family's CPU harness (tests/sensx.cpp behind the emulated solve): dict(x, status, lam_g, lam_x, dw, ok, ...)"""
    import ctypes as C
    from helpers import abi, harness_lib
    global _sensx
    if _sensx is None:
        L = C.CDLL(harness_lib("sensx"))
        dp, ip, i32, desc = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_int32, C.POINTER(abi.MpcProblemDesc)
        L.sensx_solve.argtypes = [desc, dp, dp, dp, dp, i32, i32, dp, dp, dp, ip, dp, dp, dp, i32, dp, dp, dp, dp, ip]
        L.sensweightx_solve.argtypes = L.sensboundx_solve.argtypes = [desc, dp, dp, dp, dp, i32, dp, dp, dp, ip, dp, dp, i32, dp, dp, dp, dp, dp, ip, ip]
        L.sensobstx_solve.argtypes = [desc, dp, dp, dp, dp, i32, dp, dp, dp, dp, ip, dp, dp, i32, dp, dp, dp, dp, dp, ip, ip]
        _sensx = L
    if fam == "p":
        import test_sensitivities_cpu as T
        return T.run_sensx(_sensx, cfg, x0, p, dirs, seeds)
    if fam == "weights":
        import test_sens_weights_cpu as T
        return T.run_sensweightx(_sensx, cfg, x0, p, dirs, seeds)
    if fam == "bounds":
        import test_sens_bounds_cpu as T
        return T.run_sensboundx(_sensx, cfg, x0, p, dirs, seeds)
    import test_sens_obst_cpu as T
    return T.run_sensobstx(_sensx, cfg, x0, p, obst, dirs, seeds)


# ---- the predicted loop (mpc_closed_loop_batch_pred) with another ego --------------------------------------------------------------------------
PRED_N, PRED_L, PRED_B = 10, 16, 16


def pred_loop_inputs():
    """(cfg, init [B,5], path [B,L,2], orient [B,L], vdes [B], track [B,L+N,3], obst_offset): the drift scene of tests/pred_obst_ref.py as a loop --
    an ego of 3.6 x 1.5 m (ego_offset 0.6, r_sum 3.1) on a straight path along x at 6 .. 12 m/s, a 6 x 3.5 m vehicle beside it at its speed that
    drifts towards the lane, from 0.5 m clear to 0.3 m inside over the track"""
    import pred_obst_ref
    cfg = replace(pred_obst_ref.cfg_for(PRED_N), ego_length=3.6, ego_width=1.5)
    rng = np.random.default_rng(31)
    B, L, Lt = PRED_B, PRED_L, PRED_L + PRED_N
    v = rng.uniform(6.0, 12.0, B)
    side = rng.choice([-1.0, 1.0], B)
    k = np.arange(L)
    path = np.stack([v[:, None] * cfg.dt * (k[None, :] + 1), np.zeros((B, L))], axis=2)
    init = np.stack([np.zeros(B), np.zeros(B), np.zeros(B), v, np.zeros(B)], axis=1)
    kt = np.arange(Lt)
    y = side[:, None] * (cfg.r_sum + 0.5 - 0.8 * kt[None, :] / (Lt - 1))
    track = np.stack([v[:, None] * cfg.dt * kt[None, :], y, np.zeros((B, Lt))], axis=2)
    return cfg, init, np.ascontiguousarray(path), np.zeros((B, L)), v, np.ascontiguousarray(track), 1.0


# ---- dw/dweights at D5 / D6 (mpc_sens_weights) -------------------------------------------------------------------------------------------------
# tests/sens_weights_ref.py against the CPU harness (tests/sensx: sensweightx_solve) at the point, worst max|dw - want| / max|want| over rows and
# the eight directions of tests/test_sens_weights_cpu.py, measured by tests/test_descriptor_cpu.py::test_weight_sensitivity_harness_against_the_reference
# (reference against harness, no kernel involved) on the same SENS_ROWS; D5's figure is instance 12's again (every other row: 8e-7 and below).
# The cap is the one next to the module's own HARNESS_WORST, 1e-4.
SENS_WT_HARNESS_WORST = {"D5": 1.73e-5, "D6": 3.55e-6}
SENS_WT_TOL = {k: min(10 * v, 1e-4) for k, v in SENS_WT_HARNESS_WORST.items()}


def weight_directions(cfg, B, seed=41):
    """the seven log-directions wt_q e_q and one random relative direction (tests/test_sens_weights_cpu.py: directions): [B, 8, 7]"""
    import sens_weights_ref as wref
    rng = np.random.default_rng(seed)
    wt = wref.weights_of(cfg)
    d = np.zeros((B, 8, wref.N_WT))
    d[:, :7] = np.diag(wt)
    d[:, 7] = wt * rng.normal(size=(B, wref.N_WT))
    return d


def weight_sens_errors(cfg, x, p, lam_g, lam_x, dw, dwt, rows):
    """(worst max|dw - want| / max|want| over rows and directions, rows compared, weakly active rows left out) against tests/sens_weights_ref.py"""
    import sens_weights_ref as wref
    worst, checked, weak = 0.0, 0, 0
    for b in rows:
        S, w_ = wref.sensitivity_matrix(cfg, x[b], p[b], lam_g[b], lam_x[b])
        if w_:
            weak += 1
            continue
        want = np.einsum("ij,dj->di", S, dwt[b])
        for d in range(dwt.shape[1]):
            worst = max(worst, float(np.max(np.abs(dw[b, d] - want[d])) / np.max(np.abs(want[d]))))
        checked += 1
    return worst, checked, weak
