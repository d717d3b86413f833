"""Bound structures that mpc_set_bounds accepts and the reference never sets, with the batch each is used with -- a plain module, no tests in it.

Every other GPU test installs the reference's structure (BicycleNLP.bounds(): steering rate, acceleration (upper), steering angle and speed bounded at
every stage, the friction row 0 <= . <= a_max presolved into a cap on a_0, circle rows with a lower bound only).  The points below leave it; the host
turns them into has_fl / has_fu / has_ol / has_ou, lo_mask / hi_mask, dense_mask and dec_s (csrc/mpc_host_common.h: set_bound_rows, set_bounds), on
which the kernels branch.  tests/test_bound_structures_cpu.py asserts from the oracle alone that every point converges and that a binding point
moves the optimum; tests/test_gpu_bound_structures.py holds every kernel path to the oracle at them.

A point edits the reference bounds (lbg, ubg, lbx, ubx) of a family's configuration.  A binding value is a quantile, over the family's first QB
instances, of each instance's extreme over the bounded stages in its optimum under the REFERENCE bounds (the oracle's); "late" stages are k >= N / 2,
which leaves every instance the first half of the horizon to reach the bound.

  point  what it installs                                                          what it switches
  S1     a >= q50 of min_k a, every stage                                          a lo_mask bit (dense)
  S2     v <= q50 of max over the late stages, late stages only                    clears the dense_mask bit of the speed's upper bound
  S3     q10 <= y_N <= q60 of the terminal y (the latest stage: see _s3)            a variable outside REF_BOUND_VM; inputs with heading 0
  S4     lbg[0] = 0.5                                                              has_fl: the friction row stays a row with a slack
  S5     ubg[0] = inf                                                              neither the cap on a_0 nor the row
  S6     circle rows ubg = 1000 (lane following), 60 (collision avoidance)         has_ou: two-sided circle rows, the larger LDS stash
  S7     no bounds on the steering angle, no lower bound on the speed              clears reference bits
  S8     nx = 6: progress state <= 1e4 at every stage                              dec_s = 0 (Q[5] = 0 as ever)
  S9     S1 + S2 + S3 + S4 + S6, S1's floor from the optima under the other four   all of it at once; inputs with heading 0 (see _s9_a)
  S10    S6 at obst_mult = 1 (collision avoidance) / 2 (lane following)            (the descriptor families solve at obst_mult != 3 without has_ou)
  FLOU   collision avoidance: lbg[0] = 0.5, circle rows ubg = 1000                 the case of the CPU sensitivity harness

S1, S4 and S5 leave the compiled-in variant of the kernels on (it looks the acceleration's lower side and the friction flags up at run time), every other
point switches it off (tests/test_bound_structures_cpu.py: test_launch_plan); the GPU tests run those three in both variants.

S3 and S9 use synthetic_batch(..., heading=0.0): at the default's random heading one shared box on y or psi cuts most instances off their
reference path (psi <= q60 from stage 1 on: 58 - 62 % converge).

Collision avoidance, a BINDING upper bound of the circle rows: none is kept.  Stage 0 of every instance is fixed by the initial state, 28 .. 32 m
in front of the obstacle (largest stage-0 circle distance in ca_batch: ~33.7), and the largest distance at the end of the horizon is ~31.8, so a
value that binds anywhere is violated at stage 0 by part of the batch; measured at ubg = 31: see SHARES.

Measured by tests/test_bound_structures_cpu.py from the oracle alone (QB instances; share converged / share of optima moved by > 1e-3 against the
reference-bounds optimum / largest move where the point is inactive): SHARES below.  Measured on the MI355X: GPU_WORST below."""
import functools
from dataclasses import dataclass, field

import numpy as np

from helpers import CA_CFG, FAMILIES, ca_batch
from oracle.binding import OracleSolver
from oracle.nlp_numpy import WEIGHTS_ZAM_LF, BicycleNLP, NLPConfig, synthetic_batch

QB = 64                                         # instances the quantiles are taken over, and the ones the CPU conditions are asserted on
LANE = {
    "n10": (FAMILIES["zamlf_n10_nx5"][0], {}),
    "n30": (FAMILIES["zamlf_n30_nx6"][0], {}),
    "n50": (FAMILIES["usalf_n50_nx5"][0], dict(FAMILIES["usalf_n50_nx5"][1])),       # 4 instances per stage workgroup, one per wavefront in k_solve_wg
    "n64": (NLPConfig(N=64, nx=6, **WEIGHTS_ZAM_LF), dict(v_range=(6.0, 12.0))),       # the 512-thread kernels, no stash
}
A, V, Y, DELTA, S_PROG = ("u", 1), ("x", 3), ("x", 1), ("x", 2), ("x", 5)


def late(cfg):
    return range(cfg.N // 2, cfg.N + 1)


def index(cfg, var, k):
    """index of variable var = ("u" | "x", column) of stage k in w"""
    return 2 * k + var[1] if var[0] == "u" else 2 * cfg.N + cfg.nx * k + var[1]


def extreme(cfg, x, var, stages, which):
    """[B] min / max of a variable over the stages (inputs: without the terminal stage) in the optima x [B, n_w]"""
    cols = [index(cfg, var, k) for k in stages if not (var[0] == "u" and k == cfg.N)]
    return x[:, cols].min(axis=1) if which == "min" else x[:, cols].max(axis=1)


# ---- the edits: (cfg, (lbg, ubg, lbx, ubx) -- copies, written in place --, ref: the reference-bounds optima [QB, n_w], solve: bounds -> the oracle's
#      converged optima of the same instances under them) -----------------------------------------------------------------------------------------------
def _s1(cfg, b, ref, solve=None):
    q = float(np.quantile(extreme(cfg, ref, A, range(cfg.N), "min"), 0.5))
    for k in range(cfg.N):
        b[2][index(cfg, A, k)] = q


def _s2(cfg, b, ref, solve=None):
    q = float(np.quantile(extreme(cfg, ref, V, late(cfg), "max"), 0.5))
    for k in range(cfg.N + 1):
        b[3][index(cfg, V, k)] = q if k in late(cfg) else np.inf


def _s3(cfg, b, ref, solve=None):
    """the terminal stage alone.  A box over an arc of stages leaves every pushed instance a junction stage, where its path meets the bound with
    a gap and a multiplier that are both small; the 1e-8 stop then sits 1e-6 .. 1e-4 from the optimum (the oracle at 1e-8 against itself at
    1e-12), and two correct codes end 3e-9 apart (y on k >= N / 2, N = 10: emulated solve against oracle, same iterations; 7e-15 with this box)"""
    k = cfg.N
    lo = float(np.quantile(ref[:, index(cfg, Y, k)], 0.1))
    hi = float(np.quantile(ref[:, index(cfg, Y, k)], 0.6))
    b[2][index(cfg, Y, k)], b[3][index(cfg, Y, k)] = lo, hi


def _s4(cfg, b, ref, solve=None):
    b[0][0] = 0.5


def _s5(cfg, b, ref, solve=None):
    b[1][0] = np.inf


def _ou(value):
    def edit(cfg, b, ref, solve=None):
        b[1][1 + cfg.nx * (cfg.N + 1):] = value
    return edit


def _s7(cfg, b, ref, solve=None):
    for k in range(cfg.N + 1):
        b[2][index(cfg, DELTA, k)], b[3][index(cfg, DELTA, k)] = -np.inf, np.inf
        b[2][index(cfg, V, k)] = -np.inf


def _s8(cfg, b, ref, solve=None):
    assert cfg.nx == 6
    for k in range(cfg.N + 1):
        b[3][index(cfg, S_PROG, k)] = 1e4


def _s9_a(cfg, b, ref, solve):
    """S1 inside S9.  A floor on the acceleration at the median of the reference optima and a ceiling on the late speed at theirs contradict each
    other for every instance that has to brake for the ceiling (S1 + S2 as they stand: 52 - 72 % converge).  So the floor is taken from the optima
    under the point's other bounds, at the 5 % quantile of min_k a: it binds on the hardest brakers only"""
    q = float(np.quantile(extreme(cfg, solve(b), A, range(cfg.N), "min"), 0.05))
    for k in range(cfg.N):
        b[2][index(cfg, A, k)] = q


def _all(*edits):
    def edit(cfg, b, ref, solve=None):
        for e in edits:
            e(cfg, b, ref, solve)
    return edit


@dataclass(frozen=True)
class Point:
    name: str
    edit: object = field(compare=False)
    binding: str = "inactive"                   # "binds": meant to move >= 25 % of the optima; "some": binds on a few instances; "inactive"
    kw: tuple = ()                              # further arguments of synthetic_batch (lane following)
    obst_mult: dict = field(default_factory=dict, compare=False, hash=False)       # kind -> obst_mult of the descriptor, where not 3
    nx6_only: bool = False

    def mult(self, fam):
        return self.obst_mult.get("ca" if fam == "ca" else "lane", 3)


HEADING0 = (("heading", 0.0),)
POINTS = {p.name: p for p in [
    Point("S1", _s1, binding="binds"),
    Point("S2", _s2, binding="binds"),
    Point("S3", _s3, binding="binds", kw=HEADING0),
    Point("S4", _s4, binding="some"),
    Point("S5", _s5, binding="binds"),
    Point("S6", _ou(1000.0)),
    Point("S7", _s7),
    Point("S8", _s8, nx6_only=True),
    Point("S9", _all(_s2, _s3, _s4, _ou(1000.0), _s9_a), binding="binds", kw=HEADING0),
    Point("S10", _ou(1000.0), obst_mult=dict(lane=2)),
]}
CA_POINTS = {p.name: p for p in [
    Point("S6", _ou(60.0)),
    Point("S10", _ou(60.0), obst_mult=dict(ca=1)),
    Point("FLOU", _all(_s4, _ou(1000.0)), binding="binds"),
]}
CA_BINDING_OU = Point("S6_binding", _ou(31.0), binding="binds")          # measured and not kept (see the module's text)
BINDING = tuple(n for n, p in POINTS.items() if p.binding == "binds")


def point(name, fam):
    return name if isinstance(name, Point) else (CA_POINTS if fam == "ca" else POINTS)[name]


def cfg_of(fam):
    return CA_CFG if fam == "ca" else LANE[fam][0]


def lane_cases(fams=("n10", "n30")):
    """(point, family) of every lane-following point on the families (S8 where nx = 6 only)"""
    return [(n, f) for f in fams for n, p in POINTS.items() if not (p.nx6_only and cfg_of(f).nx != 6)]


def case_id(c):
    return f"{c[0]}-{c[1]}"


def inputs(name, fam, B, start=0):
    """(x0, p) of instances start .. start + B - 1 of the batch the point is used with"""
    if fam == "ca":
        return ca_batch(CA_CFG, B, start=start)
    cfg, kw = LANE[fam]
    return synthetic_batch(cfg, B, start=start, **{**kw, **dict(point(name, fam).kw)})


def oracle_for(cfg, bounds=None, **kw):
    """the C oracle with these (lbg, ubg, lbx, ubx)"""
    o = OracleSolver(cfg, **kw)
    if bounds is not None:
        lbg, ubg, lbx, ubx = bounds
        o.lbx, o.ubx = np.ascontiguousarray(lbx, dtype=np.float64), np.ascontiguousarray(ubx, dtype=np.float64)
        o.desc.fric_lo, o.desc.fric_hi, o.desc.obst_lo, o.desc.obst_hi = float(lbg[0]), float(ubg[0]), float(lbg[-1]), float(ubg[-1])
    return o


def _frozen(r):
    for a in r.values():
        a.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def _reference_rows(fam, kw, B, start, step):
    cfg = cfg_of(fam)
    x0, p = ca_batch(cfg, B, start=start) if fam == "ca" else synthetic_batch(cfg, B, start=start, **{**LANE[fam][1], **dict(kw)})
    return _frozen(OracleSolver(cfg).solve_batch(x0[::step], p[::step], nthreads=8))


def reference_rows(name, fam, B=QB, start=0, step=1):
    """the oracle under the REFERENCE bounds on rows 0, step, .. of the point's batch: dict(x, status, iters, kkt), computed once, read-only"""
    return _reference_rows(fam, point(name, fam).kw, int(B), int(start), int(step))


@functools.lru_cache(maxsize=None)
def _bounds(pt, fam):
    cfg = cfg_of(fam)
    b = [np.array(a, dtype=np.float64) for a in BicycleNLP(cfg).bounds()]
    x0, p = inputs(pt, fam, QB)

    def solve(bb):
        r = oracle_for(cfg, bb, obst_mult=pt.mult(fam)).solve_batch(x0, p, nthreads=8)
        return r["x"][r["status"] == 1]

    pt.edit(cfg, b, _reference_rows(fam, pt.kw, QB, 0, 1)["x"], solve)
    for a in b:
        a.setflags(write=False)
    return tuple(b)


def bounds(name, fam):
    """(lbg, ubg, lbx, ubx) of the point on the family, read-only"""
    return _bounds(point(name, fam), fam)


def newly_bounded(name, fam):
    """(indices of w whose lower bound the point set or moved, ... whose upper bound)"""
    ref = BicycleNLP(cfg_of(fam)).bounds()
    b = bounds(name, fam)
    return np.flatnonzero((b[2] != ref[2]) & np.isfinite(b[2])), np.flatnonzero((b[3] != ref[3]) & np.isfinite(b[3]))


@functools.lru_cache(maxsize=None)
def _oracle(pt, fam, B, start, step):
    x0, p = inputs(pt, fam, B, start)
    return _frozen(oracle_for(cfg_of(fam), _bounds(pt, fam), obst_mult=pt.mult(fam)).solve_batch(x0[::step], p[::step], nthreads=8))


def oracle_rows(name, fam, B=QB, start=0, step=1):
    """the oracle under the point's bounds on rows 0, step, .. of inputs(name, fam, B, start): computed once per session, read-only"""
    return _oracle(point(name, fam), fam, int(B), int(start), int(step))


def imposed(b):
    """(lbg, ubg, lbx, ubx) as the solve imposes them: every finite side of an inequality moved outwards by 1e-8 max(1, |bound|) -- IPOPT's
    bound_relax_factor, relax_lo / relax_hi of csrc/mpc_host_common.h; the equality rows as they are.  An active bound's optimum sits on the moved
    side, so against the bound as given its gap is -1e-8 max(1, |bound|), and a multiplier of 10^3 (a box that pushes a path by metres) makes
    |lam x gap| 1e-5 .. 1e-4 there; against the moved side it is the barrier's mu"""
    lbg, ubg, lbx, ubx = [np.array(a, dtype=np.float64) for a in b]
    ineq = lbg < ubg
    lo = lambda a: np.where(np.isfinite(a), a - 1e-8 * np.maximum(1.0, np.abs(a)), a)          # noqa: E731
    hi = lambda a: np.where(np.isfinite(a), a + 1e-8 * np.maximum(1.0, np.abs(a)), a)          # noqa: E731
    return np.where(ineq, lo(lbg), lbg), np.where(ineq, hi(ubg), ubg), lo(lbx), hi(ubx)


def step64(B):
    """stride that leaves at most 64 evenly spaced rows of B"""
    return -(-B // 64)


def install(solver, name, fam):
    """mpc_set_bounds with the point's arrays on a BatchedMPCSolver"""
    lbg, ubg, lbx, ubx = bounds(name, fam)
    solver.set_bounds(lbx, ubx, lbg, ubg)


# ---- measured ----------------------------------------------------------------------------------------------------------------------------------
# the oracle alone on the QB instances, (point, family): (share converged, share of optima moved by > 1e-3) -- written by hand from the output of
# tests/test_bound_structures_cpu.py::test_conditions_from_the_oracle_alone, which asserts the conditions themselves
SHARES = {
    ("S1", "n10"): (1.0, 0.484), ("S2", "n10"): (1.0, 0.5), ("S3", "n10"): (1.0, 0.5), ("S4", "n10"): (1.0, 0.031), ("S5", "n10"): (1.0, 0.453),
    ("S6", "n10"): (1.0, 0.0), ("S7", "n10"): (1.0, 0.0), ("S9", "n10"): (0.969, 0.661), ("S10", "n10"): (1.0, 0.0),
    ("S1", "n30"): (1.0, 0.484), ("S2", "n30"): (1.0, 0.5), ("S3", "n30"): (1.0, 0.516), ("S4", "n30"): (1.0, 0.078), ("S5", "n30"): (1.0, 0.594),
    ("S6", "n30"): (1.0, 0.0), ("S7", "n30"): (1.0, 0.0), ("S8", "n30"): (1.0, 0.0), ("S9", "n30"): (1.0, 0.734), ("S10", "n30"): (1.0, 0.0),
    ("S1", "n50"): (1.0, 0.484), ("S2", "n50"): (1.0, 0.5), ("S3", "n50"): (1.0, 0.516), ("S4", "n50"): (1.0, 0.234), ("S5", "n50"): (1.0, 0.375),
    ("S6", "n50"): (1.0, 0.0), ("S7", "n50"): (1.0, 0.0), ("S9", "n50"): (1.0, 0.766), ("S10", "n50"): (1.0, 0.0),
    ("S1", "n64"): (1.0, 0.5), ("S2", "n64"): (1.0, 0.5), ("S3", "n64"): (1.0, 0.516), ("S4", "n64"): (1.0, 0.094), ("S5", "n64"): (1.0, 0.344),
    ("S6", "n64"): (1.0, 0.0), ("S7", "n64"): (1.0, 0.0), ("S8", "n64"): (1.0, 0.0), ("S9", "n64"): (1.0, 0.766), ("S10", "n64"): (1.0, 0.0),
    ("S6", "ca"): (0.984, 0.0), ("S10", "ca"): (1.0, 0.0), ("FLOU", "ca"): (0.984, 0.714),
    ("S6_binding", "ca"): (0.75, 1.0),          # circle rows ubg = 31: not kept
}
# the MI355X: worst |x - x_oracle| per path over the points and worst |dx| between the paths of a point, with the point it occurs at
# (tests/test_gpu_bound_structures.py prints them; before k_solve_wg symmetrised the cost-to-go under a heavy bound on y: 2.2e-7 at S3 n30, 4.8e-6 at S3 n50)
GPU_WORST = {
    "default (k_solve_wg alone)": (3.4e-10, "S3 n30"), "hybrid = 0 (k_pipeline to the end)": (7.8e-11, "S3 n30"),
    "hybrid = 0, pipeline = 0": (7.8e-11, "S3 n30"), "the same with big_wg = 1": (7.8e-11, "S3 n30"), "bound_mask = 0 at S1, S4, S5": (3.6e-14, "S5 n30"),
    "hybrid hand-over, B = 2305": (9.1e-13, "S9 n30"), "between the paths of a point": (3.0e-10, "S3 n30"),
}


# ---- dw/dbounds at a point (mpc_sens_bounds) -------------------------------------------------------------------------------------------------------
SENS_CASES = {("FLOU", "ca"): (70, list(range(6)) + list(range(64, 70))), ("S9", "n10"): (16, list(range(16)))}      # (B, rows compared)


def sens_directions(name, fam, B, seed=67):
    """dbv [B, n_dir, n_b]: the nine level directions and a random one (tests/test_sens_bounds_cpu.py: directions), then fl alone, ou alone and,
    where the point bounds one, the terminal y's upper bound alone; and the names of the last ones"""
    import sens_bounds_ref as bref
    cfg = cfg_of(fam)
    nw, nb = cfg.n_w, bref.n_b(cfg)
    extra = [("fl", 2 * nw + bref.FL), ("ou", 2 * nw + bref.OU)]
    if index(cfg, Y, cfg.N) in newly_bounded(name, fam)[1]:
        extra.append(("ubx[y_N]", nw + index(cfg, Y, cfg.N)))
    d = np.zeros((B, 10 + len(extra), nb))
    d[:, :9] = bref.level_directions(cfg)
    d[:, 9] = np.random.default_rng(seed).uniform(-1.0, 1.0, size=(B, nb))
    for q, (_, i) in enumerate(extra):
        d[:, 10 + q, i] = 1.0
    return d, [n for n, _ in extra]
