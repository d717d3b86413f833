"""CPU: the pieces of the closed loop past per-ego obstacles that move (mpc_closed_loop_batch_obst, mpc_validity_batch_ego) that need no GPU.

tests/loopx/loopx.cpp calls the functions k_loop_obst runs (csrc/mpc_closed_loop.h: loop_obstacle_centres, loop_clearance, loop_obst_instance)
on the CPU; the oracle loop over the scenes of tests/loop_obst_ref.py is the reference of tests/test_gpu_loop_obstacles.py, and what those
tests presuppose about it is checked here."""
import ctypes as C
import os

import numpy as np
import pytest

import loop_obst_ref as ref
from helpers import ROOT, abi, harness_lib, pkg
from oracle.nlp_numpy import circle_centers

scn = __import__("importlib").import_module(pkg.__name__ + ".scenario")
opt = ref.opt
_dp = abi.as_dp


def test_new_entry_points_declared_and_exported():
    new = ("mpc_closed_loop_batch_obst", "mpc_closed_loop_batch_obst_dev", "mpc_validity_batch_ego", "mpc_validity_batch_ego_dev")
    hdr = open(os.path.join(ROOT, "include", "mpcgpu.h")).read()
    L = C.CDLL(abi.LIB_PATH)
    for s in new:
        assert s in abi.EXPORTS and hasattr(L, s) and ("int " + s + "(") in hdr, s
    assert len(abi.PROTOTYPES["mpc_closed_loop_batch_obst"]) == 18 and len(abi.PROTOTYPES["mpc_closed_loop_batch_obst_dev"]) == 19
    assert abi.PROTOTYPES["mpc_validity_batch_ego"] == abi.PROTOTYPES["mpc_validity_batch"]
    assert abi.PROTOTYPES["mpc_validity_batch_ego_dev"] == abi.PROTOTYPES["mpc_validity_batch_dev"]


@pytest.fixture(scope="module")
def loopx():
    L = C.CDLL(harness_lib("loopx"))
    dp = C.POINTER(C.c_double)
    L.loopx_centres.argtypes = [C.c_int32, dp, C.c_double, dp]
    L.loopx_clearance.argtypes = [C.c_int32, C.c_double, dp, dp, C.c_double, dp]
    L.loopx_step.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, dp, C.c_double, dp, C.c_double, C.c_int32, dp, dp]
    for f in (L.loopx_centres, L.loopx_clearance, L.loopx_step):
        f.restype = None
    return L


def _random_poses(rng, n):
    return np.ascontiguousarray(np.stack([rng.uniform(-200, 200, n), rng.uniform(-50, 50, n), rng.uniform(-np.pi, np.pi, n)], axis=1))


def test_obstacle_centres_against_the_oracles_circle_centres(loopx):
    """loop_obstacle_centres restates compute_centers_of_approximation_circles (configuration.py:69-93) in the order of
    mpc_problem_desc::obstacle: against oracle.nlp_numpy.circle_centers on random poses and rectangles, to round-off (one product and one
    sum per coordinate, |coordinate| <= 200: a few ulp of 200)"""
    rng = np.random.default_rng(11)
    for length, width in ((6.0, 3.5), (4.508, 1.61), (12.3, 2.5), (0.0, 0.0)):
        poses = _random_poses(rng, 200)
        poses[0, 2] = 0.0                                           # heading 0: exact
        offset = ref.approximating_circle_radius(length, width)[1] / 4
        out = np.empty((200, 6))
        loopx.loopx_centres(200, _dp(poses), offset, _dp(out))
        want = np.array([circle_centers(x, y, length, width, th).ravel() for x, y, th in poses])
        assert np.abs(out - want).max() <= 1e-13
        assert np.array_equal(out[0], [poses[0, 0], poses[0, 1], poses[0, 0] + offset, poses[0, 1], poses[0, 0] - offset, poses[0, 1]])


def test_clearance_against_numpy(loopx):
    """loop_clearance (the NLP's circle geometry, circle_eval of mpc_stage_math.h): min over the three constrained pairs of distance - r_sum,
    against the numpy restatement to round-off (distances up to ~500 m: 1e-12 is a few ulp)"""
    rng = np.random.default_rng(12)
    n = 500
    states = np.ascontiguousarray(np.stack([rng.uniform(-200, 200, n), rng.uniform(-50, 50, n), rng.uniform(-1, 1, n), rng.uniform(0, 30, n),
                                            rng.uniform(-np.pi, np.pi, n)], axis=1))
    c6 = np.ascontiguousarray(ref.centres_numpy(_random_poses(rng, n)))
    c6[:50, 0::2] = states[:50, 0:1] + rng.uniform(-4, 4, (50, 3))        # some close by, where the three pairs differ
    c6[:50, 1::2] = states[:50, 1:2] + rng.uniform(-4, 4, (50, 3))
    out = np.empty(n)
    loopx.loopx_clearance(n, 0.75, _dp(states), _dp(c6), 3.3, _dp(out))
    want = ref.clearance_numpy(states, c6, 0.75, 3.3)
    assert np.abs(out - want).max() <= 1e-12
    # the pair that decides is not always the centre pair
    d = [np.hypot(states[:, 0] + sg * 0.75 * np.cos(states[:, 4]) - c6[:, 2 * j], states[:, 1] + sg * 0.75 * np.sin(states[:, 4]) - c6[:, 2 * j + 1])
         for j, sg in enumerate((0.0, 1.0, -1.0))]
    assert len(set(np.argmin(d, axis=0))) == 3


@pytest.mark.parametrize("nx", [5, 6])
def test_one_step_of_the_obstacle_kernel(loopx, nx):
    """loop_obst_instance, what a thread of k_loop_obst does: row min(i, Lt - 1) of the ego's track -> its row of the solve's obstacle centres,
    clearance[b, i] from its current state (rows of nx states) and nothing else of the clearance buffer; Lt = 1 holds the pose"""
    rng = np.random.default_rng(13)
    B, L = 7, 5
    state = np.ascontiguousarray(rng.uniform(-3, 3, (B, nx)))
    for Lt in (1, L, L + 3):
        track = np.ascontiguousarray(rng.uniform(-10, 10, (B, Lt, 3)))
        for i in (0, 2, L - 1):
            obst, cl = np.full((B, 6), np.nan), np.full((B, L), np.nan)
            loopx.loopx_step(B, L, Lt, nx, 0.75, _dp(track), 1.0, _dp(state), 3.3, i, _dp(obst), _dp(cl))
            row = track[:, min(i, Lt - 1)]
            want = np.stack([row[:, 0], row[:, 1], row[:, 0] + np.cos(row[:, 2]), row[:, 1] + np.sin(row[:, 2]), row[:, 0] - np.cos(row[:, 2]),
                             row[:, 1] - np.sin(row[:, 2])], axis=1)
            assert np.abs(obst - want).max() <= 1e-14
            assert np.abs(cl[:, i] - ref.clearance_numpy(state[:, :5], obst, 0.75, 3.3)).max() <= 1e-13
            assert np.isnan(np.delete(cl, i, axis=1)).all()
            loopx.loopx_step(B, L, Lt, nx, 0.75, _dp(track), 1.0, _dp(state), 3.3, i, _dp(obst), None)          # (no clearance asked for)


@pytest.mark.parametrize("moving", [True, False])
def test_oracle_loop_converges_on_every_scene(moving):
    """what the GPU tests presuppose: one oracle solve per step with that step's obstacle converges at every step of the ten scenes, in at most
    16 iterations and without a second chance, with active circle rows (the ego swerves)"""
    r = ref.oracle_loops(moving)
    assert r["status"].shape == (len(ref.SCENES), ref.L)                       # (a second chance would have logged further solves)
    assert np.all(r["status"] == 1) and r["iters"].max() <= 16
    swerve = np.abs(r["traj"][:, :, 1]).max(axis=1)
    assert swerve.max() > 0.4 and np.sum(swerve > 0.05) >= 8
    assert r["clearance"].min() > -1e-6                                        # (the plans of the oracle keep their distance at every step)


def test_oracle_loop_moving_and_static_runs_differ():
    a, b = ref.oracle_loops(True), ref.oracle_loops(False)
    assert np.abs(a["traj"] - b["traj"]).max() > 1e-2
    assert np.sum(np.abs(a["traj"] - b["traj"]).max(axis=(1, 2)) > 1e-2) >= 8


# ---- the Python layer, through stand-ins for the library ---------------------------------------------------------------------------------
class _FakeLib:
    """records the calls BatchedMPCSolver makes (no GPU, no library)"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def _solver_without_gpu():
    s = object.__new__(pkg.BatchedMPCSolver)
    s._lib, s._h, s.N, s.nx = _FakeLib(), C.c_void_p(1), 10, 5
    return s


def test_per_ego_verdict_argument_checks():
    s = _solver_without_gpu()
    B, L, n = 4, 6, 2
    traj = np.zeros((B, L, 5))
    s.validity(traj, np.ones((B, n, L, 5)))                                     # 4-d: per ego, inferred
    s.validity(traj, np.ones((B, n, 5)), per_ego=True)                          # static rectangles per ego
    s.validity(traj, np.ones((n, L + 2, 5)))                                    # shared, as before
    s.validity(traj, np.ones((B, n, L + 2, 5)), per_ego=True)                   # longer recordings are cut to L
    names = [c[0] for c in s._lib.calls]
    assert names == ["mpc_validity_batch_ego", "mpc_validity_batch_ego", "mpc_validity_batch", "mpc_validity_batch_ego"]
    assert [c[1][6] for c in s._lib.calls] == [n, n, n, n] and all(c[1][1:3] == (B, L) for c in s._lib.calls)
    for bad in (np.ones((B + 1, n, L, 5)), np.ones((B, n, L - 1, 5)), np.ones((B, n, L, 4))):
        with pytest.raises(pkg.MpcError):
            s.validity(traj, bad)
    with pytest.raises(pkg.MpcError):
        s.validity(traj, np.ones((n, 5)), per_ego=True)


def test_closed_loop_hands_the_track_over():
    s = _solver_without_gpu()
    B, L = 3, 12
    init, path, orient = np.zeros((B, 5)), np.zeros((B, L, 2)), np.zeros((B, L))
    assert len(s.closed_loop(init, path, orient, 10.0, L)) == 3
    out = s.closed_loop(init, path, orient, 10.0, L, obst_track=np.zeros((B, L, 3)), obst_offset=1.0, clearance=True)
    assert len(out) == 4 and out[3].shape == (B, L)
    assert len(s.closed_loop(init, path, orient, 10.0, L, obst_track=np.zeros((B, 3)))) == 3                  # one standing pose per ego
    (n0, _), (n1, a1), (n2, a2) = s._lib.calls
    assert (n0, n1, n2) == ("mpc_closed_loop_batch_ex", "mpc_closed_loop_batch_obst", "mpc_closed_loop_batch_obst")
    assert a1[8] == L and a1[10] == 1.0 and a1[17] is not None and a2[8] == 1 and a2[17] is None
    with pytest.raises(pkg.MpcError):
        s.closed_loop(init, path, orient, 10.0, L, clearance=True)
    with pytest.raises(pkg.MpcError):
        s.closed_loop(init, path, orient, 10.0, L, obst_track=np.zeros((B, L, 2)))


def test_optimizer_host_loop_hands_every_step_its_obstacle():
    """CasadiOptimizer with configuration.obstacle_track: the host loop passes the centres of the step's pose as obst= (the last pose once the
    track ends); without the attribute the solver is called as before"""
    seen = []

    class Spy(ref.OracleObstBackend):
        def solve(self, x0, p, obst=None):
            seen.append(None if obst is None else np.array(obst).ravel().copy())
            return super().solve(x0, p, obst)

    track = ref.track_of(ref.SCENES[2])[:25]                                   # shorter than the run: the last pose is held
    ref.host_loop(Spy(ref.CFG), track)
    assert len(seen) == ref.L
    want = ref.centres_numpy(track[np.minimum(np.arange(ref.L), 24)])
    assert np.abs(np.array(seen) - want).max() <= 1e-13
    seen.clear()
    path, orient = ref.straight_path(ref.L, 0.0, 0.0, 0.0, ref.V_EGO)
    conf = ref.make_configuration(path, orient, ref.V_EGO, ref.WEIGHTS_YAML_ZAM_LF)
    o = opt.CasadiOptimizer(configuration=conf, init_values=(np.array([0.0, 0.0]), ref.V_EGO, 0.0, 0.0), predict_horizon=ref.N)
    o.use_device_loop = False
    o._sol = opt.NlpSolverHandle(Spy(ref.NLPConfig(N=ref.N, nx=5)))
    o.optimize()
    assert len(seen) == ref.L and all(v is None for v in seen)


def test_scenario_obstacle_track(golden_dir):
    sc = scn.read_scenario(os.path.join(golden_dir, "scenarios", "USA_Lanker-2_18_T-1_route.xml"))
    o = sc.dynamic_obstacles[0]
    times = sorted(o.states)
    steps = times[-1] + 6
    track, length, width = scn.obstacle_track(sc, o.obstacle_id, steps)
    assert track.shape == (steps, 3) and (length, width) == (o.length, o.width)
    for t in times:
        assert tuple(track[t]) == o.states[t]
    assert np.array_equal(track[times[-1]:], np.tile(o.states[times[-1]], (6, 1)))       # holds the last pose when the recording ends
    assert np.array_equal(track[:times[0] + 1], np.tile(o.states[times[0]], (times[0] + 1, 1)))
    rect = scn.obstacle_rectangles(sc, times[-1] + 1)
    k = len(sc.obstacles)
    assert np.array_equal(rect[k][times[0]:, [0, 1, 4]], track[times[0]:times[-1] + 1])
    with pytest.raises(KeyError):
        scn.obstacle_track(sc, -5, 3)


def test_configuration_fills_the_track_only_when_the_settings_name_an_obstacle(golden_dir):
    from test_scenario import SETTINGS_USA, XML_USA
    sc = scn.read_scenario(XML_USA)
    conf = scn.Configuration(SETTINGS_USA, sc, 21007).configuration
    assert not hasattr(conf, "obstacle_track")
    o = sc.dynamic_obstacles[1]
    settings = dict(SETTINGS_USA, scenario_settings=dict(SETTINGS_USA["scenario_settings"], use_case="collision_avoidance", dynamic_obstacle_id=o.obstacle_id))
    conf = scn.Configuration(settings, sc, 21007).configuration
    track, length, width = scn.obstacle_track(sc, o.obstacle_id, conf.iter_length)
    assert np.array_equal(conf.obstacle_track, track) and conf.obstacle_track.shape == (conf.iter_length, 3)
    so = conf.static_obstacle
    assert (so["length"], so["width"]) == (length, width) and (so["position_x"], so["position_y"], so["orientation"]) == tuple(track[0])
    op = opt.CasadiOptimizer(configuration=conf, init_values=scn.init_values(sc, 21007), predict_horizon=10)
    assert np.array_equal(op.obstacle_track, track) and op.obstacle_offset == ref.approximating_circle_radius(length, width)[1] / 4
    assert np.abs(op.obstacle_centers_at(3) - circle_centers(track[3, 0], track[3, 1], length, width, track[3, 2]).ravel()).max() <= 1e-13
