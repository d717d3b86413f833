"""CPU: the FORCES-mode closed loop past per-ego obstacles that move (mpc_forces_closed_loop_batch_obst), the parts that need no GPU.

tests/floopx/floopx.cpp calls what the threads of k_floop_turn_setup / k_floop_turn run (csrc/mpc_closed_loop.h: forces_turn_setup_row,
forces_turn_row) and forces_qp_instance between them; tests/floop_ref.py is the numpy loop they are checked against, and what the GPU tests
presuppose about its scenes is checked here from that loop alone."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import floop_ref as ref
from helpers import ROOT, abi, harness_lib
from oracle import forces_qp_numpy as Q

_dp, _ip = abi.as_dp, abi.as_ip


def test_new_entry_points_declared_and_exported():
    new = ("mpc_forces_closed_loop_batch_obst", "mpc_forces_closed_loop_batch_obst_dev")
    hdr = open(os.path.join(ROOT, "include", "mpcgpu.h")).read()
    L = C.CDLL(abi.LIB_PATH)
    for s in new:
        assert s in abi.EXPORTS and hasattr(L, s) and ("int " + s + "(") in hdr, s
    assert len(abi.PROTOTYPES["mpc_forces_closed_loop_batch_obst"]) == 27 and len(abi.PROTOTYPES["mpc_forces_closed_loop_batch_obst_dev"]) == 28
    # the arguments the new entry adds to mpc_forces_closed_loop_batch sit between hessian_mode and the noise tail, clearance at the end
    old, new = abi.PROTOTYPES["mpc_forces_closed_loop_batch"], abi.PROTOTYPES["mpc_forces_closed_loop_batch_obst"]
    assert new[:14] == old[:14] and new[20:26] == old[14:] and new[14:20] == [C.c_int32, C.c_int32, abi._dp, C.c_double, C.c_int32, C.c_double]
    assert L.mpc_abi_version() == 1


class FloopxIn(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "N", "L", "Lp", "guess_mode", "Lt", "predict", "noise_mode")] + \
               [(n, C.POINTER(C.c_double)) for n in ("init_state", "init_acc", "path", "orient", "vdes", "track", "obstacle")] + \
               [(n, C.c_double) for n in ("offset", "r_sum", "ego_offset", "dt", "wheelbase", "sigma")] + [("seed", C.c_uint64)]


@pytest.fixture(scope="module")
def floopx():
    L = C.CDLL(harness_lib("floopx"))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L.floopx_launch.argtypes = [C.POINTER(FloopxIn), C.c_int32, C.c_int32, dp, dp, dp, dp, ip, dp, dp, ip, dp]
    L.floopx_launch.restype = None
    L.floopx_loop.argtypes = [C.POINTER(FloopxIn), C.c_int32, dp, dp, dp, C.c_double, dp, dp, dp, dp, C.c_int32, dp, dp, ip, dp, dp, dp]
    L.floopx_loop.restype = C.c_int
    return L


def _inputs(keep, N, L, init, path, orient, vdes, track=None, guess_mode=0, predict=0, obstacle=None, sigma=0.0, seed=None, init_acc=None):
    """FloopxIn over contiguous copies of the arrays (kept alive in `keep`)"""
    arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (init, init_acc, path, orient, vdes, track, obstacle)]
    keep.extend(arrs)
    s = FloopxIn(B=init.shape[0], N=N, L=L, Lp=path.shape[1], guess_mode=guess_mode, Lt=0 if track is None else track.shape[1], predict=predict,
                 noise_mode=0 if seed is None else 2, offset=ref.OBST_OFFSET, r_sum=ref.R_SUM, ego_offset=ref.EGO_OFFSET, dt=ref.DT, wheelbase=ref.WHEELBASE,
                 sigma=sigma, seed=0 if seed is None else seed)
    for name, a in zip(("init_state", "init_acc", "path", "orient", "vdes", "track", "obstacle"), arrs):
        setattr(s, name, _dp(a))
    return s


@pytest.mark.parametrize("N", [1, 2, 3, 4, 7, 10])
def test_parameter_and_guess_rows(floopx, N):
    """what the threads of one launch write, for every (b, j, k): the parameter rows of step k + 1 (of step 0 from the setup launch) and the guess rows
    against floop_ref.param_rows / next_guess -- both predict values, Lt = 1, L, L + N and no track, both guess modes with exitflags 1 and others.
    Path, velocity and orientation entries exactly, the centres to 1e-13 (the bound of test_loop_obstacles_cpu's centres test).  Lp = L - 1, so the
    last path point is repeated at every horizon; the last launch writes no row; the threads in ascending and in descending order."""
    rng = np.random.default_rng(100 + N)
    B, L = 3, 2 * N + 4
    Lp = L - 1
    init = rng.uniform(-2, 2, (B, 5))
    acc = rng.uniform(-1, 1, B)
    path, orient, vdes = rng.uniform(-50, 50, (B, Lp, 2)), rng.uniform(-3, 3, (B, Lp)), rng.uniform(1, 20, B)
    obstacle = rng.uniform(-30, 30, 6)
    z0 = np.stack([np.zeros(B), acc, init[:, 0], init[:, 1], np.zeros(B), init[:, 3], init[:, 4]], axis=1)
    for Lt in (0, 1, L, L + N):
        track = None if Lt == 0 else rng.uniform(-10, 10, (B, Lt, 3))
        for predict in ((0,) if Lt == 0 else (0, 1)):
            for guess_mode in (0, 1):
                keep = []
                A = _inputs(keep, N, L, init, path, orient, vdes, track, guess_mode, predict, obstacle, init_acc=acc)
                state, zbar, params = np.full((B, 5), np.nan), np.full((B, N, 7), np.nan), np.full((B, N, 10), np.nan)
                traj, ctrl, sf, cl = np.zeros((B, L, 5)), np.zeros((B, L, 2)), np.zeros((B, L), np.int32), np.full((B, L), np.nan)
                z_out, flag = np.zeros((B, N, 7)), np.ones(B, np.int32)

                def launch(k, reverse):
                    floopx.floopx_launch(C.byref(A), k, reverse, _dp(state), _dp(zbar), _dp(params), _dp(z_out), _ip(flag), _dp(traj), _dp(ctrl), _ip(sf),
                                         None if Lt == 0 else _dp(cl))

                def check_params(k):
                    want = ref.param_rows(k, N, L, path, orient, vdes, track, ref.OBST_OFFSET, predict, obstacle)
                    assert np.array_equal(params[:, :, :4], want[:, :, :4]), (Lt, predict, k)
                    assert np.abs(params[:, :, 4:] - want[:, :, 4:]).max() <= 1e-13, (Lt, predict, k)
                    if Lt == 0:
                        assert np.array_equal(params[:, :, 4:], want[:, :, 4:])

                launch(-1, 0)
                assert np.array_equal(zbar, np.repeat(z0[:, None], N, axis=1)) and np.array_equal(state, z0[:, 2:])
                check_params(0)
                for k in range(L):
                    z_out = np.ascontiguousarray(rng.uniform(-1, 1, (B, N, 7)))
                    flag = np.ascontiguousarray(rng.choice([1, 1, 0, -7], B).astype(np.int32))
                    before, before_p = zbar.copy(), params.copy()
                    launch(k, k & 1)
                    if k + 1 < L:
                        assert np.array_equal(zbar, ref.next_guess(before, z_out, flag, guess_mode)), (Lt, predict, guess_mode, k)
                        check_params(k + 1)
                    else:
                        assert np.array_equal(zbar, before) and np.array_equal(params, before_p)
                    assert np.array_equal(sf[:, k], flag) and np.array_equal(ctrl[:, k], z_out[:, 0, :2])
                assert np.isnan(cl).all() if Lt == 0 else not np.isnan(cl).any()


def _harness_loop(floopx, sc, guess_mode, predict, steps=ref.STEPS, seed=None, sigma=0.0, log=False):
    keep = []
    B, N, L = sc["init"].shape[0], sc["N"], sc["L"]
    A = _inputs(keep, N, L, sc["init"], sc["path"], sc["orient"], sc["vdes"], sc["track"], guess_mode, predict, sigma=sigma, seed=seed)
    traj, ctrl, sf, cl = np.zeros((B, L, 5)), np.zeros((B, L, 2)), np.zeros((B, L), np.int32), np.zeros((B, L))
    lz, lp = (np.zeros((steps, B, N, 7)), np.zeros((steps, B, N, 10))) if log else (None, None)
    w = ref.WEIGHTS
    big = lambda a: np.ascontiguousarray(np.where(np.isfinite(a), a, np.sign(a) * 1e308))          # noqa: E731
    rc = floopx.floopx_loop(C.byref(A), steps, _dp(np.array(w["Q"], float)), _dp(np.array(w["R"], float)), _dp(np.array(w["P"], float)), ref.FRICTION_DIV,
                            _dp(big(ref.LB)), _dp(big(ref.UB)), _dp(big(ref.HL)), _dp(big(ref.HU)), 0, _dp(traj), _dp(ctrl), _ip(sf), _dp(cl), _dp(lz), _dp(lp))
    assert rc == 0
    return dict(traj=traj[:, :steps], ctrl=ctrl[:, :steps], flag=sf[:, :steps], clearance=cl[:, :steps], log_zbar=lz, log_params=lp)


@functools.lru_cache(maxsize=None)
def _reference_run(name, mode):
    """the numpy loop over the emulated solver: scene `name` in the mode `mode` of floop_ref.MODES, steps 0..39"""
    sc = ref.scene(name)
    r = ref.run_scene(ref.emu_solver(sc["N"]), sc, *ref.MODES[mode])
    for v in r.values():
        v.setflags(write=False)
    return r


@pytest.mark.parametrize("mode", list(ref.MODES))
@pytest.mark.parametrize("name", ["overtake", "parked"])
def test_harness_loop_against_the_numpy_loop(floopx, name, mode):
    """the loop as the entry point enqueues it (setup, then forces_qp_instance and one turn per step) against the numpy loop over the same emulated
    solver, N = 10, steps 0..39: traj, ctrl and clearance within 1e-9 (the project's device-loop-vs-host-loop bound), flags equal.  In the
    predicted mode the dense-KKT oracle agrees with every solve of the loop on convergence, and on the step within the project's 1e-7."""
    sc = ref.scene(name)
    guess_mode, predict = ref.MODES[mode]
    got = _harness_loop(floopx, sc, guess_mode, predict, log=mode == "predicted")
    want = _reference_run(name, mode)
    assert np.array_equal(got["flag"], want["flag"])
    for key in ("traj", "ctrl", "clearance"):
        d = np.abs(got[key] - want[key]).max()
        print(name, mode, key, f"{d:.2e}")
        assert d <= 1e-9, key
    if mode == "predicted":
        worst = 0.0
        for k in range(ref.STEPS):
            zp, _, conv, _ = Q.sqp_step(got["log_zbar"][k, 0], got["log_params"][k, 0], got["traj"][0, k], ref.LB, ref.UB, ref.HL, ref.HU)
            assert conv == (got["flag"][0, k] == 1), k
            if conv and k + 1 < ref.STEPS:
                # (the solution is the next guess, shifted: rows 0 .. N - 2 of the next solve's logged guess)
                worst = max(worst, np.abs(zp[1:] - got["log_zbar"][k + 1, 0, :-1]).max())
                assert np.abs(zp[0, :2] - got["ctrl"][0, k]).max() < 1e-7
        print(name, "worst |z_oracle - z|", f"{worst:.2e}")
        assert worst < 1e-7


def test_harness_loop_with_noise_against_the_numpy_loop(floopx):
    """noise mode 2 (seeded applied-input noise, sigma 0.05): the harness loop against the numpy loop with noise.applied_noise, two egos"""
    sc = ref.scene("overtake")
    two = dict(sc, **{k: np.repeat(sc[k], 2, axis=0) for k in ("init", "path", "orient", "vdes", "track")})
    got = _harness_loop(floopx, two, 1, 1, seed=5, sigma=0.05)
    want = ref.run_scene(ref.emu_solver(10), two, 1, 1, seed=5, sigma=0.05)
    assert np.array_equal(got["flag"], want["flag"])
    assert np.abs(got["traj"] - want["traj"]).max() <= 1e-9 and np.abs(got["ctrl"] - want["ctrl"]).max() <= 1e-9
    assert np.abs(got["ctrl"][0] - got["ctrl"][1]).max() > 1e-3                                   # (each ego has its own samples)


def check_behaviour(run):
    """the behaviour conditions of the two scenes on `run(name, mode) -> dict(traj, flag, clearance)` over steps 0..39 (the GPU test holds the device
    loop to the same)"""
    r = run("overtake", "predicted")
    print("overtake predicted: speed", r["traj"][0, 39, 3], "min clearance", r["clearance"].min(), "flags != 1:", int((r["flag"] != 1).sum()))
    assert np.all(r["flag"] == 1) and abs(r["traj"][0, 39, 3] - 10.0) <= 0.1 and r["clearance"].min() >= -1e-3
    r = run("overtake", "today")
    print("overtake today: speed", r["traj"][0, 39, 3], "min clearance", r["clearance"].min(), "flags != 1:", int((r["flag"] != 1).sum()))
    assert r["traj"][0, 39, 3] < 3.0
    r = run("overtake", "shifted")
    print("overtake shifted: speed", r["traj"][0, 39, 3], "min clearance", r["clearance"].min(), "flags != 1:", int((r["flag"] != 1).sum()))
    assert np.any(r["flag"] != 1)
    for mode in ("shifted", "predicted"):
        r = run("parked", mode)
        print("parked", mode, ": speed", r["traj"][0, :, 3].min(), "..", r["traj"][0, :, 3].max(), "min clearance", r["clearance"].min())
        assert np.all(r["flag"] == 1)
    a, b = run("parked", "shifted"), run("parked", "predicted")                                    # Lt = 1: predict has nothing to look ahead at
    assert all(np.array_equal(a[k], b[k]) for k in ("traj", "ctrl", "flag", "clearance"))
    r = run("parked", "today")
    print("parked today: speed", r["traj"][0, 39, 3], "min clearance", r["clearance"].min(), "flags != 1:", int((r["flag"] != 1).sum()))
    assert np.any(r["flag"] != 1)


def test_behaviour_of_the_reference_loop():
    """what the feature is for, from the numpy loop over the emulated solver alone: past the overtaken obstacle with the shifted guess and the obstacle
    predicted per stage every solve converges, the ego keeps its speed and its distance (-1e-3: squared distances are convex, so only the QP's 1e-4
    residual and the second-order dynamics error remain); today's loop crawls; the shifted guess with the obstacle frozen fails; past the parked obstacle
    the shifted guess never fails and today's loop does; with one standing pose predict changes nothing"""
    check_behaviour(_reference_run)


# ---- the Python layer, through stand-ins for the library ---------------------------------------------------------------------------------
class _FakeLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def test_solver_hands_the_track_over():
    from helpers import pkg
    s = object.__new__(pkg.BatchedMPCSolver)
    s._lib, s._h, s.N, s.nx = _FakeLib(), C.c_void_p(1), 10, 5
    B, L = 3, 60
    init, path, orient = np.zeros((B, 5)), np.zeros((B, L, 2)), np.zeros((B, L))
    args = (init, path, orient, 10.0, L, ref.LB, ref.UB, ref.HL, ref.HU)
    out = s.forces_closed_loop_obst(*args)
    assert len(out) == 4 and out[3] is None
    out = s.forces_closed_loop_obst(*args, obst_track=np.zeros((B, L, 3)), obst_offset=1.0, predict=True, guess_mode=1)
    assert out[3].shape == (B, L)
    s.forces_closed_loop_obst(*args, obst_track=np.zeros((B, 3)), clearance=False, r_sum=4.0)
    (n0, a0), (n1, a1), (n2, a2) = s._lib.calls
    assert n0 == n1 == n2 == "mpc_forces_closed_loop_batch_obst"
    assert a0[14:20] == (0, 0, None, 0.0, 0, 3.3) and a0[26] is None
    assert a1[14:16] == (1, L) and a1[17:20] == (1.0, 1, 3.3) and a1[26] is not None
    assert a2[15] == 1 and a2[19] == 4.0 and a2[26] is None
    with pytest.raises(pkg.MpcError):
        s.forces_closed_loop_obst(*args, obst_track=np.zeros((B, L, 2)))


def test_optimizer_host_loop_honours_track_prediction_and_guess():
    """ForcesproOptimizer's step-by-step host loop with obstacle_track, predict_obstacle and guess_mode = 1: every solve gets the per-stage centres of
    floop_ref.param_rows and the shifted solution as its guess after exitflag 1; with the defaults problem["x0"] is never refreshed and every stage
    has the static obstacle's centres"""
    from helpers import WEIGHTS_YAML_ZAM_LF, EmuForcesBackend, make_configuration, pkg
    opt = __import__("importlib").import_module(pkg.__name__ + ".optimizer")
    N = 10
    sc = ref.scene("overtake", N)
    L = sc["L"]
    obstacle = dict(position_x=15.0, position_y=-2.5, length=6.0, width=3.5, orientation=0.0)
    seen = []

    class Spy(opt.ForcesSolverHandle):
        def solve(self, problem):
            out = super().solve(problem)
            seen.append((np.array(problem["x0"]).reshape(N, 7).copy(), np.array(problem["all_parameters"]).reshape(N, 10).copy(), out[0], out[1]))
            return out

    def run(**kw):
        seen.clear()
        conf = make_configuration(sc["path"][0, :L], sc["orient"][0, :L], 10.0, WEIGHTS_YAML_ZAM_LF, obstacle=obstacle, use_case="collision_avoidance")
        o = opt.ForcesproOptimizer(configuration=conf, init_values=(np.array([0.0, 0.0]), 10.0, 0.0, 0.0), predict_horizon=N, **kw)
        o.use_device_loop = False
        lb, ub, hl, hu = o.inequal_constraint()
        model = opt.ForcesModel(N, EmuForcesBackend(N, ref.WEIGHTS), lb, ub, hl, hu)
        o._pair = (model, Spy(model._backend, model))
        return o, o.optimize()

    track = sc["track"][0]
    o, (x, u, _) = run(obstacle_track=track, predict_obstacle=True, guess_mode=1)
    assert len(seen) == L and o.exitflags.shape == (L,) and np.array_equal(o.exitflags, [s[3] for s in seen])
    offset = o.obstacle_offset
    for k, (x0, par, out, flag) in enumerate(seen):
        want = ref.param_rows(k, N, L, sc["path"][:, :L], sc["orient"][:, :L], sc["vdes"], track[None], offset, 1)[0]
        assert np.array_equal(par[:, :4], want[:, :4]) and np.abs(par[:, 4:] - want[:, 4:]).max() <= 1e-13
        if k + 1 < L:
            z = np.array([out["x{0:02d}".format(i + 1)] for i in range(N)])
            nxt = seen[k + 1][0]
            assert np.array_equal(nxt, np.vstack((z[1:], z[-1:])) if flag == 1 else x0)
    assert np.all(o.exitflags[:ref.STEPS] == 1)
    o, _ = run(obstacle_track=track)                                                   # frozen over the horizon
    assert all(np.abs(par[:, 4:] - ref.centres(track[min(k, len(track) - 1)], offset)).max() <= 1e-13 for k, (_, par, _, _) in enumerate(seen))
    assert all(np.array_equal(s[0], seen[0][0]) for s in seen)
    with pytest.raises(AssertionError):                                                 # the default mode asserts the exitflag, as the reference does
        run()
