"""GPU: the FORCES-mode closed loop past per-ego obstacles that move (mpc_forces_closed_loop_batch_obst): the whole loop enqueued on the device --
k_floop_turn_setup, then k_forces_qp and one k_floop_turn per step -- against mpc_forces_closed_loop_batch (bit for bit in its mode) and against the
numpy host loop of tests/floop_ref.py over mpc_forces_solve_batch, the same kernel with numpy bookkeeping."""
import numpy as np
import pytest

import floop_ref as ref
from helpers import WEIGHTS_YAML_ZAM_LF, abi, make_configuration, pkg
from test_forces_loop_obst_cpu import check_behaviour

pytestmark = pytest.mark.gpu

_solvers = {}


def _solver(N, nx=5):
    if (N, nx) not in _solvers:
        w = ref.WEIGHTS
        _solvers[N, nx] = pkg.BatchedMPCSolver(N, nx, Q=w["Q"], R=w["R"], P=w["P"])
    return _solvers[N, nx]


BOUNDS = (ref.LB, ref.UB, ref.HL, ref.HU)


@pytest.mark.parametrize("seed", [None, 5])
def test_reference_mode_is_bit_for_bit_the_existing_loop(seed):
    """guess_mode 0, Lt 0: traj, ctrl and step_flag of mpc_forces_closed_loop_batch on the same handle, bit for bit; B = 130 perturbed egos (1300 stage
    threads: six blocks of 256, the last one ragged), N = 10, 30 steps (the last ten in the velocity ramp),
    without noise and with the seeded applied-input noise"""
    s = _solver(10)
    B, L = 130, 30
    rng = np.random.default_rng(1)
    init, path, orient, vdes = ref.ego_inputs(B, 10, 20.0, y0=rng.uniform(-0.3, 0.3, B))
    init[:, 3] *= rng.uniform(0.95, 1.0, B)
    path, orient = path[:, :L], orient[:, :L]
    kw = dict(init_acc=rng.uniform(-0.5, 0.5, B), noise_mode=0 if seed is None else 2, sigma=0.0 if seed is None else 0.1, seed=seed or 0)
    old = s.forces_closed_loop(init, path, orient, vdes, L, *BOUNDS, **kw)
    new = s.forces_closed_loop_obst(init, path, orient, vdes, L, *BOUNDS, **kw)
    assert new[3] is None and np.all(old[2] == 1)
    for a, b in zip(old, new[:3]):
        assert np.array_equal(a, b)


# name -> (family of floop_ref, N, B, dict(predict, seed)): the device loop in guess_mode 1; predict 1 and no noise unless named
CASES = {
    "overtake-N7": ("overtake", 7, 37, {}),
    "overtake-N10": ("overtake", 10, 37, {}),
    "weaving-N1": ("weaving", 1, 130, {}),
    "weaving-N2": ("weaving", 2, 130, {}),
    "weaving-N3": ("weaving", 3, 130, {}),
    "weaving-N4": ("weaving", 4, 130, {}),
    "parked-N10-Lt1": ("parked", 10, 37, {}),
    "weaving-N3-frozen": ("weaving", 3, 130, dict(predict=0)),
    # (applied-input noise of sigma 0.05 on the overtake family leaves 22 of its 37 egos with every exitflag 1 -- an ego planning along the constraint
    #  boundary is pushed where its linearised QP is inconsistent; 11 of 37 even at sigma 0.01 -- so the noise cases are the families below)
    "weaving-N4-noise": ("weaving", 4, 130, dict(seed=5)),
    "parked-N10-Lt1-noise": ("parked", 10, 37, dict(seed=5)),
}


def case_inputs(name):
    fam, N, B, kw = CASES[name]
    init, path, orient, vdes, track = getattr(ref, fam + "_family")(B, N)
    return N, B, init, path, orient, vdes, track, kw.get("predict", 1), kw.get("seed")


def compared_steps(flag):
    """per ego, the steps compared: up to and including its first step with an exitflag other than 1 in the host loop (a failed QP's output amplifies
    round-off), as a mask [B, L]"""
    failed = flag != 1
    first = np.where(failed.any(axis=1), failed.argmax(axis=1), flag.shape[1])
    return np.arange(flag.shape[1])[None, :] <= first[:, None]


@pytest.mark.parametrize("name", list(CASES))
def test_device_loop_against_the_host_loop(name):
    """guess_mode 1, the obstacle predicted per stage (frozen in one case), Lt = L (1 in two cases), noise mode 2 in two cases: traj, ctrl and clearance
    within 1e-9 of the numpy host loop over mpc_forces_solve_batch, flags equal, every ego up to and including its first failed step.  N = 7 with 37
    egos is 259 stage threads (past the 64, 128 and 256 marks); N <= 4 with 130 egos is every mapping of k_forces_qp with 64 and 32 instances per
    workgroup.  At least 3/4 of the egos keep exitflag 1 throughout in the host loop."""
    N, B, init, path, orient, vdes, track, predict, seed = case_inputs(name)
    L, _ = ref.run_length(N)
    s = _solver(N)
    noise = dict(noise_mode=0 if seed is None else 2, sigma=0.0 if seed is None else 0.05, seed=seed or 0)
    traj, ctrl, flag, cl = s.forces_closed_loop_obst(init, path, orient, vdes, L, *BOUNDS, obst_track=track, obst_offset=ref.OBST_OFFSET, predict=predict,
                                                     guess_mode=1, r_sum=ref.R_SUM, **noise)
    want = ref.host_loop(ref.backend_solver(s), init, path, orient, vdes, L, N, track=track, predict=predict, guess_mode=1, seed=seed, sigma=noise["sigma"])
    clean = np.all(want["flag"] == 1, axis=1)
    m = compared_steps(want["flag"])
    d = {k: np.abs(got - want[k])[m].max() for k, got in (("traj", traj), ("ctrl", ctrl), ("clearance", cl))}
    print(name, f"egos with every exitflag 1 in the host loop: {int(clean.sum())} of {B}; over steps 0..39: {int(np.all(want['flag'][:, :ref.STEPS] == 1, axis=1).sum())};",
          {k: f"{v:.2e}" for k, v in d.items()}, "min clearance", cl[m].min())
    assert clean.sum() >= 0.75 * B
    assert np.array_equal(flag[m], want["flag"][m])
    assert max(d.values()) <= 1e-9
    assert np.array_equal(traj[:, 0], init)


def test_behaviour_on_the_device():
    """the conditions of test_forces_loop_obst_cpu.check_behaviour on the device loop: overtake and parked, N = 10, steps 0..39 of L = 60"""
    s = _solver(10)

    def run(name, mode):
        sc = ref.scene(name)
        guess_mode, predict = ref.MODES[mode]
        traj, ctrl, flag, cl = s.forces_closed_loop_obst(sc["init"], sc["path"], sc["orient"], sc["vdes"], sc["L"], *BOUNDS, obst_track=sc["track"],
                                                         obst_offset=ref.OBST_OFFSET, predict=predict, guess_mode=guess_mode, r_sum=ref.R_SUM)
        return {k: v[:, :ref.STEPS] for k, v in dict(traj=traj, ctrl=ctrl, flag=flag, clearance=cl).items()}

    check_behaviour(run)


def test_refusals():
    """MPC_ERR_INVALID with a message: Lt = 2 < L; Lt = 0 with predict 1 or with a clearance buffer; six states"""
    N, L = 10, 30
    s = _solver(N)
    init, path, orient, vdes = ref.ego_inputs(2, N, 10.0)
    args = (init, path, orient, vdes, L) + BOUNDS
    with pytest.raises(pkg.MpcError) as e:
        s.forces_closed_loop_obst(*args, obst_track=np.zeros((2, 2, 3)))
    assert e.value.code == abi.MPC_ERR_INVALID and "Lt = 1 (the obstacle stands still) or Lt >= L" in str(e.value)
    with pytest.raises(pkg.MpcError) as e:
        s.forces_closed_loop_obst(*args, predict=True)
    assert e.value.code == abi.MPC_ERR_INVALID and "predict needs obst_track" in str(e.value)
    with pytest.raises(pkg.MpcError) as e:
        s.forces_closed_loop_obst(*args, clearance=True)
    assert e.value.code == abi.MPC_ERR_INVALID and "clearance needs obst_track" in str(e.value)
    with pytest.raises(pkg.MpcError) as e:
        _solver(N, nx=6).forces_closed_loop_obst(*args, obst_track=np.zeros((2, 1, 3)))
    assert e.value.code == abi.MPC_ERR_INVALID and "the FORCES formulation has 5 states" in str(e.value)
    assert len(s.forces_closed_loop_obst(*args, obst_track=np.tile([50.0, -8.0, 0.0], (2, 1)))) == 4          # (the handle still works)


def test_forcespro_optimizer_device_loop_against_its_host_loop():
    """ForcesproOptimizer with obstacle_track, predict_obstacle and guess_mode = 1 on the overtake scene: the device loop (mpc_forces_closed_loop_batch_obst)
    against its step-by-step host loop (runtime_parameters with per-stage centres, a refreshed problem["x0"]) at 1e-9, exitflags equal and returned
    in `exitflags`, not asserted"""
    opt = __import__("importlib").import_module(pkg.__name__ + ".optimizer")
    N = 10
    sc = ref.scene("overtake", N)
    L = sc["L"]
    obstacle = dict(position_x=15.0, position_y=-2.5, length=6.0, width=3.5, orientation=0.0)
    outs = []
    for device_loop in (True, False):
        conf = make_configuration(sc["path"][0, :L], sc["orient"][0, :L], 10.0, WEIGHTS_YAML_ZAM_LF, obstacle=obstacle, use_case="collision_avoidance")
        o = opt.ForcesproOptimizer(configuration=conf, init_values=(np.array([0.0, 0.0]), 10.0, 0.0, 0.0), predict_horizon=N, guess_mode=1,
                                   obstacle_track=sc["track"][0], predict_obstacle=True)
        o.use_device_loop = device_loop
        outs.append(o.optimize() + (o.exitflags, o.clearance))
    print("exitflags != 1:", int((outs[1][3] != 1).sum()), "|traj|", np.abs(outs[0][0] - outs[1][0]).max(), "|ctrl|", np.abs(outs[0][1] - outs[1][1]).max())
    assert np.array_equal(outs[0][3], outs[1][3]) and outs[0][3].shape == (L,)
    assert np.abs(outs[0][0] - outs[1][0]).max() < 1e-9 and np.abs(outs[0][1] - outs[1][1]).max() < 1e-9
    assert np.all(outs[0][3][:ref.STEPS] == 1)
    assert outs[1][4] is None and outs[0][4].shape == (L,) and outs[0][4][:ref.STEPS].min() >= -1e-3       # (the device loop reports the clearance too)
