"""GPU: the closed loop stepped from outside (mpc_session_*: k_session_ingest and k_session_traffic in front of the unchanged solve, k_loop_advance and
k_session_emit behind it).  Scenes: tests/loop_obst_ref.py (N = 10, L = 40) and the batches of tests/test_gpu_loop_traffic.py; numpy restatement and the
step-by-step host loop: tests/session_ref.py."""
import ctypes as C

import numpy as np
import pytest

import loop_obst_ref as lref
import session_ref as sref
import test_gpu_loop_traffic as tl
import traffic_ref as tref
from helpers import WEIGHTS_ZAM_CA, NLPConfig, abi, make_solver, pkg, set_cfg_bounds, straight_path, synthetic_batch

pytestmark = pytest.mark.gpu

N, L, DT = lref.N, lref.L, lref.DT
TOL_HOST = 1e-6            # the device loop against a step-by-step host loop: the project's bound (tests/test_gpu_loop_traffic.py)
EGO_OFFSET, R_SUM = lref.CFG.ego_offset, lref.CFG.r_sum
CFG6 = NLPConfig(N=N, nx=6, obstacle=(lref.AHEAD, lref.LATERAL[0], lref.OBST_LW[0], lref.OBST_LW[1], 0.0), **WEIGHTS_ZAM_CA)

_solvers, _plain = {}, {}


def solver(nx=5):
    if nx not in _solvers:
        cfg = lref.CFG if nx == 5 else CFG6
        _solvers[nx] = make_solver(cfg)
        set_cfg_bounds(_solvers[nx], cfg)
    return _solvers[nx]


def plain(B, nx):
    """(inputs, the plain loop on them: traj, ctrl, step_status), computed once per (B, nx)"""
    if (B, nx) not in _plain:
        inputs = tl.one_obstacle_batch(B)[:4]
        out = solver(nx).closed_loop(*inputs, L)
        for a in out:
            a.setflags(write=False)
        _plain[B, nx] = (inputs, out)
    return _plain[B, nx]


def same(got, want):
    return all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, want))


@pytest.mark.parametrize("nx", [5, 6])
@pytest.mark.parametrize("B", [10, 130])
def test_lane_following_is_the_plain_loop(B, nx):
    """(a) M = 0, measured None: every step's u is ctrl[:, i] of closed_loop(...) and the record is its traj, ctrl and step_status bit for bit; the rows of
    steps not yet taken are NaN / 0; plan and status are the solve's"""
    s = solver(nx)
    inputs, want = plain(B, nx)
    with s.session(*inputs, L) as sess:
        assert sess.steps_done == 0
        for i in range(L):
            if i == 3:
                traj, ctrl, st = sess.record()
                assert same((traj[:, :3], ctrl[:, :3], st[:, :3]), [w[:, :3] for w in want])
                assert np.isnan(traj[:, 3:]).all() and np.isnan(ctrl[:, 3:]).all() and np.all(st[:, 3:] == 0)
            u, plan, status = sess.step(outputs=("plan", "status"))
            assert np.array_equal(u, want[1][:, i]) and np.array_equal(plan[:, :2], u) and np.array_equal(status, want[2][:, i]), i
        assert sess.steps_done == L and same(sess.record(), want)
    assert s._lib.mpc_session_steps_done(s._h) == -1


@pytest.mark.parametrize("B,nx", [(10, 5), (10, 6), (130, 5)])
def test_external_plant_that_is_the_model(B, nx):
    """(b) measured = plant_step(state, u, "euler") after every step, which tests/test_gpu_descriptor.py holds to the loop's own step bit for bit: the bits
    of (a).  Replay: the recorded traj[:, i] of (a) fed back gives its ctrl.  Dropped measurements: NaN rows for a third of the egos on every other step
    change nothing"""
    s = solver(nx)
    inputs, want = plain(B, nx)
    with s.session(*inputs, L) as sess:
        x = np.zeros((B, nx))
        x[:, :5] = inputs[0]
        measured = None
        for i in range(L):
            u = sess.step(measured)
            x = s.plant_step(np.where(np.arange(nx) < 5, x, 0.0), u, "euler")          # (between two steps: another entry point of the handle)
            measured = np.ascontiguousarray(x[:, :5])
        assert same(sess.record(), want)
    with s.session(*inputs, L) as sess:
        for i in range(L):
            assert np.array_equal(sess.step(None if i == 0 else want[0][:, i]), want[1][:, i]), i
        assert same(sess.record(), want)
    with s.session(*inputs, L) as sess:
        for i in range(L):
            measured = None
            if i > 0:
                measured = want[0][:, i].copy()
                if i % 2:
                    measured[i % 3::3] = np.nan
            sess.step(measured)
        assert same(sess.record(), want)


def standing(B, six):
    """(inputs, tracks [B, M, 1, 3], offsets [B, M]): the first pose of every obstacle of the one-obstacle batch (M = 1), or of the six-obstacle decoy /
    absent set of tests/test_gpu_loop_traffic.py (four beyond 1000 m, the real one at m = 2, m = 3 absent)"""
    init, path, orient, vdes, tr = tl.one_obstacle_batch(B)
    if not six:
        return (init, path, orient, vdes), np.ascontiguousarray(tr[:, None, :1]), np.full((B, 1), lref.OFFSET)
    rng = np.random.default_rng(3)
    far = np.stack([rng.uniform(1500.0, 3000.0, (B, 4, 1)) * rng.choice([-1.0, 1.0], (B, 4, 1)), rng.uniform(1500.0, 3000.0, (B, 4, 1)),
                    rng.uniform(-3.0, 3.0, (B, 4, 1))], axis=3)
    tracks = np.ascontiguousarray(np.concatenate([far[:, :2], tr[:, None, :1], np.full((B, 1, 1, 3), np.nan), far[:, 2:]], axis=1))
    offsets = np.ascontiguousarray(rng.uniform(0.5, 1.5, (B, 6)))
    offsets[:, 2] = lref.OFFSET
    return (init, path, orient, vdes), tracks, offsets


def run_session(s, inputs, offsets, pairing, observe, measure=None, steps=L):
    """a session driven for `steps` steps, measure(i, x [B, 5], u [B, 2]) -> the measured states of step i + 1 (None: the model's): (traj, ctrl, step_status, clearance [B, steps], nearest [B, steps], chosen [B, steps, N+1, 3], plan [steps, B, n_w])"""
    cl, near, chosen, plans = [], [], [], []
    with s.session(*inputs, L, offsets=offsets, pairing=pairing) as sess:
        x = np.atleast_2d(np.asarray(inputs[0], dtype=np.float64))
        for i in range(steps):
            u, plan, c, n, ch = sess.step(None if i == 0 or measure is None else x, observe(i), outputs=("plan", "clearance", "nearest", "chosen"))
            cl.append(c), near.append(n), chosen.append(ch), plans.append(plan)
            if measure is not None:
                x = np.ascontiguousarray(measure(i, x, u))
        rec = sess.record()
    return (*rec, np.stack(cl, 1), np.stack(near, 1), np.stack(chosen, 1), np.array(plans))


@pytest.mark.parametrize("B,six", [(10, False), (10, True), (130, False)])
def test_standing_obstacles_are_the_traffic_loop(B, six):
    """(c) vx = vy = 0: traj, ctrl, step_status, clearance, nearest and chosen are those of closed_loop_traffic with Lt = 1 bit for bit -- one obstacle and
    the six-obstacle decoy / absent set, both pairings, obstacles per ego and (ego 0's) shared by all"""
    s = solver()
    inputs, tracks, offsets = standing(B, six)
    for pairing in (0, 1):
        for tr, off in ((tracks, offsets), (tracks[0], offsets[0])):
            want = s.closed_loop_traffic(*inputs, L, tr, off, pairing=pairing)
            obs = np.ascontiguousarray(np.concatenate([tr[..., 0, :], np.zeros(tr.shape[:-2] + (2,))], axis=-1))
            got = run_session(s, inputs, off, pairing, lambda i: obs)
            for name, a, b in zip(("traj", "ctrl", "status", "clearance", "nearest", "chosen"), got, want):
                assert np.array_equal(a, b), (name, pairing, tr.ndim)
            assert np.all(got[4] == (2 if six else 0)) and (tr.ndim == 3 or np.abs(got[0][:, :, 1]).max() > 0.3)      # (per ego: the obstacles were seen)


@pytest.mark.parametrize("B,pairing", [(10, 0), (130, 0), (10, 1)])
def test_constant_velocity_obstacles(B, pairing):
    """(d) the drifting obstacles of one_obstacle_batch move at constant velocity: the session that is shown (pose at step i, velocity) against
    closed_loop_traffic on the track itself, extended to L + N rows so that no horizon runs past it.  The two see the same poses up to the rounding of
    x + (k dt) v against the track's own rows: traj and ctrl within 1e-6, step_status equal and all 1, chosen and nearest equal, clearance numpy's to
    1e-12.  The plant is the model's, so the state before every step was held clear by the solve before it: >= -1e-6 in the measure the pairing's NLP
    holds, as tests/test_gpu_loop_traffic.py has it -- with pairing 1 the session's own nine-pair clearance, with pairing 0 the three pairs (j, j) the
    reference's NLP constrains (numpy on the returned trajectory; its cross pairs are free: the nine-pair clearance goes down to -0.57 m, in the loop on
    the track as in the session).  Pairing 0 is the predicted loop, which has 0 failures on these scenes; with pairing 1 the ten scenes converge on every
    step, B = 130 does not (3 steps of 5200 end with status -7 in the loop on the track, and in the session), so it is not a case.
    Observed: |dtraj| <= 5.2e-8, |dctrl| <= 4.4e-7, |clearance - numpy| <= 7.2e-15, min clearance in the pairing's measure -3.3e-8"""
    s = solver()
    init, path, orient, vdes, tr = tl.one_obstacle_batch(B)
    vel = (tr[:, 1, :2] - tr[:, 0, :2]) / DT
    k = np.arange(L + N)
    track = np.concatenate([tr[:, :1, :2] + (k * DT)[None, :, None] * vel[:, None, :], np.broadcast_to(tr[:, :1, 2:], (B, L + N, 1))], axis=2)
    assert np.abs(track[:, :tr.shape[1]] - tr).max() < 1e-12
    offsets = np.full((B, 1), lref.OFFSET)
    want = s.closed_loop_traffic(init, path, orient, vdes, L, np.ascontiguousarray(track[:, None]), offsets, pairing=pairing)
    observe = lambda i: np.ascontiguousarray(np.concatenate([track[:, i], vel], axis=1)[:, None])          # noqa: E731   [B, 1, 5]
    traj, ctrl, st, cl, near, chosen, _ = run_session(s, (init, path, orient, vdes), offsets, pairing, observe)
    held = cl if pairing == 1 else lref.clearance_numpy(traj, tref.centres(track[:, :L], lref.OFFSET).reshape(B, L, 6), EGO_OFFSET, R_SUM)
    w_cl = np.stack([sref.clearance(traj[:, i], observe(i), offsets, EGO_OFFSET, R_SUM)[0] for i in range(L)], 1)
    print(f"B = {B}, pairing {pairing}: |dtraj| {np.abs(traj - want[0]).max():.3e} |dctrl| {np.abs(ctrl - want[1]).max():.3e}; steps with status != 1: {int((st != 1).sum())} "
          f"(track loop: {int((want[2] != 1).sum())}); |clearance - numpy| {np.abs(cl - w_cl).max():.3e}; min clearance {cl.min():.3e}, in the pairing's measure {held.min():.3e}")
    assert np.abs(traj - want[0]).max() < TOL_HOST and np.abs(ctrl - want[1]).max() < TOL_HOST
    assert np.array_equal(st, want[2]) and np.all(st == 1)
    assert np.array_equal(chosen, want[5]) and np.array_equal(near, want[4]) and np.all(near == 0)
    assert np.abs(cl - w_cl).max() <= 1e-12 and held.min() >= -1e-6 and np.abs(cl - want[3]).max() < TOL_HOST
    assert np.abs(traj[:, :, 1]).max() > 0.3


def test_braking_obstacle_and_an_rk4_plant():
    """(e) what no existing loop can express (tests/session_ref.py: the obstacle ahead halves its speed at step 15, the plant integrates with RK4, all
    L = 40 steps): the session against the step-by-step host loop -- shift / warm_start / reference window of CasadiOptimizer,
    nearest_obstacle_centres on the extrapolated poses, solve(obst=[B, N+1, 6]), plant_step -- to 1e-6, traj, ctrl and every plan; the host loop's
    status 1 on every step; and the observation is read: once the obstacle has braked, the plan differs by more than 1e-3 m from that of a session
    whose observations keep reporting the old speed.
    Observed: |dtraj| 2.7e-23, |dctrl| 2.2e-22, |dplan| 6.4e-22; the ego swerves 0.236 m; the plans 0.48 m apart from step 15 on, 0 before"""
    s, host = solver(), make_solver(lref.CFG)
    set_cfg_bounds(host, lref.CFG)
    path, orient = straight_path(L, 0.0, 0.0, 0.0, lref.V_EGO)
    inputs = (np.array([[0.0, 0.0, 0.0, lref.V_EGO, 0.0]]), path[None], orient[None], np.array([lref.V_EGO]))
    offsets = np.array([lref.OFFSET])
    plant = lambda i, x, u: host.plant_step(x, u, "rk4")          # noqa: E731
    want = sref.host_loop(host, *inputs, L, N, DT, observe=sref.braking_obs, offsets=offsets, ego_offset=EGO_OFFSET, desc_obst=lref.CFG.obstacle_centers.ravel(),
                          plant=plant)
    traj, ctrl, st, cl, near, chosen, plans = run_session(s, inputs, offsets, 0, sref.braking_obs, plant)
    blind = run_session(s, inputs, offsets, 0, lambda i: sref.braking_obs(i, knows=False), plant)
    d_traj, d_ctrl, d_plan = np.abs(traj - want["traj"]).max(), np.abs(ctrl - want["ctrl"]).max(), np.abs(plans - want["plan"]).max()
    xy = lambda p: p[:, 0, 2 * N:].reshape(L, N + 1, 5)[:, :, :2]          # noqa: E731
    apart = np.abs(xy(plans) - xy(blind[6])).max(axis=(1, 2))
    print(f"session vs host loop |dtraj| {d_traj:.3e} |dctrl| {d_ctrl:.3e} |dplan| {d_plan:.3e}; host status != 1 on {int((want['status'] != 1).sum())} steps; largest "
          f"lateral move {np.abs(traj[0, :, 1]).max():.3f}; plans with / without the new speed apart by {apart[sref.BRAKE_AT:].max():.3e} m from step {sref.BRAKE_AT} on, "
          f"{apart[:sref.BRAKE_AT].max():.1e} before")
    assert np.all(want["status"] == 1) and np.array_equal(st, want["status"])
    assert d_traj < TOL_HOST and d_ctrl < TOL_HOST and d_plan < TOL_HOST
    assert np.array_equal(chosen[0], want["chosen"][:, 0]) and np.all(near == 0)
    assert apart[sref.BRAKE_AT:].max() > 1e-3 and apart[:sref.BRAKE_AT].max() == 0.0
    assert np.abs(traj[0, :, 1]).max() > 0.1                              # (the ego swerved under the external plant)
    host.close()


@pytest.mark.parametrize("traffic", [False, True])
def test_open_session_is_the_optimizers_device_loop(traffic):
    """CasadiOptimizer.open_session() stepped with measured None against optimize() on the same configuration, bit for bit: lane following, and through
    the two standing obstacles of scene S (tests/traffic_ref.py; L = 40 passes the first) -- optimize() is given their tracks and sizes, the session's
    configuration the sizes alone, and the obstacles are observed with zero velocity"""
    from helpers import WEIGHTS_YAML_ZAM_LF, make_configuration
    path, orient = straight_path(L, 0.0, 0.0, 0.0, lref.V_EGO)
    first = tref.S_TRACKS[0, 0]

    def optimiser(tracks):
        conf = make_configuration(path, orient, lref.V_EGO, WEIGHTS_YAML_ZAM_LF, use_case="collision_avoidance",
                                  obstacle=dict(position_x=first[0], position_y=first[1], length=lref.OBST_LW[0], width=lref.OBST_LW[1], orientation=first[2]))
        if traffic:
            conf.obstacle_sizes, conf.obstacle_pairing = np.tile(lref.OBST_LW, (2, 1)), 1
            if tracks:
                conf.obstacle_tracks = tref.S_TRACKS
        return lref.opt.CasadiOptimizer(configuration=conf, init_values=(np.array([0.0, 0.0]), lref.V_EGO, 0.0, 0.0), predict_horizon=N)

    loop = optimiser(True)
    states, controls, _ = loop.optimize()
    o = optimiser(False)
    obs = np.concatenate([tref.S_TRACKS[:, 0], np.zeros((2, 2))], axis=1) if traffic else None
    chosen = []
    with o.open_session() as sess:
        assert (sess.M, sess.per_ego) == ((2, 0) if traffic else (0, 0))
        for i in range(L):
            if traffic:
                u, ch = sess.step(obstacles=obs, outputs=("chosen",))
                chosen.append(ch[0])
            else:
                u = sess.step()
            assert np.array_equal(u[0], controls[i]), i
        traj, ctrl, st = sess.record()
    assert np.array_equal(traj[0], states) and np.array_equal(ctrl[0], controls) and np.array_equal(st[0], loop.solver()[0].stats()["status"])
    if traffic:
        assert np.array_equal(np.array(chosen), loop.chosen) and np.abs(states[:, 1]).max() > 0.3 and set(np.unique(loop.chosen)) == {0, 1}
    loop.solver()[0]._backend.close(), o.solver()[0]._backend.close()


def test_live_retuning_and_unrelated_calls_between_steps():
    """(f) set_weights at step 10: steps 0..9 are bit-equal to the untouched run, from step 10 on the session follows the host loop that does the same, to
    1e-6 (and has left the untouched run).  An unrelated solve() of another batch size, a plain loop of another batch size and a sensitivity solve between
    every two steps leave the session's bits unchanged.
    Observed: |dtraj| 7.1e-15, |dctrl| 8.9e-15 against the host loop; 0.73 away from the untouched run"""
    s, host = make_solver(lref.CFG), make_solver(lref.CFG)
    set_cfg_bounds(s, lref.CFG), set_cfg_bounds(host, lref.CFG)
    B, at = 3, 10
    path, orient = straight_path(L, 0.0, 0.0, 0.0, lref.V_EGO)
    init = np.tile([0.0, 0.0, 0.0, lref.V_EGO, 0.0], (B, 1))
    init[:, 1] = [0.3, 0.2, 0.1]                                       # (beside the path, on the far side of the descriptor's obstacle)
    inputs = (init, np.tile(path, (B, 1, 1)), np.tile(orient, (B, 1)), np.full(B, lref.V_EGO))
    w0 = s.weights
    Q1, R1 = w0[:5] * [4.0, 0.25, 1.0, 2.0, 1.0], w0[5:] * [0.5, 3.0]

    def run(retune, busy):
        s.set_weights(w0[:5], w0[5:])
        with s.session(*inputs, L) as sess:
            for i in range(L):
                if retune and i == at:
                    s.set_weights(Q1, R1)
                sess.step()
                if busy:
                    x0, p = synthetic_batch(lref.CFG, 7 + i % 2)
                    s.solve(x0, p, lam_p=(i % 4 == 0))
                    if i % 8 == 0:
                        s.closed_loop(*plain(10, 5)[0], N)
            return sess.record()

    base, tuned, busy = run(False, False), run(True, False), run(False, True)
    assert same(busy, base)
    assert same([a[:, :at] for a in tuned], [a[:, :at] for a in base])
    want = sref.host_loop(host, *inputs, L, N, DT, before_step=lambda i: host.set_weights(Q1, R1) if i == at else None)
    d_traj, d_ctrl = np.abs(tuned[0] - want["traj"]).max(), np.abs(tuned[1] - want["ctrl"]).max()
    print(f"retuned at step {at}: session vs host loop |dtraj| {d_traj:.3e} |dctrl| {d_ctrl:.3e}; away from the untouched run by {np.abs(tuned[1] - base[1]).max():.3e}")
    assert d_traj < TOL_HOST and d_ctrl < TOL_HOST and np.array_equal(tuned[2], want["status"]) and np.all(tuned[2] == 1)
    assert np.abs(tuned[1][:, at:] - base[1][:, at:]).max() > 1e-3
    s.close(), host.close()


def test_refusals_and_the_device_form():
    """(g) every refusal of include/mpcgpu.h returns its code and leaves a message; end followed by begin works again; the device-pointer forms give the
    bits of the host forms.  (Bounds not set -> MPC_ERR_STATE is begin_solve's check, shared with every solve; mpc_create installs the reference's bounds,
    so no live handle reaches it.)"""
    import torch
    s = make_solver(lref.CFG)
    set_cfg_bounds(s, lref.CFG)
    lib, h = s._lib, s._h
    dp, ip = abi.as_dp, abi.as_ip
    B, Ls = 10, N                                                      # (a session of L = N steps: step L + 1 is the eleventh)
    init, path, orient, vdes, tr = tl.one_obstacle_batch(B)
    vd = np.ascontiguousarray(vdes, dtype=np.float64)
    offsets = np.full((B, 2), lref.OFFSET)
    obs = np.ascontiguousarray(np.concatenate([np.stack([tr[:, 0], tr[:, 0] + [0.0, 40.0, 0.0]], 1), np.zeros((B, 2, 2))], axis=2))
    u, traj, ctrl, st = np.empty((B, 2)), np.empty((B, Ls, 5)), np.empty((B, Ls, 2)), np.empty((B, Ls), np.int32)

    def refused(rc, code, word):
        msg = lib.mpc_last_error(h)
        assert rc == code and msg and word in msg, (rc, msg)

    def begin(B=B, L=Ls, Lp=L, init=init, path=path, M=2, per_ego=1, offsets=offsets, pairing=0):
        return lib.mpc_session_begin(h, B, L, Lp, dp(init), dp(path), dp(orient), dp(vd), M, per_ego, dp(offsets), pairing)

    # no session is open
    assert lib.mpc_session_steps_done(h) == -1
    refused(lib.mpc_session_step(h, None, dp(obs), dp(u), None, None, None, None, None), abi.MPC_ERR_STATE, b"no session")
    refused(lib.mpc_session_record(h, dp(traj), dp(ctrl), ip(st)), abi.MPC_ERR_STATE, b"no session")
    refused(lib.mpc_session_end(h), abi.MPC_ERR_STATE, b"no session")
    refused(lib.mpc_session_step_dev(h, None, None, None, None, None, None, None, None, None), abi.MPC_ERR_STATE, b"no session")
    refused(lib.mpc_session_record_dev(h, None, None, None, None), abi.MPC_ERR_STATE, b"no session")
    # begin
    bad_off, nan_off = offsets.copy(), offsets.copy()
    bad_off[7, 1], nan_off[0, 0] = np.inf, np.nan
    for kw, word in ((dict(M=-1), b"M >= 0"), (dict(offsets=None), b"offsets"), (dict(offsets=bad_off), b"finite"), (dict(offsets=nan_off), b"finite"),
                     (dict(pairing=2), b"pairing"), (dict(pairing=-1), b"pairing"), (dict(per_ego=2), b"per_ego"), (dict(per_ego=-1), b"per_ego"),
                     (dict(B=0), b"B > 0"), (dict(L=N - 1), b"L >= N"), (dict(L=L, Lp=L - 1), b"Lp >= L"), (dict(init=None), b"init_state"), (dict(path=None), b"path")):
        refused(begin(**kw), abi.MPC_ERR_INVALID, word)
        assert lib.mpc_session_steps_done(h) == -1, kw
    assert begin() == abi.MPC_OK and lib.mpc_session_steps_done(h) == 0
    refused(begin(), abi.MPC_ERR_STATE, b"is open")
    refused(begin(M=0, offsets=None), abi.MPC_ERR_STATE, b"is open")
    # step
    measured = np.ascontiguousarray(init)
    refused(lib.mpc_session_step(h, dp(measured), dp(obs), dp(u), None, None, None, None, None), abi.MPC_ERR_INVALID, b"step 0")
    refused(lib.mpc_session_step(h, None, dp(obs), None, None, None, None, None, None), abi.MPC_ERR_INVALID, b"u [B, 2]")
    refused(lib.mpc_session_step(h, None, None, dp(u), None, None, None, None, None), abi.MPC_ERR_INVALID, b"obs")
    assert lib.mpc_session_steps_done(h) == 0
    host_u = []
    for i in range(Ls):
        assert lib.mpc_session_step(h, None, dp(obs), dp(u), None, None, None, None, None) == abi.MPC_OK and lib.mpc_session_steps_done(h) == i + 1
        host_u.append(u.copy())
    refused(lib.mpc_session_step(h, None, dp(obs), dp(u), None, None, None, None, None), abi.MPC_ERR_STATE, b"all L steps")
    assert lib.mpc_session_record(h, dp(traj), dp(ctrl), ip(st)) == abi.MPC_OK and np.array_equal(ctrl, np.stack(host_u, 1))
    # end, and begin works again: lane following, which takes no obstacle outputs
    assert lib.mpc_session_end(h) == abi.MPC_OK and lib.mpc_session_steps_done(h) == -1
    assert begin(M=0, offsets=None) == abi.MPC_OK
    cl = np.empty(B)
    refused(lib.mpc_session_step(h, None, None, dp(u), None, None, dp(cl), None, None), abi.MPC_ERR_INVALID, b"M > 0")
    assert lib.mpc_session_step(h, None, None, dp(u), None, None, None, None, None) == abi.MPC_OK
    assert lib.mpc_session_end(h) == abi.MPC_OK
    # the device-pointer forms: the bits of the host forms
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (init, path, orient, vd, offsets, obs)]
    o_u, o_plan = torch.empty((B, 2), dtype=torch.float64, device="cuda"), torch.empty((B, s.n_w), dtype=torch.float64, device="cuda")
    o_traj, o_ctrl = (torch.empty(sh, dtype=torch.float64, device="cuda") for sh in ((B, Ls, 5), (B, Ls, 2)))
    o_st = torch.empty((B, Ls), dtype=torch.int32, device="cuda")
    vp = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731
    assert lib.mpc_session_begin_dev(h, B, Ls, L, vp(d[0]), vp(d[1]), vp(d[2]), vp(d[3]), 2, 1, vp(d[4]), 0, None) == abi.MPC_OK
    d[1].zero_(), d[4].zero_()                                          # (begin has copied what it was given)
    sess = object.__new__(pkg.LoopSession)
    sess._s, sess._open = s, True
    for i in range(Ls):
        sess.step_device(o_u.data_ptr(), d_obs=d[5].data_ptr(), d_plan=o_plan.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(o_u.cpu().numpy(), host_u[i]) and np.array_equal(o_plan.cpu().numpy()[:, :2], host_u[i])
    assert lib.mpc_session_record_dev(h, vp(o_traj), vp(o_ctrl), vp(o_st), None) == abi.MPC_OK
    torch.cuda.synchronize()
    assert np.array_equal(o_traj.cpu().numpy(), traj) and np.array_equal(o_ctrl.cpu().numpy(), ctrl) and np.array_equal(o_st.cpu().numpy(), st)
    sess.close()
    # a snapshot does not outlive a step
    x0, p = synthetic_batch(lref.CFG, B)
    assert begin(M=0, offsets=None) == abi.MPC_OK
    s.solve(x0, p, lam_p=True)
    s.sens_adjoint(np.ones((B, s.n_w)))
    assert lib.mpc_session_step(h, None, None, dp(u), None, None, None, None, None) == abi.MPC_OK
    with pytest.raises(pkg.MpcError) as e:
        s.sens_adjoint(np.ones((B, s.n_w)))
    assert e.value.code == abi.MPC_ERR_STATE
    s.close()                                                           # (mpc_destroy releases the open session)
