"""GPU: the stepping session with a radius per obstacle (mpc_session_begin_sized) and with obstacle poses predicted by the caller
(mpc_session_step_pred): k_session_traffic_sized, k_session_pred and k_session_pred_sized in front of the unchanged solves.  Scenes: tests/loop_obst_ref.py
(N = 10, L = 40), the batches of tests/test_gpu_loop_traffic.py and scene S of tests/traffic_ref.py; the poses a caller would predict from a track and
the step-by-step host loop: tests/session_sized_ref.py."""
import ctypes as C

import numpy as np
import pytest

import loop_obst_ref as lref
import session_ref as sref
import session_sized_ref as zs
import test_gpu_loop_traffic as tl
import test_gpu_loop_traffic_sized as tz
import test_gpu_session as ts
import traffic_ref as tref
from helpers import WEIGHTS_YAML_ZAM_LF, BicycleNLP, abi, make_configuration, make_solver, pkg, set_cfg_bounds, straight_path

pytestmark = pytest.mark.gpu

N, L, DT = lref.N, lref.L, lref.DT
TOL_HOST = 1e-6            # two loops that differ by rounding: the project's bound (tests/test_gpu_session.py, tests/test_gpu_loop_traffic.py)
EGO_OFFSET, R_SUM = lref.CFG.ego_offset, lref.CFG.r_sum
OUT = ("plan", "status", "clearance", "nearest", "chosen")
NAMES = ("traj", "ctrl", "step_status", "u", "plan", "status", "clearance", "nearest", "chosen")
solver = ts.solver          # one handle per nx, the bounds of its configuration set


def run(s, inputs, offsets, pairing, feed, rsums=None, feedback=False, steps=L, length=L):
    """a session of `length` steps driven for `steps` of them; feed(i) -> the obstacle keywords of step i, dict(obstacles=) or dict(predicted=); feedback: measured =
    plant_step(x, u, "euler") of the step before, else None.  -> the arrays of NAMES: the record, then u [B, steps, 2], plan [B, steps, n_w],
    status / clearance / nearest [B, steps], chosen [B, steps, N+1, 3] of the steps"""
    log = [[] for _ in range(1 + len(OUT))]
    B = len(inputs[0])
    with s.session(*inputs, length, offsets=offsets, pairing=pairing, rsums=rsums) as sess:
        assert sess.sized == (rsums is not None)
        x = np.zeros((B, s.nx))
        x[:, :5] = inputs[0]
        measured = None
        for i in range(steps):
            got = sess.step(measured, outputs=OUT, **feed(i))
            for q, v in zip(log, got):
                q.append(v)
            if feedback:
                x = s.plant_step(np.where(np.arange(s.nx) < 5, x, 0.0), got[0], "euler")
                measured = np.ascontiguousarray(x[:, :5])
        rec = sess.record()
    return (*rec, *(np.stack(q, 1) for q in log))


def assert_same(got, want, what, names=NAMES):
    for name, a, b in zip(names, got, want):
        assert np.array_equal(a, b, equal_nan=True), (what, name)


def against_loop(run_out, loop_out, what):
    """the record, clearance, nearest and chosen of a session against (traj, ctrl, step_status, clearance, nearest, chosen) of a loop"""
    assert_same(run_out[:3] + run_out[6:], loop_out, what, NAMES[:3] + NAMES[6:])
    assert np.array_equal(run_out[3], loop_out[1]) and np.array_equal(run_out[5], loop_out[2]), what      # (every step's u and status are the record's)


def mirrored(B):
    """(inputs, tracks [B, 2, Lt, 3], offsets [B, 2]): the batch's own obstacle and its mirror image across the path
    (tests/test_gpu_loop_traffic_sized.py)"""
    init, path, orient, vdes, tr = tl.one_obstacle_batch(B)
    tracks = np.ascontiguousarray(np.stack([tr, tr * np.array([1.0, -1.0, -1.0])], axis=1))
    return (init, path, orient, vdes), tracks, np.full((B, 2), lref.OFFSET)


def mixed_rsums(shape):
    """the batch's own obstacle at the handle's radius, its mirror image 0.7 m smaller"""
    rs = np.full(shape, R_SUM)
    rs[..., 1] = R_SUM - 0.7
    return rs


def standing_obs(tracks):
    """tracks [.., M, Lt, 3] -> obs [.., M, 5]: the first pose, velocity 0"""
    return np.ascontiguousarray(np.concatenate([tracks[..., 0, :], np.zeros(tracks.shape[:-2] + (2,))], axis=-1))


# ---- (a) -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,nx,scene", [(10, 5, "six"), (10, 5, "moving"), (130, 5, "six"), (130, 5, "moving"), (10, 6, "moving")])
def test_equal_radii_are_the_plain_session(B, nx, scene):
    """(a) session(rsums = R_SUM everywhere) against session(): u, plan, status, clearance, nearest, chosen of every step and the record bit for bit --
    on the six-obstacle decoy / absent set of tests/test_gpu_session.py (standing) and on the moving one-obstacle batch, whose observed velocities
    are the finite differences of its track; both pairings"""
    s = solver(nx)
    if scene == "six":
        inputs, tracks, offsets = ts.standing(B, True)
        obs = standing_obs(tracks)
        feed = lambda i: dict(obstacles=obs)          # noqa: E731
    else:
        init, path, orient, vdes, tr = tl.one_obstacle_batch(B)
        inputs, offsets = (init, path, orient, vdes), np.full((B, 1), lref.OFFSET)
        feed = lambda i: dict(obstacles=zs.observed(tr[:, None], i, DT))          # noqa: E731
    for pairing in (0, 1):
        plain = run(s, inputs, offsets, pairing, feed)
        sized = run(s, inputs, offsets, pairing, feed, rsums=np.full(offsets.shape, R_SUM))
        assert_same(sized, plain, (scene, pairing))
        assert (plain[2] == 1).mean() > 0.5 and np.all(plain[7] == (2 if scene == "six" else 0)) and np.abs(plain[0][:, :, 1]).max() > 0.3


# ---- (b) -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [10, 130])
def test_a_sized_session_is_the_sized_loop(B):
    """(b) measured None, two standing obstacles per ego -- the batch's own and its mirror image, radius sums 0.7 m apart --, per ego and ego 0's set
    shared by all, both pairings: the record, clearance, nearest and chosen are the bits of closed_loop_traffic(..., rsums=) with Lt = 1"""
    s = solver()
    inputs, tracks, offsets = mirrored(B)
    tracks = np.ascontiguousarray(tracks[:, :, :1])
    for pairing in (0, 1):
        for tk, of in ((tracks, offsets), (np.ascontiguousarray(tracks[0]), offsets[0])):
            rs = mixed_rsums(of.shape)
            want = s.closed_loop_traffic(*inputs, L, tk, of, pairing=pairing, rsums=rs)
            obs = standing_obs(tk)
            got = run(s, inputs, of, pairing, lambda i: dict(obstacles=obs), rsums=rs)
            against_loop(got, want, (pairing, tk.ndim))
            assert (want[2] == 1).mean() > 0.5


# ---- (c) -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,pairing,nx", [(10, 0, 5), (10, 1, 5), (130, 0, 5), (130, 1, 5), (10, 1, 6)])
def test_predicted_poses_are_the_loops_past_moving_tracks(B, pairing, nx):
    """(c) pred at step i = tracks[..., min(i + k, Lt - 1), :] with Lt = L (the last N steps clamp), the mirror image absent over rows 12 .. 15, so that
    some stages of a solve see it and others do not: a plain session gives the bits of closed_loop_traffic, a sized one those of
    closed_loop_traffic(rsums=) -- record, clearance, nearest, chosen; more than half of the statuses are 1 and chosen holds both obstacles; with
    measured = plant_step(x, u, "euler") fed back the bits are unchanged"""
    s = solver(nx)
    inputs, tracks, offsets = mirrored(B)
    tracks = np.ascontiguousarray(tracks[:, :, :L])
    tracks[:, 1, 12:16] = np.nan
    feed = lambda i: dict(predicted=zs.predicted(tracks, i, N))          # noqa: E731
    here = np.isfinite(feed(5)["predicted"][:, 1, :, 0])
    assert here.any(axis=1).all() and not here.all(axis=1).any()        # (step 5: the mirror image is there for stages 0 .. 6, away for 7 .. 10)
    for rs in (None, mixed_rsums(offsets.shape)):
        want = s.closed_loop_traffic(*inputs, L, tracks, offsets, pairing=pairing, **({} if rs is None else dict(rsums=rs)))
        got = run(s, inputs, offsets, pairing, feed, rsums=rs)
        against_loop(got, want, ("sized" if rs is not None else "plain", pairing))
        assert (want[2] == 1).mean() > 0.5 and set(np.unique(want[5])) >= {0, 1}
        fed = run(s, inputs, offsets, pairing, feed, rsums=rs, feedback=True)
        assert_same(fed, got, ("fed back", rs is not None, pairing))


# ---- (d) -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,sized,pairing", [(10, False, 0), (10, True, 1), (130, True, 0), (130, False, 1)])
def test_both_step_forms_in_one_session(B, sized, pairing):
    """(d) even steps step(obstacles=), odd steps step(predicted=).  Standing obstacles (the batch's own and its mirror image), each pose repeated over
    the stages: the bits of a session that used `obstacles` throughout.  Moving obstacles (the batch's own, observed with the finite differences of
    its track; pairing 0, the predicted loop, which converges on every step of these scenes -- tests/test_gpu_session.py (d)), predicted =
    session_ref.extrapolate(obs, N, DT): within TOL_HOST -- the device may fuse x + (k dt) v where numpy cannot"""
    s = solver()
    inputs, tracks, offsets = mirrored(B)
    rs = mixed_rsums(offsets.shape) if sized else None
    obs = standing_obs(tracks)
    repeated = sref.extrapolate(obs, N, DT)
    assert np.array_equal(repeated, np.repeat(tracks[:, :, :1], N + 1, axis=2))
    base = run(s, inputs, offsets, pairing, lambda i: dict(obstacles=obs), rsums=rs)
    both = run(s, inputs, offsets, pairing, lambda i: dict(obstacles=obs) if i % 2 == 0 else dict(predicted=repeated), rsums=rs)
    assert_same(both, base, (sized, pairing))
    assert (base[2] == 1).mean() > 0.5
    # moving
    one, off1 = np.ascontiguousarray(tracks[:, :1]), offsets[:, :1]
    rs1 = np.full((B, 1), R_SUM - 0.5) if sized else None
    observe = lambda i: zs.observed(one, i, DT)          # noqa: E731
    base = run(s, inputs, off1, 0, lambda i: dict(obstacles=observe(i)), rsums=rs1)
    both = run(s, inputs, off1, 0, lambda i: dict(obstacles=observe(i)) if i % 2 == 0 else dict(predicted=sref.extrapolate(observe(i), N, DT)), rsums=rs1)
    d_traj, d_ctrl = np.abs(both[0] - base[0]).max(), np.abs(both[1] - base[1]).max()
    print(f"B = {B}, sized {sized}: moving obstacles, alternating forms vs obstacles throughout |dtraj| {d_traj:.3e} |dctrl| {d_ctrl:.3e}; statuses that "
          f"differ: {int((both[2] != base[2]).sum())}, steps with status != 1: {int((base[2] != 1).sum())}")
    assert d_traj < TOL_HOST and d_ctrl < TOL_HOST
    assert np.abs(base[0][:, :, 1]).max() > 0.3                             # (the obstacles were seen)


# ---- (e) -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pairing", [0, 1])
def test_scene_s_with_a_small_a_and_a_large_b_through_open_session(pairing):
    """(e) scene S with the sizes of tests/test_gpu_loop_traffic_sized.py, obstacle_radii = "own": CasadiOptimizer.open_session() stepped with predicted
    poses built from S_TRACKS, measured None.  Every status 1; the record is optimize()'s device loop bit for bit; the clearance of every step
    against each obstacle's own radius, in the pairing's measure, >= -1e-6, and the session's own clearance is numpy's nine-pair value to 1e-12;
    the step-by-step host loop (sized_ref.select_sized on the predicted poses, one solve(obst=, rsum=) per step) within TOL_HOST"""
    Ls = tref.S_L
    sizes = (tz.SMALL_LW, lref.OBST_LW)
    path, orient = straight_path(Ls, 0.0, 0.0, 0.0, lref.V_EGO)
    first = tref.S_TRACKS[1, 0]

    def optimiser(tracks):
        conf = make_configuration(path, orient, lref.V_EGO, WEIGHTS_YAML_ZAM_LF, use_case="collision_avoidance", noised=False,
                                  obstacle=dict(position_x=first[0], position_y=first[1], length=lref.OBST_LW[0], width=lref.OBST_LW[1], orientation=first[2]))
        conf.obstacle_sizes, conf.obstacle_pairing, conf.obstacle_radii = np.asarray(sizes, dtype=np.float64), pairing, "own"
        if tracks:
            conf.obstacle_tracks = tref.S_TRACKS
        return lref.opt.CasadiOptimizer(configuration=conf, init_values=(np.array([0.0, 0.0]), lref.V_EGO, 0.0, 0.0), predict_horizon=N)

    loop = optimiser(True)
    states, controls, _ = loop.optimize()
    o = optimiser(False)                                                               # (no tracks: the caller predicts)
    rs, off = o.obstacle_rsums, o.obstacle_offsets
    assert rs[1] - rs[0] >= 0.5 and abs(rs[1] - R_SUM) < 1e-12
    predict = lambda i: zs.predicted(tref.S_TRACKS, i, N)          # noqa: E731
    cl, chosen = [], []
    with o.open_session() as sess:
        assert (sess.M, sess.per_ego, sess.sized) == (2, 0, True)
        for i in range(Ls):
            u, c, ch = sess.step(predicted=predict(i), outputs=("clearance", "chosen"))
            assert np.array_equal(u[0], controls[i]), i
            cl.append(c[0]), chosen.append(ch[0])
        traj, ctrl, st = sess.record()
    assert np.all(st == 1)
    assert np.array_equal(traj[0], states) and np.array_equal(ctrl[0], controls) and np.array_equal(st[0], loop.solver()[0].stats()["status"])
    assert np.array_equal(np.array(chosen), loop.chosen) and np.array_equal(np.array(cl), loop.clearance) and set(np.unique(loop.chosen)) == {0, 1}
    held = np.stack([tz._own_clearance(traj[0], tref.S_TRACKS[m, 0], off[m], rs[m], pairing == 1) for m in range(2)])
    nine = np.stack([tz._own_clearance(traj[0], tref.S_TRACKS[m, 0], off[m], rs[m], True) for m in range(2)])
    backend = o.solver()[0]._backend                                                   # (the bounds open_session() set are still the handle's)
    host = zs.host_loop_sized(backend, traj[0, 0], path, orient, lref.V_EGO, Ls, N, DT, predict, off, rs, R_SUM, pairing, o.ego_offset(),
                              np.array(o.obstacle_circles_centers_tuple, dtype=np.float64).ravel())
    d_traj, d_ctrl = np.abs(traj[0] - host["traj"]).max(), np.abs(ctrl[0] - host["ctrl"]).max()
    print(f"pairing {pairing}: session vs host loop |dtraj| {d_traj:.3e} |dctrl| {d_ctrl:.3e}; min clearance against A {held[0].min():.3e}, B {held[1].min():.3e}; "
          f"|clearance - numpy| {np.abs(np.array(cl) - nine.min(0)).max():.3e}")
    assert held.min() >= -1e-6 and np.abs(np.array(cl) - nine.min(0)).max() <= 1e-12
    assert np.all(host["status"] == 1) and d_traj < TOL_HOST and d_ctrl < TOL_HOST and np.array_equal(host["chosen"], np.array(chosen))
    backend.close(), loop.solver()[0]._backend.close()


# ---- (f) -----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_optional_outputs_and_the_device_forms():
    """(f) both forms of begin_sized refuse NULL, NaN, inf and negative rsums and M = 0 with "rsums" in the message, and a finite upper bound on the
    circle rows with MPC_ERR_BOUNDS; set_bounds to such a structure between two steps: the step returns MPC_ERR_BOUNDS, steps_done is unchanged, and
    after the bounds are restored the session ends with the bits of an undisturbed one; step_pred refuses a session with M = 0, a NULL pred, and a
    measured state at step 0; every optional output may be NULL in the new forms; the device forms give the bits of the host forms"""
    import torch
    s = make_solver(lref.CFG)
    set_cfg_bounds(s, lref.CFG)
    lib, h = s._lib, s._h
    dp = abi.as_dp
    B, Ls = 10, N
    inputs, tracks, offsets = mirrored(B)
    init, path, orient, vdes = inputs
    vd = np.ascontiguousarray(vdes, dtype=np.float64)
    rs = mixed_rsums(offsets.shape)
    tracks = np.ascontiguousarray(tracks[:, :, :L])
    u = np.empty((B, 2))
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())          # noqa: E731
    cuda = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()          # noqa: E731
    d_in = [cuda(a) for a in (init, path, orient, vd)]

    def refused(rc, code, word):
        msg = lib.mpc_last_error(h)
        assert rc == code and msg and word in msg, (rc, msg)
        assert lib.mpc_session_steps_done(h) == -1

    def begin(M=2, offsets=offsets, rsums=rs):
        return lib.mpc_session_begin_sized(h, B, Ls, L, dp(init), dp(path), dp(orient), dp(vd), M, 1, dp(offsets), dp(rsums), 0)

    def begin_dev(M=2, offsets=offsets, rsums=rs):
        d_off, d_rs = cuda(offsets), cuda(rsums)
        return lib.mpc_session_begin_sized_dev(h, B, Ls, L, *(vp(t) for t in d_in), M, 1, vp(d_off), vp(d_rs), 0, None)

    for form in (begin, begin_dev):
        refused(form(rsums=None), abi.MPC_ERR_INVALID, b"rsums")
        refused(form(M=0, offsets=None), abi.MPC_ERR_INVALID, b"rsums")
        for bad in (np.nan, np.inf, -0.1):
            r = rs.copy()
            r[7, 1] = bad
            refused(form(rsums=r), abi.MPC_ERR_INVALID, b"rsums")
    lbg, ubg, lbx, ubx = BicycleNLP(lref.CFG).bounds()
    capped = ubg.copy()
    capped[1 + lref.CFG.nx * (N + 1):] = 80.0
    s.set_bounds(lbx, ubx, lbg, capped)
    for form in (begin, begin_dev):
        refused(form(), abi.MPC_ERR_BOUNDS, b"circle rows")
    s.set_bounds(lbx, ubx, lbg, ubg)
    # set_bounds between two steps of a sized session
    feed = lambda i: dict(predicted=zs.predicted(tracks, i, N)) if i % 2 else dict(obstacles=zs.observed(tracks, i, DT))          # noqa: E731
    calm = run(s, inputs, offsets, 0, feed, rsums=rs)
    with s.session(*inputs, L, offsets=offsets, rsums=rs) as sess:
        for i in range(L):
            if i in (1, 2, 7):
                s.set_bounds(lbx, ubx, lbg, capped)
                with pytest.raises(pkg.MpcError) as e:
                    sess.step(**feed(i))
                assert e.value.code == abi.MPC_ERR_BOUNDS and sess.steps_done == i
                s.set_bounds(lbx, ubx, lbg, ubg)
            sess.step(**feed(i))
        assert_same(sess.record(), calm[:3], "after MPC_ERR_BOUNDS at a step")
    # step_pred: refusals, and every optional output NULL
    pred = zs.predicted(tracks, 0, N)
    assert lib.mpc_session_begin(h, B, Ls, L, dp(init), dp(path), dp(orient), dp(vd), 0, 0, None, 0) == abi.MPC_OK

    def refused_open(rc, word, done):
        msg = lib.mpc_last_error(h)
        assert rc == abi.MPC_ERR_INVALID and msg and word in msg and lib.mpc_session_steps_done(h) == done, (rc, msg)

    refused_open(lib.mpc_session_step_pred(h, None, dp(pred), dp(u), None, None, None, None, None), b"M = 0", 0)
    assert lib.mpc_session_end(h) == abi.MPC_OK
    host_u = {}
    for sized in (False, True):
        assert (begin() if sized else lib.mpc_session_begin(h, B, Ls, L, dp(init), dp(path), dp(orient), dp(vd), 2, 1, dp(offsets), 0)) == abi.MPC_OK
        refused_open(lib.mpc_session_step_pred(h, None, None, dp(u), None, None, None, None, None), b"pred", 0)
        refused_open(lib.mpc_session_step_pred(h, None, dp(pred), None, None, None, None, None, None), b"u [B, 2]", 0)
        refused_open(lib.mpc_session_step_pred(h, dp(np.ascontiguousarray(init)), dp(pred), dp(u), None, None, None, None, None), b"step 0", 0)
        host_u[sized] = []
        for i in range(Ls):
            p_i = zs.predicted(tracks, i, N)
            assert lib.mpc_session_step_pred(h, None, dp(p_i), dp(u), None, None, None, None, None) == abi.MPC_OK and lib.mpc_session_steps_done(h) == i + 1
            host_u[sized].append(u.copy())
        rc = lib.mpc_session_step_pred(h, None, dp(pred), dp(u), None, None, None, None, None)
        assert rc == abi.MPC_ERR_STATE and b"all L steps" in lib.mpc_last_error(h)
        assert lib.mpc_session_end(h) == abi.MPC_OK
        rc = lib.mpc_session_step_pred(h, None, dp(pred), dp(u), None, None, None, None, None)
        assert rc == abi.MPC_ERR_STATE and b"no session" in lib.mpc_last_error(h)
    full = run(s, inputs, offsets, 0, lambda i: dict(predicted=zs.predicted(tracks, i, N)), rsums=rs, steps=Ls, length=Ls)
    assert np.array_equal(np.stack(host_u[True], 1), full[3])                          # (outputs asked for or not: the same step)
    assert not np.array_equal(np.stack(host_u[True], 1), np.stack(host_u[False], 1))    # (the radii matter)
    # the device-pointer forms: the bits of the host forms
    o_u = torch.empty((B, 2), dtype=torch.float64, device="cuda")
    o_cl, o_ch = torch.empty(B, dtype=torch.float64, device="cuda"), torch.empty((B, N + 1, 3), dtype=torch.int32, device="cuda")
    d_off, d_rs = cuda(offsets), cuda(rs)
    assert lib.mpc_session_begin_sized_dev(h, B, Ls, L, *(vp(t) for t in d_in), 2, 1, vp(d_off), vp(d_rs), 0, None) == abi.MPC_OK
    d_off.zero_(), d_rs.zero_()                                                         # (begin has copied what it was given)
    sess = object.__new__(pkg.LoopSession)
    sess._s, sess._open = s, True
    for i in range(Ls):
        d_pred = cuda(zs.predicted(tracks, i, N))
        if i % 2:
            sess.step_device(o_u.data_ptr(), d_pred=d_pred.data_ptr())
        else:
            sess.step_device(o_u.data_ptr(), d_pred=d_pred.data_ptr(), d_clearance=o_cl.data_ptr(), d_chosen=o_ch.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(o_u.cpu().numpy(), host_u[True][i]), i
        if i % 2 == 0:
            assert np.array_equal(o_cl.cpu().numpy(), full[6][:, i]) and np.array_equal(o_ch.cpu().numpy(), full[8][:, i]), i
    sess.close()
    s.close()
