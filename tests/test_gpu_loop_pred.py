"""GPU: the closed loop past per-ego obstacles with the obstacle predicted over each solve's horizon (mpc_closed_loop_batch_pred: k_loop_obst_stages
and k_transpose_obst_stages in front of every solve, which reads centres per stage).  Scenes, host loop pieces and numpy restatements:
tests/loop_obst_ref.py."""
import numpy as np
import pytest

import loop_obst_ref as ref
from helpers import WEIGHTS_YAML_ZAM_LF, abi, make_configuration, make_solver, pkg, set_cfg_bounds, straight_path

pytestmark = pytest.mark.gpu

opt = ref.opt
N, L = ref.N, ref.L
TOL_HOST = 1e-6            # the device loop against the step-by-step host loop (the existing loop tests' bound for the same comparison)


def track_of(scene, Lt, drift=0.0):
    """[Lt, 3] poses of the scene's obstacle (tests/loop_obst_ref.py: 25 m ahead, lateral offset and speed of the scene) at Lt loop steps;
    drift: metres per step towards the ego's lane, the heading along the motion"""
    lat, v = scene
    k = np.arange(Lt)
    y = lat - np.sign(lat) * drift * k
    return np.stack([ref.AHEAD + v * ref.DT * k, y, np.full(Lt, np.arctan2(-np.sign(lat) * drift, v * ref.DT))], axis=1)


def tracks(Lt, drift=0.0):
    return np.ascontiguousarray(np.stack([track_of(sc, Lt, drift) for sc in ref.SCENES]))


@pytest.fixture(scope="module")
def scene_solver():
    s = make_solver(ref.CFG)
    set_cfg_bounds(s, ref.CFG)
    return s


class PredictingOptimizer(opt.CasadiOptimizer):
    """the step-by-step host loop with the obstacle predicted: the solve of step i gets the centres of track rows min(i + k, Lt - 1), k = 0 .. N"""

    def obstacle_centers_at(self, step):
        return np.stack([super(PredictingOptimizer, self).obstacle_centers_at(step + k) for k in range(self.predict_horizon + 1)])


def host_loop(backend, track):
    path, orient = straight_path(L, 0.0, 0.0, 0.0, ref.V_EGO)
    conf = make_configuration(path, orient, ref.V_EGO, WEIGHTS_YAML_ZAM_LF, use_case="collision_avoidance",
                              obstacle=dict(position_x=track[0, 0], position_y=track[0, 1], length=ref.OBST_LW[0], width=ref.OBST_LW[1], orientation=track[0, 2]))
    conf.obstacle_track = track
    o = PredictingOptimizer(configuration=conf, init_values=(np.array([0.0, 0.0]), ref.V_EGO, 0.0, 0.0), predict_horizon=N)
    o.use_device_loop = False
    o._sol = opt.NlpSolverHandle(backend)
    states, controls, _ = o.optimize()
    return states, controls


def centres_of(track):
    return ref.centres_numpy(track)


@pytest.mark.parametrize("extra", [0, N])
def test_ten_scenes_predicted(scene_solver, extra):
    """the ten scenes as one batch, tracks of Lt = L (the last pose held over the last horizons) and Lt = L + N: the device loop with predict 1
    against the host loop that calls solve(obst = [1, N+1, 6]) per step; predict 0 against mpc_closed_loop_batch_obst, bit for bit; the
    clearance against numpy on the returned trajectory"""
    s = scene_solver
    init, path, orient, vdes = ref.loop_inputs()
    tr = tracks(L + extra)
    traj, ctrl, st, cl = s.closed_loop(init, path, orient, vdes, L, obst_track=tr, obst_offset=ref.OFFSET, clearance=True, predict=True)
    assert np.all(st == 1)
    host = make_solver(ref.CFG)
    hx, hu = zip(*[host_loop(host, tr[b]) for b in range(len(ref.SCENES))])
    h_traj, h_ctrl = np.abs(traj - np.array(hx)).max(), np.abs(ctrl - np.array(hu)).max()
    print(f"Lt = L + {extra}: predicted device loop vs host loop  |dtraj| {h_traj:.3e}  |dctrl| {h_ctrl:.3e}   min clearance {cl.min():.3e}")
    assert h_traj < TOL_HOST and h_ctrl < TOL_HOST
    want = ref.clearance_numpy(traj, centres_of(tr[:, :L]), ref.CFG.ego_offset, ref.CFG.r_sum)
    assert np.abs(cl - want).max() <= 1e-12
    assert np.abs(traj[:, :, 1]).max() > 0.3                                   # (the obstacles were seen)
    # predict 0 is the frozen loop
    f0 = s.closed_loop(init, path, orient, vdes, L, obst_track=tr, obst_offset=ref.OFFSET, clearance=True)
    B = init.shape[0]
    t1, c1, s1, l1 = np.empty((B, L, 5)), np.empty((B, L, 2)), np.empty((B, L), np.int32), np.empty((B, L))
    dp = abi.as_dp
    vd = np.ascontiguousarray(vdes, dtype=np.float64)
    rc = s._lib.mpc_closed_loop_batch_pred(s._h, B, L, path.shape[1], dp(init), dp(path), dp(orient), dp(vd), tr.shape[1], dp(tr), ref.OFFSET, 0, 0, 0.0, 0,
                                           dp(t1), dp(c1), abi.as_ip(s1), dp(l1))
    assert rc == 0
    for a, b in zip(f0, (t1, c1, s1, l1)):
        assert np.array_equal(a, b)
    assert np.abs(traj - f0[0]).max() > 1e-3                                    # ... and the predicted one is another loop
    # without clearance: three return values, the same loop
    t2, c2, st2 = s.closed_loop(init, path, orient, vdes, L, obst_track=tr, obst_offset=ref.OFFSET, predict=True)
    assert np.array_equal(t2, traj) and np.array_equal(c2, ctrl) and np.array_equal(st2, st)


def test_guarantee_between_steps(scene_solver):
    """noise_mode 0: the plant is the model's own forward-Euler step, so the state before step i is stage 1 of the solve of step i - 1, and that
    solve held stage 1 clear of track row i: clearance[b, i] >= -1e-6 for every i >= 1 whose previous step has status 1 -- two orders above
    the solver's bound relaxation 1e-8 r_sum plus its tolerance 1e-8; nothing is measured into the bound.  Scenes whose obstacle drifts 4 cm
    per step into the ego's lane while the ego passes it, Lt = L + 1.  The frozen loop on the same scenes is printed, not asserted on."""
    s = scene_solver
    init, path, orient, vdes = ref.loop_inputs()
    tr = tracks(L + 1, drift=0.04)
    traj, ctrl, st, cl = s.closed_loop(init, path, orient, vdes, L, obst_track=tr, obst_offset=ref.OFFSET, clearance=True, predict=True)
    ok = st[:, :-1] == 1
    held = cl[:, 1:][ok]
    frozen = s.closed_loop(init, path, orient, vdes, L, obst_track=tr, obst_offset=ref.OFFSET, clearance=True)
    print(f"predicted: steps with status 1: {int(ok.sum())} of {ok.size}, min clearance behind them {held.min():.3e} (overall {cl.min():.3e}); "
          f"frozen loop: status != 1 on {int((frozen[2] != 1).sum())} steps, min clearance {frozen[3].min():.3e}")
    assert ok.sum() >= ok.size // 2
    assert held.min() >= -1e-6
    assert np.abs(traj[:, :, 1]).max() > 0.3


def _loop_inputs(B, L_, v=15.0, psi=0.1, seed=0):
    k = np.arange(L_)
    path = np.stack([k * v * 0.1 * np.cos(psi), k * v * 0.1 * np.sin(psi)], axis=1)
    rng = np.random.default_rng(seed)
    init = np.tile([0.0, 0.0, 0.0, v, psi], (B, 1))
    init[:, 1] += rng.uniform(-0.5, 0.5, B)
    init[:, 3] *= rng.uniform(0.9, 1.1, B)
    return init, np.tile(path, (B, 1, 1)), np.full((B, L_), psi), np.full(B, v)


def test_enqueue_everything_form_with_predict():
    """B = 1088, N = 30 (17 tiles, a ragged last block of k_loop_obst_stages), L = 32 -- the loop takes L >= N --: per-ego moving tracks 6 - 10 m
    beside the path; the predicted loop enqueued without a host synchronisation gives the bits of the step-by-step form"""
    B, L_, N_ = 1088, 32, 30
    init, path, orient, vdes = _loop_inputs(B, L_ + N_)
    rng = np.random.default_rng(8)
    side = rng.uniform(6.0, 10.0, B) * rng.choice([-1.0, 1.0], B)
    Lt = L_ + 7                                                               # (shorter than L + N: the last pose is held)
    along = rng.uniform(0.0, 30.0, B)[:, None] + rng.uniform(2.0, 12.0, B)[:, None] * 0.1 * np.arange(Lt)[None]
    psi = 0.1
    track = np.ascontiguousarray(np.stack([along * np.cos(psi) - side[:, None] * np.sin(psi), along * np.sin(psi) + side[:, None] * np.cos(psi),
                                           np.broadcast_to(psi + rng.uniform(-0.2, 0.2, B)[:, None], (B, Lt))], axis=2))
    s = pkg.BatchedMPCSolver(N_, 5)
    s.set_bounds()
    ta, ca, sa, cla = s.closed_loop(init, path, orient, vdes, L_, obst_track=track, obst_offset=1.0, clearance=True, predict=True)
    assert not s.last_loop_replayed() and np.all(sa == 1)
    s.set_option("loop_async", "0")
    ts, cs, ss, cls = s.closed_loop(init, path, orient, vdes, L_, obst_track=track, obst_offset=1.0, clearance=True, predict=True)
    assert s.last_loop_replayed()
    assert np.array_equal(ta, ts) and np.array_equal(ca, cs) and np.array_equal(sa, ss) and np.array_equal(cla, cls)
    c6 = np.stack([track[..., 0], track[..., 1], track[..., 0] + np.cos(track[..., 2]), track[..., 1] + np.sin(track[..., 2]),
                   track[..., 0] - np.cos(track[..., 2]), track[..., 1] - np.sin(track[..., 2])], axis=-1)
    want = ref.clearance_numpy(ta, c6[:, :L_], s.desc.ego_offset, 1.2000000000000002)
    assert np.abs(cla - want).max() <= 1e-12 and cla.min() > 2.0             # (none active)


def test_refusals_of_the_predicted_loop(scene_solver):
    """predict outside {0, 1}; predict 1 with Lt = 0 or a NULL track (host and device-pointer forms): MPC_ERR_INVALID with a message, before
    anything is read or enqueued; the linearised loop has no predicted form; the handle works afterwards"""
    import torch
    s = scene_solver
    init, path, orient, vdes = ref.loop_inputs()
    B = init.shape[0]
    tr = tracks(L)
    vd = np.ascontiguousarray(vdes, dtype=np.float64)
    dp, ip = abi.as_dp, abi.as_ip
    traj, ctrl, st = np.empty((B, L, 5)), np.empty((B, L, 2)), np.empty((B, L), np.int32)
    lib = s._lib

    def host(Lt, track, predict):
        return lib.mpc_closed_loop_batch_pred(s._h, B, L, L, dp(init), dp(path), dp(orient), dp(vd), Lt, dp(track), ref.OFFSET, predict, 0, 0.0, 0, dp(traj),
                                              dp(ctrl), ip(st), None)
    for Lt, track, predict, word in ((L, tr, 2, b"predict"), (L, tr, -1, b"predict"), (0, None, 1, b"predict 1"), (L, None, 1, b"predict 1"),
                                     (0, tr, 1, b"predict 1"), (2, tr, 1, b"Lt"), (L, None, 0, b"obst_track")):
        assert host(Lt, track, predict) == abi.MPC_ERR_INVALID and word in lib.mpc_last_error(s._h), (Lt, predict)
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (init, path, orient, vd, tr)]
    o_traj, o_ctrl = (torch.empty(sh, dtype=torch.float64, device="cuda") for sh in ((B, L, 5), (B, L, 2)))
    args = (B, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), L, L, o_traj.data_ptr(), o_ctrl.data_ptr())
    for kw in (dict(d_obst_track=d[4].data_ptr(), Lt=L, predict=2), dict(d_obst_track=0, Lt=L, predict=1), dict(d_obst_track=d[4].data_ptr(), Lt=0, predict=1)):
        with pytest.raises(pkg.MpcError) as e:
            s.closed_loop_device(*args, obst_offset=ref.OFFSET, **kw)
        assert e.value.code == abi.MPC_ERR_INVALID and "predict" in str(e.value)
    with pytest.raises(pkg.MpcError):
        s.closed_loop(init, path, orient, vdes, L, obst_track=tr, obst_offset=ref.OFFSET, predict=True, linearize=True)
    assert len(abi.PROTOTYPES["mpc_closed_loop_batch_lin"]) == 21                 # (not extended)
    # the device form gives the rows of the host form, and the handle still works
    want = s.closed_loop(init, path, orient, vdes, L, obst_track=tr, obst_offset=ref.OFFSET, predict=True)
    torch.cuda.synchronize()
    s.closed_loop_device(*args, d_obst_track=d[4].data_ptr(), Lt=L, obst_offset=ref.OFFSET, predict=1)
    torch.cuda.synchronize()
    assert np.array_equal(o_traj.cpu().numpy(), want[0]) and np.array_equal(o_ctrl.cpu().numpy(), want[1])
