"""GPU: the closed loop past per-ego obstacles that move (mpc_closed_loop_batch_obst: k_loop_obst in front of every solve) and the per-ego
collision verdict (mpc_validity_batch_ego).  Scenes, oracle loop and numpy restatements: tests/loop_obst_ref.py; what is presupposed about
the oracle loop is checked in tests/test_loop_obstacles_cpu.py."""
import numpy as np
import pytest

import loop_obst_ref as ref
from helpers import abi, make_solver, pkg, set_cfg_bounds
from oracle import metrics_numpy as M

pytestmark = pytest.mark.gpu

TOL_ORACLE = 1e-4          # a closed loop against an independent solver (the project's north-star bound)
TOL_HOST = 1e-6            # the device loop against the step-by-step host loop (as the existing device-versus-host loop tests)


@pytest.fixture(scope="module")
def scene_solver():
    s = make_solver(ref.CFG)
    set_cfg_bounds(s, ref.CFG)
    return s


@pytest.mark.parametrize("moving", [True, False])
def test_ten_scenes_as_one_batch(scene_solver, moving):
    """The ten scenes (tests/loop_obst_ref.py: N = 10, L = 40, a 6 x 3.5 m obstacle 25 m ahead at five lateral offsets and two speeds; the ego
    swerves up to 0.44 m, the circle rows are active) as one batch of ten egos with an obstacle each -- moving tracks (Lt = L), and the same
    obstacles held at their start pose (Lt = 1): against the oracle loop (one oracle solve per step with that step's obstacle), against the
    step-by-step host loop through BatchedMPCSolver.solve(obst=...), and the clearance against numpy on the returned trajectories and
    against the oracle loop's."""
    s = scene_solver
    init, path, orient, vdes = ref.loop_inputs()
    tracks = np.stack([ref.track_of(sc, moving) for sc in ref.SCENES])
    traj, ctrl, st, cl = s.closed_loop(init, path, orient, vdes, ref.L, obst_track=tracks if moving else tracks[:, :1], obst_offset=ref.OFFSET, clearance=True)
    o = ref.oracle_loops(moving)
    d_traj, d_ctrl, d_cl = np.abs(traj - o["traj"]).max(), np.abs(ctrl - o["ctrl"]).max(), np.abs(cl - o["clearance"]).max()
    print(f"moving={moving}: device loop vs oracle loop  |dtraj| {d_traj:.3e}  |dctrl| {d_ctrl:.3e}  |dclearance| {d_cl:.3e}  min clearance {cl.min():.3e}")
    assert np.all(st == 1)
    assert d_traj < TOL_ORACLE and d_ctrl < TOL_ORACLE
    host = make_solver(ref.CFG)
    hx, hu = zip(*[ref.host_loop(host, ref.track_of(sc, moving)) for sc in ref.SCENES])
    h_traj, h_ctrl = np.abs(traj - np.array(hx)).max(), np.abs(ctrl - np.array(hu)).max()
    print(f"moving={moving}: device loop vs host loop    |dtraj| {h_traj:.3e}  |dctrl| {h_ctrl:.3e}")
    assert h_traj < TOL_HOST and h_ctrl < TOL_HOST
    want = ref.clearance_numpy(traj, ref.centres_numpy(tracks), ref.CFG.ego_offset, ref.CFG.r_sum)
    print(f"moving={moving}: clearance vs numpy on the returned trajectories {np.abs(cl - want).max():.3e}")
    assert np.abs(cl - want).max() <= 1e-12
    assert d_cl < TOL_ORACLE
    assert np.abs(traj[:, :, 1]).max() > 0.4                           # (the obstacles were seen)
    # without clearance: three return values, the same loop
    t2, c2, st2 = s.closed_loop(init, path, orient, vdes, ref.L, obst_track=tracks if moving else tracks[:, :1], obst_offset=ref.OFFSET)
    assert np.array_equal(t2, traj) and np.array_equal(c2, ctrl) and np.array_equal(st2, st)


def test_standing_obstacle_at_the_descriptors_centres_is_the_plain_loop():
    """Lt = 1 and every ego's pose set so that its centres ARE the descriptor's (heading 0: the centres are exact): bit for bit the loop of
    mpc_closed_loop_batch_ex on the same handle.  The handle is pinned to variant 0 of the loop kernels (option bound_mask = 0), as
    INTEGRATION.md section 5b prescribes where a solve with per-instance obstacle rows and one without have to agree bit for bit: by
    default the latter runs variant 2, another instruction stream of the same algorithm."""
    B = 96
    pose = (ref.AHEAD, -2.9, 0.0)
    cfg = ref.cfg_for(pose)
    s = make_solver(cfg)
    set_cfg_bounds(s, cfg)
    s.set_option("bound_mask", "0")
    assert np.array_equal(np.array(s.desc.obstacle[:]), [25.0, -2.9, 26.0, -2.9, 24.0, -2.9]) and ref.OFFSET == 1.0
    rng = np.random.default_rng(5)
    init, path, orient, vdes = ref.loop_inputs()
    init, path, orient, vdes = np.tile(init[:1], (B, 1)), np.tile(path[:1], (B, 1, 1)), np.tile(orient[:1], (B, 1)), np.tile(vdes[:1], B)
    init[:, 1] += rng.uniform(-0.3, 0.3, B)
    init[:, 3] *= rng.uniform(0.95, 1.05, B)
    t0, c0, st0 = s.closed_loop(init, path, orient, vdes, ref.L)
    t1, c1, st1, cl = s.closed_loop(init, path, orient, vdes, ref.L, obst_track=np.tile(pose, (B, 1)), obst_offset=ref.OFFSET, clearance=True)
    assert np.all(st0 == 1) and np.abs(t0[:, :, 1] - init[:, None, 1]).max() > 0.2          # (active rows: the egos swerve)
    assert np.array_equal(st1, st0) and np.array_equal(t1, t0) and np.array_equal(c1, c0)
    assert np.abs(cl.min(axis=1) - s.metrics(t0, r_sum=cfg.r_sum)["clearance"]).max() <= 1e-12


def _loop_inputs(B, L, v=15.0, psi=0.1, seed=0):
    k = np.arange(L)
    path = np.stack([k * v * 0.1 * np.cos(psi), k * v * 0.1 * np.sin(psi)], axis=1)
    rng = np.random.default_rng(seed)
    init = np.tile([0.0, 0.0, 0.0, v, psi], (B, 1))
    init[:, 1] += rng.uniform(-0.5, 0.5, B)
    init[:, 3] *= rng.uniform(0.9, 1.1, B)
    return init, np.tile(path, (B, 1, 1)), np.full((B, L), psi), np.full(B, v)


def test_enqueue_everything_path_equals_the_step_by_step_form():
    """B = 3000, N = 30, L = 32 (the sizes of the abandoned-launch test: 47 tiles in the persistent launch, a ragged last block of k_loop_obst):
    per-ego moving tracks 6 - 10 m beside the path (distinct rows, none active); the loop enqueued without a host synchronisation gives the
    bits of the step-by-step form"""
    B, L, N = 3000, 32, 30
    init, path, orient, vdes = _loop_inputs(B, L + N)
    rng = np.random.default_rng(8)
    side = rng.uniform(6.0, 10.0, B) * rng.choice([-1.0, 1.0], B)
    along = rng.uniform(0.0, 30.0, B)[:, None] + rng.uniform(2.0, 12.0, B)[:, None] * 0.1 * np.arange(L)[None]
    psi = 0.1
    track = np.stack([along * np.cos(psi) - side[:, None] * np.sin(psi), along * np.sin(psi) + side[:, None] * np.cos(psi),
                      np.broadcast_to(psi + rng.uniform(-0.2, 0.2, B)[:, None], (B, L))], axis=2)
    s = pkg.BatchedMPCSolver(N, 5)
    s.set_bounds()
    ta, ca, sa, cla = s.closed_loop(init, path, orient, vdes, L, obst_track=track, obst_offset=1.0, clearance=True)
    assert not s.last_loop_replayed() and np.all(sa == 1)
    s.set_option("loop_async", "0")
    ts, cs, ss, cls = s.closed_loop(init, path, orient, vdes, L, obst_track=track, obst_offset=1.0, clearance=True)
    assert s.last_loop_replayed()
    assert np.array_equal(ta, ts) and np.array_equal(ca, cs) and np.array_equal(sa, ss) and np.array_equal(cla, cls)
    r_sum = 1.2000000000000002                                           # the default bounds' circle rows
    c6 = np.stack([track[..., 0], track[..., 1], track[..., 0] + np.cos(track[..., 2]), track[..., 1] + np.sin(track[..., 2]),
                   track[..., 0] - np.cos(track[..., 2]), track[..., 1] - np.sin(track[..., 2])], axis=-1)
    want = ref.clearance_numpy(ta, c6, s.desc.ego_offset, r_sum)
    assert np.abs(cla - want).max() <= 1e-12 and cla.min() > 2.0        # (none active)


def test_per_ego_verdict_equals_the_oracle_per_ego():
    """mpc_validity_batch_ego on 64 random trajectories with two moving rectangles of their own each: the indices of
    oracle.metrics_numpy.validity called once per ego; and the shared-obstacle entry point, on the same data with one obstacle set for all,
    answers as before (the oracle) and as the per-ego one given that set B times"""
    rng = np.random.default_rng(21)
    B, L, n = 64, 40, 2
    k = np.arange(L)
    base = np.stack([2.0 * k, 0.02 * (2.0 * k) ** 1.5 / 4.0], 1)
    traj = np.zeros((B, L, 5))
    traj[:, :, :2] = base[None] + rng.uniform(-2.5, 2.5, (B, 1, 2)) + rng.normal(0, 0.2, (B, L, 2))
    traj[:, :, 4] = np.arctan2(np.gradient(base[:, 1]), np.gradient(base[:, 0]))[None] + rng.normal(0, 0.1, (B, L))
    ob = np.zeros((B, n, L, 5))
    for b in range(B):
        # one crossing the path somewhere (hit or missed by a few metres), one oncoming further out
        at = rng.integers(5, L - 5)
        ob[b, 0, :, :2] = base[at] + np.array([0.0, rng.uniform(-5.0, 5.0)]) + np.outer(k - at, rng.uniform(-0.5, 0.5, 2))
        ob[b, 1, :, :2] = base[::-1] * rng.uniform(0.5, 1.0) + np.array([0.0, rng.choice([-1.0, 1.0]) * rng.uniform(2.0, 6.0)])
        ob[b, :, :, 2:4] = rng.uniform(1.5, 5.0, (n, 1, 2))
        ob[b, :, :, 4] = rng.uniform(-3, 3, (n, 1))
        ob[b, rng.integers(0, n), rng.integers(0, L, 5), 2] = 0.0          # absent at some steps
    nrm = np.stack([-np.gradient(base[:, 1]), np.gradient(base[:, 0])], 1)
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    lb, rb = base + 3.0 * nrm, base - 3.0 * nrm
    s = pkg.BatchedMPCSolver(10, 5)
    r = s.validity(traj, ob, lb, rb)
    want = [M.validity(traj[b], ob[b], lb, rb) for b in range(B)]
    assert [tuple(q) for q in zip(r["first_collision"], r["first_off_road"])] == want
    assert 0.1 < np.mean(r["first_collision"] >= 0) < 0.9
    assert len({w[0] for w in want}) > 5                                       # (verdicts differ from ego to ego)
    shared = s.validity(traj, ob[3], lb, rb)
    want_s = [M.validity(traj[b], ob[3], lb, rb) for b in range(B)]
    assert [tuple(q) for q in zip(shared["first_collision"], shared["first_off_road"])] == want_s
    again = s.validity(traj, np.tile(ob[3], (B, 1, 1, 1)), lb, rb)
    assert np.array_equal(again["first_collision"], shared["first_collision"]) and np.array_equal(again["first_off_road"], shared["first_off_road"])
    assert not np.array_equal(shared["first_collision"], r["first_collision"])


def test_device_pointer_form_and_argument_errors():
    """mpc_closed_loop_batch_obst_dev on torch tensors gives the rows of the host-pointer form; Lt = 2 with L = 40, and a NULL track, each
    return MPC_ERR_INVALID with a message (host and device-pointer forms; refused before anything is read or enqueued)"""
    import torch
    s = make_solver(ref.CFG)
    set_cfg_bounds(s, ref.CFG)
    init, path, orient, vdes = ref.loop_inputs()
    B, L = init.shape[0], ref.L
    tracks = np.stack([ref.track_of(sc) for sc in ref.SCENES])
    traj, ctrl, st, cl = s.closed_loop(init, path, orient, vdes, L, obst_track=tracks, obst_offset=ref.OFFSET, clearance=True)
    assert np.all(st == 1)
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (init, path, orient, vdes, tracks)]
    o_traj, o_ctrl, o_cl = (torch.empty(sh, dtype=torch.float64, device="cuda") for sh in ((B, L, 5), (B, L, 2), (B, L)))
    o_st = torch.empty((B, L), dtype=torch.int32, device="cuda")
    args = (B, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), L, L, o_traj.data_ptr(), o_ctrl.data_ptr(), o_st.data_ptr())
    torch.cuda.synchronize()
    s.closed_loop_device(*args, d_obst_track=d[4].data_ptr(), Lt=L, obst_offset=ref.OFFSET, d_clearance=o_cl.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(o_traj.cpu().numpy(), traj) and np.array_equal(o_ctrl.cpu().numpy(), ctrl) and np.array_equal(o_st.cpu().numpy(), st)
    assert np.array_equal(o_cl.cpu().numpy(), cl)
    for kw in (dict(d_obst_track=d[4].data_ptr(), Lt=2), dict(d_obst_track=0, Lt=L)):
        with pytest.raises(pkg.MpcError) as e:
            s.closed_loop_device(*args, obst_offset=ref.OFFSET, **kw)
        assert e.value.code == abi.MPC_ERR_INVALID and "obst_track" in str(e.value) and "Lt" in str(e.value)
    with pytest.raises(pkg.MpcError) as e:
        s.closed_loop(init, path, orient, vdes, L, obst_track=np.zeros((B, 2, 3)), obst_offset=ref.OFFSET)
    assert e.value.code == abi.MPC_ERR_INVALID and "Lt" in str(e.value)
    lib, dp = s._lib, abi.as_dp
    rc = lib.mpc_closed_loop_batch_obst(s._h, B, L, L, dp(init), dp(path), dp(orient), dp(vdes), L, None, ref.OFFSET, 0, 0.0, 0, dp(traj), dp(ctrl),
                                        abi.as_ip(st), None)
    assert rc == abi.MPC_ERR_INVALID and b"obst_track" in lib.mpc_last_error(s._h)
    # the handle still works
    assert np.array_equal(s.closed_loop(init, path, orient, vdes, L, obst_track=tracks, obst_offset=ref.OFFSET)[0], traj)
