"""GPU: the closed loop through traffic of mixed sizes (mpc_closed_loop_batch_traffic_sized: k_loop_traffic_sized in front of every solve, which is a
sized one).  Identity with the traffic loop when every radius is the handle's; scene S of tests/traffic_ref.py with a small A and a large B, through
CasadiOptimizer with obstacle_radii = "own": the device loop against the step-by-step host loop (numpy selection, device sized solves)."""
import numpy as np
import pytest

import loop_obst_ref as lref
import traffic_ref as ref
from helpers import WEIGHTS_YAML_ZAM_LF, BicycleNLP, abi, make_configuration, make_solver, pkg, set_cfg_bounds, straight_path
from test_gpu_loop_traffic import one_obstacle_batch

pytestmark = pytest.mark.gpu

N, L = lref.N, lref.L
TOL_HOST = 1e-6            # the device loop against the step-by-step host loop: the bound tests/test_gpu_loop_traffic.py holds the same comparison to
EGO_OFFSET, R_SUM = lref.CFG.ego_offset, lref.CFG.r_sum
SMALL_LW = (3.0, 1.5)      # obstacle A of scene S; B keeps the 6 x 3.5 m rectangle of tests/loop_obst_ref.py


@pytest.fixture(scope="module")
def scene_solver():
    s = make_solver(lref.CFG)
    set_cfg_bounds(s, lref.CFG)
    return s


@pytest.mark.parametrize("pairing", [0, 1])
@pytest.mark.parametrize("B", [10, 130])
def test_equal_radii_give_the_bits_of_the_traffic_loop(scene_solver, B, pairing):
    """two obstacles per ego (the batch's own and its mirror image across the path), tracks per ego and ego 0's shared by all: with every rsums[m] the
    handle's bound, traj, ctrl, step_status, clearance, nearest and chosen are those of mpc_closed_loop_batch_traffic, bit for bit"""
    s = scene_solver
    init, path, orient, vdes, tr = one_obstacle_batch(B)
    mirror = tr * np.array([1.0, -1.0, -1.0])
    tracks = np.ascontiguousarray(np.stack([tr, mirror], axis=1))                    # [B, 2, Lt, 3]
    offsets = np.full((B, 2), lref.OFFSET)
    for tk, of in ((tracks, offsets), (np.ascontiguousarray(tracks[0]), offsets[0])):
        plain = s.closed_loop_traffic(init, path, orient, vdes, L, tk, of, pairing=pairing)
        sized = s.closed_loop_traffic(init, path, orient, vdes, L, tk, of, pairing=pairing, rsums=np.full(of.shape, R_SUM))
        for a, b in zip(plain, sized):
            assert np.array_equal(a, b)
        assert (plain[2] == 1).mean() > 0.5 and set(np.unique(plain[5])) >= {0, 1}


def _optimizer(backend, pairing, radii, device, sizes):
    path, orient = straight_path(ref.S_L, 0.0, 0.0, 0.0, lref.V_EGO)
    first = ref.S_TRACKS[1, 0]
    conf = make_configuration(path, orient, lref.V_EGO, WEIGHTS_YAML_ZAM_LF, use_case="collision_avoidance", noised=False,
                              obstacle=dict(position_x=first[0], position_y=first[1], length=lref.OBST_LW[0], width=lref.OBST_LW[1], orientation=first[2]))
    conf.obstacle_tracks = np.asarray(ref.S_TRACKS, dtype=np.float64)
    conf.obstacle_sizes = np.asarray(sizes, dtype=np.float64)
    conf.obstacle_pairing = pairing
    conf.obstacle_radii = radii
    o = ref._LoggingOptimizer(configuration=conf, init_values=(np.array([0.0, 0.0]), lref.V_EGO, 0.0, 0.0), predict_horizon=N)
    o.use_device_loop = device
    o._sol = ref._LoggingHandle(backend)
    return o


def _own_clearance(traj, pose, offset, rsum, nine):
    """[L] distance - rsum of a trajectory [L, 5] against one standing obstacle: the three pairs (j, j), or all nine"""
    E = ref.centres(traj[:, [0, 1, 4]], EGO_OFFSET)                                  # [L, 3, 2]
    O = ref.centres(np.asarray(pose), offset)                                        # [3, 2]
    D = np.hypot(E[:, :, None, 0] - O[None, None, :, 0], E[:, :, None, 1] - O[None, None, :, 1])
    return (D.reshape(len(traj), 9).min(1) if nine else np.min([D[:, j, j] for j in range(3)], 0)) - rsum


@pytest.mark.parametrize("pairing", [0, 1])
def test_scene_s_with_a_small_a_and_a_large_b(pairing):
    """scene S with A a 3 x 1.5 m obstacle and B the 6 x 3.5 m one, obstacle_radii = "own" (the radius sums differ by more than 0.5 m).  Every status
    1; the device loop against the step-by-step host loop (nearest_obstacle_centres with radii, device sized solves) within 1e-6; the clearance of
    every step against each obstacle's own radius, in the pairing's measure, >= -1e-6; the loop's own clearance is numpy's to 1e-12; the unsized
    loop on a handle with the small radius ends more than 1e-3 inside B; obstacle_radii = "largest" is the loop without radii"""
    sizes = (SMALL_LW, lref.OBST_LW)
    backend = make_solver(lref.CFG)
    dev = _optimizer(backend, pairing, "own", True, sizes)
    rs, off = dev.obstacle_rsums, dev.obstacle_offsets
    print(f"radius sums {rs}, offsets {off}")
    assert rs[1] - rs[0] >= 0.5 and abs(rs[1] - R_SUM) < 1e-12
    traj, ctrl, _ = dev.optimize()
    assert np.all(dev._sol._stats["status"] == 1)
    host = _optimizer(make_solver(lref.CFG), pairing, "own", False, sizes)
    hx, hu, _ = host.optimize()
    d_traj, d_ctrl = np.abs(traj - hx).max(), np.abs(ctrl - hu).max()
    held = np.stack([_own_clearance(traj, ref.S_TRACKS[m, 0], off[m], rs[m], pairing == 1) for m in range(2)])
    print(f"pairing {pairing}: device vs host loop |dtraj| {d_traj:.3e} |dctrl| {d_ctrl:.3e}; min clearance against A {held[0].min():.3e}, B {held[1].min():.3e}")
    assert np.all(np.array(host._sol.steps) == 1)
    assert d_traj < TOL_HOST and d_ctrl < TOL_HOST
    assert held.min() >= -1e-6
    nine = np.stack([_own_clearance(traj, ref.S_TRACKS[m, 0], off[m], rs[m], True) for m in range(2)])
    assert np.abs(dev.clearance - nine.min(0)).max() <= 1e-12
    assert set(np.unique(dev.chosen)) == {0, 1}
    # the direct call is that loop
    path, orient = straight_path(ref.S_L, 0.0, 0.0, 0.0, lref.V_EGO)
    init = np.array([[0.0, 0.0, 0.0, lref.V_EGO, 0.0]])
    s = make_solver(lref.CFG)
    set_cfg_bounds(s, lref.CFG)
    direct = s.closed_loop_traffic(init, path[None], orient[None], np.array([lref.V_EGO]), ref.S_L, ref.S_TRACKS, off, pairing=pairing, rsums=rs)
    assert np.abs(direct[0][0] - traj).max() < TOL_HOST and np.all(direct[2] == 1)
    # one radius, the small one: planned through the truck
    lbg, ubg, lbx, ubx = BicycleNLP(lref.CFG).bounds()
    lbg = lbg.copy()
    lbg[1 + lref.CFG.nx * (N + 1):] = rs[0]
    s.set_bounds(lbx, ubx, lbg, ubg)
    small = s.closed_loop_traffic(init, path[None], orient[None], np.array([lref.V_EGO]), ref.S_L, ref.S_TRACKS, off, pairing=pairing)
    into_b = _own_clearance(small[0][0], ref.S_TRACKS[1, 0], off[1], rs[1], pairing == 1).min()
    print(f"one radius, the small one: {into_b:.3f} m against B's own radius")
    assert into_b < -1e-3
    # "largest", the default: the loop as it was
    big = _optimizer(backend, pairing, "largest", True, sizes)
    bx, bu, _ = big.optimize()
    set_cfg_bounds(s, lref.CFG)
    plain = s.closed_loop_traffic(init, path[None], orient[None], np.array([lref.V_EGO]), ref.S_L, ref.S_TRACKS, off, pairing=pairing)
    assert big.obstacle_rsums is None and np.abs(plain[0][0] - bx).max() < TOL_HOST


def test_refusals():
    """NULL rsums, a negative or NaN entry (both forms: the device form copies them back once, as it does the offsets), a handle whose circle rows have
    a finite upper bound (MPC_ERR_BOUNDS)"""
    import torch
    s = make_solver(lref.CFG)
    set_cfg_bounds(s, lref.CFG)
    init, path, orient, vdes, tr = one_obstacle_batch(10)
    tracks, offsets = np.ascontiguousarray(tr[:, None]), np.full((10, 1), lref.OFFSET)
    for bad in (-0.1, np.nan, np.inf):
        rs = np.full((10, 1), R_SUM)
        rs[3, 0] = bad
        with pytest.raises(pkg.MpcError) as e:
            s.closed_loop_traffic(init, path, orient, vdes, L, tracks, offsets, rsums=rs)
        assert e.value.code == abi.MPC_ERR_INVALID and "rsums" in str(e.value)
        t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (init, path, orient, vdes, tracks, offsets, rs)]
        o = [torch.empty((10, L, c), dtype=torch.float64, device="cuda") for c in (5, 2)]
        with pytest.raises(pkg.MpcError) as e:
            s.closed_loop_traffic_device(10, *(a.data_ptr() for a in t[:4]), L, path.shape[1], 1, tracks.shape[2], 1, t[4].data_ptr(), t[5].data_ptr(),
                                         o[0].data_ptr(), o[1].data_ptr(), d_rsums=t[6].data_ptr())
        assert e.value.code == abi.MPC_ERR_INVALID and "rsums" in str(e.value)
    dp, ip = abi.as_dp, abi.as_ip
    traj, ctrl, st = np.empty((10, L, 5)), np.empty((10, L, 2)), np.empty((10, L), np.int32)
    rc = s._lib.mpc_closed_loop_batch_traffic_sized(s._h, 10, L, path.shape[1], dp(init), dp(path), dp(orient), dp(vdes), 1, tracks.shape[2], 1, dp(tracks),
                                                    dp(offsets), None, 0, 0, 0.0, 0, dp(traj), dp(ctrl), ip(st), None, None, None)
    assert rc == abi.MPC_ERR_INVALID and b"rsums" in s._lib.mpc_last_error(s._h)
    lbg, ubg, lbx, ubx = BicycleNLP(lref.CFG).bounds()
    ubg = ubg.copy()
    ubg[1 + lref.CFG.nx * (N + 1):] = 80.0
    s.set_bounds(lbx, ubx, lbg, ubg)
    with pytest.raises(pkg.MpcError) as e:
        s.closed_loop_traffic(init, path, orient, vdes, L, tracks, offsets, rsums=np.full((10, 1), R_SUM))
    assert e.value.code == abi.MPC_ERR_BOUNDS
