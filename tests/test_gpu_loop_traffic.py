"""GPU: the closed loop through traffic (mpc_closed_loop_batch_traffic: k_loop_traffic in front of every solve, which reads centres per stage).
Scenes and the host loop pieces: tests/loop_obst_ref.py (N = 10, L = 40, the ten one-obstacle scenes); numpy restatement of the selection, scene S
and its reference loops: tests/traffic_ref.py."""
import numpy as np
import pytest

import loop_obst_ref as lref
import traffic_ref as ref
from helpers import abi, make_solver, pkg, set_cfg_bounds, straight_path, synthetic_batch

pytestmark = pytest.mark.gpu

N, L = lref.N, lref.L
TOL_HOST = 1e-6            # the device loop against the step-by-step host loop (the bound tests/test_gpu_loop_pred.py holds the same comparison to)
EGO_OFFSET, R_SUM = lref.CFG.ego_offset, lref.CFG.r_sum


@pytest.fixture(scope="module")
def scene_solver():
    s = make_solver(lref.CFG)
    set_cfg_bounds(s, lref.CFG)
    return s


def one_obstacle_batch(B):
    """(init, path, orient, vdes, tracks [B, Lt = L + 3, 3]) -- B = 10: the ten scenes of tests/loop_obst_ref.py, the obstacle drifting 4 cm per step
    towards the ego's lane; any other B: egos starting up to 0.3 m beside the path, an obstacle each 20 .. 30 m ahead, 2.9 .. 3.3 m to either side"""
    Lt = L + 3                                                       # (shorter than L + N: the last pose is held over the last horizons)
    k = np.arange(Lt)
    if B == len(lref.SCENES):
        init, path, orient, vdes = lref.loop_inputs()
        lat, v, ahead = np.array([sc[0] for sc in lref.SCENES]), np.array([sc[1] for sc in lref.SCENES]), np.full(B, lref.AHEAD)
    else:
        rng = np.random.default_rng(B)
        p1, o1 = straight_path(L, 0.0, 0.0, 0.0, lref.V_EGO)
        init = np.tile([0.0, 0.0, 0.0, lref.V_EGO, 0.0], (B, 1))
        init[:, 1] = rng.uniform(-0.3, 0.3, B)
        path, orient, vdes = np.tile(p1, (B, 1, 1)), np.tile(o1, (B, 1)), np.full(B, lref.V_EGO)
        lat, v, ahead = rng.uniform(2.9, 3.3, B) * rng.choice([-1.0, 1.0], B), rng.uniform(1.0, 5.0, B), rng.uniform(20.0, 30.0, B)
    drift = 0.04
    y = lat[:, None] - np.sign(lat)[:, None] * drift * k[None]
    head = np.arctan2(-np.sign(lat) * drift, v * lref.DT)
    tracks = np.stack([ahead[:, None] + v[:, None] * lref.DT * k[None], y, np.broadcast_to(head[:, None], (B, Lt))], axis=2)
    return init, path, orient, vdes, np.ascontiguousarray(tracks)


_pred = {}


def predicted(s, B):
    """the predicted loop on the batch's tracks (computed once per B): (traj, ctrl, step_status)"""
    if B not in _pred:
        init, path, orient, vdes, tr = one_obstacle_batch(B)
        out = s.closed_loop(init, path, orient, vdes, L, obst_track=tr, obst_offset=lref.OFFSET, predict=True)
        for a in out:
            a.setflags(write=False)
        _pred[B] = out
    return _pred[B]


@pytest.mark.parametrize("B", [10, 130])
def test_one_obstacle_is_the_predicted_loop(scene_solver, B):
    """M = 1: traj, ctrl and step_status are bit for bit those of mpc_closed_loop_batch_pred with predict 1 on the same track -- per ego (B = 10: the
    ten scenes; B = 130: 33 blocks of the solve and a block boundary of k_loop_traffic's grid, 1430 threads); with one track shared by all egos
    against the predicted loop on that track tiled.  Pairing 0: with pairing 1 a slot may take another circle of the obstacle, which is another
    NLP.  clearance is numpy's nine-pair value to 1e-12, nearest is 0, chosen is 0 everywhere."""
    s = scene_solver
    init, path, orient, vdes, tr = one_obstacle_batch(B)
    want = predicted(s, B)
    traj, ctrl, st, cl, near, chosen = s.closed_loop_traffic(init, path, orient, vdes, L, tr[:, None], np.full((B, 1), lref.OFFSET))
    assert np.array_equal(traj, want[0]) and np.array_equal(ctrl, want[1]) and np.array_equal(st, want[2])
    assert np.abs(traj[:, :, 1]).max() > 0.3 and (st == 1).mean() > 0.5                # (the obstacles were seen)
    w_cl, w_near, _ = ref.clearance_of_run(traj, tr[:, None], np.full((B, 1), lref.OFFSET), EGO_OFFSET, R_SUM)
    print(f"B = {B}: |clearance - numpy| {np.abs(cl - w_cl).max():.3e}, min clearance (nine pairs) {cl.min():.3e}")
    assert np.abs(cl - w_cl).max() <= 1e-12 and np.all(near == 0) and np.all(chosen == 0)
    # one scene, many egos: the track of ego 0 shared (per_ego 0) against the predicted loop with that track tiled
    shared = s.closed_loop_traffic(init, path, orient, vdes, L, tr[:1], np.array([lref.OFFSET]))
    tiled = s.closed_loop(init, path, orient, vdes, L, obst_track=np.ascontiguousarray(np.tile(tr[:1], (B, 1, 1))), obst_offset=lref.OFFSET, predict=True)
    for a, b in zip(shared[:3], tiled):
        assert np.array_equal(a, b)
    w_cl, _, _ = ref.clearance_of_run(shared[0], tr[:1], np.array([lref.OFFSET]), EGO_OFFSET, R_SUM)
    assert np.abs(shared[3] - w_cl).max() <= 1e-12


@pytest.mark.parametrize("B", [10, 130])
def test_decoys_and_permutations(scene_solver, B):
    """four obstacles kept more than 1000 m away and one that is absent throughout leave the bits of the one-obstacle loop unchanged, in both forms of
    the tracks; permuting the obstacles leaves traj and ctrl bit-identical and permutes chosen and nearest"""
    s = scene_solver
    init, path, orient, vdes, tr = one_obstacle_batch(B)
    want = predicted(s, B)
    rng = np.random.default_rng(3)
    Lt = tr.shape[1]
    far = np.stack([rng.uniform(1500.0, 3000.0, (B, 4, Lt)) * rng.choice([-1.0, 1.0], (B, 4, 1)), rng.uniform(1500.0, 3000.0, (B, 4, Lt)),
                    rng.uniform(-3.0, 3.0, (B, 4, Lt))], axis=3)
    tracks = np.ascontiguousarray(np.concatenate([far[:, :2], tr[:, None], np.full((B, 1, Lt, 3), np.nan), far[:, 2:]], axis=1))     # the real one: m = 2
    offsets = np.ascontiguousarray(rng.uniform(0.5, 1.5, (B, 6)))
    offsets[:, 2] = lref.OFFSET
    base = s.closed_loop_traffic(init, path, orient, vdes, L, tracks, offsets)
    assert np.array_equal(base[0], want[0]) and np.array_equal(base[1], want[1]) and np.array_equal(base[2], want[2])
    assert np.all(base[4] == 2) and np.all(base[5] == 2) and np.isfinite(base[3]).all()
    perm = np.array([4, 2, 0, 5, 3, 1])                              # new index q holds old obstacle perm[q]
    moved = s.closed_loop_traffic(init, path, orient, vdes, L, np.ascontiguousarray(tracks[:, perm]), np.ascontiguousarray(offsets[:, perm]))
    assert np.array_equal(moved[0], base[0]) and np.array_equal(moved[1], base[1]) and np.array_equal(moved[2], base[2]) and np.array_equal(moved[3], base[3])
    assert np.array_equal(perm[moved[4]], base[4]) and np.array_equal(perm[moved[5]], base[5])
    # shared tracks: ego 0's six obstacles for everybody, against the one-obstacle loop on ego 0's track
    one = s.closed_loop_traffic(init, path, orient, vdes, L, tr[:1], np.array([lref.OFFSET]))
    six = s.closed_loop_traffic(init, path, orient, vdes, L, tracks[0], offsets[0])
    assert np.array_equal(six[0], one[0]) and np.array_equal(six[1], one[1]) and np.array_equal(six[2], one[2]) and np.array_equal(six[3], one[3])


def scene_s_inputs():
    """three egos on scene S: given both obstacles, only A (B absent throughout), only B -- one batch, tracks per ego"""
    Ls = ref.S_L
    path, orient = straight_path(Ls, 0.0, 0.0, 0.0, lref.V_EGO)
    init = np.tile([0.0, 0.0, 0.0, lref.V_EGO, 0.0], (3, 1))
    tracks = np.tile(ref.S_TRACKS, (3, 1, 1, 1))
    tracks[1, 1], tracks[2, 0] = np.nan, np.nan
    return init, np.tile(path, (3, 1, 1)), np.tile(orient, (3, 1)), np.full(3, lref.V_EGO), np.ascontiguousarray(tracks), np.tile(ref.S_OFFSETS, (3, 1))


@pytest.mark.parametrize("pairing", [0, 1])
def test_scene_s(scene_solver, pairing):
    """scene S (tests/traffic_ref.py: A 25 m ahead at -2.9, B 55 m ahead at +2.9, 75 steps -- L = 40 of the one-obstacle scenes ends 15 m short of B):
    the device loop through both obstacles against the step-by-step host loop of CasadiOptimizer on the same handle's solve, to 1e-6; every status 1;
    clearance >= -1e-6 in the measure the pairing's NLP holds (pairing 1: the loop's own nine-pair clearance; pairing 0: the three pairs (j, j),
    numpy on the returned trajectory); the loops that are given one obstacle only drive more than 0.1 m into the other one, as on the CPU; chosen
    against the host loop's wherever numpy's margin between the candidates exceeds 1e-9 m, and that is all but 1 % of the entries"""
    s = scene_solver
    init, path, orient, vdes, tracks, offsets = scene_s_inputs()
    traj, ctrl, st, cl, near, chosen = s.closed_loop_traffic(init, path, orient, vdes, ref.S_L, tracks, offsets, pairing=pairing)
    assert np.all(st == 1)
    host = make_solver(lref.CFG)
    hx, hu, h_chosen, h_st = ref.host_loop(host, ref.S_TRACKS, ref.S_OFFSETS, pairing)
    poses = ref.host_loop.poses
    d_traj, d_ctrl = np.abs(traj[0] - hx).max(), np.abs(ctrl[0] - hu).max()
    measure = ref.clearance_pairs if pairing == 0 else ref.clearance_nine
    held = np.stack([[measure(traj[b], m) for m in range(2)] for b in range(3)])          # [ego, obstacle, step]
    cpu = ref.scene_s("AB", pairing)
    print(f"pairing {pairing}: device vs host loop |dtraj| {d_traj:.3e} |dctrl| {d_ctrl:.3e}; vs the CPU reference loop |dtraj| {np.abs(traj[0] - cpu['traj']).max():.3e}; "
          f"min clearance both {held[0].min():.3e} (loop's own {cl[0].min():.3e}); only A: into B {held[1, 1].min():.3f}; only B: into A {held[2, 0].min():.3f}")
    assert d_traj < TOL_HOST and d_ctrl < TOL_HOST and np.all(h_st == 1)
    # ... and CasadiOptimizer's device path (the bounds of its own inequal_constraints) is that loop
    ox, ou, o_chosen, _ = ref.host_loop(host, ref.S_TRACKS, ref.S_OFFSETS, pairing, device=True)
    assert np.abs(ox - traj[0]).max() < TOL_HOST and np.abs(ou - ctrl[0]).max() < TOL_HOST and o_chosen.shape == (ref.S_L, N + 1, 3)
    assert held[0].min() >= -1e-6
    if pairing == 1:
        assert cl[0].min() >= -1e-6
    assert held[1, 1].min() < -ref.UNDERCUT and held[2, 0].min() < -ref.UNDERCUT
    assert held[1, 0].min() >= -1e-6 and held[2, 1].min() >= -1e-6
    assert traj[0, :, 1].max() > 0.3 and traj[0, :, 1].min() < -0.3
    # the loop's own clearance and nearest: numpy on the returned trajectories
    w_cl, w_near, m_cl = ref.clearance_of_run(traj, tracks, offsets, EGO_OFFSET, R_SUM)
    assert np.abs(cl - w_cl).max() <= 1e-12 and np.array_equal(near[m_cl > ref.MARGIN], w_near[m_cl > ref.MARGIN])
    assert set(np.unique(near[0])) == {0, 1} and np.all(near[1] == 0) and np.all(near[2] == 1)
    # chosen under the margin rule
    margin = np.stack([ref.select(i, poses[i][None], ref.S_TRACKS, ref.S_OFFSETS, pairing, EGO_OFFSET)[2][0] for i in range(ref.S_L)])
    sure = margin > ref.MARGIN
    print(f"chosen: {int((~sure).sum())} of {sure.size} entries left out by the margin rule")
    assert (~sure).sum() < 0.01 * sure.size and np.array_equal(chosen[0][sure], h_chosen[sure])
    assert set(np.unique(chosen[0])) == {0, 1}


def test_async_form_and_noise(scene_solver):
    """B = 1088, N = 30, L = 32 (17 tiles: the solves run in the persistent pipeline launch, and the last block of k_loop_traffic is ragged), four
    obstacles shared by all egos, one of them present for part of the run: the loop enqueued without a host synchronisation gives the bits of the
    step-by-step form (option loop_async "1" / "0"), outputs included.  Noise mode 1 with a seed on scene S: the device loop against its host twin,
    whose samples are noise.py's, to 1e-6"""
    B, L_, N_ = 1088, 32, 30
    rng = np.random.default_rng(8)
    v, psi = 15.0, 0.1
    k = np.arange(L_ + N_)
    p1 = np.stack([k * v * 0.1 * np.cos(psi), k * v * 0.1 * np.sin(psi)], axis=1)
    init = np.tile([0.0, 0.0, 0.0, v, psi], (B, 1))
    init[:, 1] += rng.uniform(-0.5, 0.5, B)
    init[:, 3] *= rng.uniform(0.9, 1.1, B)
    path, orient, vdes = np.tile(p1, (B, 1, 1)), np.full((B, L_ + N_), psi), np.full(B, v)
    Lt, M = L_ + 7, 4
    side = rng.uniform(6.0, 10.0, M) * np.array([-1.0, 1.0, -1.0, 1.0])
    along = rng.uniform(0.0, 40.0, M)[:, None] + rng.uniform(2.0, 12.0, M)[:, None] * 0.1 * np.arange(Lt)[None]
    tracks = np.ascontiguousarray(np.stack([along * np.cos(psi) - side[:, None] * np.sin(psi), along * np.sin(psi) + side[:, None] * np.cos(psi),
                                            np.broadcast_to(psi + rng.uniform(-0.2, 0.2, M)[:, None], (M, Lt))], axis=2))
    tracks[1, :5], tracks[1, 20:] = np.nan, np.nan
    offsets = np.array([1.0, 0.8, 1.2, 1.0])
    s = pkg.BatchedMPCSolver(N_, 5)
    s.set_bounds()
    for pairing in (0, 1):
        s.set_option("loop_async", "1")
        a = s.closed_loop_traffic(init, path, orient, vdes, L_, tracks, offsets, pairing=pairing)
        assert not s.last_loop_replayed() and np.all(a[2] == 1)
        s.set_option("loop_async", "0")
        b = s.closed_loop_traffic(init, path, orient, vdes, L_, tracks, offsets, pairing=pairing)
        assert s.last_loop_replayed()
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        w_cl, w_near, m_cl = ref.clearance_of_run(a[0], tracks, offsets, s.desc.ego_offset, 1.2000000000000002)
        assert np.abs(a[3] - w_cl).max() <= 1e-12 and np.array_equal(a[4][m_cl > ref.MARGIN], w_near[m_cl > ref.MARGIN])
        assert len(np.unique(a[5])) >= 3                            # (several obstacles were the nearest of some stage)
    s.close()
    # noise on the whole predicted input sequence (mode 1), sigma of the collision-avoidance use case
    s = scene_solver
    init, path, orient, vdes, tr, off = scene_s_inputs()
    for pairing in (0, 1):
        traj, ctrl, st, _, _, _ = s.closed_loop_traffic(init[:1], path[:1], orient[:1], vdes[:1], ref.S_L, ref.S_TRACKS, ref.S_OFFSETS, pairing=pairing,
                                                         noise_mode=1, sigma=0.05, seed=77)
        hx, hu, _, _ = ref.host_loop(make_solver(lref.CFG), ref.S_TRACKS, ref.S_OFFSETS, pairing, noise_seed=77)
        d_traj, d_ctrl = np.abs(traj[0] - hx).max(), np.abs(ctrl[0] - hu).max()
        print(f"noise mode 1, pairing {pairing}: device vs host twin |dtraj| {d_traj:.3e} |dctrl| {d_ctrl:.3e}; steps with status != 1: {int((st != 1).sum())}")
        assert d_traj < TOL_HOST and d_ctrl < TOL_HOST
        assert np.abs(ctrl[0] - s.closed_loop_traffic(init[:1], path[:1], orient[:1], vdes[:1], ref.S_L, ref.S_TRACKS, ref.S_OFFSETS, pairing=pairing)[1][0]).max() > 1e-3


def test_refusals(scene_solver):
    """every refusal of include/mpcgpu.h, host and device-pointer forms: MPC_ERR_INVALID with a message, before anything is enqueued; the handle works
    afterwards, the device form gives the rows of the host form, and like every loop the call ends the life of the sensitivity snapshot"""
    import torch
    s = scene_solver
    init, path, orient, vdes, tr = one_obstacle_batch(10)
    B, M = 10, 2
    tracks = np.ascontiguousarray(np.concatenate([tr[:, None], tr[:, None] + [0.0, 40.0, 0.0]], axis=1))       # [B, 2, Lt, 3]
    Lt = tracks.shape[2]
    offsets = np.full((B, M), lref.OFFSET)
    bad_off = offsets.copy()
    bad_off[7, 1] = np.inf
    nan_off = offsets.copy()
    nan_off[0, 0] = np.nan
    vd = np.ascontiguousarray(vdes, dtype=np.float64)
    dp, ip = abi.as_dp, abi.as_ip
    traj, ctrl, st = np.empty((B, L, 5)), np.empty((B, L, 2)), np.empty((B, L), np.int32)
    lib = s._lib
    cases = [(dict(M=0), b"M >= 1"), (dict(M=-1), b"M >= 1"), (dict(Lt=2), b"Lt"), (dict(Lt=L - 1), b"Lt"), (dict(Lt=0), b"Lt"), (dict(tracks=None), b"tracks"),
             (dict(offsets=None), b"offsets"), (dict(offsets=bad_off), b"finite"), (dict(offsets=nan_off), b"finite"), (dict(pairing=2), b"pairing"),
             (dict(pairing=-1), b"pairing"), (dict(per_ego=2), b"per_ego"), (dict(per_ego=-1), b"per_ego")]

    def host(M=M, Lt=Lt, per_ego=1, tracks=tracks, offsets=offsets, pairing=0):
        return lib.mpc_closed_loop_batch_traffic(s._h, B, L, L, dp(init), dp(path), dp(orient), dp(vd), M, Lt, per_ego, dp(tracks), dp(offsets), pairing, 0, 0.0, 0,
                                                 dp(traj), dp(ctrl), ip(st), None, None, None)
    for kw, word in cases:
        assert host(**kw) == abi.MPC_ERR_INVALID and word in lib.mpc_last_error(s._h), kw
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (init, path, orient, vd, tracks, offsets, bad_off, nan_off)]
    o_traj, o_ctrl = (torch.empty(sh, dtype=torch.float64, device="cuda") for sh in ((B, L, 5), (B, L, 2)))
    o_cl = torch.empty((B, L), dtype=torch.float64, device="cuda")
    o_near, o_chosen = (torch.empty(sh, dtype=torch.int32, device="cuda") for sh in ((B, L), (B, L, N + 1, 3)))

    def dev(M=M, Lt=Lt, per_ego=1, tracks=d[4], offsets=d[5], pairing=0, **out):
        s.closed_loop_traffic_device(B, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), L, L, M, Lt, per_ego,
                                     0 if tracks is None else tracks.data_ptr(), 0 if offsets is None else offsets.data_ptr(), o_traj.data_ptr(), o_ctrl.data_ptr(),
                                     pairing=pairing, **out)
    for kw, word in cases:
        kw = {k: (d[6] if v is bad_off else d[7] if v is nan_off else v) for k, v in kw.items()}
        with pytest.raises(pkg.MpcError) as e:
            dev(**kw)
        assert e.value.code == abi.MPC_ERR_INVALID and word.decode() in str(e.value), kw
    # the device form gives the rows of the host form, and the handle still works
    want = s.closed_loop_traffic(init, path, orient, vdes, L, tracks, offsets, pairing=1)
    torch.cuda.synchronize()
    dev(pairing=1, d_clearance=o_cl.data_ptr(), d_nearest=o_near.data_ptr(), d_chosen=o_chosen.data_ptr())
    torch.cuda.synchronize()
    for got, w in zip((o_traj, o_ctrl, o_cl, o_near, o_chosen), (want[0], want[1], want[3], want[4], want[5])):
        assert np.array_equal(got.cpu().numpy(), w)
    # a snapshot does not outlive the loop
    x0, p = synthetic_batch(lref.CFG, B)
    s.solve(x0, p, lam_p=True)
    s.sens_adjoint(np.ones((B, s.n_w)))
    s.closed_loop_traffic(init, path, orient, vdes, L, tracks, offsets)
    for call in (lambda: s.sens_adjoint(np.ones((B, s.n_w))), lambda: s.sens_obst(seed_w=np.ones((B, s.n_w)))):
        with pytest.raises(pkg.MpcError) as e:
            call()
        assert e.value.code == abi.MPC_ERR_STATE
