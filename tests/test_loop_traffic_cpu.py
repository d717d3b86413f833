"""CPU: the pieces of the loop through traffic (mpc_closed_loop_batch_traffic: k_loop_traffic in front of every solve) that need no GPU.

tests/trafx/trafx.cpp calls what the threads of k_loop_traffic run -- loop_traffic_stage of the shipped header -- in the kernel's thread numbering;
tests/traffic_ref.py restates the selection and the clearance in numpy and holds scene S with its reference loops."""
import ctypes as C
import os

import numpy as np
import pytest

import loop_obst_ref as lref
import traffic_ref as ref
from helpers import ROOT, WEIGHTS_YAML_ZAM_LF, abi, harness_lib, make_configuration, pkg, straight_path

scn = __import__("importlib").import_module(pkg.__name__ + ".scenario")
opt = lref.opt
_dp, _ip = abi.as_dp, abi.as_ip
NEW = ("mpc_closed_loop_batch_traffic", "mpc_closed_loop_batch_traffic_dev")


def test_new_entry_points_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mpcgpu.h")).read()
    L = C.CDLL(abi.LIB_PATH)
    for s in NEW:
        assert s in abi.EXPORTS and hasattr(L, s) and ("int " + s + "(") in hdr, s
    P = abi.PROTOTYPES
    # the arguments of the predicted loop with (Lt, obst_track, obst_offset, predict) replaced by (M, Lt, per_ego, tracks, offsets, pairing), and
    # nearest and chosen behind clearance
    i32, dp, ip, vp = C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_void_p
    old = P["mpc_closed_loop_batch_pred"]
    assert P["mpc_closed_loop_batch_traffic"] == old[:8] + [i32, i32, i32, dp, dp, i32] + old[12:] + [ip, ip]
    old = P["mpc_closed_loop_batch_pred_dev"]
    assert P["mpc_closed_loop_batch_traffic_dev"] == old[:8] + [i32, i32, i32, vp, vp, i32] + old[12:-1] + [vp, vp, vp]


@pytest.fixture(scope="module")
def trafx():
    L = C.CDLL(harness_lib("trafx"))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L.trafx_step.argtypes = [C.c_int32] * 9 + [C.c_double, dp, dp, dp, dp, dp, C.c_double, C.c_int32, dp, dp, ip, ip]
    L.trafx_step.restype = None
    return L


EGO_OFFSET, R_SUM = 0.75, 3.3
DESC = np.array([-100.0, 0.0, -99.0, 0.5, -101.0, -0.5])


def _scene(rng, B, L, Lt, M, per_ego):
    """seeded tracks spread over tens of metres, with absent spans: every obstacle of a moving scene is away for a span of its own, row 2 is empty
    for everybody (a stage that sees nothing), a standing scene of five lacks obstacle 3"""
    lead = (B,) if per_ego else ()
    tracks = rng.uniform(-40.0, 40.0, lead + (M, Lt, 3))
    tracks[..., 2] = rng.uniform(-np.pi, np.pi, lead + (M, Lt))
    flat = tracks.reshape(-1, Lt, 3)
    if Lt > 1:
        for q in range(flat.shape[0]):
            a = rng.integers(0, Lt)
            flat[q, a:a + rng.integers(1, 4)] = np.nan
        flat[:, 2] = np.nan
    elif M == 5:
        tracks[..., 3, :, :] = np.nan
    return np.ascontiguousarray(tracks), np.ascontiguousarray(rng.uniform(0.4, 1.6, lead + (M,)))


def _run(trafx, descending, B, L, Lt, nx, N, M, per_ego, pairing, tracks, offsets, state, x0, i):
    obst = np.full((B, N + 1, 6), np.nan)
    cl, near, chosen = np.full((B, L), np.nan), np.full((B, L), -7, np.int32), np.full((B, L, N + 1, 3), -7, np.int32)
    trafx.trafx_step(descending, B, L, Lt, nx, N, M, per_ego, pairing, EGO_OFFSET, _dp(DESC), _dp(tracks), _dp(offsets), _dp(state), _dp(x0), R_SUM, i,
                     _dp(obst), _dp(cl), _ip(near), _ip(chosen))
    return obst, cl, near, chosen


@pytest.mark.parametrize("nx", [5, 6])
@pytest.mark.parametrize("N", [1, 2, 3, 10])
def test_selection_and_clearance_against_numpy(trafx, N, nx):
    """loop_traffic_stage, what the threads of k_loop_traffic do, for every (b, k, i): M in {1, 2, 5}, Lt in {1, L, L + N}, tracks shared and per ego,
    both pairings, obstacles that come and go, a row where nothing is present, step 0 (the measured state) and later steps (the warm start's stages).
    Rows to 1e-12 (numpy's cos / sin may differ from libm's in the last bit); indices wherever numpy's margin between the best candidate and the
    runner-up exceeds 1e-9 m -- on these seeded poses that is everywhere, which is asserted; the threads in ascending and in descending order give
    the same arrays; nothing but column i of clearance / nearest and block i of chosen is written"""
    rng = np.random.default_rng(900 + 10 * N + nx)
    B, L = 5, 6
    nw = 2 * N + nx * (N + 1)
    compared = left_out = 0
    for M in (1, 2, 5):
        for Lt in (1, L, L + N):
            for per_ego in (0, 1):
                tracks, offsets = _scene(rng, B, L, Lt, M, per_ego)
                state = np.ascontiguousarray(rng.uniform(-30.0, 30.0, (B, nx)))
                x0 = np.ascontiguousarray(rng.uniform(-30.0, 30.0, (B, nw)))
                for pairing in (0, 1):
                    for i in range(L):
                        obst, cl, near, chosen = _run(trafx, 0, B, L, Lt, nx, N, M, per_ego, pairing, tracks, offsets, state, x0, i)
                        back = _run(trafx, 1, B, L, Lt, nx, N, M, per_ego, pairing, tracks, offsets, state, x0, i)
                        for a, b in zip((obst, cl, near, chosen), back):
                            assert np.array_equal(a, b, equal_nan=True)
                        poses = ref.ego_poses(i, state, x0, N, nx)
                        want, w_chosen, margin = ref.select(i, poses, tracks, offsets, pairing, EGO_OFFSET, DESC)
                        sure = margin > ref.MARGIN
                        assert np.abs(obst - want)[np.repeat(sure, 2, axis=2)].max(initial=0.0) <= 1e-12, (M, Lt, per_ego, pairing, i)
                        assert np.array_equal(chosen[:, i][sure], w_chosen[sure])
                        w_cl, w_near, m_cl = ref.clearance(i, state, tracks, offsets, EGO_OFFSET, R_SUM)
                        fin = np.isfinite(w_cl)
                        assert np.array_equal(np.isfinite(cl[:, i]), fin) and np.all(cl[:, i][~fin] == np.inf)
                        assert np.abs(cl[:, i][fin] - w_cl[fin]).max(initial=0.0) <= 1e-12
                        assert np.array_equal(near[:, i][m_cl > ref.MARGIN], w_near[m_cl > ref.MARGIN])
                        compared += sure.size + m_cl.size
                        left_out += int((~sure).sum() + (m_cl <= ref.MARGIN).sum())
                        # only column i / block i was written
                        assert np.isnan(np.delete(cl, i, axis=1)).all() and np.all(np.delete(near, i, axis=1) == -7) and np.all(np.delete(chosen, i, axis=1) == -7)
                        if Lt > 1 and i <= 2 <= i + N:
                            k = 2 - i                                            # the empty row: the descriptor's centres, chosen -1
                            assert np.array_equal(obst[:, k], np.tile(DESC, (B, 1))) and np.all(chosen[:, i, k] == -1)
                        if Lt > 1 and i == 2:
                            assert np.all(cl[:, 2] == np.inf) and np.all(near[:, 2] == -1)
                    # no output asked for: the rows alone
                    obst0 = np.full((B, N + 1, 6), np.nan)
                    trafx.trafx_step(0, B, L, Lt, nx, N, M, per_ego, pairing, EGO_OFFSET, _dp(DESC), _dp(tracks), _dp(offsets), _dp(state), _dp(x0), R_SUM,
                                     L - 1, _dp(obst0), None, None, None)
                    assert np.array_equal(obst0, obst)
    print(f"N = {N}, nx = {nx}: {compared} indices compared, {left_out} left out by the margin rule")
    assert left_out == 0 and left_out < 0.01 * compared


def test_ties_go_to_the_lowest_index(trafx):
    """the same obstacle twice, at indices 1 and 3, among farther ones: both pairings pick index 1 for every slot, and nearest is 1 -- also when the
    twin comes first in memory order of another ego (per-ego tracks, reversed)"""
    rng = np.random.default_rng(2)
    B, L, N, nx, M = 4, 3, 2, 5, 5
    tracks = rng.uniform(-40.0, 40.0, (M, 1, 3))
    tracks[:, :, :2] += 200.0                                                      # (far from the egos, which stay within 30 m of the origin)
    tracks[1] = tracks[3] = [[5.0, -3.0, 0.3]]
    offsets = np.array([1.0, 1.1, 0.7, 1.1, 1.3])
    state = np.ascontiguousarray(rng.uniform(-30.0, 30.0, (B, nx)))
    x0 = np.ascontiguousarray(rng.uniform(-30.0, 30.0, (B, 2 * N + nx * (N + 1))))
    for pairing in (0, 1):
        for i in range(L):
            _, cl, near, chosen = _run(trafx, 0, B, L, 1, nx, N, M, 0, pairing, np.ascontiguousarray(tracks), offsets, state, x0, i)
            assert np.all(chosen[:, i] == 1) and np.all(near[:, i] == 1) and np.isfinite(cl[:, i]).all()


def test_one_obstacle_gives_the_rows_of_the_predicted_loop(trafx):
    """M = 1, pairing 0: the rows are those of loop_obst_stage (tests/predx) on the same track, bit for bit -- what makes the loop through one obstacle
    the predicted loop"""
    predx = C.CDLL(harness_lib("predx"))
    dp = C.POINTER(C.c_double)
    predx.predx_loop_step.argtypes = [C.c_int32] * 6 + [C.c_double, dp, C.c_double, dp, C.c_double, C.c_int32, dp, dp]
    predx.predx_loop_step.restype = None
    rng = np.random.default_rng(5)
    B, L, N, nx = 7, 6, 3, 5
    for Lt in (1, L, L + N):
        track = np.ascontiguousarray(rng.uniform(-20, 20, (B, 1, Lt, 3)))
        off = np.full((B, 1), 1.25)
        state = np.ascontiguousarray(rng.uniform(-3, 3, (B, nx)))
        x0 = np.ascontiguousarray(rng.uniform(-3, 3, (B, 2 * N + nx * (N + 1))))
        for i in range(L):
            obst = _run(trafx, 0, B, L, Lt, nx, N, 1, 1, 0, track, off, state, x0, i)[0]
            want = np.full((B, N + 1, 6), np.nan)
            predx.predx_loop_step(1, B, L, Lt, nx, N, EGO_OFFSET, _dp(np.ascontiguousarray(track[:, 0])), 1.25, _dp(state), R_SUM, i, _dp(want), None)
            assert np.array_equal(obst, want)


def test_host_twin_selects_what_the_reference_selects():
    """optimizer.nearest_obstacle_centres, the numpy selection of CasadiOptimizer's step-by-step loop, against tests/traffic_ref.py"""
    rng = np.random.default_rng(11)
    N = 10
    for pairing in (0, 1):
        for _ in range(5):
            tracks, offsets = _scene(rng, 1, 12, 12 + N, 4, 0)
            poses = rng.uniform(-30, 30, (N + 1, 3))
            for i in (0, 1, 7):
                rows = np.minimum(i + np.arange(N + 1), tracks.shape[1] - 1)
                got, picked = opt.nearest_obstacle_centres(poses, tracks, offsets, rows, EGO_OFFSET, pairing, DESC)
                want, w_chosen, margin = ref.select(i, poses[None], tracks, offsets, pairing, EGO_OFFSET, DESC)
                assert margin.min() > ref.MARGIN
                assert np.abs(got - want[0]).max() <= 1e-12 and np.array_equal(picked, w_chosen[0])


# ---- the emulated per-stage solve ----------------------------------------------------------------------------------------------------------------
def test_emulated_per_stage_solve():
    """tests/trafx steps EmuSolve with centres per stage: with the same centres at every stage it is the emulated per-instance solve, bit for bit; with
    the moving centres of tests/pred_obst_ref.py's drift family its rows are KKT points of the staged NLP by the certificate, at the thresholds
    tests/test_pred_obst_cpu.py holds the reference's optima to"""
    import pred_obst_ref as pref
    from helpers import CA_CFG, ca_batch, emu_solve, kkt_certificate
    x0, p = ca_batch(CA_CFG, 3)
    obst = np.ascontiguousarray(np.tile(CA_CFG.obstacle_centers.ravel(), (3, 1)) + np.arange(3)[:, None] * 0.1)
    per = emu_solve(CA_CFG, x0, p, obst=obst)
    st = ref.emu_solve_stages(CA_CFG, x0, p, np.repeat(obst[:, None], CA_CFG.N + 1, axis=1))
    assert np.array_equal(st.x, per["x"]) and np.array_equal(st.status, per["status"]) and np.array_equal(st.iters, per["iters"])
    cfg = pref.cfg_for(10)
    inst = [pref.instance("drift", 10, seed) for seed in range(4)]
    r = ref.emu_solve_stages(cfg, np.array([q[0] for q in inst]), np.array([q[1] for q in inst]), np.array([q[2].reshape(-1, 6) for q in inst]))
    assert np.all(r.status == 1)
    for b, (_, p_b, stages) in enumerate(inst):
        c = kkt_certificate(pref.StagedNLP(cfg, stages), r.x[b], p_b)
        assert c["feasibility"] <= 1e-6 and c["stationarity"] <= 1e-6, (b, c)


# ---- scene S -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pairing", [0, 1])
def test_scene_s_needs_both_obstacles(pairing):
    """what the GPU test presupposes of scene S, in the reference loop alone (numpy host loop, dense interior-point method on the NLP with centres per
    stage): every status 1; the loop through both obstacles keeps clear of both to -1e-6 (the solver's bound relaxation 1e-8 r_sum plus its tolerance,
    two orders above); the loop that is given only A drives more than 0.1 m into B, the one given only B more than 0.1 m into A.
    The measure is the one the NLP of the pairing holds: with pairing 1 all nine pairs, with pairing 0 the three pairs (j, j) the reference's NLP
    constrains -- its cross pairs (front against rear) are free, which is what pairing 1 is for."""
    both, only_a, only_b = (ref.scene_s(w, pairing) for w in ("AB", "A", "B"))
    measure = ref.clearance_pairs if pairing == 0 else ref.clearance_nine
    cl = {w: np.stack([measure(r["traj"], m) for m in range(2)]) for w, r in (("AB", both), ("A", only_a), ("B", only_b))}
    print(f"pairing {pairing}: both: min clearance A {cl['AB'][0].min():.3e} B {cl['AB'][1].min():.3e}; only A: B {cl['A'][1].min():.3f}; only B: A {cl['B'][0].min():.3f}")
    for r in (both, only_a, only_b):
        assert np.all(r["status"] == 1)
    assert cl["AB"].min() >= -1e-6
    assert cl["A"][1].min() < -ref.UNDERCUT and cl["B"][0].min() < -ref.UNDERCUT
    assert cl["A"][0].min() >= -1e-6 and cl["B"][1].min() >= -1e-6
    assert both["traj"][:, 1].max() > 0.3 and both["traj"][:, 1].min() < -0.3          # left past A, right past B


# ---- scenario and optimizer ----------------------------------------------------------------------------------------------------------------------
XML_PEACH = os.path.join(ROOT, "tests", "golden", "scenarios", "USA_Peach-2_1_T-1_route.xml")
XML_ZAM = os.path.join(ROOT, "tests", "golden", "scenarios", "ZAM_Over-1_1.xml")


def test_obstacle_tracks_of_a_scenario():
    """USA_Peach-2_1_T-1: four moving obstacles, 334 leaves after time step 25 -- NaN outside each obstacle's lifetime, the recorded poses inside;
    ZAM_Over-1_1: the static obstacle repeats its pose; ids pick and order; an unknown id raises"""
    sc = scn.read_scenario(XML_PEACH)
    tr, ln, wd = scn.obstacle_tracks(sc, None, 40)
    ids = [o.obstacle_id for o in sc.dynamic_obstacles]
    assert ids == [334, 366, 380, 512] and tr.shape == (4, 40, 3) and ln.shape == wd.shape == (4,)
    for m, o in enumerate(sc.dynamic_obstacles):
        assert (ln[m], wd[m]) == (o.length, o.width)
        for i in range(40):
            if min(o.states) <= i <= max(o.states):
                assert np.array_equal(tr[m, i], o.states[i])
            else:
                assert np.isnan(tr[m, i]).all()
    assert np.isnan(tr[0, 26:]).all() and np.isfinite(tr[0, :26]).all() and np.isfinite(tr[1:]).all()
    pick, ln2, _ = scn.obstacle_tracks(sc, [512, 334], 30)
    assert np.array_equal(pick, tr[[3, 0], :30], equal_nan=True) and np.array_equal(ln2, ln[[3, 0]])
    with pytest.raises(KeyError):
        scn.obstacle_tracks(sc, [1], 10)
    zam = scn.read_scenario(XML_ZAM)
    tz, lz, wz = scn.obstacle_tracks(zam, None, 5)
    o = zam.obstacles[0]
    assert tz.shape == (1, 5, 3) and np.array_equal(tz[0], np.tile([o.position[0], o.position[1], o.orientation], (5, 1))) and (lz[0], wz[0]) == (6.0, 3.5)


def test_configuration_takes_all_or_a_list():
    sc = scn.read_scenario(XML_PEACH)
    for ids, want in (("all", [334, 366, 380, 512]), ([380, 334], [380, 334])):
        settings = {"scenario_settings": {"scenario_name": "USA_Peach-2_1_T-1", "use_case": "collision_avoidance", "draw": False, "dynamic_obstacle_id": ids},
                    "general_planning_settings": {"framework_name": "casadi", "predict_horizon": 10, "noised": False},
                    "vehicle_settings": {1500: {"reference_point": "rear", "vehicle_model": "parameters_vehicle2", "wheelbase": 2.578,
                                                "resampling_reference_path": True}},
                    "weights_setting": dict(WEIGHTS_YAML_ZAM_LF)}
        conf = scn.Configuration(settings, sc, 1500).configuration
        tr, ln, wd = scn.obstacle_tracks(sc, want, conf.iter_length)
        assert np.array_equal(conf.obstacle_tracks, tr, equal_nan=True) and np.array_equal(conf.obstacle_sizes, np.stack([ln, wd], 1))
        assert conf.static_obstacle["length"] == ln[0] and conf.static_obstacle["position_x"] == tr[0, 0, 0] and not hasattr(conf, "obstacle_track")


class _TrafficBackend:
    """stands in for BatchedMPCSolver: keeps what closed_loop_traffic is handed"""

    def __init__(self, N):
        self.N, self.calls, self.bounds = N, [], None

    def set_bounds(self, lbx, ubx, lbg, ubg):
        self.bounds = (lbx, ubx, lbg, ubg)

    def closed_loop(self, *a, **kw):
        raise AssertionError("the traffic loop was expected")

    def closed_loop_traffic(self, init, path, orient, vdes, steps, tracks, offsets, **kw):
        self.calls.append(dict(tracks=tracks, offsets=offsets, steps=steps, **kw))
        S = self.N + 1
        return (np.zeros((1, steps, 5)), np.zeros((1, steps, 2)), np.ones((1, steps), np.int32), np.full((1, steps), 1.5), np.zeros((1, steps), np.int32),
                np.zeros((1, steps, S, 3), np.int32))


def test_optimizer_hands_tracks_offsets_and_the_largest_radius_over():
    L, N = 20, 10
    path, orient = straight_path(L, 0.0, 0.0, 0.0, 10.0)
    conf = make_configuration(path, orient, 10.0, WEIGHTS_YAML_ZAM_LF, use_case="collision_avoidance",
                              obstacle=dict(position_x=25.0, position_y=3.0, length=4.0, width=1.8, orientation=0.0))
    sizes = np.array([[4.0, 1.8], [12.0, 2.5], [6.0, 3.5]])
    tracks = np.random.default_rng(0).uniform(-5, 5, (3, 7, 3))                  # (shorter than the run: the last pose is held)
    conf.obstacle_tracks, conf.obstacle_sizes, conf.obstacle_pairing = tracks, sizes, 1
    o = opt.CasadiOptimizer(configuration=conf, init_values=(np.array([0.0, 0.0]), 10.0, 0.0, 0.0), predict_horizon=N)
    be = _TrafficBackend(N)
    o._sol = opt.NlpSolverHandle(be)
    states, controls, _ = o.optimize()
    (call,) = be.calls
    assert call["tracks"].shape == (3, L, 3) and np.array_equal(call["tracks"][:, :7], tracks) and np.array_equal(call["tracks"][:, 7:], np.repeat(tracks[:, -1:], L - 7, 1))
    radii, disc = zip(*[opt.compute_approximating_circle_radius(l, w) for l, w in sizes])
    assert np.array_equal(call["offsets"], np.array(disc) / 4) and call["pairing"] == 1 and call["steps"] == L
    assert o.radius_obstacle == max(radii) and radii.index(max(radii)) != 0
    lbg = np.asarray(be.bounds[2])
    assert np.all(lbg[-9 * (N + 1):] == o.radius_ego + max(radii))
    assert states.shape == (L, 5) and o.clearance.shape == (L,) and o.nearest.shape == (L,) and o.chosen.shape == (L, N + 1, 3)


class _FakeLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def test_solver_hands_the_traffic_arguments_over():
    s = object.__new__(pkg.BatchedMPCSolver)
    s._lib, s._h, s.N, s.nx = _FakeLib(), C.c_void_p(1), 10, 5
    s._sens_gen = s._sens_B = 0
    B, L = 3, 12
    init, path, orient = np.zeros((B, 5)), np.zeros((B, L, 2)), np.zeros((B, L))
    out = s.closed_loop_traffic(init, path, orient, 10.0, L, np.zeros((4, L, 3)), np.ones(4), pairing=1)
    assert [a.shape for a in out] == [(B, L, 5), (B, L, 2), (B, L), (B, L), (B, L), (B, L, 11, 3)] and out[4].dtype == out[5].dtype == np.int32
    s.closed_loop_traffic(init, path, orient, 10.0, L, np.zeros((B, 2, 1, 3)), np.ones((B, 2)))
    s.closed_loop_traffic_device(B, 1, 2, 3, 4, L, L, 2, L, 0, 5, 6, 7, 8, pairing=1, d_chosen=9)
    (n0, a0), (n1, a1), (n2, a2) = s._lib.calls
    assert (n0, n1, n2) == ("mpc_closed_loop_batch_traffic", "mpc_closed_loop_batch_traffic", "mpc_closed_loop_batch_traffic_dev")
    assert a0[8:11] == (4, L, 0) and a0[13] == 1 and a1[8:11] == (2, 1, 1) and a1[13] == 0 and a2[8:11] == (2, L, 0) and a2[13] == 1
    assert s._sens_gen == 3                                      # (every loop ends the life of a snapshot)
    for tr, off in ((np.zeros((4, L, 2)), np.ones(4)), (np.zeros((4, L, 3)), np.ones(3)), (np.zeros((B + 1, 4, L, 3)), np.ones((B + 1, 4)))):
        with pytest.raises(pkg.MpcError):
            s.closed_loop_traffic(init, path, orient, 10.0, L, tr, off)
