"""CPU: the pieces of the stepping session (mpc_session_*: the closed loop stepped from outside) that need no GPU.

tests/sessx/sessx.cpp calls what the threads of k_session_ingest and k_session_traffic run -- session_ingest_instance and session_traffic_stage of the
shipped header -- in the kernels' thread numbering; tests/session_ref.py restates both in numpy (the selection is tests/traffic_ref.py's, on the observed
poses moved on at constant velocity)."""
import ctypes as C
import os

import numpy as np
import pytest

import session_ref as sref
import traffic_ref as tref
from helpers import ROOT, abi, harness_lib, pkg

_dp, _ip = abi.as_dp, abi.as_ip
NEW = ("mpc_session_begin", "mpc_session_begin_dev", "mpc_session_step", "mpc_session_step_dev", "mpc_session_record", "mpc_session_record_dev",
       "mpc_session_steps_done", "mpc_session_end")
EGO_OFFSET, R_SUM, DT = 0.75, 3.3, 0.1
DESC = np.array([-100.0, 0.0, -99.0, 0.5, -101.0, -0.5])


def test_new_entry_points_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mpcgpu.h")).read()
    L = C.CDLL(abi.LIB_PATH)
    for s in NEW:
        assert s in abi.EXPORTS and hasattr(L, s) and ("int " + s + "(") in hdr, s
    P = abi.PROTOTYPES
    i32, dp, ip, vp = C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_void_p
    # begin: the arguments of the traffic loop that do not change over a loop -- (h, B, L, Lp, init_state, path, orient, vdes), then M, per_ego, offsets, pairing
    old = P["mpc_closed_loop_batch_traffic"]
    assert P["mpc_session_begin"] == old[:8] + [i32, i32, dp, i32]
    assert P["mpc_session_begin_dev"] == P["mpc_closed_loop_batch_traffic_dev"][:8] + [i32, i32, vp, i32, vp]
    # step: (h, measured, obs, u, plan, status, clearance, nearest, chosen [, stream])
    assert P["mpc_session_step"] == [vp, dp, dp, dp, dp, ip, dp, ip, ip] and P["mpc_session_step_dev"] == [vp] * 10
    assert P["mpc_session_record"] == [vp, dp, dp, ip] and P["mpc_session_record_dev"] == [vp] * 5
    assert P["mpc_session_steps_done"] == [vp] and P["mpc_session_end"] == [vp]


@pytest.fixture(scope="module")
def sessx():
    L = C.CDLL(harness_lib("sessx"))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L.sessx_ingest.argtypes = [C.c_int32] * 3 + [dp] * 3
    L.sessx_ingest.restype = None
    L.sessx_traffic.argtypes = [C.c_int32] * 7 + [C.c_double, dp, dp, dp, dp, dp, C.c_double, C.c_double, C.c_int32, dp, dp, ip, ip]
    L.sessx_traffic.restype = None
    return L


@pytest.mark.parametrize("nx", [5, 6])
def test_ingest_against_numpy(sessx, nx):
    """session_ingest_instance for B = 9 egos, N in {1, 3, 10}: the first five entries of the state and of row 0 of X_ref become the measurement; rows
    whose x is NaN or inf (with finite entries behind it) are kept; the progress state of nx = 6, every other column of p, all of x0 and the words around
    the three arrays (one buffer, guard words between them) are bit-equal before and after"""
    rng = np.random.default_rng(40 + nx)
    B = 9
    for N in (1, 3, 10):
        nw = 2 * N + nx * (N + 1)
        sizes = [7, B * nx, 7, B * nw, 7, B * nw, 7]                                  # guard, state, guard, x0, guard, p, guard
        buf = rng.uniform(-30.0, 30.0, sum(sizes))
        at = np.cumsum([0] + sizes)
        state, x0, p = (buf[at[j]:at[j + 1]].reshape(B, -1) for j in (1, 3, 5))
        before = buf.copy()
        measured = np.ascontiguousarray(rng.uniform(-30.0, 30.0, (B, 5)))
        measured[2, 0], measured[5, 0], measured[7] = np.nan, np.inf, np.nan
        want_state, want_p = sref.ingest(measured, state, p, N, nx)
        sessx.sessx_ingest(B, N, nx, _dp(measured), _dp(state), _dp(p))
        assert np.array_equal(state, want_state) and np.array_equal(p, want_p)
        kept = [2, 5, 7]
        assert np.array_equal(state[kept], before[at[1]:at[2]].reshape(B, nx)[kept])
        changed = np.zeros(buf.size, bool)
        took = np.setdiff1d(np.arange(B), kept)
        changed[at[1]:at[2]].reshape(B, nx)[took, :5] = True
        changed[at[5]:at[6]].reshape(B, nw)[took, 2 * N: 2 * N + 5] = True
        assert np.array_equal(buf[~changed], before[~changed]) and np.array_equal(x0, before[at[3]:at[4]].reshape(B, nw))
        assert np.array_equal(state[took, :5], measured[took]) and np.array_equal(p[took, 2 * N: 2 * N + 5], measured[took])
        if nx == 6:
            assert np.array_equal(state[:, 5], before[at[1]:at[2]].reshape(B, nx)[:, 5])


def _scene(rng, B, M, per_ego, empty=False):
    """seeded observations spread over tens of metres, speeds up to 15 m/s; of five obstacles number 3 is absent, of two or more the last reports a
    velocity that is not finite; empty: nobody is present"""
    lead = (B,) if per_ego else ()
    obs = rng.uniform(-40.0, 40.0, lead + (M, 5))
    obs[..., 2] = rng.uniform(-np.pi, np.pi, lead + (M,))
    obs[..., 3:] = rng.uniform(-15.0, 15.0, lead + (M, 2))
    if M == 5:
        obs[..., 3, 0] = np.nan
    if M >= 2:
        obs[..., M - 1, 3], obs[..., M - 1, 4] = np.nan, np.inf
    if empty:
        obs[..., 0] = np.inf
    return np.ascontiguousarray(obs), np.ascontiguousarray(rng.uniform(0.4, 1.6, lead + (M,)))


def _run(sessx, descending, B, nx, N, M, per_ego, pairing, obs, offsets, state, x0, step, outputs=True):
    obst = np.full((B, N + 1, 6), np.nan)
    cl, near, chosen = np.full(B, np.nan), np.full(B, -7, np.int32), np.full((B, N + 1, 3), -7, np.int32)
    sessx.sessx_traffic(descending, B, nx, N, M, per_ego, pairing, EGO_OFFSET, _dp(DESC), _dp(obs), _dp(offsets), _dp(state), _dp(x0), R_SUM, DT, step,
                        _dp(obst), *((_dp(cl), _ip(near), _ip(chosen)) if outputs else (None, None, None)))
    return obst, cl, near, chosen


@pytest.mark.parametrize("nx", [5, 6])
@pytest.mark.parametrize("N", [1, 2, 3, 10])
def test_obstacle_rows_against_numpy(sessx, N, nx):
    """session_traffic_stage, what the threads of k_session_traffic do, for every (b, k) at step 0 (the ego pose is the state) and at step 3 (the stages
    of the warm start): M in {1, 2, 5}, obstacles shared and per ego, both pairings, an absent obstacle, a velocity that is not finite (it counts as 0),
    observations in which nobody is present.  Rows to 1e-12 (numpy's cos / sin may differ from libm's in the last bit, the compiler may fuse x + (k dt) vx);
    indices wherever numpy's margin between the best candidate and the runner-up exceeds 1e-9 m -- on these seeded poses that is everywhere, which is
    asserted; the threads in ascending and in descending order give the same arrays"""
    rng = np.random.default_rng(1300 + 10 * N + nx)
    B = 5
    nw = 2 * N + nx * (N + 1)
    compared = left_out = 0
    for M in (1, 2, 5):
        for per_ego in (0, 1):
            obs, offsets = _scene(rng, B, M, per_ego)
            state = np.ascontiguousarray(rng.uniform(-30.0, 30.0, (B, nx)))
            x0 = np.ascontiguousarray(rng.uniform(-30.0, 30.0, (B, nw)))
            for pairing in (0, 1):
                for step in (0, 3):
                    obst, cl, near, chosen = _run(sessx, 0, B, nx, N, M, per_ego, pairing, obs, offsets, state, x0, step)
                    for a, b in zip((obst, cl, near, chosen), _run(sessx, 1, B, nx, N, M, per_ego, pairing, obs, offsets, state, x0, step)):
                        assert np.array_equal(a, b)
                    want, w_chosen, margin = sref.select(step, state, x0, obs, offsets, pairing, EGO_OFFSET, DESC, N, nx, DT)
                    sure = margin > tref.MARGIN
                    assert np.abs(obst - want)[np.repeat(sure, 2, axis=2)].max(initial=0.0) <= 1e-12, (M, per_ego, pairing, step)
                    assert np.array_equal(chosen[sure], w_chosen[sure])
                    w_cl, w_near, m_cl = sref.clearance(state, obs, offsets, EGO_OFFSET, R_SUM)
                    assert np.isfinite(w_cl).all() and np.abs(cl - w_cl).max() <= 1e-12
                    assert np.array_equal(near[m_cl > tref.MARGIN], w_near[m_cl > tref.MARGIN])
                    compared += sure.size + m_cl.size
                    left_out += int((~sure).sum() + (m_cl <= tref.MARGIN).sum())
                    if M == 5:
                        assert not np.any(chosen == 3) and not np.any(near == 3)            # (the absent one is never picked)
                    # no output asked for: the rows alone
                    assert np.array_equal(_run(sessx, 0, B, nx, N, M, per_ego, pairing, obs, offsets, state, x0, step, outputs=False)[0], obst)
                # the velocity that is not finite counts as 0
                if M >= 2:
                    still = obs.copy()
                    still[..., M - 1, 3:] = 0.0
                    for a, b in zip(_run(sessx, 0, B, nx, N, M, per_ego, 1, obs, offsets, state, x0, 3), _run(sessx, 0, B, nx, N, M, per_ego, 1, still, offsets, state, x0, 3)):
                        assert np.array_equal(a, b)
            # nobody present: the descriptor's centres, chosen -1, clearance +inf, nearest -1
            obs, offsets = _scene(rng, B, M, per_ego, empty=True)
            obst, cl, near, chosen = _run(sessx, 0, B, nx, N, M, per_ego, 0, obs, offsets, state, x0, 3)
            assert np.array_equal(obst, np.tile(DESC, (B, N + 1, 1))) and np.all(chosen == -1) and np.all(cl == np.inf) and np.all(near == -1)
    print(f"N = {N}, nx = {nx}: {compared} indices compared, {left_out} left out by the margin rule")
    assert left_out == 0


@pytest.mark.parametrize("per_ego", [0, 1])
def test_standing_obstacles_give_the_rows_of_the_traffic_loop(sessx, per_ego):
    """all velocities 0: the rows, chosen, nearest and clearance are those of loop_traffic_stage with Lt = 1 (tests/trafx) bit for bit, at step 0 and at a
    later step, both pairings, nx 5 and 6, an absent obstacle among five -- what makes the session past standing obstacles the loop through traffic"""
    trafx = C.CDLL(harness_lib("trafx"))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    trafx.trafx_step.argtypes = [C.c_int32] * 9 + [C.c_double, dp, dp, dp, dp, dp, C.c_double, C.c_int32, dp, dp, ip, ip]
    trafx.trafx_step.restype = None
    rng = np.random.default_rng(77 + per_ego)
    B, L = 6, 5
    for nx in (5, 6):
        for N, M in ((1, 1), (3, 2), (10, 5)):
            nw = 2 * N + nx * (N + 1)
            obs, offsets = _scene(rng, B, M, per_ego)
            obs[..., 3:] = 0.0
            tracks = np.ascontiguousarray(obs[..., None, :3])                           # [.., M, Lt = 1, 3]
            state = np.ascontiguousarray(rng.uniform(-30.0, 30.0, (B, nx)))
            x0 = np.ascontiguousarray(rng.uniform(-30.0, 30.0, (B, nw)))
            for pairing in (0, 1):
                for i in (0, 3):
                    got = _run(sessx, 0, B, nx, N, M, per_ego, pairing, obs, offsets, state, x0, i)
                    obst = np.full((B, N + 1, 6), np.nan)
                    cl, near, chosen = np.full((B, L), np.nan), np.full((B, L), -7, np.int32), np.full((B, L, N + 1, 3), -7, np.int32)
                    trafx.trafx_step(0, B, L, 1, nx, N, M, per_ego, pairing, EGO_OFFSET, _dp(DESC), _dp(tracks), _dp(offsets), _dp(state), _dp(x0), R_SUM, i,
                                     _dp(obst), _dp(cl), _ip(near), _ip(chosen))
                    for a, b in zip(got, (obst, cl[:, i], near[:, i], chosen[:, i])):
                        assert np.array_equal(a, b), (nx, N, M, pairing, i)


class _FakeLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def test_solver_hands_the_session_arguments_over():
    s = object.__new__(pkg.BatchedMPCSolver)
    s._lib, s._h, s.N, s.nx, s.n_w = _FakeLib(), C.c_void_p(1), 10, 5, 75
    s._sens_gen = 0
    B, L = 3, 12
    init, path, orient = np.zeros((B, 5)), np.zeros((B, L, 2)), np.zeros((B, L))
    with s.session(init, path, orient, 10.0, L, offsets=np.ones((B, 2)), pairing=1) as sess:
        assert (sess.M, sess.per_ego) == (2, 1)
        u, plan, chosen = sess.step(obstacles=np.zeros((B, 2, 5)), outputs=("plan", "chosen"))
        assert u.shape == (B, 2) and plan.shape == (B, 75) and chosen.shape == (B, 11, 3) and chosen.dtype == np.int32
        assert sess.step(np.zeros((B, 5)), np.zeros((B, 2, 5))).shape == (B, 2)
        assert [a.shape for a in sess.record()] == [(B, L, 5), (B, L, 2), (B, L)]
        with pytest.raises(pkg.MpcError):
            sess.step(outputs=("gain",))
    with s.session(init, path, orient, 10.0, L) as lane:
        assert (lane.M, lane.per_ego) == (0, 0)
    names = [n for n, _ in s._lib.calls]
    assert names == ["mpc_session_begin", "mpc_session_step", "mpc_session_step", "mpc_session_record", "mpc_session_end", "mpc_session_begin", "mpc_session_end"]
    a = s._lib.calls[0][1]
    assert a[1:4] == (B, L, L) and a[8:10] == (2, 1) and a[11] == 1
    step0, step1 = s._lib.calls[1][1], s._lib.calls[2][1]
    assert step0[1] is None and step0[4] is not None and step0[5] is None and step0[8] is not None and step1[1] is not None and step1[4] is None
    assert s._lib.calls[5][1][8:11] == (0, 0, None)
    assert s._sens_gen == 2                                      # (every step is a solve: it ends the life of a snapshot)
    with pytest.raises(pkg.MpcError):
        s.session(init, path, orient, 10.0, L, offsets=np.ones((B + 1, 2)))


@pytest.mark.parametrize("sizes", [None, np.array([[4.0, 1.8], [12.0, 2.5], [6.0, 3.5]])])
def test_open_session_hands_the_configuration_over(sizes):
    """CasadiOptimizer.open_session(): what reaches mpc_set_bounds and mpc_session_begin.  With `obstacle_sizes` alone -- no tracks, the caller observes the
    obstacles -- M, the offsets (disc_distance / 4 of every rectangle), the pairing, and the largest obstacle's radius in the circle rows; without them
    lane following (M = 0, no offsets) under the static obstacle's radius.  A step then takes obstacles [M, 5]"""
    import loop_obst_ref as lref
    from helpers import WEIGHTS_YAML_ZAM_LF, make_configuration, straight_path
    opt = lref.opt
    L, N = 20, 10
    path, orient = straight_path(L, 0.0, 0.0, 0.0, 10.0)
    conf = make_configuration(path, orient, 10.0, WEIGHTS_YAML_ZAM_LF, use_case="collision_avoidance",
                              obstacle=dict(position_x=25.0, position_y=3.0, length=4.0, width=1.8, orientation=0.0))
    if sizes is not None:
        conf.obstacle_sizes, conf.obstacle_pairing = sizes, 1
    o = opt.CasadiOptimizer(configuration=conf, init_values=(np.array([1.0, 2.0]), 10.0, 0.0, 0.3), predict_horizon=N)
    s = object.__new__(pkg.BatchedMPCSolver)
    s._lib, s._h, s.N, s.nx = _FakeLib(), C.c_void_p(1), N, 5
    s.n_w, s.n_g = 2 * N + 5 * (N + 1), 1 + 14 * (N + 1)
    s._sens_gen, s._bounds_key = 0, None
    o._sol = opt.NlpSolverHandle(s)
    with o.open_session() as sess:
        u = sess.step(obstacles=None if sizes is None else np.zeros((3, 5)))
        assert u.shape == (1, 2)
    (n0, a0), (n1, a1) = s._lib.calls[:2]
    assert (n0, n1) == ("mpc_set_bounds", "mpc_session_begin")
    lbg = np.ctypeslib.as_array(a0[3], (s.n_g,))
    radii = [opt.compute_approximating_circle_radius(l, w)[0] for l, w in ([[4.0, 1.8]] if sizes is None else sizes)]
    assert np.all(lbg[-9 * (N + 1):] == o.radius_ego + max(radii)) and (sizes is None or radii.index(max(radii)) != 0)
    assert a1[1:4] == (1, L, L) and np.array_equal(np.ctypeslib.as_array(a1[4], (5,)), [1.0, 2.0, 0.0, 10.0, 0.3])
    assert np.array_equal(np.ctypeslib.as_array(a1[5], (L, 2)), path) and np.ctypeslib.as_array(a1[7], (1,))[0] == 10.0
    if sizes is None:
        assert a1[8:12] == (0, 0, None, 0) and o.obstacle_offsets is None
    else:
        assert a1[8:10] == (3, 0) and a1[11] == 1 and o.obstacle_tracks is None
        assert np.array_equal(np.ctypeslib.as_array(a1[10], (3,)), [opt.compute_approximating_circle_radius(l, w)[1] / 4 for l, w in sizes])
