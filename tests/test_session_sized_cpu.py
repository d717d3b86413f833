"""CPU: the pieces of the sized session and of the session stepped with predicted poses (mpc_session_begin_sized, mpc_session_step_pred) that need
no GPU.

tests/sesszx/sesszx.cpp calls what the threads of k_session_traffic_sized, k_session_pred and k_session_pred_sized run -- the three stage functions
of the shipped header that fill the square Keys x Pose of loop_traffic_place -- in the kernels' thread numbering.  The numpy restatements are
tests/traffic_ref.py's and tests/sized_ref.py's selections on the poses the stages are shown; the exact twins are the loops' own stage functions
(tests/trafx, tests/sizedx) and the plain session's (tests/sessx)."""
import ctypes as C
import os

import numpy as np
import pytest

import session_ref as sref
import session_sized_ref as zs
import sized_ref as zref
import test_loop_traffic_cpu as tl
import traffic_ref as tref
from helpers import ROOT, WEIGHTS_YAML_ZAM_LF, abi, harness_lib, make_configuration, pkg, straight_path

_dp, _ip = abi.as_dp, abi.as_ip
NEW = ("mpc_session_begin_sized", "mpc_session_begin_sized_dev", "mpc_session_step_pred", "mpc_session_step_pred_dev")
EGO_OFFSET, R_SUM, DESC, DT = tl.EGO_OFFSET, tl.R_SUM, tl.DESC, 0.1
GUARD = 7                   # words in front of and behind every output buffer


def test_new_entry_points_declared_and_exported():
    """declared in the header, exported by the library; begin_sized is begin with one pointer behind offsets, step_pred has step's prototype"""
    hdr = open(os.path.join(ROOT, "include", "mpcgpu.h")).read()
    L = C.CDLL(abi.LIB_PATH)
    for s in NEW:
        assert s in abi.EXPORTS and hasattr(L, s) and ("int " + s + "(") in hdr, s
    P = abi.PROTOTYPES
    b, bd = P["mpc_session_begin"], P["mpc_session_begin_dev"]
    assert P["mpc_session_begin_sized"] == b[:11] + [C.POINTER(C.c_double)] + b[11:]
    assert P["mpc_session_begin_sized_dev"] == bd[:11] + [C.c_void_p] + bd[11:]
    assert P["mpc_session_step_pred"] == P["mpc_session_step"] and P["mpc_session_step_pred_dev"] == P["mpc_session_step_dev"]
    assert L.mpc_abi_version() == 1


@pytest.fixture(scope="module")
def libs():
    dp, ip, i32, f64 = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_int32, C.c_double
    z = C.CDLL(harness_lib("sesszx"))
    z.sesszx_traffic_sized.argtypes = [i32] * 7 + [f64] + [dp] * 6 + [f64, f64, i32, dp, dp, ip, ip]
    z.sesszx_pred.argtypes = [i32] * 7 + [f64] + [dp] * 5 + [f64, i32, dp, dp, ip, ip]
    z.sesszx_pred_sized.argtypes = [i32] * 7 + [f64] + [dp] * 6 + [f64, i32, dp, dp, ip, ip]
    for f in (z.sesszx_traffic_sized, z.sesszx_pred, z.sesszx_pred_sized):
        f.restype = None
    assert z.sesszx_rows_per_stage() == 10
    t = C.CDLL(harness_lib("trafx"))
    t.trafx_step.argtypes = [i32] * 9 + [f64, dp, dp, dp, dp, dp, f64, i32, dp, dp, ip, ip]
    t.trafx_step.restype = None
    x = C.CDLL(harness_lib("sizedx"))
    x.sizedx_traffic_step.argtypes = [i32] * 9 + [f64] + [dp] * 6 + [f64, i32, dp, dp, ip, ip]
    x.sizedx_traffic_step.restype = None
    s = C.CDLL(harness_lib("sessx"))
    s.sessx_traffic.argtypes = [i32] * 7 + [f64, dp, dp, dp, dp, dp, f64, f64, i32, dp, dp, ip, ip]
    s.sessx_traffic.restype = None
    return z, t, x, s


class Guarded:
    """the four output buffers of a placement kernel, each between GUARD words that no call may change: rows [B, N+1, width], clearance [B], nearest
    [B], chosen [B, N+1, 3]"""

    def __init__(self, B, N, width):
        self.bufs = []
        self.rows = self._make((B, N + 1, width), np.float64, np.nan, -12345.5)
        self.cl = self._make((B,), np.float64, np.nan, -12345.5)
        self.near = self._make((B,), np.int32, -7, 123456)
        self.chosen = self._make((B, N + 1, 3), np.int32, -7, 123456)

    def _make(self, shape, dtype, fill, guard):
        n = int(np.prod(shape))
        buf = np.full(n + 2 * GUARD, guard, dtype)
        buf[GUARD:GUARD + n] = fill
        self.bufs.append((buf, n, guard))
        return buf[GUARD:GUARD + n].reshape(shape)

    def outputs(self):
        for buf, n, guard in self.bufs:
            assert np.all(buf[:GUARD] == guard) and np.all(buf[GUARD + n:] == guard)
        return self.rows.copy(), self.cl.copy(), self.near.copy(), self.chosen.copy()


def run_pred(z, descending, B, nx, N, M, per_ego, pairing, pred, offsets, state, x0, step, rsums=None, outputs=True):
    g = Guarded(B, N, 6 if rsums is None else 10)
    outs = (_dp(g.cl), _ip(g.near), _ip(g.chosen)) if outputs else (None, None, None)
    head = (descending, B, nx, N, M, per_ego, pairing, EGO_OFFSET, _dp(DESC), _dp(pred), _dp(offsets))
    if rsums is None:
        z.sesszx_pred(*head, _dp(state), _dp(x0), R_SUM, step, _dp(g.rows), *outs)
    else:
        z.sesszx_pred_sized(*head, _dp(rsums), _dp(state), _dp(x0), R_SUM, step, _dp(g.rows), *outs)
    return g.outputs()


def run_obs_sized(z, descending, B, nx, N, M, per_ego, pairing, obs, offsets, rsums, state, x0, step, outputs=True):
    g = Guarded(B, N, 10)
    outs = (_dp(g.cl), _ip(g.near), _ip(g.chosen)) if outputs else (None, None, None)
    z.sesszx_traffic_sized(descending, B, nx, N, M, per_ego, pairing, EGO_OFFSET, _dp(DESC), _dp(obs), _dp(offsets), _dp(rsums), _dp(state), _dp(x0),
                           R_SUM, DT, step, _dp(g.rows), *outs)
    return g.outputs()


def same(a, b):
    return all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a, b))


class Tally:
    def __init__(self):
        self.compared = self.left_out = 0

    def indices(self, got, want, margin):
        sure = margin > tref.MARGIN
        assert np.array_equal(got[sure], want[sure])
        self.compared += sure.size
        self.left_out += int((~sure).sum())
        return sure


def check_rows(t, rows, chosen, want, w_chosen, margin, w_rad=None):
    """rows to 1e-12 and (sized) the slots' radii exactly wherever the index is sure; the index itself; (sized) the pad"""
    sure = t.indices(chosen, w_chosen, margin)
    assert np.abs(rows[:, :, :6] - want)[np.repeat(sure, 2, axis=2)].max(initial=0.0) <= 1e-12
    if w_rad is not None:
        assert np.array_equal(rows[:, :, 6:9][sure], w_rad[sure]) and np.all(rows[:, :, 9] == 0.0)


def check_clearance(t, cl, near, w_cl, w_near, m_cl):
    fin = np.isfinite(w_cl)
    assert np.array_equal(np.isfinite(cl), fin) and np.all(cl[~fin] == np.inf) and np.all(near[~fin] == -1)
    assert np.abs(cl[fin] - w_cl[fin]).max(initial=0.0) <= 1e-12
    t.indices(near, w_near, m_cl)


@pytest.mark.parametrize("nx", [5, 6])
@pytest.mark.parametrize("N", [1, 2, 3, 10])
def test_predicted_poses_against_numpy_and_the_loops(libs, N, nx):
    """session_pred_stage and session_pred_stage_sized, what the threads of k_session_pred and k_session_pred_sized do, for every (b, k): the scenes of
    tests/test_loop_traffic_cpu.py under its seeds (M in {1, 2, 5}, Lt in {1, L, L + N}, tracks shared and per ego, obstacles that come and go, a row
    where nothing is present), both pairings, step 0 (the ego pose is the state) and step 3 (the stages of the warm start), pred[:, k] =
    tracks[:, min(i + k, Lt - 1)].  Against numpy on the track -- traffic_ref.select / clearance, sized_ref.select_sized / clearance_sized -- rows to
    1e-12, radii exactly, indices wherever numpy's margin to the runner-up exceeds traffic_ref.MARGIN (the share left out is printed and below 1 %);
    EXACTLY loop_traffic_stage (tests/trafx) and loop_traffic_stage_sized (tests/sizedx) at step i on the track; ascending and descending thread
    order the same bits; a stage whose obstacles are all absent takes the descriptor's centres while its neighbours see an obstacle; the guard
    words around every output buffer are unchanged; no output asked for: the rows alone"""
    z, trafx, sizedx, _ = libs
    rng = np.random.default_rng(900 + 10 * N + nx)
    B, L = 5, 6
    nw = 2 * N + nx * (N + 1)
    t = Tally()
    mixed = 0
    for M in (1, 2, 5):
        for Lt in (1, L, L + N):
            for per_ego in (0, 1):
                tracks, offsets = tl._scene(rng, B, L, Lt, M, per_ego)
                rsums = np.ascontiguousarray(rng.uniform(0.5, 4.0, offsets.shape))
                state = np.ascontiguousarray(rng.uniform(-30.0, 30.0, (B, nx)))
                x0 = np.ascontiguousarray(rng.uniform(-30.0, 30.0, (B, nw)))
                for pairing in (0, 1):
                    for i in (0, 3):
                        pred = zs.predicted(tracks, i, N)
                        poses = tref.ego_poses(i, state, x0, N, nx)
                        # plain
                        got = run_pred(z, 0, B, nx, N, M, per_ego, pairing, pred, offsets, state, x0, i)
                        assert same(got, run_pred(z, 1, B, nx, N, M, per_ego, pairing, pred, offsets, state, x0, i))
                        rows, cl, near, chosen = got
                        want, w_chosen, margin = tref.select(i, poses, tracks, offsets, pairing, EGO_OFFSET, DESC)
                        check_rows(t, rows, chosen, want, w_chosen, margin)
                        check_clearance(t, cl, near, *tref.clearance(i, state, tracks, offsets, EGO_OFFSET, R_SUM))
                        loop = tl._run(trafx, 0, B, L, Lt, nx, N, M, per_ego, pairing, tracks, offsets, state, x0, i)
                        assert same(got, (loop[0], loop[1][:, i], loop[2][:, i], loop[3][:, i])), (M, Lt, per_ego, pairing, i)
                        assert np.array_equal(run_pred(z, 0, B, nx, N, M, per_ego, pairing, pred, offsets, state, x0, i, outputs=False)[0], rows)
                        # sized
                        got = run_pred(z, 0, B, nx, N, M, per_ego, pairing, pred, offsets, state, x0, i, rsums)
                        assert same(got, run_pred(z, 1, B, nx, N, M, per_ego, pairing, pred, offsets, state, x0, i, rsums))
                        rows, cl, near, chosen = got
                        want, w_rad, w_chosen, margin = zref.select_sized(i, poses, tracks, offsets, rsums, R_SUM, pairing, EGO_OFFSET, DESC)
                        check_rows(t, rows, chosen, want, w_chosen, margin, w_rad)
                        check_clearance(t, cl, near, *zref.clearance_sized(i, state, tracks, offsets, rsums, EGO_OFFSET))
                        lrows = np.full((B, N + 1, 10), np.nan)
                        lcl, lnear, lchosen = np.full((B, L), np.nan), np.full((B, L), -7, np.int32), np.full((B, L, N + 1, 3), -7, np.int32)
                        sizedx.sizedx_traffic_step(0, B, L, Lt, nx, N, M, per_ego, pairing, EGO_OFFSET, _dp(DESC), _dp(tracks), _dp(offsets), _dp(rsums),
                                                   _dp(state), _dp(x0), R_SUM, i, _dp(lrows), _dp(lcl), _ip(lnear), _ip(lchosen))
                        assert same(got, (lrows, lcl[:, i], lnear[:, i], lchosen[:, i])), (M, Lt, per_ego, pairing, i)
                        assert np.array_equal(run_pred(z, 0, B, nx, N, M, per_ego, pairing, pred, offsets, state, x0, i, rsums, outputs=False)[0], rows)
                        # stages that see nobody, beside stages of the same ego that see somebody
                        p4 = np.broadcast_to(pred, (B,) + pred.shape) if not per_ego else pred                # [B, M, N+1, 3]
                        empty = ~np.isfinite(p4[..., 0]).any(axis=1)                                           # [B, N+1]
                        assert np.array_equal(rows[:, :, :6][empty], np.tile(DESC, (int(empty.sum()), 1))) and np.all(chosen[empty] == -1)
                        assert np.all(rows[:, :, 6:9][empty] == R_SUM) and np.all(chosen[~empty] >= 0)
                        mixed += int((empty.any(axis=1) & (~empty).any(axis=1)).sum())
    print(f"N = {N}, nx = {nx}: {t.compared} indices compared, {t.left_out} left out by the margin rule ({100.0 * t.left_out / t.compared:.3f} %); "
          f"{mixed} (ego, step) pairs whose horizon has stages with and without an obstacle")
    assert t.left_out < 0.01 * t.compared and (N == 1 or mixed > 0)


@pytest.mark.parametrize("nx", [5, 6])
@pytest.mark.parametrize("N", [1, 2, 3, 10])
def test_observed_poses_with_sizes_against_numpy_and_the_plain_session(libs, N, nx):
    """session_traffic_stage_sized, what the threads of k_session_traffic_sized do: the same scenes, the observation the pose of track row 0 with a
    random velocity up to 15 m/s, a velocity that is not finite on the last of two or more obstacles (it counts as 0).  Against
    sized_ref.select_sized / clearance_sized on session_ref.extrapolate(obs): rows to 1e-12, radii exactly, indices by the margin rule; with every
    radius the handle's EXACTLY session_traffic_stage (tests/sessx): rows [:6], chosen, clearance, nearest; both thread orders; guard words"""
    z, _, _, sessx = libs
    rng = np.random.default_rng(900 + 10 * N + nx)
    B, L = 5, 6
    nw = 2 * N + nx * (N + 1)
    t = Tally()
    for M in (1, 2, 5):
        for Lt in (1, L, L + N):
            for per_ego in (0, 1):
                tracks, offsets = tl._scene(rng, B, L, Lt, M, per_ego)
                rsums = np.ascontiguousarray(rng.uniform(0.5, 4.0, offsets.shape))
                state = np.ascontiguousarray(rng.uniform(-30.0, 30.0, (B, nx)))
                x0 = np.ascontiguousarray(rng.uniform(-30.0, 30.0, (B, nw)))
                obs = np.ascontiguousarray(np.concatenate([tracks[..., 0, :], rng.uniform(-15.0, 15.0, tracks.shape[:-2] + (2,))], axis=-1))
                if M >= 2:
                    obs[..., M - 1, 3], obs[..., M - 1, 4] = np.nan, np.inf
                ahead = sref.extrapolate(obs, N, DT)                                  # [.., M, N+1, 3]
                for pairing in (0, 1):
                    for step in (0, 3):
                        got = run_obs_sized(z, 0, B, nx, N, M, per_ego, pairing, obs, offsets, rsums, state, x0, step)
                        assert same(got, run_obs_sized(z, 1, B, nx, N, M, per_ego, pairing, obs, offsets, rsums, state, x0, step))
                        rows, cl, near, chosen = got
                        poses = tref.ego_poses(step, state, x0, N, nx)
                        want, w_rad, w_chosen, margin = zref.select_sized(0, poses, ahead, offsets, rsums, R_SUM, pairing, EGO_OFFSET, DESC)
                        check_rows(t, rows, chosen, want, w_chosen, margin, w_rad)
                        check_clearance(t, cl, near, *zref.clearance_sized(0, state, obs[..., None, :3], offsets, rsums, EGO_OFFSET))
                        assert np.array_equal(run_obs_sized(z, 0, B, nx, N, M, per_ego, pairing, obs, offsets, rsums, state, x0, step, outputs=False)[0], rows)
                        # every radius the handle's: the plain session's own function
                        eq = run_obs_sized(z, 0, B, nx, N, M, per_ego, pairing, obs, offsets, np.full(offsets.shape, R_SUM), state, x0, step)
                        obst = np.full((B, N + 1, 6), np.nan)
                        pcl, pnear, pchosen = np.full(B, np.nan), np.full(B, -7, np.int32), np.full((B, N + 1, 3), -7, np.int32)
                        sessx.sessx_traffic(0, B, nx, N, M, per_ego, pairing, EGO_OFFSET, _dp(DESC), _dp(obs), _dp(offsets), _dp(state), _dp(x0), R_SUM, DT,
                                            step, _dp(obst), _dp(pcl), _ip(pnear), _ip(pchosen))
                        assert same((eq[0][:, :, :6], eq[1], eq[2], eq[3]), (obst, pcl, pnear, pchosen)), (M, Lt, per_ego, pairing, step)
                        assert np.all(eq[0][:, :, 6:9] == R_SUM) and np.all(eq[0][:, :, 9] == 0.0)
    print(f"N = {N}, nx = {nx}: {t.compared} indices compared, {t.left_out} left out by the margin rule ({100.0 * t.left_out / t.compared:.3f} %)")
    assert t.left_out < 0.01 * t.compared


# ---- the Python layers without a GPU: what they hand over, what they refuse ------------------------------------------------------------------------
def _fake_solver(N=10):
    s = object.__new__(pkg.BatchedMPCSolver)
    s._lib, s._h, s.N, s.nx = tl._FakeLib(), C.c_void_p(1), N, 5
    s.n_w, s.n_g = 2 * N + 5 * (N + 1), 1 + 14 * (N + 1)
    s._sens_gen, s._bounds_key = 0, None
    return s


def test_python_layers_hand_sizes_and_predictions_over_and_refuse_without_a_gpu():
    """session(rsums=) calls mpc_session_begin_sized with rsums behind offsets, None today's mpc_session_begin with today's arguments;
    step(predicted=) calls mpc_session_step_pred and step_device(d_pred=) mpc_session_step_pred_dev with the poses in the place of obs, without them
    today's calls; rsums of another shape or without offsets, and obstacles together with predicted, raise MpcError(MPC_ERR_INVALID) before any
    library call; CasadiOptimizer.open_session() with obstacle_radii = "own" hands every obstacle's own radius sum while lbg keeps the largest,
    "largest" and an unset value hand none"""
    s = _fake_solver()
    N, B, L = 10, 3, 12
    init, path, orient = np.zeros((B, 5)), np.zeros((B, L, 2)), np.zeros((B, L))
    rs = np.arange(1.0, 1.0 + 2 * B).reshape(B, 2)
    with s.session(init, path, orient, 10.0, L, offsets=np.ones((B, 2)), pairing=1, rsums=rs) as sess:
        assert (sess.M, sess.per_ego, sess.sized) == (2, 1, True)
        u, chosen = sess.step(predicted=np.zeros((B, 2, N + 1, 3)), outputs=("chosen",))
        assert u.shape == (B, 2) and chosen.shape == (B, N + 1, 3)
        sess.step(np.zeros((B, 5)), np.zeros((B, 2, 5)))
        sess.step(np.zeros((B, 5)), predicted=np.zeros((B, 2, N + 1, 3)))
        sess.step_device(11, d_pred=12, d_measured=13, d_chosen=14, stream=15)
        sess.step_device(11, d_obs=12)
        n_calls = len(s._lib.calls)
        for call in (lambda: sess.step(obstacles=np.zeros((B, 2, 5)), predicted=np.zeros((B, 2, N + 1, 3))), lambda: sess.step_device(11, d_obs=1, d_pred=2)):
            with pytest.raises(pkg.MpcError) as e:
                call()
            assert e.value.code == abi.MPC_ERR_INVALID and len(s._lib.calls) == n_calls
        with pytest.raises(ValueError):
            sess.step(predicted=np.zeros((B, 2, N, 3)))                      # (not [B, M, N+1, 3])
    with s.session(init, path, orient, 10.0, L, offsets=np.ones(4)) as plain:
        assert (plain.M, plain.per_ego, plain.sized) == (4, 0, False)
        plain.step(predicted=np.zeros((4, N + 1, 3)))
    names = [n for n, _ in s._lib.calls]
    assert names == ["mpc_session_begin_sized", "mpc_session_step_pred", "mpc_session_step", "mpc_session_step_pred", "mpc_session_step_pred_dev",
                     "mpc_session_step_dev", "mpc_session_end", "mpc_session_begin", "mpc_session_step_pred", "mpc_session_end"]
    args = [a for _, a in s._lib.calls]
    b0, b1 = args[0], args[7]
    assert len(b0) == 13 and len(b1) == 12 and b0[1:4] == (B, L, L) and b0[8:10] == (2, 1) and b0[12] == 1 and b1[8:10] == (4, 0) and b1[11] == 0
    assert np.array_equal(np.ctypeslib.as_array(b0[11], (2 * B,)), rs.ravel()) and np.all(np.ctypeslib.as_array(b0[10], (2 * B,)) == 1.0)
    p0, o0, p1 = args[1], args[2], args[3]
    assert len(p0) == len(o0) == 9 and p0[1] is None and p0[2] is not None and p0[3] is not None and p0[4] is None and p0[8] is not None
    assert p1[1] is not None and np.ctypeslib.as_array(p0[2], (B * 2 * (N + 1) * 3,)).shape == (198,)
    d_pred, d_obs = args[4], args[5]
    assert [a.value for a in d_pred[1:]] == [13, 12, 11, None, None, None, None, 14, 15] and [a.value for a in d_obs[1:4]] == [None, 12, 11]
    assert s._sens_gen == 6
    for kw in (dict(offsets=np.ones((B, 2)), rsums=np.ones((B, 3))), dict(offsets=np.ones((B, 2)), rsums=np.ones(2)), dict(rsums=np.ones(2))):
        n_calls = len(s._lib.calls)
        with pytest.raises(pkg.MpcError) as e:
            s.session(init, path, orient, 10.0, L, **kw)
        assert e.value.code == abi.MPC_ERR_INVALID and len(s._lib.calls) == n_calls
    # CasadiOptimizer.open_session()
    opt = pkg.optimizer
    Lr = 20
    pth, ori = straight_path(Lr, 0.0, 0.0, 0.0, 10.0)
    sizes = np.array([[4.0, 1.8], [12.0, 2.5], [0.6, 0.6]])                      # a car, a truck, a pedestrian
    radii = np.array([opt.compute_approximating_circle_radius(l, w)[0] for l, w in sizes])

    def opened(radii_opt):
        conf = make_configuration(pth, ori, 10.0, WEIGHTS_YAML_ZAM_LF, use_case="collision_avoidance",
                                  obstacle=dict(position_x=25.0, position_y=3.0, length=4.0, width=1.8, orientation=0.0))
        conf.obstacle_sizes, conf.obstacle_pairing = sizes, 1
        if radii_opt is not None:
            conf.obstacle_radii = radii_opt
        o = opt.CasadiOptimizer(configuration=conf, init_values=(np.array([1.0, 2.0]), 10.0, 0.0, 0.3), predict_horizon=N)
        be = _fake_solver(N)
        o._sol = opt.NlpSolverHandle(be)
        with o.open_session() as sess:
            assert sess.step(predicted=np.zeros((3, N + 1, 3))).shape == (1, 2)
        (n0, a0), (n1, a1), (n2, _) = be._lib.calls[:3]
        assert (n0, n2) == ("mpc_set_bounds", "mpc_session_step_pred")
        lbg = np.ctypeslib.as_array(a0[3], (be.n_g,))
        assert np.all(lbg[-9 * (N + 1):] == o.radius_ego + radii.max())
        return o, n1, a1

    o, name, a = opened("own")
    assert name == "mpc_session_begin_sized" and a[8:10] == (3, 0) and a[12] == 1
    assert np.array_equal(np.ctypeslib.as_array(a[11], (3,)), radii + o.radius_ego) and radii.max() - radii.min() > 0.5
    assert np.array_equal(np.ctypeslib.as_array(a[10], (3,)), [opt.compute_approximating_circle_radius(l, w)[1] / 4 for l, w in sizes])
    for radii_opt in (None, "largest"):
        o, name, a = opened(radii_opt)
        assert name == "mpc_session_begin" and len(a) == 12 and a[8:10] == (3, 0) and a[11] == 1 and o.obstacle_rsums is None
