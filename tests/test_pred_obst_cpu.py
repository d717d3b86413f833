"""CPU: the pieces of the per-stage obstacle rows (mpc_solve_batch_stages, mpc_eval_nlp_batch_stages, mpc_closed_loop_batch_pred) that need
no GPU.

tests/predx/predx.cpp calls what the kernels run -- loop_obst_stage (k_loop_obst_stages), the transposer's element functions in the order
k_transpose_obst_stages steps them, load_obst in stage mode, nlp_eval_stage with a stage's own centres -- on the CPU, from the shipped
headers.  The reference of the GPU tests (tests/pred_obst_ref.py: the oracle's NLP subclassed to centres per stage, solved by the oracle's
dense interior-point method) is checked here too: what those tests presuppose about it."""
import ctypes as C
import os

import numpy as np
import pytest

import loop_obst_ref as lref
import pred_obst_ref as ref
from helpers import ROOT, abi, emu_desc, harness_lib, kkt_certificate, pkg
from oracle.nlp_numpy import BicycleNLP, synthetic_batch

_dp = abi.as_dp
NEW = ("mpc_solve_batch_stages", "mpc_solve_batch_stages_dev", "mpc_eval_nlp_batch_stages", "mpc_eval_nlp_batch_stages_dev",
       "mpc_closed_loop_batch_pred", "mpc_closed_loop_batch_pred_dev")


def test_new_entry_points_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mpcgpu.h")).read()
    L = C.CDLL(abi.LIB_PATH)
    for s in NEW:
        assert s in abi.EXPORTS and hasattr(L, s) and ("int " + s + "(") in hdr, s
    P = abi.PROTOTYPES
    assert P["mpc_solve_batch_stages"] == P["mpc_solve_batch_ex"] and P["mpc_solve_batch_stages_dev"] == P["mpc_solve_batch_dev_ex"]
    assert P["mpc_eval_nlp_batch_stages"] == P["mpc_eval_nlp_batch"] and P["mpc_eval_nlp_batch_stages_dev"] == P["mpc_eval_nlp_batch_dev"]
    # the arguments of the frozen loop plus `predict` behind obst_offset
    for a, b in (("mpc_closed_loop_batch_pred", "mpc_closed_loop_batch_obst"), ("mpc_closed_loop_batch_pred_dev", "mpc_closed_loop_batch_obst_dev")):
        assert P[a] == P[b][:11] + [C.c_int32] + P[b][11:]


@pytest.fixture(scope="module")
def predx():
    L = C.CDLL(harness_lib("predx"))
    dp, i64p = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    L.predx_loop_step.argtypes = [C.c_int32] * 6 + [C.c_double, dp, C.c_double, dp, C.c_double, C.c_int32, dp, dp]
    L.predx_loop_step.restype = None
    L.predx_ws_total.argtypes = [C.c_int32] * 3
    L.predx_ws_total.restype = C.c_int64
    L.predx_obst_index.argtypes = [C.c_int32] * 5
    L.predx_obst_index.restype = C.c_int64
    L.predx_layouts.argtypes = [C.c_int32] * 4 + [i64p]
    L.predx_layouts.restype = None
    L.predx_transpose.argtypes = [C.c_int32] * 5 + [dp, dp]
    L.predx_transpose.restype = None
    L.predx_load_obst.argtypes = [C.c_int32] * 4 + [dp, dp]
    L.predx_load_obst.restype = None
    L.predx_eval_stages.argtypes = [C.POINTER(abi.MpcProblemDesc), C.c_int32, dp, dp, dp, dp, dp]
    return L


# ---- k_loop_obst_stages ---------------------------------------------------------------------------------------------------------------------
def _centres(rows, offset):
    """[..., 3] poses -> [..., 6]: the centre, then +- offset along the heading (loop_obstacle_centres, operation for operation)"""
    cs, sn = np.cos(rows[..., 2]), np.sin(rows[..., 2])
    return np.stack([rows[..., 0], rows[..., 1], rows[..., 0] + offset * cs, rows[..., 1] + offset * sn, rows[..., 0] - offset * cs,
                     rows[..., 1] - offset * sn], axis=-1)


@pytest.mark.parametrize("nx", [5, 6])
@pytest.mark.parametrize("N", [1, 2, 3, 10])
def test_stage_rows_of_the_predicted_loop(predx, N, nx):
    """loop_obst_stage, what the threads of k_loop_obst_stages do: row (b, k) of the [B, N+1, 6] buffer from track row min(i + k, Lt - 1) for
    every (b, k, i) -- Lt = 1, L and L + N + 3, so that i + k crosses the end of the track and stays inside it --, clearance[b, i] from the
    state against track row min(i, Lt - 1) and nothing else of the clearance buffer; with predict 0 the rows of loop_obst_instance"""
    rng = np.random.default_rng(40 + N)
    B, L = 7, 6
    state = np.ascontiguousarray(rng.uniform(-3, 3, (B, nx)))
    for Lt in (1, L, L + N + 3):
        track = np.ascontiguousarray(rng.uniform(-10, 10, (B, Lt, 3)))
        if Lt == 1:
            track[:, :, 2] = 0.0                                                       # (heading 0: the centres are exact)
        for i in range(L):
            obst, cl = np.full((B, N + 1, 6), np.nan), np.full((B, L), np.nan)
            predx.predx_loop_step(1, B, L, Lt, nx, N, 0.75, _dp(track), 1.25, _dp(state), 3.3, i, _dp(obst), _dp(cl))
            rows = track[:, np.minimum(i + np.arange(N + 1), Lt - 1)]                  # [B, N+1, 3]
            # the centres are the track's numbers and one product and sum each: against the harness's own frozen rows, EXACTLY
            for k in range(N + 1):
                frozen = np.full((B, 6), np.nan)
                predx.predx_loop_step(0, B, L, Lt, nx, N, 0.75, _dp(track), 1.25, _dp(state), 3.3, min(i + k, Lt - 1), _dp(frozen), None)
                assert np.array_equal(obst[:, k], frozen), (Lt, i, k)
            assert np.abs(obst - _centres(rows, 1.25)).max() <= 1e-14                  # (numpy's cos / sin may differ from libm's in the last bit)
            if Lt == 1:
                assert np.array_equal(obst, _centres(rows, 1.25))                      # heading 0: exact
            want = lref.clearance_numpy(state[:, :5], obst[:, 0], 0.75, 3.3)
            assert np.abs(cl[:, i] - want).max() <= 1e-12
            assert np.isnan(np.delete(cl, i, axis=1)).all()
            # predict 0: the frozen rows, and the same clearance
            o0, c0 = np.full((B, 6), np.nan), np.full((B, L), np.nan)
            predx.predx_loop_step(0, B, L, Lt, nx, N, 0.75, _dp(track), 1.25, _dp(state), 3.3, i, _dp(o0), _dp(c0))
            assert np.array_equal(o0, obst[:, 0]) and np.array_equal(c0[:, i], cl[:, i])
            predx.predx_loop_step(1, B, L, Lt, nx, N, 0.75, _dp(track), 1.25, _dp(state), 3.3, i, _dp(obst), None)      # (no clearance asked for)


# ---- k_transpose_obst_stages ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 31, 63, 127])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_transposer_index_map(predx, B, N):
    """every (b, k, i) of obst [B, N+1, 6] lands on ws_index(row 6 k + i, b) of the obstacle section and nothing else of the workspace is
    written; the block's thread loop in ascending and in descending order, and with another block size, gives the same rows"""
    nx = 5 + (B + N) % 2
    rng = np.random.default_rng(B * 1000 + N)
    obst = np.ascontiguousarray(rng.uniform(-50, 50, (B, N + 1, 6)))
    total = predx.predx_ws_total(N, nx, B)
    outs = []
    for desc, threads in ((0, 256), (1, 256), (0, 64)):
        ws = np.full(total, np.nan)
        predx.predx_transpose(N, nx, B, desc, threads, _dp(obst), _dp(ws))
        outs.append(ws)
    assert np.array_equal(outs[0], outs[1], equal_nan=True) and np.array_equal(outs[0], outs[2], equal_nan=True)
    bs = (0, B - 1, B // 2, min(B - 1, 63), min(B - 1, 64)) if B * (N + 1) > 2000 else range(B)
    idx = np.array([[[predx.predx_obst_index(N, nx, B, 6 * k + i, b) for i in range(6)] for k in range(N + 1)] for b in bs])
    assert np.array_equal(outs[0][idx], obst[list(bs)])
    # ... and, for all of them at once: the written elements are a permutation of the input, nothing else was touched
    written = ~np.isnan(outs[0])
    assert written.sum() == obst.size and np.array_equal(np.sort(outs[0][written]), np.sort(obst.ravel()))
    if len(bs) < B:                                              # the map of the sampled instances is the pair layout: check every instance by formula
        out = np.zeros(8, np.int64)
        predx.predx_layouts(N, nx, B, 0, out.ctypes.data_as(C.POINTER(C.c_int64)))
        tile_elems, o_row = int(out[5]), int(out[7])
        b, r = np.arange(B)[:, None], np.arange(6 * (N + 1))[None, :]
        e = (b >> 6) * tile_elems + (o_row + (r & ~1)) * 64 + (r & 1) + 2 * (b & 63)
        assert np.array_equal(outs[0][e], obst.reshape(B, -1))


def test_workspace_keeps_its_layout_without_a_per_stage_call(predx):
    """ws_layout's flag: the obstacle section is the last of a tile -- without the flag the parent's rows, with it 6 N rows per instance more
    and every other section where it was"""
    for N, nx, B, mb in ((30, 6, 4096, 1), (10, 5, 65, 0), (127, 5, 64, 0)):
        out = np.zeros(8, np.int64)
        predx.predx_layouts(N, nx, B, mb, out.ctypes.data_as(C.POINTER(C.c_int64)))
        rows0, te0, tot0, o0, rows1, te1, tot1, o1 = (int(v) for v in out)
        assert o0 == o1 and rows0 == o0 + 6 and rows1 == o1 + 6 * (N + 1) and te1 - te0 == 6 * N * 64


@pytest.mark.parametrize("nx", [5, 6])
def test_stage_threads_read_their_own_rows(predx, nx):
    """load_obst as a stage thread (b, k) of the solve kernels calls it: per stage the rows the transposer left, per instance the instance's
    row at every stage, else the descriptor's centres"""
    rng = np.random.default_rng(3)
    for N, B in ((1, 1), (3, 65), (10, 130), (63, 70)):
        obst = np.ascontiguousarray(rng.uniform(-50, 50, (B, N + 1, 6)))
        out = np.full((B, N + 1, 6), np.nan)
        predx.predx_load_obst(N, nx, B, 2, _dp(obst), _dp(out))
        assert np.array_equal(out, obst)
        predx.predx_load_obst(N, nx, B, 1, _dp(np.ascontiguousarray(obst[:, 0])), _dp(out))
        assert np.array_equal(out, np.repeat(obst[:, :1], N + 1, axis=1))
        predx.predx_load_obst(N, nx, B, 0, None, _dp(out))
        assert np.array_equal(out, np.tile([-100.0, 0.0] * 3, (B, N + 1, 1)))


# ---- nlp_eval_stage with centres per stage ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [5, 6])
@pytest.mark.parametrize("N", [1, 2, 3, 10])
def test_eval_with_stage_centres_matches_the_staged_nlp(predx, N, nx):
    """f and g as k_eval_nlp computes them with obst [B, N+1, 6] against StagedNLP, to the tolerance tests/test_multipliers_cpu.py holds the
    same comparison with one obstacle to"""
    cfg = ref.cfg_for(N, nx)
    B = 6
    x0, p = synthetic_batch(cfg, B)
    rng = np.random.default_rng(17 + N)
    x = np.ascontiguousarray(x0 + rng.normal(0.0, 0.3, x0.shape))
    st = np.ascontiguousarray(x[:, None, 2 * N: 2 * N + 2].repeat(N + 1, 1).repeat(3, 2) + rng.uniform(-8.0, 8.0, (B, N + 1, 6)))
    f, g = np.empty(B), np.empty((B, cfg.n_g))
    d = emu_desc(cfg)
    assert predx.predx_eval_stages(C.byref(d), B, _dp(x), _dp(np.ascontiguousarray(p)), _dp(st), _dp(f), _dp(g)) == 0
    for b in range(B):
        nlp = ref.StagedNLP(cfg, st[b])
        fr, gr = nlp.f(x[b], p[b]), nlp.g(x[b], p[b])
        assert abs(f[b] - fr) <= 1e-13 * abs(fr)
        assert np.max(np.abs(g[b] - gr) / np.maximum(1.0, np.abs(gr))) <= 1e-13 * max(1.0, np.max(np.abs(x[b])))
    assert np.abs(np.diff(g[:, 1 + nx * (N + 1):].reshape(B, N + 1, 9), axis=1)).min() > 1e-3        # (every stage's rows differ)


# ---- the reference ----------------------------------------------------------------------------------------------------------------------------
def test_staged_nlp_with_identical_stages_is_the_oracles_nlp():
    cfg = ref.cfg_for(10)
    cfg.obstacle = (12.0, 1.0, 6.0, 3.5, 0.2)
    x0, p = synthetic_batch(cfg, 3)
    rng = np.random.default_rng(1)
    lam = rng.normal(0, 1, cfg.n_g)
    base = BicycleNLP(cfg)
    nlp = ref.StagedNLP(cfg, np.tile(cfg.obstacle_centers, (cfg.N + 1, 1, 1)))
    for b in range(3):
        w = x0[b] + rng.normal(0, 0.2, cfg.n_w)
        for _ in range(2):                                       # (twice: the stage counter starts over in every call)
            assert np.array_equal(nlp.g(w, p[b]), base.g(w, p[b])) and np.array_equal(nlp.jac(w, p[b]), base.jac(w, p[b]))
            assert np.array_equal(nlp.hess_lag(w, p[b], 0.7, lam), base.hess_lag(w, p[b], 0.7, lam))
        assert nlp.f(w, p[b]) == base.f(w, p[b]) and np.array_equal(nlp.grad(w, p[b]), base.grad(w, p[b]))


@pytest.mark.parametrize("N", [2, 10])
def test_staged_nlp_derivatives_against_central_differences(N):
    """jac and hess_lag of StagedNLP with distinct stages: central differences of g and of jac' lam (step 1e-6 on values of order 10: the
    truncation and round-off errors of the quotient are of order 1e-9 / 1e-6 = 1e-3 of the third derivative's scale -- 2e-6 holds with margin)"""
    x0, p, st = ref.instance("drift", N, 3)
    cfg = ref.cfg_for(N)
    nlp = ref.StagedNLP(cfg, st)
    rng = np.random.default_rng(2)
    w = x0 + rng.normal(0, 0.1, cfg.n_w)
    lam = rng.normal(0, 1, cfg.n_g)
    lam[0] = 0.0                                                 # (the friction row |y| has a kink; its derivatives are the parent's own)
    J, H = nlp.jac(w, p), nlp.hess_lag(w, p, 0.0, lam)
    h = 1e-6
    Jn, Hn = np.zeros_like(J), np.zeros_like(H)
    for i in range(cfg.n_w):
        e = np.zeros(cfg.n_w)
        e[i] = h
        Jn[:, i] = (nlp.g(w + e, p) - nlp.g(w - e, p)) / (2 * h)
        Hn[:, i] = (nlp.jac(w + e, p).T @ lam - nlp.jac(w - e, p).T @ lam) / (2 * h)
    rows = np.arange(1, cfg.n_g)
    assert np.abs(J[rows] - Jn[rows]).max() <= 2e-6 * max(1.0, np.abs(J).max())
    assert np.abs(H - Hn).max() <= 2e-6 * max(1.0, np.abs(H).max())


FAMILIES_USED = [("lead", 7), ("lead", 10), ("drift", 10), ("drift", 30), ("beside", 1), ("beside", 2), ("beside", 3), ("beside", 4)]


@pytest.mark.parametrize("name,N", FAMILIES_USED)
def test_reference_converges_on_the_families(name, N):
    """what the GPU tests presuppose: the dense method converges on at least 12 of the 16 instances of every (family, N) they use; the lead
    and drift families end with an active circle row, the beside family with none; without braking / steering the instances are as short of
    the distance as their description says"""
    d = ref.family(name, N)
    n = len(d["x0"])
    print(name, N, "converged", n, "of", d["tried"], "with an active row", int(d["active"].sum()))
    assert d["tried"] == ref.SEEDS and n >= ref.MIN_CONVERGED
    cfg = ref.cfg_for(N)
    unbraked = np.array([ref.clearance(cfg, d["p"][i][2 * N:].reshape(N + 1, 5), d["stages"][i]) for i in range(n)])
    if name == "beside":
        assert not d["active"].any() and unbraked.min() >= 0.2 - 1e-9 and unbraked.max() <= 0.8 + 1e-9
        assert np.abs(np.diff(d["stages"].reshape(n, N + 1, 6), axis=1)).max(axis=2).min() > 0.05      # every stage's centres differ
    else:
        assert d["active"].sum() >= ref.MIN_CONVERGED
        T2 = 2.0 * ((N - 1) * cfg.dt) ** 2
        lo, hi = (0.1 * T2, 0.3 * T2) if name == "lead" else (0.1, 0.4)
        assert np.all(unbraked[:, -1] <= -lo + 1e-9) and np.all(unbraked[:, -1] >= -hi - 1e-9)
        if name == "drift":
            assert np.abs(unbraked[:, 0] - 0.5).max() <= 1e-9
        opt = np.array([ref.clearance(cfg, d["x_ref"][i][2 * N:].reshape(N + 1, 5), d["stages"][i]).min() for i in range(n)])
        assert opt.min() >= -1e-7                                 # (the optima keep the distance, to the bound relaxation 1e-8 r_sum)
    # the reference's optima are KKT points by the certificate the GPU rows are held to, at the same thresholds -- from N = 3 on.  At N = 1, 2
    # the dense method stops earlier in these units (its tolerance applies to the scaled problem; measured: stationarity up to 7.1e-6, its x
    # 3.4e-5 from the kernels' rows, whose own certificate is at 1e-11): the figure is printed, and the GPU comparison keeps its 1e-4
    worst = 0.0
    for i in range(n):
        c = kkt_certificate(ref.StagedNLP(cfg, d["stages"][i]), d["x_ref"][i], d["p"][i])
        worst = max(worst, c["stationarity"])
        assert c["feasibility"] <= 1e-6 and (N < 3 or c["stationarity"] <= 1e-6), (i, c)
    print(name, N, "worst relative stationarity residual of the reference's optima:", worst)


def test_recorded_optima_are_the_references():
    """tests/golden/pred_obst_ref.npz (drift, N = 30: five seconds per instance): the recorded seeds are all sixteen, two instances solved again
    here give the recorded optimum to 1e-9, and every recorded row is feasible for its instance"""
    d = ref.family("drift", 30)
    assert list(d["seeds"]) == list(range(ref.SEEDS))
    cfg = ref.cfg_for(30)
    for i in (0, 11):
        x = ref.reference_solve("drift", 30, int(d["seeds"][i]))
        assert x is not None and np.abs(x - d["x_ref"][i]).max() <= 1e-9
    for i in range(len(d["x0"])):
        nlp = ref.StagedNLP(cfg, d["stages"][i])
        lbg, ubg, lbx, ubx = nlp.bounds()
        g = nlp.g(d["x_ref"][i], d["p"][i])
        assert max((lbg - g).max(), (g - ubg).max(), (lbx - d["x_ref"][i]).max(), (d["x_ref"][i] - ubx).max()) <= 1e-7


# ---- the Python layer, through a stand-in for the library ------------------------------------------------------------------------------------
class _FakeLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def _solver_without_gpu(N=10, nx=5):
    s = object.__new__(pkg.BatchedMPCSolver)
    s._lib, s._h, s.N, s.nx = _FakeLib(), C.c_void_p(1), N, nx
    s.n_w, s.n_g = 2 * N + nx * (N + 1), 1 + nx * (N + 1) + 9 * (N + 1)
    s._sens_gen = s._sens_B = 0
    return s


def test_solver_dispatches_on_the_shape_of_obst():
    s = _solver_without_gpu()
    B = 3
    x, p = np.zeros((B, s.n_w)), np.zeros((B, s.n_w))
    s.solve(x, p, np.zeros((B, 6)))
    s.solve(x, p, np.zeros((B, 11, 6)))
    s.solve(x, p, np.zeros((B, 11, 6)), multipliers=True)
    s.eval_nlp(x, p, np.zeros((B, 11, 6)))
    s.eval_nlp(x, p, np.zeros((B, 6)))
    s.solve_device(B, 1, 2, 3, d_obst=4, obst_stages=True)
    names = [c[0] for c in s._lib.calls]
    assert names == ["mpc_solve_batch", "mpc_solve_batch_stages", "mpc_solve_batch_stages", "mpc_eval_nlp_batch_stages", "mpc_eval_nlp_batch",
                     "mpc_solve_batch_stages_dev"]
    assert s._lib.calls[1][1][9:] == (None,) * 4 and all(a is not None for a in s._lib.calls[2][1][9:])
    gen = s._sens_gen
    assert gen == 3                                               # (each per-stage solve ends the life of a snapshot)
    for kw in (dict(lam_p=True), dict(dp=np.zeros((B, 1, s.n_w)))):
        with pytest.raises((pkg.MpcError, ValueError)):
            s.solve(x, p, np.zeros((B, 11, 6)), **kw)
    with pytest.raises(pkg.MpcError):
        s.solve(x, p, np.zeros((B, 10, 6)))
    with pytest.raises(pkg.MpcError):
        s.solve_device(B, 1, 2, 3, d_obst=4, obst_stages=True, d_lam_p=5)


def test_closed_loop_hands_predict_over():
    s = _solver_without_gpu()
    B, L = 3, 12
    init, path, orient = np.zeros((B, 5)), np.zeros((B, L, 2)), np.zeros((B, L))
    out = s.closed_loop(init, path, orient, 10.0, L, obst_track=np.zeros((B, L, 3)), obst_offset=1.0, clearance=True, predict=True)
    assert len(out) == 4 and out[3].shape == (B, L)
    s.closed_loop(init, path, orient, 10.0, L, obst_track=np.zeros((B, L, 3)), obst_offset=1.0)
    s.closed_loop_device(B, 1, 2, 3, 4, L, L, 5, 6, d_obst_track=7, Lt=L, predict=1)
    s.closed_loop_device(B, 1, 2, 3, 4, L, L, 5, 6, d_obst_track=7, Lt=L)
    (n0, a0), (n1, _), (n2, a2), (n3, _) = s._lib.calls
    assert (n0, n1, n2, n3) == ("mpc_closed_loop_batch_pred", "mpc_closed_loop_batch_obst", "mpc_closed_loop_batch_pred_dev", "mpc_closed_loop_batch_obst_dev")
    assert a0[8] == L and a0[10] == 1.0 and a0[11] == 1 and a0[18] is not None and a2[11] == 1
    for kw in (dict(predict=True), dict(predict=True, obst_track=np.zeros((B, L, 3)), linearize=True)):
        with pytest.raises(pkg.MpcError):
            s.closed_loop(init, path, orient, 10.0, L, **kw)
