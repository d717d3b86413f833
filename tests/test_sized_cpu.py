"""CPU: the pieces of the sized solve (mpc_solve_batch_sized: a lower bound per circle row) that need no GPU.

tests/sizedx/sizedx.cpp calls what the kernels run -- sized_pack, the sized transposer's element functions in the order k_transpose_obst_sized
steps them, load_obst in sized mode, plan_solve with the sized mode, and the emulated solve instantiated for VM_SIZED -- on the CPU, from the
shipped headers.  The reference of the GPU tests (tests/sized_ref.py: the oracle's NLP with the rows' own bounds, solved by the oracle's dense
interior-point method) is checked here too: what those tests presuppose about it."""
import ctypes as C
import os

import numpy as np
import pytest

import pred_obst_ref as ref
import sized_ref as sref
from helpers import ROOT, abi, emu_desc, harness_lib, kkt_certificate
from oracle.nlp_numpy import BicycleNLP
from test_solve_plan import CFGS, N_CU, ROWS, XCD_MASK, bounds_of
from test_solve_plan_stages import FIELDS, PER_STAGE, plan_fields

_dp = abi.as_dp
NEW = ("mpc_solve_batch_sized", "mpc_solve_batch_sized_dev", "mpc_closed_loop_batch_traffic_sized", "mpc_closed_loop_batch_traffic_sized_dev")
SIZED = 3


def test_new_entry_points_declared_and_exported():
    """declared in the header, exported by the library, prototyped as `_stages` plus one pointer behind obst"""
    hdr = open(os.path.join(ROOT, "include", "mpcgpu.h")).read()
    L = C.CDLL(abi.LIB_PATH)
    for s in NEW:
        assert s in abi.EXPORTS and hasattr(L, s) and ("int " + s + "(") in hdr, s
    P = abi.PROTOTYPES
    st, sd = P["mpc_solve_batch_stages"], P["mpc_solve_batch_stages_dev"]
    assert P["mpc_solve_batch_sized"] == st[:5] + [C.POINTER(C.c_double)] + st[5:]
    assert P["mpc_solve_batch_sized_dev"] == sd[:5] + [C.c_void_p] + sd[5:]
    # the arguments of the traffic loop plus rsums behind offsets
    tr, td = P["mpc_closed_loop_batch_traffic"], P["mpc_closed_loop_batch_traffic_dev"]
    assert P["mpc_closed_loop_batch_traffic_sized"] == tr[:13] + [C.POINTER(C.c_double)] + tr[13:]
    assert P["mpc_closed_loop_batch_traffic_sized_dev"] == td[:13] + [C.c_void_p] + td[13:]


@pytest.fixture(scope="module")
def sizedx():
    L = C.CDLL(harness_lib("sizedx"))
    dp, ip, i64p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    L.sizedx_ws_total.argtypes = [C.c_int32] * 3
    L.sizedx_ws_total.restype = C.c_int64
    L.sizedx_obst_index.argtypes = [C.c_int32] * 5
    L.sizedx_obst_index.restype = C.c_int64
    L.sizedx_layouts.argtypes = [C.c_int32] * 4 + [i64p]
    L.sizedx_layouts.restype = None
    L.sizedx_transpose.argtypes = [C.c_int32] * 5 + [dp, dp, C.c_double, C.c_double, dp]
    L.sizedx_transpose.restype = None
    L.sizedx_load.argtypes = [C.c_int32] * 3 + [dp, dp]
    L.sizedx_load.restype = None
    L.sizedx_relax_lo.argtypes = [C.c_double]
    L.sizedx_relax_lo.restype = C.c_double
    L.sizedx_solve.argtypes = [C.POINTER(abi.MpcProblemDesc)] + [dp] * 4 + [C.c_int32] + [dp] * 5 + [ip, ip, dp]
    T = C.CDLL(harness_lib("trafx"))
    T.trafx_solve_stages.argtypes = [C.POINTER(abi.MpcProblemDesc)] + [dp] * 4 + [C.c_int32] + [dp] * 4 + [ip, ip, dp]
    L.stages_sibling = T.trafx_solve_stages
    L.sizedx_traffic_step.argtypes = [C.c_int32] * 9 + [C.c_double] + [dp] * 6 + [C.c_double, C.c_int32, dp, dp, ip, ip]
    L.sizedx_traffic_step.restype = None
    L.sizedx_solve_plan.argtypes = [C.POINTER(abi.MpcProblemDesc)] + [dp] * 4 + [C.POINTER(C.c_char_p)] * 2 + [C.c_int32, i64p, C.c_int32, i64p]
    return L


# ---- k_sized_pack + k_transpose_obst_sized, load_obst<SIZED> ------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 31, 63, 127])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_sized_transposer_index_map(sizedx, B, N):
    """every (b, k, i) of obst and every (b, k, j) of rsum lands where the sized load reads it -- rows R k + i and R k + 6 + j of the section, R =
    OBST_SIZED_ROWS, the scale on row R k + 9 --, nothing else of the workspace is written, and the block's thread loop in ascending and in
    descending order, and with another block size, gives the same rows.  The offsets are relax_lo(rsum) - relax_lo(ol_raw), to rounding, and
    exactly 0.0 where rsum is ol_raw; load_obst hands a stage thread the six centres and offset x scale."""
    nx = 5 + (B + N) % 2
    R = sizedx.sizedx_rows_per_stage()
    assert R == 10
    rng = np.random.default_rng(B * 1000 + N)
    S = N + 1
    obst = np.ascontiguousarray(rng.uniform(-50, 50, (B, S, 6)))
    rsum = np.ascontiguousarray(rng.uniform(0.5, 4.0, (B, S, 3)))
    ol_raw = 3.3
    rsum[:, ::2, 1] = ol_raw                                     # (some rows with the handle's own bound)
    total = sizedx.sizedx_ws_total(N, nx, B)
    outs = []
    for desc, threads in ((0, 256), (1, 256), (0, 64)):
        ws = np.full(total, np.nan)
        sizedx.sizedx_transpose(N, nx, B, desc, threads, _dp(obst), _dp(rsum), ol_raw, 0.7, _dp(ws))
        outs.append(ws)
    assert np.array_equal(outs[0], outs[1], equal_nan=True) and np.array_equal(outs[0], outs[2], equal_nan=True)
    out = np.zeros(12, np.int64)
    sizedx.sizedx_layouts(N, nx, B, 0, out.ctypes.data_as(C.POINTER(C.c_int64)))
    tile_elems, o_row = int(out[9]), int(out[11])
    assert int(out[8]) == o_row + R * S and int(out[3]) == int(out[7]) == o_row            # (the section is the last, and starts where it did)
    b, r = np.arange(B)[:, None], np.arange(R * S)[None, :]
    e = (b >> 6) * tile_elems + (o_row + (r & ~1)) * 64 + (r & 1) + 2 * (b & 63)           # the pair layout, every instance by formula
    for bb in (0, B - 1, min(B - 1, 64)):
        for rr in (0, 7, R * S - 1):
            assert sizedx.sizedx_obst_index(N, nx, B, rr, bb) == e[bb, rr]
    got = outs[0][e].reshape(B, S, R)
    assert np.array_equal(got[:, :, :6], obst)
    od = np.array([[[sizedx.sizedx_relax_lo(v) for v in row] for row in inst] for inst in rsum]) - sizedx.sizedx_relax_lo(ol_raw)
    assert np.abs(got[:, :, 6:9] - od).max() <= 4e-16 * 4.0
    assert np.all(got[:, ::2, 7] == 0.0)
    assert np.all(got[:, :, 9] == 0.7)
    written = ~np.isnan(outs[0])
    assert written.sum() == B * S * R and np.array_equal(np.flatnonzero(written), np.sort(e.ravel()))
    held = np.full((B, S, 9), np.nan)
    sizedx.sizedx_load(N, nx, B, _dp(outs[0]), _dp(held))
    assert np.array_equal(held[:, :, :6], obst) and np.array_equal(held[:, :, 6:], got[:, :, 6:9] * 0.7)


def test_a_non_finite_radius_gives_a_nan_offset_in_its_row_only(sizedx):
    B, N, nx = 3, 4, 5
    obst = np.zeros((B, N + 1, 6))
    rsum = np.full((B, N + 1, 3), 2.0)
    rsum[1, 2, 0], rsum[1, 3, 2] = np.nan, np.inf
    ws = np.full(sizedx.sizedx_ws_total(N, nx, B), np.nan)
    sizedx.sizedx_transpose(N, nx, B, 0, 256, _dp(obst), _dp(rsum), 3.3, 1.0, _dp(ws))
    held = np.zeros((B, N + 1, 9))
    sizedx.sizedx_load(N, nx, B, _dp(ws), _dp(held))
    bad = np.isnan(held[:, :, 6:])
    assert bad.sum() == 2 and bad[1, 2, 0] and bad[1, 3, 2]


# ---- the launch plan ----------------------------------------------------------------------------------------------------------------------------
def sized_plan(L, fam, B, opts, state, mode):
    opts = dict(opts)
    d = emu_desc(CFGS[fam], fixed_iters=int(opts.pop("fixed_iters", 0)))
    lbg, ubg, lbx, ubx = bounds_of(fam)
    names = (C.c_char_p * max(1, len(opts)))(*[k.encode() for k in opts])
    values = (C.c_char_p * max(1, len(opts)))(*[str(v).encode() for v in opts.values()])
    st = dict(dict(resc_hint=0, trace=0, in_rescue=0), **state)
    i64p = C.POINTER(C.c_int64)
    assert L.sizedx_plan_fields() == len(FIELDS) + 1
    sv = np.array([N_CU, XCD_MASK, -1, 0, st["resc_hint"], B, 0, st["trace"], st["in_rescue"], 0], np.int64)
    out = np.zeros(len(FIELDS) + 1, np.int64)
    assert L.sizedx_solve_plan(C.byref(d), _dp(lbx), _dp(ubx), _dp(lbg), _dp(ubg), names, values, len(opts), sv.ctypes.data_as(i64p), mode,
                               out.ctypes.data_as(i64p)) == 0
    return dict(zip(FIELDS + ("sized",), (int(v) for v in out)))


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_sized_plan_is_the_per_stage_plan_with_the_sized_kernels(sizedx, row):
    """pure: over the shapes tests/test_solve_plan.py sweeps, the plan of a sized solve is the plan of a per-stage solve field by field -- the
    same path, grid, LDS and chunks -- and says `sized`, which picks the VM_SIZED instantiations; no other mode says it, and a sized plan is
    never `masked`"""
    _, fam, B, opts, state, _ = row
    stg = plan_fields(fam, B, opts, state, PER_STAGE)
    szd = sized_plan(sizedx, fam, B, opts, state, SIZED)
    for f in FIELDS:
        assert szd[f] == stg[f], (row[0], f)
    assert szd["sized"] == 1 and szd["masked"] == 0
    for mode in (0, 1, PER_STAGE):
        assert sized_plan(sizedx, fam, B, opts, state, mode)["sized"] == 0


# ---- the reference ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,N", sref.FAMILIES)
def test_the_reference_of_the_gpu_tests(name, N):
    """at least MIN_CONVERGED of SEEDS references converge per family; the reference's own optima pass the certificate at 1e-6 / 1e-6 with the
    instance's own bounds; they differ from the equal-radius optimum by more than 1e-3 (the radii matter) and a circle row is active on most"""
    d = sref.family(name, N)
    cfg = ref.cfg_for(N)
    n = len(d["x_ref"])
    print(f"{name} N={N}: reference converged on {n} of {d['tried']}, a circle row active on {int(d['active'].sum())}")
    assert n >= sref.MIN_CONVERGED
    have = ~np.isnan(d["x_equal"][:, 0])
    diff = np.abs(d["x_ref"] - d["x_equal"]).max(axis=1)[have]
    print(f"    min |x_ref - x_equal| = {diff.min():.3e} over {int(have.sum())}")
    assert diff.min() > 1e-3
    for i in range(n):
        nlp = sref.SizedNLP(cfg, d["stages"][i], d["radii"][i])
        c = kkt_certificate(nlp, d["x_ref"][i], d["p"][i], bounds=nlp.bounds())
        assert c["stationarity"] <= 1e-6 and c["feasibility"] <= 1e-6, (i, c)


# ---- the emulated solve in sized mode -----------------------------------------------------------------------------------------------------------
def emu_solve(L, cfg, sized, x0, p, st, rad):
    B = x0.shape[0]
    d = emu_desc(cfg)
    lbg, ubg, lbx, ubx = BicycleNLP(cfg).bounds()
    out, status, iters, kkt = np.empty_like(x0), np.empty(B, np.int32), np.empty(B, np.int32), np.empty(B)
    st, rad = np.ascontiguousarray(st, dtype=np.float64), np.ascontiguousarray(rad, dtype=np.float64)
    head, tail = (C.byref(d), _dp(lbx), _dp(ubx), _dp(lbg), _dp(ubg), B, _dp(x0), _dp(p), _dp(st)), (_dp(out), abi.as_ip(status), abi.as_ip(iters), _dp(kkt))
    assert (L.sizedx_solve(*head, _dp(rad), *tail) if sized else L.stages_sibling(*head, *tail)) == 0
    return out, status, iters, kkt


@pytest.mark.parametrize("N,nx", [(2, 6), (10, 5)])
def test_emulated_equal_radii_give_the_bits_of_stage_mode(sizedx, N, nx):
    parts = (("lead", N),) if N == 2 else (("lead", N), ("drift", N))
    cfg = ref.cfg_for(N, nx)
    inst = [ref.instance(name, n_, seed, nx) for name, n_ in parts for seed in range(5)]
    x0, p, st = (np.ascontiguousarray(np.array([q[i] for q in inst])) for i in range(3))
    B = x0.shape[0]
    rad = np.full((B, N + 1, 3), cfg.r_sum)
    a = emu_solve(sizedx, cfg, 0, x0, p, st.reshape(B, N + 1, 6), rad)
    b = emu_solve(sizedx, cfg, 1, x0, p, st.reshape(B, N + 1, 6), rad)
    for u, v in zip(a, b):
        assert np.array_equal(u, v, equal_nan=True)
    assert (a[1] == 1).sum() >= B // 2


def test_emulated_non_finite_radius_ends_its_own_instance(sizedx):
    """what the device form of the entry point relies on (it does not read rsum back): a NaN or an infinite entry ends that instance with
    status -6; every other instance has the bits it has without it"""
    d = sref.batch((("drift", 10),))
    cfg = ref.cfg_for(10)
    a = emu_solve(sizedx, cfg, 1, d["x0"], d["p"], d["stages"], d["radii"])
    B = len(a[1])
    for bad in (np.nan, np.inf):
        rad = d["radii"].copy()
        rad[B // 2, 3, 1] = bad
        b = emu_solve(sizedx, cfg, 1, d["x0"], d["p"], d["stages"], rad)
        keep = np.arange(B) != B // 2
        assert b[1][B // 2] == -6
        assert np.array_equal(a[0][keep], b[0][keep]) and np.array_equal(a[1][keep], b[1][keep])


@pytest.mark.parametrize("N", [2, 3, 4, 7, 10])
def test_emulated_solve_against_the_reference(sizedx, N):
    """status 1 wherever the reference converged, |x - x_ref| <= 1e-4: the bound DESIGN.md section 2 gives for two interior-point methods on
    one NLP"""
    parts = tuple(q for q in sref.FAMILIES if q[1] == N)
    d = sref.batch(parts)
    cfg = ref.cfg_for(N)
    x, status, iters, _ = emu_solve(sizedx, cfg, 1, d["x0"], d["p"], d["stages"], d["radii"])
    err = np.abs(x - d["x_ref"]).max(axis=1)
    print(f"N={N} {parts}: status 1 on {int((status == 1).sum())} of {len(status)}, max |x - x_ref| = {err.max():.3e}, iterations max {iters.max()}")
    assert np.all(status == 1)
    assert err.max() <= 1e-4


# ---- the selection with radii, in numpy (optimizer.nearest_obstacle_centres) ---------------------------------------------------------------------
def _brute(poses, tracks, offsets, rows, ego_offset, pairing, default, rsums, r_default):
    """restated without the incremental minimum: all keys of a stage, then argmin (ties: the lowest obstacle, then the lowest circle)"""
    K, M = len(poses), len(tracks)
    cen, chosen, rad = np.tile(np.asarray(default, float), (K, 1)).reshape(K, 3, 2), np.full((K, 3), -1, np.int32), np.full((K, 3), r_default)

    def circ(x, y, th, off):
        return np.array([[x, y], [x + off * np.cos(th), y + off * np.sin(th)], [x - off * np.cos(th), y - off * np.sin(th)]])
    for k in range(K):
        E = circ(*poses[k], ego_offset)
        present = [m for m in range(M) if np.isfinite(tracks[m][rows[k]][0])]
        if not present:
            continue
        O = {m: circ(*tracks[m][rows[k]], offsets[m]) for m in present}
        if pairing == 0:
            keys = [min(np.hypot(*(E[j] - O[m][j])) for j in range(3)) - (rsums[m] - r_default) for m in present]
            m = present[int(np.argmin(keys))]
            cen[k], chosen[k], rad[k] = O[m], m, rsums[m]
        else:
            for j in range(3):
                keys = [(np.hypot(*(E[j] - O[m][c])) - (rsums[m] - r_default), m, c) for m in present for c in range(3)]
                _, m, c = min(keys, key=lambda q: q[0])
                cen[k, j], chosen[k, j], rad[k, j] = O[m][c], m, rsums[m]
    return cen.reshape(K, 6), chosen, rad


@pytest.mark.parametrize("pairing", [0, 1])
@pytest.mark.parametrize("M", [1, 2, 5])
@pytest.mark.parametrize("N", [1, 2, 3, 10])
def test_selection_by_clearance_in_numpy(N, M, pairing):
    """every stage against the restatement, radii spread 0.5 .. 4 m, absent spans; equal radii give the call without radii; and a scene where the
    nearest obstacle by distance is not the nearest by clearance"""
    from helpers import pkg
    sel = pkg.optimizer.nearest_obstacle_centres
    rng = np.random.default_rng(100 * N + 10 * M + pairing)
    K, Lt, r0 = N + 1, N + 4, 3.3
    poses = np.column_stack([np.linspace(0, 3 * N, K), rng.uniform(-1, 1, K), rng.uniform(-0.2, 0.2, K)])
    tracks = np.stack([np.column_stack([rng.uniform(-5, 3 * N + 5, Lt), rng.uniform(-8, 8, Lt), rng.uniform(-3, 3, Lt)]) for _ in range(M)])
    if M > 1:
        tracks[1, Lt // 2:, 0] = np.nan                          # an absent span
    offsets, rsums = rng.uniform(0.0, 2.0, M), rng.uniform(0.5, 4.0, M)
    rows = np.minimum(np.arange(K) + 1, Lt - 1)
    default = np.arange(6.0) + 100.0
    got = sel(poses, tracks, offsets, rows, 0.75, pairing, default, rsums=rsums, r_default=r0)
    want = _brute(poses, tracks, offsets, rows, 0.75, pairing, default, rsums, r0)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    plain = sel(poses, tracks, offsets, rows, 0.75, pairing, default)
    same = sel(poses, tracks, offsets, rows, 0.75, pairing, default, rsums=np.full(M, r0), r_default=r0)
    assert np.array_equal(plain[0], same[0]) and np.array_equal(plain[1], same[1]) and np.all(same[2] == r0)


def test_nearest_by_distance_is_not_nearest_by_clearance():
    from helpers import pkg
    sel = pkg.optimizer.nearest_obstacle_centres
    poses = np.array([[0.0, 0.0, 0.0]])
    tracks = np.array([[[0.0, 6.0, 0.0]], [[0.0, -7.0, 0.0]]])              # A 6 m to the left, B 7 m to the right
    args = (poses, tracks, np.array([1.0, 1.0]), np.array([0]), 0.75, 0, np.zeros(6))
    assert sel(*args)[1][0, 0] == 0                                          # by distance: A
    c, chosen, rad = sel(*args, rsums=np.array([1.0, 4.0]), r_default=3.3)   # a pedestrian and a truck: B's clearance is 3.0, A's 5.0
    assert chosen[0, 0] == 1 and np.all(rad[0] == 4.0) and c[0, 1] == -7.0


# ---- k_loop_traffic_sized: the selection by clearance on the kernel's own function ---------------------------------------------------------------
def _traffic_step(sizedx, descending, B, L, Lt, nx, N, M, per_ego, pairing, tracks, offsets, rsums, state, x0, i, r_handle):
    import test_loop_traffic_cpu as tl
    rows = np.full((B, N + 1, 10), np.nan)
    cl, near, chosen = np.full((B, L), np.nan), np.full((B, L), -7, np.int32), np.full((B, L, N + 1, 3), -7, np.int32)
    sizedx.sizedx_traffic_step(descending, B, L, Lt, nx, N, M, per_ego, pairing, tl.EGO_OFFSET, _dp(tl.DESC), _dp(tracks), _dp(offsets), _dp(rsums),
                               _dp(state), _dp(x0), r_handle, i, _dp(rows), _dp(cl), abi.as_ip(near), abi.as_ip(chosen))
    return rows, cl, near, chosen


@pytest.mark.parametrize("N", [1, 2, 3, 10])
def test_sized_selection_against_numpy_without_the_cull(sizedx, N):
    """loop_traffic_stage_sized, what the threads of k_loop_traffic_sized do, for every (b, k, i): M in {1, 2, 5}, Lt in {1, L, L + N}, tracks shared
    and per ego, both pairings, absent spans, radii spread 0.5 .. 4 m, against tests/sized_ref.py's restatement, which looks at every obstacle (the
    cull must give the same).  Rows to 1e-12, the slots' radii exactly, indices wherever the margin between the best candidate and the runner-up
    exceeds 1e-9 m; both thread orders; and with every radius the handle's: loop_traffic_place's rows, chosen, clearance and nearest EXACTLY"""
    import test_loop_traffic_cpu as tl
    import traffic_ref as tref
    nx = 5 + N % 2
    rng = np.random.default_rng(1900 + N)
    trafx = C.CDLL(harness_lib("trafx"))
    trafx.trafx_step.argtypes = [C.c_int32] * 9 + [C.c_double] + [C.POINTER(C.c_double)] * 5 + [C.c_double, C.c_int32] + [C.POINTER(C.c_double)] * 2 + [C.POINTER(C.c_int32)] * 2
    trafx.trafx_step.restype = None
    B, L, r0 = 5, 6, tl.R_SUM
    nw = 2 * N + nx * (N + 1)
    compared = left_out = differ = 0
    for M in (1, 2, 5):
        for Lt in (1, L, L + N):
            for per_ego in (0, 1):
                tracks, offsets = tl._scene(rng, B, L, Lt, M, per_ego)
                rsums = np.ascontiguousarray(rng.uniform(0.5, 4.0, offsets.shape))
                state = np.ascontiguousarray(rng.uniform(-30.0, 30.0, (B, nx)))
                x0 = np.ascontiguousarray(rng.uniform(-30.0, 30.0, (B, nw)))
                for pairing in (0, 1):
                    for i in range(L):
                        rows, cl, near, chosen = _traffic_step(sizedx, 0, B, L, Lt, nx, N, M, per_ego, pairing, tracks, offsets, rsums, state, x0, i, r0)
                        back = _traffic_step(sizedx, 1, B, L, Lt, nx, N, M, per_ego, pairing, tracks, offsets, rsums, state, x0, i, r0)
                        for a, b in zip((rows, cl, near, chosen), back):
                            assert np.array_equal(a, b, equal_nan=True)
                        poses = tref.ego_poses(i, state, x0, N, nx)
                        want, w_rad, w_chosen, margin = sref.select_sized(i, poses, tracks, offsets, rsums, r0, pairing, tl.EGO_OFFSET, tl.DESC)
                        sure = margin > tref.MARGIN
                        assert np.abs(rows[:, :, :6] - want)[np.repeat(sure, 2, axis=2)].max(initial=0.0) <= 1e-12, (M, Lt, per_ego, pairing, i)
                        assert np.array_equal(rows[:, :, 6:9][sure], w_rad[sure]) and np.all(rows[:, :, 9] == 0.0)
                        assert np.array_equal(chosen[:, i][sure], w_chosen[sure])
                        w_cl, w_near, m_cl = sref.clearance_sized(i, state, tracks, offsets, rsums, tl.EGO_OFFSET)
                        fin = np.isfinite(w_cl)
                        assert np.array_equal(np.isfinite(cl[:, i]), fin) and np.all(cl[:, i][~fin] == np.inf)
                        assert np.abs(cl[:, i][fin] - w_cl[fin]).max(initial=0.0) <= 1e-12
                        assert np.array_equal(near[:, i][m_cl > tref.MARGIN], w_near[m_cl > tref.MARGIN])
                        compared += sure.size + m_cl.size
                        left_out += int((~sure).sum() + (m_cl <= tref.MARGIN).sum())
                        _, by_dist, _ = tref.select(i, poses, tracks, offsets, pairing, tl.EGO_OFFSET, tl.DESC)
                        differ += int((by_dist != w_chosen).sum())
                        assert np.isnan(np.delete(cl, i, axis=1)).all() and np.all(np.delete(near, i, axis=1) == -7) and np.all(np.delete(chosen, i, axis=1) == -7)
                        # every radius the handle's: the traffic loop's own function, exactly
                        eq = _traffic_step(sizedx, 0, B, L, Lt, nx, N, M, per_ego, pairing, tracks, offsets, np.full(offsets.shape, r0), state, x0, i, r0)
                        plain = tl._run(trafx, 0, B, L, Lt, nx, N, M, per_ego, pairing, tracks, offsets, state, x0, i)
                        assert np.array_equal(eq[0][:, :, :6], plain[0]) and np.all(eq[0][:, :, 6:9] == r0)
                        for a, b in zip(eq[1:], plain[1:]):
                            assert np.array_equal(a, b, equal_nan=True)
    print(f"N = {N}: {compared} indices compared, {left_out} left out by the margin rule, {differ} slots where clearance picks another obstacle than distance")
    assert left_out < 0.01 * compared and differ > 0


# ---- the Python layers without a GPU: what they hand over, what they refuse ------------------------------------------------------------------------
def test_python_layers_hand_the_radii_over_and_refuse_without_a_gpu():
    """BatchedMPCSolver.closed_loop_traffic(rsums=) / _device(d_rsums=) call the sized entries with rsums behind offsets, None / 0 today's entries;
    rsums of another shape, rsum without centres per stage, nearest_obstacle_centres(rsums=) without r_default and an unknown obstacle_radii are
    refused; CasadiOptimizer with obstacle_radii = "own" hands every obstacle's own radius sum to the loop, lbg keeps the largest, and "largest",
    the default, hands none"""
    import test_loop_traffic_cpu as tl
    from helpers import WEIGHTS_YAML_ZAM_LF, make_configuration, pkg, straight_path
    opt = pkg.optimizer
    s = object.__new__(pkg.BatchedMPCSolver)
    s._lib, s._h, s.N, s.nx = tl._FakeLib(), C.c_void_p(1), 10, 5
    s.n_w = 2 * 10 + 5 * 11
    s._sens_gen = s._sens_B = 0
    B, L = 3, 12
    init, path, orient = np.zeros((B, 5)), np.zeros((B, L, 2)), np.zeros((B, L))
    s.closed_loop_traffic(init, path, orient, 10.0, L, np.zeros((4, L, 3)), np.ones(4), pairing=1, rsums=np.full(4, 2.0))
    s.closed_loop_traffic(init, path, orient, 10.0, L, np.zeros((4, L, 3)), np.ones(4), pairing=1)
    s.closed_loop_traffic_device(B, 1, 2, 3, 4, L, L, 2, L, 0, 5, 6, 7, 8, pairing=1, d_rsums=11)
    s.closed_loop_traffic_device(B, 1, 2, 3, 4, L, L, 2, L, 0, 5, 6, 7, 8, pairing=1)
    names = [n for n, _ in s._lib.calls]
    assert names == ["mpc_closed_loop_batch_traffic_sized", "mpc_closed_loop_batch_traffic", "mpc_closed_loop_batch_traffic_sized_dev",
                     "mpc_closed_loop_batch_traffic_dev"]
    a0, a1, a2, a3 = (a for _, a in s._lib.calls)
    assert len(a0) == len(a1) + 1 and a0[8:11] == a1[8:11] == (4, L, 0) and a0[14] == a1[13] == 1 and len(a2) == len(a3) + 1 and a2[14] == a3[13] == 1 and a2[13].value == 11
    with pytest.raises(pkg.MpcError):
        s.closed_loop_traffic(init, path, orient, 10.0, L, np.zeros((4, L, 3)), np.ones(4), rsums=np.ones(3))
    with pytest.raises(pkg.MpcError):
        s.solve(np.zeros((B, s.n_w)), np.zeros((B, s.n_w)), np.zeros((B, 6)), rsum=np.ones((B, 11, 3)))
    with pytest.raises(pkg.MpcError):
        s.solve(np.zeros((B, s.n_w)), np.zeros((B, s.n_w)), np.zeros((B, 11, 6)), rsum=np.ones((B, 11, 2)))
    with pytest.raises(pkg.MpcError):
        s.solve_device(B, 1, 2, 3, d_rsum=5)
    with pytest.raises(ValueError):
        opt.nearest_obstacle_centres(np.zeros((2, 3)), np.zeros((1, 1, 3)), np.ones(1), np.zeros(2, int), 0.75, 0, np.zeros(6), rsums=np.ones(1))
    # CasadiOptimizer
    N = 10
    Lr = 20
    pth, ori = straight_path(Lr, 0.0, 0.0, 0.0, 10.0)
    sizes = np.array([[4.0, 1.8], [12.0, 2.5], [0.6, 0.6]])                      # a car, a truck, a pedestrian
    tracks = np.random.default_rng(0).uniform(-5, 5, (3, Lr, 3))

    def make(radii):
        conf = make_configuration(pth, ori, 10.0, WEIGHTS_YAML_ZAM_LF, use_case="collision_avoidance",
                                  obstacle=dict(position_x=25.0, position_y=3.0, length=4.0, width=1.8, orientation=0.0))
        conf.obstacle_tracks, conf.obstacle_sizes, conf.obstacle_pairing = tracks, sizes, 0
        if radii is not None:
            conf.obstacle_radii = radii
        o = opt.CasadiOptimizer(configuration=conf, init_values=(np.array([0.0, 0.0]), 10.0, 0.0, 0.0), predict_horizon=N)
        be = tl._TrafficBackend(N)
        o._sol = opt.NlpSolverHandle(be)
        return o, be
    radii = np.array([opt.compute_approximating_circle_radius(l, w)[0] for l, w in sizes])
    o, be = make("own")
    o.optimize()
    (call,) = be.calls
    assert np.array_equal(call["rsums"], radii + o.radius_ego) and radii.max() - radii.min() > 0.5
    assert np.all(np.asarray(be.bounds[2])[-9 * (N + 1):] == o.radius_ego + radii.max())
    # ... and its host loop's selection returns the slots' own radii
    placed = o.traffic_centres(0, np.zeros((N + 1, 3)))
    assert len(placed) == 3 and placed[2].shape == (N + 1, 3) and set(np.unique(placed[2])) <= set(radii + o.radius_ego)
    for radii_opt in (None, "largest"):
        o, be = make(radii_opt)
        o.optimize()
        assert "rsums" not in be.calls[0] and o.obstacle_rsums is None and len(o.traffic_centres(0, np.zeros((N + 1, 3)))) == 2
    with pytest.raises(ValueError):
        make("median")
