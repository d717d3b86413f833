"""GPU: every kernel path at the points of tests/descriptor_families.py -- mpc_problem_desc away from dt = 0.1, wheelbase = 2.5789128,
friction_div = 2.578, ego_offset = 0.75, tol = 1e-8, obst_mult = 3, the one point every other GPU test builds its handle at.

The descriptor's scalars are read in hand-written places without a CPU twin (the MFMA Riccati sweeps, the fused start kernel's rollouts,
wg_restart, the compiled-in variant, the sensitivity, loop and FORCES kernels); a literal, wheelbase and friction_div swapped (3.5e-4 apart at
the defaults) or a value cached from another handle passes at the default point.  tests/test_descriptor_cpu.py shows from the oracle alone
that every point moves the optimum of most rows by more than 1e-3, so a path that ignores a field fails the 1e-8 below.

Lane-following points: status and iterations equal to the oracle's row for row, |x - x_oracle| < 1e-8, kkt <= tol (option rescue = 0: the
oracle has no second chance).  D6: the rule of test_collision_avoidance_batch (DF.assert_ca_rule)."""
import numpy as np
import pytest

import descriptor_families as DF
from helpers import make_solver, set_cfg_bounds

pytestmark = pytest.mark.gpu

TOL_ORACLE = 1e-8


def solver_for(pt, tol=1e-8, obst_mult=3, **opts):
    s = make_solver(pt.cfg, tol=tol, obst_mult=obst_mult)
    set_cfg_bounds(s, pt.cfg)
    if pt.kind != "ca":
        s.set_option("rescue", "0")
    for k, v in opts.items():
        s.set_option(k, v)
    return s


def same_bits(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("x", "status", "iters", "kkt"))


def solve_and_compare(pt, B, start=0, tol=1e-8, obst_mult=3, s=None, **opts):
    """one solve of point.inputs(B, start) on a handle with these options, at most 64 evenly spaced rows of it against the oracle"""
    s = s or solver_for(pt, tol, obst_mult, **opts)
    x0, p = pt.inputs(B, start)
    r = s.solve(x0, p)
    step = DF.step64(B)
    ro = DF.oracle_rows(pt, B, start=start, step=step, tol=tol, obst_mult=obst_mult)
    x, status, iters, kkt = r.x[::step], r.status[::step], r.iters[::step], r.kkt[::step]
    if pt.kind == "ca":
        DF.assert_ca_rule(pt.cfg, x, status, kkt, p[::step], ro, tol)
        return s, r
    err = np.abs(x - ro["x"]).max()
    print(f"{pt.name} B={B} tol={tol:g} obst_mult={obst_mult} {opts}: max |x - x_oracle| = {err:.2e}, kkt max {r.kkt.max():.2e}")
    assert np.array_equal(status, ro["status"]) and np.all(ro["status"] == 1)
    assert np.array_equal(iters, ro["iters"])
    assert err < TOL_ORACLE
    assert kkt.max() <= tol
    return s, r


# ---- the solve on every path ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", DF.CASES, ids=DF.case_id)
def test_default_path_k_solve_wg_alone(case):
    """B = 130 at default options: k_solve_wg serves the batch alone (the fused start kernel in front of it)"""
    name, tol, mult = case
    s, _ = solve_and_compare(DF.POINTS[name], 130, tol=tol, obst_mult=mult)
    assert s.get_resident_profile()["ran"] and not s.get_pipeline_profile()["ran"]


@pytest.mark.parametrize("name", ["D2", "D5", "D6"])
def test_one_launch_per_kernel(name):
    """hybrid = 0, pipeline = 0: k_stage / k_riccati, one launch each per iteration"""
    s, _ = solve_and_compare(DF.POINTS[name], 130, hybrid="0", pipeline="0")
    assert not s.get_resident_profile()["ran"] and not s.get_pipeline_profile()["ran"]


@pytest.mark.parametrize("name", ["D5", "D6"])
def test_variant_0_and_the_refusal_of_the_masked_variant(name):
    """bound_mask = 0: bounds and obstacle looked up at run time.  The compiled-in variant has the literal obst_mult 3, and the plan refuses it
    for any other value: at obst_mult = 1 the options bound_mask = 0 and 1 give the same bits."""
    pt = DF.POINTS[name]
    solve_and_compare(pt, 130, bound_mask="0")
    s, a = solve_and_compare(pt, 130, obst_mult=1, bound_mask="0")
    s.set_option("bound_mask", "1")
    x0, p = pt.inputs(130)
    assert same_bits(a, s.solve(x0, p))


def test_the_512_thread_path():
    """N = 64: the first horizon on the 512-thread kernels, one launch per kernel"""
    solve_and_compare(DF.N64, 66)


@pytest.mark.parametrize("N", DF.SHORT_HORIZONS)
def test_short_horizons_and_the_change_of_instances_per_workgroup(N):
    solve_and_compare(DF.POINTS["D5"].at(N), 65)


def test_persistent_pipeline_to_the_end():
    """hybrid = 0 at D30, B = 1088: k_pipeline (the MFMA Riccati workers, dt in their lane words) serves the batch to the end"""
    B, start = DF.D30_BATCHES["pipeline"]
    s, _ = solve_and_compare(DF.POINTS["D30"], B, start, hybrid="0")
    assert s.get_pipeline_profile()["ran"] and not s.get_resident_profile()["ran"]


def test_hybrid_hand_over():
    """default options at D30, B = 2305: the smallest batch the plan gives to both kernels on the 256 CUs of an MI355X (up to 36 tiles of 64, 9/8
    of the 2 x 1024 wavefront slots, k_solve_wg still serves alone: mpc_solve_plan.h) -- k_pipeline, then k_solve_wg on the tiles that left it"""
    B, start = DF.D30_BATCHES["hybrid"]
    s, _ = solve_and_compare(DF.POINTS["D30"], B, start)
    assert s.get_pipeline_profile()["ran"] and s.get_resident_profile()["ran"]


def test_abandoned_launch_is_replayed():
    """the test hook abandons every persistent launch: the solve starts over with one launch per kernel from the restart's own start point
    (wg_restart / k_start read dt and the wheelbase again)"""
    B, start = DF.D30_BATCHES["abort"]
    s, _ = solve_and_compare(DF.POINTS["D30"], B, start, hybrid="0", pipe_test_abort="1")
    assert s.get_option("pipe_aborts") >= 1


def test_second_chance_at_the_other_ego():
    """D6, instances 256 .. 511 (DF.D6_STALLED stall from their cold start in the oracle and in the emulated solve; no instance of 0 .. 255
    does at this ego): the levels behind the launch (rescue_wg = 0) and inside k_solve_wg (2) bring every row home to the tolerance of the
    original NLP, rescue the same number of instances and return the same bits"""
    pt = DF.POINTS["D6"]
    x0, p = pt.inputs(256, DF.D6_STALL_START)
    res, n = [], []
    for mode in ("0", "2"):
        s = solver_for(pt, rescue_wg=mode)
        res.append(s.solve(x0, p))
        n.append(s.last_rescued())
        print("rescue_wg", mode, "rescued", n[-1], "iterations of the stalled rows", res[-1].iters[[i - DF.D6_STALL_START for i in DF.D6_STALLED]])
        assert np.all(res[-1].status == 1) and res[-1].kkt.max() <= 1e-8
    assert n[0] == n[1] and n[0] > 0
    assert same_bits(res[0], res[1])
    ro = DF.oracle_rows(pt, 256, start=DF.D6_STALL_START, step=4)
    DF.assert_ca_rule(pt.cfg, res[0].x[::4], res[0].status[::4], res[0].kkt[::4], p[::4], ro)


def test_two_handles_in_one_process_keep_their_descriptors():
    """one handle at the defaults, one at D5, solving alternately: each result is the handle's first, bit for bit (nothing of a descriptor is
    cached per process), and each is its own oracle's"""
    p5 = DF.POINTS["D5"]
    pd = DF.D5_AT_DEFAULTS
    sa, ra = solve_and_compare(pd, 130)
    sb, rb = solve_and_compare(p5, 130)
    (xa, pa), (xb, pb) = pd.inputs(130), p5.inputs(130)
    for _ in range(3):
        assert same_bits(sa.solve(xa, pa), ra)
        assert same_bits(sb.solve(xb, pb), rb)


# ---- what hangs off a solve ------------------------------------------------------------------------------------------------------------------
from helpers import pkg                                          # noqa: E402
from oracle.binding import OracleSolver                          # noqa: E402
from oracle.nlp_numpy import BicycleNLP, NLPConfig               # noqa: E402


@pytest.mark.parametrize("name,mult", [(n, m) for n in ("D5", "D6") for m in (3, 1, 2)])
def test_multipliers_f_and_g(name, mult):
    """solve(..., multipliers=True) and eval_nlp: f, g against BicycleNLP(cfg) to the tolerances of test_against_the_reference in
    tests/test_gpu_solve_stages.py; the returned multipliers balance the numpy gradient and Jacobian of the point's NLP,
    |grad + J' lam_g + lam_x|_inf <= 1e-6 max(1, |grad|_inf).  With obst_mult = m the nine circle rows of a stage stay and the three copies of a
    row carry m nu / 3 each (nu: the multiplier of the distinct row at multiplicity 1), so the sum over J' lam_g balances only with the right m."""
    pt = DF.POINTS[name]
    s = solver_for(pt, obst_mult=mult)
    x0, p = pt.inputs(64)
    r = s.solve(x0, p, multipliers=True)
    assert np.all(r.status == 1)
    f2, g2 = s.eval_nlp(r.x, p)
    assert np.array_equal(f2, r.f) and np.array_equal(g2, r.g)
    nlp = BicycleNLP(pt.cfg)
    worst, active = 0.0, 0
    for b in range(64):
        fr, gr = nlp.f(r.x[b], p[b]), nlp.g(r.x[b], p[b])
        assert abs(r.f[b] - fr) <= 1e-12 * abs(fr)
        assert np.max(np.abs(r.g[b] - gr) / np.maximum(1.0, np.abs(gr))) <= 1e-12 * max(1.0, np.max(np.abs(r.x[b])))
        grad, J = nlp.grad(r.x[b], p[b]), nlp.jac(r.x[b], p[b])
        res = np.abs(grad + J.T @ r.lam_g[b] + r.lam_x[b]).max() / max(1.0, np.abs(grad).max())
        worst = max(worst, res)
        active += bool(np.abs(r.lam_g[b, nlp.row_obst(0):]).max() > 1e-3) if pt.kind == "ca" else bool(abs(r.lam_g[b, 0]) > 1e-3)
    print(f"{name} obst_mult={mult}: worst stationarity {worst:.2e}; rows with an active {'circle' if pt.kind == 'ca' else 'friction'} row: {active}")
    assert worst <= 1e-6
    assert active >= 16                                            # (the rows whose Jacobian holds ego_offset / friction_div carry weight)
    if pt.kind == "ca" and mult != 3:
        o = r.lam_g[:, nlp.row_obst(0):].reshape(64, -1, 3)
        assert np.array_equal(o[:, :, 0], o[:, :, 1]) and np.array_equal(o[:, :, 0], o[:, :, 2])


@pytest.mark.parametrize("nx", [5, 6])
def test_plant_step_at_another_dt_and_wheelbase(nx):
    """mpc_plant_step, B = 257, Euler and RK4 at dt = 0.16, wheelbase = 3.1 against the oracle's plant steps at 1e-12, the tolerance of the
    known-answer test (libm against the device's sin / cos / tan)"""
    cfg = NLPConfig(N=10, nx=nx, dt=0.16, wheelbase=3.1)
    s, o = make_solver(cfg), OracleSolver(cfg)
    rng = np.random.default_rng(nx)
    x = rng.normal(size=(257, nx)) * ([30, 30, 0.3, 5, 1.0, 10][:nx]) + ([0, 0, 0, 12, 0, 0][:nx])
    u = rng.normal(size=(257, 2)) * [0.3, 3.0]
    for integ in ("euler", "rk4"):
        got = s.plant_step(x, u, integ)
        want = np.array([o.plant_step(a, b, integ) for a, b in zip(x, u)])
        dflt = np.array([OracleSolver(NLPConfig(N=10, nx=nx)).plant_step(a, b, integ) for a, b in zip(x[:8], u[:8])])
        assert np.abs(want[:8] - dflt).max() > 1e-2
        assert np.abs(got - want).max() < 1e-12, integ


def test_metrics_clearance_with_another_ego_offset():
    """metrics(...)["clearance"] of a handle with ego_offset = 0.6 against M.min_clearance(..., 0.6, r_sum), both pair sets, as
    test_gpu_metrics_bit_exact_against_restatement does at 0.75"""
    from oracle import metrics_numpy as M
    rng = np.random.default_rng(5)
    B, L = 37, 61
    traj = rng.normal(size=(B, L, 5)) * [30, 5, 0.1, 3, 0.5] + [50, 0, 0, 15, 0]
    oc = np.array([[59.948, 0.08323], [60.945, 0.16074], [58.951, 0.00572]])
    s = pkg.BatchedMPCSolver(10, 5, obstacle_centers=oc, ego_offset=0.6)
    m3 = s.metrics(traj, r_sum=3.1)["clearance"]
    m9 = s.metrics(traj, r_sum=3.1, all_pairs=True)["clearance"]
    moved = 0
    for b in range(B):
        assert abs(m3[b] - M.min_clearance(traj[b], oc, 0.6, 3.1)) < 1e-12
        assert abs(m9[b] - M.min_clearance(traj[b], oc, 0.6, 3.1, all_pairs=True)) < 1e-12
        moved += abs(M.min_clearance(traj[b], oc, 0.6, 3.1, all_pairs=True) - M.min_clearance(traj[b], oc, 0.75, 3.1, all_pairs=True)) > 1e-3
    assert moved >= B // 2


def loop_solver():
    s = make_solver(DF.LOOP_CFG)
    set_cfg_bounds(s, DF.LOOP_CFG)
    return s


def test_closed_loop_against_the_oracle_loop():
    """mpc_closed_loop_batch_ex at dt = 0.05, wheelbase = 3.1 (N = 10, L = 24, B = 65) against the numpy host loop over the C oracle (its solve,
    its Euler plant step), step by step at 1e-7 on traj / ctrl (measured on the MI355X: 3.6e-15 / 5.5e-15), every step's status equal"""
    s = loop_solver()
    traj, ctrl, st = s.closed_loop(*DF.loop_inputs(), DF.LOOP_L)
    t_o, c_o, s_o = DF.oracle_loop()
    print(f"device loop against the oracle loop: traj {np.abs(traj - t_o).max():.2e}, ctrl {np.abs(ctrl - c_o).max():.2e}")
    assert np.all(s_o == 1) and np.array_equal(st, s_o)
    assert np.abs(traj - t_o).max() < 1e-7 and np.abs(ctrl - c_o).max() < 1e-7


def test_closed_loop_against_the_host_loop_over_the_gpu_solve_bit_for_bit():
    """the same device loop against the numpy host loop (DF.host_loop) over this handle's own mpc_solve_batch and mpc_plant_step, bit for bit:
    statuses, traj, ctrl; and mpc_plant_step of every (traj[:, i], ctrl[:, i]) row of the device loop is its row traj[:, i + 1].

    This test found k_plant_step one unit in the last place away from the loop's own plant step (k_loop_advance) in the heading, 69 of
    65 x 23 x 5 entries: the compiler fused h * f + x of every component but that one, whose addition the two integrator branches share.  The
    solves then saw inputs one ulp apart (traj 2.2e-16, ctrl 6.7e-16 from step 3 / 4 on).  k_plant_step now writes the fused form out."""
    cfg = DF.LOOP_CFG
    init, path, orient, vdes = DF.loop_inputs()
    s = loop_solver()
    traj, ctrl, st = s.closed_loop(init, path, orient, vdes, DF.LOOP_L)

    def solve(x0, p):
        r = s.solve(x0, p)
        return r.x, r.status

    t_h, c_h, s_h = DF.host_loop(solve, lambda x, u: s.plant_step(x, u, "euler"), cfg, init, path, orient, vdes, DF.LOOP_L)
    print(f"device loop against the host loop over the GPU solve: traj {np.abs(traj - t_h).max():.2e}, ctrl {np.abs(ctrl - c_h).max():.2e}")
    nxt = np.stack([s.plant_step(np.ascontiguousarray(traj[:, i]), np.ascontiguousarray(ctrl[:, i]), "euler") for i in range(DF.LOOP_L - 1)], axis=1)
    first = [int(np.flatnonzero((a != b).any(axis=(0, 2)))[0]) if (a != b).any() else -1 for a, b in ((traj, t_h), (ctrl, c_h))]
    print(f"mpc_plant_step of the device loop's own (traj, ctrl) rows against its next traj row: {int((nxt != traj[:, 1:]).sum())} entries differ, "
          f"columns {np.flatnonzero((nxt != traj[:, 1:]).any(axis=(0, 1)))}; first step with other bits: traj {first[0]}, ctrl {first[1]}")
    assert np.array_equal(nxt, traj[:, 1:])
    assert np.array_equal(st, s_h) and np.array_equal(traj, t_h) and np.array_equal(ctrl, c_h)


# ---- FORCES mode at FP (DF.FP, DF.FP_WEIGHTS) ---------------------------------------------------------------------------------------------------
import floop_ref                                                 # noqa: E402
import forces_families as FF                                     # noqa: E402
from helpers import emu_forces_solve                             # noqa: E402
from oracle import forces_model_numpy as FM                      # noqa: E402


def fp_solver(N):
    w = DF.FP_WEIGHTS
    return pkg.BatchedMPCSolver(N, 5, Q=w["Q"], R=w["R"], P=w["P"], **DF.FP)


@pytest.mark.parametrize("terminal", [False, True])
def test_forces_stage_functions_at_fp(terminal):
    """mpc_forces_stage_eval, B = 1024, against the numpy restatement with FP's scalars passed through (tests/test_descriptor_cpu.py checks that
    against central differences) at the 1e-12 tests/test_forces_model.py uses for its random batch"""
    s = fp_solver(10)
    rng = np.random.default_rng(2)
    B = 1024
    z = rng.normal(size=(B, 7)) * [0.3, 3, 30, 5, 0.4, 8, 1.0] + [0, 0, 40, 0, 0, 12, 0]
    p = rng.normal(size=(B, 10)) * 20 + 30
    g = s.forces_stage_eval(z, p, terminal=terminal)
    rel = lambda a, b: np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max())     # noqa: E731
    for b in range(0, B, 16):
        r = FM.stage_functions(z[b], p[b], terminal=terminal, weights=DF.FP_WEIGHTS, **DF.FP)
        for name in ("f", "grad_f", "c", "jac_c", "h", "jac_h"):
            if terminal and name in ("c", "jac_c"):
                assert g[name] is None
                continue
            assert rel(g[name][b], r[name]) < 1e-12, (b, name)


@pytest.mark.parametrize("N", [3, 10, 33])
def test_forces_solve_at_fp(N):
    """mpc_forces_solve_batch on FF.binding_family, B = 64, both Hessian modes, against emu_forces_solve (the harness, which
    tests/test_descriptor_cpu.py holds to the dense oracle at FP): flags and iterations equal, |x - x_emu| below the 1e-8 of
    tests/test_forces_qp.py (GPU_EMU_BOUND)"""
    s = fp_solver(N)
    zbar, params, xinit = FF.binding_family(64, N)
    for mode in (0, 1):
        x, flag, it, _ = s.forces_solve(zbar, xinit, params, FF.LB, FF.UB, FF.HL, FF.HU, hessian_mode=mode)
        xe, ite, ste, _ = emu_forces_solve(zbar, params, xinit, DF.FP_WEIGHTS, FF.LB, FF.UB, FF.HL, FF.HU, mode, **DF.FP)
        xd, _, std, _ = emu_forces_solve(zbar, params, xinit, DF.FP_WEIGHTS, FF.LB, FF.UB, FF.HL, FF.HU, mode, **dict(DF.FP, friction_div=3.1, wheelbase=3.3))
        d = np.abs(x - xe).reshape(64, -1).max(axis=1)
        swapped = np.abs(xd - xe).reshape(64, -1).max(axis=1)[(ste == 1) & (std == 1)]
        print(f"FP N={N} mode={mode}: flags {dict(zip(*np.unique(flag, return_counts=True)))}, |x - x_emu| {d.max():.2e}; wheelbase and friction_div "
              f"swapped would move {int((swapped > 1e-6).sum())} of {len(swapped)} rows")
        assert np.array_equal(flag, ste) and np.array_equal(it, ite)
        assert (ste == 1).sum() >= 32 and d.max() < 1e-8
        assert (swapped > 1e-6).sum() >= len(swapped) // 2          # (FP tells wheelbase and friction_div apart in the QP solve)


def test_forces_closed_loop_past_obstacles_at_fp():
    """mpc_forces_closed_loop_batch_obst, L = 12, B = 33, guess_mode 1, the obstacle predicted per stage, against the numpy host loop of
    tests/floop_ref.py (dt, wheelbase, ego_offset as arguments) over mpc_forces_solve_batch of the same handle, by the rule of
    test_device_loop_against_the_host_loop: flags equal and traj, ctrl, clearance within 1e-9 up to every ego's first failed step"""
    N, L = DF.FP_LOOP_N, DF.FP_LOOP_L
    init, path, orient, vdes, track = DF.fp_loop_inputs()
    s = fp_solver(N)
    bounds = (FF.LB, FF.UB, FF.HL, FF.HU)
    traj, ctrl, flag, cl = s.forces_closed_loop_obst(init, path, orient, vdes, L, *bounds, obst_track=track, obst_offset=floop_ref.OBST_OFFSET, predict=True,
                                                     guess_mode=1, r_sum=floop_ref.R_SUM)
    want = floop_ref.host_loop(floop_ref.backend_solver(s), init, path, orient, vdes, L, N, track=track, predict=1, guess_mode=1,
                               ego_offset=DF.FP["ego_offset"], dt=DF.FP["dt"], wheelbase=DF.FP["wheelbase"])
    failed = want["flag"] != 1
    first = np.where(failed.any(axis=1), failed.argmax(axis=1), L)
    m = np.arange(L)[None, :] <= first[:, None]
    clean = np.all(want["flag"] == 1, axis=1)
    d = {k: np.abs(got - want[k])[m].max() for k, got in (("traj", traj), ("ctrl", ctrl), ("clearance", cl))}
    print(f"egos with every exitflag 1: {int(clean.sum())} of {len(clean)};", {k: f"{v:.2e}" for k, v in d.items()}, "min clearance", cl[m].min())
    assert clean.sum() >= 0.75 * len(clean)
    assert np.array_equal(flag[m], want["flag"][m])
    assert max(d.values()) <= 1e-9
    assert cl[m].min() < 0.5                                       # (the circle rows were near enough to bind)


@pytest.mark.parametrize("name", ["D5", "D6"])
@pytest.mark.parametrize("fam", DF.SENS_FAMILIES)
def test_sensitivities_of_the_optimum(fam, name):
    """dw/dp (solve(..., dp=)), dw/dweights (mpc_sens_weights), dw/dbounds (mpc_sens_bounds), dw/dobst (mpc_sens_obst, every instance an obstacle
    row of its own) behind a solve at D5 / D6, on DF.SENS_ROWS against the family's numpy reference on the point's cfg, in the measure of the
    family's own tests.  Bounds: DESC_TOL of the reference module, min(10 x the reference's distance from the CPU harness on these rows, the
    family's cap), which tests/test_descriptor_cpu.py measures; D5's instance 12 has a bound of its own.  lam_p, lam_wt, lam_obst against their
    closed forms.  At D5 the obstacle family's reference is exactly 0 (no circle row active)."""
    ref = DF._sens_ref(fam)
    pt = DF.POINTS[name]
    s = solver_for(pt)
    B = DF.SENS_B
    x0, p = pt.inputs(B)
    dirs = np.ascontiguousarray(DF.sens_directions(fam, pt.cfg, B))
    obst = DF.sens_obst_rows(pt.cfg, B) if fam == "obst" else None
    r = s.solve(x0, p, obst, multipliers=True, lam_p=True, dp=dirs if fam == "p" else None)
    assert np.all(r.status == 1)
    if fam == "p":
        dw = r.dw
    elif fam == "weights":
        o = s.sens_weights(p, dweights=dirs, lam=True)
        dw = o.dw
    elif fam == "bounds":
        dw = s.sens_bounds(dbounds=dirs).dw
    else:
        o = s.sens_obst(dirs, lam=True)
        dw = o.dw
    assert np.all(np.isfinite(dw))
    rows = range(B)[DF.SENS_ROWS]
    if fam == "obst" and name == "D5":
        errs = {b: float(np.max(np.abs(dw[b]))) for b in rows}
        assert not any(ref.sensitivity_matrix(pt.cfg, obst[b], r.x[b], p[b], r.lam_g[b], r.lam_x[b])[0].any() for b in rows)
    else:
        errs = DF.sens_row_errors(fam, pt.cfg, r.x, p, r.lam_g, r.lam_x, dw, dirs, rows, obst)
    DF.assert_sens(fam, name, errs, np.arange(B))
    for b in rows:
        if fam == "p":
            want, got = ref.lam_p(pt.cfg, r.x[b], p[b], r.lam_g[b]), r.lam_p[b]
        elif fam == "weights":
            want, got = ref.lam_weights(pt.cfg, r.x[b], p[b]), o.lam_wt[b]
        elif fam == "obst":
            want, got = ref.lam_obst(pt.cfg, obst[b], r.x[b], r.lam_g[b]), o.lam_obst[b]
        else:
            continue
        assert np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))) <= 1e-12, (fam, b)


def test_predicted_loop_clearance_with_another_ego():
    """closed_loop(..., predict=True), N = 10, B = 16, drift scenes at ego_length 3.6 / ego_width 1.5: the clearance the device reports against
    clearance_numpy (tests/loop_obst_ref.py) with the cfg's ego_offset = 0.6 and r_sum = 3.1 on the returned trajectory, at 1e-12.  The scenes are
    DF.pred_loop_inputs, the drift family of tests/pred_obst_ref.py restated as a loop (that module's instances are single solves: a guess, a
    parameter row and N + 1 stage poses, no path or track to drive a loop along); its cfg_for gives the configuration."""
    import loop_obst_ref
    cfg, init, path, orient, vdes, track, offset = DF.pred_loop_inputs()
    s = make_solver(cfg)
    set_cfg_bounds(s, cfg)
    traj, ctrl, st, cl = s.closed_loop(init, path, orient, vdes, DF.PRED_L, obst_track=track, obst_offset=offset, clearance=True, predict=True)
    c6 = loop_obst_ref.centres_numpy(track[:, :DF.PRED_L])
    want = loop_obst_ref.clearance_numpy(traj, c6, cfg.ego_offset, cfg.r_sum)
    other = loop_obst_ref.clearance_numpy(traj, c6, 0.75, 3.3)
    print(f"status 1 on {int((st == 1).sum())} of {st.size} steps; |clearance - numpy| {np.abs(cl - want).max():.2e}; min clearance {cl.min():.3f}; "
          f"largest lateral move {np.abs(traj[:, :, 1]).max():.3f}")
    assert (st == 1).mean() >= 0.9
    assert np.abs(cl - want).max() <= 1e-12
    assert np.abs(want - other).min() > 1e-3                        # (the default ego would report another clearance on every row)
    assert np.abs(traj[:, :, 1]).max() > 0.05 and cl.min() > -0.05   # the obstacle was seen and kept clear of


def test_linearised_loop_off_the_default_descriptor():
    """closed_loop(..., linearize=True), loop_tangent, loop_adjoint at dt = 0.05, wheelbase = 3.1 (tests/loop_lin_ref.py: LFD_SCENES; mpc_loop_lin.h reads
    both in its plant Jacobian): the rollout is the plain loop's bit for bit; the gains against the chained numpy reference and the tangent over
    the whole loop at ref.TOL_LFD (min(10 x the CPU harness's distance from the reference at this point, the existing bounds)); the device sweeps
    within 1e-12 of the sum of the absolute terms of the numpy recursion over the same gains, as tests/test_gpu_loop_lin.py holds them; one
    tangent / adjoint pair satisfies <seed, tangent> = <adjoint, direction>"""
    import loop_lin_ref as ref
    scenes = ref.LFD_SCENES
    cfg = scenes[0].cfg
    s = make_solver(cfg)
    set_cfg_bounds(s, cfg)
    s.set_option("loop_async", "0")
    init, path, orient, vdes, _ = ref.batch_inputs(scenes)
    plain = s.closed_loop(init, path, orient, vdes, scenes[0].L)
    lin = s.closed_loop(init, path, orient, vdes, scenes[0].L, linearize=True)
    assert np.array_equal(lin.traj, plain[0]) and np.array_equal(lin.ctrl, plain[1]) and np.array_equal(lin.status, plain[2]) and np.all(lin.status == 1)
    got = dict(traj=lin.traj, ctrl=lin.ctrl, status=lin.status, kgain=lin.kgain, wgain=lin.wgain, ogain=None)
    worst, n_weak = ref.gain_errors(scenes, "LFD", got)
    B, L = lin.traj.shape[:2]

    def sweep(b, dinit, dwt, dtrack):
        one = pkg.LoopLin(lin.traj[b:b + 1], lin.ctrl[b:b + 1], lin.status[b:b + 1], lin.kgain[b:b + 1], lin.wgain[b:b + 1])
        dtraj, dctrl = s.loop_tangent(one, dinit[None, None], dwt[None, None])
        return dtraj[0, 0], dctrl[0, 0]

    loop = ref.tangent_errors(scenes, "LFD", sweep)
    print(f"gains against the reference: k {worst['k']:.2e} (bound {ref.TOL_LFD['k']:.1e}) w {worst['w']:.2e} (bound {ref.TOL_LFD['w']:.1e}), {n_weak} weakly active "
          f"steps left out; tangent over the loop {loop:.2e} (bound {ref.TOL_LFD['loop']:.1e})")
    assert worst["k"] <= ref.TOL_LFD["k"] and worst["w"] <= ref.TOL_LFD["w"] and loop <= ref.TOL_LFD["loop"]
    rng = np.random.default_rng(7)
    nd = 3
    dinit, dwt = rng.normal(size=(B, nd, 5)), rng.normal(size=(B, nd, 7))
    st, sc = rng.normal(size=(B, L, 5)), rng.normal(size=(B, L, 2))
    dtraj, dctrl = s.loop_tangent(lin, dinit, dwt)
    gi, gw, gt = s.loop_adjoint(lin, st, sc)
    assert gt is None
    for b in range(B):
        a = (lin.traj[b], lin.kgain[b], lin.wgain[b], None, 0)
        for d in range(nd):
            want = ref.tangent(*a, dinit[b, d], dwt[b, d], None, cfg.dt, cfg.wheelbase)
            mag = ref.tangent(*a, dinit[b, d], dwt[b, d], None, cfg.dt, cfg.wheelbase, mag=True)
            for g_, w_, m_ in zip((dtraj[b, d], dctrl[b, d]), want, mag):
                assert np.all(np.abs(g_ - w_) <= 1e-12 * m_), (b, d)
            dflt = ref.tangent(*a, dinit[b, d], dwt[b, d], None, 0.1, 2.5789128)
            assert np.abs(dflt[0] - want[0]).max() > 1e-3 * np.abs(want[0]).max()          # (the default descriptor's sweep is another one)
            lhs = np.sum(st[b] * dtraj[b, d]) + np.sum(sc[b] * dctrl[b, d])
            rhs = gi[b] @ dinit[b, d] + gw[b] @ dwt[b, d]
            assert abs(lhs - rhs) <= 1e-12 * (np.sum(np.abs(st[b]) * mag[0]) + np.sum(np.abs(sc[b]) * mag[1])), (b, d, lhs, rhs)
        want = ref.adjoint(*a, st[b], sc[b], cfg.dt, cfg.wheelbase)
        mag = ref.adjoint(*a, st[b], sc[b], cfg.dt, cfg.wheelbase, mag=True)
        for g_, w_, m_ in zip((gi[b], gw[b]), want, mag):
            assert np.all(np.abs(g_ - w_) <= 1e-12 * m_), b
