"""CPU: the points of tests/descriptor_families.py -- mpc_problem_desc away from dt = 0.1, wheelbase = 2.5789128, friction_div = 2.578,
ego_offset = 0.75, tol = 1e-8, obst_mult = 3.

1. The guard: from the C oracle alone, every point converges on every row and moves the optimum of at least half the rows by more than 1e-3
   against the same inputs solved at the default value of its fields (a point that does not would not notice a kernel that ignores the field).
2. The emulated solve (tests/emu: the kernels' phase functions stepped on the CPU) against the oracle at every point and cross.
3. The numpy restatements of the FORCES mode with wheelbase, friction divisor and ego offset passed through: against central differences of
   their own f, c, h at FP; emu_forces_solve against sqp_step at FP.
4. The references of everything that hangs off a solve (tests/*_ref.py) against their CPU harnesses at D5 / D6: the figures the tolerances of
   tests/test_gpu_descriptor.py are made of."""
import numpy as np
import pytest

import descriptor_families as DF
from helpers import emu_solve

TOL_ORACLE = 1e-8               # the project's bound of a lane-following solve against the oracle (tests/test_gpu_parity.py)


@pytest.mark.parametrize("name", list(DF.POINTS) + ["N64"])
def test_every_point_converges_and_moves_the_optimum(name):
    """the oracle alone.  Measured (rows moved by more than 1e-3 among those converged on both sides / rows): D1 32/32, D2 32/32, D3 31/32,
    D4 23/32 (at the default friction_div three steered rows do not converge: the kink of the friction row), D5 32/32, D6 64/64, D30 32/32,
    N64 66/66"""
    pt = DF.N64 if name == "N64" else DF.POINTS[name]
    B = DF.GUARD_B[name]
    at, dflt = DF.oracle_rows(pt, B), DF.oracle_rows(pt, B, default=True)
    assert np.all(at["status"] == 1)
    moved = (np.abs(at["x"] - dflt["x"]).max(axis=1) > 1e-3) & (dflt["status"] == 1)
    print(name, "moved", int(moved.sum()), "of", B)
    assert moved.sum() >= B // 2


def test_the_batches_of_the_gpu_tests_converge_in_the_oracle():
    """the rows tests/test_gpu_descriptor.py compares with the oracle at the sizes it uses: all converge (status and iterations then compare
    row for row)"""
    for pt in [DF.POINTS[name] for name in ("D1", "D2", "D3", "D4", "D5")] + [DF.D5_AT_DEFAULTS]:
        assert np.all(DF.oracle_rows(pt, 130)["status"] == 1), pt.name
        assert np.all(DF.oracle_rows(pt, 130, obst_mult=1)["status"] == 1), pt.name
    for N in DF.SHORT_HORIZONS:
        assert np.all(DF.oracle_rows(DF.POINTS["D5"].at(N), 65)["status"] == 1), N
    assert np.all(DF.oracle_rows(DF.N64, 66)["status"] == 1)
    for B, start in DF.D30_BATCHES.values():
        assert np.all(DF.oracle_rows(DF.POINTS["D30"], B, start=start, step=DF.step64(B))["status"] == 1), B


@pytest.mark.parametrize("case", DF.CASES + [("D30", 1e-8, 3)], ids=DF.case_id)
def test_emulated_solve_matches_the_oracle(case):
    """variant 0 of the stage math at every point and cross.  Lane-following points: status, iterations, |x - x_oracle| < 1e-8 (measured:
    at most 1.6e-14), kkt <= tol.  D6 by the rule of test_collision_avoidance_batch: at least 85 % of the rows converged on both sides agree
    within 1e-6 (measured: all, to 7.3e-8), every other row is a KKT point by the certificate at 1e-6 / 1e-6."""
    name, tol, mult = case
    pt = DF.POINTS[name]
    B = DF.GUARD_B[name]
    x0, p = pt.inputs(B)
    re = emu_solve(pt.cfg, x0, p, tol=tol, obst_mult=mult)
    ro = DF.oracle_rows(pt, B, tol=tol, obst_mult=mult)
    if pt.kind == "ca":
        DF.assert_ca_rule(pt.cfg, re["x"], re["status"], re["kkt"], p, ro)
        return
    assert np.array_equal(re["status"], ro["status"]) and np.all(ro["status"] == 1)
    assert np.array_equal(re["iters"], ro["iters"])
    err = np.abs(re["x"] - ro["x"]).max()
    print(DF.case_id(case), f"max |x - x_oracle| = {err:.2e}, kkt max {re['kkt'].max():.2e}")
    assert err < TOL_ORACLE
    assert re["kkt"].max() <= tol


def test_tolerance_and_multiplicity_are_read():
    """tol = 1e-6 stops earlier than 1e-10 on some row and obst_mult does not move the collision-avoidance optimum beyond the tolerance: the
    crosses are no copies of their base case"""
    pt = DF.POINTS["D5"]
    loose, tight = DF.oracle_rows(pt, 32, tol=1e-6), DF.oracle_rows(pt, 32, tol=1e-10)
    assert loose["iters"].sum() < tight["iters"].sum() and loose["kkt"].max() > 1e-8 >= tight["kkt"].max()
    pt = DF.POINTS["D6"]
    m3 = DF.oracle_rows(pt, 64)
    for m in (1, 2):
        mm = DF.oracle_rows(pt, 64, obst_mult=m)
        assert not np.array_equal(mm["x"], m3["x"]) and np.abs(mm["x"] - m3["x"]).max() < 1e-6


# ---- 3. the FORCES mode at FP = (dt 0.08, l 3.1, wb 3.3, rho 0.6), weights DF.FP_WEIGHTS ------------------------------------------------------
import forces_families as FF                                    # noqa: E402
from helpers import emu_forces_solve                            # noqa: E402
from oracle import forces_model_numpy as FM                     # noqa: E402
from oracle import forces_qp_numpy as QP                        # noqa: E402


@pytest.mark.parametrize("terminal", [False, True])
def test_extended_restatement_against_central_differences_at_fp(terminal):
    """at FP the numpy restatement has no compiled reference to lean on (tests/test_forces_model.py pins it at the defaults): grad_f, jac_c,
    jac_h against central differences of its own f, c, h, with the bound of test_restatement_jacobians_by_finite_differences; and every one
    of the three scalars passed through moves the function it belongs to"""
    rng = np.random.default_rng(1)
    kw = dict(terminal=terminal, weights=DF.FP_WEIGHTS, **DF.FP)
    eps = 1e-6
    for _ in range(8):
        z = np.array([0.1, 0.5, 1.0, 2.0, 0.3, 5.0, 0.4]) + 0.1 * rng.normal(size=7)
        p = np.array([1.5, 2.5, 6.0, 0.35, 10, 1, 11, 1.2, 9, 0.8]) + 0.3 * rng.normal(size=10)
        r = FM.stage_functions(z, p, **kw)
        for name, jac in (("c", "jac_c"), ("h", "jac_h"), ("f", "grad_f")):
            if terminal and name == "c":
                assert r["c"] is None and r["jac_c"] is None
                continue
            J = np.zeros(np.shape(r[jac]))
            for j in range(7):
                dz = np.zeros(7)
                dz[j] = eps
                J[..., j] = (np.asarray(FM.stage_functions(z + dz, p, **kw)[name]) - np.asarray(FM.stage_functions(z - dz, p, **kw)[name])) / (2 * eps)
            assert np.abs(J - r[jac]).max() < 1e-6 * max(1.0, np.abs(r[jac]).max()), name
        d = FM.stage_functions(z, p, terminal=terminal, weights=DF.FP_WEIGHTS, dt=DF.FP["dt"])
        assert abs(r["h"][0] - d["h"][0]) > 1e-3 * abs(d["h"][0])                                 # friction_div
        assert np.abs(r["h"][4:] - d["h"][4:]).max() > 1e-3 and np.array_equal(r["h"][1:4], d["h"][1:4])     # ego_offset: the front / rear circles
        if not terminal:
            assert abs(r["c"][4] - d["c"][4]) > 1e-4 and np.array_equal(r["c"][2:4], d["c"][2:4])  # wheelbase: the heading


# emu_forces_solve (the kernel's QP code, stage after stage) against sqp_step (dense KKT) at FP, worst |z - z_oracle| over the converged
# instances of FF.binding_family, both Hessian modes and both bound pairs, measured here (harness against numpy, no kernel involved):
#   N = 3: 7.1e-15, N = 10: 4.9e-13, N = 33: 4.8e-13 (the first 8 instances, one bound pair)
# all below the bound of tests/test_forces_qp.py, 1e-7, which therefore holds at FP unchanged
FP_QP_BOUND = 1e-7


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("N", [3, 10, 33])
def test_emulated_forces_solve_against_the_dense_oracle_at_fp(N, mode):
    zbar, params, xinit = FF.binding_family(16, N)
    idx = range(16) if N <= 10 else range(8)
    worst, n_conv = 0.0, 0
    for lb, ub in ((FF.LB, FF.UB), (FF.LB_TIGHT, FF.UB_TIGHT))[:2 if N <= 10 else 1]:
        zo, it, st, _ = emu_forces_solve(zbar, params, xinit, DF.FP_WEIGHTS, lb, ub, FF.HL, FF.HU, mode, **DF.FP)
        for b in idx:
            zp, ito, conv, _ = QP.sqp_step(zbar[b], params[b], xinit[b], lb, ub, FF.HL, FF.HU, weights=DF.FP_WEIGHTS, mode=mode, **DF.FP)
            assert (st[b] == 1) == conv, (b, st[b], conv)
            if conv:
                n_conv += 1
                assert it[b] == ito, (b, it[b], ito)
                worst = max(worst, np.abs(zp - zo[b]).max())
    print(f"FP N={N} mode={mode}: {n_conv} converged, worst |z - z_oracle| = {worst:.2e}")
    assert n_conv >= len(idx) // 2 and worst < FP_QP_BOUND


# ---- 4. the references against their CPU harnesses at D5 / D6 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["D5", "D6"])
@pytest.mark.parametrize("fam", DF.SENS_FAMILIES)
def test_sensitivity_harness_against_the_reference(fam, name):
    """tests/sensx (the functions k_sens runs for the family, behind the emulated solve) against the family's numpy reference at the point, on the
    rows the GPU test compares: the figures DESC_HARNESS_WORST of the reference modules, which this test holds to what it measures (within 2 %).
    At D5 the presolved friction bound, whose derivative holds friction_div (mpc_sens.h: dc), is active on most rows: with the literal 2.578 in
    its place the p family's error here is 0.28.  The adjoint identity as the families' own CPU tests check it."""
    pt = DF.POINTS[name]
    x0, p = (np.ascontiguousarray(a[DF.SENS_ROWS]) for a in pt.inputs(DF.SENS_B))
    B = x0.shape[0]
    instances = np.arange(DF.SENS_B)[DF.SENS_ROWS]
    dirs = np.ascontiguousarray(DF.sens_directions(fam, pt.cfg, DF.SENS_B)[DF.SENS_ROWS])
    obst = DF.sens_obst_rows(pt.cfg, DF.SENS_B)[DF.SENS_ROWS] if fam == "obst" else None
    seeds = np.random.default_rng(3).normal(size=(B, pt.cfg.n_w))
    r = DF.sens_harness(fam, pt.cfg, x0, p, dirs, seeds, obst)
    assert np.all(r["status"] == 1) and np.all(r["ok"] == 1)
    if fam == "obst" and name == "D5":                      # no circle row is active: the reference is exactly 0
        errs = {b: float(np.max(np.abs(r["dw"][b]))) for b in range(B)}
        assert not any(DF._sens_ref(fam).sensitivity_matrix(pt.cfg, obst[b], r["x"][b], p[b], r["lam_g"][b], r["lam_x"][b])[0].any() for b in range(B))
    else:
        errs = DF.sens_row_errors(fam, pt.cfg, r["x"], p, r["lam_g"], r["lam_x"], r["dw"], dirs, range(B), obst)
    DF.assert_sens(fam, name, errs, instances, harness=True)
    if name == "D5":
        assert int((r["lam_g"][:, 0] > 1e-3).sum()) >= B // 2                # the friction bound is active on most rows
    grad = r[{"p": "grad_p", "weights": "grad_wt", "bounds": "grad_bv", "obst": "grad_obst"}[fam]]
    for b in range(B):
        for q in range(dirs.shape[1]):
            lhs, rhs = seeds[b] @ r["dw"][b, q], grad[b] @ dirs[b, q]
            assert abs(lhs - rhs) <= 1e-10 * max(1.0, np.abs(seeds[b]).sum() * np.max(np.abs(r["dw"][b, q]))), (b, q, lhs, rhs)



def test_loop_lin_reference_and_harness_off_the_default_descriptor():
    """tests/loop_lin_ref.py at LFD_SCENES (dt = 0.05, wheelbase = 3.1): the chained reference against central differences of the oracle loop at its own
    TOL_FD, then the CPU harness (tests/looplinx: the emulated solve, loop_gain_family, the sweep lanes) against the reference -- the figures
    LFD_HARNESS_WORST, which this test holds to what it measures (within 2 %)"""
    import ctypes as C
    import loop_lin_ref as ref
    import test_loop_lin_cpu as TL
    from helpers import abi, harness_lib
    scenes = ref.LFD_SCENES
    fd_worst = 0.0
    for idx in range(len(scenes)):
        scene, run, gains = ref.reference("LFD", idx)
        assert np.all(run["status"] == 1)
        for d in ref.directions(scene):
            fd = ref.fd_direction(scene, d)
            assert np.abs(fd).max() >= ref.FD_FLOOR, d[0]
            fd_worst = max(fd_worst, ref.rel_err(ref.ref_direction(scene, run, gains, d), fd))
    L = C.CDLL(harness_lib("looplinx"))
    dp, ip, i32, f64 = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_int32, C.c_double
    L.looplinx_loop.argtypes = [C.POINTER(abi.MpcProblemDesc)] + [dp] * 4 + [i32] * 3 + [dp] * 4 + [i32, dp, f64, dp, dp, ip, dp, dp, dp]
    L.looplinx_loop.restype = C.c_int
    L.looplinx_tangent.argtypes = [f64, f64, i32, i32, i32] + [dp] * 4 + [i32] + [dp] * 5
    L.looplinx_tangent.restype = None
    got = TL.harness_loop(L, scenes)
    assert np.all(got["status"] == 1)
    assert np.abs(got["traj"] - np.array([ref.reference("LFD", b)[1]["traj"] for b in range(len(scenes))])).max() <= 1e-6
    worst, n_weak = ref.gain_errors(scenes, "LFD", got)
    cfg = scenes[0].cfg

    def sweep(b, dinit, dwt, dtrack):
        c = lambda a: np.ascontiguousarray(a, dtype=np.float64)      # noqa: E731
        Ls = scenes[b].L
        dtraj, dctrl = np.zeros((Ls, 5)), np.zeros((Ls, 2))
        L.looplinx_tangent(cfg.dt, cfg.wheelbase, 1, Ls, 1, abi.as_dp(c(got["traj"][b])), abi.as_dp(c(got["kgain"][b])), abi.as_dp(c(got["wgain"][b])), None, 0,
                           abi.as_dp(c(dinit)), abi.as_dp(c(dwt)), None, abi.as_dp(dtraj), abi.as_dp(dctrl))
        return dtraj, dctrl

    loop = ref.tangent_errors(scenes, "LFD", sweep)
    print(f"reference against central differences {fd_worst:.2e}; harness against reference: k {worst['k']:.3e} w {worst['w']:.3e} loop {loop:.3e}, "
          f"{n_weak} weakly active steps left out")
    assert fd_worst <= ref.TOL_FD and n_weak <= 2
    assert worst["k"] <= 1.02 * ref.LFD_HARNESS_WORST["k"] and worst["w"] <= 1.02 * ref.LFD_HARNESS_WORST["w"] and loop <= 1.02 * ref.LFD_HARNESS_WORST["loop"]
    g0, g1 = ref.reference("LF", 0)[2], ref.reference("LFD", 0)[2]
    assert np.abs(g0["kgain"] - g1["kgain"]).max() > 1e-2          # (the gains at the default descriptor are others)
