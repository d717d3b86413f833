"""CPU: the points of tests/bound_structures.py -- bound structures mpc_set_bounds accepts and the reference never sets.

(1) The conditions that make a point worth a GPU test, from the C oracle alone: its instances converge, a binding point moves the optimum, an
    inactive one leaves it where it is.  (2) The emulated solve (the kernels' phase functions, tests/emu) against the oracle at every point.
(3) The launch plan at every point.  (4) A certificate that rests on neither interior-point code (helpers.kkt_certificate with the point's bounds).
(5) What mpc_set_bounds refuses, through the emulated entry."""
import numpy as np
import pytest

import bound_structures as BS
from helpers import CA_CFG, BicycleNLP, emu_solve, kkt_certificate
from test_solve_plan import plan

LANE_ALL = BS.lane_cases(("n10", "n30", "n50", "n64"))
LANE_EMU = BS.lane_cases(("n10", "n30"))
CA_CASES = [(n, "ca") for n in BS.CA_POINTS]
TIGHT = dict(tol=1e-10, max_iter=300)       # the oracle as tests/test_sens_bounds_cpu.py runs it where it differentiates its optima


def moved(name, fam):
    """(converged under the point's bounds, under both, distance of the two optima per instance) on the QB instances"""
    ref, r = BS.reference_rows(name, fam), BS.oracle_rows(name, fam)
    conv = r["status"] == 1
    return conv, conv & (ref["status"] == 1), np.abs(r["x"] - ref["x"]).max(axis=1)


# ---- (1) -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LANE_ALL + CA_CASES, ids=BS.case_id)
def test_conditions_from_the_oracle_alone(case):
    """Lane following: at least 90 % of the QB instances converge.  Collision avoidance: the share written in BS.SHARES (measured: 98 % and above)
    less one instance.  "binds": at least 25 % of the optima move by more than 1e-3 against the reference-bounds optimum; "some" (S4: lbg[0] = 0.5
    binds where the plan would coast, 3 - 23 % of a batch): at least one does; "inactive": with both solves at tol = 1e-10 no optimum moves by 1e-9
    (at the product's 1e-8 the two final iterates are up to 3e-7 apart, each within its tolerance of the same optimum)."""
    name, fam = case
    pt = BS.point(name, fam)
    conv, both, d = moved(name, fam)
    share = float(np.mean(d[both] > 1e-3))
    print(f"{name} {fam}: converged {conv.mean():.3f}, moved by > 1e-3: {share:.3f}, largest move {d[both].max():.2e}")
    assert np.all(BS.reference_rows(name, fam)["status"] == 1)
    assert conv.mean() >= (BS.SHARES[case][0] - 1.0 / BS.QB if fam == "ca" else 0.9)
    if pt.binding == "binds":
        assert share >= 0.25
    elif pt.binding == "some":
        assert (d[both] > 1e-3).sum() >= 1
    else:
        cfg = BS.cfg_of(fam)
        x0, p = BS.inputs(name, fam, BS.QB)
        a = BS.oracle_for(cfg, None, obst_mult=pt.mult(fam), **TIGHT).solve_batch(x0, p, nthreads=8)
        b = BS.oracle_for(cfg, BS.bounds(name, fam), obst_mult=pt.mult(fam), **TIGHT).solve_batch(x0, p, nthreads=8)
        ok = (a["status"] == 1) & (b["status"] == 1)
        worst = np.abs(a["x"] - b["x"])[ok].max()
        print(f"  at tol = 1e-10: {int(ok.sum())} of {BS.QB} converged on both sides, largest move {worst:.2e}")
        assert ok.sum() >= conv.sum() - 1 and worst <= 1e-9


def test_written_shares_are_the_measured_ones():
    """BS.SHARES (what the module's text and DESIGN.md quote) against the oracle: converged and moved shares within two instances of QB (a
    quantile sits on an instance's own extreme, so that instance is a rounding away from either side of 1e-3)"""
    for case in LANE_ALL + CA_CASES:
        conv, both, d = moved(*case)
        got = (float(conv.mean()), float(np.mean(d[both] > 1e-3)))
        assert max(abs(g - w) for g, w in zip(got, BS.SHARES[case])) <= 2.0 / BS.QB + 5e-4, (case, got)


def test_a_binding_upper_bound_of_the_circle_rows_is_not_kept():
    """collision avoidance, circle rows ubg = 31: it binds (every optimum moves) and a quarter of the batch no longer converges -- stage 0 is fixed
    by the initial state beyond it; the reason CA_POINTS has S6 at an inactive 60 only"""
    conv, both, d = moved(BS.CA_BINDING_OU, "ca")
    print(f"ubg = 31: converged {conv.mean():.3f}, moved {np.mean(d[both] > 1e-3):.3f}")
    assert conv.mean() < 0.9 and np.mean(d[both] > 1e-3) >= 0.25


# ---- (2) -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LANE_EMU, ids=BS.case_id)
def test_emulated_solve_matches_the_oracle(case):
    """24 instances: statuses and iteration counts equal, |dx| < 1e-11 where converged -- the bound of test_emulated_kernels_match_oracle"""
    name, fam = case
    pt, cfg = BS.point(name, fam), BS.cfg_of(fam)
    x0, p = BS.inputs(name, fam, 24)
    re = emu_solve(cfg, x0, p, bounds=BS.bounds(name, fam), obst_mult=pt.mult(fam))
    ro = BS.oracle_rows(name, fam)
    st, it, x = ro["status"][:24], ro["iters"][:24], ro["x"][:24]
    ok = st == 1
    err = np.abs(re["x"] - x)[ok].max()
    print(f"{name} {fam}: {int(ok.sum())} of 24 converged, max |x_emu - x_oracle| {err:.2e}")
    assert np.array_equal(re["status"], st) and np.array_equal(re["iters"], it)
    assert ok.sum() >= 20 and err < 1e-11
    assert re["kkt"][ok].max() <= 1e-8


@pytest.mark.parametrize("case", CA_CASES, ids=BS.case_id)
def test_emulated_solve_on_collision_avoidance(case):
    """the comparison of test_collision_avoidance_family, 16 instances"""
    name, fam = case
    pt = BS.point(name, fam)
    x0, p = BS.inputs(name, fam, 16)
    b = BS.bounds(name, fam)
    re = emu_solve(CA_CFG, x0, p, bounds=b, obst_mult=pt.mult(fam))
    ro = BS.oracle_rows(name, fam)
    both = (re["status"] == 1) & (ro["status"][:16] == 1)
    print(f"{name}: converged on both sides {int(both.sum())} of 16, max |dx| {np.abs(re['x'][both] - ro['x'][:16][both]).max():.2e}")
    assert both.mean() >= 0.8
    assert np.abs(re["x"][both] - ro["x"][:16][both]).max() < 1e-4
    nlp = BicycleNLP(CA_CFG)
    for w in re["x"][re["status"] == 1]:
        d = np.concatenate([nlp.obstacle_rows(x)[0] for x in nlp.split(w)[1]])
        assert d.min() >= CA_CFG.r_sum - 1e-6 and d.max() <= b[1][-1] + 1e-6


# ---- (3) -------------------------------------------------------------------------------------------------------------------------------------
# variant 2 of the kernels compiles in which variables carry a bound at all, which sides are there at every stage (all but the acceleration's
# lower one, which it looks up: mpc_stage_math.h, "Upper bits of VM") and circle rows with a lower bound only; has_fl / has_fu stay run-time flags.
# So a floor on the acceleration (S1), a kept friction row (S4) and no friction bound (S5) still run variant 2 -- the GPU tests run them in both
# variants --, every other point takes it out
KEEP_VARIANT_2 = ("S1", "S4", "S5")
STASH_ROWS = {5: (47, 53), 6: (53, 59)}       # Stash<NX>::rows(false), rows(true) = 4 (NX + 2) + 6 (+ 6) + 3 + 2 NX


@pytest.mark.parametrize("case", LANE_ALL + CA_CASES, ids=BS.case_id)
def test_launch_plan(case):
    name, fam = case
    pt, cfg = BS.point(name, fam), BS.cfg_of(fam)
    b = BS.bounds(name, fam)
    pl = plan(cfg, 130, {}, bounds=b, obst_mult=pt.mult(fam))
    ref = plan(cfg, 130, {})
    print(name, fam, {k: pl[k] for k in ("path", "masked", "stash_rows", "dec_s", "has_fl", "has_fu", "has_ol", "has_ou", "rescue")},
          hex(pl["lo_mask"]), hex(pl["hi_mask"]), hex(pl["dense_mask"]))
    assert ref["masked"] == 1 and ref["has_ou"] == 0 and ref["has_fl"] == 0 and ref["has_fu"] == 1
    assert pl["masked"] == (1 if name in KEEP_VARIANT_2 and fam != "ca" else 0)
    assert plan(cfg, 130, {"bound_mask": "0"}, bounds=b, obst_mult=pt.mult(fam))["masked"] == 0
    assert pl["has_ou"] == int(np.isfinite(b[1][-1])) and pl["has_ol"] == 1 and pl["rescue"] == 1
    assert pl["has_fl"] == int(b[0][0] > 0.0) and pl["has_fu"] == int(np.isfinite(b[1][0]))
    lo, hi = STASH_ROWS[cfg.nx]
    if pl["small_wg"]:
        assert ref["stash_rows"] == lo and pl["stash_rows"] == (hi if pl["has_ou"] else lo)
    else:
        assert pl["stash_rows"] == ref["stash_rows"] == 2 * cfg.nx          # the 512-thread stage workgroups park nothing
    assert pl["dec_s"] == (1 if cfg.nx == 6 and name != "S8" else 0) and ref["dec_s"] == int(cfg.nx == 6)
    assert pl["path"] == ref["path"]
    # the masks, from the arrays: bit i of (u0, a, x, y, delta, v, psi, s)
    nz = cfg.nx + 2
    cols = lambda a, k: np.concatenate([a[2 * k: 2 * k + 2] if k < cfg.N else [np.nan, np.nan], a[2 * cfg.N + cfg.nx * k: 2 * cfg.N + cfg.nx * (k + 1)]])  # noqa: E731
    L, U = np.array([cols(b[2], k) for k in range(cfg.N + 1)]), np.array([cols(b[3], k) for k in range(cfg.N + 1)])
    bits = lambda m: sum(1 << i for i in range(nz) if m[i])             # noqa: E731
    assert pl["lo_mask"] == bits(np.isfinite(L).any(axis=0)) and pl["hi_mask"] == bits(np.isfinite(U).any(axis=0))
    dense = bits((np.isfinite(L) | np.isnan(L)).all(axis=0)) | bits((np.isfinite(U) | np.isnan(U)).all(axis=0)) << 8
    assert pl["dense_mask"] & ((1 << nz) - 1 | ((1 << nz) - 1) << 8) == dense


# ---- (4) -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(n, f) for f in ("n10", "n30") for n in BS.BINDING + ("S4",)] + [("FLOU", "ca")], ids=BS.case_id)
def test_oracle_optima_are_kkt_points_of_the_numpy_nlp(case):
    """four oracle optima that the point moved, certified against oracle/nlp_numpy.py with the point's bounds at 1e-6 / 1e-6 (the thresholds of
    test_kkt_certificate_of_gpu_solutions and assert_ca_rule); and among the moved optima one holds a side the point set or moved in its active
    set -- lbx / ubx entries, the friction row's lower side (S4, S9, FLOU); S5 sets none"""
    name, fam = case
    pt, cfg = BS.point(name, fam), BS.cfg_of(fam)
    b = BS.bounds(name, fam)
    nlp = BicycleNLP(cfg)
    r = BS.oracle_rows(name, fam)
    _, p = BS.inputs(name, fam, BS.QB)
    conv, both, d = moved(name, fam)
    rows = np.flatnonzero(both & (d > 1e-3))
    new_lo, new_hi = BS.newly_bounded(name, fam)
    new = {("x", int(i), "lo") for i in new_lo} | {("x", int(i), "hi") for i in new_hi} | ({("g", 0, "lo")} if b[0][0] > 0.0 else set())
    hit = set()
    for n, i in enumerate(rows):
        if n >= 4 and (hit or not new):
            break
        cert = kkt_certificate(nlp, r["x"][i], p[i], bounds=b)
        if n < 4:
            assert cert["stationarity"] <= 1e-6 and cert["feasibility"] <= 1e-6, (i, cert)
        hit |= new & set(cert["active"])
    print(f"{name} {fam}: {min(4, len(rows))} optima certified; sides of the point in an active set: {sorted(hit)[:6]}")
    assert len(rows) >= (4 if pt.binding == "binds" else 1)
    assert hit or not new


def test_kkt_certificate_default_is_unchanged():
    """bounds=None is the reference's bounds: the same figures as with them passed, and no "active" key for the existing callers to trip over"""
    cfg = BS.cfg_of("n10")
    nlp = BicycleNLP(cfg)
    r = BS.reference_rows("S1", "n10")
    _, p = BS.inputs("S1", "n10", 2)
    a = kkt_certificate(nlp, r["x"][0], p[0])
    c = kkt_certificate(nlp, r["x"][0], p[0], bounds=nlp.bounds())
    assert "active" not in a and {k: c[k] for k in a} == a and a["stationarity"] <= 1e-6


# ---- (5) -------------------------------------------------------------------------------------------------------------------------------------
def refusals(cfg):
    """name -> (lbg, ubg, lbx, ubx) that mpc_set_bounds refuses with MPC_ERR_BOUNDS"""
    nlp = BicycleNLP(cfg)
    first = nlp.row_obst(0)

    def case(edit):
        b = [np.array(a, dtype=np.float64) for a in nlp.bounds()]
        edit(*b)
        return tuple(b)

    def eq(lbg, ubg, lbx, ubx): lbx[nlp.ix(3) + 3] = ubx[nlp.ix(3) + 3] = 10.0          # noqa: E704
    def gt(lbg, ubg, lbx, ubx): lbx[nlp.iu(2)] = 0.5                                     # noqa: E704  (above ubx = 0.4)
    def nan(lbg, ubg, lbx, ubx): ubx[nlp.ix(1) + 1] = np.nan                             # noqa: E704
    def circle(lbg, ubg, lbx, ubx): lbg[first + 4] = 1.0                                 # noqa: E704
    def circle_hi(lbg, ubg, lbx, ubx): ubg[first + 9 * cfg.N + 8] = 500.0                # noqa: E704
    def fric(lbg, ubg, lbx, ubx): lbg[0] = ubg[0]                                        # noqa: E704
    def fric_gt(lbg, ubg, lbx, ubx): lbg[0] = 12.0                                       # noqa: E704
    def equality(lbg, ubg, lbx, ubx): ubg[nlp.row_defect(1) + 2] = 1e-3                  # noqa: E704
    return {f.__name__: case(f) for f in (eq, gt, nan, circle, circle_hi, fric, fric_gt, equality)}


MPC_ERR_BOUNDS = -3


@pytest.mark.parametrize("fam", ["n10", "ca"])
def test_refusals_through_the_emulated_entry(fam):
    from helpers import abi
    assert abi.MPC_ERR_BOUNDS == MPC_ERR_BOUNDS
    cfg = BS.cfg_of(fam)
    x0, p = BS.inputs("S6", fam, 2)
    assert emu_solve(cfg, x0, p, want_rc=True) == 0
    for name, b in refusals(cfg).items():
        assert emu_solve(cfg, x0, p, bounds=b, want_rc=True) == MPC_ERR_BOUNDS, name


@pytest.mark.parametrize("fam", ["n10", "ca"])
def test_a_refused_call_leaves_the_problem_as_it_was(fam):
    """set_bounds (csrc/mpc_host_common.h) as a handle's second mpc_set_bounds call: refused lists -- each with a box on y and lbg[0] = 0.5 in front
    of its flaw, a structure the problem does not have -- leave LB, UB, the flags, the levels and the masks what the first call made them (the
    host used to rewrite LB / UB and the masks before it refused, beside the first call's bounds on the device); accepted lists replace them"""
    import ctypes as C
    from helpers import abi, emu_desc, emu_lib
    L = emu_lib()
    dpp = C.POINTER(C.c_double) * 4
    L.emu_set_bounds_twice.argtypes = [C.POINTER(abi.MpcProblemDesc), dpp, dpp, C.POINTER(C.c_int32)]
    L.emu_set_bounds_twice.restype = C.c_int
    cfg = BS.cfg_of(fam)
    d = emu_desc(cfg)
    pack = lambda b: [np.ascontiguousarray(a, dtype=np.float64) for a in (b[2], b[3], b[0], b[1])]     # noqa: E731  (lbx, ubx, lbg, ubg)
    ptrs = lambda arrs: dpp(*[a.ctypes.data_as(C.POINTER(C.c_double)) for a in arrs])                   # noqa: E731
    first = pack(BicycleNLP(cfg).bounds())
    same = C.c_int32(-1)
    for what, b in refusals(cfg).items():
        lbg, ubg, lbx, ubx = [a.copy() for a in b]
        lbx[BS.index(cfg, BS.Y, cfg.N)], ubx[BS.index(cfg, BS.Y, cfg.N)] = -50.0, 50.0
        if what not in ("fric", "fric_gt"):
            lbg[0] = 0.5
        second = pack((lbg, ubg, lbx, ubx))
        assert L.emu_set_bounds_twice(C.byref(d), ptrs(first), ptrs(second), C.byref(same)) == MPC_ERR_BOUNDS, what
        assert same.value == 1, what
    second = pack(BS.bounds("S6", fam))
    assert L.emu_set_bounds_twice(C.byref(d), ptrs(first), ptrs(second), C.byref(same)) == 0 and same.value == 0


# ---- (6) the reference of the bound sensitivities against its CPU harness at the points the GPU test uses -----------------------------------------
@pytest.mark.parametrize("case", list(BS.SENS_CASES), ids=BS.case_id)
def test_bound_sensitivity_reference_against_the_harness(case):
    """tests/sens_bounds_ref.py with the point's bounds against sensboundx_solve (the functions k_sens runs, behind the emulated solve) on the rows
    the GPU test compares, directions BS.sens_directions: within TOL_DW, the bound of tests/test_gpu_sens_bounds.py (measured: FLOU 8.2e-6, S9
    9.7e-7, so ten times the figure stays under the module's 1e-4 cap and no bound of S9's own is needed); the adjoint and the sum identities"""
    import ctypes as C
    import test_sens_bounds_cpu as T
    from helpers import abi, harness_lib
    name, fam = case
    B, rows = BS.SENS_CASES[case]
    cfg, b = BS.cfg_of(fam), BS.bounds(name, fam)
    x0, p = BS.inputs(name, fam, B)
    dbv, names = BS.sens_directions(name, fam, B)
    x0, p, dbv = x0[rows], p[rows], dbv[rows]
    seeds = np.random.default_rng(5).normal(size=(len(rows), cfg.n_w))
    L = C.CDLL(harness_lib("sensx"))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L.sensboundx_solve.argtypes = [C.POINTER(abi.MpcProblemDesc), dp, dp, dp, dp, C.c_int32, dp, dp, dp, ip, dp, dp, C.c_int32, dp, dp, dp, dp, dp, ip, ip]
    r = T.run_sensboundx(L, cfg, x0, p, dbv, seeds, bounds=b)
    checked, weak, worst, resp = T.check_against_reference(cfg, r, p, dbv, b)
    print(f"{name} {fam}: {checked} rows checked, {weak} weakly active, worst error {worst:.2e} (bound {T.TOL_DW:.1e}); largest max|dw|: "
          + ", ".join(f"{n} {v:.3g}" for n, v in zip(names, resp[10:])))
    assert checked >= ((r["ok"] == 1).sum() + 1) // 2 and 10 * worst <= 1e-4 and worst <= T.TOL_DW
    assert resp[10 + names.index("ou")] < 1e-9                        # the circle rows' upper side binds nowhere
    assert resp[10 + names.index("fl" if fam == "ca" else "ubx[y_N]")] > 0.1
    T.check_adjoint(r, dbv, seeds)
    T.check_lam_identities(cfg, r)
    T.check_nan_rows(r)
