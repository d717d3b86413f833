"""GPU: every solve path under the bound structures of tests/bound_structures.py -- what mpc_set_bounds accepts and the reference never sets.

Every other GPU solve installs the reference's structure, so the kernels' branches on has_fl / has_fu / has_ou, on lo_mask / hi_mask / dense_mask and
on dec_s, the larger LDS stash of two-sided circle rows and the stored multiplier rows of further variables ran only where they had to reproduce
the compiled-in variant.  tests/test_bound_structures_cpu.py shows from the oracle alone that the points converge and that the binding ones move
the optimum, and holds the emulated solve to the oracle at them.

Lane following: statuses and iteration counts equal to the oracle's row for row (option rescue = 0: the oracle has no second chance), |x - x_oracle|
< TOL_ORACLE of tests/test_gpu_parity.py where converged; between the paths of a handle equal statuses and iterations and |dx| < 1e-9, the bound
test_compiled_in_bound_structure_against_the_run_time_lookup holds two instruction streams to.  Collision avoidance: the rule of
test_collision_avoidance_batch, certified with the point's bounds."""
import numpy as np
import pytest

import bound_structures as BS
from helpers import BicycleNLP, kkt_certificate, make_solver, pkg
from test_bound_structures_cpu import KEEP_VARIANT_2, refusals
from test_gpu_parity import TOL_ORACLE

pytestmark = pytest.mark.gpu

TOL_PATHS = 1e-9
PATHS = [("default", {}), ("pipeline_to_the_end", dict(hybrid="0")), ("one_launch_per_kernel", dict(hybrid="0", pipeline="0")),
         ("512_thread_workgroups", dict(hybrid="0", pipeline="0", big_wg="1"))]
VARIANT_0 = ("run_time_lookup", dict(bound_mask="0"))          # the points that keep the compiled-in variant (KEEP_VARIANT_2), looked up at run time
DEFAULTS = dict(hybrid="1", pipeline="1", big_wg="0", bound_mask="1")
LANE_CASES = BS.lane_cases(("n10", "n30")) + [("S3", "n50"), ("S6", "n50"), ("S9", "n64"), ("S6", "n64")]


def solver_at(name, fam, **opts):
    pt, cfg = BS.point(name, fam), BS.cfg_of(fam)
    s = make_solver(cfg, obst_mult=pt.mult(fam))
    BS.install(s, name, fam)
    if fam != "ca":
        s.set_option("rescue", "0")
    for k, v in opts.items():
        s.set_option(k, v)
    return s


def same_bits(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("x", "status", "iters", "kkt"))


def against_the_oracle(name, fam, r, B, start=0, label=""):
    """at most 64 evenly spaced rows of a lane-following solve against the oracle under the point's bounds"""
    step = BS.step64(B)
    ro = BS.oracle_rows(name, fam, B, start, step)
    x, st, it, kkt = r.x[::step], r.status[::step], r.iters[::step], r.kkt[::step]
    ok = ro["status"] == 1
    err = np.abs(x - ro["x"])[ok].max()
    print(f"{name} {fam} B={B} {label}: {int(ok.sum())} of {len(ok)} rows converged in the oracle, max |x - x_oracle| = {err:.2e}")
    assert np.array_equal(st, ro["status"]) and np.array_equal(it, ro["iters"])
    assert ok.mean() >= 0.9 and err < TOL_ORACLE
    assert kkt[ok].max() <= 1e-8
    return err


# ---- 3a: the solve on every path -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LANE_CASES, ids=BS.case_id)
def test_every_path_of_a_handle_against_the_oracle(case):
    """B = 130 (two full tiles and a ragged one) on one handle: default options (k_solve_wg alone behind the fused start kernel; N = 64: the
    512-thread kernels, one launch each), the pipeline to the end, one launch per kernel, the same in 512-thread workgroups -- and with the bounds
    looked up at run time where the point keeps the compiled-in variant"""
    name, fam = case
    s = solver_at(name, fam)
    x0, p = BS.inputs(name, fam, 130)
    res = {}
    for label, opts in PATHS + ([VARIANT_0] if name in KEEP_VARIANT_2 else []):
        for k, v in {**DEFAULTS, **opts}.items():
            s.set_option(k, v)
        res[label] = s.solve(x0, p)
        against_the_oracle(name, fam, res[label], 130, label=label)
        if fam in ("n10", "n30", "n50"):
            ran = (s.get_resident_profile()["ran"], s.get_pipeline_profile()["ran"])
            assert ran == {"default": (True, False), "run_time_lookup": (True, False), "pipeline_to_the_end": (False, True)}.get(label, (False, False)), (label, ran)
    ref = res["default"]
    ok = ref.status == 1
    worst = 0.0
    for label, r in res.items():
        assert np.array_equal(r.status, ref.status) and np.array_equal(r.iters, ref.iters), label
        worst = max(worst, float(np.abs(r.x - ref.x)[ok].max()))
    print(f"{name} {fam}: largest |dx| between the paths {worst:.2e}")
    assert worst < TOL_PATHS


def ca_rule(name, x, status, kkt, p, ro):
    """DF.assert_ca_rule with the point's bounds in the certificate: at least 85 % of the rows converged on both sides agree within 1e-6, every
    other row is a KKT point of the numpy NLP under the point's bounds at 1e-6 / 1e-6"""
    cfg, b = BS.cfg_of("ca"), BS.bounds(name, "ca")
    both = (status == 1) & (ro["status"] == 1)
    dist = np.abs(x - ro["x"]).max(axis=1)
    same = both & (dist < 1e-6)
    print(f"{name} ca: converged on both {int(both.sum())} of {len(status)}, same optimum {int(same.sum())}, worst distance among them {dist[same].max():.2e}")
    assert same.sum() >= 0.85 * both.sum() and both.sum() >= 0.85 * len(status)
    assert kkt[status == 1].max() <= 1e-8
    nlp = BicycleNLP(cfg)
    for i in np.flatnonzero(~same):
        assert status[i] == 1, i
        cert = kkt_certificate(nlp, x[i], p[i], bounds=b)
        assert cert["stationarity"] <= 1e-6 and cert["feasibility"] <= 1e-6, (i, cert)


@pytest.mark.parametrize("name", list(BS.CA_POINTS))
def test_collision_avoidance_points(name):
    """B = 130, default options and one launch per kernel: two-sided circle rows (S6), at obst_mult = 1 (S10), with the kept friction row (FLOU)"""
    s = solver_at(name, "ca")
    x0, p = BS.inputs(name, "ca", 130)
    ro = BS.oracle_rows(name, "ca", 130, 0, 3)
    for opts in ({}, dict(hybrid="0", pipeline="0")):
        for k, v in {**DEFAULTS, **opts}.items():
            s.set_option(k, v)
        r = s.solve(x0, p)
        ca_rule(name, r.x[::3], r.status[::3], r.kkt[::3], p[::3], ro)


def test_hybrid_hand_over_at_s9():
    """S9, N = 30, nx = 6, instances 1 .. 2305: the smallest batch the plan gives to both kernels on 256 CUs -- k_pipeline, then k_solve_wg on the
    tiles that left it, both in the general variant"""
    s = solver_at("S9", "n30")
    x0, p = BS.inputs("S9", "n30", 2305, 1)
    r = s.solve(x0, p)
    assert s.get_pipeline_profile()["ran"] and s.get_resident_profile()["ran"]
    against_the_oracle("S9", "n30", r, 2305, 1, "hybrid")


# ---- 3b: poison ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S6", "S9"])
def test_poisoned_workspace_changes_nothing(name):
    """option poison (NaN into every row of the workspace before a solve) at N = 30, B = 600, as
    test_poisoned_workspace_changes_nothing_on_single_tile_xcds: the larger stash and the further multiplier rows read nothing they did not write"""
    x0, p = BS.inputs(name, "n30", 600)
    for opts in (dict(hybrid="0"), dict(hybrid="0", pipeline="0"), {}):
        s = solver_at(name, "n30", **opts)
        ref = s.solve(x0, p)
        assert (ref.status == 1).mean() >= 0.9
        s.set_option("poison", "1")
        for rep in range(2):
            a = s.solve(x0, p)
            assert np.all(np.isfinite(a.x[ref.status == 1])), (opts, rep)
            assert same_bits(a, ref), (opts, rep)


# ---- 3c: multipliers -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(n, f) for f in ("n10", "n30") for n in ("S1", "S3", "S4", "S6", "S9")], ids=BS.case_id)
def test_multipliers_certify_under_the_points_bounds(case):
    """solve(..., multipliers=True), B = 64: kkt_violations / check_batch of tests/test_gpu_multipliers.py at that module's thresholds, with the
    point's bounds as the solve imposes them (BS.imposed: each side 1e-8 max(1, |bound|) further out, IPOPT's bound_relax_factor).  Against the
    bounds as given the complementarity figure of S3 and S9 is that relaxation times the multiplier of the y box, 2.2e-5 .. 6.6e-5 on the MI355X
    against the threshold 1e-5; the reference's bounds never carry a multiplier of that size.  f, g against the numpy NLP as
    test_multipliers_f_and_g holds them; a multiplier on a side the point set; get_bounds bit for bit"""
    from test_gpu_multipliers import check_batch
    name, fam = case
    cfg, b = BS.cfg_of(fam), BS.bounds(name, fam)
    s = solver_at(name, fam)
    for got, want in zip(s.get_bounds(), (b[2], b[3], b[0], b[1])):
        assert np.array_equal(got, want)
    x0, p = BS.inputs(name, fam, 64)
    r = s.solve(x0, p, multipliers=True)
    ok = r.status == 1
    assert ok.mean() >= 0.9
    check_batch(cfg, r, p, BS.imposed(b))
    f2, g2 = s.eval_nlp(r.x, p)
    assert np.array_equal(f2, r.f) and np.array_equal(g2, r.g)
    nlp = BicycleNLP(cfg)
    for i in np.flatnonzero(ok)[::4]:
        fr, gr = nlp.f(r.x[i], p[i]), nlp.g(r.x[i], p[i])
        assert abs(r.f[i] - fr) <= 1e-12 * abs(fr)
        assert np.max(np.abs(r.g[i] - gr) / np.maximum(1.0, np.abs(gr))) <= 1e-12 * max(1.0, np.max(np.abs(r.x[i])))
    new_lo, new_hi = BS.newly_bounded(name, fam)
    lo = float(-r.lam_x[ok][:, new_lo].min(initial=0.0))
    hi = float(r.lam_x[ok][:, new_hi].max(initial=0.0))
    print(f"{name} {fam}: largest multiplier on a lower bound the point set {lo:.3g}, on an upper one {hi:.3g}; lam_g[0] in "
          f"[{np.nanmin(r.lam_g[ok, 0]):.3g}, {np.nanmax(r.lam_g[ok, 0]):.3g}]")
    if name in ("S1", "S9"):
        assert lo > 1e-3
    if name in ("S3", "S9"):
        assert hi > 1e-3
    if name == "S4":
        # the kept row's lower side binds where the plan would coast: negative in CasADi's convention (a lower bound holds the row) ...
        assert np.nanmin(r.lam_g[ok, 0]) < -1e-3
        # ... and the upper side, a_max, where the plan brakes or accelerates at the cap: positive
        assert np.nanmax(r.lam_g[ok, 0]) > 1e-3
    if name == "S6":
        first = nlp.row_obst(0)
        assert np.abs(r.lam_g[ok][:, first:]).max() < 1e-6          # neither side of a circle row binds, a hundred metres from the dummy obstacle


# ---- 3d: bound sensitivities -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(BS.SENS_CASES), ids=BS.case_id)
def test_bound_sensitivities_at_the_points(case):
    """mpc_sens_bounds behind a solve at FLOU (collision avoidance, lbg[0] = 0.5, circle rows ubg = 1000: the case of the CPU harness test) and at
    S9, against tests/sens_bounds_ref.py with the point's bounds at TOL_DW (tests/test_bound_structures_cpu.py measures the reference against the CPU
    harness on the same rows); directions: the nine levels, a random one, fl, ou and the terminal y's upper bound; the adjoint identity and the
    lam_bv sum identities as tests/test_gpu_sens_bounds.py holds them"""
    import sens_bounds_ref as bref
    import test_sens_bounds_cpu as T
    name, fam = case
    B, rows = BS.SENS_CASES[case]
    cfg, b = BS.cfg_of(fam), BS.bounds(name, fam)
    s = solver_at(name, fam)
    x0, p = BS.inputs(name, fam, B)
    dbv, names = BS.sens_directions(name, fam, B)
    seeds = np.random.default_rng(5).normal(size=(B, cfg.n_w))
    r = s.solve(x0, p, multipliers=True, lam_p=True)
    o = s.sens_bounds(dbv, seeds, lam=True)
    good = (r.status == 1) & ~np.isnan(r.lam_g[:, 0])
    assert np.all(np.isnan(o.dw[~good])) and np.all(np.isfinite(o.dw[good])) and np.all(np.isfinite(o.grad_bv[good])) and np.all(np.isfinite(o.lam_bv[good]))
    sub = dict(x=r.x[rows], status=r.status[rows], lam_g=r.lam_g[rows], lam_x=r.lam_x[rows], dw=o.dw[rows], grad_bv=o.grad_bv[rows],
               lam_bv=o.lam_bv[rows], ok=good[rows].astype(np.int32))
    checked, weak, worst, resp = T.check_against_reference(cfg, sub, p[rows], dbv[rows], b)
    print(f"{name} {fam}: {checked} rows checked, {weak} weakly active, worst error {worst:.2e} (bound {bref.TOL_DW:.1e}); largest max|dw|: "
          + ", ".join(f"{n} {v:.3g}" for n, v in zip(names, resp[10:])))
    assert checked >= (good[rows].sum() + 1) // 2 and worst <= bref.TOL_DW
    assert resp[10 + names.index("ou")] < 1e-9
    assert resp[10 + names.index("fl" if fam == "ca" else "ubx[y_N]")] > 0.1
    whole = dict(x=r.x, status=r.status, lam_g=r.lam_g, lam_x=r.lam_x, dw=o.dw, grad_bv=o.grad_bv, lam_bv=o.lam_bv, ok=good.astype(np.int32))
    print(f"  adjoint identity {T.check_adjoint(whole, dbv, seeds):.2e}, lam_bv sum identities {T.check_lam_identities(cfg, whole):.2e}")
    absent = ~np.isfinite(bref.bounds_vector(cfg, b))
    assert np.all(o.grad_bv[good][:, absent] == 0.0) and np.all(o.lam_bv[good][:, absent] == 0.0)


# ---- 3e: the second chance ---------------------------------------------------------------------------------------------------------------------------
def test_second_chance_with_two_sided_circle_rows():
    """collision avoidance S6 (circle rows ubg = 60), B = 256, default option rescue: the levels inside k_solve_wg (rescue_wg = 2) and behind the
    launch (0) give the same bits and rescue the same instances; a row no level brings in is the plain solve's (rescue = 0) -- the assertions of
    test_second_chance_inside_the_launch_equals_the_one_behind_it, with two-sided circle rows in the restart code"""
    s = solver_at("S6", "ca")
    x0, p = BS.inputs("S6", "ca", 256)
    res, n = {}, {}
    for mode in ("2", "0"):
        s.set_option("rescue_wg", mode)
        res[mode] = s.solve(x0, p)
        n[mode] = s.last_rescued()
    s.set_option("rescue", "0")
    plain = s.solve(x0, p)
    stalled = np.flatnonzero(plain.status != 1)
    print(f"rescued inside the launch {n['2']}, behind it {n['0']}; stalled in the plain solve {stalled}; still open {np.flatnonzero(res['2'].status != 1)}")
    assert n["2"] == n["0"] == len(stalled) and len(stalled) > 0
    assert same_bits(res["2"], res["0"])
    a = res["2"]
    untouched = np.setdiff1d(np.arange(256), stalled)
    assert np.array_equal(a.x[untouched], plain.x[untouched]) and np.array_equal(a.iters[untouched], plain.iters[untouched])
    left = stalled[a.status[stalled] != 1]
    assert np.array_equal(a.x[left], plain.x[left]) and np.array_equal(a.status[left], plain.status[left]) and np.array_equal(a.iters[left], plain.iters[left])
    nlp, b = BicycleNLP(BS.cfg_of("ca")), BS.bounds("S6", "ca")
    for i in stalled[a.status[stalled] == 1][:4]:
        cert = kkt_certificate(nlp, a.x[i], p[i], bounds=b)
        assert cert["stationarity"] <= 1e-6 and cert["feasibility"] <= 1e-6, (i, cert)
        assert a.iters[i] > plain.iters[i]


# ---- 3f: refusals ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [("S9", "n10"), ("S6", "ca")], ids=BS.case_id)
def test_a_refused_call_leaves_the_handle_as_it_was(case):
    """every refusal of tests/test_bound_structures_cpu.py returns MPC_ERR_BOUNDS with a message; the handle then holds and returns the bounds it
    had, and solves to the bits of its solve before the refusals.

    Writing this test found set_bounds (csrc/mpc_host_common.h) rewriting LB / UB and the masks on the host before it refused, beside the previous
    call's bounds on the device: a handle at the reference bounds that was refused a box on y with a bad row behind it went on with lo_mask /
    hi_mask naming y, so with the compiled-in variant switched off.  It now parses into a copy."""
    from helpers import abi
    name, fam = case
    cfg = BS.cfg_of(fam)
    x0, p = BS.inputs(name, fam, 70)
    for at_point in (False, True):
        s = solver_at(name, fam) if at_point else make_solver(cfg)
        if not at_point:
            s.set_option("rescue", "0" if fam != "ca" else "1")
        held = s.get_bounds()
        ref = s.solve(x0, p)
        for what, b in refusals(cfg).items():
            lbg, ubg, lbx, ubx = [a.copy() for a in b]
            if not at_point:                                        # (a structure the handle does not have, in front of the flaw)
                lbx[BS.index(cfg, BS.Y, cfg.N)], ubx[BS.index(cfg, BS.Y, cfg.N)] = -50.0, 50.0
                if what not in ("fric", "fric_gt"):
                    lbg[0] = 0.5
            with pytest.raises(pkg.MpcError) as e:
                s.set_bounds(lbx, ubx, lbg, ubg)
            assert e.value.code == abi.MPC_ERR_BOUNDS and len(str(e.value)) > len("mpcgpu error -3: "), what
            for got, want in zip(s.get_bounds(), held):
                assert np.array_equal(got, want), what
            assert same_bits(s.solve(x0, p), ref), what
