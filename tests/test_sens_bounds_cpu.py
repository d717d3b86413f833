"""CPU: the derivative of the optimum with respect to the bounds and the circle radius behind mpc_sens_bounds, and mpc_get_bounds' declaration
(DESIGN.md section 13).

tests/sens_bounds_ref.py (the active-set reduced KKT of tests/sens_ref.py with the bounds' right-hand side) is checked against central
differences of the C oracle's re-solves; tests/sensx/sensx.cpp (sensboundx_solve) steps the kernels' own phase functions on the CPU and then runs the
functions k_sens<NX, SensFamBounds> runs on the GPU (csrc/mpc_sens.h), checked against that reference."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import CA_CFG, ROOT, WEIGHTS_ZAM_LF, BicycleNLP, NLPConfig, abi, ca_batch, emu_desc, harness_lib, synthetic_batch
from oracle.binding import OracleSolver
import sens_ref
import sens_bounds_ref as bref
from sens_bounds_ref import TOL_DW

NEW = ["mpc_sens_bounds", "mpc_sens_bounds_dev", "mpc_get_bounds"]
LF_CFG = NLPConfig(N=10, nx=6, **WEIGHTS_ZAM_LF)
H = 1e-5
N_DIR = 10
WANT_FLOOR = 0.1                # of the error's denominator: the smallest active response found (fu, 0.15) stays on its own scale


def test_new_entry_points_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mpcgpu.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in abi.EXPORTS, name
    if os.path.exists(abi.LIB_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", abi.LIB_PATH], capture_output=True, text=True, check=True).stdout
        for name in NEW:
            assert re.search(r"\bT %s$" % name, syms, re.M), name


def test_bound_vector_round_trip():
    for cfg in (CA_CFG, LF_CFG):
        bounds = BicycleNLP(cfg).bounds()
        bv = bref.bounds_vector(cfg)
        assert bv.shape == (bref.n_b(cfg),)
        for a, b in zip(bref.unpack_bounds(cfg, bv), bounds):
            assert np.array_equal(a, b)
        d = bref.level_directions(cfg)
        assert d.shape == (9, bref.n_b(cfg)) and np.all(np.isfinite(bv[d[0] != 0])) and np.all(d.sum(axis=0) <= 1.0)


# ---- the numpy reference against central differences of the oracle's re-solves -------------------------------------------------------------
def batches():
    x0, p = ca_batch(CA_CFG, 6)
    yield "ca", CA_CFG, x0, p
    x0, p = synthetic_batch(LF_CFG, 4)
    yield "lf", LF_CFG, x0, p


def moved_oracle(cfg, bv, **kw):
    """the oracle with the bounds of bv"""
    o = OracleSolver(cfg, **kw)
    lbg, ubg, lbx, ubx = bref.unpack_bounds(cfg, bv)
    o.lbx, o.ubx = np.ascontiguousarray(lbx), np.ascontiguousarray(ubx)
    o.desc.fric_hi, o.desc.obst_lo = float(ubg[0]), float(lbg[-1])
    return o


@pytest.fixture(scope="module")
def oracle_optima():
    """per batch and row: the oracle's optimum, its least-squares multipliers, and the re-solves (warm-started at the optimum) with the bounds
    moved by +-H along each of the nine level directions"""
    kw = dict(tol=1e-10, max_iter=300)
    out = {}
    for name, cfg, x0, p in batches():
        bv, levels = bref.bounds_vector(cfg), bref.level_directions(cfg)
        rows = []
        for b in range(x0.shape[0]):
            r = OracleSolver(cfg, **kw).solve(x0[b], p[b])
            assert r["status"] == 1
            lg, lx = sens_ref.ls_multipliers(cfg, r["x"], p[b])
            moved = []
            for d in levels:
                a = moved_oracle(cfg, bv + H * d, **kw).solve(r["x"], p[b])
                m = moved_oracle(cfg, bv - H * d, **kw).solve(r["x"], p[b])
                assert a["status"] == 1 and m["status"] == 1
                moved.append((a, m))
            rows.append(dict(w=r["x"], f=r["f"], p=p[b], lam_g=lg, lam_x=lx, moved=moved))
        out[name] = (cfg, rows)
    return out


def test_reference_matches_finite_differences(oracle_optima):
    need = dict(ca=5, lf=4)
    for name, (cfg, rows) in oracle_optima.items():
        levels = bref.level_directions(cfg)
        checked, worst, active = 0, 0.0, set()
        for b, o in enumerate(rows):
            S, weak = bref.sensitivity_matrix(cfg, o["w"], o["p"], o["lam_g"], o["lam_x"])
            if weak:
                continue
            for q, (a, m) in enumerate(o["moved"]):
                fd = (a["x"] - m["x"]) / (2 * H)
                got, mx = S @ levels[q], np.max(np.abs(fd))
                err = np.max(np.abs(got - fd))
                if mx < 1e-6:
                    assert err <= 1e-6, (name, b, bref.LEVELS[q], err)
                else:
                    active.add(bref.LEVELS[q])
                    worst = max(worst, err / mx)
                    assert err <= 1e-5 * mx, (name, b, bref.LEVELS[q], err / mx)
            checked += 1
        print(f"\n  {name}: dw/dbv vs central differences of the oracle's re-solves: {checked} of {len(rows)} rows, worst relative error {worst:.2e}, "
              f"directions with a response: {sorted(active)}")
        assert checked >= need[name], (name, checked)
        if name == "ca":
            assert {"deltav_min", "deltav_max", "fu", "ol"} <= active


def test_reference_lam_bounds_is_the_gradient_of_the_optimal_objective(oracle_optima):
    for name, (cfg, rows) in oracle_optima.items():
        levels = bref.level_directions(cfg)
        worst = 0.0
        for b, o in enumerate(rows):
            lb = levels @ bref.lam_bounds(cfg, o["lam_g"], o["lam_x"])
            fd = np.array([(a["f"] - m["f"]) / (2 * H) for a, m in o["moved"]])
            err = np.max(np.abs(lb - fd) / np.maximum(1.0, np.abs(fd)))
            worst = max(worst, err)
            assert err <= 1e-5, (name, b, lb, fd)
        print(f"\n  {name}: lam_bounds vs central differences of the oracle's optimal objective: worst error {worst:.2e}")


# ---- the kernel's math on the CPU -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sensboundx():
    L = C.CDLL(harness_lib("sensx"))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L.sensboundx_solve.argtypes = [C.POINTER(abi.MpcProblemDesc), dp, dp, dp, dp, C.c_int32, dp, dp, dp, ip, dp, dp, C.c_int32, dp, dp, dp, dp, dp, ip, ip]
    return L


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def directions(cfg, B, rng):
    """the nine level directions and one random per-entry direction, its entries in [-1, 1] as a level direction's are (the entries of absent
    bounds included: they are not read)"""
    d = np.zeros((B, N_DIR, bref.n_b(cfg)))
    d[:, :9] = bref.level_directions(cfg)
    d[:, 9] = rng.uniform(-1.0, 1.0, size=(B, bref.n_b(cfg)))
    return d


def run_sensboundx(L, cfg, x0, p, dbv, seeds, force_bad=None, bounds=None):
    nlp = BicycleNLP(cfg)
    lbg, ubg, lbx, ubx = [np.ascontiguousarray(a, dtype=np.float64) for a in (nlp.bounds() if bounds is None else bounds)]
    B, nw = x0.shape
    nd, nb = dbv.shape[1], bref.n_b(cfg)
    x0, p = [np.ascontiguousarray(a, dtype=np.float64) for a in (x0, p)]
    out, st, ok = np.empty_like(x0), np.empty(B, np.int32), np.empty(B, np.int32)
    lg, lx = np.empty((B, nlp.n_g)), np.empty((B, nw))
    dw, gb, lb = np.empty((B, nd, nw)), np.empty((B, nb)), np.empty((B, nb))
    fb = np.zeros(B, np.int32) if force_bad is None else np.ascontiguousarray(force_bad, dtype=np.int32)
    d = emu_desc(cfg)
    assert L.sensboundx_solve(C.byref(d), _dp(lbx), _dp(ubx), _dp(lbg), _dp(ubg), B, _dp(x0), _dp(p), _dp(out), _ip(st), _dp(lg), _dp(lx), nd,
                              _dp(np.ascontiguousarray(dbv)), _dp(dw), _dp(np.ascontiguousarray(seeds)), _dp(gb), _dp(lb), _ip(ok), _ip(fb)) == 0
    return dict(x=out, status=st, lam_g=lg, lam_x=lx, dw=dw, grad_bv=gb, lam_bv=lb, ok=ok)


def dw_error(got, want):
    return np.max(np.abs(got - want)) / max(np.max(np.abs(want)), WANT_FLOOR)


def check_against_reference(cfg, r, p, dbv, bounds=None):
    """dw of every strictly complementary good row against sens_bounds_ref; returns (rows checked, weakly active rows, the worst error over
    rows and directions, per direction the largest max|dw| over the checked rows)"""
    checked = weak_n = 0
    worst, resp = 0.0, np.zeros(dbv.shape[1])
    for b in np.flatnonzero(r["ok"] == 1):
        S, weak = bref.sensitivity_matrix(cfg, r["x"][b], p[b], r["lam_g"][b], r["lam_x"][b], bounds)
        if weak:
            weak_n += 1
            continue
        safe = np.where(np.isfinite(bref.bounds_vector(cfg, bounds)), dbv[b], 0.0)    # (an absent bound's entry is not read)
        want = np.einsum("ij,dj->di", S, safe)
        for d in range(dbv.shape[1]):
            worst = max(worst, dw_error(r["dw"][b, d], want[d]))
            resp[d] = max(resp[d], np.max(np.abs(r["dw"][b, d])))
        checked += 1
    return checked, weak_n, worst, resp


def check_lam_identities(cfg, r):
    """lam_bv against the solve's own multipliers: the three sum identities to 1e-12 relative, and the signs"""
    nw, first = cfg.n_w, 1 + cfg.nx * (cfg.N + 1)
    worst = 0.0
    for b in np.flatnonzero(r["ok"] == 1):
        lb, lg, lx = r["lam_bv"][b], r["lam_g"][b], r["lam_x"][b]
        pairs = [(lb[:nw] + lb[nw: 2 * nw], -lx), (lb[2 * nw] + lb[2 * nw + 1], -lg[0]), (lb[2 * nw + 2] + lb[2 * nw + 3], -lg[first:].sum())]
        for got, want in pairs:
            err = np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))
            worst = max(worst, err)
            assert err <= 1e-12, (b, got, want)
        assert np.all(lb[:nw] >= 0.0) and np.all(lb[nw: 2 * nw] <= 0.0)
        assert lb[2 * nw] >= 0.0 and lb[2 * nw + 1] <= 0.0 and lb[2 * nw + 2] >= 0.0 and lb[2 * nw + 3] <= 0.0
    return worst


def check_adjoint(r, dbv, seeds):
    worst = 0.0
    for b in np.flatnonzero(r["ok"] == 1):
        for d in range(dbv.shape[1]):
            lhs, rhs = seeds[b] @ r["dw"][b, d], r["grad_bv"][b] @ dbv[b, d]
            scale = max(1.0, np.abs(seeds[b]).sum() * np.max(np.abs(r["dw"][b, d])))
            worst = max(worst, abs(lhs - rhs) / scale)
            assert abs(lhs - rhs) <= 1e-10 * scale, (b, d, lhs, rhs)
    return worst


def check_absent_entries(cfg, r):
    absent = ~np.isfinite(bref.bounds_vector(cfg))
    absent[2 * cfg.n_w] = True                                                       # fl: not imposed under friction_lb = nlp
    good = r["ok"] == 1
    assert absent.sum() > cfg.n_w and np.all(r["grad_bv"][good][:, absent] == 0.0) and np.all(r["lam_bv"][good][:, absent] == 0.0)


def check_nan_rows(r):
    bad = r["ok"] != 1
    assert np.all(r["ok"][r["status"] != 1] == 0)
    assert np.all(np.isnan(r["dw"][bad])) and np.all(np.isnan(r["grad_bv"][bad])) and np.all(np.isnan(r["lam_bv"][bad]))
    good = ~bad
    assert np.all(np.isfinite(r["dw"][good])) and np.all(np.isfinite(r["grad_bv"][good])) and np.all(np.isfinite(r["lam_bv"][good]))


def test_harness_collision_avoidance(sensboundx):
    B = 6
    x0, p = ca_batch(CA_CFG, B)
    rng = np.random.default_rng(61)
    dbv, seeds = directions(CA_CFG, B, rng), rng.normal(size=(B, CA_CFG.n_w))
    force_bad = np.zeros(B, np.int32)
    force_bad[2] = 1
    r = run_sensboundx(sensboundx, CA_CFG, x0, p, dbv, seeds, force_bad)
    conv = r["status"] == 1
    assert np.sum(conv) >= 4 and r["ok"][2] == 0
    checked, weak, worst, resp = check_against_reference(CA_CFG, r, p, dbv)
    print(f"\n  CA: dw vs numpy: {checked} rows checked, {weak} weakly active, worst max|dw - want| / max(max|want|, 0.1) {worst:.2e} (bound {TOL_DW:.1e})")
    print("  CA: largest max|dw| per direction: " + ", ".join(f"{n} {v:.3g}" for n, v in zip(bref.LEVELS + ("random",), resp)))
    assert checked >= (np.sum(r["ok"] == 1) + 1) // 2, (checked, weak)
    assert worst <= TOL_DW
    assert resp[0] > 0.1 and resp[1] > 0.1 and resp[7] > 0.01 and resp[8] > 0.1       # deltav_min, deltav_max, fu, ol move the plan
    print(f"  CA: adjoint identity, worst scaled difference {check_adjoint(r, dbv, seeds):.2e}")
    print(f"  CA: lam_bv sum identities, worst relative difference {check_lam_identities(CA_CFG, r):.2e}")
    check_absent_entries(CA_CFG, r)
    check_nan_rows(r)


def test_harness_lane_following_nx6(sensboundx):
    B = 4
    x0, p = synthetic_batch(LF_CFG, B)
    rng = np.random.default_rng(62)
    dbv, seeds = directions(LF_CFG, B, rng), rng.normal(size=(B, LF_CFG.n_w))
    r = run_sensboundx(sensboundx, LF_CFG, x0, p, dbv, seeds)
    assert np.all(r["status"] == 1) and np.all(r["ok"] == 1)
    checked, weak, worst, resp = check_against_reference(LF_CFG, r, p, dbv)
    print(f"\n  LF nx = 6: dw vs numpy: {checked} rows checked, {weak} weakly active, worst max|dw - want| / max(max|want|, 0.1) {worst:.2e} (bound {TOL_DW:.1e})")
    print("  LF nx = 6: largest max|dw| per direction: " + ", ".join(f"{n} {v:.3g}" for n, v in zip(bref.LEVELS + ("random",), resp)))
    assert checked >= 2, (checked, weak)
    assert worst <= TOL_DW
    print(f"  LF nx = 6: adjoint identity, worst scaled difference {check_adjoint(r, dbv, seeds):.2e}")
    print(f"  LF nx = 6: lam_bv sum identities, worst relative difference {check_lam_identities(LF_CFG, r):.2e}")
    check_absent_entries(LF_CFG, r)
    check_nan_rows(r)


def test_harness_kept_friction_row_and_two_sided_circle_rows(sensboundx):
    """the paths the reference's bounds do not take: a friction lower bound above 0 keeps the friction row as a row with a slack bounded on both
    sides (|a_0^2 + c| >= 0.5 binds where the plan would coast), and a finite upper bound of the circle rows gives them two sides (inactive:
    the shift is dol to rounding).  Two more directions: fl and ou alone."""
    cfg, B = CA_CFG, 6
    nw, nb = cfg.n_w, bref.n_b(cfg)
    lbg, ubg, lbx, ubx = [a.copy() for a in BicycleNLP(cfg).bounds()]
    lbg[0] = 0.5
    ubg[1 + cfg.nx * (cfg.N + 1):] = 1000.0
    bounds = (lbg, ubg, lbx, ubx)
    x0, p = ca_batch(cfg, B)
    rng = np.random.default_rng(64)
    dbv = np.zeros((B, N_DIR + 2, nb))
    dbv[:, :N_DIR] = directions(cfg, B, rng)
    dbv[:, N_DIR, 2 * nw + bref.FL] = 1.0
    dbv[:, N_DIR + 1, 2 * nw + bref.OU] = 1.0
    seeds = rng.normal(size=(B, nw))
    r = run_sensboundx(sensboundx, cfg, x0, p, dbv, seeds, bounds=bounds)
    assert np.sum(r["ok"] == 1) >= 4
    checked, weak, worst, resp = check_against_reference(cfg, r, p, dbv, bounds)
    print(f"\n  CA, fl = 0.5, ou = 1000: dw vs numpy: {checked} rows checked, {weak} weakly active, worst error {worst:.2e} (bound {TOL_DW:.1e}); "
          f"largest max|dw|: fl {resp[N_DIR]:.3g}, fu {resp[7]:.3g}, ol {resp[8]:.3g}, ou {resp[N_DIR + 1]:.3g}")
    assert checked >= (np.sum(r["ok"] == 1) + 1) // 2, (checked, weak)
    assert worst <= TOL_DW
    assert resp[N_DIR] > 0.1 and resp[7] > 0.01 and resp[8] > 0.1 and resp[N_DIR + 1] < 1e-9      # both sides of the friction row bind somewhere; ou nowhere
    good = r["ok"] == 1
    assert np.any(r["lam_bv"][good, 2 * nw + bref.FL] > 0.1) and np.any(r["lam_bv"][good, 2 * nw + bref.FU] < -0.1)
    assert np.all(r["lam_bv"][good, 2 * nw + bref.OU] < 0.0) and np.all(r["lam_bv"][good, 2 * nw + bref.OU] > -1e-6)
    print(f"  adjoint identity, worst scaled difference {check_adjoint(r, dbv, seeds):.2e}")
    print(f"  lam_bv sum identities, worst relative difference {check_lam_identities(cfg, r):.2e}")
    check_nan_rows(r)


def test_absent_entries_are_not_read(sensboundx):
    """dw does not change when the dbv entry of an absent bound does -- even to NaN"""
    B = 2
    x0, p = synthetic_batch(LF_CFG, B)
    rng = np.random.default_rng(63)
    dbv, seeds = directions(LF_CFG, B, rng)[:, 8:], rng.normal(size=(B, LF_CFG.n_w))
    a = run_sensboundx(sensboundx, LF_CFG, x0, p, dbv, seeds)
    absent = ~np.isfinite(bref.bounds_vector(LF_CFG))
    absent[2 * LF_CFG.n_w] = True
    dbv2 = dbv.copy()
    dbv2[:, :, absent] = np.nan
    c = run_sensboundx(sensboundx, LF_CFG, x0, p, dbv2, seeds)
    assert np.all(a["ok"] == 1) and np.array_equal(a["dw"], c["dw"]) and np.max(np.abs(a["dw"][:, 1])) > 1e-3
