"""CPU: the derivative of the optimum with respect to the cost weights behind mpc_sens_weights, and mpc_set_weights' declaration (DESIGN.md
section 13).

tests/sens_weights_ref.py (the active-set reduced KKT of tests/sens_ref.py with the weights' right-hand side) is checked against central
differences of the C oracle's re-solves; tests/sensx/sensx.cpp (sensweightx_solve) steps the kernels' own phase functions on the CPU and then runs the
functions k_sens<NX, SensFamWeights> runs on the GPU (csrc/mpc_sens.h), checked against that reference."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import CA_CFG, ROOT, WEIGHTS_ZAM_LF, BicycleNLP, NLPConfig, abi, ca_batch, emu_desc, harness_lib, synthetic_batch
from oracle.binding import OracleSolver
import sens_ref
import sens_weights_ref as wref
from sens_weights_ref import TOL_DW

NEW = ["mpc_set_weights", "mpc_sens_weights", "mpc_sens_weights_dev"]
LF_CFG = NLPConfig(N=10, nx=6, **WEIGHTS_ZAM_LF)
H_REL = 1e-4
N_DIR = 8


def test_new_entry_points_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mpcgpu.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in abi.EXPORTS, name
    if os.path.exists(abi.LIB_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", abi.LIB_PATH], capture_output=True, text=True, check=True).stdout
        for name in NEW:
            assert re.search(r"\bT %s$" % name, syms, re.M), name


# ---- the numpy reference against central differences of the oracle's re-solves -------------------------------------------------------------
def batches():
    x0, p = ca_batch(CA_CFG, 6)
    yield "ca", CA_CFG, x0, p
    x0, p = synthetic_batch(LF_CFG, 4)
    yield "lf", LF_CFG, x0, p


@pytest.fixture(scope="module")
def oracle_optima():
    """per batch and row: the oracle's optimum, its least-squares multipliers, and the re-solves (warm-started at the optimum) with each weight
    moved alone by +-H_REL max(1, weight)"""
    kw = dict(tol=1e-10, max_iter=300)
    out = {}
    for name, cfg, x0, p in batches():
        wt = wref.weights_of(cfg)
        rows = []
        for b in range(x0.shape[0]):
            r = OracleSolver(cfg, **kw).solve(x0[b], p[b])
            assert r["status"] == 1
            lg, lx = sens_ref.ls_multipliers(cfg, r["x"], p[b])
            moved = []
            for q in range(wref.N_WT):
                e = np.zeros(wref.N_WT)
                e[q] = H_REL * max(1.0, wt[q])
                a = OracleSolver(wref.with_weights(cfg, wt + e), **kw).solve(r["x"], p[b])
                m = OracleSolver(wref.with_weights(cfg, wt - e), **kw).solve(r["x"], p[b])
                assert a["status"] == 1 and m["status"] == 1
                moved.append((e[q], a, m))
            rows.append(dict(w=r["x"], f=r["f"], p=p[b], lam_g=lg, lam_x=lx, moved=moved))
        out[name] = (cfg, rows)
    return out


def test_reference_matches_finite_differences(oracle_optima):
    need = dict(ca=5, lf=4)
    for name, (cfg, rows) in oracle_optima.items():
        checked, worst = 0, 0.0
        for b, o in enumerate(rows):
            S, weak = wref.sensitivity_matrix(cfg, o["w"], o["p"], o["lam_g"], o["lam_x"])
            if weak:
                continue
            for q, (h, a, m) in enumerate(o["moved"]):
                fd = (a["x"] - m["x"]) / (2 * h)
                err = np.max(np.abs(S[:, q] - fd)) / np.max(np.abs(fd))
                worst = max(worst, err)
                assert err <= 1e-5, (name, b, q, err)
            checked += 1
        print(f"\n  {name}: dw/dwt vs central differences of the oracle's re-solves: {checked} of {len(rows)} rows, worst relative error {worst:.2e}")
        assert checked >= need[name], (name, checked)


def test_reference_lam_weights_is_the_gradient_of_the_optimal_objective(oracle_optima):
    for name, (cfg, rows) in oracle_optima.items():
        worst = 0.0
        for b, o in enumerate(rows):
            lw = wref.lam_weights(cfg, o["w"], o["p"])
            fd = np.array([(a["f"] - m["f"]) / (2 * h) for h, a, m in o["moved"]])
            err = np.max(np.abs(lw - fd) / np.maximum(1.0, np.abs(fd)))
            worst = max(worst, err)
            assert err <= 1e-5, (name, b, lw, fd)
        print(f"\n  {name}: lam_weights vs central differences of the oracle's optimal objective: worst error {worst:.2e}")


# ---- the kernel's math on the CPU -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sensweightx():
    L = C.CDLL(harness_lib("sensx"))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L.sensweightx_solve.argtypes = [C.POINTER(abi.MpcProblemDesc), dp, dp, dp, dp, C.c_int32, dp, dp, dp, ip, dp, dp, C.c_int32, dp, dp, dp, dp, dp, ip, ip]
    return L


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def directions(cfg, B, rng):
    """the seven log-directions wt_q e_q (unit directions would hide errors: |dw/dQ_delta| is ~6e-4 where Q_delta = 500) and one random
    relative direction"""
    wt = wref.weights_of(cfg)
    d = np.zeros((B, N_DIR, wref.N_WT))
    d[:, :7] = np.diag(wt)
    d[:, 7] = wt * rng.normal(size=(B, wref.N_WT))
    return d


def run_sensweightx(L, cfg, x0, p, dwt, seeds, force_bad=None):
    nlp = BicycleNLP(cfg)
    lbg, ubg, lbx, ubx = nlp.bounds()
    B, nw = x0.shape
    nd = dwt.shape[1]
    x0, p = [np.ascontiguousarray(a, dtype=np.float64) for a in (x0, p)]
    out, st, ok = np.empty_like(x0), np.empty(B, np.int32), np.empty(B, np.int32)
    lg, lx = np.empty((B, nlp.n_g)), np.empty((B, nw))
    dw, gw, lw = np.empty((B, nd, nw)), np.empty((B, wref.N_WT)), np.empty((B, wref.N_WT))
    fb = np.zeros(B, np.int32) if force_bad is None else np.ascontiguousarray(force_bad, dtype=np.int32)
    d = emu_desc(cfg)
    assert L.sensweightx_solve(C.byref(d), _dp(lbx), _dp(ubx), _dp(lbg), _dp(ubg), B, _dp(x0), _dp(p), _dp(out), _ip(st), _dp(lg), _dp(lx), nd,
                               _dp(np.ascontiguousarray(dwt)), _dp(dw), _dp(np.ascontiguousarray(seeds)), _dp(gw), _dp(lw), _ip(ok), _ip(fb)) == 0
    return dict(x=out, status=st, lam_g=lg, lam_x=lx, dw=dw, grad_wt=gw, lam_wt=lw, ok=ok)


def check_against_reference(cfg, r, p, dwt, min_want=None):
    """dw of every strictly complementary good row and lam_wt of every good row against sens_weights_ref; returns (rows checked, weakly
    active rows, the worst max|dw - want| / max|want| over rows and directions)"""
    checked = weak_n = 0
    worst = 0.0
    for b in np.flatnonzero(r["ok"] == 1):
        lw = wref.lam_weights(cfg, r["x"][b], p[b])
        assert np.max(np.abs(r["lam_wt"][b] - lw) / np.maximum(1.0, np.abs(lw))) <= 1e-12, (b, r["lam_wt"][b], lw)
        S, weak = wref.sensitivity_matrix(cfg, r["x"][b], p[b], r["lam_g"][b], r["lam_x"][b])
        if weak:
            weak_n += 1
            continue
        want = np.einsum("ij,dj->di", S, dwt[b])
        for d in range(dwt.shape[1]):
            mx = np.max(np.abs(want[d]))
            if min_want is not None and d < 7:
                assert mx > min_want, (b, d, mx)
            worst = max(worst, np.max(np.abs(r["dw"][b, d] - want[d])) / mx)
        checked += 1
    return checked, weak_n, worst


def check_adjoint(r, dwt, seeds):
    worst = 0.0
    for b in np.flatnonzero(r["ok"] == 1):
        for d in range(dwt.shape[1]):
            lhs, rhs = seeds[b] @ r["dw"][b, d], r["grad_wt"][b] @ dwt[b, d]
            scale = max(1.0, np.abs(seeds[b]).sum() * np.max(np.abs(r["dw"][b, d])))
            worst = max(worst, abs(lhs - rhs) / scale)
            assert abs(lhs - rhs) <= 1e-10 * scale, (b, d, lhs, rhs)
    return worst


def check_nan_rows(r):
    bad = r["ok"] != 1
    assert np.all(r["ok"][r["status"] != 1] == 0)
    assert np.all(np.isnan(r["dw"][bad])) and np.all(np.isnan(r["grad_wt"][bad])) and np.all(np.isnan(r["lam_wt"][bad]))
    good = ~bad
    assert np.all(np.isfinite(r["dw"][good])) and np.all(np.isfinite(r["grad_wt"][good])) and np.all(np.isfinite(r["lam_wt"][good]))


def test_harness_collision_avoidance(sensweightx):
    B = 6
    x0, p = ca_batch(CA_CFG, B)
    rng = np.random.default_rng(41)
    dwt, seeds = directions(CA_CFG, B, rng), rng.normal(size=(B, CA_CFG.n_w))
    force_bad = np.zeros(B, np.int32)
    force_bad[2] = 1
    r = run_sensweightx(sensweightx, CA_CFG, x0, p, dwt, seeds, force_bad)
    conv = r["status"] == 1
    assert np.sum(conv) >= 4 and r["ok"][2] == 0
    checked, weak, worst = check_against_reference(CA_CFG, r, p, dwt, min_want=1e-2)
    print(f"\n  CA: dw vs numpy: {checked} rows checked, {weak} weakly active, worst max|dw - want| / max|want| {worst:.2e} (bound {TOL_DW:.1e})")
    assert checked >= (np.sum(r["ok"] == 1) + 1) // 2, (checked, weak)
    assert worst <= TOL_DW
    print(f"  CA: adjoint identity, worst scaled difference {check_adjoint(r, dwt, seeds):.2e}")
    check_nan_rows(r)


def test_harness_lane_following_nx6(sensweightx):
    B = 4
    x0, p = synthetic_batch(LF_CFG, B)
    rng = np.random.default_rng(42)
    dwt, seeds = directions(LF_CFG, B, rng), rng.normal(size=(B, LF_CFG.n_w))
    r = run_sensweightx(sensweightx, LF_CFG, x0, p, dwt, seeds)
    assert np.all(r["status"] == 1) and np.all(r["ok"] == 1)
    checked, weak, worst = check_against_reference(LF_CFG, r, p, dwt)
    print(f"\n  LF nx = 6: dw vs numpy: {checked} rows checked, {weak} weakly active, worst max|dw - want| / max|want| {worst:.2e} (bound {TOL_DW:.1e})")
    assert checked >= 2, (checked, weak)
    assert worst <= TOL_DW
    print(f"  LF nx = 6: adjoint identity, worst scaled difference {check_adjoint(r, dwt, seeds):.2e}")
    check_nan_rows(r)
