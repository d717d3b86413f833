"""CPU: the derivative of the optimum with respect to the obstacle centres behind mpc_sens_obst.

tests/sens_obst_ref.py (the active-set reduced KKT of tests/sens_ref.py with the obstacle right-hand side) is checked against central
differences of the C oracle's solves; tests/sensx/sensx.cpp (sensobstx_solve) steps the kernels' own phase functions on the CPU with per-instance
obstacle rows and then runs the functions k_sens<NX, SensFamObst> runs on the GPU (csrc/mpc_sens.h), checked against that reference."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import CA_CFG, FAMILIES, ROOT, BicycleNLP, abi, ca_batch, emu_desc, harness_lib, synthetic_batch
from oracle.binding import OracleSolver
import sens_obst_ref
import sens_ref

NEW = ["mpc_sens_obst", "mpc_sens_obst_dev"]
H_FD = 1e-4
# lam_obst against central differences of the oracle's optimal objective: the worst relative error measured over the six instances is 4.3e-8
# (printed by the test).  The bound is ten times that, and never looser than 1e-4.
LAM_FD_BOUND = min(10 * 4.3e-8, 1e-4)


def test_new_entry_points_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mpcgpu.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in abi.EXPORTS, name
    if os.path.exists(abi.LIB_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", abi.LIB_PATH], capture_output=True, text=True, check=True).stdout
        for name in NEW:
            assert re.search(r"\bT %s$" % name, syms, re.M), name


# ---- 1 + 2. the numpy reference against central differences of the oracle's solves ------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_optima():
    """the six collision-avoidance optima at the descriptor's centres, their least-squares multipliers, and the oracle's solves with each
    centre coordinate moved alone by +-H_FD: (x, f) pairs"""
    cfg = CA_CFG
    x0, p = ca_batch(cfg, 6)
    c0 = cfg.obstacle_centers.ravel()
    kw = dict(tol=1e-10, max_iter=300)
    out = []
    for b in range(6):
        r = OracleSolver(cfg, **kw).solve(x0[b], p[b])
        assert r["status"] == 1
        lg, lx = sens_ref.ls_multipliers(cfg, r["x"], p[b])
        moved = []
        for q in range(6):
            e = np.zeros(6)
            e[q] = H_FD
            a = OracleSolver(sens_obst_ref.ObstCfg(cfg, c0 + e), **kw).solve(r["x"], p[b])
            m = OracleSolver(sens_obst_ref.ObstCfg(cfg, c0 - e), **kw).solve(r["x"], p[b])
            assert a["status"] == 1 and m["status"] == 1
            moved.append((a, m))
        out.append(dict(w=r["x"], f=r["f"], p=p[b], lam_g=lg, lam_x=lx, moved=moved))
    return c0, out


def test_reference_matches_finite_differences(oracle_optima):
    c0, opt = oracle_optima
    nlp = BicycleNLP(CA_CFG)
    checked = 0
    for b, o in enumerate(opt):
        assert np.min(o["lam_g"][nlp.row_obst(0):]) < -1e-3                   # every instance has active circle rows
        S, weak = sens_obst_ref.sensitivity_matrix(CA_CFG, c0, o["w"], o["p"], o["lam_g"], o["lam_x"])
        if weak:
            continue
        for q, (a, m) in enumerate(o["moved"]):
            fd = (a["x"] - m["x"]) / (2 * H_FD)
            err = np.max(np.abs(S[:, q] - fd))
            assert err <= 1e-4 * max(1.0, np.max(np.abs(fd))), (b, q, err)
        assert np.max(np.abs(S)) > 0.1                                        # the plan moves with the obstacle
        checked += 1
    assert checked >= 4, checked


def test_reference_lam_obst_is_the_gradient_of_the_optimal_objective(oracle_optima):
    c0, opt = oracle_optima
    worst = 0.0
    for b, o in enumerate(opt):
        lo = sens_obst_ref.lam_obst(CA_CFG, c0, o["w"], o["lam_g"])
        fd = np.array([(a["f"] - m["f"]) / (2 * H_FD) for a, m in o["moved"]])
        err = np.max(np.abs(lo - fd)) / max(1.0, np.max(np.abs(fd)))
        print(f"\n  instance {b}: lam_obst {lo}, relative error against central differences of f* {err:.2e}")
        worst = max(worst, err)
        assert np.max(np.abs(fd)) > 1e-2
    print(f"\n  lam_obst vs central differences of the oracle's optimal objective: worst relative error {worst:.2e}")
    assert worst <= LAM_FD_BOUND


# ---- 3. the kernel's math on the CPU ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sensobstx():
    L = C.CDLL(harness_lib("sensx"))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L.sensobstx_solve.argtypes = [C.POINTER(abi.MpcProblemDesc), dp, dp, dp, dp, C.c_int32, dp, dp, dp, dp, ip, dp, dp, C.c_int32, dp, dp, dp, dp,
                                  dp, ip, ip]
    L.sensobstx_circle.argtypes = [C.POINTER(abi.MpcProblemDesc), dp, C.c_int32, C.c_double, C.c_double, C.c_double, dp, dp, dp, dp, dp]
    return L


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def obst_rows(cfg, B, step=0.15):
    """the descriptor's centres shifted by a few decimetres per instance (every instance another row)"""
    c0 = cfg.obstacle_centers.ravel()
    sh = np.array([[step * (b % 4) - 0.2, 0.1 * ((b * 3) % 5) - 0.2] for b in range(B)])
    return c0[None, :] + np.tile(sh, (1, 3))


def directions(B, rng):
    """the six unit directions and one random one"""
    d = np.zeros((B, 7, 6))
    d[:, :6] = np.eye(6)
    d[:, 6] = rng.normal(size=(B, 6))
    return d


def run_sensobstx(L, cfg, x0, p, obst, dobst, seeds, force_bad=None):
    nlp = BicycleNLP(cfg)
    lbg, ubg, lbx, ubx = nlp.bounds()
    B, nw = x0.shape
    nd = dobst.shape[1]
    x0, p, obst = [np.ascontiguousarray(a, dtype=np.float64) for a in (x0, p, obst)]
    out, st, ok = np.empty_like(x0), np.empty(B, np.int32), np.empty(B, np.int32)
    lg, lx = np.empty((B, nlp.n_g)), np.empty((B, nw))
    dw, go, lo = np.empty((B, nd, nw)), np.empty((B, 6)), np.empty((B, 6))
    fb = np.zeros(B, np.int32) if force_bad is None else np.ascontiguousarray(force_bad, dtype=np.int32)
    d = emu_desc(cfg)
    assert L.sensobstx_solve(C.byref(d), _dp(lbx), _dp(ubx), _dp(lbg), _dp(ubg), B, _dp(x0), _dp(p), _dp(obst), _dp(out), _ip(st), _dp(lg), _dp(lx),
                             nd, _dp(np.ascontiguousarray(dobst)), _dp(dw), _dp(np.ascontiguousarray(seeds)), _dp(go), _dp(lo), _ip(ok), _ip(fb)) == 0
    return dict(x=out, status=st, lam_g=lg, lam_x=lx, dw=dw, grad_obst=go, lam_obst=lo, ok=ok)


def check_against_reference(cfg, r, p, obst, dobst, tol):
    """dw and lam_obst of every strictly complementary converged row against sens_obst_ref; returns (checked, weakly active)"""
    checked = weak_n = 0
    for b in np.flatnonzero(r["ok"] == 1):
        lo = sens_obst_ref.lam_obst(cfg, obst[b], r["x"][b], r["lam_g"][b])
        assert np.max(np.abs(r["lam_obst"][b] - lo)) <= 1e-12 * max(1.0, np.max(np.abs(lo))), (b, r["lam_obst"][b], lo)
        S, weak = sens_obst_ref.sensitivity_matrix(cfg, obst[b], r["x"][b], p[b], r["lam_g"][b], r["lam_x"][b])
        if weak:
            weak_n += 1
            continue
        ref = np.einsum("ij,dj->di", S, dobst[b])
        err = np.max(np.abs(r["dw"][b] - ref)) / max(1.0, np.max(np.abs(ref)))
        assert err <= tol, (b, err)
        checked += 1
    return checked, weak_n


def check_adjoint(r, dobst, seeds):
    for b in np.flatnonzero(r["ok"] == 1):
        for d in range(dobst.shape[1]):
            lhs, rhs = seeds[b] @ r["dw"][b, d], r["grad_obst"][b] @ dobst[b, d]
            assert abs(lhs - rhs) <= 1e-10 * max(1.0, np.abs(seeds[b]).sum() * np.max(np.abs(r["dw"][b, d]))), (b, d, lhs, rhs)


def check_nan_rows(r):
    bad = r["ok"] != 1
    assert np.all(r["ok"][r["status"] != 1] == 0)
    assert np.all(np.isnan(r["dw"][bad])) and np.all(np.isnan(r["grad_obst"][bad])) and np.all(np.isnan(r["lam_obst"][bad]))
    good = ~bad
    assert np.all(np.isfinite(r["dw"][good])) and np.all(np.isfinite(r["grad_obst"][good])) and np.all(np.isfinite(r["lam_obst"][good]))


def test_harness_collision_avoidance(sensobstx):
    B = 6
    x0, p = ca_batch(CA_CFG, B)
    obst = obst_rows(CA_CFG, B)
    rng = np.random.default_rng(21)
    dobst, seeds = directions(B, rng), rng.normal(size=(B, CA_CFG.n_w))
    force_bad = np.zeros(B, np.int32)
    force_bad[2] = 1
    r = run_sensobstx(sensobstx, CA_CFG, x0, p, obst, dobst, seeds, force_bad)
    conv = r["status"] == 1
    assert np.sum(conv) >= 4 and r["ok"][2] == 0
    nlp = BicycleNLP(CA_CFG)
    assert np.min(r["lam_g"][conv][:, nlp.row_obst(0):]) < -1e-3              # active circle rows
    checked, weak = check_against_reference(CA_CFG, r, p, obst, dobst, 1e-5)
    assert checked >= (np.sum(conv) + 1) // 2, (checked, weak)
    assert np.nanmax(np.abs(r["dw"])) > 0.1
    check_adjoint(r, dobst, seeds)
    check_nan_rows(r)


@pytest.mark.parametrize("fam", ["zamlf_n10_nx5", "zamlf_n30_nx6"])
def test_harness_lane_following_is_zero(sensobstx, fam):
    """the obstacle is far away: no circle row is active, the reference's derivative is exactly 0 and the barrier's (z / gap of rows a hundred
    metres from their bound) is zero to the tolerance"""
    cfg, kw = FAMILIES[fam]
    B = 4
    x0, p = synthetic_batch(cfg, B, **kw)
    obst = obst_rows(cfg, B)
    rng = np.random.default_rng(22)
    dobst, seeds = directions(B, rng), rng.normal(size=(B, cfg.n_w))
    r = run_sensobstx(sensobstx, cfg, x0, p, obst, dobst, seeds)
    assert np.all(r["status"] == 1) and np.all(r["ok"] == 1)
    for b in range(B):
        S, _ = sens_obst_ref.sensitivity_matrix(cfg, obst[b], r["x"][b], p[b], r["lam_g"][b], r["lam_x"][b])
        assert not S.any()
    assert np.max(np.abs(r["dw"])) <= 1e-5
    check_adjoint(r, dobst, seeds)
    for b in range(B):
        lo = sens_obst_ref.lam_obst(cfg, obst[b], r["x"][b], r["lam_g"][b])
        assert np.max(np.abs(r["lam_obst"][b] - lo)) <= 1e-12 * max(1.0, np.max(np.abs(lo)))


def test_circle_derivatives_follow_circle_eval(sensobstx):
    """circle_eval_centre against circle_eval: the same distance, and its derivatives with respect to the obstacle circle's centre by central
    differences of circle_eval's distance (the mixed second derivative by second differences)"""
    cfg = CA_CFG
    d = emu_desc(cfg)
    rng = np.random.default_rng(23)

    def ev(ob, j, sx, sy, psi):
        dist, only = np.empty(1), np.empty(1)
        J, Jo, Hxo = np.empty(3), np.empty(2), np.empty(6)
        assert sensobstx.sensobstx_circle(C.byref(d), _dp(np.ascontiguousarray(ob)), j, sx, sy, psi, _dp(dist), _dp(only), _dp(J), _dp(Jo), _dp(Hxo)) == 0
        return dist[0], only[0], J, Jo, Hxo.reshape(3, 2)

    for _ in range(20):
        ob = rng.normal(0, 20, size=6)
        x = np.array([rng.normal(0, 20), rng.normal(0, 20), rng.uniform(-3, 3)])
        for j in range(3):
            dist, only, J, Jo, Hxo = ev(ob, j, *x)
            assert dist == only
            eps, eps2 = 1e-6, 1e-4
            for c in range(2):
                e = np.zeros(6)
                e[2 * j + c] = 1.0
                fd = (ev(ob + eps * e, j, *x)[1] - ev(ob - eps * e, j, *x)[1]) / (2 * eps)
                assert abs(Jo[c] - fd) <= 1e-7 * max(1.0, abs(fd)), (j, c, Jo[c], fd)
                for r_ in range(3):
                    ex = np.zeros(3)
                    ex[r_] = eps2
                    f = lambda sx_, so_: ev(ob + so_ * eps2 * e, j, *(x + sx_ * ex))[1]           # noqa: E731
                    fd2 = (f(1, 1) - f(1, -1) - f(-1, 1) + f(-1, -1)) / (4 * eps2 * eps2)
                    assert abs(Hxo[r_, c] - fd2) <= 1e-5 * max(1.0, abs(fd2)), (j, r_, c, Hxo[r_, c], fd2)
            # another circle's centre does not enter
            other = np.zeros(6)
            other[2 * ((j + 1) % 3)] = 1.0
            assert ev(ob + other, j, *x)[1] == only
