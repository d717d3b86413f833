"""CPU: the parametric sensitivities behind mpc_solve_batch_sens / mpc_sens_adjoint.

tests/sens_ref.py (the active-set reduced KKT of the numpy NLP) is checked against central finite differences of the C oracle's solves at
golden optima; tests/sensx/sensx.cpp steps the kernels' own phase functions on the CPU and then runs the functions k_sens_gather,
k_sens_lam_p and k_sens<NX, SensFamP> run on the GPU (csrc/mpc_sens.h), checked against that reference."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import CA_CFG, FAMILIES, ROOT, BicycleNLP, abi, ca_batch, cfg_from_golden, emu_desc, harness_lib, synthetic_batch
from oracle.binding import OracleSolver
import sens_ref

NEW = ["mpc_solve_batch_sens", "mpc_solve_batch_sens_dev", "mpc_sens_adjoint", "mpc_sens_adjoint_dev"]
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "nlp_optima.npz"))


def test_new_entry_points_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mpcgpu.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in abi.EXPORTS, name
    if os.path.exists(abi.LIB_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", abi.LIB_PATH], capture_output=True, text=True, check=True).stdout
        for name in NEW:
            assert re.search(r"\bT %s$" % name, syms, re.M), name


# ---- 1. the numpy reference against finite differences of the oracle's solves ----------------------------------------------------------
def _fd(orc, w, p, dp, h):
    a, b = orc.solve(w, p + h * dp), orc.solve(w, p - h * dp)
    assert a["status"] == 1 and b["status"] == 1
    return (a["x"] - b["x"]) / (2 * h)


@pytest.mark.parametrize("fam", ["zamlf_n10_nx5", "usalf_n10_nx5", "zamca_n30_nx5", "first_n10_nx5", "zamlf_n30_nx6"])
def test_reference_matches_finite_differences(fam):
    cfg = cfg_from_golden(GOLD[fam + "__cfg"])
    W, Pm = GOLD[fam + "__w"], GOLD[fam + "__p"]
    orc = OracleSolver(cfg, tol=1e-10, max_iter=200)
    nlp = BicycleNLP(cfg)
    rng = np.random.default_rng(5)
    checked = 0
    for b in range(min(3, W.shape[0])):
        w, p = W[b], Pm[b]
        lg, lx = sens_ref.ls_multipliers(cfg, w, p)
        S, weak = sens_ref.sensitivity_matrix(cfg, w, p, lg, lx)
        if weak:
            continue
        x0 = nlp.ix(0)
        seeds = [rng.normal(size=cfg.n_w)] + [np.eye(cfg.n_w)[x0 + i] for i in (2, 3)]
        for dp in seeds:
            dp = dp.copy()
            dp[:x0] = 0.0
            dp /= np.linalg.norm(dp)
            fd = _fd(orc, w, p, dp, 1e-4)
            an = S @ dp
            assert np.max(np.abs(an - fd)) <= 1e-4 * max(1.0, np.max(np.abs(fd))), (fam, b, np.max(np.abs(an - fd)))
        checked += 1
    assert checked >= 2


def test_reference_sees_active_rows():
    """the golden collision-avoidance optima have active circle rows, the first-step optima an active friction row (presolved a_0 bound)"""
    for fam, row in (("zamca_n30_nx5", "circle"), ("first_n10_nx5", "friction")):
        cfg = cfg_from_golden(GOLD[fam + "__cfg"])
        nlp = BicycleNLP(cfg)
        hits = 0
        for b in range(GOLD[fam + "__w"].shape[0]):
            lg, _ = sens_ref.ls_multipliers(cfg, GOLD[fam + "__w"][b], GOLD[fam + "__p"][b])
            hits += (np.min(lg[nlp.row_obst(0):]) < -1e-3) if row == "circle" else (lg[0] > 1e-3)
        assert hits >= 1, fam


def test_reference_lam_p_is_the_parameter_gradient_of_the_lagrangian():
    fam = "zamca_n30_nx5"
    cfg = cfg_from_golden(GOLD[fam + "__cfg"])
    w, p = GOLD[fam + "__w"][0], GOLD[fam + "__p"][0]
    lg, lx = sens_ref.ls_multipliers(cfg, w, p)
    a, b = sens_ref.lam_p(cfg, w, p, lg), sens_ref.lam_p_numeric(cfg, w, p, lg, lx)
    assert np.max(np.abs(a - b)) <= 1e-6 * max(1.0, np.max(np.abs(a)))


# ---- 2. the kernels' math on the CPU ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sensx():
    L = C.CDLL(harness_lib("sensx"))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L.sensx_solve.argtypes = [C.POINTER(abi.MpcProblemDesc), dp, dp, dp, dp, C.c_int32, C.c_int32, dp, dp, dp, ip, dp, dp, dp, C.c_int32, dp, dp,
                              dp, dp, ip]
    L.sensx_model.argtypes = [C.POINTER(abi.MpcProblemDesc), dp, dp, dp, dp, dp, dp]
    return L


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def run_sensx(L, cfg, x0, p, dps, seeds, literal=0):
    nlp = BicycleNLP(cfg)
    lbg, ubg, lbx, ubx = nlp.bounds()
    B, nw = x0.shape
    nd = dps.shape[1]
    x0, p = np.ascontiguousarray(x0, dtype=np.float64), np.ascontiguousarray(p, dtype=np.float64)
    out, st, ok = np.empty_like(x0), np.empty(B, np.int32), np.empty(B, np.int32)
    lg, lx, lp = np.empty((B, nlp.n_g)), np.empty((B, nw)), np.empty((B, nw))
    dw, gp = np.empty((B, nd, nw)), np.empty((B, nw))
    d = emu_desc(cfg)
    ip = C.POINTER(C.c_int32)
    assert L.sensx_solve(C.byref(d), _dp(lbx), _dp(ubx), _dp(lbg), _dp(ubg), literal, B, _dp(x0), _dp(p), _dp(out), st.ctypes.data_as(ip), _dp(lg),
                         _dp(lx), _dp(lp), nd, _dp(np.ascontiguousarray(dps)), _dp(dw), _dp(np.ascontiguousarray(seeds)), _dp(gp),
                         ok.ctypes.data_as(ip)) == 0
    return dict(x=out, status=st, lam_g=lg, lam_x=lx, lam_p=lp, dw=dw, grad_p=gp, ok=ok)


def seeds_for(cfg, B, rng, n_rand=2):
    """n_rand random directions (U_ref part included: its derivative is 0) and the nx unit seeds of xref_0"""
    nw = cfg.n_w
    x0 = cfg.nu * cfg.N
    dps = np.zeros((B, n_rand + cfg.nx, nw))
    dps[:, :n_rand] = rng.normal(size=(B, n_rand, nw))
    for i in range(cfg.nx):
        dps[:, n_rand + i, x0 + i] = 1.0
    return dps, rng.normal(size=(B, nw))


def check_against_reference(cfg, r, p, dps, tol):
    """dw of every strictly complementary converged row against sens_ref; returns (checked, weakly active)"""
    checked = weak_n = 0
    for b in np.flatnonzero(r["status"] == 1):
        S, weak = sens_ref.sensitivity_matrix(cfg, r["x"][b], p[b], r["lam_g"][b], r["lam_x"][b])
        if weak:
            weak_n += 1
            continue
        ref = np.einsum("ij,dj->di", S, dps[b])
        err = np.max(np.abs(r["dw"][b] - ref)) / max(1.0, np.max(np.abs(ref)))
        assert err <= tol, (b, err)
        checked += 1
    return checked, weak_n


def check_adjoint(r, dps, seeds):
    for b in np.flatnonzero(r["ok"] == 1):
        for d in range(dps.shape[1]):
            lhs, rhs = seeds[b] @ r["dw"][b, d], r["grad_p"][b] @ dps[b, d]
            assert abs(lhs - rhs) <= 1e-10 * max(1.0, np.abs(seeds[b]).sum() * np.max(np.abs(r["dw"][b, d]))), (b, d, lhs, rhs)


@pytest.mark.parametrize("literal", [0, 1])
@pytest.mark.parametrize("fam", ["zamlf_n10_nx5", "zamlf_n30_nx6", "usalf_n50_nx5"])
def test_harness_matches_reference(sensx, fam, literal):
    cfg, kw = FAMILIES[fam]
    x0, p = synthetic_batch(cfg, 6, **kw)
    rng = np.random.default_rng(1)
    dps, seeds = seeds_for(cfg, 6, rng)
    r = run_sensx(sensx, cfg, x0, p, dps, seeds, literal)
    assert np.all(r["status"] == 1) and np.all(r["ok"] == 1)
    # (literal = 1 keeps the friction row with its lower bound 0 on |a_0^2 + c|, whose barrier term stays in the KKT matrix of instances that
    #  end a few 1e-3 above it with a small multiplier: the derivative of the barrier problem, not of the active set, to ~1e-4)
    checked, weak = check_against_reference(cfg, r, p, dps, 1e-6 if literal == 0 else 2e-4)
    assert checked >= 4, (checked, weak)
    assert np.all(r["dw"][:, :, : cfg.nu * cfg.N] == r["dw"][:, :, : cfg.nu * cfg.N])
    check_adjoint(r, dps, seeds)
    assert np.all(r["grad_p"][:, : cfg.nu * cfg.N] == 0.0)              # U_ref enters nowhere


def test_harness_collision_avoidance(sensx):
    x0, p = ca_batch(CA_CFG, 4)
    rng = np.random.default_rng(2)
    dps, seeds = seeds_for(CA_CFG, 4, rng)
    r = run_sensx(sensx, CA_CFG, x0, p, dps, seeds)
    assert np.sum(r["status"] == 1) >= 3
    nlp = BicycleNLP(CA_CFG)
    assert np.min(r["lam_g"][r["status"] == 1][:, nlp.row_obst(0):]) < -1e-3          # active circle rows
    checked, weak = check_against_reference(CA_CFG, r, p, dps, 1e-5)
    assert checked >= 2, (checked, weak)
    check_adjoint(r, dps, seeds)
    assert np.all(np.isnan(r["dw"][r["status"] != 1])) and np.all(np.isnan(r["lam_p"][r["status"] != 1]))


@pytest.mark.parametrize("literal", [0, 1])
def test_harness_presolved_friction_bound(sensx, literal):
    """first MPC step: a_0 brakes at the friction cap.  literal = 0: the row is presolved into a bound of a_0 whose derivative with respect to
    xref_0 (delta_0, v_0) the right-hand side must carry; literal = 1: the row is kept.  Both must give the NLP's derivative."""
    cfg = cfg_from_golden(GOLD["first_n10_nx5__cfg"])
    x0, p = GOLD["first_n10_nx5__x0"], GOLD["first_n10_nx5__p"]
    rng = np.random.default_rng(3)
    dps, seeds = seeds_for(cfg, x0.shape[0], rng)
    r = run_sensx(sensx, cfg, x0, p, dps, seeds, literal)
    assert np.all(r["status"] == 1) and np.all(r["lam_g"][:, 0] > 0)
    checked, weak = check_against_reference(cfg, r, p, dps, 1e-6 if literal == 0 else 2e-4)
    assert checked == x0.shape[0], (checked, weak)
    check_adjoint(r, dps, seeds)
    # a_0 moves with delta_0 along the cap: a nonzero derivative that frozen bounds would miss
    assert np.all(np.abs(r["dw"][:, 2 + 2, 1]) > 1e-3)


def test_harness_lam_p_closed_form(sensx):
    cfg, kw = FAMILIES["zamlf_n30_nx6"]
    x0, p = synthetic_batch(cfg, 4, **kw)
    rng = np.random.default_rng(4)
    dps, seeds = seeds_for(cfg, 4, rng, 0)
    r = run_sensx(sensx, cfg, x0, p, dps, seeds)
    for b in range(4):
        ref = sens_ref.lam_p(cfg, r["x"][b], p[b], r["lam_g"][b])
        assert np.max(np.abs(r["lam_p"][b] - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref)))
        num = sens_ref.lam_p_numeric(cfg, r["x"][b], p[b], r["lam_g"][b], r["lam_x"][b])
        assert np.max(np.abs(r["lam_p"][b] - num)) <= 1e-6 * max(1.0, np.max(np.abs(ref)))


@pytest.mark.parametrize("nx", [5, 6])
def test_dynamics_derivatives_follow_the_model(sensx, nx):
    """sens_stage_A (A = I + dt df/dx) and sens_dyn_hess (dt sum_r lam_r Hess f_r) against central differences of ode_eval, the model
    function the solver evaluates its defects with: a change of the model that is not carried into them fails here"""
    cfg = FAMILIES["zamlf_n30_nx6" if nx == 6 else "zamlf_n10_nx5"][0]
    d = emu_desc(cfg)
    rng = np.random.default_rng(12)
    A_SLOTS = [(0, 3), (0, 4), (1, 3), (1, 4), (4, 2), (4, 3)]
    H_SLOTS = [(2, 2), (2, 3), (3, 4), (4, 4)]

    def model(x, u, lam):
        f, a, h = np.empty(nx), np.empty(6), np.empty(4)
        assert sensx.sensx_model(C.byref(d), _dp(np.ascontiguousarray(x)), _dp(np.ascontiguousarray(u)), _dp(np.ascontiguousarray(lam)),
                                 _dp(f), _dp(a), _dp(h)) == 0
        return f, a, h

    for _ in range(20):
        x = np.array([rng.normal(0, 30), rng.normal(0, 30), rng.uniform(-0.9, 0.9), rng.uniform(0.5, 30), rng.uniform(-3, 3)] + [rng.normal()] * (nx - 5))
        u, lam = rng.normal(size=2), rng.normal(size=nx)
        _, a, h = model(x, u, lam)
        eps = 1e-6
        J = np.zeros((nx, nx))
        for j in range(nx):
            e = np.zeros(nx)
            e[j] = eps
            J[:, j] = (model(x + e, u, lam)[0] - model(x - e, u, lam)[0]) / (2 * eps)
        A = np.eye(nx) + cfg.dt * J
        for q, (i, j) in enumerate(A_SLOTS):
            assert abs(a[q] - A[i, j]) <= 1e-7 * max(1.0, abs(A[i, j])), (i, j, a[q], A[i, j])
        off = [(i, j) for i in range(nx) for j in range(nx) if i != j and (i, j) not in A_SLOTS and not (nx == 6 and (i, j) == (5, 3))]
        assert all(abs(A[i, j]) <= 1e-8 for i, j in off)                       # structural zeros of A - I
        if nx == 6:
            assert abs(A[5, 3] - cfg.dt) <= 1e-9
        # dt * Hessian of lam' f, from differences of the (exact) Jacobian's rows (A) -- its own entries by second differences
        phi = lambda y: lam @ model(y, u, lam)[0]                               # noqa: E731
        eps2 = 1e-4
        Hn = np.zeros((nx, nx))
        for i in range(nx):
            for j in range(nx):
                ei, ej = np.zeros(nx), np.zeros(nx)
                ei[i], ej[j] = eps2, eps2
                Hn[i, j] = (phi(x + ei + ej) - phi(x + ei - ej) - phi(x - ei + ej) + phi(x - ei - ej)) / (4 * eps2 * eps2)
        Hn *= cfg.dt
        for q, (i, j) in enumerate(H_SLOTS):
            assert abs(h[q] - Hn[i, j]) <= 1e-4 * max(1.0, abs(Hn[i, j])), (i, j, h[q], Hn[i, j])
        listed = set(H_SLOTS) | {(j, i) for i, j in H_SLOTS}
        assert all(abs(Hn[i, j]) <= 1e-4 for i in range(nx) for j in range(nx) if (i, j) not in listed)
