"""CPU: the NLP evaluation and the multiplier mapping behind mpc_eval_nlp_batch / mpc_solve_batch_ex.

tests/nlpx/nlpx.cpp steps the kernels' own phase functions on the CPU (one launch per kernel: the iterate stays tile-major) and then
runs nlp_eval_stage / mult_stage, the functions k_eval_nlp / k_mult_out run on the GPU.  f, g are checked against the C oracle
(oracle/mpc_oracle.c: mpco_objective / mpco_constraints); the multipliers against the numpy NLP (KKT conditions, CasADi's signs)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import CA_CFG, FAMILIES, ROOT, BicycleNLP, abi, ca_batch, cfg_from_golden, emu_desc, harness_lib, synthetic_batch
from oracle.binding import OracleSolver as CORACLE
from test_gpu_multipliers import kkt_violations

NEW = ["mpc_eval_nlp_batch", "mpc_eval_nlp_batch_dev", "mpc_solve_batch_ex", "mpc_solve_batch_dev_ex"]
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


@pytest.fixture(scope="module")
def nlpx():
    L = C.CDLL(harness_lib("nlpx"))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L.nlpx_solve.argtypes = [C.POINTER(abi.MpcProblemDesc), dp, dp, dp, dp, C.c_int32, C.c_int32, dp, dp, dp, ip, dp, dp]
    L.nlpx_eval.argtypes = [C.POINTER(abi.MpcProblemDesc), C.c_int32, dp, dp, dp, dp, dp]
    return L


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def solve(L, cfg, x0, p, literal=0):
    nlp = BicycleNLP(cfg)
    lbg, ubg, lbx, ubx = nlp.bounds()
    B = x0.shape[0]
    x0, p = np.ascontiguousarray(x0, dtype=np.float64), np.ascontiguousarray(p, dtype=np.float64)
    out, st = np.empty_like(x0), np.empty(B, np.int32)
    lg, lx = np.empty((B, nlp.n_g)), np.empty((B, nlp.n_w))
    d = emu_desc(cfg)
    assert L.nlpx_solve(C.byref(d), _dp(lbx), _dp(ubx), _dp(lbg), _dp(ubg), literal, B, _dp(x0), _dp(p), _dp(out),
                        st.ctypes.data_as(C.POINTER(C.c_int32)), _dp(lg), _dp(lx)) == 0
    return out, st, lg, lx


def evaluate(L, cfg, x, p, obst=None):
    B = x.shape[0]
    nlp = BicycleNLP(cfg)
    f, g = np.empty(B), np.empty((B, nlp.n_g))
    d = emu_desc(cfg)
    assert L.nlpx_eval(C.byref(d), B, _dp(np.ascontiguousarray(x)), _dp(np.ascontiguousarray(p)), _dp(obst), _dp(f), _dp(g)) == 0
    return f, g


def check(cfg, x, p, lg, lx, st, literal=0):
    nlp = BicycleNLP(cfg)
    bounds = nlp.bounds()
    worst = np.zeros(4)
    assert np.all(np.isnan(lg[st != 1]))
    for b in np.flatnonzero(st == 1):
        worst = np.maximum(worst, kkt_violations(nlp, x[b], p[b], lg[b], lx[b], bounds))
    assert worst[0] <= 1e-7 and worst[1] <= 1e-9 and worst[2] <= 1e-5 and worst[3] == 0.0, worst
    return worst


@pytest.mark.parametrize("literal", [0, 1])
@pytest.mark.parametrize("fam", ["zamlf_n10_nx5", "zamlf_n30_nx6"])
def test_mapped_multipliers_are_kkt_multipliers(nlpx, fam, literal):
    cfg, kw = FAMILIES[fam]
    x0, p = synthetic_batch(cfg, 6, **kw)
    x, st, lg, lx = solve(nlpx, cfg, x0, p, literal)
    assert np.all(st == 1)
    check(cfg, x, p, lg, lx, st)


def test_collision_avoidance_multipliers(nlpx):
    x0, p = ca_batch(CA_CFG, 4)
    x, st, lg, lx = solve(nlpx, CA_CFG, x0, p)
    assert np.sum(st == 1) >= 3
    check(CA_CFG, x, p, lg, lx, st)
    o = lg[st == 1][:, 1 + CA_CFG.nx * (CA_CFG.N + 1):]
    assert np.min(o) < -1e-3                      # an obstacle row is active: its lower bound, negative multiplier


@pytest.mark.parametrize("literal", [0, 1])
def test_first_step_brakes_at_the_cap_with_a_positive_row_multiplier(nlpx, literal):
    cfg = cfg_from_golden(GOLD["first_n10_nx5__cfg"])
    x0, p = GOLD["first_n10_nx5__x0"], GOLD["first_n10_nx5__p"]
    x, st, lg, lx = solve(nlpx, cfg, x0, p, literal)
    assert np.all(st == 1) and np.allclose(x[:, 1], -np.sqrt(11.5), atol=1e-6)
    assert np.all(lg[:, 0] > 0) and np.all(np.abs(lx[:, 1]) < 1e-8)       # the row binds, not ubx of a_0
    check(cfg, x, p, lg, lx, st)


def test_presolved_and_literal_row_agree(nlpx):
    cfg = cfg_from_golden(GOLD["first_n10_nx5__cfg"])
    x0, p = GOLD["first_n10_nx5__x0"], GOLD["first_n10_nx5__p"]
    a, b = solve(nlpx, cfg, x0, p, 0), solve(nlpx, cfg, x0, p, 1)
    assert np.max(np.abs(a[2][:, 0] - b[2][:, 0])) <= 1e-6 * np.max(np.abs(a[2][:, 0]))


@pytest.mark.parametrize("fam", ["zamlf_n10_nx5", "zamlf_n30_nx6", "ca"])
def test_eval_matches_the_oracle(nlpx, fam):
    cfg, kw = (CA_CFG, {}) if fam == "ca" else FAMILIES[fam]
    x0, p = ca_batch(cfg, 8) if fam == "ca" else synthetic_batch(cfg, 8, **kw)
    rng = np.random.default_rng(11)
    pts = [x0 + rng.normal(0.0, 0.3, x0.shape), solve(nlpx, cfg, x0, p)[0]]      # random points and solutions
    orc = CORACLE(cfg)
    for x in pts:
        f, g = evaluate(nlpx, cfg, x, p)
        for b in range(x.shape[0]):
            fr, gr = orc.objective(x[b], p[b]), orc.constraints(x[b], p[b])
            assert abs(f[b] - fr) <= 1e-13 * abs(fr)
            assert np.max(np.abs(g[b] - gr) / np.maximum(1.0, np.abs(gr))) <= 1e-13 * max(1.0, np.max(np.abs(x[b])))


def test_eval_per_instance_obstacles(nlpx):
    cfg = CA_CFG
    x0, p = ca_batch(cfg, 8)
    rng = np.random.default_rng(3)
    obst = np.tile(np.asarray(cfg.obstacle_centers).ravel(), (8, 1)) + rng.normal(0.0, 1.0, (8, 6))
    f, g = evaluate(nlpx, cfg, x0, p, obst)
    for b in range(8):
        nlp = BicycleNLP(cfg)
        nlp.obst = obst[b].reshape(3, 2)
        gr = nlp.g(x0[b], p[b])
        assert np.max(np.abs(g[b] - gr) / np.maximum(1.0, np.abs(gr))) <= 1e-13 * max(1.0, np.max(np.abs(x0[b])))
