"""numpy reference of the derivative of the NLP's optimum with respect to its bounds and the circle radius (mpc_sens_bounds; DESIGN.md
section 13).

The bound vector is bv = [lbx (n_w) | ubx (n_w) | fl, fu, ol, ou]: the arrays of mpc_set_bounds, lbg[0] / ubg[0] of the friction row and the
pair shared by the 9 (N + 1) circle rows (ol is the radius sum); n_b = 2 n_w + 4.  The equality rows have no entry.

The reduced KKT system of tests/sens_ref.py, K [dw; dnu] = G dbv, with another right-hand side.  A bound enters the active set's rows only:
an active row reads g_r(w) = its bound and an active bound w_i = its bound, so G is 1 in the row of each active bound, circle row or friction
row, at the bv entry of the side it sits on, and 0 elsewhere (the stationarity rows hold no bound).  An inactive bound has derivative 0.
"""
import numpy as np

from oracle.nlp_numpy import BicycleNLP
import sens_ref

N_ROWS = 4                      # fl, fu, ol, ou behind lbx | ubx
FL, FU, OL, OU = range(4)
LEVELS = ("deltav_min", "deltav_max", "a_ub", "delta_min", "delta_max", "v_min", "v_max", "fu", "ol")
# The bound of max|dw - want| / max(max|want|, 0.1) for the kernel's math against this reference (tests/test_sens_bounds_cpu.py, and the GPU
# tests after it).  What remains between the two is the barrier's z / gap of the final iterate against the active set, which varies from row to
# row: ten times the worst value the CPU harness measured over its two batches (printed by its tests), and never looser than the 1e-4 that
# tests/test_gpu_sensitivities.py grants the p directions of the same collision-avoidance batch.
# collision avoidance (N = 30, nx = 5): deltav_min on row 4, whose steering rate passes 3e-3 from its bound at one stage; lane following N = 10,
# nx = 6: 8.0e-7; on the GPU 5.87e-5 (the same row and direction) and 8.0e-7
HARNESS_WORST = 4.42e-5
TOL_DW = min(10 * HARNESS_WORST, 1e-4)


def n_b(cfg):
    return 2 * cfg.n_w + N_ROWS


def bounds_vector(cfg, bounds=None):
    """bv of a configuration's bounds (lbg, ubg, lbx, ubx: the order of BicycleNLP.bounds)"""
    lbg, ubg, lbx, ubx = BicycleNLP(cfg).bounds() if bounds is None else bounds
    return np.concatenate([lbx, ubx, [lbg[0], ubg[0], lbg[-1], ubg[-1]]])


def unpack_bounds(cfg, bv):
    """(lbg, ubg, lbx, ubx) of a bound vector, the equality rows 0"""
    nw, ne = cfg.n_w, cfg.nx * (cfg.N + 1)
    bv = np.asarray(bv, dtype=np.float64)
    lbg = np.concatenate([[bv[2 * nw + FL]], np.zeros(ne), np.full(9 * (cfg.N + 1), bv[2 * nw + OL])])
    ubg = np.concatenate([[bv[2 * nw + FU]], np.zeros(ne), np.full(9 * (cfg.N + 1), bv[2 * nw + OU])])
    return lbg, ubg, bv[:nw].copy(), bv[nw: 2 * nw].copy()


def level_directions(cfg):
    """the nine unit level directions [9, n_b] in the order of LEVELS: a limit of the vehicle moved at every stage at once"""
    nlp = BicycleNLP(cfg)
    nw = cfg.n_w
    d = np.zeros((len(LEVELS), n_b(cfg)))
    for k in range(cfg.N):
        d[0, nlp.iu(k)] = 1.0
        d[1, nw + nlp.iu(k)] = 1.0
        d[2, nw + nlp.iu(k) + 1] = 1.0
    for k in range(cfg.N + 1):
        d[3, nlp.ix(k) + 2] = 1.0
        d[4, nw + nlp.ix(k) + 2] = 1.0
        d[5, nlp.ix(k) + 3] = 1.0
        d[6, nw + nlp.ix(k) + 3] = 1.0
    d[7, 2 * nw + FU] = 1.0
    d[8, 2 * nw + OL] = 1.0
    return d


def kkt_matrix(cfg, w, p, lam_g, lam_x, bounds=None):
    """the reduced KKT matrix K of sens_ref, the bounds block G [n + m, n_b] (K [dw; dnu] = G dbv) and the weak-activity flag"""
    nlp = BicycleNLP(cfg)
    bounds = nlp.bounds() if bounds is None else bounds
    lbg, ubg, lbx, ubx = bounds
    K, _, weak = sens_ref.kkt_matrix(cfg, w, p, lam_g, lam_x, bounds)
    rows, bnd, _ = sens_ref.active_sets(nlp, w, p, lam_g, lam_x, bounds)
    n, nw = cfg.n_w, cfg.n_w
    g = nlp.g(w, p)
    G = np.zeros((K.shape[0], n_b(cfg)))
    first_obst = nlp.row_obst(0)
    for q, r in enumerate(rows):
        if lbg[r] == ubg[r]:
            continue
        lower = g[r] - lbg[r] <= ubg[r] - g[r]
        if r == 0:
            G[n + q, 2 * nw + (FL if lower else FU)] = 1.0
        else:
            assert r >= first_obst
            G[n + q, 2 * nw + (OL if lower else OU)] = 1.0
    for q, i in enumerate(bnd):
        lower = w[i] - lbx[i] <= ubx[i] - w[i]
        G[n + len(rows) + q, i if lower else nw + i] = 1.0
    return K, G, weak


def sensitivity_matrix(cfg, w, p, lam_g, lam_x, bounds=None):
    """dw/dbv [n_w, n_b] of the optimum and the weak-activity flag"""
    K, G, weak = kkt_matrix(cfg, w, p, lam_g, lam_x, bounds)
    return np.linalg.solve(K, G)[:cfg.n_w], weak


def lam_bounds(cfg, lam_g, lam_x):
    """d f* / d bv [n_b] by the envelope theorem, from the multipliers in CasADi's convention: -lam_x[i] on the side the multiplier's sign
    names (lam_x < 0: the lower bound holds the variable), -lam_g likewise for the friction row and, summed, for the circle rows"""
    nw = cfg.n_w
    out = np.zeros(n_b(cfg))
    out[:nw] = -np.minimum(lam_x, 0.0)
    out[nw: 2 * nw] = -np.maximum(lam_x, 0.0)
    out[2 * nw + FL] = -min(lam_g[0], 0.0)
    out[2 * nw + FU] = -max(lam_g[0], 0.0)
    lo = lam_g[1 + cfg.nx * (cfg.N + 1):]
    out[2 * nw + OL] = -np.minimum(lo, 0.0).sum()
    out[2 * nw + OU] = -np.maximum(lo, 0.0).sum()
    return out


# ---- away from the default descriptor (tests/descriptor_families.py: D5, D6) -----------------------------------------------------------------
# This reference against the CPU harness (tests/sensx: sensboundx_solve) at the point, worst max|dw - want| / max(max|want|, 0.1) over the rows the
# GPU test compares and the ten directions of tests/test_sens_bounds_cpu.py, measured by
# tests/test_descriptor_cpu.py::test_sensitivity_harness_against_the_reference.  D5 "outlier" is instance 12 alone (see tests/sens_ref.py), "rest"
# every other row (instance 16: 8.5e-6, the others 3e-7 and below).  Bounds: min(10 x the figure, the 1e-4 of TOL_DW above).
DESC_HARNESS_WORST = {"D5": dict(rest=8.6e-6, outlier=2.1e-5), "D6": dict(rest=4.11e-6)}
DESC_TOL = {k: {q: min(10 * v, 1e-4) for q, v in d.items()} for k, d in DESC_HARNESS_WORST.items()}
