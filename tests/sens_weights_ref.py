"""numpy reference of the derivative of the NLP's optimum with respect to the seven cost weights wt = [Q_0 .. Q_4 | R_0, R_1]
(mpc_sens_weights).

The reduced KKT system of tests/sens_ref.py, K [dw; dnu] = G dwt, with another right-hand side: G = -d(KKT residual)/dwt.  The weights enter
the residual through the cost gradient only -- 2 Q_i e_k[i] on the stationarity row of x_k[i], e_k = x_k - xref_{k+1}, and 2 R_j u_k[j] on
that of u_k[j], k < N -- so

    G[ix(k) + i, i]     = -2 e_k[i]      (i < 5, k < N)
    G[iu(k) + j, 5 + j] = -2 u_k[j]      (k < N)

and the rows of the active set are 0.  Q_5 (the progress state of nx = 6) is no weight of the vector.

with_weights gives a configuration other weights, for everything that reads them (BicycleNLP, the C oracle's descriptor).
"""
import dataclasses

import numpy as np

from oracle.nlp_numpy import BicycleNLP
import sens_ref

N_WT = 7
# The bound of max|dw - want| / max|want| for the kernel's math against this reference (tests/test_sens_weights_cpu.py, and the GPU tests after
# it).  What remains between the two is the barrier's z / gap of the final iterate against the active set, which varies from row to row: ten
# times the worst value the CPU harness measured over its two batches (printed by its tests), and never looser than the 1e-4 that
# tests/test_gpu_sensitivities.py grants the p directions of the same collision-avoidance batch.
HARNESS_WORST = 2.25e-5          # collision avoidance (N = 30, nx = 5); lane following N = 10, nx = 6: 5.2e-7; on the GPU 2.99e-5 and 5.2e-7
TOL_DW = min(10 * HARNESS_WORST, 1e-4)


def weights_of(cfg):
    """the seven weights of a configuration"""
    return np.concatenate([np.asarray(cfg.Q, dtype=np.float64)[:5], np.asarray(cfg.R, dtype=np.float64)])


def with_weights(cfg, wt):
    """cfg with the seven weights given; everything else is cfg's"""
    wt = np.asarray(wt, dtype=np.float64).reshape(N_WT)
    return dataclasses.replace(cfg, Q=tuple(float(v) for v in wt[:5]), R=tuple(float(v) for v in wt[5:]))


def kkt_matrix(cfg, w, p, lam_g, lam_x, bounds=None):
    """the reduced KKT matrix K of sens_ref, the weights block G [n + m, 7] (K [dw; dnu] = G dwt) and the weak-activity flag"""
    nlp = BicycleNLP(cfg)
    K, _, weak = sens_ref.kkt_matrix(cfg, w, p, lam_g, lam_x, bounds)
    U, X = nlp.split(w)
    _, Xr = nlp.split(p)
    G = np.zeros((K.shape[0], N_WT))
    for k in range(cfg.N):
        e = X[k] - Xr[k + 1]
        for i in range(5):
            G[nlp.ix(k) + i, i] = -2.0 * e[i]
        for j in range(2):
            G[nlp.iu(k) + j, 5 + j] = -2.0 * U[k, j]
    return K, G, weak


def sensitivity_matrix(cfg, w, p, lam_g, lam_x, bounds=None):
    """dw/dwt [n_w, 7] of the optimum and the weak-activity flag"""
    K, G, weak = kkt_matrix(cfg, w, p, lam_g, lam_x, bounds)
    return np.linalg.solve(K, G)[:cfg.n_w], weak


def lam_weights(cfg, w, p):
    """d/dwt [f + lam_g' g] at w in closed form, [sum_{k<N} e_k[i]^2 | sum_{k<N} u_k[j]^2]: no constraint row holds a weight.  By the
    envelope theorem the derivative of the optimal objective."""
    nlp = BicycleNLP(cfg)
    U, X = nlp.split(w)
    _, Xr = nlp.split(p)
    out = np.zeros(N_WT)
    for k in range(cfg.N):
        e = X[k] - Xr[k + 1]
        out[:5] += e[:5] * e[:5]
        out[5:] += U[k] * U[k]
    return out


# ---- away from the default descriptor (tests/descriptor_families.py: D5, D6) -----------------------------------------------------------------
# This reference against the CPU harness (tests/sensx: sensweightx_solve) at the point, worst max|dw - want| / max|want| over the rows the GPU test
# compares and the eight directions, measured by tests/test_descriptor_cpu.py::test_sensitivity_harness_against_the_reference.  D5 "outlier" is
# instance 12 alone (see tests/sens_ref.py), "rest" every other row.  Bounds: min(10 x the figure, the 1e-4 of TOL_DW above).
DESC_HARNESS_WORST = {"D5": dict(rest=8.1e-7, outlier=1.73e-5), "D6": dict(rest=3.55e-6)}
DESC_TOL = {k: {q: min(10 * v, 1e-4) for q, v in d.items()} for k, d in DESC_HARNESS_WORST.items()}
