"""numpy reference of the parametric sensitivities of the NLP's optimum (mpc_solve_batch_sens, mpc_sens_adjoint).

At a KKT point (w, lam_g, lam_x) in CasADi's convention (grad f + J_g' lam_g + lam_x = 0) the active-set derivative of the optimum with
respect to the parameter row p = [U_ref | X_ref] solves the reduced KKT system

    [ H    J_A' ] [ dw ]   [ -d(grad_w L)/dp dp ]        H = Hessian of the Lagrangian (oracle/nlp_numpy.py: hess_lag)
    [ J_A  0    ] [ dnu] = [ -d g_A / dp dp     ]        J_A = rows of the equality constraints, of the active rows, of the active bounds

grad_w L depends on p only through the cost, 2 Q (x_k - xref_{k+1}) (linear in p); of the rows only the pin x_0 - xref_0 depends on p.
The three copies of a circle distance are one row here (their multipliers summed); a row or bound is active where it is at its bound
(gap <= GAP) with a nonzero multiplier (|lam| > ACTIVE).  An instance is "weakly active" -- not strictly complementary to the solve's tolerance -- where some row or bound is near its
bound (gap <= WEAK_GAP) with a multiplier below STRICT: the barrier terms z / gap of the final iterate (mu ~ tol) then neither make it an
equality nor make it vanish, and the solver's derivative and the active-set derivative legitimately differ by more than the tolerance.
"""
import numpy as np

from oracle.nlp_numpy import BicycleNLP

ACTIVE = 1e-6
STRICT = 1e-2
GAP = 1e-4
WEAK_GAP = 1e-3


def _rows(nlp):
    """distinct rows of g: the friction row, pin + defects (equalities), the first copy of every circle distance"""
    N, nx = nlp.N, nlp.nx
    eq = list(range(1, 1 + nx * (N + 1)))
    circ = [nlp.row_obst(k) + 3 * j for k in range(N + 1) for j in range(3)]
    return eq, circ


def _circle_mult(lam_g, r):
    return lam_g[r] + lam_g[r + 1] + lam_g[r + 2]


def active_sets(nlp, w, p, lam_g, lam_x, bounds):
    """(rows, bound variables) of the active set, and whether some inequality is weakly active"""
    lbg, ubg, lbx, ubx = bounds
    g = nlp.g(w, p)
    eq, circ = _rows(nlp)
    rows, weak = list(eq), False
    for r in [0] + circ:
        m = lam_g[0] if r == 0 else _circle_mult(lam_g, r)
        gap = min(g[r] - lbg[r], ubg[r] - g[r])
        sc = max(1.0, abs(g[r]))
        if gap <= GAP * sc and abs(m) > ACTIVE:
            rows.append(r)
        if gap <= WEAK_GAP * sc and abs(m) <= STRICT:
            weak = True
    bnd = []
    for i in range(nlp.n_w):
        gap = min(w[i] - lbx[i], ubx[i] - w[i])
        sc = max(1.0, abs(w[i]))
        if gap <= GAP * sc and abs(lam_x[i]) > ACTIVE:
            bnd.append(i)
        if gap <= WEAK_GAP * sc and abs(lam_x[i]) <= STRICT:
            weak = True
    return rows, bnd, weak


def kkt_matrix(cfg, w, p, lam_g, lam_x, bounds=None):
    """the reduced KKT matrix K, the parameter block G (K [dw; dnu] = G dp) and the weak-activity flag"""
    nlp = BicycleNLP(cfg)
    bounds = nlp.bounds() if bounds is None else bounds
    rows, bnd, weak = active_sets(nlp, w, p, lam_g, lam_x, bounds)
    H = nlp.hess_lag(w, p, 1.0, lam_g)
    J = nlp.jac(w, p)
    JA = np.vstack([J[rows], np.eye(nlp.n_w)[bnd]]) if bnd else J[rows]
    n, m = nlp.n_w, JA.shape[0]
    K = np.zeros((n + m, n + m))
    K[:n, :n] = H
    K[:n, n:] = JA.T
    K[n:, :n] = JA
    # G = -d(residual)/dp: stationarity rows of x_k get 2 Q dxref_{k+1}; the pin rows get dxref_0
    G = np.zeros((n + m, n))
    Q = cfg.Qdiag
    for k in range(cfg.N):
        for i in range(cfg.nx):
            G[nlp.ix(k) + i, nlp.ix(k + 1) + i] = 2.0 * Q[i]
    for i in range(cfg.nx):
        G[n + rows.index(1 + i), nlp.ix(0) + i] = 1.0
    return K, G, weak


def sensitivity_matrix(cfg, w, p, lam_g, lam_x, bounds=None):
    """dw/dp [n_w, n_p] of the optimum, and the weak-activity flag"""
    K, G, weak = kkt_matrix(cfg, w, p, lam_g, lam_x, bounds)
    S = np.linalg.solve(K, G)
    return S[:cfg.n_w], weak


def lam_p(cfg, w, p, lam_g):
    """CasADi's lam_p = d/dp [f + lam_g' g + lam_x' x] at w: X_ref column 0 -lam_g[pin rows], column k+1 -2 Q (x_k - xref_{k+1})"""
    nlp = BicycleNLP(cfg)
    out = np.zeros(cfg.n_w)
    Q = cfg.Qdiag
    out[nlp.ix(0): nlp.ix(0) + cfg.nx] = -lam_g[1: 1 + cfg.nx]
    for k in range(cfg.N):
        out[nlp.ix(k + 1): nlp.ix(k + 1) + cfg.nx] = -2.0 * Q * (w[nlp.ix(k): nlp.ix(k) + cfg.nx] - p[nlp.ix(k + 1): nlp.ix(k + 1) + cfg.nx])
    return out


def lam_p_numeric(cfg, w, p, lam_g, lam_x, h=1e-6):
    """d/dp [f + lam_g' g + lam_x' x] by central differences of the numpy NLP (w, lam fixed)"""
    nlp = BicycleNLP(cfg)

    def L(pp):
        return nlp.f(w, pp) + lam_g @ nlp.g(w, pp) + lam_x @ w

    out = np.zeros(cfg.n_w)
    for q in range(cfg.nu * cfg.N, cfg.n_w):
        e = np.zeros(cfg.n_w)
        e[q] = h
        out[q] = (L(p + e) - L(p - e)) / (2 * h)
    return out


def ls_multipliers(cfg, w, p, gap=1e-6):
    """multipliers of a primal optimum w (e.g. a golden one) by least squares on the rows and bounds that are at their bound (gap)"""
    nlp = BicycleNLP(cfg)
    lbg, ubg, lbx, ubx = nlp.bounds()
    g = nlp.g(w, p)
    eq, circ = _rows(nlp)
    rows = list(eq) + [r for r in [0] + circ if min(g[r] - lbg[r], ubg[r] - g[r]) <= gap * max(1.0, abs(g[r]))]
    bnd = [i for i in range(nlp.n_w) if min(w[i] - lbx[i], ubx[i] - w[i]) <= gap * max(1.0, abs(w[i]))]
    J = nlp.jac(w, p)
    JA = np.vstack([J[rows], np.eye(nlp.n_w)[bnd]]) if bnd else J[rows]
    nu = np.linalg.lstsq(JA.T, -nlp.grad(w, p), rcond=None)[0]
    lam_g, lam_x = np.zeros(nlp.n_g), np.zeros(nlp.n_w)
    for q, r in enumerate(rows):
        if r in circ:
            lam_g[r: r + 3] = nu[q] / 3.0
        else:
            lam_g[r] = nu[q]
    for q, i in enumerate(bnd):
        lam_x[i] = nu[len(rows) + q]
    return lam_g, lam_x


# ---- away from the default descriptor (tests/descriptor_families.py: D5, D6) -----------------------------------------------------------------
# This reference against the CPU harness (tests/sensx) at the point, worst max|dw - ref| / max(1, max|ref|) over the rows the GPU test compares,
# measured by tests/test_descriptor_cpu.py::test_sensitivity_harness_against_the_reference (reference against harness, no kernel involved).
# D5 "outlier" is instance 12 alone, where the final iterate's barrier term on a nearly active presolved friction bound is what the active-set
# derivative does not carry (tests/test_sensitivities_cpu.py allows a kept friction row 2e-4); "rest" is every other row.  Bounds: ten times the
# figure, capped by the family's own bounds -- 1e-5 where no row is weakly held (TOL_DW of tests/test_gpu_sensitivities.py), 1e-4 for the
# outlier and for collision avoidance (what that module grants its collision-avoidance batch).
DESC_HARNESS_WORST = {"D5": dict(rest=4.9e-7, outlier=2.54e-5), "D6": dict(rest=2.62e-6)}
DESC_TOL = {"D5": dict(rest=min(10 * 4.9e-7, 1e-5), outlier=min(10 * 2.54e-5, 1e-4)), "D6": dict(rest=min(10 * 2.62e-6, 1e-4))}
