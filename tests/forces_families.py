"""Problem families of the FORCES-mode SQP step (row f3) for tests/test_forces_qp.py -- a plain module, no tests in it.

binding_family: eight kinds of instance, interleaved (instance b is of kind b % 8), built so that at the optimum of the QP every kind of
inequality row is active somewhere: both bounds of the steering rate, the acceleration, the steering angle and the speed, the friction
row and the linearised obstacle rows.  An interior-point iterate barely feels a row that stays far from active, so a wrong sign or column
in such a row's Jacobian is invisible to a family that never drives it to its bound.  active_rows says, from the dense oracle alone, which
rows an instance binds; tests/test_forces_qp.py asserts the counts."""
import numpy as np

from oracle import forces_model_numpy as FM
from oracle import forces_qp_numpy as Q

LB = np.array([-0.4, -11.5, -np.inf, -np.inf, -1.066, 0.0, -np.inf])           # optimizer.py:100-110
UB = np.array([0.4, 11.5, np.inf, np.inf, 1.066, 50.8, np.inf])
# the same with a steering-angle bound the lateral manoeuvres of kinds 1 and 6 reach (the cost pulls the angle to 0 with weight 50: no start
# that the model's own bound of 1.066 rad leaves feasible makes the QP hold it there)
LB_TIGHT = np.array([-0.4, -11.5, -np.inf, -np.inf, -0.02, 0.0, -np.inf])
UB_TIGHT = np.array([0.4, 11.5, np.inf, np.inf, 0.02, 50.8, np.inf])
HL = np.concatenate(([0.0], np.full(9, 3.3 ** 2)))
HU = np.concatenate(([11.5 ** 2], np.full(9, np.inf)))
PSI, X0, Y0 = 0.03495, 29.9948, -1.1501
N_KINDS = 8
BINDING_LABELS = ("lb0", "ub0", "lb1", "ub1", "lb4", "ub4", "lb5", "ub5", "hu0", "hl")
SEED = 7
K5_LAT, K5_A0, K5_DV = (10.6, 11.3), (1.5, 2.5), (2.0, 4.0)                    # kind 5: lateral acceleration, aLong of the guess, speed-up demand


def binding_family(B, N, seed=SEED):
    """zbar (B,N,7), params (B,N,10), xinit (B,5).  z = [deltaDot, aLong, x, y, delta, v, psi]; the guess is the start state repeated, the
    reference a straight path of 0.1 k max(vref, 0) metres along PSI, dt = 0.1.  Kinds (rows they bind at N = 10 with LB / UB):
      0  speed demand far from the speed: aLong at +-11.5 (ub1 / lb1)
      1  lateral offset of 1.5 .. 3 m: the steering rate at both bounds (lb0, ub0); with LB_TIGHT / UB_TIGHT the steering angle (lb4, ub4)
      2  slow, three obstacle circles beside and ahead, the path bent towards them: obstacle rows (hl), lb0, ub0; some end -7 or 0
      3  nearly at rest, asked to reverse: v >= 0 (lb5)
      4  at 50 .. 50.6 m/s, asked for 60: v <= 50.8 (ub5)
      5  cornering at 10.6 .. 11.3 m/s^2 of lateral acceleration and accelerating in the guess (the friction row's aLong column is 2 aLong:
         zero at a guess that coasts), asked to speed up: the friction row (hu0) at the stages past the first, lb0 / ub0
      6  heading off by 0.15 .. 0.3 rad: lb0 / ub0; with the tight pair the steering angle
      7  plain lane following: none (control)"""
    rng = np.random.default_rng(seed)
    cs, sn = np.cos(PSI), np.sin(PSI)
    zbar, params, xinit = np.zeros((B, N, 7)), np.zeros((B, N, 10)), np.zeros((B, 5))
    k = np.arange(1, N + 1)
    for b in range(B):
        kind = b % N_KINDS
        sgn = 1.0 if rng.uniform() < 0.5 else -1.0
        lat, delta, psi, v, a0 = rng.uniform(-0.2, 0.2), 0.0, PSI, rng.uniform(16.0, 19.6), 0.0
        vref, bend = v, 0.0
        ob = np.array([-100.0, 0.0, -100.0, 0.0, -100.0, 0.0])
        if kind == 0:
            vref = v + sgn * rng.uniform(8.0, 15.0)
        elif kind == 1:
            lat = sgn * rng.uniform(1.5, 3.0)
        elif kind == 2:
            v = vref = rng.uniform(3.0, 6.0)
            side, ahead = sgn * rng.uniform(3.4, 3.9), rng.uniform(0.5, 2.5)
            for j, along in enumerate((ahead, ahead + 1.0, ahead - 1.0)):
                ob[2 * j] = X0 + along * cs - side * sn
                ob[2 * j + 1] = Y0 + along * sn + side * cs
            bend = 0.5 * sgn
        elif kind == 3:
            v, vref = rng.uniform(0.2, 1.0), -5.0
        elif kind == 4:
            v, vref = rng.uniform(50.0, 50.6), 60.0
        elif kind == 5:
            v = rng.uniform(9.0, 11.0)
            delta = sgn * np.arctan(rng.uniform(*K5_LAT) * FM.WHEELBASE_FRICTION / v ** 2)
            a0 = rng.uniform(*K5_A0)
            vref = v + rng.uniform(*K5_DV)
        elif kind == 6:
            psi = PSI + sgn * rng.uniform(0.15, 0.3)
        zi = np.array([0.0, a0, X0 - lat * sn, Y0 + lat * cs, delta, v, psi])
        zbar[b] = np.tile(zi, (N, 1))
        xinit[b] = zi[2:]
        step = 0.1 * k * max(vref, 0.0)
        path = np.stack([X0 + step * cs - bend * sn, Y0 + step * sn + bend * cs], 1)
        params[b] = np.hstack([path, np.full((N, 1), vref), np.full((N, 1), PSI), np.tile(ob, (N, 1))])
    return zbar, params, xinit


def row_labels(N, lb, ub, hl, hu):
    """labels of the rows of Q.build_qp, stage by stage, in its order: lb0..lb6, ub0..ub6, hu0, hl"""
    out = []
    for k in range(N):
        lab = []
        for i in range(7):
            if k == 0 and i >= 2:
                continue
            if np.isfinite(lb[i]):
                lab.append(f"lb{i}")
            if np.isfinite(ub[i]):
                lab.append(f"ub{i}")
        for j in range(10):
            if np.isfinite(hu[j]):
                lab.append(f"hu{j}")
            if j > 0 and np.isfinite(hl[j]):
                lab.append("hl")
        out.append(lab)
    return out


def active_rows(zbar_b, params_b, xinit_b, lb, ub, hl, hu, mode=0, with_conv=False):
    """labels of the inequality rows whose slack d - G dz is below 1e-3 at the dense oracle's solution of the instance's QP"""
    N = zbar_b.shape[0]
    st = Q.build_qp(zbar_b, params_b, xinit_b, lb, ub, hl, hu)
    dz, it, conv, kkt = Q.solve_qp(st, zbar_b, xinit_b, Q.hessian_diag(FM.WEIGHTS_MODEL_C, N, mode))
    labels = set()
    for k, lab in enumerate(row_labels(N, lb, ub, hl, hu)):
        assert len(lab) == st[k]["G"].shape[0]
        slack = st[k]["d"] - st[k]["G"] @ dz[k]
        labels.update(l for l, s in zip(lab, slack) if s < 1e-3)
    return (labels, conv) if with_conv else labels
