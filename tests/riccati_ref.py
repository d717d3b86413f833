"""Extended-precision reference of the Riccati factor / solve of one instance (TEST INFRASTRUCTURE, numpy only).

A textbook recursion on DENSE stage matrices -- it knows nothing of the kernels' sparse update, their storage or their rounding:

    cost      sum_k  1/2 x_k' Q_k x_k + 1/2 u_k' R_k u_k + u_k' S_k x_k + gx_k' x_k + gu_k' u_k      (Q_N, gx_N at the terminal stage)
    dynamics  x_0 = -c0,   x_{k+1} = A_k x_k + B_k u_k - cn_k
    backward  P_N = Q_N, p_N = gx_N;   Lam = R + B'P+B,  G = S + B'P+A,  K = -Lam^-1 G,  kff = -Lam^-1 (gu + B'(p+ - P+ cn))
              P_k = Q + A'P+A + G'K,   p_k = gx + A'(p+ - P+ cn) + G'kff
    forward   du_k = K dx_k + kff,  dx_{k+1} = A dx_k + B du_k - cn,   lam_k = P_k dx_k + p_k

with Q_k = H_k + delta I, R_k = diag(ruu_k) + delta I (delta: the inertia correction, schedule of riccati_instance in csrc/mpc_stage_math.h),
A = I + dt F from the six entries a[6] (+ the progress row of nx = 6), B = dt [e_delta e_v] and, at stage 0 only, the cross term S between
the second input and the states 2, 3 (hux).  `dtype` chooses the arithmetic: np.longdouble (the reference), np.float64 (the "plain twin":
what an unremarkable float64 implementation loses on the same data -- the yardstick of the tests' tolerances) or "mp" (mpmath numbers
in object arrays, at whatever mpmath.mp.dps the caller has set).
"""
import collections

import numpy as np

assert np.finfo(np.longdouble).eps < 2e-19, "the reference needs an extended-precision long double"

DW_MIN, DW_0, DW_MAX = 1e-20, 1e-4, 1e40
KW_MINUS, KW_PLUS, KW_PLUS_BAR = 1.0 / 3.0, 8.0, 100.0
DT = 0.1
NX_PAD = 6
FAMILIES = ("benign", "barrier", "rankone", "indefinite", "decoupled")
NS_ALL = (1, 2, 3, 30)
BORDER = 1e-6                 # a draw whose det(Lam) or L00 comes this close (relative) to zero at any tried delta is rejected
MEASURES = ("P", "p", "K", "dz")


class Case:
    """One instance: N, nx, dt, H[N+1, nx, nx] (symmetric), ruu[N+1, 2], a[N+1, 6], gx[N+1, nx], gu[N+1, 2], cn[N+1, nx], c0[nx], hux[2],
    delta_last, sym (the caller's mark: keep the cost-to-go symmetric / compensate the 2x2 solve), family, name."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


# ------------------------------------------------------------------------------------------------------------------- generator
def _draw(rng, family, nx, N, idx):
    r = lambda *s: rng.uniform(-1.0, 1.0, size=s)
    S = N + 1
    H = np.zeros((S, nx, nx))
    for k in range(S):
        for i in range(min(nx, 5)):
            H[k, i, i] = 2.0 + 300.0 * abs(r())
        for (i, j, w) in ((0, 1, 3.0), (0, 4, 2.0), (1, 4, 2.0), (2, 3, 1.0), (3, 4, 1.0)):
            H[k, i, j] = H[k, j, i] = w * r()
    ruu = np.stack([2.0 + 100.0 * np.abs(r(S)), 1.0 + np.abs(r(S))], axis=1)
    c = Case(N=N, nx=nx, dt=DT, H=H, ruu=ruu, a=0.3 * r(S, 6), gx=5.0 * r(S, nx), gu=r(S, 2), cn=0.05 * r(S, nx), c0=0.1 * r(nx),
             hux=(0.3 * r(2) if idx % 2 else np.zeros(2)), delta_last=0.0, sym=False, family=family, name=f"{family}-nx{nx}-N{N}-{idx}")
    if family == "barrier":                         # late-iteration Sigma = z / s on the input bounds and the (delta, v) bounds
        on = rng.uniform(size=S) < 0.4
        on[rng.integers(S)] = True
        for k in np.nonzero(on)[0]:
            c.ruu[k] += 10.0 ** rng.uniform(4, 11, size=2)
            c.H[k, 2, 2] += 10.0 ** rng.uniform(4, 11)
            c.H[k, 3, 3] += 10.0 ** rng.uniform(4, 11)
    if family == "rankone":                         # active circle rows: w g g' on (x, y, psi)
        on = rng.uniform(size=S) < 0.5
        on[1 + rng.integers(N)] = True
        for k in np.nonzero(on)[0]:
            g = np.zeros(nx)
            g[[0, 1, 4]] = r(3)
            c.H[k] += 10.0 ** rng.uniform(6, 10) * np.outer(g, g)
        c.sym = True
    if family in ("barrier", "rankone") and nx == 6 and idx % 4 >= 2:
        c.H[:, 5, 5] = 2.0 + 300.0 * np.abs(r(S))   # a weighted progress state: column 5 of the cost-to-go is not zero
    if family == "indefinite":                      # negative curvature on y, v or psi at one or two stages that a Lam sees (k >= 1)
        for k in rng.choice(np.arange(1, S), size=min(N, 1 + idx % 2), replace=False):
            i = (1, 3, 3, 4)[rng.integers(4)]
            c.H[k, i, i] -= 10.0 ** rng.uniform(3, 4.5)
        c.delta_last = (0.0, 1e-4, 3e-2)[idx % 3]
    if family == "decoupled":
        assert nx == 6
        c.gx[:, 5] = 0.0                             # (H[5, 5] is zero already)
    return c


def generate(family, nx, N, count, seed=0):
    """`count` accepted cases of a family, and the number of draws it took (borderline draws are rejected: see BORDER)."""
    rng = np.random.default_rng([seed, FAMILIES.index(family), nx, N])
    out, draws = [], 0
    while len(out) < count:
        c = _draw(rng, family, nx, N, len(out))
        draws += 1
        c.ref = solve(c, np.longdouble)
        if c.ref["margin"] >= BORDER:
            out.append(c)
    return out, draws


def with_sym(c, sym):
    """the same data with another mark (the reference does not depend on it)"""
    d = Case(**c.__dict__)
    d.sym = sym
    d.name = c.name + ("-sym" if sym else "-nosym")
    return d


# ------------------------------------------------------------------------------------------------------------------- dense stage data
def _conv(x, dtype):
    x = np.asarray(x, dtype=np.float64)
    if dtype == "mp":
        import mpmath
        return np.vectorize(lambda v: mpmath.mpf(float(v)), otypes=[object])(x) if x.ndim else mpmath.mpf(float(x))
    return x.astype(dtype) if x.ndim else dtype(x)


def dense_stage(c, k, dtype, delta=0.0):
    """(A, B, Q, R, S, gx, gu, b) of stage k, b = -cn: x+ = A x + B u + b"""
    nx = c.nx
    A = np.eye(nx)
    a = c.a[k]
    A[0, 3], A[0, 4], A[1, 3], A[1, 4], A[4, 2], A[4, 3] = a
    if nx == 6:
        A[5, 3] = c.dt
    B = np.zeros((nx, 2))
    B[2, 0] = B[3, 1] = c.dt
    S = np.zeros((2, nx))
    if k == 0:
        S[1, 2], S[1, 3] = c.hux
    Q = c.H[k] + delta * np.eye(nx)
    R = np.diag(c.ruu[k]) + delta * np.eye(2)
    return tuple(_conv(v, dtype) for v in (A, B, Q, R, S, c.gx[k], c.gu[k], -c.cn[k]))


# ------------------------------------------------------------------------------------------------------------------- recursion
def sweep(c, delta, dtype):
    """Backward and forward recursion at one delta.  ok: every Lam positive definite (judged in `dtype`); margin: the smallest relative
    distance of a det(Lam) or an L00 from zero among the stages up to the verdict.  Arrays are float64-convertible object / dtype arrays."""
    N, nx = c.N, c.nx
    od = object if dtype == "mp" else dtype
    P = np.zeros((N + 1, nx, nx), dtype=od)
    p = np.zeros((N + 1, nx), dtype=od)
    K = np.zeros((max(N, 1), 2, nx), dtype=od)[:N]
    kff = np.zeros((max(N, 1), 2), dtype=od)[:N]
    _, _, Q, _, _, gx, _, _ = dense_stage(c, N, dtype, delta)
    P[N], p[N] = Q, gx
    ok, margin = True, np.inf
    for k in range(N - 1, -1, -1):
        A, B, Q, R, S, gx, gu, b = dense_stage(c, k, dtype, delta)
        Pn, pn = P[k + 1], p[k + 1]
        BtP = B.T @ Pn
        Lam = R + BtP @ B
        G = S + BtP @ A
        L00, L01, L11 = Lam[0, 0], Lam[0, 1], Lam[1, 1]
        det = L00 * L11 - L01 * L01
        s00 = abs(R[0, 0]) + abs(Lam[0, 0] - R[0, 0])
        sdet = abs(L00 * L11) + L01 * L01
        margin = min(margin, float(abs(L00) / s00), float(abs(det) / sdet))
        if not (L00 > 0 and det > 0):
            ok = False
            break
        inv = np.array([[L11, -L01], [-L01, L00]], dtype=od) / det
        h = pn + Pn @ b
        K[k] = -(inv @ G)
        kff[k] = -(inv @ (gu + B.T @ h))
        P[k] = Q + A.T @ Pn @ A + G.T @ K[k]
        p[k] = gx + A.T @ h + G.T @ kff[k]
    res = dict(ok=ok, margin=margin, delta=delta, P=P, p=p, K=K, kff=kff)
    if ok:
        du = np.zeros((N + 1, 2), dtype=od)
        dx = np.zeros((N + 1, nx), dtype=od)
        dx[0] = -_conv(c.c0, dtype)
        for k in range(N):
            A, B, _, _, _, _, _, b = dense_stage(c, k, dtype, delta)
            du[k] = K[k] @ dx[k] + kff[k]
            dx[k + 1] = A @ dx[k] + B @ du[k] + b
        res.update(du=du, dx=dx, lam=np.stack([P[k] @ dx[k] + p[k] for k in range(N + 1)]))
    return res


def next_delta(delta, delta_last):
    """the inertia-correction schedule of riccati_instance, in the float64 arithmetic the kernels run it in"""
    if delta == 0.0:
        return DW_0 if delta_last == 0.0 else max(DW_MIN, KW_MINUS * delta_last)
    return delta * (KW_PLUS_BAR if delta_last == 0.0 else KW_PLUS)


def solve(c, dtype):
    """the sweep repeated along the schedule: the accepted sweep's results + `sweeps`, `margin` over every sweep tried"""
    delta, sweeps, margin = 0.0, 0, np.inf
    while True:
        sweeps += 1
        res = sweep(c, delta, dtype)
        margin = min(margin, res["margin"])
        if res["ok"]:
            break
        delta = next_delta(delta, c.delta_last)
        if delta > DW_MAX:
            break
    res.update(sweeps=sweeps, margin=margin, delta=delta if res["ok"] else delta)
    return res


# ------------------------------------------------------------------------------------------------------------------- error measures
def errors(got, ref):
    """The measures of tools/ubench/ric_mfma_test.hip against `ref`: per stage, max-norm relative, the worst stage -- for the cost-to-go
    matrix P, its vector p, the gains K together with k_ff, and the step dz = (du, dx).  `got` / `ref`: dicts with P, p, K, kff, du, dx."""
    f = lambda v: np.asarray(v, dtype=np.longdouble)
    N = f(ref["p"]).shape[0] - 1

    def rel(a, b):
        s = np.abs(b).max() if b.size else 0.0
        return float(np.abs(a - b).max() / (s if s > 0 else 1.0)) if b.size else 0.0

    e = dict.fromkeys(MEASURES, 0.0)
    for k in range(N + 1):
        e["P"] = max(e["P"], rel(f(got["P"][k]), f(ref["P"][k])))
        e["p"] = max(e["p"], rel(f(got["p"][k]), f(ref["p"][k])))
        if k < N:
            e["K"] = max(e["K"], rel(np.concatenate([f(got["K"][k]).ravel(), f(got["kff"][k])]), np.concatenate([f(ref["K"][k]).ravel(), f(ref["kff"][k])])))
        e["dz"] = max(e["dz"], rel(np.concatenate([f(got["du"][k]), f(got["dx"][k])]), np.concatenate([f(ref["du"][k]), f(ref["dx"][k])])))
    return e


# ------------------------------------------------------------------------------------------------------------------- case files
# The flat batch of cases both harnesses read (tests/ricx/ricx.cpp on the CPU, tools/ubench/ric_mfma_test on the GPU), all doubles, every
# state dimension padded to six:
#   in :  [n]  then per case  [nx, N, dt, delta_last, sym, hux0, hux1, c0[6]]  +  (N + 1) x [H[6][6], ruu[2], a[6], gx[6], gu[2], cn[6]]
#   out:  per case and code path  [ok, delta, sweeps]  +  (N + 1) x [P[6][6], p[6], K0[6], K1[6], kff[2], du[2], dx[6]]
CASE_HEAD, CASE_STAGE, OUT_HEAD, OUT_STAGE = 13, 58, 3, 64


def pack_cases(cases):
    out = [np.array([float(len(cases))])]
    for c in cases:
        nx, S = c.nx, c.N + 1
        head = np.zeros(CASE_HEAD)
        head[:7] = nx, c.N, c.dt, c.delta_last, float(c.sym), c.hux[0], c.hux[1]
        head[7:7 + nx] = c.c0
        st = np.zeros((S, CASE_STAGE))
        Hp = np.zeros((S, NX_PAD, NX_PAD))
        Hp[:, :nx, :nx] = c.H
        st[:, 0:36] = Hp.reshape(S, 36)
        st[:, 36:38] = c.ruu
        st[:, 38:44] = c.a
        st[:, 44:44 + nx] = c.gx
        st[:, 50:52] = c.gu
        st[:, 52:52 + nx] = c.cn
        out += [head, st.ravel()]
    return np.concatenate(out)


def out_size(cases):
    return sum(OUT_HEAD + (c.N + 1) * OUT_STAGE for c in cases)


def unpack_results(flat, cases):
    """one dict per case, as sweep() returns them (float64), from one code path's block of an output file"""
    res, o = [], 0
    for c in cases:
        nx, S = c.nx, c.N + 1
        ok, delta, sweeps = flat[o:o + 3]
        st = flat[o + 3:o + 3 + S * OUT_STAGE].reshape(S, OUT_STAGE)
        o += OUT_HEAD + S * OUT_STAGE
        res.append(dict(ok=ok > 0, delta=float(delta), sweeps=int(sweeps), P=st[:, :36].reshape(S, 6, 6)[:, :nx, :nx], Pfull=st[:, :36].reshape(S, 6, 6),
                        p=st[:, 36:36 + nx], pfull=st[:, 36:42], K=np.stack([st[:-1, 42:42 + nx], st[:-1, 48:48 + nx]], axis=1),
                        Kfull=np.stack([st[:-1, 42:48], st[:-1, 48:54]], axis=1), kff=st[:-1, 54:56], du=st[:, 56:58], dx=st[:, 58:58 + nx]))
    assert o == flat.size, (o, flat.size)
    return res


# ------------------------------------------------------------------------------------------------------------------- the test batch
PER_GROUP = 8            # compared cases per (family, nx, N)


def accuracy_batch(seed=0):
    """The cases of the accuracy tests, in file order, and the draws spent per family: for every (nx, N) eight cases of each family (nine
    indefinite ones: three per delta_last; the rank-one cases marked, four of them once more without the mark), the families interleaved so
    that the two instances of a wavefront are of different kinds (and three indefinite ones next to each other at the end of a group)."""
    cases, draws = [], {f: [0, 0] for f in FAMILIES}
    for nx in (5, 6):
        for N in NS_ALL:
            fam = {}
            for f in FAMILIES:
                if f == "decoupled" and nx != 6:
                    continue
                n = 9 if f == "indefinite" else PER_GROUP
                fam[f], d = generate(f, nx, N, n, seed)
                draws[f][0] += d
                draws[f][1] += n
            fam["rankone-nosym"] = [with_sym(c, False) for c in fam["rankone"][:4]]
            tail = fam["indefinite"][6:]             # (three in a row: some wavefront holds two instances that are both swept again)
            fam["indefinite"] = fam["indefinite"][:6]
            for i in range(PER_GROUP):
                cases += [v[i] for v in fam.values() if i < len(v)]
            cases += tail
    return cases, draws


# ------------------------------------------------------------------------------------------------------------------- pass criteria
PATHS = {"sym": 0, "plain": 1, "decoupled": 2}        # ricx::Path of tools/ubench/ric_cases.h
MARGIN = {f: 10.0 for f in FAMILIES}                 # kernel error <= max(1e-13, MARGIN x e_plain), per family and measure
FLOOR = 1e-13                                         # the agreement csrc/mpc_riccati_mfma.h claims on benign data
# The mark (sym) is what the rank-one family is about, and the family's own bound cannot see it go missing: an uncompensated recursion is
# "within 10 x of the plain twin" by construction.  Where Lam = Ruu + w g g' is dominated by its rank-one part the twin's error IS the
# cancellation error of det(Lam) and adj(Lam) G (the family's e_plain is 1e3 x the barrier family's for that reason), and the compensated
# products carry exactly those rounding errors along, so a working compensation sits orders of magnitude below the twin, not beside
# it.  One tenth of e_plain separates the two without leaning on how many orders it is.
RANKONE_GAIN = 0.1


def family_key(c):
    return c.family + ("-nosym" if c.family == "rankone" and not c.sym else "")


def plain_errors(cases):
    """e_plain per (family, measure): the float64 twin against the long-double reference at the reference's delta, the family's worst case"""
    e = collections.defaultdict(float)
    for c in cases:
        tw = sweep(c, c.ref["delta"], np.float64)
        for m, v in errors(tw, c.ref).items():
            e[family_key(c), m] = max(e[family_key(c), m], v)
    return e


def judge(label, cases, results, e_plain, paths_of=lambda c: True):
    """prints the worst error / e_plain per family and measure; returns the failures of the asserted families"""
    worst = collections.defaultdict(float)
    who = {}
    count = collections.Counter()
    fails = []
    for c, r in zip(cases, results):
        if not paths_of(c):
            continue
        ref = c.ref
        if not (r["ok"] == ref["ok"] and r["delta"] == ref["delta"]):
            fails.append(f"{label} {c.name}: ok / delta {r['ok']} / {r['delta']!r}, reference {ref['ok']} / {ref['delta']!r}")
            continue
        count[family_key(c), c.nx, c.N] += 1
        for m, v in errors(r, ref).items():
            if v >= worst[family_key(c), m]:
                worst[family_key(c), m], who[family_key(c), m] = v, c.name
    for (fam, m), v in sorted(worst.items()):
        ep = e_plain[fam, m]
        asserted = not fam.endswith("-nosym")
        bound = max(FLOOR, MARGIN[fam.split("-")[0]] * ep)
        print(f"{label:12s} {fam:14s} {m:2s}: error {v:9.2e}  e_plain {ep:9.2e}  ratio {v / ep if ep > 0 else float('inf'):9.3g}  bound {bound:9.2e}"
              f"{'' if asserted else '  (not asserted)'}  worst: {who[fam, m]}")
        if asserted and not v <= bound:
            fails.append(f"{label} {fam} {m}: {v:.3e} > {bound:.3e} (e_plain {ep:.3e}) at {who[fam, m]}")
        if fam == "rankone" and not v <= max(FLOOR, RANKONE_GAIN * ep):
            fails.append(f"{label} {fam} {m}: {v:.3e} with the mark is not {RANKONE_GAIN} x the plain twin's {ep:.3e}: the compensation is not working")
    return fails, count


def check_counts(count, families):
    for f in families:
        for nx in (5, 6):
            if f == "decoupled" and nx == 5:
                continue
            for N in NS_ALL:
                assert count[f, nx, N] >= PER_GROUP, (f, nx, N, count[f, nx, N])


def decoupled_zeros_exact(c, r):
    """row and column 5 of every P_k, p_k[5] and K[:, 5]: exactly 0.0 (signed zeros included in "zero")"""
    return not (np.any(r["Pfull"][:, 5, :]) or np.any(r["Pfull"][:, :, 5]) or np.any(r["pfull"][:, 5]) or np.any(r["Kfull"][:, :, 5]))
