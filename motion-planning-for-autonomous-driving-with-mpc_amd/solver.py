"""
BatchedMPCSolver -- thin Python owner of an `mpc_handle` (include/mpcgpu.h).

One handle = one problem template (horizon, weights, obstacle, bounds) + its device workspace; it solves B
independent instances of the NLP of MPC_Planner/optimizer.py:373-558 per call, i.e. B times the reference's
`sol(x0=..., p=..., lbg=..., lbx=..., ubg=..., ubx=...)` (optimizer.py:607).

All arithmetic happens in the HIP kernels of csrc/mpcgpu.hip.  No CPU fallback exists: constructing a solver
without the built library or without a GPU raises.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _abi
from ._abi import MpcLibraryError, MpcProblemDesc


RESCUE_FRACTIONS = (0.0, 0.4, 0.7, 0.9, 1.0)      # of the circle-distance lower bound, see rescue_failed()


def _big(a, n):
    """a bound list of the FORCES formulation as n doubles, +-inf as +-1e308"""
    a = np.asarray(a, dtype=np.float64).reshape(n)
    return _abi.f64(np.where(np.isfinite(a), a, np.sign(a) * 1e308))


def _loop_in(init_state, path, orient, vdes):
    """what every closed loop starts from, as contiguous arrays: init_state [B,5] (or [5]: one ego), path [B,Lp,2], orient [B,Lp], vdes [B] (or a
    scalar) -> (init_state, path, orient, vdes, B, Lp)"""
    init_state = _abi.f64(init_state)
    if init_state.ndim == 1:
        init_state = init_state[None]
    B = init_state.shape[0]
    path = _abi.f64(path).reshape(B, -1, 2)
    Lp = path.shape[1]
    orient = _abi.f64(orient).reshape(B, Lp)
    vdes = _abi.f64(np.broadcast_to(np.asarray(vdes, dtype=np.float64), (B,)))
    return init_state, path, orient, vdes, B, Lp


def _vp(d_ptr):
    """a device pointer or stream handle given as an int (0: absent)"""
    return C.c_void_p(d_ptr or None)


class MpcError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"mpcgpu error {code}: {msg}")
        self.code = code


@dataclass
class SolveResult:
    x: np.ndarray          # [B, n_w] rows in the reference's decision-vector order (optimizer.py:550)
    status: np.ndarray     # [B] int32, 1 converged / 0 max-iter / -6 NaN / -7 no progress
    iters: np.ndarray      # [B] int32
    kkt: np.ndarray        # [B] scaled KKT error at exit
    # solve(..., multipliers=True): what CasADi's `sol(...)` returns besides x (include/mpcgpu.h, mpc_solve_batch_ex)
    f: np.ndarray | None = None        # [B] objective at x
    g: np.ndarray | None = None        # [B, n_g] constraint rows at x (order of mpc_set_bounds)
    lam_g: np.ndarray | None = None    # [B, n_g] multipliers of the rows, NaN where status != 1
    lam_x: np.ndarray | None = None    # [B, n_w] multipliers of the bounds (z_U - z_L), NaN where status != 1
    # solve(..., lam_p=True / dp=...): parametric sensitivities (include/mpcgpu.h, mpc_solve_batch_sens)
    lam_p: np.ndarray | None = None    # [B, n_p] CasADi's lam_p = d/dp [f + lam_g' g + lam_x' x], NaN where status != 1
    dw: np.ndarray | None = None       # [B, n_dir, n_w] (dw*/dp) dp for the seeds dp [B, n_dir, n_p], NaN where status != 1


@dataclass
class ObstSens:
    """sens_obst(): the derivative of the last solve's optimum with respect to the six obstacle circle centres o [B, 6] (mpc_sens_obst)"""
    dw: np.ndarray | None = None         # [B, n_dir, n_w] (dw*/do) dobst, NaN where status != 1
    grad_obst: np.ndarray | None = None  # [B, 6] (dw*/do)' seed_w
    lam_obst: np.ndarray | None = None   # [B, 6] d/do [f + lam_g' g] = d f*/do


@dataclass
class WeightSens:
    """sens_weights(): the derivative of the last solve's optimum with respect to the seven cost weights wt = [Q_0 .. Q_4 | R_0, R_1]
    (mpc_sens_weights).  The weights are shared by the batch; the rows are per instance (sum them for the derivative of a batch loss)"""
    dw: np.ndarray | None = None         # [B, n_dir, n_w] (dw*/dwt) dweights, NaN where status != 1
    grad_wt: np.ndarray | None = None    # [B, 7] (dw*/dwt)' seed_w
    lam_wt: np.ndarray | None = None     # [B, 7] d/dwt [f + lam_g' g] = d f*/dwt


@dataclass
class BoundSens:
    """sens_bounds(): the derivative of the last solve's optimum with respect to the bound vector bv = [lbx (n_w) | ubx (n_w) | fl, fu, ol, ou]
    (mpc_sens_bounds; n_b = 2 n_w + 4, see BatchedMPCSolver.bounds_vector).  The bounds are shared by the batch; the rows are per instance (sum
    them for the derivative of a batch loss)"""
    dw: np.ndarray | None = None         # [B, n_dir, n_w] (dw*/dbv) dbounds, NaN where status != 1
    grad_bv: np.ndarray | None = None    # [B, n_b] (dw*/dbv)' seed_w
    lam_bv: np.ndarray | None = None     # [B, n_b] d f*/dbv


@dataclass
class LoopLin:
    """closed_loop(..., linearize=True): the rollout and the per-step feedback gains of the first control of every solve
    (mpc_closed_loop_batch_lin).  Rows of a step whose status is not 1, or whose factor failed, are NaN."""
    traj: np.ndarray                      # [B, L, 5] state before step i
    ctrl: np.ndarray                      # [B, L, 2] applied controls
    status: np.ndarray                    # [B, L] int32
    kgain: np.ndarray                     # [B, L, 2, 5] d u*_0 / d traj[b, i]
    wgain: np.ndarray                     # [B, L, 2, 7] d u*_0 / d [Q_0 .. Q_4 | R_0, R_1]
    ogain: np.ndarray | None = None       # [B, L, 2, 3] d u*_0 / d (x, y, heading) of the obstacle at step i (with obst_track)
    clearance: np.ndarray | None = None   # [B, L] (with obst_track and clearance=True)
    Lt: int = 0                           # poses per track (0: no obst_track)


class BatchedMPCSolver:
    def __init__(self, N, nx=5, *, dt=0.1, Q=None, R=None, P=None, obstacle_centers=None, wheelbase=2.5789128,
                 friction_div=2.578, ego_offset=0.75, max_iter=100, tol=1e-8, fixed_iters=0, obst_mult=3, device=0,
                 lib_path=None):
        self._lib = _abi.load_library(lib_path)
        d = MpcProblemDesc()
        self._lib.mpc_default_desc(C.byref(d), int(N), int(nx))
        d.dt, d.wheelbase, d.friction_div, d.ego_offset = float(dt), float(wheelbase), float(friction_div), float(ego_offset)
        d.max_iter, d.fixed_iters, d.obst_mult, d.device, d.tol = int(max_iter), int(fixed_iters), int(obst_mult), int(device), float(tol)
        if Q is not None:
            for i in range(8):
                d.Q[i] = float(Q[i]) if i < len(Q) else 0.0
        if R is not None:
            d.R[0], d.R[1] = float(R[0]), float(R[1])
        if P is not None:
            for i in range(8):
                d.P[i] = float(P[i]) if i < len(P) else 0.0
        if obstacle_centers is not None:
            oc = np.asarray(obstacle_centers, dtype=np.float64).ravel()
            assert oc.size == 6
            for i in range(6):
                d.obstacle[i] = oc[i]
        self.desc = d
        self.N, self.nx = int(N), int(nx)
        self.n_w = 2 * self.N + self.nx * (self.N + 1)
        self.n_g = 1 + self.nx * (self.N + 1) + 9 * (self.N + 1)
        self.n_b = 2 * self.n_w + 4
        self._h = C.c_void_p()
        self._sens_gen = 0          # solves that left a snapshot of their final iterates (mpc_solve_batch_sens): autograd.py checks it
        self._sens_B = 0            # ... and the batch size of the last of them
        rc = self._lib.mpc_create(C.byref(self._h), C.byref(d))
        if rc != _abi.MPC_OK:
            raise MpcError(rc, self._lib.mpc_last_error(None).decode())
        self._bounds_key = None

    # ------------------------------------------------------------------------------------------------
    def _check(self, rc):
        if rc != _abi.MPC_OK:
            raise MpcError(rc, self._lib.mpc_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.mpc_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------------------------------------
    def set_bounds(self, lbx=None, ubx=None, lbg=None, ubg=None):
        """the four lists of `inequal_constraints()` (optimizer.py:413-491); all None = reference defaults.  The lists the solver already
        holds are not installed again; anything else reaches mpc_set_bounds, which ends the life of the sensitivity snapshot, as a solve does."""
        if lbx is None and ubx is None and lbg is None and ubg is None:
            self._sens_gen += 1                              # (a backward pass of autograd.py on the old snapshot raises)
            self._check(self._lib.mpc_set_bounds(self._h, None, None, None, None))
            self._bounds_key = None
            self._bounds = None
            return
        arrs = [_abi.f64(a).ravel() for a in (lbx, ubx, lbg, ubg)]
        if arrs[0].size != self.n_w or arrs[1].size != self.n_w or arrs[2].size != self.n_g or arrs[3].size != self.n_g:
            raise MpcError(_abi.MPC_ERR_BOUNDS, f"expected lbx/ubx of {self.n_w} and lbg/ubg of {self.n_g} entries")
        key = tuple(a.tobytes() for a in arrs)
        if key == self._bounds_key:
            return
        self._sens_gen += 1
        self._check(self._lib.mpc_set_bounds(self._h, *[_abi.as_dp(a) for a in arrs]))
        self._bounds_key = key
        self._bounds = tuple(a.copy() for a in arrs)            # (lbx, ubx, lbg, ubg), for rescue_failed()

    def get_bounds(self):
        """(lbx [n_w], ubx [n_w], lbg [n_g], ubg [n_g]) as the handle holds them (mpc_get_bounds): what set_bounds installed, the reference
        defaults of an all-None call included"""
        out = np.empty(self.n_w), np.empty(self.n_w), np.empty(self.n_g), np.empty(self.n_g)
        self._check(self._lib.mpc_get_bounds(self._h, *[_abi.as_dp(a) for a in out]))
        return out

    def bounds_vector(self):
        """the bound vector bv [n_b] = [lbx (n_w) | ubx (n_w) | fl, fu, ol, ou] of get_bounds(): fl, fu are lbg[0], ubg[0] of the friction row,
        ol, ou the pair shared by the 9 (N + 1) circle rows (ol is the radius sum); what sens_bounds differentiates with respect to"""
        lbx, ubx, lbg, ubg = self.get_bounds()
        return np.concatenate([lbx, ubx, [lbg[0], ubg[0], lbg[-1], ubg[-1]]])

    def unpack_bounds(self, bv):
        """(lbx, ubx, lbg, ubg) of a bound vector [n_b], the arguments of set_bounds: the equality rows 0, every circle row [ol, ou]"""
        bv = _abi.f64(bv).ravel()
        if bv.size != self.n_b:
            raise MpcError(_abi.MPC_ERR_BOUNDS, f"expected a bound vector of {self.n_b} entries")
        nw, ne, no = self.n_w, self.nx * (self.N + 1), 9 * (self.N + 1)
        fl, fu, ol, ou = bv[2 * nw:]
        lbg = np.concatenate([[fl], np.zeros(ne), np.full(no, ol)])
        ubg = np.concatenate([[fu], np.zeros(ne), np.full(no, ou)])
        return bv[:nw].copy(), bv[nw: 2 * nw].copy(), lbg, ubg

    def set_weights(self, Q=None, R=None):
        """replaces the cost weights Q[0..4] and / or R[0..1] of the live handle (mpc_set_weights): host bookkeeping only, no device work,
        no synchronisation; every later call (FORCES-mode solves included) sees them.  Ends the life of the sensitivity snapshot, as a solve
        does.  Invalid weights (non-finite, Q < 0, R <= 0) raise MpcError with code MPC_ERR_INVALID and change nothing."""
        q = None if Q is None else _abi.f64(Q).ravel()[:5]
        r = None if R is None else _abi.f64(R).ravel()
        if (q is not None and q.size != 5) or (r is not None and r.size != 2):
            raise MpcError(_abi.MPC_ERR_INVALID, "set_weights: Q must have 5 entries (a sixth is ignored) and R 2")
        q = None if q is None else np.ascontiguousarray(q)
        self._check(self._lib.mpc_set_weights(self._h, _abi.as_dp(q), _abi.as_dp(r)))
        self._sens_gen += 1                                  # (a backward pass of autograd.py on the old snapshot raises)
        for i in range(5 if q is not None else 0):
            self.desc.Q[i] = q[i]
        for j in range(2 if r is not None else 0):
            self.desc.R[j] = r[j]

    @property
    def weights(self):
        """the current seven cost weights [Q_0 .. Q_4 | R_0, R_1]"""
        return np.array([self.desc.Q[i] for i in range(5)] + [self.desc.R[0], self.desc.R[1]])

    def _rows_in(self, name, x, p, obst):
        """(B, x [B, n_w], p [B, n_w], obst [B, 6] | [B, N+1, 6] | None) as contiguous doubles; a single instance may come as vectors"""
        x, p = _abi.f64(x), _abi.f64(p)
        if x.ndim == 1:
            x = x[None]
        if p.ndim == 1:
            p = p[None]
        B = x.shape[0]
        if x.shape != (B, self.n_w) or p.shape != (B, self.n_w):
            raise MpcError(_abi.MPC_ERR_INVALID, f"{name}/p must be [B, {self.n_w}]")
        if obst is not None and np.ndim(obst) == 3:            # centres per stage (mpc_solve_batch_stages)
            obst = _abi.f64(obst)
            if obst.shape != (B, self.N + 1, 6):
                raise MpcError(_abi.MPC_ERR_INVALID, f"obst per stage must be [B, {self.N + 1}, 6]")
            return B, x, p, obst
        return B, x, p, None if obst is None else _abi.f64(obst, (B, 6))

    def _nlp_out(self, B):
        """f [B], g [B, n_g], lam_g [B, n_g], lam_x [B, n_w] of a solve with multipliers"""
        return np.empty(B), np.empty((B, self.n_g)), np.empty((B, self.n_g)), np.empty((B, self.n_w))

    def eval_nlp(self, x, p, obst=None):
        """objective f [B] and constraint rows g [B, n_g] of the reference's NLP at any x [B, n_w] (mpc_eval_nlp_batch); obst [B, 6], or
        [B, N+1, 6]: every stage against centres of its own (mpc_eval_nlp_batch_stages)."""
        B, x, p, obst = self._rows_in("x", x, p, obst)
        f, g = np.empty(B), np.empty((B, self.n_g))
        fn = self._lib.mpc_eval_nlp_batch_stages if obst is not None and obst.ndim == 3 else self._lib.mpc_eval_nlp_batch
        self._check(fn(self._h, B, _abi.as_dp(x), _abi.as_dp(p), _abi.as_dp(obst), _abi.as_dp(f), _abi.as_dp(g)))
        return f, g

    def solve(self, x0, p, obst=None, *, multipliers=False, lam_p=False, dp=None, rsum=None) -> SolveResult:
        """B instances at once.  multipliers=True: also f, g at the returned x and the multipliers lam_g, lam_x (CasADi's convention:
        grad f + J_g' lam_g + lam_x = 0) in the result (mpc_solve_batch_ex).  lam_p=True: CasADi's lam_p; dp [B, n_dir, n_p] (or [B, n_p]):
        forward sensitivities dw = (dw*/dp) dp of the optimum (mpc_solve_batch_sens, which also keeps the final iterates for sens_adjoint).
        p = [U_ref | X_ref], n_p = n_w.  obst [B, 6]: obstacle centres per instance; [B, N+1, 6]: per instance and stage, an obstacle that
        moves over the horizon (mpc_solve_batch_stages) -- no derivatives: lam_p / dp raise, and a later sens_* finds no snapshot.
        rsum [B, N+1, 3] (with obst [B, N+1, 6]): a lower bound per circle row, rsum[b, k, j] for ego circle j against slot j of obst[b, k]
        (mpc_solve_batch_sized); None is the call without it."""
        B, x0, p, obst = self._rows_in("x0", x0, p, obst)
        out = np.empty_like(x0)
        status = np.empty(B, np.int32)
        iters = np.empty(B, np.int32)
        kkt = np.empty(B, np.float64)
        if rsum is not None:
            if obst is None or obst.ndim != 3:
                raise MpcError(_abi.MPC_ERR_INVALID, "rsum goes with obstacle centres per stage (obst [B, N+1, 6])")
            rsum = _abi.f64(rsum)
            if rsum.shape != (B, self.N + 1, 3):
                raise MpcError(_abi.MPC_ERR_INVALID, f"rsum must be [B, {self.N + 1}, 3]")
        if obst is not None and obst.ndim == 3:
            if lam_p or dp is not None:
                raise MpcError(_abi.MPC_ERR_INVALID, "derivatives of a solve with obstacle centres per stage are not provided (obst [B, N+1, 6])")
            self._sens_gen += 1                              # (the library has ended the life of an earlier snapshot)
            f, g, lam_g, lam_x = self._nlp_out(B) if multipliers else (None,) * 4
            if rsum is not None:
                self._check(self._lib.mpc_solve_batch_sized(self._h, B, _abi.as_dp(x0), _abi.as_dp(p), _abi.as_dp(obst), _abi.as_dp(rsum),
                                                            _abi.as_dp(out), _abi.as_ip(status), _abi.as_ip(iters), _abi.as_dp(kkt), _abi.as_dp(f),
                                                            _abi.as_dp(g), _abi.as_dp(lam_g), _abi.as_dp(lam_x)))
                return SolveResult(out, status, iters, kkt, f, g, lam_g, lam_x)
            self._check(self._lib.mpc_solve_batch_stages(self._h, B, _abi.as_dp(x0), _abi.as_dp(p), _abi.as_dp(obst), _abi.as_dp(out),
                                                         _abi.as_ip(status), _abi.as_ip(iters), _abi.as_dp(kkt), _abi.as_dp(f), _abi.as_dp(g),
                                                         _abi.as_dp(lam_g), _abi.as_dp(lam_x)))
            return SolveResult(out, status, iters, kkt, f, g, lam_g, lam_x)
        if lam_p or dp is not None:
            return self._solve_sens(x0, p, obst, out, status, iters, kkt, multipliers, lam_p, dp)
        if not multipliers:
            self._check(self._lib.mpc_solve_batch(self._h, B, _abi.as_dp(x0), _abi.as_dp(p), _abi.as_dp(obst), _abi.as_dp(out),
                                                  _abi.as_ip(status), _abi.as_ip(iters), _abi.as_dp(kkt)))
            return SolveResult(out, status, iters, kkt)
        f, g, lam_g, lam_x = self._nlp_out(B)
        self._check(self._lib.mpc_solve_batch_ex(self._h, B, _abi.as_dp(x0), _abi.as_dp(p), _abi.as_dp(obst), _abi.as_dp(out),
                                                 _abi.as_ip(status), _abi.as_ip(iters), _abi.as_dp(kkt), _abi.as_dp(f), _abi.as_dp(g),
                                                 _abi.as_dp(lam_g), _abi.as_dp(lam_x)))
        return SolveResult(out, status, iters, kkt, f, g, lam_g, lam_x)

    def _solve_sens(self, x0, p, obst, out, status, iters, kkt, multipliers, want_lam_p, dp):
        B = x0.shape[0]
        f = g = lam_g = lam_x = lp = dw = None
        if multipliers:
            f, g, lam_g, lam_x = self._nlp_out(B)
        if want_lam_p:
            lp = np.empty((B, self.n_w))
        n_dir = 0
        if dp is not None:
            dp = _abi.f64(dp)
            if dp.ndim == 2:
                dp = dp[:, None, :]
            if dp.ndim != 3 or dp.shape[0] != B or dp.shape[2] != self.n_w:
                raise MpcError(_abi.MPC_ERR_INVALID, f"dp must be [B, n_dir, {self.n_w}]")
            dp = np.ascontiguousarray(dp)
            n_dir = dp.shape[1]
            dw = np.empty((B, n_dir, self.n_w))
        self._sens_gen += 1
        self._sens_B = B
        self._check(self._lib.mpc_solve_batch_sens(self._h, B, _abi.as_dp(x0), _abi.as_dp(p), _abi.as_dp(obst), _abi.as_dp(out), _abi.as_ip(status),
                                                   _abi.as_ip(iters), _abi.as_dp(kkt), _abi.as_dp(f), _abi.as_dp(g), _abi.as_dp(lam_g),
                                                   _abi.as_dp(lam_x), _abi.as_dp(lp), n_dir, _abi.as_dp(dp), _abi.as_dp(dw)))
        return SolveResult(out, status, iters, kkt, f, g, lam_g, lam_x, lp, dw)

    def lam_p_of(self, x, p, lam_g, status):
        """CasADi's lam_p from what a solve with multipliers returned (the closed form k_sens_lam_p evaluates, same operations, same bits):
        X_ref column 0 -lam_g[pin rows], column k+1 -2 Q (x_k - xref_{k+1}), U_ref 0; NaN where status != 1.  Needs no snapshot."""
        N, nx = self.N, self.nx
        B = x.shape[0]
        Q = np.array([self.desc.Q[i] for i in range(nx)])
        out = np.zeros((B, self.n_w))
        out[:, 2 * N: 2 * N + nx] = -lam_g[:, 1: 1 + nx]
        xs = x[:, 2 * N: 2 * N + nx * N].reshape(B, N, nx)
        xr = p[:, 2 * N + nx:].reshape(B, N, nx)
        out[:, 2 * N + nx:] = (-2.0 * Q * (xs - xr)).reshape(B, N * nx)
        out[status != 1] = np.nan
        return out

    def sens_adjoint(self, seed_w):
        """reverse mode on the last solve(..., lam_p / dp) of this solver: seed_w [B, n_w] -> grad_p [B, n_p] = (dw*/dp)' seed_w
        (mpc_sens_adjoint; any solve in between -> MpcError with code MPC_ERR_STATE)"""
        seed = _abi.f64(seed_w)
        if seed.ndim == 1:
            seed = seed[None]
        grad = np.empty_like(seed)
        self._check(self._lib.mpc_sens_adjoint(self._h, seed.shape[0], _abi.as_dp(seed), _abi.as_dp(grad)))
        return grad

    def sens_obst(self, dobst=None, seed_w=None, lam=False) -> ObstSens:
        """the derivative of the optimum of the last solve(..., lam_p / dp) of this solver with respect to its six obstacle circle centres
        (the solve's obst rows, or the solver's own centres): dobst [B, n_dir, 6] (or [B, 6]) -> dw [B, n_dir, n_w]; seed_w [B, n_w] ->
        grad_obst [B, 6]; lam=True: lam_obst [B, 6], the derivative of the optimal objective (mpc_sens_obst; any solve in between ->
        MpcError with code MPC_ERR_STATE)"""
        B = self._sens_B
        dw = grad = lo = None
        n_dir = 0
        if dobst is not None:
            dobst = _abi.f64(dobst)
            if dobst.ndim == 2:
                dobst = dobst[:, None, :]
            if dobst.ndim != 3 or dobst.shape[0] != B or dobst.shape[2] != 6:
                raise MpcError(_abi.MPC_ERR_INVALID, f"dobst must be [{B}, n_dir, 6]")
            dobst = np.ascontiguousarray(dobst)
            n_dir = dobst.shape[1]
            dw = np.empty((B, n_dir, self.n_w))
        if seed_w is not None:
            seed_w = _abi.f64(seed_w, (B, self.n_w))
            grad = np.empty((B, 6))
        if lam:
            lo = np.empty((B, 6))
        self._check(self._lib.mpc_sens_obst(self._h, B, n_dir, _abi.as_dp(dobst), _abi.as_dp(dw), _abi.as_dp(seed_w), _abi.as_dp(grad), _abi.as_dp(lo)))
        return ObstSens(dw, grad, lo)

    def sens_weights(self, p, dweights=None, seed_w=None, lam=False) -> WeightSens:
        """the derivative of the optimum of the last solve(..., lam_p / dp) of this solver with respect to its seven cost weights
        wt = [Q_0 .. Q_4 | R_0, R_1] (see `weights`).  p [B, n_w]: the p of that solve (not checked against it).  dweights [B, n_dir, 7] (or
        [B, 7]) -> dw [B, n_dir, n_w]; seed_w [B, n_w] -> grad_wt [B, 7]; lam=True: lam_wt [B, 7], the derivative of the optimal objective
        (mpc_sens_weights; any solve or set_weights in between -> MpcError with code MPC_ERR_STATE)"""
        B = self._sens_B
        p = _abi.f64(p, (B, self.n_w))
        dw = grad = lw = None
        n_dir = 0
        if dweights is not None:
            dweights = _abi.f64(dweights)
            if dweights.ndim == 2:
                dweights = dweights[:, None, :]
            if dweights.ndim != 3 or dweights.shape[0] != B or dweights.shape[2] != 7:
                raise MpcError(_abi.MPC_ERR_INVALID, f"dweights must be [{B}, n_dir, 7]")
            dweights = np.ascontiguousarray(dweights)
            n_dir = dweights.shape[1]
            dw = np.empty((B, n_dir, self.n_w))
        if seed_w is not None:
            seed_w = _abi.f64(seed_w, (B, self.n_w))
            grad = np.empty((B, 7))
        if lam:
            lw = np.empty((B, 7))
        self._check(self._lib.mpc_sens_weights(self._h, B, _abi.as_dp(p), n_dir, _abi.as_dp(dweights), _abi.as_dp(dw), _abi.as_dp(seed_w), _abi.as_dp(grad),
                                               _abi.as_dp(lw)))
        return WeightSens(dw, grad, lw)

    def sens_bounds(self, dbounds=None, seed_w=None, lam=False) -> BoundSens:
        """the derivative of the optimum of the last solve(..., lam_p / dp) of this solver with respect to its bound vector bv (see
        bounds_vector): dbounds [B, n_dir, n_b] (or [B, n_b]) -> dw [B, n_dir, n_w]; seed_w [B, n_w] -> grad_bv [B, n_b]; lam=True: lam_bv
        [B, n_b], the derivative of the optimal objective.  Entries of absent bounds (+-inf) and of bounds the solve did not impose are 0 and
        their dbounds entries are not read (mpc_sens_bounds; any solve, set_bounds or set_weights in between -> MpcError with code
        MPC_ERR_STATE)"""
        B = self._sens_B
        dw = grad = lb = None
        n_dir = 0
        if dbounds is not None:
            dbounds = _abi.f64(dbounds)
            if dbounds.ndim == 2:
                dbounds = dbounds[:, None, :]
            if dbounds.ndim != 3 or dbounds.shape[0] != B or dbounds.shape[2] != self.n_b:
                raise MpcError(_abi.MPC_ERR_INVALID, f"dbounds must be [{B}, n_dir, {self.n_b}]")
            dbounds = np.ascontiguousarray(dbounds)
            n_dir = dbounds.shape[1]
            dw = np.empty((B, n_dir, self.n_w))
        if seed_w is not None:
            seed_w = _abi.f64(seed_w, (B, self.n_w))
            grad = np.empty((B, self.n_b))
        if lam:
            lb = np.empty((B, self.n_b))
        self._check(self._lib.mpc_sens_bounds(self._h, B, n_dir, _abi.as_dp(dbounds), _abi.as_dp(dw), _abi.as_dp(seed_w), _abi.as_dp(grad), _abi.as_dp(lb)))
        return BoundSens(dw, grad, lb)

    def feedback_gain(self, x0, p, obst=None):
        """du_0*/dxref_0 [B, nu, nx]: the linearised control law around the optimum (xref_0 is the measured state the plan starts from)"""
        x0 = _abi.f64(x0)
        B = x0.shape[0] if x0.ndim == 2 else 1
        nx = self.nx
        dp = np.zeros((B, nx, self.n_w))
        for i in range(nx):
            dp[:, i, 2 * self.N + i] = 1.0
        r = self.solve(x0, p, obst, dp=dp)
        return np.ascontiguousarray(r.dw[:, :, 0:2].transpose(0, 2, 1))

    def last_rescued(self):
        """instances of the last solve that took the second chance of the C-ABI (mpc_last_rescued)"""
        return int(self._lib.mpc_last_rescued(self._h))

    def solve_with_rescue(self, x0, p):
        """diagnostic form of solve(): the second chance for stalled instances (homotopy on the obstacle radius) runs on the
        device behind the C-ABI in every solve; this returns the result together with the mask of the instances that needed
        it, found by solving once with the option "rescue" off.  Returns (SolveResult, rescued mask)."""
        before = self.get_option("rescue")
        self.set_option("rescue", "0")
        try:
            plain = self.solve(x0, p)
        finally:
            self.set_option("rescue", before)          # what it was (the environment or the caller may have switched it off)
        if np.all(plain.status == 1):
            return plain, np.zeros(plain.status.shape[0], dtype=bool)
        res = self.solve(x0, p)
        return res, (plain.status != 1) & (res.status == 1)

    def solve_trace(self, x0, p, obst=None):
        x0 = _abi.f64(x0)
        p = _abi.f64(p)
        B = x0.shape[0]
        out = np.empty_like(x0)
        status, iters, kkt = np.empty(B, np.int32), np.empty(B, np.int32), np.empty(B)
        rows = int(self.desc.max_iter) + 1
        trace = np.zeros((rows, 8, B))
        n_it = np.zeros(1, np.int32)
        if obst is not None:
            obst = _abi.f64(obst, (B, 6))
        self._check(self._lib.mpc_solve_batch_trace(self._h, B, _abi.as_dp(x0), _abi.as_dp(p), _abi.as_dp(obst), _abi.as_dp(out),
                                                    _abi.as_ip(status), _abi.as_ip(iters), _abi.as_dp(kkt), _abi.as_dp(trace), rows,
                                                    _abi.as_ip(n_it)))
        return SolveResult(out, status, iters, kkt), trace[: int(n_it[0]) + 1]

    def _dev_rows(self, B, d_x0, d_p, d_obst, d_x_out, d_status, d_iters, d_kkt):
        """the leading arguments of every device-pointer solve"""
        return [self._h, int(B), _vp(d_x0), _vp(d_p), _vp(d_obst), _vp(d_x_out), _vp(d_status), _vp(d_iters), _vp(d_kkt)]

    def solve_device(self, B, d_x0, d_p, d_x_out, d_status=0, d_iters=0, d_kkt=0, d_obst=0, stream=0, d_f=0, d_g=0, d_lam_g=0, d_lam_x=0,
                     d_lam_p=0, n_dir=0, d_dp=0, d_dw=0, obst_stages=False, d_rsum=0):
        """device pointers (ints, e.g. torch.Tensor.data_ptr()) and a hipStream_t handle (int, 0 = default).  d_f [B], d_g / d_lam_g
        [B, n_g], d_lam_x [B, n_w]: the extra outputs of mpc_solve_batch_dev_ex (0 = not asked for).  d_lam_p [B, n_p], n_dir > 0 with
        d_dp [B, n_dir, n_p] -> d_dw [B, n_dir, n_w]: mpc_solve_batch_sens_dev (keeps the final iterates for sens_adjoint_device).
        obst_stages=True: d_obst is [B, N+1, 6], centres per stage (mpc_solve_batch_stages_dev; no sensitivity outputs).
        d_rsum (with obst_stages): [B, N+1, 3], a lower bound per circle row (mpc_solve_batch_sized_dev); 0 is the call without it."""
        rows = self._dev_rows(B, d_x0, d_p, d_obst, d_x_out, d_status, d_iters, d_kkt)
        extra = [_vp(d_f), _vp(d_g), _vp(d_lam_g), _vp(d_lam_x)]
        if d_rsum and not obst_stages:
            raise MpcError(_abi.MPC_ERR_INVALID, "d_rsum goes with obstacle centres per stage (obst_stages)")
        if obst_stages:
            if d_lam_p or n_dir:
                raise MpcError(_abi.MPC_ERR_INVALID, "derivatives of a solve with obstacle centres per stage are not provided (obst_stages)")
            self._sens_gen += 1
            if d_rsum:
                self._check(self._lib.mpc_solve_batch_sized_dev(*rows[:5], _vp(d_rsum), *rows[5:], *extra, _vp(stream)))
                return
            self._check(self._lib.mpc_solve_batch_stages_dev(*rows, *extra, _vp(stream)))
        elif d_lam_p or n_dir:
            self._sens_gen += 1
            self._sens_B = int(B)
            self._check(self._lib.mpc_solve_batch_sens_dev(*rows, *extra, _vp(d_lam_p), int(n_dir), _vp(d_dp), _vp(d_dw), _vp(stream)))
        elif d_f or d_g or d_lam_g or d_lam_x:
            self._check(self._lib.mpc_solve_batch_dev_ex(*rows, *extra, _vp(stream)))
        else:
            self._check(self._lib.mpc_solve_batch_dev(*rows, _vp(stream)))

    def solve_sens_device(self, B, d_x0, d_p, d_x_out, d_status=0, d_iters=0, d_kkt=0, d_obst=0, stream=0, d_lam_p=0, n_dir=0, d_dp=0, d_dw=0):
        """mpc_solve_batch_sens_dev even with no sensitivity output asked for: the solve plus the snapshot of its final iterates
        (what sens_adjoint_device differentiates)"""
        self._sens_gen += 1
        self._sens_B = int(B)
        self._check(self._lib.mpc_solve_batch_sens_dev(*self._dev_rows(B, d_x0, d_p, d_obst, d_x_out, d_status, d_iters, d_kkt), None, None, None, None,
                                                       _vp(d_lam_p), int(n_dir), _vp(d_dp), _vp(d_dw), _vp(stream)))
        return self._sens_gen

    def sens_adjoint_device(self, B, d_seed_w, d_grad_p, stream=0):
        """device form of sens_adjoint (enqueued on `stream`, not synchronised)"""
        self._check(self._lib.mpc_sens_adjoint_dev(self._h, int(B), _vp(d_seed_w), _vp(d_grad_p), _vp(stream)))

    def sens_obst_device(self, B, n_dir=0, d_dobst=0, d_dw=0, d_seed_w=0, d_grad_obst=0, d_lam_obst=0, stream=0):
        """device form of sens_obst (enqueued on `stream`, not synchronised): d_dobst [B, n_dir, 6] -> d_dw [B, n_dir, n_w], d_seed_w [B, n_w] ->
        d_grad_obst [B, 6], d_lam_obst [B, 6]; 0 = not asked for"""
        self._check(self._lib.mpc_sens_obst_dev(self._h, int(B), int(n_dir), _vp(d_dobst), _vp(d_dw), _vp(d_seed_w), _vp(d_grad_obst), _vp(d_lam_obst),
                                                _vp(stream)))

    def sens_weights_device(self, B, d_p, n_dir=0, d_dweights=0, d_dw=0, d_seed_w=0, d_grad_wt=0, d_lam_wt=0, stream=0):
        """device form of sens_weights (enqueued on `stream`, not synchronised): d_p [B, n_w] the p of the solve; d_dweights [B, n_dir, 7] ->
        d_dw [B, n_dir, n_w], d_seed_w [B, n_w] -> d_grad_wt [B, 7], d_lam_wt [B, 7]; 0 = not asked for"""
        self._check(self._lib.mpc_sens_weights_dev(self._h, int(B), _vp(d_p), int(n_dir), _vp(d_dweights), _vp(d_dw), _vp(d_seed_w), _vp(d_grad_wt),
                                                   _vp(d_lam_wt), _vp(stream)))

    def sens_bounds_device(self, B, n_dir=0, d_dbounds=0, d_dw=0, d_seed_w=0, d_grad_bv=0, d_lam_bv=0, stream=0):
        """device form of sens_bounds (enqueued on `stream`, not synchronised): d_dbounds [B, n_dir, n_b] -> d_dw [B, n_dir, n_w], d_seed_w
        [B, n_w] -> d_grad_bv [B, n_b], d_lam_bv [B, n_b]; 0 = not asked for"""
        self._check(self._lib.mpc_sens_bounds_dev(self._h, int(B), int(n_dir), _vp(d_dbounds), _vp(d_dw), _vp(d_seed_w), _vp(d_grad_bv), _vp(d_lam_bv),
                                                  _vp(stream)))

    def plant_step(self, x, u, integrator="euler"):
        x = _abi.f64(x)
        u = _abi.f64(u)
        single = x.ndim == 1
        x2 = x.reshape(-1, self.nx)
        u2 = u.reshape(-1, 2)
        out = np.empty_like(x2)
        self._check(self._lib.mpc_plant_step(self._h, x2.shape[0], 0 if integrator == "euler" else 1, _abi.as_dp(x2), _abi.as_dp(u2),
                                             _abi.as_dp(out)))
        return out[0] if single else out

    def closed_loop(self, init_state, path, orient, vdes, steps, noise_mode=0, sigma=0.0, seed=0, obst_track=None, obst_offset=0.0, clearance=False,
                    linearize=False, predict=False):
        """B egos through `steps` receding-horizon steps on the device (include/mpcgpu.h: mpc_closed_loop_batch_ex; the loop
        body of CasadiOptimizer.optimize, optimizer.py:596-631).  init_state [B,5], path [B,Lp,2], orient [B,Lp],
        vdes [B] -> (traj [B,steps,5], ctrl [B,steps,2], step_status [B,steps]).  noise_mode / sigma / seed: the reference's
        `noised: True` with a counter-based generator (noise.py holds the Python mirror of the samples).
        obst_track [B,Lt,3] (x, y, heading; Lt = 1: standing still, Lt >= steps: row i at step i; [B,3] = Lt 1): every ego past an obstacle of
        its own, frozen over each solve's horizon (mpc_closed_loop_batch_obst); obst_offset: its front / rear circle centres along the heading.
        clearance=True (with a track): a fourth return value [B,steps], see include/mpcgpu.h.
        predict=True (with a track): the obstacle predicted over each solve's horizon instead -- stage k of the solve of step i sees track row
        min(i + k, Lt - 1) (mpc_closed_loop_batch_pred); not with linearize.
        linearize=True: a LoopLin instead -- the same rollout, step by step, with the gains kgain, wgain and (with a track) ogain of every step
        (mpc_closed_loop_batch_lin), what loop_tangent / loop_adjoint sweep over."""
        init_state, path, orient, vdes, B, Lp = _loop_in(init_state, path, orient, vdes)
        steps = int(steps)
        traj = np.empty((B, steps, 5))
        ctrl = np.empty((B, steps, 2))
        st = np.empty((B, steps), np.int32)
        tail = (int(noise_mode), float(sigma), int(seed) & (2 ** 64 - 1), _abi.as_dp(traj), _abi.as_dp(ctrl), _abi.as_ip(st))
        if predict and (obst_track is None or linearize):
            raise MpcError(_abi.MPC_ERR_INVALID, "predict needs obst_track, and the linearised loop has no predicted form")
        if obst_track is None:
            if clearance:
                raise MpcError(_abi.MPC_ERR_INVALID, "clearance needs obst_track")
            if linearize:
                kg, wg = np.empty((B, steps, 2, 5)), np.empty((B, steps, 2, 7))
                self._check(self._lib.mpc_closed_loop_batch_lin(self._h, B, steps, Lp, _abi.as_dp(init_state), _abi.as_dp(path), _abi.as_dp(orient),
                                                                _abi.as_dp(vdes), 0, None, 0.0, *tail, None, _abi.as_dp(kg), _abi.as_dp(wg), None))
                return LoopLin(traj, ctrl, st, kg, wg)
            self._check(self._lib.mpc_closed_loop_batch_ex(self._h, B, steps, Lp, _abi.as_dp(init_state), _abi.as_dp(path), _abi.as_dp(orient),
                                                           _abi.as_dp(vdes), *tail))
            return traj, ctrl, st
        track = _abi.f64(obst_track)
        if track.ndim == 1:
            track = track[None]
        if track.ndim == 2:                                    # one ego: its poses; a batch: one standing pose per ego
            track = track[None] if B == 1 else track[:, None, :]
        if track.ndim != 3 or track.shape[0] != B or track.shape[2] != 3:
            raise MpcError(_abi.MPC_ERR_INVALID, "obst_track must be [B, Lt, 3]")
        cl = np.empty((B, steps)) if clearance else None
        if linearize:
            kg, wg, og = np.empty((B, steps, 2, 5)), np.empty((B, steps, 2, 7)), np.empty((B, steps, 2, 3))
            self._check(self._lib.mpc_closed_loop_batch_lin(self._h, B, steps, Lp, _abi.as_dp(init_state), _abi.as_dp(path), _abi.as_dp(orient),
                                                            _abi.as_dp(vdes), track.shape[1], _abi.as_dp(track), float(obst_offset), *tail, _abi.as_dp(cl),
                                                            _abi.as_dp(kg), _abi.as_dp(wg), _abi.as_dp(og)))
            return LoopLin(traj, ctrl, st, kg, wg, og, cl, track.shape[1])
        if predict:
            self._check(self._lib.mpc_closed_loop_batch_pred(self._h, B, steps, Lp, _abi.as_dp(init_state), _abi.as_dp(path), _abi.as_dp(orient),
                                                             _abi.as_dp(vdes), track.shape[1], _abi.as_dp(track), float(obst_offset), int(predict), *tail,
                                                             _abi.as_dp(cl)))
            return (traj, ctrl, st, cl) if clearance else (traj, ctrl, st)
        self._check(self._lib.mpc_closed_loop_batch_obst(self._h, B, steps, Lp, _abi.as_dp(init_state), _abi.as_dp(path), _abi.as_dp(orient),
                                                         _abi.as_dp(vdes), track.shape[1], _abi.as_dp(track), float(obst_offset), *tail, _abi.as_dp(cl)))
        return (traj, ctrl, st, cl) if clearance else (traj, ctrl, st)

    def closed_loop_device(self, B, d_init_state, d_path, d_orient, d_vdes, steps, Lp, d_traj, d_ctrl, d_step_status=0, noise_mode=0, sigma=0.0,
                           seed=0, stream=0, d_obst_track=0, Lt=0, obst_offset=0.0, d_clearance=0, predict=0):
        """device-pointer form (ints): the whole loop is enqueued on `stream`; see mpc_closed_loop_batch_dev_ex, and with d_obst_track [B,Lt,3]
        (d_clearance [B,steps] or 0) mpc_closed_loop_batch_obst_dev; predict != 0: mpc_closed_loop_batch_pred_dev with that value"""
        head = (self._h, int(B), int(steps), int(Lp), _vp(d_init_state), _vp(d_path), _vp(d_orient), _vp(d_vdes))
        tail = (int(noise_mode), float(sigma), int(seed) & (2 ** 64 - 1), _vp(d_traj), _vp(d_ctrl), _vp(d_step_status))
        if predict:
            self._check(self._lib.mpc_closed_loop_batch_pred_dev(*head, int(Lt), _vp(d_obst_track), float(obst_offset), int(predict), *tail, _vp(d_clearance),
                                                                 _vp(stream)))
        elif d_obst_track or Lt:
            self._check(self._lib.mpc_closed_loop_batch_obst_dev(*head, int(Lt), _vp(d_obst_track), float(obst_offset), *tail, _vp(d_clearance), _vp(stream)))
        else:
            self._check(self._lib.mpc_closed_loop_batch_dev_ex(*head, *tail, _vp(stream)))

    def closed_loop_traffic(self, init_state, path, orient, vdes, steps, tracks, offsets, pairing=0, noise_mode=0, sigma=0.0, seed=0, rsums=None):
        """B egos through traffic (mpc_closed_loop_batch_traffic): before every solve each stage of each ego gets the circle centres of the obstacle
        nearest to it at that stage's time -- the nearest-obstacle formulation; two obstacles equally close to one ego circle at one stage constrain
        it only once.  tracks [M,Lt,3] (x, y, heading; NaN x: absent at that row) with offsets [M]: one scene shared by all egos; tracks [B,M,Lt,3]
        with offsets [B,M]: a scene per ego.  Lt = 1 or Lt >= steps.  pairing 0: the reference's pairs on the nearest obstacle; 1: each ego circle
        against its nearest obstacle circle.  A handle has one radius: the lower bound of its circle rows holds for every obstacle.
        -> (traj [B,steps,5], ctrl [B,steps,2], step_status [B,steps], clearance [B,steps] over all nine pairs of every present obstacle (+inf: none),
        nearest [B,steps] (the obstacle that attains it, -1: none), chosen [B,steps,N+1,3] (the obstacle behind every slot of every stage))
        rsums (shaped like offsets; None: the call without it): traffic of mixed sizes (mpc_closed_loop_batch_traffic_sized) -- rsums[m] is the radius
        sum of ego and obstacle m, the selection is by clearance (distance less rsums[m] - the handle's radius), every slot of every solve carries
        its winner's radius, and clearance is the smallest distance - rsums[m]."""
        init_state, path, orient, vdes, B, Lp = _loop_in(init_state, path, orient, vdes)
        steps = int(steps)
        tracks, offsets = _abi.f64(tracks), _abi.f64(offsets)
        if tracks.ndim not in (3, 4) or tracks.shape[-1] != 3 or (tracks.ndim == 4 and tracks.shape[0] != B) or offsets.shape != tracks.shape[:-2]:
            raise MpcError(_abi.MPC_ERR_INVALID, "tracks must be [M, Lt, 3] with offsets [M], or [B, M, Lt, 3] with offsets [B, M]")
        M, Lt = tracks.shape[-3], tracks.shape[-2]
        traj, ctrl, st = np.empty((B, steps, 5)), np.empty((B, steps, 2)), np.empty((B, steps), np.int32)
        cl, near, chosen = np.empty((B, steps)), np.empty((B, steps), np.int32), np.empty((B, steps, self.N + 1, 3), np.int32)
        self._sens_gen += 1                                  # (like every loop: the library has ended the life of an earlier snapshot)
        if rsums is not None:
            rsums = _abi.f64(rsums)
            if rsums.shape != offsets.shape:
                raise MpcError(_abi.MPC_ERR_INVALID, "rsums must have the shape of offsets")
            self._check(self._lib.mpc_closed_loop_batch_traffic_sized(
                self._h, B, steps, Lp, _abi.as_dp(init_state), _abi.as_dp(path), _abi.as_dp(orient), _abi.as_dp(vdes), M, Lt, int(tracks.ndim == 4),
                _abi.as_dp(tracks), _abi.as_dp(offsets), _abi.as_dp(rsums), int(pairing), int(noise_mode), float(sigma), int(seed) & (2 ** 64 - 1),
                _abi.as_dp(traj), _abi.as_dp(ctrl), _abi.as_ip(st), _abi.as_dp(cl), _abi.as_ip(near), _abi.as_ip(chosen)))
            return traj, ctrl, st, cl, near, chosen
        self._check(self._lib.mpc_closed_loop_batch_traffic(self._h, B, steps, Lp, _abi.as_dp(init_state), _abi.as_dp(path), _abi.as_dp(orient), _abi.as_dp(vdes),
                                                            M, Lt, int(tracks.ndim == 4), _abi.as_dp(tracks), _abi.as_dp(offsets), int(pairing), int(noise_mode),
                                                            float(sigma), int(seed) & (2 ** 64 - 1), _abi.as_dp(traj), _abi.as_dp(ctrl), _abi.as_ip(st),
                                                            _abi.as_dp(cl), _abi.as_ip(near), _abi.as_ip(chosen)))
        return traj, ctrl, st, cl, near, chosen

    def closed_loop_traffic_device(self, B, d_init_state, d_path, d_orient, d_vdes, steps, Lp, M, Lt, per_ego, d_tracks, d_offsets, d_traj, d_ctrl,
                                   d_step_status=0, pairing=0, noise_mode=0, sigma=0.0, seed=0, d_clearance=0, d_nearest=0, d_chosen=0, stream=0, d_rsums=0):
        """device-pointer form (ints; 0 = absent) of closed_loop_traffic (mpc_closed_loop_batch_traffic_dev): d_tracks [M,Lt,3] / [B,M,Lt,3], d_offsets [M] /
        [B,M] by per_ego, d_nearest [B,steps] and d_chosen [B,steps,N+1,3] int32.  The offsets are copied back once and checked, then the whole loop is
        enqueued on `stream`.  d_rsums (shaped like d_offsets; 0: the call without it): mpc_closed_loop_batch_traffic_sized_dev."""
        self._sens_gen += 1
        if d_rsums:
            self._check(self._lib.mpc_closed_loop_batch_traffic_sized_dev(
                self._h, int(B), int(steps), int(Lp), _vp(d_init_state), _vp(d_path), _vp(d_orient), _vp(d_vdes), int(M), int(Lt), int(per_ego), _vp(d_tracks),
                _vp(d_offsets), _vp(d_rsums), int(pairing), int(noise_mode), float(sigma), int(seed) & (2 ** 64 - 1), _vp(d_traj), _vp(d_ctrl),
                _vp(d_step_status), _vp(d_clearance), _vp(d_nearest), _vp(d_chosen), _vp(stream)))
            return
        self._check(self._lib.mpc_closed_loop_batch_traffic_dev(self._h, int(B), int(steps), int(Lp), _vp(d_init_state), _vp(d_path), _vp(d_orient), _vp(d_vdes),
                                                                int(M), int(Lt), int(per_ego), _vp(d_tracks), _vp(d_offsets), int(pairing), int(noise_mode),
                                                                float(sigma), int(seed) & (2 ** 64 - 1), _vp(d_traj), _vp(d_ctrl), _vp(d_step_status),
                                                                _vp(d_clearance), _vp(d_nearest), _vp(d_chosen), _vp(stream)))

    def session(self, init_state, path, orient, vdes, steps, offsets=None, per_ego=None, pairing=0, rsums=None):
        """the loop stepped from outside (mpc_session_begin): a LoopSession, `with solver.session(...) as sess: u = sess.step(measured, obstacles)`.
        The arguments of closed_loop_traffic that do not change over a loop; offsets None: lane following (M = 0), [M]: obstacles shared by all egos,
        [B, M]: per ego (per_ego overrides what the shape says, e.g. B = 1).  One session per solver; everything is copied.
        rsums (shaped like offsets; None: the call without it): a sized session (mpc_session_begin_sized) -- rsums[m] is the radius sum of ego and
        obstacle m, the selection is by clearance and every step is a sized solve, as in closed_loop_traffic(rsums=)."""
        return LoopSession(self, init_state, path, orient, vdes, steps, offsets, per_ego, pairing, rsums)

    def closed_loop_lin_device(self, B, d_init_state, d_path, d_orient, d_vdes, steps, Lp, d_traj, d_ctrl, d_step_status=0, noise_mode=0, sigma=0.0,
                               seed=0, stream=0, d_obst_track=0, Lt=0, obst_offset=0.0, d_clearance=0, d_kgain=0, d_wgain=0, d_ogain=0):
        """device-pointer form of closed_loop(..., linearize=True) (mpc_closed_loop_batch_lin_dev): d_kgain [B,steps,2,5], d_wgain [B,steps,2,7],
        d_ogain [B,steps,2,3] (needs d_obst_track), 0 = not asked for; runs step by step, every solve synchronises `stream`"""
        self._check(self._lib.mpc_closed_loop_batch_lin_dev(self._h, int(B), int(steps), int(Lp), _vp(d_init_state), _vp(d_path), _vp(d_orient), _vp(d_vdes), int(Lt),
                                                            _vp(d_obst_track), float(obst_offset), int(noise_mode), float(sigma), int(seed) & (2 ** 64 - 1), _vp(d_traj),
                                                            _vp(d_ctrl), _vp(d_step_status), _vp(d_clearance), _vp(d_kgain), _vp(d_wgain), _vp(d_ogain), _vp(stream)))

    @staticmethod
    def _loop_dirs(name, a, B, tail):
        """an optional direction / seed array as contiguous doubles [B, ...tail] (None stays None)"""
        if a is None:
            return None
        a = _abi.f64(a)
        if a.shape != (B,) + tuple(tail):
            raise MpcError(_abi.MPC_ERR_INVALID, f"{name} must be {[B] + list(tail)}")
        return a

    def loop_tangent(self, lin: LoopLin, dinit=None, dwt=None, dtrack=None):
        """forward sweep over a linearised loop, no solve (mpc_loop_tangent): dinit [B,n_dir,5], dwt [B,n_dir,7], dtrack [B,n_dir,Lt,3] (needs
        lin.ogain), any of them None (zero) but not all -> (dtraj [B,n_dir,L,5], dctrl [B,n_dir,L,2]), the derivatives of lin.traj / lin.ctrl
        along every direction.  NaN from the first step with NaN gains on."""
        B, L = lin.traj.shape[:2]
        given = [a for a in (dinit, dwt, dtrack) if a is not None]
        if not given:
            raise MpcError(_abi.MPC_ERR_INVALID, "loop_tangent: one of dinit, dwt, dtrack is required")
        n_dir = np.asarray(given[0]).shape[1] if np.asarray(given[0]).ndim >= 2 else -1
        if n_dir < 0:
            raise MpcError(_abi.MPC_ERR_INVALID, "loop_tangent: directions are [B, n_dir, ...]")
        if dtrack is not None and lin.ogain is None:
            raise MpcError(_abi.MPC_ERR_INVALID, "loop_tangent: dtrack needs a loop linearised with obst_track")
        dinit = self._loop_dirs("dinit", dinit, B, (n_dir, 5))
        dwt = self._loop_dirs("dwt", dwt, B, (n_dir, 7))
        dtrack = self._loop_dirs("dtrack", dtrack, B, (n_dir, lin.Lt, 3))
        dtraj, dctrl = np.empty((B, n_dir, L, 5)), np.empty((B, n_dir, L, 2))
        self._check(self._lib.mpc_loop_tangent(self._h, B, L, n_dir, _abi.as_dp(_abi.f64(lin.traj)), _abi.as_dp(_abi.f64(lin.ctrl)), _abi.as_dp(_abi.f64(lin.kgain)),
                                               _abi.as_dp(_abi.f64(lin.wgain)), None if lin.ogain is None else _abi.as_dp(_abi.f64(lin.ogain)), int(lin.Lt),
                                               _abi.as_dp(dinit), _abi.as_dp(dwt), _abi.as_dp(dtrack), _abi.as_dp(dtraj), _abi.as_dp(dctrl)))
        return dtraj, dctrl

    def loop_adjoint(self, lin: LoopLin, seed_traj=None, seed_ctrl=None):
        """reverse sweep, no solve (mpc_loop_adjoint): seed_traj [B,L,5], seed_ctrl [B,L,2] (None: zero) -> (grad_init [B,5], grad_wt [B,7],
        grad_track [B,Lt,3] | None): the gradients of sum(seed_traj * traj) + sum(seed_ctrl * ctrl) with respect to init_state, the weights (per
        ego: sum the rows) and the obstacle poses.  An ego with NaN gains at some step has NaN gradients."""
        B, L = lin.traj.shape[:2]
        seed_traj = self._loop_dirs("seed_traj", seed_traj, B, (L, 5))
        seed_ctrl = self._loop_dirs("seed_ctrl", seed_ctrl, B, (L, 2))
        gi, gw = np.empty((B, 5)), np.empty((B, 7))
        gt = None if lin.ogain is None else np.empty((B, lin.Lt, 3))
        self._check(self._lib.mpc_loop_adjoint(self._h, B, L, _abi.as_dp(_abi.f64(lin.traj)), _abi.as_dp(_abi.f64(lin.ctrl)), _abi.as_dp(_abi.f64(lin.kgain)),
                                               _abi.as_dp(_abi.f64(lin.wgain)), None if lin.ogain is None else _abi.as_dp(_abi.f64(lin.ogain)), int(lin.Lt),
                                               _abi.as_dp(seed_traj), _abi.as_dp(seed_ctrl), _abi.as_dp(gi), _abi.as_dp(gw), _abi.as_dp(gt)))
        return gi, gw, gt

    def loop_tangent_device(self, B, L, n_dir, d_traj, d_ctrl, d_kgain=0, d_wgain=0, d_ogain=0, Lt=0, d_dinit=0, d_dwt=0, d_dtrack=0, d_dtraj=0, d_dctrl=0,
                            stream=0):
        """device form of loop_tangent (enqueued on `stream`, not synchronised); 0 = absent"""
        self._check(self._lib.mpc_loop_tangent_dev(self._h, int(B), int(L), int(n_dir), _vp(d_traj), _vp(d_ctrl), _vp(d_kgain), _vp(d_wgain), _vp(d_ogain), int(Lt),
                                                   _vp(d_dinit), _vp(d_dwt), _vp(d_dtrack), _vp(d_dtraj), _vp(d_dctrl), _vp(stream)))

    def loop_adjoint_device(self, B, L, d_traj, d_ctrl, d_kgain=0, d_wgain=0, d_ogain=0, Lt=0, d_seed_traj=0, d_seed_ctrl=0, d_grad_init=0, d_grad_wt=0,
                            d_grad_track=0, stream=0):
        """device form of loop_adjoint (enqueued on `stream`, not synchronised); 0 = absent"""
        self._check(self._lib.mpc_loop_adjoint_dev(self._h, int(B), int(L), _vp(d_traj), _vp(d_ctrl), _vp(d_kgain), _vp(d_wgain), _vp(d_ogain), int(Lt),
                                                   _vp(d_seed_traj), _vp(d_seed_ctrl), _vp(d_grad_init), _vp(d_grad_wt), _vp(d_grad_track), _vp(stream)))

    def last_loop_replayed(self):
        return bool(self._lib.mpc_last_loop_replayed(self._h))

    def metrics(self, traj, ref_path=None, origin_path=None, r_sum=None, all_pairs=False):
        """Post-hoc metrics of B planned trajectories [B,L,5] on the device (mpc_metrics_batch; mpc_planner.py:184-199,
        279-292): dict(deviation [B,L] | None, rmsd [B,2] | None, clearance [B] | None)."""
        traj = _abi.f64(traj)
        if traj.ndim == 2:
            traj = traj[None]
        B, L = traj.shape[0], traj.shape[1]
        dev = rm = cl = None
        Lo = 0
        if origin_path is not None:
            origin_path = _abi.f64(np.broadcast_to(np.asarray(origin_path, dtype=np.float64), (B,) + np.asarray(origin_path).shape[-2:]))
            Lo = origin_path.shape[1]
            dev = np.empty((B, L))
        if ref_path is not None:
            ref_path = _abi.f64(np.broadcast_to(np.asarray(ref_path, dtype=np.float64)[..., :L, :], (B, L, 2)))
            rm = np.empty((B, 2))
        if r_sum is not None:
            cl = np.empty(B)
        self._check(self._lib.mpc_metrics_batch(self._h, B, L, Lo, _abi.as_dp(traj), _abi.as_dp(ref_path), _abi.as_dp(origin_path),
                                                C.c_double(0.0 if r_sum is None else float(r_sum)), 1 if all_pairs else 0, _abi.as_dp(dev), _abi.as_dp(rm),
                                                _abi.as_dp(cl)))
        return dict(deviation=dev, rmsd=rm, clearance=cl)

    def validity(self, traj, obstacles=None, left=None, right=None, ego_length=4.3, ego_width=1.8, per_ego=None):
        """collision / road verdict of B planned trajectories [B,L,5] on the device (mpc_validity_batch; the check of the
        reference's test, test/test_mpc_planner.py:37-47).  obstacles: [n,5] static rectangles (x, y, length, width, orientation)
        or [n,L,5] per time step; left / right: boundary polylines [m,2] of the drivable corridor in driving direction.
        per_ego=True, or a 4-d array: obstacles [B,n,L,5] ([B,n,5] with per_ego=True: static), every trajectory against its own
        (mpc_validity_batch_ego).  Returns dict(first_collision [B], first_off_road [B]) -- step index or -1."""
        traj = _abi.f64(traj)
        if traj.ndim == 2:
            traj = traj[None]
        B, L = traj.shape[0], traj.shape[1]
        n_obst, ob = 0, None
        if obstacles is not None and len(obstacles):
            ob = np.asarray(obstacles, dtype=np.float64)
            if per_ego is None:
                per_ego = ob.ndim == 4
            if per_ego:
                if ob.ndim == 3:
                    ob = np.repeat(ob[:, :, None, :], L, axis=2)
                if ob.ndim != 4 or ob.shape[0] != B or ob.shape[2] < L or ob.shape[3] != 5:
                    raise MpcError(_abi.MPC_ERR_INVALID, f"per-ego obstacles must be [B = {B}, n, L >= {L}, 5]")
                ob = _abi.f64(ob[:, :, :L])
                n_obst = ob.shape[1]
            else:
                if ob.ndim == 2:
                    ob = np.repeat(ob[:, None, :], L, axis=1)
                ob = _abi.f64(ob[:, :L])
                n_obst = ob.shape[0]
        lf = None if left is None else _abi.f64(left).reshape(-1, 2)
        rt = None if right is None else _abi.f64(right).reshape(-1, 2)
        fc, fo = np.empty(B, np.int32), np.empty(B, np.int32)
        fn = self._lib.mpc_validity_batch_ego if per_ego and n_obst else self._lib.mpc_validity_batch
        self._check(fn(self._h, B, L, _abi.as_dp(traj), float(ego_length), float(ego_width), n_obst, _abi.as_dp(ob),
                       0 if lf is None else lf.shape[0], _abi.as_dp(lf), 0 if rt is None else rt.shape[0], _abi.as_dp(rt),
                       _abi.as_ip(fc), _abi.as_ip(fo)))
        return dict(first_collision=fc, first_off_road=fo)

    def forces_stage_eval(self, z, p, terminal=False):
        """FORCES-mode stage functions of B (z, p) pairs on the device (mpc_forces_stage_eval; the generated
        FORCESNLPsolver_model.c of the reference): dict(f, grad_f, c, jac_c, h, jac_h); c / jac_c are None at the last stage."""
        z = _abi.f64(z).reshape(-1, 7)
        p = _abi.f64(p).reshape(-1, 10)
        B = z.shape[0]
        f, gf = np.empty(B), np.empty((B, 7))
        c, jc = (None, None) if terminal else (np.empty((B, 5)), np.empty((B, 5, 7)))
        hv, jh = np.empty((B, 10)), np.empty((B, 10, 7))
        self._check(self._lib.mpc_forces_stage_eval(self._h, B, 1 if terminal else 0, _abi.as_dp(z), _abi.as_dp(p), _abi.as_dp(f),
                                                    _abi.as_dp(gf), _abi.as_dp(c), _abi.as_dp(jc), _abi.as_dp(hv), _abi.as_dp(jh)))
        return dict(f=f, grad_f=gf, c=c, jac_c=jc, h=hv, jac_h=jh)

    def forces_solve(self, x0, xinit, all_parameters, lb, ub, hl, hu, hessian_mode=0):
        """FORCES-mode SQP step for B problems (mpc_forces_solve_batch): x0 [B,N,7], xinit [B,5], all_parameters [B,N,10]
        -> (x [B,N,7], exitflag [B], it [B], res [B])."""
        N = self.N
        x0 = _abi.f64(x0).reshape(-1, N, 7)
        B = x0.shape[0]
        xinit = _abi.f64(xinit).reshape(B, 5)
        par = _abi.f64(all_parameters).reshape(B, N, 10)

        out = np.empty_like(x0)
        flag, it, res = np.empty(B, np.int32), np.empty(B, np.int32), np.empty(B)
        self._check(self._lib.mpc_forces_solve_batch(self._h, B, _abi.as_dp(x0), _abi.as_dp(xinit), _abi.as_dp(par), _abi.as_dp(_big(lb, 7)),
                                                     _abi.as_dp(_big(ub, 7)), _abi.as_dp(_big(hl, 10)), _abi.as_dp(_big(hu, 10)), int(hessian_mode), _abi.as_dp(out),
                                                     _abi.as_ip(flag), _abi.as_ip(it), _abi.as_dp(res)))
        return out, flag, it, res

    def forces_solve_device(self, B, d_x0, d_xinit, d_par, lb, ub, hl, hu, d_x_out, d_flag=0, d_it=0, d_res=0, hessian_mode=0, stream=0):
        """mpc_forces_solve_batch_dev: device pointers (ints) for x0 [B,N,7], xinit [B,5], all_parameters [B,N,10] and the outputs;
        lb / ub / hl / hu are small host arrays.  Enqueues on `stream`; nothing is synchronised."""
        self._check(self._lib.mpc_forces_solve_batch_dev(self._h, int(B), _vp(d_x0), _vp(d_xinit), _vp(d_par), _abi.as_dp(_big(lb, 7)), _abi.as_dp(_big(ub, 7)),
                                                         _abi.as_dp(_big(hl, 10)), _abi.as_dp(_big(hu, 10)), int(hessian_mode), _vp(d_x_out), _vp(d_flag),
                                                         _vp(d_it), _vp(d_res), _vp(stream)))

    def forces_closed_loop(self, init_state, path, orient, vdes, steps, lb, ub, hl, hu, init_acc=None, hessian_mode=0, noise_mode=0, sigma=0.0, seed=0):
        """B egos through `steps` steps of ForcesproOptimizer.optimize (optimizer.py:246-366) on the device
        (mpc_forces_closed_loop_batch): init_state [B,5], path [B,Lp,2], orient [B,Lp], vdes [B] -> (traj [B,steps,5],
        ctrl [B,steps,2], exitflag [B,steps])."""
        init_state, path, orient, vdes, B, Lp = _loop_in(init_state, path, orient, vdes)
        acc = None if init_acc is None else _abi.f64(np.broadcast_to(np.asarray(init_acc, dtype=np.float64), (B,)))
        steps = int(steps)
        traj, ctrl, fl = np.empty((B, steps, 5)), np.empty((B, steps, 2)), np.empty((B, steps), np.int32)
        self._check(self._lib.mpc_forces_closed_loop_batch(self._h, B, steps, Lp, _abi.as_dp(init_state), _abi.as_dp(acc), _abi.as_dp(path), _abi.as_dp(orient),
                                                           _abi.as_dp(vdes), _abi.as_dp(_big(lb, 7)), _abi.as_dp(_big(ub, 7)), _abi.as_dp(_big(hl, 10)),
                                                           _abi.as_dp(_big(hu, 10)), int(hessian_mode), int(noise_mode), float(sigma), int(seed) & (2 ** 64 - 1),
                                                           _abi.as_dp(traj), _abi.as_dp(ctrl), _abi.as_ip(fl)))
        return traj, ctrl, fl

    def forces_closed_loop_obst(self, init_state, path, orient, vdes, steps, lb, ub, hl, hu, obst_track=None, obst_offset=0.0, predict=False, guess_mode=0,
                                r_sum=None, clearance=None, init_acc=None, hessian_mode=0, noise_mode=0, sigma=0.0, seed=0):
        """forces_closed_loop past per-ego obstacles that move, with a guess that may follow the plan (mpc_forces_closed_loop_batch_obst).
        obst_track [B,Lt,3] (or [B,3]: one standing pose per ego) = (x, y, heading) of ego b's obstacle at step i, Lt = 1 or >= steps; None: the
        handle's obstacle in every stage.  predict: stage j of step k sees pose min(k + j, Lt - 1) instead of min(k, Lt - 1).  guess_mode 1: the
        guess of the next solve is the solution shifted by one stage after exitflag 1, left alone otherwise.  r_sum: sum of the circle radii
        (None: sqrt(hl[1]), the bound of the squared circle distances).  clearance: None = with a track.
        -> (traj [B,steps,5], ctrl [B,steps,2], exitflag [B,steps], clearance [B,steps] | None): clearance[b, i] = min over the nine circle pairs of
        distance - r_sum of traj[b, i] against the pose at step i."""
        init_state, path, orient, vdes, B, Lp = _loop_in(init_state, path, orient, vdes)
        acc = None if init_acc is None else _abi.f64(np.broadcast_to(np.asarray(init_acc, dtype=np.float64), (B,)))
        steps = int(steps)
        Lt = 0
        if obst_track is not None:
            obst_track = _abi.f64(obst_track)
            if obst_track.ndim == 2:
                obst_track = obst_track[:, None, :]
            if obst_track.ndim != 3 or obst_track.shape[0] != B or obst_track.shape[2] != 3:
                raise MpcError(_abi.MPC_ERR_INVALID, f"obst_track must be [B = {B}, Lt, 3]")
            obst_track = _abi.f64(obst_track)
            Lt = obst_track.shape[1]
        if clearance is None:
            clearance = obst_track is not None
        if r_sum is None:
            r_sum = float(np.sqrt(np.asarray(hl, dtype=np.float64).ravel()[1]))
        traj, ctrl, fl = np.empty((B, steps, 5)), np.empty((B, steps, 2)), np.empty((B, steps), np.int32)
        cl = np.empty((B, steps)) if clearance else None
        self._check(self._lib.mpc_forces_closed_loop_batch_obst(self._h, B, steps, Lp, _abi.as_dp(init_state), _abi.as_dp(acc), _abi.as_dp(path), _abi.as_dp(orient),
                                                                _abi.as_dp(vdes), _abi.as_dp(_big(lb, 7)), _abi.as_dp(_big(ub, 7)), _abi.as_dp(_big(hl, 10)),
                                                                _abi.as_dp(_big(hu, 10)), int(hessian_mode), int(guess_mode), Lt, _abi.as_dp(obst_track),
                                                                float(obst_offset), 1 if predict else 0, float(r_sum), int(noise_mode), float(sigma),
                                                                int(seed) & (2 ** 64 - 1), _abi.as_dp(traj), _abi.as_dp(ctrl), _abi.as_ip(fl), _abi.as_dp(cl)))
        return traj, ctrl, fl, cl

    def forces_closed_loop_obst_device(self, B, steps, Lp, d_init_state, d_path, d_orient, d_vdes, lb, ub, hl, hu, d_traj, d_ctrl, d_step_flag=0, d_init_acc=0,
                                       hessian_mode=0, guess_mode=0, Lt=0, d_obst_track=0, obst_offset=0.0, predict=False, r_sum=0.0, d_clearance=0,
                                       noise_mode=0, sigma=0.0, seed=0, stream=0):
        """mpc_forces_closed_loop_batch_obst_dev: device pointers (ints; 0 = absent) for the rows, lb / ub / hl / hu small host arrays.  Enqueues the
        whole loop on `stream`; nothing is synchronised."""
        self._check(self._lib.mpc_forces_closed_loop_batch_obst_dev(self._h, int(B), int(steps), int(Lp), _vp(d_init_state), _vp(d_init_acc), _vp(d_path), _vp(d_orient),
                                                                    _vp(d_vdes), _abi.as_dp(_big(lb, 7)), _abi.as_dp(_big(ub, 7)), _abi.as_dp(_big(hl, 10)),
                                                                    _abi.as_dp(_big(hu, 10)), int(hessian_mode), int(guess_mode), int(Lt), _vp(d_obst_track),
                                                                    float(obst_offset), 1 if predict else 0, float(r_sum), int(noise_mode), float(sigma),
                                                                    int(seed) & (2 ** 64 - 1), _vp(d_traj), _vp(d_ctrl), _vp(d_step_flag), _vp(d_clearance), _vp(stream)))

    def set_option(self, name, value=None):
        """run-time switch of the handle (include/mpcgpu.h: mpc_set_option); value None restores the default.  The
        environment (MPCGPU_<NAME>) is only read when the handle is created."""
        v = None if value is None else str(value).encode()
        self._check(self._lib.mpc_set_option(self._h, str(name).encode(), v))

    def get_option(self, name):
        """current value of a run-time switch (include/mpcgpu.h: mpc_get_option)"""
        v = C.c_int64(0)
        self._check(self._lib.mpc_get_option(self._h, str(name).encode(), C.byref(v)))
        return int(v.value)

    def set_profiling(self, enable=True):
        """True / 1: HIP events around every kernel; 2: the iteration loop of a hybrid solve as one span (no marker between its two kernels)."""
        self._check(self._lib.mpc_set_profiling(self._h, int(enable) if enable in (0, 1, 2) else (1 if enable else 0)))

    def get_profile(self):
        out = np.zeros(6)
        self._check(self._lib.mpc_get_profile(self._h, _abi.as_dp(out)))
        return dict(riccati_ms=out[0], riccati_launches=int(out[1]), stage_ms=out[2], stage_launches=int(out[3]),
                    other_ms=out[4], iterations=int(out[5]))

    def get_resident_profile(self):
        """Figures of the workgroup-resident kernel of the last solve (k_solve_wg: finishes the instances of the tiles that left the
        pipeline -- the hybrid solve -- or solves a small batch alone); `ran` is False when only streaming paths ran.
        `instance_iterations`: interior-point iterations it performed (the others ran in the pipeline)."""
        out = np.zeros(8)
        self._check(self._lib.mpc_get_resident_profile(self._h, _abi.as_dp(out)))
        return dict(ms=out[0], ran=bool(out[1]), rounds=int(out[2]), workgroups=int(out[3]), workgroup_rounds=int(out[4]), sweeps=int(out[5]),
                    instance_iterations=int(out[6]))

    def measure_copy_bandwidth(self, nbytes=1 << 30, reps=5):
        """GB/s (read + write) of the library's own streaming copy kernel on this device (roofline denominator of bench.py)"""
        out = np.zeros(1)
        self._check(self._lib.mpc_measure_copy_bandwidth(self._h, nbytes, reps, _abi.as_dp(out)))
        return float(out[0])

    def get_pipeline_profile(self):
        """Figures of the single-launch pipeline (k_pipeline) for the last solve; `ran` is False when the solve used one
        launch per kernel instead (small or very large batches, MPCGPU_PIPELINE=0)."""
        out = np.zeros(8)
        self._check(self._lib.mpc_get_pipeline_profile(self._h, _abi.as_dp(out)))
        return dict(ms=out[0], ran=bool(out[1]), rounds=int(out[2]), riccati_wait_ms=out[3], stage_wait_ms=out[4],
                    stage_busy_ms=out[5], items=int(out[6]), stage_workers=int(out[7]), riccati_workers=int(round((out[7] % 1) * 1000)))


class LoopSession:
    """The closed loop stepped from outside (include/mpcgpu.h, mpc_session_*): the caller owns the plant and the perception.

        with solver.session(init_state, path, orient, vdes, steps, offsets) as sess:
            u = sess.step(obstacles=obs0)                       # step 0: init_state is the measurement
            while sess.steps_done < steps:
                u = sess.step(measured, obstacles)              # measured [B, 5] (NaN x: dropped), obstacles [M, 5] / [B, M, 5]
            traj, ctrl, status = sess.record()

    A caller with a prediction module hands over trajectories instead of velocities, sess.step(measured, predicted=pred) with pred [M, N+1, 3] /
    [B, M, N+1, 3] (mpc_session_step_pred); the two kinds of step may alternate.  rsums (shaped like offsets): a radius sum per obstacle
    (mpc_session_begin_sized).  Between two steps the solver may be used for anything else; set_weights / set_bounds take effect at the next step."""

    OUTPUTS = ("plan", "status", "clearance", "nearest", "chosen")

    def __init__(self, solver, init_state, path, orient, vdes, steps, offsets=None, per_ego=None, pairing=0, rsums=None):
        self._s = solver
        init_state, path, orient, vdes, B, Lp = _loop_in(init_state, path, orient, vdes)
        self.B, self.steps, self.M, self.per_ego = B, int(steps), 0, 0
        if offsets is not None:
            offsets = _abi.f64(offsets)
            self.per_ego = int(offsets.ndim == 2) if per_ego is None else int(per_ego)
            if offsets.ndim not in (1, 2) or (self.per_ego == 1 and offsets.shape[0] != B):
                raise MpcError(_abi.MPC_ERR_INVALID, "offsets must be [M], or [B, M] for obstacles per ego")
            self.M = offsets.shape[-1]
        if rsums is not None:
            rsums = _abi.f64(rsums)
            if offsets is None or rsums.shape != offsets.shape:
                raise MpcError(_abi.MPC_ERR_INVALID, "rsums must have the shape of offsets")
            rsums = rsums.reshape(-1)
        if offsets is not None:
            offsets = offsets.reshape(-1)
        self.sized = rsums is not None
        self._open = False
        head = (solver._h, B, self.steps, Lp, _abi.as_dp(init_state), _abi.as_dp(path), _abi.as_dp(orient), _abi.as_dp(vdes), self.M, self.per_ego,
                _abi.as_dp(offsets))
        if rsums is None:
            solver._check(solver._lib.mpc_session_begin(*head, int(pairing)))
        else:
            solver._check(solver._lib.mpc_session_begin_sized(*head, _abi.as_dp(rsums), int(pairing)))
        self._open = True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if self._open:
            self._open = False
            self._s._check(self._s._lib.mpc_session_end(self._s._h))

    @property
    def steps_done(self):
        """the index of the next step (mpc_session_steps_done)"""
        return int(self._s._lib.mpc_session_steps_done(self._s._h))

    def step(self, measured=None, obstacles=None, predicted=None, outputs=()):
        """one step (mpc_session_step) -> u [B, 2], the control to apply; with outputs, a tuple of names out of OUTPUTS, -> (u, *those arrays):
        plan [B, n_w] the solution, status [B], and with obstacles this step's clearance [B], nearest [B], chosen [B, N+1, 3].
        measured [B, 5]: the plant's state now (None: the model's own prediction; None at step 0); obstacles [M, 5] or [B, M, 5]: (x, y, heading, vx, vy)
        now, NaN x: absent.  predicted [M, N+1, 3] or [B, M, N+1, 3] in the place of obstacles (mpc_session_step_pred): (x, y, heading) of obstacle m
        as stage k is to see it, row 0 its pose now, NaN x: absent at that stage"""
        s, B = self._s, self.B
        if obstacles is not None and predicted is not None:
            raise MpcError(_abi.MPC_ERR_INVALID, "a step takes obstacles (observed poses and velocities) or predicted (poses per stage), not both")
        unknown = [o for o in outputs if o not in self.OUTPUTS]
        if unknown:
            raise MpcError(_abi.MPC_ERR_INVALID, f"outputs: {unknown} not in {self.OUTPUTS}")
        if measured is not None:
            measured = _abi.f64(measured, (B, 5))
        if obstacles is not None:
            obstacles = _abi.f64(obstacles, ((B,) if self.per_ego else ()) + (self.M, 5))
        if predicted is not None:
            predicted = _abi.f64(predicted, ((B,) if self.per_ego else ()) + (self.M, s.N + 1, 3))
        out = dict(plan=np.empty((B, s.n_w)), status=np.empty(B, np.int32), clearance=np.empty(B), nearest=np.empty(B, np.int32),
                   chosen=np.empty((B, s.N + 1, 3), np.int32))
        out = {k: (v if k in outputs else None) for k, v in out.items()}
        u = np.empty((B, 2))
        s._sens_gen += 1                                     # (a step is a solve: the library has ended the life of an earlier snapshot)
        tail = (_abi.as_dp(u), _abi.as_dp(out["plan"]), _abi.as_ip(out["status"]), _abi.as_dp(out["clearance"]), _abi.as_ip(out["nearest"]),
                _abi.as_ip(out["chosen"]))
        if predicted is None:
            s._check(s._lib.mpc_session_step(s._h, _abi.as_dp(measured), _abi.as_dp(obstacles), *tail))
        else:
            s._check(s._lib.mpc_session_step_pred(s._h, _abi.as_dp(measured), _abi.as_dp(predicted), *tail))
        return (u, *[out[o] for o in outputs]) if outputs else u

    def step_device(self, d_u, d_measured=0, d_obs=0, d_plan=0, d_status=0, d_clearance=0, d_nearest=0, d_chosen=0, stream=0, d_pred=0):
        """device-pointer form (ints; 0 = absent) of step (mpc_session_step_dev): enqueued on `stream`, the solve synchronises it.  d_pred in the
        place of d_obs: mpc_session_step_pred_dev"""
        s = self._s
        if d_obs and d_pred:
            raise MpcError(_abi.MPC_ERR_INVALID, "a step takes d_obs or d_pred, not both")
        s._sens_gen += 1
        tail = (_vp(d_u), _vp(d_plan), _vp(d_status), _vp(d_clearance), _vp(d_nearest), _vp(d_chosen), _vp(stream))
        if d_pred:
            s._check(s._lib.mpc_session_step_pred_dev(s._h, _vp(d_measured), _vp(d_pred), *tail))
        else:
            s._check(s._lib.mpc_session_step_dev(s._h, _vp(d_measured), _vp(d_obs), *tail))

    def record(self):
        """(traj [B, steps, 5], ctrl [B, steps, 2], step_status [B, steps]) as recorded so far (mpc_session_record); steps not yet taken: NaN / 0"""
        traj, ctrl, st = np.empty((self.B, self.steps, 5)), np.empty((self.B, self.steps, 2)), np.empty((self.B, self.steps), np.int32)
        self._s._check(self._s._lib.mpc_session_record(self._s._h, _abi.as_dp(traj), _abi.as_dp(ctrl), _abi.as_ip(st)))
        return traj, ctrl, st


def rescue_failed(backend, x0, p, result, bounds, fractions=RESCUE_FRACTIONS):
    """Second chance for the instances of a batch that did not converge (status != 1), by homotopy on the obstacle radius.

    IPOPT hands a start that is locally infeasible -- typically a guess that runs straight through the obstacle, where
    the linearised circle constraints cannot be met within the fraction-to-the-boundary rule -- to its restoration phase,
    which is not restated here.  Instead the failed instances are re-solved on the device with the
    lower bound of the circle-distance rows (`lbg` of the 9 (N+1) obstacle rows, optimizer.py:426-428) raised in steps
    from 0 to its true value, each solve warm-started from the previous solution; the last solve is the ORIGINAL NLP, so
    what comes back is a KKT point of the original problem to the original tolerance, or the original failure.

    backend: anything with set_bounds(lbx, ubx, lbg, ubg) and solve(x0, p) -> SolveResult (the BatchedMPCSolver).
    bounds: the (lbx, ubx, lbg, ubg) of the original problem.  Returns (result, rescued mask)."""
    status = np.asarray(result.status)
    bad = np.nonzero(status != 1)[0]
    rescued = np.zeros(status.shape[0], dtype=bool)
    if bad.size == 0:
        return result, rescued
    lbx, ubx, lbg, ubg = [np.asarray(a, dtype=np.float64).ravel().copy() for a in bounds]
    n_obst = 9 * (int(backend.N) + 1) if hasattr(backend, "N") else 9 * ((lbg.size - 1) // 14)
    xs = np.asarray(x0, dtype=np.float64)[bad].copy()
    ps = np.asarray(p, dtype=np.float64)[bad]
    iters = np.zeros(bad.size, dtype=np.int64)
    last = None
    try:
        for frac in fractions:
            lbg_f = lbg.copy()
            lbg_f[-n_obst:] = frac * lbg[-n_obst:]
            backend.set_bounds(lbx, ubx, lbg_f, ubg)
            last = backend.solve(xs, ps)
            ok = np.asarray(last.status) == 1
            xs[ok] = np.asarray(last.x)[ok]                       # warm start of the next, tighter problem
            iters += np.asarray(last.iters)
    finally:
        backend.set_bounds(lbx, ubx, lbg, ubg)
    ok = np.asarray(last.status) == 1
    x, st, it, kkt = [np.array(a, copy=True) for a in (result.x, result.status, result.iters, result.kkt)]
    sel = bad[ok]
    x[sel], st[sel], kkt[sel] = np.asarray(last.x)[ok], 1, np.asarray(last.kkt)[ok]
    it[sel] = it[sel] + iters[ok]
    rescued[sel] = True
    return SolveResult(x, st, it, kkt), rescued


__all__ = ["BatchedMPCSolver", "SolveResult", "LoopLin", "MpcError", "MpcLibraryError", "rescue_failed", "RESCUE_FRACTIONS"]
