"""
Host-side mirror of the reference's `MPC_Planner/optimizer.py` call surface, backed by the HIP solver.

What is mirrored (same names, argument meaning, return shapes, and the behaviour-defining quirks of SURVEY.md
App. C), so that `mpc_planner.py:301-309` works unchanged against this module:

    CasadiOptimizer(configuration=, init_values=, predict_horizon=)        optimizer.py:369-371
        .inequal_constraints() -> lbg, ubg, lbx, ubx                        optimizer.py:413-491
        .solver() -> (sol, f)                                               optimizer.py:513-560
              sol(x0=, p=, lbg=, lbx=, ubg=, ubx=)['x'].full()              optimizer.py:607-609
              f(x, u).full()                                                optimizer.py:649-650
        .optimize() -> (states[L,5], controls[L,2], solve_time[L])          optimizer.py:562-643
        .shift_movement(...), .desired_command_and_trajectory(...)          optimizer.py:645-702
    ForcesproOptimizer(...)  -- call surface of `solver.solve(problem)`     optimizer.py:197-366

The reference rebuilds the CasADi graph and the IPOPT object on every MPC step (optimizer.py:605); here
`solver()` returns a cached handle to the device workspace.  All NLP arithmetic runs in csrc/mpcgpu.hip through
the C-ABI of include/mpcgpu.h; this file only packs arguments.  `ca` below is a tiny numeric stand-in for the
three CasADi functions that `mpc_planner.py` reaches through its star import (mpc_planner.py:288-290).
"""
from __future__ import annotations

import math
import time
import types

import numpy as np

from . import noise as _noise
from .solver import BatchedMPCSolver, rescue_failed

# ------------------------------------------------------------------------------------------------------------
# numeric stand-ins for names the reference's planner pulls in via `from MPC_Planner.optimizer import *`
# ------------------------------------------------------------------------------------------------------------
ca = types.SimpleNamespace(
    sqrt=np.sqrt,
    vertcat=lambda *a: np.concatenate([np.atleast_1d(np.asarray(x, dtype=np.float64)).ravel() for x in a]).reshape(-1, 1),
    reshape=lambda a, r, c: DMLike(np.asarray(a.full() if hasattr(a, "full") else a, dtype=np.float64).reshape((r, c), order="F")),
    cos=np.cos, sin=np.sin, tan=np.tan,
)


class DMLike:
    """the two things the reference does with a casadi.DM: `.full()` and reshaping."""

    def __init__(self, a):
        self._a = np.array(a, dtype=np.float64)

    def full(self):
        return self._a.copy()

    def __array__(self, dtype=None, copy=None):
        return self._a if dtype is None else self._a.astype(dtype)

    @property
    def shape(self):
        return self._a.shape


def find_closest_point(path_points, current_point):
    """configuration.py:26-37."""
    diff = np.transpose(np.transpose(path_points) - current_point.reshape(2, 1))
    squared_dist = np.power(diff, 2)[:, 0] + np.power(diff, 2)[:, 1]
    return np.argmin(squared_dist)


def compute_approximating_circle_radius(ego_length, ego_width):
    """configuration.py:40-66 (radius rounding rule included)."""
    assert ego_length >= 0 and ego_width >= 0, "Invalid vehicle dimensions = {}".format([ego_length, ego_width])
    if np.isclose(ego_length, 0.0) and np.isclose(ego_width, 0.0):
        return 0.0, 0.0
    square_length = ego_length / 3
    diagonal_square = np.sqrt((square_length / 2) ** 2 + (ego_width / 2) ** 2)
    if diagonal_square > round(diagonal_square, 1):
        approx_radius = round(diagonal_square, 1) + 0.1
    else:
        approx_radius = round(diagonal_square, 1)
    return approx_radius, round(square_length * 2, 1)


def compute_centers_of_approximation_circles(x_position, y_position, v_length, v_width, orientation):
    """configuration.py:69-93: centre, front and rear circle centres."""
    _, disc_distance = compute_approximating_circle_radius(v_length, v_width)
    distance_centers = disc_distance / 2
    center = [x_position, y_position]
    center_fw = [x_position + (distance_centers / 2) * np.cos(orientation), y_position + (distance_centers / 2) * np.sin(orientation)]
    center_rw = [x_position - (distance_centers / 2) * np.cos(orientation), y_position - (distance_centers / 2) * np.sin(orientation)]
    return center, center_fw, center_rw


def nearest_obstacle_centres(poses, tracks, offsets, rows, ego_offset, pairing, default, rsums=None, r_default=None):
    """The selection of the loop through traffic (csrc/mpc_closed_loop.h, loop_traffic_stage; include/mpcgpu.h, mpc_closed_loop_batch_traffic) for one
    ego, in numpy: poses [K, 3] = predicted (x, y, psi) of the K stages, tracks [M, Lt, 3] (NaN x: absent), offsets [M], rows [K] = the track row every
    stage sees, default [6] = the centres of a stage that sees no obstacle -> (centres [K, 6], chosen [K, 3]; -1: none).
    pairing 0: the present obstacle with the smallest min_j |E_j - O_{m,j}| gives all three centres; 1: slot j is the circle nearest to ego circle j
    over all present obstacles and circles.  Ties go to the lowest obstacle, then the lowest circle.
    rsums [M] (optional; with r_default, the handle's radius sum): obstacles of their own sizes -- the selection is by CLEARANCE, every distance
    above less delta_m = rsums[m] - r_default, and a third value comes back: radii [K, 3], the winner's rsums[m] per slot (r_default where
    nothing is present) -- obst [K, 6] and rsum [K, 3] of one instance of BatchedMPCSolver.solve(..., rsum=).  With every rsums[m] equal to
    r_default the centres and `chosen` are those of the call without it."""
    def circles(x, y, th, off):
        return np.array([[x, y], [x + off * np.cos(th), y + off * np.sin(th)], [x - off * np.cos(th), y - off * np.sin(th)]])
    K = len(poses)
    out, chosen = np.tile(np.asarray(default, dtype=np.float64), (K, 1)).reshape(K, 3, 2), np.full((K, 3), -1, dtype=np.int32)
    sized = rsums is not None
    if sized and r_default is None:
        raise ValueError("nearest_obstacle_centres: rsums needs r_default, the radius sum of a stage that sees no obstacle")
    delta = np.asarray(rsums, dtype=np.float64) - r_default if sized else np.zeros(len(tracks))
    radii = np.full((K, 3), r_default if sized else np.nan)
    for k in range(K):
        E = circles(poses[k][0], poses[k][1], poses[k][2], ego_offset)
        best = np.full(3, np.inf)
        for m in range(len(tracks)):
            x, y, th = tracks[m][rows[k]]
            if not np.isfinite(x):
                continue
            O = circles(x, y, th, offsets[m])
            if pairing == 0:
                score = min(np.hypot(*(E[j] - O[j])) for j in range(3)) - delta[m]
                if chosen[k, 0] < 0 or score < best[0]:
                    best[0], chosen[k], out[k] = score, m, O
                    if sized:
                        radii[k] = rsums[m]
            else:
                for j in range(3):
                    for c in range(3):
                        dist = np.hypot(*(E[j] - O[c])) - delta[m]
                        if chosen[k, j] < 0 or dist < best[j]:
                            best[j], chosen[k, j], out[k, j] = dist, m, O[c]
                            if sized:
                                radii[k, j] = rsums[m]
    return (out.reshape(K, 6), chosen, radii) if sized else (out.reshape(K, 6), chosen)


class VehicleDynamics:
    """configuration.py:342-368 (kinematic single track); l = a + b of parameters_vehicle2."""
    l = 2.5789128

    @classmethod
    def KS_casadi(cls, x, u):
        x = np.asarray(x, dtype=np.float64).ravel()
        u = np.asarray(u, dtype=np.float64).ravel()
        return np.array([x[3] * math.cos(x[4]), x[3] * math.sin(x[4]), u[0], u[1], x[3] / cls.l * math.tan(x[2])])


class _DynamicsFunction:
    """`f = ca.Function('f', [states, controls], [rhs])` look-alike (optimizer.py:537): f(x, u).full() -> (5,1)."""

    def __call__(self, x, u):
        return DMLike(VehicleDynamics.KS_casadi(x, u).reshape(-1, 1))


class NlpSolution(dict):
    """what `sol(...)` returns: res['x'].full() is the optimal decision vector (optimizer.py:609)."""


class NlpSolverHandle:
    """`ca.nlpsol('solver', 'ipopt', nlp_prob, opts)` look-alike (optimizer.py:558): callable with the same
    keyword arguments as optimizer.py:607.  Accepts a single instance ((n_w,1) / (n_w,)) or a batch [B, n_w].

    The result has CasADi's keys: 'x' (n_w,1), 'f' (1,1), 'g' and 'lam_g' (n_g,1), 'lam_x' and 'lam_p' (n_w,1) -- rows [B, .] for a batch;
    lam_g / lam_x / lam_p are NaN for an instance whose status is not 1 (include/mpcgpu.h, mpc_solve_batch_ex; lam_p = d/dp [f + lam_g' g +
    lam_x' x], the closed form of BatchedMPCSolver.lam_p_of).  'f', 'g', 'lam_*' come with a BatchedMPCSolver backend only.  A dual warm start (lam_x0 / lam_g0) is not
    taken: those keywords are accepted and ignored."""

    # failed instances get a second chance by homotopy on the obstacle radius: on the device, behind the C-ABI
    # (mpc_solve_batch; include/mpcgpu.h).  A backend without that (the stand-in backends of the tests) gets the same
    # procedure from solver.rescue_failed.
    rescue = True

    def __init__(self, backend: BatchedMPCSolver):
        self._backend = backend
        self._stats = {}

    def __call__(self, x0=None, p=None, lbg=None, lbx=None, ubg=None, ubx=None, obst=None, rsum=None, **_unused):
        """obst (not a CasADi keyword): circle centres [6] / [B, 6] of this solve's obstacle instead of the template's, or [N+1, 6] / [B, N+1, 6]:
        centres per stage (BatchedMPCSolver.solve); rsum (with centres per stage): [N+1, 3] / [B, N+1, 3], a radius sum per circle row"""
        be = self._backend
        x0a = np.asarray(x0.full() if hasattr(x0, "full") else x0, dtype=np.float64)
        pa = np.asarray(p.full() if hasattr(p, "full") else p, dtype=np.float64)
        # a batch is [B, n_w]; the reference's own column vector is (n_w, 1) (optimizer.py:602) -- B == n_w is a batch too
        batched = x0a.ndim == 2 and x0a.shape[1] == be.n_w and x0a.shape != (be.n_w, 1)
        if not batched:
            x0a = x0a.reshape(1, -1)
            pa = pa.reshape(1, -1)
        if lbg is not None or lbx is not None or ubg is not None or ubx is not None:
            be.set_bounds(lbx, ubx, lbg, ubg)
        full = isinstance(be, BatchedMPCSolver)
        kw = {}
        if obst is not None:
            oa = np.asarray(obst, dtype=np.float64)
            kw = dict(obst=oa.reshape(x0a.shape[0], 6) if oa.size == 6 * x0a.shape[0] else oa.reshape(x0a.shape[0], -1, 6))
            if rsum is not None:
                kw["rsum"] = np.asarray(rsum, dtype=np.float64).reshape(x0a.shape[0], -1, 3)
        res = be.solve(x0a, pa, multipliers=True, **kw) if full else be.solve(x0a, pa, **kw)
        rescued = np.zeros(res.status.shape[0], dtype=bool)
        n_rescued = int(be.last_rescued()) if hasattr(be, "last_rescued") else 0      # the second chance behind the C-ABI (a count, not a mask)
        if (self.rescue and not isinstance(be, BatchedMPCSolver) and not np.all(res.status == 1) and lbg is not None and lbx is not None
                and ubg is not None and ubx is not None):
            res, rescued = rescue_failed(be, x0a, pa, res, (lbx, ubx, lbg, ubg))      # stands in for IPOPT's restoration phase
        self._stats = dict(status=res.status.copy(), iter_count=res.iters.copy(), kkt=res.kkt.copy(), rescued=rescued, n_rescued=n_rescued + int(rescued.sum()),
                           success=bool(np.all(res.status == 1)),
                           return_status="Solve_Succeeded" if np.all(res.status == 1) else "Not_Converged")
        x = res.x if batched else res.x.reshape(-1, 1)
        out = NlpSolution(x=DMLike(x))
        if full:
            res.lam_p = be.lam_p_of(res.x, pa, res.lam_g, res.status)
            if batched:
                out["f"], out["g"], out["lam_g"], out["lam_x"], out["lam_p"] = (DMLike(a) for a in (res.f, res.g, res.lam_g, res.lam_x, res.lam_p))
            else:
                out["f"] = DMLike(res.f.reshape(1, 1))
                out["g"], out["lam_g"], out["lam_x"], out["lam_p"] = (DMLike(a.reshape(-1, 1)) for a in (res.g, res.lam_g, res.lam_x, res.lam_p))
        out["status"] = res.status
        return out

    def stats(self):
        return dict(self._stats)


class Optimizer(object):
    """optimizer.py:33-83 -- pulls limits, weights, obstacle circles out of the planning configuration."""

    def __init__(self, configuration, init_values, predict_horizon):
        self.configuration = configuration
        self.delta_min = configuration.p.steering.min
        self.delta_max = configuration.p.steering.max
        self.deltav_min = configuration.p.steering.v_min
        self.deltav_max = configuration.p.steering.v_max
        self.v_min = 0
        self.v_max = configuration.p.longitudinal.v_max
        self.a_max = configuration.p.longitudinal.a_max
        self.init_position, self.init_velocity, self.init_acceleration, self.init_orientation = \
            init_values[0], init_values[1], init_values[2], init_values[3]
        self.iter_length = configuration.iter_length
        self.delta_t = configuration.delta_t
        self.desired_velocity = configuration.desired_velocity
        self.resampled_path_points = configuration.reference_path
        self.orientation = configuration.orientation
        self.predict_horizon = predict_horizon
        self.weights_setting = configuration.weights_setting
        so = configuration.static_obstacle
        self.obstacle_circles_centers_tuple = compute_centers_of_approximation_circles(
            so["position_x"], so["position_y"], so["length"], so["width"], so["orientation"])
        self.radius_obstacle, _ = compute_approximating_circle_radius(so["length"], so["width"])
        self.radius_ego, _ = compute_approximating_circle_radius(configuration.p.l, configuration.p.w)
        # optional (not in the reference): the obstacle's pose (x, y, heading) at every loop step, [L, 3]; its length and width stay static_obstacle's
        track = getattr(configuration, "obstacle_track", None)
        self.obstacle_track = None if track is None else np.asarray(track, dtype=np.float64).reshape(-1, 3)
        _, disc_distance = compute_approximating_circle_radius(so["length"], so["width"])
        self.obstacle_offset = (disc_distance / 2) / 2
        # optional (not in the reference): traffic.  obstacle_tracks [M, L, 3] = the pose of M obstacles at every loop step (NaN x: absent at that step),
        # obstacle_sizes [M, 2] = their lengths and widths; obstacle_pairing 0 / 1 (nearest_obstacle_centres).  Every stage of every solve avoids the
        # obstacle nearest to it (mpc_closed_loop_batch_traffic).  The circle centres of obstacle m lie +- disc_distance / 4 of ITS rectangle along its
        # heading; by default ONE radius: the lower bound of the circle rows (lbg) is that of the LARGEST obstacle, held against all of them (obstacle_radii below).
        # `obstacle_sizes` without tracks: what open_session() needs -- its caller observes the obstacles step by step and has no tracks to give.
        tracks = getattr(configuration, "obstacle_tracks", None)
        sizes = getattr(configuration, "obstacle_sizes", None)
        self.obstacle_tracks = self.obstacle_offsets = None
        if tracks is not None or sizes is not None:
            sizes = np.asarray(sizes, dtype=np.float64).reshape(-1, 2)
            if tracks is not None:
                self.obstacle_tracks = np.asarray(tracks, dtype=np.float64)
                if self.obstacle_tracks.ndim != 3 or self.obstacle_tracks.shape[2] != 3 or len(sizes) != len(self.obstacle_tracks):
                    raise ValueError("obstacle_tracks must be [M, L, 3] with obstacle_sizes [M, 2]")
            self.obstacle_offsets = np.array([compute_approximating_circle_radius(l, w)[1] / 4 for l, w in sizes])
            self.radius_obstacle = max(compute_approximating_circle_radius(l, w)[0] for l, w in sizes)
            # obstacle_radii (opt-in): "largest", the default -- the one radius above; "own" -- every obstacle with the radius of ITS rectangle: the
            # loops select by clearance and every solve is a sized one (mpc_closed_loop_batch_traffic_sized, BatchedMPCSolver.solve(rsum=)); lbg keeps
            # the largest radius, which a stage that sees no obstacle is held to
            self.obstacle_radii = str(getattr(configuration, "obstacle_radii", "largest"))
            if self.obstacle_radii not in ("largest", "own"):
                raise ValueError('obstacle_radii is "largest" or "own"')
            self.obstacle_rsums = None
            if self.obstacle_radii == "own":
                self.obstacle_rsums = np.array([compute_approximating_circle_radius(l, w)[0] for l, w in sizes]) + self.radius_ego
            self.obstacle_pairing = int(getattr(configuration, "obstacle_pairing", 0))
        self.nearest = self.chosen = None           # optimize() through traffic: the nearest obstacle of every step (device loop), the obstacle behind every slot
        self.clearance = None           # optimize() with a track, device loop: distance - r_sum of every step (include/mpcgpu.h, mpc_closed_loop_batch_obst)

    def obstacle_centers_at(self, step):
        """circle centres [6] of the tracked obstacle at loop step `step` (the last pose once the track ends)"""
        x, y, th = self.obstacle_track[min(step, len(self.obstacle_track) - 1)]
        so = self.configuration.static_obstacle
        return np.array(compute_centers_of_approximation_circles(x, y, so["length"], so["width"], th), dtype=np.float64).ravel()

    def equal_constraints(self, *args, **kwargs):
        pass

    def inequal_constraints(self, *args, **kwargs):
        pass

    def cost_function(self, *args, **kwargs):
        pass

    def solver(self):
        pass

    def optimize(self):
        pass


class CasadiOptimizer(Optimizer):
    """optimizer.py:369-702 with the NLP solved on the GPU.

    Not in the reference: a configuration with `obstacle_tracks` [M, L, 3] (NaN x: absent at that step) and `obstacle_sizes` [M, 2] is driven through
    traffic -- every stage of every solve avoids the obstacle nearest to it (BatchedMPCSolver.closed_loop_traffic; `obstacle_pairing` 0 / 1), on the
    device and, with the same selection in numpy, in the step-by-step host loop.  The circle offsets are each obstacle's own (disc_distance / 4 of
    its rectangle).  By default one radius: the lower bound of the circle rows (lbg) is that of the largest obstacle, held against all of them;
    `obstacle_radii = "own"` plans around every obstacle at its own size (mpc_closed_loop_batch_traffic_sized)."""

    num_states = 5
    num_controls = 2

    def __init__(self, configuration, init_values, predict_horizon, device=0):
        super(CasadiOptimizer, self).__init__(configuration, init_values, predict_horizon)
        self._device = device
        self._sol = None
        self._f = _DynamicsFunction()

    # -- bounds: optimizer.py:413-491 ---------------------------------------------------------------------------
    def inequal_constraints(self):
        N = self.predict_horizon
        lbg = [0.0]
        ubg = [self.a_max]
        for _ in range(N + 1):
            lbg += [0.0] * 5
            ubg += [0.0] * 5
        for _ in range(N + 1):
            lbg += [(self.radius_ego + self.radius_obstacle)] * 9
            ubg += [np.inf] * 9
        lbx, ubx = [], []
        for _ in range(N):
            lbx += [self.deltav_min, -np.inf]
            ubx += [self.deltav_max, self.a_max]
        for _ in range(N + 1):
            lbx += [-np.inf, -np.inf, self.delta_min, self.v_min, -np.inf]
            ubx += [np.inf, np.inf, self.delta_max, self.v_max, np.inf]
        return lbg, ubg, lbx, ubx

    # -- solver object: optimizer.py:513-560 ---------------------------------------------------------------------
    def solver(self):
        if self._sol is None:
            w = self.weights_setting
            Q = [w["weight_x"], w["weight_y"], w["weight_steering_angle"], w["weight_velocity"], w["weight_heading_angle"]]
            R = [w["weight_velocity_steering_angle"], w["weight_long_acceleration"]]
            Pt = [w["weight_x_terminate"], w["weight_y_terminate"], w["weight_steering_angle_terminate"],
                  w["weight_velocity_terminate"], w["weight_heading_angle_terminate"]]
            _, disc_distance = compute_approximating_circle_radius(self.configuration.p.l, self.configuration.p.w)
            centers = np.array(self.obstacle_circles_centers_tuple, dtype=np.float64)
            backend = BatchedMPCSolver(self.predict_horizon, 5, dt=self.delta_t, Q=Q, R=R, P=Pt, obstacle_centers=centers,
                                       ego_offset=(disc_distance / 2) / 2, max_iter=100, tol=1e-8, device=self._device)
            # the lower bound 0 of the stage-0 friction row (optimizer.py:378, 424): "nlp" (default: implied by the absolute value) or
            # "ipopt" (a barrier on it too, as IPOPT has -- a solve can then end at the kink of |.|; include/mpcgpu.h, option friction_lb)
            backend.set_option("friction_lb", str(getattr(self.configuration, "friction_lb", "nlp")))
            self._sol = NlpSolverHandle(backend)
        return self._sol, self._f

    # -- closed loop: optimizer.py:562-643 -----------------------------------------------------------------------
    # set to False to run the step-by-step host loop below even when the backend has an on-device driver
    use_device_loop = True

    def optimize(self):
        num_states, num_controls, N = 5, 2, self.predict_horizon
        lbg, ubg, lbx, ubx = self.inequal_constraints()
        sol, _ = self.solver()
        backend = getattr(sol, "_backend", None)
        noised = bool(self.configuration.noised)
        sigma = 0.1 if self.configuration.use_case == "lane_following" else 0.05          # optimizer.py:612-615
        # `noise_seed` (not in the reference, whose draws are unseeded and therefore not reproducible): with it the samples come
        # from the counter-based generator of noise.py / csrc/mpc_closed_loop.h and the loop can run on the device
        seed = getattr(self.configuration, "noise_seed", None)
        if self.use_device_loop and hasattr(backend, "closed_loop") and (not noised or seed is not None):
            # the whole loop of optimizer.py:596-631 on the device (mpc_closed_loop_batch_ex): no host round trip per step
            t_ = time.time()
            backend.set_bounds(lbx, ubx, lbg, ubg)
            init_state = np.array([self.init_position[0], self.init_position[1], 0.0, self.init_velocity, self.init_orientation])
            loop_kw = dict(noise_mode=1 if noised else 0, sigma=sigma if noised else 0.0, seed=0 if seed is None else int(seed))
            if self.obstacle_tracks is not None:
                # through traffic: every stage of every solve sees the obstacle nearest to it (mpc_closed_loop_batch_traffic)
                traj, ctrl, st, cl, near, chosen = backend.closed_loop_traffic(init_state, self.resampled_path_points, self.orientation, self.desired_velocity,
                                                                                self.iter_length, self.traffic_rows(), self.obstacle_offsets,
                                                                                pairing=self.obstacle_pairing,
                                                                                **({} if self.obstacle_rsums is None else dict(rsums=self.obstacle_rsums)), **loop_kw)
                self.clearance, self.nearest, self.chosen = cl[0], near[0], chosen[0]
            elif self.obstacle_track is None:
                traj, ctrl, st = backend.closed_loop(init_state, self.resampled_path_points, self.orientation, self.desired_velocity, self.iter_length, **loop_kw)
            else:
                # every solve sees the obstacle where it is at its step, frozen over the horizon (mpc_closed_loop_batch_obst)
                track = self.obstacle_track[np.minimum(np.arange(self.iter_length), len(self.obstacle_track) - 1)][None]
                traj, ctrl, st, cl = backend.closed_loop(init_state, self.resampled_path_points, self.orientation, self.desired_velocity, self.iter_length,
                                                         obst_track=track, obst_offset=self.obstacle_offset, clearance=True, **loop_kw)
                self.clearance = cl[0]
            ok = bool(np.all(st == 1))
            sol._stats = dict(status=st[0].copy(), success=ok, return_status="Solve_Succeeded" if ok else "Not_Converged")
            return traj[0], ctrl[0], np.full(self.iter_length, (time.time() - t_) / self.iter_length)
        # ---- host-side loop: one solve per step through `sol(...)`, the plant and the warm start on the host.  Not the default path (the device
        #      loop above is); it is what runs the reference's unseeded noise and what tests/ check the device loop against.  State of the loop:
        #      the measured state, the last plan (controls 2 x N, states nx x (N + 1)) and whether a plan exists yet.
        x_now = np.array([self.init_position[0], self.init_position[1], 0.0, self.init_velocity, self.init_orientation], dtype=float)
        plan_u, plan_x = np.zeros((num_controls, N)), np.tile(x_now[:, None], (1, N + 1))
        window = np.tile(x_now, (N + 1, 1))                       # step 0 tracks the initial state itself
        applied, visited, seconds, chosen_log = [], [x_now.copy()], [], []
        for step in range(self.iter_length):
            p_vec = np.concatenate((np.zeros(num_controls * N), window.ravel()))[:, None]           # [U_ref = 0 | X_ref], optimizer.py:552
            w0 = self.warm_start(plan_u, plan_x, first=(step == 0))
            tic = time.time()
            sol, f = self.solver()
            obst_kw = {} if self.obstacle_track is None else dict(obst=self.obstacle_centers_at(step))      # (the obstacle where it is at this step)
            if self.obstacle_tracks is not None:
                # through traffic, the host twin of k_loop_traffic: stage k against the obstacles at time step + k, seen from the measured state at step 0
                # and from the shifted last plan afterwards
                placed = self.traffic_centres(step, np.tile(x_now[[0, 1, 4]], (N + 1, 1)) if step == 0 else plan_x[[0, 1, 4]].T)
                centres, picked = placed[0], placed[1]
                obst_kw = dict(obst=centres) if len(placed) == 2 else dict(obst=centres, rsum=placed[2])
                chosen_log.append(picked)
            w = sol(x0=w0, p=p_vec, lbg=lbg, lbx=lbx, ubg=ubg, ubx=ubx, **obst_kw)["x"].full().ravel()
            seconds.append(time.time() - tic)
            plan_u = w[:num_controls * N].reshape(N, num_controls).T
            plan_x = w[num_controls * N:].reshape(N + 1, num_states).T
            if noised:
                # optimizer.py:611-615 perturbs the WHOLE predicted input sequence (20 samples at N = 10; 2 N here), applies its first column and
                # shifts the perturbed sequence into the next warm start
                eps = np.random.normal(0, sigma, 2 * N).reshape(num_controls, N) if seed is None else _noise.sequence_noise(int(seed), 0, step, N, sigma)
                plan_u = plan_u + eps
            applied.append(plan_u[:, 0].copy())
            x_now = x_now + self.delta_t * np.asarray(f(x_now, plan_u[:, 0]).full()).ravel()          # forward Euler plant, optimizer.py:649-651
            plan_u, plan_x = self.shift(plan_u), self.shift(plan_x)
            window, _ = self.desired_command_and_trajectory(step, x_now, N)
            visited.append(x_now.copy())
        self.chosen = np.array(chosen_log) if chosen_log else None
        # (what the reference returns: the states the solver was called AT -- the last propagated one is dropped, optimizer.py:639-641)
        return np.array(visited[:-1]), np.array(applied), np.array(seconds)

    def open_session(self):
        """The loop of optimize() stepped from outside (BatchedMPCSolver.session), built from the configuration as optimize() builds its device loop:
        the bounds of inequal_constraints() (the radius of the largest obstacle; with obstacle_radii = "own" every obstacle's own radius sum is handed
        over besides, and the session is a sized one, as optimize()'s loop is), the initial state, the path, its orientation, the desired velocity,
        and with `obstacle_sizes` [M, 2] the obstacles' offsets and `obstacle_pairing` -- no tracks are needed (nor handed over when the configuration has
        some): the caller observes the obstacles.  Without `obstacle_sizes` the session is lane following (M = 0) past the static obstacle.  A simulator loop is `with o.open_session() as sess: u = sess.step(measured, obstacles)`, one ego: u [1, 2],
        measured [5] (None at step 0), obstacles [M, 5] = (x, y, heading, vx, vy) now -- or predicted=[M, N+1, 3], the poses a prediction module gives for the stages."""
        lbg, ubg, lbx, ubx = self.inequal_constraints()
        backend = self.solver()[0]._backend
        backend.set_bounds(lbx, ubx, lbg, ubg)
        init_state = np.array([self.init_position[0], self.init_position[1], 0.0, self.init_velocity, self.init_orientation])
        traffic = self.obstacle_offsets is not None
        return backend.session(init_state, self.resampled_path_points, self.orientation, self.desired_velocity, self.iter_length,
                               offsets=self.obstacle_offsets if traffic else None, per_ego=0, pairing=self.obstacle_pairing if traffic else 0,
                               **({} if not traffic or self.obstacle_rsums is None else dict(rsums=self.obstacle_rsums)))

    def ego_offset(self):
        """front / rear circle centres of the ego: +- disc_distance / 4 of its rectangle along its heading (what solver() hands the backend)"""
        return compute_approximating_circle_radius(self.configuration.p.l, self.configuration.p.w)[1] / 4

    def traffic_rows(self):
        """obstacle_tracks as the loop takes them: [M, Lt, 3] with Lt = 1 or Lt >= iter_length (a shorter track holds its last pose)"""
        tr = self.obstacle_tracks
        if tr.shape[1] == 1 or tr.shape[1] >= self.iter_length:
            return tr
        return tr[:, np.minimum(np.arange(self.iter_length), tr.shape[1] - 1)]

    def traffic_centres(self, step, poses):
        """(centres [N+1, 6], chosen [N+1, 3]) of the solve of loop step `step` for the predicted ego poses [N+1, 3] (x, y, psi) of its stages; with
        obstacle_radii = "own" the selection is by clearance and the slots' radius sums [N+1, 3] come third"""
        tr = self.traffic_rows()
        own = {} if self.obstacle_rsums is None else dict(rsums=self.obstacle_rsums, r_default=self.radius_obstacle + self.radius_ego)
        return nearest_obstacle_centres(poses, tr, self.obstacle_offsets, np.minimum(step + np.arange(len(poses)), tr.shape[1] - 1), self.ego_offset(),
                                        self.obstacle_pairing, np.array(self.obstacle_circles_centers_tuple, dtype=np.float64).ravel(), **own)

    @staticmethod
    def shift(plan):
        """a plan (columns = stages) moved one step ahead: the first column leaves, the last one is repeated (optimizer.py:653-654)"""
        return np.concatenate((plan[:, 1:], plan[:, -1:]), axis=1)

    @staticmethod
    def warm_start(plan_u, plan_x, first):
        """The vector handed to `sol(x0=...)`, with the layouts the reference's reshapes produce (optimizer.py:602) -- they are
        part of the behaviour: IPOPT starts where they put it.  The solver expects [u_0 .. u_{N-1} | x_0 .. x_N] stage by stage.
          states:   step 0 hands them over COMPONENT-major ([sx of all stages, sy of all stages, ...]: `next_states` is (N + 1, nx) there and is
                    transposed before it is flattened); from step 1 on stage-major, as expected
          controls: from step 1 on COMPONENT-major ([all steering rates, all accelerations]: `shift_movement` returns the transpose); at step 0 they
                    are zeros either way"""
        u_part = plan_u.ravel() if not first else np.zeros(plan_u.size)              # (2, N) row-major = component-major
        x_part = plan_x.ravel() if first else plan_x.T.ravel()                       # (nx, N + 1) row-major = component-major; transposed = stage-major
        return np.concatenate((u_part, x_part))[:, None]

    def shift_movement(self, t0, x0, u, x_f, f):
        """the reference's method of that name (optimizer.py:645-655), kept for callers that use it: Euler plant step + shifted plan; note the
        TRANSPOSED controls it returns (App. C-7)"""
        x_next = x0 + self.delta_t * f(x0, u[:, 0]).full()
        return t0 + self.delta_t, x_next, self.shift(u).T, self.shift(x_f)

    def desired_command_and_trajectory(self, i, x0_, N_):
        """Reference window of step i (optimizer.py:657-702): row 0 = the measured state, row 1 + k = (path point, delta = 0, desired velocity,
        path heading) at index i + 1 + k -- and once i >= L - N the window stops moving: it stays on the LAST N points of the path (App. C-10)."""
        L = self.iter_length
        first = min(i, L - self.predict_horizon - 1) + 1 if i >= L - self.predict_horizon else i + 1
        idx = first + np.arange(N_)
        rows = np.column_stack((self.resampled_path_points[idx, 0], self.resampled_path_points[idx, 1], np.zeros(N_),
                                np.full(N_, float(self.desired_velocity)), np.asarray(self.orientation)[idx]))
        return np.vstack((np.asarray(x0_, dtype=float).reshape(1, -1), rows)), np.zeros((N_, 2))


class ForcesInfo(object):
    """`info` of `solver.solve(problem)` (struct FORCESNLPsolver_info, FORCESNLPsolver.h:151-203): the fields the reference
    reads are `it` and `solvetime` (optimizer.py:331,355)."""

    def __init__(self, it, solvetime, res_eq, pobj=float("nan")):
        self.it = int(it)
        self.it2opt = int(it)
        self.solvetime = float(solvetime)
        self.fevalstime = 0.0
        self.QPtime = float(solvetime)
        self.res_eq = float(res_eq)
        self.rsnorm = float(res_eq)
        self.pobj = float(pobj)


class ForcesModel(object):
    """the fields of `forcespro.nlp.SymbolicModel` that optimizer.py:203-222 sets and the closed loop reads"""

    def __init__(self, N, backend, lb, ub, hl, hu):
        self.N, self.nvar, self.neq, self.nh, self.npar = N, 7, 5, 10, 10
        self.lb, self.ub, self.hl, self.hu = lb, ub, hl, hu
        self.E = np.concatenate([np.zeros((5, 2)), np.eye(5)], axis=1)
        self.xinitidx = range(2, 7)
        self._backend = backend

    def eq(self, z):
        """one RK4 step of the vehicle ODE from x = z[2:7] with u = z[0:2] (optimizer.py:91-98), on the device"""
        z = np.asarray(z, dtype=np.float64).ravel()
        return self._backend.plant_step(z[2:7], z[0:2], "rk4")


class ForcesSolverHandle(object):
    """`solver` of `model, solver = self.solver()`: `solver.solve(problem)` -> (output, exitflag, info)
    (test/FORCESNLPsolver/interface/FORCESNLPsolver_py.py:181-300), one SQP step per call on the device."""

    def __init__(self, backend, model, hessian_mode=0):
        self._backend, self._model = backend, model
        self.hessian_mode = int(hessian_mode)

    def solve(self, problem):
        N = self._model.N
        x0 = np.asarray(problem["x0"], dtype=np.float64)
        batched = x0.ndim == 3
        x0 = x0.reshape(-1, N, 7) if batched else x0.reshape(1, N, 7)
        B = x0.shape[0]
        xinit = np.asarray(problem["xinit"], dtype=np.float64).reshape(B, 5)
        par = np.asarray(problem["all_parameters"], dtype=np.float64).reshape(B, N, 10)
        t_ = time.time()
        m = self._model
        x, flag, it, res = self._backend.forces_solve(x0, xinit, par, m.lb, m.ub, m.hl, m.hu, hessian_mode=self.hessian_mode)
        dt = time.time() - t_
        fmt = "x{0:02d}" if N >= 10 else "x{0:1d}"
        if batched:
            output = {fmt.format(i + 1): x[:, i, :] for i in range(N)}
            return output, flag, [ForcesInfo(it[b], dt / B, res[b]) for b in range(B)]
        output = {fmt.format(i + 1): x[0, i, :] for i in range(N)}
        return output, int(flag[0]), ForcesInfo(it[0], dt, res[0])


class ForcesproOptimizer(Optimizer):
    """optimizer.py:86-366 with the FORCES-mode solve on the GPU (scope row f3).

    The formulation is the reference's: z = [deltaDot, aLong, x, y, delta, v, psi], RK4 shooting, friction circle and nine
    squared circle distances per stage, terminal weights, `xinit` on the first stage, ten run-time parameters per stage, ONE
    quadratic programme per call (SQP with `maxqps = 1`, BFGS initialised to 2.5 I).  The reference's solver for it is a
    generated, licence-locked binary (FORCESNLPsolver.h:209-210): its numerics cannot be matched, only its formulation
    (stage functions pinned against the generated C, row a11) and its call surface."""

    # QP Hessian of the SQP step: 0 = exact Hessian of the least-squares cost (Gauss-Newton; the default HERE), 1 = the literal
    # `bfgs_init = 2.5 I` of optimizer.py:234-237 (with one QP per call and a guess that is never refreshed it would stay
    # 2.5 I; see csrc/mpc_forces_qp.h: forces_hessian_diag and INTEGRATION.md for why that is not the default)
    hessian_mode = 0

    # not in the reference (include/mpcgpu.h, mpc_forces_closed_loop_batch_obst).  guess_mode 1, real-time iteration: after a solve with exitflag 1
    # problem["x0"] of the next solve is the solution shifted by one stage; after any other exitflag it stays as it was.  obstacle_track [L, 3]: the
    # obstacle's pose (x, y, heading) at every loop step (None: the configuration's `obstacle_track`, if it has one; without one the static obstacle);
    # its circle centres lie +- disc_distance / 4 of the obstacle rectangle along the heading.  predict_obstacle: stage j of step k sees the pose of
    # step k + j instead of step k.  With a track or guess_mode 1 the exitflags are not asserted: optimize() leaves them in `exitflags` [L].
    guess_mode = 0
    predict_obstacle = False

    def __init__(self, configuration, init_values, predict_horizon, device=0, hessian_mode=None, guess_mode=None, obstacle_track=None,
                 predict_obstacle=None):
        super(ForcesproOptimizer, self).__init__(configuration, init_values, predict_horizon)
        self._device = device
        self._pair = None
        if hessian_mode is not None:
            self.hessian_mode = int(hessian_mode)
        if guess_mode is not None:
            self.guess_mode = int(guess_mode)
        if obstacle_track is not None:
            self.obstacle_track = np.asarray(obstacle_track, dtype=np.float64).reshape(-1, 3)
        if predict_obstacle is not None:
            self.predict_obstacle = bool(predict_obstacle)
        self.exitflags = None           # optimize(): the exitflag of every step

    def inequal_constraint(self):
        """optimizer.py:100-119."""
        z_low_bound = np.array([self.deltav_min, -self.a_max, -np.inf, -np.inf, self.delta_min, self.v_min, -np.inf])
        z_upper_bound = np.array([self.deltav_max, self.a_max, np.inf, np.inf, self.delta_max, self.v_max, np.inf])
        lo = np.concatenate((np.array([0]), np.tile(np.array([(self.radius_ego + self.radius_obstacle) ** 2]), 9)))
        hi = np.concatenate((np.array([self.a_max ** 2]), np.tile(np.array([np.inf]), 9)))
        return z_low_bound, z_upper_bound, lo, hi

    def solver(self):
        """optimizer.py:196-245: (model, solver); the device handle is created once and cached."""
        if self._pair is None:
            w = self.weights_setting
            Q = [w["weight_x"], w["weight_y"], w["weight_steering_angle"], w["weight_velocity"], w["weight_heading_angle"]]
            R = [w["weight_velocity_steering_angle"], w["weight_long_acceleration"]]
            Pt = [w["weight_x_terminate"], w["weight_y_terminate"], w["weight_steering_angle_terminate"],
                  w["weight_velocity_terminate"], w["weight_heading_angle_terminate"]]
            _, disc_distance = compute_approximating_circle_radius(self.configuration.p.l, self.configuration.p.w)
            # (the obstacle circle centres are run-time parameters 4..9 of every stage in the reference, optimizer.py:319-323; the
            #  device loop fills them from the handle's description, the host loop from runtime_parameters(): the same centres)
            backend = BatchedMPCSolver(self.predict_horizon, 5, dt=0.1, Q=Q, R=R, P=Pt,            # integrator_stepsize = 0.1, optimizer.py:97
                                       friction_div=self.configuration.wheelbase, ego_offset=(disc_distance / 2) / 2,
                                       obstacle_centers=np.array(self.obstacle_circles_centers_tuple, dtype=np.float64), device=self._device)
            lb, ub, hl, hu = self.inequal_constraint()
            model = ForcesModel(self.predict_horizon, backend, lb, ub, hl, hu)
            self._pair = (model, ForcesSolverHandle(backend, model, self.hessian_mode))
        return self._pair

    def runtime_parameters(self, k, N):
        """the (10, N) parameter block of step k (optimizer.py:292-318): next N path points, desired velocities ramping to 0
        over the last N steps, next N path orientations (all replenished with the last entry), obstacle circle centres"""
        L = self.iter_length
        v_all = np.hstack((np.ones(L - N) * self.desired_velocity, np.linspace(self.desired_velocity, 0, N)))
        v = v_all[k + 1:k + 1 + N]
        pts = self.resampled_path_points.T[:, k + 1:k + 1 + N]
        ori = np.asarray(self.orientation)[k + 1:k + 1 + N]
        while pts.shape[1] != N:
            pts = np.hstack((pts, self.resampled_path_points[-1].reshape(2, -1)))
            ori = np.hstack((ori, self.orientation[-1]))
            v = np.hstack((v, v_all[-1]))
        if self.obstacle_track is None:
            oc = np.tile(np.array(self.obstacle_circles_centers_tuple, dtype=np.float64).reshape(6, 1), (1, N))
        else:
            # per-stage centres: the pose of step k (frozen over the horizon) or of step k + j (predicted), the last pose once the track ends
            oc = np.stack([self.obstacle_centers_at(k + j if self.predict_obstacle else k) for j in range(N)], axis=1)
        return np.vstack((pts, v, ori, oc))

    use_device_loop = True      # the whole loop on the device (mpc_forces_closed_loop_batch); False: the step-by-step host loop below

    def optimize(self):
        """optimizer.py:246-366"""
        model, solver = self.solver()
        L = self.iter_length
        noised = bool(self.configuration.noised)
        seed = getattr(self.configuration, "noise_seed", None)
        backend = getattr(solver, "_backend", None)
        plain = self.guess_mode == 0 and self.obstacle_track is None               # the reference's loop: every exitflag is asserted
        if self.use_device_loop and hasattr(backend, "forces_closed_loop" if plain else "forces_closed_loop_obst") and (not noised or seed is not None):
            t_ = time.time()
            sigma = 0.1 if self.configuration.use_case == "lane_following" else 0.05
            init_state = np.array([self.init_position[0], self.init_position[1], 0.0, self.init_velocity, self.init_orientation])
            loop_kw = dict(init_acc=self.init_acceleration, hessian_mode=self.hessian_mode, noise_mode=2 if noised else 0,
                           sigma=sigma if noised else 0.0, seed=0 if seed is None else int(seed))
            if plain:
                traj, ctrl, flag = backend.forces_closed_loop(init_state, self.resampled_path_points, self.orientation, self.desired_velocity, L,
                                                              model.lb, model.ub, model.hl, model.hu, **loop_kw)
                assert np.all(flag == 1), "bad exitflag"                           # optimizer.py:330
            else:
                # (mpc_forces_closed_loop_batch_obst: the exitflags are returned, not asserted)
                track = self.obstacle_track
                if track is not None:                                              # (a track that ends before the run holds its last pose)
                    track = track[np.minimum(np.arange(max(L, len(track))), len(track) - 1)][None]
                traj, ctrl, flag, cl = backend.forces_closed_loop_obst(init_state, self.resampled_path_points, self.orientation, self.desired_velocity, L,
                                                                       model.lb, model.ub, model.hl, model.hu, obst_track=track,
                                                                       obst_offset=self.obstacle_offset, predict=self.predict_obstacle,
                                                                       guess_mode=self.guess_mode, r_sum=self.radius_ego + self.radius_obstacle, **loop_kw)
                self.clearance = None if cl is None else cl[0]
            self.exitflags = flag[0].copy()
            return traj[0], ctrl[0], np.full(L, (time.time() - t_) / L)
        x = np.zeros((5, L + 1))
        u = np.zeros((2, L))
        solve_time = np.zeros(L)
        flags = np.zeros(L, dtype=np.int32)
        x0i = np.array([0.0, self.init_acceleration, self.init_position[0], self.init_position[1], 0.0, self.init_velocity, self.init_orientation])
        x0 = np.transpose(np.tile(x0i, (1, model.N)))
        xinit = np.array([self.init_position[0], self.init_position[1], 0.0, self.init_velocity, self.init_orientation])
        x[:, 0] = xinit
        # (the reference never refreshes problem["x0"]: every call linearises at the tiled initial guess, optimizer.py:264-274)
        problem = {"x0": x0.reshape(model.N, 7), "xinit": xinit, "ToleranceEqualities": 1e-1, "ToleranceInequalities": 1e-1}
        for k in range(L):
            problem["xinit"] = x[:, k]
            params = self.runtime_parameters(k, model.N)
            problem["all_parameters"] = np.reshape(np.transpose(params), (10 * model.N, 1))
            output, exitflag, info = solver.solve(problem)
            if plain:
                assert exitflag == 1, "bad exitflag"                              # optimizer.py:330
            flags[k] = exitflag
            temp = np.zeros((model.nvar, model.N))
            for i in range(model.N):
                key = "x{0:1d}".format(i + 1)
                temp[:, i] = output[key] if key in output else output["x{0:02d}".format(i + 1)]
            if self.guess_mode == 1 and exitflag == 1:
                problem["x0"] = np.concatenate((temp[:, 1:], temp[:, -1:]), axis=1).T.copy()       # the solution shifted by one stage
            pred_u = temp[0:2, :]
            if not self.configuration.noised:
                u[:, k] = pred_u[:, 0]
            else:
                sigma = 0.1 if self.configuration.use_case == "lane_following" else 0.05
                seed = getattr(self.configuration, "noise_seed", None)
                u[:, k] = pred_u[:, 0] + (np.random.normal(np.array([0, 0]), np.array([sigma, sigma]), (2,)) if seed is None
                                          else _noise.applied_noise(int(seed), 0, k, sigma))
            x[:, k + 1] = np.transpose(model.eq(np.concatenate((u[:, k], x[:, k]))))
            solve_time[k] = info.solvetime
        x = np.delete(x, -1, axis=1)
        self.exitflags = flags
        return x.T, u.T, solve_time


__all__ = ["CasadiOptimizer", "ForcesproOptimizer", "ForcesSolverHandle", "ForcesModel", "ForcesInfo", "Optimizer", "NlpSolverHandle", "DMLike", "VehicleDynamics", "ca", "np",
           "find_closest_point", "nearest_obstacle_centres", "compute_approximating_circle_radius", "compute_centers_of_approximation_circles"]
