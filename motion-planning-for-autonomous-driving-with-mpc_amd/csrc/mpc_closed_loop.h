// mpc_closed_loop.h -- the receding-horizon loop AROUND the NLP solve, one instance per thread.
//
// Restates the body of CasadiOptimizer.optimize (MPC_Planner/optimizer.py:596-631) between two `sol(...)` calls:
//   * first control of the solution, forward-Euler plant step           shift_movement, optimizer.py:645-655
//   * warm start of the next solve: shifted controls / states           optimizer.py:602 with the layouts the reference
//     really produces: at step 0 the state block is the TRANSPOSED tile of the initial state, at
//     steps >= 1 the control block is the transposed (all steering rates, then all accelerations) shifted plan
//   * next parameter vector: X_ref row 0 = new state, rows 1..N = path window i+1.., frozen to the last N path points
//     once i >= L - N                                                   desired_command_and_trajectory, optimizer.py:657-702
// Row-major [B, n_w] buffers in the decision-vector order of optimizer.py:550 ([u_0..u_{N-1} | x_0..x_N]), i.e. exactly
// what mpc_solve_batch_dev consumes and produces; nx = 5 (the CasADi formulation's state) or 6 (the benchmark's extra progress
// state s, which starts at 0 and is not reported).
// Noise (`noised: True`): the reference draws from an unseeded numpy generator (optimizer.py:611-617 / 348-354), so its runs
// cannot be reproduced; here the samples come from a counter-based generator (Philox4x32-10 + Box-Muller) keyed by
// (seed; instance, step, sample index), identical on the device, in the CPU harness and in the Python mirror (noise.py):
//   mode 1  CasadiOptimizer: N(0, sigma) on the WHOLE predicted input sequence, (2, N) row-major = sample index r * N + k; the
//           noised first column is applied to the plant and the noised sequence is what gets shifted into the next warm start
//   mode 2  ForcesproOptimizer: N(0, sigma) on the applied input only (sample indices 0, 1)
// Shared by the HIP kernels (mpcgpu.hip) and the CPU emulation harness (tests/emu).
#pragma once
#include "mpc_stage_math.h"

namespace mpc {

struct LoopArgs {
    int32_t B, N, L, Lp;             // instances, horizon, closed-loop steps (iter_length), path points per instance
    const double* init_state;        // [B,5]  (x, y, delta, v, psi)            optimizer.py:575
    const double* path;              // [B,Lp,2] resampled path points          optimizer.py:691-693
    const double* orient;            // [B,Lp]   path orientation               optimizer.py:694
    const double* vdes;              // [B]      desired velocity
    double* state;                   // [B,5]  current plant state (work buffer)
    double* x0;                      // [B,n_w] warm start of the next solve
    double* p;                       // [B,n_w] parameters of the next solve
    const double* x_out;             // [B,n_w] solution of the solve just finished
    const int32_t* status;           // [B]     its per-instance status
    double* traj;                    // [B,L,5] planned states  (row i = state BEFORE step i, optimizer.py:636-638)
    double* ctrl;                    // [B,L,2] applied controls
    int32_t* step_status;            // [B,L]   solver status of every step (the reference never looks at it)
    int32_t nx;                      // 5 or 6 (rows of x0 / p / x_out have nx states per stage; traj reports the first 5)
    int32_t noise_mode;              // 0 none, 1 whole predicted input sequence (CasADi path), 2 applied input only (FORCES path)
    double sigma;                    // 0.1 lane following, 0.05 collision avoidance (optimizer.py:612-615)
    uint32_t seed_lo, seed_hi;
    const uint32_t* abort_flag;      // device word: nonzero = a solve of this loop was abandoned, the bookkeeping kernels do nothing
};

// ---- counter-based normal samples: Philox4x32-10 (Salmon et al., SC'11) + Box-Muller
MPC_HD void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t* out) {
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// sample j of (instance b, step i): standard normal
MPC_HD double loop_normal(const LoopArgs& A, int b, int i, int j) {
    uint32_t x[4];
    philox4x32_10((uint32_t)(j >> 1), (uint32_t)i, (uint32_t)b, 0x4D5043u, A.seed_lo, A.seed_hi, x);
    const uint64_t a1 = ((uint64_t)(x[0] >> 5) << 26) | (uint64_t)(x[1] >> 6), a2 = ((uint64_t)(x[2] >> 5) << 26) | (uint64_t)(x[3] >> 6);
    const double u1 = ((double)a1 + 1.0) * 1.1102230246251565e-16, u2 = (double)a2 * 1.1102230246251565e-16;      // 2^-53: u1 in (0,1], u2 in [0,1)
    const double r = sqrt(-2.0 * log(u1)), th = 6.283185307179586 * u2;
    return (j & 1) ? r * sin(th) : r * cos(th);
}
// noise on entry (row r, column k) of the predicted input sequence of step i (mode 1), or on the applied input (mode 2, k = 0)
MPC_HD double loop_noise(const LoopArgs& A, int b, int i, int r, int k) {
    if (A.noise_mode == 1) return A.sigma * loop_normal(A, b, i, r * A.N + k);
    if (A.noise_mode == 2 && k == 0) return A.sigma * loop_normal(A, b, i, r);
    return 0.0;
}

// reference window of step `i_next - 1` has been consumed; build X_ref for the solve of step i (optimizer.py:657-702
// is called with the index of the step that just finished)
MPC_HD void loop_write_reference(const LoopArgs& A, int b, int i_done, const double* cur) {
    const int N = A.N, nx = A.nx, nw = 2 * N + nx * (N + 1);
    double* p = A.p + (size_t)b * nw;
    for (int q = 0; q < 2 * N; ++q) p[q] = 0.0;                                  // U_ref (unused by the cost)
    double* xr = p + 2 * N;
    for (int c = 0; c < nx; ++c) xr[c] = cur[c];
    const double vd = A.vdes[b];
    for (int k = 0; k < N; ++k) {
        int idx = i_done + k + 1;
        if (i_done >= A.L - N) idx = i_done + k + 1 - (i_done - (A.L - N) + 1);    // frozen tail
        const double* pt = A.path + ((size_t)b * A.Lp + idx) * 2;
        double* r = xr + nx * (k + 1);
        r[0] = pt[0]; r[1] = pt[1]; r[2] = 0.0; r[3] = vd; r[4] = A.orient[(size_t)b * A.Lp + idx];
        if (nx == 6) r[5] = 0.0;
    }
}

// before the first solve: optimizer.py:575-594
MPC_HD void loop_setup_instance(const LoopArgs& A, int b) {
    const int N = A.N, nx = A.nx, nw = 2 * N + nx * (N + 1);
    double cur[6];
    for (int c = 0; c < nx; ++c) { cur[c] = (c < 5) ? A.init_state[(size_t)b * 5 + c] : 0.0; A.state[(size_t)b * nx + c] = cur[c]; }
    double* x0 = A.x0 + (size_t)b * nw;
    double* p = A.p + (size_t)b * nw;
    for (int q = 0; q < 2 * N; ++q) { x0[q] = 0.0; p[q] = 0.0; }
    // next_trajectories = tile(current_state) as (N+1, 5) -> p;  next_states.T.reshape(-1,1) = (5, N+1) row-major -> x0
    for (int k = 0; k <= N; ++k)
        for (int c = 0; c < nx; ++c) {
            p[2 * N + nx * k + c] = cur[c];
            x0[2 * N + c * (N + 1) + k] = cur[c];
        }
}

// after solve i: record, plant step, shift, next warm start and reference
MPC_HD void loop_advance_instance(const PRef& P, const LoopArgs& A, int b, int i) {
    const int N = A.N, nx = A.nx, nw = 2 * N + nx * (N + 1);
    const double* xo = A.x_out + (size_t)b * nw;
    double cur[6], u[2], f[6], s, c, td;
    for (int q = 0; q < nx; ++q) cur[q] = A.state[(size_t)b * nx + q];
    u[0] = xo[0] + loop_noise(A, b, i, 0, 0);
    u[1] = xo[1] + loop_noise(A, b, i, 1, 0);
    for (int q = 0; q < 5; ++q) A.traj[((size_t)b * A.L + i) * 5 + q] = cur[q];
    A.ctrl[((size_t)b * A.L + i) * 2 + 0] = u[0];
    A.ctrl[((size_t)b * A.L + i) * 2 + 1] = u[1];
    if (A.step_status) A.step_status[(size_t)b * A.L + i] = A.status ? A.status[b] : 0;
    if (nx == 5) ode_eval<5>(P, cur, u, f, s, c, td); else ode_eval<6>(P, cur, u, f, s, c, td);
    for (int q = 0; q < nx; ++q) { cur[q] = cur[q] + P.dt * f[q]; A.state[(size_t)b * nx + q] = cur[q]; }
    // warm start of solve i+1.  u_end = [u_1 .. u_{N-1}, u_{N-1}] as (N,2) of the (noised) sequence; the reference flattens its
    // TRANSPOSE:
    double* x0 = A.x0 + (size_t)b * nw;
    for (int k = 0; k < N; ++k) {
        const int src = (k + 1 < N) ? k + 1 : N - 1;
        x0[k] = xo[2 * src] + (A.noise_mode == 1 ? loop_noise(A, b, i, 0, src) : 0.0);                 // all steering rates ...
        x0[N + k] = xo[2 * src + 1] + (A.noise_mode == 1 ? loop_noise(A, b, i, 1, src) : 0.0);        // ... then all accelerations
    }
    // x_f = [x_1 .. x_N, x_N] as (nx, N+1); flattened transposed = stage-major (correct order)
    for (int k = 0; k <= N; ++k) {
        const int src = (k + 1 <= N) ? k + 1 : N;
        for (int q = 0; q < nx; ++q) x0[2 * N + nx * k + q] = xo[2 * N + nx * src + q];
    }
    loop_write_reference(A, b, i, cur);
}

// =========================================================================================================================
// Per-ego obstacles that move (mpc_closed_loop_batch_obst): the solve of loop step i sees ego b's obstacle where it is AT step i,
// frozen over that solve's horizon -- the reference's NLP has one static obstacle per solve (optimizer.py:60-64, 395-403), so this
// is that NLP, re-posed every step with other centres.  Before solve i the row of ego b in a [B, 6] buffer (the `obst` rows of
// the solve) is written from its track; the solve kernels see nothing new.
// =========================================================================================================================
struct LoopObstArgs {
    int32_t B, L, Lt, nx;            // instances, loop steps, poses per track (1: the obstacle stands still; >= L: pose i at step i), states per row of `state`
    const double* track;             // [B,Lt,3] pose of ego b's obstacle: x, y, heading
    double offset;                   // front / rear circle centres: +- offset along the heading (disc_distance / 4 of the obstacle rectangle)
    double* obst;                    // [B,6]  circle centres of the next solve (order of mpc_problem_desc::obstacle); loop_obst_stage: [B,N+1,6]
    const double* state;             // [B,nx] current plant state (LoopArgs::state)
    double* clearance;               // [B,L]  loop_clearance of the state before step i against the obstacle at step i, or null
    double r_sum;                    // sum of the two circle radii: the lower bound of the handle's circle rows
    const uint32_t* abort_flag;      // as LoopArgs::abort_flag
};
// compute_centers_of_approximation_circles (configuration.py:69-93): the centre, then +- offset along the heading
MPC_HD void loop_obstacle_centres(const double* row /* x, y, heading */, double offset, double* c6) {
    const double cs = cos(row[2]), sn = sin(row[2]);
    c6[0] = row[0];               c6[1] = row[1];
    c6[2] = row[0] + offset * cs; c6[3] = row[1] + offset * sn;
    c6[4] = row[0] - offset * cs; c6[5] = row[1] - offset * sn;
}
// minimum over the three constrained pairs (ego circle j against obstacle circle j, optimizer.py:395-403) of distance - r_sum; the ego
// circles as the NLP builds them (circle_eval, P.ego_offset)
MPC_HD double loop_clearance(const Params& P, const double* state5, const double* c6, double r_sum) {
    const Trig tg = psi_trig(state5[4]);
    double best = circle_eval(P, c6, 0, state5[0], state5[1], tg.sps, tg.cps, nullptr, nullptr, false);
    for (int j = 1; j < 3; ++j) best = fmin(best, circle_eval(P, c6, j, state5[0], state5[1], tg.sps, tg.cps, nullptr, nullptr, false));
    return best - r_sum;
}
// before solve i
MPC_HD void loop_obst_instance(const Params& P, const LoopObstArgs& A, int b, int i) {
    const int row = i < A.Lt - 1 ? i : A.Lt - 1;
    double c6[6];
    loop_obstacle_centres(A.track + ((size_t)b * A.Lt + row) * 3, A.offset, c6);
    for (int q = 0; q < 6; ++q) A.obst[(size_t)b * 6 + q] = c6[q];
    if (A.clearance) A.clearance[(size_t)b * A.L + i] = loop_clearance(P, A.state + (size_t)b * A.nx, c6, A.r_sum);
}
// The predicted loop (mpc_closed_loop_batch_pred, predict 1): stage k of the solve of step i is the state at time i + k, so it sees the
// obstacle where the track puts it then -- row min(i + k, Lt - 1), the last pose held beyond the track (the rule of the FORCES-mode loop).
// A.obst is [B, N+1, 6] here; one call per (ego, stage) writes row (b, k).  The stage-0 call also writes clearance[b, i]: the state
// before step i against the pose at step i, as loop_obst_instance does.
MPC_HD void loop_obst_stage(const Params& P, const LoopObstArgs& A, int N, int b, int k, int i) {
    const int at = i + k, row = at < A.Lt - 1 ? at : A.Lt - 1;
    double c6[6];
    loop_obstacle_centres(A.track + ((size_t)b * A.Lt + row) * 3, A.offset, c6);
    double* o = A.obst + ((size_t)b * (N + 1) + k) * 6;
    for (int q = 0; q < 6; ++q) o[q] = c6[q];
    if (k == 0 && A.clearance) A.clearance[(size_t)b * A.L + i] = loop_clearance(P, A.state + (size_t)b * A.nx, c6, A.r_sum);
}

// =========================================================================================================================
// The loop through traffic (mpc_closed_loop_batch_traffic): M obstacle tracks, and before every solve each stage of each ego is given the
// circle centres of the obstacle that threatens it at that stage's time.  The NLP keeps its three circle rows per stage: this is the
// standard NEAREST-OBSTACLE formulation, not an exact multi-obstacle NLP.  Its limit: two obstacles equally close to one ego circle at one
// stage constrain it only once -- the stage sees one of them (the lowest index) and the plan may cut into the other until a later solve,
// whose selection then turns to it.
//   * time row of stage k of step i: min(i + k, Lt - 1), the rule of loop_obst_stage; an obstacle whose x at that row is not finite is
//     ABSENT there (CommonRoad obstacles live for part of a scenario)
//   * predicted ego pose of stage k: at step 0 the measured state (the warm start of step 0 is the tiled initial state, in the reference's
//     transposed layout); from step 1 on stage k of the warm start that loop_advance_instance has just written, the shifted last plan
//   * pairing 0, the reference's pairs on ONE obstacle: score(m) = min_j |E_j - O_{m,j}|, the present obstacle with the smallest score
//     (lowest index on a tie) gives all three centres of the row
//   * pairing 1, each ego circle against its nearest circle: slot j of the row is the circle O_{m,c} nearest to ego circle j over all present
//     m and c (ties: lowest m, then lowest c); the NLP's row j measures ego circle j against slot j, so front-against-rear contacts count
//   * nothing present: the descriptor's centres, chosen = -1
// One call per (ego, stage); no call reads what another one writes.  The stage-0 call also writes clearance[b, i] and nearest[b, i]: the state
// before step i against ALL nine pairs of every obstacle present at row min(i, Lt - 1), +inf / -1 when there is none.
// =========================================================================================================================
struct LoopTrafficArgs {
    int32_t B, L, Lt, nx, N, M;      // instances, loop steps, poses per track (1 or >= L), states per row of `state`, horizon, obstacles
    int32_t per_ego, pairing;        // 0: tracks [M,Lt,3], offsets [M] shared by all egos; 1: [B,M,Lt,3], [B,M].  pairing as above
    const double* tracks;            // poses x, y, heading; x not finite: absent at that row
    const double* offsets;           // front / rear circle centres of obstacle m: +- offset along its heading
    double desc_obst[6];             // the descriptor's centres: the row of a stage that sees no obstacle
    double ego_offset;               // ego circle centres: +- ego_offset along the ego's heading
    double* obst;                    // [B,N+1,6] circle centres of the next solve
    const double* state;             // [B,nx]   current plant state (LoopArgs::state)
    const double* x0;                // [B,n_w]  warm start of the next solve (LoopArgs::x0)
    double* clearance;               // [B,L] or null
    int32_t* nearest;                // [B,L] or null
    int32_t* chosen;                 // [B,L,N+1,3] or null
    double r_sum;                    // sum of the two circle radii: the lower bound of the handle's circle rows
    const uint32_t* abort_flag;      // as LoopArgs::abort_flag
};
MPC_HD bool loop_traffic_present(const double* row) { return fabs(row[0]) <= 1.7976931348623157e308; }       // (false for NaN and +-inf)
MPC_HD const double* loop_traffic_pose(const LoopTrafficArgs& A, int b, int m, int row) {
    return A.tracks + (((size_t)(A.per_ego ? b : 0) * A.M + m) * A.Lt + row) * 3;
}
MPC_HD double loop_traffic_offset(const LoopTrafficArgs& A, int b, int m) { return A.offsets[(size_t)(A.per_ego ? b : 0) * A.M + m]; }
// the three ego circle centres of a pose: the centre, then +- ego_offset along psi
MPC_HD void loop_traffic_ego(double x, double y, double psi, double ego_offset, double* e6) {
    const double cs = cos(psi), sn = sin(psi);
    e6[0] = x;                   e6[1] = y;
    e6[2] = x + ego_offset * cs; e6[3] = y + ego_offset * sn;
    e6[4] = x - ego_offset * cs; e6[5] = y - ego_offset * sn;
}
MPC_HD double loop_traffic_dist(const double* e, const double* o) {
    const double dx = e[0] - o[0], dy = e[1] - o[1];
    return sqrt(dx * dx + dy * dy);
}
// Most obstacles of a scene are far from a given stage, and the centres of one cost a sine and a cosine.  Every circle of the ego lies within
// ego_offset of its pose, every circle of obstacle m within |offset_m| of its pose, so every pair distance lies within reach_m = ego_offset +
// |offset_m| of the distance d_m of the two poses.  loop_traffic_bound: the smallest d_m + reach_m over the obstacles present at `row` -- no winner
// of any selection is farther than that; loop_traffic_near: false for an obstacle all of whose pairs are farther (by more than rounding), which
// therefore wins nothing and ties with nothing.  The selection looks at the others only: the same result as looking at all.
// `Pose`: where obstacle m is for the stage being placed, pose(m, tmp3) -> (x, y, heading) -- a row of a track (TrafficTrackPose, the loops) or an
// observed pose moved on at constant velocity (SessionObsPose, the stepping session), which is all the two differ in.
struct TrafficTrackPose {
    const LoopTrafficArgs& A;
    int b, row;
    MPC_HD const double* operator()(int m, double*) const { return loop_traffic_pose(A, b, m, row); }
};
// `Keys`: what the selection compares.  TrafficDistance (the loop through traffic, the stepping session): a key is a distance.  TrafficClearance
// (traffic of mixed sizes, below): a key is a distance less delta_m, and the row is written packed.  Everything of the second kind stands behind
// `if constexpr (Keys::SIZED)`: the first kind's arithmetic has no `- 0.0` in it for a compiler to fold or not.
struct TrafficDistance {
    static constexpr bool SIZED = false;
    const LoopTrafficArgs& A;
    MPC_HD double delta(int, int) const { return 0.0; }
    MPC_HD double rsum(int, int) const { return A.r_sum; }
    MPC_HD double margin(double bound) const { return bound * (1.0 + 1e-12) + 1e-12; }
};
template <class Keys, class Pose>
MPC_HD double loop_traffic_bound(const Keys& K, int b, const Pose& at, const double* xy) {
    const LoopTrafficArgs& A = K.A;
    double bound = INFINITY, tmp[3];
    for (int m = 0; m < A.M; ++m) {
        const double* pose = at(m, tmp);
        if (!loop_traffic_present(pose)) continue;
        double hi = loop_traffic_dist(xy, pose) + A.ego_offset + fabs(loop_traffic_offset(A, b, m));
        if constexpr (Keys::SIZED) hi -= K.delta(b, m);
        if (hi < bound) bound = hi;
    }
    return bound;
}
template <class Keys>
MPC_HD bool loop_traffic_near(const Keys& K, int b, int m, const double* pose, const double* xy, double bound) {
    const LoopTrafficArgs& A = K.A;
    double lo = loop_traffic_dist(xy, pose) - A.ego_offset - fabs(loop_traffic_offset(A, b, m));
    if constexpr (Keys::SIZED) lo -= K.delta(b, m);
    return !(lo > K.margin(bound));
}
// row (b, k) of the solve of step i, and from the stage-0 call column `col` of clearance / nearest and block `col` of chosen (the loops: col = i)
template <class Keys, class Pose>
MPC_HD void loop_traffic_place(const Keys& K, int b, int k, int i, int col, const Pose& at) {
    const LoopTrafficArgs& A = K.A;
    const int N = A.N, S = N + 1, nw = 2 * N + A.nx * S;
    const double* st = A.state + (size_t)b * A.nx;
    const double* pl = (i == 0) ? st : A.x0 + (size_t)b * nw + 2 * N + A.nx * k;
    double e6[6], c6[6], out[6], rad[3] = {A.r_sum, A.r_sum, A.r_sum}, best[3], tmp[3];
    int32_t pick[3] = {-1, -1, -1};
    loop_traffic_ego(pl[0], pl[1], pl[4], A.ego_offset, e6);
    for (int q = 0; q < 6; ++q) out[q] = A.desc_obst[q];
    double bound = loop_traffic_bound(K, b, at, pl);
    for (int m = 0; m < A.M; ++m) {
        const double* pose = at(m, tmp);
        if (!loop_traffic_present(pose) || !loop_traffic_near(K, b, m, pose, pl, bound)) continue;
        loop_obstacle_centres(pose, loop_traffic_offset(A, b, m), c6);
        const double dm = K.delta(b, m), rm = K.rsum(b, m);
        if (A.pairing == 0) {
            double score = loop_traffic_dist(e6, c6);
            for (int j = 1; j < 3; ++j) score = fmin(score, loop_traffic_dist(e6 + 2 * j, c6 + 2 * j));
            if constexpr (Keys::SIZED) score -= dm;
            if (pick[0] < 0 || score < best[0]) {
                best[0] = score;
                pick[0] = pick[1] = pick[2] = m;
                if constexpr (Keys::SIZED) rad[0] = rad[1] = rad[2] = rm;
                for (int q = 0; q < 6; ++q) out[q] = c6[q];
            }
        } else {
            for (int j = 0; j < 3; ++j)
                for (int c = 0; c < 3; ++c) {
                    double dist = loop_traffic_dist(e6 + 2 * j, c6 + 2 * c);
                    if constexpr (Keys::SIZED) dist -= dm;
                    if (pick[j] < 0 || dist < best[j]) {
                        best[j] = dist; pick[j] = m; out[2 * j] = c6[2 * c]; out[2 * j + 1] = c6[2 * c + 1];
                        if constexpr (Keys::SIZED) rad[j] = rm;
                    }
                }
        }
    }
    double* o = A.obst + ((size_t)b * S + k) * (Keys::SIZED ? OBST_SIZED_ROWS : 6);
    for (int q = 0; q < 6; ++q) o[q] = out[q];
    if constexpr (Keys::SIZED) {
        for (int j = 0; j < 3; ++j) o[OBST_SIZED_OD + j] = rad[j];
        o[OBST_SIZED_SCALE] = 0.0;
    }
    if (A.chosen)
        for (int j = 0; j < 3; ++j) A.chosen[(((size_t)b * A.L + col) * S + k) * 3 + j] = pick[j];
    if (k != 0 || (!A.clearance && !A.nearest)) return;
    // the state before step i against every circle of every obstacle present at the step's own row
    double cl = INFINITY;
    int32_t near = -1;
    loop_traffic_ego(st[0], st[1], st[4], A.ego_offset, e6);
    bound = loop_traffic_bound(K, b, at, st);
    for (int m = 0; m < A.M; ++m) {
        const double* pose = at(m, tmp);
        if (!loop_traffic_present(pose) || !loop_traffic_near(K, b, m, pose, st, bound)) continue;
        loop_obstacle_centres(pose, loop_traffic_offset(A, b, m), c6);
        const double dm = K.delta(b, m);
        for (int j = 0; j < 3; ++j)
            for (int c = 0; c < 3; ++c) {
                double dist = loop_traffic_dist(e6 + 2 * j, c6 + 2 * c);
                if constexpr (Keys::SIZED) dist -= dm;
                if (near < 0 || dist < cl) { cl = dist; near = m; }
            }
    }
    if (A.clearance) A.clearance[(size_t)b * A.L + col] = near < 0 ? INFINITY : cl - A.r_sum;
    if (A.nearest) A.nearest[(size_t)b * A.L + col] = near;
}
MPC_HD void loop_traffic_stage(const LoopTrafficArgs& A, int b, int k, int i) {
    const int at = i + k, row = at < A.Lt - 1 ? at : A.Lt - 1;
    loop_traffic_place(TrafficDistance{A}, b, k, i, i, TrafficTrackPose{A, b, row});
}

// ---- traffic of mixed sizes (mpc_closed_loop_batch_traffic_sized): obstacle m has a radius sum of its own, rsums[m], and every solve is a sized
//      one.  The selection is by CLEARANCE: with delta_m = rsums[m] - r_sum (the handle's) every key above is a distance less delta_m -- pairing 0
//      compares min_j |E_j - O_{m,j}| - delta_m, pairing 1 |E_j - O_{m,c}| - delta_m; ties as above.  The row of the solve is written PACKED, as
//      sized_pack leaves it (mpc_stage_math.h: six centres, the three slots' radius sums, a pad): the winner's centres with the winner's rsums[m];
//      nothing present: the descriptor's centres with the handle's radius.  clearance: the smallest key over all nine pairs of every present
//      obstacle, less r_sum -- the smallest distance - rsums[m].  The cull stays exact: the keys of obstacle m lie within reach_m of d_m - delta_m.
//      delta_m = 0.0 changes no bit: with every rsums[m] = r_sum the centres, chosen, clearance and nearest are TrafficDistance's.
//      (loop_traffic_place<TrafficClearance, ..>: the one text above with its SIZED parts in.)
struct LoopTrafficSizedArgs {
    LoopTrafficArgs T;               // T.obst: the packed rows [B, N+1, OBST_SIZED_ROWS]
    const double* rsums;             // [M] or [B, M], like T.offsets
};
struct TrafficClearance {
    static constexpr bool SIZED = true;
    const LoopTrafficArgs& A;
    const double* rsums;
    MPC_HD double rsum(int b, int m) const { return rsums[(size_t)(A.per_ego ? b : 0) * A.M + m]; }
    MPC_HD double delta(int b, int m) const { return rsum(b, m) - A.r_sum; }
    MPC_HD double margin(double bound) const { return bound + fabs(bound) * 1e-12 + 1e-12; }         // (a key may be negative here: the margin is on its size)
};
MPC_HD void loop_traffic_stage_sized(const LoopTrafficSizedArgs& S, int b, int k, int i) {
    const int at = i + k, row = at < S.T.Lt - 1 ? at : S.T.Lt - 1;
    loop_traffic_place(TrafficClearance{S.T, S.rsums}, b, k, i, i, TrafficTrackPose{S.T, b, row});
}

// =========================================================================================================================
// The stepping session (mpc_session_begin / _step): the loop opened at step granularity for a caller that owns the plant and the perception.
// Around the unchanged solve and loop_advance_instance it adds two pieces:
//   * ingest: the measured state (x, y, delta, v, psi) of ego b replaces the model's prediction in `state` and in row 0 of X_ref; a row whose x is
//     not finite is a dropped measurement (the prediction stays); the progress state of nx = 6 stays the model's; the warm start is left alone
//   * obstacles: obs [M, 5] (per_ego: [B, M, 5]) = (x, y, heading, vx, vy) NOW; stage k sees obstacle m moved on at constant velocity,
//     (x + (k dt) vx, y + (k dt) vy, heading) -- computed in the thread -- and the selection is loop_traffic_place's.  x not finite: absent; a
//     velocity that is not finite counts as 0.  T.L = 1: clearance / nearest [B] and chosen [B, N+1, 3] are this step's
// =========================================================================================================================
struct SessionIngestArgs {
    int32_t B, N, nx;
    const double* measured;          // [B,5]
    double* state;                   // [B,nx] LoopArgs::state
    double* p;                       // [B,n_w] LoopArgs::p
};
MPC_HD void session_ingest_instance(const SessionIngestArgs& A, int b) {
    const double* m = A.measured + (size_t)b * 5;
    if (!loop_traffic_present(m)) return;
    double* xr = A.p + (size_t)b * (2 * A.N + A.nx * (A.N + 1)) + 2 * A.N;
    for (int c = 0; c < 5; ++c) { A.state[(size_t)b * A.nx + c] = m[c]; xr[c] = m[c]; }
}
struct SessionTrafficArgs {
    LoopTrafficArgs T;               // tracks / Lt unused; L = 1
    const double* obs;               // [M,5] or [B,M,5]
    double dt;
    int32_t step;                    // 0: the ego pose of every stage is the state; later: the stages of the warm start
};
struct SessionObsPose {
    const SessionTrafficArgs& A;
    int b;
    double ahead;                    // k dt
    MPC_HD const double* operator()(int m, double* tmp) const {
        const double* o = A.obs + ((size_t)(A.T.per_ego ? b : 0) * A.T.M + m) * 5;
        tmp[0] = o[0] + ahead * (loop_traffic_present(o + 3) ? o[3] : 0.0);
        tmp[1] = o[1] + ahead * (loop_traffic_present(o + 4) ? o[4] : 0.0);
        tmp[2] = o[2];
        return tmp;
    }
};
MPC_HD void session_traffic_stage(const SessionTrafficArgs& A, int b, int k) {
    loop_traffic_place(TrafficDistance{A.T}, b, k, A.step, 0, SessionObsPose{A, b, (double)k * A.dt});
}
// ---- the rest of the square Keys x Pose (mpc_session_begin_sized, mpc_session_step_pred): loop_traffic_place has two axes, and the session above is
//      one corner of it.
//        Pose \ Keys          TrafficDistance (a plain session)        TrafficClearance (a sized session: rsums at begin)
//        TrafficTrackPose     loop_traffic_stage                       loop_traffic_stage_sized            (the loops)
//        SessionObsPose       session_traffic_stage                    session_traffic_stage_sized
//        SessionPredPose      session_pred_stage                       session_pred_stage_sized
//      SessionPredPose: the caller predicts.  pred [M, N+1, 3] (per_ego: [B, M, N+1, 3]) = (x, y, heading) of obstacle m as stage k is to see it, its
//      pose k dt from now; the thread takes row (b or 0, m, k) as it stands -- no arithmetic, so with pred[m, k] = track[m, min(i + k, Lt - 1)] a
//      stage computes what loop_traffic_stage[_sized] computes at step i, bit for bit.  x not finite: absent AT THAT STAGE (an obstacle may enter or
//      leave within the horizon).  Row 0 is the pose now: the stage-0 call takes clearance / nearest against it.  The sized forms select by clearance
//      and write the packed rows of a sized solve, T.obst [B, N+1, OBST_SIZED_ROWS]; rsums [M] / [B, M] like T.offsets.
struct SessionTrafficSizedArgs {
    SessionTrafficArgs S;
    const double* rsums;
};
MPC_HD void session_traffic_stage_sized(const SessionTrafficSizedArgs& A, int b, int k) {
    loop_traffic_place(TrafficClearance{A.S.T, A.rsums}, b, k, A.S.step, 0, SessionObsPose{A.S, b, (double)k * A.S.dt});
}
struct SessionPredArgs {
    LoopTrafficArgs T;               // tracks / Lt unused; L = 1
    const double* pred;              // [M,N+1,3] or [B,M,N+1,3]
    int32_t step;                    // as SessionTrafficArgs::step
};
struct SessionPredPose {
    const SessionPredArgs& A;
    int b, k;
    MPC_HD const double* operator()(int m, double*) const { return A.pred + (((size_t)(A.T.per_ego ? b : 0) * A.T.M + m) * (A.T.N + 1) + k) * 3; }
};
MPC_HD void session_pred_stage(const SessionPredArgs& A, int b, int k) {
    loop_traffic_place(TrafficDistance{A.T}, b, k, A.step, 0, SessionPredPose{A, b, k});
}
struct SessionPredSizedArgs {
    SessionPredArgs S;
    const double* rsums;
};
MPC_HD void session_pred_stage_sized(const SessionPredSizedArgs& A, int b, int k) {
    loop_traffic_place(TrafficClearance{A.S.T, A.rsums}, b, k, A.S.step, 0, SessionPredPose{A.S, b, k});
}

// =========================================================================================================================
// The FORCES-mode loop (ForcesproOptimizer.optimize, MPC_Planner/optimizer.py:246-366) around `solver.solve(problem)`:
//   * the guess problem["x0"] is the tiled initial point and is NEVER refreshed                              :264-274
//   * run-time parameters of step k: the next N path points / orientations (replenished with the last one), the desired
//     velocity ramping linearly to 0 over the last N steps of the run, the obstacle circle centres          :292-323
//   * the first input of the solution (+ noise on it alone when `noised`, :348-354) goes to the plant: one RK4 step   :356
// One instance per thread; buffers row-major.
// =========================================================================================================================
struct ForcesLoopArgs {
    int32_t B, N, L, Lp;             // instances, horizon, steps (iter_length = path rows the reference has), path rows per instance given
    const double* init_state;        // [B,5]
    const double* init_acc;          // [B]   initial acceleration (second entry of the guess, optimizer.py:265)
    const double* path;              // [B,Lp,2]
    const double* orient;            // [B,Lp]
    const double* vdes;              // [B]
    double obstacle[6];              // circle centres of the obstacle (problem template)
    double* state;                   // [B,5]   plant state (work buffer) = problem["xinit"] of the next solve
    double* zbar;                    // [B,N,7] problem["x0"]
    double* params;                  // [B,N,10] problem["all_parameters"]
    const double* z_out;             // [B,N,7] solution of the solve just finished
    const int32_t* exitflag;         // [B]
    double* traj;                    // [B,L,5]
    double* ctrl;                    // [B,L,2]
    int32_t* step_flag;              // [B,L] exitflag of every step (the reference asserts == 1), or null
    double dt, wheelbase;
    int32_t noise_mode;              // 0 or 2 (applied input only)
    double sigma;
    uint32_t seed_lo, seed_hi;
};

MPC_HD void forces_loop_setup_instance(const ForcesLoopArgs& A, int b) {
    double z0[7] = {0.0, A.init_acc ? A.init_acc[b] : 0.0, A.init_state[(size_t)b * 5 + 0], A.init_state[(size_t)b * 5 + 1], 0.0,
                    A.init_state[(size_t)b * 5 + 3], A.init_state[(size_t)b * 5 + 4]};
    for (int q = 0; q < 5; ++q) A.state[(size_t)b * 5 + q] = (q == 2) ? 0.0 : A.init_state[(size_t)b * 5 + q];
    for (int j = 0; j < A.N; ++j)
        for (int i = 0; i < 7; ++i) A.zbar[((size_t)b * A.N + j) * 7 + i] = z0[i];
}
// all_parameters of step k (optimizer.py:292-323)
MPC_HD void forces_loop_params_instance(const ForcesLoopArgs& A, int b, int k) {
    const int N = A.N, L = A.L;
    const double vd = A.vdes[b];
    for (int j = 0; j < N; ++j) {
        const int idx = k + 1 + j;
        const int ip = idx < A.Lp ? idx : A.Lp - 1;                                  // replenished with the last point / orientation
        // desired velocity: vdes for the first L - N steps, then linspace(vdes, 0, N); beyond the run: its last entry
        const int iv = idx < L ? idx : L - 1;
        double v = vd;
        if (iv >= L - N) {
            const int r = iv - (L - N);
            v = (N > 1) ? vd + (double)r * ((0.0 - vd) / (double)(N - 1)) : vd;      // numpy.linspace: start + i * step
            if (r == N - 1 && N > 1) v = 0.0;                                         // ... with the end point exact
        }
        double* p = A.params + ((size_t)b * N + j) * 10;
        p[0] = A.path[((size_t)b * A.Lp + ip) * 2];
        p[1] = A.path[((size_t)b * A.Lp + ip) * 2 + 1];
        p[2] = v;
        p[3] = A.orient[(size_t)b * A.Lp + ip];
        for (int q = 0; q < 6; ++q) p[4 + q] = A.obstacle[q];
    }
}
// after solve k: applied input (+ noise), record, one RK4 step of the plant
MPC_HD void forces_loop_advance_instance(const ForcesLoopArgs& A, int b, int k) {
    Params P{};
    P.dt = A.dt; P.wheelbase = A.wheelbase; P.nx = 5;
    LoopArgs nz{};
    nz.noise_mode = A.noise_mode; nz.sigma = A.sigma; nz.seed_lo = A.seed_lo; nz.seed_hi = A.seed_hi; nz.N = A.N;
    double x[5], u[2];
    for (int q = 0; q < 5; ++q) x[q] = A.state[(size_t)b * 5 + q];
    u[0] = A.z_out[((size_t)b * A.N) * 7 + 0] + loop_noise(nz, b, k, 0, 0);
    u[1] = A.z_out[((size_t)b * A.N) * 7 + 1] + loop_noise(nz, b, k, 1, 0);
    for (int q = 0; q < 5; ++q) A.traj[((size_t)b * A.L + k) * 5 + q] = x[q];
    A.ctrl[((size_t)b * A.L + k) * 2] = u[0];
    A.ctrl[((size_t)b * A.L + k) * 2 + 1] = u[1];
    if (A.step_flag) A.step_flag[(size_t)b * A.L + k] = A.exitflag ? A.exitflag[b] : 0;
    double k1[5], k2[5], k3[5], k4[5], tmp[5], s, c, td;
    const double h = A.dt;
    ode_eval<5>(P, x, u, k1, s, c, td);
    for (int i = 0; i < 5; ++i) tmp[i] = x[i] + 0.5 * h * k1[i];
    ode_eval<5>(P, tmp, u, k2, s, c, td);
    for (int i = 0; i < 5; ++i) tmp[i] = x[i] + 0.5 * h * k2[i];
    ode_eval<5>(P, tmp, u, k3, s, c, td);
    for (int i = 0; i < 5; ++i) tmp[i] = x[i] + h * k3[i];
    ode_eval<5>(P, tmp, u, k4, s, c, td);
    for (int i = 0; i < 5; ++i) A.state[(size_t)b * 5 + i] = x[i] + h / 6.0 * (k1[i] + 2 * k2[i] + 2 * k3[i] + k4[i]);
}

// =========================================================================================================================
// The FORCES-mode loop past per-ego obstacles that move, with a guess that may follow the plan (mpc_forces_closed_loop_batch_obst).
// Not in the reference, whose loop has one static obstacle and a guess it never refreshes; with guess_mode 0 and Lt 0 it is that loop.
//   * guess_mode 1 (real-time iteration): after a solve with exitflag 1 the guess of the next solve is the solution shifted by one
//     stage, zbar[j] = z_out[min(j + 1, N - 1)]; after any other exitflag the guess stays as it was
//   * stage j of step k sees the obstacle at track row min(k, Lt - 1) (predict 0: frozen over the horizon, as the NLP loop has it) or
//     min(k + j, Lt - 1) (predict 1: stage j's state is the state at time k + j -- stage 0 is pinned to xinit); the path index stays
//     k + 1 + j, the reference's own choice
// One thread per (instance, stage): row (b, j) of the parameters and of the guess is written by thread (b, j) alone, thread (b, 0)
// also records the step and moves the plant.  z_out and zbar are distinct buffers and no thread reads what another one writes in the
// same launch.
// =========================================================================================================================
struct ForcesTurnArgs {
    ForcesLoopArgs F;                // the loop's rows; F.obstacle: the centres of every stage when there is no track (Lt = 0)
    int32_t guess_mode;              // 0: the tiled initial point, never refreshed; 1: the shifted solution after exitflag 1
    int32_t Lt, predict;             // poses per track (0: none, 1: the obstacle stands still, >= L: pose i at step i); 0 / 1 as above
    const double* track;             // [B,Lt,3] pose of ego b's obstacle: x, y, heading
    double offset;                   // front / rear circle centres: +- offset along the heading
    double* clearance;               // [B,L] forces_loop_clearance of the state before step i against the obstacle at step i, or null
    double r_sum, ego_offset;        // sum of the two circle radii; ego circle centres: +- ego_offset along the ego's heading
};
// desired velocity at path index idx: vdes for the first L - N indices, then linspace(vdes, 0, N); beyond the run: its last entry
// (the rule of forces_loop_params_instance, expression for expression: the two loops agree bit for bit)
MPC_HD double forces_loop_vdes(double vd, int idx, int L, int N) {
    const int iv = idx < L ? idx : L - 1;
    double v = vd;
    if (iv >= L - N) {
        const int r = iv - (L - N);
        v = (N > 1) ? vd + (double)r * ((0.0 - vd) / (double)(N - 1)) : vd;          // numpy.linspace: start + i * step
        if (r == N - 1 && N > 1) v = 0.0;                                             // ... with the end point exact
    }
    return v;
}
// track row that stage j of step k sees
MPC_HD int forces_turn_pose_row(const ForcesTurnArgs& A, int k, int j) {
    const int i = A.predict ? k + j : k;
    return i < A.Lt - 1 ? i : A.Lt - 1;
}
// row (b, j) of all_parameters of step k
MPC_HD void forces_turn_param_row(const ForcesTurnArgs& A, int b, int j, int k) {
    const ForcesLoopArgs& F = A.F;
    const int idx = k + 1 + j;
    const int ip = idx < F.Lp ? idx : F.Lp - 1;                                       // replenished with the last point / orientation
    double* p = F.params + ((size_t)b * F.N + j) * 10;
    p[0] = F.path[((size_t)b * F.Lp + ip) * 2];
    p[1] = F.path[((size_t)b * F.Lp + ip) * 2 + 1];
    p[2] = forces_loop_vdes(F.vdes[b], idx, F.L, F.N);
    p[3] = F.orient[(size_t)b * F.Lp + ip];
    if (A.Lt > 0) loop_obstacle_centres(A.track + ((size_t)b * A.Lt + forces_turn_pose_row(A, k, j)) * 3, A.offset, p + 4);
    else for (int q = 0; q < 6; ++q) p[4 + q] = F.obstacle[q];
}
// row (b, j) of the guess after a solve: the solution shifted by one stage, or left alone
MPC_HD void forces_turn_guess_row(const ForcesTurnArgs& A, int b, int j) {
    const ForcesLoopArgs& F = A.F;
    if (A.guess_mode != 1 || F.exitflag[b] != 1) return;
    const int src = j + 1 < F.N ? j + 1 : F.N - 1;
    for (int i = 0; i < 7; ++i) F.zbar[((size_t)b * F.N + j) * 7 + i] = F.z_out[((size_t)b * F.N + src) * 7 + i];
}
// minimum over all nine circle pairs (the FORCES model constrains every ego circle against every obstacle circle) of distance - r_sum
MPC_HD double forces_loop_clearance(double ego_offset, const double* state5, const double* c6, double r_sum) {
    const double cs = cos(state5[4]), sn = sin(state5[4]);
    double best = 0.0;
    for (int e = 0; e < 3; ++e) {
        const double sg = (e == 0) ? 0.0 : (e == 1 ? 1.0 : -1.0);
        const double ex = state5[0] + sg * ego_offset * cs, ey = state5[1] + sg * ego_offset * sn;
        for (int j = 0; j < 3; ++j) {
            const double dx = ex - c6[2 * j], dy = ey - c6[2 * j + 1];
            const double d = sqrt(dx * dx + dy * dy);
            if ((e == 0 && j == 0) || d < best) best = d;
        }
    }
    return best - r_sum;
}
// clearance[b, i]: the plant state (the state before step i) against the obstacle at step i
MPC_HD void forces_turn_clearance(const ForcesTurnArgs& A, int b, int i) {
    if (!A.clearance || A.Lt <= 0) return;
    const int row = i < A.Lt - 1 ? i : A.Lt - 1;
    double c6[6];
    loop_obstacle_centres(A.track + ((size_t)b * A.Lt + row) * 3, A.offset, c6);
    A.clearance[(size_t)b * A.F.L + i] = forces_loop_clearance(A.ego_offset, A.F.state + (size_t)b * 5, c6, A.r_sum);
}
// before the first solve, thread (b, j): row j of the tiled guess and of the parameters of step 0; thread (b, 0): the plant state, clearance[b, 0]
MPC_HD void forces_turn_setup_row(const ForcesTurnArgs& A, int b, int j) {
    const ForcesLoopArgs& F = A.F;
    const double z0[7] = {0.0, F.init_acc ? F.init_acc[b] : 0.0, F.init_state[(size_t)b * 5 + 0], F.init_state[(size_t)b * 5 + 1], 0.0,
                          F.init_state[(size_t)b * 5 + 3], F.init_state[(size_t)b * 5 + 4]};
    for (int i = 0; i < 7; ++i) F.zbar[((size_t)b * F.N + j) * 7 + i] = z0[i];
    forces_turn_param_row(A, b, j, 0);
    if (j == 0) {
        for (int q = 0; q < 5; ++q) F.state[(size_t)b * 5 + q] = (q == 2) ? 0.0 : F.init_state[(size_t)b * 5 + q];
        forces_turn_clearance(A, b, 0);
    }
}
// after solve k, thread (b, j): the guess and the parameters of step k + 1 (none after the last step); thread (b, 0): record step k, the applied
// input (+ noise), one RK4 step of the plant, clearance[b, k + 1]
MPC_HD void forces_turn_row(const ForcesTurnArgs& A, int b, int j, int k) {
    if (k + 1 < A.F.L) {
        forces_turn_guess_row(A, b, j);
        forces_turn_param_row(A, b, j, k + 1);
    }
    if (j == 0) {
        forces_loop_advance_instance(A.F, b, k);
        if (k + 1 < A.F.L) forces_turn_clearance(A, b, k + 1);
    }
}

}  // namespace mpc
