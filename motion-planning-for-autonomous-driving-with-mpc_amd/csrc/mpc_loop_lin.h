// mpc_loop_lin.h -- the closed loop as a chain of optima: per-step feedback gains and the tangent / adjoint sweeps over them
// (mpc_closed_loop_batch_lin, mpc_loop_tangent, mpc_loop_adjoint).
//
// For one ego: s_i = traj[i], u_i = u*_0(s_i, wt, o_i) + noise, o_i = track row min(i, Lt - 1), s_{i+1} = s_i + dt f(s_i, u_i).  What the
// rollout's derivative needs of solve i is three matrices of two rows each,
//   kgain[i] = d u*_0 / d s_i   [2, 5]    wgain[i] = d u*_0 / d wt   [2, 7]    ogain[i] = (d u*_0 / d c6) (d c6 / d pose)   [2, 3]
// and a row of (dw/d parameter) is one adjoint solve of the family (mpc_sens.h) with the unit seed on that entry of w: two adjoint solves per
// family against the factor of the step's snapshot, whatever the number of directions swept later.  The measured state is column 0 of X_ref
// (the pin), so kgain is that column of the p family's gradient -- at step 0 the sum over all N + 1 columns, because the loop starts from
// p = tile(current_state) (loop_setup_instance).  The warm start (an isolated optimum does not depend on it), the reference window (a function
// of the step index) and the additive noise carry no derivative; vdes and the path are not differentiated.  With nx = 6 the progress state is
// decoupled and unweighted: the gains are those of the five states of traj.
// Plain pointers only: the same bodies run in k_loop_gain<NX, Fam>, k_loop_tangent, k_loop_adjoint and in the CPU harness of the tests
// (tests/looplinx/looplinx.cpp).
#pragma once
#include "mpc_closed_loop.h"
#include "mpc_sens.h"

namespace mpc {

// the step a gain kernel works for: gain [B, L, 2, COLS] receives rows (b, i); track / Lt / offset: LoopObstArgs' (the obstacle family only)
struct LoopGainArgs {
    int32_t L, i, Lt;
    const double* track;
    double offset;
    double* gain;
};

// A family's gradient row (dw/d parameter)' e_{u_0[j]} -> row j of its gain: COLS numbers
template <class Fam>
struct LoopGainRed;
template <int NX>
struct LoopGainRed<SensFamP<NX>> {              // the pin column of X_ref, or the sum over the columns at step 0
    static constexpr int COLS = LOOP_NS;
    MPC_HD static void row(const Params& P, const LoopGainArgs& A, int, const double* g, double* out) {
        const int X0 = 2 * P.N, last = A.i == 0 ? P.N : 0;
#pragma unroll
        for (int c = 0; c < LOOP_NS; ++c) {
            double acc = 0.0;
            for (int k = 0; k <= last; ++k) acc += g[X0 + NX * k + c];
            out[c] = acc;
        }
    }
};
template <int NX>
struct LoopGainRed<SensFamWeights<NX>> {
    static constexpr int COLS = SENS_NWT;
    MPC_HD static void row(const Params&, const LoopGainArgs&, int, const double* g, double* out) {
#pragma unroll
        for (int c = 0; c < SENS_NWT; ++c) out[c] = g[c];
    }
};
template <int NX>
struct LoopGainRed<SensFamObst<NX>> {           // times d c6 / d pose of loop_obstacle_centres at the step's pose
    static constexpr int COLS = LOOP_NPOSE;
    MPC_HD static void row(const Params&, const LoopGainArgs& A, const int b, const double* g, double* out) {
        const int r = A.i < A.Lt - 1 ? A.i : A.Lt - 1;
        const double th = A.track[((size_t)b * A.Lt + r) * 3 + 2];
        const double cs = cos(th), sn = sin(th);
        out[0] = g[0] + g[2] + g[4];
        out[1] = g[1] + g[3] + g[5];
        out[2] = A.offset * ((cs * g[3] - sn * g[2]) - (cs * g[5] - sn * g[4]));
    }
};

// Instance b of P.B at loop step A.i: factor the KKT matrix of its snapshot row, the stage data of a CIRC family, the two adjoint solves with
// unit seeds on u_0[0], u_0[1], reduced to the family's gain rows.  F, W, p: sens_family's; seed [B, n_w], grad [B, Fam::row]: scratch rows.
// NaN gains where the factor failed (status not 1, friction kink, wrong inertia); returns whether it succeeded.
// (The context is built as sens_family builds it; that function is left as it is, so that k_sens keeps its machine code.)
template <int NX, class Fam>
MPC_HD bool loop_gain_family(const Params& P, const double* snap, double* F, double* W, const double* p, double* seed, double* grad, const LoopGainArgs& A,
                             const int b) {
    using R = LoopGainRed<Fam>;
    const size_t nw = (size_t)2 * P.N + (size_t)NX * (P.N + 1), Bs = (size_t)P.B, nr = Fam::row(P.N);
    const double* sb = snap + (size_t)b * Sens<NX>::len(P.N);
    SensCtx<NX> c{P, sens_factor<NX>(P, sb, F, Bs, b), F, Bs, b, W, sb, p ? p + (size_t)b * nw : nullptr, {}, {}, {}, {}};
    double* out = A.gain + ((size_t)b * A.L + A.i) * 2 * R::COLS;
    if (!c.si.ok) {
        for (int q = 0; q < 2 * R::COLS; ++q) out[q] = NAN;
        return false;
    }
    if constexpr (Fam::CIRC) {
        const size_t nn = (size_t)3 * (P.N + 1);
        sens_obst_setup<NX>(P, sb, W, Bs, b);
        double* V = W + (size_t)(P.N + 1) * SensObst<NX>::DS * Bs + b;
        c.sol = {V, Bs}; c.work = {V + nw * Bs, Bs}; c.nrow = {V + 2 * nw * Bs, Bs}; c.om = {V + (2 * nw + nn) * Bs, Bs};
    }
    double* sd = seed + (size_t)b * nw;
    double* gr = grad + (size_t)b * nr;
    for (size_t q = 0; q < nw; ++q) sd[q] = 0.0;
#pragma unroll 1
    for (int j = 0; j < 2; ++j) {
        sd[j] = 1.0;
        Fam::adjoint(c, sd, gr);
        sd[j] = 0.0;
        R::row(P, A, b, gr, out + j * R::COLS);
    }
    return true;
}

// ---- sweeps ----------------------------------------------------------------------------------------------------------------------------
// The rollout and its gains; any gain may be null (zero).  The plant is ode_eval's: f is linear in u with d f / d u = [e_2 e_3], so the
// Jacobian I + dt F_x is sens_stage_A's at traj[i] and ctrl is not read.
struct LoopSweepArgs {
    int32_t B, L, Lt, n_dir;
    const double *traj, *kgain, *wgain, *ogain;      // [B,L,5], [B,L,2,5], [B,L,2,7], [B,L,2,3]
};

// Tangent of (ego b, direction d):  ds_0 = dinit;  du_i = K_i ds_i + W_i dwt + O_i dtrack[min(i, Lt - 1)];  dtraj[i] = ds_i, dctrl[i] = du_i;
// ds_{i+1} = ds_i + dt (F_x ds_i + F_u du_i).  dinit [B,n_dir,5], dwt [B,n_dir,7], dtrack [B,n_dir,Lt,3]: null = zero; dtraj [B,n_dir,L,5],
// dctrl [B,n_dir,L,2]: null = not asked for.  A NaN gain of step i makes dctrl NaN from row i on, dtraj in the two states the
// controls drive at row i + 1 and in every state from row i + 2 on.
MPC_HD void loop_tangent_lane(const Params& P, const LoopSweepArgs& A, const int b, const int d, const double* dinit, const double* dwt,
                              const double* dtrack, double* dtraj, double* dctrl) {
    const size_t bd = (size_t)b * A.n_dir + d;
    double ds[LOOP_NS];
#pragma unroll
    for (int q = 0; q < LOOP_NS; ++q) ds[q] = dinit ? dinit[bd * LOOP_NS + q] : 0.0;
    for (int i = 0; i < A.L; ++i) {
        const size_t bi = (size_t)b * A.L + i;
        double du[2] = {0.0, 0.0};
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (A.kgain) {
                const double* K = A.kgain + (bi * 2 + j) * LOOP_NS;
#pragma unroll
                for (int q = 0; q < LOOP_NS; ++q) du[j] += K[q] * ds[q];
            }
            if (A.wgain && dwt) {
                const double* Wg = A.wgain + (bi * 2 + j) * SENS_NWT;
#pragma unroll
                for (int q = 0; q < SENS_NWT; ++q) du[j] += Wg[q] * dwt[bd * SENS_NWT + q];
            }
            if (A.ogain && dtrack) {
                const int r = i < A.Lt - 1 ? i : A.Lt - 1;
                const double* O = A.ogain + (bi * 2 + j) * LOOP_NPOSE;
#pragma unroll
                for (int q = 0; q < LOOP_NPOSE; ++q) du[j] += O[q] * dtrack[(bd * A.Lt + r) * LOOP_NPOSE + q];
            }
        }
        if (dtraj) {
#pragma unroll
            for (int q = 0; q < LOOP_NS; ++q) dtraj[(bd * A.L + i) * LOOP_NS + q] = ds[q];
        }
        if (dctrl) { dctrl[(bd * A.L + i) * 2] = du[0]; dctrl[(bd * A.L + i) * 2 + 1] = du[1]; }
        double a[6];
        sens_stage_A(P, A.traj + bi * LOOP_NS, a);
        sens_A_vec<LOOP_NS>(ds, a, P.dt);
        ds[2] += P.dt * du[0];
        ds[3] += P.dt * du[1];
    }
}

// Adjoint of ego b:  lam = 0;  for i = L - 1 .. 0:  g_u = seed_ctrl[i] + dt F_u' lam;  grad_wt += W_i' g_u;  grad_track[min(i, Lt - 1)] +=
// O_i' g_u;  lam <- seed_traj[i] + lam + dt F_x' lam + K_i' g_u;  grad_init = lam.  seed_traj [B,L,5], seed_ctrl [B,L,2]: null = zero;
// grad_init [B,5], grad_wt [B,7] (per ego: the caller sums), grad_track [B,Lt,3]: null = not asked for.  A NaN gain of step i makes grad_init,
// grad_wt and the rows of grad_track up to min(i, Lt - 1) NaN.
MPC_HD void loop_adjoint_lane(const Params& P, const LoopSweepArgs& A, const int b, const double* seed_traj, const double* seed_ctrl, double* grad_init,
                              double* grad_wt, double* grad_track) {
    double lam[LOOP_NS], gw[SENS_NWT];
#pragma unroll
    for (int q = 0; q < LOOP_NS; ++q) lam[q] = 0.0;
#pragma unroll
    for (int q = 0; q < SENS_NWT; ++q) gw[q] = 0.0;
    double* gt = (grad_track && A.ogain) ? grad_track + (size_t)b * A.Lt * LOOP_NPOSE : nullptr;
    if (grad_track)
        for (int q = 0; q < A.Lt * LOOP_NPOSE; ++q) grad_track[(size_t)b * A.Lt * LOOP_NPOSE + q] = 0.0;
    for (int i = A.L - 1; i >= 0; --i) {
        const size_t bi = (size_t)b * A.L + i;
        double gu[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) gu[j] = (seed_ctrl ? seed_ctrl[bi * 2 + j] : 0.0) + P.dt * lam[2 + j];
        if (A.wgain) {
#pragma unroll
            for (int q = 0; q < SENS_NWT; ++q) gw[q] += A.wgain[(bi * 2) * SENS_NWT + q] * gu[0] + A.wgain[(bi * 2 + 1) * SENS_NWT + q] * gu[1];
        }
        if (gt) {
            const int r = i < A.Lt - 1 ? i : A.Lt - 1;
#pragma unroll
            for (int q = 0; q < LOOP_NPOSE; ++q)
                gt[r * LOOP_NPOSE + q] += A.ogain[(bi * 2) * LOOP_NPOSE + q] * gu[0] + A.ogain[(bi * 2 + 1) * LOOP_NPOSE + q] * gu[1];
        }
        double a[6];
        sens_stage_A(P, A.traj + bi * LOOP_NS, a);
        sens_At_vec<LOOP_NS>(lam, a, P.dt);
#pragma unroll
        for (int q = 0; q < LOOP_NS; ++q) {
            double v = lam[q] + (seed_traj ? seed_traj[bi * LOOP_NS + q] : 0.0);
            if (A.kgain) v += A.kgain[(bi * 2) * LOOP_NS + q] * gu[0] + A.kgain[(bi * 2 + 1) * LOOP_NS + q] * gu[1];
            lam[q] = v;
        }
    }
    if (grad_init) {
#pragma unroll
        for (int q = 0; q < LOOP_NS; ++q) grad_init[(size_t)b * LOOP_NS + q] = lam[q];
    }
    if (grad_wt) {
#pragma unroll
        for (int q = 0; q < SENS_NWT; ++q) grad_wt[(size_t)b * SENS_NWT + q] = gw[q];
    }
}

}  // namespace mpc
