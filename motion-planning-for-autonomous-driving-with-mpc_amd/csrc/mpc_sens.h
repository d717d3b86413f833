// mpc_sens.h -- parametric sensitivities of a converged solve (mpc_solve_batch_sens, mpc_sens_adjoint).
//
// The derivative of the returned optimum w*(p) with respect to the parameter row p = [U_ref | X_ref] is sIPOPT's step: the KKT matrix of
// the final barrier iterate, with no inertia correction, solved against -d(KKT residual)/dp dp.  After the bound multipliers and the
// slacks of the friction / circle rows are eliminated (each side adds z / gap to the condensed Hessian), it is the block-tridiagonal
// equality-constrained QP of the solver's own Newton step: per stage the Lagrangian Hessian H_k (state), Ruu_k (input), the input-state
// coupling S_k (stage 0, a kept friction row only), the dynamics x_{k+1} = A_k x_k + B u_k and the pin x_0 = r_0.  It is factored by a
// Riccati recursion (u_k = -K_k x_k + kff_k); a pivot <= 0 of any M_k = Ruu_k + B' P_{k+1} B (wrong inertia) makes the instance NaN.
//
// p enters the residual in three places (U_ref in none):
//   the cost gradient of x_k:   df 2 Q (x_k - xref_{k+1})           ->  d rx_k = 2 df Q d xref_{k+1}     (k < N)
//   the pin rows:               x_0 - xref_0                         ->  d c_0  = d xref_0
//   a presolved friction row:   the bounds -+ sqrt(fu - c(delta_0, v_0)) of a_0 (prestart_a0_of), with (delta_0, v_0) = xref_0
//                               ->  d ru_0[a] = sum over the sides the row set of z / gap * d bound / d (delta_0, v_0)
// The objective scaling df multiplies the Hessian, the gradient and the multipliers alike and drops out of the primal step.
//
// Two layers, plain pointers only, so that the same code runs in the kernels (k_sens_gather, k_sens_factor_solve) and in the CPU harness of
// the tests (tests/sensx/sensx.cpp):
//   snapshot  instance-major copy of the final iterate [(N + 1) stages of SS | a tail of T_COUNT], written by sens_gather_stage
//   factor    per stage FS doubles, [stage][entry][Bs] (entry e of stage k of instance b at (k FS + e) Bs + b: lanes of a wave coalesce)
#pragma once

namespace mpc {

template <int NX>
struct Sens {
    static constexpr int NZ = NX + 2;
    // snapshot, per stage: iterate (u | x), bound multipliers, equality multipliers, circle-row slacks / multipliers / slack-bound multipliers
    static constexpr int Z = 0, ZL = NZ, ZU = 2 * NZ, LAM = 3 * NZ, SO = 3 * NZ + NX, NUO = SO + 3, ZLO = SO + 6, ZUO = SO + 9, SS = SO + 12;
    // snapshot tail: valid flag (1: status 1 and the iterate found), df, per-instance bounds of a_0, friction row kept, its slack and
    // multipliers, the obstacle centres
    static constexpr int T_OK = 0, T_DF = 1, T_A0LB = 2, T_A0UB = 3, T_FROW = 4, T_SF = 5, T_NUF = 6, T_ZLF = 7, T_ZUF = 8, T_OBST = 9, T_COUNT = 16;
    // factor, per stage: gains K (2 x NX, row-major), M = Ruu + B'PB (00, 01, 11), its Cholesky factor (l00, l10, l11), the off-identity
    // entries of A (a03 a04 a13 a14 a42 a43), the feed-forward kff of the right-hand side being solved
    static constexpr int F_K = 0, F_M = 2 * NX, F_L = F_M + 3, F_A = F_L + 3, F_KFF = F_A + 6, FS = F_KFF + 2;
    MPC_HD static size_t len(int N) { return (size_t)(N + 1) * SS + T_COUNT; }
};

// what the solves of one instance need besides the factor
struct SensInst {
    bool ok;            // snapshot valid, not on the friction kink, every pivot > 0
    double df;
    double frd[2];      // d ru_0[a_0] / d xref_0[(delta, v)] of a presolved friction row (0 otherwise)
};

// ---- snapshot --------------------------------------------------------------------------------------------------------------------------
// stage k of instance b of the workspace (tile-major rows, or the mailbox when in_mb) -> its snapshot row snap; stage 0 adds the tail.
// ob: the instance's six obstacle centres
template <int NX>
MPC_HD void sens_gather_stage(const Params& P, const int b, const int k, const bool in_mb, const double* ob, const bool ok, double* snap) {
    using S = Sens<NX>;
    constexpr int NZ = NX + 2;
    double* s = snap + (size_t)k * S::SS;
#pragma unroll
    for (int i = 0; i < NZ; ++i) {
        s[S::Z + i] = mult_row(P, P.Z, P.MZ, in_mb, NZ, k, i, b);
        s[S::ZL + i] = mult_row(P, P.ZL, P.MZL, in_mb, NZ, k, i, b);
        s[S::ZU + i] = mult_row(P, P.ZU, P.MZU, in_mb, NZ, k, i, b);
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) s[S::LAM + i] = mult_row(P, P.LAM, P.MLAM, in_mb, NX, k, i, b);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        s[S::SO + j] = mult_row(P, P.SO, P.MSO, in_mb, 3, k, j, b);
        s[S::NUO + j] = mult_row(P, P.NUO, P.MNUO, in_mb, 3, k, j, b);
        s[S::ZLO + j] = mult_row(P, P.ZLO, P.MZLO, in_mb, 3, k, j, b);
        s[S::ZUO + j] = mult_row(P, P.ZUO, P.MZUO, in_mb, 3, k, j, b);
    }
    if (k != 0) return;
    double* t = snap + (size_t)(P.N + 1) * S::SS;
    auto sc = [&](int row) { return P.SC[ws_index(P, P.SC, (uint32_t)row, (uint32_t)b)]; };
    t[S::T_OK] = ok ? 1.0 : 0.0;
    t[S::T_DF] = sc(SC_DF);
    t[S::T_A0LB] = sc(SC_A0LB);
    t[S::T_A0UB] = sc(SC_A0UB);
    t[S::T_FROW] = P.ISC[ws_index(P, P.ISC, (uint32_t)IS_FROW, (uint32_t)b)] != 0 ? 1.0 : 0.0;
    t[S::T_SF] = sc(SC_SF);
    t[S::T_NUF] = sc(SC_NUF);
    t[S::T_ZLF] = sc(SC_ZLF);
    t[S::T_ZUF] = sc(SC_ZUF);
#pragma unroll
    for (int i = 0; i < 6; ++i) t[S::T_OBST + i] = ob[i];
}

// ---- the final KKT matrix, stage by stage ----------------------------------------------------------------------------------------------
// A = I + E with E = (A - I) sparse: a = (a03 a04 a13 a14 a42 a43), and dt at (5, 3) for NX = 6.  Symmetric matrices are kept as their upper
// triangle (Dim<NX>::sidx); sens_sym(Ps, i, j) reads / writes either triangle.
template <int NX>
MPC_HD double& sens_sym(double* Ps, const int i, const int j) { return Ps[i <= j ? Dim<NX>::sidx(i, j) : Dim<NX>::sidx(j, i)]; }
// P <- A'PA and rows 2, 3 of PA (B'PA = dt of them) -> pa2, pa3:  W = P E (columns 2, 3, 4), A'PA = P + W + W' + E'W
template <int NX>
MPC_HD void sens_congruence(double* Ps, const double* a, const double dt, double* pa2, double* pa3) {
    double W[NX][3];
#pragma unroll
    for (int r = 0; r < NX; ++r) {
        const double p0 = sens_sym<NX>(Ps, r, 0), p1 = sens_sym<NX>(Ps, r, 1), p4 = sens_sym<NX>(Ps, r, 4);
        W[r][0] = p4 * a[4];
        W[r][1] = p0 * a[0] + p1 * a[2] + p4 * a[5];
        if (NX == 6) W[r][1] += sens_sym<NX>(Ps, r, NX - 1) * dt;
        W[r][2] = p0 * a[1] + p1 * a[3];
    }
#pragma unroll
    for (int j = 0; j < NX; ++j) {
        pa2[j] = sens_sym<NX>(Ps, 2, j) + ((j >= 2 && j <= 4) ? W[2][j - 2] : 0.0);
        pa3[j] = sens_sym<NX>(Ps, 3, j) + ((j >= 2 && j <= 4) ? W[3][j - 2] : 0.0);
    }
    // E'W (rows / columns 2..4): row 2 a42 W[4], row 3 a03 W[0] + a13 W[1] + a43 W[4] (+ dt W[5]), row 4 a04 W[0] + a14 W[1]
    double EW[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        EW[0][c] = a[4] * W[4][c];
        EW[1][c] = a[0] * W[0][c] + a[2] * W[1][c] + a[5] * W[4][c];
        if (NX == 6) EW[1][c] += dt * W[NX - 1][c];
        EW[2][c] = a[1] * W[0][c] + a[3] * W[1][c];
    }
#pragma unroll
    for (int i = 0; i < NX; ++i)
#pragma unroll
        for (int j = i; j < NX; ++j) {
            double v = Ps[Dim<NX>::sidx(i, j)];
            if (j >= 2 && j <= 4) v += W[i][j - 2];
            if (i >= 2 && i <= 4) v += W[j][i - 2];
            if (i >= 2 && i <= 4 && j >= 2 && j <= 4) v += EW[i - 2][j - 2];
            Ps[Dim<NX>::sidx(i, j)] = v;
        }
}
template <int NX>
MPC_HD void sens_At_vec(double* v, const double* a, const double dt) {
    const double r2 = v[2] + a[4] * v[4];
    double r3 = v[3] + a[0] * v[0] + a[2] * v[1] + a[5] * v[4];
    if (NX == 6) r3 += dt * v[NX - 1];
    const double r4 = v[4] + a[1] * v[0] + a[3] * v[1];
    v[2] = r2; v[3] = r3; v[4] = r4;
}
template <int NX>
MPC_HD void sens_A_vec(double* v, const double* a, const double dt) {
    const double v0 = v[0] + a[0] * v[3] + a[1] * v[4];
    const double v1 = v[1] + a[2] * v[3] + a[3] * v[4];
    const double v4 = v[4] + a[4] * v[2] + a[5] * v[3];
    if (NX == 6) v[NX - 1] += dt * v[3];
    v[0] = v0; v[1] = v1; v[4] = v4;
}

// The derivatives of the dynamics x_{k+1} = x_k + dt f(x_k, u_k) (ode_eval) the KKT matrix needs -- written out as phase_eval_model writes
// them, and checked against central differences of ode_eval itself by tests/test_sensitivities_cpu.py (sensx_model):
// A_k = I + dt df/dx at x: its off-identity entries
MPC_HD void sens_stage_A(const Params& P, const double* x, double* a) {
    const double dt = P.dt;
    double sps, cps;
    mpc_sincos(x[4], sps, cps);
    const double td = tan(x[2]), secd2 = 1.0 + td * td, v = x[3], il = 1.0 / P.wheelbase;
    a[0] = dt * cps; a[1] = -dt * v * sps; a[2] = dt * sps; a[3] = dt * v * cps;
    a[4] = dt * v * secd2 * il; a[5] = dt * td * il;
}
// dt sum_r lamn_r Hess_x f_r at x (f is linear in u): its entries (2,2), (2,3), (3,4), (4,4), the others are zero
MPC_HD void sens_dyn_hess(const Params& P, const double* x, const double* lamn, double* h) {
    const double dt = P.dt;
    double sps, cps;
    mpc_sincos(x[4], sps, cps);
    const double td = tan(x[2]), secd2 = 1.0 + td * td, v = x[3], il = 1.0 / P.wheelbase;
    h[0] = dt * (lamn[4] * v * 2.0 * td * secd2 * il);
    h[1] = dt * (lamn[4] * secd2 * il);
    h[2] = dt * (-lamn[0] * sps + lamn[1] * cps);
    h[3] = dt * (-v * (lamn[0] * cps + lamn[1] * sps));
}
// Stage k of the condensed KKT matrix at the snapshot (what phase_ineq_assemble / phase_eval_model assemble at an iterate, without the
// inertia correction): adds H_k into Hx, writes Ruu_k (ruu) and the coupling of a_0 with (delta_0, v_0) (hx, stage 0).
// tail: the snapshot's tail; sn: stage k's snapshot, snn: stage k + 1's (k < N)
template <int NX>
MPC_HD void sens_stage_kkt(const Params& P, const int k, const double* tail, const double* sn, const double* snn, double* Hs, double* ruu,
                           double* hx) {
    using S = Sens<NX>;
    constexpr int NZ = NX + 2;
    const int N = P.N, m = P.obst_mult;
    const double dt = P.dt, df = tail[S::T_DF];
    const double* z = sn + S::Z;
    const double* x = z + 2;
    ruu[0] = ruu[1] = 0.0;
    hx[0] = hx[1] = 0.0;
    double sps, cps;
    mpc_sincos(x[4], sps, cps);
    if (k < N) {
#pragma unroll
        for (int i = 0; i < NX; ++i) sens_sym<NX>(Hs, i, i) += df * 2 * P.Q[i];
        double h[4];
        sens_dyn_hess(P, x, snn + S::LAM, h);
        sens_sym<NX>(Hs, 2, 2) -= h[0]; sens_sym<NX>(Hs, 2, 3) -= h[1]; sens_sym<NX>(Hs, 3, 4) -= h[2]; sens_sym<NX>(Hs, 4, 4) -= h[3];
        ruu[0] = df * 2 * P.R[0];
        ruu[1] = df * 2 * P.R[1];
    }
    // variable bounds: z / gap of every side
#pragma unroll
    for (int i = 0; i < NZ; ++i) {
        if (i < 2 && k == N) continue;
        double lb = P.LB[k * NZ + i], ub = P.UB[k * NZ + i];
        if (k == 0 && i == 1) { lb = tail[S::T_A0LB]; ub = tail[S::T_A0UB]; }
        double sg = 0.0;
        if (has_lo(lb)) sg += sn[S::ZL + i] / (z[i] - lb);
        if (has_hi(ub)) sg += sn[S::ZU + i] / (ub - z[i]);
        if (i < 2) ruu[i] += sg;
        else sens_sym<NX>(Hs, i - 2, i - 2) += sg;
    }
    // circle rows (obst_mult copies of one row each; the loop stays rolled: unrolled, k_sens_factor_solve<6> goes past 256 VGPRs)
    const int oi[3] = {0, 1, 4};
#pragma unroll 1
    for (int j = 0; j < 3; ++j) {
        double J[3], Ho[6];
        circle_eval(P, tail + S::T_OBST, j, x[0], x[1], sps, cps, J, Ho, true);
        const double s = sn[S::SO + j], nu = sn[S::NUO + j];
        double sg = 0.0;
        if (P.has_ol) sg += sn[S::ZLO + j] / (s - P.ol);
        if (P.has_ou) sg += sn[S::ZUO + j] / (P.ou - s);
        int q = 0;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = r; c < 3; ++c, ++q) sens_sym<NX>(Hs, oi[r], oi[c]) += m * (nu * Ho[q] + sg * J[r] * J[c]);
    }
    // the friction row, where it is kept as a row
    if (k == 0 && tail[S::T_FROW] != 0.0) {
        double g[3], h[4];
        friction_eval(P, z[1], x[2], x[3], g, h, true);
        const double s = tail[S::T_SF], nu = tail[S::T_NUF];
        double sg = 0.0;
        if (P.has_fl) sg += tail[S::T_ZLF] / (s - P.fl);
        if (P.has_fu) sg += tail[S::T_ZUF] / (P.fu - s);
        ruu[1] += nu * h[0] + sg * g[0] * g[0];
        sens_sym<NX>(Hs, 2, 2) += nu * h[1] + sg * g[1] * g[1];
        sens_sym<NX>(Hs, 2, 3) += nu * h[2] + sg * g[1] * g[2];
        sens_sym<NX>(Hs, 3, 3) += nu * h[3] + sg * g[2] * g[2];
        hx[0] = sg * g[0] * g[1];
        hx[1] = sg * g[0] * g[2];
    }
}

// ---- factor ----------------------------------------------------------------------------------------------------------------------------
// Riccati recursion of instance b (snapshot row snap) into F (stride Bs): P_N = H_N; for k = N-1 .. 0 with P = P_{k+1}:
//   M_k = Ruu_k + B'PB, N_k = S_k + B'PA_k, K_k = M_k^-1 N_k, P_k = H_k + A_k'PA_k - N_k'K_k      (B = dt [e_2 e_3])
// Returns what the solves need; ok = false: snapshot invalid, friction kink, or a pivot of some M_k <= 0 (no regularisation).
template <int NX>
MPC_HD SensInst sens_factor(const Params& P, const double* snap, double* F, const size_t Bs, const int b) {
    using S = Sens<NX>;
    const int N = P.N;
    const double dt = P.dt;
    const double* tail = snap + (size_t)(N + 1) * S::SS;
    SensInst r;
    r.df = tail[S::T_DF];
    r.frd[0] = r.frd[1] = 0.0;
    r.ok = tail[S::T_OK] == 1.0;
    if (!r.ok) return r;
    auto f = [&](int k, int e) -> double& { return F[((size_t)k * S::FS + e) * Bs + b]; };
    // presolved friction row: which sides of a_0 it set, and how those bounds move with (delta_0, v_0)
    {
        const double* z0 = snap + S::Z;
        const double a = z0[1], dl = z0[2 + 2], v0 = z0[2 + 3];
        if (a * a + v0 * (tan(dl) * v0 / P.friction_div) == 0.0) { r.ok = false; return r; }      // the kink (lam_g[0] is NaN there too)
        if (tail[S::T_FROW] == 0.0) {
            const double lb = tail[S::T_A0LB], ub = tail[S::T_A0UB];
            const double td = tan(dl);
            const double dc[2] = {v0 * v0 * (1.0 + td * td) / P.friction_div, 2.0 * v0 * td / P.friction_div};       // dc / d(delta_0, v_0)
            double w = 0.0;
            if (has_lo(lb) && lb > P.LB[1]) w += snap[S::ZL + 1] / (a - lb) * (1.0 / (2.0 * -lb));          // d lb = +dc / (2 amax), amax = -lb
            if (has_hi(ub) && ub < P.UB[1]) w -= snap[S::ZU + 1] / (ub - a) * (1.0 / (2.0 * ub));           // d ub = -dc / (2 amax), amax = ub
            r.frd[0] = w * dc[0];
            r.frd[1] = w * dc[1];
        }
    }
    double Pm[Dim<NX>::NS];
    {
        double ruu[2], hx[2];
#pragma unroll
        for (int i = 0; i < Dim<NX>::NS; ++i) Pm[i] = 0.0;
        sens_stage_kkt<NX>(P, N, tail, snap + (size_t)N * S::SS, nullptr, Pm, ruu, hx);
    }
    for (int k = N - 1; k >= 0; --k) {
        const double* sn = snap + (size_t)k * S::SS;
        double ruu[2], hx[2], a[6];
        const double p22 = sens_sym<NX>(Pm, 2, 2), p23 = sens_sym<NX>(Pm, 2, 3), p33 = sens_sym<NX>(Pm, 3, 3);
        sens_stage_A(P, sn + S::Z + 2, a);
        double Nk[2][NX];
        sens_congruence<NX>(Pm, a, dt, Nk[0], Nk[1]);                  // A'PA, rows 2 and 3 of PA
#pragma unroll
        for (int j = 0; j < NX; ++j) { Nk[0][j] *= dt; Nk[1][j] *= dt; }
        // (a compiler barrier: without it the stage's snapshot loads are hoisted above the congruence and k_sens_factor_solve<6> holds 248
        //  VGPRs, a few short of the 256 where this toolchain starts AGPR copies; with it, 220)
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" ::: "memory");
#endif
        sens_stage_kkt<NX>(P, k, tail, sn, sn + S::SS, Pm, ruu, hx);   // + H_k
        Nk[1][2] += hx[0];
        Nk[1][3] += hx[1];
        const double m00 = ruu[0] + dt * dt * p22, m01 = dt * dt * p23, m11 = ruu[1] + dt * dt * p33;
        const double l00 = m00 > 0.0 ? sqrt(m00) : 1.0, l10 = m01 / l00;
        const double d1 = m11 - l10 * l10;
        if (!(m00 > 0.0) || !(d1 > 0.0)) { r.ok = false; return r; }
        const double l11 = sqrt(d1);
        // M = L L': Y = L^-1 N in place of N, N'M^-1 N = Y'Y, K = L'^-1 Y (stored at once: no second 2 x NX block stays live)
#pragma unroll
        for (int j = 0; j < NX; ++j) {
            const double y0 = Nk[0][j] / l00, y1 = (Nk[1][j] - l10 * y0) / l11;
            Nk[0][j] = y0;
            Nk[1][j] = y1;
            const double k1 = y1 / l11;
            f(k, S::F_K + NX + j) = k1;
            f(k, S::F_K + j) = (y0 - l10 * k1) / l00;
        }
#pragma unroll
        for (int i = 0; i < NX; ++i)
#pragma unroll
            for (int j = i; j < NX; ++j) Pm[Dim<NX>::sidx(i, j)] -= Nk[0][i] * Nk[0][j] + Nk[1][i] * Nk[1][j];
        f(k, S::F_M) = m00; f(k, S::F_M + 1) = m01; f(k, S::F_M + 2) = m11;
        f(k, S::F_L) = l00; f(k, S::F_L + 1) = l10; f(k, S::F_L + 2) = l11;
#pragma unroll
        for (int e = 0; e < 6; ++e) f(k, S::F_A + e) = a[e];
    }
    return r;
}

// ---- solves ----------------------------------------------------------------------------------------------------------------------------
// One right-hand side against the factor: stationarity rows (ru_k, rx_k) from rhs_u(k, i) / rhs_x(k, i), the pin row c_0, every defect row 0.
//   backward  s_N = rx_N;  kff_k = M_k^-1 (ru_k + B' s_{k+1}),  s_k = rx_k + A_k' s_{k+1} - K_k' M_k kff_k
//   forward   x_0 = c_0;  u_k = -K_k x_k + kff_k,  x_{k+1} = A_k x_k + B u_k;  the pin multiplier lam_0 = s_0 - P_0 x_0 (= s_0 for c_0 = 0)
// out_u(k, u) / out_x(k, x) receive the primal step stage by stage; returns lam_0 through lam0 (meaningful for c_0 = 0 only).
template <int NX, class RU, class RX, class OU, class OX>
MPC_HD void sens_solve(const Params& P, double* F, const size_t Bs, const int b, const double* c0, RU rhs_u, RX rhs_x, OU out_u, OX out_x,
                       double* lam0) {
    using S = Sens<NX>;
    const int N = P.N;
    const double dt = P.dt;
    auto f = [&](int k, int e) -> double& { return F[((size_t)k * S::FS + e) * Bs + b]; };
    double s[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) s[i] = rhs_x(N, i);
    for (int k = N - 1; k >= 0; --k) {
        double a[6];
#pragma unroll
        for (int e = 0; e < 6; ++e) a[e] = f(k, S::F_A + e);
        const double l00 = f(k, S::F_L), l10 = f(k, S::F_L + 1), l11 = f(k, S::F_L + 2);
        const double g0 = rhs_u(k, 0) + dt * s[2], g1 = rhs_u(k, 1) + dt * s[3];
        const double y0 = g0 / l00, y1 = (g1 - l10 * y0) / l11;
        const double kf1 = y1 / l11, kf0 = (y0 - l10 * kf1) / l00;
        f(k, S::F_KFF) = kf0;
        f(k, S::F_KFF + 1) = kf1;
        const double mk0 = f(k, S::F_M) * kf0 + f(k, S::F_M + 1) * kf1, mk1 = f(k, S::F_M + 1) * kf0 + f(k, S::F_M + 2) * kf1;
        sens_At_vec<NX>(s, a, dt);
#pragma unroll
        for (int i = 0; i < NX; ++i) s[i] += rhs_x(k, i) - (f(k, S::F_K + i) * mk0 + f(k, S::F_K + NX + i) * mk1);
    }
    if (lam0) {
#pragma unroll
        for (int i = 0; i < NX; ++i) lam0[i] = s[i];
    }
    double x[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = c0 ? c0[i] : 0.0;
    for (int k = 0; k < N; ++k) {
        out_x(k, x);
        double a[6], u[2];
#pragma unroll
        for (int e = 0; e < 6; ++e) a[e] = f(k, S::F_A + e);
        u[0] = f(k, S::F_KFF);
        u[1] = f(k, S::F_KFF + 1);
#pragma unroll
        for (int i = 0; i < NX; ++i) { u[0] -= f(k, S::F_K + i) * x[i]; u[1] -= f(k, S::F_K + NX + i) * x[i]; }
        out_u(k, u);
        sens_A_vec<NX>(x, a, dt);
        x[2] += dt * u[0];
        x[3] += dt * u[1];
    }
    out_x(N, x);
}

// forward direction: dp [n_p] (the p row's layout) -> dw [n_w]
template <int NX>
MPC_HD void sens_forward(const Params& P, const SensInst& si, double* F, const size_t Bs, const int b, const double* dp, double* dw) {
    const int N = P.N, X0 = 2 * N;
    const double df = si.df;
    const double f0 = si.frd[0] * dp[X0 + 2] + si.frd[1] * dp[X0 + 3];
    sens_solve<NX>(P, F, Bs, b, dp + X0,
                   [&](int k, int i) { return (k == 0 && i == 1) ? f0 : 0.0; },
                   [&](int k, int i) { return k < N ? df * 2 * P.Q[i] * dp[X0 + NX * (k + 1) + i] : 0.0; },
                   [&](int k, const double* u) { dw[2 * k] = u[0]; dw[2 * k + 1] = u[1]; },
                   [&](int k, const double* x) {
#pragma unroll
                       for (int i = 0; i < NX; ++i) dw[X0 + NX * k + i] = x[i];
                   },
                   nullptr);
}

// reverse: seed_w [n_w] -> grad_p [n_p] = (dw/dp)' seed_w
template <int NX>
MPC_HD void sens_adjoint(const Params& P, const SensInst& si, double* F, const size_t Bs, const int b, const double* seed, double* gp) {
    const int N = P.N, X0 = 2 * N;
    const double df = si.df;
    double lam0[NX], ua0 = 0.0;
    for (int q = 0; q < X0; ++q) gp[q] = 0.0;
    sens_solve<NX>(P, F, Bs, b, nullptr,
                   [&](int k, int i) { return seed[2 * k + i]; },
                   [&](int k, int i) { return seed[X0 + NX * k + i]; },
                   [&](int k, const double* u) { if (k == 0) ua0 = u[1]; },
                   [&](int k, const double* x) {
                       if (k < N) {
#pragma unroll
                           for (int i = 0; i < NX; ++i) gp[X0 + NX * (k + 1) + i] = df * 2 * P.Q[i] * x[i];
                       }
                   },
                   lam0);
#pragma unroll
    for (int i = 0; i < NX; ++i) gp[X0 + i] = lam0[i];
    gp[X0 + 2] += si.frd[0] * ua0;
    gp[X0 + 3] += si.frd[1] * ua0;
}

// CasADi's lam_p = d/dp [f + lam_g' g + lam_x' x] at the returned x: X_ref column 0 -lam_g[pin rows], column k + 1 -2 Q (x_k - xref_{k+1}),
// U_ref 0; entry q of instance b's row (w, pr, lg: its rows of x, p, lam_g); NaN where the status is not 1
template <int NX>
MPC_HD double sens_lam_p_entry(const Params& P, const int q, const bool conv, const double* w, const double* pr, const double* lg) {
    const int N = P.N, X0 = 2 * N;
    if (!conv) return NAN;
    if (q < X0) return 0.0;
    const int k = (q - X0) / NX, i = (q - X0) - NX * k;
    if (k == 0) return -lg[1 + i];
    return -2.0 * P.Q[i] * (w[X0 + NX * (k - 1) + i] - pr[q]);
}

}  // namespace mpc
