// mpc_sens.h -- parametric sensitivities of a converged solve (mpc_solve_batch_sens, mpc_sens_adjoint, mpc_sens_obst, mpc_sens_weights,
// mpc_sens_bounds).
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
// The obstacle centres, the cost weights and the bounds are further right-hand sides against the same factor: their sections below state them.
//
// Two layers, plain pointers only, so that the same code runs in the kernels (k_sens_gather, k_sens<NX, Fam>) and in the CPU harness of the
// tests (tests/sensx/sensx.cpp):
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
// CIRCLE_SG = false leaves the slack weights sg J J' of the circle rows out (sens_solve_circ keeps those rows' multipliers as unknowns).
// tail: the snapshot's tail; sn: stage k's snapshot, snn: stage k + 1's (k < N)
template <int NX, bool CIRCLE_SG = true>
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
    // circle rows (obst_mult copies of one row each; the loop stays rolled: unrolled, k_sens<6, SensFamP<6>> goes past 256 VGPRs)
    const int oi[3] = {0, 1, 4};
#pragma unroll 1
    for (int j = 0; j < 3; ++j) {
        double J[3], Ho[6];
        circle_eval(P, tail + S::T_OBST, j, x[0], x[1], sps, cps, J, Ho, true);
        const double s = sn[S::SO + j], nu = sn[S::NUO + j];
        double sg = 0.0;
        if (CIRCLE_SG && P.has_ol) sg += sn[S::ZLO + j] / (s - P.ol);
        if (CIRCLE_SG && P.has_ou) sg += sn[S::ZUO + j] / (P.ou - s);
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
        // (a compiler barrier: without it the stage's snapshot loads are hoisted above the congruence and k_sens<6, SensFamP<6>> holds 248
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

// ---- the obstacle centres (mpc_sens_obst, SensFamObst) ----------------------------------------------------------------------------------
// The same step against the same factor with another right-hand side.  The centre o_j (two numbers) of obstacle circle j enters circle row j
// of every stage, dist_j(x_k, o_j) - s = 0, and nothing else.  With the row's slack eliminated (d nu = sg (J_x dx + J_o do), sg = sum z / gap,
// as sens_stage_kkt does for the matrix) the stationarity rows of x_k at the state components oi = {0, 1, 4} change by
//   m (nu Hxo + sg J_x J_o') do_j,     J_o = d dist / d o_j,  Hxo = d J_x / d o_j  (3 x 2),  m = obst_mult
// and the right-hand side is minus that; the pin row and the friction term do not depend on the obstacle.  The multipliers of the snapshot
// carry the objective scaling df, as the matrix does: it drops out of the primal step.
//
// circle_eval's distance and Jacobian J3 wrt (sx, sy, psi) with the derivatives wrt the centre of obstacle circle j:
// Jo2 = d dist / d o_j = -(ex, ey), Hxo6 = d J3 / d o_j = -T' M, row-major [3][2] (T = [I | d centre / d psi], M = (I - e e') / dist)
MPC_HD double circle_eval_centre(const Params& P, const double* obst, int j, double sx, double sy, double sps, double cps, double* J3, double* Jo2,
                                 double* Hxo6) {
    const double rho = P.ego_offset;
    const double sg = (j == 0) ? 0.0 : (j == 1 ? 1.0 : -1.0);
    const double cx = sx + sg * rho * cps - obst[2 * j];
    const double cy = sy + sg * rho * sps - obst[2 * j + 1];
    double r, ir;
    mpc_sqrt_rcp(cx * cx + cy * cy, r, ir);
    const double ex = cx * ir, ey = cy * ir;
    const double tx = -sg * rho * sps, ty = sg * rho * cps;
    J3[0] = ex;
    J3[1] = ey;
    J3[2] = ex * tx + ey * ty;
    Jo2[0] = -ex;
    Jo2[1] = -ey;
    const double m00 = (1 - ex * ex) * ir, m01 = -ex * ey * ir, m11 = (1 - ey * ey) * ir;
    Hxo6[0] = -m00; Hxo6[1] = -m01;
    Hxo6[2] = -m01; Hxo6[3] = -m11;
    Hxo6[4] = -(tx * m00 + ty * m01); Hxo6[5] = -(tx * m01 + ty * m11);
    return r;
}
// one circle row of a stage: what circle_eval_centre returns, the row's weighted multiplier m nu and slack weight m sg (sg = sum z / gap)
struct SensCirc { double J[3], Jo[2], Hxo[6], mnu, msg; };
template <int NX>
MPC_HD void sens_circ_row(const Params& P, const double* tail, const double* sn, const int j, const double sps, const double cps, SensCirc& C) {
    using S = Sens<NX>;
    const double* x = sn + S::Z + 2;
    circle_eval_centre(P, tail + S::T_OBST, j, x[0], x[1], sps, cps, C.J, C.Jo, C.Hxo);
    const double s = sn[S::SO + j];
    double sg = 0.0;
    if (P.has_ol) sg += sn[S::ZLO + j] / (s - P.ol);
    if (P.has_ou) sg += sn[S::ZUO + j] / (P.ou - s);
    C.mnu = P.obst_mult * sn[S::NUO + j];
    C.msg = P.obst_mult * sg;
}
// What the solves against the obstacle centres need of every stage, computed once per instance (it does not depend on the right-hand side:
// no trigonometry and no square root is left in the sweeps): the stage Hessian H0_k without the circle rows' slack weights sg J J', Ruu_k, the
// coupling hx, and the three circle rows.  Per stage DS doubles, [stage][entry][Bs] as the factor.
template <int NX>
struct SensObst {
    static constexpr int H = 0, RUU = Dim<NX>::NS, HX = RUU + 2, CIRC = HX + 2, CS = 13, DS = CIRC + 3 * CS;
    MPC_HD static void load_row(const double* D, const size_t Bs, const int b, const int k, const int j, SensCirc& C) {
        const double* d = D + ((size_t)k * DS + CIRC + CS * j) * Bs + b;
#pragma unroll
        for (int r = 0; r < 3; ++r) C.J[r] = d[(size_t)r * Bs];
        C.Jo[0] = d[3 * Bs]; C.Jo[1] = d[4 * Bs];
#pragma unroll
        for (int r = 0; r < 6; ++r) C.Hxo[r] = d[(size_t)(5 + r) * Bs];
        C.mnu = d[11 * Bs]; C.msg = d[12 * Bs];
    }
};
template <int NX>
MPC_HD void sens_obst_setup(const Params& P, const double* snap, double* D, const size_t Bs, const int b) {
    using S = Sens<NX>;
    using O = SensObst<NX>;
    const int N = P.N;
    const double* tail = snap + (size_t)(N + 1) * S::SS;
    for (int k = 0; k <= N; ++k) {
        const double* sn = snap + (size_t)k * S::SS;
        double* d = D + (size_t)k * O::DS * Bs + b;
        {
            double Hs[Dim<NX>::NS], ruu[2], hx[2];
#pragma unroll
            for (int i = 0; i < Dim<NX>::NS; ++i) Hs[i] = 0.0;
            sens_stage_kkt<NX, false>(P, k, tail, sn, k < N ? sn + S::SS : nullptr, Hs, ruu, hx);
#pragma unroll
            for (int i = 0; i < Dim<NX>::NS; ++i) d[(size_t)(O::H + i) * Bs] = Hs[i];
            d[(size_t)O::RUU * Bs] = ruu[0]; d[(size_t)(O::RUU + 1) * Bs] = ruu[1];
            d[(size_t)O::HX * Bs] = hx[0]; d[(size_t)(O::HX + 1) * Bs] = hx[1];
        }
        double sps, cps;
        mpc_sincos(sn[S::Z + 2 + 4], sps, cps);
#pragma unroll 1
        for (int j = 0; j < 3; ++j) {
            SensCirc C;
            sens_circ_row<NX>(P, tail, sn, j, sps, cps, C);
            double* c = d + (size_t)(O::CIRC + O::CS * j) * Bs;
#pragma unroll
            for (int r = 0; r < 3; ++r) c[(size_t)r * Bs] = C.J[r];
            c[3 * Bs] = C.Jo[0]; c[4 * Bs] = C.Jo[1];
#pragma unroll
            for (int r = 0; r < 6; ++r) c[(size_t)(5 + r) * Bs] = C.Hxo[r];
            c[11 * Bs] = C.mnu; c[12 * Bs] = C.msg;
        }
    }
}
// a vector of one instance in memory: entry q at p[q st] (st = 1: a caller's row; st = the batch: scratch, lanes of a wave coalesce)
struct SensVec {
    double* p;
    size_t st;
    MPC_HD double& operator[](const size_t q) const { return p[q * st]; }
};
constexpr int SENS_OBST_REFINE = 2;

// One right-hand side that carries circle-row terms, against the factor, to working precision.
//   stationarity rows (gu_k, gx_k) and a shift t_kj of every circle row: the row reads J_kj dx_k - t_kj - ds = 0, so that with the slack
//   eliminated its multiplier is n_kj = m sg_kj (J_kj dx_k - t_kj) and the condensed right-hand side of x_k is gx_k + sum_j m sg_kj J_kj t_kj.
// On an active row sg ~ 1 / mu: the condensed right-hand side and the matrix hold terms of 1e10 that cancel to O(1), the solve of the condensed
// system alone is good to ~1e-6 (measured: forward and adjoint disagree by up to 6e-5), and n_kj cannot be had from dx at all (J dx - t is
// known to 1e-16, times sg).  So SENS_OBST_REFINE steps of iterative refinement on the system with the circle multipliers kept as unknowns,
// whose residual is O(1) arithmetic throughout (one step leaves 6e-10 of that disagreement, two 1e-14):
//   rho_x = gx - H0 dx - S'du - sum_j J_j n_j,  rho_u = gu - Ruu du - S dx     (H0: the stage Hessian without the sg J J' terms)
//   r_nu_j = t_j - J_j dx + n_j / (m sg_j),     om_j = m sg_j r_nu_j
// the dynamics rows hold exactly (dx is rolled out with the factor's A_k), so only the residual reduced onto the inputs matters:
//   q_N = rho_x,N;  r_u,k = rho_u,k + B' q_{k+1},  q_k = rho_x,k + A_k' q_{k+1}
// the correction solves the condensed system against (r_u, sum_j J_j om_j); n_j += m sg_j J_j d(dx) - om_j.
// base(k, gx [NX], gu [2]) starts the right-hand side of stage k, row(k, j, C, gx) adds what circle row j (C) contributes and returns t_kj;
// fin(k, j, C, x [NX], n) receives the result row by row.  sol (n_w, the layout of a row of w) receives the primal step; nrow, om
// (3 (N + 1)) and work (n_w) are scratch.  REFINE: the number of refinement steps (>= 1).
template <int NX, int REFINE = SENS_OBST_REFINE, class BASE, class ROW, class FIN>
MPC_HD void sens_solve_circ(const Params& P, double* F, const size_t Bs, const int b, const double* D, BASE base, ROW row, FIN fin,
                            const SensVec sol, const SensVec nrow, const SensVec om, const SensVec work) {
    using S = Sens<NX>;
    using O = SensObst<NX>;
    const int N = P.N, X0 = 2 * N;
    const double dt = P.dt;
    auto dd = [&](int k, int e) { return D[((size_t)k * O::DS + e) * Bs + b]; };
    auto solve = [&](const SensVec v) {
        sens_solve<NX>(P, F, Bs, b, nullptr,
                       [&](int k, int i) { return v[2 * k + i]; },
                       [&](int k, int i) { return v[X0 + NX * k + i]; },
                       [&](int k, const double* u) { v[2 * k] = u[0]; v[2 * k + 1] = u[1]; },
                       [&](int k, const double* x) {
#pragma unroll
                           for (int i = 0; i < NX; ++i) v[X0 + NX * k + i] = x[i];
                       },
                       nullptr);
    };
    // the condensed solve (its right-hand side staged in sol: sens_solve has read all of it before it writes the first step)
    for (int k = 0; k <= N; ++k) {
        double gx[NX], gu[2];
        base(k, gx, gu);
#pragma unroll 1
        for (int j = 0; j < 3; ++j) {
            SensCirc C;
            O::load_row(D, Bs, b, k, j, C);
            const double tt = C.msg * row(k, j, C, gx);
            gx[0] += C.J[0] * tt; gx[1] += C.J[1] * tt; gx[4] += C.J[2] * tt;
        }
#pragma unroll
        for (int i = 0; i < NX; ++i) sol[X0 + NX * k + i] = gx[i];
        if (k < N) { sol[2 * k] = gu[0]; sol[2 * k + 1] = gu[1]; }
    }
    solve(sol);
    for (int it = 0; it < REFINE; ++it) {
        double q[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) q[i] = 0.0;
        for (int k = N; k >= 0; --k) {
            double gx[NX], gu[2], dx[NX], du[2] = {0.0, 0.0};
            base(k, gx, gu);
#pragma unroll
            for (int i = 0; i < NX; ++i) dx[i] = sol[X0 + NX * k + i];
            if (k < N) { du[0] = sol[2 * k]; du[1] = sol[2 * k + 1]; }
            const double ruu[2] = {dd(k, O::RUU), dd(k, O::RUU + 1)}, hx[2] = {dd(k, O::HX), dd(k, O::HX + 1)};
#pragma unroll
            for (int i = 0; i < NX; ++i)
#pragma unroll
                for (int c = i; c < NX; ++c) {
                    const double h = dd(k, O::H + Dim<NX>::sidx(i, c));
                    gx[i] -= h * dx[c];
                    if (c != i) gx[c] -= h * dx[i];
                }
            gx[2] -= hx[0] * du[1];
            gx[3] -= hx[1] * du[1];
            double wx[3] = {0.0, 0.0, 0.0};
#pragma unroll 1
            for (int j = 0; j < 3; ++j) {
                SensCirc C;
                O::load_row(D, Bs, b, k, j, C);
                const double t = row(k, j, C, gx);
                const double jd = C.J[0] * dx[0] + C.J[1] * dx[1] + C.J[2] * dx[4];
                double n, w;
                if (it == 0) { n = C.msg * (jd - t); w = 0.0; nrow[3 * k + j] = n; }
                else { n = nrow[3 * k + j]; w = C.msg * (t - jd) + n; }
                om[3 * k + j] = w;
                gx[0] -= C.J[0] * n; gx[1] -= C.J[1] * n; gx[4] -= C.J[2] * n;
                wx[0] += C.J[0] * w; wx[1] += C.J[1] * w; wx[2] += C.J[2] * w;
            }
            if (k < N) {
                work[2 * k] = gu[0] - ruu[0] * du[0] + dt * q[2];
                work[2 * k + 1] = gu[1] - ruu[1] * du[1] - (hx[0] * dx[2] + hx[1] * dx[3]) + dt * q[3];
                double a[6];
#pragma unroll
                for (int e = 0; e < 6; ++e) a[e] = F[((size_t)k * S::FS + S::F_A + e) * Bs + b];
                sens_At_vec<NX>(q, a, dt);
            }
#pragma unroll
            for (int i = 0; i < NX; ++i) { q[i] += gx[i]; work[X0 + NX * k + i] = 0.0; }
            work[X0 + NX * k] = wx[0]; work[X0 + NX * k + 1] = wx[1]; work[X0 + NX * k + 4] = wx[2];
        }
        solve(work);
        for (int k = 0; k <= N; ++k) {
            double x[NX], d0, d1, d4;
#pragma unroll
            for (int i = 0; i < NX; ++i) x[i] = work[X0 + NX * k + i];
            d0 = x[0]; d1 = x[1]; d4 = x[4];
#pragma unroll
            for (int i = 0; i < NX; ++i) { x[i] += sol[X0 + NX * k + i]; sol[X0 + NX * k + i] = x[i]; }
            if (k < N) { sol[2 * k] += work[2 * k]; sol[2 * k + 1] += work[2 * k + 1]; }
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                SensCirc C;
                O::load_row(D, Bs, b, k, j, C);
                const double n = nrow[3 * k + j] + (C.msg * (C.J[0] * d0 + C.J[1] * d1 + C.J[2] * d4) - om[3 * k + j]);
                nrow[3 * k + j] = n;
                if (it == REFINE - 1) fin(k, j, C, x, n);
            }
        }
    }
}

// the pieces of a right-hand side that several families share: the seed of an adjoint as base, a circle row without shift, a result nobody reads
template <int NX>
struct SensSeedRhs {
    const double* seed;
    int N;
    MPC_HD void operator()(const int k, double* gx, double* gu) const {
        const int X0 = 2 * N;
#pragma unroll
        for (int i = 0; i < NX; ++i) gx[i] = seed[X0 + NX * k + i];
        gu[0] = k < N ? seed[2 * k] : 0.0;
        gu[1] = k < N ? seed[2 * k + 1] : 0.0;
    }
};
struct SensNoShift { MPC_HD double operator()(int, int, const SensCirc&, double*) const { return 0.0; } };
struct SensNoFin { MPC_HD void operator()(int, int, const SensCirc&, const double*, double) const {} };

// forward direction: dobst [6] -> dw [n_w].  The centre o_j moves circle row j of every stage: gx_k = -m nu Hxo do_j at oi, t_kj = -J_o do_j.
// D: the stage data of sens_obst_setup; nrow, om, work: scratch of sens_solve_circ
template <int NX>
MPC_HD void sens_forward_obst(const Params& P, double* F, const size_t Bs, const int b, const double* D, const double* dobst, double* dw,
                              const SensVec nrow, const SensVec om, const SensVec work) {
    sens_solve_circ<NX>(P, F, Bs, b, D,
                        [&](int, double* gx, double* gu) {
#pragma unroll
                            for (int i = 0; i < NX; ++i) gx[i] = 0.0;
                            gu[0] = gu[1] = 0.0;
                        },
                        [&](int, int j, const SensCirc& C, double* gx) {
                            const double d0 = dobst[2 * j], d1 = dobst[2 * j + 1];
                            gx[0] -= C.mnu * (C.Hxo[0] * d0 + C.Hxo[1] * d1);
                            gx[1] -= C.mnu * (C.Hxo[2] * d0 + C.Hxo[3] * d1);
                            gx[4] -= C.mnu * (C.Hxo[4] * d0 + C.Hxo[5] * d1);
                            return -(C.Jo[0] * d0 + C.Jo[1] * d1);
                        },
                        SensNoFin{}, SensVec{dw, 1}, nrow, om, work);
}

// reverse: seed_w [n_w] -> grad_o [6] = (dw/do)' seed_w.  The solve of the seed (t = 0) gives x_k and the circle multipliers n_kj; the
// transposed right-hand side of the forward direction applied to them, summed over the stages: grad_o_j = -sum_k (m nu Hxo' x_k + J_o n_kj).
// sol: scratch for the solve's primal step (n_w)
template <int NX>
MPC_HD void sens_adjoint_obst(const Params& P, double* F, const size_t Bs, const int b, const double* D, const double* seed, double* go,
                              const SensVec sol, const SensVec nrow, const SensVec om, const SensVec work) {
    const int N = P.N, X0 = 2 * N;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    sens_solve_circ<NX>(P, F, Bs, b, D,
                        SensSeedRhs<NX>{seed, N},
                        SensNoShift{},
                        [&](int, int j, const SensCirc& C, const double* x, double n) {
                            acc[2 * j] -= C.mnu * (C.Hxo[0] * x[0] + C.Hxo[2] * x[1] + C.Hxo[4] * x[4]) + C.Jo[0] * n;
                            acc[2 * j + 1] -= C.mnu * (C.Hxo[1] * x[0] + C.Hxo[3] * x[1] + C.Hxo[5] * x[4]) + C.Jo[1] * n;
                        },
                        sol, nrow, om, work);
#pragma unroll
    for (int i = 0; i < 6; ++i) go[i] = acc[i];
}

// lam_o [6] = d/do [f + lam_g' g] at the snapshot's iterate, in CasADi's sign and scale: per circle j the sum over the stages of the row's
// multiplier -- the three copies of mult_stage summed, m nu / df -- times d dist_j / d o_j.  By the envelope theorem d f* / d o.
template <int NX>
MPC_HD void sens_lam_obst(const Params& P, const double* snap, double* lo) {
    using S = Sens<NX>;
    const int N = P.N;
    const double* tail = snap + (size_t)(N + 1) * S::SS;
    const double wm = P.obst_mult / 3.0, idf = 1.0 / tail[S::T_DF];
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k <= N; ++k) {
        const double* sn = snap + (size_t)k * S::SS;
        const double* x = sn + S::Z + 2;
        double sps, cps;
        mpc_sincos(x[4], sps, cps);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double J[3], Jo[2], Hxo[6];
            circle_eval_centre(P, tail + S::T_OBST, j, x[0], x[1], sps, cps, J, Jo, Hxo);
            const double lg = 3.0 * (sn[S::NUO + j] * idf * wm);
            acc[2 * j] += lg * Jo[0];
            acc[2 * j + 1] += lg * Jo[1];
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) lo[i] = acc[i];
}

// ---- the cost weights (mpc_sens_weights, SensFamWeights) ---------------------------------------------------------------------------------
// The same step against the same factor with a third right-hand side.  The weight vector is wt = [Q_0 .. Q_4 | R_0, R_1] (SENS_NWT numbers
// for NX = 5 and 6 alike: Q_5, the progress state's weight, is not among them).  The weights enter the residual through the cost gradient only,
//   of x_k:  df 2 Q_i e_k[i],  e_k = x_k - xref_{k+1}  (i < 5, k < N)         of u_k:  df 2 R_j u_k[j]  (k < N)
// so the right-hand side of a direction dwt is
//   rx_k[i] = -2 df e_k[i] dQ_i,   ru_k[j] = -2 df u_k[j] dR_j   (k < N);   stage N, the pin row and the friction term are 0
// (a presolved friction bound depends on xref_0, not on the weights).  df drops out of dw as it does for p.  df is held FIXED: the
// gradient-based scaling makes it a function of Q through the starting point, which moves the final barrier point at the order of mu only and
// the optimum of the NLP not at all.
// The right-hand side holds no sg = z / gap, but the MATRIX does: on an active circle row the factor carries terms of 1e10, and one sens_solve
// against it, forward and adjoint, disagree by up to 2.4e-10 of sum |seed| max |dw| (measured on the collision-avoidance batch; the bound asked
// of the adjoint identity is 1e-10).  So the solve is sens_solve_circ's, with every circle shift t = 0 and SENS_WT_REFINE step of refinement
// (the obstacle right-hand side starts from 6e-5 and needs two): the identity then holds to 5e-16.
// x_k, u_k: the snapshot's Z; xref: the instance's p row pr (the p of the solve; the snapshot does not hold it).
constexpr int SENS_WT_REFINE = 1;      // (SENS_NWT, SENS_NWQ: mpc_host_common.h)

// forward direction: dwt [7] -> dw [n_w].  D: the stage data of sens_obst_setup; nrow, om, work: scratch of sens_solve_circ
template <int NX>
MPC_HD void sens_forward_weights(const Params& P, const SensInst& si, double* F, const size_t Bs, const int b, const double* D, const double* snap,
                                 const double* pr, const double* dwt, double* dw, const SensVec nrow, const SensVec om, const SensVec work) {
    using S = Sens<NX>;
    const int N = P.N, X0 = 2 * N;
    const double m2df = -2.0 * si.df;
    sens_solve_circ<NX, SENS_WT_REFINE>(P, F, Bs, b, D,
                        [&](int k, double* gx, double* gu) {
                            const double* z = snap + (size_t)k * S::SS + S::Z;
#pragma unroll
                            for (int i = 0; i < NX; ++i) gx[i] = (k < N && i < SENS_NWQ) ? m2df * (z[2 + i] - pr[X0 + NX * (k + 1) + i]) * dwt[i] : 0.0;
                            gu[0] = k < N ? m2df * z[0] * dwt[SENS_NWQ] : 0.0;
                            gu[1] = k < N ? m2df * z[1] * dwt[SENS_NWQ + 1] : 0.0;
                        },
                        SensNoShift{},
                        SensNoFin{}, SensVec{dw, 1}, nrow, om, work);
}

// reverse: seed_w [n_w] -> gwt [7] = (dw/dwt)' seed_w.  The solve of the seed gives (y_u,k, y_x,k) in sol; the transposed right-hand side of the
// forward direction applied to them: grad_Q_i = sum_{k<N} -2 df e_k[i] y_x,k[i],  grad_R_j = sum_{k<N} -2 df u_k[j] y_u,k[j]
template <int NX>
MPC_HD void sens_adjoint_weights(const Params& P, const SensInst& si, double* F, const size_t Bs, const int b, const double* D, const double* snap,
                                 const double* pr, const double* seed, double* gwt, const SensVec sol, const SensVec nrow, const SensVec om,
                                 const SensVec work) {
    using S = Sens<NX>;
    const int N = P.N, X0 = 2 * N;
    const double m2df = -2.0 * si.df;
    sens_solve_circ<NX, SENS_WT_REFINE>(P, F, Bs, b, D,
                        SensSeedRhs<NX>{seed, N},
                        SensNoShift{},
                        SensNoFin{}, sol, nrow, om, work);
    double acc[SENS_NWT] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < N; ++k) {
        const double* z = snap + (size_t)k * S::SS + S::Z;
#pragma unroll
        for (int i = 0; i < SENS_NWQ; ++i) acc[i] += m2df * (z[2 + i] - pr[X0 + NX * (k + 1) + i]) * sol[X0 + NX * k + i];
        acc[SENS_NWQ] += m2df * z[0] * sol[2 * k];
        acc[SENS_NWQ + 1] += m2df * z[1] * sol[2 * k + 1];
    }
#pragma unroll
    for (int i = 0; i < SENS_NWT; ++i) gwt[i] = acc[i];
}

// lam_wt [7] = d/dwt [f + lam_g' g] at the snapshot's iterate = [sum_{k<N} e_k[i]^2 | sum_{k<N} u_k[j]^2] (no constraint row holds a weight):
// by the envelope theorem the derivative of the optimal objective, unscaled
template <int NX>
MPC_HD void sens_lam_weights(const Params& P, const double* snap, const double* pr, double* lwt) {
    using S = Sens<NX>;
    const int N = P.N, X0 = 2 * N;
    double acc[SENS_NWT] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < N; ++k) {
        const double* z = snap + (size_t)k * S::SS + S::Z;
#pragma unroll
        for (int i = 0; i < SENS_NWQ; ++i) { const double e = z[2 + i] - pr[X0 + NX * (k + 1) + i]; acc[i] += e * e; }
        acc[SENS_NWQ] += z[0] * z[0];
        acc[SENS_NWQ + 1] += z[1] * z[1];
    }
#pragma unroll
    for (int i = 0; i < SENS_NWT; ++i) lwt[i] = acc[i];
}

// ---- the bounds and the circle radius (mpc_sens_bounds, SensFamBounds) --------------------------------------------------------------------
// The same step against the same factor with a fourth right-hand side.  The bound vector is bv = [lbx (n_w) | ubx (n_w) | fl, fu, ol, ou]: the
// arrays of mpc_set_bounds, lbg[0] / ubg[0] of the friction row and the pair shared by the circle rows (ol is the radius sum); n_b = 2 n_w + 4.
// With SL = z_L / gap_L and SU = z_U / gap_U of a side (what sens_stage_kkt adds to the diagonal; 0 where the side has no bound) a direction
// dbv enters
//   a variable bound of entry i of stage k:  z_L = mu / (x - lb), so d z_L = -SL (dx - dlb): the stationarity row gets  SL dlb + SU dub
//   a_0 (stage 0, input 1): the bounds in force are the snapshot tail's.  A side the presolved friction row set (tighter than the caller's, the
//     test of sens_factor: lb = -amax, ub = amax, amax = sqrt(fu - c)) moves with fu, d lb = dfu / (2 lb), d ub = dfu / (2 ub), and the
//     caller's entry of that side has no effect
//   a circle row:  J dx - t - ds = 0 with t = (SL dol + SU dou) / (SL + SU), the same for every stage and circle: sens_solve_circ's shift (the
//     sides' shares SL / (SL + SU) are formed from the snapshot: the stage data keeps only their sum).  ou = inf: t = dol
//   the friction row where it is kept as a row:  with tf = SL dfl + SU dfu the rows of (a_0, delta_0, v_0) get g tf, g the row's gradient
// An entry whose side has no bound, or whose bound the solve did not impose (fl under friction_lb = nlp; the caller's side of a_0 behind a
// presolved one), has SL = SU = 0: its derivative is 0 and its dbv entry is not read.  The entries are the caller's bounds; the solve relaxes
// them by BOUND_RELAX (1e-8 relative), a factor 1 + 1e-8 at most on a derivative, which is left out.
// An active side carries S ~ 1e10 in the right-hand side and in the matrix alike, as an active circle row does for the centres: the solve is
// sens_solve_circ's with SENS_BV_REFINE step of refinement.  Measured with the harness (tests/sensx/sensx.cpp, sensboundx_solve) on the twelve collision-avoidance rows the tests
// compare (N = 30, nx = 5; every row has active steering-rate bounds and circle rows), the worst |seed' dw - grad_bv' dbv| /
// max(1, sum |seed| max |dw|) over ten directions: one step 1.1e-13, two 2.8e-17, three 2.9e-17; the bound asked of the identity is 1e-10, and
// dw against the active-set reference is the same to every printed digit for one, two and three steps.  (The kernel with one step, over all 70
// rows of that batch: 2.0e-12.)
constexpr int SENS_BV_REFINE = 1;
constexpr int SENS_BV_FL = 0, SENS_BV_FU = 1, SENS_BV_OL = 2, SENS_BV_OU = 3, SENS_BV_ROWS = 4;      // the four row bounds behind lbx | ubx

// z / gap of the two sides of variable i of stage k (0: no bound on that side), and for a side of a_0 the presolved friction row set
// d bound / d fu (cl, cu; 0: the side is the caller's own)
template <int NX>
MPC_HD void sens_var_sides(const Params& P, const double* tail, const double* sn, const int k, const int i, double& SL, double& SU, double& cl,
                           double& cu) {
    using S = Sens<NX>;
    constexpr int NZ = NX + 2;
    double lb = P.LB[k * NZ + i], ub = P.UB[k * NZ + i];
    cl = cu = 0.0;
    if (k == 0 && i == 1) {
        const double a0lb = tail[S::T_A0LB], a0ub = tail[S::T_A0UB];
        if (has_lo(a0lb) && a0lb > lb) cl = 1.0 / (2.0 * a0lb);
        if (has_hi(a0ub) && a0ub < ub) cu = 1.0 / (2.0 * a0ub);
        lb = a0lb; ub = a0ub;
    }
    const double z = sn[S::Z + i];
    SL = has_lo(lb) ? sn[S::ZL + i] / (z - lb) : 0.0;
    SU = has_hi(ub) ? sn[S::ZU + i] / (ub - z) : 0.0;
}
// the shares SL / (SL + SU), SU / (SL + SU) of the two sides of circle row j of a stage (0: no bound on that side)
template <int NX>
MPC_HD void sens_circ_shares(const Params& P, const double* sn, const int j, double& wl, double& wu) {
    using S = Sens<NX>;
    const double s = sn[S::SO + j];
    const double SL = P.has_ol ? sn[S::ZLO + j] / (s - P.ol) : 0.0, SU = P.has_ou ? sn[S::ZUO + j] / (P.ou - s) : 0.0;
    const double tot = SL + SU;
    wl = tot > 0.0 ? SL / tot : 0.0;
    wu = tot > 0.0 ? SU / tot : 0.0;
}
// the kept friction row: z / gap of its two sides and its gradient g wrt (a_0, delta_0, v_0); false where the row is presolved
template <int NX>
MPC_HD bool sens_fric_sides(const Params& P, const double* tail, const double* snap, double& SL, double& SU, double* g) {
    using S = Sens<NX>;
    if (tail[S::T_FROW] == 0.0) return false;
    const double* z0 = snap + S::Z;
    double h[4];
    friction_eval(P, z0[1], z0[2 + 2], z0[2 + 3], g, h, true);
    const double s = tail[S::T_SF];
    SL = P.has_fl ? tail[S::T_ZLF] / (s - P.fl) : 0.0;
    SU = P.has_fu ? tail[S::T_ZUF] / (P.fu - s) : 0.0;
    return true;
}

// forward direction: dbv [n_b] -> dw [n_w].  D: the stage data of sens_obst_setup; nrow, om, work: scratch of sens_solve_circ
template <int NX>
MPC_HD void sens_forward_bounds(const Params& P, double* F, const size_t Bs, const int b, const double* D, const double* snap, const double* dbv,
                                double* dw, const SensVec nrow, const SensVec om, const SensVec work) {
    using S = Sens<NX>;
    constexpr int NZ = NX + 2;
    const int N = P.N, X0 = 2 * N, nw = X0 + NX * (N + 1);
    const double* tail = snap + (size_t)(N + 1) * S::SS;
    const double* dr = dbv + 2 * (size_t)nw;
    sens_solve_circ<NX, SENS_BV_REFINE>(P, F, Bs, b, D,
                        [&](int k, double* gx, double* gu) {
                            const double* sn = snap + (size_t)k * S::SS;
                            gu[0] = gu[1] = 0.0;
#pragma unroll
                            for (int i = 0; i < NZ; ++i) {
                                if (i < 2 && k == N) continue;
                                const int q = i < 2 ? 2 * k + i : X0 + NX * k + (i - 2);
                                double SL, SU, cl, cu, g = 0.0;
                                sens_var_sides<NX>(P, tail, sn, k, i, SL, SU, cl, cu);
                                if (SL != 0.0) g += SL * (cl != 0.0 ? cl * dr[SENS_BV_FU] : dbv[q]);
                                if (SU != 0.0) g += SU * (cu != 0.0 ? cu * dr[SENS_BV_FU] : dbv[nw + q]);
                                if (i < 2) gu[i] = g;
                                else gx[i - 2] = g;
                            }
                            double SL, SU, g[3];
                            if (k == 0 && sens_fric_sides<NX>(P, tail, snap, SL, SU, g)) {
                                double tf = 0.0;
                                if (SL != 0.0) tf += SL * dr[SENS_BV_FL];
                                if (SU != 0.0) tf += SU * dr[SENS_BV_FU];
                                gu[1] += g[0] * tf; gx[2] += g[1] * tf; gx[3] += g[2] * tf;
                            }
                        },
                        [&](int k, int j, const SensCirc&, double*) {
                            double wl, wu, t = 0.0;
                            sens_circ_shares<NX>(P, snap + (size_t)k * S::SS, j, wl, wu);
                            if (wl != 0.0) t += wl * dr[SENS_BV_OL];
                            if (wu != 0.0) t += wu * dr[SENS_BV_OU];
                            return t;
                        },
                        SensNoFin{}, SensVec{dw, 1}, nrow, om, work);
}

// reverse: seed_w [n_w] -> gbv [n_b] = (dw/dbv)' seed_w.  The solve of the seed (every shift t = 0) gives (y_u,k, y_x,k) in sol and the circle
// multipliers n_kj; the transposed right-hand side of the forward direction applied to them: an entry of lbx / ubx gets S y of its variable,
// fu the presolved sides of a_0 through d bound / d fu, fl / fu of a kept row S g' (y_a0, y_delta0, y_v0), ol / ou the sum of their shares of n_kj
template <int NX>
MPC_HD void sens_adjoint_bounds(const Params& P, double* F, const size_t Bs, const int b, const double* D, const double* snap, const double* seed,
                                double* gbv, const SensVec sol, const SensVec nrow, const SensVec om, const SensVec work) {
    using S = Sens<NX>;
    constexpr int NZ = NX + 2;
    const int N = P.N, X0 = 2 * N, nw = X0 + NX * (N + 1);
    const double* tail = snap + (size_t)(N + 1) * S::SS;
    double acc[SENS_BV_ROWS] = {0.0, 0.0, 0.0, 0.0};
    sens_solve_circ<NX, SENS_BV_REFINE>(P, F, Bs, b, D,
                        SensSeedRhs<NX>{seed, N},
                        SensNoShift{},
                        [&](int k, int j, const SensCirc&, const double*, double n) {
                            double wl, wu;
                            sens_circ_shares<NX>(P, snap + (size_t)k * S::SS, j, wl, wu);
                            acc[SENS_BV_OL] += wl * n;
                            acc[SENS_BV_OU] += wu * n;
                        },
                        sol, nrow, om, work);
    for (int k = 0; k <= N; ++k) {
        const double* sn = snap + (size_t)k * S::SS;
#pragma unroll
        for (int i = 0; i < NZ; ++i) {
            if (i < 2 && k == N) continue;
            const int q = i < 2 ? 2 * k + i : X0 + NX * k + (i - 2);
            double SL, SU, cl, cu;
            sens_var_sides<NX>(P, tail, sn, k, i, SL, SU, cl, cu);
            const double y = sol[q];
            if (cl != 0.0) { acc[SENS_BV_FU] += SL * cl * y; SL = 0.0; }
            if (cu != 0.0) { acc[SENS_BV_FU] += SU * cu * y; SU = 0.0; }
            gbv[q] = SL * y;
            gbv[nw + q] = SU * y;
        }
    }
    double SL, SU, g[3];
    if (sens_fric_sides<NX>(P, tail, snap, SL, SU, g)) {
        const double gy = g[0] * sol[1] + g[1] * sol[X0 + 2] + g[2] * sol[X0 + 3];
        acc[SENS_BV_FL] += SL * gy;
        acc[SENS_BV_FU] += SU * gy;
    }
#pragma unroll
    for (int i = 0; i < SENS_BV_ROWS; ++i) gbv[2 * (size_t)nw + i] = acc[i];
}

// lam_bv [n_b] = d f* / d bv (envelope theorem) at the snapshot's iterate, in CasADi's sign and unscaled: z_L / df of a lower side, -z_U / df
// of an upper one, summed over the rows fl / fu / ol / ou bound (the circle rows weighted as sens_lam_obst weights them: the three copies of a
// row together carry m z / df).  A presolved side of a_0 hands its multiplier on to fu through the friction row's gradient at a_0, the very
// quotient mult_stage forms lam_g[0] from (2 a_0 against the 2 lb / 2 ub of the right-hand side: a difference of the order of mu), so that
//   lam_bv[lbx_i] + lam_bv[ubx_i] = -lam_x[i],  lam_bv[fl] + lam_bv[fu] = -lam_g[0],  lam_bv[ol] + lam_bv[ou] = -(sum of lam_g over the circle rows)
// hold to rounding and to what the final iterate leaves of nu = z_U - z_L of a row's slack.
template <int NX>
MPC_HD void sens_lam_bounds(const Params& P, const double* snap, double* lbv) {
    using S = Sens<NX>;
    constexpr int NZ = NX + 2;
    const int N = P.N, X0 = 2 * N, nw = X0 + NX * (N + 1);
    const double* tail = snap + (size_t)(N + 1) * S::SS;
    const double idf = 1.0 / tail[S::T_DF], wm = P.obst_mult / 3.0;
    double acc[SENS_BV_ROWS] = {0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k <= N; ++k) {
        const double* sn = snap + (size_t)k * S::SS;
#pragma unroll
        for (int i = 0; i < NZ; ++i) {
            if (i < 2 && k == N) continue;
            const int q = i < 2 ? 2 * k + i : X0 + NX * k + (i - 2);
            const double lb = P.LB[k * NZ + i], ub = P.UB[k * NZ + i];
            double zl = has_lo(lb) ? sn[S::ZL + i] : 0.0, zu = has_hi(ub) ? sn[S::ZU + i] : 0.0;
            if (k == 0 && i == 1 && tail[S::T_FROW] == 0.0) {
                const double a0lb = tail[S::T_A0LB], a0ub = tail[S::T_A0UB];
                double zr = 0.0, g[3], h[4];
                zl = zu = 0.0;
                if (has_lo(a0lb)) { if (a0lb > lb) zr -= sn[S::ZL + 1]; else zl = sn[S::ZL + 1]; }
                if (has_hi(a0ub)) { if (a0ub < ub) zr += sn[S::ZU + 1]; else zu = sn[S::ZU + 1]; }
                friction_eval(P, sn[S::Z + 1], sn[S::Z + 2 + 2], sn[S::Z + 2 + 3], g, h, true);
                if (g[0] != 0.0) acc[SENS_BV_FU] -= zr * idf / g[0];
            }
            lbv[q] = zl * idf;
            lbv[nw + q] = -(zu * idf);
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (P.has_ol) acc[SENS_BV_OL] += 3.0 * (sn[S::ZLO + j] * idf * wm);
            if (P.has_ou) acc[SENS_BV_OU] -= 3.0 * (sn[S::ZUO + j] * idf * wm);
        }
    }
    if (tail[S::T_FROW] != 0.0) {
        if (P.has_fl) acc[SENS_BV_FL] += tail[S::T_ZLF] * idf;
        if (P.has_fu) acc[SENS_BV_FU] -= tail[S::T_ZUF] * idf;
    }
#pragma unroll
    for (int i = 0; i < SENS_BV_ROWS; ++i) lbv[2 * (size_t)nw + i] = acc[i];
}

// ---- parameter families ----------------------------------------------------------------------------------------------------------------
// What the solves of one instance work on: the factor, the stage data D of sens_obst_setup and the scratch vectors of sens_solve_circ (null
// for a family without CIRC), the instance's snapshot row and its row pr of the solve's p (null where the family does not read it).
template <int NX>
struct SensCtx {
    const Params& P;
    SensInst si;
    double* F;
    size_t Bs;
    int b;
    const double* D;
    const double* snap;
    const double* pr;
    SensVec sol, work, nrow, om;
};
// A family of parameters is a type Fam<NX> with
//   CIRC                    whether its solves are sens_solve_circ's (they need sens_obst_setup's stage data and the scratch vectors)
//   LAM                     whether it has a lam (the p row's is k_sens_lam_p's: another thread mapping)
//   row(N)                  the length of a direction, a gradient and a lam row
//   forward(c, dir, dw)     dir [row] -> dw [n_w]
//   adjoint(c, seed, grad)  seed_w [n_w] -> grad [row] = (dw/d parameter)' seed_w
//   lam(c, out)             out [row] = d/d parameter [f + lam_g' g] at the snapshot's iterate
// over the functions of the sections above.  Those keep their plain arguments: with the bodies taking the context and unpacking it, the same
// arithmetic compiled to 85 more reloads of spilled SGPRs in the bounds' kernel and its directions ran 0.8 % slower.
// sens_family runs a family: it is the body of k_sens<NX, Fam> and of the harness of the tests.
template <int NX>
struct SensFamP {               // the p row [U_ref | X_ref]: n_p = n_w
    static constexpr bool CIRC = false, LAM = false;
    MPC_HD static size_t row(const int N) { return (size_t)2 * N + (size_t)NX * (N + 1); }
    MPC_HD static void forward(const SensCtx<NX>& c, const double* dp, double* dw) { sens_forward<NX>(c.P, c.si, c.F, c.Bs, c.b, dp, dw); }
    MPC_HD static void adjoint(const SensCtx<NX>& c, const double* seed, double* gp) { sens_adjoint<NX>(c.P, c.si, c.F, c.Bs, c.b, seed, gp); }
};
template <int NX>
struct SensFamObst {            // the six obstacle centres
    static constexpr bool CIRC = true, LAM = true;
    MPC_HD static size_t row(int) { return 6; }
    MPC_HD static void forward(const SensCtx<NX>& c, const double* dobst, double* dw) { sens_forward_obst<NX>(c.P, c.F, c.Bs, c.b, c.D, dobst, dw, c.nrow, c.om, c.work); }
    MPC_HD static void adjoint(const SensCtx<NX>& c, const double* seed, double* go) { sens_adjoint_obst<NX>(c.P, c.F, c.Bs, c.b, c.D, seed, go, c.sol, c.nrow, c.om, c.work); }
    MPC_HD static void lam(const SensCtx<NX>& c, double* lo) { sens_lam_obst<NX>(c.P, c.snap, lo); }
};
template <int NX>
struct SensFamWeights {         // the seven cost weights; reads the instance's p row
    static constexpr bool CIRC = true, LAM = true;
    MPC_HD static size_t row(int) { return SENS_NWT; }
    MPC_HD static void forward(const SensCtx<NX>& c, const double* dwt, double* dw) {
        sens_forward_weights<NX>(c.P, c.si, c.F, c.Bs, c.b, c.D, c.snap, c.pr, dwt, dw, c.nrow, c.om, c.work);
    }
    MPC_HD static void adjoint(const SensCtx<NX>& c, const double* seed, double* gwt) {
        sens_adjoint_weights<NX>(c.P, c.si, c.F, c.Bs, c.b, c.D, c.snap, c.pr, seed, gwt, c.sol, c.nrow, c.om, c.work);
    }
    MPC_HD static void lam(const SensCtx<NX>& c, double* lwt) { sens_lam_weights<NX>(c.P, c.snap, c.pr, lwt); }
};
template <int NX>
struct SensFamBounds {          // the bound vector bv: n_b = 2 n_w + 4
    static constexpr bool CIRC = true, LAM = true;
    MPC_HD static size_t row(const int N) { return (size_t)2 * ((size_t)2 * N + (size_t)NX * (N + 1)) + SENS_BV_ROWS; }
    MPC_HD static void forward(const SensCtx<NX>& c, const double* dbv, double* dw) { sens_forward_bounds<NX>(c.P, c.F, c.Bs, c.b, c.D, c.snap, dbv, dw, c.nrow, c.om, c.work); }
    MPC_HD static void adjoint(const SensCtx<NX>& c, const double* seed, double* gbv) {
        sens_adjoint_bounds<NX>(c.P, c.F, c.Bs, c.b, c.D, c.snap, seed, gbv, c.sol, c.nrow, c.om, c.work);
    }
    MPC_HD static void lam(const SensCtx<NX>& c, double* lbv) { sens_lam_bounds<NX>(c.P, c.snap, lbv); }
};

// ---- one instance, one family ------------------------------------------------------------------------------------------------------------
// doubles per instance of the scratch W of a CIRC family: the stage data of sens_obst_setup, then sol, work (n_w each) and nrow, om (3 (N + 1) each)
template <int NX>
MPC_HD size_t sens_obst_scratch_len(int N) { return (size_t)(N + 1) * SensObst<NX>::DS + (size_t)2 * ((size_t)2 * N + (size_t)NX * (N + 1)) + (size_t)6 * (N + 1); }

// Instance b of P.B: factor the final KKT matrix of its snapshot row (F: [stage][entry][B] factor storage), the stage data where the family
// needs it and a direction or a gradient is asked for (W: [sens_obst_scratch_len][B]; null otherwise), then n_dir forward directions
// dir [B, n_dir, row] -> dw [B, n_dir, n_w], one adjoint seed [B, n_w] -> grad [B, row] and lam [B, row], each optional (n_dir = 0, null).
// p [B, n_w]: the p rows of the solve, for a family that reads them.  NaN where the factor failed; returns whether it succeeded.
template <int NX, class Fam>
MPC_HD bool sens_family(const Params& P, const double* snap, double* F, double* W, const double* p, const int b, const int n_dir, const double* dir,
                        double* dw, const double* seed, double* grad, double* lam) {
    const size_t nw = (size_t)2 * P.N + (size_t)NX * (P.N + 1), Bs = (size_t)P.B, nr = Fam::row(P.N);
    const double* sb = snap + (size_t)b * Sens<NX>::len(P.N);
    SensCtx<NX> c{P, sens_factor<NX>(P, sb, F, Bs, b), F, Bs, b, W, sb, p ? p + (size_t)b * nw : nullptr, {}, {}, {}, {}};
    const bool ok = c.si.ok;
    if constexpr (Fam::CIRC) {
        const size_t nn = (size_t)3 * (P.N + 1);
        if (ok && (n_dir > 0 || grad)) sens_obst_setup<NX>(P, sb, W, Bs, b);
        double* V = W + (size_t)(P.N + 1) * SensObst<NX>::DS * Bs + b;
        c.sol = {V, Bs}; c.work = {V + nw * Bs, Bs}; c.nrow = {V + 2 * nw * Bs, Bs}; c.om = {V + (2 * nw + nn) * Bs, Bs};
    }
    for (int d = 0; d < n_dir; ++d) {
        double* o = dw + ((size_t)b * n_dir + d) * nw;
        if (ok) Fam::forward(c, dir + ((size_t)b * n_dir + d) * nr, o);
        else for (size_t q = 0; q < nw; ++q) o[q] = NAN;
    }
    if (grad) {
        double* o = grad + (size_t)b * nr;
        if (ok) Fam::adjoint(c, seed + (size_t)b * nw, o);
        else for (size_t q = 0; q < nr; ++q) o[q] = NAN;
    }
    if constexpr (Fam::LAM) {
        if (lam) {
            double* o = lam + (size_t)b * nr;
            if (ok) Fam::lam(c, o);
            else for (size_t q = 0; q < nr; ++q) o[q] = NAN;
        }
    }
    return ok;
}

}  // namespace mpc
