// tests/floopx/floopx.cpp -- CPU harness of the FORCES-mode closed loop past per-ego obstacles (TEST INFRASTRUCTURE, not shipped).
//
// Calls the functions of <package>/csrc/mpc_closed_loop.h that k_floop_turn_setup and k_floop_turn run on the GPU -- forces_turn_setup_row and
// forces_turn_row, one call per (instance, stage) as the kernels' threads do -- and, for whole loops, forces_qp_instance (mpc_forces_qp.h) as the
// solve between two turns.  Built by tests/test_forces_loop_obst_cpu.py with g++ into a temporary directory.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../motion-planning-for-autonomous-driving-with-mpc_amd/csrc/mpc_closed_loop.h"
#include "../../motion-planning-for-autonomous-driving-with-mpc_amd/csrc/mpc_forces_qp.h"

using namespace mpc;

// the inputs of a loop, as the entry point gets them
struct FloopxIn {
    int32_t B, N, L, Lp, guess_mode, Lt, predict, noise_mode;
    const double *init_state, *init_acc, *path, *orient, *vdes, *track, *obstacle;
    double offset, r_sum, ego_offset, dt, wheelbase, sigma;
    uint64_t seed;
};

static ForcesTurnArgs turn_args(const FloopxIn& in, double* state, double* zbar, double* params, const double* z_out, const int32_t* exitflag, double* traj,
                                double* ctrl, int32_t* step_flag, double* clearance) {
    ForcesTurnArgs A{};
    ForcesLoopArgs& F = A.F;
    F.B = in.B; F.N = in.N; F.L = in.L; F.Lp = in.Lp;
    F.init_state = in.init_state; F.init_acc = in.init_acc; F.path = in.path; F.orient = in.orient; F.vdes = in.vdes;
    for (int i = 0; i < 6; ++i) F.obstacle[i] = in.obstacle ? in.obstacle[i] : 0.0;
    F.state = state; F.zbar = zbar; F.params = params; F.z_out = z_out; F.exitflag = exitflag; F.traj = traj; F.ctrl = ctrl; F.step_flag = step_flag;
    F.dt = in.dt; F.wheelbase = in.wheelbase; F.noise_mode = in.noise_mode; F.sigma = in.sigma; F.seed_lo = (uint32_t)in.seed; F.seed_hi = (uint32_t)(in.seed >> 32);
    A.guess_mode = in.guess_mode; A.Lt = in.Lt; A.predict = in.predict; A.track = in.track; A.offset = in.offset;
    A.clearance = clearance; A.r_sum = in.r_sum; A.ego_offset = in.ego_offset;
    return A;
}
// every thread of one launch, in ascending (reverse = 0) or descending order: no thread reads what another writes, so the order must not matter
template <class Fn>
static void all_threads(const FloopxIn& in, int reverse, Fn&& fn) {
    const int n = in.B * in.N;
    for (int q = 0; q < n; ++q) {
        const int t = reverse ? n - 1 - q : q;
        fn(t / in.N, t % in.N);
    }
}

extern "C" {

// one launch of k_floop_turn_setup (k < 0) or of k_floop_turn(.., k)
void floopx_launch(const FloopxIn* in, int32_t k, int32_t reverse, double* state, double* zbar, double* params, const double* z_out, const int32_t* exitflag,
                   double* traj, double* ctrl, int32_t* step_flag, double* clearance) {
    const ForcesTurnArgs A = turn_args(*in, state, zbar, params, z_out, exitflag, traj, ctrl, step_flag, clearance);
    if (k < 0) all_threads(*in, reverse, [&](int b, int j) { forces_turn_setup_row(A, b, j); });
    else all_threads(*in, reverse, [&](int b, int j) { forces_turn_row(A, b, j, k); });
}

// the first `steps` steps of the loop as mpc_forces_closed_loop_batch_obst_dev enqueues it: setup, then solve and turn per step.  log_zbar [steps,B,N,7],
// log_params [steps,B,N,10]: the guess and the parameters every solve saw, or null
int floopx_loop(const FloopxIn* in, int32_t steps, const double* Q, const double* R, const double* Pt, double friction_div, const double* lb, const double* ub,
                const double* hl, const double* hu, int32_t hessian_mode, double* traj, double* ctrl, int32_t* step_flag, double* clearance, double* log_zbar,
                double* log_params) {
    const int B = in->B, N = in->N;
    std::vector<double> state((size_t)B * 5), zbar((size_t)B * N * 7), params((size_t)B * N * 10), z_out((size_t)B * N * 7), kkt(B), ws((size_t)FQ_ROWS * N * B, 0.0);
    std::vector<int32_t> flag(B), iters(B);
    ForcesQpArgs S{};
    S.B = B; S.Bp = B; S.N = N; S.max_it = 60;
    S.dt = in->dt; S.l = in->wheelbase; S.wb = friction_div; S.rho = in->ego_offset; S.tol = 1e-4; S.tol_mu = 1e-6;
    for (int i = 0; i < 5; ++i) { S.Q[i] = Q[i]; S.Pt[i] = Pt[i]; }
    S.R[0] = R[0]; S.R[1] = R[1];
    forces_hessian_diag(hessian_mode, S.Q, S.R, S.Pt, S.hd, S.hdN);
    for (int i = 0; i < 7; ++i) { S.lb[i] = lb[i]; S.ub[i] = ub[i]; }
    for (int i = 0; i < 10; ++i) { S.hl[i] = hl[i]; S.hu[i] = hu[i]; }
    S.zbar = zbar.data(); S.params = params.data(); S.xinit = state.data(); S.z_out = z_out.data(); S.iters = iters.data(); S.status = flag.data(); S.kkt = kkt.data();
    S.ws = ws.data();
    const ForcesTurnArgs A = turn_args(*in, state.data(), zbar.data(), params.data(), z_out.data(), flag.data(), traj, ctrl, step_flag, clearance);
    all_threads(*in, 0, [&](int b, int j) { forces_turn_setup_row(A, b, j); });
    for (int k = 0; k < steps; ++k) {
        if (log_zbar) memcpy(log_zbar + (size_t)k * zbar.size(), zbar.data(), zbar.size() * 8);
        if (log_params) memcpy(log_params + (size_t)k * params.size(), params.data(), params.size() * 8);
        for (int b = 0; b < B; ++b) forces_qp_instance(S, b);
        all_threads(*in, k & 1, [&](int b, int j) { forces_turn_row(A, b, j, k); });
    }
    return 0;
}

}  // extern "C"
