// tests/emu/emu.cpp -- CPU emulation harness for the HIP kernels (TEST INFRASTRUCTURE, not shipped).
//
// The build container has no GPU.  The per-thread phase functions of the kernels live in
// <package>/csrc/mpc_stage_math.h as __host__ __device__ code; EmuSolve (emu_solve.h) steps them thread by thread in
// the kernels' order, so that the kernel math can be checked against the oracle in the `-m "not gpu"` test suite.
// This harness is its entry point with the mailbox layout, and that of the host-side pieces below.  It is compiled
// into tests/emu/libmpc_emu.so by tests/emu/build.py and is never loaded by the product package.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../motion-planning-for-autonomous-driving-with-mpc_amd/csrc/mpc_closed_loop.h"
#include "../../motion-planning-for-autonomous-driving-with-mpc_amd/csrc/mpc_forces_qp.h"
#include "../../motion-planning-for-autonomous-driving-with-mpc_amd/csrc/mpc_host_common.h"
#include "../../motion-planning-for-autonomous-driving-with-mpc_amd/csrc/mpc_solve_plan.h"
#include "../../motion-planning-for-autonomous-driving-with-mpc_amd/csrc/mpc_stamps.h"
#include "emu_solve.h"

using namespace mpc;

// bx > 0: that many instances per block; trace [trace_rows, 8, B] and n_it may be null
extern "C" int emu_solve_batch(const mpc_problem_desc* desc, const double* lbx, const double* ubx, const double* lbg,
                               const double* ubg, int32_t B, const double* x0, const double* p, const double* obst,
                               double* x_out, int32_t* status, int32_t* iters, double* kkt, double* trace,
                               int32_t trace_rows, int32_t* n_it, int32_t bx) {
    HostProblem hp;
    const int rc = emu_problem(hp, desc, lbx, ubx, lbg, ubg);
    if (rc) return rc;
    EmuOpts o;
    o.obst = obst; o.bx = bx; o.fixed_iters = true; o.trace = trace; o.trace_rows = trace_rows;
    int it;
    if (desc->nx == 5) { EmuSolve<5> e; e.run(hp, B, x0, p, x_out, status, iters, kkt, o); it = e.n_it; }
    else { EmuSolve<6> e; e.run(hp, B, x0, p, x_out, status, iters, kkt, o); it = e.n_it; }
    if (n_it) *n_it = it;
    return MPC_OK;
}
extern "C" void emu_default_desc(mpc_problem_desc* d, int32_t N, int32_t nx) { default_desc(d, N, nx); }

// the launch plan of one solve (mpc_solve_plan.h) for a handle with these options (set as mpc_set_option would) and this state:
// state = [n_cu, xcd_mask, ws_mailbox (-1: as a handle's first solve finds it), pipe_disabled, resc_hint, B, per_inst_obst, trace, in_rescue,
// async_loop]; out = [path (0 one launch per kernel, 1 pipeline, 2 k_solve_wg alone), bx, hyb_bx, hand, Riccati workers per XCD, pipe_help,
// max_rows, mailbox, rescue, XCDs, tiles per XCD, k_solve_wg workgroups, tiles, masked, wg_resc, groups, loop_async, xcd_mask, rows of the
// stage workgroups' LDS stash, dec_s, has_fl, has_fu, has_ol, has_ou, lo_mask, hi_mask, dense_mask, 256-thread stage workgroups]
extern "C" int emu_solve_plan(const mpc_problem_desc* desc, const double* lbx, const double* ubx, const double* lbg, const double* ubg,
                              const char* const* opt_names, const char* const* opt_values, int32_t n_opts, const int64_t* state, int64_t* out) {
    HostProblem hp;
    hp.desc = *desc;
    std::string err;
    Knobs kn;
    for (int i = 0; i < n_opts; ++i)
        if (set_knob(kn, opt_names[i], opt_values[i])) return MPC_ERR_INVALID;
    hp.fric_literal = kn.friction_lb ? 1 : 0;
    int rc = validate_desc(hp.desc, err);
    if (!rc) rc = set_bounds(hp, lbx, ubx, lbg, ubg, err);
    if (rc) return rc;
    PlanState st;
    st.n_cu = (int)state[0]; st.xcd_mask = (uint32_t)state[1]; st.pipe_disabled = state[3] != 0; st.resc_hint = state[4] != 0;
    st.B = (int32_t)state[5]; st.per_inst_obst = state[6] != 0; st.trace = state[7] != 0; st.in_rescue = state[8] != 0; st.async_loop = state[9] != 0;
    st.ws_mailbox = state[2] != 0;
    if (state[2] < 0) st.ws_mailbox = plan_solve(hp, kn, st).mailbox;      // (ensure_ws before the first solve)
    const SolvePlan pl = plan_solve(hp, kn, st);
    const int64_t v[] = {pl.res_path ? 2 : pl.pipe_path ? 1 : 0, pl.bx, pl.hyb_bx, pl.hand, pl.n_ric, pl.pipe_help, (int64_t)pl.max_rows, pl.mailbox,
                         pl.rescue, pl.n_xcd, pl.tiles_x, pl.wg_grid, pl.ntiles, pl.masked, pl.wg_resc, pl.G, pl.loop_async, pl.xcd_mask,
                         pl.stash_rows, dec_s_of(hp), hp.has_fl, hp.has_fu, hp.has_ol, hp.has_ou, hp.lo_mask, hp.hi_mask, hp.dense_mask, pl.small_wg};
    for (size_t i = 0; i < sizeof v / sizeof v[0]; ++i) out[i] = v[i];
    return MPC_OK;
}

// set_bounds (mpc_host_common.h) twice on one problem, as a handle's mpc_set_bounds calls arrive: the first lists must be accepted; returns what
// the second call returned.  same[0] = 1 where the problem is, field for field, what the first call left (LB, UB, the has_* flags and their
// levels, the raw levels, n_mult, n_z, the three masks, bounds_set)
extern "C" int emu_set_bounds_twice(const mpc_problem_desc* desc, const double* const* first, const double* const* second, int32_t* same) {
    HostProblem hp;
    hp.desc = *desc;
    std::string err;
    if (validate_desc(hp.desc, err) || set_bounds(hp, first[0], first[1], first[2], first[3], err)) return MPC_ERR_INVALID;
    const HostProblem was = hp;
    const int rc = set_bounds(hp, second[0], second[1], second[2], second[3], err);
    const auto eq = [](const std::vector<double>& a, const std::vector<double>& b) { return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0); };
    same[0] = eq(hp.LB, was.LB) && eq(hp.UB, was.UB) && hp.has_fl == was.has_fl && hp.has_fu == was.has_fu && hp.has_ol == was.has_ol && hp.has_ou == was.has_ou &&
              hp.fl == was.fl && hp.fu == was.fu && hp.ol == was.ol && hp.ou == was.ou && hp.ol_raw == was.ol_raw && hp.fl_raw == was.fl_raw &&
              hp.n_mult == was.n_mult && hp.n_z == was.n_z && hp.lo_mask == was.lo_mask && hp.hi_mask == was.hi_mask && hp.dense_mask == was.dense_mask &&
              hp.bounds_set == was.bounds_set && !(rc && err.empty());
    return rc;
}

// what solve_dev does behind a launch (mpc_solve_plan.h: after_solve): in = [pl.rescue, failed, resc_ran, resc_in_kernel, rescued_in_kernel];
// out = [run_rescue, set_hint, hint]
extern "C" void emu_after_solve(const int64_t* in, int64_t* out) {
    SolvePlan pl{};
    pl.rescue = in[0] != 0;
    SolveOutcome o;
    o.failed = (uint32_t)in[1]; o.resc_ran = in[2] != 0; o.resc_in_kernel = in[3] != 0; o.rescued_in_kernel = (int)in[4];
    const AfterSolve a = after_solve(pl, o);
    out[0] = a.run_rescue; out[1] = a.set_hint; out[2] = a.hint;
}

// closed-loop driver pieces (mpc_closed_loop.h) on host arrays: mode 0 = setup, 1 = advance after step i
extern "C" int emu_closed_loop_piece(int32_t mode, int32_t i, double dt, double wheelbase, int32_t B, int32_t N, int32_t L, int32_t Lp,
                                     const double* init_state, const double* path, const double* orient, const double* vdes,
                                     double* state, double* x0, double* p, const double* x_out, const int32_t* status,
                                     double* traj, double* ctrl, int32_t* step_status, int32_t nx, int32_t noise_mode, double sigma, uint64_t seed) {
    LoopArgs A{};
    A.B = B; A.N = N; A.L = L; A.Lp = Lp;
    A.nx = nx; A.noise_mode = noise_mode; A.sigma = sigma; A.seed_lo = (uint32_t)seed; A.seed_hi = (uint32_t)(seed >> 32);
    A.init_state = init_state; A.path = path; A.orient = orient; A.vdes = vdes;
    A.state = state; A.x0 = x0; A.p = p; A.x_out = x_out; A.status = status; A.traj = traj; A.ctrl = ctrl; A.step_status = step_status;
    Params P{};
    P.dt = dt; P.wheelbase = wheelbase; P.nx = nx;
    for (int b = 0; b < B; ++b) {
        if (mode == 0) loop_setup_instance(A, b);
        else loop_advance_instance(P, A, b, i);
    }
    return 0;
}

// pieces of the FORCES-mode closed loop (mpc_closed_loop.h): mode 0 setup, 1 parameters of step k, 2 advance after solve k
extern "C" int emu_forces_loop_piece(int32_t mode, int32_t k, double dt, double wheelbase, int32_t B, int32_t N, int32_t L, int32_t Lp,
                                     const double* init_state, const double* init_acc, const double* path, const double* orient, const double* vdes,
                                     const double* obstacle, double* state, double* zbar, double* params, const double* z_out, const int32_t* exitflag,
                                     double* traj, double* ctrl, int32_t* step_flag, int32_t noise_mode, double sigma, uint64_t seed) {
    ForcesLoopArgs A{};
    A.B = B; A.N = N; A.L = L; A.Lp = Lp;
    A.init_state = init_state; A.init_acc = init_acc; A.path = path; A.orient = orient; A.vdes = vdes;
    for (int i = 0; i < 6; ++i) A.obstacle[i] = obstacle[i];
    A.state = state; A.zbar = zbar; A.params = params; A.z_out = z_out; A.exitflag = exitflag; A.traj = traj; A.ctrl = ctrl; A.step_flag = step_flag;
    A.dt = dt; A.wheelbase = wheelbase; A.noise_mode = noise_mode; A.sigma = sigma; A.seed_lo = (uint32_t)seed; A.seed_hi = (uint32_t)(seed >> 32);
    for (int b = 0; b < B; ++b) {
        if (mode == 0) forces_loop_setup_instance(A, b);
        else if (mode == 1) forces_loop_params_instance(A, b, k);
        else forces_loop_advance_instance(A, b, k);
    }
    return 0;
}

// FORCES-mode SQP step (mpc_forces_qp.h), one instance after the other on host arrays
extern "C" int emu_forces_solve(int32_t B, int32_t N, double dt, double l, double wb, double rho, const double* Q, const double* R,
                                const double* Pt, const double* lb, const double* ub, const double* hl, const double* hu, int32_t hessian_mode,
                                const double* zbar, const double* params, const double* xinit, double* z_out, int32_t* iters,
                                int32_t* status, double* kkt) {
    ForcesQpArgs A{};
    A.B = B; A.Bp = B; A.N = N; A.max_it = 60;
    A.dt = dt; A.l = l; A.wb = wb; A.rho = rho; A.tol = 1e-4; A.tol_mu = 1e-6;
    for (int i = 0; i < 5; ++i) { A.Q[i] = Q[i]; A.Pt[i] = Pt[i]; }
    A.R[0] = R[0]; A.R[1] = R[1];
    forces_hessian_diag(hessian_mode, A.Q, A.R, A.Pt, A.hd, A.hdN);
    for (int i = 0; i < 7; ++i) { A.lb[i] = lb[i]; A.ub[i] = ub[i]; }
    for (int i = 0; i < 10; ++i) { A.hl[i] = hl[i]; A.hu[i] = hu[i]; }
    A.zbar = zbar; A.params = params; A.xinit = xinit; A.z_out = z_out; A.iters = iters; A.status = status; A.kkt = kkt;
    std::vector<double> ws((size_t)FQ_ROWS * N * B, 0.0);
    A.ws = ws.data();
    for (int b = 0; b < B; ++b) forces_qp_instance(A, b);
    return 0;
}

// the stamp reports of option timing (mpc_stamps.h) over host rows: 0 k_start, 1 k_solve_wg, 2 k_pipeline, 3 one launch per kernel (n blocks, n2
// tiles), 4 wg_trace; the text goes to out (cap bytes), its length is returned
extern "C" int emu_stamp_report(int32_t which, const unsigned long long* rows, int32_t n, int32_t n2, char* out, int32_t cap) {
    const std::string s = which == 0 ? format_start_timing(rows, n) : which == 1 ? format_wg_timing(rows, n) : which == 2 ? format_pipe_timing(rows, n)
                        : which == 3 ? format_stage_timing(rows, n, n2) : format_wg_trace(rows, n);
    if ((int)s.size() >= cap) return -1;
    memcpy(out, s.c_str(), s.size() + 1);
    return (int)s.size();
}

// SolveIo::rows (mpc_solve_plan.h) for a problem of N stages and nx states: the ten row members in declaration order (x0, p, obst, x_out, status,
// iters, kkt, lam_g, lam_x, snap) point `at[i]` bytes into `base` (negative: null); out[0] = B of the slice, out[1 + i] = how many elements of
// its own type member i moved (-1: it is null in the slice).  Nothing is dereferenced.
extern "C" int emu_solve_io_rows(int32_t N, int32_t nx, int64_t snap_len, int32_t B, char* base, const int64_t* at, int64_t off, int32_t n, int64_t* out) {
    HostProblem hp;
    hp.desc.N = N; hp.desc.nx = nx;
    SolveIo io;
    io.B = B; io.n_w = hp.n_w(); io.n_g = hp.n_g(); io.snap_len = (size_t)snap_len;
    const auto ptr = [&](int i) { return at[i] < 0 ? nullptr : base + at[i]; };
    io.x0 = (const double*)ptr(0); io.p = (const double*)ptr(1); io.obst = (const double*)ptr(2); io.x_out = (double*)ptr(3);
    io.status = (int32_t*)ptr(4); io.iters = (int32_t*)ptr(5); io.kkt = (double*)ptr(6); io.lam_g = (double*)ptr(7); io.lam_x = (double*)ptr(8);
    io.snap = (double*)ptr(9);
    const SolveIo r = io.rows((size_t)off, n);
    out[0] = r.B;
    out[1] = r.x0 ? r.x0 - io.x0 : -1; out[2] = r.p ? r.p - io.p : -1; out[3] = r.obst ? r.obst - io.obst : -1; out[4] = r.x_out ? r.x_out - io.x_out : -1;
    out[5] = r.status ? r.status - io.status : -1; out[6] = r.iters ? r.iters - io.iters : -1; out[7] = r.kkt ? r.kkt - io.kkt : -1;
    out[8] = r.lam_g ? r.lam_g - io.lam_g : -1; out[9] = r.lam_x ? r.lam_x - io.lam_x : -1; out[10] = r.snap ? r.snap - io.snap : -1;
    return 0;
}

// A LoopIo (mpc_solve_plan.h) from the harness: dims = [B, L, Lp, Lt, M, per_ego, noise_mode, tracked]; the fifteen array members in the order
// init_state, path, orient, vdes, track, offsets, traj, ctrl, step_status, clearance, nearest, chosen, kgain, wgain, ogain point `at[i]` bytes into
// `base` (negative: null).  Nothing is dereferenced.
static LoopIo emu_loop_io(const int32_t* dims, double sigma, double offset, char* base, const int64_t* at) {
    const auto ptr = [&](int i) { return at[i] < 0 ? nullptr : base + at[i]; };
    LoopIo io;
    io.B = dims[0]; io.L = dims[1]; io.Lp = dims[2]; io.Lt = dims[3]; io.M = dims[4]; io.per_ego = dims[5]; io.noise_mode = dims[6]; io.tracked = dims[7] != 0;
    io.sigma = sigma; io.offset = offset;
    io.init_state = (const double*)ptr(0); io.path = (const double*)ptr(1); io.orient = (const double*)ptr(2); io.vdes = (const double*)ptr(3);
    io.track = (const double*)ptr(4); io.offsets = (const double*)ptr(5); io.traj = (double*)ptr(6); io.ctrl = (double*)ptr(7);
    io.step_status = (int32_t*)ptr(8); io.clearance = (double*)ptr(9); io.nearest = (int32_t*)ptr(10); io.chosen = (int32_t*)ptr(11);
    io.kgain = (double*)ptr(12); io.wgain = (double*)ptr(13); io.ogain = (double*)ptr(14);
    return io;
}
// LoopIo::each_array under a horizon of N stages, in the order it visits the arrays: where[i] = the offset in `base` of the i-th member visited (-1:
// null), bytes[i] = its size, written[i] = the loop writes it.  Returns the number of arrays visited, negative if that is not LoopIo::N_ARRAYS.
extern "C" int emu_loop_io_arrays(const int32_t* dims, int32_t N, char* base, const int64_t* at, int64_t* where, int64_t* bytes, int32_t* written) {
    LoopIo io = emu_loop_io(dims, 0.0, 0.0, base, at);
    int n = 0;
    io.each_array(N, [&](auto*& m, bool out, size_t b) {
        where[n] = m ? (const char*)m - base : -1;
        bytes[n] = (int64_t)b;
        written[n++] = out;
    });
    return n == (int)LoopIo::N_ARRAYS ? n : -n;
}
// loop_refusal (mpc_solve_plan.h): the text into out (cap bytes), its length returned; 0: nothing is refused
extern "C" int emu_loop_refusal(const int32_t* dims, double sigma, double offset, char* base, const int64_t* at, int32_t N, char* out, int32_t cap) {
    const char* bad = loop_refusal(emu_loop_io(dims, sigma, offset, base, at), N);
    if (!bad) return 0;
    snprintf(out, (size_t)cap, "%s", bad);
    return (int)strlen(bad);
}
