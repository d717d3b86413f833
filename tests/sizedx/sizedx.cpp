// tests/sizedx/sizedx.cpp -- CPU harness of the sized solve (TEST INFRASTRUCTURE, not shipped).
//
// Calls, on the CPU, what the kernels of mpc_solve_batch_sized run on the GPU, from the shipped headers: sized_pack and the sized transposer's
// element functions obst_xs_read / obst_xs_write stepped as k_transpose_obst_sized steps them, load_obst in sized mode on the rows they leave
// (mpc_stage_math.h), plan_solve with the sized obstacle mode (mpc_solve_plan.h) -- and the emulated solve with a lower bound per circle row:
// EmuSolve (tests/emu/emu_solve.h), unchanged, whose calls that depend on the obstacle mode -- ws_layout, fill_params, the stage context and the
// five phases that take a circle row's value -- are redirected while its header is read, as tests/trafx does for the per-stage mode.  Built by
// tests/helpers.py (harness_lib) with g++.
#include <cstdint>
#include <limits>
#include <string>
#include <vector>

#include "../../motion-planning-for-autonomous-driving-with-mpc_amd/csrc/mpc_closed_loop.h"
#include "../../motion-planning-for-autonomous-driving-with-mpc_amd/csrc/mpc_solve_plan.h"

namespace mpc {
// k_sized_pack, then k_transpose_obst_sized stepped on the CPU: grid (tiles, chunks of OBST_XS_KC stages), `threads` threads whose trip runs in
// ascending or descending thread order; obst [B, N+1, 6], rsum [B, N+1, 3] -> the obstacle section of ws
static void sized_rows_in(int N, int nx, int B, bool mailbox, int descending, int threads, const double* obst, const double* rsum, double ol_raw,
                          double scale, double* ws) {
    const int S = N + 1;
    std::vector<double> rows((size_t)B * S * OBST_SIZED_ROWS);
    for (size_t e = (size_t)B * S; e-- > 0;) sized_pack(obst, rsum, rows.data(), e);
    const WsLayout w = ws_layout(N, nx, ((size_t)B + 63) / 64 * 64, mailbox, 2);
    const ObstXposeSized X{rows.data(), ws + w.OBST * 64, B, S, (uint32_t)w.tile_elems, ol_raw, BOUND_RELAX, scale};
    std::vector<ObstPair> lds((size_t)64 * OBST_XS_LD);
    for (int tl = 0; tl < (int)w.ntiles; ++tl)
        for (int k0 = 0; k0 <= N; k0 += OBST_XS_KC) {
            const double nan = std::numeric_limits<double>::quiet_NaN();
            for (ObstPair& q : lds) q = ObstPair{nan, nan};
            const int n = obst_xs_count(X, k0);
            for (int pass = 0; pass < 2; ++pass)            // (the barrier between the two trips)
                for (int j = 0; j < threads; ++j) {
                    const int t = descending ? threads - 1 - j : j;
                    for (int e = t; e < n; e += threads) {
                        if (pass == 0) obst_xs_read(X, tl, k0, e, lds.data());
                        else obst_xs_write(X, tl, k0, e, lds.data());
                    }
                }
        }
}

static const double *g_obst = nullptr, *g_rsum = nullptr;      // [B, N+1, 6], [B, N+1, 3] of the solve that is running
inline WsLayout ws_layout_sized(int N, int nx, size_t Bp, bool mailbox) { return ws_layout(N, nx, Bp, mailbox, 2); }
inline void fill_params_sized(Params& P, const HostProblem& hp, int B, size_t Bp, int bx, double* base, int32_t* ibase, const double* dLB,
                              const double* dUB, bool mailbox) {
    fill_params(P, hp, B, Bp, bx, base, ibase, dLB, dUB, mailbox, 2);
    P.per_inst_obst = OBST_PER_STAGE_SIZED;
    sized_rows_in(hp.desc.N, hp.desc.nx, B, mailbox, 0, 256, g_obst, g_rsum, hp.ol_raw, 1.0, base);
}
// the phases EmuSolve names, in the instantiations a sized solve runs (the mask 0xFF | VM_SIZED), on the context that holds the offsets
constexpr uint32_t SV = 0xFFu | VM_SIZED;
template <int NX> inline void phase_init_point_sized(const PRef& P, CtxSized<NX>& c, Red0& r) { phase_init_point<NX, true, true>(P, c, r); }
template <int NX> inline void phase_preload_sized(const PRef& P, CtxSized<NX>& c, PreTmp<NX>& t) { phase_preload<NX, false, SV>(P, c, t); }
template <int NX> inline void phase_premath_sized(const PRef& P, CtxSized<NX>& c, const PreTmp<NX>& t) { phase_premath<NX, SV>(P, c, t); }
template <int NX> inline void phase_trial_eval_sized(const PRef& P, CtxSized<NX>& c, Red2& r) { phase_trial_eval<NX, SV>(P, c, r); }
template <int NX, bool REUSE> inline void phase_eval_assemble_sized(const PRef& P, CtxSized<NX>& c, Red3& r) { phase_eval_assemble<NX, REUSE, false, SV>(P, c, r); }
}  // namespace mpc
#define ws_layout(...) ws_layout_sized(__VA_ARGS__)
#define fill_params(...) fill_params_sized(__VA_ARGS__)
#define Ctx CtxSized
#define phase_init_point phase_init_point_sized
#define phase_preload phase_preload_sized
#define phase_premath phase_premath_sized
#define phase_trial_eval phase_trial_eval_sized
#define phase_eval_assemble phase_eval_assemble_sized
#include "../emu/emu_solve.h"
#undef ws_layout
#undef fill_params
#undef Ctx
#undef phase_init_point
#undef phase_preload
#undef phase_premath
#undef phase_trial_eval
#undef phase_eval_assemble

using namespace mpc;

template <int NX>
static void load_all(int32_t N, int32_t B, const double* ws, double* out) {
    HostProblem hp;
    default_desc(&hp.desc, N, NX);
    const size_t Bp = ((size_t)B + 63) / 64 * 64;
    Params P;
    fill_params(P, hp, B, Bp, 4, const_cast<double*>(ws), nullptr, nullptr, nullptr, false, 2);
    P.per_inst_obst = OBST_PER_STAGE_SIZED;
    for (int b = 0; b < B; ++b)
        for (int k = 0; k <= N; ++k) {
            CtxSized<NX> c{};
            c.b = b; c.k = k;
            load_obst<NX, false, true, true>(P, c);
            double* o = out + ((size_t)b * (N + 1) + k) * 9;
            for (int i = 0; i < 6; ++i) o[i] = c.obst[i];
            for (int j = 0; j < 3; ++j) o[6 + j] = c.od[j];
        }
}

extern "C" {

// doubles of the workspace (no mailbox) with the sized obstacle section for B instances; where the section starts; its rows per stage
int64_t sizedx_ws_total(int32_t N, int32_t nx, int32_t B) { return (int64_t)ws_layout(N, nx, ((size_t)B + 63) / 64 * 64, false, 2).total; }
int32_t sizedx_rows_per_stage() { return OBST_SIZED_ROWS; }
// element of (row, b) of the obstacle section
int64_t sizedx_obst_index(int32_t N, int32_t nx, int32_t B, int32_t row, int32_t b) {
    const WsLayout w = ws_layout(N, nx, ((size_t)B + 63) / 64 * 64, false, 2);
    Params P{};
    P.tile_elems = (uint32_t)w.tile_elems;
    return (int64_t)(w.OBST * 64) + (int64_t)ws_index(P, (const double*)nullptr, (uint32_t)row, (uint32_t)b);
}
// sizes of the layout with no per-stage section, with the per-stage one, with the sized one: [rows, tile_elems, total, OBST] x 3
void sizedx_layouts(int32_t N, int32_t nx, int32_t B, int32_t mailbox, int64_t* out) {
    for (int os = 0; os < 3; ++os) {
        const WsLayout w = ws_layout(N, nx, ((size_t)B + 63) / 64 * 64, mailbox != 0, os);
        out[4 * os] = (int64_t)w.rows; out[4 * os + 1] = (int64_t)w.tile_elems; out[4 * os + 2] = (int64_t)w.total; out[4 * os + 3] = (int64_t)w.OBST;
    }
}
// pack + transposer: ws (sizedx_ws_total doubles) is touched in the obstacle section only
void sizedx_transpose(int32_t N, int32_t nx, int32_t B, int32_t descending, int32_t threads, const double* obst, const double* rsum, double ol_raw,
                      double scale, double* ws) {
    sized_rows_in(N, nx, B, false, descending, threads, obst, rsum, ol_raw, scale, ws);
}
// load_obst in sized mode on such a workspace: out [B, N+1, 9] -- six centres and three offsets (x scale) as stage thread (b, k) holds them
void sizedx_load(int32_t N, int32_t nx, int32_t B, const double* ws, double* out) {
    if (nx == 5) load_all<5>(N, B, ws, out); else load_all<6>(N, B, ws, out);
}
// what one launch of k_loop_traffic_sized(.., i) does: loop_traffic_stage_sized, one call per (ego, stage) in the kernel's thread numbering, ascending
// or descending; rows [B, N+1, OBST_SIZED_ROWS] packed (centres, the slots' radius sums, a pad), clearance / nearest [B, L] (column i), chosen
// [B, L, N+1, 3] (block i); any of the last three may be null
void sizedx_traffic_step(int32_t descending, int32_t B, int32_t L, int32_t Lt, int32_t nx, int32_t N, int32_t M, int32_t per_ego, int32_t pairing,
                         double ego_offset, const double* desc_obst, const double* tracks, const double* offsets, const double* rsums, const double* state,
                         const double* x0, double r_sum, int32_t i, double* rows, double* clearance, int32_t* nearest, int32_t* chosen) {
    LoopTrafficSizedArgs A{};
    A.T.B = B; A.T.L = L; A.T.Lt = Lt; A.T.nx = nx; A.T.N = N; A.T.M = M; A.T.per_ego = per_ego; A.T.pairing = pairing;
    A.T.tracks = tracks; A.T.offsets = offsets; A.T.ego_offset = ego_offset; A.T.obst = rows; A.T.state = state; A.T.x0 = x0;
    A.T.clearance = clearance; A.T.nearest = nearest; A.T.chosen = chosen; A.T.r_sum = r_sum; A.rsums = rsums;
    for (int q = 0; q < 6; ++q) A.T.desc_obst[q] = desc_obst[q];
    const int S = N + 1, T = B * S;
    for (int n = 0; n < T; ++n) {
        const int t = descending ? T - 1 - n : n;
        loop_traffic_stage_sized(A, t / S, t % S, i);
    }
}
// what relax_lo makes of a bound (the host's, mpc_host_common.h)
double sizedx_relax_lo(double lo) { return relax_lo(lo); }

// the solve kernels' phase functions stepped by EmuSolve in the instantiations of a sized solve, rsum [B, N+1, 3] beside obst [B, N+1, 6]
// (the per-stage sibling the identity is against: tests/trafx, trafx_solve_stages)
int sizedx_solve(const mpc_problem_desc* desc, const double* lbx, const double* ubx, const double* lbg, const double* ubg, int32_t B,
                 const double* x0, const double* p, const double* obst, const double* rsum, double* x_out, int32_t* status, int32_t* iters, double* kkt) {
    HostProblem hp;
    const int rc = emu_problem(hp, desc, lbx, ubx, lbg, ubg);
    if (rc) return rc;
    g_obst = obst; g_rsum = rsum;
    if (desc->nx == 5) { EmuSolve<5> e; e.run(hp, B, x0, p, x_out, status, iters, kkt); }
    else { EmuSolve<6> e; e.run(hp, B, x0, p, x_out, status, iters, kkt); }
    g_obst = g_rsum = nullptr;
    return MPC_OK;
}

// plan_solve as tests/predx's predx_solve_plan calls it (same options, same state vector, the obstacle mode given): every field of the plan a
// per-stage solve is compared on, then `sized`: out[0 .. SIZEDX_PLAN_FIELDS)
constexpr int SIZEDX_PLAN_FIELDS = 47;
int sizedx_plan_fields() { return SIZEDX_PLAN_FIELDS; }
int sizedx_solve_plan(const mpc_problem_desc* desc, const double* lbx, const double* ubx, const double* lbg, const double* ubg,
                      const char* const* opt_names, const char* const* opt_values, int32_t n_opts, const int64_t* state, int32_t obst_mode, int64_t* out) {
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
    st.B = (int32_t)state[5]; st.per_inst_obst = obst_mode; st.trace = state[7] != 0; st.in_rescue = state[8] != 0; st.async_loop = state[9] != 0;
    st.ws_mailbox = state[2] != 0;
    if (state[2] < 0) st.ws_mailbox = plan_solve(hp, kn, st).mailbox;
    const SolvePlan pl = plan_solve(hp, kn, st);
    const int64_t v[SIZEDX_PLAN_FIELDS] = {
        pl.small_wg, pl.S, pl.bx, pl.threads, pl.nblk, pl.ntiles, pl.G, pl.stash_rows, (int64_t)pl.lds_bytes, (int64_t)pl.lds_init, (int64_t)pl.ric_lds,
        pl.masked, pl.cap, pl.chunk, pl.polled, pl.fused, (int64_t)pl.lds_pre, (int64_t)pl.lds_start, pl.res_path, pl.pipe_path, pl.hyb_bx,
        pl.resc_alone, pl.hyb_ok, pl.hand, pl.wg_resc, (int64_t)pl.wg_lds, pl.wg_grid, pl.xcd_mask, pl.n_xcd, pl.tiles_x, pl.cu_x, pl.n_ric,
        pl.pipe_cap, pl.pipe_help, pl.pipe_lead, pl.mbw_live, pl.stage_timing, pl.start_timing, pl.wg_timing, pl.wg_trace, pl.pipe_timing,
        pl.poison, (int64_t)pl.max_rows, pl.mailbox, pl.rescue, pl.loop_async, pl.sized};
    for (int i = 0; i < SIZEDX_PLAN_FIELDS; ++i) out[i] = v[i];
    return MPC_OK;
}

}  // extern "C"
