// mpc_stage_math.h -- per-thread math of the batched interior-point solver (product code).
//
// Every function here is the body of one *phase* of a HIP kernel for ONE thread, written as
// `__host__ __device__` so that the very same source is (a) inlined into the gfx950 kernels of
// mpc_kernels.hip and (b) stepped thread-by-thread by the CPU emulation harness used in tests
// (tests/emu/), which exists because the build container has no GPU.  The emulation harness is test
// infrastructure only; the shipped library (libmpcgpu.so) contains no CPU solve path.
//
// Problem solved (reference: MPC_Planner/optimizer.py, CasadiOptimizer):
//   decision vector / parameters ........ optimizer.py:550,552
//   cost ................................. optimizer.py:507-511
//   constraints g ........................ optimizer.py:378-403   (friction | x0 pin | Euler defects | obstacle)
//   bounds ............................... optimizer.py:421-491
//   ODE .................................. configuration.py:353-368
//   circle geometry ...................... configuration.py:69-93
//   the call being replaced .............. optimizer.py:607   sol(x0=,p=,lbg=,lbx=,ubg=,ubx=)
//
// Data layout in HBM: tile-major structure-of-arrays with interleaved row pairs, [tile of 64 instances][row pair]
// [instance][2] (mpc_prow below): a wavefront working on consecutive instances of one horizon stage reads contiguous
// 16-byte elements.  Rows are (stage k, component i) pairs.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MPC_HD __host__ __device__ __forceinline__
#else
#define MPC_HD inline
#endif

// Device code addresses the SoA workspace through ONE buffer resource descriptor (SRSRC, 4 SGPRs) with
//   soffset (SGPR)  = byte offset of the array inside the workspace (uniform),
//   voffset (VGPR)  = the instance's 32-bit byte offset inside its tile (+ the tile's base),
// i.e. buffer_load / buffer_store (dwordx2, or dwordx4 for a row pair) instead of flat accesses with 64-bit VGPR addresses: kernel-argument
// pointers that arrive inside a by-value struct are otherwise treated as generic pointers (2-3 VALU of 64-bit
// address arithmetic per access, no scalar-base addressing).  The workspace is < 4 GiB (checked on the host);
// out-of-range accesses are dropped by the hardware bounds check.  On the host (emulation harness) the same macros
// are plain array indexing.
#if defined(__HIP_DEVICE_COMPILE__)
#define MPC_GLOBAL_AS __attribute__((address_space(1)))
#else
#define MPC_GLOBAL_AS
#endif
// plain global-pointer access (small tables and the caller's row-major buffers)
#define MPC_GP(ptr, idx) (((MPC_GLOBAL_AS __typeof__(*(ptr))*)(ptr))[(uint32_t)(idx)])

namespace mpc {

// ---- IPOPT default constants (Waechter & Biegler 2006) -------------------------------------------------
constexpr double MU_INIT = 0.1, KAPPA_EPS = 10.0, KAPPA_MU = 0.2, THETA_MU = 1.5, TAU_MIN = 0.99;
constexpr double KAPPA_1 = 1e-2, KAPPA_2 = 1e-2, S_MAX = 100.0, KAPPA_SIGMA = 1e10;
constexpr double GAMMA_THETA = 1e-5, GAMMA_PHI = 1e-8, LS_DELTA = 1.0, S_THETA = 1.1, S_PHI = 2.3;
constexpr double ETA_PHI = 1e-8, GAMMA_ALPHA = 0.05;
constexpr double DW_MIN = 1e-20, DW_0 = 1e-4, DW_MAX = 1e40, KW_MINUS = 1.0 / 3.0, KW_PLUS = 8.0, KW_PLUS_BAR = 100.0;
constexpr double SCALING_MAX_GRAD = 100.0;
constexpr int FILTER_MAX = 32;
constexpr int ST_RUNNING = 99;          // internal status while iterating
constexpr int ST_SWEEP_FAILED = -70;    // internal, launches that write the caller's rows themselves (Params::emit): the Riccati sweep of the pipeline gave the
                                        // instance up (no admissible inertia correction) and its row is not out yet -- the next stage item of its block
                                        // writes it with status -7 (the sweep's lane holds one instance, not its stages)
constexpr double BIG = 1e300;
constexpr double ROLLOUT_FACTOR = 10.0;   // start-point safeguard, see prestart_instance()
// constraint violations (1-norm) below this are round-off, two orders under the 1e-8 feasibility tolerance: the
// theta comparisons of the filter line search clamp at this floor (noise ~1e-12 would otherwise reject the last
// Newton steps, which only reduce the dual infeasibility)
constexpr double THETA_FLOOR = 1e-10;
constexpr double EPS10 = 10.0 * 2.220446049250313e-16;
// Circle rows that are active late in the iteration put weights z / s of 1e10 ... 1e13 into the condensed Hessian; the wave-per-instance
// MFMA sweep reads its cost-to-go transposed where a product wants it so, and a matrix that is symmetric only up to 1e-16 x 1e12 then
// costs the collision-avoidance family iterations (mean 25.6 against 24.5, and most of its instances that wander to the iteration limit:
// profiles/r04_ca_lottery.txt).  Instances with such a row are symmetrised every stage, like the ones that ever needed an inertia correction.
constexpr double ILL_WEIGHT = 1e4;
// A bound on a state the reference's NLP leaves free -- x, y, the heading, the progress state: bits 2, 3, 6, 7 of (u, x) -- does the same once it
// is active (a box on the terminal y, N = 30 / 50: k_solve_wg alone needed an iteration more than every other path and the oracle on 4 - 14 % of
// the rows and ended up to 5e-6 from them; tests/test_gpu_bound_structures.py).  The bounds of the steering angle and the speed do not: their
// states sit one stage behind an input.
constexpr uint32_t ILL_STATE_VM = 0xCCu;

#if defined(__HIP_DEVICE_COMPILE__)
typedef __attribute__((address_space(3))) const double* mpc_lds_cptr;
typedef __attribute__((address_space(3))) double* mpc_lds_ptr;
#else
typedef const double* mpc_lds_cptr;
typedef double* mpc_lds_ptr;
#endif

// ---- per-instance scalar rows ----------------------------------------------------------------------------
enum ScRow {
    SC_MU = 0, SC_TAU, SC_DF, SC_THETA, SC_FCOST, SC_LOGSUM, SC_THMAX, SC_THMIN, SC_DLAST, SC_DELTA, SC_E0,
    SC_SF, SC_NUF, SC_ZLF, SC_ZUF, SC_DFRIC, SC_GFR0, SC_GFR1, SC_GFR2, SC_HUX0, SC_HUX1,
    SC_C0,                       // 6 rows: c_0 = x_0 - r_0
    SC_ALPHA = SC_C0 + 6, SC_ADU, SC_PHI, SC_NTRIAL,
    SC_A0LB, SC_A0UB,            // per-instance bounds of a_0 (stage-0 friction row presolved into a bound)
    SC_E0S,                      // second chance inside k_solve_wg: the KKT error the first attempt stopped at (given back with its row when every level fails)
    SC_COUNT
};
enum IsRow { IS_STATUS = 0, IS_ITERS, IS_NFILT, IS_HAVETH0, IS_CONV, IS_ROLL, IS_FROW,
             IS_ILL,                      // a circle row (or a bound of a state in ILL_STATE_VM) of the instance carries a large weight z / s (set by the stage phases of k_solve_wg, sticky): its MFMA sweeps keep the cost-to-go symmetric
             IS_RLEV, IS_ITACC,           // second chance inside k_solve_wg: level index (| 0x100: a level of this pass has converged; | 0x200: the first attempt stopped with
                                          // status -7, else 0; bits 16-30: its iteration count), iterations of the attempts that count so far
             IS_COUNT };
// whose obstacle centres the circle rows of a solve are measured against: the descriptor's for the whole batch, six per instance (obst [B, 6]),
// or six per instance and stage (obst [B, N+1, 6]: an obstacle that moves over the horizon); OBST_PER_STAGE_SIZED: per instance and stage as well,
// and every circle row of a stage with a lower bound of its own (mpc_solve_batch_sized: rsum [B, N+1, 3]) -- see OBST_SIZED_ROWS
enum ObstMode : int32_t { OBST_SHARED = 0, OBST_PER_INSTANCE = 1, OBST_PER_STAGE = 2, OBST_PER_STAGE_SIZED = 3 };
MPC_HD constexpr bool obst_mode_staged(int32_t m) { return m == OBST_PER_STAGE || m == OBST_PER_STAGE_SIZED; }
struct Params {
    int32_t B, Bp, N, nx, bx;    // instances, padded instances (multiple of 64), horizon, states, instances/block
    int32_t obst_mult, max_iter, fixed_iters;
    int32_t has_fl, has_fu, has_ol, has_ou;
    int32_t per_inst_obst;       // obstacle centres of the solve: OBST_SHARED `obst` below, OBST_PER_INSTANCE / OBST_PER_STAGE the rows of OBST
    double dt, wheelbase, friction_div, ego_offset, tol;
    double Q[6], R[2], obst[6];
    double fl, fu, ol, ou;       // relaxed slack bounds of the friction / obstacle rows
    int32_t dec_s;               // nx = 6 with a costless, unbounded progress state: the Riccati sweep may skip it (see ric_matrix_step)
    unsigned long long* tile_mask;   // [tiles] bit l: instance l of the tile was iterating when the last Riccati launch started (stage workgroups with no such instance leave before touching HBM)
    int32_t* run_counter;        // device counter of this launch: += instances still iterating after it (nullptr: none)
    uint32_t inv_S;              // ceil(2^32 / (N+1)): segment -> (row, stage) split of the LDS prefetch
    uint32_t dense_mask;         // bit i / bit 8 + i: variable i of (u, x) has its lower / upper bound at every stage it exists at
    uint32_t lo_mask, hi_mask;   // bit i: variable i of (u, x) has a finite lower / upper bound at SOME stage (multiplier rows of the others never move)
    const double* x0;            // [B][n_w] row-major (ABI input)
    const double* p;             // [B][n_w] row-major (ABI input)
    const double* LB;            // [(N+1)*NZ] relaxed variable bounds, -inf = absent
    const double* UB;
    double *Z, *ZL, *ZU;         // [(N+1)*NZ][Bp]   iterate (u|x per stage) and its bound multipliers
    double *SO, *NUO, *ZLO, *ZUO;  // [(N+1)*3][Bp]  obstacle slacks, row multipliers, slack-bound multipliers
    double *LAM;                 // [(N+1)*NX][Bp]   equality multipliers (stage 0: x_0 pin, k>=1: defect k-1 -> k)
    double *REF;                 // [(N+1)*NX][Bp]   X_ref
    double *DZ;                  // [(N+1)*NZ][Bp]   Newton step from the Riccati sweep
    double *PK;                  // [(N+1)*(NS+NX)][Bp]  cost-to-go P_k (upper triangle) and p_k
    double *KK;                  // [N*(2*NX+2)][Bp]     feedback gains K_k, k_k
    double *BLK;                 // [(N+1)*NBLK][Bp]     condensed stage blocks consumed by the Riccati sweep
    double *ROLL;                // [(N+1)*NX][Bp]       dynamics rollout of the warm-start controls (start-point safeguard)
    // "mailbox" copies of the three arrays the stage phases and the KKT solve hand to each other, instance-major ([instance][stage][row],
    // behind the tile-major section of the same workspace): used by the workgroup-resident path (k_solve_wg), where one wavefront reads
    // all stages of one or two instances -- in the tile-major layout every (stage, row pair) of an instance is a different 1 KiB row, so
    // the 14 / 4 / 17 sixteen-byte pieces of a thread lie in as many cache lines; here they are 224 / 64 / 272 contiguous bytes
    double *MBLK, *MPK, *MDZ;
    double *MZ, *MZL, *MZU, *MSO, *MNUO, *MZLO, *MZUO, *MLAM, *MREF;     // the iterate, its multipliers and the reference, likewise (filled by k_solve_wg from the tile-major arrays when it takes an instance over)
    double *SC;                  // [SC_COUNT][Bp]
    double *FILT;                // [2*FILTER_MAX][Bp]
    const double* OBST;          // [6][Bp] per-instance obstacle centres (optional); OBST_PER_STAGE: [(N+1)*6][Bp], six rows per stage
    int32_t* ISC;                // [IS_COUNT][Bp]
    double* WS;                  // base of the double workspace (all arrays above live inside it)
    int32_t* IWS;                // base of the int32 workspace
    uint32_t ws_bytes, iws_bytes;
    uint32_t tile_elems, itile_elems;   // elements per 64-instance tile of the double / int32 workspace
    int32_t tile0;                      // first 64-instance tile handled by this launch (sub-batch pipelining)
    int32_t mbw_live;                   // k_pipeline: stage items of a tile with at most this many instances iterating write the mailbox arrays too (0: never)
    unsigned long long* DBG;            // optional [blocks][16] shader-clock stamps of the stage kernel (profiling aid), or null
    double* x_out;               // [B][n_w] row-major (ABI output)
    int32_t* status_out;
    int32_t* iters_out;
    double* kkt_out;
    // emit != 0: an instance's row of x_out / status / iterations / KKT error is written by its own stage threads at the moment its status becomes
    // final (emit_result) -- the loop kernels are then the last to touch the batch, no output transpose (k_egest) behind them; fail_count (optional)
    // += instances that end with status 0 / -7 (the host decides from it whether a second chance is due)
    int32_t emit;
    // k_pipeline: the stage items' reduction behind the evaluation in its transposed form (block_reduce_t; option red_transpose) -- the same bits
    // either way.  (In the four bytes between `emit` and the pointer behind it: no offset of the kernel-argument segment moves.)
    int32_t red_t;
    uint32_t* fail_count;
    // k_solve_wg as the last kernel of a solve: the workgroup that leaves last copies the head of the solve's control block (fin_ctl) into the
    // handle's pinned host block (fin_host) -- see its epilogue; null: nobody does
    uint32_t *fin_ctl, *fin_host;
};

// Layout of a tile of 64 instances: rows come in PAIRS, interleaved per instance -- rows 2j and 2j+1 of an array are
// the two halves of one 16-byte element per lane, [row pair][instance][2].  A thread that touches rows e and e+1
// (e even) of its instance does so with ONE 16-byte access (the compiler merges the two 8-byte buffer operations, their
// immediates differ by 8), the bx = 8 instance columns of a stage workgroup are a full 128-byte line per (row pair,
// stage), and the Riccati wave writes 1 KiB per store instruction.  Every array starts on a pair boundary and every
// per-stage row count is padded to an even number (MPC_EV), so that the parity of a row is the parity of its
// within-stage index, a compile-time literal at every hot call site.
#define MPC_EV(R) ((((uint32_t)(R)) + 1u) & ~1u)
MPC_HD constexpr uint32_t mpc_prow(uint32_t r) { return (r & ~1u) * 64u + (r & 1u); }      // element offset of row r (instance 0) inside its array
// element index of (row, instance b) relative to the first row of an array, tile-major layout
MPC_HD uint32_t ws_index(const Params& P, const double*, uint32_t row, uint32_t b) { return (b >> 6) * P.tile_elems + mpc_prow(row) + (b & 63u) * 2u; }
MPC_HD uint32_t ws_index(const Params& P, const int32_t*, uint32_t row, uint32_t b) { return (b >> 6) * P.itile_elems + mpc_prow(row) + (b & 63u) * 2u; }

#if defined(__HIP_DEVICE_COMPILE__)
typedef unsigned int mpc_v2u __attribute__((ext_vector_type(2)));
// buffer descriptor over a workspace; base pointer and scalar offsets pass through readfirstlane so that the compiler
// can PROVE they are wave-uniform (otherwise each buffer op is wrapped in a waterfall loop)
__host__ __device__ __forceinline__ __amdgpu_buffer_rsrc_t mpc_rsrc(const void* base, uint32_t bytes) {
    const uint64_t a = (uint64_t)(uintptr_t)base;
    uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a);
    uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(a >> 32));
    bytes = (uint32_t)__builtin_amdgcn_readfirstlane((int)bytes);
    asm("" : "+s"(lo), "+s"(hi), "+s"(bytes));       // pin to SGPRs right at the use (a phi through divergent control flow would move the descriptor to VGPRs)
    return __builtin_amdgcn_make_buffer_rsrc((void*)(uintptr_t)(((uint64_t)hi << 32) | lo), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ int mpc_uni(uint32_t v) { return __builtin_amdgcn_readfirstlane((int)v); }
// What device code sees as "the parameters": the kernel's by-value Params plus the two buffer descriptors, built ONCE at the top of the
// kernel.  (Before, every access site rebuilt its descriptor from the base pointer and the size -- values the register allocator had
// spilled with the rest of their kernel-argument tuple: k_solve_wg reloaded those eight words at 46 places, four v_readlane + three
// s_mov + one s_and per site.)
// `xcu`: the kernel reads workspace rows that ANOTHER compute unit wrote earlier IN THE SAME LAUNCH (k_pipeline: tiles travel between Riccati and
// stage workers of one XCD).  A CU's vector L1 is never refreshed by another CU's stores and `buffer_inv sc0` / workgroup-scope fences do not
// drop its lines (measured: profiles/r05_store_pairing.txt, tools/ubench/stale_l1.hip), so every workspace load of such a kernel carries the
// sc1 bit: served by the XCD's L2, where the producer's plain stores are once `s_waitcnt vmcnt(0)` has returned.  A literal of the kernel
// (`const PRef P(Pk, true)`), folded into every load after inlining; tests/test_isa_hazards.py proves from the ISA that no buffer load of
// k_pipeline is without the bit.
constexpr int MPC_AUX_SC1 = 16;         // cache-policy operand of the gfx940+ buffer instructions: bit 0 sc0, bit 1 nt, bit 4 sc1
struct DevParams : Params {
    __amdgpu_buffer_rsrc_t rws, riws;
    bool xcu;
    // (host + device: host functions of a translation unit are type-checked in the device pass too, e.g. the host-side reference of tools/ubench)
    __host__ __device__ __forceinline__ explicit DevParams(const Params& q, const bool xcu_ = false)
        : Params(q), rws(mpc_rsrc(q.WS, q.ws_bytes)), riws(mpc_rsrc(q.IWS, q.iws_bytes)), xcu(xcu_) {}
};
typedef DevParams PRef;
// (the parameter block of a kernel, `xcu` a literal of the call site -- also how an out-of-line device function rebuilds its own copy)
__device__ __forceinline__ PRef mpc_pref(const Params& q, const bool xcu) { return DevParams(q, xcu); }
__device__ __forceinline__ mpc_v2u mpc_bload64(const DevParams& P, const __amdgpu_buffer_rsrc_t r, const int voff, const int soff) {
    return P.xcu ? __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, MPC_AUX_SC1) : __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0);
}
__device__ __forceinline__ unsigned mpc_bload32(const DevParams& P, const __amdgpu_buffer_rsrc_t r, const int voff, const int soff) {
    return P.xcu ? __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, MPC_AUX_SC1) : __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0);
}
struct WsRefD {          // element of the double workspace: converts to double (load) / assigns from double (store)
    const PRef& P;
    uint32_t aoff, uoff, voff;     // array offset (uniform), uniform row offset, per-lane offset; bytes
    __device__ __forceinline__ operator double() const {
        const __amdgpu_buffer_rsrc_t r = P.rws;
        const mpc_v2u v = mpc_bload64(P, r, (int)voff, mpc_uni(aoff + uoff));
        return __builtin_bit_cast(double, v);
    }
    __device__ __forceinline__ double operator=(double x) const {
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(mpc_v2u, x), P.rws, (int)voff, mpc_uni(aoff + uoff), 0);
        return x;
    }
    __device__ __forceinline__ double operator=(const WsRefD& o) const { return (*this = (double)o); }
};
struct WsRefI {          // element of the int32 workspace
    const PRef& P;
    uint32_t soff, voff;
    __device__ __forceinline__ operator int32_t() const {
        const __amdgpu_buffer_rsrc_t r = P.riws;
        return (int32_t)mpc_bload32(P, r, (int)voff, mpc_uni(soff));
    }
    __device__ __forceinline__ int32_t operator=(int32_t x) const {
        const __amdgpu_buffer_rsrc_t r = P.riws;
        __builtin_amdgcn_raw_buffer_store_b32((unsigned)x, r, (int)voff, mpc_uni(soff), 0);
        return x;
    }
};
// rows e (even) and e + 1 of one instance in ONE 16-byte access; `r` refers to row e
typedef unsigned int mpc_v4u __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void ws_load2(const WsRefD& r, double& lo, double& hi) {
    const __amdgpu_buffer_rsrc_t d = r.P.rws;
    const mpc_v4u v = r.P.xcu ? __builtin_amdgcn_raw_buffer_load_b128(d, (int)r.voff, mpc_uni(r.aoff + r.uoff), MPC_AUX_SC1)
                              : __builtin_amdgcn_raw_buffer_load_b128(d, (int)r.voff, mpc_uni(r.aoff + r.uoff), 0);
    lo = __builtin_bit_cast(double, mpc_v2u{v.x, v.y});
    hi = __builtin_bit_cast(double, mpc_v2u{v.z, v.w});
}
// NOTE the scalar offset goes into the VECTOR offset here and soffset stays the constant 0.  A buffer store of more than
// 64 bits still reads its data registers for a few cycles after issue; a VALU instruction that overwrites one of them
// right behind it corrupts the last lanes read (observed on gfx950: lanes 12-15 of every 16, timing dependent).  The
// compiler inserts the wait states for this hazard only when soffset is NOT a register (GCNHazardRecognizer follows the
// older ISA manuals, which exempt the SGPR-soffset form) -- with an SGPR soffset it scheduled `v_add_u32 v18, ...`
// directly behind `buffer_store_dwordx4 v[18:21], ...`.
__device__ __forceinline__ void ws_store2(const WsRefD& r, double lo, double hi) {
    const __amdgpu_buffer_rsrc_t d = r.P.rws;
    const mpc_v2u a = __builtin_bit_cast(mpc_v2u, lo), b = __builtin_bit_cast(mpc_v2u, hi);
    __builtin_amdgcn_raw_buffer_store_b128(mpc_v4u{a.x, a.y, b.x, b.y}, d, (int)(r.voff + (uint32_t)mpc_uni(r.aoff + r.uoff)), 0, 0);
}
#define MPC_LD2(ref, lo, hi) ws_load2((ref), (lo), (hi))
#define MPC_ST2(ref, lo, hi) ws_store2((ref), (lo), (hi))
// keeps two 8-byte stores of neighbouring rows apart (all accesses share ONE descriptor value, so the compiler merges such a pair into
// a 16-byte store with an SGPR soffset -- the form whose data-register hazard it does not guard; tools/check_store_hazard.py looks for it)
#define MPC_STORE_FENCE() asm volatile("" ::: "memory")
// uni: uniform element offset (-> scalar/immediate offset), b: instance, extra: further per-lane elements
__device__ __forceinline__ WsRefD ws_ref3(const PRef& P, const double* arr, uint32_t uni, uint32_t b, uint32_t extra) {
    return WsRefD{P, (uint32_t)(uintptr_t)arr - (uint32_t)(uintptr_t)P.WS, uni * 8u, ((b >> 6) * P.tile_elems + (b & 63u) * 2u + extra) * 8u};
}
__device__ __forceinline__ WsRefI ws_ref3(const PRef& P, const int32_t* arr, uint32_t uni, uint32_t b, uint32_t extra) {
    return WsRefI{P, (uint32_t)(uintptr_t)arr - (uint32_t)(uintptr_t)P.IWS + uni * 4u, ((b >> 6) * P.itile_elems + (b & 63u) * 2u + extra) * 4u};
}
// accessors: (array, uniform element offset -> SGPR soffset / immediate, per-lane element offset -> VGPR voffset)
//   MPC_K(arr, R, dk, e)  stage kernel: row (k + dk) * R + e of thread c (k per lane, e and dk uniform)
//   MPC_S(arr, row)       per-instance scalar row (row uniform) of thread c
//   MPC_SD(arr, row)      same, row may differ between lanes
//   MPC_U(arr, row)       instance-per-thread kernels (a wavefront = one tile): uniform row, instance `bb` in scope
#define MPC_K(ptr, R, dk, e) ws_ref3(P, (ptr), (uint32_t)(dk) * (MPC_EV(R) * 64u) + mpc_prow((uint32_t)(e)), (uint32_t)c.b, (uint32_t)c.k * (MPC_EV(R) * 64u))
#define MPC_S(ptr, row) ws_ref3(P, (ptr), mpc_prow((uint32_t)(row)), (uint32_t)c.b, 0u)
#define MPC_SD(ptr, row) ws_ref3(P, (ptr), 0u, (uint32_t)c.b, mpc_prow((uint32_t)(row)))
#define MPC_U(ptr, row) ws_ref3(P, (ptr), mpc_prow((uint32_t)(row)), (uint32_t)bb, 0u)
#define MPC_UB(ptr, row, b_) ws_ref3(P, (ptr), mpc_prow((uint32_t)(row)), (uint32_t)(b_), 0u)
//   MPC_UK(arr, R, k, e)  same kernels, row e of stage k (R rows per stage) with a loop-variant k and a literal e: ONE scalar
//                         offset per (array, stage), the literal goes into the instruction's immediate / a hoisted lane offset
#define MPC_UK(ptr, R, k_, e) ws_ref3(P, (ptr), (uint32_t)(k_) * (MPC_EV(R) * 64u), (uint32_t)bb, mpc_prow((uint32_t)(e)))
//   MPC_KM(arr, R, dk, e) mailbox array (instance-major): row e of stage k + dk of thread c
#define MPC_KM(ptr, R, dk, e) WsRefD{P, (uint32_t)(uintptr_t)(ptr) - (uint32_t)(uintptr_t)P.WS, ((uint32_t)(dk) * MPC_EV(R) + (uint32_t)(e)) * 8u, \
                                     (((uint32_t)c.b * (uint32_t)(P.N + 1) + (uint32_t)c.k) * MPC_EV(R)) * 8u}
//   MPC_KI(arr, R, dk, e) mailbox array of the iterate (MZ ... MLAM) and of the stage blocks (MBLK), stage-fastest inside the block of ONE instance:
//                         [instance][row pair][stage][2] -- the 16-byte pieces the stage threads of an instance touch with one instruction are
//                         contiguous (4 - 5 cache lines per instance and wave instruction instead of one per lane).  The address depends on the
//                         instance alone, not on who works on it: the stage workers of k_pipeline write these arrays for the tiles about to leave
//                         (Ctx::mbw), any workgroup of k_solve_wg can take the instance over.
#define MPC_KI(ptr, R, dk, e) WsRefD{P, (uint32_t)(uintptr_t)(ptr) - (uint32_t)(uintptr_t)P.WS, \
                                     ((((uint32_t)(e) >> 1) * (uint32_t)(P.N + 1) + (uint32_t)(dk)) * 2u + ((uint32_t)(e) & 1u)) * 8u, \
                                     ((uint32_t)c.b * (uint32_t)(P.N + 1) * MPC_EV(R) + (uint32_t)c.k * 2u) * 8u}
#else
typedef Params PRef;
MPC_HD PRef mpc_pref(const Params& q, bool) { return q; }
#define MPC_KI(ptr, R, dk, e) ((ptr)[(size_t)c.b * (size_t)(P.N + 1) * MPC_EV(R) + (size_t)((uint32_t)(e) >> 1) * (size_t)(P.N + 1) * 2 + \
                                     (size_t)(c.k + (dk)) * 2 + ((uint32_t)(e) & 1u)])
#define MPC_KM(ptr, R, dk, e) ((ptr)[((size_t)c.b * (size_t)(P.N + 1) + (size_t)c.k + (size_t)(dk)) * MPC_EV(R) + (size_t)(e)])
#define MPC_K(ptr, R, dk, e) ((ptr)[ws_index(P, (ptr), ((uint32_t)c.k + (uint32_t)(dk)) * MPC_EV(R) + (uint32_t)(e), (uint32_t)c.b)])
#define MPC_S(ptr, row) ((ptr)[ws_index(P, (ptr), (uint32_t)(row), (uint32_t)c.b)])
#define MPC_SD(ptr, row) MPC_S(ptr, row)
#define MPC_U(ptr, row) ((ptr)[ws_index(P, (ptr), (uint32_t)(row), (uint32_t)bb)])
#define MPC_UB(ptr, row, b_) ((ptr)[ws_index(P, (ptr), (uint32_t)(row), (uint32_t)(b_))])
#define MPC_UK(ptr, R, k_, e) ((ptr)[ws_index(P, (ptr), (uint32_t)(k_) * MPC_EV(R) + (uint32_t)(e), (uint32_t)bb)])
// (the two rows of a pair are adjacent doubles)
#define MPC_LD2(ref, lo, hi) do { const double* p2_ = &(ref); (lo) = p2_[0]; (hi) = p2_[1]; } while (0)
#define MPC_ST2(ref, lo, hi) do { double* p2_ = &(ref); p2_[0] = (lo); p2_[1] = (hi); } while (0)
#define MPC_STORE_FENCE() do { } while (0)
#endif
//   MPC_KX(ARR, R, dk, e) array ARR of the iterate: the instance-major mailbox copy MARR where the phase is instantiated with MB (the
//                         workgroup-resident path), the tile-major array otherwise
#define MPC_KX(arr_, R, dk, e) (MB ? MPC_KI(P.M##arr_, R, dk, e) : MPC_K(P.arr_, R, dk, e))
// CNT consecutive rows starting at an EVEN row: pairs with 16-byte accesses, an odd last row on its own.  `ref(e)` names
// row e of the run (use MPC_ROWS around one of the accessors above, written in terms of `e`).
#define MPC_ROWS(expr) [&](int e) -> decltype(auto) { return (expr); }
template <int CNT, class RefFn>
MPC_HD void ws_load_rows(RefFn ref, double* dst) {
#pragma unroll
    for (int i = 0; i + 1 < CNT; i += 2) MPC_LD2(ref(i), dst[i], dst[i + 1]);
    if (CNT & 1) dst[CNT - 1] = ref(CNT - 1);
}
// the same for a run that starts at any row START (ref takes the row itself): an odd first row goes on its own
template <int START, int CNT, class RefFn>
MPC_HD void ws_store_run(RefFn ref, const double* src) {
    constexpr int HEAD = START & 1;
    if (HEAD) ref(START) = src[0];
#pragma unroll
    for (int i = HEAD; i + 1 < CNT; i += 2) MPC_ST2(ref(START + i), src[i], src[i + 1]);
    if ((CNT - HEAD) & 1) ref(START + CNT - 1) = src[CNT - 1];
}
template <int CNT, class RefFn>
MPC_HD void ws_store_rows(RefFn ref, const double* src) {
#pragma unroll
    for (int i = 0; i + 1 < CNT; i += 2) MPC_ST2(ref(i), src[i], src[i + 1]);
    if (CNT & 1) ref(CNT - 1) = src[CNT - 1];
}

template <int NX>
struct Dim {
    static constexpr int NU = 2;
    static constexpr int NZ = NX + 2;
    static constexpr int NS = NX * (NX + 1) / 2;
    // Structural nonzeros of the condensed state Hessian: the diagonal (cost, bound barriers) plus (x,y), (x,psi), (y,psi)
    // from the circle rows, (delta,v) from the dynamics / friction row and (v,psi) from the dynamics; the other 10 entries
    // of the upper triangle are identically zero and are neither stored nor read nor added.
    static constexpr int NH = NX + 5;
    MPC_HD static constexpr int hrow(int i, int j) {     // i <= j: row inside the H part of a stage block, -1 = structural zero
        return i == j ? i : (i == 0 && j == 1) ? NX : (i == 0 && j == 4) ? NX + 1 : (i == 1 && j == 4) ? NX + 2
             : (i == 2 && j == 3) ? NX + 3 : (i == 3 && j == 4) ? NX + 4 : -1;
    }
    // BLK rows per stage
    // (A and the defect rows are copied on their own by the forward sweep: both start on a row-pair boundary)
    static constexpr int B_A = 0, B_RUU = 6, B_GU = 8, B_CN = 10, B_GX = 10 + NX, B_H = 10 + 2 * NX;
    static constexpr int NBLK = NH + 10 + 2 * NX;
    static constexpr int NPK = NS + NX;
    static constexpr int NKK = 2 * NX + 2;
    MPC_HD static constexpr int sidx(int i, int j) { return i * NX - i * (i - 1) / 2 + (j - i); }   // i <= j
};

// ---- reductions over the stages of one instance ---------------------------------------------------------
struct Red0 { double gmax; };
struct Red1 { double a_pr, a_du, dphi; };
struct Red2 { double theta, fcost, logsum, bad; };
struct Red3 { double dual_inf, prim_inf, cmin, cmax, sum_mult, sum_z, theta, fcost, logsum, nan; };

MPC_HD Red0 red_neutral0() { return Red0{0.0}; }
MPC_HD Red1 red_neutral1() { return Red1{1.0, 1.0, 0.0}; }
MPC_HD Red2 red_neutral2() { return Red2{0.0, 0.0, 0.0, 0.0}; }
MPC_HD Red3 red_neutral3() { return Red3{0.0, 0.0, BIG, -BIG, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}; }
MPC_HD void red_combine(Red0& a, const Red0& b) { a.gmax = fmax(a.gmax, b.gmax); }
MPC_HD void red_combine(Red1& a, const Red1& b) { a.a_pr = fmin(a.a_pr, b.a_pr); a.a_du = fmin(a.a_du, b.a_du); a.dphi += b.dphi; }
MPC_HD void red_combine(Red2& a, const Red2& b) { a.theta += b.theta; a.fcost += b.fcost; a.logsum += b.logsum; a.bad = fmax(a.bad, b.bad); }
MPC_HD void red_combine(Red3& a, const Red3& b) {
    a.dual_inf = fmax(a.dual_inf, b.dual_inf); a.prim_inf = fmax(a.prim_inf, b.prim_inf);
    a.cmin = fmin(a.cmin, b.cmin); a.cmax = fmax(a.cmax, b.cmax);
    a.sum_mult += b.sum_mult; a.sum_z += b.sum_z; a.theta += b.theta; a.fcost += b.fcost; a.logsum += b.logsum;
    a.nan = fmax(a.nan, b.nan);
}


// ---- elementary functions of the phases, in one place -------------------------------------------------------------------------------
// A stage thread spends ~2 400 of its ~8 100 instructions per iteration inside the math library's division, pow, sincos, tan, log and sqrt
// (counted in round 4 by stubbing each out, profiles/r04_instruction_diet.txt) -- at one wavefront per SIMD every instruction is an issue slot.  The device versions below
// are accurate to 1-2 ulp on the ranges the phases call them with (the host versions are libm: the emulation harness and the oracle
// agree with the kernels to round-off, never bit for bit -- as before, the device library is not libm either).
// 1 / x for a positive, normal x (gaps to bounds, circle distances, cos of the steering angle): hardware estimate + two Newton steps
// (5 instructions; the IEEE division sequence is 11)
MPC_HD double mpc_rcp(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    double y = __builtin_amdgcn_rcp(x);
    y = fma(y, fma(-x, y, 1.0), y);
    y = fma(y, fma(-x, y, 1.0), y);
    return y;
#else
    return 1.0 / x;
#endif
}
// sin and cos of a heading / steering angle: Cody-Waite reduction by pi/2 in three parts (exact products by fma: good to 1 ulp for
// |x| < ~1e5), then the two minimax kernels on [-pi/4, pi/4] (coefficients of fdlibm's __kernel_sin / __kernel_cos); ~35 instructions
// against ~200 of the library's sincos, which carries the Payne-Hanek reduction for huge arguments (no fallback to it: its code next to
// this one costs 40 registers; the reduction stays exact in its products for any finite x, the quadrant is meaningless beyond 2^31 pi/2 --
// a heading of that size is a diverged iterate, and the values stay finite).
MPC_HD void mpc_sincos(double x, double& s, double& c) {
#if defined(__HIP_DEVICE_COMPILE__)
    const double fn = rint(x * 6.36619772367581382433e-01);
    double r = fma(-fn, 1.57079632679489655800e+00, x);           // pi/2 = hi + mid + lo
    r = fma(-fn, 6.12323399573676603587e-17, r);
    r = fma(-fn, -1.49738490485916983294e-33, r);
    const double z = r * r;
    const double ps = fma(z, fma(z, fma(z, fma(z, fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08), 2.75573137070700676789e-06),
                                           -1.98412698298579493134e-04), 8.33333333332248946124e-03), -1.66666666666666324348e-01);
    const double sn = fma(r * z, ps, r);
    const double pc = fma(z, fma(z, fma(z, fma(z, fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09), -2.75573143513906633035e-07),
                                           2.48015872894767294178e-05), -1.38888888888741095749e-03), 4.16666666666666019037e-02);
    const double cs = fma(z * z, pc, fma(z, -0.5, 1.0));
    const int q = (int)fn;
    const double a = (q & 1) ? cs : sn, b = (q & 1) ? sn : cs;
    s = (q & 2) ? -a : a;
    c = ((q + 1) & 2) ? -b : b;
#else
    s = sin(x); c = cos(x);
#endif
}
// tan of a steering angle (|x| well inside pi/2: the variable is bounded): sin / cos from the reduction above
MPC_HD double mpc_tan(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    double sn, cs;
    mpc_sincos(x, sn, cs);
    double t = sn * mpc_rcp(cs);
    asm volatile("" : "+v"(t));       // (opaque: left visible, the product is contracted into whatever adds to it -- in one kernel and not in another)
    return t;
#else
    return tan(x);
#endif
}
MPC_HD double mpc_log(double x) { return log(x); }
MPC_HD double mpc_sqrt(double x) { return sqrt(x); }
// r = sqrt(q) and 1 / r of a positive, normal q (circle distances) in one coupled iteration: hardware rsq estimate, two Goldschmidt steps
// on (g, h) -> (sqrt q, 1 / (2 sqrt q)) and one correction of g -- 12 instructions against the 19 + 5 of sqrt and the reciprocal
MPC_HD void mpc_sqrt_rcp(double q, double& r, double& ir) {
#if defined(__HIP_DEVICE_COMPILE__)
    const double y = __builtin_amdgcn_rsq(q);
    double g = q * y, h = 0.5 * y;
    double e = fma(-h, g, 0.5);
    g = fma(g, e, g); h = fma(h, e, h);
    e = fma(-h, g, 0.5);
    g = fma(g, e, g); h = fma(h, e, h);
    g = fma(fma(-g, g, q), h, g);
    r = g;
    ir = h + h;
#else
    r = mpc_sqrt(q);
    ir = mpc_rcp(r);
#endif
}
// theta^s_theta / (-dphi)^s_phi of the switching condition and of alpha_min (Waechter & Biegler eq. (19), (23)): one exp of two logs on
// the device (the two pow cost ~420 instructions); 0 for theta = 0
MPC_HD double mpc_switch_ratio(double theta, double mdphi) {
#if defined(__HIP_DEVICE_COMPILE__)
    return exp(S_THETA * log(theta) - S_PHI * log(mdphi));
#else
    return pow(theta, S_THETA) / pow(mdphi, S_PHI);
#endif
}

// ---- small helpers -----------------------------------------------------------------------------------------
MPC_HD bool has_lo(double lb) { return lb > -BIG; }
MPC_HD bool has_hi(double ub) { return ub < BIG; }

MPC_HD double push_in(double v, double lo, double hi) {
    const bool hl = has_lo(lo), hu = has_hi(hi);
    if (hl && hu) {
        const double pl = fmin(KAPPA_1 * fmax(1.0, fabs(lo)), KAPPA_2 * (hi - lo));
        const double pu = fmin(KAPPA_1 * fmax(1.0, fabs(hi)), KAPPA_2 * (hi - lo));
        v = fmax(v, lo + pl);
        v = fmin(v, hi - pu);
    } else if (hl) {
        v = fmax(v, lo + KAPPA_1 * fmax(1.0, fabs(lo)));
    } else if (hu) {
        v = fmin(v, hi - KAPPA_1 * fmax(1.0, fabs(hi)));
    }
    return v;
}

// push_in(v, lo, hi) == fmin(fmax(v, L), H) with these limits (an absent side: -inf / +inf) -- for the callers that clip a CHAIN of values against
// bounds known beforehand: the limits come out of the chain
MPC_HD void push_limits(double lo, double hi, double& L, double& H) {
    const bool hl = has_lo(lo), hu = has_hi(hi);
    L = -__builtin_inf();
    H = __builtin_inf();
    if (hl && hu) {
        const double pl = fmin(KAPPA_1 * fmax(1.0, fabs(lo)), KAPPA_2 * (hi - lo));
        const double pu = fmin(KAPPA_1 * fmax(1.0, fabs(hi)), KAPPA_2 * (hi - lo));
        L = lo + pl;
        H = hi - pu;
    } else if (hl) {
        L = lo + KAPPA_1 * fmax(1.0, fabs(lo));
    } else if (hu) {
        H = hi - KAPPA_1 * fmax(1.0, fabs(hi));
    }
}

// IPOPT's Compare_le (IpUtils.cpp): lhs <= rhs up to 10 machine epsilons of a reference magnitude
MPC_HD bool cmp_le(double lhs, double rhs, double base) { return lhs - rhs <= EPS10 * fabs(base); }

// fraction-to-the-boundary bookkeeping: alpha_pr = min(1, min_i -tau gap_i/dg_i), alpha_du = min(1, min_i -tau z_i/dz_i).
// The minimising side is selected by cross-multiplication and divided ONCE at the end (fp64 division costs ~13 issue
// slots and there are ~22 bound sides per thread); for the selected side the value is the same expression as before.
struct StepSel { double pg, pd, dn, dd; };
MPC_HD void sel_init(StepSel& s, double tau) { s.pg = 1.0; s.pd = -tau; s.dn = 1.0; s.dd = -tau; }
MPC_HD double sel_primal(const StepSel& s, double tau) { return -tau * s.pg / s.pd; }
MPC_HD double sel_dual(const StepSel& s, double tau) { return -tau * s.dn / s.dd; }
// multiplier step of one bound side and its fraction-to-the-boundary candidates.  gap > 0 is the distance to the
// bound, dg its change along the step, z its multiplier; ig returns 1/gap (kept by the caller for the update phase)
MPC_HD double side_step(double gap, double z, double dg, double mu, StepSel& s, double& ig) {
    ig = mpc_rcp(gap);
    const double dz = (mu - z * dg) * ig - z;               // mu/gap - z - (z/gap) dg
    if (dg < 0 && gap * s.pd > s.pg * dg) { s.pg = gap; s.pd = dg; }       // gap/(-dg) < pg/(-pd)
    if (dz < 0 && z * s.dd > s.dn * dz) { s.dn = z; s.dd = dz; }          // z/(-dz) < dn/(-dd)
    return dz;
}
// new multiplier after the dual step, clamped to [mu/(kappa gap), kappa mu/gap] (IPOPT eq. (16)); ign = 1/gap_new
MPC_HD double side_update(double ig_old, double z, double dg, double mu, double a_du, double ign) {
    const double dz = (mu - z * dg) * ig_old - z;
    const double lo = mu * ign * (1.0 / KAPPA_SIGMA), hi = KAPPA_SIGMA * mu * ign;
    return fmin(fmax(z + a_du * dz, lo), hi);
}
// KKT bookkeeping of one bound side at the new iterate: sigma, barrier-gradient factor, complementarity, log product
// (ig = 1/gap, handed over from the update phase when there was one)
MPC_HD void side_kkt(double gap, double ig, double z, double sign, int mult, double& sg, double& gbb, double& rz, double& cmin,
                     double& cmax, double& sz, double& gp) {
    sg += z * ig;
    gbb -= sign * ig;
    rz -= sign * z;
    const double cc = gap * z;
    cmin = fmin(cmin, cc);
    cmax = fmax(cmax, cc);
    sz += mult * z;
    double gm = gap;
    for (int q = 1; q < mult; ++q) gm *= gap;
    gp *= gm;
}
MPC_HD double powi_small(double g, int m) { double r = g; for (int q = 1; q < m; ++q) r *= g; return r; }

MPC_HD double zreset(double z, double gap, double mu) {
    const double lo = mu / (KAPPA_SIGMA * gap), hi = KAPPA_SIGMA * mu / gap;
    return fmin(fmax(z, lo), hi);
}

// LDS record of one (instance, stage) of the workgroup-resident path (k_solve_wg; sweeps in mpc_riccati_mfma.h), in doubles.  What lives
// in it changes along a round -- nothing of it goes through memory:
//   stage phases (phase_eval_finish / phase_finish)  ->  the condensed stage block: A, -c (NCN), and in the overlay area Ruu, gu, gx, H
//   backward sweep of stage k                        ->  the gain rows K0 / K1 (for the forward sweep), and OVER the overlay area -- whose
//                                                        entries the sweep has consumed one stage earlier -- the cost-to-go P_k, p_k
//   forward sweep                                    ->  the step, over entries IT has consumed: du_k on A[0..1], dx_k on NCN
//   stage phases (phase_preload)                     <-  step and cost-to-go
// ZERO / ONE / DT: the "no entry" / identity / dt operands of the sweeps' per-lane offsets; HX: Hux of stage 0 (zero elsewhere).  A sweep
// that has to be repeated (inertia correction) finds its Ruu / gu / gx / H overwritten: the records are rebuilt from the blocks' copy in
// memory (MBLK, written by the same phases) first -- the rare path.
template <int NX>
struct Rec {
    using D = Dim<NX>;
    static constexpr int A = 0, NCN = 6, ZERO = 6 + (int)MPC_EV(NX), ONE = ZERO + 1, DT = ZERO + 2;
    static constexpr int K0 = (DT + 2) & ~1, K1 = K0 + 8;        // Kt rows: [K0 (NX) | 0.. | kff0], [K1 | .. | kff1]
    static constexpr int HX = K1 + 8;                            // 2
    static constexpr int OV = HX + 2;                            // overlay area: stage-block part / cost-to-go
    static constexpr int RUU = OV, GU = OV + 2, GX = OV + 4, H = GX + NX;
    static constexpr int PK = OV;
    static constexpr int DU = A, DX = NCN;                       // the step, once the forward sweep has passed
    static constexpr int SIZE = OV + ((int)MPC_EV(4 + NX + D::NH) > (int)MPC_EV(D::NPK) ? (int)MPC_EV(4 + NX + D::NH) : (int)MPC_EV(D::NPK));
    static constexpr int DUMMY = -1;                             // (marks lanes that have no gain entry to write)
    static_assert(OV % 2 == 0 && K0 % 2 == 0 && NCN % 2 == 0 && SIZE % 2 == 0 && GX % 2 == 0, "pairs of a record are 16-byte aligned");
    // slot of row i of the stage block as the phases store it (BLK rows: A | Ruu | gu | c | gx | H)
    MPC_HD static constexpr int slot(int i) {
        return i < D::B_RUU ? A + i : i < D::B_GU ? RUU + (i - D::B_RUU) : i < D::B_CN ? GU + (i - D::B_GU) : i < D::B_GX ? NCN + (i - D::B_CN)
             : i < D::B_H ? GX + (i - D::B_GX) : H + (i - D::B_H);
    }
};

template <int CNT> MPC_HD void rec_load(mpc_lds_cptr r, double* dst) {
#pragma unroll
    for (int i = 0; i < CNT; ++i) dst[i] = r[i];
}
template <int CNT> MPC_HD void rec_store(mpc_lds_ptr r, const double* src) {
#pragma unroll
    for (int i = 0; i < CNT; ++i) r[i] = src[i];
}

// k_solve_wg keeps a copy of what its stage phases read of an instance EVERY round -- ten scalar rows, six integer rows, the filter -- in LDS
// (slots of doubles; the integers are exact): the workspace rows are still written (whoever looks at the instance after the launch reads them),
// but no round waits for them to come back from the L2 (2.6 k of a 56 k-tick round, and the filter entries inside the line search)
struct WgScl {
    static constexpr int MU = 0, TAU = 1, DF = 2, THETA = 3, FCOST = 4, LOGSUM = 5, THMAX = 6, THMIN = 7, A0LB = 8, A0UB = 9;
    static constexpr int STATUS = 10, NFILT = 11, ITERS = 12, CONV = 13, FROW = 14, HAVETH0 = 15, FILT = 16, SIZE = 16 + 2 * FILTER_MAX;
};
// (a scalar row written by a phase instantiated with MB goes to both)
#define MPC_SCW(arr, row, slot, val) do { MPC_S(P.arr, row) = (val); if (MB) c.scl[WgScl::slot] = (double)(val); } while (0)

// per-thread context kept in registers across the phases of the stage kernel
template <int NX>
struct PreTmp { double pk[Dim<NX>::NPK], lam[NX]; };      // loaded by phase_preload, consumed by phase_premath

template <int NX>
struct Ctx {
    static constexpr int NZ = NX + 2;
    int b, k;
    int mb, bl;      // (k_solve_wg: first instance slot of the workgroup's block, this thread's slot in it)
    bool mbw = false;    // (k_pipeline: the stage phases write iterate and stage block to the mailbox arrays as well -- the tile is about to leave)
    bool valid;      // b < B and k <= N
    bool active;     // valid and instance still iterating
    // --- iterate pieces live across the line search
    double z[NZ], dz[NZ];
    double xn[NX], dxn[NX];          // x_{k+1} and its step (k < N)
    double lam[NX], lamn[NX];        // equality multipliers of stage k and k+1 at the new iterate (exchanged through LDS)
    double zl[NZ], zu[NZ];           // bound multipliers of (u_k, x_k), register resident across the phases (0 = no bound)
    double nuo[3], zlo[3], zuo[3];   // obstacle-row multipliers and their slack-bound multipliers
    double nuf, zlf, zuf;            // friction row (k == 0, only when the row is kept)
    double igl[NZ], igu[NZ], iglo[3], iguo[3];   // 1/gap of every bound side: at the current iterate (phase 1 -> 3), then at the new one (3 -> 4)
    double dlam[NX];                 // step of the equality multipliers, -(P_k dx_k + p_k) - lambda_k
    double r0[NX];                   // r_0 (k == 0)
    double dfric0, gfr0[3];          // friction row value / gradient at the current iterate (k == 0, row kept)
    double pw_theta;                 // theta^s_theta / (-dphi)^s_phi of the switching condition (cached per line search)
    double rn[NX];                   // r_{k+1} (k < N)
    double so[3], dso[3];
    double sf, dsf;                  // friction slack (k == 0)
    double zt[NZ], sot[3], sft;      // current / accepted trial point
    double obst[6];
    // --- per-instance scalars (every thread of the instance holds the same values)
    double mu, tau, df, theta, phi, thmax, thmin;
    double a_pr, a_du, dphi, alpha, a_min;
    int nfilt, ntrial, iters, status;
    bool searching, accepted, ftype;
    bool fric_row;   // stage-0 friction row kept as a row (false: presolved into the bounds a0lb/a0ub of a_0)
    double a0lb, a0ub;
    bool conv;       // fixed-iteration (benchmark) mode: tolerance already reached, steps are accepted as they come
    bool ill;        // a circle row, or a bound of a state in ILL_STATE_VM, of this stage has a weight z / s above ILL_WEIGHT at the new iterate (phase_ineq_assemble)
    mpc_lds_cptr bnd;                        // LDS copy of the bounds table [LB (N+1)*NZ | UB (N+1)*NZ] (device)
    int bnd_ub;
    mpc_lds_ptr rec;                         // k_solve_wg (the MB instantiations of the phases): the LDS record of this (instance, stage)
    mpc_lds_ptr scl;                         // ... and the LDS copy of the instance's scalars and filter (WgScl)
    // --- pieces of the condensed gradient held across the KKT-error reduction (gx = gx_a + mu * gx_b)
    double gxa[NX], gxb[NX], gua[2], gub[2];
};

// The caller's row of an instance (optimizer.py:550 order: [u_0 .. u_{N-1} | x_0 .. x_N]), written by the instance's own stage threads -- every
// one its two inputs and NX states -- when the status becomes final; the stage-0 thread adds status, iteration count and KKT error.
struct EmitDst { double* x_out; int32_t* status_out; int32_t* iters_out; double* kkt_out; uint32_t* fail_count; };
MPC_HD EmitDst emit_dst(const Params& P) { return EmitDst{P.x_out, P.status_out, P.iters_out, P.kkt_out, P.fail_count}; }
template <int NX>
MPC_HD void emit_row(const EmitDst& d, const int N, const int b, const int k, const double* z, const int status, const int iters, const double e0) {
    const uint32_t nw = (uint32_t)(2 * N + NX * (N + 1)), row = (uint32_t)b * nw;
    if (k < N) { MPC_GP(d.x_out, row + 2u * (uint32_t)k) = z[0]; MPC_GP(d.x_out, row + 2u * (uint32_t)k + 1u) = z[1]; }
#pragma unroll
    for (int i = 0; i < NX; ++i) MPC_GP(d.x_out, row + (uint32_t)(2 * N + NX * k + i)) = z[2 + i];
    if (k == 0) {
        if (d.status_out) MPC_GP(d.status_out, b) = status;
        if (d.iters_out) MPC_GP(d.iters_out, b) = iters;
        if (d.kkt_out) MPC_GP(d.kkt_out, b) = e0;
        if (d.fail_count != nullptr && (status == 0 || status == -7)) {
#if defined(__HIP_DEVICE_COMPILE__)
            __hip_atomic_fetch_add(d.fail_count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
            ++*d.fail_count;
#endif
        }
    }
}
template <int NX>
MPC_HD void emit_result(const PRef& P, const Ctx<NX>& c, const int status, const int iters, const double e0) {
    emit_row<NX>(emit_dst(P), P.N, c.b, c.k, c.z, status, iters, e0);
}

// VM: compile-time mask of the variables of (u, x) that have a bound at SOME stage (0xFF: not known -- every side is looked up in the bounds
// table at run time); variant 2 of the kernels is instantiated for the mask of the reference's bounds, where the sides of x, y, psi (and the
// progress state) vanish from the code together with their registers.  (Round 4's split of a stage thread into a model thread and an
// inequality thread -- template parameter ROLE, variant 1 of the kernels, measured 40 - 70 % slower: profiles/r04_stage_split.txt -- left the
// sources in round 6; what remains of it is that phase 4 is written in three pieces, below.)
// Upper bits of VM: more of the reference's structure compiled in (the host checks the handle before it picks such an instantiation)
//   VM_OSPEC  circle-distance rows with a lower bound only, multiplicity 3, one obstacle for the whole batch (optimizer.py:395-403, 426-428)
//   bits 16-23 / 24-31: variables whose LOWER / UPPER bound is there at every stage the variable exists at (optimizer.py:421-491): no
//             presence test of that side (the acceleration has an upper bound only -- and a per-instance lower one at stage 0, from the
//             presolved friction row: its lower side keeps the run-time test)
constexpr uint32_t VM_OSPEC = 0x100u;
//   VM_SIZED  a lower bound per circle row (OBST_PER_STAGE_SIZED): the stage's obstacle rows carry, behind the six centres, the three offsets
//             od = (the row's own relaxed bound) - P.ol and a scale (OBST_SIZED_ROWS); wherever a phase takes a circle row's VALUE it takes
//             dist - od, so that slack, barrier, fraction-to-boundary and KKT error see the row's own bound through the shared P.ol.  Derivatives
//             are the distance's.  od = 0.0 changes no bit: with every bound the handle's, the instantiation computes what its per-stage sibling does.
constexpr uint32_t VM_SIZED = 0x200u;
// The three offsets of a stage thread live in a context of their own type, CtxSized, which the VM_SIZED instantiations of the kernels declare in
// place of Ctx (CtxOf) and whose phases see through their Ctx reference: Ctx itself, and with it every other kernel's code, is what it was (a member
// added to Ctx, used or not, changed the machine code of kernels that never read it: k_stage, k_pipeline<NX, 0>, k_solve_wg<6, 2>).
template <int NX>
struct CtxSized : Ctx<NX> { double od[3]; };
template <int NX, bool SIZED> struct CtxPick { typedef Ctx<NX> type; };
template <int NX> struct CtxPick<NX, true> { typedef CtxSized<NX> type; };
template <int NX, uint32_t VM> using CtxOf = typename CtxPick<NX, (VM & VM_SIZED) != 0u>::type;
#define MPC_OD_REF(c_) (static_cast<CtxSized<NX>&>(c_).od)
#define MPC_OD(j) ((VM & VM_SIZED) ? static_cast<const CtxSized<NX>&>(c).od[j] : 0.0)
MPC_HD constexpr uint32_t vm_dense(uint32_t lo, uint32_t hi) { return (lo << 16) | (hi << 24); }
#define MPC_HAS_OL ((VM & VM_OSPEC) ? true : (P.has_ol != 0))
#define MPC_HAS_OU ((VM & VM_OSPEC) ? false : (P.has_ou != 0))
#define MPC_OMULT ((VM & VM_OSPEC) ? 3 : P.obst_mult)
#define MPC_HAS_LO(lb_) (((VM >> (16 + i)) & 1u) ? true : has_lo(lb_))
#define MPC_HAS_HI(ub_) (((VM >> (24 + i)) & 1u) ? true : has_hi(ub_))
template <uint32_t VM>
MPC_HD constexpr bool side_mine(int i) { return ((VM >> i) & 1u) != 0u; }
// Rows of the hand-over: 3 i + {0, 1, 2} = (sum z/gap, barrier-gradient factor, -zl + zu) of variable i; behind them the circle rows'
// contributions to the (x, y, psi) entries of rx / gx_a / gx_b (3 each) and to the Hessian entries (xx, xy, xpsi, yy, ypsi, psipsi).
// (The carrier is a template parameter of the phases: IneqOut, registers.)
template <int NX>
struct IneqRows {
    static constexpr int NZ = NX + 2;
    static constexpr int SG = 0, GBB = 1, RZ = 2;                       // + 3 i
    static constexpr int ORX = 3 * NZ, OGXA = 3 * NZ + 3, OGXB = 3 * NZ + 6, OH = 3 * NZ + 9, COUNT = 3 * NZ + 15;
};
template <int NX>
struct IneqOut {
    double v[IneqRows<NX>::COUNT];
    MPC_HD void put(int r, double x) { v[r] = x; }
    MPC_HD double get(int r) const { return v[r]; }
    MPC_HD void sync() const {}          // (the LDS carrier of the kernels waits here for the inequality thread's puts)
};
// what the inequality rows leave for the KKT-error reduction
struct KktPart { double dual, prim, cmin, cmax, sz, smult, theta, gp; };
MPC_HD KktPart kkt_part_neutral() { return KktPart{0.0, 0.0, BIG, -BIG, 0.0, 0.0, 0.0, 1.0}; }
struct Trig { double sps, cps; };
MPC_HD Trig psi_trig(double psi) {
    Trig t;
    mpc_sincos(psi, t.sps, t.cps);
    return t;
}

// bounds of variable i of stage k; a_0 (k = 0, i = 1) carries the per-instance presolved friction bound
// (device: from the workgroup's LDS copy of the table, c.bnd = [LB | UB] -- a global load here would sit behind the
//  kernel's own stores in the shared vmcnt counter and stall until all of them are acknowledged)
#if defined(__HIP_DEVICE_COMPILE__)
#define MPC_BOUNDS(k, i, lb, ub)                                    \
    double lb = c.bnd[(k) * NZ + (i)], ub = c.bnd[c.bnd_ub + (k) * NZ + (i)];    \
    if ((k) == 0 && (i) == 1) { lb = c.a0lb; ub = c.a0ub; }
#else
#define MPC_BOUNDS(k, i, lb, ub)                                    \
    double lb = MPC_GP(P.LB, (k) * NZ + (i)), ub = MPC_GP(P.UB, (k) * NZ + (i));    \
    if ((k) == 0 && (i) == 1) { lb = c.a0lb; ub = c.a0ub; }
#endif

// ---- model pieces ----------------------------------------------------------------------------------------
// kinematic single-track ODE, configuration.py:353-368
// (TG: sin / cos of the heading are handed in)
template <int NX, bool TG = false>
MPC_HD void ode_eval(const Params& P, const double* x, const double* u, double* f, double& sps, double& cps, double& td) {
    if (!TG) {
        mpc_sincos(x[4], sps, cps);
    }
    td = mpc_tan(x[2]);
    f[0] = x[3] * cps;
    f[1] = x[3] * sps;
    f[2] = u[0];
    f[3] = u[1];
    f[4] = x[3] / P.wheelbase * td;
    if (NX == 6) f[5] = x[3];
}

// circle distance of pair (j, j) (optimizer.py:395-403; j = 0 centre, 1 front, 2 rear circle of the ego vehicle), optionally its
// Jacobian wrt (sx, sy, psi) -> J3 and the 6 distinct Hessian entries (00,01,02,11,12,22) -> H6
MPC_HD double circle_eval(const Params& P, const double* obst, int j, double sx, double sy, double sps, double cps, double* J3, double* H6, bool derivs) {
    const double rho = P.ego_offset;
    const double sg = (j == 0) ? 0.0 : (j == 1 ? 1.0 : -1.0);
    const double cx = sx + sg * rho * cps - obst[2 * j];
    const double cy = sy + sg * rho * sps - obst[2 * j + 1];
    double r, ir;
    mpc_sqrt_rcp(cx * cx + cy * cy, r, ir);         // (the same r with and without derivatives: a trial point and its re-evaluation agree bit for bit)
    if (!derivs) return r;
    const double ex = cx * ir, ey = cy * ir;
    const double tx = -sg * rho * sps, ty = sg * rho * cps;
    J3[0] = ex;
    J3[1] = ey;
    J3[2] = ex * tx + ey * ty;
    if (H6 == nullptr) return r;
    const double m00 = (1 - ex * ex) * ir, m01 = -ex * ey * ir, m11 = (1 - ey * ey) * ir;
    const double mt0 = m00 * tx + m01 * ty, mt1 = m01 * tx + m11 * ty;
    const double nxx = -sg * rho * cps, nyy = -sg * rho * sps;
    H6[0] = m00; H6[1] = m01; H6[2] = mt0;
    H6[3] = m11; H6[4] = mt1;
    H6[5] = tx * mt0 + ty * mt1 + ex * nxx + ey * nyy;
    return r;
}
// all three pairs at once
MPC_HD void obstacle_eval(const Params& P, const double* obst, double sx, double sy, double sps, double cps,
                          double dist[3], double J[9], double H[18], bool derivs) {
#pragma unroll
    for (int j = 0; j < 3; ++j) dist[j] = circle_eval(P, obst, j, sx, sy, sps, cps, J ? J + 3 * j : nullptr, H ? H + 6 * j : nullptr, derivs);
}

// friction row optimizer.py:378: sqrt((a^2 + v*(tan(delta)*v/2.578))^2) = |y|; d|y| = sign(y) dy, sign(0) = 0.
// g: derivative wrt (a, delta, v); h: (aa, dd, dv, vv) second derivatives
MPC_HD double friction_eval(const Params& P, double a, double dl, double v, double g[3], double h[4], bool derivs) {
    const double kap = P.friction_div;
    const double td = tan(dl);
    const double y = a * a + v * (td * v / kap);
    if (derivs) {
        const double cd = cos(dl), icd2 = mpc_rcp(cd * cd);
        const double sg = (y > 0.0) ? 1.0 : ((y < 0.0) ? -1.0 : 0.0);
        g[0] = sg * 2 * a;
        g[1] = sg * v * v * icd2 / kap;
        g[2] = sg * 2 * v * td / kap;
        h[0] = sg * 2.0;
        h[1] = sg * 2 * v * v * td * icd2 / kap;
        h[2] = sg * 2 * v * icd2 / kap;
        h[3] = sg * 2 * td / kap;
    }
    return fabs(y);
}

// The six centres the circle rows of stage thread c are measured against.  BATCH_WIDE (variant 2: one obstacle per batch) reads no mode at
// all.  STAGES = false compiles the per-stage mode out: the kernels whose machine code is pinned (k_start, wg_restart) have a second instantiation with it
// (k_start<NX, true>, wg_restart<NX, true>), which a per-stage solve runs, and a third for a sized solve (k_start / wg_restart<NX, true, SIZED_VM>).
// Per stage: six rows per stage in the tile-major pair layout of every other per-stage array -- three 16-byte loads, one scalar offset
// (the stage's) more than the per-instance rows.  The mode is a kernel argument: the branch is wave-uniform.
// SIZED (the VM_SIZED instantiations, which only a sized solve runs: no look at the mode): OBST_SIZED_ROWS rows per stage -- the six centres in the
// three 16-byte loads of the per-stage mode, then (od_0, od_1) and (od_2, scale): two loads more.  The scale is 1.0 but at a level of the second
// chance, which scales every row's offset by its fraction (x 1.0 changes no bit).  The three products stay in CtxSized: the line search evaluates the
// rows at every trial point, and a re-read there would put two loads behind the kernel's own stores in every trial.
constexpr int OBST_SIZED_ROWS = 10, OBST_SIZED_OD = 6, OBST_SIZED_SCALE = 9;
template <int NX, bool BATCH_WIDE = false, bool STAGES = true, bool SIZED = false>
MPC_HD void load_obst(const PRef& P, Ctx<NX>& c) {
    if constexpr (SIZED) {
        double r[OBST_SIZED_ROWS];
        ws_load_rows<OBST_SIZED_ROWS>(MPC_ROWS(MPC_K(P.OBST, OBST_SIZED_ROWS, 0, e)), r);
#pragma unroll
        for (int i = 0; i < 6; ++i) c.obst[i] = r[i];
#pragma unroll
        for (int j = 0; j < 3; ++j) MPC_OD_REF(c)[j] = r[OBST_SIZED_OD + j] * r[OBST_SIZED_SCALE];
        return;
    }
    if (!BATCH_WIDE && STAGES && P.per_inst_obst == OBST_PER_STAGE) {
        ws_load_rows<6>(MPC_ROWS(MPC_K(P.OBST, 6, 0, e)), c.obst);
        return;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) c.obst[i] = (!BATCH_WIDE && P.per_inst_obst) ? (double)MPC_S(P.OBST, i) : P.obst[i];
}

// ---- the caller's per-stage obstacle rows [B, N+1, 6] (row-major) -> the tile-major obstacle section, what k_transpose_obst_stages does in
//      front of every per-stage solve.  The row of an instance is 6 (N + 1) contiguous doubles; the section wants, per row PAIR, the 64
//      instances of a tile side by side (1 KiB).  Rows 2q and 2q + 1 of an instance are neighbours on both sides, so the unit is a 16-byte
//      pair: a workgroup takes one tile and OBST_XP_KC stages, element e of its trip is pair e % pc of instance e / pc on the way in (3 kc
//      consecutive pairs per instance: whole 16-byte lanes, 384 contiguous bytes per instance) and instance e % 64 of pair e / 64 on the
//      way out (1 KiB per 64 lanes), an LDS tile in between.  The elements are independent: any order of the trip gives the same rows.
constexpr int OBST_XP_KC = 8;                    // stages per workgroup: 64 x 24 pairs = 24 KiB of LDS whatever the horizon
constexpr int OBST_XP_LD = 3 * OBST_XP_KC + 1;   // pairs per instance row of the LDS tile (odd: the lanes of the way out fall into different banks)
struct alignas(16) ObstPair { double lo, hi; };
struct ObstXpose {
    const double* obst;          // [B][S][6]
    double* OBST;                // first row of the obstacle section in tile 0 (ws_layout(.., obst_stages = true).OBST)
    int32_t B, S;                // instances, stages N + 1
    uint32_t tile_elems;
};
MPC_HD int obst_xp_stages(const ObstXpose& A, int k0) { return A.S - k0 < OBST_XP_KC ? A.S - k0 : OBST_XP_KC; }
MPC_HD int obst_xp_count(const ObstXpose& A, int k0) { return 64 * 3 * obst_xp_stages(A, k0); }
MPC_HD void obst_xp_read(const ObstXpose& A, int tile, int k0, int e, ObstPair* lds) {
    const int pc = 3 * obst_xp_stages(A, k0), l = e / pc, p = e - l * pc, b = tile * 64 + l;
    if (b >= A.B) return;
    const double* s = A.obst + ((size_t)b * A.S + k0) * 6 + 2 * p;
    // (a caller's buffer that starts on an odd double -- the second chance's sub-batch may -- is read in halves)
    lds[l * OBST_XP_LD + p] = ((uintptr_t)A.obst & 15u) == 0 ? *reinterpret_cast<const ObstPair*>(s) : ObstPair{s[0], s[1]};
}
MPC_HD void obst_xp_write(const ObstXpose& A, int tile, int k0, int e, const ObstPair* lds) {
    const int p = e >> 6, l = e & 63;
    if (tile * 64 + l >= A.B) return;
    // rows 2q, 2q + 1 with q = 3 k0 + p: mpc_prow(2q) = 128 q
    *reinterpret_cast<ObstPair*>(A.OBST + (size_t)tile * A.tile_elems + (size_t)(3 * k0 + p) * 128u + 2u * (uint32_t)l) = lds[l * OBST_XP_LD + p];
}

// ---- the sized sibling (k_transpose_obst_sized, in front of every sized solve).  The rows come packed, [B, N+1, OBST_SIZED_ROWS] row-major: a
//      stage's six centres, its three radius sums and a pad (sized_pack below, what the entry points make of obst and rsum -- one row per
//      instance for the chunks and the second chance's gather to cut and copy).  Same trip, five pairs per stage instead of three; pairs 3 and 4
//      of a stage are converted on the way in: (rsum_0, rsum_1) -> (od_0, od_1), (rsum_2, pad) -> (od_2, scale), with
//          od = relax_lo(rsum) - relax_lo(ol_raw) = (rsum - ol_raw) - relax (max(1, |rsum|) - max(1, |ol_raw|)),
//      written so that rsum == ol_raw gives 0.0 whatever the compiler contracts, and a non-finite rsum a NaN (that row ends with status -6).
constexpr int OBST_XS_KC = 4;                    // stages per workgroup: 64 x 21 pairs = 21 KiB of LDS
constexpr int OBST_XS_PP = OBST_SIZED_ROWS / 2;  // pairs per stage
constexpr int OBST_XS_LD = OBST_XS_PP * OBST_XS_KC + 1;
struct ObstXposeSized {
    const double* rows;          // [B][S][OBST_SIZED_ROWS]
    double* OBST;                // first row of the obstacle section in tile 0 (ws_layout(.., obst_sized = true).OBST)
    int32_t B, S;
    uint32_t tile_elems;
    double ol_raw, relax, scale; // the handle's circle lower bound as set, BOUND_RELAX, the level's fraction (1.0: the problem itself)
};
MPC_HD double sized_od(const ObstXposeSized& A, double rsum) { return (rsum - A.ol_raw) - A.relax * (fmax(1.0, fabs(rsum)) - fmax(1.0, fabs(A.ol_raw))); }
MPC_HD int obst_xs_stages(const ObstXposeSized& A, int k0) { return A.S - k0 < OBST_XS_KC ? A.S - k0 : OBST_XS_KC; }
MPC_HD int obst_xs_count(const ObstXposeSized& A, int k0) { return 64 * OBST_XS_PP * obst_xs_stages(A, k0); }
MPC_HD void obst_xs_read(const ObstXposeSized& A, int tile, int k0, int e, ObstPair* lds) {
    const int pc = OBST_XS_PP * obst_xs_stages(A, k0), l = e / pc, p = e - l * pc, b = tile * 64 + l;
    if (b >= A.B) return;
    const double* s = A.rows + ((size_t)b * A.S + k0) * OBST_SIZED_ROWS + 2 * p;
    ObstPair v = ((uintptr_t)A.rows & 15u) == 0 ? *reinterpret_cast<const ObstPair*>(s) : ObstPair{s[0], s[1]};
    const int q = p % OBST_XS_PP;
    if (q == 3) v = ObstPair{sized_od(A, v.lo), sized_od(A, v.hi)};
    if (q == 4) v = ObstPair{sized_od(A, v.lo), A.scale};
    lds[l * OBST_XS_LD + p] = v;
}
MPC_HD void obst_xs_write(const ObstXposeSized& A, int tile, int k0, int e, const ObstPair* lds) {
    const int p = e >> 6, l = e & 63;
    if (tile * 64 + l >= A.B) return;
    *reinterpret_cast<ObstPair*>(A.OBST + (size_t)tile * A.tile_elems + (size_t)(OBST_XS_PP * k0 + p) * 128u + 2u * (uint32_t)l) = lds[l * OBST_XS_LD + p];
}
// obst [B, S, 6] and rsum [B, S, 3] -> rows [B, S, OBST_SIZED_ROWS]; element e = b S + k
MPC_HD void sized_pack(const double* obst, const double* rsum, double* rows, size_t e) {
    double* r = rows + e * OBST_SIZED_ROWS;
    for (int i = 0; i < 6; ++i) r[i] = obst[e * 6 + i];
    for (int j = 0; j < 3; ++j) r[OBST_SIZED_OD + j] = rsum[e * 3 + j];
    r[OBST_SIZED_SCALE] = 0.0;
}

// =========================================================================================================
// Start-point safeguard (one instance per thread, before the init kernel).
// The caller's x0 is IPOPT's starting point in the reference (optimizer.py:602,607).  The reference's very first
// MPC step hands over a state guess in a transposed layout whose dynamics defects are of
// the order of 1e3; from such a point an interior-point method jams against the steering-rate bounds.  When
// the defect of the given state guess exceeds ROLLOUT_FACTOR * max(1, defect of a forward rollout of the
// (bound-projected) control guess), the state guess is replaced by that rollout.  The optimum the solver
// converges to is a KKT point of the same NLP either way.
// =========================================================================================================
// caller rows -> workspace (what the LDS-tiled k_ingest kernel does on the GPU): Z <- x0 (raw), REF <- X_ref part of p
template <int NX>
MPC_HD void ingest_instance(const PRef& P, int b) {
    constexpr int NZ = NX + 2;
    const int N = P.N;
    const uint32_t bb = (uint32_t)b;
    const size_t nw = (size_t)2 * N + (size_t)NX * (N + 1);
    const double* x0b = P.x0 + (size_t)b * nw;
    const double* pb = P.p + (size_t)b * nw;
    for (int k = 0; k <= N; ++k) {
        for (int i = 0; i < 2; ++i) MPC_UK(P.Z, NZ, k, i) = (k < N) ? x0b[2 * k + i] : 0.0;
        for (int i = 0; i < NX; ++i) {
            MPC_UK(P.Z, NZ, k, 2 + i) = x0b[2 * N + NX * k + i];
            MPC_UK(P.REF, NX, k, i) = pb[2 * N + NX * k + i];
        }
    }
}

#define X0U(k_, i_) ((double)MPC_UK(P.Z, NZ, (k_), (i_)))
#define X0X(k_, i_) ((double)MPC_UK(P.Z, NZ, (k_), 2u + (uint32_t)(i_)))
#define PRX(k_, i_) ((double)MPC_UK(P.REF, NX, (k_), (i_)))
// presolve of the stage-0 friction row |a_0^2 + c| <= fu, c = v_0^2 tan(delta_0) / kappa: x_0 is pinned to r_0
// by the equality rows, so c is a constant and the row is the simple bound a_0^2 <= fu - c (valid when the
// lower branch of the absolute value cannot bind, -fu - c <= 0).  The row has zero gradient at the usual warm
// start a_0 = 0; the bound form is exact, has the same KKT points and needs no slack.
template <int NX>
MPC_HD int prestart_a0_of(const PRef& P, const double dl0, const double v0, double& a0lb, double& a0ub) {
    a0lb = MPC_GP(P.LB, 1);
    a0ub = MPC_GP(P.UB, 1);
    int frow = 1;
    if (!P.has_fl && P.has_fu) {
        const double cf = v0 * (tan(dl0) * v0 / P.friction_div);
        const double Rhi = P.fu - cf, Rlo = -P.fu - cf;
        if (Rhi > 0.0 && Rlo <= 0.0) {
            const double amax = sqrt(Rhi);
            a0lb = fmax(a0lb, -amax);
            a0ub = fmin(a0ub, amax);
            frow = 0;
        }
    }
    return frow;
}
template <int NX>
MPC_HD int prestart_a0(const PRef& P, int b, double& a0lb, double& a0ub) {
    const uint32_t bb = (uint32_t)b;
    const double dl0 = PRX(0, 2), v0 = PRX(0, 3);
    return prestart_a0_of<NX>(P, dl0, v0, a0lb, a0ub);
}
// The two chains of the start-point safeguard are independent of each other (the GPU runs them in two wavefronts):
//   ROLLOUT = true : forward rollout of the caller's control guess from r_0, stored in ROLL; returns its clipping defect
//   ROLLOUT = false: returns the dynamics defect of the caller's state guess
// The loads of stage k+1 are issued before the arithmetic of stage k (the chain is otherwise load-latency bound).
template <int NX, bool ROLLOUT>
MPC_HD double prestart_chain(const PRef& P, int b, double a0lb, double a0ub, mpc_lds_cptr bnd) {
    // bnd: LDS copy of the bounds table [LB | UB] on the device (a global load per stage would expose its latency in
    // the dependent chain), nullptr on the host
#if defined(__HIP_DEVICE_COMPILE__)
#define PS_LB(q) bnd[(q)]
#define PS_UB(q) bnd[(P.N + 1) * NZ + (q)]
#else
#define PS_LB(q) MPC_GP(P.LB, (q))
#define PS_UB(q) MPC_GP(P.UB, (q))
    (void)bnd;
#endif
    constexpr int NZ = NX + 2;
    const int N = P.N;
    const uint32_t bb = (uint32_t)b;
    double x[NX], f[NX], u[2], un[2], gnext[NX], s, c, td;
    double th = 0.0;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
        const double r0 = PRX(0, i);
        x[i] = push_in(ROLLOUT ? r0 : X0X(0, i), PS_LB(2 + i), PS_UB(2 + i));
        th += fabs(x[i] - r0);
        if (ROLLOUT) MPC_U(P.ROLL, (uint32_t)i) = x[i];
        gnext[i] = ROLLOUT ? 0.0 : X0X(1, i);
    }
    un[0] = X0U(0, 0);
    un[1] = X0U(0, 1);
    for (int k = 0; k < N; ++k) {
        u[0] = push_in(un[0], PS_LB(k * NZ), PS_UB(k * NZ));
        u[1] = push_in(un[1], (k == 0) ? a0lb : PS_LB(k * NZ + 1), (k == 0) ? a0ub : PS_UB(k * NZ + 1));
        double graw[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) graw[i] = gnext[i];
        if (k + 1 < N) {                                   // next stage's inputs: in flight during this stage's arithmetic
            un[0] = X0U(k + 1, 0);
            un[1] = X0U(k + 1, 1);
            if (!ROLLOUT) {
#pragma unroll
                for (int i = 0; i < NX; ++i) gnext[i] = X0X(k + 2, i);
            }
        }
        ode_eval<NX>(P, x, u, f, s, c, td);
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            const double lb = PS_LB((k + 1) * NZ + 2 + i), ub = PS_UB((k + 1) * NZ + 2 + i);
            const double raw = f[i] * P.dt + x[i];
            if (ROLLOUT) {
                const double rn = push_in(raw, lb, ub);
                th += fabs(rn - raw);
                x[i] = rn;
                MPC_UK(P.ROLL, NX, k + 1, i) = rn;
            } else {
                const double gn = push_in(graw[i], lb, ub);
                th += fabs(gn - raw);
                x[i] = gn;
            }
        }
    }
    return th;
#undef PS_LB
#undef PS_UB
}
template <int NX>
MPC_HD void prestart_decide(const PRef& P, int b, int frow, double a0lb, double a0ub, double th_g, double th_r) {
    const uint32_t bb = (uint32_t)b;
    MPC_U(P.SC, (uint32_t)SC_A0LB) = a0lb;
    MPC_U(P.SC, (uint32_t)SC_A0UB) = a0ub;
    MPC_U(P.ISC, (uint32_t)IS_FROW) = frow;
    const bool use = !(th_g <= ROLLOUT_FACTOR * fmax(1.0, th_r));      // also true when th_g is NaN
    MPC_U(P.ISC, (uint32_t)IS_ROLL) = use ? 1 : 0;
}
template <int NX>
MPC_HD void prestart_instance(const PRef& P, int b) {
    // the caller's rows were transposed into the workspace by the ingest kernel: Z holds the raw x0, REF holds X_ref
    double a0lb, a0ub;
    const int frow = prestart_a0<NX>(P, b, a0lb, a0ub);
    const double th_r = prestart_chain<NX, true>(P, b, a0lb, a0ub, nullptr);
    const double th_g = prestart_chain<NX, false>(P, b, a0lb, a0ub, nullptr);
    prestart_decide<NX>(P, b, frow, a0lb, a0ub, th_g, th_r);
}
#undef X0U
#undef X0X
#undef PRX

// =========================================================================================================
// Phase 0 (init kernel only): build the start iterate from the caller's x0 (IPOPT section 3.6)
// =========================================================================================================
template <int NX, bool OSTG = true, bool SIZED = false>           // (OSTG, SIZED: load_obst's STAGES, SIZED)
MPC_HD void phase_init_point(const PRef& P, Ctx<NX>& c, Red0& red) {
    using D = Dim<NX>;
    constexpr int NZ = D::NZ;
    red = red_neutral0();
    if (!c.valid) return;
    const int N = P.N, k = c.k;
    load_obst<NX, false, OSTG, SIZED>(P, c);
    c.fric_row = MPC_S(P.ISC, IS_FROW) != 0;
    c.a0lb = MPC_S(P.SC, SC_A0LB);
    c.a0ub = MPC_S(P.SC, SC_A0UB);
    const bool roll = MPC_S(P.ISC, IS_ROLL) != 0;
    // (the guess, the rollout and the next stage's reference with paired loads, all requested before the verdict `roll` is looked at: one round
    //  trip to the L2 instead of two, a third of the load instructions)
    double zraw[MPC_EV(NZ)], rroll[MPC_EV(NX)], rnext[MPC_EV(NX)];
    ws_load_rows<NZ>(MPC_ROWS(MPC_K(P.Z, NZ, 0, e)), zraw);
    ws_load_rows<NX>(MPC_ROWS(MPC_K(P.ROLL, NX, 0, e)), rroll);
    if (k < N) ws_load_rows<NX>(MPC_ROWS(MPC_K(P.REF, NX, 1, e)), rnext);
    else {
#pragma unroll
        for (int i = 0; i < NX; ++i) rnext[i] = 0.0;
    }
    double gmax = 0.0;
#pragma unroll
    for (int i = 0; i < NZ; ++i) {
        const bool isu = i < 2;
        double raw = 0.0, lb = -INFINITY, ub = INFINITY;
        if (!(isu && k == N)) {
            raw = (!isu && roll) ? rroll[i >= 2 ? i - 2 : 0] : zraw[i];    // raw x0 (ingested)
            MPC_BOUNDS(k, i, lbt, ubt);               // (device: the workgroup's LDS table, like every other phase)
            lb = lbt;
            ub = ubt;
        }
        if (k < N) {
            // |grad f| at the user's start point (objective scaling, IPOPT section 3.8)
            const double g = isu ? 2 * P.R[i] * raw : 2 * P.Q[i - 2] * (raw - rnext[i >= 2 ? i - 2 : 0]);
            gmax = fmax(gmax, fabs(g));
        }
        const double v = push_in(raw, lb, ub);
        c.z[i] = v;
        c.zl[i] = has_lo(lb) ? 1.0 : 0.0;
        c.zu[i] = has_hi(ub) ? 1.0 : 0.0;
    }
    // (stores by row pair -- half the store instructions of the start iterate)
    {
        double zero[MPC_EV(NZ)];
#pragma unroll
        for (int i = 0; i < (int)MPC_EV(NZ); ++i) zero[i] = 0.0;
        ws_store_rows<NZ>(MPC_ROWS(MPC_K(P.Z, NZ, 0, e)), c.z);
        // (multiplier pairs of variables that have a bound nowhere are never loaded -- phase_preload's condition -- and not written here either;
        //  the step DZ is written by the first Riccati sweep, whole, before anything reads it: no zeros for it)
#pragma unroll
        for (int i = 0; i < NZ; i += 2) {
            const bool a0 = (i == 0) && (k == 0);
            const uint32_t both = (i + 1 < NZ) ? 3u : 1u;
            if (((P.lo_mask >> i) & both) || a0) { if (i + 1 < NZ) MPC_ST2(MPC_K(P.ZL, NZ, 0, i), c.zl[i], c.zl[i + 1]); else MPC_K(P.ZL, NZ, 0, i) = c.zl[i]; }
            if (((P.hi_mask >> i) & both) || a0) { if (i + 1 < NZ) MPC_ST2(MPC_K(P.ZU, NZ, 0, i), c.zu[i], c.zu[i + 1]); else MPC_K(P.ZU, NZ, 0, i) = c.zu[i]; }
        }
        ws_store_rows<NX>(MPC_ROWS(MPC_K(P.LAM, NX, 0, e)), zero);
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) {
        c.lam[i] = 0.0;
        c.rn[i] = rnext[i];
        c.r0[i] = (k == 0) ? (double)MPC_S(P.REF, i) : 0.0;
    }
    // slacks: s = d(w0) pushed inside its bounds
    double sps, cps;
    mpc_sincos(c.z[2 + 4], sps, cps);
    double dist[3];
    obstacle_eval(P, c.obst, c.z[2], c.z[3], sps, cps, dist, nullptr, nullptr, false);
    if constexpr (SIZED) {
#pragma unroll
        for (int j = 0; j < 3; ++j) dist[j] -= MPC_OD_REF(c)[j];
    }
    const double ol = P.has_ol ? P.ol : -INFINITY, ou = P.has_ou ? P.ou : INFINITY;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        c.so[j] = push_in(dist[j], ol, ou);
        c.nuo[j] = 0.0;
        c.zlo[j] = P.has_ol ? 1.0 : 0.0;
        c.zuo[j] = P.has_ou ? 1.0 : 0.0;
    }
    ws_store_rows<3>(MPC_ROWS(MPC_K(P.SO, 3, 0, e)), c.so);
    ws_store_rows<3>(MPC_ROWS(MPC_K(P.NUO, 3, 0, e)), c.nuo);
    ws_store_rows<3>(MPC_ROWS(MPC_K(P.ZLO, 3, 0, e)), c.zlo);
    ws_store_rows<3>(MPC_ROWS(MPC_K(P.ZUO, 3, 0, e)), c.zuo);
    if (k == 0) {
        const double fl = P.has_fl ? P.fl : -INFINITY, fu = P.has_fu ? P.fu : INFINITY;
        const double dfr = c.fric_row ? friction_eval(P, c.z[1], c.z[2 + 2], c.z[2 + 3], nullptr, nullptr, false) : 0.0;
        c.sf = c.fric_row ? push_in(dfr, fl, fu) : 0.0;
        MPC_S(P.SC, SC_SF) = c.sf;
        c.nuf = 0.0;
        c.zlf = (c.fric_row && P.has_fl) ? 1.0 : 0.0;
        c.zuf = (c.fric_row && P.has_fu) ? 1.0 : 0.0;
        MPC_S(P.SC, SC_NUF) = 0.0;
        MPC_S(P.SC, SC_ZLF) = c.zlf;
        MPC_S(P.SC, SC_ZUF) = c.zuf;
        MPC_S(P.SC, SC_DFRIC) = 0.0;
        MPC_S(P.SC, SC_GFR0) = 0.0;
        MPC_S(P.SC, SC_GFR1) = 0.0;
        MPC_S(P.SC, SC_GFR2) = 0.0;
        MPC_S(P.SC, SC_HUX0) = 0.0;
        MPC_S(P.SC, SC_HUX1) = 0.0;
    }
    red.gmax = gmax;
}

template <int NX>
MPC_HD void phase_init_scalars(const PRef& P, Ctx<NX>& c, const Red0& red) {
    if (!c.valid) return;
    c.df = red.gmax > SCALING_MAX_GRAD ? SCALING_MAX_GRAD / red.gmax : 1.0;
    c.mu = MU_INIT;
    c.tau = fmax(TAU_MIN, 1.0 - c.mu);
    c.nfilt = 0;
    c.iters = 0;
    c.status = ST_RUNNING;
    c.active = true;
    c.conv = false;
    c.thmax = 0.0;
    c.thmin = 0.0;
    if (c.k == 0) {
        MPC_S(P.SC, SC_DF) = c.df;
        MPC_S(P.SC, SC_DLAST) = 0.0;
        MPC_S(P.SC, SC_DELTA) = 0.0;
        MPC_S(P.SC, SC_THMAX) = 0.0;
        MPC_S(P.SC, SC_THMIN) = 0.0;
        MPC_S(P.SC, SC_ALPHA) = 0.0;
        MPC_S(P.SC, SC_ADU) = 0.0;
        MPC_S(P.SC, SC_PHI) = 0.0;
        MPC_S(P.SC, SC_NTRIAL) = 0.0;
        MPC_S(P.ISC, IS_NFILT) = 0;
        MPC_S(P.ISC, IS_HAVETH0) = 0;
        MPC_S(P.ISC, IS_CONV) = 0;
        MPC_S(P.ISC, IS_ITERS) = 0;
        MPC_S(P.ISC, IS_ILL) = 0;
    }
}

// =========================================================================================================
// Phase 1: load the Newton step, slack/dual steps, fraction-to-the-boundary candidates, d(phi)
// =========================================================================================================
template <int NX, bool MB = false>
MPC_HD void phase_load_scalars(const PRef& P, Ctx<NX>& c) {
    c.status = 0;
    c.active = false;
    c.ill = false;
    if (!c.valid) return;
    int32_t status, nfilt, iters, convf, frow, haveth0;
    double mu, tau, df, theta, fcost, logsum, thmax, thmin, a0lb, a0ub;
    if (MB) {
        mpc_lds_cptr q = c.scl;
        status = (int32_t)q[WgScl::STATUS]; nfilt = (int32_t)q[WgScl::NFILT]; iters = (int32_t)q[WgScl::ITERS];
        convf = (int32_t)q[WgScl::CONV]; frow = (int32_t)q[WgScl::FROW]; haveth0 = (int32_t)q[WgScl::HAVETH0];
        mu = q[WgScl::MU]; tau = q[WgScl::TAU]; df = q[WgScl::DF]; theta = q[WgScl::THETA]; fcost = q[WgScl::FCOST]; logsum = q[WgScl::LOGSUM];
        thmax = q[WgScl::THMAX]; thmin = q[WgScl::THMIN]; a0lb = q[WgScl::A0LB]; a0ub = q[WgScl::A0UB];
    } else {
        // every load is issued before anything is consumed: one memory round trip for all per-instance scalars
        status = MPC_S(P.ISC, IS_STATUS); nfilt = MPC_S(P.ISC, IS_NFILT); iters = MPC_S(P.ISC, IS_ITERS);
        convf = MPC_S(P.ISC, IS_CONV); frow = MPC_S(P.ISC, IS_FROW); haveth0 = MPC_S(P.ISC, IS_HAVETH0);
        mu = MPC_S(P.SC, SC_MU); tau = MPC_S(P.SC, SC_TAU); df = MPC_S(P.SC, SC_DF); theta = MPC_S(P.SC, SC_THETA);
        fcost = MPC_S(P.SC, SC_FCOST); logsum = MPC_S(P.SC, SC_LOGSUM);
        thmax = MPC_S(P.SC, SC_THMAX); thmin = MPC_S(P.SC, SC_THMIN);
        a0lb = MPC_S(P.SC, SC_A0LB); a0ub = MPC_S(P.SC, SC_A0UB);
    }
    c.status = status;
    c.active = status == ST_RUNNING;
    c.mu = mu; c.tau = tau; c.df = df; c.theta = theta;
    c.phi = df * fcost - mu * logsum;
    c.thmax = thmax; c.thmin = thmin;
    c.nfilt = nfilt; c.iters = iters;
    c.conv = P.fixed_iters > 0 && convf != 0;
    c.fric_row = frow != 0;
    c.a0lb = a0lb; c.a0ub = a0ub;
    if (!haveth0) {                        // first iteration: theta_max / theta_min from theta(w_0)
        c.thmax = 1e4 * fmax(1.0, theta);
        c.thmin = 1e-4 * fmax(1.0, theta);
    }
}

// all array loads of the stage kernel in ONE batch (no dependence on the per-instance scalars), plus the arithmetic
// that needs nothing else: slack steps ds = J dx + (d - s) and multiplier steps dlam = -(P dx + p) - lam
// MB (here, in phase_eval_assemble and phase_finish): the step, the cost-to-go and the stage blocks travel through the instance-major
// mailbox arrays instead of the tile-major ones (workgroup-resident path)
// REC (MB only): also read what the sweeps left in the LDS record (step, cost-to-go); false: memory only -- k_solve_wg issues these
// loads between its two sweeps and reads the record once the forward sweep is through (phase_preload_rec)
// KEEPC (k_solve_wg, from a workgroup's second round on its instances): what does not change from round to round -- the reference of the next
// stage, r_0, and whether any instance of the workgroup keeps its friction row at all -- is the caller's business (LDS / a register): no loads
// STEP (tile-major only): also read the rows the forward Riccati sweep writes -- the step, P.DZ; false: the EARLY batch, everything else -- a stage
// worker of k_pipeline issues it while the forward sweep of its tile is still running and reads the step behind it (phase_preload_step)
template <int NX, bool MB = false, uint32_t VM = 0xFFu, bool REC = true, bool KEEPC = false, bool STEP = true>
MPC_HD void phase_preload(const PRef& P, Ctx<NX>& c, PreTmp<NX>& tmp, const bool fric_maybe = true) {
    static_assert(STEP || !MB, "the mailbox path takes its step from the LDS record (REC)");
    using D = Dim<NX>;
    constexpr int NZ = D::NZ;
    if (!c.valid) return;
    const int N = P.N, k = c.k;
    load_obst<NX, (VM & 0x100u) != 0u, true, (VM & VM_SIZED) != 0u>(P, c);
    // (rows come in pairs, one 16-byte load per pair: see mpc_prow)
    ws_load_rows<NZ>(MPC_ROWS(MPC_KX(Z, NZ, 0, e)), c.z);
    // (MB: step and cost-to-go come from the LDS record the sweeps of this workgroup left them in -- see Rec)
    if (MB) { if (REC) { rec_load<2>(c.rec + Rec<NX>::DU, c.dz); rec_load<NX>(c.rec + Rec<NX>::DX, c.dz + 2); } }
    else if (STEP) ws_load_rows<NZ>(MPC_ROWS(MPC_K(P.DZ, NZ, 0, e)), c.dz);
#pragma unroll
    for (int i = 0; i < NZ; i += 2) {
        // multipliers of bounds that exist nowhere are never read (a_0 has per-instance bounds: stage 0 always loads its pair);
        // a row of the pair whose bound is absent holds the zero the start iterate wrote
        const bool a0 = (i == 0) && (k == 0);
        const uint32_t both = (i + 1 < NZ) ? 3u : 1u;
        c.zl[i] = 0.0;
        c.zu[i] = 0.0;
        if (i + 1 < NZ) { c.zl[i + 1] = 0.0; c.zu[i + 1] = 0.0; }
        const bool mine = side_mine<VM>(i) || (i + 1 < NZ && side_mine<VM>(i + 1));      // (compile time: whose pair of rows)
        if (mine && (((P.lo_mask >> i) & both) || a0)) {
            if (i + 1 < NZ) MPC_LD2(MPC_KX(ZL, NZ, 0, i), c.zl[i], c.zl[i + 1]); else c.zl[i] = MPC_KX(ZL, NZ, 0, i);
        }
        if (mine && (((P.hi_mask >> i) & both) || a0)) {
            if (i + 1 < NZ) MPC_LD2(MPC_KX(ZU, NZ, 0, i), c.zu[i], c.zu[i + 1]); else c.zu[i] = MPC_KX(ZU, NZ, 0, i);
        }
    }
    if (k < N) {
        if (!KEEPC) ws_load_rows<NX>(MPC_ROWS(MPC_K(P.REF, NX, 1, e)), c.rn);           // (constant: read where the start kernel put it, MB or not)
        ws_load_rows<NX>(MPC_ROWS(MPC_KX(Z, NZ, 1, 2 + e)), c.xn);
        if (MB) { if (REC) rec_load<NX>(c.rec + Rec<NX>::SIZE + Rec<NX>::DX, c.dxn); } else if (STEP) ws_load_rows<NX>(MPC_ROWS(MPC_K(P.DZ, NZ, 1, 2 + e)), c.dxn);
    } else {
#pragma unroll
        for (int i = 0; i < NX; ++i) { if (!KEEPC) c.rn[i] = 0.0; c.xn[i] = 0.0; c.dxn[i] = 0.0; }
    }
    {
        ws_load_rows<NX>(MPC_ROWS(MPC_KX(LAM, NX, 0, e)), tmp.lam);
        if (!KEEPC) {
#pragma unroll
            for (int i = 0; i < NX; ++i) c.r0[i] = (k == 0) ? (double)MPC_S(P.REF, i) : 0.0;
        }
        if (MB) { if (REC) rec_load<D::NPK>(c.rec + Rec<NX>::PK, tmp.pk); } else ws_load_rows<D::NPK>(MPC_ROWS(MPC_K(P.PK, D::NPK, 0, e)), tmp.pk);
    }
    c.so[0] = c.so[1] = c.so[2] = 0.0;
    c.nuo[0] = c.nuo[1] = c.nuo[2] = 0.0;
    c.zlo[0] = c.zlo[1] = c.zlo[2] = 0.0;
    c.zuo[0] = c.zuo[1] = c.zuo[2] = 0.0;
    {
        ws_load_rows<3>(MPC_ROWS(MPC_KX(SO, 3, 0, e)), c.so);
        ws_load_rows<3>(MPC_ROWS(MPC_KX(NUO, 3, 0, e)), c.nuo);
        if (MPC_HAS_OL) ws_load_rows<3>(MPC_ROWS(MPC_KX(ZLO, 3, 0, e)), c.zlo);
        if (MPC_HAS_OU) ws_load_rows<3>(MPC_ROWS(MPC_KX(ZUO, 3, 0, e)), c.zuo);
    }
    c.sf = c.dsf = c.nuf = c.zlf = c.zuf = c.dfric0 = 0.0;
    c.gfr0[0] = c.gfr0[1] = c.gfr0[2] = 0.0;
    if (k == 0 && fric_maybe) {                  // (fric_row is not known yet; the values are only used if it is set)
        c.sf = MPC_S(P.SC, SC_SF);
        c.nuf = MPC_S(P.SC, SC_NUF);
        c.zlf = P.has_fl ? (double)MPC_S(P.SC, SC_ZLF) : 0.0;
        c.zuf = P.has_fu ? (double)MPC_S(P.SC, SC_ZUF) : 0.0;
        c.dfric0 = MPC_S(P.SC, SC_DFRIC);
        c.gfr0[0] = MPC_S(P.SC, SC_GFR0);
        c.gfr0[1] = MPC_S(P.SC, SC_GFR1);
        c.gfr0[2] = MPC_S(P.SC, SC_GFR2);
    }
}

// the part of phase_preload<.., MB, .., REC = false> left out: step and cost-to-go from the LDS record
template <int NX>
MPC_HD void phase_preload_rec(const PRef& P, Ctx<NX>& c, PreTmp<NX>& tmp) {
    using D = Dim<NX>;
    if (!c.valid) return;
    rec_load<2>(c.rec + Rec<NX>::DU, c.dz);
    rec_load<NX>(c.rec + Rec<NX>::DX, c.dz + 2);
    if (c.k < P.N) rec_load<NX>(c.rec + Rec<NX>::SIZE + Rec<NX>::DX, c.dxn);
    rec_load<D::NPK>(c.rec + Rec<NX>::PK, tmp.pk);
}

// the part of phase_preload<.., STEP = false> left out: the step of this stage and the state step of the next one, the only rows of a stage
// item's loads that the forward sweep writes (the last stage keeps the zeros the early batch gave its dxn)
template <int NX>
MPC_HD void phase_preload_step(const PRef& P, Ctx<NX>& c) {
    using D = Dim<NX>;
    constexpr int NZ = D::NZ;
    if (!c.valid) return;
    ws_load_rows<NZ>(MPC_ROWS(MPC_K(P.DZ, NZ, 0, e)), c.dz);
    if (c.k < P.N) ws_load_rows<NX>(MPC_ROWS(MPC_K(P.DZ, NZ, 1, 2 + e)), c.dxn);
}

// arithmetic on the loaded arrays only: slack steps ds = J dx + (d - s), multiplier steps dlam = -(P dx + p) - lam
template <int NX, uint32_t VM = 0xFFu>          // (VM: VM_SIZED alone is read)
MPC_HD void phase_premath(const PRef& P, Ctx<NX>& c, const PreTmp<NX>& tmp) {
    using D = Dim<NX>;
    if (!c.valid) return;
    // slack steps need the circle distances and their Jacobians at the iterate: recomputed here (the same evaluation
    // phase 4 of the previous launch made, bit for bit) rather than stored and re-read -- the kernel is bandwidth bound
    {
        const int oi[3] = {0, 1, 4};
        const Trig tg = psi_trig(c.z[2 + 4]);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double J[3];
            const double dist = circle_eval(P, c.obst, j, c.z[2], c.z[3], tg.sps, tg.cps, J, nullptr, true) - MPC_OD(j);
            double ds = dist - c.so[j];
#pragma unroll
            for (int a = 0; a < 3; ++a) ds += J[a] * c.dz[2 + oi[a]];
            c.dso[j] = ds;
        }
    }
    {
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            double s = tmp.pk[D::NS + i];
#pragma unroll
            for (int j = 0; j < NX; ++j) s += tmp.pk[(i <= j) ? D::sidx(i, j) : D::sidx(j, i)] * c.dz[2 + j];
            c.lam[i] = tmp.lam[i];
            c.dlam[i] = -s - tmp.lam[i];
        }
        c.dsf = c.dfric0 - c.sf + c.gfr0[0] * c.dz[1] + c.gfr0[1] * c.dz[2 + 2] + c.gfr0[2] * c.dz[2 + 3];
    }
}

template <int NX, uint32_t VM = 0xFFu>
MPC_HD void phase_step_candidates(const PRef& P, Ctx<NX>& c, Red1& red) {
    using D = Dim<NX>;
    constexpr int NZ = D::NZ;
    red = red_neutral1();
    if (!c.active) return;
    const int N = P.N, k = c.k, m = MPC_OMULT;
    const double mu = c.mu, tau = c.tau;
    double dphi = 0.0;
    StepSel sel;
    sel_init(sel, tau);
#pragma unroll
    for (int i = 0; i < NZ; ++i) {
        const bool isu = i < 2;
        c.igl[i] = c.igu[i] = 0.0;
        if (isu && k == N) continue;
        const double zi = c.z[i], dv = c.dz[i];
        double gradf = 0.0;
        if (k < N) gradf = isu ? c.df * 2 * P.R[i] * zi : c.df * 2 * P.Q[i - 2] * (zi - c.rn[i - 2]);
        double gb = 0.0;
        if (side_mine<VM>(i)) {
            MPC_BOUNDS(k, i, lb, ub);
            if (MPC_HAS_LO(lb)) { side_step(zi - lb, c.zl[i], dv, mu, sel, c.igl[i]); gb -= mu * c.igl[i]; }
            if (MPC_HAS_HI(ub)) { side_step(ub - zi, c.zu[i], -dv, mu, sel, c.igu[i]); gb += mu * c.igu[i]; }
        }
        dphi += (gradf + gb) * dv;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double s = c.so[j], ds = c.dso[j];
        double gb = 0.0;
        c.iglo[j] = c.iguo[j] = 0.0;
        if (MPC_HAS_OL) { side_step(s - P.ol, c.zlo[j], ds, mu, sel, c.iglo[j]); gb -= mu * c.iglo[j]; }
        if (MPC_HAS_OU) { side_step(P.ou - s, c.zuo[j], -ds, mu, sel, c.iguo[j]); gb += mu * c.iguo[j]; }
        dphi += m * gb * ds;
    }
    if (k == 0 && c.fric_row) {
        const double s = c.sf, ds = c.dsf;
        double gb = 0.0, ig;
        if (P.has_fl) { side_step(s - P.fl, c.zlf, ds, mu, sel, ig); gb -= mu * ig; }
        if (P.has_fu) { side_step(P.fu - s, c.zuf, -ds, mu, sel, ig); gb += mu * ig; }
        dphi += gb * ds;
    } else {
        c.sf = c.dsf = c.nuf = c.zlf = c.zuf = 0.0;
    }
    red.a_pr = sel_primal(sel, tau);
    red.a_du = sel_dual(sel, tau);
    red.dphi = dphi;
}

// after the reduction: start of the filter line search (Waechter & Biegler section 2.3, eq. (23) for alpha_min)
template <int NX>
MPC_HD void phase_linesearch_begin(const PRef& P, Ctx<NX>& c, const Red1& red) {
    c.searching = false;
    c.accepted = false;
    c.ftype = false;
    c.ntrial = 0;
    if (!c.active) return;
    c.a_pr = red.a_pr;
    c.a_du = red.a_du;
    c.dphi = red.dphi;
    double a_min;
    c.pw_theta = 0.0;          // theta^s_theta / (-dphi)^s_phi
    if (c.dphi < 0 && c.theta <= c.thmin) c.pw_theta = mpc_switch_ratio(c.theta, -c.dphi);          // the only case in which the switching condition can hold
    if (c.dphi < 0 && c.theta <= c.thmin)
        a_min = fmin(fmin(GAMMA_THETA, GAMMA_PHI * c.theta / (-c.dphi)), LS_DELTA * c.pw_theta);
    else if (c.dphi < 0)
        a_min = fmin(GAMMA_THETA, GAMMA_PHI * c.theta / (-c.dphi));
    else
        a_min = GAMMA_THETA;
    c.a_min = c.conv ? 0.0 : a_min * GAMMA_ALPHA;
    c.alpha = c.a_pr;
    c.searching = c.alpha >= c.a_min;
    if (!c.searching) c.status = -7;       // no admissible step length at all
}

// =========================================================================================================
// Phase 2: evaluate constraint violation / barrier objective at the trial point w + alpha dw
// =========================================================================================================
template <int NX, uint32_t VM = 0xFFu>
MPC_HD void phase_trial_eval(const PRef& P, Ctx<NX>& c, Red2& red) {
    using D = Dim<NX>;
    constexpr int NZ = D::NZ;
    red = red_neutral2();
    if (!(c.active && c.searching)) return;
    const int N = P.N, k = c.k, m = MPC_OMULT;
    const double al = c.alpha;
    double theta = 0.0, fc = 0.0, gp = 1.0, bad = 0.0;      // gp: product of all gaps; sum of logs = log(gp), one log per thread
    double zt[NZ];                                          // the trial point (the update phase forms the accepted one again)
#pragma unroll
    for (int i = 0; i < NZ; ++i) {
        const bool isu = i < 2;
        const double v = c.z[i] + al * c.dz[i];
        zt[i] = v;
        if (isu && k == N) continue;
        if (side_mine<VM>(i)) {
            MPC_BOUNDS(k, i, lb, ub);
            if (MPC_HAS_LO(lb)) { const double gap = v - lb; if (gap <= 0) bad = 1.0; else gp *= gap; }
            if (MPC_HAS_HI(ub)) { const double gap = ub - v; if (gap <= 0) bad = 1.0; else gp *= gap; }
        }
        if (k < N) {
            if (isu) fc += P.R[i] * v * v;
            else { const double e = v - c.rn[i - 2]; fc += P.Q[i - 2] * e * e; }
        }
    }
    const Trig tg = psi_trig(zt[2 + 4]);                    // (both threads of a pair: the dynamics and the circle centres need it)
    {
        double f[NX], sps = tg.sps, cps = tg.cps, td;
        ode_eval<NX, true>(P, zt + 2, zt, f, sps, cps, td);
        if (k < N) {
#pragma unroll
            for (int i = 0; i < NX; ++i) {
                const double xnt = c.xn[i] + al * c.dxn[i];
                theta += fabs(xnt - (f[i] * P.dt + zt[2 + i]));
            }
        }
        if (k == 0) {
#pragma unroll
            for (int i = 0; i < NX; ++i) theta += fabs(zt[2 + i] - c.r0[i]);
        }
    }
    {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double dist = circle_eval(P, c.obst, j, zt[2], zt[3], tg.sps, tg.cps, nullptr, nullptr, false) - MPC_OD(j);
            const double s = c.so[j] + al * c.dso[j];
            theta += m * fabs(dist - s);
            if (MPC_HAS_OL) { const double gap = s - P.ol; if (gap <= 0) bad = 1.0; else gp *= powi_small(gap, m); }
            if (MPC_HAS_OU) { const double gap = P.ou - s; if (gap <= 0) bad = 1.0; else gp *= powi_small(gap, m); }
        }
    }
    if (k == 0 && c.fric_row) {
        const double s = c.sf + al * c.dsf;
        const double dfr = friction_eval(P, zt[1], zt[2 + 2], zt[2 + 3], nullptr, nullptr, false);
        theta += fabs(dfr - s);
        if (P.has_fl) { const double gap = s - P.fl; if (gap <= 0) bad = 1.0; else gp *= gap; }
        if (P.has_fu) { const double gap = P.fu - s; if (gap <= 0) bad = 1.0; else gp *= gap; }
    }
    red.theta = theta;
    red.fcost = fc;
    red.logsum = mpc_log(gp);
    red.bad = bad;
}

// acceptance test of the trial point against the filter, the switching and the Armijo conditions
template <int NX, bool MB = false>
MPC_HD void phase_linesearch_decide(const PRef& P, Ctx<NX>& c, const Red2& red) {
    if (!(c.active && c.searching)) return;
    ++c.ntrial;
    const double th_t = red.theta;
    const double ph_t = red.bad > 0.0 ? INFINITY : c.df * red.fcost - c.mu * red.logsum;
    bool good = isfinite(th_t) && isfinite(ph_t) && th_t <= c.thmax;
    for (int q = 0; q < c.nfilt && good; ++q) {
        const double tf = MB ? (double)c.scl[WgScl::FILT + 2 * q] : (double)MPC_SD(P.FILT, 2 * q), pf = MB ? (double)c.scl[WgScl::FILT + 2 * q + 1] : (double)MPC_SD(P.FILT, 2 * q + 1);
        if (!(cmp_le(fmax(th_t, THETA_FLOOR), fmax(tf, THETA_FLOOR), tf) || cmp_le(ph_t, pf, pf))) good = false;
    }
    if (good && c.conv) {
        c.accepted = true;
        c.ftype = true;
    } else if (good) {
        const bool sw = c.theta <= c.thmin && c.dphi < 0 && c.alpha > LS_DELTA * c.pw_theta;
        if (sw) {
            if (cmp_le(ph_t - c.phi, ETA_PHI * c.alpha * c.dphi, c.phi)) { c.accepted = true; c.ftype = true; }
        } else if (cmp_le(fmax(th_t, THETA_FLOOR), fmax((1 - GAMMA_THETA) * c.theta, THETA_FLOOR), c.theta) ||
                   cmp_le(ph_t - c.phi, -GAMMA_PHI * c.theta, c.phi)) {
            c.accepted = true;
        }
    }
    if (c.accepted) {
        c.searching = false;
    } else {
        c.alpha *= 0.5;
        if (c.alpha < c.a_min || c.ntrial >= 64) { c.searching = false; c.status = -7; }
    }
}

// =========================================================================================================
// Phase 3: accept the step -- update primal, slack, multiplier values, augment the filter
// =========================================================================================================
template <int NX, bool MB = false, uint32_t VM = 0xFFu>
MPC_HD void phase_apply_update(const PRef& P, Ctx<NX>& c) {
    using D = Dim<NX>;
    constexpr int NZ = D::NZ;
    if (!c.active) return;
    const int N = P.N, k = c.k;
    if (!c.accepted) {                      // line search failed: freeze the instance
        c.active = false;
        if (k == 0) { MPC_SCW(ISC, IS_STATUS, STATUS, c.status); MPC_S(P.SC, SC_ALPHA) = 0.0; MPC_S(P.SC, SC_NTRIAL) = c.ntrial; }
        // (the iterate the search started from; MB -- k_solve_wg -- writes the rows of an instance when it leaves the workgroup's mask)
        if (!MB && P.emit) emit_result<NX>(P, c, c.status, c.iters, k == 0 ? (double)MPC_S(P.SC, SC_E0) : 0.0);
        return;
    }
    const double mu = c.mu, al = c.alpha, ad = c.a_du;
#pragma unroll
    for (int i = 0; i < NZ; ++i) {
        if (i < 2 && k == N) continue;
        const double zi = c.z[i], dv = c.dz[i], zn = zi + al * dv;       // (the accepted trial point, formed again)
        if (side_mine<VM>(i)) {
            MPC_BOUNDS(k, i, lb, ub);
            if (MPC_HAS_LO(lb)) { const double ign = mpc_rcp(zn - lb); c.zl[i] = side_update(c.igl[i], c.zl[i], dv, mu, ad, ign); c.igl[i] = ign; }
            if (MPC_HAS_HI(ub)) { const double ign = mpc_rcp(ub - zn); c.zu[i] = side_update(c.igu[i], c.zu[i], -dv, mu, ad, ign); c.igu[i] = ign; }
        }
        (void)zi;
        c.z[i] = zn;
    }
    // stores by row pair (the u rows of the terminal stage keep their zeros; multiplier rows of absent bounds keep theirs)
    ws_store_rows<NZ>(MPC_ROWS(MPC_KX(Z, NZ, 0, e)), c.z);
    const bool mbw = !MB && c.mbw;           // (wave-uniform: a property of the tile)
    if (mbw) ws_store_rows<NZ>(MPC_ROWS(MPC_KI(P.MZ, NZ, 0, e)), c.z);
#pragma unroll
    for (int i = 0; i < NZ; i += 2) {
        const bool a0 = (i == 0) && (k == 0);
        const uint32_t both = (i + 1 < NZ) ? 3u : 1u;
        const bool mine = side_mine<VM>(i) || (i + 1 < NZ && side_mine<VM>(i + 1));
        if (mine && (((P.lo_mask >> i) & both) || a0)) {
            if (i + 1 < NZ) MPC_ST2(MPC_KX(ZL, NZ, 0, i), c.zl[i], c.zl[i + 1]); else MPC_KX(ZL, NZ, 0, i) = c.zl[i];
            if (mbw) { if (i + 1 < NZ) MPC_ST2(MPC_KI(P.MZL, NZ, 0, i), c.zl[i], c.zl[i + 1]); else MPC_KI(P.MZL, NZ, 0, i) = c.zl[i]; }
        }
        if (mine && (((P.hi_mask >> i) & both) || a0)) {
            if (i + 1 < NZ) MPC_ST2(MPC_KX(ZU, NZ, 0, i), c.zu[i], c.zu[i + 1]); else MPC_KX(ZU, NZ, 0, i) = c.zu[i];
            if (mbw) { if (i + 1 < NZ) MPC_ST2(MPC_KI(P.MZU, NZ, 0, i), c.zu[i], c.zu[i + 1]); else MPC_KI(P.MZU, NZ, 0, i) = c.zu[i]; }
        }
    }
    // equality multipliers: lambda+ = -(P_k dx_k + p_k), step computed in phase_preload
    {
#pragma unroll
        for (int i = 0; i < NX; ++i) c.lam[i] += al * c.dlam[i];
        ws_store_rows<NX>(MPC_ROWS(MPC_KX(LAM, NX, 0, e)), c.lam);
        if (mbw) ws_store_rows<NX>(MPC_ROWS(MPC_KI(P.MLAM, NX, 0, e)), c.lam);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double s = c.so[j], ds = c.dso[j], sn = s + al * ds;
        double sg = 0.0, gb = 0.0;
        if (MPC_HAS_OL) {
            const double ig = c.iglo[j], ign = mpc_rcp(sn - P.ol);
            sg += c.zlo[j] * ig; gb -= mu * ig;
            c.zlo[j] = side_update(ig, c.zlo[j], ds, mu, ad, ign);
            c.iglo[j] = ign;
        }
        if (MPC_HAS_OU) {
            const double ig = c.iguo[j], ign = mpc_rcp(P.ou - sn);
            sg += c.zuo[j] * ig; gb += mu * ig;
            c.zuo[j] = side_update(ig, c.zuo[j], -ds, mu, ad, ign);
            c.iguo[j] = ign;
        }
        (void)s;
        { c.nuo[j] += al * (gb - c.nuo[j] + sg * ds); c.so[j] = sn; }
    }
    {
        if (MPC_HAS_OL) ws_store_rows<3>(MPC_ROWS(MPC_KX(ZLO, 3, 0, e)), c.zlo);
        if (MPC_HAS_OU) ws_store_rows<3>(MPC_ROWS(MPC_KX(ZUO, 3, 0, e)), c.zuo);
        ws_store_rows<3>(MPC_ROWS(MPC_KX(NUO, 3, 0, e)), c.nuo);
        ws_store_rows<3>(MPC_ROWS(MPC_KX(SO, 3, 0, e)), c.so);
        if (mbw) {
            if (MPC_HAS_OL) ws_store_rows<3>(MPC_ROWS(MPC_KI(P.MZLO, 3, 0, e)), c.zlo);
            if (MPC_HAS_OU) ws_store_rows<3>(MPC_ROWS(MPC_KI(P.MZUO, 3, 0, e)), c.zuo);
            ws_store_rows<3>(MPC_ROWS(MPC_KI(P.MNUO, 3, 0, e)), c.nuo);
            ws_store_rows<3>(MPC_ROWS(MPC_KI(P.MSO, 3, 0, e)), c.so);
        }
    }
    if (k == 0 && c.fric_row) {
        const double s = c.sf, ds = c.dsf, sn = s + al * ds;
        double sg = 0.0, gb = 0.0;
        if (P.has_fl) {
            const double ig = mpc_rcp(s - P.fl);
            sg += c.zlf * ig; gb -= mu * ig;
            c.zlf = side_update(ig, c.zlf, ds, mu, ad, mpc_rcp(sn - P.fl));
            MPC_S(P.SC, SC_ZLF) = c.zlf;
        }
        if (P.has_fu) {
            const double ig = mpc_rcp(P.fu - s);
            sg += c.zuf * ig; gb += mu * ig;
            c.zuf = side_update(ig, c.zuf, -ds, mu, ad, mpc_rcp(P.fu - sn));
            MPC_S(P.SC, SC_ZUF) = c.zuf;
        }
        c.nuf += al * (gb - c.nuf + sg * ds);
        MPC_S(P.SC, SC_NUF) = c.nuf;
        MPC_S(P.SC, SC_SF) = sn;
        c.sf = sn;
    }
    if (k == 0) {
        // filter augmentation (h-type iteration) and bookkeeping
        if (!c.ftype) {
            int nf = c.nfilt;
            if (nf == FILTER_MAX) {
#pragma unroll 1
                for (int q = 1; q < FILTER_MAX; ++q) {          // (a cold path: unrolled, its 62 loads in flight set the register count of the kernel)
                    MPC_SD(P.FILT, 2 * (q - 1)) = MPC_SD(P.FILT, 2 * q);
                    MPC_SD(P.FILT, 2 * (q - 1) + 1) = MPC_SD(P.FILT, 2 * q + 1);
                    if (MB) { c.scl[WgScl::FILT + 2 * (q - 1)] = c.scl[WgScl::FILT + 2 * q]; c.scl[WgScl::FILT + 2 * (q - 1) + 1] = c.scl[WgScl::FILT + 2 * q + 1]; }
                }
                --nf;
            }
            MPC_SD(P.FILT, 2 * nf) = (1 - GAMMA_THETA) * c.theta;
            MPC_STORE_FENCE();       // (the two rows of an entry are one row pair: through the shared descriptor the compiler would merge the stores)
            MPC_SD(P.FILT, 2 * nf + 1) = c.phi - GAMMA_PHI * c.theta;
            if (MB) { c.scl[WgScl::FILT + 2 * nf] = (1 - GAMMA_THETA) * c.theta; c.scl[WgScl::FILT + 2 * nf + 1] = c.phi - GAMMA_PHI * c.theta; }
            MPC_SCW(ISC, IS_NFILT, NFILT, nf + 1);
        }
        MPC_SCW(ISC, IS_ITERS, ITERS, c.iters + 1);
        MPC_SCW(ISC, IS_HAVETH0, HAVETH0, 1);
        MPC_SCW(SC, SC_THMAX, THMAX, c.thmax);
        MPC_SCW(SC, SC_THMIN, THMIN, c.thmin);
        MPC_S(P.SC, SC_ALPHA) = al;
        MPC_S(P.SC, SC_ADU) = ad;
        MPC_S(P.SC, SC_PHI) = c.phi;
        MPC_S(P.SC, SC_NTRIAL) = c.ntrial;
    }
    if (!c.ftype) { if (c.nfilt == FILTER_MAX) --c.nfilt; ++c.nfilt; }
    ++c.iters;
}

// =========================================================================================================
// Phase 4: derivatives at the (new) iterate, KKT residuals, condensed Hessian blocks
//          (requires that Z and LAM of the neighbouring stage are visible: block barrier before)
// =========================================================================================================
// REUSE: the update phase ran before and left 1/gap of every bound side at the new iterate in c.ig* (no division here)
// the inequality rows' share of phase 4: sigma, barrier-gradient factor and multiplier sum of
// every variable bound; the circle rows with their geometry (distances, Jacobians, Hessians at the new iterate) and what they add to the
// stationarity residual, the condensed gradient and the condensed Hessian -> xo; complementarity extremes, multiplier sums, gap product,
// the rows' primal and dual residuals -> kp.  tg: sin / cos of the heading of this stage at the new iterate
template <int NX, bool REUSE = false, class OUT = IneqOut<NX>, uint32_t VM = 0xFFu>
MPC_HD void phase_ineq_assemble(const PRef& P, Ctx<NX>& c, OUT& xo, KktPart& kp, const Trig& tg) {
    using D = Dim<NX>;
    using IR = IneqRows<NX>;
    constexpr int NZ = D::NZ;
    kp = kkt_part_neutral();
    if (!c.active) return;
    const int N = P.N, k = c.k, m = MPC_OMULT;
#pragma unroll
    for (int i = 0; i < NZ; ++i) {
        if (!side_mine<VM>(i)) continue;            // (rows of the other thread's / of absent sides are never read either)
        const bool isu = i < 2;
        double sg = 0.0, gbb = 0.0, rz = 0.0;
        if (!(isu && k == N)) {
            MPC_BOUNDS(k, i, lb, ub);
            const double zi = c.z[i];
            if (MPC_HAS_LO(lb)) side_kkt(zi - lb, REUSE ? c.igl[i] : mpc_rcp(zi - lb), c.zl[i], 1.0, 1, sg, gbb, rz, kp.cmin, kp.cmax, kp.sz, kp.gp);
            if (MPC_HAS_HI(ub)) side_kkt(ub - zi, REUSE ? c.igu[i] : mpc_rcp(ub - zi), c.zu[i], -1.0, 1, sg, gbb, rz, kp.cmin, kp.cmax, kp.sz, kp.gp);
        }
        // (a heavy bound on x, y, the heading or the progress state -- none in the reference's NLP -- weighs on the cost-to-go as a heavy circle row does)
        // (discarded where the compiled-in mask holds none of these states: variant 2 keeps its machine code)
        if constexpr ((VM & ILL_STATE_VM) != 0u) { if (((ILL_STATE_VM >> i) & 1u) && sg > ILL_WEIGHT) c.ill = true; }
        xo.put(3 * i + IR::SG, sg); xo.put(3 * i + IR::GBB, gbb); xo.put(3 * i + IR::RZ, rz);
    }
    double orx[3] = {0.0, 0.0, 0.0}, ogxa[3] = {0.0, 0.0, 0.0}, ogxb[3] = {0.0, 0.0, 0.0}, oH[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        double J[3], Ho[6];
        const double dist = circle_eval(P, c.obst, j, c.z[2], c.z[3], tg.sps, tg.cps, J, Ho, true) - MPC_OD(j);
        const double s = c.so[j], nu = c.nuo[j];
        double sg = 0.0, gbb = 0.0, rs = -nu;
        if (MPC_HAS_OL) side_kkt(s - P.ol, REUSE ? c.iglo[j] : mpc_rcp(s - P.ol), c.zlo[j], 1.0, m, sg, gbb, rs, kp.cmin, kp.cmax, kp.sz, kp.gp);
        if (MPC_HAS_OU) side_kkt(P.ou - s, REUSE ? c.iguo[j] : mpc_rcp(P.ou - s), c.zuo[j], -1.0, m, sg, gbb, rs, kp.cmin, kp.cmax, kp.sz, kp.gp);
        if (m * sg > ILL_WEIGHT) c.ill = true;
        kp.dual = fmax(kp.dual, fabs(rs));
        const double res = dist - s;
        // (a sized row whose own bound is not finite: fmax drops a NaN from the residual norms and the row's multiplier is still zero, so nothing
        //  the termination test reads would show it before the sweeps choke on the Hessian -- status -7; into the stationarity residual, whose
        //  non-finite entries end the instance with status -6)
        if constexpr ((VM & VM_SIZED) != 0u) { if (!isfinite(res)) orx[0] = res; }
        kp.theta += m * fabs(res);
        kp.prim = fmax(kp.prim, fabs(res));
        kp.smult += m * fabs(nu);
        int q = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double ja = J[a];
            orx[a] += m * nu * ja;
            ogxa[a] += ja * (m * sg * res);
            ogxb[a] += ja * (m * gbb);
#pragma unroll
            for (int bq = a; bq < 3; ++bq, ++q) oH[q] += m * (nu * Ho[q] + sg * ja * J[bq]);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) { xo.put(IR::ORX + a, orx[a]); xo.put(IR::OGXA + a, ogxa[a]); xo.put(IR::OGXB + a, ogxb[a]); }
#pragma unroll
    for (int q = 0; q < 6; ++q) xo.put(IR::OH + q, oH[q]);
}

// The rest of phase 4 in two pieces:
//   phase_eval_model   derivatives of the dynamics and the cost at the new iterate, stationarity residual, condensed Hessian -- everything
//                      that does not need the inequality rows -> EvalTmp
//   phase_eval_finish  adds what the inequality rows contribute (xk: phase_ineq_assemble's), then the residual norms and the stage-block stores
// kp: the partial results of phase_ineq_assemble.  TG: sin / cos of the heading are handed in (tg).
template <int NX>
struct EvalTmp {
    double H[Dim<NX>::NS], rx[NX], ru[2], ruu[2], cn[NX], a[6];
    double theta, fc, prim, dual, cmin, cmax, smult, sz, gp;
    double hx0, hx1;              // Hux of stage 0 (the kept friction row's; zero otherwise)
};
template <int NX, bool REUSE = false, bool TG = false, uint32_t VM = 0xFFu>
MPC_HD void phase_eval_model(const PRef& P, Ctx<NX>& c, EvalTmp<NX>& t, const KktPart& kp, const Trig tg = Trig{0.0, 0.0}) {
    using D = Dim<NX>;
    constexpr int NZ = D::NZ, NS = D::NS;
    if (!c.active) return;
    const int N = P.N, k = c.k, m = MPC_OMULT;
    const double dt = P.dt, df = c.df;
    const double* x = c.z + 2;
    const double* u = c.z;
    double* H = t.H;
#pragma unroll
    for (int i = 0; i < NS; ++i) H[i] = 0.0;
    double lamn[NX], lam[NX], f[NX], sps = tg.sps, cps = tg.cps, td;
    double* cn = t.cn;
    // c.xn / c.lamn (stage k+1 at the new iterate) were exchanged through LDS by the kernel
#pragma unroll
    for (int i = 0; i < NX; ++i) {
        lam[i] = c.lam[i];
        lamn[i] = (k < N) ? c.lamn[i] : 0.0;
        if (k >= N) c.xn[i] = 0.0;
    }
    ode_eval<NX, TG>(P, x, u, f, sps, cps, td);
    const double secd2 = 1.0 + td * td, v = x[3], il = 1.0 / P.wheelbase;      // sec^2 = 1 + tan^2 (td from ode_eval)
    // A = I + dt * df/dx : six off-identity entries
    const double a03 = dt * cps, a04 = -dt * v * sps, a13 = dt * sps, a14 = dt * v * cps;
    const double a42 = dt * v * secd2 * il, a43 = dt * td * il;
    double theta = kp.theta, fc = 0.0, ls = 0.0, prim = kp.prim, dual = kp.dual, cmin = kp.cmin, cmax = kp.cmax, smult = kp.smult, sz = kp.sz;
    // rx: stationarity residual of x_k ; start with lambda terms
    double* rx = t.rx;
    double* ru = t.ru;
    ru[0] = ru[1] = 0.0;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
        rx[i] = lam[i];
        smult += fabs(lam[i]);
        c.gxa[i] = 0.0;
        c.gxb[i] = 0.0;
    }
    c.gua[0] = c.gua[1] = c.gub[0] = c.gub[1] = 0.0;
    double* ruu = t.ruu;
    ruu[0] = ruu[1] = 0.0;
    if (k < N) {
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            cn[i] = c.xn[i] - (f[i] * dt + x[i]);
            theta += fabs(cn[i]);
            prim = fmax(prim, fabs(cn[i]));
            rx[i] -= lamn[i];
            const double e = x[i] - c.rn[i];
            fc += P.Q[i] * e * e;
            const double g = df * 2 * P.Q[i] * e;
            c.gxa[i] = g;
            rx[i] += g;
            H[D::sidx(i, i)] = df * 2 * P.Q[i];
        }
        // - (dt Fx)' lambda_{k+1}
        rx[2] -= a42 * lamn[4];
        rx[3] -= a03 * lamn[0] + a13 * lamn[1] + a43 * lamn[4];
        rx[4] -= a04 * lamn[0] + a14 * lamn[1];
        if (NX == 6) rx[3] -= dt * lamn[5];
        // - dt * sum_r lambda_{k+1,r} Hess f_r
        H[D::sidx(2, 2)] -= dt * (lamn[4] * v * 2.0 * td * secd2 * il);
        H[D::sidx(2, 3)] -= dt * (lamn[4] * secd2 * il);
        H[D::sidx(3, 4)] -= dt * (-lamn[0] * sps + lamn[1] * cps);
        H[D::sidx(4, 4)] -= dt * (-v * (lamn[0] * cps + lamn[1] * sps));
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            fc += P.R[i] * u[i] * u[i];
            const double g = df * 2 * P.R[i] * u[i];
            c.gua[i] = g;
            ru[i] = g - dt * lamn[2 + i];
            ruu[i] = df * 2 * P.R[i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < NX; ++i) cn[i] = 0.0;
    }
    if (k == 0) {
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            const double c0 = x[i] - c.r0[i];
            MPC_S(P.SC, SC_C0 + i) = c0;
            theta += fabs(c0);
            prim = fmax(prim, fabs(c0));
        }
    }
    double gp = kp.gp;                                         // product of all gaps; sum of logs = log(gp)
    // friction row (stage 0), unless presolved into the bounds of a_0
    t.hx0 = t.hx1 = 0.0;
    if (k == 0 && c.fric_row) {
        double g[3], h[4];
        const double dfr = friction_eval(P, u[1], x[2], x[3], g, h, true);
        const double s = c.sf, nu = c.nuf;
        double sg = 0.0, gbb = 0.0, rs = -nu;
        if (P.has_fl) side_kkt(s - P.fl, mpc_rcp(s - P.fl), c.zlf, 1.0, 1, sg, gbb, rs, cmin, cmax, sz, gp);
        if (P.has_fu) side_kkt(P.fu - s, mpc_rcp(P.fu - s), c.zuf, -1.0, 1, sg, gbb, rs, cmin, cmax, sz, gp);
        dual = fmax(dual, fabs(rs));
        const double res = dfr - s;
        theta += fabs(res);
        prim = fmax(prim, fabs(res));
        smult += fabs(nu);
        ru[1] += nu * g[0];
        rx[2] += nu * g[1];
        rx[3] += nu * g[2];
        c.gua[1] += g[0] * sg * res; c.gub[1] += g[0] * gbb;
        c.gxa[2] += g[1] * sg * res; c.gxb[2] += g[1] * gbb;
        c.gxa[3] += g[2] * sg * res; c.gxb[3] += g[2] * gbb;
        ruu[1] += nu * h[0] + sg * g[0] * g[0];
        H[D::sidx(2, 2)] += nu * h[1] + sg * g[1] * g[1];
        H[D::sidx(2, 3)] += nu * h[2] + sg * g[1] * g[2];
        H[D::sidx(3, 3)] += nu * h[3] + sg * g[2] * g[2];
        t.hx0 = sg * g[0] * g[1];
        t.hx1 = sg * g[0] * g[2];
        MPC_S(P.SC, SC_HUX0) = t.hx0;
        MPC_S(P.SC, SC_HUX1) = t.hx1;
        MPC_S(P.SC, SC_DFRIC) = dfr;
        MPC_S(P.SC, SC_GFR0) = g[0];
        MPC_S(P.SC, SC_GFR1) = g[1];
        MPC_S(P.SC, SC_GFR2) = g[2];
    }
    t.a[0] = a03; t.a[1] = a04; t.a[2] = a13; t.a[3] = a14; t.a[4] = a42; t.a[5] = a43;
    t.theta = theta; t.fc = fc; t.prim = prim; t.dual = dual; t.cmin = cmin; t.cmax = cmax; t.smult = smult; t.sz = sz; t.gp = gp;
}

template <int NX, bool MB = false, class IN = IneqOut<NX>, uint32_t VM = 0xFFu>
MPC_HD void phase_eval_finish(const PRef& P, Ctx<NX>& c, Red3& red, const IN& xk, EvalTmp<NX>& t) {
    using D = Dim<NX>;
    using IR = IneqRows<NX>;
    constexpr int NZ = D::NZ;
    red = red_neutral3();
    if (!c.active) return;
    const int N = P.N, k = c.k;
    double* H = t.H;
    double* rx = t.rx;
    double* ru = t.ru;
    double* ruu = t.ruu;
    const double* cn = t.cn;
    double dual = t.dual;
    const double theta = t.theta, fc = t.fc, prim = t.prim, cmin = t.cmin, cmax = t.cmax, smult = t.smult, sz = t.sz, gp = t.gp;
#pragma unroll
    for (int i = 0; i < NZ; ++i) {
        const bool isu = i < 2;
        if (!side_mine<VM>(i)) continue;
        if (isu && k == N) continue;
        const double sg = xk.get(3 * i + IR::SG), gbb = xk.get(3 * i + IR::GBB), rz = xk.get(3 * i + IR::RZ);
        if (isu) { ruu[i] += sg; c.gub[i] += gbb; ru[i] += rz; }
        else { H[D::sidx(i - 2, i - 2)] += sg; c.gxb[i - 2] += gbb; rx[i - 2] += rz; }
    }
    {
        const int oi[3] = {0, 1, 4};
        int q = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            rx[oi[a]] += xk.get(IR::ORX + a);
            c.gxa[oi[a]] += xk.get(IR::OGXA + a);
            c.gxb[oi[a]] += xk.get(IR::OGXB + a);
#pragma unroll
            for (int bq = a; bq < 3; ++bq, ++q) H[D::sidx(oi[a], oi[bq])] += xk.get(IR::OH + q);
        }
    }
    double nanflag = 0.0;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
        dual = fmax(dual, fabs(rx[i]));
        if (!isfinite(rx[i])) nanflag = 1.0;
    }
    if (k < N) dual = fmax(dual, fmax(fabs(ru[0]), fabs(ru[1])));
    // stage blocks that do not depend on the barrier parameter
    {
        static_assert(D::B_A == 0 && D::B_RUU == 6 && D::B_CN % 2 == 0 && D::B_H % 2 == 0, "stage-block runs start on row-pair boundaries");
        const double head[8] = {t.a[0], t.a[1], t.a[2], t.a[3], t.a[4], t.a[5], ruu[0], ruu[1]};
        double hh[D::NH];
#pragma unroll
        for (int i = 0; i < NX; ++i) {
#pragma unroll
            for (int j = i; j < NX; ++j)
                if (D::hrow(i, j) >= 0) hh[D::hrow(i, j) >= 0 ? D::hrow(i, j) : 0] = H[D::sidx(i, j)];
        }
        if (MB) {
            // (the copy in memory is what a repeated sweep rebuilds the records from -- the entries its cost-to-go went over: Ruu, gu, gx, H; A and
            //  the defect are still in the record then; the sweeps themselves read the record: the defect negated)
            MPC_ST2(MPC_KI(P.MBLK, D::NBLK, 0, D::B_RUU), head[6], head[7]);
            ws_store_rows<D::NH>(MPC_ROWS(MPC_KI(P.MBLK, D::NBLK, 0, D::B_H + e)), hh);
            using RC = Rec<NX>;
            double ncn[NX];
#pragma unroll
            for (int i = 0; i < NX; ++i) ncn[i] = -cn[i];
            rec_store<6>(c.rec + RC::A, head);
            rec_store<2>(c.rec + RC::RUU, head + 6);
            rec_store<NX>(c.rec + RC::NCN, ncn);
            rec_store<D::NH>(c.rec + RC::H, hh);
            if (k == 0) { c.rec[RC::HX] = t.hx0; c.rec[RC::HX + 1] = t.hx1; }
        } else {
            ws_store_rows<8>(MPC_ROWS(MPC_K(P.BLK, D::NBLK, 0, D::B_A + e)), head);
            ws_store_rows<NX>(MPC_ROWS(MPC_K(P.BLK, D::NBLK, 0, D::B_CN + e)), cn);
            ws_store_rows<D::NH>(MPC_ROWS(MPC_K(P.BLK, D::NBLK, 0, D::B_H + e)), hh);
            if (c.mbw) {        // (the whole block: k_solve_wg builds its first records from this copy)
                ws_store_rows<8>(MPC_ROWS(MPC_KI(P.MBLK, D::NBLK, 0, D::B_A + e)), head);
                ws_store_rows<NX>(MPC_ROWS(MPC_KI(P.MBLK, D::NBLK, 0, D::B_CN + e)), cn);
                ws_store_rows<D::NH>(MPC_ROWS(MPC_KI(P.MBLK, D::NBLK, 0, D::B_H + e)), hh);
            }
        }
    }
    red.dual_inf = dual; red.prim_inf = prim; red.cmin = cmin; red.cmax = cmax;
    const double ls = mpc_log(gp);
    red.sum_mult = smult; red.sum_z = sz; red.theta = theta; red.fcost = fc; red.logsum = ls; red.nan = nanflag;
}

// (one thread per (instance, stage): the three pieces back to back, one sincos for all)
template <int NX, bool REUSE = false, bool MB = false, uint32_t VM = 0xFFu>
MPC_HD void phase_eval_assemble(const PRef& P, Ctx<NX>& c, Red3& red) {
    IneqOut<NX> xo;
    KktPart kp;
    EvalTmp<NX> t;
    const Trig tg = psi_trig(c.z[2 + 4]);
    phase_ineq_assemble<NX, REUSE, IneqOut<NX>, VM>(P, c, xo, kp, tg);
    phase_eval_model<NX, REUSE, true, VM>(P, c, t, kp, tg);
    phase_eval_finish<NX, MB, IneqOut<NX>, VM>(P, c, red, xo, t);
}

// =========================================================================================================
// Phase 5: termination test, monotone barrier update, final gradient rows of the condensed system
// =========================================================================================================
template <int NX, bool MB = false>
MPC_HD void phase_finish(const PRef& P, Ctx<NX>& c, const Red3& red, int n_mult, int n_z) {
    using D = Dim<NX>;
    if (!c.active) return;
    const int k = c.k;
    // host counts exclude the friction row and the bounds of a_0, which are per instance
    n_mult += c.fric_row ? 1 : 0;
    n_z += (has_lo(c.a0lb) ? 1 : 0) + (has_hi(c.a0ub) ? 1 : 0) + (c.fric_row ? (P.has_fl + P.has_fu) : 0);
    const int nden = n_mult + n_z;
    const double s_d = fmax(S_MAX, (red.sum_mult + red.sum_z) / (nden > 0 ? nden : 1)) / S_MAX;
    const double s_c = fmax(S_MAX, red.sum_z / (n_z > 0 ? n_z : 1)) / S_MAX;
    const double base = fmax(red.dual_inf / s_d, red.prim_inf);
    const double E0 = fmax(base, (n_z ? fmax(red.cmax, -red.cmin) : 0.0) / s_c);
    int status = ST_RUNNING;
    const int cap = P.fixed_iters > 0 ? P.fixed_iters : P.max_iter;
    if (red.nan > 0.0 || !isfinite(E0) || !isfinite(red.fcost)) status = -6;
    else if (P.fixed_iters <= 0 && E0 <= P.tol) status = 1;
    else if (c.iters >= cap) status = P.fixed_iters > 0 ? 1 : 0;
    double mu = c.mu, tau = c.tau;
    bool mu_changed = false;
    if (status == ST_RUNNING) {
        for (int guard = 0; guard < 64; ++guard) {
            const double Emu = fmax(base, (n_z ? fmax(red.cmax - mu, mu - red.cmin) : 0.0) / s_c);
            if (!(Emu <= KAPPA_EPS * mu)) break;
            const double nm = fmax(P.tol / 10.0, fmin(KAPPA_MU * mu, mu * sqrt(mu)));     // theta_mu = 1.5
            if (nm == mu) break;
            mu = nm;
            tau = fmax(TAU_MIN, 1.0 - mu);
            mu_changed = true;
        }
        double gx[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) gx[i] = c.gxa[i] + mu * c.gxb[i];
        if (MB) {
            const double gu[2] = {c.gua[0] + mu * c.gub[0], c.gua[1] + mu * c.gub[1]};
            ws_store_run<D::B_GX, NX>(MPC_ROWS(MPC_KI(P.MBLK, D::NBLK, 0, e)), gx);
            MPC_ST2(MPC_KI(P.MBLK, D::NBLK, 0, D::B_GU), gu[0], gu[1]);
            rec_store<NX>(c.rec + Rec<NX>::GX, gx);
            rec_store<2>(c.rec + Rec<NX>::GU, gu);
        } else {
            ws_store_run<D::B_GX, NX>(MPC_ROWS(MPC_K(P.BLK, D::NBLK, 0, e)), gx);
            MPC_ST2(MPC_K(P.BLK, D::NBLK, 0, D::B_GU), c.gua[0] + mu * c.gub[0], c.gua[1] + mu * c.gub[1]);
            if (c.mbw) {
                ws_store_run<D::B_GX, NX>(MPC_ROWS(MPC_KI(P.MBLK, D::NBLK, 0, e)), gx);
                MPC_ST2(MPC_KI(P.MBLK, D::NBLK, 0, D::B_GU), c.gua[0] + mu * c.gub[0], c.gua[1] + mu * c.gub[1]);
            }
        }
    }
    c.status = status;
    if (!MB && P.emit && status != ST_RUNNING) emit_result<NX>(P, c, status, c.iters, E0);
    if (k == 0) {
        MPC_SCW(SC, SC_MU, MU, mu);
        MPC_SCW(SC, SC_TAU, TAU, tau);
        MPC_SCW(SC, SC_THETA, THETA, red.theta);
        MPC_SCW(SC, SC_FCOST, FCOST, red.fcost);
        MPC_SCW(SC, SC_LOGSUM, LOGSUM, red.logsum);
        MPC_S(P.SC, SC_E0) = E0;
        MPC_SCW(ISC, IS_STATUS, STATUS, status);
        if (mu_changed) MPC_SCW(ISC, IS_NFILT, NFILT, 0);       // the filter is reset whenever mu changes
        if (P.fixed_iters > 0 && E0 <= P.tol) MPC_SCW(ISC, IS_CONV, CONV, 1);
    }
}

// =========================================================================================================
// Riccati factor/solve of the condensed KKT system: ONE instance per thread, sequential over the stages.
//   backward:  P_N = H_N,  p_N = g_N
//              Lam = Ruu + B' P+ B,  G = Hux + B' P+ A,  K = -Lam^-1 G,  kff = -Lam^-1 (gu + B'(p+ + P+ b))
//              P_k = H_k + A' P+ A + G' K,   p_k = gx + A'(p+ + P+ b) + G' kff
//   forward:   dx_0 = -c_0,  du_k = K dx_k + kff,  dx_{k+1} = A dx_k + B du_k + b_k,   b_k = -c_{k+1}
// with A = I + dt*df/dx (six off-identity entries) and B = dt*[e_delta e_v], both exploited below.
// Inertia correction: if some 2x2 block Lam is not positive definite the factorisation is repeated with
// delta_w * I added to the Hessian (IPOPT section 3.1 schedule).
// =========================================================================================================
template <int NX>
struct RicStage {
    double H[Dim<NX>::NS], ruu[2], a[6], gx[NX], gu[2], cn[NX];
};

template <int NX>
MPC_HD void ric_load(const PRef& P, int b, int k, RicStage<NX>& s) {
    using D = Dim<NX>;
    const uint32_t bb = (uint32_t)b;
#define RL(row) MPC_UK(P.BLK, D::NBLK, k, (row))
#pragma unroll
    for (int i = 0; i < NX; ++i) {
#pragma unroll
        for (int j = i; j < NX; ++j) s.H[D::sidx(i, j)] = (D::hrow(i, j) >= 0) ? (double)RL(D::B_H + (D::hrow(i, j) >= 0 ? D::hrow(i, j) : 0)) : 0.0;
    }
    s.ruu[0] = RL(D::B_RUU); s.ruu[1] = RL(D::B_RUU + 1);
#pragma unroll
    for (int i = 0; i < 6; ++i) s.a[i] = RL(D::B_A + i);
#pragma unroll
    for (int i = 0; i < NX; ++i) { s.gx[i] = RL(D::B_GX + i); s.cn[i] = RL(D::B_CN + i); }
    s.gu[0] = RL(D::B_GU); s.gu[1] = RL(D::B_GU + 1);
#undef RL
}

// M = P * A for the sparse A (columns 2,3,4 get extra terms); P symmetric, stored upper
template <int NX>
MPC_HD double sym(const double* Ps, int i, int j) { return Ps[(i <= j) ? Dim<NX>::sidx(i, j) : Dim<NX>::sidx(j, i)]; }

// One backward step of the recursion, in two halves that only meet through (P+, G, Lam^-1):
//   ric_matrix_step  P+ -> P_k, gains K            (the critical chain: the next stage needs P_k)
//   ric_vector_step  p+ -> p_k, feed-forward kff   (needs P+, G, Lam^-1 of the same stage; nothing waits for it)
// riccati_backward_step below chains them on one thread (the emulation harness, k_solve_wg's scalar fallbacks, riccati_instance).
// riccati_tile runs them on TWO wavefronts that both walk the matrix half: one stores what that half produces, the other -- a loader
// wave that idles in the backward sweep -- adds the vector half and stores the rows with an entry of it (ric_store_matrix /
// ric_store_vector below); nothing is handed over between them.  (Round 2 measured this form and dropped it: the sweep got shorter,
// the batch did not, because the stage pool was the binding bound then, and the second wave's copy of the recursion rounded
// differently.  Neither holds any more -- the pool has slack, and the contraction of every sum of products below is spelled out so
// that a lane's bits do not depend on the instantiation: DESIGN.md section 4.  Handing G and Lam^-1 over through LDS, the vector
// half one stage behind, stays rejected: ~18 ds_write per stage on the critical wave.)
// With A = I + dtF (F has 7 nonzeros) the products are organised around W = P+ (dtF), which has only three nonzero
// columns (delta, v, psi):   A'P+A = P+ + W + W' + (dtF)'W,   P+A = P+ + W,
// so the 6x6 product P+A is never formed and P_k is accumulated onto P+ (18 + 12 + 12 temporaries instead of 36 + 21).
// Neither half stores anything: the gains and the cost-to-go stay in registers (RicGain, Ps, pv) and ric_store_stage
// writes them as 16-byte row pairs once both halves are done -- a global store holds the issuing wave for ~25-30 cycles
// whatever its width (tools/ubench/store_cost.hip), so 21 wide stores cost half of 41 narrow ones.
// a b + c d with the fused operation spelled out (which of the two products the compiler fuses is otherwise its choice, per instantiation)
#define MPC_FMA2(a, b, c, d) fma((a), (b), (c) * (d))
template <int NX>
struct RicGain {
    double G0[NX], G1[NX], i00, i01, i11;       // G = B'(P+ A) (+ Hux at stage 0), Lam^-1
    double L00, L01, L11, idet;                 // (SYM: Lam itself, for the compensated products of marked instances)
    bool comp;
    double K0[NX], K1[NX], kf0, kf1;            // feedback gains K = -Lam^-1 G and feed-forward kff (rows of KK)
};

// NE < NX (NE = 5 with NX = 6): the progress state s (index 5: s' = v, zero weight, unbounded) is decoupled -- its row and
// column of the cost-to-go are identically zero as long as no inertia correction is added -- so the recursion runs on NE
// states and writes explicit zeros where the six-state layout has entries of s.
template <int NX, int NE = NX, bool SYM = true>
MPC_HD bool ric_matrix_step(const PRef& P, int k, const RicStage<NX>& s, double delta, double hux0, double hux1, double* Ps, RicGain<NX>& g,
                            bool sym_gk = false) {
    // Which product of a sum a b + c d is fused into the addition is, by default, the optimiser's choice -- made per INSTANTIATION, from what
    // surrounds the expression.  A lane's bits must not depend on whether its wavefront runs the SYM instantiation (some mate carries an
    // inertia correction) or the plain one: here the front end fuses, expression by expression as written, the same way everywhere.
#if defined(__clang__)
#pragma clang fp contract(on)
#endif
    using D = Dim<NX>;
    const double dt = P.dt;
    const double a03 = s.a[0], a04 = s.a[1], a13 = s.a[2], a14 = s.a[3], a42 = s.a[4], a43 = s.a[5];
    // W[i][c] = (P+ dtF)[i][2 + c], c = 0,1,2  (columns delta, v, psi)
    double W[NX][3];
#pragma unroll
    for (int i = 0; i < NE; ++i) {
        const double pi0 = sym<NX>(Ps, i, 0), pi1 = sym<NX>(Ps, i, 1), pi4 = sym<NX>(Ps, i, 4);
        W[i][0] = pi4 * a42;
        double t = pi0 * a03 + pi1 * a13 + pi4 * a43;
        if (NE == 6) t += sym<NX>(Ps, i, 5) * dt;
        W[i][1] = t;
        W[i][2] = pi0 * a04 + pi1 * a14;
    }
    // G = B'(P+A) (+ Hux at stage 0) = dt * rows (2,3) of (P+ + W);  Lam = Ruu + B'P+B
#pragma unroll
    for (int j = 0; j < NE; ++j) {
        double g0 = sym<NX>(Ps, 2, j), g1 = sym<NX>(Ps, 3, j);
        if (j >= 2 && j <= 4) { g0 += W[2][j - 2]; g1 += W[3][j - 2]; }
        g.G0[j] = dt * g0;
        g.G1[j] = dt * g1;
    }
    if (k == 0) { g.G1[2] += hux0; g.G1[3] += hux1; }
    const double L00 = s.ruu[0] + dt * dt * sym<NX>(Ps, 2, 2) + delta;
    const double L01 = dt * dt * sym<NX>(Ps, 2, 3);
    const double L11 = s.ruu[1] + dt * dt * sym<NX>(Ps, 3, 3) + delta;
    // (sym_gk -- instances with heavily weighted circle rows or an inertia correction behind them: Lam = Ruu + w g g' is dominated by a rank-one
    //  term, L00 L11 and L01^2 agree to the first ten digits and the rounding error of L01^2 is as large as det itself -- Kahan's difference of
    //  products; likewise adj(Lam) G below.  This cancellation, not the asymmetry, was what made the collision-avoidance family a lottery of
    //  instances wandering at a KKT error of 1e-8 ... 1e-4 (profiles/r05_ca_lottery.txt).)
    double det = fma(-L01, L01, L00 * L11);             // (spelled out: the same bits in every instantiation)
    if (SYM) {
        const double l01sq = L01 * L01;
        const double detc = fma(L00, L11, -l01sq) - fma(L01, L01, -l01sq);
        det = sym_gk ? detc : det;
    }
    // (no early exit when Lam is not positive definite: the lane just carries garbage to the end of the sweep, which is
    //  repeated with a larger delta_w anyway -- a divergent exit here costs every lane ~70 select instructions per stage)
    const bool pd = (L00 > 0.0) && (det > 0.0);
    const double idet = 1.0 / det;
    g.i00 = L11 * idet; g.i01 = -L01 * idet; g.i11 = L00 * idet;
    if (SYM) { g.L00 = L00; g.L01 = L01; g.L11 = L11; g.idet = idet; g.comp = sym_gk; }
    double* K0 = g.K0;
    double* K1 = g.K1;
#pragma unroll
    for (int j = 0; j < NE; ++j) {
        if (SYM) {
            // -adj(Lam) G / det with the rounding errors of the leading products carried along (same bits as below for the instances without the mark)
            const double a0 = L11 * g.G0[j], b0 = L00 * g.G1[j];
            const double e0 = sym_gk ? fma(L11, g.G0[j], -a0) : 0.0, e1 = sym_gk ? fma(L00, g.G1[j], -b0) : 0.0;
            // (the unmarked form with its fused operation spelled out: the same bits in both instantiations, whatever surrounds it)
            const double k0 = sym_gk ? -((fma(-L01, g.G1[j], a0) + e0) * idet) : -MPC_FMA2(g.i00, g.G0[j], g.i01, g.G1[j]);
            const double k1 = sym_gk ? -((fma(-L01, g.G0[j], b0) + e1) * idet) : -MPC_FMA2(g.i01, g.G0[j], g.i11, g.G1[j]);
            K0[j] = k0;
            K1[j] = k1;
        } else {
            K0[j] = -MPC_FMA2(g.i00, g.G0[j], g.i01, g.G1[j]);
            K1[j] = -MPC_FMA2(g.i01, g.G0[j], g.i11, g.G1[j]);
        }
    }
#pragma unroll
    for (int j = NE; j < NX; ++j) { K0[j] = 0.0; K1[j] = 0.0; g.G0[j] = 0.0; g.G1[j] = 0.0; }
    // P_k = H + P+ + W + W' + (dtF)'W + G'K, upper triangle, accumulated onto P+
#pragma unroll
    for (int i = 0; i < NX; ++i) {
#pragma unroll
        for (int j = i; j < NX; ++j) {
            if (j >= NE) {                                    // entries of the decoupled state: zero
                Ps[D::sidx(i, j)] = 0.0;
                continue;
            }
            double t = Ps[D::sidx(i, j)];
            if (D::hrow(i, j) >= 0) t += s.H[D::sidx(i, j)];
            const double gk = g.G0[i] * K0[j] + g.G1[i] * K1[j];
            t += gk;
            if (j >= 2 && j <= 4) t += W[i][j - 2];
            if (i >= 2 && i <= 4) t += W[j][i - 2];
            if (i >= 2 && i <= 4 && j >= 2 && j <= 4) {          // ((dtF)'W)[i][j], rows/cols (delta, v, psi)
                const int cj = j - 2;
                if (i == 2) t += a42 * W[4][cj];
                if (i == 3) { t += a03 * W[0][cj] + a13 * W[1][cj] + a43 * W[4][cj]; if (NE == 6) t += dt * W[5][cj]; }
                if (i == 4) t += a04 * W[0][cj] + a14 * W[1][cj];
            }
            if (i == j) t += delta;
            // Nonconvex instances (any that ever needed an inertia correction): the term G'K = -G' Lam^-1 G cancels most of A'P+A once
            // active circle rows put weights of 1/mu into the cost-to-go, and the rounding of K makes G'K slightly unsymmetric -- taking
            // (i, j) from one triangle only then feeds an error of 1e-16 x 1e9 back into every later stage, spurious "indefinite" verdicts
            // and steps that do not reduce the KKT error follow (collision avoidance: up to 95 iterations where the dense-KKT solver
            // needs 26).  The mean of the two triangles -- what symmetrising P_k amounts to -- removes that; 3 more instructions per entry,
            // so only for the instances that need it (lane following never does: same bits as before).  SYM = false is the
            // instantiation without the term, for a wavefront none of whose instances asks for it (adding the 0.0 of the select
            // changes no bits, so which of the two a wavefront runs does not show in the results).
            if (SYM && i != j) t += sym_gk ? 0.5 * ((g.G0[j] * K0[i] + g.G1[j] * K1[i]) - gk) : 0.0;
            Ps[D::sidx(i, j)] = t;
        }
    }
    return pd;
}

// Pn = P_{k+1} (the cost-to-go the matrix half STARTED from), g = what the matrix half of stage k left; pv: p+ -> p_k
template <int NX, int NE = NX, bool SYM = false>
MPC_HD void ric_vector_step(const PRef& P, const RicStage<NX>& s, const double* Pn, RicGain<NX>& g, double* pv) {
#if defined(__clang__)
#pragma clang fp contract(on)          // (see ric_matrix_step)
#endif
    using D = Dim<NX>;
    constexpr int NS = D::NS;
    const double dt = P.dt;
    const double a03 = s.a[0], a04 = s.a[1], a13 = s.a[2], a14 = s.a[3], a42 = s.a[4], a43 = s.a[5];
    // h = p+ - P+ c_{k+1}
    double h[NX];
#pragma unroll
    for (int i = 0; i < NE; ++i) {
        double t = pv[i];
#pragma unroll
        for (int j = 0; j < NE; ++j) t -= sym<NX>(Pn, i, j) * s.cn[j];
        h[i] = t;
    }
    // l = gu + B'h,  kff = -Lam^-1 l
    const double l0 = s.gu[0] + dt * h[2], l1 = s.gu[1] + dt * h[3];
    double kf0 = -MPC_FMA2(g.i00, l0, g.i01, l1), kf1 = -MPC_FMA2(g.i01, l0, g.i11, l1);
    if (SYM) {           // (as for the gain rows in ric_matrix_step)
        const double a0 = g.L11 * l0, b0 = g.L00 * l1;
        const double c0 = -((fma(-g.L01, l1, a0) + fma(g.L11, l0, -a0)) * g.idet), c1 = -((fma(-g.L01, l0, b0) + fma(g.L00, l1, -b0)) * g.idet);
        kf0 = g.comp ? c0 : kf0;
        kf1 = g.comp ? c1 : kf1;
    }
    g.kf0 = kf0;
    g.kf1 = kf1;
    // p_k = gx + A'h + G'kff
#pragma unroll
    for (int i = 0; i < NX; ++i) {
        if (i >= NE) { pv[i] = 0.0; continue; }
        double t = s.gx[i] + h[i] + g.G0[i] * kf0 + g.G1[i] * kf1;
        if (i == 2) t += a42 * h[4];
        if (i == 3) { t += a03 * h[0] + a13 * h[1] + a43 * h[4]; if (NE == 6) t += dt * h[NX - 1]; }
        if (i == 4) t += a04 * h[0] + a14 * h[1];
        pv[i] = t;
    }
}

// rows of stage k: gains [K0 | K1 | kff] -> KK, cost-to-go [P_k upper triangle | p_k] -> PK
template <int NX>
MPC_HD void ric_store_stage(const PRef& P, uint32_t bb, int k, const double* Ps, const double* pv, const RicGain<NX>& g) {
    using D = Dim<NX>;
    double kk[D::NKK], pk[D::NPK];
#pragma unroll
    for (int j = 0; j < NX; ++j) { kk[j] = g.K0[j]; kk[NX + j] = g.K1[j]; }
    kk[2 * NX] = g.kf0;
    kk[2 * NX + 1] = g.kf1;
#pragma unroll
    for (int i = 0; i < D::NS; ++i) pk[i] = Ps[i];
#pragma unroll
    for (int i = 0; i < NX; ++i) pk[D::NS + i] = pv[i];
    ws_store_rows<D::NKK>(MPC_ROWS(MPC_UK(P.KK, D::NKK, k, e)), kk);
    ws_store_rows<D::NPK>(MPC_ROWS(MPC_UK(P.PK, D::NPK, k, e)), pk);
}

// The same rows as two disjoint sets of 16-byte row pairs, for the two compute waves of riccati_tile's backward sweep (each pair is
// written whole by exactly one of them, so the order in which the two waves' stores land does not matter):
//   ric_store_matrix  what the matrix half alone knows: the gain rows K0, K1 (pairs 0 .. NX-1 of KK) and the pairs of PK that hold only P_k
//   ric_store_vector  everything with an entry of the vector half in it: the (kf0, kf1) pair of KK and the pairs of PK from the first one
//                     that holds an entry of p_k -- the mixed pair (P_k[NS-1], p_k[0]) included, where NS is odd (NX = 5 and 6): the wave
//                     that runs the vector half carries P_k as well -- to the end (NPK odd, NX = 6: the last row on its own)
// Together they write the rows of ric_store_stage, each once.  PK_SPLIT: first row of PK that belongs to the vector set.
template <int NX>
struct RicSplit { static constexpr int PK_SPLIT = Dim<NX>::NS & ~1; };
template <int NX>
MPC_HD void ric_store_matrix_pk(const PRef& P, uint32_t bb, int k, const double* Ps) {
    using D = Dim<NX>;
    ws_store_rows<RicSplit<NX>::PK_SPLIT>(MPC_ROWS(MPC_UK(P.PK, D::NPK, k, e)), Ps);
}
template <int NX>
MPC_HD void ric_store_vector_pk(const PRef& P, uint32_t bb, int k, const double* Ps, const double* pv) {
    using D = Dim<NX>;
    constexpr int S0 = RicSplit<NX>::PK_SPLIT, CNT = D::NPK - S0;
    double pk[CNT];
#pragma unroll
    for (int i = S0; i < D::NS; ++i) pk[i - S0] = Ps[i];
#pragma unroll
    for (int i = 0; i < NX; ++i) pk[D::NS - S0 + i] = pv[i];
    ws_store_rows<CNT>(MPC_ROWS(MPC_UK(P.PK, D::NPK, k, S0 + e)), pk);
}
template <int NX>
MPC_HD void ric_store_matrix(const PRef& P, uint32_t bb, int k, const double* Ps, const RicGain<NX>& g) {
    using D = Dim<NX>;
    double kk[2 * NX];
#pragma unroll
    for (int j = 0; j < NX; ++j) { kk[j] = g.K0[j]; kk[NX + j] = g.K1[j]; }
    ws_store_rows<2 * NX>(MPC_ROWS(MPC_UK(P.KK, D::NKK, k, e)), kk);
    ric_store_matrix_pk<NX>(P, bb, k, Ps);
}
template <int NX>
MPC_HD void ric_store_vector(const PRef& P, uint32_t bb, int k, const double* Ps, const double* pv, const RicGain<NX>& g) {
    using D = Dim<NX>;
    MPC_ST2(MPC_UK(P.KK, D::NKK, k, 2 * NX), g.kf0, g.kf1);
    ric_store_vector_pk<NX>(P, bb, k, Ps, pv);
}

// both halves on one thread: consumes stage block `s`, updates (Ps, pv) IN PLACE, stores gains and cost-to-go
template <int NX, int NE = NX, bool SYM = true>
MPC_HD bool riccati_backward_step(const PRef& P, uint32_t bb, int k, const RicStage<NX>& s, double delta, double hux0,
                                  double hux1, double* Ps, double* pv, bool sym_gk = false) {
    constexpr int NS = Dim<NX>::NS;
    double Pn[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) Pn[i] = Ps[i];
    RicGain<NX> g;
    if (!ric_matrix_step<NX, NE, SYM>(P, k, s, delta, hux0, hux1, Ps, g, sym_gk)) return false;
    ric_vector_step<NX, NE, SYM>(P, s, Pn, g, pv);
    ric_store_stage<NX>(P, bb, k, Ps, pv, g);
    return true;
}

// the step with the decoupled-state shortcut where it applies: six states, flagged by the host, and no inertia correction in
// this sweep (delta_w would put a nonzero entry on the diagonal of the decoupled state)
template <int NX>
MPC_HD bool ric_bwd_any(const PRef& P, uint32_t bb, int k, const RicStage<NX>& s, double delta, double hux0, double hux1,
                        double* Ps, double* pv, bool sym_gk = false) {
    // (measured on MI355X: the five-state recursion -- 301 instead of 402 instructions per stage -- does not shorten the
    //  stage, 40.4 vs 39.8 us per launch, so the GPU kernel runs the general step; the emulation harness keeps exercising
    //  the NE = 5 instantiation through this function so that it stays correct)
    if (NX == 6 && P.dec_s && delta == 0.0) return riccati_backward_step<NX, (NX == 6 ? 5 : NX)>(P, bb, k, s, delta, hux0, hux1, Ps, pv, sym_gk);
    return riccati_backward_step<NX>(P, bb, k, s, delta, hux0, hux1, Ps, pv, sym_gk);
}

// stage data of the forward sweep
template <int NX>
struct FwdStage {
    double K0[NX], K1[NX], kf0, kf1, a[6], cn[NX];
};
template <int NX>
MPC_HD void fwd_load(const PRef& P, uint32_t bb, int k, FwdStage<NX>& f) {
    using D = Dim<NX>;
#pragma unroll
    for (int j = 0; j < NX; ++j) {
        f.K0[j] = MPC_UK(P.KK, D::NKK, k, j);
        f.K1[j] = MPC_UK(P.KK, D::NKK, k, NX + j);
        f.cn[j] = MPC_UK(P.BLK, D::NBLK, k, D::B_CN + j);
    }
    f.kf0 = MPC_UK(P.KK, D::NKK, k, 2 * NX);
    f.kf1 = MPC_UK(P.KK, D::NKK, k, 2 * NX + 1);
#pragma unroll
    for (int i = 0; i < 6; ++i) f.a[i] = MPC_UK(P.BLK, D::NBLK, k, D::B_A + i);
}

// one step of the forward sweep: du_k = K dx_k + kff, dx_{k+1} = A dx_k + B du_k - c_{k+1}; stores (du_k, dx_k)
template <int NX>
MPC_HD void riccati_forward_step(const PRef& P, uint32_t bb, int k, const FwdStage<NX>& f, double* dx) {
    using D = Dim<NX>;
    const double dt = P.dt;
    double du0 = f.kf0, du1 = f.kf1;
#pragma unroll
    for (int j = 0; j < NX; ++j) { du0 += f.K0[j] * dx[j]; du1 += f.K1[j] * dx[j]; }
    {
        double dz[D::NZ];
        dz[0] = du0;
        dz[1] = du1;
#pragma unroll
        for (int i = 0; i < NX; ++i) dz[2 + i] = dx[i];
        ws_store_rows<D::NZ>(MPC_ROWS(MPC_UK(P.DZ, D::NZ, k, e)), dz);
    }
    double dn[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) dn[i] = dx[i] - f.cn[i];
    dn[0] += f.a[0] * dx[3] + f.a[1] * dx[4];
    dn[1] += f.a[2] * dx[3] + f.a[3] * dx[4];
    dn[2] += dt * du0;
    dn[3] += dt * du1;
    dn[4] += f.a[4] * dx[2] + f.a[5] * dx[3];
    if (NX == 6) dn[5] += dt * dx[3];
#pragma unroll
    for (int i = 0; i < NX; ++i) dx[i] = dn[i];
}

template <int NX>
MPC_HD void riccati_instance(const PRef& P, int b) {
    using D = Dim<NX>;
    constexpr int NS = D::NS;
    const int N = P.N;
    const uint32_t Bp = (uint32_t)P.Bp, bb = (uint32_t)b;
    if (MPC_U(P.ISC, (uint32_t)IS_STATUS) != ST_RUNNING) return;
    const double dt = P.dt;
    const double delta_last = MPC_U(P.SC, (uint32_t)SC_DLAST);
    const double hux0 = MPC_U(P.SC, (uint32_t)SC_HUX0), hux1 = MPC_U(P.SC, (uint32_t)SC_HUX1);
    double delta = 0.0;
    bool ok = false;
    for (;;) {
        ok = true;
        double Ps[NS], pv[NX];
        RicStage<NX> cur, nxt;
        ric_load<NX>(P, b, N - 1, cur);        // in flight while the terminal block is processed
        {
            RicStage<NX> s;
            ric_load<NX>(P, b, N, s);
#pragma unroll
            for (int i = 0; i < NS; ++i) Ps[i] = s.H[i];
#pragma unroll
            for (int i = 0; i < NX; ++i) { Ps[D::sidx(i, i)] += delta; pv[i] = s.gx[i]; }
#pragma unroll
            for (int i = 0; i < NS; ++i) MPC_UK(P.PK, D::NPK, N, i) = Ps[i];
#pragma unroll
            for (int i = 0; i < NX; ++i) MPC_UK(P.PK, D::NPK, N, NS + i) = pv[i];
        }
        // software pipeline: the block of stage k-1 is requested before stage k is processed, so its HBM latency
        // overlaps the ~330 fp64 operations of the step (two stages per trip: cur/nxt ping-pong without copies)
        int k = N - 1;
        for (; k >= 1; k -= 2) {
            ric_load<NX>(P, b, k - 1, nxt);
            if (!ric_bwd_any<NX>(P, bb, k, cur, delta, hux0, hux1, Ps, pv, delta != 0.0 || delta_last != 0.0)) { ok = false; break; }
            if (k >= 2) ric_load<NX>(P, b, k - 2, cur);
            if (!ric_bwd_any<NX>(P, bb, k - 1, nxt, delta, hux0, hux1, Ps, pv, delta != 0.0 || delta_last != 0.0)) { ok = false; break; }
        }
        if (ok && k == 0) {
            if (!ric_bwd_any<NX>(P, bb, 0, cur, delta, hux0, hux1, Ps, pv, delta != 0.0 || delta_last != 0.0)) ok = false;
        }
        if (ok) break;
        if (delta == 0.0) delta = (delta_last == 0.0) ? DW_0 : fmax(DW_MIN, KW_MINUS * delta_last);
        else delta *= (delta_last == 0.0) ? KW_PLUS_BAR : KW_PLUS;
        if (delta > DW_MAX) break;
    }
    if (!ok) { MPC_U(P.ISC, (uint32_t)IS_STATUS) = P.emit ? ST_SWEEP_FAILED : -7; return; }
    if (delta > 0.0) MPC_U(P.SC, (uint32_t)SC_DLAST) = delta;
    MPC_U(P.SC, (uint32_t)SC_DELTA) = delta;
    // forward sweep (same software pipeline)
    double dx[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) dx[i] = -MPC_U(P.SC, (uint32_t)(SC_C0 + i));
    FwdStage<NX> fa, fb;
    fwd_load<NX>(P, bb, 0, fa);
    auto fwd_step = [&](int k, const FwdStage<NX>& f) { riccati_forward_step<NX>(P, bb, k, f, dx); };
    int k = 0;
    for (; k + 1 < N; k += 2) {
        fwd_load<NX>(P, bb, k + 1, fb);
        fwd_step(k, fa);
        if (k + 2 < N) fwd_load<NX>(P, bb, k + 2, fa);
        fwd_step(k + 1, fb);
    }
    if (k < N) fwd_step(k, fa);
    {
        MPC_UK(P.DZ, D::NZ, N, 0) = 0.0;
        MPC_UK(P.DZ, D::NZ, N, 1) = 0.0;
#pragma unroll
        for (int i = 0; i < NX; ++i) MPC_UK(P.DZ, D::NZ, N, 2 + i) = dx[i];
    }
}

// =========================================================================================================
// output: SoA iterate -> caller's row-major x_out + per-instance status
// =========================================================================================================
template <int NX>
MPC_HD void output_instance(const PRef& P, int b) {
    using D = Dim<NX>;
    const int N = P.N;
    const uint32_t Bp = (uint32_t)P.Bp, bb = (uint32_t)b;
    const size_t nw = (size_t)2 * N + (size_t)NX * (N + 1);
    MPC_GLOBAL_AS double* xo = (MPC_GLOBAL_AS double*)P.x_out + (size_t)bb * nw;
    for (int k = 0; k <= N; ++k) {
        if (k < N) {
            xo[2 * k] = MPC_UK(P.Z, D::NZ, k, 0);
            xo[2 * k + 1] = MPC_UK(P.Z, D::NZ, k, 1);
        }
        for (int i = 0; i < NX; ++i) xo[2 * N + NX * k + i] = MPC_UK(P.Z, D::NZ, k, 2 + i);
    }
    int st = MPC_U(P.ISC, (uint32_t)IS_STATUS);
    if (st == ST_RUNNING) st = 0;     // iteration budget of the launch loop exhausted
    if (P.status_out) P.status_out[b] = st;
    if (P.iters_out) P.iters_out[b] = MPC_U(P.ISC, (uint32_t)IS_ITERS);
    if (P.kkt_out) P.kkt_out[b] = MPC_U(P.SC, (uint32_t)SC_E0);
}

// =========================================================================================================
// The NLP as the caller states it (mpc_eval_nlp_batch, the f / g outputs of mpc_solve_batch_ex) and the solver's multipliers mapped
// onto its rows (lam_g / lam_x).  One call per (instance, stage); plain pointers, no workspace accessors: the same code runs in the
// kernels k_eval_nlp / k_mult_out and in the CPU harness of the tests.
// Rows of g (n_g = 1 + nx (N + 1) + 9 (N + 1), the rows of mpc_set_bounds): 0 friction | 1 .. nx the x_0 pin | nx per defect k -> k + 1 |
// 9 per stage: circle pair j (j = 0, 1, 2) three times (optimizer.py:395-403).
// =========================================================================================================
MPC_HD int nlp_n_g(const Params& P) { return 1 + P.nx * (P.N + 1) + 9 * (P.N + 1); }

// stage k of instance (w, pr: its rows of x and p, obst: its six circle centres): the g rows stage k owns (row 0 and the pin at k = 0,
// the defect k-1 -> k at k >= 1, the circle rows of stage k) -> g (the instance's row, may be null); returns the stage's cost term
template <int NX>
MPC_HD double nlp_eval_stage(const Params& P, const double* w, const double* pr, const double* obst, const int k, double* g) {
    const int N = P.N;
    const double* x = w + 2 * N + NX * k;
    double fk = 0.0;
    if (k < N) {
        const double* u = w + 2 * k;
        const double* rn = pr + 2 * N + NX * (k + 1);
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            const double e = x[i] - rn[i];
            fk += P.Q[i] * e * e;
        }
        fk += P.R[0] * u[0] * u[0] + P.R[1] * u[1] * u[1];
    }
    if (g == nullptr) return fk;
    if (k == 0) {
        g[0] = friction_eval(P, w[1], x[2], x[3], nullptr, nullptr, false);
#pragma unroll
        for (int i = 0; i < NX; ++i) g[1 + i] = x[i] - pr[2 * N + i];
    } else {
        const double* xp = w + 2 * N + NX * (k - 1);
        const double* up = w + 2 * (k - 1);
        double f[NX], s, c, td;
        ode_eval<NX>(P, xp, up, f, s, c, td);
#pragma unroll
        for (int i = 0; i < NX; ++i) g[1 + NX * k + i] = x[i] - (f[i] * P.dt + xp[i]);
    }
    double sps, cps;
    mpc_sincos(x[4], sps, cps);
    const int r0 = 1 + NX * (N + 1) + 9 * k;
    for (int j = 0; j < 3; ++j) {
        const double d = circle_eval(P, obst, j, x[0], x[1], sps, cps, nullptr, nullptr, false);
        for (int q = 0; q < 3; ++q) g[r0 + 3 * j + q] = d;
    }
    return fk;
}

// Where the final iterate of an instance lies: the tile-major rows (MPC_K) or the instance-major mailbox (MPC_KI, k_solve_wg)
MPC_HD size_t mult_tile_index(const Params& P, const int R, const int k, const int e, const int b) {
    return ws_index(P, (const double*)nullptr, (uint32_t)(k * (int)MPC_EV(R) + e), (uint32_t)b);
}
MPC_HD size_t mult_mb_index(const Params& P, const int R, const int k, const int e, const int b) {
    return (size_t)b * (size_t)(P.N + 1) * MPC_EV(R) + (size_t)(e >> 1) * (size_t)(P.N + 1) * 2 + (size_t)k * 2 + (size_t)(e & 1);
}
MPC_HD double mult_row(const Params& P, const double* tile, const double* mb, const bool in_mb, const int R, const int k, const int e, const int b) {
    return in_mb ? mb[mult_mb_index(P, R, k, e, b)] : tile[mult_tile_index(P, R, k, e, b)];
}

// Multipliers of stage k of instance b in CasADi's convention, grad f + J_g' lam_g + lam_x = 0: the kernels' multipliers of the objective
// scaled by df (SC_DF) are divided by it; lam_x = z_U - z_L, 0 where the variable has no finite bound; the kernels carry the copies of a
// circle row once, with weight m = obst_mult and multiplier nu: each of the three copies of the NLP gets m nu / 3 (nu itself for the
// reference's m = 3).  The stage-0 friction row:
//   kept as a row (IS_FROW != 0; friction_lb = ipopt, or |a_0^2 + c| <= a_max is not one interval): lam_g[0] = nu_f / df
//   presolved into bounds of a_0 (prestart_a0_of): a side of a_0 whose bound is tighter than the caller's lbx / ubx comes from the row,
//     lam_g[0] = (z_U - z_L of those sides) / (d g_0 / d a_0), d g_0 / d a_0 = 2 a_0 sign(a_0^2 + c); the pin rows give back what the row
//     gradient adds in (delta_0, v_0): lam_pin -= lam_g[0] d g_0 / d (delta_0, v_0)
//   at the kink a_0^2 + c = 0 (the row is not differentiable there) lam_g[0] = NaN.
// w: the instance's returned row of x (the friction row's gradient is taken there).  lam_g / lam_x: the instance's output rows.
template <int NX>
MPC_HD void mult_stage(const Params& P, const int b, const int k, const bool in_mb, const double* w, double* lam_g, double* lam_x) {
    constexpr int NZ = NX + 2;
    const int N = P.N;
    const double wm = P.obst_mult / 3.0;
    const double idf = 1.0 / P.SC[ws_index(P, P.SC, (uint32_t)SC_DF, (uint32_t)b)];
    double zl[NZ], zu[NZ], lam[NX];
#pragma unroll
    for (int i = 0; i < NZ; ++i) {
        zl[i] = mult_row(P, P.ZL, P.MZL, in_mb, NZ, k, i, b);
        zu[i] = mult_row(P, P.ZU, P.MZU, in_mb, NZ, k, i, b);
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) lam[i] = mult_row(P, P.LAM, P.MLAM, in_mb, NX, k, i, b) * idf;
    // bound multipliers
#pragma unroll
    for (int i = 0; i < NZ; ++i) {
        if (i < 2 && k == N) continue;
        const double lb = P.LB[k * NZ + i], ub = P.UB[k * NZ + i];
        double v = 0.0;
        if (has_lo(lb)) v -= zl[i];
        if (has_hi(ub)) v += zu[i];
        if (k == 0 && i == 1) continue;              // a_0: below, with the friction row
        lam_x[i < 2 ? 2 * k + i : 2 * N + NX * k + (i - 2)] = v * idf;
    }
    if (k == 0) {
        const double a = w[1], dl = w[2 * N + 2], v0 = w[2 * N + 3];
        double gr[3], h[4];
        friction_eval(P, a, dl, v0, gr, h, true);
        const bool kink = a * a + v0 * (tan(dl) * v0 / P.friction_div) == 0.0;        // (friction_eval's sign(0) = 0: a zero gradient)
        const bool frow = P.ISC[ws_index(P, P.ISC, (uint32_t)IS_FROW, (uint32_t)b)] != 0;
        const double a0lb = P.SC[ws_index(P, P.SC, (uint32_t)SC_A0LB, (uint32_t)b)], a0ub = P.SC[ws_index(P, P.SC, (uint32_t)SC_A0UB, (uint32_t)b)];
        const double lb = P.LB[1], ub = P.UB[1];
        double lg0, zx = 0.0;
        if (frow) {
            lg0 = P.SC[ws_index(P, P.SC, (uint32_t)SC_NUF, (uint32_t)b)] * idf;
            if (has_lo(lb)) zx -= zl[1];
            if (has_hi(ub)) zx += zu[1];
        } else {
            // sides of a_0 that the presolved row set (tighter than the caller's bound), and those that are the caller's own
            double zr = 0.0;
            if (has_lo(a0lb)) { if (a0lb > lb) zr -= zl[1]; else zx -= zl[1]; }
            if (has_hi(a0ub)) { if (a0ub < ub) zr += zu[1]; else zx += zu[1]; }
            lg0 = (gr[0] != 0.0) ? zr * idf / gr[0] : 0.0;
            lam[2] -= lg0 * gr[1];
            lam[3] -= lg0 * gr[2];
        }
        lam_x[1] = zx * idf;
        lam_g[0] = kink ? NAN : lg0;
#pragma unroll
        for (int i = 0; i < NX; ++i) lam_g[1 + i] = lam[i];
    } else {
#pragma unroll
        for (int i = 0; i < NX; ++i) lam_g[1 + NX * k + i] = lam[i];
    }
    const int r0 = 1 + NX * (N + 1) + 9 * k;
    for (int j = 0; j < 3; ++j) {
        const double nu = mult_row(P, P.NUO, P.MNUO, in_mb, 3, k, j, b) * idf * wm;
        for (int q = 0; q < 3; ++q) lam_g[r0 + 3 * j + q] = nu;
    }
}
// the rows mult_stage writes for stage k, all set to v (NaN: the instance did not converge)
template <int NX>
MPC_HD void mult_stage_fill(const Params& P, const int k, const double v, double* lam_g, double* lam_x) {
    const int N = P.N;
    if (k < N) { lam_x[2 * k] = v; lam_x[2 * k + 1] = v; }
    for (int i = 0; i < NX; ++i) lam_x[2 * N + NX * k + i] = v;
    if (k == 0) lam_g[0] = v;
    for (int i = 0; i < NX; ++i) lam_g[1 + NX * k + i] = v;
    const int r0 = 1 + NX * (N + 1) + 9 * k;
    for (int q = 0; q < 9; ++q) lam_g[r0 + q] = v;
}

}  // namespace mpc
