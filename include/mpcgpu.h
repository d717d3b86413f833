/*
 * mpcgpu.h -- C-ABI of the MI355X-native batched NLP solver for the receding-horizon optimisation of
 *             TGoldC/Motion-Planning-for-Autonomous-Driving-with-MPC (MPC_Planner/optimizer.py).
 *
 * This is the drop-in boundary.  What each entry point replaces in the reference:
 *
 *   mpc_create / mpc_destroy ........ `ca.nlpsol('solver','ipopt', nlp_prob, opts_setting)`
 *                                     (MPC_Planner/optimizer.py:513-560, rebuilt every step at :605) and
 *                                     `model.generate_solver(options=codeoptions)` (optimizer.py:197-245).
 *                                     The handle owns the device workspace; create it once, reuse it.
 *   mpc_set_bounds .................. the `lbg, ubg, lbx, ubx` lists of `inequal_constraints()`
 *                                     (optimizer.py:413-491) that the reference passes to every `sol(...)` call.
 *   mpc_solve_batch ................. `res = sol(x0=init_control, p=c_p, lbg=lbg, lbx=lbx, ubg=ubg, ubx=ubx)`
 *                                     (optimizer.py:607) for B independent instances at once; row b of x_out is
 *                                     `res['x'].full().ravel()` of instance b (optimizer.py:609).
 *                                     FORCESPRO twin: `solver.solve(problem)` (optimizer.py:326), C side
 *                                     `FORCESNLPsolver_solve(params, output, info, fs, extfunc)`
 *                                     (test/FORCESNLPsolver/include/FORCESNLPsolver.h:219); the status codes
 *                                     below follow that header's exit codes (FORCESNLPsolver.h:68-106).
 *   mpc_solve_batch_dev ............. same with device-resident buffers on a caller-supplied HIP stream
 *                                     (no PCIe traffic; this is what bench.py times).
 *   mpc_plant_step .................. `shift_movement` plant update `x0 + delta_t * f(x0, u[:,0])`
 *                                     (optimizer.py:645-650) / `model.eq` RK4 step (optimizer.py:98,356).
 *   mpc_closed_loop_batch[_dev] ..... the loop body of `CasadiOptimizer.optimize` between two solves (optimizer.py:596-631,
 *                                     645-702): first control, plant step, shifted warm start, next reference window.
 *   mpc_forces_stage_eval ........... `FORCESNLPsolver_casadi2forces` (test/FORCESNLPsolver/FORCESNLPsolver_interface.c:41-198):
 *                                     FORCES-mode stage cost / RK4 dynamics / inequalities with their derivatives.
 *   mpc_forces_solve_batch .......... `output, exitflag, info = solver.solve(problem)` of ForcesproOptimizer (optimizer.py:326).
 *   mpc_forces_closed_loop_batch .... the loop of ForcesproOptimizer.optimize around it (optimizer.py:246-366).
 *   mpc_forces_closed_loop_batch_obst  that loop past per-ego moving obstacles, predicted per stage, with a guess that follows the plan.
 *   mpc_metrics_batch ............... deviation.txt / RMSD.txt of MPCPlanner (mpc_planner.py:184-199, 279-292), circle clearance.
 *   mpc_validity_batch .............. the collision / road-boundary verdict of test/test_mpc_planner.py:37-47.
 *
 * Conventions (modelled on FORCESNLPsolver.h:117-203): caller-owned plain buffers, int return codes, no
 * exceptions, no callbacks, no globals; the library never keeps a host pointer past the call.
 * Row layout of x0 / p / x_out is the reference's decision-vector order (optimizer.py:550,552):
 *     [u_0(2) u_1(2) ... u_{N-1}(2) | x_0(nx) x_1(nx) ... x_N(nx)],   n_w = 2 N + nx (N + 1)
 * All floating point is IEEE double.  A handle is not thread-safe: one handle per host thread / stream.
 */
#ifndef MPCGPU_H
#define MPCGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPCGPU_ABI_VERSION 1

/* per-instance numerical status (FORCESNLPsolver.h:68-106 semantics) */
#define MPC_STATUS_CONVERGED   1    /* OPTIMAL: scaled KKT error <= tol                        */
#define MPC_STATUS_MAXITER     0    /* MAXITREACHED                                            */
#define MPC_STATUS_NAN        (-6)  /* BADFUNCEVAL: NaN/Inf met in a function evaluation       */
#define MPC_STATUS_NOPROGRESS (-7)  /* NOPROGRESS: line search or regularisation gave up       */

/* API return codes (0 = ok, negative = error; mpc_last_error() has the text) */
#define MPC_OK                 0
#define MPC_ERR_INVALID      (-1)   /* bad argument / unsupported problem shape                */
#define MPC_ERR_HIP          (-2)   /* HIP runtime failure (no device, OOM, launch error)      */
#define MPC_ERR_BOUNDS       (-3)   /* lbg/ubg do not have the structure of optimizer.py:421-469 */
#define MPC_ERR_STATE        (-4)   /* call order (e.g. solve before set_bounds)               */

/* formulation of the stage model */
#define MPC_FORM_CASADI_EULER  0    /* CasadiOptimizer: forward Euler multiple shooting (optimizer.py:380-382) */

typedef struct mpc_handle mpc_handle;

typedef struct mpc_problem_desc {
    int32_t N;             /* predict_horizon (optimizer.py:520); 1 <= N <= 127 for the NLP entry points,
                              <= 192 for the FORCES-mode solve; a handle of a longer horizon is refused
                              (MPC_ERR_INVALID) by the entry points that cannot run it                    */
    int32_t nx;            /* 5 = reference state [x, y, delta, v, psi]; 6 appends a decoupled progress
                              state s (s' = v, no weight, unbounded) used by the synthetic benchmark      */
    int32_t nu;            /* must be 2: [deltaDot, aLong]                                                */
    int32_t formulation;   /* MPC_FORM_CASADI_EULER                                                       */
    int32_t max_iter;      /* ipopt.max_iter = 100 (optimizer.py:556)                                     */
    int32_t fixed_iters;   /* 0 = iterate to convergence; k > 0 = exactly k iterations (benchmark mode)   */
    int32_t obst_mult;     /* 3: each of the 3 circle-pair distances is appended 3x (optimizer.py:395-403)*/
    int32_t device;        /* HIP device ordinal                                                          */
    double dt;             /* scenario.dt (optimizer.py:52)                                               */
    double wheelbase;      /* p.a + p.b = 2.5789128 (configuration.py:362-363)                            */
    double friction_div;   /* literal 2.578 of optimizer.py:378                                           */
    double ego_offset;     /* centre offset of the front/rear ego circle, 0.75 (configuration.py:69-93)   */
    double tol;            /* IPOPT tol, 1e-8                                                             */
    double Q[8];           /* diag(weight_x, weight_y, weight_steering_angle, weight_velocity,
                              weight_heading_angle[, 0]) (optimizer.py:500-502)                           */
    double R[2];           /* diag(weight_velocity_steering_angle, weight_long_acceleration) (:503)       */
    double P[8];           /* terminal weights (:504-505) -- built but unused by the CasADi cost (dead
                              expression at :510); kept for the FORCES formulation                        */
    double obstacle[6];    /* obstacle circle centres (x,y) x 3: centre, front, rear (optimizer.py:60-64) */
} mpc_problem_desc;

/* fills *desc with the reference defaults for horizon N and nx in {5,6} (ZAM_Over-1_1 lane-following
 * weights, dummy obstacle at (-100,0)) */
void mpc_default_desc(mpc_problem_desc* desc, int32_t N, int32_t nx);

int mpc_create(mpc_handle** out, const mpc_problem_desc* desc);
int mpc_destroy(mpc_handle* h);
const char* mpc_last_error(const mpc_handle* h);   /* h may be NULL: error of the last failed mpc_create */

/* lbx/ubx: n_w entries (optimizer.py:470-491), +-inf = absent.  lbg/ubg: n_g = 1 + nx(N+1) + 9(N+1) entries
 * (optimizer.py:421-469): row 0 friction [lo, hi]; nx(N+1) equality rows (lbg == ubg); 9(N+1) obstacle rows,
 * all with the same [lo, hi].  Anything else -> MPC_ERR_BOUNDS.  A friction lower bound <= 0 is implied by the
 * absolute value in the row and gets no barrier.  Passing NULL for all four installs the reference defaults.
 * Like mpc_set_weights and like a solve, it ends the life of the sensitivity snapshot (the same bounds again included):
 * mpc_sens_adjoint / mpc_sens_obst / mpc_sens_weights / mpc_sens_bounds after it -> MPC_ERR_STATE (their factor reads
 * the bounds, which must be those of the solve).
 * mpc_get_bounds: the bounds that are installed, as they were given (the defaults of an all-NULL call included), in the
 * same layout; any argument may be NULL.  Before the first mpc_set_bounds -> MPC_ERR_STATE.                         */
int mpc_set_bounds(mpc_handle* h, const double* lbx, const double* ubx, const double* lbg, const double* ubg);
int mpc_get_bounds(const mpc_handle* h, double* lbx, double* ubx, double* lbg, double* ubg);

/* Replaces the cost weights of a live handle: Q [5] -> desc.Q[0..4], R [2] -> desc.R[0..1]; NULL keeps the current ones.  Q[5] (the progress
 * state's weight), P, the bounds and every option stay.  A non-finite value, a Q[i] < 0 or an R[j] <= 0 (R > 0 keeps the KKT matrix's input
 * blocks positive definite) -> MPC_ERR_INVALID, and the handle is as it was.  Host bookkeeping only: no device work and no synchronisation.
 * Every launch carries its weights by value, so work already enqueued keeps the weights it was enqueued with; every call from the next one on
 * -- NLP solves, closed loops and the FORCES-mode entries, which read the same descriptor -- sees the new ones.  Like a solve, it ends the
 * life of the sensitivity snapshot: mpc_sens_adjoint / mpc_sens_obst / mpc_sens_weights / mpc_sens_bounds after it -> MPC_ERR_STATE (their
 * factor reads the weights, which must be those of the solve).  mpc_set_bounds does the same.                                               */
int mpc_set_weights(mpc_handle* h, const double* Q, const double* R);

/* Host-buffer entry point.  x0, p, x_out: [B, n_w] row-major.  obst: [B, 6] per-instance obstacle circle
 * centres or NULL (shared centres of the descriptor).  status/iters/kkt: [B], any may be NULL.            */
int mpc_solve_batch(mpc_handle* h, int32_t B, const double* x0, const double* p, const double* obst,
                    double* x_out, int32_t* status, int32_t* iters, double* kkt);

/* Second chance (both entry points, on unless the option "rescue" is "0"; not in fixed_iters mode): instances whose line search
 * or regularisation gave up (status -7, where IPOPT would enter its feasibility-restoration phase) or that ran out of
 * iterations are re-solved on the device with the lower bound of the circle-distance rows raised in steps from 0 to its value,
 * each level warm-started from the last; the final level is the original problem, so a row that comes back with status 1 is a
 * KKT point of the ORIGINAL NLP to the original tolerance (possibly another local optimum than IPOPT's); rows that still fail keep
 * their first result and status.  iters[] includes the iterations of the second chance.  mpc_last_rescued: how many instances
 * of the last solve took it.                                                                                              */
int mpc_last_rescued(const mpc_handle* h);

/* Device-buffer entry point: same arguments as device pointers, work enqueued on `stream` (a hipStream_t,
 * NULL = default stream).  Returns after enqueueing + the convergence polls; the outputs are complete when
 * the stream is synchronised (the call itself synchronises the stream unless fixed_iters > 0).            */
int mpc_solve_batch_dev(mpc_handle* h, int32_t B, const double* d_x0, const double* d_p, const double* d_obst,
                        double* d_x_out, int32_t* d_status, int32_t* d_iters, double* d_kkt, void* stream);

/* The rest of what CasADi's `sol(...)` returns (`res['f']`, `res['g']`, `res['lam_g']`, `res['lam_x']`).
 * n_g = 1 + nx(N+1) + 9(N+1) rows in the order of mpc_set_bounds: row 0 the friction row, then the x_0 pin (nx rows), then the
 * defects x_{k+1} - x_k - dt f(x_k, u_k) (nx rows per k), then per stage k the three circle-pair distances, each three times in a row
 * (optimizer.py:395-403; the solver weights the copies by obst_mult).
 *
 * mpc_eval_nlp_batch: objective f [B] and all rows g [B, n_g] of the reference's NLP at ANY x [B, n_w] with parameters p [B, n_w]
 * and obstacle centres obst [B, 6] (NULL: the descriptor's).  g is the literal row: row 0 is sqrt((a_0^2 + v_0^2 tan(delta_0)/2.578)^2)
 * whatever "friction_lb" says; f is the reference's cost sum_{k<N} |x_k - xref_{k+1}|_Q^2 + |u_k|_R^2 (its terminal term is dead code).
 * Either output may be NULL.  Does not need mpc_set_bounds.                                                                         */
int mpc_eval_nlp_batch(mpc_handle* h, int32_t B, const double* x, const double* p, const double* obst, double* f, double* g);
int mpc_eval_nlp_batch_dev(mpc_handle* h, int32_t B, const double* d_x, const double* d_p, const double* d_obst,
                           double* d_f, double* d_g, void* stream);

/* mpc_solve_batch[_dev] plus f [B] and g [B, n_g] at the returned x, and the multipliers lam_g [B, n_g], lam_x [B, n_w] of the final
 * iterate; any of the four may be NULL, and with all four NULL the call IS mpc_solve_batch[_dev] (same kernels, same bits).
 * Multipliers follow CasADi: grad f + J_g' lam_g + lam_x = 0 at the solution; lam_x = z_U - z_L (an active lower bound negative, an
 * active upper bound positive, exactly 0 where a variable has no finite bound); lam_g by the same sign rule per row, equality rows either
 * sign; the three copies of a circle row carry equal multipliers that sum to that distance's multiplier.
 * Rows with status != 1 get NaN in lam_g and lam_x (a row that failed may carry its first attempt's x, which the last iterate does not
 * belong to); f and g are always evaluated at the returned x.  lam_g[0] is NaN where the friction row sits exactly on its kink
 * a_0^2 + v_0^2 tan(delta_0)/2.578 = 0 (not differentiable there).  Asking for a multiplier with fixed_iters > 0 -> MPC_ERR_INVALID.
 * The _dev form synchronises `stream` when any of the four is asked for.                                                            */
int mpc_solve_batch_ex(mpc_handle* h, int32_t B, const double* x0, const double* p, const double* obst,
                       double* x_out, int32_t* status, int32_t* iters, double* kkt,
                       double* f, double* g, double* lam_g, double* lam_x);
int mpc_solve_batch_dev_ex(mpc_handle* h, int32_t B, const double* d_x0, const double* d_p, const double* d_obst,
                           double* d_x_out, int32_t* d_status, int32_t* d_iters, double* d_kkt,
                           double* d_f, double* d_g, double* d_lam_g, double* d_lam_x, void* stream);

/* Obstacle centres per STAGE: an obstacle that moves over the horizon.  mpc_solve_batch_stages[_dev] takes the arguments of
 * mpc_solve_batch[_dev]_ex, mpc_eval_nlp_batch_stages[_dev] those of mpc_eval_nlp_batch[_dev], with one difference: obst is REQUIRED and is
 * [B, N+1, 6] -- row (b, k) holds the six circle centres (order of mpc_problem_desc::obstacle) that the nine circle rows of stage k of instance
 * b are measured against.  obst NULL -> MPC_ERR_INVALID.  The outputs x_out .. lam_x are NULL-able as in _ex and mean the same: f, g, lam_g, lam_x
 * belong to the NLP with the per-stage centres.  The solve runs the kernels of a solve with obst [B, 6] (second chance, chunks, every horizon,
 * nx 5 and 6): with all N+1 rows of an instance equal it returns the bits of mpc_solve_batch[_dev]_ex with that row.  A device buffer should
 * start on a 16-byte boundary (one that does not is read in 8-byte halves).  The first per-stage call of a handle grows its workspace by
 * 6 N rows per instance, once; a handle that never makes one keeps the workspace it had.
 * Derivatives of a per-stage solve are not provided: it takes no sensitivity snapshot and, like every solve, ends the life of an earlier one --
 * any mpc_sens_* call after it returns MPC_ERR_STATE.                                                                                     */
int mpc_solve_batch_stages(mpc_handle* h, int32_t B, const double* x0, const double* p, const double* obst,
                           double* x_out, int32_t* status, int32_t* iters, double* kkt,
                           double* f, double* g, double* lam_g, double* lam_x);
int mpc_solve_batch_stages_dev(mpc_handle* h, int32_t B, const double* d_x0, const double* d_p, const double* d_obst,
                               double* d_x_out, int32_t* d_status, int32_t* d_iters, double* d_kkt,
                               double* d_f, double* d_g, double* d_lam_g, double* d_lam_x, void* stream);
int mpc_eval_nlp_batch_stages(mpc_handle* h, int32_t B, const double* x, const double* p, const double* obst, double* f, double* g);
int mpc_eval_nlp_batch_stages_dev(mpc_handle* h, int32_t B, const double* d_x, const double* d_p, const double* d_obst,
                                  double* d_f, double* d_g, void* stream);

/* A radius per obstacle: mpc_solve_batch_sized[_dev] takes the arguments of mpc_solve_batch_stages[_dev] plus rsum [B, N+1, 3] directly behind
 * obst.  rsum[b, k, j] is the lower bound of the three copies of circle row j of stage k of instance b -- ego circle j against slot j of
 * obst[b, k] -- in place of the one lower bound of mpc_set_bounds; it is relaxed as that one is.  The upper side of the circle rows and every
 * other bound stay the handle's: a handle whose circle rows have a finite upper bound or no lower bound -> MPC_ERR_BOUNDS with a message.  obst
 * or rsum NULL -> MPC_ERR_INVALID.  The host form also refuses an entry of rsum that is not finite or is negative; the device form does not
 * read the buffer back: a non-finite entry ends that instance with status -6 and touches no other.  x_out .. lam_x mean what they mean in
 * _stages; g is the literal distance, so f and g are mpc_eval_nlp_batch_stages' bits at the returned x, and lam_g follows the same sign rule.
 * Every level of the second chance scales each row's bound by the level's fraction; the last level is the problem itself.  fixed_iters, chunks,
 * nx 5 / 6 and every horizon behave as in _stages.  With every entry of rsum equal to the circle lower bound given to mpc_set_bounds the call
 * returns the bits of mpc_solve_batch_stages[_dev].  The first sized call of a handle grows its workspace once (10 rows per stage and instance
 * in place of 6).  No sensitivity snapshot, as for _stages: any mpc_sens_* call after it returns MPC_ERR_STATE.                              */
int mpc_solve_batch_sized(mpc_handle* h, int32_t B, const double* x0, const double* p, const double* obst, const double* rsum,
                          double* x_out, int32_t* status, int32_t* iters, double* kkt,
                          double* f, double* g, double* lam_g, double* lam_x);
int mpc_solve_batch_sized_dev(mpc_handle* h, int32_t B, const double* d_x0, const double* d_p, const double* d_obst, const double* d_rsum,
                              double* d_x_out, int32_t* d_status, int32_t* d_iters, double* d_kkt,
                              double* d_f, double* d_g, double* d_lam_g, double* d_lam_x, void* stream);

/* Parametric sensitivities of the returned optimum (sIPOPT's step).  p = [U_ref (N nu) | X_ref ((N+1) nx)], n_p = n_w.
 * mpc_solve_batch[_dev]_ex plus: lam_p [B, n_p] (NULL: not computed), CasADi's d/dp [f + lam_g' g + lam_x' x] at the returned x (X_ref column 0
 * -lam_g[pin rows], column k+1 -2 Q (x_k - xref_{k+1}), U_ref 0); n_dir >= 0 forward seeds dp [B, n_dir, n_p] -> dw [B, n_dir, n_w] = (dw/dp) dp
 * from the KKT matrix of the final barrier iterate, without regularisation.  Keeps the final iterates for mpc_sens_adjoint.  x_out .. lam_x are
 * bit for bit those of mpc_solve_batch[_dev]_ex; with lam_p NULL and n_dir 0 nothing more is written.  Rows with status != 1 get NaN in lam_p
 * and dw, and so do rows whose final KKT matrix has the wrong inertia (a Riccati pivot <= 0) or that sit on the friction kink (lam_g[0] NaN).
 * fixed_iters > 0 -> MPC_ERR_INVALID.  The derivative with respect to the obstacle centres: mpc_sens_obst below; with respect to the cost
 * weights: mpc_sens_weights below; with respect to the bounds and the circle radius: mpc_sens_bounds below.  A derivative with respect to x0
 * (the initial guess) is not provided: at an isolated optimum it is zero.
 * The _dev form synchronises `stream`.                                                                                                     */
int mpc_solve_batch_sens(mpc_handle* h, int32_t B, const double* x0, const double* p, const double* obst, double* x_out,
                         int32_t* status, int32_t* iters, double* kkt, double* f, double* g, double* lam_g, double* lam_x,
                         double* lam_p, int32_t n_dir, const double* dp, double* dw);
int mpc_solve_batch_sens_dev(mpc_handle* h, int32_t B, const double* d_x0, const double* d_p, const double* d_obst, double* d_x_out,
                             int32_t* d_status, int32_t* d_iters, double* d_kkt, double* d_f, double* d_g, double* d_lam_g, double* d_lam_x,
                             double* d_lam_p, int32_t n_dir, const double* d_dp, double* d_dw, void* stream);
/* Reverse mode on the last mpc_solve_batch_sens[_dev] of this handle: seed_w [B, n_w] -> grad_p [B, n_p] = (dw/dp)' seed_w (NaN rows as above).
 * Any solve of the handle after it (plain, _ex, closed loop, FORCES), or a different B -> MPC_ERR_STATE.  The _dev form is enqueued on
 * `stream` and does not synchronise it: it reads the handle's snapshot and writes the handle's factor storage when it runs, so until it has
 * completed the caller must not start another mpc_solve_batch_sens[_dev] or mpc_sens_adjoint[_dev] of this handle on a different stream
 * (on the same stream, stream order takes care of it; the handle is not for concurrent use from several streams, as for every entry).         */
int mpc_sens_adjoint(mpc_handle* h, int32_t B, const double* seed_w, double* grad_p);
int mpc_sens_adjoint_dev(mpc_handle* h, int32_t B, const double* d_seed_w, double* d_grad_p, void* stream);
/* The derivative of the optimum with respect to the six obstacle circle centres o [B, 6] (the `obst` rows of the solve, or the descriptor's
 * centres where it had none; order of mpc_problem_desc::obstacle), on the snapshot of the last mpc_solve_batch_sens[_dev] of this handle -- a
 * solve with lam_p NULL and n_dir 0 is enough to take it.  Any part may be left out:
 *   n_dir > 0 forward directions dobst [B, n_dir, 6] -> dw [B, n_dir, n_w] = (dw/do) dobst;
 *   one adjoint seed seed_w [B, n_w] -> grad_obst [B, 6] = (dw/do)' seed_w (both or neither);
 *   lam_obst [B, 6] = d/do [f + lam_g' g] at the returned x, which is the derivative of the optimal objective (envelope theorem).
 * NaN rows, MPC_ERR_STATE and the stream rule of the _dev form are those of mpc_sens_adjoint; n_dir < 0, n_dir > 0 without dobst and dw, or
 * only one of seed_w / grad_obst -> MPC_ERR_INVALID.  It shares the factor storage of mpc_sens_adjoint.                                    */
int mpc_sens_obst(mpc_handle* h, int32_t B, int32_t n_dir, const double* dobst, double* dw, const double* seed_w, double* grad_obst,
                  double* lam_obst);
int mpc_sens_obst_dev(mpc_handle* h, int32_t B, int32_t n_dir, const double* d_dobst, double* d_dw, const double* d_seed_w, double* d_grad_obst,
                      double* d_lam_obst, void* stream);
/* The derivative of the optimum with respect to the seven cost weights wt = [Q_0 .. Q_4 | R_0, R_1] (n_wt = 7 for nx 5 and 6 alike; the
 * handle's current ones, see mpc_set_weights), on the snapshot of the last mpc_solve_batch_sens[_dev] of this handle -- a solve with lam_p NULL
 * and n_dir 0 is enough to take it.  p [B, n_w]: the p rows of that solve; required, because the snapshot does not hold X_ref, and NOT checked
 * against the solve (another p gives the derivative of nothing).  Any part may be left out:
 *   n_dir > 0 forward directions dwt [B, n_dir, 7] -> dw [B, n_dir, n_w] = (dw/dwt) dwt;
 *   one adjoint seed seed_w [B, n_w] -> grad_wt [B, 7] = (dw/dwt)' seed_w (both or neither);
 *   lam_wt [B, 7] = d/dwt [f + lam_g' g] at the returned x = [sum_{k<N} (x_k - xref_{k+1})_i^2 | sum_{k<N} u_k[j]^2], which is the derivative
 *   of the optimal objective (envelope theorem).
 * The weights are shared by the batch; the rows of grad_wt / lam_wt are per instance, to be summed by the caller.  The objective scaling of
 * the solve is held fixed.  NaN rows, MPC_ERR_STATE (also after mpc_set_weights) and the stream rule of the _dev form
 * are those of mpc_sens_adjoint; p NULL, n_dir < 0, n_dir > 0 without dwt and dw, or only one of seed_w / grad_wt -> MPC_ERR_INVALID.  It
 * shares the factor storage of mpc_sens_adjoint.                                                                                            */
int mpc_sens_weights(mpc_handle* h, int32_t B, const double* p, int32_t n_dir, const double* dwt, double* dw, const double* seed_w, double* grad_wt,
                     double* lam_wt);
int mpc_sens_weights_dev(mpc_handle* h, int32_t B, const double* d_p, int32_t n_dir, const double* d_dwt, double* d_dw, const double* d_seed_w,
                         double* d_grad_wt, double* d_lam_wt, void* stream);
/* The derivative of the optimum with respect to the bounds and the circle radius, on the snapshot of the last mpc_solve_batch_sens[_dev] of
 * this handle -- a solve with lam_p NULL and n_dir 0 is enough to take it.  The bound vector is bv = [lbx (n_w) | ubx (n_w) | fl, fu, ol, ou],
 * n_b = 2 n_w + 4: the arrays of mpc_set_bounds, then lbg[0], ubg[0] of the friction row and the pair [lo, hi] shared by the 9 (N + 1) circle
 * rows -- ol is the radius sum.  The equality rows have no entry.  Any part may be left out:
 *   n_dir > 0 forward directions dbv [B, n_dir, n_b] -> dw [B, n_dir, n_w] = (dw/dbv) dbv;
 *   one adjoint seed seed_w [B, n_w] -> grad_bv [B, n_b] = (dw/dbv)' seed_w (both or neither);
 *   lam_bv [B, n_b] = d f* / d bv, the derivative of the optimal objective (envelope theorem), in CasADi's sign and unscaled: entries of lbx, fl,
 *   ol are >= 0, entries of ubx, fu, ou <= 0, and lam_bv[lbx_i] + lam_bv[ubx_i] = -lam_x[i], lam_bv[fl] + lam_bv[fu] = -lam_g[0],
 *   lam_bv[ol] + lam_bv[ou] = -(sum of lam_g over the circle rows).
 * The bounds are shared by the batch; the rows of grad_bv / lam_bv are per instance, to be summed by the caller.  An entry whose bound is absent
 * (+-inf), or that the solve did not impose (fl under the default friction_lb = nlp; the caller's bound of a_0 on a side where the presolved
 * friction row is tighter: that side moves with fu), has derivative 0 in all three outputs, and its dbv entry is not read.  NaN rows,
 * MPC_ERR_STATE (also after mpc_set_bounds / mpc_set_weights) and the stream rule of the _dev form are those of mpc_sens_adjoint; n_dir < 0,
 * n_dir > 0 without dbv and dw, or only one of seed_w / grad_bv -> MPC_ERR_INVALID; a call that asks for nothing returns MPC_OK at once.  It
 * shares the factor storage of mpc_sens_adjoint.                                                                                            */
int mpc_sens_bounds(mpc_handle* h, int32_t B, int32_t n_dir, const double* dbv, double* dw, const double* seed_w, double* grad_bv, double* lam_bv);
int mpc_sens_bounds_dev(mpc_handle* h, int32_t B, int32_t n_dir, const double* d_dbv, double* d_dw, const double* d_seed_w, double* d_grad_bv,
                        double* d_lam_bv, void* stream);

/* Batched plant step on the device path: x_next = x + dt f(x,u) (integrator 0 = forward Euler,
 * optimizer.py:649-650) or one RK4 step (integrator 1, optimizer.py:97-98).  x: [B, nx], u: [B, 2] host. */
int mpc_plant_step(mpc_handle* h, int32_t B, int32_t integrator, const double* x, const double* u, double* x_next);
/* same with device pointers; the kernel is enqueued on `stream`, nothing is synchronised or allocated */
int mpc_plant_step_dev(mpc_handle* h, int32_t B, int32_t integrator, const double* d_x, const double* d_u, double* d_x_next, void* stream);

/* Closed-loop driver (scope row f1): the loop body of CasadiOptimizer.optimize (optimizer.py:596-631) run for B egos
 * without host round trips between the solves -- per step: mpc_solve_batch_dev, first control, forward-Euler plant
 * step (shift_movement, optimizer.py:645-655), shifted warm start in the layouts the reference produces
 * (optimizer.py:602), next reference window incl. the frozen tail (desired_command_and_trajectory, :657-702).
 * init_state [B,5] = (x, y, 0, v, psi) (optimizer.py:575); path [B,Lp,2], orient [B,Lp]: resampled path
 * points and orientation of every ego, Lp >= L = iter_length >= N; vdes [B].  Outputs: traj [B,L,5] (row i = state
 * before step i: what optimize() returns as its first array), ctrl [B,L,2] (second array), step_status [B,L] or NULL
 * (solver status of every step; the reference ignores it).  No noise (`noised: False`).                           */
int mpc_closed_loop_batch(mpc_handle* h, int32_t B, int32_t L, int32_t Lp, const double* init_state, const double* path,
                          const double* orient, const double* vdes, double* traj, double* ctrl, int32_t* step_status);
/* The same loop with the reference's `noised: True` behaviour, reproducibly: N(0, sigma) samples from a counter-based generator
 * (Philox4x32-10 + Box-Muller, keyed by seed and (instance, step, sample); csrc/mpc_closed_loop.h, mirrored by noise.py).
 * noise_mode 0: none; 1: CasadiOptimizer (optimizer.py:611-617) -- noise on the whole predicted input sequence, the noised first
 * column is applied and the noised sequence is shifted into the next warm start; 2: ForcesproOptimizer (optimizer.py:348-354) --
 * noise on the applied input only.  sigma: 0.1 lane following, 0.05 collision avoidance (the reference's values).
 * nx = 5 or 6 (the progress state of nx = 6 starts at 0 and is not reported: traj stays [B,L,5]).
 * The device-pointer form enqueues the WHOLE loop without a host synchronisation per step when the solves run in the persistent
 * pipeline launch; an abandoned launch or an instance that needs the second chance is noticed once, at the end, and the loop is
 * then replayed step by step (mpc_last_loop_replayed tells).  Option "loop_async" = "0" forces the step-by-step form.          */
int mpc_closed_loop_batch_ex(mpc_handle* h, int32_t B, int32_t L, int32_t Lp, const double* init_state, const double* path,
                             const double* orient, const double* vdes, int32_t noise_mode, double sigma, uint64_t seed,
                             double* traj, double* ctrl, int32_t* step_status);
int mpc_closed_loop_batch_dev_ex(mpc_handle* h, int32_t B, int32_t L, int32_t Lp, const double* d_init_state, const double* d_path,
                                 const double* d_orient, const double* d_vdes, int32_t noise_mode, double sigma, uint64_t seed,
                                 double* d_traj, double* d_ctrl, int32_t* d_step_status, void* stream);
int mpc_last_loop_replayed(const mpc_handle* h);
/* The same loop past per-ego obstacles that move.  obst_track [B, Lt, 3] = (x, y, heading) of ego b's obstacle: Lt = 1, it stands still; Lt >= L,
 * row i is its pose at loop step i (anything else, or a NULL track: MPC_ERR_INVALID with a message).  The solve of step i sees the obstacle where
 * it is at step i, FROZEN over that solve's horizon -- the reference's NLP has one static obstacle per solve (optimizer.py:60-64, 395-403); this
 * is that NLP, re-posed every step (its circle centres: the pose's centre, then +- obst_offset along the heading, compute_centers_of_
 * approximation_circles, configuration.py:69-93 -- obst_offset = disc_distance / 4 of the obstacle rectangle).  The obstacle's SIZE stays the
 * handle's: the radius sits in the lower bound of the circle rows given to mpc_set_bounds, one obstacle size per handle.
 * A frozen obstacle gives no guarantee between steps: the plan of step i-1 kept its distance from the obstacle at step i-1.  A caller who needs a
 * margin inflates the radius by the obstacle's travel per step, or lets every stage see the obstacle where it will be: mpc_closed_loop_batch_pred.
 * clearance [B, L] or NULL: clearance[b, i] = min over the three constrained circle pairs (ego circle j, obstacle circle j) of distance - r_sum for
 * the state BEFORE step i (traj[b, i]) against the obstacle at step i; r_sum = the lower bound of the handle's circle rows.
 * Noise modes, nx = 5 / 6, step_status, mpc_last_loop_replayed and option "loop_async" as in mpc_closed_loop_batch_ex.                     */
int mpc_closed_loop_batch_obst(mpc_handle* h, int32_t B, int32_t L, int32_t Lp, const double* init_state, const double* path,
                               const double* orient, const double* vdes, int32_t Lt, const double* obst_track, double obst_offset,
                               int32_t noise_mode, double sigma, uint64_t seed, double* traj, double* ctrl, int32_t* step_status,
                               double* clearance);
int mpc_closed_loop_batch_obst_dev(mpc_handle* h, int32_t B, int32_t L, int32_t Lp, const double* d_init_state, const double* d_path,
                                   const double* d_orient, const double* d_vdes, int32_t Lt, const double* d_obst_track, double obst_offset,
                                   int32_t noise_mode, double sigma, uint64_t seed, double* d_traj, double* d_ctrl, int32_t* d_step_status,
                                   double* d_clearance, void* stream);
/* The loop past per-ego obstacles with the obstacle PREDICTED over each solve's horizon.  The arguments of mpc_closed_loop_batch_obst[_dev] plus
 * `predict`: 0 is that loop, bit for bit; 1: stage k of the solve of step i sees track row min(i + k, Lt - 1) -- stage 0 is pinned to the measured
 * state at time i and stage k's state is the state at time i + k, so every stage keeps its distance from where the obstacle will be then; rows
 * past the track repeat its last pose (Lt = 1: the obstacle stands still, predict changes nothing but the kernels).  Each solve is an
 * mpc_solve_batch_stages_dev.  With noise_mode 0 the plant is the model's own forward-Euler step: the state before step i is stage 1 of the solve
 * of step i - 1, which held it clear of track row i -- clearance[b, i] >= 0 up to the solver's tolerance wherever that solve converged, the
 * guarantee the frozen loop lacks.  clearance keeps its meaning (the state before step i against the pose at step i); noise modes, step_status,
 * option "loop_async" (the whole loop enqueued without a host synchronisation) and mpc_last_loop_replayed as in mpc_closed_loop_batch_obst.
 * predict outside {0, 1}, or predict 1 with Lt <= 0 or a NULL track -> MPC_ERR_INVALID.  mpc_closed_loop_batch_lin takes no `predict`.      */
int mpc_closed_loop_batch_pred(mpc_handle* h, int32_t B, int32_t L, int32_t Lp, const double* init_state, const double* path,
                               const double* orient, const double* vdes, int32_t Lt, const double* obst_track, double obst_offset,
                               int32_t predict, int32_t noise_mode, double sigma, uint64_t seed, double* traj, double* ctrl,
                               int32_t* step_status, double* clearance);
int mpc_closed_loop_batch_pred_dev(mpc_handle* h, int32_t B, int32_t L, int32_t Lp, const double* d_init_state, const double* d_path,
                                   const double* d_orient, const double* d_vdes, int32_t Lt, const double* d_obst_track, double obst_offset,
                                   int32_t predict, int32_t noise_mode, double sigma, uint64_t seed, double* d_traj, double* d_ctrl,
                                   int32_t* d_step_status, double* d_clearance, void* stream);
/* The loop through TRAFFIC: M >= 1 obstacles, and every stage of every solve avoids the one nearest to it.  The arguments of
 * mpc_closed_loop_batch_pred[_dev] with (Lt, obst_track, obst_offset, predict) replaced by (M, Lt, per_ego, tracks, offsets, pairing).
 * per_ego 0: tracks [M, Lt, 3], offsets [M], shared by all egos (one scene, many egos); per_ego 1: tracks [B, M, Lt, 3], offsets [B, M].  Lt = 1 or
 * Lt >= L as above.  A pose whose x is not finite (NaN) means that the obstacle is ABSENT at that row: CommonRoad obstacles live for part of a scenario.
 * Before the solve of step i, stage k of ego b gets the circle centres of an obstacle at track row r = min(i + k, Lt - 1), picked against the
 * predicted ego pose of that stage -- at step 0 the measured state, from step 1 on stage k of the shifted last plan (the solve's warm start):
 *   pairing 0  (the reference's pairs, on one obstacle): the present obstacle m with the smallest min_j |E_j - O_{m,j}| (ego circle j against
 *              obstacle circle j; lowest m on a tie) gives all three centres;  chosen[b, i, k, 0..2] = m
 *   pairing 1  (each ego circle against its nearest circle): slot j is the circle O_{m,c} nearest to ego circle j over all present m and c (ties:
 *              lowest m, then lowest c), so front-against-rear contacts count too;  chosen[b, i, k, j] = m
 * No obstacle present at r: the descriptor's centres, chosen = -1.  This is the standard nearest-obstacle formulation, not an exact multi-obstacle
 * NLP: two obstacles equally close to one ego circle at one stage constrain it only once.  The solves are mpc_solve_batch_stages_dev's, unchanged;
 * with M = 1 and pairing 0 traj, ctrl and step_status are bit for bit those of mpc_closed_loop_batch_pred with predict 1 on that track.  One radius
 * per handle, as in every loop but mpc_closed_loop_batch_traffic_sized: the lower bound of the circle rows holds for all obstacles.
 * clearance [B, L] or NULL: clearance[b, i] = min over the obstacles present at row min(i, Lt - 1) and over ALL nine circle pairs of distance - r_sum
 * for the state before step i, +inf when none is present; nearest [B, L] (int32) or NULL: the obstacle that attains it, or -1; chosen
 * [B, L, N+1, 3] (int32) or NULL.  MPC_ERR_INVALID with a message: M < 1; Lt neither 1 nor >= L; NULL tracks or offsets; an offset that is not
 * finite (the device-pointer form copies the offsets back once, before it enqueues anything); pairing or per_ego outside {0, 1}.  Noise modes,
 * step_status, option "loop_async" and mpc_last_loop_replayed as in mpc_closed_loop_batch_obst; like every loop it ends the life of the
 * sensitivity snapshot.                                                                                                                          */
int mpc_closed_loop_batch_traffic(mpc_handle* h, int32_t B, int32_t L, int32_t Lp, const double* init_state, const double* path,
                                  const double* orient, const double* vdes, int32_t M, int32_t Lt, int32_t per_ego, const double* tracks,
                                  const double* offsets, int32_t pairing, int32_t noise_mode, double sigma, uint64_t seed, double* traj,
                                  double* ctrl, int32_t* step_status, double* clearance, int32_t* nearest, int32_t* chosen);
int mpc_closed_loop_batch_traffic_dev(mpc_handle* h, int32_t B, int32_t L, int32_t Lp, const double* d_init_state, const double* d_path,
                                      const double* d_orient, const double* d_vdes, int32_t M, int32_t Lt, int32_t per_ego,
                                      const double* d_tracks, const double* d_offsets, int32_t pairing, int32_t noise_mode, double sigma,
                                      uint64_t seed, double* d_traj, double* d_ctrl, int32_t* d_step_status, double* d_clearance,
                                      int32_t* d_nearest, int32_t* d_chosen, void* stream);
/* Traffic of mixed sizes: mpc_closed_loop_batch_traffic_sized[_dev] takes the arguments of mpc_closed_loop_batch_traffic[_dev] plus rsums behind
 * offsets, in the same shape ([M], per_ego: [B, M]): rsums[m] is the radius sum of ego and obstacle m, checked as the offsets are -- finite -- and
 * >= 0 (MPC_ERR_INVALID with a message; NULL likewise).  The selection is by CLEARANCE, not by distance: with delta_m = rsums[m] - r_sum (the
 * handle's circle lower bound) pairing 0 compares min_j |E_j - O_{m,j}| - delta_m, pairing 1 |E_j - O_{m,c}| - delta_m; ties as above.  The slot's
 * row of the next solve gets the winner's centres and the winner's rsums[m]; no obstacle present: the descriptor's centres, the handle's radius,
 * chosen = -1.  Every solve is an mpc_solve_batch_sized_dev (its refusal of the handle's bound structure: MPC_ERR_BOUNDS).  clearance[b, i] = min
 * over the present obstacles and all nine pairs of distance - rsums[m]; nearest the obstacle that attains it.  Noise modes, "loop_async", replay
 * and step_status as in the traffic loop.  With every rsums[m] equal to the handle's bound traj, ctrl, step_status, clearance, nearest and chosen
 * are the bits of mpc_closed_loop_batch_traffic.                                                                                                  */
int mpc_closed_loop_batch_traffic_sized(mpc_handle* h, int32_t B, int32_t L, int32_t Lp, const double* init_state, const double* path,
                                        const double* orient, const double* vdes, int32_t M, int32_t Lt, int32_t per_ego, const double* tracks,
                                        const double* offsets, const double* rsums, int32_t pairing, int32_t noise_mode, double sigma,
                                        uint64_t seed, double* traj, double* ctrl, int32_t* step_status, double* clearance, int32_t* nearest,
                                        int32_t* chosen);
int mpc_closed_loop_batch_traffic_sized_dev(mpc_handle* h, int32_t B, int32_t L, int32_t Lp, const double* d_init_state, const double* d_path,
                                            const double* d_orient, const double* d_vdes, int32_t M, int32_t Lt, int32_t per_ego,
                                            const double* d_tracks, const double* d_offsets, const double* d_rsums, int32_t pairing,
                                            int32_t noise_mode, double sigma, uint64_t seed, double* d_traj, double* d_ctrl,
                                            int32_t* d_step_status, double* d_clearance, int32_t* d_nearest, int32_t* d_chosen, void* stream);
/* The loop stepped FROM OUTSIDE: a session.  Every loop above is closed over its own model -- the plant is the NLP's forward-Euler step, the obstacles
 * come from tracks that already hold the future.  A simulator or a vehicle owns the plant and reports a measured state every step; perception reports
 * where the obstacles are NOW and how fast they move.  One session per handle; it owns device buffers of its own (the rows of its solves, the loop's work
 * buffers, the record, copies of path / orient / vdes / offsets), released by mpc_session_end and mpc_destroy, so between two steps every other entry
 * point of the handle may run -- solves, sens calls, other loops, mpc_set_weights, mpc_set_bounds: the next step uses the new weights and bounds.
 *   mpc_session_begin   the arguments of mpc_closed_loop_batch_traffic that do not change over a loop; L >= N still fixes the frozen tail of the reference
 *                       window, Lp >= L.  M = 0: lane following (plain solves, offsets NULL); M > 0: offsets [M] (per_ego: [B, M]), finite.  Everything is
 *                       copied and the set-up has run when the call returns (both forms synchronise).  The record is filled with NaN / 0.
 *   mpc_session_step    step i = mpc_session_steps_done(h), in stream order:
 *       ingest      measured [B, 5] or NULL (the model's own Euler prediction: the loops above; required NULL at step 0, where init_state is the
 *                   measurement) replaces the first five entries of the state and of row 0 of X_ref; a row whose x is not finite is a DROPPED
 *                   measurement, that ego keeps the prediction; with nx = 6 the progress state stays the model's; the warm start stays the shifted last plan
 *       obstacles   (M > 0) obs [M, 5] (per_ego: [B, M, 5]) = (x, y, heading, vx, vy) now; x not finite: absent; a velocity that is not finite counts
 *                   as 0.  Stage k sees obstacle m at (x + (k dt) vx, y + (k dt) vy, heading), constant-velocity prediction, and the selection is
 *                   mpc_closed_loop_batch_traffic's (both pairings, ties, the descriptor's centres when nothing is present; the ego pose is the state at
 *                   step 0, stage k of the warm start afterwards).  clearance [B], nearest [B], chosen [B, N+1, 3], any of them NULL: this step's, as
 *                   defined there, against the observed poses (M = 0: they must be NULL)
 *       solve       mpc_solve_batch_dev (M > 0: mpc_solve_batch_stages_dev) on the session's rows, second chance included, synchronous
 *       advance     the step is recorded (traj[b, i] = the state the solve started from, ctrl, step_status), the model's Euler step is the prediction
 *                   for step i + 1, the next warm start and reference window are written; no noise
 *       emit        u [B, 2] (required) the applied control, plan [B, n_w] the solution, status [B]; complete when the stream is synchronised
 *   mpc_session_record  copies out what has been recorded so far (rows of steps not yet taken: NaN / 0); any argument may be NULL
 *   mpc_session_steps_done  the index of the next step, -1 when no session is open
 * With measured NULL at every step the record is bit for bit that of the loop it opens (M = 0: mpc_closed_loop_batch_ex; standing obstacles, vx = vy = 0:
 * mpc_closed_loop_batch_traffic with Lt = 1, clearance / nearest / chosen included).  A step ends the life of a sensitivity snapshot, as any solve does.
 * MPC_ERR_STATE: step / record / end without an open session, begin while one is open, step L + 1, bounds not set.  MPC_ERR_INVALID: M < 0; M > 0 with
 * NULL or non-finite offsets; obs NULL with M > 0; measured at step 0; u NULL; pairing or per_ego outside {0, 1}; the shape rules of the loops.
 *
 * Two things the caller may know better than the session, each an entry point of its own; the four above keep their arguments and their bits.
 *   mpc_session_begin_sized   a radius per obstacle: the arguments of mpc_session_begin plus rsums behind offsets, in the same shape ([M], per_ego:
 *                       [B, M]); rsums[m] is the radius sum of ego and obstacle m, copied as the offsets are and checked once, here, as
 *                       mpc_closed_loop_batch_traffic_sized checks it: finite and >= 0 (the device form copies it back once, next to the offsets).
 *                       Every step of such a session is a sized solve (mpc_solve_batch_sized_dev's, second chance included) and the selection is by
 *                       CLEARANCE, as in mpc_closed_loop_batch_traffic_sized: a slot's row carries the winner's centres and the winner's rsums[m];
 *                       nothing present: the descriptor's centres with the handle's radius, chosen = -1.  clearance is the smallest distance -
 *                       rsums[m], nearest the obstacle that attains it.  With every rsums[m] equal to the handle's bound every output of every step has
 *                       the bits of a plain session; with standing obstacles and measured NULL the record, clearance, nearest and chosen are those of
 *                       mpc_closed_loop_batch_traffic_sized with Lt = 1.  MPC_ERR_INVALID with "rsums" in the message: M < 1, rsums NULL, an entry that
 *                       is not finite or negative.  MPC_ERR_BOUNDS: the circle rows of the handle have no lower bound or a finite upper one -- checked
 *                       here, and again at every step (mpc_set_bounds may run between two steps): that step returns the code, is not counted, and the
 *                       session stays open.
 *   mpc_session_step_pred     poses predicted by the caller: the arguments of mpc_session_step with obs replaced by pred [M, N+1, 3] (per_ego:
 *                       [B, M, N+1, 3]) = (x, y, heading) of obstacle m as stage k is to see it, its pose k dt from now -- a trajectory from a
 *                       prediction module instead of a velocity: a vehicle that turns, cuts in or brakes to a stop.  The rows are taken as they stand.
 *                       An x that is not finite: absent AT THAT STAGE, so an obstacle may enter or leave within the horizon.  Row 0 is the pose now:
 *                       clearance and nearest are taken against it.  Everything else -- ingest, the ego pose of the selection, both pairings, ties,
 *                       solve, advance, emit, the record -- is mpc_session_step's; it works in a plain and in a sized session, and the two step forms
 *                       may alternate freely within one.  With measured NULL and pred[m, k] = tracks[m, min(i + k, Lt - 1)] at step i the record,
 *                       clearance, nearest and chosen are bit for bit those of mpc_closed_loop_batch_traffic (a sized session:
 *                       mpc_closed_loop_batch_traffic_sized) on those tracks.  The device form reads d_pred in stream order and copies nothing back.
 *                       MPC_ERR_INVALID: a session with M = 0; pred NULL; u NULL; measured at step 0.  MPC_ERR_STATE as mpc_session_step.                 */
int mpc_session_begin(mpc_handle* h, int32_t B, int32_t L, int32_t Lp, const double* init_state, const double* path, const double* orient,
                      const double* vdes, int32_t M, int32_t per_ego, const double* offsets, int32_t pairing);
int mpc_session_begin_dev(mpc_handle* h, int32_t B, int32_t L, int32_t Lp, const double* d_init_state, const double* d_path, const double* d_orient,
                          const double* d_vdes, int32_t M, int32_t per_ego, const double* d_offsets, int32_t pairing, void* stream);
int mpc_session_step(mpc_handle* h, const double* measured, const double* obs, double* u, double* plan, int32_t* status, double* clearance,
                     int32_t* nearest, int32_t* chosen);
int mpc_session_step_dev(mpc_handle* h, const double* d_measured, const double* d_obs, double* d_u, double* d_plan, int32_t* d_status,
                         double* d_clearance, int32_t* d_nearest, int32_t* d_chosen, void* stream);
int mpc_session_begin_sized(mpc_handle* h, int32_t B, int32_t L, int32_t Lp, const double* init_state, const double* path, const double* orient,
                            const double* vdes, int32_t M, int32_t per_ego, const double* offsets, const double* rsums, int32_t pairing);
int mpc_session_begin_sized_dev(mpc_handle* h, int32_t B, int32_t L, int32_t Lp, const double* d_init_state, const double* d_path,
                                const double* d_orient, const double* d_vdes, int32_t M, int32_t per_ego, const double* d_offsets,
                                const double* d_rsums, int32_t pairing, void* stream);
int mpc_session_step_pred(mpc_handle* h, const double* measured, const double* pred, double* u, double* plan, int32_t* status, double* clearance,
                          int32_t* nearest, int32_t* chosen);
int mpc_session_step_pred_dev(mpc_handle* h, const double* d_measured, const double* d_pred, double* d_u, double* d_plan, int32_t* d_status,
                              double* d_clearance, int32_t* d_nearest, int32_t* d_chosen, void* stream);
int mpc_session_record(mpc_handle* h, double* traj, double* ctrl, int32_t* step_status);
int mpc_session_record_dev(mpc_handle* h, double* d_traj, double* d_ctrl, int32_t* d_step_status, void* stream);
int mpc_session_steps_done(const mpc_handle* h);
int mpc_session_end(mpc_handle* h);
/* The same loop as a chain of optima, linearised: besides traj / ctrl / step_status / clearance, the per-step feedback gains of the first
 * control of every solve,
 *   kgain [B,L,2,5] = d u*_0 / d s_i  (s_i = traj[b,i], the measured state)      wgain [B,L,2,7] = d u*_0 / d wt  (wt = [Q_0..Q_4 | R_0, R_1])
 *   ogain [B,L,2,3] = d u*_0 / d pose of the obstacle at step i (x, y, heading; through the six circle centres)
 * each two adjoint solves per step on the snapshot of that step's solve (mpc_solve_batch_sens' math).  Any gain may be NULL; with all three NULL
 * the call is the loop it wraps.  Lt = 0 with a NULL obst_track: the plain loop without per-ego obstacles -- ogain and clearance must then be
 * NULL (MPC_ERR_INVALID).  Otherwise the arguments of mpc_closed_loop_batch_obst.  With a gain asked for the loop runs step by step (every solve
 * synchronises); traj, ctrl and step_status are bit for bit those of the step-by-step loop (option "loop_async" = "0") on the same handle.
 * fixed_iters > 0 -> MPC_ERR_INVALID.  A step whose status is not 1, or whose factor fails (friction kink, wrong inertia: as
 * mpc_solve_batch_sens), gets NaN gains.  Like every loop it ends the life of the sensitivity snapshot (mpc_sens_* after it -> MPC_ERR_STATE).
 * The warm start, the reference window and the noise carry no derivative; vdes and the path are not differentiated.                      */
int mpc_closed_loop_batch_lin(mpc_handle* h, int32_t B, int32_t L, int32_t Lp, const double* init_state, const double* path,
                              const double* orient, const double* vdes, int32_t Lt, const double* obst_track, double obst_offset,
                              int32_t noise_mode, double sigma, uint64_t seed, double* traj, double* ctrl, int32_t* step_status,
                              double* clearance, double* kgain, double* wgain, double* ogain);
int mpc_closed_loop_batch_lin_dev(mpc_handle* h, int32_t B, int32_t L, int32_t Lp, const double* d_init_state, const double* d_path,
                                  const double* d_orient, const double* d_vdes, int32_t Lt, const double* d_obst_track, double obst_offset,
                                  int32_t noise_mode, double sigma, uint64_t seed, double* d_traj, double* d_ctrl, int32_t* d_step_status,
                                  double* d_clearance, double* d_kgain, double* d_wgain, double* d_ogain, void* stream);
/* Forward sweep over a recorded loop, n_dir directions per ego, no solve:  ds_0 = dinit;  du_i = K_i ds_i + W_i dwt + O_i dtrack[min(i, Lt-1)];
 * dtraj[i] = ds_i, dctrl[i] = du_i;  ds_{i+1} = ds_i + dt (F_x ds_i + F_u du_i), the plant Jacobians at traj[i] (the plant is linear in u: ctrl
 * is accepted for symmetry and not read, it may be NULL).  dinit [B,n_dir,5], dwt [B,n_dir,7], dtrack [B,n_dir,Lt,3]: NULL = zero; dtrack needs
 * ogain, dwt needs wgain (MPC_ERR_INVALID).  A NULL gain is zero.  dtraj [B,n_dir,L,5], dctrl [B,n_dir,L,2]: either may be NULL.  NaN gains of
 * step i make dctrl NaN from row i on, dtraj in the steering angle and the velocity at row i+1 and in every state from row i+2 on.  Stateless: reads its arguments and the handle's dt and wheelbase, may follow
 * any call; the _dev form enqueues on `stream` and does not synchronise.                                                                  */
int mpc_loop_tangent(mpc_handle* h, int32_t B, int32_t L, int32_t n_dir, const double* traj, const double* ctrl, const double* kgain,
                     const double* wgain, const double* ogain, int32_t Lt, const double* dinit, const double* dwt, const double* dtrack,
                     double* dtraj, double* dctrl);
int mpc_loop_tangent_dev(mpc_handle* h, int32_t B, int32_t L, int32_t n_dir, const double* d_traj, const double* d_ctrl, const double* d_kgain,
                         const double* d_wgain, const double* d_ogain, int32_t Lt, const double* d_dinit, const double* d_dwt,
                         const double* d_dtrack, double* d_dtraj, double* d_dctrl, void* stream);
/* Reverse sweep, its transpose:  lam = 0;  for i = L-1 .. 0:  g_u = seed_ctrl[i] + dt F_u' lam;  grad_wt += W_i' g_u;  grad_track[min(i, Lt-1)] +=
 * O_i' g_u;  lam <- seed_traj[i] + lam + dt F_x' lam + K_i' g_u;  grad_init = lam.  seed_traj [B,L,5], seed_ctrl [B,L,2]: NULL = zero.
 * grad_init [B,5], grad_wt [B,7] (per ego: sum the rows for shared weights, as mpc_sens_weights), grad_track [B,Lt,3] (needs ogain): any may
 * be NULL.  NaN gains of step i make grad_init, grad_wt and the rows of grad_track up to min(i, Lt-1) of that ego NaN.  Stateless as above.  */
int mpc_loop_adjoint(mpc_handle* h, int32_t B, int32_t L, const double* traj, const double* ctrl, const double* kgain, const double* wgain,
                     const double* ogain, int32_t Lt, const double* seed_traj, const double* seed_ctrl, double* grad_init, double* grad_wt,
                     double* grad_track);
int mpc_loop_adjoint_dev(mpc_handle* h, int32_t B, int32_t L, const double* d_traj, const double* d_ctrl, const double* d_kgain,
                         const double* d_wgain, const double* d_ogain, int32_t Lt, const double* d_seed_traj, const double* d_seed_ctrl,
                         double* d_grad_init, double* d_grad_wt, double* d_grad_track, void* stream);
/* FORCES-mode stage functions (scope row a11): what `FORCESNLPsolver_casadi2forces` evaluates per stage
 * (test/FORCESNLPsolver/FORCESNLPsolver_interface.c:41-198 -> casadi_f0..f9, FORCESNLPsolver_model.c:75-1756; the model
 * of ForcesproOptimizer, optimizer.py:91-245) for B independent (z, p) pairs.  z [B,7] = (deltaDot, aLong, x, y, delta, v,
 * psi), p [B,10] = (x_ref, y_ref, v_des, psi_ref, obstacle centre / front / rear circle).  Outputs, row-major, any may be
 * NULL: f [B], grad_f [B,7], c [B,5] (one RK4 step of length dt), jac_c [B,5,7], h [B,10] (friction circle, nine squared
 * circle distances), jac_h [B,10,7].  terminal != 0: the last stage (terminal weights P, no input cost, no c).
 * Weights: Q / R / P of the handle's descriptor; dt, wheelbase (ODE), friction_div (2.578 in psi_dot), ego_offset too. */
int mpc_forces_stage_eval(mpc_handle* h, int32_t B, int32_t terminal, const double* z, const double* p, double* f,
                          double* grad_f, double* c, double* jac_c, double* hval, double* jac_h);

/* FORCES-mode solve (scope row f3): `output, exitflag, info = solver.solve(problem)` of ForcesproOptimizer
 * (optimizer.py:326; C side FORCESNLPsolver_solve, test/FORCESNLPsolver/include/FORCESNLPsolver.h:117-219) for B independent
 * problems: ONE step of sequential quadratic programming from the guess x0, as the reference configures FORCESPRO
 * (sqp_nlp.maxqps = 1, BFGS initialised to 2.5 I, reg_hessian 5e-6; optimizer.py:225-240).  Horizon N = the descriptor's
 * N (at most 192), weights Q / R / P of the descriptor.  x0 [B,N,7] = problem["x0"], xinit [B,5], all_parameters [B,N,10] (optimizer.py:
 * 124-127, 313-318); lb/ub [7], hl/hu [10] = inequal_constraint() (optimizer.py:100-119; +-inf or |v| >= 1e300 = absent).
 * hessian_mode 0: QP Hessian = exact Hessian of the least-squares cost (Gauss-Newton SQP, default); 1: the literal
 * `bfgs_init = 2.5 I` (see csrc/mpc_forces_qp.h: forces_hessian_diag for why that is not the default).
 * Outputs: x_out [B,N,7] = output["x01".."xN"]; exitflag [B] (1 solved, 0 iteration limit, -6 NaN, -7 inconsistent
 * linearised constraints; FORCESNLPsolver.h:68-106); it [B] interior-point iterations; res [B] final residual.          */
int mpc_forces_solve_batch(mpc_handle* h, int32_t B, const double* x0, const double* xinit, const double* all_parameters,
                           const double* lb, const double* ub, const double* hl, const double* hu, int32_t hessian_mode,
                           double* x_out, int32_t* exitflag, int32_t* it, double* res);

/* The FORCES-mode closed loop around that solve (ForcesproOptimizer.optimize, optimizer.py:246-366) for B egos, on the device with
 * nothing coming back to the host between the steps: the never-refreshed guess problem["x0"] = tiled initial point (:264-274), the
 * run-time parameters of every step (next N path points / orientations replenished with the last one, desired velocity ramping to 0
 * over the last N steps of the run, obstacle circle centres of the descriptor; :292-323), one SQP step, first input (+ N(0, sigma)
 * on it alone with noise_mode 2, :348-354; 0 = none; seeded counter-based samples as in mpc_closed_loop_batch_ex), one RK4 plant step
 * (:356).  init_state [B,5], init_acc [B] or NULL (0), path [B,Lp,2], orient [B,Lp] (the reference has Lp = L = iter_length), vdes [B];
 * lb/ub/hl/hu as in mpc_forces_solve_batch (host arrays).  Outputs traj [B,L,5], ctrl [B,L,2], step_flag [B,L] or NULL (the exitflag of
 * every step; the reference asserts it is 1, optimizer.py:330).                                                                  */
int mpc_forces_closed_loop_batch(mpc_handle* h, int32_t B, int32_t L, int32_t Lp, const double* init_state, const double* init_acc,
                                 const double* path, const double* orient, const double* vdes, const double* lb, const double* ub,
                                 const double* hl, const double* hu, int32_t hessian_mode, int32_t noise_mode, double sigma, uint64_t seed,
                                 double* traj, double* ctrl, int32_t* step_flag);
int mpc_forces_closed_loop_batch_dev(mpc_handle* h, int32_t B, int32_t L, int32_t Lp, const double* d_init_state, const double* d_init_acc,
                                     const double* d_path, const double* d_orient, const double* d_vdes, const double* lb, const double* ub,
                                     const double* hl, const double* hu, int32_t hessian_mode, int32_t noise_mode, double sigma, uint64_t seed,
                                     double* d_traj, double* d_ctrl, int32_t* d_step_flag, void* stream);
/* The same loop past per-ego obstacles that move, with a guess that may follow the plan (neither is in the reference).  Everything not named
 * here keeps the meaning it has in mpc_forces_closed_loop_batch[_dev].
 * guess_mode 0: the reference's guess, the tiled initial point, never refreshed.  1 (real-time iteration): after a solve with exitflag 1 the guess of
 * the next solve is the solution shifted by one stage, zbar[j] = z_out[min(j + 1, N - 1)]; after any other exitflag the guess stays as it was.  Step 0
 * uses the tiled initial point in both modes; the applied input is always z_out[0][0:2] (+ noise).
 * obst_track [B, Lt, 3] = (x, y, heading) of ego b's obstacle at loop step i; its circle centres: the pose's centre, then +- obst_offset along the
 * heading (as mpc_closed_loop_batch_obst).  Lt = 1: the obstacle stands still; Lt >= L: it moves; Lt = 0 with a NULL track: the descriptor's centres in
 * every stage -- predict must then be 0 and clearance NULL; any other Lt: MPC_ERR_INVALID with a message.
 * predict 0: every stage of step k sees pose row min(k, Lt - 1), frozen over the horizon as in the NLP loop.  1: stage j sees row min(k + j, Lt - 1) --
 * stage j's state is the state at time k + j (stage 0 is pinned to xinit); rows past the track repeat its last pose.  The path index of stage j
 * stays k + 1 + j, the reference's own choice (optimizer.py:292-318).
 * clearance [B, L] or NULL: clearance[b, i] = min over ALL NINE circle pairs (the FORCES model constrains every ego circle against every obstacle
 * circle) of distance - r_sum for the state before step i (traj[b, i]) against the pose at step i; ego circles: the descriptor's ego_offset.
 * With guess_mode 0 and Lt 0 the outputs are bit for bit those of mpc_forces_closed_loop_batch[_dev] on the same handle.  The _dev form enqueues the
 * whole loop on `stream` (one bookkeeping launch between two solves) and synchronises nothing.  nx != 5, L < N and a bad noise mode are refused as
 * there.  Like every loop it ends the life of the sensitivity snapshot.                                                                            */
int mpc_forces_closed_loop_batch_obst(mpc_handle* h, int32_t B, int32_t L, int32_t Lp, const double* init_state, const double* init_acc,
                                      const double* path, const double* orient, const double* vdes, const double* lb, const double* ub,
                                      const double* hl, const double* hu, int32_t hessian_mode, int32_t guess_mode, int32_t Lt,
                                      const double* obst_track, double obst_offset, int32_t predict, double r_sum, int32_t noise_mode, double sigma,
                                      uint64_t seed, double* traj, double* ctrl, int32_t* step_flag, double* clearance);
int mpc_forces_closed_loop_batch_obst_dev(mpc_handle* h, int32_t B, int32_t L, int32_t Lp, const double* d_init_state, const double* d_init_acc,
                                          const double* d_path, const double* d_orient, const double* d_vdes, const double* lb, const double* ub,
                                          const double* hl, const double* hu, int32_t hessian_mode, int32_t guess_mode, int32_t Lt,
                                          const double* d_obst_track, double obst_offset, int32_t predict, double r_sum, int32_t noise_mode,
                                          double sigma, uint64_t seed, double* d_traj, double* d_ctrl, int32_t* d_step_flag, double* d_clearance,
                                          void* stream);

/* Post-hoc trajectory metrics (scope row f4) for B planned trajectories traj [B,L,5] (host buffers, any output may be NULL):
 *   deviation [B,L]  distance to the nearest point of origin_path [B,Lo,2]   (plot_deviation_euclidean_dis,
 *                    mpc_planner.py:184-199; find_closest_point, configuration.py:26-37)
 *   rmsd [B,2]       sqrt(sum_i (ref_path[i] - x[i])^2 / (L-1)) of x and y   (compute_rmsd, mpc_planner.py:279-292)
 *   clearance [B]    min over steps and circle pairs of distance - r_sum; all_pairs = 0: the three pairs (ego circle j,
 *                    obstacle circle j) that optimizer.py:395-403 constrains (each three times), all_pairs = 1: all nine
 *                    pairs; circle centres of the handle's problem template                                          */
int mpc_metrics_batch(mpc_handle* h, int32_t B, int32_t L, int32_t Lo, const double* traj, const double* ref_path,
                      const double* origin_path, double r_sum, int32_t all_pairs, double* deviation, double* rmsd,
                      double* clearance);
/* Collision / road verdict of B planned trajectories traj [B,L,5] (scope row f4): what the reference's test asks of
 * commonroad_dc's collision checker (test/test_mpc_planner.py:37-47) -- does the ego rectangle (mpc_planner.py:99: length 4.3,
 * width 1.8, centred on the planned position, heading psi) of some step overlap an obstacle rectangle of the same time step, or
 * leave the drivable corridor?  obst [n_obst,L,5] = (x, y, length, width, orientation) per obstacle and time step (a static
 * obstacle repeats its row; length <= 0 = absent at that step), or n_obst = 0.  left [n_left,2] / right [n_right,2]: boundary
 * polylines of the corridor in driving direction (0 points = no road check).  Outputs [B]: index of the first offending step,
 * -1 = none.                                                                                                              */
int mpc_validity_batch(mpc_handle* h, int32_t B, int32_t L, const double* traj, double ego_length, double ego_width, int32_t n_obst,
                       const double* obst, int32_t n_left, const double* left, int32_t n_right, const double* right,
                       int32_t* first_collision, int32_t* first_off_road);
int mpc_validity_batch_dev(mpc_handle* h, int32_t B, int32_t L, const double* d_traj, double ego_length, double ego_width, int32_t n_obst,
                           const double* d_obst, int32_t n_left, const double* d_left, int32_t n_right, const double* d_right,
                           int32_t* d_first_collision, int32_t* d_first_off_road, void* stream);
/* ... with obstacles of its own per trajectory: obst [B,n_obst,L,5], everything else as above (a sweep of egos that each had their own
 * obstacle, mpc_closed_loop_batch_obst)                                                                                       */
int mpc_validity_batch_ego(mpc_handle* h, int32_t B, int32_t L, const double* traj, double ego_length, double ego_width, int32_t n_obst,
                           const double* obst, int32_t n_left, const double* left, int32_t n_right, const double* right,
                           int32_t* first_collision, int32_t* first_off_road);
int mpc_validity_batch_ego_dev(mpc_handle* h, int32_t B, int32_t L, const double* d_traj, double ego_length, double ego_width, int32_t n_obst,
                               const double* d_obst, int32_t n_left, const double* d_left, int32_t n_right, const double* d_right,
                               int32_t* d_first_collision, int32_t* d_first_off_road, void* stream);
int mpc_closed_loop_batch_dev(mpc_handle* h, int32_t B, int32_t L, int32_t Lp, const double* d_init_state, const double* d_path,
                              const double* d_orient, const double* d_vdes, double* d_traj, double* d_ctrl,
                              int32_t* d_step_status, void* stream);
/* device-pointer forms of the two entry points above: work enqueued on `stream`, no allocation per call (scratch lives in
 * the handle), no synchronisation.  lb / ub / hl / hu of the FORCES solve are small HOST arrays (they go by value).      */
int mpc_metrics_batch_dev(mpc_handle* h, int32_t B, int32_t L, int32_t Lo, const double* d_traj, const double* d_ref_path,
                          const double* d_origin_path, double r_sum, int32_t all_pairs, double* d_deviation, double* d_rmsd,
                          double* d_clearance, void* stream);
int mpc_forces_solve_batch_dev(mpc_handle* h, int32_t B, const double* d_x0, const double* d_xinit, const double* d_all_parameters,
                               const double* lb, const double* ub, const double* hl, const double* hu, int32_t hessian_mode,
                               double* d_x_out, int32_t* d_exitflag, int32_t* d_it, double* d_res, void* stream);

/* Run-time switches of a handle (20).  They are read from the environment once, at mpc_create (MPCGPU_<NAME IN CAPITALS>), and changed afterwards
 * only through this call; value NULL restores the default.  Unknown name -> MPC_ERR_INVALID.
 *   what is solved
 *     "friction_lb"      the lower bound lbg[0] = 0 of the reference's stage-0 friction row sqrt((a_0^2 + v_0^2 tan(delta_0)/2.578)^2)
 *                        (MPC_Planner/optimizer.py:378, 424-425): "nlp" / 0 (default) = implied by the absolute value, no barrier -- a solve returns
 *                        the optimum of the NLP; "ipopt" / 1 = the row as IPOPT sees it, a slack with both bounds and a log barrier on the lower one
 *                        too: the kink of |.| becomes a wall the slack does not cross and a solve can end AT it, depending on the warm start --
 *                        what the reference's recorded ZAM_Over-1_1 run shows at steps 4 and 13 (tests/test_recorded_residuals.py)
 *     "rescue"           0: no second chance for stalled instances (see above)
 *     "rescue_wg"        0: the second chance only behind the launch (rescue_dev); 2: inside k_solve_wg wherever the batch runs one instance per
 *                        workgroup; 1 (default): inside k_solve_wg when the handle's previous solve had stalled instances, else behind the launch
 *                        -- same levels, same bookkeeping, same bits either way (the kernel with the second chance inside costs a batch that
 *                        never stalls 6 - 10 %)
 *     "rescue_alone"     1: the caller knows that instances of this handle's batches stall (collision avoidance): batches up to 8192 instances run in
 *                        k_solve_wg alone, one instance per wavefront, with the second chance inside the launch (B = 4096: 8.3 -> 4.9 ms); an option, not
 *                        a heuristic, because it changes which Riccati sweeps serve an instance -- the last bits of the rows
 *   which kernels serve the iteration loop (every combination gives the same iteration counts; bits as documented in DESIGN.md section 4)
 *     "pipeline"         0: one launch per kernel and iteration (the path of horizons above 63 and trace mode, and what
 *                        an abandoned persistent launch falls back to) instead of the single persistent launch k_pipeline
 *     "hybrid"           0: the pipeline runs every tile to its end; default 1: tiles with few instances left go to k_solve_wg
 *     "hybrid_bx"        instances per wavefront of k_solve_wg: 1, 2, or 0 (default) = by batch size
 *     "hybrid_live"      live instances per tile of 64 at which a tile changes over (a smaller last tile: the same fraction; -1, default: from the
 *                        machine's size; 64: k_solve_wg alone)
 *     "pipe_help"        1 / 0: the Riccati workers of the pipeline take / do not take one published stage item while their tile is with the stage
 *                        workers; -1 (default): where a round has more than three stage items per stage worker (N = 50, B = 8192).  Only the
 *                        kernels with the reference's bound structure compiled in have that variant ("bound_mask"): ignored elsewhere
 *     "pipe_early"       stages before the end of a tile's forward Riccati sweep at which its stage items go into the pipeline's ready queue (the
 *                        stage workers then have the loads that do not read the step in flight when the sweep ends): 0 behind the sweep, n stages
 *                        (clamped to the horizon); -1 (default): 18 in converged mode, 0 with a fixed iteration count.  Never with helping
 *                        Riccati workers ("pipe_help").  Same bits at every value
 *     "red_transpose"    default 1: the stage items of the pipeline reduce their ten-field record over the stages of an instance by a transpose
 *                        through LDS (one lane per field and instance folds the column); 0: by the lane butterfly.  Same bits either way
 *     "bound_mask"       0: every bound side looked up at run time (variant 0 of the loop kernels); default 1: the kernels with the bound structure
 *                        of the reference's NLPs compiled in (optimizer.py:421-491) whenever the bounds handed to mpc_set_bounds have it
 *     "big_wg"           1: 512-thread stage workgroups (what horizons above 63 use) also for short horizons
 *     "groups"           2..4: sub-batches on streams of their own (one launch per kernel; measured, not the default)
 *     "max_batch"        instances per chunk (a batch whose workspace would pass 4 GiB is solved in chunks of whole tiles anyway)
 *   host side
 *     "loop_async"       0: closed loop with a host round trip per step
 *     "sync_spin"        0: block in the one synchronisation of a solve instead of polling the stream
 *   states (mpc_get_option only): "pipe_aborts" persistent launches of this handle that had to be abandoned (each such solve started over with one
 *                        launch per kernel), "pipe_disabled" 1 once there were three: the handle stays on one launch per kernel
 *   test and measurement aids
 *     "pipe_test_abort"  1: the persistent launch raises its abort word at once (exercises the restart path)
 *     "pipe_xcd_mask"    pretend XCDs away (a partitioned device)
 *     "poison"           1: NaN into every row of the workspace before a solve (a read of something the solve has not written shows as status -6)
 *     "timing"           sum of 1 (k_stage / k_riccati), 2 (k_pipeline workers), 4 (k_solve_wg rounds), 8 (k_start), 16 (k_solve_wg workgroup trace):
 *                        shader-clock stamps of those kernels printed to stderr after the solve (tools/pipe_timing.py, res_timing.py, ...)       */
int mpc_set_option(mpc_handle* h, const char* name, const char* value);
/* current value of an option (so that a caller that changes one for a moment can put the PREVIOUS value back, not the default) */
int mpc_get_option(const mpc_handle* h, const char* name, int64_t* value);

/* ---- measurement helpers (bench.py / tests) ---------------------------------------------------------- */
/* kernel timing of the LAST mpc_solve_batch[_dev] call, measured with HIP events on the solve stream when
 * profiling is enabled: out[0] = total ms in the Riccati factor/solve kernel, out[1] = its launch count,
 * out[2] = total ms in the stage (line-search/assemble) kernel, out[3] = its launch count,
 * out[4] = ms in init + output kernels, out[5] = IPM iterations launched.                                 */
/* enable = 2: the two kernels of a hybrid solve's iteration loop are timed as ONE span (mpc_get_pipeline_profile out[0] = the loop, the
 * resident profile's out[0] = 0): no event between them -- a marker costs the stream a few microseconds that a production solve does not pay */
int mpc_set_profiling(mpc_handle* h, int32_t enable);
int mpc_get_profile(const mpc_handle* h, double out[6]);
/* When the last call ran all its iterations in ONE persistent launch (k_pipeline: batches of 1024..8192 instances;
 * MPCGPU_PIPELINE=0 turns it off) the per-kernel figures above are zero and this reports instead:
 * out[0] = ms of that launch (profiling enabled only), out[1] = 1 if the pipeline ran (0: one launch per kernel),
 * out[2] = iterations of the slowest tile, out[3] / out[4] = ms the Riccati / stage workers spent waiting for work,
 * summed over workers, out[5] = ms the stage workers spent on work items, out[6] = work items processed,
 * out[7] = stage workers + Riccati workers / 1000.                                                          */
int mpc_get_pipeline_profile(const mpc_handle* h, double out[8]);
/* The workgroup-resident kernels.  k_solve_wg (a workgroup keeps its instances for all their remaining iterations: the stage phases of
 * the other paths + a wave-per-instance Riccati on the fp64 matrix pipe) finishes the instances of the tiles that left the pipeline
 * (hybrid solve, the default: options "hybrid", "hybrid_bx", "hybrid_live") or solves a small batch alone ("hybrid_live" = 64: any batch).
 * out[0] = ms of that launch (profiling enabled only), out[1] = 1 if such a kernel ran in the last call, out[2] = rounds (iterations)
 * of its slowest workgroup, out[3] = workgroups of the launch, out[4] = rounds summed over the workgroups, out[5] = backward Riccati
 * sweeps (> rounds when inertia corrections repeat a sweep; two instances of a wavefront share a sweep), out[6] = instance-iterations
 * it performed (the rest of the call's iterations ran in the pipeline).                                                             */
int mpc_get_resident_profile(const mpc_handle* h, double out[8]);
/* Measurement helper for the roofline of bench.py: GB/s (bytes read + bytes written per second) of a plain streaming copy kernel of
 * this library (16 bytes per lane and access, grid-stride loop over `bytes` of device memory, best of `reps` launches on the handle's
 * stream) -- the bandwidth a kernel that only moves data reaches on this device, next to the 8 TB/s of the data sheet.              */
int mpc_measure_copy_bandwidth(mpc_handle* h, size_t bytes, int32_t reps, double* gbs);

/* debugging: per-iteration per-instance scalars of a host solve.  trace: [max_iter+1, 8, B] doubles
 * rows {mu, theta, phi, alpha, alpha_dual, delta_w, E0, n_trials}; returns iterations launched in *n_it. */
int mpc_solve_batch_trace(mpc_handle* h, int32_t B, const double* x0, const double* p, const double* obst,
                          double* x_out, int32_t* status, int32_t* iters, double* kkt,
                          double* trace, int32_t trace_rows, int32_t* n_it);

int mpc_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MPCGPU_H */
