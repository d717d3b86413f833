// tests/nlpx/nlpx.cpp -- CPU harness of the NLP evaluation and the multiplier mapping (TEST INFRASTRUCTURE, not shipped).
//
// The emulated solve of tests/emu/emu_solve.h (one launch per kernel and iteration: the iterate stays in the tile-major rows), then what
// k_eval_nlp and k_mult_out run on the GPU: nlp_eval_stage and mult_stage.  Built by tests/helpers.py (harness_lib) with g++ into a
// temporary directory.
#include <cmath>
#include <string>
#include <vector>

#include "../emu/emu_solve.h"

using namespace mpc;

template <int NX>
static void run(const HostProblem& hp, int B, const double* x0, const double* p, double* x_out, int32_t* status, double* lam_g, double* lam_x) {
    EmuSolve<NX> e;
    EmuOpts o;
    o.mailbox = false;
    e.run(hp, B, x0, p, x_out, status, nullptr, nullptr, o);
    e.multipliers(hp, x_out, status, lam_g, lam_x);
}

extern "C" int nlpx_solve(const mpc_problem_desc* desc, const double* lbx, const double* ubx, const double* lbg, const double* ubg,
                          int32_t friction_literal, int32_t B, const double* x0, const double* p, double* x_out, int32_t* status,
                          double* lam_g, double* lam_x) {
    HostProblem hp;
    const int rc = emu_problem(hp, desc, lbx, ubx, lbg, ubg, friction_literal);
    if (rc) return rc;
    if (desc->nx == 5) run<5>(hp, B, x0, p, x_out, status, lam_g, lam_x);
    else run<6>(hp, B, x0, p, x_out, status, lam_g, lam_x);
    return MPC_OK;
}

extern "C" int nlpx_eval(const mpc_problem_desc* desc, int32_t B, const double* x, const double* p, const double* obst, double* f, double* g) {
    HostProblem hp;
    hp.desc = *desc;
    Params P;
    fill_params(P, hp, B, ((size_t)B + 63) / 64 * 64, 1, nullptr, nullptr, nullptr, nullptr, false);
    const int N = desc->N, nx = desc->nx;
    const size_t nw = hp.n_w(), ng = hp.n_g();
    for (int b = 0; b < B; ++b) {
        const double* ob = obst ? obst + (size_t)b * 6 : P.obst;
        double fs = 0.0;
        for (int k = 0; k <= N; ++k)
            fs += nx == 5 ? nlp_eval_stage<5>(P, x + b * nw, p + b * nw, ob, k, g + b * ng) : nlp_eval_stage<6>(P, x + b * nw, p + b * nw, ob, k, g + b * ng);
        f[b] = fs;
    }
    return MPC_OK;
}
