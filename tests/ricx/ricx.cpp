// tests/ricx/ricx.cpp -- CPU harness of the one-instance-per-lane Riccati recursion (TEST INFRASTRUCTURE, not shipped).
//
// Runs a batch of cases (tests/riccati_ref.py writes them) through ric_matrix_step / ric_vector_step / riccati_forward_step of
// <package>/csrc/mpc_stage_math.h with the inertia-correction loop of riccati_instance, in the instantiation the caller names -- the driver
// is tools/ubench/ric_cases.h, the same lines the device kernel of tools/ubench/ric_mfma_test.hip runs one case per lane.  Built by
// tests/test_riccati_accuracy_cpu.py with g++ into a temporary directory.
#include <vector>

#include "../../tools/ubench/ric_cases.h"

using namespace ricx;

template <int NX>
static void run_case(const double* cs, int path, double* out) {
    const int N = (int)cs[C_N];
    Params P{};
    P.N = N; P.dt = cs[C_DT]; P.nx = NX; P.B = 1; P.Bp = 64;
    P.tile_elems = dz_tile_elems<NX>(N);
    std::vector<double> dz(P.tile_elems, 0.0);
    P.WS = dz.data(); P.DZ = dz.data();
    const uint32_t bb = 3;                    // (any instance of the tile)
    lane_backward<NX>(P, cs, path, out);
    lane_forward<NX>(P, bb, N, cs, out);
    copy_step<NX>(dz.data(), P.tile_elems, bb, N, out);
}

// in: a case file of n_in doubles; out: n_out doubles, one result block per case.  Returns 0, or a negative number for a malformed file.
extern "C" int ricx_run(const double* in, size_t n_in, int path, double* out, size_t n_out) {
    if (n_in < 1 || path < 0 || path >= N_PATHS) return -1;
    const int n = (int)in[0];
    size_t ci = 1, oi = 0;
    for (int c = 0; c < n; ++c) {
        if (ci + CASE_HEAD > n_in) return -2;
        const int nx = (int)in[ci + C_NX], N = (int)in[ci + C_N];
        if ((nx != 5 && nx != 6) || N < 1 || ci + case_doubles(N) > n_in || oi + out_doubles(N) > n_out) return -3;
        for (size_t q = 0; q < out_doubles(N); ++q) out[oi + q] = 0.0;
        if (nx == 5) run_case<5>(in + ci, path, out + oi);
        else run_case<6>(in + ci, path, out + oi);
        ci += case_doubles(N);
        oi += out_doubles(N);
    }
    return (ci == n_in && oi == n_out) ? 0 : -4;
}
