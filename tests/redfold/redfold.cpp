// redfold.cpp -- harness of tests/test_red_fold_cpu.py: the reductions of the stage phases three ways, on the caller's leaves.
//   1. block_reduce (csrc/mpcgpu.hip) emulated LITERALLY for every thread of a workgroup of one to eight wavefronts: __shfl_xor as an index
//      permutation inside each wavefront, level by level, then the pass through LDS as it is written there;
//   2. red_fold (csrc/mpc_red_fold.h) on the leaves of each instance column, whole records through red_combine;
//   3. red_fold_field, the unrolled per-field form the transposed reduction runs on one lane per (field, column).
// The test compares the three bit for bit.
#include <cstring>
#include <vector>

#include "../../motion-planning-for-autonomous-driving-with-mpc_amd/csrc/mpc_red_fold.h"

using namespace mpc;

namespace {

template <class R>
void butterfly(std::vector<R>& r, const int bx, const int nw) {
    constexpr int NQ = sizeof(R) / sizeof(double);
    // for (int m = bx; m < 64; m <<= 1) { const R o = shfl_xor_struct(r, m); red_combine(r, o); }      -- every lane of every wavefront
    for (int wave = 0; wave < nw; ++wave) {
        R* w = r.data() + wave * 64;
        for (int m = bx; m < 64; m <<= 1) {
            R o[64];
            for (int lane = 0; lane < 64; ++lane) o[lane] = w[lane ^ m];
            for (int lane = 0; lane < 64; ++lane) red_combine(w[lane], o[lane]);
        }
    }
    if (nw > 1) {
        std::vector<double> lds((size_t)nw * NQ * bx);
        for (int t = 0; t < nw * 64; ++t) {
            const int wave = t >> 6, lane = t & 63;
            const double* mine = reinterpret_cast<const double*>(&r[t]);
            if (lane < bx)
                for (int q = 0; q < NQ; ++q) lds[(wave * NQ + q) * bx + lane] = mine[q];
        }
        // lds_barrier();
        for (int t = 0; t < nw * 64; ++t) {
            const int lane = t & 63, bl = lane & (bx - 1);
            R acc;
            double* a = reinterpret_cast<double*>(&acc);
            for (int q = 0; q < NQ; ++q) a[q] = lds[q * bx + bl];
            for (int w = 1; w < nw; ++w) {
                R o;
                double* op = reinterpret_cast<double*>(&o);
                for (int q = 0; q < NQ; ++q) op[q] = lds[(w * NQ + q) * bx + bl];
                red_combine(acc, o);
            }
            r[t] = acc;
        }
    }
}

template <int KIND, class Leaf> double field_w(const int bx, const int nw, Leaf&& leaf) {
    switch (bx) {
        case 1: return red_fold_field<KIND, 64>(nw, leaf);
        case 2: return red_fold_field<KIND, 32>(nw, leaf);
        case 4: return red_fold_field<KIND, 16>(nw, leaf);
        default: return red_fold_field<KIND, 8>(nw, leaf);
    }
}
Red0 neutral_of(const Red0*) { return red_neutral0(); }
Red1 neutral_of(const Red1*) { return red_neutral1(); }
Red2 neutral_of(const Red2*) { return red_neutral2(); }
Red3 neutral_of(const Red3*) { return red_neutral3(); }

// vals: [nw * 64][NQ] by thread (thread t = stage t / bx of column t % bx); threads of stages >= n_real must carry the neutral record
// out_emu: [nw * 64][NQ]; out_fold, out_field: [bx][NQ]
template <class R>
int run(const double* vals, const int bx, const int nw, const int n_real, double* out_emu, double* out_fold, double* out_field) {
    constexpr int NQ = sizeof(R) / sizeof(double);
    const int T = nw * 64, W = 64 / bx;
    std::vector<R> r((size_t)T);
    std::memcpy(r.data(), vals, sizeof(R) * T);
    const R neutral = neutral_of((const R*)nullptr);
    for (int t = 0; t < T; ++t)
        if (t / bx >= n_real && std::memcmp(&r[t], &neutral, sizeof(R)) != 0) return 2;
    butterfly(r, bx, nw);
    std::memcpy(out_emu, r.data(), sizeof(R) * T);
    for (int bl = 0; bl < bx; ++bl) {
        std::vector<R> leaves((size_t)nw * W);
        for (int s = 0; s < nw * W; ++s) std::memcpy(&leaves[s], vals + (size_t)(s * bx + bl) * NQ, sizeof(R));
        const R f = red_fold(leaves.data(), bx, nw);
        std::memcpy(out_fold + bl * NQ, &f, sizeof(R));
        for (int q = 0; q < NQ; ++q) {
            auto leaf = [&](int s) { return vals[(size_t)(s * bx + bl) * NQ + q]; };
            const int kind = red_kind((const R*)nullptr, q);
            out_field[bl * NQ + q] = kind == RED_SUM ? field_w<RED_SUM>(bx, nw, leaf) : kind == RED_MIN ? field_w<RED_MIN>(bx, nw, leaf) : field_w<RED_MAX>(bx, nw, leaf);
        }
    }
    return 0;
}

}  // namespace

extern "C" {
int redfold_nq(int which) { return which == 0 ? 1 : which == 1 ? 3 : which == 2 ? 4 : which == 3 ? 10 : -1; }
void redfold_neutral(int which, double* out) {
    const Red0 n0 = red_neutral0(); const Red1 n1 = red_neutral1(); const Red2 n2 = red_neutral2(); const Red3 n3 = red_neutral3();
    if (which == 0) std::memcpy(out, &n0, sizeof n0);
    if (which == 1) std::memcpy(out, &n1, sizeof n1);
    if (which == 2) std::memcpy(out, &n2, sizeof n2);
    if (which == 3) std::memcpy(out, &n3, sizeof n3);
}
int redfold_kind(int which, int q) {
    return which == 0 ? red_kind((const Red0*)nullptr, q) : which == 1 ? red_kind((const Red1*)nullptr, q) : which == 2 ? red_kind((const Red2*)nullptr, q)
                                                                                                                          : red_kind((const Red3*)nullptr, q);
}
int redfold_run(int which, const double* vals, int bx, int nw, int n_real, double* out_emu, double* out_fold, double* out_field) {
    if (!(bx == 1 || bx == 2 || bx == 4 || bx == 8) || nw < 1 || nw > 8 || n_real < 1 || n_real > nw * 64 / bx) return 1;
    switch (which) {
        case 0: return run<Red0>(vals, bx, nw, n_real, out_emu, out_fold, out_field);
        case 1: return run<Red1>(vals, bx, nw, n_real, out_emu, out_fold, out_field);
        case 2: return run<Red2>(vals, bx, nw, n_real, out_emu, out_fold, out_field);
        case 3: return run<Red3>(vals, bx, nw, n_real, out_emu, out_fold, out_field);
    }
    return 1;
}
}
