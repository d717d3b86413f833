// mpc_red_fold.h -- the ORDER in which the per-instance reductions of the stage phases combine their leaves, as plain C++ (host and device).
//
// A reduction (Red0 .. Red3, mpc_stage_math.h) combines one value per stage thread over the stages of an instance column.  The wave-level
// form (block_reduce, mpcgpu.hip) is an xor butterfly over the lanes of a wavefront -- distances bx, 2 bx, .., 32 in lane terms, 1, 2, ..,
// 32 / bx in stage terms -- followed, in a workgroup of several wavefronts, by a sequential fold over the wavefronts' results through LDS.
// What the lane of stage 0 of a column computes that way is, with W = 64 / bx stages per wavefront,
//     T(lo, 1)   = leaf[lo]
//     T(lo, len) = T(lo, len / 2) o T(lo + len / 2, len / 2)                  the balanced tree, the lower half on the left
//     result     = ((T(0, W) o T(W, W)) o T(2 W, W)) o T(3 W, W)              across the wavefronts, left to right
// with `a o b` = red_combine(a, b): `a` is the lane's own value, `b` the one it receives.  Stage threads beyond the horizon (and those of
// a column that is not iterating) carry red_neutralN().
//
// red_fold() states that order once; the transposed form of the reduction (block_reduce_t, mpcgpu.hip: the leaves of a column go through
// LDS to ONE lane per (field, column), which folds them with red_tree_field) and tests/redfold (the butterfly emulated lane by lane) are
// both written against it.
//
// Bit identity with the butterfly:
//   * the lane of stage 0 performs exactly the combines above, operands in this order: its result and red_fold's are the same bits whatever
//     the operators do;
//   * every OTHER lane of the column performs the same tree with the operands of some combines exchanged (lane s receives T(s ^ 1, 1) as
//     `b` where stage 0's subtree has it as `a`).  That all lanes of a column end with the same bits -- which the phases rely on, and which
//     makes handing every lane the stage-0 result a change of no bit -- ASSUMES the three operators commutative bit for bit:
//       +     is, for every pair of IEEE doubles that are not both NaN;
//       fmin / fmax are where the hardware's v_min_f64 / v_max_f64 are used (they order -0 below +0, so fmin(+0, -0) = fmin(-0, +0) = -0, and
//             return the other operand for a quiet NaN); a HOST libm may return its first operand for a pair of zeros of opposite sign --
//             there the lanes of a column can differ in the sign of a zero, the lane of stage 0 and red_fold never do;
//       NaN   two NaNs of different payload combine to either: the phases produce no NaN in a min / max field (Red3::nan is a 0 / 1 flag,
//             combined by fmax), and a NaN in a sum field reaches every lane as the canonical quiet NaN.
#pragma once

#include "mpc_stage_math.h"

namespace mpc {

// ---- per-field view of red_combine: which operator combines field q of a reduction record (the doubles of the struct, in order).
//      KEEP IN STEP with red_combine (mpc_stage_math.h), which stays the definition; tests/redfold checks the two against each other
//      for every field of every record.
enum RedOp : int { RED_SUM = 0, RED_MIN = 1, RED_MAX = 2 };
MPC_HD constexpr int red_kind(const Red0*, int) { return RED_MAX; }
MPC_HD constexpr int red_kind(const Red1*, int q) { return q < 2 ? RED_MIN : RED_SUM; }
MPC_HD constexpr int red_kind(const Red2*, int q) { return q < 3 ? RED_SUM : RED_MAX; }
MPC_HD constexpr int red_kind(const Red3*, int q) { return q == 2 ? RED_MIN : (q >= 4 && q <= 8) ? RED_SUM : RED_MAX; }
template <int KIND> MPC_HD double red_op(double a, double b) {
    if constexpr (KIND == RED_SUM) return a + b;
    else if constexpr (KIND == RED_MIN) return fmin(a, b);
    else return fmax(a, b);
}

// ---- the fold of whole records: `leaves` = the values of one instance column, stage by stage, nwaves * (64 / bx) of them
template <class R> MPC_HD R red_fold_tree(const R* leaves, int len) {
    if (len == 1) return leaves[0];
    R a = red_fold_tree(leaves, len / 2);
    const R b = red_fold_tree(leaves + len / 2, len / 2);
    red_combine(a, b);
    return a;
}
template <class R> MPC_HD R red_fold(const R* leaves, int bx, int nwaves) {
    const int W = 64 / bx;
    R acc = red_fold_tree(leaves, W);
    for (int w = 1; w < nwaves; ++w) {
        const R o = red_fold_tree(leaves + w * W, W);
        red_combine(acc, o);
    }
    return acc;
}

// ---- the same fold of ONE field, unrolled: leaf(s) gives the field's value at stage s (lo is a literal after inlining)
template <int KIND, int LEN, class Leaf> MPC_HD double red_tree_field(const int lo, Leaf&& leaf) {
    if constexpr (LEN == 1) {
        return leaf(lo);
    } else {
        const double a = red_tree_field<KIND, LEN / 2>(lo, leaf);
        const double b = red_tree_field<KIND, LEN / 2>(lo + LEN / 2, leaf);
        return red_op<KIND>(a, b);
    }
}
// W = 64 / bx stages per wavefront (a literal: 8 .. 64), nwaves wavefronts
template <int KIND, int W, class Leaf> MPC_HD double red_fold_field(const int nwaves, Leaf&& leaf) {
    double acc = red_tree_field<KIND, W>(0, leaf);
    for (int w = 1; w < nwaves; ++w) acc = red_op<KIND>(acc, red_tree_field<KIND, W>(w * W, leaf));
    return acc;
}

}  // namespace mpc
