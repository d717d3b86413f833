"""GPU (-m gpu): the reduction over an instance's stages in its transposed form (block_reduce_t, csrc/mpcgpu.hip: the leaves of a column
go through LDS to one lane per (field, column), which folds them in the order of csrc/mpc_red_fold.h) against the lane butterfly
(block_reduce) of the SAME build -- option red_transpose = 1 (the default) and 0 on one handle.  The two perform the same combines in the same
order (tests/test_red_fold_cpu.py), so rows, statuses, iteration counts and KKT errors must be the same bytes.

The transposed form serves the four-wavefront stage items of k_pipeline (their ten-field record, Red3); the single-wavefront workgroups
of k_solve_wg keep the butterfly (DESIGN_HISTORY.md: built there too, slower, not kept).  The shapes that run in k_solve_wg alone stay in
the list: they hold the option to changing nothing there.

Shapes: the smallest at which the reduction can go wrong --
  lane following N = 30, nx = 6, B = 3      k_solve_wg alone, one instance per wavefront (31 of 64 lanes: the upper half of the tree is neutral)
  B = 2 with hybrid_bx = 2                  two instances per wavefront, 62 lanes, two padding lanes
  N = 1 and N = 2                           the tree's shortest forms: two and three leaves
  N = 31 with hybrid_bx = 2                 all 32 stages of both columns in use, no padding lane
  B = 65 through the pipeline (hybrid = 0)  a ragged second tile, four-wavefront stage items, a finished column next to one that runs
  B = 130 with the hand-over                both loop kernels in one solve (hybrid_live = 40)
  N = 23 and N = 16 through the pipeline    stage items of three wavefronts: the fold over the wavefronts one step shorter
  collision avoidance B = 8, rescue_wg = 2  the restart path: wg_restart's reductions between the rounds' own
"""
import numpy as np
import pytest

from helpers import CA_CFG, FAMILIES, ca_batch, make_solver, set_cfg_bounds
from oracle.nlp_numpy import WEIGHTS_ZAM_LF, NLPConfig, synthetic_batch

pytestmark = pytest.mark.gpu

LF30 = FAMILIES["zamlf_n30_nx6"][0]


def lf(N):
    return NLPConfig(N=N, nx=6, **WEIGHTS_ZAM_LF)


# name: (config, B, options, k_solve_wg runs, k_pipeline runs)
CASES = {
    "n30_B3_one_per_wavefront": (LF30, 3, {}, True, False),
    "n30_B2_two_per_wavefront": (LF30, 2, {"hybrid_bx": "2"}, True, False),
    "n1_B3": (lf(1), 3, {}, True, False),
    "n1_B2_two_per_wavefront": (lf(1), 2, {"hybrid_bx": "2"}, True, False),
    "n2_B3": (lf(2), 3, {}, True, False),
    "n2_B2_two_per_wavefront": (lf(2), 2, {"hybrid_bx": "2"}, True, False),
    # (32 stages of two instances would fill a wavefront without a padding lane, but their records do not fit a quarter of a CU's LDS: the
    #  plan keeps such a batch in the pipeline -- the case runs as the plan decides; with one instance per wavefront the 32 stages are the
    #  full lower half of the tree)
    "n31_B2_two_per_wavefront_asked": (lf(31), 2, {"hybrid_bx": "2"}, False, True),
    "n31_B3_full_half_tree": (lf(31), 3, {}, True, False),
    "n30_B65_pipeline": (LF30, 65, {"hybrid": "0"}, False, True),
    "n30_B130_hand_over": (LF30, 130, {"hybrid_live": "40"}, True, True),
    # three-wavefront stage items: 24 stages fill them (N = 23), 17 leave the third wavefront with one real stage (N = 16)
    "n23_B65_pipeline_three_wavefronts": (lf(23), 65, {"hybrid": "0"}, False, True),
    "n16_B65_pipeline_padding_wavefront": (lf(16), 65, {"hybrid": "0"}, False, True),
    "ca_B8_restarts": (CA_CFG, 8, {"rescue_wg": "2"}, True, False),
}


@pytest.mark.parametrize("name", list(CASES))
def test_transposed_reduction_gives_the_butterflys_bytes(name):
    cfg, B, opts, wg, pipe = CASES[name]
    if cfg is CA_CFG:
        x0, p = ca_batch(cfg, B)
    else:
        x0, p = synthetic_batch(cfg, B)
    s = make_solver(cfg)
    if cfg is CA_CFG:
        set_cfg_bounds(s, cfg)
    for k, v in opts.items():
        s.set_option(k, v)
    assert s.get_option("red_transpose") == 1
    res = {}
    for form in ("1", "0", "1"):
        s.set_option("red_transpose", form)
        r = s.solve(x0, p)
        assert s.get_resident_profile()["ran"] == wg and s.get_pipeline_profile()["ran"] == pipe, (name, form)
        assert int(s.get_option("pipe_aborts")) == 0
        if form in res:          # (the transposed form twice: what it leaves in the records between solves changes nothing either)
            for k in ("x", "status", "iters", "kkt"):
                assert np.array_equal(getattr(r, k), res[form][k]), (name, "repeat", k)
        res[form] = {k: np.array(getattr(r, k), copy=True) for k in ("x", "status", "iters", "kkt")}
    print(f"{name}: converged {np.mean(res['1']['status'] == 1):.3f}, iterations {res['1']['iters'].mean():.2f} / {res['1']['iters'].max()}")
    assert np.any(res["1"]["status"] == 1)
    for k in ("x", "status", "iters", "kkt"):
        assert np.array_equal(res["1"][k], res["0"][k]), (name, k)
