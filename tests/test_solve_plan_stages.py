"""The launch plan of a solve with obstacle rows per stage (csrc/mpc_solve_plan.h: plan_solve with PlanState::per_inst_obst = OBST_PER_STAGE)
is the plan of a solve with one row per instance, field by field -- the same kernels, therefore the same bits where every stage's row is the
instance's -- over the shapes tests/test_solve_plan.py sweeps.  tests/emu's binding sets the mode from a flag (shared / per instance), so
the mode goes in through tests/predx (predx_solve_plan: the same options and state vector, every field of the plan out); for the modes
the emulation harness can express, the two bindings must tell the same plan."""
import ctypes as C

import numpy as np
import pytest

from helpers import abi, emu_desc, emu_lib, harness_lib
from test_solve_plan import CFGS, N_CU, OUT, ROWS, XCD_MASK, bounds_of

FIELDS = ("small_wg", "S", "bx", "threads", "nblk", "ntiles", "G", "stash_rows", "lds_bytes", "lds_init", "ric_lds", "masked", "cap", "chunk", "polled",
          "fused", "lds_pre", "lds_start", "res_path", "pipe_path", "hyb_bx", "resc_alone", "hyb_ok", "hand", "wg_resc", "wg_lds", "wg_grid", "xcd_mask",
          "n_xcd", "tiles_x", "cu_x", "n_ric", "pipe_cap", "pipe_help", "pipe_lead", "mbw_live", "stage_timing", "start_timing", "wg_timing", "wg_trace",
          "pipe_timing", "poison", "max_rows", "mailbox", "rescue", "loop_async")
SHARED, PER_INSTANCE, PER_STAGE = 0, 1, 2


def _args(fam, B, opts, state):
    opts = dict(opts)
    d = emu_desc(CFGS[fam], fixed_iters=int(opts.pop("fixed_iters", 0)))
    lbg, ubg, lbx, ubx = bounds_of(fam)
    names = (C.c_char_p * max(1, len(opts)))(*[k.encode() for k in opts])
    values = (C.c_char_p * max(1, len(opts)))(*[str(v).encode() for v in opts.values()])
    st = dict(dict(resc_hint=0, trace=0, in_rescue=0), **state)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))      # noqa: E731
    return d, (dp(lbx), dp(ubx), dp(lbg), dp(ubg)), names, values, len(opts), st, (lbx, ubx, lbg, ubg)


def plan_fields(fam, B, opts, state, mode):
    L = C.CDLL(harness_lib("predx"))
    i64p = C.POINTER(C.c_int64)
    L.predx_solve_plan.argtypes = [C.POINTER(abi.MpcProblemDesc)] + [C.POINTER(C.c_double)] * 4 + [C.POINTER(C.c_char_p)] * 2 + [C.c_int32, i64p, C.c_int32, i64p]
    assert L.predx_plan_fields() == len(FIELDS)
    d, b, names, values, n, st, keep = _args(fam, B, opts, state)
    sv = np.array([N_CU, XCD_MASK, -1, 0, st["resc_hint"], B, 0, st["trace"], st["in_rescue"], 0], np.int64)
    out = np.zeros(len(FIELDS), np.int64)
    assert L.predx_solve_plan(C.byref(d), *b, names, values, n, sv.ctypes.data_as(i64p), mode, out.ctypes.data_as(i64p)) == 0
    return dict(zip(FIELDS, (int(v) for v in out)))


def emu_plan(fam, B, opts, state, per_inst):
    L = emu_lib()
    i64p = C.POINTER(C.c_int64)
    L.emu_solve_plan.argtypes = [C.POINTER(abi.MpcProblemDesc)] + [C.POINTER(C.c_double)] * 4 + [C.POINTER(C.c_char_p)] * 2 + [C.c_int32, i64p, i64p]
    L.emu_solve_plan.restype = C.c_int
    d, b, names, values, n, st, keep = _args(fam, B, opts, state)
    sv = np.array([N_CU, XCD_MASK, -1, 0, st["resc_hint"], B, per_inst, st["trace"], st["in_rescue"], 0], np.int64)
    out = np.zeros(len(OUT), np.int64)
    assert L.emu_solve_plan(C.byref(d), *b, names, values, n, sv.ctypes.data_as(i64p), out.ctypes.data_as(i64p)) == 0
    return dict(zip(OUT, (int(v) for v in out)))


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_per_stage_plan_is_the_per_instance_plan(row):
    _, fam, B, opts, state, _ = row
    # a batch beyond the chunk size: the call's first chunk and its last, as the library plans them
    sizes = {B}
    chunk = plan_fields(fam, B, opts, state, PER_INSTANCE)["max_rows"]
    if B > chunk:
        sizes |= {chunk, B - (B - 1) // chunk * chunk}
    for b in sorted(sizes):
        one, stg, shared = (plan_fields(fam, b, opts, state, m) for m in (PER_INSTANCE, PER_STAGE, SHARED))
        for f in FIELDS:
            assert stg[f] == one[f], (row[0], b, f)
        assert stg["masked"] == 0                                # (centres of its own per instance: never the kernels with one obstacle compiled in)
        # the binding tests/test_solve_plan.py uses tells the same plans for the modes it can express
        for per_inst, mine in ((0, shared), (1, one)):
            e = emu_plan(fam, b, opts, state, per_inst)
            got = dict(path=2 if mine["res_path"] else 1 if mine["pipe_path"] else 0, bx=mine["bx"], hyb_bx=mine["hyb_bx"], hand=mine["hand"],
                       n_ric=mine["n_ric"], help=mine["pipe_help"], chunk=mine["max_rows"], mailbox=mine["mailbox"], rescue=mine["rescue"],
                       n_xcd=mine["n_xcd"], tiles_x=mine["tiles_x"], wg_grid=mine["wg_grid"], ntiles=mine["ntiles"], masked=mine["masked"],
                       wg_resc=mine["wg_resc"], groups=mine["G"], loop_async=mine["loop_async"], xcd_mask=mine["xcd_mask"],
                       stash_rows=mine["stash_rows"], small_wg=mine["small_wg"])
            # (behind these, emu_solve_plan tells what set_bounds made of the lists -- flags and masks, no fields of the plan)
            assert set(e) - set(got) == {"dec_s", "has_fl", "has_fu", "has_ol", "has_ou", "lo_mask", "hi_mask", "dense_mask"}
            assert got == {k: e[k] for k in got}, (row[0], b, per_inst)


def test_the_shared_plan_differs_where_the_masked_kernels_serve_it():
    """(so that the comparison above is not one of three equal plans: the headline shape runs variant 2 without obstacle rows of its own)"""
    a, b = plan_fields("zamlf_n30_nx6", 4096, {}, {}, SHARED), plan_fields("zamlf_n30_nx6", 4096, {}, {}, PER_STAGE)
    assert a["masked"] == 1 and b["masked"] == 0 and a["pipe_path"] == b["pipe_path"] == 1
