"""The launch plan of a solve (csrc/mpc_solve_plan.h: plan_solve) -- which kernels serve the iteration loop, how many instances per
wavefront of k_solve_wg, the hand-over threshold, the Riccati workers per XCD of the pipeline, the chunk size of a large batch, the
mailbox section of the workspace and the second chance -- on the CPU through the emulation harness (tests/emu: emu_solve_plan), and
against what the library reports on the GPU.

The expected values are read off the decision as solve_dev_impl made it before the plan was extracted (n_cu = 256, all eight XCDs);
the comment of a row says why.  A batch beyond the chunk size is solved in chunks: the path columns then describe its LAST chunk, which
is what the library's profiles describe after the call."""
import ctypes as C

import numpy as np
import pytest

from helpers import CA_CFG, FAMILIES, abi, ca_batch, emu_desc, emu_lib, make_solver, set_cfg_bounds
from oracle.nlp_numpy import WEIGHTS_ZAM_LF, BicycleNLP, NLPConfig, synthetic_batch

N_CU, XCD_MASK = 256, 0xFF
PATHS = {0: "kernels", 1: "pipe", 2: "wg"}          # one launch per kernel and iteration | k_pipeline (+ k_solve_wg) | k_solve_wg alone
OUT = ("path", "bx", "hyb_bx", "hand", "n_ric", "help", "chunk", "mailbox", "rescue", "n_xcd", "tiles_x", "wg_grid", "ntiles", "masked",
       "wg_resc", "groups", "loop_async", "xcd_mask", "stash_rows", "dec_s", "has_fl", "has_fu", "has_ol", "has_ou", "lo_mask", "hi_mask", "dense_mask",
       "small_wg")

LF30 = "zamlf_n30_nx6"
CFGS = {LF30: FAMILIES[LF30][0], "usalf_n50_nx5": FAMILIES["usalf_n50_nx5"][0], "ca": CA_CFG,
        "lf_n64_nx6": NLPConfig(N=64, nx=6, **WEIGHTS_ZAM_LF)}
# 4 GiB of workspace (32-bit buffer offsets) in whole tiles of 64 instances, without the mailbox section (mpc_host_common.h: ws_layout):
# N = 30, nx = 6: 4492 rows per tile -> 1867 tiles; N = 64: 9320 rows -> 900 tiles
WS_CHUNK_N30, WS_CHUNK_N64 = 1867 * 64, 900 * 64
PIPE_CHUNK = 256 * 64                                # PIPE_MAX_TILES tiles: what one persistent launch takes

# (id, family, B, options, state, expected); state: resc_hint, trace, in_rescue; gpu: the GPU can put a fresh handle into this state
ROWS = [
    # B <= 4 n_cu: one instance per wavefront; every tile would hand over at once (base = 4 x 256 / tiles >= 64): k_solve_wg alone
    ("b256", LF30, 256, {}, {}, dict(path="wg", bx=8, hyb_bx=1, hand=64, n_ric=1, help=0, chunk=PIPE_CHUNK, mailbox=1, rescue=1, wg_grid=256)),
    ("b1024", LF30, 1024, {}, {}, dict(path="wg", hyb_bx=1, hand=64, n_ric=2, help=0, chunk=PIPE_CHUNK, mailbox=1, rescue=1, wg_grid=1024)),
    # two instances per wavefront beyond 4 n_cu; 2048 / 32 tiles = 64 still
    ("b2048", LF30, 2048, {}, {}, dict(path="wg", hyb_bx=2, hand=64, n_ric=4, help=0, chunk=PIPE_CHUNK, mailbox=1, rescue=1, wg_grid=1024)),
    # 33 tiles: base 62, but 33 x 512 <= 9/8 of the 2 x 1024 slots: alone still
    ("b2049", LF30, 2049, {}, {}, dict(path="wg", hyb_bx=2, hand=64, n_ric=5, help=0, chunk=PIPE_CHUNK, mailbox=1, rescue=1, wg_grid=1025)),
    # the headline: base 32 -> hand 3/2 x 32 = 48; 8 tiles per XCD, 8 Riccati workers; 8 items x 8 tiles <= 3 x 24 stage workers: no help
    ("b4096", LF30, 4096, {}, {}, dict(path="pipe", bx=8, hyb_bx=2, hand=48, n_ric=8, help=0, chunk=PIPE_CHUNK, mailbox=1, rescue=1, wg_grid=1536)),
    # base 16 -> 7/4 x 16 = 28; 16 tiles per XCD > 3/8 x 32: no worker per tile; 128 items > 72: the Riccati workers help
    ("b8192", LF30, 8192, {}, {}, dict(path="pipe", hyb_bx=2, hand=28, n_ric=8, help=1, chunk=PIPE_CHUNK, mailbox=1, rescue=1, wg_grid=1792)),
    ("b16384", LF30, 16384, {}, {}, dict(path="pipe", hyb_bx=2, hand=14, n_ric=8, help=1, chunk=PIPE_CHUNK, mailbox=1, rescue=1, wg_grid=1792)),
    # chunks of 256 tiles: the last one is a single instance
    ("b16385", LF30, 16385, {}, {}, dict(path="wg", hyb_bx=1, hand=64, n_ric=1, help=0, chunk=PIPE_CHUNK, mailbox=1, rescue=1, wg_grid=1)),
    # N = 50: 4 instances per 256-thread workgroup, one per wavefront (51 x 2 > 64); base 16 -> 28 -> at least 40; 16 items x 8 tiles > 72
    ("n50_b4096", "usalf_n50_nx5", 4096, {}, {}, dict(path="pipe", bx=4, hyb_bx=1, hand=40, n_ric=8, help=1, chunk=PIPE_CHUNK, mailbox=1, rescue=1,
                                                     wg_grid=2560)),
    # collision avoidance: the same path with a clean history and after stalled instances; the hint puts the second chance inside
    ("ca_b1024", "ca", 1024, {}, {}, dict(path="wg", hyb_bx=1, hand=64, n_ric=2, help=0, chunk=PIPE_CHUNK, mailbox=1, rescue=1, wg_resc=0)),
    ("ca_b1024_hint", "ca", 1024, {}, dict(resc_hint=1), dict(path="wg", hyb_bx=1, hand=64, n_ric=2, help=0, chunk=PIPE_CHUNK, mailbox=1, rescue=1,
                                                               wg_resc=1)),
    # ... and where the hint changes the instances per wavefront: 36 x 512 <= 18 x 1024 slots
    ("ca_b2304", "ca", 2304, {}, {}, dict(path="wg", hyb_bx=2, hand=64, n_ric=5, help=0, chunk=PIPE_CHUNK, mailbox=1, rescue=1, wg_resc=0)),
    ("ca_b2304_hint", "ca", 2304, {}, dict(resc_hint=1), dict(path="wg", hyb_bx=1, hand=64, n_ric=5, help=0, chunk=PIPE_CHUNK, mailbox=1, rescue=1,
                                                               wg_resc=1)),
    # option rescue_alone: k_solve_wg alone, one instance per wavefront, the second chance inside (up to 128 tiles)
    ("rescue_alone", LF30, 4096, {"rescue_alone": "1"}, {}, dict(path="wg", hyb_bx=1, hand=64, n_ric=8, help=0, chunk=PIPE_CHUNK, mailbox=1, rescue=1,
                                                                wg_resc=1, wg_grid=4096)),
    # a fixed iteration count: no hand-over, no mailbox, no second chance; the pipeline takes 64 tiles, the workspace limit sets the chunks
    ("fixed_iters", LF30, 4096, {"fixed_iters": 20}, {}, dict(path="pipe", hyb_bx=2, hand=0, n_ric=8, help=0, chunk=WS_CHUNK_N30, mailbox=0, rescue=0,
                                                             wg_grid=0)),
    # N = 64: 512-thread stage workgroups (4 x 65 > 256): one launch per kernel
    ("n64_b4096", "lf_n64_nx6", 4096, {}, {}, dict(path="kernels", bx=4, hyb_bx=1, hand=0, n_ric=8, help=0, chunk=WS_CHUNK_N64, mailbox=0, rescue=1)),
    # trace: one launch per kernel, no second chance
    ("trace", LF30, 256, {}, dict(trace=1), dict(path="kernels", hyb_bx=1, hand=0, n_ric=1, help=0, chunk=PIPE_CHUNK, mailbox=1, rescue=0)),
    # a level of the second chance: k_solve_wg alone, one instance per wavefront, whatever the hand-over threshold (40 here)
    ("in_rescue", LF30, 3000, {}, dict(in_rescue=1), dict(path="wg", hyb_bx=1, hand=40, n_ric=6, help=0, chunk=PIPE_CHUNK, mailbox=1, rescue=1,
                                                           wg_resc=0)),
    ("pipeline0", LF30, 4096, {"pipeline": "0"}, {}, dict(path="kernels", hyb_bx=2, hand=0, n_ric=8, help=0, chunk=WS_CHUNK_N30, mailbox=0, rescue=1)),
    ("hybrid0", LF30, 4096, {"hybrid": "0"}, {}, dict(path="pipe", hyb_bx=2, hand=0, n_ric=8, help=0, chunk=PIPE_CHUNK, mailbox=0, rescue=1,
                                                       wg_grid=0)),
    ("hybrid_live64", LF30, 4096, {"hybrid_live": "64"}, {}, dict(path="wg", hyb_bx=2, hand=64, n_ric=8, help=0, chunk=PIPE_CHUNK, mailbox=1,
                                                                   rescue=1, wg_grid=2048)),
    # one instance per wavefront pinned: base 16 -> 28 -> at least 40
    ("hybrid_bx1", LF30, 4096, {"hybrid_bx": "1"}, {}, dict(path="pipe", hyb_bx=1, hand=40, n_ric=8, help=0, chunk=PIPE_CHUNK, mailbox=1, rescue=1,
                                                             wg_grid=2560)),
    ("hybrid_bx2", LF30, 256, {"hybrid_bx": "2"}, {}, dict(path="wg", hyb_bx=2, hand=64, n_ric=1, help=0, chunk=PIPE_CHUNK, mailbox=1, rescue=1,
                                                            wg_grid=128)),
    # the general kernels: the helping Riccati workers only exist in the variant with the reference's bound structure compiled in
    ("bound_mask0", LF30, 8192, {"bound_mask": "0"}, {}, dict(path="pipe", hyb_bx=2, hand=28, n_ric=8, help=0, chunk=PIPE_CHUNK, mailbox=1, rescue=1,
                                                               masked=0)),
    # chunks of 3008 instances: the last one (1088, 17 tiles) runs in k_solve_wg alone
    ("max_batch", LF30, 4096, {"max_batch": "3000"}, {}, dict(path="wg", hyb_bx=2, hand=64, n_ric=3, help=0, chunk=3008, mailbox=1, rescue=1,
                                                               wg_grid=544)),
    # four XCDs: 16 tiles and 64 CUs each, 16 Riccati workers; 8 x 16 items <= 3 x 48: no help
    ("pipe_xcd_mask", LF30, 4096, {"pipe_xcd_mask": "0x0F"}, {}, dict(path="pipe", hyb_bx=2, hand=48, n_ric=16, help=0, chunk=PIPE_CHUNK, mailbox=1,
                                                                       rescue=1, n_xcd=4)),
]
GPU_ROWS = [r for r in ROWS if not (set(r[4]) & {"resc_hint", "in_rescue"})]


def bounds_of(fam):
    return [np.ascontiguousarray(a, dtype=np.float64) for a in BicycleNLP(CFGS[fam]).bounds()]


def plan(fam, B, opts, n_cu=N_CU, xcd_mask=XCD_MASK, ws_mailbox=-1, pipe_disabled=0, resc_hint=0, trace=0, in_rescue=0, async_loop=0, bounds=None,
         obst_mult=3):
    """emu_solve_plan for a handle of family `fam` (a name of CFGS, or an NLPConfig) with options `opts` (fixed_iters: the descriptor's);
    ws_mailbox -1 = a handle's first solve; bounds: (lbg, ubg, lbx, ubx) in place of the family's reference bounds"""
    L = emu_lib()
    if not getattr(L, "_plan_ready", False):
        L.emu_solve_plan.argtypes = [C.POINTER(abi.MpcProblemDesc)] + [C.POINTER(C.c_double)] * 4 + [C.POINTER(C.c_char_p)] * 2 + \
                                    [C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.emu_solve_plan.restype = C.c_int
        L._plan_ready = True
    opts = dict(opts)
    cfg = CFGS[fam] if isinstance(fam, str) else fam
    d = emu_desc(cfg, fixed_iters=int(opts.pop("fixed_iters", 0)), obst_mult=obst_mult)
    lbg, ubg, lbx, ubx = [np.ascontiguousarray(a, dtype=np.float64) for a in (BicycleNLP(cfg).bounds() if bounds is None else bounds)]
    names = (C.c_char_p * max(1, len(opts)))(*[k.encode() for k in opts])
    values = (C.c_char_p * max(1, len(opts)))(*[str(v).encode() for v in opts.values()])
    state = np.array([n_cu, xcd_mask, ws_mailbox, pipe_disabled, resc_hint, B, 0, trace, in_rescue, async_loop], np.int64)
    out = np.zeros(len(OUT), np.int64)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))      # noqa: E731
    rc = L.emu_solve_plan(C.byref(d), dp(lbx), dp(ubx), dp(lbg), dp(ubg), names, values, len(opts), state.ctypes.data_as(C.POINTER(C.c_int64)),
                          out.ctypes.data_as(C.POINTER(C.c_int64)))
    assert rc == 0
    r = dict(zip(OUT, (int(v) for v in out)))
    r["path"] = PATHS[r["path"]]
    return r


def last_chunk(fam, B, opts, **state):
    """the plan of a call's last chunk, and the chunk size"""
    chunk = plan(fam, B, opts, **state)["chunk"]
    b_last = B if B <= chunk else B - (B - 1) // chunk * chunk
    return plan(fam, b_last, opts, **state), chunk


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_plan_table(row):
    _, fam, B, opts, state, want = row
    p, chunk = last_chunk(fam, B, opts, **state)
    got = dict(p, chunk=chunk)
    print(row[0], {k: got[k] for k in want})
    assert {k: got[k] for k in want} == want


def test_plan_mailbox_as_the_workspace_has_it():
    """a handle whose workspace was allocated without the mailbox section cannot hand tiles over to k_solve_wg"""
    p = plan(LF30, 4096, {}, ws_mailbox=0)
    assert p["path"] == "pipe" and p["hand"] == 0 and p["mailbox"] == 1
    # ... a disabled pipeline (abandoned launches) leaves one launch per kernel, and no wish for the section
    p = plan(LF30, 4096, {}, pipe_disabled=1)
    assert p["path"] == "kernels" and p["mailbox"] == 0 and p["chunk"] == WS_CHUNK_N30


def test_plan_closed_loop_async():
    """the closed loop is enqueued without host synchronisation where the pipeline may run and the batch fits one chunk"""
    assert plan(LF30, 4096, {})["loop_async"] == 1
    assert plan(LF30, PIPE_CHUNK + 1, {})["loop_async"] == 0
    assert plan(LF30, 4096, {"loop_async": "0"})["loop_async"] == 0
    assert plan(LF30, 4096, {"fixed_iters": 20})["loop_async"] == 0
    assert plan(LF30, 4096, {}, pipe_disabled=1)["loop_async"] == 0


def test_plan_options_are_parsed_like_mpc_set_option():
    """the option table: "" sets a flag, "nlp" / "ipopt" for friction_lb, a mask in any base; an unknown name is refused"""
    assert plan(LF30, 4096, {"pipe_xcd_mask": "0x3"})["n_xcd"] == 2
    assert plan(LF30, 4096, {"pipeline": ""})["path"] == "pipe"
    assert plan(LF30, 4096, {"hybrid_live": "64", "rescue_alone": ""})["wg_resc"] == 0      # (rescue_alone needs hybrid_live < 0)
    assert plan(LF30, 4096, {"rescue_alone": ""})["wg_resc"] == 1
    assert plan(LF30, 4096, {"friction_lb": "ipopt"})["path"] == "pipe"
    with pytest.raises(AssertionError):
        plan(LF30, 4096, {"no_such_option": "1"})


# ---- behind the launch (after_solve): the second chance behind it, the hint for the handle's next solve --------------------------------
# (id, pl.rescue, outcome: failed, resc_ran, resc_in_kernel, rescued_in_kernel; expected: run_rescue, set_hint, hint -- None: not written).
# Read off solve_dev as it stood before the decision was extracted; a fix of ADVICE.md's findings about this region shows as a changed row.
AFTER_ROWS = [
    # every instance converged, none stalled on the way: nothing to do, the next solve needs no second chance inside its launch
    ("clean", 1, (0, 0, 0, 0), (0, 1, 0)),
    # instances left open and no second chance inside the launch: rescue_dev gives them their levels; the next solve takes the kernel that has it
    ("failed", 1, (3, 0, 0, 0), (1, 1, 1)),
    # k_solve_wg<.., RESC> alone over every instance: what is still open has had its levels -- rescue_dev would only repeat them
    ("failed_in_kernel", 1, (3, 1, 1, 5), (0, 1, 1)),
    # ... behind the pipeline it saw the handed-over instances only: one that stalled inside the pipeline is still rescue_dev's
    ("failed_behind_pipeline", 1, (2, 1, 0, 4), (1, 1, 1)),
    # all home, some through the second chance inside the launch: the family stalls, the hint stays
    ("rescued_in_kernel", 1, (0, 1, 1, 7), (0, 1, 1)),
    # no second chance for this solve (option rescue = 0, a fixed iteration count, a trace, no circle rows): the handle's hint is left alone
    ("no_rescue", 0, (3, 0, 0, 0), (0, 0, None)),
]


@pytest.mark.parametrize("row", AFTER_ROWS, ids=[r[0] for r in AFTER_ROWS])
def test_after_solve_table(row):
    _, rescue, outcome, want = row
    L = emu_lib()
    L.emu_after_solve.argtypes = [C.POINTER(C.c_int64)] * 2
    L.emu_after_solve.restype = None
    inp, out = np.array((rescue,) + outcome, np.int64), np.zeros(3, np.int64)
    L.emu_after_solve(inp.ctypes.data_as(C.POINTER(C.c_int64)), out.ctypes.data_as(C.POINTER(C.c_int64)))
    got = (int(out[0]), int(out[1]), int(out[2]) if out[1] else None)
    print(row[0], got)
    assert got == want


# ---- the GPU: what the library reports after one solve of each row on a fresh handle ----------------------------------------------------

def gpu_workers(p, n_cu):
    """Riccati and stage workers of a pipeline launch as k_pipeline counts them: n_cu workgroups dealt round-robin over the eight XCDs; on
    an XCD of the plan's set with t tiles, min(n_ric, t) sweep, the others take stage items; elsewhere they leave at once"""
    n_xcd = p["n_xcd"]
    ric = stage = 0
    for x in range(n_xcd):
        t = (p["ntiles"] - x + n_xcd - 1) // n_xcd if p["ntiles"] > x else 0
        if t:
            ric += min(p["n_ric"], t)
            stage += n_cu // 8 - min(p["n_ric"], t)
    return ric, stage


@pytest.mark.gpu
@pytest.mark.parametrize("row", GPU_ROWS, ids=[r[0] for r in GPU_ROWS])
def test_plan_is_what_the_library_runs(row):
    """one solve per row: the library's pipeline / resident profiles against emu_solve_plan for this device (collision avoidance with
    option rescue = 0: the levels of the second chance behind the launch would overwrite the resident profile).  Where k_solve_wg serves
    the batch alone, its counters in the control block are the caller's iteration counts: instance-rounds their sum, the rounds of the
    slowest workgroup their maximum"""
    import torch
    _, fam, B, opts, state, _ = row
    opts = dict(opts, **({"rescue": "0"} if fam == "ca" else {}))
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    p, chunk = last_chunk(fam, B, opts, n_cu=n_cu, xcd_mask=0xFF, **state)
    cfg = CFGS[fam]
    kw = dict(fixed_iters=int(opts["fixed_iters"])) if "fixed_iters" in opts else {}
    s = make_solver(cfg, **kw)
    set_cfg_bounds(s, cfg)
    for k, v in opts.items():
        if k != "fixed_iters":
            s.set_option(k, v)
    x0, p_ = ca_batch(cfg, B) if fam == "ca" else synthetic_batch(cfg, B, **FAMILIES.get(fam, (None, {}))[1])
    r = s.solve_trace(x0, p_)[0] if state.get("trace") else s.solve(x0, p_)
    pp, rp = s.get_pipeline_profile(), s.get_resident_profile()
    print(row[0], p, pp, rp, "rescued", s.last_rescued(), "status", np.unique(r.status))
    assert pp["ran"] == (p["path"] == "pipe")
    if pp["ran"]:
        assert (pp["riccati_workers"], pp["stage_workers"]) == gpu_workers(p, n_cu)
    assert rp["ran"] == (p["path"] == "wg" or (p["path"] == "pipe" and p["hand"] > 0))
    if rp["ran"]:
        assert rp["workgroups"] == p["wg_grid"]
    if p["path"] == "wg" and fam != "ca":
        # k_solve_wg alone: its counters against the iteration counts the caller gets (of the call's last chunk: what the profile describes)
        it = r.iters[(B - 1) // chunk * chunk:]
        print(row[0], "iters sum", int(it.sum()), "max", int(it.max()))
        assert rp["instance_iterations"] == int(it.sum())
        assert rp["rounds"] == int(it.max())
