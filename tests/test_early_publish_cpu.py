"""CPU: the two load batches of a stage item of k_pipeline (csrc/mpc_stage_math.h: phase_preload<.., STEP = false> + phase_preload_step), the
launch plan's lead (csrc/mpc_solve_plan.h: SolvePlan::pipe_lead, option pipe_early) and the step-ready words of the control block, through
tests/earlyx/earlyx.cpp built by g++.

A stage item that was published before the forward Riccati sweep of its tile ended issues every load that does not read the step, waits for
the sweep, and loads the step (P.DZ) behind it.  Checked here, for nx = 5 and 6, at stage 0, an interior stage and stage N, with the bounds
looked up at run time and with the reference's bound structure compiled in (REF_VM):
  * on a one-tile workspace image of random bit patterns the two batches + phase_premath leave every byte of Ctx and PreTmp as the one batch
    + phase_premath does;
  * the same with every row the forward sweep writes holding a NaN pattern while the early batch runs: the early batch reads none of them."""
import ctypes as C

import numpy as np
import pytest

from helpers import abi, emu_desc, harness_lib
from oracle.nlp_numpy import BicycleNLP, NLPConfig
from test_solve_plan import CFGS, LF30, N_CU, ROWS, XCD_MASK

N = 30
ST_RUNNING = 0


@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(harness_lib("earlyx"))
    L.earlyx_ws_doubles.restype = C.c_long
    L.earlyx_iws_words.restype = C.c_long
    L.earlyx_status_index.restype = C.c_long
    L.earlyx_dz_range.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_long), C.POINTER(C.c_long)]
    L.earlyx_run.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_char_p, C.c_char_p]
    L.earlyx_plan.argtypes = [C.POINTER(abi.MpcProblemDesc)] + [C.POINTER(C.c_double)] * 4 + [C.POINTER(C.c_char_p)] * 2 + \
                             [C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.earlyx_ctl_layout.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_int64)]
    L.earlyx_item.argtypes = [C.c_uint32] * 3 + [C.POINTER(C.c_uint32)]
    L.earlyx_item.restype = C.c_uint32
    return L


@pytest.fixture(scope="module")
def images(lib):
    """nx -> (double image, int32 image) of one tile: random BIT PATTERNS (NaNs, infinities and denormals among them); instance 3 is running"""
    out = {}
    for nx in (5, 6):
        rng = np.random.default_rng(1100 + nx)
        ws = rng.integers(0, 2**64, size=lib.earlyx_ws_doubles(nx, N), dtype=np.uint64).view(np.float64)
        iws = rng.integers(-2**31, 2**31, size=lib.earlyx_iws_words(nx, N), dtype=np.int64).astype(np.int32)
        iws[lib.earlyx_status_index(nx, N, 3)] = ST_RUNNING
        out[nx] = (ws, iws)
    return out


def run(lib, nx, masked, k, b, poison, ws, iws):
    n = lib.earlyx_out_bytes(nx)
    one, two = C.create_string_buffer(n), C.create_string_buffer(n)
    rc = lib.earlyx_run(nx, masked, N, k, b, poison, ws.ctypes.data_as(C.POINTER(C.c_double)), iws.ctypes.data_as(C.POINTER(C.c_int32)), one, two)
    assert rc == 0
    return one.raw, two.raw


@pytest.mark.parametrize("poison", [0, 1], ids=["step-there", "step-NaN-during-early-batch"])
@pytest.mark.parametrize("b", [3, 40], ids=["running", "any-status"])
@pytest.mark.parametrize("k", [0, 13, N])
@pytest.mark.parametrize("masked", [0, 1], ids=["runtime-bounds", "REF_VM"])
@pytest.mark.parametrize("nx", [5, 6])
def test_two_batches_leave_the_bits_of_one(lib, images, nx, masked, k, b, poison):
    ws, iws = images[nx]
    one, two = run(lib, nx, masked, k, b, poison, ws, iws)
    assert len(one) > 500
    assert one == two


def test_the_image_is_not_trivial(lib, images):
    """the comparison above would also hold for a harness that loads nothing: the step rows do reach the context (another image, other bytes)"""
    ws, iws = images[6]
    first, last = C.c_long(), C.c_long()
    lib.earlyx_dz_range(6, N, C.byref(first), C.byref(last))
    assert 0 < first.value < last.value <= len(ws)
    other = ws.copy()
    other[first.value:last.value] = 1.5
    assert run(lib, 6, 0, 13, 3, 1, ws, iws)[1] != run(lib, 6, 0, 13, 3, 1, other, iws)[1]


def lead(lib, cfg, B, opts):
    opts = dict(opts)
    d = emu_desc(cfg, fixed_iters=int(opts.pop("fixed_iters", 0)))
    lbg, ubg, lbx, ubx = [np.ascontiguousarray(a, dtype=np.float64) for a in BicycleNLP(cfg).bounds()]
    names = (C.c_char_p * max(1, len(opts)))(*[k.encode() for k in opts])
    values = (C.c_char_p * max(1, len(opts)))(*[str(v).encode() for v in opts.values()])
    state = np.array([N_CU, XCD_MASK, B], np.int64)
    out = np.zeros(3, np.int64)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))      # noqa: E731
    rc = lib.earlyx_plan(C.byref(d), dp(lbx), dp(ubx), dp(lbg), dp(ubg), names, values, len(opts), state.ctypes.data_as(C.POINTER(C.c_int64)),
                         out.ctypes.data_as(C.POINTER(C.c_int64)))
    assert rc == 0
    return dict(pipe=int(out[0]), help=int(out[1]), lead=int(out[2]))


PIPE_ROWS = [r for r in ROWS if r[5].get("path") == "pipe"]


@pytest.mark.parametrize("row", PIPE_ROWS, ids=[r[0] for r in PIPE_ROWS])
def test_lead_of_the_plan_table_rows_that_take_the_pipeline(lib, row):
    name, fam, B, opts, _, want = row
    p = lead(lib, CFGS[fam], B, opts)
    print(name, p)
    assert p["pipe"] == 1 and p["help"] == want["help"]
    horizon = CFGS[fam].N
    if "fixed_iters" in opts or want["help"]:
        assert p["lead"] == 0           # the stage workers are the bound already | a helper must never wait for another tile's sweep
    else:
        assert 0 < p["lead"] <= horizon
    # the option: off, and a lead of the caller's (clamped to the horizon; never with helping Riccati workers)
    assert lead(lib, CFGS[fam], B, dict(opts, pipe_early=0))["lead"] == 0
    assert lead(lib, CFGS[fam], B, dict(opts, pipe_early=7))["lead"] == (0 if want["help"] else 7)
    assert lead(lib, CFGS[fam], B, dict(opts, pipe_early=1000))["lead"] == (0 if want["help"] else horizon)


def test_lead_headline_and_short_horizon(lib):
    assert lead(lib, CFGS[LF30], 4096, {})["lead"] > 0
    assert lead(lib, CFGS[LF30], 256, {})["lead"] == 0                  # (k_solve_wg alone: no pipeline, no lead)
    short = NLPConfig(N=2, nx=5)
    p = lead(lib, short, 4096, {"hybrid": "0"})
    assert p["pipe"] == 1 and p["lead"] == 2                            # a horizon shorter than the default lead: published at stage 0
    assert lead(lib, short, 4096, {"hybrid": "0", "pipe_early": 30})["lead"] == 2


@pytest.mark.parametrize("ntiles,cap", [(1, 16), (64, 128), (65, 256), (256, 1024)])
def test_control_block_layout(lib, ntiles, cap):
    out = (C.c_int64 * 4)()
    lib.earlyx_ctl_layout(ntiles, cap, out)
    words, slots, step, hdr = (int(v) for v in out)
    # [8 XCD records of 64 words | head of 32 | stage_done[ntiles] | pad | slots: 8 XCDs x cap uint64 | step_ready[ntiles] | pad]
    assert hdr == 8 * 64 + 32
    assert slots == (hdr + ntiles + 1) // 2 * 2                         # (where the queue stood before the step-ready words were added)
    assert step == slots + 16 * cap                                     # behind everything that was there
    assert words == step + (ntiles + 1) // 2 * 2 and words % 2 == 0


def test_slot_payload_round_trips(lib):
    out = (C.c_uint32 * 3)()
    for tile, q, rnd in [(0, 0, 1), (255, 15, 0xFFFF), (63, 7, 0x12345)]:
        it = lib.earlyx_item(tile, q, rnd, out)
        assert (out[0], out[1], out[2]) == (tile, q, rnd & 0xFFFF)
        assert it != 0xFFFFFFFF                                         # (PIPE_EXIT: no item)
