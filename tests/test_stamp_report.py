"""The stamp reports of option timing (csrc/mpc_stamps.h): the text the library prints to stderr -- labels, order, punctuation, number
formats; tools/*_timing.py read it -- from synthetic stamp rows, on the CPU through the emulation harness (tests/emu: emu_stamp_report).

A report averages the ticks between consecutive slots of its order over the workgroups that ran.  Two rows per report: the slot at
position j of the order holds 1000 + 100 j in the first and 1000 + 300 j in the second, so every span between neighbours has mean 200;
a third row lacks the slot that says "ran" and must not be counted.  The expected lines are written out from the label lists the
reports had when they were functions of mpcgpu.hip."""
import ctypes as C

import numpy as np

from helpers import emu_lib

START, WG, PIPE, STAGE, WG_TRACE = range(5)


def report(which, rows, n, n2=0):
    L = emu_lib()
    L.emu_stamp_report.argtypes = [C.c_int32, C.POINTER(C.c_uint64), C.c_int32, C.c_int32, C.c_char_p, C.c_int32]
    L.emu_stamp_report.restype = C.c_int
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    buf = C.create_string_buffer(8192)
    n_out = L.emu_stamp_report(which, rows.ctypes.data_as(C.POINTER(C.c_uint64)), n, n2, buf, len(buf))
    assert n_out >= 0
    return buf.value.decode()


def row(order, step, width=16):
    r = np.zeros(width, np.uint64)
    for j, slot in enumerate(order):
        r[slot] = 1000 + step * j
    return r


def rows_of(order, lacking):
    """the two rows, and between them one without the slot `lacking`"""
    skipped = row(order, 100)
    skipped[lacking] = 0
    return np.concatenate([row(order, 100), skipped, row(order, 300)])


START_ORDER = [11, 12, 13, 1, 2, 3, 4, 5, 6, 14, 15, 0, 7, 8, 9, 10]
START_SPANS = ("rows->LDS={0} Z/REF stores={0} bounds+a0={0} defects={0} scan1={0} tan+scan2={0} sincos+scan3={0} ROLL+sums={0} decide={0} fence={0} "
               "enter={0} init point+exchange={0} eval+assemble={0} reduce={0} finish={0}")


def test_start_timing():
    got = report(START, np.concatenate([row(START_ORDER, 100), row(START_ORDER, 300)]), 2)
    # first start: slot 11 = 1000 in both rows; last end: slot 10 = 1000 + 300 x 15
    assert got == "[mpcgpu k_start timing, shader-clock ticks, mean over 2 workgroups] " + START_SPANS.format(200) + "; first start to last end 4500\n"


def test_start_timing_counts_every_workgroup():
    """every workgroup of k_start stamps every slot: the report has no "ran" slot and divides by the grid -- a row of zeros is averaged in
    (400 / 3) and is the first start"""
    got = report(START, np.concatenate([row(START_ORDER, 100), np.zeros(16, np.uint64), row(START_ORDER, 300)]), 3)
    assert got == "[mpcgpu k_start timing, shader-clock ticks, mean over 3 workgroups] " + START_SPANS.format(133) + "; first start to last end 5500\n"


def test_wg_timing():
    order = [12, 13, 14, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 15]
    want = ("[mpcgpu k_solve_wg timing, shader-clock ticks, third round of 2 workgroups] records=200 sweeps=200 enter=200 load+premath=200 or=200 P1=200 "
            "reduce1+ls-begin=200 linesearch=200 P3-update=200 exchange=200 P4-eval=200 reduce3=200 P5=200 drain=200\n")
    assert report(WG, rows_of(order, 15), 3) == want          # (a workgroup without a third round)
    assert report(WG, rows_of(order, 10), 3) == want          # (... or whose instances had all finished before its stage phases)


def test_pipe_timing():
    stage = [11, 12, 13, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 14, 15]
    # a Riccati worker's pass: wait 11 -> 12, backward -> 1, forward -> 2, publish -> 13; stage 15 of the backward sweep 3 -> 4 -> 5, of the
    # forward sweep 6 -> 7 -> 8; slot 9 (the forward sweep's first stage) nine positions behind slot 1: 9 x 200
    ric = [11, 12, 1, 2, 13, 3, 4, 5, 6, 7, 8, 9]
    # (a row that is neither: no slot 15 -- not a stage worker's -- and no slot 2 -- no pass of a Riccati worker either)
    rows = np.concatenate([row(stage, 100), row(stage, 300), rows_of(ric, 2)])
    assert report(PIPE, rows, 5) == (
        "[mpcgpu pipeline timing, shader-clock ticks, last item of 2 stage workers] dequeue=200 acquire+bcast=200 enter=200 issue-loads=200 "
        "wait+barrier=200 P1=200 reduce1=200 linesearch=200 P3-update=200 exchange=200 P4-eval=200 reduce3=200 P5=200 drain=200 signal=200\n"
        "[last pass of 2 Riccati workers] wait=200 backward=200 forward=200 publish=200; stage 15 of the backward sweep: barrier=200 step=200, "
        "of the forward sweep: barrier=200 step=200, its first stage starts 1800 ticks after the backward sweep\n")


def test_stage_timing():
    """one launch per kernel: six blocks, of which two ran (the third has no slot 10); the Riccati kernel's rows start at word 8 x 6 of the
    same buffer, one per tile: tile 0, a tile that did not run (no slot 2), tile 2 -- a fourth would lie beyond the buffer"""
    block, tile = list(range(11)), list(range(9))
    rows = np.concatenate([rows_of(block, 10), rows_of(tile, 2)])
    want = ("[mpcgpu stage timing, shader-clock ticks per block, mean over 2 blocks] issue-loads=200 wait+barrier=200 P1=200 reduce1=200 linesearch=200 "
            "P3-update=200 exchange=200 P4-eval=200 reduce3=200 P5=200\n"
            "[riccati stage 15 of tile 0] bwd barrier-wait=100 compute=100 | fwd barrier-wait=100 compute=100\n"
            "[mpcgpu riccati timing, ticks per workgroup, mean over 2] backward=200 forward=200\n")
    assert report(STAGE, rows, 6, 3) == want
    assert report(STAGE, rows, 6, 4) == want


def test_wg_trace():
    """rows of four words: start, end (100 MHz ticks), rounds, instance-rounds (low 16 bits; the take-over and first-round times above them
    are zero here); a workgroup without rounds is not listed; the last to finish comes first"""
    rows = rows_of([0, 1, 2, 3], 2).reshape(3, 16)[:, :4]
    line = ("    workgroup {:5d}: start    0.0 us  end {:6.1f} us  rounds {}  instance-rounds {}  -> 0.0 us per round; instances taken over after 0.0 us, "
            "first round done after 0.0 us, later rounds 0.0 us each\n")
    assert report(WG_TRACE, rows, 3) == (
        "[mpcgpu wg_trace] 2 workgroups with work of 3; span 3.0 us; 0 of them start more than 5 us after the first (latest start 0.0 us); "
        "the last to finish:\n" + line.format(2, 3.0, 1600, 1900) + line.format(0, 1.0, 1200, 1300))
