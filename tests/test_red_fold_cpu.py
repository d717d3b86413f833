"""The order of the stage phases' reductions, on the CPU (harness tests/redfold/redfold.cpp).

block_reduce (csrc/mpcgpu.hip) -- the xor butterfly over the lanes of a wavefront, then the pass through LDS over the wavefronts -- is
emulated literally for every thread of the workgroup and compared bit for bit with red_fold (csrc/mpc_red_fold.h), the same association
order as plain C++, and with red_fold_field, the unrolled per-field form that the transposed reduction (block_reduce_t) runs on one lane
per (field, instance column).

What is compared:
  * the lane of stage 0 of every column against red_fold, and red_fold_field against red_fold: the same bits on every input -- the three
    perform the same combines with the same operands in the same order;
  * every OTHER thread of the workgroup against red_fold: the same bits as well; this rests on `+`, fmin and fmax being commutative bit for
    bit (the other lanes run the tree with operands exchanged).  The one place where a host libm may not be -- fmin / fmax of two zeros of
    opposite sign, where the device's v_min_f64 / v_max_f64 are -- is the family "zeros": there the other threads are held to the same
    VALUE in the min / max fields (a zero of either sign), to the same bits everywhere else.
"""
import ctypes as C

import numpy as np
import pytest

from helpers import harness_lib

NQ = {0: 1, 1: 3, 2: 4, 3: 10}
SUM, MIN, MAX = 0, 1, 2
STAGES = (2, 3, 31, 32, 64)            # N = 1, 2, 30, 31, 63
FAMILIES = ("random", "magnitudes", "zeros", "nan", "idle")


@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(harness_lib("redfold"))
    dp = C.POINTER(C.c_double)
    L.redfold_run.argtypes = [C.c_int, dp, C.c_int, C.c_int, C.c_int, dp, dp, dp]
    L.redfold_neutral.argtypes = [C.c_int, dp]
    for which, nq in NQ.items():
        assert L.redfold_nq(which) == nq
    return L


def neutral(lib, which):
    out = np.zeros(NQ[which])
    lib.redfold_neutral(which, out.ctypes.data_as(C.POINTER(C.c_double)))
    return out


def kinds(lib, which):
    return [lib.redfold_kind(which, q) for q in range(NQ[which])]


def test_kinds_and_neutral_elements_match_red_combine(lib):
    """red_kind (the per-field view) against red_combine itself: two leaves per field, chosen so that the three operators give three
    different results; and the neutral element of a field is neutral for the field's operator."""
    for which, nq in NQ.items():
        ks, ne = kinds(lib, which), neutral(lib, which)
        vals = np.tile(ne, (64, 1))
        vals[0], vals[1] = 0.75, 0.5                     # a + b = 1.25, min 0.5, max 0.75; stages 0 and 1 of column 0 (bx = 1)
        emu, fold, field = run(lib, which, vals, 1, 1, 2)
        for q in range(nq):
            want = {SUM: 1.25, MIN: 0.5, MAX: 0.75}[ks[q]]
            assert fold[0, q] == want == field[0, q], (which, q, ks[q], fold[0, q], field[0, q])
            assert {SUM: 0.0, MIN: 1.0, MAX: 0.0}[ks[q]] == ne[q] or abs(ne[q]) > 1e30, (which, q)


def run(lib, which, vals, bx, nw, n_real):
    nq = NQ[which]
    vals = np.ascontiguousarray(vals, dtype=np.float64)
    assert vals.shape == (nw * 64, nq)
    dp = C.POINTER(C.c_double)
    emu, fold, field = np.zeros((nw * 64, nq)), np.zeros((bx, nq)), np.zeros((bx, nq))
    rc = lib.redfold_run(which, vals.ctypes.data_as(dp), bx, nw, n_real, emu.ctypes.data_as(dp), fold.ctypes.data_as(dp), field.ctypes.data_as(dp))
    assert rc == 0, rc
    return emu, fold, field


def leaves(rng, family, which, ks, ne, bx, nw, S):
    """[nw * 64][NQ] by thread: thread t is stage t // bx of column t % bx; stages >= S carry the neutral record"""
    nq, T = NQ[which], nw * 64
    real = (np.arange(T) // bx) < S
    if family == "random":
        v = rng.standard_normal((T, nq))
    elif family in ("magnitudes", "nan", "idle"):
        # spread over 1e-300 .. 1e300, both signs: every association of a sum rounds differently, and a wrong pairing of min / max shows
        v = rng.choice([-1.0, 1.0], (T, nq)) * 10.0 ** rng.uniform(-300.0, 300.0, (T, nq))
        # (sums of a few hundred of these stay finite: the largest is below 1e300 and there are at most 512 of them)
        v[:, [q for q in range(nq) if ks[q] == SUM]] *= 1e-3
    else:       # zeros: the min / max fields hold zeros of both signs -- whole columns of them, and among other values
        v = rng.standard_normal((T, nq))
        for q in range(nq):
            if ks[q] != SUM:
                z = rng.choice([0.0, -0.0], T)
                if rng.integers(2):
                    v[:, q] = z
                else:
                    sel = rng.random(T) < 0.5
                    v[sel, q] = z[sel]
                    v[~sel, q] = np.abs(v[~sel, q]) * (1.0 if ks[q] == MIN else -1.0)        # the zeros decide the result
    if family == "nan" and which == 3:
        t = int(rng.choice(np.flatnonzero(real)))
        v[:, 9] = rng.choice([0.0, 1.0], T)
        v[t, 9] = np.nan                                                   # one NaN in Red3::nan
    if family == "idle":
        # neutral records inside the horizon as well: a whole column that is not iterating, and single stage threads
        if bx > 1:
            v[(np.arange(T) % bx) == int(rng.integers(bx))] = ne
        v[rng.random(T) < 0.2] = ne
    v[~real] = ne
    return v


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


CASES = [(which, bx, S) for which in NQ for bx in (1, 2, 4, 8) for S in STAGES]


@pytest.mark.parametrize("family", FAMILIES)
def test_butterfly_equals_red_fold_bit_for_bit(lib, family):
    rng = np.random.default_rng(["random", "magnitudes", "zeros", "nan", "idle"].index(family) + 17)
    n_checked = 0
    for which, bx, S in CASES:
        ks, ne = kinds(lib, which), neutral(lib, which)
        minmax = [q for q in range(NQ[which]) if ks[q] != SUM]
        nw_min = (S * bx + 63) // 64                                       # the workgroup the plan gives these stages ...
        for nw in sorted({nw_min, max(nw_min, 2), max(nw_min, 4)}):       # ... and larger ones: wavefronts of padding threads only
            for rep in range(3):
                v = leaves(rng, family, which, ks, ne, bx, nw, S)
                emu, fold, field = run(lib, which, v, bx, nw, S)
                tag = (family, which, bx, S, nw, rep)
                assert np.array_equal(bits(field), bits(fold)), tag
                assert np.array_equal(bits(emu[:bx]), bits(fold)), tag               # the lanes of stage 0: threads 0 .. bx - 1
                want = np.tile(fold, (nw * 64 // bx, 1))                             # thread t: column t % bx
                if family == "zeros":
                    same = bits(emu) == bits(want)
                    zero = (emu == 0.0) & (want == 0.0)
                    ok = same.copy()
                    ok[:, minmax] |= zero[:, minmax]
                    assert ok.all(), tag
                else:
                    assert np.array_equal(bits(emu), bits(want)), tag
                n_checked += 1
    assert n_checked >= 3 * len(CASES)


def test_association_order_matters_on_these_inputs(lib):
    """the inputs do tell the orders apart: a left-to-right sum of the same leaves differs from the tree in many sum fields (family "random";
    with magnitudes spread over 600 decades the largest leaf alone decides most sums, and only a few per cent of them differ)"""
    rng = np.random.default_rng(5)
    ks, ne = kinds(lib, 3), neutral(lib, 3)
    differ = 0
    for rep in range(20):
        v = leaves(rng, "random", 3, ks, ne, 2, 1, 31)
        _, fold, _ = run(lib, 3, v, 2, 1, 31)
        for bl in range(2):
            col = v[bl::2]
            for q in range(4, 9):
                acc = 0.0
                for x in col[:, q]:
                    acc += x
                differ += acc != fold[bl, q]
    assert differ >= 20, differ
