"""The backward Riccati step as riccati_tile's two compute waves run it, on the CPU.

riccati_tile's backward sweep keeps the matrix recursion on wave 0 and gives the vector half (p_k, kff) to wave 2, which walks the same matrix
recursion; each wave stores its own row pairs.  Nothing is exchanged between them, so the result is the one of riccati_backward_step (which the
emulation harness and k_solve_wg's scalar fallbacks keep running) only if
  1. ric_matrix_step followed by ric_vector_step on a copy of the state leaves bit for bit the P_k, p_k, gains and kff of riccati_backward_step,
     and ric_matrix_step alone the same P_k and gains;
  2. ric_store_matrix and ric_store_vector together write exactly the rows ric_store_stage writes, the same bits, each row by one of them
     (a 16-byte row pair never by both -- the two waves' stores land in no defined order).
Harness: tests/ricsplitx/ricsplitx.cpp, built with g++ (helpers.harness_lib).  Everything is compared as bit patterns; the workspace images start as a NaN with a
payload no computation produces, so "written" is "no longer the sentinel".
"""
import ctypes as C

import numpy as np
import pytest

from helpers import harness_lib

SENTINEL = np.uint64(0x7FF8DEADBEEF1234)
N_HORIZON = 6


@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(harness_lib("ricsplitx"))
    dp = C.POINTER(C.c_double)
    L.ricsplit_image_doubles.restype = C.c_long
    L.ricsplit_row_index.restype = C.c_long
    L.ricsplit_run.argtypes = [C.c_int] * 7 + [dp] * 5
    return L


def stage_input(rng, nx, ne, k0, mark, delta, indefinite=False):
    """a random positive definite cost-to-go and a stage of the size the solver sees (weights 1e-1 .. 1e3, dt = 0.1); NE < NX: the
    decoupled progress state's row and column of P+ and H are the zeros the five-state recursion relies on"""
    n_in = 75
    v = np.zeros(n_in)
    v[0] = 0.1
    v[1] = delta
    if k0:
        v[2:4] = rng.normal(size=2)
    v[4] = 1.0 if mark else 0.0
    sidx = lambda i, j: i * nx - i * (i - 1) // 2 + (j - i)
    M = rng.normal(size=(ne, ne))
    Pm = np.zeros((nx, nx))
    Pm[:ne, :ne] = M @ M.T * 10.0 + np.diag(10.0 ** rng.uniform(-1, 3, ne))
    Hm = np.zeros((nx, nx))
    Hm[:ne, :ne] = np.diag(10.0 ** rng.uniform(-1, 3, ne))
    for (i, j) in ((0, 1), (0, 4), (1, 4), (2, 3), (3, 4)):
        Hm[i, j] = Hm[j, i] = rng.normal()
    for i in range(nx):
        for j in range(i, nx):
            v[5 + sidx(i, j)] = Pm[i, j]
            v[32 + sidx(i, j)] = Hm[i, j]
    v[26:26 + ne] = rng.normal(size=ne) * 10.0
    v[53:55] = (-1e6, -1e6) if indefinite else 10.0 ** rng.uniform(-1, 2, 2)
    v[55:61] = rng.normal(size=6) * 0.1
    v[61:61 + ne] = rng.normal(size=ne)
    v[67:69] = rng.normal(size=2)
    v[69:69 + ne] = rng.normal(size=ne) * 0.01
    return v


def run(L, nx, ne, sym, k, bb, terminal, vin):
    img = L.ricsplit_image_doubles(nx, N_HORIZON)
    ws = np.full(3 * img, SENTINEL, dtype=np.uint64).view(np.float64)
    outs = [np.zeros(42) for _ in range(3)]
    dp = C.POINTER(C.c_double)
    rc = L.ricsplit_run(nx, ne, int(sym), N_HORIZON, k, bb, int(terminal), vin.ctypes.data_as(dp), *[o.ctypes.data_as(dp) for o in outs], ws.ctypes.data_as(dp))
    assert rc == 0, rc
    return outs, ws.view(np.uint64).reshape(3, img)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def expected_rows(L, nx, k, bb):
    """{flat index in an image: (array, row)} of every row of stage k of instance bb"""
    rows = {}
    for pk in (0, 1):
        for e in range(L.ricsplit_rows(nx, pk)):
            rows[L.ricsplit_row_index(nx, N_HORIZON, pk, k, e, bb)] = ("PK" if pk else "KK", e)
    return rows


CASES = [(nx, ne, sym, k) for (nx, ne) in ((5, 5), (6, 6), (6, 5)) for sym in (False, True) for k in (0, 3)]


@pytest.mark.parametrize("nx,ne,sym,k", CASES)
def test_two_waves_leave_the_bits_of_the_single_step(lib, nx, ne, sym, k):
    rng = np.random.default_rng(1000 * nx + 100 * ne + 10 * sym + k)
    ns = nx * (nx + 1) // 2
    # (the compensated products of a marked lane and an inertia correction exist in the SYM instantiation only; the five-state recursion runs without delta)
    variants = [(False, 0.0)] + ([(True, 0.0)] + ([(True, 1e-4)] if ne == nx else []) if sym else [])
    for mark, delta in variants:
        for rep in range(4):
            vin = stage_input(rng, nx, ne, k == 0, mark, delta)
            (single, mat, vec), _ = run(lib, nx, ne, sym, k, 7, False, vin)
            assert single[0] == 1.0 and mat[0] == 1.0 and vec[0] == 1.0
            # the vector wave: everything
            assert np.array_equal(bits(vec[1:1 + ns]), bits(single[1:1 + ns])), "P_k"
            assert np.array_equal(bits(vec[22:22 + nx]), bits(single[22:22 + nx])), "p_k"
            # the matrix wave: P_k and the gain rows, p+ untouched
            assert np.array_equal(bits(mat[1:1 + ns]), bits(single[1:1 + ns])), "P_k (matrix wave)"
            assert np.array_equal(bits(mat[22:22 + nx]), bits(vin[26:26 + nx]))
            assert np.array_equal(bits(mat[28:40]), bits(vec[28:40])), "gain rows of the two waves"
            assert np.any(single[22:22 + ne] != vin[26:26 + ne]) and np.any(single[1:1 + ns] != vin[5:5 + ns])     # (the step did something)


@pytest.mark.parametrize("nx,ne,sym,k", CASES)
def test_store_halves_write_the_rows_of_the_single_store_each_once(lib, nx, ne, sym, k):
    rng = np.random.default_rng(7000 + 1000 * nx + 100 * ne + 10 * sym + k)
    ns, nkk = nx * (nx + 1) // 2, 2 * nx + 2
    for bb in (0, 7, 63):
        vin = stage_input(rng, nx, ne, k == 0, sym, 0.0)
        (single, mat, vec), img = run(lib, nx, ne, sym, k, bb, False, vin)
        w = [set(np.nonzero(img[q] != SENTINEL)[0].tolist()) for q in range(3)]
        rows = expected_rows(lib, nx, k, bb)
        assert w[0] == set(rows), "the single store writes the rows of stage k of this instance and nothing else"
        assert not (w[1] & w[2]), sorted(rows[i] for i in w[1] & w[2])
        assert (w[1] | w[2]) == w[0]
        for i in w[1]:
            assert img[1][i] == img[0][i], rows[i]
        for i in w[2]:
            assert img[2][i] == img[0][i], rows[i]
        # no 16-byte row pair is shared: the pairs (2q, 2q + 1) of an array are adjacent doubles
        pair = lambda i: (rows[i][0], rows[i][1] // 2)
        assert not ({pair(i) for i in w[1]} & {pair(i) for i in w[2]})
        # who writes what: the matrix wave the gain rows and the pairs of PK that hold only P_k; the vector wave every row with kff or p_k in it
        assert {rows[i] for i in w[1]} == {("KK", e) for e in range(2 * nx)} | {("PK", e) for e in range(ns & ~1)}
        assert {rows[i] for i in w[2]} == {("KK", 2 * nx), ("KK", 2 * nx + 1)} | {("PK", e) for e in range(ns & ~1, ns + nx)}
        # ... and the stored values are the registers' (gains, kff, P_k, p_k)
        kk = np.concatenate([vec[28:28 + nx], vec[34:34 + nx], vec[40:42]])
        pkv = np.concatenate([vec[1:1 + ns], vec[22:22 + nx]])
        for i, (arr, e) in rows.items():
            assert img[0][i] == bits(np.array([kk[e] if arr == "KK" else pkv[e]]))[0], (arr, e)
        assert nkk == lib.ricsplit_rows(nx, 0)


@pytest.mark.parametrize("nx", [5, 6])
def test_terminal_stage_is_stored_as_two_disjoint_sets_of_pairs(lib, nx):
    rng = np.random.default_rng(90 + nx)
    ns = nx * (nx + 1) // 2
    for delta in (0.0, 1e-4):
        vin = stage_input(rng, nx, nx, False, False, delta)
        (single, mat, vec), img = run(lib, nx, nx, True, N_HORIZON, 11, True, vin)
        w = [set(np.nonzero(img[q] != SENTINEL)[0].tolist()) for q in range(3)]
        rows = {i: r for i, r in expected_rows(lib, nx, N_HORIZON, 11).items() if r[0] == "PK"}
        assert w[0] == set(rows) and not (w[1] & w[2]) and (w[1] | w[2]) == w[0]
        assert all(img[1][i] == img[0][i] for i in w[1]) and all(img[2][i] == img[0][i] for i in w[2])
        assert {rows[i] for i in w[1]} == {("PK", e) for e in range(ns & ~1)}
        pkv = np.concatenate([single[1:1 + ns], single[22:22 + nx]])
        assert all(img[0][i] == bits(np.array([pkv[e]]))[0] for i, (_, e) in rows.items())


@pytest.mark.parametrize("nx,ne,sym", [(5, 5, False), (6, 6, True), (6, 5, False)])
def test_an_indefinite_stage_is_refused_by_both_waves_and_nothing_is_stored(lib, nx, ne, sym):
    rng = np.random.default_rng(5 + nx + ne)
    vin = stage_input(rng, nx, ne, False, False, 0.0, indefinite=True)
    (single, mat, vec), img = run(lib, nx, ne, sym, 2, 5, False, vin)
    assert single[0] == 0.0 and mat[0] == 0.0 and vec[0] == 0.0
    assert np.all(img == SENTINEL)
