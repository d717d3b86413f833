"""CPU: the linearised closed loop (mpc_closed_loop_batch_lin, mpc_loop_tangent, mpc_loop_adjoint) without a GPU.

tests/loop_lin_ref.py is the numpy chained reference (the oracle loop, the active-set derivatives of every step, the recursions); it is held to
central differences of the oracle loop here.  tests/looplinx/looplinx.cpp runs the kernels' bodies -- the emulated solve, loop_gain_family, the
sweep lanes -- on the CPU against it."""
import ctypes as C
import os

import numpy as np
import pytest

import loop_lin_ref as ref
import loop_obst_ref as obst_ref
from helpers import ROOT, BicycleNLP, abi, emu_desc, harness_lib, pkg

_dp, _ip = abi.as_dp, abi.as_ip
NEW = ["mpc_closed_loop_batch_lin", "mpc_closed_loop_batch_lin_dev", "mpc_loop_tangent", "mpc_loop_tangent_dev", "mpc_loop_adjoint", "mpc_loop_adjoint_dev"]
SCENES = [("LF", i) for i in range(len(ref.LF_SCENES))] + [("OB", i) for i in range(len(ref.OB_SCENES))]


# ---- 1: the C-ABI ------------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_declared_exported_prototyped_and_present():
    hdr = open(os.path.join(ROOT, "include", "mpcgpu.h")).read()
    L = C.CDLL(abi.LIB_PATH)
    for s in NEW:
        assert s in abi.EXPORTS and s in abi.PROTOTYPES and hasattr(L, s) and ("int " + s + "(") in hdr, s
    n = {s: len(abi.PROTOTYPES[s]) for s in NEW}
    assert n["mpc_closed_loop_batch_lin"] == len(abi.PROTOTYPES["mpc_closed_loop_batch_obst"]) + 3
    assert n["mpc_closed_loop_batch_lin_dev"] == n["mpc_closed_loop_batch_lin"] + 1
    assert (n["mpc_loop_tangent"], n["mpc_loop_tangent_dev"], n["mpc_loop_adjoint"], n["mpc_loop_adjoint_dev"]) == (15, 16, 14, 15)


# ---- 2: the reference against central differences of the oracle loop -----------------------------------------------------------------------
@pytest.mark.parametrize("kind,index", SCENES)
def test_reference_against_finite_differences(kind, index):
    """every unit direction (5 of the initial state, 7 of the weights, with a track 3 of the pose): the chained tangent against central
    differences of the oracle loop, max|delta| / max|FD| <= TOL_FD over (traj | ctrl).  Worst measured: LF 8.6e-7, OB 1.8e-5."""
    scene, run, gains = ref.reference(kind, index)
    assert np.all(run["status"] == 1)
    skipped, worst = 0, 0.0
    for d in ref.directions(scene):
        fd = ref.fd_direction(scene, d)
        if np.abs(fd).max() < ref.FD_FLOOR:
            skipped += 1
            continue
        err = ref.rel_err(ref.ref_direction(scene, run, gains, d), fd)
        worst = max(worst, err)
        assert err <= ref.TOL_FD, (d[0], err)
    print(f"\n  {kind} {index}: worst max|ref - FD| / max|FD| {worst:.2e} over {len(ref.directions(scene)) - skipped} directions, {skipped} skipped")
    assert skipped <= ref.MAX_SKIPPED


def test_reverse_sweep_is_the_transpose_of_the_forward_one():
    scene, run, gains = ref.reference("OB", 4)
    cfg, rng = scene.cfg, np.random.default_rng(3)
    st, sc = rng.normal(size=(scene.L, 5)), rng.normal(size=(scene.L, 2))
    gi, gw, gt = ref.adjoint(run["traj"], gains["kgain"], gains["wgain"], gains["ogain"], scene.L, st, sc, cfg.dt, cfg.wheelbase)
    for _, dinit, dwt, dtrack in ref.directions(scene):
        dtraj, dctrl = ref.tangent(run["traj"], gains["kgain"], gains["wgain"], gains["ogain"], scene.L, dinit, dwt, dtrack, cfg.dt, cfg.wheelbase)
        lhs = np.sum(st * dtraj) + np.sum(sc * dctrl)
        rhs = gi @ dinit + gw @ dwt + (0.0 if dtrack is None else np.sum(gt * dtrack))
        assert abs(lhs - rhs) <= 1e-12 * max(1.0, np.sum(np.abs(st * dtraj)) + np.sum(np.abs(sc * dctrl)))


# ---- 3: the kernels' bodies on the CPU -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def looplinx():
    L = C.CDLL(harness_lib("looplinx"))
    dp, ip, i32, f64 = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_int32, C.c_double
    L.looplinx_loop.argtypes = [C.POINTER(abi.MpcProblemDesc)] + [dp] * 4 + [i32] * 3 + [dp] * 4 + [i32, dp, f64, dp, dp, ip, dp, dp, dp]
    L.looplinx_loop.restype = C.c_int
    L.looplinx_tangent.argtypes = [f64, f64, i32, i32, i32] + [dp] * 4 + [i32] + [dp] * 5
    L.looplinx_adjoint.argtypes = [f64, f64, i32, i32] + [dp] * 4 + [i32] + [dp] * 5
    L.looplinx_tangent.restype = L.looplinx_adjoint.restype = None
    return L


def harness_loop(looplinx, scenes, nx=5):
    """the emulated lin loop of a batch of scenes of one kind: dict(traj, ctrl, status, kgain, wgain, ogain | None)"""
    cfg = scenes[0].cfg if nx == 5 else ref.dataclasses.replace(scenes[0].cfg, nx=nx)
    init, path, orient, vdes, track = ref.batch_inputs(scenes)
    B, L = len(scenes), scenes[0].L
    lbg, ubg, lbx, ubx = [np.ascontiguousarray(a, dtype=np.float64) for a in BicycleNLP(cfg).bounds()]
    out = dict(traj=np.zeros((B, L, 5)), ctrl=np.zeros((B, L, 2)), status=np.zeros((B, L), np.int32), kgain=np.zeros((B, L, 2, 5)),
               wgain=np.zeros((B, L, 2, 7)), ogain=None if track is None else np.zeros((B, L, 2, 3)))
    d = emu_desc(cfg)
    rc = looplinx.looplinx_loop(C.byref(d), _dp(lbx), _dp(ubx), _dp(lbg), _dp(ubg), B, L, L, _dp(init), _dp(path), _dp(orient), _dp(vdes),
                                0 if track is None else track.shape[1], _dp(track), obst_ref.OFFSET, _dp(out["traj"]), _dp(out["ctrl"]), _ip(out["status"]),
                                _dp(out["kgain"]), _dp(out["wgain"]), _dp(out["ogain"]))
    assert rc == 0
    return out


@pytest.mark.parametrize("kind", ["LF", "OB"])
def test_harness_against_reference(looplinx, kind):
    """emu_solve.h + loop_gain_family + the sweep lanes: the rollout equals the oracle's to the solves' tolerance, the per-step gains are within the
    per-family bounds of the reference, and the tangent over the whole loop within TOL_LOOP.
    Measured: see HARNESS_WORST_LOOP in tests/loop_lin_ref.py."""
    scenes = ref.LF_SCENES if kind == "LF" else ref.OB_SCENES
    got = harness_loop(looplinx, scenes)
    assert np.all(got["status"] == 1)
    runs = [ref.reference(kind, b)[1] for b in range(len(scenes))]
    assert np.abs(got["traj"] - np.array([r["traj"] for r in runs])).max() <= 1e-6
    worst, n_weak = ref.gain_errors(scenes, kind, got)
    cfg = scenes[0].cfg

    def sweep(b, dinit, dwt, dtrack):                       # (loop_tangent_lane on the harness's own rollout and gains)
        L = scenes[b].L
        c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)      # noqa: E731
        dtraj, dctrl = np.zeros((L, 5)), np.zeros((L, 2))
        looplinx.looplinx_tangent(cfg.dt, cfg.wheelbase, 1, L, 1, _dp(c(got["traj"][b])), _dp(c(got["kgain"][b])), _dp(c(got["wgain"][b])),
                                  _dp(None if got["ogain"] is None else c(got["ogain"][b])), 0 if dtrack is None else L, _dp(c(dinit)), _dp(c(dwt)), _dp(c(dtrack)),
                                  _dp(dtraj), _dp(dctrl))
        return dtraj, dctrl

    loop = ref.tangent_errors(scenes, kind, sweep)
    print(f"\n  {kind}: gains vs reference, worst k {worst['k']:.2e} (bound {ref.TOL_K:.0e}) w {worst['w']:.2e} (bound {ref.TOL_W:.0e}) o {worst['o']:.2e} "
          f"(bound {ref.TOL_O:.0e}), {n_weak} weakly active steps excluded; tangent over the loop {loop:.2e} (bound {ref.TOL_LOOP:.1e})")
    assert worst["k"] <= ref.TOL_K and worst["w"] <= ref.TOL_W and worst["o"] <= ref.TOL_O
    assert loop <= ref.TOL_LOOP


def test_harness_step_zero_sums_the_reference_columns(looplinx):
    """at step 0 p = tile(current_state): kgain[0] is the gradient summed over all N + 1 columns of X_ref, at the later steps the pin column alone --
    the two differ on the reference, so the comparison above tells them apart"""
    scene, run, g = ref.reference("LF", 0)
    K_pin = ref.step_gains(scene.cfg, run["w"][0], run["p"][0], False)[0]
    assert np.abs(K_pin - g["kgain"][0]).max() > 1e-3 * np.abs(g["kgain"][0]).max()


# ---- 4: the sweeps on random gains ---------------------------------------------------------------------------------------------------------
B4, L4, ND4, DT4, WB4 = 7, 5, 3, 0.1, 2.578


def random_loop(Lt, seed):
    rng = np.random.default_rng(seed)
    c = np.ascontiguousarray
    traj = c(np.stack([rng.uniform(-5, 5, (B4, L4)), rng.uniform(-5, 5, (B4, L4)), rng.uniform(-0.5, 0.5, (B4, L4)), rng.uniform(2, 12, (B4, L4)),
                       rng.uniform(-1, 1, (B4, L4))], axis=2))
    return dict(traj=traj, kgain=c(rng.normal(size=(B4, L4, 2, 5))), wgain=c(rng.normal(size=(B4, L4, 2, 7))), ogain=c(rng.normal(size=(B4, L4, 2, 3))),
                dinit=c(rng.normal(size=(B4, ND4, 5))), dwt=c(rng.normal(size=(B4, ND4, 7))), dtrack=c(rng.normal(size=(B4, ND4, Lt, 3))),
                seed_traj=c(rng.normal(size=(B4, L4, 5))), seed_ctrl=c(rng.normal(size=(B4, L4, 2))))


def run_tangent(looplinx, r, Lt, dinit, dwt, dtrack, kgain="kgain", wgain="wgain", ogain="ogain"):
    dtraj, dctrl = np.full((B4, ND4, L4, 5), 7.0), np.full((B4, ND4, L4, 2), 7.0)
    looplinx.looplinx_tangent(DT4, WB4, B4, L4, ND4, _dp(r["traj"]), _dp(r.get(kgain)), _dp(r.get(wgain)), _dp(r.get(ogain)), Lt, _dp(dinit), _dp(dwt), _dp(dtrack),
                              _dp(dtraj), _dp(dctrl))
    return dtraj, dctrl


def run_adjoint(looplinx, r, Lt, seed_traj, seed_ctrl, want_track=True):
    gi, gw, gt = np.full((B4, 5), 7.0), np.full((B4, 7), 7.0), np.full((B4, Lt, 3), 7.0)
    looplinx.looplinx_adjoint(DT4, WB4, B4, L4, _dp(r["traj"]), _dp(r["kgain"]), _dp(r["wgain"]), _dp(r["ogain"]), Lt, _dp(seed_traj), _dp(seed_ctrl), _dp(gi),
                              _dp(gw), _dp(gt) if want_track else None)
    return gi, gw, gt


@pytest.mark.parametrize("Lt", [1, L4, L4 + 3])
def test_sweeps_on_random_gains(looplinx, Lt):
    """loop_tangent_lane / loop_adjoint_lane against the numpy recursion, within 1e-13 of the sum of the absolute terms of every entry; the adjoint
    identity <seed, tangent> = <adjoint, direction> to the same bound; a null argument behaves as zero"""
    r = random_loop(Lt, 40 + Lt)
    dtraj, dctrl = run_tangent(looplinx, r, Lt, r["dinit"], r["dwt"], r["dtrack"])
    gi, gw, gt = run_adjoint(looplinx, r, Lt, r["seed_traj"], r["seed_ctrl"])
    for b in range(B4):
        a = (r["traj"][b], r["kgain"][b], r["wgain"][b], r["ogain"][b], Lt)
        for d in range(ND4):
            want = ref.tangent(*a, r["dinit"][b, d], r["dwt"][b, d], r["dtrack"][b, d], DT4, WB4)
            mag = ref.tangent(*a, r["dinit"][b, d], r["dwt"][b, d], r["dtrack"][b, d], DT4, WB4, mag=True)
            assert np.all(np.abs(dtraj[b, d] - want[0]) <= 1e-13 * mag[0]) and np.all(np.abs(dctrl[b, d] - want[1]) <= 1e-13 * mag[1])
            lhs = np.sum(r["seed_traj"][b] * dtraj[b, d]) + np.sum(r["seed_ctrl"][b] * dctrl[b, d])
            rhs = gi[b] @ r["dinit"][b, d] + gw[b] @ r["dwt"][b, d] + np.sum(gt[b] * r["dtrack"][b, d])
            terms = np.sum(np.abs(r["seed_traj"][b]) * mag[0]) + np.sum(np.abs(r["seed_ctrl"][b]) * mag[1])
            assert abs(lhs - rhs) <= 1e-13 * terms, (b, d, lhs, rhs)
        want = ref.adjoint(*a, r["seed_traj"][b], r["seed_ctrl"][b], DT4, WB4)
        mag = ref.adjoint(*a, r["seed_traj"][b], r["seed_ctrl"][b], DT4, WB4, mag=True)
        for got, w_, m_ in zip((gi[b], gw[b], gt[b]), want, mag):
            assert np.all(np.abs(got - w_) <= 1e-13 * m_)
    # null arguments are zero
    z = {k: np.zeros_like(r[k]) for k in ("dinit", "dwt", "dtrack", "seed_traj", "seed_ctrl", "kgain", "wgain", "ogain")}
    for null in ("dinit", "dwt", "dtrack"):
        args = {k: (None if k == null else r[k]) for k in ("dinit", "dwt", "dtrack")}
        zero = {k: (z[k] if k == null else r[k]) for k in ("dinit", "dwt", "dtrack")}
        for x, y in zip(run_tangent(looplinx, r, Lt, **args), run_tangent(looplinx, r, Lt, **zero)):
            assert np.array_equal(x, y)
    for null in ("kgain", "wgain", "ogain"):
        rz = dict(r, **{null: z[null]})
        kw = {null: "absent"}
        dwt = None if null == "wgain" else r["dwt"]
        dtrack = None if null == "ogain" else r["dtrack"]
        for x, y in zip(run_tangent(looplinx, r, Lt, r["dinit"], dwt, dtrack, **kw), run_tangent(looplinx, rz, Lt, r["dinit"], r["dwt"], r["dtrack"])):
            assert np.array_equal(x, y)
    for st, sc in ((None, r["seed_ctrl"]), (r["seed_traj"], None)):
        got = run_adjoint(looplinx, r, Lt, st, sc)
        want = run_adjoint(looplinx, r, Lt, z["seed_traj"] if st is None else st, z["seed_ctrl"] if sc is None else sc)
        assert all(np.array_equal(x, y) for x, y in zip(got, want))
    gi2, gw2, gt2 = run_adjoint(looplinx, r, Lt, r["seed_traj"], r["seed_ctrl"], want_track=False)
    assert np.array_equal(gi2, gi) and np.array_equal(gw2, gw) and np.all(gt2 == 7.0)
    # either output of the tangent may be null
    only = np.full((B4, ND4, L4, 2), 7.0)
    looplinx.looplinx_tangent(DT4, WB4, B4, L4, ND4, _dp(r["traj"]), _dp(r["kgain"]), _dp(r["wgain"]), _dp(r["ogain"]), Lt, _dp(r["dinit"]), _dp(r["dwt"]),
                              _dp(r["dtrack"]), None, _dp(only))
    assert np.array_equal(only, dctrl)


@pytest.mark.parametrize("Lt", [1, L4, L4 + 3])
def test_nan_gains_spread_as_documented(looplinx, Lt):
    """NaN gains at step 2 of ego 3: dctrl is NaN from row 2 on, dtraj in the two states the controls drive (steering angle, velocity) at row 3 and in
    every state from row 4 on, both untouched before; the adjoint's grad_init and grad_wt of that ego are NaN, and the rows of grad_track up to
    min(2, Lt - 1); every other ego is untouched"""
    r = random_loop(Lt, 50 + Lt)
    clean = run_tangent(looplinx, r, Lt, r["dinit"], r["dwt"], r["dtrack"]), run_adjoint(looplinx, r, Lt, r["seed_traj"], r["seed_ctrl"])
    for k in ("kgain", "wgain", "ogain"):
        r[k][3, 2] = np.nan
    dtraj, dctrl = run_tangent(looplinx, r, Lt, r["dinit"], r["dwt"], r["dtrack"])
    gi, gw, gt = run_adjoint(looplinx, r, Lt, r["seed_traj"], r["seed_ctrl"])
    assert np.all(np.isnan(dctrl[3, :, 2:])) and np.all(np.isnan(dtraj[3, :, 3, 2:4])) and np.all(np.isnan(dtraj[3, :, 4:]))
    assert np.array_equal(dctrl[3, :, :2], clean[0][1][3, :, :2]) and np.array_equal(dtraj[3, :, :3], clean[0][0][3, :, :3])
    assert np.array_equal(dtraj[3, :, 3, [0, 1, 4]], clean[0][0][3, :, 3, [0, 1, 4]])
    assert np.all(np.isnan(gi[3])) and np.all(np.isnan(gw[3]))
    last = min(2, Lt - 1)
    assert np.all(np.isnan(gt[3, :last + 1])) and np.array_equal(gt[3, last + 1:], clean[1][2][3, last + 1:])
    others = [b for b in range(B4) if b != 3]
    for got, want in zip((dtraj, dctrl, gi, gw, gt), clean[0] + clean[1]):
        assert np.array_equal(got[others], want[others])


# ---- 5: the Python layer, through a stand-in for the library ---------------------------------------------------------------------------------
class _FakeLib:
    """records the calls BatchedMPCSolver makes (no GPU, no library)"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def _solver_without_gpu():
    s = object.__new__(pkg.BatchedMPCSolver)
    s._lib, s._h, s.N, s.nx = _FakeLib(), C.c_void_p(1), 10, 5
    return s


def test_closed_loop_linearize_routes_to_the_lin_entry_point():
    s = _solver_without_gpu()
    B, L = 3, 12
    init, path, orient = np.zeros((B, 5)), np.zeros((B, L, 2)), np.zeros((B, L))
    lin = s.closed_loop(init, path, orient, 10.0, L, linearize=True)
    assert isinstance(lin, pkg.LoopLin) and lin.ogain is None and lin.clearance is None and lin.Lt == 0
    assert lin.traj.shape == (B, L, 5) and lin.kgain.shape == (B, L, 2, 5) and lin.wgain.shape == (B, L, 2, 7) and lin.status.dtype == np.int32
    lo = s.closed_loop(init, path, orient, 10.0, L, obst_track=np.zeros((B, L, 3)), obst_offset=1.0, clearance=True, linearize=True)
    assert lo.ogain.shape == (B, L, 2, 3) and lo.clearance.shape == (B, L) and lo.Lt == L
    l1 = s.closed_loop(init, path, orient, 10.0, L, obst_track=np.zeros((B, 3)), linearize=True)
    assert l1.Lt == 1 and l1.clearance is None
    assert len(s.closed_loop(init, path, orient, 10.0, L)) == 3                                     # (without linearize: as before)
    (n0, a0), (n1, a1), (n2, a2), (n3, _) = s._lib.calls
    assert (n0, n1, n2, n3) == ("mpc_closed_loop_batch_lin",) * 3 + ("mpc_closed_loop_batch_ex",)
    assert len(a0) == len(a1) == len(abi.PROTOTYPES["mpc_closed_loop_batch_lin"])
    assert a0[8] == 0 and a0[9] is None and a0[17] is None and a0[18] is not None and a0[19] is not None and a0[20] is None
    assert a1[8] == L and a1[10] == 1.0 and all(a1[q] is not None for q in (9, 17, 18, 19, 20))
    assert a2[8] == 1 and a2[17] is None
    with pytest.raises(pkg.MpcError):
        s.closed_loop(init, path, orient, 10.0, L, clearance=True, linearize=True)


def test_sweep_argument_checks_and_routing():
    s = _solver_without_gpu()
    B, L, nd = 3, 6, 2
    z = np.zeros
    lin = pkg.LoopLin(z((B, L, 5)), z((B, L, 2)), z((B, L), np.int32), z((B, L, 2, 5)), z((B, L, 2, 7)))
    lo = pkg.LoopLin(z((B, L, 5)), z((B, L, 2)), z((B, L), np.int32), z((B, L, 2, 5)), z((B, L, 2, 7)), z((B, L, 2, 3)), None, L)
    dtraj, dctrl = s.loop_tangent(lin, dinit=z((B, nd, 5)))
    assert dtraj.shape == (B, nd, L, 5) and dctrl.shape == (B, nd, L, 2)
    s.loop_tangent(lo, dwt=z((B, nd, 7)), dtrack=z((B, nd, L, 3)))
    gi, gw, gt = s.loop_adjoint(lin, seed_traj=z((B, L, 5)))
    assert gi.shape == (B, 5) and gw.shape == (B, 7) and gt is None
    assert s.loop_adjoint(lo, seed_ctrl=z((B, L, 2)))[2].shape == (B, L, 3)
    (n0, a0), (n1, a1), (n2, a2), (n3, a3) = s._lib.calls
    assert (n0, n1, n2, n3) == ("mpc_loop_tangent", "mpc_loop_tangent", "mpc_loop_adjoint", "mpc_loop_adjoint")
    assert len(a0) == len(abi.PROTOTYPES["mpc_loop_tangent"]) and len(a2) == len(abi.PROTOTYPES["mpc_loop_adjoint"])
    assert a0[1:4] == (B, L, nd) and a0[8] is None and a0[9] == 0 and a0[10] is not None and a0[11] is None and a0[12] is None
    assert a1[8] is not None and a1[9] == L and a1[10] is None and a1[11] is not None and a1[12] is not None
    assert a2[1:3] == (B, L) and a2[8] == 0 and a2[9] is not None and a2[10] is None and a2[13] is None
    assert a3[8] == L and a3[9] is None and a3[10] is not None and a3[13] is not None
    for bad in (dict(), dict(dtrack=z((B, nd, L, 3))), dict(dinit=z((B, nd, 4))), dict(dinit=z((B, nd, 5)), dwt=z((B, nd + 1, 7))), dict(dinit=z((B + 1, nd, 5)))):
        with pytest.raises(pkg.MpcError):
            s.loop_tangent(lin, **bad)
    with pytest.raises(pkg.MpcError):
        s.loop_tangent(lo, dtrack=z((B, nd, L + 1, 3)))
    with pytest.raises(pkg.MpcError):
        s.loop_adjoint(lin, seed_traj=z((B, L, 4)))
    s._lib.calls.clear()
    s.closed_loop_lin_device(B, 1, 2, 3, 4, L, L, 5, 6, d_kgain=7)
    s.loop_tangent_device(B, L, nd, 1, 2, d_kgain=3, d_dinit=4, d_dtraj=5)
    s.loop_adjoint_device(B, L, 1, 2, d_kgain=3, d_seed_traj=4, d_grad_init=5)
    names = [c[0] for c in s._lib.calls]
    assert names == ["mpc_closed_loop_batch_lin_dev", "mpc_loop_tangent_dev", "mpc_loop_adjoint_dev"]
    assert [len(c[1]) for c in s._lib.calls] == [len(abi.PROTOTYPES[n]) for n in names]
