"""GPU: the linearised closed loop -- per-step feedback gains beside the rollout, the tangent and adjoint sweeps over them and the torch layer
(mpc_closed_loop_batch_lin[_dev], mpc_loop_tangent[_dev], mpc_loop_adjoint[_dev], autograd.mpc_closed_loop).

The scenes, the numpy chained reference and every bound are those of tests/loop_lin_ref.py, which tests/test_loop_lin_cpu.py holds to central
differences of the oracle loop."""
import dataclasses
import importlib

import numpy as np
import pytest

import loop_lin_ref as ref
import loop_obst_ref as obst_ref
from helpers import abi, make_solver, pkg, set_cfg_bounds, synthetic_batch

pytestmark = pytest.mark.gpu
_dp = abi.as_dp
MPC_ERR_INVALID, MPC_ERR_STATE = -1, -4
B_TILED = 130                      # two full blocks of 64 lanes of the gain kernels and a partial one


def solver_for(cfg, **kw):
    s = make_solver(cfg, **kw)
    set_cfg_bounds(s, cfg)
    s.set_option("loop_async", "0")
    return s


def loop_args(scenes, copies=None):
    """(positional arguments, keyword arguments) of closed_loop for a batch of scenes, tiled to `copies` egos"""
    init, path, orient, vdes, track = ref.batch_inputs(scenes)
    if copies is not None:
        idx = np.arange(copies) % len(scenes)
        init, path, orient, vdes = init[idx], path[idx], orient[idx], vdes[idx]
        track = None if track is None else np.ascontiguousarray(track[idx])
    kw = {} if track is None else dict(obst_track=track, obst_offset=obst_ref.OFFSET)
    return (init, path, orient, vdes, scenes[0].L), kw


def as_dict(lin):
    return dict(traj=lin.traj, ctrl=lin.ctrl, status=lin.status, kgain=lin.kgain, wgain=lin.wgain, ogain=lin.ogain)


@pytest.fixture(scope="module", params=["LF", "OB"])
def batch(request):
    """one kind of scenes on one handle: the step-by-step plain loop, then the lin loop"""
    kind = request.param
    scenes = ref.LF_SCENES if kind == "LF" else ref.OB_SCENES
    s = solver_for(scenes[0].cfg)
    args, kw = loop_args(scenes)
    plain = s.closed_loop(*args, **kw)
    lin = s.closed_loop(*args, linearize=True, **kw)
    yield kind, scenes, s, plain, lin
    s.close()


# ---- 1 -----------------------------------------------------------------------------------------------------------------------------------
def test_rollout_is_bitwise_the_plain_loops_and_gains_match_the_reference(batch):
    kind, scenes, s, plain, lin = batch
    assert np.array_equal(lin.traj, plain[0]) and np.array_equal(lin.ctrl, plain[1]) and np.array_equal(lin.status, plain[2])
    assert np.all(lin.status == 1)
    assert (lin.ogain is None) == (kind == "LF")
    worst, n_weak = ref.gain_errors(scenes, kind, as_dict(lin))
    print(f"\n  {kind}: gains vs reference, worst k {worst['k']:.2e} (bound {ref.TOL_K:.0e}) w {worst['w']:.2e} (bound {ref.TOL_W:.0e}) o {worst['o']:.2e} "
          f"(bound {ref.TOL_O:.0e}), {n_weak} weakly active steps excluded")
    assert worst["k"] <= ref.TOL_K and worst["w"] <= ref.TOL_W and worst["o"] <= ref.TOL_O


def test_device_sweeps_against_the_numpy_recursion(batch):
    """mpc_loop_tangent / mpc_loop_adjoint on the device's own gains: within 1e-12 of the sum of the absolute terms of every entry of the numpy
    recursion over the same gains"""
    kind, scenes, s, _, lin = batch
    B, L = lin.traj.shape[:2]
    cfg, rng = scenes[0].cfg, np.random.default_rng(7)
    nd = 3
    dinit, dwt = rng.normal(size=(B, nd, 5)), rng.normal(size=(B, nd, 7))
    dtrack = None if lin.ogain is None else rng.normal(size=(B, nd, lin.Lt, 3))
    st, sc = rng.normal(size=(B, L, 5)), rng.normal(size=(B, L, 2))
    dtraj, dctrl = s.loop_tangent(lin, dinit, dwt, dtrack)
    gi, gw, gt = s.loop_adjoint(lin, st, sc)
    worst = 0.0
    for b in range(B):
        a = (lin.traj[b], lin.kgain[b], lin.wgain[b], None if lin.ogain is None else lin.ogain[b], lin.Lt)
        for d in range(nd):
            dt_b = None if dtrack is None else dtrack[b, d]
            want = ref.tangent(*a, dinit[b, d], dwt[b, d], dt_b, cfg.dt, cfg.wheelbase)
            mag = ref.tangent(*a, dinit[b, d], dwt[b, d], dt_b, cfg.dt, cfg.wheelbase, mag=True)
            for got, w_, m_ in zip((dtraj[b, d], dctrl[b, d]), want, mag):
                assert np.all(np.abs(got - w_) <= 1e-12 * m_), (b, d)
                worst = max(worst, float(np.max(np.abs(got - w_) / np.maximum(m_, 1e-300))))
        want = ref.adjoint(*a, st[b], sc[b], cfg.dt, cfg.wheelbase)
        mag = ref.adjoint(*a, st[b], sc[b], cfg.dt, cfg.wheelbase, mag=True)
        for got, w_, m_ in zip((gi[b], gw[b]) + (() if gt is None else (gt[b],)), want, mag):
            assert np.all(np.abs(got - w_) <= 1e-12 * m_), b
            worst = max(worst, float(np.max(np.abs(got - w_) / np.maximum(m_, 1e-300))))
    print(f"\n  {kind}: device sweeps vs numpy recursion, worst |delta| / sum of absolute terms {worst:.2e}")


# ---- 2 -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["LF", "OB"])
def test_tiled_batch_every_copy_equals_the_first(kind):
    scenes = ref.LF_SCENES if kind == "LF" else ref.OB_SCENES
    s = solver_for(scenes[0].cfg)
    args, kw = loop_args(scenes, B_TILED)
    lin = s.closed_loop(*args, linearize=True, **kw)
    n = len(scenes)
    assert np.all(lin.status == 1)
    for name, a in as_dict(lin).items():
        if a is None:
            continue
        assert np.all(np.isfinite(a)), name
        for b in range(n, B_TILED):
            assert np.array_equal(a[b], a[b % n]), (name, b)
    s.close()


# ---- 3 -----------------------------------------------------------------------------------------------------------------------------------
def test_nx6_gains_match_the_reference():
    scenes = ref.LF_SCENES
    s = solver_for(dataclasses.replace(scenes[0].cfg, nx=6))
    args, kw = loop_args(scenes)
    lin = s.closed_loop(*args, linearize=True, **kw)
    assert np.all(lin.status == 1)
    worst, n_weak = ref.gain_errors(scenes, "LF", as_dict(lin))
    print(f"\n  LF nx = 6: gains vs reference, worst k {worst['k']:.2e} (bound {ref.TOL_K:.0e}) w {worst['w']:.2e} (bound {ref.TOL_W:.0e}), {n_weak} weak steps excluded")
    assert worst["k"] <= ref.TOL_K and worst["w"] <= ref.TOL_W
    s.close()


# ---- 4 -----------------------------------------------------------------------------------------------------------------------------------
def _device_fd(s, scenes, noise, which):
    """central difference of the device loop's (traj | ctrl) along one direction of every ego, and the device tangent of the unperturbed loop"""
    (init, path, orient, vdes, L), kw = loop_args(scenes)
    B = init.shape[0]
    wt0 = s.weights.copy()
    lin = s.closed_loop(init, path, orient, vdes, L, linearize=True, **noise, **kw)
    assert np.all(lin.status == 1)
    dinit = dwt = dtrack = None
    if which == "init_y":
        h = ref.FD_REL * np.maximum(1.0, np.abs(init[:, 1]))
        dinit = np.zeros((B, 1, 5)); dinit[:, 0, 1] = 1.0
    elif which == "Q1":
        h = np.full(B, ref.FD_REL * wt0[1])
        dwt = np.zeros((B, 1, 7)); dwt[:, 0, 1] = 1.0
    else:
        h = ref.FD_REL * np.maximum(1.0, np.abs(kw["obst_track"][:, :, 1]).max(axis=1))
        dtrack = np.zeros((B, 1, lin.Lt, 3)); dtrack[:, 0, :, 1] = 1.0
    runs = []
    for sg in (1.0, -1.0):
        i2, k2 = init.copy(), dict(kw)
        if which == "init_y":
            i2[:, 1] += sg * h
        elif which == "Q1":
            w2 = wt0.copy(); w2[1] += sg * h[0]
            s.set_weights(w2[:5], w2[5:])
        else:
            t2 = kw["obst_track"].copy(); t2[:, :, 1] += sg * h[:, None]
            k2["obst_track"] = t2
        r = s.closed_loop(i2, path, orient, vdes, L, **noise, **k2)
        assert np.all(r[2] == 1)
        runs.append(np.concatenate([r[0], r[1]], axis=2))
    s.set_weights(wt0[:5], wt0[5:])
    fd = (runs[0] - runs[1]) / (2 * h[:, None, None])
    dtraj, dctrl = s.loop_tangent(lin, dinit, dwt, dtrack)
    return fd, np.concatenate([dtraj[:, 0], dctrl[:, 0]], axis=2)


@pytest.mark.parametrize("kind,which,noised", [("LF", "init_y", False), ("LF", "Q1", False), ("OB", "pose_y", False), ("LF", "init_y", True)])
def test_tangent_against_finite_differences_of_the_device_loop(kind, which, noised):
    """the device tangent against central differences (relative step FD_REL) of the device's own loop, per ego max|delta| / max|FD| <= TOL_LOOP;
    once with noise on the applied input (noise_mode 2, sigma 0.1, the same seed on both sides: the noise is additive and carries no derivative)"""
    scenes = ref.LF_SCENES if kind == "LF" else ref.OB_SCENES
    s = solver_for(scenes[0].cfg)
    noise = dict(noise_mode=2, sigma=0.1, seed=20241019) if noised else {}
    fd, tan = _device_fd(s, scenes, noise, which)
    errs = [ref.rel_err(tan[b], fd[b]) for b in range(len(scenes))]
    print(f"\n  {kind} {which}{' noised' if noised else ''}: tangent vs FD of the device loop per ego " + " ".join(f"{e:.1e}" for e in errs) + f" (bound {ref.TOL_LOOP:.1e})")
    assert all(np.abs(fd[b]).max() >= ref.FD_FLOOR for b in range(len(scenes)))
    assert max(errs) <= ref.TOL_LOOP
    s.close()


# ---- 5 -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_iter", [3, 7])
def test_steps_that_do_not_converge_get_nan_gains(max_iter):
    """max_iter = 3: no step of the obstacle scenes converges (the oracle needs 6 to 12 iterations per step); max_iter = 7: the first sixteen steps
    of every scene need at most 7.  NaN gains exactly on the steps whose status is not 1; the rollout is still the plain loop's, bit for bit"""
    scenes = ref.OB_SCENES
    s = solver_for(scenes[0].cfg, max_iter=max_iter)
    args, kw = loop_args(scenes)
    plain = s.closed_loop(*args, **kw)
    lin = s.closed_loop(*args, linearize=True, **kw)
    assert np.array_equal(lin.traj, plain[0]) and np.array_equal(lin.ctrl, plain[1]) and np.array_equal(lin.status, plain[2])
    bad = lin.status != 1
    print(f"\n  max_iter = {max_iter}: {int(bad.sum())} of {bad.size} steps did not converge")
    assert bad.any() if max_iter == 3 else (~bad).any()
    for g in (lin.kgain, lin.wgain, lin.ogain):
        assert np.all(np.isnan(g[bad])) and np.all(np.isfinite(g[~bad]))
    s.close()


# ---- 6 -----------------------------------------------------------------------------------------------------------------------------------
def test_autograd_layer_matches_the_adjoint_sweep(batch):
    import torch
    ag = importlib.import_module(pkg.__name__ + ".autograd")
    kind, scenes, s, _, lin = batch
    (init, path, orient, vdes, L), kw = loop_args(scenes)
    dev = torch.device("cuda")
    t = lambda a, g=False: torch.tensor(a, dtype=torch.float64, device=dev, requires_grad=g)      # noqa: E731
    wt0 = s.weights.copy()
    wt_set = wt0 * (1.0 + 1e-3 * np.arange(7))
    ti, tw = t(init, True), torch.tensor(wt_set, dtype=torch.float64, requires_grad=True)
    tt = None if kind == "LF" else t(kw["obst_track"], True)
    try:
        traj, ctrl = ag.mpc_closed_loop(s, ti, tw, t(path), t(orient), t(vdes), L, obst_track=tt, obst_offset=kw.get("obst_offset", 0.0))
        assert np.array_equal(s.weights, wt_set)
        ((traj ** 2).sum() + ctrl.sum()).backward()
        lin2 = s.closed_loop(init, path, orient, vdes, L, linearize=True, **kw)
        assert np.array_equal(lin2.traj, traj.detach().cpu().numpy()) and np.array_equal(lin2.ctrl, ctrl.detach().cpu().numpy())
        gi, gw, gt = s.loop_adjoint(lin2, 2.0 * lin2.traj, np.ones_like(lin2.ctrl))
        pairs = [(ti.grad.cpu().numpy(), gi), (tw.grad.numpy(), gw.sum(axis=0))] + ([] if tt is None else [(tt.grad.cpu().numpy(), gt)])
        for got, want in pairs:
            assert np.all(np.isfinite(want)) and np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    finally:
        s.set_weights(wt0[:5], wt0[5:])                      # (the handle is the module's)


# ---- 7 -----------------------------------------------------------------------------------------------------------------------------------
def test_errors():
    scenes = ref.LF_SCENES
    cfg = scenes[0].cfg
    (init, path, orient, vdes, L), _ = loop_args(scenes)
    B = init.shape[0]
    fixed = solver_for(cfg, fixed_iters=5)
    with pytest.raises(pkg.MpcError) as e:
        fixed.closed_loop(init, path, orient, vdes, L, linearize=True)
    assert e.value.code == MPC_ERR_INVALID
    fixed.close()
    s = solver_for(cfg)
    traj, ctrl, st = np.empty((B, L, 5)), np.empty((B, L, 2)), np.empty((B, L), np.int32)
    og = np.empty((B, L, 2, 3))
    rc = s._lib.mpc_closed_loop_batch_lin(s._h, B, L, L, _dp(init), _dp(path), _dp(orient), _dp(vdes), 0, None, 0.0, 0, 0.0, 0, _dp(traj), _dp(ctrl),
                                          abi.as_ip(st), None, None, None, _dp(og))
    assert rc == MPC_ERR_INVALID
    kg = np.zeros((B, L, 2, 5))
    dtrack, dtraj = np.zeros((B, 1, L, 3)), np.empty((B, 1, L, 5))
    rc = s._lib.mpc_loop_tangent(s._h, B, L, 1, _dp(traj), _dp(ctrl), _dp(kg), None, None, L, None, None, _dp(dtrack), _dp(dtraj), None)
    assert rc == MPC_ERR_INVALID
    # a lin loop ends the life of the sensitivity snapshot, as every loop does
    x0, p = synthetic_batch(cfg, B)
    s.solve(x0, p, lam_p=True)
    s.sens_adjoint(np.ones((B, s.n_w)))
    s.closed_loop(init, path, orient, vdes, L, linearize=True)
    for call in (lambda: s.sens_adjoint(np.ones((B, s.n_w))), lambda: s.sens_weights(p, seed_w=np.ones((B, s.n_w))), lambda: s.sens_obst(seed_w=np.ones((B, s.n_w))),
                 lambda: s.sens_bounds(seed_w=np.ones((B, s.n_w)))):
        with pytest.raises(pkg.MpcError) as e:
            call()
        assert e.value.code == MPC_ERR_STATE
    s.close()
