"""GPU: the derivative of the optimum with respect to the obstacle circle centres -- forward dw = (dw*/do) dobst, the adjoint grad_obst,
lam_obst and the torch layer (mpc_sens_obst[_dev], autograd.py).

Every instance solves against obstacle rows of its own (the descriptor's centres shifted by a few decimetres per instance) and is compared
with the active-set derivative of the numpy NLP at its own centres (tests/sens_obst_ref.py): rows mixed up between instances show."""
import ctypes as C
import importlib

import numpy as np
import pytest

import sens_obst_ref
from helpers import CA_CFG, NLPConfig, WEIGHTS_ZAM_LF, ca_batch, make_solver, pkg, set_cfg_bounds, synthetic_batch

MPC_ERR_INVALID, MPC_ERR_STATE = -1, -4
TOL_DW = 1e-5
N_DIR = 7
LF_CFG = NLPConfig(N=10, nx=6, **WEIGHTS_ZAM_LF)


def solver_for(cfg, **kw):
    s = make_solver(cfg, **kw)
    set_cfg_bounds(s, cfg)
    return s


def obst_rows(cfg, B):
    """the descriptor's centres shifted by a few decimetres per instance (every instance another row)"""
    c0 = cfg.obstacle_centers.ravel()
    sh = np.array([[0.15 * (b % 4) - 0.2, 0.1 * ((b * 3) % 5) - 0.2] for b in range(B)])
    return np.ascontiguousarray(c0[None, :] + np.tile(sh, (1, 3)))


def directions(B, seed):
    """the six unit directions and one random one"""
    d = np.zeros((B, N_DIR, 6))
    d[:, :6] = np.eye(6)
    d[:, 6] = np.random.default_rng(seed).normal(size=(B, 6))
    return d


def check_nan_rule(status, lam_g, dw, grad, lam):
    kink = np.isnan(lam_g[:, 0]) & (status == 1)
    bad = (status != 1) | kink
    assert np.all(np.isnan(dw[bad])) and np.all(np.isnan(grad[bad])) and np.all(np.isnan(lam[bad]))
    good = ~bad
    assert np.all(np.isfinite(dw[good])) and np.all(np.isfinite(grad[good])) and np.all(np.isfinite(lam[good]))
    return good


def check_adjoint(good, seeds, dw, grad, dobst):
    for b in np.flatnonzero(good):
        for d in range(dobst.shape[1]):
            lhs, rhs = seeds[b] @ dw[b, d], grad[b] @ dobst[b, d]
            assert abs(lhs - rhs) <= 1e-10 * max(1.0, np.abs(seeds[b]).sum() * np.max(np.abs(dw[b, d]))), (b, d, lhs, rhs)


def check_reference(cfg, ref, good, x, lam_g, obst, dobst, dw, lam):
    """dw of the strictly complementary rows and lam_obst of every good row against numpy; returns the number of rows compared"""
    checked, worst = 0, 0.0
    for b in np.flatnonzero(good):
        lo = sens_obst_ref.lam_obst(cfg, obst[b], x[b], lam_g[b])
        assert np.max(np.abs(lam[b] - lo)) <= 1e-12 * max(1.0, np.max(np.abs(lo))), (b, lam[b], lo)
        S, weak = ref[b]
        if weak:
            continue
        want = np.einsum("ij,dj->di", S, dobst[b])
        err = np.max(np.abs(dw[b] - want)) / max(1.0, np.max(np.abs(want)))
        assert np.isfinite(err) and err <= TOL_DW, (b, err)
        worst = max(worst, err)
        checked += 1
    print(f"\n  dw vs numpy: {checked} of {int(good.sum())} rows checked, worst relative error {worst:.2e}")
    return checked


@pytest.fixture(scope="module")
def ca():
    """the collision-avoidance batch solved once through the host-pointer form, its obstacle derivative, and the numpy reference per row"""
    cfg, B = CA_CFG, 8
    x0, p = ca_batch(cfg, B)
    obst = obst_rows(cfg, B)
    dobst = directions(B, 31)
    seeds = np.random.default_rng(32).normal(size=(B, cfg.n_w))
    s = solver_for(cfg)
    r = s.solve(x0, p, obst, multipliers=True, lam_p=True)
    o = s.sens_obst(dobst, seeds, lam=True)
    ref = {int(b): sens_obst_ref.sensitivity_matrix(cfg, obst[b], r.x[b], p[b], r.lam_g[b], r.lam_x[b]) for b in np.flatnonzero(r.status == 1)}
    return dict(cfg=cfg, B=B, x0=x0, p=p, obst=obst, dobst=dobst, seeds=seeds, solver=s, r=r, o=o, ref=ref)


@pytest.mark.gpu
def test_host_form_matches_reference(ca):
    cfg, r, o = ca["cfg"], ca["r"], ca["o"]
    assert np.sum(r.status == 1) >= 6
    nlp_rows = 1 + cfg.nx * (cfg.N + 1)
    assert np.min(r.lam_g[r.status == 1][:, nlp_rows:]) < -1e-3                       # active circle rows
    good = check_nan_rule(r.status, r.lam_g, o.dw, o.grad_obst, o.lam_obst)
    checked = check_reference(cfg, ca["ref"], good, r.x, r.lam_g, ca["obst"], ca["dobst"], o.dw, o.lam_obst)
    assert checked >= (int(np.sum(r.status == 1)) + 1) // 2, checked
    assert np.nanmax(np.abs(o.dw)) > 0.1                                              # the plan moves with the obstacle
    check_adjoint(good, ca["seeds"], o.dw, o.grad_obst, ca["dobst"])
    # every part alone gives the same numbers
    s = ca["solver"]
    assert np.array_equal(s.sens_obst(ca["dobst"]).dw, o.dw, equal_nan=True)
    assert np.array_equal(s.sens_obst(seed_w=ca["seeds"]).grad_obst, o.grad_obst, equal_nan=True)
    assert np.array_equal(s.sens_obst(lam=True).lam_obst, o.lam_obst, equal_nan=True)


@pytest.mark.gpu
def test_device_form_on_a_stream(ca):
    """a _sens solve with no sensitivity output is enough for the snapshot; the _dev form on a side stream gives the host form's numbers"""
    import torch
    cfg, B, s = ca["cfg"], ca["B"], solver_for(ca["cfg"])
    dev = torch.device("cuda")
    t = {k: torch.from_numpy(np.ascontiguousarray(ca[k])).to(dev) for k in ("x0", "p", "obst", "dobst", "seeds")}
    tx, tst = torch.empty_like(t["x0"]), torch.empty(B, dtype=torch.int32, device=dev)
    tdw = torch.empty((B, N_DIR, cfg.n_w), dtype=torch.float64, device=dev)
    tgo, tlo = torch.empty((B, 6), dtype=torch.float64, device=dev), torch.empty((B, 6), dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        s.solve_sens_device(B, t["x0"].data_ptr(), t["p"].data_ptr(), tx.data_ptr(), d_status=tst.data_ptr(), d_obst=t["obst"].data_ptr(),
                            stream=stream.cuda_stream)
        before = tx.clone()
        s.sens_obst_device(B, N_DIR, t["dobst"].data_ptr(), tdw.data_ptr(), t["seeds"].data_ptr(), tgo.data_ptr(), tlo.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    r, o = ca["r"], ca["o"]
    assert torch.equal(before, tx)
    assert np.array_equal(tx.cpu().numpy(), r.x) and np.array_equal(tst.cpu().numpy(), r.status)
    dw, go, lo = tdw.cpu().numpy(), tgo.cpu().numpy(), tlo.cpu().numpy()
    good = check_nan_rule(r.status, r.lam_g, dw, go, lo)
    checked = check_reference(cfg, ca["ref"], good, r.x, r.lam_g, ca["obst"], ca["dobst"], dw, lo)
    assert checked >= (int(np.sum(r.status == 1)) + 1) // 2, checked
    check_adjoint(good, ca["seeds"], dw, go, ca["dobst"])
    for a, b in ((dw, o.dw), (go, o.grad_obst), (lo, o.lam_obst)):
        assert np.allclose(a, b, rtol=0, atol=1e-12 * max(1.0, np.nanmax(np.abs(b))), equal_nan=True)


@pytest.mark.gpu
def test_rows_that_did_not_converge_are_nan(ca):
    s = solver_for(ca["cfg"], max_iter=3)
    r = s.solve(ca["x0"], ca["p"], ca["obst"], multipliers=True, lam_p=True)
    assert np.all(r.status != 1)
    o = s.sens_obst(ca["dobst"], ca["seeds"], lam=True)
    assert np.all(np.isnan(o.dw)) and np.all(np.isnan(o.grad_obst)) and np.all(np.isnan(o.lam_obst))


@pytest.mark.gpu
def test_small_lane_following_case_is_zero():
    """nx = 6, N = 10, B = 3, the obstacle a hundred metres away: no circle row is active, the reference's derivative is exactly 0 and the
    solver's is 0 to the tolerance, through both forms"""
    import torch
    cfg, B = LF_CFG, 3
    x0, p = synthetic_batch(cfg, B)
    obst = obst_rows(cfg, B)
    dobst = directions(B, 33)
    seeds = np.random.default_rng(34).normal(size=(B, cfg.n_w))
    s = solver_for(cfg)
    r = s.solve(x0, p, obst, multipliers=True, lam_p=True)
    assert np.all(r.status == 1)
    o = s.sens_obst(dobst, seeds, lam=True)
    for b in range(B):
        S, _ = sens_obst_ref.sensitivity_matrix(cfg, obst[b], r.x[b], p[b], r.lam_g[b], r.lam_x[b])
        assert not S.any()
        lo = sens_obst_ref.lam_obst(cfg, obst[b], r.x[b], r.lam_g[b])
        assert np.max(np.abs(o.lam_obst[b] - lo)) <= 1e-12 * max(1.0, np.max(np.abs(lo)))
    assert np.all(np.isfinite(o.dw)) and np.max(np.abs(o.dw)) <= TOL_DW
    check_adjoint(np.ones(B, bool), seeds, o.dw, o.grad_obst, dobst)
    dev = torch.device("cuda")
    tdo, tse = torch.from_numpy(dobst).to(dev), torch.from_numpy(seeds).to(dev)
    tdw = torch.empty((B, N_DIR, cfg.n_w), dtype=torch.float64, device=dev)
    tgo = torch.empty((B, 6), dtype=torch.float64, device=dev)
    s.sens_obst_device(B, N_DIR, tdo.data_ptr(), tdw.data_ptr(), tse.data_ptr(), tgo.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(tdw.cpu().numpy(), o.dw) and np.array_equal(tgo.cpu().numpy(), o.grad_obst)


@pytest.mark.gpu
def test_call_order_and_arguments(ca):
    cfg, B, s = ca["cfg"], ca["B"], solver_for(ca["cfg"])
    L = s._lib
    dptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    dobst, seeds = np.ascontiguousarray(ca["dobst"]), np.ascontiguousarray(ca["seeds"])
    dw, go, lo = np.empty((B, N_DIR, cfg.n_w)), np.empty((B, 6)), np.empty((B, 6))
    call = lambda B_, nd, do, w, se, g, l: L.mpc_sens_obst(s._h, B_, nd, do, w, se, g, l)  # noqa: E731
    # no snapshot yet
    assert call(B, N_DIR, dptr(dobst), dptr(dw), dptr(seeds), dptr(go), dptr(lo)) == MPC_ERR_STATE
    s.solve(ca["x0"], ca["p"], ca["obst"], lam_p=True)
    assert call(B, N_DIR, dptr(dobst), dptr(dw), dptr(seeds), dptr(go), dptr(lo)) == 0
    # bad arguments: a seed without its gradient, directions without both arrays, a negative count
    assert call(B, 0, None, None, dptr(seeds), None, None) == MPC_ERR_INVALID
    assert b"seed_w" in L.mpc_last_error(s._h)
    assert call(B, N_DIR, dptr(dobst), None, None, None, None) == MPC_ERR_INVALID
    assert call(B, N_DIR, None, dptr(dw), None, None, None) == MPC_ERR_INVALID
    assert call(B, -1, None, None, None, None, dptr(lo)) == MPC_ERR_INVALID
    assert b"n_dir" in L.mpc_last_error(s._h)
    # another B, then an intervening plain solve: the snapshot is not this call's
    assert call(B - 1, 0, None, None, None, None, dptr(lo)) == MPC_ERR_STATE
    assert call(B, 0, None, None, None, None, dptr(lo)) == 0
    s.solve(ca["x0"][:4], ca["p"][:4])
    assert call(B, 0, None, None, None, None, dptr(lo)) == MPC_ERR_STATE
    with pytest.raises(pkg.MpcError) as e:
        s.sens_obst(lam=True)
    assert e.value.code == MPC_ERR_STATE


@pytest.mark.gpu
def test_solve_outputs_keep_their_bits(ca):
    """x_out .. lam_p, dw of mpc_solve_batch_sens are the same bits whether or not mpc_sens_obst runs afterwards, and the solve after it too"""
    cfg, B, s = ca["cfg"], ca["B"], solver_for(ca["cfg"])
    dp = np.zeros((B, 2, cfg.n_w))
    dp[:, 0] = np.random.default_rng(35).normal(size=(B, cfg.n_w))
    dp[:, 1, 2 * cfg.N + 3] = 1.0
    solve = lambda: s.solve(ca["x0"], ca["p"], ca["obst"], multipliers=True, lam_p=True, dp=dp)  # noqa: E731
    a = solve()
    b = solve()
    s.sens_obst(ca["dobst"], ca["seeds"], lam=True)
    c = solve()
    for fld in ("x", "status", "iters", "kkt", "f", "g", "lam_g", "lam_x", "lam_p", "dw"):
        assert np.array_equal(getattr(a, fld), getattr(b, fld), equal_nan=True), fld
        assert np.array_equal(getattr(a, fld), getattr(c, fld), equal_nan=True), fld
    # ... and the p-adjoint on the same snapshot is not disturbed by the obstacle solves in between (they share the factor storage)
    g0 = s.sens_adjoint(ca["seeds"])
    s.sens_obst(ca["dobst"], ca["seeds"], lam=True)
    assert np.array_equal(s.sens_adjoint(ca["seeds"]), g0, equal_nan=True)


@pytest.mark.gpu
def test_torch_layer_gradients(ca):
    import torch
    ag = importlib.import_module(pkg.__name__ + ".autograd")
    cfg, B, s = ca["cfg"], ca["B"], solver_for(ca["cfg"])
    dev = torch.device("cuda")
    x0, p, obst = ca["x0"], ca["p"], ca["obst"]
    wts_np = np.random.default_rng(36).normal(size=(B, cfg.n_w))
    tx0, wts = torch.from_numpy(x0).to(dev), torch.from_numpy(wts_np).to(dev)
    # gradients to obst and p from one backward pass
    tp = torch.from_numpy(p).to(dev).requires_grad_(True)
    tob = torch.from_numpy(obst).to(dev).requires_grad_(True)
    x, st = ag.mpc_solve(s, tx0, tp, obst=tob)
    (wts * x).sum().backward()
    assert np.array_equal(st.cpu().numpy(), ca["r"].status) and np.array_equal(x.detach().cpu().numpy(), ca["r"].x)
    s.solve(x0, p, obst, lam_p=True)
    want_o, want_p = s.sens_obst(seed_w=wts_np).grad_obst, s.sens_adjoint(wts_np)
    assert np.allclose(tob.grad.cpu().numpy(), want_o, rtol=1e-12, atol=1e-12, equal_nan=True)
    assert np.allclose(tp.grad.cpu().numpy(), want_p, rtol=1e-12, atol=1e-12, equal_nan=True)
    conv = ca["r"].status == 1
    assert np.all(np.isfinite(want_o[conv])) and np.max(np.abs(want_o[conv])) > 1e-3
    # through the pose of the obstacle: obstacle_centres is loop_obstacle_centres in torch
    off = 1.0
    pose_np = np.stack([obst[:, 0], obst[:, 1], np.full(B, 0.07759)], axis=1)
    pose = torch.from_numpy(pose_np).to(dev).requires_grad_(True)
    cen = ag.obstacle_centres(pose, off)
    cs, sn = np.cos(pose_np[:, 2]), np.sin(pose_np[:, 2])
    cen_np = np.stack([pose_np[:, 0], pose_np[:, 1], pose_np[:, 0] + off * cs, pose_np[:, 1] + off * sn, pose_np[:, 0] - off * cs,
                       pose_np[:, 1] - off * sn], axis=1)
    assert np.allclose(cen.detach().cpu().numpy(), cen_np, rtol=0, atol=1e-14)
    x2, st2 = ag.mpc_solve(s, tx0, torch.from_numpy(p).to(dev), failed="zero", obst=cen)
    (wts * x2).sum().backward()
    s.solve(x0, p, cen_np, lam_p=True)
    go = np.nan_to_num(s.sens_obst(seed_w=wts_np).grad_obst)
    go[st2.cpu().numpy() != 1] = 0.0
    want_pose = np.stack([go[:, 0] + go[:, 2] + go[:, 4], go[:, 1] + go[:, 3] + go[:, 5],
                          off * (-sn * (go[:, 2] - go[:, 4]) + cs * (go[:, 3] - go[:, 5]))], axis=1)
    assert np.allclose(pose.grad.cpu().numpy(), want_pose, rtol=1e-10, atol=1e-10)
    # obst=None: the layer of before, the same bits as the adjoint through the C-ABI
    tp3 = torch.from_numpy(p).to(dev).requires_grad_(True)
    x3, _ = ag.mpc_solve(s, tx0, tp3)
    (wts * x3).sum().backward()
    s.solve(x0, p, lam_p=True)
    assert np.array_equal(tp3.grad.cpu().numpy(), s.sens_adjoint(wts_np), equal_nan=True)
    # backward after another solve raises, for obst as for p
    tob4 = torch.from_numpy(obst).to(dev).requires_grad_(True)
    x4, _ = ag.mpc_solve(s, tx0, torch.from_numpy(p).to(dev), obst=tob4)
    s.solve(x0[:4], p[:4])
    with pytest.raises(Exception):
        x4.sum().backward()
