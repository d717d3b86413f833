"""GPU: the derivative of the optimum with respect to the seven cost weights wt = [Q_0 .. Q_4 | R_0, R_1] -- forward dw = (dw*/dwt) dwt, the
adjoint grad_wt, lam_wt and the torch layer (mpc_sens_weights[_dev], autograd.py) -- and the weights of a live handle (mpc_set_weights);
DESIGN.md section 13.

Shapes: the collision-avoidance family (N = 30, nx = 5) at B = 70, one full 64-lane block and a partial second one, rows 0-5 and 64-69
compared with the active-set derivative of the numpy NLP (tests/sens_weights_ref.py); lane following (N = 10, nx = 6) at B = 8, every row."""
import ctypes as C
import dataclasses
import importlib

import numpy as np
import pytest

import sens_weights_ref as wref
from helpers import CA_CFG, NLPConfig, WEIGHTS_ZAM_LF, ca_batch, make_solver, pkg, set_cfg_bounds, straight_path, synthetic_batch
from sens_weights_ref import TOL_DW

MPC_ERR_INVALID, MPC_ERR_STATE = -1, -4
N_DIR = 8
LF_CFG = NLPConfig(N=10, nx=6, **WEIGHTS_ZAM_LF)
SOLVE_FIELDS = ("x", "status", "iters", "kkt", "f", "g", "lam_g", "lam_x")


def solver_for(cfg, **kw):
    s = make_solver(cfg, **kw)
    set_cfg_bounds(s, cfg)
    return s


def directions(cfg, B, seed):
    """the seven log-directions wt_q e_q and one random relative direction"""
    wt = wref.weights_of(cfg)
    d = np.zeros((B, N_DIR, 7))
    d[:, :7] = np.diag(wt)
    d[:, 7] = wt * np.random.default_rng(seed).normal(size=(B, 7))
    return d


def check_nan_rule(status, lam_g, dw, grad, lam):
    kink = np.isnan(lam_g[:, 0]) & (status == 1)
    bad = (status != 1) | kink
    assert np.all(np.isnan(dw[bad])) and np.all(np.isnan(grad[bad])) and np.all(np.isnan(lam[bad]))
    good = ~bad
    assert np.all(np.isfinite(dw[good])) and np.all(np.isfinite(grad[good])) and np.all(np.isfinite(lam[good]))
    return good


def check_adjoint(good, seeds, dw, grad, dwt):
    worst = 0.0
    for b in np.flatnonzero(good):
        for d in range(dwt.shape[1]):
            lhs, rhs = seeds[b] @ dw[b, d], grad[b] @ dwt[b, d]
            scale = max(1.0, np.abs(seeds[b]).sum() * np.max(np.abs(dw[b, d])))
            worst = max(worst, abs(lhs - rhs) / scale)
            assert abs(lhs - rhs) <= 1e-10 * scale, (b, d, lhs, rhs)
    print(f"\n  adjoint identity over {int(good.sum())} rows: worst scaled difference {worst:.2e}")


def check_reference(c, good, dw, lam):
    """lam_wt of the compared good rows and dw of the strictly complementary ones against numpy; returns (rows compared, good rows among the
    rows to compare)"""
    cfg, r = c["cfg"], c["r"]
    checked, worst, worst_lam, n_good = 0, 0.0, 0.0, 0
    for b in c["rows"]:
        if not good[b]:
            continue
        n_good += 1
        lw = wref.lam_weights(cfg, r.x[b], c["p"][b])
        err = np.max(np.abs(lam[b] - lw) / np.maximum(1.0, np.abs(lw)))
        worst_lam = max(worst_lam, err)
        assert err <= 1e-12, (b, lam[b], lw)
        S, weak = c["ref"][b]
        if weak:
            continue
        want = np.einsum("ij,dj->di", S, c["dwt"][b])
        for d in range(N_DIR):
            err = np.max(np.abs(dw[b, d] - want[d])) / np.max(np.abs(want[d]))
            assert np.isfinite(err) and err <= TOL_DW, (b, d, err)
            worst = max(worst, err)
        checked += 1
    print(f"\n  dw vs numpy: {checked} of {n_good} rows checked, worst max|dw - want| / max|want| {worst:.2e} (bound {TOL_DW:.1e}); "
          f"lam_wt worst relative error {worst_lam:.2e}")
    return checked, n_good


def make_case(cfg, x0, p, rows, seed):
    """a batch solved once through the host-pointer form, its weights derivative, and the numpy reference of the rows to compare"""
    B = x0.shape[0]
    dwt = directions(cfg, B, seed)
    seeds = np.random.default_rng(seed + 1).normal(size=(B, cfg.n_w))
    s = solver_for(cfg)
    r = s.solve(x0, p, multipliers=True, lam_p=True)
    o = s.sens_weights(p, dwt, seeds, lam=True)
    ref = {int(b): wref.sensitivity_matrix(cfg, r.x[b], p[b], r.lam_g[b], r.lam_x[b]) for b in rows if r.status[b] == 1}
    return dict(cfg=cfg, B=B, x0=x0, p=p, rows=list(rows), dwt=dwt, seeds=seeds, solver=s, r=r, o=o, ref=ref)


@pytest.fixture(scope="module")
def ca():
    x0, p = ca_batch(CA_CFG, 70)
    return make_case(CA_CFG, x0, p, list(range(6)) + list(range(64, 70)), 51)


@pytest.fixture(scope="module")
def lf():
    x0, p = synthetic_batch(LF_CFG, 8)
    return make_case(LF_CFG, x0, p, range(8), 53)


def host_form_checks(c):
    r, o, s = c["r"], c["o"], c["solver"]
    good = check_nan_rule(r.status, r.lam_g, o.dw, o.grad_wt, o.lam_wt)
    checked, n_good = check_reference(c, good, o.dw, o.lam_wt)
    assert checked >= (n_good + 1) // 2, (checked, n_good)
    check_adjoint(good, c["seeds"], o.dw, o.grad_wt, c["dwt"])
    # every part alone gives the same bits
    assert np.array_equal(s.sens_weights(c["p"], c["dwt"]).dw, o.dw, equal_nan=True)
    assert np.array_equal(s.sens_weights(c["p"], seed_w=c["seeds"]).grad_wt, o.grad_wt, equal_nan=True)
    assert np.array_equal(s.sens_weights(c["p"], lam=True).lam_wt, o.lam_wt, equal_nan=True)
    return good


@pytest.mark.gpu
def test_host_form_collision_avoidance(ca):
    r = ca["r"]
    assert np.sum(r.status[ca["rows"]] == 1) >= 9
    nlp_rows = 1 + ca["cfg"].nx * (ca["cfg"].N + 1)
    assert np.min(r.lam_g[r.status == 1][:, nlp_rows:]) < -1e-3                       # active circle rows
    good = host_form_checks(ca)
    assert np.max(np.abs(ca["o"].dw[good])) > 0.1                                     # the plan moves with the weights


@pytest.mark.gpu
def test_host_form_lane_following_nx6(lf):
    assert np.all(lf["r"].status == 1)
    good = host_form_checks(lf)
    assert np.all(good)
    assert np.max(np.abs(lf["o"].dw[:, :, 2 * LF_CFG.N + 5::6])) > 1e-3                # the progress state (nx = 6) moves with the weights too


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["ca", "lf"])
def test_device_form_on_a_stream(which, request):
    """a _sens solve with no sensitivity output is enough for the snapshot; the _dev form on a side stream gives the host form's bits"""
    import torch
    c = request.getfixturevalue(which)
    cfg, B, s = c["cfg"], c["B"], solver_for(c["cfg"])
    dev = torch.device("cuda")
    t = {k: torch.from_numpy(np.ascontiguousarray(c[k])).to(dev) for k in ("x0", "p", "dwt", "seeds")}
    tx, tst = torch.empty_like(t["x0"]), torch.empty(B, dtype=torch.int32, device=dev)
    tdw = torch.empty((B, N_DIR, cfg.n_w), dtype=torch.float64, device=dev)
    tgw, tlw = torch.empty((B, 7), dtype=torch.float64, device=dev), torch.empty((B, 7), dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        s.solve_sens_device(B, t["x0"].data_ptr(), t["p"].data_ptr(), tx.data_ptr(), d_status=tst.data_ptr(), stream=stream.cuda_stream)
        before = tx.clone()
        s.sens_weights_device(B, t["p"].data_ptr(), N_DIR, t["dwt"].data_ptr(), tdw.data_ptr(), t["seeds"].data_ptr(), tgw.data_ptr(), tlw.data_ptr(),
                              stream=stream.cuda_stream)
    stream.synchronize()
    r, o = c["r"], c["o"]
    assert torch.equal(before, tx)
    assert np.array_equal(tx.cpu().numpy(), r.x) and np.array_equal(tst.cpu().numpy(), r.status)
    assert np.array_equal(tdw.cpu().numpy(), o.dw, equal_nan=True)
    assert np.array_equal(tgw.cpu().numpy(), o.grad_wt, equal_nan=True)
    assert np.array_equal(tlw.cpu().numpy(), o.lam_wt, equal_nan=True)


@pytest.mark.gpu
def test_rows_that_did_not_converge_are_nan(lf):
    s = solver_for(lf["cfg"], max_iter=2)
    r = s.solve(lf["x0"], lf["p"], lam_p=True)
    assert np.all(r.status != 1)
    o = s.sens_weights(lf["p"], lf["dwt"], lf["seeds"], lam=True)
    assert np.all(np.isnan(o.dw)) and np.all(np.isnan(o.grad_wt)) and np.all(np.isnan(o.lam_wt))


@pytest.mark.gpu
def test_call_order_and_arguments(lf):
    cfg, B, s = lf["cfg"], lf["B"], solver_for(lf["cfg"])
    L = s._lib
    dptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    p, dwt, seeds = np.ascontiguousarray(lf["p"]), np.ascontiguousarray(lf["dwt"]), np.ascontiguousarray(lf["seeds"])
    dw, gw, lw = np.empty((B, N_DIR, cfg.n_w)), np.empty((B, 7)), np.empty((B, 7))
    call = lambda B_, p_, nd, dd, w, se, g, l: L.mpc_sens_weights(s._h, B_, p_, nd, dd, w, se, g, l)  # noqa: E731
    full = lambda: call(B, dptr(p), N_DIR, dptr(dwt), dptr(dw), dptr(seeds), dptr(gw), dptr(lw))  # noqa: E731
    # no snapshot yet
    assert full() == MPC_ERR_STATE
    s.solve(lf["x0"], lf["p"], lam_p=True)
    assert full() == 0
    # bad arguments: no p, a seed without its gradient and the reverse, directions without both arrays, a negative count
    assert call(B, None, 0, None, None, None, None, dptr(lw)) == MPC_ERR_INVALID
    assert b"p " in L.mpc_last_error(s._h)
    assert call(B, dptr(p), 0, None, None, dptr(seeds), None, None) == MPC_ERR_INVALID
    assert b"seed_w" in L.mpc_last_error(s._h)
    assert call(B, dptr(p), 0, None, None, None, dptr(gw), None) == MPC_ERR_INVALID
    assert call(B, dptr(p), N_DIR, dptr(dwt), None, None, None, None) == MPC_ERR_INVALID
    assert call(B, dptr(p), N_DIR, None, dptr(dw), None, None, None) == MPC_ERR_INVALID
    assert call(B, dptr(p), -1, None, None, None, None, dptr(lw)) == MPC_ERR_INVALID
    assert b"n_dir" in L.mpc_last_error(s._h)
    # another B, then an intervening plain solve: the snapshot is not this call's
    assert call(B - 1, dptr(p), 0, None, None, None, None, dptr(lw)) == MPC_ERR_STATE
    assert call(B, dptr(p), 0, None, None, None, None, dptr(lw)) == 0
    s.solve(lf["x0"][:4], lf["p"][:4])
    assert call(B, dptr(p), 0, None, None, None, None, dptr(lw)) == MPC_ERR_STATE
    # set_weights ends the snapshot's life as a solve does, for every entry that factors it; the same weights again make no difference
    s.solve(lf["x0"], lf["p"], lam_p=True)
    assert full() == 0
    s.set_weights(s.weights[:5], s.weights[5:])
    assert full() == MPC_ERR_STATE
    with pytest.raises(pkg.MpcError) as e:
        s.sens_weights(lf["p"], lam=True)
    assert e.value.code == MPC_ERR_STATE
    with pytest.raises(pkg.MpcError) as e:
        s.sens_adjoint(seeds)
    assert e.value.code == MPC_ERR_STATE
    # ... and the next _sens solve brings it back, with the host form's bits
    s.solve(lf["x0"], lf["p"], lam_p=True)
    assert full() == 0
    assert np.array_equal(dw, lf["o"].dw) and np.array_equal(gw, lf["o"].grad_wt) and np.array_equal(lw, lf["o"].lam_wt)


@pytest.mark.gpu
def test_set_weights_equals_a_handle_created_with_them(ca):
    """a handle created with the lane-following weights and then given the collision-avoidance ones against a handle created with those:
    plain solve, _ex, a short closed loop; invalid weights change nothing; lam_p_of follows"""
    cfg = ca["cfg"]
    wt_lf, wt_ca = wref.weights_of(LF_CFG), wref.weights_of(cfg)
    x0, p = ca["x0"], ca["p"]
    s = solver_for(wref.with_weights(cfg, wt_lf))
    assert np.array_equal(s.weights, wt_lf)
    other = s.solve(x0, p)
    s.set_weights(wt_ca[:5], wt_ca[5:])
    assert np.array_equal(s.weights, wt_ca)
    a, r = s.solve(x0, p), ca["r"]
    assert not np.array_equal(other.x, a.x)
    for fld in ("x", "status", "iters", "kkt"):
        assert np.array_equal(getattr(a, fld), getattr(r, fld), equal_nan=True), fld
    ex = s.solve(x0, p, multipliers=True)
    for fld in SOLVE_FIELDS:
        assert np.array_equal(getattr(ex, fld), getattr(r, fld), equal_nan=True), fld
    # lam_p_of computes with the weights on the Python side
    assert np.array_equal(s.lam_p_of(ex.x, p, ex.lam_g, ex.status), r.lam_p, equal_nan=True)
    # Q alone, R alone
    s.set_weights(Q=wt_lf[:5])
    assert np.array_equal(s.weights, np.concatenate([wt_lf[:5], wt_ca[5:]]))
    s.set_weights(R=wt_lf[5:])
    assert np.array_equal(s.weights, wt_lf)
    assert np.array_equal(s.solve(x0, p).x, other.x, equal_nan=True)
    s.set_weights(wt_ca[:5], wt_ca[5:])
    # invalid weights: MPC_ERR_INVALID, the handle as it was
    nan, inf = float("nan"), float("inf")
    for Q, R in (([1, 1, -1e-300, 1, 1], None), ([1, nan, 1, 1, 1], None), (None, [0.0, 1.0]), (None, [1.0, -2.0]), (None, [inf, 1.0]),
                 ([1, 1, 1, 1, inf], [1.0, 1.0]), (wt_lf[:5], [1.0, nan])):
        with pytest.raises(pkg.MpcError) as e:
            s.set_weights(Q, R)
        assert e.value.code == MPC_ERR_INVALID
        assert np.array_equal(s.weights, wt_ca)
    assert np.array_equal(s.solve(x0, p).x, r.x, equal_nan=True)
    # a zero Q entry is allowed (Q >= 0)
    s.set_weights(Q=[2.3, 2.3, 500.0, 0.0, 160.0])
    assert s.weights[3] == 0.0
    # a short closed loop: N = 10, ten steps (the driver asks for L >= N), three egos
    cfg10 = dataclasses.replace(cfg, N=10)
    N, L, B = 10, 10, 3
    path, orient = straight_path(L + N + 1, 29.9948, -1.1501, 0.03495, 20.0)
    init = np.tile([29.9948, -1.1501, 0.0, 20.0, 0.03495], (B, 1))
    init[:, 1] += [0.0, 0.3, -0.4]
    args = (init, np.tile(path, (B, 1, 1)), np.tile(orient, (B, 1)), np.full(B, 20.0), L)
    want = solver_for(cfg10).closed_loop(*args)
    s10 = solver_for(wref.with_weights(cfg10, wt_lf))
    before = s10.closed_loop(*args)
    s10.set_weights(wt_ca[:5], wt_ca[5:])
    got = s10.closed_loop(*args)
    assert not np.array_equal(before[0], got[0])
    for g, w in zip(got, want):
        assert np.array_equal(g, w, equal_nan=True)


@pytest.mark.gpu
def test_solve_and_other_sensitivities_keep_their_bits(ca):
    """x_out .. lam_p, dw of mpc_solve_batch_sens are the same bits whether or not mpc_sens_weights runs afterwards, and mpc_sens_adjoint /
    mpc_sens_obst on the same snapshot are not disturbed by it (they share the factor storage and the solves' scratch)"""
    cfg, B, s = ca["cfg"], ca["B"], solver_for(ca["cfg"])
    dp = np.zeros((B, 2, cfg.n_w))
    dp[:, 0] = np.random.default_rng(55).normal(size=(B, cfg.n_w))
    dp[:, 1, 2 * cfg.N + 3] = 1.0
    solve = lambda: s.solve(ca["x0"], ca["p"], multipliers=True, lam_p=True, dp=dp)  # noqa: E731
    a = solve()
    s.sens_weights(ca["p"], ca["dwt"], ca["seeds"], lam=True)
    c = solve()
    for fld in SOLVE_FIELDS + ("lam_p", "dw"):
        assert np.array_equal(getattr(a, fld), getattr(c, fld), equal_nan=True), fld
        if fld != "dw":
            assert np.array_equal(getattr(a, fld), getattr(ca["r"], fld), equal_nan=True), fld
    dobst = np.random.default_rng(56).normal(size=(B, 2, 6))
    g0, o0 = s.sens_adjoint(ca["seeds"]), s.sens_obst(dobst, ca["seeds"], lam=True)
    w0 = s.sens_weights(ca["p"], ca["dwt"], ca["seeds"], lam=True)
    assert np.array_equal(s.sens_adjoint(ca["seeds"]), g0, equal_nan=True)
    o1 = s.sens_obst(dobst, ca["seeds"], lam=True)
    for fld in ("dw", "grad_obst", "lam_obst"):
        assert np.array_equal(getattr(o0, fld), getattr(o1, fld), equal_nan=True), fld
    for fld in ("dw", "grad_wt", "lam_wt"):
        assert np.array_equal(getattr(w0, fld), getattr(ca["o"], fld), equal_nan=True), fld


@pytest.mark.gpu
def test_torch_layer_gradients(lf, ca):
    import torch
    ag = importlib.import_module(pkg.__name__ + ".autograd")
    dev = torch.device("cuda")
    # -- lane following: wt.grad of loss = sum |x*(wt) - x_target|^2 against central differences of the loss over re-solves
    cfg, B, x0, p = lf["cfg"], lf["B"], lf["x0"], lf["p"]
    s = solver_for(cfg)
    wt0 = wref.weights_of(cfg)
    tx0, tp = torch.from_numpy(x0).to(dev), torch.from_numpy(p).to(dev)
    s.set_weights(*np.split(wt0 * (1.0 + 0.4 * np.random.default_rng(57).uniform(-1, 1, 7)), [5]))
    target = s.solve(x0, p)
    assert np.all(target.status == 1)
    xt = torch.from_numpy(target.x).to(dev)

    def loss_at(wt):
        s.set_weights(wt[:5], wt[5:])
        r = s.solve(x0, p)
        assert np.all(r.status == 1)
        return float(((r.x - target.x) ** 2).sum())

    fd = np.zeros(7)
    for q in range(7):
        e = np.zeros(7)
        e[q] = 1e-4 * wt0[q]
        fd[q] = (loss_at(wt0 + e) - loss_at(wt0 - e)) / (2 * e[q])
    wt = torch.tensor(wt0, dtype=torch.float64, requires_grad=True)                   # a host tensor
    x, st = ag.mpc_solve(s, tx0, tp, weights=wt)
    assert np.array_equal(s.weights, wt0)
    ((x - xt) ** 2).sum().backward()
    got = wt.grad.numpy()
    print(f"\n  lane following: wt.grad {got}\n  central differences {fd}\n  worst |difference| / max(1, |fd|) {np.max(np.abs(got - fd) / np.maximum(1.0, np.abs(fd))):.2e}")
    assert np.all(np.abs(got - fd) <= 1e-3 * np.maximum(1.0, np.abs(fd))), (got, fd)
    assert np.max(np.abs(got * wt0)) > 1e-3                                           # (the loss does depend on the weights)
    # ... it is sens_weights(seed_w = dloss/dx) summed over the rows; a device tensor gives the same, on its device
    seed = 2.0 * (x.detach().cpu().numpy() - target.x)
    s.solve(x0, p, lam_p=True)
    rows = s.sens_weights(p, seed_w=seed).grad_wt
    assert np.allclose(got, rows.sum(axis=0), rtol=1e-12, atol=1e-12)
    wtd = torch.tensor(wt0, dtype=torch.float64, device=dev, requires_grad=True)
    xd, _ = ag.mpc_solve(s, tx0, tp, weights=wtd)
    ((xd - xt) ** 2).sum().backward()
    assert wtd.grad.is_cuda and np.array_equal(wtd.grad.cpu().numpy(), got)
    # weights=None: the layer of before, the same bits as the adjoint through the C-ABI, and the solver's weights are not touched
    wts_np = np.random.default_rng(58).normal(size=(B, cfg.n_w))
    wts = torch.from_numpy(wts_np).to(dev)
    tp3 = torch.from_numpy(p).to(dev).requires_grad_(True)
    x3, _ = ag.mpc_solve(s, tx0, tp3)
    (wts * x3).sum().backward()
    assert np.array_equal(x3.detach().cpu().numpy(), lf["r"].x) and np.array_equal(s.weights, wt0)
    s.solve(x0, p, lam_p=True)
    assert np.array_equal(tp3.grad.cpu().numpy(), s.sens_adjoint(wts_np), equal_nan=True)
    # gradients to p and the weights from one backward pass
    tp4 = torch.from_numpy(p).to(dev).requires_grad_(True)
    wt4 = torch.tensor(wt0, dtype=torch.float64, requires_grad=True)
    x4, _ = ag.mpc_solve(s, tx0, tp4, weights=wt4)
    (wts * x4).sum().backward()
    s.solve(x0, p, lam_p=True)
    assert np.array_equal(tp4.grad.cpu().numpy(), s.sens_adjoint(wts_np), equal_nan=True)
    assert np.allclose(wt4.grad.numpy(), s.sens_weights(p, seed_w=wts_np).grad_wt.sum(axis=0), rtol=1e-12, atol=1e-12)
    # backward after set_weights or another solve raises
    wt5 = torch.tensor(wt0, dtype=torch.float64, requires_grad=True)
    x5, _ = ag.mpc_solve(s, tx0, tp, weights=wt5)
    s.set_weights(R=wt0[5:])
    with pytest.raises(Exception):
        x5.sum().backward()
    # -- failed="zero" with one row forced to fail (a NaN in its reference): a finite gradient, the sum over the other rows; "nan": NaN
    p_bad = p.copy()
    p_bad[3, 2 * cfg.N + cfg.nx + 1] = np.nan
    tpb = torch.from_numpy(p_bad).to(dev)
    for failed in ("zero", "nan"):
        wt6 = torch.tensor(wt0, dtype=torch.float64, requires_grad=True)
        x6, st6 = ag.mpc_solve(s, tx0, tpb, failed=failed, weights=wt6)
        stn = st6.cpu().numpy()
        assert stn[3] != 1 and np.all(np.delete(stn, 3) == 1)
        (wts * torch.nan_to_num(x6)).sum().backward()
        if failed == "nan":
            assert np.all(np.isnan(wt6.grad.numpy()))
            continue
        s.solve(x0, p_bad, lam_p=True)
        rows = s.sens_weights(p_bad, seed_w=wts_np).grad_wt
        assert np.all(np.isnan(rows[3])) and np.all(np.isfinite(wt6.grad.numpy()))
        assert np.allclose(wt6.grad.numpy(), np.delete(rows, 3, axis=0).sum(axis=0), rtol=1e-12, atol=1e-12)
    # -- collision avoidance, eight rows: the layer's gradient is the C-ABI's adjoint summed over the converged rows
    cfg, x0, p = ca["cfg"], ca["x0"][:8], ca["p"][:8]
    s = solver_for(cfg)
    wts_np = np.random.default_rng(59).normal(size=(8, cfg.n_w))
    wt7 = torch.tensor(wref.weights_of(cfg), dtype=torch.float64, requires_grad=True)
    x7, st7 = ag.mpc_solve(s, torch.from_numpy(x0).to(dev), torch.from_numpy(p).to(dev), failed="zero", weights=wt7)
    (torch.from_numpy(wts_np).to(dev) * torch.nan_to_num(x7)).sum().backward()
    assert np.array_equal(st7.cpu().numpy(), ca["r"].status[:8])
    s.solve(x0, p, lam_p=True)
    rows = s.sens_weights(p, seed_w=wts_np).grad_wt
    conv = ca["r"].status[:8] == 1
    assert conv.sum() >= 6 and np.all(np.isfinite(wt7.grad.numpy()))
    assert np.allclose(wt7.grad.numpy(), rows[conv].sum(axis=0), rtol=1e-12, atol=1e-12 * np.max(np.abs(rows[conv])))
