"""GPU: the derivative of the optimum with respect to the bounds and the circle radius, bv = [lbx (n_w) | ubx (n_w) | fl, fu, ol, ou] -- forward
dw = (dw*/dbv) dbv, the adjoint grad_bv, lam_bv and the torch layer (mpc_sens_bounds[_dev], autograd.py) -- the bounds a handle holds
(mpc_get_bounds), and mpc_set_bounds ending the life of the sensitivity snapshot; DESIGN.md section 13.

Shapes: the collision-avoidance family (N = 30, nx = 5) at B = 70, one full 64-lane block and a partial second one, rows 0-5 and 64-69
compared with the active-set derivative of the numpy NLP (tests/sens_bounds_ref.py); lane following (N = 10, nx = 6) at B = 8, every row."""
import ctypes as C
import importlib

import numpy as np
import pytest

import sens_bounds_ref as bref
from helpers import CA_CFG, BicycleNLP, NLPConfig, WEIGHTS_ZAM_LF, ca_batch, make_solver, pkg, set_cfg_bounds, synthetic_batch
from sens_bounds_ref import TOL_DW

MPC_ERR_INVALID, MPC_ERR_STATE = -1, -4
N_DIR = 10
WANT_FLOOR = 0.1                # of the error's denominator (tests/test_sens_bounds_cpu.py)
LF_CFG = NLPConfig(N=10, nx=6, **WEIGHTS_ZAM_LF)
D_DELTAV_MIN, D_DELTAV_MAX, D_FU, D_OL = 0, 1, 7, 8


def solver_for(cfg, **kw):
    s = make_solver(cfg, **kw)
    set_cfg_bounds(s, cfg)
    return s


def directions(cfg, B, seed):
    """the nine level directions and one random per-entry direction with entries in [-1, 1]"""
    d = np.zeros((B, N_DIR, bref.n_b(cfg)))
    d[:, :9] = bref.level_directions(cfg)
    d[:, 9] = np.random.default_rng(seed).uniform(-1.0, 1.0, size=(B, bref.n_b(cfg)))
    return d


def absent_entries(cfg):
    """entries of bv whose bound is absent (+-inf) or not imposed (fl under the default friction_lb = nlp)"""
    absent = ~np.isfinite(bref.bounds_vector(cfg))
    absent[2 * cfg.n_w + bref.FL] = True
    return absent


def check_nan_rule(status, lam_g, dw, grad, lam):
    kink = np.isnan(lam_g[:, 0]) & (status == 1)
    bad = (status != 1) | kink
    assert np.all(np.isnan(dw[bad])) and np.all(np.isnan(grad[bad])) and np.all(np.isnan(lam[bad]))
    good = ~bad
    assert np.all(np.isfinite(dw[good])) and np.all(np.isfinite(grad[good])) and np.all(np.isfinite(lam[good]))
    return good


def check_adjoint(good, seeds, dw, grad, dbv):
    worst = 0.0
    for b in np.flatnonzero(good):
        for d in range(dbv.shape[1]):
            lhs, rhs = seeds[b] @ dw[b, d], grad[b] @ dbv[b, d]
            scale = max(1.0, np.abs(seeds[b]).sum() * np.max(np.abs(dw[b, d])))
            worst = max(worst, abs(lhs - rhs) / scale)
            assert abs(lhs - rhs) <= 1e-10 * scale, (b, d, lhs, rhs)
    print(f"\n  adjoint identity over {int(good.sum())} rows: worst scaled difference {worst:.2e}")


def check_lam(c, good, lam):
    """the three sum identities with the solve's own multipliers to 1e-12 relative, the signs, and exact zeros at absent bounds"""
    cfg, r = c["cfg"], c["r"]
    nw, first = cfg.n_w, 1 + cfg.nx * (cfg.N + 1)
    worst = 0.0
    for b in np.flatnonzero(good):
        lb, lg, lx = lam[b], r.lam_g[b], r.lam_x[b]
        pairs = [(lb[:nw] + lb[nw: 2 * nw], -lx), (lb[2 * nw] + lb[2 * nw + 1], -lg[0]), (lb[2 * nw + 2] + lb[2 * nw + 3], -lg[first:].sum())]
        for got, want in pairs:
            err = np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))
            worst = max(worst, err)
            assert err <= 1e-12, (b, got, want)
        assert np.all(lb[:nw] >= 0.0) and np.all(lb[nw: 2 * nw] <= 0.0)
        assert lb[2 * nw] >= 0.0 and lb[2 * nw + 1] <= 0.0 and lb[2 * nw + 2] >= 0.0 and lb[2 * nw + 3] <= 0.0
    assert np.all(lam[good][:, absent_entries(cfg)] == 0.0)
    print(f"\n  lam_bv sum identities over {int(good.sum())} rows: worst relative difference {worst:.2e}")


def check_reference(c, good, dw):
    """dw of the strictly complementary compared rows against numpy; returns (rows compared, good rows among the rows to compare, per compared
    row the max|dw| of every direction)"""
    cfg = c["cfg"]
    finite = np.isfinite(bref.bounds_vector(cfg))
    checked, worst, n_good, resp = 0, 0.0, 0, []
    for b in c["rows"]:
        if not good[b]:
            continue
        n_good += 1
        S, weak = c["ref"][b]
        if weak:
            continue
        want = np.einsum("ij,dj->di", S, np.where(finite, c["dbv"][b], 0.0))            # (an absent bound's entry is not read)
        for d in range(N_DIR):
            err = np.max(np.abs(dw[b, d] - want[d])) / max(np.max(np.abs(want[d])), WANT_FLOOR)
            worst = max(worst, err)
            print(f"  row {b} direction {d}: error {err:.2e}, max|dw| {np.max(np.abs(dw[b, d])):.3g}")
            assert np.isfinite(err) and err <= TOL_DW, (b, d, err)
        resp.append(np.max(np.abs(dw[b]), axis=1))
        checked += 1
    print(f"\n  dw vs numpy: {checked} of {n_good} rows checked, worst max|dw - want| / max(max|want|, 0.1) {worst:.2e} (bound {TOL_DW:.1e})")
    return checked, n_good, np.array(resp)


def make_case(cfg, x0, p, rows, seed):
    """a batch solved once through the host-pointer form, its bounds derivative, and the numpy reference of the rows to compare"""
    B = x0.shape[0]
    dbv = directions(cfg, B, seed)
    seeds = np.random.default_rng(seed + 1).normal(size=(B, cfg.n_w))
    s = solver_for(cfg)
    r = s.solve(x0, p, multipliers=True, lam_p=True)
    o = s.sens_bounds(dbv, seeds, lam=True)
    ref = {int(b): bref.sensitivity_matrix(cfg, r.x[b], p[b], r.lam_g[b], r.lam_x[b]) for b in rows if r.status[b] == 1}
    return dict(cfg=cfg, B=B, x0=x0, p=p, rows=list(rows), dbv=dbv, seeds=seeds, solver=s, r=r, o=o, ref=ref)


@pytest.fixture(scope="module")
def ca():
    x0, p = ca_batch(CA_CFG, 70)
    return make_case(CA_CFG, x0, p, list(range(6)) + list(range(64, 70)), 71)


@pytest.fixture(scope="module")
def lf():
    x0, p = synthetic_batch(LF_CFG, 8)
    return make_case(LF_CFG, x0, p, range(8), 73)


def host_form_checks(c):
    r, o, s = c["r"], c["o"], c["solver"]
    good = check_nan_rule(r.status, r.lam_g, o.dw, o.grad_bv, o.lam_bv)
    checked, n_good, resp = check_reference(c, good, o.dw)
    assert checked >= (n_good + 1) // 2, (checked, n_good)
    check_adjoint(good, c["seeds"], o.dw, o.grad_bv, c["dbv"])
    check_lam(c, good, o.lam_bv)
    assert np.all(o.grad_bv[good][:, absent_entries(c["cfg"])] == 0.0)
    # every part alone gives the same bits
    assert np.array_equal(s.sens_bounds(c["dbv"]).dw, o.dw, equal_nan=True)
    assert np.array_equal(s.sens_bounds(seed_w=c["seeds"]).grad_bv, o.grad_bv, equal_nan=True)
    assert np.array_equal(s.sens_bounds(lam=True).lam_bv, o.lam_bv, equal_nan=True)
    # the dbv entry of an absent bound is not read
    moved = c["dbv"].copy()
    moved[:, :, absent_entries(c["cfg"])] = np.nan
    assert np.array_equal(s.sens_bounds(moved).dw, o.dw, equal_nan=True)
    return good, resp


@pytest.mark.gpu
def test_host_form_collision_avoidance(ca):
    r = ca["r"]
    assert np.sum(r.status[ca["rows"]] == 1) >= 9
    good, resp = host_form_checks(ca)
    # the compared rows exercise it: the radius and the steering-rate limits move every plan, the friction limit at least six
    assert np.all(resp[:, [D_OL, D_DELTAV_MIN, D_DELTAV_MAX]] > 0.1), resp[:, [D_OL, D_DELTAV_MIN, D_DELTAV_MAX]]
    assert np.sum(resp[:, D_FU] > 0.01) >= 6, resp[:, D_FU]


@pytest.mark.gpu
def test_host_form_lane_following_nx6(lf):
    assert np.all(lf["r"].status == 1)
    good, resp = host_form_checks(lf)
    assert np.all(good)
    assert np.max(np.abs(lf["o"].dw[:, D_DELTAV_MIN, 2 * LF_CFG.N + 5::6])) > 1e-3      # the progress state (nx = 6) moves with a steering-rate limit


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["ca", "lf"])
def test_device_form_on_a_stream(which, request):
    """a _sens solve with no sensitivity output is enough for the snapshot; the _dev form on a side stream gives the host form's bits"""
    import torch
    c = request.getfixturevalue(which)
    cfg, B, s = c["cfg"], c["B"], solver_for(c["cfg"])
    nb = bref.n_b(cfg)
    dev = torch.device("cuda")
    t = {k: torch.from_numpy(np.ascontiguousarray(c[k])).to(dev) for k in ("x0", "p", "dbv", "seeds")}
    tx, tst = torch.empty_like(t["x0"]), torch.empty(B, dtype=torch.int32, device=dev)
    tdw = torch.empty((B, N_DIR, cfg.n_w), dtype=torch.float64, device=dev)
    tgb, tlb = torch.empty((B, nb), dtype=torch.float64, device=dev), torch.empty((B, nb), dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        s.solve_sens_device(B, t["x0"].data_ptr(), t["p"].data_ptr(), tx.data_ptr(), d_status=tst.data_ptr(), stream=stream.cuda_stream)
        before = tx.clone()
        s.sens_bounds_device(B, N_DIR, t["dbv"].data_ptr(), tdw.data_ptr(), t["seeds"].data_ptr(), tgb.data_ptr(), tlb.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    r, o = c["r"], c["o"]
    assert torch.equal(before, tx)
    assert np.array_equal(tx.cpu().numpy(), r.x) and np.array_equal(tst.cpu().numpy(), r.status)
    assert np.array_equal(tdw.cpu().numpy(), o.dw, equal_nan=True)
    assert np.array_equal(tgb.cpu().numpy(), o.grad_bv, equal_nan=True)
    assert np.array_equal(tlb.cpu().numpy(), o.lam_bv, equal_nan=True)


@pytest.mark.gpu
def test_rows_that_did_not_converge_are_nan(lf):
    s = solver_for(lf["cfg"], max_iter=2)
    r = s.solve(lf["x0"], lf["p"], lam_p=True)
    assert np.all(r.status != 1)
    o = s.sens_bounds(lf["dbv"], lf["seeds"], lam=True)
    assert np.all(np.isnan(o.dw)) and np.all(np.isnan(o.grad_bv)) and np.all(np.isnan(o.lam_bv))


@pytest.mark.gpu
def test_call_order_and_arguments(lf):
    cfg, B, s = lf["cfg"], lf["B"], solver_for(lf["cfg"])
    L, nb = s._lib, bref.n_b(cfg)
    dptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    p, dbv, seeds = np.ascontiguousarray(lf["p"]), np.ascontiguousarray(lf["dbv"]), np.ascontiguousarray(lf["seeds"])
    dw, gb, lb = np.empty((B, N_DIR, cfg.n_w)), np.empty((B, nb)), np.empty((B, nb))
    call = lambda B_, nd, dd, w, se, g, l: L.mpc_sens_bounds(s._h, B_, nd, dd, w, se, g, l)  # noqa: E731
    full = lambda: call(B, N_DIR, dptr(dbv), dptr(dw), dptr(seeds), dptr(gb), dptr(lb))  # noqa: E731
    # no snapshot yet
    assert full() == MPC_ERR_STATE
    s.solve(lf["x0"], lf["p"], lam_p=True)
    assert full() == 0
    # a call that asks for nothing
    assert call(B, 0, None, None, None, None, None) == 0
    # bad arguments: a seed without its gradient and the reverse, directions without both arrays, a negative count, no rows
    assert call(B, 0, None, None, dptr(seeds), None, None) == MPC_ERR_INVALID
    assert b"seed_w" in L.mpc_last_error(s._h)
    assert call(B, 0, None, None, None, dptr(gb), None) == MPC_ERR_INVALID
    assert call(B, N_DIR, dptr(dbv), None, None, None, None) == MPC_ERR_INVALID
    assert call(B, N_DIR, None, dptr(dw), None, None, None) == MPC_ERR_INVALID
    assert call(B, -1, None, None, None, None, dptr(lb)) == MPC_ERR_INVALID
    assert b"n_dir" in L.mpc_last_error(s._h)
    assert call(0, 0, None, None, None, None, dptr(lb)) == MPC_ERR_INVALID
    # another B, then an intervening plain solve: the snapshot is not this call's
    assert call(B - 1, 0, None, None, None, None, dptr(lb)) == MPC_ERR_STATE
    assert call(B, 0, None, None, None, None, dptr(lb)) == 0
    s.solve(lf["x0"][:4], lf["p"][:4])
    assert call(B, 0, None, None, None, None, dptr(lb)) == MPC_ERR_STATE
    # mpc_set_bounds ends the snapshot's life as a solve does, for every entry that factors it; the same bounds again make no difference
    s.solve(lf["x0"], lf["p"], lam_p=True)
    assert full() == 0
    held = [np.ascontiguousarray(a) for a in s.get_bounds()]
    assert L.mpc_set_bounds(s._h, *[dptr(a) for a in held]) == 0
    assert full() == MPC_ERR_STATE
    assert b"mpc_set_bounds" in L.mpc_last_error(s._h)
    for fn in (lambda: s.sens_bounds(lam=True), lambda: s.sens_adjoint(seeds), lambda: s.sens_obst(seed_w=seeds),
               lambda: s.sens_weights(p, lam=True)):
        with pytest.raises(pkg.MpcError) as e:
            fn()
        assert e.value.code == MPC_ERR_STATE
    # ... and the next _sens solve brings it back, with the host form's bits
    s.solve(lf["x0"], lf["p"], lam_p=True)
    assert full() == 0
    assert np.array_equal(dw, lf["o"].dw) and np.array_equal(gb, lf["o"].grad_bv) and np.array_equal(lb, lf["o"].lam_bv)
    s.sens_adjoint(seeds), s.sens_obst(seed_w=seeds), s.sens_weights(p, lam=True)


@pytest.mark.gpu
def test_get_bounds_returns_what_is_installed(lf):
    cfg = lf["cfg"]
    lbg, ubg, lbx, ubx = BicycleNLP(cfg).bounds()
    # a handle that was given nothing holds the reference defaults
    s = make_solver(cfg)
    for got, want in zip(s.get_bounds(), (lbx, ubx, lbg, ubg)):
        assert np.array_equal(got, want)
    assert np.array_equal(s.bounds_vector(), bref.bounds_vector(cfg))
    # other bounds, then all-None again; any argument of the C entry may be NULL
    bv = bref.bounds_vector(cfg)
    bv[2 * cfg.n_w + bref.OL] = 0.9
    bv[0] = -0.3
    bv[cfg.n_w + 1] = np.inf
    s.set_bounds(*s.unpack_bounds(bv))
    assert np.array_equal(s.bounds_vector(), bv)
    r_lbg, r_ubg, r_lbx, r_ubx = bref.unpack_bounds(cfg, bv)
    for got, want in zip(s.unpack_bounds(bv), (r_lbx, r_ubx, r_lbg, r_ubg)):
        assert np.array_equal(got, want)
    only = np.empty(cfg.n_g)
    assert s._lib.mpc_get_bounds(s._h, None, None, only.ctypes.data_as(C.POINTER(C.c_double)), None) == 0
    assert only[0] == 0.0 and only[-1] == 0.9
    s.set_bounds()
    assert np.array_equal(s.bounds_vector(), bref.bounds_vector(cfg))


def torch_case(ag, cfg, x0, p, seed, levels):
    """bv.grad of loss = sum(x c) over the converged rows along the given level directions against central differences of the loss over
    re-solves with set_bounds; returns the layer's x and bv.grad"""
    import torch
    dev = torch.device("cuda")
    s = solver_for(cfg)
    bv0, d_all = s.bounds_vector(), bref.level_directions(cfg)
    c = np.random.default_rng(seed).normal(size=x0.shape)
    tx0, tp, tc = (torch.from_numpy(a).to(dev) for a in (x0, p, c))
    bv = torch.tensor(bv0, dtype=torch.float64, requires_grad=True)                    # a host tensor
    x, st = ag.mpc_solve(s, tx0, tp, failed="zero", bounds=bv)
    conv = st.cpu().numpy() == 1
    assert conv.sum() >= (len(conv) + 1) // 2
    (torch.nan_to_num(x) * tc)[torch.from_numpy(conv).to(dev)].sum().backward()
    got = bv.grad.numpy().copy()
    assert np.array_equal(s.bounds_vector(), bv0) and np.all(got[~np.isfinite(bv0)] == 0.0)

    def loss_at(b):
        s.set_bounds(*s.unpack_bounds(b))
        r = s.solve(x0, p)
        assert np.array_equal(r.status == 1, conv)
        return float((r.x * c)[conv].sum())

    h = 1e-4
    for q in levels:
        fd = (loss_at(bv0 + h * d_all[q]) - loss_at(bv0 - h * d_all[q])) / (2 * h)
        ad = got @ d_all[q]
        print(f"\n  {bref.LEVELS[q]}: bv.grad along the level {ad:.9g}, central differences {fd:.9g}, |difference| / max(1, |fd|) {abs(ad - fd) / max(1.0, abs(fd)):.2e}")
        assert abs(ad - fd) <= 1e-3 * max(1.0, abs(fd)), (bref.LEVELS[q], ad, fd)
    s.set_bounds(*s.unpack_bounds(bv0))
    return s, x, got, c, conv


@pytest.mark.gpu
def test_torch_layer_gradients(lf, ca):
    import torch
    ag = importlib.import_module(pkg.__name__ + ".autograd")
    dev = torch.device("cuda")
    levels = (D_OL, D_FU, D_DELTAV_MIN)
    # -- lane following, every row; collision avoidance, rows 0-5
    cfg, B, x0, p = lf["cfg"], lf["B"], lf["x0"], lf["p"]
    s, x, got, c, conv = torch_case(ag, cfg, x0, p, 77, levels)
    assert np.all(conv) and abs(got @ bref.level_directions(cfg)[D_DELTAV_MIN]) > 1e-3   # (the loss does depend on the steering-rate limit)
    _, _, got_ca, _, _ = torch_case(ag, ca["cfg"], ca["x0"][:6], ca["p"][:6], 78, levels)
    d_ca = bref.level_directions(ca["cfg"])
    assert min(abs(got_ca @ d_ca[q]) for q in levels) > 1e-3
    # ... it is sens_bounds(seed_w = dloss/dx) summed over the rows; a device tensor gives the same, on its device
    tx0, tp, tc = (torch.from_numpy(a).to(dev) for a in (x0, p, c))
    s.solve(x0, p, lam_p=True)
    rows = s.sens_bounds(seed_w=c).grad_bv
    assert np.allclose(got, rows.sum(axis=0), rtol=1e-12, atol=1e-12 * np.max(np.abs(rows)))
    bvd = torch.tensor(s.bounds_vector(), dtype=torch.float64, device=dev, requires_grad=True)
    xd, _ = ag.mpc_solve(s, tx0, tp, failed="zero", bounds=bvd)
    (xd * tc).sum().backward()
    assert bvd.grad.is_cuda and np.array_equal(bvd.grad.cpu().numpy(), got)
    # bounds=None: the bits of the layer without the argument, and the solver's bounds are not touched
    before = s.bounds_vector()
    tp3 = torch.from_numpy(p).to(dev).requires_grad_(True)
    x3, st3 = ag.mpc_solve(s, tx0, tp3, bounds=None)
    (tc * x3).sum().backward()
    tp4 = torch.from_numpy(p).to(dev).requires_grad_(True)
    x4, st4 = ag.MPCSolve.apply(s, tx0, tp4)
    (tc * x4).sum().backward()
    assert torch.equal(x3, x4) and torch.equal(st3, st4) and torch.equal(tp3.grad, tp4.grad)
    assert np.array_equal(x3.detach().cpu().numpy(), lf["r"].x) and np.array_equal(s.bounds_vector(), before)
    s.solve(x0, p, lam_p=True)
    assert np.array_equal(tp3.grad.cpu().numpy(), s.sens_adjoint(c), equal_nan=True)
    # backward after set_bounds with other bounds raises
    bv5 = torch.tensor(before, dtype=torch.float64, requires_grad=True)
    x5, _ = ag.mpc_solve(s, tx0, tp, bounds=bv5)
    moved = before.copy()
    moved[2 * cfg.n_w + bref.OL] = 1.0
    s.set_bounds(*s.unpack_bounds(moved))
    with pytest.raises(Exception):
        x5.sum().backward()
    # failed="nan" with one row forced to fail: the whole sum is NaN; "zero": the sum over the other rows
    s.set_bounds(*s.unpack_bounds(before))
    p_bad = p.copy()
    p_bad[3, 2 * cfg.N + cfg.nx + 1] = np.nan
    tpb = torch.from_numpy(p_bad).to(dev)
    for failed in ("zero", "nan"):
        bv6 = torch.tensor(before, dtype=torch.float64, requires_grad=True)
        x6, st6 = ag.mpc_solve(s, tx0, tpb, failed=failed, bounds=bv6)
        stn = st6.cpu().numpy()
        assert stn[3] != 1 and np.all(np.delete(stn, 3) == 1)
        (tc * torch.nan_to_num(x6)).sum().backward()
        if failed == "nan":
            assert np.all(np.isnan(bv6.grad.numpy()))
            continue
        s.solve(x0, p_bad, lam_p=True)
        rows = s.sens_bounds(seed_w=c).grad_bv
        assert np.all(np.isnan(rows[3])) and np.all(np.isfinite(bv6.grad.numpy()))
        assert np.allclose(bv6.grad.numpy(), np.delete(rows, 3, axis=0).sum(axis=0), rtol=1e-12, atol=1e-12 * np.nanmax(np.abs(rows)))
