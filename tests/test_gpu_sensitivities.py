"""GPU: parametric sensitivities of the optimum -- lam_p, forward dw = (dw*/dp) dp, the adjoint and the torch layer
(mpc_solve_batch_sens[_dev], mpc_sens_adjoint[_dev], autograd.py).

dw is checked against the active-set derivative of the numpy NLP (tests/sens_ref.py) at the returned (x, lam_g, lam_x) on every converged
row of a sample that is strictly complementary to the solve's tolerance (sens_ref.active_sets: no row or bound within WEAK_GAP of its
bound with a multiplier below STRICT); the excluded count is printed."""
import ctypes as C
import importlib

import numpy as np
import pytest

import sens_ref
from helpers import CA_CFG, FAMILIES, ca_batch, cfg_from_golden, make_solver, pkg, set_cfg_bounds, synthetic_batch

GOLD = np.load(__import__("os").path.join(__import__("os").path.dirname(__file__), "golden", "nlp_optima.npz"))
TOL_DW = 1e-5
MPC_ERR_INVALID, MPC_ERR_STATE = -1, -4


def solver_for(cfg, **opts):
    s = make_solver(cfg)
    set_cfg_bounds(s, cfg)
    for k, v in opts.items():
        s.set_option(k, str(v))
    return s


def seeds(cfg, B, n_rand=2, seed=0):
    rng = np.random.default_rng(seed)
    dp = np.zeros((B, n_rand + cfg.nx, cfg.n_w))
    dp[:, :n_rand] = rng.normal(size=(B, n_rand, cfg.n_w))
    for i in range(cfg.nx):
        dp[:, n_rand + i, 2 * cfg.N + i] = 1.0
    return dp


def check_dw(cfg, res, p, dp, rows, tol=TOL_DW):
    """NaN exactly on the rows that did not converge or sit on the friction kink -- every other row of the batch finite (a snapshot row that
    was not found or not written, or a failed pivot, shows as NaN) --, then dw of the sampled rows against numpy; returns the rows compared"""
    assert np.all(np.isnan(res.dw[res.status != 1])) and np.all(np.isnan(res.lam_p[res.status != 1]))
    kink = np.isnan(res.lam_g[:, 0]) & (res.status == 1)
    assert np.all(np.isnan(res.dw[kink]))
    good = (res.status == 1) & ~kink
    bad = np.flatnonzero(good & ~np.all(np.isfinite(res.dw.reshape(res.dw.shape[0], -1)), axis=1))
    assert bad.size == 0, f"converged rows with non-finite dw: {bad[:16]} ({bad.size})"
    assert np.all(np.isfinite(res.lam_p[res.status == 1]))
    compared, weak = [], 0
    worst = 0.0
    for b in rows:
        if not good[b]:
            continue
        S, w_ = sens_ref.sensitivity_matrix(cfg, res.x[b], p[b], res.lam_g[b], res.lam_x[b])
        if w_:
            weak += 1
            continue
        ref = np.einsum("ij,dj->di", S, dp[b])
        err = np.max(np.abs(res.dw[b] - ref)) / max(1.0, np.max(np.abs(ref)))
        assert np.isfinite(err) and err <= tol, (b, err)
        worst = max(worst, err)
        compared.append(int(b))
    print(f"\n  dw vs numpy: {len(compared)} rows checked, {weak} weakly active rows excluded, worst relative error {worst:.2e}")
    assert len(compared) >= max(1, len(rows) // 3), (len(compared), weak)
    return compared


def compare_ex(a, b):
    for fld in ("x", "status", "iters", "kkt", "f", "g", "lam_g", "lam_x"):
        assert np.array_equal(getattr(a, fld), getattr(b, fld), equal_nan=True), fld


# ---- 3 + 4: bit-identical to _ex on every path; dw against numpy --------------------------------------------------------------------------
CASES = {
    "headline": (FAMILIES["zamlf_n30_nx6"][0], 4096, {}, {}),
    "wg_alone": (CA_CFG, 1024, dict(hybrid_live=64), None),
    "ca_second_chance": (CA_CFG, 3072, dict(rescue_wg=0), None),
    "chunked": (FAMILIES["zamlf_n10_nx5"][0], 16448, {}, {}),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_sens_matches_ex_and_reference(name):
    cfg, B, opts, kw = CASES[name]
    x0, p = ca_batch(cfg, B) if kw is None else synthetic_batch(cfg, B, **kw)
    s = solver_for(cfg, **opts)
    ex = s.solve(x0, p, multipliers=True)
    dp = seeds(cfg, B)
    r = s.solve(x0, p, multipliers=True, lam_p=True, dp=dp)
    compare_ex(ex, r)
    if name == "ca_second_chance":
        assert s.last_rescued() > 0
    rows = np.random.default_rng(7).choice(B, 16, replace=False)
    rescued = np.zeros(0, int)
    if name == "ca_second_chance":       # and rows that took the second chance (converged now, not without it)
        plain = solver_for(cfg, rescue=0).solve(x0, p)
        rescued = np.flatnonzero((plain.status != 1) & (r.status == 1))
        assert rescued.size > 0
        rows = np.concatenate([rows, rescued[:12]])
    if name == "chunked":                # both chunks: chunk 1 = rows 0 .. 16383, chunk 2 = the last 64 rows (the snapshot's offset per chunk)
        assert B > 16384
        rows = np.concatenate([rows, np.arange(0, 8), np.arange(16384, B, 8), [B - 1]])
    compared = check_dw(cfg, r, p, dp, rows, 1e-5 if cfg is not CA_CFG else 1e-4)
    if name == "ca_second_chance":
        assert len(set(compared) & set(rescued.tolist())) >= 1, "no rescued row was compared"
    if name == "chunked":
        assert len([b for b in compared if b >= 16384]) >= 4 and len([b for b in compared if b < 8]) >= 3


@pytest.mark.gpu
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_families_dw_and_finite_differences(fam):
    cfg, kw = FAMILIES[fam]
    B = 256
    x0, p = synthetic_batch(cfg, B, **kw)
    s = solver_for(cfg)
    dp = seeds(cfg, B, seed=1)
    r = s.solve(x0, p, lam_p=True, dp=dp, multipliers=True)
    assert np.mean(r.status == 1) > 0.99
    check_dw(cfg, r, p, dp, np.arange(0, B, 16))
    # 5: the whole stack against the solver itself, directional differences of GPU solves
    # (rows with a weakly active row or bound are left out: a step of h can cross the kink of the active set there)
    h = 1e-4
    rows = [b for b in np.flatnonzero(r.status == 1)[:12] if not sens_ref.kkt_matrix(cfg, r.x[b], p[b], r.lam_g[b], r.lam_x[b])[2]][:4]
    rows = np.asarray(rows)
    for d in (0, 2 + 2, 2 + 3):
        a = s.solve(x0[rows], p[rows] + h * dp[rows, d])
        b = s.solve(x0[rows], p[rows] - h * dp[rows, d])
        ok = (a.status == 1) & (b.status == 1)
        fd = (a.x - b.x) / (2 * h)
        err = np.max(np.abs(fd[ok] - r.dw[rows][ok, d]), axis=1) / np.maximum(1.0, np.max(np.abs(fd[ok]), axis=1))
        assert ok.sum() >= 3 and np.all(err <= 1e-3), (d, err)


@pytest.mark.gpu
def test_first_step_presolved_friction_bound():
    cfg = cfg_from_golden(GOLD["first_n30_nx5__cfg"])
    x0, p = GOLD["first_n30_nx5__x0"], GOLD["first_n30_nx5__p"]
    s = solver_for(cfg)
    dp = seeds(cfg, x0.shape[0])
    r = s.solve(x0, p, lam_p=True, dp=dp, multipliers=True)
    assert np.all(r.status == 1) and np.all(r.lam_g[:, 0] > 0)
    check_dw(cfg, r, p, dp, np.arange(x0.shape[0]))
    assert np.all(np.abs(r.dw[:, 2 + 2, 1]) > 1e-3)          # a_0 follows delta_0 along the friction cap


# ---- 6: adjoint consistency, errors ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_adjoint_consistency_on_a_stream_and_state_errors():
    import torch
    cfg = FAMILIES["zamlf_n30_nx6"][0]
    B, nd = 512, 3
    x0, p = synthetic_batch(cfg, B)
    s = solver_for(cfg)
    dev = torch.device("cuda")
    dp = np.ascontiguousarray(seeds(cfg, B, n_rand=nd, seed=3)[:, :nd])
    seed_w = np.random.default_rng(4).normal(size=(B, cfg.n_w))
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in dict(x0=x0, p=p, dp=dp, seed=seed_w).items()}
    tx, tst = torch.empty_like(t["x0"]), torch.empty(B, dtype=torch.int32, device=dev)
    tdw, tlp, tgp = torch.empty((B, nd, cfg.n_w), dtype=torch.float64, device=dev), torch.empty_like(t["p"]), torch.empty_like(t["p"])
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        s.solve_device(B, t["x0"].data_ptr(), t["p"].data_ptr(), tx.data_ptr(), tst.data_ptr(), stream=stream.cuda_stream, d_lam_p=tlp.data_ptr(),
                       n_dir=nd, d_dp=t["dp"].data_ptr(), d_dw=tdw.data_ptr())
        s.sens_adjoint_device(B, t["seed"].data_ptr(), tgp.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    dw, gp, st = tdw.cpu().numpy(), tgp.cpu().numpy(), tst.cpu().numpy()
    assert np.all(st == 1)
    lhs = np.einsum("bj,bdj->bd", seed_w, dw)
    rhs = np.einsum("bj,bdj->bd", gp, dp)
    assert np.max(np.abs(lhs - rhs) / np.maximum(1.0, np.abs(lhs))) <= 1e-10
    assert np.all(gp[:, : 2 * cfg.N] == 0.0)
    # the host adjoint agrees with the device one
    assert np.allclose(s.sens_adjoint(seed_w), gp, rtol=0, atol=1e-12 * max(1.0, np.max(np.abs(gp))))
    # wrong B, then an intervening plain solve: the snapshot is gone
    L = s._lib
    dptr = lambda a_: a_.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    g2 = np.empty((B - 1, cfg.n_w))
    assert L.mpc_sens_adjoint(s._h, B - 1, dptr(np.ascontiguousarray(seed_w[:-1])), dptr(g2)) == MPC_ERR_STATE
    s.solve(x0[:8], p[:8])
    assert L.mpc_sens_adjoint(s._h, B, dptr(seed_w), dptr(np.empty_like(seed_w))) == MPC_ERR_STATE
    # fixed_iters > 0: invalid
    f = make_solver(cfg, fixed_iters=20)
    set_cfg_bounds(f, cfg)
    with pytest.raises(pkg.MpcError) as e:
        f.solve(x0[:8], p[:8], lam_p=True)
    assert e.value.code == MPC_ERR_INVALID


# ---- 7: lam_p ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_lam_p_and_casadi_keys():
    cfg = CA_CFG
    x0, p = ca_batch(cfg, 64)
    s = solver_for(cfg)
    r = s.solve(x0, p, multipliers=True, lam_p=True)
    for b in np.flatnonzero(r.status == 1)[:6]:
        num = sens_ref.lam_p_numeric(cfg, r.x[b], p[b], r.lam_g[b], r.lam_x[b])
        assert np.max(np.abs(r.lam_p[b] - num)) <= 1e-6 * max(1.0, np.max(np.abs(num)))
        assert np.array_equal(r.lam_p[b], sens_ref.lam_p(cfg, r.x[b], p[b], r.lam_g[b]))
    opt = importlib.import_module(pkg.__name__ + ".optimizer")
    h = opt.NlpSolverHandle(s)
    one = h(x0=x0[0].reshape(-1, 1), p=p[0].reshape(-1, 1))
    assert one["lam_p"].full().shape == (cfg.n_w, 1)
    batch = h(x0=x0, p=p)
    assert batch["lam_p"].full().shape == (64, cfg.n_w)
    assert np.array_equal(batch["lam_p"].full(), r.lam_p, equal_nan=True)
    assert np.array_equal(batch["x"].full(), r.x)


# ---- 8: the torch layer --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_torch_layer_gradients():
    import torch
    ag = importlib.import_module(pkg.__name__ + ".autograd")
    cfg = FAMILIES["zamlf_n30_nx5"][0]
    B = 64
    x0, p = synthetic_batch(cfg, B)
    s = solver_for(cfg)
    dev = torch.device("cuda")
    tx0 = torch.from_numpy(x0).to(dev)
    tp = torch.from_numpy(p).to(dev).requires_grad_(True)
    wts = torch.from_numpy(np.random.default_rng(9).normal(size=(B, cfg.n_w))).to(dev)
    x, st = ag.mpc_solve(s, tx0, tp)
    loss = (wts * x).sum() + (x[:, 2 * cfg.N:] ** 2).sum()
    loss.backward()
    g = tp.grad.cpu().numpy()
    assert np.all(st.cpu().numpy() == 1)
    # the adjoint of the same seed through the C-ABI
    seed = (wts + torch.cat([torch.zeros_like(x[:, : 2 * cfg.N]), 2 * x[:, 2 * cfg.N:]], 1)).detach().cpu().numpy()
    s.solve(x0, p, lam_p=True)
    assert np.allclose(g, s.sens_adjoint(seed), rtol=1e-12, atol=1e-12)
    # finite differences of the loss along a random direction
    # (along a direction that moves only strictly complementary rows: a weakly active one can change its active set within h)
    d = np.random.default_rng(10).normal(size=p.shape)
    d[:, : 2 * cfg.N] = 0.0
    m = s.solve(x0, p, multipliers=True)
    for b in range(B):
        if sens_ref.kkt_matrix(cfg, m.x[b], p[b], m.lam_g[b], m.lam_x[b])[2]:
            d[b] = 0.0
    assert np.count_nonzero(d.any(axis=1)) >= B // 2
    h = 1e-4

    def L(pp):
        xx = s.solve(x0, pp).x
        return float(np.sum(wts.cpu().numpy() * xx) + np.sum(xx[:, 2 * cfg.N:] ** 2))
    fd = (L(p + h * d) - L(p - h * d)) / (2 * h)
    assert abs(fd - np.sum(g * d)) <= 1e-3 * max(1.0, abs(fd))
    # backward after an invalidating solve raises
    tp2 = torch.from_numpy(p).to(dev).requires_grad_(True)
    x2, _ = ag.mpc_solve(s, tx0, tp2)
    s.solve(x0[:4], p[:4])
    with pytest.raises(Exception):
        x2.sum().backward()
    tp3 = torch.from_numpy(p).to(dev).requires_grad_(True)
    x3, _ = ag.mpc_solve(s, tx0, tp3)
    ag.mpc_solve(s, tx0, torch.from_numpy(p).to(dev))
    with pytest.raises(RuntimeError):
        x3.sum().backward()
    # failed="zero" masks rows that did not converge (none here: the same gradient)
    tp4 = torch.from_numpy(p).to(dev).requires_grad_(True)
    x4, _ = ag.mpc_solve(s, tx0, tp4, failed="zero")
    ((wts * x4).sum() + (x4[:, 2 * cfg.N:] ** 2).sum()).backward()
    assert np.allclose(tp4.grad.cpu().numpy(), g, rtol=1e-12, atol=1e-12)


@pytest.mark.gpu
def test_feedback_gain_matches_xref0_seeds():
    cfg = FAMILIES["zamlf_n30_nx6"][0]
    x0, p = synthetic_batch(cfg, 32)
    s = solver_for(cfg)
    K = s.feedback_gain(x0, p)
    assert K.shape == (32, 2, cfg.nx)
    r = s.solve(x0, p, dp=seeds(cfg, 32, n_rand=0))
    assert np.array_equal(K, r.dw[:, :, 0:2].transpose(0, 2, 1))
