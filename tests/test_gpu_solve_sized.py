"""GPU: the NLP solve with a lower bound per circle row (mpc_solve_batch_sized).

Identity: with every entry of rsum the handle's circle lower bound, the solve is mpc_solve_batch_stages on the same handle, bit for bit, on every
path a per-stage solve takes.  Distinct radii: chunks, placement, the poison aid.  Against the reference of tests/sized_ref.py (the oracle's
dense interior-point method on the oracle's NLP with the rows' own bounds): optima, KKT certificates with the instance's bounds, f and g.
Refusals."""
import numpy as np
import pytest

import pred_obst_ref as ref
import sized_ref as sref
from helpers import CA_CFG, abi, ca_batch, kkt_certificate, make_solver, pkg, set_cfg_bounds
from oracle.nlp_numpy import BicycleNLP, synthetic_batch
from test_gpu_solve_stages import FIELDS, assert_same_bits, drift_batch, rows_beside, solver_for

pytestmark = pytest.mark.gpu


def identity(s, cfg, x0, p, st, what):
    """solve(obst [B, N+1, 6]) and the same with rsum [B, N+1, 3] = the handle's radius sum everywhere, on handle s: the same bits in every output"""
    B = x0.shape[0]
    a = s.solve(x0, p, st, multipliers=True)
    b = s.solve(x0, p, st, multipliers=True, rsum=np.full((B, cfg.N + 1, 3), cfg.r_sum))
    assert_same_bits(a, b, what)
    return a, b


def stages_of(row, N):
    return np.ascontiguousarray(np.repeat(row[:, None, :], N + 1, axis=1))


@pytest.mark.parametrize("N,nx,B", [(1, 5, 1), (1, 5, 65), (2, 6, 1), (2, 5, 65), (3, 6, 65), (10, 5, 130), (31, 5, 70), (32, 5, 70), (63, 5, 66), (64, 5, 66)])
def test_equal_radii_give_the_bits_of_the_per_stage_solve(N, nx, B):
    """the shapes of tests/test_gpu_solve_stages.py: short horizons, several blocks, N = 31 / 32 where the instances per workgroup change, N = 63
    / 64: the last horizon of the 256-thread kernels and the first on the 512-thread one-launch-per-kernel path"""
    cfg = ref.cfg_for(N, nx)
    x0, p = synthetic_batch(cfg, B, v_range=(6.0, 12.0))
    s = solver_for(cfg)
    a, _ = identity(s, cfg, x0, p, stages_of(rows_beside(cfg, x0, p, N), N), (N, nx, B))
    print(N, nx, B, "converged", int((a.status == 1).sum()), "of", B)
    assert B == 1 or (a.status == 1).sum() >= B // 2


def test_identity_through_the_pipeline_through_k_solve_wg_and_the_restart():
    """N = 30, nx = 6, B = 1088: with hybrid = 0 the persistent pipeline serves the batch to the end, at default options k_solve_wg does; the
    restart after an abandoned persistent launch (the test hook abandons every launch) starts over with one launch per kernel"""
    cfg = ref.cfg_for(30, 6)
    x0, p = synthetic_batch(cfg, 1088, v_range=(6.0, 12.0))
    st = stages_of(rows_beside(cfg, x0, p, 5), 30)
    s = solver_for(cfg, hybrid="0")
    a, _ = identity(s, cfg, x0, p, st, "pipeline")
    out = np.zeros(8)
    assert s._lib.mpc_get_pipeline_profile(s._h, abi.as_dp(out)) == 0 and out[1] == 1
    s2 = solver_for(cfg)
    b, _ = identity(s2, cfg, x0, p, st, "k_solve_wg")
    assert s2.get_resident_profile()["ran"] and not s2.get_pipeline_profile()["ran"]
    assert (a.status == 1).sum() >= 1000 and (b.status == 1).sum() >= 1000
    s3 = solver_for(cfg, hybrid="0", pipe_test_abort="1")
    identity(s3, cfg, x0[:200], p[:200], st[:200], "restart")
    assert s3.get_option("pipe_aborts") >= 1


def test_identity_through_the_second_chance():
    """collision-avoidance cold starts: the levels behind the launch (rescue_dev, whose gather copies the packed rows -- centres and radii) and
    the second chance inside k_solve_wg (every level scales the rows' offsets by its fraction; here they are zero)"""
    x0, p = ca_batch(CA_CFG, 256)
    st = stages_of(np.tile(np.asarray(CA_CFG.obstacle_centers).ravel(), (256, 1)), CA_CFG.N)
    for mode in ("0", "2"):
        s = solver_for(CA_CFG, rescue_wg=mode)
        a = s.solve(x0, p, st, multipliers=True)
        n_a = s.last_rescued()
        b = s.solve(x0, p, st, multipliers=True, rsum=np.full((256, CA_CFG.N + 1, 3), CA_CFG.r_sum))
        print("rescue_wg", mode, "rescued", n_a, s.last_rescued(), "status != 1:", int((a.status != 1).sum()))
        assert n_a > 0 and s.last_rescued() == n_a
        assert_same_bits(a, b, mode)


def test_second_chance_scales_distinct_radii_alike_behind_and_inside_the_launch():
    """collision-avoidance cold starts with the front and rear rows' radius 0.2 m over the handle's (offsets of 0, 0.2, 0.2 m, so the scale of a level
    matters: at fraction 0 every row's bound is 0, not 0.2; on the CPU emulation instances 25, 35 and 154 stall from their cold start under
    these radii): the levels behind the launch (rescue_dev hands the fraction to the transposer) and the levels
    inside k_solve_wg (the workgroup writes the scale row of its instance) give the same bits -- which of the two paths gave an instance its
    second chance does not show (csrc/mpc_solve_plan.h) --, and the last level is the problem itself: every rescued row passes the certificate
    with its own bounds"""
    x0, p = ca_batch(CA_CFG, 256)
    st = stages_of(np.tile(np.asarray(CA_CFG.obstacle_centers).ravel(), (256, 1)), CA_CFG.N)
    rad = np.full((256, CA_CFG.N + 1, 3), CA_CFG.r_sum)
    rad[:, :, 1:] += 0.2
    runs = {}
    for mode in ("0", "2"):
        s = solver_for(CA_CFG, rescue_wg=mode)
        runs[mode] = s.solve(x0, p, st, multipliers=True, rsum=rad)
        runs[mode + "n"] = s.last_rescued()
        print("rescue_wg", mode, "rescued", runs[mode + "n"], "status != 1:", int((runs[mode].status != 1).sum()))
    assert runs["0n"] > 0 and runs["0n"] == runs["2n"]
    assert_same_bits(runs["0"], runs["2"], "behind / inside")
    r = runs["0"]
    for b in np.flatnonzero(r.status == 1)[::16]:
        nlp = sref.SizedNLP(CA_CFG, st[b], rad[b])
        c = kkt_certificate(nlp, r.x[b], p[b], bounds=nlp.bounds())
        assert c["stationarity"] <= 1e-6 and c["feasibility"] <= 1e-6, (b, c)


def test_distinct_radii_chunks_placement_poison():
    """the drift family, N = 10, B = 300, every row with a radius of its own: chunks of 128 give the bits of the unchunked solve; the batch permuted
    gives the same rows; the poison aid (NaN into the workspace before the solve) changes nothing -- the rows go in behind it"""
    cfg = ref.cfg_for(10)
    x0, p, st = drift_batch(10, 300)
    st = st.reshape(300, 11, 6)
    rad = np.ascontiguousarray(np.array([sref.radii("drift", 10, seed) for seed in range(300)]))
    s = solver_for(cfg)
    a = s.solve(x0, p, st, multipliers=True, rsum=rad)
    print("status 1 on", int((a.status == 1).sum()), "of 300")
    assert not np.any(a.status == -6) and not s.get_pipeline_profile()["ran"]
    assert not np.array_equal(a.x, s.solve(x0, p, st).x)                        # (the radii were read: test_against_the_reference says by how much)
    s.set_option("max_batch", "128")
    assert_same_bits(a, s.solve(x0, p, st, multipliers=True, rsum=rad), "chunks")
    s.set_option("max_batch", None)
    perm = np.random.default_rng(0).permutation(300)
    b = s.solve(x0[perm], p[perm], np.ascontiguousarray(st[perm]), multipliers=True, rsum=np.ascontiguousarray(rad[perm]))
    for f in FIELDS:
        assert np.array_equal(getattr(b, f), getattr(a, f)[perm], equal_nan=True), f
    s.set_option("poison", "1")
    c = s.solve(x0, p, st, multipliers=True, rsum=rad)
    assert_same_bits(a, c, "poison")


@pytest.mark.parametrize("N", [2, 3, 4, 7, 10])
def test_against_the_reference(N):
    """one batch per N, the families interleaved.  Status 1 wherever the reference converged; |x - x_ref| <= 1e-4, the bound DESIGN.md section 2
    gives for two interior-point methods on one NLP; every row a KKT point of ITS NLP by the certificate of tests/helpers.py at 1e-6 / 1e-6 with
    the instance's own bounds; f, g of the solve are eval_nlp's bits (the literal distances); the optimum is more than 1e-3 from the per-stage
    solve with the handle's radius, so the radii were read"""
    parts = tuple(q for q in sref.FAMILIES if q[1] == N)
    d = sref.batch(parts)
    cfg = ref.cfg_for(N)
    s = solver_for(cfg)
    x0, p, st, rad = d["x0"], d["p"], d["stages"], d["radii"]
    B = x0.shape[0]
    r = s.solve(x0, p, st, multipliers=True, rsum=rad)
    err = np.abs(r.x - d["x_ref"]).max(axis=1)
    print(f"N={N} {parts} B={B}: status 1 on {int((r.status == 1).sum())}, max |x - x_ref| = {err.max():.3e}, iterations max {r.iters.max()}")
    assert np.all(r.status == 1)
    assert err.max() <= 1e-4
    f2, g2 = s.eval_nlp(r.x, p, st)
    assert np.array_equal(f2, r.f) and np.array_equal(g2, r.g)
    worst = 0.0
    for b in range(B):
        nlp = sref.SizedNLP(cfg, st[b], rad[b])
        c = kkt_certificate(nlp, r.x[b], p[b], bounds=nlp.bounds())
        worst = max(worst, c["stationarity"])
        assert c["stationarity"] <= 1e-6 and c["feasibility"] <= 1e-6, (b, c)
    print(f"N={N}: worst relative stationarity residual {worst:.2e}")
    equal = s.solve(x0, p, st)
    diff = np.abs(r.x - equal.x).max(axis=1)
    print(f"N={N}: min over instances of |x - x_equal_radius| = {diff.min():.3e}")
    assert diff.min() > 1e-3


def test_refusals():
    """rsum / obst NULL (host and device form), a negative / NaN entry in the host form, a handle whose circle rows have a finite upper bound,
    mpc_sens_* after a sized solve (MPC_ERR_STATE); the device form gives the rows of the host form, and a NaN entry there ends its own
    instance with status -6 and touches no other"""
    import torch
    cfg = ref.cfg_for(10)
    d = sref.batch((("drift", 10),))
    x0, p, st, rad = d["x0"], d["p"], d["stages"], np.ascontiguousarray(d["radii"])
    B = x0.shape[0]
    s = solver_for(cfg)
    lib, dp, ip = s._lib, abi.as_dp, abi.as_ip
    out, status, iters, kkt = np.empty_like(x0), np.empty(B, np.int32), np.empty(B, np.int32), np.empty(B)
    tail = (dp(out), ip(status), ip(iters), dp(kkt), None, None, None, None)
    rc = lib.mpc_solve_batch_sized(s._h, B, dp(x0), dp(p), dp(st), None, *tail)
    assert rc == abi.MPC_ERR_INVALID and b"rsum" in lib.mpc_last_error(s._h)
    rc = lib.mpc_solve_batch_sized(s._h, B, dp(x0), dp(p), None, dp(rad), *tail)
    assert rc == abi.MPC_ERR_INVALID and b"obst" in lib.mpc_last_error(s._h)
    for bad in (-0.1, np.nan, np.inf):
        r2 = rad.copy()
        r2[B // 2, 3, 1] = bad
        rc = lib.mpc_solve_batch_sized(s._h, B, dp(x0), dp(p), dp(st), dp(r2), *tail)
        assert rc == abi.MPC_ERR_INVALID and b"rsum" in lib.mpc_last_error(s._h), bad
    with pytest.raises(pkg.MpcError):
        s.solve(x0, p, np.ascontiguousarray(st[:, 0]), rsum=rad)                 # (rsum without centres per stage)
    # a finite upper bound on the circle rows: a sized row has no meaning
    s_up = make_solver(cfg)
    lbg, ubg, lbx, ubx = BicycleNLP(cfg).bounds()
    ubg = ubg.copy()
    ubg[1 + cfg.nx * (cfg.N + 1):] = 50.0
    s_up.set_bounds(lbx, ubx, lbg, ubg)
    with pytest.raises(pkg.MpcError) as e:
        s_up.solve(x0, p, st, rsum=rad)
    assert e.value.code == abi.MPC_ERR_BOUNDS
    assert np.any(s_up.solve(x0, p, st).status == 1)                            # (the handle works)
    # a snapshot solve, then a sized solve: the snapshot's life has ended
    s.solve(x0, p, np.ascontiguousarray(st[:, 0]), lam_p=True)
    assert s.sens_obst(lam=True).lam_obst.shape == (B, 6)
    r = s.solve(x0, p, st, rsum=rad)
    assert np.all(r.status == 1)
    for call in (lambda: s.sens_obst(lam=True), lambda: s.sens_adjoint(np.zeros((B, cfg.n_w))), lambda: s.sens_weights(p, lam=True),
                 lambda: s.sens_bounds(lam=True)):
        with pytest.raises(pkg.MpcError) as e:
            call()
        assert e.value.code == abi.MPC_ERR_STATE
    for kw in (dict(lam_p=True), dict(dp=np.zeros((B, 1, cfg.n_w)))):
        with pytest.raises((pkg.MpcError, ValueError)):
            s.solve(x0, p, st, rsum=rad, **kw)
    # the device form gives the rows of the host form
    t = [torch.from_numpy(a).cuda() for a in (x0, p, st, rad)]
    o = torch.empty_like(t[0])
    d_status = torch.empty(B, dtype=torch.int32, device="cuda")
    with pytest.raises(pkg.MpcError) as e:
        s.solve_device(B, t[0].data_ptr(), t[1].data_ptr(), o.data_ptr(), d_obst=0, obst_stages=True, d_rsum=t[3].data_ptr())
    assert e.value.code == abi.MPC_ERR_INVALID
    s.solve_device(B, t[0].data_ptr(), t[1].data_ptr(), o.data_ptr(), d_status=d_status.data_ptr(), d_obst=t[2].data_ptr(), obst_stages=True,
                   d_rsum=t[3].data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(o.cpu().numpy(), r.x) and np.array_equal(d_status.cpu().numpy(), r.status)
    # ... and does not read the buffer back: a NaN entry ends that instance with status -6, every other row as it was
    r2 = rad.copy()
    r2[B // 2, 3, 1] = np.nan
    d_r2 = torch.from_numpy(r2).cuda()
    s.solve_device(B, t[0].data_ptr(), t[1].data_ptr(), o.data_ptr(), d_status=d_status.data_ptr(), d_obst=t[2].data_ptr(), obst_stages=True,
                   d_rsum=d_r2.data_ptr())
    torch.cuda.synchronize()
    st2, x2 = d_status.cpu().numpy(), o.cpu().numpy()
    keep = np.arange(B) != B // 2
    assert st2[B // 2] == -6 and np.array_equal(st2[keep], r.status[keep]) and np.array_equal(x2[keep], r.x[keep])
