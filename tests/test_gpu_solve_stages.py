"""GPU: the NLP solve with obstacle centres per stage (mpc_solve_batch_stages, mpc_eval_nlp_batch_stages).

Identity: with all N + 1 stage rows of an instance equal, the solve is the solve with obst [B, 6] on the same handle, bit for bit, on every
path a [B, 6] solve takes.  Distinct stages: chunks, placement, the poison aid.  Against the reference of tests/pred_obst_ref.py (the oracle's
dense interior-point method on the oracle's NLP subclassed to centres per stage): optima, KKT certificates, g.  Refusals."""
import numpy as np
import pytest

import pred_obst_ref as ref
from helpers import CA_CFG, abi, ca_batch, kkt_certificate, make_solver, pkg, set_cfg_bounds
from oracle.nlp_numpy import synthetic_batch

pytestmark = pytest.mark.gpu

FIELDS = ("x", "status", "iters", "kkt", "f", "g", "lam_g", "lam_x")


def solver_for(cfg, **opts):
    s = make_solver(cfg)
    set_cfg_bounds(s, cfg)
    for k, v in opts.items():
        s.set_option(k, v)
    return s


def rows_beside(cfg, x0, p, seed):
    """one obstacle row [B, 6] per instance: a 6 x 3.5 m rectangle 3.4 .. 6 m beside the reference at mid-horizon (some circle rows active)"""
    rng = np.random.default_rng(seed)
    B, N, nx = x0.shape[0], cfg.N, cfg.nx
    Xr = p[:, 2 * N:].reshape(B, N + 1, nx)
    mid = Xr[:, (N + 1) // 2]
    side = rng.choice([-1.0, 1.0], B) * rng.uniform(3.4, 6.0, B)
    pose = np.stack([mid[:, 0] - side * np.sin(mid[:, 4]), mid[:, 1] + side * np.cos(mid[:, 4]), mid[:, 4] + rng.uniform(-0.1, 0.1, B)], axis=1)
    return np.ascontiguousarray(ref.centres(pose).reshape(B, 6))


def assert_same_bits(a, b, what):
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True), (what, f)


def identity(s, cfg, x0, p, row, what):
    """solve(obst [B, 6]) and solve(obst [B, N+1, 6]) with every stage row the instance's, on handle s: the same bits in every output"""
    a = s.solve(x0, p, row, multipliers=True)
    b = s.solve(x0, p, np.repeat(row[:, None, :], cfg.N + 1, axis=1), multipliers=True)
    assert_same_bits(a, b, what)
    return a, b


@pytest.mark.parametrize("N,nx,B", [(1, 5, 1), (1, 5, 65), (2, 6, 1), (2, 5, 65), (3, 5, 1), (3, 6, 65), (10, 5, 130), (31, 5, 70), (32, 5, 70), (63, 5, 66),
                                    (64, 5, 66)])
def test_equal_stage_rows_give_the_bits_of_the_per_instance_solve(N, nx, B):
    """short horizons, several blocks, N = 31 / 32 where the instances per workgroup change, N = 63 / 64: the last horizon of the 256-thread
    kernels and the first on the 512-thread one-launch-per-kernel path"""
    cfg = ref.cfg_for(N, nx)
    x0, p = synthetic_batch(cfg, B, v_range=(6.0, 12.0))
    s = solver_for(cfg)
    a, _ = identity(s, cfg, x0, p, rows_beside(cfg, x0, p, N), (N, nx, B))
    print(N, nx, B, "converged", int((a.status == 1).sum()), "of", B)
    assert B == 1 or (a.status == 1).sum() >= B // 2             # (the identity holds for every row, whatever its status)


def test_identity_through_the_pipeline_and_through_k_solve_wg():
    """N = 30, nx = 6, B = 1088: with hybrid = 0 the persistent pipeline serves the batch to the end, at default options k_solve_wg does"""
    cfg = ref.cfg_for(30, 6)
    x0, p = synthetic_batch(cfg, 1088, v_range=(6.0, 12.0))
    row = rows_beside(cfg, x0, p, 5)
    s = solver_for(cfg, hybrid="0")
    a, _ = identity(s, cfg, x0, p, row, "pipeline")
    out = np.zeros(8)
    assert s._lib.mpc_get_pipeline_profile(s._h, abi.as_dp(out)) == 0 and out[1] == 1
    s2 = solver_for(cfg)
    b, _ = identity(s2, cfg, x0, p, row, "k_solve_wg")
    assert s2.get_resident_profile()["ran"] and not s2.get_pipeline_profile()["ran"]
    assert (a.status == 1).sum() >= 1000 and (b.status == 1).sum() >= 1000
    # the restart after an abandoned persistent launch (the test hook abandons every launch: the solve starts over with one launch per kernel)
    s3 = solver_for(cfg, hybrid="0", pipe_test_abort="1")
    identity(s3, cfg, x0[:200], p[:200], row[:200], "restart")
    assert s3.get_option("pipe_aborts") >= 1


def test_identity_through_the_second_chance():
    """collision-avoidance cold starts (instance 94 of the family stalls from its cold start): the levels behind the launch (rescue_dev, whose
    gather copies 6 (N + 1) doubles per instance) and the second chance inside k_solve_wg (the restart reads the stage's own rows)"""
    x0, p = ca_batch(CA_CFG, 256)
    row = np.tile(np.asarray(CA_CFG.obstacle_centers).ravel(), (256, 1))
    for mode in ("0", "2"):
        s = solver_for(CA_CFG, rescue_wg=mode)
        a = s.solve(x0, p, row, multipliers=True)
        n_a = s.last_rescued()
        b = s.solve(x0, p, np.repeat(row[:, None, :], CA_CFG.N + 1, axis=1), multipliers=True)
        print("rescue_wg", mode, "rescued", n_a, s.last_rescued(), "status != 1:", int((a.status != 1).sum()))
        assert n_a > 0 and s.last_rescued() == n_a
        assert_same_bits(a, b, mode)


def drift_batch(N, B):
    inst = [ref.instance("drift", N, seed) for seed in range(B)]
    return (np.ascontiguousarray(np.array([q[i] for q in inst])) for i in range(3))


def test_distinct_stages_chunks_placement_poison():
    """the drift family, N = 10, B = 300 (every stage's centres differ, circle rows active): chunks of 128 give the bits of the unchunked solve;
    the batch permuted gives the same rows (k_solve_wg serves it at default options: an instance's arithmetic does not depend on its
    company there); the poison aid (NaN into the workspace before the solve) changes nothing -- the stage rows go in behind it"""
    cfg = ref.cfg_for(10)
    x0, p, st = drift_batch(10, 300)
    st = st.reshape(300, 11, 6)
    s = solver_for(cfg)
    a = s.solve(x0, p, st, multipliers=True)
    assert np.all(a.status == 1) and not s.get_pipeline_profile()["ran"]
    frozen = s.solve(x0, p, np.ascontiguousarray(st[:, 0]), multipliers=True)
    assert np.abs(a.x - frozen.x).max(axis=1).min() > 1e-3                      # (the stages were read)
    s.set_option("max_batch", "128")
    assert_same_bits(a, s.solve(x0, p, st, multipliers=True), "chunks")
    s.set_option("max_batch", None)
    perm = np.random.default_rng(0).permutation(300)
    b = s.solve(x0[perm], p[perm], np.ascontiguousarray(st[perm]), multipliers=True)
    for f in FIELDS:
        assert np.array_equal(getattr(b, f), getattr(a, f)[perm], equal_nan=True), f
    s.set_option("poison", "1")
    c = s.solve(x0, p, st, multipliers=True)
    assert not np.any(c.status == -6)
    assert_same_bits(a, c, "poison")


REF_BATCHES = {7: [("lead", 7)], 10: [("lead", 10), ("drift", 10)], 30: [("drift", 30)], 1: [("beside", 1)], 2: [("beside", 2)], 3: [("beside", 3)],
               4: [("beside", 4)]}


@pytest.mark.parametrize("N", sorted(REF_BATCHES))
def test_against_the_reference(N):
    """one batch per N, the families interleaved.  Status 1 wherever the reference converged; |x - x_ref| <= 1e-4, the bound DESIGN.md section 2
    gives for two interior-point methods on one NLP (observed maxima: DESIGN.md section 7); every status-1 row a KKT point of ITS NLP by the
    certificate of tests/helpers.py at 1e-6 / 1e-6, the thresholds tests/test_gpu_parity.py holds collision-avoidance rows to (its 1e-7 is for
    families of its own: the REFERENCE's optima of drift N = 30 reach 2.2e-7 on this certificate, which forces exact complementarity on an
    interior-point solution -- tests/test_pred_obst_cpu.py holds the reference to the same 1e-6); g of the solve and of eval_nlp against StagedNLP.g to the
    tolerance of the existing eval test; on the lead family the optimum is more than 1e-3 away from the solve with the obstacle frozen at
    its stage-0 pose"""
    parts = REF_BATCHES[N]
    d = ref.batch(tuple(parts))
    cfg = ref.cfg_for(N)
    s = solver_for(cfg)
    x0, p, st = d["x0"], d["p"], d["stages"]
    B = x0.shape[0]
    r = s.solve(x0, p, st, multipliers=True)
    err = np.abs(r.x - d["x_ref"]).max(axis=1)
    print(f"N={N} {parts} B={B}: status 1 on {int((r.status == 1).sum())}, max |x - x_ref| = {err.max():.3e}, iterations max {r.iters.max()}")
    assert np.all(r.status == 1)
    assert err.max() <= 1e-4
    f2, g2 = s.eval_nlp(r.x, p, st)
    assert np.array_equal(f2, r.f) and np.array_equal(g2, r.g)
    worst = 0.0
    for b in range(B):
        nlp = ref.StagedNLP(cfg, st[b])
        c = kkt_certificate(nlp, r.x[b], p[b])
        worst = max(worst, c["stationarity"])
        assert c["stationarity"] <= 1e-6 and c["feasibility"] <= 1e-6, (b, c)
        fr, gr = nlp.f(r.x[b], p[b]), nlp.g(r.x[b], p[b])
        assert abs(r.f[b] - fr) <= 1e-12 * abs(fr)
        assert np.max(np.abs(r.g[b] - gr) / np.maximum(1.0, np.abs(gr))) <= 1e-12 * max(1.0, np.max(np.abs(r.x[b])))
    print(f"N={N}: worst relative stationarity residual {worst:.2e}")
    frozen = s.solve(x0, p, np.ascontiguousarray(st[:, 0]))
    for i, (name, _) in enumerate(parts):
        if name == "lead":
            diff = np.abs(r.x - frozen.x).max(axis=1)[d["fam"] == i]
            print(f"N={N}: lead family, min over instances of |x - x_frozen| = {diff.min():.3e}")
            assert diff.min() > 1e-3


def test_refusals():
    """obst NULL for the _stages entries (host and device form), sensitivities of a per-stage solve (Python: raised before the call; library:
    mpc_sens_* after a _stages solve finds no snapshot -- MPC_ERR_STATE), and the handle works afterwards"""
    import torch
    cfg = ref.cfg_for(10)
    d = ref.batch((("drift", 10),))
    x0, p, st = d["x0"], d["p"], d["stages"]
    B = x0.shape[0]
    s = solver_for(cfg)
    lib, dp, ip = s._lib, abi.as_dp, abi.as_ip
    out, status, iters, kkt = np.empty_like(x0), np.empty(B, np.int32), np.empty(B, np.int32), np.empty(B)
    rc = lib.mpc_solve_batch_stages(s._h, B, dp(x0), dp(p), None, dp(out), ip(status), ip(iters), dp(kkt), None, None, None, None)
    assert rc == abi.MPC_ERR_INVALID and b"obst" in lib.mpc_last_error(s._h)
    f, g = np.empty(B), np.empty((B, cfg.n_g))
    rc = lib.mpc_eval_nlp_batch_stages(s._h, B, dp(x0), dp(p), None, dp(f), dp(g))
    assert rc == abi.MPC_ERR_INVALID and b"obst" in lib.mpc_last_error(s._h)
    t = [torch.from_numpy(a).cuda() for a in (x0, p)]
    o = torch.empty_like(t[0])
    with pytest.raises(pkg.MpcError) as e:
        s.solve_device(B, t[0].data_ptr(), t[1].data_ptr(), o.data_ptr(), d_obst=0, obst_stages=True)
    assert e.value.code == abi.MPC_ERR_INVALID and "obst" in str(e.value)
    rc = lib.mpc_eval_nlp_batch_stages_dev(s._h, B, t[0].data_ptr(), t[1].data_ptr(), None, o.data_ptr(), None, None)
    assert rc == abi.MPC_ERR_INVALID
    # a snapshot solve, then a per-stage solve: the snapshot's life has ended
    row = np.ascontiguousarray(st[:, 0])
    s.solve(x0, p, row, lam_p=True)
    assert s.sens_obst(lam=True).lam_obst.shape == (B, 6)
    r = s.solve(x0, p, st)
    assert np.all(r.status == 1)
    for call in (lambda: s.sens_obst(lam=True), lambda: s.sens_adjoint(np.zeros((B, cfg.n_w))), lambda: s.sens_weights(p, lam=True),
                 lambda: s.sens_bounds(lam=True)):
        with pytest.raises(pkg.MpcError) as e:
            call()
        assert e.value.code == abi.MPC_ERR_STATE
    for kw in (dict(lam_p=True), dict(dp=np.zeros((B, 1, cfg.n_w)))):
        with pytest.raises((pkg.MpcError, ValueError)):
            s.solve(x0, p, st, **kw)
    # the device form gives the rows of the host form
    d_st = torch.from_numpy(st).cuda()
    d_status = torch.empty(B, dtype=torch.int32, device="cuda")
    s.solve_device(B, t[0].data_ptr(), t[1].data_ptr(), o.data_ptr(), d_status=d_status.data_ptr(), d_obst=d_st.data_ptr(), obst_stages=True)
    torch.cuda.synchronize()
    assert np.array_equal(o.cpu().numpy(), r.x) and np.array_equal(d_status.cpu().numpy(), r.status)
