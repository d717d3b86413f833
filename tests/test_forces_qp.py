"""Row f3: the FORCES-mode SQP step (one stage-structured QP per call).
CPU: the numpy oracle (dense KKT) against scipy on the same QP; the kernels' stage-wise (Riccati) solver, stepped by the
emulation harness, against the oracle.  GPU: mpc_forces_solve_batch against the oracle, and the ForcesproOptimizer call
surface end to end."""
import ctypes as C

import numpy as np
import pytest

import forces_families as FF
from helpers import WEIGHTS_YAML_ZAM_LF, abi, emu_lib, make_configuration, pkg, straight_path
from oracle import forces_model_numpy as FM
from oracle import forces_qp_numpy as Q

N = 10
LB = np.array([-0.4, -11.5, -np.inf, -np.inf, -1.066, 0.0, -np.inf])           # optimizer.py:100-110
UB = np.array([0.4, 11.5, np.inf, np.inf, 1.066, 50.8, np.inf])
HL = np.concatenate(([0.0], np.full(9, 3.3 ** 2)))
HU = np.concatenate(([11.5 ** 2], np.full(9, np.inf)))
OBST = [59.948, 0.08323, 60.945, 0.16074, 58.951, 0.00572]                      # ZAM_Over-1_1 obstacle circles


def family(B, seed=0, obstacle_every=2):
    rng = np.random.default_rng(seed)
    zbar, params, xinit = np.zeros((B, N, 7)), np.zeros((B, N, 10)), np.zeros((B, 5))
    for b in range(B):
        zi = np.array([0.0, 0.0, 29.9948, -1.1501, 0.0, 20.0, 0.03495])
        zi[3] += rng.uniform(-0.5, 0.5)
        zi[5] *= rng.uniform(0.8, 0.98)
        zbar[b] = np.tile(zi, (N, 1))
        xinit[b] = zi[2:]
        k = np.arange(1, N + 1)
        path = np.stack([zi[2] + k * 2 * np.cos(0.03495), -1.1501 + k * 2 * np.sin(0.03495)], 1)
        ob = OBST if (obstacle_every and b % obstacle_every) else [-100.0, 0, -100, 0, -100, 0]
        params[b] = np.hstack([path, np.full((N, 1), 20.0), np.full((N, 1), 0.03495), np.tile(ob, (N, 1))])
    return zbar, params, xinit


def _big(a):
    return np.where(np.isfinite(a), a, np.sign(a) * 1e308)


def emu_forces(zbar, params, xinit, w=FM.WEIGHTS_MODEL_C, mode=0, lb=LB, ub=UB):
    B, N = zbar.shape[:2]
    zbar, params, xinit = (np.ascontiguousarray(a, dtype=np.float64) for a in (zbar, params, xinit))
    big = _big
    zo, it, st, kk = np.zeros_like(zbar), np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B)
    dp = abi.as_dp
    rc = emu_lib().emu_forces_solve(B, N, C.c_double(0.1), C.c_double(FM.WHEELBASE_ODE), C.c_double(2.578), C.c_double(0.75),
                                    dp(np.array(w["Q"], float)), dp(np.array(w["R"], float)), dp(np.array(w["P"], float)),
                                    dp(big(lb)), dp(big(ub)), dp(big(HL)), dp(big(HU)), mode, dp(zbar), dp(params), dp(xinit), dp(zo),
                                    abi.as_ip(it), abi.as_ip(st), dp(kk))
    assert rc == 0
    return zo, it, st, kk


def test_oracle_qp_against_scipy():
    from scipy.optimize import minimize
    zbar, params, xinit = family(4, seed=1)
    for b in (0, 1):
        st = Q.build_qp(zbar[b], params[b], xinit[b], LB, UB, HL, HU)
        Hd = Q.hessian_diag(FM.WEIGHTS_MODEL_C, N)
        hv = Hd.ravel()
        dz, it, conv, kkt = Q.solve_qp(st, zbar[b], xinit[b], Hd)
        assert conv and it < 20
        g = np.concatenate([s["g"] for s in st])
        cons = [dict(type="eq", fun=lambda x, b=b: x.reshape(N, 7)[0, 2:] - (xinit[b] - zbar[b, 0, 2:]))]
        for k in range(N - 1):
            cons.append(dict(type="eq", fun=lambda x, k=k, b=b: x.reshape(N, 7)[k + 1, 2:] - (st[k]["C"] @ x.reshape(N, 7)[k] + st[k]["c"] - zbar[b, k + 1, 2:])))
        for k in range(N):
            cons.append(dict(type="ineq", fun=lambda x, k=k: st[k]["d"] - st[k]["G"] @ x.reshape(N, 7)[k]))
        r = minimize(lambda x: g @ x + 0.5 * (hv * x) @ x, dz.ravel() * 0.0, jac=lambda x: g + hv * x, constraints=cons,
                     method="SLSQP", options=dict(ftol=1e-10, maxiter=300))
        assert r.status in (0, 9)                                                # 9: iteration limit, still a feasible descent sequence
        f_ipm = g @ dz.ravel() + 0.5 * (hv * dz.ravel()) @ dz.ravel()
        assert abs(f_ipm - r.fun) < 1e-5 * max(1.0, abs(r.fun))                  # same optimal value (strictly convex: same point)
        assert np.abs(r.x.reshape(N, 7) - dz).max() < 5e-3


@pytest.mark.parametrize("mode", [0, 1])
def test_stagewise_solver_matches_dense_oracle(mode):
    zbar, params, xinit = family(24, seed=2)
    zo, it, st, kk = emu_forces(zbar, params, xinit, mode=mode)
    n_ok = 0
    for b in range(zbar.shape[0]):
        zp, ito, conv, kkt = Q.sqp_step(zbar[b], params[b], xinit[b], LB, UB, HL, HU, mode=mode)
        assert (st[b] == 1) == conv
        if conv:
            n_ok += 1
            assert it[b] == ito
            assert np.abs(zp - zo[b]).max() < 1e-7
            assert np.allclose(zo[b, 0, 2:], xinit[b], rtol=0, atol=1e-4)       # initial condition (to the residual tolerance)
            assert zo[b, :, 0].min() > -0.4 - 1e-6 and zo[b, :, 1].max() < 11.5 + 1e-6
    assert n_ok >= 20
    # inconsistent linearised constraints (the obstacle constraint linearised 15 m away caps the travel below what the
    # brakes allow) are reported, not hidden
    zb, pr, xi = family(2, seed=3)
    pr[:, :, 4:] = OBST
    xi[:, 3] = 21.5                                                              # 30 m before the obstacle at 21.5 m/s:
    zb[:, :, 5] = 21.5                                                           # linearised there, it allows 14.8 m of travel
    _, _, st2, _ = emu_forces(zb, pr, xi)
    assert np.all(st2 != 1)


def test_binding_family_binds_every_row_kind():
    """the conditions on FF.binding_family, from the dense oracle alone (N = 10, B = 64, the committed seed): with the model's bounds the
    oracle converges on at least 56 instances and at least one ends otherwise; among the converged ones every row kind binds in at least
    three -- the steering-angle bounds under the tight pair FF.LB_TIGHT / FF.UB_TIGHT, all others under FF.LB / FF.UB"""
    zbar, params, xinit = FF.binding_family(64, 10)
    count = {}
    for name, lb, ub in (("model", FF.LB, FF.UB), ("tight", FF.LB_TIGHT, FF.UB_TIGHT)):
        n_conv, cnt = 0, dict.fromkeys(FF.BINDING_LABELS, 0)
        for b in range(64):
            labels, conv = FF.active_rows(zbar[b], params[b], xinit[b], lb, ub, FF.HL, FF.HU, with_conv=True)
            n_conv += conv
            for lab in labels if conv else ():
                cnt[lab] = cnt.get(lab, 0) + 1
        count[name] = cnt
        print(name, "converged", n_conv, cnt)
        if name == "model":
            assert 56 <= n_conv < 64
    for lab in FF.BINDING_LABELS:
        assert count["tight" if lab in ("lb4", "ub4") else "model"][lab] >= 3, lab
    # the friction row binds where the steering angle and the speed are free (stages past the first), and its aLong column is not zero there
    lab5 = FF.active_rows(zbar[5], params[5], xinit[5], FF.LB, FF.UB, FF.HL, FF.HU)
    assert "hu0" in lab5 and zbar[5, 1, 1] != 0.0


# instances checked against the dense oracle per horizon: all 16 up to N = 30, 8 at N = 50, kinds 1 and 5 beyond (the oracle takes
# ~0.1 s per instance at N = 30, ~2 s at N = 96 and ~8 s at N = 192)
def _oracle_instances(N):
    return range(16) if N <= 30 else range(8) if N <= 50 else (1, 5)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("N", [1, 2, 3, 4, 10, 30, 50, 96, 97, 192])
def test_stagewise_solver_matches_dense_oracle_at_every_horizon(N, mode):
    """emu_forces (the kernel's phase functions, stage after stage) against the dense-KKT oracle on FF.binding_family, at the horizons at
    which k_forces_qp changes its thread mapping.  With the tight bound pair too up to N = 30 (the steering-angle rows).
    Worst |z - z_oracle| over the converged instances, both modes and bound pairs (the bound is the project's 1e-7):
      N = 1: 2.2e-16, 2: 1.4e-13, 3: 4.2e-14, 4: 7.1e-15, 10: 3.0e-12, 30: 2.5e-11, 50: 3.7e-12, 96: 2.1e-12, 97: 1.4e-13, 192: 1.0e-11
    The friction-row kind is what long horizons are sensitive to under the literal 2.5 I Hessian: with a speed-up demand of 6 .. 12 m/s
    instead of FF.K5_DV the same instance is 1.1e-7 from the oracle at N = 192, and the oracle 5.6e-8 from itself with its KKT solves
    refined in extended precision -- round-off of both routes amplified alike, so K5_DV keeps the reference's own error far below the bound."""
    zbar, params, xinit = FF.binding_family(16, N)
    idx = list(_oracle_instances(N))
    worst, n_conv = 0.0, 0
    for lb, ub in ((FF.LB, FF.UB), (FF.LB_TIGHT, FF.UB_TIGHT))[:2 if N <= 30 else 1]:
        zo, it, st, kk = emu_forces(zbar, params, xinit, mode=mode, lb=lb, ub=ub)
        for b in idx:
            zp, ito, conv, kkt = Q.sqp_step(zbar[b], params[b], xinit[b], lb, ub, HL, HU, mode=mode)
            assert (st[b] == 1) == conv, (b, st[b], conv)
            if conv:
                n_conv += 1
                assert it[b] == ito, (b, it[b], ito)
                worst = max(worst, np.abs(zp - zo[b]).max())
    print(f"N={N} mode={mode}: {n_conv} converged, worst |z - z_oracle| = {worst:.2e}")
    assert n_conv >= len(idx) // 2 and worst < 1e-7


@pytest.mark.gpu
def test_gpu_forces_solve_matches_oracle():
    w = FM.WEIGHTS_MODEL_C
    s = pkg.BatchedMPCSolver(N, 5, Q=w["Q"], R=w["R"], P=w["P"])
    zbar, params, xinit = family(200, seed=4)
    for mode in (0, 1):
        x, flag, it, res = s.forces_solve(zbar, xinit, params, LB, UB, HL, HU, hessian_mode=mode)
        assert (flag == 1).mean() > 0.9
        for b in range(0, 200, 9):
            zp, ito, conv, kkt = Q.sqp_step(zbar[b], params[b], xinit[b], LB, UB, HL, HU, mode=mode)
            assert (flag[b] == 1) == conv
            if conv:
                assert it[b] == ito and np.abs(zp - x[b]).max() < 1e-7
    # the CPU emulation of the same code gives the same answers
    xe, ite, ste, _ = emu_forces(zbar[:16], params[:16], xinit[:16])
    x, flag, it, res = s.forces_solve(zbar[:16], xinit[:16], params[:16], LB, UB, HL, HU)
    assert np.array_equal(flag, ste) and np.array_equal(it, ite) and np.abs(x - xe).max() < 1e-8


# ---- k_forces_qp in every regime of its thread mapping.  mpc_forces_solve_batch_dev chooses IB, the instances per workgroup, from N (thread t:
# stage t / IB of instance t % IB); the batch sizes are a single instance, one short of a block, one past a block, several blocks with a ragged tail
HORIZON_BATCHES = {1: (1, 63, 65, 130), 2: (1, 63, 65, 130), 3: (1, 63, 65, 130), 4: (1, 33, 81), 10: (1, 17, 41),
                   30: (1, 5, 11), 50: (1, 5, 11), 96: (1, 5, 11), 97: (1, 5, 11), 192: (1, 5, 11)}
# |x_gpu - x_emu| of every instance: the bound test_gpu_forces_solve_matches_oracle uses at N = 10 (measured: DESIGN section 11)
GPU_EMU_BOUND = dict.fromkeys(HORIZON_BATCHES, 1e-8)
# N = 192: instance 4 (60 m/s asked for at the speed bound) ends -7 under the 2.5 I Hessian, in the kernel, the emulation and the dense oracle alike
# (18 iterations each); its diverging iterate is 8.94e-7 from the emulation's on the MI355X, the emulation's 2.03e-5 from the oracle's and the kernel's
# 2.11e-5 -- as close to the oracle as the emulation is (within 4 x), so the distance is FMA contraction and device libm on an iterate without a limit,
# and the bound of this horizon is 4 x the measured distance.  Every converged instance at N = 192 is within 1.0e-11.
GPU_EMU_BOUND[192] = 4 * 8.94e-7


def _instances_per_block(N):
    """IB as mpc_forces_solve_batch_dev computes it (workgroups of at most 192 threads, whole wavefronts)"""
    IB = 1
    while (IB * 2 * N + 63) // 64 * 64 <= 192 and IB < 64:
        IB *= 2
    return IB


def test_instances_per_block_table():
    """the N -> IB -> threads table of DESIGN section 11"""
    rows = {N: (_instances_per_block(N), (_instances_per_block(N) * N + 63) // 64 * 64) for N in HORIZON_BATCHES}
    assert rows == {1: (64, 64), 2: (64, 128), 3: (64, 192), 4: (32, 128), 10: (16, 192), 30: (4, 128), 50: (2, 128), 96: (2, 192),
                    97: (1, 128), 192: (1, 192)}


def _forces_solver(N, nx=5):
    w = FM.WEIGHTS_MODEL_C
    return pkg.BatchedMPCSolver(N, nx, Q=w["Q"], R=w["R"], P=w["P"])


@pytest.mark.gpu
@pytest.mark.parametrize("N", list(HORIZON_BATCHES))
def test_gpu_forces_kernel_in_every_horizon_regime(N):
    """mpc_forces_solve_batch on FF.binding_family at the horizon N, both Hessian modes:
    every instance of every batch size against the emulation harness (flag, iterations, x to GPU_EMU_BOUND; up to N = 30 the largest
    batch with the tight bound pair too, as on the CPU -- beyond, the obstacle instance of that pair takes 34 iterations and the emulation
    itself is 2.1e-7 from the dense oracle at N = 96, past the project's bound: no case to hold the kernel to); at N <= 10 every instance
    of the largest batch against the dense oracle; the result of an instance does not depend on where it sits (the batch permuted, the
    first instance of each kind alone: bit for bit); a NaN in one instance's guess stays in that instance; the optional outputs may be null."""
    s = _forces_solver(N)
    Bs = HORIZON_BATCHES[N]
    Bmax = Bs[-1]
    zbar, params, xinit = FF.binding_family(Bmax, N)
    worst, worst_conv, clean = 0.0, 0.0, {}
    for mode in (0, 1):
        for B in Bs:
            for lb, ub in ((LB, UB), (FF.LB_TIGHT, FF.UB_TIGHT))[:2 if B == Bmax and N <= 30 else 1]:
                x, flag, it, res = s.forces_solve(zbar[:B], xinit[:B], params[:B], lb, ub, HL, HU, hessian_mode=mode)
                xe, ite, ste, _ = emu_forces(zbar[:B], params[:B], xinit[:B], mode=mode, lb=lb, ub=ub)
                d = np.abs(x - xe).reshape(B, -1).max(1)
                print(f"N={N} B={B} mode={mode} tight={lb is not LB}: flags {dict(zip(*np.unique(flag, return_counts=True)))}, "
                      f"|x - x_emu| {d.max():.2e} (converged {d[ste == 1].max() if (ste == 1).any() else 0.0:.2e})")
                assert np.array_equal(flag, ste) and np.array_equal(it, ite)
                worst, worst_conv = max(worst, d.max()), max(worst_conv, d[ste == 1].max() if (ste == 1).any() else 0.0)
                assert d.max() < GPU_EMU_BOUND[N] and (not (ste == 1).any() or d[ste == 1].max() < 1e-8)
                if lb is LB and B == Bmax:
                    clean[mode] = (x, flag, it, res)
        # an independent route on the device: the dense oracle
        if N <= 10:
            x, flag, it, res = clean[mode]
            for b in range(Bmax):
                zp, ito, conv, kkt = Q.sqp_step(zbar[b], params[b], xinit[b], LB, UB, HL, HU, mode=mode)
                assert (flag[b] == 1) == conv
                if conv:
                    assert it[b] == ito and np.abs(zp - x[b]).max() < 1e-7
        # placement: permuted, and alone
        perm = np.random.default_rng(11).permutation(Bmax)
        moved = s.forces_solve(zbar[perm], xinit[perm], params[perm], LB, UB, HL, HU, hessian_mode=mode)
        for a, m in zip(clean[mode], moved):
            assert np.array_equal(a[perm], m)
        for b in range(min(FF.N_KINDS, Bmax)):
            alone = s.forces_solve(zbar[b:b + 1], xinit[b:b + 1], params[b:b + 1], LB, UB, HL, HU, hessian_mode=mode)
            for a, m in zip(clean[mode], alone):
                assert np.array_equal(a[b:b + 1], m)
        # containment: NaN in the guess of one instance in the middle of a block
        IB = _instances_per_block(N)
        bad = IB + IB // 2 if IB + IB // 2 < Bmax else Bmax // 2
        zn = zbar.copy()
        zn[bad, N // 2, 3] = np.nan
        hurt = s.forces_solve(zn, xinit, params, LB, UB, HL, HU, hessian_mode=mode)
        assert hurt[1][bad] == -6
        keep = np.arange(Bmax) != bad
        for a, m in zip(clean[mode], hurt):
            assert np.array_equal(a[keep], m[keep])
    print(f"N={N}: worst |x - x_emu| = {worst:.2e} (converged instances {worst_conv:.2e})")
    # the optional outputs through the raw ABI
    out = np.empty_like(zbar)
    dp = abi.as_dp
    rc = s._lib.mpc_forces_solve_batch(s._h, Bmax, dp(zbar), dp(xinit), dp(params), dp(_big(LB)), dp(_big(UB)), dp(_big(HL)), dp(_big(HU)), 1,
                                       dp(out), None, None, None)
    assert rc == 0 and np.array_equal(out, clean[1][0])


@pytest.mark.gpu
def test_gpu_forces_solve_refuses_what_it_cannot_run():
    """refused with MPC_ERR_INVALID and a message, nothing launched: a horizon above 192 stages, six states.  (A handle of such a horizon
    exists -- the FORCES-mode solve goes to 192, the NLP entry points to 127 -- and every entry point refuses what it cannot run.)"""
    zbar, params, xinit = FF.binding_family(2, 193)
    s = _forces_solver(193)
    with pytest.raises(pkg.MpcError) as e:
        s.forces_solve(zbar, xinit, params, LB, UB, HL, HU)
    assert e.value.code == abi.MPC_ERR_INVALID and "horizons above 192 stages are not supported" in str(e.value)
    for call in (lambda: s.solve(np.zeros((2, s.n_w)), np.zeros((2, s.n_w))), lambda: s.eval_nlp(np.zeros((2, s.n_w)), np.zeros((2, s.n_w)))):
        with pytest.raises(pkg.MpcError) as e:
            call()
        assert e.value.code == abi.MPC_ERR_INVALID and "horizons up to 127" in str(e.value)
    zbar, params, xinit = FF.binding_family(2, 10)
    with pytest.raises(pkg.MpcError) as e:
        _forces_solver(10, nx=6).forces_solve(zbar, xinit, params, LB, UB, HL, HU)
    assert e.value.code == abi.MPC_ERR_INVALID and "the FORCES formulation has 5 states" in str(e.value)
    with pytest.raises(pkg.MpcError) as e:
        _forces_solver(1025)
    assert e.value.code == abi.MPC_ERR_INVALID


@pytest.mark.gpu
def test_gpu_forcespro_optimizer_closed_loop():
    """the reference's FORCES caller path (mpc_planner.py:301-309 with framework_name: forcespro) end to end on the GPU"""
    opt = __import__("importlib").import_module("motion-planning-for-autonomous-driving-with-mpc_amd.optimizer")
    path, orient = straight_path(30, 29.9948, -1.1501, 0.03495, 20.0)
    conf = make_configuration(path, orient, 20.0, WEIGHTS_YAML_ZAM_LF)
    o = opt.ForcesproOptimizer(configuration=conf, init_values=(np.array([29.9948, -1.1501]), 20.0, 0.0, 0.03495), predict_horizon=10)
    states, controls, t = o.optimize()
    assert states.shape == (30, 5) and controls.shape == (30, 2) and t.shape == (30,)
    lateral = (states[:, 1] + 1.1501) * np.cos(0.03495) - (states[:, 0] - 29.9948) * np.sin(0.03495)
    assert np.abs(lateral).max() < 0.3 and states[-1, 3] < 19.0
    # consecutive rows are one RK4 step of the plant (optimizer.py:356), as in the recorded forcespro runs
    from oracle.binding import OracleSolver
    from oracle.nlp_numpy import NLPConfig
    orc = OracleSolver(NLPConfig(N=10, nx=5))
    for k in range(29):
        assert np.abs(orc.plant_step(states[k], controls[k], "rk4") - states[k + 1]).max() < 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [None, 5])
def test_gpu_forces_closed_loop_on_the_device_matches_the_host_loop(seed):
    """mpc_forces_closed_loop_batch (the whole loop of optimizer.py:246-366 enqueued on the device: parameters, SQP step, applied
    input with the seeded applied-input noise, RK4 plant step) against ForcesproOptimizer.optimize's step-by-step host loop over
    mpc_forces_solve_batch / mpc_plant_step; then 512 egos with perturbed starts in one call"""
    opt = __import__("importlib").import_module("motion-planning-for-autonomous-driving-with-mpc_amd.optimizer")
    path, orient = straight_path(30, 29.9948, -1.1501, 0.03495, 20.0)
    outs = []
    for device_loop in (True, False):
        conf = make_configuration(path, orient, 20.0, WEIGHTS_YAML_ZAM_LF, noised=seed is not None)
        if seed is not None:
            conf.noise_seed = seed
        o = opt.ForcesproOptimizer(configuration=conf, init_values=(np.array([29.9948, -1.1501]), 20.0, 0.0, 0.03495), predict_horizon=10)
        o.use_device_loop = device_loop
        outs.append(o.optimize())
    assert np.abs(outs[0][0] - outs[1][0]).max() < 1e-9 and np.abs(outs[0][1] - outs[1][1]).max() < 1e-9
    if seed is not None:
        nz = __import__("importlib").import_module("motion-planning-for-autonomous-driving-with-mpc_amd.noise")
        conf = make_configuration(path, orient, 20.0, WEIGHTS_YAML_ZAM_LF)
        clean = opt.ForcesproOptimizer(configuration=conf, init_values=(np.array([29.9948, -1.1501]), 20.0, 0.0, 0.03495), predict_horizon=10).optimize()
        assert np.abs(outs[0][1][0] - clean[1][0] - nz.applied_noise(seed, 0, 0, 0.1)).max() < 1e-12
    # a batch: one call, 512 egos
    model, solver = o.solver()
    be = solver._backend
    B = 512
    rng = np.random.default_rng(1)
    init = np.tile([29.9948, -1.1501, 0.0, 20.0, 0.03495], (B, 1))
    init[:, 1] += rng.uniform(-0.3, 0.3, B)
    init[:, 3] *= rng.uniform(0.95, 1.0, B)
    traj, ctrl, flag = be.forces_closed_loop(init, np.tile(path, (B, 1, 1)), np.tile(orient, (B, 1)), np.full(B, 20.0), 30, model.lb, model.ub, model.hl, model.hu)
    assert np.all(flag == 1) and np.array_equal(traj[:, 0], init)
    lateral = (traj[:, -1, 1] + 1.1501) * np.cos(0.03495) - (traj[:, -1, 0] - 29.9948) * np.sin(0.03495)
    assert np.abs(lateral).max() < 0.3


@pytest.mark.gpu
@pytest.mark.parametrize("horizon", [4, 30])
def test_gpu_forces_closed_loop_on_the_device_matches_the_host_loop_at_other_horizons(horizon):
    """the device loop against the host loop where k_forces_qp maps its threads otherwise than at predict_horizon = 10 (32 and 4 instances
    per workgroup): 30 steps, no noise"""
    opt = __import__("importlib").import_module("motion-planning-for-autonomous-driving-with-mpc_amd.optimizer")
    path, orient = straight_path(30, 29.9948, -1.1501, 0.03495, 20.0)
    outs = []
    for device_loop in (True, False):
        conf = make_configuration(path, orient, 20.0, WEIGHTS_YAML_ZAM_LF)
        o = opt.ForcesproOptimizer(configuration=conf, init_values=(np.array([29.9948, -1.1501]), 20.0, 0.0, 0.03495), predict_horizon=horizon)
        o.use_device_loop = device_loop
        outs.append(o.optimize())
    assert outs[0][0].shape == (30, 5) and outs[0][1].shape == (30, 2)
    assert np.abs(outs[0][0] - outs[1][0]).max() < 1e-9 and np.abs(outs[0][1] - outs[1][1]).max() < 1e-9


@pytest.mark.gpu
def test_gpu_forcespro_collision_avoidance_device_loop_sees_the_obstacle():
    """use_case = collision_avoidance on the FORCES path: the obstacle circle centres are run-time parameters 4..9 of every stage
    (optimizer.py:319-323).  The device loop takes them from the handle, the host loop from runtime_parameters(): both must plan
    around the same obstacle (round 2 created the handle without it: the device loop drove straight through)."""
    opt = __import__("importlib").import_module("motion-planning-for-autonomous-driving-with-mpc_amd.optimizer")
    # (slow ego, obstacle 12 m ahead and 3 m to the right: the reference linearises the squared distances at a guess it never refreshes, optimizer.py:264-274,
    #  i.e. at the START state -- a half-plane about half-way to the obstacle; at 20 m/s the QP of a later step would be infeasible)
    v0, psi = 2.0, 0.03495
    path, orient = straight_path(30, 29.9948, -1.1501, psi, v0)
    obstacle = dict(position_x=29.9948 + 12.0 * np.cos(psi) + 3.0 * np.sin(psi), position_y=-1.1501 + 12.0 * np.sin(psi) - 3.0 * np.cos(psi),
                    length=4.0, width=1.8, orientation=psi)
    outs = []
    for device_loop in (True, False):
        conf = make_configuration(path, orient, v0, WEIGHTS_YAML_ZAM_LF, obstacle=obstacle, use_case="collision_avoidance")
        o = opt.ForcesproOptimizer(configuration=conf, init_values=(np.array([29.9948, -1.1501]), v0, 0.0, psi), predict_horizon=10)
        o.use_device_loop = device_loop
        outs.append(o.optimize())
    assert np.abs(outs[0][0] - outs[1][0]).max() < 1e-9 and np.abs(outs[0][1] - outs[1][1]).max() < 1e-9
    conf = make_configuration(path, orient, v0, WEIGHTS_YAML_ZAM_LF)
    free = opt.ForcesproOptimizer(configuration=conf, init_values=(np.array([29.9948, -1.1501]), v0, 0.0, psi), predict_horizon=10).optimize()
    assert np.abs(outs[0][0] - free[0]).max() > 1e-2                     # the obstacle changes the plan
    # clearance of the three ego circles from the three obstacle circles along the device loop's plan (squared distances, optimizer.py:146-155)
    oc = np.array(o.obstacle_circles_centers_tuple).reshape(3, 2)
    x = outs[0][0]
    ego = np.stack([x[:, :2], x[:, :2] + 0.75 * np.stack([np.cos(x[:, 4]), np.sin(x[:, 4])], 1), x[:, :2] - 0.75 * np.stack([np.cos(x[:, 4]), np.sin(x[:, 4])], 1)], 1)
    dist = np.linalg.norm(ego[:, :, None, :] - oc[None, None, :, :], axis=-1)
    assert dist.min() > (o.radius_ego + o.radius_obstacle) - 0.05
