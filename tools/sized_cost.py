"""Cost of a radius per circle row: ms per call of mpc_solve_batch_sized_dev with every radius the handle's against mpc_solve_batch_stages_dev -- same
handle, same inputs, device-pointer forms, alternating windows in one process, medians.  With equal radii the two return the same
bits (checked), so what differs is the kernels: the sized instantiations (three offsets held by every stage thread, two 16-byte loads more per stage and
round) and, in front of the solve, k_sized_pack + k_transpose_obst_sized in place of k_transpose_obst_stages.  N = 30, nx = 6, B = 4096: the headline
shape.  Then the loop through traffic of mixed sizes against the traffic loop, in the same way (below).  Usage: python tools/sized_cost.py [out.txt]"""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from oracle.nlp_numpy import BicycleNLP, synthetic_batch  # noqa: E402
import pred_obst_ref as ref  # noqa: E402

pkg = importlib.import_module("motion-planning-for-autonomous-driving-with-mpc_amd")
N, NX, B = 30, 6, 4096
CALLS, REPS = 10, 15
cfg = ref.cfg_for(N, NX)
x0, p = synthetic_batch(cfg, B, v_range=(6.0, 12.0))
# one obstacle 3.4 .. 6 m beside the reference at mid-horizon per instance, the same at every stage (some circle rows active)
rng = np.random.default_rng(5)
Xr = p[:, 2 * N:].reshape(B, N + 1, NX)
mid = Xr[:, (N + 1) // 2]
side = rng.choice([-1.0, 1.0], B) * rng.uniform(3.4, 6.0, B)
pose = np.stack([mid[:, 0] - side * np.sin(mid[:, 4]), mid[:, 1] + side * np.cos(mid[:, 4]), mid[:, 4] + rng.uniform(-0.1, 0.1, B)], axis=1)
st = np.ascontiguousarray(np.repeat(ref.centres(pose).reshape(B, 1, 6), N + 1, axis=1))
rsum = np.full((B, N + 1, 3), cfg.r_sum)

s = pkg.BatchedMPCSolver(cfg.N, cfg.nx, dt=cfg.dt, Q=cfg.Qdiag, R=cfg.R, obstacle_centers=cfg.obstacle_centers, ego_offset=cfg.ego_offset,
                         wheelbase=cfg.wheelbase, friction_div=cfg.friction_div)
lbg, ubg, lbx, ubx = BicycleNLP(cfg).bounds()
s.set_bounds(lbx, ubx, lbg, ubg)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()                        # noqa: E731
d_x0, d_p, d_st, d_rs = map(dev, (x0, p, st, rsum))
d_out = torch.empty_like(d_x0)
d_status = torch.empty(B, dtype=torch.int32, device="cuda")


def stages():
    s.solve_device(B, d_x0.data_ptr(), d_p.data_ptr(), d_out.data_ptr(), d_status=d_status.data_ptr(), d_obst=d_st.data_ptr(), obst_stages=True)


def sized():
    s.solve_device(B, d_x0.data_ptr(), d_p.data_ptr(), d_out.data_ptr(), d_status=d_status.data_ptr(), d_obst=d_st.data_ptr(), obst_stages=True,
                   d_rsum=d_rs.data_ptr())


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(CALLS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / CALLS * 1e3


for fn in (stages, sized, stages, sized):
    fn()
torch.cuda.synchronize()
stages()
torch.cuda.synchronize()
want = (d_out.cpu().numpy().copy(), d_status.cpu().numpy().copy())
sized()
torch.cuda.synchronize()
same = np.array_equal(want[0], d_out.cpu().numpy()) and np.array_equal(want[1], d_status.cpu().numpy())
res = {"stages": [], "sized": []}
for _ in range(REPS):
    for name, fn in (("stages", stages), ("sized", sized)):
        res[name].append(timed(fn))
lines = [f"B={B} N={N} nx={NX}; ms per solve (device-pointer forms, {CALLS} calls per window, {REPS} alternating windows); status 1 on "
         f"{int((want[1] == 1).sum())} of {B}; sized with equal radii bit-identical to stages: {same}"]
base = np.median(res["stages"])
for name, t in res.items():
    t = np.array(t)
    lines.append(f"  {name:8s} median {np.median(t):8.4f}  min {t.min():8.4f}  max {t.max():8.4f}  spread(max-min) {t.max() - t.min():7.4f}   ratio to stages {np.median(t) / base:.4f}")
s.close()

# ---- the loop: mpc_closed_loop_batch_traffic_sized_dev with every radius the handle's against mpc_closed_loop_batch_traffic_dev -- the scenes of
#      tools/loop_traffic_cost.py (B = 4096, L = 30, N = 10 / 30, M = 1 / 4 / 16 tracks per ego, obstacle 0 6 - 10 m beside the path, the others 60 - 200 m
#      off), bit-identical outputs (checked): what differs is k_loop_traffic_sized in place of k_loop_traffic and the sized solves
LB, LL, LCALLS, LREPS = 4096, 30, 5, 7
for LN in (10, 30):
    rng = np.random.default_rng(LN)
    v, psi, Lp, Lt = 15.0, 0.1, LL + LN, LL + LN
    k = np.arange(Lp)
    init = np.tile([0.0, 0.0, 0.0, v, psi], (LB, 1))
    init[:, 1] += rng.uniform(-0.5, 0.5, LB)
    init[:, 3] *= rng.uniform(0.9, 1.1, LB)
    path = np.tile(np.stack([k * v * 0.1 * np.cos(psi), k * v * 0.1 * np.sin(psi)], axis=1), (LB, 1, 1))
    orient, vdes = np.full((LB, Lp), psi), np.full(LB, v)
    M_MAX = 16
    side = rng.uniform(60.0, 200.0, (LB, M_MAX)) * rng.choice([-1.0, 1.0], (LB, M_MAX))
    side[:, 0] = rng.uniform(6.0, 10.0, LB) * rng.choice([-1.0, 1.0], LB)
    along = rng.uniform(0.0, 30.0, (LB, M_MAX, 1)) + rng.uniform(2.0, 12.0, (LB, M_MAX, 1)) * 0.1 * np.arange(Lt)
    tracks = np.stack([along * np.cos(psi) - side[..., None] * np.sin(psi), along * np.sin(psi) + side[..., None] * np.cos(psi),
                       np.broadcast_to(psi + rng.uniform(-0.2, 0.2, (LB, M_MAX, 1)), (LB, M_MAX, Lt))], axis=3)
    ls = pkg.BatchedMPCSolver(LN, 5)
    ls.set_bounds()
    r_handle = float(np.asarray(ls.get_bounds()[2])[-1])                                  # the circle lower bound the handle was given
    d_init, d_path, d_orient, d_vdes = map(dev, (init, path, orient, vdes))
    d_tracks = {M: dev(tracks[:, :M]) for M in (1, 4, 16)}
    d_off = {M: dev(np.ones((LB, M))) for M in (1, 4, 16)}
    d_rs = {M: dev(np.full((LB, M), r_handle)) for M in (1, 4, 16)}
    d_traj, d_ctrl = (torch.empty((LB, LL, c), dtype=torch.float64, device="cuda") for c in (5, 2))
    d_st, d_cl = torch.empty((LB, LL), dtype=torch.int32, device="cuda"), torch.empty((LB, LL), dtype=torch.float64, device="cuda")
    d_near, d_chosen = torch.empty((LB, LL), dtype=torch.int32, device="cuda"), torch.empty((LB, LL, LN + 1, 3), dtype=torch.int32, device="cuda")
    head = (LB, d_init.data_ptr(), d_path.data_ptr(), d_orient.data_ptr(), d_vdes.data_ptr(), LL, Lp)

    def loop(M, with_radii):
        ls.closed_loop_traffic_device(*head, M, Lt, 1, d_tracks[M].data_ptr(), d_off[M].data_ptr(), d_traj.data_ptr(), d_ctrl.data_ptr(), d_st.data_ptr(),
                                      d_clearance=d_cl.data_ptr(), d_nearest=d_near.data_ptr(), d_chosen=d_chosen.data_ptr(),
                                      d_rsums=d_rs[M].data_ptr() if with_radii else 0)

    def ltimed(M, with_radii):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(LCALLS):
            loop(M, with_radii)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / LCALLS * 1e3

    outs = (d_traj, d_ctrl, d_st, d_cl, d_near, d_chosen)
    for M in (1, 4, 16):
        loop(M, False)
        loop(M, True)
        torch.cuda.synchronize()
        loop(M, False)
        torch.cuda.synchronize()
        want = [a.cpu().numpy().copy() for a in outs]
        loop(M, True)
        torch.cuda.synchronize()
        same = all(np.array_equal(x, y.cpu().numpy()) for x, y in zip(want, outs))
        t0, t1 = [], []
        for _ in range(LREPS):
            t0.append(ltimed(M, False))
            t1.append(ltimed(M, True))
        t0, t1 = np.array(t0), np.array(t1)
        lines.append(f"loop B={LB} L={LL} N={LN} M={M}: ms per loop call ({LCALLS} calls per window, {LREPS} alternating windows); all status 1: {bool((want[2] == 1).all())}; "
                     f"bit-identical: {same}; traffic median {np.median(t0):8.3f} ({t0.min():.3f} .. {t0.max():.3f})  sized median {np.median(t1):8.3f} "
                     f"({t1.min():.3f} .. {t1.max():.3f})  ratio {np.median(t1) / np.median(t0):.4f}")
    ls.close()
print("\n".join(lines))
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
