"""Cost of the parametric sensitivities (mpc_solve_batch_sens_dev, mpc_sens_adjoint_dev) against the plain device solve and _ex, same handle,
same batch, alternating samples: plain | _ex (f, g, lam_g, lam_x) | _sens with lam_p only | _sens with n_dir = nx forward seeds | the
adjoint alone (on the snapshot of the last _sens call) | mpc_sens_obst_dev alone on the same snapshot: its adjoint with lam_obst, and six
forward directions (the unit directions of the obstacle centres) | mpc_sens_weights_dev alone on the same snapshot: its adjoint with
lam_wt, and seven forward directions (the unit directions of the weights) | mpc_sens_bounds_dev alone on the same snapshot: its adjoint with
lam_bv, and nine forward directions (the limits of the vehicle, the friction limit and the circle radius, each moved at every stage at once).
Usage (GPU box): python tools/sens_cost.py [B] [family] [reps] [libmpcgpu.so]     family: a key of helpers.FAMILIES, or `ca` (the collision-avoidance
configuration of the tests); a library path measures that build instead of the package's own (a parent build, for an A/B of alternating runs)"""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np
import torch
from helpers import CA_CFG, FAMILIES, ca_batch, make_solver, set_cfg_bounds
from oracle.nlp_numpy import synthetic_batch

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
fam = sys.argv[2] if len(sys.argv) > 2 else "zamlf_n30_nx6"
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 30
if fam == "ca":
    cfg = CA_CFG
    x0, p = ca_batch(cfg, B)
else:
    cfg, kw = FAMILIES[fam]
    x0, p = synthetic_batch(cfg, B, **kw)
s = make_solver(cfg, lib_path=sys.argv[4] if len(sys.argv) > 4 else None)
set_cfg_bounds(s, cfg)
dev = "cuda"
nx, nw = cfg.nx, s.n_w
tx0, tp = torch.from_numpy(x0).to(dev), torch.from_numpy(p).to(dev)
out = torch.empty_like(tx0)
st = torch.empty(B, dtype=torch.int32, device=dev); it = torch.empty_like(st); kk = torch.empty(B, dtype=torch.float64, device=dev)
f = torch.empty(B, dtype=torch.float64, device=dev)
g = torch.empty((B, s.n_g), dtype=torch.float64, device=dev); lg = torch.empty_like(g)
lx = torch.empty((B, nw), dtype=torch.float64, device=dev); lp = torch.empty_like(lx)
dp = torch.zeros((B, nx, nw), dtype=torch.float64, device=dev)
for i in range(nx):
    dp[:, i, 2 * cfg.N + i] = 1.0
dw = torch.empty_like(dp)
seed = torch.randn((B, nw), dtype=torch.float64, device=dev); gp = torch.empty_like(seed)
dob = torch.eye(6, dtype=torch.float64, device=dev).repeat(B, 1, 1).contiguous(); dwo = torch.empty((B, 6, nw), dtype=torch.float64, device=dev)
go = torch.empty((B, 6), dtype=torch.float64, device=dev); lo = torch.empty_like(go)
dwt = torch.eye(7, dtype=torch.float64, device=dev).repeat(B, 1, 1).contiguous(); dww = torch.empty((B, 7, nw), dtype=torch.float64, device=dev)
gw = torch.empty((B, 7), dtype=torch.float64, device=dev); lw = torch.empty_like(gw)
nb = s.n_b
dbv = torch.zeros((B, 9, nb), dtype=torch.float64, device=dev)
for k in range(cfg.N):
    dbv[:, 0, 2 * k] = 1.0; dbv[:, 1, nw + 2 * k] = 1.0; dbv[:, 2, nw + 2 * k + 1] = 1.0                    # deltav_min, deltav_max, a_ub
for k in range(cfg.N + 1):
    for q, (side, i) in enumerate(((0, 2), (nw, 2), (0, 3), (nw, 3))):                                       # delta_min, delta_max, v_min, v_max
        dbv[:, 3 + q, side + 2 * cfg.N + nx * k + i] = 1.0
dbv[:, 7, 2 * nw + 1] = 1.0; dbv[:, 8, 2 * nw + 2] = 1.0                                                     # fu, ol
dwb = torch.empty((B, 9, nw), dtype=torch.float64, device=dev)
gb = torch.empty((B, nb), dtype=torch.float64, device=dev); lb = torch.empty_like(gb)
ptrs = (tx0.data_ptr(), tp.data_ptr(), out.data_ptr(), st.data_ptr(), it.data_ptr(), kk.data_ptr())


def plain():
    s.solve_device(B, *ptrs)


def ex():
    s.solve_device(B, *ptrs, d_f=f.data_ptr(), d_g=g.data_ptr(), d_lam_g=lg.data_ptr(), d_lam_x=lx.data_ptr())


def sens_lam_p():
    s.solve_device(B, *ptrs, d_lam_p=lp.data_ptr())


def sens_fwd():
    s.solve_device(B, *ptrs, n_dir=nx, d_dp=dp.data_ptr(), d_dw=dw.data_ptr())


def adjoint():
    s.sens_adjoint_device(B, seed.data_ptr(), gp.data_ptr())


def obst_adjoint():
    s.sens_obst_device(B, d_seed_w=seed.data_ptr(), d_grad_obst=go.data_ptr(), d_lam_obst=lo.data_ptr())


def obst_fwd():
    s.sens_obst_device(B, 6, dob.data_ptr(), dwo.data_ptr())


def wt_adjoint():
    s.sens_weights_device(B, tp.data_ptr(), d_seed_w=seed.data_ptr(), d_grad_wt=gw.data_ptr(), d_lam_wt=lw.data_ptr())


def wt_fwd():
    s.sens_weights_device(B, tp.data_ptr(), 7, dwt.data_ptr(), dww.data_ptr())


def bv_adjoint():
    s.sens_bounds_device(B, d_seed_w=seed.data_ptr(), d_grad_bv=gb.data_ptr(), d_lam_bv=lb.data_ptr())


def bv_fwd():
    s.sens_bounds_device(B, 9, dbv.data_ptr(), dwb.data_ptr())


def sample(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


fns = dict(plain=plain, ex=ex, sens_lam_p=sens_lam_p, sens_fwd_nx=sens_fwd, adjoint=adjoint, obst_adjoint=obst_adjoint, obst_fwd_6=obst_fwd,
           wt_adjoint=wt_adjoint, wt_fwd_7=wt_fwd, bv_adjoint=bv_adjoint, bv_fwd_9=bv_fwd)
ON_SNAPSHOT = ("adjoint", "obst_adjoint", "obst_fwd_6", "wt_adjoint", "wt_fwd_7", "bv_adjoint", "bv_fwd_9")
for _ in range(3):
    for k, fn in fns.items():
        if k in ON_SNAPSHOT:
            sens_lam_p()
        fn()
t = {k: [] for k in fns}
for _ in range(reps):
    for k, fn in fns.items():
        if k in ON_SNAPSHOT:
            sens_lam_p()                         # (these need the snapshot of a _sens solve as the handle's last solve)
        t[k].append(sample(fn))
med = {k: float(np.median(v)) for k, v in t.items()}
print(f"B={B} {fam} ({reps} samples each, median / min ms):")
for k, v in t.items():
    print(f"  {k:12s} {med[k]:8.4f} / {min(v):8.4f}")
print(f"  cost over plain: _ex {1e3 * (med['ex'] - med['plain']):.1f} us, _sens lam_p {1e3 * (med['sens_lam_p'] - med['plain']):.1f} us, "
      f"_sens n_dir = {nx} {1e3 * (med['sens_fwd_nx'] - med['plain']):.1f} us, adjoint alone {1e3 * med['adjoint']:.1f} us, "
      f"obstacle adjoint + lam_obst alone {1e3 * med['obst_adjoint']:.1f} us, six obstacle directions alone {1e3 * med['obst_fwd_6']:.1f} us, "
      f"weights adjoint + lam_wt alone {1e3 * med['wt_adjoint']:.1f} us, seven weight directions alone {1e3 * med['wt_fwd_7']:.1f} us, "
      f"bounds adjoint + lam_bv alone {1e3 * med['bv_adjoint']:.1f} us, nine bound directions alone {1e3 * med['bv_fwd_9']:.1f} us")
