"""Cost of the linearised closed loop: ms per step of the step-by-step plain loop (option loop_async = 0) against mpc_closed_loop_batch_lin_dev with
two families of gains (kgain, wgain) and with three (ogain too, on an obstacle track), and ms of one tangent sweep (n_dir directions) and of one
adjoint sweep over the recorded gains.  Same handle, same egos, alternating samples in one process after a warm-up, medians.  The obstacles are
far away, so every loop's solves do the same work.
Usage (GPU box): python tools/loop_lin_cost.py [B] [N] [L] [reps] [nx] [n_dir]"""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np
import torch
from helpers import pkg

arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d      # noqa: E731
B, N, L, reps, nx, n_dir = arg(1, 4096), arg(2, 30), arg(3, 40), arg(4, 9), arg(5, 6), arg(6, 12)
v, psi = 15.0, 0.1
k = np.arange(L)
rng = np.random.default_rng(0)
path = np.tile(np.stack([k * v * 0.1 * np.cos(psi), k * v * 0.1 * np.sin(psi)], axis=1), (B, 1, 1))
init = np.tile([0.0, 0.0, 0.0, v, psi], (B, 1))
init[:, 1] += rng.uniform(-0.5, 0.5, B)
init[:, 3] *= rng.uniform(0.9, 1.1, B)
track = np.zeros((B, L, 3))
track[:, :, 0] = -100.0 + 0.5 * k[None]                     # (around the descriptor's obstacle at (-100, 0): far behind every ego)
track[:, :, 1] = rng.uniform(-5.0, 5.0, B)[:, None]
dev = "cuda"
d_init, d_path, d_orient, d_vdes, d_track = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (init, path, np.full((B, L), psi), np.full(B, v), track))
new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)      # noqa: E731
d_traj, d_ctrl, d_kg, d_wg, d_og = new(B, L, 5), new(B, L, 2), new(B, L, 2, 5), new(B, L, 2, 7), new(B, L, 2, 3)
d_st = torch.empty((B, L), dtype=torch.int32, device=dev)
d_dinit, d_dwt, d_dtrack = (torch.randn(shape, dtype=torch.float64, device=dev) for shape in ((B, n_dir, 5), (B, n_dir, 7), (B, n_dir, L, 3)))
d_dtraj, d_dctrl = new(B, n_dir, L, 5), new(B, n_dir, L, 2)
d_seed_t, d_seed_c = torch.randn((B, L, 5), dtype=torch.float64, device=dev), torch.randn((B, L, 2), dtype=torch.float64, device=dev)
d_gi, d_gw, d_gt = new(B, 5), new(B, 7), new(B, L, 3)
s = pkg.BatchedMPCSolver(N, nx)
s.set_bounds()
s.set_option("loop_async", "0")
head = (B, d_init.data_ptr(), d_path.data_ptr(), d_orient.data_ptr(), d_vdes.data_ptr(), L, L, d_traj.data_ptr(), d_ctrl.data_ptr(), d_st.data_ptr())
tr = dict(d_obst_track=d_track.data_ptr(), Lt=L, obst_offset=1.0)
gains = dict(d_kgain=d_kg.data_ptr(), d_wgain=d_wg.data_ptr(), d_ogain=d_og.data_ptr())
loops = dict(plain=lambda: s.closed_loop_device(*head),
             lin_kw=lambda: s.closed_loop_lin_device(*head, d_kgain=d_kg.data_ptr(), d_wgain=d_wg.data_ptr()),
             plain_track=lambda: s.closed_loop_device(*head, **tr),
             lin_kwo=lambda: s.closed_loop_lin_device(*head, **tr, **gains))
sweeps = dict(tangent=lambda: s.loop_tangent_device(B, L, n_dir, d_traj.data_ptr(), d_ctrl.data_ptr(), **gains, Lt=L, d_dinit=d_dinit.data_ptr(), d_dwt=d_dwt.data_ptr(),
                                                    d_dtrack=d_dtrack.data_ptr(), d_dtraj=d_dtraj.data_ptr(), d_dctrl=d_dctrl.data_ptr()),
              adjoint=lambda: s.loop_adjoint_device(B, L, d_traj.data_ptr(), d_ctrl.data_ptr(), **gains, Lt=L, d_seed_traj=d_seed_t.data_ptr(), d_seed_ctrl=d_seed_c.data_ptr(),
                                                    d_grad_init=d_gi.data_ptr(), d_grad_wt=d_gw.data_ptr(), d_grad_track=d_gt.data_ptr()))


def sample(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


print(f"B={B} N={N} nx={nx} L={L} n_dir={n_dir} ({reps} alternating samples each, median / min):", flush=True)
for fn in list(loops.values()) + list(sweeps.values()):
    fn()
t = {name: [] for name in list(loops) + list(sweeps)}
for _ in range(reps):
    for name, fn in loops.items():
        t[name].append(sample(fn) / L)
    for name, fn in sweeps.items():
        t[name].append(sample(fn))
assert bool((d_st == 1).all()) and bool(torch.isfinite(d_kg).all()) and bool(torch.isfinite(d_dtraj).all()) and bool(torch.isfinite(d_gi).all())
med = {name: float(np.median(x)) for name, x in t.items()}
print("  ms per loop step: " + "  ".join(f"{name} {med[name]:.4f} / {min(t[name]):.4f}" for name in loops), flush=True)
print(f"  two families {1e3 * (med['lin_kw'] - med['plain']):+.1f} us/step, three {1e3 * (med['lin_kwo'] - med['plain_track']):+.1f} us/step", flush=True)
print("  ms per sweep: " + "  ".join(f"{name} {med[name]:.4f} / {min(t[name]):.4f}" for name in sweeps), flush=True)
