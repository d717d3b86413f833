"""Cost of per-ego obstacle tracks in the closed loop: ms per step of mpc_closed_loop_batch_dev_ex against mpc_closed_loop_batch_obst_dev (with
and without the clearance output), same handle, same egos, alternating samples, medians.  The obstacles are far away, so the solves do the same
work; what the second loop adds is one launch of a B-thread kernel per step (k_loop_obst) and k_transpose_obst in every solve -- and, on a
handle whose bounds have the reference's structure, variant 0 of the loop kernels instead of variant 2, so both
settings of option bound_mask are measured: with bound_mask = 0 the two loops run the same solve kernels.
Usage (GPU box): python tools/loop_obst_cost.py [B] [N] [L] [reps]"""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np
import torch
from helpers import pkg

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
N = int(sys.argv[2]) if len(sys.argv) > 2 else 30
L = int(sys.argv[3]) if len(sys.argv) > 3 else 40
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 15
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
d_traj = torch.empty((B, L, 5), dtype=torch.float64, device=dev)
d_ctrl = torch.empty((B, L, 2), dtype=torch.float64, device=dev)
d_cl = torch.empty((B, L), dtype=torch.float64, device=dev)
d_st = torch.empty((B, L), dtype=torch.int32, device=dev)
s = pkg.BatchedMPCSolver(N, 5)
s.set_bounds()
head = (B, d_init.data_ptr(), d_path.data_ptr(), d_orient.data_ptr(), d_vdes.data_ptr(), L, L, d_traj.data_ptr(), d_ctrl.data_ptr(), d_st.data_ptr())


def plain():
    s.closed_loop_device(*head)


def obst():
    s.closed_loop_device(*head, d_obst_track=d_track.data_ptr(), Lt=L, obst_offset=1.0)


def obst_clearance():
    s.closed_loop_device(*head, d_obst_track=d_track.data_ptr(), Lt=L, obst_offset=1.0, d_clearance=d_cl.data_ptr())


def sample(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    assert not s.last_loop_replayed()
    return (time.perf_counter() - t0) * 1e3 / L


fns = dict(plain=plain, obst=obst, obst_clearance=obst_clearance)
print(f"B={B} N={N} L={L} ({reps} alternating samples each; ms per loop step, median / min):")
for mask in ("1", "0"):
    s.set_option("bound_mask", mask)
    for fn in fns.values():
        fn()
    t = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            t[name].append(sample(fn))
    assert bool((d_st == 1).all())
    med = {name: float(np.median(x)) for name, x in t.items()}
    print(f"  bound_mask={mask}: " + "  ".join(f"{name} {med[name]:.4f} / {min(x):.4f}" for name, x in t.items()) +
          f"   obst - plain {1e3 * (med['obst'] - med['plain']):+.1f} us/step, with clearance {1e3 * (med['obst_clearance'] - med['plain']):+.1f} us/step")
