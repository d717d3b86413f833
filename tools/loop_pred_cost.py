"""Cost of predicting the obstacle over the horizon in the closed loop: ms per step of mpc_closed_loop_batch_pred_dev with predict 0 (the frozen
loop, mpc_closed_loop_batch_obst_dev's) against predict 1, same handle, same egos, alternating samples in one process, medians.  The obstacles are
far away, so the solves do the same work; what predict 1 adds per step is k_loop_obst_stages (B (N + 1) threads instead of B), k_transpose_obst_stages
(6 (N + 1) doubles per instance through LDS instead of 6) and three 16-byte loads per stage thread and phase in place of six scalar-row loads.
The share of the obstacle rows in a solve: HIP events around single device solves that differ in nothing but the shape of obst -- [B, 6]
against [B, N+1, 6] with every stage row the instance's (the same kernels, the same bits) -- whose difference is the transposer and the
per-stage loads; the library has no event of its own around the transposer.
Usage (GPU box): python tools/loop_pred_cost.py [B] [N] [L] [reps]"""
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
k = np.arange(L + N)
rng = np.random.default_rng(0)
path = np.tile(np.stack([k * v * 0.1 * np.cos(psi), k * v * 0.1 * np.sin(psi)], axis=1), (B, 1, 1))
init = np.tile([0.0, 0.0, 0.0, v, psi], (B, 1))
init[:, 1] += rng.uniform(-0.5, 0.5, B)
init[:, 3] *= rng.uniform(0.9, 1.1, B)
track = np.zeros((B, L + N, 3))
track[:, :, 0] = -100.0 + 0.5 * k[None]                     # (around the descriptor's obstacle at (-100, 0): far behind every ego)
track[:, :, 1] = rng.uniform(-5.0, 5.0, B)[:, None]
dev = "cuda"
d_init, d_path, d_orient, d_vdes, d_track = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (init, path, np.full((B, L + N), psi), np.full(B, v), track))
d_traj = torch.empty((B, L, 5), dtype=torch.float64, device=dev)
d_ctrl = torch.empty((B, L, 2), dtype=torch.float64, device=dev)
d_cl = torch.empty((B, L), dtype=torch.float64, device=dev)
d_st = torch.empty((B, L), dtype=torch.int32, device=dev)
s = pkg.BatchedMPCSolver(N, 5)
s.set_bounds()
head = (B, d_init.data_ptr(), d_path.data_ptr(), d_orient.data_ptr(), d_vdes.data_ptr(), L, L + N, d_traj.data_ptr(), d_ctrl.data_ptr(), d_st.data_ptr())
kw = dict(d_obst_track=d_track.data_ptr(), Lt=L + N, obst_offset=1.0, d_clearance=d_cl.data_ptr())


def frozen():
    s.closed_loop_device(*head, **kw)


def predicted():
    s.closed_loop_device(*head, predict=1, **kw)


def sample(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    assert not s.last_loop_replayed()
    return (time.perf_counter() - t0) * 1e3 / L


fns = dict(predict0=frozen, predict1=predicted)
for fn in fns.values():
    fn()
t = {name: [] for name in fns}
for _ in range(reps):
    for name, fn in fns.items():
        t[name].append(sample(fn))
assert bool((d_st == 1).all())
med = {name: float(np.median(x)) for name, x in t.items()}
print(f"B={B} N={N} L={L} ({reps} alternating samples each; ms per loop step, median / min):")
print("  " + "  ".join(f"{name} {med[name]:.4f} / {min(x):.4f}" for name, x in t.items()) +
      f"   predict1 - predict0 {1e3 * (med['predict1'] - med['predict0']):+.1f} us/step ({100 * (med['predict1'] / med['predict0'] - 1):+.1f} %)")

# one solve, [B, 6] against [B, N+1, 6] with equal stage rows: HIP events around each
from oracle.nlp_numpy import NLPConfig, synthetic_batch  # noqa: E402
cfg = NLPConfig(N=N, nx=5)
x0, p = synthetic_batch(cfg, B)
row = np.tile([-100.0, 0.0, -99.0, 0.0, -101.0, 0.0], (B, 1)) + rng.uniform(-1, 1, (B, 6))
d_x0, d_p, d_row, d_stg = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (x0, p, row, np.repeat(row[:, None, :], N + 1, axis=1)))
d_out = torch.empty_like(d_x0)
d_status = torch.empty(B, dtype=torch.int32, device=dev)


def solve(stages):
    s.solve_device(B, d_x0.data_ptr(), d_p.data_ptr(), d_out.data_ptr(), d_status=d_status.data_ptr(), d_obst=(d_stg if stages else d_row).data_ptr(),
                   obst_stages=stages)


def event_ms(stages):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    solve(stages)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


for stages in (False, True):
    solve(stages)
ts = {False: [], True: []}
for _ in range(reps):
    for stages in (False, True):
        ts[stages].append(event_ms(stages))
m0, m1 = float(np.median(ts[False])), float(np.median(ts[True]))
print(f"  one solve, HIP events: obst [B,6] {m0:.4f} ms  obst [B,N+1,6] {m1:.4f} ms   difference {1e3 * (m1 - m0):+.1f} us = {100 * (m1 - m0) / m1:.1f} % of the per-stage solve "
      f"({B * (N + 1) * 6 * 8 / 1e6:.1f} MB of obstacle rows in, as much out)")
