"""mpc_forces_closed_loop_batch_dev against mpc_forces_closed_loop_batch_obst_dev (reference mode; shifted guess + predicted moving track) at the bench shape:
device-pointer forms, one process, interleaved windows (profiles/r10_forces_loop_obst.txt).  Usage: python tools/forces_loop_timing.py [out.txt]"""
import importlib, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
pkg = importlib.import_module("motion-planning-for-autonomous-driving-with-mpc_amd")
import floop_ref as ref
from ctypes import c_void_p as vp
B, N, L = 4096, 10, 30
w = ref.WEIGHTS
s = pkg.BatchedMPCSolver(N, 5, Q=w["Q"], R=w["R"], P=w["P"])
rng = np.random.default_rng(1)
init, path, orient, vdes = ref.ego_inputs(B, N, 10.0, y0=rng.uniform(-0.2, 0.2, B))
path, orient = path[:, :L], orient[:, :L]
start, speed, lat = rng.uniform(14, 17, B), rng.uniform(3.5, 4.5, B), rng.uniform(-2.7, -2.3, B)
i = np.arange(L)
track = np.stack([start[:, None] + speed[:, None] * 0.1 * i, np.repeat(lat[:, None], L, 1), np.zeros((B, L))], 2)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
d_init, d_path, d_orient, d_vdes, d_track = map(dev, (init, path, orient, vdes, track))
d_traj, d_ctrl = torch.empty((B, L, 5), dtype=torch.float64, device="cuda"), torch.empty((B, L, 2), dtype=torch.float64, device="cuda")
d_flag, d_cl = torch.empty((B, L), dtype=torch.int32, device="cuda"), torch.empty((B, L), dtype=torch.float64, device="cuda")
abi = importlib.import_module(pkg.__name__ + "._abi")
from importlib import import_module
big = import_module(pkg.__name__ + ".solver")._big
lb, ub, hl, hu = big(ref.LB, 7), big(ref.UB, 7), big(ref.HL, 10), big(ref.HU, 10)
dp = abi.as_dp
def old():
    rc = s._lib.mpc_forces_closed_loop_batch_dev(s._h, B, L, L, vp(d_init.data_ptr()), None, vp(d_path.data_ptr()), vp(d_orient.data_ptr()), vp(d_vdes.data_ptr()),
                                                 dp(lb), dp(ub), dp(hl), dp(hu), 0, 0, 0.0, 0, vp(d_traj.data_ptr()), vp(d_ctrl.data_ptr()), vp(d_flag.data_ptr()), None)
    assert rc == 0
def new(guess=0, predict=0, with_track=False):
    s.forces_closed_loop_obst_device(B, L, L, d_init.data_ptr(), d_path.data_ptr(), d_orient.data_ptr(), d_vdes.data_ptr(), ref.LB, ref.UB, ref.HL, ref.HU,
                                     d_traj.data_ptr(), d_ctrl.data_ptr(), d_flag.data_ptr(), guess_mode=guess, Lt=L if with_track else 0,
                                     d_obst_track=d_track.data_ptr() if with_track else 0, obst_offset=1.0, predict=predict, r_sum=3.3,
                                     d_clearance=d_cl.data_ptr() if with_track else 0)
variants = {"old": old, "new_ref": new, "new_rti_predicted": lambda: new(1, 1, True)}
CALLS, REPS = 10, 9
def timed(fn):
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(CALLS): fn()
    torch.cuda.synchronize(); return (time.perf_counter() - t) / CALLS * 1e3
for fn in variants.values():
    for _ in range(3): fn()
torch.cuda.synchronize()
# same results first
old(); torch.cuda.synchronize(); a = (d_traj.cpu().numpy().copy(), d_ctrl.cpu().numpy().copy(), d_flag.cpu().numpy().copy())
new(); torch.cuda.synchronize(); b = (d_traj.cpu().numpy(), d_ctrl.cpu().numpy(), d_flag.cpu().numpy())
same = all(np.array_equal(x, y) for x, y in zip(a, b))
res = {k: [] for k in variants}
for r in range(REPS):
    for k, fn in variants.items():
        res[k].append(timed(fn))
lines = [f"B={B} N={N} L={L}; ms per loop call (device-pointer form, {CALLS} calls per window, {REPS} interleaved windows); reference mode bit-identical to old: {same}"]
for k, v in res.items():
    v = np.array(v)
    lines.append(f"{k:18s} median {np.median(v):8.3f}  min {v.min():8.3f}  max {v.max():8.3f}  spread(max-min) {v.max()-v.min():7.3f}   ego-steps/s {B*L/np.median(v)*1e3:.3e}")
new(1, 1, True); torch.cuda.synchronize()
fl = d_flag.cpu().numpy()
lines.append(f"rti_predicted: egos with every exitflag 1: {int((fl == 1).all(1).sum())} of {B}; min clearance {float(d_cl.min()):.4f}")
print("\n".join(lines))
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
