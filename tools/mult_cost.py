"""Cost of asking a solve for everything CasADi returns (f, g, lam_g, lam_x; mpc_solve_batch_dev_ex) against the plain device solve,
same handle, same batch, alternating samples.
Usage (GPU box): python tools/mult_cost.py [B] [family] [reps]"""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np
import torch
from helpers import FAMILIES, make_solver, set_cfg_bounds
from oracle.nlp_numpy import synthetic_batch

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
fam = sys.argv[2] if len(sys.argv) > 2 else "zamlf_n30_nx6"
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 50
cfg, kw = FAMILIES[fam]
x0, p = synthetic_batch(cfg, B, **kw)
s = make_solver(cfg)
set_cfg_bounds(s, cfg)
dev = "cuda"
tx0, tp = torch.from_numpy(x0).to(dev), torch.from_numpy(p).to(dev)
out = torch.empty_like(tx0)
st = torch.empty(B, dtype=torch.int32, device=dev); it = torch.empty_like(st); kk = torch.empty(B, dtype=torch.float64, device=dev)
f = torch.empty(B, dtype=torch.float64, device=dev)
g = torch.empty((B, s.n_g), dtype=torch.float64, device=dev); lg = torch.empty_like(g)
lx = torch.empty((B, s.n_w), dtype=torch.float64, device=dev)


def plain():
    s.solve_device(B, tx0.data_ptr(), tp.data_ptr(), out.data_ptr(), st.data_ptr(), it.data_ptr(), kk.data_ptr())


def full():
    s.solve_device(B, tx0.data_ptr(), tp.data_ptr(), out.data_ptr(), st.data_ptr(), it.data_ptr(), kk.data_ptr(),
                   d_f=f.data_ptr(), d_g=g.data_ptr(), d_lam_g=lg.data_ptr(), d_lam_x=lx.data_ptr())


def sample(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


for _ in range(5):
    plain(); full()
tp_, tf_ = [], []
for _ in range(reps):
    tp_.append(sample(plain))
    tf_.append(sample(full))
tp_, tf_ = np.array(tp_), np.array(tf_)
print(f"B={B} {fam}: plain median {np.median(tp_):.4f} ms (min {tp_.min():.4f}), with f/g/lam_g/lam_x median {np.median(tf_):.4f} ms "
      f"(min {tf_.min():.4f}); cost median {1e3 * (np.median(tf_) - np.median(tp_)):.1f} us, min-to-min {1e3 * (tf_.min() - tp_.min()):.1f} us")
