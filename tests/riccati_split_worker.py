"""Child process of tests/test_gpu_riccati_split.py: solves the test's batches on the GPU through the persistent launch (k_pipeline) and
through one launch per kernel (k_riccati + k_stage) and writes what came back into an .npz.  A process of its own so that the test can put
the GPU work under a time limit: riccati_tile's waves meet at one workgroup barrier per stage, and a wave that walked one barrier too few would
not fail, it would wait.  Usage: python riccati_split_worker.py OUT.npz"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402


def cases():
    """name -> (cfg, x0, p, collision avoidance?); shared with the test, which computes the oracle's side"""
    from helpers import CA_CFG, FAMILIES, ca_batch
    from oracle.nlp_numpy import NLPConfig, synthetic_batch
    out = {}
    for nx in (6, 5):
        cfg, kw = FAMILIES[f"zamlf_n30_nx{nx}"]
        for B in (64, 70):                      # one full tile; a second, ragged one
            out[f"lf_nx{nx}_B{B}"] = (cfg, *synthetic_batch(cfg, B, **kw), False)
    cfg = NLPConfig(N=2, nx=5)                  # a horizon shorter than the backward ring (RIC_DEPTH = 4 slots)
    out["lf_N2_B64"] = (cfg, *synthetic_batch(cfg, 64), False)
    out["ca_B64"] = (CA_CFG, *ca_batch(CA_CFG, 64), True)       # cold starts through the obstacle: inertia corrections (asserted by the test)
    return out


def main(path):
    from helpers import make_solver, set_cfg_bounds
    res = {}
    for name, (cfg, x0, p, _) in cases().items():
        s = make_solver(cfg)
        set_cfg_bounds(s, cfg)
        s.set_option("rescue", "0")             # the oracle has no second chance: the first solve
        s.set_option("hybrid", "0")             # riccati_tile serves every iteration (no k_solve_wg behind the pipeline)
        for mode, pipe in (("kernels", "0"), ("pipe", "1")):
            s.set_option("pipeline", pipe)
            r = s.solve(x0, p)
            pp = s.get_pipeline_profile()
            for k, v in (("x", r.x), ("status", r.status), ("iters", r.iters), ("kkt", r.kkt), ("ran", np.array(bool(pp["ran"])))):
                res[f"{name}__{mode}__{k}"] = v
        if name == "ca_B64":
            _, tr = s.solve_trace(x0, p)
            res["ca_B64__trace_delta"] = np.asarray(tr)[:, 5, :]
    np.savez(path, **res)


if __name__ == "__main__":
    main(sys.argv[1])
