"""Records tests/golden/pred_obst_ref.npz: the optima of the oracle's dense interior-point method (oracle/ipm_numpy.py, unchanged) on the
per-stage NLP of tests/pred_obst_ref.py, for the families it needs minutes for.  Run from the repository root:
    python tests/golden/make_pred_obst_ref.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import pred_obst_ref as ref  # noqa: E402

RECORDED = (("drift", 30, 5),)

if __name__ == "__main__":
    out = {}
    for name, N, nx in RECORDED:
        sols = [(seed, ref.reference_solve(name, N, seed, nx)) for seed in range(ref.SEEDS)]
        sols = [(s, x) for s, x in sols if x is not None]
        key = f"{name}_n{N}_nx{nx}"
        out[key + "__seeds"] = np.array([s for s, _ in sols], dtype=np.int64)
        out[key + "__x_ref"] = np.array([x for _, x in sols])
        print(key, "converged", len(sols), "of", ref.SEEDS)
    np.savez(ref.GOLDEN, **out)
