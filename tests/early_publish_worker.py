"""Child process of tests/test_gpu_early_publish.py: solves the test's batches on the GPU through the persistent launch (k_pipeline) with the
stage items of a tile published before its forward Riccati sweep ends (option pipe_early: the plan's default, off, a lead beyond the horizon)
and through one launch per kernel, and writes what came back into an .npz.  A process of its own so that the test can put the GPU work under a
time limit: a stage worker that waits for a step-ready word nobody writes would not fail, it would wait (for the bounded spin, then the solve
would be run again).  Usage: python early_publish_worker.py OUT.npz"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402

LEADS = (("default", "-1"), ("off", "0"), ("beyond", "100"))        # option pipe_early
HAND_B = 2368                                                       # 37 tiles: the pipeline with k_solve_wg behind it (hand-over at 55 of 64)


def hand_batch():
    from helpers import FAMILIES
    from oracle.nlp_numpy import synthetic_batch
    cfg, kw = FAMILIES["zamlf_n30_nx6"]
    return (cfg, *synthetic_batch(cfg, HAND_B, **kw))


def record(res, key, s, r):
    pp = s.get_pipeline_profile()
    for k, v in (("x", r.x), ("status", r.status), ("iters", r.iters), ("kkt", r.kkt), ("ran", np.array(bool(pp["ran"]))),
                 ("aborts", np.array(int(s.get_option("pipe_aborts"))))):
        res[f"{key}__{k}"] = v


def main(path):
    from helpers import make_solver, set_cfg_bounds
    from riccati_split_worker import cases
    res = {}
    for name, (cfg, x0, p, _) in cases().items():
        s = make_solver(cfg)
        set_cfg_bounds(s, cfg)
        s.set_option("rescue", "0")             # the oracle has no second chance: the first solve
        s.set_option("hybrid", "0")             # the pipeline serves every iteration (no k_solve_wg behind it)
        s.set_option("pipeline", "0")
        record(res, f"{name}__kernels", s, s.solve(x0, p))
        s.set_option("pipeline", "1")
        for tag, lead in LEADS:
            s.set_option("pipe_early", lead)
            record(res, f"{name}__{tag}", s, s.solve(x0, p))
        if name == "lf_nx6_B70":
            # helping Riccati workers: their variant of the kernel publishes behind the sweep whatever the option says
            s.set_option("pipe_early", "-1")
            s.set_option("pipe_help", "1")
            record(res, f"{name}__help", s, s.solve(x0, p))
    # default options: the tiles leave the pipeline for k_solve_wg with instances still iterating
    cfg, x0, p = hand_batch()
    s = make_solver(cfg)
    for tag, lead in LEADS[:2]:
        s.set_option("pipe_early", lead)
        r = s.solve(x0, p)
        record(res, f"hand__{tag}", s, r)
        res[f"hand__{tag}__wg_ran"] = np.array(bool(s.get_resident_profile()["ran"]))
    np.savez(path, **res)


if __name__ == "__main__":
    main(sys.argv[1])
