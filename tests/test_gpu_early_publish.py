"""GPU (-m gpu): early publication in the persistent launch (k_pipeline) -- a tile's stage items go into the ready queue before its forward
Riccati sweep has ended, the stage workers issue the loads that do not read the step, wait for the tile's step-ready word and load the step
behind it (option pipe_early: -1 the plan's default, 0 off, n stages of lead).  Nothing in it changes an operand or an order of operations, so
every lead must give the bytes of every other and of one launch per kernel (k_riccati + k_stage):
  lane following B = 64 (one tile) and B = 70 (a second, ragged tile), N = 30 with nx = 6 and nx = 5
  N = 2                 a horizon shorter than any lead: published at the first forward stage
  B = 64 collision-avoidance cold starts through the obstacle: repeated backward sweeps (the tickets are drawn in front of the drain of the
                        LAST pass only) and the status / delta_w stores that moved in front of that drain
each with the persistent launch serving every iteration (pipeline = 1, hybrid = 0, rescue = 0) at the plan's lead, with the option off and with
a lead beyond the horizon; the lane-following batches also against the oracle at the tolerances of tests/test_gpu_parity.py.  Then one batch
with default options that goes through the hand-over to k_solve_wg (B = 2368), and one with helping Riccati workers (pipe_help = 1: their
kernel publishes behind the sweep).  The GPU work runs in ONE child process (tests/early_publish_worker.py) under a time limit: a stage
worker that waits for a step-ready word nobody writes hangs (until the bounded spin ends the launch), it does not fail."""
import os
import subprocess
import sys

import numpy as np
import pytest

from early_publish_worker import LEADS
from oracle.binding import OracleSolver
from riccati_split_worker import cases

pytestmark = pytest.mark.gpu

TOL_ORACLE = 1e-8          # (tests/test_gpu_parity.py)
HERE = os.path.dirname(os.path.abspath(__file__))
LF = ["lf_nx6_B64", "lf_nx6_B70", "lf_nx5_B64", "lf_nx5_B70", "lf_N2_B64"]
ROWS = ("x", "status", "iters", "kkt")


@pytest.fixture(scope="module")
def batches():
    return cases()


@pytest.fixture(scope="module")
def gpu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("earlypub") / "gpu.npz")
    # (six batches of at most 70 instances, four or five solves each, and two solves of 2368 instances: seconds; the limit is for a launch that never ends)
    r = subprocess.run([sys.executable, os.path.join(HERE, "early_publish_worker.py"), out], timeout=300, capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert "abandoned" not in r.stderr
    return np.load(out)


@pytest.fixture(scope="module")
def oracle(batches):
    return {name: OracleSolver(batches[name][0]).solve_batch(batches[name][1], batches[name][2], nthreads=8) for name in LF}


@pytest.mark.parametrize("tag", [t for t, _ in LEADS])
@pytest.mark.parametrize("name", LF + ["ca_B64"])
def test_every_lead_gives_the_bytes_of_one_launch_per_kernel(gpu, name, tag):
    assert bool(gpu[f"{name}__{tag}__ran"]) and not bool(gpu[f"{name}__kernels__ran"])
    assert int(gpu[f"{name}__{tag}__aborts"]) == 0
    for k in ROWS:
        assert gpu[f"{name}__{tag}__{k}"].tobytes() == gpu[f"{name}__kernels__{k}"].tobytes(), k


@pytest.mark.parametrize("name", LF)
def test_lane_following_against_the_oracle(gpu, oracle, name):
    ro = oracle[name]
    x, st, it = gpu[f"{name}__default__x"], gpu[f"{name}__default__status"], gpu[f"{name}__default__iters"]
    assert np.all(st == 1) and np.all(ro["status"] == 1)
    assert np.array_equal(it, ro["iters"])
    err = float(np.abs(x - ro["x"]).max())
    print(f"{name}: max |x - x_oracle| = {err:.3e}, iterations {it.mean():.2f} / {it.max()}")
    assert err < TOL_ORACLE


def test_hand_over_to_the_stragglers_kernel_gives_the_same_bytes(gpu):
    for tag in ("default", "off"):
        assert bool(gpu[f"hand__{tag}__ran"]) and bool(gpu[f"hand__{tag}__wg_ran"]) and int(gpu[f"hand__{tag}__aborts"]) == 0
    assert np.all(gpu["hand__default__status"] == 1)
    for k in ROWS:
        assert gpu[f"hand__default__{k}"].tobytes() == gpu[f"hand__off__{k}"].tobytes(), k


def test_helping_riccati_workers_give_the_same_bytes(gpu):
    assert bool(gpu["lf_nx6_B70__help__ran"]) and int(gpu["lf_nx6_B70__help__aborts"]) == 0
    for k in ROWS:
        assert gpu[f"lf_nx6_B70__help__{k}"].tobytes() == gpu[f"lf_nx6_B70__kernels__{k}"].tobytes(), k
