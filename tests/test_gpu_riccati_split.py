"""GPU (-m gpu): the backward Riccati sweep on two compute waves (riccati_tile: wave 0 the matrix recursion, wave 2 the same recursion plus
the vector half, each storing its own row pairs) through both kernels that contain it -- the persistent launch (k_pipeline) and one launch per
kernel (k_riccati + k_stage) -- at the sizes where it can go wrong:
  B = 64 (one full tile) and B = 70 (a second, ragged tile: lanes without an instance on both waves), N = 30 with nx = 6 and nx = 5
  N = 2  a horizon shorter than the backward ring (RIC_DEPTH = 4 slots: the loader never refills, the sweep is three barriers long)
  B = 64 collision-avoidance cold starts through the obstacle, several of which take inertia corrections: the SYM instantiation and the
         repeated sweep, on both waves (who needs a correction is established on the CPU, from the oracle's trace, and asserted)
Against the oracle at the tolerances of tests/test_gpu_parity.py (same status, same iteration count, |x - x_oracle| < 1e-8; the nonconvex
family: where both end in the same optimum -- at least 85 % -- to 1e-6, a KKT certificate elsewhere), and the two GPU paths against each other
bit for bit.  The GPU work runs in ONE child process (tests/riccati_split_worker.py) under a time limit: the waves of riccati_tile meet at a
barrier per stage, and a wave that walked one barrier too few would hang, not fail."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import CA_CFG, kkt_certificate
from oracle.binding import OracleSolver
from oracle.nlp_numpy import BicycleNLP
from riccati_split_worker import cases

pytestmark = pytest.mark.gpu

TOL_ORACLE = 1e-8          # (tests/test_gpu_parity.py)
HERE = os.path.dirname(os.path.abspath(__file__))
LF = ["lf_nx6_B64", "lf_nx6_B70", "lf_nx5_B64", "lf_nx5_B70", "lf_N2_B64"]


@pytest.fixture(scope="module")
def batches():
    return cases()


@pytest.fixture(scope="module")
def gpu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ricsplit") / "gpu.npz")
    # (six batches of at most 70 instances, two solves each and one traced solve: seconds; the limit is for a launch that never ends)
    subprocess.run([sys.executable, os.path.join(HERE, "riccati_split_worker.py"), out], check=True, timeout=300)
    return np.load(out)


@pytest.fixture(scope="module")
def oracle(batches):
    return {name: OracleSolver(cfg).solve_batch(x0, p, nthreads=8) for name, (cfg, x0, p, _) in batches.items()}


@pytest.mark.parametrize("name", LF + ["ca_B64"])
def test_persistent_launch_and_one_launch_per_kernel_give_the_same_bits(gpu, name):
    assert bool(gpu[f"{name}__pipe__ran"]) and not bool(gpu[f"{name}__kernels__ran"])
    for k in ("x", "status", "iters", "kkt"):
        a, b = gpu[f"{name}__pipe__{k}"], gpu[f"{name}__kernels__{k}"]
        assert a.tobytes() == b.tobytes(), k


@pytest.mark.parametrize("mode", ["pipe", "kernels"])
@pytest.mark.parametrize("name", LF)
def test_lane_following_against_the_oracle(gpu, oracle, name, mode):
    ro = oracle[name]
    x, st, it = gpu[f"{name}__{mode}__x"], gpu[f"{name}__{mode}__status"], gpu[f"{name}__{mode}__iters"]
    assert np.all(st == 1) and np.all(ro["status"] == 1)
    assert np.array_equal(it, ro["iters"])
    err = float(np.abs(x - ro["x"]).max())
    print(f"{name} {mode}: max |x - x_oracle| = {err:.3e}, iterations {it.mean():.2f} / {it.max()}")
    assert err < TOL_ORACLE


def test_collision_avoidance_batch_takes_inertia_corrections_and_matches_the_oracle(gpu, oracle, batches):
    cfg, x0, p, _ = batches["ca_B64"]
    # on the CPU: which instances the oracle's Riccati sweep had to repeat with delta_w > 0 (trace column 5)
    o = OracleSolver(cfg)
    corrected = [b for b in range(len(x0)) if np.any(o.solve(x0[b], p[b], trace=True)["trace"][:, 5] > 0.0)]
    print("instances with an inertia correction in the oracle:", corrected)
    assert len(corrected) >= 1
    # ... and the device's sweeps repeated for them too (delta_w of the traced solve, one launch per kernel)
    dev = [b for b in range(len(x0)) if np.any(gpu["ca_B64__trace_delta"][:, b] > 0.0)]
    print("instances with an inertia correction on the device:", dev)
    assert set(corrected) <= set(dev)
    ro = oracle["ca_B64"]
    nlp = BicycleNLP(CA_CFG)
    for mode in ("pipe", "kernels"):
        x, st, it = gpu[f"ca_B64__{mode}__x"], gpu[f"ca_B64__{mode}__status"], gpu[f"ca_B64__{mode}__iters"]
        both = (ro["status"] == 1) & (st == 1)
        assert both.sum() >= 0.9 * len(x0)
        dist = np.abs(x - ro["x"]).max(axis=1)
        same = both & (dist < 1e-6)
        print(f"ca_B64 {mode}: {int(same.sum())} of {int(both.sum())} in the oracle's optimum, of those {int((it[same] == ro['iters'][same]).sum())} with its iteration count; "
              f"corrected instances: iterations {it[corrected]} (oracle {ro['iters'][corrected]}), distance {dist[corrected]}")
        assert same.sum() >= 0.85 * both.sum()
        for b in np.nonzero(both & ~same)[0][:4]:
            cert = kkt_certificate(nlp, x[b], p[b])
            assert cert["stationarity"] <= 1e-6 and cert["feasibility"] <= 1e-6, (b, cert)
