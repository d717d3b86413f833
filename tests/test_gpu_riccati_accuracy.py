"""Both Riccati sweeps on the device against the extended-precision reference (tests/riccati_ref.py; the CPU half is
tests/test_riccati_accuracy_cpu.py, which also validates the reference itself).

tools/ubench/ric_mfma_test <cases> <results> (built by __graft_entry__.build) runs every case of the batch, in ONE process,
  * through the one-instance-per-lane recursion as the device compiler builds it (k_lane: ric_matrix_step / ric_vector_step /
    riccati_forward_step, one case and instantiation per lane, the last wavefront partly filled) -- the arithmetic of k_pipeline's
    riccati_tile, fused products and all, which the g++ harness cannot show -- in the three instantiations riccati_tile uses, and
  * through mfma_backward / mfma_forward of csrc/mpc_riccati_mfma.h with one and with two instances per wavefront, delta_last and the
    symmetry mark taken from the case.
Compared here, against the long-double reference only: cost-to-go, gains and step within max(1e-13, MARGIN x e_plain) per family and measure
(e_plain: what a plain float64 recursion loses on the same cases, computed at every run), verdict and delta of the inertia correction and
the sweep count exactly the reference's -- for both members of a two-instance wavefront, whose sweeps are the larger of the two.

The batch has 328 cases -- eight per family, state dimension and horizon, which the asserted coverage asks for, nine in the indefinite
family (three per delta_last) and four rank-one cases once more without the mark -- on 3 x 328 lanes and 2 x 328 wavefront slots: 1 s of GPU time.

Measured on MI355X (worst error / e_plain over the measures P, p, K, dz; every margin stays at 10):
    family               per lane <NX,NX,true> / <NX,NX,false>   <6,5,false>   MFMA x 1 = MFMA x 2
    benign               1.5                                     -             5.3
    barrier              1.6                                     -             6.0
    rank-one, marked     0.0015                                  -             0.0016
    rank-one, unmarked   2.4  (printed, not asserted)            -             3.2
    indefinite           2.4                                     -             8.2
    decoupled            1.2                                     1.2           4.3
"""
import collections
import os
import subprocess

import numpy as np
import pytest

import riccati_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tools", "ubench", "ric_mfma_test")
BLOCKS = ("sym", "plain", "decoupled", "mfma1", "mfma2")          # the result blocks of the binary's case-file mode, in file order


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """the batch, the plain twin's errors and the five result blocks of ONE run of the binary"""
    if not os.path.exists(EXE):
        pytest.fail("tools/ubench/ric_mfma_test is not built: run __graft_entry__.build()")
    cases, _ = R.accuracy_batch()
    d = tmp_path_factory.mktemp("ric")
    fin, fout = str(d / "cases.bin"), str(d / "results.bin")
    R.pack_cases(cases).tofile(fin)
    r = subprocess.run([EXE, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
    return cases, R.plain_errors(cases), split_blocks(np.fromfile(fout), cases)


def split_blocks(flat, cases):
    blk = R.out_size(cases)
    assert flat.size == len(BLOCKS) * blk, (flat.size, blk)
    return {name: R.unpack_results(flat[i * blk:(i + 1) * blk], cases) for i, name in enumerate(BLOCKS)}


def wave_sweeps(cases, per_wave):
    """the sweeps a wavefront of the MFMA form runs for each case: neighbours of a (nx, N) group in file order share one (a group of odd
    size: the last case next to a copy of itself), and a wavefront sweeps until its last instance is done"""
    groups = collections.defaultdict(list)
    for i, c in enumerate(cases):
        groups[c.nx, c.N].append(i)
    out = [0] * len(cases)
    for g in groups.values():
        for j in range(0, len(g), per_wave):
            mates = g[j:j + per_wave]
            for i in mates:
                out[i] = max(cases[q].ref["sweeps"] for q in mates)
    return out


def check(run, block, mine=lambda c: True, families=R.FAMILIES):
    cases, e_plain, blocks = run
    res = blocks[block]
    fails, count = R.judge(block, cases, res, e_plain, mine)
    want = wave_sweeps(cases, 2 if block == "mfma2" else 1)
    for c, r, w in zip(cases, res, want):
        if mine(c) and r["sweeps"] != w:
            fails.append(f"{block} {c.name}: {r['sweeps']} sweeps, reference {w}")
    assert not fails, "\n".join(fails)
    R.check_counts(count, families)
    return res


@pytest.mark.parametrize("block", ["sym", "plain"])
def test_per_lane_recursion_on_the_device(run, block):
    check(run, block)


def test_per_lane_decoupled_instantiation_on_the_device(run):
    cases = run[0]
    res = check(run, "decoupled", lambda c: c.family == "decoupled", ["decoupled"])
    bad = [c.name for c, r in zip(cases, res) if c.family == "decoupled" and not R.decoupled_zeros_exact(c, r)]
    assert not bad, bad


@pytest.mark.parametrize("block", ["mfma1", "mfma2"])
def test_mfma_sweeps(run, block):
    check(run, block)


def test_two_instance_wavefronts_hold_mates_of_both_kinds(run):
    """what test_mfma_sweeps[mfma2] covers: wavefronts of which one instance is swept again and the other is not, and wavefronts whose
    instances both are, a different number of times"""
    cases = run[0]
    one = wave_sweeps(cases, 1)
    two = wave_sweeps(cases, 2)
    waits = sum(o == 1 and t > 1 for o, t in zip(one, two))
    both = sum(1 < o < t for o, t in zip(one, two))
    assert waits >= 8 and both >= 1, (waits, both)
