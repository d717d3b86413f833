"""GPU (-m gpu): parity of the HIP path, called through the C-ABI (include/mpcgpu.h), against the oracle, the
committed golden optima and size-independent properties at BASELINE.json's full sizes.

Tolerances: BASELINE.json's north_star asks for 1e-4 on optimal state/control trajectories.  The kernels run the
same algorithm as the oracle in IEEE double, so the tests below hold them to 1e-8 against the oracle and 2e-6
against the independent scipy optima (scipy's own accuracy)."""
import os

import numpy as np
import pytest

from helpers import (CA_CFG, FAMILIES, WEIGHTS_YAML_ZAM_LF, OracleBackend, abi, ca_batch, cfg_from_golden, make_configuration,
                     make_solver, pkg, set_cfg_bounds, straight_path)
from oracle.binding import OracleSolver
from oracle.nlp_numpy import BicycleNLP, NLPConfig, synthetic_batch

pytestmark = pytest.mark.gpu
opt = __import__("importlib").import_module("motion-planning-for-autonomous-driving-with-mpc_amd.optimizer")

TOL_ORACLE = 1e-8
TOL_GOLDEN = 2e-6


@pytest.mark.parametrize("fam", list(FAMILIES))
def test_matches_oracle(fam):
    cfg, kw = FAMILIES[fam]
    B = 256
    x0, p = synthetic_batch(cfg, B, **kw)
    s = make_solver(cfg)
    set_cfg_bounds(s, cfg)
    r = s.solve(x0, p)
    ro = OracleSolver(cfg).solve_batch(x0, p, nthreads=8)
    assert np.all(r.status == 1) and np.all(ro["status"] == 1)
    assert np.array_equal(r.iters, ro["iters"])
    assert np.abs(r.x - ro["x"]).max() < TOL_ORACLE
    assert r.kkt.max() <= 1e-8


@pytest.mark.parametrize("fam,B", [("zamlf_n30_nx6", 4096), ("usalf_n50_nx5", 2048), ("zamlf_n30_nx5", 2048), ("zamlf_n10_nx5", 4096)])
def test_every_instance_of_a_full_batch_against_the_oracle(fam, B):
    """BASELINE.json's metric configuration (N = 30, nx = 6, B = 4096) and the other lane-following families at full batch sizes: EVERY
    instance against the C oracle -- same iteration count, |x - x_oracle| <= 1e-8, same status -- on the default path (variant 2 of the
    kernels, hybrid solve, device math helpers); north_star asks for 1e-4 against IPOPT, the oracle restates IPOPT's algorithm"""
    cfg, kw = FAMILIES[fam]
    x0, p = synthetic_batch(cfg, B, **kw)
    s = make_solver(cfg)
    set_cfg_bounds(s, cfg)
    r = s.solve(x0, p)
    ro = OracleSolver(cfg).solve_batch(x0, p, nthreads=16)
    assert np.all(r.status == 1) and np.all(ro["status"] == 1)
    assert np.array_equal(r.iters, ro["iters"])
    assert np.abs(r.x - ro["x"]).max() < TOL_ORACLE


@pytest.mark.parametrize("fam", [f"{w}_n{n}_nx5" for w in ("zamlf", "usalf", "zamca", "first") for n in (10, 30, 50)] + ["zamlf_n30_nx6"])
def test_matches_golden_optima(golden_dir, fam):
    """the grid of SURVEY.md section 8(c): optima from COLD starts of two scipy solvers (none seeded by the oracle or the kernels);
    the nonconvex collision-avoidance family keeps every local optimum found, the kernel must land in one of them"""
    from test_oracle_golden import nearest_basin
    g = np.load(os.path.join(golden_dir, "nlp_optima.npz"))
    cfg = cfg_from_golden(g[f"{fam}__cfg"])
    s = make_solver(cfg)
    set_cfg_bounds(s, cfg)
    r = s.solve(g[f"{fam}__x0"], g[f"{fam}__p"])
    assert np.all(r.status == 1)
    basins = []
    for b in range(len(r.x)):
        k, dist = nearest_basin(r.x[b], g[f"{fam}__w_alt"][b], g[f"{fam}__f_alt"][b])
        basins.append(k)
        assert dist <= max(TOL_GOLDEN, 2 * g[f"{fam}__dtc_alt"][b, k]), (fam, b, k, dist)      # scipy's own accuracy per optimum
    print(fam, "basins the kernel lands in:", basins)


@pytest.mark.parametrize("B", [1, 2, 15, 16, 17, 63, 64, 65, 130])
def test_ragged_batch_sizes(B):
    cfg, kw = FAMILIES["zamlf_n30_nx6"]
    x0, p = synthetic_batch(cfg, 130, **kw)
    s = make_solver(cfg)
    full = s.solve(x0, p)
    part = s.solve(x0[:B], p[:B])
    assert np.array_equal(part.x, full.x[:B]) and np.array_equal(part.iters, full.iters[:B])


def test_batches_beyond_the_workspace_limit_are_solved_in_chunks():
    """the workspace is addressed with 32-bit offsets (< 4 GiB, ~100 k instances at N = 30); a larger batch is cut into chunks of
    whole tiles behind the C-ABI.  Option "max_batch" lowers the limit so that the path can be exercised: same bits as one solve."""
    cfg, kw = FAMILIES["zamlf_n30_nx6"]
    x0, p = synthetic_batch(cfg, 300, **kw)
    s = make_solver(cfg)
    full = s.solve(x0, p)
    s.set_option("max_batch", "128")                      # 128 + 128 + 44
    part = s.solve(x0, p)
    assert _same(part, full)
    x0c, pc = ca_batch(CA_CFG, 200)
    sc = make_solver(CA_CFG)
    set_cfg_bounds(sc, CA_CFG)
    fullc = sc.solve(x0c, pc)
    n = sc.last_rescued()
    sc.set_option("max_batch", "64")
    partc = sc.solve(x0c, pc)
    assert _same(partc, fullc) and sc.last_rescued() == n and np.all(partc.status == 1)


# shift of the per-instance obstacle rows of the test below, in metres per row index: with it 17 of the 1024 instances stall without the
# second chance (counted at the commit before the host solve chain took its rows as one struct)
OBST_ROW_SHIFT = 1e-4


def test_chunks_with_obstacle_rows_absent_outputs_multipliers_sensitivities_and_second_chance():
    """every per-instance buffer of a solve through the chunk loop at once: obstacle rows (width 6) that differ from row to row, multipliers
    (n_g, n_w), the snapshot behind lam_p / dw, a stalled instance in each of the three chunks (the second chance's sub-batch), and a device
    call whose status / iters / kkt are absent.  A wrong row width, or a chunk that reads another chunk's rows, changes bits."""
    import torch
    cfg = CA_CFG
    x0, p = ca_batch(cfg, 1024)
    obst = np.tile(np.asarray(cfg.obstacle_centers, dtype=np.float64).ravel(), (1024, 1)) + OBST_ROW_SHIFT * np.arange(1024)[:, None]
    s0 = make_solver(cfg)
    set_cfg_bounds(s0, cfg)
    s0.set_option("rescue", "0")
    plain = s0.solve(x0, p, obst)
    stalled, ok = np.nonzero(plain.status != 1)[0], np.nonzero(plain.status == 1)[0]
    print("stalled without the second chance:", stalled.size, "of 1024")
    rows = ok[:130].copy()
    placed = [3, 70, 129][: min(3, stalled.size)]
    rows[placed] = stalled[: len(placed)]
    assert len(placed) > 0
    x0, p, obst = (np.ascontiguousarray(a[rows]) for a in (x0, p, obst))
    B = 130
    seeds = np.zeros((B, 2, cfg.n_w))
    seeds[:, 0, 2 * cfg.N] = 1.0                         # xref_0[0]
    seeds[:, 1, 2 * cfg.N + 1] = 1.0                     # xref_0[1]
    s = make_solver(cfg)
    set_cfg_bounds(s, cfg)
    a = s.solve(x0, p, obst, multipliers=True, lam_p=True, dp=seeds)
    na = s.last_rescued()
    s.set_option("max_batch", "64")                      # 64 + 64 + 2
    b = s.solve(x0, p, obst, multipliers=True, lam_p=True, dp=seeds)
    for name in ("x", "status", "iters", "kkt", "f", "g", "lam_g", "lam_x", "lam_p", "dw"):
        assert np.array_equal(getattr(a, name), getattr(b, name), equal_nan=True), name
    assert s.last_rescued() == na and na > 0
    assert np.all(a.status[placed] == 1) and np.all(b.status[placed] == 1)
    d = [torch.from_numpy(v).cuda() for v in (x0, p, obst)]
    out = torch.empty_like(d[0])
    s.solve_device(B, d[0].data_ptr(), d[1].data_ptr(), out.data_ptr(), d_obst=d[2].data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), a.x)


@pytest.mark.parametrize("env", ["MPCGPU_BIG_WG", "MPCGPU_GROUPS"])
def test_optional_kernel_variants_are_bit_identical(env, monkeypatch):
    """The opt-in variants (512-thread stage workgroups -- the kernel long horizons use --, sub-batch streams) run the
    same arithmetic: results must equal the default path bit for bit, run after run (the 512-thread kernel is the one
    in which a 16-byte store was once followed directly by a VALU write of its data register, see ws_store2)."""
    cfg, kw = FAMILIES["zamlf_n30_nx6"]
    x0, p = synthetic_batch(cfg, 600, **kw)
    s = make_solver(cfg)
    s.set_option("hybrid", "0")                # (the streaming paths against each other: the hybrid solve rounds differently)
    ref = s.solve(x0, p)
    s.set_option(env[len("MPCGPU_"):].lower(), "2" if env == "MPCGPU_GROUPS" else "1")
    for _ in range(4):
        alt = s.solve(x0, p)
        assert np.array_equal(alt.x, ref.x) and np.array_equal(alt.iters, ref.iters) and np.array_equal(alt.status, ref.status)


@pytest.mark.parametrize("fam,B,masked", [("zamlf_n30_nx6", 4096, True), ("usalf_n50_nx5", 2500, True), ("zamlf_n30_nx6", 1500, False)])
def test_riccati_workers_that_help_with_stage_items_change_nothing(fam, B, masked):
    """Option pipe_help (k_pipeline<.., HELP>; default: on when a round has more than three stage items per stage worker, e.g. N = 50): a Riccati
    worker whose tile has just gone to the stage workers takes one published stage item itself instead of idling.  Who serves an item does not
    enter the arithmetic: rows, statuses and iteration counts are the bits of the launch without helpers, with the hybrid solve and without it,
    run after run (a helper that drew a ticket for an item nobody publishes, or released a tile's arrival counter early, would show here as a
    timeout / restart or as different bits)."""
    cfg, kw = FAMILIES[fam]
    x0, p = synthetic_batch(cfg, B, **kw)
    s = make_solver(cfg)
    if masked:
        set_cfg_bounds(s, cfg)
    assert s.get_option("pipe_help") == -1
    for hyb in ("1", "0"):
        s.set_option("hybrid", hyb)
        s.set_option("pipe_help", "0")
        ref = s.solve(x0, p)
        piped = hyb == "0" or B > 2048                     # (the hybrid solve of a small batch has no pipeline launch at all)
        assert s.get_pipeline_profile()["ran"] == piped and np.all(ref.status == 1)
        s.set_option("pipe_help", "1")
        for _ in range(3):
            alt = s.solve(x0, p)
            assert s.get_pipeline_profile()["ran"] == piped
            assert np.array_equal(alt.x, ref.x) and np.array_equal(alt.iters, ref.iters) and np.array_equal(alt.status, ref.status)


@pytest.mark.parametrize("opts", [(("hybrid", "0"),), (("hybrid", "0"), ("pipeline", "0")), ()])
def test_poisoned_workspace_changes_nothing_on_single_tile_xcds(opts):
    """Option poison: NaN into every row of every tile of the workspace before a solve.  (a) A solve reads nothing it has not written itself -- no
    NaN comes out, every row is the bits of the unpoisoned solve; (b) at B = 600 six of the eight XCDs hold ONE tile, 31 stage workers share its 8 items
    per round and idle for rounds with their L1 untouched: the configuration in which a stage worker was found to read its own stale copy of a line when a
    16-byte store re-created that line at the end of a stage item (profiles/r05_store_pairing.txt; invariants (I1) / (I2) of DESIGN.md section 4) --
    repeated, every repetition must be the same bits."""
    cfg, kw = FAMILIES["zamlf_n30_nx6"]
    x0, p = synthetic_batch(cfg, 600, **kw)
    s = make_solver(cfg)
    for k, v in opts:
        s.set_option(k, v)
    ref = s.solve(x0, p)
    assert np.all(ref.status == 1)
    s.set_option("poison", "1")
    for rep in range(4):
        a = s.solve(x0, p)
        assert np.all(np.isfinite(a.x)) and np.array_equal(a.status, ref.status), rep
        assert np.array_equal(a.x, ref.x) and np.array_equal(a.iters, ref.iters), rep


@pytest.mark.parametrize("fam,B,masked", [("zamlf_n30_nx6", 4096, True), ("usalf_n50_nx5", 3000, True), ("zamlf_n30_nx5", 2600, False)])
def test_mailbox_rows_written_by_the_pipeline_equal_the_ones_copied_at_the_hand_over(fam, B, masked):
    """The stage items of a tile that is about to leave the pipeline write iterate, multipliers and stage block into the instance-major mailbox
    arrays as well (Ctx::mbw), and k_solve_wg takes those instances over without copying them out of the tile-major rows (bit 31 of the tile's
    arrival counter tells it).  Rows, statuses and iteration counts of a batch must be the bits of its first solve on a fresh handle, run after
    run -- stale mailbox rows of an earlier solve (a different batch is solved in between) or a tile flagged without its last items having written
    them would show here.  (Round 5 compared with the copying take-over, option mb_pipe = 0, bit for bit; the option is gone with its use.)"""
    cfg, kw = FAMILIES[fam]
    x0, p = synthetic_batch(cfg, B, **kw)
    x0b, pb = synthetic_batch(cfg, B, start=50000, **kw)
    s = make_solver(cfg)
    if masked:
        set_cfg_bounds(s, cfg)
    ref = s.solve(x0, p)
    assert s.get_pipeline_profile()["ran"] and s.get_resident_profile()["ran"] and np.all(ref.status == 1)
    for rep in range(3):
        other = s.solve(x0b, pb)                                           # (leaves ITS rows in the mailbox)
        assert np.all(other.status == 1)
        alt = s.solve(x0, p)
        assert s.get_pipeline_profile()["ran"] and s.get_resident_profile()["ran"]
        assert np.array_equal(alt.x, ref.x) and np.array_equal(alt.iters, ref.iters) and np.array_equal(alt.status, ref.status), rep


@pytest.mark.parametrize("fam", ["zamlf_n30_nx6", "zamlf_n30_nx5", "usalf_n50_nx5"])
def test_compiled_in_bound_structure_against_the_run_time_lookup(fam):
    """Variant 2 of the kernels (option bound_mask, the default whenever the handle's bounds have the reference's structure: only steering
    rate, acceleration, steering angle and speed bounded, circle rows with a lower bound only and multiplicity 3) compiles that structure
    into the stage phases; variant 0 looks every side up at run time.  Same algorithm, different instruction streams (the compiler
    contracts a few expressions differently): same iteration counts and statuses, |dx| at round-off level, both against the oracle --
    and the specialised phases give the same bits on every path of a handle (pipeline, hybrid off, one launch per kernel)."""
    cfg, kw = FAMILIES[fam]
    x0, p = synthetic_batch(cfg, 700, **kw)
    s = make_solver(cfg)
    set_cfg_bounds(s, cfg)
    assert s.get_option("bound_mask") == 1
    a = s.solve(x0, p)
    s.set_option("hybrid", "0")
    a_pipe = s.solve(x0, p)
    s.set_option("pipeline", "0")
    a_launch = s.solve(x0, p)
    assert _same(a_pipe, a_launch)
    s.set_option("pipeline", "1")
    s.set_option("hybrid", "1")
    s.set_option("bound_mask", "0")
    b = s.solve(x0, p)
    assert np.array_equal(a.status, b.status) and np.array_equal(a.iters, b.iters) and np.all(a.status == 1)
    assert np.max(np.abs(a.x - b.x)) < 1e-9 and np.max(np.abs(a_pipe.x - b.x)) < 1e-9
    ro = OracleSolver(cfg).solve_batch(x0[:64], p[:64], nthreads=8)
    assert np.array_equal(a.iters[:64], ro["iters"]) and np.max(np.abs(a.x[:64] - ro["x"])) < TOL_ORACLE


@pytest.mark.parametrize("fam", ["zamlf_n30_nx6", "zamlf_n30_nx5", "usalf_n50_nx5", "ca", "transposed"])
def test_start_point_safeguard_in_the_fused_start_kernel_and_on_its_own(fam):
    """The start-point safeguard (one thread per instance and stage, three short scans) inside k_start -- guess and reference read from LDS -- against
    the same code as a kernel of its own behind k_ingest (k_prestart_par + k_stage<INIT>: what horizons above 63 use; forced here by the 512-thread
    stage workgroups of option big_wg): same rollout, same decisions, hence the same solve bit for bit -- lane following, the long horizon,
    collision-avoidance cold starts, and the reference's transposed step-0 state guess, for which the safeguard takes the
    rollout.  (The two-chain form of the safeguard, prestart_chain, is what the CPU harness steps: tests/test_emulated_kernels.py.)"""
    if fam == "ca":
        cfg, (x0, p) = CA_CFG, ca_batch(CA_CFG, 300)
    elif fam == "transposed":
        cfg, kw = FAMILIES["zamlf_n30_nx5"]
        x0, p = synthetic_batch(cfg, 200, **kw)
        N, nx = cfg.N, cfg.nx
        X = x0[:, 2 * N:].reshape(-1, N + 1, nx)
        x0 = x0.copy()
        x0[:, 2 * N:] = X.transpose(0, 2, 1).reshape(-1, (N + 1) * nx)       # state guess handed over in the (nx, N+1) order
    else:
        cfg, kw = FAMILIES[fam]
        x0, p = synthetic_batch(cfg, 600, **kw)
    s = make_solver(cfg)
    set_cfg_bounds(s, cfg)
    s.set_option("rescue", "0")
    s.set_option("hybrid", "0")
    s.set_option("pipeline", "0")               # (one launch per kernel on both sides: the 512-thread kernels have no pipeline)
    new = s.solve(x0, p)
    s.set_option("big_wg", "1")
    old = s.solve(x0, p)
    assert _same(new, old)
    if fam == "transposed":
        assert np.all(new.status == 1)


def _same(a, b):
    return np.array_equal(a.x, b.x) and np.array_equal(a.iters, b.iters) and np.array_equal(a.status, b.status) and np.array_equal(a.kkt, b.kkt)


@pytest.mark.parametrize("B,fixed", [(4096, 0), (4096, 20), (1000, 0), (2048 + 17, 0), (8192, 0)])
def test_single_launch_pipeline_is_bit_identical(B, fixed, monkeypatch):
    """k_pipeline (all iterations in one persistent launch, tiles cycling independently between Riccati and stage workers)
    runs the same per-instance arithmetic as one launch per kernel and iteration: bit-identical results, and it is the
    path that actually ran."""
    cfg, kw = FAMILIES["zamlf_n30_nx6"]
    x0, p = synthetic_batch(cfg, B, **kw)
    s = make_solver(cfg, fixed_iters=fixed) if fixed else make_solver(cfg)
    s.set_option("hybrid", "0")                # (the pure pipeline; the hybrid solve has its own tests below)
    s.set_option("pipeline", "0")
    ref = s.solve(x0, p)
    assert not s.get_pipeline_profile()["ran"]
    s.set_option("pipeline", "1")
    for _ in range(3):                       # repeated: the hand-offs must not depend on what the caches hold from the last solve
        alt = s.solve(x0, p)
        pp = s.get_pipeline_profile()
        assert pp["ran"] and pp["rounds"] == int(ref.iters.max()) and pp["stage_workers"] > 0 and pp["riccati_workers"] > 0
        assert _same(alt, ref)


def test_single_launch_pipeline_on_collision_avoidance(monkeypatch):
    """long nonconvex solves (up to max_iter, inertia corrections, failures): the tiles of a batch finish tens of
    iterations apart, which is what the pipeline is for; results stay bit-identical"""
    B = 1024
    x0, p = ca_batch(CA_CFG, B)
    s = make_solver(CA_CFG)
    set_cfg_bounds(s, CA_CFG)
    s.set_option("hybrid", "0")
    s.set_option("pipeline", "0")
    ref = s.solve(x0, p)
    s.set_option("pipeline", "1")
    alt = s.solve(x0, p)
    assert s.get_pipeline_profile()["ran"] and _same(alt, ref)


@pytest.mark.parametrize("mask", ["0x0F", "0x81", "0x10"])
def test_pipeline_on_a_subset_of_the_xcds(mask, monkeypatch):
    """The pipeline routes a tile's work by the XCD a workgroup really runs on and learns the set of XCDs from the device
    (8 on a whole MI355X, fewer in a partitioned mode).  MPCGPU_PIPE_XCD_MASK pretends XCDs away: workgroups that land
    there leave, the tiles are dealt to the remaining ones -- four, two or a single XCD -- and the bits stay the same."""
    cfg, kw = FAMILIES["zamlf_n30_nx6"]
    x0, p = synthetic_batch(cfg, 1500, **kw)
    s = make_solver(cfg)
    s.set_option("hybrid", "0")
    s.set_option("pipeline", "0")
    ref = s.solve(x0, p)
    s.set_option("pipeline", "1")
    s.set_option("pipe_xcd_mask", mask)
    alt = s.solve(x0, p)
    assert s.get_pipeline_profile()["ran"] and _same(alt, ref)


def test_pipeline_restart(monkeypatch):
    """Option pipe_test_abort raises the pipeline's abort word: the host must notice and start over with one launch per kernel from the
    untouched inputs -- also when rows of the abandoned attempt have already reached the caller's buffers (the loop kernels write them
    themselves): the restart overwrites every one of them.  One abandoned launch may be a transient (another tenant's workgroups held the
    CUs): the next solve tries the pipeline again; after three the handle stays on one launch per kernel (state `pipe_disabled`)."""
    cfg, kw = FAMILIES["zamlf_n30_nx6"]
    x0, p = synthetic_batch(cfg, 2048, **kw)
    s = make_solver(cfg)
    s.set_option("hybrid", "0")
    s.set_option("pipeline", "0")
    ref = s.solve(x0, p)
    s.set_option("pipeline", "1")
    assert _same(s.solve(x0, p), ref) and s.get_pipeline_profile()["ran"]
    s.set_option("pipe_test_abort", "1")
    assert _same(s.solve(x0, p), ref) and not s.get_pipeline_profile()["ran"]
    assert s.get_option("pipe_aborts") == 1 and s.get_option("pipe_disabled") == 0
    s.set_option("pipe_test_abort", None)
    assert _same(s.solve(x0, p), ref) and s.get_pipeline_profile()["ran"]          # a single abandoned launch: the pipeline is tried again
    s.set_option("pipe_test_abort", "1")
    for n in (2, 3):
        assert _same(s.solve(x0, p), ref) and not s.get_pipeline_profile()["ran"] and s.get_option("pipe_aborts") == n
    assert s.get_option("pipe_disabled") == 1
    s.set_option("pipe_test_abort", None)
    assert _same(s.solve(x0, p), ref) and not s.get_pipeline_profile()["ran"] and s.get_option("pipe_aborts") == 3      # three: this handle stays on the per-kernel path
    # the same with the hybrid solve behind the pipeline: the kernel that finishes the stragglers sees the abort word and leaves,
    # the restart is the per-kernel path
    s2 = make_solver(cfg)
    s2.set_option("hybrid_live", "16")
    s2.set_option("pipe_test_abort", "1")
    assert _same(s2.solve(x0, p), ref) and not s2.get_pipeline_profile()["ran"] and s2.get_option("pipe_aborts") == 1


def test_two_handles_solve_concurrently():
    """Two handles driven from two host threads: their persistent launches compete for the same CUs (each wants one
    workgroup per CU).  Whatever the dispatcher does -- interleave them, starve one for a while, or make a bounded wait
    run out so that a solve restarts on the per-kernel path -- both must return the bits of a solve that ran alone."""
    import threading
    cfg, kw = FAMILIES["zamlf_n30_nx6"]
    xa, pa = synthetic_batch(cfg, 2048, **kw)
    xb, pb = synthetic_batch(cfg, 3000, start=5000, **kw)
    sa, sb = make_solver(cfg), make_solver(cfg)
    ra, rb = sa.solve(xa, pa), sb.solve(xb, pb)
    out = {}

    def work(name, s, x, p):
        out[name] = [s.solve(x, p) for _ in range(6)]

    ts = [threading.Thread(target=work, args=("a", sa, xa, pa)), threading.Thread(target=work, args=("b", sb, xb, pb))]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in ts)
    assert all(_same(r, ra) for r in out["a"]) and all(_same(r, rb) for r in out["b"])


def test_full_size_batch_properties():
    """BASELINE metric size: N = 30, nx = 6, B = 4096.  Size-independent properties: every instance converged;
    permuting instances / splitting the batch changes nothing -- bit-exactly on the streaming paths; with the hybrid solve (default)
    which KKT solver (one instance per lane, or one per wavefront on the matrix pipe) serves an iteration of an instance depends on
    how many instances of its tile are still iterating, the two round differently, and the property holds to 1e-9 with the same
    iteration counts; the returned points satisfy the reference's constraints g (checked with the oracle's g on a sample)."""
    cfg, kw = FAMILIES["zamlf_n30_nx6"]
    B = 4096
    x0, p = synthetic_batch(cfg, B, **kw)
    perm = np.random.default_rng(0).permutation(B)
    s = make_solver(cfg)
    for hybrid in ("0", "1"):
        s.set_option("hybrid", hybrid)
        r = s.solve(x0, p)
        assert np.all(r.status == 1) and r.kkt.max() <= 1e-8 and r.iters.max() <= 40
        rp = s.solve(x0[perm], p[perm])
        h1, h2 = s.solve(x0[:1000], p[:1000]), s.solve(x0[1000:], p[1000:])
        if hybrid == "0":
            assert np.array_equal(rp.x, r.x[perm]) and np.array_equal(rp.iters, r.iters[perm])
            assert np.array_equal(np.vstack([h1.x, h2.x]), r.x)
        else:
            assert np.abs(rp.x - r.x[perm]).max() < 1e-9 and np.array_equal(rp.iters, r.iters[perm])
            assert np.abs(np.vstack([h1.x, h2.x]) - r.x).max() < 1e-9
            assert np.array_equal(s.solve(x0, p).x, r.x)                      # the same batch again: the same bits
    o = OracleSolver(cfg)
    lbg, ubg, lbx, ubx = BicycleNLP(cfg).bounds()
    for b in range(0, B, 97):
        g = o.constraints(r.x[b], p[b])
        # IPOPT relaxes every bound by 1e-8 * max(1, |bound|) (bound_relax_factor); allow that plus round-off
        tol_g = 2e-8 * np.maximum(1.0, np.abs(np.where(np.isfinite(ubg), ubg, lbg))) + 1e-9
        assert np.all(g >= lbg - tol_g) and np.all(g <= ubg + tol_g)
        assert np.all(r.x[b] >= lbx - 1e-6) and np.all(r.x[b] <= ubx + 1e-6)
    ro = o.solve_batch(x0[::64], p[::64], nthreads=8)
    assert np.abs(r.x[::64] - ro["x"]).max() < TOL_ORACLE


def test_long_horizon_full_batch():
    """config 4 of BASELINE.json: USA_Lanker weights, N = 50, B = 4096"""
    cfg, kw = FAMILIES["usalf_n50_nx5"]
    x0, p = synthetic_batch(cfg, 4096, **kw)
    r = make_solver(cfg).solve(x0, p)
    assert np.all(r.status == 1) and r.kkt.max() <= 1e-8
    ro = OracleSolver(cfg).solve_batch(x0[::128], p[::128], nthreads=8)
    assert np.abs(r.x[::128] - ro["x"]).max() < TOL_ORACLE


def test_collision_avoidance_batch():
    """config 3 of BASELINE.json: ZAM_Over-1_1 obstacle, N = 30, B = 1024 (nonconvex: pass left/right)"""
    B = 1024
    x0, p = ca_batch(CA_CFG, B)
    s = make_solver(CA_CFG)
    set_cfg_bounds(s, CA_CFG)
    r = s.solve(x0, p)
    # every cold start comes home through the C-ABI (the stalled ones by the second chance), to the tolerance of the original NLP
    assert np.all(r.status == 1) and r.kkt.max() <= 1e-8 and s.last_rescued() > 0
    nlp = BicycleNLP(CA_CFG)
    for w in r.x[::37]:
        _, X = nlp.split(w)
        assert min(nlp.obstacle_rows(x)[0].min() for x in X) >= CA_CFG.r_sum - 1e-6
    # against the oracle: nonconvex (pass left / right), two correct solvers may end in different local optima -- where they end in the
    # same one (the large majority) they agree to 1e-6, and what the kernels return elsewhere is a KKT point by the certificate that uses
    # the numpy restatement of the NLP alone
    from helpers import kkt_certificate
    ro = OracleSolver(CA_CFG).solve_batch(x0[:64], p[:64], nthreads=8)
    both = ro["status"] == 1
    dist = np.abs(r.x[:64] - ro["x"]).max(axis=1)
    same = both & (dist < 1e-6)
    assert same.sum() >= 0.85 * both.sum()
    for b in np.nonzero(~same)[0][:4]:
        cert = kkt_certificate(nlp, r.x[b], p[b])
        assert cert["stationarity"] <= 1e-6 and cert["feasibility"] <= 1e-6, (b, cert)
    # the same obstacle handed over per instance: variant 0 of the kernels (bounds and obstacle looked up at run time) against variant 2 --
    # two instruction streams of one algorithm; bit for bit when the batch-wide solve is put on variant 0 too
    per = s.solve(x0[:32], p[:32], obst=np.tile(CA_CFG.obstacle_centers.ravel(), (32, 1)))
    assert np.all(per.status == 1) and np.max(np.abs(per.x - r.x[:32])) < 1e-6
    s.set_option("bound_mask", "0")
    assert np.array_equal(per.x, s.solve(x0[:32], p[:32]).x)


def test_second_chance_inside_the_launch_equals_the_one_behind_it():
    """k_solve_wg<.., RESC> (option rescue_wg = 2; one instance per workgroup) starts the obstacle-radius homotopy of a stalled
    instance inside the running launch; rescue_dev does the same on the host once the launch is over (sub-batch, one solve per level).
    Same schedule, same warm starts, same arithmetic: every row, status and accumulated iteration count is the same bit for bit, the same
    instances are rescued -- and the result certifies against the NLP alone"""
    from helpers import kkt_certificate
    B = 1024
    x0, p = ca_batch(CA_CFG, B)
    s = make_solver(CA_CFG)
    set_cfg_bounds(s, CA_CFG)
    assert s.get_option("rescue_wg") == 1
    # the default (1) picks by the handle's history: the first solve of a fresh handle gives its stalled instances their second chance behind the
    # launch, the next one -- the last had stalled instances -- inside it; 2 / 0 pin the choice.  All the same bits.
    first = s.solve(x0, p)
    n1 = s.last_rescued()
    second = s.solve(x0, p)
    assert s.last_rescued() == n1 and n1 > 0
    assert np.array_equal(first.x, second.x) and np.array_equal(first.iters, second.iters)
    s.set_option("rescue_wg", "2")
    a = s.solve(x0, p)
    na = s.last_rescued()
    s.set_option("rescue_wg", "0")
    b = s.solve(x0, p)
    nb = s.last_rescued()
    assert na == nb == n1 and np.all(a.status == 1)
    assert np.array_equal(a.x, b.x) and np.array_equal(a.status, b.status) and np.array_equal(a.iters, b.iters)
    assert np.array_equal(a.x, first.x) and np.array_equal(a.iters, first.iters)
    s.set_option("rescue", "0")
    plain = s.solve(x0, p)
    stalled = np.flatnonzero(plain.status != 1)
    assert len(stalled) == na
    # the wave-per-instance sweep keeps the cost-to-go of instances with heavily weighted circle rows symmetric (IS_ILL): without it the family
    # needed 25.56 iterations on average and left two instances at the limit that the lane sweep and the oracle solve in 24 (24.55 with it)
    assert plain.iters.mean() < 25.2 and int((plain.iters >= 100).sum()) <= 1
    nlp = BicycleNLP(CA_CFG)
    for i in stalled[:4]:
        cert = kkt_certificate(nlp, a.x[i], p[i])
        assert cert["stationarity"] <= 1e-6 and cert["feasibility"] <= 1e-6, (i, cert)
        assert a.iters[i] > plain.iters[i]              # (all attempts together)


@pytest.mark.parametrize("max_iter", [14, 22])
def test_second_chance_paths_agree_when_levels_fail(max_iter):
    """advisor, round 4: the cases the test above does not reach.  With a short iteration budget the first attempts of the collision-avoidance
    cold starts run out, many instances need the SECOND pass of the schedule and some fail every level.  k_solve_wg<.., RESC> must then
    report what rescue_dev reports: an instance brought in by pass 2 counts its first attempt and the levels of pass 2 (not those of the
    pass that ended open), and an instance no level brings in goes back as its first attempt left it -- row, status, iterations, KKT error."""
    B = 512
    x0, p = ca_batch(CA_CFG, B)
    s = make_solver(CA_CFG, max_iter=max_iter)
    set_cfg_bounds(s, CA_CFG)
    s.set_option("rescue_wg", "2")
    a = s.solve(x0, p)
    na = s.last_rescued()
    s.set_option("rescue_wg", "0")
    b = s.solve(x0, p)
    nb = s.last_rescued()
    s.set_option("rescue", "0")
    plain = s.solve(x0, p)
    assert na == nb == int((plain.status != 1).sum()) and na > 0
    assert np.array_equal(a.status, b.status) and np.array_equal(a.iters, b.iters)
    assert np.array_equal(a.x, b.x) and np.array_equal(a.kkt, b.kkt)
    lost = np.flatnonzero(a.status != 1)                      # no level converged: the first attempt's row comes back
    assert np.array_equal(a.x[lost], plain.x[lost]) and np.array_equal(a.iters[lost], plain.iters[lost]) and np.array_equal(a.kkt[lost], plain.kkt[lost])
    assert np.array_equal(a.status[lost], plain.status[lost])
    won = np.flatnonzero((a.status == 1) & (plain.status != 1))
    # pass 1 = two levels, pass 2 = five, every level at least one iteration: instances beyond the budget of pass 1 were brought in by pass 2
    by_pass2 = won[a.iters[won] - plain.iters[won] > 2 * max_iter]
    if max_iter == 14:
        assert len(lost) > 0 and len(by_pass2) > 0, (len(lost), len(won), len(by_pass2))


def test_second_chance_behind_the_pipeline_with_one_instance_per_wavefront():
    """advisor, round 5: the configuration the two tests above do not reach -- collision avoidance at B = 4096 with one instance per wavefront of
    k_solve_wg (hybrid_bx = 1): the pipeline runs first, k_solve_wg<.., RESC> takes its instances from the hand-over lists, so the instance of a
    workgroup is a LIST ENTRY, not #blockIdx.x (the second chance once restarted the wrong instance), and an instance that stalls INSIDE the pipeline
    is on no list: it must still get its levels (rescue_dev, behind the launch).  Against the host-side second chance alone (rescue_wg = 0): every
    instance converges either way, the same instances are rescued, rows agree to the hybrid solve's round-off (the KKT solver that serves an
    iteration differs between the two), and the rescued rows certify against the NLP alone."""
    from helpers import kkt_certificate
    B = 4096
    x0, p = ca_batch(CA_CFG, B)
    s = make_solver(CA_CFG)
    set_cfg_bounds(s, CA_CFG)
    s.set_option("hybrid_bx", "1")
    s.set_option("rescue_wg", "2")
    a = s.solve(x0, p)
    na = s.last_rescued()
    assert s.get_pipeline_profile()["ran"] and s.get_resident_profile()["ran"]
    s.set_option("rescue_wg", "0")
    b = s.solve(x0, p)
    nb = s.last_rescued()
    assert s.get_pipeline_profile()["ran"] and s.get_resident_profile()["ran"]
    s.set_option("rescue", "0")
    plain = s.solve(x0, p)
    stalled = np.flatnonzero(plain.status != 1)
    assert len(stalled) > 0 and na == nb == len(stalled)
    assert np.all(a.status == 1) and np.all(b.status == 1)
    same_basin = np.abs(a.x - b.x).max(axis=1) < 1e-6
    assert same_basin.mean() > 0.99 and np.all(same_basin[plain.status == 1])
    nlp = BicycleNLP(CA_CFG)
    for i in stalled[:6]:
        cert = kkt_certificate(nlp, a.x[i], p[i])
        assert cert["stationarity"] <= 1e-6 and cert["feasibility"] <= 1e-6, (i, cert)
        assert a.iters[i] > plain.iters[i]


@pytest.mark.parametrize("B", [1024, 4096])
def test_getters_describe_the_main_solve_after_a_second_chance(B):
    """The levels of the host-side second chance (rescue_dev) are solves of their own; what the handle reports afterwards -- iterations, the
    pipeline's profile -- is still the main solve's.  Collision avoidance on two fresh handles, one without the second chance: B = 1024 is
    k_solve_wg alone, B = 4096 the pipeline with k_solve_wg behind it.  The rows of the instances that needed no second chance are the same
    bits."""
    x0, p = ca_batch(CA_CFG, B)
    plain_s, s = make_solver(CA_CFG), make_solver(CA_CFG)
    for h in (plain_s, s):
        set_cfg_bounds(h, CA_CFG)
    plain_s.set_option("rescue", "0")
    plain = plain_s.solve(x0, p)
    r = s.solve(x0, p)
    pp0, pp = plain_s.get_pipeline_profile(), s.get_pipeline_profile()
    print(B, "rescued", s.last_rescued(), plain_s.get_profile(), s.get_profile(), pp0, pp)
    assert pp0["ran"] == (B == 4096)
    assert plain_s.last_rescued() == 0 and s.last_rescued() > 0
    assert s.get_profile()["iterations"] == plain_s.get_profile()["iterations"]
    assert pp["ran"] == pp0["ran"] and pp["rounds"] == pp0["rounds"]
    home = plain.status == 1
    assert home.sum() < B and np.array_equal(r.x[home], plain.x[home]) and np.array_equal(r.iters[home], plain.iters[home])


def test_fixed_iteration_mode_matches_converged():
    cfg, kw = FAMILIES["zamlf_n30_nx6"]
    x0, p = synthetic_batch(cfg, 512, **kw)
    rf = make_solver(cfg, fixed_iters=20).solve(x0, p)
    rc = make_solver(cfg).solve(x0, p)
    assert np.all(rf.iters == 20) and np.all(rf.status == 1)
    assert np.abs(rf.x - rc.x).max() < 1e-5


def test_trace_matches_oracle():
    cfg, kw = FAMILIES["zamlf_n30_nx5"]
    x0, p = synthetic_batch(cfg, 8, **kw)
    r, tr = make_solver(cfg).solve_trace(x0, p)
    for b in range(8):
        ro = OracleSolver(cfg).solve(x0[b], p[b], trace=True)
        n = ro["iters"]
        assert np.allclose(tr[:n, 3, b], ro["trace"][:n, 3], rtol=1e-9, atol=1e-12)      # primal step lengths
        assert np.allclose(tr[:n - 1, 0, b], ro["trace"][1:n, 0], rtol=1e-12)          # barrier parameter (row it = mu of it+1)


def test_bounds_errors_and_last_error():
    cfg = NLPConfig(N=10, nx=5)
    s = make_solver(cfg)
    lbg, ubg, lbx, ubx = BicycleNLP(cfg).bounds()
    bad = ubg.copy()
    bad[3] = 1.0
    with pytest.raises(pkg.MpcError) as e:
        s.set_bounds(lbx, ubx, lbg, bad)
    assert e.value.code == abi.MPC_ERR_BOUNDS and "equality" in str(e.value)
    with pytest.raises(pkg.MpcError):
        pkg.BatchedMPCSolver(0)
    with pytest.raises(pkg.MpcError):
        pkg.BatchedMPCSolver(10, nx=7)


def test_plant_step_kat(golden_dir):
    """device plant step vs the reference's recorded rows (libm vs device sin/cos/tan: 1e-12, not bit-exact)"""
    kat = np.load(os.path.join(golden_dir, "plant_step_kat.npz"))
    s = pkg.BatchedMPCSolver(10, 5)
    for run in sorted({k.rsplit("__", 1)[0] for k in kat.files}):
        xs, us = kat[f"{run}__x"], kat[f"{run}__u"]
        xn = s.plant_step(xs[:-1], us[:-1], "euler" if run.startswith("casadi") else "rk4")
        assert np.abs(xn - xs[1:]).max() < 1e-12


def test_casadi_optimizer_closed_loop_on_gpu():
    """the reference's caller path (mpc_planner.py:301-309): CasadiOptimizer(...).optimize(), 30 steps, N = 10,
    incl. the transposed step-0 warm start (App. C-6); compared with the same loop on the oracle stand-in."""
    path, orient = straight_path(30, 29.9948, -1.1501, 0.03495, 20.0)
    conf = make_configuration(path, orient, 20.0, WEIGHTS_YAML_ZAM_LF)
    init_values = (np.array([29.9948, -1.1501]), 20.0, 0.0, 0.03495)
    og = opt.CasadiOptimizer(configuration=conf, init_values=init_values, predict_horizon=10)
    xs, us, tv = og.optimize()
    oc = opt.CasadiOptimizer(configuration=conf, init_values=init_values, predict_horizon=10)
    oc._sol = opt.NlpSolverHandle(OracleBackend(NLPConfig(N=10, nx=5)))
    xo, uo, _ = oc.optimize()
    assert xs.shape == (30, 5) and us.shape == (30, 2) and tv.shape == (30,)
    assert abs(us[0, 1] + np.sqrt(11.5)) < 1e-5
    assert np.abs(xs - xo).max() < 1e-6 and np.abs(us - uo).max() < 1e-6
    assert og.solver()[0].stats()["success"]


def test_device_closed_loop_matches_host_loop():
    """row f1: mpc_closed_loop_batch (all steps on the device) against the step-by-step host loop of the optimizer.py
    mirror, both with GPU solves; plus a batch of shifted egos through the same driver."""
    N, L = 10, 30
    path, orient = straight_path(L, 29.9948, -1.1501, 0.03495, 20.0)
    conf = make_configuration(path, orient, 20.0, WEIGHTS_YAML_ZAM_LF)
    init_values = (np.array([29.9948, -1.1501]), 20.0, 0.0, 0.03495)
    host = opt.CasadiOptimizer(configuration=conf, init_values=init_values, predict_horizon=N)
    host.use_device_loop = False
    hs, hc, _ = host.optimize()
    dev = opt.CasadiOptimizer(configuration=conf, init_values=init_values, predict_horizon=N)
    ds, dc, dt_ = dev.optimize()
    assert ds.shape == (L, 5) and dc.shape == (L, 2) and dt_.shape == (L,)
    assert np.abs(ds - hs).max() < 1e-7 and np.abs(dc - hc).max() < 1e-7
    assert abs(dc[0, 1] + np.sqrt(11.5)) < 1e-5                      # step 0 brakes at the friction cap
    # a batch of egos with lateral / speed offsets through the same path: all steps converge, all merge onto the path
    sol, _ = dev.solver()
    be = sol._backend
    B = 96
    rng = np.random.default_rng(3)
    init = np.tile([29.9948, -1.1501, 0.0, 20.0, 0.03495], (B, 1))
    init[:, 1] += rng.uniform(-0.5, 0.5, B)
    init[:, 3] *= rng.uniform(0.9, 1.1, B)
    traj, ctrl, st = be.closed_loop(init, np.tile(path, (B, 1, 1)), np.tile(orient, (B, 1)), np.full(B, 20.0), L)
    assert np.all(st == 1)
    lateral = (traj[:, -1, 1] - path[-1, 1]) * np.cos(0.03495) - (traj[:, -1, 0] - path[-1, 0]) * np.sin(0.03495)
    assert np.abs(lateral).max() < 0.3
    l = 2.5789128
    x, u = traj[:, :-1], ctrl[:, :-1]
    xn = x + 0.1 * np.stack([x[..., 3] * np.cos(x[..., 4]), x[..., 3] * np.sin(x[..., 4]), u[..., 0], u[..., 1], x[..., 3] / l * np.tan(x[..., 2])], -1)
    assert np.abs(traj[:, 1:] - xn).max() < 1e-12


def test_raw_c_abi_brings_every_collision_avoidance_cold_start_home():
    """BASELINE config 3 (ZAM_Over-1_1 collision avoidance, cold starts through the obstacle): ~1.4 % of the instances stall
    where IPOPT would enter its restoration phase.  The second chance (homotopy on the circle radius) runs on the device BEHIND
    the C-ABI: a plain mpc_solve_batch / mpc_solve_batch_dev call returns every instance at a KKT point of the ORIGINAL problem."""
    import torch
    from helpers import kkt_certificate
    x0, p = ca_batch(CA_CFG, 1024)
    s = make_solver(CA_CFG)
    set_cfg_bounds(s, CA_CFG)
    res = s.solve(x0, p)                                 # raw mpc_solve_batch
    n = s.last_rescued()
    assert np.all(res.status == 1) and res.kkt.max() <= 1e-8 and 0 < n < 0.03 * 1024
    s.set_option("rescue", "0")
    plain = s.solve(x0, p)
    s.set_option("rescue", None)
    rescued = plain.status != 1
    assert rescued.sum() == n and s.last_rescued() == 0
    assert np.array_equal(res.x[~rescued], plain.x[~rescued]) and np.array_equal(res.iters[~rescued], plain.iters[~rescued])
    assert np.all(res.iters[rescued] > plain.iters[rescued])            # iterations of the second chance are counted
    nlp = BicycleNLP(CA_CFG)
    for b in np.nonzero(rescued)[0]:
        c = kkt_certificate(nlp, res.x[b], p[b])
        assert c["stationarity"] < 1e-7 and c["feasibility"] < 1e-6, (b, c)
    # device-pointer entry point, status row not requested: same rows
    d = [torch.from_numpy(a).cuda() for a in (x0, p)]
    out = torch.empty_like(d[0])
    s.solve_device(1024, d[0].data_ptr(), d[1].data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), res.x) and s.last_rescued() == n
    res2, mask = s.solve_with_rescue(x0, p)
    assert np.array_equal(mask, rescued) and np.array_equal(res2.x, res.x)


@pytest.mark.parametrize("N", [1, 2, 3, 20, 23, 31, 32, 63, 64, 127])
def test_extreme_horizons_match_oracle(N):
    """shortest horizons, the largest one the C-ABI accepts (N <= 127: 512-thread stage workgroups, bx = 4) and the
    boundaries of the workgroup shapes in between (N = 23: 192-thread pipeline workgroups; 31 | 32: 8 | 4 instances per
    256-thread workgroup; 63 | 64: 256 | 512 threads): same iterates as the oracle"""
    cfg = NLPConfig(N=N, nx=5)
    B = 40 if N < 100 else 24
    x0, p = synthetic_batch(cfg, B)
    s = make_solver(cfg)
    set_cfg_bounds(s, cfg)
    s.set_option("rescue", "0")                             # the oracle has no second chance: compare the first solve
    r = s.solve(x0, p)
    ro = OracleSolver(cfg).solve_batch(x0, p, nthreads=8)
    assert np.array_equal(r.status, ro["status"]) and np.array_equal(r.iters, ro["iters"])
    ok = r.status == 1
    assert ok.mean() > 0.8 and np.abs(r.x[ok] - ro["x"][ok]).max() < TOL_ORACLE          # (at N = 127 a few of the 12.7 s synthetic problems stall, in the oracle too)


def test_bad_inputs_are_contained_and_reported():
    """NaN / Inf in one instance's inputs: that instance reports -6 (BADFUNCEVAL, FORCESNLPsolver.h:68-106 convention) and its
    neighbours in the same workgroup and tile are bit-identical to a clean run; argument errors come back as error codes."""
    cfg, kw = FAMILIES["zamlf_n30_nx6"]
    x0, p = synthetic_batch(cfg, 130, **kw)
    s = make_solver(cfg)
    clean = s.solve(x0, p)
    bad_x0, bad_p = x0.copy(), p.copy()
    bad_x0[9, 2 * cfg.N + 3] = np.nan            # a NaN in the STATE guess is survivable: the start-point safeguard rolls the controls out
    bad_p[5, 2 * cfg.N + cfg.nx + 1] = np.nan    # reference entries are not
    bad_p[70, 2 * cfg.N + 2 * cfg.nx] = np.inf
    r = s.solve(bad_x0, bad_p)
    assert r.status[5] == -6 and r.status[70] == -6 and r.status[9] == 1
    assert np.abs(r.x[9] - clean.x[9]).max() < 1e-6
    keep = np.ones(130, bool)
    keep[[5, 9, 70]] = False
    assert np.array_equal(r.x[keep], clean.x[keep]) and np.array_equal(r.status[keep], clean.status[keep])
    with pytest.raises(pkg.MpcError) as e:
        s.solve(x0[:, :-1], p[:, :-1])
    assert e.value.code == abi.MPC_ERR_INVALID
    L = abi.load_library()
    h = s._h
    assert L.mpc_solve_batch(h, 0, abi.as_dp(x0), abi.as_dp(p), None, abi.as_dp(np.empty_like(x0)), None, None, None) == abi.MPC_ERR_INVALID
    assert L.mpc_solve_batch(h, 4, None, abi.as_dp(p), None, abi.as_dp(np.empty_like(x0)), None, None, None) == abi.MPC_ERR_INVALID
    assert b"required" in L.mpc_last_error(h)
    assert s.last_rescued() == 0                       # NaN instances are not handed to the second chance
    with pytest.raises(pkg.MpcError):
        s.set_option("no_such_switch", "1")
    s.set_option("pipeline", None)


def test_mixed_sweep_shard_matches_oracle():
    """BASELINE configuration 5, one shard on one GPU: 4096 rows dealt over the four problem families (tools/workloads.py), one
    handle per family; a sample of every family is checked against the oracle, every converged row against its own constraints"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import workloads as wl
    shard = wl.mixed_shard(0, 8)
    assert sum(len(v[0]) for v in shard.values()) == wl.MIXED_SHARD
    for name, (rows, x0, p) in shard.items():
        fam = wl.FAMILIES[name]
        cfg = NLPConfig(N=fam.N, nx=fam.nx, dt=fam.dt, Q=fam.Q, R=fam.R, obstacle=fam.obstacle)
        s = wl.make_solver(fam)
        r = s.solve(x0, p)
        ok = r.status == 1
        assert ok.all(), (name, ok.mean())                  # (the collision-avoidance cold starts included: second chance behind the C-ABI)
        sel = np.arange(0, len(rows), max(1, len(rows) // 48))[:48]
        ro = OracleSolver(cfg).solve_batch(x0[sel], p[sel], nthreads=8)
        both = ok[sel] & (ro["status"] == 1)
        assert both.mean() >= 0.95
        if fam.kind == "ca":                                 # nonconvex: the same local optimum for the large majority
            assert np.mean(np.abs(r.x[sel][both] - ro["x"][both]).max(axis=1) < 1e-6) >= 0.85
        else:
            assert np.abs(r.x[sel][both] - ro["x"][both]).max() < TOL_ORACLE, name
        nlp = BicycleNLP(cfg)
        lbg, ubg, lbx, ubx = nlp.bounds()
        for b in np.nonzero(ok)[0][:: max(1, int(ok.sum()) // 64)]:
            g = nlp.g(r.x[b], p[b])
            assert np.all(g >= lbg - 1e-6) and np.all(g <= ubg + 1e-6) and np.all(r.x[b] >= lbx - 1e-7) and np.all(r.x[b] <= ubx + 1e-7)


def test_mixed_sweep_every_shard_maps_rows_to_families():
    """shards 1..7 of BASELINE configuration 5 (an 8-GPU run solves them on ranks 1..7; one GPU here): the rows a rank would solve,
    with the handle of the family the generator assigns them to, against per-row oracle solves of the GLOBAL row index -- the
    generator + family mapping of every shard, not only shard 0"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import workloads as wl
    solvers = {name: wl.make_solver(wl.FAMILIES[name]) for name in wl.MIXED_ORDER}
    for rank in range(1, 8):
        shard = wl.mixed_shard(rank, 8)
        lo = rank * wl.MIXED_SHARD
        for i, name in enumerate(wl.MIXED_ORDER):
            rows, x0, p = shard[name]
            assert rows[0] >= lo and rows[-1] < lo + wl.MIXED_SHARD and np.all(rows % len(wl.MIXED_ORDER) == i)
            fam = wl.FAMILIES[name]
            sel = np.arange(0, len(rows), len(rows) // 6)[:6]
            r = solvers[name].solve(x0[sel], p[sel])
            cfg = NLPConfig(N=fam.N, nx=fam.nx, dt=fam.dt, Q=fam.Q, R=fam.R, obstacle=fam.obstacle)
            for j, g in enumerate(rows[sel]):
                xg, pg = wl.instance(fam, int(g))                         # the row by its GLOBAL index
                assert np.array_equal(xg, x0[sel][j]) and np.array_equal(pg, p[sel][j])
            ro = OracleSolver(cfg).solve_batch(x0[sel], p[sel], nthreads=6)
            both = (r.status == 1) & (ro["status"] == 1)
            assert both.mean() >= 0.8, (rank, name)
            d = np.abs(r.x[both] - ro["x"][both]).max(axis=1)
            assert (np.mean(d < 1e-6) >= 0.8) if fam.kind == "ca" else (d.max() < TOL_ORACLE), (rank, name, d)


def test_gpu_replays_the_dense_ipm_closed_loop_triplets(golden_dir):
    """BASELINE configuration 1 (N = 30, L = 30, window frozen from step 0): the (p, x0) of every step of the closed loop that
    the LITERAL dense IPM drove (tests/golden/make_closed_loop_golden.py) solved on the GPU -> its x*; and the whole loop through
    the product path (scenario XML -> configuration -> CasadiOptimizer.optimize, device-side driver) -> its states / controls.
    Tolerance: north_star's 1e-4 on trajectories; most rows agree to 1e-6 (see tests/test_parity_pins.py)."""
    from test_parity_pins import TOL_TRAJ, config1_optimizer
    g = np.load(os.path.join(golden_dir, "closed_loop_n30.npz"))
    cfg = NLPConfig(N=30, nx=5)
    s = make_solver(cfg)
    set_cfg_bounds(s, cfg)
    r = s.solve(g["x0"], g["p"])
    assert np.all(r.status == 1)
    err = np.abs(r.x - g["w"]).max(axis=1)
    assert err.max() < TOL_TRAJ and np.mean(err < 1e-6) >= 0.8, err
    o, conf = config1_optimizer()
    states, controls, _ = o.optimize()                     # mpc_closed_loop_batch on the device
    assert o._sol.stats()["success"]
    assert np.abs(states - g["states"]).max() < TOL_TRAJ and np.abs(controls - g["controls"]).max() < TOL_TRAJ
    o2, _ = config1_optimizer()
    o2.use_device_loop = False                             # the step-by-step host loop over mpc_solve_batch
    s2, c2, _ = o2.optimize()
    assert np.abs(s2 - g["states"]).max() < TOL_TRAJ and np.abs(c2 - g["controls"]).max() < TOL_TRAJ


def test_pipeline_survives_copy_kernels_of_another_stream():
    """multi-GPU readiness on a one-GPU box: with `--gather overlap` RCCL's copy kernels of the 8.1 MB packed block run
    on a stream of their own WHILE the next solve's persistent k_pipeline owns every CU.  Here a second stream is kept busy with copy kernels
    of that size for the whole duration of the solves: the pipeline's workgroups then arrive late / share their CUs, the roles are dealt by
    arrival order and the waits are bounded -- the launch must neither be abandoned nor restarted, and the rows must be the bits of the solve
    without company.  Prints the slowdown (not asserted: it is the price of the overlap, measured)."""
    import time
    import torch
    cfg, kw = FAMILIES["zamlf_n30_nx6"]
    B = 4096
    x0, p = synthetic_batch(cfg, B, **kw)
    s = make_solver(cfg)
    d = [torch.from_numpy(a).cuda() for a in (x0, p)]
    out = torch.empty_like(d[0]); st = torch.empty(B, dtype=torch.int32, device="cuda"); it = torch.empty_like(st)

    def step():
        s.solve_device(B, d[0].data_ptr(), d[1].data_ptr(), out.data_ptr(), st.data_ptr(), it.data_ptr())
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        step()
    t_solo = (time.perf_counter() - t0) / 10
    assert s.get_pipeline_profile()["ran"] and s.get_resident_profile()["ran"]
    ref, ref_it = out.cpu().numpy().copy(), it.cpu().numpy().copy()
    n_el = (B * (x0.shape[1] + 2))                                       # the packed block of sharding.pack_rows: rows + status + iterations
    src = torch.randn(n_el, dtype=torch.float64, device="cuda"); dst = torch.empty_like(src)
    side = torch.cuda.Stream()
    import threading
    t_busy, bad, done = [], [], threading.Event()

    def solves():                                                        # (ctypes releases the GIL inside the call: the copies below are issued meanwhile)
        try:
            for rep in range(24):
                t0 = time.perf_counter()
                step()
                t_busy.append(time.perf_counter() - t0)
                if not (s.get_pipeline_profile()["ran"] and s.get_resident_profile()["ran"]):
                    bad.append(("fallback", rep))                       # abandoned launch / one launch per kernel
                if not (np.array_equal(out.cpu().numpy(), ref) and np.array_equal(it.cpu().numpy(), ref_it)):
                    bad.append(("bits", rep))
        finally:
            done.set()
    th = threading.Thread(target=solves)
    n_copies = 0
    with torch.cuda.stream(side):
        th.start()
        while not done.is_set():                                           # an 8.1 MB copy kernel every few tens of microseconds for as long as the solves run
            dst.copy_(src, non_blocking=True)
            n_copies += 1
            if n_copies % 64 == 0:
                side.synchronize()                                          # (bounds the queue: the copies stay BESIDE the solves, not ahead of them)
    th.join()
    torch.cuda.synchronize()
    assert not bad, bad
    assert torch.equal(dst, src) and n_copies >= 100
    print(f"\n[copy kernels beside the pipeline] solve alone {t_solo * 1e3:.3f} ms, with {n_copies} 8.1 MB copy kernels of another stream beside {len(t_busy)} solves "
          f"{np.median(t_busy) * 1e3:.3f} ms (x{np.median(t_busy) / t_solo:.2f}, slowest {max(t_busy) * 1e3:.3f} ms); pipeline ran every time, rows bit-identical")


def test_option_rescue_alone_for_families_that_stall():
    """collision-avoidance cold starts beyond the machine's wavefront slots (B = 3000): by default the pipeline takes the batch and the stalled
    instances get their levels behind the launch; option rescue_alone = 1 keeps the whole batch in k_solve_wg, one instance per wavefront, the
    second chance inside -- every instance converged on both, the same instances rescued, rows to 1e-4 (other sweeps serve the iterations:
    ill-conditioned rows differ in the last digits), the KKT error within the tolerance, the same bits from call to call."""
    B = 3000
    x0, p = ca_batch(CA_CFG, B)
    s = make_solver(CA_CFG)
    set_cfg_bounds(s, CA_CFG)
    ra = s.solve(x0, p)
    na = s.last_rescued()
    assert s.get_pipeline_profile()["ran"] and np.all(ra.status == 1) and na > 20
    s.set_option("rescue_alone", "1")
    rb = s.solve(x0, p)
    nb = s.last_rescued()
    rc = s.solve(x0, p)
    assert not s.get_pipeline_profile()["ran"] and s.get_resident_profile()["ran"]
    assert np.all(rb.status == 1) and rb.kkt.max() <= 1e-8 and nb == na
    assert np.array_equal(rb.x, rc.x) and np.array_equal(rb.iters, rc.iters)
    d = np.abs(ra.x - rb.x).max(axis=1)
    assert (d > 1e-2).sum() <= 3 and d[d <= 1e-2].max() < 1e-4            # (an instance or two may pass the obstacle on the other side)


def test_second_chance_paths_agree_when_thousands_of_instances_stall():
    """found by tools/fuzz_sizes.py: with an iteration limit of 6 three quarters of a lane-following batch stop unconverged and take the second
    chance (the dummy obstacle gives them the levels) -- behind the pipeline at N = 50 some inside the stragglers' launch, most behind it.  The
    sub-batch of rescue_dev used to go through the pipeline when it was larger than the machine holds one instance per wavefront, whose sweeps
    round differently from k_solve_wg's: the two paths then differed in the last bits (1e-15) of the instances rescued inside the launch, and so
    did two consecutive solves of a handle (option rescue_wg = 1 picks by history).  The levels now always run on k_solve_wg alone, one instance
    per wavefront: rows, statuses and iteration counts are the same bits on rescue_wg = 0 / 2 and from call to call."""
    cfg, kw = FAMILIES["usalf_n50_nx5"]
    x0, p = synthetic_batch(cfg, 2724, **kw)
    res = {}
    for rw in ("0", "2", "1"):
        s = make_solver(cfg, max_iter=6)
        s.set_option("rescue_wg", rw)
        r1 = s.solve(x0, p)
        n1 = s.last_rescued()
        r2 = s.solve(x0, p)
        assert s.get_pipeline_profile()["ran"] and s.get_resident_profile()["ran"] and n1 > 1500
        assert np.array_equal(r1.x, r2.x) and np.array_equal(r1.status, r2.status) and np.array_equal(r1.iters, r2.iters), rw
        res[rw] = r2
    for rw in ("2", "1"):
        assert np.array_equal(res["0"].x, res[rw].x) and np.array_equal(res["0"].status, res[rw].status) and np.array_equal(res["0"].iters, res[rw].iters), rw
    assert 0.3 < (res["0"].status == 1).mean() < 0.9                  # (what converges within six iterations per attempt and level)


def test_status_iters_and_kkt_buffers_may_be_null():
    """include/mpcgpu.h: "status/iters/kkt: [B], any may be NULL" -- the loop kernels write the caller's rows themselves (Params::emit), so the
    optional outputs are tested where they are written; the second chance needs the statuses and keeps an internal row then.  Rows with and
    without the optional buffers: the same bits, on the pipeline + stragglers, on the stragglers' kernel alone and on collision avoidance."""
    import torch
    cases = [(FAMILIES["zamlf_n30_nx6"][0], synthetic_batch(FAMILIES["zamlf_n30_nx6"][0], 4096), False),
             (FAMILIES["usalf_n50_nx5"][0], synthetic_batch(FAMILIES["usalf_n50_nx5"][0], 300, **FAMILIES["usalf_n50_nx5"][1]), False),
             (CA_CFG, ca_batch(CA_CFG, 600), True)]
    for cfg, (x0, p), ca in cases:
        s = make_solver(cfg)
        if ca:
            set_cfg_bounds(s, cfg)
        B = x0.shape[0]
        d0, d1 = torch.from_numpy(x0).cuda(), torch.from_numpy(p).cuda()
        o1, o2 = torch.zeros_like(d0), torch.zeros_like(d0)
        st = torch.zeros(B, dtype=torch.int32, device="cuda")
        for _ in range(2):                                   # (collision avoidance: the second call has the second chance inside the launch)
            s.solve_device(B, d0.data_ptr(), d1.data_ptr(), o1.data_ptr(), st.data_ptr())
            n1 = s.last_rescued()
            s.solve_device(B, d0.data_ptr(), d1.data_ptr(), o2.data_ptr())
            torch.cuda.synchronize()
            assert torch.equal(o1, o2) and bool((st == 1).all()) and s.last_rescued() == n1 and (n1 > 0) == ca


def test_rccl_all_gather_of_the_packed_block_beside_the_pipeline():
    """the same question with RCCL's OWN kernel (the stand-in above uses torch's copy kernels): `MPC_BENCH_FORCE_GATHER=1` sends a single rank
    of bench.py through the collective code of the multi-GPU path -- an `all_gather_into_tensor` of the 8.1 MB packed block on RCCL's stream
    under the next solve's persistent launch (`--gather overlap`) and inside the step (`--gather sync`).  No launch may be abandoned, the
    block that arrives must be the rank's own rows, statuses and iteration counts, and every instance converges as without the collective.
    (A group of one moves the block with a copy kernel of RCCL's, not over xGMI: what is exercised is the stream / buffer / wait logic of
    the step and RCCL's workgroups beside the pipeline's, not the links.)"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for mode in ("overlap", "sync"):
        env = dict(os.environ, MPC_BENCH_FORCE_GATHER="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29610 + (mode == "sync")))
        for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
            env.pop(k, None)
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--full", "--headline-only", "--no-cpu-baseline", "--no-traffic", "--steps", "12",
                            "--warmup", "2", "--gather", mode], env=env, capture_output=True, text=True, timeout=600, cwd=root)
        assert r.returncode == 0, r.stderr[-3000:]
        line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        g = line["gather"]
        assert g["mode"] == mode and g["own_rows_round_trip"] is True and g["pipeline_abandoned"] is False, g
        assert g["bytes_per_rank"] == 4096 * (2 * 30 + 6 * 31 + 2) * 8              # rows + status + iterations: 8.13 MB
        assert line["converged_frac"] == 1.0 and line["value"] > 1e6
        assert "bounded wait expired" not in r.stderr and "abandon" not in r.stderr.lower().replace("pipeline_abandoned", "")
        print(f"\n[RCCL all-gather of one rank, --gather {mode}] {line['ms_per_step']:.3f} ms per step, the collective alone {g['gather_ms_alone']:.3f} ms, "
              f"waited inside a step {g['wait_ms_in_step']}")


@pytest.mark.parametrize("friction_lb", ["ipopt", "nlp"])
def test_gpu_replays_the_friction_row_fixture(golden_dir, friction_lb):
    """the loop that visits the kink of the reference's stage-0 friction row (tests/test_parity_pins.py, closed_loop_n30_friction.npz: N = 30, no
    noise, answers of the dense IPM with the LITERAL row): the kernels with the row as IPOPT sees it (`friction_lb = ipopt`) and with the
    default reading reproduce every triplet to north_star's 1e-4 (1e-5 in fact)"""
    g = np.load(os.path.join(golden_dir, "closed_loop_n30_friction.npz"))
    cfg = NLPConfig(N=30, nx=5)
    s = make_solver(cfg)
    set_cfg_bounds(s, cfg)
    s.set_option("friction_lb", friction_lb)
    r = s.solve(g["x0"], g["p"])
    assert np.all(r.status == 1)
    err = np.abs(r.x - g["w"]).max(axis=1)
    assert err.max() < 1e-5 and np.mean(err < 1e-6) >= 0.9, err


@pytest.mark.parametrize("fam", ["zamlf_n30_nx6", "usalf_n50_nx5", "zamca_n30_nx5"])
def test_kkt_certificate_of_gpu_solutions(fam):
    """acceptance that does not rest on the sibling interior-point implementations: stationarity / feasibility of the KERNELS'
    answers evaluated with the numpy restatement of the NLP alone (multipliers by sign-constrained least squares)"""
    from helpers import kkt_certificate
    if fam == "zamca_n30_nx5":
        cfg, (x0, p) = CA_CFG, ca_batch(CA_CFG, 256)
    else:
        cfg, kw = FAMILIES[fam]
        x0, p = synthetic_batch(cfg, 256, **kw)
    s = make_solver(cfg)
    set_cfg_bounds(s, cfg)
    r = s.solve(x0, p)
    assert np.all(r.status == 1)
    nlp = BicycleNLP(cfg)
    worst = 0.0
    for b in range(0, 256, 8):
        c = kkt_certificate(nlp, r.x[b], p[b])
        worst = max(worst, c["stationarity"])
        assert c["stationarity"] < 1e-7 and c["feasibility"] < 1e-6, (fam, b, c)
    print(fam, "worst relative stationarity residual of 32 GPU solutions:", worst)


def _loop_inputs(B, L, v=15.0, psi=0.1, seed=0):
    k = np.arange(L)
    path = np.stack([k * v * 0.1 * np.cos(psi), k * v * 0.1 * np.sin(psi)], axis=1)
    rng = np.random.default_rng(seed)
    init = np.tile([0.0, 0.0, 0.0, v, psi], (B, 1))
    init[:, 1] += rng.uniform(-0.5, 0.5, B)
    init[:, 3] *= rng.uniform(0.9, 1.1, B)
    return init, np.tile(path, (B, 1, 1)), np.full((B, L), psi), np.full(B, v)


@pytest.mark.parametrize("N", [10, 30])
def test_seeded_noise_device_loop_matches_host_loop(N):
    """`noised: True` (optimizer.py:611-617) with the counter-based samples: the device-side driver (mpc_closed_loop_batch_ex,
    noise generated in k_loop_advance) against the step-by-step host loop of the Python mirror drawing from noise.py"""
    path, orient = straight_path(30, 29.9948, -1.1501, 0.03495, 20.0)
    outs = []
    for device_loop in (True, False):
        conf = make_configuration(path, orient, 20.0, WEIGHTS_YAML_ZAM_LF, noised=True)
        conf.noise_seed = 77
        o = opt.CasadiOptimizer(configuration=conf, init_values=(np.array([29.9948, -1.1501]), 20.0, 0.0, 0.03495), predict_horizon=N)
        o.use_device_loop = device_loop
        outs.append(o.optimize())
    assert np.abs(outs[0][0] - outs[1][0]).max() < 1e-6 and np.abs(outs[0][1] - outs[1][1]).max() < 1e-6
    conf = make_configuration(path, orient, 20.0, WEIGHTS_YAML_ZAM_LF, noised=False)
    clean = opt.CasadiOptimizer(configuration=conf, init_values=(np.array([29.9948, -1.1501]), 20.0, 0.0, 0.03495), predict_horizon=N).optimize()
    nz = __import__("importlib").import_module("motion-planning-for-autonomous-driving-with-mpc_amd.noise")
    assert np.abs(outs[0][1][0] - clean[1][0] - nz.sequence_noise(77, 0, 0, N, 0.1)[:, 0]).max() < 1e-9      # step 0: same solve, noised first column applied


def test_closed_loop_whose_pipeline_launch_is_abandoned_is_replayed():
    """the asynchronous closed loop looks at the device's abort word once, at the end: a launch abandoned on the way (option pipe_test_abort)
    makes the bookkeeping kernels behind it do nothing and the host replay the loop step by step on one launch per kernel -- the same
    trajectories as the undisturbed loop to the difference between the two paths' arithmetic; one such incident does not take the pipeline
    away from the handle (three do, tests above)"""
    B, L, N = 3000, 32, 30                                   # (a batch the pipeline serves: 47 tiles)
    init, path, orient, vdes = _loop_inputs(B, L + N)
    s = pkg.BatchedMPCSolver(N, 5)
    s.set_bounds()
    t0, c0, st0 = s.closed_loop(init, path, orient, vdes, L)
    assert not s.last_loop_replayed() and np.all(st0 == 1)
    s.set_option("pipe_test_abort", "1")
    t1, c1, st1 = s.closed_loop(init, path, orient, vdes, L)
    assert s.last_loop_replayed() and s.get_option("pipe_aborts") == 1 and s.get_option("pipe_disabled") == 0
    assert np.array_equal(st1, st0) and np.abs(t1 - t0).max() < 1e-9 and np.abs(c1 - c0).max() < 1e-9
    s.set_option("pipe_test_abort", None)
    t2, c2, st2 = s.closed_loop(init, path, orient, vdes, L)
    assert not s.last_loop_replayed() and np.array_equal(t2, t0) and np.array_equal(c2, c0)


def test_closed_loop_without_host_round_trips_nx6_and_applied_noise():
    """B = 4096, N = 30: (1) the whole loop enqueued without a host synchronisation per step (every solve in the persistent
    launch; what went wrong would be noticed at the end and replayed) gives the same bits as the step-by-step form; (2) the
    nx = 6 model (extra progress state) plans the same first five states; (3) noise mode 2 (ForcesproOptimizer convention,
    optimizer.py:348-354) perturbs the applied input only"""
    B, L, N = 4096, 40, 30
    init, path, orient, vdes = _loop_inputs(B, L)
    s5 = pkg.BatchedMPCSolver(N, 5)
    s5.set_bounds()
    t_a, c_a, st_a = s5.closed_loop(init, path, orient, vdes, L)
    assert not s5.last_loop_replayed() and np.all(st_a == 1)
    s5.set_option("loop_async", "0")
    t_s, c_s, st_s = s5.closed_loop(init, path, orient, vdes, L)
    assert s5.last_loop_replayed()
    assert np.array_equal(t_a, t_s) and np.array_equal(c_a, c_s) and np.array_equal(st_a, st_s)
    s5.set_option("loop_async", None)
    s6 = pkg.BatchedMPCSolver(N, 6)
    s6.set_bounds()
    t6, c6, st6 = s6.closed_loop(init[:512], path[:512], orient[:512], vdes[:512], L)
    assert np.all(st6 == 1) and np.abs(t6 - t_a[:512]).max() < 1e-7 and np.abs(c6 - c_a[:512]).max() < 1e-7
    nz = __import__("importlib").import_module("motion-planning-for-autonomous-driving-with-mpc_amd.noise")
    t2, c2, _ = s5.closed_loop(init[:256], path[:256], orient[:256], vdes[:256], L, noise_mode=2, sigma=0.05, seed=5)
    want0 = np.stack([nz.applied_noise(5, b, 0, 0.05) for b in range(256)])
    assert np.abs(c2[:, 0] - c_a[:256, 0] - want0).max() < 1e-12 and np.array_equal(t2[:, 0], t_a[:256, 0])
    t0, c0, _ = s5.closed_loop(init[:256], path[:256], orient[:256], vdes[:256], L, noise_mode=2, sigma=0.0, seed=5)
    # (a 256-ego batch is solved by the wave-per-instance kernel alone, the 4096-ego one starts in the pipeline: same optima,
    #  different rounding of the KKT solves)
    assert np.abs(t0 - t_a[:256]).max() < 1e-8 and np.abs(c0 - c_a[:256]).max() < 1e-8


# ---- hybrid solve: pipeline while a tile has many instances iterating, then one wavefront per instance with the MFMA Riccati ----------

@pytest.mark.parametrize("B", [4096, 3000, 256])
def test_hybrid_solve_matches_oracle_and_the_pipeline(B):
    """default path at the BASELINE size and below: both kernels took part (B = 4096, 3000) or the wave-per-instance kernel alone
    (B = 256: every tile would hand over at once); against the oracle 1e-8 with the same iteration counts, against the pure
    pipeline 1e-9"""
    cfg, kw = FAMILIES["zamlf_n30_nx6"]
    x0, p = synthetic_batch(cfg, B, **kw)
    s = make_solver(cfg)
    r = s.solve(x0, p)
    pp, rp = s.get_pipeline_profile(), s.get_resident_profile()
    assert np.all(r.status == 1) and r.kkt.max() <= 1e-8
    if B == 256:
        assert not pp["ran"] and rp["ran"] and rp["rounds"] == int(r.iters.max())
    else:
        assert pp["ran"] and 0 < pp["rounds"] < int(r.iters.max())
    s.set_option("hybrid", "0")
    ref = s.solve(x0, p)
    assert np.array_equal(r.iters, ref.iters) and np.array_equal(r.status, ref.status) and np.abs(r.x - ref.x).max() < 1e-9
    sub = slice(0, B, max(1, B // 64))
    ro = OracleSolver(cfg).solve_batch(x0[sub], p[sub], nthreads=8)
    assert np.array_equal(r.iters[sub], ro["iters"]) and np.abs(r.x[sub] - ro["x"]).max() < TOL_ORACLE


def test_instances_per_wavefront_follow_the_batch_size():
    """hybrid_bx = 0 (the default): one instance per wavefront of k_solve_wg while the batch fits the machine that way (B <= 4 x CUs),
    two beyond; the statistics of the launch behind a pipeline come back with the pipeline's control block"""
    import torch
    cfg, kw = FAMILIES["zamlf_n30_nx6"]
    s = make_solver(cfg)
    assert s.get_option("hybrid_bx") == 0 and s.get_option("hybrid") == 1
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    for B in (256, 4 * n_cu, 4096):
        x0, p = synthetic_batch(cfg, B, **kw)
        r = s.solve(x0, p)
        rp, pp = s.get_resident_profile(), s.get_pipeline_profile()
        assert (r.status == 1).all() and rp["ran"]
        bx = 1 if B <= 4 * n_cu else 2
        # (behind the pipeline the workgroups are dealt from the hand-over lists: as many as the machine holds at once, or the lists' capacity)
        if pp["ran"]:
            assert 4 * n_cu <= rp["workgroups"] <= (B + bx - 1) // bx
        else:
            assert rp["workgroups"] == (B + bx - 1) // bx
        # every iteration of every instance is served by exactly one of the two kernels (k_solve_wg counts its own)
        assert rp["instance_iterations"] <= int(r.iters.sum()) and rp["sweeps"] >= rp["workgroup_rounds"] > 0
        assert pp["ran"] == (B > 2048) and (not pp["ran"] or rp["instance_iterations"] < int(r.iters.sum()))


@pytest.mark.parametrize("fam", ["zamlf_n30_nx6", "usalf_n50_nx5", "ca"])
def test_wave_per_instance_kernel_options_agree(fam):
    """k_solve_wg alone (hand-over threshold 64) with one or two instances per wavefront: an instance's result does not depend on which
    instance shares its wavefront -- bit-identical"""
    if fam == "ca":
        cfg = CA_CFG
        x0, p = ca_batch(cfg, 256)
    else:
        cfg, kw = FAMILIES[fam]
        x0, p = synthetic_batch(cfg, 256, **kw)
    s = make_solver(cfg)
    set_cfg_bounds(s, cfg)
    s.set_option("rescue", "0")
    s.set_option("hybrid_live", "64")
    res = []
    for bx in ("1", "2"):
        s.set_option("hybrid_bx", bx)
        res.append(s.solve(x0, p))
        rp = s.get_resident_profile()
        assert rp["ran"] and not s.get_pipeline_profile()["ran"]
        if fam == "ca":
            # the case the comparison is for: wavefronts whose two instances part ways -- one re-sweeps with an inertia correction
            # (more sweeps than rounds) or gives up (-7) while its mate goes on
            st = res[-1].status
            assert rp["sweeps"] > rp["workgroup_rounds"] and (st == -7).any()
            if bx == "2":
                assert ((st[0::2] == -7) != (st[1::2] == -7)).any()
    assert _same(res[0], res[1])
    ro = OracleSolver(cfg).solve_batch(x0[:64], p[:64], nthreads=8)
    both = (res[0].status[:64] == 1) & (ro["status"] == 1)
    assert both.mean() > 0.9
    if fam != "ca":
        assert np.array_equal(res[0].iters[:64], ro["iters"]) and np.abs(res[0].x[:64] - ro["x"]).max() < TOL_ORACLE
    else:       # nonconvex: the same basin for nearly all, a handful may differ
        assert np.mean(np.abs(res[0].x[:64][both] - ro["x"][both]).max(axis=1) < 1e-6) > 0.9


# ---- advisor round 3: the batch dependence of the hybrid solve ---------------------------------------

def test_hybrid_solve_keeps_the_basin_of_every_collision_avoidance_instance_under_permutation():
    """the hybrid solve's KKT solver of an iteration depends on how many instances of the 64-instance tile still iterate (DESIGN.md section 4,
    INTEGRATION.md "Reproducibility"): results depend on the batch composition at the 1e-9 level.  On the nonconvex family that must not
    move an instance to the other side of the obstacle: a permuted batch returns, row for row, the same status and the same local optimum."""
    B = 4096
    x0, p = ca_batch(CA_CFG, B)
    s = make_solver(CA_CFG)
    set_cfg_bounds(s, CA_CFG)
    s.set_option("rescue", "0")                       # (the second chance re-solves failed rows in sub-batches of their own)
    a = s.solve(x0, p)
    assert s.get_pipeline_profile()["ran"] and s.get_resident_profile()["ran"]
    perm = np.random.default_rng(5).permutation(B)
    b = s.solve(x0[perm], p[perm])
    bx, bst = np.empty_like(b.x), np.empty_like(b.status)
    bx[perm], bst[perm] = b.x, b.status
    both = (a.status == 1) & (bst == 1)
    assert np.mean(a.status == bst) >= 0.995 and both.mean() >= 0.97
    assert np.abs(a.x[both] - bx[both]).max() < 1e-5          # same basin (the two basins of an instance differ by metres)
    s.set_option("hybrid", "0")                       # the reproducible mode: bit-exact under permutation
    c = s.solve(x0, p)
    d = s.solve(x0[perm], p[perm])
    dx = np.empty_like(d.x)
    dx[perm] = d.x
    assert np.array_equal(c.x, dx)


def test_workspace_gets_its_mailbox_section_only_when_k_solve_wg_can_run():
    """advisor round 3: the instance-major mailbox arrays (as large as the tile-major section) are allocated for handles that can launch
    k_solve_wg; switching the hybrid solve on later re-allocates, and either way the results are those of the oracle"""
    cfg, kw = FAMILIES["zamlf_n30_nx6"]
    x0, p = synthetic_batch(cfg, 300, **kw)
    ro = OracleSolver(cfg).solve_batch(x0[:32], p[:32], nthreads=8)
    s = make_solver(cfg)
    s.set_option("hybrid", "0")                       # before the first solve: no k_solve_wg on this handle, no mailbox
    r0 = s.solve(x0, p)
    assert not s.get_resident_profile()["ran"] and np.abs(r0.x[:32] - ro["x"]).max() < TOL_ORACLE
    s.set_option("hybrid", "1")                       # now the kernel is wanted: the workspace grows its mailbox section
    r1 = s.solve(x0, p)
    assert s.get_resident_profile()["ran"] and np.array_equal(r1.iters, r0.iters) and np.abs(r1.x - r0.x).max() < 1e-9
    s.set_option("hybrid", "0")
    r2 = s.solve(x0, p)
    assert np.array_equal(r2.x, r0.x)


def test_mfma_riccati_unit_test_binary():
    """tools/ubench/ric_mfma_test (built by __graft_entry__.build): the wave-per-instance MFMA sweeps of mpc_riccati_mfma.h against the scalar
    recursion on random stage blocks, one and two instances per wavefront, convex and with an indefinite stage (inertia correction, the
    mate re-swept or not) -- relative errors <= 1e-10, identical sweep counts"""
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "ubench", "ric_mfma_test")
    if not os.path.exists(exe):
        pytest.fail("tools/ubench/ric_mfma_test is not built: run __graft_entry__.build()")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
    assert "with an indefinite stage" in r.stdout and "mismatching sweep counts 0" in r.stdout


