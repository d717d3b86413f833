"""CPU: the product-side workload generators (tools/workloads.py -- what bench.py times) produce exactly the rows the oracle-side
generators of the tests produce; the mixed scenario sweep (BASELINE configuration 5) partitions its rows by shard and family
without loss; bench.py refuses to report fewer GPUs than it was asked for; the mixed shard -> family mapping under a 2-rank gloo
group with the per-rank solves done by the kernel emulation harness."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from helpers import CA_CFG, FAMILIES, ROOT, ca_batch, emu_solve
from oracle.nlp_numpy import BicycleNLP, NLPConfig, synthetic_batch

sys.path.insert(0, os.path.join(ROOT, "tools"))
import workloads as wl  # noqa: E402


def _cfg_of(fam):
    return NLPConfig(N=fam.N, nx=fam.nx, dt=fam.dt, Q=fam.Q, R=fam.R, obstacle=fam.obstacle)


def test_generators_agree_with_the_oracle_side():
    for name, oname, kw in (("zamlf_n30_nx6", "zamlf_n30_nx6", {}), ("usalf_n50_nx5", "usalf_n50_nx5", dict(v_range=(5.0, 9.0))),
                            ("tutlf_n30_nx5", "zamlf_n30_nx5", dict(v_range=(3.0, 9.0)))):
        fam = wl.FAMILIES[name]
        x0, p = wl.batch(fam, 9, start=5)
        xo, po = synthetic_batch(FAMILIES[oname][0], 9, start=5, **kw)
        assert np.array_equal(x0, xo) and np.array_equal(p, po)
    fam = wl.FAMILIES["zamca_n30_nx5"]
    x0, p = wl.batch(fam, 7, start=3)
    xo, po = ca_batch(CA_CFG, 7, start=3)
    assert np.array_equal(x0, xo) and np.array_equal(p, po)


@pytest.mark.parametrize("name", list(wl.FAMILIES))
def test_bounds_agree_with_the_oracle_side(name):
    fam = wl.FAMILIES[name]
    lbx, ubx, lbg, ubg = wl.bounds(fam)
    olbg, oubg, olbx, oubx = BicycleNLP(_cfg_of(fam)).bounds()
    for a, b in ((lbx, olbx), (ubx, oubx), (lbg, olbg), (ubg, oubg)):
        assert np.array_equal(a, b)
    assert fam.n_w == _cfg_of(fam).n_w and fam.n_g == _cfg_of(fam).n_g


def test_mixed_sweep_partition():
    """32 768 rows, 8 shards of 4096, four families dealt row by row: every row exactly once, shards contiguous"""
    seen = np.zeros(wl.MIXED_TOTAL, dtype=int)
    for r in range(8):
        rows = wl.mixed_shard_rows(r, 8)
        allr = np.sort(np.concatenate(list(rows.values())))
        assert allr[0] == r * wl.MIXED_SHARD and allr[-1] == (r + 1) * wl.MIXED_SHARD - 1 and len(allr) == wl.MIXED_SHARD
        for i, name in enumerate(wl.MIXED_ORDER):
            assert np.all(rows[name] % len(wl.MIXED_ORDER) == i)
            assert len(rows[name]) == wl.MIXED_SHARD // len(wl.MIXED_ORDER)
        seen[allr] += 1
    assert np.all(seen == 1)
    assert wl.MIXED_ROW_WIDTH == 355


def test_bench_refuses_to_shrink_the_job():
    """no GPU here: `--gpus 2` without a launcher must fail loudly, never print an n_gpus = 1 line; a launcher whose world size
    disagrees with --gpus must fail too"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "n_gpus" not in r.stdout and "refusing" in (r.stderr + r.stdout)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], env=dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "n_gpus" not in r.stdout and "must agree" in (r.stderr + r.stdout)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


TOTAL = 24          # a small "sweep": 2 shards of 12 rows, 3 rows per family and shard


def _worker(rank, world, port, outdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    per = TOTAL // world
    res = torch.zeros(per, wl.MIXED_ROW_WIDTH, dtype=torch.float64)
    for name, (rows, x0, p) in wl.mixed_shard(rank, world, total=TOTAL).items():
        fam = wl.FAMILIES[name]
        r = emu_solve(_cfg_of(fam), x0, p)                          # one "handle" per family on every rank
        assert np.all(r["status"] == 1)
        res[torch.from_numpy(rows - rank * per), : fam.n_w] = torch.from_numpy(r["x"])
    outs = [torch.empty_like(res) for _ in range(world)]
    dist.all_gather(outs, res)                                       # the one collective of the path
    if rank == 0:
        np.save(os.path.join(outdir, "mixed.npy"), torch.cat(outs).numpy())
    dist.destroy_process_group()


def test_mixed_sweep_two_ranks_gloo(tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    got = np.load(tmp_path / "mixed.npy")
    assert got.shape == (TOTAL, wl.MIXED_ROW_WIDTH)
    for g in range(TOTAL):
        fam = wl.FAMILIES[wl.MIXED_ORDER[g % len(wl.MIXED_ORDER)]]
        x0, p = wl.instance(fam, g)
        ref = emu_solve(_cfg_of(fam), x0[None], p[None])["x"][0]
        assert np.abs(got[g, : fam.n_w] - ref).max() < 1e-12 and np.all(got[g, fam.n_w:] == 0.0)


TOTAL8 = 48         # 8 shards of 6 rows: 2 + 2 + 1 + 1 rows per family, and WHICH families get two shifts from rank to rank (ragged per rank and family)


def _oracle_rows(fam, x0, p):
    from oracle.binding import OracleSolver
    r = OracleSolver(_cfg_of(fam)).solve_batch(x0, p, nthreads=1)
    return r["x"], r["status"].astype(np.int32), r["iters"].astype(np.int32)


def _worker8(rank, world, port, outdir):
    """what bench.py's run_mixed does on a rank, with the solves answered by the oracle: one 'handle' per family, result rows scattered into the
    rank's padded block at their LOCAL row, status and iteration count in the two extra columns, ONE packed all-gather, statistics reduced over ranks"""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sharding = __import__("importlib").import_module("motion-planning-for-autonomous-driving-with-mpc_amd.sharding")
    per = TOTAL8 // world
    W, PW = wl.MIXED_ROW_WIDTH, sharding.packed_width(wl.MIXED_ROW_WIDTH)
    blk = torch.zeros(per, PW, dtype=torch.float64)
    sizes, stats = {}, {}
    for name, (rows, x0, p) in wl.mixed_shard(rank, world, total=TOTAL8).items():
        fam = wl.FAMILIES[name]
        sizes[name] = len(rows)
        x, st, it = _oracle_rows(fam, x0, p)
        local = torch.from_numpy(rows - rank * per)
        blk[local, : fam.n_w] = torch.from_numpy(x)
        blk[local, W] = torch.from_numpy(st).double()
        blk[local, W + 1] = torch.from_numpy(it).double()
        stats[name] = sharding.solve_stats_over_ranks(st, it)              # (every rank calls it for every family, in the same order)
    out = torch.empty((world * per, PW), dtype=torch.float64)
    sharding.gather_packed(blk, out)
    np.savez(os.path.join(outdir, "r%d.npz" % rank), out=out.numpy(), sizes=np.array([sizes[n] for n in wl.MIXED_ORDER]),
             **{"stat_" + n: np.array([stats[n]["rows"], stats[n]["mean_iters"], stats[n]["max_iters"], stats[n]["converged_frac"]]) for n in wl.MIXED_ORDER})
    dist.destroy_process_group()


def test_mixed_sweep_eight_ranks_gloo_packed_gather_and_statistics(tmp_path):
    """SURVEY 8(e) / BASELINE configuration 5 at its real rank count (no 8-GPU node in this build): eight processes, the shard -> family mapping of
    bench.py's run_mixed with family sizes that differ from rank to rank, the packed all-gather, the per-family statistics over all ranks.  Every
    rank must end with the same block; row g of it is the solve of GLOBAL row g by the family the generator assigns, with its status and iterations."""
    world = 8
    mp.spawn(_worker8, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    got = [np.load(tmp_path / ("r%d.npz" % r)) for r in range(world)]
    sizes = np.array([g["sizes"] for g in got])
    assert sizes.sum() == TOTAL8 and len({tuple(s) for s in sizes}) > 1                 # ragged: not every rank has the same family sizes
    W = wl.MIXED_ROW_WIDTH
    for r in range(1, world):
        assert np.array_equal(got[r]["out"], got[0]["out"])
    out = got[0]["out"]
    its = {n: [] for n in wl.MIXED_ORDER}
    for g in range(TOTAL8):
        name = wl.MIXED_ORDER[g % len(wl.MIXED_ORDER)]
        fam = wl.FAMILIES[name]
        x0, p = wl.instance(fam, g)
        x, st, it = _oracle_rows(fam, x0[None], p[None])
        assert np.array_equal(out[g, : fam.n_w], x[0]) and np.all(out[g, fam.n_w:W] == 0.0)
        assert out[g, W] == st[0] and out[g, W + 1] == it[0]
        its[name].append(int(it[0]))
    for n in wl.MIXED_ORDER:
        rows, mean_it, max_it, conv = got[3]["stat_" + n]
        assert rows == len(its[n]) and abs(mean_it - np.mean(its[n])) < 1e-12 and max_it == max(its[n]) and conv == 1.0


def test_bench_line_is_compact_and_carries_the_contract():
    """bench.py prints ONE line that fits the driver's 2000-character tail: every contract key, `roofline` (with the kernels of the loop one by
    one) and `cpu_baseline` as objects, configurations 2 - 5 and the side paths as arrays (the long form goes to stderr)"""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    long_form = json.load(open(os.path.join(ROOT, "tests", "golden", "bench_detail_sample.json")))
    line = bench.compact_line(long_form)
    text = json.dumps(line, separators=(",", ":"))
    assert len(text) < 2000, len(text)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in line, k
    assert line["config"]["workload"].startswith("N=30 nx=6") and "model" not in line["config"] and line["vs_baseline"] is None
    r = line["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and r["traffic"] > 0
    assert set(r["kernels"]) == {"k_pipeline", "k_solve_wg"} and all(len(v) == 3 for v in r["kernels"].values())
    cb = line["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and isinstance(cb["sample"], str)
    assert [c[0] for c in line["configs"]] == ["2", "3", "4", "5"] and all(len(c) == 9 for c in line["configs"])
    assert len(line["fixed20"]) == 2 and "forces_sqp" in line["other_paths"]


def test_plain_bench_line_and_output_dump(tmp_path):
    """a run without --full: the same contract keys with the extra objects null; --dump-outputs writes float64 .npy files, and a fixed seeded
    sample of the rows (with their indices) once the arrays exceed the limit"""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    long_form = json.load(open(os.path.join(ROOT, "tests", "golden", "bench_detail_sample.json")))
    long_form.update(fixed20=None, roofline=None, cpu_baseline=None, configs=None, other_paths=None, gather=None)
    line = bench.compact_line(long_form)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert line[k] == (long_form[k] if k not in ("value", "ms_per_step") else bench._g(long_form[k], 6 if k == "value" else 5)), k
    assert line["roofline"] is None and line["cpu_baseline"] is None and "configs" not in line
    rng = np.random.default_rng(3)
    arrays = dict(x=rng.normal(size=(100, 7)), status=np.ones(100, np.int32), kkt=rng.random(100))
    bench.dump_outputs(str(tmp_path / "all"), arrays)
    for k, a in arrays.items():
        got = np.load(tmp_path / "all" / (k + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, a)
    assert not (tmp_path / "all" / "rows.npy").exists()
    limit = 30 * (9 * 8 + 8)                                      # room for 30 of the 100 rows and their indices
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), arrays, limit=limit)
    rows = np.load(tmp_path / "s1" / "rows.npy")
    assert len(rows) == 30 and np.array_equal(rows, np.load(tmp_path / "s2" / "rows.npy")) and np.all(np.diff(rows) > 0)
    assert sum(np.load(tmp_path / "s1" / (k + ".npy")).nbytes for k in list(arrays) + ["rows"]) <= limit
    assert np.array_equal(np.load(tmp_path / "s1" / "x.npy"), arrays["x"][rows.astype(int)])
