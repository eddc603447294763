"""bench.py's plain run, `--full` and `--dump-outputs`.

A plain run carries the headline alone; the secondary workloads appear only
under `--full`; `--dump-outputs DIR` writes what the last timed step returned
(count, changed) and the registers it left, which must equal the CPU oracle's
over the same seeded C2 keys and must not change from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
SECONDARY = ("bloom", "c4", "c5", "c5_zipf", "pcie_inclusive")


def test_dump_outputs_formats_and_fixed_sample(tmp_path, monkeypatch):
    import bench

    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 8192)
    big = np.arange(10_000, dtype=np.uint64) * 3
    arrays = {"big": big, "small": np.array([7], np.uint64), "regs": np.arange(16, dtype=np.uint8).astype(np.float32)}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in arrays}
    assert got["small"].dtype == np.float64 and got["small"].tolist() == [7.0]
    assert got["regs"].dtype == np.float32 and np.array_equal(got["regs"], arrays["regs"])
    # over its share of the budget: a sample of the array's own elements, in order, the same every time
    assert got["big"].dtype == np.float64 and got["big"].nbytes <= 8192 // 3 and got["big"].size > 100
    assert np.all(np.diff(got["big"]) >= 0) and np.all(np.isin(got["big"], big.astype(np.float64)))
    assert np.array_equal(got["big"], np.load(tmp_path / "b" / "big.npy"))
    assert sum(a.nbytes for a in got.values()) <= 8192


def _bench(args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1"] + args, env=env, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_dumps_match_the_oracle(tmp_path, orc):
    n = 200_003
    head = ["--steps", "3", "--warmup", "1", "--keys", str(n)]
    plain = _bench(head + ["--dump-outputs", str(tmp_path / "plain")])
    assert plain["steps"] == 3 and plain["warmup"] == 1 and plain["ms_per_step"] > 0
    assert plain["unit"] == "keys/s" and plain["dtype"] == "u64" and plain["higher_is_better"] is True
    assert plain["roofline"]["launches"] == 3  # --steps is the number of timed steps
    assert plain["value"] == pytest.approx(n / (plain["ms_per_step"] / 1e3), rel=1e-9)
    assert not [k for k in SECONDARY if k in plain] and plain["cpu_baseline"] is None
    assert sorted(os.listdir(tmp_path / "plain")) == ["changed.npy", "count.npy", "registers.npy"]
    out = {f[:-4]: np.load(tmp_path / "plain" / f) for f in os.listdir(tmp_path / "plain")}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    ref = np.zeros(orc.REGISTERS, np.uint8)
    orc.hll_add(ref, orc.gen_keys16(0x5EED0002, 0, n), None, 16, n)
    assert np.array_equal(out["registers"], ref.astype(np.float32))
    assert out["count"].tolist() == [float(orc.hll_count_dense(ref))] and plain["count"] == orc.hll_count_dense(ref)
    assert out["changed"].tolist() == [0.0]  # the warm-up step had already added every key
    # --full: the same headline over the same inputs, and the secondary legs beside it
    # (here the CPU baseline and the host-resident keys, on a small sample)
    full = _bench(head + ["--dump-outputs", str(tmp_path / "full"), "--full", "--no-extra", "--no-bloom",
                          "--cpu-sample", "65536", "--cpu-passes", "1"])
    assert full["cpu_baseline"]["value"] > 0 and full["pcie_inclusive"]["value"] > 0
    assert full["count"] == plain["count"]
    for f in os.listdir(tmp_path / "plain"):
        assert np.array_equal(np.load(tmp_path / "full" / f), out[f[:-4]])


@pytest.mark.gpu
def test_c5_dump_is_the_steps_replies(tmp_path, engine):
    """--workload c5: counts / count_with are the step's replies (taken before
    its mergeWith), merged_counts the destinations' counts after it; the same
    calls made here over the same seeded pairs and ids must give them."""
    from redisson_amd import devmem
    from redisson_amd.hyperloglog import GroupedHyperLogLog

    n, G, ops = 100_003, 1000, 257
    res = _bench(["--workload", "c5", "--steps", "2", "--warmup", "1", "--keys", str(n), "--groups", str(G),
                  "--batch-ops", str(ops), "--dump-outputs", str(tmp_path)])
    assert res["unit"] == "pairs/s" and "checkpoint" not in res
    out = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert sorted(out) == ["count_with", "counts", "merged_counts"]
    assert all(a.dtype == np.float64 for a in out.values())
    rng = np.random.default_rng(5)  # bench.py's ids of rank 0
    cw = np.stack([rng.integers(0, G, size=ops, dtype=np.uint64), rng.integers(0, G, size=ops, dtype=np.uint64)], 1)
    md = rng.integers(0, G, size=ops, dtype=np.uint64)
    ms = rng.integers(0, G, size=ops, dtype=np.uint64)
    groups, gkeys = devmem.gen_grouped(engine, 0x5EED0006, G, 0, n)
    pool = GroupedHyperLogLog(engine, G)
    try:
        pool.add(gkeys.keys_fixed(n, 16), groups)
        assert np.array_equal(out["counts"], pool.count().astype(np.float64))
        assert np.array_equal(out["count_with"], pool.countWith(cw).astype(np.float64))
        pool.mergeWith(md, ms)
        assert np.array_equal(out["merged_counts"], pool.count(md).astype(np.float64))
    finally:
        pool.close()
        groups.free()
        gkeys.free()
