"""CPU: bench.py's rank fan-out.  `python bench.py --gpus 2`
without a launcher starts two ranks itself; a launcher whose WORLD_SIZE
differs from --gpus is an error.  MPLIB_AMD_BENCH_DRYRUN=1 runs the launch,
process group (gloo), barrier and max-over-ranks reduction without device
work (no GPU here); the -m gpu twin is test_bench_one_rank_nccl."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                              "MASTER_PORT")}
    env.update(kw)
    return env


def test_bench_gpus2_spawns_two_ranks():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2",
                          "--warmup", "0"], env=_env(MPLIB_AMD_BENCH_DRYRUN="1", MPLIB_AMD_DIST_BACKEND="gloo"),
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout  # rank 0 only
    r = json.loads(lines[0])
    assert r["n_gpus"] == 2 and r["dry_run"] and r["max_rank"] == 1 and r["backend"] == "gloo"


def test_bench_world_size_mismatch_fails():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"],
                         env=_env(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", MPLIB_AMD_BENCH_DRYRUN="1"),
                         capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert out.returncode != 0 and "WORLD_SIZE=1" in out.stderr


def test_dump_outputs_formats_and_sample(tmp_path):
    """--dump-outputs: flags as float32, 32-bit mask words (unsigned) as
    float64, every value exact; above the byte limit a seeded sample that is
    the same rows for every array and the same from call to call."""
    import numpy as np
    import bench
    rng = np.random.default_rng(5)
    n, W = 1000, 5
    flags = rng.integers(0, 2, n).astype(np.uint8)
    masks = rng.integers(-2**31, 2**31, (n, W)).astype(np.int32)  # the device buffer's dtype
    bench.dump_outputs(str(tmp_path / "a"), {"flags": flags, "masks": masks})
    f, m = np.load(tmp_path / "a" / "flags.npy"), np.load(tmp_path / "a" / "masks.npy")
    assert f.dtype == np.float32 and m.dtype == np.float64
    np.testing.assert_array_equal(f, flags)
    np.testing.assert_array_equal(m, masks.view(np.uint32))
    limit = (4 + 8 * W) * 300
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), {"flags": flags, "masks": masks}, limit)
    f, m = np.load(tmp_path / "b" / "flags.npy"), np.load(tmp_path / "b" / "masks.npy")
    assert len(f) == len(m) == 300 and f.nbytes + m.nbytes <= limit
    rows = np.sort(np.random.default_rng(0).choice(n, 300, replace=False))
    np.testing.assert_array_equal(f, flags[rows])
    np.testing.assert_array_equal(m, masks.view(np.uint32)[rows])
    np.testing.assert_array_equal(f, np.load(tmp_path / "c" / "flags.npy"))
    np.testing.assert_array_equal(m, np.load(tmp_path / "c" / "masks.npy"))


def test_full_and_dump_outputs_are_off_by_default(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"
