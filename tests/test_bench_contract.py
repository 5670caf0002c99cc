"""CPU checks of bench.py's reporting helpers (the timed part needs the GPU): the roofline object
carries every field the contract names for both arithmetics, and the profiled-traffic lookup picks
the newest committed summary of the right precision."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_roofline_fields_and_arithmetic():
    import bench
    rays = 640000
    for precision, peak, per in (("fp32", 157.3, 1), ("f16x3", 2516.6, 3)):
        r = bench.roofline(precision, rays, kernel_ms=100.0, launches=5, with_traffic=True)
        for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
            assert key in r
        flop = rays * 127 * bench.FLOP_PER_SAMPLE
        assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and r["peak"] == peak
        assert abs(r["achieved"] - flop / 0.1 / 1e12) < 1e-9
        assert abs(r["frac"] - r["achieved"] / peak) < 1e-12
        assert abs(r["executed_frac"] - per * r["frac"]) < 1e-12
        assert r["algorithmic_bytes"] == rays * 212 + 48
        assert r["traffic"] is not None and r["traffic"] < 2 * r["algorithmic_bytes"]
        assert ("f16x3" in r["traffic_source"]) == (precision == "f16x3")
        json.dumps(r)


def test_bench_constants_match_the_survey():
    import bench
    assert bench.FLOP_PER_SAMPLE == 2 * (96 * 256 + 4 * 256 * 256 + 256 * 54)
    assert (bench.IMAGE, bench.SAMPLES) == (800, 128)


def test_defaults_are_the_reference_arithmetic_and_the_one_frame_partition(monkeypatch):
    """The driver-checked line: fp32 (the reference's arithmetic) and, for N > 1, row blocks of ONE
    frame (BASELINE config 4), 100 rows per GPU at N = 8."""
    import bench
    src = open(bench.__file__).read()
    assert 'os.environ.get("NERF_BENCH_PRECISION", "fp32")' in src
    assert 'choices=("weak", "strong"), default="strong"' in src
    assert [bench.shard_rows(r, 8) for r in (0, 3, 7)] == [(0, 100), (300, 400), (700, 800)]
    for world in (1, 2, 3, 4, 8):
        blocks = [bench.shard_rows(r, world) for r in range(world)]
        assert blocks[0][0] == 0 and blocks[-1][1] == bench.IMAGE
        assert all(a[1] == b[0] for a, b in zip(blocks, blocks[1:]))
    # one partition for the product and the bench: same blocks, and the per-rank ray counts the
    # line reports (`rays_per_gpu`) add up to the frame for every N the driver runs
    from nerf_amd import parallel
    for world in (1, 2, 4, 8):
        blocks = [bench.shard_rows(r, world) for r in range(world)]
        assert blocks == [parallel.shard_rows(bench.IMAGE, r, world) for r in range(world)]
        rays = [(e - b) * bench.IMAGE for b, e in blocks]
        assert sum(rays) == bench.IMAGE * bench.IMAGE and max(rays) - min(rays) <= bench.IMAGE
        assert rays[0] == bench.IMAGE * bench.IMAGE // world
    assert "--allow-gloo" in src and "refusing to measure" in src      # N > 1 without RCCL fails loudly
    assert bench.PRECISIONS["fp32"]["dtype"] == "f32"
    assert bench.physical_cores() >= 1
    assert isinstance(bench.cpu_model(), str) and bench.cpu_model()


def test_secondary_timings_carry_a_spread():
    """Every secondary figure is REPEATS loops of >= 50 steps (anything under 10 ms) or >= 5 steps (frames) with
    min / median / max in the entry (round-5 verdict: boxes differ by 4-6 %, targets sit 1-5 % away)."""
    import bench
    assert bench.REPEATS >= 5 and bench.SHORT_STEPS >= 50 and bench.FRAME_STEPS >= 5
    sp = bench.spread([3.0, 1.0, 2.0, 5.0, 4.0])
    assert (sp["min"], sp["median"], sp["max"], sp["loops"]) == (1.0, 3.0, 5.0, 5)
    assert bench.spread([1.0, 2.0, 3.0, 4.0])["median"] == 2.5
    src = open(bench.__file__).read()
    for fn in ("train_step_timing", "legacy_train_step_timing", "small_batch_step_timing", "legacy_workload_timing",
               "baseline_configs"):
        body = src[src.index("def " + fn):]
        body = body[:body.index("\ndef ", 10)]
        assert "timed_loops(" in body and "spread(" in body, fn
    for fn in ("train_step_timing", "legacy_train_step_timing"):      # per-kernel split of a training step
        body = src[src.index("def " + fn):]
        assert "kernel_split(" in body[:body.index("\ndef ", 10)], fn
    assert bench.train_tiles_of(256) == 16 and bench.train_tiles_of(128) == 8


def _bench(*argv, env=None, timeout=600):
    import subprocess
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True,
                          env=e, timeout=timeout)


def test_plain_gpus_8_starts_its_own_eight_ranks_dry_run():
    """``python bench.py --gpus 8`` with no launcher around it (the shape of the driver's one-GPU command) must not
    die on first contact: it starts the eight ranks itself before any GPU call.  ``--dry-run`` walks launch,
    rendezvous and partitions over gloo without a GPU, so the 8-rank form runs here: 100 rows = 80,000 rays of the
    frame and 512 rays of the config-5 batch per rank, one JSON line from rank 0, exit code 0."""
    run = _bench("--gpus", "8", "--steps", "2", "--warmup", "1", "--dry-run")
    assert run.returncode == 0, run.stderr[-3000:]
    assert "starting the ranks" in run.stderr and "torch.distributed.run" in run.stderr
    lines = [x for x in run.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["n_gpus"] == 8 and line["dry_run"] is True and line["value"] is None
    assert line["config"]["rays_per_gpu"] == 80000
    assert line["config"]["row_blocks"] == [[100 * r, 100 * (r + 1)] for r in range(8)]
    dp = line["train_step_dp"]
    assert dp["rays_per_rank"] == 512 and dp["global_batch"] == 4096
    assert dp["batch_blocks"] == [[512 * r, 512 * (r + 1)] for r in range(8)]
    assert dp["gradient_bytes"] == 304438 * 4 and dp["flat_all_reduce_matches_weighted_sum"] is True
    assert dp["scaling"] == "strong"
    weak = line["train_step_dp_weak"]              # the weak form of the same entry: 4096 rays PER RANK
    assert weak["scaling"] == "weak" and weak["rays_per_rank"] == 4096 and weak["global_batch"] == 8 * 4096
    assert weak["batch_blocks"] == [[4096 * r, 4096 * (r + 1)] for r in range(8)]


def test_launcher_and_gpus_disagreeing_is_a_message_not_an_assert():
    run = _bench("--gpus", "4", "--dry-run", env={"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert run.returncode == 2 and "WORLD_SIZE=2" in run.stderr and "AssertionError" not in run.stderr
    one = _bench("--gpus", "1", "--dry-run")                     # N = 1: no launcher, no rendezvous
    assert one.returncode == 0 and json.loads(one.stdout.strip().splitlines()[-1])["config"]["rays_per_gpu"] == 640000


def test_dump_outputs_writes_float32_arrays_within_64_mb(tmp_path):
    """--dump-outputs: the whole image and a fixed seeded pixel sample of the segmentation, float32, <= 64 MB for the
    full 800x800 frame; the sample is the same from call to call (two builds compare file by file); N > 1 ranks
    write their own row blocks under suffixed names."""
    import numpy as np
    import torch
    import bench
    image = torch.rand(1, bench.IMAGE, bench.IMAGE, 3)
    pixels = torch.arange(bench.IMAGE * bench.IMAGE, dtype=torch.float32)        # every class holds its pixel's index
    seg = pixels.reshape(1, bench.IMAGE, bench.IMAGE, 1).repeat(1, 1, 1, 50)
    for out in (tmp_path / "a", tmp_path / "b"):
        bench.dump_outputs(str(out), image, seg)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["image.npy", "segmentation_sample.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float32 and np.array_equal(a, b)
    assert np.array_equal(np.load(tmp_path / "a" / "image.npy"), image.numpy())
    sample = np.load(tmp_path / "a" / "segmentation_sample.npy")
    assert sample.shape == (bench.DUMP_SEG_PIXELS, 50)
    pixel = sample[:, 0].astype(np.int64)              # the sample's rows are whole pixels, in increasing order
    assert np.array_equal(sample, seg.reshape(-1, 50).numpy()[pixel]) and (np.diff(pixel) > 0).all()
    bench.dump_outputs(str(tmp_path / "r"), image[:, :100], seg[:, :100], rank=3)
    assert sorted(os.listdir(tmp_path / "r")) == ["image_rank3.npy", "segmentation_sample_rank3.npy"]
    assert np.load(tmp_path / "r" / "segmentation_sample_rank3.npy").shape == (bench.DUMP_SEG_PIXELS // 8, 50)


def test_steps_and_dump_outputs_are_options():
    run = _bench("--gpus", "1", "--steps", "0", "--dry-run")
    assert run.returncode == 2 and "--steps must be at least 1" in run.stderr
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert '"--dump-outputs"' in src and '"ms_per_step": m["elapsed"] / args.steps * 1e3' in src
