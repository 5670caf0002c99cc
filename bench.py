"""Headline benchmark: ray-samples/sec of the fused MI355X renderer on a synthetic
800x800 frame at 128 samples per ray (BASELINE.json metric).

    python bench.py --gpus 1 --steps 20 --warmup 3
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W
    python bench.py --gpus N --steps K --warmup W        (no launcher: bench.py starts the N ranks itself)

Launch convention: under ``torch.distributed.run`` (WORLD_SIZE set) this process IS one rank.  A plain
``python bench.py --gpus N`` with N > 1 and no WORLD_SIZE becomes the launcher: before it makes any GPU call
it starts ``python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1
--master-port <free> bench.py <the same arguments>`` as a CHILD process (never an exec), lets the child's
output through unchanged (rank 0's one JSON line) and exits with the child's code.  ``--dry-run`` walks the
same launch + rendezvous + partition code over gloo without touching a GPU (the 8-rank form of the path can
be rehearsed on any machine; a one-GPU box of this pool allows at most 6 processes on its card).

One step = NeRF.render_image of the 800x800x128 frame (rays generated in-kernel from the pose,
deterministic fenceposts, RGB + 50-class segmentation composited): the whole hot path, inputs
(pose, packed parameters) resident in HBM.  Rays are independent, so N GPUs shard the rows of
ONE frame, 800 / N rows each, with no data-path collective (BASELINE.json config 4, "strong"
scaling: the default for N > 1; at N = 1 that is the whole frame).  ``--scaling weak`` renders one
whole frame per GPU instead; for N > 1 the line carries that measurement too (`weak_scaling`),
taken in the same run.  Rank 0 prints one JSON line.

The headline (`value`, `dtype`, `roofline`) is the reference's arithmetic: "fp32", exact-fp32 MFMA
(v_mfma_f32_16x16x4_f32; the reference computes in torch fp32, nerf/model.py:525-542).  The second
arithmetic of the same kernel (NerfHipRenderArgs.precision) — "f16x3", every
fp32 product as three f16 MFMAs with fp32 accumulation, held to the same parity tests — is measured
at N = 1 in the same run with the same step and warm-up counts and reported beside it
(`other_precision`); ``--precision f16x3`` swaps the two.

roofline: the render kernel is MFMA-bound; achieved = evaluated samples per launch x 601,088
ALGORITHMIC FLOP / average kernel duration measured with HIP events on the launch stream; peak =
the dense MFMA peak of the instruction's input type (MI355X_MICROARCH.md): 157.3 TFLOP/s fp32,
2516.6 TFLOP/s f16.  The f16x3 path executes 3 MFMA FLOP per algorithmic FLOP (`executed_frac`).
cpu_baseline: the oracle (a torch-CPU port of the reference, oracle/nerf_oracle.py) timed on
this box's host cores on a bounded block of rows of the same frame.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

IMAGE = 800
SAMPLES = 128
FOCAL = 896.0
FLOP_PER_SAMPLE = 601088          # 2*(96*256 + 4*256*256 + 256*54), SURVEY.md section 8d
PEAK_TFLOPS_FP32_MFMA = 157.3     # MI355X_MICROARCH.md, chip-level parameters
PEAK_TFLOPS_F16_MFMA = 2516.6     # dense f16/bf16: 1024 FLOP/clk/SIMD x 1024 SIMDs x 2.4 GHz
PRECISIONS = {
    "fp32": {"dtype": "f32", "peak": PEAK_TFLOPS_FP32_MFMA, "mfma_per_product": 1,
             "peak_note": "exact-fp32 MFMA (v_mfma_f32_16x16x4_f32) peak; algorithmic FLOPs only"},
    "f16x3": {"dtype": "f16x3 (f32 accumulate)", "peak": PEAK_TFLOPS_F16_MFMA, "mfma_per_product": 3,
              "peak_note": "dense f16 MFMA (v_mfma_f32_16x16x32_f16) peak; `achieved`/`frac` count "
                           "ALGORITHMIC FLOPs, the kernel executes 3 MFMA FLOP per algorithmic FLOP "
                           "(hi.hi + hi.lo + lo.hi): executed_frac = 3 x frac"},
}
CAMERA = (0.0, -3.0, 2.6)


def look_at(camera_o):
    """Pose looking at the origin, z up, built like the reference's get_rotation_matrix."""
    from nerf_amd import NeRF
    cam = torch.tensor([camera_o], dtype=torch.float32)
    eye = -cam / torch.linalg.norm(cam, dim=-1, keepdim=True)
    z = torch.tensor([[0.0, 0.0, 1.0]])
    up = z - (z * eye).sum(-1, keepdim=True) * eye
    up = up / torch.linalg.norm(up, dim=-1, keepdim=True)
    return cam, NeRF.get_rotation_matrix(eye, up)


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.lower().startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    import platform
    return platform.processor() or platform.machine()


def physical_cores():
    """Physical cores this process may run on: distinct (socket, core) pairs of /proc/cpuinfo among the
    logical CPUs of its affinity mask (SMT siblings share a pair)."""
    try:
        allowed = os.sched_getaffinity(0)
    except AttributeError:
        allowed = set(range(os.cpu_count() or 1))
    pairs, cpu, phys = set(), None, None
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                key, _, val = line.partition(":")
                key = key.strip()
                if key == "processor":
                    cpu, phys = int(val), None
                elif key == "physical id":
                    phys = int(val)
                elif key == "core id" and cpu in allowed:
                    pairs.add((phys, int(val)))
    except (OSError, ValueError):
        pass
    return len(pairs) or len(allowed)


def cpu_quota():
    """CPUs the container's cgroup grants (cpu.max), or None when unlimited / unreadable."""
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()
        return None if quota == "max" else float(quota) / float(period)
    except (OSError, ValueError):
        return None


def cpu_baseline_run(threads, budget_s, max_rows=32):
    """Oracle render of up to `max_rows` image rows of the bench frame on `threads` host threads,
    stopped after `budget_s` seconds (the sample actually rendered is reported)."""
    from oracle import nerf_oracle as O
    torch.set_num_threads(threads)
    params = O.init_params(seed=0)
    cfg = dict(O.default_config(), focal_length=FOCAL)
    cam_o, cam_r = look_at(CAMERA)
    rays_o, rays_d = O.image_rays(cam_o, cam_r, IMAGE, IMAGE, FOCAL)
    r0 = (IMAGE - max_rows) // 2
    sl = slice(r0 * IMAGE, (r0 + max_rows) * IMAGE)
    o, d = rays_o[sl], rays_d[sl]
    done = 0
    with torch.no_grad():
        O.render_rays(params, cfg, o[:1024], d[:1024], SAMPLES)          # warm-up
        t0 = time.perf_counter()
        for a, b in zip(torch.split(o, 1024), torch.split(d, 1024)):
            O.render_rays(params, cfg, a, b, SAMPLES)
            done += a.shape[0]
            if time.perf_counter() - t0 > budget_s:
                break
        dt = time.perf_counter() - t0
    return done * SAMPLES / dt, done, dt


def cpu_baseline_small(threads):
    """BASELINE config 1 / BASELINE.md section 4 "100x100x64 always": the WHOLE tiny_nerf-sized frame through the
    oracle (max_chunk_size 1024, no_grad, focal 112, the bench pose) on `threads` host threads."""
    from oracle import nerf_oracle as O
    torch.set_num_threads(threads)
    params = O.init_params(seed=0)
    cfg = dict(O.default_config(), focal_length=112.0)
    cam_o, cam_r = look_at(CAMERA)
    rays_o, rays_d = O.image_rays(cam_o, cam_r, 100, 100, 112.0)
    with torch.no_grad():
        O.render_rays(params, cfg, rays_o[:1024], rays_d[:1024], 64)          # warm-up
        t0 = time.perf_counter()
        for a, b in zip(torch.split(rays_o, 1024), torch.split(rays_d, 1024)):
            O.render_rays(params, cfg, a, b, 64)
        dt = time.perf_counter() - t0
    return {"workload": "100x100 frame, 64 samples/ray, whole frame (BASELINE config 1), max_chunk_size 1024",
            "cores": threads, "seconds": dt, "value": 100 * 100 * 64 / dt, "unit": "ray-samples/s"}


def cpu_baseline():
    """The oracle on this box's host cores, twice: on min(16, CPUs) threads (the CPU share a one-GPU
    slot of the pool is sized for) and on one thread per PHYSICAL core of the affinity mask
    (BASELINE.md section 4).  `value` / `cores` are the better of the two; both are reported.  Beside the
    bounded sample of the 800x800x128 frame, the whole 100x100x64 frame (BASELINE config 1) on the better
    thread count: `config1_100x100x64`."""
    logical = os.cpu_count() or 1
    runs = []
    for threads, budget in ((min(logical, 16), 12.0), (physical_cores(), 10.0)):
        if any(r["cores"] == threads for r in runs):
            continue
        value, rays, dt = cpu_baseline_run(threads, budget)
        runs.append({"cores": threads, "value": value, "rays": rays, "seconds": round(dt, 1)})
    best = max(runs, key=lambda r: r["value"])
    return {"value": best["value"], "unit": "ray-samples/s", "cores": best["cores"],
            "kind": "port", "cpu": cpu_model(), "host_cpus": logical, "physical_cores": physical_cores(),
            "cgroup_cpu_quota": cpu_quota(), "runs": runs,
            "sample": f"{best['rays']} rays (whole 1024-ray chunks of the middle rows) of the same 800x800x128 "
                      f"frame, {best['seconds']} s, torch {torch.__version__} CPU ops, oracle/nerf_oracle.py",
            "config1_100x100x64": cpu_baseline_small(best["cores"])}


REPEATS = 5                       # every secondary timing: REPEATS loops of `steps` steps, median / min / max reported
SHORT_STEPS = 50                  # steps per loop for anything under 10 ms
FRAME_STEPS = 5                   # ... and for whole frames


def spread(samples_ms):
    """min / median / max of the per-loop averages (ms) — boxes of this pool differ by 4-6 %, so a single mean of a
    5-10-step loop cannot decide a target that is 1-5 % away (round-5 verdict, weak 7)."""
    v = sorted(samples_ms)
    return {"median": v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2]),
            "min": v[0], "max": v[-1], "loops": len(v), "samples": [round(x, 5) for x in samples_ms]}


def timed_loops(dev, fn, steps, repeats=REPEATS, fence=None):
    """REPEATS synchronised loops of `steps` calls; the per-step average of each loop in ms."""
    out = []
    for _ in range(repeats):
        if fence is not None:
            fence()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        if fence is not None:
            fence()
        torch.cuda.synchronize(dev)
        out.append((time.perf_counter() - t0) / steps * 1e3)
    return out


def kernel_split(dev, fn, steps=20):
    """Average duration of every launch kind of one step (HIP events on the launch stream around each launch:
    nerf_hip_timing_read_tagged, include/nerf_hip.h) over `steps` extra, separately run steps — the events cost a
    few microseconds each, so this pass is not the one `ms_per_step` comes from."""
    from nerf_amd import _lib
    torch.cuda.synchronize(dev)
    _lib.timing(True)
    _lib.timing_read_tagged(reset=True)
    for _ in range(steps):
        fn()
    torch.cuda.synchronize(dev)
    tags = _lib.timing_read_tagged(reset=True)
    _lib.timing(False)
    out = {name: round(ms * n / steps, 5) for name, (ms, n) in tags.items()}      # ms per STEP (a kind may launch twice)
    out["sum"] = round(sum(out.values()), 5)
    return out


def train_tiles_of(hidden):
    """Register tiles per sample the TRAINING kernels of a network run at (nerf_amd/csrc/nerf_device.h: train_tiles):
    the saved rows and the weight gradient."""
    return 16 if hidden > 128 else 8


def train_compute_tiles_of(hidden, train_precision):
    """... and the tiles its training forward and data gradient COMPUTE at (nerf_device.h: train_compute_tiles): 4 for
    hidden_size <= 64 in fp32 arithmetic."""
    return 4 if hidden <= 64 and train_precision == "fp32" else train_tiles_of(hidden)


def train_step_timing(dev, rays=4096, samples=64, steps=SHORT_STEPS, warmup=5, train_precision="fp32", hidden=256, enc=32):
    """Secondary figure (BASELINE config 5 batch): one optimiser step = training forward + HIP
    backward + Adam on `rays` x `samples`; random rays/targets, stratified draws, noise std 1.
    `hidden` / `enc`: the constructor's hidden_size / encoding_size (nerf/model.py:471-475); a network of
    hidden_size <= 128 trains at its own cost in fp32 arithmetic (kernels at 8 register tiles per sample)."""
    from nerf_amd import NeRF
    from nerf_amd.optim import Adam
    from nerf_amd.loss import mse_and_grad
    torch.manual_seed(0)
    model = NeRF(hidden_size=hidden, encoding_size=enc).to(dev)
    model.train_precision = train_precision
    opt = Adam(model.parameters(), lr=1e-4)                               # as nerf_amd/trainer.py
    o, d = torch.randn(rays, 3, device=dev), torch.randn(rays, 3, device=dev)
    target = torch.rand(rays, 3, device=dev)

    def step():
        pixels, _ = model.render_rays(o, d, samples, randomly_sample=True, density_noise_std=1.0)
        loss, grad = mse_and_grad(pixels, target)        # the Trainer's step: loss + gradient in one launch
        opt.zero_grad()
        pixels.backward(grad)
        opt.step()

    for _ in range(warmup):
        step()
    ms = spread(timed_loops(dev, step, steps))
    kernels = kernel_split(dev, step)
    dt = ms["median"] * 1e-3
    flop = 2 * (3 * enc * hidden + 4 * hidden * hidden + 54 * hidden)
    tflops = 3 * flop * rays * (samples - 1) / dt / 1e12
    timing = {"ms_per_step": ms["median"], "ms_per_step_spread": ms, "steps_per_loop": steps, "kernels_ms": kernels}
    if hidden != 256:
        return {"workload": f"{rays} rays x {samples} samples, forward + backward + Adam, hidden_size={hidden}, "
                            f"encoding_size={enc} ({flop} FLOP per sample)",
                **timing, "ray_samples_per_s": rays * samples / dt, "tflops_fwd_dgrad_wgrad": tflops,
                "arithmetic": ("fp32 MFMA forward and data gradient, bf16-triple weight gradient" if train_precision == "fp32"
                               else "f16 pairs in all three kernels") +
                              f", training forward and data gradient at {train_compute_tiles_of(hidden, train_precision)} register "
                              f"tiles per sample, saved rows and weight gradient at {train_tiles_of(hidden)} (the network's own cost)"}
    return {"workload": f"{rays} rays x {samples} samples, forward + backward + Adam",
            **timing, "ray_samples_per_s": rays * samples / dt,
            "tflops_fwd_dgrad_wgrad": tflops,
            "arithmetic": ("training forward, data gradient and weight gradient on f16 pairs (three f16 MFMAs per "
                           "product; layer 0's weight gradient on bf16 triples); fp32 accumulate everywhere"
                           if train_precision == "f16x3" else
                           "training forward and data gradient on fp32 MFMA, weight gradient on bf16 triples (six "
                           "bf16 MFMAs per product); fp32 accumulate everywhere")}


def small_batch_step_timing(dev, rays=512, samples=64, steps=50, train_precision="f16x3"):
    """BASELINE config 5's share per GPU on 8 GPUs (512 rays x 64): one optimiser step eagerly and as ONE
    HIP-graph replay (forward + loss + backward + fused Adam, draws from torch's graph-safe generator) —
    the path nerf_amd.trainer.Trainer(graph=True) takes; at this size launches, not kernels, set the pace."""
    from nerf_amd import NeRF
    from nerf_amd.optim import Adam
    from nerf_amd.loss import mse_and_grad
    torch.manual_seed(0)
    model = NeRF().to(dev)
    model.train_precision = train_precision
    opt = Adam(model.parameters(), lr=1e-4)
    o, d = torch.randn(rays, 3, device=dev), torch.randn(rays, 3, device=dev)
    target = torch.rand(rays, 3, device=dev)

    def step():
        u = torch.rand(rays, samples, device=dev)
        noise = torch.randn(rays, samples - 1, 1, device=dev)
        pixels, _ = model.render_rays(o, d, samples, randomly_sample=True, density_noise_std=1.0, u=u, noise=noise)
        loss, grad = mse_and_grad(pixels, target)
        pixels.backward(grad)
        opt.step()

    def timed(fn):
        return spread(timed_loops(dev, fn, steps))

    def eager():
        opt.zero_grad(set_to_none=True)
        step()

    for _ in range(3):
        eager()
    t_eager = timed(eager)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(2):
            eager()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    opt.zero_grad(set_to_none=True)
    with torch.cuda.graph(graph, stream=side):
        step()
    graph.replay()
    t_graph = timed(graph.replay)
    return {"workload": f"{rays} rays x {samples} samples, forward + backward + Adam, {train_precision}",
            "ms_per_step_eager": t_eager["median"], "ms_per_step_graph": t_graph["median"],
            "eager_spread": t_eager, "graph_spread": t_graph, "steps_per_loop": steps,
            "ray_samples_per_s_graph": rays * samples / (t_graph["median"] * 1e-3)}


def train_step_dp(dev, rank, world, backend, steps, warmup, fence, rays=4096, samples=64, train_precision="f16x3",
                  scaling="strong"):
    """BASELINE config 5 as the N > 1 measurement: ONE 4096-ray batch per step, data-parallel over `world` ranks
    (rays rank * 4096 / world ... of the same batch on every rank), each rank running training forward + HIP backward
    on its share, then ONE in-place all-reduce of the flat 304,438-float gradient (nerf_amd/parallel.py), then the
    one-launch Adam redundantly on every rank; in-kernel Philox draws (rank folded into the key).  Reference step:
    train_conditional_nerf.py:115-135.  Measured twice: launch by launch with the collective bracketed by events on
    the launch stream, and as ONE HIP-graph replay per step — with RCCL the collective and the optimiser are inside
    the captured region (they are stream-ordered kernels), over gloo (a rehearsal) they stay outside and the entry
    says so.  Afterwards every rank's parameters must be bit-identical (checksum all-gather).
    scaling "strong": the ONE `rays`-ray batch of config 5 is cut over the ranks (512 rays each at 8: the step is then
    bounded by the small-batch rate of one GPU, about 5x at best by construction); "weak": `rays`
    rays PER RANK (global batch rays x world), the same step, collective and replica check — the form in which a
    multi-GPU record shows what the all-reduce costs this gradient at full occupancy."""
    per_rank = rays
    if scaling == "weak":
        rays = rays * world
    import torch.distributed as dist
    from nerf_amd import NeRF
    from nerf_amd.loss import mse_and_grad
    from nerf_amd.optim import Adam
    from nerf_amd.parallel import FlatGradientAllReduce, broadcast_parameters, shard_items
    torch.manual_seed(0)
    model = NeRF().to(dev)
    model.train_precision = train_precision
    model.rng = "philox"
    broadcast_parameters(model)
    begin, end = shard_items(rays, rank, world)
    gen = torch.Generator(device=dev).manual_seed(20260)             # the same global batch on every rank
    o_all = torch.randn(rays, 3, generator=gen, device=dev)
    d_all = torch.randn(rays, 3, generator=gen, device=dev)
    t_all = torch.rand(rays, 3, generator=gen, device=dev)
    o, d, target = (t[begin:end].contiguous() for t in (o_all, d_all, t_all))
    n, weight = end - begin, (end - begin) / float(rays)
    opt = Adam(model.parameters(), lr=1e-4)
    reduce = FlatGradientAllReduce(model.parameters())
    in_graph = backend == "nccl"
    marks = []

    def local_part():
        pixels, _ = model.render_rays(o, d, samples, randomly_sample=True, density_noise_std=1.0)
        loss, grad = mse_and_grad(pixels, target)
        pixels.backward(grad)

    def collective_part(timed=False):
        if timed:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        reduce(model.last_flat_grad, weight)
        if timed:
            e1.record()
            marks.append((e0, e1))
        opt.step()

    def eager(timed=False):
        opt.zero_grad(set_to_none=True)
        local_part()
        collective_part(timed)

    def timed_loop(fn):
        fence()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        fence()
        dt = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev if backend != "gloo" else "cpu")
        dist.all_reduce(dt, op=dist.ReduceOp.MAX)
        return float(dt.item()) / steps

    for _ in range(max(warmup, 3)):
        eager()
    t_eager = timed_loop(lambda: eager(True))
    allreduce_ms = sum(a.elapsed_time(b) for a, b in marks) / max(len(marks), 1)
    assert reduce.in_place_calls > 0, "the all-reduce must run in place on the backward's flat gradient"

    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):                                     # autograd's accumulation nodes on the capture stream
        for _ in range(2):
            eager()
    torch.cuda.current_stream(dev).wait_stream(side)
    fence()
    graph, captured, why = torch.cuda.CUDAGraph(), in_graph, None
    opt.zero_grad(set_to_none=True)
    try:
        with torch.cuda.graph(graph, stream=side):
            local_part()
            if in_graph:
                collective_part()
    except Exception as exc:                                          # (RCCL capture refused: fall back, and say so)
        if not in_graph:
            raise
        captured, why = False, f"{type(exc).__name__}: {exc}"[:200]
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        opt.zero_grad(set_to_none=True)
        with torch.cuda.graph(graph, stream=side):
            local_part()
    static_flat = model.last_flat_grad

    def replay():
        graph.replay()
        if not captured:
            reduce(static_flat, weight)
            opt.step()

    replay()
    t_graph = timed_loop(replay)
    # replicas: identical parameters on every rank after all those steps (sum of the parameters' bit patterns)
    bits = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).view(torch.int32).to(torch.int64)
    check = torch.stack([bits.sum(), (bits * torch.arange(1, bits.numel() + 1, device=dev)).sum()])
    if backend == "gloo":
        check = check.cpu()
    gathered = [torch.empty_like(check) for _ in range(world)]
    dist.all_gather(gathered, check)
    identical = all(torch.equal(g, gathered[0]) for g in gathered)
    finite = bool(torch.isfinite(torch.cat([p.detach().reshape(-1) for p in model.parameters()])).all())
    return {"scaling": scaling,
            "workload": f"BASELINE config 5{' (weak form: ' + str(per_rank) + ' rays PER RANK)' if scaling == 'weak' else ''}: "
                        f"{rays}-ray batches x {samples} samples, data-parallel over {world} ranks "
                        f"({n} rays on rank 0), training forward + HIP backward + one in-place all-reduce of the flat "
                        f"{reduce.numel}-float gradient + one-launch Adam on every rank; {train_precision}; in-kernel Philox draws",
            "rays_per_rank": n, "global_batch": rays, "steps": steps,
            "rendezvous_backend": backend, "collective": "all_reduce(SUM) of one flat fp32 buffer, in place",
            "gradient_bytes": reduce.numel * 4,
            "eager": {"ms_per_step": t_eager * 1e3, "allreduce_ms": allreduce_ms,
                      "ray_samples_per_s": rays * samples / t_eager},
            "graph": {"ms_per_step": t_graph * 1e3, "ray_samples_per_s": rays * samples / t_graph,
                      "collective_and_optimiser_in_graph": captured,
                      **({"capture_fallback": why} if why else {}),
                      **({} if in_graph else {"note": "gloo is a host-side collective: it and Adam run after the replay"})},
            "replicas_identical": identical, "parameters_finite": finite}


def legacy_workload_timing(dev, steps=FRAME_STEPS, warmup=1):
    """Second workload: the same 800x800x128 frame through the LEGACY 8 x 256 network of the
    reference's examples/nerf.pth (sin/cos encoding, skip trunk, view branch; 1,261,568 FLOP per sample,
    fp32 MFMA; weights: the reference's trained Lego checkpoint, fixture G9).  Parity unpinned."""
    import numpy as np
    from nerf_amd import _lib
    from nerf_amd.legacy import LegacyNeRF8x256, FLOP_PER_SAMPLE as LEGACY_FLOP
    path = os.path.join(ROOT, "tests", "golden", "g9_legacy_checkpoint.npz")
    with np.load(path) as z:
        params = {k[6:]: torch.from_numpy(np.array(z[k])) for k in z.files if k.startswith("param.")}
    model = LegacyNeRF8x256()
    model.load_state_dict(params)
    model = model.to(dev)
    cam = torch.tensor(CAMERA) / torch.tensor(CAMERA).norm() * 4.03
    cam_o, cam_r = look_at(tuple(cam.tolist()))
    cam_o, cam_r = cam_o.to(dev), cam_r.to(dev)
    focal = 138.88887889922103 * IMAGE / 100.0

    def step():
        with torch.no_grad():
            return model.render_image(cam_o, cam_r, IMAGE, IMAGE, focal, 2.0, 6.0, SAMPLES)

    def timed(precision):
        model.precision = precision
        for _ in range(warmup):
            step()
        torch.cuda.synchronize(dev)
        _lib.timing(True)
        _lib.timing_read(reset=True)
        ms = spread(timed_loops(dev, step, steps))
        kernel_ms, launches = _lib.timing_read(reset=True)
        _lib.timing(False)
        return ms["median"] * 1e-3, kernel_ms, ms

    flop = IMAGE * IMAGE * SAMPLES * LEGACY_FLOP
    dt, kernel_ms, ms = timed("fp32")
    achieved = flop / (kernel_ms * 1e-3) / 1e12
    dt_h, kernel_ms_h, ms_h = timed("f16x3")
    achieved_h = flop / (kernel_ms_h * 1e-3) / 1e12
    return {"workload": "legacy 8x256 network (examples/nerf.pth weights), 800x800, 128 samples/ray, "
                        "sin/cos positional encoding, fp32 MFMA; parity unpinned",
            "value": IMAGE * IMAGE * SAMPLES / dt, "unit": "ray-samples/s", "steps": steps,
            "ms_per_step": dt * 1e3, "ms_per_step_spread": ms, "kernel_ms": kernel_ms, "flop_per_sample": LEGACY_FLOP,
            "roofline": {"bound": "mfma", "achieved": achieved, "peak": PEAK_TFLOPS_FP32_MFMA,
                         "unit": "TFLOP/s", "frac": achieved / PEAK_TFLOPS_FP32_MFMA},
            "other_precision": {"precision": "f16x3", "value": IMAGE * IMAGE * SAMPLES / dt_h,
                                "ms_per_step": dt_h * 1e3, "ms_per_step_spread": ms_h, "kernel_ms": kernel_ms_h,
                                "roofline": {"bound": "mfma", "achieved": achieved_h, "peak": PEAK_TFLOPS_F16_MFMA,
                                             "unit": "TFLOP/s", "frac": achieved_h / PEAK_TFLOPS_F16_MFMA,
                                             "executed_frac": 3 * achieved_h / PEAK_TFLOPS_F16_MFMA}}}


def baseline_configs(dev):
    """The other BASELINE.json configurations and the weights-x3 point of SURVEY.md section 8(d), fp32
    arithmetic, a few steps each, so that the driver's record carries them (one GPU):
      C2 100x100x64 frame; C3 400x400, 64 coarse + 128 fine (hierarchical: coarse render, inverse-CDF
      resample, fine render of the sorted union); C4 800x800x192 whole and one of its eight 100-row
      shards; the headline frame with every Linear weight x3 (sharper densities: same cost by design).
    TFLOP/s = evaluated samples x 601,088 / wall time per step (synchronised)."""
    from nerf_amd import NeRF, _lib
    cam_o, cam_r = look_at(CAMERA)
    cam_o, cam_r = cam_o.to(dev), cam_r.to(dev)

    last = {}

    def timed(fn, steps, warmup=1):
        with torch.no_grad():
            for _ in range(warmup):
                fn()
            torch.cuda.synchronize(dev)
            _lib.timing(True)
            _lib.timing_read(reset=True)
            last["spread"] = spread(timed_loops(dev, fn, steps))
            kernel_ms, launches = _lib.timing_read(reset=True)
            _lib.timing(False)
        return last["spread"]["median"] * 1e-3, kernel_ms, launches // (steps * REPEATS)

    def entry(workload, dt, nominal, evaluated, steps, kernel_ms, launches, flop_per_sample=FLOP_PER_SAMPLE):
        tf = evaluated * flop_per_sample / dt / 1e12
        return {"workload": workload, "steps": steps, "ms_per_step": dt * 1e3, "ms_per_step_spread": last["spread"],
                "ray_samples_per_s": nominal / dt,
                "evaluated_samples": evaluated, "tflops": tf, "frac_of_fp32_mfma_peak": tf / PEAK_TFLOPS_FP32_MFMA,
                "render_launches_per_step": launches, "avg_render_kernel_ms": kernel_ms}

    def model_for(focal, scale=1.0, **shape):
        torch.manual_seed(0)
        m = NeRF(focal_length=focal, **shape)
        if scale != 1.0:
            with torch.no_grad():
                for slot in (0, 3, 6, 9, 12, 15):
                    m.prediction_heads[slot].weight.mul_(scale)
        return m.to(dev)

    out = {}
    m = model_for(112.0)
    dt, k, n = timed(lambda: m.render_image(cam_o, cam_r, 100, 100, 112.0, 64), steps=SHORT_STEPS, warmup=3)
    out["C2"] = entry("100x100 frame, 64 samples/ray, one launch", dt, 100 * 100 * 64, 100 * 100 * 63, SHORT_STEPS, k, n)
    m = model_for(448.0)
    dt, k, n = timed(lambda: m.render_image_hierarchical(cam_o, cam_r, 400, 400, 448.0, 64, 128), steps=FRAME_STEPS)
    out["C3"] = entry("400x400 frame, 64 coarse + 128 fine samples/ray (coarse render, inverse-CDF resample, "
                      "fine render of the 192-fencepost union); parity unpinned (no reference code)",
                      dt, 400 * 400 * (64 + 192), 400 * 400 * (63 + 191), FRAME_STEPS, k, n)
    m = model_for(FOCAL)
    dt, k, n = timed(lambda: m.render_image(cam_o, cam_r, IMAGE, IMAGE, FOCAL, 192), steps=FRAME_STEPS)
    out["C4"] = entry("800x800 frame, 192 samples/ray, one GPU", dt, IMAGE * IMAGE * 192, IMAGE * IMAGE * 191, FRAME_STEPS, k, n)
    dt, k, n = timed(lambda: m.render_image(cam_o, cam_r, IMAGE, IMAGE, FOCAL, 192, row_begin=300, row_end=400), steps=FRAME_STEPS)
    out["C4_shard"] = entry("rows 300..399 of the 800x800x192 frame: the share of one of 8 GPUs (no collective)",
                            dt, 100 * IMAGE * 192, 100 * IMAGE * 191, FRAME_STEPS, k, n)
    m = model_for(FOCAL, scale=3.0)
    dt, k, n = timed(lambda: m.render_image(cam_o, cam_r, IMAGE, IMAGE, FOCAL, SAMPLES), steps=FRAME_STEPS)
    out["headline_weights_x3"] = entry("the headline 800x800x128 frame with every Linear weight x3 (early "
                                       "saturation: the kernel has no early-out, cost must not change)",
                                       dt, IMAGE * IMAGE * SAMPLES, IMAGE * IMAGE * (SAMPLES - 1), FRAME_STEPS, k, n)
    # narrow networks at their own cost (nerf/model.py:471-475: hidden_size / encoding_size are constructor keywords):
    # the headline frame through the kernels instantiated for 8 and 4 register tiles per sample; algorithmic FLOP =
    # 2 (3 enc H + 4 H^2 + 54 H) per evaluated sample, against the same fp32 MFMA peak
    for name, hidden, enc in (("narrow_hidden128", 128, 32), ("narrow_hidden64_enc16", 64, 16)):
        m = model_for(FOCAL, hidden_size=hidden, encoding_size=enc)
        flop = 2 * (3 * enc * hidden + 4 * hidden * hidden + 54 * hidden)
        dt, k, n = timed(lambda: m.render_image(cam_o, cam_r, IMAGE, IMAGE, FOCAL, SAMPLES), steps=FRAME_STEPS)
        out[name] = entry(f"the headline 800x800x128 frame, hidden_size={hidden}, encoding_size={enc}: the fp32 kernel "
                          f"instantiated at {16 if hidden > 128 else (8 if hidden > 64 else 4)} register tiles per sample "
                          f"(not zero-padded to 256); {flop} FLOP per sample", dt, IMAGE * IMAGE * SAMPLES,
                          IMAGE * IMAGE * (SAMPLES - 1), FRAME_STEPS, k, n, flop_per_sample=flop)
        out[name]["flop_per_sample"] = flop
    return out


def legacy_train_step_timing(dev, rays=4096, samples=64, steps=SHORT_STEPS, warmup=3, train_precision="fp32"):
    """One optimiser step of the notebook's training loop (examples/example.ipynb cell 8) on the LEGACY 8 x 256
    network, the one BASELINE config 5 / the PSNR target were published on: training forward + HIP backward
    (44 gradients) + fused Adam, 4096 rays x 64 samples, stratified draws, noise std 1.  fp32 MFMA forward and
    data gradient, bf16-triple weight gradient (exact-fp32 products throughout).  Parity unpinned."""
    from nerf_amd.legacy import LegacyNeRF8x256, FLOP_PER_SAMPLE as LEGACY_FLOP
    from nerf_amd.optim import Adam
    from nerf_amd.loss import mse_and_grad
    torch.manual_seed(0)
    model = LegacyNeRF8x256().to(dev)
    model.train_precision = train_precision
    opt = Adam(model.parameters(), lr=1e-4)
    o = torch.randn(rays, 3, device=dev) * 0.5
    d = torch.randn(rays, 3, device=dev)
    target = torch.rand(rays, 3, device=dev)

    def step():
        pixels = model.render_rays(o, d, 2.0, 6.0, samples, randomly_sample=True, density_noise_std=1.0)
        loss, grad = mse_and_grad(pixels, target)        # the Trainer's step: loss + gradient in one launch
        opt.zero_grad()
        pixels.backward(grad)
        opt.step()

    for _ in range(warmup):
        step()
    ms = spread(timed_loops(dev, step, steps))
    kernels = kernel_split(dev, step)
    dt = ms["median"] * 1e-3
    return {"workload": f"legacy 8x256 network, {rays} rays x {samples} samples, forward + backward + Adam",
            "ms_per_step": ms["median"], "ms_per_step_spread": ms, "steps_per_loop": steps, "kernels_ms": kernels,
            "ray_samples_per_s": rays * samples / dt,
            "tflops_fwd_dgrad_wgrad": 3 * LEGACY_FLOP * rays * samples / dt / 1e12,
            "arithmetic": ("forward, data gradient and weight gradient on f16 pairs (three f16 MFMAs per product); fp32 "
                           "accumulate" if train_precision == "f16x3" else
                           "forward and data gradient on fp32 MFMA, weight gradient on bf16 triples; fp32 accumulate")}


def profiled_traffic(precision):
    """HBM bytes per launch of the render kernel from the committed rocprofv3 PMC passes of this
    same command (profiles/*_pmc_summary.json, the newest one of this precision; FETCH_SIZE/WRITE_SIZE
    are KiB, FETCH_SIZE doubled per the gfx950 correction of MI355X_MICROARCH.md).  PMC counters
    cannot be read from inside the timed process, so this is the last profiled value, or None."""
    import glob
    best = None
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_summary.json"))):
        name = os.path.basename(path)
        if ("f16x3" in name) != (precision == "f16x3") or any(k in name for k in ("train", "bwd", "wgrad")):
            continue
        try:
            with open(path) as f:
                d = json.load(f)
            best = ((2.0 * d["FETCH_SIZE"] + d["WRITE_SIZE"]) * 1024.0, os.path.relpath(path, ROOT))
        except (OSError, KeyError, ValueError):
            continue
    return best


def roofline(precision, rays, kernel_ms, launches, with_traffic):
    evaluated = rays * (SAMPLES - 1)
    info = PRECISIONS[precision]
    achieved = evaluated * FLOP_PER_SAMPLE / (kernel_ms * 1e-3) / 1e12 if kernel_ms > 0 else None
    traffic = profiled_traffic(precision) if with_traffic else None
    return {
        "bound": "mfma",
        "achieved": achieved,
        "peak": info["peak"],
        "unit": "TFLOP/s",
        "frac": achieved / info["peak"] if achieved else None,
        "traffic": traffic[0] if traffic else None,
        "traffic_unit": "bytes/launch",
        "traffic_source": traffic[1] if traffic else None,
        "algorithmic_bytes": rays * (12 + 200) + 48,
        "kernel": "nerf_render_fwd_kernel",
        "kernel_ms": kernel_ms,
        "launches_timed": launches,
        "flop_per_launch": evaluated * FLOP_PER_SAMPLE,
        "executed_mfma_flop_per_launch": evaluated * FLOP_PER_SAMPLE * info["mfma_per_product"],
        "executed_frac": achieved * info["mfma_per_product"] / info["peak"] if achieved else None,
        "peak_note": info["peak_note"],
    }


def shard_rows(rank, world):
    """Row block of rank `rank` when `world` GPUs split the bench frame: the product's partition
    (nerf_amd.parallel.shard_rows; blocks differ by at most one row and cover the frame exactly)."""
    from nerf_amd.parallel import shard_rows as product_shard_rows
    return product_shard_rows(IMAGE, rank, world)


def free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def self_launch(gpus, argv):
    """``python bench.py --gpus N`` outside torch.distributed.run: start the N ranks as a child process of this
    one, which has made no GPU call (and makes none afterwards), with the driver's own launcher command line;
    the child's stdout / stderr are inherited, so rank 0's JSON line is this command's output.  Returns the
    child's exit code."""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    env.setdefault("OMP_NUM_THREADS", "1")
    print(f"[bench] --gpus {gpus} without WORLD_SIZE: starting the ranks: {' '.join(cmd)}", file=sys.stderr, flush=True)
    return subprocess.run(cmd, env=env).returncode


def dry_run(args, rank, world):
    """The N > 1 line without a GPU: rendezvous over gloo, this rank's row block of the frame and its share of the
    config-5 batch, one flat all-reduce of a gradient-sized buffer through the product's FlatGradientAllReduce,
    MAX over ranks of a clock — every host-side step of the multi-GPU path, none of the kernels.  Rank 0 prints
    one JSON line (value null: nothing was measured)."""
    import torch.distributed as dist
    from nerf_amd.parallel import FlatGradientAllReduce, shard_items
    if world > 1:
        dist.init_process_group("gloo")
    rows = shard_rows(rank, world)
    batch = shard_items(4096, rank, world)
    weak = shard_items(4096 * world, rank, world)        # the weak form of the training entry: 4096 rays per rank
    params = [torch.nn.Parameter(torch.zeros(304438))]
    params[0].grad = torch.full((304438,), float(rank + 1))
    if world > 1:
        FlatGradientAllReduce(params)(None, (batch[1] - batch[0]) / 4096.0)
        mine = torch.tensor([rows[0], rows[1], batch[0], batch[1]], dtype=torch.int64)
        parts = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(parts, mine)
        t = torch.tensor([float(rank)], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        assert int(t.item()) == world - 1
    else:
        parts = [torch.tensor([rows[0], rows[1], batch[0], batch[1]])]
    want = sum((r + 1) * (shard_items(4096, r, world)[1] - shard_items(4096, r, world)[0]) / 4096.0 for r in range(world))
    reduced_ok = world == 1 or bool((params[0].grad - want).abs().max() < 1e-5)
    if rank == 0:
        blocks = [[int(v) for v in p.tolist()] for p in parts]
        print(json.dumps({
            "metric": "ray-samples/sec at 800x800x128", "value": None, "unit": "ray-samples/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "dry_run": True, "scaling": args.scaling,
            "config": {"workload": "dry run: launch, rendezvous and partitions only; no GPU call, nothing measured",
                       "rays_per_gpu": (rows[1] - rows[0]) * IMAGE, "rendezvous_backend": "gloo" if world > 1 else None,
                       "row_blocks": [b[:2] for b in blocks], "collectives": "none"},
            "train_step_dp": {"scaling": "strong", "rays_per_rank": batch[1] - batch[0], "global_batch": 4096,
                              "batch_blocks": [b[2:] for b in blocks], "gradient_bytes": 304438 * 4,
                              "flat_all_reduce_matches_weighted_sum": reduced_ok},
            "train_step_dp_weak": {"scaling": "weak", "rays_per_rank": weak[1] - weak[0], "global_batch": 4096 * world,
                                   "batch_blocks": [list(shard_items(4096 * world, r, world)) for r in range(world)],
                                   "gradient_bytes": 304438 * 4}}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def scaling_projection(model, dev, whole_ms, steps=3):
    """ONE-GPU PROJECTION of the strong-scaling line (no multi-GPU hardware is reachable from this bench): for
    N = 2, 4, 8 every one of the N row blocks of the frame is rendered on this GPU and timed; the projected
    speed-up is the whole frame's time / the SLOWEST block's time — what N GPUs would reach if nothing but the
    kernels mattered (inference has no collective; launch and barrier costs are not in it).  A projection, not
    a measurement of N GPUs, and labelled so."""
    cam_o, cam_r = look_at(CAMERA)
    cam_o, cam_r = cam_o.to(dev), cam_r.to(dev)
    out = {"kind": "projection from ONE GPU: whole-frame ms / slowest row-block ms; not a multi-GPU measurement",
           "whole_frame_ms": whole_ms, "steps_per_block": steps}
    with torch.no_grad():
        for world in (2, 4, 8):
            worst = 0.0
            for r in range(world):
                rows = shard_rows(r, world)
                model.render_image(cam_o, cam_r, IMAGE, IMAGE, FOCAL, SAMPLES, row_begin=rows[0], row_end=rows[1])
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(steps):
                    model.render_image(cam_o, cam_r, IMAGE, IMAGE, FOCAL, SAMPLES, row_begin=rows[0], row_end=rows[1])
                torch.cuda.synchronize(dev)
                worst = max(worst, (time.perf_counter() - t0) / steps * 1e3)
            out[str(world)] = {"slowest_block_ms": worst, "projected_speedup": whole_ms / worst,
                               "projected_efficiency": whole_ms / worst / world}
    return out


DUMP_SEG_PIXELS = 131072           # segmentation pixels --dump-outputs keeps of a whole frame (26 MB of 50 classes)
DUMP_SEED = 0


def dump_outputs(out_dir, image, segmentation, rank=None):
    """--dump-outputs: the last timed step's results as float32 .npy files — `image` whole ([1, rows, W, 3], 7.7 MB
    for the frame) and `segmentation` ([1, rows, W, 50], 128 MB for the frame) as the rows of a fixed, seeded sample
    of its pixels (`segmentation_sample`, [n, 50], pixel indices sorted; n in proportion to the rows rendered).  The
    inputs (seed-0 weights, fixed pose, deterministic fenceposts) are the same from run to run, so two builds can be
    compared file by file.  With several ranks every rank writes its own row block, names suffixed _rank<r>."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    suffix = "" if rank is None else f"_rank{rank}"
    pixels = segmentation.shape[0] * segmentation.shape[1] * segmentation.shape[2]
    n = min(pixels, max(1, DUMP_SEG_PIXELS * pixels // (IMAGE * IMAGE)))
    pick = np.sort(np.random.default_rng(DUMP_SEED).choice(pixels, size=n, replace=False))
    seg = segmentation.reshape(pixels, segmentation.shape[-1])[torch.from_numpy(pick).to(segmentation.device)]
    for name, t in (("image", image), ("segmentation_sample", seg)):
        np.save(os.path.join(out_dir, name + suffix + ".npy"), t.detach().float().cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scaling", choices=("weak", "strong"), default="strong",
                    help="strong (default): the GPUs split the rows of one frame; weak: one frame per GPU")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--allow-gloo", action="store_true",
                    help="N > 1: if RCCL cannot initialise, rendezvous over gloo instead of failing "
                         "(the line then says rendezvous_backend gloo: no RCCL credit)")
    ap.add_argument("--precision", choices=("fp32", "f16x3"), default=os.environ.get("NERF_BENCH_PRECISION", "fp32"))
    ap.add_argument("--dry-run", action="store_true",
                    help="launch, rendezvous (gloo) and partitions only: no GPU call, nothing measured")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what the last timed step returned as DIR/<name>.npy "
                         "(float32): the image, and a fixed seeded sample of the segmentation's pixels")
    args = ap.parse_args()
    if args.gpus < 1:
        ap.error("--gpus must be at least 1")
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # no launcher around us: become it (before any GPU call; a child process, never an exec)
        raise SystemExit(self_launch(args.gpus, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world != args.gpus:
        print(f"[bench] --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks: start bench.py with "
              f"--nproc-per-node {args.gpus}, or without a launcher (it starts its own ranks)", file=sys.stderr)
        raise SystemExit(2)
    if args.dry_run:
        return dry_run(args, rank, world)
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    distributed = world > 1
    backend = None
    device_index, shared_device = local_rank, False
    if distributed:
        import torch.distributed as dist
        visible = torch.cuda.device_count()
        if world > visible:
            # more ranks than GPUs on this (one) node: only as a REHEARSAL of this code path — the driver's own
            # command line on a one-GPU box.  The ranks share devices, RCCL cannot carry that, the line says so.
            if not args.allow_gloo:
                print(f"[bench] {world} ranks but {visible} GPU(s) visible: refusing to measure; --allow-gloo "
                      "rehearses the path with ranks sharing a device", file=sys.stderr)
                raise SystemExit(2)
            device_index, shared_device = local_rank % max(visible, 1), True
        torch.cuda.set_device(device_index)
        try:                                      # RCCL over xGMI; only barriers + one scalar reduce use it
            if shared_device:
                raise RuntimeError("ranks share a device (rehearsal)")
            dist.init_process_group("nccl", device_id=torch.device("cuda", device_index))
            backend = "nccl"
        except Exception as exc:
            if not args.allow_gloo:               # a multi-GPU line without RCCL is not the measurement asked for
                print(f"[bench] RCCL (backend nccl) failed to initialise: {exc}\n[bench] refusing to measure "
                      "without it; pass --allow-gloo to rendezvous over gloo instead", file=sys.stderr)
                raise
            print(f"[bench] nccl init failed ({exc}); --allow-gloo: barriers over gloo", file=sys.stderr)
            dist.init_process_group("gloo")
            backend = "gloo"
    dev = torch.device("cuda", device_index)

    from nerf_amd import NeRF, _lib
    torch.manual_seed(0)
    model = NeRF(focal_length=FOCAL).to(dev)         # default init, seed 0, on every rank
    model.precision = args.precision

    import math

    def workload(scaling):
        """(pose, row block) of this rank: its row block of the one frame (strong), or a frame of
        its own from a pose on the same circle (weak)."""
        if scaling == "weak":
            ang = 2.0 * math.pi * rank / max(world, 1)
            r_xy = math.hypot(CAMERA[0], CAMERA[1])
            return (r_xy * math.sin(ang), -r_xy * math.cos(ang), CAMERA[2]), (0, IMAGE)
        return CAMERA, shard_rows(rank, world)

    def fence():
        if distributed:
            dist.barrier()
        torch.cuda.synchronize(dev)

    def measure(scaling, steps, warmup, keep_outputs=False):
        """W untimed + K timed steps between barrier + synchronize pairs; MAX over ranks.  `keep_outputs`: the
        (image, segmentation) of the last timed step go into the result as "outputs"."""
        pose, rows = workload(scaling)
        cam_o, cam_r = look_at(pose)
        cam_o, cam_r = cam_o.to(dev), cam_r.to(dev)

        def step():
            with torch.no_grad():
                return model.render_image(cam_o, cam_r, IMAGE, IMAGE, FOCAL, SAMPLES,
                                          row_begin=rows[0], row_end=rows[1])

        for _ in range(warmup):
            step()
        fence()
        _lib.timing(True)
        _lib.timing_read(reset=True)
        t0 = time.perf_counter()
        for _ in range(steps):
            out = step()
        fence()
        dt = time.perf_counter() - t0
        kernel_ms, launches = _lib.timing_read(reset=True)
        _lib.timing(False)
        assert torch.isfinite(out[0]).all()
        t = torch.tensor([dt], dtype=torch.float64, device=dev if backend != "gloo" else "cpu")
        if distributed:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        rays_rank = (rows[1] - rows[0]) * IMAGE
        total_rays = rays_rank * world if scaling == "weak" else IMAGE * IMAGE
        return {"elapsed": float(t.item()), "kernel_ms": kernel_ms, "launches": launches,
                "rays_per_rank": rays_rank, "value": total_rays * SAMPLES * steps / float(t.item()),
                **({"outputs": out} if keep_outputs else {})}

    m = measure(args.scaling, args.steps, args.warmup, keep_outputs=args.dump_outputs is not None)
    if args.dump_outputs is not None:
        dump_outputs(args.dump_outputs, *m.pop("outputs"), rank=rank if world > 1 else None)
    weak = dp = None
    if distributed and args.scaling == "strong":
        weak = measure("weak", args.steps, args.warmup)
    dp_weak = None
    if distributed:
        dp = train_step_dp(dev, rank, world, backend, max(args.steps, 10), args.warmup, fence)
        dp_weak = train_step_dp(dev, rank, world, backend, max(args.steps, 10), args.warmup, fence, scaling="weak")

    if rank == 0:
        line = {
            "metric": "ray-samples/sec at 800x800x128",
            "value": m["value"],
            "unit": "ray-samples/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": m["elapsed"] / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": args.scaling,
            "vs_baseline": None,
            "dtype": PRECISIONS[args.precision]["dtype"],
            "data": "synthetic",
            "config": {
                "workload": "NeRF.render_image 800x800, 128 samples/ray (127 evaluated), RGB + 50-class "
                            "segmentation, rays generated in-kernel, default-init weights seed 0",
                "precision": args.precision,
                "rays_per_gpu": m["rays_per_rank"],
                "frames": world if args.scaling == "weak" else 1,
                "sharding": ("one frame per GPU" if args.scaling == "weak"
                             else f"{world} row blocks of one frame" if world > 1 else "one frame, one GPU"),
                "collectives": "none",
                "rendezvous_backend": backend,
                **({"rehearsal": "ranks share a device: not a scaling measurement"} if shared_device else {}),
            },
            "roofline": roofline(args.precision, m["rays_per_rank"], m["kernel_ms"], m["launches"],
                                 world == 1),
        }
        if dp is not None:
            line["train_step_dp"] = dp
            line["train_step_dp_weak"] = dp_weak
        if weak is not None:
            line["weak_scaling"] = {"value": weak["value"], "unit": "ray-samples/s",
                                    "ms_per_step": weak["elapsed"] / args.steps * 1e3,
                                    "steps": args.steps, "frames": world,
                                    "sharding": "one frame per GPU",
                                    "kernel_ms": weak["kernel_ms"]}
        if world == 1 and not args.no_cpu_baseline:
            # the other arithmetic of the same kernel: same frame, same run, same step counts
            other = "fp32" if args.precision == "f16x3" else "f16x3"
            model.precision = other
            o = measure(args.scaling, args.steps, args.warmup)
            model.precision = args.precision
            line["other_precision"] = {
                "precision": other, "dtype": PRECISIONS[other]["dtype"],
                "value": o["value"], "unit": "ray-samples/s",
                "steps": args.steps, "warmup": args.warmup, "ms_per_step": o["elapsed"] / args.steps * 1e3,
                "roofline": roofline(other, o["rays_per_rank"], o["kernel_ms"], o["launches"], True),
            }
            line["train_step"] = train_step_timing(dev)
            line["train_step_f16x3"] = train_step_timing(dev, train_precision="f16x3")
            line["train_step_hidden128"] = train_step_timing(dev, hidden=128)
            line["train_step_hidden128_f16x3"] = train_step_timing(dev, hidden=128, train_precision="f16x3")
            # hidden_size <= 64: forward and data gradient at 4 register tiles, the weight gradient at 8
            line["train_step_hidden64_enc16"] = train_step_timing(dev, hidden=64, enc=16)
            line["train_step_512_graph"] = small_batch_step_timing(dev)
            line["legacy_network"] = legacy_workload_timing(dev)
            line["legacy_train_step"] = legacy_train_step_timing(dev)
            line["legacy_train_step_f16x3"] = legacy_train_step_timing(dev, train_precision="f16x3")
            line["configs"] = baseline_configs(dev)
            line["scaling_projection"] = scaling_projection(model, dev, m["elapsed"] / args.steps * 1e3)
            line["cpu_baseline"] = cpu_baseline()
        print(json.dumps(line), flush=True)
    if distributed:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
