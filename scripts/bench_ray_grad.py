"""Timing of the ray gradient (nerf_hip_render_backward_rays) at 4096 rays x 64 fenceposts, hidden 256 and 64, both
training arithmetics: (a) the parameter-only training step, (b) the same step with the rays requiring grad, (c) the
frozen-network pose step (forward + compositing backward + data gradient + ray kernel).  Wall time per step and the
per-kernel split from the library's tagged HIP-event timing (nerf_hip_timing_read_tagged)."""
import os, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nerf_amd import NeRF, _lib
dev = torch.device('cuda:0')
n, S = int(sys.argv[1]) if len(sys.argv) > 1 else 4096, 64
K = 10


def run(model, o, d, rays_grad):
    og, dg = o.clone().requires_grad_(rays_grad), d.clone().requires_grad_(rays_grad)
    rgb, _ = model.render_rays(og, dg, S, randomly_sample=True, density_noise_std=1.0)
    (rgb * rgb).mean().backward()


def timed(model, o, d, rays_grad):
    for _ in range(3):
        run(model, o, d, rays_grad)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(K):
        run(model, o, d, rays_grad)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / K
    _lib.timing(True)
    _lib.timing_read_tagged(reset=True)
    for _ in range(K):
        run(model, o, d, rays_grad)
    tags = _lib.timing_read_tagged(reset=True)
    _lib.timing(False)
    return wall, tags


for hidden in (256, 64):
    for precision in ("fp32", "f16x3"):
        torch.manual_seed(0)
        model = NeRF(hidden_size=hidden).to(dev)
        model.train_precision = precision
        o = torch.randn(n, 3, device=dev)
        d = torch.randn(n, 3, device=dev)
        for name, rays_grad, frozen in (("(a) parameters", False, False), ("(b) parameters + rays", True, False),
                                        ("(c) pose, frozen network", True, True)):
            for p in model.parameters():
                p.requires_grad_(not frozen)
                p.grad = None
            wall, tags = timed(model, o, d, rays_grad)
            split = "  ".join(f"{k} {ms:.3f}" for k, (ms, _) in tags.items())
            print(f"hidden {hidden} {precision:5s} {name:26s}: {wall * 1e3:7.2f} ms/step | per kernel (ms): {split}")
