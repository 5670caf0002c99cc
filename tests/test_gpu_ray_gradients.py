"""GPU tests of the ray gradient (nerf_hip_render_backward_rays): dL/d rays_o, dL/d rays_d through NeRF.render_rays,
NeRF.forward and NeRF.render_image against the oracle's autograd, which is differentiable in the rays as the
reference's is.  Gate-aware like tests/gate_aware.py: the oracle differentiates with the ReLU gates the kernel ran
with, and each ray-gradient tensor must lie within 5e-6 + 4 x (the fp32 oracle's own distance from fp64) of the nearer
of the two oracles, relative to its largest element; the flipped gates are counted and reported."""
import pytest
import torch

import gate_aware
import workspace_mirror as W
from conftest import golden_params
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu
CFG = O.default_config()
BOUND = 5e-6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(params=["fp32", "f16x3"])
def precision(request):
    return request.param


def make_model(dev, params, precision, hidden=256, encoding=32):
    from nerf_amd import NeRF
    model = NeRF(hidden_size=hidden, encoding_size=encoding)
    model.load_state_dict(params)
    model.train_precision = model.precision = precision
    model.keep_workspace = True
    return model.to(dev)


def net_params(hidden, encoding, seed=0):
    if hidden == 256 and encoding == 32:
        return golden_params(2.0)
    cfg = dict(CFG, hidden_size=hidden, encoding_size=encoding)
    params = O.init_params(seed, cfg)
    params["prediction_heads.15.bias"][0] += 0.5          # some density on every ray: the gradient is not trivially 0
    return params


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


def oracle_ray_grads(loss_fn, o, d, dtype):
    """loss_fn(o, d, dtype) -> scalar; (dL/do, dL/dd) of the oracle in ``dtype``."""
    oo = o.to(dtype).clone().requires_grad_(True)
    dd = d.to(dtype).clone().requires_grad_(True)
    loss_fn(oo, dd, dtype).backward()
    return oo.grad, dd.grad


def check_rays(got, loss_fn, o, d, tag, bound=BOUND):
    """got = (d_rays_o, d_rays_d) of the kernel; loss_fn evaluates the oracle on the kernel's gates."""
    r32 = oracle_ray_grads(loss_fn, o, d, torch.float32)
    r64 = oracle_ray_grads(loss_fn, o, d, torch.float64)
    lines, bad = [], []
    for name, g, a, b in zip(("rays_o", "rays_d"), got, r32, r64):
        assert float(b.abs().max()) > 0, name
        floor = rel_err(a, b)
        e64, e32 = rel_err(g, b), rel_err(g, a)
        lines.append(f"[{tag}] d {name}: vs fp64 {e64:.2e} vs fp32 {e32:.2e} floor {floor:.2e}")
        if min(e64, e32) > bound + 4.0 * floor:
            bad.append(name)
    print("\n".join(lines))
    assert not bad, "\n".join(lines)


def count_flips(params, cfg, o, d, num_samples, gates, **kw):
    own = []
    with torch.no_grad():
        O.render_rays(params, cfg, o, d, num_samples, record=own, **kw)
    return sum(int((a != b).sum()) for a, b in zip(own, gates)), sum(int(g.numel()) for g in gates)


def render_t(params, cfg, o, d, t, gates):
    """O.render_rays on explicit fenceposts, with forced gates (the Philox path's reference)."""
    means, covs, h, density, color, seg = O.field(params, cfg, o, d, t, gates=gates[:5])
    weights = O.composite_weights(means, density, gates[5])
    rgb = (weights * torch.sigmoid(color)).sum(dim=-2)
    seg_out = (torch.log(weights + 1e-10) + torch.log_softmax(seg, dim=-1)).logsumexp(dim=-2)
    return rgb, seg_out


CASES = [  # n_rays, num_samples, hidden, encoding_size, draws
    (5, 9, 256, 32, "det"), (64, 33, 128, 16, "captured"), (130, 64, 64, 32, "det"),
    (64, 33, 64, 16, "captured"), (130, 64, 256, 32, "captured"), (5, 9, 128, 32, "captured"),
    (64, 33, 256, 16, "det"), (130, 64, 128, 32, "det")]


@pytest.mark.parametrize("n_rays,num_samples,hidden,encoding,draws", CASES)
@pytest.mark.parametrize("with_seg", [False, True])
def test_render_rays_ray_gradients(dev, precision, n_rays, num_samples, hidden, encoding, draws, with_seg):
    params = net_params(hidden, encoding)
    cfg = dict(CFG, hidden_size=hidden, encoding_size=encoding)
    gen = torch.Generator().manual_seed(n_rays + num_samples + hidden)
    o = torch.randn(n_rays, 3, generator=gen)
    d = torch.randn(n_rays, 3, generator=gen)                       # |d| != 1
    u = noise = None
    std = 0.0
    if draws == "captured":
        u = torch.rand(n_rays, num_samples, generator=gen)
        noise = torch.randn(n_rays, num_samples - 1, 1, generator=gen)
        std = 1.0
    w_rgb = torch.randn(n_rays, 3, generator=gen)
    w_seg = torch.randn(n_rays, 50, generator=gen) * 0.1
    if with_seg:
        w_seg = w_seg * gate_aware.rays_with_weight(params, cfg, o, d, num_samples, u, noise, std)[:, None]
    else:
        w_seg = w_seg * 0.0

    model = make_model(dev, params, precision, hidden, encoding)
    og = o.to(dev).requires_grad_(True)
    dg = d.to(dev).requires_grad_(True)
    kw = {} if u is None else dict(randomly_sample=True, u=u.to(dev), noise=noise.to(dev), density_noise_std=std)
    rgb, seg = model.render_rays(og, dg, num_samples, **kw)
    loss = (rgb[:, 0] * w_rgb.to(dev)).sum() + (seg[:, 0] * w_seg.to(dev)).sum()
    loss.backward()
    assert og.grad is not None and dg.grad is not None
    gates = gate_aware.kernel_gates(model, params, n_rays, num_samples)

    def loss_fn(oo, dd, dtype):
        p = {k: v.to(dtype) for k, v in params.items()}
        c = lambda t: None if t is None else t.to(dtype)
        r, s = O.render_rays(p, cfg, oo, dd, num_samples, u=c(u), noise=c(noise), density_noise_std=std, gates=gates)
        return (r * w_rgb.to(dtype)).sum() + (s * w_seg.to(dtype)).sum()

    flips, total = count_flips(params, cfg, o, d, num_samples, gates, u=u, noise=noise, density_noise_std=std)
    print(f"{flips} of {total} gates differ from the oracle's own")
    assert flips <= max(gate_aware.FLIP_BOUND * total, 2)
    check_rays((og.grad, dg.grad), loss_fn, o, d, f"{precision} {n_rays}x{num_samples} h{hidden} e{encoding} {draws} "
               f"seg={with_seg}")


def test_philox_fenceposts(dev, precision):
    params = golden_params(2.0)
    n_rays, num_samples = 64, 33
    gen = torch.Generator().manual_seed(7)
    o, d = torch.randn(n_rays, 3, generator=gen), torch.randn(n_rays, 3, generator=gen)
    w_rgb = torch.randn(n_rays, 3, generator=gen)
    model = make_model(dev, params, precision)
    model.rng = "philox"
    seed, offset = model._next_philox_state()
    counter = int(model._philox_device_counter(dev).item())
    t = model.fenceposts_used(o.to(dev), d.to(dev), num_samples, randomly_sample=True,
                              rng_state=(seed, offset + counter)).cpu()
    og, dg = o.to(dev).requires_grad_(True), d.to(dev).requires_grad_(True)
    rgb, _ = model.render_rays(og, dg, num_samples, randomly_sample=True)
    (rgb[:, 0] * w_rgb.to(dev)).sum().backward()
    gates = gate_aware.kernel_gates(model, params, n_rays, num_samples)

    def loss_fn(oo, dd, dtype):
        p = {k: v.to(dtype) for k, v in params.items()}
        return (render_t(p, CFG, oo, dd, t.to(dtype), gates)[0] * w_rgb.to(dtype)).sum()

    check_rays((og.grad, dg.grad), loss_fn, o, d, f"{precision} philox")


def field_case(dev, precision, w_density, w_color, w_seg, w_mean, hidden=256, encoding=32):
    params = net_params(hidden, encoding)
    cfg = dict(CFG, hidden_size=hidden, encoding_size=encoding)
    n_rays, num_samples = 37, 20
    gen = torch.Generator().manual_seed(11)
    o, d = torch.randn(n_rays, 3, generator=gen), torch.randn(n_rays, 3, generator=gen)
    t = torch.sort(torch.rand(n_rays, num_samples, generator=gen) * 40 + 0.1, dim=-1).values
    P = num_samples - 1
    w = [torch.randn(n_rays, P, k, generator=gen) * s for k, s in ((1, w_density), (3, w_color), (50, w_seg), (3, w_mean))]
    model = make_model(dev, params, precision, hidden, encoding)
    og, dg = o.to(dev).requires_grad_(True), d.to(dev).requires_grad_(True)
    mean, dens, col, seg = model(og, dg, t.to(dev))
    assert mean.requires_grad
    loss = sum((x * wi.to(dev)).sum() for x, wi in zip((dens, col, seg, mean), w))
    loss.backward()
    gates = W.saved_gates(model.last_workspace, params, n_rays, num_samples)

    def loss_fn(oo, dd, dtype):
        p = {k: v.to(dtype) for k, v in params.items()}
        means, _, _, de, co, se = O.field(p, cfg, oo, dd, t.to(dtype), gates=gates)
        return sum((x * wi.to(dtype)).sum() for x, wi in zip((de, co, se, means), w))

    return model, params, (o, d, t, w), (og.grad, dg.grad), loss_fn


def test_forward_ray_gradients(dev, precision):
    _, _, (o, d, _, _), got, loss_fn = field_case(dev, precision, 1.0, 1.0, 0.1, 1.0)
    check_rays(got, loss_fn, o, d, f"{precision} forward()")


def test_forward_mean_only(dev, precision):
    """Only `mean` reaches the loss: d rays_o = sum of d mean, d rays_d = sum of t_mean d mean (no network route)."""
    _, params, (o, d, t, w), (go, gd), _ = field_case(dev, precision, 0.0, 0.0, 0.0, 1.0)
    t0, t1 = t[:, :-1].double(), t[:, 1:].double()
    mu, hw = (t0 + t1) / 2, (t1 - t0) / 2
    t_mean = mu + (2 * mu * hw ** 2) / (3 * mu ** 2 + hw ** 2)
    wm = w[3].double()
    assert rel_err(go, wm.sum(dim=1)) <= 1e-6
    assert rel_err(gd, (t_mean[..., None] * wm).sum(dim=1)) <= 1e-6


def test_render_image_pose_gradients(dev, precision):
    params = golden_params(2.0)
    cam_o = torch.tensor([[0.0, -3.0, 2.6], [2.0, 2.0, 1.5]])
    cam_r = torch.cat([O.look_at_pose(c.tolist()) for c in cam_o])
    H, Wd, S, focal = 6, 5, 24, 6.2
    gen = torch.Generator().manual_seed(3)
    w_img = torch.randn(2, H, Wd, 3, generator=gen)
    model = make_model(dev, params, precision)
    for p in model.parameters():
        p.requires_grad_(False)
    co, cr = cam_o.to(dev).requires_grad_(True), cam_r.to(dev).requires_grad_(True)
    img, _ = model.render_image(co, cr, H, Wd, focal, S, max_chunk_size=64)       # one chunk: one workspace
    assert img.requires_grad
    (img * w_img.to(dev)).sum().backward()
    gates = gate_aware.kernel_gates(model, params, 2 * H * Wd, S)
    r32, r64 = [], []
    for dtype, out in ((torch.float32, r32), (torch.float64, r64)):
        p = {k: v.to(dtype) for k, v in params.items()}
        o_ = cam_o.to(dtype).clone().requires_grad_(True)
        r_ = cam_r.to(dtype).clone().requires_grad_(True)
        ro, rd = O.image_rays(o_, r_, H, Wd, focal)
        rgb, _ = O.render_rays(p, CFG, ro, rd, S, gates=gates)
        (rgb.reshape(2, H, Wd, 3) * w_img.to(dtype)).sum().backward()
        out += [o_.grad, r_.grad]
    for name, g, a, b in zip(("camera_o", "camera_r"), (co.grad, cr.grad), r32, r64):
        floor = rel_err(a, b)
        e = min(rel_err(g, a), rel_err(g, b))
        print(f"[{precision}] d {name}: {e:.2e} floor {floor:.2e}")
        assert e <= BOUND + 4.0 * floor, (name, e, floor)


def test_w0_zero_isolates_the_distance_route(dev, precision):
    params = golden_params(2.0)
    params["prediction_heads.0.weight"] = torch.zeros_like(params["prediction_heads.0.weight"])
    n_rays, num_samples = 40, 33
    gen = torch.Generator().manual_seed(5)
    o, d = torch.randn(n_rays, 3, generator=gen), torch.randn(n_rays, 3, generator=gen)
    w_rgb = torch.randn(n_rays, 3, generator=gen)
    model = make_model(dev, params, precision)
    og, dg = o.to(dev).requires_grad_(True), d.to(dev).requires_grad_(True)
    rgb, _ = model.render_rays(og, dg, num_samples)
    (rgb[:, 0] * w_rgb.to(dev)).sum().backward()
    assert torch.count_nonzero(og.grad) == 0
    assert torch.count_nonzero(dg.grad) > 0
    gates = gate_aware.kernel_gates(model, params, n_rays, num_samples)

    def loss_fn(oo, dd, dtype):
        p = {k: v.to(dtype) for k, v in params.items()}
        return (O.render_rays(p, CFG, oo, dd, num_samples, gates=gates)[0] * w_rgb.to(dtype)).sum()

    r64 = oracle_ray_grads(loss_fn, o, d, torch.float64)
    r32 = oracle_ray_grads(loss_fn, o, d, torch.float32)
    floor = rel_err(r32[1], r64[1])
    e = min(rel_err(dg.grad, r64[1]), rel_err(dg.grad, r32[1]))
    print(f"[{precision}] W0 = 0: d rays_d {e:.2e} floor {floor:.2e}")
    assert e <= BOUND + 4.0 * floor


def _step(model, o, d, num_samples, w_rgb, need_o=True, need_d=True, u=None):
    og = o.clone().requires_grad_(need_o)
    dg = d.clone().requires_grad_(need_d)
    kw = {} if u is None else dict(randomly_sample=True, u=u)
    rgb, seg = model.render_rays(og, dg, num_samples, **kw)
    ((rgb[:, 0] * w_rgb).sum() + seg[:, 0, :3].sum()).backward()
    return og.grad, dg.grad


def _small_batch(dev, n_rays=70, num_samples=40):
    gen = torch.Generator().manual_seed(9)
    o, d = torch.randn(n_rays, 3, generator=gen), torch.randn(n_rays, 3, generator=gen)
    u = torch.rand(n_rays, num_samples, generator=gen)
    w = torch.randn(n_rays, 3, generator=gen)
    return o.to(dev), d.to(dev), u.to(dev), w.to(dev), num_samples


def test_one_ray_input_and_determinism(dev, precision):
    model = make_model(dev, golden_params(2.0), precision)
    o, d, u, w, S = _small_batch(dev)
    go, gd = _step(model, o, d, S, w, u=u)
    go2, gd2 = _step(model, o, d, S, w, u=u)
    assert torch.equal(go, go2) and torch.equal(gd, gd2)                   # bitwise reproducible
    only_o = _step(model, o, d, S, w, need_d=False, u=u)
    only_d = _step(model, o, d, S, w, need_o=False, u=u)
    assert only_o[1] is None and torch.equal(only_o[0], go)
    assert only_d[0] is None and torch.equal(only_d[1], gd)


def test_parameter_gradients_unchanged_and_frozen_network(dev, precision):
    from nerf_amd import _lib
    model = make_model(dev, golden_params(2.0), precision)
    o, d, u, w, S = _small_batch(dev)
    # parameter-only step: no ray_gradient launch
    model.zero_grad(set_to_none=True)
    _lib.timing(True)
    try:
        _lib.timing_read_tagged(reset=True)
        _step(model, o, d, S, w, need_o=False, need_d=False, u=u)
        tags = _lib.timing_read_tagged(reset=True)
        assert "ray_gradient" not in tags and "weight_gradient" in tags, tags
        plain = {k: p.grad.clone() for k, p in model.named_parameters()}
        model.zero_grad(set_to_none=True)
        full = _step(model, o, d, S, w, u=u)
        tags = _lib.timing_read_tagged(reset=True)
        assert "ray_gradient" in tags and "weight_gradient" in tags, tags
        for k, p in model.named_parameters():
            assert torch.equal(p.grad, plain[k]), k
        model.zero_grad(set_to_none=True)
        for p in model.parameters():
            p.requires_grad_(False)
        frozen = _step(model, o, d, S, w, u=u)
        tags = _lib.timing_read_tagged(reset=True)
    finally:
        _lib.timing(False)
    assert "ray_gradient" in tags and "weight_gradient" not in tags and "reduce" not in tags, tags
    assert all(p.grad is None for p in model.parameters())
    assert torch.equal(frozen[0], full[0]) and torch.equal(frozen[1], full[1])


def test_pose_refinement_moves_toward_the_true_pose(dev):
    """iNeRF-style: a frozen network, camera_o fitted by Adam through render_image."""
    params = golden_params(2.0)
    model = make_model(dev, params, "fp32")
    model.keep_workspace = False
    for p in model.parameters():
        p.requires_grad_(False)
    H = Wd = 16
    S, focal = 32, 16.0
    true_o = torch.tensor([[0.0, -3.0, 2.6]])
    cam_r = O.look_at_pose(true_o[0].tolist())
    with torch.no_grad():
        target, _ = model.render_image(true_o.to(dev), cam_r.to(dev), H, Wd, focal, S)
    start = true_o + 0.05 * torch.tensor([[1.0, -1.0, 1.0]]) / 3 ** 0.5        # 0.05 away
    cam_o = start.clone().to(dev).requires_grad_(True)
    opt = torch.optim.Adam([cam_o], lr=2e-3)
    first = None
    for _ in range(20):
        opt.zero_grad()
        img, _ = model.render_image(cam_o, cam_r.to(dev), H, Wd, focal, S, max_chunk_size=256)
        ((img - target) ** 2).mean().backward()
        if first is None:
            first = cam_o.grad.detach().cpu().clone()
        opt.step()
    end = float((cam_o.detach().cpu() - true_o).norm())
    print(f"pose error {float((start - true_o).norm()):.4f} -> {end:.4f}")
    assert end < float((start - true_o).norm())
    # the oracle's first step: the same direction
    ro = start.clone().double().requires_grad_(True)
    p64 = {k: v.double() for k, v in params.items()}
    with torch.no_grad():
        tgt = O.render_image(p64, CFG, true_o.double(), cam_r.double(), H, Wd, focal, S)[0]
    img = O.render_image(p64, CFG, ro, cam_r.double(), H, Wd, focal, S)[0]
    ((img - tgt) ** 2).mean().backward()
    assert torch.equal(torch.sign(first), torch.sign(ro.grad.float())), (first, ro.grad)
