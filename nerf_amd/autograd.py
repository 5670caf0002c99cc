"""Differentiable wrapper of the fused renderer (training path).

``render_rays_function`` is what ``NeRF.render_rays`` calls: without gradients it is a plain
kernel launch; with gradients — a parameter, ``rays_o`` or ``rays_d`` requires grad — it goes through
``torch.autograd.Function`` whose backward runs the HIP backward kernels: the parameter gradient, and the
ray gradient when a ray input asks for one (pose refinement; with the network frozen no weight gradient is
launched).  Fenceposts and random draws are not differentiated (the reference's fenceposts do not depend on
the rays).
"""
import torch


def _needs_grad(model, rays_o=None, rays_d=None):
    if not torch.is_grad_enabled():
        return False
    if any(t is not None and t.requires_grad for t in (rays_o, rays_d)):
        return True
    return any(p.requires_grad for p in model.parameters())


def render_rays_function(model, rays_o, rays_d, num_samples, u, noise, density_noise_std, rng_mode,
                         t_values=None, want_weights=False):
    """-> (rgb [N,3], seg [N,50], weights [N,S-1] or None)."""
    if not _needs_grad(model, rays_o, rays_d):
        rgb, seg, _, _, weights = model._launch(
            rays_o.shape[0], num_samples, rays_o.device, rays_o=rays_o, rays_d=rays_d, u=u, noise=noise,
            density_noise_std=density_noise_std, rng_mode=rng_mode, t_values=t_values,
            want_weights=want_weights)
        return rgb, seg, weights
    from .backward import RenderRaysFunction
    rgb, seg, weights = RenderRaysFunction.apply(model, rays_o, rays_d, num_samples, u, noise,
                                                 density_noise_std, rng_mode, t_values, want_weights,
                                                 *model._param_list())
    return rgb, seg, (weights if want_weights else None)
