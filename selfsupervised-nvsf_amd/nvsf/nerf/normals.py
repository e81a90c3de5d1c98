"""Geometry of the learned density field: its spatial gradient, surface normals n = -grad sigma / |grad sigma|, and rendered normal /
incidence-angle maps.  The reference has no counterpart: it wraps its hash look-ups in torch.no_grad()
(network_dynamic.py:245-265) and never differentiates a field with respect to position.

Static hash field (NeRFNetworkStatic) only.  Everything here runs under no_grad as direct operator calls -- four launches per batch of
points, no autograd graph -- so it is first order: normals cannot enter a training loss.  The 4-D hash encoders and the flow warp of
the space-time model have no coordinate gradient.
"""
import torch

from nvsf import _hip
from nvsf import field_ops as ops
from nvsf.nerf import activation


def _static_model(model, what):
    from nvsf.nerf.models.network_static import NeRFNetworkStatic
    if not isinstance(model, NeRFNetworkStatic):
        raise NotImplementedError(f"{what}: only the static hash field (NeRFNetworkStatic) has a coordinate gradient; the 4-D hash "
                                  "encoders and the flow warp of the space-time model do not")


def logit_gradient_blocks(enc_spec, net_spec):
    """F where the density MLP can hand d h0 / d features to hashgrid_grad_x level by level ([L, M, F], mlp_backward(grad_x_blocks=F)),
    else 0 (rows [M, L F])."""
    return enc_spec.F if (enc_spec.F in (2, 4) and net_spec.n_in == enc_spec.L * enc_spec.F and net_spec.n_in % 8 == 0) else 0


def density_gradient(model, x, cal_lidar_color=False):
    """{"sigma" [M], "grad" [M, 3], "normal" [M, 3]} (fp32) of the raw density (no density_scale, as in the mesh export) at the
    world-space points x [M, 3] on the HIP device:
        hashgrid_forward -> mlp_forward -> mlp_backward(one-hot gradient of output column 0, input gradient only) -> hashgrid_grad_x,
        grad = clamp(sigma, exp(-15), exp(15)) * d h0 / d x01 / (2 bound)       (trunc_exp's derivative, nerf/activation.py)
        normal = -grad / |grad|, 0 where |grad| is 0 or not finite."""
    _static_model(model, "density_gradient")
    if not torch.is_tensor(x) or not x.is_cuda:
        raise _hip.NvsfHipError("density_gradient needs points on a HIP device (got a CPU tensor); there is no CPU fallback")
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"density_gradient: x must be [M, 3] (got {tuple(x.shape)})")
    enc, net = model._modality(cal_lidar_color)[:2]
    with torch.no_grad():
        x01 = ((x.float() + model.bound) / (2 * model.bound)).contiguous()  # as NeRFNetworkStatic.density normalises
        M = x01.shape[0]
        table, w16 = enc.table_f16(), net.weights_f16()
        feat = ops.hashgrid_forward(x01, (0, 1, 2), table, enc.spec)
        h = ops.mlp_forward(feat, w16, net.spec)
        sigma = torch.empty(M, dtype=torch.float32, device=x01.device)
        _hip.call("nvsf_exp_col", _hip.ptr(h), h.stride(0), 0, M, _hip.ptr(sigma))
        one_hot = torch.zeros(M, net.spec.out_cols, dtype=torch.float32, device=x01.device)
        one_hot[:, 0] = 1.0
        # the kernel carries its fp16 gradients times MLP_GRAD_SCALE and divides it back out on the way out (the default of every caller)
        g_feat, _ = ops.mlp_backward(feat, w16, net.spec, one_hot[:, :net.spec.n_out], need_grad_x=True,
                                     grad_x_blocks=logit_gradient_blocks(enc.spec, net.spec))
        dh = ops.hashgrid_grad_x(x01, (0, 1, 2), table, enc.spec, g_feat)
        grad = (sigma.clamp(activation._LO, activation._HI).unsqueeze(-1) * dh) / (2 * model.bound)
        norm = torch.linalg.vector_norm(grad, dim=-1, keepdim=True)
        ok = torch.isfinite(norm) & (norm > 0)
        normal = torch.where(ok, -grad / torch.where(ok, norm, torch.ones_like(norm)), torch.zeros_like(grad))
    return {"sigma": sigma, "grad": grad, "normal": normal}


def render_normals(model, rays_o, rays_d, cal_lidar_color=False, num_steps=768, max_ray_batch=4096, return_samples=False):
    """Normal and incidence-angle maps of the rays (rays_o, rays_d) [N, 3]: uniform samples as NeRFRenderer.run takes them (no
    perturbation), density_gradient at the samples, the compositing weights of the uniform compositor (ops.CompositeWeightsFn), and the image
    compositor on the unit normals with a zero background.  Staged in chunks of max_ray_batch rays, like render(staged=True).
      normal         [N, 3]  sum_i w_i n_i (not renormalised: its length says how much of the ray's weight agrees on a direction)
      weights_sum    [N]
      cos_incidence  [N]     -normal . d / |d|: what a LiDAR intensity model is a function of
    `return_samples` adds "weights" [N, T] and "sample_normals" [N, T, 3]."""
    _static_model(model, "render_normals")
    if not rays_o.is_cuda or not rays_d.is_cuda:
        raise _hip.NvsfHipError("render_normals needs rays on a HIP device (got a CPU tensor); there is no CPU fallback")
    rays_o = rays_o.contiguous().view(-1, 3).float()
    rays_d = rays_d.contiguous().view(-1, 3).float()
    N, T, dev = rays_o.shape[0], int(num_steps), rays_o.device
    out = {"normal": torch.empty(N, 3, dtype=torch.float32, device=dev), "weights_sum": torch.empty(N, dtype=torch.float32, device=dev)}
    if return_samples:
        out["weights"] = torch.empty(N, T, dtype=torch.float32, device=dev)
        out["sample_normals"] = torch.empty(N, T, 3, dtype=torch.float32, device=dev)
    aabb = model.aabb_train if model.training else model.aabb_infer
    zero_bg = ops.device_constant([0.0, 0.0, 0.0], dev)
    with torch.no_grad():
        for head in range(0, N, int(max_ray_batch)):
            tail = min(head + int(max_ray_batch), N)
            o, d = rays_o[head:tail].contiguous(), rays_d[head:tail].contiguous()
            nears, fars = model._near_far(o, d, cal_lidar_color, aabb)
            z_vals, xyzs = ops.uniform_samples(o, d, nears, fars, T, aabb, None)
            field = density_gradient(model, xyzs.view(-1, 3), cal_lidar_color)
            weights, weights_sum, _ = ops.CompositeWeightsFn.apply(field["sigma"].view(tail - head, T), z_vals, nears, fars, model._k_scale())
            normals = field["normal"].view(tail - head, T, 3)
            out["normal"][head:tail] = ops.CompositeImageFn.apply(weights, normals, weights_sum, zero_bg)
            out["weights_sum"][head:tail] = weights_sum
            if return_samples:
                out["weights"][head:tail] = weights
                out["sample_normals"][head:tail] = normals
        d_hat = rays_d / torch.linalg.vector_norm(rays_d, dim=-1, keepdim=True)
        out["cos_incidence"] = -(out["normal"] * d_hat).sum(-1)
    return out
