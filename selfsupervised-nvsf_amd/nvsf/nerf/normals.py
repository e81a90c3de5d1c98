"""Geometry of the learned density field: its spatial gradient, surface normals n = -grad sigma / |grad sigma|, and rendered normal /
incidence-angle maps (DESIGN.md sections 9l, 9m).  The reference has no counterpart: it wraps its hash look-ups in torch.no_grad()
(network_dynamic.py:245-265) and never differentiates a field with respect to position.

Both models.  Everything here runs under no_grad as direct operator calls -- four launches per batch of points for the static hash
field (NeRFNetworkStatic), the chain of section 9m for the space-time NeRFNetwork (at a frame time, on a HIP device only: the chain
rule through the K-planes, the static grid, the time-sliced 2-D grids and the flow warp x + flow(x, t)) -- with no autograd graph,
so it is first order: normals cannot enter a training loss.
"""
import numpy as np
import torch

from nvsf import _hip
from nvsf import field_ops as ops
from nvsf.nerf import activation

W_BASE, W_NEIGHBOUR = 0.5, 0.25  # the neighbour blend of the space-time model (network_dynamic.py:273-274)


def _is_static(model):
    from nvsf.nerf.models.network_static import NeRFNetworkStatic
    return isinstance(model, NeRFNetworkStatic)


def _space_time_model(model, what, on_device):
    """The checks of a space-time model, in the order the callers document: the device first, then the model's shape."""
    from nvsf.nerf.models.network_dynamic import NeRFNetwork
    if not isinstance(model, NeRFNetwork):
        raise NotImplementedError(f"{what}: the static hash field (NeRFNetworkStatic) and the space-time NeRFNetwork have a coordinate gradient")
    if not (on_device and model.aabb_infer.is_cuda):
        raise NotImplementedError(f"{what}: the space-time model's coordinate gradient has no CPU form (points and model on a HIP device)")


def logit_gradient_blocks(enc_spec, net_spec):
    """F where the density MLP can hand d h0 / d features to hashgrid_grad_x level by level ([L, M, F], mlp_backward(grad_x_blocks=F)),
    else 0 (rows [M, L F])."""
    return enc_spec.F if (enc_spec.F in (2, 4) and net_spec.n_in == enc_spec.L * enc_spec.F and net_spec.n_in % 8 == 0) else 0


def _finish(sigma, dh, bound):
    """grad = clamp(sigma) * d h0 / d x01 / (2 bound) (trunc_exp's derivative) and the unit normal."""
    grad = (sigma.clamp(activation._LO, activation._HI).unsqueeze(-1) * dh) / (2 * bound)
    norm = torch.linalg.vector_norm(grad, dim=-1, keepdim=True)
    ok = torch.isfinite(norm) & (norm > 0)
    normal = torch.where(ok, -grad / torch.where(ok, norm, torch.ones_like(norm)), torch.zeros_like(grad))
    return {"sigma": sigma, "grad": grad, "normal": normal}


def density_gradient(model, x, cal_lidar_color=False, time=None, fp16=None, flow_jacobian=True):
    """{"sigma" [M], "grad" [M, 3], "normal" [M, 3]} (fp32) of the raw density (no density_scale, as in the mesh export) at the
    world-space points x [M, 3] on the HIP device:
        grad = clamp(sigma, exp(-15), exp(15)) * d h0 / d x01 / (2 bound)       (trunc_exp's derivative, nerf/activation.py)
        normal = -grad / |grad|, 0 where |grad| is 0 or not finite.
    NeRFNetworkStatic (`time`, `fp16`, `flow_jacobian` are ignored):
        hashgrid_forward -> mlp_forward -> mlp_backward(one-hot gradient of output column 0, input gradient only) -> hashgrid_grad_x.
    The space-time NeRFNetwork at the frame time `time` (float or tensor; required), `fp16` as in render (the flow MLP's regime): the
    forward is model.density's own (same sigma, bit for bit); d h0 / d features comes from the density MLP's backward on the rounded
    network input, and with u = x01, f = flow(u, t), c = (0.5, 0.25, 0.25) (an absent neighbour's weight goes to c0)
        a0 = d/du [g_ps . plane_s(u) + c0 g_pd . plane_d(u, t) + g_hs . hash_s(u) + c0 g_hd . hash_d(u, t)]
        a_k = d/dp [c_k (g_pd . plane_d(p, t_k) + g_hd . hash_d(p, t_k))] at p = u + f_k,  k = 1, 2
        d h0 / d u = a0 + a1 + a2 + J_f(u)^T [a1; a2]          (the last term only with `flow_jacobian`)
    from the plane kernels' position gradients, hashgrid_grad_x and HashGrid4D.dynamic_grad_x."""
    if not _is_static(model):
        _space_time_model(model, "density_gradient", torch.is_tensor(x) and x.is_cuda)
        if time is None:
            raise ValueError("density_gradient: the space-time model needs `time` (the frame time in [0, 1]) to evaluate its density")
    if not torch.is_tensor(x) or not x.is_cuda:
        raise _hip.NvsfHipError("density_gradient needs points on a HIP device (got a CPU tensor); there is no CPU fallback")
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"density_gradient: x must be [M, 3] (got {tuple(x.shape)})")
    if not _is_static(model):
        return _density_gradient_space_time(model, x, cal_lidar_color, time, fp16, flow_jacobian)
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
        return _finish(sigma, dh, model.bound)


def expand_lagrange_gradient(g_red, weights4):
    """The gradient of the flow grid's reduction, reduced[:, 2 l + e] = sum_i w_i feature[:, 8 l + 2 i + e]: g_red [M, 2 L] -> [M, 8 L],
    feature 2 i + e of level l receives w_i * g_red[:, 2 l + e] (weights4: the four host values of lagrange_weights_host)."""
    M, L = g_red.shape[0], g_red.shape[1] // 2
    w = ops.device_constant(weights4, g_red.device)
    return (g_red.reshape(M, L, 1, 2) * w.view(1, 1, 4, 1)).reshape(M, 8 * L)


def flow_grid_jtp(flow_net, xt, t_host, g_red):
    """J^T g of the flow field's front end (3-D grid, D = 3, F = 8, and its Lagrange reduction over time) with respect to the position:
    xt [M, >= 3] fp32, g_red [M, 2 L] -> fp32 [M, 3]."""
    from nvsf.nerf.models.hash_field import lagrange_weights_host
    enc = flow_net.grid_enc
    g8 = expand_lagrange_gradient(g_red.float(), lagrange_weights_host(t_host, 4, xt.is_cuda))  # the weights _grid_lagrange passes
    return ops.hashgrid_grad_x(xt, (0, 1, 2), enc.table_f16(), enc.spec, g8)


def flow_mlp_jtp(flow_net, reduced, a, fp16=None):
    """J^T a of the flow MLP at its input `reduced` [M, 2 L] (a [M, 6] fp32) -> fp32 [M, 2 L], in the regime the forward ran in: the
    fused backward kernel (fp16 operands; `a` is handed over relative to its largest entry so that the kernel's fp16 gradients neither
    overflow nor vanish, no host read) or, for the fp32 Linear layers, autograd on those three layers alone."""
    if flow_net.mlp_mode(fp16) == "fused" and flow_net._fused_mlp_ok():
        w16 = flow_net._mlp_weights_f16()
        peak = a.abs().amax(dim=1, keepdim=True).clamp_min(torch.finfo(torch.float32).tiny)  # per row: a sample's result does not depend on its batch
        g_red, _ = ops.mlp_backward(reduced.contiguous(), w16, flow_net._mlp_spec, (a / peak).contiguous(), need_grad_x=True)
        return g_red * peak
    with torch.enable_grad():
        r = reduced.detach().requires_grad_(True)
        (g_red,) = torch.autograd.grad(flow_net.mlp(r), r, a)
    return g_red.detach()


def _density_gradient_space_time(model, x, cal_lidar_color, time, fp16, flow_jacobian):
    from nvsf.nerf.models.hash_field import _host_time, neighbour_frames
    dev = x.device
    hash_enc = model.hash_encoder_lidar if cal_lidar_color else model.hash_encoder_camera
    planes_enc = model.planes_encoder_lidar if cal_lidar_color else model.planes_encoder_camera
    net = model.sigma_net
    with torch.no_grad():
        # the frame time on the host without a device read where the caller has it there (a float, a CPU tensor); a device tensor is
        # read once per tensor object (_host_time remembers it), so a chunked render does not drain the stream per chunk
        t_host = float(np.float32(_host_time(time)))  # the fp32 value, as the forward reads it back from its [1, 1] tensor
        t = time if (torch.is_tensor(time) and time.is_cuda and time.dtype == torch.float32 and tuple(time.shape) == (1, 1)) \
            else ops.device_constant([float(np.float32(t_host))], dev).view(1, 1)
        frame_idx = int(np.float32(t_host) * np.float32(model.num_frames - 1))  # as NeRFNetwork._dynamic_features
        u = model._unit_cube(x.float())
        M = u.shape[0]
        # ---- forward: model.density's own launches, keeping h, the rounded network input and the flow field's intermediates
        kept = {}
        feats = model._dynamic_features_fused(u, t, t_host, frame_idx, hash_enc, planes_enc, fp16, keep=kept)
        h, x16 = model._density_tail_fused(*feats, keep_input=True)
        xt, flow = kept["xt"].contiguous(), kept["flow"]
        sigma = torch.empty(M, dtype=torch.float32, device=dev)
        _hip.call("nvsf_exp_col", _hip.ptr(h), h.stride(0), 0, M, _hip.ptr(sigma))
        # ---- g = d h0 / d features [M, 120] = g_ps | g_pd | g_hs | g_hd
        spec, w16 = net.spec, net.weights_f16()
        one_hot = torch.zeros(M, spec.out_cols, dtype=torch.float32, device=dev)
        one_hot[:, 0] = 1.0
        g, _ = ops.mlp_backward(x16[:, :spec.n_in], w16, spec, one_hot[:, :spec.n_out], need_grad_x=True)
        nb = neighbour_frames(frame_idx, model.num_frames)
        c0 = W_BASE + sum(W_NEIGHBOUR for n in nb if n is None)  # an absent neighbour is the base evaluation (hash_feat_1 = hash_feat_d)
        # the plane gradients as rows of their own, the dynamic one times c0, in one pass (the plane backward reads dense rows)
        g_ps = torch.empty(M, 32, dtype=torch.float32, device=dev)
        g_pd0 = torch.empty(M, 32, dtype=torch.float32, device=dev)
        _hip.call("nvsf_density_tail_grad_split", _hip.ptr_rows(g), g.stride(0), M, _hip.ptr(g_pd0), None, None, 0, 0, None, 0, _hip.ptr(g_ps), c0)
        g_pd, g_hs, g_hd = g[:, 32:64], g[:, 64:96], g[:, 96:120]
        # ---- a0: the base term
        cl, res = planes_enc._channel_last(), _hip.host_u32(planes_enc._res_host)
        S = len(planes_enc._res_host) // 4
        g_xt = torch.empty(M, 4, dtype=torch.float32, device=dev)
        _hip.call("nvsf_planes_bwd", _hip.ptr(xt), M, _hip.ptr(cl), S, 8, res, 3, _hip.ptr(g_ps), _hip.ptr(g_pd0), None, _hip.ptr(g_xt))
        static = hash_enc.hash_static
        dh = ops.hashgrid_grad_x(u, (0, 1, 2), static.table_f16(), static.spec, g_hs)
        dh += g_xt[:, :3]
        hash_enc.dynamic_grad_x(u, t, t_host, g_hd, grad_scale=c0, out=dh, accumulate=True)
        # ---- a1, a2: the warped terms, side by side in one [M, 6] buffer (the columns of an absent neighbour stay zero)
        present = [n for n in nb if n is not None]
        if present:
            a = (torch.empty if len(present) == 2 else torch.zeros)(M, 6, dtype=torch.float32, device=dev)
            fl = ops._f32_rows(flow)
            n_ev = len(present)
            eval_args = ops._eval_args([1] * n_ev, [fl] * n_ev, [n[2] for n in present], [float(n[0]) for n in present])
            _hip.call("nvsf_planes_multi_bwd", _hip.ptr_rows(u), u.stride(0), M, _hip.ptr(cl), S, 8, res, n_ev, *eval_args,
                      ops._ptr_array([g_pd] * n_ev), _hip.host_u32([g.stride(0)] * n_ev), _hip.host_f32([W_NEIGHBOUR] * n_ev), None,
                      ops._ptr_array([a] * n_ev), _hip.host_u32([6] * n_ev), _hip.host_u32([n[2] for n in present]))
            for tn, tn_host, col in present:
                hash_enc.dynamic_grad_x(u, tn, tn_host, g_hd, grad_scale=W_NEIGHBOUR, offset=fl, offset_col=col, out=a[:, col:col + 3],
                                        accumulate=True)
            dh += a[:, :3]
            dh += a[:, 3:]
            if flow_jacobian:
                g_red = flow_mlp_jtp(model.flow_net, kept["reduced"], a, fp16)
                dh += flow_grid_jtp(model.flow_net, xt, t_host, g_red)
        return _finish(sigma, dh, model.bound)


def render_normals(model, rays_o, rays_d, cal_lidar_color=False, num_steps=768, max_ray_batch=4096, return_samples=False, time=None,
                   fp16=None, flow_jacobian=True):
    """Normal and incidence-angle maps of the rays (rays_o, rays_d) [N, 3]: uniform samples as NeRFRenderer.run takes them (no
    perturbation), density_gradient at the samples, the compositing weights of the uniform compositor (ops.CompositeWeightsFn), and the image
    compositor on the unit normals with a zero background.  Staged in chunks of max_ray_batch rays, like render(staged=True).
    `time`, `fp16`, `flow_jacobian`: passed to density_gradient (the space-time model needs `time`).  For the space-time model a ray's
    result does not depend on the chunking only with the fused flow MLP (fp16=True or an autocast region): the fp32 Linear layers of the
    other regime are library GEMMs whose summation order may follow the batch size (differences of a few 1e-8 then, as in the forward).
      normal         [N, 3]  sum_i w_i n_i (not renormalised: its length says how much of the ray's weight agrees on a direction)
      weights_sum    [N]
      cos_incidence  [N]     -normal . d / |d|: what a LiDAR intensity model is a function of
    `return_samples` adds "weights" [N, T] and "sample_normals" [N, T, 3]."""
    if not _is_static(model):
        _space_time_model(model, "render_normals", rays_o.is_cuda and rays_d.is_cuda)
        if time is None:
            raise ValueError("render_normals: the space-time model needs `time` (the frame time in [0, 1]) to evaluate its density")
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
            field = density_gradient(model, xyzs.view(-1, 3), cal_lidar_color, time=time, fp16=fp16, flow_jacobian=flow_jacobian)
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
