"""TEST INFRASTRUCTURE -- a differentiable float64 restatement of the static field's TRAINING render, run on the device.

NeRFNetworkStatic's training forward (renderer_dynamic.py's `run` with the static hash field inside: ops.RenderRaysFn, or the operator
chain it replaces) written as plain torch algebra in float64, so that autograd's gradient of any functional of (weights, weights_sum,
depth, image) is an independent high-precision statement of what the HIP backward kernels compute.  oracle/torch_cpu_path.py is the
model; the rules that make the two comparable:

  * where the kernels must agree exactly, they are followed: sample positions, the box clamp, the unit-cube normalisation, the
    hash-grid cell indices and fractions and the interpolation weights are computed in fp32 operation by operation as the kernels
    compute them (`-ffp-contract=off`; fma only where the kernel says fmaf), then promoted;
  * the fp16 roundings of the forward are applied (table, encoded features, MLP inputs and hidden activations, MLP weights, the
    geometry rows handed to the heads, the direction encodings); their gradient passes straight through, as it does in the kernels;
  * everything else -- interpolation, MLP products, trunc_exp, alpha / transmittance / weights, sigmoid, compositing -- is float64;
  * the table gradient is autograd's gradient of the float64 gather (an fp64 sum);
  * the only values taken from the kernels are the sample depths `z_vals` and the `weights > w_thresh` mask, both inputs of the
    forward, never anything their backward produced.

`render_packed` restates the third training path the same way: the occupancy-grid render (NeRFRenderer.run_cuda in training mode:
march_rays_train -> density / color on the packed samples -> composite_rays_train).  It takes the marcher's outputs (positions,
directions, the two step columns and the (id, offset, count) rows; the marcher is pinned bit for bit to the oracle) and nothing else;
`composite_packed` is its per-ray part, the early-terminated sums of the packed compositor, also compared with the kernel alone.
"""
import math

import numpy as np
import torch

_P1, _P2 = 2654435761, 805459861
_LO = float(torch.exp(torch.tensor(-15.0, dtype=torch.float32)))  # trunc_exp's gradient clamp, as nerf/activation.py states it
_HI = float(torch.exp(torch.tensor(15.0, dtype=torch.float32)))


class _F16(torch.autograd.Function):
    """Forward: round to the nearest fp16 (value kept in fp64); backward: straight through (the kernels' hand-overs)."""

    @staticmethod
    def forward(ctx, x):
        return x.half().to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


class _ReluF16(torch.autograd.Function):
    """A hidden activation: fp16(relu(z)); the gate of the backward is the stored activation > 0 (FullyFusedMLP's rule)."""

    @staticmethod
    def forward(ctx, z):
        a = torch.relu(z).half().to(z.dtype)
        ctx.save_for_backward(a)
        return a

    @staticmethod
    def backward(ctx, g):
        (a,) = ctx.saved_tensors
        return g * (a > 0).to(g.dtype)


class _TruncExp(torch.autograd.Function):
    """sigma = exp(h); towards h the gradient is multiplied by exp(clamp(h, -15, 15)) (nerf/activation.py)."""

    @staticmethod
    def forward(ctx, h):
        s = torch.exp(h)
        ctx.save_for_backward(s)
        return s

    @staticmethod
    def backward(ctx, g):
        (s,) = ctx.saved_tensors
        return g * s.clamp(_LO, _HI)


def f16(x):
    return _F16.apply(x)


def sample_positions(rays_o, rays_d, z_vals, bound):
    """x01 [N T, 3] fp32, as the training kernels form it: p = o + d z, clamped to the box, (p + bound) * (1 / (2 bound))."""
    p = rays_o[:, None, :] + rays_d[:, None, :] * z_vals[:, :, None]
    p = torch.minimum(torch.maximum(p, torch.tensor(-float(bound), device=p.device)), torch.tensor(float(bound), device=p.device))
    inv_extent = float(np.float32(1.0) / np.float32(2.0 * bound))
    return ((p + float(bound)) * inv_extent).reshape(-1, 3)


def _corners(x01, spec):
    """(level, table row offset, rows [M] int64, weight [M] fp32) of every corner of every level of x01 [M, 3] fp32, as the kernels
    form them."""
    for l in range(spec.L):
        scale = np.float32(spec.scales[l])
        res, off = int(spec.res[l]), int(spec.offsets[l])
        rows = int(spec.offsets[l + 1]) - off
        # pos = fmaf(scale, x, 0.5): the fp64 product of two fp32 values is exact, + 0.5 too (< 53 bits), one rounding to fp32
        pos = (x01.double() * float(scale) + 0.5).float()
        cell = torch.floor(pos)
        frac = pos - cell
        c = cell.to(torch.int64)
        dense = res ** 3 <= rows
        for k in range(8):
            b = [(k >> d) & 1 for d in range(3)]
            cc = [c[:, d] + b[d] for d in range(3)]
            if dense:
                idx = (cc[0] + cc[1] * res + cc[2] * res * res) % rows
            else:
                idx = ((cc[0] & 0xFFFFFFFF) ^ ((cc[1] * _P1) & 0xFFFFFFFF) ^ ((cc[2] * _P2) & 0xFFFFFFFF)) % rows
            w = torch.ones_like(frac[:, 0])  # ((1 w0) w1) w2 in fp32, as the kernel multiplies
            for d in range(3):
                w = w * (frac[:, d] if b[d] else 1.0 - frac[:, d])
            yield l, off, idx, w


def hash_features(x01, table64, spec):
    """x01 [M, 3] fp32 -> [M, L F] fp64 features (fp16-rounded forward), differentiable in table64 [n_rows F] (fp64 leaf)."""
    tab = f16(table64).view(-1, spec.F)
    acc = [None] * spec.L
    for l, off, idx, w in _corners(x01, spec):
        term = w.double()[:, None] * tab[off + idx]
        acc[l] = term if acc[l] is None else acc[l] + term
    return f16(torch.cat(acc, -1))


def touched_entries(x01, spec):
    """bool [n_rows F]: the table entries some corner of x01 reads (whatever its weight) -- all others must receive no gradient."""
    hit = torch.zeros(spec.n_rows, dtype=torch.bool, device=x01.device)
    for _, off, idx, _ in _corners(x01, spec):
        hit[off + idx] = True
    return hit.repeat_interleave(spec.F)


def mlp(x, w64, spec):
    """Bias-free ReLU MLP (FullyFusedMLP as DESIGN.md 4.3 states it): input fp16-rounded and padded with ones to in_cols, fp16 weights
    (w64: fp64 leaf holding the fp32 parameters), hidden activations fp16(relu(.)), output in full precision -> [M, out_cols]."""
    M = x.shape[0]
    pad = torch.ones(M, spec.in_cols - spec.n_in, dtype=x.dtype, device=x.device)
    a = torch.cat([f16(x), pad], -1)
    mats = spec.split(f16(w64))
    for W in mats[:-1]:
        a = _ReluF16.apply(a @ W.t())
    return a @ mats[-1].t()


def freq_encode(d01, n_freq=12):
    """sin / cos(2^k pi x) of the fp32 direction, evaluated in fp64 and rounded to fp16 -> [N, 6 n_freq]."""
    k = torch.arange(n_freq, dtype=torch.float64, device=d01.device)
    a = d01.double()[:, :, None] * (2.0 ** k)[None, None, :] * math.pi
    return torch.stack([torch.sin(a), torch.cos(a)], -1).reshape(d01.shape[0], -1).half().double()


def sh4_encode(d01):
    """16 real spherical-harmonics basis functions of 2 d01 - 1 (d01 fp32, the kernel's fp32 argument), fp64, rounded to fp16."""
    x, y, z = ((d01[:, i] * 2.0 - 1.0).double() for i in range(3))
    xy, xz, yz, x2, y2, z2 = x * y, x * z, y * z, x * x, y * y, z * z
    o = [torch.full_like(x, 0.28209479177387814), -0.48860251190291987 * y, 0.48860251190291987 * z, -0.48860251190291987 * x,
         1.0925484305920792 * xy, -1.0925484305920792 * yz, 0.94617469575755997 * z2 - 0.31539156525251999, -1.0925484305920792 * xz,
         0.54627421529603959 * x2 - 0.54627421529603959 * y2, 0.59004358992664352 * y * (-3.0 * x2 + y2), 2.8906114426405538 * xy * z,
         0.45704579946446572 * y * (1.0 - 5.0 * z2), 0.3731763325901154 * z * (5.0 * z2 - 3.0), 0.45704579946446572 * x * (1.0 - 5.0 * z2),
         1.4453057213202769 * z * (x2 - y2), 0.59004358992664352 * x * (-x2 + 3.0 * y2)]
    return torch.stack(o, -1).half().double()


def leaves(model, lidar):
    """fp64 copies of the parameters one modality's render reads, as autograd leaves: {name: tensor}."""
    names = ["hash_encoder_lidar" if lidar else "hash_encoder_camera", "sigma_net"]
    names += ["raydrop_net", "intensity_net"] if lidar else ["color_net"]
    return {n: getattr(model, n).params.detach().double().requires_grad_() for n in names}


def head_logits(model, p64, enc_rows, geo, lidar):
    """Logits of the per-sample heads on the rows [direction encoding | geo] (both already fp16-rounded): [M, 2] = [raydrop,
    intensity] for LiDAR samples, [M, 3] colour logits otherwise."""
    rows = torch.cat([enc_rows, geo], -1)
    if lidar:
        hs = model.raydrop_net.spec
        return torch.cat([mlp(rows, p64["raydrop_net"], hs)[:, :1], mlp(rows, p64["intensity_net"], hs)[:, :1]], -1)
    return mlp(rows, p64["color_net"], model.color_net.spec)[:, :3]


def render(model, p64, rays_o, rays_d, nears, fars, z_vals, mask, lidar, bg=None):
    """The training render of `model` (a NeRFNetworkStatic) in fp64 with the parameters `p64` (leaves()).  rays [N, 3], nears / fars
    [N], z_vals [N, T] (fp32, the kernel's samples), mask [N, T] bool (the kernel's weights > w_thresh), bg: camera background
    (sequence of 3) -> weights [N, T], weights_sum [N], depth [N], image [N, C] (fp64)."""
    N, T = z_vals.shape
    enc = model.hash_encoder_lidar if lidar else model.hash_encoder_camera
    x01 = sample_positions(rays_o, rays_d, z_vals, float(model.bound))
    feat = hash_features(x01, p64["hash_encoder_lidar" if lidar else "hash_encoder_camera"], enc.spec)
    h = mlp(feat, p64["sigma_net"], model.sigma_net.spec)
    sigma = _TruncExp.apply(h[:, 0]).view(N, T)
    geo = f16(h[:, 1:model.sigma_net.spec.n_out])  # the fp16 geometry rows handed to the heads
    # compositing (renderer_dynamic.py:181-194, 216-221): deltas and the last step in fp32 as the kernels form them
    sample_dist = ((fars - nears) / float(T)).double()
    deltas = torch.cat([(z_vals[:, 1:] - z_vals[:, :-1]).double(), sample_dist[:, None]], -1)
    z64 = z_vals.double()
    alphas = 1.0 - torch.exp(-deltas * float(model._k_scale()) * sigma)
    trans = torch.cumprod(torch.cat([torch.ones(N, 1, dtype=torch.float64, device=z64.device), 1.0 - alphas + 1e-15], -1), -1)[:, :-1]
    weights = alphas * trans
    ws = weights.sum(-1)
    depth = (weights * z64).sum(-1)
    # heads on [direction encoding | geo] of the samples above the weight threshold, sigmoid
    d01 = (rays_d + 1) / 2
    enc_ray = freq_encode(d01, model.view_encoder_lidar.n_frequencies) if lidar else sh4_encode(d01)
    C = 2 if lidar else 3
    m = mask.reshape(-1)
    rgbs = torch.zeros(N * T, C, dtype=torch.float64, device=z64.device)
    if bool(m.any()):
        logits = head_logits(model, p64, enc_ray.repeat_interleave(T, 0)[m], geo[m], lidar)
        rgbs = rgbs.index_put((m.nonzero().squeeze(1),), torch.sigmoid(logits))
    image = (weights[:, :, None] * rgbs.view(N, T, C)).sum(1)
    if not lidar:
        image = image + (1.0 - ws)[:, None] * torch.tensor([float(v) for v in bg], dtype=torch.float64, device=z64.device)
    return {"weights": weights, "weights_sum": ws, "depth": depth, "image": image, "x01": x01, "logits": h[:, 0]}


def composite_packed(sigmas, rgbs, deltas, rays, T_thresh):
    """composite_rays_train in fp64, differentiable in sigmas [M] and rgbs [M, 3] (fp64).  deltas [M, 2]: column 0 is the step that
    enters alpha, column 1 the step that advances t; rays [N, 3] int = (ray id, first row, row count).  A ray is empty when its count
    is 0 or its rows do not fit (first + count > M).  alpha_i = 1 - exp(-sigma_i deltas[i, 0]), T the exclusive product of
    1 - alpha (no 1e-15 term in this compositor), `stop` the first i whose OUTGOING transmittance T_{i+1} is below T_thresh (that
    sample included), else count - 1; the sums run over i <= stop.  -> weights_sum [N], depth [N], image [N, 3], indexed by ray id,
    and per ROW of `rays`: stop (int64, -1 for an empty ray) and margin = min_i |T_{i+1} / T_thresh - 1| over i <= stop (how close
    the ray comes to stopping one sample earlier or later; inf for an empty ray or T_thresh == 0)."""
    M, N, dev = sigmas.shape[0], rays.shape[0], sigmas.device
    d64 = deltas.double()
    ids, ws, dp, im, stops, margins = [], [], [], [], [], []
    for ray_id, off, cnt in rays.tolist():
        if cnt == 0 or off + cnt > M:
            stops.append(-1)
            margins.append(math.inf)
            continue
        alpha = 1.0 - torch.exp(-sigmas[off:off + cnt] * d64[off:off + cnt, 0])
        T_out = torch.cumprod(1.0 - alpha, 0)
        below = (T_out.detach() < T_thresh).nonzero()
        stop = int(below[0]) if below.numel() else cnt - 1
        k = stop + 1
        T_in = torch.cat([torch.ones(1, dtype=torch.float64, device=dev), T_out[:stop]])
        w = alpha[:k] * T_in
        ids.append(ray_id)
        ws.append(w.sum())
        dp.append((w * torch.cumsum(d64[off:off + k, 1], 0)).sum())
        im.append((w[:, None] * rgbs[off:off + k]).sum(0))
        stops.append(stop)
        margins.append(float((T_out.detach()[:k] / T_thresh - 1.0).abs().min()) if T_thresh > 0 else math.inf)
    out_ws = torch.zeros(N, dtype=torch.float64, device=dev)
    out_dp = torch.zeros(N, dtype=torch.float64, device=dev)
    out_im = torch.zeros(N, 3, dtype=torch.float64, device=dev)
    if ids:
        at = (torch.tensor(ids, dtype=torch.int64, device=dev),)
        out_ws, out_dp, out_im = out_ws.index_put(at, torch.stack(ws)), out_dp.index_put(at, torch.stack(dp)), out_im.index_put(at, torch.stack(im))
    return out_ws, out_dp, out_im, torch.tensor(stops, dtype=torch.int64, device=dev), torch.tensor(margins, dtype=torch.float64, device=dev)


def render_packed(model, p64, xyzs, dirs, deltas, rays, lidar, T_thresh, bg=None):
    """The occupancy-grid training render of `model` (a NeRFNetworkStatic with enable_occupancy_grid()) in fp64 with the parameters
    `p64` (leaves()), on the packed samples march_rays_train returned: xyzs, dirs [M, 3], deltas [M, 2] (fp32), rays [N, 3] int32.
    Positions and directions are normalised in fp32 with torch's own operations, as NeRFNetworkStatic.density / color write them (a
    true division, not the fused render's reciprocal multiply); the direction encoding is per sample; the heads run on every packed
    row (no weight mask in this path); sigma = trunc_exp(h0) density_scale; LiDAR images get a third channel of zeros; camera:
    image + (1 - weights_sum) bg after the compositor, as run_cuda does.  -> weights_sum [N], depth [N], image [N, 2 | 3] (by ray id),
    x01 [M, 3], logits [M] and, per row of `rays`, stop and margin (composite_packed)."""
    enc = model.hash_encoder_lidar if lidar else model.hash_encoder_camera
    x01 = (xyzs + model.bound) / (2 * model.bound)
    feat = hash_features(x01, p64["hash_encoder_lidar" if lidar else "hash_encoder_camera"], enc.spec)
    h = mlp(feat, p64["sigma_net"], model.sigma_net.spec)
    sigma = _TruncExp.apply(h[:, 0]) * float(model.density_scale)
    geo = f16(h[:, 1:model.sigma_net.spec.n_out])
    d01 = (dirs + 1) / 2
    enc_rows = freq_encode(d01, model.view_encoder_lidar.n_frequencies) if lidar else sh4_encode(d01)
    rgbs = torch.sigmoid(head_logits(model, p64, enc_rows, geo, lidar))
    if lidar:
        rgbs = torch.cat([rgbs, torch.zeros_like(rgbs[:, :1])], -1)
    ws, depth, image, stop, margin = composite_packed(sigma, rgbs, deltas, rays, T_thresh)
    if lidar:
        image = image[:, :2]
    else:
        image = image + (1.0 - ws)[:, None] * torch.tensor([float(v) for v in bg], dtype=torch.float64, device=ws.device)
    return {"weights_sum": ws, "depth": depth, "image": image, "x01": x01, "logits": h[:, 0], "stop": stop, "margin": margin}
