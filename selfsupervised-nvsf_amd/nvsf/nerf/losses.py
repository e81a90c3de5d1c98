"""The loss terms of the training step (nvsf/nerf/train_step.py): the Python half of csrc/losses.hip.

Restated from the reference's `Trainer.train_step` (nvsf/nerf/trainer.py:153-656) with the default CLI settings of
nvsf/scripts/main_nvsf.py:60-97; nothing here depends on the step object:
  * LiDAR: ground truth masked by the ray-drop channel (trainer.py:186-189), predictions masked the same way (:203-206),
    per-ray L1 range (alpha_d 1) + MSE ray-drop against label-smoothed targets (`--smooth_factor`, default 0.0; alpha_r 0.01)
    + MSE intensity (alpha_i 0.1), all `reduction="none"` and SUMMED over the rays (main_nvsf.py:205-221, trainer.py:540-543);
    the predicted and the true point cloud `rays_d * depth / scale` of the chamfer term (trainer.py:229-233): `LidarLossFn`,
    `lidar_losses_host`; URF line-of-sight loss (trainer.py:276-294): `UrfLossFn` on the device, `urf_line_of_sight_loss` on the host;
  * the criteria of these terms and of the colour term are selectable (`--depth_loss`, `--raydrop_loss`, `--intensity_loss`,
    `--rgb_loss`, main_nvsf.py:83-88: l1 / mse / huber / smoothl1 / bce): `LidarCritLossFn`, `CritSumFn`, `CameraCritLossFn`; the
    defaults keep the entries named above;
  * camera: MSE RGB summed over rays and channels (alpha_rgb 1; trainer.py:491-503): `MseSumFn`; optional depth term against the
    LiDAR-projected camera depth map (`--use_rgbd_loss`, trainer.py:505-518: both capped at 80 m, masked where the map is empty,
    summed): `CameraLossFn`, `rgb_depth_loss_host`;
  * the structural regularisation on LiDAR patches in its `grad_loss` form (trainer.py:296-470: first differences (or Sobel
    gradients) of the rendered / true range inside pH x pW patches, masked by the true ray-drop channel and the flatness of the true
    frame; criteria `--depth_grad_loss` l1 / mse / huber / smoothl1 / cos, `--sobel_grad`): `LidarGradLossFn`;
  * the error maps the patch sampler draws from (trainer.py:552-630): `update_error_map`;
  * the distortion loss of mip-NeRF 360 on the rows of both renders (sketched and commented out at renderer_dynamic.py:242-245):
    `DistortionLossFn` on the device, `distortion_loss` on the host.
"""
import math

import torch


def _f32(t):
    return t.detach().float().contiguous()


def _f32_or_none(t):
    return None if t is None else t.float().contiguous()


def criterion_code(criterion, scale, table, option):
    """Criterion name -> (kernel code of `table`, parameter): Huber delta = 0.2 x scale, SmoothL1 beta = 0.1 (main_nvsf.py:207-209).
    option: (name, line) of the CLI option, for the error text."""
    if criterion not in table:
        raise ValueError(f"{option[0]}={criterion!r}: one of {sorted(table)} (main_nvsf.py:{option[1]})")
    param = 0.2 * float(scale) if criterion == "huber" else (0.1 if criterion == "smoothl1" else 0.0)
    return table[criterion], param


# the criteria of the four per-ray terms (main_nvsf.py:205-210) as kernel codes, and the lines of their CLI options.  No "cos":
# CosineSimilarity over dim 1 of a [B, N] or [B, N, 3] pair is no per-ray loss (the same reasoning as CameraLossFn.CRITERIA)
PER_RAY_CRITERIA = {"l1": 0, "mse": 1, "huber": 2, "smoothl1": 3, "bce": 4}
PER_RAY_OPTIONS = {"rgb_loss": 83, "depth_loss": 85, "intensity_loss": 87, "raydrop_loss": 88}
DEFAULT_CRITERIA = {"depth_loss": "l1", "raydrop_loss": "mse", "intensity_loss": "mse", "rgb_loss": "mse"}


def per_ray_criterion(option, criterion, scale):
    """(kernel code, parameter) of `--depth_loss` / `--raydrop_loss` / `--intensity_loss` / `--rgb_loss`; an unknown name raises."""
    return criterion_code(criterion, scale, PER_RAY_CRITERIA, (option, PER_RAY_OPTIONS[option]))


def torch_criterion(criterion, scale, option="rgb_depth_loss"):
    """The torch.nn criterion of main_nvsf.py:205-210 with reduction "none": what the host branches evaluate."""
    line = PER_RAY_OPTIONS.get(option, 91)
    _, param = criterion_code(criterion, scale, PER_RAY_CRITERIA, (option, line))
    return {"l1": torch.nn.L1Loss, "mse": torch.nn.MSELoss, "bce": torch.nn.BCEWithLogitsLoss,
            "smoothl1": lambda **kw: torch.nn.SmoothL1Loss(beta=param, **kw),
            "huber": lambda **kw: torch.nn.HuberLoss(delta=param, **kw)}[criterion](reduction="none")


def urf_line_of_sight_loss(weights, z_vals, gt_depth, eps):
    """Line-of-sight loss of Urban Radiance Fields as written at trainer.py:276-294."""
    gt = gt_depth.reshape(z_vals.shape[0], 1)
    n_valid = (gt > 0.0).sum()
    empty = (z_vals < gt - eps) | (z_vals > gt + eps)
    loss_empty = ((empty * weights) ** 2).sum() / n_valid
    near = (z_vals > gt - eps) & (z_vals < gt + eps)
    distance = near * (z_vals - gt)
    sigma = eps / 3.0
    distr = 1.0 / (sigma * math.sqrt(2 * math.pi)) * torch.exp(-(distance ** 2 / (2 * sigma ** 2)))
    distr = distr / distr.max()
    distr = distr * near
    loss_near = ((near * weights - distr) ** 2).sum() / n_valid
    return 0.1 * loss_empty + 0.1 * loss_near


class UrfLossFn(torch.autograd.Function):
    """urf_line_of_sight_loss on the device (nvsf_urf_loss_fwd / _bwd, csrc/losses.hip): weights, z_vals [N, T], gt_depth [N] (any shape
    with N elements: the masked true range), eps a Python float -> scalar.  The ~25 launches of the expression over the [N, T] arrays (and
    as many again under autograd) become two streaming passes forward and one backward; distr.max() and the count of valid rays stay on
    the device.  Gradient to `weights` only (z_vals and gt_depth carry none in the step)."""
    WS_BYTES = 1024 * 8 * 8  # per-workgroup partials of the forward

    @staticmethod
    def forward(ctx, weights, z_vals, gt_depth, eps):
        from nvsf import _hip
        w, z, g = _f32(weights), _f32(z_vals), _f32(gt_depth).view(-1)
        if w.dim() != 2 or z.shape != w.shape or g.numel() != w.shape[0]:
            raise ValueError(f"UrfLossFn: weights {tuple(weights.shape)}, z_vals {tuple(z_vals.shape)} and gt_depth {tuple(gt_depth.shape)} "
                             "do not describe one [N, T] sample batch")
        N, T = w.shape
        eps = float(eps)
        eps_hi = float(torch.tensor(eps, dtype=torch.float32))  # the band edges use the fp32 value, sigma the double: passed as hi + lo
        out = torch.empty((), dtype=torch.float32, device=w.device)
        state = torch.empty(2, dtype=torch.float64, device=w.device)
        ws = torch.empty(UrfLossFn.WS_BYTES // 8, dtype=torch.float64, device=w.device)
        _hip.call("nvsf_urf_loss_fwd", _hip.ptr(w), _hip.ptr(z), _hip.ptr(g), N, T, eps_hi, eps - eps_hi, _hip.ptr(ws), UrfLossFn.WS_BYTES,
                  _hip.ptr(out), _hip.ptr(state))
        ctx.save_for_backward(w, z, g, state)
        ctx.eps, ctx.shape = (eps_hi, eps - eps_hi), weights.shape
        return out

    @staticmethod
    def backward(ctx, grad):
        from nvsf import _hip
        w, z, g, state = ctx.saved_tensors
        grad_w = torch.empty_like(w)
        _hip.call("nvsf_urf_loss_bwd", _hip.ptr(w), _hip.ptr(z), _hip.ptr(g), w.shape[0], w.shape[1], *ctx.eps, _hip.ptr(state),
                  _hip.ptr(_f32_or_none(grad)), _hip.ptr(grad_w))
        return grad_w.view(ctx.shape), None, None, None


def distortion_ray_losses(weights, z_vals, nears, fars):
    """The per-ray distortion loss of mip-NeRF 360 (Barron et al. 2022, eq. 15; sketched at renderer_dynamic.py:242-245) in its O(T)
    form, in the dtype of the inputs: weights, z_vals [N, T] (z non-decreasing along a row), nears, fars [N] -> [N].  With the
    compositor's intervals delta_i = z_{i+1} - z_i, delta_{T-1} = R / T, R = far - near:
      m_i = (z_i + delta_i / 2 - near) / R, d_i = delta_i / R,
      ray = sum_ij w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 d_i = 2 sum_i w_i (m_i W_<i - M_<i) + 1/3 sum_i w_i^2 d_i
    (W_<i, M_<i: exclusive prefix sums of w and w m).  A ray whose R is not finite or not > 0 gives 0 and no gradient."""
    N, T = weights.shape
    near, R = nears.reshape(N, 1), (fars - nears).reshape(N, 1)
    ok = torch.isfinite(R) & (R > 0)
    zero = torch.zeros((), dtype=weights.dtype, device=weights.device)
    w, z, near, R = torch.where(ok, weights, zero), torch.where(ok, z_vals, zero), torch.where(ok, near, zero), torch.where(ok, R, zero + 1)
    delta = torch.cat([z[:, 1:] - z[:, :-1], R / T], dim=1)
    m, d = (z + delta / 2 - near) / R, delta / R
    head = torch.zeros(N, 1, dtype=w.dtype, device=w.device)
    w_lt = torch.cat([head, torch.cumsum(w, dim=1)[:, :-1]], dim=1)
    m_lt = torch.cat([head, torch.cumsum(w * m, dim=1)[:, :-1]], dim=1)
    return 2 * (w * (m * w_lt - m_lt)).sum(dim=1) + (w * w * d).sum(dim=1) / 3


def distortion_loss(weights, z_vals, nears, fars, alpha):
    """alpha x the mean over the N rays of `distortion_ray_losses` (a ray that gives 0 still counts in N): the host branch of
    `RenderTrainStep.losses`, and evaluated in float64 the formulation the device kernels are tested against."""
    N = weights.shape[0]
    if N == 0:
        return weights.sum() * 0
    return alpha * distortion_ray_losses(weights, z_vals, nears, fars).sum() / N


class DistortionLossFn(torch.autograd.Function):
    """distortion_loss on the device (nvsf_distortion_loss_fwd / _bwd, csrc/losses.hip): weights, z_vals [N, T], nears, fars [N] (any
    shape with N elements), alpha a Python float -> scalar, or (scalar, per-ray losses [N]) with ray_losses=True.  One scan per ray each
    way in fp64 (one wave per ray), the row totals kept for the backward.  Gradient to `weights` only."""

    @staticmethod
    def forward(ctx, weights, z_vals, nears, fars, alpha, ray_losses=False):
        from nvsf import _hip
        w, z, near, far = _f32(weights), _f32(z_vals), _f32(nears).view(-1), _f32(fars).view(-1)
        if w.dim() != 2 or z.shape != w.shape or near.numel() != w.shape[0] or far.numel() != w.shape[0]:
            raise ValueError(f"DistortionLossFn: weights {tuple(weights.shape)}, z_vals {tuple(z_vals.shape)}, nears {tuple(nears.shape)} and "
                             f"fars {tuple(fars.shape)} do not describe one [N, T] sample batch")
        N, T = w.shape
        out = torch.empty((), dtype=torch.float32, device=w.device)
        rays = torch.empty(N, dtype=torch.float32, device=w.device) if ray_losses else None
        state = torch.empty(N, 2, dtype=torch.float64, device=w.device)
        ws = torch.empty(max(1, (N + 3) // 4), dtype=torch.float64, device=w.device)  # one partial per workgroup of four rays
        _hip.call("nvsf_distortion_loss_fwd", _hip.ptr(w), _hip.ptr(z), _hip.ptr(near), _hip.ptr(far), N, T, float(alpha), _hip.ptr(ws),
                  8 * ws.numel(), _hip.ptr(rays), _hip.ptr(out), _hip.ptr(state))
        ctx.save_for_backward(w, z, near, far, state)
        ctx.alpha, ctx.shape = float(alpha), weights.shape
        if ray_losses:
            ctx.mark_non_differentiable(rays)
            return out, rays
        return out

    @staticmethod
    def backward(ctx, grad, _g_rays=None):
        from nvsf import _hip
        w, z, near, far, state = ctx.saved_tensors
        grad_w = torch.empty_like(w)
        _hip.call("nvsf_distortion_loss_bwd", _hip.ptr(w), _hip.ptr(z), _hip.ptr(near), _hip.ptr(far), w.shape[0], w.shape[1], ctx.alpha,
                  _hip.ptr(state), _hip.ptr(_f32_or_none(grad)), _hip.ptr(grad_w))
        return grad_w.view(ctx.shape), None, None, None, None, None


class LidarLossFn(torch.autograd.Function):
    """The LiDAR terms of Trainer.train_step (trainer.py:187-219) as one HIP launch forward and one backward (csrc/losses.hip): at
    4096 rays each of the ~60 elementwise / reduction launches the expression costs under autograd is a launch latency.
    Returns (loss_depth, loss_raydrop, loss_intensity, pred_depth [1,N], pred_points [1,N,3], gt_points [1,N,3]); the point clouds
    are the inputs of the chamfer term (None when `rays_d` is None)."""

    ENTRIES = ("nvsf_lidar_losses_fwd", "nvsf_lidar_losses_bwd")

    @staticmethod
    def forward(ctx, image_lidar, depth_lidar, gt_rd, gt_i, gt_d, rays_d, alpha_d, alpha_r, alpha_i, smooth, scale):
        return LidarLossFn._forward(ctx, LidarLossFn.ENTRIES, (), image_lidar, depth_lidar, gt_rd, gt_i, gt_d, rays_d, alpha_d, alpha_r, alpha_i,
                                    smooth, scale)

    @staticmethod
    def _forward(ctx, entries, crit, image_lidar, depth_lidar, gt_rd, gt_i, gt_d, rays_d, alpha_d, alpha_r, alpha_i, smooth, scale):
        """entries: the (forward, backward) entry points; crit: the criterion arguments of the `_crit` pair ((kind, parameter) per term),
        () for the default pair."""
        from nvsf import _hip
        N, dev = depth_lidar.numel(), depth_lidar.device
        img, dep, rd, gi, gd = _f32(image_lidar), _f32(depth_lidar), _f32(gt_rd), _f32(gt_i), _f32(gt_d)
        dirs = _f32(rays_d) if rays_d is not None else None
        l = [torch.empty((), dtype=torch.float32, device=dev) for _ in range(3)]
        pred_depth = torch.empty(1, N, dtype=torch.float32, device=dev)
        pp = torch.empty(1, N, 3, dtype=torch.float32, device=dev) if dirs is not None else None
        gp = torch.empty(1, N, 3, dtype=torch.float32, device=dev) if dirs is not None else None
        _hip.call(entries[0], _hip.ptr(img), _hip.ptr(dep), _hip.ptr(rd), _hip.ptr(gi), _hip.ptr(gd), _hip.ptr(dirs), N,
                  float(alpha_d), float(alpha_r), float(alpha_i), float(smooth), float(scale), *crit, _hip.ptr(l[0]), _hip.ptr(l[1]), _hip.ptr(l[2]),
                  _hip.ptr(pred_depth), _hip.ptr(pp), _hip.ptr(gp))
        ctx.save_for_backward(img, dep, rd, gi, gd, dirs)
        ctx.consts = (float(alpha_d), float(alpha_r), float(alpha_i), float(smooth), float(scale), image_lidar.shape, depth_lidar.shape)
        ctx.entries, ctx.crit = entries, tuple(crit)
        if gp is not None:
            ctx.mark_non_differentiable(gp)
        return l[0], l[1], l[2], pred_depth, pp, gp

    @staticmethod
    def backward(ctx, g_d, g_r, g_i, g_pd, g_pp, _g_gp):
        from nvsf import _hip
        img, dep, rd, gi, gd, dirs = ctx.saved_tensors
        a_d, a_r, a_i, smooth, scale, shape_img, shape_dep = ctx.consts
        N = dep.numel()
        g_d, g_r, g_i, g_pd, g_pp = (_f32_or_none(g) for g in (g_d, g_r, g_i, g_pd, g_pp))
        grad_img, grad_dep = torch.empty_like(img), torch.empty_like(dep)
        _hip.call(ctx.entries[1], _hip.ptr(img), _hip.ptr(dep), _hip.ptr(rd), _hip.ptr(gi), _hip.ptr(gd), _hip.ptr(dirs), N,
                  a_d, a_r, a_i, smooth, scale, *ctx.crit, _hip.ptr(g_d), _hip.ptr(g_r), _hip.ptr(g_i), _hip.ptr(g_pd), _hip.ptr(g_pp),
                  _hip.ptr(grad_img), _hip.ptr(grad_dep))
        return (grad_img.view(shape_img), grad_dep.view(shape_dep)) + (None,) * (10 if ctx.crit else 9)


def lidar_criteria_args(criteria, scale):
    """criteria = (depth_loss, raydrop_loss, intensity_loss) names -> the six criterion arguments of the `_crit` LiDAR entries."""
    args = []
    for option, name in zip(("depth_loss", "raydrop_loss", "intensity_loss"), criteria):
        kind, param = per_ray_criterion(option, name, scale)
        args += [kind, float(param)]
    return tuple(args)


class LidarCritLossFn(torch.autograd.Function):
    """LidarLossFn with the criterion of each term chosen (`--depth_loss`, `--raydrop_loss`, `--intensity_loss`, main_nvsf.py:85-88):
    nvsf_lidar_losses_crit_fwd / _bwd, still one launch each way.  criteria = (depth, raydrop, intensity) names.  With raydrop "bce" the
    prediction passes a sigmoid and then BCEWithLogitsLoss's own (trainer.py:208-209), as the reference trains."""
    ENTRIES = ("nvsf_lidar_losses_crit_fwd", "nvsf_lidar_losses_crit_bwd")

    @staticmethod
    def forward(ctx, image_lidar, depth_lidar, gt_rd, gt_i, gt_d, rays_d, alpha_d, alpha_r, alpha_i, smooth, scale, criteria):
        return LidarLossFn._forward(ctx, LidarCritLossFn.ENTRIES, lidar_criteria_args(criteria, scale), image_lidar, depth_lidar, gt_rd, gt_i,
                                    gt_d, rays_d, alpha_d, alpha_r, alpha_i, smooth, scale)

    backward = staticmethod(LidarLossFn.backward)


def lidar_losses_host(image_lidar, depth_lidar, gt_rd, gt_i, gt_d, rays_d, alpha_d, alpha_r, alpha_i, smooth, scale, criteria=None):
    """LidarLossFn / LidarCritLossFn as torch expressions (trainer.py:187-219, 229-233): the host branch of `RenderTrainStep.losses`.  Same
    arguments and the same six results; criteria = (depth, raydrop, intensity) names, None = the defaults (l1, mse, mse)."""
    gt_int, gt_depth = gt_i * gt_rd, gt_d * gt_rd  # trainer.py:187-189
    pred_rd = image_lidar[:, :, 0]
    pred_int = image_lidar[:, :, 1] * gt_rd
    pred_depth = depth_lidar * gt_rd
    if criteria is None:
        l_depth = (alpha_d * (pred_depth - gt_depth).abs()).sum()
        l_raydrop = (alpha_r * (pred_rd - gt_rd.clamp(smooth, 1 - smooth)) ** 2).sum()
        l_intensity = (alpha_i * (pred_int - gt_int) ** 2).sum()
    else:
        crit_d, crit_r, crit_i = (torch_criterion(name, scale, option) for option, name in
                                  zip(("depth_loss", "raydrop_loss", "intensity_loss"), criteria))
        if criteria[1] == "bce":
            pred_rd = torch.sigmoid(pred_rd)  # trainer.py:208-209: a sigmoid ahead of BCEWithLogitsLoss's own
        l_depth = (alpha_d * crit_d(pred_depth, gt_depth)).sum()
        l_raydrop = (alpha_r * crit_r(pred_rd, gt_rd.clamp(smooth, 1 - smooth))).sum()
        l_intensity = (alpha_i * crit_i(pred_int, gt_int)).sum()
    pred_pts, gt_pts = (None, None) if rays_d is None else (rays_d * pred_depth.unsqueeze(-1) / scale, rays_d * gt_depth.unsqueeze(-1) / scale)
    return l_depth, l_raydrop, l_intensity, pred_depth, pred_pts, gt_pts


class MseSumFn(torch.autograd.Function):
    """sum(alpha (a - b)^2) -- the camera term (trainer.py:491-503, summed at :540-543) -- as one launch each way."""

    @staticmethod
    def forward(ctx, a, b, alpha):
        from nvsf import _hip
        a32, b32 = _f32(a), _f32(b)
        out = torch.empty((), dtype=torch.float32, device=a.device)
        _hip.call("nvsf_mse_sum_fwd", _hip.ptr(a32), _hip.ptr(b32), a32.numel(), float(alpha), _hip.ptr(out))
        ctx.save_for_backward(a32, b32)
        ctx.alpha, ctx.shape = float(alpha), a.shape
        return out

    @staticmethod
    def backward(ctx, g):
        from nvsf import _hip
        a32, b32 = ctx.saved_tensors
        grad = torch.empty_like(a32)
        _hip.call("nvsf_mse_sum_bwd", _hip.ptr(a32), _hip.ptr(b32), a32.numel(), ctx.alpha, _hip.ptr(_f32_or_none(g)), _hip.ptr(grad))
        return grad.view(ctx.shape), None, None


class CritSumFn(torch.autograd.Function):
    """sum(alpha crit(a, b)): the camera term under `--rgb_loss` (main_nvsf.py:83, trainer.py:503), one launch each way
    (nvsf_crit_sum_fwd / _bwd).  criterion: a name of PER_RAY_CRITERIA."""

    @staticmethod
    def forward(ctx, a, b, alpha, criterion, scale):
        from nvsf import _hip
        kind, param = per_ray_criterion("rgb_loss", criterion, scale)
        a32, b32 = _f32(a), _f32(b)
        out = torch.empty((), dtype=torch.float32, device=a.device)
        ctx.args = (_hip.ptr(a32), _hip.ptr(b32), a32.numel(), float(alpha), kind, float(param))
        _hip.call("nvsf_crit_sum_fwd", *ctx.args, _hip.ptr(out))
        ctx.save_for_backward(a32, b32)
        ctx.shape = a.shape
        return out

    @staticmethod
    def backward(ctx, g):
        from nvsf import _hip
        a32, _ = ctx.saved_tensors
        grad = torch.empty_like(a32)
        _hip.call("nvsf_crit_sum_bwd", *ctx.args, _hip.ptr(_f32_or_none(g)), _hip.ptr(grad))
        return grad.view(ctx.shape), None, None, None, None


def rgb_loss_host(image, gt_rgb, alpha_rgb, criterion, scale):
    """The colour term as torch expressions: the host branch of `RenderTrainStep.losses` (MSE spelled out as it always was)."""
    if criterion == "mse":
        return (alpha_rgb * (image - gt_rgb) ** 2).sum()
    return (alpha_rgb * torch_criterion(criterion, scale, "rgb_loss")(image, gt_rgb)).sum()


class CameraLossFn(torch.autograd.Function):
    """The two camera terms of Trainer.train_step with `--use_rgbd_loss` (trainer.py:491-518) as one launch each way
    (nvsf_camera_loss_fwd / _bwd): sum alpha_rgb (image - gt_rgb)^2 and the depth term against the LiDAR-projected depth map --
    gt = gt_depth_m * scale capped at 80 * scale, the rendered depth capped the same way (a capped ray gets no gradient), mask = gt > 0,
    alpha_rd * sum criterion(depth * mask, gt * mask).  criterion: `--rgb_depth_loss` (main_nvsf.py:91, 205-212).
    Returns (loss_rgb, loss_rgb_depth)."""
    CRITERIA = {"l1": 0, "mse": 1, "huber": 2, "smoothl1": 3, "bce": 4}  # no "cos": CosineSimilarity over dim 1 of a [B, N] pair is no per-ray loss

    @staticmethod
    def criterion_code(criterion, scale):
        return criterion_code(criterion, scale, CameraLossFn.CRITERIA, ("rgb_depth_loss", 91))

    ENTRIES = ("nvsf_camera_loss_fwd", "nvsf_camera_loss_bwd")

    @staticmethod
    def forward(ctx, image, depth, gt_rgb, gt_depth_m, alpha_rgb, alpha_rd, scale, criterion):
        return CameraLossFn._forward(ctx, CameraLossFn.ENTRIES, (), image, depth, gt_rgb, gt_depth_m, alpha_rgb, alpha_rd, scale, criterion)

    @staticmethod
    def _forward(ctx, entries, rgb_crit, image, depth, gt_rgb, gt_depth_m, alpha_rgb, alpha_rd, scale, criterion):
        """entries: the (forward, backward) entry points; rgb_crit: (kind, parameter) of the colour term for the `_crit` pair, () = MSE."""
        from nvsf import _hip
        kind, param = CameraLossFn.criterion_code(criterion, scale)
        img, dep, rgb, gtd = _f32(image), _f32(depth), _f32(gt_rgb), _f32(gt_depth_m)
        N = dep.numel()
        if img.numel() != 3 * N or rgb.numel() != 3 * N or gtd.numel() != N:
            raise ValueError(f"CameraLossFn: image {tuple(image.shape)}, gt_rgb {tuple(gt_rgb.shape)}, depth {tuple(depth.shape)} and "
                             f"gt_rgb_depth {tuple(gt_depth_m.shape)} do not describe one ray batch")
        out = [torch.empty((), dtype=torch.float32, device=dep.device) for _ in range(2)]
        args = (_hip.ptr(img), _hip.ptr(rgb), _hip.ptr(dep), _hip.ptr(gtd), N, float(alpha_rgb), float(alpha_rd), float(scale),
                80 * float(scale), kind, float(param), *rgb_crit)
        _hip.call(entries[0], *args, _hip.ptr(out[0]), _hip.ptr(out[1]))
        ctx.save_for_backward(img, rgb, dep, gtd)
        ctx.args, ctx.shapes, ctx.entries, ctx.n_in = args, (image.shape, depth.shape), entries, 8 + (1 if rgb_crit else 0)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_rgb, g_depth):
        from nvsf import _hip
        img, _, dep, _ = ctx.saved_tensors
        g_rgb, g_depth = _f32_or_none(g_rgb), _f32_or_none(g_depth)
        grad_img, grad_dep = torch.empty_like(img), torch.empty_like(dep)
        _hip.call(ctx.entries[1], *ctx.args, _hip.ptr(g_rgb), _hip.ptr(g_depth), _hip.ptr(grad_img), _hip.ptr(grad_dep))
        return (grad_img.view(ctx.shapes[0]), grad_dep.view(ctx.shapes[1])) + (None,) * (ctx.n_in - 2)


class CameraCritLossFn(torch.autograd.Function):
    """CameraLossFn with the colour term under `--rgb_loss` instead of MSE (nvsf_camera_loss_crit_fwd / _bwd): `use_rgbd_loss` with a
    non-default `rgb_loss`, still one launch each way.  Returns (loss_rgb, loss_rgb_depth)."""
    ENTRIES = ("nvsf_camera_loss_crit_fwd", "nvsf_camera_loss_crit_bwd")

    @staticmethod
    def forward(ctx, image, depth, gt_rgb, gt_depth_m, alpha_rgb, alpha_rd, scale, criterion, rgb_criterion):
        kind, param = per_ray_criterion("rgb_loss", rgb_criterion, scale)
        return CameraLossFn._forward(ctx, CameraCritLossFn.ENTRIES, (kind, float(param)), image, depth, gt_rgb, gt_depth_m, alpha_rgb, alpha_rd,
                                     scale, criterion)

    backward = staticmethod(CameraLossFn.backward)


def rgb_depth_loss_host(depth, gt_depth_m, scale, criterion, alpha_rd):
    """The depth term of CameraLossFn as torch expressions (trainer.py:506-518): the host branch of `RenderTrainStep.losses` and the
    formulation the device kernels are tested against."""
    crit = torch_criterion(criterion, scale)
    max_depth = 80 * scale
    gt = (gt_depth_m * scale).clamp(max=max_depth)
    pred = torch.where(depth > max_depth, torch.full_like(depth, max_depth), depth)  # assignment into the tensor: no gradient there
    mask = (gt > 0).to(pred.dtype)
    return (alpha_rd * crit(pred * mask, gt * mask)).sum()


class LidarGradLossFn(torch.autograd.Function):
    """Structural regularisation of trainer.py:296-470 in its `grad_loss` form as one launch each way (nvsf_lidar_grad_loss_fwd / _bwd):
    pred_depth, gt_depth [1, N] the masked ranges (scene units), gt_raydrop [1, N], pano_inds int64 [1, N] pixel indices of the batch
    (N / (pH pW) patches in patch order), pano_frame [H, W, 3] (or [1, H, W, 3]) the frame's ground truth (channel 2 = range x scale).
    criterion: `--depth_grad_loss` (main_nvsf.py:86, 204-221); sobel: `--sobel_grad` (:107)."""
    CRITERIA = {"l1": 0, "mse": 1, "huber": 2, "smoothl1": 3, "cos": 4}

    @staticmethod
    def forward(ctx, pred_depth, gt_depth, gt_raydrop, pano_inds, pano_frame, patch, scale, criterion, alpha, sobel=False):
        from nvsf import _hip
        kind, param = criterion_code(criterion, scale, LidarGradLossFn.CRITERIA, ("depth_grad_loss", 86))
        pd, gd, rd = _f32(pred_depth), _f32(gt_depth), _f32(gt_raydrop)
        inds = pano_inds.detach().long().contiguous()
        frame = pano_frame.detach().float()
        frame = frame[0] if frame.dim() == 4 else frame
        frame = frame.contiguous()
        H, W, C = frame.shape
        if C < 3:  # the reference reads data['pano_frame'][0, ..., 2] (trainer.py:296-470): the range channel is channel 2
            raise ValueError(f"LidarGradLossFn: pano_frame needs >= 3 channels [raydrop, intensity, range], got {C}")
        pH, pW = int(patch[0]), int(patch[1])
        N = pd.numel()
        out = torch.empty((), dtype=torch.float32, device=pd.device)
        stats = torch.empty(N // (pH * pW), 6, dtype=torch.float32, device=pd.device) if criterion == "cos" else None
        args = (_hip.ptr(pd), _hip.ptr(gd), _hip.ptr(rd), _hip.ptr(inds), frame.data_ptr() + 4 * 2, C, N, pH, pW, H, W,
                float(scale), kind, float(param), float(alpha), 1 if sobel else 0, _hip.ptr(stats))
        _hip.call("nvsf_lidar_grad_loss_fwd", *args, _hip.ptr(out))
        ctx.save_for_backward(pd, gd, rd, inds, frame, *(() if stats is None else (stats,)))
        ctx.args, ctx.shape = args, pred_depth.shape
        return out

    @staticmethod
    def backward(ctx, g):
        from nvsf import _hip
        pd = ctx.saved_tensors[0]
        grad = torch.empty_like(pd)
        _hip.call("nvsf_lidar_grad_loss_bwd", *ctx.args, _hip.ptr(_f32_or_none(g)), _hip.ptr(grad))
        return (grad.view(ctx.shape),) + (None,) * 9


def update_error_map(frames, idx, modality, stash, inds, alphas, smooth=0.0, criteria=None, scale=1.0):
    """trainer.py:552-630 on the device for one modality of frame `idx` of the FrameSet `frames`: per-ray loss -> min / max ->
    normalised to [1, 1000] -> EMA into the frame's coarse map at the rays' pixels `inds` (a handful of small launches, no host read).
    modality "lidar": stash = (image_lidar, depth_lidar, gt_raydrop, gt_intensity, gt_range), alphas = (alpha_d, alpha_r, alpha_i);
    "camera": stash = (image, gt_rgb), alphas = (alpha_rgb,).  A FrameSet without that modality's map is left alone.
    criteria: the criteria the step trains with, (depth, raydrop, intensity) names / (rgb,) name (with `scale` for Huber's delta);
    None = the defaults and their entries.  The `_crit` entries write the true (min, max), negative values included."""
    from nvsf import _hip
    lidar = modality == "lidar"
    emap, H, W = (frames.error_map, frames.H_lidar, frames.W_lidar) if lidar else (frames.error_map_rgb, frames.H, frames.W)
    if emap is None:
        return
    inds = inds.detach().long().contiguous().view(-1)
    N, dev = inds.numel(), inds.device
    ray_loss = torch.empty(N, dtype=torch.float32, device=dev)
    stats = frames.error_map_stats(dev)
    if lidar:
        img, dep, rd, gi, gd = (_f32(t) for t in stash)
        if criteria is None:
            _hip.call("nvsf_lidar_ray_losses", _hip.ptr(img), _hip.ptr(dep), _hip.ptr(rd), _hip.ptr(gi), _hip.ptr(gd), N, *alphas, smooth,
                      _hip.ptr(ray_loss), _hip.ptr(stats))
        else:
            _hip.call("nvsf_lidar_ray_losses_crit", _hip.ptr(img), _hip.ptr(dep), _hip.ptr(rd), _hip.ptr(gi), _hip.ptr(gd), N, *alphas, smooth,
                      *lidar_criteria_args(criteria, scale), _hip.ptr(ray_loss), _hip.ptr(stats))
    else:
        img, gt = (_f32(t) for t in stash)
        if criteria is None:
            _hip.call("nvsf_mse_rows", _hip.ptr(img), _hip.ptr(gt), N, img.shape[-1], *alphas, _hip.ptr(ray_loss), _hip.ptr(stats))
        else:
            kind, param = per_ray_criterion("rgb_loss", criteria[0], scale)
            _hip.call("nvsf_crit_rows", _hip.ptr(img), _hip.ptr(gt), N, img.shape[-1], *alphas, kind, float(param), _hip.ptr(ray_loss),
                      _hip.ptr(stats))
    eH, eW = emap.shape[-2:]
    _hip.call("nvsf_error_map_update", _hip.ptr(ray_loss), _hip.ptr(inds), N, int(W), emap[idx].data_ptr(), int(eH), int(eW), float(eH / H),
              float(eW / W), _hip.ptr(stats), _hip.ptr(frames.error_map_owner(dev, eH * eW)))
