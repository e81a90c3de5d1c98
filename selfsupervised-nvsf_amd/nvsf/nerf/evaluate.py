"""Whole-frame evaluation, no part of training (nvsf/nerf/train_step.py): the reference's Trainer.eval_step / test_step
(nvsf/nerf/trainer.py:658-903) and the metric half of its evaluate_one_epoch (:1458-1560) -- host-side PSNR and depth RMSE in metres
(nvsf/lib/error_matrices.py:48-57, 263-285), PointsMeter (:299-356) on csrc/chamfer.hip, the device table of nvsf/nerf/meters.py."""
import numpy as np
import torch

from nvsf import frame_shard
from nvsf.nerf import meters as M


def psnr(pred, truth):
    """-10 log10(mean((p - t)^2) + 1e-8), images in [0, 1]."""
    p, t = (np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=np.float64) for a in (pred, truth))
    return float(-10 * np.log10(np.mean((p - t) ** 2) + 1e-8))


def depth_rmse(pred, truth, scale, min_depth=1e-6, max_depth=80.0):
    """RMSE in metres: both ranges divided by the scene scale and clamped to [1e-6, 80] m."""
    p, t = (np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=np.float64) / scale for a in (pred, truth))
    p, t = np.clip(p, min_depth, max_depth), np.clip(t, min_depth, max_depth)
    return float(np.sqrt(np.mean((t - p) ** 2)))


def fscore(dist1, dist2, threshold=0.001):
    """F-score of two point clouds from their SQUARED nearest-neighbour distances [B, n] / [B, m] (nvsf/lib/error_matrices.py:12-26):
    2 p r / (p + r) with p, r the fractions below `threshold`, 0 where both are 0.  Returns fscore, precision, recall ([B])."""
    p1 = (dist1 < threshold).float().mean(dim=1)
    p2 = (dist2 < threshold).float().mean(dim=1)
    f = 2 * p1 * p2 / (p1 + p2)
    return torch.nan_to_num(f, nan=0.0), p1, p2


def pano_to_lidar(pano, intrinsics, intrinsics_hoz=(180.0, 360.0)):
    """Range image [H, W] -> points [n, 3] in the LiDAR frame, on the device of `pano` (nvsf/lib/convert.py:221-291): pixel (row j,
    column i) looks along azimuth beta = -(i - W / 2) / W * fov_hoz and elevation alpha = fov_up - j / H * fov (degrees; `intrinsics` =
    (fov_up, fov), `intrinsics_hoz` = (fov_hoz_up, fov_hoz)).  Pixels of range exactly 0 (dropped rays, ~30 % of a KITTI-360 frame) give
    no point -- the reference filters them with `np.where(pano != 0.0)` (convert.py:262-266) before the chamfer distance sees the
    cloud -- so n <= H * W, in row-major pixel order (one device->host read for the count; this is evaluation code)."""
    H, W = pano.shape
    fov_up, fov = (float(v) for v in intrinsics)
    fov_hoz = float(intrinsics_hoz[1])
    i = torch.arange(W, dtype=torch.float32, device=pano.device)[None, :]
    j = torch.arange(H, dtype=torch.float32, device=pano.device)[:, None]
    beta = -(i - W / 2) / W * fov_hoz / 180 * np.pi
    alpha = (fov_up - j / H * fov) / 180 * np.pi
    dirs = torch.stack([torch.cos(alpha) * torch.cos(beta), torch.cos(alpha) * torch.sin(beta), torch.sin(alpha).expand(H, W)], -1)
    pano = pano.float()
    return (dirs * pano[..., None])[pano != 0.0]


class PointsMeter:
    """Chamfer distance and F-score of whole rendered range images against the measured ones -- the reference's PointsMeter
    (nvsf/lib/error_matrices.py:299-356: ranges divided by the scene scale, pano_to_lidar with the sensor's intrinsics,
    CD = mean d1 + mean d2 over squared distances, F-score at 0.05) with the clouds built on the device and the nearest neighbours
    from the HIP chamfer kernel (csrc/chamfer.hip), which also serves the training loss."""

    def __init__(self, scale, intrinsics, intrinsics_hoz=(180.0, 360.0), threshold=0.05):
        self.scale, self.intrinsics, self.intrinsics_hoz, self.threshold = float(scale), intrinsics, intrinsics_hoz, threshold
        self.clear()

    def clear(self):
        self.V, self.N = [], 0

    def update(self, preds, truths):
        """preds, truths: [1, H, W] (or [H, W]) range images in scene units."""
        from nvsf.nerf.chamfer3D.dist_chamfer_3D import chamfer_3DDist
        p, t = (a.reshape(a.shape[-2], a.shape[-1]).float() / self.scale for a in (preds, truths))
        with torch.no_grad():
            cp, ct = pano_to_lidar(p, self.intrinsics, self.intrinsics_hoz), pano_to_lidar(t, self.intrinsics, self.intrinsics_hoz)
            if cp.shape[0] == 0 or ct.shape[0] == 0:
                # a cloud without points (e.g. every predicted pixel gated off by the ray-drop mask): the reference's means over
                # an empty distance array are NaN and its F-score 0 / 0 -> 0 (error_matrices.py:12-26, 322-335)
                cd, f = float("nan"), 0.0
            else:
                d1, d2, _, _ = chamfer_3DDist()(cp[None], ct[None])
                cd = d1.mean() + d2.mean()
                f = fscore(d1, d2, self.threshold)[0][0]
        self.V.append([float(cd), float(f)])
        self.N += 1

    def measure(self):
        assert self.N == len(self.V), "prediction and gt should should be equal"
        return np.array(self.V).mean(0)

    def report(self):
        cd, f = self.measure()
        return f"Points_error(CD, F-score) = {[round(float(cd), 3), round(float(f), 3)]}"


def _predict_frame(model, data, num_steps, lidar_hw, camera_hw, gate, raydrop_thres, max_ray_batch, split_rays, refiner, bg_color=None,
                   perturb=False, **render_kwargs):
    """The frame prediction eval_step and test_step share, under the caller's no_grad: the staged render of the LiDAR frame, reshaped to
    [B, Hl, Wl], then the refiner per frame or the `pred_raydrop > raydrop_thres` gate; `gate` False (test_step at alpha_r = 0) leaves
    intensity and range as rendered and keeps only the refiner's probability.  Returns (pred_raydrop, pred_intensity, pred_depth, camera);
    `camera()` renders the camera frame over `bg_color` (None: white) -> (pred_rgb [B, H, W, 3], pred_rgb_depth [B, H, W]) -- a second
    call, so that what the caller does with the LiDAR planes (loss terms, masks) is still enqueued between the two renders."""
    render = (lambda *a, **k: frame_shard.render_sharded(model, *a, **k)) if split_rays else \
        (lambda o, d, t, **k: model.render(o, d, t, staged=True, **k))  # the whole frame on this rank (evaluate_frames(shard="frames"))
    common = dict(num_steps=num_steps, max_ray_batch=max_ray_batch, perturb=perturb, **render_kwargs)
    B, (Hl, Wl), (H, W) = data["rays_o_lidar"].shape[0], lidar_hw, camera_hw
    o = render(data["rays_o_lidar"], data["rays_d_lidar"], data["time"], cal_lidar_color=True, **common)
    img = o["image_lidar"].reshape(B, Hl, Wl, 2)
    pred_raydrop, pred_intensity, pred_depth = img[..., 0], img[..., 1], o["depth_lidar"].reshape(B, Hl, Wl)
    if refiner is not None:
        refined = [refiner(pred_raydrop[b].float(), pred_intensity[b].float(), pred_depth[b].float(), thres=raydrop_thres if gate else None)
                   for b in range(B)]
        if gate:  # the U-Net's last kernel wrote the gated planes
            pred_raydrop, pred_intensity, pred_depth = (torch.stack([f[k] for f in refined]) for k in range(3))
        else:
            pred_raydrop = torch.stack(refined)
    elif gate:
        mask = (pred_raydrop > raydrop_thres).to(pred_depth.dtype)
        pred_intensity, pred_depth = pred_intensity * mask, pred_depth * mask

    def camera():
        c = render(data["rays_o"], data["rays_d"], data["time"], bg_color=1 if bg_color is None else bg_color, **common)
        return c["image"].reshape(B, H, W, 3), c["depth"].reshape(B, H, W)
    return pred_raydrop, pred_intensity, pred_depth, camera


def eval_step(model, data, num_steps, alpha_d=1.0, alpha_r=0.01, alpha_i=0.1, alpha_rgb=1.0, raydrop_thres=0.5, max_ray_batch=4096,
              split_rays=True, refiner=None, **render_kwargs):
    """Whole-frame evaluation of one frame, the reference's Trainer.eval_step (nvsf/nerf/trainer.py:658-815):
    `data` = FrameSet(..., training=False).collate([i]) -- every pixel of the range image and of the camera image.  `refiner`: a
    RaydropRefiner (nvsf/nerf/refine.py); with one, `pred_raydrop` becomes the U-Net's refined probability of the rendered
    (ray-drop, intensity, range) planes and the gate below uses it (:721-733, the shipped configuration's `use_refine`), one HIP
    forward per frame whose last kernel also writes the gated intensity and range.  None: the field's own probability.  Both modalities go through the staged render, a frame's rays split over the ranks (frame_shard.render_sharded); the
    predicted ray-drop mask (`pred_raydrop > raydrop_thres`, :726) gates predicted intensity and range, the ground truth is gated by
    its own mask (:695-696); loss = the reference's mean-reduced L1 range + MSE ray-drop + MSE intensity + MSE RGB (:733-737, :795-796;
    criteria as main_nvsf.py:205-221).  Returns a dict of [B, H, W(, C)] predictions / ground truths and `loss`."""
    loss = torch.zeros((), device=data["rays_o_lidar"].device)
    with torch.no_grad():
        gl, gi = data["images_lidar"], data["images"]  # [B, H, W, 3] = raydrop, intensity, range; [B, H, W, 3 or 4]
        gt_raydrop = gl[..., 0]
        gt_intensity, gt_depth = gl[..., 1] * gt_raydrop, gl[..., 2] * gt_raydrop
        pred_raydrop, pred_intensity, pred_depth, camera = _predict_frame(
            model, data, num_steps, gl.shape[1:3], gi.shape[1:3], True, raydrop_thres, max_ray_batch, split_rays, refiner, **render_kwargs)
        loss = loss + alpha_d * (pred_depth - gt_depth).abs().mean() + alpha_r * ((pred_raydrop - gt_raydrop) ** 2).mean() \
            + alpha_i * ((pred_intensity - gt_intensity) ** 2).mean()
        gt_rgb = gi[..., :3] * gi[..., 3:] + (1 - gi[..., 3:]) if gi.shape[-1] == 4 else gi  # fixed white background (:774-781)
        pred_rgb, pred_rgb_depth = camera()
        loss = loss + alpha_rgb * ((pred_rgb - gt_rgb) ** 2).mean()
        out = dict(pred_raydrop=pred_raydrop, pred_intensity=pred_intensity, pred_depth=pred_depth, gt_raydrop=gt_raydrop,
                   gt_intensity=gt_intensity, gt_depth=gt_depth, pred_rgb=pred_rgb, pred_rgb_depth=pred_rgb_depth, gt_rgb=gt_rgb, loss=loss)
        if "image_depths" in data:  # the LiDAR-projected camera depth map, metres (trainer.py:761-762)
            out["gt_rgb_depth"] = data["image_depths"].reshape(pred_rgb_depth.shape)
    return out


def test_step(model, data, num_steps, alpha_r=0.01, raydrop_thres=0.5, max_ray_batch=4096, split_rays=True, refiner=None, bg_color=None,
              perturb=False, **render_kwargs):
    """Predictions of one whole frame without ground truth, the reference's Trainer.test_step (nvsf/nerf/trainer.py:817-903): `data` =
    FrameSet(..., training=False[, sensor=SensorChange(...)]).collate([i]).  Both modalities go through the staged render as in
    eval_step (a frame's rays split over the ranks unless split_rays=False); with a `refiner` the ray-drop plane becomes the U-Net's
    refined probability (:865-867); the mask `pred_raydrop > raydrop_thres` gates intensity and range only when alpha_r > 0 (:870-875);
    `data["masks_lidar"]` [B, H_lidar, W_lidar] multiplies range, ray-drop and intensity, `data["masks"]` [B, H, W, 1] the image
    (:876-879, 897-898).  bg_color None is the white background eval_step fixes; perturb jitters the samples.
    Returns (pred_rgb [B, H, W, 3], pred_rgb_depth [B, H, W], pred_raydrop, pred_intensity, pred_depth [B, H_lidar, W_lidar])."""
    with torch.no_grad():
        Hl, Wl, H, W = (int(data[k]) for k in ("H_lidar", "W_lidar", "H", "W"))  # a sensor= FrameSet carries no images
        pred_raydrop, pred_intensity, pred_depth, camera = _predict_frame(
            model, data, num_steps, (Hl, Wl), (H, W), alpha_r > 0, raydrop_thres, max_ray_batch, split_rays, refiner, bg_color, perturb, **render_kwargs)
        if "masks_lidar" in data:
            m = data["masks_lidar"].reshape(-1, Hl, Wl)
            pred_depth, pred_raydrop, pred_intensity = pred_depth * m, pred_raydrop * m, pred_intensity * m
        pred_rgb, pred_rgb_depth = camera()
        if "masks" in data:
            pred_rgb = pred_rgb * data["masks"].reshape(pred_rgb.shape[0], H, W, 1)
    return pred_rgb, pred_rgb_depth, pred_raydrop, pred_intensity, pred_depth


test_step.__test__ = False  # a library function, not a test


_LISTS = {"depth": 5, "intensity": 5, "raydrop": 3}  # the results that are lists, and their widths; every other one is a scalar
_METER = {"rgb_psnr": "psnr", "rgb_ssim": "ssim", "rgb_rmse": "rmse", "rgb_depth_rmse": "rgb_depth"}  # result key -> meter, where they differ
_HOST_METRICS = ("loss", "psnr", "depth_rmse_m")  # per-frame Python floats, always summed on their own by np.sum


def _group_keys(group, table, rgb_depth):
    """Result keys, before the suffix, from one group's PointsMeter and table meters; groups: "" whole frames, "_static", "_dynamic"."""
    keys = ("depth", "intensity", "raydrop") + (("rgb_psnr", "rgb_ssim") if group else ("rgb_ssim", "rgb_rmse")) + (("rgb_depth_rmse",) if rgb_depth else ())
    return ("chamfer_distance", "f_score") + (keys if table else ())


def stats_layout(table=False, rgb_depth=False, splits=False):
    """The statistics vector of evaluate_frames as an ordered list of (result key, width, kind): kind "scalar" / "list" results are
    frame means (a float / a list of `width` floats), the one "count" is the number of frames.  pack_sums and unpack_means walk this
    list and nothing else knows an offset.  `rgb_depth` and `splits` only matter with `table`."""
    groups = [""] + ([f"_{s}" for s in M.SPLITS] if table and splits else [])
    lay = [(k + g, _LISTS.get(k, 1), "list" if k in _LISTS else "scalar") for g in groups for k in _group_keys(g, table, rgb_depth)]
    return [(k, 1, "scalar") for k in _HOST_METRICS] + [("frames", 1, "count")] + lay


def pack_sums(layout, values):
    """values[key]: this rank's per-frame values, [F] or [F, width] ("frames": ones) -> their float64 sums in layout order, the vector
    frame_shard.allreduce_sums adds over the ranks.  One [F, total width] matrix summed frame after frame; the host metrics by np.sum
    over their own list, pairwise on a long one -- the two roundings these sums have always had."""
    it = iter(np.concatenate([np.asarray(values[k], dtype=np.float64).reshape(-1, w) for k, w, _ in layout], axis=1).sum(0))
    sums = {k: [next(it) for _ in range(w)] for k, w, _ in layout}
    sums.update({k: [np.sum(values[k])] for k in _HOST_METRICS})
    return [float(v) for k, _, _ in layout for v in sums[k]]


def unpack_means(layout, sums):
    """The (all-reduced) vector of pack_sums -> the result dictionary: every sum divided once by max(frames, 1)."""
    it = iter(sums)
    cols = {k: [float(next(it)) for _ in range(w)] for k, w, _ in layout}
    n = max(cols["frames"][0], 1.0)
    return {k: int(cols[k][0]) if kind == "count" else [v / n for v in cols[k]] if kind == "list" else cols[k][0] / n for k, _, kind in layout}


def evaluate_frames(model, frames, num_steps, indices=None, ema=None, shard="rays", meters=None, intensity_inv_scale=1, refiner=None,
                    **eval_kwargs):
    """The metric half of the reference's evaluate_one_epoch (trainer.py:1458-1560) over a FrameSet opened with training=False:
    per frame eval_step, then the two quality metrics of the headline benchmark -- PSNR of the image (error_matrices.py:48-57), range
    RMSE in metres (:263-285) -- and chamfer distance / F-score of the range image's point cloud (PointsMeter, :299-356, on
    csrc/chamfer.hip); means over the frames.  `ema`: the step's ExponentialMovingAverage (RenderTrainStep.ema) -- the reference
    evaluates under `ema.store(); ema.copy_to()` and `restore()`s afterwards (trainer.py:1475-1477, 1843-1844), so metrics are
    those of the averaged weights once EMA is on (its default).
    Across ranks, `shard`:
      "rays"   every frame's rays are split over the ranks and the renders all-gathered (frame_shard.render_sharded): every rank
               computes the same statistics from the same full frames, no statistics collective is needed;
      "frames" the reference's scheme (trainer.py:1495-1524): rank r evaluates frames r, r + W, ... on its own and the per-rank SUMS
               of loss and metrics go through ONE all-reduce (frame_shard.allreduce_sums = the `dist.all_reduce(loss)` of
               trainer.py:1508, widened to the metrics); no per-pixel data crosses xGMI.
    Every rank returns the same numbers.  `meters="table"` adds the rest of the reference's evaluation table, computed on
    the device by nvsf/nerf/meters.py from the same eval_step tensors, fed as evaluate_one_epoch feeds its own (trainer.py:1537-1584):
    "depth" and "intensity" = [RMSE, MedAE, LPIPS, SSIM, PSNR] (DepthMeter_L4D(frames.scale), IntensityMeter_L4D(intensity_inv_scale,
    the reference's --intensity_inv_scale, default 1); the LPIPS slot is NaN: no weights here), "raydrop" = [RMSE, accuracy, F1]
    (RaydropMeter at `raydrop_thres`), "rgb_ssim" (SSIMMeter) and "rgb_rmse" (RMSE of the rendered against the measured image);
    frame means, the per-frame values riding in the same all-reduce under shard="frames".  Over a FrameSet opened with camera_depth=True
    the table also has "rgb_depth_rmse": RMSEMeter(rgb_metric=True) on pred_rgb_depth / scale against the LiDAR-projected depth map, as
    trainer.py:761-762, 1540-1541 feed it.  Over a FrameSet opened with `annotations` the table is also reported over the static
    background and over the annotated moving objects, as trainer.py:1545-1626 feeds metrics_static / metrics_dynamic and
    depth_metrics_static / depth_metrics_dynamic: per frame the masks of nvsf/nerf/object_masks.py (the prediction's range image gives
    the prediction's mask, the ground truth's its own; the camera image one mask from the projected boxes; a frame without boxes: ones /
    zeros), products by plain torch ops, the same meter kernels; keys "depth", "intensity", "raydrop", "chamfer_distance", "f_score",
    "rgb_psnr", "rgb_ssim" (and "rgb_depth_rmse") with the suffixes "_static" and "_dynamic", riding in the same all-reduce.  The range
    limit of the masks' z-buffer is the model's `lidar_max_depth`.  The default (None) returns exactly the six keys above from the same
    code path as before.  `refiner`: passed to eval_step -- every LiDAR figure, the split tables included, is then that of the refined
    ray-drop probability and of the intensity and range it gates; the keys do not change."""
    if shard not in ("rays", "frames"):
        raise ValueError("shard: 'rays' or 'frames'")
    if meters not in (None, "table"):
        raise ValueError("meters: None or 'table'")
    rank, ws = frame_shard.world()
    was_training = model.training
    model.eval()
    if ema is not None:
        ema.store()
        ema.copy_to()
    try:
        points = PointsMeter(frames.scale, frames.intrinsics_lidar, frames.intrinsics_hoz_lidar)
        ps, rm, ls = [], [], []
        table = split = None
        if meters == "table":
            table = M.table_meters(frames.scale, intensity_inv_scale, eval_kwargs.get("raydrop_thres", 0.5))
            if getattr(frames, "image_depths", None) is not None:  # FrameSet(camera_depth=True): the reference's camera depth RMSE
                table["rgb_depth"] = M.RMSEMeter(rgb_metric=True)
            if getattr(frames, "annotations", None) is not None:  # FrameSet(annotations=...): the static / dynamic tables
                split = {s: M.split_table_meters(frames.scale, intensity_inv_scale, eval_kwargs.get("raydrop_thres", 0.5), "rgb_depth" in table)
                         for s in M.SPLITS}
                split_points = {s: PointsMeter(frames.scale, frames.intrinsics_lidar, frames.intrinsics_hoz_lidar) for s in M.SPLITS}
        todo = list(range(len(frames)) if indices is None else indices)
        if shard == "frames" and ws > 1:
            todo = todo[rank::ws]
        for i in todo:
            data = frames.collate([int(i)])
            e = eval_step(model, data, num_steps, split_rays=(shard == "rays"), refiner=refiner, **eval_kwargs)
            ps.append(psnr(e["pred_rgb"], e["gt_rgb"]))
            rm.append(depth_rmse(e["pred_depth"], e["gt_depth"], frames.scale))
            points.update(e["pred_depth"], e["gt_depth"])
            if table is not None:
                M.update_table(table, e, frames.scale)  # launches only; read once, after the last frame
            if split is not None:
                masks = M.frame_object_masks(e, data, frames, model.lidar_max_depth)
                for s in M.SPLITS:
                    M.update_table(split[s], e, frames.scale, masks[s])
                    split_points[s].update(e["pred_depth"] * masks[s][0], e["gt_depth"] * masks[s][1])
            ls.append(float(e["loss"]))
    finally:
        if ema is not None:
            ema.restore()
        model.train(was_training)
    rgb_depth = table is not None and "rgb_depth" in table
    groups = {"": (table, points), **{f"_{s}": (split[s], split_points[s]) for s in (M.SPLITS if split is not None else ())}}
    vals = {"loss": ls, "psnr": ps, "depth_rmse_m": rm, "frames": np.ones(len(ps))}
    for g, (t, p) in groups.items():  # per-frame values under their result keys: one device -> host read per meter
        own = dict(zip(("chamfer_distance", "f_score"), np.array(p.V, dtype=np.float64).reshape(-1, 2).T))
        vals.update({k + g: own[k] if k in own else t[_METER.get(k, k)].frame_values() for k in _group_keys(g, table is not None, rgb_depth)})
    layout = stats_layout(table is not None, rgb_depth, split is not None)
    sums = pack_sums(layout, vals)
    if shard == "frames":
        sums = frame_shard.allreduce_sums(sums, device=next(model.parameters()).device)
    return unpack_means(layout, sums)
