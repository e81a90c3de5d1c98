"""The reference's evaluation meters (nvsf/lib/error_matrices.py:28-157, 159-297, 359-470; built by main_nvsf.py:224-240) on the
device: PSNRMeter, RMSEMeter, MAEMeter, DepthMeter_L4D, IntensityMeter_L4D, RaydropMeter, SSIMMeter.

`update(preds, truths)` takes fp32 DEVICE tensors and only enqueues work: the sums, extrema, median, SSIM mean and confusion counts
of the frame are computed by csrc/metrics.hip (include/nvsf_hip.h section 10) into one row of a device result tensor the meter owns.
Nothing is read back.  `measure()` does the one device -> host read of all rows and the scalar formulas (square root, log10, ratios,
means over the frames) in float64.  There is no CPU path: a CPU tensor, or one that is not float32, raises before any launch.

Definitions:
  * sums are fp64 sums of fp32 differences (the reference: numpy's fp32 pairwise mean);
  * DepthMeter_L4D / IntensityMeter_L4D: inputs divided by `scale`, clamped to [1e-6, 80] / [1e-6, 1]; SSIM is
    skimage.metrics.structural_similarity's default form -- uniform 7 x 7 window, sample covariance, data_range = max - min of the
    clamped truth -- and SSIMMeter is torchmetrics' default form -- Gaussian 11 x 11, sigma 1.5, population covariance,
    data_range = max(pred.max - pred.min, truth.max - truth.min) -- both evaluated in fp64 over the pixels whose window lies inside
    the image (the region both libraries crop to);
  * LPIPS: the AlexNet weights are not part of this package.  `lpips_fn=None` leaves the slot NaN; a callable is called as the reference
    calls its own (`lpips_fn(pred, truth, normalize=True)` on the clamped [H, W] images) and its result stored in the slot.
"""
import os

import numpy as np
import torch

_ROWS_PER_BLOCK = 64
_INF = float("inf")
WINDOW_UNIFORM, WINDOW_GAUSSIAN = 0, 1
MAX_WINDOW = 11

_workspaces = {}


def _streaming_rows(n):
    return min((int(n) + 1023) // 1024, 2048)


def stats_ws_bytes(n):
    return 64 * _streaming_rows(n)


def confusion_ws_bytes(n):
    return 48 * _streaming_rows(n)


MEDIAN_WS_BYTES = (16 + 2 * 2048) * 4


def ssim_ws_bytes(H, W, size):
    return 8 * ((int(W) - size + 1 + 31) // 32) * ((int(H) - size + 1 + 15) // 16)


def _workspace(device, nbytes):
    """Scratch of the launches of one (device, stream): they are ordered on that stream, so one buffer serves them all."""
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() * 8 < nbytes:
        ws = torch.empty(max((nbytes + 7) // 8, 4096), dtype=torch.float64, device=device)
        _workspaces[key] = ws
    return ws


def _check_pair(pred, truth, who):
    from nvsf import _hip
    for name, a in (("preds", pred), ("truths", truth)):
        if not isinstance(a, torch.Tensor):
            raise TypeError(f"{who}: {name} must be a torch tensor on a HIP device, got {type(a).__name__}")
        if not a.is_cuda:
            raise _hip.NvsfHipError(f"{who}: {name} is a CPU tensor; the meters run on the HIP device and have no CPU fallback")
        if a.dtype != torch.float32:
            raise ValueError(f"{who}: {name} must be float32, got {a.dtype}")
    if pred.shape != truth.shape or pred.device != truth.device:
        raise ValueError(f"{who}: preds {tuple(pred.shape)} on {pred.device} and truths {tuple(truth.shape)} on {truth.device} differ")
    if pred.numel() == 0:
        raise ValueError(f"{who}: empty frame")


def _check_out(out, n, like):
    if out is None:
        return torch.empty(n, dtype=torch.float64, device=like.device)
    if out.dtype != torch.float64 or out.numel() != n or not out.is_contiguous() or out.device != like.device:
        raise ValueError(f"out must be a contiguous float64 tensor of {n} elements on {like.device}")
    return out


def image_error_stats(pred, truth, lo=-_INF, hi=_INF, out=None, wide=False):
    """fp64 [6] device tensor: sum d^2, sum |d|, min / max of truth, min / max of pred, after clamping both to [lo, hi].  d = t - p is
    an fp32 difference; `wide`: an fp64 one."""
    from nvsf import _hip
    _check_pair(pred, truth, "image_error_stats")
    pred, truth = pred.contiguous(), truth.contiguous()
    out = _check_out(out, 6, pred)
    nbytes = stats_ws_bytes(pred.numel())
    _hip.call("nvsf_image_error_stats_wide" if wide else "nvsf_image_error_stats", _hip.ptr(pred), _hip.ptr(truth), pred.numel(), float(lo), float(hi),
              _hip.ptr(_workspace(pred.device, nbytes)), nbytes, _hip.ptr(out))
    return out


def median_abs_error(pred, truth, lo=-_INF, hi=_INF, out=None):
    """fp64 [1] device tensor: np.median of the float32 array |truth - pred| after the clamp, exactly."""
    from nvsf import _hip
    _check_pair(pred, truth, "median_abs_error")
    pred, truth = pred.contiguous(), truth.contiguous()
    out = _check_out(out, 1, pred)
    _hip.call("nvsf_median_abs_error", _hip.ptr(pred), _hip.ptr(truth), pred.numel(), float(lo), float(hi),
              _hip.ptr(_workspace(pred.device, MEDIAN_WS_BYTES)), MEDIAN_WS_BYTES, _hip.ptr(out))
    return out


def ssim_mean(pred, truth, data_range, window=WINDOW_UNIFORM, size=7, sigma=1.5, sample_cov=True, out=None):
    """fp64 [1] device tensor: mean SSIM of [H, W] or [H, W, C] images (C in {1, 3}) over the window positions inside the image.
    `data_range`: float64 DEVICE tensor of one element, read when the kernel runs."""
    from nvsf import _hip
    _check_pair(pred, truth, "ssim_mean")
    if pred.dim() not in (2, 3):
        raise ValueError("ssim_mean: images must be [H, W] or [H, W, C]")
    H, W = pred.shape[:2]
    C = pred.shape[2] if pred.dim() == 3 else 1
    size = int(size)
    if C not in (1, 3) or size % 2 == 0 or not 3 <= size <= MAX_WINDOW or H < size or W < size or window not in (0, 1):
        raise ValueError(f"ssim_mean: unsupported shape / window (H {H}, W {W}, C {C}, size {size}, window {window})")
    if not isinstance(data_range, torch.Tensor) or data_range.dtype != torch.float64 or data_range.numel() != 1 or data_range.device != pred.device:
        raise ValueError("ssim_mean: data_range must be a float64 tensor of one element on the images' device")
    pred, truth = pred.contiguous(), truth.contiguous()
    out = _check_out(out, 1, pred)
    nbytes = ssim_ws_bytes(H, W, size)
    _hip.call("nvsf_ssim_mean", _hip.ptr(pred), _hip.ptr(truth), H, W, C, int(window), size, float(sigma), 1 if sample_cov else 0,
              data_range.data_ptr(), _hip.ptr(_workspace(pred.device, nbytes)), nbytes, _hip.ptr(out))
    return out


def raydrop_confusion(pred, truth, ratio=0.5, out=None):
    """fp64 [6] device tensor whose first five words are int64 counts (`out[:5].view(torch.int64)`): TP, FP, TN, FN and
    #((pred > ratio) == truth); out[5] = sum d^2."""
    from nvsf import _hip
    _check_pair(pred, truth, "raydrop_confusion")
    pred, truth = pred.contiguous(), truth.contiguous()
    out = _check_out(out, 6, pred)
    nbytes = confusion_ws_bytes(pred.numel())
    _hip.call("nvsf_raydrop_confusion", _hip.ptr(pred), _hip.ptr(truth), pred.numel(), float(ratio),
              _hip.ptr(_workspace(pred.device, nbytes)), nbytes, _hip.ptr(out))
    return out


class _DeviceMeter:
    """Rows of per-frame statistics in device memory, in blocks of 64 frames; `rows()` is the one read."""
    COLS = 6

    def __init__(self):
        self.clear()

    def clear(self):
        self.N = 0
        self._blocks, self._counts = [], []

    def _next_row(self, device, count):
        if self.N % _ROWS_PER_BLOCK == 0:
            self._blocks.append(torch.full((_ROWS_PER_BLOCK, self.COLS), float("nan"), dtype=torch.float64, device=device))
        row = self._blocks[-1][self.N % _ROWS_PER_BLOCK]
        self._counts.append(float(count))
        self.N += 1
        return row

    def rows(self):
        """(rows [N, COLS] float64 numpy, element counts [N]): the meter's only device -> host read."""
        if self.N == 0:
            return np.zeros((0, self.COLS)), np.zeros(0)
        return torch.cat(self._blocks)[:self.N].cpu().numpy(), np.asarray(self._counts, dtype=np.float64)

    def frame_values(self):
        raise NotImplementedError

    def _mean_like_reference_scalar(self):
        v = self.frame_values()
        return float(v.sum() / (self.N + 1e-8))  # V / (N + 1e-8), error_matrices.py:59-60

    def _mean_like_reference_rows(self):
        v = self.frame_values()
        assert self.N == len(v)
        with np.errstate(invalid="ignore"), _quiet_empty_mean():
            return v.mean(0)


class _quiet_empty_mean:
    def __enter__(self):
        import warnings
        self._w = warnings.catch_warnings()
        self._w.__enter__()
        warnings.simplefilter("ignore", category=RuntimeWarning)

    def __exit__(self, *exc):
        return self._w.__exit__(*exc)


class PSNRMeter(_DeviceMeter):
    """Peak signal to noise ratio of images in [0, 1]: -10 log10(mean d^2 + 1e-8) per frame (error_matrices.py:28-66)."""

    def update(self, preds, truths):
        _check_pair(preds, truths, "PSNRMeter")
        image_error_stats(preds, truths, out=self._next_row(preds.device, preds.numel()))

    def frame_values(self):
        r, n = self.rows()
        return -10 * np.log10(r[:, 0] / n + 1e-8)

    def measure(self):
        return self._mean_like_reference_scalar()

    def write(self, writer, global_step, prefix=""):
        writer.add_scalar(os.path.join(prefix, "PSNR"), self.measure(), global_step)

    def report(self):
        return f"PSNR = {self.measure():.3f}"


class RMSEMeter(_DeviceMeter):
    """Root mean square error per frame (error_matrices.py:68-115).  rgb_metric=True is the camera-depth form: predictions are zeroed
    where the truth is 0 and both are capped at 80; the differences are fp64 ones there, as numpy's are once `preds * zero_mask`
    (error_matrices.py:93-94) has widened the predictions."""

    def __init__(self, rgb_metric=False):
        self.rgb_metric = rgb_metric
        super().__init__()

    def update(self, preds, truths):
        _check_pair(preds, truths, "RMSEMeter")
        hi = _INF
        if self.rgb_metric:
            preds, hi = preds * (truths != 0).to(preds.dtype), 80.0
        image_error_stats(preds, truths, hi=hi, out=self._next_row(preds.device, preds.numel()), wide=self.rgb_metric)

    def frame_values(self):
        r, n = self.rows()
        return np.sqrt(r[:, 0] / n)

    def measure(self):
        return self._mean_like_reference_scalar()

    def write(self, writer, global_step, prefix=""):
        writer.add_scalar(os.path.join(prefix, "RMSE"), self.measure(), global_step)

    def report(self):
        if self.rgb_metric:
            return f"RMSE = {self.measure():.3f}"
        return f"RMSE_intensity = {self.measure():.3f}"


class MAEMeter(_DeviceMeter):
    """Mean absolute error of truths * s - preds * s per frame (error_matrices.py:117-157)."""

    def __init__(self, intensity_inv_scale=1.0):
        self.intensity_inv_scale = intensity_inv_scale
        super().__init__()

    def update(self, preds, truths):
        _check_pair(preds, truths, "MAEMeter")
        s = self.intensity_inv_scale
        image_error_stats(preds * s, truths * s, out=self._next_row(preds.device, preds.numel()))

    def frame_values(self):
        r, n = self.rows()
        return r[:, 1] / n

    def measure(self):
        return self._mean_like_reference_scalar()

    def write(self, writer, global_step, prefix=""):
        writer.add_scalar(os.path.join(prefix, "MAE"), self.measure(), global_step)

    def report(self):
        return f"MAE_intensity = {self.measure():.3f}"


class _L4DMeter(_DeviceMeter):
    """RMSE, MedAE, LPIPS, SSIM, PSNR of one [1, H, W] (or [H, W]) LiDAR channel per frame (error_matrices.py:159-297).
    Row: 0-5 the error statistics, 6 data range, 7 median, 8 SSIM, 9 LPIPS."""
    COLS = 10
    LO, HI = 1e-6, 1.0
    TAG, NAME = "", ""

    def __init__(self, scale, lpips_fn=None):
        self.scale, self.lpips_fn = scale, lpips_fn
        super().__init__()

    def update(self, preds, truths):
        _check_pair(preds, truths, type(self).__name__)
        if preds.dim() == 3 and preds.shape[0] == 1:
            preds, truths = preds[0], truths[0]
        if preds.dim() != 2:
            raise ValueError(f"{type(self).__name__}: expected [1, H, W] or [H, W] images, got {tuple(preds.shape)}")
        lo, hi = self.LO, self.HI
        p, t = (preds / self.scale).clamp(lo, hi), (truths / self.scale).clamp(lo, hi)
        row = self._next_row(p.device, p.numel())
        image_error_stats(p, t, lo, hi, out=row[0:6])
        torch.sub(row[3], row[2], out=row[6])  # data_range = max(gt) - min(gt), on the device
        median_abs_error(p, t, lo, hi, out=row[7:8])
        ssim_mean(p, t, row[6:7], WINDOW_UNIFORM, 7, sample_cov=True, out=row[8:9])
        if self.lpips_fn is not None:
            row[9:10].copy_(torch.as_tensor(self.lpips_fn(p, t, normalize=True), dtype=torch.float64).reshape(1))

    def frame_values(self):
        r, n = self.rows()
        mse = r[:, 0] / n
        with np.errstate(divide="ignore", invalid="ignore"):
            psnr = 10 * np.log10(float(self.HI) ** 2 / mse)
        return np.stack([np.sqrt(mse), r[:, 7], r[:, 9], r[:, 8], psnr], axis=1)

    def measure(self):
        return self._mean_like_reference_rows()

    def write(self, writer, global_step, prefix="", suffix=""):
        writer.add_scalar(os.path.join(prefix, f"{self.TAG}{suffix}"), self.measure()[0], global_step)

    def report(self):
        return f"{self.NAME} (RMSE, MedAE, LPIPS, SSIM, PNSR) = {self.measure()}"


class DepthMeter_L4D(_L4DMeter):
    """Range errors in metres: inputs in scene units, `scale` the scene scale; clamp [1e-6, 80] m."""
    LO, HI = 1e-6, 80
    TAG, NAME = "depth error", "Depth_error"


class IntensityMeter_L4D(_L4DMeter):
    """Intensity errors: inputs divided by `scale` (the reference passes its --intensity_inv_scale here); clamp [1e-6, 1]."""
    LO, HI = 1e-6, 1.0
    TAG, NAME = "intensity error", "Intensity_error"


class RaydropMeter(_DeviceMeter):
    """RMSE, accuracy and F1 of the predicted ray-drop probability against the measured mask (error_matrices.py:359-413)."""
    COLS = 6

    def __init__(self, ratio=0.5):
        self.ratio = ratio
        super().__init__()

    def update(self, preds, truths):
        _check_pair(preds, truths, "RaydropMeter")
        raydrop_confusion(preds, truths, self.ratio, out=self._next_row(preds.device, preds.numel()))

    def frame_values(self):
        r, n = self.rows()
        counts = np.ascontiguousarray(r[:, :5]).view(np.int64).astype(np.float64)
        tp, fp, fn = counts[:, 0], counts[:, 1], counts[:, 3]
        with np.errstate(divide="ignore", invalid="ignore"):  # 0 / 0 -> NaN, as the reference's numpy scalars give
            precision, recall = tp / (tp + fp), tp / (tp + fn)
            f1 = 2 * (precision * recall) / (precision + recall)
        return np.stack([np.sqrt(r[:, 5] / n), counts[:, 4] / n, f1], axis=1)

    def measure(self):
        return self._mean_like_reference_rows()

    def write(self, writer, global_step, prefix="", suffix=""):
        writer.add_scalar(os.path.join(prefix, "raydrop error"), self.measure()[0], global_step)

    def report(self):
        return f"Rdrop_error (RMSE, Accuracy, F_score) = {self.measure()}"


class SSIMMeter(_DeviceMeter):
    """Structural similarity of [1, H, W, C] (or [H, W, C]) images, torchmetrics' defaults (error_matrices.py:415-470); a NaN frame
    counts as 0.  Row: 0-5 the error statistics, 6 data range, 7 SSIM."""
    COLS = 8

    def __init__(self, device=None):
        self.device = device
        super().__init__()

    def update(self, preds, truths):
        _check_pair(preds, truths, "SSIMMeter")
        if preds.dim() == 4 and preds.shape[0] == 1:
            preds, truths = preds[0], truths[0]
        if preds.dim() != 3:
            raise ValueError(f"SSIMMeter: expected [1, H, W, C] or [H, W, C] images, got {tuple(preds.shape)}")
        row = self._next_row(preds.device, preds.numel())
        image_error_stats(preds, truths, out=row[0:6])
        torch.maximum(row[5] - row[4], row[3] - row[2], out=row[6])
        ssim_mean(preds, truths, row[6:7], WINDOW_GAUSSIAN, 11, sigma=1.5, sample_cov=False, out=row[7:8])

    def frame_values(self):
        r, _ = self.rows()
        return np.where(np.isnan(r[:, 7]), 0.0, r[:, 7])

    def measure(self):
        return self._mean_like_reference_scalar()

    def write(self, writer, global_step, prefix=""):
        writer.add_scalar(os.path.join(prefix, "SSIM"), self.measure(), global_step)

    def report(self):
        return f"SSIM = {self.measure():.3f}"


def table_meters(scale, intensity_inv_scale=1, raydrop_ratio=0.5, lpips_fn=None):
    """The meters of the reference's evaluation table (main_nvsf.py:224-240) minus PointsMeter (evaluate.PointsMeter) and
    LPIPSMeter (no weights here): {"depth", "intensity", "raydrop", "psnr", "rmse", "ssim"}.  "rmse" compares the rendered image
    with the measured one.  The reference feeds its camera RMSE meter the LiDAR-projected camera DEPTH image (trainer.py:1540-1541):
    that is the further meter "rgb_depth" = RMSEMeter(rgb_metric=True), which evaluate_frames adds when the frames carry the map
    (FrameSet(camera_depth=True))."""
    return {"depth": DepthMeter_L4D(scale, lpips_fn), "intensity": IntensityMeter_L4D(intensity_inv_scale, lpips_fn),
            "raydrop": RaydropMeter(raydrop_ratio), "psnr": PSNRMeter(), "rmse": RMSEMeter(), "ssim": SSIMMeter()}


def update_table(meters, e, scale=1.0, masks=None):
    """Feeds the meters of `table_meters` from eval_step's output, as evaluate_one_epoch feeds its own (trainer.py:1537-1584).  A
    "rgb_depth" meter is fed pred_rgb_depth / scale against the depth map in metres (trainer.py:761-762).  `masks` = (mask_pred, mask_gt,
    mask_img) feeds one of the two further tables (`split_table_meters`) as trainer.py:1553-1569, 1604-1626 do: the prediction times its own
    mask, the ground truth times the ground truth's; the camera image and its depth times the one image mask.  None multiplies nothing."""
    mp, mg, mi, mc = (None,) * 4 if masks is None else (*masks, masks[2][..., None])
    on = lambda x, m: x if m is None else x * m
    if "rgb_depth" in meters:
        meters["rgb_depth"].update(on(e["pred_rgb_depth"] / scale, mi), on(e["gt_rgb_depth"], mi))
    for k in ("depth", "intensity", "raydrop"):
        meters[k].update(on(e["pred_" + k], mp), on(e["gt_" + k], mg))
    for k in ("psnr", "rmse", "ssim"):
        if k in meters:
            meters[k].update(on(e["pred_rgb"], mc), on(e["gt_rgb"], mc))


SPLITS = ("static", "dynamic")


def split_table_meters(scale, intensity_inv_scale=1, raydrop_ratio=0.5, camera_depth=False):
    """The meters of ONE of the reference's two further tables (metrics_static / depth_metrics_static, or the _dynamic pair,
    main_nvsf.py:224-240) minus PointsMeter and LPIPSMeter: {"depth", "intensity", "raydrop", "psnr", "ssim"} and, when the frames carry
    the camera depth map, "rgb_depth"."""
    m = {"depth": DepthMeter_L4D(scale), "intensity": IntensityMeter_L4D(intensity_inv_scale), "raydrop": RaydropMeter(raydrop_ratio),
         "psnr": PSNRMeter(), "ssim": SSIMMeter()}
    if camera_depth:
        m["rgb_depth"] = RMSEMeter(rgb_metric=True)
    return m


def frame_object_masks(e, data, frames, lidar_max_depth):
    """The masks of one evaluated frame as trainer.py:1545-1551, 1586-1602 build them: {"static": (range-image mask of the prediction,
    of the ground truth, camera-image mask), "dynamic": likewise}, each [1, H, W] fp32 on the device.  A frame without boxes gets
    ones / zeros."""
    from nvsf.nerf import object_masks as OM
    pd, gd = e["pred_depth"], e["gt_depth"]
    if len(data["3d_annotation"]) > 0:
        args = (data, frames.scale, frames.offset, frames.intrinsics_lidar, frames.intrinsics_hoz_lidar, lidar_max_depth)
        sp, dp = OM.compute_object_masks(pd[0].float().contiguous(), *args)
        sg, dg = OM.compute_object_masks(gd[0].float().contiguous(), *args)
        si, di = OM.compute_object_masks_img(data, frames.scale, frames.offset, device=pd.device)
    else:
        sp = sg = torch.ones_like(pd[0])
        dp = dg = torch.zeros_like(pd[0])
        si = torch.ones(e["pred_rgb"].shape[1:3], dtype=pd.dtype, device=pd.device)
        di = torch.zeros_like(si)
    cast = lambda *ms: tuple(m[None].to(pd.dtype) for m in ms)
    return {"static": cast(sp, sg, si), "dynamic": cast(dp, dg, di)}


def report_lines(meters):
    """The reference's report lines, LiDAR meters first (trainer.py:1794-1827)."""
    return [meters[k].report() for k in ("depth", "intensity", "raydrop", "psnr", "rmse", "ssim", "rgb_depth") if k in meters]


def table_report(res):
    """The reference's report lines (trainer.py:1794-1827) from the dictionary evaluate_frames(meters="table") returns."""
    return [f"Points_error(CD, F-score) = {[round(float(res['chamfer_distance']), 3), round(float(res['f_score']), 3)]}",
            f"Depth_error (RMSE, MedAE, LPIPS, SSIM, PNSR) = {np.array(res['depth'])}",
            f"Intensity_error (RMSE, MedAE, LPIPS, SSIM, PNSR) = {np.array(res['intensity'])}",
            f"Rdrop_error (RMSE, Accuracy, F_score) = {np.array(res['raydrop'])}",
            f"RMSE_intensity = {res['rgb_rmse']:.3f}", f"PSNR = {res['psnr']:.3f}", f"SSIM = {res['rgb_ssim']:.3f}"] + \
        ([f"RMSE = {res['rgb_depth_rmse']:.3f}"] if "rgb_depth_rmse" in res else []) + \
        [line for s in SPLITS if f"depth_{s}" in res for line in _split_report(res, s)]


def _split_report(res, s):
    """The lines of the static / dynamic table (trainer.py:1800-1840 print the same meters under "Background" / "Foreground")."""
    g = lambda k: res[f"{k}_{s}"]
    return [f"[{s}] Points_error(CD, F-score) = {[round(float(g('chamfer_distance')), 3), round(float(g('f_score')), 3)]}",
            f"[{s}] Depth_error (RMSE, MedAE, LPIPS, SSIM, PNSR) = {np.array(g('depth'))}",
            f"[{s}] Intensity_error (RMSE, MedAE, LPIPS, SSIM, PNSR) = {np.array(g('intensity'))}",
            f"[{s}] Rdrop_error (RMSE, Accuracy, F_score) = {np.array(g('raydrop'))}",
            f"[{s}] PSNR = {g('rgb_psnr'):.3f}", f"[{s}] SSIM = {g('rgb_ssim'):.3f}"] + \
        ([f"[{s}] RMSE = {g('rgb_depth_rmse'):.3f}"] if f"rgb_depth_rmse_{s}" in res else [])
