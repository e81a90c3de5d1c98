"""Timing of the device meters (nvsf/nerf/meters.py, csrc/metrics.hip).

    python tools/bench_meters.py [--reps 20] [--out profiles/meters_bench.json]

Two frames: a 66 x 1030 x 1 range image (nvsf.synthetic.street_range_image, seed 0, and a noisy prediction of it; clamp [1e-6, 80],
SSIM uniform 7) and a smooth 376 x 1408 x 3 image pair in [0, 1] (no clamp, SSIM Gaussian 11).  Every leg is the median and min .. max
of --reps runs after warm-up, in milliseconds between device events on the current stream (so a leg that waits for the host, like the
host path, is charged that wait).  A kernel and its yardstick are interleaved rep by rep, so that a busy neighbour hits both.
Legs per frame:
  stats / median / ssim / confusion   one entry point alone, through its Python wrapper, against a torch-on-device restatement of the
                                      same statistic (elementwise ops and reductions; kthvalue; conv2d moments in fp64, or fp32 where
                                      the device has no fp64 convolution -- `ssim_torch_dtype` says which);
  table                               all meters of the evaluation table for one frame (launches only, no read), against the host path
                                      evaluate_frames has used so far: evaluate.psnr + evaluate.depth_rmse on the same tensors.
`fraction_of_hbm_peak`: the compulsory traffic of the stats and SSIM kernels is one read of both images, 8 bytes per value; the figure
is (8 n / 8 TB/s) / median.  `decided`: whether the medians differ by more than the two spreads (max - min) combined.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "selfsupervised-nvsf_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from nvsf import _hip, synthetic as S  # noqa: E402
from nvsf.nerf import meters as M  # noqa: E402
from nvsf.nerf.evaluate import depth_rmse, psnr  # noqa: E402

HBM_PEAK = 8e12
INF = float("inf")


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def versus(kernel, yard, reps):
    for _ in range(3):
        kernel(), yard()
    torch.cuda.synchronize()
    tk, ty = [], []
    for _ in range(reps):
        tk.append(event_ms(kernel))
        ty.append(event_ms(yard))
    k, y = stats(tk), stats(ty)
    spreads = (k["max"] - k["min"]) + (y["max"] - y["min"])
    return {"kernel_ms": k, "yardstick_ms": y, "yardstick_over_kernel": y["median"] / k["median"],
            "decided": bool(abs(y["median"] - k["median"]) > spreads)}


def torch_stats(p, t, lo, hi):
    p, t = p.clamp(lo, hi), t.clamp(lo, hi)
    d = (t - p).double()
    return torch.stack([(d * d).sum(), d.abs().sum(), t.min().double(), t.max().double(), p.min().double(), p.max().double()])


def torch_median(p, t, lo, hi):
    e = (t.clamp(lo, hi) - p.clamp(lo, hi)).abs().reshape(-1)
    n = e.numel()
    return (e.kthvalue((n - 1) // 2 + 1).values + e.kthvalue(n // 2 + 1).values) / 2


def torch_confusion(p, t, ratio):
    m = p > ratio
    d = (t - p).double()
    return torch.stack([((t == 1) & m).sum(), ((t == 0) & m).sum(), ((t == 0) & ~m).sum(), ((t == 1) & ~m).sum(), (m.float() == t).sum()]), (d * d).sum()


def torch_ssim(p, t, R, window, size, sigma, sample_cov, dtype):
    p, t = (a.reshape(a.shape[0], a.shape[1], -1).permute(2, 0, 1)[None].to(dtype) for a in (p, t))
    C = p.shape[1]
    d = torch.arange(size, dtype=dtype, device=p.device) - (size - 1) / 2
    w = torch.exp(-0.5 * (d / sigma) ** 2) if window == M.WINDOW_GAUSSIAN else torch.ones_like(d)
    w = w / w.sum()
    kernel = (w[:, None] * w[None, :]).expand(C, 1, size, size).contiguous()
    mp, mt, mpp, mtt, mpt = F.conv2d(torch.cat([p, t, p * p, t * t, p * t]), kernel, groups=C)
    k = size * size / (size * size - 1.0) if sample_cov else 1.0
    c1, c2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    s = ((2 * mp * mt + c1) * (2 * k * (mpt - mp * mt) + c2)) / ((mp * mp + mt * mt + c1) * (k * (mpp - mp * mp) + k * (mtt - mt * mt) + c2))
    return s.mean()


def frames(dev):
    rng = np.random.default_rng(0)
    truth = S.street_range_image(rng)[0]
    pred = np.where(truth > 0, truth + rng.normal(0.0, 0.15, truth.shape), 0.0).astype(np.float32)
    pred[rng.random(truth.shape) < 0.1] = 0.0
    H, W = S.CAM_HW
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    img = np.stack([0.5 + 0.4 * np.sin(0.01 * (c + 1) * x + 0.02 * y + c) for c in range(3)], -1).astype(np.float32)
    noisy = np.clip(img + rng.normal(0, 0.02, img.shape), 0, 1).astype(np.float32)
    to = lambda a: torch.from_numpy(a).to(dev)
    return {"lidar_66x1030x1": (to(pred), to(truth), 1e-6, 80.0, M.WINDOW_UNIFORM, 7, True),
            "camera_376x1408x3": (to(noisy), to(img), -INF, INF, M.WINDOW_GAUSSIAN, 11, False)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"unit": "ms (device events)", "reps": args.reps}
    try:
        torch_ssim(torch.rand(16, 16, device=dev), torch.rand(16, 16, device=dev), 1.0, 0, 7, 1.5, True, torch.float64)
        torch.cuda.synchronize()
        ssim_dtype = torch.float64
    except RuntimeError:
        ssim_dtype = torch.float32
    res["ssim_torch_dtype"] = str(ssim_dtype)
    for name, (p, t, lo, hi, window, size, cov) in frames(dev).items():
        n = p.numel()
        out6, out1 = torch.empty(6, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.float64, device=dev)
        R = torch.tensor([float(t.max() - t.min())], dtype=torch.float64, device=dev)
        Rf = float(R)
        leg = {"values": n}
        leg["stats"] = versus(lambda: M.image_error_stats(p, t, lo, hi, out=out6), lambda: torch_stats(p, t, lo, hi), args.reps)
        leg["median"] = versus(lambda: M.median_abs_error(p, t, lo, hi, out=out1), lambda: torch_median(p, t, lo, hi), args.reps)
        leg["ssim"] = versus(lambda: M.ssim_mean(p, t, R, window, size, 1.5, cov, out=out1),
                             lambda: torch_ssim(p, t, Rf, window, size, 1.5, cov, ssim_dtype), args.reps)
        mask_p, mask_t = (p > 0).float() * 0.7 + 0.1, (t > (0 if lo > 0 else 0.5)).float()
        leg["confusion"] = versus(lambda: M.raydrop_confusion(mask_p, mask_t, 0.5, out=out6), lambda: torch_confusion(mask_p, mask_t, 0.5), args.reps)
        for k in ("stats", "ssim"):
            leg[k]["fraction_of_hbm_peak"] = (8.0 * n / HBM_PEAK) / (leg[k]["kernel_ms"]["median"] * 1e-3)
        got, want = float(M.ssim_mean(p, t, R, window, size, 1.5, cov)), float(torch_ssim(p, t, Rf, window, size, 1.5, cov, ssim_dtype))
        leg["ssim"]["kernel_minus_torch"] = got - want
        leg["median"]["kernel_minus_torch"] = float(M.median_abs_error(p, t, lo, hi)) - float(torch_median(p, t, lo, hi))
        res[name] = leg
    # the whole table of one frame against the host path of the two metrics evaluate_frames had
    (lp, lt, *_), (cp, ct, *_) = frames(dev).values()
    scale = S.SCALE
    e = {"pred_depth": (lp * scale)[None], "gt_depth": (lt * scale)[None], "pred_intensity": (lp / 80)[None], "gt_intensity": (lt / 80)[None],
         "pred_raydrop": ((lp > 0).float() * 0.7 + 0.1)[None], "gt_raydrop": (lt > 0).float()[None], "pred_rgb": cp[None], "gt_rgb": ct[None]}
    table = M.table_meters(scale)

    def device_table():
        for m in table.values():
            m.clear()
        M.update_table(table, e)

    def host_path():
        psnr(e["pred_rgb"], e["gt_rgb"])
        depth_rmse(e["pred_depth"], e["gt_depth"], scale)
    res["table_per_frame"] = versus(device_table, host_path, args.reps)
    res["table_per_frame"]["kernel"] = "all meters of the table, launches only (3 range-image meters + 3 camera meters)"
    res["table_per_frame"]["yardstick"] = "evaluate.psnr + evaluate.depth_rmse: two whole-frame copies to the host each, float64 numpy"
    res["table_report"] = M.report_lines(table)
    res["device"] = torch.cuda.get_device_name(0)
    res["build_digest"] = _hip.build_digest()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
