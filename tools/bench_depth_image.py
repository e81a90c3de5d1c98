"""Timing of the LiDAR-projected camera depth maps and of the camera depth loss (csrc/projection.hip, csrc/losses.hip).

    python tools/bench_depth_image.py [--reps 20] [--out profiles/depth_image_bench.json]

Every leg is the median and min .. max of --reps runs after warm-up, in milliseconds between device events on the current stream (a leg
that waits for the host, like the numpy loop, is charged that wait).  An entry and its yardstick are interleaved rep by rep, so that a
busy neighbour hits both.  `decided`: whether the medians differ by more than the two spreads (max - min) combined.
Legs:
  depth_images_1 / _60   nvsf_lidar_depth_images for 1 frame and for 60 frames of 66 x 1030 (nvsf.synthetic.street_range_image) into
                         376 x 1408, through a KITTI-360-like rig, against
                           torch     a torch-on-device restatement (fp32 directions, fp64 projection, scatter_reduce(amin) over the same
                                     points);
                           numpy     the host path restated: vectorised projection, then a Python loop with one iteration per point in
                                     view, as dataset_utils.get_lidar_depth_image has (range images already on the host; the result stays there;
                                     at 60 frames a run takes seconds, so it joins the first 5 reps only);
                         `kernel_ms` is the Python wrapper (it copies the poses to the host and forms lidar2cam there),
                         `entry_point_alone_ms` the C entry point with lidar2cam already on the device (a memset and one launch);
                         `fraction_of_hbm_peak`: compulsory traffic = the range images in + the maps out (0.27 + 2.1 MB per frame)
                         over the entry point's time, against 8 TB/s;
  camera_loss            CameraLossFn (both camera terms, one launch each way) forward + backward on 4096 rays against MseSumFn for the
                         RGB term + torch ops under autograd for the depth term (L1);
  train_step             the config-4 training step (4096 + 4096 rays x 768 samples, static field) with the depth term on against the
                         same step with it off, two step objects on two copies of the model, interleaved.
"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "selfsupervised-nvsf_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from nvsf import _hip, synthetic as S  # noqa: E402
from nvsf.nerf.dataset import depth_image as D  # noqa: E402
from nvsf.nerf.losses import CameraLossFn, MseSumFn, rgb_depth_loss_host  # noqa: E402
from nvsf.nerf.train_step import RenderTrainStep  # noqa: E402

HBM_PEAK = 8e12


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def versus(kernel, yards, reps, warm=3, fewer=None):
    """kernel and every yardstick of `yards` ({name: fn}), interleaved rep by rep.  `fewer` ({name: n}): a yardstick that takes seconds
    per run joins only the first n reps (and one warm-up run); its row says how many."""
    fewer = fewer or {}
    for w in range(warm):
        kernel()
        for name, y in yards.items():
            if w == 0 or name not in fewer:
                y()
    torch.cuda.synchronize()
    tk, ty = [], {k: [] for k in yards}
    for rep in range(reps):
        tk.append(event_ms(kernel))
        for name, y in yards.items():
            if rep < fewer.get(name, reps):
                ty[name].append(event_ms(y))
    k = stats(tk)
    out = {"kernel_ms": k}
    for name, v in ty.items():
        y = stats(v)
        spreads = (k["max"] - k["min"]) + (y["max"] - y["min"])
        out[name] = {"yardstick_ms": y, "reps": len(v), "yardstick_over_kernel": y["median"] / k["median"],
                     "decided": bool(abs(y["median"] - k["median"]) > spreads)}
    return out


def rig(n):
    """(poses, poses_lidar) fp32 [n, 4, 4]: the camera looks along the LiDAR's +x, lever arm 2 to 80 cm, 0.02 rad yaw."""
    yaw = 0.02
    perm = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])
    rz = np.array([[np.cos(yaw), -np.sin(yaw), 0.0], [np.sin(yaw), np.cos(yaw), 0.0], [0.0, 0.0, 1.0]])
    l2c = np.eye(4)
    l2c[:3, :3], l2c[:3, 3] = perm @ rz, [0.02, -0.25, -0.8]
    poses, poses_lidar = [], []
    for f in range(n):
        pl = np.eye(4)
        pl[:3, 3] = [0.8 * f, 0.0, 0.0]
        poses_lidar.append(pl)
        poses.append(pl @ np.linalg.inv(l2c))
    return np.stack(poses).astype(np.float32), np.stack(poses_lidar).astype(np.float32)


def lidar2cam(poses, poses_lidar):
    return np.stack([np.linalg.inv(p) @ l for p, l in zip(poses, poses_lidar)]).astype(np.float32)


def torch_depth_images(r, l2c, K, H, W, fov_up, fov, fov_hoz):
    F, Hl, Wl = r.shape
    i = torch.arange(Wl, dtype=torch.float32, device=r.device)[None, :]
    j = torch.arange(Hl, dtype=torch.float32, device=r.device)[:, None]
    beta = -(i - Wl / 2) / Wl * fov_hoz / 180 * np.pi
    alpha = (fov_up - j / Hl * fov) / 180 * np.pi
    dirs = torch.stack([torch.cos(alpha) * torch.cos(beta), torch.cos(alpha) * torch.sin(beta), torch.sin(alpha).expand(Hl, Wl)], -1)
    pts = (dirs[None] * r[..., None]).double().reshape(F, -1, 3)
    cam = pts @ l2c[:, :3, :3].double().transpose(1, 2) + l2c[:, None, :3, 3].double()
    q = cam @ K.T
    z = q[..., 2].clamp(1e-5, 99999)
    u, v = q[..., 0] / z, q[..., 1] / z
    ok = (u >= 0) & (u < W) & (v >= 0) & (v < H) & (r.reshape(F, -1) != 0)
    frame = torch.arange(F, device=r.device)[:, None].expand_as(u)
    pix = (frame * (H * W) + v.clamp(0, H - 1).long() * W + u.clamp(0, W - 1).long())[ok]
    out = torch.full((F * H * W,), float("inf"), dtype=torch.float32, device=r.device)
    out.scatter_reduce_(0, pix, z[ok].float(), "amin")
    return torch.where(torch.isinf(out), torch.zeros_like(out), out).view(F, H, W)


def numpy_depth_images(r, l2c, K, H, W, fov_up, fov, fov_hoz):
    """The host path in numpy: fp32 directions times range, fp64 projection, then the z-buffer as a Python loop with one iteration per
    point in view, which is what dataset_utils.py:92-95 does (here over flat pixel indices)."""
    F, Hl, Wl = r.shape
    az = -(np.arange(Wl, dtype=np.float32) - Wl / 2) / Wl * fov_hoz / 180 * np.pi
    el = (fov_up - np.arange(Hl, dtype=np.float32) / Hl * fov) / 180 * np.pi
    dirs = np.stack([np.cos(el)[:, None] * np.cos(az)[None, :], np.cos(el)[:, None] * np.sin(az)[None, :], np.broadcast_to(np.sin(el)[:, None], (Hl, Wl))], -1)
    out = np.zeros((F, H * W))
    for f in range(F):
        cloud = (dirs * r[f][..., None])[r[f] != 0.0].astype(np.float64)
        q = (cloud @ l2c[f, :3, :3].T.astype(np.float64) + l2c[f, :3, 3]) @ K.T
        z = np.clip(q[:, 2], 1e-5, 99999)
        u, v = q[:, 0] / z, q[:, 1] / z
        seen = (u >= 0) & (u < W) & (v >= 0) & (v < H)
        img = out[f]
        for pix, depth in zip(v[seen].astype(np.int64) * W + u[seen].astype(np.int64), z[seen]):
            if img[pix] == 0 or depth < img[pix]:
                img[pix] = depth
    return out.reshape(F, H, W)


def depth_image_legs(dev, reps):
    H, W = S.CAM_HW
    fov_up, fov, fov_hoz = S.LIDAR_FOV
    K = np.array([[S.CAM_K[0], 0.0, S.CAM_K[2]], [0.0, S.CAM_K[1], S.CAM_K[3]], [0.0, 0.0, 1.0]])
    ranges = np.stack([S.street_range_image(np.random.default_rng(f))[0] for f in range(60)]).astype(np.float32)
    poses, poses_lidar = rig(60)
    res = {}
    for n in (1, 60):
        r_host, l2c_host = ranges[:n], lidar2cam(poses[:n], poses_lidar[:n])
        r, p, pl = (torch.from_numpy(a[:n]).to(dev) for a in (ranges, poses, poses_lidar))
        l2c, Kd = torch.from_numpy(l2c_host).to(dev), torch.from_numpy(K).to(dev)
        entry = lambda: D.lidar_depth_images(r, p, pl, K, H, W, (fov_up, fov), (180.0, fov_hoz))
        leg = versus(entry, {"torch": lambda: torch_depth_images(r, l2c, Kd, H, W, fov_up, fov, fov_hoz),
                             "numpy": lambda: numpy_depth_images(r_host, l2c_host, K, H, W, fov_up, fov, fov_hoz)}, reps,
                     fewer={"numpy": 5} if n > 1 else None)
        # the entry point alone (memset + one launch), lidar2cam already on the device: the wrapper above also copies the poses to the
        # host and inverts them there
        out, l2c16, Kh = torch.empty(n, H, W, device=dev), l2c.reshape(n, 16).contiguous(), _hip.host_f64(K.reshape(-1))
        raw = lambda: _hip.call("nvsf_lidar_depth_images", _hip.ptr(r), n, r.shape[1], r.shape[2], fov_up, fov, fov_hoz, _hip.ptr(l2c16), Kh, H, W,
                                _hip.ptr(out))
        raw()
        torch.cuda.synchronize()
        leg["entry_point_alone_ms"] = stats([event_ms(raw) for _ in range(reps)])
        got, want = entry().cpu().numpy(), torch_depth_images(r, l2c, Kd, H, W, fov_up, fov, fov_hoz).cpu().numpy()
        nbytes = 4.0 * (r.numel() + n * H * W)
        leg.update(frames=n, points=int((r != 0).sum()), non_empty_pixels=int((got != 0).sum()), bytes=nbytes,
                   fraction_of_hbm_peak=(nbytes / HBM_PEAK) / (leg["entry_point_alone_ms"]["median"] * 1e-3),
                   pixels_not_bit_equal_to_torch=int((got.view(np.uint32) != want.view(np.uint32)).sum()))
        res[f"depth_images_{n}"] = leg
    return res


def camera_loss_leg(dev, reps, n=4096):
    scale = S.SCALE
    g = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.rand(*s, generator=g)
    gt_m = rnd(1, n) * 95 + 0.5
    gt_m[rnd(1, n) < 0.85] = 0.0
    image, gt_rgb, depth, gt_m = (t.to(dev) for t in (rnd(1, n, 3), rnd(1, n, 3), rnd(1, n) * 100 * scale, gt_m))
    image.requires_grad_()
    depth.requires_grad_()

    def fused():
        a, b = CameraLossFn.apply(image, depth, gt_rgb, gt_m, 1.0, 1.0, scale, "l1")
        image.grad = depth.grad = None
        (a + b).backward()

    def unfused():
        a = MseSumFn.apply(image, gt_rgb, 1.0)
        b = rgb_depth_loss_host(depth, gt_m, scale, "l1", 1.0)
        image.grad = depth.grad = None
        (a + b).backward()
    leg = versus(fused, {"mse_sum_plus_torch": unfused}, reps)
    leg["rays"] = n
    return leg


def train_step_leg(dev, reps, n=4096, T=768):
    from nvsf.nerf.models.network_static import NeRFNetworkStatic
    torch.manual_seed(0)
    model = NeRFNetworkStatic(bound=S.BOUND, min_near=S.MIN_NEAR, min_near_lidar=S.MIN_NEAR, lidar_max_depth=S.LIDAR_MAX_DEPTH,
                              num_frames=S.NUM_FRAMES).to(dev)
    rng = np.random.default_rng(1000)
    lo, ld = S.lidar_rays(n, rng)
    co, cd = S.camera_rays(n, rng)
    to = lambda a: torch.from_numpy(a).to(dev)[None]
    g = torch.Generator(device="cpu").manual_seed(3)
    batch = {"rays_o_lidar": to(lo), "rays_d_lidar": to(ld), "rays_o": to(co), "rays_d": to(cd), "time": torch.tensor([[0.5]], device=dev),
             "gt_depth": torch.rand(1, n, generator=g).to(dev) * 0.5, "gt_raydrop": (torch.rand(1, n, generator=g) > 0.3).float().to(dev),
             "gt_intensity": torch.rand(1, n, generator=g).to(dev), "gt_rgb": torch.rand(1, n, 3, generator=g).to(dev)}
    gt_m = torch.rand(1, n, generator=g) * 95 + 0.5
    gt_m[torch.rand(1, n, generator=g) < 0.85] = 0.0
    batch["gt_rgb_depth"] = gt_m.to(dev)
    on = RenderTrainStep(model, num_steps=T, scale=S.SCALE, use_rgbd_loss=True)
    off = RenderTrainStep(copy.deepcopy(model), num_steps=T, scale=S.SCALE)
    plain = {k: v for k, v in batch.items() if k != "gt_rgb_depth"}

    def run(step, b):
        step.step(b)
        step.sync()
    leg = versus(lambda: run(on, batch), {"term_off": lambda: run(off, plain)}, reps, warm=8)
    leg.update(rays="4096 + 4096", samples=T, parts_on=sorted(on.step(batch)[1]))
    return leg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"unit": "ms (device events)", "reps": args.reps}
    res.update(depth_image_legs(dev, args.reps))
    res["camera_loss"] = camera_loss_leg(dev, args.reps)
    res["train_step"] = train_step_leg(dev, args.reps)
    res["device"] = torch.cuda.get_device_name(0)
    res["build_digest"] = _hip.build_digest()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
