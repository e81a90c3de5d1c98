"""Prediction export on the device (csrc/export.hip, include/nvsf_hip.h section 14): a rendered frame -> the simulated LiDAR sweep as
point clouds in the LiDAR and the world frame, and the uint8 planes of the image files.

The reference's Trainer.test (nvsf/nerf/trainer.py:1109-1283) renders every frame of a split with test_step, quantises the planes with
`(pred * 255).astype(np.uint8)`, builds the cloud with utils.get_pcd_bound_to_world (nvsf/nerf/utils.py:444-474) over
convert.pano_to_lidar_with_intensities (nvsf/lib/convert.py:221-268) and writes text clouds, a PCD file and PNGs.  Here the per-pixel
work is one call into the library each; the host reads one count per cloud and the finished arrays.

Deviations from the reference, all deliberate:
  * get_pcd_bound_to_world rescales the translation of `frame_data['poses_lidar']` IN PLACE (`.numpy()` shares the tensor's memory), so
    the batch's pose is altered by the call and a second call on the same batch -- evaluate_one_epoch makes two per frame
    (trainer.py:1681, 1688) -- rescales it twice.  pano_to_cloud works on a copy.
  * The colour maps of the reference's PNGs (cv2.applyColorMap, tables 1 and 20) are cv2's; without cv2 the planes are written greyscale.
  * The PCD file is the reference's through Open3D; ours is PCD v0.7 ASCII with the fields x y z intensity, a layout of our own.
  * No mp4 (imageio).
"""
import os

import numpy as np
import torch

# csrc/export.hip: kPixels, the consecutive pixels one workgroup of the compaction counts and places.  A constant so that it can be read
# without the library; library_sizes() returns the library's own value and tests/test_export_cpu.py holds the two together.
PIXELS_PER_WORKGROUP = 1024
MAX_PIXELS = 1 << 24         # H W of one range image


def _check_plane(t, name, who, shape=None):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{who}: {name} must be a torch tensor on a HIP device, got {type(t).__name__}")
    if not t.is_cuda:
        raise ValueError(f"{who}: {name} is a CPU tensor; the export runs on the HIP device and has no CPU fallback")
    if t.dtype != torch.float32:
        raise ValueError(f"{who}: {name} must be float32, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{who}: {name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def world_matrix(pose_lidar, scale, offset):
    """utils.py:466-467 on a COPY of the fp32 pose: `T[:3, 3] = T[:3, 3] / scale + offset`, an fp32 division, the float64 sum with the
    offset rounded back to fp32 by the assignment.  Returns [4, 4] fp32 (numpy)."""
    T = np.array(pose_lidar.detach().cpu().numpy() if torch.is_tensor(pose_lidar) else pose_lidar, dtype=np.float32, copy=True)
    if T.shape != (4, 4):
        raise ValueError(f"pano_to_cloud: pose_lidar must be [4, 4], got {T.shape}")
    T[:3, 3] = (T[:3, 3] / scale) + np.asarray(offset, dtype=np.float64)
    return T


def workspace_bytes(n_pixels):
    """Workspace of nvsf_pano_to_cloud by the header's formula: one uint32 per workgroup."""
    return 4 * ((int(n_pixels) + PIXELS_PER_WORKGROUP - 1) // PIXELS_PER_WORKGROUP)


def library_sizes(H, W):
    """(workspace bytes, pixels per workgroup) of nvsf_pano_to_cloud at H x W as the LIBRARY states them (nvsf_pano_to_cloud_sizes; no
    launch, needs no device).  pano_to_cloud sizes its workspace by this."""
    import ctypes
    from nvsf import _hip
    sizes = (ctypes.c_uint64 * 2)()
    status = _hip.load().nvsf_pano_to_cloud_sizes(int(H), int(W), ctypes.cast(sizes, ctypes.c_void_p), None)
    if status != 0:
        raise _hip.NvsfHipError(f"nvsf_pano_to_cloud_sizes rejected {H} x {W} (status {status})")
    return int(sizes[0]), int(sizes[1])


def pano_to_cloud(range_image, payload, pose_lidar, scale, offset, intrinsics, intrinsics_hoz=(180.0, 360.0), capacity=None):
    """utils.get_pcd_bound_to_world.  range_image [H, W] fp32 in scene units (device), payload [H, W] fp32 or None (column 3 is then 0),
    pose_lidar [4, 4] sensor-to-world in scene units or None (no world cloud), scale / offset: world = pose / scale + offset,
    intrinsics = (fov_up, fov), intrinsics_hoz = (fov_hoz_up, fov_hoz), degrees.
    Returns (cloud_lidar [n, 4] fp32, cloud_world [n, 4] fp64 or None) on the device: one row per pixel of range != 0, row-major pixel
    order, x y z in metres (the LiDAR-frame coordinates are divided by `scale` in fp32) and the payload.  One device -> host read, for
    the count.  `capacity`: rows to allocate (default H W, which always holds the cloud); a smaller one keeps the first rows and the
    returned views are that long.  The two results are VIEWS of the buffers of `capacity` rows (16 + 32 bytes per row), which stay
    alive with them: nothing at the 68 k pixels of a sweep, 768 MB near the 2^24-pixel limit -- `.clone()` them to let the rest go."""
    from nvsf import _hip
    who = "pano_to_cloud"
    r = _check_plane(range_image, "range_image", who)
    if r.dim() != 2 or r.shape[0] < 1 or r.shape[1] < 1:
        raise ValueError(f"{who}: range_image must be [H, W] with H, W >= 1, got {tuple(r.shape)}")
    H, W = int(r.shape[0]), int(r.shape[1])
    if H * W > MAX_PIXELS:
        raise ValueError(f"{who}: {H} x {W} exceeds the {MAX_PIXELS} pixels one range image may hold")
    if payload is not None:
        _check_plane(payload, "payload", who, (H, W))
        if payload.device != r.device:
            raise ValueError(f"{who}: payload is on {payload.device}, range_image on {r.device}")
    scale = float(scale)
    fov_up, fov, fov_hoz = float(intrinsics[0]), float(intrinsics[1]), float(intrinsics_hoz[1])
    if not (scale > 0 and fov > 0 and fov_hoz > 0):
        raise ValueError(f"{who}: scale, fov and fov_hoz must be positive, got {scale}, {fov}, {fov_hoz}")
    T = None if pose_lidar is None else world_matrix(pose_lidar, scale, offset).astype(np.float64)
    cap = H * W if capacity is None else int(capacity)
    if cap < 0:
        raise ValueError(f"{who}: capacity must be >= 0")
    dev = r.device
    with torch.cuda.device(dev):
        ws = torch.empty((library_sizes(H, W)[0] + 3) // 4, dtype=torch.int32, device=dev)
        lidar = torch.empty(max(cap, 1), 4, dtype=torch.float32, device=dev)
        world = torch.empty(max(cap, 1), 4, dtype=torch.float64, device=dev) if T is not None else None
        count = torch.empty(1, dtype=torch.int32, device=dev)
        _hip.call("nvsf_pano_to_cloud", _hip.ptr(r.contiguous()), _hip.ptr(payload.contiguous()) if payload is not None else None, H, W,
                  _hip.host_f64([fov_up, fov, fov_hoz, scale]), _hip.host_f64(T.reshape(-1)) if T is not None else None, _hip.ptr(ws),
                  ws.numel() * 4, _hip.ptr(lidar), _hip.ptr(world), cap, _hip.ptr(count))
        n = min(int(count.item()), cap)
    return lidar[:n], (world[:n] if world is not None else None)


def quantize_u8(x, srgb=False):
    """`(x * 255).astype(np.uint8)` on the device (fp32 product, truncation), after utils.linear_to_srgb when `srgb`; uint8, shape of x.
    Where numpy's cast is undefined it saturates: product <= -1 -> 0, >= 256 -> 255, NaN -> 0."""
    from nvsf import _hip
    x = _check_plane(x, "x", "quantize_u8").contiguous()
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _hip.call("nvsf_quantize_u8", _hip.ptr(x) if x.numel() else None, x.numel(), 1 if srgb else 0, _hip.ptr(out) if x.numel() else None)
    return out


def linear_to_srgb(x):
    """utils.linear_to_srgb (utils.py:31-36) on the device, fp32: where(x < 0.0031308, 12.92 x, 1.055 x^0.41666 - 0.055)."""
    from nvsf import _hip
    x = _check_plane(x, "x", "linear_to_srgb").contiguous()
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _hip.call("nvsf_linear_to_srgb", _hip.ptr(x) if x.numel() else None, x.numel(), _hip.ptr(out) if x.numel() else None)
    return out


# ---- file writers (host) ---------------------------------------------------------------------------------------------------------

def write_cloud_txt(path, cloud):
    """np.savetxt(path, cloud, fmt="%f"), space-delimited: the reference's `_pcd_world.txt` / `_pcd_lidar.txt`."""
    np.savetxt(path, np.asarray(cloud).reshape(-1, 4), fmt="%f", delimiter=" ")


def write_pcd(path, cloud):
    """PCD v0.7, ASCII, fields x y z intensity (float32).  The reference writes this file through Open3D, which is not available: the
    layout is this project's, not pinned to Open3D's output."""
    c = np.asarray(cloud, dtype=np.float32).reshape(-1, 4)
    n = c.shape[0]
    with open(path, "w") as f:
        f.write("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\n"
                f"WIDTH {n}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\nDATA ascii\n")
        np.savetxt(f, c, fmt="%.6f", delimiter=" ")


def write_png(path, array_u8):
    """uint8 [H, W] (greyscale) or [H, W, 3] (RGB) through PIL."""
    from PIL import Image
    a = np.ascontiguousarray(array_u8, dtype=np.uint8)
    Image.fromarray(a, mode="L" if a.ndim == 2 else "RGB").save(path)


def frame_paths(out_dir, name, i):
    """The reference's file names for frame i (trainer.py:1169-1254)."""
    stem = os.path.join(out_dir, f"test_{name}_{i:04d}")
    return {"pcd_world": stem + "_pcd_world.txt", "pcd_lidar": stem + "_pcd_lidar.txt", "pcd": stem + "_pcd_lidar.pcd", "lidar_png": stem + ".png",
            "rgb": os.path.join(out_dir, f"{name}_{i:04d}_rgb.png"), "rgb_depth": os.path.join(out_dir, f"{name}_{i:04d}_rgb_depth.png")}


def write_frame(out_dir, name, i, raydrop_u8, intensity_u8, range_u8, rgb_u8, rgb_depth_u8, cloud_lidar, cloud_world):
    """Writes the six files of one frame from host arrays; returns their paths."""
    p = frame_paths(out_dir, name, i)
    write_cloud_txt(p["pcd_world"], cloud_world)
    write_cloud_txt(p["pcd_lidar"], cloud_lidar)
    write_pcd(p["pcd"], cloud_lidar)
    write_png(p["lidar_png"], np.concatenate([raydrop_u8, intensity_u8, range_u8], axis=0))
    write_png(p["rgb"], rgb_u8)
    write_png(p["rgb_depth"], rgb_depth_u8)
    return p


def export_frames(model, frames, out_dir, name, num_steps, refiner=None, color_space="srgb", indices=None, ema=None, raydrop_thres=0.5,
                  alpha_r=0.01, write=True, **test_kwargs):
    """The reference's Trainer.test over a FrameSet opened with training=False (and, for a novel sensor, sensor=SensorChange(...)):
    per frame test_step, the quantised planes, the two clouds, the files of frame_paths.  Planes as trainer.py:1147-1194: the ray-drop mask
    `pred_raydrop > raydrop_thres`, the intensity, the range and the camera depth (both in scene units, as there) and the image, each
    times 255 and truncated; the image goes through linear_to_srgb first when color_space == "linear".  The cloud's fourth column is
    the QUANTISED intensity as a float, as the reference passes `img_intensity_pred` (trainer.py:1197-1204).  `ema`: evaluate under the averaged weights, as evaluate_frames.
    Across ranks every rank calls this (test_step splits a frame's rays over them); `write=False` on all but one keeps the files single.
    Returns the per-frame point counts."""
    from nvsf.nerf.evaluate import test_step
    if color_space not in ("srgb", "linear"):
        raise ValueError("color_space: 'srgb' or 'linear'")
    if write:
        os.makedirs(out_dir, exist_ok=True)
    was_training = model.training
    model.eval()
    if ema is not None:
        ema.store()
        ema.copy_to()
    counts = []
    try:
        for i in (range(len(frames)) if indices is None else indices):
            data = frames.collate([int(i)])
            rgb, rgb_depth, raydrop, intensity, depth = test_step(model, data, num_steps, alpha_r=alpha_r, raydrop_thres=raydrop_thres,
                                                                  refiner=refiner, **test_kwargs)
            raydrop, intensity, depth = raydrop[0].float().contiguous(), intensity[0].float().contiguous(), depth[0].float().contiguous()
            raydrop_u8 = quantize_u8((raydrop > raydrop_thres).to(torch.float32))
            intensity_u8 = quantize_u8(intensity)
            range_u8 = quantize_u8(depth)
            rgb_u8 = quantize_u8(rgb[0].float(), srgb=(color_space == "linear"))
            rgb_depth_u8 = quantize_u8(rgb_depth[0].float())
            lidar, world = pano_to_cloud(depth, intensity_u8.to(torch.float32), data["poses_lidar"][0], frames.scale, frames.offset,
                                         frames.intrinsics_lidar, frames.intrinsics_hoz_lidar)
            if write:
                write_frame(out_dir, name, int(i), raydrop_u8.cpu().numpy(), intensity_u8.cpu().numpy(), range_u8.cpu().numpy(),
                            rgb_u8.cpu().numpy(), rgb_depth_u8.cpu().numpy(), lidar.cpu().numpy(), world.cpu().numpy())
            counts.append(int(lidar.shape[0]))
    finally:
        if ema is not None:
            ema.restore()
        model.train(was_training)
    return counts
