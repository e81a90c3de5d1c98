"""LiDAR-projected camera depth maps on the device: the pseudo ground-truth camera depth image the reference builds for every frame
(nvsf/nerf/dataset/base_dataset.py:153-157: convert.pano_to_lidar -> dataset_utils.lidar2points2d -> dataset_utils.get_lidar_depth_image,
a Python loop over the points) as one launch for the whole split (csrc/projection.hip, include/nvsf_hip.h section 11).

Both functions take DEVICE tensors only; a CPU tensor raises, as the meters do.  Maps are in metres, 0 where no point landed.
"""
import numpy as np
import torch


def _on_device(t, name, who):
    from nvsf import _hip
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{who}: {name} must be a torch tensor on a HIP device, got {type(t).__name__}")
    if not t.is_cuda:
        raise _hip.NvsfHipError(f"{who}: {name} is a CPU tensor; the depth maps are built on the HIP device and have no CPU fallback")
    return t


def _intrinsics(K, who):
    K = np.asarray(K.detach().cpu() if torch.is_tensor(K) else K, dtype=np.float64)
    if K.ndim != 2 or K.shape[0] < 3 or K.shape[1] < 3:
        raise ValueError(f"{who}: K must be at least 3 x 3")
    return np.ascontiguousarray(K[:3, :3])  # lidar2points2d reads intrinsics[:3, :3]


def lidar_depth_images(range_images, poses, poses_lidar, K, H, W, intrinsics_lidar, intrinsics_hoz_lidar=(180.0, 360.0)):
    """range_images [F, Hl, Wl] fp32 in metres, poses / poses_lidar [F, 4, 4] fp32 (camera-to-world, LiDAR-to-world), K the 3 x 3 pinhole
    (host values), intrinsics_lidar = (fov_up, fov), intrinsics_hoz_lidar = (fov_hoz_up, fov_hoz) in degrees -> [F, H, W] fp32: per
    pixel the depth of the nearest range-image point that projects into it.  lidar2cam = inv(pose) @ pose_lidar is formed on the host
    in fp32, as base_dataset.py:155 forms it."""
    from nvsf import _hip
    who = "lidar_depth_images"
    r = _on_device(range_images, "range_images", who)
    for name, p in (("poses", poses), ("poses_lidar", poses_lidar)):
        _on_device(p, name, who)
    if r.dim() != 3 or r.dtype != torch.float32:
        raise ValueError(f"{who}: range_images must be float32 [F, Hl, Wl], got {r.dtype} {tuple(r.shape)}")
    F, Hl, Wl = r.shape
    if tuple(poses.shape) != (F, 4, 4) or tuple(poses_lidar.shape) != (F, 4, 4):
        raise ValueError(f"{who}: poses and poses_lidar must be [{F}, 4, 4]")
    cam = poses.detach().cpu().numpy().astype(np.float32)
    lid = poses_lidar.detach().cpu().numpy().astype(np.float32)
    l2c = np.stack([np.linalg.inv(cam[f]) @ lid[f] for f in range(F)], 0).astype(np.float32) if F else np.zeros((0, 4, 4), np.float32)
    l2c = torch.from_numpy(np.ascontiguousarray(l2c.reshape(F, 16))).to(r.device)
    Kh = _hip.host_f64(_intrinsics(K, who).reshape(-1))
    fov_up, fov = (float(v) for v in intrinsics_lidar)
    out = torch.empty(F, int(H), int(W), dtype=torch.float32, device=r.device)
    _hip.call("nvsf_lidar_depth_images", _hip.ptr(r.contiguous()), F, Hl, Wl, fov_up, fov, float(intrinsics_hoz_lidar[1]), _hip.ptr(l2c), Kh,
              int(H), int(W), _hip.ptr(out))
    return out


def points_depth_image(points, lidar2cam, K, H, W):
    """points [P, 3] fp32 in the LiDAR frame (device), lidar2cam 4 x 4 and K 3 x 3 (host values) -> [H, W] fp32 depth map."""
    from nvsf import _hip
    who = "points_depth_image"
    p = _on_device(points, "points", who)
    if p.dim() != 2 or p.shape[1] != 3 or p.dtype != torch.float32:
        raise ValueError(f"{who}: points must be float32 [P, 3], got {p.dtype} {tuple(p.shape)}")
    m = np.asarray(lidar2cam.detach().cpu() if torch.is_tensor(lidar2cam) else lidar2cam, dtype=np.float32)
    if m.shape != (4, 4):
        raise ValueError(f"{who}: lidar2cam must be 4 x 4")
    out = torch.empty(int(H), int(W), dtype=torch.float32, device=p.device)
    _hip.call("nvsf_points_depth_image", _hip.ptr(p.contiguous()) if p.shape[0] else None, p.shape[0], _hip.host_f32(m.reshape(-1)),
              _hip.host_f64(_intrinsics(K, who).reshape(-1)), int(H), int(W), _hip.ptr(out))
    return out
