"""Static / dynamic object masks on the device, and the range-image z-buffer (csrc/object_masks.hip, include/nvsf_hip.h section 12).

The reference reports its evaluation table over the whole frame, over the static background and over the annotated moving objects
(trainer.py:1545-1626).  The masks come from utils.compute_object_masks (nvsf/nerf/utils.py:750-807: range image -> cloud ->
scipy Delaunay membership per box -> lidar_to_pano_with_intensities, a Python loop over the points) and utils.compute_object_masks_img
(:810-873, a double Python loop over pixels).  Here the per-box host arithmetic (a few 4 x 4 products) stays on the host in the
reference's dtypes and everything per point or per pixel is one call into the library.  NumPy only; no scipy.

lidar_to_pano / range_view are the same z-buffer as a preprocessing step: a raw sweep -> the range-image array formats.py reads
(preprocess/generate_rangeview.py:185-258).
"""
import itertools
import json

import numpy as np
import torch

KMAX = 12        # faces of the hull of eight points in general position (triangles); a parallelepiped has 6
MAX_PLANES = 768  # B * KMAX of one launch (the library's LDS budget: 24 KiB)


def _on_device(t, name, who):
    from nvsf import _hip
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{who}: {name} must be a torch tensor on a HIP device, got {type(t).__name__}")
    if not t.is_cuda:
        raise _hip.NvsfHipError(f"{who}: {name} is a CPU tensor; the object masks are built on the HIP device and have no CPU fallback")
    return t


def hull_planes(vertices):
    """vertices [8, 3] (any M >= 4 works) fp64 -> [K, 4] fp64: the supporting half-spaces (nx, ny, nz, d), n.p + d <= 0 inside, of the
    convex hull, unit outward normals.  Every vertex triple whose plane has all vertices on one side (within 1e-9 of the box size),
    duplicates merged (a quadrilateral face is found by four triples); K <= 12 for eight points, 6 for a parallelepiped."""
    v = np.asarray(vertices, dtype=np.float64)
    if v.ndim != 2 or v.shape[1] != 3 or v.shape[0] < 4:
        raise ValueError(f"hull_planes: expected [M >= 4, 3] vertices, got {v.shape}")
    size = float(np.linalg.norm(v.max(0) - v.min(0)))
    if not size > 0.0:
        raise ValueError("hull_planes: the vertices coincide")
    tol = 1e-9 * size
    planes = []
    for i, j, k in itertools.combinations(range(v.shape[0]), 3):
        n = np.cross(v[j] - v[i], v[k] - v[i])
        length = np.linalg.norm(n)
        if length <= 1e-9 * size * size:  # collinear triple
            continue
        n = n / length
        d = -float(n @ v[i])
        s = v @ n + d
        if np.all(s <= tol):
            p = np.array([n[0], n[1], n[2], d])
        elif np.all(s >= -tol):
            p = np.array([-n[0], -n[1], -n[2], -d])
        else:
            continue
        if not any(np.abs(p[:3] - q[:3]).max() <= 1e-7 and abs(p[3] - q[3]) <= 1e-7 * size for q in planes):
            planes.append(p)
    if len(planes) < 4:
        raise ValueError("hull_planes: the vertices are coplanar")
    return np.stack(planes, 0)


def pack_planes(hulls):
    """list of [K_b, 4] -> (planes [B, KMAX, 4] fp64, counts [B] uint32), host arrays in the layout of nvsf_points_in_hulls."""
    B = len(hulls)
    kmax = max([KMAX] + [h.shape[0] for h in hulls])
    if B * kmax > MAX_PLANES:
        raise ValueError(f"{B} boxes of up to {kmax} planes exceed the {MAX_PLANES} planes one launch stages in LDS")
    planes = np.zeros((B, kmax, 4), np.float64)
    counts = np.zeros(B, np.uint32)
    for b, h in enumerate(hulls):
        planes[b, :h.shape[0]] = h
        counts[b] = h.shape[0]
    return planes, counts


def _device_planes(planes, counts, device):
    p = torch.from_numpy(np.ascontiguousarray(planes, dtype=np.float64)).to(device)
    c = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.uint32).view(np.int32)).to(device)
    return p, c


def _geom(intrinsics, intrinsics_hoz, max_depth):
    from nvsf import _hip
    return _hip.host_f64([intrinsics[0], intrinsics[1], intrinsics_hoz[0], intrinsics_hoz[1], max_depth])


def points_in_hulls(points, planes, counts):
    """points [P, 3] fp32 (device), planes [B, K, 4] fp64 / counts [B] (host arrays, pack_planes) -> uint8 [P]: 1 where some box holds
    the point (the OR over boxes of tools.check_in_hull, utils.py:781-794)."""
    from nvsf import _hip
    who = "points_in_hulls"
    p = _on_device(points, "points", who)
    if p.dim() != 2 or p.shape[1] != 3 or p.dtype != torch.float32:
        raise ValueError(f"{who}: points must be float32 [P, 3], got {p.dtype} {tuple(p.shape)}")
    B, K = int(planes.shape[0]), int(planes.shape[1]) if planes.ndim == 3 else 0
    out = torch.empty(p.shape[0], dtype=torch.uint8, device=p.device)
    dp, dc = _device_planes(planes, counts, p.device) if B else (None, None)
    _hip.call("nvsf_points_in_hulls", _hip.ptr(p.contiguous()) if p.shape[0] else None, p.shape[0], _hip.ptr(dp), _hip.ptr(dc), B, K,
              _hip.ptr(out) if p.shape[0] else None)
    return out


def lidar_to_pano(points, H, W, intrinsics, intrinsics_hoz, max_depth):
    """points [P, 3 or 4] fp32 in the LiDAR frame (device; column 3 = intensity or any payload) -> (pano [H, W], intensities [H, W]) fp32:
    lidar_to_pano_with_intensities (lib/convert.py:105-181).  Three columns give zero intensities, as convert.lidar_to_pano does."""
    from nvsf import _hip
    who = "lidar_to_pano"
    p = _on_device(points, "points", who)
    if p.dim() != 2 or p.shape[1] not in (3, 4) or p.dtype != torch.float32:
        raise ValueError(f"{who}: points must be float32 [P, 3 or 4], got {p.dtype} {tuple(p.shape)}")
    H, W, P = int(H), int(W), p.shape[0]
    xyz = p[:, :3].contiguous()
    payload = p[:, 3].contiguous() if p.shape[1] == 4 else None
    ws = torch.empty(H * W, dtype=torch.int64, device=p.device)
    pano = torch.empty(H, W, dtype=torch.float32, device=p.device)
    inten = torch.empty(H, W, dtype=torch.float32, device=p.device) if payload is not None else None
    _hip.call("nvsf_lidar_to_pano", _hip.ptr(xyz) if P else None, _hip.ptr(payload) if P else None, P, H, W,
              _geom(intrinsics, intrinsics_hoz, max_depth), _hip.ptr(ws), ws.numel() * 8, _hip.ptr(pano), _hip.ptr(inten))
    return pano, (inten if inten is not None else torch.zeros_like(pano))


def range_view(points, H, W, intrinsics, intrinsics_hoz, max_depth):
    """LiDAR_2_Pano (preprocess/generate_rangeview.py:185-217): [H, W, 3] fp32 with channel 1 = intensity, 2 = range, 0 left zero --
    the array a `lidar_file_path` of the data set holds."""
    pano, inten = lidar_to_pano(points, H, W, intrinsics, intrinsics_hoz, max_depth)
    return torch.stack([torch.zeros_like(pano), inten, pano], -1)


def _world_pose(pose, scale, offset):
    """The reference's `T[:3, 3] = T[:3, 3] / scale + offset` (utils.py:772, 835) on a COPY of the fp32 pose: fp32 division, the fp64 sum
    with the offset list rounded back to fp32 by the assignment."""
    T = np.array(pose.detach().cpu().numpy() if torch.is_tensor(pose) else pose, dtype=np.float32, copy=True)
    T[:3, 3] = (T[:3, 3] / scale) + np.asarray(offset, dtype=np.float64)
    return T


def _vertices_in(T_inv, vertices):
    v = np.asarray(vertices, dtype=np.float64)
    v = np.column_stack((v, np.ones(v.shape[0])))
    return np.matmul(T_inv, v.T).T[:, :3]


def lidar_frame_hulls(data, scale, offset):
    """The half-spaces of every annotated box of `data` in the LiDAR frame (utils.py:769-787): T_lidar2world fp32, its fp32 inverse,
    vertices through it in fp64."""
    T = _world_pose(data["poses_lidar"][0], scale, offset)
    T_inv = np.linalg.inv(T)
    return [hull_planes(_vertices_in(T_inv, ann["vertices"])) for ann in data["3d_annotation"]]


def compute_object_masks(depth, data, scale, offset, intrinsics_lidar, intrinsics_hoz_lidar, lidar_max_depth):
    """utils.compute_object_masks (utils.py:750-807).  depth [H, W] fp32 range image in scene units (device), data: the collated
    frame ("poses_lidar" [1, 4, 4], "3d_annotation": list of {"vertices": [8, 3] world frame, metres}), lidar_max_depth in scene units
    -> (static [H, W], dynamic [H, W]) fp32 on the device.  dynamic = 1 where the nearest point that re-projects into the pixel lies in
    a box; static = (dynamic == 0), so an empty pixel is static.  No annotation: ones / zeros."""
    from nvsf import _hip
    who = "compute_object_masks"
    d = _on_device(depth, "depth", who)
    if d.dim() != 2 or d.dtype != torch.float32:
        raise ValueError(f"{who}: depth must be float32 [H, W], got {d.dtype} {tuple(d.shape)}")
    H, W = d.shape
    planes, counts = pack_planes(lidar_frame_hulls(data, scale, offset))
    B = planes.shape[0]
    # depth / scale as numpy divides an fp32 array by a Python float: a true fp32 division by the rounded scale
    range_m = torch.div(d.contiguous(), torch.full((), float(scale), dtype=torch.float32, device=d.device))
    dyn = torch.empty(H, W, dtype=torch.float32, device=d.device)
    ws = torch.empty(H * W, dtype=torch.int64, device=d.device)
    dp, dc = _device_planes(planes, counts, d.device) if B else (None, None)
    _hip.call("nvsf_range_image_object_mask", _hip.ptr(range_m), H, W, _geom(intrinsics_lidar, intrinsics_hoz_lidar, lidar_max_depth / scale),
              _hip.ptr(dp), _hip.ptr(dc), B, planes.shape[1] if B else 0, _hip.ptr(ws), ws.numel() * 8, _hip.ptr(dyn))
    return (dyn == 0).to(torch.float32), dyn


def image_boxes(data, scale, offset):
    """The clamped 2-D boxes of utils.compute_object_masks_img (utils.py:823-856), host fp64: int32 [B', 4] = (x_min, y_min, x_max,
    y_max), inclusive.  A box with a vertex behind the camera (z <= 0) is skipped; `int()` truncates toward zero."""
    T_inv = np.linalg.inv(_world_pose(data["pose"][0], scale, offset))
    K = data["intrinsic_cam"]
    K = np.asarray(K.detach().cpu() if torch.is_tensor(K) else K)
    H, W = int(data["H"]), int(data["W"])
    boxes = []
    lim = 2 ** 31 - 1
    for ann in data["3d_annotation"]:
        v2 = np.matmul(K, _vertices_in(T_inv, ann["vertices"]).T).T
        if np.all(v2[:, 2] > 0):
            v2 = (v2 / v2[:, [2]])[:, :2]
            x_min, y_min = max(0, int(v2[:, 0].min())), max(0, int(v2[:, 1].min()))
            x_max, y_max = min(W - 1, int(v2[:, 0].max())), min(H - 1, int(v2[:, 1].max()))
            boxes.append([min(x_min, lim), min(y_min, lim), max(x_max, -lim), max(y_max, -lim)])
    return np.array(boxes, dtype=np.int32).reshape(-1, 4)


def box_mask_image(boxes, H, W, device):
    """boxes int32 [B, 4] (host) -> uint8 [H, W] on `device`: 1 inside any box."""
    from nvsf import _hip
    device = torch.device(device)
    if device.type != "cuda":
        raise _hip.NvsfHipError("box_mask_image: the mask is built on the HIP device and has no CPU fallback")
    boxes = np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 4)
    out = torch.empty(int(H), int(W), dtype=torch.uint8, device=device)
    db = torch.from_numpy(boxes).to(device) if boxes.shape[0] else None
    _hip.call("nvsf_box_mask_image", _hip.ptr(db), boxes.shape[0], int(H), int(W), _hip.ptr(out))
    return out


def compute_object_masks_img(data, scale, offset, device=None):
    """utils.compute_object_masks_img (utils.py:810-873) -> (static [H, W], dynamic [H, W]) fp32 on the device of data["pose"]."""
    device = data["pose"].device if device is None else device
    dyn = box_mask_image(image_boxes(data, scale, offset), data["H"], data["W"], device).to(torch.float32)
    return 1 - dyn, dyn


def load_annotations(path):
    """The project's JSON sidecar {"<frame_id>": [{"class": str, "vertices": [[x, y, z] x 8]}, ...]} (world frame, metres) ->
    {frame_id (int): [{"class": str, "vertices": fp64 [8, 3]}, ...]}."""
    with open(path) as f:
        raw = json.load(f)
    out = {}
    for fid, anns in raw.items():
        boxes = []
        for a in anns:
            v = np.asarray(a["vertices"], dtype=np.float64)
            if v.shape != (8, 3):
                raise ValueError(f"{path}: frame {fid}: a box needs 8 vertices of 3 coordinates, got {v.shape}")
            boxes.append({"class": str(a.get("class", "")), "vertices": v})
        out[int(fid)] = boxes
    return out
