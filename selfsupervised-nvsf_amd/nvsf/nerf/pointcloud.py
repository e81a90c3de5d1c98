"""The point clouds of the scene-flow loss, built on the device: Trainer.process_pointcloud (nvsf/nerf/trainer.py:1848-1912) over
utils.point_removal (nvsf/nerf/utils.py:151-268).

Per frame: range image -> points, range / ego-vehicle filter, statistical outlier removal, RANSAC ground fit (six rounds, union of
their inliers below z = -1 m), second outlier removal, transform to the scaled world frame.  The result feeds
`RenderTrainStep(flow_loss=True, pc_list=...)`.  The neighbour statistic and the plane inlier tests run on csrc/pointcloud.hip
(include/nvsf_hip.h section 9); there is no CPU fallback for them.  `range_filter` and `plane_from_triples` are plain tensor
expressions and also accept CPU tensors.

Deviations from the reference: the outlier filter follows Open3D's published definition (Open3D itself is not
a dependency); every RANSAC round scores a fixed batch of hypotheses drawn from a seeded `torch.Generator` instead of Python's global
`random` with adaptive stopping; a sample triple is rejected only when its normal has zero length.
"""
import torch

MAX_NEIGHBORS = 64  # one neighbour per lane of a wave (csrc/pointcloud.hip)
MIN_DY = 3.0        # metres between a triple's first two points along y (utils.py:173)


def _check_points(points, who):
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{who}: points must be a [N, 3] tensor")
    if points.dtype != torch.float32:
        raise ValueError(f"{who}: points must be float32")
    if not points.is_contiguous():
        raise ValueError(f"{who}: points must be contiguous")


def knn_mean_distance(points, k=MAX_NEIGHBORS):
    """[N] fp32: the mean Euclidean distance from every point to its min(k, N) nearest points of the same cloud, itself included."""
    from nvsf import _hip
    if not 1 <= int(k) <= MAX_NEIGHBORS:
        raise ValueError(f"knn_mean_distance: k must be in 1..{MAX_NEIGHBORS}, got {k}")
    _check_points(points, "knn_mean_distance")
    n = points.shape[0]
    out = torch.empty(n, dtype=torch.float32, device=points.device)
    if n == 0:
        return out
    _hip.call("nvsf_knn_mean_distance", _hip.ptr(points), n, int(k), _hip.ptr(out))
    return out


def outlier_threshold(means, std_ratio):
    """mu + std_ratio sigma of the per-point means in float64: mu over all points, sigma = sqrt(sum (m - mu)^2 / (N - 1))."""
    m = means.double()
    mu = m.mean()
    sigma = torch.sqrt(((m - mu) ** 2).sum() / max(m.numel() - 1, 1))
    return mu + float(std_ratio) * sigma


def outlier_keep_mask(means, std_ratio):
    """Open3D's rule on the per-point means: keep where 0 < m < mu + std_ratio sigma."""
    if means.numel() == 0:
        return torch.zeros(0, dtype=torch.bool, device=means.device)
    m = means.double()
    return (m > 0) & (m < outlier_threshold(means, std_ratio))


def remove_statistical_outlier(points, nb_neighbors=MAX_NEIGHBORS, std_ratio=3.0):
    """Open3D's remove_statistical_outlier: (kept points [M, 3], keep mask [N] bool)."""
    keep = outlier_keep_mask(knn_mean_distance(points, nb_neighbors), std_ratio)
    return points[keep], keep


def range_filter(points, dist_min=1, dist_max=50, z_limit=(-2.5, 4)):
    """[N] bool (utils.py:207-229): dist_min <= |p| <= dist_max, z inside z_limit, outside the ego-vehicle box |x| < 2, |y| < 1, |z| < 2."""
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] < 3:
        raise ValueError("range_filter: points must be a [N, >= 3] tensor")
    x, y, z = points[:, 0], points[:, 1], points[:, 2]
    dist = torch.sqrt((points[:, :3] ** 2).sum(dim=1))
    ego = (x > -2) & (x < 2) & (y > -1) & (y < 1) & (z > -2) & (z < 2)
    return (dist >= dist_min) & (dist <= dist_max) & (z > z_limit[0]) & (z < z_limit[1]) & ~ego


def plane_from_triples(points, triples):
    """Planes through point triples: (planes [K, 4] fp32 = (a, b, c, d) with unit normal (a, b, c) and d = -n . p0, valid [K] bool).
    A triple whose normal has zero length (repeated or collinear points) is invalid; its row is zero."""
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("plane_from_triples: points must be [N, 3]")
    if triples.dim() != 2 or triples.shape[1] != 3:
        raise ValueError("plane_from_triples: triples must be [K, 3]")
    p = points.double()[triples.long()]  # [K, 3, 3]
    normal = torch.linalg.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    length = torch.linalg.norm(normal, dim=1)
    valid = length > 0
    unit = normal / torch.where(valid, length, torch.ones_like(length))[:, None]
    planes = torch.cat([unit, -(unit * p[:, 0]).sum(dim=1, keepdim=True)], dim=1)
    return torch.where(valid[:, None], planes, torch.zeros_like(planes)).float().contiguous(), valid


def plane_inlier_count(points, planes, threshold):
    """[K] int32: points within `threshold` of each plane of planes [K, 4] (unit normals)."""
    from nvsf import _hip
    _check_points(points, "plane_inlier_count")
    _check_planes(planes, points, "plane_inlier_count")
    counts = torch.zeros(planes.shape[0], dtype=torch.int32, device=points.device)
    if points.shape[0] and planes.shape[0]:
        _hip.call("nvsf_plane_inlier_count", _hip.ptr(points), points.shape[0], _hip.ptr(planes), planes.shape[0], float(threshold),
                  _hip.ptr(counts))
    return counts


def plane_inlier_mask(points, planes, threshold, z_max):
    """[N] bool: within `threshold` of any plane of planes [R, 4] and z < z_max."""
    from nvsf import _hip
    _check_points(points, "plane_inlier_mask")
    _check_planes(planes, points, "plane_inlier_mask")
    mask = torch.zeros(points.shape[0], dtype=torch.uint8, device=points.device)
    if points.shape[0] and planes.shape[0]:
        _hip.call("nvsf_plane_inlier_mask", _hip.ptr(points), points.shape[0], _hip.ptr(planes), planes.shape[0], float(threshold),
                  float(z_max), _hip.ptr(mask))
    return mask.bool()


def _check_planes(planes, points, who):
    if planes.dim() != 2 or planes.shape[1] != 4 or planes.dtype != torch.float32 or not planes.is_contiguous():
        raise ValueError(f"{who}: planes must be [K, 4] float32 contiguous")
    if planes.device != points.device:
        raise ValueError(f"{who}: planes and points must be on one device")


def fit_ground(points, distance_threshold=0.15, rounds=6, hypotheses=64, z_max=-1.0, generator=None):
    """[N] bool ground mask.  Each of `rounds` rounds draws `hypotheses` index triples from `generator` (default: a CPU generator seeded
    0), drops those whose first two points are less than 3 m apart in y and the zero-area ones, counts the inliers of all of them in
    one launch and keeps the plane with the most (ties: lowest index).  The mask is the union of the kept planes' inliers with
    z < z_max.  A round without a usable triple contributes nothing."""
    _check_points(points, "fit_ground")
    if distance_threshold < 0 or rounds < 0 or hypotheses < 1:
        raise ValueError("fit_ground: distance_threshold >= 0, rounds >= 0, hypotheses >= 1")
    n, dev = points.shape[0], points.device
    if n < 3 or rounds == 0:
        return torch.zeros(n, dtype=torch.bool, device=dev)
    if generator is None:
        generator = torch.Generator().manual_seed(0)
    best = []
    for _ in range(rounds):
        triples = torch.randint(0, n, (hypotheses, 3), generator=generator, device=generator.device).to(dev)
        planes, valid = plane_from_triples(points, triples)
        valid &= (points[triples[:, 0], 1] - points[triples[:, 1], 1]).abs() >= MIN_DY
        counts = torch.where(valid, plane_inlier_count(points, planes, distance_threshold), torch.full_like(valid, -1, dtype=torch.int32))
        index = torch.arange(hypotheses, device=dev)
        top = torch.where(counts == counts.max(), index, hypotheses).min()  # the lowest index among the best
        row = torch.cat([planes[top], counts[top].float()[None]])
        best.append(row)
    rows = torch.stack(best).cpu()  # the one device -> host read of the fit
    chosen = rows[rows[:, 4] >= 0, :4].contiguous().to(dev)
    return plane_inlier_mask(points, chosen, distance_threshold, z_max)


def point_removal(pc_raw, dist_min=1, dist_max=50, z_limit=(-2.5, 4), generator=None):
    """utils.py:231-268: (points [P, 3] without ground and outliers, ground [G, 3]), both in the frame of `pc_raw` [N, >= 3]."""
    pc = pc_raw[:, :3].float()
    pc = pc[range_filter(pc, dist_min, dist_max, z_limit)].contiguous()
    pc, _ = remove_statistical_outlier(pc)
    pc = pc.contiguous()
    ground = fit_ground(pc, generator=generator)
    rest, _ = remove_statistical_outlier(pc[~ground].contiguous())
    return rest.contiguous(), pc[ground].contiguous()


def process_pointcloud(frames, lidar_max_depth, z_limit=(-2.5, 4), generator=None):
    """trainer.py:1848-1912 over a `FrameSet(training=False)`: (pc_list, pc_ground_list), dicts {frame index: [P, 3] fp32 device tensor}
    in the scaled world frame, keyed int(time * (num_frames - 1)) as RenderTrainStep.flow_loss looks them up."""
    from nvsf.nerf.evaluate import pano_to_lidar
    if generator is None:
        generator = torch.Generator().manual_seed(0)
    scale = float(frames.scale)
    num_frames = int(frames.meta["num_frames"])
    pc_list, pc_ground_list = {}, {}
    for i in range(len(frames)):
        pano = frames.images_lidar[i]
        rng = pano[..., 2] * pano[..., 0] / scale  # metres; dropped rays -> 0 -> no point
        local = pano_to_lidar(rng, frames.intrinsics_lidar, frames.intrinsics_hoz_lidar)
        points, ground = point_removal(local, dist_min=1, dist_max=0.75 * lidar_max_depth / scale, z_limit=z_limit, generator=generator)
        pose = frames.poses_lidar[i].float()
        key = int(float(frames.times[i]) * (num_frames - 1))
        pc_list[key] = ((points * scale) @ pose[:3, :3].T + pose[:3, 3]).contiguous()
        pc_ground_list[key] = ((ground * scale) @ pose[:3, :3].T + pose[:3, 3]).contiguous()
    return pc_list, pc_ground_list
