"""LiDAR cloud cleaning on the device (csrc/pointcloud.hip via nvsf/nerf/pointcloud.py).

Oracles: scipy's cKDTree in float64 for the neighbour statistic (Open3D's published definition of remove_statistical_outlier: k-nearest
search of the cloud against itself, self included, per-point mean of the Euclidean distances, mu over all points,
sigma = sqrt(sum (m - mu)^2 / (N - 1)), keep where 0 < m < mu + std_ratio sigma), float64 numpy for the plane tests.

The scene: a 66 x 1030 range image, intrinsics (2.0, 26.9) / (180, 360), ground plane z = -1.7 m, ten axis-aligned boxes within
+-35 m, ranges above 80 m and a random 10 % of the pixels dropped, 0.2 % of the pixels replaced by a uniform range in [5, 60] m
(nvsf.synthetic.street_range_image, seeded).

Bar of the neighbour statistic: relative error <= 1e-5 per point (absolute 1e-6 m where the oracle mean is 0).  Squared distances from
coordinate differences carry <= ~4 ulp in fp32, the square root ~3 ulp on d, a 64-term fp32 sum at worst 64 ulp: ~70 x 2^-24 = 4e-6.
Measured on an MI355X: 1.64e-7 on the scene, <= 1.51e-7 on the small clouds; outlier mask identical to the oracle's; inlier counts exact.
"""
import os

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

from nvsf import synthetic as S
from nvsf.nerf import pointcloud as P
from nvsf.nerf.dataset import formats as F

pytestmark = pytest.mark.gpu

INTRINSICS, INTRINSICS_HOZ = (2.0, 26.9), (180.0, 360.0)
GROUND_Z = -1.7


def pano_to_lidar_numpy(pano):
    """Float64 restatement of train_step.pano_to_lidar: (points [n, 3], flat pixel index [n]) of the non-zero pixels, row-major."""
    H, W = pano.shape
    i, j = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    beta = -(i - W / 2) / W * INTRINSICS_HOZ[1] / 180 * np.pi
    alpha = (INTRINSICS[0] - j / H * INTRINSICS[1]) / 180 * np.pi
    dirs = np.stack([np.cos(alpha) * np.cos(beta), np.cos(alpha) * np.sin(beta), np.broadcast_to(np.sin(alpha), (H, W))], -1)
    keep = pano != 0.0
    return (dirs * pano.astype(np.float64)[..., None])[keep], np.flatnonzero(keep.reshape(-1))


def knn_mean_oracle(points, k):
    p = np.asarray(points, np.float64)
    d, _ = cKDTree(p).query(p, k=min(k, len(p)))
    return d.reshape(len(p), -1).mean(axis=1)


def check_knn(points, k, dev):
    """Every point against the oracle, and two runs bit for bit.  Returns the largest relative error."""
    pts = torch.from_numpy(np.ascontiguousarray(points, np.float32)).to(dev)
    got_t = P.knn_mean_distance(pts, k)
    again = P.knn_mean_distance(pts, k)
    assert got_t.dtype == torch.float32 and got_t.shape == (len(points),)
    assert torch.equal(got_t, again)
    got = got_t.cpu().numpy().astype(np.float64)
    want = knn_mean_oracle(np.ascontiguousarray(points, np.float32), k)
    zero = want == 0
    err = np.abs(got - want)
    rel = float((err[~zero] / want[~zero]).max()) if (~zero).any() else 0.0
    print(f"knn_mean_distance N={len(points)} k={k}: max rel err {rel:.3e}, max abs err at zero means "
          f"{float(err[zero].max()) if zero.any() else 0.0:.3e}")
    assert np.isfinite(got).all()
    assert (err[zero] <= 1e-6).all()
    assert rel <= 1e-5
    return rel


@pytest.fixture(scope="module")
def scene():
    """The scene's cloud after the range filter (dist_max 60), with its isolated-return flags and the oracle's per-point means."""
    pano, boxes, iso = S.street_range_image(np.random.default_rng(0))
    pts64, pix = pano_to_lidar_numpy(pano)
    pts = pts64.astype(np.float32)
    keep = P.range_filter(torch.from_numpy(pts), 1, 60).numpy()
    pts, isolated = np.ascontiguousarray(pts[keep]), iso.reshape(-1)[pix][keep]
    means = knn_mean_oracle(pts, 64)
    thr = means.mean() + 3.0 * means.std(ddof=1)
    print(f"scene: {len(keep)} points, {len(pts)} after the range filter, oracle keeps {int(((means > 0) & (means < thr)).sum())} "
          f"at threshold {thr:.3f} m; {int(isolated.sum())} isolated returns")
    return {"points": pts, "isolated": isolated, "means": means, "threshold": thr}


def test_knn_mean_distance_on_the_scene(dev, scene):
    from nvsf.nerf.evaluate import pano_to_lidar
    pano, _, _ = S.street_range_image(np.random.default_rng(0))
    on_dev = pano_to_lidar(torch.from_numpy(pano).to(dev), INTRINSICS, INTRINSICS_HOZ)
    assert on_dev.shape[0] == int((pano != 0).sum())  # the device's cloud is the restatement's, pixel for pixel
    assert 50000 <= len(scene["points"]) <= 60000
    for k in (64, 8, 1):
        check_knn(scene["points"], k, dev)


@pytest.mark.parametrize("n", [1, 37, 64, 1000, 1024 + 64 + 5, 4096 + 17])
@pytest.mark.parametrize("k", [1, 8, 64])
def test_knn_mean_distance_small_clouds(dev, n, k):
    """N = 1, N < k, N = the wave size, a random cloud, N not a multiple of the LDS tile / of the queries per workgroup."""
    rng = np.random.default_rng(n * 100 + k)
    check_knn(rng.standard_normal((n, 3)) * 10.0, k, dev)


@pytest.mark.parametrize("k", [1, 8, 64])
def test_knn_mean_distance_with_exact_duplicates(dev, k):
    rng = np.random.default_rng(7)
    pts = (rng.standard_normal((1500, 3)) * 5.0).astype(np.float32)
    pts[rng.choice(1500, size=100, replace=False)] = pts[0]  # ~100 copies of one point: their first ~100 neighbours are at 0
    got = P.knn_mean_distance(torch.from_numpy(pts).to(dev), k).cpu().numpy()
    assert (got[(pts == pts[0]).all(axis=1)] == 0).all()
    check_knn(pts, k, dev)


def test_remove_statistical_outlier_matches_the_oracle_mask(dev, scene):
    pts, means, thr = scene["points"], scene["means"], scene["threshold"]
    want = (means > 0) & (means < thr)
    kept, keep = P.remove_statistical_outlier(torch.from_numpy(pts).to(dev), 64, 3.0)
    keep = keep.cpu().numpy()
    assert np.array_equal(kept.cpu().numpy(), pts[keep])
    excused = np.abs(means - thr) <= 1e-4 * thr
    wrong = keep != want
    print(f"outlier filter: keeps {int(keep.sum())} of {len(pts)} (oracle {int(want.sum())}), {int(wrong.sum())} differ, "
          f"{int(excused.sum())} within 1e-4 of the threshold")
    assert excused.sum() <= 1e-3 * len(pts)
    assert not (wrong & ~excused).any()
    # an isolated return with no other point within 64 / 63 of the threshold has a mean above it (its own 0 and 63 larger terms)
    d, _ = cKDTree(pts.astype(np.float64)).query(pts[scene["isolated"]].astype(np.float64), k=2)
    far = np.flatnonzero(scene["isolated"])[d[:, 1] > thr * 64 / 63]
    print(f"isolated returns farther than the threshold from everything else: {len(far)} of {int(scene['isolated'].sum())}")
    assert len(far) >= 1
    assert not keep[far].any()


def plane_distance(points, planes):
    return np.abs(points.astype(np.float64) @ planes[:, :3].astype(np.float64).T + planes[:, 3].astype(np.float64))  # [N, K]


def test_plane_inlier_count_and_mask(dev, scene):
    pts = scene["points"]
    pts_d = torch.from_numpy(pts).to(dev)
    triples = torch.randint(0, len(pts), (64, 3), generator=torch.Generator().manual_seed(3))
    planes_d, valid = P.plane_from_triples(pts_d, triples.to(dev))
    assert bool(valid.all())
    planes = planes_d.cpu().numpy()
    thr = float(np.float32(0.15))  # what the kernel receives
    dist = plane_distance(pts, planes)
    want = (dist < thr).sum(axis=0)
    band = (np.abs(dist - thr) <= 1e-5).sum(axis=0)
    got = P.plane_inlier_count(pts_d, planes_d, 0.15).cpu().numpy()
    print(f"plane_inlier_count: max |count - float64 count| = {int(np.abs(got - want).max())}, band sizes up to {int(band.max())}, "
          f"counts {int(want.min())} .. {int(want.max())}")
    assert got.dtype == np.int32 and (np.abs(got - want) <= band).all()
    assert np.array_equal(got, P.plane_inlier_count(pts_d, planes_d, 0.15).cpu().numpy())
    # more hypotheses than one LDS chunk holds, and a cloud that is not a multiple of the workgroup
    many = planes_d.repeat(5, 1)[:300].contiguous()
    got_many = P.plane_inlier_count(pts_d[:50001].contiguous(), many, 0.15).cpu().numpy()
    dist_many = plane_distance(pts[:50001], many.cpu().numpy())
    assert (np.abs(got_many - (dist_many < thr).sum(axis=0)) <= (np.abs(dist_many - thr) <= 1e-5).sum(axis=0)).all()
    # the mask: the union over six planes, below z_max
    for rows, z_max in ((slice(0, 6), -1.0), (slice(6, 7), 100.0), (slice(0, 64), 0.0)):
        got_mask = P.plane_inlier_mask(pts_d, planes_d[rows].contiguous(), 0.15, z_max).cpu().numpy()
        want_mask = (dist[:, rows] < thr).any(axis=1) & (pts[:, 2] < np.float32(z_max))
        in_band = (np.abs(dist[:, rows] - thr) <= 1e-5).any(axis=1)
        assert got_mask.dtype == np.bool_ and not ((got_mask != want_mask) & ~in_band).any()
    assert not P.plane_inlier_mask(pts_d, planes_d[:0].contiguous(), 0.15, 0.0).any()


def test_fit_ground_on_the_scene(dev, scene):
    pts_d, _ = P.remove_statistical_outlier(torch.from_numpy(scene["points"]).to(dev))
    pts_d = pts_d.contiguous()
    pts = pts_d.cpu().numpy()
    ground = np.abs(pts[:, 2].astype(np.float64) - GROUND_Z) < 1e-3
    mask = P.fit_ground(pts_d, generator=torch.Generator().manual_seed(0)).cpu().numpy()
    off_plane = np.abs(pts[:, 2].astype(np.float64) - GROUND_Z) >= 0.3
    print(f"fit_ground: {int(mask.sum())} in the mask; recall {mask[ground].mean():.4f} of {int(ground.sum())} ground points; "
          f"{int(mask[~ground].sum())} of {int((~ground).sum())} other points in it")
    assert mask[ground].mean() >= 0.99
    assert not mask[~ground & off_plane].any()
    assert not mask[pts[:, 2] >= -1.0].any()
    again = P.fit_ground(pts_d, generator=torch.Generator().manual_seed(0)).cpu().numpy()
    assert np.array_equal(mask, again)
    assert np.array_equal(mask, P.fit_ground(pts_d).cpu().numpy())  # the default generator is seeded 0


# ---- three frames: a box that moves, non-identity poses -------------------------------------------------------------------------
SCALE = 0.01
LIDAR_MAX_DEPTH_M = 80.0


def make_frames(root, dev):
    rng = np.random.default_rng(5)
    _, boxes, _ = S.street_range_image(rng)
    panos, isolated, poses = [], [], []
    for i in range(3):
        moved = boxes.copy()
        moved[0, [0, 3]] += 1.5 * i  # the first box drives along x
        pano, _, iso = S.street_range_image(rng, boxes=moved)
        yaw = 0.1 * (i + 1)
        pose = np.eye(4)
        pose[:3, :3] = [[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]]
        pose[:3, 3] = [0.02 * i, -0.01 * i, 0.005]
        panos.append(pano), isolated.append(iso.reshape(-1)), poses.append(pose)
    seq = "0000"
    os.makedirs(os.path.join(root, "train", seq), exist_ok=True)
    frames = [{"frame_id": 10 + i, "file_path": f"train/{seq}/img_{i:04d}.npy", "transform_matrix": poses[i],
               "lidar_file_path": f"train/{seq}/pano_{i:04d}.npy", "lidar2world": poses[i]} for i in range(3)]
    H, W = 4, 6
    F.write_transforms(F.transforms_path(root, seq, "train"), w=W, h=H, w_lidar=panos[0].shape[1], h_lidar=panos[0].shape[0],
                       K=np.array([[5.0, 0, 3], [0, 5.0, 2], [0, 0, 1]]), frame_start=10, frame_end=12, num_frames=3, frames=frames)
    range_images = [np.stack([np.zeros_like(p), np.full_like(p, 0.5), p], axis=-1) for p in panos]
    fs = F.FrameSet(root, seq, "train", SCALE, intrinsics_lidar=INTRINSICS, intrinsics_hoz_lidar=INTRINSICS_HOZ, device=dev, training=False,
                    images=[np.zeros((H, W, 3), np.uint8)] * 3, range_images=range_images)
    return fs, panos, isolated, [np.asarray(p, np.float32) for p in poses]


def test_process_pointcloud_on_three_frames(dev, tmp_path):
    from nvsf.nerf.evaluate import pano_to_lidar
    fs, panos, isolated, poses = make_frames(str(tmp_path), dev)
    pc_list, ground_list = P.process_pointcloud(fs, LIDAR_MAX_DEPTH_M * SCALE, generator=torch.Generator().manual_seed(0))
    assert sorted(pc_list) == [0, 1, 2] and sorted(ground_list) == [0, 1, 2]
    assert all(isinstance(k, int) for k in pc_list)
    n_far = 0
    gen = torch.Generator().manual_seed(0)  # the restatement draws what process_pointcloud drew, frame by frame
    for i in range(3):
        # the selection runs on the device's own points; the coordinates are restated in float64 from the range image
        local = pano_to_lidar(fs.images_lidar[i][..., 2] * fs.images_lidar[i][..., 0] / SCALE, INTRINSICS, INTRINSICS_HOZ).contiguous()
        local64, pix = pano_to_lidar_numpy(panos[i])
        assert local.shape == local64.shape
        m1 = P.range_filter(local, 1, 0.75 * LIDAR_MAX_DEPTH_M, (-2.5, 4))
        idx = torch.nonzero(m1)[:, 0]
        _, keep = P.remove_statistical_outlier(local[idx].contiguous())
        idx = idx[keep]
        g = P.fit_ground(local[idx].contiguous(), generator=gen)
        idx_ground, idx = idx[g], idx[~g]
        _, keep = P.remove_statistical_outlier(local[idx].contiguous())
        idx = idx[keep].cpu().numpy()
        got, got_ground = pc_list[i].cpu().numpy(), ground_list[i].cpu().numpy()
        assert pc_list[i].device.type == "cuda" and pc_list[i].dtype == torch.float32 and pc_list[i].is_contiguous()
        assert got.shape == (len(idx), 3) and got_ground.shape == (len(idx_ground), 3) and len(idx) > 500
        pose = poses[i].astype(np.float64)
        want = (local64[idx] * SCALE) @ pose[:3, :3].T + pose[:3, 3]
        want_ground = (local64[idx_ground.cpu().numpy()] * SCALE) @ pose[:3, :3].T + pose[:3, 3]
        print(f"frame {i}: {len(idx)} points, {len(idx_ground)} ground; max |world - restatement| = {np.abs(got - want).max():.2e}")
        assert np.abs(got - want).max() <= 1e-6 and np.abs(got_ground - want_ground).max() <= 1e-6
        # no ground and no isolated return is left
        kept_local = local64[idx]
        assert not (np.abs(kept_local[:, 2] - GROUND_Z) < 1e-3).any()
        assert (local64[idx_ground.cpu().numpy()][:, 2] < -1.0).all()
        iso = isolated[i][pix]
        d, _ = cKDTree(local64).query(local64[iso], k=2)
        means = knn_mean_oracle(local64[m1.cpu().numpy()], 64)
        thr = means.mean() + 3 * means.std(ddof=1)
        far = np.flatnonzero(iso)[d[:, 1] > thr * 64 / 63]
        n_far += len(far)
        assert not np.isin(far, idx).any()
    assert n_far >= 1
    # the box that moves shows up as a displacement between the frames' clouds in the lidar frame: the clouds differ
    assert pc_list[0].shape != pc_list[2].shape or not torch.equal(pc_list[0], pc_list[2])


def test_flow_loss_end_to_end(dev, tmp_path):
    """RenderTrainStep(flow_loss=True, pc_list=process_pointcloud(...)[0]) on the space-time network: a finite flow term and gradients on
    the flow parameters for the middle frame (both neighbours exist)."""
    from nvsf.nerf.models.network_dynamic import NeRFNetwork
    from nvsf.nerf.train_step import RenderTrainStep
    fs, _, _, _ = make_frames(str(tmp_path), dev)
    pc_list, _ = P.process_pointcloud(fs, LIDAR_MAX_DEPTH_M * SCALE)
    torch.manual_seed(0)
    model = NeRFNetwork(time_resolution=8, num_frames=3, bound=S.BOUND, min_near=S.MIN_NEAR, min_near_lidar=S.MIN_NEAR,
                        lidar_max_depth=LIDAR_MAX_DEPTH_M * SCALE).to(dev)
    step = RenderTrainStep(model, scale=SCALE, ema_decay=None, flow_loss=True, pc_list=pc_list)
    assert all(float(pc.abs().max()) < S.BOUND for pc in pc_list.values())
    loss = step.flow_loss(fs.times[1].reshape(1, 1))
    assert loss is not None and torch.isfinite(loss) and float(loss) > 0
    loss.backward()
    grads = [p.grad for p in model.flow_net.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads) and sum(float(g.abs().sum()) for g in grads) > 0
    assert step.flow_loss(torch.tensor([[0.0]], device=dev)) is not None  # the first frame: forward term only
