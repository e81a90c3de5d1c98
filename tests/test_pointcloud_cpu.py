"""Host-side parts of the LiDAR cloud cleaning (nvsf/nerf/pointcloud.py) that run on CPU tensors for real: the
range / ego-vehicle filter and the planes through point triples against numpy restatements, Open3D's mean / sigma rule on a hand-made
vector, and the argument checks that must fire before any launch."""
import numpy as np
import pytest
import torch

from nvsf.nerf import pointcloud as P


def range_filter_numpy(pcd, dist_min, dist_max, z_limit):
    dist = np.sqrt(np.sum(pcd[:, :3] ** 2, axis=1))
    ego = (pcd[:, 0] > -2) & (pcd[:, 0] < 2) & (pcd[:, 1] > -1) & (pcd[:, 1] < 1) & (pcd[:, 2] > -2) & (pcd[:, 2] < 2)
    return (dist >= dist_min) & (dist <= dist_max) & (pcd[:, 2] > z_limit[0]) & (pcd[:, 2] < z_limit[1]) & ~ego


def test_range_filter_matches_numpy_and_cuts_the_ego_box():
    rng = np.random.default_rng(0)
    pts = (rng.standard_normal((5000, 3)) * [25.0, 25.0, 2.5]).astype(np.float32)
    named = np.array([[1.9, 0.9, 1.9],      # inside the ego box (distance 2.8 >= dist_min): cut
                      [1.9, 0.9, -1.9],     # inside the ego box
                      [2.1, 0.0, 0.0],      # just outside in x: kept
                      [0.0, 1.1, 0.0],      # just outside in y, distance 1.1 >= 1: kept
                      [0.0, 0.0, 2.5],      # above the box, inside z_limit: kept
                      [0.5, 0.5, 0.5],      # distance < dist_min and inside the box
                      [30.0, 0.0, 4.5],     # above z_limit
                      [30.0, 0.0, -2.6],    # below z_limit
                      [49.0, 9.0, 0.0],     # distance 49.8 <= 50: kept
                      [50.0, 9.0, 0.0]],    # distance 50.8 > 50
                     np.float32)
    pts = np.concatenate([named, pts])
    for args in ((1, 50, (-2.5, 4)), (1, 60, (-2.5, 4)), (2.5, 30.0, (-3.5, 4))):
        got = P.range_filter(torch.from_numpy(pts), *args)
        assert got.dtype == torch.bool and got.shape == (len(pts),)
        assert np.array_equal(got.numpy(), range_filter_numpy(pts, *args))
    got = P.range_filter(torch.from_numpy(pts)).numpy()
    assert got[:10].tolist() == [False, False, True, True, True, False, False, False, True, False]
    assert P.range_filter(torch.zeros(0, 3)).shape == (0,)
    # a fourth column (intensity) is ignored, as in the reference
    with_i = np.concatenate([pts, rng.random((len(pts), 1)).astype(np.float32) * 100], axis=1)
    assert np.array_equal(P.range_filter(torch.from_numpy(with_i)).numpy(), got)


def test_plane_from_triples_matches_numpy():
    rng = np.random.default_rng(1)
    pts = (rng.standard_normal((200, 3)) * 20).astype(np.float32)
    pts[10] = pts[11]                             # a repeated point
    pts[20], pts[21], pts[22] = [1, 2, 3], [2, 4, 6], [4, 8, 12]  # collinear, exactly representable
    triples = rng.integers(0, 200, size=(64, 3))
    triples[0] = [10, 11, 50]
    triples[1] = [20, 21, 22]
    triples[2] = [5, 5, 5]
    planes, valid = P.plane_from_triples(torch.from_numpy(pts), torch.from_numpy(triples))
    assert planes.dtype == torch.float32 and planes.shape == (64, 4) and valid.dtype == torch.bool
    p = pts.astype(np.float64)[triples]
    normal = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    length = np.linalg.norm(normal, axis=1)
    want_valid = length > 0
    assert not want_valid[:3].any() and want_valid[3:].sum() >= 55
    assert np.array_equal(valid.numpy(), want_valid)
    assert np.array_equal(planes.numpy()[~want_valid], np.zeros((int((~want_valid).sum()), 4), np.float32))
    unit = normal[want_valid] / length[want_valid, None]
    want = np.concatenate([unit, -(unit * p[want_valid, 0]).sum(1, keepdims=True)], axis=1)
    assert np.abs(planes.numpy()[want_valid] - want).max() <= 1e-6 * max(1.0, np.abs(want).max())
    got = planes.numpy()[want_valid].astype(np.float64)
    assert np.abs(np.linalg.norm(got[:, :3], axis=1) - 1).max() <= 1e-6
    for k in range(3):  # the three points of a triple lie on its plane
        assert np.abs((got[:, :3] * p[want_valid, k]).sum(1) + got[:, 3]).max() <= 1e-4


def test_statistical_outlier_rule_on_a_hand_made_vector():
    means = torch.tensor([1.0, 2.0, 3.0, 4.0, 0.0, 20.0])
    # mu = 5, sum (m - mu)^2 = 16 + 9 + 4 + 1 + 25 + 225 = 280, sigma = sqrt(280 / 5) = 7.4833
    thr = P.outlier_threshold(means, 1.0)
    assert thr.dtype == torch.float64 and abs(float(thr) - (5.0 + np.sqrt(56.0))) <= 1e-12
    assert P.outlier_keep_mask(means, 1.0).tolist() == [True, True, True, True, False, False]  # a mean of exactly 0 is dropped
    assert P.outlier_keep_mask(means, 3.0).tolist() == [True, True, True, True, False, True]   # 20 < 5 + 3 * 7.48
    assert abs(float(P.outlier_threshold(means, 3.0)) - (5.0 + 3 * np.sqrt(56.0))) <= 1e-12
    edge = torch.tensor([1.0, 1.0, 1.0, 1.0])   # sigma = 0: nothing is strictly below mu
    assert P.outlier_keep_mask(edge, 3.0).tolist() == [False] * 4
    assert P.outlier_keep_mask(torch.zeros(0), 3.0).shape == (0,)


def test_argument_errors_come_before_any_launch():
    good = torch.zeros(8, 3)
    for k in (0, -1, 65, 1000):
        with pytest.raises(ValueError):
            P.knn_mean_distance(good, k)
    for bad in (torch.zeros(8, 4), torch.zeros(8), torch.zeros(2, 8, 3), torch.zeros(8, 3, dtype=torch.float64),
                torch.zeros(8, 3, dtype=torch.float16), torch.zeros(3, 8).t(), torch.zeros(8, 6)[:, ::2], np.zeros((8, 3), np.float32)):
        for fn in (P.knn_mean_distance, P.remove_statistical_outlier, P.fit_ground):
            with pytest.raises(ValueError):
                fn(bad)
    with pytest.raises(ValueError):
        P.remove_statistical_outlier(good, nb_neighbors=65)
    with pytest.raises(ValueError):
        P.plane_inlier_count(good, torch.zeros(4, 3), 0.15)
    with pytest.raises(ValueError):
        P.plane_inlier_mask(good, torch.zeros(4, 4, dtype=torch.float64), 0.15, -1.0)
    with pytest.raises(ValueError):
        P.fit_ground(good, hypotheses=0)
    with pytest.raises(ValueError):
        P.plane_from_triples(good, torch.zeros(4, 2, dtype=torch.long))


def test_empty_cloud_needs_no_device():
    empty = torch.zeros(0, 3)
    out = P.knn_mean_distance(empty, 64)
    assert out.shape == (0,) and out.dtype == torch.float32
    kept, keep = P.remove_statistical_outlier(empty)
    assert kept.shape == (0, 3) and keep.shape == (0,) and keep.dtype == torch.bool
    assert P.fit_ground(empty).shape == (0,)
    assert P.plane_inlier_count(empty, torch.zeros(5, 4), 0.15).tolist() == [0] * 5
    assert P.plane_inlier_mask(empty, torch.zeros(5, 4), 0.15, -1.0).shape == (0,)
    points, ground = P.point_removal(torch.zeros(0, 3))
    assert points.shape == (0, 3) and ground.shape == (0, 3)
    # everything filtered away by the range filter: the same
    points, ground = P.point_removal(torch.tensor([[0.1, 0.1, 0.1], [100.0, 0.0, 0.0]]))
    assert points.shape == (0, 3) and ground.shape == (0, 3)
