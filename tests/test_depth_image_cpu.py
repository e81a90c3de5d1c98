"""CPU tests of the LiDAR-projected camera depth maps and the camera depth loss (no GPU): the numpy restatement the GPU tests lean on
reproduces the reference's images; the reference's own share of boundary points stays under the caps the GPU tests allow; the host
branch of RenderTrainStep.losses equals the restatement of trainer.py:506-518 in depth_image_oracle.py."""
import numpy as np
import pytest
import torch

import depth_image_oracle as O


def test_numpy_restatement_reproduces_the_reference_images_bit_for_bit():
    fx = O.fixture()
    H, W = int(fx["H"]), int(fx["W"])
    for f in range(2):
        cloud = O.fixture_cloud(fx, f)
        assert np.array_equal(O.range_cloud(fx["range_m"][f], fx["fov"], fx["fov_hoz"]).view(np.uint32), cloud.view(np.uint32))
        uvz = O.project(cloud, fx["lidar2cam"][f], fx["K"])
        img = O.zbuffer(uvz, H, W)
        assert np.array_equal(img.view(np.uint32), O.fixture_image(fx, f"f{f}").view(np.uint32))
        # the stored fp64 (u, v, z) came out of numpy's matmul: the written-out sums agree to a few fp64 roundings
        np.testing.assert_allclose(uvz[fx[f"f{f}_view_idx"]], fx[f"f{f}_view_uvz"], rtol=1e-12, atol=1e-10)
    uvz = O.project(fx["list_points"], fx["list_lidar2cam"], fx["list_K"])
    assert np.array_equal(O.zbuffer(uvz, H, W).view(np.uint32), O.fixture_image(fx, "list").view(np.uint32))
    good = np.abs(fx["list_uvz"][:, :2]) < 1e7  # behind the camera (u, v) = q / 1e-5 is of the order 1e8: compare the rest
    np.testing.assert_allclose(uvz[:, :2][good], fx["list_uvz"][:, :2][good], rtol=1e-12, atol=1e-10)
    np.testing.assert_array_equal(uvz[:, 2], fx["list_uvz"][:, 2])


def test_point_list_follows_the_reference_on_the_bounds():
    fx = O.fixture()
    img = O.fixture_image(fx, "list")
    u, v = fx["list_uvz"][:, 0], fx["list_uvz"][:, 1]
    assert (u[40], u[41], v[42], v[43]) == (0.0, 1408.0, 0.0, 376.0) and (u[44], v[44], u[45], v[45]) == (0.0, 0.0, 1408.0, 376.0)
    assert img[188, 0] == 4.0 and img[0, 704] == 4.0 and img[0, 0] == 8.0          # u = 0 and v = 0 are inside
    assert img[195, 390] == np.float32(1e-5)                                        # a point BEHIND the camera, clipped into the image
    assert int(u[46]) == int(u[47]) and int(v[46]) == int(v[47]) and img[int(v[46]), int(u[46])] == 16.0  # equal depths, one pixel
    assert int(u[48]) == int(u[49]) and img[int(v[48]), int(u[48])] == 12.0         # the nearer of two
    behind = fx["list_points"][1:40, 0] < 0
    assert behind.all() and not ((u[1:40] >= 0) & (u[1:40] < 1408) & (v[1:40] >= 0) & (v[1:40] < 376)).any()


def test_borderline_shares_of_the_reference_stay_under_the_caps():
    """The GPU tests may leave out at most 0.1 % of the non-empty pixels at 1e-9 px (points entry) and 2 % at 1e-3 px (range-image entry):
    asserted here for the reference alone, so that the caps are known to be met before any device arithmetic enters."""
    fx = O.fixture()
    H, W = int(fx["H"]), int(fx["W"])
    for f in range(2):
        uvz = O.project(O.fixture_cloud(fx, f), fx["lidar2cam"][f], fx["K"])
        filled = O.fixture_image(fx, f"f{f}") != 0
        for eps, cap in ((1e-9, 0.001), (1e-3, 0.02)):
            mask, n_close = O.borderline_pixels(uvz, eps, H, W)
            share = (mask & filled).sum() / filled.sum()
            print(f"frame {f}: eps {eps:g}: {n_close} points, {int((mask & filled).sum())} of {int(filled.sum())} non-empty pixels = {share:.4%}")
            assert share <= cap
        assert O.borderline_pixels(uvz, 1e-9, H, W)[1] == 0  # the fixture has none at 1e-9 px


class _Stub(torch.nn.Module):
    num_frames = 4

    def __init__(self, image, depth):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(1))
        self.image, self.depth = image, depth

    def get_params(self, lr):
        return [{"params": [self.w], "lr": lr}]

    def render(self, o, d, t, **kw):
        return {"image": self.image * self.w, "depth": self.depth}


@pytest.mark.parametrize("criterion", O.CRITERIA)
def test_host_branch_equals_the_reference_formulation(criterion):
    from nvsf.nerf.train_step import RenderTrainStep
    scale, alpha_rd, n = 0.0108, 0.7, 512
    image, gt_rgb, depth, gt_m = O.loss_rays(n, scale, seed=3, dtype=torch.float64)
    depth.requires_grad_()
    step = RenderTrainStep(_Stub(image, depth), scale=scale, ema_decay=None, fp16=False, use_rgbd_loss=True, rgb_depth_loss=criterion,
                           alpha_rd=alpha_rd)
    batch = {"rays_o": torch.zeros(1, n, 3), "rays_d": torch.zeros(1, n, 3), "gt_rgb": gt_rgb, "gt_rgb_depth": gt_m, "time": torch.tensor([[0.5]])}
    total, parts = step.losses(batch)
    assert set(parts) == {"rgb", "rgb_depth"}
    (g_host,) = torch.autograd.grad(parts["rgb_depth"], depth)
    ref_depth = depth.detach().clone().requires_grad_()
    ref = O.reference_depth_terms(ref_depth, gt_m.unsqueeze(-1), scale, criterion, alpha_rd).sum()
    (g_ref,) = torch.autograd.grad(ref, ref_depth)
    assert float(parts["rgb_depth"].detach()) == pytest.approx(float(ref.detach()), rel=1e-13)
    torch.testing.assert_close(g_host, g_ref, rtol=1e-13, atol=0.0)
    capped = depth.detach() > 80 * scale
    masked = gt_m == 0
    assert capped.any() and masked.float().mean() > 0.8 and (gt_m > 80).any()
    assert bool((g_host[capped | masked] == 0).all()) and bool((g_host[~(capped | masked)] != 0).any())
    assert float(parts["rgb"]) == pytest.approx(float(((image - gt_rgb) ** 2).sum()), rel=1e-13)
    if criterion == "bce":  # taken literally: every masked ray adds log 2
        inside = ~masked
        part = O.reference_depth_terms(depth.detach(), gt_m.unsqueeze(-1), scale, criterion, alpha_rd)
        assert float(part[masked].sum()) == pytest.approx(alpha_rd * float(masked.sum()) * np.log(2.0), rel=1e-12) and bool(inside.any())


def test_switches_default_off_and_reject_what_the_reference_cannot_run():
    from nvsf.nerf.train_step import RenderTrainStep
    n = 16
    image, gt_rgb, depth, gt_m = O.loss_rays(n, 0.01, seed=4)
    batch = {"rays_o": torch.zeros(1, n, 3), "rays_d": torch.zeros(1, n, 3), "gt_rgb": gt_rgb, "time": torch.tensor([[0.5]])}
    off = RenderTrainStep(_Stub(image, depth), scale=0.01, ema_decay=None, fp16=False)
    assert off.use_rgbd_loss is False and set(off.losses(dict(batch, gt_rgb_depth=gt_m))[1]) == {"rgb"}
    on = RenderTrainStep(_Stub(image, depth), scale=0.01, ema_decay=None, fp16=False, use_rgbd_loss=True)
    assert on.rgb_depth_loss == "l1" and on.alpha_rd == 1.0
    with pytest.raises(ValueError, match="gt_rgb_depth"):
        on.losses(batch)
    for bad in ("cos", "nope"):
        with pytest.raises(ValueError):
            RenderTrainStep(_Stub(image, depth), scale=0.01, ema_decay=None, fp16=False, use_rgbd_loss=True, rgb_depth_loss=bad)


def test_device_tensors_only():
    from nvsf import _hip
    from nvsf.nerf.dataset import depth_image as D
    K = np.eye(3)
    with pytest.raises(_hip.NvsfHipError):
        D.points_depth_image(torch.zeros(4, 3), np.eye(4), K, 8, 8)
    with pytest.raises(_hip.NvsfHipError):
        D.lidar_depth_images(torch.zeros(1, 4, 8), torch.eye(4)[None], torch.eye(4)[None], K, 8, 8, (2.0, 26.9))
    with pytest.raises(TypeError):
        D.points_depth_image(np.zeros((4, 3), np.float32), np.eye(4), K, 8, 8)
    with pytest.raises(ValueError):
        D._intrinsics(np.arange(9.0), "test")  # a flat K
