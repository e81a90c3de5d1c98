"""GPU tests of the LiDAR-projected camera depth maps (csrc/projection.hip), the fused camera loss (csrc/losses.hip) and what is built
on them: FrameSet(camera_depth=True), RenderTrainStep(use_rgbd_loss=True), evaluate_frames' rgb_depth_rmse.

Bounds.  nvsf_points_depth_image and the fixture both work in fp64 from the same fp32 cloud: every pixel is bit-equal, except those that
hold or border a point within 1e-9 px of a pixel boundary (at most 0.1 % of the non-empty pixels; the fixture has none).
nvsf_lidar_depth_images forms the cloud itself, and the device's fp32 cos / sin may differ from numpy's by an ulp: that moves u by up to
about 6e-8 x 1408 x a few roundings ~ 3e-4 px, so pixels that hold or could receive a point within 1e-3 px of a boundary are left out (at
most 2 % of the non-empty pixels; the reference alone is at 0.3-0.4 %, test_depth_image_cpu.py), all others match in occupancy and to 1e-6
relative in value (about 8 fp32 roundings of 6e-8).  Camera loss: values to 1e-6 relative against fp64 autograd (fp64 sums of fp32
terms), gradients to 2e-6 ABSOLUTE per ray and per image element (the gradients are O(1): at most 2.7 for the image, 0.5 for the depth
with the upstream factors used, so a few fp32 roundings leave about 5e-7), exactly 0 at capped and masked rays."""
import ctypes
import os

import numpy as np
import pytest
import torch

import depth_image_oracle as O

pytestmark = pytest.mark.gpu


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def test_points_entry_is_bit_equal_to_the_reference(dev):
    from nvsf.nerf.dataset import depth_image as D
    fx = O.fixture()
    H, W = int(fx["H"]), int(fx["W"])
    for f in range(2):
        pc = O.fixture_cloud(fx, f)
        got = D.points_depth_image(_dev(pc, dev), fx["lidar2cam"][f], fx["K"], H, W).cpu().numpy()
        want = O.fixture_image(fx, f"f{f}")
        skip, n_close = O.borderline_pixels(O.project(pc, fx["lidar2cam"][f], fx["K"]), 1e-9, H, W)
        filled = want != 0
        share = (skip & filled).sum() / filled.sum()
        differ = got.view(np.uint32) != want.view(np.uint32)
        print(f"frame {f}: {int(filled.sum())} non-empty pixels, {n_close} points within 1e-9 px, excepted share {share:.4%}, "
              f"{int(differ.sum())} pixels differ ({int((differ & ~skip).sum())} outside the exception)")
        assert share <= 0.001
        assert not (differ & ~skip).any()


def test_point_list_behind_the_camera_and_on_the_bounds(dev):
    from nvsf.nerf.dataset import depth_image as D
    fx = O.fixture()
    H, W = int(fx["H"]), int(fx["W"])
    got = D.points_depth_image(_dev(fx["list_points"], dev), fx["list_lidar2cam"], fx["list_K"], H, W).cpu().numpy()
    want = O.fixture_image(fx, "list")
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got[188, 0] == 4.0 and got[0, 704] == 4.0 and got[0, 0] == 8.0 and got[195, 390] == np.float32(1e-5)
    assert np.count_nonzero(got) == fx["list_img_idx"].size
    empty = D.points_depth_image(torch.zeros(0, 3, device=dev), fx["list_lidar2cam"], fx["list_K"], H, W)
    assert empty.shape == (H, W) and not bool(empty.any())


def _lidar_images(fx, dev, ranges=None, frames=(0, 1)):
    from nvsf.nerf.dataset import depth_image as D
    sel = list(frames)
    r = fx["range_m"][sel] if ranges is None else ranges
    return D.lidar_depth_images(_dev(r, dev), _dev(fx["poses"][sel], dev), _dev(fx["poses_lidar"][sel], dev), fx["K"], int(fx["H"]), int(fx["W"]),
                                tuple(fx["fov"]), tuple(fx["fov_hoz"]))


def test_range_image_entry_against_the_reference(dev):
    fx = O.fixture()
    H, W = int(fx["H"]), int(fx["W"])
    got = _lidar_images(fx, dev).cpu().numpy()
    assert got.shape == (2, H, W) and got.dtype == np.float32
    for f in range(2):
        want = O.fixture_image(fx, f"f{f}")
        skip, n_close = O.borderline_pixels(O.project(O.fixture_cloud(fx, f), fx["lidar2cam"][f], fx["K"]), 1e-3, H, W)
        filled = want != 0
        share = (skip & filled).sum() / filled.sum()
        keep = ~skip
        occ = ((got[f] != 0) != filled) & keep
        both = filled & (got[f] != 0) & keep
        rel = np.abs(got[f][both].astype(np.float64) - want[both]) / want[both]
        print(f"frame {f}: {int(filled.sum())} non-empty pixels, {n_close} points within 1e-3 px, left out {share:.4%}; occupancy differs at "
              f"{int(occ.sum())} kept pixels; worst relative value error {rel.max():.3e}; bit-equal pixels {int((got[f].view(np.uint32) == want.view(np.uint32)).sum())} of {H * W}")
        assert share <= 0.02
        assert not occ.any()
        assert rel.max() <= 1e-6


def test_batch_equals_single_calls_and_two_runs_are_bit_equal(dev):
    fx = O.fixture()
    both = _lidar_images(fx, dev)
    again = _lidar_images(fx, dev)
    assert np.array_equal(_bits(both), _bits(again))
    for f in range(2):
        assert np.array_equal(_bits(_lidar_images(fx, dev, frames=(f,))[0]), _bits(both[f]))
    from nvsf.nerf.dataset import depth_image as D
    pc = _dev(O.fixture_cloud(fx, 1), dev)
    a = D.points_depth_image(pc, fx["lidar2cam"][1], fx["K"], int(fx["H"]), int(fx["W"]))
    b = D.points_depth_image(pc.flip(0).contiguous(), fx["lidar2cam"][1], fx["K"], int(fx["H"]), int(fx["W"]))  # another arrival order
    assert np.array_equal(_bits(a), _bits(b))


def test_empty_and_non_finite_ranges_produce_no_pixel(dev):
    fx = O.fixture()
    zero = _lidar_images(fx, dev, ranges=np.zeros_like(fx["range_m"]))
    assert not bool(zero.any())
    r = fx["range_m"].copy()
    hit = np.argwhere(r[0] != 0)
    rows = hit[np.random.default_rng(0).permutation(len(hit))[:900]]
    dropped = r.copy()
    for k, bad in enumerate((np.nan, np.inf, -np.inf)):
        sel = rows[300 * k:300 * (k + 1)]
        r[0, sel[:, 0], sel[:, 1]] = bad
        dropped[0, sel[:, 0], sel[:, 1]] = 0.0
    got, want = _lidar_images(fx, dev, ranges=r), _lidar_images(fx, dev, ranges=dropped)
    assert np.array_equal(_bits(got), _bits(want)) and bool(torch.isfinite(got).all())
    assert int((want[0] != 0).sum()) < int((_lidar_images(fx, dev, frames=(0,))[0] != 0).sum())  # the 900 pixels did matter


def test_invalid_arguments_leave_the_output_untouched(dev, hip_lib):
    fx = O.fixture()
    H, W, Hl, Wl = 16, 24, 66, 1030
    r = _dev(fx["range_m"], dev)
    l2c = _dev(fx["lidar2cam"].reshape(2, 16), dev)
    K = (ctypes.c_double * 9)(*fx["K"].reshape(-1))
    m = (ctypes.c_float * 16)(*fx["lidar2cam"][0].reshape(-1))
    pts = _dev(fx["list_points"], dev)
    out = torch.full((2, H, W), -7.0, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    P = lambda x: x.data_ptr()

    def images(F=2, Hl=Hl, Wl=Wl, fov_up=2.0, fov=26.9, fov_hoz=360.0, r_=P(r), l_=P(l2c), K_=K, H=H, W=W, out_=P(out)):
        return hip_lib.nvsf_lidar_depth_images(r_, F, Hl, Wl, fov_up, fov, fov_hoz, l_, K_, H, W, out_, stream)

    def points(p_=P(pts), n=200, m_=m, K_=K, H=H, W=W, out_=P(out)):
        return hip_lib.nvsf_points_depth_image(p_, n, m_, K_, H, W, out_, stream)
    assert images(F=0) == -1 and images(H=0) == -1 and images(W=0) == -1 and images(Hl=0) == -1 and images(Wl=0) == -1
    assert images(r_=None) == -1 and images(l_=None) == -1 and images(K_=None) == -1 and images(out_=None) == -1
    assert images(fov=0.0) == -1 and images(fov=-26.9) == -1 and images(fov_hoz=0.0) == -1 and images(fov=float("nan")) == -1
    assert points(H=0) == -1 and points(W=0) == -1 and points(p_=None) == -1 and points(m_=None) == -1 and points(K_=None) == -1
    assert points(out_=None) == -1
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())  # nothing ran
    assert images() == 0 and points() == 0
    torch.cuda.synchronize()
    assert bool((out[1] >= 0).all()) and bool((out[0] >= 0).all())
    a = torch.rand(8, 3, device=dev)
    l = torch.full((2,), -7.0, device=dev)
    g = torch.full((8, 4), -7.0, device=dev)

    def loss(n=8, crit=0, param=0.0, img=P(a), lr=P(l), ld=P(l) + 4):
        return hip_lib.nvsf_camera_loss_fwd(img, P(a), P(a), P(a), n, 1.0, 1.0, 0.01, 0.8, crit, param, lr, ld, stream)

    def back(n=8, crit=0, param=0.0, gi=P(g), gd=P(g) + 96):
        return hip_lib.nvsf_camera_loss_bwd(P(a), P(a), P(a), P(a), n, 1.0, 1.0, 0.01, 0.8, crit, param, lr_one, lr_one, gi, gd, stream)
    one = torch.ones(1, device=dev)
    lr_one = P(one)
    assert loss(crit=5) == -1 and loss(crit=-1) == -1 and loss(crit=2) == -1 and loss(crit=3, param=0.0) == -1  # Huber / SmoothL1 need a parameter
    assert loss(img=None) == -1 and loss(lr=None) == -1 and loss(ld=None) == -1
    assert back(crit=5) == -1 and back(gi=None) == -1 and back(gd=None) == -1 and back(crit=2) == -1
    torch.cuda.synchronize()
    assert bool((l == -7.0).all()) and bool((g == -7.0).all())


def test_wide_error_stats_take_fp64_differences(dev, hip_lib):
    """nvsf_image_error_stats_wide against nvsf_image_error_stats on a pair whose fp32 differences round: the wide sums equal the
    float64 numpy sums of exact differences to 1e-13, the narrow ones those of the fp32-rounded differences, and the two differ."""
    from nvsf.nerf import meters as M
    rng = np.random.default_rng(5)
    t = (rng.random(50000) * 80).astype(np.float32)
    p = (rng.random(50000) * 80).astype(np.float32)  # unrelated magnitudes: t - p needs more than 24 bits (close pairs subtract exactly)
    pd, td = _dev(p, dev), _dev(t, dev)
    wide, narrow = M.image_error_stats(pd, td, wide=True).cpu().numpy(), M.image_error_stats(pd, td).cpu().numpy()
    d64, d32 = t.astype(np.float64) - p.astype(np.float64), (t - p).astype(np.float64)
    np.testing.assert_allclose(wide[:2], [np.sum(d64 * d64), np.sum(np.abs(d64))], rtol=1e-13)
    np.testing.assert_allclose(narrow[:2], [np.sum(d32 * d32), np.sum(np.abs(d32))], rtol=1e-13)
    assert wide[0] != narrow[0] and np.array_equal(wide[2:], narrow[2:])
    capped = M.image_error_stats(pd, td, hi=40.0, wide=True).cpu().numpy()
    c64 = np.minimum(t, 40.0).astype(np.float64) - np.minimum(p, 40.0).astype(np.float64)
    np.testing.assert_allclose(capped[0], np.sum(c64 * c64), rtol=1e-13)
    ws = torch.full((4096,), -7.0, dtype=torch.float64, device=dev)
    out = torch.full((8,), -7.0, dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    P = lambda x: x.data_ptr()
    n = p.size
    f = hip_lib.nvsf_image_error_stats_wide
    assert f(P(pd), P(td), 0, 0.0, 1.0, P(ws), 4096, P(out), stream) == -1
    assert f(P(pd), P(td), n, 1.0, 0.0, P(ws), 4096, P(out), stream) == -1
    assert f(P(pd), P(td), n, 0.0, 1.0, P(ws), M.stats_ws_bytes(n) - 1, P(out), stream) == -1
    assert f(None, P(td), n, 0.0, 1.0, P(ws), 4096, P(out), stream) == -1 and f(P(pd), P(td), n, 0.0, 1.0, P(ws), 4096, None, stream) == -1
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((ws == -7.0).all())


@pytest.mark.parametrize("criterion", O.CRITERIA)
def test_camera_loss_against_fp64_autograd(dev, criterion):
    from nvsf.nerf.losses import CameraLossFn
    scale, alpha_rgb, alpha_rd, n = 0.0108, 0.9, 0.7, 4096
    image, gt_rgb, depth, gt_m = (t.to(dev) for t in O.loss_rays(n, scale, seed=11))
    image.requires_grad_()
    depth.requires_grad_()
    l_rgb, l_d = CameraLossFn.apply(image, depth, gt_rgb, gt_m, alpha_rgb, alpha_rd, scale, criterion)
    (l_rgb * 1.5 + l_d * 0.5).backward()
    i64, d64 = image.detach().double().cpu().requires_grad_(), depth.detach().double().cpu().requires_grad_()
    r_rgb = (alpha_rgb * (i64 - gt_rgb.double().cpu()) ** 2).sum()
    r_d = O.reference_depth_terms(d64, gt_m.double().cpu().unsqueeze(-1), scale, criterion, alpha_rd).sum()
    (r_rgb * 1.5 + r_d * 0.5).backward()
    rel = lambda a, b: abs(float(a) - float(b)) / abs(float(b))
    gd, gi = depth.grad.double().cpu(), image.grad.double().cpu()
    err_d, err_i = (gd - d64.grad).abs().max(), (gi - i64.grad).abs().max()
    print(f"{criterion}: rgb {float(l_rgb):.6f} (rel {rel(l_rgb, r_rgb):.2e}), depth {float(l_d):.6f} (rel {rel(l_d, r_d):.2e}), "
          f"worst absolute gradient error: depth {float(err_d):.2e}, image {float(err_i):.2e}")
    assert rel(l_rgb, r_rgb) <= 1e-6 and rel(l_d, r_d) <= 1e-6
    torch.testing.assert_close(gd, d64.grad, rtol=0.0, atol=2e-6)
    torch.testing.assert_close(gi, i64.grad, rtol=0.0, atol=2e-6)
    capped = (depth.detach() > 80 * scale).cpu()
    masked = (gt_m == 0).cpu()
    assert capped.any() and 0.8 < float(masked.float().mean()) < 0.9 and bool((gt_m > 80).any())
    assert bool((gd[capped | masked] == 0).all()) and bool((gd[~(capped | masked)] != 0).all())
    again = CameraLossFn.apply(image.detach(), depth.detach(), gt_rgb, gt_m, alpha_rgb, alpha_rd, scale, criterion)
    assert float(again[0]) == float(l_rgb) and float(again[1]) == float(l_d)  # fixed-order fp64 fold: the same bits
    with pytest.raises(ValueError):
        CameraLossFn.apply(image, depth, gt_rgb, gt_m, alpha_rgb, alpha_rd, scale, "cos")


def _street_dataset(root, n_frames=2, H=48, W=64, Hl=16, Wl=128, seed=0):
    """A small data set in the reference's formats whose camera looks along the LiDAR's +x, so that the range image does project into it."""
    from nvsf.nerf.dataset import formats as F
    rng = np.random.default_rng(seed)
    seq = "1908"
    d = os.path.join(root, "train", seq)
    os.makedirs(d, exist_ok=True)
    l2c = np.eye(4)
    l2c[:3, :3] = [[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]]
    l2c[:3, 3] = [0.02, -0.1, -0.3]
    frames, pcs = [], []
    for i in range(n_frames):
        l2w = np.eye(4)
        l2w[:3, 3] = [0.3 * i, 0.1, 0.0]
        pose = l2w @ np.linalg.inv(l2c)
        pc = np.zeros((Hl, Wl, 3), np.float32)
        pc[..., 1] = rng.random((Hl, Wl))
        pc[..., 2] = rng.uniform(3.0, 95.0, (Hl, Wl))  # some beyond the 80 m cap
        pc[rng.random((Hl, Wl)) < 0.3, 2] = 0.0
        np.save(os.path.join(d, f"img_{i:04d}.npy"), rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8))
        np.save(os.path.join(d, f"pano_{i:04d}.npy"), pc)
        frames.append({"frame_id": 1908 + i, "file_path": f"train/{seq}/img_{i:04d}.npy", "transform_matrix": pose,
                       "lidar_file_path": f"train/{seq}/pano_{i:04d}.npy", "lidar2world": l2w})
        pcs.append(pc)
    K = np.array([[40.0, 0, 32.0], [0, 40.0, 24.0], [0, 0, 1]])
    F.write_transforms(F.transforms_path(root, seq, "train"), w=W, h=H, w_lidar=Wl, h_lidar=Hl, K=K, frame_start=1908, frame_end=1908 + max(n_frames - 1, 1),
                       num_frames=n_frames, frames=frames)
    return seq, pcs, K


def _model(dev, seed=1):
    from nvsf.nerf.models.network_static import NeRFNetworkStatic
    torch.manual_seed(seed)
    m = NeRFNetworkStatic(bound=2.0, min_near=0.01, min_near_lidar=0.01, lidar_max_depth=0.9).to(dev)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1 and p.numel() > 10000:
                p.normal_(0, 0.3)
    return m


def test_frame_set_carries_the_depth_maps(dev, tmp_path):
    from nvsf.nerf.dataset import formats as F
    seq, pcs, K = _street_dataset(str(tmp_path))
    scale = 0.0108
    plain = F.FrameSet(str(tmp_path), seq, "train", scale, num_rays=256, num_rays_lidar=256, device=dev)
    assert plain.image_depths is None and "image_depths" not in plain.collate([0]) and "gt_rgb_depth" not in plain.train_batch([0])
    fs = F.FrameSet(str(tmp_path), seq, "train", scale, num_rays=256, num_rays_lidar=256, device=dev, camera_depth=True)
    assert fs.image_depths.shape == (2, 48, 64) and fs.image_depths.dtype == torch.float32
    maps = fs.image_depths.cpu().numpy()
    t = F.load_transforms(F.transforms_path(str(tmp_path), seq, "train"))
    for f in range(2):  # metres, as the reference stores them: the numpy restatement from the frame's files, bounds of the range-image test
        l2c = np.linalg.inv(t["poses"][f]) @ t["poses_lidar"][f]
        assert l2c.dtype == np.float32
        uvz = O.project(O.range_cloud(pcs[f][:, :, 2], (2.0, 26.9), (180.0, 360.0)), l2c, K)
        want = O.zbuffer(uvz, 48, 64)
        skip = O.borderline_pixels(uvz, 1e-3, 48, 64)[0]
        filled = want != 0
        assert (skip & filled).sum() <= 0.02 * filled.sum()
        assert not (((maps[f] != 0) != filled) & ~skip).any()
        both = filled & ~skip
        assert (np.abs(maps[f][both].astype(np.float64) - want[both]) / want[both]).max() <= 1e-6
        assert 100 < filled.sum() < 48 * 64 and (maps[f] > 80).any()
    c = fs.collate([1])
    assert c["image_depths"].shape == (1, 256, 1)
    assert torch.equal(c["image_depths"][0, :, 0], fs.image_depths[1].reshape(-1)[c["rays_rgb_inds"][0]])
    b = fs.train_batch([0])
    assert b["gt_rgb_depth"].shape == (1, 256)
    whole = F.FrameSet(str(tmp_path), seq, "train", scale, device=dev, training=False, camera_depth=True)
    assert torch.equal(whole.collate([1])["image_depths"], fs.image_depths[1:2])


def test_train_step_with_and_without_the_depth_term(dev, tmp_path):
    from nvsf.nerf.dataset import formats as F
    from nvsf.nerf.train_step import RenderTrainStep
    seq, pcs, K = _street_dataset(str(tmp_path))
    scale, alpha_rd = 0.0108, 0.6
    fs = F.FrameSet(str(tmp_path), seq, "train", scale, num_rays=512, num_rays_lidar=512, device=dev, camera_depth=True)
    torch.manual_seed(3)
    batch = fs.train_batch([1])
    assert float((batch["gt_rgb_depth"] > 0).float().mean()) > 0.02

    def run(**kw):
        m = _model(dev)
        step = RenderTrainStep(m, num_steps=48, scale=scale, ema_decay=None, **kw)
        seen = {}
        real = m.render

        def render(o, d, t, **k):
            r = real(o, d, t, **k)
            if not k.get("cal_lidar_color"):
                seen["depth"] = r["depth"].detach().clone()
            return r
        m.render = render
        torch.manual_seed(7)  # the jitter of perturb=True
        loss, parts, _ = step.step(batch)
        torch.cuda.synchronize()
        return loss, parts, seen["depth"]
    base_loss, base, _ = run()
    off_loss, off, _ = run(use_rgbd_loss=False, rgb_depth_loss="mse", alpha_rd=alpha_rd)
    assert set(off) == set(base) and "rgb_depth" not in off
    for k in base:
        assert np.array_equal(_bits(off[k].reshape(1)), _bits(base[k].reshape(1))), k
    assert np.array_equal(_bits(off_loss.reshape(1)), _bits(base_loss.reshape(1)))
    for criterion in ("l1", "huber"):
        loss, parts, depth = run(use_rgbd_loss=True, rgb_depth_loss=criterion, alpha_rd=alpha_rd)
        assert set(parts) == set(base) | {"rgb_depth"}
        want = O.reference_depth_terms(depth.double().cpu(), batch["gt_rgb_depth"].double().cpu().unsqueeze(-1), scale, criterion, alpha_rd).sum()
        print(f"{criterion}: rgb_depth {float(parts['rgb_depth']):.6f}, formulation on the render's own depth {float(want):.6f}")
        assert float(want) > 0 and float(parts["rgb_depth"]) == pytest.approx(float(want), rel=1e-6)
        assert float(parts["rgb"]) == pytest.approx(float(base["rgb"]), rel=1e-6)  # the fused entry's fp64 sum against MseSumFn's fp32 tree
        for k in ("depth", "raydrop", "intensity"):
            assert np.array_equal(_bits(parts[k].reshape(1)), _bits(base[k].reshape(1))), k
    with pytest.raises(ValueError, match="gt_rgb_depth"):
        RenderTrainStep(_model(dev), num_steps=48, scale=scale, ema_decay=None, use_rgbd_loss=True).losses(
            {k: v for k, v in batch.items() if k != "gt_rgb_depth"})


def test_evaluate_frames_reports_the_camera_depth_rmse(dev, tmp_path):
    from nvsf.nerf.dataset import formats as F
    from nvsf.nerf.evaluate import eval_step, evaluate_frames
    from nvsf.nerf import meters as M
    seq, pcs, K = _street_dataset(str(tmp_path))
    scale = 0.0108
    m = _model(dev)
    plain = F.FrameSet(str(tmp_path), seq, "train", scale, device=dev, training=False)
    fe = F.FrameSet(str(tmp_path), seq, "train", scale, device=dev, training=False, camera_depth=True)
    old = evaluate_frames(m, plain, 48, meters="table")
    assert set(old) == {"loss", "psnr", "depth_rmse_m", "chamfer_distance", "f_score", "frames", "depth", "intensity", "raydrop", "rgb_ssim", "rgb_rmse"}
    assert "gt_rgb_depth" not in eval_step(m, plain.collate([0]), 48)
    assert set(evaluate_frames(m, fe, 48)) == {"loss", "psnr", "depth_rmse_m", "chamfer_distance", "f_score", "frames"}
    res = evaluate_frames(m, fe, 48, meters="table")
    assert set(res) == set(old) | {"rgb_depth_rmse"}
    for k in old:
        np.testing.assert_array_equal(np.asarray(res[k], np.float64), np.asarray(old[k], np.float64), err_msg=k)
    want = []
    for i in range(2):  # the formula of error_matrices.py:90-100 on eval_step's tensors
        e = eval_step(m, fe.collate([i]), 48)
        assert e["gt_rgb_depth"].shape == e["pred_rgb_depth"].shape == (1, 48, 64)
        want.append(O.camera_depth_rmse((e["pred_rgb_depth"] / scale).cpu().numpy(), e["gt_rgb_depth"].cpu().numpy()))
    print(f"rgb_depth_rmse {res['rgb_depth_rmse']!r}, numpy {np.mean(want)!r}")
    assert np.isfinite(res["rgb_depth_rmse"]) and res["rgb_depth_rmse"] > 0
    np.testing.assert_allclose(res["rgb_depth_rmse"], np.mean(want), rtol=1e-12, atol=0)
    by_frames = evaluate_frames(m, fe, 48, meters="table", shard="frames")
    np.testing.assert_allclose(by_frames["rgb_depth_rmse"], res["rgb_depth_rmse"], rtol=1e-12, atol=0)
    lines = M.table_report(res)
    assert len(lines) == 8 and lines[-1].startswith("RMSE = ") and len(M.table_report(old)) == 7
