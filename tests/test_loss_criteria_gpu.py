"""GPU: the selectable criteria of the four per-ray loss terms (`--depth_loss`, `--raydrop_loss`, `--intensity_loss`, `--rgb_loss`,
main_nvsf.py:83-88, 205-222) in csrc/losses.hip against the torch.nn formulation of trainer.py:203-218 / :503 in fp64.
  * per-ray values and gradients: the project's bar for per-ray loss values (test_shipped_config_losses_gpu.py: rtol 2e-6, atol 1e-7);
  * the sums: twice the error the fp32 torch.nn expression makes on the CPU against the fp64 one on the same inputs (printed).
The weights, the label smoothing and Huber's delta are numbers fp32 holds exactly (1, 0.5, 0.25; 0.125; 0.2 x 1.25), so that the float
arguments of the C ABI are the numbers the fp64 formulation uses."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KINDS = ("l1", "mse", "huber", "smoothl1", "bce")
LIDAR_TERMS = ("depth_loss", "raydrop_loss", "intensity_loss")
DEFAULTS = {"depth_loss": "l1", "raydrop_loss": "mse", "intensity_loss": "mse", "rgb_loss": "mse"}
SIZES = (1, 63, 64, 65, 1025)  # around a wave and around the 1024 threads of the single workgroup
ALPHAS, ALPHA_RGB, SMOOTH, SCALE = (1.0, 0.5, 0.25), 0.5, 0.125, 1.25
RTOL, ATOL = 2e-6, 1e-7


def criterion(name, scale=SCALE):
    """main_nvsf.py:205-210."""
    return {"mse": torch.nn.MSELoss(reduction="none"), "l1": torch.nn.L1Loss(reduction="none"),
            "smoothl1": torch.nn.SmoothL1Loss(reduction="none", beta=0.1), "huber": torch.nn.HuberLoss(reduction="none", delta=0.2 * scale),
            "bce": torch.nn.BCEWithLogitsLoss(reduction="none")}[name]


@functools.lru_cache(maxsize=None)
def rays():
    """1025 LiDAR rays and colours (fp32, CPU); the sizes under test are its leading rows.  Row 0 an ordinary returning ray; row 1 a
    dropped ray (mask 0); row 2 exact zero residuals (the l1 derivative at 0); row 3 a range target of 3 under a prediction of 2 (BCE
    against a target above 1: a negative per-ray loss); the residuals of the rest lie on both sides of delta = 0.25 and beta = 0.1."""
    g = torch.Generator().manual_seed(11)
    n = max(SIZES)
    rnd = lambda *s: torch.rand(*s, generator=g)
    image = torch.stack([rnd(n) * 2 - 0.5, rnd(n)], -1)
    depth = rnd(n) * 1.5
    gt_rd = (rnd(n) > 0.3).float()
    gt_i = (image[:, 1] + (rnd(n) - 0.5) * 0.6).clamp(0, 1)
    gt_d = (depth + (rnd(n) - 0.5)).clamp(min=0)
    gt_rd[0], gt_rd[1], gt_rd[2], gt_rd[3] = 1.0, 0.0, 1.0, 1.0
    image[2, 0], image[2, 1], gt_d[2] = 1.0 - SMOOTH, gt_i[2], depth[2]
    depth[3], gt_d[3] = 2.0, 3.0
    rgb = rnd(n, 3)
    gt_rgb = (rgb + (rnd(n, 3) - 0.5) * 0.8).clamp(0, 1)
    gt_rgb[2] = rgb[2]
    return image, depth, gt_rd, gt_i, gt_d, rgb, gt_rgb


def lidar_reference(n, criteria, dtype):
    """trainer.py:187-218 -> (per-ray loss [n], the three sums, gradients with respect to image [n, 2] and depth [n] of their total)."""
    image, depth, gt_rd, gt_i, gt_d = (t[:n].to(dtype) for t in rays()[:5])
    image, depth = image.clone().requires_grad_(), depth.clone().requires_grad_()
    gt_intensity, gt_depth = gt_i * gt_rd, gt_d * gt_rd
    pred_raydrop, pred_intensity, pred_depth = image[:, 0], image[:, 1] * gt_rd, depth * gt_rd
    if criteria[1] == "bce":
        pred_raydrop = torch.sigmoid(pred_raydrop)
    terms = (ALPHAS[0] * criterion(criteria[0])(pred_depth, gt_depth), ALPHAS[1] * criterion(criteria[1])(pred_raydrop, gt_rd.clamp(SMOOTH, 1 - SMOOTH)),
             ALPHAS[2] * criterion(criteria[2])(pred_intensity, gt_intensity))
    sums = [t.sum() for t in terms]
    g_image, g_depth = torch.autograd.grad(sum(sums), (image, depth))
    return sum(terms).detach(), [s.detach() for s in sums], g_image, g_depth


def assert_sums(tag, got, ref64, ref32, names=("depth", "raydrop", "intensity")):
    for name, a, b64, b32 in zip(names, got, ref64, ref32):
        err32, err = abs(float(b32) - float(b64)), abs(float(a) - float(b64))
        print(f"{tag} sum {name}: {float(b64):.9e} err fp32-cpu {err32:.3e} kernel {err:.3e}")
        assert err <= 2 * err32, (tag, name)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("term", LIDAR_TERMS)
def test_lidar_terms_under_every_criterion(dev, term, kind):
    from nvsf import _hip
    from nvsf.nerf.losses import LidarCritLossFn, lidar_criteria_args
    criteria = tuple(kind if t == term else DEFAULTS[t] for t in LIDAR_TERMS)
    for n in SIZES:
        image, depth, gt_rd, gt_i, gt_d = (t[:n].contiguous().to(dev) for t in rays()[:5])
        image, depth = image.view(1, n, 2).requires_grad_(), depth.view(1, n).requires_grad_()
        out = LidarCritLossFn.apply(image, depth, gt_rd.view(1, n), gt_i.view(1, n), gt_d.view(1, n), None, *ALPHAS, SMOOTH, SCALE, criteria)
        g_image, g_depth = torch.autograd.grad(out[0] + out[1] + out[2], (image, depth))
        ray_loss, stats = torch.empty(n, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
        _hip.call("nvsf_lidar_ray_losses_crit", _hip.ptr(image.detach()), _hip.ptr(depth.detach()), _hip.ptr(gt_rd), _hip.ptr(gt_i), _hip.ptr(gt_d), n,
                  *ALPHAS, SMOOTH, *lidar_criteria_args(criteria, SCALE), _hip.ptr(ray_loss), _hip.ptr(stats))
        r_loss, r_sums, r_gi, r_gd = lidar_reference(n, criteria, torch.float64)
        _, r_sums32, _, _ = lidar_reference(n, criteria, torch.float32)
        np.testing.assert_allclose(ray_loss.cpu().numpy(), r_loss.numpy(), rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(g_image.cpu().view(n, 2).numpy(), r_gi.numpy(), rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(g_depth.cpu().view(n).numpy(), r_gd.numpy(), rtol=RTOL, atol=ATOL)
        assert torch.equal(out[3].cpu().view(n), (rays()[1][:n] * rays()[2][:n]))  # the masked range, as the default entry gives it
        lo, hi = stats.cpu().numpy().view(np.float32)
        assert lo == ray_loss.min().item() and hi == ray_loss.max().item()
        assert_sums(f"{term}={kind} N={n}", out[:3], r_sums, r_sums32)
        if n >= 4:
            assert float(g_depth[0, 1]) == 0.0 and float(g_image[0, 1, 1]) == 0.0       # the dropped ray
            if kind == "l1":
                assert float((g_depth if term == "depth_loss" else g_image[..., 0 if term == "raydrop_loss" else 1])[0, 2]) == 0.0  # residual 0
            if term == "depth_loss" and kind == "bce":
                assert float(ray_loss[3]) < 0 and lo < 0                                    # the negative per-ray loss reaches the statistics


@pytest.mark.parametrize("kind", KINDS)
def test_colour_term_under_every_criterion(dev, kind):
    from nvsf import _hip
    from nvsf.nerf.losses import CritSumFn, per_ray_criterion

    def reference(n, dtype):
        rgb, gt = (t[:n].to(dtype) for t in rays()[5:])
        rgb = rgb.clone().requires_grad_()
        term = ALPHA_RGB * criterion(kind)(rgb, gt)                                      # trainer.py:503
        (grad,) = torch.autograd.grad(term.sum(), rgb)
        return term.sum(dim=1).detach(), term.sum().detach(), grad                       # trainer.py:609: the error map's per-ray form
    code, param = per_ray_criterion("rgb_loss", kind, SCALE)
    for n in SIZES:
        rgb, gt = (t[:n].contiguous().to(dev) for t in rays()[5:])
        rgb = rgb.view(1, n, 3).requires_grad_()
        total = CritSumFn.apply(rgb, gt.view(1, n, 3), ALPHA_RGB, kind, SCALE)
        (grad,) = torch.autograd.grad(total, rgb)
        rows, stats = torch.empty(n, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
        _hip.call("nvsf_crit_rows", _hip.ptr(rgb.detach()), _hip.ptr(gt), n, 3, ALPHA_RGB, code, float(param), _hip.ptr(rows), _hip.ptr(stats))
        r_rows, r_sum, r_grad = reference(n, torch.float64)
        np.testing.assert_allclose(rows.cpu().numpy(), r_rows.numpy(), rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(grad.cpu().view(n, 3).numpy(), r_grad.numpy(), rtol=RTOL, atol=ATOL)
        lo, hi = stats.cpu().numpy().view(np.float32)
        assert lo == rows.min().item() and hi == rows.max().item()
        assert_sums(f"rgb_loss={kind} N={n}", [total], [r_sum], [reference(n, torch.float32)[1]], names=("rgb",))
        if n >= 4 and kind == "l1":
            assert not bool(grad[0, 2].any())


def _scene(dev, n=256, hashmap=12):
    from test_train_step_gpu import _batch
    from nvsf import synthetic as S
    from nvsf.nerf.models.network_static import NeRFNetworkStatic
    kw = dict(bound=S.BOUND, min_near=S.MIN_NEAR, min_near_lidar=S.MIN_NEAR, lidar_max_depth=S.LIDAR_MAX_DEPTH, log2_hashmap_size=hashmap)
    torch.manual_seed(1)
    teacher = NeRFNetworkStatic(**kw)
    with torch.no_grad():
        g = torch.Generator().manual_seed(7)
        for enc in (teacher.hash_encoder_lidar, teacher.hash_encoder_camera):
            enc.params.copy_(torch.randn(enc.params.shape, generator=g) * 0.2)
    teacher = teacher.to(dev).eval()
    return S, NeRFNetworkStatic(**kw).to(dev), _batch(S, teacher, dev, n=n)


def test_default_criteria_by_name_are_the_step_without_them(dev):
    """The no-behaviour-change check: the defaults spelled out go through the entries a step built without them uses -- the same bits."""
    from nvsf.nerf.train_step import RenderTrainStep
    S, student, batch = _scene(dev)
    parts = []
    for kw in ({}, dict(DEFAULTS)):
        step = RenderTrainStep(student, num_steps=48, scale=S.SCALE, ema_decay=None, use_urf_loss=False, **kw)
        assert step.lidar_criteria is None and step.rgb_criterion is None
        torch.manual_seed(5)
        total, p = step.losses(batch)
        assert type(p["depth"].grad_fn).__name__.startswith("LidarLossFn") and type(p["rgb"].grad_fn).__name__.startswith("MseSumFn")
        parts.append({k: v.detach().clone() for k, v in p.items()} | {"total": total.detach().clone()})
        step.sync()
    assert set(parts[0]) == set(parts[1]) and all(torch.equal(parts[0][k], parts[1][k]) for k in parts[0])


def test_rgb_criterion_with_the_camera_depth_term(dev):
    """rgb_loss = "huber" with use_rgbd_loss: both camera terms in one launch each way, the colour under Huber, the depth term as before."""
    import depth_image_oracle as O
    from nvsf.nerf.losses import CameraCritLossFn, CameraLossFn
    scale, alpha_rd, n = 1.25, 0.5, 1025
    image, gt_rgb, depth, gt_m = (t.to(dev) for t in O.loss_rays(n, scale, seed=11))
    image.requires_grad_()
    depth.requires_grad_()
    l_rgb, l_d = CameraCritLossFn.apply(image, depth, gt_rgb, gt_m, ALPHA_RGB, alpha_rd, scale, "l1", "huber")
    g_image, g_depth = torch.autograd.grad(l_rgb + l_d, (image, depth))
    refs = {}
    for dt in (torch.float64, torch.float32):
        i, d = image.detach().cpu().to(dt).requires_grad_(), depth.detach().cpu().to(dt).requires_grad_()
        r_rgb = (ALPHA_RGB * criterion("huber", scale)(i, gt_rgb.cpu().to(dt))).sum()
        r_d = O.reference_depth_terms(d, gt_m.cpu().to(dt).unsqueeze(-1), scale, "l1", alpha_rd).sum()
        refs[dt] = (r_rgb.detach(), r_d.detach()) + torch.autograd.grad(r_rgb + r_d, (i, d))
    r_rgb, r_d, r_gi, r_gd = refs[torch.float64]
    assert_sums("rgbd rgb_loss=huber", [l_rgb], [r_rgb], [refs[torch.float32][0]], names=("rgb",))
    assert abs(float(l_d) - float(r_d)) <= 1e-6 * abs(float(r_d))                        # the depth term's own bar (test_depth_image_gpu.py)
    np.testing.assert_allclose(g_image.cpu().numpy(), r_gi.numpy(), rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(g_depth.cpu().double(), r_gd, rtol=0.0, atol=2e-6)
    plain = CameraLossFn.apply(image.detach(), depth.detach(), gt_rgb, gt_m, ALPHA_RGB, alpha_rd, scale, "l1")
    assert float(plain[1]) == float(l_d) and float(plain[0]) != float(l_rgb)


class _Params(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(4))

    def get_params(self, lr):
        return [{"params": [self.w], "lr": lr}]


class _Frames:
    """What update_error_map reads of a FrameSet: one frame, a LiDAR error map as large as the range image."""

    def __init__(self, dev, H, W):
        self.error_map, self.error_map_rgb = torch.ones(1, H, W, device=dev), None
        self.H_lidar, self.W_lidar, self.H, self.W = H, W, 1, 1

    def error_map_stats(self, device):
        return torch.tensor([0x7f800000, 0], dtype=torch.int64).to(torch.int32).to(device)

    def error_map_owner(self, device, n_cells):
        return torch.zeros(n_cells, dtype=torch.int32, device=device)


@pytest.mark.parametrize("batch_kind", ["all_negative", "mixed"])
def test_error_map_normalisation_with_negative_losses(dev, batch_kind):
    """Through RenderTrainStep.update_error_maps with depth_loss = "bce": the map follows trainer.py:572-587 with the TRUE minimum and
    maximum of the per-ray losses, for a batch whose losses are all negative and for a mixed one."""
    from nvsf.nerf.train_step import RenderTrainStep
    n, H, W = 1025, 33, 64
    image, depth, gt_rd, gt_i, gt_d = (t.clone() for t in rays()[:5])
    if batch_kind == "all_negative":  # every ray returns, predictions of 2-3 under targets of 3-4: x - x t + log1p(exp(-x)) < 0
        gt_rd = torch.ones(n)
        depth, gt_d = 2.0 + depth / 1.5, 3.0 + gt_d.clamp(max=1.0)
    criteria = ("bce", "mse", "mse")
    step = RenderTrainStep(_Params().to(dev), scale=SCALE, ema_decay=None, smooth_factor=SMOOTH, alpha_d=ALPHAS[0], alpha_r=ALPHAS[1],
                           alpha_i=ALPHAS[2], depth_loss="bce")
    assert step.lidar_criteria == criteria
    frames = _Frames(dev, H, W)
    step.error_maps = frames
    step._for_error_map = {"lidar": tuple(t.to(dev) for t in (image.view(1, n, 2), depth.view(1, n), gt_rd.view(1, n), gt_i.view(1, n), gt_d.view(1, n)))}
    inds = torch.randperm(H * W, generator=torch.Generator().manual_seed(2))[:n]  # one ray per cell
    step.update_error_maps({"index": [0], "rays_pano_inds": inds.view(1, n).to(dev)})
    # trainer.py:213-218 and :572-587 in fp64
    d64 = lambda t: t.double()
    pd, gd = d64(depth) * d64(gt_rd), d64(gt_d) * d64(gt_rd)
    loss = (ALPHAS[0] * criterion("bce")(pd, gd) + ALPHAS[1] * (d64(image[:, 0]) - d64(gt_rd).clamp(SMOOTH, 1 - SMOOTH)) ** 2
            + ALPHAS[2] * (d64(image[:, 1]) * d64(gt_rd) - d64(gt_i) * d64(gt_rd)) ** 2)
    assert bool((loss < 0).all()) if batch_kind == "all_negative" else (bool((loss < 0).any()) and bool((loss > 0).any()))
    error = (loss - loss.min()) / (loss.max() - loss.min() + torch.finfo(torch.float32).eps) * (1e3 - 1) + 1
    expect = torch.ones(H * W, dtype=torch.float64)
    expect[inds] = 0.1 * 1.0 + 0.9 * error
    got = frames.error_map[0].cpu().double().view(-1)
    np.testing.assert_allclose(got.numpy(), expect.numpy(), rtol=3e-5, atol=1e-4)   # the bar of test_error_map_update_matches_the_restatement
    assert abs(float(got.min()) - 1.0) <= 1e-4 and abs(float(got.max()) - (0.1 + 0.9 * 1000.0)) <= 0.05


def test_step_with_non_default_criteria(dev):
    from nvsf.nerf.train_step import RenderTrainStep
    S, student, batch = _scene(dev)
    step = RenderTrainStep(student, lr=1e-2, iters=400, num_steps=48, scale=S.SCALE, depth_loss="huber", raydrop_loss="bce",
                           intensity_loss="smoothl1", rgb_loss="l1")
    from nvsf.nerf.loss_scaler import LossScaler
    step.scaler = LossScaler(init_scale=64.0, growth_interval=10 ** 6)  # a loss scale the first step does not overflow at
    loss, parts, _ = step.step(batch)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(v)) for v in parts.values())
    assert set(parts) == {"depth", "raydrop", "intensity", "chamfer", "rgb"}
    table = student.hash_encoder_lidar.params
    assert table.grad is not None and bool(torch.isfinite(table.grad).all()) and float(table.grad.abs().max()) > 0
    step.sync()
