"""CPU: the criterion switches of the four per-ray terms (`--depth_loss`, `--raydrop_loss`, `--intensity_loss`, `--rgb_loss`,
main_nvsf.py:83-88) on RenderTrainStep: what the constructor accepts and rejects, and the host branch of `losses()` against the torch.nn
criteria of main_nvsf.py:205-212 applied as trainer.py:203-218 and :503 write them, in fp64 on the same tensors."""
import pytest
import torch

OPTIONS = ("depth_loss", "raydrop_loss", "intensity_loss", "rgb_loss")
NAMES = ("l1", "mse", "huber", "smoothl1", "bce")
LINES = {"rgb_loss": 83, "depth_loss": 85, "intensity_loss": 87, "raydrop_loss": 88}


class _Stub(torch.nn.Module):
    num_frames = 4

    def __init__(self, outputs):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(1))
        self.outputs = outputs

    def get_params(self, lr):
        return [{"params": [self.w], "lr": lr}]

    def render(self, o, d, t, **kw):
        return self.outputs


def reference_criterion(name, scale):
    """main_nvsf.py:205-210, literally."""
    return {"mse": torch.nn.MSELoss(reduction="none"), "l1": torch.nn.L1Loss(reduction="none"),
            "smoothl1": torch.nn.SmoothL1Loss(reduction="none", beta=0.1), "huber": torch.nn.HuberLoss(reduction="none", delta=0.2 * scale),
            "bce": torch.nn.BCEWithLogitsLoss(reduction="none")}[name]


def _step(**kw):
    from nvsf.nerf.train_step import RenderTrainStep
    return RenderTrainStep(_Stub({}), ema_decay=None, fp16=False, **kw)


@pytest.mark.parametrize("option", OPTIONS)
def test_constructor_accepts_every_criterion_and_names_the_option_it_rejects(option):
    for name in NAMES:
        step = _step(**{option: name})
        assert step.criteria[option] == name
    for bad in ("cos", "l3"):  # CosineSimilarity over dim 1 of a [B, N] / [B, N, 3] pair is no per-ray loss
        with pytest.raises(ValueError, match=rf"{option}='{bad}'.*main_nvsf\.py:{LINES[option]}"):
            _step(**{option: bad})
    step = _step()
    assert step.criteria == {"depth_loss": "l1", "raydrop_loss": "mse", "intensity_loss": "mse", "rgb_loss": "mse"}
    assert step.lidar_criteria is None and step.rgb_criterion is None  # the defaults keep their own entries


def _lidar_case(n, seed, scale):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    image = rnd(1, n, 2) * 2 - 0.5
    depth = rnd(1, n) * 1.5                                   # range targets above 1 among them
    gt_rd = (rnd(1, n) > 0.3).double()
    gt_i, gt_d = rnd(1, n), depth + (rnd(1, n) - 0.5) * 8 * 0.2 * scale  # residuals on both sides of Huber's delta
    gt_d[0, :4] = depth[0, :4]                                # exact zero residuals
    return image, depth, gt_rd, gt_i, gt_d


@pytest.mark.parametrize("smooth", [0.0, 0.2])
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("option", OPTIONS[:3])
def test_host_lidar_terms_equal_the_reference_criteria(option, name, smooth):
    n, scale = 257, 0.7
    image, depth, gt_rd, gt_i, gt_d = _lidar_case(n, 5, scale)
    image.requires_grad_()
    depth.requires_grad_()
    from nvsf.nerf.train_step import RenderTrainStep
    step = RenderTrainStep(_Stub({"image_lidar": image, "depth_lidar": depth}), ema_decay=None, fp16=False, scale=scale, chamfer_loss=False,
                           smooth_factor=smooth, alpha_d=0.9, alpha_r=0.3, alpha_i=0.2, **{option: name})
    batch = {"rays_o_lidar": torch.zeros(1, n, 3), "rays_d_lidar": torch.zeros(1, n, 3), "gt_raydrop": gt_rd, "gt_intensity": gt_i,
             "gt_depth": gt_d, "time": torch.tensor([[0.5]])}
    total, parts = step.losses(batch)
    assert set(parts) == {"depth", "raydrop", "intensity"}
    # trainer.py:187-218
    crit = {k: reference_criterion(step.criteria[k], scale) for k in OPTIONS[:3]}
    ri, rd = image.detach().clone().requires_grad_(), depth.detach().clone().requires_grad_()
    pred_raydrop = ri[:, :, 0]
    pred_intensity = ri[:, :, 1] * gt_rd
    pred_depth = rd * gt_rd
    if step.criteria["raydrop_loss"] == "bce":
        pred_raydrop = torch.sigmoid(pred_raydrop)            # ... and BCEWithLogitsLoss applies its own: two sigmoids, as written
    ref = {"depth": (0.9 * crit["depth_loss"](pred_depth, gt_d * gt_rd)).sum(),
           "raydrop": (0.3 * crit["raydrop_loss"](pred_raydrop, gt_rd.clamp(smooth, 1 - smooth))).sum(),
           "intensity": (0.2 * crit["intensity_loss"](pred_intensity, gt_i * gt_rd)).sum()}
    for k in ref:
        assert float(parts[k].detach()) == pytest.approx(float(ref[k].detach()), rel=1e-13), k
    g_host = torch.autograd.grad(total, (image, depth))
    g_ref = torch.autograd.grad(sum(ref.values()), (ri, rd))
    for a, b in zip(g_host, g_ref):
        torch.testing.assert_close(a, b, rtol=1e-13, atol=1e-16)
    assert bool((g_host[1][gt_rd == 0] == 0).all()) and bool((gt_rd == 0).any())


@pytest.mark.parametrize("rgbd", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_host_colour_term_equals_the_reference_criterion(name, rgbd):
    n, scale = 129, 0.7
    g = torch.Generator().manual_seed(7)
    image = torch.rand(1, n, 3, generator=g, dtype=torch.float64).requires_grad_()
    gt_rgb = (image.detach() + (torch.rand(1, n, 3, generator=g, dtype=torch.float64) - 0.5) * 0.5).clamp(0, 1)
    depth, gt_m = torch.rand(1, n, generator=g, dtype=torch.float64), torch.rand(1, n, generator=g, dtype=torch.float64) * 50
    from nvsf.nerf.train_step import RenderTrainStep
    step = RenderTrainStep(_Stub({"image": image, "depth": depth}), ema_decay=None, fp16=False, scale=scale, alpha_rgb=0.6, rgb_loss=name,
                           use_rgbd_loss=rgbd)
    batch = {"rays_o": torch.zeros(1, n, 3), "rays_d": torch.zeros(1, n, 3), "gt_rgb": gt_rgb, "gt_rgb_depth": gt_m, "time": torch.tensor([[0.5]])}
    _, parts = step.losses(batch)
    assert set(parts) == ({"rgb", "rgb_depth"} if rgbd else {"rgb"})
    ref_image = image.detach().clone().requires_grad_()
    ref = (0.6 * reference_criterion(name, scale)(ref_image, gt_rgb)).sum()  # trainer.py:503, summed at :545-547
    assert float(parts["rgb"].detach()) == pytest.approx(float(ref.detach()), rel=1e-13)
    torch.testing.assert_close(torch.autograd.grad(parts["rgb"], image)[0], torch.autograd.grad(ref, ref_image)[0], rtol=1e-13, atol=1e-16)
