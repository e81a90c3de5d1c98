"""CPU: the distortion loss of mip-NeRF 360 as the step's host branch has it (`losses.distortion_loss`, the O(T) prefix-sum form)
against the O(T^2) definition of tests/distortion_oracle.py, both in float64; closed forms; degenerate rays; the switch on
RenderTrainStep (constructor check, parts of the default step, the host branch through `losses()`)."""
import pytest
import torch

import distortion_oracle as O

SHAPES = [(1, 1), (3, 2), (5, 65), (4, 832)]


def _host(w, z, nears, fars, alpha):
    """value and autograd gradient of losses.distortion_loss in float64"""
    from nvsf.nerf.losses import distortion_loss, distortion_ray_losses
    w = w.double().clone().requires_grad_()
    z, nears, fars = z.double(), nears.double(), fars.double()
    loss = distortion_loss(w, z, nears, fars, alpha)
    (grad,) = torch.autograd.grad(loss, w)
    return distortion_ray_losses(w.detach(), z, nears, fars), loss.detach(), grad


@pytest.mark.parametrize("kind", ["spread", "peaked", "ties"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_prefix_sum_form_equals_the_definition(shape, kind):
    c = O.case(shape[0], shape[1], kind)
    if kind == "ties" and shape[1] > 1:
        assert bool((c["z"][:, 1::2] == c["z"][:, 0:shape[1] - 1:2]).all())
    ray, loss, grad = _host(c["w"], c["z"], c["nears"], c["fars"], O.ALPHA)
    ref_ray, ref_loss, ref_grad = O.reference(shape[0], shape[1], kind)
    errs = (float((ray - ref_ray).abs().max()), abs(float(loss) - float(ref_loss)), float((grad - ref_grad).abs().max()))
    print(f"distortion host {shape[0]}x{shape[1]} {kind}: loss {float(ref_loss):.6e}, |ray err| {errs[0]:.2e}, |loss err| {errs[1]:.2e}, |grad err| {errs[2]:.2e}")
    assert float(ref_loss) > 0 and max(errs) <= 1e-13


def test_closed_forms():
    T, near, far = 9, 0.25, 2.25
    R = far - near
    z = torch.tensor([[0.3, 0.35, 0.6, 0.6, 0.9, 1.4, 1.5, 2.0, 2.2]], dtype=torch.float64)
    nears, fars = torch.tensor([near], dtype=torch.float64), torch.tensor([far], dtype=torch.float64)
    delta = torch.cat([z[0, 1:] - z[0, :-1], torch.tensor([R / T], dtype=torch.float64)])
    m, d = (z[0] + delta / 2 - near) / R, delta / R
    for i in (0, 3, 8):  # a one-hot row: w^2 d_i / 3 (i = 8: the last interval is R / T)
        w = torch.zeros(1, T, dtype=torch.float64)
        w[0, i] = 0.7
        ray, loss, grad = _host(w, z, nears, fars, 0.5)
        assert float(ray[0]) == pytest.approx(0.49 * float(d[i]) / 3, rel=1e-14, abs=1e-18)
        assert float(loss) == pytest.approx(0.5 * float(ray[0]), rel=1e-14)
        assert float(O.distortion(w, z, nears, fars, 0.5)[0][0]) == pytest.approx(float(ray[0]), rel=1e-14, abs=1e-18)
    for i, j in ((1, 6), (2, 3), (0, 8)):  # two spikes ((2, 3): equal depths, different midpoints)
        w = torch.zeros(1, T, dtype=torch.float64)
        w[0, i], w[0, j] = 0.3, 0.6
        want = 2 * 0.3 * 0.6 * abs(float(m[i] - m[j])) + (0.09 * float(d[i]) + 0.36 * float(d[j])) / 3
        ray, _, grad = _host(w, z, nears, fars, 1.0)
        assert float(ray[0]) == pytest.approx(want, rel=1e-14)
        # d ray / d w_k = 2 sum_j w_j |m_k - m_j| + 2/3 w_k d_k, also where w_k = 0
        k = 4
        assert float(grad[0, k]) == pytest.approx(2 * (0.3 * abs(float(m[k] - m[i])) + 0.6 * abs(float(m[k] - m[j]))), rel=1e-13)
        assert float(grad[0, i]) == pytest.approx(2 * 0.6 * abs(float(m[i] - m[j])) + 2 / 3 * 0.3 * float(d[i]), rel=1e-13)


def test_degenerate_rays_give_zero_and_no_gradient():
    c = O.case(5, 65, "degenerate")
    assert float(c["fars"][0]) == float(c["nears"][0]) and float(c["fars"][2]) < float(c["nears"][2]) and not bool(torch.isfinite(c["fars"][4]))
    ray, loss, grad = _host(c["w"], c["z"], c["nears"], c["fars"], O.ALPHA)
    ref_ray, ref_loss, ref_grad = O.reference(5, 65, "degenerate")
    for n in (0, 2, 4):
        assert float(ray[n]) == 0.0 and bool((grad[n] == 0).all())
    for n in (1, 3):
        assert float(ray[n]) > 0 and bool((grad[n] != 0).any())
    assert bool(torch.isfinite(grad).all()) and abs(float(loss) - float(ref_loss)) <= 1e-13 and float((grad - ref_grad).abs().max()) <= 1e-13
    assert float(loss) == pytest.approx(O.ALPHA * float(ray.sum()) / 5, rel=1e-14)  # the rays that give 0 count in N
    # every ray degenerate: 0, and a zero gradient
    w = torch.rand(2, 3, dtype=torch.float64).requires_grad_()
    from nvsf.nerf.losses import distortion_loss
    loss = distortion_loss(w, torch.rand(2, 3, dtype=torch.float64).sort(dim=1).values, torch.ones(2, dtype=torch.float64), torch.tensor([1.0, 0.5], dtype=torch.float64), 1.0)
    assert float(loss.detach()) == 0.0 and bool((torch.autograd.grad(loss, w)[0] == 0).all())


class _Stub(torch.nn.Module):
    """What RenderTrainStep needs of a model on the host branch: parameters, a render that returns fixed rows, the renderer's range."""
    num_frames = 4

    def __init__(self, outputs, nears, fars):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(1))
        self.outputs, self.range, self.aabb_train, self.aabb_infer = outputs, (nears, fars), "train", "infer"
        self.asked = []

    def get_params(self, lr):
        return [{"params": [self.w], "lr": lr}]

    def render(self, o, d, t, **kw):
        return self.outputs

    def _near_far(self, rays_o, rays_d, cal_lidar_color, aabb):
        self.asked.append((tuple(rays_o.shape), bool(cal_lidar_color), aabb))
        return self.range


def _step_case(n, T):
    c = O.case(n, T, "peaked")
    w = c["w"].double().clone().requires_grad_()
    outputs = {"image_lidar": torch.rand(1, n, 2, dtype=torch.float64), "depth_lidar": torch.rand(1, n, dtype=torch.float64),
               "image": torch.rand(1, n, 3, dtype=torch.float64), "depth": torch.rand(1, n, dtype=torch.float64), "weights": w,
               "z_vals": c["z"].double()}
    batch = {"rays_o_lidar": torch.zeros(1, n, 3), "rays_d_lidar": torch.zeros(1, n, 3), "gt_raydrop": torch.ones(1, n, dtype=torch.float64),
             "gt_intensity": torch.rand(1, n, dtype=torch.float64), "gt_depth": torch.rand(1, n, dtype=torch.float64),
             "rays_o": torch.zeros(1, n, 3), "rays_d": torch.zeros(1, n, 3), "gt_rgb": torch.rand(1, n, 3, dtype=torch.float64),
             "time": torch.tensor([[0.5]])}
    return c, w, _Stub(outputs, c["nears"].double(), c["fars"].double()), batch


def test_default_step_has_no_distortion_parts():
    from nvsf.nerf.train_step import RenderTrainStep
    _, _, model, batch = _step_case(5, 65)
    step = RenderTrainStep(model, ema_decay=None, fp16=False, chamfer_loss=False)
    assert step.distortion is False
    _, parts = step.losses(batch)
    assert set(parts) == {"depth", "raydrop", "intensity", "rgb"} and model.asked == []  # and the range is not asked for


def test_switch_adds_both_parts_on_the_host_branch():
    from nvsf.nerf.train_step import RenderTrainStep
    n, T = 5, 65
    c, w, model, batch = _step_case(n, T)
    step = RenderTrainStep(model, ema_decay=None, fp16=False, chamfer_loss=False, distortion_loss=True, alpha_dist=O.ALPHA)
    assert step.distortion is True and step.alpha_dist == O.ALPHA
    total, parts = step.losses(batch)
    assert set(parts) == {"depth", "raydrop", "intensity", "rgb", "dist_lidar", "dist"}
    assert model.asked == [((n, 3), True, "train"), ((n, 3), False, "train")]  # as `run` asks: flat rays, the training box
    _, ref_loss, ref_grad = O.reference(n, T, "peaked")
    for key in ("dist_lidar", "dist"):
        assert abs(float(parts[key].detach()) - float(ref_loss)) <= 1e-13
    (grad,) = torch.autograd.grad(total, w)
    assert float((grad - 2 * ref_grad).abs().max()) <= 1e-13  # both terms read the stub's one row set
    assert RenderTrainStep(model, ema_decay=None, fp16=False, distortion_loss=True).alpha_dist == 0.01


def test_constructor_refuses_the_occupancy_grid_path():
    from nvsf.nerf.models.network_static import NeRFNetworkStatic
    from nvsf.nerf.train_step import RenderTrainStep
    m = NeRFNetworkStatic(bound=2, log2_hashmap_size=8)
    assert RenderTrainStep(m, ema_decay=None, distortion_loss=True).distortion is True
    m.cuda_ray = True  # what enable_occupancy_grid() sets: run_cuda returns no [N, T] rows
    with pytest.raises(ValueError, match="occupancy-grid"):
        RenderTrainStep(m, ema_decay=None, distortion_loss=True)
    assert RenderTrainStep(m, ema_decay=None).distortion is False


def test_function_names_the_shapes_it_rejects():
    from nvsf.nerf.losses import DistortionLossFn
    w, z = torch.rand(4, 8), torch.rand(4, 8)
    with pytest.raises(ValueError, match=r"weights \(4, 8\), z_vals \(4, 7\)"):
        DistortionLossFn.apply(w, z[:, :7], torch.zeros(4), torch.ones(4), 0.01)
    with pytest.raises(ValueError, match=r"nears \(3,\) and fars \(4,\)"):
        DistortionLossFn.apply(w, z, torch.zeros(3), torch.ones(4), 0.01)
