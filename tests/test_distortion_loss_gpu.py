"""GPU: the distortion loss of mip-NeRF 360 on the device (DistortionLossFn: nvsf_distortion_loss_fwd / _bwd) against the O(T^2)
definition in float64 (tests/distortion_oracle.py).  The bar is per element |kernel - ref| <= 2^-23 |ref| + 1e-12: one fp32 rounding of
an fp64 result with a factor two of slack; the absolute part is ten times what the order of an fp64 sum of 768 terms <= 1 can move
it (the cases keep every row of weights at a sum <= 1, as a compositor's rows are).  At 4096 x 768 the reference is
`losses.distortion_loss` in float64, which tests/test_distortion_loss_cpu.py pins to the definition."""
import functools

import numpy as np
import pytest
import torch

import distortion_oracle as O

pytestmark = pytest.mark.gpu

# tile edges (63, 64, 65, 129), the four-rays-per-workgroup edge (1, 3, 5, 9, 257 rays), T + U of the shipped sizes (832)
SHAPES = [(1, 1), (3, 2), (4, 63), (5, 64), (5, 65), (9, 129), (257, 48), (64, 832)]
BIG = (4096, 768)


def _device_run(c, dev, alpha=O.ALPHA, grad_loss=None):
    from nvsf.nerf.losses import DistortionLossFn
    w = c["w"].to(dev).requires_grad_()
    loss, ray = DistortionLossFn.apply(w, c["z"].to(dev), c["nears"].to(dev), c["fars"].to(dev), alpha, True)
    (grad,) = torch.autograd.grad(loss, w, grad_outputs=None if grad_loss is None else torch.tensor(grad_loss, device=dev))
    return ray.detach().cpu(), loss.detach().cpu(), grad.cpu()


def _check(tag, got, ref):
    """every element of (ray, loss, grad) inside the bar; prints the worst excess first"""
    worst = []
    for name, g, r in zip(("ray_loss", "loss", "grad"), got, ref):
        g, r = g.double().reshape(-1), r.reshape(-1)
        assert g.shape == r.shape, name
        err, bar = (g - r).abs(), O.bar(r)
        k = int((err - bar).argmax())
        worst.append((name, float(err[k]), float(bar[k]), float(r[k])))
    print(f"distortion {tag}: " + "; ".join(f"{n} err {e:.3e} bar {b:.3e} at ref {r:.6e}" for n, e, b, r in worst))
    for name, e, b, _ in worst:
        assert e <= b, name  # a NaN fails here as well


@pytest.mark.parametrize("kind", O.KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_loss_and_gradient_against_the_definition(dev, shape, kind):
    N, T = shape
    c = O.case(N, T, kind)
    ref = O.reference(N, T, kind)
    got = _device_run(c, dev)
    _check(f"{N}x{T} {kind}", got, ref)
    ray, loss, grad = got
    assert bool(torch.isfinite(grad).all())
    if kind == "degenerate":
        bad = ~(torch.isfinite(c["fars"] - c["nears"]) & (c["fars"] > c["nears"]))
        assert bool(bad[0]) and bool((ray[bad] == 0).all()) and bool((grad[bad] == 0).all())
        assert N == 1 or (float(ref[1]) > 0 and bool((grad[~bad] != 0).any()))
    elif kind == "zeros":
        assert bool((ray[::3] == 0).all())
        # a row of zero weights still has a gradient 2 sum_j w_j |m_k - m_j| = 0 only because its own weights are zero
        assert bool((grad[::3] == 0).all())
    else:
        assert float(ref[1]) > 0


@functools.lru_cache(maxsize=None)
def _big_reference():
    """4096 x 768, the cancellation case: `distortion_loss` in float64 on the CPU (value, per-ray values, autograd gradient)."""
    from nvsf.nerf.losses import distortion_loss, distortion_ray_losses
    c = O.case(BIG[0], BIG[1], "peaked")
    w = c["w"].double().clone().requires_grad_()
    z, nears, fars = c["z"].double(), c["nears"].double(), c["fars"].double()
    loss = distortion_loss(w, z, nears, fars, O.ALPHA)
    (grad,) = torch.autograd.grad(loss, w)
    return distortion_ray_losses(w.detach(), z, nears, fars), loss.detach(), grad


def test_full_size_against_the_float64_host_form(dev):
    c = O.case(BIG[0], BIG[1], "peaked")
    _check(f"{BIG[0]}x{BIG[1]} peaked", _device_run(c, dev), _big_reference())


@pytest.mark.parametrize("shape", [(3, 2), (257, 48), BIG], ids=lambda s: f"{s[0]}x{s[1]}")
def test_two_runs_are_bit_identical(dev, shape):
    c = O.case(shape[0], shape[1], "peaked" if shape == BIG else "spread")
    a, b = _device_run(c, dev), _device_run(c, dev)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def _entries(dev, w, z, nears, fars, N, T, alpha, grad_loss=1.0, ws_bytes=None):
    """the two entries called directly on flat device buffers -> (ray, loss, state, grad) on the CPU"""
    from nvsf import _hip
    ray, loss = torch.empty(N, device=dev), torch.empty((), device=dev)
    state, ws = torch.empty(N, 2, dtype=torch.float64, device=dev), torch.empty((N + 3) // 4, dtype=torch.float64, device=dev)
    gl, grad = torch.tensor(grad_loss, device=dev), torch.full((N * T + 1,), 7.0, device=dev)
    head = (w.data_ptr(), z.data_ptr(), _hip.ptr(nears), _hip.ptr(fars), N, T, alpha)
    _hip.call("nvsf_distortion_loss_fwd", *head, _hip.ptr(ws), 8 * ws.numel() if ws_bytes is None else ws_bytes, _hip.ptr(ray), _hip.ptr(loss),
              _hip.ptr(state))
    _hip.call("nvsf_distortion_loss_bwd", *head, _hip.ptr(state), _hip.ptr(gl), grad.data_ptr())
    assert float(grad[-1]) == 7.0  # nothing past the last row
    return ray.cpu(), loss.cpu(), state.cpu(), grad[:-1].view(N, T).cpu()


def test_unaligned_views_give_the_same_bits(dev):
    """An [N, T] view that starts one element into its buffer, T = 7: rows at every 4-byte phase."""
    N, T = 6, 7
    c = O.case(N, T, "spread")
    res = []
    for shift in (0, 1):
        buf = [torch.zeros(N * T + 4, device=dev) for _ in range(2)]
        w, z = (b[shift:shift + N * T] for b in buf)
        w.copy_(c["w"].view(-1)), z.copy_(c["z"].view(-1))
        assert w.data_ptr() % 16 == 4 * shift
        res.append(_entries(dev, w, z, c["nears"].to(dev), c["fars"].to(dev), N, T, O.ALPHA))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    ray, loss, state, grad = res[1]
    _check("6x7 shifted view", (ray, loss, grad), O.reference(N, T, "spread"))
    assert float((state[:, 0] - c["w"].double().sum(dim=1)).abs().max()) <= 1e-15  # state = the row totals (W, M)


def test_grad_loss_scales_the_gradient(dev):
    c = O.case(9, 129, "spread")
    ref = O.distortion(c["w"], c["z"], c["nears"], c["fars"], O.ALPHA, grad_loss=2.5)
    got = _device_run(c, dev, grad_loss=2.5)
    _check("9x129 grad_loss 2.5", got, ref)  # one rounding of 2.5 alpha / N d ray / d w, not a rounded gradient times 2.5
    assert not torch.equal(got[2], _device_run(c, dev)[2])


def test_bad_arguments_are_refused_before_any_launch(dev):
    from nvsf import _hip
    N, T = 9, 5
    c = O.case(N, T, "spread")
    w, z, nears, fars = (c[k].to(dev).contiguous() for k in ("w", "z", "nears", "fars"))
    ray, loss = torch.full((N,), 3.0, device=dev), torch.full((), 3.0, device=dev)
    state, ws = torch.zeros(N, 2, dtype=torch.float64, device=dev), torch.zeros(3, dtype=torch.float64, device=dev)
    fwd = lambda *a: _hip.call("nvsf_distortion_loss_fwd", *a)
    ok = (_hip.ptr(w), _hip.ptr(z), _hip.ptr(nears), _hip.ptr(fars), N, T, O.ALPHA, _hip.ptr(ws), 24, _hip.ptr(ray), _hip.ptr(loss), _hip.ptr(state))
    with pytest.raises(_hip.NvsfHipError, match=r"status -1 "):  # 9 rays are three workgroups: 24 bytes
        fwd(*ok[:8], 16, *ok[9:])
    with pytest.raises(_hip.NvsfHipError, match=r"status -1 "):
        fwd(*ok[:5], 0, *ok[6:])  # T = 0
    for k in (0, 1, 2, 3, 7, 10, 11):  # a null pointer (ray_loss alone may be null)
        with pytest.raises(_hip.NvsfHipError, match=r"status -1 "):
            fwd(*ok[:k], None, *ok[k + 1:])
    with pytest.raises(_hip.NvsfHipError, match=r"status -1 "):
        _hip.call("nvsf_distortion_loss_bwd", *ok[:7], None, _hip.ptr(loss), _hip.ptr(w))
    torch.cuda.synchronize()
    assert float(loss) == 3.0 and bool((ray == 3.0).all()) and bool((state == 0).all())  # nothing was launched
    fwd(*ok[:9], None, *ok[10:])  # without per-ray losses
    assert abs(float(loss) - float(O.reference(N, T, "spread")[1])) <= float(O.bar(O.reference(N, T, "spread")[1]))
    fwd(*ok[:4], 0, *ok[5:])  # N = 0 writes loss = 0
    assert float(loss) == 0.0


def _step_case(dev, **kw):
    from test_train_step_gpu import _batch
    from nvsf import synthetic as S
    from nvsf.nerf.models.network_static import NeRFNetworkStatic
    from nvsf.nerf.train_step import RenderTrainStep
    mk = dict(bound=S.BOUND, min_near=S.MIN_NEAR, min_near_lidar=S.MIN_NEAR, lidar_max_depth=S.LIDAR_MAX_DEPTH, log2_hashmap_size=12)
    torch.manual_seed(3)
    teacher = NeRFNetworkStatic(**mk).to(dev).eval()
    student = NeRFNetworkStatic(**mk).to(dev)
    step = RenderTrainStep(student, iters=400, scale=S.SCALE, ema_decay=None, distortion_loss=True, **kw)
    return step, student, _batch(S, teacher, dev, n=256)


@pytest.mark.parametrize("sizes", [dict(num_steps=48), dict(num_steps=24, upsample_steps=8)], ids=["T48", "T24+U8"])
def test_step_losses_use_the_kernel_on_the_device(dev, sizes):
    """`losses()` with the switch on a device render: both parts come from DistortionLossFn and equal the definition on the rows the
    renders returned, with the ranges `run` used."""
    step, student, batch = _step_case(dev, **sizes)
    assert step.alpha_dist == 0.01
    seen, render = [], step._render

    def keep(*a, **k):
        seen.append(render(*a, **k))
        return seen[-1]
    step._render = keep
    total, parts = step.losses(batch)
    assert len(seen) == 2 and bool(torch.isfinite(total))
    rows = sizes["num_steps"] + sizes.get("upsample_steps", 0)
    for key, r, lidar in (("dist_lidar", seen[0], True), ("dist", seen[1], False)):
        assert parts[key].grad_fn is not None and type(parts[key].grad_fn).__name__.startswith("DistortionLossFn")
        assert tuple(r["weights"].shape) == (256, rows) and tuple(r["z_vals"].shape) == (256, rows)
        (gw,) = torch.autograd.grad(parts[key], r["weights"], retain_graph=True)
        assert gw.shape == r["weights"].shape and float(gw.abs().max()) > 0 and bool(torch.isfinite(gw).all())
        sfx = "_lidar" if lidar else ""
        o, d = batch["rays_o" + sfx].view(-1, 3), batch["rays_d" + sfx].view(-1, 3)
        nears, fars = student._near_far(o, d, lidar, student.aabb_train)
        w, z = r["weights"].detach().float().cpu(), r["z_vals"].detach().float().cpu()
        hit = (fars > nears).cpu()  # a camera ray that misses the box has no range, and its row no order
        assert bool(hit.any()) and bool((z[hit][:, 1:] >= z[hit][:, :-1]).all())
        _, ref, ref_grad = O.distortion(w, z, nears.cpu(), fars.cpu(), float(np.float32(0.01)))
        err, bar = abs(float(parts[key].detach()) - float(ref)), float(O.bar(ref))
        gerr = (gw.double().cpu() - ref_grad).abs() - O.bar(ref_grad)
        print(f"distortion step {key} rows {rows}: loss {float(ref):.6e} err {err:.3e} bar {bar:.3e}; grad excess {float(gerr.max()):.3e}")
        assert float(ref) > 0 and err <= bar and float(gerr.max()) <= 0
    step.sync()


@pytest.mark.parametrize("kw", [dict(), dict(split_backward=False), dict(ray_chunks=2)], ids=["split", "joint", "chunks2"])
def test_full_step_with_the_switch_ends_with_finite_parameters(dev, kw):
    step, student, batch = _step_case(dev, num_steps=48, **kw)
    loss, parts, _ = step.step(batch)
    step.sync()
    torch.cuda.synchronize()
    assert {"dist_lidar", "dist"} <= set(parts) and all(bool(torch.isfinite(v)) for v in parts.values()) and bool(torch.isfinite(loss))
    assert float(parts["dist_lidar"]) > 0 and float(parts["dist"]) > 0
    assert all(bool(torch.isfinite(p).all()) for p in student.parameters())
