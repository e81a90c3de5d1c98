"""GPU parity of the occupancy-grid render (BASELINE config 3: march_rays_train / composite_rays_train in training
mode, the march_rays / composite_rays survivor loop in evaluation mode) of the static hash field against the CPU
oracle composition (tests/oracle_lib.render_occupancy_*), plus the density-grid maintenance driver."""
import numpy as np
import pytest
import torch

import oracle_lib as O

pytestmark = pytest.mark.gpu


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# the grid of BASELINE config 2 (16 levels x 2 features) and the reference-default shape (8 levels x 4; here with dense coarse levels)
GRIDS = {"L16F2": {}, "L8F4": dict(n_levels_hash=8, n_features_per_level_hash=4, base_resolution=16, max_resolution=1024)}


@pytest.fixture(scope="module", params=list(GRIDS))
def setup(dev, request):
    from nvsf import synthetic as S, field_ops as ops
    from nvsf.nerf.models.network_static import NeRFNetworkStatic
    torch.manual_seed(0)
    m = NeRFNetworkStatic(bound=S.BOUND, min_near=S.MIN_NEAR, min_near_lidar=S.MIN_NEAR, lidar_max_depth=S.LIDAR_MAX_DEPTH, log2_hashmap_size=15,
                          **GRIDS[request.param])
    assert ops.occupancy_fused_eligible(m.hash_encoder_camera.spec)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for enc in (m.hash_encoder_lidar, m.hash_encoder_camera):
            enc.params.copy_(torch.randn(enc.params.shape, generator=g) * 0.1)
        m.sigma_net.params.mul_(2.0)
    m = m.to(dev).enable_occupancy_grid().to(dev)
    rng = np.random.default_rng(0)
    grid = S.boxes_density_grid(rng, cascades=m.cascade, H=m.grid_size, n_boxes=48)
    m.set_density_grid(_t(grid, dev), thresh=0.5)
    bits = O.packbits(grid, 0.5)
    assert np.array_equal(m.density_bitfield.cpu().numpy(), bits)
    return m, bits, S


def _field(m, lidar):
    enc = m.hash_encoder_lidar if lidar else m.hash_encoder_camera
    f16 = lambda net: net.params.detach().cpu().numpy().astype(np.float16)
    return (enc.params.detach().cpu().numpy().astype(np.float16), enc.spec, f16(m.sigma_net),
            f16(m.raydrop_net) if lidar else f16(m.color_net), f16(m.intensity_net) if lidar else None)


def _near_far(m, S, o, d, lidar):
    if lidar:
        return np.full(len(o), m.min_near_lidar, np.float32), np.full(len(o), m.lidar_max_depth, np.float32)
    return O.near_far_from_aabb(o, d, np.array([-S.BOUND] * 3 + [S.BOUND] * 3, np.float32), m.min_near)


def _assert_close_up_to_one_terminal_sample(out, ref, sfx, pick, T_thresh, t_max, min_exact):
    """1e-4 abs on every ray, except that a ray whose transmittance lands within float noise of T_thresh may take ONE more
    sample on one side only.  That sample is met with transmittance T ~ T_thresh (the compositor stops after the first sample
    whose incoming T is below the threshold, raymarching.cu:1015-1040), so its weight alpha * T is at most T_thresh: the exempt
    rays are bounded by that one weight -- weights_sum and every image channel (colour in [0, 1], background <= 1) by T_thresh,
    depth by T_thresh * t_max -- on top of the 1e-4."""
    ws = out["weights_sum" + sfx].cpu().numpy()[pick]
    dp = out["depth" + sfx][0].cpu().numpy()[pick]
    im = out["image" + sfx][0].cpu().numpy()[pick]
    e_ws, e_dp, e_im = np.abs(ws - ref["weights_sum"]), np.abs(dp - ref["depth"]), np.abs(im - ref["image"]).max(-1)
    exact = (e_ws <= 1e-4) & (e_dp <= 1e-4) & (e_im <= 1e-4)
    assert exact.mean() >= min_exact, exact.mean()
    w1 = 1.05 * T_thresh  # one terminal sample's weight (5 % for the noise in T itself)
    assert (e_ws <= 1e-4 + w1).all(), float(e_ws.max())
    assert (e_im <= 1e-4 + w1).all(), float(e_im.max())
    assert (e_dp <= 1e-4 + w1 * t_max).all(), float(e_dp.max())


@pytest.mark.parametrize("lidar", [True, False])
def test_training_mode_matches_oracle_and_backpropagates(dev, setup, lidar):
    m, bits, S = setup
    m.train()
    rng = np.random.default_rng(5)
    N, max_steps = 300, 256
    o, d = (S.lidar_rays if lidar else S.camera_rays)(N, rng)
    nears, fars = _near_far(m, S, o, d, lidar)
    ref = O.render_occupancy_train(o, d, nears, fars, bits, float(S.BOUND), m.cascade, m.grid_size, max_steps, 0.0, np.zeros(N, np.float32),
                                   _field(m, lidar), lidar)
    out = m.render(_t(o, dev)[None], _t(d, dev)[None], torch.tensor([[0.5]], device=dev), cal_lidar_color=lidar, force_all_rays=True,
                   max_steps=max_steps, perturb=False)
    sfx = "_lidar" if lidar else ""
    assert int(m.step_counter[(m.local_step - 1) % 16, 0]) == ref["n_samples"] > 0
    np.testing.assert_allclose(out["weights_sum" + sfx].detach().cpu().numpy(), ref["weights_sum"], atol=1e-4, rtol=0)
    np.testing.assert_allclose(out["depth" + sfx][0].detach().cpu().numpy(), ref["depth"], atol=1e-4, rtol=0)
    np.testing.assert_allclose(out["image" + sfx][0].detach().cpu().numpy(), ref["image"], atol=1e-4, rtol=0)
    (out["image" + sfx].sum() + out["weights_sum" + sfx].sum()).backward()
    enc = m.hash_encoder_lidar if lidar else m.hash_encoder_camera
    assert enc.params.grad is not None and torch.isfinite(enc.params.grad).all() and enc.params.grad.abs().sum() > 0
    m.zero_grad(set_to_none=True)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("lidar", [True, False])
def test_evaluation_loop_matches_oracle(dev, setup, lidar, fused):
    """fused=False: the host loop over surviving rays (march_rays -> field -> composite_rays);
    fused=True: the one-launch kernel nvsf_render_occupancy_fwd.  Both against the oracle's loop."""
    m, bits, S = setup
    m.eval()
    rng = np.random.default_rng(6)
    N, max_steps = 257, 128
    o, d = (S.lidar_rays if lidar else S.camera_rays)(N, rng)
    nears, fars = _near_far(m, S, o, d, lidar)
    ref = O.render_occupancy_infer(o, d, nears, fars, bits, float(S.BOUND), m.cascade, m.grid_size, max_steps, 0.0, _field(m, lidar), lidar,
                                   T_thresh=1e-2)
    with torch.no_grad():
        out = m.render(_t(o, dev)[None], _t(d, dev)[None], torch.tensor([[0.5]], device=dev), cal_lidar_color=lidar, max_steps=max_steps,
                       T_thresh=1e-2, fused=fused)
    sfx = "_lidar" if lidar else ""
    _assert_close_up_to_one_terminal_sample(out, ref, sfx, slice(None), 1e-2, float(fars[fars < 1e30].max()), min_exact=0.99)


@pytest.mark.parametrize("lidar", [True, False])
def test_fused_occupancy_equals_host_loop(dev, setup, lidar):
    """Larger batch, default T_thresh, coloured background: one-launch kernel vs the host loop of the same library.
    The two differ only in where a march restarts (the loop restarts from the compositor's accumulated t), i.e. by
    float noise; a ray may flip one borderline sample, hence the 99.5 % criterion."""
    m, bits, S = setup
    m.eval()
    rng = np.random.default_rng(8)
    N, max_steps = 2000, 512
    o, d = (S.lidar_rays if lidar else S.camera_rays)(N, rng)
    args = (_t(o, dev)[None], _t(d, dev)[None], torch.tensor([[0.5]], device=dev))
    bg = None if lidar else torch.tensor([0.1, 0.5, 0.9], device=dev)
    from nvsf import field_ops as ops
    launches, real = [], ops.render_occupancy
    ops.render_occupancy = lambda *a_, **k_: (launches.append(1), real(*a_, **k_))[1]
    try:
        with torch.no_grad():
            a = m.render(*args, cal_lidar_color=lidar, max_steps=max_steps, bg_color=bg, fused=True)
            b = m.render(*args, cal_lidar_color=lidar, max_steps=max_steps, bg_color=bg, fused=False)
    finally:
        ops.render_occupancy = real
    assert len(launches) == 1  # the one-launch kernel ran for `fused=True` (either grid shape), the survivor loop for the other
    sfx = "_lidar" if lidar else ""
    assert float(b["weights_sum" + sfx].max()) > 0.05  # the batch does hit occupied space
    for k in ("weights_sum" + sfx, "depth" + sfx, "image" + sfx):
        x, y = a[k].reshape(N, -1), b[k].reshape(N, -1)
        ok = ((x - y).abs() <= 1e-4).all(-1).float().mean()
        assert float(ok) > 0.995, (k, float(ok))


def test_fused_occupancy_step_cap_and_empty(dev, setup):
    """max_steps caps the samples of a ray; rays that never meet an occupied cell return the background."""
    m, bits, S = setup
    m.eval()
    rng = np.random.default_rng(9)
    o, d = S.camera_rays(64, rng)
    args = (_t(o, dev)[None], _t(d, dev)[None], torch.tensor([[0.5]], device=dev))
    with torch.no_grad():
        few = m.render(*args, max_steps=4, fused=True)
        many = m.render(*args, max_steps=1024, fused=True)
    assert float(few["weights_sum"].max()) < float(many["weights_sum"].max())
    saved = m.density_bitfield.clone()
    m.density_bitfield.zero_()
    with torch.no_grad():
        empty = m.render(*args, max_steps=256, fused=True)
    m.density_bitfield.copy_(saved)
    assert float(empty["weights_sum"].abs().max()) == 0.0 and float(empty["depth"].abs().max()) == 0.0
    assert torch.equal(empty["image"], torch.ones_like(empty["image"]))


def test_train_step_on_an_occupancy_model(dev):
    """RenderTrainStep on a model with enable_occupancy_grid(): a LiDAR + camera batch through run_cuda's training branch, three
    steps with force_all_rays left at its default.  The first step has no mean_count yet and reads the marcher's counter back; after
    the next update_extra_state the budgeted path runs (mean_count > 0: no host read, rays past the budget recorded but empty, the
    marcher's failure flag looked at by step()).  One counter row per RENDER: a step with both modalities writes two (camera first)."""
    from nvsf import synthetic as S
    from nvsf.nerf.loss_scaler import LossScaler
    from nvsf.nerf.models.network_static import NeRFNetworkStatic
    from nvsf.nerf.raymarching import raymarching
    from nvsf.nerf.train_step import RenderTrainStep
    from test_train_step_gpu import _batch
    kw = dict(bound=S.BOUND, min_near=S.MIN_NEAR, min_near_lidar=S.MIN_NEAR, lidar_max_depth=S.LIDAR_MAX_DEPTH, log2_hashmap_size=14)
    torch.manual_seed(3)
    teacher = NeRFNetworkStatic(**kw)
    with torch.no_grad():
        for enc in (teacher.hash_encoder_lidar, teacher.hash_encoder_camera):
            enc.params.normal_(0.0, 0.2)
    teacher = teacher.to(dev).eval()
    n = 256
    batch = _batch(S, teacher, dev, n=n, T=32, seed=4)
    torch.manual_seed(4)
    m = NeRFNetworkStatic(**kw)
    with torch.no_grad():
        for enc in (m.hash_encoder_lidar, m.hash_encoder_camera):
            enc.params.normal_(0.0, 0.1)
    m = m.to(dev).enable_occupancy_grid().to(dev)
    step = RenderTrainStep(m, num_steps=32, scale=S.SCALE, ema_decay=None)
    step.scaler = LossScaler(init_scale=64.0, growth_interval=10 ** 6)  # no overflow at this scale: no step is skipped
    t = batch["time"]
    m.update_extra_state(t, cal_lidar_color=True)
    assert m.mean_count == 0 and m.local_step == 0 and int(m.density_bitfield.count_nonzero()) > 0

    calls, real = [], raymarching.march_rays_train

    def spy(*args):
        out = real(*args)
        calls.append(dict(mean_count=args[9], force_all_rays=args[12], rows=out[0].shape[0], rays=out[3].detach().clone()))
        return out

    def one_step():
        before = {k: p.detach().clone() for k, p in m.named_parameters()}
        del calls[:]
        raymarching.march_rays_train = spy
        try:
            loss, parts, _ = step.step(batch)
        finally:
            raymarching.march_rays_train = real
        step.sync()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(v)) for v in parts.values()), (loss, parts)
        assert set(parts) == {"depth", "raydrop", "intensity", "chamfer", "rgb"}
        assert float(step.scaler.get_scale()) == 64.0  # not skipped
        moved = {k: not torch.equal(p.detach(), before[k]) for k, p in m.named_parameters() if p.grad is not None and p.numel() > 0}
        assert len(moved) == 6 and all(moved.values()), moved  # two tables, the density MLP, three heads
        assert len(calls) == 2  # the camera render, then the LiDAR render
        return list(calls)

    first = one_step()
    assert all(c["mean_count"] == 0 and not c["force_all_rays"] for c in first)
    rows = m.step_counter.cpu()
    for k, c in enumerate(first):
        total = int(c["rays"][:, 2].sum())
        assert rows[k].tolist() == [total, n] and total > 0
        assert c["rows"] == total + (128 - total % 128)  # the counter was read back: sliced to the aligned live count
    assert m.local_step == 2
    want = int(int(rows[:2, 0].sum()) / 2)
    m.update_extra_state(t, cal_lidar_color=True)
    assert m.mean_count == want > 0 and m.local_step == 0

    dropped = []
    for k in range(2):
        later = one_step()
        rows = m.step_counter.cpu()
        for j, c in enumerate(later):
            assert c["mean_count"] == want and not c["force_all_rays"]
            assert c["rows"] == want + (128 - want % 128)  # the budget, whatever the batch needs
            assert rows[2 * k + j].tolist() == [int(c["rays"][:, 2].sum()), n]  # rays past the budget are counted too
            dropped.append(int(((c["rays"][:, 1] + c["rays"][:, 2]) > c["rows"]).sum()))
        assert not raymarching.march_status_pending()  # step() looked at the failure flag of both launches
    assert m.local_step == 4
    print(f"budget {want} rows; rays past it per render (camera, LiDAR, camera, LiDAR): {dropped}")
    want = int(int(m.step_counter[:4, 0].sum()) / 4)
    m.update_extra_state(t, cal_lidar_color=True)
    assert m.mean_count == want

    # a budget that suffices: the budgeted render is the force_all_rays render of the same rays, bit for bit
    m.train()
    for lidar in (True, False):
        sfx = "_lidar" if lidar else ""
        o, d = (batch["rays_o_lidar"], batch["rays_d_lidar"]) if lidar else (batch["rays_o"], batch["rays_d"])
        with torch.no_grad():
            a = m.render(o, d, t, cal_lidar_color=lidar, force_all_rays=True, perturb=False, bg_color=1)
            total = int(m.step_counter[(m.local_step - 1) % 16, 0])
            m.mean_count = total + 1000
            b = m.render(o, d, t, cal_lidar_color=lidar, perturb=False, bg_color=1)
        raymarching.check_march_status(wait=True)
        assert int(m.step_counter[(m.local_step - 1) % 16, 0]) == total > 0
        for key in ("weights_sum" + sfx, "depth" + sfx, "image" + sfx):
            assert torch.equal(a[key], b[key]), key
        assert float(a["weights_sum" + sfx].max()) > 0.05


def test_density_grid_maintenance(dev, setup):
    m, bits, S = setup
    import copy
    mm = copy.deepcopy(m)
    mm.density_grid.zero_()
    mm.iter_density, mm.local_step = 0, 0
    t = torch.tensor([[0.5]], device=dev)
    mm.update_extra_state(t, cal_lidar_color=True)
    g1 = mm.density_grid.clone()
    assert mm.iter_density == 1 and (g1 > 0).all()  # every cell visited; sigma = exp(.) > 0
    # values are field densities at jittered cell centres: spot-check against the field at the exact centres (same order of magnitude)
    idx = torch.tensor([[10, 20, 30], [64, 64, 64], [127, 0, 5]], dtype=torch.int32, device=dev)
    from nvsf.nerf.raymarching import raymarching
    mo = raymarching.morton3D(idx).long()
    centres = (2 * idx.float() / (mm.grid_size - 1) - 1) * (1 - 1 / mm.grid_size)
    with torch.no_grad():
        sig = mm.density(centres, t, True)["sigma"]
    ratio = g1[0, mo] / sig
    assert (ratio > 0.2).all() and (ratio < 5).all()
    mm.update_extra_state(t, cal_lidar_color=True)
    assert (mm.density_grid >= g1 * 0.95 - 1e-6).all()  # exponential moving maximum with decay 0.95
    thr = min(mm.mean_density, mm.density_thresh)
    assert np.array_equal(mm.density_bitfield.cpu().numpy(), O.packbits(mm.density_grid.cpu().numpy(), thr))
    mm.iter_density = 16
    mm.update_extra_state(t, cal_lidar_color=True)  # partial update path
    assert mm.iter_density == 17 and torch.isfinite(mm.density_grid).all()


@pytest.mark.parametrize("lidar", [True, False])
def test_config3_full_size_matches_oracle(dev, lidar):
    """BASELINE config 3 as stated: the config-2 field (L16 F2, log2_hashmap_size 19), occupancy grid, at most 1024 samples per
    ray, early termination at T < 1e-4 -- the whole 4096-ray batch through the one-launch kernel, 48 of its rays against the
    oracle's survivor loop (march_rays -> field -> composite_rays)."""
    from nvsf import synthetic as S
    from nvsf.nerf.models.network_static import NeRFNetworkStatic
    torch.manual_seed(0)
    m = NeRFNetworkStatic(bound=S.BOUND, min_near=S.MIN_NEAR, min_near_lidar=S.MIN_NEAR, lidar_max_depth=S.LIDAR_MAX_DEPTH)
    assert m.hash_encoder_lidar.spec.log2_hashmap_size == 19 and m.hash_encoder_lidar.spec.L == 16
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for enc in (m.hash_encoder_lidar, m.hash_encoder_camera):
            enc.params.copy_(torch.randn(enc.params.shape, generator=g) * 0.1)
        m.sigma_net.params.mul_(2.0)
    m = m.to(dev).enable_occupancy_grid().to(dev).eval()
    rng = np.random.default_rng(0)
    grid = S.boxes_density_grid(rng, cascades=m.cascade, H=m.grid_size, n_boxes=64)
    m.set_density_grid(_t(grid, dev), thresh=0.5)
    bits = O.packbits(grid, 0.5)
    N, K, max_steps = 4096, 48, 1024
    o, d = (S.lidar_rays if lidar else S.camera_rays)(N, rng)
    with torch.no_grad():
        out = m.render(_t(o, dev)[None], _t(d, dev)[None], torch.tensor([[0.5]], device=dev), cal_lidar_color=lidar, max_steps=max_steps,
                       T_thresh=1e-4, fused=True)
    pick = np.sort(rng.choice(N, K, replace=False))
    nears, fars = _near_far(m, S, o[pick], d[pick], lidar)
    ref = O.render_occupancy_infer(o[pick], d[pick], nears, fars, bits, float(S.BOUND), m.cascade, m.grid_size, max_steps, 0.0, _field(m, lidar),
                                   lidar, T_thresh=1e-4)
    sfx = "_lidar" if lidar else ""
    assert float(ref["weights_sum"].max()) > 0.05
    _assert_close_up_to_one_terminal_sample(out, ref, sfx, pick, 1e-4, float(fars[fars < 1e30].max()), min_exact=0.97)
