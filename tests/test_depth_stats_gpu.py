"""GPU: the depth statistics of DESIGN.md section 9n on the device (nvsf_ray_depth_stats_fwd / nvsf_ray_depth_quantile_bwd through
ops.ray_depth_stats and ops.DepthQuantileFn) against the float64 restatement of tests/depth_stats_oracle.py, and NeRFRenderer.run's
`depth_mode` on every form that renders a batch.

The bars (depth_stats_oracle.quantile_bar, std_bar, grad_bar) come from the kernel's arithmetic, not from its results.  The kernel
forms every sum in fp64 from the fp32 inputs and rounds once to fp32.  What separates it from the restatement is
  * that one rounding: 2^-24 of the value;
  * the order of its scan: a parallel and a sequential fp64 sum of T terms adding up to W differ by at most about T 2^-53 W, so
    a = tau - C_{i-1} (two such sums) moves by scan_error = T 2^-52 W, which the quantile carries as scan_error delta_i / w_i and the
    crossing sample's own gradient entry as scan_error delta_i / w_i^2;
  * the fp64 roundings of the last expression: 2^-50 (|z_i| + delta_i), resp. 2^-49 of the terms a gradient entry is added up from;
  * std: the w-weighted L2 norm of z - mu moves by at most the error of mu, T 2^-52 max|z|, plus T 2^-52 of itself.
A ray whose crossing the scan order could move to the neighbouring sample (the oracle's margin min_i |C_i - tau| below scan_error) would
have to be left out; tests/test_depth_stats_cpu.py asserts that the shared cases have none, and every case here asserts it again for
the rows it made on the device, so no ray is left out anywhere.  The strongest return is exact: an fp32 depth picked by comparisons of
fp32 weights."""
import functools

import numpy as np
import pytest
import torch

import depth_stats_oracle as O

pytestmark = pytest.mark.gpu


def _to(dev, *ts):
    return tuple(t.to(dev) for t in ts)


def _check_stats(tag, got, ref, T, levels):
    """quantiles, mode, std of one call against the oracle's `stats`, inside the bars; prints the worst ratio to the bar first"""
    report = []
    q = got["quantiles"].double().cpu()
    assert tuple(q.shape) == tuple(ref["quantiles"].shape)
    for l, p in enumerate(ref["parts"]):
        assert bool(O.settled(p, T).all()), (tag, "unsettled rays", l)
        err, bar = (q[:, l] - p["t"]).abs(), O.quantile_bar(p, T)
        k = int((err / bar.clamp(min=1e-300)).argmax())
        report.append(f"q={levels[l]} err {float(err[k]):.3e} bar {float(bar[k]):.3e}")
        assert bool((err <= bar).all()), (tag, levels[l], k, float(err[k]), float(bar[k]))  # a NaN fails here as well
        assert bool((q[:, l][~p["ok"]] == 0).all())
    if "mode" in got:
        assert torch.equal(got["mode"].double().cpu(), ref["mode"]), (tag, "mode")
    if "std" in got:
        err, bar = (got["std"].double().cpu() - ref["std"]).abs(), O.std_bar(ref, T)
        report.append(f"std err {float(err.max()):.3e} bar {float(bar[int(err.argmax())]):.3e}")
        assert bool((err <= bar).all()), (tag, "std")
    print(f"depth stats {tag}: " + "; ".join(report))


# ---- the two entries against the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [True, False], ids=["normalised", "absolute"])
@pytest.mark.parametrize("Q", [1, 4])
@pytest.mark.parametrize("kind", O.KINDS)
@pytest.mark.parametrize("shape", O.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_statistics_and_gradient_against_the_definition(dev, shape, kind, Q, normalize):
    from nvsf import field_ops as ops
    N, T = shape
    c, levels = O.case(N, T, kind), O.LEVELS[Q]
    ref = O.reference(N, T, kind, Q, normalize)
    w, z, nears, fars = _to(dev, c["w"], c["z"], c["nears"], c["fars"])
    got = ops.ray_depth_stats(w, z, nears, fars, levels, normalize)
    _check_stats(f"{N}x{T} {kind} Q={Q} norm={normalize}", got, ref, T, levels)
    # the autograd node: the same values, and the gradient entry by entry
    gq = O.grad_seed(N, Q)
    wg = w.clone().requires_grad_()
    t = ops.DepthQuantileFn.apply(wg, z, nears, fars, levels, normalize)
    assert torch.equal(t.detach(), got["quantiles"])
    (grad,) = torch.autograd.grad(t, wg, grad_outputs=gq.to(dev))
    g_ref = O.quantile_grad(c["w"], c["z"], c["nears"], c["fars"], levels, normalize, gq)
    bar = O.grad_bar(c["w"], c["z"], c["nears"], c["fars"], levels, normalize, gq, g_ref)
    err = (grad.double().cpu() - g_ref).abs()
    assert bool((err <= bar).all()), (float((err - bar).max()), int((err - bar).argmax()))
    dead = torch.stack([~p["ok"] for p in ref["parts"]], 1).all(dim=1)
    assert bool((grad.cpu()[dead] == 0).all())
    if kind == "zeros":
        assert bool(dead[::3].all())
    elif kind == "random" and T > 1:  # distinct depths, positive weights (T = 1: t = z + q delta whatever the weight)
        assert float(g_ref.abs().max()) > 0 and float(grad.abs().max()) > 0


@functools.lru_cache(maxsize=None)
def _big_reference():
    c = O.case(*O.BIG, "random")
    return O.stats(c["w"], c["z"], c["nears"], c["fars"], O.LEVELS[4], True)


def test_workload_size(dev):
    """4096 x 768, the shipped batch: twelve chunks per row, 1024 workgroups."""
    from nvsf import field_ops as ops
    N, T = O.BIG
    c = O.case(N, T, "random")
    got = ops.ray_depth_stats(*_to(dev, c["w"], c["z"], c["nears"], c["fars"]), O.LEVELS[4], True)
    _check_stats(f"{N}x{T} random", got, _big_reference(), T, O.LEVELS[4])


@pytest.mark.parametrize("shape", [(5, 64), (67, 200)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_weights_of_a_real_compositor_call(dev, shape):
    """Rows as the renders make them: ops.CompositeWeightsFn on random densities (some rays saturate, some stay thin)."""
    from nvsf import field_ops as ops
    N, T = shape
    gen = torch.Generator().manual_seed(11 * N + T)
    nears = torch.full((N,), 0.01)
    fars = torch.full((N,), 0.81)
    z = (nears[:, None] + (fars - nears)[:, None] * torch.sort(torch.rand(N, T, generator=gen), dim=1).values).to(dev)
    sigma = torch.rand(N, T, generator=gen) ** 6 * 40.0 * torch.rand(N, 1, generator=gen) * T
    sigma[0] *= 1e-3
    sigma = sigma.to(dev)
    nears, fars = _to(dev, nears, fars)
    w, ws, depth = ops.CompositeWeightsFn.apply(sigma, z, nears, fars, 1.0)
    assert float(ws.max()) > 0.99 and float(ws.min()) < 0.9
    for normalize in (True, False):
        got = ops.ray_depth_stats(w, z, nears, fars, O.LEVELS[4], normalize)
        _check_stats(f"{N}x{T} composited norm={normalize}", got, O.stats(w, z, nears, fars, O.LEVELS[4], normalize), T, O.LEVELS[4])


def test_dyadic_rows_are_bit_identical_to_the_oracle(dev):
    """Every sum exact in fp64 whatever its order (tests/test_depth_stats_cpu.py): what is left is one fp64 division and addition,
    the same on either side, so the kernel's quantiles ARE the oracle's rounded to fp32; q = 1 included (the crossing test sees the
    total of its own scan)."""
    from nvsf import field_ops as ops
    w, z, nears, fars, levels = O.dyadic_case()
    ref = O.stats(w, z, nears, fars, levels)
    got = ops.ray_depth_stats(*_to(dev, w, z, nears, fars), levels, True)
    assert torch.equal(got["quantiles"].cpu(), ref["quantiles"].float())
    assert torch.equal(got["mode"].cpu(), ref["mode"].float())
    assert bool((got["quantiles"][0] == 0).all()) and float(got["std"][0]) == 0.0


def test_edge_rows(dev):
    """All-zero weights, a crossing in the first and in the last sample, q = 1, T = 1, the absolute form below its level."""
    from nvsf import field_ops as ops
    T = 8
    z = (torch.arange(T, dtype=torch.float64) / 16)[None].float().repeat(4, 1)
    w = torch.zeros(4, T)
    w[1, 0], w[1, 1] = 0.5, 0.25
    w[2, -1] = 0.5
    w[3, 0], w[3, 1] = 0.25, 0.125
    nears, fars = torch.zeros(4), torch.full((4,), 0.5)
    got = ops.ray_depth_stats(*_to(dev, w, z, nears, fars), (0.25, 0.5, 1.0), True)
    q = got["quantiles"].cpu()
    assert torch.equal(q, O.stats(w, z, nears, fars, (0.25, 0.5, 1.0))["quantiles"].float())
    assert bool((q[0] == 0).all()) and float(got["mode"][0]) == 0 and float(got["std"][0]) == 0
    assert float(q[1, 0]) == (1 / 16) * 0.1875 / 0.5 and float(q[1, 2]) == 1 / 8 and float(q[2, 1]) == 7 / 16 + 1 / 32 and float(q[2, 2]) == 0.5
    absolute = ops.ray_depth_stats(*_to(dev, w, z, nears, fars), (0.25, 0.5), False)["quantiles"].cpu()
    assert float(absolute[3, 0]) == 1 / 16 and float(absolute[3, 1]) == 0.0 and float(absolute[2, 1]) == 0.5
    one = ops.ray_depth_stats(*_to(dev, torch.tensor([[0.25]]), torch.tensor([[0.125]]), nears[:1], fars[:1]), (0.5, 1.0))
    assert one["quantiles"].cpu().tolist() == [[0.375, 0.625]] and float(one["mode"]) == 0.125 and float(one["std"]) == 0
    wg = w.to(dev).requires_grad_()
    t = ops.DepthQuantileFn.apply(wg, z.to(dev), nears.to(dev), fars.to(dev), (0.5,), False)
    (g,) = torch.autograd.grad(t.sum(), wg)
    assert bool((g[0] == 0).all()) and bool((g[3] == 0).all()) and bool((g[1] != 0).any())  # "no return" has no gradient
    empty = ops.ray_depth_stats(*_to(dev, torch.zeros(0, 5), torch.zeros(0, 5), torch.zeros(0), torch.zeros(0)))
    assert tuple(empty["quantiles"].shape) == (0, 1) and tuple(empty["mode"].shape) == (0,)


def test_two_runs_are_bit_identical(dev):
    from nvsf import field_ops as ops
    c = O.case(67, 200, "random")
    args = _to(dev, c["w"], c["z"], c["nears"], c["fars"])
    gq = O.grad_seed(67, 4).to(dev)
    runs = []
    for _ in range(2):
        wg = args[0].clone().requires_grad_()
        t = ops.DepthQuantileFn.apply(wg, *args[1:], O.LEVELS[4], True)
        (g,) = torch.autograd.grad(t, wg, grad_outputs=gq)
        s = ops.ray_depth_stats(*args, O.LEVELS[4], True)
        runs.append((t.detach(), g, s["quantiles"], s["mode"], s["std"]))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_unaligned_views_and_null_outputs(dev):
    """Rows that start one row (T = 7: 28 bytes) into a larger buffer, so at every 4-byte phase; and each output pointer NULL in turn."""
    from nvsf import _hip, field_ops as ops
    N, T = 6, 7
    c = O.case(N + 1, T, "random")
    w_buf, z_buf = _to(dev, c["w"], c["z"])
    w, z = w_buf[1:, :], z_buf[1:, :]
    assert w.data_ptr() % 16 != 0 and w.is_contiguous()
    nears, fars = _to(dev, c["nears"][1:].contiguous(), c["fars"][1:].contiguous())
    ref = O.stats(c["w"][1:], c["z"][1:], c["nears"][1:], c["fars"][1:], O.LEVELS[4])
    got = ops.ray_depth_stats(w, z, nears, fars, O.LEVELS[4])
    _check_stats("6x7 view", got, ref, T, O.LEVELS[4])
    assert torch.equal(ops.ray_depth_stats(w.clone(), z.clone(), nears, fars, O.LEVELS[4])["quantiles"], got["quantiles"])
    wg = w_buf.clone().requires_grad_()
    t = ops.DepthQuantileFn.apply(wg[1:, :], z, nears, fars, O.LEVELS[4], True)
    (g,) = torch.autograd.grad(t.sum(), wg)
    assert bool((g[0] == 0).all()) and bool((g[1:] != 0).any())
    # NULL outputs: only what is asked for is written
    for want in (("quantiles",), ("mode",), ("std",), ("mode", "std")):
        part = ops.ray_depth_stats(w, z, nears, fars, O.LEVELS[4], True, want)
        assert set(part) == set(want)
        for k in want:
            assert torch.equal(part[k], got[k]), k
    lv = _hip.host_f64(O.LEVELS[4])
    _hip.call("nvsf_ray_depth_stats_fwd", _hip.ptr(w), _hip.ptr(z), _hip.ptr(nears), _hip.ptr(fars), N, T, lv, 4, 1, None, None, None, None)
    torch.cuda.synchronize()


def test_bad_arguments_are_refused_before_any_launch(dev):
    from nvsf import _hip, field_ops as ops
    N, T = 5, 9
    c = O.case(N, T, "random")
    w, z, nears, fars = _to(dev, c["w"], c["z"], c["nears"], c["fars"])
    q_out, state = torch.full((N, 4), 3.0, device=dev), torch.zeros(N, 4, 2, dtype=torch.float64, device=dev)
    grad = torch.full((N, T), 3.0, device=dev)
    lv = lambda *v: _hip.host_f64(v)
    fwd = lambda *a: _hip.call("nvsf_ray_depth_stats_fwd", *a)
    bwd = lambda *a: _hip.call("nvsf_ray_depth_quantile_bwd", *a)
    ok = (_hip.ptr(w), _hip.ptr(z), _hip.ptr(nears), _hip.ptr(fars), N, T, lv(0.5, 0.9), 2, 1, _hip.ptr(q_out), None, None, _hip.ptr(state))
    okb = ok[:9] + (_hip.ptr(state), _hip.ptr(q_out), _hip.ptr(grad))
    refused = pytest.raises(_hip.NvsfHipError, match=r"status -1 ")
    for bad in (lv(0.0, 0.5), lv(0.5, -0.1), lv(0.5, 1.5), lv(float("nan"), 0.5), None):  # a level outside (0, 1], NaN, no levels
        with refused:
            fwd(*ok[:6], bad, *ok[7:])
        with refused:
            bwd(*okb[:6], bad, *okb[7:])
    for Q in (0, 5):
        with refused:
            fwd(*ok[:7], Q, *ok[8:])
    with refused:
        fwd(*ok[:5], 0, *ok[6:])  # T = 0
    with refused:
        fwd(*ok[:4], 1 << 20, 1 << 12, *ok[6:])  # N T > 2^31
    for k in (0, 1, 2, 3):
        with refused:
            fwd(*ok[:k], None, *ok[k + 1:])
    for k in (0, 1, 2, 3, 9, 10, 11):
        with refused:
            bwd(*okb[:k], None, *okb[k + 1:])
    torch.cuda.synchronize()
    assert bool((q_out == 3.0).all()) and bool((state == 0).all()) and bool((grad == 3.0).all())  # nothing was launched
    fwd(*ok[:4], 0, *ok[5:])  # N = 0: a successful no-op
    bwd(*okb[:4], 0, *okb[5:])
    torch.cuda.synchronize()
    assert bool((q_out == 3.0).all())
    with pytest.raises(ValueError):
        ops.ray_depth_stats(w, z, nears, fars, q=(0.5, float("nan")))
    with pytest.raises(_hip.NvsfHipError):
        ops.ray_depth_stats(w.cpu(), z.cpu(), nears.cpu(), fars.cpu())  # no CPU fall-back


# ---- run(depth_mode=...) ----------------------------------------------------------------------------------------------------------------
def _static(dev, seed=5):
    import test_static_grad_f64_gpu as G
    return G._model(dev, "L16F2", True, {}, seed)


def _lidar_batch(dev, N=64, seed=5):
    import test_static_grad_f64_gpu as G
    o, d, _ = G._rays(True, N, {}, seed, dev)
    return o, d, torch.tensor([[0.5]], device=dev)


def _stat_of(out, m, o, d, depth_mode, lidar=True):
    """the statistic `depth_mode` names, from the rows a run returned: ops.ray_depth_stats on its weights and z_vals"""
    from nvsf import field_ops as ops
    stat, level, normalize = ops.parse_depth_mode(depth_mode)
    nears, fars = m._near_far(o, d, lidar, m.aabb_train if m.training else m.aabb_infer)
    w, z = out["weights"].detach(), out["z_vals"].detach()
    if stat == "mode":
        return ops.ray_depth_stats(w, z, nears, fars, want=("mode",))["mode"]
    return ops.ray_depth_stats(w, z, nears, fars, (level,), normalize, ("quantiles",))["quantiles"][:, 0]


MODES = ["median", "mode", 0.9, ("absolute", 0.5)]


@pytest.mark.parametrize("form", ["fused", "hierarchical", "chain", "train"])
def test_run_returns_the_statistic_of_its_own_rows(dev, form):
    """64 rays x 64 samples of a small static field through every form that renders a batch: the three fused kernels (no_grad), the
    hierarchical pass (no_grad), the operator chain (gradients recorded, the field's fused training forward switched off) and the
    training forms (gradients recorded: the one-node render for the mean, the fused density forward + compositor for a quantile).
    `depth_lidar` is the chosen statistic of the returned weights / z_vals, everything else is what the same form returns without the
    argument, and depth_mode="mean" is byte-identical to a call without it."""
    m = _static(dev)
    o, d, t = _lidar_batch(dev)
    kw = dict(cal_lidar_color=True, num_steps=64, perturb=False)
    grad = form in ("chain", "train")
    m.train(grad)
    if form == "chain":
        m.fused_train_forward = False
    elif form == "hierarchical":
        kw.update(hierarchical=True, upsample_steps=16)
    same_rows = form != "train"  # there the mean comes from another form than a quantile: rows equal up to their fp32 roundings
    with torch.set_grad_enabled(grad):
        plain = {k: v.detach().clone() for k, v in m.run(o[None], d[None], t, **kw).items()}
        mean = m.run(o[None], d[None], t, depth_mode="mean", **kw)
        assert set(plain) == set(mean)
        for k in plain:
            assert torch.equal(plain[k], mean[k].detach()), k
        if form == "train":
            assert type(mean["weights"].grad_fn).__name__ == "RenderRaysFnBackward"
        del mean
        assert tuple(plain["weights"].shape) == (64, 80 if form == "hierarchical" else 64)
        for mode in MODES:
            if grad and mode == "mode":
                with pytest.raises(ValueError, match="piecewise constant"):
                    m.run(o[None], d[None], t, depth_mode=mode, **kw)
                continue
            out = m.run(o[None], d[None], t, depth_mode=mode, **kw)
            assert set(out) == set(plain) and out["depth_lidar"].shape == plain["depth_lidar"].shape
            assert out["depth_lidar"].requires_grad == grad
            for k in plain:
                if k != "depth_lidar" and same_rows:
                    assert torch.equal(out[k].detach(), plain[k]), (mode, k)
                elif k != "depth_lidar":
                    assert float((out[k].detach() - plain[k]).abs().max()) <= 1e-4, (mode, k)
            if grad:
                assert type(out["weights"].grad_fn).__name__ == "CompositeWeightsFnBackward"
            want = _stat_of(out, m, o, d, mode)
            assert torch.equal(out["depth_lidar"].detach().view(-1), want), mode
            assert not torch.equal(out["depth_lidar"].detach(), plain["depth_lidar"]), mode
        out = m.run(o[None], d[None], t, depth_stats=True, **kw)  # the mean stays, three more planes
        assert torch.equal(out["depth_lidar"].detach(), plain["depth_lidar"])
        assert set(out) - set(plain) == {"depth_median_lidar", "depth_mode_lidar", "depth_std_lidar"}
        assert torch.equal(out["depth_median_lidar"].view(-1), _stat_of(out, m, o, d, "median"))
        assert torch.equal(out["depth_mode_lidar"].view(-1), _stat_of(out, m, o, d, "mode"))
        assert out["depth_std_lidar"].shape == plain["depth_lidar"].shape and float(out["depth_std_lidar"].min()) >= 0
        assert not out["depth_std_lidar"].requires_grad
        both = m.run(o[None], d[None], t, depth_mode="median", depth_stats=True, **kw)
        assert torch.equal(both["depth_lidar"].detach(), both["depth_median_lidar"])
    assert float(plain["weights_sum_lidar"].max()) > 0.01  # the field is not empty


def test_camera_rays_get_the_statistic_too(dev):
    m = _static(dev).eval()
    import test_static_grad_f64_gpu as G
    o, d, _ = G._rays(False, 64, {}, 5, dev)
    t = torch.tensor([[0.5]], device=dev)
    with torch.no_grad():
        plain = m.run(o[None], d[None], t, num_steps=64)
        out = m.run(o[None], d[None], t, num_steps=64, depth_mode="median", depth_stats=True)
    assert torch.equal(out["image"], plain["image"]) and {"depth_median", "depth_mode", "depth_std"} <= set(out)
    assert torch.equal(out["depth"].view(-1), _stat_of(out, m, o, d, "median", lidar=False))


def test_staged_and_sharded_renders_return_the_median(dev):
    """The staged loop (chunks of 24 of the 64 rays) and frame_shard.render_sharded forward the keyword: their `depth_lidar` is the
    median of a whole-batch run, chunk by chunk the same kernels on the same rows."""
    from nvsf import frame_shard
    m = _static(dev).eval()
    o, d, t = _lidar_batch(dev)
    with torch.no_grad():
        whole = m.run(o[None], d[None], t, cal_lidar_color=True, num_steps=64, depth_mode="median")
        mean = m.render(o[None], d[None], t, cal_lidar_color=True, staged=True, max_ray_batch=24, num_steps=64)
        staged = m.render(o[None], d[None], t, cal_lidar_color=True, staged=True, max_ray_batch=24, num_steps=64, depth_mode="median")
        sharded = frame_shard.render_sharded(m, o[None], d[None], t, cal_lidar_color=True, max_ray_batch=24, num_steps=64, depth_mode="median")
    want = _stat_of(whole, m, o, d, "median")
    for got in (staged, sharded):
        assert set(got) == {"depth_lidar", "image_lidar"} and tuple(got["depth_lidar"].shape) == (1, 64)
        assert torch.equal(got["image_lidar"], mean["image_lidar"])
        # a chunk of 24 rays may take another kernel formulation than the batch of 64: same rows up to their fp32 roundings
        assert float((got["depth_lidar"].view(-1) - want).abs().max()) <= 1e-3
        assert not torch.equal(got["depth_lidar"], mean["depth_lidar"])
    assert torch.equal(staged["depth_lidar"], sharded["depth_lidar"])


def test_refusals_of_run(dev):
    m = _static(dev)
    o, d, t = _lidar_batch(dev, N=8)
    m.train()
    with pytest.raises(ValueError, match="piecewise constant"):
        m.run(o[None], d[None], t, cal_lidar_color=True, num_steps=16, depth_mode="mode")
    with pytest.raises(ValueError, match="depth_mode"):
        m.run(o[None], d[None], t, cal_lidar_color=True, num_steps=16, depth_mode="max")
    with torch.no_grad():
        with pytest.raises(ValueError, match="quantile level"):
            m.run(o[None], d[None], t, cal_lidar_color=True, num_steps=16, depth_mode=1.5)
        m.enable_occupancy_grid()
        with pytest.raises(ValueError, match="occupancy-grid march"):
            m.render(o[None], d[None], t, cal_lidar_color=True, depth_mode="median")
        with pytest.raises(ValueError, match="occupancy-grid march"):
            m.run_cuda(o[None], d[None], t, cal_lidar_color=True, depth_mode=("absolute", 0.5))


def test_median_range_l1_reaches_the_density_parameters(dev):
    """Training mode, T = 64 (where the one-node render would apply: it is bypassed for the fused density forward + compositor, whose
    weights carry the graph): the gradient of sum_n c_n |median_n - target_n| reaches sigma_net and the table through DepthQuantileFn
    and CompositeWeightsFn, and equals autograd through the float64 chain of tests/torch_f64_static.py composed with the oracle's
    quantile, at the bars of tests/test_static_grad_f64_gpu.py (the backward kernels below the quantile node are the ones pinned
    there; the node itself adds 2^-24, see above).  Rays stay in the functional where both sides provably differentiate the same
    expression: the crossing sample of the fp32 rows and of the fp64 rows is the same, it holds at least 1 % of the ray's weight (the
    1e-6 relative difference between fp32 and fp64 weights, amplified by W / w_i in delta a / w_i^2, stays below 1e-4), and the
    median is at least 1e-3 away from its target (the sign of the L1 term is settled), and the ray is not nearly empty (W >= 0.05:
    delta / w_i of a thinner ray, times the loss scale of 64, leaves the fp16 range of the MLP backward's hand-overs, the overflow a
    loss scaler answers by skipping the step).  At least half of the rays must qualify."""
    import test_static_grad_f64_gpu as G
    import torch_f64_static as R
    from nvsf import field_ops as ops
    N, T = 64, 64
    m = _static(dev).train()
    o, d, t = _lidar_batch(dev, N)
    for p in m.parameters():
        p.grad = None
    out = m.run(o[None], d[None], t, cal_lidar_color=True, num_steps=T, perturb=False, depth_mode="median")
    median, weights, z_vals = out["depth_lidar"].view(-1), out["weights"], out["z_vals"]
    assert median.requires_grad and weights.requires_grad
    assert type(weights.grad_fn).__name__ == "CompositeWeightsFnBackward"  # not RenderRaysFn: that form is bypassed
    assert torch.equal(median.detach(), _stat_of(out, m, o, d, "median"))
    nears, fars = m._near_far(o, d, True, m.aabb_train)
    mask = weights.detach() > ops.W_THRESH
    p64 = R.leaves(m, True)
    ref = R.render(m, p64, o, d, nears, fars, z_vals.detach(), mask, True)
    assert float((weights.detach().double() - ref["weights"].detach()).abs().max()) <= 1e-4
    part32 = O.quantile_parts(weights.detach().double(), z_vals.detach().double(), nears.double(), fars.double(), 0.5)
    part64 = O.quantile_parts(ref["weights"], z_vals.detach().double(), nears.double(), fars.double(), 0.5)
    gen = torch.Generator().manual_seed(3)
    target = (0.1 + 0.6 * torch.rand(N, generator=gen)).to(dev)
    keep = part32["ok"] & part64["ok"] & (part32["idx"] == part64["idx"]) & (part32["wi"] >= 0.01 * part32["W"]) & (part32["W"] >= 0.05) \
        & ((part64["t"].detach() - target.double()).abs() >= 1e-3)
    assert int(keep.sum()) >= N // 2, int(keep.sum())
    assert float((median.detach().double() - part64["t"].detach())[keep].abs().max()) <= 1e-4
    coef = (torch.rand(N, generator=gen) + 0.5).to(dev) * keep
    ((coef * (median - target).abs()).sum() * G.SCALE).backward()
    torch.cuda.synchronize()
    ((coef.double() * (part64["t"] - target.double()).abs()).sum() * G.SCALE).backward()
    enc = m.hash_encoder_lidar
    touched = R.touched_entries(ref["x01"], enc.spec)
    worst_t = G._compare("table", enc.params.grad, p64["hash_encoder_lidar"].grad, enc.spec, touched)
    worst_s = G._compare("sigma_net", m.sigma_net.params.grad, p64["sigma_net"].grad)
    print(f"median L1 through the render: {int(keep.sum())} of {N} rays; largest |g - g64| / bar: table {worst_t:.3f}, sigma_net {worst_s:.3f}")
    for head in (m.raydrop_net, m.intensity_net):  # the range says nothing about the heads
        assert head.params.grad is None or not bool(head.params.grad.any())


# ---- what the statistics are for ---------------------------------------------------------------------------------------------------------
def _two_box_field(dev, boxes_m, thickness_m):
    """An analytic field on NeRFRenderer: density 1 / thickness_m (per metre) inside the axis-aligned boxes, 0 outside; metres as the
    scene of nvsf/synthetic.py has them (scene units = metres x SCALE), the sensor at the origin."""
    from nvsf import synthetic as S
    from nvsf.nerf.models.renderer_dynamic import NeRFRenderer
    lo = torch.tensor(np.asarray(boxes_m)[:, :3] * S.SCALE, dtype=torch.float32, device=dev)
    hi = torch.tensor(np.asarray(boxes_m)[:, 3:] * S.SCALE, dtype=torch.float32, device=dev)

    class Boxes(NeRFRenderer):
        def __init__(self):
            super().__init__(bound=S.BOUND, min_near=S.MIN_NEAR, min_near_lidar=S.MIN_NEAR, lidar_max_depth=S.LIDAR_MAX_DEPTH)
            self.out_color_dim, self.out_lidar_color_dim = 3, 2

        def density(self, x, t=None, cal_lidar_color=False, **kwargs):
            inside = ((x[:, None, :] >= lo[None]) & (x[:, None, :] <= hi[None])).all(-1).any(-1)
            return {"sigma": inside.float() / (thickness_m * S.SCALE), "geo_feat": torch.zeros(x.shape[0], 1, device=x.device)}

        def color(self, x, d, cal_lidar_color=False, mask=None, **kwargs):
            return torch.full((x.shape[0], self.out_dim), 0.5, device=x.device)
    return Boxes().to(dev).eval()


def test_edge_rays_of_a_two_box_scene(dev):
    """Two boxes of nvsf.synthetic.street_range_image, one 10 m and one 25 m from the sensor, as a density field with a 0.3 m
    extinction length.  A beam that cuts the near box's corner through a few decimetres leaves about half of its weight there and
    the rest on the far box: its mean range floats between the two, metres from either; its median lies on one of the two faces
    (within the corner's chord resp. the extinction depth, 0.75 m, plus one sample spacing).  Edge rays are picked by the weight the
    near box holds (0.3 to 0.7 of the total), which is none of the statistics under test."""
    from nvsf import synthetic as S
    H, W, fov = 4, 2048, (2.0, 2.0, 8.0)
    near_box, far_box = [10.0, -3.0, -1.7, 12.0, 0.5, 3.0], [25.0, -6.0, -1.7, 27.0, 6.0, 3.0]
    rng = np.random.default_rng(0)
    first, _, _ = S.street_range_image(rng, boxes=[near_box, far_box], drop=0.0, isolated=0.0, hw=(H, W), fov=fov)
    behind, _, _ = S.street_range_image(rng, boxes=[far_box], drop=0.0, isolated=0.0, hw=(H, W), fov=fov)
    i, j = np.arange(W)[None, :], np.arange(H)[:, None]  # the sensor model of street_range_image
    beta = -(i - W / 2) / W * fov[2] * np.pi / 180.0
    alpha = (fov[0] - j / H * fov[1]) * np.pi / 180.0
    d = np.stack([np.cos(alpha) * np.cos(beta), np.cos(alpha) * np.sin(beta), np.broadcast_to(np.sin(alpha), (H, W))], -1).reshape(-1, 3)
    d = torch.from_numpy(np.ascontiguousarray(d, np.float32)).to(dev)
    o = torch.zeros_like(d)
    T = 768
    m = _two_box_field(dev, [near_box, far_box], 0.3)
    with torch.no_grad():
        out = m.run(o[None], d[None], torch.tensor([[0.5]], device=dev), cal_lidar_color=True, num_steps=T, depth_stats=True)
    to_m = 1.0 / S.SCALE
    w, z = out["weights"].double(), out["z_vals"].double() * to_m
    mean = out["depth_lidar"].view(-1).double() * to_m
    median, std = out["depth_median_lidar"].view(-1).double() * to_m, out["depth_std_lidar"].view(-1).double() * to_m
    t_near, t_far = (torch.from_numpy(a.reshape(-1)).to(dev).double() for a in (first, behind))
    sees_both = (t_near > 0) & (t_far > 0) & (t_near < t_far - 5.0)
    share = (w * (z < 0.5 * (t_near + t_far)[:, None])).sum(1) / w.sum(1).clamp(min=1e-9)
    edge = sees_both & (share > 0.3) & (share < 0.7)
    assert int(edge.sum()) >= 8, int(edge.sum())
    step = float(S.LIDAR_MAX_DEPTH - S.MIN_NEAR) / T * to_m
    tol = 0.75 + step
    on_face = lambda r: ((r >= t_near - step) & (r <= t_near + tol)) | ((r >= t_far - step) & (r <= t_far + tol))
    assert bool(on_face(median)[edge].all())
    assert not bool(on_face(mean)[edge].any())
    assert float(torch.minimum((mean - t_near).abs(), (mean - t_far).abs())[edge].min()) > 3.0  # metres from either surface
    solid = sees_both & (share > 0.99)  # rays through the body of the near box: every statistic agrees there, and the spread is small
    assert int(solid.sum()) > 100 and bool(on_face(median)[solid].all()) and bool(on_face(mean)[solid].all())
    # two masses s and 1 - s a distance `sep` apart have the spread sep sqrt(s (1 - s)); each mass is itself at most ~0.3 m deep
    sep = t_far - t_near
    assert bool((std[edge] >= sep[edge] * (0.3 * 0.7) ** 0.5 - 0.3).all()) and float(std[edge].min()) > 5.0
    assert bool((std[solid] <= sep[solid] * (0.01 * 0.99) ** 0.5 + 0.3).all()) and float(std[solid].max()) < 2.5
    print(f"two boxes: {int(edge.sum())} edge rays; mean is {float((mean - t_near)[edge].mean()):.2f} m behind the near face on average, "
          f"median within {float(torch.minimum((median - t_near).abs(), (median - t_far).abs())[edge].max()):.2f} m of a face")


def test_export_frames_builds_its_clouds_from_the_median_plane(dev, tmp_path):
    """export_frames forwards the keyword to test_step: the range plane and both clouds are the median's."""
    import test_export_gpu as E
    from test_formats_cpu import make_dataset
    from nvsf.nerf import export as X
    from nvsf.nerf.dataset import formats as F
    from nvsf.nerf.evaluate import eval_step, test_step
    root = str(tmp_path / "scene")
    seq, *_ = make_dataset(root, n_frames=2, H=6, W=8, Hl=6, Wl=32)
    m = E._model(dev)
    fs = F.FrameSet(root, seq, "train", 0.01, device=dev, training=False)
    data = fs.collate([0])
    thres = float(test_step(m, data, 32)[2].median())
    mean = test_step(m, data, 32, raydrop_thres=thres)
    med = test_step(m, data, 32, raydrop_thres=thres, depth_mode="median")
    for k in (0, 2, 3):
        assert torch.equal(mean[k], med[k])
    assert not torch.equal(mean[4], med[4]) and not torch.equal(mean[1], med[1])  # the LiDAR range plane and the camera depth plane
    ev = eval_step(m, data, 32, raydrop_thres=thres, depth_mode="median")
    assert torch.equal(ev["pred_depth"], med[4])
    out_dir = str(tmp_path / "out")
    counts = X.export_frames(m, fs, out_dir, "run", 32, raydrop_thres=thres, indices=[0], depth_mode="median")
    assert counts == X.export_frames(m, fs, out_dir + "_none", "run", 32, raydrop_thres=thres, indices=[0], depth_mode="median", write=False)
    depth = med[4][0].contiguous()
    lidar, world = X.pano_to_cloud(depth, X.quantize_u8(med[3][0].contiguous()).float(), data["poses_lidar"][0], fs.scale, fs.offset,
                                   fs.intrinsics_lidar, fs.intrinsics_hoz_lidar)
    assert counts == [int((depth != 0).sum())] and 0 < counts[0] < 6 * 32
    back = np.loadtxt(X.frame_paths(out_dir, "run", 0)["pcd_lidar"], ndmin=2)
    assert back.shape == (counts[0], 4) and np.abs(back - lidar.cpu().numpy()).max() <= 5e-7 + 1e-12
    lidar_mean, _ = X.pano_to_cloud(mean[4][0].contiguous(), X.quantize_u8(mean[3][0].contiguous()).float(), data["poses_lidar"][0], fs.scale,
                                    fs.offset, fs.intrinsics_lidar, fs.intrinsics_hoz_lidar)
    assert lidar_mean.shape != lidar.shape or np.abs(back - lidar_mean.cpu().numpy()).max() > 1e-4
