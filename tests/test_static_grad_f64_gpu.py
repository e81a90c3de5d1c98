"""GPU: every parameter gradient of the static field's training render against a float64 restatement (tests/torch_f64_static.py).

Until this file the static model's backward was compared only with itself (the one-node render with the operator chain, the composed
density gradient with the matrix form, binned with atomic scatters), so an error shared by both sides -- in the sigmoid, head,
compositor or density-MLP backward, the trunc_exp clamp, a head tile skipped by the weight test, the level-major hand-over -- could
not show.  Here each case renders a small NeRFNetworkStatic through the production path (NeRFRenderer.run -> render_from_rays_train ->
ops.RenderRaysFn, or the chain it falls back to), back-propagates a fixed random linear functional of (weights, weights_sum, depth,
image) multiplied by a loss scale, and compares the table, sigma_net and head gradients element by element with autograd of the
same functional through the fp64 restatement.  The restatement takes only the sample depths and the weights > 1e-4 mask from the
kernels.

The bar, |g - g64| <= atol + rtol |g64|, from the arithmetic of the backward kernels:
  * every MFMA of the MLP backward reads fp16 operands: the incoming gradient rows are rounded to fp16 (relative 2^-11 = u each)
    before every layer's product.  The deepest path -- logits -> two hidden layers of a head -> geometry rows -> density MLP
    (output, one or two hidden layers) -> feature gradient -> table -- passes through at most 6 such roundings, so each addend of a
    gradient entry carries at most ~6u = 2.9e-3 of relative error (rtol 4e-3 with margin);
  * an entry that is a sum of addends of both signs can cancel: its error is bounded by 6u times the sum of the addends' magnitudes,
    not by its own value -- atol = 4e-3 of the largest entry of the tensor, the same 8u.  A table entry sums interpolation weights
    times the density MLP's input gradient, itself a 64-term sum of fp16 products over the hidden units (dX = W0^T fp16(dP0)) that
    cancels by a few times on a sample: 6u of its terms' magnitudes reaches ~3 x 6u of the level's scale, so a table's atol is
    1e-2 of the largest entry of its LEVEL (a level's entries share their magnitude; measured: 0.3 - 0.6 of that bar);
  * the fp32 atomics of the weight-gradient flushes and the table scatter add n addends with relative 2^-24 each: below 1e-5 of
    the sum for the n <= 2^18 addends here, negligible against the above;
  * the forward's own fp16 roundings are applied by the reference as the kernels apply them, so they are not part of the error;
    what remains are the rare rows where fp32 and fp64 products round a hidden activation to neighbouring fp16 values (one u on
    one addend) -- inside the bar.
One wrong ray (1/37 of a weight gradient, all of a table entry it alone touches) or one skipped head tile moves entries by far more
than 8u.  Every entry the reference has above 1e-4 of its tensor's largest must be non-zero, and a table entry no sample reads must
be exactly zero.
"""
import numpy as np
import pytest
import torch

import torch_f64_static as R

pytestmark = pytest.mark.gpu

RTOL = 4e-3
ATOL = 4e-3  # x the largest entry of the tensor
ATOL_TABLE = 1e-2  # x the largest entry of the level
SCALE = 64.0  # the loss scale the functional is multiplied with (GradScaler-like: the fp16 hand-overs carry scaled gradients)
# ... except in the "edges" cases: at densities up to e^25 a logit gradient g_sigma sigma times 64 times the MLP backward's own 128
# leaves fp16 -- a genuine overflow, which GradScaler answers by skipping the step and halving the scale -- so they run at scale 1

# id: (lidar, grid, T, N, perturb, options)
CASES = {
    "lidar_L16F2_T64_N37": (True, "L16F2", 64, 37, True, {}),
    "lidar_L16F2_T16_N1": (True, "L16F2", 16, 1, False, {}),
    "lidar_L16F2_T48_N37_matrix_staged": (True, "L16F2", 48, 37, True, {"density_grad": "matrix", "mlp_bwd": "staged"}),
    "lidar_L8F4_T64_N37_edges": (True, "L8F4", 64, 37, False, {"edges": True}),
    "lidar_L16F2_T100_chain_rows": (True, "L16F2", 100, 37, True, {"heads_input": "rows"}),
    "camera_L16F2_T64_N37_miss": (False, "L16F2", 64, 37, True, {"miss": True}),
    "camera_L16F2_T768_N8_edges_wave": (False, "L16F2", 768, 8, True, {"edges": True, "miss": True, "mlp_bwd": "wave"}),
    "camera_L8F4_T64_sliced_sink": (False, "L8F4", 64, 37, True, {"density_sliced": True, "sink": True}),
    "camera_L16F2_T64_two_hidden": (False, "L16F2", 64, 37, True, {"num_layers_sigma": 3}),
    "lidar_L16F2_T64_two_hidden": (True, "L16F2", 64, 37, False, {"num_layers_sigma": 3}),
    # N T = 2^18: the binned table scatter and the level-major hand-over of the density MLP (field_ops._bin_from), and the atomic
    # scatter (table_scatter="atomic") on the same render against the same reference
    "lidar_L16F2_T512_N512_binned": (True, "L16F2", 512, 512, True, {"sink": True, "atomic_too": True}),
}


def _model(dev, grid, lidar, opts, seed):
    from nvsf import synthetic as S
    from nvsf.nerf.models.network_static import NeRFNetworkStatic
    L, F = (16, 2) if grid == "L16F2" else (8, 4)
    torch.manual_seed(seed)
    m = NeRFNetworkStatic(bound=S.BOUND, min_near=S.MIN_NEAR, min_near_lidar=S.MIN_NEAR, lidar_max_depth=S.LIDAR_MAX_DEPTH,
                          log2_hashmap_size=14, n_levels_hash=L, n_features_per_level_hash=F,
                          num_layers_sigma=opts.get("num_layers_sigma", 2))
    with torch.no_grad():
        for enc in (m.hash_encoder_lidar, m.hash_encoder_camera):
            enc.params.normal_(0.0, 0.25)
    m = m.to(dev)
    if opts.get("edges"):
        # density logits far beyond +-15 (trunc_exp's clamp) on both sides, rays whose transmittance reaches ~0 inside them and head
        # tiles whose 16 samples are all below the weight threshold behind that: the density row of the output layer scaled so that
        # the logits of random points in the box spread to +-25 (99th percentile of |h0|)
        with torch.no_grad():
            x = (torch.rand(4096, 3, generator=torch.Generator().manual_seed(seed)) * 2 - 1).to(dev) * float(m.bound)
            h0 = torch.log(m.density(x, cal_lidar_color=lidar)["sigma"].double())
            W = m.sigma_net.spec.split(m.sigma_net.params)[-1]
            W[0] -= W[0].mean()  # hidden activations are >= 0: a centred row gives logits of both signs
            h0 = torch.log(m.density(x, cal_lidar_color=lidar)["sigma"].double())
            W[0] *= 25.0 / float(h0.abs().quantile(0.99))
    return m


def _rays(lidar, N, opts, seed, dev):
    from nvsf import synthetic as S
    rng = np.random.default_rng(seed)
    o, d = (S.lidar_rays if lidar else S.camera_rays)(N, rng)
    miss = np.zeros(N, bool)
    if opts.get("miss"):
        # rays that start outside the box and point away from it (near = far = FLT_MAX: no sample has a weight), and -- at moderate
        # densities: negative steps make alpha negative and the weights grow like exp(|step| sigma) -- rays that start just inside a
        # face and leave through it (the box exit lies before min_near: near > far)
        k = max(1, N // 8)
        o[:k] = [2.5, 2.5, 2.5]
        d[:k] = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)
        miss[:k] = True
        if not opts.get("edges"):
            o[k:2 * k] = [1.9995, 0.3, -0.2]
            d[k:2 * k] = [1.0, 0.0, 0.0]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    return t(o), t(d), torch.from_numpy(miss).to(dev)


def _render(m, o, d, lidar, T, perturb, bg, ctx_route):
    from nvsf import field_ops as ops
    m.train()
    tctx = None
    if ctx_route:
        tctx = ops.TrainContext()
        for mod in m.modules():
            mod.__dict__["_train_ctx"] = tctx
        tctx.begin_step()
    out = m.render(o[None], d[None], torch.tensor([[0.5]], device=o.device), cal_lidar_color=lidar, num_steps=T, perturb=perturb,
                   bg_color=None if lidar else torch.tensor(bg, device=o.device))
    sfx = "_lidar" if lidar else ""
    return out["weights"], out["weights_sum" + sfx], out["depth" + sfx].view(-1), out["image" + sfx].view(o.shape[0], -1), out["z_vals"], tctx


def _backward(outs, coef, tctx, scale):
    from nvsf import field_ops as ops
    loss = sum((a * c).sum() for a, c in zip(outs, coef)) * scale
    if tctx is None:
        loss.backward()
        return
    tctx.overlap, tctx.sink = True, ops.LocalGradSink()
    try:
        loss.backward()
        tctx.end_pass()
        scattered = [p for p, _ in tctx.sink.side_scatters]
    finally:
        tctx.overlap, tctx.sink = False, None
        tctx.end_step()
    ops.sync_side_streams()
    assert len(scattered) == 1  # the table gradient came from the side stream into .grad, not through autograd


def _compare(name, g, g64, spec=None, touched=None):
    """-> max over the tensor of |g - g64| / (atol + rtol |g64|); asserts the bar, the non-zero pattern and finiteness.  Tables:
    `touched` = the entries the samples read (torch_f64_static.touched_entries)."""
    g, g64 = g.double().reshape(-1), g64.reshape(-1)
    assert bool(torch.isfinite(g).all()), name
    if spec is not None:  # a table: atol per level
        atol = torch.empty_like(g64)
        for l in range(spec.L):
            a, b = spec.offsets[l] * spec.F, spec.offsets[l + 1] * spec.F
            atol[a:b] = ATOL_TABLE * float(g64[a:b].abs().max())
        assert int(((g != 0) & ~touched).sum()) == 0, f"{name}: gradient in table entries no sample touched"
    else:
        atol = torch.full_like(g64, ATOL * float(g64.abs().max()))
    top = float(g64.abs().max())
    assert top > 0, name
    big = g64.abs() > 1e-4 * top
    assert bool((g[big] != 0).all()), f"{name}: zero where the reference is not ({int((g[big] == 0).sum())} entries)"
    ratio = (g - g64).abs() / (atol + RTOL * g64.abs())
    worst = float(ratio.max())
    i = int(ratio.argmax())
    assert worst <= 1.0, f"{name}: |g - g64| / bar = {worst:.3g} at {i}: {float(g[i]):.6g} vs {float(g64[i]):.6g} (max {top:.3g})"
    return worst


@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
def test_static_training_gradients_against_fp64(dev, variants, case):
    from nvsf import field_ops as ops
    lidar, grid, T, N, perturb, opts = CASES[case]
    seed = sum(map(ord, case))
    m = _model(dev, grid, lidar, opts, seed)
    o, d, miss = _rays(lidar, N, opts, seed, dev)
    for k in ("density_grad", "heads_input", "density_sliced"):
        if k in opts:
            variants.set(**{k: opts[k]})
    if "mlp_bwd" in opts:
        variants.set(mlp_bwd=opts["mlp_bwd"])
    bg = [0.25, 0.5, 0.75]
    scale = 1.0 if opts.get("edges") else SCALE
    C = 2 if lidar else 3
    gen = torch.Generator().manual_seed(seed + 1)
    coef = [torch.randn(N, T, generator=gen), torch.randn(N, generator=gen), torch.randn(N, generator=gen), torch.randn(N, C, generator=gen)]
    coef = [c.to(dev) for c in coef]
    # a missed ray's samples sit at z = FLT_MAX (the reference's sentinel, raymarching near_far_from_aabb): d depth / d weight is
    # FLT_MAX there and FLT_MAX x g x 0 is not finite in fp32 autograd -- the reference's torch graph included -- so that ray's DEPTH
    # stays out of the functional (no loss of the step ever gives a camera ray a depth gradient); its other terms stay in
    coef[2] = torch.where(miss, torch.zeros_like(coef[2]), coef[2])
    enc = m.hash_encoder_lidar if lidar else m.hash_encoder_camera
    params = {"table": enc.params, "sigma_net": m.sigma_net.params}
    params.update({"raydrop_net": m.raydrop_net.params, "intensity_net": m.intensity_net.params} if lidar else {"color_net": m.color_net.params})

    def production(atomic=False):
        for p in m.parameters():
            p.grad = None
        if atomic:
            variants.set(table_scatter="atomic")
        torch.manual_seed(seed + 2)  # same jitter every time
        weights, ws, depth, image, z_vals, tctx = _render(m, o, d, lidar, T, perturb, bg, opts.get("sink", False))
        node = type(weights.grad_fn).__name__
        _backward((weights, ws, depth, image), coef, tctx, scale)
        torch.cuda.synchronize()
        if atomic:
            variants.clear("table_scatter")
        return node, (weights.detach(), ws.detach(), depth.detach(), image.detach(), z_vals.detach()), {k: p.grad.clone() for k, p in params.items()}

    node, fwd, grads = production()
    eligible = T % 16 == 0 and opts.get("num_layers_sigma", 2) == 2
    assert (node == "RenderRaysFnBackward") == eligible, node  # the one-node training render where it applies, else the chain
    if opts.get("atomic_too"):
        assert ops._bin_from(enc.spec, N * T, T) is not None  # this size takes the binned scatter (and the level-major hand-over)
    weights, ws, depth, image, z_vals = fwd
    mask = weights > ops.W_THRESH
    nears, fars = m._near_far(o, d, lidar, m.aabb_train)
    p64 = R.leaves(m, lidar)
    ref = R.render(m, p64, o, d, nears, fars, z_vals, mask, lidar, bg)
    # the restatement renders what the kernels rendered (the oracle's bar): else the gradient comparison below would mean nothing
    for name, a, b in (("weights", weights, ref["weights"]), ("weights_sum", ws, ref["weights_sum"]), ("image", image, ref["image"])):
        assert float((a.double() - b.detach()).abs().max()) <= 1e-4, name
    dmax = float(ref["depth"].detach().abs().max().clamp(min=1.0))
    assert float((depth.double() - ref["depth"].detach()).abs().max()) <= 1e-4 * dmax
    # samples within rounding of the weight threshold, where the kernel's mask (used by the reference) and the fp64 weights disagree
    border = int(((ref["weights"].detach() > ops.W_THRESH) != mask).sum())
    assert border <= max(2, mask.numel() // 1000), border
    if opts.get("edges"):
        h0 = ref["logits"].detach()
        assert int((h0 > 15).sum()) > 0 and int((h0 < -15).sum()) > 0  # trunc_exp's clamp is exercised on both sides
        tiles = mask.view(N, T // 16, 16).any(-1)
        assert bool((tiles.any(-1) & ~tiles.all(-1)).any())            # rays with skipped head tiles beside active ones
        assert float(ref["weights_sum"].detach().max()) > 1 - 1e-6      # saturating rays
    if node == "RenderRaysFnBackward":  # the premise "positions as the kernels form them": bit for bit the node's saved rows
        assert torch.equal(R.sample_positions(o, d, z_vals, float(m.bound)), _saved_positions(m, o, d, lidar, T, perturb, bg, seed))
    loss64 = sum((a * c.double()).sum() for a, c in zip((ref["weights"], ref["weights_sum"], ref["depth"], ref["image"]), coef)) * scale
    loss64.backward()
    ref_grads = {"table": p64["hash_encoder_lidar" if lidar else "hash_encoder_camera"].grad, "sigma_net": p64["sigma_net"].grad}
    ref_grads.update({k: p64[k].grad for k in params if k not in ("table", "sigma_net")})
    touched = R.touched_entries(ref["x01"], enc.spec)
    runs = [("", grads)]
    if opts.get("atomic_too"):
        runs.append(("atomic ", production(atomic=True)[2]))
    report = []
    for tag, gs in runs:
        for k, g in gs.items():
            worst = _compare(tag + k, g, ref_grads[k], *((enc.spec, touched) if k == "table" else ()))
            report.append(f"{tag}{k} {worst:.3f}")
    print(f"{case}: {node}; largest |g - g64| / bar: " + ", ".join(report))


def _saved_positions(m, o, d, lidar, T, perturb, bg, seed):
    """The positions the one-node render saved for its backward (ops.RenderRaysFn: first saved tensor), from a fresh forward."""
    torch.manual_seed(seed + 2)
    out = _render(m, o, d, lidar, T, perturb, bg, False)
    x01 = out[0].grad_fn.saved_tensors[0].clone()
    del out
    return x01
