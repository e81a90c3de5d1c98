"""GPU: every parameter gradient of the occupancy-grid TRAINING render against a float64 restatement (torch_f64_static.render_packed).

The third training path -- NeRFRenderer.run_cuda in training mode: march_rays_train -> density / color on the packed samples ->
composite_rays_train (BASELINE config 3) -- composes the backward kernels of the uniform render differently: arbitrary row counts
padded to a multiple of 128 with all-zero rows, direction encodings per sample, DensityFn without a rows-per-ray hint,
sigma * density_scale in torch, the LiDAR image padded to three channels, a compositor that drops grad_depth and terminates a ray at
T_thresh.  Each case renders a small NeRFNetworkStatic with an occupancy grid through model.render in train() mode, back-propagates
    scale * (sum c_ws ws + sum c_dp depth + sum c_img image)
with fixed random coefficients, and compares the table, sigma_net and head gradients element by element with autograd of the fp64
restatement.  The restatement takes the marcher's outputs (xyzs, dirs, deltas, rays: pinned bit for bit to the oracle in
test_raymarching_gpu.py) and nothing else, and its functional OMITS the depth term: agreement also proves that grad_depth is dropped,
as the reference drops it.

Borderline rays: a ray whose outgoing transmittance comes within 1e-3 (relative) of T_thresh at some sample may stop one sample
apart in fp32 and fp64.  Such rays (decided by the restatement alone) get all three coefficients set to zero on both sides and stay
out of the forward gate; their number is capped at max(1, N // 16) and asserted.

The bar is test_static_grad_f64_gpu.py's (RTOL / ATOL / ATOL_TABLE, imported), with its justification: the backward runs the same
MLP, head and scatter kernels with the same count of at most six fp16 hand-overs on the deepest path; the compositor and
density_scale are fp32 (relative 2^-24 per operation: nothing against 6u).

Measured on an MI355X, largest |g - g64| / bar (table, sigma_net, heads; the test prints them):
    camera_L16F2_boxes              0.047  0.023  0.017          lidar_L16F2_boxes               0.102  0.035  0.021 0.010
    camera_L8F4_dense_three_rounds  0.045  0.050  0.009          lidar_L8F4_dense_edges          0.044  0.051  0.034 0.041
    camera_L16F2_no_termination     0.039  0.039  0.012          lidar_L16F2_half                0.058  0.027  0.012 0.016
    camera_L16F2_budget             0.098  0.017  0.005          camera_L16F2_chain_two_hidden   0.075  0.041  0.025

Found by lidar_L8F4_dense_edges: its table gradient was 75.6 x the bar (-0.0371 where fp64 has -0.0002).  composite_rays_train's
backward took the colour that remains behind a sample as (final image - running sum), with the final image from the forward's lane
sums and the running sum from its own scan: behind the last live sample that difference is a rounding residue of a few ulps instead
of 0, and trunc_exp's backward multiplies it by up to e^15 on exactly the saturating samples that end a ray.  The kernel now uses 0
(and T_after for 1 - weights_sum) where nothing can lie behind a sample; the figures above are with that fix.
"""
import numpy as np
import pytest
import torch

import torch_f64_static as R
from test_static_grad_f64_gpu import ATOL, ATOL_TABLE, RTOL, SCALE, _compare, _model  # noqa: F401  (the bar and the model builder of the uniform render's file)

pytestmark = pytest.mark.gpu

N_RAYS = 37
BORDER = 1e-3  # |T_{i+1} / T_thresh - 1| below which fp32 and fp64 may stop one sample apart
BG = [0.25, 0.5, 0.75]

# id: (lidar, grid, bit field, max_steps, T_thresh, options)
#   density_scale: NeRFRenderer.density_scale (applied in torch by _packed_field; 1 would hide a factor applied twice)
#   seed: added to the id's checksum -- chosen on the CPU (oracle marcher + the restatement) so that the case's own conditions hold
#         and the restatement's borderline rays stay under the cap
CASES = {
    "camera_L16F2_boxes": (False, "L16F2", "boxes", 128, 1e-4, {"perturb": True, "density_scale": 1.5, "seed": 2}),
    "lidar_L16F2_boxes": (True, "L16F2", "boxes", 128, 1e-4, {"density_scale": 16.0, "seed": 2}),
    "camera_L8F4_dense_three_rounds": (False, "L8F4", "dense", 200, 1e-4, {"density_scale": 2.0, "sigma_gain": 8.0}),
    "lidar_L8F4_dense_edges": (True, "L8F4", "dense", 200, 1e-4, {"edges": True, "scale": 1.0}),
    "camera_L16F2_no_termination": (False, "L16F2", "boxes", 128, 0.0, {"dt_gamma": 1.0 / 128, "density_scale": 2.0, "seed": 1}),
    "lidar_L16F2_half": (True, "L16F2", "dense", 96, 0.5, {"density_scale": 2.5, "seed": 1}),
    "camera_L16F2_budget": (False, "L16F2", "dense", 128, 1e-4, {"budget": True, "density_scale": 1.5}),
    "camera_L16F2_chain_two_hidden": (False, "L16F2", "boxes", 128, 1e-4, {"num_layers_sigma": 3, "density_fn": "chain", "density_scale": 10.0}),
}


def _seed(case):
    return sum(map(ord, case)) + CASES[case][5].get("seed", 0)


def _scene(case, dev):
    """-> model (occupancy grid enabled, bit field installed), rays_o, rays_d [N, 3] on `dev`."""
    from nvsf import synthetic as S
    lidar, grid, field, max_steps, T_thresh, opts = CASES[case]
    seed = _seed(case)
    m = _model(dev, grid, lidar, opts, seed)
    if "sigma_gain" in opts:  # the density row of the output layer: spreads the logits, so that rays of one batch stop in different rounds
        with torch.no_grad():
            m.sigma_net.spec.split(m.sigma_net.params)[-1][0] *= float(opts["sigma_gain"])
    m.density_scale = float(opts.get("density_scale", 1.0))
    m = m.to(dev).enable_occupancy_grid().to(dev)
    rng = np.random.default_rng(seed)
    if field == "boxes":
        g = torch.from_numpy(S.boxes_density_grid(rng, cascades=m.cascade, H=m.grid_size, n_boxes=int(opts.get("n_boxes", 128))))
    else:
        g = torch.ones(m.cascade, m.grid_size ** 3)
    m.set_density_grid(g.to(dev), thresh=0.5)
    o, d = (S.lidar_rays if lidar else S.camera_rays)(N_RAYS, rng)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    return m, t(o), t(d)


def _coefficients(case, C, dev):
    gen = torch.Generator().manual_seed(_seed(case) + 1)
    return [torch.randn(N_RAYS, generator=gen).to(dev), torch.randn(N_RAYS, generator=gen).to(dev), torch.randn(N_RAYS, C, generator=gen).to(dev)]


def _render(m, o, d, case, **extra):
    """model.render in train() mode -> (weights_sum [N], depth [N], image [N, C]) and what march_rays_train handed on."""
    from nvsf.nerf.raymarching import raymarching
    lidar, _, _, max_steps, T_thresh, opts = CASES[case]
    m.train()
    marched, real = [], raymarching.march_rays_train

    def spy(*args):
        out = real(*args)
        marched.append(tuple(t.detach() for t in out))
        return out

    raymarching.march_rays_train = spy
    try:
        out = m.render(o[None], d[None], torch.tensor([[0.5]], device=o.device), cal_lidar_color=lidar, perturb=bool(opts.get("perturb", False)),
                       max_steps=max_steps, T_thresh=T_thresh, dt_gamma=float(opts.get("dt_gamma", 0.0)),
                       bg_color=None if lidar else torch.tensor(BG, device=o.device), **extra)
    finally:
        raymarching.march_rays_train = real
    sfx = "_lidar" if lidar else ""
    (xyzs, dirs, deltas, rays), = marched
    return (out["weights_sum" + sfx], out["depth" + sfx].view(-1), out["image" + sfx].view(o.shape[0], -1)), (xyzs, dirs, deltas, rays)


def _conditions(case, rays, M, stop, logits, ws64):
    """What each case exists for, asserted with the observed values (all from the marcher's rows and the restatement)."""
    _, _, field, _, _, opts = CASES[case]
    off, cnt = rays[:, 1].long(), rays[:, 2].long()
    if field == "boxes":
        n_empty, n_short = int((cnt == 0).sum()), int(((cnt > 0) & (cnt < 64)).sum())
        assert n_empty > 0 and n_short > 0, f"{case}: {n_empty} rays without samples, {n_short} with 0 < count < 64"
    if case == "camera_L8F4_dense_three_rounds":
        third = int(((cnt > 128) & (stop >= 128)).sum())
        second = int(((stop >= 64) & (stop < 128) & (stop < cnt - 1)).sum())
        assert third > 0 and second > 0, f"{case}: {third} rays live in the third round, {second} stopped early in the second (counts up to {int(cnt.max())})"
    if case == "lidar_L16F2_half":
        early = int(((cnt > 0) & (stop < cnt - 1)).sum())
        assert 2 * early > N_RAYS, f"{case}: {early} of {N_RAYS} rays stop early"
    if opts.get("budget"):
        over = int((off + cnt > M).sum())
        assert 0 < over < N_RAYS, f"{case}: {over} rays past the budget of {M} rows"
    if opts.get("edges"):
        hi, lo, top = int((logits > 15).sum()), int((logits < -15).sum()), float(ws64.max())
        assert hi > 0 and lo > 0 and top > 1 - 1e-6, f"{case}: {hi} logits > 15, {lo} < -15, max weights_sum {top!r}"


@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
def test_occupancy_training_gradients_against_fp64(dev, variants, case):
    from nvsf.nerf.raymarching import raymarching
    lidar, grid, field, max_steps, T_thresh, opts = CASES[case]
    seed = _seed(case)
    m, o, d = _scene(case, dev)
    assert m.cuda_ray and float(m.density_scale) == float(opts.get("density_scale", 1.0))
    if "density_fn" in opts:
        variants.set(density_fn=opts["density_fn"])
    scale = float(opts.get("scale", SCALE))
    C = 2 if lidar else 3
    coef = _coefficients(case, C, dev)
    enc = m.hash_encoder_lidar if lidar else m.hash_encoder_camera
    params = {"table": enc.params, "sigma_net": m.sigma_net.params}
    params.update({"raydrop_net": m.raydrop_net.params, "intensity_net": m.intensity_net.params} if lidar else {"color_net": m.color_net.params})

    extra = {}
    if opts.get("budget"):
        # the budgeted marcher path (mean_count > 0 without force_all_rays: no host read-back, rays past the budget recorded but
        # empty): about half of what the batch needs, taken from a render that reads its counter back
        with torch.no_grad():
            _render(m, o, d, case, force_all_rays=True)
        total = int(m.step_counter[(m.local_step - 1) % 16, 0])
        assert total > 256, total
        m.mean_count = total // 2
        extra["force_all_rays"] = False
    torch.manual_seed(seed + 2)
    (ws, depth, image), (xyzs, dirs, deltas, rays) = _render(m, o, d, case, **extra)
    M = xyzs.shape[0]
    assert M % 128 == 0 and M <= 7424 and rays.shape[0] == N_RAYS, (M, rays.shape)
    if opts.get("budget"):
        raymarching.check_march_status(wait=True)  # must not raise: the launch completed, the dropped rays are no failure
        assert M == m.mean_count + (128 - m.mean_count % 128)
        dropped = rays[(rays[:, 1] + rays[:, 2]) > M, 0].long()
        assert float(ws[dropped].abs().max()) == 0.0 and float(depth[dropped].abs().max()) == 0.0
        assert torch.equal(image[dropped], torch.tensor(BG, device=dev).expand(dropped.numel(), 3))

    p64 = R.leaves(m, lidar)
    ref = R.render_packed(m, p64, xyzs, dirs, deltas, rays, lidar, T_thresh, BG)
    stop, margin = ref["stop"], ref["margin"]
    _conditions(case, rays, M, stop, ref["logits"].detach(), ref["weights_sum"].detach())
    border = torch.zeros(N_RAYS, dtype=torch.bool, device=dev)
    border[rays[:, 0].long()] = margin < BORDER
    n_border = int(border.sum())
    assert n_border <= max(1, N_RAYS // 16), f"{case}: {n_border} borderline rays (margins {sorted(margin.tolist())[:4]})"
    keep = ~border
    # the restatement renders what the kernels rendered: else the gradient comparison below would mean nothing
    for name, a, b in (("weights_sum", ws, ref["weights_sum"]), ("image", image, ref["image"])):
        err = float((a.double() - b.detach())[keep].abs().max())
        assert err <= 1e-4, f"{case}: {name} differs from the restatement by {err:.3g}"
    dmax = float(ref["depth"].detach().abs().max().clamp(min=1.0))
    err = float((depth.double() - ref["depth"].detach())[keep].abs().max())
    assert err <= 1e-4 * dmax, f"{case}: depth differs from the restatement by {err:.3g} (max depth {dmax:.3g})"

    coef = [torch.where(border.view(-1, *[1] * (c.dim() - 1)), torch.zeros_like(c), c) for c in coef]
    for p in m.parameters():
        p.grad = None
    ((ws * coef[0]).sum() + (depth * coef[1]).sum() + (image * coef[2]).sum()).mul(scale).backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.clone() for k, p in params.items()}
    # the restatement's functional has NO depth term (the production one does, with non-zero coefficients)
    assert float(coef[1].abs().max()) > 0
    ((ref["weights_sum"] * coef[0].double()).sum() + (ref["image"] * coef[2].double()).sum()).mul(scale).backward()
    ref_grads = {"table": p64["hash_encoder_lidar" if lidar else "hash_encoder_camera"].grad, "sigma_net": p64["sigma_net"].grad}
    ref_grads.update({k: p64[k].grad for k in params if k not in ("table", "sigma_net")})
    # live rows: samples 0..stop of the rays that are neither empty nor borderline -- the only rows a gradient may come from
    live = torch.zeros(M, dtype=torch.bool, device=dev)
    for (ray_id, off, cnt), s in zip(rays.tolist(), stop.tolist()):
        if s >= 0 and not bool(border[ray_id]):
            live[off:off + s + 1] = True
    assert int(live.sum()) > 0
    touched = R.touched_entries(ref["x01"][live], enc.spec)
    report = []
    for k, g in grads.items():
        worst = _compare(k, g, ref_grads[k], *((enc.spec, touched) if k == "table" else ()))
        report.append(f"{k} {worst:.3f}")
    cnt = rays[:, 2]
    print(f"{case}: M {M}, counts up to {int(cnt.max())}, stops up to {int(stop.max())}, {int((stop < cnt - 1).sum())} rays stop early, "
          f"{n_border} borderline; largest |g - g64| / bar: " + ", ".join(report))
