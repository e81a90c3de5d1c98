"""GPU: hierarchical importance resampling of the uniform ray render (csrc/resample.hip).

  1. nvsf_sample_pdf against the float64 restatement (tests/resample_oracle.py) and against the reference's fp32 samples
     (tests/golden/resample.npz);
  2. nvsf_resample_merge against the restatement at the shapes where it can go wrong, with the special rays inside a batch;
  3. MergeRowsFn against torch.gather, forward and backward, bit for bit;
  4. run(hierarchical=True) on NeRFNetworkStatic: outputs and parameter gradients against tests/torch_f64_static.render, at the bars
     of tests/test_static_grad_f64_gpu.py (the merged render runs those kernels plus copies);
  5. the space-time model: run(hierarchical=True) equals the chain composed by hand from the public ops, bit for bit;
  6. it does what it is for: on an analytic thin shell the resampled render's range error is a fraction of the even render's at the
     same sample count;
  7. RenderTrainStep(upsample_steps=16): the loss falls, gradients reach table entries only resampled positions touch.
"""
import copy
import os

import numpy as np
import pytest
import torch

import resample_oracle as RO
import torch_f64_static as R
import test_static_grad_f64_gpu as G
from test_resample_cpu import CASES as FIXTURE_CASES, GOLD, fixture_case

pytestmark = pytest.mark.gpu


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("det", [True, False], ids=["det", "rand"])
@pytest.mark.parametrize("c", range(len(FIXTURE_CASES)), ids=[f"nw{a}_U{b}" for a, b in FIXTURE_CASES])
def test_sample_pdf_against_oracle_and_reference(dev, c, det):
    from nvsf import field_ops as ops
    from nvsf.nerf.models.renderer_dynamic import sample_pdf
    bins, w, u, ref, width = fixture_case(np.load(GOLD), c, det)
    got = ops.sample_pdf(_t(bins, dev), _t(w, dev), _t(u, dev)).cpu().numpy()
    want = RO.sample_pdf(bins, w, u).astype(np.float32)
    ok, left_out, worst = RO.close_or_excused(got, want, width)
    far, share = RO.reference_conditions(got, ref, width)
    print(f"{FIXTURE_CASES[c]} det={det}: {left_out} of {got.size} beyond 2 ulp of the oracle (worst {worst:.3g} bin widths); against the "
          f"reference: largest difference {far:.3g} bin widths, share beyond 0.01 bin width {share:.3g}")
    assert ok, (left_out, worst)
    assert far <= 1.0 and share <= 1e-3
    # the module-level function with the reference's signature: the same launch
    U = FIXTURE_CASES[c][1]
    if det:
        assert np.array_equal(sample_pdf(_t(bins, dev), _t(w, dev), U, det=True).cpu().numpy(), got)
    else:
        assert np.array_equal(sample_pdf(_t(bins, dev), _t(w, dev), U, u=_t(u, dev)).cpu().numpy(), got)
        torch.manual_seed(5)
        drawn = sample_pdf(_t(bins, dev), _t(w, dev), U)
        torch.manual_seed(5)
        assert torch.equal(drawn, ops.sample_pdf(_t(bins, dev), _t(w, dev), torch.rand(64, U, dtype=torch.float32, device=dev)))


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
MERGE_SHAPES = ((3, 1, False), (3, 5, False), (67, 64, False), (64, 65, True), (130, 128, True), (768, 128, False), (1024, 256, True))
ZERO, ONE_HOT, BROKEN, PLATEAU = 0, 1, 2, 3  # the special rays of a batch of at least five


def _merge_inputs(N, T, U, per_ray, seed):
    """Synthetic LiDAR rays: perturbed linspace depths and the compositing weights of one Gaussian density bump per ray (numpy, fp32)."""
    from nvsf import synthetic as S
    rng = np.random.default_rng(seed)
    o, d = S.lidar_rays(N, rng)
    o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
    near = np.float32(S.MIN_NEAR)
    far = (near + (0.3 + 0.7 * rng.random((N, 1))) * (S.LIDAR_MAX_DEPTH - S.MIN_NEAR)).astype(np.float32)
    dist = (far - near) / np.float32(T)
    z = (near + (far - near) * np.linspace(0, 1, T, dtype=np.float32)[None] + (rng.random((N, T), dtype=np.float32) - 0.5) * dist).astype(np.float32)
    centre = near + (far - near) * rng.random((N, 1))
    width = (far - near) * (0.002 + 0.048 * rng.random((N, 1)))
    sigma = np.exp(9 * rng.random((N, 1))) * np.exp(-0.5 * ((z - centre) / width) ** 2) + 0.3 * rng.random((N, T))
    alpha = 1 - np.exp(-np.concatenate([np.diff(z, axis=-1), dist], -1) * sigma)
    trans = np.cumprod(np.concatenate([np.ones((N, 1)), 1 - alpha + 1e-15], -1), -1)[:, :-1]
    w = (alpha * trans).astype(np.float32)
    u = rng.random((N, U), dtype=np.float32) if per_ray else np.linspace(0.5 / U, 1 - 0.5 / U, U).astype(np.float32)
    k = None
    if N >= 5:
        k = 1 + (T - 2) // 2  # the one-hot weight's sample: pdf weight k - 1, the bin [mid[k-1], mid[k]] around z[k]
        w[ZERO] = 0
        w[ONE_HOT] = 0
        w[ONE_HOT, k] = 1
        w[PLATEAU] = 0
        w[PLATEAU, k] = 1e6
        z[PLATEAU, k - 1] = z[PLATEAU, k]
        if k + 1 < T:
            z[PLATEAU, k + 1] = z[PLATEAU, k]
        if per_ray:
            u[PLATEAU] = 0.01 + 0.98 * u[PLATEAU]
    aabb = np.array([-S.BOUND] * 3 + [S.BOUND] * 3, np.float32)
    return o, d, aabb, z, w, u, k


@pytest.mark.parametrize("N", [1, 5, 257])
@pytest.mark.parametrize("T,U,per_ray", MERGE_SHAPES, ids=[f"T{t}_U{u}_{'perray' if p else 'shared'}" for t, u, p in MERGE_SHAPES])
def test_resample_merge_against_oracle(dev, T, U, per_ray, N):
    from nvsf import field_ops as ops
    o, d, aabb, z, w, u, k = _merge_inputs(N, T, U, per_ray, seed=1000 * T + 10 * U + N)
    w_dev = w.copy()
    if N >= 5:
        w_dev[BROKEN, 1::3] = np.nan
        w_dev[BROKEN, 2::3] = np.inf
        w_dev[BROKEN, 1] = -1.0
    args = lambda weights: (_t(o, dev), _t(d, dev), _t(aabb, dev), _t(z, dev), _t(weights, dev), _t(u, dev))
    z_new, xyz_new, z_merged, src = ops.resample_merge(*args(w_dev))
    torch.cuda.synchronize()
    assert tuple(z_new.shape) == (N, U) and tuple(xyz_new.shape) == (N, U, 3) and tuple(z_merged.shape) == (N, T + U) and src.dtype == torch.int32
    # the positions: the clipped torch expression on the device, bit for bit
    box = _t(aabb, dev)
    want_xyz = torch.min(torch.max(_t(o, dev)[:, None, :] + _t(d, dev)[:, None, :] * z_new[:, :, None], box[:3]), box[3:])
    assert torch.equal(xyz_new, want_xyz)
    zn, zm, sr = z_new.cpu().numpy(), z_merged.cpu().numpy(), src.cpu().numpy()
    assert np.isfinite(zn).all()
    assert (np.diff(zn, axis=-1) >= 0).all() and (np.diff(zm, axis=-1) >= 0).all()
    assert (np.sort(sr, -1) == np.arange(T + U, dtype=np.int32)).all()  # a permutation on every ray
    cat = np.concatenate([z, zn], -1)
    assert np.array_equal(np.take_along_axis(cat, sr.astype(np.int64), -1).view(np.int32), zm.view(np.int32))
    tie = zm[:, 1:] == zm[:, :-1]
    assert (sr[:, 1:][tie] > sr[:, :-1][tie]).all()  # equal values: coarse before new, each in its own order
    # the oracle (it counts non-finite and negative weights as 0 itself)
    ref = RO.resample_merge(o, d, aabb, z, w_dev, u)
    mid = ref["mid"]
    width = ((mid[:, -1].astype(np.float64) - mid[:, 0]) / (T - 2))[:, None]
    ok, left_out, worst = RO.close_or_excused(zn, ref["z_new"], np.maximum(width, 1e-30))
    assert ok, ("z_new", left_out, worst)
    ok, left_out, worst = RO.close_or_excused(zm, ref["z_merged"], np.maximum(width, 1e-30))
    assert ok, ("z_merged", left_out, worst)
    same = (zn.view(np.int32) == ref["z_new"].view(np.int32)).all(-1)
    assert same.mean() >= 0.9 and np.array_equal(sr[same], ref["src"][same])  # where the depths agree bit for bit, so does the order
    assert ((zn >= mid[:, :1]) & (zn <= mid[:, -1:])).all()
    if N < 5:
        return
    # all-zero weights: the new samples are spread evenly over [mid_0, mid_last] -- the inverse of a uniform cdf at u
    lo, hi = float(mid[ZERO, 0]), float(mid[ZERO, -1])
    u_zero = np.sort(u[ZERO] if per_ray else u).astype(np.float64)
    knots = np.interp(u_zero * (T - 2), np.arange(T - 1), mid[ZERO].astype(np.float64))
    assert np.abs(zn[ZERO] - knots).max() <= 1e-5 * (hi - lo) + 2e-7 * hi
    # a one-hot weight: the draws whose u falls into its share of the cdf lie in its bin
    total = 1.0 + (T - 2) * 1e-5
    c_lo = (k - 1) * 1e-5 / total
    c_hi = c_lo + (1.0 + 1e-5) / total
    u_hot = (u[ONE_HOT] if per_ray else u).astype(np.float64)
    expected = int(((u_hot > c_lo + 1e-6) & (u_hot < c_hi - 1e-6)).sum())
    in_bin = int(((zn[ONE_HOT] >= mid[ONE_HOT, k - 1]) & (zn[ONE_HOT] <= mid[ONE_HOT, k])).sum())
    assert in_bin >= expected > 0.9 * U - 1  # the other bins hold (T - 3) 1e-5 of the mass: about 1 % at T = 1024
    # the plateau: every draw lands on the three equal coarse depths; they come first, in order, then the new ones in order
    assert (zn[PLATEAU] == z[PLATEAU, k]).all()
    first = int(np.searchsorted(zm[PLATEAU], z[PLATEAU, k], side="left"))
    n_coarse = int((z[PLATEAU] == z[PLATEAU, k]).sum())
    assert n_coarse == (3 if k + 1 < T else 2)
    assert list(sr[PLATEAU, first:first + n_coarse + U]) == list(range(k - 1, k - 1 + n_coarse)) + list(range(T, T + U))
    # NaN / inf / negative weights: finite samples inside the bins, and no other ray of the batch changes
    assert np.isfinite(zn[BROKEN]).all() and (zn[BROKEN] >= mid[BROKEN, 0]).all() and (zn[BROKEN] <= mid[BROKEN, -1]).all()
    clean = ops.resample_merge(*args(w))
    others = [i for i in range(N) if i != BROKEN]
    for a, b in zip((z_new, xyz_new, z_merged, src), clean):
        assert torch.equal(a[others], b[others])


def test_resample_entries_reject_bad_arguments(dev):
    """Status codes of the C ABI: zero sizes and null pointers are invalid arguments, sizes beyond the LDS plan are unsupported, an
    empty batch is a no-op -- nothing is launched in any of them."""
    from nvsf import _hip
    lib = _hip.load()
    buf = torch.zeros(1 << 16, device=dev)
    p, idx = buf.data_ptr(), torch.zeros(1 << 12, dtype=torch.int32, device=dev).data_ptr()
    assert lib.nvsf_sample_pdf(p, p, p, 0, 0, 8, 4, p, None) == 0
    assert lib.nvsf_sample_pdf(p, p, p, 0, 4, 1, 4, p, None) == -1
    assert lib.nvsf_sample_pdf(p, p, p, 0, 4, 8, 0, p, None) == -1
    assert lib.nvsf_sample_pdf(None, p, p, 0, 4, 8, 4, p, None) == -1
    assert lib.nvsf_sample_pdf(p, p, p, 0, 4, 1025, 4, p, None) == -2
    assert lib.nvsf_resample_merge(p, p, p, p, p, p, 0, 0, 8, 4, p, p, p, idx, None) == 0
    assert lib.nvsf_resample_merge(p, p, p, p, p, p, 0, 4, 2, 4, p, p, p, idx, None) == -1
    assert lib.nvsf_resample_merge(p, p, p, p, p, p, 0, 4, 8, 0, p, p, p, idx, None) == -1
    assert lib.nvsf_resample_merge(p, p, p, p, p, None, 0, 4, 8, 4, p, p, p, idx, None) == -1
    assert lib.nvsf_resample_merge(p, p, p, p, p, p, 0, 4, 1025, 4, p, p, p, idx, None) == -2
    assert lib.nvsf_resample_merge(p, p, p, p, p, p, 0, 4, 8, 257, p, p, p, idx, None) == -2
    assert lib.nvsf_merge_rows(p, p, idx, 0, 8, 4, 4, p, None) == 0
    assert lib.nvsf_merge_rows(p, p, idx, 4, 8, 4, 0, p, None) == -1
    assert lib.nvsf_merge_rows(p, None, idx, 4, 8, 4, 4, p, None) == -1
    assert lib.nvsf_split_rows(p, idx, 0, 8, 4, 4, p, p, None) == 0
    assert lib.nvsf_split_rows(p, None, 4, 8, 4, 4, p, p, None) == -1
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ["f32x1", "f32x3", "f16x16", "f32x15"])
def test_merge_rows_equals_gather(dev, row):
    """row_bytes 4, 12, 32 (16-byte vectors), 60: forward = torch.gather on the concatenation, backward = autograd through that gather,
    bit for bit (both directions are copies)."""
    from nvsf import field_ops as ops
    dtype, C = {"f32x1": (torch.float32, 1), "f32x3": (torch.float32, 3), "f16x16": (torch.float16, 16), "f32x15": (torch.float32, 15)}[row]
    N, T, U = 37, 67, 13
    g = torch.Generator().manual_seed(C)
    a = torch.randn(N, T, C, generator=g).to(dtype).to(dev).requires_grad_()
    b = torch.randn(N, U, C, generator=g).to(dtype).to(dev).requires_grad_()
    src = torch.stack([torch.randperm(T + U, generator=g) for _ in range(N)]).to(torch.int32).to(dev)
    cot = torch.randn(N, T + U, C, generator=g).to(dtype).to(dev)
    out = ops.MergeRowsFn.apply(a, b, src)
    assert out.dtype == dtype and tuple(out.shape) == (N, T + U, C)
    want = torch.gather(torch.cat([a, b], 1), 1, src.long()[:, :, None].expand(N, T + U, C))
    assert torch.equal(out, want)
    ga, gb = torch.autograd.grad(out, (a, b), cot)
    wa, wb = torch.autograd.grad(want, (a, b), cot)
    assert torch.equal(ga, wa) and torch.equal(gb, wb)
    # flat rows [N, T] (sigma) go through the same node
    flat = ops.MergeRowsFn.apply(a[:, :, 0].contiguous(), b[:, :, 0].contiguous(), src)
    assert torch.equal(flat, want[:, :, 0])


# ---- 4 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("perturb", [False, True], ids=["det", "perturb"])
@pytest.mark.parametrize("lidar", [True, False], ids=["lidar", "camera"])
@pytest.mark.parametrize("T,U", [(16, 16), (67, 13), (96, 32)])
def test_hierarchical_run_static_against_fp64(dev, T, U, lidar, perturb):
    """Outputs and parameter gradients of run(hierarchical=True) against the float64 restatement on the run's merged z_vals and its
    weights > W_THRESH mask, at the bars of tests/test_static_grad_f64_gpu.py (operator chain): outputs 1e-4, gradients
    |g - g64| <= atol + 4e-3 |g64| with atol = 4e-3 of the tensor's (1e-2 of the table level's) largest entry."""
    from nvsf import field_ops as ops
    N, seed = 64, 7 * T + U + 2 * lidar + perturb
    m = G._model(dev, "L16F2", lidar, {}, seed)
    o, d, _ = G._rays(lidar, N, {}, seed, dev)
    m.train()
    bg = [0.25, 0.5, 0.75]
    t = torch.tensor([[0.5]], device=dev)
    kw = dict(cal_lidar_color=lidar, num_steps=T, perturb=perturb, bg_color=None if lidar else torch.tensor(bg, device=dev))
    sfx = "_lidar" if lidar else ""
    # hierarchical=False: bit-identical to a call that omits the keyword, whatever upsample_steps says
    torch.manual_seed(seed + 2)
    plain = m.render(o[None], d[None], t, upsample_steps=U, **kw)
    torch.manual_seed(seed + 2)
    off = m.render(o[None], d[None], t, upsample_steps=U, hierarchical=False, **kw)
    assert set(plain) == set(off) and tuple(off["z_vals"].shape) == (N, T)
    for key in plain:
        assert torch.equal(plain[key], off[key]), key
    del plain, off
    for p in m.parameters():
        p.grad = None
    torch.manual_seed(seed + 2)
    out = m.render(o[None], d[None], t, upsample_steps=U, hierarchical=True, **kw)
    weights, ws, depth, image, z_vals = out["weights"], out["weights_sum" + sfx], out["depth" + sfx].view(-1), out["image" + sfx].view(N, -1), out["z_vals"]
    assert tuple(weights.shape) == tuple(z_vals.shape) == (N, T + U)
    assert bool((z_vals[:, 1:] >= z_vals[:, :-1]).all())
    C = 2 if lidar else 3
    gen = torch.Generator().manual_seed(seed + 1)
    coef = [c.to(dev) for c in (torch.randn(N, T + U, generator=gen), torch.randn(N, generator=gen), torch.randn(N, generator=gen),
                                torch.randn(N, C, generator=gen))]
    G._backward((weights, ws, depth, image), coef, None, G.SCALE)
    torch.cuda.synchronize()
    enc = m.hash_encoder_lidar if lidar else m.hash_encoder_camera
    params = {"table": enc.params, "sigma_net": m.sigma_net.params}
    params.update({"raydrop_net": m.raydrop_net.params, "intensity_net": m.intensity_net.params} if lidar else {"color_net": m.color_net.params})
    grads = {k: p.grad.clone() for k, p in params.items()}
    mask = weights.detach() > ops.W_THRESH
    nears, fars = m._near_far(o, d, lidar, m.aabb_train)
    p64 = R.leaves(m, lidar)
    ref = R.render(m, p64, o, d, nears, fars, z_vals.detach(), mask, lidar, bg)
    report = []
    for name, a, b in (("weights", weights, ref["weights"]), ("weights_sum", ws, ref["weights_sum"]), ("image", image, ref["image"])):
        err = float((a.detach().double() - b.detach()).abs().max())
        report.append(f"{name} {err:.2e}")
        assert err <= 1e-4, (name, err)
    dmax = float(ref["depth"].detach().abs().max().clamp(min=1.0))
    err = float((depth.detach().double() - ref["depth"].detach()).abs().max())
    report.append(f"depth {err:.2e}")
    assert err <= 1e-4 * dmax
    border = int(((ref["weights"].detach() > ops.W_THRESH) != mask).sum())
    assert border <= max(2, mask.numel() // 1000), border
    loss64 = sum((a * c.double()).sum() for a, c in zip((ref["weights"], ref["weights_sum"], ref["depth"], ref["image"]), coef)) * G.SCALE
    loss64.backward()
    ref_grads = {"table": p64["hash_encoder_lidar" if lidar else "hash_encoder_camera"].grad, "sigma_net": p64["sigma_net"].grad}
    ref_grads.update({k: p64[k].grad for k in params if k not in ("table", "sigma_net")})
    touched = R.touched_entries(ref["x01"], enc.spec)
    for k, g in grads.items():
        worst = G._compare(k, g, ref_grads[k], *((enc.spec, touched) if k == "table" else ()))
        report.append(f"{k} {worst:.3f}")
    print(f"T={T} U={U} lidar={lidar} perturb={perturb}: output errors and largest |g - g64| / bar: " + ", ".join(report))


# ---- 5 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lidar", [True, False], ids=["lidar", "camera"])
def test_hierarchical_run_dynamic_equals_hand_composed_chain(dev, lidar):
    from nvsf import field_ops as ops
    from nvsf import synthetic as S
    from nvsf.nerf.models.network_dynamic import NeRFNetwork
    torch.manual_seed(4)
    base = NeRFNetwork(time_resolution=4, num_frames=16, bound=2.0, min_resolution=16, base_resolution=32, max_resolution=512,
                       log2_hashmap_size=13, min_near=S.MIN_NEAR, min_near_lidar=S.MIN_NEAR, lidar_max_depth=S.LIDAR_MAX_DEPTH).to(dev)
    with torch.no_grad():
        for n_, p in base.named_parameters():
            if "hash" in n_ and p.numel() > 1000:
                p.uniform_(-0.5, 0.5)
    N, T, U = 32, 32, 16
    rng = np.random.default_rng(2)
    o, d = (S.lidar_rays if lidar else S.camera_rays)(N, rng)
    o, d = _t(np.asarray(o, np.float32), dev), _t(np.asarray(d, np.float32), dev)
    time = torch.tensor([[0.375]], device=dev)
    sfx = "_lidar" if lidar else ""
    for grad in (False, True):
        with torch.set_grad_enabled(grad):
            m = copy.deepcopy(base).train(grad)
            torch.manual_seed(9)
            out = m.run(o[None], d[None], time, cal_lidar_color=lidar, num_steps=T, upsample_steps=U, perturb=grad, hierarchical=True)
            # the same chain from the public ops
            m = copy.deepcopy(base).train(grad)
            m.out_dim = m.out_lidar_color_dim if lidar else m.out_color_dim
            torch.manual_seed(9)
            aabb = m.aabb_train if m.training else m.aabb_infer
            nears, fars = m._near_far(o, d, lidar, aabb)
            noise = torch.rand(N, T, dtype=torch.float32, device=dev) if grad else None
            u = torch.rand(N, U, dtype=torch.float32, device=dev) if grad else ops.stratified_u(U, dev)
            z, xyz = ops.uniform_samples(o, d, nears, fars, T, aabb, noise)
            with m._rows_hint().rows(T):
                coarse = m.density(xyz.view(-1, 3), time, lidar)
            with torch.no_grad():
                w0 = ops.CompositeWeightsFn.apply(coarse["sigma"].detach().view(N, T), z, nears, fars, m._k_scale())[0]
            z_new, xyz_new, z_merged, src = ops.resample_merge(o, d, aabb, z, w0, u)
            with m._rows_hint().rows(U):
                fine = m.density(xyz_new.view(-1, 3), time, lidar)
            sigma = ops.MergeRowsFn.apply(coarse["sigma"].reshape(N, T, -1), fine["sigma"].reshape(N, U, -1), src).view(N, T + U)
            geo = ops.MergeRowsFn.apply(coarse["geo_feat"].reshape(N, T, -1), fine["geo_feat"].reshape(N, U, -1), src).view(N * (T + U), -1)
            pos = ops.MergeRowsFn.apply(xyz, xyz_new, src).view(-1, 3)
            weights, ws, depth = ops.CompositeWeightsFn.apply(sigma, z_merged, nears, fars, m._k_scale())
            rgbs = m.color(pos, d.view(-1, 1, 3).expand(N, T + U, 3).reshape(-1, 3), cal_lidar_color=lidar,
                           mask=(weights > ops.W_THRESH).reshape(-1), ray_dirs=d, geo_feat=geo)
            bg = None if lidar else ops.device_constant([1.0] * 3, dev)
            image = ops.CompositeImageFn.apply(weights, rgbs.view(N, T + U, m.out_dim), ws, bg)
        assert torch.equal(out["z_vals"], z_merged) and torch.equal(out["weights"], weights) and torch.equal(out["weights_sum" + sfx], ws)
        assert torch.equal(out["depth" + sfx].view(-1), depth) and torch.equal(out["image" + sfx].view(N, -1), image)
        assert bool(torch.isfinite(image).all()) and float(ws.detach().max()) > 0
        assert out["weights"].requires_grad == grad


# ---- 6 -------------------------------------------------------------------------------------------------------------------------
def _shell_field(dev, spacing, radius=0.5):
    """An analytic field on NeRFRenderer: density a Gaussian shell around the origin (standard deviation half of `spacing`, peak
    40 / spacing), colour a constant."""
    from nvsf import synthetic as S
    from nvsf.nerf.models.renderer_dynamic import NeRFRenderer

    class Shell(NeRFRenderer):
        def __init__(self):
            super().__init__(bound=S.BOUND, min_near=S.MIN_NEAR, min_near_lidar=S.MIN_NEAR, lidar_max_depth=S.LIDAR_MAX_DEPTH)
            self.out_color_dim, self.out_lidar_color_dim = 3, 2

        def density(self, x, t=None, cal_lidar_color=False, **kwargs):
            r = x.norm(dim=-1)
            sigma = (40.0 / spacing) * torch.exp(-0.5 * ((r - radius) / (0.5 * spacing)) ** 2)
            return {"sigma": sigma, "geo_feat": torch.zeros(x.shape[0], 1, device=x.device)}

        def color(self, x, d, cal_lidar_color=False, mask=None, **kwargs):
            return torch.full((x.shape[0], self.out_dim), 0.5, device=x.device)
    return Shell().to(dev).eval()


@pytest.mark.parametrize("T,U,bar", [(192, 64, 1.0 / 3.0), (64, 64, 0.5)])
def test_resampling_sharpens_the_range_of_a_thin_surface(dev, T, U, bar):
    """1024 LiDAR rays through a shell half a coarse spacing thick, from origins jittered by a few coarse spacings; truth: 16384 even
    samples through the same operator chain.  The mean absolute range error of T coarse + U resampled samples is at most `bar` times
    that of T + U even samples (a float64 simulation of the compositing gives 1/7 at (192, 64) and about 1/3 at (64, 64))."""
    from nvsf import synthetic as S
    N = 1024
    spacing = float(S.LIDAR_MAX_DEPTH - S.MIN_NEAR) / T
    m = _shell_field(dev, spacing)
    g = torch.Generator().manual_seed(T)
    d = torch.randn(N, 3, generator=g)
    d = (d / d.norm(dim=-1, keepdim=True)).to(dev)
    o = ((torch.rand(N, 3, generator=g) * 2 - 1) * 3 * spacing).to(dev)
    t = torch.tensor([[0.5]], device=dev)
    with torch.no_grad():
        depth = lambda **kw: m.run(o[None], d[None], t, cal_lidar_color=True, perturb=False, **kw)["depth_lidar"].view(-1).double()
        truth = depth(num_steps=16384)
        even = float((depth(num_steps=T + U) - truth).abs().mean())
        hier = float((depth(num_steps=T, upsample_steps=U, hierarchical=True) - truth).abs().mean())
    assert 0.3 < float(truth.mean()) < 0.7  # the rays do cross the shell
    print(f"(T, U) = ({T}, {U}): mean |range error| even {even / spacing:.4f}, resampled {hier / spacing:.4f} coarse spacings, ratio {hier / even:.3f}")
    assert hier <= bar * even, (hier, even)


# ---- 7 -------------------------------------------------------------------------------------------------------------------------
def test_train_step_with_upsample_steps(dev):
    from nvsf import field_ops as ops
    from nvsf import synthetic as S
    from nvsf.nerf.loss_scaler import LossScaler
    from nvsf.nerf.models.network_static import NeRFNetworkStatic
    from nvsf.nerf.train_step import RenderTrainStep
    from test_train_step_gpu import _batch
    kw = dict(bound=S.BOUND, min_near=S.MIN_NEAR, min_near_lidar=S.MIN_NEAR, lidar_max_depth=S.LIDAR_MAX_DEPTH, log2_hashmap_size=14)
    torch.manual_seed(1)
    teacher = NeRFNetworkStatic(**kw)
    with torch.no_grad():
        g = torch.Generator().manual_seed(7)
        for enc in (teacher.hash_encoder_lidar, teacher.hash_encoder_camera):
            enc.params.copy_(torch.randn(enc.params.shape, generator=g) * 0.2)
    teacher = teacher.to(dev).eval()
    m = NeRFNetworkStatic(**kw).to(dev)
    T, U = 32, 16
    step = RenderTrainStep(m, lr=1e-2, iters=100, num_steps=T, upsample_steps=U, use_urf_loss=True, scale=S.SCALE, ema_decay=None)
    step.scaler = LossScaler(init_scale=64.0, growth_interval=10 ** 6)
    batch = _batch(S, teacher, dev, n=256, T=T)
    calls, real = [], ops.resample_merge

    def recording(rays_o, rays_d, aabb, z_vals, weights, u):
        out = real(rays_o, rays_d, aabb, z_vals, weights, u)
        calls.append(tuple(a.detach().cpu().numpy() for a in (rays_o, rays_d, aabb, z_vals, weights, u, out[0])))
        return out
    ops.resample_merge = recording
    try:
        torch.manual_seed(10)
        loss, parts, _ = step.forward_backward(batch)
    finally:
        ops.resample_merge = real
    torch.cuda.synchronize()
    ops.sync_side_streams()
    assert bool(torch.isfinite(loss)) and "los" in parts and bool(torch.isfinite(parts["los"]))
    assert len(calls) == 2  # both modalities render hierarchically
    for lidar, enc in ((True, m.hash_encoder_lidar), (False, m.hash_encoder_camera)):
        o = batch["rays_o_lidar" if lidar else "rays_o"][0].cpu().numpy()
        (call,) = [c for c in calls if np.array_equal(c[0], o)]
        assert call[3].shape == (256, T) and call[5].shape == (256, U)  # perturb=True: draws per ray
        ref = RO.resample_merge(*call[:6], bound=float(S.BOUND))
        # The set is the restatement's: the entries some corner of its new positions reads and no corner of a coarse position does.
        # The device reproduces the restatement's depths to 2 ulp, not always bit for bit (test 2: at least 0.9 of the rays, hence of
        # the samples, bit for bit), and a depth an ulp away can put its position into the neighbouring cell of some level, where
        # the device reads other corners than the restatement.  Such a sample's entries are set aside; EVERY other entry of the set
        # must have a gradient.  (An entry's gradient is a sum of corner weight times feature gradient over the samples that read
        # it; this model is freshly initialised and thin, so no new sample is fully occluded or below the fp16 hand-over.)
        moved = call[6].view(np.int32) != ref["z_new"].view(np.int32)
        assert moved.mean() <= 0.1, moved.mean()
        x01 = _t(ref["x01"], dev)
        coarse = R.touched_entries(R.sample_positions(_t(call[0], dev), _t(call[1], dev), _t(call[3], dev), float(S.BOUND)), enc.spec)
        only_new = R.touched_entries(x01.reshape(-1, 3), enc.spec) & ~coarse
        aside = R.touched_entries(x01[_t(moved, dev)].reshape(-1, 3), enc.spec) if moved.any() else torch.zeros_like(only_new)
        must = only_new & ~aside
        grad = enc.params.grad
        assert int(must.sum()) > 1000
        without = int((grad[must] == 0).sum())
        print(f"{'lidar' if lidar else 'camera'} table: {int(only_new.sum())} entries touched by resampled positions only, {int((only_new & aside).sum())} "
              f"of them set aside for {int(moved.sum())} of {moved.size} depths that differ from the restatement's in the last bits, "
              f"{without} of the other {int(must.sum())} without a gradient")
        assert without == 0
    found = step.scaler.found_inf([p.grad for p in m.parameters() if p.grad is not None])
    assert float(found) == 0.0
    losses = []
    torch.manual_seed(11)
    for _ in range(3):
        loss, parts, _ = step.step(batch)
        losses.append(float(loss))
    step.sync()
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    assert float(step.scaler.get_scale()) == 64.0  # no step found an overflow
