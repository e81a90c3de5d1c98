"""CPU tests (no GPU): pin the oracle.

  * uniform sampler / compositor restatement (oracle/field_oracle.c) against fixtures produced by the
    reference's own NeRFRenderer.run (tests/golden/renderer_uniform.npz, generator tests/golden/make_golden.py);
  * raymarching restatement (oracle/raymarching_oracle.c) against closed-form known answers and against the
    reference's importable torch compositor formulas (the compiled CUDA extension is compared with the HIP kernels on
    the GPU, tests/test_compiled_reference_gpu.py);
  * field operators against independent numpy / fp64 evaluations of the published formulas.
"""
import os

import numpy as np
import pytest
import torch

import oracle_lib as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _cases(path):
    z = np.load(os.path.join(GOLD, path))
    out = {}
    for k in z.files:
        case, name = k.split("/")
        out.setdefault(case, {})[name] = z[k]
    return out


RENDER_CASES = _cases("renderer_uniform.npz")


@pytest.mark.parametrize("name", sorted(RENDER_CASES))
def test_uniform_renderer_restatement_matches_reference(name):
    c = RENDER_CASES[name]
    o, d, T, lidar = c["rays_o"], c["rays_d"], int(c["T"]), bool(c["lidar"])
    N = o.shape[0]
    bound = float(c["bound"])
    aabb = np.array([-bound] * 3 + [bound] * 3, np.float32)
    if lidar:
        nears, fars = np.full(N, c["min_near_lidar"], np.float32), np.full(N, c["lidar_max_depth"], np.float32)
    else:
        nears, fars = O.near_far_from_aabb(o, d, aabb, float(c["min_near"]))
    lin = torch.linspace(0.0, 1.0, T).numpy()
    noise = c["noise"] if c["noise"].size else None
    z, xyz = O.uniform_samples(o, d, nears, fars, lin, noise, aabb)
    assert np.array_equal(z, c["z_vals"])  # same fp32 operations in the same order as the torch code
    if c["xyzs"].size:
        assert np.array_equal(xyz, c["xyzs"])
    k = float(c["density_scale"]) * (2.0 if bool(c["active"]) else 1.0)
    w, ws, dp = O.composite_uniform_weights(c["sigma"], z, nears, fars, k)
    np.testing.assert_allclose(w, c["weights"], atol=2e-7, rtol=2e-6)  # torch.exp (SLEEF) vs libm expf: ulp-level
    np.testing.assert_allclose(ws, c["weights_sum"], atol=2e-6, rtol=0)
    np.testing.assert_allclose(dp, c["depth"], atol=2e-6, rtol=0)
    mask = c["weights"] > 1e-4
    assert np.array_equal(mask, c["mask"])
    rgb = np.where(mask[..., None], c["rgb_full"], 0.0).astype(np.float32)
    bg = None if lidar else (c["bg"] if c["bg"].size else np.ones(3, np.float32))
    img = O.composite_uniform_image(c["weights"], rgb, c["weights_sum"], bg)
    np.testing.assert_allclose(img, c["image"], atol=2e-6, rtol=0)


def test_trunc_exp_golden():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(GOLD), "..", "selfsupervised-nvsf_amd"))
    from nvsf.nerf.activation import trunc_exp
    g = np.load(os.path.join(GOLD, "trunc_exp.npz"))
    x = torch.tensor(g["x"], requires_grad=True)
    y = trunc_exp(x)
    y.backward(torch.ones_like(y))
    assert np.array_equal(y.detach().numpy(), g["y"]) and np.array_equal(x.grad.numpy(), g["grad"])


def test_planes_restatement_matches_reference():
    """oracle_planes_fwd vs the outputs of the reference's own Planes4D (pure torch, F.grid_sample)."""
    import sys
    sys.path.insert(0, GOLD)
    import golden_dynamic as GD
    import param_init
    g = np.load(os.path.join(GOLD, "planes4d.npz"))
    res = [[8 * m, 8 * m, 8 * m, 5] for m in (1, 2, 4, 8)]
    pairs = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
    planes = []
    for s, r in enumerate(res):
        for p, (a, b) in enumerate(pairs):
            planes.append(param_init.plane_params((1, 8, r[b], r[a]), GD._seed(f"planes.{s}.{p}"), time_plane=p in (2, 4, 5)))
    st, dy = O.planes_fwd(g["xt"], planes, res, 3)
    np.testing.assert_allclose(st, g["static"], atol=1e-6, rtol=1e-5)
    np.testing.assert_allclose(dy, g["dynamic"], atol=1e-6, rtol=1e-5)
    st_only, none = O.planes_fwd(g["xt"], planes, res, 1)
    assert none is None and np.array_equal(st_only, st)


# ---- raymarching restatement: closed-form pins ------------------------------------------------------
def test_near_far_against_fp64_slab_test():
    rng = np.random.default_rng(0)
    N = 5000
    o = rng.uniform(-3, 3, (N, 3)).astype(np.float32)
    d = rng.standard_normal((N, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    aabb = np.array([-1, -1.5, -0.5, 1, 1.5, 2.0], np.float32)
    n, f = O.near_far_from_aabb(o, d, aabb, 0.05)
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    t0, t1 = (aabb[:3] - o64) / d64, (aabb[3:] - o64) / d64
    tn, tf = np.minimum(t0, t1).max(1), np.maximum(t0, t1).min(1)
    hit = tn <= tf
    clear = np.abs(tn - tf) > 1e-4  # away from grazing rays, fp32 and fp64 agree on hit / miss
    assert np.array_equal((n < 1e30)[clear], hit[clear])
    ok = hit & clear
    np.testing.assert_allclose(n[ok], np.maximum(tn[ok], 0.05), rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(f[ok], tf[ok], rtol=2e-5, atol=2e-6)
    assert np.all(n[~hit & clear] == np.finfo(np.float32).max) and np.all(f[~hit & clear] == np.finfo(np.float32).max)


def test_morton_known_answers_and_roundtrip():
    assert O.morton3D(np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [3, 0, 0], [1023, 1023, 1023], [5, 2, 7]], np.int32)).tolist() == \
        [1, 2, 4, 9, (1 << 30) - 1, int("".join(f"{(7 >> b) & 1}{(2 >> b) & 1}{(5 >> b) & 1}" for b in (2, 1, 0)), 2)]
    rng = np.random.default_rng(1)
    c = rng.integers(0, 1024, (20000, 3)).astype(np.int32)
    assert np.array_equal(O.morton3D_invert(O.morton3D(c)), c)


def test_packbits_is_numpy_little_endian_packbits():
    rng = np.random.default_rng(2)
    g = rng.standard_normal(8 * 4096).astype(np.float32)
    assert np.array_equal(O.packbits(g, 0.25), np.packbits(g > 0.25, bitorder="little"))


def test_sph_from_ray_hits_the_sphere():
    rng = np.random.default_rng(3)
    o = rng.uniform(-0.5, 0.5, (1000, 3)).astype(np.float32)
    d = rng.standard_normal((1000, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    R = 2.5
    c = O.sph_from_ray(o, d, R)
    theta, phi = (c[:, 0] + 1) * np.pi / 2, c[:, 1] * np.pi
    p = R * np.stack([np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi)], -1)  # y-up convention of the kernel
    t = ((p - o) * d).sum(1)
    np.testing.assert_allclose(o + t[:, None] * d, p, atol=2e-5)
    assert np.all(t > 0)


def _uniform_packed(N, T, rng):
    """A packed-sample layout equivalent to uniform sampling: deltas = (dz, dz)."""
    sig = (rng.random((N, T)) * 30).astype(np.float32)
    sig[rng.random((N, T)) < 0.4] = 0
    rgb = rng.random((N, T, 3)).astype(np.float32)
    dz = (rng.random((N, 1)) * 0.02 + 0.002).astype(np.float32)
    deltas = np.repeat(np.repeat(dz, T, 1)[..., None], 2, -1)
    rays = np.stack([np.arange(N), np.arange(N) * T, np.full(N, T)], -1).astype(np.int32)
    return sig, rgb, deltas, rays, dz


def test_packed_compositor_equals_reference_torch_formulas():
    """composite_rays_train (T_thresh = 0) must reproduce the reference's torch compositor
    (renderer_dynamic.py:185-224) when fed uniform samples; its backward must equal torch autograd."""
    rng = np.random.default_rng(4)
    N, T = 64, 48
    sig, rgb, deltas, rays, dz = _uniform_packed(N, T, rng)
    ws, dp, img = O.composite_rays_train_forward(sig.reshape(-1), rgb.reshape(-1, 3), deltas.reshape(-1, 2), rays, 0.0)
    s64 = torch.tensor(sig, dtype=torch.float64, requires_grad=True)
    c64 = torch.tensor(rgb, dtype=torch.float64, requires_grad=True)
    alphas = 1 - torch.exp(-torch.tensor(deltas[..., 0], dtype=torch.float64) * s64)
    shifted = torch.cat([torch.ones_like(alphas[:, :1]), 1 - alphas + 1e-15], -1)
    w = alphas * torch.cumprod(shifted, -1)[:, :-1]
    t_end = torch.cumsum(torch.tensor(deltas[..., 1], dtype=torch.float64), -1)  # the kernel's depth uses the END of each step
    np.testing.assert_allclose(ws, w.sum(-1).detach().numpy(), atol=2e-6)
    np.testing.assert_allclose(dp, (w * t_end).sum(-1).detach().numpy(), atol=2e-6)
    np.testing.assert_allclose(img, (w.unsqueeze(-1) * c64).sum(-2).detach().numpy(), atol=2e-6)
    g_ws, g_img = rng.standard_normal(N), rng.standard_normal((N, 3))
    ((w.sum(-1) * torch.tensor(g_ws)).sum() + ((w.unsqueeze(-1) * c64).sum(-2) * torch.tensor(g_img)).sum()).backward()
    gs, gc = O.composite_rays_train_backward(g_ws, g_img, sig.reshape(-1), rgb.reshape(-1, 3), deltas.reshape(-1, 2), rays, ws, img, 0.0)
    np.testing.assert_allclose(gc.reshape(N, T, 3), c64.grad.numpy(), atol=1e-5, rtol=1e-4)
    np.testing.assert_allclose(gs.reshape(N, T), s64.grad.numpy(), atol=2e-5, rtol=1e-3)


def test_packed_compositor_early_termination_and_invalid_rays():
    rng = np.random.default_rng(5)
    N, T = 32, 40
    sig, rgb, deltas, rays, dz = _uniform_packed(N, T, rng)
    sig[:] = 200.0  # opaque: terminates after a few samples
    ws, dp, img = O.composite_rays_train_forward(sig.reshape(-1), rgb.reshape(-1, 3), deltas.reshape(-1, 2), rays, 1e-4)
    a = 1 - np.exp(-200.0 * dz[:, 0].astype(np.float64))
    k = np.ceil(np.log(1e-4) / np.log(1 - a)).astype(int)  # first step after which T < 1e-4
    expect = 1 - (1 - a) ** np.minimum(k, T)
    np.testing.assert_allclose(ws, expect, atol=1e-5)
    rays2 = rays.copy()
    rays2[3, 2] = 0
    rays2[5, 1] = N * T - 3  # runs past M -> treated as empty
    ws2, dp2, img2 = O.composite_rays_train_forward(sig.reshape(-1), rgb.reshape(-1, 3), deltas.reshape(-1, 2), rays2, 1e-4)
    assert ws2[3] == 0 and ws2[5] == 0 and not img2[[3, 5]].any() and np.array_equal(ws2[[0, 1, 2]], ws[[0, 1, 2]])


def test_marcher_invariants():
    """Samples lie in occupied cells, inside the box, ordered along the ray, deltas consistent; counts bounded."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(GOLD), "..", "selfsupervised-nvsf_amd"))
    from nvsf import synthetic as S
    rng = np.random.default_rng(6)
    grid = S.boxes_density_grid(rng, 2, 128, 48)
    bits = O.packbits(grid, 0.5)
    n, max_steps = 600, 512
    o, d = S.camera_rays(n, rng)
    aabb = np.array([-2, -2, -2, 2, 2, 2], np.float32)
    nears, fars = O.near_far_from_aabb(o, d, aabb, 0.02)
    M = n * max_steps
    xyz, dirs, deltas, rays, counter = O.march_rays_train(o, d, bits, 2.0, 0.0, max_steps, 2, 128, M, nears, fars, np.zeros(n, np.float32))
    total = int(counter[0])
    assert counter[1] == n and total == rays[:, 2].sum() and total > 0
    assert np.array_equal(rays[:, 0], np.arange(n)) and np.array_equal(rays[:, 1], np.cumsum(rays[:, 2]) - rays[:, 2])
    assert np.all(np.abs(xyz[:total]) <= 2.0) and rays[:, 2].max() <= max_steps
    # every emitted sample sits in an occupied cell of its cascade
    p = xyz[:total]
    level = np.where(np.abs(p).max(1) > 1.0, 1, 0)
    mb = np.where(level == 1, 2.0, 1.0)[:, None]
    cell = np.clip((0.5 * (p / mb + 1) * 128).astype(np.int64), 0, 127)
    idx = level * 128 ** 3 + O.morton3D(cell.astype(np.int32)).astype(np.int64)
    assert np.all((bits[idx // 8] >> (idx % 8)) & 1)
    dt_min = np.float32(2 * np.sqrt(3.0) / max_steps)
    assert np.allclose(deltas[:total, 0], dt_min, rtol=1e-6) and np.all(deltas[:total, 1] >= dt_min * 0.999)
    for r in rays[rays[:, 2] > 1][:50]:
        seg = p[r[1]:r[1] + r[2]]
        t = (seg - o[r[0]]) @ d[r[0]]
        assert np.all(np.diff(t) > 0)
    # a second call with the counter carried over appends after the first batch
    xyz2, _, _, rays2, counter2 = O.march_rays_train(o, d, bits, 2.0, 0.0, max_steps, 2, 128, 2 * M, nears, fars, np.zeros(n, np.float32),
                                                     counter=counter.copy())
    assert counter2[0] == 2 * total and counter2[1] == 2 * n
    assert np.array_equal(xyz2[total:2 * total], xyz[:total]) and not xyz2[:total].any()


# ---- field operators ---------------------------------------------------------------------------------
def test_hashgrid_against_independent_numpy_evaluation():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(GOLD), "..", "selfsupervised-nvsf_amd"))
    from nvsf.field_ops import GridSpec
    spec = GridSpec(3, 6, 2, 12, 4, 1.6)
    rng = np.random.default_rng(7)
    table = rng.standard_normal(spec.n_params).astype(np.float16)
    x = rng.random((500, 3)).astype(np.float32)
    got = O.hashgrid_fwd(x, (0, 1, 2), table, spec).astype(np.float64)
    tab = table.astype(np.float64).reshape(-1, 2)
    ref = np.zeros((500, 12))
    for l in range(6):
        res, rows, off = spec.res[l], spec.offsets[l + 1] - spec.offsets[l], spec.offsets[l]
        pos = x.astype(np.float64) * spec.scales[l] + 0.5
        c0 = np.floor(pos).astype(np.int64)
        fr = pos - c0
        for corner in range(8):
            b = np.array([(corner >> k) & 1 for k in range(3)])
            cc = (c0 + b).astype(np.uint64)
            wgt = np.prod(np.where(b, fr, 1 - fr), axis=1)
            if res ** 3 <= rows:
                idx = cc[:, 0] + cc[:, 1] * res + cc[:, 2] * res * res
            else:
                idx = (cc[:, 0] * 1) ^ ((cc[:, 1] * 2654435761) & 0xFFFFFFFF) ^ ((cc[:, 2] * 805459861) & 0xFFFFFFFF)
            idx = (idx % rows).astype(np.int64)
            ref[:, 2 * l:2 * l + 2] += wgt[:, None] * tab[off + idx]
    np.testing.assert_allclose(got, ref, atol=2e-3, rtol=2e-3)  # fp16 output rounding + fp32 positions
    assert spec.res == [4, 7, 11, 17, 27, 42]  # ceil(4 * 1.6^l - 1) + 1


def test_mlp_frequency_sh_against_fp64():
    rng = np.random.default_rng(8)
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(GOLD), "..", "selfsupervised-nvsf_amd"))
    from nvsf.field_ops import MlpSpec
    spec = MlpSpec(87, 1, 64, 2)
    assert (spec.in_cols, spec.out_cols, spec.n_params) == (96, 16, 64 * 96 + 64 * 64 + 16 * 64)
    w = np.concatenate([(rng.uniform(-1, 1, a * b) * np.sqrt(6 / (a + b))).astype(np.float16) for a, b in spec.shapes])
    x = rng.standard_normal((200, 87)).astype(np.float32)
    out, hid = O.mlp_fwd(x, w, 87, 96, 2, want_hidden=True)
    W0, W1, W2 = [m.astype(np.float64) for m in (w[:64 * 96].reshape(64, 96), w[64 * 96:64 * 96 + 4096].reshape(64, 64), w[-1024:].reshape(16, 64))]
    a = np.concatenate([x.astype(np.float16).astype(np.float64), np.ones((200, 9))], 1)
    h1 = np.maximum(a @ W0.T, 0).astype(np.float16).astype(np.float64)
    h2 = np.maximum(h1 @ W1.T, 0).astype(np.float16).astype(np.float64)
    np.testing.assert_allclose(out, h2 @ W2.T, atol=5e-3, rtol=0)
    assert (hid[:, 0].astype(np.float64) == h1).mean() > 0.995
    d = rng.random((300, 3)).astype(np.float32)
    f = O.freq_encode(d, 12).astype(np.float64).reshape(300, 3, 12, 2)
    ang = (d.astype(np.float64)[:, :, None] * (2.0 ** np.arange(12))) * np.pi
    np.testing.assert_allclose(f[..., 0], np.sin(ang), atol=6e-4)
    np.testing.assert_allclose(f[..., 1], np.cos(ang), atol=6e-4)
    sh = O.sh4_encode(d).astype(np.float64)
    v = d.astype(np.float64) * 2 - 1
    np.testing.assert_allclose(sh[:, 0], 0.28209479177387814, atol=2e-4)
    np.testing.assert_allclose(sh[:, 2], 0.48860251190291987 * v[:, 2], atol=5e-4)
    np.testing.assert_allclose(sh[:, 6], 0.94617469575755997 * v[:, 2] ** 2 - 0.31539156525251999, atol=1e-3)
    # orthonormality of the 16 basis functions over the sphere (Monte-Carlo): gram matrix ~ identity / (4 pi) * 4 pi
    u = rng.standard_normal((200000, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    Y = O.sh4_encode(((u + 1) / 2).astype(np.float32)).astype(np.float64)
    gram = Y.T @ Y / len(u) * 4 * np.pi
    np.testing.assert_allclose(gram, np.eye(16), atol=0.03)


def test_chamfer_restatement_against_numpy():
    import ctypes
    O.build()
    lib = ctypes.CDLL(os.path.join(os.path.dirname(GOLD), "..", "oracle", "liboracle_chamfer.so"))
    rng = np.random.default_rng(9)
    B, n, m = 2, 300, 170
    a, b = rng.standard_normal((B, n, 3)).astype(np.float32), rng.standard_normal((B, m, 3)).astype(np.float32)
    d1, d2 = np.empty((B, n), np.float32), np.empty((B, m), np.float32)
    i1, i2 = np.empty((B, n), np.int32), np.empty((B, m), np.int32)
    P = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    U = ctypes.c_uint32
    lib.oracle_chamfer_forward(P(a), P(b), U(B), U(n), U(m), P(d1), P(d2), P(i1), P(i2))
    D = ((a[:, :, None, :].astype(np.float64) - b[:, None, :, :]) ** 2).sum(-1)
    assert np.array_equal(i1, D.argmin(2)) and np.array_equal(i2, D.argmin(1))
    np.testing.assert_allclose(d1, D.min(2), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(d2, D.min(1), rtol=1e-5, atol=1e-6)
    # gradient of sum(g1*d1) + sum(g2*d2) by finite differences on one coordinate
    g1, g2 = rng.standard_normal((B, n)).astype(np.float32), rng.standard_normal((B, m)).astype(np.float32)
    ga, gb = np.zeros_like(a), np.zeros_like(b)
    lib.oracle_chamfer_backward(P(a), P(b), U(B), U(n), U(m), P(g1), P(g2), P(i1), P(i2), P(ga), P(gb))
    def loss(a_, b_):
        D_ = ((a_[:, :, None, :].astype(np.float64) - b_[:, None, :, :]) ** 2).sum(-1)
        return (g1 * D_.min(2)).sum() + (g2 * D_.min(1)).sum()
    eps = 1e-4
    ap = a.copy(); ap[1, 17, 2] += eps
    am = a.copy(); am[1, 17, 2] -= eps
    np.testing.assert_allclose((loss(ap, b) - loss(am, b)) / (2 * eps), ga[1, 17, 2], rtol=2e-2, atol=2e-3)


# ---------------------------------------------------------------------------------------------------------------------
# The wave-cooperative marcher builds 64 chain members t_k = fl(t_{k-1} + c) at once for a constant step
# (csrc/march_device.h, Marcher::fill_batch).  The integer closed form below is the host restatement of that device
# code, line by line; it must reproduce the serial fp32 recurrence of the reference's marcher
# (raymarching.cu:414-416, 434-437: `t += dt`) bit for bit.
def _chain_closed_form(t0, c, K=64):
    tb, cb = int(np.float32(t0).view(np.uint32)), int(np.float32(c).view(np.uint32))
    e, ec = tb >> 23, cb >> 23
    d = e - ec
    if not (0 <= d <= 24 and 24 <= e < 254 and ec > 0):
        return None  # the device takes the serial path
    m0, mc = (tb & 0x7FFFFF) | 0x800000, (cb & 0x7FFFFF) | 0x800000
    q, rem, half = mc >> d, mc & ((1 << d) - 1), (1 << (d - 1)) if d > 0 else 0
    if d > 0 and rem == half:
        s, s_first = q + (q & 1), q + ((m0 + q) & 1)
    else:
        s = q + (1 if (d > 0 and rem > half) else 0)
        s_first = s
    if s == 0:
        return None
    scale = np.uint32((e - 23) << 23).view(np.float32)
    k = np.arange(K, dtype=np.int64)
    mk = np.where(k == 0, m0, m0 + s_first + (k - 1) * s)
    mprev = np.where(k <= 1, m0, m0 + s_first + (k - 2) * s)
    valid = (k == 0) | (mprev + q < (1 << 24))
    nb = int(valid.sum())
    assert valid[:nb].all()
    return (mk[:nb].astype(np.float32) * scale).astype(np.float32)


def test_constant_step_chain_closed_form():
    rng = np.random.default_rng(0)
    checked = 0
    for it in range(40000):
        ee = int(rng.integers(-12, 4))
        t0 = np.float32(rng.uniform(1, 2) * 2.0 ** ee)
        mode = it % 4
        if mode == 0:    # the marcher's own steps: 2 sqrt(3) / max_steps
            c = np.float32(np.float32(2.0) * np.float32(1.7320508075688772) / np.float32(rng.choice([128, 256, 512, 768, 1000, 1024, 2048, 4096])))
        elif mode == 1:  # arbitrary steps, from far below one ulp of t to larger than t
            c = np.float32(rng.uniform(1, 2) * 2.0 ** int(rng.integers(ee - 26, ee + 2)))
        elif mode == 2:  # exact ties (remainder == half an ulp): round-to-even alternation
            d = int(rng.integers(1, 24))
            cb = int(np.float32(rng.uniform(1, 2) * 2.0 ** (ee - d)).view(np.uint32))
            c = np.uint32(((cb >> d) << d) | (1 << (d - 1))).view(np.float32)
        else:            # start just below a power of two: the batch must stop at the binade crossing
            t0 = np.float32(np.float32(2.0 ** (ee + 1)) - np.float32(int(rng.integers(1, 3000)) * 2.0 ** (ee - 23)))
            c = np.float32(rng.uniform(1, 2) * 2.0 ** int(rng.integers(ee - 12, ee + 1)))
        got = _chain_closed_form(t0, c)
        if got is None:
            continue
        t = np.float32(t0)
        for v in got:
            assert v == t, (t0, c)
            t = np.float32(t + np.float32(c))
        checked += len(got)
    assert checked > 1_000_000


def test_torch_cpu_path_matches_the_c_oracle():
    """oracle/torch_cpu_path.py (the vectorised PyTorch-CPU restatement bench.py times as `cpu_baseline.torch_cpu`) renders the same
    images as the scalar C oracle: 1e-4 on image / depth / weights_sum for a LiDAR and a camera batch of the config-2 field shape
    (smaller table)."""
    import importlib.util
    import sys
    import torch
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(ROOT, "selfsupervised-nvsf_amd"))
    from nvsf import field_ops as ops, synthetic as S
    spec_ = importlib.util.spec_from_file_location("torch_cpu_path", os.path.join(ROOT, "oracle", "torch_cpu_path.py"))
    TP = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(TP)
    rng = np.random.default_rng(2)
    grid = ops.GridSpec(3, 16, 2, 14, 16, float(np.exp2(np.log2(2048 / 16) / 15)))
    table = (rng.standard_normal(grid.n_params) * 0.3).astype(np.float16)
    sig, hl, hc = ops.MlpSpec(32, 16, 64, 1), ops.MlpSpec(87, 1, 64, 2), ops.MlpSpec(31, 3, 64, 2)
    w = lambda sp: np.concatenate([(rng.uniform(-1, 1, a * b) * np.sqrt(6.0 / (a + b))).astype(np.float16) for a, b in sp.shapes])
    w_sigma, w_rd, w_int, w_col = w(sig), w(hl), w(hl), w(hc)
    N, T = 48, 96
    aabb = np.array([-S.BOUND] * 3 + [S.BOUND] * 3, np.float32)
    for lidar in (True, False):
        o, d = (S.lidar_rays if lidar else S.camera_rays)(N, rng)
        if lidar:
            nears, fars = np.full(N, S.MIN_NEAR, np.float32), np.full(N, S.LIDAR_MAX_DEPTH, np.float32)
        else:
            nears, fars = O.near_far_from_aabb(o, d, aabb, S.MIN_NEAR)
        ref = O.render_static(o, d, nears, fars, torch.linspace(0.0, 1.0, T).numpy(), None, float(S.BOUND), table, grid, w_sigma, lidar,
                              w_rd if lidar else w_col, w_int if lidar else None, np.ones(3, np.float32))
        t = torch.from_numpy
        img, dep, ws = TP.render_static(t(o), t(d), t(nears), t(fars), T, float(S.BOUND), t(table), grid, t(w_sigma), sig, lidar,
                                        t(w_rd if lidar else w_col), t(w_int) if lidar else None, hl if lidar else hc)
        assert float(ref["weights_sum"].max()) > 0.05
        np.testing.assert_allclose(img.numpy(), ref["image"], atol=1e-4, rtol=0)
        np.testing.assert_allclose(dep.numpy(), ref["depth"], atol=1e-4, rtol=0)
        np.testing.assert_allclose(ws.numpy(), ref["weights_sum"], atol=1e-4, rtol=0)


@pytest.mark.parametrize("table_std,n_rays", [(0.1, 64), (0.5, 16)])
def test_specification_against_tcnn_published_arithmetic(table_std, n_rays):
    """DESIGN.md section 4.1 / 4.3 deviate from tiny-cuda-nn's published arithmetic in two places (hash-grid corners accumulated in
    fp32 instead of fp16 per corner; network outputs delivered in fp32 instead of __half).  This MEASURES the consequence on the
    config-2 render (64 rays x 768 samples per modality, N(0, 0.1) tables; a second, harsher table scale) by rendering both ways with the
    oracle (render_static(tcnn_arith=...)) and asserts the bound written into DESIGN.md: composited depth / image / weights_sum differ
    by far less than the north_star tolerance (1e-4 abs), so no `tcnn_exact` switch is offered; per-sample sigma differs by at
    most ~1e-3 relative (one fp16 rounding of the density logit: |h0| 2^-11)."""
    import torch
    from nvsf import synthetic as S
    from nvsf.nerf.models.network_static import NeRFNetworkStatic
    torch.manual_seed(0)
    m = NeRFNetworkStatic(bound=S.BOUND, min_near=S.MIN_NEAR, min_near_lidar=S.MIN_NEAR, lidar_max_depth=S.LIDAR_MAX_DEPTH)
    with torch.no_grad():
        g = torch.Generator().manual_seed(5)
        for enc in (m.hash_encoder_lidar, m.hash_encoder_camera):
            enc.params.copy_(torch.randn(enc.params.shape, generator=g) * table_std)
    f16 = lambda net: net.params.detach().numpy().astype(np.float16)
    rng = np.random.default_rng(0)
    T = 768
    worst = {}
    for lidar in (True, False):
        o, d = (S.lidar_rays if lidar else S.camera_rays)(n_rays, rng)
        enc = m.hash_encoder_lidar if lidar else m.hash_encoder_camera
        if lidar:
            nears, fars = np.full(n_rays, m.min_near_lidar, np.float32), np.full(n_rays, m.lidar_max_depth, np.float32)
        else:
            nears, fars = O.near_far_from_aabb(o, d, np.array([-S.BOUND] * 3 + [S.BOUND] * 3, np.float32), m.min_near)
        spec_out, tcnn_out = (O.render_static(o, d, nears, fars, torch.linspace(0.0, 1.0, T).numpy(), None, float(S.BOUND),
                                             enc.params.detach().numpy().astype(np.float16), enc.spec, f16(m.sigma_net), lidar,
                                             f16(m.raydrop_net) if lidar else f16(m.color_net), f16(m.intensity_net) if lidar else None,
                                             np.ones(3, np.float32), tcnn_arith=ta) for ta in (False, True))
        assert float(spec_out["weights_sum"].mean()) > 0.3  # the rays do hit something: the comparison is not of empty renders
        for k in ("depth", "image", "weights_sum"):
            worst[k] = max(worst.get(k, 0.0), float(np.abs(spec_out[k].astype(np.float64) - tcnn_out[k].astype(np.float64)).max()))
        rel = np.abs(spec_out["sigmas"].astype(np.float64) - tcnn_out["sigmas"]) / np.maximum(spec_out["sigmas"], 1e-12)
        worst["sigma_rel"] = max(worst.get("sigma_rel", 0.0), float(rel.max()))
    print(f"spec vs tcnn arithmetic (table std {table_std}): {worst}")
    # measured: depth 2e-6 / 9e-6, image 1.6e-5 / 1.6e-5, weights_sum 1.7e-6 / 5.4e-6, sigma 1.9e-4 / 7.8e-4 relative (std 0.1 / 0.5)
    assert worst["depth"] <= 2e-5 and worst["image"] <= 4e-5 and worst["weights_sum"] <= 2e-5
    assert worst["sigma_rel"] <= 2e-3
    assert max(worst["depth"], worst["image"], worst["weights_sum"]) < 1e-4  # the bar under which no tcnn_exact option is needed


# ---- the one deviation of the a1-a9 oracle from a compiled reference that had no price: nvcc's default multiply-add contraction -------
_FMAD_KINDS = ["random10", "random50", "dense", "empty", "scene", "stripes"]


def _fmad_grid(kind, rng):
    from nvsf import synthetic as S
    if kind == "scene":
        return O.packbits(S.boxes_density_grid(np.random.default_rng(0), cascades=2, H=128, n_boxes=64), 0.5)
    if kind == "stripes":
        g = np.zeros((2, 128 ** 3), bool)
        g[:, (np.arange(128 ** 3) % 7) == 0] = True
        return np.packbits(g.reshape(-1), bitorder="little")
    p = {"random10": 0.1, "random50": 0.5, "dense": 1.0, "empty": 0.0}[kind]
    return np.packbits(rng.random(2 * 128 ** 3) < p, bitorder="little")


@pytest.mark.parametrize("modality", ["cam", "lidar"])
def test_price_of_nvcc_multiply_add_contraction_on_the_marcher(modality):
    """VERDICT r4 item 7.  raymarching.cu compiled by nvcc (--fmad=true, the default) contracts `ox + t * dx`, `x * mip_rbound + 1`,
    the cell-exit expressions and the jitter of t0 (raymarching.cu:375, 386-388, 400-405, 420-433) into single-rounding FMAs; the
    oracle and the HIP build round every operation (-ffp-contract=off) and agree with EACH OTHER bit for bit.  Here the same
    restatement is built both ways (oracle/Makefile: liboracle_raymarching_fmad.so = -DORACLE_FMAD) and config 3's batch -- 4096 rays,
    max_steps 1024, bound 2, 2 cascades x 128^3 -- is marched through the six grid kinds of the GPU parity tests, without and with
    jitter, with dt_gamma 0 and 1/256.  Recorded: the fraction of rays whose sample COUNT differs (a discrete
    decision flipped: a voxel index at a cell face, the exit of a skip) and max |delta xyz| over the samples of rays whose counts agree."""
    from nvsf import synthetic as S
    n, max_steps = 4096, 1024
    rng = np.random.default_rng(21)
    o, d = (S.camera_rays if modality == "cam" else S.lidar_rays)(n, np.random.default_rng(12))
    aabb = np.array([-2, -2, -2, 2, 2, 2], np.float32)
    nears, fars = O.near_far_from_aabb(o, d, aabb, 0.02)
    worst_frac, worst_xyz, worst_dt, total_rays, total_diff, total_samples, moved = 0.0, 0.0, 0.0, 0, 0, 0, 0
    for kind in _FMAD_KINDS:
        bits = _fmad_grid(kind, rng)
        for dt_gamma, noises in ((0.0, np.zeros(n, np.float32)), (0.0, rng.random(n).astype(np.float32)), (1.0 / 256, rng.random(n).astype(np.float32))):
            M = n * max_steps
            xa, _, la, ra, ca = O.march_rays_train(o, d, bits, 2.0, dt_gamma, max_steps, 2, 128, M, nears, fars, noises)
            xb, _, lb, rb, cb = O.march_rays_train(o, d, bits, 2.0, dt_gamma, max_steps, 2, 128, M, nears, fars, noises, fmad=True)
            same = ra[:, 2] == rb[:, 2]
            frac = 1.0 - float(same.mean())
            worst_frac = max(worst_frac, frac)
            total_rays += n
            total_diff += int((~same).sum())
            # matched samples: the rays whose counts agree, sample by sample (offsets differ once an earlier ray's count does)
            idx_a = np.concatenate([np.arange(off, off + c) for off, c in ra[same][:, 1:3] if c > 0] or [np.zeros(0, np.int64)]).astype(np.int64)
            idx_b = np.concatenate([np.arange(off, off + c) for off, c in rb[same][:, 1:3] if c > 0] or [np.zeros(0, np.int64)]).astype(np.int64)
            assert idx_a.shape == idx_b.shape
            if idx_a.size:
                dx = np.abs(xa[idx_a] - xb[idx_b])
                worst_xyz = max(worst_xyz, float(dx.max()))
                worst_dt = max(worst_dt, float(np.abs(la[idx_a] - lb[idx_b]).max()))
                total_samples += idx_a.size
                moved += int((dx.max(axis=1) > 0).sum())
            if kind == "empty":
                assert ca[0] == 0 and cb[0] == 0
    # the numbers DESIGN.md section 3 quotes; printed with -s
    print(f"[fmad {modality}] rays whose sample count differs: {total_diff} of {total_rays} ({100.0 * total_diff / total_rays:.4f} %), worst case "
          f"{100.0 * worst_frac:.4f} % of a batch; matched samples {total_samples}, {moved} of them moved, max |dxyz| {worst_xyz:.3e}, max |ddelta| {worst_dt:.3e}")
    assert worst_frac < 0.01            # << 1 % of the rays of any batch see a flipped decision
    assert worst_xyz <= 1e-6            # positions of matched samples: one ulp of a coordinate in [-2, 2] is 2.4e-7
    assert worst_dt <= 1e-6
