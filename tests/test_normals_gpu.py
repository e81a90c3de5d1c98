"""GPU tests of the hash grid's coordinate gradient (nvsf_hashgrid_grad_x) and of what is built on it: autograd through
tinycudann.Encoding, density_gradient / render_normals (nvsf/nerf/normals.py) and the mesh export's vertex normals.  DESIGN.md 9l.

The kernel is pinned to the numpy float64 oracle tests/hashgrid_gradx_oracle.py with the bar (L F 2^D + 8) 2^-24 A[m, d] per element,
A = the sum of the absolute values of the output's addends: the standard bound for a sum of that many fp32 addends in any order with
a few roundings per addend.  Every figure that is asserted is printed first (run with -s to see them).
"""
import numpy as np
import pytest
import torch

import hashgrid_gradx_oracle as GX

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _spec(D, L, F, log2_T, base, top):
    from nvsf.field_ops import GridSpec
    pls = float(np.exp2(np.log2(top / base) / (L - 1))) if L > 1 else 1.0
    return GridSpec(D, L, F, log2_T, base, pls)


def _bar(spec, A):
    return (spec.L * spec.F * (1 << spec.D) + 8) * U * A


def _positions(rng, M, D):
    """Random positions in the unit cube; from 63 rows on the first rows are 0, 1, 0.5 (a grid node of the coarsest level: scale 3),
    mixtures of them, and positions outside the unit cube ([-0.4, 1.5], as test_hashgrid_backward_positions_outside_the_unit_cube)."""
    x = rng.random((M, D)).astype(np.float32)
    if M >= 63:
        x[0], x[1], x[2] = 0.0, 1.0, 0.5
        x[3] = [0.0, 1.0, 0.5][:D]
        x[4] = [0.5, 0.0, 1.0][:D]
        x[5:25] = (rng.random((20, D)) * 1.9 - 0.4).astype(np.float32)
        assert (x < 0).any() and (x > 1).any()
    return x


@pytest.fixture(scope="module")
def ops(hip_lib):
    from nvsf import field_ops
    return field_ops


@pytest.mark.parametrize("L,log2_T", [(1, 10), (5, 11), (16, 12)])
@pytest.mark.parametrize("F", [2, 4, 8])
@pytest.mark.parametrize("D", [2, 3])
def test_kernel_matches_the_float64_oracle(ops, dev, D, F, L, log2_T):
    """Every supported (D, F), L in {1, 5, 16} (L % 4 != 0 included), a small table (base 4 -> top 64: dense and hashed levels), M in
    {1, 63, 64, 65, 1000}, x as columns (3, 0, 2) of a 5-column matrix, fp32 and fp16 gradients, rows (contiguous and a padded,
    4-byte aligned view) and level-major layouts -- the three layouts agree bit for bit -- positions at 0, at 1, on grid nodes and
    outside the unit cube."""
    if D == 2:
        log2_T = 10  # 64^2 entries fit 2^12: the smallest table of the range keeps the fine 2-D levels hashed
    spec = _spec(D, L, F, log2_T, 4, 64)
    if L > 1:
        dense = [int(r) ** D <= int(n) for r, n in zip(spec.res, np.diff(spec.offsets))]
        assert any(dense) and not all(dense)
    rng = np.random.default_rng(1000 * D + 100 * F + L)
    table = (rng.standard_normal(spec.n_params) * 0.5).astype(np.float16)
    table_d = _t(table, dev)
    cols = (3, 0, 2)[:D]
    worst = 0.0
    for M in (1, 63, 64, 65, 1000):
        xw = rng.standard_normal((M, 5)).astype(np.float32)
        xw[:, list(cols)] = _positions(rng, M, D)
        x_d = _t(xw, dev)
        for half in (False, True):
            g = rng.standard_normal((M, L, F)).astype(np.float32)
            if half:
                g = g.astype(np.float16)
            ref, A = GX.grad_x(xw[:, list(cols)], table, spec, g.astype(np.float64))
            rows = _t(g.reshape(M, L * F), dev)
            got = ops.hashgrid_grad_x(x_d, cols, table_d, spec, rows)
            assert got.shape == (M, D) and got.dtype == torch.float32
            padded = torch.zeros(M, L * F + 3, dtype=rows.dtype, device=dev)[:, 1:1 + L * F]
            padded.copy_(rows)
            level_major = _t(np.ascontiguousarray(g.transpose(1, 0, 2)), dev)
            assert torch.equal(ops.hashgrid_grad_x(x_d, cols, table_d, spec, padded), got)
            assert torch.equal(ops.hashgrid_grad_x(x_d, cols, table_d, spec, level_major), got)
            err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
            bar = _bar(spec, A)
            assert (bar > 0).all()
            worst = max(worst, float((err / bar).max()))
            assert (err <= bar).all(), (M, half, float((err / bar).max()))
    print(f"hashgrid_grad_x D={D} F={F} L={L}: largest error / bar = {worst:.4f}")


def test_kernel_rejects_unsupported_shapes_and_accepts_empty_batches(ops, dev):
    from nvsf import _hip
    spec = _spec(3, 2, 2, 10, 4, 8)
    table = torch.zeros(spec.n_params, dtype=torch.float16, device=dev)
    out = ops.hashgrid_grad_x(torch.zeros(0, 3, device=dev), (0, 1, 2), table, spec, torch.zeros(0, 4, device=dev))
    assert out.shape == (0, 3)
    bad = _spec(3, 2, 1, 10, 4, 8)  # F = 1 is not instantiated
    with pytest.raises(_hip.NvsfHipError):
        ops.hashgrid_grad_x(torch.zeros(4, 3, device=dev), (0, 1, 2), torch.zeros(bad.n_params, dtype=torch.float16, device=dev), bad,
                            torch.zeros(4, 2, device=dev))


def _index_table(spec, rng):
    """Feature 0 of every entry = the x index of its grid vertex (every level dense: row = ix + iy res + iz res^2), feature 1 random."""
    table = (rng.standard_normal((spec.n_rows, spec.F)) * 0.5).astype(np.float16)
    for l in range(spec.L):
        res, off, n = int(spec.res[l]), int(spec.offsets[l]), int(spec.offsets[l + 1] - spec.offsets[l])
        assert res ** 3 <= n
        table[off:off + n, 0] = (np.arange(n) % res).astype(np.float16)
    return table.reshape(-1)


def test_exact_case_on_a_table_of_cell_indices(ops, dev):
    """Dense levels whose feature 0 is the vertex's integer x index, power-of-two gradients on feature 0 and none on feature 1:
    the encoded feature is pos_x, so dL/dx_x = sum_l scale_l g_l up to the bar of that final sum, and dL/dx_y = dL/dx_z = 0 EXACTLY
    (the kernel differences each corner pair before it blends)."""
    spec = _spec(3, 5, 2, 19, 4, 64)
    rng = np.random.default_rng(3)
    table = _index_table(spec, rng)
    M = 257
    x = (rng.random((M, 3)) * 0.75 + 0.05).astype(np.float32)  # x < 1 - 0.5 / 3: cell + 1 stays below res on every level, no wrap into the next row
    g = np.zeros((M, spec.L, spec.F), np.float32)
    g[:, :, 0] = (2.0 ** rng.integers(-6, 3, (M, spec.L))) * rng.choice([-1.0, 1.0], (M, spec.L))
    want = (g[:, :, 0].astype(np.float64) * np.array(spec.scales)[None, :]).sum(-1)
    ref, _ = GX.grad_x(x, table, spec, g)
    assert np.abs(ref[:, 0] - want).max() <= 1e-12 * np.abs(want).max() and np.abs(ref[:, 1:]).max() <= 1e-12
    for grad in (g, g.astype(np.float16)):
        got = ops.hashgrid_grad_x(_t(x, dev), (0, 1, 2), _t(table, dev), spec, _t(grad.reshape(M, -1), dev)).cpu().numpy()
        assert (got[:, 1:] == 0).all()
        bar = _bar(spec, (np.abs(g[:, :, 0]).astype(np.float64) * np.array(spec.scales)[None, :]).sum(-1))
        err = np.abs(got[:, 0].astype(np.float64) - want)
        print(f"exact case: largest error / bar = {float((err / bar).max()):.4f}")
        assert (err <= bar).all()


def test_reruns_are_bit_identical_and_unaligned_output_views_work(ops, dev):
    spec = _spec(3, 16, 2, 12, 4, 64)
    rng = np.random.default_rng(9)
    M = 1000
    x = _t(_positions(rng, M, 3), dev)
    table = _t((rng.standard_normal(spec.n_params) * 0.5).astype(np.float16), dev)
    g = _t(rng.standard_normal((M, 32)).astype(np.float32), dev)
    first = ops.hashgrid_grad_x(x, (0, 1, 2), table, spec, g)
    for _ in range(3):
        assert torch.equal(ops.hashgrid_grad_x(x, (0, 1, 2), table, spec, g), first)
    wide = torch.full((M, 5), 7.0, device=dev)
    view = wide[:, 1:4]  # rows of 20 bytes starting at byte 4: 4-byte aligned only
    assert ops.hashgrid_grad_x(x, (0, 1, 2), table, spec, g, out=view) is view
    assert torch.equal(view, first) and bool((wide[:, 0] == 7.0).all()) and bool((wide[:, 4] == 7.0).all())


def test_mlp_column_blocks_feed_the_kernel_without_a_transpose(ops, dev):
    """The column-block dL/dx of mlp_backward(grad_x_blocks=F) is the level-major gradient: same bits as its row form."""
    spec = _spec(3, 16, 2, 12, 4, 64)
    net = ops.MlpSpec(32, 16, 64, 1)
    rng = np.random.default_rng(13)
    M = 777
    x = _t(rng.random((M, 3)).astype(np.float32), dev)
    table = _t((rng.standard_normal(spec.n_params) * 0.5).astype(np.float16), dev)
    w = _t((rng.standard_normal(net.n_params) * 0.2).astype(np.float16), dev)
    feat = ops.hashgrid_forward(x, (0, 1, 2), table, spec)
    go = _t(rng.standard_normal((M, 16)).astype(np.float32), dev)
    blocks, _ = ops.mlp_backward(feat, w, net, go, grad_x_blocks=2)
    rows, _ = ops.mlp_backward(feat, w, net, go)
    assert tuple(blocks.shape) == (16, M, 2)
    assert torch.equal(ops.hashgrid_grad_x(x, (0, 1, 2), table, spec, blocks), ops.hashgrid_grad_x(x, (0, 1, 2), table, spec, rows))


# ---- autograd ------------------------------------------------------------------------------------------------------------------------
def _encoding(dev, L, F, log2_T, base, pls, seed=3):
    import tinycudann as tcnn
    enc = tcnn.Encoding(3, {"otype": "HashGrid", "n_levels": L, "n_features_per_level": F, "log2_hashmap_size": log2_T,
                            "base_resolution": base, "per_level_scale": pls}, seed=seed)
    with torch.no_grad():
        enc.params.normal_(0.0, 0.5, generator=torch.Generator().manual_seed(seed))
    return enc.to(dev)


def test_autograd_returns_the_coordinate_gradient_rows(ops, dev):
    """tcnn.Encoding(3, HashGrid)(x) with x.requires_grad: x.grad is ops.hashgrid_grad_x bit for bit and the table gradient of the
    same backward is the one of a run without requires_grad, which is the parent's behaviour: the forward output and the table
    gradient equal direct calls of hashgrid_forward / hashgrid_backward.  Positions j / 16 on integer scales and gradients k / 8 make
    every addend of the table gradient a multiple of 2^-15 below 2^3, so the fp32 atomic sums are exact in any order and the
    comparison of the scattered tables can be bitwise."""
    enc = _encoding(dev, 5, 2, 10, 4, 2.0)
    spec = enc.spec
    assert [float(s) for s in spec.scales] == [3.0, 7.0, 15.0, 31.0, 63.0]
    rng = np.random.default_rng(21)
    M = 200
    x = _t((rng.integers(1, 16, (M, 3)) / 16.0).astype(np.float32), dev)
    go = _t((rng.integers(-8, 9, (M, 10)) / 8.0).astype(np.float16), dev)
    # without requires_grad: the parent's behaviour
    y0 = enc(x)
    y0.backward(go)
    table_grad0 = enc.params.grad.clone()
    enc.params.grad = None
    assert torch.equal(y0, ops.hashgrid_forward(x, (0, 1, 2), enc.table_f16(), spec))
    assert torch.equal(table_grad0, ops.hashgrid_backward(x, (0, 1, 2), spec, go))
    assert bool((table_grad0 != 0).any())
    # with it
    xg = x.clone().requires_grad_()
    y1 = enc(xg)
    assert torch.equal(y1, y0)
    y1.backward(go)
    assert xg.grad is not None and xg.grad.dtype == torch.float32 and not xg.grad.requires_grad
    assert torch.equal(xg.grad, ops.hashgrid_grad_x(x, (0, 1, 2), enc.table_f16(), spec, go))
    assert bool((xg.grad != 0).any())
    assert torch.equal(enc.params.grad, table_grad0)
    # coordinates only: the table is frozen
    enc.params.requires_grad_(False)
    xg2 = x.clone().requires_grad_()
    enc(xg2).backward(go)
    assert torch.equal(xg2.grad, xg.grad)
    # columns of a wider matrix: the other columns receive zeros
    enc.params.requires_grad_(True)
    wide = torch.zeros(M, 5, device=dev)
    wide[:, [3, 0, 2]] = x
    wide.requires_grad_()
    enc.encode_columns(wide, (3, 0, 2)).backward(go)
    assert torch.equal(wide.grad[:, [3, 0, 2]], xg.grad) and bool((wide.grad[:, [1, 4]] == 0).all())


def test_autograd_returns_the_coordinate_gradient_level_major(ops, dev):
    """The level-major layout of the L8 F4 grid (fp16 [L, M, F] features): x.grad is ops.hashgrid_grad_x of the [L, M, F] gradient bit
    for bit; the eight samples touch 512 distinct table rows (asserted), so every entry of the table gradient has one addend and the
    scatter is comparable bitwise with and without requires_grad."""
    enc = _encoding(dev, 8, 4, 19, 512, float(np.exp2(np.log2(32768 / 512) / 7)))
    spec = enc.spec
    assert ops.level_major_eligible(spec)
    rng = np.random.default_rng(22)
    M = 8
    xh = rng.random((M, 3)).astype(np.float32)
    for l in range(spec.L):
        scale, res, off, n = GX._level(spec, l)
        cell, _ = GX.cells(xh, scale)
        touched = np.concatenate([GX.rows(cell + np.array([(c >> d) & 1 for d in range(3)], np.int64)[None, :], res, n) for c in range(8)])
        assert np.unique(touched).size == 8 * M
    x = _t(xh, dev)
    go = _t(rng.standard_normal((spec.L, M, spec.F)).astype(np.float16), dev)
    y0 = enc(x, level_major=True)
    assert tuple(y0.shape) == (spec.L, M, spec.F)
    y0.backward(go)
    table_grad0 = enc.params.grad.clone()
    enc.params.grad = None
    xg = x.clone().requires_grad_()
    y1 = enc(xg, level_major=True)
    assert torch.equal(y1, y0)
    y1.backward(go)
    assert torch.equal(xg.grad, ops.hashgrid_grad_x(x, (0, 1, 2), enc.table_f16(), spec, go))
    assert torch.equal(xg.grad, ops.hashgrid_grad_x(x, (0, 1, 2), enc.table_f16(), spec, go.permute(1, 0, 2).reshape(M, -1)))
    assert bool((xg.grad != 0).all()) and torch.equal(enc.params.grad, table_grad0) and bool((table_grad0 != 0).any())


def test_static_density_differentiates_with_respect_to_position(dev, field_model):
    """NeRFNetworkStatic.density takes its operator chain when x.requires_grad; sigma is the fused node's and
    d sigma.sum() / d x is density_gradient's gradient up to the fp16 hand-overs of the autograd chain (the MLP node returns its
    input gradient in the feature dtype)."""
    from nvsf.nerf import normals
    m = field_model
    g = torch.Generator().manual_seed(2)
    x = ((torch.rand(500, 3, generator=g) * 1.9 - 0.95) * m.bound).to(dev)
    with torch.no_grad():
        sigma0 = m.density(x, cal_lidar_color=True)["sigma"]
    xg = x.clone().requires_grad_()
    with torch.enable_grad():
        sigma = m.density(xg, cal_lidar_color=True)["sigma"]
        sigma.sum().backward()
    assert torch.allclose(sigma.detach(), sigma0, rtol=1e-5, atol=0)  # the same logits; torch.exp against the fused node's exp kernel
    direct = normals.density_gradient(m, x, cal_lidar_color=True)
    assert torch.equal(direct["sigma"], sigma0)
    scale = float(direct["grad"].abs().max())
    err = float((xg.grad - direct["grad"]).abs().max())
    print(f"density autograd vs density_gradient: max |diff| = {err:.3e} of max |grad| = {scale:.3e}")
    assert scale > 0 and err <= 2e-2 * scale  # fp16 gradient of 32 features: 2^-11 relative each, cancelling sums; a wrong chain is O(1) off
    for p in m.parameters():
        p.grad = None


# ---- density_gradient ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def field_model(dev):
    from nvsf import synthetic as S
    from nvsf.nerf.models.network_static import NeRFNetworkStatic
    torch.manual_seed(0)
    m = NeRFNetworkStatic(bound=S.BOUND, min_near=S.MIN_NEAR, min_near_lidar=S.MIN_NEAR, lidar_max_depth=S.LIDAR_MAX_DEPTH, log2_hashmap_size=14)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for enc in (m.hash_encoder_lidar, m.hash_encoder_camera):
            enc.params.copy_(torch.randn(enc.params.shape, generator=g) * 0.1)
        m.sigma_net.params.mul_(2.0)
    return m.to(dev).eval()


@pytest.mark.parametrize("lidar", [True, False])
def test_density_gradient_is_its_operator_chain(ops, dev, field_model, lidar):
    """density_gradient equals the explicit chain of the four public operators bit for bit, its sigma is model.density's, and the
    normal is -grad / |grad|."""
    from nvsf.nerf import activation, normals
    m = field_model
    g = torch.Generator().manual_seed(5)
    x = ((torch.rand(1000, 3, generator=g) * 2 - 1) * m.bound).to(dev)
    out = normals.density_gradient(m, x, cal_lidar_color=lidar)
    enc, net = (m.hash_encoder_lidar if lidar else m.hash_encoder_camera), m.sigma_net
    with torch.no_grad():
        x01 = (x + m.bound) / (2 * m.bound)
        feat = ops.hashgrid_forward(x01, (0, 1, 2), enc.table_f16(), enc.spec)
        h = ops.mlp_forward(feat, net.weights_f16(), net.spec)
        one_hot = torch.zeros(x.shape[0], 16, device=dev)
        one_hot[:, 0] = 1.0
        g_feat, _ = ops.mlp_backward(feat, net.weights_f16(), net.spec, one_hot, grad_x_blocks=enc.spec.F)
        g_rows, _ = ops.mlp_backward(feat, net.weights_f16(), net.spec, one_hot)
        dh = ops.hashgrid_grad_x(x01, (0, 1, 2), enc.table_f16(), enc.spec, g_feat)
        assert torch.equal(dh, ops.hashgrid_grad_x(x01, (0, 1, 2), enc.table_f16(), enc.spec, g_rows))
        sigma = m.density(x, cal_lidar_color=lidar)["sigma"]
        assert torch.allclose(sigma, torch.exp(h[:, 0]), rtol=1e-5, atol=0)
        grad = (sigma.clamp(activation._LO, activation._HI).unsqueeze(-1) * dh) / (2 * m.bound)
    assert torch.equal(out["sigma"], sigma) and torch.equal(out["grad"], grad)
    assert set(out) == {"sigma", "grad", "normal"} and not out["grad"].requires_grad
    norm = grad.double().norm(dim=-1, keepdim=True)
    assert bool((norm > 0).all())
    assert torch.allclose(out["normal"].double(), -grad.double() / norm, rtol=0, atol=1e-6)


def test_density_gradient_on_an_exactly_linear_field(ops, dev):
    """Small-integer weights: the table of the exact case (feature 0 = x index: the encoded feature is pos_x = scale_l x + 0.5) and a
    sigma net whose four live hidden units sum the features through positive pre-activations, so d h0 / d feature is the same exact
    dyadic number for every sample, h0 is linear in x, normal == (-1, 0, 0) exactly and grad == sigma' a / (2 bound) with
    a = sum_l scale_l g_l, up to the bar of that sum and one fp32 rounding per multiply."""
    from nvsf.nerf import activation, normals
    from nvsf.nerf.models.network_static import NeRFNetworkStatic
    m = NeRFNetworkStatic(bound=1, base_resolution=4, max_resolution=64, n_levels_hash=5, n_features_per_level_hash=2, log2_hashmap_size=19)
    spec, net = m.hash_encoder_camera.spec, m.sigma_net.spec
    assert [float(s) for s in spec.scales] == [3.0, 7.0, 15.0, 31.0, 63.0] and net.n_in == 10 and net.in_cols == 16 and net.n_hidden == 1
    rng = np.random.default_rng(31)
    table = _index_table(spec, rng).reshape(-1, 2)
    table[:, 1] = 0
    W0 = np.zeros((64, 16))
    k = rng.integers(1, 4, (4, 5))
    W0[:4, 0:10:2] = k * 2.0 ** -8   # feature 0 of level l, hidden unit j
    W0[:4, 15] = 2.0 ** -4           # a padding column (reads 1.0): keeps every pre-activation positive
    W_out = np.zeros((16, 64))
    W_out[0, :4] = np.array([1, 2, 1, 3]) * 2.0 ** -3
    with torch.no_grad():
        m.hash_encoder_camera.params.copy_(torch.from_numpy(table.reshape(-1).astype(np.float32)))
        m.sigma_net.params.copy_(torch.from_numpy(np.concatenate([W0.reshape(-1), W_out.reshape(-1)]).astype(np.float32)))
    m = m.to(dev).eval()
    g_l = W_out[0, :4] @ W0[:4, 0:10:2]  # d h0 / d (feature 0 of level l)
    a = float((g_l * np.array(spec.scales)).sum())
    assert a > 0
    M = 300
    x = _t(((rng.random((M, 3)) * 0.75 + 0.05) * 2 - 1).astype(np.float32), dev)  # x01 in [0.05, 0.8]: no wrap, as in the exact case
    out = normals.density_gradient(m, x)
    assert bool((out["normal"] == torch.tensor([-1.0, 0.0, 0.0], device=dev)).all())
    assert bool((out["grad"][:, 1:] == 0).all())
    s = out["sigma"].clamp(activation._LO, activation._HI).double().cpu().numpy()
    assert s.min() > 1.0 and s.max() < 1e3
    want = s * a / 2.0
    rel = np.abs(out["grad"][:, 0].double().cpu().numpy() - want) / want
    bar = (spec.L * spec.F * 8 + 8) * U + 2 * U  # the final sum's bar as in the exact case (every g_l positive: sum_l scale_l |g_l| = a) + the two products
    print(f"linear field: largest relative error of grad_x = {rel.max():.3e}, bar {bar:.3e}")
    assert (rel <= bar).all()


def test_density_gradient_against_the_float64_restatement(dev):
    """The reference is the float64 gradient of the restated field (torch_f64_static.hash_features -> mlp -> exp) at 2048 points of a
    randomly initialised NeRFNetworkStatic.  The bar is measured from the reference alone: per sample, the distance between that
    restatement with the forward's fp16 rounding points and the same restatement without them (the documented size of the fp16
    regime), times 4 -- the MLP backward adds one fp16 rounding of the hidden gradient per layer.  Samples whose |grad sigma| is
    below 1e-6 of the batch maximum are left out, at most 1 % (tests/test_normals_cpu.py checks the cap on the restatement)."""
    from nvsf.nerf import normals
    from test_normals_cpu import f64_case
    m, x = f64_case()
    _, ref = GX.field_gradient_f64(m, x, lidar=True, rounded=True)
    _, plain = GX.field_gradient_f64(m, x, lidar=True, rounded=False)
    norm = np.linalg.norm(ref, axis=-1)
    keep = norm >= 1e-6 * norm.max()
    assert (~keep).sum() <= 0.01 * keep.size
    bar = 4.0 * np.linalg.norm(ref - plain, axis=-1)
    got = normals.density_gradient(m.to(dev), x.to(dev), cal_lidar_color=True)["grad"].double().cpu().numpy()
    err = np.linalg.norm(got - ref, axis=-1)
    ratio = err[keep] / bar[keep]
    print(f"density_gradient vs fp64: median |grad| {np.median(norm):.3e}; bar median {np.median(bar[keep]):.3e} min {bar[keep].min():.3e}; "
          f"error median {np.median(err[keep]):.3e} max {err[keep].max():.3e}; error / bar median {np.median(ratio):.4f} max {ratio.max():.4f}")
    assert (err[keep] <= bar[keep]).all(), float(ratio.max())


# ---- render_normals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lidar", [True, False])
def test_render_normals(dev, field_model, lidar):
    """64 rays x 96 samples: normal = sum_i w_i n_i of the function's own per-sample weights and normals (float64 sum; one fp32
    rounding per addend), weights_sum is model.render's on the same rays bit for bit (its operator chain: the same kernels in the same
    order), cos_incidence = -normal . d / |d|, and a chunked run equals the unchunked one bit for bit."""
    from nvsf import synthetic as S
    from nvsf.nerf import normals
    m = field_model
    N, T = 64, 96
    o, d = (S.lidar_rays if lidar else S.camera_rays)(N, np.random.default_rng(17))
    o, d = _t(o, dev), _t(d, dev)
    out = normals.render_normals(m, o, d, cal_lidar_color=lidar, num_steps=T, return_samples=True)
    assert out["normal"].shape == (N, 3) and out["weights_sum"].shape == (N,) and out["cos_incidence"].shape == (N,)
    w, n = out["weights"].double(), out["sample_normals"].double()
    assert bool((out["weights_sum"] > 1e-3).any()) and bool((n.norm(dim=-1) - 1).abs().max() < 1e-6)
    want = (w[:, :, None] * n).sum(1)
    tol = (T + 2) * U * (w[:, :, None] * n).abs().sum(1)
    assert bool(((out["normal"].double() - want).abs() <= tol).all())
    d_hat = d / d.norm(dim=-1, keepdim=True)
    assert torch.allclose(out["cos_incidence"], -(out["normal"] * d_hat).sum(-1), rtol=0, atol=1e-6)
    m.fused_train_forward = False  # model.render with autograd enabled then walks uniform_samples -> density -> compositor
    try:
        with torch.enable_grad():
            ref = m.render(o[None], d[None], torch.tensor([[0.5]], device=dev), cal_lidar_color=lidar, num_steps=T)
    finally:
        del m.fused_train_forward
    assert torch.equal(out["weights_sum"], ref["weights_sum_lidar" if lidar else "weights_sum"].detach())
    assert torch.equal(out["weights"], ref["weights"].detach())
    chunked = normals.render_normals(m, o, d, cal_lidar_color=lidar, num_steps=T, max_ray_batch=24)
    assert set(chunked) == {"normal", "weights_sum", "cos_incidence"}
    for key in chunked:
        assert torch.equal(chunked[key], out[key]), key


# ---- mesh export ---------------------------------------------------------------------------------------------------------------------
def test_mesh_export_with_vertex_normals(dev, field_model, tmp_path):
    from nvsf.nerf import mesh, normals
    m = field_model
    b_min, b_max, res = [-0.5, -0.5, 0.06], [0.5, 0.5, 0.09], (17, 33, 5)
    with torch.no_grad():
        u, _ = mesh.extract_fields(b_min, b_max, res, lambda p: m.density(p)["sigma"].float(), device=dev)
    thr = float(u.median())
    plain = mesh.export_mesh_density(m, str(tmp_path / "plain.ply"), bound_min=b_min, bound_max=b_max, xyz_res=res, threshold=thr)
    assert len(plain) == 2
    v, t, n = mesh.export_mesh_density(m, str(tmp_path / "normals.ply"), bound_min=b_min, bound_max=b_max, xyz_res=res, threshold=thr, normals=True)
    assert v.shape[0] > 0 and t.shape[0] > 0 and v.tobytes() == plain[0].tobytes() and np.array_equal(t, plain[1])
    assert n.dtype == np.float32 and n.shape == v.shape
    want = normals.density_gradient(m, torch.from_numpy(v.astype(np.float32)).to(dev))["normal"].cpu().numpy()
    assert n.tobytes() == want.tobytes()
    assert np.abs(np.linalg.norm(n, axis=-1) - 1).max() < 1e-6
    chunk = mesh._NORMAL_CHUNK
    mesh._NORMAL_CHUNK = 100  # several chunks, the last one short
    try:
        assert v.shape[0] > 250
        n_chunked = mesh.export_mesh_density(m, str(tmp_path / "chunked.ply"), bound_min=b_min, bound_max=b_max, xyz_res=res, threshold=thr, normals=True)[2]
    finally:
        mesh._NORMAL_CHUNK = chunk
    assert n_chunked.tobytes() == n.tobytes() and open(tmp_path / "chunked.ply", "rb").read() == open(tmp_path / "normals.ply", "rb").read()
    data = open(tmp_path / "normals.ply", "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode("ascii")
    assert f"element vertex {v.shape[0]}\n" in header and "property float nx\nproperty float ny\nproperty float nz\n" in header
    assert len(data) == end + 36 * v.shape[0] + 13 * t.shape[0]
    rec = np.frombuffer(data, np.dtype([("p", "<f8", (3,)), ("n", "<f4", (3,))]), v.shape[0], end)
    assert rec["p"].tobytes() == v.tobytes() and rec["n"].tobytes() == n.tobytes()
    faces = np.frombuffer(data, np.dtype([("k", "u1"), ("i", "<i4", (3,))]), t.shape[0], end + 36 * v.shape[0])
    assert (faces["k"] == 3).all() and np.array_equal(faces["i"], t)
