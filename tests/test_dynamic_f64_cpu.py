"""The float64 restatements of the space-time encoders (tests/torch_f64_dynamic.py) checked WITHOUT a device: against torch's own
float64 grid_sample and its autograd, against the fixtures the reference's model files produced on the CPU (planes4d.npz,
hash4d_flow.npz) and against the CPU oracle's hash-grid lookup.  tests/test_dynamic_f64_gpu.py then holds the HIP kernels to them."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import golden_dynamic as GD  # noqa: E402
import torch_f64_dynamic as T64  # noqa: E402

GOLD = os.path.join(HERE, "golden")
RES = [32, 32, 32, 8]
MULT = [1, 2, 4, 8]


def _res_host():
    return tuple(v for m in MULT for v in [r * m for r in RES[:3]] + RES[3:])


def _planes(seed=0):
    """The channel-last parameter of Planes4D(resolution=[32, 32, 32, 8], multiscale_res=[1, 2, 4, 8]): spatial planes in [0.1, 0.5],
    time planes around 1."""
    g = torch.Generator().manual_seed(seed)
    pieces = []
    for _, q, _, H, W in T64.plane_layout(_res_host()):
        v = torch.rand(H * W * T64.C, generator=g, dtype=torch.float64)
        pieces.append(1.0 + 0.4 * (v - 0.5) if T64.PLANE_PAIRS[q][1] == 3 else 0.1 + 0.4 * v)
    return torch.cat(pieces).float().double()  # fp32 values


def _torch_reference(xt64, planes64, res_host, g_s, g_d):
    """F.grid_sample in float64 (bilinear, align_corners, border padding) on the 24 planes as [1, C, H, W] leaves, products and
    concatenation as the reference writes them; -> static, dynamic, d/d xt, the plane gradients in the channel-last layout."""
    xt = xt64.clone().requires_grad_()
    leaves, outs = [], [[], []]
    layout = T64.plane_layout(res_host)
    for s in range(len(res_host) // 4):
        feats = [None, None]
        for q, (a, b) in enumerate(T64.PLANE_PAIRS):
            _, _, off, H, W = layout[6 * s + q]
            leaf = planes64[off:off + H * W * T64.C].view(H, W, T64.C).permute(2, 0, 1)[None].clone().requires_grad_()
            leaves.append(leaf)
            grid = (torch.stack([xt[:, a], xt[:, b]], -1) * 2.0 - 1.0)[None, :, None, :]
            v = F.grid_sample(leaf, grid, mode="bilinear", padding_mode="border", align_corners=True)[0, :, :, 0].t()
            grp = 1 if b == 3 else 0
            feats[grp] = v if feats[grp] is None else feats[grp] * v
        outs[0].append(feats[0])
        outs[1].append(feats[1])
    s_, d_ = torch.cat(outs[0], -1), torch.cat(outs[1], -1)
    ((s_ * g_s).sum() + (d_ * g_d).sum()).backward()
    g_planes = torch.cat([l.grad[0].permute(1, 2, 0).reshape(-1) for l in leaves])
    return s_.detach(), d_.detach(), xt.grad, g_planes


def _mine(xt32, planes64, res_host, g_s, g_d):
    leaf = xt32.double().requires_grad_()
    p = planes64.clone().requires_grad_()
    s_, d_ = T64.planes_features(xt32, p, res_host, 3, xt_leaf=leaf)
    ((s_ * g_s).sum() + (d_ * g_d).sum()).backward()
    return s_.detach(), d_.detach(), leaf.grad, p.grad


def _derived_bars(xt32, planes64, res_host, g_s, g_d):
    """What the fp32 rounding of u may move, derived.  make_axis rounds u = p (R - 1) once (p 2 - 1 + 1 and / 2 are exact for p in
    (0, 1)): |du| <= 2^-24 u < 2^-23 (R - 1) with room to spare.  With D_a, D_b the largest texel difference of a plane along its two
    axes and V its largest texel, a plane's bilinear value moves by dv <= du_a D_a + du_b D_b, a bilinear weight by dw <= du_a + du_b, the
    derivative along a by du_b 2 D_a (a difference of two differences).  Features are products of three plane values; a plane-gradient
    addend is g (v_i v_k) w, a coordinate-gradient addend g (v_i v_k) (R_a - 1) dv_j / du_a.  -> bars for the feature rows [S 8] (static,
    dynamic), per texel entry of the channel-last parameter, and per row and coordinate [M, 4]."""
    layout = T64.plane_layout(res_host)
    M = xt32.shape[0]
    eps = 2.0 ** -23
    bar_feat = [[], []]
    bar_planes = torch.zeros_like(planes64)
    bar_xt = torch.zeros(M, 4, dtype=torch.float64)
    for s in range(len(res_host) // 4):
        r = [int(v) for v in res_host[4 * s:4 * s + 4]]
        du = [eps * (R - 1) for R in r]
        cells = [T64._axis(xt32[:, d], r[d])[2:4] for d in range(4)]
        for grp in (0, 1):
            qs = T64._GROUPS[grp]
            g = (g_s if grp == 0 else g_d)[:, s * 8:(s + 1) * 8].abs()
            V, dv, Da = [], [], []
            for q in qs:
                a, b = T64.PLANE_PAIRS[q]
                _, _, off, H, W = layout[6 * s + q]
                tex = planes64[off:off + H * W * 8].view(H, W, 8)
                d_a, d_b = float((tex[:, 1:] - tex[:, :-1]).abs().max()), float((tex[1:] - tex[:-1]).abs().max())
                V.append(float(tex.abs().max()))
                dv.append(du[a] * d_a + du[b] * d_b)
                Da.append((d_a, d_b))
            bar_feat[grp].append(sum(dv[j] * V[(j + 1) % 3] * V[(j + 2) % 3] for j in range(3)) * torch.ones(8, dtype=torch.float64))
            for j, q in enumerate(qs):
                a, b = T64.PLANE_PAIRS[q]
                _, _, off, H, W = layout[6 * s + q]
                i, k = (j + 1) % 3, (j + 2) % 3
                d_other = dv[i] * V[k] + dv[k] * V[i]
                per_addend = d_other + V[i] * V[k] * (du[a] + du[b])  # w <= 1
                n_abs = torch.zeros(H * W, 8, dtype=torch.float64)  # sum of |g| over the rows that touch the texel
                for cb in cells[b]:
                    for ca in cells[a]:
                        n_abs.index_add_(0, cb * W + ca, g)
                bar_planes[off:off + H * W * 8] += (per_addend * n_abs).reshape(-1)
                gsum = g.sum(-1)
                bar_xt[:, a] += gsum * (r[a] - 1) * (d_other * Da[j][0] + V[i] * V[k] * du[b] * 2 * Da[j][0])
                bar_xt[:, b] += gsum * (r[b] - 1) * (d_other * Da[j][1] + V[i] * V[k] * du[a] * 2 * Da[j][1])
    return torch.cat(bar_feat[0]), torch.cat(bar_feat[1]), bar_planes, bar_xt


def _generic_rows(n, res_host, seed):
    """n rows of (0, 1)^4 whose u = p (R - 1) is at least 1e-3 away from an integer on every axis of every scale."""
    g = torch.Generator().manual_seed(seed)
    xt = torch.rand(4 * n, 4, generator=g)
    ok = torch.ones(4 * n, dtype=torch.bool)
    for s in range(len(res_host) // 4):
        for d in range(4):
            u = xt[:, d].double() * (res_host[4 * s + d] - 1)
            ok &= (u - torch.round(u)).abs() >= 1e-3
    xt = xt[ok][:n]
    assert xt.shape[0] == n
    return xt


def _gradients(M, width, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(M, width, generator=g, dtype=torch.float64), torch.randn(M, width, generator=g, dtype=torch.float64)


def test_planes_restatement_equals_float64_grid_sample_on_generic_rows():
    """2000 random rows away from every cell boundary: values, ALL 24 plane gradients and the coordinate gradients against
    F.grid_sample in float64 and its autograd.  The only difference is the fp32 rounding of u; the bars are derived from it
    (_derived_bars), nothing measured."""
    res = _res_host()
    planes = _planes()
    xt = _generic_rows(2000, res, 1)
    g_s, g_d = _gradients(2000, 32, 2)
    ref = _torch_reference(xt.double(), planes, res, g_s, g_d)
    got = _mine(xt, planes, res, g_s, g_d)
    b_s, b_d, b_p, b_x = _derived_bars(xt, planes, res, g_s, g_d)
    worst = {}
    for name, a, b, bar in (("static", got[0], ref[0], b_s[None]), ("dynamic", got[1], ref[1], b_d[None]), ("grad_xt", got[2], ref[2], b_x),
                            ("grad_planes", got[3], ref[3], b_p)):
        err = (a - b).abs()
        worst[name] = (float(err.max()), float((err / (bar + 1e-300)).max()))
        assert bool((err <= bar + 1e-15).all()), (name, worst[name])
    print("planes restatement against float64 grid_sample: (largest error, largest share of its derived bar)", worst)
    assert float(got[3].abs().max()) > 0 and float(got[2].abs().max()) > 0
    # every one of the 24 planes received a gradient and was compared
    for _, _, off, H, W in T64.plane_layout(res):
        assert bool(ref[3][off:off + H * W * 8].any())


def test_planes_restatement_border_rows():
    """Rows exactly at 0 and at 1 and outside the box: the same values as torch's float64 grid_sample and a zero coordinate gradient
    on the clamped axis, as torch gives it; the other axes of those rows within the derived bars."""
    res = _res_host()
    planes = _planes()
    xt = _generic_rows(64, res, 3)
    edge = [0.0, 1.0, -0.25, 1.25, -0.0]
    clamped = torch.zeros(64, 4, dtype=torch.bool)
    for i in range(64):
        d = i % 4
        xt[i, d] = edge[(i // 4) % len(edge)]
        clamped[i, d] = True
        if i >= 40:  # two clamped axes in one row
            xt[i, (d + 1) % 4] = edge[(i // 4 + 1) % len(edge)]
            clamped[i, (d + 1) % 4] = True
    g_s, g_d = _gradients(64, 32, 4)
    ref = _torch_reference(xt.double(), planes, res, g_s, g_d)
    got = _mine(xt, planes, res, g_s, g_d)
    b_s, b_d, b_p, b_x = _derived_bars(xt, planes, res, g_s, g_d)
    assert bool(((got[0] - ref[0]).abs() <= b_s[None] + 1e-15).all()) and bool(((got[1] - ref[1]).abs() <= b_d[None] + 1e-15).all())
    assert not bool(ref[2][clamped].any()) and not bool(got[2][clamped].any())  # torch passes no gradient at or beyond the border
    assert bool(((got[2] - ref[2]).abs() <= b_x + 1e-15).all())
    assert bool(((got[3] - ref[3]).abs() <= b_p + 1e-15).all())
    assert bool(got[2][~clamped].any())


def test_planes_restatement_against_the_reference_fixture():
    """planes4d.npz (the reference's Planes4D on the CPU, fp32): values, grad_xt and the three stored plane gradients, at the tolerances
    of test_planes4d_forward_backward or tighter (values 1e-5, grad_xt 2e-3, plane gradients 2e-4)."""
    from nvsf.nerf.models.planes_field import Planes4D
    g = np.load(os.path.join(GOLD, "planes4d.npz"))
    enc = Planes4D(resolution=[8, 8, 8, 5], multiscale_res=[1, 2, 4, 8])
    GD.init_by_name(enc)
    xt = torch.from_numpy(g["xt"])
    leaf = xt.double().requires_grad_()
    p = enc.planes_cl.detach().double().requires_grad_()
    s_, d_ = T64.planes_features(xt, p, enc._res_host, 3, xt_leaf=leaf)
    np.testing.assert_allclose(s_.detach().numpy(), g["static"], atol=1e-5, rtol=1e-5)
    np.testing.assert_allclose(d_.detach().numpy(), g["dynamic"], atol=1e-5, rtol=1e-5)
    ((s_ * torch.from_numpy(g["grad_static"]).double()).sum() + (d_ * torch.from_numpy(g["grad_dynamic"]).double()).sum()).backward()
    np.testing.assert_allclose(leaf.grad.numpy(), g["grad_xt"], atol=2e-3, rtol=2e-3)
    for (si, pi), key in (((0, 0), "grad_plane_0_0"), ((3, 5), "grad_plane_3_5"), ((2, 3), "grad_plane_2_3")):
        np.testing.assert_allclose(enc._view(p.grad, si, pi).numpy(), g[key], atol=2e-4, rtol=2e-4)


@pytest.fixture(scope="module")
def hash_case():
    from nvsf.nerf.models.hash_field import HashGrid4D
    g = np.load(os.path.join(GOLD, "hash4d_flow.npz"))
    enc = HashGrid4D(base_resolution=16, max_resolution=256, time_resolution=4, n_levels=8, n_features_per_level=4, log2_hashmap_size=12)
    GD.init_by_name(enc)
    tables = [[pl.hash_t[k].params.detach().double() for k in range(4)] for pl in enc.hash_dynamic]
    specs = [pl.hash_t[0].spec for pl in enc.hash_dynamic]
    return g, torch.from_numpy(g["x"]), tables, specs


def test_hash_time_restatement_against_the_reference_fixture(hash_case):
    """hash4d_flow.npz: regime 0 (`dyn_t11_*`, atol 1e-6 / rtol 1e-5) and regime 1 (`dyn_t0_*`, 2e-3 of the largest entry) at all five
    times, the tolerances of test_hashgrid4d_and_flow, every element.  The fixture's t was a CPU tensor: true division in the Lagrange
    weights.  With rounding="sum" (the float64 sum itself rounded to fp16) a few regime-0 features land on the other side of an fp16
    boundary than the fp32 chain of the reference and of the kernels: they are counted and printed, not hidden."""
    g, x, tables, specs = hash_case
    flips = 0
    for i in range(5):
        tv = float(g[f"t{i}"])
        out = T64.hash_time_features(x, tables, specs, 4, tv, reciprocal_division=False)
        np.testing.assert_allclose(out.numpy(), g[f"dyn_t11_{i}"], atol=1e-6, rtol=1e-5)
        out0 = T64.hash_time_features_f16(x, tables, specs, 4, tv, reciprocal_division=False)
        assert out0.dtype == torch.float16
        ref0 = g[f"dyn_t0_{i}"].astype(np.float32)
        np.testing.assert_allclose(out0.float().numpy(), ref0, atol=2e-3 * np.abs(ref0).max(), rtol=0)
        alt = T64.hash_time_features(x, tables, specs, 4, tv, reciprocal_division=False, rounding="sum").numpy()
        ref = g[f"dyn_t11_{i}"]
        flips += int((np.abs(alt - ref) > 1e-6 + 1e-5 * np.abs(ref)).sum())
    print("regime-0 features where the float64 sum rounds to the other fp16 neighbour than the fp32 chain:", flips, "of", 5 * 600 * 24)
    assert flips <= 5 * 600 * 24 // 1000  # near-ties are rare: more would mean the two roundings disagree for another reason


def test_flow_grid_restatement_against_the_reference_fixture():
    """The fixture stores the flow, not the reduced grid features: the three bias-free Linear layers (ReLU between) are applied in
    float64 to the restated features; atol 1e-5 / rtol 1e-4 as test_hashgrid4d_and_flow."""
    from nvsf.nerf.models.flow_field import FlowField
    g = np.load(os.path.join(GOLD, "hash4d_flow.npz"))
    flow = FlowField(n_levels=16, n_features_per_level=8, base_resolution=32, max_resolution=8192, log2_hashmap_size=14)
    GD.init_by_name(flow)
    xt = torch.from_numpy(g["flow_xt"])
    h = T64.flow_grid_features(xt, flow.grid_enc.params.detach().double(), flow.grid_enc.spec, float(xt[0, 3]), reciprocal_division=False)
    lin = [m for m in flow.mlp if isinstance(m, torch.nn.Linear)]
    for j, layer in enumerate(lin):
        h = h @ layer.weight.detach().double().t()
        if j + 1 < len(lin):
            h = torch.relu(h)
    np.testing.assert_allclose(h.numpy(), g["flow"], atol=1e-5, rtol=1e-4)


def test_two_column_lookup_equals_the_cpu_oracle(hash_case):
    """grid_features with a column pair against oracle_lib.hashgrid_fwd (the CPU oracle's fp32 lookup, rounded to fp16), on the fixture's
    points and on points on grid nodes, outside the box and at the box faces: bit-equal with the chain rounding; with rounding="sum"
    the near-ties are counted and printed."""
    import oracle_lib as O
    g, x, tables, specs = hash_case
    rng = np.random.default_rng(5)
    extra = rng.random((300, 3)).astype(np.float32)
    extra[:40] = np.round(extra[:40] * 15) / 15           # nodes of the dense first level (scale 15)
    extra[40:60] = extra[40:60] * 1.5 - 0.25              # outside the box on some axes
    extra[60:70, 0], extra[70:80, 1], extra[80:90, 2] = 0.0, 1.0, np.nextafter(np.float32(1), np.float32(0))
    xs = torch.cat([x, torch.from_numpy(extra)])
    ties = total = 0
    for pl, cols in enumerate(T64.HASH_PAIRS):
        spec = specs[pl]
        for k in (0, 3):
            want = O.hashgrid_fwd(xs.numpy(), cols, tables[pl][k].half().numpy(), spec)
            got = T64.grid_features(xs, tables[pl][k], spec, cols).reshape(xs.shape[0], -1).half().numpy()
            assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
            alt = T64.grid_features(xs, tables[pl][k], spec, cols, rounding="sum").reshape(xs.shape[0], -1).half().numpy()
            diff = alt.view(np.uint16) != want.view(np.uint16)
            assert float(np.abs(alt.astype(np.float32) - want.astype(np.float32))[diff].max(initial=0.0)) <= 2.0 ** -10 * float(np.abs(want).max())
            ties += int(diff.sum())
            total += diff.size
    print("slice features where the float64 sum rounds to the other fp16 neighbour than the oracle's fp32 chain:", ties, "of", total)
    assert ties <= total // 1000


def test_absolute_value_restatements_bound_the_signed_ones(hash_case):
    """abs_sum=True is the same expression on |addends|: it dominates the signed value entry by entry, for features and gradients."""
    g, x, tables, specs = hash_case
    leaves = [[t.clone().requires_grad_() for t in row] for row in tables]
    w = torch.randn(600, 24, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    out = T64.hash_time_features(x, leaves, specs, 4, 0.77)
    (out * w).sum().backward()
    ab = [[t.clone().requires_grad_() for t in row] for row in tables]
    out_a = T64.hash_time_features(x, ab, specs, 4, 0.77, abs_sum=True)
    (out_a * w.abs()).sum().backward()
    assert bool((out.detach().abs() <= out_a.detach() * (1 + 1e-3)).all())
    for row, row_a in zip(leaves, ab):
        for k, (t, ta) in enumerate(zip(row, row_a)):
            if t.grad is None:
                assert k not in (2, 3)
                continue
            assert bool((t.grad.abs() <= ta.grad * (1 + 1e-12) + 1e-300).all())
    res = _res_host()
    planes = _planes()
    xt = _generic_rows(200, res, 9)
    g_s, g_d = _gradients(200, 32, 10)
    got = _mine(xt, planes, res, g_s, g_d)
    leaf, p = xt.double().requires_grad_(), planes.clone().requires_grad_()
    s_, d_ = T64.planes_features(xt, p, res, 3, abs_sum=True, xt_leaf=leaf)
    ((s_ * g_s.abs()).sum() + (d_ * g_d.abs()).sum()).backward()
    assert bool((got[2].abs() <= leaf.grad * (1 + 1e-12)).all()) and bool((got[3].abs() <= p.grad * (1 + 1e-12)).all())
    assert bool((leaf.grad >= 0).all()) and bool((p.grad >= 0).all())


def test_wrong_variants_of_the_restatement_still_apply():
    """tools/mutate_f64_dynamic.py validates the GPU pins by running them against deliberately wrong copies of the restatement; each of its
    edits must still match the restatement's text (a variant that no longer applies would count as caught for the wrong reason), change
    it, and leave it importable."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("mutate_f64_dynamic", os.path.join(os.path.dirname(HERE), "tools", "mutate_f64_dynamic.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    clean = open(tool.SOURCE).read()
    assert set(tool.VARIANTS) == {"swap_blend", "drop_lagrange", "grad_at_clamp", "floor_f64", "blend_quarter"}
    for name in tool.VARIANTS:
        text = tool.mutated_source(name)
        assert text != clean
        compile(text, name, "exec")
