"""The restatements of the density tail and the flow MLP (tests/torch_f64_tail.py) checked WITHOUT a device: the input assembly against
the literal torch expression bit for bit, the MLPs against the CPU oracle, the whole chain (encoder restatements of
tests/torch_f64_dynamic.py -> flow layers -> density_tail) against the fixtures the reference's model produced on the CPU, and every
assertion the GPU cases of tests/test_dynamic_tail_gpu.py make about their own data (exact operands and sums, the cap on ReLU-fragile
rows).  tests/test_dynamic_tail_gpu.py then holds the HIP kernels to the restatements."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import golden_dynamic as GD  # noqa: E402
import oracle_lib as O  # noqa: E402
import test_dynamic_tail_gpu as G  # noqa: E402  (the seeded case builders; nothing in them touches a device)
import torch_f64_dynamic as T64  # noqa: E402
import torch_f64_static as S64  # noqa: E402
import torch_f64_tail as T  # noqa: E402

GOLD = os.path.join(HERE, "golden")


def _literal(plane_s, plane_d, plane_1, plane_2, hash_s, hash_d, hash_1, hash_2):
    """network_dynamic.py:273-287 as torch evaluates it, then what tcnn.Network does to its input: fp16, padded with ones."""
    plane_b = 0.5 * plane_d + 0.25 * (plane_1 + plane_2)
    hash_b = 0.5 * hash_d + 0.25 * (hash_1 + hash_2)
    row = torch.cat([plane_s, plane_b, hash_s, hash_b], dim=-1)
    assert row.dtype == torch.float32
    return torch.cat([row.half(), torch.ones(row.shape[0], 8, dtype=torch.float16)], -1)


@pytest.mark.parametrize("kind", ["random", "edges", "quarters"])
def test_tail_input_is_the_literal_expression_bit_for_bit(kind):
    """All four (hash_1, hash_2) dtype pairs; the four results differ from each other on these inputs (otherwise the regime flags would
    test nothing); handing the dtypes over as `half=` with float64 leaves gives the same bits."""
    M = 77
    base = {"random": G.random_features(M, 1), "edges": G.edge_features(M, 2), "quarters": G.quarter_features(M, 3)}[kind]
    outs = []
    for pair in G.PAIRS:
        feats = G.with_pair(base, pair)
        want = _literal(*feats)
        got = T.tail_input(*feats, dtype=torch.float32)
        assert got.dtype == torch.float32 and G.all_same_bits(got.half(), want) and G.all_same_bits(got.half().float(), got)
        got64 = T.tail_input(*[f.double() for f in feats], dtype=torch.float64, half=pair)
        assert G.all_same_bits(got64.half(), want)
        lm = list(feats)
        lm[4] = G.level_major(feats[4])
        assert G.all_same_bits(T.tail_input(*lm, dtype=torch.float32), got)
        outs.append(want)
        assert bool((want[:, 120:] == 1).all())
    if kind != "quarters":  # (multiples of 1/4 are exact in every regime: that is what the exact GPU case relies on)
        # (fp32, fp32) / one fp16 neighbour: the neighbour's own rounding; (fp16, fp16): also the sum's and the product's
        for i in range(4):
            for j in range(i + 1, 4):
                assert not G.all_same_bits(outs[i], outs[j]), (G.PAIRS[i], G.PAIRS[j])
        # ... and the half regime differs from "both neighbours rounded, then fp32 arithmetic"
        rounded = G.with_pair(G.with_pair(base, (True, True)), (False, False))
        assert not G.all_same_bits(_literal(*rounded), outs[3])
    else:
        assert all(G.all_same_bits(o, outs[0]) for o in outs)


def test_tail_input_gradient_is_the_blend_factors():
    """Float64 autograd through tail_input against autograd through the plain float64 expression (no rounding): the same numbers (powers
    of two), with plane_1 aliasing plane_d, with one blended tensor, and with level-major hash_s."""
    M = 9
    coef = torch.randn(M, 128, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    for kind in ("distinct", "alias", "blended"):
        for lm in (False, True):
            feats = G.with_pair(G.random_features(M, 4), (True, False))
            if lm:
                feats[4] = G.level_major(feats[4])
            a = G.alias_planes([f.double().requires_grad_() for f in feats], kind)
            b = G.alias_planes([f.double().requires_grad_() for f in feats], kind)
            (T.tail_input(*a, half=(True, False)) * coef).sum().backward()
            hs = b[4].permute(1, 0, 2).reshape(M, 32) if lm else b[4]
            plain = torch.cat([b[0], 0.5 * b[1] + 0.25 * (b[2] + b[3]), hs, 0.5 * b[5] + 0.25 * (b[6] + b[7])], -1)
            (plain * coef[:, :120]).sum().backward()
            for x, y in zip(a, b):
                assert torch.equal(x.grad, y.grad), (kind, lm)


def test_mlps_agree_with_the_c_oracle():
    """density_tail and flow_mlp in fp32 against oracle_lib.mlp_fwd on the same fp16 input, at the bars of test_mlp_forward."""
    spec = G.tail_spec()
    M = 3001
    feats = G.with_pair(G.random_features(M, 5), (True, True))
    W0, W1 = G.xavier(spec.shapes, 6)
    w = torch.cat([W0.reshape(-1), W1.reshape(-1)])
    sigma, geo, h, x = T.density_tail(*feats, w, spec, dtype=torch.float32)
    ref = O.mlp_fwd(x[:, :120].half().numpy(), w.half().numpy(), 120, 128, 1)
    scale = np.abs(ref).max()
    np.testing.assert_allclose(h.numpy(), ref, atol=1e-3 * scale, rtol=0)
    assert (np.abs(h.numpy() - ref) <= 2e-6 * scale).mean() > 0.97
    assert torch.equal(sigma, torch.exp(h[:, 0])) and torch.equal(geo, h[:, 1:16])
    xf, w0, w1, w2, _, _ = G.flow_random_case(M, 7, 1.0)
    from nvsf.nerf.models.flow_field import _pack_flow_weights
    ref = O.mlp_fwd(xf.half().numpy(), _pack_flow_weights(w0, w1, w2).numpy(), 32, 32, 2)
    got = T.flow_mlp(xf, w0, w1, w2).numpy()
    scale = np.abs(ref).max()
    assert got.shape == (M, 6) and not ref[:, 6:].any()
    np.testing.assert_allclose(got, ref[:, :6], atol=1e-3 * scale, rtol=0)
    assert (np.abs(got - ref[:, :6]) <= 2e-6 * scale).mean() > 0.97


# ---- what the GPU cases assert about their own data, checked here ------------------------------------------------------------------------
@pytest.mark.parametrize("M", G.M_FORWARD)
def test_exact_forward_case_is_exact(M):
    G.exact_forward_reference(M)


@pytest.mark.parametrize("case", list(G.TAIL_EXACT_CASES))
def test_exact_tail_cases_are_exact(case):
    for M in G.M_TAIL_EXACT:
        feats, kind, w, g_sigma, g_geo, grads = G.tail_exact_reference(M, case)
        needs = G.TAIL_EXACT_CASES[case][3]
        assert all((g is not None) == (slot in needs) for slot, g in enumerate(grads))
        # (without a geometry gradient only the zero logit row of the output layer receives one: sigma == 1 whatever the input is)
        assert M == 1 or (bool(grads[8].any()) if 8 in needs else True)
        assert M == 1 or not G.TAIL_EXACT_CASES[case][5] or all(bool(g.any()) for g in grads if g is not None)


def test_exact_flow_cases_are_exact():
    for M in G.M_FLOW:
        case, out, gx, gw = G.flow_exact_reference(M)
        assert gw[2].shape == (6, 64) and (M == 1 or (bool(out.any()) and bool(gx.any()) and all(bool(g.any()) for g in gw)))


def test_random_cases_stay_within_the_fragile_cap():
    """The seeds of the random GPU cases: at most MAX_FRAGILE rows each are set aside by the restatement's own rule, the sizes are the
    ones the issue names, and the "edges" logits do spread beyond trunc_exp's clamp on both sides."""
    assert sorted({c[0] for c in G.TAIL_RANDOM_CASES.values()}) == list(G.M_TAIL_RANDOM)
    assert sorted({c[0] for c in G.FLOW_RANDOM_CASES.values()}) == list(G.M_FLOW)
    for name, (M, seed, edges, pair, lm, kind) in G.TAIL_RANDOM_CASES.items():
        feats, w, g_sigma, g_geo, n = G.tail_random_case(M, seed, edges, pair, kind)
        assert n <= G.MAX_FRAGILE, name
        if edges and M > 100:
            h0 = T.density_tail(*feats, w.double(), G.tail_spec(), half=pair)[2][:, 0]
            assert float(h0.max()) > 15 and float(h0.min()) < -15, name
            scaled = 128.0 * g_sigma.double() * torch.exp(h0).clamp(S64._LO, S64._HI)
            assert float(scaled.abs().max()) < 65504.0, name  # the scaled logit gradient stays inside fp16
    for name, (M, seed, g_scale) in G.FLOW_RANDOM_CASES.items():
        assert G.flow_random_case(M, seed, g_scale)[-1] <= G.MAX_FRAGILE, name


def test_fragile_rows_rule():
    """A pre-activation that cancels to 2^-21 of its addends is flagged, one at 2^-19 is not, an exact zero of zeros is not."""
    W = torch.zeros(64, 128)
    W[0, 0], W[0, 1] = 1.0, -1.0
    x = torch.zeros(3, 128, dtype=torch.float64)
    x[0, 0], x[0, 1] = 1.0, 1.0 - 2.0 ** -20       # 2^-20 of a sum of 2: 2^-21 relative
    x[1, 0], x[1, 1] = 1.0, 1.0 - 2.0 ** -18
    assert T.fragile_rows(x, [W]).tolist() == [True, False, False]


# ---- the mutation list of tools/mutate_f64_tail.py ---------------------------------------------------------------------------------------
def test_wrong_variants_of_the_restatement_still_apply():
    import importlib.util
    spec = importlib.util.spec_from_file_location("mutate_f64_tail", os.path.join(os.path.dirname(HERE), "tools", "mutate_f64_tail.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    clean = open(tool.SOURCE).read()
    assert set(tool.VARIANTS) == {"swap_factors", "drop_half_rounding", "pad_zeros", "no_clamp", "swap_levels", "blended_half"}
    for name in tool.VARIANTS:
        for old, _ in tool.VARIANTS[name][1]:
            assert clean.count(old) == 1, (name, old)
        text = tool.mutated_source(name)
        assert text != clean
        compile(text, name, "exec")


# ---- chain anchor: encoder restatements -> flow layers -> density_tail against the reference's CPU fixture ----------------------------------
@pytest.fixture(scope="module")
def anchor_model():
    from nvsf import synthetic as S
    from nvsf.nerf.models.network_dynamic import NeRFNetwork
    m = NeRFNetwork(min_near=S.MIN_NEAR, min_near_lidar=S.MIN_NEAR, lidar_max_depth=S.LIDAR_MAX_DEPTH, **GD.SMALL).eval()
    GD.init_by_name(m)
    return m


def _chain(m, pts, tv, lidar):
    """density(pts, t) of network_dynamic.py:213-287 from the restatements alone -> sigma, geo [M, 15] (float64) and the dtype pair."""
    F = m.num_frames
    hash_enc = m.hash_encoder_lidar if lidar else m.hash_encoder_camera
    planes_enc = m.planes_encoder_lidar if lidar else m.planes_encoder_camera
    x = (pts + m.bound) / (2 * m.bound)
    t_host = float(np.float32(tv))
    frame = int(np.float32(t_host) * np.float32(F - 1))
    # flow: grid + Lagrange reduction, the three Linear layers in float64 (a CPU time tensor: true division in the Lagrange weights)
    fl = m.flow_net
    h = T64.flow_grid_features(x, fl.grid_enc.params.detach().double(), fl.grid_enc.spec, t_host, reciprocal_division=False)
    lin = [l for l in fl.mlp if isinstance(l, torch.nn.Linear)]
    for j, layer in enumerate(lin):
        h = h @ layer.weight.detach().double().t()
        if j + 1 < len(lin):
            h = torch.relu(h)
    flow = h.float()
    nb = [np.float32(f / F) if 0 <= f <= F - 1 else None for f in (frame + 1, frame - 1)]  # torch.tensor(frame / F): fp32
    planes = planes_enc.planes_cl.detach().double()
    plane_s, plane_d, plane_1, plane_2 = T64.planes_multi_features(x, flow, planes, planes_enc._res_host, t_host, nb[0], nb[1])
    tables = [[pl.hash_t[k].params.detach().double() for k in range(pl.time_resolution)] for pl in hash_enc.hash_dynamic]
    specs = [pl.hash_t[0].spec for pl in hash_enc.hash_dynamic]
    R = hash_enc.hash_dynamic[0].time_resolution
    hash_s = T64.grid_features(x, hash_enc.hash_static.params.detach().double(), hash_enc.hash_static.spec, (0, 1, 2)).reshape(x.shape[0], -1).half()
    hash_d = T64.hash_time_features(x, tables, specs, R, t_host, reciprocal_division=False).float()
    hn = []
    for tn, col in zip(nb, (0, 3)):
        hn.append(None if tn is None else T64.hash_time_features_f16(x + flow[:, col:col + 3], tables, specs, R, float(tn), reciprocal_division=False))
    f32 = lambda v: v.float()
    plane_d = f32(plane_d)
    feats = [f32(plane_s), plane_d, plane_d if plane_1 is None else f32(plane_1), plane_d if plane_2 is None else f32(plane_2),
             hash_s, hash_d, hash_d if hn[0] is None else hn[0], hash_d if hn[1] is None else hn[1]]
    pair = (feats[6].dtype == torch.float16, feats[7].dtype == torch.float16)
    sigma, geo, _, _ = T.density_tail(*feats, m.sigma_net.params.detach().double(), m.sigma_net.spec)
    return sigma, geo, pair


@pytest.mark.parametrize("tag,tv,pair", [("mid", 0.5, (True, True)), ("first", 0.0, (True, False)), ("last", 1.0, (False, True))])
def test_chain_reproduces_the_reference_density(anchor_model, tag, tv, pair):
    """The `pts` of network_dynamic.npz through the composition above: density_{mid,first,last}_{1,0}_{sigma,geo} at the tolerances
    test_network_density_and_flow applies to the kernels (sigma rtol 3e-3 / atol 1e-6, geo 3e-3 of the largest entry).  The three
    frames are three of the four dtype regimes of the hash blend: both neighbours fp16, only the next, only the previous."""
    g = np.load(os.path.join(GOLD, "network_dynamic.npz"))
    pts = torch.from_numpy(g["pts"])
    for lidar in (1, 0):
        sigma, geo, got_pair = _chain(anchor_model, pts, tv, bool(lidar))
        assert got_pair == pair
        sr, gr = g[f"density_{tag}_{lidar}_sigma"], g[f"density_{tag}_{lidar}_geo"]
        np.testing.assert_allclose(sigma.numpy(), sr, rtol=3e-3, atol=1e-6, err_msg=f"{tag} {lidar}")
        np.testing.assert_allclose(geo.numpy(), gr, atol=3e-3 * np.abs(gr).max(), rtol=0, err_msg=f"{tag} {lidar}")
