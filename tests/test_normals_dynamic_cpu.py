"""CPU tests of the oracles behind the space-time model's coordinate gradient: the float64 statement of the
time-sliced 2-D grids' gradient against central differences of its own feature function, the float64 chain (K-planes, hash grids, flow
warp, both MLPs) against central differences of its own h0, and the seed check of the GPU test that compares density_gradient with
that chain.  Nothing here needs a device."""
import numpy as np
import torch

import dynamic_gradx_oracle as DX
import hash4d_gradx_oracle as H4


def _pair_specs(log2_sizes, base, top):
    from nvsf.field_ops import GridSpec
    pls = float(np.exp2(np.log2(top / base) / 7))
    return [GridSpec(2, 8, 4, t, base, pls) for t in log2_sizes]


def test_hash_oracle_equals_central_differences_of_its_float64_features():
    """L(p) = sum g . features(p) is linear along an axis inside a cell, so its central difference with a step that stays inside the
    cell on every level of every pair IS the derivative, up to the float64 rounding of the two evaluations divided by the step.
    Points j / 1024 with the integer scales 2^(l + 1) - 1 make pos = scale p + 0.5 exact in fp32 (the oracle's fp32 cells and fracs are
    the float64 function's); pos sits on a face only for j = 512, which is not drawn, and is at least 1 / 1024 from one otherwise:
    1 / (1024 * 255) of p, above the step 2^-18.  t on a slice (one table per pair) and between two slices."""
    from nvsf.nerf.models.hash_field import time_slot
    specs = _pair_specs((11, 9, 10), 2, 256)
    assert [float(s) for s in specs[0].scales] == [2.0 ** (l + 1) - 1 for l in range(8)]
    rng = np.random.default_rng(21)
    M, step, R = 300, 2.0 ** -18, 3
    j = rng.integers(1, 512, (M, 3)) + 512 * rng.integers(0, 2, (M, 3))
    p = (j / 1024.0).astype(np.float32)
    margin = H4.face_margin(p, specs)
    assert int((margin > step).sum()) == M  # no point dropped
    slices = [[(rng.standard_normal(s.n_params) * 0.5).astype(np.float16) for s in specs] for _ in range(R)]
    g = rng.standard_normal((M, 24))
    seen = set()
    for t in (0.5, 0.3):
        slot = time_slot(torch.tensor(t), t, R)
        seen.add(slot.same)
        tables = slices[slot.k1] + slices[slot.k2]
        got, A = H4.grad_x(p, tables, specs, slot, g, grad_scale=0.25)
        n_add = 256 if slot.same else 512
        for d in range(3):
            e = np.zeros(3)
            e[d] = step
            hi = (0.25 * g * H4.features(p.astype(np.float64) + e, tables, specs, slot)).sum(-1)
            lo = (0.25 * g * H4.features(p.astype(np.float64) - e, tables, specs, slot)).sum(-1)
            cd = (hi - lo) / (2 * step)
            # each evaluation: n_add addends of a few float64 roundings each, |addend| <= A's addend / scale_0 (= 1); divided by the step
            tol = (n_add + 8) * 2.0 ** -53 * A[:, d] / (float(specs[0].scales[0]) * step)
            err = np.abs(got[:, d] - cd)
            assert (err <= tol).all(), (t, d, float((err / tol).max()))
            assert np.abs(cd).max() > 1.0  # the comparison is not of zeros
    assert seen == {True, False}


def chain_case(n_points=2048):
    """The model and points of the comparison of density_gradient with the float64 chain (tests/test_normals_dynamic_gpu.py), built on
    the CPU: a small NeRFNetwork with random hash tables (freshly constructed ones give sigma == 1 everywhere) and a flow field whose
    last layer is scaled up until the warped positions leave the base cell on the finest level of the time-sliced grids (scale 255)."""
    from nvsf.nerf.models.network_dynamic import NeRFNetwork
    torch.manual_seed(0)
    m = NeRFNetwork(time_resolution=3, num_frames=9, bound=2.0, min_resolution=8, base_resolution=16, max_resolution=256, log2_hashmap_size=12)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for enc in (m.hash_encoder_lidar, m.hash_encoder_camera):
            for p in enc.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
        # the flow grid: level l with amplitude 0.5 scale_0 / scale_l -- a field whose slope is the same on every level, as a fitted one's
        # is; with one amplitude for all 16 levels the finest (scale 8192) would move the flow MLP's input by 1e-4 of itself per 2^-24 of
        # position and a per cent of the points would sit within that of a ReLU switching
        spec = m.flow_net.grid_enc.spec
        table = torch.randn(spec.n_rows, spec.F, generator=g) * 0.5
        for l in range(spec.L):
            table[int(spec.offsets[l]):int(spec.offsets[l + 1])] *= float(spec.scales[0]) / float(spec.scales[l])
        m.flow_net.grid_enc.params.copy_(table.reshape(-1))
        m.flow_net.mlp[-1].weight.mul_(FLOW_GAIN)
        m.sigma_net.params.mul_(2.0)
    x = (torch.rand(n_points, 3, generator=g) * 3.8 - 1.9).float()
    return m.eval(), x


FLOW_GAIN = 40.0
FRAME_TIMES = {"first": 0.0, "interior": 0.5, "last": 1.0}  # frames 0, 4 and 8 of 9


def test_chain_oracle_equals_central_differences_of_its_own_h0():
    """With every position, cell and frac in float64 the chain is the exact derivative of the float64 h0(u) wherever h0 is smooth:
    inside a cell of every grid at the three positions u, u + f1, u + f2 and with no hidden unit of either MLP switching.  Points
    within the step of a cell face (expected ~0.6 %: per axis of the flow grid 2 step sum_l scale_l ~ 0.2 % at a finest scale of
    8192, the other grids are coarser) or whose ReLU gates differ between the two evaluations are left out, at most 5 %.
    Tolerance: the float64 rounding of the two evaluations -- K = 4096 roundings' worth of 2^-53 of `habs`, the sum of the |addend|
    behind h0 (a few hundred addends per feature, 128 x 64 products in the network) -- divided by the step, plus the truncation of
    the central difference: h0 is cubic along an axis through the product of three planes, relative (R step)^2 < 1e-9 at R = 64."""
    m, x = chain_case(256)
    u = ((x.double() + m.bound) / (2 * m.bound))
    step = 2.0 ** -24
    t = FRAME_TIMES["interior"]
    ref = DX.evaluate(m, u, t, True, rounded=False, pos_dtype=np.float64)
    assert np.abs(ref["a"]).max() > 0 and np.abs(ref["flow"]).max() > 1e-3  # the warp and its Jacobian term take part
    keep = ref["margin"] > step
    cds = []
    for d in range(3):
        e = torch.zeros(1, 3, dtype=torch.float64)
        e[0, d] = step
        hi = DX.evaluate(m, u + e, t, True, rounded=False, pos_dtype=np.float64, want_grad=False)
        lo = DX.evaluate(m, u - e, t, True, rounded=False, pos_dtype=np.float64, want_grad=False)
        keep &= (hi["gates"] == lo["gates"]).all(-1)  # pre-activations are linear along the axis inside a cell: equal at both ends, equal between
        cds.append(((hi["h0"] - lo["h0"]) / (2 * step), hi["habs"] + lo["habs"]))
    left_out = int((~keep).sum())
    print(f"chain oracle vs central differences: {left_out} of {keep.size} points left out")
    assert left_out <= 0.05 * keep.size
    for d, (cd, habs) in enumerate(cds):
        tol = 4096 * 2.0 ** -53 * habs / (2 * step) + 1e-9 * np.abs(cd)
        err = np.abs(ref["dh"][:, d] - cd)
        print(f"  axis {d}: largest error / tolerance = {float((err / tol)[keep].max()):.3f}, largest |cd| = {float(np.abs(cd[keep]).max()):.3g}")
        assert (err[keep] <= tol[keep]).all(), (d, float((err / tol)[keep].max()))
        assert np.abs(cd[keep]).max() > 1e-2  # the compared gradients are not zeros


def test_restated_gradient_keeps_the_small_gradient_cap():
    """The GPU test may leave out samples whose |grad sigma| is below 1e-6 of the batch maximum, at most 1 % of them: the restatement
    alone stays inside that cap for the chosen seed, at the three frame times the GPU test uses."""
    m, x = chain_case()
    for name, t in FRAME_TIMES.items():
        _, grad = DX.field_gradient_f64(m, x, t, lidar=True, rounded=True, fp16=True)
        norm = np.linalg.norm(grad, axis=-1)
        assert np.isfinite(norm).all() and norm.max() > 0
        small = norm < 1e-6 * norm.max()
        assert small.sum() <= 0.01 * norm.size, (name, int(small.sum()))
