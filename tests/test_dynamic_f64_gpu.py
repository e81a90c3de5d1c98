"""The space-time encoders' HIP kernels against the float64 restatements of tests/torch_f64_dynamic.py, operator by operator: the
K-planes (PlanesFn, PlanesMultiFn and their scatter forms), the time-sliced 2-D hash grids (HashDynFn / HashDyn3Fn, regime 0 and
regime 1) and the flow field's grid with Lagrange reduction (FlowGridFn and the encoder chain).  No MLP, no render, no training step:
every operator is linear in its table, so nothing has to be left out of a comparison and nothing is.

Bars (none of them taken from the kernels' own error):
  * sparsity is exact: an entry no tap / corner of any row reads (touched_texels / touched_entries) has gradient exactly 0, and so has
    every entry whose addends are all zero;
  * per entry, errors are counted in units of 2^-24 A, A = the restatement evaluated on the absolute value of every addend.  The BASELINE is the same restatement evaluated in float32 on the device (torch's elementwise kernels,
    index_add_ scatters): its largest distance from float64, in the same units, is measured per case, and the kernel may be at most
    4 times as far (the margin test_composite_rays_train gives a kernel over a compiled fp32 reference: another association of the
    same sums, the arbitrary order of fp32 atomics), with a floor of 8 units for what the baseline happens to hit exactly;
  * regime-1 features (every product and sum rounded to fp16) are held to the FIXED floor of 8 units of 2^-11 A: behind the slice
    features the restatement is fp32 -> fp16 arithmetic whatever its dtype, so its float32 evaluation is the same computation (0 units)
    and measures nothing;
  * per tensor, every table / plane / coordinate / flow gradient lies within 2e-5 of the largest entry of its float64 gradient (the bar
    test_planes_multi_node_equals_one_node_per_evaluation uses between HIP forms);
  * a flow gradient is exactly 0 on every axis whose warped coordinate is clamped.
Each test prints the worst ratio of the kernel and of the baseline (`-s`); DESIGN.md section 4.5 carries the measured figures.

Inputs are shared: ray-ordered rows (long runs inside one cell), random rows, and an edge block in the first rows and again across a
64-row boundary -- coordinates exactly 0, 1, -0.0, the floats next to 0 and 1 on both sides, -0.25 and 1.25, texel centres
k / (R - 1) of every K-planes scale, grid nodes of a dense and of a hashed level, a denormal.  Incoming gradients have zero rows
(w[::6] = 0) and zero columns.  Row counts 1, 63, 64, 65, 211 * 29 and 2^16 + 77 (the last switches both LDS scatter forms on).
w[::6] = 0 leaves the single row of M = 1 without a gradient (its backward checks reduce to "exactly 0"), so every operator has a
second one-row case, LIVE1, whose zero rows start at row 3: one row with a gradient.
"""
import numpy as np
import pytest
import torch

import torch_f64_dynamic as T64

pytestmark = pytest.mark.gpu

M_RAYS, M_BIG = 211 * 29, (1 << 16) + 77
F32 = np.float32
_one, _zero = F32(1), F32(0)
EDGE = [0.0, 1.0, -0.0, float(np.nextafter(_zero, _one)), float(np.nextafter(_zero, -_one)), float(np.nextafter(_one, F32(2))),
        float(np.nextafter(_one, _zero)), -0.25, 1.25,
        float(F32(7) / F32(31)), float(F32(30) / F32(31)), float(F32(11) / F32(63)), float(F32(50) / F32(127)), float(F32(101) / F32(255)),
        float(F32(254) / F32(255)),                      # texel centres of the four K-planes scales
        float(F32(3.5) / F32(15)),                       # a node of the dense first level of the 2-D grids (pos = 15 x + 0.5 = 4)
        float(F32(199.5) / F32(510.99981689453125)),     # ... of their hashed last level
        float(F32(10.5) / F32(31)),                      # ... of the flow grid's first level
        1e-40, 0.5]
_below = float(np.nextafter(F32(3) / F32(7), _zero))
PLANE_TIMES = [0.0, 1.0] + [float(F32(k) / F32(7)) for k in range(1, 7)] + [0.37, _below]  # Planes4D's time resolution is 8: nodes k / 7


def _edge_block(rng):
    blk = rng.random((len(EDGE) + 4, 3)).astype(np.float32)
    for i, e in enumerate(EDGE):
        blk[i, i % 3] = e
    for i, e in enumerate((0.0, 1.0, -0.25, 1.25)):
        blk[len(EDGE) + i, :] = e
    return blk


_ROWS = {}


def rows(M, dev):
    """[M, 3] fp32 positions (see the module docstring), the same for every test."""
    if M not in _ROWS:
        rng = np.random.default_rng(100 + M)
        T = 211
        n_ray = (M * 3 // 5) // T * T
        parts = []
        if n_ray:
            o = rng.random((n_ray // T, 1, 3)) * 0.4 + 0.3
            d = rng.standard_normal((n_ray // T, 1, 3))
            d /= np.linalg.norm(d, axis=-1, keepdims=True)
            parts.append(np.clip(o + d * np.linspace(0, 0.35, T).reshape(1, T, 1), 0, 1).reshape(-1, 3))
        parts.append(rng.random((M - n_ray, 3)))
        x = np.concatenate(parts).astype(np.float32)
        blk = _edge_block(rng)
        E = len(blk)
        x[:E] = blk[:M]
        if M > 64 + E:
            x[64 - E // 2:64 - E // 2 + E] = blk
        elif M > E:
            x[M - E:] = blk  # M = 63, 64, 65: the block ends at the last row (M = 65: across the 64-row boundary)
        _ROWS[M] = torch.from_numpy(x)
    return _ROWS[M].to(dev)


LIVE1 = -1  # as a row count: ONE row whose incoming gradient is not zero


def row_count(M):
    """(rows, first zero row of the incoming gradients) of a row-count parameter."""
    return (1, 3) if M == LIVE1 else (M, 0)


def incoming(shape, seed, dev, zero_cols=(3, 17), z0=0):
    g = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    g[z0::6] = 0.0
    for c in zero_cols:
        if c < shape[1]:
            g[:, c] = 0.0
    return g.to(dev)


def units(got, ref, A, eps):
    """Largest |got - ref| in units of eps A; where A == 0 (no addend, or only zero addends) `got` must be exactly 0."""
    err = (got.double() - ref).abs()
    zero = A <= 0
    assert not bool(got[zero].any()), "an entry without a non-zero addend is not exactly 0"
    if bool(zero.all()):
        return 0.0
    return float((err[~zero] / (eps * A[~zero])).max())


def check(name, got, base, ref, A, eps=2.0 ** -24, tensor_bar=True, touched=None):
    """The bars of the module docstring for one tensor; prints (name, kernel units, baseline units)."""
    got, ref, A = got.reshape(-1), ref.reshape(-1), A.reshape(-1)
    if touched is not None:
        assert not bool(got[~touched.reshape(-1)].any()), f"{name}: a gradient outside the touched entries"
    rk, rb = units(got, ref, A, eps), units(base.reshape(-1), ref, A, eps)
    print(f"{name}: kernel {rk:.2f} units, float32 baseline {rb:.2f} units")
    assert rk <= max(4.0 * rb, 8.0), (name, rk, rb)
    if tensor_bar:
        scale = float(ref.abs().max())
        assert float((got.double() - ref).abs().max()) <= 2e-5 * scale, (name, float((got.double() - ref).abs().max()), scale)


# ------------------------------------------------------------------------------------------------------------------------------------
# K-planes
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planes_enc(dev):
    from nvsf.nerf.models.planes_field import Planes4D
    torch.manual_seed(11)
    enc = Planes4D(resolution=[32, 32, 32, 8], multiscale_res=[1, 2, 4, 8]).to(dev)
    with torch.no_grad():  # the time planes off their all-ones initialisation
        for si, pi, *_ in enc._layout:
            if pi in (2, 4, 5):
                v = enc.plane(si, pi)
                v.copy_(1.0 + 0.4 * (torch.rand(v.shape, generator=torch.Generator().manual_seed(20 + 6 * si + pi)) - 0.5).to(dev))
    return enc


def _planes_reference(fn, planes, g_list, leaf_shape):
    """fn(planes_leaf, coord_leaf, dtype, abs_sum) -> outputs (None for absent ones); -> per mode (float64, abs, float32 baseline):
    (outputs, plane gradient, coordinate-leaf gradient)."""
    res = {}
    for mode, dtype, ab in (("ref", torch.float64, False), ("abs", torch.float64, True), ("base", torch.float32, False)):
        p = planes.detach().to(dtype).requires_grad_()
        leaf = None if leaf_shape is None else torch.zeros(leaf_shape, dtype=dtype, device=planes.device).requires_grad_()
        outs = fn(p, leaf, dtype, ab)
        loss = None
        for o, g in zip(outs, g_list):
            if o is not None and g is not None:
                term = (o * (g.abs() if ab else g).to(dtype)).sum()
                loss = term if loss is None else loss + term
        loss.backward()
        res[mode] = ([None if o is None else o.detach() for o in outs], p.grad, None if leaf is None else leaf.grad)
    return res


@pytest.mark.parametrize("want", [1, 2, 3])
@pytest.mark.parametrize("M", [1, LIVE1, 63, 64, 65, M_RAYS, M_BIG])
def test_planes_fn(dev, planes_enc, variants, M, want):
    """PlanesFn, `want` = static / dynamic / both: features, the WHOLE planes_cl gradient (all 24 planes) and xt.grad; the texel scatter
    in its run-merging form (default) and as one atomic per (sample, texel, channel).  The time column runs through 0, 1, every slice
    node k / 7, a value between nodes and the float just below a node."""
    enc, res = planes_enc, planes_enc._res_host
    live1 = M == LIVE1
    M, z0 = row_count(M)
    x = rows(M, dev)
    i = torch.arange(M)
    t = torch.where((i < len(PLANE_TIMES)) | (i % 3 == 0), torch.tensor(PLANE_TIMES, dtype=torch.float32)[i % len(PLANE_TIMES)],
                    torch.rand(M, generator=torch.Generator().manual_seed(M))).to(dev)
    xt = torch.cat([x, t[:, None]], -1).contiguous()
    g_s = incoming((M, 32), 1, dev, z0=z0) if want & 1 else None
    g_d = incoming((M, 32), 2, dev, zero_cols=(5, 30), z0=z0) if want & 2 else None
    R = _planes_reference(lambda p, leaf, dt, ab: T64.planes_features(xt, p, res, want, dtype=dt, abs_sum=ab, xt_leaf=leaf), enc.planes_cl,
                          (g_s, g_d), (M, 4))
    touched = T64.touched_texels([(grp, xt) for grp in (0, 1) if want & (1 << grp)], res)
    for form in ("runs", "atomic"):
        if form == "atomic":
            variants.set(planes_bwd="atomic")
        enc.planes_cl.grad = None
        xin = xt.clone().requires_grad_()
        out = {1: lambda: (enc.forward_static(xin), None), 2: lambda: (None, enc.forward_dynamic(xin)), 3: lambda: tuple(enc(xin))}[want]()
        loss = sum((o * g).sum() for o, g in zip(out, (g_s, g_d)) if o is not None)
        loss.backward()
        tag = f"planes_fn M={M} want={want} {form}"
        for k, nm in ((0, "static"), (1, "dynamic")):
            if out[k] is not None and form == "runs":
                check(f"{tag} {nm}", out[k].detach(), R["base"][0][k], R["ref"][0][k], R["abs"][0][k], tensor_bar=False)
        check(f"{tag} grad planes_cl", enc.planes_cl.grad, R["base"][1], R["ref"][1], R["abs"][1], touched=touched)
        check(f"{tag} grad xt", xin.grad, R["base"][2], R["ref"][2], R["abs"][2])
        assert bool(enc.planes_cl.grad.any()) == (M > 1 or live1)
        if want != 3:  # the planes of the group that was not asked for receive exactly nothing
            for si, pi, off, Cc, H, W in enc._layout:
                if (pi in (2, 4, 5)) != (want == 2):
                    assert not bool(enc.planes_cl.grad[off:off + Cc * H * W].any())
    enc.planes_cl.grad = None


_MULTI_TIMES = [(0.37, 0.4, 0.34375), (0.0, float(F32(1) / F32(7)), 1.0), (1.0, _below, float(F32(2) / F32(7))), (float(F32(3) / F32(7)), 0.5, 0.0)]
_NB = [(True, True), (True, False), (False, True), (False, False)]
_MULTI_CASES = ([(M_RAYS, nb, blend, fs) for nb in _NB for blend in (False, True) for fs in (3e-3, 0.3)]
                + [(1, _NB[0], True, 0.3), (LIVE1, _NB[0], True, 0.3), (LIVE1, _NB[0], False, 3e-3), (63, _NB[0], False, 3e-3), (64, _NB[1], True, 3e-3), (65, _NB[0], True, 0.3)]
                + [(M_BIG, _NB[0], True, 3e-3), (M_BIG, _NB[1], False, 0.3), (M_BIG, _NB[2], True, 0.3), (M_BIG, _NB[0], False, 3e-3)])


@pytest.mark.parametrize("M,nb,blend,flow_scale", _MULTI_CASES)
def test_planes_multi_fn(dev, planes_enc, variants, M, nb, blend, flow_scale):
    """PlanesMultiFn: static at x, dynamic at (x, t0), (x + flow[:, :3], t1), (x + flow[:, 3:], t2) with either neighbour absent, blend off
    and on (the blend's gradient handed over as a column slice of a wider matrix), flows of 3e-3 and flows of 0.3 that push warped
    positions out of the box: features, the planes_cl gradient and the flow gradient.  Scatter forms: nvsf_planes_multi_bwd has TWO --
    the time planes through the LDS image (the default from 2^16 rows on) and every evaluation through the run-merging kernel (the
    default below 2^16 rows, and what ANY non-zero planes_bwd variant selects: "atomic" and "global" are one form in this entry point,
    the one-atomic-per-addend kernel belongs to nvsf_planes_bwd and is pinned in test_planes_fn).  So a case below 2^16 rows runs the
    one form there is, and a case at 2^16 + 77 rows runs both."""
    from nvsf import field_ops as ops
    enc, res = planes_enc, planes_enc._res_host
    case = _MULTI_CASES.index((M, nb, blend, flow_scale))
    t0, t1, t2 = _MULTI_TIMES[case % len(_MULTI_TIMES)]
    t1, t2 = (t1 if nb[0] else None), (t2 if nb[1] else None)
    M, z0 = row_count(M)
    x = rows(M, dev)
    has_flow = nb[0] or nb[1]
    wide_flow = ((torch.rand(M, 8, generator=torch.Generator().manual_seed(case)) - 0.5) * 2 * flow_scale).to(dev)  # rows wider than the six components
    flow = wide_flow[:, :6] if has_flow else None
    n_out = 2 if blend else 4
    wide = incoming((M, 48), 40 + case, dev, zero_cols=(9, 20), z0=z0)
    g_list = [incoming((M, 32), 3, dev, z0=z0), wide[:, 8:40] if blend else incoming((M, 32), 4, dev, zero_cols=(5, 30), z0=z0)]
    if not blend:
        g_list += [incoming((M, 32), 5, dev, z0=z0) if nb[0] else None, incoming((M, 32), 6, dev, zero_cols=(0,), z0=z0) if nb[1] else None]
    R = _planes_reference(lambda p, leaf, dt, ab: T64.planes_multi_features(x, flow, p, res, t0, t1, t2, blend=blend, dtype=dt, abs_sum=ab,
                                                                           flow_leaf=leaf), enc.planes_cl, g_list, (M, 6) if has_flow else None)
    evals = [(e[0], e[1]) for e in T64.multi_positions(x, flow, t0, t1, t2, blend) if e is not None]
    touched = T64.touched_texels(evals, res)
    forms = ["default"] + (["global"] if M >= (1 << 16) else [])
    for form in forms:
        if form != "default":
            variants.set(planes_bwd=form)
        enc.planes_cl.grad = None
        fl = wide_flow.clone().requires_grad_()
        outs = ops.PlanesMultiFn.apply(x, fl[:, :6] if has_flow else None, enc.planes_cl, res, float(F32(t0)), None if t1 is None else float(F32(t1)),
                                       None if t2 is None else float(F32(t2)), None, blend)
        live = [(o, g) for o, g in zip(outs[:n_out], g_list) if g is not None]
        torch.autograd.backward([o for o, _ in live], [g for _, g in live])
        tag = f"planes_multi M={M} nb={nb} blend={blend} flow={flow_scale} {form}"
        if form == "default":
            for k, nm in enumerate(("static", "blend" if blend else "d", "d1", "d2")[:n_out]):
                if R["ref"][0][k] is None:
                    assert outs[k].numel() == 0
                    continue
                check(f"{tag} {nm}", outs[k].detach(), R["base"][0][k], R["ref"][0][k], R["abs"][0][k], tensor_bar=False)
        check(f"{tag} grad planes_cl", enc.planes_cl.grad, R["base"][1], R["ref"][1], R["abs"][1], touched=touched)
        assert bool(enc.planes_cl.grad.any()) == (M > 1 or z0 > 0)
        if has_flow:
            gf = fl.grad[:, :6]
            assert not bool(fl.grad[:, 6:].any())
            check(f"{tag} grad flow", gf, R["base"][2], R["ref"][2], R["abs"][2])
            for col, tn in ((0, t1), (3, t2)):
                if tn is None:
                    assert not bool(gf[:, col:col + 3].any())  # an absent neighbour's columns stay zero
                    continue
                clamped = T64.clamped_axes(x + flow[:, col:col + 3], res)
                assert not bool(gf[:, col:col + 3][clamped].any())
                if flow_scale > 0.1 and M >= 63:
                    assert int(clamped.sum()) > M // 8  # the large flows do leave the box
    enc.planes_cl.grad = None


# ------------------------------------------------------------------------------------------------------------------------------------
# space-time hash grid
# ------------------------------------------------------------------------------------------------------------------------------------
_ENC = {}


def _hash_enc(dev, dyn):
    from nvsf.nerf.models.hash_field import HashGrid4D
    if dyn not in _ENC:
        torch.manual_seed(5)
        enc = HashGrid4D(base_resolution=16, max_resolution=512, time_resolution=4, n_levels=8, n_features_per_level=4, log2_hashmap_size=12,
                         hash_size_dynamic=list(dyn)).to(dev)
        with torch.no_grad():
            for p in enc.parameters():
                p.uniform_(-0.5, 0.5)
        _ENC[dyn] = enc
    return _ENC[dyn]


_just_below = float(np.nextafter(F32(2) / F32(3), _zero))
# (t, frame index of 16): both neighbours between nodes / first frame on node 0 / last frame on node 1 / node 1/3 / the float below node 2/3 /
# node 2/3 itself (F32(2) / F32(3) * 3 rounds to 2.0: floor == ceil == 2, slice 2 alone receives the gradient)
_HASH_TIMES = [(0.4, 6), (0.0, 0), (1.0, 15), (float(F32(1) / F32(3)), 5), (_just_below, 10), (float(F32(2) / F32(3)), 11)]
_NODES = (1, 2, 3, 5)
SMALL, SHIPPED = (11, 10, 10), (15, 13, 13)
_HASH_CASES = ([(SMALL, M, i) for i, M in enumerate((1, 63, 64, 65))] + [(SMALL, LIVE1, 0), (SMALL, LIVE1, 5)]
               + [(SMALL, M_RAYS, i) for i in range(6)] + [(SMALL, M_BIG, 0), (SMALL, M_BIG, 3)]
               + [(SHIPPED, M_RAYS, 0), (SHIPPED, M_RAYS, 5), (SHIPPED, M_BIG, 0), (SHIPPED, M_BIG, 1)])


def _hash_reference(x, enc, t_host, g, handover):
    specs = [pl.hash_t[0].spec for pl in enc.hash_dynamic]
    R_t = enc.hash_dynamic[0].time_resolution
    res = {}
    for mode, dtype, ab in (("ref", torch.float64, False), ("abs", torch.float64, True), ("base", torch.float32, False)):
        tables = [[s.params.detach().to(dtype).requires_grad_() for s in pl.hash_t] for pl in enc.hash_dynamic]
        out = T64.hash_time_features(x, tables, specs, R_t, t_host, reciprocal_division=True, dtype=dtype, abs_sum=ab, handover=handover)
        (out * (g.abs() if ab else g).to(dtype)).sum().backward()
        res[mode] = (out.detach(), [[s.grad for s in row] for row in tables])
    return res


def _check_hash_grads(tag, enc, R, x, k1, k2):
    """Exactly the slices floor and ceil received a gradient (one of them at a node), every entry inside both bars."""
    for pl, plane in enumerate(enc.hash_dynamic):
        touched = T64.touched_entries(x, plane.hash_t[0].spec, T64.HASH_PAIRS[pl])
        for k, sl in enumerate(plane.hash_t):
            got = sl.params.grad
            if k not in (k1, k2):
                assert got is None or not bool(got.any()), f"{tag}: slice {k} of pair {pl} received a gradient"
                assert R["ref"][1][pl][k] is None
                continue
            assert got is not None and bool(got.any()) == bool(R["ref"][1][pl][k].any())
            check(f"{tag} grad pair {pl} slice {k}", got, R["base"][1][pl][k], R["ref"][1][pl][k], R["abs"][1][pl][k], touched=touched)


def _clear(enc):
    for p in enc.parameters():
        p.grad = None


@pytest.mark.parametrize("dyn,M,ti", _HASH_CASES)
def test_hash_dynamic_training(dev, variants, monkeypatch, dyn, M, ti):
    """HashGrid4D's dynamic half under autograd: training_fused3 (HashDyn3Fn: regime-0 features at (x, t), regime-1 features of the flow-
    warped neighbours, for a frame with both neighbours, the first and the last frame) and forward_dynamic (HashDynFn), the gradient of
    EVERY slice parameter; forms hash4d_train fused / slices, hash4d_bwd default / run-merging, and at 2^16 + 77 rows the LDS kernel fed
    by rows and by the column-major [24][M] gradient (the test sees to it that nvsf_hashgrid4d_dynamic_bwd_scalar_t itself took it, not
    the row-major entry HashDynFn falls back to).  hash_size_dynamic [15, 13, 13] takes the two-row-range LDS launch.  The regime-1
    features are held to the fixed floor of 8 units of 2^-11 A (module docstring)."""
    from nvsf import _hip
    enc = _hash_enc(dev, dyn)
    specs = [pl.hash_t[0].spec for pl in enc.hash_dynamic]
    t_host, frame = _HASH_TIMES[ti]
    t_host = float(F32(t_host))
    t = torch.tensor([[t_host]], dtype=torch.float32, device=dev)
    M, z0 = row_count(M)
    x = rows(M, dev)
    g = incoming((M, 24), 7 + ti, dev, zero_cols=(3, 17), z0=z0)
    k1, k2 = T64.time_constants(t_host, 4, True)[:2]
    assert (k1 == k2) == (ti in _NODES) and (ti != 5 or k1 == 2) and (ti != 4 or (k1, k2) == (1, 2))
    R = _hash_reference(x, enc, t_host, g, handover=False)
    tag = f"hash4d {dyn} M={M} t={t_host:.7g}"
    # ---- HashDyn3Fn: the three evaluations of a density query
    flow = ((torch.rand(M, 8, generator=torch.Generator().manual_seed(M + ti)) - 0.5) * (0.6 if ti % 2 else 6e-3)).to(dev)
    _clear(enc)
    outs = enc.training_fused3(x, t, t_host, flow, frame, 16)
    assert outs is not None
    check(f"{tag} fused3 features", outs[0].detach(), R["base"][0], R["ref"][0], R["abs"][0], tensor_bar=False)
    (outs[0] * g).sum().backward()
    _check_hash_grads(f"{tag} fused3", enc, R, x, k1, k2)
    assert any(bool(p.grad.any()) for p in enc.hash_dynamic.parameters() if p.grad is not None) == (M > 1 or z0 > 0)
    for e, (col, nf) in enumerate(((0, frame + 1), (3, frame - 1)), start=1):
        if not 0 <= nf <= 15:
            assert outs[e].numel() == 0
            continue
        tn = float(F32(nf / 16))
        xn = x + flow[:, col:col + 3]
        tabs = [[s.params.detach().double() for s in pl.hash_t] for pl in enc.hash_dynamic]
        ref1 = T64.hash_time_features_f16(xn, tabs, specs, 4, tn, reciprocal_division=False)
        A1 = T64.hash_time_features_f16(xn, tabs, specs, 4, tn, reciprocal_division=False, abs_sum=True)
        base1 = T64.hash_time_features_f16(xn, [[s.float() for s in row] for row in tabs], specs, 4, tn, reciprocal_division=False, dtype=torch.float32)
        assert outs[e].dtype == torch.float16
        print(f"{tag} fused3 neighbour {e}: {int((outs[e] != ref1).sum())} of {ref1.numel()} fp16 values differ from the restatement's")
        check(f"{tag} fused3 neighbour {e} (regime 1)", outs[e].detach(), base1, ref1.double(), A1, eps=2.0 ** -11, tensor_bar=False)
    # ---- HashDynFn and its forms
    forms = [("fused", "default"), ("fused", "runs"), ("slices", "default")]
    if M >= (1 << 16):
        forms.append(("fused", "colmajor"))
    for train, bwd in forms:
        variants.set(hash4d_train=train)
        if bwd == "runs":
            variants.set(hash4d_bwd="runs")
        Rf = R if train == "fused" else _hash_reference(x, enc, t_host, g, handover=True)
        _clear(enc)
        out = enc.forward_dynamic(x, t, t_host)
        check(f"{tag} {train}/{bwd} features", out.detach().float(), Rf["base"][0], Rf["ref"][0], Rf["abs"][0], tensor_bar=False)
        if bwd == "colmajor":
            gcm = g.t().contiguous().t()  # [M, 24] with strides (1, M): what DensityTailFn.backward hands over
            assert gcm.stride() == (1, M)
            done, real_call = [], _hip.call

            def recording_call(name, *args):
                result = real_call(name, *args)  # raises where the entry point refuses: only calls that went through are recorded
                done.append(name)
                return result
            monkeypatch.setattr(_hip, "call", recording_call)
            out.backward(gcm)
            monkeypatch.setattr(_hip, "call", real_call)
            scatters = [n for n in done if n.startswith("nvsf_hashgrid4d_dynamic_bwd")]
            assert scatters == ["nvsf_hashgrid4d_dynamic_bwd_scalar_t"], scatters  # the column-major LDS kernel, and nothing in its place
        else:
            (out.float() * g).sum().backward()
        _check_hash_grads(f"{tag} {train}/{bwd}", enc, Rf, x, k1, k2)
        variants.clear("hash4d_bwd")
        variants.clear("hash4d_train")
    _clear(enc)


# ------------------------------------------------------------------------------------------------------------------------------------
# flow grid
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def flow_field(dev):
    from nvsf.nerf.models.flow_field import FlowField
    torch.manual_seed(6)
    flow = FlowField(n_levels=16, n_features_per_level=8, base_resolution=32, max_resolution=8192, log2_hashmap_size=14).to(dev)
    with torch.no_grad():
        flow.grid_enc.params.uniform_(-0.5, 0.5)
    flow.mlp = torch.nn.Identity()  # the operator under test is the grid with its Lagrange reduction: forward() returns the reduced features
    return flow


_FLOW_CASES = ([(M_RAYS, t, mode) for t in (0.0, 0.4, 1.0) for mode in ("fused", "chain")]
               + [(1, 0.4, "fused"), (LIVE1, 0.4, "fused"), (LIVE1, 1.0, "chain"), (63, 0.0, "chain"), (64, 1.0, "fused"), (65, 0.4, "chain"), (M_BIG, 0.4, "fused"), (M_BIG, 0.4, "chain")])


@pytest.mark.parametrize("M,t_val,mode", _FLOW_CASES)
def test_flow_grid(dev, flow_field, M, t_val, mode):
    """FlowField's grid (L = 16, F = 8, 2^14 rows per level) with the Lagrange reduction, grid_train_mode "fused" (FlowGridFn) and "chain"
    (encoder -> .float() -> lagrange_reduce under autograd): the reduced features and the table gradient at t in {0, 0.4, 1}."""
    flow = flow_field
    spec = flow.grid_enc.spec
    M, z0 = row_count(M)
    x = rows(M, dev)
    t_host = float(F32(t_val))
    xt = torch.cat([x, torch.full((M, 1), t_host, device=dev)], -1).contiguous()
    g = incoming((M, 32), 9, dev, zero_cols=(3, 17), z0=z0) * 64.0  # what a loss scaler would supply
    R = {}
    for m_, dtype, ab in (("ref", torch.float64, False), ("abs", torch.float64, True), ("base", torch.float32, False)):
        tab = flow.grid_enc.params.detach().to(dtype).requires_grad_()
        out = T64.flow_grid_features(x, tab, spec, t_host, reciprocal_division=True, dtype=dtype, abs_sum=ab, handover=mode == "chain")
        (out * (g.abs() if ab else g).to(dtype)).sum().backward()
        R[m_] = (out.detach(), tab.grad)
    flow.grid_train_mode = mode
    flow.grid_enc.params.grad = None
    try:
        out = flow(xt)
        (out * g).sum().backward()
    finally:
        flow.grid_train_mode = "fused"
    tag = f"flow_grid M={M} t={t_val} {mode}"
    check(f"{tag} reduced", out.detach(), R["base"][0], R["ref"][0], R["abs"][0], tensor_bar=False)
    check(f"{tag} grad table", flow.grid_enc.params.grad, R["base"][1], R["ref"][1], R["abs"][1], touched=T64.touched_entries(x, spec, (0, 1, 2)))
    assert bool(flow.grid_enc.params.grad.any()) == (M > 1 or z0 > 0)
    flow.grid_enc.params.grad = None
