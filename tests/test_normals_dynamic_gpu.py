"""GPU tests of the coordinate gradient of the time-sliced 2-D hash grids (nvsf_hashgrid4d_dynamic_grad_x, HashGrid4D.dynamic_grad_x) and
of what is built on it: density_gradient / render_normals for the space-time NeRFNetwork (nvsf/nerf/normals.py: the chain rule through
the K-planes, the hash grids and the flow warp) and the mesh export's vertex normals at a frame time.  DESIGN.md 9m.

The kernel is pinned to the numpy float64 oracle tests/hash4d_gradx_oracle.py with the bar (n + 8) 2^-24 A[m, d] per element, n = 512
addends per output (256 on a slice time), A = the sum of their absolute values; the chain to tests/dynamic_gradx_oracle.py with a bar
measured from that restatement alone.  Every figure that is asserted is printed first (run with -s to see them).
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

import dynamic_gradx_oracle as DX
import hash4d_gradx_oracle as H4
from test_normals_dynamic_cpu import FRAME_TIMES, chain_case

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# fp16-rounded intermediate gradients on the path of d h0 / d u (csrc/mlp_bwd.hip: gradients travel between the layers as fp16 MFMA
# operands): the density MLP's backward rounds the output gradient and the hidden layer's (2, as the static chain's); the flow MLP's
# backward in the fused regime rounds the output gradient and those of its two hidden layers (3); the fp32 Linear layers round none.
# Everything else on the path (the plane and grid kernels, the one-pass split, the sums) is fp32.
K_DENSITY, K_FLOW_FUSED = 2, 3


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _grid(dev, sizes, top=64, R=5, seed=7, **kw):
    """A HashGrid4D whose time-sliced grids run base 4 -> top with the three table sizes `sizes`, random fp16-exact tables."""
    from nvsf.nerf.models.hash_field import HashGrid4D
    enc = HashGrid4D(base_resolution=4, max_resolution=top, time_resolution=R, log2_hashmap_size=10, hash_size_dynamic=list(sizes), **kw)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in enc.parameters():
            p.copy_((torch.randn(p.shape, generator=g) * 0.5).half().float())
    return enc.to(dev).eval()


def _oracle_inputs(enc, t):
    from nvsf.nerf.models.hash_field import time_slot
    slot = time_slot(t, float(t), enc.hash_dynamic[0].time_resolution)  # t on the device: the division form of the device's weights
    tables = [tb.cpu().numpy() for tb in enc._slice_tables(slot)]
    return slot, tables, [pl.hash_t[0].spec for pl in enc.hash_dynamic]


def _positions(rng, M):
    """Random positions in the unit cube; from 63 rows on the first rows are 0, 1, 0.5 (a grid node of the coarsest level: scale 3),
    mixtures of them, and positions in [-0.4, 1.5]."""
    x = rng.random((M, 3)).astype(np.float32)
    if M >= 63:
        x[0], x[1], x[2] = 0.0, 1.0, 0.5
        x[3], x[4] = [0.0, 1.0, 0.5], [0.5, 0.0, 1.0]
        x[5:25] = (rng.random((20, 3)) * 1.9 - 0.4).astype(np.float32)
        assert (x < 0).any() and (x > 1).any()
    return x


def test_kernel_matches_the_float64_oracle(hip_lib, dev):
    """Tables of 2^10, 2^8 and 2^9 rows per level (base 4 -> top 64: dense and hashed levels in every pair), M in {1, 63, 64, 65, 1000},
    t at 0, on an interior slice, between slices and at 1, with and without an offset (columns 3..5 of a 7-column matrix), x as columns of
    a wider matrix, grad_out as columns 96..119 of a 128-column matrix, grad_scale 0.25, rows of 3 and of 5 floats; a second run and the
    accumulating form (one more fp32 add onto what the destination held) are bit-identical."""
    enc = _grid(dev, (10, 8, 9))
    for pl in enc.hash_dynamic:
        spec = pl.hash_t[0].spec
        dense = [int(r) ** 2 <= int(n) for r, n in zip(spec.res, np.diff(spec.offsets))]
        assert any(dense) and not all(dense)
    rng = np.random.default_rng(5)
    worst, seen = 0.0, set()
    for M in (1, 63, 64, 65, 1000):
        for t_host in (0.0, 0.5, 0.3, 1.0):
            t = torch.tensor([[t_host]], dtype=torch.float32, device=dev)
            slot, tables, specs = _oracle_inputs(enc, t)
            seen.add((slot.k1, slot.k2))
            n_add = 256 if slot.same else 512
            for with_offset in (False, True):
                xw = rng.standard_normal((M, 6)).astype(np.float32)
                xw[:, 2:5] = _positions(rng, M)
                ow = (rng.standard_normal((M, 7)) * 0.05).astype(np.float32)
                gw = rng.standard_normal((M, 128)).astype(np.float32)
                p = xw[:, 2:5] + ow[:, 3:6] if with_offset else xw[:, 2:5]  # fp32 sum, as the kernel's
                ref, A = H4.grad_x(p, tables, specs, slot, gw[:, 96:120], grad_scale=0.25)
                x_d, o_d, g_d = _t(xw, dev)[:, 2:5], _t(ow, dev), _t(gw, dev)[:, 96:120]
                kw = dict(grad_scale=0.25, offset=o_d if with_offset else None, offset_col=3)
                got = enc.dynamic_grad_x(x_d, t, t_host, g_d, **kw)
                assert got.shape == (M, 3) and got.dtype == torch.float32
                assert torch.equal(enc.dynamic_grad_x(x_d, t, t_host, g_d, **kw), got)
                wide = _t(rng.standard_normal((M, 5)).astype(np.float32), dev)
                before = wide.clone()
                assert enc.dynamic_grad_x(x_d, t, t_host, g_d, out=wide[:, 1:4], accumulate=True, **kw) is not None
                assert torch.equal(wide[:, 1:4], before[:, 1:4] + got) and torch.equal(wide[:, [0, 4]], before[:, [0, 4]])
                enc.dynamic_grad_x(x_d, t, t_host, g_d, out=wide[:, 1:4], **kw)
                assert torch.equal(wide[:, 1:4], got) and torch.equal(wide[:, [0, 4]], before[:, [0, 4]])
                err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
                bar = (n_add + 8) * U * A
                assert (bar > 0).all()
                worst = max(worst, float((err / bar).max()))
                assert (err <= bar).all(), (M, t_host, with_offset, float((err / bar).max()))
    assert seen == {(0, 0), (2, 2), (1, 2), (4, 4)}
    print(f"hashgrid4d_dynamic_grad_x: largest error / bar = {worst:.4f}")


def test_exact_case_on_tables_of_cell_indices(hip_lib, dev):
    """Dense levels whose four features are the vertex's first cell coordinate (small integers), the same in every slice: the feature of
    pair (a, b) is pos_a (sum_i w_i) (b_lo + b_hi), so the derivative along b is 0.0f EXACTLY (the kernel differences each corner pair
    before it blends) and along a it is sum_l scale_l G_l (sum_i w_i) (b_lo + b_hi), inside the bar of that sum."""
    enc = _grid(dev, (14, 14, 14))
    with torch.no_grad():
        for pl in enc.hash_dynamic:
            spec = pl.hash_t[0].spec
            table = torch.zeros(spec.n_rows, 4)
            for l in range(spec.L):
                res, off, n = int(spec.res[l]), int(spec.offsets[l]), int(spec.offsets[l + 1] - spec.offsets[l])
                assert res ** 2 <= n
                table[off:off + n] = (torch.arange(n) % res).float()[:, None]
            for sl in pl.hash_t:
                sl.params.copy_(table.reshape(-1).to(sl.params.device))
    rng = np.random.default_rng(3)
    M = 257
    x = (rng.random((M, 3)) * 0.75 + 0.05).astype(np.float32)  # cell + 1 stays below res on every level: no wrap into the next row
    scales = np.array([float(s) for s in enc.hash_dynamic[0].hash_t[0].spec.scales])
    for t_host in (0.5, 0.3):
        t = torch.tensor([[t_host]], dtype=torch.float32, device=dev)
        slot, tables, specs = _oracle_inputs(enc, t)
        c = sum(float(np.float32(v)) for v in slot.lag) * (1.0 if slot.same else float(np.float32(slot.b_lo)) + float(np.float32(slot.b_hi)))
        n_add = 256 if slot.same else 512
        for zero_pair_2 in (False, True):
            g = rng.standard_normal((M, 3, 8)).astype(np.float32)
            if zero_pair_2:
                g[:, 2] = 0.0
            S = (g.astype(np.float64) * scales[None, None, :]).sum(-1) * c  # per pair: sum_l scale_l g_l (sum_i w_i) (b_lo + b_hi)
            want = np.stack([S[:, 0] + S[:, 1], S[:, 2], np.zeros(M)], -1)  # x: axis a of pairs 0, 1; y: a of pair 2 (b of pair 0); z: b only
            ref, A = H4.grad_x(x, tables, specs, slot, g.reshape(M, 24))
            assert np.abs(ref - want).max() <= 1e-9 * np.abs(want).max()
            got = enc.dynamic_grad_x(_t(x, dev), t, t_host, _t(g.reshape(M, 24), dev)).cpu().numpy()
            assert (got[:, 2] == 0).all()
            if zero_pair_2:
                assert (got[:, 1] == 0).all()
            err, bar = np.abs(got.astype(np.float64) - want), (n_add + 8) * U * A
            print(f"exact case t = {t_host}: largest error / bar = {float((err[:, :2] / bar[:, :2]).max()):.4f}")
            assert (err[:, :2] <= bar[:, :2]).all()


def test_refusals_and_empty_batches(hip_lib, dev):
    from nvsf import _hip
    from nvsf.nerf.models.hash_field import HashGrid4D
    enc = _grid(dev, (10, 8, 9))
    t = torch.tensor([[0.3]], dtype=torch.float32, device=dev)
    z = lambda *s: torch.zeros(*s, device=dev)
    out = enc.dynamic_grad_x(z(0, 3), t, 0.3, z(0, 24))
    assert out.shape == (0, 3)
    with pytest.raises(_hip.NvsfHipError):
        enc.dynamic_grad_x(torch.zeros(4, 3), t, 0.3, z(4, 24))
    with pytest.raises(_hip.NvsfHipError):
        enc.dynamic_grad_x(z(4, 3), t, 0.3, torch.zeros(4, 24))
    with pytest.raises(NotImplementedError):
        _grid(dev, (10, 8, 9), n_levels=4).dynamic_grad_x(z(4, 3), t, 0.3, z(4, 24))
    # the entry point itself: a null pointer among its arguments is refused before any launch, M = 0 is accepted whatever the pointers
    slot, _, _ = _oracle_inputs(enc, t)
    _, h_scales, h_res, h_off = enc.pair_level_tables()
    tables = (ctypes.c_void_p * 6)(*[tb.data_ptr() for tb in enc._slice_tables(slot)])
    h_time = _hip.host_f32([slot.b_lo, slot.b_hi] + slot.lag)
    x, g, o = z(4, 3), z(4, 24), z(4, 3)

    def call(M=4, x=x.data_ptr(), tables=tables, h_time=h_time, g=g.data_ptr(), o=o.data_ptr(), same=0):
        _hip.call("nvsf_hashgrid4d_dynamic_grad_x", x, 3, None, 0, 0, M, tables, h_scales, h_res, h_off, h_time, same, g, 24, 1.0, o, 3, 0)
    call()
    call(M=0, x=None, g=None, o=None, tables=None, h_time=None)
    for bad in (dict(x=None), dict(g=None), dict(o=None), dict(tables=None), dict(h_time=None)):
        with pytest.raises(_hip.NvsfHipError):
            call(**bad)
    lo_only = (ctypes.c_void_p * 6)(*([tb.data_ptr() for tb in enc._slice_tables(slot)][:3] + [None] * 3))
    call(tables=lo_only, same=1)  # the hi slices may be null on a slice time ...
    with pytest.raises(_hip.NvsfHipError):
        call(tables=lo_only, same=0)  # ... and only then
    torch.cuda.synchronize()


# ---- the chain -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case(dev):
    m_cpu, x = chain_case()
    return m_cpu, copy.deepcopy(m_cpu).to(dev).eval(), x


def _t11(t, dev):
    return torch.tensor([[t]], dtype=torch.float32, device=dev)


@pytest.mark.parametrize("frame", list(FRAME_TIMES))
@pytest.mark.parametrize("lidar", [True, False])
def test_the_forward_is_the_models_own(dev, case, lidar, frame):
    from nvsf.nerf import normals
    _, m, x = case
    t = FRAME_TIMES[frame]
    out = normals.density_gradient(m, x.to(dev), cal_lidar_color=lidar, time=t)
    with torch.no_grad():
        sigma = m.density(x.to(dev), _t11(t, dev), lidar)["sigma"]
    assert torch.equal(out["sigma"], sigma) and bool((sigma > 0).all())
    assert set(out) == {"sigma", "grad", "normal"} and out["grad"].shape == (x.shape[0], 3) and not out["grad"].requires_grad
    norm = out["grad"].double().norm(dim=-1, keepdim=True)
    ok = norm[:, 0] > 0
    assert bool(ok.any())
    assert torch.allclose(out["normal"].double()[ok], (-out["grad"].double() / norm)[ok], rtol=0, atol=1e-6)


def _device_flow(m, x, t, fp16, dev):
    """The flow the model itself evaluates at these points in this regime: the warped positions decide cells."""
    with torch.no_grad():
        u = m._unit_cube(x.to(dev).float())
        xt = torch.cat([u, _t11(t, dev).expand(u.shape[0], 1)], dim=-1)
        return u.cpu(), m.flow_net(xt, float(np.float32(t)), fp16=fp16).float().cpu()


def _compare(m_cpu, m, x, t, fp16, flow_jacobian, k, dev, label):
    from nvsf.nerf import normals
    u, flow = _device_flow(m, x, t, fp16, dev)
    _, ref = DX.field_gradient_f64(m_cpu, x, t, True, rounded=True, fp16=fp16, flow_jacobian=flow_jacobian, flow32=flow)
    _, plain = DX.field_gradient_f64(m_cpu, x, t, True, rounded=False, fp16=fp16, flow_jacobian=flow_jacobian, flow32=flow)
    norm = np.linalg.norm(ref, axis=-1)
    keep = norm >= 1e-6 * norm.max()
    assert (~keep).sum() <= 0.01 * keep.size
    bar = k * np.linalg.norm(ref - plain, axis=-1)
    got = normals.density_gradient(m, x.to(dev), cal_lidar_color=True, time=t, fp16=fp16, flow_jacobian=flow_jacobian)["grad"].double().cpu().numpy()
    err = np.linalg.norm(got - ref, axis=-1)
    ratio = err[keep] / bar[keep]
    print(f"{label}: k = {k}; median |grad| {np.median(norm):.3e}; bar median {np.median(bar[keep]):.3e} min {bar[keep].min():.3e}; "
          f"error median {np.median(err[keep]):.3e} max {err[keep].max():.3e}; error / bar median {np.median(ratio):.4f} max {ratio.max():.4f}")
    assert (err[keep] <= bar[keep]).all(), float(ratio.max())
    return u, flow


@pytest.mark.parametrize("fp16", [True, False])
@pytest.mark.parametrize("frame", list(FRAME_TIMES))
def test_density_gradient_against_the_float64_chain(dev, case, frame, fp16):
    """2048 points of the small space-time model, first, interior and last frame, both regimes of the flow MLP.  The bar is measured
    from the restatement alone: per sample, k times the distance between the chain with the forward's fp16 rounding points and the chain
    without them, k = 2 + the number of fp16-rounded intermediate gradients on the path (K_DENSITY, K_FLOW_FUSED above): 7 with the
    fused flow MLP, 4 with the fp32 Linear layers.  Samples whose |grad| is below 1e-6 of the batch maximum are left out, at most 1 %
    (tests/test_normals_dynamic_cpu.py checks the cap on the restatement).  Some warped positions leave the base cell on the finest
    level of the time-sliced grids (asserted).
    Measured on one MI355X (error / bar, median and largest): see DESIGN.md 9m."""
    m_cpu, m, x = case
    k = 2 + K_DENSITY + (K_FLOW_FUSED if fp16 else 0)
    u, flow = _compare(m_cpu, m, x, FRAME_TIMES[frame], fp16, True, k, dev, f"density_gradient vs fp64 chain, {frame} frame, fp16={fp16}")
    scale = float(m.hash_encoder_lidar.hash_dynamic[0].hash_t[0].spec.scales[-1])
    cell = lambda p: np.floor(p.numpy().astype(np.float64) * scale + 0.5)
    moved = [(cell(u + flow[:, c:c + 3]) != cell(u)).any(-1) for c in (0, 3)]
    assert moved[0].any() and moved[1].any()


def test_flow_jacobian_switch(dev, case):
    """flow_jacobian=False is the chain without the J_f^T term (no flow-MLP backward on the path: k = 2 + K_DENSITY); with the flow
    net's last layer zeroed the flow and its Jacobian vanish and both settings return equal tensors."""
    from nvsf.nerf import normals
    m_cpu, m, x = case
    t = FRAME_TIMES["interior"]
    _compare(m_cpu, m, x, t, True, False, 2 + K_DENSITY, dev, "density_gradient(flow_jacobian=False) vs fp64 chain")
    xd = x.to(dev)
    with_j = normals.density_gradient(m, xd, cal_lidar_color=True, time=t, fp16=True)
    without = normals.density_gradient(m, xd, cal_lidar_color=True, time=t, fp16=True, flow_jacobian=False)
    assert not torch.equal(with_j["grad"], without["grad"]) and torch.equal(with_j["sigma"], without["sigma"])
    still = copy.deepcopy(m)
    with torch.no_grad():
        still.flow_net.mlp[-1].weight.zero_()
    for fp16 in (True, False):
        a = normals.density_gradient(still, xd, cal_lidar_color=True, time=t, fp16=fp16)
        b = normals.density_gradient(still, xd, cal_lidar_color=True, time=t, fp16=fp16, flow_jacobian=False)
        assert torch.equal(a["grad"], b["grad"]) and bool((a["grad"] != 0).any())


@pytest.mark.parametrize("lidar", [True, False])
def test_render_normals_at_a_frame_time(dev, case, lidar):
    """64 rays x 96 samples: normal = sum_i w_i n_i of the function's own per-sample weights and normals (float64 sum; one fp32
    rounding per addend), cos_incidence = -normal . d / |d|, a chunked run equals the unchunked one bit for bit, and a missing `time`
    is a ValueError.  The flow MLP runs in the fused regime (fp16=True, the shipped configuration's): its kernels compute a sample from
    that sample alone, whereas the fp32 Linear layers of the other regime are library GEMMs whose summation order may follow the batch
    size -- there the chunked run is compared to 1e-6 (outputs of magnitude <= 1)."""
    from nvsf.nerf import normals
    _, m, _ = case
    N, T = 64, 96
    g = torch.Generator().manual_seed(17)
    o = ((torch.rand(N, 3, generator=g) - 0.5) * 0.5).to(dev)
    d = torch.randn(N, 3, generator=g)
    d = (d / d.norm(dim=-1, keepdim=True)).to(dev)
    t = FRAME_TIMES["interior"]
    out = normals.render_normals(m, o, d, cal_lidar_color=lidar, num_steps=T, return_samples=True, time=t, fp16=True)
    assert out["normal"].shape == (N, 3) and out["weights_sum"].shape == (N,) and out["cos_incidence"].shape == (N,)
    w, n = out["weights"].double(), out["sample_normals"].double()
    assert bool((out["weights_sum"] > 1e-3).any()) and bool(((n.norm(dim=-1) - 1).abs() < 1e-6).any())
    want = (w[:, :, None] * n).sum(1)
    tol = (T + 2) * U * (w[:, :, None] * n).abs().sum(1)
    assert bool(((out["normal"].double() - want).abs() <= tol).all())
    assert torch.allclose(out["cos_incidence"], -(out["normal"] * d).sum(-1), rtol=0, atol=1e-6)
    chunked = normals.render_normals(m, o, d, cal_lidar_color=lidar, num_steps=T, max_ray_batch=24, time=t, fp16=True)
    assert set(chunked) == {"normal", "weights_sum", "cos_incidence"}
    for key in chunked:
        assert torch.equal(chunked[key], out[key]), key
    whole32 = normals.render_normals(m, o, d, cal_lidar_color=lidar, num_steps=T, time=t, fp16=False)
    chunked32 = normals.render_normals(m, o, d, cal_lidar_color=lidar, num_steps=T, max_ray_batch=24, time=t, fp16=False)
    for key in chunked32:
        diff = float((chunked32[key] - whole32[key]).abs().max())
        print(f"render_normals, fp32 flow MLP, chunked against whole: {key} max |diff| = {diff:.3e}")
        assert diff <= 1e-6, key  # |normal|, weights_sum <= 1; a GEMM's summation order moves a flow by a few fp32 ulps: observed 1.9e-8
    with pytest.raises(ValueError):
        normals.render_normals(m, o, d, cal_lidar_color=lidar, num_steps=T)
    with pytest.raises(ValueError):
        normals.density_gradient(m, o, cal_lidar_color=lidar)


def test_mesh_export_of_the_space_time_model_with_vertex_normals(dev, case, tmp_path):
    from nvsf.nerf import mesh, normals
    _, m, _ = case
    t = FRAME_TIMES["interior"]
    b_min, b_max, res = [-0.5, -0.5, 0.06], [0.5, 0.5, 0.09], (17, 33, 5)
    with torch.no_grad():
        u, _ = mesh.extract_fields(b_min, b_max, res, lambda p: m.density(p, _t11(t, dev), False)["sigma"].float(), device=dev)
    thr = float(u.median())
    kw = dict(bound_min=b_min, bound_max=b_max, xyz_res=res, threshold=thr, time=t)
    plain = mesh.export_mesh_density(m, str(tmp_path / "plain.ply"), **kw)
    assert len(plain) == 2
    v, tri, n = mesh.export_mesh_density(m, str(tmp_path / "normals.ply"), normals=True, **kw)
    assert v.shape[0] > 0 and tri.shape[0] > 0 and v.tobytes() == plain[0].tobytes() and tri.tobytes() == plain[1].tobytes()
    assert n.dtype == np.float32 and n.shape == v.shape
    want = normals.density_gradient(m, torch.from_numpy(v.astype(np.float32)).to(dev), time=t)["normal"].cpu().numpy()
    assert n.tobytes() == want.tobytes() and np.abs(np.linalg.norm(n, axis=-1) - 1).max() < 1e-6
    data = open(tmp_path / "normals.ply", "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    rec = np.frombuffer(data, np.dtype([("p", "<f8", (3,)), ("n", "<f4", (3,))]), v.shape[0], end)
    assert rec["p"].tobytes() == v.tobytes() and rec["n"].tobytes() == n.tobytes()
