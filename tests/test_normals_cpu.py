"""CPU tests of the coordinate gradient's oracle and of the host side of the normals feature: the float64 oracle
against central differences of the float64 feature function, the PLY writer with vertex normals, the argument checks raised before
anything reaches a device, and the seed check of the GPU test that compares density_gradient with the float64 restatement."""
import numpy as np
import pytest
import torch

import hashgrid_gradx_oracle as GX
from test_mesh_cpu import read_ply


def _spec(D, L, F, log2_T, base, top):
    from nvsf.field_ops import GridSpec
    pls = float(np.exp2(np.log2(top / base) / (L - 1))) if L > 1 else 1.0
    return GridSpec(D, L, F, log2_T, base, pls)


@pytest.mark.parametrize("D,F", [(2, 2), (3, 2), (3, 4)])
def test_oracle_equals_central_differences_of_the_float64_features(D, F):
    """L(x) = sum g . features(x) is linear along an axis inside a cell, so its central difference with a step that stays inside the
    cell on every level IS the derivative, up to the float64 rounding of the two evaluations divided by the step.  Points j / 1024
    with integer scales (4 2^l - 1) make pos = scale x + 0.5 exact in fp32, so the oracle's fp32 cells and fracs are the float64
    function's; pos sits on a cell face only for j = 512, which is not drawn.  Dense and hashed levels both occur (log2_T = 10)."""
    spec = _spec(D, 5, F, 10, 4, 64)
    assert [float(s) for s in spec.scales] == [3.0, 7.0, 15.0, 31.0, 63.0]
    n_rows = np.diff(spec.offsets)
    kinds = [int(r) ** D <= int(n) for r, n in zip(spec.res, n_rows)]
    assert any(kinds) and not all(kinds)
    rng = np.random.default_rng(11 + D + F)
    M, step = 300, 2.0 ** -18
    j = rng.integers(1, 512, (M, D)) + 512 * rng.integers(0, 2, (M, D))
    x = (j / 1024.0).astype(np.float32)
    margin = GX.face_margin(x, spec)
    assert int((margin > step).sum()) == M  # no point dropped: every one is at least the step away from every cell face on every level
    table = (rng.standard_normal(spec.n_params) * 0.5).astype(np.float16)
    g = rng.standard_normal((M, spec.L, spec.F))
    got, A = GX.grad_x(x, table, spec, g)
    n_add = spec.L * spec.F * (1 << D)
    for d in range(D):
        e = np.zeros(D)
        e[d] = step
        hi = (g * GX.features(x.astype(np.float64) + e, table, spec)).sum((1, 2))
        lo = (g * GX.features(x.astype(np.float64) - e, table, spec)).sum((1, 2))
        cd = (hi - lo) / (2 * step)
        # each evaluation: n_add addends of a few float64 roundings each, |addend| <= A's addend / scale_0; divided by the step
        tol = (n_add + 8) * 2.0 ** -53 * A[:, d] / (float(spec.scales[0]) * step)
        err = np.abs(got[:, d] - cd)
        assert (err <= tol).all(), (d, float((err / tol).max()))
        assert np.abs(cd).max() > 1.0  # the comparison is not of zeros


def test_oracle_rows_follow_the_kernel_index_arithmetic():
    """Inside the unit cube the oracle's rows are those of tests/torch_f64_static.py::_corners (the restatement the static field's
    training gradients are pinned with), level by level and corner by corner, and so are its weights."""
    import torch_f64_static as S
    spec = _spec(3, 5, 2, 10, 4, 64)
    rng = np.random.default_rng(5)
    x = rng.random((200, 3)).astype(np.float32)
    seen = 0
    for k, (l, off, idx, w) in enumerate(S._corners(torch.from_numpy(x), spec)):
        c = k % 8
        scale, res, off2, n_rows = GX._level(spec, l)
        cell, frac = GX.cells(x, scale)
        bits = np.array([(c >> d) & 1 for d in range(3)], np.int64)
        assert off == off2 and np.array_equal(idx.numpy(), GX.rows(cell + bits[None, :], res, n_rows))
        w64 = np.prod(np.where(bits[None, :] == 1, frac, 1.0 - frac), -1)
        np.testing.assert_allclose(w.numpy(), w64, rtol=3e-7, atol=1e-12)
        seen += 1
    assert seen == spec.L * 8


def test_ply_with_normals_round_trips(tmp_path):
    from nvsf.nerf import mesh
    rng = np.random.default_rng(4)
    v = rng.standard_normal((29, 3))
    t = rng.integers(0, 29, (41, 3)).astype(np.int32)
    n = rng.standard_normal((29, 3)).astype(np.float32)
    n[0] = (np.nan, -0.0, np.inf)
    path = tmp_path / "n.ply"
    mesh.write_ply(str(path), v, t, normals=n)
    data = open(path, "rb").read()
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex 29\nproperty double x\nproperty double y\nproperty double z\n"
              "property float nx\nproperty float ny\nproperty float nz\nelement face 41\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii")
    assert data.startswith(header) and len(data) == len(header) + 29 * 36 + 41 * 13
    rec = np.frombuffer(data, np.dtype([("p", "<f8", (3,)), ("n", "<f4", (3,))]), 29, len(header))
    assert rec["p"].tobytes() == v.astype("<f8").tobytes() and rec["n"].tobytes() == n.astype("<f4").tobytes()
    off = len(header) + 29 * 36
    for i in range(41):
        assert data[off] == 3 and np.array_equal(np.frombuffer(data, "<i4", 3, off + 1), t[i])
        off += 13
    with pytest.raises(ValueError):
        mesh.write_ply(str(path), v, t, normals=n[:5])


def test_ply_without_normals_is_unchanged(tmp_path):
    """normals=None: byte for byte the file the writer produced before the argument existed (the layout tests/test_mesh_cpu.py reads)."""
    from nvsf.nerf import mesh
    rng = np.random.default_rng(6)
    v = rng.standard_normal((13, 3))
    t = rng.integers(0, 13, (7, 3)).astype(np.int32)
    a, b = tmp_path / "a.ply", tmp_path / "b.ply"
    mesh.write_ply(str(a), v, t)
    mesh.write_ply(str(b), v, t, normals=None)
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex 13\nproperty double x\nproperty double y\nproperty double z\n"
              "element face 7\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii")
    faces = b"".join(b"\x03" + t[i].astype("<i4").tobytes() for i in range(7))
    assert open(a, "rb").read() == open(b, "rb").read() == header + v.astype("<f8").tobytes() + faces
    v2, t2 = read_ply(str(a))
    assert v2.tobytes() == v.tobytes() and np.array_equal(t2, t)


@pytest.fixture(scope="module")
def static_model():
    from nvsf.nerf.models.network_static import NeRFNetworkStatic
    return NeRFNetworkStatic(bound=2, n_levels_hash=2, log2_hashmap_size=8)


def test_cpu_tensors_are_refused(static_model, tmp_path):
    from nvsf import _hip, field_ops as ops
    from nvsf.nerf import normals
    with pytest.raises(_hip.NvsfHipError):
        normals.density_gradient(static_model, torch.zeros(4, 3))
    with pytest.raises(_hip.NvsfHipError):
        normals.render_normals(static_model, torch.zeros(4, 3), torch.ones(4, 3), num_steps=8)
    enc = static_model.hash_encoder_camera
    with pytest.raises(_hip.NvsfHipError):
        ops.hashgrid_grad_x(torch.zeros(4, 3), (0, 1, 2), enc.params.detach().half(), enc.spec, torch.zeros(4, enc.n_output_dims))


def test_space_time_model_is_refused(tmp_path):
    from nvsf.nerf import mesh, normals
    from nvsf.nerf.models.network_dynamic import NeRFNetwork
    m = NeRFNetwork(time_resolution=2, num_frames=4, bound=1, log2_hashmap_size=8)
    with pytest.raises(NotImplementedError):
        normals.density_gradient(m, torch.zeros(4, 3))
    with pytest.raises(NotImplementedError):
        normals.render_normals(m, torch.zeros(4, 3), torch.ones(4, 3), num_steps=8)
    with pytest.raises(NotImplementedError):
        mesh.export_mesh_density(m, str(tmp_path / "m.ply"), xyz_res=(4, 4, 4), time=0.5, normals=True)
    assert not (tmp_path / "m.ply").exists()


def f64_case():
    """The model and points of the comparison of density_gradient with the float64 restatement (tests/test_normals_gpu.py), built on
    the CPU: a NeRFNetworkStatic with a random table (a freshly constructed one gives sigma == 1 everywhere) and 2048 points."""
    from nvsf.nerf.models.network_static import NeRFNetworkStatic
    torch.manual_seed(0)
    m = NeRFNetworkStatic(bound=1, n_levels_hash=16, log2_hashmap_size=14, max_resolution=512)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for enc in (m.hash_encoder_lidar, m.hash_encoder_camera):
            enc.params.copy_(torch.randn(enc.params.shape, generator=g) * 0.1)
        m.sigma_net.params.mul_(2.0)
    x = (torch.rand(2048, 3, generator=g) * 1.9 - 0.95).float()
    return m.eval(), x


def test_restated_gradient_keeps_the_small_gradient_cap():
    """The GPU test may leave out samples whose |grad sigma| is below 1e-6 of the batch maximum, at most 1 % of them: the restatement
    alone stays inside that cap for the chosen seed."""
    m, x = f64_case()
    _, grad = GX.field_gradient_f64(m, x, lidar=True, rounded=True)
    norm = np.linalg.norm(grad, axis=-1)
    assert np.isfinite(norm).all() and norm.max() > 0
    small = norm < 1e-6 * norm.max()
    assert small.sum() <= 0.01 * norm.size, int(small.sum())
