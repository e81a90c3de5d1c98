"""Marching cubes on the device (csrc/marching_cubes.hip via nvsf/nerf/mesh.py) against a vectorised numpy restatement of the contract
 -- bit for bit -- plus table-independent geometry of a sphere mesh and the export path on both field networks."""
import os
import sys

import numpy as np
import pytest
import torch

from nvsf.nerf import mesh

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_mesh_cpu import read_ply  # noqa: E402

pytestmark = pytest.mark.gpu


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def mc_numpy(u, iso):
    """(vertices fp32 [V, 3], triangles int32 [T, 3], cases int64 [C]) by the contract, with the package's table, in fp32."""
    u = np.ascontiguousarray(u, np.float32)
    iso = np.float32(iso)
    nx, ny, nz = u.shape
    if min(nx, ny, nz) < 2:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros(0, np.int64)
    ins = u >= iso
    idx = np.indices(u.shape).astype(np.float32)
    valid = np.zeros(u.shape + (3,), bool)
    pos = np.zeros(u.shape + (3, 3), np.float32)
    for ax in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        a, b = u[tuple(lo)], u[tuple(hi)]
        cross = ins[tuple(lo)] != ins[tuple(hi)]
        with np.errstate(all="ignore"):
            t = (iso - a) / (b - a)
            bad = ~(np.isfinite(a) & np.isfinite(b))
            t = np.where(bad, np.where(np.isnan(t), np.float32(0.5), np.clip(t, np.float32(0), np.float32(1))), t).astype(np.float32)
        valid[tuple(lo) + (ax,)] = cross
        for c in range(3):
            p = idx[c][tuple(lo)]
            pos[tuple(lo) + (ax, c)] = (p + t).astype(np.float32) if c == ax else p
    flat_valid = valid.reshape(-1)
    vid = np.cumsum(flat_valid) - 1
    vertices = pos.reshape(-1, 3)[flat_valid]
    # cubes: case from the 8 corners, in cube linear order
    cs = (nx - 1, ny - 1, nz - 1)
    case = np.zeros(cs, np.int64)
    for k, (dx, dy, dz) in enumerate(mesh.CORNERS):
        case |= ins[dx:dx + cs[0], dy:dy + cs[1], dz:dz + cs[2]].astype(np.int64) << k
    case = case.reshape(-1)
    cx, cy, cz = [a.reshape(-1) for a in np.indices(cs)]
    rows = mesh.TRI_TABLE[case].astype(np.int64)  # [C, 16]
    tri = np.full((case.size, 5, 3), -1, np.int64)
    for s in range(15):
        e = rows[:, s]
        ok = e >= 0
        own = np.array([mesh.edge_owner(k) for k in range(12)], np.int64)[np.where(ok, e, 0)]
        p = ((cx + own[:, 0]) * ny + (cy + own[:, 1])) * nz + (cz + own[:, 2])
        tri[:, s // 3, s % 3] = np.where(ok, vid[p * 3 + own[:, 3]], -1)
    keep = tri[:, :, 0] >= 0
    return vertices, tri[keep].astype(np.int32), case


def run_gpu(u, iso, dev):
    v, t = mesh.marching_cubes(torch.from_numpy(np.ascontiguousarray(u, np.float32)).to(dev), iso)
    torch.cuda.synchronize()
    return v.cpu().numpy(), t.cpu().numpy()


def assert_same(u, iso, dev):
    v_ref, t_ref, case = mc_numpy(u, iso)
    v, t = run_gpu(u, iso, dev)
    assert v.shape == v_ref.shape and t.shape == t_ref.shape, (v.shape, v_ref.shape, t.shape, t_ref.shape)
    assert t.dtype == np.int32 and v.dtype == np.float32
    assert np.array_equal(t, t_ref)
    assert v.tobytes() == v_ref.tobytes()
    return v, t, case


# ---- fields ---------------------------------------------------------------------------------------------------------------------
def _coords(shape):
    return [a.astype(np.float32) for a in np.indices(shape)]


def sphere(shape, centre, r):
    x, y, z = _coords(shape)
    c = np.float32(centre)
    return (np.float32(r) - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)).astype(np.float32)


def torus(shape):
    x, y, z = _coords(shape)
    c = (np.array(shape, np.float32) - 1) / 2 + np.float32(0.37)
    big, small = 0.3 * min(shape[0], shape[1]), max(1.2, 0.35 * shape[2])
    q = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2) - big
    return (np.float32(small) - np.sqrt(q ** 2 + (z - c[2]) ** 2)).astype(np.float32)


def smooth_random(shape, seed, modes=24, wavelength=2.5):
    rng = np.random.default_rng(seed)
    x, y, z = _coords(shape)
    u = np.zeros(shape, np.float64)
    for _ in range(modes):
        k = rng.standard_normal(3)
        k *= 2 * np.pi / wavelength / np.linalg.norm(k)
        u += np.cos(k[0] * x + k[1] * y + k[2] * z + rng.uniform(0, 2 * np.pi))
    return u.astype(np.float32)


SHAPES = [(17, 33, 5), (128, 128, 128), (500, 500, 50)]


@pytest.mark.parametrize("shape", SHAPES)
def test_sphere_and_torus_match_the_restatement(dev, shape):
    c = (np.array(shape) - 1) / 2 + np.array([0.31, -0.27, 0.13])
    assert_same(sphere(shape, c, 0.4 * min(shape)), 0.0, dev)
    assert_same(torus(shape), 0.0, dev)


@pytest.mark.parametrize("shape", SHAPES)
def test_smooth_random_field_reaches_every_case(dev, shape):
    u = smooth_random(shape, 7)
    _, t, case = assert_same(u, 0.25, dev)
    if shape == (128, 128, 128):
        assert np.unique(case).size == 256  # all 256 cases, the ambiguous ones included
    assert t.shape[0] > 0


@pytest.mark.parametrize("shape", SHAPES)
def test_corners_exactly_at_the_threshold(dev, shape):
    u = np.round(smooth_random(shape, 11) * 2) / 2  # values in steps of 0.5: many corners equal the threshold
    assert (u == 0.5).mean() > 0.05
    assert_same(u.astype(np.float32), 0.5, dev)


@pytest.mark.parametrize("shape", SHAPES)
def test_non_finite_values(dev, shape):
    rng = np.random.default_rng(5)
    u = smooth_random(shape, 13)
    flat = u.reshape(-1)
    for val in (np.nan, np.inf, -np.inf):
        flat[rng.choice(flat.size, max(3, flat.size // 50), replace=False)] = val
    v, t, _ = assert_same(u, 0.0, dev)
    assert np.isfinite(v).all()


@pytest.mark.parametrize("shape", SHAPES)
def test_constant_field_is_empty(dev, shape):
    for val in (0.0, 1.0):
        v, t = run_gpu(np.full(shape, val, np.float32), 0.5, dev)
        assert v.shape == (0, 3) and t.shape == (0, 3)


def test_thin_and_flat_grids(dev):
    u2 = smooth_random((40, 37, 2), 3)
    _, t, _ = assert_same(u2, 0.0, dev)
    assert t.shape[0] > 0
    for shape in ((40, 37, 1), (1, 9, 9), (5, 1, 7), (1, 1, 1)):
        v, t = run_gpu(smooth_random(shape, 3), 0.0, dev)
        assert v.shape == (0, 3) and t.shape == (0, 3)


def test_abi_rejects_short_buffers(dev, hip_lib):
    from nvsf import _hip
    u = torch.from_numpy(smooth_random((9, 10, 11), 1)).to(dev)
    tables = mesh._tables_on(u.device)
    ws_bytes = mesh.workspace_bytes(u.shape)
    ws = torch.empty(ws_bytes // 8 + 1, dtype=torch.int64, device=dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    args = [_hip.ptr(u), 9, 10, 11, 0.0, _hip.ptr(tables), _hip.ptr(ws)]
    stream = torch.cuda.current_stream().cuda_stream
    assert hip_lib.nvsf_marching_cubes_count(*args, ws_bytes - 4, _hip.ptr(totals), stream) == -1
    assert hip_lib.nvsf_marching_cubes_count(_hip.ptr(u), 9, 0, 11, 0.0, _hip.ptr(tables), _hip.ptr(ws), ws_bytes, _hip.ptr(totals), stream) == -1
    assert hip_lib.nvsf_marching_cubes_count(_hip.ptr(u), 2 ** 11, 2 ** 10, 2 ** 10, 0.0, _hip.ptr(tables), _hip.ptr(ws), ws_bytes,
                                             _hip.ptr(totals), stream) == -1
    assert hip_lib.nvsf_marching_cubes_count(*args, ws_bytes, _hip.ptr(totals), stream) == 0
    n_v, n_t = (int(x) for x in totals.cpu())
    assert n_v > 0 and n_t > 0
    v = torch.empty(n_v, 3, device=dev)
    t = torch.empty(n_t, 3, dtype=torch.int32, device=dev)
    assert hip_lib.nvsf_marching_cubes_emit(*args, ws_bytes, n_v, n_t, _hip.ptr(v), n_v - 1, _hip.ptr(t), n_t, stream) == -1
    assert hip_lib.nvsf_marching_cubes_emit(*args, ws_bytes, n_v, n_t, _hip.ptr(v), n_v, _hip.ptr(t), n_t - 1, stream) == -1
    assert hip_lib.nvsf_marching_cubes_emit(*args, ws_bytes - 4, n_v, n_t, _hip.ptr(v), n_v, _hip.ptr(t), n_t, stream) == -1
    assert hip_lib.nvsf_marching_cubes_emit(*args, ws_bytes, n_v, n_t, _hip.ptr(v), n_v, _hip.ptr(t), n_t, stream) == 0
    torch.cuda.synchronize()


# ---- geometry of the sphere, without the table ----------------------------------------------------------------------------------
def test_sphere_mesh_is_a_closed_outward_sphere(dev):
    shape, r = (128, 128, 128), 40.3
    c = np.array([63.37, 64.71, 62.19])
    u = sphere(shape, c, r)
    v, t = run_gpu(u, 0.0, dev)
    V, F = v.shape[0], t.shape[0]
    sides = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
    uniq, counts = np.unique(sides, axis=0, return_counts=True)
    assert (counts == 2).all()
    E = uniq.shape[0]
    assert V - E + F == 2
    assert len(np.unique(t)) == V
    p = v.astype(np.float64) - c
    vol = np.einsum("ij,ij->i", p[t[:, 0]], np.cross(p[t[:, 1]], p[t[:, 2]])).sum() / 6
    assert abs(vol / (4 / 3 * np.pi * r ** 3) - 1) < 0.01, vol
    # the field, interpolated (trilinearly == linearly along the vertex's edge) at each vertex, is the threshold
    i0 = np.clip(np.floor(v).astype(np.int64), 0, np.array(shape) - 2)
    f = v.astype(np.float64) - i0
    val = np.zeros(V)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                w = (f[:, 0] if dx else 1 - f[:, 0]) * (f[:, 1] if dy else 1 - f[:, 1]) * (f[:, 2] if dz else 1 - f[:, 2])
                val += w * u[i0[:, 0] + dx, i0[:, 1] + dy, i0[:, 2] + dz]
    assert np.abs(val).max() < 1e-5


# ---- the export path on the field networks --------------------------------------------------------------------------------------
def _linspace_points(b_min, b_max, res, dev):
    axes = [torch.linspace(float(b_min[i]), float(b_max[i]), res[i]) for i in range(3)]
    g = torch.meshgrid(*axes, indexing="ij")
    return torch.stack(g, -1).reshape(-1, 3).to(dev)


@pytest.fixture(scope="module")
def static_model(dev):
    from nvsf import synthetic as S
    from nvsf.nerf.models.network_static import NeRFNetworkStatic
    torch.manual_seed(0)
    m = NeRFNetworkStatic(bound=S.BOUND, min_near=S.MIN_NEAR, min_near_lidar=S.MIN_NEAR, lidar_max_depth=S.LIDAR_MAX_DEPTH)
    with torch.no_grad():
        for enc in (m.hash_encoder_lidar, m.hash_encoder_camera):
            enc.params.normal_(0.0, 0.5)
    return m.to(dev).eval()


def test_static_export_matches_the_direct_query(dev, static_model, tmp_path):
    m = static_model
    b_min, b_max, res = [-0.5, -0.5, 0.06], [0.5, 0.5, 0.09], [61, 47, 23]
    query = lambda p: m.density(p)["sigma"].float()
    with torch.no_grad():
        direct = query(_linspace_points(b_min, b_max, res, dev)).reshape(res)
        u, pts = mesh.extract_fields(b_min, b_max, res, query, device=dev, return_points=True)
        u_small, _ = mesh.extract_fields(b_min, b_max, res, query, S=12, device=dev)  # 1728 points: one z-plane per query
    assert torch.equal(u, direct) and torch.equal(u_small, direct)
    assert torch.equal(pts[:, 3], direct.reshape(-1)) and torch.equal(pts[:, :3], _linspace_points(b_min, b_max, res, dev))
    thr = float(direct.median())
    path = str(tmp_path / "static.ply")
    v_exp, t_exp = mesh.export_mesh_density(m, path, bound_min=b_min, bound_max=b_max, xyz_res=res, threshold=thr)
    with torch.no_grad():
        v_ref, t_ref, _ = mesh.extract_geometry(torch.tensor(b_min), torch.tensor(b_max), res, thr, query, device=dev)
    v_file, t_file = read_ply(path)
    assert t_ref.shape[0] > 0
    assert v_file.tobytes() == v_ref.tobytes() and np.array_equal(t_file, t_ref)
    # the mapping to world coordinates is the reference's (utils.py:380-383) applied to the index-space result
    vi, ti = mesh.marching_cubes(direct.contiguous(), thr)
    b0, b1 = np.float32(b_min), np.float32(b_max)
    want = vi.cpu().numpy().astype(np.float64) / (np.array(res) - 1.0) * (b1 - b0)[None, :] + b0[None, :]
    assert want.tobytes() == v_ref.tobytes() and np.array_equal(ti.cpu().numpy(), t_ref)


def test_space_time_export_uses_the_time(dev, tmp_path):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import golden_dynamic as GD
    from nvsf import synthetic as S
    from nvsf.nerf.models.network_dynamic import NeRFNetwork
    m = NeRFNetwork(min_near=S.MIN_NEAR, min_near_lidar=S.MIN_NEAR, lidar_max_depth=S.LIDAR_MAX_DEPTH, **GD.SMALL).eval()
    GD.init_by_name(m)
    m = m.to(dev)
    b_min, b_max, res = [-1.0, -1.2, -0.3], [1.1, 0.9, 0.4], [33, 29, 17]
    grids = []
    for time in (0.25, 0.75):
        t = torch.tensor([[time]], dtype=torch.float32, device=dev)
        query = lambda p: m.density(p, t)["sigma"].float()
        with torch.no_grad():
            direct = query(_linspace_points(b_min, b_max, res, dev)).reshape(res)
            u, _ = mesh.extract_fields(b_min, b_max, res, query, device=dev)
        assert torch.equal(u, direct)
        grids.append(u)
        thr = float(u.median())
        path = str(tmp_path / f"dyn_{time}.ply")
        mesh.export_mesh_density(m, path, bound_min=b_min, bound_max=b_max, xyz_res=res, threshold=thr, time=time)
        v_file, t_file = read_ply(path)
        with torch.no_grad():
            v_ref, t_ref, _ = mesh.extract_geometry(torch.tensor(b_min), torch.tensor(b_max), res, thr, query, device=dev)
        assert t_ref.shape[0] > 0 and v_file.tobytes() == v_ref.tobytes() and np.array_equal(t_file, t_ref)
    assert not torch.equal(grids[0], grids[1])
    with pytest.raises(ValueError, match="time"):
        mesh.export_mesh_density(m, str(tmp_path / "none.ply"), xyz_res=(8, 8, 8))
