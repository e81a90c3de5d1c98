"""CPU tests of the mesh export (nvsf/nerf/mesh.py): the case tables over all 256 cases, the binary PLY writer against an independent
reader, and the argument checks of export_mesh_density (all raised before anything reaches a device)."""
import numpy as np
import pytest

from nvsf.nerf import mesh


def read_ply(path):
    """Independent reader of binary little-endian PLY files with double x y z vertices and `list uchar int` faces."""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    counts, props = {}, {}
    elem = None
    for line in lines[2:]:
        w = line.split()
        if w[0] == "element":
            elem = w[1]
            counts[elem] = int(w[2])
            props[elem] = []
        elif w[0] == "property":
            props[elem].append(tuple(w[1:]))
    assert props["vertex"] == [("double", "x"), ("double", "y"), ("double", "z")]
    assert props["face"] == [("list", "uchar", "int", "vertex_indices")]
    nv, nf = counts["vertex"], counts["face"]
    v = np.frombuffer(data, "<f8", 3 * nv, end).reshape(nv, 3)
    off = end + 24 * nv
    tris = np.empty((nf, 3), np.int32)
    for i in range(nf):
        assert data[off] == 3
        tris[i] = np.frombuffer(data, "<i4", 3, off + 1)
        off += 13
    assert off == len(data)
    return v, tris


def _case_corners(case):
    return np.array([(case >> k) & 1 for k in range(8)], bool)


def test_edge_table_is_the_crossing_edges():
    for case in range(256):
        ins = _case_corners(case)
        want = sum(1 << e for e, (a, b) in enumerate(mesh.EDGES) if ins[a] != ins[b])
        assert int(mesh.EDGE_TABLE[case]) == want, case


def test_every_triangle_edge_crosses_and_every_crossing_edge_is_used():
    counts = []
    for case in range(256):
        row = mesh.TRI_TABLE[case]
        n = int(mesh.TRI_COUNT[case])
        counts.append(n)
        assert (row[:3 * n] >= 0).all() and (row[3 * n:] == -1).all(), case
        used = set(int(e) for e in row[:3 * n])
        crossing = {e for e in range(12) if (int(mesh.EDGE_TABLE[case]) >> e) & 1}
        assert used <= crossing, (case, used - crossing)
        assert used == crossing, (case, crossing - used)
        tris = row[:3 * n].reshape(-1, 3)
        assert all(len(set(t)) == 3 for t in tris.tolist()), case
    assert counts[0] == counts[255] == 0 and max(counts) <= 5


def test_triangle_normals_point_from_inside_to_outside():
    """Corner values +1 (inside) / -1 (outside): every vertex sits at its edge's midpoint; each triangle's normal has a positive
    component along (outside end - inside end) of its edges."""
    corners = mesh.CORNERS.astype(np.float64)
    for case in range(256):
        ins = _case_corners(case)
        n = int(mesh.TRI_COUNT[case])
        for t in mesh.TRI_TABLE[case][:3 * n].reshape(-1, 3):
            p = [(corners[mesh.EDGES[e][0]] + corners[mesh.EDGES[e][1]]) / 2 for e in t]
            normal = np.cross(p[1] - p[0], p[2] - p[0])
            assert np.linalg.norm(normal) > 1e-9, (case, t)
            out_dir = np.zeros(3)
            for e in t:
                a, b = mesh.EDGES[e]
                out_dir += corners[b] - corners[a] if ins[a] else corners[a] - corners[b]
            assert np.dot(normal, out_dir) > 0, (case, t)


def test_closed_surface_of_each_case_within_the_cube():
    """Each case's triangles form a surface whose only boundary lies on the cube's faces: every triangle side is used once or twice,
    and a side used once joins two vertices on a common face (the contour the neighbouring cube continues)."""
    corners = mesh.CORNERS
    faces_of_edge = []
    for a, b in mesh.EDGES:
        faces_of_edge.append({(ax, int(corners[a][ax])) for ax in range(3) if corners[a][ax] == corners[b][ax]})
    for case in range(256):
        n = int(mesh.TRI_COUNT[case])
        sides = {}
        for t in mesh.TRI_TABLE[case][:3 * n].reshape(-1, 3).tolist():
            for i in range(3):
                key = tuple(sorted((t[i], t[(i + 1) % 3])))
                sides[key] = sides.get(key, 0) + 1
        for (e1, e2), c in sides.items():
            assert c in (1, 2), (case, e1, e2)
            if c == 1:
                assert faces_of_edge[e1] & faces_of_edge[e2], (case, e1, e2)
        boundary = sum(1 for c in sides.values() if c == 1)
        assert boundary == bin(int(mesh.EDGE_TABLE[case])).count("1"), case  # each crossing edge ends two contour segments, each segment has two ends


def test_tables_image_layout():
    blob = mesh.tables_bytes()
    assert len(blob) == 4432
    tri = np.frombuffer(blob, np.int8, 4096).reshape(256, 16)
    assert (tri == mesh.TRI_TABLE).all()
    assert (np.frombuffer(blob, np.uint8, 256, 4096) == mesh.TRI_COUNT).all()
    edges = np.frombuffer(blob, np.int8, 48, 4352).reshape(12, 4)
    for e, (a, b) in enumerate(mesh.EDGES):
        lo = np.minimum(mesh.CORNERS[a], mesh.CORNERS[b])
        assert tuple(edges[e, :3]) == tuple(lo) and mesh.CORNERS[b][edges[e, 3]] != mesh.CORNERS[a][edges[e, 3]]
    corners = np.frombuffer(blob, np.int8, 32, 4400).reshape(8, 4)
    assert (corners[:, :3] == mesh.CORNERS).all() and (corners[:, 3] == 0).all()
    assert mesh.workspace_bytes((17, 33, 5)) == 8 * 1 + 4 * 17 * 33 * 5
    assert mesh.workspace_bytes((512, 512, 512)) == 8 * 32768 + 4 * 512 ** 3


def test_ply_round_trip_bit_for_bit(tmp_path):
    rng = np.random.default_rng(3)
    v = rng.standard_normal((37, 3)) * np.array([1e-300, 1.0, 1e300])
    v[0] = (np.nan, np.inf, -0.0)
    t = rng.integers(0, 37, (55, 3)).astype(np.int32)
    t[0] = (np.iinfo(np.int32).max, 0, -1)
    path = tmp_path / "m.ply"
    mesh.write_ply(str(path), v, t)
    v2, t2 = read_ply(str(path))
    assert v2.dtype == np.float64 and t2.dtype == np.int32
    assert v2.tobytes() == v.astype("<f8").tobytes() and t2.tobytes() == t.astype("<i4").tobytes()
    mesh.write_ply(str(path), np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    v3, t3 = read_ply(str(path))
    assert v3.shape == (0, 3) and t3.shape == (0, 3)


@pytest.fixture(scope="module")
def static_model():
    from nvsf.nerf.models.network_static import NeRFNetworkStatic
    return NeRFNetworkStatic(bound=2, n_levels_hash=2, log2_hashmap_size=8)


def test_export_rejects_bounds_outside_the_aabb(static_model, tmp_path):
    for lo, hi in (([-2.5, -1, -1], [1, 1, 1]), ([-1, -1, -1], [1, 2.01, 1]), ([0, 0, 0], [-1, 1, 1])):
        with pytest.raises(ValueError):
            mesh.export_mesh_density(static_model, str(tmp_path / "m.ply"), bound_min=lo, bound_max=hi, xyz_res=(4, 4, 4))
    assert not (tmp_path / "m.ply").exists()


def test_export_rejects_small_resolutions(static_model, tmp_path):
    for res in ((1, 4, 4), (4, 4, 1), (4, 0, 4), (4, 4)):
        with pytest.raises(ValueError):
            mesh.export_mesh_density(static_model, str(tmp_path / "m.ply"), xyz_res=res)
        with pytest.raises(ValueError):
            mesh.extract_fields([0, 0, 0], [1, 1, 1], res, lambda p: p[:, 0])


def test_export_rejects_smoothing(static_model, tmp_path):
    with pytest.raises(NotImplementedError, match="mcubes.smooth"):
        mesh.export_mesh_density(static_model, str(tmp_path / "m.ply"), xyz_res=(4, 4, 4), smoothing=True)
    with pytest.raises(NotImplementedError, match="mcubes.smooth"):
        mesh.extract_geometry([0, 0, 0], [1, 1, 1], [4, 4, 4], 0.0, lambda p: p[:, 0], smoothing=True)


def test_export_of_the_space_time_model_needs_a_time(tmp_path):
    from nvsf.nerf.models.network_dynamic import NeRFNetwork
    m = NeRFNetwork(time_resolution=2, num_frames=4, bound=1, log2_hashmap_size=8)
    with pytest.raises(ValueError, match="time"):
        mesh.export_mesh_density(m, str(tmp_path / "m.ply"), xyz_res=(4, 4, 4))
    assert not (tmp_path / "m.ply").exists()
