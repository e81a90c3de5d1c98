"""Mesh export of the learned density field: the last step of the reference's test pipeline (scripts/main_nvsf.py:297-300 ->
Trainer.export_mesh_density, nvsf/nerf/utils.py:559-608, over extract_fields / extract_geometry, :296-384).

The reference samples the field chunk by chunk into host numpy and runs PyMCubes on the CPU, then writes the mesh through trimesh.
Here the grid stays on the device, marching cubes runs on csrc/marching_cubes.hip, and a small binary PLY writer replaces trimesh.
Deviations from the reference: `time` is an argument (the space-time model needs it), the bounds are checked
against `model.aabb_infer` instead of asserted inside [-1, 1], `mcubes.smooth` is not provided, and the optional point array is filled
at the right rows.

The case tables live here, once: `TRI_TABLE` [256, 16] (edge ids of the case's triangles, -1 padded) and `EDGE_TABLE` [256] (bit e:
edge e crosses) over the classic corner / edge numbering (`CORNERS`, `EDGES`).  The triangles are derived from the cube by one fixed rule
rather than copied from a listing: on every face the contour separates the face's inside corners from each other where they are
diagonal (the face-ambiguous case), the contour segments are chained into loops around the cube, and each loop is triangulated (the
fan from its lowest edge unless that puts a triangle flat into a cube face; see _triangulate).  The face rule depends on the face's corners only, so neighbouring cubes agree and the surface is closed wherever it does
not leave the grid.  Loops are oriented so that (v1 - v0) x (v2 - v0) points from inside (u >= iso) to outside.
"""
import os

import numpy as np
import torch

# corner k = (dx, dy, dz); edge e joins corners EDGES[e] (Bourke's numbering)
CORNERS = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)], np.int64)
EDGES = ((0, 1), (1, 2), (3, 2), (0, 3), (4, 5), (5, 6), (7, 6), (4, 7), (0, 4), (1, 5), (2, 6), (3, 7))
_FACES = ((0, 3, 7, 4), (1, 2, 6, 5), (0, 1, 5, 4), (3, 2, 6, 7), (0, 1, 2, 3), (4, 5, 6, 7))  # corner cycles of the -x +x -y +y -z +z faces
_FACE_NORMALS = np.array([(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)], np.float64)


def _edge_between(a, b):
    return next(e for e, ab in enumerate(EDGES) if set(ab) == {a, b})


def edge_owner(e):
    """(dx, dy, dz, axis): the corner that owns cube edge e (its lower end) and the edge's axis (0 x, 1 y, 2 z)."""
    a, b = EDGES[e]
    lo = np.minimum(CORNERS[a], CORNERS[b])
    return (*(int(v) for v in lo), int(np.argmax(np.abs(CORNERS[b] - CORNERS[a]))))


def _polygon_triangulations(idx):
    """Every triangulation of the convex-ordered polygon idx (a list of loop positions), the fan from idx[0] first."""
    if len(idx) < 3:
        yield []
        return
    a, b = idx[0], idx[-1]
    for k in range(len(idx) - 2, 0, -1):  # apex of the triangle on side (a, b); k = len - 2 first gives the fan from a
        for left in _polygon_triangulations(idx[:k + 1]):
            for right in _polygon_triangulations(idx[k:]):
                yield left + right + [(a, idx[k], b)]


def _triangulate(loop, ins, mid):
    """Triangles of one contour loop (edge ids in boundary order): the first triangulation, over the loop's rotations starting at its
    lowest edge, in which every triangle has a positive normal component along the inside -> outside directions of its three edges
    (with the vertices at the edge midpoints).  This excludes triangles flat in a cube face."""
    n = len(loop)
    for r in range(n):
        rot = loop[r:] + loop[:r]
        for tri in _polygon_triangulations(list(range(n))):
            out = []
            for i, j, k in tri:
                t = (rot[i], rot[j], rot[k])
                normal = np.cross(mid[t[1]] - mid[t[0]], mid[t[2]] - mid[t[0]])
                out_dir = sum((CORNERS[b] - CORNERS[a]) if ins[a] else (CORNERS[a] - CORNERS[b]) for a, b in (EDGES[e] for e in t))
                if np.dot(normal, out_dir) <= 0:
                    break
                out.append(t)
            else:
                return sorted(out, key=lambda t: [rot.index(e) for e in t])
    raise AssertionError(f"no oriented triangulation of loop {loop}")


def _build_tables():
    mid = [(CORNERS[a] + CORNERS[b]) / 2.0 for a, b in EDGES]
    tri = np.full((256, 16), -1, np.int8)
    edge_mask = np.zeros(256, np.uint16)
    for case in range(256):
        ins = [(case >> k) & 1 for k in range(8)]
        for e, (a, b) in enumerate(EDGES):
            if ins[a] != ins[b]:
                edge_mask[case] |= 1 << e
        nxt = {}
        for f, cyc in enumerate(_FACES):
            fin = [ins[k] for k in cyc]
            if sum(fin) in (0, 4):
                continue
            segs = []  # (edge, edge, direction from inside to outside in the face)
            if fin in ([1, 0, 1, 0], [0, 1, 0, 1]):  # ambiguous face: cut off each inside corner on its own
                for i in range(4):
                    if fin[i]:
                        c = cyc[i]
                        segs.append((_edge_between(cyc[i - 1], c), _edge_between(c, cyc[(i + 1) % 4]),
                                     CORNERS[list(cyc)].mean(0) - CORNERS[c]))
            else:
                es = [_edge_between(cyc[i], cyc[(i + 1) % 4]) for i in range(4) if fin[i] != fin[(i + 1) % 4]]
                out_c = CORNERS[[cyc[i] for i in range(4) if not fin[i]]].mean(0)
                in_c = CORNERS[[cyc[i] for i in range(4) if fin[i]]].mean(0)
                segs.append((es[0], es[1], out_c - in_c))
            for ea, eb, n in segs:
                # boundary of a polygon whose normal n points outward runs along n x (face normal) on that face
                if np.dot(mid[eb] - mid[ea], np.cross(n, _FACE_NORMALS[f])) < 0:
                    ea, eb = eb, ea
                nxt[ea] = eb
        seen, tris = set(), []
        for e0 in sorted(nxt):
            if e0 in seen:
                continue
            loop, e = [e0], nxt[e0]
            seen.add(e0)
            while e != e0:
                loop.append(e)
                seen.add(e)
                e = nxt[e]
            tris += _triangulate(loop, ins, mid)
        for i, t in enumerate(tris):
            tri[case, 3 * i:3 * i + 3] = t
    return tri, edge_mask


TRI_TABLE, EDGE_TABLE = _build_tables()
TRI_COUNT = ((TRI_TABLE >= 0).sum(1) // 3).astype(np.uint8)


def tables_bytes():
    """The device image of the tables (csrc/marching_cubes.hip: tri [256][16] int8 | ntri [256] uint8 | edge [12][4] int8 | corner [8][4] int8)."""
    edges = np.array([edge_owner(e) for e in range(12)], np.int8)
    corners = np.concatenate([CORNERS, np.zeros((8, 1), np.int64)], 1).astype(np.int8)
    blob = TRI_TABLE.tobytes() + TRI_COUNT.tobytes() + edges.tobytes() + corners.tobytes()
    assert len(blob) == 4432
    return blob


_device_tables = {}


def _tables_on(device):
    key = (device.type, device.index)
    if key not in _device_tables:
        host = torch.frombuffer(bytearray(tables_bytes()), dtype=torch.uint8)
        _device_tables[key] = host.to(device)
    return _device_tables[key]


def workspace_bytes(shape):
    """Scratch bytes nvsf_marching_cubes_count / _emit need for a grid of this shape: two uint32 per tile of 4096 points + one per point."""
    n = int(np.prod([int(s) for s in shape]))
    return 8 * ((n + 4095) // 4096) + 4 * n


def marching_cubes(u, threshold):
    """Marching cubes of a device fp32 grid u [nx, ny, nz] (u[x, y, z], z fastest) at `threshold`: (vertices [V, 3] fp32 in index space,
    triangles [T, 3] int32), both on u's device.  Inside iff u >= threshold; the contract is the one of include/nvsf_hip.h section 8."""
    from nvsf import _hip
    if u.dim() != 3:
        raise ValueError("marching_cubes: u must be [nx, ny, nz]")
    if not u.is_cuda:
        raise _hip.NvsfHipError("marching_cubes runs on the HIP device; there is no CPU fallback")
    if u.dtype != torch.float32:
        raise ValueError("marching_cubes: u must be fp32")
    u = u.contiguous()
    dev = u.device
    nx, ny, nz = (int(s) for s in u.shape)
    if min(nx, ny, nz) < 1 or nx * ny * nz >= 2 ** 31:
        raise ValueError(f"marching_cubes: grid shape {tuple(u.shape)} is empty or has 2^31 points or more")
    tables = _tables_on(dev)
    ws_bytes = workspace_bytes(u.shape)
    ws = torch.empty(max(ws_bytes, 8) // 8 + 1, dtype=torch.int64, device=dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    iso = float(np.float32(threshold))
    args = [_hip.ptr(u), nx, ny, nz, iso, _hip.ptr(tables), _hip.ptr(ws)]
    _hip.call("nvsf_marching_cubes_count", *args, ws_bytes, _hip.ptr(totals))
    n_v, n_t = (int(v) for v in totals.cpu())  # the one device -> host read: sizes of the outputs
    if n_v >= 2 ** 31 or n_t >= 2 ** 31:
        raise ValueError(f"marching_cubes: {n_v} vertices / {n_t} triangles exceed int32 indices")
    vertices = torch.empty(n_v, 3, dtype=torch.float32, device=dev)
    triangles = torch.empty(n_t, 3, dtype=torch.int32, device=dev)
    _hip.call("nvsf_marching_cubes_emit", *args, ws_bytes, n_v, n_t, _hip.ptr(vertices) if n_v else None, n_v,
              _hip.ptr(triangles) if n_t else None, n_t)
    return vertices, triangles


def _check_res(xyz_res):
    res = [int(r) for r in xyz_res]
    if len(res) != 3 or min(res) < 2:
        raise ValueError(f"xyz_res must be three sizes of at least 2 (got {list(xyz_res)})")
    return res


def extract_fields(bound_min, bound_max, xyz_res, query_func, S=128, return_points=False, device=None):
    """Samples `query_func` on the grid torch.linspace(bound_min[i], bound_max[i], xyz_res[i]) per axis (ij order): u[x, y, z], fp32,
    on `device` (default: the current HIP device).  The reference's signature and grid (utils.py:296-347): the axes are the reference's
    CPU linspace values, the points are assembled from them on the device, and the grid is filled in place slab by slab along z (as many
    z-planes per query as fit in S^3 points, at least one), with no host copy.

    Returns (u, pnts_w_sigma): pnts_w_sigma [N, 4] = (x, y, z, sigma) in u's linear order when `return_points`, else None.  The
    reference fills this array wrongly: it offsets its rows by xi * S only (utils.py:344), so the chunks of every (y, z) block overwrite
    each other.  It is not reproduced."""
    nx, ny, nz = _check_res(xyz_res)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    axes = [torch.linspace(float(bound_min[i]), float(bound_max[i]), r).to(dev) for i, r in enumerate((nx, ny, nz))]
    dz = max(1, min(nz, int(S) ** 3 // (nx * ny)))
    u = pts_all = None
    with torch.no_grad():
        for z0 in range(0, nz, dz):
            z1 = min(nz, z0 + dz)
            xx, yy, zz = torch.meshgrid(axes[0], axes[1], axes[2][z0:z1], indexing="ij")
            pts = torch.stack([xx, yy, zz], dim=-1).reshape(-1, 3)
            val = query_func(pts).reshape(nx, ny, z1 - z0)
            if u is None:
                u = torch.empty(nx, ny, nz, dtype=torch.float32, device=dev)
                if return_points:
                    pts_all = torch.empty(nx, ny, nz, 4, dtype=torch.float32, device=dev)
            u[:, :, z0:z1] = val
            if return_points:
                pts_all[:, :, z0:z1, :3] = pts.reshape(nx, ny, z1 - z0, 3)
                pts_all[:, :, z0:z1, 3] = val
    return u, (pts_all.reshape(-1, 4) if return_points else None)


def extract_geometry(bound_min, bound_max, xyz_res, threshold, query_func, smoothing=False, return_points=False, device=None):
    """Marching cubes of the sampled field (utils.py:350-384): (vertices [V, 3] float64 in world coordinates, triangles [T, 3] int32,
    pnts_w_sigma or None), numpy.  Vertices are mapped as the reference maps mcubes' output: v / (xyz_res - 1) (b_max - b_min) + b_min
    with the bounds in fp32."""
    if smoothing:
        raise NotImplementedError("smoothing: mcubes.smooth (the reference's optional Laplacian-like smoothing of the field) is out of scope")
    res = _check_res(xyz_res)
    u, pnts = extract_fields(bound_min, bound_max, res, query_func, return_points=return_points, device=device)
    v, t = marching_cubes(u, threshold)
    b_min = np.asarray(torch.as_tensor(bound_min, dtype=torch.float32).cpu())
    b_max = np.asarray(torch.as_tensor(bound_max, dtype=torch.float32).cpu())
    vertices = v.cpu().numpy().astype(np.float64) / (np.array(res) - 1.0) * (b_max - b_min)[None, :] + b_min[None, :]
    return vertices, t.cpu().numpy(), (pnts.cpu().numpy() if pnts is not None else None)


def write_ply(path, vertices, triangles, normals=None):
    """Binary little-endian PLY: `double x y z` per vertex, `list uchar int vertex_indices` per face.  `normals` [V, 3]: every vertex
    record gains `float nx ny nz` (36 bytes per vertex instead of 24); None: the file is byte for byte what it was without the argument."""
    v = np.ascontiguousarray(vertices, dtype="<f8").reshape(-1, 3)
    t = np.ascontiguousarray(triangles, dtype="<i4").reshape(-1, 3)
    normal_props = ""
    if normals is not None:
        n = np.ascontiguousarray(normals, dtype="<f4").reshape(-1, 3)
        if n.shape[0] != v.shape[0]:
            raise ValueError(f"write_ply: {n.shape[0]} normals for {v.shape[0]} vertices")
        normal_props = "property float nx\nproperty float ny\nproperty float nz\n"
        records = np.empty(v.shape[0], dtype=[("p", "<f8", (3,)), ("n", "<f4", (3,))])
        records["p"] = v
        records["n"] = n
        v = records
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {v.shape[0]}\nproperty double x\nproperty double y\nproperty double z\n{normal_props}"
              f"element face {t.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n")
    faces = np.empty(t.shape[0], dtype=[("n", "u1"), ("i", "<i4", (3,))])
    faces["n"] = 3
    faces["i"] = t
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(v.tobytes())
        f.write(faces.tobytes())


_NORMAL_CHUNK = 1 << 18  # vertices per density_gradient call of export_mesh_density(normals=True)


def _is_space_time(model):
    from nvsf.nerf.models.network_static import NeRFNetworkStatic
    return not isinstance(model, NeRFNetworkStatic)


def export_mesh_density(model, save_path, bound_min=None, bound_max=None, xyz_res=(256, 256, 256), threshold=10, smoothing=False,
                        time=None, cal_lidar_color=False, normals=False):
    """Trainer.export_mesh_density (utils.py:559-608) as a function of the model: samples the raw density
    `model.density(pts, t, cal_lidar_color)["sigma"]` (no density_scale) under no_grad in evaluation mode -- the regime of eval_step --
    on the grid of extract_fields, runs marching cubes at `threshold` on the device and writes a binary PLY to `save_path`.
    Bounds default to model.aabb_infer and must lie inside it (the reference asserts [-1, 1] instead, which its own defaults fail at
    bound = 2).  `time` (float or tensor) is required for the space-time NeRFNetwork -- the reference calls density without one, which
    that model cannot evaluate -- and ignored by the static network.  Returns (vertices, triangles) as written.
    `normals`: the unit normals -grad sigma / |grad sigma| of the field at the vertices (nvsf.nerf.normals.density_gradient, evaluated in
    chunks; for the space-time model at `time`, on a HIP device only) are written with them and returned: (vertices, triangles,
    normals [V, 3] fp32)."""
    if normals and _is_space_time(model) and not model.aabb_infer.is_cuda:
        raise NotImplementedError("export_mesh_density(normals=True): the space-time model's coordinate gradient has no CPU form")
    if smoothing:
        raise NotImplementedError("smoothing: mcubes.smooth (the reference's optional Laplacian-like smoothing of the field) is out of scope")
    res = _check_res(xyz_res)
    aabb = [float(v) for v in model.aabb_infer.detach().cpu().tolist()]
    b_min = aabb[:3] if bound_min is None else [float(v) for v in bound_min]
    b_max = aabb[3:] if bound_max is None else [float(v) for v in bound_max]
    if len(b_min) != 3 or len(b_max) != 3:
        raise ValueError("bound_min / bound_max: three values each")
    b32 = lambda v: [float(np.float32(x)) for x in v]
    if any(lo < a for lo, a in zip(b32(b_min), aabb[:3])) or any(hi > a for hi, a in zip(b32(b_max), aabb[3:])):
        raise ValueError(f"mesh bounds {b_min} .. {b_max} must lie inside the model's aabb_infer {aabb[:3]} .. {aabb[3:]}")
    if any(lo > hi for lo, hi in zip(b_min, b_max)):
        raise ValueError(f"bound_min {b_min} exceeds bound_max {b_max}")
    dev = model.aabb_infer.device
    t = None
    if _is_space_time(model):
        if time is None:
            raise ValueError("export_mesh_density: the space-time model needs `time` (the frame time in [0, 1]) to evaluate its density")
        t = torch.as_tensor(time, dtype=torch.float32).reshape(1, 1).to(dev)

    def query_func(pts):
        return model.density(pts, t, cal_lidar_color)["sigma"].float()

    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            vertices, triangles, _ = extract_geometry(torch.tensor(b_min, dtype=torch.float32), torch.tensor(b_max, dtype=torch.float32),
                                                      res, threshold, query_func, device=dev)
    finally:
        model.train(was_training)
    d = os.path.dirname(os.path.abspath(save_path))
    os.makedirs(d, exist_ok=True)
    if not normals:
        write_ply(save_path, vertices, triangles)
        return vertices, triangles
    from nvsf.nerf.normals import density_gradient
    vertex_normals = np.empty((vertices.shape[0], 3), np.float32)
    for i in range(0, vertices.shape[0], _NORMAL_CHUNK):
        pts = torch.from_numpy(vertices[i:i + _NORMAL_CHUNK].astype(np.float32)).to(dev)
        vertex_normals[i:i + _NORMAL_CHUNK] = density_gradient(model, pts, cal_lidar_color, time=t)["normal"].cpu().numpy()
    write_ply(save_path, vertices, triangles, vertex_normals)
    return vertices, triangles, vertex_normals

