"""CPU side of the object-mask tests: the fixture of tests/golden/golden_object_masks.py, the inputs it was made from (rebuilt from
tests/golden/depth_image.npz, so that they are stored once), and numpy restatements of the four device entries of
include/nvsf_hip.h section 12 in the reference's dtypes (numpy 2 promotion: a Python float beside an fp32 array is cast to fp32)."""
import os

import numpy as np

import depth_image_oracle as DO

HERE = os.path.dirname(os.path.abspath(__file__))
SCALE, OFFSET, LIDAR_MAX_DEPTH_M = 0.01, [1.5, -2.0, 0.25], 80.0
FAR_PIXEL = (0, 30, 500)  # (frame, row, column) of the one range pixel set beyond 80 m
FAR_RANGE = 85.0
EPS_ROUND = 1e-3


def fixture():
    return dict(np.load(os.path.join(HERE, "golden", "object_masks.npz")))


def scene_pose(pose_world, scale=SCALE, offset=OFFSET):
    """A metre-frame pose of depth_image.npz taken into scene units: the reference's `T[:3, 3] / scale + offset` brings it back."""
    T = np.array(pose_world, dtype=np.float32, copy=True)
    T[:3, 3] = ((T[:3, 3].astype(np.float64) - np.asarray(offset)) * scale).astype(np.float32)
    return T


def inputs():
    """What generator and tests both start from: range images in scene units (frame 0 with its far pixel), poses in scene units."""
    dx = DO.fixture()
    range_m = dx["range_m"].copy()
    f, j, i = FAR_PIXEL
    range_m[f, j, i] = FAR_RANGE
    depth = range_m * np.float32(SCALE)  # scene units, fp32
    assert depth.dtype == np.float32
    return {"depth": depth, "poses": np.stack([scene_pose(p) for p in dx["poses"]]), "poses_lidar": np.stack([scene_pose(p) for p in dx["poses_lidar"]]),
            "K": dx["K"], "H": int(dx["H"]), "W": int(dx["W"]), "fov": tuple(float(v) for v in dx["fov"]),
            "fov_hoz": tuple(float(v) for v in dx["fov_hoz"]), "Hl": depth.shape[1], "Wl": depth.shape[2]}


def annotations(fx):
    return [{"class": "car", "vertices": v} for v in fx["box_vertices"]]


def unpack(fx, key, shape):
    n = int(np.prod(shape))
    return np.unpackbits(fx[key])[:n].reshape(shape).astype(bool)


def sparse_image(fx, key, shape):
    img = np.zeros(int(np.prod(shape)), np.float32)
    img[fx[key + "_idx"]] = fx[key + "_val"]
    return img.reshape(shape)


# ---- restatements ----------------------------------------------------------------------------------------------------------------

def points_in_hulls(points, hulls):
    """Entry 1: OR over the boxes of `every half-space has ((nx x + ny y) + nz z) + d <= 0` in fp64."""
    p = np.asarray(points, np.float32).astype(np.float64)
    out = np.zeros(p.shape[0], bool)
    for h in hulls:
        inside = np.ones(p.shape[0], bool)
        for nx, ny, nz, d in h:
            inside &= ((p[:, 0] * nx + p[:, 1] * ny) + p[:, 2] * nz) + d <= 0.0
        out |= inside
    return out


def pano_constants(H, W, fov, fov_hoz, max_depth):
    fov_up, fov_v = fov
    fov_hoz_up, fov_h = fov_hoz
    return (np.float32(fov_hoz_up * np.pi / 180), np.float32((fov_h * np.pi / 180) / W), np.float32((fov_v - fov_up) / 180 * np.pi),
            np.float32(fov_v / 180 * np.pi / H), np.float32(max_depth))


def pano_coordinates(points, H, W, fov, fov_hoz, max_depth, dtype=np.float32):
    """dist and the unrounded (row, column) of convert.py:137-163 in `dtype` (fp32: as the reference; fp64: for the margins)."""
    p = np.asarray(points, np.float32)[:, :3].astype(dtype)
    az0, step_h, el0, step_v, _ = (dtype(v) for v in pano_constants(H, W, fov, fov_hoz, max_depth))
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    xx, yy = x * x, y * y
    dist = np.sqrt((xx + yy) + z * z)
    beta = az0 - np.arctan2(y, x)
    alpha = np.arctan2(z, np.sqrt(xx + yy)) + el0
    return dist, dtype(H) - alpha / step_v, beta / step_h


def lidar_to_pano(points, payload, H, W, fov, fov_hoz, max_depth):
    """Entry 2: (pano, payload image) fp32, the winner of a pixel = smallest (dist bits, index)."""
    dist, rf, cf = pano_coordinates(points, H, W, fov, fov_hoz, max_depth)
    assert dist.dtype == np.float32 and rf.dtype == np.float32 and cf.dtype == np.float32
    r, c = np.rint(rf), np.rint(cf)
    keep = (dist < np.float32(max_depth)) & (dist != 0) & (r >= 0) & (r < H) & (c >= 0) & (c < W)
    idx = np.nonzero(keep)[0]
    key = (dist[idx].view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
    ws = np.full(H * W, np.iinfo(np.uint64).max, np.uint64)
    np.minimum.at(ws, r[idx].astype(np.int64) * W + c[idx].astype(np.int64), key)
    hit = ws != np.iinfo(np.uint64).max
    pano, img = np.zeros(H * W, np.float32), np.zeros(H * W, np.float32)
    pano[hit] = (ws[hit] >> np.uint64(32)).astype(np.uint32).view(np.float32)
    if payload is not None:
        img[hit] = np.asarray(payload, np.float32)[(ws[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)]
    return pano.reshape(H, W), img.reshape(H, W)


def range_image_object_mask(range_m, hulls, fov, fov_hoz, max_depth):
    """Entry 3 = entry 2 over the cloud of the range image with entry 1's mask as payload."""
    H, W = range_m.shape
    pc = DO.range_cloud(range_m, fov, fov_hoz)
    return lidar_to_pano(pc, points_in_hulls(pc, hulls).astype(np.float32), H, W, fov, fov_hoz, max_depth)[1]


def box_mask_image(boxes, H, W):
    """Entry 4."""
    m = np.zeros((H, W), bool)
    for x0, y0, x1, y1 in np.asarray(boxes).reshape(-1, 4):
        if x1 >= x0 and y1 >= y0:
            m[max(y0, 0):y1 + 1, max(x0, 0):x1 + 1] = True
    return m


def rounding_margin(points, H, W, fov, fov_hoz, max_depth):
    """Per point, in fp64: the distance of its fractional row / column from the nearest rounding boundary (x.5), for the points the
    z-buffer can keep (inside the range and within half a pixel of the image); inf for the others."""
    dist, rf, cf = pano_coordinates(points, H, W, fov, fov_hoz, max_depth, dtype=np.float64)
    near = (dist < max_depth * (1 + 1e-6)) & (rf > -1) & (rf < H + 1) & (cf > -1) & (cf < W + 1)
    m = np.minimum(np.abs(rf - np.floor(rf) - 0.5), np.abs(cf - np.floor(cf) - 0.5))
    return np.where(near, m, np.inf), rf, cf


def borderline_pixels(points, H, W, fov, fov_hoz, max_depth, eps=EPS_ROUND):
    """bool [H, W]: every pixel a point within eps of a rounding boundary can reach by rounding either way -> (mask, such points)."""
    m, rf, cf = rounding_margin(points, H, W, fov, fov_hoz, max_depth)
    close = m < eps
    mask = np.zeros((H, W), bool)
    for dr in (-eps, eps):
        for dc in (-eps, eps):
            r, c = np.rint(rf[close] + dr).astype(np.int64), np.rint(cf[close] + dc).astype(np.int64)
            ok = (r >= 0) & (r < H) & (c >= 0) & (c < W)
            mask[r[ok], c[ok]] = True
    return mask, int(close.sum())


def face_margin(points, hulls):
    """Smallest distance of any point from any supporting plane of any box, over the points within 1 m of that box."""
    p = np.asarray(points, np.float32).astype(np.float64)
    best = np.inf
    for h in hulls:
        s = p @ h[:, :3].T + h[:, 3]          # [P, K] signed distances
        near = s.max(1) < 1.0                 # inside or within 1 m of the box
        if near.any():
            best = min(best, float(np.abs(s[near]).min()))
    return best
