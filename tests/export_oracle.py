"""CPU side of the prediction-export tests: the fixture of tests/golden/golden_export.py and float64 numpy restatements of the device
entries of include/nvsf_hip.h section 14 -- the oracle for the shapes the fixture does not store.

Distances between clouds are per-point Euclidean distances over x, y, z (metres); `e_ref_*` of the fixture is the largest such distance
of the REFERENCE's fp32 result from the float64 restatement below, i.e. the reference's own fp32 noise floor."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SCALE, OFFSET = 0.01, [1.5, -2.0, 0.25]
FOV, FOV_HOZ = (2.0, 26.9), (180.0, 360.0)
CROP = (0, 25, 400, 16, 256)  # frame, first row, first column, rows, columns of the street range image the fixture's pano is cut from
SRGB_EPS = 1e-3               # a value whose product by 255 lies this close to an integer may round to either side

# the sensor-change cases of the fixture: the reference's argument names (base_dataset.py:43-52); SENSOR = the recording's sensors
CHANGES = {
    "lidar": dict(delta_position=[0.5, -1.25, 0.75], delta_orientation=[2.0, -3.5, 30.0], H_lidar_new=32, W_lidar_new=515,
                  intrinsics_lidar_new=[10.0, 40.0], intrinsics_hoz_lidar_new=[90.0, 180.0]),
    "camera": dict(delta_pos_camera=[1.0, 0.25, -0.5], delta_orient_camera=[5.0, -2.0, 12.5], H_new=48, W_new=160),
    "all": dict(delta_position=[-2.0, 0.5, 1.5], delta_orientation=[-1.0, 4.0, -75.0], H_lidar_new=16, W_lidar_new=256,
                intrinsics_lidar_new=[15.0, 30.0], intrinsics_hoz_lidar_new=[180.0, 360.0], delta_pos_camera=[-0.75, 2.0, 0.1],
                delta_orient_camera=[-3.0, 6.0, -20.0], H_new=100, W_new=301),
}
DEFAULTS = dict(delta_position=[0., 0., 0.], delta_orientation=[0., 0., 0.], H_lidar_new=0, W_lidar_new=0, intrinsics_lidar_new=[0.0, 0.0],
                intrinsics_hoz_lidar_new=[0.0, 0.0], delta_pos_camera=[0., 0., 0.], delta_orient_camera=[0., 0., 0.], H_new=0, W_new=0)
SENSOR = dict(H=94, W=352, H_lidar=66, W_lidar=1030, intrinsics_lidar=[2.0, 26.9], intrinsics_hoz_lidar=[180.0, 360.0], scale=0.01,
              offset=[1.5, -2.0, 0.25])


def fixture():
    return dict(np.load(os.path.join(HERE, "golden", "export.npz")))


def kept(range_image):
    """Row-major indices of the pixels that give a point: range != 0 (-0.0 is dropped, NaN and negative values are kept)."""
    return np.nonzero(np.asarray(range_image, np.float32).reshape(-1) != 0.0)[0]


def pano_cloud(range_image, payload, fov, fov_hoz, scale):
    """convert.pano_to_lidar_with_intensities (convert.py:221-268) and the division by the scale (utils.py:463) in float64 on the fp32
    range image; the scale is the fp32 value numpy divides an fp32 array by.  -> [n, 4] float64, row-major pixel order."""
    r = np.asarray(range_image, np.float32).astype(np.float64)
    H, W = r.shape
    fov_up, fov_v = (float(v) for v in fov)
    fov_h = float(fov_hoz[1])
    i, j = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), indexing="xy")
    beta = -(i - W / 2) / W * fov_h / 180 * np.pi
    alpha = (fov_up - j / H * fov_v) / 180 * np.pi
    dirs = np.stack([np.cos(alpha) * np.cos(beta), np.cos(alpha) * np.sin(beta), np.sin(alpha)], -1)
    with np.errstate(invalid="ignore"):  # an infinite range times a zero direction
        pts = dirs * r[..., None] / float(np.float32(scale))
    pay = np.zeros((H, W), np.float64) if payload is None else np.asarray(payload, np.float32).astype(np.float64)
    idx = kept(range_image)
    return np.concatenate([pts.reshape(-1, 3)[idx], pay.reshape(-1, 1)[idx]], axis=1)


def world_matrix(pose_lidar, scale, offset):
    """utils.py:466-467 on a copy: fp32 pose, translation t / scale + offset rounded to fp32."""
    T = np.array(pose_lidar, dtype=np.float32, copy=True)
    T[:3, 3] = (T[:3, 3] / scale) + np.asarray(offset, dtype=np.float64)
    return T


def world_affine(cloud, T):
    """The float64 affine of a cloud [n, 4] under the 4 x 4 matrix T; column 3 is carried over."""
    c = np.asarray(cloud).astype(np.float64)
    T = np.asarray(T).astype(np.float64)
    out = c.copy()
    with np.errstate(invalid="ignore"):  # NaN and infinite points stay what they are
        out[:, :3] = c[:, :3] @ T[:3, :3].T + T[:3, 3]
    return out


def distance(a, b):
    """Largest per-point Euclidean distance over x, y, z; 0 for empty clouds."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.sqrt(((a[:, :3] - b[:, :3]) ** 2).sum(1)).max()) if a.shape[0] else 0.0


def quantize(x):
    """(x * 255).astype(np.uint8) with the fp32 product; where the cast is undefined: product <= -1 -> 0, >= 256 -> 255, NaN -> 0."""
    p = (np.asarray(x, np.float32) * np.float32(255.0)).astype(np.float64)
    p = np.where(np.isnan(p), 0.0, p)
    return np.trunc(np.clip(p, 0.0, 255.0)).astype(np.uint8)


def linear_to_srgb(x):
    """utils.linear_to_srgb (utils.py:31-36) in float64 on the fp32 input."""
    x = np.asarray(x, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(x < 0.0031308, 12.92 * x, 1.055 * np.power(x, 0.41666) - 0.055)


def srgb_boundary(x, eps=SRGB_EPS):
    """Flat indices of the values whose float64 sRGB product by 255 lies within eps of an integer."""
    p = linear_to_srgb(x).reshape(-1) * 255.0
    return np.nonzero(np.abs(p - np.rint(p)) < eps)[0]


def seeded_range_image(H, W, seed, drop=0.3, range_m=(2.0, 60.0)):
    """A seeded range image in scene units with ranges drawn inside `range_m` metres and about `drop` of its pixels 0, and a payload plane."""
    rng = np.random.default_rng(seed)
    r = (rng.uniform(range_m[0], range_m[1], (H, W)) * SCALE).astype(np.float32)
    r[rng.random((H, W)) < drop] = 0.0
    return r, rng.random((H, W)).astype(np.float32)

