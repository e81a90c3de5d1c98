"""Fixture generator for the LiDAR-projected camera depth maps: runs the reference's own three functions on the CPU --
nvsf/lib/convert.py::pano_to_lidar, nvsf/nerf/dataset/dataset_utils.py::lidar2points2d and ::get_lidar_depth_image, chained as
nvsf/nerf/dataset/base_dataset.py:153-157 chains them (import-only dependencies stubbed; none of the three uses them) -- and writes
tests/golden/depth_image.npz:

    python tests/golden/golden_depth_image.py

Inputs
  * two 66 x 1030 range images of a synthetic street: a ground plane 1.7 m under the sensor, walls at 4-60 m per column, 30 % dropped
    pixels; ranges on a 1/512 m raster (a spinning LiDAR reports a few millimetres; it also keeps the file small);
  * a KITTI-360-like rig: camera 376 x 1408, fx = fy = 552.55, cx = 682.05, cy = 238.77, axes permuted so that the camera looks along the
    LiDAR's +x, a lever arm with components between 2 cm and 80 cm, a 0.02 rad yaw; lidar2cam = inv(pose) @ pose_lidar in fp32;
  * a 200-point list seen through an exactly representable camera (fx = fy = 512, cx = 704, cy = 188, a pure axis permutation): points
    behind the camera (one of which the reference's clip to 1e-5 puts INSIDE the image), points exactly on all four field-of-view
    bounds, two at equal depth in one pixel.
Stored
  * the inputs;
  * the reference's clouds.  A cloud is dirs * range at the non-zero pixels and dirs[j, i] = (ca[j] cb[i], ca[j] sb[i], sa[j]) with
    ca, sa = cos, sin of the 66 elevations and cb, sb of the 1030 azimuths: the four vectors are stored, the generator ASSERTS that
    they rebuild the reference's clouds bit for bit, and tests/depth_image_oracle.py::fixture_cloud rebuilds them (two clouds in full
    would be 1.1 MB);
  * fp64 (u, v, z) of every point of the list, and of every cloud point that lands within one pixel of the image (any other point is
    more than a pixel away from mattering), with the point's index in the cloud;
  * the expected images in sparse form: flat pixel index and the depth rounded to fp32, which is what the reference keeps of its
    float64 image (base_dataset.py:240, `.float()`).
"""
import importlib.util
import os
import sys
import types

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
H, W, HL, WL = 376, 1408, 66, 1030
FOV, FOV_HOZ = (2.0, 26.9), (180.0, 360.0)


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    for name in ("cv2", "trimesh", "matplotlib", "matplotlib.pyplot", "open3d", "tqdm", "nvsf", "nvsf.lib", "nvsf.lib.tools"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["tqdm"].tqdm = lambda x, *a, **k: x
    ema = types.ModuleType("torch_ema")
    ema.ExponentialMovingAverage = object
    sys.modules.setdefault("torch_ema", ema)
    sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    sys.modules["nvsf.lib"].tools = sys.modules["nvsf.lib.tools"]
    convert = _load("nvsf.lib.convert", "nvsf/lib/convert.py")
    sys.modules["nvsf.lib.convert"] = convert
    sys.modules["nvsf.lib"].convert = convert
    du = _load("nvsf.nerf.dataset.dataset_utils", "nvsf/nerf/dataset/dataset_utils.py")
    return convert, du


def street(rng):
    j, i = np.meshgrid(np.arange(HL, dtype=np.float64), np.arange(WL, dtype=np.float64), indexing="ij")
    alpha = (FOV[0] - j / HL * FOV[1]) / 180 * np.pi
    wall = np.repeat(rng.uniform(4.0, 60.0, (WL + 19) // 20), 20)[:WL][None, :] / np.cos(alpha)
    with np.errstate(divide="ignore"):
        ground = np.where(alpha < 0, 1.7 / np.sin(-alpha), np.inf)
    r = np.minimum(wall, ground)
    r = np.round(r * 512) / 512
    r[rng.random((HL, WL)) < 0.3] = 0.0
    return r.astype(np.float32)


def rig(rng, frame):
    """(pose, pose_lidar) fp32: camera-to-world and LiDAR-to-world."""
    yaw = 0.02
    perm = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])  # camera x = -LiDAR y, y = -LiDAR z, z = LiDAR x
    rz = np.array([[np.cos(yaw), -np.sin(yaw), 0.0], [np.sin(yaw), np.cos(yaw), 0.0], [0.0, 0.0, 1.0]])
    l2c = np.eye(4)
    l2c[:3, :3] = perm @ rz
    l2c[:3, 3] = [0.02, -0.25, -0.8] if frame == 0 else [-0.05, -0.8, -0.3]
    heading = 0.3 + 0.05 * frame
    pose_lidar = np.eye(4)
    pose_lidar[:3, :3] = [[np.cos(heading), -np.sin(heading), 0.0], [np.sin(heading), np.cos(heading), 0.0], [0.0, 0.0, 1.0]]
    pose_lidar[:3, 3] = [12.0 + 1.5 * frame, -7.0, 1.9]
    pose = pose_lidar @ np.linalg.inv(l2c)
    return pose.astype(np.float32), pose_lidar.astype(np.float32)


def point_list(rng):
    pts = np.zeros((200, 3), np.float32)
    pts[:, 0] = rng.uniform(2.0, 40.0, 200)
    pts[:, 1] = rng.uniform(-1.2, 1.2, 200) * pts[:, 0]
    pts[:, 2] = rng.uniform(-0.4, 0.4, 200) * pts[:, 0]
    pts[:40, 0] *= -1.0                      # behind the camera: z is clipped to 1e-5, (u, v) fly off -- except for the next one
    pts[0] = [-1.0, -(1.375 + 2.0 ** -17), -(0.3671875 + 2.0 ** -18)]  # q0 = 2^-8, q1 = 2^-9, z -> 1e-5: pixel (195, 390) with depth 1e-5, as the reference has it
    pts[40] = [4.0, 5.5, 0.0]                # u = 0 exactly: inside
    pts[41] = [4.0, -5.5, 0.0]               # u = W exactly: outside
    pts[42] = [4.0, 0.0, 1.46875]            # v = 0 exactly: inside
    pts[43] = [4.0, 0.0, -1.46875]           # v = H exactly: outside
    pts[44] = [8.0, 11.0, 2.9375]            # the corner (0, 0): inside
    pts[45] = [8.0, -11.0, -2.9375]          # the corner (W, H): outside
    pts[46] = [16.0, 1.01, 1.01]             # two points at equal depth in one pixel ...
    pts[47] = [16.0, 1.015, 1.015]
    pts[48] = [12.0, 1.0, 1.0]               # ... and a nearer and a farther one in a pixel of their own pair
    pts[49] = [12.5, 1.04, 1.04]
    return pts


def main():
    convert, du = load_reference()
    rng = np.random.default_rng(20260)
    K = np.array([[552.55, 0.0, 682.05], [0.0, 552.55, 238.77], [0.0, 0.0, 1.0]])
    out = {"K": K, "H": np.int64(H), "W": np.int64(W), "fov": np.array(FOV), "fov_hoz": np.array(FOV_HOZ)}
    # the factored directions, checked against the reference's cloud of an all-ones image
    i, j = np.arange(WL, dtype=np.float32), np.arange(HL, dtype=np.float32)
    beta = -(i - WL / 2) / WL * FOV_HOZ[1] / 180 * np.pi
    alpha = (FOV[0] - j / HL * FOV[1]) / 180 * np.pi
    assert beta.dtype == np.float32 and alpha.dtype == np.float32
    ca, sa, cb, sb = np.cos(alpha), np.sin(alpha), np.cos(beta), np.sin(beta)
    out.update(ca=ca, sa=sa, cb=cb, sb=sb)
    dirs = np.stack([ca[:, None] * cb[None, :], ca[:, None] * sb[None, :], np.broadcast_to(sa[:, None], (HL, WL))], -1)
    ones = convert.pano_to_lidar(np.ones((HL, WL), np.float32), list(FOV), list(FOV_HOZ))
    assert ones.dtype == np.float32 and np.array_equal(ones.view(np.uint32), dirs.reshape(-1, 3).view(np.uint32))
    ranges, poses, poses_lidar, l2cs = [], [], [], []
    stats = []
    for f in range(2):
        r = street(rng)
        pose, pose_lidar = rig(rng, f)
        l2c = np.linalg.inv(pose) @ pose_lidar  # base_dataset.py:155, fp32
        assert l2c.dtype == np.float32
        pc = convert.pano_to_lidar(r, list(FOV), list(FOV_HOZ))
        rebuilt = (dirs * r[..., None])[r != 0.0]
        assert pc.dtype == np.float32 and np.array_equal(pc.view(np.uint32), rebuilt.view(np.uint32)), "factored cloud != reference cloud"
        pts = du.lidar2points2d(pc, K, l2c)
        img = du.get_lidar_depth_image(pts, img_shape=(H, W))  # divides pts in place: pts is (u, v, z) afterwards
        assert pts.dtype == np.float64 and img.dtype == np.float64
        u, v = pts[:, 0], pts[:, 1]
        near = np.nonzero((u >= -1) & (u < W + 1) & (v >= -1) & (v < H + 1))[0]
        inside = (u >= 0) & (u < W) & (v >= 0) & (v < H)
        val = img.astype(np.float32)
        idx = np.nonzero(val.reshape(-1))[0]
        assert np.count_nonzero(img) == idx.size
        out.update({f"f{f}_view_idx": near.astype(np.int32), f"f{f}_view_uvz": pts[near], f"f{f}_n_points": np.int64(pc.shape[0]),
                    f"f{f}_img_idx": idx.astype(np.int32), f"f{f}_img_val": val.reshape(-1)[idx]})
        frac = np.minimum.reduce([u[inside] - np.floor(u[inside]), np.ceil(u[inside]) - u[inside], v[inside] - np.floor(v[inside]),
                                  np.ceil(v[inside]) - v[inside]])
        stats.append((pc.shape[0], int(inside.sum()), idx.size, int((frac < 1e-3).sum()), int((frac < 1e-4).sum())))
        ranges.append(r); poses.append(pose); poses_lidar.append(pose_lidar); l2cs.append(l2c)
    out.update(range_m=np.stack(ranges), poses=np.stack(poses), poses_lidar=np.stack(poses_lidar), lidar2cam=np.stack(l2cs))
    # the point list through the exactly representable camera
    lk = np.array([[512.0, 0.0, 704.0], [0.0, 512.0, 188.0], [0.0, 0.0, 1.0]])
    ll2c = np.array([[0, -1, 0, 0], [0, 0, -1, 0], [1, 0, 0, 0], [0, 0, 0, 1]], np.float32)
    lp = point_list(rng)
    pts = du.lidar2points2d(lp.copy(), lk, ll2c)
    img = du.get_lidar_depth_image(pts, img_shape=(H, W))
    val = img.astype(np.float32)
    idx = np.nonzero(val.reshape(-1))[0]
    assert val[195, 390] == np.float32(1e-5) and val[0, 0] == 8.0 and val.reshape(-1)[idx].size == np.count_nonzero(img)
    out.update(list_points=lp, list_K=lk, list_lidar2cam=ll2c, list_uvz=pts, list_img_idx=idx.astype(np.int32), list_img_val=val.reshape(-1)[idx])
    path = os.path.join(HERE, "depth_image.npz")
    np.savez_compressed(path, **out)
    print("depth_image.npz", os.path.getsize(path), "bytes")
    for f, s in enumerate(stats):
        print(f"frame {f}: {s[0]} points, {s[1]} in view, {s[2]} non-empty pixels, {s[3]} within 1e-3 px of a pixel boundary, {s[4]} within 1e-4 px")
    print("list:", idx.size, "non-empty pixels")


if __name__ == "__main__":
    main()
