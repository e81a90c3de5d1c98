"""Fixture generator for the prediction export and the sensor change: runs the reference's own code on the CPU --
nvsf/lib/convert.py::pano_to_lidar_with_intensities, nvsf/nerf/utils.py::get_pcd_bound_to_world and utils.py::linear_to_srgb, loaded as
tests/golden/golden_object_masks.py::load_reference loads them -- and writes tests/golden/export.npz:

    python tests/golden/golden_export.py

Stored
  * pano crop: 16 x 256 pixels of a street range image of tests/golden/depth_image.npz (export_oracle.CROP) in scene units, treated as a
    whole pano with H = 16, W = 256, a seeded tenth of its remaining pixels set to 0 as the ray-drop gate would, a seeded payload plane;
    the reference's LiDAR-frame cloud (pano_to_lidar_with_intensities, xyz / scale as utils.py:463) and its world cloud
    (get_pcd_bound_to_world, float64 [n, 4]) for the scene-unit pose of the frame, scale 0.01, offset (1.5, -2, 0.25);
  * e_ref_lidar, e_ref_world: the largest per-point distance of those two clouds from the float64 restatement of the same formulas
    (tests/export_oracle.py) -- the reference's own fp32 noise floor;
  * quantisation: a seeded plane with the values 0, 1 and k / 255 planted, and `(x * 255).astype(np.uint8)` of it; a seeded image, the
    reference's linear_to_srgb of it (fp32) and the uint8 of that, e_ref_srgb = its largest distance from float64, and the pixels whose
    float64 value times 255 lies within 1e-3 of an integer;
  * sensor change: seeded poses in metres and the result of base_dataset.py:182-231 (the change, then the recentring into scene units)
    under three changes: LiDAR only, camera only, everything at once.  BaseDataset.__post_init__ cannot run as a whole here (it reads
    files and needs cv2), so `reference_sensor_change` below reads exactly those lines from the reference tree at run time and executes
    them on a namespace standing for the data set: the arrays are the output of the reference's own statements, none of which is
    written down here.
Conditions asserted here and again in tests/test_export_cpu.py: between 10 % and 90 % of the crop dropped; at most 1 % of the sRGB
values on the boundary list; the fixture under 300 KB.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import depth_image_oracle as DO  # noqa: E402
import export_oracle as EO  # noqa: E402
import object_masks_oracle as OM  # noqa: E402
from golden_object_masks import REF, load_reference  # noqa: E402


def reference_sensor_change(poses, poses_lidar, intrinsics, cfg, change):
    """RUNS the reference's own lines: nvsf/nerf/dataset/base_dataset.py:182-231 -- the body of the sensor-change branch of
    BaseDataset.__post_init__ and the recentring into scene units that follows it -- are read from the reference tree when the generator
    runs, dedented and executed with `self` bound to a namespace that holds the fields those lines read (metre poses fp32 [F, 4, 4],
    intrinsics, sizes, the change under the reference's argument names) and with the `np` and `Rotation` the module imports.
    __post_init__ as a whole cannot run here (it reads files and needs cv2).  Returns the namespace: what the data set then holds."""
    import textwrap
    import warnings
    from scipy.spatial.transform import Rotation
    s = types.SimpleNamespace(**EO.DEFAULTS)
    s.__dict__.update(change)
    s.poses, s.poses_lidar, s.intrinsics = poses.copy(), poses_lidar.copy(), np.array(intrinsics, dtype=np.float64)
    s.H, s.W, s.H_lidar, s.W_lidar = cfg["H"], cfg["W"], cfg["H_lidar"], cfg["W_lidar"]
    s.intrinsics_lidar, s.intrinsics_hoz_lidar, s.scale, s.offset = cfg["intrinsics_lidar"], cfg["intrinsics_hoz_lidar"], cfg["scale"], cfg["offset"]
    lines = open(os.path.join(REF, "nvsf", "nerf", "dataset", "base_dataset.py")).read().split("\n")
    first, last = 182, 231  # 1-based, inclusive
    assert "Rotation.from_euler" in lines[first - 1] and "delta_orientation" in lines[first - 1], lines[first - 1]
    assert lines[last - 1].strip().startswith("self.poses[:, :3, -1] =") and "Disable validation" in lines[222 - 1], lines[last - 1]
    branch, after = lines[first - 1:227], lines[228:last]   # the `if` body (:182-227), then the recentring at the method's level (:229-231)
    env = {"np": np, "Rotation": Rotation, "self": s}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)  # np.row_stack
        for block in (branch, after):
            exec(compile(textwrap.dedent("\n".join(block)), "base_dataset.py", "exec"), env)
    assert s.images is None and s.images_lidar is None and s.image_depths is None  # the branch's "Disable validation" ran
    return s


def seeded_poses(rng, F):
    """Rigid metre poses: a yawed, slightly tilted rig some hundred metres from the origin."""
    from scipy.spatial.transform import Rotation
    out = np.tile(np.eye(4, dtype=np.float64), (F, 1, 1))
    for f in range(F):
        out[f, :3, :3] = Rotation.from_euler("xyz", [rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-180, 180)], degrees=True).as_matrix()
        out[f, :3, 3] = [rng.uniform(-300, 300), rng.uniform(-300, 300), rng.uniform(-5, 5)]
    return out.astype(np.float32)


def main():
    assert type(1.5 - np.float32(1)) is np.float32, "the fixture pins numpy 2 promotion"
    convert, _, utils = load_reference()
    rng = np.random.default_rng(20262)
    out = {"numpy_version": np.array(np.__version__)}

    # ---- the pano crop and its two clouds
    dx = DO.fixture()
    f, j0, i0, H, W = EO.CROP
    pano = (dx["range_m"][f, j0:j0 + H, i0:i0 + W] * np.float32(EO.SCALE)).astype(np.float32)
    pano[(rng.random((H, W)) < 0.1)] = 0.0
    payload = rng.random((H, W)).astype(np.float32)
    dropped = float((pano == 0).mean())
    assert 0.1 <= dropped <= 0.9, dropped
    pose = OM.scene_pose(dx["poses_lidar"][f], EO.SCALE, EO.OFFSET)
    fov, fov_hoz = list(EO.FOV), list(EO.FOV_HOZ)
    ref_lidar = convert.pano_to_lidar_with_intensities(pano, payload, fov, fov_hoz)
    ref_lidar[:, :3] = ref_lidar[:, :3] / EO.SCALE
    assert ref_lidar.dtype == np.float32
    loader = types.SimpleNamespace(_data=types.SimpleNamespace(intrinsics_lidar=fov, intrinsics_hoz_lidar=fov_hoz, scale=EO.SCALE, offset=EO.OFFSET))
    batch = {"poses_lidar": torch.from_numpy(pose[None].copy())}
    ref_world = utils.get_pcd_bound_to_world(pano, payload, loader, batch)
    assert ref_world.dtype == np.float64 and ref_world.shape == ref_lidar.shape
    # the deviation the product records: the call rescales the pose of the batch it is given
    assert not np.array_equal(batch["poses_lidar"][0].numpy(), pose)
    assert np.array_equal(batch["poses_lidar"][0].numpy(), EO.world_matrix(pose, EO.SCALE, EO.OFFSET))
    want_lidar = EO.pano_cloud(pano, payload, fov, fov_hoz, EO.SCALE)
    want_world = EO.world_affine(want_lidar, EO.world_matrix(pose, EO.SCALE, EO.OFFSET))
    assert np.array_equal(ref_lidar[:, 3], payload.reshape(-1)[EO.kept(pano)]) and np.array_equal(ref_world[:, 3], ref_lidar[:, 3].astype(np.float64))
    e_lidar, e_world = EO.distance(ref_lidar, want_lidar), EO.distance(ref_world, want_world)
    print(f"crop: {ref_lidar.shape[0]} points of {H * W}, {dropped:.3f} dropped, e_ref_lidar {e_lidar:.3e} m, e_ref_world {e_world:.3e} m, "
          f"|world| <= {np.abs(ref_world[:, :3]).max():.1f} m")
    out.update(pano=pano, payload=payload, pose_lidar=pose, ref_lidar=ref_lidar, ref_world=ref_world, e_ref_lidar=np.float64(e_lidar),
               e_ref_world=np.float64(e_world))

    # ---- quantisation
    q = rng.random((48, 64)).astype(np.float32)
    q.reshape(-1)[:256] = np.arange(256, dtype=np.float32) / np.float32(255.0)
    q.reshape(-1)[256:259] = [0.0, 1.0, np.float32(1.0) - np.float32(2.0 ** -24)]
    prod = q * 255
    assert prod.dtype == np.float32 and prod.min() >= 0 and prod.max() < 256
    q_u8 = prod.astype(np.uint8)
    assert np.array_equal(q_u8, EO.quantize(q))
    img = rng.random((24, 32, 3)).astype(np.float32)
    img.reshape(-1)[:64] = rng.uniform(0.0, 0.0062616, 64).astype(np.float32)  # both sides of the branch point
    srgb = utils.linear_to_srgb(torch.from_numpy(img)).numpy()
    assert srgb.dtype == np.float32
    srgb_u8 = (srgb * 255).astype(np.uint8)
    srgb64 = EO.linear_to_srgb(img)
    e_srgb = float(np.abs(srgb.astype(np.float64) - srgb64).max())
    boundary = EO.srgb_boundary(img)
    assert boundary.size <= 0.01 * img.size, boundary.size
    off = np.ones(img.size, bool)
    off[boundary] = False
    assert np.array_equal(srgb_u8.reshape(-1)[off], np.trunc(srgb64.reshape(-1) * 255.0).astype(np.uint8)[off])
    print(f"quantisation: e_ref_srgb {e_srgb:.3e}, {boundary.size} of {img.size} sRGB values within {EO.SRGB_EPS} of an integer")
    out.update(q_in=q, q_u8=q_u8, srgb_in=img, srgb_ref=srgb, srgb_u8=srgb_u8, e_ref_srgb=np.float64(e_srgb), srgb_boundary=boundary.astype(np.int32))

    # ---- sensor change
    F = 3
    poses_m, poses_lidar_m = seeded_poses(rng, F), seeded_poses(rng, F)
    K = np.array([[552.554261, 0.0, 682.049453 / 4], [0.0, 552.554261, 238.769549 / 4], [0.0, 0.0, 1.0]])
    out.update(sc_poses_m=poses_m, sc_poses_lidar_m=poses_lidar_m, sc_K=K)
    for name, change in EO.CHANGES.items():
        s = reference_sensor_change(poses_m, poses_lidar_m, K, EO.SENSOR, change)
        assert s.poses.dtype == np.float32 and s.poses_lidar.dtype == np.float32
        out.update({f"sc_{name}_poses": s.poses, f"sc_{name}_poses_lidar": s.poses_lidar, f"sc_{name}_K": s.intrinsics,
                    f"sc_{name}_sizes": np.array([s.H, s.W, s.H_lidar, s.W_lidar], np.int64),
                    f"sc_{name}_fov": np.array(list(s.intrinsics_lidar) + list(s.intrinsics_hoz_lidar), np.float64)})
    path = os.path.join(HERE, "export.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 300_000, size
    print("export.npz", size, "bytes")


if __name__ == "__main__":
    main()
