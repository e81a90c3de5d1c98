"""CPU half of the prediction export: the sensor change (nvsf/nerf/dataset/formats.py) against the fixture the reference's lines produced
(tests/golden/golden_export.py), FrameSet's constructor, the file writers of nvsf/nerf/export.py and the float64 oracle of
tests/export_oracle.py against the reference's own clouds.

Bounds.  Rotation blocks, sizes and intrinsics of the sensor change are compared exactly.  Translations: the reference changes the metre
pose and recentres afterwards, the product works on the stored scene-unit pose, so one fp32 rounding comes from that stored pose and one
from ours: 2 ulps of the largest |translation|.  Text clouds read back within 5e-7 (`%f` keeps six decimals).  The oracle reproduces the
reference's clouds within the e_ref the generator measured, and its uint8 planes exactly (off the boundary list for sRGB)."""
import os

import numpy as np
import pytest
import torch

import export_oracle as EO
import object_masks_oracle as OM


@pytest.fixture(scope="module")
def fx():
    return EO.fixture()


def _change(name):
    from nvsf.nerf.dataset import formats as F
    return F.SensorChange(**EO.CHANGES[name])


def _scene_poses(poses_m):
    """What a transforms file of this project holds for metre poses: (t - offset) * scale, rounded to fp32 once."""
    return np.stack([OM.scene_pose(p, EO.SENSOR["scale"], EO.SENSOR["offset"]) for p in poses_m])


def test_fixture_conditions(fx):
    dropped = float((fx["pano"] == 0).mean())
    assert 0.1 <= dropped <= 0.9, dropped
    assert fx["srgb_boundary"].size <= 0.01 * fx["srgb_in"].size
    assert np.array_equal(fx["srgb_boundary"], EO.srgb_boundary(fx["srgb_in"]))
    assert os.path.getsize(os.path.join(EO.HERE, "golden", "export.npz")) < 300_000
    assert fx["pano"].shape == EO.CROP[3:] and fx["ref_lidar"].shape[0] == EO.kept(fx["pano"]).size == fx["ref_world"].shape[0]
    assert fx["e_ref_lidar"] > 0 and fx["e_ref_world"] > 0 and fx["e_ref_srgb"] > 0


def test_sensor_change_defaults_are_the_references():
    from nvsf.nerf.dataset import formats as F
    c = F.SensorChange()
    assert c.is_trivial()
    for k, v in EO.DEFAULTS.items():
        assert list(np.atleast_1d(getattr(c, k))) == list(np.atleast_1d(v)), k
    for k, v in (("delta_position", (0, 0, 1e-3)), ("delta_orientation", (0, 1, 0)), ("H_lidar_new", 32), ("W_lidar_new", 100),
                 ("intrinsics_lidar_new", (0, 30.0)), ("intrinsics_hoz_lidar_new", (90.0, 0)), ("delta_pos_camera", (1, 0, 0)),
                 ("delta_orient_camera", (0, 0, -2)), ("H_new", 4), ("W_new", 4)):
        assert not F.SensorChange(**{k: v}).is_trivial(), k


def test_euler_matrix_is_scipys():
    from scipy.spatial.transform import Rotation
    from nvsf.nerf.dataset import formats as F
    rng = np.random.default_rng(3)
    for _ in range(50):
        a = rng.uniform(-180, 180, 3)
        assert np.abs(F.euler_xyz_matrix(a) - Rotation.from_euler("xyz", a, degrees=True).as_matrix()).max() < 1e-15
    assert np.array_equal(F.world_to_camera_axes([1.0, 2.0, 3.0]), [-2.0, -3.0, 1.0])


@pytest.mark.parametrize("name", ["lidar", "camera", "all"])
def test_apply_sensor_change_equals_the_reference(fx, name):
    from nvsf.nerf.dataset import formats as F
    S = EO.SENSOR
    poses, poses_lidar = _scene_poses(fx["sc_poses_m"]), _scene_poses(fx["sc_poses_lidar_m"])
    keep = (poses.copy(), poses_lidar.copy(), fx["sc_K"].copy())
    got = F.apply_sensor_change(torch.from_numpy(poses) if name == "all" else poses, poses_lidar, fx["sc_K"], S["H"], S["W"], S["H_lidar"], S["W_lidar"],
                                tuple(S["intrinsics_lidar"]), tuple(S["intrinsics_hoz_lidar"]), S["scale"], _change(name))
    assert np.array_equal(poses, keep[0]) and np.array_equal(poses_lidar, keep[1]) and np.array_equal(fx["sc_K"], keep[2])  # inputs untouched
    for key in ("poses", "poses_lidar"):
        want, mine = fx[f"sc_{name}_{key}"], got[key]
        assert mine.dtype == np.float32 and mine.shape == want.shape
        assert np.array_equal(mine[:, :3, :3], want[:, :3, :3]), key       # rotation blocks: exact
        assert np.array_equal(mine[:, 3], want[:, 3])                      # the last row
        bound = 2 * float(np.spacing(np.float32(np.abs(want[:, :3, 3]).max())))
        err = float(np.abs(mine[:, :3, 3].astype(np.float64) - want[:, :3, 3]).max())
        print(f"{name} {key}: translation error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (key, err, bound)
    assert [got["H"], got["W"], got["H_lidar"], got["W_lidar"]] == fx[f"sc_{name}_sizes"].tolist()
    assert np.array_equal(np.asarray(got["intrinsics"], np.float64), fx[f"sc_{name}_K"])
    assert list(got["intrinsics_lidar"]) + list(got["intrinsics_hoz_lidar"]) == fx[f"sc_{name}_fov"].tolist()
    if name == "lidar":   # the camera keeps everything
        assert np.array_equal(got["poses"], poses) and got["intrinsics"] is fx["sc_K"]
    if name == "camera":  # and the LiDAR likewise
        assert np.array_equal(got["poses_lidar"], poses_lidar) and (got["H_lidar"], got["W_lidar"]) == (S["H_lidar"], S["W_lidar"])
        assert got["intrinsics"][0, 0] == fx["sc_K"][0, 0] and got["intrinsics"][1, 1] == fx["sc_K"][1, 1]  # focal lengths stay


def test_zero_change_returns_its_inputs(fx):
    from nvsf.nerf.dataset import formats as F
    S = EO.SENSOR
    poses, poses_lidar = _scene_poses(fx["sc_poses_m"]), _scene_poses(fx["sc_poses_lidar_m"])
    for change in (None, F.SensorChange()):
        got = F.apply_sensor_change(poses, poses_lidar, fx["sc_K"], S["H"], S["W"], S["H_lidar"], S["W_lidar"], (2.0, 26.9), (180.0, 360.0),
                                    S["scale"], change)
        assert got["poses"] is poses and got["poses_lidar"] is poses_lidar and got["intrinsics"] is fx["sc_K"]
        assert (got["H"], got["W"], got["H_lidar"], got["W_lidar"]) == (S["H"], S["W"], S["H_lidar"], S["W_lidar"])
        assert got["intrinsics_lidar"] == (2.0, 26.9) and got["intrinsics_hoz_lidar"] == (180.0, 360.0)
    one = F.apply_sensor_change(poses, poses_lidar, fx["sc_K"], S["H"], S["W"], S["H_lidar"], S["W_lidar"], (2.0, 26.9), (180.0, 360.0), S["scale"],
                                F.SensorChange(W_new=176))  # one size only: the other keeps its value (the recorded deviation)
    assert (one["H"], one["W"]) == (S["H"], 176) and one["intrinsics"][0, 2] == fx["sc_K"][0, 2] * (176 / S["W"]) \
        and one["intrinsics"][1, 2] == fx["sc_K"][1, 2]


def test_frameset_constructor(tmp_path):
    from test_formats_cpu import make_dataset
    from nvsf.nerf.dataset import formats as F
    seq, frames, images, pcs, K = make_dataset(str(tmp_path))
    change = F.SensorChange(delta_position=(0.5, 0.0, 1.0), H_lidar_new=6, W_lidar_new=12, intrinsics_lidar_new=(10.0, 40.0), H_new=5, W_new=4)
    with pytest.raises(ValueError, match="training=False"):
        F.FrameSet(str(tmp_path), seq, "train", 0.01, device="cpu", sensor=change)
    for trivial in (None, F.SensorChange()):  # today's path: even with training=True
        fs = F.FrameSet(str(tmp_path), seq, "train", 0.01, device="cpu", sensor=trivial)
        assert fs.sensor is None and fs.images is not None and fs.images_lidar.shape == (3, 4, 10, 3) and (fs.H, fs.W) == (6, 8)
    plain = F.FrameSet(str(tmp_path), seq, "train", 0.01, device="cpu", training=False)
    fs = F.FrameSet(str(tmp_path), seq, "train", 0.01, device="cpu", training=False, sensor=change, camera_depth=True)
    assert fs.sensor is change and fs.images is None and fs.images_lidar is None and fs.image_depths is None
    assert (fs.H, fs.W, fs.H_lidar, fs.W_lidar) == (5, 4, 8, 12) and fs.intrinsics_lidar == (10.0, 40.0) and fs.intrinsics_hoz_lidar == (180.0, 360.0)
    assert len(fs) == 3 and fs.num_rays == -1 and torch.equal(fs.poses, plain.poses) and torch.equal(fs.times, plain.times)
    want = plain.poses_lidar.numpy().astype(np.float64)
    want[:, :3, 3] += want[:, :3, :3] @ (np.array([0.5, 0.0, 1.0]) * 0.01)
    assert np.array_equal(fs.poses_lidar.numpy(), want.astype(np.float32))
    assert fs.intrinsics[0, 2] == K[0, 2] * (4 / 8) and fs.intrinsics[1, 2] == K[1, 2] * (5 / 6) and fs.intrinsics[0, 0] == K[0, 0]


def test_oracle_reproduces_the_fixture(fx):
    lidar = EO.pano_cloud(fx["pano"], fx["payload"], EO.FOV, EO.FOV_HOZ, EO.SCALE)
    T = EO.world_matrix(fx["pose_lidar"], EO.SCALE, EO.OFFSET)
    world = EO.world_affine(lidar, T)
    assert np.array_equal(lidar[:, 3], fx["ref_lidar"][:, 3].astype(np.float64)) and np.array_equal(world[:, 3], fx["ref_world"][:, 3])
    assert EO.distance(lidar, fx["ref_lidar"]) <= fx["e_ref_lidar"] and EO.distance(world, fx["ref_world"]) <= fx["e_ref_world"]
    # the reference's world cloud IS the float64 affine of its own fp32 cloud (np.ones promotes): a few float64 roundings at 24 m
    assert EO.distance(EO.world_affine(fx["ref_lidar"], T), fx["ref_world"]) <= 1e-12
    assert np.array_equal(EO.quantize(fx["q_in"]), fx["q_u8"])
    assert np.abs(EO.linear_to_srgb(fx["srgb_in"]) - fx["srgb_ref"]).max() <= fx["e_ref_srgb"]
    off = np.ones(fx["srgb_in"].size, bool)
    off[fx["srgb_boundary"]] = False
    assert np.array_equal(np.trunc(EO.linear_to_srgb(fx["srgb_in"]).reshape(-1) * 255.0).astype(np.uint8)[off], fx["srgb_u8"].reshape(-1)[off])
    special = np.array([np.nan, -0.0, -1e-3, -1.0, -np.inf, 1.0, 256 / 255, 1.01, np.inf, 1e30], np.float32)
    assert EO.quantize(special).tolist() == [0, 0, 0, 0, 0, 255, 255, 255, 255, 255]
    # which pixels the oracle keeps: numpy's `!= 0.0` (-0.0 dropped; NaN, negative, infinite and denormal ranges kept)
    r = np.array([[0.0, -0.0, np.nan, -1.0], [1.0, 0.0, np.inf, 1e-45]], np.float32)
    assert EO.kept(r).tolist() == [2, 3, 4, 6, 7] == np.flatnonzero(r.reshape(-1) != 0.0).tolist()
    c = EO.pano_cloud(r, None, EO.FOV, EO.FOV_HOZ, EO.SCALE)
    assert c.shape == (5, 4) and not c[:, 3].any() and np.isnan(c[0, :3]).all() and np.isfinite(c[1, :3]).all()


def test_file_writers(fx, tmp_path):
    from PIL import Image
    from nvsf.nerf import export as X
    rng = np.random.default_rng(5)
    H, W, Hl, Wl = 6, 8, 4, 10
    planes = [rng.integers(0, 256, (Hl, Wl), dtype=np.uint8) for _ in range(3)]
    rgb, rgb_depth = rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H, W), dtype=np.uint8)
    lidar, world = fx["ref_lidar"], fx["ref_world"]
    p = X.write_frame(str(tmp_path), "run", 7, *planes, rgb, rgb_depth, lidar, world)
    assert sorted(os.path.basename(v) for v in p.values()) == sorted(
        ["test_run_0007_pcd_world.txt", "test_run_0007_pcd_lidar.txt", "test_run_0007_pcd_lidar.pcd", "test_run_0007.png", "run_0007_rgb.png",
         "run_0007_rgb_depth.png"])
    assert sorted(os.listdir(str(tmp_path))) == sorted(os.path.basename(v) for v in p.values())
    for key, want in (("pcd_world", world), ("pcd_lidar", lidar)):
        back = np.loadtxt(p[key], ndmin=2)
        assert back.shape == want.shape and np.abs(back - want.astype(np.float64)).max() <= 5e-7 + 1e-12, key
        assert open(p[key]).readline().count(" ") == 3
    lines = open(p["pcd"]).read().splitlines()
    head = dict(l.split(" ", 1) for l in lines[1:11])
    assert lines[0].startswith("# .PCD v0.7") and head["VERSION"] == "0.7" and head["FIELDS"] == "x y z intensity" and head["DATA"] == "ascii"
    assert int(head["POINTS"]) == int(head["WIDTH"]) == len(lines) - 11 == lidar.shape[0] and head["HEIGHT"] == "1"
    assert np.abs(np.loadtxt(lines[11:], ndmin=2) - lidar).max() <= 5e-7 + 1e-12
    stack = np.asarray(Image.open(p["lidar_png"]))
    assert stack.shape == (3 * Hl, Wl) and np.array_equal(stack, np.concatenate(planes, 0))  # ray-drop mask, intensity, range; greyscale
    assert np.array_equal(np.asarray(Image.open(p["rgb"])), rgb) and np.array_equal(np.asarray(Image.open(p["rgb_depth"])), rgb_depth)
    X.write_pcd(p["pcd"], np.zeros((0, 4), np.float32))  # an empty cloud is a valid file
    assert open(p["pcd"]).read().splitlines()[-2:] == ["POINTS 0", "DATA ascii"]
    X.write_cloud_txt(p["pcd_world"], np.zeros((0, 4)))
    assert os.path.getsize(p["pcd_world"]) == 0


def test_export_refuses_host_tensors(hip_lib):
    from nvsf import _hip
    from nvsf.nerf import export as X
    # the Python constant and formula are the library's own: a changed kernel tile cannot leave them behind
    P = X.PIXELS_PER_WORKGROUP
    for H, W in ((1, 1), (1, P - 1), (1, P), (1, P + 1), (66, 1030), (129, 2048), (4096, 4096)):
        assert X.library_sizes(H, W) == (X.workspace_bytes(H * W), P), (H, W)
    assert X.workspace_bytes(1) == 4 and X.workspace_bytes(P) == 4 and X.workspace_bytes(P + 1) == 8
    for H, W in ((0, 4), (4, 0), (4097, 4096)):
        with pytest.raises(_hip.NvsfHipError):
            X.library_sizes(H, W)
    with pytest.raises(ValueError, match="CPU tensor"):
        X.pano_to_cloud(torch.zeros(4, 8), None, None, 0.01, (0, 0, 0), (2.0, 26.9))
    with pytest.raises(ValueError, match="torch tensor"):
        X.pano_to_cloud(np.zeros((4, 8), np.float32), None, None, 0.01, (0, 0, 0), (2.0, 26.9))
    with pytest.raises(ValueError, match="CPU tensor"):
        X.quantize_u8(torch.zeros(4))
    T = X.world_matrix(torch.eye(4), 0.01, (1.5, -2.0, 0.25))
    assert T.dtype == np.float32 and T[:3, 3].tolist() == [1.5, -2.0, 0.25]
    pose = torch.eye(4)
    pose[:3, 3] = torch.tensor([0.1, 0.2, 0.3])
    keep = pose.clone()
    X.world_matrix(pose, 0.01, (1.5, -2.0, 0.25))
    assert torch.equal(pose, keep)  # a copy: the batch's pose is not rescaled (the reference's is)
