"""CPU tests of the object masks (no GPU): the conditions the fixture of tests/golden/golden_object_masks.py must meet, numpy
restatements of the four device entries (tests/object_masks_oracle.py) that reproduce the reference's masks and images bit for bit,
hull_planes against scipy's ConvexHull, the host halves of compute_object_masks / compute_object_masks_img, the JSON sidecar, FrameSet's
annotations, the report lines, and the refusal of CPU tensors."""
import json
import os

import numpy as np
import pytest
import torch

import object_masks_oracle as OM
from depth_image_oracle import range_cloud


@pytest.fixture(scope="module")
def fx():
    return OM.fixture()


@pytest.fixture(scope="module")
def inp():
    return OM.inputs()


def _frame_data(inp, fx, f):
    return {"poses_lidar": torch.from_numpy(inp["poses_lidar"][f:f + 1].copy()), "pose": torch.from_numpy(inp["poses"][f:f + 1].copy()),
            "3d_annotation": OM.annotations(fx), "H": inp["H"], "W": inp["W"], "intrinsic_cam": inp["K"]}


def test_fixture_pins_numpy2_promotion(fx):
    assert type(1.5 - np.float32(1)) is np.float32  # a Python float beside an fp32 scalar: fp32 (NEP 50), what the fixture was made under
    assert int(str(fx["numpy_version"]).split(".")[0]) >= 2
    assert fx["box_vertices"].shape == (10, 8, 3) and fx["raw_cloud"].shape == (4096, 4) and fx["raw_cloud"].dtype == np.float32


@pytest.mark.parametrize("f", [0, 1])
def test_range_image_masks_conditions_and_restatement(fx, inp, f):
    from nvsf.nerf import object_masks as LIB
    Hl, Wl, fov, fov_hoz = inp["Hl"], inp["Wl"], inp["fov"], inp["fov_hoz"]
    data = _frame_data(inp, fx, f)
    before = data["poses_lidar"].clone()
    hulls = LIB.lidar_frame_hulls(data, OM.SCALE, OM.OFFSET)
    assert torch.equal(data["poses_lidar"], before)  # the pose is copied, not edited in place
    assert len(hulls) == 10 and all(h.shape == (6, 4) for h in hulls)
    depth_m = inp["depth"][f] / OM.SCALE
    assert depth_m.dtype == np.float32
    pc = range_cloud(depth_m, fov, fov_hoz)
    assert pc.shape[0] == int(fx[f"f{f}_n_points"])
    max_depth = OM.LIDAR_MAX_DEPTH_M * OM.SCALE / OM.SCALE
    # conditions
    assert OM.face_margin(pc, hulls) > 1e-6
    margin, _, _ = OM.rounding_margin(pc, Hl, Wl, fov, fov_hoz, max_depth)
    assert margin.min() > OM.EPS_ROUND
    # entry 1 and entry 3, bit for bit
    member = OM.unpack(fx, f"f{f}_member", (pc.shape[0],))
    assert np.array_equal(OM.points_in_hulls(pc, hulls), member) and member.sum() > 1000
    want = OM.unpack(fx, f"f{f}_dyn_pano", (Hl, Wl))
    got = OM.range_image_object_mask(depth_m, hulls, fov, fov_hoz, max_depth)
    assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32)) and want.sum() > 1000
    if f == 0:  # the one point beyond max_depth lies in a box and leaves no pixel
        assert member.sum() == want.sum() + 1


@pytest.mark.parametrize("f", [0, 1])
def test_image_mask_restatement(fx, inp, f):
    from nvsf.nerf import object_masks as LIB
    data = _frame_data(inp, fx, f)
    before = data["pose"].clone()
    boxes = LIB.image_boxes(data, OM.SCALE, OM.OFFSET)
    assert torch.equal(data["pose"], before)
    assert boxes.dtype == np.int32 and boxes.shape == (9, 4)  # the box behind the camera is skipped
    assert boxes[:, 2].max() == inp["W"] - 1 and boxes[:, 3].max() == inp["H"] - 1  # clamped
    want = OM.unpack(fx, f"f{f}_dyn_img", (inp["H"], inp["W"]))
    assert np.array_equal(OM.box_mask_image(boxes, inp["H"], inp["W"]), want) and want.any()
    assert not OM.box_mask_image([[5, 5, 4, 9], [5, 9, 9, 5]], 16, 16).any()  # inverted boxes cover nothing


def test_raw_cloud_restatement_and_borderline_share(fx, inp):
    Hl, Wl, fov, fov_hoz = inp["Hl"], inp["Wl"], inp["fov"], inp["fov_hoz"]
    raw = fx["raw_cloud"]
    excl, n_close = OM.borderline_pixels(raw, Hl, Wl, fov, fov_hoz, OM.LIDAR_MAX_DEPTH_M)
    assert n_close <= 0.01 * raw.shape[0]
    assert np.array_equal(np.nonzero(excl.reshape(-1))[0], fx["raw_excluded"])
    pano, img = OM.lidar_to_pano(raw[:, :3], raw[:, 3], Hl, Wl, fov, fov_hoz, OM.LIDAR_MAX_DEPTH_M)
    want_p, want_i = OM.sparse_image(fx, "raw_pano", (Hl, Wl)), OM.sparse_image(fx, "raw_payload", (Hl, Wl))
    assert np.array_equal(pano.view(np.uint32), want_p.view(np.uint32)) and np.array_equal(img.view(np.uint32), want_i.view(np.uint32))
    r, c = fx["tie_pixel"]
    assert want_i[r, c] == raw[5, 3] and raw[5, 3] != raw[10, 3] and np.array_equal(raw[5, :3], raw[10, :3])  # the lower index keeps the pixel
    dist, rf, cf = OM.pano_coordinates(raw, Hl, Wl, fov, fov_hoz, OM.LIDAR_MAX_DEPTH_M)
    assert dist[20] == 80.0 and dist[21] == 80.0  # exactly at max_depth: dropped ...
    assert not np.isin(want_p, dist[[20, 21]]).any() and want_p[int(np.rint(rf[22])), int(np.rint(cf[22]))] == dist[22]  # ... the next fp32 below: kept
    assert ((rf < -0.5) | (rf >= Hl - 0.5)).sum() > 100  # points outside the vertical field of view


def test_hull_planes_of_boxes():
    from nvsf.nerf import object_masks as LIB
    rng = np.random.default_rng(3)
    for _ in range(5):
        yaw, c = rng.uniform(-3, 3), rng.uniform(-20, 20, 3)
        R = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
        half = rng.uniform(0.3, 4.0, 3)
        corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * half
        v = corners @ R.T + c
        p = LIB.hull_planes(v)
        assert p.shape == (6, 4) and np.allclose(np.linalg.norm(p[:, :3], axis=1), 1.0, atol=1e-14)
        assert (v @ p[:, :3].T + p[:, 3]).max() < 1e-9 and np.all(c @ p[:, :3].T + p[:, 3] < 0)
        # every face is `half` away from the centre along a box axis
        assert np.allclose(sorted(-(c @ p[:, :3].T + p[:, 3])), sorted(np.repeat(half, 2)), atol=1e-9)
    with pytest.raises(ValueError):
        LIB.hull_planes(np.zeros((8, 3)))
    with pytest.raises(ValueError):
        LIB.hull_planes(np.array([[x, y, 0.0] for x in (0, 1) for y in (0, 1)] * 2))  # coplanar
    planes, counts = LIB.pack_planes([LIB.hull_planes(v)] * 3)
    assert planes.shape == (3, 12, 4) and planes.dtype == np.float64 and counts.tolist() == [6, 6, 6] and not planes[:, 6:].any()
    with pytest.raises(ValueError, match="768"):
        LIB.pack_planes([LIB.hull_planes(v)] * 65)


def test_hull_planes_against_scipy():
    spatial = pytest.importorskip("scipy.spatial")
    from nvsf.nerf import object_masks as LIB
    rng = np.random.default_rng(4)
    for case in range(8):
        v = rng.normal(size=(8, 3)) * rng.uniform(0.5, 5.0) + rng.uniform(-10, 10, 3)  # eight points in general position: a triangulated hull
        if case >= 4:  # a sheared box: quadrilateral faces, which qhull reports as two triangles each
            v = (np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=np.float64) @ rng.normal(size=(3, 3))) + rng.uniform(-5, 5, 3)
        mine = LIB.hull_planes(v)
        eq = spatial.ConvexHull(v).equations  # [n, 4]: unit outward normals and offsets, n.x + d <= 0 inside
        uniq = []
        for e in eq:
            if not any(np.abs(e - u).max() < 1e-7 for u in uniq):
                uniq.append(e)
        assert mine.shape[0] == len(uniq) <= 12
        for e in uniq:
            assert np.abs(mine - e).max(1).min() < 1e-9
        pts = rng.normal(size=(20000, 3)) * 4 + v.mean(0)
        inside = OM.points_in_hulls(pts.astype(np.float32), [mine])
        assert np.array_equal(inside, spatial.Delaunay(v).find_simplex(pts.astype(np.float32)) >= 0) or \
            OM.face_margin(pts.astype(np.float32), [mine]) < 1e-6


def test_annotation_sidecar_and_frameset(tmp_path):
    from test_formats_cpu import make_dataset
    from nvsf.nerf import object_masks as LIB
    from nvsf.nerf.dataset import formats as F
    v = np.arange(24, dtype=np.float64).reshape(8, 3)
    path = os.path.join(str(tmp_path), "boxes.json")
    with open(path, "w") as fh:
        json.dump({"1909": [{"class": "car", "vertices": v.tolist()}], "1910": []}, fh)
    ann = LIB.load_annotations(path)
    assert set(ann) == {1909, 1910} and ann[1909][0]["class"] == "car" and np.array_equal(ann[1909][0]["vertices"], v) and ann[1910] == []
    with open(path + ".bad", "w") as fh:
        json.dump({"1": [{"class": "car", "vertices": v[:7].tolist()}]}, fh)
    with pytest.raises(ValueError, match="8 vertices"):
        LIB.load_annotations(path + ".bad")
    seq, frames, images, pcs, K = make_dataset(str(tmp_path))
    plain = F.FrameSet(str(tmp_path), seq, "train", 0.01, device="cpu", training=False)
    assert plain.annotations is None and plain.offset == (0.0, 0.0, 0.0)
    for given in (path, [[], [{"class": "car", "vertices": v}], []]):  # collate needs the device: tests/test_object_masks_gpu.py
        fs = F.FrameSet(str(tmp_path), seq, "train", 0.01, device="cpu", training=False, annotations=given, offset=(1, 2, 3))
        assert fs.offset == (1.0, 2.0, 3.0) and [len(a) for a in fs.annotations] == [0, 1, 0]
        assert fs.annotations[1][0]["class"] == "car" and np.array_equal(fs.annotations[1][0]["vertices"], v)
    with pytest.raises(ValueError, match="entries"):
        F.FrameSet(str(tmp_path), seq, "train", 0.01, device="cpu", training=False, annotations=[[]])


def test_report_lines_and_cpu_refusal(fx, inp):
    from nvsf import _hip
    from nvsf.nerf import meters as M
    from nvsf.nerf import object_masks as LIB
    res = {"chamfer_distance": 1.0, "f_score": 0.5, "depth": [1.0] * 5, "intensity": [2.0] * 5, "raydrop": [3.0] * 3, "rgb_rmse": 0.1, "psnr": 20.0,
           "rgb_ssim": 0.9}
    assert len(M.table_report(res)) == 7
    for s in M.SPLITS:
        res.update({f"chamfer_distance_{s}": 2.0, f"f_score_{s}": 0.25, f"depth_{s}": [1.5] * 5, f"intensity_{s}": [2.5] * 5, f"raydrop_{s}": [3.5] * 3,
                    f"rgb_psnr_{s}": 21.0, f"rgb_ssim_{s}": 0.8})
    lines = M.table_report(res)
    assert len(lines) == 7 + 2 * 6 and lines[7].startswith("[static] Points_error") and lines[-1] == "[dynamic] SSIM = 0.800"
    res.update(rgb_depth_rmse=1.0, rgb_depth_rmse_static=1.25, rgb_depth_rmse_dynamic=1.5)
    assert M.table_report(res)[-1] == "[dynamic] RMSE = 1.500" and len(M.table_report(res)) == 8 + 2 * 7
    data = _frame_data(inp, fx, 0)
    with pytest.raises(_hip.NvsfHipError):
        LIB.compute_object_masks(torch.from_numpy(inp["depth"][0]), data, OM.SCALE, OM.OFFSET, inp["fov"], inp["fov_hoz"], 0.8)
    with pytest.raises(_hip.NvsfHipError):
        LIB.lidar_to_pano(torch.from_numpy(fx["raw_cloud"]), 66, 1030, inp["fov"], inp["fov_hoz"], 80.0)
    with pytest.raises(_hip.NvsfHipError):
        LIB.compute_object_masks_img(data, OM.SCALE, OM.OFFSET)
    with pytest.raises(_hip.NvsfHipError):
        LIB.points_in_hulls(torch.zeros(4, 3), *LIB.pack_planes(LIB.lidar_frame_hulls(data, OM.SCALE, OM.OFFSET)))
