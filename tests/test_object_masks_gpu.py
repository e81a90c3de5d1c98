"""Device-side object masks (csrc/object_masks.hip, nvsf/nerf/object_masks.py) against the fixture the reference's own Python produced
(tests/golden/golden_object_masks.py), and evaluate_frames' static / dynamic tables.

Bounds.  Everything is compared BIT FOR BIT: membership, the dynamic range-image mask, the image mask, the range and payload images of
the raw cloud.  The only pixels left out are, for the raw cloud, those a point within 1e-3 of a rounding boundary of its row or column
can reach (the device's atan2 and the host's differ by ulps; fp32 has ~1e-4 absolute resolution at column 1000): the fixture lists them
and the test asserts that at most 1 % of the points are of that kind.  The re-projected range images keep a margin of 0.4999, so no
pixel of theirs is left out.  The tables of evaluate_frames are compared with the same meters fed by hand at rtol 1e-12 (the same
kernels on the same inputs; the only freedom is the order of host float64 sums)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import object_masks_oracle as OM
from depth_image_oracle import range_cloud

pytestmark = pytest.mark.gpu
INVALID = -1


@pytest.fixture(scope="module")
def fx():
    return OM.fixture()


@pytest.fixture(scope="module")
def inp():
    return OM.inputs()


@pytest.fixture(scope="module")
def frames(fx, inp):
    """Per fixture frame: the collated-frame dict, the LiDAR-frame hulls, the range image in metres and its cloud (host)."""
    from nvsf.nerf import object_masks as LIB
    out = []
    for f in range(2):
        data = {"poses_lidar": torch.from_numpy(inp["poses_lidar"][f:f + 1].copy()), "pose": torch.from_numpy(inp["poses"][f:f + 1].copy()),
                "3d_annotation": OM.annotations(fx), "H": inp["H"], "W": inp["W"], "intrinsic_cam": inp["K"]}
        depth_m = inp["depth"][f] / OM.SCALE
        out.append({"data": data, "hulls": LIB.lidar_frame_hulls(data, OM.SCALE, OM.OFFSET), "depth_m": depth_m,
                    "cloud": range_cloud(depth_m, inp["fov"], inp["fov_hoz"])})
    return out


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


@pytest.mark.parametrize("f", [0, 1])
def test_points_in_hulls_equals_the_reference_membership(dev, fx, frames, f):
    from nvsf.nerf import object_masks as LIB
    planes, counts = LIB.pack_planes(frames[f]["hulls"])
    pc = torch.from_numpy(frames[f]["cloud"]).to(dev)
    want = OM.unpack(fx, f"f{f}_member", (pc.shape[0],))
    got = LIB.points_in_hulls(pc, planes, counts).cpu().numpy()
    assert got.dtype == np.uint8 and set(np.unique(got)) <= {0, 1}
    assert np.array_equal(got.astype(bool), want)
    inside = np.nonzero(want)[0]
    for P in (1, 257, 4097):  # one point, and sizes that are no multiple of the 256-thread workgroup; the window holds members
        start = max(0, int(inside[0]) - P // 2)
        assert np.array_equal(LIB.points_in_hulls(pc[start:start + P], planes, counts).cpu().numpy().astype(bool), want[start:start + P]), P
    assert want[int(inside[0])] and bool(LIB.points_in_hulls(pc[int(inside[0]):int(inside[0]) + 1], planes, counts)[0])
    assert LIB.points_in_hulls(pc[:0], planes, counts).shape == (0,)                                      # P = 0
    assert not LIB.points_in_hulls(pc[:1000], np.zeros((0, 12, 4)), np.zeros(0, np.uint32)).any()         # B = 0
    counts0 = counts.copy()
    counts0[:] = 0
    assert not LIB.points_in_hulls(pc, planes, counts0).any()                                             # boxes without planes hold nothing


def test_lidar_to_pano_raw_cloud(dev, fx, inp):
    from nvsf.nerf import object_masks as LIB
    Hl, Wl, fov, fov_hoz = inp["Hl"], inp["Wl"], inp["fov"], inp["fov_hoz"]
    raw = torch.from_numpy(fx["raw_cloud"]).to(dev)
    excl = np.zeros(Hl * Wl, bool)
    excl[fx["raw_excluded"]] = True
    _, n_close = OM.borderline_pixels(fx["raw_cloud"], Hl, Wl, fov, fov_hoz, OM.LIDAR_MAX_DEPTH_M)
    assert n_close <= 0.01 * raw.shape[0] and excl.sum() <= 4 * n_close
    want_p, want_i = OM.sparse_image(fx, "raw_pano", (Hl, Wl)), OM.sparse_image(fx, "raw_payload", (Hl, Wl))
    pano, img = LIB.lidar_to_pano(raw, Hl, Wl, fov, fov_hoz, OM.LIDAR_MAX_DEPTH_M)
    assert pano.shape == img.shape == (Hl, Wl) and pano.dtype == img.dtype == torch.float32
    keep = ~excl
    print(f"raw cloud: {int((_bits(pano).reshape(-1) != want_p.view(np.uint32).reshape(-1)).sum())} range pixels differ in all, "
          f"{int(excl.sum())} excluded")
    assert np.array_equal(_bits(pano).reshape(-1)[keep], want_p.view(np.uint32).reshape(-1)[keep])
    assert np.array_equal(_bits(img).reshape(-1)[keep], want_i.view(np.uint32).reshape(-1)[keep])
    r, c = (int(v) for v in fx["tie_pixel"])  # two points at bit-equal range: the lower index keeps the pixel
    assert not excl[r * Wl + c] and float(img[r, c]) == float(fx["raw_cloud"][5, 3]) != float(fx["raw_cloud"][10, 3])
    flipped = raw.clone()  # the winner's payload follows the index, not the arrival order
    flipped[5, 3], flipped[10, 3] = raw[10, 3], raw[5, 3]
    assert float(LIB.lidar_to_pano(flipped, Hl, Wl, fov, fov_hoz, OM.LIDAR_MAX_DEPTH_M)[1][r, c]) == float(fx["raw_cloud"][10, 3])
    pano2, img2 = LIB.lidar_to_pano(raw, Hl, Wl, fov, fov_hoz, OM.LIDAR_MAX_DEPTH_M)
    assert np.array_equal(_bits(pano2), _bits(pano)) and np.array_equal(_bits(img2), _bits(img))  # two runs, the same bits
    # three columns: zero intensities; the range view in the data set's layout
    p3, i3 = LIB.lidar_to_pano(raw[:, :3].contiguous(), Hl, Wl, fov, fov_hoz, OM.LIDAR_MAX_DEPTH_M)
    assert np.array_equal(_bits(p3), _bits(pano)) and not i3.any()
    rv = LIB.range_view(raw, Hl, Wl, fov, fov_hoz, OM.LIDAR_MAX_DEPTH_M)
    assert rv.shape == (Hl, Wl, 3) and not rv[..., 0].any() and torch.equal(rv[..., 1], img) and torch.equal(rv[..., 2], pano)
    # every point dropped: beyond the range, outside the vertical field of view, at distance 0; and no point at all
    gone = torch.tensor([[90.0, 0, 0, 1], [0, 80.0, 0, 1], [1.0, 0, 5.0, 1], [1.0, 0, -5.0, 1], [0, 0, 0, 1]], device=dev)
    for cloud in (gone, gone[:0]):
        p0, i0 = LIB.lidar_to_pano(cloud, Hl, Wl, fov, fov_hoz, OM.LIDAR_MAX_DEPTH_M)
        assert not p0.any() and not i0.any()
    # an odd image that is no multiple of the workgroup, against the numpy restatement (same exclusion rule)
    H2, W2 = 13, 37
    e2, _ = OM.borderline_pixels(fx["raw_cloud"], H2, W2, fov, fov_hoz, OM.LIDAR_MAX_DEPTH_M)
    wp, wi = OM.lidar_to_pano(fx["raw_cloud"][:, :3], fx["raw_cloud"][:, 3], H2, W2, fov, fov_hoz, OM.LIDAR_MAX_DEPTH_M)
    gp, gi = LIB.lidar_to_pano(raw, H2, W2, fov, fov_hoz, OM.LIDAR_MAX_DEPTH_M)
    assert np.array_equal(_bits(gp)[~e2], wp.view(np.uint32)[~e2]) and np.array_equal(_bits(gi)[~e2], wi.view(np.uint32)[~e2]) and e2.mean() < 0.2


@pytest.mark.parametrize("f", [0, 1])
def test_range_image_object_mask(dev, fx, inp, frames, f):
    from nvsf.nerf import object_masks as LIB
    Hl, Wl, fov, fov_hoz = inp["Hl"], inp["Wl"], inp["fov"], inp["fov_hoz"]
    fr = frames[f]
    want = OM.unpack(fx, f"f{f}_dyn_pano", (Hl, Wl)).astype(np.float32)
    depth = torch.from_numpy(inp["depth"][f]).to(dev)
    lidar_max_depth = OM.LIDAR_MAX_DEPTH_M * OM.SCALE
    static, dyn = LIB.compute_object_masks(depth, fr["data"], OM.SCALE, OM.OFFSET, fov, fov_hoz, lidar_max_depth)
    assert dyn.shape == static.shape == (Hl, Wl) and dyn.dtype == static.dtype == torch.float32
    assert np.array_equal(_bits(dyn), want.view(np.uint32))  # every pixel, no exclusion
    assert torch.equal(static, (dyn == 0).float()) and float(static.sum() + dyn.sum()) == Hl * Wl
    assert torch.equal(fr["data"]["poses_lidar"], torch.from_numpy(inp["poses_lidar"][f:f + 1]))  # the pose was not edited
    # the fused entry = the z-buffer over the cloud with the membership as payload, bit for bit
    planes, counts = LIB.pack_planes(fr["hulls"])
    pc = torch.from_numpy(fr["cloud"]).to(dev)
    member = LIB.points_in_hulls(pc, planes, counts)
    max_depth = lidar_max_depth / OM.SCALE
    _, composed = LIB.lidar_to_pano(torch.cat([pc, member.float()[:, None]], 1), Hl, Wl, fov, fov_hoz, max_depth)
    assert np.array_equal(_bits(composed), _bits(dyn))
    # no annotation: ones / zeros
    s0, d0 = LIB.compute_object_masks(depth, dict(fr["data"], **{"3d_annotation": []}), OM.SCALE, OM.OFFSET, fov, fov_hoz, lidar_max_depth)
    assert bool((s0 == 1).all()) and not d0.any()


@pytest.mark.parametrize("f", [0, 1])
def test_box_mask_image(dev, fx, inp, frames, f):
    from nvsf.nerf import object_masks as LIB
    H, W = inp["H"], inp["W"]
    want = OM.unpack(fx, f"f{f}_dyn_img", (H, W))
    data = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in frames[f]["data"].items()}
    static, dyn = LIB.compute_object_masks_img(data, OM.SCALE, OM.OFFSET)
    assert dyn.is_cuda and dyn.dtype == torch.float32 and np.array_equal(dyn.cpu().numpy() == 1.0, want) and torch.equal(static, 1 - dyn)
    # an inverted box and a box the clamps turned inside out cover nothing; B = 0; more boxes than one LDS pass holds
    none = LIB.box_mask_image(np.array([[9, 3, 4, 8], [3, 9, 8, 4], [W + 5, 0, W - 1, 9], [0, H + 2, 7, H - 1]], np.int32), H, W, dev)
    assert none.dtype == torch.uint8 and not none.any() and not LIB.box_mask_image(np.zeros((0, 4), np.int32), H, W, dev).any()
    rng = np.random.default_rng(5)
    many = np.stack([rng.integers(0, 37, 1500), rng.integers(0, 13, 1500), rng.integers(0, 37, 1500), rng.integers(0, 13, 1500)], 1).astype(np.int32)
    many[:1400, 2] = many[:1400, 0] - 1  # only the boxes of the second pass cover anything
    assert np.array_equal(LIB.box_mask_image(many, 13, 37, dev).cpu().numpy().astype(bool), OM.box_mask_image(many, 13, 37))
    assert OM.box_mask_image(many, 13, 37).any() and not OM.box_mask_image(many, 13, 37).all()


def test_invalid_arguments_leave_everything_untouched(dev, hip_lib, fx, inp, frames):
    from nvsf.nerf import object_masks as LIB
    Hl, Wl = inp["Hl"], inp["Wl"]
    stream = torch.cuda.current_stream().cuda_stream
    P = lambda t: t.data_ptr()
    geom = (ctypes.c_double * 5)(2.0, 26.9, 180.0, 360.0, 80.0)
    bad_geom = (ctypes.c_double * 5)(2.0, 0.0, 180.0, 360.0, 80.0)
    planes, counts = LIB.pack_planes(frames[0]["hulls"])
    dp = torch.from_numpy(planes).to(dev)
    dc = torch.from_numpy(counts.view(np.int32)).to(dev)
    B, K = planes.shape[:2]
    pts = torch.from_numpy(fx["raw_cloud"][:, :3].copy()).to(dev)
    pay = torch.from_numpy(fx["raw_cloud"][:, 3].copy()).to(dev)
    n = pts.shape[0]
    ws = torch.full((Hl * Wl,), -7, dtype=torch.int64, device=dev)
    ws_bytes = ws.numel() * 8
    pano = torch.full((Hl, Wl), -7.0, device=dev)
    img = torch.full((Hl, Wl), -7.0, device=dev)
    mask = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    rng_img = torch.from_numpy(frames[0]["depth_m"]).to(dev)
    boxes = torch.tensor([[0, 0, 5, 5]], dtype=torch.int32, device=dev)
    bmask = torch.full((13, 37), 7, dtype=torch.uint8, device=dev)
    hulls, pano_, mask_, box_ = hip_lib.nvsf_points_in_hulls, hip_lib.nvsf_lidar_to_pano, hip_lib.nvsf_range_image_object_mask, hip_lib.nvsf_box_mask_image
    assert hulls(None, n, P(dp), P(dc), B, K, P(mask), stream) == INVALID          # null points with P > 0
    assert hulls(P(pts), n, P(dp), P(dc), B, K, None, stream) == INVALID
    assert hulls(P(pts), n, None, P(dc), B, K, P(mask), stream) == INVALID
    assert hulls(P(pts), n, P(dp), P(dc), 65, 12, P(mask), stream) == INVALID     # B KMAX = 780 > 768
    assert hulls(P(pts), n, P(dp), P(dc), 1, 769, P(mask), stream) == INVALID
    assert hulls(P(pts), n, P(dp), P(dc), B, 0, P(mask), stream) == INVALID
    assert pano_(None, P(pay), n, Hl, Wl, geom, P(ws), ws_bytes, P(pano), P(img), stream) == INVALID
    assert pano_(P(pts), None, n, Hl, Wl, geom, P(ws), ws_bytes, P(pano), P(img), stream) == INVALID   # a payload image without a payload
    assert pano_(P(pts), P(pay), n, Hl, Wl, geom, P(ws), ws_bytes - 8, P(pano), P(img), stream) == INVALID  # short workspace
    assert pano_(P(pts), P(pay), n, Hl, Wl, geom, None, ws_bytes, P(pano), P(img), stream) == INVALID
    assert pano_(P(pts), P(pay), n, 0, Wl, geom, P(ws), ws_bytes, P(pano), P(img), stream) == INVALID       # H W = 0
    assert pano_(P(pts), P(pay), n, Hl, 0, geom, P(ws), ws_bytes, P(pano), P(img), stream) == INVALID
    assert pano_(P(pts), P(pay), n, Hl, Wl, bad_geom, P(ws), ws_bytes, P(pano), P(img), stream) == INVALID  # fov = 0
    assert pano_(P(pts), P(pay), n, Hl, Wl, None, P(ws), ws_bytes, P(pano), P(img), stream) == INVALID
    assert pano_(P(pts), P(pay), n, Hl, Wl, geom, P(ws), ws_bytes, None, P(img), stream) == INVALID
    assert mask_(None, Hl, Wl, geom, P(dp), P(dc), B, K, P(ws), ws_bytes, P(pano), stream) == INVALID
    assert mask_(P(rng_img), Hl, Wl, geom, P(dp), P(dc), B, K, P(ws), ws_bytes - 1, P(pano), stream) == INVALID
    assert mask_(P(rng_img), Hl, Wl, geom, P(dp), P(dc), 65, 12, P(ws), ws_bytes, P(pano), stream) == INVALID
    assert mask_(P(rng_img), Hl, Wl, geom, None, P(dc), B, K, P(ws), ws_bytes, P(pano), stream) == INVALID
    assert mask_(P(rng_img), 0, Wl, geom, P(dp), P(dc), B, K, P(ws), ws_bytes, P(pano), stream) == INVALID
    assert mask_(P(rng_img), Hl, Wl, bad_geom, P(dp), P(dc), B, K, P(ws), ws_bytes, P(pano), stream) == INVALID
    assert mask_(P(rng_img), Hl, Wl, geom, P(dp), P(dc), B, K, P(ws), ws_bytes, None, stream) == INVALID
    assert box_(None, 1, 13, 37, P(bmask), stream) == INVALID
    assert box_(P(boxes), 1, 0, 37, P(bmask), stream) == INVALID and box_(P(boxes), 1, 13, 0, P(bmask), stream) == INVALID
    assert box_(P(boxes), 1, 13, 37, None, stream) == INVALID
    torch.cuda.synchronize()
    assert bool((ws == -7).all()) and bool((pano == -7.0).all()) and bool((img == -7.0).all()) and bool((mask == 7).all()) and bool((bmask == 7).all())
    # the valid forms of the same calls run
    assert hulls(P(pts), n, P(dp), P(dc), B, K, P(mask), stream) == 0 and box_(P(boxes), 1, 13, 37, P(bmask), stream) == 0
    assert pano_(P(pts), P(pay), n, Hl, Wl, geom, P(ws), ws_bytes, P(pano), None, stream) == 0
    assert mask_(P(rng_img), Hl, Wl, geom, P(dp), P(dc), B, K, P(ws), ws_bytes, P(img), stream) == 0
    torch.cuda.synchronize()
    assert int(bmask.sum()) == 36 and set(mask.unique().tolist()) <= {0, 1} and bool((pano >= 0).all()) and set(img.unique().tolist()) == {0.0, 1.0}


# ---- evaluate_frames: the static / dynamic tables -------------------------------------------------------------------------------

def _rig_dataset(root, n_frames=2, H=24, W=32, Hl=16, Wl=64, seed=0):
    """A 2-frame data set in the reference's formats whose camera looks along the LiDAR's +x from 30 cm beside it (scene units on
    disk), with ranges of 2-40 m."""
    from nvsf.nerf.dataset import formats as F
    rng = np.random.default_rng(seed)
    seq, scale = "1908", 0.0108
    d = os.path.join(root, "train", seq)
    os.makedirs(d, exist_ok=True)
    frames = []
    for i in range(n_frames):
        l2w = np.eye(4)
        yaw = 0.2 + 0.1 * i
        l2w[:3, :3] = [[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]]
        l2w[:3, 3] = np.array([3.0 + i, -2.0, 1.5]) * scale
        cam = np.eye(4)
        cam[:3, :3] = l2w[:3, :3] @ np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])  # camera z = LiDAR x, x = -y, y = -z
        cam[:3, 3] = l2w[:3, 3] + l2w[:3, :3] @ (np.array([0.0, 0.3, -0.2]) * scale)
        pc = np.zeros((Hl, Wl, 3), np.float32)
        pc[..., 1] = rng.random((Hl, Wl))
        pc[..., 2] = rng.uniform(2.0, 40.0, (Hl, Wl))
        pc[rng.random((Hl, Wl)) < 0.3, 2] = 0.0
        np.save(os.path.join(d, f"img_{i:04d}.npy"), rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8))
        np.save(os.path.join(d, f"pano_{i:04d}.npy"), pc)
        frames.append({"frame_id": 1908 + i, "file_path": f"train/{seq}/img_{i:04d}.npy", "transform_matrix": cam,
                       "lidar_file_path": f"train/{seq}/pano_{i:04d}.npy", "lidar2world": l2w})
    K = np.array([[20.0, 0, 16.0], [0, 20.0, 12.0], [0, 0, 1]])
    F.write_transforms(F.transforms_path(root, seq, "train"), w=W, h=H, w_lidar=Wl, h_lidar=Hl, K=K, frame_start=1908, frame_end=1971,
                       num_frames=64, frames=frames)
    return seq, scale, frames


def _box_in_front(l2w_scene, scale, offset):
    """One yawed box 4-24 m in front of the sensor, in the world frame (metres): about 30 range pixels, two thirds of the camera image."""
    T = np.array(l2w_scene, dtype=np.float64)
    T[:3, 3] = T[:3, 3] / scale + np.asarray(offset)
    yaw = 0.3
    R = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
    corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * [10.0, 4.0, 3.0]
    return (corners @ R.T + [14.0, 1.0, -2.0]) @ T[:3, :3].T + T[:3, 3]


def test_evaluate_frames_static_and_dynamic_tables(dev, tmp_path):
    from nvsf.nerf import meters as M
    from nvsf.nerf import object_masks as LIB
    from nvsf.nerf.dataset import formats as F
    from nvsf.nerf.models.network_static import NeRFNetworkStatic
    from nvsf.nerf.evaluate import PointsMeter, eval_step, evaluate_frames
    seq, scale, frames = _rig_dataset(str(tmp_path))
    offset = (4.0, -3.0, 0.5)
    anns = [[{"class": "car", "vertices": _box_in_front(fr["lidar2world"], scale, offset)}] for fr in frames]
    sidecar = os.path.join(str(tmp_path), "boxes.json")
    with open(sidecar, "w") as fh:
        json.dump({str(fr["frame_id"]): [{"class": "car", "vertices": a[0]["vertices"].tolist()}] for fr, a in zip(frames, anns)}, fh)
    kw = dict(device=dev, training=False, camera_depth=True)
    plain = F.FrameSet(str(tmp_path), seq, "train", scale, **kw)
    fe = F.FrameSet(str(tmp_path), seq, "train", scale, annotations=sidecar, offset=offset, **kw)
    empty = F.FrameSet(str(tmp_path), seq, "train", scale, annotations=[[], []], offset=offset, **kw)
    c = fe.collate([1])
    assert set(c) == set(plain.collate([1])) | {"3d_annotation"} and np.array_equal(c["3d_annotation"][0]["vertices"], anns[1][0]["vertices"])
    torch.manual_seed(1)
    m = NeRFNetworkStatic(bound=2.0, min_near=0.01, min_near_lidar=0.01, lidar_max_depth=0.9).to(dev)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1 and p.numel() > 10000:
                p.normal_(0, 0.3)
    thres = float(eval_step(m, fe.collate([1]), 48)["pred_raydrop"].median())
    old = evaluate_frames(m, plain, 48, raydrop_thres=thres, meters="table")
    # without annotations: exactly today's keys, with or without the table
    assert set(old) == {"loss", "psnr", "depth_rmse_m", "chamfer_distance", "f_score", "frames", "depth", "intensity", "raydrop", "rgb_ssim", "rgb_rmse",
                        "rgb_depth_rmse"}
    assert set(evaluate_frames(m, fe, 48, raydrop_thres=thres)) == {"loss", "psnr", "depth_rmse_m", "chamfer_distance", "f_score", "frames"}
    res = evaluate_frames(m, fe, 48, raydrop_thres=thres, meters="table")
    new = {f"{k}_{s}" for s in ("static", "dynamic") for k in ("depth", "intensity", "raydrop", "chamfer_distance", "f_score", "rgb_psnr", "rgb_ssim",
                                                               "rgb_depth_rmse")}
    assert set(res) == set(old) | new
    for k in old:  # the unsplit table is computed as before
        np.testing.assert_array_equal(np.asarray(res[k], np.float64), np.asarray(old[k], np.float64), err_msg=k)
    # the same meters fed by hand with host-built masks (numpy restatements of the device entries)
    near = lambda a, b, k: np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=1e-12, atol=0, equal_nan=True, err_msg=k)
    hand = {s: M.split_table_meters(scale, 1, thres, True) for s in M.SPLITS}
    pts = {s: PointsMeter(scale, fe.intrinsics_lidar, fe.intrinsics_hoz_lidar) for s in M.SPLITS}
    n_dyn = []
    for i in range(2):
        data = fe.collate([i])
        e = eval_step(m, data, 48, raydrop_thres=thres)
        hulls = LIB.lidar_frame_hulls(data, scale, offset)
        host = {}
        for key in ("pred_depth", "gt_depth"):
            range_m = e[key][0].cpu().numpy() / scale
            assert range_m.dtype == np.float32
            assert OM.face_margin(range_cloud(range_m, fe.intrinsics_lidar, fe.intrinsics_hoz_lidar), hulls) > 1e-6
            host[key] = OM.range_image_object_mask(range_m, hulls, fe.intrinsics_lidar, fe.intrinsics_hoz_lidar, m.lidar_max_depth / scale)
        img = OM.box_mask_image(LIB.image_boxes(data, scale, offset), fe.H, fe.W).astype(np.float32)
        n_dyn.append((int(host["pred_depth"].sum()), int(host["gt_depth"].sum()), int(img.sum())))
        for s in M.SPLITS:
            pick = (lambda a: a) if s == "dynamic" else (lambda a: (a == 0).astype(np.float32))
            mp, mg, mi = (torch.from_numpy(pick(a)).to(dev)[None] for a in (host["pred_depth"], host["gt_depth"], img))
            M.update_table(hand[s], e, scale, masks=(mp, mg, mi))
            pts[s].update(e["pred_depth"] * mp, e["gt_depth"] * mg)
    print("dynamic pixels per frame (prediction, ground truth, image):", n_dyn)
    assert all(g > 20 and 0 < im < fe.H * fe.W for _, g, im in n_dyn)
    for s in M.SPLITS:
        near(res[f"depth_{s}"], hand[s]["depth"].frame_values().mean(0), f"depth_{s}")
        near(res[f"intensity_{s}"], hand[s]["intensity"].frame_values().mean(0), f"intensity_{s}")
        near(res[f"raydrop_{s}"], hand[s]["raydrop"].frame_values().mean(0), f"raydrop_{s}")
        near([res[f"chamfer_distance_{s}"], res[f"f_score_{s}"]], np.array(pts[s].V).mean(0), f"points_{s}")
        near(res[f"rgb_psnr_{s}"], hand[s]["psnr"].frame_values().mean(), f"rgb_psnr_{s}")
        near(res[f"rgb_ssim_{s}"], hand[s]["ssim"].frame_values().mean(), f"rgb_ssim_{s}")
        near(res[f"rgb_depth_rmse_{s}"], hand[s]["rgb_depth"].frame_values().mean(), f"rgb_depth_rmse_{s}")
    assert res["depth_static"][0] != res["depth"][0] and res["rgb_psnr_static"] != res["rgb_psnr_dynamic"]
    # the reference's per-rank-frames scheme gives the same table
    by_frames = evaluate_frames(m, fe, 48, raydrop_thres=thres, meters="table", shard="frames")
    assert by_frames.keys() == res.keys()
    for k in res:
        near(by_frames[k], res[k], k)
    # an empty box list: the static table is the unsplit one, the dynamic one sees zeros
    none = evaluate_frames(m, empty, 48, raydrop_thres=thres, meters="table")
    assert set(none) == set(res)
    for k in ("depth", "intensity", "raydrop", "chamfer_distance", "f_score", "rgb_ssim", "rgb_depth_rmse"):
        near(none[f"{k}_static"], old[k], k)
    assert none["rgb_psnr_static"] == pytest.approx(old["psnr"], rel=1e-6)  # the device PSNR meter against the host path's
    assert none["depth_dynamic"][0] == 0.0 and none["f_score_dynamic"] == 0.0 and np.isnan(none["chamfer_distance_dynamic"])
    lines = M.table_report(res)
    assert len(lines) == 8 + 2 * 7 and lines[8].startswith("[static] Points_error") and lines[-1].startswith("[dynamic] RMSE = ")
    assert len(M.table_report(old)) == 8
