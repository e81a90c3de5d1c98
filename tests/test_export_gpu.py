"""Device-side prediction export (csrc/export.hip, nvsf/nerf/export.py), test_step and the sensor change on the device, against the
fixture the reference's own Python produced (tests/golden/golden_export.py) and the float64 oracle of tests/export_oracle.py.

Bounds.
  * count, the payload column and the row <-> pixel correspondence: exact.
  * LiDAR-frame xyz against the float64 oracle: 4 x e_ref_lidar, e_ref_lidar = the reference's own largest distance from that oracle on
    the fixture's crop (ranges up to RANGE_M metres) -- the project's margin for "the reference's own distance from fp64".  The seeded
    shapes keep their ranges inside RANGE_M, so the same figure holds; the 66 x 1030 street frame reaches farther and fp32 error grows
    with the coordinate, so its bar is scaled by max range / RANGE_M.
  * world against the float64 affine of the device's OWN LiDAR cloud: 1e-9 m (a few float64 operations on coordinates below 1e5 m,
    2^-53 x 1e5 x a handful); world against the fixture: 4 x e_ref_world.
  * quantize_u8: bit-equal to the fixture; the sRGB floats within 4 x e_ref_srgb of float64; the sRGB uint8 equal off the fixture's list of
    values within 1e-3 of an integer.
  * test_step against eval_step, masks, two runs: bit for bit."""
import os

import numpy as np
import pytest
import torch

import export_oracle as EO
import object_masks_oracle as OM

pytestmark = pytest.mark.gpu
INVALID = -1
CANARY_F32, CANARY_F64 = -12345.5, -54321.25


@pytest.fixture(scope="module")
def fx():
    return EO.fixture()


def _pose(fx):
    return torch.from_numpy(fx["pose_lidar"].copy())


def _cloud(dev, r, payload, pose=None, **kw):
    from nvsf.nerf import export as X
    p = None if payload is None else torch.from_numpy(np.ascontiguousarray(payload)).to(dev)
    lidar, world = X.pano_to_cloud(torch.from_numpy(np.ascontiguousarray(r)).to(dev), p, pose, EO.SCALE, EO.OFFSET, EO.FOV, EO.FOV_HOZ, **kw)
    return lidar.cpu().numpy(), (None if world is None else world.cpu().numpy())


def _raw(dev, r, payload, T, capacity, H=None, W=None, ws_bytes=None, geom=None):
    """nvsf_pano_to_cloud called directly on buffers filled with canaries -> (status, count, cloud_lidar, cloud_world) with ALL rows."""
    from nvsf import _hip
    from nvsf.nerf import export as X
    lib = _hip.load()
    rt = torch.from_numpy(np.ascontiguousarray(r, dtype=np.float32)).to(dev)
    H, W = (rt.shape if H is None else (H, W))
    pt = None if payload is None else torch.from_numpy(np.ascontiguousarray(payload, dtype=np.float32)).to(dev)
    rows = max(capacity, 1) + 8
    lidar = torch.full((rows, 4), CANARY_F32, dtype=torch.float32, device=dev)
    world = torch.full((rows, 4), CANARY_F64, dtype=torch.float64, device=dev) if T is not None else None
    count = torch.full((1,), 0x7eadbeef, dtype=torch.int32, device=dev)
    ws = torch.zeros(X.workspace_bytes(int(H) * int(W)) // 4 + 1, dtype=torch.int32, device=dev)
    g = _hip.host_f64(geom if geom is not None else [EO.FOV[0], EO.FOV[1], EO.FOV_HOZ[1], EO.SCALE])
    status = lib.nvsf_pano_to_cloud(_hip.ptr(rt), _hip.ptr(pt), int(H), int(W), g, _hip.host_f64(np.asarray(T, np.float64).reshape(-1)) if T is not None else None,
                                    _hip.ptr(ws), (ws.numel() - 1) * 4 if ws_bytes is None else ws_bytes, _hip.ptr(lidar), _hip.ptr(world),
                                    capacity, _hip.ptr(count), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return status, int(count.item()), lidar.cpu().numpy(), (None if world is None else world.cpu().numpy())


def _check(dev, r, payload, pose, e_ref, what):
    """One range image against the oracle: count, payload and order exact, xyz within 4 e_ref, world = the affine of the device's own cloud."""
    lidar, world = _cloud(dev, r, payload, pose)
    want = EO.pano_cloud(r, payload, EO.FOV, EO.FOV_HOZ, EO.SCALE)
    idx = EO.kept(r)
    assert lidar.shape == (idx.size, 4) and lidar.dtype == np.float32, (what, lidar.shape, idx.size)
    assert np.array_equal(lidar[:, 3].astype(np.float64), want[:, 3], equal_nan=True), what
    finite = np.isfinite(want[:, :3]).all(1)
    assert np.array_equal(np.isnan(lidar[:, :3]).any(1), np.isnan(want[:, :3]).any(1)), what
    d = EO.distance(lidar[finite], want[finite])
    print(f"{what}: {idx.size} points, lidar distance {d:.3e} m (bar {4 * e_ref:.3e})")
    assert d <= 4 * e_ref, (what, d)
    if pose is not None:
        T = EO.world_matrix(pose.numpy(), EO.SCALE, EO.OFFSET)
        assert world.shape == lidar.shape and world.dtype == np.float64
        assert np.array_equal(world[:, 3], lidar[:, 3].astype(np.float64), equal_nan=True)
        dw = EO.distance(world[finite], EO.world_affine(lidar, T)[finite])
        assert dw <= 1e-9, (what, dw)
    return lidar, world


RANGE_M = 12.0  # the fixture's crop and the seeded shapes keep their ranges below this many metres


def test_fixture_cloud(dev, fx):
    r, payload, pose = fx["pano"], fx["payload"], _pose(fx)
    assert float(r.max()) / EO.SCALE <= RANGE_M
    lidar, world = _check(dev, r, payload, pose, float(fx["e_ref_lidar"]), "fixture crop")
    assert lidar.shape[0] == fx["ref_lidar"].shape[0]                                   # count: exact
    assert np.array_equal(lidar[:, 3], fx["ref_lidar"][:, 3])                           # the intensity column: exact
    assert np.array_equal(world[:, 3], fx["ref_world"][:, 3])
    pix = np.arange(r.size, dtype=np.float32).reshape(r.shape)                          # row k <-> the k-th kept pixel
    by_index, _ = _cloud(dev, r, pix, None)
    assert np.array_equal(by_index[:, 3].astype(np.int64), EO.kept(r))
    assert np.array_equal(by_index[:, :3], lidar[:, :3])
    d_ref, d_world = EO.distance(lidar, fx["ref_lidar"]), EO.distance(world, fx["ref_world"])
    print(f"against the reference: lidar {d_ref:.3e} m, world {d_world:.3e} m (e_ref {float(fx['e_ref_lidar']):.3e}, {float(fx['e_ref_world']):.3e})")
    assert d_world <= 4 * float(fx["e_ref_world"])
    assert torch.equal(pose, _pose(fx))                                                 # the pose given is not rescaled


def _pattern(H, W, kind, seed):
    r, payload = EO.seeded_range_image(H, W, seed, range_m=(2.0, RANGE_M - 0.01))  # every kept pixel its own range, inside the crop's span
    assert float(r.max()) / EO.SCALE <= RANGE_M
    flat = r.reshape(-1)
    if kind == "kept":
        flat[flat == 0] = np.float32(0.05)
    elif kind == "dropped":
        flat[:] = 0.0
    elif kind == "last":
        flat[:] = 0.0
        flat[-1] = np.float32(0.07)
    elif kind == "alternating":
        flat[flat == 0] = np.float32(0.05)
        flat[::2] = 0.0
    else:
        assert kind == "seeded"
    return r, payload


def _shapes():
    from nvsf.nerf.export import PIXELS_PER_WORKGROUP as P
    return [(1, 1, "kept"), (1, 1, "dropped"), (3, 63, "seeded"), (3, 64, "seeded"), (3, 65, "seeded"), (1, P - 1, "seeded"), (1, P, "seeded"),
            (1, P + 1, "seeded"), (1, P + 1, "last"), (128, 2048, "seeded"),   # 256 workgroups: one full round of the scan stage
            (129, 2048, "seeded"),                                             # 258: a second round with a carry
            (5, 300, "dropped"), (5, 300, "kept"), (7, 333, "last"), (9, 257, "alternating"), (2, 3 * P, "alternating")]


@pytest.mark.parametrize("case", range(16))
def test_compaction_shapes(dev, fx, case):
    from nvsf.nerf.export import PIXELS_PER_WORKGROUP as P
    assert len(_shapes()) == 16 and 128 * 2048 == 256 * P and 129 * 2048 > 256 * P  # the two large shapes: one full scan round, and a second
    H, W, kind = _shapes()[case]
    r, payload = _pattern(H, W, kind, 100 + case)
    pose = _pose(fx)
    lidar, world = _check(dev, r, payload, pose, float(fx["e_ref_lidar"]), f"{H} x {W} {kind}")
    if kind == "dropped":
        assert lidar.shape[0] == 0 and world.shape[0] == 0
    if kind == "last":
        assert lidar.shape[0] == 1 and lidar[0, 3] == payload.reshape(-1)[-1]


def test_special_ranges(dev, fx):
    """-0.0 is dropped; NaN, negative, infinite and denormal ranges are kept, as np.where(pano != 0.0) keeps them."""
    r = np.zeros((2, 70), np.float32)
    r[0, :8] = [0.0, -0.0, np.nan, -0.25, 0.25, np.inf, 1e-45, -0.0]
    r[1, 60:] = 0.1
    r[1, 65] = -0.0
    payload = np.arange(140, dtype=np.float32).reshape(2, 70)
    lidar, world = _check(dev, r, payload, _pose(fx), float(fx["e_ref_lidar"]), "special ranges")
    assert lidar[:, 3].astype(int).tolist() == [2, 3, 4, 5, 6] + [130 + k for k in range(10) if k != 5]
    assert np.isnan(lidar[0, :3]).all() and np.isnan(world[0, :3]).all()
    assert np.isinf(lidar[3, :3]).any() and np.isfinite(lidar[[1, 2, 4], :3]).all()


def test_canaries_capacity_and_null_arguments(dev, fx):
    r, payload = fx["pano"], fx["payload"]
    T = EO.world_matrix(fx["pose_lidar"], EO.SCALE, EO.OFFSET)
    n = EO.kept(r).size
    st, count, full_l, full_w = _raw(dev, r, payload, T, r.size)
    assert st == 0 and count == n
    assert (full_l[n:] == CANARY_F32).all() and (full_w[n:] == CANARY_F64).all()            # rows at or beyond count: never touched
    # all dropped: count 0 and nothing written
    st, count, l0, w0 = _raw(dev, np.zeros_like(r), payload, T, r.size)
    assert st == 0 and count == 0 and (l0 == CANARY_F32).all() and (w0 == CANARY_F64).all()
    # capacity < count: the total is reported, rows past the capacity keep the canary, the rows before it are those of the full run
    for cap in (0, 1, 1000, n - 1):
        st, count, l1, w1 = _raw(dev, r, payload, T, cap)
        assert st == 0 and count == n, cap
        assert np.array_equal(l1[:cap], full_l[:cap]) and np.array_equal(w1[:cap], full_w[:cap]), cap
        assert (l1[cap:] == CANARY_F32).all() and (w1[cap:] == CANARY_F64).all(), cap
    # payload NULL: column 3 is 0; world NULL: the LiDAR cloud alone, the same bits
    st, count, l2, w2 = _raw(dev, r, None, T, r.size)
    assert st == 0 and count == n and not l2[:n, 3].any() and not w2[:n, 3].any()
    assert np.array_equal(l2[:n, :3], full_l[:n, :3]) and np.array_equal(w2[:n, :3], full_w[:n, :3])
    st, count, l3, w3 = _raw(dev, r, payload, None, r.size)
    assert st == 0 and count == n and w3 is None and np.array_equal(l3, full_l)
    from nvsf.nerf import export as X
    lidar, world = X.pano_to_cloud(torch.from_numpy(r).to(dev), None, None, EO.SCALE, EO.OFFSET, EO.FOV, EO.FOV_HOZ)
    assert world is None and np.array_equal(lidar.cpu().numpy(), l2[:n])
    short, short_w = X.pano_to_cloud(torch.from_numpy(r).to(dev), torch.from_numpy(payload).to(dev), _pose(fx), EO.SCALE, EO.OFFSET, EO.FOV,
                                     EO.FOV_HOZ, capacity=100)
    assert np.array_equal(short.cpu().numpy(), full_l[:100]) and np.array_equal(short_w.cpu().numpy(), full_w[:100])


def test_two_runs_are_bit_identical(dev, fx):
    r, payload = _pattern(128, 2048, "seeded", 7)
    a, aw = _cloud(dev, r, payload, _pose(fx))
    b, bw = _cloud(dev, r, payload, _pose(fx))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(aw.view(np.uint64), bw.view(np.uint64))


def test_rejected_arguments_launch_nothing(dev, fx):
    from nvsf.nerf import export as X
    r, payload = fx["pano"], fx["payload"]
    T = EO.world_matrix(fx["pose_lidar"], EO.SCALE, EO.OFFSET)

    def untouched(res):
        st, count, lidar, world = res
        assert st == INVALID and count == 0x7eadbeef and (lidar == CANARY_F32).all() and (world is None or (world == CANARY_F64).all())
    big = np.zeros((4097, 4096), np.float32)  # H W = 2^24 + 4096: beyond the supported range (the buffers are real all the same)
    big[0, :5] = 0.1
    untouched(_raw(dev, big, None, T, 64))
    st, count, lidar, _ = _raw(dev, big[:4096], None, None, 64)  # exactly 2^24 pixels is inside it
    assert st == 0 and count == 5 and (lidar[5:] == CANARY_F32).all()
    untouched(_raw(dev, r, payload, T, 64, ws_bytes=X.workspace_bytes(r.size) - 4))               # workspace too small
    untouched(_raw(dev, r, payload, T, 64, geom=[EO.FOV[0], 0.0, EO.FOV_HOZ[1], EO.SCALE]))       # fov = 0
    untouched(_raw(dev, r, payload, T, 64, geom=[EO.FOV[0], EO.FOV[1], EO.FOV_HOZ[1], 0.0]))      # scale = 0
    untouched(_raw(dev, r, payload, T, 64, H=0, W=16))
    with pytest.raises(ValueError, match="exceeds"):
        X.pano_to_cloud(torch.zeros(4097, 4096, device=dev), None, None, EO.SCALE, EO.OFFSET, EO.FOV, EO.FOV_HOZ)
    with pytest.raises(ValueError, match="float32"):
        X.pano_to_cloud(torch.zeros(4, 8, device=dev, dtype=torch.float64), None, None, EO.SCALE, EO.OFFSET, EO.FOV, EO.FOV_HOZ)
    with pytest.raises(ValueError, match=r"\[H, W\]"):
        X.pano_to_cloud(torch.zeros(1, 4, 8, device=dev), None, None, EO.SCALE, EO.OFFSET, EO.FOV, EO.FOV_HOZ)
    with pytest.raises(ValueError, match="shape"):
        X.pano_to_cloud(torch.zeros(4, 8, device=dev), torch.zeros(8, 4, device=dev), None, EO.SCALE, EO.OFFSET, EO.FOV, EO.FOV_HOZ)
    with pytest.raises(ValueError, match="CPU tensor"):
        X.pano_to_cloud(torch.zeros(4, 8, device=dev), torch.zeros(4, 8), None, EO.SCALE, EO.OFFSET, EO.FOV, EO.FOV_HOZ)
    with pytest.raises(ValueError, match="positive"):
        X.pano_to_cloud(torch.zeros(4, 8, device=dev), None, None, 0.0, EO.OFFSET, EO.FOV, EO.FOV_HOZ)


def test_street_frame(dev, fx):
    import depth_image_oracle as DO
    dx = DO.fixture()
    r = (dx["range_m"][1] * np.float32(EO.SCALE)).astype(np.float32)
    assert r.shape == (66, 1030)
    payload = np.random.default_rng(9).random(r.shape).astype(np.float32)
    grow = max(1.0, float(dx["range_m"][1].max()) / RANGE_M)  # fp32 error grows with the coordinate: the bar with it
    pose = torch.from_numpy(OM.scene_pose(dx["poses_lidar"][1], EO.SCALE, EO.OFFSET))
    _check(dev, r, payload, pose, float(fx["e_ref_lidar"]) * grow, "street frame 66 x 1030")


# ---- quantisation ------------------------------------------------------------------------------------------------------------------

def test_quantize_u8(dev, fx):
    from nvsf.nerf import export as X
    q = torch.from_numpy(fx["q_in"]).to(dev)
    got = X.quantize_u8(q)
    assert got.dtype == torch.uint8 and got.shape == q.shape and np.array_equal(got.cpu().numpy(), fx["q_u8"])   # bit-equal to numpy's cast
    for n in (1, 255, 256, 257):  # one element, and sizes around the 256-thread workgroup
        assert np.array_equal(X.quantize_u8(q.reshape(-1)[:n].contiguous()).cpu().numpy(), fx["q_u8"].reshape(-1)[:n]), n
    assert X.quantize_u8(q[:0]).shape == (0, q.shape[1])
    x = torch.from_numpy(fx["srgb_in"]).to(dev)
    s = X.linear_to_srgb(x).cpu().numpy()
    want = EO.linear_to_srgb(fx["srgb_in"])
    err = float(np.abs(s.astype(np.float64) - want).max())
    print(f"sRGB floats: distance from float64 {err:.3e} (the reference's {float(fx['e_ref_srgb']):.3e}; bar 4 x)")
    assert s.dtype == np.float32 and err <= 4 * float(fx["e_ref_srgb"])
    u = X.quantize_u8(x, srgb=True).cpu().numpy()
    off = np.ones(x.numel(), bool)
    off[fx["srgb_boundary"]] = False
    assert np.array_equal(u.reshape(-1)[off], fx["srgb_u8"].reshape(-1)[off])
    assert np.abs(u.reshape(-1).astype(int) - fx["srgb_u8"].reshape(-1).astype(int)).max() <= 1
    assert np.array_equal(u, X.quantize_u8(X.linear_to_srgb(x)).cpu().numpy())  # the fused path = the two calls


def test_quantize_u8_saturates_where_numpy_is_undefined(dev):
    from nvsf.nerf import export as X
    special = np.array([np.nan, -0.0, -1e-3, -1.0, -np.inf, 1.0, 256 / 255, 1.01, np.inf, 1e30, 0.5, -0.003], np.float32)
    got = X.quantize_u8(torch.from_numpy(special).to(dev)).cpu().numpy()
    assert got.tolist() == [0, 0, 0, 0, 0, 255, 255, 255, 255, 255, 127, 0] == EO.quantize(special).tolist()
    lin = X.quantize_u8(torch.from_numpy(special).to(dev), srgb=True).cpu().numpy()
    assert lin[0] == 0 and lin[3] == 0 and lin[4] == 0 and lin[8] == 255  # NaN -> 0; negatives take the linear branch; +inf saturates
    x = torch.tensor([1.0, 0.5])  # the reference's fp32 expression on the host: 1.055 * 1 - 0.055 rounds BELOW 1, so white is 254
    ref = (torch.where(x < 0.0031308, 12.92 * x, 1.055 * x ** 0.41666 - 0.055).numpy() * 255).astype(np.uint8)
    assert ref.tolist() == [254, 187] and [int(lin[5]), int(lin[10])] == ref.tolist()


# ---- test_step, the sensor change on the device, export_frames --------------------------------------------------------------------------

def _model(dev, seed=1):
    from nvsf.nerf.models.network_static import NeRFNetworkStatic
    torch.manual_seed(seed)
    m = NeRFNetworkStatic(bound=2.0, min_near=0.01, min_near_lidar=0.01, lidar_max_depth=0.9).to(dev)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1 and p.numel() > 10000:
                p.normal_(0, 0.3)
    return m.eval()


@pytest.fixture(scope="module")
def scene(dev, tmp_path_factory):
    from test_formats_cpu import make_dataset
    root = str(tmp_path_factory.mktemp("export_scene"))
    seq, frames, images, pcs, K = make_dataset(root, n_frames=2, H=6, W=8, Hl=6, Wl=32)
    return {"root": root, "seq": seq, "K": K, "model": _model(dev), "scale": 0.01}


def _frames(scene, dev, **kw):
    from nvsf.nerf.dataset import formats as F
    return F.FrameSet(scene["root"], scene["seq"], "train", scene["scale"], device=dev, training=False, **kw)


def test_test_step_equals_eval_step(dev, scene):
    from nvsf.nerf.evaluate import eval_step, test_step
    m, fe = scene["model"], _frames(scene, dev)
    data = fe.collate([0])
    thres = float(eval_step(m, data, 32)["pred_raydrop"].median())
    e = eval_step(m, data, 32, raydrop_thres=thres)
    out = test_step(m, data, 32, raydrop_thres=thres)
    for got, key in zip(out, ("pred_rgb", "pred_rgb_depth", "pred_raydrop", "pred_intensity", "pred_depth")):
        assert got.shape == e[key].shape and torch.equal(got, e[key]), key
    assert out[0].shape == (1, 6, 8, 3) and out[4].shape == (1, 6, 32)
    gated = int((out[2] <= thres).sum())
    assert 0 < gated < 6 * 32 and not out[4][out[2] <= thres].any()
    # alpha_r = 0: nothing is gated; the gated planes are these times the mask
    raw = test_step(m, data, 32, raydrop_thres=thres, alpha_r=0.0)
    mask = (raw[2] > thres).to(raw[4].dtype)
    assert torch.equal(raw[2], out[2]) and torch.equal(raw[3] * mask, out[3]) and torch.equal(raw[4] * mask, out[4])
    assert raw[4][raw[2] <= thres].ne(0).any()
    # masks_lidar / masks multiply through
    g = torch.Generator().manual_seed(3)
    ml = (torch.rand(1, 6, 32, generator=g) < 0.5).float().to(dev)
    mc = (torch.rand(1, 6, 8, 1, generator=g) < 0.5).float().to(dev)
    masked = test_step(m, dict(data, masks_lidar=ml.reshape(1, -1), masks=mc), 32, raydrop_thres=thres)
    assert torch.equal(masked[0], out[0] * mc) and torch.equal(masked[1], out[1])
    for k in (2, 3, 4):
        assert torch.equal(masked[k], out[k] * ml), k
    # a black background changes the image only
    black = test_step(m, data, 32, raydrop_thres=thres, bg_color=0)
    assert not torch.equal(black[0], out[0]) and torch.equal(black[4], out[4])
    whole = test_step(m, data, 32, raydrop_thres=thres, split_rays=False, max_ray_batch=50)
    for a, b in zip(whole, out):
        assert torch.equal(a, b)


def test_changed_sensor_on_the_device(dev, scene):
    from nvsf.nerf.dataset import dataset_utils, formats as F
    from nvsf.nerf.evaluate import test_step
    m, plain = scene["model"], _frames(scene, dev)
    change = F.SensorChange(delta_position=(0.5, -0.25, 1.0), delta_orientation=(1.0, -2.0, 25.0), H_lidar_new=8, W_lidar_new=48,
                            intrinsics_lidar_new=(10.0, 35.0), delta_pos_camera=(0.5, 0.1, 0.0), delta_orient_camera=(0.0, 3.0, -10.0), H_new=5, W_new=12)
    fs = _frames(scene, dev, sensor=change)
    data = fs.collate([1])
    for key in ("images", "images_lidar", "pano_frame", "image_depths"):
        assert key not in data, key
    assert (data["H"], data["W"], data["H_lidar"], data["W_lidar"]) == (5, 12, 10, 48)
    c = F.apply_sensor_change(plain.poses.cpu(), plain.poses_lidar.cpu(), plain.intrinsics, 6, 8, 6, 32, plain.intrinsics_lidar,
                              plain.intrinsics_hoz_lidar, scene["scale"], change)
    rl = dataset_utils.get_lidar_rays(torch.from_numpy(c["poses_lidar"][1:2]).to(dev), (10.0, 35.0), plain.intrinsics_hoz_lidar, 10, 48)
    rc = dataset_utils.get_rays(torch.from_numpy(c["poses"][1:2]).to(dev), c["intrinsics"], 5, 12)
    assert torch.equal(data["rays_o_lidar"], rl["rays_o"]) and torch.equal(data["rays_d_lidar"], rl["rays_d"])
    assert torch.equal(data["rays_o"], rc["rays_o"]) and torch.equal(data["rays_d"], rc["rays_d"])
    assert data["rays_o_lidar"].shape == (1, 480, 3) and data["rays_o"].shape == (1, 60, 3)
    assert not torch.equal(data["poses_lidar"], plain.poses_lidar[1:2]) and not torch.equal(data["pose"], plain.poses[1:2])
    out = test_step(m, data, 32)
    assert out[0].shape == (1, 5, 12, 3) and out[1].shape == (1, 5, 12) and all(o.shape == (1, 10, 48) for o in out[2:])


def test_export_frames(dev, scene, tmp_path):
    from PIL import Image
    from nvsf.nerf import export as X
    from nvsf.nerf.dataset import formats as F
    from nvsf.nerf.evaluate import test_step
    m = scene["model"]
    fs = _frames(scene, dev, sensor=F.SensorChange(delta_position=(0.0, 0.0, 0.5), H_lidar_new=6, W_lidar_new=40), offset=(1.5, -2.0, 0.25))
    thres = float(test_step(m, fs.collate([0]), 32)[2].median())
    counts = X.export_frames(m, fs, str(tmp_path), "run", 32, raydrop_thres=thres)
    want_files = []
    for i in range(2):
        want_files += [os.path.basename(p) for p in X.frame_paths(str(tmp_path), "run", i).values()]
        data = fs.collate([i])
        _, _, raydrop, intensity, depth = test_step(m, data, 32, raydrop_thres=thres)
        i_u8 = X.quantize_u8(intensity[0].contiguous())
        lidar, world = X.pano_to_cloud(depth[0].contiguous(), i_u8.float(), data["poses_lidar"][0], fs.scale, fs.offset, fs.intrinsics_lidar,
                                       fs.intrinsics_hoz_lidar)
        assert counts[i] == lidar.shape[0] == int((depth[0] != 0).sum()) and 0 < counts[i] < 8 * 40
        p = X.frame_paths(str(tmp_path), "run", i)
        back_l, back_w = np.loadtxt(p["pcd_lidar"], ndmin=2), np.loadtxt(p["pcd_world"], ndmin=2)
        assert back_l.shape == (counts[i], 4) and np.abs(back_l - lidar.cpu().numpy()).max() <= 5e-7 + 1e-12
        assert back_w.shape == (counts[i], 4) and np.abs(back_w - world.cpu().numpy()).max() <= 5e-7 + 1e-12
        assert np.array_equal(back_l[:, 3], np.floor(back_l[:, 3])) and back_l[:, 3].max() <= 255  # the QUANTISED intensity rides along
        assert f"POINTS {counts[i]}" in open(p["pcd"]).read()
        stack = np.asarray(Image.open(p["lidar_png"]))
        assert stack.shape == (3 * 8, 40) and set(np.unique(stack[:8])) <= {0, 255}
        assert np.array_equal(stack[:8] == 255, (raydrop[0] > thres).cpu().numpy()) and np.array_equal(stack[8:16], i_u8.cpu().numpy())
        assert np.asarray(Image.open(p["rgb"])).shape == (6, 8, 3) and np.asarray(Image.open(p["rgb_depth"])).shape == (6, 8)
    assert sorted(os.listdir(str(tmp_path))) == sorted(want_files)
    assert m.training is False
