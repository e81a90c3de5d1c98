"""GPU tests of the U-Net ray-drop refinement (csrc/unet.hip through nvsf/nerf/refine.py): the HIP forward against the fixture of the
reference's own module and against the torch module on the device, the fused gate, repacking after a fit, the eval_step /
evaluate_frames wiring and the argument checks.

Error bar of every comparison of probabilities: 8 x `floor`, where `floor` = max |fp32 - fp64| of the reference's module on CPU, read
from the fixture for the shape (34 x 70's for the shapes the fixture does not hold).  x 2 for two independent fp32 evaluations, x 4 for
the matrix instruction's different accumulation order over up to 4608 terms and for the device's exp.

Measured on MI355X (max |HIP - reference|): 34 x 70: 3.4e-6 against the fixture (bar 1.5e-5), 3.8e-6 against torch on the device;
66 x 1030: 6.9e-6 against the fixture (bar 7.2e-5); 18 x 38: 1.4e-6 against torch on the device."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import unet_params as P  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "unet.npz"))


@pytest.fixture(scope="module")
def refiner(dev, golden):
    from nvsf.nerf.refine import RaydropRefiner
    r = RaydropRefiner(dev)
    assert P.load_into(r.unet) == str(golden["weights_sha256"])
    r.repack()
    return r


@pytest.mark.parametrize("shape", P.SHAPES)
def test_forward_matches_the_reference_fixture(refiner, golden, dev, shape):
    tag = f"{shape[0]}x{shape[1]}"
    floor = float(golden[f"floor_{tag}"])
    x = torch.from_numpy(golden[f"input_{tag}"]).to(dev)
    p = refiner(x[0], x[1], x[2])
    assert p.shape == shape and p.dtype == torch.float32
    err = float((p.cpu() - torch.from_numpy(golden[f"output_{tag}"])).abs().max())
    print(f"{tag}: max |HIP - reference| = {err:.3e}, floor {floor:.3e}, bar {8 * floor:.3e}")
    assert err <= 8 * floor
    assert torch.equal(p, refiner(x[0][None], x[1][None], x[2][None])[0])  # [1, H, W] planes; deterministic


@pytest.mark.parametrize("shape", [(18, 38), (34, 70)])
def test_forward_matches_the_module_on_the_device(refiner, golden, dev, shape):
    floor = float(golden["floor_34x70"])
    x = torch.from_numpy(P.unet_input(*shape, seed=5)).to(dev)
    p, want = refiner(x[0], x[1], x[2]), refiner.torch_forward(x[0], x[1], x[2])
    err = float((p - want).abs().max())
    print(f"{shape}: max |HIP - module on the device| = {err:.3e}, bar {8 * floor:.3e}")
    assert err <= 8 * floor


def test_gated_outputs(refiner, golden, dev):
    thres = 0.5
    for tag in ("34x70", "66x1030"):
        floor = float(golden[f"floor_{tag}"])
        x = torch.from_numpy(golden[f"input_{tag}"]).to(dev)
        p, gi, gd = refiner(x[0], x[1], x[2], thres=thres)
        assert torch.equal(p, refiner(x[0], x[1], x[2]))
        assert torch.equal(gi, x[1] * (p > thres)) and torch.equal(gd, x[2] * (p > thres))  # exactly, with the kernel's own p
        ref = torch.from_numpy(golden[f"output_{tag}"]).to(dev)
        sure = (ref - thres).abs() > 8 * floor
        excluded = 1.0 - float(sure.float().mean())
        print(f"{tag}: {100 * excluded:.4f} % of the pixels within 8 floor of the threshold")
        assert excluded <= 0.005
        assert torch.equal((p > thres)[sure], (ref > thres)[sure])


def test_repacked_after_fit(dev, golden):
    """Three iterations move the weights AND the BatchNorm running statistics: stale or mis-folded packed weights show here."""
    from nvsf.nerf.refine import RaydropRefiner
    torch.manual_seed(3)
    r = RaydropRefiner(dev)
    x = torch.stack([torch.from_numpy(P.unet_input(34, 70, s)) for s in (1, 2)]).to(dev)
    before = r(x[0, 0], x[0, 1], x[0, 2]).clone()
    mean0 = r.unet.down1.conv.double_conv[0].running_mean.clone()
    losses = r.fit_tensors(x, (x[:, :1] > 0.5).float(), iterations=3, generator=torch.Generator().manual_seed(2))
    assert len(losses) == 3 and all(np.isfinite(losses)) and not r.unet.training
    assert not torch.equal(mean0, r.unet.down1.conv.double_conv[0].running_mean)
    p, want = r(x[0, 0], x[0, 1], x[0, 2]), r.torch_forward(x[0, 0], x[0, 1], x[0, 2])
    err, moved = float((p - want).abs().max()), float((p - before).abs().max())
    print(f"after the fit: max |HIP - module| = {err:.3e}; the fit moved the output by {moved:.3e}")
    assert err <= 8 * float(golden["floor_34x70"]) and moved > 1e-3


def test_eval_step_and_table_with_refiner(refiner, tmp_path):
    from test_formats_cpu import make_dataset
    from nvsf.nerf.dataset import formats as F
    from nvsf.nerf.models.network_static import NeRFNetworkStatic
    from nvsf.nerf.evaluate import eval_step, evaluate_frames
    from nvsf.nerf import meters as M
    dev = torch.device("cuda:0")
    seq, *_ = make_dataset(str(tmp_path), n_frames=2, H=24, W=32, Hl=16, Wl=64)
    scale = 0.0108
    fe = F.FrameSet(str(tmp_path), seq, "train", scale, device=dev, training=False)
    torch.manual_seed(1)
    m = NeRFNetworkStatic(bound=2.0, min_near=0.01, min_near_lidar=0.01, lidar_max_depth=0.9).to(dev)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1 and p.numel() > 10000:
                p.normal_(0, 0.3)
    data = fe.collate([1])
    plain = eval_step(m, data, 48, raydrop_thres=-1.0)  # a mask of ones: the unrefined planes as eval_step itself renders them
    rd, it, dp = plain["pred_raydrop"], plain["pred_intensity"], plain["pred_depth"]
    assert rd.shape == (1, 16, 64)
    thres = float(refiner(rd, it, dp).median())
    e = eval_step(m, data, 48, raydrop_thres=thres, refiner=refiner)
    p, gi, gd = refiner(rd, it, dp, thres=thres)
    assert torch.equal(e["pred_raydrop"], p) and not torch.equal(p, rd)
    mask = (p > thres).float()
    assert 0 < float(mask.mean()) < 1
    assert torch.equal(e["pred_intensity"], it * mask) and torch.equal(e["pred_depth"], dp * mask)
    # the reference's loss (trainer.py:736-740, 795-796): L1 range + MSE ray-drop + MSE intensity + MSE RGB, mean-reduced
    lidar = 1.0 * (e["pred_depth"] - e["gt_depth"]).abs().mean() + 0.01 * ((p - e["gt_raydrop"]) ** 2).mean() \
        + 0.1 * ((e["pred_intensity"] - e["gt_intensity"]) ** 2).mean()
    assert float(e["loss"]) == pytest.approx(float(lidar + ((e["pred_rgb"] - e["gt_rgb"]) ** 2).mean()), rel=1e-6)
    without = evaluate_frames(m, fe, 48, raydrop_thres=thres, meters="table")
    res = evaluate_frames(m, fe, 48, raydrop_thres=thres, meters="table", refiner=refiner)
    assert set(res) == set(without) and res["raydrop"] != without["raydrop"]
    hand = M.RaydropMeter(ratio=thres)
    for i in range(2):
        ei = eval_step(m, fe.collate([i]), 48, raydrop_thres=thres, refiner=refiner)
        hand.update(ei["pred_raydrop"], ei["gt_raydrop"])
    np.testing.assert_allclose(np.asarray(res["raydrop"], np.float64), np.asarray(hand.measure(), np.float64), rtol=1e-12, atol=0)


def test_rejections_before_any_launch(refiner, dev):
    from nvsf import _hip
    from nvsf.nerf.refine import RaydropRefiner
    x = torch.from_numpy(P.unet_input(34, 70)).to(dev)
    with pytest.raises(_hip.NvsfHipError):
        refiner(x[0].cpu(), x[1], x[2])
    with pytest.raises((ValueError, _hip.NvsfHipError)):
        refiner(x[0].double(), x[1], x[2])
    with pytest.raises((ValueError, _hip.NvsfHipError)):
        refiner(x[0, :15], x[1, :15], x[2, :15])
    with pytest.raises((ValueError, _hip.NvsfHipError)):
        refiner(x[0], x[1], x[2, :, :64])
    with pytest.raises((ValueError, _hip.NvsfHipError)):
        RaydropRefiner(dev, channels=16)(x[0], x[1], x[2])
    # the C entry itself: status -1, nothing written
    lib, P_ = _hip.load(), _hip.ptr
    out = torch.full((34, 70), -7.0, device=dev)
    ws = refiner._ws[(34, 70)]
    stream = torch.cuda.current_stream().cuda_stream
    args = lambda H, W, n, wsb, gi: (P_(x[0]), P_(x[1]), P_(x[2]), H, W, P_(refiner._packed), n, P_(ws), wsb, 0.5, P_(out), gi, None, stream)
    n = refiner._packed.numel()
    assert lib.nvsf_unet_forward(*args(15, 70, n, ws.numel() * 4, None)) == -1
    assert lib.nvsf_unet_forward(*args(34, 70, n - 1, ws.numel() * 4, None)) == -1
    assert lib.nvsf_unet_forward(*args(34, 70, n, ws.numel() * 4 - 4, None)) == -1
    assert lib.nvsf_unet_forward(*args(34, 70, n, ws.numel() * 4, P_(out))) == -1  # one gated output without the other
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


def test_all_rays_dropped_runs_clean(refiner, dev):
    x = torch.from_numpy(P.unet_input(34, 70, seed=9)).to(dev)
    x[2] = 0.0
    p, gi, gd = refiner(x[0], x[1], x[2], thres=0.5)
    assert bool(torch.isfinite(p).all()) and bool(((p >= 0) & (p <= 1)).all()) and bool((gd == 0).all()) and bool(torch.isfinite(gi).all())
    assert float((p - refiner.torch_forward(x[0], x[1], x[2])).abs().max()) <= 8 * 1.9e-6  # 34 x 70's floor
