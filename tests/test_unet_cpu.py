"""CPU tests of the ray-drop refinement U-Net: the torch module against the reference's schema and the fixture generated from the
reference's own module (tests/golden/golden_unet.py), the BatchNorm folding the kernels rely on, the augmentation boxes, the fit
loop and the checkpoint round trip.  No GPU."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import unet_params as P  # noqa: E402

from nvsf.nerf.models.unet import UNet  # noqa: E402
from nvsf.nerf import refine as R  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "unet.npz"))


@pytest.fixture(scope="module")
def net(golden):
    m = UNet().eval()
    assert P.load_into(m) == str(golden["weights_sha256"])
    return m


def test_state_dict_is_the_reference_schema():
    keys = json.load(open(os.path.join(HERE, "golden", "network_state_dict_keys.json")))
    want = {k[len("unet."):]: list(v) for k, v in keys.items() if k.startswith("unet.")}
    assert len(want) == 112
    assert {k: list(v.shape) for k, v in UNet(in_channels=3, channels=32, out_channels=1).state_dict().items()} == want


@pytest.mark.parametrize("shape", P.SHAPES)
def test_module_matches_the_reference_fixture(net, golden, shape):
    tag = f"{shape[0]}x{shape[1]}"
    floor = float(golden[f"floor_{tag}"])
    np.testing.assert_array_equal(golden[f"input_{tag}"], P.unet_input(*shape))
    with torch.no_grad():
        y, a = net(torch.from_numpy(golden[f"input_{tag}"])[None], return_attention=True)
    err = float(np.abs(y[0, 0].numpy() - golden[f"output_{tag}"]).max())
    print(f"{tag}: max |module - reference| = {err:.3e}, floor {floor:.3e}")
    assert err <= 4 * floor
    if f"attn_{tag}" in golden.files:  # pins the reinterpretation of [heads, HW, C / heads] as [H, W, C]
        ref = golden[f"attn_{tag}"]
        aerr = float(np.abs(a[0].numpy() - ref).max())
        print(f"{tag}: attention max |diff| = {aerr:.3e} of max |value| {np.abs(ref).max():.3e}")
        assert aerr <= 4 * floor


def test_folded_batchnorm_equals_eval_batchnorm():
    g = torch.Generator().manual_seed(3)
    bn = torch.nn.BatchNorm2d(24).eval()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(24, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(24, generator=g) * 0.3)
        bn.running_mean.copy_(torch.randn(24, generator=g))
        bn.running_var.copy_(torch.rand(24, generator=g) * 3 + 0.01)
    x = torch.randn(2, 24, 5, 7, generator=g) * 3
    scale, shift = R.fold_batchnorm(bn)
    with torch.no_grad():
        want = bn(x)
    got = x * scale[None, :, None, None] + shift[None, :, None, None]
    # two fp32 evaluations of the same affine map: a few ulp of the largest term
    assert float((got - want).abs().max()) <= 8 * float(np.finfo(np.float32).eps) * float((x.abs() * scale.abs()[None, :, None, None]).max() + shift.abs().max())


def test_packed_weights_have_the_documented_layout(net):
    packed = R.pack_weights(net)
    n = 0
    for cin, t, cout in [(3, 1, 32)] + [(a, 9, b) for a, b in ((32, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 256))] \
            + [(256, 1, 768), (256, 1, 256)] + [(a, 9, b) for a, b in ((512, 512), (512, 128), (256, 256), (256, 64), (128, 128), (128, 32), (64, 64), (64, 32))] \
            + [(32, 1, 1)]:
        cp = (cin + 15) // 16 * 16
        n += 2 * cp + cout + cp * t * cout
    assert packed.numel() == n and packed.dtype == torch.float32
    # first record: identity scale / zero shift, bias, then w[(ci, tap), co] = weight[co, ci]
    assert torch.equal(packed[:16], torch.ones(16)) and torch.equal(packed[16:32], torch.zeros(16))
    assert torch.equal(packed[32:64], net.inc.conv.bias.detach())
    w = packed[64:64 + 16 * 32].reshape(16, 32)
    assert torch.equal(w[:3], net.inc.conv.weight.detach()[:, :, 0, 0].t()) and torch.equal(w[3:], torch.zeros(13, 32))
    # second record (down1's first convolution): its BatchNorm folded, 3 x 3 taps in (ky, kx) order
    o = 64 + 16 * 32
    scale, shift = R.fold_batchnorm(net.down1.conv.double_conv[0])
    assert torch.equal(packed[o:o + 32], scale) and torch.equal(packed[o + 32:o + 64], shift)
    w = packed[o + 64 + 64:o + 128 + 32 * 9 * 64].reshape(32, 9, 64)
    assert torch.equal(w[5, 7], net.down1.conv.double_conv[3].weight.detach()[:, 5, 2, 1])


LAYOUT_SHAPES = ((16, 16), (31, 47), (34, 70), (66, 1030), (2048, 16), (1448, 1448))


@pytest.mark.parametrize("shape", LAYOUT_SHAPES)
def test_workspace_layout_rows(hip_lib, shape):
    """nvsf_unet_layout: 13 rows {offset in floats, C, H, W} in the order x0 .. x4, mid, qkv, att, x4a, u0 .. u3; host-only, no launch."""
    H, W = shape
    sizes, layout = np.zeros(2, np.uint64), np.full((13, 4), 2 ** 63 + 5, np.uint64)
    assert hip_lib.nvsf_unet_sizes(H, W, sizes.ctypes.data, None) == 0
    assert hip_lib.nvsf_unet_layout(H, W, layout.ctypes.data, None) == 0
    rows = [tuple(int(v) for v in r) for r in layout]
    hs, ws = [H], [W]
    for _ in range(4):  # MaxPool2d(2): floor
        hs.append(hs[-1] // 2)
        ws.append(ws[-1] // 2)
    level = [0, 1, 2, 3, 4, 0, 4, 4, 4, 3, 2, 1, 0]
    chans = [32, 64, 128, 256, 256, 64, 768, 256, 256, 128, 64, 32, 32]
    assert [r[1:] for r in rows] == [(c, hs[l], ws[l]) for c, l in zip(chans, level)]
    end = 0
    for off, c, h, w in rows:
        assert off % 64 == 0 and off >= end  # ascending, no overlap
        end = off + c * h * w
    assert rows[0][0] == 0 and end <= int(sizes[0]) // 4 and int(sizes[0]) % 4 == 0
    # `mid` is the scratch of every Down's and Up's first convolution: the next row starts behind the largest of them
    largest = max(64 * hs[0] * ws[0], 128 * hs[1] * ws[1], 256 * hs[2] * ws[2], 512 * hs[3] * ws[3], 256 * hs[4] * ws[4])
    assert rows[6][0] - rows[5][0] >= largest


@pytest.mark.parametrize("shape", [(15, 70), (70, 15), (387, 5419)])  # 387 x 5419 = 2^21 + 1 pixels
def test_workspace_layout_rejects_what_the_forward_rejects(hip_lib, shape):
    layout, sizes = np.full((13, 4), 77, np.uint64), np.full(2, 77, np.uint64)
    assert hip_lib.nvsf_unet_layout(*shape, layout.ctypes.data, None) == -1
    assert hip_lib.nvsf_unet_sizes(*shape, sizes.ctypes.data, None) == -1
    assert bool((layout == 77).all()) and bool((sizes == 77).all())
    assert hip_lib.nvsf_unet_layout(16, 16, None, None) == -1


def test_stage_oracle_captures_the_module_and_its_logit_band_keeps_enough_pixels():
    """tests/unet_stage_oracle.py, the reference of test_unet_stages_gpu.py: its hooks leave the module's output what it was, its stages
    have the shapes of the workspace rows, and the band 0.02 < p < 0.98 of the fp64 reference alone keeps at least 40 % of the pixels at
    every shape and weight draw of the logit comparison (a condition on the reference, checked before any kernel is involved)."""
    import unet_stage_oracle as O
    m = UNet().eval()
    P.load_into(m, 1)
    with torch.no_grad():
        want = m(torch.from_numpy(P.unet_input(31, 47, O.INPUT_SEED))[None])[0]
    got = O.run_stages(31, 47, 1, O.INPUT_SEED, torch.float32)
    assert torch.equal(got["prob"], want) and torch.equal(torch.sigmoid(got["logit"]), want)
    chans = dict(zip(O.STAGES, (32, 64, 128, 256, 256, 64, 768, 256, 256, 128, 64, 32, 32)))
    level = dict(zip(O.STAGES, (0, 1, 2, 3, 4, 0, 4, 4, 4, 3, 2, 1, 0)))
    for name in O.STAGES:
        assert got[name].shape == (chans[name], 31 >> level[name], 47 >> level[name]) and got[name].is_contiguous(), name
    # att is the tensor the projection reads (a dense copy of attend's permuted view): a mis-ordered capture is off by O(1), a
    # convolution of the copy instead of the view by a few ulp of values up to 4
    assert float((got["x4a"] - (got["x4"] + m.attn.proj(got["att"][None])[0].detach())).abs().max()) <= 64 * float(np.finfo(np.float32).eps)
    for shape in O.SHAPES:
        for seed in O.LOGIT_WEIGHT_SEEDS:
            p = O.run_stages(*shape, seed, O.INPUT_SEED, torch.float64)["prob"]
            kept = float(((p > O.LOGIT_BAND[0]) & (p < O.LOGIT_BAND[1])).double().mean())
            print(f"{shape}, weight draw {seed}: {100 * kept:.1f} % of the pixels inside the band")
            assert kept >= O.BAND_MIN_KEPT, (shape, seed)


def test_augmentation_boxes_stay_within_the_reference_bounds():
    H, W = 66, 1030
    g = torch.Generator().manual_seed(11)
    counts = []
    for _ in range(200):
        boxes = R.draw_boxes(H, W, 32, g)
        counts.append(len(boxes))
        assert len(boxes) < 32
        for y, x, bh, bw in boxes:
            assert 1 <= bh < int(0.1 * H) and 1 <= bw < int(0.1 * W)   # np.random.randint(1, int(0.1 * side))
            assert 0 <= y < H - bh and 0 <= x < W - bw                # np.random.randint(side - size)
    assert min(counts) == 0 and max(counts) == 31
    g2 = torch.Generator().manual_seed(11)
    assert R.draw_boxes(H, W, 32, g2) == R.draw_boxes(H, W, 32, torch.Generator().manual_seed(11))


def _small_fit(seed):
    torch.manual_seed(seed)
    r = R.RaydropRefiner(channels=8)
    x = torch.stack([torch.from_numpy(P.unet_input(34, 70, s)) for s in (1, 2)])
    gt = (x[:, :1] > 0.5).float()
    before = torch.get_rng_state()
    losses = r.fit_tensors(x, gt, iterations=30, generator=torch.Generator().manual_seed(5))
    assert torch.equal(before, torch.get_rng_state())  # the global generator is left alone
    return r, losses


def test_fit_tensors_is_reproducible_and_learns():
    r1, l1 = _small_fit(0)
    r2, l2 = _small_fit(0)
    assert l1 == l2 and len(l1) == 30 and all(np.isfinite(l1))
    assert np.mean(l1[-5:]) < np.mean(l1[:5])
    assert not r1.unet.training
    for a, b in zip(r1.unet.state_dict().values(), r2.unet.state_dict().values()):
        assert torch.equal(a, b)
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=1e-3)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=1e-3, total_steps=30)
    want = []
    for _ in range(30):
        want.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    assert r1.fit_lrs == want


def test_hip_forward_has_no_cpu_fallback():
    from nvsf import _hip
    r = R.RaydropRefiner()
    x = torch.from_numpy(P.unet_input(34, 70))
    with pytest.raises(_hip.NvsfHipError):
        r(x[0], x[1], x[2])
    p = r.torch_forward(x[0][None], x[1][None], x[2][None])  # the module runs anywhere
    assert p.shape == (1, 34, 70) and bool(((p > 0) & (p < 1)).all())


def test_checkpoint_round_trip(tmp_path):
    from nvsf.nerf.models.network_static import NeRFNetworkStatic
    from nvsf.nerf.train_step import RenderTrainStep
    checkpoint_state = RenderTrainStep.checkpoint_state

    class Stub:  # the members checkpoint_state touches for a model-only checkpoint
        model = NeRFNetworkStatic(bound=2)
        global_step = 7

        def sync(self):
            pass

    torch.manual_seed(1)
    r = R.RaydropRefiner()
    with torch.no_grad():
        r.unet.outc.conv[0].running_mean.normal_()
    plain = checkpoint_state(Stub(), full=False)
    state = checkpoint_state(Stub(), full=False, refiner=r)
    assert set(plain) == set(state) and set(state["model"]) - set(plain["model"]) == set(r.state_entries())
    assert not any(k.startswith("unet.") for k in plain["model"])
    path = tmp_path / "ckpt.pth"
    torch.save(state, path)
    for source in (state, str(path), r.state_entries()):
        torch.manual_seed(2)
        r2 = R.RaydropRefiner()
        r2.load_from_checkpoint(source)
        for (ka, a), (kb, b) in zip(r.unet.state_dict().items(), r2.unet.state_dict().items()):
            assert ka == kb and torch.equal(a, b)
    with pytest.raises(KeyError):
        R.RaydropRefiner().load_from_checkpoint(plain)
