"""The rotating wave priority of the one-launch LiDAR render (k_render_uniform<true, false, false, *>) steers speed
only: with `wave_priority` = "off" every wave stays at the default priority, and the five outputs are the same bits.  Shapes: one ray,
fewer rays than a workgroup, T below / no multiple of the 8-tile period and of a tile, more than one period, and more rays than the
device has wave slots (4096 + 4: freed slots are refilled, so two resident waves of a SIMD can share a phase).  The camera head and the
training forward do not carry the priority code; one case each shows the switch leaves them alone."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_render_static_gpu import _model, _t

SHAPES = [(1, 16, False), (3, 7, False), (5, 48, True), (37, 100, False), (64, 128, False), (259, 272, True), (4100, 16, False)]


@pytest.fixture(scope="module")
def model():
    return _model(torch.device("cuda", 0), table_std=0.5, seed=3)


def _args(m, N, T, noise, lidar):
    from nvsf import synthetic as S
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1000 + N + T)
    o, d = (S.lidar_rays if lidar else S.camera_rays)(N, rng)
    near = np.full(N, S.MIN_NEAR, np.float32)
    far = np.full(N, S.LIDAR_MAX_DEPTH if lidar else 2.0 * S.BOUND, np.float32)
    nz = torch.rand(N, T, generator=torch.Generator().manual_seed(N * T)).to(dev) if noise else None
    enc = m.hash_encoder_lidar if lidar else m.hash_encoder_camera
    heads = (m.raydrop_net.weights_f16(), m.intensity_net.weights_f16()) if lidar else (m.color_net.weights_f16(), None)
    bg = None if lidar else [1.0, 0.5, 0.25]
    return (_t(o, dev), _t(d, dev), _t(near, dev), _t(far, dev), T, m._aabb_host, float(m.bound), enc.table_f16(), enc.spec,
            m.sigma_net.weights_f16(), lidar, heads[0], heads[1], m._k_scale(), bg, nz)


def _both(fn):
    from nvsf import testing
    on = fn()
    with testing.variant(wave_priority="off"):
        off = fn()
    torch.cuda.synchronize()
    return on, off


@pytest.mark.parametrize("level_kinds", ["compiled", "runtime"])
@pytest.mark.parametrize("N,T,noise", SHAPES)
def test_lidar_render_is_bit_identical_with_and_without_the_rotating_priority(model, N, T, noise, level_kinds):
    from nvsf import field_ops as ops, testing
    args = _args(model, N, T, noise, True)
    with testing.variant(level_kinds=level_kinds):
        on, off = _both(lambda: ops.render_uniform(*args, sliced=False))
    assert len(on) == 5
    for name, a, b in zip(("z_vals", "weights", "weights_sum", "depth", "image"), on, off):
        assert torch.equal(a, b), name
    assert bool(torch.isfinite(on[4]).all()) and float(on[2].abs().sum()) > 0.0


def test_switch_leaves_the_camera_head_and_the_training_forward_alone(model):
    from nvsf import field_ops as ops
    N, T = 37, 100
    cam = _args(model, N, T, True, False)
    on, off = _both(lambda: ops.render_uniform(*cam, sliced=False))
    for a, b in zip(on, off):
        assert torch.equal(a, b)
    a = _args(model, N, T, True, True)
    targs = (*a[:4], T, a[5], a[6], a[15], a[7], a[8], a[9], True, a[11], a[12], a[13], a[14], ops.W_THRESH, False)
    on, off = _both(lambda: ops.render_uniform_train_forward(*targs))
    assert len(on) == 10
    for x, y in zip(on, off):
        assert torch.equal(x, y)
