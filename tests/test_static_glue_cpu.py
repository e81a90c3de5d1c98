"""The host glue of the static field's render path, checked WITHOUT a device against the literal expressions its callers used to spell
out: the per-modality record (NeRFRenderer._modality), the form choice (NeRFNetworkStatic._prefer_sliced), the two shape predicates
(Modality.density_from_rays_built / render_node_built) and the background conversion (renderer_dynamic.bg_host)."""
from types import SimpleNamespace as NS

import pytest
import torch

from nvsf import field_ops as ops
from nvsf import testing
from nvsf.nerf.models.network_static import NeRFNetworkStatic
from nvsf.nerf.models.renderer_dynamic import Modality, bg_host


@pytest.fixture(scope="module", params=["L16F2", "L8F4"])
def model(request):
    kw = {} if request.param == "L16F2" else dict(n_levels_hash=8, n_features_per_level_hash=4)
    m = NeRFNetworkStatic(bound=2, log2_hashmap_size=8, **kw)
    assert ops.sliced_only(m.hash_encoder_camera.spec) == (request.param == "L8F4")
    return m


@pytest.mark.parametrize("lidar", [True, False])
def test_modality_record_is_the_literal_picks(model, lidar):
    self = model
    m = self._modality(lidar)
    assert m.grid is (self.hash_encoder_lidar if lidar else self.hash_encoder_camera)
    assert m.net is self.sigma_net
    if lidar:
        head_a, head_b, venc = self.raydrop_net, self.intensity_net, self.view_encoder_lidar
    else:
        head_a, head_b, venc = self.color_net, None, self.view_encoder_camera
    assert m.head_a is head_a and m.head_b is head_b and m.venc is venc
    ray_length = float(self.lidar_max_depth - self.min_near_lidar) if lidar else 2.0 * float(self.bound)
    assert type(m.ray_length) is float and m.ray_length == ray_length
    assert tuple(m) == (m.grid, m.net, head_a, head_b, venc, ray_length)
    with pytest.raises(AttributeError):
        m.grid = None


@pytest.mark.parametrize("forced", [None, False, True])
def test_form_choice_is_the_three_literal_expressions(model, forced):
    self = model
    seen = set()
    with testing.variant(density_sliced=forced):
        for lidar in (True, False):
            m = self._modality(lidar)
            enc = self.hash_encoder_lidar if lidar else self.hash_encoder_camera
            ray_length = float(self.lidar_max_depth - self.min_near_lidar) if lidar else 2.0 * float(self.bound)
            for N in (256, 4096):
                for T in (48, 64, 768):
                    for coherent in (False, True):
                        # fused_uniform_render (the only caller that knows about coherent batches)
                        want = ops.prefer_sliced(enc.spec, N, T, ray_length, float(self.bound), coherent=coherent)
                        assert self._prefer_sliced(m, N, T, coherent=coherent) == want, (lidar, N, T, coherent)
                        seen.add(want)
                    # density_from_rays
                    assert self._prefer_sliced(m, N, T) == ops.prefer_sliced(enc.spec, N, T, ray_length, float(self.bound))
                    # render_from_rays_train
                    want = ops.prefer_sliced(enc.spec, N, T, ray_length, float(self.bound)) and T % 32 == 0
                    assert self._prefer_sliced(m, N, T, whole_node=True) == want, (lidar, N, T)
                    seen.add(want)
    if forced or ops.sliced_only(self.hash_encoder_camera.spec):
        assert seen == {False, True}  # the choice is exercised both ways (False: T = 48 under whole_node)


def _stand_in(hidden=64, n_hidden=1, in_cols=32, out_cols=16, n_enc=72, head_n_hidden=2, head_n_in=None, b_n_in=None, b_n_out=1, b_n_hidden=2,
              camera=False):
    head_n_in = n_enc + 15 if head_n_in is None else head_n_in
    head = NS(spec=NS(n_hidden=head_n_hidden, n_in=head_n_in, n_out=1))
    head_b = None if camera else NS(spec=NS(n_hidden=b_n_hidden, n_in=head_n_in if b_n_in is None else b_n_in, n_out=b_n_out))
    return Modality(None, NS(spec=NS(n_hidden=n_hidden, hidden=hidden, in_cols=in_cols, out_cols=out_cols)), head, head_b,
                    NS(n_output_dims=n_enc), 1.0)


_CASES = [  # (stand-in arguments, T, density from rays, whole render node)
    (dict(), 64, True, True),
    (dict(camera=True), 64, True, True),
    (dict(hidden=32), 64, False, False),
    (dict(n_hidden=2), 64, False, False),
    (dict(in_cols=48), 64, False, False),
    (dict(out_cols=32), 64, False, False),
    (dict(b_n_in=80), 64, True, False),
    (dict(b_n_out=2), 64, True, False),
    (dict(b_n_hidden=1), 64, True, False),
    (dict(head_n_hidden=1), 64, True, False),
    (dict(head_n_in=90), 64, True, False),
    (dict(n_enc=73), 64, True, False),   # n_enc % 8 != 0
    (dict(n_enc=16, camera=True), 64, True, True),
    (dict(), 72, True, False),           # T % 16 != 0
    (dict(), 48, True, True),
]


@pytest.mark.parametrize("kw, T, want_density, want_node", _CASES)
def test_shape_predicates_are_the_literal_conjunctions(kw, T, want_density, want_node):
    m = _stand_in(**kw)
    net, head_a, head_b, venc = m.net, m.head_a, m.head_b, m.venc
    density = net.spec.n_hidden == 1 and net.spec.hidden == 64 and net.spec.in_cols == 32 and net.spec.out_cols == 16
    hs = head_a.spec
    n_enc = venc.n_output_dims
    node = (net.spec.n_hidden == 1 and net.spec.hidden == 64 and net.spec.in_cols == 32 and net.spec.out_cols == 16
            and hs.n_hidden == 2 and hs.n_in == n_enc + 15 and n_enc % 8 == 0 and T % 16 == 0
            and (head_b is None or (head_b.spec.n_in == hs.n_in and head_b.spec.n_out == hs.n_out and head_b.spec.n_hidden == 2)))
    assert (density, node) == (want_density, want_node)  # each case violates the conjunct it is named for, and only that
    assert m.density_from_rays_built() is density
    assert m.render_node_built(T) is node


def test_the_models_networks_pass_the_predicates(model):
    for lidar in (True, False):
        m = model._modality(lidar)
        assert m.density_from_rays_built() and m.render_node_built(64) and not m.render_node_built(40)


def _old_run(bg_color, out_dim, lidar):
    """NeRFRenderer.run's conversion as it was written (without the bg_radius branch, which stays in `run`)."""
    per_ray_bg = None
    host = None
    if not lidar:
        if bg_color is None:
            host = [1.0] * out_dim
        elif torch.is_tensor(bg_color) and bg_color.numel() > out_dim:
            per_ray_bg = bg_color.reshape(-1, out_dim).to("cpu", torch.float32)
        elif torch.is_tensor(bg_color):
            host = [float(v) for v in bg_color.reshape(-1).expand(out_dim).tolist()] if bg_color.numel() == 1 \
                else [float(v) for v in bg_color.reshape(-1).tolist()]
        else:
            host = [float(bg_color)] * out_dim
    return host, per_ray_bg


def _old_run_cuda(bg_color, lidar):
    """NeRFRenderer.run_cuda's conversion as it was written (reached only with bg_color None, a number or a tensor of <= 3 elements)."""
    if lidar:
        host = None
    elif bg_color is None:
        host = [1.0, 1.0, 1.0]
    elif torch.is_tensor(bg_color):
        host = [float(v) for v in bg_color.reshape(-1).expand(3).tolist()] if bg_color.numel() == 1 \
            else [float(v) for v in bg_color.reshape(-1).tolist()]
    else:
        host = [float(bg_color)] * 3
    return host


@pytest.mark.parametrize("name", ["none", "number", "scalar tensor", "one-element tensor", "three-element tensor", "per-ray rows"])
def test_bg_host_is_both_literal_conversions(name):
    torch.manual_seed(0)
    bg_color = {"none": None, "number": 0.5, "scalar tensor": torch.tensor(0.25), "one-element tensor": torch.tensor([0.75]),
                "three-element tensor": torch.tensor([0.1, 0.2, 0.3]), "per-ray rows": torch.rand(7, 3)}[name]
    for lidar in (False, True):
        host, rows = bg_host(bg_color, 3, lidar)
        want_host, want_rows = _old_run(bg_color, 3, lidar)
        assert host == want_host and (host is None or all(type(v) is float for v in host))
        assert (rows is None) == (want_rows is None)
        if rows is not None:
            assert rows.shape == (7, 3) and torch.equal(rows.to("cpu", torch.float32), want_rows)
        if lidar:
            assert (host, rows) == (None, None)
        if name != "per-ray rows":
            assert rows is None and host == _old_run_cuda(bg_color, lidar)
