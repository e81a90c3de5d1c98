"""Status codes of the fused render entry points for arguments they reject (include/nvsf_hip.h: -1 = NVSF_ERR_INVALID_ARG,
-2 = NVSF_ERR_UNSUPPORTED).  Every case passes real, correctly sized tensors (N = 2 rays, T = 16 samples) with exactly ONE property
wrong, and must be turned away before anything is launched: the status is in NvsfHipError's message and the outputs keep the
sentinel they were filled with.  The same arguments with nothing wrong are accepted (status 0)."""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

N, T = 2, 16
SIGMA_W = 64 * 32 + 16 * 64                 # 32 -> 64 -> 16
HEAD_W = {False: 64 * 32 + 64 * 64 + 16 * 64,   # camera: 32 -> 64 -> 64 -> 16
          True: 64 * 96 + 64 * 64 + 16 * 64}    # LiDAR: 96 -> 64 -> 64 -> 16
SENTINEL = -7.0


def _grids():
    from nvsf import field_ops as ops
    return {"l16f2": ops.GridSpec(3, 16, 2, 12, 16, 1.38), "l8f4": ops.GridSpec(3, 8, 4, 12, 16, 1.5), "l4f8": ops.GridSpec(3, 4, 8, 12, 16, 1.5),
            "l8f2": ops.GridSpec(3, 8, 2, 12, 16, 1.5),
            "decreasing": ops.GridSpec(3, 16, 2, 12, 64, 0.8)}  # hashed levels (64^3 cells in 2^12 rows) before dense ones


class Batch:
    """Arguments of the four entry points, by name, all valid; a case replaces one of them."""

    def __init__(self, dev, grid="l16f2", lidar=False):
        from nvsf import _hip
        g = torch.Generator().manual_seed(5)
        f32 = lambda *shape: torch.rand(*shape, generator=g).to(dev)
        out = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float32, device=dev)
        f16 = lambda n: (torch.randn(n, generator=g) * 0.1).to(torch.float16).to(dev)
        spec = _grids()[grid]
        self.spec, self.lidar, C = spec, lidar, (2 if lidar else 3)
        d = torch.nn.functional.normalize(f32(N, 3) - 0.5, dim=1)
        self.t = dict(rays_o=f32(N, 3) - 0.5, rays_d=d, nears=torch.full((N,), 0.1, device=dev), fars=torch.full((N,), 2.0, device=dev),
                      lin=torch.linspace(0.0, 1.0, T, device=dev), noise=None, table=f16(spec.n_params), sigma_w=f16(SIGMA_W),
                      head_a=f16(HEAD_W[lidar]), head_b=f16(HEAD_W[lidar]) if lidar else None,
                      z_vals=out(N, T), sigmas=out(N, T), weights=out(N, T), weights_sum=out(N), depth=out(N), image=out(N, C),
                      geo=torch.zeros(N * T, 16, dtype=torch.float16, device=dev), x01=out(N * T, 3), h32=out(N * T, 16),
                      feat_rows=torch.zeros(N * T, 32, dtype=torch.float16, device=dev),
                      scratch=torch.zeros(16, N * T, dtype=torch.int32, device=dev))
        self.v = dict(bound=1.0, passes=3, occ_C=1, occ_H=16, max_steps=64)
        self.aabb = _hip.host_f32([-1.0] * 3 + [1.0] * 3)
        self.bg = None if lidar else _hip.host_f32([1.0, 0.5, 0.25])

    def p(self, name):
        from nvsf import _hip
        return _hip.ptr(self.t[name])

    def lead(self):  # rays_o ... h_offsets
        s = self.spec
        return (self.p("rays_o"), self.p("rays_d"), self.p("nears"), self.p("fars"), self.p("lin"), self.p("noise"), self.aabb, float(self.v["bound"]),
                N, T, self.p("table"), s.L, s.F, s.h_scales, s.h_res, s.h_offsets)

    def sliced(self):
        from nvsf import _hip
        _hip.call("nvsf_field_density_uniform_sliced_fwd", *self.lead(), self.p("sigma_w"), self.p("z_vals"), self.p("sigmas"), self.p("geo"),
                  self.p("scratch"), int(self.v["passes"]))

    def train(self):
        from nvsf import _hip
        _hip.call("nvsf_field_density_uniform_train_fwd", *self.lead(), self.p("sigma_w"), self.p("z_vals"), self.p("sigmas"), self.p("geo"),
                  self.p("x01"), self.p("feat_rows"), self.p("h32"), self.p("scratch"))

    def render(self):
        from nvsf import _hip
        _hip.call("nvsf_render_uniform_fwd", *self.lead(), self.p("sigma_w"), 1 if self.lidar else 0, self.p("head_a"), self.p("head_b"), 1.0, 1e-4,
                  self.bg, self.p("scratch"), self.p("z_vals"), self.p("weights"), self.p("weights_sum"), self.p("depth"), self.p("image"))

    def occupancy(self):
        from nvsf import _hip
        C, H, s = int(self.v["occ_C"]), int(self.v["occ_H"]), self.spec
        bits = torch.full((max(1, C * H ** 3 // 8),), 255, dtype=torch.uint8, device=self.t["rays_o"].device)
        _hip.call("nvsf_render_occupancy_fwd", self.p("rays_o"), self.p("rays_d"), self.p("nears"), self.p("fars"), _hip.ptr(bits), float(self.v["bound"]),
                  0.0, int(self.v["max_steps"]), C, H, N, self.p("table"), s.L, s.F, s.h_scales, s.h_res, s.h_offsets, self.p("sigma_w"),
                  1 if self.lidar else 0, self.p("head_a"), self.p("head_b"), 1.0, 1e-4, self.bg, self.p("weights_sum"), self.p("depth"),
                  self.p("image"))

    def untouched(self):
        torch.cuda.synchronize()
        outs = [self.t[k] for k in ("z_vals", "sigmas", "weights", "weights_sum", "depth", "image", "x01", "h32")]
        return all(bool((t == SENTINEL).all()) for t in outs if t is not None)


# (entry point, grid, lidar, the one wrong property, status)
CASES = [
    ("sliced", "l16f2", False, ("v", "passes", 0), -1),
    ("sliced", "l16f2", False, ("v", "passes", 4), -1),
    ("sliced", "l16f2", False, ("t", "scratch", None), -1),
    ("sliced", "l4f8", False, None, -2),
    ("sliced", "decreasing", False, None, -2),
    ("train", "l16f2", False, ("t", "x01", None), -1),
    ("train", "l8f4", False, ("t", "scratch", None), -2),
    ("render", "l16f2", True, ("t", "head_b", None), -1),
    ("render", "l8f4", False, ("t", "scratch", None), -2),
    ("render", "decreasing", False, None, -2),
    ("render", "l16f2", False, ("v", "bound", 0.0), -1),
    ("occupancy", "l16f2", False, ("v", "occ_C", 9), -1),
    ("occupancy", "l16f2", False, ("v", "occ_H", 1), -1),
    ("occupancy", "l16f2", False, ("v", "max_steps", 0), -1),
    ("occupancy", "l8f2", False, None, -2),
    ("occupancy", "decreasing", False, None, -2),
]


def _id(case):
    entry, grid, lidar, wrong, status = case
    what = grid if wrong is None else f"{wrong[1]}={wrong[2]}"
    return f"{entry}-{'lidar-' if lidar else ''}{what}"


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_rejected_with_status(dev, case):
    from nvsf import _hip
    entry, grid, lidar, wrong, status = case
    b = Batch(dev, grid, lidar)
    if wrong is not None:
        kind, name, value = wrong
        (b.t if kind == "t" else b.v)[name] = value
    with pytest.raises(_hip.NvsfHipError) as err:
        getattr(b, entry)()
    found = re.search(r"status (-?\d+)", str(err.value))
    assert found and int(found.group(1)) == status, str(err.value)
    assert b.untouched()  # turned away before any launch


@pytest.mark.parametrize("entry,grid,lidar", [("sliced", "l16f2", False), ("sliced", "l8f4", False), ("train", "l16f2", False), ("train", "l8f4", False),
                                              ("render", "l16f2", True), ("render", "l16f2", False), ("render", "l8f4", False),
                                              ("occupancy", "l16f2", False), ("occupancy", "l8f4", True)])
def test_accepted_when_nothing_is_wrong(dev, entry, grid, lidar):
    """The batches the cases above start from are valid: status 0 (no exception), and the entry point's outputs are written."""
    b = Batch(dev, grid, lidar)
    getattr(b, entry)()
    torch.cuda.synchronize()
    first_output = {"sliced": "sigmas", "train": "h32", "render": "weights", "occupancy": "weights_sum"}[entry]
    assert not bool((b.t[first_output] == SENTINEL).any())
