"""GPU: the operators between the space-time encoders and (sigma, geo_feat, flow) against references that need no model around them.

  a. k_density_dynamic<0/1> through its four C entries on values where every product and sum is exact: EQUAL to a float64 evaluation;
  b. the blend arithmetic of the same kernel on awkward values (signed zeros, denormals, fp16 overflow, NaN, inf): `x_out` EQUAL to
     tests/torch_f64_tail.tail_input in fp32, which tests/test_dynamic_tail_cpu.py pins to the literal torch expression;
  c. nvsf_density_tail_grad_split through the C ABI: every output is a power-of-two scaling or a cast, EQUAL to the torch expression;
  d. DensityTailFn on exact integers: all gradients EQUAL to float64 autograd through the restatement;
  e. DensityTailFn on random encoder-scale features against float64, element by element at the bar of test_static_grad_f64_gpu.py;
  f. FlowMlpFn, exact and random, the same way.

Every case's data is generated on the CPU from a seed (the builders below carry no device code), so what the references assert about
the data -- exactness of every operand and sum, the number of ReLU-fragile rows -- is checked without a device by
tests/test_dynamic_tail_cpu.py on the same builders.

Measured on an MI355X (largest |g - g64| / bar per tensor over the cases of e and f, rows set aside): see DESIGN.md 4.6.
"""
import itertools

import numpy as np
import pytest
import torch

import torch_f64_tail as T
from test_static_grad_f64_gpu import ATOL, RTOL, SCALE

pytestmark = pytest.mark.gpu

ENTRIES = ("nvsf_density_dynamic_fwd", "nvsf_density_dynamic_f16planes_fwd", "nvsf_density_dynamic_lm_fwd", "nvsf_density_dynamic_lm32_fwd")
PAIRS = ((False, False), (True, False), (False, True), (True, True))  # (hash_1 is fp16, hash_2 is fp16)
CANARY = -777.0
FWD_CAP = 2048 * 4 * 16   # rows one pass of the forward's grid covers (2048 workgroups x 4 waves x 16 rows)
SPLIT_CAP = 4096 * 64     # ... and of the split kernel's
M_FORWARD = (1, 15, 16, 17, 63, 64, 65, 4099, FWD_CAP + 69)
M_SPLIT = (1, 63, 64, 65, 4099, SPLIT_CAP + 65)
M_TAIL_EXACT = (1, 17, 31, 32, 33, 130)
M_TAIL_RANDOM = (1, 17, 130, 4099)
M_FLOW = (1, 31, 32, 33, 5000)
MAX_FRAGILE = 2


def tail_spec():
    from nvsf import field_ops as ops
    return ops.MlpSpec(120, 16, 64, 1)


# ---- builders (CPU, seeded) -----------------------------------------------------------------------------------------------------------
def sparse_integer_weights(shapes, seed, keep=0.2):
    """Sparse small integers as test_mlp_bwd_exact_integers draws them: asymmetric, so a transposed or permuted fragment cannot pass."""
    rng = np.random.default_rng(seed)
    mats = []
    for a, b in shapes:
        W = rng.integers(-2, 3, size=(a, b)).astype(np.float32)
        W[rng.random((a, b)) >= keep] = 0
        mats.append(W)
    return mats


def tail_integer_weights(seed, logit_row):
    """sigma_net weights [W0 64 x 128 | W_out 16 x 64] as one flat fp32 vector.  logit_row: "zero" (sigma == 1, trunc_exp's factor
    exactly 1) or "tame" (the logit is the difference of two hidden units that read six inputs each: |h0| <= 48, exp stays finite)."""
    W0, W1 = sparse_integer_weights(tail_spec().shapes, seed)
    W1[0] = 0
    if logit_row == "tame":
        rng = np.random.default_rng(seed + 1)
        for unit, sign in ((5, 1.0), (41, -1.0)):
            W0[unit] = 0
            W0[unit, rng.choice(128, 6, replace=False)] = rng.choice([-1.0, 1.0], 6)
            W1[0, unit] = sign
    return torch.from_numpy(np.concatenate([W0.reshape(-1), W1.reshape(-1)]))


def quarter_features(M, seed, amplitude=4.0):
    """The eight inputs with multiples of 1/4, |v| <= amplitude: planes fp32 [M, 32], hash_s fp16 [M, 32], hash_d / hash_1 / hash_2 fp32
    [M, 24] (exactly representable in fp16: the caller casts the neighbours for the fp16 regimes)."""
    rng = np.random.default_rng(seed)
    n = int(4 * amplitude)
    q = lambda w: torch.from_numpy((rng.integers(-n, n + 1, size=(M, w)) / 4.0).astype(np.float32))
    return [q(32), q(32), q(32), q(32), q(32).half(), q(24), q(24), q(24)]


def random_features(M, seed):
    """Encoder-scale features: K-planes products around 0.1 - 1, hash features a few tenths."""
    g = torch.Generator().manual_seed(seed)
    r = lambda w, s: torch.randn(M, w, generator=g) * s
    return [r(32, 0.5), r(32, 0.5), r(32, 0.5), r(32, 0.5), r(32, 0.3).half(), r(24, 0.3), r(24, 0.3), r(24, 0.3)]


def xavier(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(a, b, generator=g) * 2 - 1) * (6.0 / (a + b)) ** 0.5 for a, b in shapes]


def with_pair(feats, pair):
    f = list(feats)
    f[6] = f[6].half() if pair[0] else f[6].float()
    f[7] = f[7].half() if pair[1] else f[7].float()
    return f


def alias_planes(tensors, kind):
    """kind "alias": plane_1 is plane_d; "blended": one tensor for plane_d / plane_1 / plane_2; "distinct": as they are."""
    t = list(tensors)
    if kind in ("alias", "blended"):
        t[2] = t[1]
    if kind == "blended":
        t[3] = t[1]
    return t


def level_major(rows):
    return rows.view(rows.shape[0], 8, 4).permute(1, 0, 2).contiguous()


def exact_forward_reference(M):
    """(features, flat weights, x64 [M, 128], h64 [M, 16]) of the exact forward case, with the assertions that make EQUAL the right
    bar: operands of at most 11 significant bits (fp16 holds them), sums below 2^24 units (fp32 accumulation is exact in any order)."""
    feats = quarter_features(M, 100 + M)
    w = tail_integer_weights(7, "tame")
    spec = tail_spec()
    x = T.tail_input(*feats, dtype=torch.float64)
    W0, W1 = [m.double() for m in spec.split(w)]
    unit = 1.0 / 16.0  # the blend of multiples of 1/4
    assert bool((x / unit == torch.round(x / unit)).all()) and float(x.abs().max()) <= 2048 * unit
    assert float((x.abs() @ W0.abs().t()).max()) < 2 ** 24 * unit
    a = torch.relu(x @ W0.t())
    assert float(a.max()) <= 2048 * unit  # an 11-bit multiple of 1/16: the fp16 hidden activation is exact
    assert float((a @ W1.abs().t()).max()) < 2 ** 24 * unit
    h = a @ W1.t()
    assert float(h[:, 0].abs().max()) <= 48
    # the restatement's own MLP says the same
    assert torch.equal(T.density_tail(*feats, w.double(), spec)[2], h)
    return feats, w, x, h


EDGE_TRIPLES = [  # (d, d1, d2) of 0.5 d + 0.25 (d1 + d2)
    (0.0, -0.0, 0.0), (-0.0, -0.0, -0.0), (0.0, 0.0, -0.0), (-0.0, 0.0, 0.0),
    (2.0 ** -24, 2.0 ** -24, 2.0 ** -24), (3 * 2.0 ** -24, -2.0 ** -24, 0.0), (-2.0 ** -24, 0.0, 2.0 ** -23), (2.0 ** -14, 2.0 ** -24, -2.0 ** -15),
    (2.0 ** -149, 0.0, 0.0), (-2.0 ** -140, 2.0 ** -130, 2.0 ** -149), (3 * 2.0 ** -149, 2.0 ** -149, 2.0 ** -149), (-2.0 ** -127, -2.0 ** -127, 0.0),
    (-1.0, 40000.0, 40000.0), (1.0, 65504.0, 65504.0), (0.0, 65504.0, 32.0), (0.0, -65504.0, -16.0), (0.0, 2049.0, 1.0), (0.0, 4098.0, 4098.0),
    (131008.0, 0.0, 0.0), (131038.0, 0.0, 0.0), (131039.99, 0.0, 0.0), (131040.0, 0.0, 0.0), (131072.0, 0.0, 0.0), (-131039.99, 0.0, 0.0),
    (65504.0, 65504.0, 65504.0), (65519.0, 65519.0, 65519.0), (65520.0, 65520.0, 65520.0), (1e5, 1e5, -3e5),
    (float("nan"), 1.0, 1.0), (1.0, float("nan"), 1.0), (float("inf"), 1.0, 1.0), (1.0, float("inf"), float("-inf")), (1.0, 1.0, float("-inf")),
]
EDGE_ROWS = tuple(range(0, 10)) + tuple(range(12, 21))  # the first rows, and across the 16-row tile boundary


def edge_features(M, seed):
    """Random rows with the edge block written over EDGE_ROWS: column j of edge row r holds triple (7 r + j) mod K in (plane_d, plane_1,
    plane_2) and in (hash_d, hash_1, hash_2); plane_s and hash_s hold the triple's first value."""
    f = random_features(M, seed)
    tri = torch.tensor(EDGE_TRIPLES, dtype=torch.float32)
    for r in EDGE_ROWS:
        if r >= M:
            continue
        k32 = (7 * r + torch.arange(32)) % tri.shape[0]
        k24 = k32[:24]
        f[0][r], f[1][r], f[2][r], f[3][r] = tri[k32, 0], tri[k32, 0], tri[k32, 1], tri[k32, 2]
        f[4][r] = tri[k32, 0].half()
        f[5][r], f[6][r], f[7][r] = tri[k24, 0], tri[k24, 1], tri[k24, 2]
    return f


def same_bits(a, b):
    """Elementwise: the same bit pattern, or both NaN."""
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    view = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return (a.contiguous().view(view) == b.contiguous().view(view)) | (torch.isnan(a) & torch.isnan(b))


def all_same_bits(a, b):
    return bool(same_bits(a, b).all())


def tail_random_case(M, seed, edges, pair, kind):
    """Features, weights and incoming gradients of one random DensityTailFn case.  edges: the logit row centred and scaled so that the
    logits spread to +-25 (99th percentile), as test_static_grad_f64_gpu._model(..., edges=True) does; loss scale 1 there, else 64.
    The incoming sigma gradient of the edges case falls off like 1 / sigma for positive logits, as a compositor's does once alpha
    saturates: g_sigma clamp(sigma) times the backward's own 128 then stays inside fp16.  Rows the restatement calls ReLU-fragile get
    a zero incoming gradient (both sides read the same tensors)."""
    spec = tail_spec()
    feats = alias_planes(with_pair(random_features(M, seed), pair), kind)
    W0, W1 = xavier(spec.shapes, seed + 1)
    W0, W1 = W0.half().float(), W1.half().float()
    x = T.tail_input(*feats, dtype=torch.float64)
    if edges:
        probe = T.tail_input(*random_features(4096, seed + 2), dtype=torch.float64)
        a = torch.relu(probe @ W0.double().t()).half().double()
        W1[0] -= W1[0].mean()
        W1 = W1.half().float()
        h0 = a @ W1[0].double()
        W1[0] *= 25.0 / float(h0.abs().quantile(0.99))
    w = torch.cat([W0.reshape(-1), W1.reshape(-1)])
    scale = 1.0 if edges else SCALE
    g = torch.Generator().manual_seed(seed + 3)
    g_sigma = torch.randn(M, generator=g, dtype=torch.float64)
    g_geo = torch.randn(M, 15, generator=g, dtype=torch.float64)
    if edges:
        h0 = torch.relu(x @ W0.double().t()).half().double() @ W1[0].half().double()
        g_sigma = g_sigma * torch.exp(-h0.clamp(min=0.0))
    fragile = T.fragile_rows(x, [W0])
    g_sigma = torch.where(fragile, torch.zeros_like(g_sigma), g_sigma) * scale
    g_geo = torch.where(fragile[:, None], torch.zeros_like(g_geo), g_geo) * scale
    return feats, w, g_sigma.float(), g_geo.float(), int(fragile.sum())


TAIL_RANDOM_CASES = {  # id: (M, seed, edges, (hash_1 fp16, hash_2 fp16), level-major hash_s, planes)
    "M1": (1, 11, False, (True, True), False, "distinct"),
    "M17_lm": (17, 12, False, (True, False), True, "distinct"),
    "M130_edges": (130, 13, True, (True, True), True, "blended"),
    "M4099_alias": (4099, 14, False, (False, True), True, "alias"),
    "M4099_edges": (4099, 15, True, (True, True), False, "distinct"),
}


def flow_integer_case(M, seed=3):
    """x [M, 32] small integers, Linear weights sparse small integers, incoming gradient [M, 6] sparse small integers."""
    rng = np.random.default_rng(seed + M)
    w0, w1, w2 = [torch.from_numpy(m) for m in sparse_integer_weights([(64, 32), (64, 64), (6, 64)], seed, keep=0.1)]
    x = torch.from_numpy(rng.integers(-2, 3, size=(M, 32)).astype(np.float32))
    g = rng.integers(-1, 2, size=(M, 6)).astype(np.float32)  # two layers of sums must keep 128 g inside fp16's integers
    g[rng.random((M, 6)) < 0.5] = 0
    if M > 1000:
        g[rng.random(M) < 0.9] = 0
    return x, w0, w1, w2, torch.from_numpy(g)


def flow_random_case(M, seed, g_scale):
    g = torch.Generator().manual_seed(seed)
    w0, w1, w2 = xavier([(64, 32), (64, 64), (6, 64)], seed + 1)
    w2 = torch.randn(6, 64, generator=g) * 0.2
    x = torch.randn(M, 32, generator=g) * 0.3
    x16 = x.half().double()
    fragile = T.fragile_rows(x16, [w0, w1])
    go = torch.randn(M, 6, generator=g, dtype=torch.float64)
    go = torch.where(fragile[:, None], torch.zeros_like(go), go) * g_scale
    return x, w0, w1, w2, go.float(), int(fragile.sum())


FLOW_RANDOM_CASES = {"M1_x64": (1, 21, 64.0), "M31_x64": (31, 22, 64.0), "M32_tiny": (32, 26, 2.0 ** -10), "M33_tiny": (33, 23, 2.0 ** -10), "M5000_x64": (5000, 28, 64.0),
                     "M5000_tiny": (5000, 25, 2.0 ** -10)}


def representable_after_scale(g, scale=128.0):
    """Integers whose product with the MLP backward's own gradient scale is an fp16 value (|k| <= 2048)."""
    return bool((g == torch.round(g)).all()) and float(g.abs().max()) * scale <= 2048.0


def tail_exact_reference(M, case):
    """Float64 autograd of one exact DensityTailFn case -> (features, requires-grad mask, weights, g_sigma, g_geo, gradients by slot)
    with the assertions that make EQUAL the right bar."""
    kind, pair, lm, needs, use_sigma, use_geo = TAIL_EXACT_CASES[case]
    feats = with_pair(quarter_features(M, 300 + M, amplitude=2.0), pair)
    if lm:
        feats[4] = level_major(feats[4])
    w = tail_integer_weights(9, "zero")
    rng = np.random.default_rng(M)
    g_sigma = torch.from_numpy(rng.integers(-2, 3, size=M).astype(np.float32))
    g_geo = torch.from_numpy(rng.integers(-1, 2, size=(M, 15)).astype(np.float32))  # 15 of them meet in a hidden unit's gradient
    leaves = alias_planes([f.double().requires_grad_(i in needs) for i, f in enumerate(feats)], kind)
    w64 = w.double().requires_grad_(8 in needs)
    spec = tail_spec()
    sigma, geo, h, x = T.density_tail(*leaves, w64, spec, half=pair)
    assert bool((sigma == 1).all())
    loss = 0.0
    if use_sigma:
        loss = loss + (sigma * g_sigma.double()).sum()
    if use_geo:
        loss = loss + (geo * g_geo.double()).sum()
    loss.backward()
    # exactness: the logit and hidden gradients times 128 are fp16 values, every sum stays below 2^24 units of 1/16
    W0, W1 = [m.double() for m in spec.split(w)]
    G = torch.zeros(M, 16, dtype=torch.float64)
    if use_sigma:
        G[:, 0] = g_sigma.double()
    if use_geo:
        G[:, 1:] = g_geo.double()
    a = torch.relu(x.detach() @ W0.t())
    assert float(a.max()) <= 128.0
    gh = (G @ W1) * (a > 0)
    assert representable_after_scale(G) and representable_after_scale(gh)
    assert float((gh.abs().t() @ x.detach().abs()).max()) * 16 < 2 ** 24 and float((G.abs().t() @ a).max()) * 16 < 2 ** 24
    assert float((gh.abs() @ W0.abs()).max()) <= 2048  # the hash_s gradient is handed back in fp16
    grads = [None if (l.grad is None) else l.grad for l in leaves] + [w64.grad]
    return feats, kind, w, g_sigma, g_geo, grads


# id: (planes, (hash_1 fp16, hash_2 fp16), level-major hash_s, slots that require a gradient (0..5 inputs, 8 = params), g_sigma, g_geo)
_ALL = (0, 1, 2, 3, 4, 5, 8)
TAIL_EXACT_CASES = {
    "distinct_rows": ("distinct", (True, True), False, _ALL, True, True),
    "alias_plane_1": ("alias", (False, True), True, _ALL, True, True),
    "blended_lm": ("blended", (True, False), True, _ALL, True, True),
    "distinct_lm_f32_neighbours": ("distinct", (False, False), True, _ALL, True, True),
    "only_params": ("distinct", (True, True), True, (8,), True, True),
    "only_hash_d": ("blended", (True, True), False, (5,), True, True),
    "no_g_sigma": ("distinct", (True, True), True, _ALL, False, True),
    "no_g_geo": ("alias", (True, True), False, _ALL, True, False),
}


def compare_to_bar(name, g, g64):
    """-> max |g - g64| / (ATOL max|g64| + RTOL |g64|), the bar of tests/test_static_grad_f64_gpu.py; asserts it, finiteness, and that
    no entry the reference has above 1e-4 of the largest is zero."""
    g, g64 = g.double().reshape(-1).cpu(), g64.reshape(-1).cpu()
    assert g.shape == g64.shape and bool(torch.isfinite(g).all()), name
    top = float(g64.abs().max())
    assert top > 0, name
    big = g64.abs() > 1e-4 * top
    assert bool((g[big] != 0).all()), f"{name}: zero where the reference is not"
    ratio = (g - g64).abs() / (ATOL * top + RTOL * g64.abs())
    worst, i = float(ratio.max()), int(ratio.argmax())
    assert worst <= 1.0, f"{name}: |g - g64| / bar = {worst:.3g} at {i}: {float(g[i]):.6g} vs {float(g64[i]):.6g} (max {top:.3g})"
    return worst


# ---- device helpers ---------------------------------------------------------------------------------------------------------------------
def _canaried(rows, cols, dtype, dev, pad=8):
    buf = torch.full(((rows + pad) * cols,), CANARY, dtype=dtype, device=dev)
    return buf, buf[:rows * cols].view(rows, cols) if cols > 1 else buf[:rows]


def _untouched(buf, n):
    return bool((buf[n:] == CANARY).all())


def run_forward(entry, feats, w16, dev, rot, want_x):
    """One launch of a forward entry on the CPU tensors `feats` (hash_1 / hash_2 in the dtype of their regime) -> dict of outputs;
    asserts that the rows behind every output keep their canary."""
    from nvsf import _hip
    M = feats[0].shape[0]
    ps, pd, p1, p2, hs, hd, h1, h2 = feats
    keep = []

    def on(t):
        keep.append(t.contiguous().to(dev))
        return _hip.ptr(keep[-1])
    if entry in (ENTRIES[0], ENTRIES[3]):
        planes = [on(ps), on(pd), on(p1), on(p2)]
    else:  # what nvsf_planes_multi_fwd(blend = 2) hands over: the fp32 blend rounded to fp16
        planes = [on(ps.half()), on((0.5 * pd + 0.25 * (p1 + p2)).half())]
    hash_s = on(level_major(hs) if entry in (ENTRIES[2], ENTRIES[3]) else hs)
    args = planes + [hash_s, on(hd), on(h1), 1 if h1.dtype == torch.float16 else 0, on(h2), 1 if h2.dtype == torch.float16 else 0, M, _hip.ptr(w16)]
    out = {}
    xb, x = _canaried(M, 128, torch.float16, dev)
    if rot == 0:
        hb, h = _canaried(M, 16, torch.float32, dev)
        _hip.call(entry, *args, _hip.ptr(hb), None, None, _hip.ptr(xb) if want_x else None)
        assert _untouched(hb, M * 16)
        out["h"] = h
    else:
        sb, s = _canaried(M, 1, torch.float32, dev)
        gb, geo = _canaried(M, 16, torch.float16, dev)
        _hip.call(entry, *args, None, _hip.ptr(sb), _hip.ptr(gb), _hip.ptr(xb) if want_x else None)
        assert _untouched(sb, M) and _untouched(gb, M * 16)
        out["sigma"], out["geo"] = s, geo
    assert _untouched(xb, M * 128 if want_x else 0)
    if want_x:
        out["x"] = x
    return out


@pytest.fixture(scope="module")
def tail_net(dev):
    from nvsf.nerf.models.network_dynamic import NeRFNetwork
    torch.manual_seed(1)
    return NeRFNetwork(time_resolution=3, num_frames=9, bound=2.0, min_resolution=8, base_resolution=16, max_resolution=256,
                       log2_hashmap_size=12).to(dev)


def _set_sigma_net(net, w):
    with torch.no_grad():
        net.sigma_net.params.copy_(w.to(net.sigma_net.params.device))
    net.sigma_net.params.grad = None


def run_tail_fn(net, feats, kind, needs, g_sigma, g_geo, dev, use_sigma=True, use_geo=True):
    """DensityTailFn.apply on device copies of `feats` -> (sigma, geo, gradients by slot [8 inputs + params], composed-path flag).
    The geometry gradient arrives as 15 columns of 16-float rows, the layout the heads' backward leaves it in."""
    from nvsf import field_ops as ops
    from nvsf.nerf.models.network_dynamic import DensityTailFn
    leaves = alias_planes([f.to(dev).requires_grad_(i in needs) for i, f in enumerate(feats)], kind)
    params = net.sigma_net.params
    params.requires_grad_(8 in needs)
    params.grad = None
    sigma, geo = DensityTailFn.apply(net, *leaves, params)
    outs, gouts = [], []
    if use_sigma:
        outs.append(sigma)
        gouts.append(g_sigma.to(dev))
    if use_geo:
        rows = torch.zeros(geo.shape[0], 16, device=dev)
        rows[:, :15] = g_geo.to(dev)
        outs.append(geo)
        gouts.append(rows[:, :15])
    seen = []
    real = ops.density_logit_gradient_parts

    def spy(*a, **k):
        seen.append(real(*a, **k))
        return seen[-1]
    ops.density_logit_gradient_parts = spy
    try:
        torch.autograd.backward(outs, gouts)
    finally:
        ops.density_logit_gradient_parts = real
        params.requires_grad_(True)
    grads = [l.grad for l in leaves] + [params.grad]
    return sigma.detach(), geo.detach(), grads, bool(seen and seen[-1] is not None)


# ---- a. forward, exact ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", M_FORWARD)
def test_forward_exact(dev, M):
    """All four entries x ROT 0 / 1 x x_out requested or not, the four (hash_1, hash_2) dtype pairs taken in turn: `h` and all 128
    columns of `x_out` EQUAL the float64 evaluation; ROT = 1: geo[:, :15] == half(h[:, 1:16]), geo[:, 15] == 1, sigma within 2 fp32
    ulps of the float64 exponential of the logit (the device expf is documented at 1 ulp, the second covers the reference's own
    rounding to fp32); canary rows behind every output stay untouched."""
    feats, w, x64, h64 = exact_forward_reference(M)
    w16 = w.half().to(dev)
    h_ref, x_ref = h64.float().to(dev), x64.half().to(dev)
    geo_ref = torch.cat([h_ref[:, 1:16].half(), torch.ones(M, 1, dtype=torch.float16, device=dev)], -1)
    s64 = torch.exp(h64[:, 0])
    s_ref = s64.float().to(dev)
    ulp = (torch.nextafter(s_ref, torch.full_like(s_ref, float("inf"))) - s_ref).double()
    for n, (entry, rot, want_x) in enumerate(itertools.product(ENTRIES, (0, 1), (True, False))):
        pair = PAIRS[(n + n // 4) % 4]
        out = run_forward(entry, with_pair(feats, pair), w16, dev, rot, want_x)
        tag = (entry, rot, want_x, pair)
        if rot == 0:
            assert torch.equal(out["h"], h_ref), tag
        else:
            assert torch.equal(out["geo"], geo_ref), tag
            assert bool(((out["sigma"].double() - s64.to(dev)).abs() <= 2 * ulp).all()), tag
        if want_x:
            assert torch.equal(out["x"], x_ref), tag


# ---- b. forward, blend arithmetic on awkward values ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", (40, 77))
def test_forward_blend_on_awkward_values(dev, M):
    """x_out is elementwise with no contraction: bit for bit tail_input in fp32, evaluated on the device and on the CPU (NaN = NaN), for
    the four dtype pairs and the four entries; the fp32-plane and the fp16-plane entries give bit-identical `h`."""
    spec = tail_spec()
    W0, W1 = xavier(spec.shapes, 5)
    w16 = torch.cat([W0.reshape(-1), W1.reshape(-1)]).half().to(dev)
    base = edge_features(M, 40 + M)
    for pair in PAIRS:
        feats = with_pair(base, pair)
        ref_cpu = T.tail_input(*feats, dtype=torch.float32).half()
        ref_dev = T.tail_input(*[f.to(dev) for f in feats], dtype=torch.float32).half()
        assert all_same_bits(ref_dev.cpu(), ref_cpu), pair
        hs = []
        for entry in ENTRIES:
            out = run_forward(entry, feats, w16, dev, 0, True)
            bad = ~same_bits(out["x"].cpu(), ref_cpu)
            assert not bool(bad.any()), (entry, pair, bad.nonzero()[:4].tolist(), out["x"].cpu()[bad][:4], ref_cpu[bad][:4])
            hs.append(out["h"])
        for h in hs[1:]:
            assert all_same_bits(h, hs[0]), pair
        clean = torch.ones(M, dtype=torch.bool)
        clean[list(EDGE_ROWS)] = False
        assert bool(torch.isfinite(hs[0].cpu()[clean]).all())  # what an edge row holds stays in its row


# ---- c. nvsf_density_tail_grad_split ------------------------------------------------------------------------------------------------------
def split_input(M, stride, seed=0):
    g = torch.Generator().manual_seed(seed + M)
    gx = torch.randn(M, stride, generator=g) * torch.exp(torch.randn(M, 1, generator=g) * 4)
    special = torch.tensor([0.0, -0.0, 65504.0, 65519.9, 65520.0, -1e6, 3e38, 2.0 ** -149, -2.0 ** -130, 2.0 ** -126, 2.0 ** -24, 3 * 2.0 ** -25,
                            float("nan"), float("inf"), float("-inf"), 2.0 ** -14 * 0.999])
    n = min(M, 5)
    for r in range(n):
        gx[r] = special[(torch.arange(stride) + 3 * r) % special.numel()]
    gx[M - 1, :120] = special[(torch.arange(120) * 5) % special.numel()]
    return gx


def split_reference(gx, hs_f16, hs_lm, hd_col, half_scale):
    """The torch expressions of DensityTailFn.backward's fallback branch, on the CPU."""
    hs = gx[:, 64:96].to(torch.float16 if hs_f16 else torch.float32)
    hd = 0.5 * gx[:, 96:120]
    return {"half": half_scale * gx[:, 32:64], "quarter": 0.25 * gx[:, 32:64], "hash_s": level_major(hs.contiguous()) if hs_lm else hs,
            "hash_d": hd.t().contiguous() if hd_col else hd.contiguous(), "plane_s": gx[:, 0:32].contiguous()}


_SPLIT_OUTPUTS = ("half", "quarter", "hash_s", "hash_d", "plane_s")


def run_split(gx_dev, M, stride, present, hs_f16, hs_lm, hd_col, half_scale, dev, ref):
    """One launch; -> list of (label, device bool) that every present output equals `ref` bit for bit and every canary survived."""
    from nvsf import _hip
    bufs, ptrs = {}, {}
    for name in _SPLIT_OUTPUTS:
        dtype = torch.float16 if (name == "hash_s" and hs_f16) else torch.float32
        n = M * (24 if name == "hash_d" else 32)
        bufs[name] = torch.full((n + 64,), CANARY, dtype=dtype, device=dev)
        ptrs[name] = bufs[name].data_ptr() if name in present else None
    _hip.call("nvsf_density_tail_grad_split", gx_dev.data_ptr(), stride, M, ptrs["half"], ptrs["quarter"], ptrs["hash_s"], 1 if hs_f16 else 0,
              1 if hs_lm else 0, ptrs["hash_d"], 1 if hd_col else 0, ptrs["plane_s"], float(half_scale))
    checks = []
    for name in _SPLIT_OUTPUTS:
        n = bufs[name].numel() - 64
        if name in present:
            checks.append((name, same_bits(bufs[name][:n], ref[name].reshape(-1)).all() & (bufs[name][n:] == CANARY).all()))
        else:
            checks.append((name + " (absent)", (bufs[name] == CANARY).all()))
    return checks


@pytest.mark.parametrize("M", M_SPLIT)
def test_grad_split_equals_the_torch_expressions(dev, M):
    """hash_s fp16 / fp32 x rows / level-major, hash_d row- / column-major, plane_half_scale 0.5 / 1, gx_stride 120 / 124 / 128, each
    output pointer absent once and all present; the full product at the tile sizes, a covering subset above them."""
    layouts = list(itertools.product((True, False), (False, True), (False, True), (0.5, 1.0)))
    presents = [tuple(_SPLIT_OUTPUTS)] + [tuple(n for n in _SPLIT_OUTPUTS if n != skip) for skip in _SPLIT_OUTPUTS]
    if M <= 65:
        combos = list(itertools.product((120, 124, 128), layouts, presents))
    elif M <= 4099:
        combos = [(s, l, presents[(i + j) % 6]) for i, s in enumerate((120, 124, 128)) for j, l in enumerate(layouts)]
    else:
        combos = [(120, layouts[0], presents[0]), (128, layouts[15], presents[0]), (124, layouts[6], presents[3])]
    failed = []
    cache = {}
    for stride, (hs_f16, hs_lm, hd_col, half_scale), present in combos:
        if stride not in cache:
            gx = split_input(M, stride)
            cache = {stride: (gx.to(dev), {})}
        gx_dev, refs = cache[stride]
        key = (hs_f16, hs_lm, hd_col, half_scale)
        if key not in refs:
            refs[key] = {k: v.to(dev) for k, v in split_reference(gx_dev.cpu(), *key).items()}
        for label, ok in run_split(gx_dev, M, stride, present, hs_f16, hs_lm, hd_col, half_scale, dev, refs[key]):
            failed.append(((stride, key, label), ok))
    verdicts = torch.stack([ok for _, ok in failed]).cpu()
    assert bool(verdicts.all()), [failed[i][0] for i in (~verdicts).nonzero().flatten().tolist()][:8]


def test_grad_split_rejects_and_writes_nothing(dev):
    """The REQUIRE lines: no input, a stride below 120 or not a multiple of 4, no output at all, a misaligned pointer -> an error
    status, and no output byte written."""
    from nvsf import _hip
    M = 70
    gx = split_input(M, 128).to(dev)
    outs = {n: torch.full((M * 32 + 64,), CANARY, device=dev) for n in _SPLIT_OUTPUTS}
    hs16 = torch.full((M * 32 + 64,), CANARY, dtype=torch.float16, device=dev)
    p = {n: t.data_ptr() for n, t in outs.items()}
    ok = (gx.data_ptr(), 128, M, p["half"], p["quarter"], p["hash_s"], 0, 0, p["hash_d"], 1, p["plane_s"], 0.5)

    def bad(**change):
        names = ("gx", "stride", "M", "half", "quarter", "hash_s", "hs_f16", "hs_lm", "hash_d", "hd_col", "plane_s", "scale")
        args = list(ok)
        for k, v in change.items():
            args[names.index(k)] = v
        with pytest.raises(_hip.NvsfHipError, match="rejected arguments"):
            _hip.call("nvsf_density_tail_grad_split", *args)
    bad(gx=None)
    bad(stride=119)
    bad(stride=116)
    bad(stride=122)
    bad(half=None, quarter=None, hash_s=None, hash_d=None, plane_s=None)
    bad(gx=gx.data_ptr() + 4)
    for name in ("half", "quarter", "hash_d", "plane_s", "hash_s"):
        bad(**{name: p[name] + 4})
    bad(hash_s=hs16.data_ptr() + 2, hs_f16=1)
    bad(hash_s=hs16.data_ptr() + 4, hs_f16=1)
    torch.cuda.synchronize()
    assert all(bool((t == CANARY).all()) for t in outs.values()) and bool((hs16 == CANARY).all())
    _hip.call("nvsf_density_tail_grad_split", *ok)  # and the unchanged arguments are accepted
    assert not bool((outs["half"][:M * 32] == CANARY).all())


# ---- d. DensityTailFn, exact ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(TAIL_EXACT_CASES))
@pytest.mark.parametrize("M", M_TAIL_EXACT)
def test_tail_fn_exact(dev, tail_net, variants, M, case):
    """Gradients of every input that requires one and of sigma_net.params EQUAL float64 autograd through density_tail, under mlp_bwd
    wave / staged x density_grad composed / matrix; an input that requires none gets None (hash_1 / hash_2 never do: `density`
    takes this node only when they carry no gradient)."""
    _, _, _, needs, use_sigma, use_geo = TAIL_EXACT_CASES[case]
    feats, kind, w, g_sigma, g_geo, ref = tail_exact_reference(M, case)
    _set_sigma_net(tail_net, w)
    for bwd, dg in itertools.product(("wave", "staged"), ("composed", "matrix")):
        variants.set(mlp_bwd=bwd, density_grad=dg)
        sigma, geo, grads, composed = run_tail_fn(tail_net, feats, kind, needs, g_sigma, g_geo, dev, use_sigma, use_geo)
        tag = (bwd, dg)
        assert composed == (dg == "composed" and use_geo), tag
        assert bool((sigma == 1).all()), tag
        for slot, (g, g64) in enumerate(zip(grads, ref)):
            if slot not in needs:
                assert g is None and g64 is None, (tag, slot)
                continue
            assert g is not None and g.shape == g64.shape and g.dtype == (feats[slot].dtype if slot < 8 else torch.float32), (tag, slot)
            assert torch.equal(g.double().cpu(), g64), (tag, slot, float((g.double().cpu() - g64).abs().max()))


# ---- e. DensityTailFn, random, against float64 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(TAIL_RANDOM_CASES))
def test_tail_fn_random_against_fp64(dev, tail_net, case):
    """Encoder-scale features: geo within the forward bar of test_mlp_forward (1e-3 of the largest logit, 97 % within 2e-6 of it), sigma
    relative to the float64 exponential accordingly; every gradient element within RTOL / ATOL of test_static_grad_f64_gpu.py (derived
    there for six fp16 operand roundings; this path has three: logit gradient, hidden gradient, the fp16 hash_s hand-over).  The largest
    fraction of the bar per tensor is printed (below one fifth everywhere)."""
    M, seed, edges, pair, lm, kind = TAIL_RANDOM_CASES[case]
    spec = tail_spec()
    feats, w, g_sigma, g_geo, n_fragile = tail_random_case(M, seed, edges, pair, kind)
    assert n_fragile <= MAX_FRAGILE
    if lm:
        feats[4] = level_major(feats[4])
    needs = _ALL
    leaves = alias_planes([f.double().requires_grad_(i in needs) for i, f in enumerate(feats)], kind)
    w64 = w.double().requires_grad_()
    s64, geo64, h64, _ = T.density_tail(*leaves, w64, spec, half=pair)
    ((s64 * g_sigma.double()).sum() + (geo64 * g_geo.double()).sum()).backward()
    _set_sigma_net(tail_net, w)
    sigma, geo, grads, _ = run_tail_fn(tail_net, feats, kind, needs, g_sigma, g_geo, dev)
    # outputs: the forward bar of test_mlp_forward on the logits (1e-3 of the largest, 97 % within 2e-6 of it), sigma accordingly
    h64 = h64.detach()
    scale = float(h64.abs().max())
    err = (geo.double().cpu() - h64[:, 1:16]).abs()
    assert float(err.max()) <= 1e-3 * scale
    rel = (sigma.double().cpu() / s64.detach() - 1.0).abs()
    assert float(rel.max()) <= float(np.expm1(1e-3 * scale)) + 2.0 ** -22
    if M >= 100:
        assert float((err <= 2e-6 * scale).double().mean()) > 0.97
        assert float((rel <= float(np.expm1(2e-6 * scale)) + 2.0 ** -22).double().mean()) > 0.97
    worst = {}
    names = ("plane_s", "plane_d", "plane_1", "plane_2", "hash_s", "hash_d", "hash_1", "hash_2", "params")
    for slot, (g, l) in enumerate(zip(grads, leaves + [w64])):
        if slot in (6, 7):
            assert g is None
            continue
        if any(l is m for m in leaves[:slot]):
            continue  # the same leaf as plane_d
        worst[names[slot]] = round(compare_to_bar(f"{case}/{names[slot]}", g, l.grad), 3)
    print(f"tail {case}: rows set aside {n_fragile}, largest |g - g64| / bar: {worst}")
    assert max(worst.values()) <= 1.0


# ---- f. FlowMlpFn ---------------------------------------------------------------------------------------------------------------------------
def _flow_fn(x, w0, w1, w2, go, dev, need_x=True):
    from nvsf.nerf.models.flow_field import FlowMlpFn
    xd = x.to(dev).requires_grad_(need_x)
    ws = [w.to(dev).requires_grad_() for w in (w0, w1, w2)]
    out = FlowMlpFn.apply(xd, *ws)
    out.backward(go.to(dev))
    return out.detach(), xd.grad, [w.grad for w in ws]


def flow_exact_reference(M):
    x, w0, w1, w2, go = flow_integer_case(M)
    xl = x.double().requires_grad_()
    wl = [w.double().requires_grad_() for w in (w0, w1, w2)]
    out = T.flow_mlp(xl, *wl)
    (out * go.double()).sum().backward()
    a1 = torch.relu(x.double() @ w0.double().t())
    a2 = torch.relu(a1 @ w1.double().t())
    g2 = (go.double() @ w2.double()) * (a2 > 0)
    g1 = (g2 @ w1.double()) * (a1 > 0)
    assert max(float(a1.max()), float(a2.max())) <= 2048
    assert representable_after_scale(go.double()) and representable_after_scale(g2) and representable_after_scale(g1)
    for a, g in ((x.double(), g1), (a1, g2), (a2, go.double())):
        assert float((g.abs().t() @ a.abs()).max()) < 2 ** 24
    return (x, w0, w1, w2, go), out.detach(), xl.grad, [w.grad for w in wl]


@pytest.mark.parametrize("kernel", ["wave", "staged"])
@pytest.mark.parametrize("M", M_FLOW)
def test_flow_mlp_fn_exact(dev, variants, M, kernel):
    """Forward and every gradient EQUAL float64 autograd through flow_mlp; g2 comes back as [6, 64] (nothing of the padded rows 6..15
    of the kernels' output layer leaks); x.grad is None when x requires none."""
    variants.set(mlp_bwd=kernel)
    case, out64, gx64, gw64 = flow_exact_reference(M)
    out, gx, gw = _flow_fn(*case, dev)
    assert out.shape == (M, 6) and torch.equal(out.double().cpu(), out64)
    assert torch.equal(gx.double().cpu(), gx64)
    for g, g64, shape in zip(gw, gw64, ((64, 32), (64, 64), (6, 64))):
        assert tuple(g.shape) == shape and g.is_contiguous() and torch.equal(g.double().cpu(), g64)
    out2, gx2, gw2 = _flow_fn(*case, dev, need_x=False)
    assert gx2 is None and torch.equal(out2, out) and all(torch.equal(a, b) for a, b in zip(gw2, gw))


@pytest.mark.parametrize("case", list(FLOW_RANDOM_CASES))
def test_flow_mlp_fn_random_against_fp64(dev, case):
    """Random Linear weights and Lagrange-reduced-scale inputs against flow_mlp in float64: the bar and the fragile-row rule of the
    test above, incoming gradients at x 64 (what a loss scaler supplies) and x 2^-10."""
    M, seed, g_scale = FLOW_RANDOM_CASES[case]
    x, w0, w1, w2, go, n_fragile = flow_random_case(M, seed, g_scale)
    assert n_fragile <= MAX_FRAGILE
    xl = x.double().requires_grad_()
    wl = [w.double().requires_grad_() for w in (w0, w1, w2)]
    out64 = T.flow_mlp(xl, *wl)
    (out64 * go.double()).sum().backward()
    out, gx, gw = _flow_fn(x, w0, w1, w2, go, dev)
    scale = float(out64.detach().abs().max())
    err = (out.double().cpu() - out64.detach()).abs()
    assert float(err.max()) <= 1e-3 * scale
    if M >= 100:
        assert float((err <= 2e-6 * scale).double().mean()) > 0.97
    worst = {"x": round(compare_to_bar(f"{case}/x", gx, xl.grad), 3)}
    for i, (g, l) in enumerate(zip(gw, wl)):
        assert g.shape == l.shape
        worst[f"w{i}"] = round(compare_to_bar(f"{case}/w{i}", g, l.grad), 3)
    print(f"flow {case}: rows set aside {n_fragile}, largest |g - g64| / bar: {worst}")
