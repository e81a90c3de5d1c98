"""GPU parity against the COMPILED reference: the reference's own raymarching and chamfer kernels, built for gfx950 by
oracle/build_ref.py into oracle/_ref (loaded through tests/ref_lib.py), and the product's HIP kernels, driven with the same device
tensors.  tests/test_raymarching_gpu.py and tests/test_chamfer_gpu.py compare with C restatements written from the same reading of
the .cu files as the kernels; a misreading shared by both passes there and fails here.

Inputs stay inside the reference's own contract (contiguous fp32 / int32 / uint8 device tensors, output buffers of the sizes its Python
wrappers allocate), so its kernels read and write only what they own.  `_ref_raymarching` and `_ref_chamfer` are built with
-ffp-contract=off (every operation rounded, as the HIP kernels and the oracle); `_ref_raymarching_fmad` with hipcc's default
contraction.  Measured values: DESIGN.md section 3.
"""
import numpy as np
import pytest
import torch

import oracle_lib as O
import ref_lib
from test_raymarching_gpu import _handbuilt_reference, _rays, _t  # helpers only: inputs shared with the oracle tests

pytestmark = pytest.mark.gpu
AABB2 = np.array([-2, -2, -2, 2, 2, 2], np.float32)


@pytest.fixture(scope="module")
def ref(dev):
    return ref_lib.load("_ref_raymarching")


@pytest.fixture(scope="module")
def rm(dev):
    from nvsf.nerf.raymarching import raymarching
    return raymarching


@pytest.fixture(scope="module")
def scene():
    from nvsf import synthetic as S
    grid = S.boxes_density_grid(np.random.default_rng(0), cascades=2, H=128, n_boxes=64)
    return dict(grid=grid, bits=O.packbits(grid, 0.5))


def _bits_equal(a, b):
    """fp32 tensors equal bit for bit (signed zeros told apart)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- near_far_from_aabb, sph_from_ray, morton3D, packbits ---------------------------------------------------------------------------
def _near_far_inputs(n):
    o, d = _rays(n, 1)
    o[: n // 2] = o[: n // 2] * 8.0 + np.random.default_rng(n).uniform(-4, 4, (n // 2, 3)).astype(np.float32)  # half of the origins spread to
    # three times the box (rays that miss, rays that enter from outside), the others at the shared origin inside it
    d[: n // 8, 0] = 0.0                    # axis-parallel rays, 1 / 0 = inf: outside ...
    d[n // 2: n // 2 + n // 8, 1] = 0.0     # ... and inside the box
    if n > 1:                               # origin ON a slab plane with that direction component 0: 0 * inf = NaN
        o[n - 1] = (-2.0, 0.3, 0.1)
        d[n - 1] = (0.0, 0.6, 0.8)
    return o, d


@pytest.mark.parametrize("min_near", [0.05, 3.0])  # 3.0: above the slab entry of most rays that hit
@pytest.mark.parametrize("n", [1, 63, 4096])
def test_near_far_from_aabb(ref, rm, dev, n, min_near):
    o, d = _near_far_inputs(n)
    to, td, ta = _t(o, dev), _t(d, dev), _t(AABB2, dev)
    nr, fr = torch.empty(n, device=dev), torch.empty(n, device=dev)
    ref.near_far_from_aabb(to, td, ta, n, min_near, nr, fr)
    ng, fg = rm.near_far_from_aabb(to, td, ta, min_near)
    nr, fr, ng, fg = (x.cpu().numpy() for x in (nr, fr, ng, fg))
    assert np.array_equal(nr, ng, equal_nan=True) and np.array_equal(fr, fg, equal_nan=True)
    if n == 4096:  # misses, hits from outside, origins inside (near clamped to min_near), and the NaN of 0 * inf
        big = np.finfo(np.float32).max
        assert (nr == big).any() and (nr == np.float32(min_near)).any() and ((nr > np.float32(min_near)) & (nr < big)).any()
        assert np.isnan(nr).any() or np.isnan(fr).any()


def test_near_far_origin_on_a_slab_plane(ref, rm, dev):
    o = np.array([[-2.0, 0.3, 0.1], [2.0, -0.5, 0.0], [0.1, -2.0, 0.2]], np.float32)
    d = np.array([[0.0, 0.6, 0.8], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]], np.float32)
    for k in range(3):  # also as the one-ray batch
        to, td, ta = _t(o[k:k + 1], dev), _t(d[k:k + 1], dev), _t(AABB2, dev)
        nr, fr = torch.empty(1, device=dev), torch.empty(1, device=dev)
        ref.near_far_from_aabb(to, td, ta, 1, 0.05, nr, fr)
        ng, fg = rm.near_far_from_aabb(to, td, ta, 0.05)
        assert np.array_equal(nr.cpu().numpy(), ng.cpu().numpy(), equal_nan=True)
        assert np.array_equal(fr.cpu().numpy(), fg.cpu().numpy(), equal_nan=True)


def test_sph_from_ray(ref, rm, dev):
    """The bar of test_raymarching_gpu.py (2e-6, there device libm against glibc).  Both sides use the device's libm here: measured on an
    MI355X, max |difference| = 0, all 4096 coordinates bit-identical."""
    n = 2048
    o, d = _rays(n, 3)
    to, td = _t(o, dev), _t(d, dev)
    want = torch.empty(n, 2, device=dev)
    ref.sph_from_ray(to, td, 3.0, n, want)
    got = rm.sph_from_ray(to, td, 3.0)
    err = float((got - want).abs().max())
    print(f"sph_from_ray: max |kernel - compiled reference| = {err:.3g}")
    assert torch.isfinite(want).all() and err <= 2e-6


def test_morton3D_and_invert(ref, rm, dev):
    rng = np.random.default_rng(4)
    idx = torch.arange(128, device=dev, dtype=torch.int32)
    cube = torch.stack(torch.meshgrid(idx, idx, idx, indexing="ij"), -1).reshape(-1, 3).contiguous()
    for c in (_t(rng.integers(0, 1024, size=(100000, 3)).astype(np.int32), dev), cube):
        n = c.shape[0]
        want = torch.empty(n, dtype=torch.int32, device=dev)
        ref.morton3D(c, n, want)
        got = rm.morton3D(c)
        assert torch.equal(got, want)
        back = torch.empty(n, 3, dtype=torch.int32, device=dev)
        ref.morton3D_invert(want, n, back)
        assert torch.equal(rm.morton3D_invert(got), back) and torch.equal(back, c)


def test_packbits(ref, rm, dev, scene):
    rng = np.random.default_rng(5)
    g2 = rng.standard_normal((2, 128 ** 3)).astype(np.float32)
    g3 = rng.standard_normal((1, 64 ** 3)).astype(np.float32)
    g3[0, ::5] = np.float32(0.01)       # exactly at the threshold: not occupied (strict >)
    g3[0, 1::7] = -1.0                  # the "never updated" marker of the density grid
    g3[0, 3::11] = np.nan               # a NaN compares false
    g3[0, 4::13] = np.nextafter(np.float32(0.01), np.float32(1.0))
    for grid, thresh in ((scene["grid"], 0.5), (g2, 0.01), (g3, 0.01)):
        tg = _t(grid, dev)
        n = grid.size // 8
        want = torch.empty(n, dtype=torch.uint8, device=dev)
        ref.packbits(tg, n, thresh, want)
        assert torch.equal(rm.packbits(tg, thresh), want)
        assert 0 < int(want.count_nonzero()) < n or grid is g2


# ---- march_rays_train ---------------------------------------------------------------------------------------------------------------
# (entry point, `march` variant).  "wave" is the production selection (variant value 0); it is SET for every entry, because a variant
# left over from the entry before changes what runs: nvsf_march_rays_train falls back to the three-launch form under any other value,
# and nvsf_march_rays_train_ws walks its batches member by member under "serial" (its only variant).
_ENTRIES = (("nvsf_march_rays_train_passes", "wave"), ("nvsf_march_rays_train_passes", "serial"), ("nvsf_march_rays_train_passes", "thread"),
            ("nvsf_march_rays_train_ws", "wave"), ("nvsf_march_rays_train_ws", "serial"), ("nvsf_march_rays_train", "wave"))


def _grid_bits(kind, C, H, scene):
    if kind == "scene":
        assert (C, H) == (2, 128)
        return scene["bits"]
    p = {"random10": 0.1, "random30": 0.3, "random50": 0.5, "dense": 1.0, "empty": 0.0}[kind]
    return np.packbits(np.random.default_rng(11).random(C * H ** 3) < p, bitorder="little")


def _march_buffers(n, M, dev):
    return (torch.zeros(M, 3, device=dev), torch.zeros(M, 3, device=dev), torch.zeros(M, 2, device=dev),
            torch.empty(n, 3, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int32, device=dev))


def _march_reference(mod, dev, to, td, tb, bound, dt_gamma, max_steps, n, C, H, tn, tf, tz):
    M = n * max_steps  # the wrapper's allocation (raymarching.py:226, 235-240): every ray fits
    xyzs, dirs, deltas, rays, counter = _march_buffers(n, M, dev)
    mod.march_rays_train(to, td, tb, float(bound), float(dt_gamma), max_steps, n, C, H, M, tn, tf, xyzs, dirs, deltas, rays, counter, tz)
    torch.cuda.synchronize()
    return counter, rays, xyzs, dirs, deltas


def _march_product(entry, dev, to, td, tb, bound, dt_gamma, max_steps, n, C, H, tn, tf, tz):
    from nvsf import _hip
    M = n * max_steps
    xyzs, dirs, deltas, rays, counter = _march_buffers(n, M, dev)
    extra = ()
    if entry.endswith("_ws"):
        nb = _hip.march_ws_bytes(n)
        ws = torch.empty(nb // 8, dtype=torch.int64, device=dev)
        extra = (_hip.ptr(ws), nb, 0)
    _hip.call(entry, _hip.ptr(to), _hip.ptr(td), _hip.ptr(tb), float(bound), float(dt_gamma), max_steps, n, C, H, M, _hip.ptr(tn), _hip.ptr(tf),
              _hip.ptr(xyzs), _hip.ptr(dirs), _hip.ptr(deltas), _hip.ptr(rays), _hip.ptr(counter), _hip.ptr(tz), *extra)
    torch.cuda.synchronize()
    return counter, rays, xyzs, dirs, deltas


def _per_ray(rays, n, total):
    """rays [n, 3] int32 in any row order -> (offset, count) indexed by ray id; asserts that the ids are a permutation and that the
    non-empty segments tile [0, total) without gap or overlap."""
    r = rays.long()
    r = r[r[:, 0].argsort()]
    assert torch.equal(r[:, 0], torch.arange(n, device=r.device)), "ray ids are not a permutation"
    nz = r[r[:, 2] > 0]
    nz = nz[nz[:, 1].argsort()]
    assert int(nz[:, 2].sum()) == total and torch.equal(nz[:, 1], torch.cumsum(nz[:, 2], 0) - nz[:, 2]), "segments do not tile the samples"
    return r[:, 1], r[:, 2]


def _matched_rows(off_a, off_b, cnt, keep=None):
    """Row indices into a's and b's sample arrays of the samples of the rays in `keep` (default all), ray by ray, sample by sample."""
    c = cnt if keep is None else cnt * keep
    total = int(c.sum())
    within = torch.arange(total, device=cnt.device) - torch.repeat_interleave(torch.cumsum(c, 0) - c, c)
    return torch.repeat_interleave(off_a, c) + within, torch.repeat_interleave(off_b, c) + within


@pytest.mark.parametrize("kind,C,H,bound,n,max_steps,dt_gamma,perturb_seed", [
    ("scene", 2, 128, 2.0, 1000, 256, 1.0 / 128, 7), ("scene", 2, 128, 2.0, 4096, 1024, 0.0, None), ("scene", 2, 128, 2.0, 1, 64, 0.0, None),
    ("scene", 2, 128, 2.0, 7, 33, 0.0, 3), ("random10", 2, 128, 2.0, 1000, 256, 1.0 / 128, 7), ("dense", 2, 128, 2.0, 1000, 256, 1.0 / 128, 7),
    ("empty", 2, 128, 2.0, 1000, 256, 1.0 / 128, 7), ("random30", 1, 128, 1.0, 700, 256, 0.0, 5), ("random30", 1, 128, 1.0, 700, 256, 1.0 / 128, 5)])
def test_march_rays_train(ref, dev, scene, variants, kind, C, H, bound, n, max_steps, dt_gamma, perturb_seed):
    """The reference hands out sample offsets and `rays` rows by atomics in arrival order: its rows are a permutation and its offsets
    differ from the product's ray-index order.  Compared per ray id: the same (ray id, count) pairs, counter == [total, n], and each
    ray's segment of xyzs / dirs / deltas bit for bit, for every product entry point with every variant it has (three-launch form
    with the wave / serial / thread kernels, one-launch form on a caller's scratch block with its batch-parallel and its serial walk,
    reference-shaped entry on its production path: the one-launch kernel on a block of the stream-ordered pool).  The reference gets M = n * max_steps, so
    every ray fits; a too-small M is NOT compared here -- which rays fit depends on the arrival order in the reference -- and stays
    with the oracle tests (test_raymarching_gpu.py: ..._ws_equals_three_launch_form, ..._wrapper_semantics)."""
    o, d = _rays(n, 6, "lidar" if n == 1000 else "cam")
    o *= np.float32(bound / 2.0)  # the synthetic rays are laid out for bound 2
    nears, fars = O.near_far_from_aabb(o, d, np.array([-bound] * 3 + [bound] * 3, np.float32), 0.02)
    noises = np.zeros(n, np.float32) if perturb_seed is None else np.random.default_rng(perturb_seed).random(n).astype(np.float32)
    args = [_t(a, dev) for a in (o, d, _grid_bits(kind, C, H, scene))] + [bound, dt_gamma, max_steps, n, C, H] + [_t(a, dev) for a in (nears, fars, noises)]
    rc, rr, rx, rd, rl = _march_reference(ref, dev, *args)
    total = int(rc[0])
    assert rc.tolist() == [total, n] and (total > 0) == (kind != "empty")
    r_off, r_cnt = _per_ray(rr, n, total)
    for entry, march in _ENTRIES:
        variants.set(march=march)
        oc, orr, ox, od, ol = _march_product(entry, dev, *args)
        assert oc.tolist() == [total, n], (entry, march)
        o_off, o_cnt = _per_ray(orr, n, total)
        assert torch.equal(o_cnt, r_cnt), (entry, march)  # with the permutation check: the same multiset of (ray id, count)
        ia, ib = _matched_rows(r_off, o_off, r_cnt)
        for name, a, b in (("xyzs", rx, ox), ("dirs", rd, od), ("deltas", rl, ol)):
            assert _bits_equal(a[ia], b[ib]), (name, entry, march)


@pytest.mark.parametrize("kind,dt_gamma,perturb_seed", [("scene", 0.0, None), ("random10", 1.0 / 256, 21), ("random50", 0.0, 21)])
def test_march_rays_train_against_the_contracted_build(dev, scene, kind, dt_gamma, perturb_seed):
    """`_ref_raymarching_fmad` (hipcc's default contraction: whatever multiply-adds clang fuses) against the product kernel on the
    4096 x 1024 case (and on two random grids with jitter, on which the oracle pair does differ), next to the CPU oracle pair (liboracle_raymarching.so against its -DORACLE_FMAD build, four hand-placed fmaf
    sites) on the same rays.  Asserted against each other, not against a constant: the fraction of rays whose sample count differs
    may be 4 x the oracle pair's plus 2 rays (clang may contract more sites than the oracle places by hand), and on rays whose
    counts agree the samples differ by no more than the oracle pair's own largest per-sample difference.  DESIGN.md section 3 has
    the two fractions."""
    fm = ref_lib.load("_ref_raymarching_fmad")
    n, max_steps = 4096, 1024
    o, d = _rays(n, 6, "cam")
    nears, fars = O.near_far_from_aabb(o, d, AABB2, 0.02)
    noises = np.zeros(n, np.float32) if perturb_seed is None else np.random.default_rng(perturb_seed).random(n).astype(np.float32)
    bits = _grid_bits(kind, 2, 128, scene)
    args = [_t(a, dev) for a in (o, d, bits)] + [2.0, dt_gamma, max_steps, n, 2, 128] + [_t(a, dev) for a in (nears, fars, noises)]
    fc, fr, fx, _, fl = _march_reference(fm, dev, *args)
    oc, orr, ox, _, ol = _march_product("nvsf_march_rays_train_ws", dev, *args)
    f_off, f_cnt = _per_ray(fr, n, int(fc[0]))
    o_off, o_cnt = _per_ray(orr, n, int(oc[0]))
    M = n * max_steps
    xa, _, la, ra, ca = O.march_rays_train(o, d, bits, 2.0, dt_gamma, max_steps, 2, 128, M, nears, fars, noises)
    xb, _, lb, rb, cb = O.march_rays_train(o, d, bits, 2.0, dt_gamma, max_steps, 2, 128, M, nears, fars, noises, fmad=True)
    assert np.array_equal(ra[:, 2], o_cnt.cpu().numpy())  # the product is the uncontracted oracle, as test_raymarching_gpu.py pins it
    same_gpu = f_cnt == o_cnt
    same_cpu = torch.from_numpy(ra[:, 2] == rb[:, 2]).to(dev)
    diff_gpu, diff_cpu = int((~same_gpu).sum()), int((~same_cpu).sum())
    both = (same_gpu & same_cpu).long()
    ia, ib = _matched_rows(f_off, o_off, o_cnt, both)
    gpu_xyz = float((fx[ia] - ox[ib]).abs().max()); gpu_dl = float((fl[ia] - ol[ib]).abs().max())
    ca_off, cb_off = torch.from_numpy(ra[:, 1].astype(np.int64)).to(dev), torch.from_numpy(rb[:, 1].astype(np.int64)).to(dev)
    ja, jb = _matched_rows(ca_off, cb_off, o_cnt, both)
    ja, jb = ja.cpu().numpy(), jb.cpu().numpy()
    cpu_xyz = float(np.abs(xa[ja] - xb[jb]).max()); cpu_dl = float(np.abs(la[ja] - lb[jb]).max())
    print(f"contraction, 4096 x 1024 {kind} dt_gamma {dt_gamma:g}: rays whose count differs, compiled fmad reference vs kernel {diff_gpu} of {n} ({100.0 * diff_gpu / n:.4f} %), "
          f"oracle pair {diff_cpu} ({100.0 * diff_cpu / n:.4f} %); matched rays, max |dxyz| {gpu_xyz:.3e} vs {cpu_xyz:.3e}, max |ddelta| {gpu_dl:.3e} vs {cpu_dl:.3e}")
    assert diff_gpu <= 4 * diff_cpu + 2
    assert gpu_xyz <= cpu_xyz and gpu_dl <= cpu_dl


# ---- composite_rays_train ----------------------------------------------------------------------------------------------------------
def _deviation_rows(r):
    """Rows on which the product's backward deviates from the reference's formula on purpose: behind a ray's LAST
    live sample, or behind one that leaves no transmittance in fp32, nothing remains -- the kernel uses 0 for the colour behind it
    and T_after for 1 - weights_sum, the reference (forward's total - its own running sum) and 1 - weights_sum, a rounding residue."""
    rows = np.zeros(r["sig"].shape[0], bool)
    for (_, off, cnt), k in zip(r["rays"].tolist(), r["stop"].tolist()):
        if k < 0:
            continue
        rows[off + k] = True
        T_out = np.cumprod(np.exp(-r["sig"][off:off + k + 1].astype(np.float64) * r["dl"][off:off + k + 1, 0]))
        rows[off:off + k + 1] |= T_out < 2.0 ** -126  # zero or denormal in fp32
    return rows


@pytest.mark.parametrize("T_thresh", [1e-4, 0.0, 0.5])
def test_composite_rays_train(ref, rm, dev, T_thresh):
    """Forward and backward on the hand-built rays of test_raymarching_gpu.py::test_composite_rays_train_against_fp64 (counts 0 .. 200
    around the 64-sample rounds, rays that stop exactly at 63 / 64 / 127 / 128, permuted ray ids, a ray that does not fit, padding).
    Forward: 1e-5 abs against the compiled reference, and the kernel no further from fp64 than 4 x the compiled reference is.
    Backward, in the closed form's fp32 units: kernel <= 4 x the compiled reference's own distance from fp64; 2e-5 abs directly
    between the two on every row outside the documented deviation (_deviation_rows: compared with fp64, and the reference's
    residue there -- printed -- held to the size DESIGN.md documents, 1e-7).  Measured on an MI355X (T_thresh 1e-4 / 0 / 0.5): see DESIGN.md section 3."""
    r = _handbuilt_reference(T_thresh)
    M, N = r["sig"].shape[0], r["rays"].shape[0]
    sig, rgb, dl, rays = _t(r["sig"], dev), _t(r["rgb"], dev), _t(r["dl"], dev), _t(r["rays"], dev)
    ws_r, dp_r, img_r = torch.empty(N, device=dev), torch.empty(N, device=dev), torch.empty(N, 3, device=dev)
    ref.composite_rays_train_forward(sig, rgb, dl, rays, M, N, T_thresh, ws_r, dp_r, img_r)
    ts, tc = sig.clone().requires_grad_(), rgb.clone().requires_grad_()
    ws_g, dp_g, img_g = rm.composite_rays_train(ts, tc, dl, rays, T_thresh)
    for name, got, want, f64 in (("weights_sum", ws_g, ws_r, r["ws"]), ("depth", dp_g, dp_r, r["dp"]), ("image", img_g, img_r, r["img"])):
        got, want = got.detach().cpu().numpy().astype(np.float64), want.cpu().numpy().astype(np.float64)
        e_direct, e_k, e_r = float(np.abs(got - want).max()), float(np.abs(got - f64).max()), float(np.abs(want - f64).max())
        print(f"T_thresh {T_thresh} forward {name}: kernel - reference {e_direct:.3g}; from fp64: kernel {e_k:.3g}, reference {e_r:.3g}")
        assert e_direct <= 1e-5 and e_r <= 1e-5 and e_k <= 4.0 * e_r, name
    empty = r["stop"] < 0
    assert empty.any() and not ws_r.cpu().numpy()[r["rays"][empty, 0]].any() and not img_g.detach().cpu().numpy()[r["rays"][empty, 0]].any()
    # backward: each side on its own forward outputs, as its autograd function saves them
    g_ws, g_img = _t(r["g_ws"], dev), _t(r["g_img"], dev)
    gs_r, gc_r = torch.zeros(M, device=dev), torch.zeros(M, 3, device=dev)
    ref.composite_rays_train_backward(g_ws, g_img, sig, rgb, dl, rays, ws_r, img_r, M, N, T_thresh, gs_r, gc_r)
    (ws_g * g_ws).sum().add((img_g * g_img).sum()).add((dp_g * 3.0).sum()).backward()  # the depth gradient is dropped on both sides
    gs_r, gc_r, gs, gc = gs_r.cpu().numpy(), gc_r.cpu().numpy(), ts.grad.cpu().numpy(), tc.grad.cpu().numpy()
    live, dev_rows = r["live"], _deviation_rows(r)
    assert dev_rows.any() and (live & ~dev_rows).any() and not (dev_rows & ~live).any()
    for a in (gs_r, gc_r, gs, gc):
        assert not a[~live].any()
    units = lambda g, g64, unit: np.abs(g - g64) / unit
    ref_s, ref_c = float(units(gs_r, r["gs64"], r["unit_s"])[live].max()), float(units(gc_r, r["gc64"], r["unit_c"])[live].max())
    k_s, k_c = float(units(gs, r["gs64"], r["unit_s"])[live].max()), float(units(gc, r["gc64"], r["unit_c"])[live].max())
    plain = live & ~dev_rows
    d_s, d_c = float(np.abs(gs - gs_r)[plain].max()), float(np.abs(gc - gc_r)[live].max())
    res_direct = float(np.abs(gs - gs_r)[dev_rows].max())
    res_ref, res_k = float(units(gs_r, r["gs64"], r["unit_s"])[dev_rows].max()), float(units(gs, r["gs64"], r["unit_s"])[dev_rows].max())
    print(f"T_thresh {T_thresh} backward, fp32 units from fp64: reference sigma {ref_s:.2f} rgb {ref_c:.2f}, kernel sigma {k_s:.2f} rgb {k_c:.2f}; "
          f"kernel - reference: sigma {d_s:.3g} on {int(plain.sum())} plain rows, rgb {d_c:.3g}; {int(dev_rows.sum())} deviation rows: "
          f"kernel - reference {res_direct:.3g}, from fp64 in units reference {res_ref:.2f} kernel {res_k:.2f}")
    assert k_s <= 4.0 * ref_s and k_c <= 4.0 * ref_c
    assert d_s <= 2e-5 and d_c <= 2e-5
    # the documented size of the deviation (measured 9.3e-9): the reference's residue is (1 - weights_sum) - T_after,
    # a few roundings of sums of at most 1 (<= 8 x 2^-24 = 4.8e-7), times |g_ws| deltas[:, 0] <= 4 x 0.03 -- below 1e-7
    assert res_direct <= 1e-7, f"deviation rows: kernel - reference {res_direct:.3g}"


# ---- march_rays + composite_rays: the survivor loop --------------------------------------------------------------------------------
@pytest.mark.parametrize("dt_gamma", [0.0, 1.0 / 128])
def test_inference_march_and_composite_loop(ref, rm, dev, scene, dt_gamma):
    """Six iterations of the evaluation loop with n_step = max(min(n // n_alive, 8), 1) as the reference's renderer chooses it, seeded
    noises shared through the C ABI, each side on its own state.  After every iteration: rays_alive, positions, directions and steps
    bit for bit, rays_t exactly, weights_sum / depth / image to 1e-5 (the bars of test_raymarching_gpu.py's loop)."""
    from nvsf import _hip
    n, max_steps, T_thresh = 1500, 256, 1e-2
    o, d = _rays(n, 13)
    nears, fars = O.near_far_from_aabb(o, d, AABB2, 0.02)
    rng = np.random.default_rng(14)
    to, td, tb, tn, tf = (_t(a, dev) for a in (o, d, scene["bits"], nears, fars))
    state = [dict(alive=torch.arange(n, dtype=torch.int32, device=dev), t=tn.clone(), ws=torch.zeros(n, device=dev), dp=torch.zeros(n, device=dev),
                  img=torch.zeros(n, 3, device=dev)) for _ in range(2)]
    sr, sg = state
    steps_seen, worst = set(), dict(ws=0.0, dp=0.0, img=0.0)
    for it in range(6):
        n_alive = int(sr["alive"].shape[0])
        assert n_alive > 0
        n_step = max(min(n // n_alive, 8), 1)
        steps_seen.add(n_step)
        M = n_alive * n_step
        M += 128 - M % 128  # the renderer's align
        noises = _t(rng.random(n_alive).astype(np.float32), dev)
        sig, rgb = _t(rng.random(M).astype(np.float32) * 80.0, dev), _t(rng.random((M, 3)).astype(np.float32), dev)
        xr, dr, lr = torch.zeros(M, 3, device=dev), torch.zeros(M, 3, device=dev), torch.zeros(M, 2, device=dev)
        ref.march_rays(n_alive, n_step, sr["alive"], sr["t"], to, td, 2.0, dt_gamma, max_steps, 2, 128, tb, tn, tf, xr, dr, lr, noises)
        xg, dg, lg = torch.zeros(M, 3, device=dev), torch.zeros(M, 3, device=dev), torch.zeros(M, 2, device=dev)
        _hip.call("nvsf_march_rays", n_alive, n_step, _hip.ptr(sg["alive"]), _hip.ptr(sg["t"]), _hip.ptr(to), _hip.ptr(td), 2.0, float(dt_gamma), max_steps,
                  2, 128, _hip.ptr(tb), _hip.ptr(tn), _hip.ptr(tf), _hip.ptr(xg), _hip.ptr(dg), _hip.ptr(lg), _hip.ptr(noises))
        assert _bits_equal(xg, xr) and _bits_equal(dg, dr) and _bits_equal(lg, lr), it
        assert lr.any()
        ref.composite_rays(n_alive, n_step, T_thresh, sr["alive"], sr["t"], sig, rgb, lr, sr["ws"], sr["dp"], sr["img"])
        rm.composite_rays(n_alive, n_step, sg["alive"], sg["t"], sig, rgb, lg, sg["ws"], sg["dp"], sg["img"], T_thresh)
        assert torch.equal(sg["alive"], sr["alive"]), it
        assert torch.equal(sg["t"], sr["t"]), it
        for k in ("ws", "dp", "img"):
            worst[k] = max(worst[k], float((sg[k] - sr[k]).abs().max()))
            assert worst[k] <= 1e-5, (k, it)
        for s in state:
            s["alive"] = s["alive"][s["alive"] >= 0].contiguous()
    print(f"survivor loop dt_gamma {dt_gamma:g}: {int(sr['alive'].shape[0])} of {n} rays alive after six iterations, n_step {sorted(steps_seen)}; "
          f"max |kernel - reference| weights_sum {worst['ws']:.3g} depth {worst['dp']:.3g} image {worst['img']:.3g}")
    assert int(sr["alive"].shape[0]) < n and len(steps_seen) > 1  # rays died and n_step grew


# ---- chamfer -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,n,m", [(1, 4096, 4096), (2, 1000, 37), (3, 5, 3000), (1, 1, 1), (1, 511, 513), (2, 513, 511), (1, 512, 512)])
def test_chamfer_forward_backward(dev, B, n, m):
    """Indices equal -- the tie-break pinned to the reference's own, not to the oracle's reading of it -- and distances bit for bit;
    the gradients to the bar of test_chamfer_gpu.py (fp32 atomics in arrival order on both sides).  511 / 512 / 513: both sides of
    the 512 points the reference kernel stages per batch."""
    from nvsf.nerf.chamfer3D.dist_chamfer_3D import chamfer_3DDist
    cd = ref_lib.load("_ref_chamfer")
    rng = np.random.default_rng(B * 100 + n)
    a = rng.standard_normal((B, n, 3)).astype(np.float32)
    b = rng.standard_normal((B, m, 3)).astype(np.float32)
    if n > 10 and m > 10:
        b[:, 5] = b[:, 3]  # duplicated target ...
        a[:, 7] = b[:, 5]  # ... and an exact hit on it
        if m > 520:
            b[:, 517] = b[:, 3]  # the same point again in the next staged batch
    ta, tb = _t(a, dev), _t(b, dev)
    d1, d2 = torch.zeros(B, n, device=dev), torch.zeros(B, m, device=dev)
    i1, i2 = torch.zeros(B, n, dtype=torch.int32, device=dev), torch.zeros(B, m, dtype=torch.int32, device=dev)
    cd.forward(ta, tb, d1, d2, i1, i2)
    pa, pb = ta.clone().requires_grad_(), tb.clone().requires_grad_()
    gd1, gd2, gi1, gi2 = chamfer_3DDist()(pa, pb)
    assert torch.equal(gi1.int(), i1) and torch.equal(gi2.int(), i2)
    assert _bits_equal(gd1.detach(), d1) and _bits_equal(gd2.detach(), d2)
    if n > 10 and m > 10:
        assert (i1[:, 7] == 3).all() and (d1[:, 7] == 0).all()
    g1, g2 = _t(rng.standard_normal((B, n)).astype(np.float32), dev), _t(rng.standard_normal((B, m)).astype(np.float32), dev)
    ga, gb = torch.zeros_like(ta), torch.zeros_like(tb)
    cd.backward(ta, tb, ga, gb, g1, g2, i1, i2)
    ((gd1 * g1).sum() + (gd2 * g2).sum()).backward()
    print(f"chamfer backward ({B}, {n}, {m}): max |kernel - reference| {float((pa.grad - ga).abs().max()):.3g} / {float((pb.grad - gb).abs().max()):.3g}, "
          f"largest entry {float(ga.abs().max()):.3g} / {float(gb.abs().max()):.3g}")
    np.testing.assert_allclose(pa.grad.cpu().numpy(), ga.cpu().numpy(), atol=2e-5, rtol=5e-5)
    np.testing.assert_allclose(pb.grad.cpu().numpy(), gb.cpu().numpy(), atol=2e-5, rtol=5e-5)
