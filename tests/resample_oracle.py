"""float64 restatement of the hierarchical resampling pass, in numpy, written from the
specification: bins and pdf weights of a coarse row, the inverse-CDF sampler, the sort of the new depths, the stable merge with the
coarse row and its source index, and the clipped positions of the new samples.  No device, no project code."""
import numpy as np

DENOM_FLOOR = float(np.float32(1e-5))


def sample_pdf(bins, weights, u):
    """bins [B, nb] fp32, weights [B, nb - 1] fp32, u [U] or [B, U] fp32 -> float64 [B, U] in the order of u (not rounded)."""
    bins = np.asarray(bins, np.float32)
    B, nb = bins.shape
    w = (np.asarray(weights, np.float32) + np.float32(1e-5)).astype(np.float64)  # the sum in fp32, then promoted
    assert w.shape == (B, nb - 1)
    pdf = w / w.sum(-1, keepdims=True)
    cdf = np.concatenate([np.zeros((B, 1)), np.cumsum(pdf, -1)], -1)
    u = np.asarray(u, np.float32).astype(np.float64)
    u = np.broadcast_to(u, (B, u.shape[-1]))
    b64 = bins.astype(np.float64)
    out = np.empty(u.shape, np.float64)
    for r in range(B):
        inds = np.searchsorted(cdf[r], u[r], side="right")
        below, above = np.maximum(inds - 1, 0), np.minimum(inds, nb - 1)
        denom = cdf[r, above] - cdf[r, below]
        denom = np.where(denom < DENOM_FLOOR, 1.0, denom)
        out[r] = b64[r, below] + (u[r] - cdf[r, below]) / denom * (b64[r, above] - b64[r, below])
    return out


def mid_bins(z_vals):
    z = np.asarray(z_vals, np.float32)
    return (z[:, :-1] + np.float32(0.5) * (z[:, 1:] - z[:, :-1])).astype(np.float32)


def pdf_weights(weights):
    """weights[:, 1 : T-1] with non-finite and negative entries counted as 0."""
    w = np.asarray(weights, np.float32)[:, 1:-1]
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(w) & (w >= 0), w, np.float32(0)).astype(np.float32)


def resample_merge(rays_o, rays_d, aabb, z_vals, weights, u, bound=None):
    """-> dict: mid [N, T-1], z_new [N, U] fp32 sorted, z_new64 (the same before rounding, sorted), z_merged [N, T+U], src int32 [N, T+U]
    (index into cat([coarse, new]); coarse first on equal values), xyz_new [N, U, 3] fp32 (product, then sum, then clip), and, with
    `bound`, x01 = (xyz_new + bound) * (1 / (2 bound)), the unit-cube positions a static field encodes."""
    z = np.asarray(z_vals, np.float32)
    N, T = z.shape
    mid = mid_bins(z)
    s64 = np.sort(sample_pdf(mid, pdf_weights(weights), u), -1)
    z_new = s64.astype(np.float32)  # rounding is monotone: still sorted
    cat = np.concatenate([z, z_new], -1)
    src = np.argsort(cat, -1, kind="stable").astype(np.int32)  # stable: a coarse index is smaller than every new one
    z_merged = np.take_along_axis(cat, src.astype(np.int64), -1)
    o, d, box = (np.asarray(a, np.float32) for a in (rays_o, rays_d, aabb))
    prod = (d[:, None, :] * z_new[:, :, None]).astype(np.float32)
    xyz = np.minimum(np.maximum((o[:, None, :] + prod).astype(np.float32), box[:3]), box[3:]).astype(np.float32)
    out = {"mid": mid, "z_new": z_new, "z_new64": s64, "z_merged": z_merged, "src": src, "xyz_new": xyz}
    if bound is not None:
        out["x01"] = ((xyz + np.float32(bound)) * (np.float32(1.0) / np.float32(2 * bound))).astype(np.float32)  # as the kernels form it
    return out


def ulp_distance(a, b):
    """Distance in units in the last place between two finite fp32 arrays."""
    def key(x):
        i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, np.int64(-2 ** 31) - i, i)
    return np.abs(key(a) - key(b))


def close_or_excused(got, want, bin_width, max_ulp=2, share=1e-4):
    """The rule of the device tests: `got` equals `want` (fp32) within `max_ulp`; at most `share` of the samples may be left out, and
    those lie within one bin width (a float64 sum in another order can flip a bin decision within about 1e-15 of a knot).
    Returns (ok, number left out, largest difference of those in bin widths)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    bad = ulp_distance(got, want) > max_ulp
    n_bad = int(bad.sum())
    width = np.broadcast_to(np.asarray(bin_width, np.float64), got.shape)
    worst = float((np.abs(got.astype(np.float64) - want.astype(np.float64)) / width)[bad].max()) if n_bad else 0.0
    return n_bad <= share * got.size and worst <= 1.0, n_bad, worst


def reference_conditions(got, ref, bin_width):
    """The two conditions against the reference's fp32 samples: (largest difference in bin widths, share beyond 0.01 bin width); the
    tests ask <= 1 and <= 1e-3."""
    diff = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)) / np.broadcast_to(np.asarray(bin_width, np.float64), np.shape(got))
    return float(diff.max()), float((diff > 0.01).mean())
