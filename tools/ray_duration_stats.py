"""Per-ray wave durations of the one-launch LiDAR render against candidate cost keys (profiles/NOTES.md, Round 10):

    python tools/ray_duration_stats.py [tests/golden/lidar_ray_durations.npz]

Every array of the file (`index`, `reversed`, `snake`) holds, per SLOT (slot = 4 x workgroup + wave) of one launch of k_render_uniform<lidar> on the batch bench.py times
(S.lidar_rays(4096, default_rng(1000)), T = 768), the clock ticks between entry and exit of the slot's wave (experiment build of
tools/build_variant.py: clock64() at both ends; nothing of it is in csrc/).  Which ray a slot rendered follows from the array's name: the
batch in index order, reversed, or dealt (`snake`: the rotated snake deal by (|dy| + |dz|), `deal`).  Workgroup j runs on compute unit
j mod 256 (read from the hardware id register in the same build: XCD j mod 8, every CU takes the workgroups j, j + 256, j + 512, j + 768).

Prints min / median / max, what the dispatch round j div 256 explains of the variance, the rank correlation of the durations with each
key, and max / mean of the durations summed per workgroup, per 16 consecutive slots and per compute unit -- measured, and as the host
restatement "every ray keeps its measured duration" gives it for the snake deal by each key.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "selfsupervised-nvsf_amd"))
from nvsf import synthetic as S  # noqa: E402

N = 4096


def ranks(v):
    r = np.empty(len(v))
    r[np.argsort(v, kind="stable")] = np.arange(len(v))
    return r


def spearman(a, b):
    return float(np.corrcoef(ranks(a), ranks(b))[0, 1])


def deal(key, rotate=True):
    """slot -> ray: workgroup j takes {r_j, r_(N/2-1-j), r_(N/2+j), r_(N-1-j)} of the ranking by `key` (N a multiple of 4); with
    `rotate` the stratum on wave position w moves on by one per workgroup."""
    r = np.argsort(key, kind="stable")
    n, h = len(r), len(r) // 2
    j = np.arange(n // 4)
    q = np.stack([r[j], r[h - 1 - j], r[h + j], r[n - 1 - j]], 1)
    if rotate:
        q = np.stack([np.roll(q[i], i & 3) for i in range(len(q))])
    return q.reshape(-1)


def keys():
    _, d = S.lidar_rays(N, np.random.default_rng(1000))
    a = np.abs(d.astype(np.float64))
    span = (S.LIDAR_MAX_DEPTH - S.MIN_NEAR) / (2.0 * S.BOUND)  # range x inv_extent: one constant for a LiDAR batch
    return {"(|dy|+|dz|) range": (a[:, 1] + a[:, 2]) * span, "L1 (share gate)": a.sum(1) * span}


GOLDEN = os.path.join(ROOT, "tests", "golden", "lidar_ray_durations.npz")


def slot_to_ray(name, k):
    if name == "reversed":
        return np.arange(N)[::-1]
    if name == "snake":
        return deal(k["(|dy|+|dz|) range"])
    return np.arange(N)


def sums(by_slot):
    """max / mean of the durations summed per workgroup, per 16 consecutive slots, per compute unit."""
    wg = by_slot.reshape(-1, 4).sum(1)
    g16 = by_slot.reshape(-1, 16).sum(1)
    cu = wg.reshape(4, 256).sum(0)
    return tuple(float(s.max() / s.mean()) for s in (wg, g16, cu))


def round_split(by_slot):
    """(medians per dispatch round, share of the variance the round explains, residual)."""
    rnd = np.arange(N) // 1024
    mean = np.array([by_slot[rnd == r].mean() for r in range(4)])
    res = by_slot - mean[rnd]
    return [float(np.median(by_slot[rnd == r])) for r in range(4)], float(1.0 - res.var() / by_slot.var()), res


def main():
    k = keys()
    data = np.load(sys.argv[1] if len(sys.argv) > 1 else GOLDEN)
    for path in data.files:
        dur = data[path].astype(np.float64)
        assert dur.shape == (N,)
        ray = slot_to_ray(path, k)
        med, explained, res = round_split(dur)
        print(f"{path}: min {dur.min():.0f}  median {np.median(dur):.0f}  max {dur.max():.0f}  cv {dur.std() / dur.mean():.4f}")
        print(f"  medians of the dispatch rounds {[int(m) for m in med]}; the round explains {explained:.4f} of the variance, residual cv {res.std() / dur.mean():.4f}")
        print(f"  rank corr with the slot {spearman(np.arange(N), dur):+.3f}")
        A = np.stack([np.ones(N), k["(|dy|+|dz|) range"][ray], k["L1 (share gate)"][ray]], 1)
        coef = np.linalg.lstsq(A, dur, rcond=None)[0]
        by_ray = np.empty(N)
        by_ray[ray] = dur
        fit = np.empty(N)
        fit[ray] = A @ coef
        kk = dict(k)
        kk["fit of both"] = fit
        print("  measured order:        per workgroup %.4f  per 16 slots %.4f  per compute unit %.4f" % sums(dur))
        for name, v in kk.items():
            print(f"  {name:20s} rank corr {spearman(v, by_ray):+.3f}, with the residual {spearman(v[ray], res):+.3f};  snake deal of the measured durations: "
                  "per workgroup %.4f  per 16 slots %.4f  per compute unit %.4f" % sums(by_ray[deal(v)]))


if __name__ == "__main__":
    main()
