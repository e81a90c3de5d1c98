"""CPU checks of the ray-order measurement (profiles/NOTES.md, Round 10): the committed per-slot wave durations of the LiDAR launch
say what the notes say, and tools/ray_duration_stats.py restates the proposed deal as specified."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ray_duration_stats as R  # noqa: E402


def _load(name="index"):
    return np.load(R.GOLDEN)[name].astype(np.float64)


@pytest.mark.parametrize("rotate", [False, True])
def test_deal_is_a_permutation_with_one_ray_of_every_quarter_per_workgroup(rotate):
    keys = R.keys()
    for key in keys.values():
        order = R.deal(key, rotate)
        assert np.array_equal(np.sort(order), np.arange(R.N))
        quarter = (R.ranks(key)[order] // (R.N // 4)).astype(int).reshape(-1, 4)
        assert (np.sort(quarter, 1) == np.arange(4)).all()
        if rotate:  # the stratum on wave position 0 moves on with the workgroup index
            assert (quarter[:, 0] == (-np.arange(R.N // 4)) % 4).all()
    # ties and exact zeros: every key equal, axis-aligned directions
    assert np.array_equal(np.sort(R.deal(np.zeros(R.N), rotate)), np.arange(R.N))


def test_deal_balances_the_key_sums_of_the_bench_batch():
    """Under the cost model the proposal rested on (a ray's cost = its key) the deal does equalise the workgroups."""
    for key in R.keys().values():
        per_wg = lambda order: key[order].reshape(-1, 4).sum(1)  # noqa: E731
        dealt, index = per_wg(R.deal(key)), per_wg(np.arange(R.N))
        assert dealt.max() / dealt.mean() < index.max() / index.mean()


def test_durations_follow_the_slot_not_the_ray():
    index, rev, dealt = _load(), _load("reversed"), _load("snake")
    keys = R.keys()
    for dur in (index, rev, dealt):
        assert dur.shape == (R.N,)
        med, explained, _ = R.round_split(dur)
        assert explained > 0.95 and med == sorted(med)  # the dispatch round of the workgroup on its compute unit
    for key in keys.values():
        assert abs(R.spearman(key, index)) < 0.1
    # the same ray in the reversed batch takes the time of its new slot
    assert R.spearman(index, rev[::-1]) < -0.8
    # per real compute unit the launch is balanced to a few per cent already, and the deal's measured effect is of that size
    assert R.sums(index)[2] < 1.07 and R.sums(dealt)[2] < R.sums(index)[2]
