"""The host arithmetic shared by the space-time density path, checked WITHOUT a device: hash_field.time_slot against the literal fp32
expressions its six callers used to spell out, hash_field.neighbour_frames at the first, a middle and the last frame, and the one packer
of the flow MLP's fp16 weights behind FlowField's cache.  End frames and exact slice times are otherwise reached by GPU tests only."""
import math

import numpy as np
import pytest
import torch

from nvsf.nerf.models.flow_field import FlowField, _pack_flow_weights
from nvsf.nerf.models.hash_field import lagrange_weights_host, neighbour_frames, time_slot


def _slice_times(R):
    """Every exact slice time k / (R - 1), rounded to fp32."""
    return [float(np.float32(k / (R - 1))) for k in range(R)]


def _times(R):
    s = np.float32(_slice_times(R)[R // 2])  # the fp32 neighbours of one slice time, one step down and one step up
    near = [float(np.nextafter(s, np.float32(0))), float(np.nextafter(s, np.float32(1)))]
    return [0.0, 1.0] + _slice_times(R) + [0.5, 0.77, float(np.float32(1) / np.float32(3))] + near


class _DeviceFlag(torch.Tensor):
    """A tensor that reports `is_cuda`: what time_slot decides the division form of the Lagrange weights from."""
    is_cuda = True


def _time_arguments(t_host):
    """(t as the callers pass it, the division form PyTorch uses for it)"""
    fake = torch.Tensor._make_subclass(_DeviceFlag, torch.tensor([[t_host]], dtype=torch.float32))
    assert torch.is_tensor(fake) and fake.is_cuda
    return [(torch.tensor([[t_host]], dtype=torch.float32), False), (torch.tensor(t_host), False), (t_host, False), (fake, True)]


@pytest.mark.parametrize("R", [8, 25])
def test_time_slot_is_the_literal_expressions(R):
    for t_host in _times(R):
        idx = np.float32(t_host) * np.float32(R - 1)
        k1, k2 = int(math.floor(idx)), int(math.ceil(idx))
        b_lo, b_hi = float(np.float32(k2) - idx), float(idx - np.float32(k1))
        for t, reciprocal in _time_arguments(t_host):
            slot = time_slot(t, t_host, R)
            assert (slot.k1, slot.k2) == (k1, k2) and 0 <= k1 <= k2 <= R - 1, t_host
            assert type(slot.idx) is np.float32 and slot.idx == idx
            assert type(slot.b_lo) is float and type(slot.b_hi) is float and slot.b_lo == b_lo and slot.b_hi == b_hi
            assert slot.same is (k1 == k2)
            assert len(slot.lag) == 4 and slot.lag == lagrange_weights_host(t_host, 4, reciprocal), (t_host, reciprocal)
    # the two division forms do differ somewhere on these times (otherwise the flag would test nothing)
    assert any(lagrange_weights_host(v, 4, True) != lagrange_weights_host(v, 4, False) for v in _times(R))


@pytest.mark.parametrize("R", [8, 25])
def test_time_slot_is_one_slice_exactly_at_the_slice_times(R):
    exact = set(_slice_times(R))
    assert len(exact) == R
    for t_host in _times(R):
        slot = time_slot(t_host, t_host, R)
        # (for these R the fp32 product fp32(k / (R - 1)) * (R - 1) is k again, and the fp32 neighbours of a slice time miss it)
        assert slot.same == (t_host in exact), t_host
        if slot.same:
            assert slot.k1 == slot.k2 == _slice_times(R).index(t_host) and (slot.b_lo, slot.b_hi) == (0.0, 0.0), t_host
        else:
            assert slot.k2 == slot.k1 + 1 and slot.b_lo > 0 and slot.b_hi > 0, t_host


def test_neighbour_frames_at_the_ends_and_in_the_middle():
    F = 16
    for frame, present in ((0, (True, False)), (7, (True, True)), (15, (False, True))):
        nb = neighbour_frames(frame, F)
        assert len(nb) == 2 and tuple(n is not None for n in nb) == present
        for n, other, col in zip(nb, (frame + 1, frame - 1), (0, 3)):
            if n is None:
                continue
            t_n, t_n_host, flow_col = n
            assert flow_col == col
            assert type(t_n_host) is float and t_n_host == float(np.float32(other / 16))
            assert t_n.dim() == 0 and t_n.device.type == "cpu" and t_n.dtype == torch.float32 and float(t_n) == t_n_host


def test_flow_weights_have_one_packer_behind_the_cache():
    torch.manual_seed(0)
    field = FlowField(n_levels=8, log2_hashmap_size=6, base_resolution=4, max_resolution=16)
    lin = [m for m in field.mlp if isinstance(m, torch.nn.Linear)]
    assert [tuple(l.weight.shape) for l in lin] == [(64, 16), (64, 64), (6, 64)]
    w16 = field._mlp_weights_f16()
    assert w16.dtype == torch.float16 and w16.shape == (64 * 16 + 64 * 64 + 16 * 64,)
    assert torch.equal(w16, _pack_flow_weights(*[l.weight for l in lin]))
    assert not w16[-10 * 64:].any() and bool(w16[-16 * 64:-10 * 64].any())  # W2's six rows, then ten rows of padding
    key = field._mlp_key
    assert key == tuple((l.weight.data_ptr(), l.weight._version) for l in lin)
    assert field._mlp_weights_f16() is w16 and field._mlp_key == key  # unchanged weights: the cached tensor
    with torch.no_grad():
        lin[1].weight.mul_(2.0)
    again = field._mlp_weights_f16()
    assert field._mlp_key != key and field._mlp_key == tuple((l.weight.data_ptr(), l.weight._version) for l in lin)
    assert again is not w16 and not torch.equal(again, w16)
    assert torch.equal(again, _pack_flow_weights(*[l.weight for l in lin]))
