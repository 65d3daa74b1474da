"""torch.ops.texbias.kspace_spikes / kspace_spikes_grad and LearnedSpikeLayer without a device: fake-tensor
shapes on meta tensors, every argument error raised in Python before the library is touched, and the layer's
location draws."""
import numpy as np
import pytest
import torch

import texbias.ops  # noqa: F401 - registers torch.ops.texbias.*
from texbias import runtime as rt
from texbias._abi import TB_MAX_OPS
from texbias.spikes import LearnedSpikeLayer

OP = torch.ops.texbias.kspace_spikes
GRAD = torch.ops.texbias.kspace_spikes_grad


def test_fake_shapes_of_the_forward():
    x = torch.empty((2, 3, 24, 20, 15), device="meta")
    logi = torch.empty((2,), device="meta")
    y, coef = OP(x, logi, [1, 2, 3, 12, 10, 7], 3, 3, 5)
    assert tuple(y.shape) == (2, 3, 24, 20, 20) and y.dtype == torch.float32
    assert tuple(coef.shape) == (2, 3, 2, 2) and coef.dtype == torch.float64
    # four transformed axes, a singleton leading one (the reference's call of the layer)
    y, coef = OP(torch.empty((2, 1, 1, 16, 12, 10), device="meta"), logi[:1], [0, 3, 4, 5], 4, 1)
    assert tuple(y.shape) == (2, 1, 1, 16, 12, 10) and tuple(coef.shape) == (2, 1, 1, 2)


def test_fake_shapes_of_the_gradient():
    g = torch.empty((2, 3, 24, 20, 20), device="meta")[..., :15]
    coef = torch.empty((2, 3, 2, 2), dtype=torch.float64, device="meta")
    logi = torch.empty((2,), device="meta")
    gx, dI = GRAD(g, coef, logi, [1, 2, 3, 12, 10, 7], 3, 3, True)
    assert tuple(gx.shape) == (2, 3, 24, 20, 15) and gx.dtype == torch.float32
    assert tuple(dI.shape) == (2,) and dI.dtype == torch.float32
    gx, dI = GRAD(g, coef, logi, [1, 2, 3, 12, 10, 7], 3, 3, False)
    assert gx.numel() == 0 and tuple(dI.shape) == (2,)
    gx, dI = GRAD(g, coef, logi, [1, 2, 3, 12, 10, 7], 3, 3, True, False)
    assert tuple(gx.shape) == (2, 3, 24, 20, 15) and dI.numel() == 0


X = torch.zeros((2, 3, 8, 6, 5))
ERRORS = [
    ("index_high", IndexError, dict(loc=[1, 2, 5])),
    ("index_negative", IndexError, dict(loc=[-1, 2, 3])),
    ("equal", ValueError, dict(loc=[1, 2, 3, 1, 2, 3], S=2)),
    ("conjugate", ValueError, dict(loc=[5, 4, 3, 3, 2, 1], S=2)),        # k = (1, 1, 1) and (-1, -1, -1)
    ("nyquist_twice", ValueError, dict(loc=[0, 0, 2, 0, 0, 2], S=2)),
    ("too_many", ValueError, dict(loc=[v for j in range(TB_MAX_OPS + 1) for v in (j, 0, 0)], S=TB_MAX_OPS + 1)),
    ("none", ValueError, dict(loc=[])),
    ("ragged", ValueError, dict(loc=[1, 2, 3, 4])),
    ("intensity_shape", ValueError, dict(loc=[1, 2, 3], logi=torch.zeros(2))),
    ("intensity_scalar", ValueError, dict(loc=[1, 2, 3], logi=torch.zeros(()))),
    ("intensity_dtype", ValueError, dict(loc=[1, 2, 3], logi=torch.zeros(1, dtype=torch.float64))),
]


@pytest.mark.parametrize("name,exc,kw", ERRORS, ids=[e[0] for e in ERRORS])
def test_argument_errors_are_raised_without_a_device(name, exc, kw):
    logi = kw.get("logi", torch.zeros(kw.get("S", 1)))
    with pytest.raises(exc):
        OP(X, logi, kw["loc"], 3, 3, 0)
    coef = torch.zeros((2, 3, max(int(logi.numel()), 1), 2), dtype=torch.float64)
    with pytest.raises(exc):
        GRAD(X, coef, logi, kw["loc"], 3, 3, True)


def test_valid_arguments_reach_the_device_check():
    # the last check: a CPU tensor is refused by the launcher, not computed some other way
    with pytest.raises(rt.TexbiasError):
        OP(X, torch.zeros(1), [1, 2, 3], 3, 3, 0)
    with pytest.raises(ValueError):   # a coef of the wrong shape, before the device is asked for
        GRAD(X, torch.zeros((2, 3, 2, 2), dtype=torch.float64), torch.zeros(1), [1, 2, 3], 3, 3, True)


def test_spike_locations_are_the_unshifted_hwd_frequencies():
    assert rt.spike_locations("t", [4, 3, 2, 0, 0, 0], (8, 6, 5)) == [(0, 0, 0), (4, 3, 3)]
    # singleton axes are squeezed as the plans squeeze them
    assert rt.spike_locations("t", [0, 5, 4, 3], (1, 8, 6, 5)) == [(1, 1, 1)]
    assert rt.spike_locations("t", [5, 3], (8, 6)) == [(1, 0, 0)]


def test_layer_registers_its_parameters():
    layer = LearnedSpikeLayer(12.0, n_spikes=3, seed=0)
    params = dict(layer.named_parameters())
    assert list(params) == ["log_intensity"]
    p = params["log_intensity"]
    assert tuple(p.shape) == (3,) and p.dtype == torch.float32 and p.requires_grad
    assert torch.equal(p.detach(), torch.full((3,), 12.0))
    assert tuple(LearnedSpikeLayer().log_intensity.shape) == (1,)
    assert torch.equal(LearnedSpikeLayer([6.0, 7.0], 2).log_intensity.detach(), torch.tensor([6.0, 7.0]))
    with pytest.raises(ValueError):
        LearnedSpikeLayer(1.0, n_spikes=0)
    with pytest.raises(ValueError):
        LearnedSpikeLayer(1.0, n_spikes=TB_MAX_OPS + 1)
    with pytest.raises(ValueError):
        LearnedSpikeLayer([1.0, 2.0, 3.0], n_spikes=2)


def test_layer_draws_non_touching_locations_and_replays_from_its_seed():
    spatial = (4, 3, 4)       # 48 bins, 6 spikes: redraws happen
    layer = LearnedSpikeLayer(10.0, n_spikes=6, seed=123)
    first = [layer.draw(spatial) for _ in range(50)]
    for locs in first:
        assert len(locs) == 6 and all(0 <= v < n for l in locs for v, n in zip(l, spatial))
        rt.spike_locations("draw", [v for l in locs for v in l], spatial)    # raises if two touch
    layer.set_rand_state(123)
    assert [layer.draw(spatial) for _ in range(50)] == first
    again = LearnedSpikeLayer(10.0, 6, seed=123)
    assert [again.draw(spatial) for _ in range(50)] == first
    # the first spike is numpy's own stream: randint(0, n) per axis
    r = np.random.RandomState(123)
    assert first[0][0] == tuple(int(r.randint(0, n)) for n in spatial)
    with pytest.raises(ValueError):
        LearnedSpikeLayer(10.0, n_spikes=3, seed=0).draw((1, 1, 2))   # two bins, both self-conjugate


def test_layer_checks_arguments_before_the_device():
    layer = LearnedSpikeLayer(10.0, n_spikes=2)
    x = torch.zeros((2, 1, 8, 6, 5))
    with pytest.raises(IndexError):
        layer(x, loc=[(1, 2, 3), (8, 0, 0)])
    with pytest.raises(ValueError):
        layer(x, loc=[(1, 2, 3), (1, 2, 3)])
    with pytest.raises(ValueError):
        layer(x, loc=[(1, 2, 3)])
    with pytest.raises(rt.TexbiasError):
        layer(x, loc=[(1, 2, 3), (0, 0, 0)])
    assert layer.last_loc is None


def test_as_transform_holds_the_trained_intensities():
    layer = LearnedSpikeLayer([6.5, 7.25], n_spikes=2)
    t = layer.as_transform([(1, 2, 3), (0, 0, 0)])
    assert type(t).__name__ == "KSpaceSpikeNoise"
    assert list(t.loc) == [(1, 2, 3), (0, 0, 0)] and list(t.k_intensity) == [6.5, 7.25]
    with pytest.raises(ValueError):
        layer.as_transform()
