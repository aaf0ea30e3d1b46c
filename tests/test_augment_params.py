"""Host side of 3dunetcnn_amd.augment (no device): what HipAugmenter accepts, and what sample_params draws and composes."""
import importlib
import json
import math
import os

import pytest
import torch

aug = importlib.import_module("3dunetcnn_amd.augment")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SPATIAL = [{"name": "RandFlipD", "spatial_axis": 0, "prob": 0.5}, {"name": "RandFlipD", "spatial_axis": [1, 2], "prob": 0.5},
           {"name": "RandRotateD", "prob": 0.5, "range_x": 0.2, "range_y": [0.0, 0.1], "range_z": 0.2},
           {"name": "RandZoomD", "prob": 0.5, "min_zoom": 0.9, "max_zoom": 1.2}]
INTENSITY = [{"name": "RandScaleIntensityD", "factors": 0.1, "prob": 0.7}, {"name": "RandShiftIntensityD", "offsets": [-0.05, 0.2], "prob": 0.7}]


def _mk(seed, **kw):
    return aug.HipAugmenter(kw.pop("spatial", SPATIAL), kw.pop("intensity", INTENSITY), generator=torch.Generator().manual_seed(seed), **kw)


def test_same_seed_same_parameters():
    a, b, c = _mk(7).sample_params(4, (3, 20, 18, 16)), _mk(7).sample_params(4, (3, 20, 18, 16)), _mk(8).sample_params(4, (3, 20, 18, 16))
    assert torch.equal(a.matrices, b.matrices) and torch.equal(a.gains, b.gains) and torch.equal(a.offsets, b.offsets)
    assert not torch.equal(a.matrices, c.matrices)
    assert a.matrices.shape == (4, 3, 4) and a.matrices.dtype == torch.float32 and a.gains.shape == (4, 3) and a.out_shape == (20, 18, 16)
    assert _mk(7).sample_params(2, (20, 18, 16)).gains.shape == (2, 1)


def test_prob_zero_is_the_identity():
    zero = lambda entries: [dict(e, prob=0.0) for e in entries]
    p = _mk(1, spatial=zero(SPATIAL), intensity=zero(INTENSITY)).sample_params(5, (2, 9, 8, 7))
    assert torch.equal(p.matrices, torch.eye(4)[:3].expand(5, 3, 4)) and p.trivial_intensity
    assert torch.equal(p.gains, torch.ones(5, 2)) and torch.equal(p.offsets, torch.zeros(5, 2)) and p.out_shape == (9, 8, 7)


def test_drawn_values_lie_inside_their_ranges():
    size = (21, 16, 12)
    c = (torch.tensor(size, dtype=torch.float64) - 1) / 2
    rot = _mk(2, spatial=[{"name": "RandRotateD", "prob": 1.0, "range_x": 0.2, "range_y": [0.0, 0.1], "range_z": 0.0}], intensity=[])
    zoom = _mk(3, spatial=[{"name": "RandZoomD", "prob": 1.0, "min_zoom": 0.9, "max_zoom": 1.2}], intensity=[])
    inten = _mk(4, spatial=[], intensity=[dict(INTENSITY[0], prob=1.0), dict(INTENSITY[1], prob=1.0)])
    pr, pz, pi = rot.sample_params(1000, size), zoom.sample_params(1000, size), inten.sample_params(1000, (2, *size))
    seen = set()
    for m in pr.matrices.double():
        a = m[:, :3]                                      # R0(ax) @ R1(ay): a[0, 2] = sin(ay), a[1, 2] = -sin(ax) cos(ay)
        assert torch.allclose(a @ a.T, torch.eye(3, dtype=torch.float64), atol=1e-6)
        assert torch.allclose(a @ c + m[:, 3], c, atol=1e-4)                                  # about the centre
        ay = math.asin(float(a[0, 2]))
        ax = math.asin(float(-a[1, 2]) / math.cos(ay))
        assert -1e-6 <= ay <= 0.1 + 1e-6 and abs(ax) <= 0.2 + 1e-6 and abs(float(a[0, 1])) < 1e-6     # range_z = 0
        seen.add(ax > 0)
    assert seen == {True, False}
    for m in pz.matrices.double():
        f = 1.0 / float(m[0, 0])
        assert 0.9 - 1e-6 <= f <= 1.2 + 1e-6 and torch.allclose(m[:, :3], torch.eye(3, dtype=torch.float64) / f, atol=1e-6)
        assert torch.allclose(m[:, :3] @ c + m[:, 3], c, atol=1e-4)
    u = pi.gains.double() - 1.0                            # v * (1 + u) + shift: gain = 1 + u, offset = shift
    assert float(u.abs().max()) <= 0.1 + 1e-6 and float(u.min()) < -0.05 and float(u.max()) > 0.05
    assert torch.equal(pi.gains[:, 0], pi.gains[:, 1])    # one draw per sample
    assert -0.05 - 1e-6 <= float(pi.offsets.min()) and float(pi.offsets.max()) <= 0.2 + 1e-6 and not pi.trivial_intensity
    cw = _mk(4, spatial=[], intensity=[dict(INTENSITY[0], prob=1.0, channel_wise=True)]).sample_params(50, (2, *size))
    assert not torch.equal(cw.gains[:, 0], cw.gains[:, 1])


def test_flips_and_crops_are_exact_signed_permutations():
    size, roi = (20, 18, 16), (12, 18, 9)
    a = _mk(5, spatial=[{"name": "RandFlipD", "spatial_axis": 0, "prob": 0.5}, {"name": "RandFlipD", "spatial_axis": [1, 2], "prob": 0.5},
                        {"name": "RandFlipD", "spatial_axis": None, "prob": 0.3}], intensity=[], random_crop=roi)
    p = a.sample_params(200, size)
    assert p.out_shape == roi
    kinds = set()
    for m in p.matrices:
        lin, t = m[:, :3], m[:, 3]
        assert torch.equal(lin.abs(), torch.eye(3)) and torch.equal(t, t.round())
        lo, hi = m @ torch.tensor([0.0, 0, 0, 1]), m @ torch.tensor([roi[0] - 1.0, roi[1] - 1.0, roi[2] - 1.0, 1])
        for k in range(3):                                # the window stays inside the volume
            assert 0 <= min(lo[k], hi[k]) and max(lo[k], hi[k]) <= size[k] - 1
        kinds.add(tuple(int(v) for v in lin.diagonal()))
    assert len(kinds) == 4                                # axis 0 and axes (1, 2) flip independently; the all-axes entry composes with them
    assert aug.HipAugmenter(random_crop=(64, 64, 64)).sample_params(1, (20, 18, 16)).out_shape == (20, 18, 16)   # roi clipped to the volume


def test_composition_order_is_the_config_order():
    """rotation then flip differs from flip then rotation; each equals the product of the single maps in the listed order."""
    size = (11, 9, 7)
    rot = {"name": "RandRotateD", "prob": 1.0, "range_x": [0.15, 0.15], "range_y": [0.0, 0.0], "range_z": [-0.1, -0.1]}
    flip = {"name": "RandFlipD", "spatial_axis": 1, "prob": 1.0}
    one = lambda entries: _mk(0, spatial=entries, intensity=[]).sample_params(1, size).matrices[0].double()
    to4 = lambda m: torch.cat([m, torch.tensor([[0.0, 0, 0, 1]], dtype=torch.float64)])
    mr, mf = to4(one([rot])), to4(one([flip]))
    assert torch.allclose(to4(one([rot, flip])), mr @ mf, atol=1e-5) and torch.allclose(to4(one([flip, rot])), mf @ mr, atol=1e-5)
    assert not torch.allclose(mr @ mf, mf @ mr, atol=1e-3)
    assert torch.allclose(mr[:3, :3], aug.rotation(0.15, 0.0, -0.1), atol=1e-6)


def test_sppin_config_block_constructs():
    block = json.load(open(os.path.join(GOLDEN, "sppin_dataset_block.json")))["dataset"]
    a = aug.HipAugmenter.from_config(block, generator=torch.Generator().manual_seed(0))
    assert a.normalize and a.random_crop is None and a.padding == "border"
    assert [n for n, _ in a.spatial] == ["RandFlipD", "RandFlipD", "RandRotateD"]
    assert [n for n, _ in a.intensity] == ["RandScaleIntensityD", "RandShiftIntensityD"]
    p = a.sample_params(2, (4, 192, 192, 192))
    assert p.out_shape == (192, 192, 192) and p.gains.shape == (2, 4) and not p.trivial_intensity
    crop = aug.HipAugmenter.from_config(dict(block, random_crop=True, desired_shape=[96, 96, 96]))
    assert crop.random_crop == (96, 96, 96) and crop.sample_params(1, (4, 192, 192, 192)).out_shape == (96, 96, 96)
    assert not aug.HipAugmenter.from_config(dict(block, normalization=None)).normalize


@pytest.mark.parametrize("kw,offender", [
    (dict(spatial_augmentations=[{"name": "Rand3DElasticD", "prob": 0.1}]), "Rand3DElasticD"),
    (dict(intensity_augmentations=[{"name": "RandGaussianNoiseD", "prob": 0.1}]), "RandGaussianNoiseD"),
    (dict(spatial_augmentations=[{"name": "RandRotateD", "range_x": 0.1, "keep_size": False}]), "keep_size"),
    (dict(spatial_augmentations=[{"name": "RandZoomD", "keep_size": False}]), "keep_size"),
    (dict(spatial_augmentations=[{"name": "RandRotateD", "range_x": 0.1, "padding_mode": "reflection"}]), "reflection"),
    (dict(spatial_augmentations=[{"name": "RandFlipD", "spatial_axis": 0, "lazy": True}]), "lazy"),
    (dict(spatial_augmentations=[{"name": "RandRotateD", "padding_mode": "zeros"}, {"name": "RandRotateD"}]), "padding_mode"),
])
def test_unsupported_entries_raise_at_construction(kw, offender):
    with pytest.raises(NotImplementedError, match=offender):
        aug.HipAugmenter(**kw)


def test_unsupported_normalization_raises():
    with pytest.raises(NotImplementedError, match="nonzero"):
        aug.HipAugmenter.from_config({"normalization": "NormalizeIntensityD", "normalization_kwargs": {"channel_wise": True, "nonzero": True}})
    with pytest.raises(NotImplementedError, match="zero_mean"):
        aug.HipAugmenter.from_config({})               # the reference's default normalises over the whole image, not per channel
